"""The launch cutting of the four kernels that run several environments per workgroup (``mjh_postconstraint``, ``mjh_contact_sensors``, ``mjh_energy``,
``mjh_integrate``) on the GPU: one helper of the library's host side cuts a batch into launches for all of them."""
import os
import subprocess
import sys
import tempfile

import pytest
import torch

from _util import load_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CUT_B, CUT_LOG2 = 70, 2
CUT_MODELS = (("humanoid", "float64"), ("sensor_rig2", "float32"))  # contacts under load; a touch, a framelinacc, a jointlimitpos and an e_potential sensor
CUT_DROP = {"sensor_rig2": 0.85}  # its free root starts 0.9 above the floor: lowered until the hull and the sled rest in it
FIVE = ("cacc", "cfrc_int", "cfrc_ext", "subtree_linvel", "subtree_angmom")
STATE = ("qpos", "qvel", "act", "time")

_CUT_CHILD = r'''
import sys
sys.path.insert(0, "tests"); sys.path.insert(0, "mujoco-torch_amd"); sys.path.insert(0, "oracle")
import numpy as np, torch, mujoco_torch_amd as mt
from _util import load_model
B = int(sys.argv[2])
res = {}
for spec in sys.argv[3:]:
    xml, dts, drop = spec.split(":")
    dt = getattr(torch, dts)
    mc = load_model(xml, dtype=dt)
    mx = mc.to("cuda")
    rng = np.random.RandomState(3)
    d = mt.make_data(mc).expand(B).clone()
    qpos = d.qpos + torch.tensor(0.05 * rng.randn(*d.qpos.shape))
    qpos[:, 2] -= float(drop)
    d = d.replace(qpos=qpos, qvel=torch.tensor(0.2 * rng.randn(B, int(mc.nv))), ctrl=torch.tensor(0.3 * rng.randn(B, int(mc.nu))))
    if dt != torch.float64: d = d.to(dt)
    d = mt.forward(mx, d.to("cuda"))
    out = {}
    post = mt.fwd_postconstraint(mx, d)
    for k in ("cacc", "cfrc_int", "cfrc_ext", "subtree_linvel", "subtree_angmom"):
        out[k] = getattr(post, k)
    out["contact_force"] = mt.contact_force(mx, d)
    out["sensordata"] = mt.sensor_postconstraint(mx, d, all_sensors=True).sensordata
    out["energy"] = mt.energy(mx, d)
    out["qderiv"] = mt.deriv_smooth_vel(mx, d)
    for tag, fn in (("implicit", mt.implicit), ("euler", mt.euler)):
        nxt, qacc = fn(mx, d, return_qacc=True)
        for k in ("qpos", "qvel", "act", "time"):
            out[tag + "_" + k] = getattr(nxt, k)
        out[tag + "_qacc"] = qacc
    res[spec] = {k: o.cpu() for k, o in out.items()}
torch.save(res, sys.argv[1])
print("ran")
'''


def test_the_models_of_the_cut_test_have_what_it_exercises():
    """Between them the two models have contacts, a touch and a frame-acceleration sensor, and a limit and an
    energy sensor; neither has actuator activations, and humanoid has no sensors, so those two outputs are empty."""
    hum, rig = (load_model(x, dtype=getattr(torch, t)) for x, t in CUT_MODELS)
    assert hum.constraint_sizes_py[3] > 0 and rig.constraint_sizes_py[3] > 0
    assert {0, 33} <= {int(r[0]) for r in rig.tables.contact_sensors["rows"]}  # touch, framelinacc
    assert {20, 43} <= {int(r[0]) for r in rig.tables.energy_sensors["rows"]}  # jointlimitpos, e_potential
    assert int(hum.na) == int(rig.na) == 0 and int(hum.nsensordata) == 0 and int(rig.nsensordata) > 0


@pytest.mark.gpu
def test_batches_past_one_launch_are_cut_on_the_host():
    """MJH_MAX_GRID_LOG2=2 caps a launch at 4 workgroups.  The four kernels run 256-thread workgroups with at least 16 lanes per environment, so 1 to 16
    environments per workgroup and at most 64 per launch: 70 environments go out in several launches with a short last one, whatever the plan.  The five leaves of
    fwd_postconstraint, contact_force, the sensordata of sensor_postconstraint(all_sensors=True), energy, deriv_smooth_vel and what implicit / euler return must
    be bit-identical to the uncut run, in a fresh process each (the library reads the switch once)."""
    for envs in range(1, 17):
        assert (envs << CUT_LOG2) <= 64 < CUT_B and CUT_B % (envs << CUT_LOG2) != 0, envs
    specs = [f"{x}:{t}:{CUT_DROP.get(x, 0.0)}" for x, t in CUT_MODELS]
    with tempfile.TemporaryDirectory() as td:
        res = {}
        for tag, env in (("one", {}), ("cut", {"MJH_MAX_GRID_LOG2": str(CUT_LOG2)})):
            out = os.path.join(td, tag + ".pt")
            base = {k: v for k, v in os.environ.items() if k != "MJH_MAX_GRID_LOG2"}
            r = subprocess.run([sys.executable, "-c", _CUT_CHILD, out, str(CUT_B)] + specs, cwd=ROOT, env=dict(base, **env), capture_output=True, text=True,
                               timeout=600)
            assert r.returncode == 0 and "ran" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
            res[tag] = torch.load(out)
    assert sorted(res["one"]) == sorted(specs)
    for (xml, _), spec in zip(CUT_MODELS, specs):
        outs = res["one"][spec]
        assert sorted(outs) == sorted(FIVE + ("contact_force", "sensordata", "energy", "qderiv", "implicit_qacc", "euler_qacc")
                                      + tuple(f"{i}_{k}" for i in ("implicit", "euler") for k in STATE))
        empty = {"implicit_act", "euler_act"} | ({"sensordata"} if xml == "humanoid" else set())  # (na == 0; no sensors: the test above)
        for k, a in outs.items():
            assert a.shape[0] == CUT_B and torch.isfinite(a).all(), (spec, k)
            assert (a.numel() == 0) if k in empty else bool(a.any()), (spec, k)
            assert torch.equal(a, res["cut"][spec][k]), (spec, k)
