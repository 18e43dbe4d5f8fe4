"""tendon / transmission / passive / fwd_velocity / fwd_actuation / fwd_acceleration on the GPU (mujoco_torch_amd/dynamics.py, csrc/mjh_dynamics.h) against the
reference's recordings on EDITED leaves (tests/golden/dynamics/, tools/gen_dynamics_golden.py), against ``forward`` and against themselves.

The bound is the project's own for pre-solver leaves, ``TOL_PRE[dtype]`` (tests/_cases.py: 1e-9 / 2e-4) as ``_util.rel_err`` measures; the generator asserts that the
reference's recorded outputs lie within it of the longdouble evaluation (tests/_dynamics_ref.py, pinned by tests/test_dynamics_host.py).  Nothing is read off the
kernels.  Measured on one MI355X, worst error / bound over the recorded cases: see DESIGN.md section 4."""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import _dynamics_ref as dr
import mujoco_torch_amd as mt
from _cases import TOL_PRE
from _util import load_model, rel_err
from mujoco_torch_amd import _postpass, dynamics, native, smooth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
F64, F32 = torch.float64, torch.float32
OP = dict(tendon="tendon", transmission="transmission", passive="passive", fwd_actuation="actuation", fwd_acceleration="acceleration", fwd_velocity="velocity")
_DEVICE = {}


def device_model(c, compiled=False):
    key = (c.name, compiled)
    if key not in _DEVICE:
        _DEVICE[key] = (c.compiled if compiled else c.model).to(DEV)
    return _DEVICE[key]


def host(t):
    return t.detach().cpu().numpy()


def batches(c, fn):
    """1, 3 and one past the environments of a workgroup (a partly filled last workgroup), the count read from the library's plan."""
    envs = dynamics.plan(OP[fn], c.model, c.dtype)[1]
    return (1, 3, envs + 1)


@pytest.mark.parametrize("name", dr.CASES)
def test_every_function_on_the_recorded_edited_leaves(name):
    """Every function on the recorded (edited) inputs, in batches of 1, 3 and one past a workgroup: each replaced leaf within TOL_PRE of the recording."""
    c = dr.case(name)
    mx, tol = device_model(c), TOL_PRE[c.dtype]
    worst = {}
    for fn in dr.functions(c.V):
        for B in batches(c, fn):
            d = c.data(B, DEV, fn)
            out = getattr(mt, fn)(mx, d)
            for n in dr.writes(c.V, fn):
                got = host(getattr(out, n))
                assert got.shape == tuple(getattr(d, n).shape) and getattr(out, n).dtype == c.dtype, (fn, n)
                for e in range(B):
                    r = rel_err(got[e], c.outs[e % c.nenv][fn][n].reshape(got[e].shape)) / tol
                    print(f"{name} {fn}.{n} B={B} env {e}: error / TOL_PRE {r:.3g}")
                    worst[fn] = max(worst.get(fn, 0.0), r)
    print(f"{name}: worst error / TOL_PRE " + ", ".join(f"{t} {v:.3g}" for t, v in worst.items()))
    assert max(worst.values()) <= 1, worst


@pytest.mark.parametrize("name", dr.CASES)
def test_every_function_reproduces_the_leaves_of_forward(name):
    """On the unedited leaves of ``forward(mx, d)``, every function reproduces ``forward``'s own leaves within TOL_PRE (the compiled model: ``forward`` runs the
    native model's values)."""
    c = dr.case(name)
    mx, tol = device_model(c, compiled=True), TOL_PRE[c.dtype]
    V = dr.model_values(c.compiled)
    f = mt.forward(mx, c.data(c.nenv, DEV))
    worst = 0.0
    for fn in dr.functions(V):
        out = getattr(mt, fn)(mx, f)
        for n in dr.writes(V, fn):
            for e in range(c.nenv):
                r = rel_err(host(getattr(out, n))[e], host(getattr(f, n))[e]) / tol
                print(f"{name} {fn}.{n} env {e}: error / TOL_PRE {r:.3g}")
                worst = max(worst, r)
    assert worst <= 1, worst


@pytest.mark.parametrize("xml,dtype", [("pendula", F64), ("muscle_arm", F64), ("humanoid", F64), ("humanoid", F32)])
def test_the_chain_reproduces_forward_up_to_qacc_smooth(xml, dtype):
    """kinematics -> com_pos -> tendon -> crb -> tendon_armature -> factor_m -> transmission -> fwd_velocity -> fwd_actuation -> fwd_acceleration from ``make_data`` and
    a seeded qpos / qvel / ctrl (act) reproduces ``forward``'s ``qfrc_smooth`` and ``qacc_smooth``, and the leaves on the way, within TOL_PRE."""
    mc = load_model(xml, dtype=dtype)
    mx = mc.to(DEV)
    B, rng = 5, np.random.RandomState(11)
    d = mt.make_data(mc).expand(B).clone()
    d = d.replace(qpos=d.qpos + torch.tensor(0.2 * rng.randn(*d.qpos.shape)), qvel=torch.tensor(0.5 * rng.randn(B, int(mc.nv))),
                  ctrl=torch.tensor(rng.uniform(-0.5, 1.2, (B, int(mc.nu)))), act=torch.tensor(rng.uniform(0, 1, (B, int(mc.na)))))
    d = (d if dtype == F64 else d.to(dtype)).to(DEV)
    f = mt.forward(mx, d)
    s = d
    for fn in (mt.kinematics, mt.com_pos, mt.tendon, mt.crb, mt.tendon_armature, mt.factor_m, mt.transmission, mt.fwd_velocity, mt.fwd_actuation, mt.fwd_acceleration):
        s = fn(mx, s)
    worst = {}
    names = ["actuator_length", "actuator_moment", "actuator_velocity", "qfrc_passive", "qfrc_bias", "act_dot", "actuator_force", "qfrc_actuator", "qfrc_smooth", "qacc_smooth"]
    if int(mc.ntendon) > 0:
        names += ["ten_length", "ten_J", "ten_velocity"]
    if mc.has_gravcomp:
        names += ["qfrc_gravcomp"]
    for n in names:
        for e in range(B):
            worst[n] = max(worst.get(n, 0.0), rel_err(host(getattr(s, n))[e], host(getattr(f, n))[e]) / TOL_PRE[dtype])
    print(f"{xml} {dtype}: the chain against forward, error / TOL_PRE " + ", ".join(f"{n} {v:.3g}" for n, v in worst.items()))
    assert max(worst.values()) <= 1, worst


@pytest.mark.parametrize("name", ["pendula_f64", "humanoid_f32", "swimmer_fluid_f64", "halfcheetah_nospring_f64"])
def test_fwd_velocity_is_the_sequence_bit_for_bit(name):
    c = dr.case(name)
    mx = device_model(c)
    d = c.data(5, DEV, "fwd_velocity")
    got = mt.fwd_velocity(mx, d)
    seq = mt.rne(mx, mt.passive(mx, mt.com_vel(mx, dynamics._velocity_products(mx, d))))
    for n in dr.writes(c.V, "fwd_velocity"):
        assert torch.equal(getattr(got, n), getattr(seq, n)), n
    want = host(d.actuator_moment.reshape(5, c.V["nu"], c.V["nv"]).to(F64) @ d.qvel.to(F64).unsqueeze(-1)).reshape(5, -1)
    assert rel_err(host(got.actuator_velocity).astype(np.float64), want) <= TOL_PRE[c.dtype]


def spread(c, fn, B, seed=3):
    """B different environments for ``fn``: the recorded edited inputs, each perturbed by up to 5 %."""
    d = c.data(B, DEV, fn)
    rng = np.random.RandomState(seed)
    return d.replace(**{n: getattr(d, n) * torch.tensor(1 + 0.05 * rng.uniform(-1, 1, tuple(getattr(d, n).shape)), dtype=c.dtype, device=DEV) for n in dr.reads(c.V, fn)})


@pytest.mark.parametrize("name", ["pendula_f64", "humanoid_f32", "centipede_f64", "dynamics_actuators_f64", "swimmer_fluid_f64"])
def test_an_environment_of_a_batch_equals_itself_alone_and_batch_shapes_agree(name):
    """Lanes, environments per workgroup and LDS follow from the model alone: environment e of 70 is the call on it alone, bit for bit; batch shape (2, 3) is the flat 6."""
    c = dr.case(name)
    mx = device_model(c)
    for fn in dr.functions(c.V):
        d = spread(c, fn, 70)
        full = getattr(mt, fn)(mx, d)
        ws = dr.writes(c.V, fn)
        for n in ws:
            assert torch.isfinite(getattr(full, n)).all(), (fn, n)
        assert any(not torch.equal(getattr(full, n)[:3], getattr(full, n)[3:6]) for n in ws), fn
        for lo, hi in ((0, 1), (7, 8), (33, 34), (69, 70), (0, 3), (64, 67)):
            part = getattr(mt, fn)(mx, d[lo:hi])
            for n in ws:
                assert torch.equal(getattr(part, n), getattr(full, n)[lo:hi]), (fn, n, lo, hi)
        flat = d[:6]
        six = getattr(mt, fn)(mx, flat.replace(**{n: t.reshape((2, 3) + tuple(t.shape[1:])) for n, t in flat.items() if isinstance(t, torch.Tensor)}))
        for n in ws:
            assert tuple(getattr(six, n).shape[:2]) == (2, 3) and torch.equal(getattr(six, n).reshape(getattr(full, n)[:6].shape), getattr(full, n)[:6]), (fn, n)


_CUT_CHILD = r'''
import sys
sys.path.insert(0, "tests"); sys.path.insert(0, "mujoco-torch_amd"); sys.path.insert(0, "oracle")
import torch, mujoco_torch_amd as mt
import _dynamics_ref as dr
res = {}
for name in sys.argv[3:]:
    c = dr.case(name)
    mx = c.model.to("cuda")
    for fn in dr.functions(c.V):
        d = c.data(int(sys.argv[2]), "cuda", fn)
        out = getattr(mt, fn)(mx, d)
        for n in dr.writes(c.V, fn):
            res[f"{name}/{fn}/{n}"] = getattr(out, n).cpu()
torch.save(res, sys.argv[1])
print("ran", len(res))
'''


def test_batches_past_one_launch_are_cut_on_the_host():
    """MJH_MAX_GRID_LOG2=2 (the launch cap tests/test_smooth.py uses) caps a launch at 4 workgroups of at most 16 environments: 70 environments go out in several
    launches with a short last one.  All six kernels must give the bits of the uncut run, in a fresh process each (the library reads the switch once)."""
    names = ["pendula_f64", "dynamics_actuators_f64"]
    with tempfile.TemporaryDirectory() as td:
        res = {}
        for tag, env in (("one", {}), ("cut", {"MJH_MAX_GRID_LOG2": "2"})):
            out = os.path.join(td, tag + ".pt")
            base = {k: v for k, v in os.environ.items() if k != "MJH_MAX_GRID_LOG2"}
            r = subprocess.run([sys.executable, "-c", _CUT_CHILD, out, "70"] + names, cwd=ROOT, env=dict(base, **env), capture_output=True, text=True, timeout=300)
            assert r.returncode == 0 and "ran" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
            res[tag] = torch.load(out)
    assert {k.split("/")[1] for k in res["one"]} == set(dr.FUNCTIONS)
    for k, a in res["one"].items():
        assert a.shape[0] == 70 and torch.isfinite(a).all(), k
        assert torch.equal(a, res["cut"][k]), k


def _want(V, c, fn, n, e=0):
    return np.asarray(dr.FN[fn](V, dict(c.passes[e], **c.ins[e][fn]))[n], dtype=np.float64)


def _edit_case(name, fn, leaf, edit):
    """``fn`` on the case's first recorded environment with the Model as recorded and with ``edit(cpu model)``: the edited result against the restatement's on the
    edited values, and the native model both calls ran on."""
    dev = torch.device("cuda", 0)
    c = dr.case(name)
    mx = device_model(c)
    m2_cpu = edit(c.model)
    assert m2_cpu.tables.uid == c.model.tables.uid  # a value-only edit
    m2 = m2_cpu.to(DEV)
    d = c.data(1, DEV, fn)
    a, b = getattr(mt, fn)(mx, d), getattr(mt, fn)(m2, d)
    V2 = dr.model_values(m2_cpu)
    for n in dr.writes(V2, fn):
        r = rel_err(host(getattr(b, n))[0], _want(V2, c, fn, n)) / TOL_PRE[c.dtype]
        print(f"{name} {fn}.{n} after the edit: error / TOL_PRE {r:.3g}")
        assert r <= 1, (fn, n, r)
    assert not torch.equal(getattr(a, leaf), getattr(b, leaf)), leaf
    assert _postpass.handle(m2, dev, c.dtype) is _postpass.handle(mx, dev, c.dtype)
    return a, b


def test_value_edits_of_the_callers_model_take_effect_on_the_same_native_model():
    _edit_case("humanoid_f64", "passive", "qfrc_passive", lambda m: m.replace(dof_damping=m.dof_damping * 3 + 0.1))

    def gain(m):
        g = m.actuator_gainprm.clone()
        g[2, 0] = g[2, 0] * 2.5
        return m.replace(actuator_gainprm=g)

    a, b = _edit_case("humanoid_f64", "fwd_actuation", "qfrc_actuator", gain)
    assert not torch.equal(a.actuator_force[:, 2], b.actuator_force[:, 2]) and torch.equal(a.actuator_force[:, 3:], b.actuator_force[:, 3:])
    _edit_case("gravcomp_arm_f64", "passive", "qfrc_gravcomp", lambda m: m.replace(opt=m.opt.replace(gravity=torch.tensor([0.5, -1.0, -3.0], dtype=F64))))
    _edit_case("swimmer_fluid_f64", "passive", "qfrc_passive", lambda m: m.replace(opt=m.opt.replace(viscosity=torch.tensor(0.3, dtype=F64))))


@pytest.mark.parametrize("name", ["pendula_f64", "humanoid_f32", "hopper_nograv_noact_f64", "halfcheetah_nospring_f64", "gravcomp_arm_f64"])
def test_only_the_listed_leaves_are_replaced_and_the_input_is_not_written(name):
    c = dr.case(name)
    mx = device_model(c)
    for fn in dr.functions(c.V):
        d = c.data(3, DEV, fn)
        before = {n: t.clone() for n, t in d.items() if isinstance(t, torch.Tensor)}
        out = getattr(mt, fn)(mx, d)
        for n, t in before.items():
            assert torch.equal(getattr(d, n), t), (fn, n)
            if n in dr.writes(c.V, fn):
                assert getattr(out, n) is not getattr(d, n) and (getattr(out, n).data_ptr() != getattr(d, n).data_ptr() or t.numel() == 0), (fn, n)
            else:
                assert getattr(out, n) is getattr(d, n), (fn, n)


def test_the_no_launch_branches_on_the_device():
    c = dr.case("hopper_nograv_noact_f64")
    mx, d = device_model(c), c.data(2, DEV)
    a = mt.fwd_actuation(mx, d)
    assert not a.act_dot.any() and not a.qfrc_actuator.any() and a.actuator_force is d.actuator_force and tuple(a.qfrc_actuator.shape) == (2, c.V["nv"])
    c = dr.case("halfcheetah_nospring_f64")
    mx, d = device_model(c), c.data(2, DEV)
    p = mt.passive(mx, d)
    assert not p.qfrc_passive.any() and not p.qfrc_gravcomp.any() and p.qfrc_passive is not d.qfrc_passive
    c = dr.case("humanoid_f64")
    mx, d = device_model(c), c.data(2, DEV)
    assert mt.tendon(mx, d) is d and mt.passive(mx, d).qfrc_gravcomp is d.qfrc_gravcomp
    e = d[:0]
    for fn in dr.functions(c.V):
        out = getattr(mt, fn)(mx, e)
        for n in dr.writes(c.V, fn):
            assert getattr(out, n).shape[0] == 0, (fn, n)


def test_every_op_is_timed_under_its_id(monkeypatch):
    """One launch per function under kernel id 63 + op; ``fwd_velocity`` is its documented sequence: the products, com_vel, passive, rne."""
    c = dr.case("pendula_f64")
    mx = device_model(c)
    nm = native.get_native_model(mx, torch.device("cuda", 0), F64)
    seen = []

    def recording(real):
        def call(*a, **k):
            real(*a, **k)
            ms, ids = (ctypes.c_float * 16)(), (ctypes.c_int * 16)()
            k_ = nm.lib.mjh_debug_phase_times(ms, ids, 16)
            seen.extend((ids[i], ms[i]) for i in range(k_))
        return call

    monkeypatch.setattr(dynamics, "call", recording(dynamics.call))
    monkeypatch.setattr(smooth, "call", recording(smooth.call))
    want = dict(tendon=[63], transmission=[64], passive=[66], fwd_actuation=[67], fwd_acceleration=[68], fwd_velocity=[65, 61, 66, 62])
    nm.lib.mjh_debug_phase_timing(1)
    try:
        for fn, ids in want.items():
            del seen[:]
            getattr(mt, fn)(mx, c.data(3, DEV, fn))
            assert [i for i, _ in seen] == ids and all(ms > 0 for _, ms in seen), (fn, seen)
    finally:
        nm.lib.mjh_debug_phase_timing(0)
    rw = (ctypes.c_int64 * 2)()
    assert nm.lib.mjh_model_kernel_io(nm.handle, 63, rw) == -2  # (not accounted: include/mjhip.h)
