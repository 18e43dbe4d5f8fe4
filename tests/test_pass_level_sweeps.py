"""The level sweeps of the whole-pass kernel -- kinematics (lane b owns body b, its joints' constants in registers, the levels of the tree in order) and com_vel (the sums of a
body's own joints formed ahead of the sweep, in registers; the sweep itself the additions in joint order) -- against the forms they replace.

The reference is bit for bit and lives in the library: MJH_FUSE_ALL=0 routes the same model through the separate phase kernels, whose kinematics is the serial ancestor walk and
whose com_vel sweep reads every joint's staged products inside the sweep (both whole-pass forms are compiled into the whole-pass instantiations only).  The kinematic leaves and
what is computed from them down to qacc are compared with `==` after a forward call and after each of three steps, at a batch of 2 (one lone wave) and of 6.  Every case asserts
that the launch table chose the whole-pass kernel (even batches, 16 < nv <= 28): otherwise the comparison would be of the phase kernels with themselves.

Models: the humanoid (bodies with one, two and three hinges, depth 7; one and three solver iterations -- the <.., 36> and <.., 34> forms -- and float32); hinge_chain20 (depth 20,
its last two links in contact); mocap_chain (a ball joint at depths 2 and 7, a hinge and a slide in one body, a free body that is the last body, a chain under a mocap body);
joint_mix_tree (bodies with three, four and five joints -- three ride in registers, the rest are read at use -- with slides among them, a ball joint at depth 3, a slide joint in the
body below a hinge and below a ball, two siblings on one level, a mocap body, a free body last).  qpos is seeded off the rest pose (no rotation is the identity), qvel is non-zero."""
import os
import subprocess
import sys
import tempfile

import pytest
import torch

from _cases import F32, F64
from test_pass_loop_batches import CHAIN_OPT, WHOLE_PASS, case_key

MODELS = [("humanoid", {"solver": 1}, F64), ("humanoid", {"solver": 1, "iterations": 3}, F64), ("humanoid", {"solver": 1}, F32),
          ("hinge_chain20", CHAIN_OPT, F64), ("mocap_chain", CHAIN_OPT, F64), ("joint_mix_tree", CHAIN_OPT, F64), ("joint_mix_tree", CHAIN_OPT, F32)]
BATCHES = (2, 6)
CASES = [(xml, ov, dt, B) for xml, ov, dt in MODELS for B in BATCHES]
LEAVES = ["xpos", "xquat", "xmat", "xanchor", "xaxis", "xipos", "ximat", "geom_xpos", "geom_xmat", "site_xpos", "subtree_com", "cdof", "cvel", "cdof_dot", "qfrc_bias", "qacc"]
NSTEPS = 3

CHILD = r'''
import sys
sys.path.insert(0, "tests"); sys.path.insert(0, "mujoco-torch_amd"); sys.path.insert(0, "oracle")
import torch, mujoco_torch_amd as mt
from mujoco_torch_amd import native
from test_pass_loop_batches import case_key, make_batch, launched_ids
from test_pass_level_sweeps import CASES, LEAVES, NSTEPS
out = {}
for c in CASES:
    mx, d = make_batch(*c)
    mdev, dg = mx.to("cuda"), d.to("cuda")
    res = {"nv": mx.nv}
    fw = mt.forward(mdev, dg)
    res.update({f"{n}#forward": native.data_field_tensor(fw, n).cpu() for n in LEAVES})
    for s in range(NSTEPS):
        dg = mt.step(mdev, dg)
        res.update({f"{n}#step{s}": native.data_field_tensor(dg, n).cpu() for n in LEAVES})
    res["_ids"] = launched_ids(mdev, dg)
    out[case_key(c)] = res
torch.save(out, sys.argv[1])
print("ran")
'''


@pytest.fixture(scope="module")
def both_paths():
    """Every case in one child process per path: [whole-pass kernel, separate phase kernels]."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = []
    with tempfile.TemporaryDirectory() as td:
        for i, env in enumerate(({}, {"MJH_FUSE_ALL": "0"})):
            f = os.path.join(td, f"{i}.pt")
            base = {k: v for k, v in os.environ.items() if k != "MJH_FUSE_ALL"}
            r = subprocess.run([sys.executable, "-c", CHILD, f], cwd=root, env=dict(base, **env), capture_output=True, text=True, timeout=300)
            assert r.returncode == 0 and "ran" in r.stdout, (env, r.stdout[-1500:] + r.stderr[-3000:])
            res.append(torch.load(f))
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_key)
def test_level_sweeps_are_bit_identical_to_the_phase_kernels(case, both_paths):
    """forward and three steps through the whole-pass kernel and through the phase kernels: every listed leaf equal; the whole-pass kernel really ran on one side and not on the other."""
    fused, split = (r[case_key(case)] for r in both_paths)
    assert 16 < fused["nv"] <= 28, fused["nv"]
    assert fused["_ids"] == [WHOLE_PASS], fused["_ids"]
    assert WHOLE_PASS not in split["_ids"], split["_ids"]
    names = [f"{n}#{w}" for n in LEAVES for w in ["forward"] + [f"step{s}" for s in range(NSTEPS)]]
    assert set(names) <= set(fused) and set(names) <= set(split)
    bad = [n for n in names if fused[n].numel() == 0 and n.split("#")[0] not in ("site_xpos",)]
    assert not bad, ("empty leaves", bad)
    for n in names:
        t, o = fused[n], split[n]
        assert not torch.isnan(t).any() and not torch.isnan(o).any(), n
        if not torch.equal(t, o):
            bad.append((n, int((t != o).sum())))
    assert not bad, (case_key(case), bad)


def test_the_models_carry_the_joint_arrangements():
    """(No GPU.)  What the cases are chosen for is read off the compiled models, not assumed: depth, joints per body, ball / slide / free placement, a mocap body."""
    import numpy as np

    from _util import load_model

    FREE, BALL, SLIDE, HINGE = 0, 1, 2, 3
    seen = set()
    for xml, ov in (("humanoid", {"solver": 1}), ("hinge_chain20", CHAIN_OPT), ("mocap_chain", CHAIN_OPT), ("joint_mix_tree", CHAIN_OPT)):
        mx = load_model(xml, ov, F64)
        par, jn, ja, jt = (np.asarray(getattr(a, "data", a)).astype(int) for a in (mx.body_parentid, mx.body_jntnum, mx.body_jntadr, mx.jnt_type))
        depth = np.zeros(len(par), dtype=int)
        for b in range(1, len(par)):
            depth[b] = depth[par[b]] + 1
        assert len(par) <= 32 and 16 < mx.nv <= 28, (xml, len(par), mx.nv)
        if depth.max() > 7:
            seen.add("deeper than the humanoid")
        seen.update(f"{n} joints" for n in jn if n >= 3)
        for b in range(1, len(par)):
            types = list(jt[ja[b]:ja[b] + jn[b]])
            if BALL in types and depth[b] > 1:
                seen.add("ball below depth 1")
            if SLIDE in types and HINGE in list(jt[ja[par[b]]:ja[par[b]] + jn[par[b]]]):
                seen.add("slide below a hinge")
            if SLIDE in types[3:]:
                seen.add("slide past the register joints")
            if FREE in types and b > 1:
                seen.add("free body that is not the first")
        if int(mx.nmocap) > 0:
            seen.add("mocap")
    want = {"deeper than the humanoid", "3 joints", "4 joints", "5 joints", "ball below depth 1", "slide below a hinge", "slide past the register joints",
            "free body that is not the first", "mocap"}
    assert want <= seen, want - seen
