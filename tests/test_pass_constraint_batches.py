"""The batched contact-row loop of the whole-pass kernel's fused constraint stage -- the (active contact, dof) items of four 32-lane trips formed first, then the contacts' table
entries (condim, roots, dof-mask bits, friction) of all four requested, then the four trips' arithmetic, block after block -- against the rolled loop it replaces.

The reference is bit for bit and lives in the library: MJH_FUSE_ALL=0 routes the same model through kernels 13 + 14, which keep the rolled loop (the batched form is compiled into
the whole-pass instantiations only).  A forward call and three steps, every real and integer leaf compared with `==`, at a batch of 2 (one lone wave) and of 6.  Every case asserts
that the launch table chose the whole-pass kernel, and reads what it is there for -- active contacts per environment, rows -- off the results.

Cases: the humanoid (27 dofs, 8 pyramidal contacts of 4 rows, 53 rows: two trips of the efc_aref / efc_D row loop) with every environment pressed into the floor (8 active contacts:
7 trips, a full block and a partial one) and with one environment of a wave lifted clear of the floor beside one in contact (no item at all in one half of the wave: the halves
run different trip counts), one and three solver iterations (the <.., 36> and <.., 34> forms), float32; hinge_chain20_flat (20 frictionless contacts of one row, 17 - 20 of them
active: 340 - 400 items, eleven to thirteen trips, more than two blocks -- and more than the eight trips a first form of the loop held in registers; 22 rows: one trip of the row
loop); hinge_chain20 and joint_mix_tree (18 and 30 rows, no contact active: a loop of no trip)."""
import os
import subprocess
import sys
import tempfile

import pytest
import torch

import mujoco_torch_amd as mt
from _cases import F32, F64
from test_pass_loop_batches import CHAIN_OPT, WHOLE_PASS

MODELS = [("humanoid", {"solver": 1}, F64, "floor"), ("humanoid", {"solver": 1}, F64, "lifted"), ("humanoid", {"solver": 1, "iterations": 3}, F64, "lifted"),
          ("humanoid", {"solver": 1}, F32, "floor"), ("humanoid", {"solver": 1}, F32, "lifted"),
          ("hinge_chain20_flat", CHAIN_OPT, F64, ""), ("hinge_chain20_flat", CHAIN_OPT, F32, ""), ("hinge_chain20", CHAIN_OPT, F64, ""), ("joint_mix_tree", CHAIN_OPT, F64, "")]
BATCHES = (2, 6)
CASES = [(xml, ov, dt, pose, B) for xml, ov, dt, pose in MODELS for B in BATCHES]
LIFTED = (1, 4)  # environments lifted clear of the floor: the second half of the first wave, the first half of the third
NSTEPS = 3
BLOCK_TRIPS, LANES = 4, 32  # trips of one block of the contact-row loop; lanes per environment


def case_key(c):
    xml, ov, dt, pose, B = c
    return f"{xml}-{'-'.join(f'{k}{v}' for k, v in ov.items())}-{str(dt)[6:]}{'-' + pose if pose else ''}-B{B}"


def make_case(xml, ov, dt, pose, B):
    """test_pass_loop_batches.make_batch (bent joints, small velocities, controls, applied forces); the humanoid's root height set per pose."""
    from test_pass_loop_batches import make_batch

    mx, d = make_batch(xml, ov, dt, B)
    if pose:
        q = d.qpos.clone()
        z0 = float(mt.make_data(mx).qpos[2])
        q[:, 2] = z0 - 0.3  # feet (and, bent far enough, shins) pressed into the floor however the seeded joints bend
        if pose == "lifted":
            for i in LIFTED:
                if i < B:
                    q[i, 2] = z0 + 1.0
        d = d.replace(qpos=q)
    return mx, d


CHILD = r'''
import sys
sys.path.insert(0, "tests"); sys.path.insert(0, "mujoco-torch_amd"); sys.path.insert(0, "oracle")
import torch, mujoco_torch_amd as mt
from mujoco_torch_amd import native
from _util import REAL_LEAVES, INT_LEAVES
from test_pass_loop_batches import launched_ids
from test_pass_constraint_batches import CASES, NSTEPS, case_key, make_case
out = {}
for c in CASES:
    mx, d = make_case(*c)
    mdev, dg = mx.to("cuda"), d.to("cuda")
    res = {"nv": mx.nv}
    fw = mt.forward(mdev, dg)
    res.update({f"{n}#forward": native.data_field_tensor(fw, n).cpu() for n in REAL_LEAVES + INT_LEAVES})
    for s in range(NSTEPS):
        dg = mt.step(mdev, dg)
        res.update({f"{n}#step{s}": native.data_field_tensor(dg, n).cpu() for n in REAL_LEAVES + INT_LEAVES})
    res["_ids"] = launched_ids(mdev, dg)
    out[case_key(c)] = res
torch.save(out, sys.argv[1])
print("ran")
'''


@pytest.fixture(scope="module")
def both_paths():
    """Every case in one child process per path: [whole-pass kernel, kernels 13 + 14]."""
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


def active_contacts(res, when):
    """Active contacts of every environment at a recorded point: contact_dist - contact_includemargin < 0."""
    return ((res[f"contact_dist#{when}"] - res[f"contact_includemargin#{when}"]) < 0).sum(dim=1)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_key)
def test_constraint_batches_are_bit_identical_to_kernels_13_and_14(case, both_paths):
    """forward and three steps through the whole-pass kernel and through kernels 13 + 14: every leaf equal; the whole-pass kernel really ran on one side and not on the other; the
    active contacts and rows are what the case is there for."""
    xml, ov, dt, pose, B = case
    fused, split = (r[case_key(case)] for r in both_paths)
    nv = fused["nv"]
    assert 16 < nv <= 28, nv
    assert fused["_ids"] == [WHOLE_PASS], fused["_ids"]
    assert WHOLE_PASS not in split["_ids"], split["_ids"]
    whens = ["forward"] + [f"step{s}" for s in range(NSTEPS)]
    nefc = fused["efc_D#forward"].shape[1]
    assert 0 < nefc <= 2 * LANES, nefc
    for w in whens:
        nact = active_contacts(fused, w)
        print(case_key(case), w, "active contacts per environment", nact.tolist(), "rows", nefc)
        if xml == "humanoid":
            assert nefc > LANES, nefc  # two trips of the row loop
            up = [i for i in LIFTED if i < B] if pose == "lifted" else []
            assert all(int(nact[i]) == 0 for i in up) and all(int(nact[i]) > 0 for i in range(B) if i not in up), (w, nact.tolist())
        if xml == "hinge_chain20_flat":
            assert nefc <= LANES and int(nact.min()) * nv > 2 * BLOCK_TRIPS * LANES, (w, nefc, nact.tolist())  # more than two blocks in every environment
        assert not torch.isnan(fused[f"qacc#{w}"]).any(), w
    bad = []
    for n, t in fused.items():
        if n in ("_ids", "nv"):
            continue
        o = split[n]
        if not (torch.equal(t, o) or (t.is_floating_point() and torch.equal(torch.isnan(t), torch.isnan(o)) and torch.equal(torch.nan_to_num(t), torch.nan_to_num(o)))):
            bad.append((n, int((t != o).sum())))
    assert not bad, (case_key(case), bad)


def test_the_models_carry_the_row_and_contact_counts():
    """(No GPU.)  What the cases are chosen for is read off the compiled models: one condim per model, one row per contact for the frictionless chain with more (contact, dof) items
    than two blocks of trips hold, a model within one trip of the row loop and one with two."""
    from _util import load_model

    rows = {}
    for xml, ov in (("humanoid", {"solver": 1}), ("hinge_chain20_flat", CHAIN_OPT), ("hinge_chain20", CHAIN_OPT), ("joint_mix_tree", CHAIN_OPT)):
        mx = load_model(xml, ov, F64)
        per = [int(r) for r in mx.tables.con_rows]
        nefc = int(mx.tables.constraint_sizes[-1])
        assert 16 < mx.nv <= 28 and len(set(per)) == 1 and sum(per) <= LANES and nefc <= 2 * LANES, (xml, mx.nv, per, nefc)
        rows[xml] = (per[0], len(per), nefc)
    assert rows["humanoid"][0] == 4 and LANES < rows["humanoid"][2] <= 2 * LANES, rows
    flat = rows["hinge_chain20_flat"]
    assert flat[0] == 1 and flat[1] * 20 > 2 * BLOCK_TRIPS * LANES and flat[2] <= LANES, rows
    assert rows["hinge_chain20"][2] <= LANES, rows
