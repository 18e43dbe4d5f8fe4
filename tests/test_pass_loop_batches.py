"""The whole-pass kernel's batched loop forms (subtree sums in chunks, the qM pairs' codes and armatures up front, the symmetric row store with an incremental index, the first
trip's table entries of the cinert / cdof / inert_mul / passive / actuation loops requested ahead) against the loops they replace.

The reference is bit for bit and lives in the library: MJH_FUSE_ALL=0 routes the same model through the separate phase kernels, which keep the rolled loops (the batched forms are
compiled into the whole-pass instantiations only).  Two consecutive steps, every real and integer leaf compared exactly.  Shapes at which the chunking can go wrong: the humanoid
(subtree lengths 1 .. 17, 243 qM pairs and 729 qM entries: neither a multiple of 32; one and three solver iterations -- the <.., 36> and <.., 34> forms; float32), a tree under
a mocap body, and a serial chain of 20 hinges whose longest subtree is two chunks of eight and a remainder and whose 210 qM pairs are every (i, j <= i); batches of 2 and 64 (one wave, many waves); seeded non-zero ctrl and qfrc_applied so that the actuation loop carries
values.  Batches of 1 and 3 are stepped too: the launch table gives the whole-pass kernel even batches only (one wavefront per PAIR of environments, no half-filled wave), so an odd
batch runs the phase kernels on both sides of the comparison -- the test says so instead of assuming it (test_which_cases_run_the_whole_pass_kernel)."""
import ctypes
import os
import subprocess
import sys
import tempfile
import zlib

import numpy as np
import pytest
import torch

import mujoco_torch_amd as mt
from _cases import F32, F64, TOL_PRE, seeded_tol_sol
from _util import INT_LEAVES, REAL_LEAVES, check_against_oracle, gpu_out_to_numpy, load_model

pytestmark = pytest.mark.gpu

CHAIN_OPT = {"solver": 1, "iterations": 1, "ls_iterations": 4}  # (the options of the existing switch test's mocap_chain case)
MODELS = [("humanoid", {"solver": 1}, F64), ("humanoid", {"solver": 1, "iterations": 3}, F64), ("mocap_chain", CHAIN_OPT, F64), ("hinge_chain20", CHAIN_OPT, F64), ("humanoid", {"solver": 1}, F32)]
BATCHES = (1, 2, 3, 64)
CASES = [(xml, ov, dt, B) for xml, ov, dt in MODELS for B in BATCHES]
WHOLE_PASS = 16  # timing id of the whole-pass launch (test_launch_sequences_of_the_baseline_workloads)


def case_key(c):
    xml, ov, dt, B = c
    return f"{xml}-{'-'.join(f'{k}{v}' for k, v in ov.items())}-{str(dt)[6:]}-B{B}"


def make_batch(xml, ov, dt, B):
    """Seeded inputs: bent joints, small velocities, controls across the ctrl ranges, applied joint forces."""
    mx = load_model(xml, ov, dt)
    rng = np.random.RandomState(zlib.crc32(xml.encode()) % 1000 + B)
    d = mt.make_data(mx).expand(B).clone()
    d = d.replace(qpos=d.qpos + 0.1 * torch.tensor(rng.randn(B, mx.nq)), qvel=torch.tensor(0.05 * rng.randn(B, mx.nv)),
                  ctrl=torch.tensor(rng.uniform(-1.2, 1.2, size=(B, mx.nu))), qfrc_applied=torch.tensor(0.5 * rng.randn(B, mx.nv)))
    if dt != torch.float64:
        d = d.to(dt)
    return mx, d


def launched_ids(mdev, dg):
    from mujoco_torch_amd import native

    lib = native.load_library()
    lib.mjh_debug_phase_timing(1)
    try:
        mt.step(mdev, dg)
        ms, ids = (ctypes.c_float * 96)(), (ctypes.c_int * 96)()
        n = lib.mjh_debug_phase_times(ms, ids, 96)
        assert n >= 0, lib.mjh_last_error().decode()
        return [ids[i] for i in range(n)]
    finally:
        lib.mjh_debug_phase_timing(0)


CHILD = r'''
import sys
sys.path.insert(0, "tests"); sys.path.insert(0, "mujoco-torch_amd"); sys.path.insert(0, "oracle")
import torch, mujoco_torch_amd as mt
from mujoco_torch_amd import native
from _util import REAL_LEAVES, INT_LEAVES
from test_pass_loop_batches import CASES, case_key, make_batch, launched_ids
out = {}
for c in CASES:
    mx, d = make_batch(*c)
    mdev, dg = mx.to("cuda"), d.to("cuda")
    res = {}
    for s in range(2):
        dg = mt.step(mdev, dg)
        res.update({f"{n}#step{s}": native.data_field_tensor(dg, n).cpu() for n in REAL_LEAVES + INT_LEAVES})
    res["_ids"] = launched_ids(mdev, dg)
    out[case_key(c)] = res
torch.save(out, sys.argv[1])
print("ran")
'''


@pytest.fixture(scope="module")
def both_paths():
    """Every case stepped twice in one child process per path: [whole-pass kernel, separate phase kernels]."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = []
    with tempfile.TemporaryDirectory() as td:
        for i, env in enumerate(({}, {"MJH_FUSE_ALL": "0"})):
            f = os.path.join(td, f"{i}.pt")
            base = {k: v for k, v in os.environ.items() if k != "MJH_FUSE_ALL"}
            r = subprocess.run([sys.executable, "-c", CHILD, f], cwd=root, env=dict(base, **env), capture_output=True, text=True, timeout=600)
            assert r.returncode == 0 and "ran" in r.stdout, (env, r.stdout[-1500:] + r.stderr[-3000:])
            res.append(torch.load(f))
    return res


@pytest.mark.parametrize("case", CASES, ids=case_key)
def test_batched_loops_are_bit_identical_to_the_phase_kernels(case, both_paths):
    """Two steps through the whole-pass kernel and through the phase kernels: every leaf equal (a NaN only where the other path has one)."""
    fused, split = (r[case_key(case)] for r in both_paths)
    assert WHOLE_PASS not in split["_ids"], split["_ids"]
    bad = []
    for n, t in fused.items():
        if n == "_ids":
            continue
        o = split[n]
        if not (torch.equal(t, o) or (t.is_floating_point() and torch.equal(torch.isnan(t), torch.isnan(o)) and torch.equal(torch.nan_to_num(t), torch.nan_to_num(o)))):
            bad.append(n)
    assert not bad, (case_key(case), bad)


@pytest.mark.parametrize("case", CASES, ids=case_key)
def test_which_cases_run_the_whole_pass_kernel(case, both_paths):
    """The launch table selects the whole-pass kernel for every model at every even batch (the chain is short enough for it, its contact rows cover the geom frames they overlay), so
    the comparison above is of the batched forms there; an odd batch is not served by it."""
    ids = both_paths[0][case_key(case)]["_ids"]
    if case[3] % 2 == 0:
        assert ids == [WHOLE_PASS], ids
    else:
        assert WHOLE_PASS not in ids, ids


def test_hinge_chain_matches_the_oracle(oracle_lib):
    """The new chain model against the CPU oracle, at the bounds tests/_cases.py gives the humanoid's float64 cases."""
    xml, ov, dt, B = "hinge_chain20", CHAIN_OPT, F64, 64
    mx, d = make_batch(xml, ov, dt, B)
    mdev, dg = mx.to("cuda"), d.to("cuda")
    for s in range(2):
        og = mt.step(mdev, dg)
        frac, worst = check_against_oracle(mx, dg.cpu(), gpu_out_to_numpy(og), TOL_PRE[dt], seeded_tol_sol("humanoid", {"solver": 1}, dt), what=f"{xml} step{s}", nthreads=4)
        print(f"{xml} step {s}: {frac:.1%} envs on a non-natural line-search branch, worst solver rel err {worst:.2e}")
        dg = og
