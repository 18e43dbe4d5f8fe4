"""The primitive narrow phase -- plane-sphere, plane-capsule, sphere-sphere, sphere-capsule and capsule-capsule of ``Env::collision()`` (csrc/mjh_kernels.h) with
``make_frame`` / ``normalize_n`` (csrc/mjh_device.h) -- off the bundled models: the family of tests/_prim_scenes.py (pair counts 1 .. 135 around the 16-, 32- and 64-lane
trips, mixed condims, three parameter sources, exact degenerate arrangements, either side of every switch, near-parallel capsules, max_contact_points with ties) through
``mt.forward(mx, d, stages=0x07)`` against tests/_prim_ref.py on that run's own ``geom_xpos`` / ``geom_xmat``, and the contact leaves of the stage prefix bit for bit
against a full forward, Euler and RK4 steps, the general (frictionloss) phase and the whole-pass kernel.  tests/test_primitive_contacts_host.py ties the yardstick to the
reference's recordings and runs the same rules on the CPU oracle.

No bound is read off a kernel: ``TOL_PRE[dtype]`` by ``_util.rel_err`` per leaf on the rows ``_prim_ref`` keeps; capsule-capsule below ``denom = 1e-2``:
max(TOL_PRE, 4 x the error of the same formulas in numpy in the dtype), the rule of tests/test_pgs.py; 64 eps for the frame properties; everything else is equality.

Measured (one MI355X), worst error as a share of its bound over the rows compared, float64 / float32, and the entry that gave it (dist | pos | frame):
  plane_sphere      3.7e-7 (n15) / 7.2e-4 (n17-first) | 2.9e-7 (n17-first) / 7.3e-4 (n17-first) | 1.1e-7 (n1) / 3.8e-4 (n1)
  plane_capsule     3.9e-7 (n15) / 7.8e-4 (n32-last) | 2.4e-7 (n16-last) / 6.2e-4 (params) | 2.6e-7 (n65-first) / 5.9e-4 (n65-last); the normal is the plane's column, bit for bit
  sphere_sphere     2.5e-7 (n65-first) / 1.4e-3 (side-frame) | 1.8e-7 (n64-last) / 4.4e-4 (n65-first) | 3.3e-7 (n135) / 9.6e-4 (n65-first)
  sphere_capsule    2.7e-7 (n16-last) / 9.1e-4 (n32-last) | 1.8e-7 (n32-last) / 6.5e-4 (n15) | 1.3e-6 (params) / 4.2e-3 (params)
  capsule_capsule   1.2e-6 (side-capsules) / 8.9e-4 (n65-last) | 5.2e-6 (near-parallel-0.01) / 2.2e-2 (near-parallel-0.01) | 1.7e-5 (n65-last) / 4.1e-2 (n65-last)
  ... denom < 1e-2  6.9e-7 (n32-last) / 1.0e-3 (n32-last) | 1.6e-7 (near-parallel-0.0001) / 4.5e-4 (n65-last) | 3.0e-7 (n32-last) / 9.9e-4 (n65-last)
  max_contact_points, the kept distances against the reference's smallest: 4.9e-7 / 1.3e-3 (topk-many); against the uncapped twin: equal
i.e. 1e-16 .. 2e-14 in float64 and 1e-7 .. 8e-6 in float32, absolute on values of order 1.
Contacts left out: none in any entry, either dtype.  Held to either ``d1 < d2`` pick (``_prim_ref.Contacts.against``), float64 / float32: n16-last 5 / 4 of 95, n17-last 1 / 14
of 105, n17-first 1 / 4 of 90, n32-last 7 / 20 of 195, n33-last 8 / 18 of 205, n33-first 4 / 4 of 170, n64-last and topk-many 3 / 28 of 355, n65-last 11 / 40 of 365, n65-first
0 / 8 of 330, n135 24 / 32 of 720, the mixed entries 2 / 2 of 70; float32 only: exact-capsules 4 of 11, side-capsules 9 of 9, near-parallel-0.01 4 of 5; no other entry any.
Kernel ids seen by the instantiation test: 0, 1, 2, 4, 6, 7, 8, 9, 12, 13, 14, 16, 17, 18, 19 -- the stage prefix runs the direct constraint phase (8) behind the kinematics
(0, 1); float32 RK4 at B = 8 the stage kernel (18), at B = 5 kernels 17 / 13, 8, 9 per stage; the frictionloss twin the general phase (7); with nv = 18 under CG, n17-first (18 rows)
runs the fused constraint + solver kernel (14) at B = 5 and the whole-pass kernel (16) at B = 8, n65-first and mixed-pyramidal (66 and 80 rows) kernels 13, 2, 4 at either.
No entry had to be shrunk: the largest (n135: 135 pairs, 144 contacts, nv = 6) is accepted in both dtypes.
"""
import ctypes
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import _prim_scenes as ps
import mujoco_torch_amd as mt
from _prim_scenes import F32, F64
from _util import INT_LEAVES, REAL_LEAVES, gpu_out_to_numpy, leaf
from mujoco_torch_amd import native

pytestmark = pytest.mark.gpu

DEV = "cuda"
STAGES_COLLISION = 0x07  # kinematics, com_pos / crb prefix, collision
CONTACT_LEAVES = [n for n in REAL_LEAVES + INT_LEAVES if n.startswith("contact_")]
WORST = {}    # (pair function, leaf, dtype) -> (error / bound, entry)
LEFT = {}     # (entry, dtype) -> contacts left out
KERNELS = {}  # what ran -> kernel ids


def tag(dtype):
    return "f64" if dtype == F64 else "f32"


@functools.lru_cache(maxsize=None)
def on_device(name, dtype, dummies=0, floss=False, uncapped=False, option=()):
    mx, d = ps.placed(name, dtype, dummies, floss, uncapped, **dict(option))
    return mx, mx.to(DEV), d.to(DEV)


def poisoned(d):
    """The Data with NaN in the three leaves the narrow phase writes (``replace`` gives fresh leaves): a slot that comes back finite was written."""
    nan = lambda t: torch.full_like(t, float("nan"))
    return d.replace(contact=d.contact.replace(dist=nan(d.contact.dist), pos=nan(d.contact.pos), frame=nan(d.contact.frame)))


def prefix(name, dtype, **kw):
    mx, mdev, d = on_device(name, dtype, **kw)
    return mx, gpu_out_to_numpy(mt.forward(mdev, poisoned(d), stages=STAGES_COLLISION))


def with_kernel_ids(what, fn):
    lib = native.load_library()
    lib.mjh_debug_phase_timing(1)
    try:
        out = fn()
        ms, ids = (ctypes.c_float * 96)(), (ctypes.c_int * 96)()
        n = lib.mjh_debug_phase_times(ms, ids, 96)
        assert n >= 0, lib.mjh_last_error().decode()
        KERNELS[what] = [ids[i] for i in range(n)]
        return out
    finally:
        lib.mjh_debug_phase_timing(0)


def record(name, dtype, share, left):
    for (fn, lf), v in share.items():
        if v > WORST.get((fn, lf, tag(dtype)), (-1.0, ""))[0]:
            WORST[(fn, lf, tag(dtype))] = (v, name)
    LEFT[(name, tag(dtype))] = max(left.values())


# ---- values ---------------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,dtype", ps.CASES, ids=ps.CASE_IDS)
def test_contacts_against_the_reference(name, dtype):
    """Every entry, both dtypes: dist, pos and frame by the rules of ``_prim_scenes.check_values``; the properties at 64 eps; every slot written (the input leaves are NaN);
    the model-constant leaves equal to ``static_contact_params`` through ``pair_dst``; with max_contact_points, the selection against the uncapped twin."""
    e = ps.BY_NAME[name]
    print(f"{name} {tag(dtype)}: {e.why}")
    mx, out = prefix(name, dtype)
    if mx.tables.topk:
        twin, tout = prefix(name, dtype, uncapped=True)
        C, share, left = ps.check_values(name, dtype, twin, tout)
        ps.check_properties(dtype, ps.contact_leaves(tout, e.B, ps.slots(twin)), C)
        ps.check_constants(dtype, twin, tout, e.B)
        got = ps.contact_leaves(out, e.B, mx.constraint_sizes_py[3])
        assert all(np.isfinite(got[k]).all() for k in got)
        share[("max_contact_points", "dist")] = ps.check_topk(name, dtype, mx, out, twin, tout)
    else:
        C, share, left = ps.check_values(name, dtype, mx, out)
        ps.check_properties(dtype, ps.contact_leaves(out, e.B, ps.slots(mx)), C)
        ps.check_constants(dtype, mx, out, e.B)
    record(name, dtype, share, left)


# ---- the instantiations ---------------------------------------------------------------------------------------------------------------------------------------------

def contact_leaves_of(d):
    return {n: leaf(d, n).detach().cpu() for n in CONTACT_LEAVES}


def assert_same_contacts(what, got, want, rows=slice(None), address_shift=0):
    for n in CONTACT_LEAVES:
        g, w = got[n], want[n][rows]
        if n == "contact_efc_address":
            g = g - address_shift
        assert g.shape == w.shape and torch.equal(g, w), (what, n)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", ps.INSTANTIATION_ENTRIES)
def test_contact_leaves_are_the_same_in_every_instantiation(name, dtype):
    """From one qpos, the contact leaves of (a) the stage prefix are, bit for bit, those of (b) a full forward, (c) an Euler step, (d) an RK4 step at B = 8 and at B = 5 (the
    stage kernel serves multiples of four only), (e) the scene with one frictionloss dof added (the general phase; its efc addresses are one row on) and (g) the scene with
    two more free bodies under CG (nv = 18), at B = 5 (the fused constraint + solver kernel) and B = 8 (the whole-pass kernel, which serves even batches of models
    of at most 32 contact rows: the geom frames arrive through registers).  (f): float32 takes the direct phase."""
    t = f"{name} {tag(dtype)}"
    mx, mdev, d = on_device(name, dtype)
    a = contact_leaves_of(with_kernel_ids(t + " prefix", lambda: mt.forward(mdev, poisoned(d), stages=STAGES_COLLISION)))
    assert all(torch.isfinite(v).all() for v in a.values() if v.is_floating_point())
    assert_same_contacts("forward", contact_leaves_of(with_kernel_ids(t + " forward", lambda: mt.forward(mdev, poisoned(d)))), a)
    assert_same_contacts("euler", contact_leaves_of(with_kernel_ids(t + " step euler", lambda: mt.step(mdev, poisoned(d)))), a)
    _, mrk, drk = on_device(name, dtype, option=(("integrator", "RK4"),))
    assert_same_contacts("rk4 B=5", contact_leaves_of(with_kernel_ids(t + " step rk4 B=5", lambda: mt.step(mrk, poisoned(drk)))), a)
    d8 = torch.cat([drk, drk[:3]])
    rk8 = contact_leaves_of(with_kernel_ids(t + " step rk4 B=8", lambda: mt.step(mrk, poisoned(d8))))
    assert_same_contacts("rk4 B=8", {n: v[:5] for n, v in rk8.items()}, a)
    assert_same_contacts("rk4 B=8, the repeated environments", {n: v[5:] for n, v in rk8.items()}, a, slice(0, 3))
    mfl, mfdev, dfl = on_device(name, dtype, floss=True)
    assert mfl.constraint_sizes_py[1] == 1
    assert_same_contacts("frictionloss", contact_leaves_of(with_kernel_ids(t + " forward, frictionloss", lambda: mt.forward(mfdev, poisoned(dfl)))), a, address_shift=1)
    mbig, mbdev, dbig = on_device(name, dtype, dummies=2, option=(("solver", "CG"),))
    assert mbig.nv == mx.nv + 12
    assert_same_contacts("nv + 12, CG", contact_leaves_of(with_kernel_ids(t + " step euler CG, nv + 12, B=5", lambda: mt.step(mbdev, poisoned(dbig)))), a)
    big8 = contact_leaves_of(with_kernel_ids(t + " step euler CG, nv + 12, B=8", lambda: mt.step(mbdev, poisoned(torch.cat([dbig, dbig[:3]])))))
    assert_same_contacts("nv + 12, CG, B=8", {n: v[:5] for n, v in big8.items()}, a)
    assert_same_contacts("nv + 12, CG, B=8, the repeated environments", {n: v[5:] for n, v in big8.items()}, a, slice(0, 3))
    for k, v in KERNELS.items():
        if k.startswith(t):
            print(f"  {k}: kernels {v}")


def test_the_instantiations_ran():
    """Together the runs above covered the whole-pass kernel (16), the RK4 stage kernel (18) and a separate constraint phase (2, 7 or 8)."""
    if not KERNELS:
        for name in ps.INSTANTIATION_ENTRIES[:1]:
            for dtype in (F64, F32):
                test_contact_leaves_are_the_same_in_every_instantiation(name, dtype)
    seen = sorted({i for v in KERNELS.values() for i in v})
    print(f"kernel ids seen: {seen}")
    assert 16 in seen and 18 in seen and {2, 7, 8} & set(seen), seen
    assert any(7 in v for k, v in KERNELS.items() if "frictionloss" in k)  # the general phase


# ---- RK4's pair cull ------------------------------------------------------------------------------------------------------------------------------------------------

def test_pair_cull_of_rk4_stages_is_invisible_on_a_65_pair_entry():
    """``n65-first`` through ``mt.step`` with RK4 (float32, B = 8: the stage kernel; float64, B = 5) in a fresh child process, against the same with MJH_PAIR_CULL=0: every
    returned leaf ``torch.equal``."""
    code = r'''
import sys
sys.path.insert(0, "tests"); sys.path.insert(0, "mujoco-torch_amd"); sys.path.insert(0, "oracle")
import torch, mujoco_torch_amd as mt
import _prim_scenes as ps
from mujoco_torch_amd import native
from _util import REAL_LEAVES, INT_LEAVES
out = {}
for dt, nb in ((torch.float32, 8), (torch.float64, 5)):
    mx, d = ps.placed("n65-first", dt, integrator="RK4")
    d = torch.cat([d, d[:3]])[:nb]
    got = mt.step(mx.to("cuda"), d.to("cuda"))
    out[str(dt)] = {n: native.data_field_tensor(got, n).cpu() for n in REAL_LEAVES + INT_LEAVES}
torch.save(out, sys.argv[1])
print("ran")
'''
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as td:
        res = []
        for i, env in enumerate(({}, {"MJH_PAIR_CULL": "0"})):
            f = os.path.join(td, f"{i}.pt")
            r = subprocess.run([sys.executable, "-c", code, f], cwd=root, env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
            assert r.returncode == 0 and "ran" in r.stdout, (env, r.stdout[-1500:] + r.stderr[-1500:])
            res.append(torch.load(f))
    for case in res[0]:
        assert torch.isfinite(res[0][case]["contact_dist"]).all()
        for n, t in res[0][case].items():
            o = res[1][case][n]
            assert torch.equal(t, o) or (t.is_floating_point() and torch.equal(torch.nan_to_num(t), torch.nan_to_num(o))), (case, n)


# ---- the report -----------------------------------------------------------------------------------------------------------------------------------------------------

def test_zz_report():
    """Prints what the module's docstring records (run the whole module with -s)."""
    for (fn, lf, dt), (v, name) in sorted(WORST.items()):
        print(f"worst {fn:32s} {lf:7s} {dt}: {v:.3g} of its bound ({name})")
    print("left out per entry:", {k: v for k, v in sorted(LEFT.items()) if v})
    print("kernel ids seen:", sorted({i for v in KERNELS.values() for i in v}))
