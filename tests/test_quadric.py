"""Plane-cylinder / plane-ellipsoid collisions on the GPU (mjh_quadric_kernel, csrc/mjh_quadric.h); tests/test_quadric_host.py is the CPU part.

The CPU oracle does not know the two pair functions, so the yardsticks are the reference's recordings (tests/golden/quadric/*.npz, tools/gen_quadric_golden.py)
and the numpy longdouble restatement tests/_quadric_ref.py, which the CPU part pins against those recordings.
"""
import ctypes

import numpy as np
import pytest
import torch

import mujoco_torch_amd as mt
import pyoracle
from mujoco_torch_amd import native
from _cases import TOL_PRE, TOL_SOL
from _quadric_ref import FN_PLANE_CYLINDER, PAR_EDGE, pair_contacts
from _util import INT_LEAVES, PRE_SOLVER, REAL_LEAVES, SOLVER_LEAVES, Golden, assert_ints_equal, assert_leaves_close, gpu_out_to_numpy, leaf, load_model, rel_err

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64, F32 = torch.float64, torch.float32
CASES = ["quadric/euler_newton_pyr_f64", "quadric/euler_cg_ell_f64", "quadric/rk4_newton_ell_f32", "quadric/topk_f64"]
CONTACT_LEAVES = ("contact_dist", "contact_pos", "contact_frame")
_GOLDEN = {}


def golden(case):
    if case not in _GOLDEN:
        _GOLDEN[case] = Golden(case)
    return _GOLDEN[case]


# ---- 4. golden parity ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES)
def test_step_matches_the_reference_recording(case):
    """Every recorded step of every recording through mt.step, teacher-forced and batched over the environments: integer leaves equal, every real leaf upstream of
    the solver at TOL_PRE, the solver's outputs at TOL_SOL.  The max_contact_points recording runs the hand-over through the candidate arrays of the workspace,
    the RK4 one the per-stage launches (asserted on the models)."""
    g = golden(case)
    if case.endswith("topk_f64"):
        assert g.model.tables.topk and any(p[0] >= 9 for p in g.model.tables.pairs)
        kept = {int(x) for e in range(g.nenv) for x in g.expected(e, 0, "contact_geom2")}
        assert kept & {2, 3, 4, 6, 7}, kept  # cylinder / ellipsoid contacts are among the kept ones
    if "rk4" in case:
        assert int(g.model.opt.integrator) == 1
    mdev = g.model.to(DEV)
    d = g.input_data()
    worst_pre = worst_sol = 0.0
    for s in range(g.nsteps):
        out = gpu_out_to_numpy(mt.step(mdev, d.to(DEV)))
        want = lambda n: np.stack([g.expected(e, s, n) for e in range(g.nenv)])
        worst_pre = max(worst_pre, max(rel_err(out[n], want(n)) for n in PRE_SOLVER))
        worst_sol = max(worst_sol, max(rel_err(out[n], want(n)) for n in SOLVER_LEAVES))
        print(f"{case} step {s}: worst pre-solver leaf {worst_pre:.2e} (bound {TOL_PRE[g.dtype]:g}), worst solver leaf {worst_sol:.2e} (bound {TOL_SOL[g.dtype]:g})")
        assert_ints_equal(lambda n: out[n], want, what=f"{case} step{s}")
        assert_leaves_close(lambda n: out[n], want, TOL_PRE[g.dtype], names=PRE_SOLVER, what=f"{case} step{s}")
        assert_leaves_close(lambda n: out[n], want, TOL_SOL[g.dtype], names=SOLVER_LEAVES, what=f"{case} step{s}")
        d = pyoracle.apply(d, {n: want(n) for n in REAL_LEAVES + INT_LEAVES})


# ---- 5. every branch of the two functions in one forward ----------------------------------------------------------------------------------------------------

def _quat(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    return np.concatenate([[np.cos(angle / 2)], np.sin(angle / 2) * a / np.linalg.norm(a)])


def _qmul(u, v):
    return np.array([u[0] * v[0] - u[1] * v[1] - u[2] * v[2] - u[3] * v[3], u[0] * v[1] + u[1] * v[0] + u[2] * v[3] - u[3] * v[2],
                     u[0] * v[2] - u[1] * v[3] + u[2] * v[0] + u[3] * v[1], u[0] * v[3] + u[1] * v[2] - u[2] * v[1] + u[3] * v[0]])


DISC_HALF, ROLLER_HALF = 0.02, 0.15  # half-lengths of the two free cylinders of tests/golden/quadric.xml
EDGE = float(PAR_EDGE)
# the disc (axis = body z) over the floor: (label, quaternion); "down": the axis is on the -normal side (plane_cylinder does not turn it round)
DISC_POSES = [
    ("flat", np.array([1.0, 0, 0, 0])),                                   # identity: len_ == 0 exactly, axis along +normal
    ("flat-down", np.array([0.0, 1, 0, 0])),                               # half a turn about x: len_ == 0 exactly, axis along -normal
    ("tilt-0.05", _quat([1, 0, 0], 0.05)), ("tilt-0.3", _quat([0, 1, 0], 0.3)), ("tilt-1.0", _quat([1, 1, 0], 1.0)), ("tilt-1.5", _quat([1, -2, 0], 1.5)),
    ("down-0.05", _quat([1, 0, 0], np.pi - 0.05)), ("down-0.7", _quat([0, 1, 0], np.pi - 0.7)),
    ("side", _quat([1, 0, 0], np.pi / 2)),                                  # tilted by pi / 2: on its side
    ("edge-below", _quat([1, 0, 0], np.arccos(EDGE * (1 - 1e-2) / DISC_HALF))), ("edge-above", _quat([1, 0, 0], np.arccos(EDGE * (1 + 1e-2) / DISC_HALF))),
    ("edge-below-down", _quat([1, 0, 0], np.pi - np.arccos(EDGE * (1 - 1e-2) / DISC_HALF))), ("edge-above-down", _quat([1, 0, 0], np.pi - np.arccos(EDGE * (1 + 1e-2) / DISC_HALF))),
]
# the roller (axis = body y) over the floor: turned about x by phi, |prjaxis * half| = 0.15 |sin phi|
ROLLER_POSES = [("side", 0.0), ("edge-below", np.arcsin(EDGE * (1 - 1e-2) / ROLLER_HALF)), ("edge-above", -np.arcsin(EDGE * (1 + 1e-2) / ROLLER_HALF)), ("tilt-0.4", 0.4), ("tilt--1.2", -1.2)]
ROLLER_UP, DISC_Z = (0.3, 0.0), (0.01, 0.25)  # the roller lifted clear of every margin or resting on the floor; the disc's centre 1 cm over the floor (every pose penetrates) or clear of it


def branch_batch(dtype, B=67, xml="quadric"):
    """B environments of tests/golden/quadric.xml (not a multiple of 64: the last workgroup of the kernel is partly filled) cycling through the poses above,
    the ellipsoid at random orientations: (model, Data on the CPU, per-environment (disc label, roller label))."""
    mx = load_model(xml, {}, dtype)
    rng = np.random.RandomState(11)
    d = mt.make_data(mx).expand(B).clone()
    q = d.qpos.clone().to(torch.float64).numpy()
    labels = []
    for e in range(B):
        dl, dq = DISC_POSES[e % len(DISC_POSES)]
        rl, phi = ROLLER_POSES[(e // 2) % len(ROLLER_POSES)]
        hi = (e // len(DISC_POSES)) % 2
        if not dl.startswith("flat") and e >= len(DISC_POSES):  # a yaw about the floor's normal changes no branch quantity of the floor pair
            dq = _qmul(_quat([0, 0, 1], rng.uniform(-3, 3)), dq)
        q[e, 2] += ROLLER_UP[hi]
        q[e, 3:7] = _quat([1, 0, 0], phi)
        q[e, 9] = DISC_Z[hi]                                     # where the roller is up the disc is down, and the other way round
        q[e, 10:14] = dq
        q[e, 14:17] += 0.03 * rng.randn(3)
        q[e, 17:21] = rng.randn(4)                               # ellipsoid: random orientation, un-normalised
        labels.append((dl, rl))
    d = d.replace(qpos=torch.tensor(q))
    return mx, (d if dtype == F64 else d.to(dtype)), labels


@pytest.mark.parametrize("dtype", [F64, F32], ids=["float64", "float32"])
def test_every_branch_in_one_forward(dtype):
    """contact_dist / pos / frame of the new pairs against tests/_quadric_ref.py evaluated on the GPU's OWN geom_xpos / geom_xmat, at TOL_PRE: the flat disc
    (len_ == 0) both ways up, axes towards and away from the plane, cylinders on their side, tilts from 0.05 rad to pi / 2, |prjaxis * half| at 1e-3 (1 -+ 1e-2),
    bodies above every margin and pushed into the floor, ellipsoids at random orientations.  The longdouble reference must see every environment on the branch
    it was posed for, every plane-cylinder pair of the batch clear of the two discontinuities by those margins: no environment is left out."""
    mx, d, labels = branch_batch(dtype)
    B = len(labels)
    out = gpu_out_to_numpy(mt.forward(mx.to(DEV), d.to(DEV)))
    got = {n: np.asarray(out[n], dtype=np.float64).reshape(B, -1, w) for n, w in zip(CONTACT_LEAVES, (1, 3, 9))}
    want = {n: got[n].copy() for n in CONTACT_LEAVES}
    seen, states = set(), set()
    margin = out["contact_includemargin"]
    for e in range(B):
        for c in pair_contacts(mx, out["geom_xpos"][e], out["geom_xmat"][e]):
            for k, t in enumerate(c["dst"]):
                want["contact_dist"][e, t, 0], want["contact_pos"][e, t], want["contact_frame"][e, t] = c["dist"][k], c["pos"][k], c["frame"][k].reshape(-1)
                states.add(bool(c["dist"][k] < margin[e, t]))
            if c["fn"] != FN_PLANE_CYLINDER:
                continue
            i = c["info"]
            assert (i["flat"] and i["len"] == 0) or i["len"] >= 0.049, (e, c["pair"], i)
            assert abs(float(i["prj_half"]) / EDGE - 1) >= 0.9e-2, (e, c["pair"], i)
            if c["geom1"] == 0 and c["geom2"] in (2, 3):  # the two posed cylinders over the floor
                label = labels[e][1 if c["geom2"] == 2 else 0]
                seen.add((c["geom2"], label))
                assert i["flat"] == label.startswith("flat"), (e, label, i)
                assert i["par"] == (label.startswith("side") or label.startswith("edge-below")), (e, label, i)
                if c["geom2"] == 3 and not label.startswith("side"):
                    assert i["flipped"] == ("down" not in label), (e, label, i)
    assert seen == {(3, l) for l, _ in DISC_POSES} | {(2, l) for l, _ in ROLLER_POSES}
    assert states == {True, False}  # contacts above the margin and penetrating
    errs = {n: rel_err(got[n], want[n]) for n in CONTACT_LEAVES}
    print(f"{dtype}: worst contact leaf of the new pairs against the longdouble reference {errs} (bound {TOL_PRE[dtype]:g})")
    assert max(errs.values()) <= TOL_PRE[dtype], errs


# ---- 6. bit-for-bit identities -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("xml,dtype", [("quadric", F64), ("quadric", F32), ("quadric_topk", F64)], ids=["float64", "float32", "topk-float64"])
def test_rows_of_a_batch_equal_single_environment_calls(xml, dtype):
    """B = 65 (a full workgroup of items and a partly filled one), B = 3 and B = 1 agree bit for bit on the handed-over contacts, environment by environment."""
    mx, d, _ = branch_batch(dtype, 65, xml)
    mdev, dg = mx.to(DEV), d.to(DEV)
    full = {n: leaf(mt.forward(mdev, dg), n).cpu().numpy() for n in CONTACT_LEAVES}
    three = {n: leaf(mt.forward(mdev, dg[:3]), n).cpu().numpy() for n in CONTACT_LEAVES}
    for n in CONTACT_LEAVES:
        assert np.array_equal(three[n], full[n][:3]), n
    for e in range(65):
        one = mt.forward(mdev, dg[e : e + 1])
        for n in CONTACT_LEAVES:
            assert np.array_equal(leaf(one, n).cpu().numpy()[0], full[n][e]), (n, e)


def _launch_ids(mdev, d):
    """Kernel ids of the launches of one step (the library's per-launch events)."""
    lib = native.load_library()
    lib.mjh_debug_phase_timing(1)
    try:
        mt.step(mdev, d)
        ms, kid = (ctypes.c_float * 96)(), (ctypes.c_int * 96)()
        n = lib.mjh_debug_phase_times(ms, kid, 96)
        return [kid[i] for i in range(n)]
    finally:
        lib.mjh_debug_phase_timing(0)


def test_the_kernel_runs_once_per_pass_and_is_accounted_alone():
    """One launch of kernel 44 per Euler step and one per RK4 stage, none of the convex kernel (10) for a model without box / mesh pairs -- and the other way
    round for a box / mesh scene; mjh_model_kernel_io accounts each of the two kernels over its own pairs."""
    QUADRIC, CONVEX = 44, 10
    rw = (ctypes.c_int64 * 2)()
    for ov, launches in (({}, 1), ({"integrator": 1}, 4)):
        mx = load_model("quadric", ov, F64)
        mdev = mx.to(DEV)
        ids = _launch_ids(mdev, mt.make_data(mx).expand(5).clone().to(DEV))
        assert ids.count(QUADRIC) == launches and CONVEX not in ids, ids
        nm = native.get_native_model(mdev, torch.device(DEV, torch.cuda.current_device()), F64)
        assert nm.lib.mjh_model_kernel_io(nm.handle, QUADRIC, rw) == 0 and (rw[0], rw[1]) == (24 * 7 * 8, 13 * 3 * 7 * 8)  # seven pairs: two frames in, up to three contacts out
        assert nm.lib.mjh_model_kernel_io(nm.handle, CONVEX, rw) == -2
    mx = load_model("mesh_contact", {}, F64)
    mdev = mx.to(DEV)
    ids = _launch_ids(mdev, mt.make_data(mx).expand(5).clone().to(DEV))
    assert ids.count(CONVEX) == 1 and QUADRIC not in ids, ids
    nm = native.get_native_model(mdev, torch.device(DEV, torch.cuda.current_device()), F64)
    npair = sum(p[0] >= 5 for p in mx.tables.pairs)
    assert nm.lib.mjh_model_kernel_io(nm.handle, CONVEX, rw) == 0 and (rw[0], rw[1]) == (24 * npair * 8, 13 * 4 * npair * 8)
    assert nm.lib.mjh_model_kernel_io(nm.handle, QUADRIC, rw) == -2


# ---- 7. downstream of a finished pass ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [F64, F32], ids=["float64", "float32"])
def test_contact_force_and_postconstraint_run_on_a_finished_pass(dtype):
    mx, d, _ = branch_batch(dtype, 16)
    mdev = mx.to(DEV)
    done = mt.forward(mdev, mt.step(mdev, d.to(DEV)))
    f = mt.contact_force(mdev, done)
    ncon = mx.constraint_sizes_py[3]
    assert f.shape == (16, ncon, 6) and bool(torch.isfinite(f).all())
    active = leaf(done, "contact_dist") < leaf(done, "contact_includemargin")
    assert bool(active.any()) and bool((~active).any())
    assert bool((f[~active] == 0).all())  # rows of inactive contacts are zero
    assert bool((f[active][:, 0] >= 0).all()) and bool((f[active][:, 0] > 0).any())  # normal forces push
    post = mt.fwd_postconstraint(mdev, done)
    for n in ("cacc", "cfrc_int", "cfrc_ext", "subtree_linvel", "subtree_angmom"):
        assert bool(torch.isfinite(getattr(post, n)).all()), n
    assert bool((post.cfrc_ext[:, 1:].abs().amax((1, 2)) > 0).any())  # contact forces on the bodies
