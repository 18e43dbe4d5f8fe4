"""``ik_site`` on the GPU (mjh_ik_site_kernel, csrc/mjh_ik.h) against the numpy longdouble reference tests/_ik_ref.py, which tests/test_ik_host.py pins on its
normal equations and on the Jacobian reference, on the targets tests/_ik_cases.py commits; and the identities the loop promises, bit for bit.

Bounds.  One iteration is compared through its update: delta = qpos' (-) qpos, formed in longdouble from the kernel's output, against the reference's delta on
the pass's own leaves, at TOL_PRE[dtype] * max(1, |qpos|, |delta|) per environment.  Errors (err_norm) are held to TOL_PRE[dtype] * max(1, err_norm).  The
condition number of G = J J^T + damping I is printed beside the shares, not allowed for.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import _ik_cases as ic
import _ik_ref as ir
import _qpos_ref as qr
import mujoco_torch_amd as mt
from _cases import F32, F64, TOL_PRE

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
LD = ir.LD
DTYPES = [pytest.param(F64, id="f64"), pytest.param(F32, id="f32")]
KEY = {F64: "f64", F32: "f32"}
B = 70
SUBSET = [1, 2, 3, 5, 7, 8]  # hinges, the slide and the ball-joint wrist


def data(mx, q):
    """A Data on the device whose qpos is q [S..., nq] (a tensor of the model's dtype), everything else as make_data leaves it."""
    d = mt.make_data(mx)
    d = d if q.dtype == F64 else d.to(q.dtype)
    return d.expand(*q.shape[:-1]).clone().replace(qpos=q.clone()).to(DEV)


def setup(dtype, seed, nb=B, spread=0.2):
    """(host model, device model, Data on the device with seeded configurations about qpos0, their float64 values)."""
    mx = ic.model(dtype)
    J = qr.joints(mx)
    rng = np.random.RandomState(seed)
    q = qr.integrate_pos(J, np.broadcast_to(mx.qpos0.double().numpy(), (nb, J[1])), spread * rng.randn(nb, J[2]), 1.0)
    q = torch.tensor(np.asarray(q, dtype=np.float64)).to(dtype)
    return mx, mx.to(DEV), data(mx, q), q.double().numpy()


def leaves_of(mdev, d, qpos=None):
    """The kinematics pass's leaves at ``qpos`` (default: d's), as host arrays."""
    p = mt.forward(mdev, d if qpos is None else d.replace(qpos=qpos), stages=ic.STAGE_KINEMATICS)
    return {n: getattr(p, n).reshape(p.qpos.shape[0], -1).double().cpu().numpy() for n in ("cdof", "subtree_com", "site_xpos", "site_xmat")}


def random_targets(dtype, seed, nb=B, reach=0.3):
    """Per-environment targets within reach of the arm's tip at qpos0: positions about it, orientations anywhere (float64 values of the dtype)."""
    rng = np.random.RandomState(seed)
    mx = ic.model()
    L = ic.kinematics(mx)(mx.qpos0.double().numpy()[None])
    tp = L["site_xpos"].reshape(-1, 3)[ic.TIP] + reach * rng.uniform(-1, 1, (nb, 3))
    tq = rng.randn(nb, 4)
    tq /= np.linalg.norm(tq, axis=-1, keepdims=True)
    rnd = lambda a: torch.tensor(a).to(dtype)
    return rnd(tp), rnd(tq)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", ["pos", "quat", "both"])
@pytest.mark.parametrize("joints", [None, SUBSET], ids=["all", "subset"])
def test_one_iteration_against_the_reference(joints, mode, dtype):
    """max_steps = 1 on the pass's own leaves: the update and the two errors, with per-environment targets and with the shared target of environment 0; with
    max_update_norm = 0.05 nearly every first update is capped (with the default 2.0 those towards a far orientation are).  rot_weight is 1, 0.37 and 2.5 in the
    three variants: it scales the orientation part of both errors and nothing else."""
    mx, mdev, d, q = setup(dtype, seed=21)
    tp, tq = random_targets(dtype, seed=22)
    tp, tq = (tp if mode != "quat" else None), (tq if mode != "pos" else None)
    T = ir.tables(mx, ic.TIP, joints)
    n = 6 if mode == "both" else 3
    L0 = leaves_of(mdev, d)
    worst = {}
    for what, shared, cap, rw in (("per-environment", False, 2.0, 1.0), ("shared", True, 2.0, 0.37), ("capped", False, 0.05, 2.5)):
        pick = lambda t: None if t is None else (t[0] if shared else t)
        host = lambda t: None if t is None else pick(t).double().numpy()
        devt = lambda t: None if t is None else pick(t).to(DEV)
        ref = ir.iteration(T, L0, q, host(tp), host(tq), tol=0.0, max_update_norm=cap, rot_weight=rw)
        res = mt.ik_site(mdev, d, ic.TIP, devt(tp), devt(tq), joints=joints, tol=0.0, max_steps=1, max_update_norm=cap, rot_weight=rw)
        zero = mt.ik_site(mdev, d, ic.TIP, devt(tp), devt(tq), joints=joints, tol=0.0, max_steps=0, rot_weight=rw)
        assert (res.steps == 1).all() and (zero.steps == 0).all() and not res.success.any() and torch.equal(zero.qpos, d.qpos)
        got_q = res.qpos.double().cpu().numpy()
        assert np.isfinite(got_q).all()
        # the error at the start, and the error at the new configuration on the pass's own leaves there
        e0 = np.abs(zero.err_norm.double().cpu().numpy() - ref["err_norm"]) / (TOL_PRE[dtype] * np.maximum(1, ref["err_norm"]))
        _, e1_ref = ir.error(T, leaves_of(mdev, d, res.qpos), host(tp), host(tq), rw)
        e1 = np.abs(res.err_norm.double().cpu().numpy() - e1_ref) / (TOL_PRE[dtype] * np.maximum(1, e1_ref))
        # the update
        delta = qr.differentiate_pos(T["J"], q, got_q, 1.0)
        G = np.asarray(ref["J"] @ np.swapaxes(ref["J"], -1, -2), dtype=np.float64) + 1e-6 * np.eye(n)
        cond = np.linalg.cond(G)
        dn = np.sqrt((ref["delta"] ** 2).sum(-1))
        bound = TOL_PRE[dtype] * np.maximum(1, np.maximum(np.abs(q).max(-1), dn))
        ed = np.abs(delta - ref["delta"]).max(-1) / bound
        worst[what] = (float(e0.max()), float(e1.max()), float(ed.max()), float(cond.max()))
        # |delta| <= max_update_norm to rounding (the update is read off qpos, whose entries are rounded), and = max_update_norm where the reference caps
        raw = np.sqrt((ir.iteration(T, L0, q, host(tp), host(tq), tol=0.0, max_update_norm=1e30)["delta"] ** 2).sum(-1))
        got_n, slack = np.sqrt((delta ** 2).sum(-1)), TOL_PRE[dtype] * np.maximum(1, np.abs(q).max(-1))
        assert (got_n <= cap + slack).all()
        capped = raw > cap * (1 + 1e-6)
        assert (np.abs(got_n - cap)[capped] <= slack[capped]).all() and (capped.mean() > 0.9 or cap > 1), capped.mean()
        # joints outside the selection: bit for bit
        for (t, qa, da), moved in zip(T["J"][0], T["moved"]):
            if not moved:
                w = {qr.FREE: 7, qr.BALL: 4}.get(t, 1)
                assert torch.equal(res.qpos[:, qa:qa + w], d.qpos[:, qa:qa + w])
    print(f"{mode} {'all' if joints is None else 'subset'} {dtype}: (start error, end error, update) over bound, largest cond(G): "
          f"{({k: tuple(f'{x:.2e}' for x in v) for k, v in worst.items()})}")
    assert max(max(v[:3]) for v in worst.values()) <= 1, worst


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", list(ic.CASES))
def test_the_loop_on_the_committed_targets(case, dtype):
    """success everywhere; on clear targets the reference's step count exactly; the site pose of the result, recomputed with forward, meets tol; every
    quaternion of the result is unit to TOL_PRE."""
    key = KEY[dtype]
    t, ref, tol = ic.targets(case, key), ic.reference(case, key), ic.TOL[key]
    mx = ic.model(dtype)
    mdev = mx.to(DEV)
    nb = t["qpos0"].shape[0]
    d = data(mx, torch.tensor(t["qpos0"]).to(dtype))
    tens = lambda a: None if a is None else torch.tensor(a).to(dtype).to(DEV)
    tp, tq = tens(t["target_pos"]), tens(t["target_quat"])
    res = mt.ik_site(mdev, d, t["site"], tp, tq, joints=t["joints"], tol=tol, max_steps=ic.MAX_STEPS, **t["kw"])
    steps = res.steps.cpu().numpy()
    print(f"{case} {key}: steps {steps.tolist()}, reference {ref['steps'].tolist()}, clear {ref['clear'].astype(int).tolist()}, "
          f"worst err_norm {res.err_norm.max().item():.2e} (tol {tol:g})")
    assert res.success.all() and (res.err_norm < tol).all()
    assert np.array_equal(steps[ref["clear"]], ref["steps"][ref["clear"]])
    T = ir.tables(mx, t["site"], t["joints"])
    host = lambda x: None if x is None else x.double().cpu().numpy()
    _, err = ir.error(T, leaves_of(mdev, d, res.qpos), host(tp), host(tq))
    print(f"{case} {key}: worst recomputed error {float(err.max()):.2e}")
    assert (err < tol).all()
    q = res.qpos.double().cpu().numpy()
    for k in qr.quat_slices(T["J"]):
        assert np.abs(np.linalg.norm(q[:, k:k + 4], axis=-1) - 1).max() <= TOL_PRE[dtype]


def _problem(dtype):
    """B = 70 environments: seeded configurations, near qpos0 in the first half and far from it in the second (so that the step counts differ), the committed
    tip_both targets of the dtype repeated."""
    mx, mdev, d, q = setup(dtype, seed=23, spread=np.where(np.arange(B) < B // 2, 0.05, 0.8)[:, None])
    t = ic.targets("tip_both", KEY[dtype])
    reps = -(-B // t["qpos0"].shape[0])
    tp = torch.tensor(np.tile(t["target_pos"], (reps, 1))[:B]).to(dtype).to(DEV)
    tq = torch.tensor(np.tile(t["target_quat"], (reps, 1))[:B]).to(dtype).to(DEV)
    return mx, mdev, d, tp, tq


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("dtype", DTYPES)
def test_identities_bit_for_bit(dtype):
    mx, mdev, d, tp, tq = _problem(dtype)
    tol = ic.TOL[KEY[dtype]]
    full = mt.ik_site(mdev, d, ic.TIP, tp, tq, tol=tol)
    assert full.success.all() and len(set(full.steps.tolist())) > 1
    # an environment alone, and as a row of a (2, 3) batch
    for e in (0, 33, 69):
        one = mt.ik_site(mdev, data(mx, d.qpos[e:e + 1].cpu()), ic.TIP, tp[e:e + 1], tq[e:e + 1], tol=tol)
        assert _same(one, [x[e:e + 1] for x in full]), e
    six = mt.ik_site(mdev, data(mx, d.qpos[:6].reshape(2, 3, -1).cpu()), ic.TIP, tp[:6].reshape(2, 3, 3), tq[:6].reshape(2, 3, 4), tol=tol)
    assert tuple(six.steps.shape) == (2, 3) and _same([x.reshape((6,) + tuple(x.shape[2:])) for x in six], [x[:6] for x in full])
    # a shared target: the row of the environment whose target it is
    shared = mt.ik_site(mdev, d, ic.TIP, tp[4], tq[4], tol=tol)
    assert _same([x[4] for x in shared], [x[4] for x in full])
    # max_steps = k and k + 5: equal wherever the environment was done by k
    k = int(full.steps.min().item())
    short, longer = (mt.ik_site(mdev, d, ic.TIP, tp, tq, tol=tol, max_steps=m) for m in (k, k + 5))
    done = short.success
    assert done.any() and not done.all() and longer.success.sum() > done.sum()
    assert _same([x[done] for x in short], [x[done] for x in longer]) and (short.steps[~done] == k).all()
    # unselected joints keep their entries: the subset leaves the other hinges and the probe's free joint alone, qpos of d is not written
    before = d.qpos.clone()
    sub = mt.ik_site(mdev, d, ic.TIP, tp, tq, joints=SUBSET, tol=tol)
    T = ir.tables(mx, ic.TIP, SUBSET)
    kept = np.ones(int(mx.nq), dtype=bool)
    for (t, qa, da), moved in zip(T["J"][0], T["moved"]):
        if moved:
            kept[qa:qa + {qr.FREE: 7, qr.BALL: 4}.get(t, 1)] = False
    kept = torch.tensor(kept, device=DEV)
    assert kept.sum() == 3 + 7 and torch.equal(sub.qpos[:, kept], before[:, kept]) and not torch.equal(sub.qpos[:, ~kept], before[:, ~kept])
    assert torch.equal(d.qpos, before)


def test_kernel_ids_and_byte_accounts():
    """The two kernels report under their timing ids (48, 49), one launch a call at this batch, and ``mjh_model_kernel_io`` accounts them per environment:
    an integrate call reads qpos and qvel and writes qpos; an updating IK call with both targets reads cdof, the site's frame (12 reals), its root's
    subtree_com (3), the targets (7), qpos and the three state words, and writes qpos and the state words."""
    import ctypes

    from mujoco_torch_amd import native

    mx, mdev, d, tp, tq = _problem(F64)
    nm = native.get_native_model(mdev, torch.device("cuda", 0), F64)
    nq, nv = int(mx.nq), int(mx.nv)
    rw = (ctypes.c_int64 * 2)()
    assert nm.lib.mjh_model_kernel_io(nm.handle, 48, rw) == 0 and (rw[0], rw[1]) == ((nq + nv) * 8, nq * 8)
    assert nm.lib.mjh_model_kernel_io(nm.handle, 49, rw) == 0 and (rw[0], rw[1]) == ((6 * nv + 12 + 3 + 7 + nq + 1) * 8 + 5, (nq + 1) * 8 + 5)
    calls = {48: lambda: mt.integrate_pos(mdev, d.qpos, torch.zeros(B, nv, dtype=F64, device=DEV), 0.1), 49: lambda: mt.ik_site(mdev, d, ic.TIP, tp, tq, max_steps=2)}
    for kid, call in calls.items():
        nm.lib.mjh_debug_phase_timing(1)
        try:
            call()
            ms, ids = (ctypes.c_float * 96)(), (ctypes.c_int * 96)()
            n = nm.lib.mjh_debug_phase_times(ms, ids, 96)  # (the launches of the most recent native call)
        finally:
            nm.lib.mjh_debug_phase_timing(0)
        assert [ids[i] for i in range(n)] == [kid] and ms[0] > 0, kid


_CUT_CHILD = r'''
import sys
sys.path.insert(0, "tests"); sys.path.insert(0, "mujoco-torch_amd"); sys.path.insert(0, "oracle")
import torch, mujoco_torch_amd as mt
import test_ik as ti
res = {}
for dtype in (torch.float64, torch.float32):
    mx, mdev, d, tp, tq = ti._problem(dtype)
    r = mt.ik_site(mdev, d, 0, tp, tq, tol=ti.ic.TOL[ti.KEY[dtype]])
    v = torch.ones(ti.B, int(mx.nv), dtype=dtype, device="cuda") * 0.3
    out = dict(qpos=r.qpos, err_norm=r.err_norm, steps=r.steps, success=r.success, integrate=mt.integrate_pos(mdev, d.qpos, v, 0.5),
               differentiate=mt.differentiate_pos(mdev, d.qpos, r.qpos, 0.5), normalize=mt.normalize_quat(mdev, 3 * r.qpos))
    res[str(dtype)] = {k: o.cpu() for k, o in out.items()}
torch.save(res, sys.argv[1])
print("ran")
'''
CUT_LOG2 = 2


def test_batches_past_one_launch_are_cut_on_the_host():
    """MJH_MAX_GRID_LOG2=2 caps a launch at 4 workgroups: 4 environments of the IK kernel, 256 (environment, joint) items of the arithmetic kernel (700 in
    all, the boundaries inside an environment).  The loop and the three operations on 70 environments must be bit-identical to the uncut run, in a fresh
    process each (the library reads the switch once)."""
    assert B > (1 << CUT_LOG2) and B % (1 << CUT_LOG2) != 0 and (64 << CUT_LOG2) % 10 != 0 and B * 10 > (64 << CUT_LOG2)
    with tempfile.TemporaryDirectory() as td:
        res = {}
        for tag, env in (("one", {}), ("cut", {"MJH_MAX_GRID_LOG2": str(CUT_LOG2)})):
            f = os.path.join(td, tag + ".pt")
            base = {k: v for k, v in os.environ.items() if k != "MJH_MAX_GRID_LOG2"}
            r = subprocess.run([sys.executable, "-c", _CUT_CHILD, f], cwd=ROOT, env=dict(base, **env), capture_output=True, text=True, timeout=600)
            assert r.returncode == 0 and "ran" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
            res[tag] = torch.load(f)
    for dts, outs in res["one"].items():
        assert len(outs) == 7 and outs["success"].all()
        for k, a in outs.items():
            assert a.shape[0] == B and torch.isfinite(a.double()).all() and torch.equal(a, res["cut"][dts][k]), (dts, k)


@pytest.mark.parametrize("dtype", DTYPES)
def test_an_unreachable_target(dtype):
    """10 m beyond the reach of the hinges and the wrist (the slide, which has no range, is left out of the selection): no success, every update taken, every
    output finite."""
    mx, mdev, d, q = setup(dtype, seed=24, nb=5)
    tp = torch.tensor([11.5, 0.0, 0.3]).to(dtype).to(DEV)  # (the arm is 1.45 m long)
    for tq in (None, torch.tensor([1.0, 0, 0, 0]).to(dtype).to(DEV)):
        res = mt.ik_site(mdev, d, ic.TIP, tp, tq, joints=list(range(7)) + [8], max_steps=7)
        assert not res.success.any() and (res.steps == 7).all() and (res.err_norm > 9.5).all()
        assert all(torch.isfinite(x.double()).all() for x in res)
        assert torch.equal(res.qpos[:, 7], d.qpos[:, 7])
