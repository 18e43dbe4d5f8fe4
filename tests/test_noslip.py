"""``solve_noslip`` on the device (csrc/mjh_noslip.h) against the numpy longdouble reference tests/_noslip_ref.py -- the definitions in the ``A`` / ``b`` form, which
tests/test_noslip_host.py pins on hand-worked problems -- evaluated on the SAME rounded inputs: the leaves of this library's own ``forward``, B in {1, 3, 70}.

The states (``state``).  humanoid and centipede_106: ``_cases.seeded_batch`` as it is.  The ant has no floor: its contacts are between its own capsules, and at the
seeded pose the only active ones join geoms that cannot move against each other (``J = 0``: degenerate blocks).  Its joints are therefore thrown far past their
ranges (``qpos`` +- 2.5 rad) so that legs meet, with joint velocities from 5e-5 to 5 rad/s over the batch: contacts that stick and contacts that slide, friction-loss
rows inside and on their bounds.  convex_primitives: the seeded poses, but the small box (condim 4) stands alone on the floor instead of on the large one -- stacked,
two of its box-box contacts have identical rows, ``A`` is singular across them and Gauss-Seidel needs some 400 sweeps where the slip check allows 64 --, and the
large box, the small box and the sphere get tangential velocities and spins from 1e-3 to 3 over the batch.  Under the elliptic cone the model's torsional and
rolling coefficients are 0 on the boxes (a singular block: ``v = 0``, covered by every third environment, which keeps them) and 0.01 / 0.001 on the sphere (a
cone no update ends inside), so the ``contact.friction`` leaf -- an input of ``solve_noslip`` -- is set to 0.05 / 0.3 there on the other environments AFTER the pass:
those inputs are forward's leaves but for that one.  centipede_106 stages 5 chunks of 19 rows and a last one of 4.

No bound here is read off the kernel.  Values are held to ``max(TOL_PRE[dtype], 4 x the error of _noslip_ref run in the same dtype on the same inputs at the same
sweep count)`` by ``_util.rel_err``, the rule of tests/test_pgs.py.  The random ``force0`` is of unit size, not of the size of the pass's forces (1e5 to 1e6 on
the ant): a block is put back when its cost change exceeds 1e-10, an absolute figure, and with forces of 1e6 the rounding of that change in float64 (some 1e-7) is
far above it -- at a block's fixed point the choice is then rounding's, in any arithmetic, and the force moves by 1e-9 of its size with it.  With forces of order
one the change is resolved against the threshold.  The promises (untouched rows, bounds, signs, ``iterations=0``) and the bit identities carry no tolerance.
The slacks of the properties are written down where they are used.
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

import _efc_ref as er
import _noslip_ref as nr
import mujoco_torch_amd as mt
from _cases import F32, F64, TOL_PRE, seeded_batch
from _util import rel_err
from mujoco_torch_amd import native

pytestmark = pytest.mark.gpu

DEV = "cuda"
LD = er.LD
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ELL = (("cone", 1),)
MODELS = [("humanoid", (), F64), ("ant", ELL, F64), ("ant", ELL, F32), ("ant_frictionloss", (), F64), ("convex_primitives", (), F64), ("convex_primitives", ELL, F64),
          ("centipede_106", (), F64)]
IDS = [f"{x}-{'elliptic-' if ov else ''}{str(t)[6:]}" for x, ov, t in MODELS]
BATCHES = (1, 3, 70)
SWEEPS = (1, 2, 7)
LEAVES = ("efc_J", "efc_D", "efc_aref", "efc_frictionloss", "efc_force", "qLD", "qacc_smooth")
NAMES = ("efc_force", "qfrc_constraint", "qacc", "cost", "improvement")
NPDT = {F64: np.float64, F32: np.float32}


def sizes(m):
    ne, nf, _, ncon, nefc = (int(x) for x in m.constraint_sizes_py)
    return ne, nf, nefc, int(m.nv), float(m.stat.meaninertia) * max(1, int(m.nv)), ncon


def host(t):
    return t.detach().cpu().numpy()


def f64(x):
    return np.asarray(x, dtype=np.float64)


def state(xml, ov, dtype, B):
    """(host model, Data before the pass, what to do to the Data after it): the module's docstring has the recipe."""
    mc, d = seeded_batch(xml, dict(ov), dtype, B)
    rng = np.random.RandomState(3)
    after = lambda d: d
    if xml.startswith("ant"):
        s = 10.0 ** np.linspace(-5, 0, B)
        d = d.replace(qpos=d.qpos + torch.tensor(2.5 * rng.uniform(-1, 1, (B, int(mc.nq))), dtype=dtype),
                      qvel=torch.tensor(5.0 * s[:, None] * rng.randn(B, int(mc.nv)), dtype=dtype), ctrl=d.ctrl * torch.tensor(s[:, None], dtype=dtype))
    if xml == "convex_primitives":
        q = d.qpos.clone()  # (free joints in order: box2, smallbox, ball, capsule, capsule_edge)
        q[:, 7:10] = torch.tensor(np.array([2.2, 1.0, 0.1]) + np.array([0.01, 0.01, 0.003]) * rng.randn(B, 3), dtype=dtype)
        v, s = np.zeros((B, int(mc.nv))), 10.0 ** np.linspace(-3, 0.5, B)
        for a in (0, 6, 12):  # box2, smallbox, ball: tangential velocity and spin
            v[:, a:a + 2] = s[:, None] * rng.randn(B, 2)
            v[:, a + 3:a + 6] = 3 * s[:, None] * rng.randn(B, 3)
        d = d.replace(qpos=q, qvel=d.qvel + torch.tensor(v, dtype=dtype))
        if ov:
            def after(d):
                fr = d.contact.friction.clone()
                e = torch.arange(B, device=fr.device)
                for r, v in ((1, 0.05), (2, 0.3)):
                    fr[e % 3 == r, :, 2:] = fr[e % 3 == r, :, 2:].clamp(min=v)
                return d.replace(contact=d.contact.replace(friction=fr))
    return mc, d, after


def start_of(mc, f, con, elliptic, seed=5):
    """A random start of unit size (the module's docstring says why not of the size of the pass's forces): both signs on the friction-loss rows (far past their bounds) and on the friction rows of elliptic contacts,
    non-negative on every other row (limit rows, normals, pyramid edges), as a main solver leaves them."""
    ne, nf, nefc, *_ = sizes(mc)
    rng = np.random.RandomState(seed)
    f0 = rng.randn(*f.shape)
    signed = np.zeros(nefc, dtype=bool)
    signed[:ne + nf] = True
    if elliptic:
        for adr, dim in con:
            signed[adr + 1:adr + dim] = True
    f0[:, ~signed] = np.abs(f0[:, ~signed])
    return f0


@functools.lru_cache(maxsize=None)
def passed(xml, ov, dtype, B, device=None):
    """(host model, device model, Data after forward on the device, its leaves on the host [B, ...] with the contact table, a random start on the device): computed
    once and shared."""
    device = device or DEV
    mc, d, after = state(xml, ov, dtype, B)
    mx = mc.to(device)
    d = after(mt.forward(mx, d.to(device)))
    ne, nf, nefc, nv, _, ncon = sizes(mc)
    tail = dict(efc_J=(nefc, nv), qLD=(nv, nv))
    A = {n: host(getattr(d, n)).reshape((B,) + tail.get(n, (-1,))) for n in LEAVES}
    dims = np.asarray(mc.tables.con_dim)[:ncon]
    A["con"] = nr.contacts(dims, mc.tables.con_efc_address, ncon)
    A["mu"] = host(d.contact.friction).reshape(B, ncon, 5)[:, [i for i, x in enumerate(dims) if x > 1]]
    A["elliptic"] = int(mc.opt.cone) == 1
    f0 = torch.tensor(start_of(mc, A["efc_force"], A["con"], A["elliptic"]), dtype=dtype, device=device)
    return mc, mx, d, A, f0


def run_reference(mc, A, start, sweeps, dtype=LD, tolerance=-np.inf):
    ne, nf, _, _, scale, _ = sizes(mc)
    return nr.solve_noslip(A["efc_J"], A["efc_D"], A["efc_aref"], A["efc_frictionloss"], A["qLD"], A["qacc_smooth"], start, A["mu"], ne, nf, A["con"], A["elliptic"],
                           scale, sweeps, tolerance=tolerance, dtype=dtype)


@functools.lru_cache(maxsize=None)
def reference(xml, ov, dtype, B, warm, sweeps=max(SWEEPS)):
    """(the longdouble reference, the reference in the dtype) of ``sweeps`` sweeps that never stop (``tolerance = -inf``): every sweep's force, improvement, cost
    and block status."""
    mc, _, _, A, f0 = passed(xml, ov, dtype, B)
    start = host(f0) if warm else A["efc_force"]
    return run_reference(mc, A, start, sweeps), run_reference(mc, A, start, sweeps, NPDT[dtype])


def at_sweep(A, ref, niter, dtype=LD):
    """The reference's outputs with environment e taken after ``niter[e]`` sweeps."""
    e = np.arange(len(niter))
    f = ref["forces"][niter, e]
    qfrc, qacc = nr.pr.finish(A["efc_J"], A["qLD"], A["qacc_smooth"], f, dtype)
    imp = np.where(niter > 0, ref["improvements"][np.maximum(niter, 1) - 1, e], 0)
    return dict(efc_force=f, qfrc_constraint=qfrc, qacc=qacc, cost=ref["costs"][niter, e], improvement=imp)


def touched_rows(mc, A):
    """The rows a sweep may change: friction-loss rows, the rows of pyramidal contacts of condim > 1, the friction rows of elliptic ones."""
    ne, nf, nefc, *_ = sizes(mc)
    t = np.zeros(nefc, dtype=bool)
    t[ne:ne + nf] = True
    for adr, dim in A["con"]:
        if A["elliptic"]:
            t[adr + 1:adr + dim] = True
        else:
            t[adr:adr + 2 * (dim - 1)] = True
    return t


def coverage(A, status):
    """{condim: [blocks without a positive normal force, ended strictly inside, on the boundary, put back, degenerate]} of one sweep's block statuses."""
    out = {}
    for (ci, _), s in ((k, v) for k, v in status.items() if k != "fl"):
        out.setdefault(A["con"][ci][1], np.zeros(5, dtype=int))
        out[A["con"][ci][1]] += np.bincount(s, minlength=5)
    return out


# ---- the inputs exercise the code ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("xml,ov,dtype", MODELS, ids=IDS)
def test_the_inputs_exercise_the_code(xml, ov, dtype):
    """Counted with the reference, over the 70 environments, on the first sweep from the pass's own force: every condim present has a contact with a positive
    normal force whose update ends strictly inside its cone (pair: both edges positive) and one whose update ends on the boundary; friction-loss rows, where the
    model has them, end inside and on their bounds.  Expected condims: humanoid, the ants and the centipede 3; convex_primitives 3, 4 and 6 (QCQPs of 2, 3 and 5
    rows, 2, 3 and 5 pairs)."""
    mc, _, _, A, _ = passed(xml, ov, dtype, 70)
    ref, _ = reference(xml, ov, dtype, 70, False)
    cov = coverage(A, ref["status"][0])
    print(f"{xml} {dict(ov)} {dtype}: nv {sizes(mc)[3]}, nefc {sizes(mc)[2]}, contacts with friction {len(A['con'])}; first sweep, by condim "
          f"[no normal force, inside, boundary, put back, degenerate]: { {k: v.tolist() for k, v in cov.items()} }")
    assert sorted(cov) == ([3, 4, 6] if xml == "convex_primitives" else [3])
    for dim, c in cov.items():
        assert c[nr.INTERIOR] >= 1 and c[nr.BOUNDARY] >= 1, (dim, c)
    if xml == "ant_frictionloss":
        fl = np.bincount(ref["status"][0]["fl"].ravel(), minlength=3)
        print(f"  friction-loss rows [skipped, inside, on a bound]: {fl.tolist()}")
        assert sizes(mc)[1] == 8 and fl[nr.INTERIOR] >= 1 and fl[nr.BOUNDARY] >= 1
    if xml == "convex_primitives" and ov:
        assert cov[4][nr.DEGENERATE] >= 1  # (the singular block: torsional coefficient 0)


# ---- fixed sweeps against the reference -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("warm", [False, True], ids=["efc_force", "force0"])
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("xml,ov,dtype", MODELS, ids=IDS)
def test_fixed_sweeps_against_the_reference(xml, ov, dtype, B, warm):
    """``tolerance = 0``, 1, 2 and 7 sweeps, from the pass's own force and from a random ``force0``: force, ``J^T f``, ``qacc``, cost and improvement against
    longdouble, each within ``max(TOL_PRE, 4 x the same-dtype reference's error)``.  ``niter == iterations`` -- unless the environment's own improvement came out
    negative, which by the stopping rule ``improvement < tolerance`` ends it at ``tolerance = 0`` too (a converged environment whose accepted blocks raise the
    cost by rounding, each by less than 1e-10): every environment is compared with the reference after the sweeps IT ran, the reference never stopping.

    Measured: the table of ``solve_noslip`` in DESIGN.md."""
    mc, mx, d, A, f0 = passed(xml, ov, dtype, B)
    ref, same = reference(xml, ov, dtype, B, warm)
    assert ref["qcqp_converged"]  # (the yardstick's QCQPs are iterated until they stop by themselves)
    worst = 0.0
    print(f"{xml} {dict(ov)} {dtype} B={B} {'force0' if warm else 'efc_force'}: nv {sizes(mc)[3]}, nefc {sizes(mc)[2]}")
    for k in SWEEPS:
        res = mt.solve_noslip(mx, d, iterations=k, tolerance=0.0, force0=f0 if warm else None)
        niter = host(res.niter)
        assert res.niter.dtype == torch.int32 and (niter >= 1).all() and ((niter == k) | ((niter < k) & (host(res.improvement) < 0))).all()
        want, other = at_sweep(A, ref, niter), at_sweep(A, same, niter, NPDT[dtype])
        for n in NAMES:
            e_same, e_new = rel_err(f64(other[n]), f64(want[n])), rel_err(host(getattr(res, n)), f64(want[n]))
            bound = max(TOL_PRE[dtype], 4 * e_same)
            worst = max(worst, e_new / bound)
            print(f"  {k} sweeps: {n}: rel_err {e_new:.3g}, the reference in the dtype {e_same:.3g}, bound {bound:.3g} ({e_new / bound:.2g} of it)")
            assert np.isfinite(e_new) and e_new <= bound, (n, k, e_new, bound)
    print(f"  worst error / bound {worst:.3g}")


# ---- what noslip promises, with no tolerance ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("xml,ov,dtype", MODELS, ids=IDS)
def test_promises_hold_exactly(xml, ov, dtype):
    """After 0, 1, 3 and 16 sweeps from either start: every row that is not a friction dimension equals the start bit for bit; friction-loss rows are within
    their bounds (after at least one sweep from the random start, which is far outside them); pyramid forces are ``>= 0``; ``iterations=0`` returns the start
    bit for bit, with ``niter = 0``, ``improvement = 0`` and the ``qfrc_constraint``, ``qacc`` and ``cost`` of that force."""
    mc, mx, d, A, f0 = passed(xml, ov, dtype, 70)
    ne, nf, nefc, nv, _, _ = sizes(mc)
    touched = touched_rows(mc, A)
    print(f"{xml} {dict(ov)} {dtype}: {int(touched.sum())} of {nefc} rows are friction dimensions")
    assert touched.any() and (touched.all() == (xml == "convex_primitives" and not ov))  # (the pyramidal convex primitives have nothing but contacts with friction)
    for start in (None, f0):
        s = A["efc_force"] if start is None else host(f0)
        for k in (0, 1, 3, 16):
            res = mt.solve_noslip(mx, d, iterations=k, tolerance=0.0, force0=start)
            f = host(res.efc_force)
            assert np.isfinite(f).all()
            assert np.array_equal(f[:, ~touched], s[:, ~touched])
            if k or start is None:
                assert (np.abs(f[:, ne:ne + nf]) <= A["efc_frictionloss"][:, ne:ne + nf]).all()
            if not A["elliptic"]:
                assert (f[:, ne + nf:] >= 0).all()
            if k == 0:
                assert np.array_equal(f, s) and not res.niter.any() and not res.improvement.any()
                ref = run_reference(mc, A, s, 0)
                for n in ("qfrc_constraint", "qacc", "cost"):
                    assert rel_err(host(getattr(res, n)), f64(ref[n])) <= TOL_PRE[dtype], n
    shared = mt.solve_noslip(mx, d[:3], iterations=2, tolerance=0.0, force0=f0[1].contiguous())  # a shared start is that start repeated
    assert all(torch.equal(a, b) for a, b in zip(shared, mt.solve_noslip(mx, d[:3], iterations=2, tolerance=0.0, force0=f0[1].expand(3, -1).contiguous())))


# ---- properties, with rounding slack only ---------------------------------------------------------------------------------------------------------

def residuals(A, prob, f):
    """res = A f + b in longdouble, [B, n], and the rounding floor of its evaluation in the dtype's arithmetic per unit eps: sum_j |A_ij f_j| + |b_i|."""
    Am, b, _ = prob
    f = er.ld(f)
    return np.einsum("bij,bj->bi", Am, f) + b, np.einsum("bij,bj->bi", np.abs(Am), np.abs(f)) + np.abs(b)


@pytest.mark.parametrize("xml,ov,dtype", MODELS, ids=IDS)
def test_properties_up_to_rounding(xml, ov, dtype):
    """From the pass's own force, B = 70.

    * A pyramid pair's sum is kept: ``mid`` rounds the sum once, ``mid + yy`` and ``mid - yy`` round once each: after k sweeps within ``4 k eps`` of the pair's
      magnitude.
    * An elliptic block whose friction rows are not the start's bits (it was updated, not put back) satisfies ``sum (f_k / mu_k)^2 <= f_n^2 (1 + 8 eps)``, a row with
      ``mu_k = 0`` carrying 0; with ``f_n < MINVAL`` the friction rows are 0.
    * ``cost`` after 1, 4 and 16 sweeps is non-increasing within ``2 TOL_PRE S``, ``S`` the sum of the magnitudes of the terms of ``1/2 f^T A f + f . b`` (the
      slack tests/test_pgs.py derives: two evaluations in the dtype are compared; an accepted block may raise the cost by 1e-10, far below it).
    * The slip the feature removes.  On the rows that end strictly interior after 64 sweeps -- both members of a pair ``> 0``, an elliptic block inside its cone,
      a friction-loss row inside its bounds; the blocks the solver cannot move are left out (a pair with ``K1 < MINVAL``, an elliptic block whose ``A_s`` has no
      Cholesky factor: their residual is a constant) -- the residual (``res_j - res_j+1`` for a pair, ``res`` otherwise), recomputed in longdouble from the device's force,
      is per environment (the largest over those rows) smaller after 64 sweeps than after 4, unless the value after 4 is already at the rounding floor of a
      residual in the dtype, ``(nefc + nv) eps (sum_j |A_ij f_j| + |b_i|)``, or the four sweeps had reached the fixed point (the same bits after 64).
      (Gauss-Seidel lowers the cost sweep by sweep, not every row's residual before it has converged: the states of this file converge within 64 sweeps -- the
      small box of convex_primitives stands alone, see the module's docstring.)"""
    mc, mx, d, A, _ = passed(xml, ov, dtype, 70)
    ne, nf, nefc, nv, _, _ = sizes(mc)
    eps, tol = float(torch.finfo(dtype).eps), TOL_PRE[dtype]
    s = A["efc_force"]
    runs = {k: mt.solve_noslip(mx, d, iterations=k, tolerance=0.0) for k in (1, 4, 16, 64)}
    F = {k: host(r.efc_force) for k, r in runs.items()}
    mu = A["mu"]
    for k in (1, 4):
        f = F[k]
        for ci, (adr, dim) in enumerate(A["con"]):
            if A["elliptic"]:
                rows = slice(adr + 1, adr + dim)
                m, fn = er.ld(mu[:, ci, :dim - 1]), er.ld(f[:, adr])
                same = (f[:, rows] == s[:, rows]).all(-1)
                assert not f[:, rows][np.broadcast_to(m == 0, f[:, rows].shape) & ~same[:, None]].any()
                ratio = ((er.ld(f[:, rows]) / np.where(m == 0, 1, m)) ** 2).sum(-1)
                small = f[:, adr] < nr.MINVAL
                assert (same | small | (ratio <= fn * fn * (1 + 8 * eps))).all(), (ci, dim)
                assert not f[:, rows][small & ~same].any()
            else:
                for p in range(dim - 1):
                    j = adr + 2 * p
                    drift = np.abs((er.ld(f[:, j]) + er.ld(f[:, j + 1])) - (er.ld(s[:, j]) + er.ld(s[:, j + 1])))
                    assert (drift <= 4 * k * eps * (np.abs(s[:, j]) + np.abs(s[:, j + 1]))).all(), (ci, p, k)
    prob = nr.problem(A["efc_J"], A["efc_D"], A["efc_aref"], A["qLD"], A["qacc_smooth"])
    Am, b, _ = prob
    S = {k: f64(np.einsum("bi,bij,bj->b", np.abs(er.ld(F[k])), np.abs(Am), np.abs(er.ld(F[k]))) / 2 + (np.abs(er.ld(F[k])) * np.abs(b)).sum(-1)) for k in F}
    cost = {k: host(r.cost).astype(np.float64) for k, r in runs.items()}
    for a, c in ((1, 4), (4, 16)):
        slack = 2 * tol * np.maximum(S[a], S[c])
        print(f"{xml} {dict(ov)} {dtype}: cost after {c} sweeps - after {a}: max {float((cost[c] - cost[a]).max()):.3g}, largest (difference / slack) "
              f"{float(((cost[c] - cost[a]) / np.maximum(slack, 1e-300)).max()):.3g}")
        assert (cost[c] <= cost[a] + slack).all()
    f = F[64]
    sel, kind = np.zeros((70, nefc), dtype=bool), np.zeros(nefc, dtype=int)  # kind 1: the first row of a pair (its residual: res_j - res_j+1)
    sel[:, ne:ne + nf] = np.abs(f[:, ne:ne + nf]) < A["efc_frictionloss"][:, ne:ne + nf]
    for ci, (adr, dim) in enumerate(A["con"]):
        if A["elliptic"]:
            m = er.ld(mu[:, ci, :dim - 1])
            rows = slice(adr + 1, adr + dim)
            ratio = ((er.ld(f[:, rows]) / np.where(m == 0, 1, m)) ** 2).sum(-1)
            idx = np.arange(adr + 1, adr + dim)
            regular = nr._chol(Am[:, idx[:, None], idx[None, :]] * m[:, :, None] * m[:, None, :])[1]
            inside = regular & (f[:, adr] >= nr.MINVAL) & (ratio < er.ld(f[:, adr]) ** 2 * (1 - 8 * eps))
            sel[:, rows] = inside[:, None]
        else:
            for p in range(dim - 1):
                j = adr + 2 * p
                K1 = Am[:, j, j] + Am[:, j + 1, j + 1] - Am[:, j, j + 1] - Am[:, j + 1, j]
                sel[:, j] = (f[:, j] > 0) & (f[:, j + 1] > 0) & ~(K1 < nr.MINVAL)
                kind[j] = 1
    slip, floor = {}, {}
    for k in (4, 64):
        res, mag = residuals(A, prob, F[k])
        pair = kind == 1
        res[:, pair] = res[:, pair] - res[:, np.flatnonzero(pair) + 1]
        mag[:, pair] = mag[:, pair] + mag[:, np.flatnonzero(pair) + 1]
        slip[k] = f64(np.where(sel, np.abs(res), 0).max(-1))
        floor[k] = f64((nefc + nv) * eps * np.where(sel, mag, 0).max(-1))
    has = sel.any(-1)
    settled = (F[4] == F[64]).all(-1)
    print(f"  interior rows after 64 sweeps: {int(sel.sum())} in {int(has.sum())} environments; largest residual on them after 4 sweeps: median "
          f"{np.median(slip[4][has]) if has.any() else 0:.3g}, after 64: {np.median(slip[64][has]) if has.any() else 0:.3g}; at the floor after 4: "
          f"{int((slip[4] <= floor[4])[has].sum())}, at the fixed point: {int(settled[has].sum())}; none of the three: "
          f"{np.flatnonzero(has & ~((slip[64] < slip[4]) | (slip[4] <= floor[4]) | settled)).tolist()}")
    assert has.any()
    assert ((slip[64] < slip[4]) | (slip[4] <= floor[4]) | settled)[has].all()


# ---- stopping -----------------------------------------------------------------------------------------------------------------------------------

STOP_SWEEPS = 12


@pytest.mark.parametrize("xml,ov,dtype", MODELS, ids=IDS)
def test_environments_stop_on_their_own(xml, ov, dtype):
    """``tolerance`` is the median over the environments of the reference's improvement at the fifth sweep (0 where that is not positive: then nothing stops
    early).  Nothing is compared with the reference's stopping sweep: an improvement next to the tolerance may fall on either side of it.  What holds on the
    device's own numbers: ``niter <= iterations``; ``improvement < tolerance`` wherever ``niter < iterations``; an environment's outputs are those of ``niter``
    sweeps at ``tolerance = 0``, bit for bit."""
    mc, mx, d, A, _ = passed(xml, ov, dtype, 70)
    ref, _ = reference(xml, ov, dtype, 70, False, STOP_SWEEPS)
    tol = max(float(np.median(f64(ref["improvements"][4]))), 0.0)
    res = mt.solve_noslip(mx, d, iterations=STOP_SWEEPS, tolerance=tol)
    niter = host(res.niter)
    print(f"{xml} {dict(ov)} {dtype}: tolerance {tol:.3g}; niter histogram {np.bincount(niter, minlength=STOP_SWEEPS + 1).tolist()}")
    assert (niter >= 1).all() and (niter <= STOP_SWEEPS).all()
    early = niter < STOP_SWEEPS
    assert (host(res.improvement)[early] < tol).all()
    for k in np.unique(niter):
        fixed = mt.solve_noslip(mx, d, iterations=int(k), tolerance=0.0)
        rows = torch.tensor(niter == k, device=res.niter.device)
        assert (fixed.niter[rows] == int(k)).all()  # (their earlier improvements were >= tolerance > 0: they do not stop at tolerance = 0 either)
        for a, b in zip(res, fixed):
            assert torch.equal(a[rows], b[rows]), k


# ---- bit identities ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("xml,ov,dtype", MODELS, ids=IDS)
def test_an_environment_alone_is_its_row_of_the_batch(xml, ov, dtype):
    mc, mx, d, A, f0 = passed(xml, ov, dtype, 70)
    whole = mt.solve_noslip(mx, d, iterations=7, tolerance=0.0, force0=f0)
    for e in (0, 37, 69):
        one = mt.solve_noslip(mx, d[e:e + 1], iterations=7, tolerance=0.0, force0=f0[e:e + 1])
        for a, b in zip(one, whole):
            assert torch.equal(a, b[e:e + 1])


_CUT_CHILD = r'''
import sys
sys.path.insert(0, "tests"); sys.path.insert(0, "mujoco-torch_amd"); sys.path.insert(0, "oracle")
import torch, mujoco_torch_amd as mt
import test_noslip as t
res = {}
for spec in sys.argv[2:]:
    xml, cone, dts = spec.split(":")
    mc, mx, d, A, f0 = t.passed(xml, t.ELL if cone == "1" else (), getattr(torch, dts), 70)
    out = {k: getattr(d, k) for k in ("efc_J", "efc_D", "qLD", "qacc_smooth")}  # the leaves: a difference there is forward's
    out.update(mt.solve_noslip(mx, d, iterations=7, tolerance=0.0, force0=f0)._asdict())
    res[spec] = {k: o.cpu() for k, o in out.items()}
torch.save(res, sys.argv[1])
print("ran")
'''
CUT_MODELS = (("humanoid", "0", "float64"), ("ant", "1", "float32"), ("centipede_106", "0", "float64"))


def test_a_batch_cut_into_several_launches_is_bit_identical():
    """MJH_MAX_GRID_LOG2=2 caps a launch at 4 workgroups, one environment each: 70 environments go out as 18 launches, the last one of 2, and every output must
    equal the single launch of the default bit for bit (fresh child processes: the library reads the switch once)."""
    with tempfile.TemporaryDirectory() as td:
        res = {}
        for tag, env in (("one", {}), ("cut", {"MJH_MAX_GRID_LOG2": "2"})):
            f = os.path.join(td, tag + ".pt")
            base = {k: v for k, v in os.environ.items() if k != "MJH_MAX_GRID_LOG2"}
            r = subprocess.run([sys.executable, "-c", _CUT_CHILD, f] + [":".join(c) for c in CUT_MODELS], cwd=ROOT, env=dict(base, **env), capture_output=True,
                               text=True, timeout=600)
            assert r.returncode == 0 and "ran" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
            res[tag] = torch.load(f)
    assert len(res["one"]) == len(CUT_MODELS)
    for case, outs in res["one"].items():
        assert len(outs) == 4 + 6
        for k, a in outs.items():
            assert a.shape[0] == 70 and a.any() and (a.dtype == torch.int32 or torch.isfinite(a).all()), (case, k)
            assert torch.equal(a, res["cut"][case][k]), (case, k)


# ---- the plan, the refusals, the bookkeeping -----------------------------------------------------------------------------------------------------

def test_the_large_model_stages_several_chunks_with_a_short_last_one():
    from mujoco_torch_amd import noslip
    mc = passed("centipede_106", (), F64, 1)[0]
    _, _, nefc, nv, _, ncon = sizes(mc)
    chunk, nchunk, last, lds = noslip.plan(nv, nefc, ncon, F64)
    assert nv > 32 and nchunk >= 3 and 0 < last < chunk and (nchunk - 1) * chunk + last == nefc and 64 * 1024 < lds <= 160 * 1024, (chunk, nchunk, last, lds)
    mc, _ = seeded_batch("centipede_154", {}, F64, 1)
    _, _, nefc, nv, _, ncon = sizes(mc)
    with pytest.raises(RuntimeError, match=rf"nv = {nv}, nefc = {nefc}, ncon = {ncon} .* need \d+ bytes of LDS"):
        noslip.plan(nv, nefc, ncon, F64)


def test_kernel_id_and_byte_account():
    """The kernel reports under timing id 55, one launch a call, and ``mjh_model_kernel_io`` accounts it per environment by the formula of csrc/mjh_noslip.h:
    read ``2 nefc nv + nv^2 + 4 nefc + nv`` reals (``+ 5 ncon`` with an elliptic cone), written ``nefc + 2 nv + 2`` reals and 4 bytes."""
    for xml, ov, dtype, size in (("humanoid", (), F64, 8), ("ant", ELL, F32, 4)):
        mc, mx, d, A, f0 = passed(xml, ov, dtype, 3)
        _, _, n, nv, _, ncon = sizes(mc)
        nm = native.get_native_model(mx, torch.device("cuda", 0), dtype)
        rw = (ctypes.c_int64 * 2)()
        assert nm.lib.mjh_model_kernel_io(nm.handle, 55, rw) == 0
        assert (rw[0], rw[1]) == ((2 * n * nv + nv * nv + 4 * n + nv + (5 * ncon if ov else 0)) * size, (n + 2 * nv + 2) * size + 4)
        nm.lib.mjh_debug_phase_timing(1)
        try:
            mt.solve_noslip(mx, d, iterations=3, force0=f0)
            ms, ids = (ctypes.c_float * 16)(), (ctypes.c_int * 16)()
            k = nm.lib.mjh_debug_phase_times(ms, ids, 16)
        finally:
            nm.lib.mjh_debug_phase_timing(0)
        assert [ids[i] for i in range(k)] == [55] and ms[0] > 0


def test_a_side_stream_and_untouched_inputs():
    """The call runs on the caller's stream; nothing is written to the Data or to ``force0``."""
    mc, mx, d, A, f0 = passed("ant", ELL, F32, 3)
    names = ("efc_J", "efc_D", "efc_aref", "efc_frictionloss", "qLD", "qacc_smooth", "efc_force", "qacc", "qfrc_constraint")
    before = {n: getattr(d, n).clone() for n in names}
    fr, f0c = d.contact.friction.clone(), f0.clone()
    want = mt.solve_noslip(mx, d, iterations=5, tolerance=0.0, force0=f0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = mt.solve_noslip(mx, d, iterations=5, tolerance=0.0, force0=f0)
    s.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    own = mt.solve_noslip(mx, d, iterations=5, tolerance=0.0)
    assert torch.equal(own.efc_force, mt.solve_noslip(mx, d, iterations=5, tolerance=0.0, force0=d.efc_force.clone()).efc_force)
    assert all(torch.equal(getattr(d, n), t) for n, t in before.items()) and torch.equal(d.contact.friction, fr) and torch.equal(f0, f0c)
