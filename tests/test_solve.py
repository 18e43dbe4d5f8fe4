"""``solve`` on the device (csrc/mjh_solve.h) against the numpy reference tests/_solve_ref.py -- the algorithm from its definitions, which tests/test_solve_host.py pins
on a hand-worked problem and on the recordings -- evaluated on the SAME rounded inputs: the leaves of this library's own ``forward`` on the seeded batches of
tests/_cases.py, B in {1, 3, 70}.  After ``forward`` the warm start of a Data is the pass's own solution, from which a converged model does not move: the tests that
need a solve to travel start it cold, ``qacc_warmstart = qacc_smooth``.

Models: the ant (Newton, 8 dofs: the clamped inline Cholesky), the ant with friction loss in float64 and float32 (friction rows and their linear zones, 256 rows: two
staging chunks in float64), the equality loops (``ne > 0``, 17 dofs: the ``+ 1e-10 I`` factorisation), the humanoid (CG, 27 dofs, one body of four line-search
bodies), the centipede (72 dofs: more dofs than lanes; float32 and float64, both fit the plan) and the ant with ``DisableBit.WARMSTART``.

No bound here is read off the kernel: the three rules are stated in tests/test_solve_host.py (``certificate``, ``decided``, ``CAP``) and the slack of the cost
inequalities where it is used (``cost_slack``).  The bit identities carry no tolerance.
"""
import functools

import numpy as np
import pytest
import torch

import _solve_ref as sr
import mujoco_torch_amd as mt
from _cases import F64, TOL_PRE, TOL_SOL, seeded_batch
from _util import rel_err
from test_constraint_space_host import sizes
from test_solve_host import (NOWARM, BATCHES, BODIES, CAP, IDS, INPUTS, MODELS, NEWTON, NPDT, TRAJECTORY_IDS, TRAJECTORY_MODELS, certificate, decided, f64, m_norm, reference,
                             started, trajectories, trajectory_runs)

pytestmark = pytest.mark.gpu

DEV = "cuda"
LD = np.longdouble
OUTPUTS = ("qacc", "qacc_warmstart", "qfrc_constraint", "efc_force")


def host(t):
    return t.detach().cpu().numpy()


def key(overrides):
    return tuple(sorted(overrides.items()))


@functools.lru_cache(maxsize=None)
def passed(xml, overrides, dtype, B):
    """(host model, device model, Data after forward on the device, its leaves on the host [B, ...], the same Data with a cold start): computed once and shared."""
    mc, d = seeded_batch(xml, dict(overrides), dtype, B)
    mx = mc.to(DEV)
    d = mt.forward(mx, d.to(DEV))
    _, _, nefc, nv, _ = sizes(mc)
    tail = dict(efc_J=(nefc, nv), qM=(nv, nv), qLD=(nv, nv))
    A = {n: host(getattr(d, n)).reshape((B,) + tail.get(n, (-1,))) for n in INPUTS + ("qacc",)}
    return mc, mx, d, A, d.replace(qacc_warmstart=d.qacc_smooth.clone())


def problem(mc, A, dtype=LD):
    ne_nf, floss, _, _, scale = sizes(mc)
    return sr.Problem(*(A[n] for n in INPUTS[:-1]), ne_nf, floss, scale, dtype)


def cost_slack(mc, A, x, bodies):
    """The rounding a cost the kernel reports at ``x`` after ``bodies`` bodies may carry, per environment.  The cost is a sum of ``nefc + nv`` terms, each a product of
    factors that are themselves sums with cancellation: ``jar = J x - aref`` (``nv + 1`` terms of magnitude ``j = |J| |x| + |aref|``; the row's term ``1/2 D jar^2`` then
    moves by at most ``D j`` times the error of ``jar``), ``Ma - qfrc_smooth`` (``m = |M| |x| + |qfrc_smooth|``) and ``x - qacc_smooth`` (``|x| + |qacc_smooth|``); and
    ``jar`` and ``Ma`` have been moved ``bodies`` times, one rounding each.  Hence ``(nefc + 2 nv + 4 + 4 bodies) eps S`` with
    ``S = sum_rows D j^2 + sum_dofs m (|x| + |qacc_smooth|)`` in longdouble (the linear zones' terms are smaller than the quadratic ones they replace).  An environment
    without an active row shows why the magnitudes and not the values enter: its cost at the smooth start is an exact zero and after a body the rounding of
    ``M qacc_smooth - qfrc_smooth``, 1e-22 where the terms are 1e3."""
    P = problem(mc, A)
    st = P.evaluate(x)
    ax = np.abs(st["qacc"])
    j = np.einsum("bnv,bv->bn", np.abs(P.J), ax) + np.abs(P.aref)
    m = np.einsum("bij,bj->bi", np.abs(P.M), ax) + np.abs(P.fs)
    S = (P.D * j * j).sum(-1) + (m * (ax + np.abs(P.qs))).sum(-1)
    _, _, nefc, nv, _ = sizes(mc)
    return (nefc + 2 * nv + 4 + 4 * bodies) * float(np.finfo(NPDT[mc.qpos0.dtype]).eps) * S, st


# ---- evaluation at the returned point, stopping ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("xml,overrides,dtype", MODELS, ids=IDS)
def test_the_outputs_are_the_evaluation_at_the_returned_point(xml, overrides, dtype, B):
    """``efc_force``, ``qfrc_constraint``, ``cost`` and ``grad_norm`` (on the scale of its terms) against the longdouble evaluation at the returned ``qacc`` (rule 2), for the model's own options from
    the pass's start and for three fixed bodies of either solver from the cold start; ``qacc_warmstart`` is ``qacc`` bit for bit.  Then the stopping rule of the
    model's own options: an environment that stopped early did so on its gradient or its improvement.

    Measured (one MI355X), worst error / bound over B and the runs: ant 1.9e-8, ant with friction loss 3.0e-6 (float64) / 3.6e-4 (float32), equality loops 1.9e-5,
    humanoid 2.0e-5, centipede 3.9e-6 (float64) / 8.3e-3 (float32).  Own options: the converged models stop at ``niter`` 0 or 1 of 100 (50), the humanoid runs its one body."""
    mc, mx, d, A, cold = passed(xml, key(overrides), dtype, B)
    P, Q = problem(mc, A), problem(mc, A, NPDT[dtype])
    worst = 0.0
    runs = [(d, dict()), (cold, dict(solver=mt.SolverType.CG, iterations=3, fixed_iterations=True)), (cold, dict(solver=mt.SolverType.NEWTON, iterations=3, fixed_iterations=True))]
    for data, kw in runs:
        out, st = mt.solve(mx, data, stats=True, **kw)
        assert torch.equal(out.qacc, out.qacc_warmstart) and out.qacc.data_ptr() != out.qacc_warmstart.data_ptr()
        x = host(out.qacc).reshape(B, -1)
        want, same = P.evaluate(x), Q.evaluate(x)
        got = dict(force=host(out.efc_force), qfrc=host(out.qfrc_constraint), cost=host(st.cost), grad_norm=host(st.grad_norm))
        want["grad_norm"], same["grad_norm"] = P.grad_norm(want), Q.grad_norm(same)
        # grad = Ma - qfrc_smooth - J^T force: at a point a solver returns the three terms cancel to its residual, thousands of times smaller than they are, and the
        # result of ANY evaluation in the dtype is a rounding of the terms.  As tests/test_constraint_space.py reads it at the pass's own qacc: on the scale of the
        # largest term (over the scale of grad_norm), within sqrt(nv) x the bound of an entry.
        terms = max(float(np.abs(f64(v)).max()) for v in (want["Ma"], P.fs, want["qfrc"])) / float(P.scale)
        for n in got:
            floor = (terms,) if n == "grad_norm" else ()
            e_same, e_new = rel_err(f64(same[n]), f64(want[n]), *floor), rel_err(got[n], f64(want[n]), *floor)
            bound = max(TOL_PRE[dtype] * (np.sqrt(sizes(mc)[3]) if n == "grad_norm" else 1), 4 * e_same)
            worst = max(worst, e_new / bound)
            print(f"{xml} {dtype} B={B} {kw or 'own options'}: {n}: rel_err {e_new:.3g}, numpy in the dtype {e_same:.3g}, bound {bound:.3g} ({e_new / bound:.2g} of it)")
            assert np.isfinite(e_new) and e_new <= bound, (n, kw, e_new, bound)
    print(f"  worst error / bound {worst:.3g}")
    out, st = mt.solve(mx, d, stats=True)
    iterations, tol = int(mc.opt.iterations), float(mc.opt.tolerance)
    niter, gn, imp = host(st.niter), host(st.grad_norm), host(st.improvement)
    assert st.niter.dtype == torch.int32 and (niter <= iterations).all()
    if iterations != 1:
        early = niter < iterations
        assert ((gn[early] < tol) | (imp[early] < tol)).all()
    else:
        assert (niter == 1).all()
    print(f"  own options: niter {niter.min()} .. {niter.max()} of {iterations}")


@pytest.mark.parametrize("xml,overrides,dtype", MODELS, ids=IDS)
def test_fixed_iterations_and_no_iteration(xml, overrides, dtype):
    """``fixed_iterations=True``: ``niter == iterations`` everywhere.  ``iterations = 0``: the start -- the pass's warm start, or ``qacc_smooth`` from the cold Data or with
    ``DisableBit.WARMSTART`` -- bit for bit, with its evaluation (rule 2), ``niter = 0`` and ``improvement = +inf``."""
    B = 3
    mc, mx, d, A, cold = passed(xml, key(overrides), dtype, B)
    for k in (0, 1, 4):
        for solver in (mt.SolverType.CG, mt.SolverType.NEWTON):
            _, st = mt.solve(mx, cold, True, solver=solver, iterations=k, stats=True)
            assert (st.niter == k).all()
    P, Q = problem(mc, A), problem(mc, A, NPDT[dtype])
    nowarm = bool(int(mc.opt.disableflags) & mt.DisableBit.WARMSTART)
    for data, start in ((d, "qacc_smooth" if nowarm else "qacc_warmstart"), (cold, "qacc_smooth")):
        out, st = mt.solve(mx, data, iterations=0, stats=True)
        if not nowarm and data is d:  # (the warm start is taken where it costs strictly less: checked where the two costs differ by more than their rounding)
            cw, cs = P.evaluate(A["qacc_warmstart"])["cost"], P.evaluate(A["qacc_smooth"])["cost"]
            slack = cost_slack(mc, A, A["qacc_warmstart"], 0)[0] + cost_slack(mc, A, A["qacc_smooth"], 0)[0]
            is_warm, is_smooth = (host(out.qacc) == A["qacc_warmstart"]).all(-1), (host(out.qacc) == A["qacc_smooth"]).all(-1)
            assert (is_warm | is_smooth).all() and is_warm[cw < cs - slack].all() and is_smooth[cw > cs + slack].all()
        else:
            assert torch.equal(out.qacc, getattr(data, start))
        assert not st.niter.any() and torch.isposinf(st.improvement).all()
        x = host(out.qacc)
        want, same = P.evaluate(x), Q.evaluate(x)
        for n, got in (("force", out.efc_force), ("qfrc", out.qfrc_constraint), ("cost", st.cost)):
            assert rel_err(host(got), f64(want[n])) <= max(TOL_PRE[dtype], 4 * rel_err(f64(same[n]), f64(want[n]))), n


# ---- convergence ------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def optimum(xml, overrides, dtype, B):
    """``q*`` of the device's leaves: the reference, Newton in longdouble, ``tolerance = 0``, 30 bodies of 50 line-search bodies from the smooth start."""
    mc, _, _, A, _ = passed(xml, overrides, dtype, B)
    return reference(mc, started(A, "cold"), solver=NEWTON, iterations=30, tolerance=0.0, ls_iterations=50)["qacc"]


@pytest.mark.parametrize("xml,overrides,dtype", MODELS, ids=IDS)
def test_convergence(xml, overrides, dtype):
    """``iterations = 100``, ``ls_iterations = 50``, both solvers from the cold start, B = 3 and 70: the result against the longdouble ``q*`` and CG against Newton by the
    certificate (rule 1); on the models whose own options converge, ``solve(mx, fx).qacc`` against the pass's ``fx.qacc`` by the same rule.

    Measured (one MI355X): CG takes 24 to 40 bodies on the humanoid, 10 to 29 on the equality loops, up to 52 on the centipede, Newton 1 to 6; the worst share of the
    certificate is 1.0 where no row is active (the certificate is an equality there; ant with friction loss in float32, centipede B = 70), 0.93 on the equality loops,
    0.51 on the humanoid; ``solve(mx, fx).qacc`` is ``fx.qacc`` bit for bit."""
    for B in (3, 70):
        mc, mx, d, A, cold = passed(xml, key(overrides), dtype, B)
        q = optimum(xml, key(overrides), dtype, B)
        cq = certificate(mc, A, q)[0]
        res = {}
        for solver in (mt.SolverType.CG, mt.SolverType.NEWTON):
            out, st = mt.solve(mx, cold, solver=solver, iterations=100, ls_iterations=50, stats=True)
            x = host(out.qacc)
            res[solver] = (x, certificate(mc, A, x)[0])
            dist = m_norm(A, x - q)
            ratio = float((dist / (res[solver][1] + cq)).max())
            print(f"{xml} {dtype} B={B} {solver.name}: niter {int(st.niter.min())} .. {int(st.niter.max())}, |qacc - q*|_M {float(dist.max()):.3g}, worst share of the certificate {ratio:.3g}")
            assert (dist <= res[solver][1] + cq).all()
        (xc, cc), (xn, cn) = res[mt.SolverType.CG], res[mt.SolverType.NEWTON]
        assert (m_norm(A, xc - xn) <= cc + cn).all()
        if xml in ("ant", "ant_frictionloss", "equality_loops"):
            x = host(mt.solve(mx, d).qacc)
            dist = m_norm(A, x - A["qacc"])
            print(f"  solve(mx, fx).qacc against fx.qacc: |difference|_M {float(dist.max()):.3g}")
            assert (dist <= certificate(mc, A, x)[0] + certificate(mc, A, A["qacc"])[0]).all()


# ---- trajectories -------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def references(xml, overrides, dtype, B, start, solver):
    mc, _, _, A, _ = passed(xml, overrides, dtype, B)
    return trajectories(mc, started(A, start), dtype, solver)


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("xml,overrides,dtype", TRAJECTORY_MODELS, ids=TRAJECTORY_IDS)
def test_fixed_bodies_against_the_reference(xml, overrides, dtype, B):
    """``fixed_iterations=True`` with 1, 2 and 5 bodies, both solvers from the cold start and the model's own from the pass's: ``qacc`` and ``cost`` against the longdouble
    reference within ``max(TOL_SOL, 4 x the same-dtype reference's error)`` on the decided environments (rule 3), of which at most 1/8 may be missing.

    Measured (one MI355X), worst error / bound per model: ant 0 (nothing of its pass is active), ant with friction loss 2.4e-8, equality loops 0.25, humanoid with 50
    line-search bodies 0.022 (float64) / 0.25 (float32), centipede 0.25 (float64) / 0.098 (float32); 0.25 is the kernel and the same-dtype reference carrying the same
    figure.  No environment was undecided."""
    mc, mx, d, A, cold = passed(xml, key(overrides), dtype, B)
    worst = 0.0
    for start, solver in trajectory_runs(mc):
        ld, same = references(xml, key(overrides), dtype, B, start, solver)
        for k in BODIES:
            out, st = mt.solve(mx, cold if start == "cold" else d, True, solver=solver, iterations=k, stats=True)
            assert (st.niter == k).all()
            ok = decided(ld, same, k, dtype)
            assert (~ok).sum() <= CAP * B, (start, solver, k, int((~ok).sum()))
            for n, got, hist in (("qacc", out.qacc, "qaccs"), ("cost", st.cost, "costs")):
                got = host(got).reshape(B, -1)[ok]
                want, other = f64(ld[hist][k]).reshape(B, -1)[ok], f64(same[hist][k]).reshape(B, -1)[ok]
                e_same = max([rel_err(other[i], want[i]) for i in range(len(want))], default=0.0)
                e_new = max([rel_err(got[i], want[i]) for i in range(len(want))], default=0.0)
                bound = max(TOL_SOL[dtype], 4 * e_same)
                worst = max(worst, e_new / bound)
                print(f"{xml} {dtype} B={B} {start} solver {solver} {k} bodies: {n}: rel_err {e_new:.3g}, the reference in the dtype {e_same:.3g}, bound {bound:.3g}, "
                      f"{int((~ok).sum())} undecided")
                assert np.isfinite(e_new) and e_new <= bound, (start, solver, k, n, e_new, bound)
    print(f"  worst error / bound {worst:.3g}")


# ---- the cost falls, the start is the cheaper one ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("xml,overrides,dtype", MODELS, ids=IDS)
def test_the_cost_never_rises_and_starts_at_the_cheaper_start(xml, overrides, dtype):
    """Fixed bodies 0 .. 5 of either solver from the cold start: ``cost[k + 1] <= cost[k] + slack``, the slack being the rounding of the two reported costs
    (``cost_slack``).  From the pass's Data: the cost after the model's own options is at most ``min(cost(qacc_warmstart), cost(qacc_smooth))`` plus that slack.

    Measured (one MI355X): the largest rise is 2.6e-13 in float32 and 1.7e-22 in float64 (the centipede's environments without an active row), at most 2.8e-13 of the
    slack; against the cheaper start the cost is higher by at most 24.9 on 3.5e8 (ant with friction loss, float32: 5e-4 of the slack)."""
    B = 70
    mc, mx, d, A, cold = passed(xml, key(overrides), dtype, B)
    for solver in (mt.SolverType.CG, mt.SolverType.NEWTON):
        costs, slacks = [], []
        for k in range(6):
            out, st = mt.solve(mx, cold, True, solver=solver, iterations=k, stats=True)
            costs.append(host(st.cost).astype(np.float64))
            slacks.append(f64(cost_slack(mc, A, host(out.qacc), k)[0]))
        rise = np.array([costs[k + 1] - costs[k] for k in range(5)])
        slack = np.array([slacks[k + 1] + slacks[k] for k in range(5)])
        print(f"{xml} {dtype} {solver.name}: cost {costs[0].max():.6g} -> {costs[5].max():.6g}; largest rise {rise.max():.3g}, largest rise / slack {(rise / np.maximum(slack, 1e-300)).max():.3g}")
        assert (rise <= slack).all()
    out, st = mt.solve(mx, d, stats=True)
    P = problem(mc, A)
    floor = np.minimum(P.evaluate(A["qacc_warmstart"])["cost"], P.evaluate(A["qacc_smooth"])["cost"]) if not int(mc.opt.disableflags) & mt.DisableBit.WARMSTART else P.evaluate(A["qacc_smooth"])["cost"]
    slack = cost_slack(mc, A, host(out.qacc), int(st.niter.max()))[0] + cost_slack(mc, A, A["qacc_smooth"], 0)[0]
    print(f"  own options: cost - the cheaper start's, largest {float((host(st.cost) - floor).max()):.3g} (slack {float(slack.max()):.3g})")
    assert (host(st.cost) <= floor + slack).all()


def test_a_disabled_warm_start_is_ignored():
    """``DisableBit.WARMSTART``: a deliberately better ``qacc_warmstart`` (the converged solution) changes nothing -- one body gives the bits of the run started from
    ``qacc_smooth``, and those of the model with the warm start enabled when that is handed ``qacc_smooth`` as its warm start."""
    mc, mx, d, A, cold = passed("ant_frictionloss", key({"disableflags": NOWARM}), F64, 70)
    better = mt.solve(mx, cold, iterations=100, ls_iterations=50).qacc
    P = problem(mc, A)
    assert (P.evaluate(host(better))["cost"] < P.evaluate(A["qacc_smooth"])["cost"]).all()
    got = mt.solve(mx, d.replace(qacc_warmstart=better), iterations=1)
    want = mt.solve(mx, cold, iterations=1)
    _, mw, dw, _, coldw = passed("ant_frictionloss", key({}), F64, 70)
    assert torch.equal(dw.efc_J, d.efc_J) and torch.equal(dw.qacc_smooth, d.qacc_smooth)  # (the same pass: the flag only changes the solver's start)
    warm = mt.solve(mw, coldw, iterations=1)
    for n in OUTPUTS:
        assert torch.equal(getattr(got, n), getattr(want, n)) and torch.equal(getattr(got, n), getattr(warm, n)), n
    assert not torch.equal(got.qacc, d.qacc_smooth)  # (the body moved)
    taken = mt.solve(mw, dw.replace(qacc_warmstart=better), iterations=0)
    assert torch.equal(taken.qacc, better)  # (with the warm start enabled the better start is taken)


# ---- bit identities ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("xml,overrides,dtype", MODELS, ids=IDS)
def test_bits_do_not_depend_on_the_batch_and_inputs_are_untouched(xml, overrides, dtype):
    """Rows of the B = 70 result equal the same environments run alone and as a batch of three; a second call returns the same bits; every input leaf is untouched."""
    mc, mx, d, A, cold = passed(xml, key(overrides), dtype, 70)
    for data, kw in ((d, dict()), (cold, dict(solver=mt.SolverType.CG, iterations=4)), (cold, dict(solver=mt.SolverType.NEWTON, iterations=4, fixed_iterations=True))):
        before = {n: getattr(data, n).clone() for n in INPUTS + ("qacc", "efc_force", "qfrc_constraint")}
        full, st = mt.solve(mx, data, stats=True, **kw)
        again, st2 = mt.solve(mx, data, stats=True, **kw)
        assert all(torch.equal(getattr(full, n), getattr(again, n)) for n in OUTPUTS) and all(torch.equal(a, b) for a, b in zip(st, st2))
        assert all(torch.equal(getattr(data, n), t) for n, t in before.items())
        for i, width in ((0, 1), (41, 1), (69, 1), (5, 3), (67, 3)):
            part, sp = mt.solve(mx, data[i:i + width], stats=True, **kw)
            for n in OUTPUTS:
                assert torch.equal(getattr(part, n), getattr(full, n)[i:i + width]), (n, i, width)
            assert all(torch.equal(a, b[i:i + width]) for a, b in zip(sp, st)), (i, width)
