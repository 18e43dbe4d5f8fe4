"""``solve`` without a GPU: the tests' numpy reference (tests/_solve_ref.py, the yardstick of tests/test_solve.py) pinned on a problem worked by hand and on the recorded
solver outputs of the goldens, the condition under which tests/test_solve.py compares trajectories, the library's plan, and the public function with the launch
replaced by that reference.

The three rules of comparison (shared with tests/test_solve.py; none is read off the kernel):

1. The certificate.  The cost is convex and its Hessian is at least ``qM`` wherever it exists, so ``|x - q*|_M <= |grad(x)|_{M^-1}`` for ANY ``x`` (``q*``: the
   minimiser) and ``|x - y|_M <= |grad(x)|_{M^-1} + |grad(y)|_{M^-1}`` for any two points; both gradients are evaluated in longdouble from the inputs, ``M^-1``
   through a longdouble Cholesky factorisation of ``qM`` itself (``certificate``).
2. A formula's value at a given point: ``max(TOL_PRE[dtype], 4 x the error of the same formula in numpy in that dtype)`` by ``_util.rel_err``.
3. Trajectories: ``max(TOL_SOL[dtype], 4 x the same-dtype reference's error)`` on DECIDED environments -- those where the same-dtype reference agrees with the
   longdouble one within ``TOL_SOL[dtype]`` after that many bodies, i.e. no line-search branch was flipped by rounding (``decided``).  At most ``CAP`` = 1/8 of the
   environments of a (model, dtype, B, body count) may be undecided: asserted here for the reference alone on the stand-in's passes, and in tests/test_solve.py on its
   own inputs.

Measured here (printed by the tests).  The recorded ``qacc`` of the converged recordings against the reference's ``q*`` (Newton, longdouble, ``tolerance = 0``, 30
bodies; 40 leave ``grad_norm`` where it is): ``|x - q*|_M`` is 0.15 of the certificate on the ant with friction loss (Newton and CG; 1.9e-14 and 1.5e-14) and 0.98 on
the equality loops (1.6e-6, where ``q*`` itself keeps a ``grad_norm`` of 2.4e-9 on one environment: a step there would improve a cost of 3e5 by less than longdouble
resolves); the recorded ``efc_force`` is reproduced to 2.3e-15 by ``_util.rel_err``.  The humanoid recordings (one body): the recorded ``qacc`` costs 1.4e3 to 1.1e4
(CG) and 5.8e5 to 1.4e7 (Newton) less than the smooth start and lies at 0.98 / 0.12 of the certificate from ``q*``.
Undecided environments, over B, the starts, the solvers and the body counts 1, 2, 5: none on any model of ``TRAJECTORY_MODELS``; on the two models left out of it, up to 52 of 70 (humanoid as configured) and 70 of 70 (ant with friction loss, float32).
"""
import ctypes
import functools
import re

import numpy as np
import pytest
import torch

import _efc_ref as er
import _hostsim
import _solve_ref as sr
import mujoco_torch_amd as mt
from _cases import F32, F64, TOL_SOL, seeded_batch
from _util import rel_err
from mujoco_torch_amd import native
from mujoco_torch_amd import solver as sv
from test_abi import header_fields
from test_constraint_space_host import forwarded, recorded, sizes

LD = er.LD
NPDT = {F64: np.float64, F32: np.float32}
CAP = 1 / 8
BODIES = (1, 2, 5)
BATCHES = (1, 3, 70)
CG, NEWTON = int(mt.SolverType.CG), int(mt.SolverType.NEWTON)
NOWARM = int(mt.DisableBit.WARMSTART)
INPUTS = ("efc_J", "efc_D", "efc_aref", "efc_frictionloss", "qM", "qLD", "qfrc_smooth", "qacc_smooth", "qacc_warmstart")
# (xml, overrides, dtype) of tests/test_solve.py; the solver is the model's unless a test passes solver=
MODELS = [("ant", {}, F64), ("ant_frictionloss", {}, F64), ("ant_frictionloss", {}, F32), ("equality_loops", {}, F64), ("humanoid", {"solver": 1}, F64),
          ("centipede", {}, F32), ("centipede", {}, F64), ("ant", {"disableflags": NOWARM}, F64)]
IDS = ["ant-f64", "ant_frictionloss-f64", "ant_frictionloss-f32", "equality_loops-f64", "humanoid-f64", "centipede-f32", "centipede-f64", "ant_nowarm-f64"]
# Rule 3's models.  The humanoid as configured (one body of FOUR line-search bodies) stops its line search on a knife edge: the float64 reference alone leaves up to
# 52 of 70 environments undecided (tests/_cases.py: max_alt 0.40), and the ant with friction loss in float32 leaves every one (its qacc is rounding of forces 1e4
# times larger).  Both break the cap, so other models take their place here, as the cap is a condition: the humanoid with 50 line-search bodies (the max_alt = 0
# case of tests/_cases.py) in float64 and float32; the two stay in every other check of tests/test_solve.py.
HUMANOID_LS50 = {"solver": 1, "iterations": 100, "ls_iterations": 50}
TRAJECTORY_MODELS = [("ant", {}, F64), ("ant_frictionloss", {}, F64), ("equality_loops", {}, F64), ("humanoid", HUMANOID_LS50, F64), ("humanoid", HUMANOID_LS50, F32),
                     ("centipede", {}, F32), ("centipede", {}, F64), ("ant", {"disableflags": NOWARM}, F64)]
TRAJECTORY_IDS = ["ant-f64", "ant_frictionloss-f64", "equality_loops-f64", "humanoid_ls50-f64", "humanoid_ls50-f32", "centipede-f32", "centipede-f64", "ant_nowarm-f64"]


def trajectory_runs(m):
    """(start, solver) of the trajectories compared on a model: both solvers from the smooth start (``qacc_warmstart = qacc_smooth``: after ``forward`` the warm start is
    the pass's own solution, from which a converged model does not move), and the model's own solver from the pass's warm start."""
    return [("cold", CG), ("cold", NEWTON), ("pass", int(m.opt.solver))]


def started(A, start):
    return dict(A, qacc_warmstart=A["qacc_smooth"]) if start == "cold" else A


def f64(x):
    return np.asarray(x, dtype=np.float64)


def options(m):
    """The keyword arguments of ``_solve_ref.solve`` a model's ``opt`` implies."""
    return dict(solver=int(m.opt.solver), iterations=int(m.opt.iterations), tolerance=float(m.opt.tolerance), ls_iterations=int(m.opt.ls_iterations),
                ls_tolerance=float(m.opt.ls_tolerance), warmstart=not int(m.opt.disableflags) & mt.DisableBit.WARMSTART)


def reference(m, A, dtype=LD, **kw):
    """``_solve_ref.solve`` on the leaves ``A`` ({name: [B, ...]}) of model ``m``, its options overridden by ``kw``."""
    ne_nf, floss, _, _, scale = sizes(m)
    return sr.solve(*(A[n] for n in INPUTS), ne_nf, floss, scale, dtype=dtype, **dict(options(m), **kw))


def certificate(m, A, x):
    """``|grad(x)|_{M^-1}`` per environment, in longdouble (rule 1), and the longdouble evaluation at ``x``.  The figure includes the rounding of that evaluation
    itself, which matters where ``x`` is an optimum to the last bits (there the inequality of rule 1 is an equality when no row is quadratic: the Hessian is ``qM``):
    a component of ``grad = M x - qfrc_smooth + J^T (D (J x - aref))`` is a sum of at most ``nv + nefc + 2`` terms each of which went through at most ``nv + 2``
    roundings before, so its error is at most ``(2 nv + nefc + 4) eps_LD`` times the sum of the terms' magnitudes,
    ``mag = |M| |x| + |qfrc_smooth| + |J|^T (D (|J| |x| + |aref|))``, and ``|d grad|_{M^-1} <= |d grad|_2 / sqrt(lambda_min(M))``."""
    ne_nf, floss, nefc, nv, scale = sizes(m)
    P = sr.Problem(*(A[n] for n in INPUTS[:-1]), ne_nf, floss, scale)
    st = P.evaluate(x)
    mg = er.cholesky_solve(A["qM"], st["grad"][:, None, :])[:, 0]
    mag = np.einsum("bij,bj->bi", np.abs(P.M), np.abs(st["qacc"])) + np.abs(P.fs)
    mag = mag + np.einsum("bnv,bn->bv", np.abs(P.J), P.D * (np.einsum("bnv,bv->bn", np.abs(P.J), np.abs(st["qacc"])) + np.abs(P.aref)))
    lam = np.linalg.eigvalsh(f64(P.M)).min(-1)
    rounding = (2 * nv + nefc + 4) * np.finfo(LD).eps * np.sqrt((mag * mag).sum(-1)) / np.sqrt(lam)
    return np.sqrt((st["grad"] * mg).sum(-1)) + rounding, st


def m_norm(A, v):
    v = er.ld(v)
    return np.sqrt(np.einsum("bi,bij,bj->b", v, er.ld(A["qM"]), v))


def decided(ld, same, k, dtype):
    """The environments whose trajectory is compared after ``k`` bodies (rule 3): the same-dtype reference agrees with the longdouble one within TOL_SOL."""
    return np.array([rel_err(f64(same["qaccs"][k][i]), f64(ld["qaccs"][k][i])) <= TOL_SOL[dtype] for i in range(ld["qaccs"].shape[1])])


# ---- 1. the reference on a problem worked by hand ------------------------------------------------------------------------------------------

def hand(aref, ne=1, nf=0, fl=(0.0, 0.0)):
    """nv = 2, ``qM = qLD = I``, ``J = [[1, 0], [1, 1]]``, ``D = (1, 1)``, ``qfrc_smooth = qacc_smooth = 0``: the cost is ``1/2 |x|^2`` plus the rows' terms at
    ``jar = (x_0, x_0 + x_1) - aref``.  Row 0 is an equality row (always quadratic), row 1 unilateral; ``scale = 2``."""
    z = np.zeros((1, 2))
    A = dict(efc_J=np.array([[[1.0, 0.0], [1.0, 1.0]]]), efc_D=np.ones((1, 2)), efc_aref=np.array([aref], dtype=np.float64), efc_frictionloss=np.array([fl]),
             qM=np.eye(2)[None], qLD=np.eye(2)[None], qfrc_smooth=z, qacc_smooth=z, qacc_warmstart=z)
    return lambda **kw: sr.solve(*(A[n] for n in INPUTS), ne + nf, nf > 0, 2.0, **kw)


def test_the_reference_on_a_hand_worked_problem():
    """``aref = (2, 4)``: at ``x = 0`` ``jar = (-2, -4)``, both rows quadratic, forces ``(2, 4)``, cost ``1/2 (4 + 16) = 10``, ``grad = -J^T f = (-6, -4)``.
    With both rows quadratic the cost is ``1/2 x^T H x - (6, 4) . x + 10``, ``H = I + J^T J = [[3, 1], [1, 2]]``: minimiser ``H x = (6, 4)``, ``x = (8/5, 6/5)``,
    where ``jar = (-2/5, -6/5)`` (both still quadratic), forces ``(2/5, 6/5)``, ``J^T f = (8/5, 6/5)``, cost ``1/2 (64 + 36) / 25 + 1/2 (4 + 36) / 25 = 14/5``.

    Newton, one body: ``Mgrad = H^-1 grad = 1/5 [[2, -1], [-1, 3]] (-6, -4) = (-8/5, -6/5)``; along ``search = (8/5, 6/5)`` the rows stay quadratic up to
    ``alpha = 5/4``, so the line search sees one parabola with its minimum at ``alpha = 1``: the optimum after one body, ``improvement = (10 - 14/5) / 2 = 18/5``.
    CG, one body: ``Mgrad = grad`` (``qLD = I``), ``search = (6, 4)``, ``jv = (6, 10)``, ``d cost / d alpha = 52 alpha + 6 (6 alpha - 2) + 10 (10 alpha - 4) =
    188 alpha - 52``: ``alpha = 13/47``, ``x = (78/47, 52/47)``, ``jar = (-16/47, -58/47)`` (quadratic), cost ``10 - 1/2 52^2 / 188 = 132/47``.

    ``aref = (2, -4)``: row 1 starts and stays satisfied (``jar_1 = x_0 + x_1 + 4 > 0``): the optimum of ``1/2 |x|^2 + 1/2 (x_0 - 2)^2`` is ``x = (1, 0)``, force
    ``(1, 0)``, cost 1; Newton: ``H = diag(2, 1)``, ``grad = (-2, 0)``, one body.  Row 0 as a friction-loss row with ``fl = 1/4`` and ``aref = (2, 4)``: ``r fl = 1/4``,
    the optimum has row 0 in its linear zone, force ``(1/4, 5/4)``, ``x = J^T f = (3/2, 5/4)`` (``jar_0 = -1/2 <= -1/4``; row 1: ``f_1 = 4 - x_0 - x_1``)."""
    fifth, eps = LD(1) / 5, 8 * float(np.finfo(LD).eps)
    run = hand((2.0, 4.0))
    for solver in (CG, NEWTON):
        zero = run(solver=solver, iterations=0)
        assert zero["niter"][0] == 0 and zero["cost"][0] == 10 and np.array_equal(zero["efc_force"][0], [2, 4]) and np.array_equal(zero["qfrc_constraint"][0], [6, 4])
        assert zero["grad_norm"][0] == np.sqrt(LD(52)) / 2 and np.isposinf(zero["improvement"][0])
    one = run(solver=NEWTON, iterations=1)
    assert one["niter"][0] == 1 and np.abs(one["qacc"][0] - np.array([8 * fifth, 6 * fifth])).max() < eps and abs(one["cost"][0] - 14 * fifth) < 10 * eps
    assert np.abs(one["efc_force"][0] - np.array([2 * fifth, 6 * fifth])).max() < eps and abs(one["improvement"][0] - 18 * fifth) < 10 * eps and one["grad_norm"][0] < eps
    one = run(solver=CG, iterations=1)
    assert np.abs(one["qacc"][0] - np.array([LD(78) / 47, LD(52) / 47])).max() < eps and abs(one["cost"][0] - LD(132) / 47) < 10 * eps
    for solver in (CG, NEWTON):
        end = run(solver=solver, iterations=40, tolerance=0.0)
        assert np.abs(end["qacc"][0] - np.array([8 * fifth, 6 * fifth])).max() < 4 * eps and abs(end["cost"][0] - 14 * fifth) < 10 * eps
        assert (np.diff(f64(end["costs"][:, 0])) <= 0).all()
        stop = run(solver=solver, iterations=40, tolerance=1e-9)  # (the loop ends on its own)
        assert stop["niter"][0] < 40 and (stop["improvement"][0] < 1e-9 or stop["grad_norm"][0] < 1e-9) and np.abs(stop["qacc"][0] - end["qacc"][0]).max() < 1e-8
        fixed = run(solver=solver, iterations=7, tolerance=1e-9, fixed=True)
        assert fixed["niter"][0] == 7 and len(fixed["qaccs"]) == 8
    assert run(solver=NEWTON, iterations=40, tolerance=1e-9)["niter"][0] == 1  # (the gradient test stops Newton after the body that finds the optimum)
    sat = hand((2.0, -4.0))(solver=NEWTON, iterations=1)
    assert np.abs(sat["qacc"][0] - np.array([1, 0])).max() < eps and np.abs(sat["efc_force"][0] - np.array([1, 0])).max() < eps and abs(sat["cost"][0] - 1) < eps
    for solver in (CG, NEWTON):
        fric = hand((2.0, 4.0), ne=0, nf=1, fl=(0.25, 0.0))(solver=solver, iterations=40, tolerance=0.0)
        assert np.abs(fric["qacc"][0] - np.array([1.5, 1.25])).max() < 4 * eps and fric["efc_force"][0][0] == 0.25 and abs(fric["efc_force"][0][1] - 1.25) < 4 * eps
    # the start: a warm start is taken only when its cost is strictly lower
    ne_nf, warm = 1, np.array([[1.6, 1.2]])
    A = [np.array([[[1.0, 0.0], [1.0, 1.0]]]), np.ones((1, 2)), np.array([[2.0, 4.0]]), np.zeros((1, 2)), np.eye(2)[None], np.eye(2)[None], np.zeros((1, 2)), np.zeros((1, 2))]
    assert np.array_equal(sr.solve(*A, warm, ne_nf, False, 2.0, solver=CG, iterations=0)["qacc"], warm)
    assert not sr.solve(*A, warm, ne_nf, False, 2.0, solver=CG, iterations=0, warmstart=False)["qacc"].any()
    assert not sr.solve(*A, np.array([[9.0, 9.0]]), ne_nf, False, 2.0, solver=CG, iterations=0)["qacc"].any()


# ---- 2. the reference on the recordings ---------------------------------------------------------------------------------------------------

def recorded_inputs(r):
    return dict({n: r[n] for n in INPUTS[:-1]}, qacc_warmstart=r["qacc_smooth"])


@pytest.mark.parametrize("case", ["ant_frictionloss_newton_f64", "ant_frictionloss_cg_f64", "equality_loops_f64"])
def test_the_converged_recordings_lie_within_the_certificate_of_the_optimum(case):
    """The recorded ``qacc`` against the reference's ``q*`` (Newton in longdouble, ``tolerance = 0``, 30 bodies; ``grad_norm`` has stopped falling: 40 bodies leave
    it where it is within a factor 10) by rule 1, and the recorded ``efc_force`` as the evaluation of the recorded ``qacc`` at TOL_SOL."""
    m, r = recorded(case)
    A = recorded_inputs(r)
    ref = reference(m, A, solver=NEWTON, iterations=30, tolerance=0.0, ls_iterations=50)
    more = reference(m, A, solver=NEWTON, iterations=40, tolerance=0.0, ls_iterations=50)
    assert (f64(more["grad_norm"]) >= f64(ref["grad_norm"]) / 10).all() and f64(ref["grad_norm"]).max() < float(m.opt.tolerance)
    c_rec, st = certificate(m, A, r["qacc"])
    c_ref, _ = certificate(m, A, ref["qacc"])
    dist = m_norm(A, er.ld(r["qacc"]) - ref["qacc"])
    print(f"{case}: |qacc - q*|_M {float(dist.max()):.3g}, certificate {float((c_rec + c_ref).max()):.3g}, worst ratio {float((dist / (c_rec + c_ref)).max()):.3g}; "
          f"q* grad_norm {float(ref['grad_norm'].max()):.3g}")
    assert (dist <= c_rec + c_ref).all()
    err = max(rel_err(f64(st["force"][i]), r["efc_force"][i]) for i in range(len(dist)))
    print(f"  recorded efc_force against the evaluation of the recorded qacc: {err:.3g}")
    assert err <= TOL_SOL[F64]


@pytest.mark.parametrize("case", ["humanoid_cg_f64", "humanoid_newton_f64"])
def test_the_one_body_recordings_lower_the_cost_and_obey_the_certificate(case):
    """The humanoid is configured for ONE body: its recorded ``qacc`` is no optimum.  It must cost less than the smooth start (the start costs no more than that, and
    a body never raises the cost), and lie within rule 1 of ``q*``."""
    m, r = recorded(case)
    A = recorded_inputs(r)
    ref = reference(m, A, solver=NEWTON, iterations=30, tolerance=0.0, ls_iterations=50)
    c_rec, st = certificate(m, A, r["qacc"])
    c_ref, _ = certificate(m, A, ref["qacc"])
    dist = m_norm(A, er.ld(r["qacc"]) - ref["qacc"])
    smooth = certificate(m, A, r["qacc_smooth"])[1]["cost"]
    print(f"{case}: cost of qacc_smooth - cost of the recorded qacc {float((smooth - st['cost']).min()):.4g} .. {float((smooth - st['cost']).max()):.4g}; "
          f"|qacc - q*|_M / certificate {float((dist / (c_rec + c_ref)).max()):.3g}")
    assert (st["cost"] < smooth).all() and (ref["cost"] <= st["cost"]).all() and (dist <= c_rec + c_ref).all()


# ---- 3. the condition of rule 3, for the reference alone -------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def host_pass(xml, overrides, dtype, B):
    """(model, the leaves [B, ...] of a pass on the CPU stand-in)."""
    with pytest.MonkeyPatch.context() as mp:
        _hostsim.install(mp)
        mx, d = forwarded(xml, dtype, (B,), dict(overrides))
    _, _, nefc, nv, _ = sizes(mx)
    tail = dict(efc_J=(nefc, nv), qM=(nv, nv), qLD=(nv, nv))
    return mx, {n: getattr(d, n).detach().numpy().reshape((B,) + tail.get(n, (-1,))) for n in INPUTS}


def trajectories(m, A, dtype, solver):
    """(longdouble, same-dtype) references of max(BODIES) fixed bodies with the model's line-search options."""
    kw = dict(solver=solver, iterations=max(BODIES), fixed=True)
    return reference(m, A, **kw), reference(m, A, NPDT[dtype], **kw)


@pytest.mark.parametrize("xml,overrides,dtype", TRAJECTORY_MODELS, ids=TRAJECTORY_IDS)
def test_the_reference_alone_keeps_the_undecided_share_under_the_cap(xml, overrides, dtype):
    """Rule 3's condition on every (model, dtype, B, start, solver, body count) of tests/test_solve.py, here on the stand-in's passes of the same seeded batches."""
    for B in BATCHES:
        m, A = host_pass(xml, tuple(sorted(overrides.items())), dtype, B)
        for start, solver in trajectory_runs(m):
            ld, same = trajectories(m, started(A, start), dtype, solver)
            for k in BODIES:
                ok = decided(ld, same, k, dtype)
                print(f"{xml} {dtype} B={B} {start} solver {solver} {k} bodies: {int((~ok).sum())} of {B} undecided")
                assert (~ok).sum() <= CAP * B


def test_the_models_left_out_of_rule_3_break_its_cap():
    """Why two models of tests/test_solve.py have stand-ins in ``TRAJECTORY_MODELS``: the reference alone leaves more than 1/8 of their environments undecided."""
    for xml, overrides, dtype in (("humanoid", {"solver": 1}, F64), ("ant_frictionloss", {}, F32)):
        m, A = host_pass(xml, tuple(sorted(overrides.items())), dtype, 70)
        ld, same = trajectories(m, A, dtype, int(m.opt.solver))
        worst = max(int((~decided(ld, same, k, dtype)).sum()) for k in BODIES)
        print(f"{xml} {dtype}: up to {worst} of 70 undecided")
        assert worst > CAP * 70


# ---- 4. the plan -----------------------------------------------------------------------------------------------------------------------------

def test_the_plan_is_the_librarys():
    """(rows per staging step, steps, rows of the last step, LDS bytes): a staged row takes nv | 1 reals, every step but the last is full, and the LDS holds two
    packed triangles, all nefc rows, five reals a row (six for Newton), ten dof vectors and 64 partial sums."""
    for nv, nefc, dtype in ((27, 53, F64), (8, 256, F64), (8, 256, F32), (17, 194, F64), (72, 60, F64), (72, 60, F32), (106, 80, F32), (1, 1, F32)):
        size = 8 if dtype == F64 else 4
        for solver, rows in ((mt.SolverType.CG, 5), (mt.SolverType.NEWTON, 6)):
            chunk, nchunk, last, lds = sv.plan(solver, nv, nefc, dtype)
            assert 1 <= last <= chunk and (nchunk - 1) * chunk + last == nefc
            assert chunk == max(1, min(16 * 1024 // ((nv | 1) * size), nefc))
            assert lds == ((nv * (nv + 1) + nefc * (nv | 1) + rows * nefc + 10 * nv + 64) * size + 15) // 16 * 16 <= 160 * 1024
    assert sv.plan(CG, 8, 256, F64)[:3] == (227, 2, 29) and sv.plan(2, 72, 60, F64) == (28, 3, 4, 86240)
    with pytest.raises(RuntimeError, match=r"solver = 2, nv = 154, nefc = 100 in torch.float64 need 332592 bytes of LDS \(solver NEWTON.*\); a workgroup has 163840"):
        sv.plan(mt.SolverType.NEWTON, 154, 100, F64)
    with pytest.raises(ValueError, match="solver= must be SolverType.CG or SolverType.NEWTON"):
        sv.plan(mt.SolverType.PGS, 8, 8, F64)
    lib = native.load_library()
    out = (ctypes.c_int * 4)()
    assert lib.mjh_solve_plan(2, 154, 100, 8, out) == -12 and out[3] == 332592 and lib.mjh_solve_plan(1, -1, 1, 8, out) == -22 and lib.mjh_solve_plan(1, 1, 1, 2, out) == -22
    assert lib.mjh_solve_plan(0, 1, 1, 8, out) == -22 and lib.mjh_solve_plan(1, 128, 100, 4, out) == 0


# ---- 5. the public function on a stand-in ----------------------------------------------------------------------------------------------------------

SCALARS = ("ne", "nf", "floss", "solver", "iterations", "ls_iterations", "fixed", "warmstart", "B", "tolerance", "ls_tolerance", "meaninertia")


class StandIn:
    """``mjh_solve`` of the CPU stand-in library: the numpy reference, in the model's dtype, on the host pointers it is handed."""

    def __init__(self):
        self.calls = []

    def install(self, monkeypatch):
        _hostsim.install(monkeypatch)
        monkeypatch.setattr(_hostsim._Lib, "mjh_solve", self, raising=False)
        return self

    def __get__(self, lib, owner=None):
        return lambda *args: self.run(lib, *args)

    def run(self, lib, handle, args, stream):
        a = args._obj
        nv, n, B = int(lib.o.desc.nv), int(lib.o.desc.nefc), int(a.B)
        ct, dt = (ctypes.c_double, np.float64) if lib.o.dt == 0 else (ctypes.c_float, np.float32)
        view = lambda p, count, c=ct: np.ctypeslib.as_array((c * count).from_address(p))
        leaf = lambda name, *shape: view(getattr(a, name), B * int(np.prod(shape))).reshape((B,) + shape)
        put = lambda name, value, c=ct, t=dt: view(getattr(a, name), value.size, c).__setitem__(slice(None), np.asarray(value, dtype=t).reshape(-1))
        self.calls.append({k: getattr(a, k) for k in SCALARS})
        out = sr.solve(leaf("efc_J", n, nv), leaf("efc_D", n), leaf("efc_aref", n), leaf("efc_frictionloss", n), leaf("qM", nv, nv), leaf("qLD", nv, nv),
                       leaf("qfrc_smooth", nv), leaf("qacc_smooth", nv), leaf("qacc_warmstart", nv), a.ne + a.nf, bool(a.floss), a.meaninertia * max(1, nv), int(a.solver),
                       int(a.iterations), a.tolerance, int(a.ls_iterations), a.ls_tolerance, fixed=bool(a.fixed), warmstart=bool(a.warmstart), dtype=dt)
        for name, key in (("qacc_out", "qacc"), ("qacc_warmstart_out", "qacc"), ("qfrc_constraint_out", "qfrc_constraint"), ("efc_force_out", "efc_force"),
                          ("cost", "cost"), ("improvement", "improvement"), ("grad_norm", "grad_norm")):
            put(name, out[key])
        put("niter", out["niter"], ctypes.c_int32, np.int32)
        return 0


@pytest.fixture
def stand_in(monkeypatch):
    return StandIn().install(monkeypatch)


def leaves_of(mx, d, B):
    _, _, nefc, nv, _ = sizes(mx)
    tail = dict(efc_J=(nefc, nv), qM=(nv, nv), qLD=(nv, nv))
    return {n: getattr(d, n).detach().numpy().reshape((B,) + tail.get(n, (-1,))) for n in INPUTS}


def test_the_function_and_the_entry_point_are_public():
    assert callable(mt.solve) and mt.SolveStats._fields == ("niter", "cost", "improvement", "grad_norm") and mt.solver.solve is mt.solve
    assert native.ABI_VERSION >= 26
    text = open(native.HEADER).read()
    assert re.search(r"int mjh_solve\(const mjhModel\* m, const mjhSolveArgs\* args, void\* hip_stream\);", text)
    assert re.search(r"int mjh_solve_plan\(int solver, int nv, int nefc, int real_bytes, int\* chunk_nchunk_last_lds\);", text)
    assert re.search(r"#define MJH_KERNEL_SOLVE 56\b", text)
    assert list(native.SolveArgs._fields_) == header_fields(text, "mjhSolveArgs")
    assert len(native.ARGS) == 6 and "mjh_solve" not in native.ARGS  # (bound beside the table, like mjh_pgs)
    lib = native.load_library()
    assert lib.mjh_solve.argtypes[1]._type_ is native.SolveArgs and "``solve``" in mt.__doc__ and "solve" in mt.__doc__
    usage = open(native.LIB_PATH.replace("libmjhip.so", "resource_usage.txt")).read().splitlines()
    mine = [u for u in usage if "mjh_solve_kernel" in u]
    assert len(mine) == 2 and all("ScratchSize [bytes/lane]: 0" in u for u in mine)  # (no scratch memory, float64 and float32)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("batch", [(), (3,), (2, 2)], ids=["unbatched", "b3", "b2x2"])
def test_the_function_returns_the_reference(stand_in, batch, dtype):
    mx, d = forwarded("ant_frictionloss", dtype, batch)
    ne_nf, floss, nefc, nv, _ = sizes(mx)
    ne, nf = (int(x) for x in mx.constraint_sizes_py[:2])
    B = int(np.prod(batch)) if batch else 1
    before = {n: getattr(d, n).clone() for n in INPUTS + ("efc_force", "qacc", "qfrc_constraint")}
    out = mt.solve(mx, d)
    assert isinstance(out, type(d)) and tuple(out.batch_size) == tuple(d.batch_size)
    defaults = dict(ne=ne, nf=nf, floss=1, solver=int(mx.opt.solver), iterations=int(mx.opt.iterations), ls_iterations=int(mx.opt.ls_iterations), fixed=0, warmstart=1, B=B,
                    tolerance=float(mx.opt.tolerance), ls_tolerance=float(mx.opt.ls_tolerance), meaninertia=float(mx.stat.meaninertia))
    assert stand_in.calls[-1] == defaults and floss and nf > 0
    A = leaves_of(mx, d, B)
    want = reference(mx, A, NPDT[dtype])
    shapes = dict(qacc=batch + (nv,), qacc_warmstart=batch + (nv,), qfrc_constraint=batch + (nv,), efc_force=batch + (nefc,))
    for n, s in shapes.items():
        got = getattr(out, n)
        assert tuple(got.shape) == s and got.dtype == dtype, n
        assert np.array_equal(got.numpy().reshape(B, -1), want["qacc" if n == "qacc_warmstart" else n]), n
    assert out.qacc.data_ptr() != out.qacc_warmstart.data_ptr() and torch.equal(out.qacc, out.qacc_warmstart)
    assert all(torch.equal(getattr(d, n), t) for n, t in before.items())  # nothing is written to d
    assert all(getattr(out, n).data_ptr() == getattr(d, n).data_ptr() for n in ("qpos", "qvel", "efc_J", "qM"))  # every other leaf is the caller's
    # stats, the positional drop-in and every keyword
    out2, st = mt.solve(mx, d, stats=True)
    assert isinstance(st, mt.SolveStats) and torch.equal(out2.qacc, out.qacc)
    for n in st._fields:
        got = getattr(st, n)
        assert tuple(got.shape) == batch and got.dtype == (torch.int32 if n == "niter" else dtype), n
        assert np.array_equal(got.numpy().reshape(B), np.asarray(want[n]).astype(got.numpy().dtype)), n
    mt.solve(mx, d, True)
    assert stand_in.calls[-1] == dict(defaults, fixed=1)
    mt.solve(mx, d, solver=mt.SolverType.CG, iterations=3, tolerance=1e-5, ls_iterations=7, ls_tolerance=0.25)
    assert stand_in.calls[-1] == dict(defaults, solver=CG, iterations=3, tolerance=1e-5, ls_iterations=7, ls_tolerance=0.25)
    zero, st = mt.solve(mx, d, iterations=0, stats=True)
    assert stand_in.calls[-1]["iterations"] == 0 and not st.niter.any() and torch.isposinf(st.improvement).all()


def test_the_flags_follow_the_models_disable_bits(stand_in):
    mx, d = forwarded("ant_frictionloss", F64, (2,), {"disableflags": int(mt.DisableBit.WARMSTART)})
    better = mt.solve(mx, d, iterations=30).qacc
    out = mt.solve(mx, d.replace(qacc_warmstart=better), iterations=0)
    assert stand_in.calls[-1]["warmstart"] == 0 and stand_in.calls[-1]["floss"] == 1
    assert torch.equal(out.qacc, d.qacc_smooth)  # (the better warm start is ignored)
    mx, d = forwarded("ant_frictionloss", F64, (2,), {"disableflags": int(mt.DisableBit.FRICTIONLOSS)})
    mt.solve(mx, d)
    assert stand_in.calls[-1]["warmstart"] == 1 and stand_in.calls[-1]["floss"] == 0
    mx, d = forwarded("ant", F64, (2,))
    mt.solve(mx, d)
    assert stand_in.calls[-1]["floss"] == 0 and stand_in.calls[-1]["nf"] == 0  # (no friction rows: no linear zones)


def test_the_output_of_step_is_valid_input_and_a_fixed_point(stand_in):
    """The leaves ``step`` integrated: its ``qacc`` is the warm start now, and on the ant with friction loss (a converged Newton solve) solving again stays within the
    certificate of it (rule 1)."""
    mx, d = seeded_batch("ant_frictionloss", {}, F64, 2)
    d = mt.step(mx, d)
    out = mt.solve(mx, d.replace(qacc_warmstart=d.qacc))
    A = leaves_of(mx, d, 2)
    c0, c1 = certificate(mx, A, d.qacc.numpy())[0], certificate(mx, A, out.qacc.numpy())[0]
    assert (m_norm(A, out.qacc.numpy() - d.qacc.numpy()) <= c0 + c1).all()


def test_empty_cases_are_answered_on_the_host(stand_in):
    mx, d = forwarded("ant_frictionloss", F64, (3,))
    _, _, nefc, nv, _ = sizes(mx)
    n0 = len(stand_in.calls)
    out, st = mt.solve(mx, d[:0], stats=True)
    assert tuple(out.efc_force.shape) == (0, nefc) and tuple(out.qacc.shape) == (0, nv) and tuple(st.cost.shape) == (0,) and st.niter.dtype == torch.int32
    mx, d = forwarded("humanoid", F64, (3,), {"disableflags": 1})
    assert sizes(mx)[2] == 0
    out, st = mt.solve(mx, d, stats=True)
    assert tuple(out.efc_force.shape) == (3, 0) and tuple(out.qfrc_constraint.shape) == (3, int(mx.nv)) and not out.qfrc_constraint.any()
    assert torch.equal(out.qacc, d.qacc_smooth) and torch.equal(out.qacc_warmstart, d.qacc_smooth)
    assert len({out.qacc.data_ptr(), out.qacc_warmstart.data_ptr(), d.qacc_smooth.data_ptr()}) == 3
    assert not st.cost.any() and not st.grad_norm.any() and not st.niter.any() and torch.isposinf(st.improvement).all()
    assert len(stand_in.calls) == n0


def test_refusals_come_before_any_call(stand_in, monkeypatch):
    mx, d = forwarded("ant_frictionloss", F64, (3,))
    n0 = len(stand_in.calls)
    bad = [
        (ValueError, "solver= must be SolverType.CG or SolverType.NEWTON", lambda: mt.solve(mx, d, solver=mt.SolverType.PGS)),
        (ValueError, "solver= must be SolverType.CG or SolverType.NEWTON", lambda: mt.solve(mx, d, solver="newton")),
        (ValueError, "solver= must be SolverType.CG or SolverType.NEWTON", lambda: mt.solve(mx, d, solver=3)),
        (ValueError, "iterations must be an integer >= 0", lambda: mt.solve(mx, d, iterations=-1)),
        (ValueError, "iterations must be an integer >= 0", lambda: mt.solve(mx, d, iterations=2.5)),
        (ValueError, "ls_iterations must be an integer >= 0", lambda: mt.solve(mx, d, ls_iterations=-1)),
        (ValueError, "tolerance must be >= 0", lambda: mt.solve(mx, d, tolerance=-1e-9)),
        (ValueError, "tolerance must be >= 0", lambda: mt.solve(mx, d, tolerance=float("nan"))),
        (ValueError, "ls_tolerance must be >= 0", lambda: mt.solve(mx, d, ls_tolerance=-1.0)),
        (ValueError, "efc_J has shape", lambda: mt.solve(mx, d.replace(efc_J=d.efc_J[:, :-1]))),
        (ValueError, "efc_D", lambda: mt.solve(mx, d.replace(efc_D=d.efc_D[:1]))),
        (ValueError, "qLD", lambda: mt.solve(mx, d.replace(qLD=d.qLD.float()))),
        (ValueError, "qacc_warmstart", lambda: mt.solve(mx, d.replace(qacc_warmstart=d.qacc_warmstart[:, :-1]))),
        (ValueError, "dtype|float32", lambda: mt.solve(mx, d.to(F32))),
        (ValueError, "meaninertia", lambda: mt.solve(mx.replace(stat=mx.stat.replace(meaninertia=0.0)), d)),
        (NotImplementedError, "solve cannot be used under torch.vmap", lambda: torch.vmap(lambda x: mt.solve(mx, d.replace(qacc_warmstart=x)).qacc)(torch.zeros(2, 3, int(mx.nv), dtype=F64))),
    ]
    for exc, match, run in bad:
        with pytest.raises(exc, match=match):
            run()
    with pytest.raises(Exception, match="solve cannot be used under torch.vmap / torch.compile"):
        torch.compile(lambda x: mt.solve(mx, d.replace(qacc_warmstart=x)).qacc, backend="eager", fullgraph=True)(d.qacc_warmstart)
    with pytest.raises(NotImplementedError, match="solver PGS not implemented"):  # device_put refuses opt.solver = PGS as before
        seeded_batch("ant", {"solver": 0}, F64, 1)
    # a model that does not fit: the library's plan, named sizes
    monkeypatch.setattr(sv, "plan", lambda solver, nv, nefc, dtype: sv._dual.plan("solve", "mjh_solve_plan", dict(solver=int(solver), nv=154, nefc=100), dtype, "x"))
    with pytest.raises(RuntimeError, match=r"solve: solver = 2, nv = 154, nefc = 100 in torch.float64 need 332592 bytes of LDS"):
        mt.solve(mx, d)
    assert len(stand_in.calls) == n0


def test_without_the_stand_in_cpu_data_is_refused(monkeypatch):
    _hostsim.install(monkeypatch)
    mx, d = forwarded("ant_frictionloss", F64, (2,))
    monkeypatch.undo()
    with pytest.raises(RuntimeError, match="HIP device"):
        mt.solve(mx, d)


def test_a_library_from_before_the_function_is_named(monkeypatch):
    _hostsim.install(monkeypatch)  # (its library has no mjh_solve)
    mx, d = forwarded("ant_frictionloss", F64, (2,))
    with pytest.raises(RuntimeError, match=r"predates solve \(no mjh_solve\): rebuild the library"):
        mt.solve(mx, d)
