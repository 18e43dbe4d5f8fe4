"""``solve``: the reference's constraint solver (``solver.solve``, ``_src/solver.py:244-553``: CG and Newton with an exact line search) on a caller's ``Data`` -- the solver
``step`` runs, as a function on the leaves of a finished pass.  One native launch (``mjh_solve``, ``csrc/mjh_solve.h``, whose header states the kernel, its LDS layout and
the order of every sum) on the caller's current stream.

It minimises, per environment, the cost ``constraint_update`` evaluates (``constraint_space``'s docstring): ``1/2 (M qacc - qfrc_smooth) . (qacc - qacc_smooth)`` plus the
rows' terms.  Every constraint row is a scalar row: ``opt.cone`` only changes which rows ``make_constraint`` emitted, so pyramidal and elliptic models run the same code.
The start is ``qacc_warmstart`` when its cost is strictly below that of ``qacc_smooth`` (``qacc_smooth`` otherwise, and always with ``DisableBit.WARMSTART``); one body is a
line search along ``search``, the evaluation, the gradient ``M qacc - qfrc_smooth - J^T efc_force`` and the next direction: ``-H^-1 grad`` with
``H = qM + J^T diag(D active) J`` (Newton; factored by ``math.small_cholesky``'s rule: up to 16 dofs pivots clamped at 1e-12, above ``H + 1e-10 I``) or ``-M^-1 grad``
through ``qLD`` plus the Polak-Ribiere term (CG).  ``iterations == 1`` runs one body unconditionally, ``fixed_iterations`` exactly ``iterations`` bodies of exactly
``ls_iterations`` line-search bodies; otherwise an environment stops when ``niter >= iterations``, ``improvement < tolerance`` or ``grad_norm < tolerance`` -- on its own: a
workgroup is one environment.  ``iterations = 0`` returns the chosen start with its forces.

Reads ``efc_J``, ``efc_D``, ``efc_aref``, ``efc_frictionloss``, ``qM`` (dense), ``qLD``, ``qfrc_smooth``, ``qacc_smooth`` and ``qacc_warmstart``; returns the caller's ``Data``
with ``qacc``, ``qacc_warmstart`` (the same values, distinct storage), ``qfrc_constraint`` and ``efc_force`` replaced.  ``device_put`` refuses ``opt.solver = PGS`` as before,
and so does this function.  A model whose working set does not fit a workgroup's LDS is a ``RuntimeError`` (``plan``).

Every leading dimension of a leaf is the batch (S); nothing is written to the input.  ``torch.vmap`` / ``torch.compile``: there is no operator; they raise
``NotImplementedError``.
"""

from __future__ import annotations

import math
import operator
from typing import NamedTuple

import torch

from . import _dual, native
from ._enums import DisableBit, SolverType
from ._postpass import bind, call, check_leaves, probe, refuse_tracing, require_device

_WHAT = "solve"


class SolveStats(NamedTuple):
    """What ``solve(..., stats=True)`` reports per environment; ``scale = m.stat.meaninertia * max(1, nv)``."""

    niter: torch.Tensor        # S int32: the bodies run
    cost: torch.Tensor         # S: the cost at the returned qacc
    improvement: torch.Tensor  # S: (prev_cost - cost) / scale of the last body; +inf when niter == 0
    grad_norm: torch.Tensor    # S: |grad| / scale at the returned qacc


def _solver(solver) -> SolverType:
    try:
        solver = SolverType(int(solver))
    except (TypeError, ValueError):
        raise ValueError(f"solve: solver= must be SolverType.CG or SolverType.NEWTON; got {solver!r}") from None
    if solver not in (SolverType.CG, SolverType.NEWTON):
        raise ValueError(f"solve: solver= must be SolverType.CG or SolverType.NEWTON; got {solver!r}")
    return solver


def plan(solver, nv: int, nefc: int, dtype) -> tuple[int, int, int, int]:
    """(rows of ``efc_J`` per staging step, steps, rows of the last step, bytes of LDS per workgroup) of one call: the library's own plan (``mjh_solve_plan``, a host
    computation).  The LDS holds ``nv (nv + 1) + nefc (nv | 1) + r nefc + 10 nv + 64`` reals, ``r`` = 5 (CG) or 6 (Newton); a model that exceeds a workgroup's LDS is a
    ``RuntimeError`` naming nv, nefc, the solver and the bytes."""
    solver = _solver(solver)
    return _dual.plan(_WHAT, "mjh_solve_plan", dict(solver=int(solver), nv=nv, nefc=nefc), dtype,
                      f"solver {solver.name}: two packed triangles and all nefc rows of nv | 1 reals")


def _count(name: str, value) -> int:
    try:
        value = operator.index(value)
    except TypeError:
        raise ValueError(f"solve: {name} must be an integer >= 0; got {value!r}") from None
    if value < 0 or value >= 2 ** 31:
        raise ValueError(f"solve: {name} must be an integer >= 0; got {value!r}")
    return value


def solve(m, d, fixed_iterations: bool = False, *, solver=None, iterations: int | None = None, tolerance: float | None = None, ls_iterations: int | None = None,
          ls_tolerance: float | None = None, stats: bool = False):
    """The reference's ``solve(m, d, fixed_iterations)`` on the pass in ``d``: ``d`` with ``qacc``, ``qacc_warmstart``, ``qfrc_constraint`` and ``efc_force`` replaced; the
    module's docstring has the definitions.

    ``solver`` (``SolverType.CG`` / ``NEWTON``), ``iterations``, ``tolerance``, ``ls_iterations`` and ``ls_tolerance`` default to ``m.opt``'s and override it for this call;
    ``m.opt.disableflags`` decides the warm start and the friction-loss zones.  ``stats=True`` returns ``(Data, SolveStats)``.  A model without dofs or rows makes no
    launch: ``qacc = qacc_warmstart = qacc_smooth``, no force."""
    name = _WHAT
    refuse_tracing(name, d.efc_J, d.qacc_warmstart)
    ne, nf, _, _, nefc = (int(x) for x in m.constraint_sizes_py)
    nv = int(m.nv)
    solver = _solver(m.opt.solver if solver is None else solver)
    iterations, tolerance = _dual.check_sweeps(name, int(m.opt.iterations) if iterations is None else iterations, float(m.opt.tolerance) if tolerance is None else tolerance)
    ls_iterations = _count("ls_iterations", int(m.opt.ls_iterations) if ls_iterations is None else ls_iterations)
    ls_tolerance = float(m.opt.ls_tolerance if ls_tolerance is None else ls_tolerance)
    if not ls_tolerance >= 0:
        raise ValueError(f"solve: ls_tolerance must be >= 0; got {ls_tolerance!r}")
    flags = int(m.opt.disableflags)
    tails = dict(efc_J=(nefc, nv), efc_D=(nefc,), efc_aref=(nefc,), efc_frictionloss=(nefc,), qM=(nv, nv), qLD=(nv, nv), qfrc_smooth=(nv,), qacc_smooth=(nv,),
                 qacc_warmstart=(nv,))
    leaves = {n: getattr(d, n) for n in tails}
    batch, dtype, device = probe(name, m, "efc_J", leaves["efc_J"], (nefc, nv))
    check_leaves(name, leaves, tails, batch, dtype, device, 2)
    B = int(math.prod(batch)) if batch else 1
    meaninertia = _dual.check_meaninertia(name, m)
    require_device(device)
    new = lambda *tail, dt=dtype: torch.empty(batch + tail, dtype=dt, device=device)
    if B == 0 or nv == 0 or nefc == 0:
        out = d.replace(qacc=leaves["qacc_smooth"].clone(), qacc_warmstart=leaves["qacc_smooth"].clone(), qfrc_constraint=new(nv).zero_(), efc_force=new(nefc).zero_())
        return (out, SolveStats(new(dt=torch.int32).zero_(), new().zero_(), new().fill_(math.inf), new().zero_())) if stats else out
    plan(solver, nv, nefc, dtype)  # (the refusal that names the sizes)
    outs = dict(qacc_out=new(nv), qacc_warmstart_out=new(nv), qfrc_constraint_out=new(nv), efc_force_out=new(nefc), cost=new(), improvement=new(), grad_norm=new(),
                niter=new(dt=torch.int32))
    a = native.SolveArgs(ne=ne, nf=nf, floss=int(nf > 0 and not flags & DisableBit.FRICTIONLOSS), solver=int(solver), iterations=iterations, ls_iterations=ls_iterations,
                         fixed=int(bool(fixed_iterations)), warmstart=int(not flags & DisableBit.WARMSTART), B=B, tolerance=tolerance, ls_tolerance=ls_tolerance,
                         meaninertia=meaninertia)
    bind(a, dict(leaves, **outs))
    call(name, m, "mjh_solve", a, device, dtype, what=_WHAT)
    out = d.replace(qacc=outs["qacc_out"], qacc_warmstart=outs["qacc_warmstart_out"], qfrc_constraint=outs["qfrc_constraint_out"], efc_force=outs["efc_force_out"])
    return (out, SolveStats(outs["niter"], outs["cost"], outs["improvement"], outs["grad_norm"])) if stats else out
