"""``solve_pgs``: projected Gauss-Seidel on the dual problem of a finished pass -- MuJoCo's third solver (``mj_solPGS``) for rows of dimension one, which the
reference (CG and Newton alone) does not have.  One native launch (``mjh_pgs``, ``csrc/mjh_pgs.h``, whose header states the kernel) on the caller's current stream.

For one environment, with ``AR``, ``b`` and ``R`` as ``constraint_space`` defines them (``AR = J (L L^T)^-1 J^T + diag(R)``, ``L = qLD``, ``R = 1 / efc_D`` where
``efc_D > 0`` else 0, ``b = J qacc_smooth - efc_aref``) and ne, nf the model's equality and friction row counts, the solver minimises the dual cost
``1/2 f^T AR f + f^T b`` over the feasible set

* rows ``i < ne``: free;  rows ``ne <= i < ne + nf``: ``|f_i| <= efc_frictionloss_i``;  every later row (limits, frictionless and pyramidal contact rows): ``f_i >= 0``.

``force0`` (default zeros) is projected onto that set.  One sweep visits the rows in order, starting with ``improvement = 0``:
``res = sum_j AR_ij f_j + b_i``; a row with ``AR_ii <= 0`` is skipped; ``f_i <- project_i(f_i - res / AR_ii)``; with ``delta`` the change,
``improvement -= delta (1/2 delta AR_ii + res)``.  After the sweep ``improvement *= 1 / (m.stat.meaninertia * max(1, nv))`` and ``niter += 1``; an environment
stops when ``improvement < tolerance`` or ``niter == iterations``.  The kernel never forms ``AR``: with ``W = (L^-1 J^T)^T`` and ``y = sum_j f_j w_j`` kept on chip,
row ``i`` of ``AR f`` is ``w_i . y + R_i f_i``.

Rows of inactive contacts carry ``J = 0`` and ``b = 0``: they keep ``f = 0``.  ``opt.cone == ELLIPTIC`` with a contact of ``condim > 1`` is refused
(``NotImplementedError``): such rows need a cone projection; a frictionless elliptic model has rows of dimension one only and is served.  ``device_put`` refuses
``opt.solver = PGS`` as before: the step stays CG / Newton, this is a function on its output.

Every leading dimension of a leaf is the batch (S); nothing is written to the input.  ``torch.vmap`` / ``torch.compile``: there is no operator; they raise
``NotImplementedError``.
"""

from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np
import torch

from . import _dual, native
from ._enums import ConeType
from ._postpass import bind, call, check_leaves, probe, refuse_tracing, require_device

_WHAT = "solve_pgs"


class PGSResult(NamedTuple):
    """``solve_pgs``'s result."""

    efc_force: torch.Tensor        # S + (nefc,): dual feasible after every sweep
    qfrc_constraint: torch.Tensor  # S + (nv,) = J^T efc_force
    qacc: torch.Tensor             # S + (nv,) = qacc_smooth + (L L^T)^-1 J^T efc_force
    cost: torch.Tensor             # S: the dual cost 1/2 f^T AR f + f^T b
    improvement: torch.Tensor      # S: the scaled improvement of the last sweep (0 without one)
    niter: torch.Tensor            # S int32: the sweeps run


def plan(nv: int, nefc: int, dtype) -> tuple[int, int, int, int]:
    """(rows of ``efc_J`` per staging step, steps, rows of the last step, bytes of LDS per workgroup) of one call: the library's own plan (``mjh_pgs_plan``, a
    host computation).  A model whose ``qLD`` triangle and ``nefc`` rows of ``nv | 1`` reals exceed a workgroup's LDS is a ``RuntimeError`` naming the sizes."""
    return _dual.plan(_WHAT, "mjh_pgs_plan", dict(nv=nv, nefc=nefc), dtype, "the qLD triangle and all nefc rows of nv | 1 reals")


def _refuse_elliptic(m):
    if int(m.opt.cone) != ConeType.ELLIPTIC:
        return
    ncon = int(m.constraint_sizes_py[3])
    dims = np.asarray(m.tables.con_dim)[:ncon]
    if (dims > 1).any():
        raise NotImplementedError(f"solve_pgs: opt.cone is ELLIPTIC and the model has contacts of condim {sorted(set(int(x) for x in dims if x > 1))}: their rows "
                                  "need a cone projection this solver does not have (pyramidal cones and frictionless contacts are served)")


def solve_pgs(m, d, *, iterations: int | None = None, tolerance: float | None = None, force0: torch.Tensor | None = None) -> PGSResult:
    """Projected Gauss-Seidel on the dual problem of the pass in ``d`` (MuJoCo's ``mj_solPGS`` for rows of dimension one): a ``PGSResult``; the module's
    docstring has the definitions.

    Reads ``efc_J``, ``efc_D``, ``efc_aref``, ``efc_frictionloss``, ``qLD`` and ``qacc_smooth``: the output of ``forward`` or ``step`` as it is.  ``iterations``
    (default ``m.opt.iterations``) bounds the sweeps; ``tolerance`` (default ``m.opt.tolerance``) stops an environment once a sweep's scaled improvement falls
    below it; ``iterations=0`` returns the projected ``force0`` with ``niter = 0`` and ``improvement = 0``.  ``force0``: ``S + (nefc,)`` or ``(nefc,)`` (shared),
    default zeros.  A model that does not fit a workgroup's LDS is a ``RuntimeError`` naming the sizes (``pgs.plan``)."""
    name = "solve_pgs"
    refuse_tracing(name, d.efc_J, force0)
    ne, nf, _, _, nefc = (int(x) for x in m.constraint_sizes_py)
    nv = int(m.nv)
    iterations = int(m.opt.iterations) if iterations is None else iterations
    tolerance = float(m.opt.tolerance) if tolerance is None else tolerance
    iterations, tolerance = _dual.check_sweeps(name, iterations, tolerance)
    _refuse_elliptic(m)
    tails = dict(efc_J=(nefc, nv), efc_D=(nefc,), efc_aref=(nefc,), efc_frictionloss=(nefc,), qLD=(nv, nv), qacc_smooth=(nv,))
    leaves = {n: getattr(d, n) for n in tails}
    batch, dtype, device = probe(name, m, "efc_J", leaves["efc_J"], (nefc, nv))
    check_leaves(name, leaves, tails, batch, dtype, device, 2)
    B = int(math.prod(batch)) if batch else 1
    stride = 0
    if force0 is not None:
        stride = _dual.check_force0(name, force0, batch, nefc, dtype, device)
    meaninertia = _dual.check_meaninertia(name, m)
    require_device(device)
    outs = _dual.new_outputs(batch, nefc, nv, dtype, device)
    if B == 0 or nv == 0 or nefc == 0:  # (no rows or no dofs: no force, qacc is qacc_smooth; without dofs J is empty and the rows are untouched zeros)
        for t in outs.values():
            t.zero_()
        if nv > 0:
            outs["qacc"] = leaves["qacc_smooth"].clone()
        return PGSResult(**outs)
    plan(nv, nefc, dtype)  # (the refusal that names the sizes)
    a = native.PgsArgs(ne=ne, nf=nf, iterations=iterations, B=B, meaninertia=meaninertia, tolerance=tolerance, force0_env=stride)
    tensors = dict(leaves, **outs)
    if force0 is not None:
        tensors["force0"] = force0
    bind(a, tensors)
    call(name, m, "mjh_pgs", a, device, dtype, what=_WHAT)
    return PGSResult(**outs)
