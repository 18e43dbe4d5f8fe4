"""``solve_noslip``: the no-slip friction post-solver on a finished pass -- MuJoCo's ``mj_solNoSlip`` (``noslip_iterations``), which the reference does not have.
The soft model's regulariser ``R`` lets friction rows slip even inside the cone; this is a Gauss-Seidel pass AFTER the main solver, on the unregularised matrix
``A = J M^-1 J^T`` and over the friction dimensions only: the normal forces stay exactly as the main solver left them.  One native launch (``mjh_noslip``,
``csrc/mjh_noslip.h``, whose header states the kernel) on the caller's current stream.

For one environment, with ``W = (L^-1 J^T)^T`` (``L = qLD``), ``y = sum_j f_j w_j``, ``b = J qacc_smooth - efc_aref`` and ``R = 1 / efc_D`` where ``efc_D > 0`` else
0 as ``solve_pgs`` defines them: ``A_ij = w_i . w_j`` (no ``R``), the row residual is ``res_i = w_i . y + b_i``, ``scale = 1 / (m.stat.meaninertia * max(1, nv))``,
``MINVAL = 1e-15``.  The start ``force0`` (default ``d.efc_force``) is NOT projected.  One sweep starts with ``improvement = 0`` -- the first sweep alone with
``1/2 sum_i R_i f_i^2``, the cost of dropping the regulariser -- and visits

1. the friction-loss rows ``ne <= i < ne + nf``: a row with ``A_ii < MINVAL`` is skipped; ``f_i <- clamp(f_i - res_i / A_ii, +-efc_frictionloss_i)``;
   ``improvement -= delta (1/2 delta A_ii + res_i)``;
2. every contact of ``condim > 1`` in slot order (``m.tables.con_dim`` / ``con_efc_address``, ``opt.cone``), block by block; ``A_c`` is the block of ``A``,
   ``bc = res - A_c f_old``:

   * a pyramidal contact, each of its ``dim - 1`` pairs of opposing edges ``(j, j + 1)`` in turn: ``mid = (f_j + f_j+1) / 2``,
     ``K1 = A_00 + A_11 - A_01 - A_10``, ``K0 = mid (A_00 - A_11) + bc_0 - bc_1``; ``K1 < MINVAL``: both become ``mid``; otherwise ``yy = clamp(-K0 / K1, +-mid)``,
     ``f_j = mid + yy``, ``f_j+1 = mid - yy``: the pair's sum, and so the contact's normal force, is kept;
   * an elliptic contact, its ``dim - 1`` friction rows (the normal row ``i`` is not touched): ``f_i < MINVAL``: they become 0; otherwise
     ``v = argmin 1/2 v^T A_c v + v . bc`` subject to ``sum_k (v_k / mu_k)^2 <= f_i^2``, ``mu = d.contact.friction[slot, :dim - 1]``.  With ``v_k = mu_k u_k``
     (``A_s``, ``b_s``): Newton on the multiplier ``lambda >= 0`` of ``|u|^2 <= f_i^2`` from 0, ``u = -(A_s + lambda I)^-1 b_s``, until ``|u|^2 <= f_i^2``, or the
     step is ``<= 0``, or it no longer changes ``lambda``; 30 factorisations at most; a pivot of ``A_s + lambda I`` that is not positive and finite gives
     ``v = 0``; with the constraint active (``lambda > 0``) ``v`` is rescaled onto the surface, ``v *= f_i / sqrt(sum (v_k / mu_k)^2)``;

   after the block ``change = 1/2 delta^T A_c delta + delta . res``; ``change > 1e-10``: the block is put back and ``change = 0``; ``improvement -= change``;
3. no other row: equality rows, limit rows, frictionless contact rows and elliptic normals are returned bit for bit.

After the sweep ``improvement *= scale`` and ``niter += 1``; an environment stops when ``improvement < tolerance`` or ``niter == iterations``.
``cost = 1/2 y . y + f . b`` (no ``R`` term), ``qfrc_constraint = J^T f``, ``qacc = qacc_smooth + L^-T y``.

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

_WHAT = "solve_noslip"
NOSLIP_TOLERANCE = 1e-6  # MuJoCo's default opt.noslip_tolerance


class NoslipResult(NamedTuple):
    """``solve_noslip``'s result."""

    efc_force: torch.Tensor        # S + (nefc,): the start with its friction dimensions updated; every other row the same bits
    qfrc_constraint: torch.Tensor  # S + (nv,) = J^T efc_force
    qacc: torch.Tensor             # S + (nv,) = qacc_smooth + (L L^T)^-1 J^T efc_force
    cost: torch.Tensor             # S: 1/2 f^T A f + f^T b, the dual cost without the regulariser
    improvement: torch.Tensor      # S: the scaled improvement of the last sweep (0 without one)
    niter: torch.Tensor            # S int32: the sweeps run


def plan(nv: int, nefc: int, ncon: int, dtype) -> tuple[int, int, int, int]:
    """(rows of ``efc_J`` per staging step, steps, rows of the last step, bytes of LDS per workgroup) of one call: the library's own plan (``mjh_noslip_plan``, a
    host computation).  A model whose ``qLD`` triangle, ``nefc`` rows of ``nv | 1`` reals and 22 reals a contact slot exceed a workgroup's LDS is a
    ``RuntimeError`` naming the sizes."""
    return _dual.plan(_WHAT, "mjh_noslip_plan", dict(nv=nv, nefc=nefc, ncon=ncon), dtype,
                      "the qLD triangle, all nefc rows of nv | 1 reals and 22 reals a contact slot")


def solve_noslip(m, d, *, iterations: int | None = None, tolerance: float | None = None, force0: torch.Tensor | None = None) -> NoslipResult:
    """The no-slip friction post-solver on the pass in ``d`` (MuJoCo's ``mj_solNoSlip``): a ``NoslipResult``; the module's docstring has the definitions.

    Reads ``efc_J``, ``efc_D``, ``efc_aref``, ``efc_frictionloss``, ``qLD``, ``qacc_smooth``, ``efc_force`` and ``contact.friction``: the output of ``forward`` or
    ``step`` as it is.  ``iterations`` bounds the sweeps (default ``m.opt.noslip_iterations`` where the Model carries it; otherwise it must be given);
    ``tolerance`` (default 1e-6, MuJoCo's ``noslip_tolerance``) stops an environment once a sweep's scaled improvement falls below it.  ``force0``:
    ``S + (nefc,)`` or ``(nefc,)`` (shared), default ``d.efc_force``; it is not projected, and ``iterations=0`` returns it unchanged with the
    ``qfrc_constraint``, ``qacc`` and ``cost`` that belong to it.  A model that does not fit a workgroup's LDS is a ``RuntimeError`` naming the sizes
    (``noslip.plan``)."""
    name = "solve_noslip"
    refuse_tracing(name, d.efc_J, force0)
    ne, nf, _, ncon, nefc = (int(x) for x in m.constraint_sizes_py)
    nv = int(m.nv)
    if iterations is None:
        iterations = getattr(m.opt, "noslip_iterations", None)
        if iterations is None:
            raise ValueError(f"{name}: iterations must be given: this Model's options carry no noslip_iterations to default to")
    tolerance = NOSLIP_TOLERANCE if tolerance is None else tolerance
    iterations, tolerance = _dual.check_sweeps(name, iterations, tolerance)
    dims = np.asarray(m.tables.con_dim)[:ncon]
    odd = sorted(set(int(x) for x in dims if int(x) not in (1, 3, 4, 6)))
    if odd:
        raise ValueError(f"{name}: contacts of condim {odd}: the friction blocks are defined for condim 1, 3, 4 and 6")
    elliptic = int(m.opt.cone) == ConeType.ELLIPTIC
    tails = dict(efc_J=(nefc, nv), efc_D=(nefc,), efc_aref=(nefc,), efc_frictionloss=(nefc,), qLD=(nv, nv), qacc_smooth=(nv,), efc_force=(nefc,))
    leaves = {n: getattr(d, n) for n in tails}
    batch, dtype, device = probe(name, m, "efc_J", leaves["efc_J"], (nefc, nv))
    if elliptic and ncon:
        tails["contact_friction"] = (ncon, 5)
        leaves["contact_friction"] = d.contact.friction
    check_leaves(name, leaves, tails, batch, dtype, device, 2)
    B = int(math.prod(batch)) if batch else 1
    stride = nefc if batch else 0
    if force0 is not None:
        stride = _dual.check_force0(name, force0, batch, nefc, dtype, device)
    meaninertia = _dual.check_meaninertia(name, m)
    require_device(device)
    outs = _dual.new_outputs(batch, nefc, nv, dtype, device)
    if B == 0 or nv == 0 or nefc == 0:  # (no rows or no dofs: no force, qacc is qacc_smooth; without dofs J is empty and the rows are untouched)
        for t in outs.values():
            t.zero_()
        if nv > 0:
            outs["qacc"] = leaves["qacc_smooth"].clone()
        if nefc > 0 and B > 0:
            outs["efc_force"] = (leaves["efc_force"] if force0 is None else force0.expand(batch + (nefc,))).clone()
        return NoslipResult(**outs)
    plan(nv, nefc, ncon, dtype)  # (the refusal that names the sizes)
    a = native.NoslipArgs(ne=ne, nf=nf, iterations=iterations, B=B, meaninertia=meaninertia, tolerance=tolerance, force0_env=stride)
    tensors = {n: t for n, t in leaves.items() if n != "efc_force"}
    tensors["force0"] = leaves["efc_force"] if force0 is None else force0
    tensors.update(outs)
    bind(a, tensors)
    call(name, m, "mjh_noslip", a, device, dtype, what=_WHAT)
    return NoslipResult(**outs)
