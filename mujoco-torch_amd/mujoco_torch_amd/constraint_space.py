"""The constraint problem of a finished pass in constraint space -- MuJoCo's ``mj_mulJacVec``, ``mj_mulJacTVec`` and ``mj_constraintUpdate``, and the Delassus
matrix ``efc_AR`` every dual method starts from -- by the definitions of the reference's solver (``_src/solver.py:293-357``, ``501-508``).  Each call is one
native launch (``mjh_constraint_space``, ``csrc/mjh_efc.h``, whose header states the kernels) on the caller's current stream.

For one environment, with ``J = efc_J`` (nefc x nv), ``D = efc_D``, ``fl = efc_frictionloss`` and ne, nf the model's equality and friction row counts:

* ``jar = J qacc - efc_aref``; ``r = 1 / (D + (D == 0) mjMINVAL)``.
* A row is *linear-neg* if ``fl > 0`` and ``jar <= -r fl``, *linear-pos* if ``fl > 0`` and ``jar >= r fl`` (only if the model has friction rows and
  ``DisableBit.FRICTIONLOSS`` is clear), *quadratic* if it is not linear and (``row < ne + nf`` or ``jar < 0``), else *satisfied*: ``efc_state`` 2, 3, 1, 0
  (MuJoCo's ``mjtConstraintState``).
* ``efc_force = -D jar`` (quadratic), ``+fl`` (linear-neg), ``-fl`` (linear-pos), 0 (satisfied); ``qfrc_constraint = J^T efc_force``.
* ``gauss = 1/2 (M qacc - qfrc_smooth) . (qacc - qacc_smooth)``;
  ``cost = 1/2 sum_quadratic D jar^2 + sum_linear (-1/2 r fl^2 -/+ fl jar) + gauss`` (``-`` on linear-neg rows, ``+`` on linear-pos rows).
* ``grad = M qacc - qfrc_smooth - qfrc_constraint``; ``grad_norm = |grad| / (m.stat.meaninertia * max(1, nv))``: the quantity the reference's solver
  compares with ``opt.tolerance`` to stop -- how far from converged an environment is.
* ``AR = J (L L^T)^-1 J^T + diag(R)`` with ``L = qLD``'s lower triangle (as ``solve_m`` reads it) and ``R = 1 / D`` where ``D > 0``, else 0;
  ``b = J qacc_smooth - efc_aref``.  At the solution ``jar = (AR - diag R) efc_force + b``.

Rows of inactive contacts carry ``J = 0``, ``aref = 0`` and ``D > 0``: they come out satisfied with zero force, and their row of ``AR`` is ``R`` on the diagonal.

After ``forward`` every leaf these functions read belongs to the same pass, and ``qacc`` defaults to ``d.qacc``.  ``step`` returns the constraint leaves, ``qM``,
``qLD``, ``qfrc_smooth``, ``qacc_smooth`` and ``qacc`` of the pass it integrated (the pre-step state), so the defaults are right on its output too; only
``qpos`` / ``qvel`` are already advanced there, and none of these functions reads them.

Every leading dimension of a leaf is the batch (S); nothing is written to the input.  Only dense models exist here.  ``torch.vmap`` / ``torch.compile``: there is
no operator for these functions; they raise ``NotImplementedError``.
"""

from __future__ import annotations

import ctypes
import math
from typing import NamedTuple

import torch

from . import native
from ._enums import DisableBit
from ._postpass import bind, call, check_leaves, check_override, probe, refuse_tracing, require_device
from .support import _query_mode, _strides

MUL_J, MUL_JT, UPDATE, AR = range(4)  # include/mjhip.h MJH_EFC_*
_WHAT = "the constraint-space functions"


class ConstraintUpdate(NamedTuple):
    """``constraint_update``'s result; ``gauss``, ``grad`` and ``grad_norm`` are ``None`` in the ``jar=`` form."""

    jar: torch.Tensor              # S + (nefc,)
    efc_force: torch.Tensor        # S + (nefc,)
    efc_state: torch.Tensor        # S + (nefc,) int32: 0 satisfied, 1 quadratic, 2 linear-neg, 3 linear-pos
    qfrc_constraint: torch.Tensor  # S + (nv,)
    cost: torch.Tensor             # S
    gauss: torch.Tensor | None     # S
    grad: torch.Tensor | None      # S + (nv,)
    grad_norm: torch.Tensor | None  # S


class EfcDual(NamedTuple):
    """``efc_ar``'s result."""

    AR: torch.Tensor  # S + (nefc, nefc)
    b: torch.Tensor   # S + (nefc,)


def plan(op: int, nv: int, nefc: int, dtype) -> tuple[int, int, int, int]:
    """(rows of ``efc_J`` per LDS chunk, chunks, rows of the last chunk, bytes of LDS per workgroup) of one call: the library's own plan
    (``mjh_constraint_space_plan``, a host computation).  A model whose ``efc_ar`` does not fit a workgroup's LDS is a ``RuntimeError``."""
    lib = native.load_library()
    fn = getattr(lib, "mjh_constraint_space_plan", None)
    if fn is None:
        raise RuntimeError(f"{native.LIB_PATH} predates {_WHAT} (no mjh_constraint_space_plan): rebuild the library")
    out = (ctypes.c_int * 4)()
    rc = fn(int(op), int(nv), int(nefc), 8 if dtype == torch.float64 else 4, out)
    if rc != 0:
        raise RuntimeError(f"constraint_space.plan failed ({rc}): {lib.mjh_last_error().decode()}")
    return tuple(out)


def _sizes(m):
    ne, nf, _, _, nefc = m.constraint_sizes_py
    return int(ne), int(nf), int(nefc), int(m.nv)


def _leaves(name, m, d, names):
    """The leaves ``names`` of ``d`` checked against the Model: (batch, dtype, device, B, {name: tensor})."""
    _, _, nefc, nv = _sizes(m)
    tails = dict(efc_J=(nefc, nv), efc_D=(nefc,), efc_aref=(nefc,), efc_frictionloss=(nefc,), qM=(nv, nv), qLD=(nv, nv), qfrc_smooth=(nv,), qacc_smooth=(nv,),
                 qacc=(nv,))
    leaves = {n: getattr(d, n) for n in names}
    batch, dtype, device = probe(name, m, "efc_J", leaves["efc_J"], (nefc, nv))
    check_leaves(name, leaves, tails, batch, dtype, device, 2)
    return batch, dtype, device, (int(math.prod(batch)) if batch else 1), leaves


def _launch(name, m, device, dtype, a, tensors):
    bind(a, tensors)
    call(name, m, "mjh_constraint_space", a, device, dtype, what=_WHAT)


def _mul(name, op, m, d, vec):
    refuse_tracing(name, d.efc_J, vec)
    _, _, nefc, nv = _sizes(m)
    batch, dtype, device, B, leaves = _leaves(name, m, d, ("efc_J",))
    width, other = (nv, nefc) if op == MUL_J else (nefc, nv)
    if not isinstance(vec, torch.Tensor):
        raise ValueError(f"{name}: vec must be a tensor; got {type(vec).__name__}")
    mode = _query_mode(f"{name}: vec", tuple(vec.shape), batch, width)
    if vec.dtype != dtype or vec.device != device:
        raise ValueError(f"{name}: vec is {vec.dtype} on {vec.device}, the Data is {dtype} on {device}")
    if mode[1] == 0:
        raise ValueError(f"{name}: no vectors")
    K = mode[1] or 1
    require_device(device)
    shape = batch + ((mode[1],) if mode[1] is not None else ()) + (other,)
    if B == 0 or nv == 0 or nefc == 0:
        return torch.zeros(shape, dtype=dtype, device=device)
    out = torch.empty(shape, dtype=dtype, device=device)
    a = native.ConstraintSpaceArgs(op=op, K=K, B=B)
    a.vec_env, a.vec_k = _strides(mode, K, width)
    _launch(name, m, device, dtype, a, dict(efc_J=leaves["efc_J"], vec=vec, out=out))
    return out


def mul_jac_vec(m, d, vec: torch.Tensor) -> torch.Tensor:
    """``efc_J @ vec`` per environment (MuJoCo's ``mj_mulJacVec``).  ``vec``: ``(nv,)`` (shared), ``S + (nv,)`` or ``S + (K, nv)``: K independent vectors, as for
    ``mul_m``.  Returns ``S + (nefc,)`` or ``S + (K, nefc)``.  Reads ``d.efc_J``: the output of ``forward`` or ``step`` as it is."""
    return _mul("mul_jac_vec", MUL_J, m, d, vec)


def mul_jac_t_vec(m, d, vec: torch.Tensor) -> torch.Tensor:
    """``efc_J^T @ vec`` per environment (MuJoCo's ``mj_mulJacTVec``).  ``vec``: ``(nefc,)`` (shared), ``S + (nefc,)`` or ``S + (K, nefc)``.  Returns
    ``S + (nv,)`` or ``S + (K, nv)``.  Reads ``d.efc_J``: the output of ``forward`` or ``step`` as it is."""
    return _mul("mul_jac_t_vec", MUL_JT, m, d, vec)


def constraint_update(m, d, qacc: torch.Tensor | None = None, *, jar: torch.Tensor | None = None) -> ConstraintUpdate:
    """States, forces, cost and gradient of the constraint problem at an acceleration (the reference's ``_update_constraint`` / ``_update_gradient``, MuJoCo's
    ``mj_constraintUpdate``): a ``ConstraintUpdate``; the module's docstring has the definitions.

    ``qacc``: ``S + (nv,)``, default ``d.qacc`` -- right on the output of ``forward`` and of ``step`` (which keeps the ``qacc`` and the constraint leaves of the
    pass it integrated).  Reads ``efc_J``, ``efc_D``, ``efc_aref``, ``efc_frictionloss``, ``qM``, ``qfrc_smooth``, ``qacc_smooth`` (and ``qacc``).
    ``grad_norm`` is the reference solver's stopping quantity: below ``m.opt.tolerance`` the environment counts as converged.

    ``jar=`` (``S + (nefc,)``; MuJoCo's ``mj_constraintUpdate`` form) classifies a given ``jar`` instead: only ``efc_J``, ``efc_D`` and ``efc_frictionloss``
    are read, ``gauss`` / ``grad`` / ``grad_norm`` are ``None`` and ``cost`` leaves the Gauss term out.  ``qacc`` together with ``jar`` is a ``ValueError``."""
    name = "constraint_update"
    if qacc is not None and jar is not None:
        raise ValueError(f"{name}: pass qacc= or jar=, not both (with jar= nothing that needs qacc is computed)")
    refuse_tracing(name, d.efc_J, qacc, jar)
    ne, nf, nefc, nv = _sizes(m)
    names = ("efc_J", "efc_D", "efc_frictionloss") + (("efc_aref", "qM", "qfrc_smooth", "qacc_smooth", "qacc") if jar is None else ())
    batch, dtype, device, B, leaves = _leaves(name, m, d, names)
    if qacc is not None:
        check_override(name, "qacc", qacc, batch + (nv,), dtype, device, "the acceleration to evaluate, per environment")
        leaves["qacc"] = qacc
    if jar is not None:
        check_override(name, "jar", jar, batch + (nefc,), dtype, device, "J qacc - aref, per environment")
    meaninertia = float(m.stat.meaninertia)
    if jar is None and not meaninertia > 0:
        raise ValueError(f"{name}: Model.stat.meaninertia is {meaninertia}, expected a positive number")
    require_device(device)
    new = lambda *tail, dt=dtype: torch.empty(batch + tail, dtype=dt, device=device)
    outs = dict(efc_force=new(nefc), efc_state=new(nefc, dt=torch.int32), qfrc_constraint=new(nv), cost=new())
    if jar is None:
        outs.update(jar=new(nefc), gauss=new(), grad=new(nv), grad_norm=new())
    if B == 0 or nv == 0 or nefc == 0:  # (no rows: no force, and with qacc the Gauss term alone)
        for t in outs.values():
            t.zero_()
        if jar is None and B > 0 and nv > 0:
            q = leaves["qacc"]
            ms = torch.matmul(leaves["qM"].reshape(batch + (nv, nv)), q.unsqueeze(-1)).squeeze(-1) - leaves["qfrc_smooth"]
            outs["gauss"] = 0.5 * (ms * (q - leaves["qacc_smooth"])).sum(-1)
            outs["cost"] = outs["gauss"].clone()
            outs["grad"] = ms
            outs["grad_norm"] = ms.norm(dim=-1) / (meaninertia * max(1, nv))
    else:
        floss = nf > 0 and not (int(m.opt.disableflags) & DisableBit.FRICTIONLOSS)
        a = native.ConstraintSpaceArgs(op=UPDATE, B=B, ne_nf=ne + nf, floss=int(floss), meaninertia=meaninertia)
        tensors = dict(leaves, **outs)
        if jar is not None:
            tensors["jar_in"] = jar
        _launch(name, m, device, dtype, a, tensors)
    if jar is not None:
        return ConstraintUpdate(jar, outs["efc_force"], outs["efc_state"], outs["qfrc_constraint"], outs["cost"], None, None, None)
    return ConstraintUpdate(outs["jar"], outs["efc_force"], outs["efc_state"], outs["qfrc_constraint"], outs["cost"], outs["gauss"], outs["grad"], outs["grad_norm"])


def efc_ar(m, d) -> EfcDual:
    """The dual problem of the pass: ``EfcDual(AR, b)`` with ``AR = J M^-1 J^T + diag(R)``, ``S + (nefc, nefc)``, and ``b = J qacc_smooth - efc_aref``,
    ``S + (nefc,)`` (MuJoCo's ``efc_AR`` / ``efc_b``).  ``AR`` is symmetric bit for bit: both triangles are stored from one computed value.  Reads ``efc_J``,
    ``efc_D``, ``efc_aref``, ``qLD`` and ``qacc_smooth``: the output of ``forward`` or ``step`` as it is.  For nv > 16 the reference factors ``M + 1e-10 I``
    (see ``solve_m``), and so does ``AR``.  A model whose ``qLD`` triangle and two row chunks exceed a workgroup's LDS is a ``RuntimeError``."""
    name = "efc_ar"
    refuse_tracing(name, d.efc_J)
    _, _, nefc, nv = _sizes(m)
    batch, dtype, device, B, leaves = _leaves(name, m, d, ("efc_J", "efc_D", "efc_aref", "qLD", "qacc_smooth"))
    require_device(device)
    if B == 0 or nefc == 0 or nv == 0:
        AR_ = torch.zeros(batch + (nefc, nefc), dtype=dtype, device=device)
        b = torch.zeros(batch + (nefc,), dtype=dtype, device=device)
        if B > 0 and nefc > 0:  # (no dofs: J is empty)
            D = leaves["efc_D"]
            AR_ = torch.diag_embed(torch.where(D > 0, 1 / D, torch.zeros_like(D)))
            b = -leaves["efc_aref"].clone()
        return EfcDual(AR_, b)
    AR_ = torch.empty(batch + (nefc, nefc), dtype=dtype, device=device)
    b = torch.empty(batch + (nefc,), dtype=dtype, device=device)
    a = native.ConstraintSpaceArgs(op=AR, B=B)
    _launch(name, m, device, dtype, a, dict(leaves, AR=AR_, b=b))
    return EfcDual(AR_, b)
