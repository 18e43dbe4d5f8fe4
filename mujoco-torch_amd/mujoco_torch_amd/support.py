"""Functions that read a finished forward pass and return a tensor (reference ``_src/support.py`` and ``_src/smooth.py``).

``jac(m, d, point, body_id)``, ``apply_ft(m, d, force, torque, point, body_id)``, ``xfrc_accumulate(m, d)``, ``mul_m(m, d, vec)``,
``solve_m(m, d, x)`` and ``full_m(m, d)`` keep the reference's names and parameters and take a batched ``Data`` directly: every leading
dimension of a leaf is the batch (S below).  Each call is one native launch (``mjh_support``, ``csrc/mjh_support.h``) on the caller's
current stream and reads only the leaves it needs (``cdof``, ``subtree_com``, ``xipos``, ``xfrc_applied``, ``qM`` or ``qLD``), so the
caller runs ``forward`` / ``step`` first, as in the reference.  Only dense models exist here (``device_put`` refuses sparse inertia).

Query shapes follow ``ray``: ``point`` / ``force`` / ``torque`` are ``(3,)`` (shared), ``S + (3,)`` or ``S + (P, 3)``; ``body_id`` is an
int, a 0-d integer tensor, or P ids (a sequence or a 1-D integer tensor) shared by every environment.  Per-environment ids are refused.
``torch.vmap`` / ``torch.compile`` go through the ``support_leaves`` operator (compile_op.py).
"""

from __future__ import annotations

import math
from collections.abc import Sequence

import numpy as np
import torch

from . import native
from ._postpass import bind, cached, call, require_device

JAC, APPLY_FT, XFRC, MUL_M, SOLVE_M = range(5)  # include/mjhip.h MJH_SUPPORT_*
_NAMES = ("jac", "apply_ft", "xfrc_accumulate", "mul_m", "solve_m")


# ---- arguments --------------------------------------------------------------------------------------------------------------

def body_ids(body_id, nbody: int) -> tuple[tuple[int, ...], bool]:
    """(ids, listed): the ids as ints validated against [0, nbody); ``listed`` when P ids were given (the result gains a P dimension)."""
    if isinstance(body_id, torch.Tensor):
        from torch._C._functorch import is_batchedtensor

        if is_batchedtensor(body_id):
            raise ValueError("body_id is mapped by torch.vmap: the body ids must be the same for every environment")
        if body_id.dtype.is_floating_point or body_id.dtype.is_complex or body_id.dtype == torch.bool:
            raise ValueError(f"body_id must hold integers, got {body_id.dtype}")
        if body_id.dim() > 1:
            raise ValueError(f"body_id must be an int or P ids shared by every environment (0-d or 1-D); got shape {tuple(body_id.shape)}: "
                             "per-environment body ids are not supported")
        listed, ids = body_id.dim() == 1, body_id.reshape(-1).tolist()
    elif isinstance(body_id, (int, np.integer)) and not isinstance(body_id, bool):
        listed, ids = False, [int(body_id)]
    elif isinstance(body_id, np.ndarray):
        if body_id.ndim != 1 or not (body_id.size == 0 or np.issubdtype(body_id.dtype, np.integer)):
            raise ValueError("body_id must be an int or a flat sequence of ints shared by every environment: per-environment body ids are not supported")
        listed, ids = True, [int(b) for b in body_id.tolist()]
    elif isinstance(body_id, Sequence) and not isinstance(body_id, str):  # (plain Python: traced by Dynamo)
        if not all(isinstance(b, (int, np.integer)) and not isinstance(b, bool) for b in body_id):
            raise ValueError("body_id must be an int or a flat sequence of ints shared by every environment: per-environment body ids are not supported")
        listed, ids = True, [int(b) for b in body_id]
    else:
        raise ValueError(f"body_id must be an int, an integer tensor or a sequence of ints, got {type(body_id).__name__}")
    if not ids:
        raise ValueError("body_id holds no ids")
    bad = [b for b in ids if not 0 <= b < nbody]
    if bad:
        raise ValueError(f"body ids {bad} are outside [0, {nbody})")
    return tuple(ids), listed


def _query_mode(name: str, shape: tuple, batch: tuple, width: int):
    """(per environment?, count or None) of a query of trailing size ``width``: (width,) shared, batch + (width,), batch + (N, width)."""
    k = len(batch)
    if shape == (width,):
        return False, None
    if len(shape) == k + 1 and shape[:k] == batch and shape[-1] == width:
        return True, None
    if len(shape) == k + 2 and shape[:k] == batch and shape[-1] == width:
        return True, shape[k]
    n = "P" if width == 3 else "K"
    raise ValueError(f"{name} must have shape ({width},), {batch + (width,)} or {batch + (n, width)} for a Data of batch shape {batch}; got {shape}")


def _leaf_batch(leaf: torch.Tensor, trailing: int, name: str) -> tuple:
    if leaf.dim() < trailing:
        raise ValueError(f"{name} has shape {tuple(leaf.shape)}")
    return tuple(leaf.shape[: leaf.dim() - trailing])


def plan(op: int, leaves, queries, ids: tuple, listed: bool):
    """Shape checks shared by the direct call and the operator: (batch, count P or K, query modes, output shapes)."""
    if op in (JAC, APPLY_FT, XFRC):
        cdof, com = leaves[0], leaves[1]
        batch = _leaf_batch(cdof, 2, "cdof")
        if cdof.shape[-1] != 6 or com.shape[-1:] != (3,) or _leaf_batch(com, 2, "subtree_com") != batch:
            raise ValueError(f"cdof / subtree_com have shapes {tuple(cdof.shape)} / {tuple(com.shape)}")
        nv = cdof.shape[-2]
        if op == XFRC:
            xipos, xfrc = leaves[2], leaves[3]
            nb = com.shape[-2]
            if tuple(xipos.shape) != batch + (nb, 3) or tuple(xfrc.shape) != batch + (nb, 6):
                raise ValueError(f"xipos / xfrc_applied have shapes {tuple(xipos.shape)} / {tuple(xfrc.shape)} for {nb} bodies")
            return batch, 1, [], [batch + (nv,)]
        names = ("point",) if op == JAC else ("point", "force", "torque")
        modes = [_query_mode(n, tuple(q.shape), batch, 3) for n, q in zip(names, queries)]
        counts = {c for _, c in modes if c is not None} | ({len(ids)} if listed else set())
        if len(counts) > 1:
            raise ValueError(f"the query counts do not agree: {sorted(counts)} (points / forces / torques per environment and body ids)")
        P = counts.pop() if counts else None
        if P == 0:
            raise ValueError("no query points")
        if listed and len(ids) != P:
            raise ValueError(f"{len(ids)} body ids for {P} points")
        tail = ((P,) if P is not None else ()) + (nv,)
        outs = [batch + tail + (3,)] * 2 if op == JAC else [batch + tail]
        return batch, P or 1, modes, outs
    mat = leaves[0]
    batch = _leaf_batch(mat, 2, "qM" if op == MUL_M else "qLD")
    nv = mat.shape[-1]
    if mat.shape[-2] != nv:
        raise ValueError(f"{'qM' if op == MUL_M else 'qLD'} has shape {tuple(mat.shape)}: not square")
    mode = _query_mode("vec" if op == MUL_M else "x", tuple(queries[0].shape), batch, nv)
    if mode[1] == 0:
        raise ValueError("no vectors")
    return batch, mode[1] or 1, [mode], [batch + ((mode[1],) if mode[1] is not None else ()) + (nv,)]


# ---- the native call --------------------------------------------------------------------------------------------------------

_IDS = {}  # (ids, device) -> int32 device tensor


def _device_ids(ids, device):
    return cached(_IDS, (ids, device), lambda: torch.tensor(ids, dtype=torch.int32, device=device))


def _strides(mode, count, width):
    """(environment stride, query stride) in elements of a query laid out contiguously."""
    env, n = mode
    if not env:
        return 0, 0
    if n is None:
        return width, 0
    return width * n, width if n > 1 else 0


def support_native(m, op: int, leaves, queries, ids: tuple, listed: bool):
    """One ``mjh_support`` call on plain tensors (the direct path and the eager body of ``support_leaves``)."""
    batch, count, modes, out_shapes = plan(op, leaves, queries, ids, listed)
    ref = leaves[0]
    dtype, device = ref.dtype, ref.device
    require_device(device)
    if dtype not in (torch.float64, torch.float32):
        raise RuntimeError(f"unsupported Data dtype {dtype}")
    for name, t in zip(("cdof", "subtree_com", "xipos", "xfrc_applied") if op != MUL_M and op != SOLVE_M else ("qM/qLD",), leaves):
        if t.device != device or t.dtype != dtype:
            raise ValueError(f"{name} is {t.dtype} on {t.device}, the Data is {dtype} on {device}")
    nv, nb = int(m.nv), int(m.nbody)
    if op in (JAC, APPLY_FT, XFRC) and (leaves[0].shape[-2] != nv or leaves[1].shape[-2] != nb):
        raise ValueError(f"the Data holds {leaves[0].shape[-2]} dofs / {leaves[1].shape[-2]} bodies, the Model {nv} / {nb}")
    if op in (MUL_M, SOLVE_M) and leaves[0].shape[-1] != nv:
        raise ValueError(f"the Data holds {leaves[0].shape[-1]} dofs, the Model {nv}")
    outs = [torch.empty(s, dtype=dtype, device=device) for s in out_shapes]
    B = int(math.prod(batch)) if batch else 1
    if B == 0 or nv == 0:
        return [o.zero_() for o in outs]
    a = native.ARGS["mjh_support"](op=op, B=B)
    tensors = {f"out{i}": o for i, o in enumerate(outs)}
    if op in (JAC, APPLY_FT, XFRC):
        tensors.update(cdof=leaves[0].reshape(B, nv, 6), subtree_com=leaves[1].reshape(B, nb, 3))
    if op == XFRC:
        tensors.update(xipos=leaves[2].reshape(B, nb, 3), xfrc_applied=leaves[3].reshape(B, nb, 6))
    if op in (JAC, APPLY_FT):
        a.P = count
        a.body_stride = 1 if listed else 0
        tensors.update(body_id=_device_ids(ids, device))
        for name, q, mode in zip(("point", "force", "torque"), queries, modes):
            tensors[name] = q.to(device=device, dtype=dtype)
            e, s = _strides(mode, count, 3)
            setattr(a, name + "_env", e)
            setattr(a, name + "_q", s)
    if op in (MUL_M, SOLVE_M):
        a.K = count
        tensors["qM" if op == MUL_M else "qLD"] = leaves[0].reshape(B, nv, nv)
        tensors["vec"] = queries[0].to(device=device, dtype=dtype)
        a.vec_env, a.vec_k = _strides(modes[0], count, nv)
    bind(a, tensors)
    call(_NAMES[op], m, "mjh_support", a, device, dtype, what="the support functions")
    return outs


def _call(m, op: int, leaves, queries, body_id=None):
    from .forward import _plain

    if op in (JAC, APPLY_FT):
        ids, listed = body_ids(body_id, int(m.nbody))
    else:
        ids, listed = (0,), False
    queries = [q if isinstance(q, torch.Tensor) else torch.as_tensor(q) for q in queries]
    if torch.compiler.is_compiling() or not all(_plain(t) for t in list(leaves) + queries):
        from . import compile_op  # noqa: F401  (registers the operator)

        return torch.ops.mujoco_torch_amd.support_leaves(op, list(leaves), queries, m._op_key_t, m._struct_uid, list(ids), listed)
    return support_native(m, op, leaves, queries, ids, listed)


# ---- public functions -------------------------------------------------------------------------------------------------------

def jac(m, d, point: torch.Tensor, body_id) -> tuple[torch.Tensor, torch.Tensor]:
    """The pair of (nv, 3) Jacobians ``(jacp, jacr)`` of a global point attached to a body (reference support.py:138-153), per environment.

    ``point``: ``(3,)``, ``S + (3,)`` or ``S + (P, 3)``; ``body_id``: an int, a 0-d integer tensor, or P ids shared by every environment.
    Returns two tensors of shape ``S + (nv, 3)``, or ``S + (P, nv, 3)`` when a P dimension is present.  Reads ``cdof`` / ``subtree_com``."""
    return tuple(_call(m, JAC, (d.cdof, d.subtree_com), (point,), body_id))


def apply_ft(m, d, force: torch.Tensor, torque: torch.Tensor, point: torch.Tensor, body_id) -> torch.Tensor:
    """Generalized force ``jacp @ force + jacr @ torque`` of a Cartesian force and torque applied at a point on a body (reference
    support.py:169-181): ``S + (nv,)``, or ``S + (P, nv)``.  ``force`` / ``torque`` / ``point`` take the shapes ``jac``'s ``point`` takes;
    the Jacobian is never formed."""
    return _call(m, APPLY_FT, (d.cdof, d.subtree_com), (point, force, torque), body_id)[0]


def xfrc_accumulate(m, d) -> torch.Tensor:
    """``apply_ft`` of every body's ``xfrc_applied`` at its ``xipos``, summed over the bodies (world included): ``S + (nv,)`` (reference
    support.py:184-194)."""
    return _call(m, XFRC, (d.cdof, d.subtree_com, d.xipos, d.xfrc_applied), ())[0]


def mul_m(m, d, vec: torch.Tensor) -> torch.Tensor:
    """``qM @ vec`` per environment (reference smooth.py:370-374, dense).  ``vec``: ``(nv,)`` (shared), ``S + (nv,)`` or ``S + (K, nv)``: K
    independent vectors, each with nv as the trailing dimension (a column matrix ``(nv, K)`` must be passed transposed).  The result has
    the shape of ``vec`` with the batch in front: ``S + (nv,)`` or ``S + (K, nv)``."""
    return _call(m, MUL_M, (d.qM,), (vec,))[0]


def solve_m(m, d, x: torch.Tensor) -> torch.Tensor:
    """``(L L^T)^-1 x`` with ``L = d.qLD`` per environment (reference smooth.py:335-338, math.small_cholesky_solve): the inverse mass
    matrix applied to ``x``.  ``x`` takes the shapes of ``mul_m``'s ``vec`` (a column matrix ``(nv, K)`` must be passed transposed).
    For nv > 16 the reference factors ``M + 1e-10 I`` (math.py:112-113), so ``solve_m(mul_m(x))`` is not ``x`` to the last digits."""
    return _call(m, SOLVE_M, (d.qLD,), (x,))[0]


def full_m(m, d) -> torch.Tensor:
    """The dense mass matrix: ``d.qM`` itself (reference support.py:83-87; models are dense here)."""
    return d.qM
