"""Arithmetic on configurations: MuJoCo's ``mj_integratePos``, ``mj_differentiatePos`` and ``mj_normalizeQuat`` on plain tensors, and with them the difference and
the sum of physics states in the tangent coordinates of ``transition_fd``.  One native launch each (``mjh_qpos_arith``, ``csrc/mjh_qpos.h``, whose header states the
definitions): one lane per (environment, joint).

* ``integrate_pos(m, qpos, qvel, dt)`` -> ``qpos (+) dt qvel``, ``S + (nq,)``: the step's position update (reference ``forward._integrate_pos``): ``q + dt v`` for
  slide / hinge entries and a free joint's position, ``normalize(q * [cos(dt |w| / 2), w / |w| sin(dt |w| / 2)])`` for every quaternion.
* ``differentiate_pos(m, qpos1, qpos2, dt=1.0)`` -> ``(qpos2 (-) qpos1) / dt``, ``S + (nv,)``: ``(q2 - q1) / dt`` for scalars and positions, for every quaternion
  the reference's ``math.quat_sub(q2, q1) / dt`` -- axis times angle of ``q1^-1 * q2``, the angle in ``(-pi, pi]``.  It is expressed in the frame ``integrate_pos``
  advances in: ``integrate_pos(m, q1, differentiate_pos(m, q1, q2, dt), dt)`` is ``q2`` as a configuration (a quaternion may come back as ``-q``).
* ``normalize_quat(m, qpos)`` -> ``qpos`` with every ball / free quaternion divided by its norm, ``(1, 0, 0, 0)`` where the norm is below 1e-15; every other entry
  is copied bit for bit.
* ``state_sub(m, x2, x1)`` / ``state_add(m, x, dx)`` on physics states ``x = [qpos, qvel, act]`` (``S + (nq + nv + na,)``) and tangent vectors
  ``dx = [dq, dv, dact]`` (``S + (2 nv + na,)``): the ``qpos`` block goes through the two functions above with ``dt = 1``, the rest is plain ``-`` / ``+``.  These
  are the coordinates of the ``A`` / ``B`` that ``transition_fd`` returns: ``state_sub(m, step(state_add(m, x, dx)), step(x))`` is ``A dx`` to first order.

The functions read only the Model's joint tables; the tensors are of the Model's dtype, on a HIP device, and every leading dimension is the batch (S).  Nothing is
written to an input.  The calls run on the caller's current stream.  ``torch.vmap`` / ``torch.compile``: there is no operator for these functions; they raise
``NotImplementedError``.
"""

from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from ._postpass import call, check_override, probe, refuse_tracing, require_device

INTEGRATE, DIFFERENTIATE, NORMALIZE = 0, 1, 2


def _dt(name, dt, nonzero):
    if isinstance(dt, (torch.Tensor, np.ndarray)) and dt.ndim == 0:
        dt = dt.item()
    if not isinstance(dt, (int, float, np.integer, np.floating)) or isinstance(dt, bool) or not math.isfinite(float(dt)) or (nonzero and float(dt) == 0.0):
        raise ValueError(f"{name}: dt must be a finite{' non-zero' if nonzero else ''} Python float or a 0-d value; got {dt!r}")
    return float(dt)


def _arith(name, m, op, a, b, b_len, out_len, dt):
    """One ``mjh_qpos_arith`` call: ``a`` is ``S + (nq,)``, ``b`` (or None) ``S + (b_len,)``; every refusal comes before the launch."""
    refuse_tracing(name, a, b)
    nq = int(m.nq)
    batch, dtype, device = probe(name, m, "qpos" if b is None or op == INTEGRATE else "qpos1", a, (nq,))
    if b is not None:
        check_override(name, "qvel" if op == INTEGRATE else "qpos2", b, batch + (b_len,), dtype, device, "the batch shape of the first argument")
    require_device(device)
    B = int(math.prod(batch)) if batch else 1
    out = torch.empty((B, out_len), dtype=dtype, device=device)
    if B and out_len:
        ac = a.reshape(B, nq).contiguous()
        bc = None if b is None else b.reshape(B, b_len).contiguous()
        ptr = lambda t: ctypes.c_void_p(None if t is None else t.data_ptr())
        call(name, m, "mjh_qpos_arith", (op, ptr(ac), ptr(bc), ctypes.c_double(dt), ptr(out), B), device, dtype)
    return out.reshape(batch + (out_len,))


def integrate_pos(m, qpos, qvel, dt):
    """``qpos (+) dt qvel``, ``S + (nq,)``: the step's position update (quaternions renormalised)."""
    return _arith("integrate_pos", m, INTEGRATE, qpos, qvel, int(m.nv), int(m.nq), _dt("integrate_pos", dt, False))


def differentiate_pos(m, qpos1, qpos2, dt=1.0):
    """``(qpos2 (-) qpos1) / dt``, ``S + (nv,)`` (MuJoCo's ``mj_differentiatePos``)."""
    return _arith("differentiate_pos", m, DIFFERENTIATE, qpos1, qpos2, int(m.nq), int(m.nv), _dt("differentiate_pos", dt, True))


def normalize_quat(m, qpos):
    """``qpos`` with every ball / free quaternion divided by its norm (MuJoCo's ``mj_normalizeQuat``); the other entries bit for bit."""
    return _arith("normalize_quat", m, NORMALIZE, qpos, None, 0, int(m.nq), 1.0)


def _blocks(name, m, x, arg, n0):
    nv, na = int(m.nv), int(m.na)
    if not isinstance(x, torch.Tensor) or x.dim() < 1 or x.shape[-1] != n0 + nv + na:
        raise ValueError(f"{name}: {arg} must have shape (..., {n0 + nv + na}); got {tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__}")
    return x[..., :n0], x[..., n0:]


def state_sub(m, x2, x1):
    """``x2 (-) x1`` of two physics states ``[qpos, qvel, act]``, ``S + (2 nv + na,)``: the tangent coordinates of ``transition_fd``."""
    refuse_tracing("state_sub", x2, x1)
    q2, r2 = _blocks("state_sub", m, x2, "x2", int(m.nq))
    q1, r1 = _blocks("state_sub", m, x1, "x1", int(m.nq))
    if x2.shape != x1.shape:
        raise ValueError(f"state_sub: x2 has shape {tuple(x2.shape)}, x1 {tuple(x1.shape)}")
    return torch.cat([_arith("state_sub", m, DIFFERENTIATE, q1, q2, int(m.nq), int(m.nv), 1.0), r2 - r1], dim=-1)


def state_add(m, x, dx):
    """``x (+) dx`` of a physics state ``[qpos, qvel, act]`` and a tangent vector ``[dq, dv, dact]``, ``S + (nq + nv + na,)``."""
    refuse_tracing("state_add", x, dx)
    q, r = _blocks("state_add", m, x, "x", int(m.nq))
    dq, dr = _blocks("state_add", m, dx, "dx", int(m.nv))
    if x.shape[:-1] != dx.shape[:-1]:
        raise ValueError(f"state_add: x has shape {tuple(x.shape)}, dx {tuple(dx.shape)}")
    return torch.cat([_arith("state_add", m, INTEGRATE, q, dq, int(m.nv), int(m.nq), 1.0), r + dr], dim=-1)
