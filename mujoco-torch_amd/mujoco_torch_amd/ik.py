"""Batched inverse kinematics for a site pose: damped least squares on the site Jacobian, the scheme of dm_control's ``qpos_from_site_pose`` with constant
regularisation.  Per iteration one kinematics pass (``forward(..., stages=STAGE_KINEMATICS)``, exactly as it is) and one native launch (``mjh_ik_site_step``,
``csrc/mjh_ik.h``, whose header states the definitions): error, Jacobian, the 3x3 or 6x6 Cholesky solve and the update for every environment, one wavefront each.

``ik_site(m, d, site_id, target_pos=None, target_quat=None, *, joints=None, tol=None, max_steps=20, damping=1e-6, max_update_norm=2.0, rot_weight=1.0)`` returns
``IKResult(qpos, err_norm, steps, success)``: ``S + (nq,)``, ``S``, ``S`` int32, ``S`` bool for a Data of batch shape ``S``.

* ``site_id``: one site, shared by every environment.  ``target_pos``: ``(3,)`` or ``S + (3,)``; ``target_quat``: ``(4,)`` or ``S + (4,)``, unit; at least one.
* ``joints``: ``None`` for every dof, or a flat list of joint ids shared by every environment; only their dofs move.  The ``qpos`` entries of every other joint
  come back bit for bit.
* ``tol``: an environment is done once ``err_norm = |e_pos| + rot_weight |e_rot| < tol`` (default: 1e-9 in float64, 2e-4 in float32), ``e_pos = target_pos -
  site_xpos``, ``e_rot`` the rotation vector (angle in [0, pi], world frame) of ``R_target site_xmat^T``.  A done environment is never touched again.
* an update: ``delta = J^T (J J^T + damping I)^-1 e`` with ``J`` the rows of ``jac_site`` asked for, the columns of the other dofs zeroed (a 3x3 or 6x6 Cholesky solve, pivots clamped at 1e-12: a rank-deficient selection gives a capped step, never a NaN); ``|delta|`` is capped
  at ``max_update_norm``; ``qpos <- integrate_pos(qpos, delta, 1)``.  At most ``max_steps`` updates, ``max_steps + 1`` kinematics passes: the last pass only
  evaluates ``err_norm`` and ``success``.  ``steps`` counts the updates of each environment.

Only ``d.qpos`` and what the kinematics stage reads are used; nothing is written to ``d``.  The done flags and counters live on the device: the loop never
synchronises with the host.  The call runs on the caller's current stream.  ``torch.vmap`` / ``torch.compile``: there is no operator for this function; it
raises ``NotImplementedError``.
"""

from __future__ import annotations

import ctypes
import math
from typing import NamedTuple

import numpy as np
import torch

from ._postpass import _module, cached, call, check_override, probe, refuse_tracing, require_device

STAGE_KINEMATICS = 0x001  # (include/mjhip.h: MJH_STAGE_KINEMATICS)
DEFAULT_TOL = {torch.float64: 1e-9, torch.float32: 2e-4}  # the pre-solver tolerance of each dtype
_HOST = {}  # tables uid -> the joint and site tables on the host
_SEL = {}  # (tables uid, the selection's bytes, device) -> the dof mask on the device


class IKResult(NamedTuple):
    qpos: torch.Tensor
    err_norm: torch.Tensor
    steps: torch.Tensor
    success: torch.Tensor


def _host_ints(x):
    x = x.data if not isinstance(x, (torch.Tensor, np.ndarray)) and isinstance(getattr(x, "data", None), torch.Tensor) else x  # (an UnbatchedTensor)
    return np.asarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x).astype(np.int64).reshape(-1)


def _tables(m):
    return cached(_HOST, m.tables.uid, lambda: dict(site_body=_host_ints(m.site_bodyid), jnt_type=_host_ints(m.jnt_type), jnt_dofadr=_host_ints(m.jnt_dofadr)))


def _one_id(name, arg, v, count, what):
    if isinstance(v, (torch.Tensor, np.ndarray)):
        if v.ndim != 0 or (v.dtype.kind not in "iu" if isinstance(v, np.ndarray) else v.dtype.is_floating_point or v.dtype == torch.bool):
            raise ValueError(f"{name}: {arg} must be one integer {what} id, shared by every environment; got shape {tuple(v.shape)}, dtype {v.dtype}")
        v = int(v.item())
    if not isinstance(v, (int, np.integer)) or isinstance(v, bool):
        raise ValueError(f"{name}: {arg} must be one integer {what} id, shared by every environment; got {v!r}")
    if not 0 <= int(v) < count:
        raise ValueError(f"{name}: {arg} is {what} id {int(v)}, the Model has {count} {what}s")
    return int(v)


def dof_selection(name, m, joints):
    """The dof mask of ``joints`` (None: every dof), ``[nv]`` int32 on the host: every refusal about the joint ids is made here."""
    nv, nj = int(m.nv), int(m.njnt)
    sel = np.zeros(nv, dtype=np.int32)
    if joints is None:
        sel[:] = 1
        return sel
    if isinstance(joints, torch.Tensor):
        if joints.dtype.is_floating_point or joints.dtype == torch.bool:
            raise ValueError(f"{name}: joints must hold integer joint ids; got a {joints.dtype} tensor")
        joints = joints.detach().cpu().numpy()
    arr = np.asarray(joints)
    if arr.ndim != 1 or (arr.size and arr.dtype.kind not in "iu"):
        raise ValueError(f"{name}: joints must be a flat list of integer joint ids, shared by every environment; got shape {arr.shape}, dtype {arr.dtype}")
    T = _tables(m)
    for j in arr.tolist():
        if not 0 <= j < nj:
            raise ValueError(f"{name}: joints holds joint id {j}, the Model has {nj} joints")
        a, t = int(T["jnt_dofadr"][j]), int(T["jnt_type"][j])
        sel[a:a + (6 if t == 0 else 3 if t == 1 else 1)] = 1
    return sel


def _target(name, arg, t, n, batch, dtype, device):
    """(the target as a contiguous tensor, its element stride per environment) or (None, 0)."""
    if t is None:
        return None, 0
    if not isinstance(t, torch.Tensor) or tuple(t.shape) not in ((n,), batch + (n,)):
        raise ValueError(f"{name}: {arg} must be a tensor of shape {(n,)} or {batch + (n,)}; got {tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
    check_override(name, arg, t, tuple(t.shape), dtype, device, "the target")
    shared = tuple(t.shape) == (n,) and batch != ()
    return t.reshape(-1, n).contiguous(), 0 if shared or not batch else n


def ik_site(m, d, site_id, target_pos=None, target_quat=None, *, joints=None, tol=None, max_steps=20, damping=1e-6, max_update_norm=2.0, rot_weight=1.0):
    """``IKResult(qpos, err_norm, steps, success)`` of the configurations that put ``site_id`` at the target pose; the module's docstring has the conventions."""
    name = "ik_site"
    qpos = d.qpos
    refuse_tracing(name, qpos, target_pos, target_quat, site_id, joints)
    nq, nv, nb, ns = int(m.nq), int(m.nv), int(m.nbody), int(m.nsite)
    batch, dtype, device = probe(name, m, "qpos", qpos, (nq,))
    site = _one_id(name, "site_id", site_id, ns, "site")
    if target_pos is None and target_quat is None:
        raise ValueError(f"{name}: neither target_pos nor target_quat is given")
    tp, tp_stride = _target(name, "target_pos", target_pos, 3, batch, dtype, device)
    tq, tq_stride = _target(name, "target_quat", target_quat, 4, batch, dtype, device)
    sel = dof_selection(name, m, joints)
    if nv == 0:
        raise ValueError(f"{name}: the Model has no dofs")
    if tol is None:
        tol = DEFAULT_TOL[dtype]
    for arg, v, ok in (("tol", tol, lambda x: x >= 0), ("damping", damping, lambda x: x > 0), ("max_update_norm", max_update_norm, lambda x: x >= 0),
                       ("rot_weight", rot_weight, lambda x: x >= 0)):
        if not isinstance(v, (int, float, np.integer, np.floating)) or isinstance(v, bool) or not math.isfinite(float(v)) or not ok(float(v)):
            raise ValueError(f"{name}: {arg} must be a finite float{' > 0' if arg == 'damping' else ' >= 0'}; got {v!r}")
    if not isinstance(max_steps, (int, np.integer)) or isinstance(max_steps, bool) or max_steps < 0:
        raise ValueError(f"{name}: max_steps must be an integer >= 0; got {max_steps!r}")
    require_device(device)
    B = int(math.prod(batch)) if batch else 1
    q = qpos.detach().reshape(B, nq).clone(memory_format=torch.contiguous_format)  # (the working copy the kernel advances in place)
    err = torch.zeros(B, dtype=dtype, device=device)
    steps = torch.zeros(B, dtype=torch.int32, device=device)
    done = torch.zeros(B, dtype=torch.uint8, device=device)
    if B:
        body = int(_tables(m)["site_body"][site])
        sel_dev = cached(_SEL, (m.tables.uid, sel.tobytes(), device), lambda: torch.tensor(sel, dtype=torch.int32, device=device).contiguous())
        params = (ctypes.c_double * 4)(float(tol), float(damping), float(max_update_norm), float(rot_weight))
        ptr = lambda t: ctypes.c_void_p(None if t is None else t.data_ptr())
        forward = _module("forward").forward
        dq = d.replace(qpos=q.reshape(batch + (nq,)))
        for k in range(int(max_steps) + 1):
            p = forward(m, dq, stages=STAGE_KINEMATICS)
            cdof, com = p.cdof.reshape(B, nv * 6).contiguous(), p.subtree_com.reshape(B, nb * 3).contiguous()
            sx, sm = p.site_xpos.reshape(B, ns * 3).contiguous(), p.site_xmat.reshape(B, ns * 9).contiguous()
            call(name, m, "mjh_ik_site_step", (ptr(cdof), ptr(com), ptr(sx), ptr(sm), site, body, ptr(tp), tp_stride, ptr(tq), tq_stride, ptr(sel_dev), params,
                                               int(k == max_steps), ptr(q), ptr(err), ptr(steps), ptr(done), B), device, dtype)
    return IKResult(q.reshape(batch + (nq,)), err.reshape(batch), steps.reshape(batch), done.reshape(batch).bool())

