"""A numpy longdouble reference of the configuration arithmetic (mujoco_torch_amd/qpos.py), for the tests only.  It restates the three definitions:

* ``integrate_pos``:     slide / hinge and free positions ``q + dt v``; every quaternion ``normalize(q * [cos(dt |w| / 2), a sin(dt |w| / 2)])``,
                         ``a = w / (|w| + 1e-6 [|w| == 0])`` (reference forward.py:231-252, math.quat_integrate).
* ``differentiate_pos``: scalars and positions ``(q2 - q1) / dt``; every quaternion axis times angle of ``q1^-1 * q2`` over ``dt``, ``angle = 2 atan2(|xyz|, w)`` taken
                         into ``(-pi, pi]``, the zero vector when ``|xyz| == 0`` (reference math.quat_sub; MuJoCo's mj_differentiatePos).
* ``normalize_quat``:    every ball / free quaternion over its norm, ``(1, 0, 0, 0)`` below 1e-15; the rest copied.

Inputs: arrays with any leading dimensions; the joint tables as ``joints(mx)`` returns them.  Outputs are longdouble.
"""
import numpy as np
import torch

LD = np.longdouble
FREE, BALL = 0, 1
PI = LD(4) * np.arctan(LD(1))


def _np(x):
    x = x.data if not isinstance(x, (torch.Tensor, np.ndarray)) and isinstance(getattr(x, "data", None), torch.Tensor) else x  # (an UnbatchedTensor)
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def joints(mx):
    """[(type, qposadr, dofadr)] of the model's joints, and (nq, nv)."""
    rows = list(zip(_np(mx.jnt_type).astype(int).tolist(), _np(mx.jnt_qposadr).astype(int).tolist(), _np(mx.jnt_dofadr).astype(int).tolist()))
    return rows, int(mx.nq), int(mx.nv)


def quat_mul(u, v):
    """u * v, the terms paired so that conj(q) * q has an exactly zero vector part in any precision."""
    return np.stack([u[..., 0] * v[..., 0] - u[..., 1] * v[..., 1] - u[..., 2] * v[..., 2] - u[..., 3] * v[..., 3],
                     (u[..., 0] * v[..., 1] + u[..., 1] * v[..., 0]) + (u[..., 2] * v[..., 3] - u[..., 3] * v[..., 2]),
                     (u[..., 0] * v[..., 2] + u[..., 2] * v[..., 0]) + (u[..., 3] * v[..., 1] - u[..., 1] * v[..., 3]),
                     (u[..., 0] * v[..., 3] + u[..., 3] * v[..., 0]) + (u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1])], -1)


def quat_integrate(q, w, dt):
    n = np.sqrt((w * w).sum(-1, keepdims=True))
    a = w / (n + LD(1e-6) * (n == 0))
    ang = LD(dt) * n
    r = quat_mul(q, np.concatenate([np.cos(ang / 2), a * np.sin(ang / 2)], -1))
    rn = np.sqrt((r * r).sum(-1, keepdims=True))
    return r / (rn + LD(1e-6) * (rn == 0))


def quat_sub(q2, q1):
    """axis times angle of q1^-1 * q2, the angle in (-pi, pi]."""
    inv = q1 * np.array([1, -1, -1, -1], dtype=LD)
    r = quat_mul(inv, q2)
    s = np.sqrt((r[..., 1:] ** 2).sum(-1, keepdims=True))
    axis = r[..., 1:] / (s + LD(1e-6) * (s == 0))
    ang = 2 * np.arctan2(s, r[..., :1])
    ang = np.where(ang > PI, ang - 2 * PI, ang)
    return axis * ang


def integrate_pos(J, qpos, qvel, dt):
    rows, nq, nv = J
    q, v = np.asarray(qpos, dtype=LD), np.asarray(qvel, dtype=LD)
    out = np.empty(q.shape, dtype=LD)
    for t, qa, da in rows:
        if t == FREE:
            out[..., qa:qa + 3] = q[..., qa:qa + 3] + LD(dt) * v[..., da:da + 3]
            out[..., qa + 3:qa + 7] = quat_integrate(q[..., qa + 3:qa + 7], v[..., da + 3:da + 6], dt)
        elif t == BALL:
            out[..., qa:qa + 4] = quat_integrate(q[..., qa:qa + 4], v[..., da:da + 3], dt)
        else:
            out[..., qa] = q[..., qa] + LD(dt) * v[..., da]
    return out


def differentiate_pos(J, qpos1, qpos2, dt=1.0):
    rows, nq, nv = J
    q1, q2 = np.asarray(qpos1, dtype=LD), np.asarray(qpos2, dtype=LD)
    out = np.empty(q1.shape[:-1] + (nv,), dtype=LD)
    for t, qa, da in rows:
        if t == FREE:
            out[..., da:da + 3] = (q2[..., qa:qa + 3] - q1[..., qa:qa + 3]) / LD(dt)
            out[..., da + 3:da + 6] = quat_sub(q2[..., qa + 3:qa + 7], q1[..., qa + 3:qa + 7]) / LD(dt)
        elif t == BALL:
            out[..., da:da + 3] = quat_sub(q2[..., qa:qa + 4], q1[..., qa:qa + 4]) / LD(dt)
        else:
            out[..., da] = (q2[..., qa] - q1[..., qa]) / LD(dt)
    return out


def normalize_quat(J, qpos):
    rows, nq, nv = J
    q = np.asarray(qpos, dtype=LD)
    out = q.copy()
    for t, qa, da in rows:
        if t in (FREE, BALL):
            k = qa + (3 if t == FREE else 0)
            n = np.sqrt((q[..., k:k + 4] ** 2).sum(-1, keepdims=True))
            unit = np.zeros(4, dtype=LD)
            unit[0] = 1
            out[..., k:k + 4] = np.where(n < LD(1e-15), unit, q[..., k:k + 4] / np.where(n == 0, LD(1), n))
    return out


def quat_slices(J):
    """The start of every quaternion in qpos."""
    return [qa + (3 if t == FREE else 0) for t, qa, da in J[0] if t in (FREE, BALL)]
