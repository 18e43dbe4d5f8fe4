"""A plain numpy reference of what ``transition_fd`` does around the steps (MuJoCo's ``mjd_transitionFD``), for the tests only.

It knows nothing of the library: it takes host arrays and three joint tables (``jnt_type``: 0 free, 1 ball, 2 slide, 3 hinge; ``jnt_qposadr``;
``jnt_dofadr``) and works in the dtype of the arrays it is given (float64 unless a test hands it float32).

State ``x = [dq (nv, tangent space), qvel (nv), act (na)]``, ``ns = 2 nv + na``; column ``c < ns`` perturbs entry ``c`` of ``x``, column ``ns + i``
perturbs ``ctrl[i]``.

* ``integrate(jt, qpos, v, dt)``: ``qpos`` moved along the tangent ``v`` over ``dt``: slide / hinge joints and free translations add ``dt v``;
  ball joints and the rotation of free joints rotate: ``q <- normalize(q * [cos(a / 2), axis sin(a / 2)])``, ``a = dt |v|``, ``axis = v / |v|``;
  a quaternion whose part of ``v`` is exactly zero is left untouched.
* ``difference(jt, q0, q1)``: the tangent ``v`` with ``integrate(q0, v, 1) == q1``: subtraction, or the rotation vector of ``q0^-1 q1``
  (``2 atan2(|vec|, w)`` about ``vec / |vec|``, brought into ``(-pi, pi]``).
* ``ctrl_sides``: the control rule.  A nudge is taken only if ``ctrl`` and the nudged ``ctrl`` both lie inside the range of a limited actuator; the
  backward one only if ``centered`` or if the forward one was refused.
* ``perturbed`` builds the inputs of every perturbed step, ``jacobians`` differences the stepped results: one-sided ``(y+ - y0) / eps`` or
  ``(y0 - y-) / eps``; centered state columns ``(y+ - y-) / (2 eps)``; a control column with both sides is the mean of its two one-sided
  differences; with none it is zero.

``bound``: how far two correct evaluations of a quaternion-touched entry may lie apart (see there).
"""
import numpy as np

FREE, BALL, SLIDE, HINGE = 0, 1, 2, 3


class Joints:
    """The joint tables, and per dof: the qpos address it adds to (``adr``), or of its quaternion with the axis it turns about (``axis`` 0..2, else -1)."""

    def __init__(self, jnt_type, jnt_qposadr, jnt_dofadr, nq, nv):
        self.type = np.asarray(jnt_type).astype(np.int64).reshape(-1)
        self.qadr = np.asarray(jnt_qposadr).astype(np.int64).reshape(-1)
        self.dadr = np.asarray(jnt_dofadr).astype(np.int64).reshape(-1)
        self.nq, self.nv = int(nq), int(nv)
        self.adr, self.axis = np.zeros(self.nv, dtype=np.int64), -np.ones(self.nv, dtype=np.int64)
        self.quats = []  # (qpos address of the quaternion, dof address of its three rotational dofs)
        for t, qa, da in zip(self.type, self.qadr, self.dadr):
            if t == FREE:
                self.adr[da:da + 3] = qa + np.arange(3)
                self.adr[da + 3:da + 6], self.axis[da + 3:da + 6] = qa + 3, np.arange(3)
                self.quats.append((qa + 3, da + 3))
            elif t == BALL:
                self.adr[da:da + 3], self.axis[da:da + 3] = qa, np.arange(3)
                self.quats.append((qa, da))
            else:
                self.adr[da] = qa
        self.rot_dofs = np.nonzero(self.axis >= 0)[0]


def quat_mul(u, v):
    return np.stack([u[..., 0] * v[..., 0] - u[..., 1] * v[..., 1] - u[..., 2] * v[..., 2] - u[..., 3] * v[..., 3],
                     u[..., 0] * v[..., 1] + u[..., 1] * v[..., 0] + u[..., 2] * v[..., 3] - u[..., 3] * v[..., 2],
                     u[..., 0] * v[..., 2] - u[..., 1] * v[..., 3] + u[..., 2] * v[..., 0] + u[..., 3] * v[..., 1],
                     u[..., 0] * v[..., 3] + u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1] + u[..., 3] * v[..., 0]], axis=-1)


def _norm(x):
    s = x[..., 0] * x[..., 0]
    for i in range(1, x.shape[-1]):
        s = s + x[..., i] * x[..., i]
    return np.sqrt(s)


def _unit(x):
    """(x / |x|, |x|); a zero vector stays zero."""
    n = _norm(x)
    den = n + x.dtype.type(1e-6) * (n == 0)
    return x / den[..., None], n


def quat_integrate(q, v, dt):
    axis, n = _unit(v)
    half = (q.dtype.type(dt) * n) * q.dtype.type(0.5)
    qr = np.concatenate([np.cos(half)[..., None], axis * np.sin(half)[..., None]], axis=-1)
    return _unit(quat_mul(q, qr))[0]


def quat_sub(q1, q0):
    """The rotation vector of q0^-1 q1."""
    inv = q0 * np.array([1, -1, -1, -1], dtype=q0.dtype)
    q = quat_mul(inv, q1)
    axis, s = _unit(q[..., 1:])
    a = 2 * np.arctan2(s, q[..., 0])
    a = np.where(a > q.dtype.type(np.pi), a - 2 * q.dtype.type(np.pi), a)
    return axis * a[..., None]


def integrate(jt, qpos, v, dt):
    qpos, v = np.asarray(qpos), np.asarray(v, dtype=np.asarray(qpos).dtype)
    out = np.array(qpos)
    add = np.nonzero(jt.axis < 0)[0]
    out[..., jt.adr[add]] = qpos[..., jt.adr[add]] + qpos.dtype.type(dt) * v[..., add]
    for qa, da in jt.quats:  # (a quaternion whose tangent is exactly zero is left as it is, not re-normalised)
        w = np.broadcast_to(v[..., da:da + 3], qpos.shape[:-1] + (3,))
        moved = quat_integrate(qpos[..., qa:qa + 4], w, dt)
        out[..., qa:qa + 4] = np.where((w != 0).any(-1, keepdims=True), moved, qpos[..., qa:qa + 4])
    return out


def difference(jt, q0, q1):
    q0, q1 = np.asarray(q0), np.asarray(q1)
    out = np.zeros(np.broadcast_shapes(q0.shape[:-1], q1.shape[:-1]) + (jt.nv,), dtype=q0.dtype)
    add = np.nonzero(jt.axis < 0)[0]
    out[..., add] = q1[..., jt.adr[add]] - q0[..., jt.adr[add]]
    for qa, da in jt.quats:
        out[..., da:da + 3] = quat_sub(q1[..., qa:qa + 4], q0[..., qa:qa + 4])
    return out


def ctrl_sides(ctrl, eps, limited, ctrlrange, centered):
    """(forward taken, backward taken), bool arrays shaped like ``ctrl`` ([..., nu]); ``limited`` [nu], ``ctrlrange`` [nu, 2]."""
    u = np.asarray(ctrl)
    h = u.dtype.type(eps)
    lim = np.asarray(limited).astype(bool)
    lo, hi = np.asarray(ctrlrange, dtype=u.dtype)[:, 0], np.asarray(ctrlrange, dtype=u.dtype)[:, 1]
    inside = lambda x: (x >= lo) & (x <= hi)
    fwd = ~lim | (inside(u) & inside(u + h))
    bwd = (bool(centered) | ~fwd) & (~lim | (inside(u) & inside(u - h)))
    return fwd, bwd


def perturbed(jt, qpos, qvel, act, ctrl, eps, centered, limited, ctrlrange):
    """The inputs of the perturbed steps: {qpos, qvel, act, ctrl}, each [B, ncol, nside, n], and the control flags (fwd, bwd) [B, nu].
    One-sided, a control column carries the forward nudge, else the backward one, else nothing; centered, side 0 the forward and side 1 the
    backward nudge, a refused side nothing."""
    qpos, qvel, act, ctrl = (np.asarray(x) for x in (qpos, qvel, act, ctrl))
    B, nv, na, nu = qpos.shape[0], jt.nv, act.shape[-1], ctrl.shape[-1]
    ns, nside = 2 * nv + na, 2 if centered else 1
    h = qpos.dtype.type(eps)
    rep = lambda x: np.array(np.broadcast_to(x[:, None, None, :], (B, ns + nu, nside, x.shape[-1])))
    P = dict(qpos=rep(qpos), qvel=rep(qvel), act=rep(act), ctrl=rep(ctrl))
    fwd, bwd = ctrl_sides(ctrl, eps, limited, ctrlrange, centered) if nu else (np.zeros((B, 0), bool), np.zeros((B, 0), bool))
    for side in range(nside):
        s = -h if side else h
        for j in range(nv):
            e = np.zeros(nv, dtype=qpos.dtype)
            e[j] = 1
            P["qpos"][:, j, side] = integrate(jt, qpos, e, s)
        for j in range(nv):
            P["qvel"][:, nv + j, side, j] = qvel[:, j] + s
        for j in range(na):
            P["act"][:, 2 * nv + j, side, j] = act[:, j] + s
        for j in range(nu):
            if centered:
                take, sj = (bwd[:, j] if side else fwd[:, j]), np.full(B, s)
            else:
                take, sj = fwd[:, j] | bwd[:, j], np.where(fwd[:, j], h, -h)
            P["ctrl"][:, ns + j, side, j] = np.where(take, ctrl[:, j] + sj, ctrl[:, j])
    return P, (fwd, bwd)


def _state_sub(jt, y1, y0, sensors):
    parts = [difference(jt, y0["qpos"], y1["qpos"]), y1["qvel"] - y0["qvel"], y1["act"] - y0["act"]]
    if sensors:
        parts.append(y1["sensordata"] - y0["sensordata"])
    return np.concatenate(parts, axis=-1)


def jacobians(jt, y0, y, eps, centered, sides, sensors=False):
    """A, B (C, D) from the nominal results ``y0`` ({leaf: [B, n]}) and the perturbed ones ``y`` ({leaf: [B, ncol, nside, n]})."""
    fwd, bwd = sides
    dt = y0["qvel"].dtype
    h = dt.type(eps)
    nv, na = jt.nv, y0["act"].shape[-1]
    ns, nu = 2 * nv + na, fwd.shape[-1]
    base = {k: v[:, None, :] for k, v in y0.items()}
    plus, minus = {k: v[:, :, 0] for k, v in y.items()}, {k: v[:, :, -1] for k, v in y.items()}
    f = _state_sub(jt, plus, base, sensors) / h    # [B, ncol, rows]
    b = _state_sub(jt, base, minus, sensors) / h
    if centered:
        J = _state_sub(jt, plus, minus, sensors) / (2 * h)
        both = (f[:, ns:] + b[:, ns:]) * dt.type(0.5)
        F, Bk = fwd[:, :, None], bwd[:, :, None]
        J[:, ns:] = np.where(F & Bk, both, np.where(F, f[:, ns:], np.where(Bk, b[:, ns:], 0)))
    else:
        J = np.array(f)
        F, Bk = fwd[:, :, None], bwd[:, :, None]
        J[:, ns:] = np.where(F, f[:, ns:], np.where(Bk, b[:, ns:], 0))
    J = np.swapaxes(J, 1, 2)  # [B, rows, ncol]
    out = (J[:, :ns, :ns], J[:, :ns, ns:])
    return out + ((J[:, ns:, :ns], J[:, ns:, ns:]) if sensors else ())


# roundings that can separate two correct evaluations of the rotation vector of q0^-1 q1 for nearby quaternions: each component of the product
# is 4 products and 3 additions of terms of magnitude <= 1 (7 roundings that do NOT shrink with the result: the vector part cancels), doubled by
# the factor 2 of the angle; the normalisation, atan2 and the final product add 6 more, relative to the rotation vector itself (|r| <= pi).
QUAT_SUB_OPS = 2 * 7 + 6 * np.pi
# ... and of a quaternion integrated over a small angle: cos, the 7 roundings of a product component, and 4 squares, 3 additions, a root and a
# division of the normalisation, relative to components of magnitude <= 1 (the sine's error is scaled by the half angle and drops out)
QUAT_INTEGRATE_OPS = 1 + 7 + 9


def bound(machine_eps, eps):
    """Allowed distance between two correct evaluations of a finite difference whose ROW is a rotational dof of a ball / free joint: both may be
    ``QUAT_SUB_OPS`` roundings off, the difference is divided by ``eps`` (one-sided; a centered one divides twice that by ``2 eps``)."""
    return 2.0 * QUAT_SUB_OPS * float(machine_eps) / float(eps)


def column_bound(machine_eps, eps, ref_rot_columns):
    """... whose COLUMN is one: the two perturbed quaternions may differ by ``2 QUAT_INTEGRATE_OPS`` roundings in each of 4 components, i.e. by a
    rotation of at most ``2 * sqrt(4)`` times that (d omega = 2 q^-1 dq), which the step carries to its outputs through the three columns of that
    joint's rotational dofs; ``ref_rot_columns`` [..., rows, 3] are those columns of the yardstick.  Returns [..., rows]."""
    domega = 2.0 * 2.0 * (2.0 * QUAT_INTEGRATE_OPS * float(machine_eps))
    return domega / float(eps) * np.abs(np.asarray(ref_rot_columns, dtype=np.float64)).sum(-1)
