"""A plain numpy reference of the support functions (jac / apply_ft / xfrc_accumulate / mul_m / solve_m), for the tests only.

It takes the Data leaves (``cdof``, ``subtree_com``, ``xipos``, ``xfrc_applied``, ``qM``, ``qLD``) and the model tables (``body_parentid``,
``body_rootid``, ``dof_bodyid``) as host arrays, every leaf with ONE leading environment axis.  The ancestor-dof mask of a body comes from
walking ``body_parentid`` here (``ancestor_mask``); the library's own ``body_dofmask`` table is never read.

* ``jac_same`` evaluates jacp / jacr in the leaves' own dtype, operation by operation as the header of csrc/mjh_support.h states them
  (the library is built without floating-point contraction), so it is bit-identical to the kernel and to the reference project.
* the ``*_hp`` functions evaluate the same operations in ``HP`` and return ``(value, S_abs)``: per output element the value and the sum of
  the absolute values of the elementary terms it is made of (the unrounded high-precision products, a cross product counted as its two
  products).  ``HP`` is ``numpy.longdouble`` where that is wider than float64 (x86-64: the 80-bit extended format, eps 1.1e-19), float64 otherwise;
  ``bound`` adds the reference's own rounding (``EPS_HP``) to the format's, so that the checks stay derived where the two coincide.

Bounds (``bound``): a sum of n products that is evaluated with one rounding per product and per addition, in any order, is within
``(n + 2) eps S_abs`` of its exact value (the forward bound of recursive summation, gamma_n <= (n + 2) eps for n eps < 0.1, Higham, Accuracy
and Stability of Numerical Algorithms, section 4.2).  ``solve_m`` is held by its residual instead (``solve_m_residual``, Higham section 8.1).
"""
import numpy as np

HP = np.longdouble if np.finfo(np.longdouble).eps < np.finfo(np.float64).eps else np.float64
EPS_HP = float(np.finfo(HP).eps)

# roundings an elementary term of jacp has taken before it is multiplied by a force or a velocity: offset = point - com, the product, the
# subtraction of the two cross products, the addition of cdof[3 + k] (the mask multiplies by exactly 0 or 1)
JACP_ROUNDINGS = 4


def ancestor_mask(body_parentid, dof_bodyid):
    """bool [nbody, nv]: dof d acts on body b when d's body is b or one of b's ancestors (the world body 0 carries no dof)."""
    parent, dof_body = np.asarray(body_parentid).astype(np.int64), np.asarray(dof_bodyid).astype(np.int64)
    mask = np.zeros((parent.shape[0], dof_body.shape[0]), dtype=bool)
    for b in range(parent.shape[0]):
        a = b
        while a > 0:
            mask[b, dof_body == a] = True
            a = int(parent[a])
    return mask


def bound(n, eps, s_abs):
    """Per element: the error allowed to a sum of n rounded products of total magnitude ``s_abs``, the reference's own rounding included."""
    return (np.asarray(n, dtype=np.float64) + 2.0) * (float(eps) + EPS_HP) * np.asarray(s_abs, dtype=np.float64)


def _points(point, B, P):
    """point as [B, P, 3]: (3,), [B, 3] (P = 1) or [B, P, 3]."""
    point = np.asarray(point)
    if point.ndim == 1:
        return np.broadcast_to(point, (B, P, 3))
    if point.ndim == 2:
        return np.broadcast_to(point[:, None, :], (B, P, 3))
    return point


def _jac(cdof, subtree_com, body_rootid, mask, point, ids, dtype, with_abs):
    cdof, com = np.asarray(cdof, dtype=dtype), np.asarray(subtree_com, dtype=dtype)
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    B, P = cdof.shape[0], ids.shape[0]
    point = np.asarray(_points(point, B, P), dtype=dtype)
    off = point - com[:, np.asarray(body_rootid).astype(np.int64)[ids]]  # [B, P, 3]
    on = mask[ids].astype(dtype)[None, :, :]                           # [1, P, nv]
    cd = cdof[:, None, :, :]                                           # [B, 1, nv, 6]
    jacp, jacr = np.zeros((B, P, cdof.shape[1], 3), dtype=dtype), np.zeros((B, P, cdof.shape[1], 3), dtype=dtype)
    absp, absr = (np.zeros_like(jacp), np.zeros_like(jacr)) if with_abs else (None, None)
    for k in range(3):
        k1, k2 = (k + 1) % 3, (k + 2) % 3
        a, b = cd[..., k1] * off[:, :, None, k2], cd[..., k2] * off[:, :, None, k1]
        c = a - b
        jacp[..., k] = (cd[..., 3 + k] + c) * on
        jacr[..., k] = cd[..., k] * on
        if with_abs:
            absp[..., k] = (np.abs(cd[..., 3 + k]) + np.abs(a) + np.abs(b)) * on
            absr[..., k] = np.abs(cd[..., k]) * on
    return jacp, jacr, absp, absr


def jac_same(cdof, subtree_com, body_rootid, mask, point, ids):
    """(jacp, jacr), each [B, P, nv, 3], in the dtype of ``cdof``: off = point - subtree_com[root], c_k = cdof[k1] off[k2] - cdof[k2] off[k1],
    jacp = (cdof[3 + k] + c_k) * mask, jacr = cdof[k] * mask -- every operation rounded once, in that dtype."""
    dtype = np.asarray(cdof).dtype
    assert dtype in (np.float32, np.float64) and np.asarray(subtree_com).dtype == dtype and np.asarray(point).dtype == dtype
    return _jac(cdof, subtree_com, body_rootid, mask, point, ids, dtype, False)[:2]


def jac_hp(cdof, subtree_com, body_rootid, mask, point, ids):
    """((jacp, S_abs of jacp), (jacr, S_abs of jacr)) in HP."""
    jp, jr, ap, ar = _jac(cdof, subtree_com, body_rootid, mask, point, ids, HP, True)
    return (jp, ap), (jr, ar)


def apply_ft_hp(cdof, subtree_com, body_rootid, mask, point, force, torque, ids):
    """jacp . force + jacr . torque per (environment, query, dof): ([B, P, nv], S_abs).  force / torque take the shapes of point."""
    (jp, ap), (jr, ar) = jac_hp(cdof, subtree_com, body_rootid, mask, point, ids)
    B, P = jp.shape[:2]
    f, t = np.asarray(_points(force, B, P), dtype=HP)[:, :, None, :], np.asarray(_points(torque, B, P), dtype=HP)[:, :, None, :]
    return (jp * f + jr * t).sum(-1), (ap * np.abs(f) + ar * np.abs(t)).sum(-1)


def xfrc_hp(cdof, subtree_com, xipos, xfrc_applied, body_rootid, mask):
    """apply_ft of every body's xfrc_applied at its xipos, summed over all bodies: ([B, nv], S_abs)."""
    x = np.asarray(xfrc_applied)
    val, s = apply_ft_hp(cdof, subtree_com, body_rootid, mask, xipos, x[..., :3], x[..., 3:], np.arange(x.shape[1]))
    return val.sum(1), s.sum(1)


def point_velocity_hp(cdof, subtree_com, body_rootid, mask, point, ids, qvel):
    """jacp^T qvel and jacr^T qvel per (environment, query): ((v [B, P, 3], S_abs), (omega [B, P, 3], S_abs))."""
    (jp, ap), (jr, ar) = jac_hp(cdof, subtree_com, body_rootid, mask, point, ids)
    q = np.asarray(qvel, dtype=HP)[:, None, :, None]
    return ((jp * q).sum(2), (ap * np.abs(q)).sum(2)), ((jr * q).sum(2), (ar * np.abs(q)).sum(2))


def mul_m_hp(qM, vec):
    """qM x for vec [B, K, nv]: ([B, K, nv], S_abs = |qM| |x|)."""
    M, x = np.asarray(qM, dtype=HP)[:, None, :, :], np.asarray(vec, dtype=HP)[:, :, None, :]
    return (M * x).sum(-1), (np.abs(M) * np.abs(x)).sum(-1)


def solve_m_hp(qLD, vec):
    """(L L^T)^-1 b for vec [B, K, nv] by forward and backward substitution on L = tril(qLD): ([B, K, nv], S_abs = |L| |L^T| |x|)."""
    L = np.tril(np.asarray(qLD, dtype=HP))
    x = np.array(np.asarray(vec, dtype=HP))
    nv = L.shape[-1]
    for i in range(nv):  # L y = b
        x[:, :, i] = (x[:, :, i] - (L[:, None, i, :i] * x[:, :, :i]).sum(-1)) / L[:, None, i, i]
    for i in range(nv - 1, -1, -1):  # L^T x = y
        x[:, :, i] = (x[:, :, i] - (L[:, None, i + 1:, i] * x[:, :, i + 1:]).sum(-1)) / L[:, None, i, i]
    return x, _abs_llt(L, x)


def _abs_llt(L, x):
    aL = np.abs(L)
    return (aL[:, None] * (np.swapaxes(aL, 1, 2)[:, None] * np.abs(x)[:, :, None, :]).sum(-1)[:, :, None, :]).sum(-1)


def solve_m_residual(qLD, vec, x):
    """Of a computed solution x [B, K, nv] of L L^T x = b: (|b - L L^T x|, |L| |L^T| |x|), in HP, per component."""
    L = np.tril(np.asarray(qLD, dtype=HP))
    x, b = np.asarray(x, dtype=HP), np.asarray(vec, dtype=HP)
    ltx = (np.swapaxes(L, 1, 2)[:, None] * x[:, :, None, :]).sum(-1)
    return np.abs(b - (L[:, None] * ltx[:, :, None, :]).sum(-1)), _abs_llt(L, x)


def solve_m_factor(nv, eps):
    """2 g + g^2, g = gamma_(nv + 1): the componentwise backward error of a forward and a backward substitution with the same factor."""
    g = (nv + 1) * (float(eps) + EPS_HP) / (1.0 - (nv + 1) * (float(eps) + EPS_HP))
    return 2.0 * g + g * g


def solve_m_forward_bound(qLD, x, eps):
    """|x - x_exact| <= |(L L^T)^-1| r, r the residual bound of ``x``: the forward error the residual bound implies, per component."""
    L = np.asarray(qLD)
    nv = L.shape[-1]
    eye = np.broadcast_to(np.eye(nv, dtype=HP), (L.shape[0], nv, nv))
    inv = np.abs(solve_m_hp(qLD, eye)[0])  # rows of the (symmetric) inverse
    r = solve_m_factor(nv, eps) * _abs_llt(np.tril(np.asarray(qLD, dtype=HP)), np.asarray(x, dtype=HP))
    return (inv[:, None] * r[:, :, None, :]).sum(-1)
