"""A plain numpy reference of jac_dot, jac_subtree_com and angmom_mat (mujoco_torch_amd/jacobian.py), for the tests only, in the style of tests/_support_ref.py.

It takes the Data leaves (``cdof``, ``cdof_dot``, ``cvel``, ``subtree_com``, ``xipos``, ``ximat``) as host arrays with ONE leading environment axis and the model
tables as ``tables(mx)`` returns them; the ancestor mask of a body comes from walking ``body_parentid`` (``_support_ref.ancestor_mask``), a subtree from the same
walk: the library's own ``body_dofmask`` / ``body_subtree_end`` tables are never read.

Per environment, with c(b) = subtree_com[body_rootid[b]], (w_i, v_i) = cdof[i], mask(b, i) and J_b(x)[i] = (v_i + w_i x (x - c(b))) mask(b, i):

* ``subtree_com_hp``:  out[i] = (sum_{b in subtree(body)} body_mass[b] J_b(xipos[b])[i]) / body_subtreemass[body]
* ``angmom_hp``:       out[i] = sum_{b in subtree(body)} (R_b diag(body_inertia[b]) R_b^T w_i mask(b, i) + body_mass[b] (xipos[b] - C) x (J_b(xipos[b])[i] - subtree_com_hp[i])),
                       R_b = ximat[b], C = subtree_com[body]
* ``dot_hp``:          jacr_dot[i] = wd_i mask(body, i), jacp_dot[i] = (vd_i + wd_i x (p - c) + w_i x pdot) mask(body, i), pdot = U + W x (p - c), (W, U) = cvel[body];
                       (wd_i, vd_i) = cdof_dot[i], but for the dofs of a ball joint and the rotations of a free joint the motion cross product of
                       cvel[dof_bodyid[i]] with cdof[i]: wd_i = Wb x w_i, vd_i = Wb x v_i + Ub x w_i.

Each returns ``(value, S_abs, n)`` per output element, value and S_abs in ``HP``: S_abs is the same expression evaluated on the absolute values of its inputs with
every subtraction turned into an addition (differences of positions -- point - c, xipos - C -- are formed first and enter by their absolute value, as in
``_support_ref``), i.e. the sum of the absolute values of the elementary products the element is made of; n counts those products plus the roundings an
elementary product takes on its way into the sum (``_support_ref.JACP_ROUNDINGS`` for a J_b entry).  A kernel that rounds once per operation is then within
``_support_ref.bound(n, eps, S_abs)`` (Higham, section 4.2).  ``product`` contracts a matrix with a vector: nv more terms.
"""
import numpy as np
import torch

from _support_ref import EPS_HP, HP, JACP_ROUNDINGS, ancestor_mask, bound  # noqa: F401  (bound / EPS_HP: for the tests)

FREE, BALL = 0, 1
LEAVES = ("cdof", "cdof_dot", "cvel", "subtree_com", "xipos", "ximat")


def _np(x):
    x = x.data if not isinstance(x, (torch.Tensor, np.ndarray)) and isinstance(getattr(x, "data", None), torch.Tensor) else x  # (an UnbatchedTensor)
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def tables(mx):
    """The model tables and values the definitions use, as host arrays."""
    parent, dof_body = _np(mx.body_parentid).astype(np.int64), _np(mx.dof_bodyid).astype(np.int64)
    nb = parent.shape[0]
    sub = np.zeros((nb, nb), dtype=bool)  # sub[a, b]: b lies in the subtree of a
    for b in range(nb):
        a = b
        while True:
            sub[a, b] = True
            if a == 0:
                break
            a = int(parent[a])
    jt, jadr, dj = _np(mx.jnt_type).astype(np.int64), _np(mx.jnt_dofadr).astype(np.int64), _np(mx.dof_jntid).astype(np.int64)
    idx = np.arange(dof_body.shape[0])
    rot = (jt[dj] == BALL) | ((jt[dj] == FREE) & (idx - jadr[dj] >= 3)) if idx.size else np.zeros(0, dtype=bool)
    return dict(nbody=nb, parent=parent, root=_np(mx.body_rootid).astype(np.int64), dof_body=dof_body, mask=ancestor_mask(parent, dof_body), sub=sub, rot=rot,
                mass=_np(mx.body_mass).astype(HP), subtreemass=_np(mx.body_subtreemass).astype(HP), inertia=_np(mx.body_inertia).astype(HP).reshape(nb, 3))


def leaves_of(src):
    """The leaves the definitions read, [B, ...] host arrays, from a batched Data (one batch dimension) or a dict of arrays (an oracle pass)."""
    get = (lambda n: np.asarray(src[n])) if isinstance(src, dict) else (lambda n: _np(getattr(src, n)))
    out = {n: get(n) for n in LEAVES}
    B = out["cdof"].shape[0]
    shapes = dict(cdof=(-1, 6), cdof_dot=(-1, 6), cvel=(-1, 6), subtree_com=(-1, 3), xipos=(-1, 3), ximat=(-1, 3, 3))
    return {n: v.reshape((B,) + shapes[n]) for n, v in out.items()}


def _cr(a, b, s):
    """cross(a, b) along the last axis for s = -1; for s = +1 the sum of the absolute products (of absolute inputs)."""
    return np.stack([a[..., 1] * b[..., 2] + s * (a[..., 2] * b[..., 1]), a[..., 2] * b[..., 0] + s * (a[..., 0] * b[..., 2]),
                     a[..., 0] * b[..., 1] + s * (a[..., 1] * b[..., 0])], -1)


def _points(point, B, P):
    point = np.asarray(point)
    if point.ndim == 1:
        return np.broadcast_to(point, (B, P, 3))
    if point.ndim == 2:
        return np.broadcast_to(point[:, None, :], (B, P, 3))
    return point


def _both(fn):
    """(value, S_abs) of fn(g, s): g maps an input to what enters (itself / its absolute value), s is the sign of a subtraction."""
    return fn(lambda x: x, -1), fn(np.abs, +1)


def _hp(L):
    return {n: np.asarray(L[n], dtype=HP) for n in L}


def _subtree(T, L, body, g, s):
    """[B, nv, 3]: the subtree-com matrix of `body`."""
    cd, com = g(L["cdof"]), L["subtree_com"]
    acc = np.zeros(cd.shape[:2] + (3,), dtype=HP)
    for b in np.nonzero(T["sub"][body])[0]:
        off = g(L["xipos"][:, b] - com[:, T["root"][b]])[:, None, :]
        j = (cd[..., 3:] + _cr(cd[..., :3], off, s)) * T["mask"][b].astype(HP)[None, :, None]
        acc = acc + g(T["mass"][b]) * j
    return acc / g(T["subtreemass"][body])


def subtree_com_hp(T, leaves, ids):
    """(value, S_abs, n), each [B, P, nv, 3]."""
    L = _hp(leaves)
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    val, mag = _both(lambda g, s: np.stack([_subtree(T, L, int(b), g, s) for b in ids], 1))
    # per body of the subtree three products; an entry of J_b has taken JACP_ROUNDINGS, then the mass, then the division
    n = np.array([3 * int(T["sub"][b].sum()) + JACP_ROUNDINGS + 2 for b in ids], dtype=np.int64)
    return val, mag, np.broadcast_to(n[None, :, None, None], val.shape)


def _angmom(T, L, body, g, s):
    cd, com = g(L["cdof"]), L["subtree_com"]
    sc = _subtree(T, L, body, g, s)
    acc = np.zeros_like(sc)
    for b in np.nonzero(T["sub"][body])[0]:
        on = T["mask"][b].astype(HP)[None, :, None]
        off = g(L["xipos"][:, b] - com[:, T["root"][b]])[:, None, :]
        j = (cd[..., 3:] + _cr(cd[..., :3], off, s)) * on
        w = j + s * sc  # J_b - sc; magnitudes add
        d = g(L["xipos"][:, b] - com[:, body])[:, None, :]
        R = g(L["ximat"][:, b])                                               # [B, 3, 3]
        loc = np.einsum("brc,bir->bic", R, cd[..., :3]) * g(T["inertia"][b])  # inertia * (R^T w_i)
        rot = np.einsum("brc,bic->bir", R, loc) * on
        acc = acc + (rot + g(T["mass"][b]) * _cr(d, w, s))
    return acc


def angmom_hp(T, leaves, ids):
    """(value, S_abs, n), each [B, P, nv, 3]."""
    L = _hp(leaves)
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    val, mag = _both(lambda g, s: np.stack([_angmom(T, L, int(b), g, s) for b in ids], 1))
    # per body: nine products of R I R^T w, and the cross product's two entries of (J_b - subtree matrix), 3 + 3 nsub products each, times d and the mass; a product's
    # path: the subtree matrix's own roundings, then the difference, the product with d, the cross product's subtraction, the mass, the sum with the rotational part
    nsub = np.array([int(T["sub"][b].sum()) for b in ids], dtype=np.int64)
    n = nsub * (9 + 2 * (3 + 3 * nsub)) + (3 * nsub + JACP_ROUNDINGS + 2) + 5
    return val, mag, np.broadcast_to(n[None, :, None, None], val.shape)


def _dot(T, L, point, ids, g, s):
    cd, cdd, com, cvel = g(L["cdof"]), g(L["cdof_dot"]), L["subtree_com"], g(L["cvel"])
    wd, vd = cdd[..., :3].copy(), cdd[..., 3:].copy()
    for i in np.nonzero(T["rot"])[0]:
        Vb = cvel[:, T["dof_body"][i]]
        wd[:, i] = _cr(Vb[:, :3], cd[:, i, :3], s)
        vd[:, i] = _cr(Vb[:, :3], cd[:, i, 3:], s) + _cr(Vb[:, 3:], cd[:, i, :3], s)
    jp, jr = [], []
    for p, body in enumerate(ids):
        on = T["mask"][body].astype(HP)[None, :, None]
        off = g(point[:, p] - com[:, T["root"][body]])[:, None, :]
        V = cvel[:, body][:, None, :]
        pd = V[..., 3:] + _cr(V[..., :3], off, s)
        jp.append(((vd + _cr(wd, off, s)) + _cr(cd[..., :3], pd, s)) * on)
        jr.append(wd * on)
    return np.stack(jp, 1), np.stack(jr, 1)


def dot_hp(T, leaves, point, ids):
    """((jacp_dot, S_abs, n), (jacr_dot, S_abs, n)), each [B, P, nv, 3]."""
    L = _hp(leaves)
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    pt = np.asarray(_points(point, L["cdof"].shape[0], ids.shape[0]), dtype=HP)
    (vp, vr), (mp, mr) = _both(lambda g, s: _dot(T, L, pt, ids, g, s))
    # jacp_dot of a ball / free-rotation dof: vd 4 products, wd x off 4, w x pdot 2 + 4; the deepest product's path: off, W x off's product and subtraction, + U,
    # the product with w, the cross product's subtraction, the two additions of the three parts (8).  jacr_dot: wd's two products and its subtraction.
    return (vp, mp, np.full(vp.shape, 14 + 8, dtype=np.int64)), (vr, mr, np.full(vr.shape, 2 + 1, dtype=np.int64))


def point_hp(T, leaves, point, ids):
    """((jacp, S_abs, n), (jacr, S_abs, n)) of jac itself (``_support_ref.jac_hp``), each [B, P, nv, 3]."""
    from _support_ref import jac_hp

    (jp, ap), (jr, ar) = jac_hp(leaves["cdof"], leaves["subtree_com"], T["root"], T["mask"], point, ids)
    return (jp, ap, np.full(jp.shape, 3 + JACP_ROUNDINGS, dtype=np.int64)), (jr, ar, np.zeros(jr.shape, dtype=np.int64))


def product(triple, vec):
    """sum_i M[i, :] vec[i] of a (value, S_abs, n) matrix triple [B, P, nv, 3] with vec [B, nv]: (value, S_abs, n), each [B, P, 3]."""
    val, mag, n = triple
    q = np.asarray(vec, dtype=HP)[:, None, :, None]
    return (val * q).sum(2), (mag * np.abs(q)).sum(2), n.max(2) + val.shape[2]
