"""A plain numpy reference of rne_postconstraint / subtree_vel (MuJoCo's mj_rnePostConstraint / mj_subtreeVel), for the tests only.

It restates the definitions in the header of csrc/mjh_postcon.h with per-body loops, in ``HP`` (``numpy.longdouble`` where that is wider than
float64, as tests/_support_ref.py).  Spatial vectors are [rotational(3), translational(3)] in the world frame about subtree_com[root(b)];
move(w, from, to) of a wrench [t, f] is t' = t - (to - from) x f.

``evaluate`` returns, for each of the five leaves, ``(value, S, n)``:
* ``S`` -- the same expression with every product term replaced by its absolute value (every subtraction becomes an addition of magnitudes, so
  cancellation never shrinks it); it is obtained by running the very same code on the magnitudes of the inputs with ``s = +1`` in place of ``s = -1``;
* ``n`` -- the number of additions on the longest path of accumulated terms behind the element (sums are nested, so path lengths add: a subtree sum
  of forces that each carry an ancestor-chain sum counts both), worked out from the tree below (``term_counts``).
The element-wise bound used by every comparison is ``bound(n, eps, S) = (n + 16) (eps + EPS_HP) S``: the forward bound of recursive summation
(Higham, Accuracy and Stability of Numerical Algorithms, section 4.2) over the n accumulated terms, the 16 covering the fixed depth of products and
small fixed sums inside one term (a rotation by a 3 x 3 matrix, a cross product, inert_mul: at most 3 + 2 + 3 + 2 + ... roundings deep).
"""
import numpy as np

HP = np.longdouble if np.finfo(np.longdouble).eps < np.finfo(np.float64).eps else np.float64
EPS_HP = float(np.finfo(HP).eps)
MINVAL = 1e-15  # mjMINVAL
ACCELEROMETER, FORCE, TORQUE, SUBTREELINVEL, SUBTREEANGMOM = 1, 4, 5, 36, 37


def bound(n, eps, s_abs):
    return (np.asarray(n, dtype=np.float64) + 16.0) * (float(eps) + EPS_HP) * np.asarray(s_abs, dtype=np.float64)


def tables(mx):
    """The model constants the definitions use, as host arrays (values in the model's dtype, widened)."""
    A = lambda n: np.asarray(getattr(mx, n).detach().cpu().numpy() if hasattr(getattr(mx, n), "detach") else getattr(mx, n))
    parent = A("body_parentid").astype(np.int64)
    nb = parent.shape[0]
    end = np.arange(1, nb + 1)
    for b in range(nb - 1, 0, -1):  # bodies are in DFS order: a subtree is a contiguous range
        end[parent[b]] = max(end[parent[b]], end[b])
    grav = np.asarray(mx.opt.gravity.detach().cpu().numpy())
    if int(mx.opt.disableflags) & (1 << 7):  # DisableBit.GRAVITY
        grav = np.zeros(3)
    return dict(nbody=nb, parent=parent, root=A("body_rootid").astype(np.int64), dofadr=A("body_dofadr").astype(np.int64), dofnum=A("body_dofnum").astype(np.int64),
                end=end, geom_bodyid=A("geom_bodyid").astype(np.int64), mass=A("body_mass").astype(HP), inertia=A("body_inertia").astype(HP).reshape(nb, 3),
                subtreemass=A("body_subtreemass").astype(HP), gravity=np.asarray(grav, dtype=HP), pyramidal=int(mx.opt.cone) == 0)


def _cross(a, b, s):
    return np.array([a[1] * b[2] + s * (a[2] * b[1]), a[2] * b[0] + s * (a[0] * b[2]), a[0] * b[1] + s * (a[1] * b[0])])


def _inert_mul(i, v, s):
    pos, mass = i[6:9], i[9]
    c1, c2 = _cross(pos, v[3:], s), _cross(pos, v[:3], s)
    rot = np.array([i[0] * v[0] + i[3] * v[1] + i[4] * v[2], i[3] * v[0] + i[1] * v[1] + i[5] * v[2], i[4] * v[0] + i[5] * v[1] + i[2] * v[2]]) + c1
    return np.concatenate([rot, mass * v[3:] + s * c2])


def _cross_force(v, f, s):
    return np.concatenate([_cross(v[:3], f[:3], s) + _cross(v[3:], f[3:], s), _cross(v[:3], f[3:], s)])


def _move(t, f, frm, to, s):
    return np.concatenate([t + s * _cross(to + s * frm, f, s), f])


def contact_wrench(T, L, c, s):
    """(b1, b2, torque, force) of contact slot c in the world frame at contact.pos, or None for a skipped slot."""
    g1, g2 = int(L["contact_geom"][c, 0]), int(L["contact_geom"][c, 1])
    if g1 < 0 or g2 < 0:
        return None
    dim, adr = int(L["contact_dim"][c]), int(L["contact_efc_address"][c])
    w = np.zeros(6, dtype=L["contact_pos"].dtype)
    if not T["pyramidal"] or dim == 1:
        w[:dim] = L["efc_force"][adr:adr + dim]
    else:
        p = L["efc_force"][adr:adr + 2 * (dim - 1)]
        w[0] = p.sum()
        for k in range(1, dim):
            w[k] = (p[2 * (k - 1)] + s * p[2 * (k - 1) + 1]) * L["contact_friction"][c, k - 1]
    F = L["contact_frame"][c].reshape(3, 3)
    return int(T["geom_bodyid"][g1]), int(T["geom_bodyid"][g2]), F.T @ w[3:], F.T @ w[:3]


def _eval_env(T, L, s, rne=True, subtree=True):
    """One environment.  s = -1: the values, from the leaves; s = +1: the magnitudes, from the leaves' absolute values."""
    nb, parent, root, end = T["nbody"], T["parent"], T["root"], T["end"]
    com, xipos, cvel = L["subtree_com"], L["xipos"], L["cvel"]
    dt = cvel.dtype
    out = {}
    if rne:
        ext = np.zeros((nb, 6), dtype=dt)
        for b in range(1, nb):
            ext[b] = _move(L["xfrc_applied"][b, 3:], L["xfrc_applied"][b, :3], xipos[b], com[root[b]], s)
        for c in range(L["contact_geom"].shape[0] if L.get("efc_force") is not None and L["efc_force"].shape[0] else 0):
            cw = contact_wrench(T, L, c, s)
            if cw is None:
                continue
            b1, b2, tq, fc = cw
            if b1 != 0:
                ext[b1] = ext[b1] + s * _move(tq, fc, L["contact_pos"][c], com[root[b1]], s)
            if b2 != 0:
                ext[b2] = ext[b2] + _move(tq, fc, L["contact_pos"][c], com[root[b2]], s)
        cacc = np.zeros((nb, 6), dtype=dt)
        cacc[0, 3:] = T["gravity"] if s > 0 else -T["gravity"]
        loc = np.zeros((nb, 6), dtype=dt)
        for b in range(nb):
            if b > 0:
                a = cacc[parent[b]].copy()
                for i in range(T["dofadr"][b], T["dofadr"][b] + T["dofnum"][b]):
                    a = a + (L["cdof_dot"][i] * L["qvel"][i] + L["cdof"][i] * L["qacc"][i])
                cacc[b] = a
            loc[b] = _inert_mul(L["cinert"][b], cacc[b], s) + _cross_force(cvel[b], _inert_mul(L["cinert"][b], cvel[b], s), s) + s * ext[b]
        out["cfrc_ext"], out["cacc"] = ext, cacc
        out["cfrc_int"] = np.stack([loc[b:end[b]].sum(0) for b in range(nb)])
    if subtree:
        v = np.stack([cvel[b, 3:] + s * _cross(xipos[b] + s * com[root[b]], cvel[b, :3], s) for b in range(nb)])
        mv = T["mass"][:, None] * v
        lin = np.stack([mv[b:end[b]].sum(0) / max(dt.type(MINVAL), T["subtreemass"][b]) for b in range(nb)])
        am = np.zeros((nb, 3), dtype=dt)
        for b in range(nb):
            R = L["ximat"][b].reshape(3, 3)
            am[b] = R @ (T["inertia"][b] * (R.T @ cvel[b, :3]))
        for b in range(nb - 1, -1, -1):
            am[b] = am[b] + _cross(xipos[b] + s * com[b], T["mass"][b] * (v[b] + s * lin[b]), s)
            if b > 0:  # (MuJoCo's walk ends above the world body, whose parent is itself)
                p = parent[b]
                am[p] = am[p] + (am[b] + _cross(com[b] + s * com[p], T["subtreemass"][b] * (lin[b] + s * lin[p]), s))
        out["subtree_linvel"], out["subtree_angmom"] = lin, am
    return out


def term_counts(T, ncon):
    """n per body for each leaf: additions on the longest path of accumulated terms (see the module docstring)."""
    nb, parent, end = T["nbody"], T["parent"], T["end"]
    chain = np.zeros(nb, dtype=np.int64)  # dofs on the chain world -> b
    for b in range(1, nb):
        chain[b] = chain[parent[b]] + T["dofnum"][b]
    n_ext = np.full(nb, 1 + 2 * ncon + 10)   # xfrc, two wrenches per contact slot, the pyramid's sum over at most ten rows
    n_ext[0] = 0
    n_cacc = 1 + 2 * chain                   # the base, two products per dof on the chain
    n_loc = n_cacc + n_ext + 8               # cinert cacc and cvel x* (cinert cvel): two fixed sums of products, minus cfrc_ext
    n_int = np.array([(end[b] - b) + n_loc[b:end[b]].max() for b in range(nb)])
    n_lin = np.array([(end[b] - b) + 4 for b in range(nb)])  # the subtree sum over mass * v (v: a leaf entry minus a cross product), the division
    n_am = np.zeros(nb, dtype=np.int64)
    kids = [[c for c in range(b + 1, end[b]) if parent[c] == b] for b in range(nb)]
    for b in range(nb - 1, -1, -1):  # what the children hand up (each carrying its own path and two subtree velocities), the body's own term
        n_am[b] = 6 + 2 * n_lin[b] + 2 * len(kids[b]) + max([n_am[c] for c in kids[b]], default=0)
    six, three = (lambda n: np.repeat(np.asarray(n)[:, None], 6, 1)), (lambda n: np.repeat(np.asarray(n)[:, None], 3, 1))
    return dict(cfrc_ext=six(n_ext), cacc=six(n_cacc), cfrc_int=six(n_int), subtree_linvel=three(n_lin), subtree_angmom=three(n_am))


LEAVES = ("qvel", "qacc", "cdof", "cdof_dot", "cvel", "cinert", "xipos", "ximat", "subtree_com", "xfrc_applied", "efc_force", "contact_pos", "contact_frame",
          "contact_friction", "contact_dim", "contact_geom", "contact_efc_address")
_INT = ("contact_dim", "contact_geom", "contact_efc_address")


def evaluate(T, leaves, rne=True, subtree=True, dtype=HP):
    """leaves: name -> array with ONE leading environment axis (contact_* and efc_force may be absent or empty).  Returns name -> (value, S, n),
    each [B, nbody, 6 or 3]; value and S in ``dtype`` (HP; float64 to see the rounding of a float64 evaluation of the same definitions)."""
    B = np.asarray(leaves["cvel"]).shape[0]
    ncon = int(np.asarray(leaves["contact_geom"]).shape[1]) if leaves.get("contact_geom") is not None and leaves.get("efc_force") is not None and np.asarray(leaves["efc_force"]).shape[1] else 0
    n = term_counts(T, ncon)
    T = dict(T, **{k: T[k].astype(dtype) for k in ("mass", "inertia", "subtreemass", "gravity")})
    Ta = dict(T, mass=np.abs(T["mass"]), inertia=np.abs(T["inertia"]), subtreemass=np.abs(T["subtreemass"]), gravity=np.abs(T["gravity"]))
    vals, mags = [], []
    for e in range(B):
        L = {k: (np.asarray(v[e]) if k in _INT else np.asarray(v[e], dtype=dtype)) for k, v in leaves.items() if v is not None}
        La = {k: (v if k in _INT else np.abs(v)) for k, v in L.items()}
        vals.append(_eval_env(T, L, -1, rne, subtree))
        mags.append(_eval_env(Ta, La, +1, rne, subtree))
    return {k: (np.stack([v[k] for v in vals]), np.stack([m[k] for m in mags]), np.broadcast_to(n[k], (B,) + n[k].shape)) for k in vals[0]}


def site_sensor(kind, R, pos, com_root, cvel, cacc=None, cfrc_int=None):
    """The accelerometer / force / torque formulas of sensor_value (csrc/mjh_sensor.h) for one site on one body, in HP: R the site's xmat (3 x 3),
    pos its xpos, com_root the subtree_com of the body's root."""
    R, dif = np.asarray(R, dtype=HP).reshape(3, 3), np.asarray(pos, dtype=HP) - np.asarray(com_root, dtype=HP)
    if kind == FORCE:
        return R.T @ np.asarray(cfrc_int, dtype=HP)[3:]
    if kind == TORQUE:
        cf = np.asarray(cfrc_int, dtype=HP)
        return R.T @ (cf[:3] - np.cross(dif, cf[3:]))
    cv, ca = np.asarray(cvel, dtype=HP), np.asarray(cacc, dtype=HP)
    lin = R.T @ (cv[3:] - np.cross(dif, cv[:3]))
    ang = R.T @ cv[:3]
    return R.T @ (ca[3:] - np.cross(dif, ca[:3])) + np.cross(ang, lin)


def leaves_of(d, names=LEAVES):
    """The leaves ``evaluate`` reads from a batched Data (one batch dimension), as host arrays."""
    out = {}
    for n in names:
        t = getattr(d.contact, {"contact_dim": "contact_dim"}.get(n, n[len("contact_"):])) if n.startswith("contact_") else getattr(d, n)
        out[n] = t.detach().cpu().numpy()
    return out


# ---- the joint-projection identity -------------------------------------------------------------------------------------------------------
# For every dof i of body b:  cdof[i] . cfrc_int[b] = (qM qacc)[i] - dof_armature[i] qacc[i] + qfrc_bias[i] - (J^T cfrc_ext)[i]
# (the subtree's Newton-Euler balance projected on the joint axis; qM carries the armature on its diagonal, the bodies do not).  It uses no solver
# output other than qacc itself.  J^T cfrc_ext = xfrc_accumulate + apply_ft of every contact's world wrench at contact.pos: -W on body 1, +W on body 2.

def contact_queries(T, leaves, e, dtype):
    """The apply_ft queries of environment e's contacts: (points [P, 3], forces, torques, body ids [P]), P = 2 ncon; a skipped slot is a zero force on the world body."""
    has = leaves.get("efc_force") is not None and np.asarray(leaves["efc_force"]).shape[1] > 0
    ncon = int(np.asarray(leaves["contact_geom"]).shape[1]) if has else 0
    L = {k: (np.asarray(v[e]) if k in _INT else np.asarray(v[e], dtype=dtype)) for k, v in leaves.items() if v is not None}
    pts, fo, to, ids = np.zeros((2 * ncon, 3), dtype=dtype), np.zeros((2 * ncon, 3), dtype=dtype), np.zeros((2 * ncon, 3), dtype=dtype), np.zeros(2 * ncon, dtype=np.int64)
    for c in range(ncon):
        cw = contact_wrench(T, L, c, -1)
        if cw is None:
            continue
        b1, b2, tq, fc = cw
        pts[2 * c] = pts[2 * c + 1] = L["contact_pos"][c]
        ids[2 * c], ids[2 * c + 1] = b1, b2
        fo[2 * c], to[2 * c], fo[2 * c + 1], to[2 * c + 1] = -fc, -tq, fc, tq
    return pts, fo, to, ids


def identity_scale(mx, leaves, qM):
    """The host's part of the identity: sum of |terms| of J^T cfrc_ext per dof ([B, nv], from tests/_support_ref.py's S_abs) and |qM| |qacc|."""
    import _support_ref as sr

    T = tables(mx)
    mask, root = sr.ancestor_mask(mx.body_parentid, mx.dof_bodyid), np.asarray(mx.body_rootid)
    _, s = sr.xfrc_hp(leaves["cdof"], leaves["subtree_com"], leaves["xipos"], leaves["xfrc_applied"], root, mask)
    B = np.asarray(leaves["cdof"]).shape[0]
    for e in range(B):
        pts, fo, to, ids = contact_queries(T, leaves, e, HP)
        if len(ids):
            s[e] = s[e] + sr.apply_ft_hp(leaves["cdof"][e:e + 1], leaves["subtree_com"][e:e + 1], root, mask, pts[None], fo[None], to[None], ids)[1][0].sum(0)
    return s.astype(np.float64) + (np.abs(np.asarray(qM, dtype=np.float64)) * np.abs(np.asarray(leaves["qacc"], dtype=np.float64))[:, None, :]).sum(-1)


def identity_ratio(mx, leaves, cfrc_int, Mq, bias, jt_ext, scale_host, eps):
    """max over (environment, dof) of |lhs - rhs| / (eps * sum |terms|); every array is [B, ...] in the Data dtype or wider."""
    f = lambda a: np.asarray(a, dtype=np.float64)
    dofb = np.asarray(mx.dof_bodyid).astype(np.int64)
    cd, ci, qa = f(leaves["cdof"]), f(cfrc_int)[:, dofb], f(leaves["qacc"])
    arm = f(mx.dof_armature.detach().cpu().numpy())
    lhs = (cd * ci).sum(-1)
    rhs = f(Mq) - arm * qa + f(bias) - f(jt_ext)
    S = np.abs(cd * ci).sum(-1) + np.abs(arm * qa) + np.abs(f(bias)) + scale_host
    return float((np.abs(lhs - rhs) / (eps * S)).max()), lhs, rhs


# The identity's constant in  |lhs - rhs| <= C eps sum|terms|  (tests/_postcon_ref.py identity_ratio), from evaluating it once with the reference in float64 on
# the five passes of tests/test_postconstraint_host.py (IDENTITY_MODELS): measured ratios 4.93 (humanoid), 0.41 (ant), 10.1 (capsules_topk: free bodies, whose cfrc_int cancels to nothing against the terms of the
# right side), 1.43 (equality), 0.60 (cartpole); 4 x the largest.
IDENTITY_C = 40.0


def within(got, want, allowed, what):
    err = np.abs(np.asarray(got, dtype=HP) - np.asarray(want, dtype=HP)).astype(np.float64)
    allowed = np.broadcast_to(np.asarray(allowed, dtype=np.float64), err.shape)
    i = np.unravel_index(np.argmax(err - allowed), err.shape) if err.size else ()
    assert (err <= allowed).all(), f"{what}: worst at {i}: error {err[i]:.3e}, allowed {allowed[i]:.3e}"
