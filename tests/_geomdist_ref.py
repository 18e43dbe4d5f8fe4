"""numpy longdouble reference of ``geom_distance`` (csrc/mjh_geomdist.h states the definitions), vectorised over environments.

The yardstick of tests/test_geom_distance.py, pinned in tests/test_geom_distance_host.py on the recorded contacts of the goldens and, for the box parts, on
alternating projections and sampled support functions.  Beside the distance itself: a signed distance function per shape (``sdf``), the support function
(``support``) and an optimality certificate for a returned ``(dist, fromto)`` (``certificate``), which looks at the output alone.

n is the unit vector from geom1 towards geom2 and ``to - from = dist * n``.  A pair of cores (point, segment, box: kind 0, 1, 2) is worked in the frame of the
core of the higher kind ("B"); the other ("A") is c, U there.
"""
import numpy as np

LD = np.longdouble
PLANE, SPHERE, CAPSULE, ELLIPSOID, CYLINDER, BOX = 0, 2, 3, 4, 5, 6
KIND = {SPHERE: 0, CAPSULE: 1, BOX: 2}
NAMES = {PLANE: "plane", SPHERE: "sphere", CAPSULE: "capsule", ELLIPSOID: "ellipsoid", CYLINDER: "cylinder", BOX: "box"}
# |e_a x e_b|^2 at or below PAR2: the cross product is no axis and the edge pair counts as parallel; d_core at or below TINY * size: no direction.  The kernel's
# constants per dtype (mjh_geomdist.h GdConst): the reference takes the ones of the dtype it is compared with, so that both skip the same axes.
# "exact": nothing is skipped above longdouble noise -- the yardstick of the nearly-parallel poses, which shares no threshold with the kernel
CONSTS = {"exact": (LD(1e-34), LD(1e-13)), "float64": (LD(1e-24), LD(1e-13)), "float32": (LD(np.float32(1e-10)), LD(np.float32(1e-6)))}


def _ld(x):
    return np.asarray(x, dtype=LD)


def _dot(a, b):
    return (a * b).sum(-1)


def _half_axes(gtype, size):
    """(kind, half-axes [3], radius) of a sphere / capsule / box as a core plus a radius."""
    size = _ld(size)
    if gtype == SPHERE:
        return 0, _ld([0, 0, 0]), size[0]
    if gtype == CAPSULE:
        return 1, _ld([0, 0, size[1]]), size[0]
    return 2, size.copy(), LD(0)


def _corners(k, h):
    if k == 0:
        return [_ld([0, 0, 0])]
    if k == 1:
        return [_ld([0, 0, -h[2]]), _ld([0, 0, h[2]])]
    return [_ld([h[0] if v & 1 else -h[0], h[1] if v & 2 else -h[1], h[2] if v & 4 else -h[2]]) for v in range(8)]


def _edges(k, h):
    """[(axis, centre [3], half length)] of a core's edges; the segment is its own single edge."""
    if k == 0:
        return []
    if k == 1:
        return [(2, _ld([0, 0, 0]), h[2])]
    out = []
    for j in range(3):
        j1, j2 = (j + 1) % 3, (j + 2) % 3
        for s in range(4):
            c = _ld([0, 0, 0])
            c[j1], c[j2] = (h[j1] if s & 1 else -h[j1]), (h[j2] if s & 2 else -h[j2])
            out.append((j, c, h[j]))
    return out


def enumerate_cores(ka, kb, c, U, a, b, par2):
    """The fixed enumeration: -> (d2 [B], pa [B, 3], pb [B, 3]) in B's frame, first minimum."""
    cand = []
    for s in _corners(ka, a):  # corners of A onto B
        p = c + U @ s
        q = np.clip(p, -b, b)
        cand.append((_dot(p - q, p - q), p, q))
    for w in _corners(kb, b):  # corners of B onto A
        z = np.clip(np.einsum("bij,bi->bj", U, w - c), -a, a)
        p = c + np.einsum("bij,bj->bi", U, z)
        cand.append((_dot(p - w, p - w), p, np.broadcast_to(w, p.shape).copy()))
    # (the kernel's order: A's axis, B's axis, then B's edge outside A's)
    ea, eb = _edges(ka, a), _edges(kb, b)
    for ja in sorted({e[0] for e in ea}):
        for ib in sorted({e[0] for e in eb}):
            for (_, cb, lb) in [e for e in eb if e[0] == ib]:
                for (_, cal, la) in [e for e in ea if e[0] == ja]:
                    ca = c + U @ cal
                    u = U[:, :, ja]
                    r = ca - cb
                    cc, f, bb = _dot(u, r), r[:, ib], u[:, ib]
                    i1, i2 = (ib + 1) % 3, (ib + 2) % 3
                    denom = u[:, i1] ** 2 + u[:, i2] ** 2  # sin^2 of the angle between the edges, without cancellation
                    skew = denom > par2
                    s = np.where(skew, np.clip(-(u[:, i1] * r[:, i1] + u[:, i2] * r[:, i2]) / np.where(skew, denom, 1), -la, la), 0)
                    t = bb * s + f
                    tc = np.clip(t, -lb, lb)
                    s = np.where(tc != t, np.clip(bb * tc - cc, -la, la), s)
                    pa = ca + u * s[:, None]
                    pb = np.broadcast_to(cb, pa.shape).copy()
                    pb[:, ib] = tc
                    cand.append((_dot(pa - pb, pa - pb), pa, pb))
    d2 = np.stack([x[0] for x in cand])
    k = np.argmin(d2, 0)
    e = np.arange(d2.shape[1])
    return d2[k, e], np.stack([x[1] for x in cand])[k, e], np.stack([x[2] for x in cand])[k, e]


def separation(ka, c, U, a, b, par2):
    """Largest signed separation of core A from the box B over the face normals and the edge cross products: (sep [B], n [B, 3] from A towards B)."""
    nB = c.shape[0]
    axes = [(np.broadcast_to(np.eye(3, dtype=LD)[i], (nB, 3)), np.ones(nB, bool)) for i in range(3)]
    if ka == 2:
        axes += [(U[:, :, j], np.ones(nB, bool)) for j in range(3)]
    if ka >= 1:
        for i in range(3):
            for j in (range(3) if ka == 2 else (2,)):
                m = np.cross(np.broadcast_to(np.eye(3, dtype=LD)[i], (nB, 3)), U[:, :, j])
                m2 = _dot(m, m)
                ok = m2 > par2
                axes.append((m / np.sqrt(np.where(ok, m2, 1))[:, None], ok))
    seps, ns = [], []
    for d, ok in axes:
        cd = _dot(c, d)
        reach = sum(a[j] * np.abs(_dot(U[:, :, j], d)) + b[j] * np.abs(d[:, j]) for j in range(3))
        seps.append(np.where(ok, np.abs(cd) - reach, -np.inf))
        ns.append(np.where((cd > 0)[:, None], -d, d))
    seps = np.stack(seps)
    k = np.argmax(seps, 0)
    e = np.arange(nB)
    return seps[k, e], np.stack(ns)[k, e]


def core_pair(ka, kb, c, U, a, b, ra, rb, zdir, consts):
    """Cores A, B (ka <= kb) with radii in B's frame: dict(dist, on_a, on_b, n, overlap (cores), nodir) over the environments."""
    par2, tiny = consts
    nB = c.shape[0]
    if kb == 2:
        sep, n = separation(ka, c, U, a, b, par2)
        overlap = sep <= 0
    else:
        sep, overlap = np.ones(nB, dtype=LD), np.zeros(nB, bool)
        # the direction where the cores leave none: the world +z for two points; with a segment a unit vector perpendicular to it (B's x axis, or for two
        # segments the cross product of the axes unless they are parallel), so that a point moved by a radius along it stays on the capsule's surface
        n = zdir.copy() if kb == 0 else np.broadcast_to(_ld([1, 0, 0]), (nB, 3)).copy()
        if ka == 1 and kb == 1:
            m = np.stack([U[:, 1, 2], -U[:, 0, 2], np.zeros(nB, dtype=LD)], -1)  # U[:, :, 2] x e_z
            m2 = _dot(m, m)
            n = np.where((m2 > par2)[:, None], m / np.sqrt(np.where(m2 > par2, m2, 1))[:, None], n)
    cs = np.where(overlap[:, None], c + sep[:, None] * n, c)
    d2, pa, pb = enumerate_cores(ka, kb, cs, U, a, b, par2)
    d = np.sqrt(d2)
    nodir = ~overlap & ~(d > tiny * (ra + rb + a.sum() + b.sum()))
    unit = (pb - pa) / np.where(d > 0, d, 1)[:, None]
    n = np.where((overlap | nodir)[:, None], n, unit)
    qa = np.where(overlap[:, None], pb - sep[:, None] * n, pa)
    dcore = np.where(overlap, sep, d)
    return dict(dist=dcore - ra - rb, on_a=qa + ra * n, on_b=pb - rb * n, n=n, overlap=overlap, nodir=nodir)


def plane_pair(ppos, pmat, gtype, size, pos, mat):
    """Plane against a body: (dist [B], on_plane [B, 3], on_body [B, 3])."""
    size = _ld(size)
    npl = pmat[:, :, 2]
    nl = np.einsum("bij,bi->bj", mat, npl)
    sgn = np.where(nl < 0, LD(1), LD(-1))
    s, rad = np.zeros_like(nl), LD(0)
    if gtype == SPHERE:
        rad = size[0]
    elif gtype == CAPSULE:
        rad = size[0]
        s[:, 2] = sgn[:, 2] * size[1]
    elif gtype == BOX:
        s = sgn * size
    elif gtype == ELLIPSOID:
        v = size * nl
        ln = np.sqrt(_dot(v, v))
        s = -size * v / np.where(ln > 0, ln, 1)[:, None]
    elif gtype == CYLINDER:
        ln = np.sqrt(nl[:, 0] ** 2 + nl[:, 1] ** 2)
        s[:, :2] = -nl[:, :2] * (np.where(ln > 0, size[0] / np.where(ln > 0, ln, 1), 0))[:, None]
        s[:, 2] = sgn[:, 2] * size[1]
    else:
        raise NotImplementedError(gtype)
    on_body = pos + np.einsum("bij,bj->bi", mat, s) - rad * npl
    dist = _dot(npl, on_body - ppos)
    return dist, on_body - dist[:, None] * npl, on_body


def pair_distance(t1, size1, pos1, mat1, t2, size2, pos2, mat2, dtype="float64"):
    """One pair over B environments: dict(dist [B], from [B, 3], to [B, 3], overlap [B] (of the cores), nodir [B]).  Positions [B, 3], frames [B, 3, 3]."""
    pos1, mat1, pos2, mat2 = map(_ld, (pos1, mat1, pos2, mat2))
    nB = pos1.shape[0]
    none = np.zeros(nB, bool)
    if t1 == PLANE and t2 != PLANE:
        dist, on_plane, on_body = plane_pair(pos1, mat1, t2, size2, pos2, mat2)
        return {"dist": dist, "from": on_plane, "to": on_body, "overlap": none, "nodir": none}
    if t2 == PLANE and t1 != PLANE:
        dist, on_plane, on_body = plane_pair(pos2, mat2, t1, size1, pos1, mat1)
        return {"dist": dist, "from": on_body, "to": on_plane, "overlap": none, "nodir": none}
    if t1 not in KIND or t2 not in KIND:
        raise NotImplementedError(f"{NAMES.get(t1, t1)}-{NAMES.get(t2, t2)}")
    swap = KIND[t1] > KIND[t2]
    A, B = ((t2, size2, pos2, mat2), (t1, size1, pos1, mat1)) if swap else ((t1, size1, pos1, mat1), (t2, size2, pos2, mat2))
    ka, a, ra = _half_axes(A[0], A[1])
    kb, b, rb = _half_axes(B[0], B[1])
    c = np.einsum("bij,bi->bj", B[3], A[2] - B[2])
    U = np.einsum("bki,bkj->bij", B[3], A[3])
    r = core_pair(ka, kb, c, U, a, b, ra, rb, B[3][:, 2, :].copy(), CONSTS[dtype])
    on_a = B[2] + np.einsum("bij,bj->bi", B[3], r["on_a"])
    on_b = B[2] + np.einsum("bij,bj->bi", B[3], r["on_b"])
    return {"dist": r["dist"], "from": on_b if swap else on_a, "to": on_a if swap else on_b, "overlap": r["overlap"], "nodir": r["nodir"]}


def evaluate(rows, size, xpos, xmat, distmax=None, dtype="float64"):
    """``rows`` [P, 4] (geom1, geom2, type1, type2), ``size`` [ngeom, 3], frames [B, ngeom, 3] / [B, ngeom, 3, 3] -> dict(dist [B, P], fromto [B, P, 6],
    overlap [B, P], nodir [B, P]); with ``distmax`` the cut is applied."""
    xpos, xmat = _ld(xpos), _ld(xmat).reshape(xpos.shape[0], -1, 3, 3)
    out = {k: [] for k in ("dist", "fromto", "overlap", "nodir")}
    for g1, g2, t1, t2 in np.asarray(rows).tolist():
        r = pair_distance(t1, size[g1], xpos[:, g1], xmat[:, g1], t2, size[g2], xpos[:, g2], xmat[:, g2], dtype)
        dist, ft = r["dist"], np.concatenate([r["from"], r["to"]], -1)
        if distmax is not None:
            cut = dist > LD(distmax)
            dist, ft = np.where(cut, LD(distmax), dist), np.where(cut[:, None], LD(0), ft)
        out["dist"].append(dist)
        out["fromto"].append(ft)
        out["overlap"].append(r["overlap"])
        out["nodir"].append(r["nodir"])
    return {k: np.stack(v, 1) for k, v in out.items()}


# ---- signed distance and support functions ----------------------------------------------------------------------------------------------

def sdf(gtype, size, pos, mat, x):
    """Signed distance of the points x [B, 3] from the geom's surface (negative inside); the ellipsoid's is first order in the distance."""
    size, pos, mat, x = _ld(size), _ld(pos), _ld(mat), _ld(x)
    y = np.einsum("bij,bi->bj", mat, x - pos)
    if gtype == PLANE:
        return y[:, 2]
    if gtype == SPHERE:
        return np.sqrt(_dot(y, y)) - size[0]
    if gtype == CAPSULE:
        y = y.copy()
        y[:, 2] -= np.clip(y[:, 2], -size[1], size[1])
        return np.sqrt(_dot(y, y)) - size[0]
    if gtype == BOX:
        q = np.abs(y) - size
        return np.sqrt(_dot(np.maximum(q, 0), np.maximum(q, 0))) + np.minimum(q.max(-1), 0)
    if gtype == CYLINDER:
        q = np.stack([np.sqrt(y[:, 0] ** 2 + y[:, 1] ** 2) - size[0], np.abs(y[:, 2]) - size[1]], -1)
        return np.sqrt(_dot(np.maximum(q, 0), np.maximum(q, 0))) + np.minimum(q.max(-1), 0)
    if gtype == ELLIPSOID:
        k0, k1 = np.sqrt(_dot(y / size, y / size)), np.sqrt(_dot(y / size**2, y / size**2))
        return k0 * (k0 - 1) / np.where(k1 > 0, k1, 1)
    raise NotImplementedError(gtype)


def support(gtype, size, pos, mat, d):
    """max over the geom of d . x for unit d [B, 3] (sphere, capsule, box)."""
    size, pos, mat, d = _ld(size), _ld(pos), _ld(mat), _ld(d)
    dl = np.abs(np.einsum("bij,bi->bj", mat, d))
    k, h, r = _half_axes(gtype, size)
    return _dot(d, pos) + _dot(dl, h) + r


def certificate(t1, size1, pos1, mat1, t2, size2, pos2, mat2, dist, fromto):
    """Residuals of a returned (dist [B], fromto [B, 6]) of a sphere / capsule / box pair, from the output alone: dict(on1, on2: |sdf| of the two points;
    length: ||to - from| - |dist||; gap: dist minus the support gap along n = (to - from) / dist (positive: the claimed distance is not a lower bound)).
    on1, on2 and length make dist an upper bound on the true distance, gap a lower bound."""
    dist, fromto = _ld(dist), _ld(fromto)
    fr, to = fromto[:, :3], fromto[:, 3:]
    diff = to - fr
    ln = np.sqrt(_dot(diff, diff))
    n = diff / np.where(dist != 0, dist, 1)[:, None]
    n = n / np.where(ln > 0, np.sqrt(_dot(n, n)), 1)[:, None]
    gap = -support(t2, size2, pos2, mat2, -n) - support(t1, size1, pos1, mat1, n)
    return dict(on1=np.abs(sdf(t1, size1, pos1, mat1, fr)), on2=np.abs(sdf(t2, size2, pos2, mat2, to)), length=np.abs(ln - np.abs(dist)), gap=dist - gap)


# ---- what the tests share -----------------------------------------------------------------------------------------------------------------

def supported(t1, t2):
    return (t1 in KIND and t2 in KIND) or (t1 == PLANE and t2 in (SPHERE, CAPSULE, BOX, ELLIPSOID, CYLINDER)) or (t2 == PLANE and t1 in (SPHERE, CAPSULE, BOX, ELLIPSOID, CYLINDER))


def all_rows(gtype):
    """Every supported ordered pair of distinct geoms of a model with geom types ``gtype``: [P, 4] int32 (geom1, geom2, type1, type2)."""
    gtype = [int(t) for t in gtype]
    return np.array([(i, j, a, b) for i, a in enumerate(gtype) for j, b in enumerate(gtype) if i != j and supported(a, b)], dtype=np.int32)


def random_rotations(rng, n):
    """n rotation matrices [n, 3, 3] (float64, orthonormal to rounding) from seeded unit quaternions."""
    q = rng.randn(n, 4)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], 1)


def reach(gtype, size):
    """Radius of a ball about the geom's centre that holds it (the plane: 0)."""
    s = np.asarray(size, dtype=np.float64)
    return {PLANE: 0.0, SPHERE: s[0], CAPSULE: s[0] + s[1], BOX: float(np.linalg.norm(s)), ELLIPSOID: float(s.max()), CYLINDER: float(np.hypot(s[0], s[1]))}[gtype]


def axis_angle(axis, angle):
    """Rotation matrices [n, 3, 3] about ``axis`` [n, 3] by ``angle`` [n] (Rodrigues)."""
    axis = np.asarray(axis, dtype=np.float64)
    axis = axis / np.linalg.norm(axis, axis=-1, keepdims=True)
    K = np.zeros(axis.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0], K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -axis[..., 2], axis[..., 1], axis[..., 2], -axis[..., 0], -axis[..., 1], axis[..., 0]
    angle = np.asarray(angle, dtype=np.float64)[..., None, None]
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)
