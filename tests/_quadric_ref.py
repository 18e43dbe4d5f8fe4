"""numpy longdouble restatement of the reference's plane_ellipsoid / plane_cylinder (collision_primitive.py:77-169, smooth_collisions off).

The yardstick of tests/test_quadric_host.py (pinned there against the reference's own recorded contacts) and of tests/test_quadric.py (evaluated on the
geom frames the GPU returned).  Operation by operation like the reference, in extended precision, with its quirks: math.sign is +1 at 0, math.norm is
zero-safe, normalize divides by n + 1e-6 (n == 0), the flat disc (len_ < 1e-12) takes mat[:, 0] * radius, the `par` test looks at prjaxis AFTER its scaling
by the half-length, and the sideways vector is scaled by torch.sqrt(torch.full((), 3.0)) * 0.5 -- a float32 value in every model dtype.
"""
import numpy as np

LD = np.longdouble
SQRT3_HALF = LD(np.sqrt(np.float32(3.0))) * LD(0.5)  # the float32-rounded sqrt(3), widened
FN_PLANE_ELLIPSOID, FN_PLANE_CYLINDER = 9, 10
PAR_EDGE = LD(1e-3)   # |prjaxis * half| below this: the cylinder lies on its side
FLAT_EDGE = LD(1e-12)  # len_ below this: the disc lies flat


def _ld(x):
    return np.asarray(x, dtype=LD)


def _norm(x):
    return LD(0) if not x.any() else np.sqrt((x * x).sum())


def _normalize(x):
    n = _norm(x)
    return x / (n + LD(1e-6) * LD(n == 0))


def make_frame(a):
    a = _normalize(_ld(a))
    b = _ld([0, 1, 0]) if -0.5 < a[1] < 0.5 else _ld([0, 0, 1])
    b = b - a * (a * b).sum()
    b = _normalize(b) * LD(a.any())
    return np.stack([a, b, np.cross(a, b)])


def plane_ellipsoid(ppos, pmat, epos, emat, size):
    """-> dist [1], pos [1, 3], frame [1, 3, 3]"""
    ppos, pmat, epos, emat, size = map(_ld, (ppos, pmat, epos, emat, size))
    n = pmat[:, 2]
    support = -_normalize((emat.T * n).sum(-1) * size)
    pos = epos + (emat * (support * size)).sum(-1)
    dist = (n * (pos - ppos)).sum()
    pos = pos - n * dist * LD(0.5)
    return np.array([dist]), pos[None], make_frame(n)[None]


def plane_cylinder(ppos, pmat, cpos, cmat, size):
    """-> dist [3], pos [3, 3], frame [3, 3, 3], {len, prj_half, par, flat, flipped}: the quantities the function's branches test
    (flipped: the axis was on the +normal side and has been turned round to point towards the plane)"""
    ppos, pmat, cpos, cmat, size = map(_ld, (ppos, pmat, cpos, cmat, size))
    n, axis = pmat[:, 2], cmat[:, 2]
    radius, half = size[0], size[1]
    prjaxis = (n * axis).sum()
    sign = LD(1) if prjaxis < 0 else LD(-1)  # -math.sign
    axis, prjaxis = axis * sign, prjaxis * sign
    dist0 = ((cpos - ppos) * n).sum()
    vec = axis * prjaxis - n
    len_ = _norm(vec)
    flat = bool(len_ < FLAT_EDGE)
    vec = cmat[:, 0] * radius if flat else vec / (len_ + LD(1e-15) * LD(len_ == 0)) * radius
    prjvec = (vec * n).sum()
    axis, prjaxis = axis * half, prjaxis * half
    prjvec1 = -prjvec * LD(0.5)
    vec1 = _normalize(np.cross(vec, axis)) * radius
    vec1 = vec1 * SQRT3_HALF
    d1 = dist0 + prjaxis + prjvec
    d2 = dist0 + prjaxis + prjvec1
    pos_disk = cpos + axis + np.stack([vec - n * d1 * LD(0.5), vec1 + vec * LD(-0.5) - n * d2 * LD(0.5), -vec1 + vec * LD(-0.5) - n * d2 * LD(0.5)])
    d3 = dist0 - prjaxis + prjvec
    par = bool(abs(prjaxis) < PAR_EDGE)
    if par:
        dist = np.array([d1, d3, d2])
        pos = np.stack([pos_disk[0], cpos + vec - axis - n * d3 * LD(0.5), pos_disk[2]])
    else:
        dist, pos = np.array([d1, d2, d2]), pos_disk
    info = dict(len=len_, prj_half=abs(prjaxis), par=par, flat=flat, flipped=bool(sign < 0))
    return dist, pos, np.stack([make_frame(n)] * 3), info


def pair_contacts(model, geom_xpos, geom_xmat):
    """The contacts of every plane-ellipsoid / plane-cylinder pair of ``model`` for ONE environment's geom frames ([ngeom, 3], [ngeom, 3, 3] or
    flat): a list of dict(pair, fn, geom1, geom2, dst [k] (contact slots; candidate indices with max_contact_points), dist, pos, frame, info)."""
    xpos = np.asarray(geom_xpos).reshape(-1, 3)
    xmat = np.asarray(geom_xmat).reshape(-1, 3, 3)
    size = np.asarray(model.geom_size.detach().cpu().numpy())
    out = []
    for pi, (fn, k, c, _) in enumerate(model.tables.pairs):
        if fn not in (FN_PLANE_ELLIPSOID, FN_PLANE_CYLINDER):
            continue
        g1, g2 = c.geom1, c.geom2
        info = {}
        if fn == FN_PLANE_ELLIPSOID:
            dist, pos, frame = plane_ellipsoid(xpos[g1], xmat[g1], xpos[g2], xmat[g2], size[g2])
        else:
            dist, pos, frame, info = plane_cylinder(xpos[g1], xmat[g1], xpos[g2], xmat[g2], size[g2])
        out.append(dict(pair=pi, fn=fn, geom1=g1, geom2=g2, dst=np.asarray(model.tables.pair_dst[pi][:k]), dist=dist, pos=pos, frame=frame, info=info))
    return out
