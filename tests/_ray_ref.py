"""A plain numpy reference of ray casting with a running error bound, for the tests only.

The formulas are the reference project's ``_src/ray.py`` (``_ray_quad``, the primitives plane / sphere / capsule / ellipsoid / cylinder / box,
``_ray_triangle``), ``math.orthogonals(math.normalize(vec))`` and the frame change ``x.T @ (pnt - y)``, ``x.T @ vec``, evaluated in ``HP``
(``_support_ref.HP``) and vectorised over rays.  Nothing is read from the library: no kernel constant, no table.

Every value is a pair ``(v, e)``: the high-precision value and a rigorous bound of the distance between ``v`` and what an evaluation gives that
rounds every operation once in the Data dtype (the library is built without contraction or fast-math, so that is what the device does).

* Inputs enter with ``e = 0`` (or a stated error).
* ``+ - * / sqrt`` propagate the operand errors by the interval rule -- for a product ``|a| eb + |b| ea + ea eb``, for a quotient
  ``(|a| eb + |b| ea) / (|b| (|b| - eb))``, for a root ``e / (sqrt(v - e) + sqrt(v))`` -- and add the operation's own rounding
  ``(eps + EPS_HP) (|result| + propagated error)``, ``eps`` the dtype's ``finfo.eps`` as in ``_support_ref.bound``; a product or quotient
  that can fall below the smallest normal number adds the smallest subnormal instead of a relative error.
* A root or a quotient whose operand interval touches zero (and is not exactly zero) makes the ray *undecided*.
* A comparison is yes / no when the two intervals are apart and *maybe* when they overlap.  A ray is evaluated twice, every maybe taken as true
  and every maybe taken as false.  It is **decided** when both evaluations hit (their distance intervals overlapping, the ids equal or a tie of two
  geoms) or both miss; its value is then the hull of the two intervals.  Otherwise it is **left out**: its answer depends on a rounding.

``cast`` is ``ray`` (candidates in the table's order, the first minimum wins; ``mesh_strict`` applies the renderer's rule that a mesh wins
only when strictly closer and at a positive distance).  ``pixel_rays_ref`` evaluates the renderer's primary directions in the same arithmetic.
"""
import numpy as np

from _support_ref import EPS_HP, HP

MINVAL = 1e-15  # mujoco.mjMINVAL
MESH = 7


class Ctx:
    """One evaluation: the dtype whose roundings are bounded, how a maybe is taken, and the rays found undecided so far."""

    def __init__(self, dtype, n, maybe):
        self.dtype = np.dtype(dtype)
        fi = np.finfo(self.dtype)
        self.u = HP(float(fi.eps)) + HP(EPS_HP)
        self.min_normal, self.subnormal = HP(float(fi.tiny)), HP(float(fi.smallest_subnormal))
        self.n, self.maybe = n, bool(maybe)
        self.bad = np.zeros(n, dtype=bool)

    def value(self, x, e=None):
        """An input (already a value of the dtype) or a constant as the dtype holds it; with an error ``e``, a high-precision value as it is."""
        x = np.asarray(x)
        if e is None and (x.dtype.kind != "f" or x.dtype.itemsize > self.dtype.itemsize):
            x = x.astype(self.dtype)
        return Val(self, np.broadcast_to(x.astype(HP), (self.n,)), np.broadcast_to(np.asarray(0.0 if e is None else e, dtype=HP), (self.n,)))

    def zeros(self):
        return self.value(np.zeros(self.n))

    def _decide(self, yes, no):
        return np.where(yes, True, np.where(no, False, self.maybe))


class Val:
    __slots__ = ("c", "v", "e")

    def __init__(self, c, v, e):
        self.c, self.v, self.e = c, v, e

    def _lift(self, o):
        return o if isinstance(o, Val) else self.c.value(o)

    def _rounded(self, r, ep, scaled):
        c = self.c
        mag = np.abs(r) + ep
        rnd = c.u * mag
        if scaled:  # a product or a quotient can underflow: an absolute error of one subnormal there (zero stays exact)
            rnd = np.where((mag < c.min_normal) & (mag > 0), rnd + c.subnormal, rnd)
        return Val(c, r, ep + rnd)

    def __neg__(self):
        return Val(self.c, -self.v, self.e)

    def __abs__(self):
        return Val(self.c, np.abs(self.v), self.e)

    def __add__(self, o):
        o = self._lift(o)
        return self._rounded(self.v + o.v, self.e + o.e, False)

    __radd__ = __add__

    def __sub__(self, o):
        o = self._lift(o)
        return self._rounded(self.v - o.v, self.e + o.e, False)

    def __rsub__(self, o):
        return self._lift(o) - self

    def __mul__(self, o):
        o = self._lift(o)
        return self._rounded(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e, True)

    __rmul__ = __mul__

    def __truediv__(self, o):
        """Plain division: a divisor whose interval touches zero makes the ray undecided."""
        o = self._lift(o)
        touch = np.abs(o.v) <= o.e
        self.c.bad |= touch
        dv, de = np.where(touch, HP(1), o.v), np.where(touch, HP(0), o.e)
        ad = np.abs(dv)
        return self._rounded(self.v / dv, (np.abs(self.v) * de + ad * self.e) / (ad * (ad - de)), True)

    def __rtruediv__(self, o):
        return self._lift(o) / self

    def sqrt(self):
        """Of an operand that is exactly zero or whose interval lies above zero; an interval wholly below zero gives a value no later
        comparison can select (the callers test the operand's sign first); one that touches zero makes the ray undecided."""
        c = self.c
        exact0 = (self.v == 0) & (self.e == 0)
        below = self.v + self.e < 0
        touch = ~exact0 & ~below & (self.v - self.e <= 0)
        c.bad |= touch
        safe = ~(exact0 | below | touch)
        v, e = np.where(safe, self.v, HP(1)), np.where(safe, self.e, HP(0))
        r = np.sqrt(v)
        out = self._rounded(r, e / (np.sqrt(v - e) + r), False)
        return Val(c, np.where(safe, out.v, HP(0)), np.where(safe, out.e, HP(0)))

    # comparisons as the formulas write them: yes / no when the intervals are apart, else the evaluation's way of taking a maybe
    def lt(self, o):
        o = self._lift(o)
        return self.c._decide(self.v + self.e < o.v - o.e, self.v - self.e >= o.v + o.e)

    def le(self, o):
        o = self._lift(o)
        return self.c._decide(self.v + self.e <= o.v - o.e, self.v - self.e > o.v + o.e)

    def gt(self, o):
        return self._lift(o).lt(self)

    def ge(self, o):
        return self._lift(o).le(self)

    def eq0(self):
        return self.c._decide((self.v == 0) & (self.e == 0), np.abs(self.v) > self.e)


def where(cond, a, b):
    return Val(a.c, np.where(cond, a.v, b.v), np.where(cond, a.e, b.e))


def safe_div(num, den):
    """math.safe_div: num / (den + mjMINVAL * (den == 0)).  The product of the Python float and the boolean tensor is a float32 tensor in torch,
    so what is added to a zero denominator is float32(1e-15) in either dtype (the recorded float64 edge table shows it: 1 / that, not 1e15)."""
    c = den.c
    num = den._lift(num)
    zero = den.eq0()
    return num / where(zero, c.value(np.float32(MINVAL)), den)


def dot(a, b):
    s = a[0] * b[0]
    for x, y in zip(a[1:], b[1:]):
        s = s + x * y
    return s


class Dist:
    """A distance that may be a miss: ``x`` where ``ok``, infinity elsewhere."""
    __slots__ = ("x", "ok")

    def __init__(self, x, ok):
        self.x, self.ok = x, ok

    def closer(self, o):
        """self < o as the formulas write it between two distances (infinity is not less than anything; everything finite is less than it)."""
        return self.ok & (~o.ok | self.x.lt(o.x))

    def take(self, cond, o):
        """o where cond, else self."""
        return Dist(where(cond, o.x, self.x), np.where(cond, o.ok, self.ok))


def miss(c):
    return Dist(c.zeros(), np.zeros(c.n, dtype=bool))


def ray_quad(a, b, c):
    """_ray_quad: both roots of a x^2 + 2 b x + c = 0, infinity when det < mjMINVAL or the root is negative."""
    det = b * b - a * c
    det2 = det.sqrt()
    invalid = det.lt(MINVAL)
    r0, r1 = safe_div(-b - det2, a), safe_div(-b + det2, a)
    return Dist(r0, ~(invalid | r0.lt(0))), Dist(r1, ~(invalid | r1.lt(0)))


def _first(x0, x1):
    return x1.take(x0.ok, x0)  # where(isinf(x0), x1, x0)


def _plane(size, p, v):
    x = -safe_div(p[2], v[2])
    valid = v[2].le(-v[2].c.value(MINVAL)) & x.ge(0)
    for i in range(2):
        q = p[i] + x * v[i]
        valid = valid & ((size[i].v <= 0) | abs(q).le(size[i]))
    return Dist(x, valid)


def _sphere(size, p, v):
    return _first(*ray_quad(dot(v, v), dot(v, p), dot(p, p) - size[0] * size[0]))


def _round_side(size, p, v):
    x = _first(*ray_quad(dot(v[:2], v[:2]), dot(v[:2], p[:2]), dot(p[:2], p[:2]) - size[0] * size[0]))
    return Dist(x.x, x.ok & abs(p[2] + x.x * v[2]).le(size[1]))


def _capsule(size, p, v):
    x = _round_side(size, p, v)
    for sign in (1, -1):
        dif = [p[0], p[1], p[2] - size[1] if sign > 0 else p[2] + size[1]]
        for xi in ray_quad(dot(v, v), dot(v, dif), dot(dif, dif) - size[0] * size[0]):
            z = p[2] + xi.x * v[2]
            side = z.ge(size[1]) if sign > 0 else z.le(-size[1])
            x = x.take(side & xi.closer(x), xi)
    return x


def _cylinder(size, p, v):
    x = _round_side(size, p, v)
    for sign in (1, -1):
        t = safe_div((size[1] if sign > 0 else -size[1]) - p[2], v[2])
        q = [p[0] + t * v[0], p[1] + t * v[1]]
        cap = Dist(t, t.ge(0) & dot(q, q).le(size[0] * size[0]))
        x = x.take(cap.closer(x), cap)
    return x


def _ellipsoid(size, p, v):
    s = [safe_div(1.0, size[i] * size[i]) for i in range(3)]
    sv, sp = [s[i] * v[i] for i in range(3)], [s[i] * p[i] for i in range(3)]
    return _first(*ray_quad(dot(sv, v), dot(sv, p), dot(sp, p) - 1.0))


def _box(size, p, v):
    best = miss(p[0].c)
    iface = ((1, 2), (0, 2), (0, 1))
    for f in range(6):
        ax = f % 3
        i0, i1 = iface[ax]
        x = safe_div(size[ax] - p[ax], v[ax]) if f < 3 else -safe_div(size[ax] + p[ax], v[ax])
        q0, q1 = p[i0] + x * v[i0], p[i1] + x * v[i1]
        face = Dist(x, abs(q0).le(size[i0]) & abs(q1).le(size[i1]) & x.ge(0))
        best = best.take(face.closer(best), face)  # torch.min: any of equal values is the same value
    return best


_PRIMITIVE = {0: _plane, 2: _sphere, 3: _capsule, 4: _ellipsoid, 5: _cylinder, 6: _box}


def ray_geom_val(c, gtype, size, p, v):
    """The primitive's distance in its own frame.  size / p / v: lists of three Val."""
    return _PRIMITIVE[int(gtype)](size, p, v)


def ray_to_geom(xmat, xpos, pnt, vec):
    """x.T @ (pnt - y), x.T @ vec.  xmat: 9 Val (row-major), the rest 3 Val."""
    d = [pnt[i] - xpos[i] for i in range(3)]
    col = lambda i, w: xmat[i] * w[0] + xmat[3 + i] * w[1] + xmat[6 + i] * w[2]
    return [col(i, d) for i in range(3)], [col(i, vec) for i in range(3)]


def _normalize(c, x):
    """math.normalize: x / (n + 1e-6 (n == 0)), n = 0 for the zero vector."""
    zero = x[0].eq0() & x[1].eq0() & x[2].eq0()
    n = where(zero, c.zeros(), dot(x, x).sqrt())
    den = n + where(zero, c.value(1e-6), c.zeros())
    return [x[i] / den for i in range(3)]


def ray_basis(c, vec):
    """math.orthogonals(math.normalize(vec)): the two in-plane axes of _ray_mesh's basis."""
    a = _normalize(c, vec)
    ydir = a[1].gt(-0.5) & a[1].lt(0.5)
    one, zero = c.value(1.0), c.zeros()
    y = [zero, where(ydir, one, zero), where(ydir, zero, one)]
    ab = dot(a, y)
    bb = _normalize(c, [y[i] - a[i] * ab for i in range(3)])
    anynz = ~(a[0].eq0() & a[1].eq0() & a[2].eq0())
    b = [bb[i] * where(anynz, one, zero) for i in range(3)]
    return b, [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def ray_triangle(c, vert, p, v, b, cc):
    """_ray_triangle.  vert: 9 Val (three vertices)."""
    pl = []
    for i in range(3):
        d = [vert[3 * i + k] - p[k] for k in range(3)]
        pl.append((dot(d, b), dot(d, cc)))
    A00, A01, A10, A11 = pl[0][0] - pl[2][0], pl[0][1] - pl[2][1], pl[1][0] - pl[2][0], pl[1][1] - pl[2][1]
    b0, b1 = -pl[2][0], -pl[2][1]
    det = A00 * A11 - A10 * A01
    t0, t1 = safe_div(A11 * b0 - A10 * b1, det), safe_div(-A01 * b0 + A00 * b1, det)
    valid = t0.ge(0) & t1.ge(0) & (t0 + t1).le(1.0)
    e0, e1 = [vert[k] - vert[6 + k] for k in range(3)], [vert[3 + k] - vert[6 + k] for k in range(3)]
    n = [e0[1] * e1[2] - e0[2] * e1[1], e0[2] * e1[0] - e0[0] * e1[2], e0[0] * e1[1] - e0[1] * e1[0]]
    w = [vert[6 + k] - p[k] for k in range(3)]
    dist = safe_div(dot(w, n), dot(v, n))
    return Dist(dist, valid & dist.ge(0))


def _cast_once(dtype, maybe, xpos, xmat, pnt, vec, cand, mesh_strict, vec_err):
    n = pnt.shape[0]
    c = Ctx(dtype, n, maybe)
    P = [c.value(pnt[:, k]) for k in range(3)]
    V = [c.value(vec[:, k], None if vec_err is None else vec_err[:, k]) for k in range(3)]
    best, bid = miss(c), np.full(n, -1, dtype=np.int64)
    for g, gtype, size, tri in cand:
        gp = [c.value(xpos[:, g, k]) for k in range(3)]
        gm = [c.value(xmat[:, g].reshape(n, 9)[:, k]) for k in range(9)]
        lp, lv = ray_to_geom(gm, gp, P, V)
        if int(gtype) == MESH:
            b, cc = ray_basis(c, lv)
            x = miss(c)
            for t in np.asarray(tri).reshape(-1, 9):
                y = ray_triangle(c, [c.value(t[k]) for k in range(9)], lp, lv, b, cc)
                x = x.take(y.closer(x), y)
            take = x.closer(best)
            if mesh_strict:
                take = take & x.x.gt(0)
        else:
            x = ray_geom_val(c, gtype, [c.value(float(size[k])) for k in range(3)], lp, lv)
            take = x.closer(best)
        best = best.take(take, x)
        bid = np.where(take, g, bid)
    return best, bid, c.bad


def combine(a, b):
    """Two evaluations (Dist, ids, undecided) -> dict(decided, hit, v, e, id0, id1): the hull of the two intervals where both hit and overlap."""
    (da, ia, ba), (db, ib, bb) = a, b
    lo_a, hi_a, lo_b, hi_b = da.x.v - da.x.e, da.x.v + da.x.e, db.x.v - db.x.e, db.x.v + db.x.e
    both = da.ok & db.ok
    overlap = both & (lo_a <= hi_b) & (lo_b <= hi_a)
    decided = ~(ba | bb) & (overlap | (~da.ok & ~db.ok))
    lo, hi = np.minimum(lo_a, lo_b), np.maximum(hi_a, hi_b)
    hit = decided & both
    return dict(decided=decided, hit=hit, v=np.where(hit, (lo + hi) / 2, HP(-1)), e=np.where(hit, (hi - lo) / 2 * (1 + HP(EPS_HP)), HP(0)),
                id0=np.where(hit, ia, -1), id1=np.where(hit, ib, -1))


def cast(dtype, xpos, xmat, pnt, vec, cand, mesh_strict=False, vec_err=None):
    """``ray`` for n rays, ray i against the frames ``xpos[i]`` [ngeom, 3] / ``xmat[i]`` [ngeom, 3, 3] (arrays of the dtype).

    ``cand``: the candidates in tie-break order, ``(geom id, type, size (3), triangles [k, 9] or None)``.  ``vec_err``: an absolute input error
    of ``vec``.  Returns dict(decided, hit, v, e, id0, id1): per ray, whether it is decided; if so whether it hits, the distance and its bound
    (``-1`` / ``0`` for a miss) and the one or two geom ids that are right."""
    args = (np.asarray(xpos), np.asarray(xmat), np.asarray(pnt), np.asarray(vec), cand, mesh_strict, vec_err)
    with np.errstate(all="ignore"):
        return combine(_cast_once(dtype, True, *args), _cast_once(dtype, False, *args))


def ray_geom_ref(dtype, gtype, size, pnt, vec):
    """``ray_geom`` of one primitive type for n rows (size / pnt / vec [n, 3] of the dtype): dict(decided, hit, v, e)."""
    size, pnt, vec = np.asarray(size), np.asarray(pnt), np.asarray(vec)
    n = pnt.shape[0]

    def once(maybe):
        c = Ctx(dtype, n, maybe)
        x = ray_geom_val(c, gtype, *[[c.value(t[:, k]) for k in range(3)] for t in (size, pnt, vec)])
        return x, np.zeros(n, dtype=np.int64), c.bad

    with np.errstate(all="ignore"):
        return combine(once(True), once(False))


def pixel_rays_ref(cam_xpos, cam_xmat, fovy, W, H, ssaa):
    """The renderer's primary rays (the reference's ``_generate_rays``) of a ``W x H`` image super-sampled ``ssaa`` times, for cameras
    ``cam_xpos`` [B, 3] / ``cam_xmat`` [B, 3, 3] (their dtype is the Data's): ``(pnt, vec, vec_err)``, each [B, H, W, ssaa, ssaa, 3]
    (sample (sy, sx) of pixel (py, px); pnt is the camera position, exact).  The operations: u = px * ssaa + sx + 0.5, (2 u / RW - 1) * half_w, (1 - 2 v / RH) * half_h, -1; the norm; the division; the
    rotation by cam_xmat.  half_h = tan(fovy * pi / 360) in the dtype and half_w = half_h * (W / H) enter as the call computes them, in torch."""
    import torch

    tdt = getattr(torch, np.asarray(cam_xmat).dtype.name)
    half_h_t = torch.tan(torch.tensor(float(fovy) * (torch.pi / 360.0), dtype=tdt))
    half_h, half_w = float(half_h_t), float(half_h_t * (W / H))
    cam_xpos, cam_xmat = np.asarray(cam_xpos), np.asarray(cam_xmat)
    dtype = cam_xmat.dtype
    B = cam_xmat.shape[0]
    S, RW, RH = int(ssaa), W * int(ssaa), H * int(ssaa)
    py, px, sy, sx = np.meshgrid(np.arange(H), np.arange(W), np.arange(S), np.arange(S), indexing="ij")
    n = px.size
    with np.errstate(all="ignore"):
        c = Ctx(dtype, n, True)
        u, v = c.value((px * S + sx).ravel().astype(np.float64)) + 0.5, c.value((py * S + sy).ravel().astype(np.float64)) + 0.5
        dc = [(2.0 * u / float(RW) - 1.0) * c.value(half_w), (1.0 - 2.0 * v / float(RH)) * c.value(half_h), c.value(-1.0)]
        dn = dot(dc, dc).sqrt()
        dc = [x / dn for x in dc]
        assert not c.bad.any()
        out_v, out_e = np.zeros((B, n, 3), dtype=HP), np.zeros((B, n, 3), dtype=HP)
        for b in range(B):
            m = [c.value(float(x)) for x in cam_xmat[b].reshape(9).astype(np.float64)]
            for i in range(3):
                r = m[3 * i] * dc[0] + m[3 * i + 1] * dc[1] + m[3 * i + 2] * dc[2]
                out_v[b, :, i], out_e[b, :, i] = r.v, r.e
    shape = (B, H, W, S, S, 3)
    pnt = np.broadcast_to(cam_xpos[:, None, :], (B, n, 3)).reshape(shape)
    return pnt, out_v.reshape(shape), out_e.reshape(shape)
