"""The yardstick of the primitive narrow phase (``Env::collision()`` of csrc/mjh_kernels.h, ``make_frame`` / ``normalize_n`` of csrc/mjh_device.h): the five analytic pair
functions -- plane-sphere, plane-capsule, sphere-sphere, sphere-capsule, capsule-capsule -- and ``make_frame`` in numpy, written from the definitions the kernel header cites
(reference collision_primitive.py:29-74, :172-221, math.py:216-230, :485-569) with their quirks: ``x / (n + 1e-6 (n == 0))``, ``+ 1e-6`` in both closest-point denominators,
plane-capsule's fallback ``b`` that is not orthogonalised against ``n``, ``b * any(a)``.

``evaluate`` takes the ``geom_xpos`` / ``geom_xmat`` the run under test produced and ``geom_size``; it does not redo the kinematics.  With ``dt=np.longdouble`` (the default) it
is the reference; with ``dt=np.float32`` / ``np.float64`` it is the same formulas in the dtype.  Per contact it returns dist, pos, frame, the branch it took at every switch
and the margin of each:

  frame_sw   ||a[1]| - 0.5| of make_frame                       frame_y      b = y (else z)
  pc_bn      |bn - 0.5| of plane-capsule                        pc_fallback  bn < 0.5
  pc_n1      ||n[1]| - 0.5| of its fallback (where taken)       pc_fb_y      the fallback took y
  d          the centre distance of sphere_sphere               coincident   d == 0 (normal = x)
  t          distance of sphere-capsule's t from its clamps     t_side       -1: t < 0, +1: t > 1, 0: inside
  ota, otb   ... of capsule-capsule's line parameters           ota_side, otb_side
  in1, in2   ... of the t of its two closest_segment_point      in1_side, in2_side
  d1d2       |d1 - d2| / max(d1, d2)                            pick         d1 < d2
  denom      1 - (dir_a . dir_b)^2
  pick_move  how far pos moves if the d1 < d2 pick goes the other way (absolute)

``Contacts.comparable(eps)`` is the mask built from them: ``dist`` is always compared; ``pos`` and the normal where ``d`` exceeds ``1e3 eps`` times the pair's size and the
``d1 < d2`` pick is not within ``1e3 eps`` relative of a tie; frame rows 1 and 2 where, additionally, every 0.5-switch margin the contact met exceeds ``1e3 eps``.  Two exact
outcomes stay comparable, because they are the same in every precision when the inputs are: ``d == 0`` exactly (the normal is x by definition), and ``d1 == d2`` exactly
where the two sides of the comparison are the same arithmetic on the same numbers (``exact_tie``: the float32 and float64 evaluations tie bit for bit as well).

A near-tie of ``d1`` and ``d2`` is not rare: away from the clamps ``new_a`` is ``best_a`` up to the 1e-6 regulariser, and with one parameter clamped and the axes near
perpendicular ``best_b`` is ``new_b`` up to it, so in float32 most capsule pairs are within ``1e3 eps`` of one, and the two picks are 1e-6 .. 1e-3 apart.  Leaving them all
out would leave capsule-capsule untested in float32.  ``Contacts.against(got_pos, eps)`` therefore keeps such a contact and holds it to WHICHEVER of the two picks the run
under test is nearer to (``alt_*``: the contact of the other pick; neither is asserted, both must be well-conditioned by the rules above): it compares more than
``comparable`` does, never less, and a contact that is neither of the two still fails.
"""
import numpy as np

LD = np.longdouble
FN_PLANE_SPHERE, FN_PLANE_CAPSULE, FN_SPHERE_SPHERE, FN_SPHERE_CAPSULE, FN_CAPSULE_CAPSULE = range(5)
FN_NAMES = ("plane_sphere", "plane_capsule", "sphere_sphere", "sphere_capsule", "capsule_capsule")
FN_IN_KERNEL = 5  # pair_fn < MJH_FN_PLANE_CONVEX
MARGINS = ("frame_sw", "pc_bn", "pc_n1", "d", "t", "ota", "otb", "in1", "in2", "d1d2", "denom", "pick_move", "alt_d", "alt_frame_sw")
SIDES = ("frame_y", "any_a", "pc_fallback", "pc_fb_y", "coincident", "t_side", "ota_side", "otb_side", "in1_side", "in2_side", "pick")


def _dot(a, b):
    return (a * b).sum(-1)


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def normalize_with_norm(x, dt):  # math.py:216-230
    n = np.sqrt(_dot(x, x))
    return x / (n + dt(1e-6) * (n == 0).astype(dt))[..., None], n


def make_frame(a, dt):  # math.py:485-500 -> frame [.., 3, 3], {frame_sw, frame_y, any_a}
    a, _ = normalize_with_norm(a, dt)
    y_pick = (dt(-0.5) < a[..., 1]) & (a[..., 1] < dt(0.5))
    b = np.zeros_like(a)
    b[..., 1] = y_pick
    b[..., 2] = ~y_pick
    b = b - a * _dot(a, b)[..., None]
    any_a = (a != 0).any(-1)
    b = normalize_with_norm(b, dt)[0] * any_a.astype(dt)[..., None]
    return np.stack([a, b, _cross(a, b)], -2), dict(frame_sw=np.abs(np.abs(a[..., 1]) - dt(0.5)), frame_y=y_pick, any_a=any_a)


def _plane_sphere(n, ppos, spos, r, dt):  # collision_primitive.py:29-38
    dist = _dot(spos - ppos, n) - r
    return dist, spos - n * (r + dt(0.5) * dist)[..., None]


def _sphere_sphere(p1, r1, p2, r2, dt):  # :172-186
    n, d = normalize_with_norm(p2 - p1, dt)
    zero = d == 0
    n = np.where(zero[..., None], np.array([1, 0, 0], dtype=dt), n)
    dist = d - (r1 + r2)
    return dist, p1 + n * (r1 + dist * dt(0.5))[..., None], n, dict(d=d, coincident=zero)


def _clamp_info(t, lo, hi):
    side = np.where(t < lo, -1, np.where(t > hi, 1, 0)).astype(np.int8)
    return side, np.minimum(np.abs(t - lo), np.abs(t - hi))


def closest_segment_point(a, b, pt, dt):  # math.py:506-510 -> point, t side, t margin
    ab = b - a
    t = _dot(pt - a, ab) / (_dot(ab, ab) + dt(1e-6))
    side, margin = _clamp_info(t, dt(0), dt(1))
    return a + np.clip(t, dt(0), dt(1))[..., None] * ab, side, margin


def closest_segment_to_segment_points(a0, a1, b0, b1, dt):  # math.py:523-569 -> best_a, best_b, the other pick's (best_a, best_b), info
    dir_a, len_a = normalize_with_norm(a1 - a0, dt)
    dir_b, len_b = normalize_with_norm(b1 - b0, dt)
    hla, hlb = len_a * dt(0.5), len_b * dt(0.5)
    a_mid, b_mid = a0 + dir_a * hla[..., None], b0 + dir_b * hlb[..., None]
    trans = a_mid - b_mid
    dadb, dat, dbt = _dot(dir_a, dir_b), _dot(dir_a, trans), _dot(dir_b, trans)
    denom = dt(1) - dadb * dadb
    ota = (-dat + dadb * dbt) / (denom + dt(1e-6))
    otb = dbt + ota * dadb
    ota_side, ota_m = _clamp_info(ota, -hla, hla)
    otb_side, otb_m = _clamp_info(otb, -hlb, hlb)
    best_a = a_mid + dir_a * np.clip(ota, -hla, hla)[..., None]
    best_b = b_mid + dir_b * np.clip(otb, -hlb, hlb)[..., None]
    new_a, in1_side, in1 = closest_segment_point(a0, a1, best_b, dt)
    new_b, in2_side, in2 = closest_segment_point(b0, b1, best_a, dt)
    d1, d2 = _dot(best_b - new_a, best_b - new_a), _dot(best_a - new_b, best_a - new_b)
    pick = d1 < d2
    big = np.maximum(d1, d2)
    info = dict(ota=ota_m, otb=otb_m, in1=in1, in2=in2, ota_side=ota_side, otb_side=otb_side, in1_side=in1_side, in2_side=in2_side, pick=pick, denom=denom,
                d1d2=np.where(big > 0, np.abs(d1 - d2) / np.where(big > 0, big, dt(1)), dt(0)), exact_tie=d1 == d2)
    p = pick[..., None]
    return np.where(p, new_a, best_a), np.where(p, best_b, new_b), (np.where(p, best_a, new_a), np.where(p, new_b, best_b)), info


class Contacts:
    """Contacts of one evaluation, slot-major: ``dist`` [B, n], ``pos`` [B, n, 3], ``frame`` [B, n, 3, 3]; ``fn`` / ``pair`` / ``q`` / ``size`` [n] say which pair function,
    which pair, which of its contacts and how large the pair is; ``margin[name]`` [B, n] (NaN where the contact does not meet that branch) and ``side[name]`` [B, n]."""

    def __init__(self, B, n, dt):
        self.dt = dt
        self.dist, self.pos, self.frame = np.full((B, n), np.nan, dtype=dt), np.full((B, n, 3), np.nan, dtype=dt), np.full((B, n, 3, 3), np.nan, dtype=dt)
        self.fn, self.pair, self.q, self.size = -np.ones(n, dtype=np.int32), -np.ones(n, dtype=np.int32), -np.ones(n, dtype=np.int32), np.zeros(n)
        self.margin = {k: np.full((B, n), np.nan) for k in MARGINS}
        self.side = {k: np.zeros((B, n), dtype=np.int8) for k in SIDES}
        self.exact_tie = np.zeros((B, n), dtype=bool)
        self.alt_dist, self.alt_pos, self.alt_frame = self.dist.copy(), self.pos.copy(), self.frame.copy()  # capsule-capsule: the contact of the other d1 < d2 pick

    def _masks(self, eps):
        m, thr = self.margin, 1e3 * eps
        gone = lambda k: np.isnan(m[k])
        ok_d = lambda k: gone(k) | (m[k] == 0) | (m[k] > thr * self.size)
        tie_ok = gone("d1d2") | (m["d1d2"] > thr) | self.exact_tie
        sw = np.ones_like(tie_ok)
        for k in ("frame_sw", "pc_bn", "pc_n1"):
            sw &= gone(k) | (m[k] > thr)
        return ok_d("d"), tie_ok, sw, ok_d("alt_d"), gone("alt_frame_sw") | (m["alt_frame_sw"] > thr)

    def comparable(self, eps):
        """{dist, pos, normal, frame: bool [B, n]}: what a correct implementation in a precision of ``eps`` is held to (module docstring)."""
        d_ok, tie_ok, sw, _, _ = self._masks(eps)
        pos = d_ok & tie_ok
        return dict(dist=np.ones_like(pos), pos=pos, normal=pos, frame=pos & sw)

    def against(self, got_pos, eps):
        """({leaf: reference values}, {leaf: rows compared}) for a run whose ``contact_pos`` is ``got_pos``: the comparable rows, and the rows only a near-tie of the
        ``d1 < d2`` pick leaves out, each of those held to the pick (``alt_*`` or not) its ``got_pos`` is nearer to."""
        d_ok, tie_ok, sw, alt_d_ok, alt_sw = self._masks(eps)
        either = ~tie_ok & d_ok & alt_d_ok
        got = np.asarray(got_pos, dtype=np.float64).reshape(self.pos.shape)
        use_alt = either & (np.abs(got - self.alt_pos.astype(np.float64)).max(-1) < np.abs(got - self.pos.astype(np.float64)).max(-1))
        want = dict(dist=np.where(use_alt, self.alt_dist, self.dist), pos=np.where(use_alt[..., None], self.alt_pos, self.pos),
                    frame=np.where(use_alt[..., None, None], self.alt_frame, self.frame))
        want["normal"] = want["frame"][:, :, 0]
        pos = d_ok & (tie_ok | either)
        return want, dict(dist=np.ones_like(pos), pos=pos, normal=pos, frame=pos & sw & (tie_ok | alt_sw))


def evaluate(pairs, dst, nslot, geom_xpos, geom_xmat, geom_size, dt=LD):
    """``pairs``: [(fn, ncon of the pair, geom1, geom2)] in pair order (pairs with ``fn >= FN_IN_KERNEL`` are skipped); ``dst`` [npair, >= 2]: the slot of each pair's
    contacts (``tables.pair_dst``); ``geom_xpos`` [B, ngeom, 3], ``geom_xmat`` [B, ngeom, 9] (row-major), ``geom_size`` [ngeom, 3] -> Contacts over ``nslot`` slots."""
    xpos = np.asarray(geom_xpos).astype(dt).reshape(-1, np.asarray(geom_size).shape[0], 3)
    xmat = np.asarray(geom_xmat).astype(dt).reshape(xpos.shape[0], -1, 3, 3)
    size = np.asarray(geom_size).astype(dt)
    B = xpos.shape[0]
    C = Contacts(B, nslot, dt)
    half = dt(0.5)
    for p, (fn, k, g1, g2) in enumerate(pairs):
        if fn >= FN_IN_KERNEL:
            continue
        p1, p2, m1, m2, s1, s2 = xpos[:, g1], xpos[:, g2], xmat[:, g1], xmat[:, g2], size[g1], size[g2]
        info, alt = {}, None
        if fn == FN_PLANE_SPHERE:
            n = m1[:, :, 2]
            dist, pos = _plane_sphere(n, p1, p2, s2[0], dt)
            frame, info = make_frame(n, dt)
            dist, pos = [dist], [pos]
        elif fn == FN_PLANE_CAPSULE:  # :48-74
            n, axis = m1[:, :, 2], m2[:, :, 2]
            b, bn = normalize_with_norm(axis - n * _dot(n, axis)[..., None], dt)
            fb = bn < half
            fb_y = (-half < n[:, 1]) & (n[:, 1] < half)
            e = np.eye(3, dtype=dt)
            b = np.where(fb[:, None], np.where(fb_y[:, None], e[1], e[2]), b)
            frame = np.stack([n, b, _cross(n, b)], -2)
            info = dict(pc_bn=np.abs(bn - half), pc_fallback=fb, pc_fb_y=fb & fb_y, pc_n1=np.where(fb, np.abs(np.abs(n[:, 1]) - half), np.nan))
            seg = axis * s2[1]
            dist, pos = zip(*[_plane_sphere(n, p1, p2 + off, s2[0], dt) for off in (seg, -seg)])
        else:
            if fn == FN_SPHERE_SPHERE:
                a, r1, b, r2 = p1, s1[0], p2, s2[0]
            elif fn == FN_SPHERE_CAPSULE:  # :195-201
                seg = m2[:, :, 2] * s2[1]
                b, side, margin = closest_segment_point(p2 - seg, p2 + seg, p1, dt)
                a, r1, r2 = p1, s1[0], s2[0]
                info = dict(t=margin, t_side=side)
            else:  # :204-221
                seg1, seg2 = m1[:, :, 2] * s1[1], m2[:, :, 2] * s2[1]
                a, b, (alt_a, alt_b), info = closest_segment_to_segment_points(p1 - seg1, p1 + seg1, p2 - seg2, p2 + seg2, dt)
                r1, r2 = s1[0], s2[0]
                alt = _sphere_sphere(alt_a, r1, alt_b, r2, dt)
            dist, pos, n, ss = _sphere_sphere(a, r1, b, r2, dt)
            frame, fi = make_frame(n, dt)
            info = dict(info, **ss, **fi)
            if alt is not None:
                alt_frame, alt_fi = make_frame(alt[2], dt)
                info.update(pick_move=np.abs(alt[1] - pos).max(-1), alt_d=alt[3]["d"], alt_frame_sw=alt_fi["frame_sw"])
            dist, pos = [dist], [pos]
        psize = float(s1[0] + s2[0] + (s1[1] if fn == FN_CAPSULE_CAPSULE else 0) + (s2[1] if fn in (FN_PLANE_CAPSULE, FN_SPHERE_CAPSULE, FN_CAPSULE_CAPSULE) else 0))
        for q in range(min(k, 2)):
            c = int(dst[p][q])
            C.dist[:, c], C.pos[:, c], C.frame[:, c] = dist[q], pos[q], frame
            C.fn[c], C.pair[c], C.q[c], C.size[c] = fn, p, q, psize
            C.alt_dist[:, c], C.alt_pos[:, c], C.alt_frame[:, c] = (alt[0], alt[1], alt_frame) if alt is not None else (dist[q], pos[q], frame)
            for name, v in info.items():
                if name == "exact_tie":
                    C.exact_tie[:, c] = v
                elif name in C.margin:
                    C.margin[name][:, c] = np.asarray(v, dtype=np.float64)
                else:
                    C.side[name][:, c] = v
    return C


def exact_ties_in_every_precision(pairs, dst, nslot, geom_xpos, geom_xmat, geom_size):
    """Where ``d1 == d2`` bit for bit in longdouble, float64 AND float32: the comparison is the same arithmetic on the same numbers, so ``d1 < d2`` is false in every precision."""
    return np.logical_and.reduce([evaluate(pairs, dst, nslot, geom_xpos, geom_xmat, geom_size, dt).exact_tie for dt in (LD, np.float64, np.float32)])


def reference(pairs, dst, nslot, geom_xpos, geom_xmat, geom_size):
    """The longdouble evaluation, its ``exact_tie`` narrowed to the ties that hold in every precision."""
    C = evaluate(pairs, dst, nslot, geom_xpos, geom_xmat, geom_size, LD)
    if C.exact_tie.any():
        C.exact_tie = exact_ties_in_every_precision(pairs, dst, nslot, geom_xpos, geom_xmat, geom_size)
    return C


def pairs_of(tables):
    """``[(fn, ncon, geom1, geom2)]`` of a placed model's ``tables.pairs``."""
    return [(int(fn), int(k), int(c.geom1), int(c.geom2)) for fn, k, c, _ in tables.pairs]


def topk_smallest(cand_dist, ncon):
    """max_contact_points as a multiset: the ``ncon`` smallest candidate distances per environment, ascending (compared in the dtype they came in)."""
    return np.sort(np.asarray(cand_dist), axis=-1)[..., :ncon]
