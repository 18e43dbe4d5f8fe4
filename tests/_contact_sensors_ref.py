"""A plain numpy reference of contact_force and the touch / framelinacc / frameangacc sensors (csrc/mjh_contact_sensors.h), for the tests only.

It restates the definitions of that header with plain loops in ``HP`` (tests/_postcon_ref.py) and reuses ``_postcon_ref.contact_wrench`` for the decode.  Per
element it returns ``(value, S, n)``: ``S`` the sum of the absolute values of the terms the element is made of, ``n`` the number of additions; the comparison
bound is ``_postcon_ref.bound(n, eps, S) = (n + 16) (eps + EPS_HP) S``.  A pure copy has ``n = 0`` and is compared bit for bit by the tests.

The ray / shape test of a touch zone is restated here in HP from the geometry (is there a t >= 0 with pnt + t vec on the shape's surface), not from the kernel's
formulas: ``zone_hit``.  A decision is *fragile* when it flips under a scaling of the zone by 1 +- 1e-3 (``touch_decisions``).
"""
import numpy as np

import _postcon_ref as pr
from _postcon_ref import HP

TOUCH, FRAMELINACC, FRAMEANGACC = 0, 33, 34
SPHERE, CAPSULE, ELLIPSOID, CYLINDER, BOX = 2, 3, 4, 5, 6
POS_LEAVES = ("xipos", "xpos", "geom_xpos", "site_xpos", "cam_xpos")
LEAVES = pr.LEAVES + ("xpos", "geom_xpos", "site_xpos", "site_xmat", "cam_xpos", "cacc", "sensordata")
FRAGILE_SCALE = 1e-3


def leaves_of(d, cacc=None):
    out = pr.leaves_of(d, [n for n in LEAVES if n != "cacc"])
    out["cacc"] = (d.cacc if cacc is None else cacc).detach().cpu().numpy()
    return out


def sensor_rows(mx):
    """(type, adr, objid, leaf kind, body, root, datatype, site type, cutoff) per touch / framelinacc / frameangacc sensor, from the compiled model's own sensor
    arrays (``tables.source``: the model ``device_put`` was given)."""
    src = mx.tables.source
    A = lambda n: np.asarray(getattr(src, n))
    if int(mx.opt.disableflags) & (1 << 13) or int(getattr(mx, "nsensor", 0) or 0) == 0:  # DisableBit.SENSOR
        return []
    body_of = {1: None, 2: None, 5: "geom_bodyid", 6: "site_bodyid", 7: "cam_bodyid"}
    kind_of = {1: 0, 2: 1, 5: 2, 6: 3, 7: 4}
    rows = []
    for i, t in enumerate(A("sensor_type")):
        t, obj = int(t), int(A("sensor_objid")[i])
        if t == TOUCH:
            kind, body, st = 3, int(A("site_bodyid")[obj]), int(A("site_type")[obj])
        elif t in (FRAMELINACC, FRAMEANGACC):
            ot = int(A("sensor_objtype")[i])
            kind, body, st = kind_of[ot], (obj if body_of[ot] is None else int(A(body_of[ot])[obj])), -1
        else:
            continue
        rows.append((t, int(A("sensor_adr")[i]), obj, kind, body, int(A("body_rootid")[body]), int(A("sensor_datatype")[i]), st, float(A("sensor_cutoff")[i])))
    return rows


# ---- contact_force ---------------------------------------------------------------------------------------------------------------------------------------

def _env(leaves, e, dtype=HP):
    return {k: (np.asarray(v[e]) if k in pr._INT else np.asarray(v[e], dtype=dtype)) for k, v in leaves.items() if v is not None}


def _valid(T, L, c, ngeom, nefc):
    g1, g2 = int(L["contact_geom"][c, 0]), int(L["contact_geom"][c, 1])
    dim, adr = int(L["contact_dim"][c]), int(L["contact_efc_address"][c])
    rows = 2 * (dim - 1) if T["pyramidal"] and dim > 1 else dim
    return 0 <= g1 < ngeom and 0 <= g2 < ngeom and 1 <= dim <= 6 and adr >= 0 and adr + rows <= nefc


def contact_frame_wrench(T, L, c, s):
    """w[6] of slot c in the contact frame (s = -1: the values; s = +1, on the leaves' magnitudes: the sums of |terms|), zeros for a skipped slot.  Recovered
    from ``_postcon_ref.contact_wrench`` (which returns frame^T w) with an identity frame."""
    ngeom, nefc = len(T["geom_bodyid"]), L["efc_force"].shape[0]
    if not _valid(T, L, c, ngeom, nefc):
        return None
    eye = dict(L, contact_frame=np.broadcast_to(np.eye(3, dtype=L["contact_pos"].dtype).reshape(9), L["contact_frame"].reshape(-1, 9).shape))
    b1, b2, tq, fc = pr.contact_wrench(T, eye, c, s)
    return b1, b2, np.concatenate([fc, tq])


def contact_force(T, leaves, to_world=False):
    """(value, S, n), each [B, ncon, 6].  Contact frame: n = the pyramid's additions (at most 10 rows); elliptic / dim 1 rows are copies (n = 0, S = |value|).
    World frame: three products more."""
    B, ncon = np.asarray(leaves["contact_geom"]).shape[:2]
    val, mag, n = np.zeros((B, ncon, 6), dtype=HP), np.zeros((B, ncon, 6), dtype=HP), np.zeros((B, ncon, 6))
    for e in range(B):
        L = _env(leaves, e)
        La = {k: (v if k in pr._INT else np.abs(v)) for k, v in L.items()}
        for c in range(ncon):
            w = contact_frame_wrench(T, L, c, -1)
            if w is None:
                continue
            wa = contact_frame_wrench(T, La, c, +1)[2]
            dim = int(L["contact_dim"][c])
            pyr = T["pyramidal"] and dim > 1
            if to_world:
                F, Fa = L["contact_frame"][c].reshape(3, 3), La["contact_frame"][c].reshape(3, 3)
                val[e, c] = np.concatenate([F.T @ w[2][:3], F.T @ w[2][3:]])
                mag[e, c] = np.concatenate([Fa.T @ wa[:3], Fa.T @ wa[3:]])
                n[e, c] = 3 + (2 * (dim - 1) if pyr else 0)
            else:
                val[e, c], mag[e, c] = w[2], wa
                n[e, c, 0] = 2 * (dim - 1) if pyr else 0
                n[e, c, 1:] = 2 if pyr else 0
    return val, mag, n


def copies(T, leaves):
    """bool [B, ncon]: the slot's contact-frame row is a pure copy of efc_force rows (or zeros): elliptic cone, dim 1, or a skipped slot."""
    dim = np.asarray(leaves["contact_dim"])
    return np.ones_like(dim, dtype=bool) if not T["pyramidal"] else (dim <= 1) | (np.asarray(leaves["contact_geom"]) < 0).any(-1)


# ---- touch -------------------------------------------------------------------------------------------------------------------------------------------------

def _roots(a, b, c):
    """real roots of a t^2 + 2 b t + c"""
    det = b * b - a * c
    if a <= 0 or det < 0:
        return []
    r = np.sqrt(det)
    return [(-b - r) / a, (-b + r) / a]


def zone_hit(stype, size, p, v):
    """Does the ray p + t v, t >= 0, in the site's frame meet the surface of the shape?  From the geometry, in the dtype of p."""
    size = np.asarray(size, dtype=p.dtype)
    ts = []
    if stype == SPHERE:
        ts = _roots(v @ v, v @ p, p @ p - size[0] ** 2)
    elif stype == ELLIPSOID:
        s = 1 / size ** 2
        ts = _roots((s * v) @ v, (s * v) @ p, (s * p) @ p - 1)
    elif stype in (CAPSULE, CYLINDER):
        r, h = size[0], size[1]
        ts = [t for t in _roots(v[0] ** 2 + v[1] ** 2, v[0] * p[0] + v[1] * p[1], p[0] ** 2 + p[1] ** 2 - r * r) if abs(p[2] + t * v[2]) <= h]
        for sgn in (1, -1):
            if stype == CAPSULE:
                q = p - np.array([0, 0, sgn * h], dtype=p.dtype)
                ts += [t for t in _roots(v @ v, v @ q, q @ q - r * r) if sgn * (p[2] + t * v[2]) >= h]
            elif v[2] != 0:
                t = (sgn * h - p[2]) / v[2]
                if (p[0] + t * v[0]) ** 2 + (p[1] + t * v[1]) ** 2 <= r * r:
                    ts.append(t)
    elif stype == BOX:
        for ax in range(3):
            if v[ax] == 0:
                continue
            o = [i for i in range(3) if i != ax]
            for sgn in (1, -1):
                t = (sgn * size[ax] - p[ax]) / v[ax]
                if all(abs(p[i] + t * v[i]) <= size[i] for i in o):
                    ts.append(t)
    else:
        raise ValueError(f"site type {stype}")
    return any(t >= 0 for t in ts)


def touch_decisions(T, L, row, site_size):
    """Per contact slot that could count for the touch sensor `row` (valid, on the sensor's body, w[0] > 0): (slot, w0, |w0| sum, hit, fragile, direction_matters)."""
    _, _, site, _, body, _, _, stype, _ = row
    R, sp = L["site_xmat"][site].reshape(3, 3), L["site_xpos"][site]
    size = np.asarray(site_size[site], dtype=HP)
    La = None
    out = []
    for c in range(L["contact_geom"].shape[0]):
        w = contact_frame_wrench(T, L, c, -1)
        if w is None or body not in (w[0], w[1]) or not w[2][0] > 0:
            continue
        if La is None:
            La = {k: (v if k in pr._INT else np.abs(v)) for k, v in L.items()}
        normal = L["contact_frame"][c].reshape(9)[:3]
        v = normal if w[0] == body else -normal
        p, dv = R.T @ (L["contact_pos"][c] - sp), R.T @ v
        hit = zone_hit(stype, size, p, dv)
        fragile = any(zone_hit(stype, size * HP(k), p, dv) != hit for k in (1 - FRAGILE_SCALE, 1 + FRAGILE_SCALE))
        out.append((c, w[2][0], contact_frame_wrench(T, La, c, +1)[2][0], hit, fragile, zone_hit(stype, size, p, -dv) != hit))
    return out


def clip(v, datatype, cutoff):
    if cutoff > 0:
        return np.clip(v, -cutoff, cutoff) if datatype == 0 else (np.minimum(v, cutoff) if datatype == 1 else v)
    return v


# ---- the frame sensors -------------------------------------------------------------------------------------------------------------------------------------

def frame_acc(L, La, row):
    """(value[3], S[3], n) of a framelinacc / frameangacc sensor before the cutoff."""
    t, _, obj, kind, body, root, _, _, _ = row
    if t == FRAMEANGACC:
        a = L["cacc"][body, :3]
        return a, np.abs(a), 0

    def ev(L, s):
        dif = L[POS_LEAVES[kind]][obj] + s * L["subtree_com"][root]
        om, al = L["cvel"][body, :3], L["cacc"][body, :3]
        vlin = L["cvel"][body, 3:] + s * pr._cross(dif, om, s)
        return (L["cacc"][body, 3:] + s * pr._cross(dif, al, s)) + pr._cross(om, vlin, s)

    return ev(L, -1), ev(La, +1), 8  # three terms, each a difference of two products of (differences of) leaves


def evaluate(mx, leaves, site_size):
    """The sensors of one batched pass: a list per sensor row of dict(row, value [B, dim], S, n, and for touch: decisions per environment)."""
    T, rows = pr.tables(mx), sensor_rows(mx)
    B = np.asarray(leaves["cvel"]).shape[0]
    has_con = leaves.get("efc_force") is not None and np.asarray(leaves["efc_force"]).shape[1] > 0 and np.asarray(leaves["contact_geom"]).shape[1] > 0
    out = []
    for row in rows:
        dim = 1 if row[0] == TOUCH else 3
        r = dict(row=row, value=np.zeros((B, dim), dtype=HP), S=np.zeros((B, dim), dtype=HP), n=np.zeros((B, dim)), decisions=[], raw=np.zeros((B, dim), dtype=HP))
        for e in range(B):
            L = _env(leaves, e)
            if row[0] == TOUCH:
                dec = touch_decisions(T, L, row, site_size) if has_con else []
                r["decisions"].append(dec)
                hits = [d for d in dec if d[3]]
                r["raw"][e, 0] = sum((d[1] for d in hits), HP(0))
                r["S"][e, 0] = sum((d[2] for d in hits), HP(0))
                r["n"][e, 0] = len(hits) + 10  # the sum over the slots, the pyramid's sum inside a term
            else:
                La = {k: (v if k in pr._INT else np.abs(v)) for k, v in L.items()}
                r["raw"][e], r["S"][e], n = frame_acc(L, La, row)
                r["n"][e] = n
            r["value"][e] = clip(r["raw"][e], row[6], row[8])
        out.append(r)
    return out
