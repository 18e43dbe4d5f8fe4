"""Shared by tests/test_convex_large_host.py (CPU) and tests/test_convex_large.py (GPU): the convex_large model's pair list, and two properties of the
plane-convex and sphere-convex contacts evaluated in numpy ``longdouble`` from ``geom_xpos`` / ``geom_xmat`` and the hull tables alone -- no reference and
no oracle involved.

Bounds.  Every checked quantity is a sum of products s = sum_i n_i (sum_j R_ij v_j + p_i - q_i) (a plane or face normal against a rotated, translated
hull vertex).  A sum of n rounded products, added in any order, is within (n + 2) eps S of its exact value, S = the sum of the absolute values of its
terms (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2; tests/_support_ref.py uses the same bound).  The outer sum has n = 3 terms:
the bound is (3 + 2) eps S with S = sum_i |n_i| (sum_j |R_ij v_j| + |p_i| + |q_i|) (+ the radius for the sphere), eps the epsilon of the leaves' dtype
plus longdouble's own.  The kernel, the oracle and the reference all evaluate the sum in the hull's frame instead (R^T applied to the plane / the centre),
which regroups the same elementary products; the inner roundings are NOT covered by a worst-case analysis of that grouping ((11 + 2) eps S would be),
so (3 + 2) is the tighter, stated bound and the tests print the worst error as a fraction of it.
"""
import numpy as np

HP = np.longdouble
EPS_HP = float(np.finfo(HP).eps)

# geom ids of convex_large.xml (body order) and the eleven pairs its contype / conaffinity bits leave
PLANE, BLOB, BLOB_SMALL, PRISM18, PRISM44, BOX, SPHERE, CAPSULE = range(8)
PAIRS = [(PLANE, BLOB), (PLANE, PRISM44), (BLOB, BLOB_SMALL), (BLOB, PRISM18), (PRISM18, PRISM44), (BOX, BLOB), (BOX, PRISM18), (SPHERE, BLOB),
         (SPHERE, PRISM18), (CAPSULE, BLOB), (CAPSULE, PRISM18)]
# (vertices, faces, edges, vertices per face) of the hull tables
TABLE_SIZES = {BLOB: (100, 196, 294, 3), BLOB_SMALL: (100, 196, 294, 3), PRISM18: (36, 20, 54, 18), PRISM44: (88, 46, 44, 15), BOX: (8, 6, 12, 4)}


def pair_slots(out, pair):
    """Contact slots of a geom pair (the slot layout is static: the same for every environment)."""
    g1, g2 = np.asarray(out["contact_geom1"]).reshape(-1, np.asarray(out["contact_dist"]).shape[-1])[0], np.asarray(out["contact_geom2"]).reshape(-1, np.asarray(out["contact_dist"]).shape[-1])[0]
    return np.nonzero((g1 == pair[0]) & (g2 == pair[1]))[0]


def _world_vertices(xpos, xmat, g, verts):
    """(R v + p, sum_j |R_ij v_j| + |p_i|) per hull vertex, longdouble."""
    R, p, v = np.asarray(xmat, dtype=HP).reshape(-1, 3, 3)[g], np.asarray(xpos, dtype=HP).reshape(-1, 3)[g], np.asarray(verts, dtype=HP)
    return v @ R.T + p, np.abs(v) @ np.abs(R).T + np.abs(p)


def _clear_argmax(score, cand, margin):
    """Index of the largest score among the candidates, or None when the runner-up is within `margin` of it (rounding could decide)."""
    idx = np.nonzero(cand)[0]
    if len(idx) == 0:
        return None
    order = idx[np.argsort(-score[idx], kind="stable")]
    if len(order) > 1 and not (score[order[0]] - score[order[1]] > margin):
        return None
    return int(order[0])


def farthest_pair(w, below, named, eps):
    """_manifold_points (collision_convex.py:183-235) picks a point a of the masked set and then b = the masked point farthest from a, an arg-max over ALL hull
    vertices.  Whatever slot holds which: two of the vertices the contacts name must be such a pair.  For every named vertex x, the vertex below the plane farthest
    from x in longdouble (skipped when the runner-up is within 1e4 eps of it: rounding could decide) -> the list of (x, farthest) that are decided."""
    res = []
    for x in sorted(set(named)):
        sq = ((w[x] - w) ** 2).sum(1)
        y = _clear_argmax(sq, below, 1e4 * eps * sq.max())
        if y is not None:
            res.append((x, y))
    return res


def plane_convex_property(out, model, pair, eps):
    """ONE environment.  For every contact of a plane-convex pair: `pos` is a hull vertex (R v + p, each coordinate within the bound above), and a
    contact that counts (dist != 1: the reference gives a repeated vertex dist = 1) carries dist = n . (R v + p - p_plane) of that vertex.  (The reference's
    contact position IS the vertex, collision_convex.py:613-616; pos + dist n / 2, the midpoint convention, is not -- measured 3e-5 .. 0.3 off on its recordings.)
    No contact is deeper than the deepest hull vertex.  Where the set of vertices below the plane is decided (none within rounding of it) and not empty: every
    contact that counts names a vertex below the plane; with exactly one below, the smallest dist IS the minimum over all vertices; with several, the manifold keeps
    the four points that span the largest area, which need not include the deepest (the reference's own recordings have such environments), and the contacts are
    held to `farthest_pair` instead -- one named vertex is the farthest of ALL vertices below from another named one.
    Returns (worst error over its bound, vertices below the plane, 1 if farthest_pair was checked, the largest index of a vertex below the plane there or -1)."""
    verts = model.tables.convex[pair[1]]["vert"]
    xpos, xmat = out["geom_xpos"], out["geom_xmat"]
    w, w_abs = _world_vertices(xpos, xmat, pair[1], verts)
    n = np.asarray(xmat, dtype=HP).reshape(-1, 3, 3)[pair[0]][:, 2]
    q = np.asarray(xpos, dtype=HP).reshape(-1, 3)[pair[0]]
    val = (w - q) @ n
    s_abs = (w_abs + np.abs(q)) @ np.abs(n)
    e = eps + EPS_HP
    slots = pair_slots(out, pair)
    assert len(slots) == 4
    dist, pos = np.asarray(out["contact_dist"], dtype=HP).reshape(-1)[slots], np.asarray(out["contact_pos"], dtype=HP).reshape(-1, 3)[slots]
    worst, named = 0.0, []
    for k in range(4):
        ratio = (np.abs(w - pos[k]) / (5 * e * np.maximum(w_abs, 1e-30))).max(1)  # per vertex: the worst coordinate over its bound
        v = int(np.argmin(ratio))
        assert ratio[v] <= 1, f"pair {pair} contact {k}: pos is no hull vertex ({float(ratio[v]):.2f} x the bound at the closest one)"
        worst = max(worst, float(ratio[v]))
        named.append(v)
        if dist[k] != 1:
            r = float(abs(dist[k] - val[v]) / (5 * e * s_abs[v]))
            assert r <= 1, f"pair {pair} contact {k}: dist {float(dist[k])} is not n . (R v + p - p_plane) = {float(val[v])} of its vertex ({r:.2f} x the bound)"
            worst = max(worst, r)
    below = val < -5 * e * s_abs
    lo = int(np.argmin(val))
    assert dist.min() >= val[lo] - 5 * e * s_abs[lo], f"pair {pair}: a contact deeper than every hull vertex"
    checked, top = 0, -1
    if below.sum() + (val > 5 * e * s_abs).sum() == len(val):  # no vertex within rounding of the plane: the set of vertices below is decided
        if below.sum() == 1:
            r = float(abs(dist.min() - val[lo]) / (5 * e * s_abs[lo]))
            assert r <= 1, f"pair {pair}: smallest dist {float(dist.min())} is not the hull's minimum {float(val[lo])} ({r:.2f} x the bound)"
            worst = max(worst, r)
        if below.sum() >= 1:
            assert all(below[v] for k, v in enumerate(named) if dist[k] != 1), f"pair {pair}: a contact that counts names a vertex above the plane ({named})"
        if below.sum() >= 2:
            far = farthest_pair(w, below, [v for k, v in enumerate(named) if dist[k] != 1], eps)
            if far:
                assert any(y in named and y != x for x, y in far), f"pair {pair}: no named vertex {named} is the farthest below the plane from another one ({far})"
                checked, top = 1, int(np.nonzero(below)[0].max())
    return worst, int(below.sum()), checked, top


def sphere_convex_property(out, model, pair, eps):
    """ONE environment.  Where the sphere's centre is outside the hull, closer than its radius to exactly the plane of the face f it is farthest in front of,
    and its projection falls strictly inside that face's polygon (all decided in longdouble, with a margin of 1e-6 of the hull's size), the face interior is the
    nearest feature and dist = n_f . (c - v_f) - r.  Returns (worst error over its bound, or None where the condition does not hold)."""
    t = model.tables.convex[pair[1]]
    verts, face, fn = np.asarray(t["vert"], dtype=HP), np.asarray(t["face"]), np.asarray(t["facenormal"], dtype=HP)
    xpos, xmat = np.asarray(out["geom_xpos"], dtype=HP).reshape(-1, 3), np.asarray(out["geom_xmat"], dtype=HP).reshape(-1, 3, 3)
    R, p, c = xmat[pair[1]], xpos[pair[1]], xpos[pair[0]]
    r = HP(np.asarray(model.geom_size)[pair[0]][0])
    w, w_abs = _world_vertices(out["geom_xpos"], out["geom_xmat"], pair[1], verts)
    nw = fn @ R.T  # face normals in the world frame
    s = ((c - w[face[:, 0]]) * nw).sum(1)
    f = int(np.argmax(s))
    size = float(np.abs(verts).max())
    if not (1e-6 * size < s[f] < r - 1e-6 * size):
        return None
    ids = [int(i) for k, i in enumerate(face[f]) if k == 0 or i != face[f][k - 1]]  # (padding repeats the last id)
    proj = c - s[f] * nw[f]
    for k in range(len(ids)):
        a, b = w[ids[k - 1]], w[ids[k]]
        if not (np.dot(proj - a, np.cross(b - a, nw[f])) < -1e-6 * size * float(np.linalg.norm(b - a))):
            return None
    s_abs = float((np.abs(nw[f]) * (np.abs(c) + w_abs[face[f, 0]])).sum() + abs(r))
    slots = pair_slots(out, pair)
    assert len(slots) == 1
    dist = HP(np.asarray(out["contact_dist"]).reshape(-1)[slots[0]])
    ratio = float(abs(dist - (s[f] - r)) / (5 * (eps + EPS_HP) * s_abs))
    assert ratio <= 1, f"pair {pair}: dist {float(dist)} is not n_f . (c - v_f) - r = {float(s[f] - r)} ({ratio:.2f} x the bound)"
    return ratio


def check_properties(out_env, model, eps):
    """Both properties on ONE environment's leaves ({leaf: array}) -> dict: `plane` / `sphere` worst error over the bound (sphere: None where no pair meets its
    condition), `below` vertices below the planes, and per plane pair whether farthest_pair was checked (`checked`) and the largest index of a vertex below the plane there (`top`)."""
    res = dict(plane=0.0, sphere=None, below=0, checked={}, top={})
    for pair in ((PLANE, BLOB), (PLANE, PRISM44)):
        r, b, k, top = plane_convex_property(out_env, model, pair, eps)
        res["plane"], res["below"] = max(res["plane"], r), res["below"] + b
        res["checked"][pair], res["top"][pair] = k, top
    for pair in ((SPHERE, BLOB), (SPHERE, PRISM18)):
        r = sphere_convex_property(out_env, model, pair, eps)
        if r is not None:
            res["sphere"] = max(res["sphere"] or 0.0, r)
    return res


class PropertyTally:
    """Accumulates check_properties over environment-steps; `assert_covered` holds the coverage both the CPU and the GPU test must reach."""

    def __init__(self):
        self.plane = self.sphere = 0.0
        self.below = self.sphere_hits = 0
        self.checked = {(PLANE, BLOB): 0, (PLANE, PRISM44): 0}
        self.top = {(PLANE, BLOB): -1, (PLANE, PRISM44): -1}

    def add(self, res):
        self.plane, self.sphere = max(self.plane, res["plane"]), max(self.sphere, res["sphere"] or 0.0)
        self.below, self.sphere_hits = self.below + res["below"], self.sphere_hits + (res["sphere"] is not None)
        for pair in self.checked:
            self.checked[pair] += res["checked"][pair]
            self.top[pair] = max(self.top[pair], res["top"][pair])

    def assert_covered(self):
        """Both plane pairs had farthest_pair checked (several vertices below, the selection over all vertices decided in longdouble) on at least two
        environment-steps; on blob100 with a vertex past the first 64 (the second trip of the kernel's vertex loops) below the plane and named by a contact; a
        sphere sat over a face interior.  NOT covered by this property: on the recorded poses only one cap of prism44 ever dips below the plane (vertex
        indices up to 40 of 88), so its second-trip vertices are candidates that are masked out, never selected; prism44's second trip is held by the comparison
        with the recording alone."""
        assert self.sphere_hits > 0 and self.below > 0
        for pair in self.checked:
            assert self.checked[pair] >= 2, (pair, self.checked)
        assert self.top[(PLANE, BLOB)] >= 64, self.top

    def __str__(self):
        return (f"plane-convex worst {self.plane:.2f} of its bound, sphere-convex worst {self.sphere:.2f} ({self.sphere_hits} face-interior cases), {self.below} vertices below a plane, "
                f"farthest-pair env-steps checked {list(self.checked.values())}, largest vertex index below the plane there {list(self.top.values())}")
