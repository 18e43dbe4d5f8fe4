"""geom_distance on the GPU (mjh_geomdist_kernel, csrc/mjh_geomdist.h) against the numpy longdouble reference tests/_geomdist_ref.py, which
tests/test_geom_distance_host.py pins on the goldens' recorded contacts, on alternating projections and on sampled support functions.

The bound is the project's pre-solver tolerance TOL_PRE[dtype] times max(1, the pair's scale), the scale being the largest coordinate of the two geom centres or
their bounding radii.  Measured on the MI355X, worst error over bound per type pair (the random poses, B = 70): see DESIGN.md section 3.2.
"""
import numpy as np
import pytest
import torch

import _geomdist_ref as gr
import mujoco_torch_amd as mt
from _cases import F32, F64, TOL_PRE
from _util import load_model

pytestmark = pytest.mark.gpu

DEV = "cuda"
LD = gr.LD
DTYPES = [pytest.param(F64, id="f64"), pytest.param(F32, id="f32")]
PLANE_G, BALL_S, BALL_L, PILL_S, PILL_L, BRICK_S, BRICK_L, EGG, CAN = range(9)  # tests/golden/geom_distance.xml
_MODELS = {}


def model(dtype):
    if dtype not in _MODELS:
        mx = load_model("geom_distance", dtype=dtype)
        _MODELS[dtype] = (mx, mx.to(DEV), np.asarray(mx.tables.ray["geom_type"]).astype(int), mx.geom_size.numpy().astype(np.float64))
    return _MODELS[dtype]


def data(mx, xpos, xmat, dtype):
    """A Data whose geoms sit at xpos [S..., ng, 3] / xmat [S..., ng, 3, 3] (numpy float64, rounded to the dtype): nothing else is read."""
    batch = tuple(xpos.shape[:-2])
    d = mt.make_data(mx)
    if dtype != F64:
        d = d.to(dtype)
    if batch:
        d = d.expand(*batch).clone()
    return d.replace(geom_xpos=torch.tensor(xpos).to(dtype), geom_xmat=torch.tensor(xmat).to(dtype))


def random_poses(gtype, size, B, seed):
    """Seeded poses: in every environment the geoms gather about one point, each within its own bounding radius of it, so that about half of the pairs overlap."""
    rng = np.random.RandomState(seed)
    ng = len(gtype)
    reach = np.array([10.0 if t == gr.PLANE else gr.reach(int(t), s) for t, s in zip(gtype, size)])  # (the plane: anywhere among the large geoms)
    xpos = rng.randn(B, 1, 3) + 0.3 * reach[None, :, None] * rng.randn(B, ng, 3)
    return xpos, gr.random_rotations(rng, B * ng).reshape(B, ng, 3, 3)


def check(rows, gtype, size, xpos, xmat, dist, fromto, dtype, what="", consts=None):
    """(dist [B, P], fromto [B, P, 6]) of the kernel against the reference on the SAME (rounded) frames: the distance, to - from = dist * n with |n| = 1, both
    points on their surfaces and -- for cores that do not overlap -- the optimality certificate, all at TOL_PRE[dtype] * max(1, scale); the certificate's support
    gap, taken along the n that the two returned points define, is allowed that bound times 1 + 2 (reach1 + reach2) / |dist| (see below).  Returns
    {type pair: worst error over bound}."""
    name = "float64" if dtype == F64 else "float32"
    ref = gr.evaluate(rows, size.astype(LD), xpos, xmat, dtype=consts or name)
    B, P = dist.shape
    assert np.isfinite(dist).all() and np.isfinite(fromto).all(), what
    worst = {}
    for k, (g1, g2, t1, t2) in enumerate(np.asarray(rows).tolist()):
        scale = np.maximum(1.0, np.maximum(np.abs(xpos[:, [g1, g2]]).max((1, 2)), max(gr.reach(t1, size[g1]), gr.reach(t2, size[g2]))))
        bound = TOL_PRE[dtype] * scale
        d, ft = dist[:, k].astype(LD), fromto[:, k].astype(LD)
        errs = [np.abs(d - ref["dist"][:, k])]
        diff = ft[:, 3:] - ft[:, :3]
        errs.append(np.abs(np.sqrt((diff * diff).sum(-1)) - np.abs(d)))
        errs.append(np.abs(gr.sdf(t1, size[g1], xpos[:, g1], xmat[:, g1], ft[:, :3])))
        errs.append(np.abs(gr.sdf(t2, size[g2], xpos[:, g2], xmat[:, g2], ft[:, 3:])))
        if t1 in gr.KIND and t2 in gr.KIND:
            apart = ~ref["overlap"][:, k] & ~ref["nodir"][:, k] & (np.abs(d) > bound)  # (n = (to - from) / dist needs a distance)
            cert = gr.certificate(t1, size[g1], xpos[:, g1], xmat[:, g1], t2, size[g2], xpos[:, g2], xmat[:, g2], d, ft)
            # n is formed from the two returned points, each allowed `bound`: it may turn by 2 * bound / |dist|, which moves the support gap of the two
            # shapes by up to their bounding radii times that angle -- the share of the gap's residual that is the certificate's own, not the kernel's
            turn = 2 * (gr.reach(t1, size[g1]) + gr.reach(t2, size[g2])) / np.where(apart, np.abs(d), 1)
            errs.append(np.where(apart, np.maximum(cert["gap"], 0) / (1 + turn), 0))
        err = np.max(np.stack(errs) / bound, 0)
        key = f"{gr.NAMES[t1]}-{gr.NAMES[t2]}"
        worst[key] = max(worst.get(key, 0.0), float(err.max()))
        assert err.max() <= 1, (what, key, g1, g2, int(err.argmax()), [float(x.max()) for x in errs], float(bound.min()))
    return worst


def run(mdev, d, rows, distmax=1e9):
    dist, fromto = mt.geom_distance(mdev, d.to(DEV), torch.tensor(rows[:, 0]), torch.tensor(rows[:, 1]), distmax)
    torch.cuda.synchronize()
    return dist, fromto


# ---- random poses ----------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=DTYPES)
def random_run(request):
    dtype = request.param
    mx, mdev, gtype, size = model(dtype)
    rows = gr.all_rows(gtype)
    xpos, xmat = random_poses(gtype, size, 70, seed=2024)
    d = data(mx, xpos, xmat, dtype)
    dist, fromto = run(mdev, d, rows)
    return dict(dtype=dtype, rows=rows, d=d, mx=mx, dist=dist, fromto=fromto, xpos=d.geom_xpos.double().numpy(), xmat=d.geom_xmat.double().numpy())


def test_random_poses_against_the_reference(random_run):
    """B = 70 (in the pair-major order a wave holds the tail of one pair and the head of the next, of other types), every supported type pair in both orders."""
    r = random_run
    mx, mdev, gtype, size = model(r["dtype"])
    assert tuple(r["dist"].shape) == (70, len(r["rows"])) and tuple(r["fromto"].shape) == (70, len(r["rows"]), 6)
    assert r["dist"].dtype == r["fromto"].dtype == r["dtype"] and r["dist"].device.type == torch.device(DEV).type
    dist, fromto = r["dist"].cpu().numpy(), r["fromto"].cpu().numpy()
    cores = np.array([t1 in gr.KIND and t2 in gr.KIND for t1, t2 in r["rows"][:, 2:].tolist()])
    share = float((dist[:, cores] < 0).mean())
    worst = check(r["rows"], gtype, size, r["xpos"], r["xmat"], dist, fromto, r["dtype"], what="random poses")
    print(f"{r['dtype']}: {share:.0%} of the sphere / capsule / box pairs overlap; worst error over bound per type pair: "
          + ", ".join(f"{k} {v:.1e}" for k, v in sorted(worst.items())))
    assert 0.25 < share < 0.75


def test_swapped_order_gives_the_same_distance(random_run):
    r = random_run
    rows, dist = r["rows"], r["dist"].cpu().numpy()
    index = {(a, b): k for k, (a, b) in enumerate(rows[:, :2].tolist())}
    for (a, b), k in index.items():
        back = index[(b, a)]
        assert np.abs(dist[:, k] - dist[:, back]).max() <= TOL_PRE[r["dtype"]] * max(1.0, np.abs(r["xpos"]).max()), (a, b)


def test_rows_and_pairs_are_independent_bit_for_bit(random_run):
    """Row e of the batch equals the call on environment e alone (B = 1); a pair listed alone (P = 1) equals the same pair inside the long list, and listed twice;
    B = 3 and the batch shape (2, 3) give the rows of the long run."""
    r = random_run
    mx, mdev, gtype, size = model(r["dtype"])
    rows, d = r["rows"], r["d"]
    for e in (0, 37, 69):
        dist, fromto = run(mdev, d[e], rows)
        assert tuple(dist.shape) == (len(rows),) and torch.equal(dist, r["dist"][e]) and torch.equal(fromto, r["fromto"][e])
    dist, fromto = run(mdev, d[:3], rows)
    assert torch.equal(dist, r["dist"][:3]) and torch.equal(fromto, r["fromto"][:3])
    ng = len(gtype)
    dist, fromto = run(mdev, data(mx, r["xpos"][4:10].reshape(2, 3, ng, 3), r["xmat"][4:10].reshape(2, 3, ng, 3, 3), r["dtype"]), rows)
    assert tuple(dist.shape) == (2, 3, len(rows)) and tuple(fromto.shape) == (2, 3, len(rows), 6)
    assert torch.equal(dist.reshape(6, -1), r["dist"][4:10]) and torch.equal(fromto.reshape(6, -1, 6), r["fromto"][4:10])
    box_box = [k for k, row in enumerate(rows.tolist()) if row[2:] == [gr.BOX, gr.BOX]][0]
    for k in (0, box_box, len(rows) - 1):
        g1, g2 = int(rows[k, 0]), int(rows[k, 1])
        one, ft = mt.geom_distance(mdev, d.to(DEV), g1, g2, 1e9)
        assert tuple(one.shape) == (70,) and torch.equal(one, r["dist"][:, k]) and torch.equal(ft, r["fromto"][:, k])
        two, ft = mt.geom_distance(mdev, d.to(DEV), [g1, g1], [g2, g2], 1e9)
        assert torch.equal(two[:, 0], one) and torch.equal(two[:, 1], one) and torch.equal(ft[:, 0], ft[:, 1])


# ---- poses placed by hand ----------------------------------------------------------------------------------------------------------------------

I3 = np.eye(3)
S2 = np.sqrt(0.5)


def rot(axis, angle):
    c, s = np.cos(angle), np.sin(angle)
    return {"x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), "y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]), "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])}[axis]


TILT = rot("x", 0.3) @ rot("y", -0.4)   # a plane that is not level
SPIN = rot("z", 0.7) @ rot("x", 0.9) @ rot("y", 0.35)
CORNER_DOWN = np.abs(SPIN[2]) @ np.array([0.03, 0.01, 0.05])  # height of brick_s's lowest corner under its centre in the pose SPIN


def _plane_cases():
    """Every body above and below the tilted plane, the plane as geom1 and as geom2; the body's support height along the normal by hand."""
    n = TILT[:, 2]
    out = []
    heights = {BALL_L: (I3, 2.0), PILL_L: (rot("y", 0.5), 0.5 + 3 * abs((rot("y", 0.5).T @ TILT[:, 2])[2])),
               BRICK_L: (SPIN, np.abs(SPIN.T @ TILT[:, 2]) @ np.array([10.0, 4.0, 1.0])),
               EGG: (SPIN, np.linalg.norm(np.array([0.3, 0.2, 0.1]) * (SPIN.T @ TILT[:, 2]))),
               CAN: (SPIN, 0.4 * np.hypot(*(SPIN.T @ TILT[:, 2])[:2]) + 0.15 * abs((SPIN.T @ TILT[:, 2])[2]))}
    for g, (mat, h) in heights.items():
        for gap in (0.25, -0.125):
            pos = np.array([0.3, -0.2, 0.1]) + (h + gap) * n
            out.append((f"plane-{g} gap {gap}", PLANE_G, g, (np.array([0.3, -0.2, 0.1]), TILT), (pos, mat), gap, n))
            out.append((f"{g}-plane gap {gap}", g, PLANE_G, (pos, mat), (np.array([0.3, -0.2, 0.1]), TILT), gap, -n))
    # the cylinder lying flat on the level plane (its disc: no radial direction) and standing on its rim at 45 degrees
    out.append(("can flat", PLANE_G, CAN, (np.zeros(3), I3), (np.array([0.0, 0, 0.15 + 0.5]), I3), 0.5, np.array([0.0, 0, 1])))
    out.append(("can on its rim", PLANE_G, CAN, (np.zeros(3), I3), (np.array([0.0, 0, (0.4 + 0.15) * S2 + 0.5]), rot("x", np.pi / 4)), 0.5, np.array([0.0, 0, 1])))
    return out


# (name, geom1, geom2, (pos1, mat1), (pos2, mat2), dist by hand, n by hand or None where the direction is not unique or undefined)
Z90 = rot("y", np.pi / 2)  # local z -> world x
HAND = [
    ("sphere centre inside a box", BRICK_L, BALL_S, (np.zeros(3), I3), (np.array([9.5, 0.2, 0.1]), I3), -0.5 - 0.01, np.array([1.0, 0, 0])),
    ("sphere at a box's centre", BRICK_L, BALL_L, (np.zeros(3), I3), (np.zeros(3), SPIN), -1.0 - 2.0, None),
    ("capsule axis through a box", PILL_L, BRICK_S, (np.array([0.0, 0.004, 0]), Z90), (np.zeros(3), I3), -0.006 - 0.5, np.array([0.0, -1, 0])),
    ("boxes face to face", BRICK_L, BRICK_S, (np.zeros(3), I3), (np.array([1.0, -2.0, 1 + 0.05 + 0.2]), I3), 0.2, None),
    ("boxes edge across edge", BRICK_S, BRICK_L, (np.zeros(3), rot("y", np.pi / 4)), (np.array([0.0, 3 * S2, 5 * S2 + 0.08 * S2 + 0.3]), rot("x", np.pi / 4)), 0.3,
     np.array([0.0, 0, 1])),
    ("box vertex to face", BRICK_L, BRICK_S, (np.zeros(3), I3), (np.array([3.0, 1.0, 1 + CORNER_DOWN + 0.125]), SPIN), 0.125, np.array([0.0, 0, 1])),
    ("boxes in shallow overlap", BRICK_L, BRICK_S, (np.zeros(3), I3), (np.array([3.0, 1.0, 1 + CORNER_DOWN - 0.005]), SPIN), -0.005, np.array([0.0, 0, 1])),
    ("boxes in deep overlap", BRICK_L, BRICK_S, (np.zeros(3), I3), (np.array([3.0, 1.0, 0.8]), SPIN), -(0.2 + CORNER_DOWN), np.array([0.0, 0, 1])),
    ("a box inside the other", BRICK_L, BRICK_S, (np.zeros(3), I3), (np.array([9.8, 0.5, 0.2]), I3), -(0.2 + 0.03), np.array([1.0, 0, 0])),
    ("capsules parallel", PILL_S, PILL_L, (np.array([1.0, 0, 0.5]), I3), (np.zeros(3), I3), 1 - 0.5 - 0.02, None),
    ("capsules with skew axes", PILL_L, PILL_S, (np.zeros(3), I3), (np.array([0.0, 0.8, 1.0]), Z90), 0.8 - 0.52, np.array([0.0, 1, 0])),
    # no direction from the cores: the axes meet, lie on one line, or the sphere's centre sits on the axis -- n must still be perpendicular to the segments
    ("capsules with crossing axes", PILL_L, PILL_S, (np.zeros(3), I3), (np.array([0.0, 0, 1.0]), Z90), -0.52, None),
    ("capsules with crossing axes, tilted", PILL_S, PILL_L, (SPIN @ np.array([0.0, 0, 1.5]), SPIN @ rot("x", 1.1)), (np.zeros(3), SPIN), -0.52, None),
    ("capsules on one axis", PILL_S, PILL_L, (SPIN @ np.array([0.0, 0, 0.5]), SPIN), (np.zeros(3), SPIN), -0.52, None),
    ("sphere on a capsule's axis", BALL_S, PILL_L, (np.array([0.0, 0, 1.0]), SPIN), (np.zeros(3), I3), -0.51, None),
    ("capsule's axis through a sphere's centre", PILL_L, BALL_L, (np.zeros(3), SPIN), (SPIN @ np.array([0.0, 0, -2.0]), I3), -2.5, None),
    ("concentric spheres", BALL_S, BALL_L, (np.array([0.5, 0.5, 0.5]), SPIN), (np.array([0.5, 0.5, 0.5]), I3), -2.01, np.array([0.0, 0, 1])),
    ("spheres touching", BALL_S, BALL_L, (np.array([0.0, 2.01, 0]), I3), (np.zeros(3), I3), 0.0, None),
    ("box resting on a box", BRICK_S, BRICK_L, (np.array([0.0, 0, 1.05]), I3), (np.zeros(3), I3), 0.0, None),
    ("sphere touching a capsule", BALL_L, PILL_L, (np.array([2.5, 0, 1.0]), I3), (np.zeros(3), I3), 0.0, None),
] + _plane_cases()


@pytest.mark.parametrize("dtype", DTYPES)
def test_poses_placed_by_hand(dtype):
    """One environment per pose: the distance by hand, the reference's checks, and n where it is unique."""
    mx, mdev, gtype, size = model(dtype)
    ng, B = len(gtype), len(HAND)
    xpos = np.tile(100.0 * np.arange(1, ng + 1)[None, :, None], (B, 1, 3))  # (the geoms a pose does not use: far away)
    xmat = np.tile(I3, (B, ng, 1, 1))
    for e, (_, g1, g2, (p1, m1), (p2, m2), _, _) in enumerate(HAND):
        xpos[e, g1], xmat[e, g1], xpos[e, g2], xmat[e, g2] = p1, m1, p2, m2
    pairs = sorted({(h[1], h[2]) for h in HAND})
    rows = np.array([(a, b, gtype[a], gtype[b]) for a, b in pairs], dtype=np.int32)
    d = data(mx, xpos, xmat, dtype)
    dist, fromto = run(mdev, d, rows)
    dist, fromto = dist.cpu().numpy(), fromto.cpu().numpy()
    xp, xm = d.geom_xpos.double().numpy(), d.geom_xmat.double().numpy()
    tol = TOL_PRE[dtype]
    for e, (name, g1, g2, _, _, want, n) in enumerate(HAND):
        k = pairs.index((g1, g2))
        check(rows[k:k + 1], gtype, size, xp[e:e + 1], xm[e:e + 1], dist[e:e + 1, k:k + 1], fromto[e:e + 1, k:k + 1], dtype, what=name)
        scale = max(1.0, np.abs(xp[e, [g1, g2]]).max(), gr.reach(gtype[g1], size[g1]), gr.reach(gtype[g2], size[g2]))
        assert abs(dist[e, k] - want) <= tol * scale, (name, dist[e, k], want)
        diff = (fromto[e, k, 3:] - fromto[e, k, :3]).astype(np.float64)
        assert abs(np.linalg.norm(diff) - abs(dist[e, k])) <= tol * scale, name
        if n is not None and abs(want) > 0:
            assert np.abs(diff / dist[e, k] - n).max() <= tol * scale / abs(want), (name, diff / dist[e, k], n)
    # the poses whose cores leave no direction reach that branch (the reference says so on the rounded frames), and n is perpendicular to every capsule's axis
    nodir = [h[0] for h in HAND if h[0].startswith(("capsules with crossing axes", "capsules on one axis", "sphere on a capsule", "capsule's axis through", "concentric"))]
    assert len(nodir) == 6
    for name in nodir:
        e = [h[0] for h in HAND].index(name)
        g1, g2 = HAND[e][1], HAND[e][2]
        k = pairs.index((g1, g2))
        ref = gr.evaluate(rows[k:k + 1], size.astype(LD), xp[e:e + 1], xm[e:e + 1], dtype="float64" if dtype == F64 else "float32")
        assert ref["nodir"][0, 0] and not ref["overlap"][0, 0], name
        n = (fromto[e, k, 3:] - fromto[e, k, :3]).astype(np.float64) / dist[e, k]
        assert abs(np.linalg.norm(n) - 1) <= 10 * tol, name
        for g in (g1, g2):
            if gtype[g] == gr.CAPSULE:
                assert abs(n @ xm[e, g][:, 2]) <= 10 * tol, (name, n, xm[e, g][:, 2])
    e = [h[0] for h in HAND].index("concentric spheres")
    k = pairs.index((BALL_S, BALL_L))
    assert np.abs(fromto[e, k] - np.array([0.5, 0.5, 0.51, 0.5, 0.5, -1.5])).max() <= tol * 2  # n is the world +z


NEARLY_PARALLEL = (9e-4, 3e-4, 1e-4, 2e-5, 3e-6, 1e-7)  # angles between the two edges, radians


@pytest.mark.parametrize("dtype", DTYPES)
def test_boxes_whose_nearest_edges_are_nearly_parallel(dtype):
    """Two large boxes (half-axes 10 4 1 and 5 2 0.5), an edge of one across an edge of the other at the angles of NEARLY_PARALLEL, 1e-3 and 1e-2 apart and 1e-3
    deep: the pose at which a cross product of nearly parallel edge directions is the separating axis and the nearest points lie inside both edges.  The
    yardstick is the reference with NO axis skipped (CONSTS["exact"]), so it shares no threshold with the kernel; the bound is the one of every other pose.
    (With 1 - (u . e)^2 for the sine and a threshold of 1e-6 on it, float32 missed this bound at 9e-4 rad: 2.3e-3 against 2.2e-3, the sign of a 1e-3 gap lost.)"""
    mx, mdev, gtype, size = model(dtype)
    size = size.copy()
    size[BRICK_S] = [5.0, 2.0, 0.5]
    grown = mdev.replace(geom_size=torch.tensor(size, dtype=dtype, device=DEV))
    rng = np.random.RandomState(31)
    per = 48
    N = per * len(NEARLY_PARALLEL)
    angle = np.repeat(NEARLY_PARALLEL, per)
    delta = np.tile(np.repeat([1e-3, 1e-2, -1e-3], per // 3), len(NEARLY_PARALLEL))
    R = gr.axis_angle(rng.randn(N, 3), angle * rng.uniform(0.5, 1.0, N)) @ gr.axis_angle(np.tile([1.0, 0, 0], (N, 1)), rng.uniform(0.3, 1.2, N))
    n = np.cross(np.tile([1.0, 0, 0], (N, 1)), R[:, :, 0])
    n = n / np.linalg.norm(n, axis=1, keepdims=True) * np.sign(n[:, 1] + n[:, 2])[:, None]
    on_a = np.stack([rng.uniform(-6, 6, N), np.full(N, 4.0), np.full(N, 1.0)], -1)      # a point of the large box's edge y = 4, z = 1
    on_b = np.stack([rng.uniform(-3, 3, N), np.full(N, -2.0), np.full(N, -0.5)], -1)    # ... and of the other's edge, in its frame
    ng = len(gtype)
    xpos = np.tile(100.0 * np.arange(1, ng + 1)[None, :, None], (N, 1, 3))
    xmat = np.tile(I3, (N, ng, 1, 1))
    xpos[:, BRICK_L], xpos[:, BRICK_S], xmat[:, BRICK_S] = 0.0, on_a + delta[:, None] * n - np.einsum("bij,bj->bi", R, on_b), R
    rows = np.array([(BRICK_L, BRICK_S, gr.BOX, gr.BOX), (BRICK_S, BRICK_L, gr.BOX, gr.BOX)], dtype=np.int32)
    d = data(mx, xpos, xmat, dtype)
    dist, fromto = run(grown, d, rows)
    dist, fromto = dist.cpu().numpy(), fromto.cpu().numpy()
    xp, xm = d.geom_xpos.double().numpy(), d.geom_xmat.double().numpy()
    ref = gr.evaluate(rows[:1], size.astype(LD), xp, xm, dtype="exact")["dist"][:, 0].astype(np.float64)
    on_edges = np.abs(ref - delta) <= 1e-5  # (the poses where that edge pair is indeed the nearest feature, on the rounded frames)
    assert on_edges.mean() > 0.2
    for a in NEARLY_PARALLEL:
        sel = angle == a
        worst = check(rows, gtype, size, xp[sel], xm[sel], dist[sel], fromto[sel], dtype, what=f"edges {a:g} rad apart", consts="exact")
        err = np.abs(dist[sel, 0] - ref[sel])
        print(f"{dtype} edges {a:g} rad apart: {int(on_edges[sel].sum())} of {per} poses on the edge pair, worst |dist - exact| {err.max():.1e}, worst error over bound {max(worst.values()):.1e}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_distmax_cut(dtype):
    """A pair just inside distmax keeps its distance and points, one just beyond gives distmax and zeros; overlapping pairs are never cut."""
    mx, mdev, gtype, size = model(dtype)
    xpos, xmat = random_poses(gtype, size, 3, seed=5)
    xpos[:, BALL_S], xpos[:, BALL_L] = np.array([0.0, 0, 0]), np.array([0.0, 0, 5.0])  # 2.99 apart
    d = data(mx, xpos, xmat, dtype)
    step = 1e-6 if dtype == F64 else 1e-3
    inside, ft = mt.geom_distance(mdev, d.to(DEV), BALL_S, BALL_L, 2.99 + step)
    assert torch.allclose(inside.cpu().double(), torch.full((3,), 2.99, dtype=F64), rtol=0, atol=TOL_PRE[dtype] * 5)
    assert torch.allclose(ft.cpu().double(), torch.tensor([0, 0, 0.01, 0, 0, 3.0], dtype=F64).expand(3, 6), rtol=0, atol=TOL_PRE[dtype] * 5)
    beyond, ft = mt.geom_distance(mdev, d.to(DEV), BALL_S, BALL_L, 2.99 - step)
    assert (beyond.cpu().double() == float(torch.tensor(2.99 - step, dtype=dtype))).all() and not ft.any()
    rows = gr.all_rows(gtype)
    far, _ = run(mdev, d, rows)
    cut, ft = run(mdev, d, rows, distmax=0.0)
    assert torch.equal(cut, far.clamp(max=0)) and not ft[far > 0].any() and ft[far < 0].any()


def test_a_value_only_geom_size_edit_reaches_the_kernel():
    mx, mdev, gtype, size = model(F64)
    xpos, xmat = random_poses(gtype, size, 3, seed=6)
    xpos[:, BALL_L] += 20
    d = data(mx, xpos, xmat, F64).to(DEV)
    before, _ = mt.geom_distance(mdev, d, BALL_S, BALL_L, 1e9)
    grown = mdev.replace(geom_size=mdev.geom_size + 0.25)
    assert grown.tables is mdev.tables
    after, _ = mt.geom_distance(grown, d, BALL_S, BALL_L, 1e9)
    assert torch.allclose(after, before - 0.5, rtol=0, atol=1e-12)
    again, _ = mt.geom_distance(mdev, d, BALL_S, BALL_L, 1e9)
    assert torch.equal(again, before)
