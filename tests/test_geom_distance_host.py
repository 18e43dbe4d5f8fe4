"""geom_distance without a GPU: the tests' numpy longdouble reference (tests/_geomdist_ref.py, the yardstick of tests/test_geom_distance.py) pinned on the
recorded contacts of the goldens and -- the box parts -- on alternating projections and sampled support functions, and the public function with the launch
replaced by that reference.

Measured here (printed by the tests): against the recorded contact_dist, worst |difference| 2.2e-11 (capsule-capsule, the ant; 8.9e-12 capsules_topk), sphere-capsule
3.2e-12, the plane pairs 2.5e-16 or better; alternating projections (4000 sweeps in longdouble, 360 seeded poses of which 219 apart): worst 2.2e-19; the
separating-axis depth against the sampled bound (141 overlapping poses): never above it, slack between 2.5e-5 and 1.7e-2 (the sampling's coarseness)."""
import ctypes
import re

import numpy as np
import pytest
import torch

import _geomdist_ref as gr
import _hostsim
import mujoco_torch_amd as mt
from _cases import F32, F64, TOL_PRE
from _util import Golden, load_model
from mujoco_torch_amd import native

LD = gr.LD

# ---- 1. the reference on the recordings -----------------------------------------------------------------------------------------------------

PRIMITIVE_CASES = ["humanoid_cg_f64", "capsules_topk_f64", "ant_euler_newton_pyr_f64", "hopper_f64", "halfcheetah_f64", "convex_primitives_f64"]
QUADRIC_CASES = ["quadric/euler_newton_pyr_f64", "quadric/euler_cg_ell_f64", "quadric/topk_f64"]
PINNED = {(gr.PLANE, gr.SPHERE), (gr.PLANE, gr.CAPSULE), (gr.SPHERE, gr.CAPSULE), (gr.CAPSULE, gr.CAPSULE)}
PINNED_QUADRIC = {(gr.PLANE, gr.ELLIPSOID), (gr.PLANE, gr.CYLINDER)}


@pytest.mark.parametrize("case", PRIMITIVE_CASES + QUADRIC_CASES)
def test_the_reference_reproduces_the_recorded_contact_distances(case):
    """On the recorded geom_xpos / geom_xmat of every environment and step, the reference's distance of a pair equals the smallest recorded contact_dist of that
    pair at TOL_PRE[float64].  The recorded plane-box contacts are no pin: plane_convex keeps four contacts whose minimum is not the support distance."""
    g = Golden(case)
    gtype = np.asarray(g.model.tables.ray["geom_type"])
    size = g.model.geom_size.detach().cpu().numpy()
    want = PINNED_QUADRIC if case in QUADRIC_CASES else PINNED
    pairs = sorted({(int(p[2].geom1), int(p[2].geom2)) for p in g.model.tables.pairs if (int(gtype[p[2].geom1]), int(gtype[p[2].geom2])) in want})
    assert pairs, "the recording has none of the pinned pairs"
    rows = np.array([(a, b, gtype[a], gtype[b]) for a, b in pairs], dtype=np.int32)
    worst, n, seen = {}, 0, set()
    for s in range(g.nsteps):
        xpos = np.stack([g.expected(e, s, "geom_xpos").reshape(-1, 3) for e in range(g.nenv)])
        xmat = np.stack([g.expected(e, s, "geom_xmat").reshape(-1, 3, 3) for e in range(g.nenv)])
        got = gr.evaluate(rows, size, xpos, xmat)["dist"]
        for e in range(g.nenv):
            cd, g1, g2 = g.expected(e, s, "contact_dist"), g.expected(e, s, "contact_geom1"), g.expected(e, s, "contact_geom2")
            for k, (a, b) in enumerate(pairs):
                mine = cd[(g1 == a) & (g2 == b)]
                if not len(mine):  # (max_contact_points kept none of this pair's candidates)
                    continue
                key = (gr.NAMES[int(rows[k, 2])], gr.NAMES[int(rows[k, 3])])
                err = abs(float(got[e, k] - LD(mine.min())))
                worst[key] = max(worst.get(key, 0.0), err)
                n += 1
                seen.add(key)
    print(f"{case}: {n} pair distances; worst |reference - recorded| per type pair: " + ", ".join(f"{a}-{b} {w:.1e}" for (a, b), w in sorted(worst.items())))
    assert n >= g.nenv * g.nsteps and max(worst.values()) <= TOL_PRE[F64], worst


# ---- 2. the box parts on something independent --------------------------------------------------------------------------------------------------

KINDS = [(0, 2), (1, 2), (2, 2), (1, 1)]  # point-box, segment-box, box-box, segment-segment
N_POSES, SWEEPS, DIRECTIONS = 90, 4000, 200_000


def _poses(ka, kb, seed):
    """N_POSES seeded poses of cores A, B in B's frame: centres within the cores' sizes of each other, so that about half of the pairs with a box overlap."""
    rng = np.random.RandomState(seed)
    half = lambda k: np.stack([rng.uniform(0.05, 1.5, N_POSES) * m for m in {0: (0, 0, 0), 1: (0, 0, 1), 2: (1, 1, 1)}[k]], -1)
    a, b = half(ka), half(kb)
    c = rng.randn(N_POSES, 3) * 0.3 * (np.linalg.norm(a, axis=1) + np.linalg.norm(b, axis=1))[:, None]
    return c, gr.random_rotations(rng, N_POSES), a, b


def _core(k, c, U, a, b, i):
    """Pose i through the reference's core routine (one environment)."""
    return gr.core_pair(*k, LD(1) * c[i:i + 1], LD(1) * U[i:i + 1], LD(1) * a[i], LD(1) * b[i], LD(0), LD(0), np.array([[0, 0, 1]], dtype=LD), gr.CONSTS["float64"])


@pytest.fixture(scope="module")
def core_results():
    out = {}
    for s, k in enumerate(KINDS):
        c, U, a, b = _poses(*k, seed=100 + s)
        rs = [_core(k, c, U, a, b, i) for i in range(N_POSES)]
        out[k] = (c, U, a, b, {n: np.concatenate([r[n] for r in rs]) for n in ("dist", "on_a", "on_b", "overlap")})
    return out


def test_cores_apart_agree_with_alternating_projections(core_results):
    """Non-overlapping cores: SWEEPS sweeps of projecting onto A, then onto B, from the reference's own witness moved off by a fifth of the sizes (the limit is the
    distance whatever the start); the distance found may not differ from the enumeration's by more than TOL_PRE[float64]."""
    worst, n = 0.0, 0
    for k, (c, U, a, b, r) in core_results.items():
        apart = ~r["overlap"]
        cc, UU, aa, bb = c[apart].astype(LD), U[apart].astype(LD), a[apart].astype(LD), b[apart].astype(LD)
        onto_a = lambda x: cc + np.einsum("bij,bj->bi", UU, np.clip(np.einsum("bij,bi->bj", UU, x - cc), -aa, aa))
        x = r["on_b"][apart] + LD(0.2) * (aa + bb)
        for _ in range(SWEEPS):
            pa = onto_a(x)
            x = np.clip(pa, -bb, bb)
        d = np.sqrt(((onto_a(x) - x) ** 2).sum(-1))
        err = np.abs(d - r["dist"][apart])
        worst, n = max(worst, float(err.max())), n + int(apart.sum())
        assert (r["dist"][apart] > 0).all() and err.max() <= TOL_PRE[F64], (k, float(err.max()))
    print(f"alternating projections: {n} poses apart of {len(KINDS) * N_POSES}, worst |difference| {worst:.1e}")
    assert n >= 150


def test_overlap_depth_never_exceeds_the_sampled_bound(core_results):
    """Overlapping cores: the depth along ANY direction d, h_A(d) + h_B(-d), bounds the minimum translation distance from above; over DIRECTIONS sampled
    directions the separating-axis depth must stay at or below the smallest.  One-sided: the sampling is coarse."""
    rng = np.random.RandomState(7)
    d = rng.randn(DIRECTIONS, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    slack, n = [], 0
    for k, (c, U, a, b, r) in core_results.items():
        for i in np.nonzero(r["overlap"])[0]:
            h_a = d @ c[i] + np.abs(d @ U[i]) @ a[i]  # max over A of d . x
            h_b = np.abs(d) @ b[i]                    # max over B of -d . x
            bound = float((h_a + h_b).min())
            depth = -float(r["dist"][i])
            assert depth > 0 and depth <= bound + 1e-12, (k, i, depth, bound)
            slack.append(bound - depth)
            n += 1
    print(f"sampled bound: {n} overlapping poses, largest bound - depth {max(slack):.1e}, smallest {min(slack):.1e}")
    assert n >= 100
    assert not core_results[(1, 1)][4]["overlap"].any()  # segments have no interior


# ---- 3. the host API on a stand-in -------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def models():
    return {F64: load_model("geom_distance"), F32: load_model("geom_distance", dtype=F32)}


def place(mx, batch, seed, dtype=F64, spread=1.0):
    """A Data of batch shape ``batch`` whose geoms sit at seeded random poses (no physics runs: the function reads geom_xpos / geom_xmat alone)."""
    rng = np.random.RandomState(seed)
    ng, B = int(mx.ngeom), int(np.prod(batch)) if batch else 1
    d = mt.make_data(mx)
    if dtype != F64:
        d = d.to(dtype)
    if batch:
        d = d.expand(*batch).clone()
    xpos = torch.tensor(spread * rng.randn(B, ng, 3)).to(dtype).reshape(batch + (ng, 3))
    xmat = torch.tensor(gr.random_rotations(rng, B * ng)).to(dtype).reshape(batch + (ng, 3, 3))
    return d.replace(geom_xpos=xpos, geom_xmat=xmat)


class StandIn:
    """``mjh_geom_distance`` of the CPU stand-in library: the numpy reference on the host pointers it is handed."""

    def __init__(self):
        self.calls = []

    def install(self, monkeypatch):
        _hostsim.install(monkeypatch)
        monkeypatch.setattr(_hostsim._Lib, "mjh_geom_distance", self, raising=False)
        return self

    def __get__(self, lib, owner=None):  # (bound like a method: the library instance knows the model)
        return lambda *args: self.run(lib, *args)

    def run(self, lib, handle, xpos, xmat, size, pairs, npair, distmax, dist, fromto, B, stream):
        ng = int(lib.o.desc.ngeom)
        ct, dt, name = (ctypes.c_double, np.float64, "float64") if lib.o.dt == 0 else (ctypes.c_float, np.float32, "float32")
        view = lambda p, n, c=ct: np.ctypeslib.as_array((c * n).from_address(p.value))
        rows = view(pairs, 4 * npair, ctypes.c_int32).reshape(npair, 4).copy()
        self.calls.append(dict(rows=rows, B=B, distmax=distmax.value, dtype=name))
        r = gr.evaluate(rows, view(size, 3 * ng).reshape(ng, 3).astype(LD), view(xpos, 3 * ng * B).reshape(B, ng, 3), view(xmat, 9 * ng * B).reshape(B, ng, 3, 3),
                        distmax=distmax.value, dtype=name)
        view(dist, B * npair)[:] = r["dist"].astype(dt).reshape(-1)
        view(fromto, 6 * B * npair)[:] = r["fromto"].astype(dt).reshape(-1)
        return 0


@pytest.fixture
def stand_in(monkeypatch):
    return StandIn().install(monkeypatch)


def test_the_function_and_the_entry_point_are_public():
    assert callable(mt.geom_distance) and native.ABI_VERSION >= 21
    text = open(native.HEADER).read()
    assert re.search(r"\bint mjh_geom_distance\s*\(const mjhModel\* m, const void\* geom_xpos, const void\* geom_xmat, const void\* geom_size, const int32_t\* pairs,"
                     r"\s*int64_t npair, double distmax,\s*void\* dist, void\* fromto, int64_t B, void\* hip_stream\);", text)
    assert re.search(r"#define MJH_KERNEL_GEOM_DISTANCE 47\b", text)
    assert len(native.ARGS) == 6 and "mjh_geom_distance" not in native.ARGS


def test_the_scene_has_what_it_is_meant_to_have(models):
    mx = models[F64]
    gtype = np.asarray(mx.tables.ray["geom_type"]).tolist()
    assert sorted(gtype) == sorted([gr.PLANE] + 2 * [gr.SPHERE, gr.CAPSULE, gr.BOX] + [gr.ELLIPSOID, gr.CYLINDER])
    size = mx.geom_size.numpy()
    assert size[size > 0].min() == 0.01 and size.max() == 10 and len(mx.tables.pairs) == 0
    assert len(gr.all_rows(gtype)) == 6 * 5 + 2 * 8  # every ordered pair of the six cores, the plane with its eight bodies in both orders


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("batch", [(), (3,), (2, 3)], ids=["unbatched", "b3", "b2x3"])
def test_shapes_dtypes_and_values(stand_in, models, batch, dtype):
    mx = models[dtype]
    d = place(mx, batch, seed=5, dtype=dtype)
    rows = gr.all_rows(mx.tables.ray["geom_type"])
    P, B = len(rows), int(np.prod(batch)) if batch else 1
    dist, fromto = mt.geom_distance(mx, d, rows[:, 0].tolist(), torch.tensor(rows[:, 1]), 100.0)
    assert tuple(dist.shape) == batch + (P,) and tuple(fromto.shape) == batch + (P, 6) and dist.dtype == fromto.dtype == dtype
    assert len(stand_in.calls) == 1 and np.array_equal(stand_in.calls[0]["rows"], rows) and stand_in.calls[0]["B"] == B
    want = gr.evaluate(rows, mx.geom_size.numpy().astype(LD), d.geom_xpos.reshape(B, -1, 3).numpy(), d.geom_xmat.reshape(B, -1, 3, 3).numpy(), distmax=100.0,
                       dtype=stand_in.calls[0]["dtype"])
    assert np.array_equal(dist.reshape(B, P).numpy(), want["dist"].astype(dist.numpy().dtype))
    assert np.array_equal(fromto.reshape(B, P, 6).numpy(), want["fromto"].astype(dist.numpy().dtype))
    # two single ids: no pair dimension; an int and a 0-d tensor
    one, ft = mt.geom_distance(mx, d, int(rows[7, 0]), torch.tensor(int(rows[7, 1])), 100.0)
    assert tuple(one.shape) == batch and tuple(ft.shape) == batch + (6,)
    assert torch.equal(one, dist[..., 7]) and torch.equal(ft, fromto[..., 7, :])
    # the nearest points: to - from = dist * n, |n| = 1
    diff = (fromto[..., 3:] - fromto[..., :3]).double()
    assert torch.allclose(diff.norm(dim=-1), dist.double().abs(), rtol=0, atol=TOL_PRE[dtype] * 10)


def test_one_id_broadcasts_against_many(stand_in, models):
    mx = models[F64]
    d = place(mx, (3,), seed=6)
    dist, fromto = mt.geom_distance(mx, d, 0, [1, 2, 3, 5], 50.0)
    assert tuple(dist.shape) == (3, 4) and stand_in.calls[-1]["rows"][:, :2].tolist() == [[0, 1], [0, 2], [0, 3], [0, 5]]
    back, _ = mt.geom_distance(mx, d, np.array([1, 2, 3, 5]), torch.tensor(0), 50.0)
    assert stand_in.calls[-1]["rows"][:, :2].tolist() == [[1, 0], [2, 0], [3, 0], [5, 0]] and torch.allclose(back, dist, rtol=0, atol=1e-12)
    single, _ = mt.geom_distance(mx, d, [4], [6], 50.0)  # (a list of one id keeps the pair dimension)
    assert tuple(single.shape) == (3, 1)
    zero_d, _ = mt.geom_distance(mx, d, np.asarray(4), np.int64(6), 50.0)  # (a 0-d integer array is one id, like a 0-d tensor)
    assert tuple(zero_d.shape) == (3,) and torch.equal(zero_d, single[:, 0])


def test_refusals_come_before_any_call(stand_in, models):
    mx = models[F64]
    d = place(mx, (3,), seed=8)
    ng = int(mx.ngeom)
    egg, can = 7, 8
    bad = [
        (ValueError, "every environment", lambda: mt.geom_distance(mx, d, torch.zeros((3, 2), dtype=torch.int64), [1, 2], 1.0)),
        (ValueError, "every environment", lambda: mt.geom_distance(mx, d, [[1, 2], [1, 2], [1, 2]], 3, 1.0)),
        (ValueError, f"geom id {ng}", lambda: mt.geom_distance(mx, d, 1, ng, 1.0)),
        (ValueError, "geom id -1", lambda: mt.geom_distance(mx, d, [-1, 2], 1, 1.0)),
        (ValueError, "with itself", lambda: mt.geom_distance(mx, d, [1, 2], [3, 2], 1.0)),
        (ValueError, "do not broadcast", lambda: mt.geom_distance(mx, d, [1, 2], [3, 4, 5], 1.0)),
        (ValueError, "integer", lambda: mt.geom_distance(mx, d, torch.tensor([1.0]), 2, 1.0)),
        (ValueError, "integer|ids", lambda: mt.geom_distance(mx, d, [1.5], 2, 1.0)),
        (ValueError, "distmax", lambda: mt.geom_distance(mx, d, 1, 2, -0.5)),
        (ValueError, "distmax", lambda: mt.geom_distance(mx, d, 1, 2, float("nan"))),
        (ValueError, "distmax", lambda: mt.geom_distance(mx, d, 1, 2, None)),
        (NotImplementedError, r"geoms 7, 1\) is ellipsoid-sphere", lambda: mt.geom_distance(mx, d, egg, 1, 1.0)),
        (NotImplementedError, "box-cylinder", lambda: mt.geom_distance(mx, d, [1, 5], [2, can], 1.0)),
        (NotImplementedError, "ellipsoid-cylinder", lambda: mt.geom_distance(mx, d, egg, can, 1.0)),
        (ValueError, "geom_xpos has shape", lambda: mt.geom_distance(mx, d.replace(geom_xpos=d.geom_xpos[:, :-1]), 1, 2, 1.0)),
        (ValueError, "geom_xmat", lambda: mt.geom_distance(mx, d.replace(geom_xmat=d.geom_xmat[:1]), 1, 2, 1.0)),
        (ValueError, "geom_xmat", lambda: mt.geom_distance(mx, d.replace(geom_xmat=d.geom_xmat.float()), 1, 2, 1.0)),
        (ValueError, "dtype|float32", lambda: mt.geom_distance(mx, d.to(F32), 1, 2, 1.0)),
        (ValueError, "geom_size", lambda: mt.geom_distance(mx.replace(geom_size=mx.geom_size[:-1]), d, 1, 2, 1.0)),
        (NotImplementedError, "geom_distance cannot be used under torch.vmap", lambda: torch.vmap(lambda x: mt.geom_distance(mx, d.replace(geom_xpos=x), 1, 2, 1.0)[0])(d.geom_xpos)),
    ]
    for exc, match, run in bad:
        with pytest.raises(exc, match=match):
            run()
    assert not stand_in.calls


def test_plane_plane_and_mesh_pairs_are_refused_by_name(stand_in):
    """(A model with an hfield cannot be built: device_put refuses it.)"""
    two = mt.device_put(mt.mjcf.from_xml_string("""<mujoco><worldbody><geom type="plane" size="1 1 .1" contype="0" conaffinity="0"/>
        <geom type="plane" pos="0 0 -1" size="1 1 .1" contype="0" conaffinity="0"/></worldbody></mujoco>"""))
    with pytest.raises(NotImplementedError, match="plane-plane"):
        mt.geom_distance(two, mt.make_data(two), 0, 1, 1.0)
    mesh = load_model("mesh_contact")
    gtype = np.asarray(mesh.tables.ray["geom_type"]).tolist()
    m = gtype.index(int(mt.GeomType.MESH))
    with pytest.raises(NotImplementedError, match="mesh"):
        mt.geom_distance(mesh, mt.make_data(mesh), m, (m + 1) % len(gtype), 1.0)
    assert not stand_in.calls


def test_without_the_stand_in_cpu_data_is_refused(models):
    with pytest.raises(RuntimeError, match="HIP device"):
        mt.geom_distance(models[F64], place(models[F64], (2,), seed=1), 1, 2, 1.0)


def test_the_distmax_cut(stand_in, models):
    """A pair just inside distmax keeps its distance and points; one just beyond gives distmax and zeros (MuJoCo's convention)."""
    mx = models[F64]
    d = place(mx, (), seed=9)
    eye = torch.eye(3, dtype=F64)
    xpos, xmat = d.geom_xpos.clone(), d.geom_xmat.clone()
    xpos[1], xpos[2], xmat[1], xmat[2] = torch.tensor([0.0, 0, 0]), torch.tensor([0.0, 0, 5.0]), eye, eye  # the spheres (r = 0.01, 2): 2.99 apart
    d = d.replace(geom_xpos=xpos, geom_xmat=xmat)
    inside, ft = mt.geom_distance(mx, d, 1, 2, 2.99 + 1e-9)
    assert abs(float(inside) - 2.99) < 1e-12 and torch.allclose(ft, torch.tensor([0, 0, 0.01, 0, 0, 3.0], dtype=F64), rtol=0, atol=1e-12)
    beyond, ft = mt.geom_distance(mx, d, 1, 2, 2.99 - 1e-9)
    assert float(beyond) == 2.99 - 1e-9 and not ft.any()
    zero, ft = mt.geom_distance(mx, d, 1, 2, 0)  # (distmax = 0: only overlapping pairs report)
    assert float(zero) == 0 and not ft.any()
    assert [c["distmax"] for c in stand_in.calls] == [2.99 + 1e-9, 2.99 - 1e-9, 0.0]


def test_a_value_only_geom_size_edit_is_honoured(stand_in, models):
    mx = models[F64]
    d = place(mx, (2,), seed=10, spread=4.0)
    before, _ = mt.geom_distance(mx, d, 1, 2, 100.0)
    grown = mx.replace(geom_size=mx.geom_size + 0.25)
    assert grown.tables is mx.tables
    after, _ = mt.geom_distance(grown, d, 1, 2, 100.0)
    assert torch.allclose(after, before - 0.5, rtol=0, atol=1e-12)  # two radii, 0.25 each
    again, _ = mt.geom_distance(mx, d, 1, 2, 100.0)
    assert torch.equal(again, before)


def test_empty_batches_and_pair_lists_return_without_a_call(stand_in, models):
    mx = models[F64]
    dist, ft = mt.geom_distance(mx, place(mx, (0,), seed=1), [1, 3], [2, 4], 1.0)
    assert tuple(dist.shape) == (0, 2) and tuple(ft.shape) == (0, 2, 6)
    dist, ft = mt.geom_distance(mx, place(mx, (2, 0), seed=1), 1, 2, 1.0)
    assert tuple(dist.shape) == (2, 0) and tuple(ft.shape) == (2, 0, 6)
    dist, ft = mt.geom_distance(mx, place(mx, (3,), seed=1), [], torch.zeros(0, dtype=torch.int64), 1.0)
    assert tuple(dist.shape) == (3, 0) and tuple(ft.shape) == (3, 0, 6) and dist.dtype == F64
    assert not stand_in.calls
