"""Seeded inputs of tests/test_ray_edges.py and tests/test_render_edges.py, made without a GPU so that tests/test_ray_ref_host.py can hold
the reference's left-out shares on the very same rays and pixels.

Frames: the recorded ``geom_xpos`` / ``geom_xmat`` of a golden (tests/golden/ray/, tests/golden/render/), tiled to ``B`` environments, every
geom of environment ``e`` shifted by its own small seeded offset: no two environments are alike.

Rays: every case mixes the families of ``FAMILIES`` ray by ray (ray i of the flattened (environment, ray) grid belongs to family
``i % len(FAMILIES)`` once the leading slots -- one ray aimed at a geom of every candidate type, one that misses -- are filled).
Offsets from a decision boundary (a mesh edge, a capsule seam, a cylinder rim) are drawn log-uniformly from ``OFFSET_EPS`` x the dtype's eps
up to 1e-2: the reference leaves a ray out when its answer depends on a rounding, and a ray aimed at a boundary to within the arithmetic's
own error does (tests/test_ray_ref_host.py holds the left-out share of every family to 1 %).
"""
import functools
import importlib
import json
import os

import numpy as np
import torch

import _ray_ref as rr
from _util import GOLD, load_model

RAY_GOLD, RENDER_GOLD = os.path.join(GOLD, "ray"), os.path.join(GOLD, "render")
FAMILIES = ("mix", "mesh_edge", "seam_rim", "graze", "inside")
OFFSET_EPS = 1e5  # smallest offset from a decision boundary, in units of the dtype's eps (of an O(1) length)
SHIFT = 0.02      # per-environment offset of every geom

# name: (ray golden whose frames are used, flg_static, bodyexclude)
RAY_MODELS = {
    "humanoid_f64": ("humanoid_f64", True, -1),                       # 20 candidates
    "humanoid_nostatic_f64": ("humanoid_nostatic_f64", False, [1]),   # 17: an odd tail chunk
    "ray_scene_f64": ("ray_scene_f64", True, -1),                     # every type, two meshes, 9
    "ray_scene_f32": ("ray_scene_f32", False, -1),                    # 7: a tail of 3 at chunk 4
    "mesh_contact_f32": ("mesh_contact_f32", True, -1),
}
# (B, R): what each reaches is said in tests/test_ray_edges.py
RAY_SHAPES = ((300, 1), (5, 3), (7, 85), (4, 255), (3, 256), (3, 257), (40, 16))


def _npz(path):
    z = np.load(path)
    return z, json.loads(str(z["meta"]))


@functools.lru_cache(maxsize=None)
def ray_golden(case):
    z, meta = _npz(os.path.join(RAY_GOLD, case + ".npz"))
    g = lambda k: np.stack([z[f"{e}/{k}"] for e in range(meta["nenv"])])
    return meta, {k: g(k) for k in ("geom_xpos", "geom_xmat", "pnt", "vec", "dist", "geomid", "runner_up")}


@functools.lru_cache(maxsize=None)
def host_model(xml, dtype_name):
    return load_model(xml, dtype=getattr(torch, dtype_name))


def candidate_list(mx, ids, dtype):
    """(geom id, type, size, triangles) of the geoms ``ids`` (tie-break order) from the compiled model's own arrays: sizes and float32 mesh
    vertices as the dtype holds them."""
    T = mx.tables.ray
    size = np.asarray(mx.geom_size.detach().cpu().numpy(), dtype=dtype)
    out = []
    for g in ids:
        t, tri = int(T["geom_type"][g]), None
        if t == rr.MESH:
            mid = int(T["geom_dataid"][g])
            fa, fn, va = int(T["mesh_faceadr"][mid]), int(T["mesh_facenum"][mid]), int(T["mesh_vertadr"][mid])
            tri = np.asarray(T["mesh_vert"], dtype=np.float32)[np.asarray(T["mesh_face"])[fa:fa + fn] + va].reshape(-1, 9).astype(dtype)
        out.append((int(g), t, size[g], tri))
    return out


def tiled_frames(xpos, xmat, B, seed):
    """[n, ngeom, ..] recorded frames -> B environments, environment e = recording e % n with every geom shifted by a seeded offset."""
    n = xpos.shape[0]
    idx = np.arange(B) % n
    off = np.random.RandomState(seed).uniform(-SHIFT, SHIFT, (B,) + xpos.shape[1:]).astype(xpos.dtype)
    return (xpos[idx] + off).astype(xpos.dtype), np.ascontiguousarray(xmat[idx])


def _unit(rng):
    u = rng.randn(3)
    return u / np.linalg.norm(u)


def _perp(rng, d):
    n = np.cross(d, _unit(rng))
    return n / np.linalg.norm(n)


def _offset(rng, eps):
    lo = np.log10(OFFSET_EPS * eps)
    return 10.0 ** rng.uniform(lo, max(lo, -2.0)) * (1 if rng.rand() < 0.5 else -1)


def _reach(g, t, size, tri):
    """A radius that encloses the geom about its centre."""
    if t == rr.MESH:
        return float(np.abs(tri).max()) * 1.8
    return {2: size[0], 3: size[0] + size[1], 4: max(size), 5: float(np.hypot(size[0], size[1])), 6: float(np.linalg.norm(size))}.get(t, 1.0)


def _aimed_at(rng, cand_entry, xpos, xmat, local=None):
    """A ray from outside the geom through the point ``local`` (geom frame; the centre by default), direction unnormalised."""
    g, t, size, tri = cand_entry
    if t == 0:  # the plane: from above, downward through a point of it
        q = xpos[g] + xmat[g] @ (np.r_[rng.uniform(-0.4, 0.4, 2), 0.0] if local is None else local)
        p = q + xmat[g] @ np.r_[rng.uniform(-0.3, 0.3, 2), rng.uniform(0.5, 1.5)]
        return p, (q - p) * rng.uniform(0.5, 2.0)
    q = xpos[g] + xmat[g] @ (np.zeros(3) if local is None else local)
    u = _unit(rng)
    u[2] = abs(u[2])  # from above: the floor is not in the way
    p = q + (xmat[g] @ u if local is not None else u) * (_reach(*cand_entry) + rng.uniform(0.05, 0.3))
    return p, (q - p) * rng.uniform(0.5, 2.0)


def _mix(rng, i, cand, xpos, xmat):
    """The scene generator's mix (tools/gen_ray_golden.py make_rays)."""
    k = i % 16
    inside = [c for c in cand if c[1] in (2, 3, 6)]
    if k < 4:
        c = cand[rng.randint(len(cand))]
        p = xpos[c[0]] + rng.uniform(0.5, 2.0) * _unit(rng)
        return p, (xpos[c[0]] - p) * rng.uniform(0.3, 3.0)
    if k < 6:
        return rng.uniform(-1.5, 1.5, 3) + [0, 0, 0.5], _unit(rng) * rng.uniform(0.2, 2.0)
    if k < 8 and inside:
        c = inside[rng.randint(len(inside))]
        return xpos[c[0]] + 0.01 * rng.randn(3), _unit(rng)
    if k < 10:  # the height scan, a little off the vertical: a ray exactly parallel to a mesh face has no decided answer (its triangle's det is 0)
        return np.array([rng.uniform(-0.9, 0.9), rng.uniform(-0.9, 0.9), 2.0]), np.r_[0.01 * rng.randn(2), -1.0] * rng.uniform(0.5, 2.0)
    if k == 10:
        return np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(0.05, 0.6)]), np.r_[_unit(rng)[:2], 0.0]
    if k == 11:
        return _miss(rng)
    return (np.array([rng.uniform(-1.5, 1.5), rng.uniform(-1.5, 1.5), rng.uniform(0.8, 2.5)]),
            np.array([rng.randn(), rng.randn(), -abs(rng.randn()) - 0.3]))


def _miss(rng):
    return np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), 20.0]), np.array([0.1 * rng.randn(), 0.1 * rng.randn(), 1.0])


def _family_ray(fam, rng, i, cand, xpos, xmat, eps):
    """One ray of family ``fam`` (the mix where the candidates hold no geom the family needs) -> (pnt, vec)."""
    pick = lambda types: [c for c in cand if c[1] in types]
    if fam == "mesh_edge" and pick((rr.MESH,)):  # through a shared edge or a vertex of a mesh, off it by a small offset
        c = pick((rr.MESH,))[rng.randint(len(pick((rr.MESH,))))]
        v = c[3][rng.randint(len(c[3]))].reshape(3, 3).astype(np.float64)
        k = rng.randint(3)
        s = rng.choice([0.0, 1.0, rng.uniform(0.1, 0.9)])  # a vertex or a point of the edge
        q = v[k] * (1 - s) + v[(k + 1) % 3] * s
        return _aimed_at(rng, c, xpos, xmat, local=q + _unit(rng) * abs(_offset(rng, eps)))
    if fam == "seam_rim" and pick((3, 5)):  # the capsule's side / cap seam, the cylinder's rim
        c = pick((3, 5))[rng.randint(len(pick((3, 5))))]
        a = rng.uniform(0, 2 * np.pi)
        r = c[2][0] * (1.0 if c[1] == 3 else 1.0 + min(_offset(rng, eps), 0.0))  # the rim: from inside the cap's disc or at it
        q = np.array([r * np.cos(a), r * np.sin(a), (c[2][1] + _offset(rng, eps)) * (1 if rng.rand() < 0.5 else -1)])
        return _aimed_at(rng, c, xpos, xmat, local=q)
    if fam == "graze" and pick((2,)):  # past a sphere at (1 +- 1e-3) of its radius: decided, and ill-conditioned
        c = pick((2,))[rng.randint(len(pick((2,))))]
        d = _unit(rng)
        q = xpos[c[0]] + _perp(rng, d) * c[2][0] * (1.0 + (1e-3 if rng.rand() < 0.5 else -1e-3))
        return q - d * rng.uniform(0.3, 1.0), d * rng.uniform(0.5, 2.0)
    if fam == "inside" and pick((2, 3, 4, 5, 6)):  # an origin inside a closed primitive
        c = pick((2, 3, 4, 5, 6))[rng.randint(len(pick((2, 3, 4, 5, 6))))]
        depth = {2: c[2][0], 3: c[2][0], 4: min(c[2]), 5: min(c[2][:2]), 6: min(c[2])}[c[1]]
        return xpos[c[0]] + 0.5 * depth * rng.uniform(0, 1) * _unit(rng), _unit(rng) * rng.uniform(0.5, 2.0)
    return _mix(rng, i, cand, xpos, xmat)


def make_rays(cand, xpos, xmat, R, dtype, seed):
    """(pnt [B, R, 3], vec [B, R, 3] of the dtype, family index [B, R]).  The leading slots of the flattened grid: one ray aimed at a geom
    of every candidate type (family -1), one miss (family -2); every following ray i belongs to family i % len(FAMILIES)."""
    B = xpos.shape[0]
    eps = float(np.finfo(dtype).eps)
    rng = np.random.RandomState(seed)
    types = sorted({c[1] for c in cand})
    P, V, F = np.zeros((B * R, 3)), np.zeros((B * R, 3)), np.zeros(B * R, dtype=np.int64)
    x64, m64 = xpos.astype(np.float64), xmat.astype(np.float64)
    for i in range(B * R):
        e = i // R
        if i < len(types):
            of_type = [c for c in cand if c[1] == types[i]]
            P[i], V[i], F[i] = _aimed_at(rng, of_type[rng.randint(len(of_type))], x64[e], m64[e]) + (-1,)
        elif i == len(types):
            P[i], V[i], F[i] = _miss(rng) + (-2,)
        else:
            F[i] = i % len(FAMILIES)
            P[i], V[i] = _family_ray(FAMILIES[F[i]], rng, i, cand, x64[e], m64[e], eps)
    return P.reshape(B, R, 3).astype(dtype), V.reshape(B, R, 3).astype(dtype), F.reshape(B, R)


@functools.lru_cache(maxsize=None)
def ray_case(name, B, R):
    """Everything test_ray_edges sends to the GPU for one (model, shape), and the reference's answer for it."""
    gold, flg_static, bodyexclude = RAY_MODELS[name]
    meta, a = ray_golden(gold)
    dtype = np.dtype(meta["dtype"])
    mx = host_model(meta["xml"], meta["dtype"])
    cand = candidate_list(mx, meta["candidates"], dtype)
    seed = 1000 * B + R
    xpos, xmat = tiled_frames(a["geom_xpos"], a["geom_xmat"], B, seed)
    pnt, vec, fam = make_rays(cand, xpos, xmat, R, dtype, seed + 1)
    rep = lambda t: np.repeat(t, R, axis=0)
    ref = rr.cast(dtype, rep(xpos), rep(xmat), pnt.reshape(-1, 3), vec.reshape(-1, 3), cand)
    return dict(meta=meta, dtype=dtype, cand=cand, xpos=xpos, xmat=xmat, pnt=pnt, vec=vec, family=fam.reshape(-1), ref=ref,
                flg_static=flg_static, bodyexclude=bodyexclude)


def left_out_by_family(cases):
    """{family: (left out, rays)} over ``cases`` (ray_case results)."""
    out = {}
    for c in cases:
        for f in np.unique(c["family"]):
            sel = c["family"] == f
            name = FAMILIES[max(f, 0)]  # the leading slots (a ray at every type, a miss) are rays of the mix
            n0, n1 = out.get(name, (0, 0))
            out[name] = (n0 + int((~c["ref"]["decided"][sel]).sum()), n1 + int(sel.sum()))
    return out


# ---- the exact edge table (tests/golden/ray_edges/, tools/gen_ray_golden.py edge_table) -----------------------------------------------

EDGES = os.path.join(GOLD, "ray_edges", "ray_geom_edges.npz")


def edge_rows():
    z = np.load(EDGES)
    return z, json.loads(str(z["meta"]))


def held_to_the_edge_table(got, z, dtype, what):
    """got (inf for a miss) against the recorded rows: hit / miss equal; bit for bit on the rows flagged exact, elsewhere within one unit in the
    last place of the dtype."""
    got, want = np.asarray(got, dtype=np.float64), z["dist"]
    notes = json.loads(str(z["meta"]))["notes"]
    flips = np.isinf(got) != np.isinf(want)
    assert not flips.any(), f"{what}: hit / miss differs on rows {[(int(i), notes[i]) for i in np.nonzero(flips)[0]]}"
    hit = np.isfinite(want)
    ulp = np.spacing(np.abs(want[hit]).astype(dtype)).astype(np.float64)
    allowed = np.where(z["exact"][hit], 0.0, ulp)
    over = np.abs(got[hit] - want[hit]) > allowed
    rows = np.nonzero(hit)[0][over]
    assert not over.any(), f"{what}: rows {[(int(i), notes[i], float(got[i]), float(want[i])) for i in rows]}"


# ---- render ---------------------------------------------------------------------------------------------------------------------

RENDER_LEAVES = ("geom_xpos", "geom_xmat", "cam_xpos", "cam_xmat", "light_xpos", "light_xdir")
# 4c: (render golden, (W, H, ssaa) ...)
RENDER_REF_CASES = ("humanoid_f64", "ray_scene_f64", "mesh_contact_f32")
RENDER_REF_SIZES = ((1, 1, 1), (15, 17, 1), (16, 16, 1), (4, 2, 8))


@functools.lru_cache(maxsize=None)
def render_golden(case):
    z, meta = _npz(os.path.join(RENDER_GOLD, case + ".npz"))
    return meta, {k: np.stack([z[f"{e}/{k}"] for e in range(meta["nenv"])]) for k in RENDER_LEAVES}


@functools.lru_cache(maxsize=None)
def render_model(case):
    import mujoco_torch_amd as mt

    meta, _ = render_golden(case)
    dtype = getattr(torch, meta["dtype"])
    data = os.path.dirname(mt.test_data_path("ant.xml"))
    return mt.device_put(mt.mjcf.from_xml_string(meta["xml"], base_dir=data), dtype=None if dtype == torch.float64 else dtype)


def render_frames(case, B, seed=7):
    """The recorded leaves tiled to B environments, the geoms shifted per environment (cameras and lights as recorded)."""
    _, a = render_golden(case)
    out = {k: np.ascontiguousarray(v[np.arange(B) % v.shape[0]]) for k, v in a.items()}
    out["geom_xpos"], out["geom_xmat"] = tiled_frames(a["geom_xpos"], a["geom_xmat"], B, seed)
    return out


def visible_candidates(mx, dtype):
    """The renderer's candidates: every visible geom, primitives in type-major order, then the meshes (the order the recorded ray goldens'
    unfiltered candidate lists have; tests/test_ray_host.py pins it)."""
    R = importlib.import_module("mujoco_torch_amd.ray")
    ids = R.candidates(mx.tables.ray, (True, (), ()))["geom"]
    return candidate_list(mx, ids, dtype)


@functools.lru_cache(maxsize=None)
def render_ref_case(case, W, H, S, B=4):
    """depth / seg of render(W, H, ssaa=S) by the reference, per pixel: dict(decided, depth, err, seg0, seg1), each [B, H, W]."""
    meta, _ = render_golden(case)
    dtype = np.dtype(meta["dtype"])
    mx = render_model(case)
    fr = render_frames(case, B)
    cam = meta["camera_id"]
    cand = visible_candidates(mx, dtype)
    fovy = float(mx.tables.render["cam_fovy"][cam])
    pnt, vec, err = rr.pixel_rays_ref(fr["cam_xpos"][:, cam], fr["cam_xmat"][:, cam], fovy, W, H, S)
    n = H * W * S * S
    rep = lambda t: np.repeat(t, n, axis=0)
    r = rr.cast(dtype, rep(fr["geom_xpos"]), rep(fr["geom_xmat"]), pnt.reshape(-1, 3), vec.reshape(-1, 3), cand, mesh_strict=True,
                vec_err=err.reshape(-1, 3))
    shp = (B, H, W, S, S)
    dec, v, e = r["decided"].reshape(shp), r["v"].reshape(shp), r["e"].reshape(shp)
    # the kernel adds the samples in (sy, sx) order into an accumulator of the dtype and divides once: the same (v, e) arithmetic
    c = rr.Ctx(dtype, B * H * W, True)
    acc = None
    for sy in range(S):
        for sx in range(S):
            s = c.value(v[..., sy, sx].reshape(-1), e[..., sy, sx].reshape(-1))
            acc = s if acc is None else acc + s
    if S > 1:
        acc = acc / float(S * S)
    mid = (Ellipsis, S // 2, S // 2)
    return dict(decided=dec.all(axis=(3, 4)), depth=acc.v.reshape(B, H, W), err=acc.e.reshape(B, H, W), frames=fr,
                seg0=r["id0"].reshape(shp)[mid], seg1=r["id1"].reshape(shp)[mid])
