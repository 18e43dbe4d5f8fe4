"""The ray reference of tests/_ray_ref.py, pinned without a GPU: against the reference project's recorded values (the primitive table, every scene
golden, the exact edge table), against ``mt.ray_geom`` on the CPU in both dtypes, and -- with the reference alone -- the share of rays and
pixels it leaves out of the very cases tests/test_ray_edges.py and tests/test_render_edges.py send to the GPU (a condition, not a measurement)."""
import json
import os

import numpy as np
import pytest
import torch

import mujoco_torch_amd as mt
import _ray_cases as rc
import _ray_ref as rr
from _util import GOLD

RAY_GOLD = os.path.join(GOLD, "ray")
RAY_CASES = sorted(f[:-4] for f in os.listdir(RAY_GOLD) if f.endswith(".npz") and f != "ray_geom.npz")
MAX_RAYS_LEFT_OUT = 0.01    # per (scene, dtype, family)
MAX_PIXELS_LEFT_OUT = 0.02  # per render case: the share tests/test_render.py allows its edge pixels
PRIMITIVES = (0, 2, 3, 4, 5, 6)


def _held(got, ref, what, sel=None):
    """got (inf or -1 for a miss) against a reference result on its decided rows: hit / miss equal, |got - v| <= e.  Prints the worst ratio."""
    got = np.asarray(got, dtype=rr.HP)
    dec = ref["decided"] if sel is None else ref["decided"] & sel
    got_hit = np.isfinite(got) & (got != -1)
    flips = dec & (got_hit != ref["hit"])
    assert not flips.any(), f"{what}: hit / miss differs on {int(flips.sum())} decided rays, first {np.nonzero(flips)[0][:5]}"
    hit = dec & ref["hit"]
    err = np.abs(np.where(hit, got, 0) - np.where(hit, ref["v"], 0))
    ratio = float((err / np.maximum(ref["e"], rr.HP(1e-300)))[hit].max(initial=0))
    print(f"{what}: worst error / bound {ratio:.3f} over {int(hit.sum())} hits, {int((dec & ~ref['hit']).sum())} misses, {int((~ref['decided']).sum())} left out")
    over = hit & (err > ref["e"])
    assert not over.any(), f"{what}: {int(over.sum())} distances beyond their bound (worst ratio {ratio:.3g}), first {np.nonzero(over)[0][:5]}"
    return ratio


def test_primitive_table_is_decided_and_inside_the_bound():
    z = np.load(os.path.join(RAY_GOLD, "ray_geom.npz"))
    assert len(z["type"]) == 144
    for t in PRIMITIVES:
        sel = z["type"] == t
        ref = rr.ray_geom_ref(np.float64, t, z["size"][sel], z["pnt"][sel], z["vec"][sel])
        assert ref["decided"].all(), (t, np.nonzero(~ref["decided"])[0])
        _held(z["dist"][sel], ref, f"ray_geom.npz type {t}")


@pytest.mark.parametrize("case", RAY_CASES)
def test_scene_goldens_lie_inside_the_bound(case):
    """The recorded answers are the reference's float64 evaluation of the recorded frames and rays widened to float64: held at float64's eps."""
    meta, a = rc.ray_golden(case)
    mx = rc.host_model(meta["xml"], "float64")
    cand = rc.candidate_list(mx, meta["candidates"], np.float64)
    n, R = a["pnt"].shape[:2]
    rep = lambda t: np.repeat(t.astype(np.float64), R, axis=0)
    ref = rr.cast(np.float64, rep(a["geom_xpos"]), rep(a["geom_xmat"]), a["pnt"].reshape(-1, 3).astype(np.float64), a["vec"].reshape(-1, 3).astype(np.float64), cand)
    assert (~ref["decided"]).mean() <= MAX_RAYS_LEFT_OUT, (case, int((~ref["decided"]).sum()))
    _held(a["dist"].reshape(-1), ref, case)
    gid = a["geomid"].reshape(-1)
    bad = ref["decided"] & (gid != ref["id0"]) & (gid != ref["id1"])
    assert not bad.any(), f"{case}: geomid differs on {int(bad.sum())} rays that are no tie by the reference's intervals"


def _table_rays(t, n, seed):
    """n rows drawn as tools/gen_ray_golden.py's geom_table draws them, every second one aimed at the geom."""
    rng = np.random.RandomState(seed)
    i = np.arange(n)
    size = rng.uniform(0.1, 1.0, (n, 3)) if t else np.c_[rng.uniform(0.5, 3.0, (n, 2)) * (i % 3 != 0)[:, None], np.full(n, 0.1)]
    p = rng.uniform(-2, 2, (n, 3)) * np.where(i % 6 == 5, 0.2, 1.0)[:, None]
    v = np.where((i % 2 == 0)[:, None], rng.randn(n, 3), -p + 0.1 * rng.randn(n, 3))
    return size, p, v


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_host_ray_geom_lies_inside_the_bound(dtype):
    npdt = np.dtype(str(dtype).replace("torch.", ""))
    for t in PRIMITIVES:
        size, p, v = (x.astype(npdt) for x in _table_rays(t, 20000, 100 + t))
        ref = rr.ray_geom_ref(npdt, t, size, p, v)
        assert (~ref["decided"]).mean() <= MAX_RAYS_LEFT_OUT, (t, int((~ref["decided"]).sum()))
        assert ref["hit"].mean() > 0.2 and (ref["decided"] & ~ref["hit"]).mean() > 0.05, t
        got = mt.ray_geom(torch.tensor(size), torch.tensor(p), torch.tensor(v), t)
        assert got.dtype == dtype
        _held(got.numpy(), ref, f"ray_geom {npdt.name} type {t}")


@pytest.mark.parametrize("model", list(rc.RAY_MODELS))
def test_left_out_share_of_the_gpu_rays(model):
    """At most 1 % of the rays of a family are left out, and every case keeps hits on every candidate type it contains and misses."""
    cases = [rc.ray_case(model, B, R) for B, R in rc.RAY_SHAPES]
    for (B, R), c in zip(rc.RAY_SHAPES, cases):
        ref, types = c["ref"], {g: t for g, t, _, _ in c["cand"]}
        assert sorted({types[g] for g in ref["id0"][ref["hit"]]}) == sorted(set(types.values())), (model, B, R)
        assert (ref["decided"] & ~ref["hit"]).any(), (model, B, R)
    shares = rc.left_out_by_family(cases)
    print(model, {f: f"{a} / {n}" for f, (a, n) in shares.items()})
    assert set(shares) == set(rc.FAMILIES)
    for f, (a, n) in shares.items():
        assert a <= MAX_RAYS_LEFT_OUT * n, f"{model}: family {f} leaves out {a} of {n} rays"


@pytest.mark.parametrize("case", rc.RENDER_REF_CASES)
def test_left_out_share_of_the_gpu_pixels(case):
    """At most 2 % of a case's pixels (its four image sizes together: the 4 x 2 image alone has 32) are left out; every size keeps hits."""
    out = total = 0
    for W, H, S in rc.RENDER_REF_SIZES:
        r = rc.render_ref_case(case, W, H, S)
        assert (r["decided"] & (r["seg0"] >= 0)).any(), (case, W, H, S)
        out, total = out + int((~r["decided"]).sum()), total + r["decided"].size
    print(f"{case}: {out} of {total} pixels left out")
    assert out <= MAX_PIXELS_LEFT_OUT * total, (case, out, total)


def test_pixel_directions_match_the_ones_test_render_builds():
    """pixel_rays_ref against the torch construction of tests/test_render.py::test_depth_and_seg_agree_with_ray (on the CPU), within its bound."""
    for case in ("ray_scene_f64", "mesh_contact_f32", "humanoid_f64"):
        meta, a = rc.render_golden(case)
        mx = rc.render_model(case)
        W, H, c = meta["width"], meta["height"], meta["camera_id"]
        dtype = getattr(torch, meta["dtype"])
        fovy = float(mx.tables.render["cam_fovy"][c])
        half_h = torch.tan(torch.tensor(fovy * (torch.pi / 360.0), dtype=dtype))
        half_w = half_h * (W / H)
        u = torch.linspace(0.5, W - 0.5, W, dtype=dtype)
        v = torch.linspace(0.5, H - 0.5, H, dtype=dtype)
        u, v = torch.meshgrid(u, v, indexing="xy")
        dc = torch.stack([(2 * u / W - 1) * half_w, (1 - 2 * v / H) * half_h, -torch.ones_like(u)], -1)
        dc = dc / torch.sqrt((dc * dc).sum(-1, keepdim=True))
        xm = torch.tensor(a["cam_xmat"][:, c])
        vec = torch.stack([xm[:, i, 0, None, None] * dc[..., 0] + xm[:, i, 1, None, None] * dc[..., 1] + xm[:, i, 2, None, None] * dc[..., 2]
                           for i in range(3)], -1)
        pnt, want, err = rr.pixel_rays_ref(a["cam_xpos"][:, c], a["cam_xmat"][:, c], fovy, W, H, 1)
        assert np.array_equal(pnt[:, 0, 0, 0, 0], a["cam_xpos"][:, c].astype(rr.HP))
        diff = np.abs(vec.numpy().astype(rr.HP) - want[:, :, :, 0, 0])
        ratio = float((diff / np.maximum(err[:, :, :, 0, 0], rr.HP(1e-300))).max())
        print(f"{case}: pixel directions, worst error / bound {ratio:.3f}")
        assert (diff <= err[:, :, :, 0, 0]).all(), (case, ratio)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_host_ray_geom_on_the_exact_edge_table(dtype):
    z, meta = rc.edge_rows()
    for k in ("tangent", "origin on the surface", "origin inside", "zero vector", "rim", "seam", "edge", "corner", "vertex", "border", "size 0", "== 0"):
        assert any(k in n for n in meta["notes"]), k
    npdt = np.dtype(str(dtype).replace("torch.", ""))
    got = np.full(len(z["type"]), np.nan)
    for t in PRIMITIVES:
        sel = z["type"] == t
        got[sel] = mt.ray_geom(torch.tensor(z["size"][sel], dtype=dtype), torch.tensor(z["pnt"][sel], dtype=dtype), torch.tensor(z["vec"][sel], dtype=dtype), t).double().numpy()
    prim = z["type"] != rr.MESH
    sub = {k: z[k][prim] for k in ("dist", "exact")}
    sub["meta"] = np.array(json.dumps(dict(notes=[n for n, p in zip(meta["notes"], prim) if p])))
    rc.held_to_the_edge_table(got[prim], sub, npdt, f"ray_geom {npdt.name}")
