"""``mt.ray`` on the GPU against the high-precision reference of tests/_ray_ref.py at the launch shapes where the kernel's environment slots, LDS
chunks and workgroup boundaries can go wrong, on the reference project's exact edge table (tests/golden/ray_edges/), and with no candidates.

Every distance is held to the reference's own propagated bound at the Data dtype's eps (``|got - v| <= e``), a miss is exactly ``-1 / -1``, an id is
the reference's or one of a tie by its intervals; everything else is ``torch.equal``.  The inputs (tests/_ray_cases.py) and the share of rays the
reference leaves out of them (at most 1 % per family) are checked without a GPU in tests/test_ray_ref_host.py.

Shapes ``(B, R)`` -- ``span`` environments' frames x ``chunk`` candidates are staged in LDS per round (48 KB / (span x 12 reals)):
  (300, 1)   a workgroup of 256 environments: span at its cap of 256, chunk 2 (float64) / 4 (float32), 10 / 5 staging rounds for 20 candidates
  (5, 3)     one partly filled workgroup: the inactive lanes clone the last pair
  (7, 85)    a workgroup that starts on the last ray of an environment touches 4 environments
  (4, 255), (3, 256), (3, 257)   the switch to span = 2, workgroup boundaries inside an environment
  (40, 16)   a middle chunk size
"""
import functools
import os

import numpy as np
import pytest
import torch

import mujoco_torch_amd as mt
import _ray_cases as rc
import _ray_ref as rr
from _util import load_model

pytestmark = pytest.mark.gpu

DEV = "cuda"
DATA = os.path.dirname(mt.test_data_path("ant.xml"))


@functools.lru_cache(maxsize=None)
def _model(xml, dtype_name):
    return load_model(xml, dtype=getattr(torch, dtype_name)).to(DEV)


def _data(mx, xpos, xmat):
    d = mt.make_data(mx).expand(xpos.shape[0]).clone().to(DEV)
    return d.replace(geom_xpos=torch.tensor(xpos, device=DEV), geom_xmat=torch.tensor(xmat, device=DEV))


@pytest.mark.parametrize("shape", rc.RAY_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("model", list(rc.RAY_MODELS))
def test_ray_lies_inside_the_reference_bound(model, shape):
    B, R = shape
    c = rc.ray_case(model, B, R)
    meta, ref = c["meta"], c["ref"]
    mx = _model(meta["xml"], meta["dtype"])
    d = _data(mx, c["xpos"], c["xmat"])
    pnt, vec = torch.tensor(c["pnt"], device=DEV), torch.tensor(c["vec"], device=DEV)
    if R == 1:
        pnt, vec = pnt[:, 0], vec[:, 0]  # one ray per environment: the (B, 3) form
    dist, gid = mt.ray(mx, d, pnt, vec, flg_static=c["flg_static"], bodyexclude=c["bodyexclude"])
    assert dist.shape == ((B,) if R == 1 else (B, R)) and gid.shape == dist.shape and dist.dtype == pnt.dtype and gid.dtype == torch.int64
    dist, gid = dist.cpu().numpy().reshape(-1), gid.cpu().numpy().reshape(-1)
    what = f"{model} {B} x {R}"
    dec, hit = ref["decided"], ref["decided"] & ref["hit"]
    miss = dec & ~ref["hit"]
    types = {g: t for g, t, _, _ in c["cand"]}
    assert sorted({types[g] for g in ref["id0"][hit]}) == sorted(set(types.values())) and miss.any(), what  # hits on every candidate type, and misses
    assert np.all(dist[miss] == -1) and np.all(gid[miss] == -1), f"{what}: {int(np.sum(gid[miss] != -1))} misses hit"
    assert np.all(gid[hit] >= 0), f"{what}: {int(np.sum(gid[hit] < 0))} hits missed, first {np.nonzero(hit & (gid < 0))[0][:5]}"
    err = np.abs(dist.astype(rr.HP) - ref["v"])
    ratio = float((err / np.maximum(ref["e"], rr.HP(1e-300)))[hit].max())
    print(f"{what}: worst error / bound {ratio:.3f} over {int(hit.sum())} hits, {int(miss.sum())} misses, {int((~dec).sum())} left out, "
          f"{int((ref['id0'] != ref['id1'])[hit].sum())} ties; largest bound {float(ref['e'].max()):.3g}")
    over = hit & (err > ref["e"])
    assert not over.any(), f"{what}: {int(over.sum())} distances beyond their bound (worst ratio {ratio:.3g}), first {np.nonzero(over)[0][:5]}"
    wrong = hit & (gid != ref["id0"]) & (gid != ref["id1"])
    assert not wrong.any(), f"{what}: geomid differs on {int(wrong.sum())} rays without a tie, first {np.nonzero(wrong)[0][:5]}"


# ---- the exact edge table: one geom per type, isolated by geomgroup (the mesh by bodyexclude), posed in signed-permutation frames ------------

_GROUP = {0: 0, 2: 1, 3: 2, 4: 3, 5: 4, 6: 5, 7: 0}  # type -> geom group in the table's scene; geom ids are in the same order


def _mask(g):
    return tuple(1 if k == g else 0 for k in range(6))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_ray_on_the_exact_edge_table(dtype):
    z, meta = rc.edge_rows()
    npdt = np.dtype(str(dtype).replace("torch.", ""))
    lite = mt.mjcf.from_xml_string(meta["xml"], base_dir=DATA)
    assert np.asarray(lite.mesh_vert).shape == z["mesh_vert"].shape
    lite.mesh_vert = z["mesh_vert"].astype(np.asarray(lite.mesh_vert).dtype)  # the tetrahedron's vertices by value
    mx = mt.device_put(lite, dtype=None if dtype == torch.float64 else dtype).to(DEV)
    gtype = np.asarray(mx.tables.ray["geom_type"])
    assert gtype.tolist() == [0, 2, 3, 4, 5, 6, 7]
    got = np.full(len(z["type"]), np.nan)
    for t in np.unique(z["type"]):
        g = int(np.nonzero(gtype == t)[0][0])
        for size in np.unique(z["size"][z["type"] == t], axis=0):
            rows = np.nonzero((z["type"] == t) & (z["size"] == size).all(1))[0]
            gs = mx.geom_size.clone()
            gs[g] = torch.tensor(size, dtype=gs.dtype)
            xpos, xmat = np.zeros((len(rows), len(gtype), 3)), np.tile(np.eye(3), (len(rows), len(gtype), 1, 1))
            xpos[:, g], xmat[:, g] = z["geom_xpos"][rows], z["geom_xmat"][rows]
            pnt = z["geom_xpos"][rows] + np.einsum("rij,rj->ri", z["geom_xmat"][rows], z["pnt"][rows])  # exact: multiples of 1/4, signed permutations
            vec = np.einsum("rij,rj->ri", z["geom_xmat"][rows], z["vec"][rows])
            d = _data(mx, xpos.astype(npdt), xmat.astype(npdt))
            dist, gid = mt.ray(mx.replace(geom_size=gs), d, torch.tensor(pnt.astype(npdt), device=DEV), torch.tensor(vec.astype(npdt), device=DEV),
                               geomgroup=_mask(_GROUP[int(t)]), bodyexclude=0 if t == rr.MESH else 6)
            dist, gid = dist.double().cpu().numpy(), gid.cpu().numpy()
            assert np.array_equal(gid, np.where(dist == -1, -1, g)), (t, gid)  # a family's hits name the intended geom
            got[rows] = np.where(gid < 0, np.inf, dist)
    rc.held_to_the_edge_table(got, z, npdt, f"ray {npdt.name}")
    assert np.isfinite(got[z["type"] == rr.MESH]).any() and np.isfinite(got[z["type"] == 5]).any()


def test_no_candidates_returns_a_miss_everywhere():
    """geomgroup of all zeros: a launch with ncand = 0."""
    c = rc.ray_case("ray_scene_f64", 5, 3)
    mx = _model("ray_scene", "float64")
    d = _data(mx, c["xpos"], c["xmat"])
    dist, gid = mt.ray(mx, d, torch.tensor(c["pnt"], device=DEV), torch.tensor(c["vec"], device=DEV), geomgroup=(0,) * 6)
    assert dist.shape == (5, 3) and torch.equal(dist, torch.full_like(dist, -1.0)) and torch.equal(gid, torch.full_like(gid, -1))
