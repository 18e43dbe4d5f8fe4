"""Ray casting without a GPU: ``ray_geom`` against the reference's recorded values, the candidate tables against the recorded filter semantics
(tests/golden/ray/, tools/gen_ray_golden.py), argument validation, and the C entry point."""
import importlib
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import mujoco_torch_amd as mt
from _util import GOLD, load_model
from mujoco_torch_amd import native

R = importlib.import_module("mujoco_torch_amd.ray")
RAY_GOLD = os.path.join(GOLD, "ray")
RAY_CASES = sorted(f[:-4] for f in os.listdir(RAY_GOLD) if f.endswith(".npz") and f != "ray_geom.npz")


def test_ray_and_ray_geom_are_public_with_the_reference_signatures():
    assert list(inspect.signature(mt.ray).parameters) == ["m", "d", "pnt", "vec", "geomgroup", "flg_static", "bodyexclude"]
    assert list(inspect.signature(mt.ray_geom).parameters) == ["size", "pnt", "vec", "geomtype"]


def test_entry_point_is_declared_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(native.HEADER).read(), flags=re.S)
    assert re.search(r"\bint mjh_ray\s*\(const mjhModel\* m, const void\* geom_xpos, const void\* geom_xmat, const void\* pnt, int64_t pnt_env,", text)
    assert re.search(r"typedef struct mjhRayCands \{\s*int64_t ncand;\s*const int32_t\* cand;\s*const void\* tri;\s*const void\* geom_size;\s*\} mjhRayCands;", text)
    if os.path.exists(native.LIB_PATH):
        assert hasattr(native.load_library(), "mjh_ray")


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_ray_geom_matches_the_reference_table(dtype):
    z = np.load(os.path.join(RAY_GOLD, "ray_geom.npz"))
    tol = 1e-12 if dtype == torch.float64 else 1e-4
    for t in np.unique(z["type"]):
        sel = z["type"] == t
        got = mt.ray_geom(torch.tensor(z["size"][sel], dtype=dtype), torch.tensor(z["pnt"][sel], dtype=dtype), torch.tensor(z["vec"][sel], dtype=dtype), int(t))
        want = z["dist"][sel]
        got = got.double().numpy()
        assert np.array_equal(np.isinf(got), np.isinf(want)) or dtype == torch.float32, (t, got, want)
        fin = np.isfinite(want) & np.isfinite(got)
        assert np.all(np.abs(got[fin] - want[fin]) <= tol * np.maximum(1.0, np.abs(want[fin]))), (t, got, want)
        # elementwise: one row at a time gives the same as the batch
        i = int(np.nonzero(sel)[0][0])
        one = mt.ray_geom(torch.tensor(z["size"][i], dtype=dtype), torch.tensor(z["pnt"][i], dtype=dtype), torch.tensor(z["vec"][i], dtype=dtype), int(t))
        assert one.shape == () and float(one) == float(got[0]) or (np.isinf(float(one)) and np.isinf(got[0]))


def test_ray_geom_refuses_meshes():
    with pytest.raises(ValueError):
        mt.ray_geom(torch.ones(3), torch.zeros(3), torch.ones(3), mt.GeomType.MESH)


def _meta(case):
    return json.loads(str(np.load(os.path.join(RAY_GOLD, case + ".npz"))["meta"]))


@pytest.mark.parametrize("case", RAY_CASES)
def test_candidates_follow_the_recorded_filters(case):
    """Order (type-major, ascending id), flg_static, bodyexclude, geomgroup and alpha: the table is the reference's candidate list."""
    meta = _meta(case)
    mx = load_model(meta["xml"])
    key = R.filter_key(mx.tables.ray, meta["geomgroup"], meta["flg_static"], meta["bodyexclude"])
    c = R.candidates(mx.tables.ray, key)
    assert c["geom"].tolist() == meta["candidates"]
    gtype = mx.tables.ray["geom_type"]
    assert c["type"].tolist() == [int(gtype[g]) for g in meta["candidates"]]
    for g, (b, e) in zip(c["geom"], c["tri_range"]):
        if gtype[g] == 7:
            assert e > b and c["tri"][b:e].shape[1] == 9
            assert np.array_equal(c["tri"][b:e], c["tri"][b:e].astype(np.float32).astype(np.float64))  # float32-rounded vertices


def test_ray_scene_filters():
    mx = load_model("ray_scene")
    T = mx.tables.ray
    names = ["floor", "pillar", "ghost", "ball", "arm", "egg", "crate", "can", "gem", "spike"]
    ids = lambda key: [names[g] for g in R.candidates(T, key)["geom"]]
    assert ids(R.filter_key(T, (), True, -1)) == ["floor", "ball", "arm", "egg", "pillar", "can", "crate", "gem", "spike"]  # ghost: alpha 0
    assert ids(R.filter_key(T, (), False, -1)) == ["ball", "arm", "egg", "can", "crate", "gem", "spike"]  # no static geoms
    assert ids(R.filter_key(T, (), True, [1, 3])) == ["floor", "pillar", "can", "crate", "spike"]  # torso and gem excluded
    assert ids(R.filter_key(T, (0, 1, 0, 0, 0, 0), True, -1)) == ["pillar", "crate"]  # group 1 only
    assert ids(R.filter_key(T, (0,) * 6, True, -1)) == []
    assert R.filter_key(T, (), True, 2) == R.filter_key(T, (), True, [2])


def test_argument_validation():
    mx = load_model("ray_scene")
    d = mt.make_data(mx).expand(4).clone()
    f64 = dict(dtype=torch.float64)
    ok = torch.zeros(3, **f64)
    for bad in (torch.zeros(4, **f64), torch.zeros(2, 3, **f64), torch.zeros(4, 5, 2, **f64), torch.zeros(4, 2, 2, 3, **f64)):
        with pytest.raises(ValueError):
            mt.ray(mx, d, bad, ok)
        with pytest.raises(ValueError):
            mt.ray(mx, d, ok, bad)
    with pytest.raises(ValueError):  # rays per environment do not broadcast
        mt.ray(mx, d, torch.zeros(4, 2, 3, **f64), torch.zeros(4, 3, 3, **f64))
    with pytest.raises(ValueError):  # dtype
        mt.ray(mx, d, torch.zeros(3, dtype=torch.float32), ok)
    with pytest.raises(ValueError):  # device
        mt.ray(mx, d, ok, torch.zeros(3, dtype=torch.float64, device="meta"))
    with pytest.raises(ValueError):  # a 6-entry mask
        mt.ray(mx, d, ok, ok, geomgroup=(1, 1))
    with pytest.raises(RuntimeError, match="HIP device"):  # no CPU path: the error step raises
        mt.ray(mx, d, ok, ok)
    assert R.ray_shapes((4,), (3,), (4, 7, 3))[:2] == ((4, 7), 7)
    assert R.ray_shapes((4,), (4, 3), (3,))[:2] == ((4,), 1)
    assert R.ray_shapes((2, 4), (2, 4, 1, 3), (2, 4, 5, 3))[:2] == ((2, 4, 5), 5)
    assert R.ray_shapes((), (6, 3), (3,))[:2] == ((6,), 6)


def test_geom_group_out_of_range_raises():
    lite = mt.mjcf.from_xml_path(mt.test_data_path("ray_scene.xml"))
    lite.geom_group = np.array(lite.geom_group).copy()
    lite.geom_group[3] = 7
    mx = mt.device_put(lite)
    d = mt.make_data(mx)
    z = torch.zeros(3, dtype=torch.float64)
    with pytest.raises(ValueError, match="geom groups"):
        mt.ray(mx, d, z, z, geomgroup=(1, 1, 1, 1, 1, 1))
    with pytest.raises(RuntimeError, match="HIP device"):  # without a mask the groups are not read
        mt.ray(mx, d, z, z)
