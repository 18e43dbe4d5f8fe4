"""Rendering without a GPU: the public signatures, the C entry point, materials in the compiler (and that they leave ray casting and the
rangefinders alone), argument validation, the texture warning and the zoo's pixel observation spec."""
import importlib
import inspect
import os
import re
import warnings

import numpy as np
import pytest
import torch

import mujoco_torch_amd as mt
from _util import load_model
from mujoco_torch_amd import native
from mujoco_torch_amd.device import _sensor_tables
from mujoco_torch_amd.ray import candidates
from mujoco_torch_amd.zoo import ENVS, base

R = importlib.import_module("mujoco_torch_amd.render")  # (the package attribute `render` is the function)
REF_PARAMS = ["camera_id", "width", "height", "precomp", "shading", "background", "shadows", "fog", "ssaa"]
DATA = os.path.dirname(mt.test_data_path("ant.xml"))
BUNDLED = sorted(f[:-4] for f in os.listdir(DATA) if f.endswith(".xml"))


def test_render_functions_are_public_with_the_reference_signatures():
    assert list(inspect.signature(mt.precompute_render_data).parameters) == ["m"]
    assert list(inspect.signature(mt.render).parameters) == ["m", "d"] + REF_PARAMS
    assert list(inspect.signature(mt.render_batch).parameters) == ["m", "d_batch"] + REF_PARAMS
    for f in (mt.render, mt.render_batch):
        p = inspect.signature(f).parameters
        assert [p[n].default for n in REF_PARAMS] == [0, 64, 64, None, True, None, False, None, 1]


def test_entry_point_is_declared_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(native.HEADER).read(), flags=re.S)
    assert re.search(r"\bint mjh_render\s*\(const mjhModel\* m, const void\* geom_xpos, const void\* geom_xmat, const void\* cam_xpos,", text)
    assert re.search(r"typedef struct mjhRenderScene \{.*?\} mjhRenderScene;", text, flags=re.S)
    assert re.search(r"typedef struct mjhRenderParams \{.*?\} mjhRenderParams;", text, flags=re.S)
    assert re.search(r"#define MJH_KERNEL_RENDER 22\b", open(native.HEADER).read())
    if os.path.exists(native.LIB_PATH):
        lib = native.load_library()
        assert hasattr(lib, "mjh_render")
        native.check_abi(lib)


def test_materials_compile():
    lite = mt.mjcf.from_xml_path(mt.test_data_path("ant.xml"))
    assert lite.nmat == 1 and lite.ntex == 0
    np.testing.assert_array_equal(lite.mat_rgba, np.array([[0.8, 0.6, 0.4, 1.0]], dtype=np.float32))
    assert (lite.geom_matid == 0).all()  # every geom takes `self` from the default class
    scene = mt.mjcf.from_xml_path(mt.test_data_path("render_scene.xml"))
    names = ["floor", "pillar", "block", "ball", "arm", "egg"]
    assert scene.geom_matid.tolist() == [2, 0, -1, 1, -1, -1]  # plain (rgba defaults to 1 1 1 1), clay, none, jade through a class
    np.testing.assert_array_equal(scene.mat_rgba[2], np.ones(4, dtype=np.float32))
    assert len(names) == scene.ngeom
    nomat = mt.mjcf.from_xml_path(mt.test_data_path("mesh_contact.xml"))
    assert nomat.nmat == 0 and (nomat.geom_matid == -1).all() and not hasattr(nomat, "mat_rgba")
    with pytest.raises(ValueError, match="unknown material"):
        mt.mjcf.from_xml_string('<mujoco><worldbody><geom size="1" material="nope"/></worldbody></mujoco>')


def _no_materials(lite):
    lite.geom_matid = -np.ones(int(lite.ngeom), dtype=np.int32)
    if hasattr(lite, "mat_rgba"):
        del lite.mat_rgba
    lite.nmat = 0
    return lite


@pytest.mark.parametrize("xml", BUNDLED)
def test_materials_leave_ray_candidates_and_rangefinders_unchanged(xml):
    """Every bundled material is opaque: the ray candidate tables and the rangefinder geom lists are those of the model without materials."""
    with_mat = mt.mjcf.from_xml_path(mt.test_data_path(xml + ".xml"))
    without = _no_materials(mt.mjcf.from_xml_path(mt.test_data_path(xml + ".xml")))
    from mujoco_torch_amd.ray import host_tables

    ta, tb = host_tables(with_mat), host_tables(without)
    for key in ((True, (), ()), (False, (), ()), (True, (1,), ())):
        ca, cb = candidates(ta, key), candidates(tb, key)
        for k in ("geom", "type", "tri_range", "tri"):
            np.testing.assert_array_equal(ca[k], cb[k])
    if int(getattr(with_mat, "nsensor", 0) or 0):
        sa, sb = _sensor_tables(with_mat), _sensor_tables(without)
        assert sa["rf_geom"] == sb["rf_geom"] and sa["rfadr"] == sb["rfadr"]


def test_argument_validation():
    mx = load_model("render_scene")
    d = mt.make_data(mx)
    for kw in (dict(camera_id=1), dict(camera_id=-1), dict(width=0), dict(height=0), dict(ssaa=0), dict(background=(1, 2))):
        with pytest.raises(ValueError):
            mt.render(mx, d, **kw)
    with pytest.raises(ValueError):
        mt.render(mx, d, precomp=mt.precompute_render_data(load_model("ray_scene")))
    with pytest.raises(ValueError):
        mt.render_batch(mx, d)  # no batch dimension
    with pytest.raises(RuntimeError, match="HIP device"):  # the same refusal as ray / step: no CPU path
        mt.render(mx, d, precomp=mt.precompute_render_data(mx))
    with pytest.raises(ValueError):
        mt.render(load_model("mesh_contact"), mt.make_data(load_model("mesh_contact")))  # no camera


def test_rgb_dtypes_follow_the_reference():
    mx = load_model("render_scene")
    o = lambda **kw: R._options(mx, 0, 8, 4, kw.get("shading", True), None, False, kw.get("fog"), 1)
    assert R.rgb_dtype(mx, torch.float64, o()) == torch.float64
    assert R.rgb_dtype(mx, torch.float64, o(shading=False)) == torch.float32
    assert R.rgb_dtype(mx, torch.float64, o(shading=False, fog=((0, 0, 0), 1, 2))) == torch.float64
    assert R.rgb_dtype(mx, torch.float32, o()) == torch.float32
    assert R.rgb_dtype(mx, torch.float64, o(), u8=True) == torch.uint8


def test_texture_warning_once_per_model():
    mx = load_model("humanoid")  # its floor's material names a texture
    R._WARNED.discard(mx.tables.uid)
    with pytest.warns(UserWarning, match="texture"):
        R._texture_warning(mx)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        R._texture_warning(mx)
        R._texture_warning(load_model("render_scene"))  # no textures: no warning


def test_light_rows():
    mx = load_model("render_scene")
    rows = R.light_rows(mx.tables.render, torch.float64)
    assert rows.shape == (3, 16)
    assert float(rows[0, 12]) == float(torch.cos(torch.tensor(35.0 * torch.pi / 180, dtype=torch.float64)))
    assert rows[:, 13].tolist() == [0.0, 1.0, 0.0] and rows[:, 14].tolist() == [1.0, 1.0, 0.0]
    assert float(rows[2, 12]) == 2.0  # cutoff 180: no cone
    np.testing.assert_array_equal(rows[2, 9:12].numpy(), np.array([1, 0.2, 0.05], dtype=np.float32).astype(np.float64))


@pytest.mark.parametrize("pixel_only", [False, True])
def test_zoo_pixel_spec(monkeypatch, pixel_only):
    monkeypatch.setattr(base, "step", lambda m, d, **kw: d)  # the constructor's warm-up step: not what is tested here
    env = ENVS["cartpole"](num_envs=3, from_pixels=True, pixel_only=pixel_only, render_width=20, render_height=10)
    spec = env.observation_spec["pixels"]
    assert tuple(spec.shape) == (3, 10, 20, 3) and spec.dtype == torch.uint8
    assert ("observation" in env.observation_spec.keys()) != pixel_only
    assert ENVS["satellite_small"].RENDER_BACKGROUND == (0.0, 0.0, 0.05) and ENVS["cartpole"].RENDER_BACKGROUND == (0.4, 0.6, 0.8)
