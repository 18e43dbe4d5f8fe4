"""Rendering on the GPU: ``mujoco_torch_amd.render`` against the reference's own renderer (tests/golden/render/, tools/gen_render_golden.py),
depth / seg against ``ray`` on the same pixel rays, the vmap / compile operator, batches cut into several launches, no mutation of the input,
value edits of the model, the uint8 path and the zoo's pixel observations."""
import importlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import mujoco_torch_amd as mt
from _util import GOLD, load_model
from mujoco_torch_amd.zoo import ENVS

pytestmark = pytest.mark.gpu

R = importlib.import_module("mujoco_torch_amd.render")
RENDER_GOLD = os.path.join(GOLD, "render")
CASES = sorted(f[:-4] for f in os.listdir(RENDER_GOLD) if f.endswith(".npz"))
LEAVES = ("geom_xpos", "geom_xmat", "cam_xpos", "cam_xmat", "light_xpos", "light_xdir")
DATA = os.path.dirname(mt.test_data_path("ant.xml"))
DEV = "cuda"


def _case(case):
    z = np.load(os.path.join(RENDER_GOLD, case + ".npz"))
    meta = json.loads(str(z["meta"]))
    g = lambda k: np.stack([z[f"{e}/{k}"] for e in range(meta["nenv"])])
    dtype = getattr(torch, meta["dtype"])
    mx = mt.device_put(mt.mjcf.from_xml_string(meta["xml"], base_dir=DATA), dtype=None if dtype == torch.float64 else dtype).to(DEV)
    d = mt.make_data(mx).expand(meta["nenv"]).clone().to(DEV)
    d = d.replace(**{k: torch.tensor(g(k), device=DEV) for k in LEAVES})
    return meta, mx, d, {k: g(k) for k in ("rgb", "depth", "seg", "edge")}


def _kw(meta):
    kw = dict(meta["settings"])
    if "fog" in kw:
        kw["fog"] = (tuple(kw["fog"][0]), kw["fog"][1], kw["fog"][2])
    return dict(camera_id=meta["camera_id"], width=meta["width"], height=meta["height"], **kw)


@pytest.mark.parametrize("case", CASES)
def test_matches_the_reference(case):
    meta, mx, d, want = _case(case)
    rgb, depth, seg = mt.render(mx, d, **_kw(meta))
    assert [str(t.dtype).replace("torch.", "") for t in (rgb, depth, seg)] == meta["out_dtypes"]
    n, H, W = meta["nenv"], meta["height"], meta["width"]
    assert rgb.shape == (n, H, W, 3) and depth.shape == (n, H, W) and seg.shape == (n, H, W)
    edge = want["edge"]
    assert edge.mean(axis=(1, 2)).max() <= 0.02, f"{case}: edge pixels {edge.mean(axis=(1, 2))}"
    ok = ~edge
    seg = seg.cpu().numpy()
    assert np.array_equal(seg[ok], want["seg"][ok]), f"{case}: seg differs on {int((seg[ok] != want['seg'][ok]).sum())} pixels"
    # the tolerances of test_ray.py by the model's dtype; a float32 image of a float64 model (flat colours) to a few float32 ulps
    tol = 1e-9 if meta["dtype"] == "float64" else 1e-4
    rtol = tol if rgb.dtype == torch.float64 or meta["dtype"] == "float32" else 1e-6
    err_d = np.abs(depth.double().cpu().numpy() - want["depth"])[ok] / np.maximum(1.0, np.abs(want["depth"][ok]))
    err_c = np.abs(rgb.double().cpu().numpy() - want["rgb"])[ok].max(axis=-1, initial=0)
    assert err_d.max(initial=0) <= tol, f"{case}: depth err {err_d.max():.3e}"
    assert err_c.max(initial=0) <= rtol, f"{case}: rgb err {err_c.max():.3e}"


def test_depth_and_seg_agree_with_ray():
    """shading=False: depth / seg are mt.ray's answer for the same per-pixel rays, bit for bit."""
    for case in ("ray_scene_f64", "mesh_contact_f32", "humanoid_f64"):
        meta, mx, d, _ = _case(case)
        W, H = meta["width"], meta["height"]
        _, depth, seg = mt.render(mx, d, camera_id=meta["camera_id"], width=W, height=H, shading=False)
        dtype = d.geom_xpos.dtype
        c = meta["camera_id"]
        fovy = float(mx.tables.render["cam_fovy"][c])
        half_h = torch.tan(torch.tensor(fovy * (torch.pi / 360.0), dtype=dtype))
        half_w = half_h * (W / H)
        u = torch.linspace(0.5, W - 0.5, W, dtype=dtype)
        v = torch.linspace(0.5, H - 0.5, H, dtype=dtype)
        u, v = torch.meshgrid(u, v, indexing="xy")
        dc = torch.stack([(2 * u / W - 1) * half_w, (1 - 2 * v / H) * half_h, -torch.ones_like(u)], -1)
        dc = dc / torch.sqrt((dc * dc).sum(-1, keepdim=True))
        dc = dc.to(DEV)
        xm = d.cam_xmat[:, c]
        vec = torch.stack([xm[:, i, 0, None, None] * dc[..., 0] + xm[:, i, 1, None, None] * dc[..., 1] + xm[:, i, 2, None, None] * dc[..., 2]
                           for i in range(3)], -1)
        dist, gid = mt.ray(mx, d, d.cam_xpos[:, c], vec.reshape(vec.shape[0], -1, 3))
        # the same arithmetic up to the rounding of the pixel direction: ids agree off grazing pixels, distances to the dtype's tolerance
        tol = 1e-9 if dtype == torch.float64 else 1e-4
        same = gid.reshape(seg.shape) == seg
        assert same.float().mean() > 0.98, case
        both = same & (seg >= 0)
        err = ((dist.reshape(depth.shape) - depth).abs() / depth.abs().clamp(min=1))[both]
        assert err.max() <= tol, (case, float(err.max()))


def test_vmap_and_compile_are_bit_identical_to_render_batch():
    meta, mx, d, _ = _case("render_scene_f64")
    kw = dict(width=meta["width"], height=meta["height"], shadows=True, fog=((0.3, 0.3, 0.3), 1.0, 4.0))
    want = mt.render_batch(mx, d, **kw)
    got = torch.vmap(lambda dd: mt.render(mx, dd, **kw))(d)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and torch.equal(a, b)
    f = torch.compile(lambda dd: mt.render(mx, dd, **kw), fullgraph=True)
    for a, b in zip(f(d), want):
        assert a.dtype == b.dtype and torch.equal(a, b)
    one = mt.render(mx, d[1], **kw)  # an unbatched Data: the same image as its row of the batch
    for a, b in zip(one, want):
        assert torch.equal(a, b[1])


def test_input_data_is_not_mutated():
    meta, mx, d, _ = _case("mesh_contact_f64")
    before = {k: getattr(d, k).clone() for k in LEAVES + ("qpos",)}
    mt.render(mx, d, width=16, height=8, shadows=True)
    for k, t in before.items():
        assert torch.equal(getattr(d, k), t), k


def test_value_edits_take_effect():
    meta, mx, d, _ = _case("render_scene_f64")
    kw = dict(width=meta["width"], height=meta["height"], shading=False)
    rgb0, depth0, seg0 = mt.render(mx, d, **kw)
    block = 2  # no material: its colour is geom_rgba
    rgba = mx.geom_rgba.clone()
    rgba[block, :3] = torch.tensor([0.25, 0.5, 0.75], dtype=rgba.dtype)
    rgb1, _, seg1 = mt.render(mx.replace(geom_rgba=rgba), d, **kw)
    on = seg0 == block
    assert on.any() and torch.equal(seg1, seg0)
    assert torch.equal(rgb1[on], torch.tensor([0.25, 0.5, 0.75], dtype=rgb1.dtype, device=DEV).expand(int(on.sum()), 3))
    assert torch.equal(rgb1[~on], rgb0[~on])
    size = mx.geom_size.clone()
    ball = 3
    size[ball, 0] = 0.35
    _, depth2, seg2 = mt.render(mx.replace(geom_size=size), d, **kw)
    assert (seg2 == ball).sum() > (seg0 == ball).sum()
    assert torch.equal(mt.render(mx, d, **kw)[1], depth0)  # the original model keeps its sizes


def test_uint8_path_equals_the_float_conversion():
    for case in ("render_scene_f64", "ray_scene_flat_f64", "ant_f32"):
        meta, mx, d, _ = _case(case)
        for bg in (None, (0.4, 0.6, 0.8)):
            rgb, _, _ = mt.render(mx, d, camera_id=meta["camera_id"], width=meta["width"], height=meta["height"], background=bg)
            u8 = R.render_uint8(mx, d, camera_id=meta["camera_id"], width=meta["width"], height=meta["height"], background=bg)
            assert u8.dtype == torch.uint8 and torch.equal(u8, (rgb * 255).clamp(0, 255).to(torch.uint8)), case


def test_batches_past_one_launch_are_cut_on_the_host():
    """MJH_MAX_GRID_LOG2=2 caps a launch at 4 workgroups (1024 pixels): 7 environments of 24 x 32 run in several launches, boundaries falling
    inside an image, bit-identical to one launch."""
    code = r'''
import sys, os, json
sys.path.insert(0, "tests"); sys.path.insert(0, "mujoco-torch_amd"); sys.path.insert(0, "oracle")
import numpy as np, torch, mujoco_torch_amd as mt
import test_render as T
res = {}
for case in ("render_scene_f64", "mesh_contact_f32", "humanoid_ssaa_f64"):
    meta, mx, d, _ = T._case(case)
    d = d[torch.arange(7) % meta["nenv"]].clone()
    res[case] = [t.cpu() for t in mt.render(mx, d, **T._kw(meta))]
torch.save(res, sys.argv[1])
print("ran")
'''
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as td:
        res = {}
        for tag, env in (("one", {}), ("cut", {"MJH_MAX_GRID_LOG2": "2"})):
            f = os.path.join(td, tag + ".pt")
            r = subprocess.run([sys.executable, "-c", code, f], cwd=root, env=dict(os.environ, **env), capture_output=True, text=True, timeout=900)
            assert r.returncode == 0 and "ran" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
            res[tag] = torch.load(f)
    for case in res["one"]:
        for a, b in zip(res["one"][case], res["cut"][case]):
            assert torch.equal(a, b), case


def test_zoo_pixels_step_with_auto_reset():
    env = ENVS["cartpole"](num_envs=6, device=DEV, from_pixels=True, auto_reset=True, max_episode_steps=3, render_width=20, render_height=12)
    td = env.reset()
    assert td["pixels"].shape == (6, 12, 20, 3) and td["pixels"].dtype == torch.uint8
    resets = 0
    for _ in range(5):  # past max_episode_steps: the environments auto-reset after their observation is taken
        action = torch.zeros(6, int(env.action_spec.shape[-1]), dtype=env.dtype, device=DEV)
        out = env.step(td.set("action", action))["next"]
        px, done = out["pixels"], out["done"].squeeze(-1)
        assert px.dtype == torch.uint8 and px.shape == (6, 12, 20, 3)
        rgb, _, _ = mt.render(env.mx, env._dx, width=20, height=12, background=env.RENDER_BACKGROUND)
        keep = ~done  # rows not reset since the observation: their pixels are the render of the resident state
        assert torch.equal(px[keep], (rgb * 255).clamp(0, 255).to(torch.uint8)[keep])
        resets += int(done.sum())
        td = out
    assert resets > 0
    img = env.render(width=16, height=10)
    assert img.shape == (10, 16, 3) and img.dtype == np.uint8
    assert np.array_equal(img, (mt.render(env.mx, env._dx[0:1], width=16, height=10, background=env.RENDER_BACKGROUND)[0][0] * 255)
                          .clamp(0, 255).to(torch.uint8).cpu().numpy())
