"""``mt.render`` on the GPU where its goldens do not reach: tiny images, whose workgroups span many environments and whose candidate frames no
longer stay resident in LDS (the kernel then re-stages them chunk by chunk for the primary ray and for every shadow ray), against the large
resident render of the same samples bit for bit; a row of a batch against the single environment bit for bit; ``depth`` / ``seg`` against the
high-precision reference of tests/_ray_ref.py on the renderer's own pixel rays; and the uint8 path on thumbnails.

``run_render``'s rule (csrc/mjhip.hip): a workgroup's 256 pixels touch at most ``span`` environments, 2 for an image of 256 pixels or more, else
``min(255 // P + 2, 256)``; ``chunk = 48 KB // (span * 12 * sizeof(real))`` candidates are staged at a time, and the frames stay resident when
``chunk >= ncand``.  The frames, cameras and lights are those recorded in tests/golden/render/, tiled to B environments with the geoms of every
environment shifted by their own offset (tests/_ray_cases.py).  No tolerance is chosen here: every check is ``torch.equal`` or the reference's
own propagated bound (tests/test_ray_ref_host.py holds the share of pixels the reference leaves out to 2 % without a GPU)."""
import importlib

import numpy as np
import pytest
import torch

import mujoco_torch_amd as mt
import _ray_cases as rc
import _ray_ref as rr

pytestmark = pytest.mark.gpu

R = importlib.import_module("mujoco_torch_amd.render")
DEV = "cuda"
FOG = ((0.3, 0.3, 0.3), 1.0, 4.0)


def _scene(case, B):
    meta, _ = rc.render_golden(case)
    mx = rc.render_model(case).to(DEV)
    fr = rc.render_frames(case, B)
    d = mt.make_data(mx).expand(B).clone().to(DEV)
    return meta, mx, d.replace(**{k: torch.tensor(v, device=DEV) for k, v in fr.items()})


def _launch(mx, W, H):
    """(span, chunk, resident) of render(width=W, height=H) by run_render's documented rule and the model's candidate count."""
    ncand = len(rc.visible_candidates(mx, np.float64))
    P = W * H
    span = 2 if P >= 256 else min(255 // P + 2, 256)
    chunk = (48 * 1024) // (span * 12 * torch.empty(0, dtype=mx.geom_size.dtype).element_size())
    return span, chunk, chunk >= ncand


# (golden, settings, (W, H, S), (span, chunk, resident) of the small launch)
CHUNKED = [
    ("humanoid_shadows_f64", dict(shadows=True), (4, 2, 8), (33, 15, False)),         # 20 candidates in chunks of 15
    ("render_scene_f64", dict(shadows=True, fog=FOG), (2, 1, 16), (129, 3, False)),
    ("mesh_contact_f64", dict(shadows=True), (2, 1, 16), (129, 3, True)),             # its 3 candidates fit a chunk of 3: 129 slots, resident
    ("mesh_contact_f64", dict(shadows=True), (1, 1, 16), (256, 2, False)),            # ... chunked at the cap: shadow passes over nprim = 2 < ncand = 3
    ("render_scene_f32", dict(shadows=True), (1, 1, 32), (256, 4, False)),            # span at its cap
    ("render_scene_f64", dict(shadows=True, fog=FOG), (5, 3, 3), (19, 26, True)),     # resident on both sides: the decomposition itself
]


@pytest.mark.parametrize("case,kw,size,launch", CHUNKED, ids=[f"{c[0]}-{c[2][0]}x{c[2][1]}s{c[2][2]}" for c in CHUNKED])
def test_chunked_render_equals_the_resident_one(case, kw, size, launch):
    """render(W, H, ssaa=S) computes the sample directions of render(W S, H S) by the same operations and adds its S x S samples in (sy, sx) order
    into an accumulator of the output dtype, dividing once: it equals that sum of the large image formed on the host, bit for bit."""
    W, H, S = size
    B = 40
    meta, mx, d = _scene(case, B)
    cam = meta["camera_id"]
    assert _launch(mx, W, H) == launch, _launch(mx, W, H)  # the small launch is the chunked one (but for the two resident controls)
    assert _launch(mx, W * S, H * S)[2]  # ... and the large one keeps its frames resident
    rgb, depth, seg = (t.cpu() for t in mt.render(mx, d, camera_id=cam, width=W, height=H, ssaa=S, **kw))
    big_rgb, big_depth, big_seg = (t.cpu() for t in mt.render(mx, d, camera_id=cam, width=W * S, height=H * S, ssaa=1, **kw))
    assert (big_seg >= 0).any()
    assert torch.equal(seg, big_seg[:, S // 2::S, S // 2::S]), f"{case}: seg differs on {int((seg != big_seg[:, S // 2::S, S // 2::S]).sum())} pixels"
    for name, small, big in (("depth", depth, big_depth), ("rgb", rgb, big_rgb)):
        if name == "rgb" and rgb.dtype != depth.dtype:
            continue  # the float32 rgb of a flat float64 render cannot be re-summed
        acc = torch.zeros_like(small)
        for sy in range(S):
            for sx in range(S):
                acc = acc + big[:, sy::S, sx::S]
        want = acc / float(S * S)
        assert torch.equal(small, want), f"{case} {name}: {int((small != want).sum())} of {small.numel()} values differ, worst {float((small - want).abs().max()):.3g}"
    assert rgb.dtype == depth.dtype  # every case here is shaded: rgb went through the comparison


@pytest.mark.parametrize("size", [(1, 1), (2, 1), (15, 17), (16, 16), (257, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("case", ["render_scene_f64", "render_scene_f32"])
def test_a_batch_row_equals_the_single_environment(case, size):
    """A workgroup of the batch serves up to 256 environment slots (1 x 1), 128 (2 x 1) or 2; the single call runs slot 0 alone."""
    W, H = size
    B = 70
    meta, mx, d = _scene(case, B)
    kw = dict(camera_id=meta["camera_id"], width=W, height=H, shadows=True)
    batch = mt.render(mx, d, **kw)
    assert (batch[2] >= 0).any()
    distinct = {tuple(batch[1][i].reshape(-1).tolist()) for i in range(B)}
    assert len(distinct) > B // 2  # the environments are not alike: a wrong slot shows
    for i in range(B):
        one = mt.render(mx, d[i:i + 1], **kw)
        for name, a, b in zip(("rgb", "depth", "seg"), one, batch):
            assert a.dtype == b.dtype and torch.equal(a[0], b[i]), f"{case} {W} x {H}: {name} of environment {i} differs"


@pytest.mark.parametrize("size", rc.RENDER_REF_SIZES, ids=lambda s: f"{s[0]}x{s[1]}s{s[2]}")
@pytest.mark.parametrize("case", rc.RENDER_REF_CASES)
def test_depth_and_seg_lie_inside_the_reference_bound(case, size):
    W, H, S = size
    ref = rc.render_ref_case(case, W, H, S)
    meta, mx, d = _scene(case, ref["decided"].shape[0])
    _, depth, seg = mt.render(mx, d, camera_id=meta["camera_id"], width=W, height=H, ssaa=S)
    depth, seg = depth.cpu().numpy(), seg.cpu().numpy()
    what = f"{case} {W} x {H} ssaa {S}"
    dec = ref["decided"]
    err = np.abs(depth.astype(rr.HP) - ref["depth"])
    ratio = float((err / np.maximum(ref["err"], rr.HP(1e-300)))[dec & (ref["err"] > 0)].max(initial=0))
    print(f"{what}: worst error / bound {ratio:.3f} over {int(dec.sum())} pixels ({int((dec & (ref['seg0'] >= 0)).sum())} hit at their centre), "
          f"{int((~dec).sum())} left out; largest bound {float(ref['err'].max()):.3g}")
    over = dec & (err > ref["err"])  # a pixel all of whose samples miss has depth -1 and bound 0
    assert not over.any(), f"{what}: {int(over.sum())} depths beyond their bound (worst ratio {ratio:.3g})"
    wrong = dec & (seg != ref["seg0"]) & (seg != ref["seg1"])
    assert not wrong.any(), f"{what}: seg differs on {int(wrong.sum())} pixels without a tie"


@pytest.mark.parametrize("size", [(2, 1), (15, 17)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_thumbnail_uint8_equals_the_float_conversion(size):
    W, H = size
    for case in ("render_scene_f64", "ray_scene_flat_f64", "ant_f32"):
        meta, mx, d = _scene(case, 40)
        for bg in (None, (0.4, 0.6, 0.8)):
            rgb, _, _ = mt.render(mx, d, camera_id=meta["camera_id"], width=W, height=H, background=bg)
            u8 = R.render_uint8(mx, d, camera_id=meta["camera_id"], width=W, height=H, background=bg)
            assert u8.dtype == torch.uint8 and u8.shape == (40, H, W, 3)
            assert torch.equal(u8, (rgb * 255).clamp(0, 255).to(torch.uint8)), (case, bg)
