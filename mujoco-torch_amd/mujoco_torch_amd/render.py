"""``precompute_render_data`` / ``render`` / ``render_batch``: the ray-cast renderer (reference ``_src/render.py``).

``render(m, d, camera_id=0, width=64, height=64, precomp=None, shading=True, background=None, shadows=False, fog=None, ssaa=1)`` draws every
environment of a (batched) ``Data`` in one native launch sequence (``mjh_render``, ``csrc/mjh_render.h``): one lane per (environment, output
pixel).  Only ``cam_xpos`` / ``cam_xmat`` / ``light_xpos`` / ``light_xdir`` / ``geom_xpos`` / ``geom_xmat`` are read, so the caller runs
``forward`` / ``step`` first, as in the reference.  The result is ``(rgb, depth, seg)``.

The rules are the reference's (``render.py:179-861``): pixel rays through the camera (row 0 at the top), the nearest visible geom (the
primitives in type-major order, first minimum wins, then the meshes triangle by triangle, a mesh winning only when strictly closer), the
material's or the geom's colour, Lambert + Phong shading per light with attenuation, a ``cos^10`` spotlight cone and shadow rays against the
primitives, linear fog on hits, and super-sampling averaged per output pixel (``seg``: the centre sample).  Output dtypes follow the
reference: MuJoCo keeps colours in float32, so a float64 model's flat (unshaded, unfogged) image is float32.

Deviations: mesh normals keep the reference's radial approximation ``normalize(hit_local)``, not the face normal; textures are not
compiled, so a material that names one renders with its own rgba (a ``UserWarning``, once per model).

The scene tables (visible geoms in tie-break order, mesh triangles, materials, lights) are built from the model at ``device_put``; geom sizes
and ``geom_rgba`` are read from the device ``Model`` by every call.  ``torch.vmap`` / ``torch.compile`` go through the ``render_leaves`` operator.
"""

from __future__ import annotations

import ctypes
import math
import warnings

import numpy as np
import torch

from ._enums import GeomType
from ._postpass import cached, call, require_device

_LIGHT_ROW = 16  # reals per light row (include/mjhip.h mjhRenderScene)


# ---- host tables ------------------------------------------------------------------------------------------------------------

def host_tables(m) -> dict:
    """What the render tables are built from, taken from the compiled model at ``device_put`` (structure: materials, lights, cameras)."""
    ng, nl = int(m.ngeom), int(getattr(m, "nlight", 0) or 0)
    A = lambda n, default: np.asarray(getattr(m, n)) if getattr(m, n, None) is not None else default
    f32 = lambda n, shape, fill: A(n, np.full(shape, fill)).astype(np.float32).reshape(shape)
    return dict(
        geom_matid=A("geom_matid", -np.ones(ng, dtype=np.int32)).astype(np.int32).reshape(ng),
        mat_rgba=A("mat_rgba", np.ones((0, 4))).astype(np.float32).reshape(-1, 4),
        mat_has_texture=A("mat_has_texture", np.zeros(0, dtype=bool)).astype(bool).reshape(-1),
        cam_fovy=A("cam_fovy", np.zeros(0)).astype(np.float64).reshape(-1),
        light_type=A("light_type", np.zeros(nl, dtype=np.int32)).astype(np.int64).reshape(nl),
        light_castshadow=A("light_castshadow", np.ones(nl, dtype=bool)).astype(bool).reshape(nl),
        light_diffuse=f32("light_diffuse", (nl, 3), 0.7), light_ambient=f32("light_ambient", (nl, 3), 0.0),
        light_specular=f32("light_specular", (nl, 3), 0.3), light_attenuation=f32("light_attenuation", (nl, 3), 0.0),
        light_cutoff=f32("light_cutoff", (nl,), 45.0),
    )


def light_rows(t, dtype) -> torch.Tensor:
    """[nlight, 16] of the call's dtype: diffuse, ambient, specular, attenuation (float32 values), cos(cutoff) of a spotlight (render.py:567-576:
    the cosine in the call's dtype of cutoff * pi / 180; 2 when cutoff >= 180: no cone), directional, castshadow, unused."""
    nl = len(t["light_type"])
    rows = torch.zeros((nl, _LIGHT_ROW), dtype=dtype)
    for i in range(nl):
        for j, n in enumerate(("light_diffuse", "light_ambient", "light_specular", "light_attenuation")):
            rows[i, 3 * j : 3 * j + 3] = torch.tensor(t[n][i].astype(np.float64), dtype=dtype)
        cutoff = float(t["light_cutoff"][i])
        rows[i, 12] = torch.cos(torch.tensor(cutoff * (torch.pi / 180.0), dtype=dtype)) if cutoff < 180.0 else 2.0
        rows[i, 13] = 1.0 if int(t["light_type"][i]) == 1 else 0.0
        rows[i, 14] = 1.0 if bool(t["light_castshadow"][i]) else 0.0
    return rows


_DEV = {}  # (tables uid, dtype, device) -> device tables of one model structure
_WARNED = set()  # tables uids whose texture warning was issued


def _scene(m, dtype, device):
    """(candidate rows [ncand, 4] int32, primitive rows, triangles, geom_matid, mat_rgba, light rows) on the device."""
    from .ray import candidates

    def make():
        T = m.tables
        c = candidates(T.ray, (True, (), ()))  # the visible geoms, no filter: render.py:54-56, ray.py's tie-break order, meshes last
        rows = np.zeros((len(c["geom"]), 4), dtype=np.int32)
        rows[:, 0], rows[:, 1], rows[:, 2:] = c["geom"], c["type"], c["tri_range"]
        R = T.render
        nprim = int(np.sum(c["type"] != int(GeomType.MESH)))
        mat = R["mat_rgba"] if len(R["mat_rgba"]) else np.ones((1, 4), dtype=np.float32)
        return dict(cand=torch.tensor(rows, device=device), nprim=nprim, tri=torch.tensor(c["tri"], dtype=dtype, device=device).contiguous(),
                    matid=torch.tensor(R["geom_matid"], device=device), mat=torch.tensor(mat, device=device).contiguous(),
                    light=light_rows(R, dtype).to(device).contiguous())

    return cached(_DEV, (m.tables.uid, dtype, device), make)


def _texture_warning(m):
    T = m.tables
    if T.uid in _WARNED:
        return
    _WARNED.add(T.uid)
    R = T.render
    mid = R["geom_matid"][T.ray["geom_visible"]]
    tex = R["mat_has_texture"]
    if len(tex) and np.any(tex[mid[mid >= 0]]):
        warnings.warn("render: this model's materials name textures, which are not compiled: those geoms render with the material's rgba, "
                      "without texture modulation", UserWarning, stacklevel=3)


class RenderPrecomp:
    """``precompute_render_data``'s result: the model structure it was made for.  The scene tables themselves live with the model (built at
    ``device_put``, uploaded once per dtype and device), so this only lets callers keep the reference's ``precomp=`` idiom."""

    def __init__(self, struct_uid: str):
        self.struct_uid = struct_uid

    def __repr__(self):
        return f"RenderPrecomp({self.struct_uid})"


def precompute_render_data(m) -> RenderPrecomp:
    """The reference's per-model precomputation (render.py:33-114).  Here an opaque handle: pass it as ``precomp=`` or pass ``None``."""
    return RenderPrecomp(m._struct_uid)


# ---- argument checks --------------------------------------------------------------------------------------------------------

def _options(m, camera_id, width, height, shading, background, shadows, fog, ssaa) -> tuple:
    """The call's settings as a hashable tuple; raises ValueError on bad ones."""
    ncam = len(m.tables.render["cam_fovy"])
    for name, v in (("camera_id", camera_id), ("width", width), ("height", height), ("ssaa", ssaa)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{name} must be an int, got {v!r}")
    if not 0 <= int(camera_id) < ncam:
        raise ValueError(f"camera_id {camera_id} is out of range: the model has {ncam} camera(s)")
    for name, v in (("width", width), ("height", height), ("ssaa", ssaa)):
        if int(v) < 1:
            raise ValueError(f"{name} must be >= 1, got {v}")
    if int(width) * int(height) > (1 << 24) or int(ssaa) > 64:
        raise ValueError(f"image too large: {width} x {height}, ssaa {ssaa}")
    bg = () if background is None else tuple(float(x) for x in background)
    if len(bg) not in (0, 3):
        raise ValueError(f"background must be an RGB triple, got {background!r}")
    fg = ()
    if fog is not None:
        color, start, end = fog
        fg = tuple(float(x) for x in color) + (float(start), float(end))
        if len(fg) != 5:
            raise ValueError(f"fog must be ((r, g, b), start, end), got {fog!r}")
    return (int(camera_id), int(width), int(height), bool(shading), bg, bool(shadows), fg, int(ssaa))


def rgb_dtype(m, dtype, opts, u8=False):
    """The reference's rgb dtype: the model dtype when the image is shaded (shading and lights) or fogged, else float32 (MuJoCo's colours)."""
    if u8:
        return torch.uint8
    shaded = opts[3] and len(m.tables.render["light_type"]) > 0
    return dtype if (shaded or opts[6]) else torch.float32


def check_args(m, leaves):
    """Dtype / device / shape validation shared by the direct call and the operator; returns the Data's batch shape."""
    xpos, xmat, cxpos, cxmat, lxpos, lxdir = leaves
    for name, t in (("cam_xpos", cxpos), ("cam_xmat", cxmat), ("light_xpos", lxpos), ("light_xdir", lxdir), ("geom_xmat", xmat)):
        if t.dtype != xpos.dtype:
            raise ValueError(f"{name} is {t.dtype}, geom_xpos is {xpos.dtype}")
        if t.device != xpos.device:
            raise ValueError(f"{name} is on {t.device}, geom_xpos is on {xpos.device}")
    if xpos.dim() < 2 or xpos.shape[-1] != 3 or tuple(xmat.shape[:-2]) != tuple(xpos.shape[:-1]) or xmat.shape[-2:] != (3, 3):
        raise ValueError(f"geom_xpos / geom_xmat have shapes {tuple(xpos.shape)} / {tuple(xmat.shape)}")
    batch = tuple(xpos.shape[:-2])
    ncam, nl, ng = len(m.tables.render["cam_fovy"]), len(m.tables.render["light_type"]), int(m.ngeom)
    if xpos.shape[-2] != ng:
        raise ValueError(f"the Data holds {xpos.shape[-2]} geoms, the Model {ng}")
    for name, t, want in (("cam_xpos", cxpos, (ncam, 3)), ("cam_xmat", cxmat, (ncam, 3, 3)), ("light_xpos", lxpos, (nl, 3)), ("light_xdir", lxdir, (nl, 3))):
        if tuple(t.shape) != batch + want:
            raise ValueError(f"{name} has shape {tuple(t.shape)}, expected {batch + want}")
    return batch


# ---- the native call --------------------------------------------------------------------------------------------------------

def render_native(m, leaves, opts, u8=False):
    """One ``mjh_render`` call on plain tensors (the direct path and the eager body of ``render_leaves``)."""
    from . import native

    batch = check_args(m, leaves)
    xpos = leaves[0]
    require_device(xpos.device)
    dtype, device = xpos.dtype, xpos.device
    if dtype not in (torch.float64, torch.float32):
        raise RuntimeError(f"unsupported Data dtype {dtype}")
    cam, W, H, shading, bg, shadows, fg, ssaa = opts
    B = int(math.prod(batch)) if batch else 1
    rdt = rgb_dtype(m, dtype, opts, u8)
    rgb = torch.empty(batch + (H, W, 3), dtype=rdt, device=device)
    depth = torch.empty(batch + (H, W), dtype=dtype, device=device)
    seg = torch.empty(batch + (H, W), dtype=torch.int64, device=device)
    if B == 0:
        return rgb, depth, seg
    _texture_warning(m)
    sc = _scene(m, dtype, device)
    size, rgba = m.geom_size, m.geom_rgba
    size = size.to(device=device, dtype=dtype).contiguous()
    rgba = rgba.to(device=device, dtype=dtype).contiguous()
    nl = len(m.tables.render["light_type"])
    flat = [t.reshape((B,) + tuple(t.shape[len(batch):])).contiguous() for t in leaves]
    ptr = lambda t: ctypes.c_void_p(t.data_ptr() if t.numel() else None)
    scene = native.RenderScene(sc["cand"].shape[0], sc["nprim"], ptr(sc["cand"]), ptr(sc["tri"]), ptr(size), ptr(rgba), ptr(sc["matid"]),
                               ptr(sc["mat"]), nl, ptr(sc["light"]))
    # render.py:196-198 half angles, in the call's dtype (the aspect ratio of the super-sampled image is the same float)
    half_h = torch.tan(torch.tensor(float(m.tables.render["cam_fovy"][cam]) * (torch.pi / 360.0), dtype=dtype))
    half_w = half_h * (W / H)
    pre_fog = rgb_dtype(m, dtype, opts[:6] + ((),) + opts[7:])  # the rgb dtype the fog colour is made in (render.py:706)
    bgv = torch.tensor(bg if bg else (0.0, 0.0, 0.0), dtype=torch.float32).double().tolist()  # render.py:800-804: the base colour's dtype
    fc = torch.tensor(fg[:3] if fg else (0.0, 0.0, 0.0), dtype=pre_fog).double().tolist()
    params = native.RenderParams(camera=cam, width=W, height=H, ssaa=ssaa, shading=int(shading), shadows=int(shadows), fog=int(bool(fg)),
                                 rgb_f32=int(rgb_dtype(m, dtype, opts) == torch.float32), u8=int(u8), half_w=float(half_w), half_h=float(half_h),
                                 background=(ctypes.c_double * 3)(*bgv), fog_color=(ctypes.c_double * 3)(*fc),
                                 fog_start=fg[3] if fg else 0.0, fog_range=(fg[4] - fg[3]) if fg else 1.0)
    call("render", m, "mjh_render", tuple(ptr(t) for t in flat) + (B, ctypes.byref(scene), ctypes.byref(params), ptr(rgb), ptr(depth), ptr(seg)), device, dtype,
         what="rendering")
    return rgb, depth, seg


def _leaves(d):
    return (d.geom_xpos, d.geom_xmat, d.cam_xpos, d.cam_xmat, d.light_xpos, d.light_xdir)


def _render(m, d, opts, u8=False):
    from .forward import _plain

    leaves = _leaves(d)
    if torch.compiler.is_compiling() or not all(_plain(t) for t in leaves):
        from . import compile_op  # noqa: F401  (registers the operator)

        cam, W, H, shading, bg, shadows, fg, ssaa = opts
        return torch.ops.mujoco_torch_amd.render_leaves(*leaves, m._op_key_t, m._struct_uid, cam, W, H, shading, list(bg), shadows, list(fg), ssaa, u8)
    return render_native(m, leaves, opts, u8)


def _check_precomp(m, precomp):
    if precomp is not None and not (isinstance(precomp, RenderPrecomp) and precomp.struct_uid == m._struct_uid):
        raise ValueError("precomp must be None or precompute_render_data() of a Model of this structure")


def render(m, d, camera_id: int = 0, width: int = 64, height: int = 64, precomp=None, shading: bool = True,
           background: tuple[float, float, float] | None = None, shadows: bool = False,
           fog: tuple[tuple[float, float, float], float, float] | None = None, ssaa: int = 1) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Ray-cast render (reference render.py:719-861): ``(rgb, depth, seg)``.

    ``d``: a Data after ``forward`` / ``step``, with or without batch dimensions ``S``.  ``rgb``: ``S + (height, width, 3)`` in [0, 1] (the model
    dtype when shaded or fogged, else float32, as the reference); ``depth``: ``S + (height, width)``, the model dtype, ``-1`` for a miss;
    ``seg``: ``S + (height, width)`` int64 geom ids, ``-1`` for a miss.  ``precomp``: ``None`` or ``precompute_render_data(m)``.
    ``background``: the RGB of a miss (black by default); ``fog``: ``((r, g, b), start, end)``; ``ssaa``: super-sampling factor."""
    _check_precomp(m, precomp)
    opts = _options(m, camera_id, width, height, shading, background, shadows, fog, ssaa)
    return _render(m, d, opts)


def render_batch(m, d_batch, camera_id: int = 0, width: int = 64, height: int = 64, precomp=None, shading: bool = True,
                 background: tuple[float, float, float] | None = None, shadows: bool = False,
                 fog: tuple[tuple[float, float, float], float, float] | None = None, ssaa: int = 1) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``render`` of a batched Data (reference render.py:864-907): outputs ``(B, H, W, 3)`` / ``(B, H, W)`` / ``(B, H, W)``, one launch sequence."""
    if d_batch.geom_xpos.dim() < 3:
        raise ValueError("render_batch takes a Data with a leading batch dimension; use render for one environment")
    return render(m, d_batch, camera_id, width, height, precomp, shading, background, shadows, fog, ssaa)


def render_uint8(m, d, camera_id=0, width=64, height=64, background=None):
    """The zoo's pixels: ``(rgb * 255).clamp(0, 255).to(torch.uint8)`` of ``render``'s rgb, written by the kernel directly."""
    opts = _options(m, camera_id, width, height, True, background, False, None, 1)
    return _render(m, d, opts, u8=True)[0]
