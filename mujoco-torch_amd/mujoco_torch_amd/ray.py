"""``ray`` / ``ray_geom``: ray casting against a model's geoms (reference ``_src/ray.py:375-465``).

``ray(m, d, pnt, vec, geomgroup=(), flg_static=True, bodyexclude=-1) -> (dist, geomid)`` casts rays in every environment of a
batched ``Data`` in one native launch (``mjh_ray``, ``csrc/mjh_ray.h``): one lane per (environment, ray) pair.  Only ``d.geom_xpos`` /
``d.geom_xmat`` are read, so the caller runs ``forward`` / ``step`` first, as in the reference.

The geoms a call tests (its *candidates*) follow the reference's filters (``ray.py:400-415``): ``flg_static`` / ``bodyexclude`` /
``geomgroup`` and the alpha of ``geom_rgba``.  They are listed in its tie-break order -- type-major (plane, sphere, capsule, ellipsoid,
cylinder, box, mesh), ascending geom id within a type -- and the first minimum wins, as ``torch.argmin`` does.  The candidate table is
built on the host once per (model structure, dtype, device, filters); geom sizes are read from the device ``m.geom_size`` by every call.
Meshes are tested triangle by triangle (``_ray_mesh`` / ``_ray_triangle``) on the raw ``mesh_face`` / ``mesh_vert``.

Deviations from the reference: the result is always ``(dist, geomid)`` (the reference's no-candidate early return swaps the
two), and every mesh geom is alpha-filtered on its own like the primitives.

``ray_geom(size, pnt, vec, geomtype)`` is the reference's single-primitive distance in plain torch, on any device.
"""

from __future__ import annotations

import ctypes
import math
from collections.abc import Sequence

import numpy as np
import torch

from ._enums import GeomType
from ._postpass import cached, call, require_device

_MINVAL = 1e-15  # mujoco.mjMINVAL
_NGROUP = 6  # mujoco.mjNGROUP
# the reference's _RAY_FUNC order (ray.py:282-290): the tie-break order of the candidates
RAY_GEOM_ORDER = (GeomType.PLANE, GeomType.SPHERE, GeomType.CAPSULE, GeomType.ELLIPSOID, GeomType.CYLINDER, GeomType.BOX, GeomType.MESH)


# ---- host tables ------------------------------------------------------------------------------------------------------------

def host_tables(m) -> dict:
    """What the candidate tables are built from, taken from the compiled model at ``device_put`` (structure, not values: ``geom_rgba``'s alpha
    and the meshes are fixed there; geom sizes are read per call)."""
    ng = int(m.ngeom)
    A = lambda n, default: np.asarray(getattr(m, n)) if getattr(m, n, None) is not None else default
    rgba = A("geom_rgba", np.ones((ng, 4))).reshape(ng, 4)
    matid = A("geom_matid", -np.ones(ng, dtype=np.int32)).reshape(ng)
    mat_rgba = A("mat_rgba", np.ones((0, 4))).reshape(-1, 4)
    visible = (matid != -1) | (rgba[:, 3] != 0)  # ray.py:417-418
    if len(mat_rgba):
        visible &= (matid == -1) | (mat_rgba[np.clip(matid, 0, len(mat_rgba) - 1), 3] != 0)
    gbody = A("geom_bodyid", np.zeros(ng, dtype=np.int32)).astype(np.int64)
    nmesh = int(getattr(m, "nmesh", 0) or 0)
    return dict(
        geom_type=A("geom_type", np.zeros(ng, dtype=np.int32)).astype(np.int64),
        geom_bodyid=gbody,
        geom_static=A("body_weldid", np.zeros(int(m.nbody), dtype=np.int32)).astype(np.int64)[gbody] == 0,
        geom_group=A("geom_group", np.zeros(ng, dtype=np.int32)).astype(np.int64),
        geom_visible=visible,
        geom_dataid=A("geom_dataid", -np.ones(ng, dtype=np.int32)).astype(np.int64),
        mesh_vert=A("mesh_vert", np.zeros((0, 3))).reshape(-1, 3).astype(np.float32).astype(np.float64),  # MuJoCo keeps mesh_vert in float32
        mesh_face=A("mesh_face", np.zeros((0, 3), dtype=np.int32)).reshape(-1, 3).astype(np.int64),
        mesh_vertadr=A("mesh_vertadr", np.zeros(nmesh, dtype=np.int32)).astype(np.int64),
        mesh_faceadr=A("mesh_faceadr", np.zeros(nmesh, dtype=np.int32)).astype(np.int64),
        mesh_facenum=A("mesh_facenum", np.zeros(nmesh, dtype=np.int32)).astype(np.int64),
    )


def filter_key(tables, geomgroup, flg_static, bodyexclude) -> tuple:
    """The call's filters as a hashable key; raises ValueError on a malformed group mask or a geom group outside 0..5 when one is given."""
    if isinstance(bodyexclude, (int, np.integer)) or (isinstance(bodyexclude, torch.Tensor) and bodyexclude.dim() == 0):
        bodyexclude = [bodyexclude]
    if not isinstance(bodyexclude, (Sequence, np.ndarray, torch.Tensor)):
        raise ValueError(f"bodyexclude must be an int or a sequence of ints, got {type(bodyexclude).__name__}")
    be = tuple(sorted({int(b) for b in bodyexclude}))
    gg = tuple(bool(g) for g in geomgroup)
    if gg:
        if len(gg) != _NGROUP:
            raise ValueError(f"geomgroup must have {_NGROUP} entries (one per geom group), got {len(gg)}")
        grp = tables["geom_group"]
        if len(grp) and (grp.min() < 0 or grp.max() >= _NGROUP):
            raise ValueError(f"geom groups must lie in 0..{_NGROUP - 1} to be filtered by geomgroup (this model has {sorted(set(grp.tolist()))})")
    return (bool(flg_static), be, gg)


def candidates(tables, key) -> dict:
    """The candidate table of one filter key (host arrays): ``geom`` ids in tie-break order, their ``type``, the ``[tri_begin, tri_end)``
    range of every mesh candidate into ``tri`` ([ntri, 9] float64, vertices in the geom frame; meshes shared by several geoms appear once)."""
    cache = tables.setdefault("_cand", {})
    hit = cache.get(key)
    if hit is not None:
        return hit
    flg_static, be, gg = key
    gtype = tables["geom_type"]
    keep = tables["geom_visible"].copy()
    if not flg_static:
        keep &= ~tables["geom_static"]
    for b in be:
        keep &= tables["geom_bodyid"] != b
    if gg:
        keep &= np.array(gg, dtype=bool)[tables["geom_group"]]
    ids, types, rng, tris, mesh_rng = [], [], [], [], {}
    ntri = 0
    for gt in RAY_GEOM_ORDER:
        for g in np.nonzero(keep & (gtype == int(gt)))[0]:
            ids.append(int(g))
            types.append(int(gt))
            if gt != GeomType.MESH:
                rng.append((0, 0))
                continue
            mid = int(tables["geom_dataid"][g])
            if mid not in mesh_rng:
                fa, fn, va = tables["mesh_faceadr"][mid], tables["mesh_facenum"][mid], tables["mesh_vertadr"][mid]
                face = tables["mesh_face"][fa : fa + fn] + va
                tris.append(tables["mesh_vert"][face].reshape(-1, 9))
                mesh_rng[mid] = (ntri, ntri + int(fn))
                ntri += int(fn)
            rng.append(mesh_rng[mid])
    hit = dict(geom=np.array(ids, dtype=np.int64), type=np.array(types, dtype=np.int64),
               tri_range=np.array(rng, dtype=np.int64).reshape(-1, 2),
               tri=np.concatenate(tris) if tris else np.zeros((0, 9)))
    if len(cache) > 64:
        cache.clear()
    cache[key] = hit
    return hit


_DEV = {}  # (tables uid, filter key, dtype, device) -> (candidate rows [ncand, 4] int32, triangles [ntri, 9]) on the device


def _device_candidates(m, key, dtype, device):
    def make():
        c = candidates(m.tables.ray, key)
        rows = np.zeros((len(c["geom"]), 4), dtype=np.int32)
        rows[:, 0], rows[:, 1], rows[:, 2:] = c["geom"], c["type"], c["tri_range"]
        return (torch.tensor(rows, device=device), torch.tensor(c["tri"], dtype=dtype, device=device).contiguous())

    return cached(_DEV, (m.tables.uid, key, dtype, device), make)


# ---- shapes -----------------------------------------------------------------------------------------------------------------

def ray_shapes(batch: tuple, pnt_shape: tuple, vec_shape: tuple):
    """(output shape, rays per environment R, per-argument (environment-wise?, rays)) for Data batch shape ``batch``.  ``pnt`` / ``vec``:
    (3,) shared, batch + (3,) one ray per environment, or batch + (R, 3) R rays per environment; the two broadcast against each other."""
    k = len(batch)
    modes = []
    for name, s in (("pnt", tuple(pnt_shape)), ("vec", tuple(vec_shape))):
        if len(s) == 1 and s == (3,):
            modes.append((False, None))
        elif len(s) == k + 1 and s[:k] == batch and s[-1] == 3:
            modes.append((True, None))
        elif len(s) == k + 2 and s[:k] == batch and s[-1] == 3:
            modes.append((True, s[k]))
        else:
            raise ValueError(f"{name} must have shape (3,), {batch + (3,)} or {batch + ('R', 3)} for a Data of batch shape {batch}; got {s}")
    rays = [r for _, r in modes if r is not None]
    if len(rays) == 2 and rays[0] != rays[1] and 1 not in rays:
        raise ValueError(f"pnt and vec do not broadcast: {rays[0]} against {rays[1]} rays per environment")
    R = max(rays) if rays else 1
    return batch + ((R,) if rays else ()), R, modes


def _flat(t, mode, B, R):
    """(contiguous tensor, environment stride, ray stride) in elements for the kernel's pnt / vec addressing."""
    env, rays = mode
    if not env:
        return t.contiguous(), 0, 0
    if rays is None:
        return t.reshape(B, 3).contiguous(), 3, 0
    return t.reshape(B, rays, 3).contiguous(), 3 * rays, 3 if rays > 1 else 0


def check_args(xpos, xmat, pnt, vec):
    """Dtype / device / shape validation shared by the direct call and the operator; returns ``ray_shapes``' result."""
    for name, t in (("pnt", pnt), ("vec", vec)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a tensor")
        if t.dtype != xpos.dtype:
            raise ValueError(f"{name} is {t.dtype}, the Data is {xpos.dtype}: pass rays in the Data dtype")
        if t.device != xpos.device:
            raise ValueError(f"{name} is on {t.device}, the Data is on {xpos.device}")
    if xpos.dim() < 2 or xpos.shape[-1] != 3 or tuple(xmat.shape[:-2]) != tuple(xpos.shape[:-1]) or xmat.shape[-2:] != (3, 3):
        raise ValueError(f"geom_xpos / geom_xmat have shapes {tuple(xpos.shape)} / {tuple(xmat.shape)}")
    return ray_shapes(tuple(xpos.shape[:-2]), tuple(pnt.shape), tuple(vec.shape))


# ---- the native call --------------------------------------------------------------------------------------------------------

def ray_native(m, xpos, xmat, pnt, vec, key):
    """One ``mjh_ray`` call on plain tensors (the direct path and the eager body of ``ray_leaves``)."""
    from . import native

    out_shape, R, modes = check_args(xpos, xmat, pnt, vec)
    key = filter_key(m.tables.ray, key[2], key[0], key[1])
    require_device(xpos.device)
    dtype, device = xpos.dtype, xpos.device
    if dtype not in (torch.float64, torch.float32):
        raise RuntimeError(f"unsupported Data dtype {dtype}")
    batch = tuple(xpos.shape[:-2])
    B = int(math.prod(batch)) if batch else 1
    ng = int(m.ngeom)
    if xpos.shape[-2] != ng:
        raise ValueError(f"the Data holds {xpos.shape[-2]} geoms, the Model {ng}")
    dist = torch.empty(out_shape, dtype=dtype, device=device)
    geomid = torch.empty(out_shape, dtype=torch.int64, device=device)
    if B * R == 0:
        return dist, geomid
    cand, tri = _device_candidates(m, key, dtype, device)
    size = m.geom_size
    if size.dtype != dtype or size.device != device:
        size = size.to(device=device, dtype=dtype)
    size = size.contiguous()
    xpos_c, xmat_c = xpos.reshape(B, ng, 3).contiguous(), xmat.reshape(B, ng, 9).contiguous()
    p, pe, pr = _flat(pnt, modes[0], B, R)
    v, ve, vr = _flat(vec, modes[1], B, R)
    cands = native.RayCands(cand.shape[0], ctypes.c_void_p(cand.data_ptr()), ctypes.c_void_p(tri.data_ptr() if tri.numel() else None),
                            ctypes.c_void_p(size.data_ptr()))
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    call("ray", m, "mjh_ray", (ptr(xpos_c), ptr(xmat_c), ptr(p), pe, pr, ptr(v), ve, vr, B, R, ctypes.byref(cands), ptr(dist), ptr(geomid)), device, dtype,
         what="ray casting")
    return dist, geomid


def ray(m, d, pnt: torch.Tensor, vec: torch.Tensor, geomgroup: Sequence[int] = (), flg_static: bool = True,
        bodyexclude: Sequence[int] | int = -1) -> tuple[torch.Tensor, torch.Tensor]:
    """Nearest geom hit by each ray (reference ray.py:375-452): ``(dist, geomid)``, ``-1.0`` / ``-1`` for a miss.

    ``d``: a (batched) Data after ``forward`` / ``step``; only ``geom_xpos`` / ``geom_xmat`` are read.  ``pnt`` / ``vec`` (the Data's dtype and
    device): ``(3,)`` one ray for every environment, ``S + (3,)`` one per environment, ``S + (R, 3)`` R per environment (S: the Data's batch
    shape); they broadcast against each other.  ``vec`` is not normalised: ``dist`` is the ray parameter.  ``dist`` has the Data dtype,
    ``geomid`` is int64, both of shape ``S`` or ``S + (R,)``.  ``geomgroup``: empty, or a 6-entry inclusion mask indexed by ``geom_group``;
    ``flg_static=False`` skips geoms of bodies welded to the world; ``bodyexclude``: a body id or a sequence of them.
    ``torch.vmap`` / ``torch.compile`` go through the ``ray_leaves`` operator."""
    from .forward import _plain

    xpos, xmat = d.geom_xpos, d.geom_xmat
    if isinstance(bodyexclude, (int, np.integer)):
        be = [int(bodyexclude)]
    else:
        be = [int(b) for b in bodyexclude]
    gg = [1 if g else 0 for g in geomgroup]
    if torch.compiler.is_compiling() or not (_plain(xpos) and _plain(pnt) and _plain(vec)):
        from . import compile_op  # noqa: F401  (registers the operator)

        return torch.ops.mujoco_torch_amd.ray_leaves(xpos, xmat, pnt, vec, m._op_key_t, m._struct_uid, gg, bool(flg_static), be)
    return ray_native(m, xpos, xmat, pnt, vec, (bool(flg_static), be, gg))


# ---- ray_geom: the reference's single-primitive distance, plain torch ---------------------------------------------------------

def _safe_div(num, den):
    return num / (den + _MINVAL * (den == 0))


def _dot(a, b):
    return (a * b).sum(-1)


def _quad(a, b, c):  # ray.py:28-40
    det = b * b - a * c
    det2 = torch.sqrt(det)
    x0, x1 = _safe_div(-b - det2, a), _safe_div(-b + det2, a)
    inf = torch.full_like(x0, math.inf)
    x0 = torch.where((det < _MINVAL) | (x0 < 0), inf, x0)
    x1 = torch.where((det < _MINVAL) | (x1 < 0), inf, x1)
    return x0, x1


def _first(x0, x1):
    return torch.where(torch.isinf(x0), x1, x0)


def _ray_geom(size, p, v, geomtype):
    inf = torch.full(p.shape[:-1], math.inf, dtype=p.dtype, device=p.device)
    s0 = size[..., 0]
    if geomtype == GeomType.PLANE:  # :43-57
        x = -_safe_div(p[..., 2], v[..., 2])
        valid = (v[..., 2] <= -_MINVAL) & (x >= 0)
        q = p[..., 0:2] + x[..., None] * v[..., 0:2]
        valid = valid & torch.all((size[..., 0:2] <= 0) | (torch.abs(q) <= size[..., 0:2]), -1)
        return torch.where(valid, x, inf)
    if geomtype == GeomType.SPHERE:  # :60-69
        return _first(*_quad(_dot(v, v), _dot(v, p), _dot(p, p) - s0 * s0))
    if geomtype == GeomType.ELLIPSOID:  # :109-129
        s = _safe_div(1, size[..., 0:3] * size[..., 0:3])
        sv = s * v
        return _first(*_quad(_dot(sv, v), _dot(sv, p), _dot(s * p, p) - 1))
    if geomtype in (GeomType.CAPSULE, GeomType.CYLINDER):  # :72-106, :235-268
        s1 = size[..., 1]
        x = _first(*_quad(_dot(v[..., 0:2], v[..., 0:2]), _dot(v[..., 0:2], p[..., 0:2]), _dot(p[..., 0:2], p[..., 0:2]) - s0 * s0))
        x = torch.where(torch.abs(p[..., 2] + x * v[..., 2]) <= s1, x, inf)
        for sign in (1, -1):
            if geomtype == GeomType.CAPSULE:
                dif = torch.stack([p[..., 0], p[..., 1], p[..., 2] - sign * s1], -1)
                x0, x1 = _quad(_dot(v, v), _dot(v, dif), _dot(dif, dif) - s0 * s0)
                for xi in (x0, x1):
                    z = p[..., 2] + xi * v[..., 2]
                    x = torch.where(((z >= s1) if sign > 0 else (z <= -s1)) & (xi < x), xi, x)
            else:
                t = _safe_div(sign * s1 - p[..., 2], v[..., 2])
                q = p[..., 0:2] + t[..., None] * v[..., 0:2]
                x = torch.where((t >= 0) & (_dot(q, q) <= s0 * s0) & (t < x), t, x)
        return x
    if geomtype == GeomType.BOX:  # :132-161
        sz = size[..., 0:3]
        x = torch.cat([_safe_div(sz - p, v), -_safe_div(sz + p, v)], -1)
        iface = torch.tensor([[1, 2], [0, 2], [0, 1], [1, 2], [0, 2], [0, 1]], device=p.device)
        p0 = p[..., iface[:, 0]] + x * v[..., iface[:, 0]]
        p1 = p[..., iface[:, 1]] + x * v[..., iface[:, 1]]
        valid = (torch.abs(p0) <= sz[..., iface[:, 0]]) & (torch.abs(p1) <= sz[..., iface[:, 1]]) & (x >= 0)
        return torch.where(valid, x, torch.full_like(x, math.inf)).min(-1).values
    raise ValueError(f"ray_geom takes a primitive geom type (plane, sphere, capsule, ellipsoid, cylinder, box), got {geomtype!r}")


def ray_geom(size: torch.Tensor, pnt: torch.Tensor, vec: torch.Tensor, geomtype) -> torch.Tensor:
    """Distance along ``vec`` from ``pnt`` to a primitive geom of ``size`` at the origin of its own frame (reference ray.py:455-465); ``inf``
    for a miss.  Elementwise over leading batch dimensions (broadcast), plain torch on any device."""
    geomtype = GeomType(int(geomtype))
    dtype = torch.promote_types(pnt.dtype, vec.dtype)
    size = torch.as_tensor(size, dtype=dtype, device=pnt.device)
    if size.dim() == 0:
        size = size.reshape(1)
    if size.shape[-1] < 3:  # sizes (1,) / (2,) of spheres / capsules: entries a type does not read
        size = torch.cat([size, size.new_zeros(size.shape[:-1] + (3 - size.shape[-1],))], -1)
    lead = torch.broadcast_shapes(size.shape[:-1], pnt.shape[:-1], vec.shape[:-1])
    size, p, v = size.expand(lead + (3,)), pnt.to(dtype).expand(lead + (3,)), vec.to(dtype).expand(lead + (3,))
    return _ray_geom(size, p, v, geomtype)
