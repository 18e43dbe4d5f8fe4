"""The signed distance between geoms and their nearest points on a finished pass -- MuJoCo's ``mj_geomDistance``, which the reference lacks.  One native launch
(``mjh_geom_distance``, ``csrc/mjh_geomdist.h``, whose header states the definitions): one lane per (pair, environment).

``geom_distance(m, d, geom1, geom2, distmax)`` returns ``(dist, fromto)``.  ``geom1`` / ``geom2``: one geom id each (an int or a 0-d integer tensor or array) or P ids (a
sequence or a 1-D integer tensor), shared by every environment; one id broadcasts against P.  For a Data of batch shape ``S``: ``dist`` is ``S + (P,)`` and
``fromto`` ``S + (P, 6)`` (``S`` and ``S + (6,)`` for two single ids), in the Data dtype.  ``fromto[..., :3]`` is the nearest point on the surface of ``geom1``,
``fromto[..., 3:]`` the one on ``geom2``: with ``n`` the unit vector from geom1 towards geom2, ``to - from = dist * n`` -- also where the geoms overlap; then
``dist < 0`` and the points are the witnesses of the minimum translation.  Where the geometry leaves no direction, ``dist`` is still exact and the points still
lie on the surfaces: ``n`` is the world ``+z`` for concentric spheres, and a unit vector perpendicular to the capsule's segment for capsules whose axes meet or
coincide and for a sphere centred on a capsule's axis.  Where ``dist > distmax`` the result is ``dist = distmax`` and ``fromto = 0``
(MuJoCo's convention).

Supported: sphere, capsule and box with each other, and a plane (infinite, as in collisions) with a sphere, capsule, box, ellipsoid or cylinder, in either order.
Anything with a mesh or hfield, an ellipsoid or cylinder with anything but a plane, and plane-plane raise ``NotImplementedError``.

Only ``d.geom_xpos`` / ``d.geom_xmat`` are read: the output of any pass that ran the position stage.  ``geom_size`` is read from the caller's ``Model`` at each
call, so a value-only edit ``mx.replace(geom_size=...)`` takes effect without a new native model; the geom types come from the tables.  Geoms that never collide
(``contype=0``) have a distance like any other.

Every leading dimension of a leaf is the batch (S); nothing is written to the input.  The call runs on the caller's current stream.  ``torch.vmap`` /
``torch.compile``: there is no operator for this function; it raises ``NotImplementedError``.
"""

from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from ._enums import GeomType
from ._postpass import cached, call, check_leaves, model_value, probe, refuse_tracing, require_device

_CORE = (int(GeomType.SPHERE), int(GeomType.CAPSULE), int(GeomType.BOX))
_ON_PLANE = _CORE + (int(GeomType.ELLIPSOID), int(GeomType.CYLINDER))
_DEV = {}  # (tables uid, the pair rows' bytes, device) -> the rows on the device


def _ids(name, arg, g, ngeom):
    """(ids as a list, single?) of one of the two id arguments."""
    if isinstance(g, torch.Tensor):
        if g.dtype in (torch.bool, torch.float16, torch.bfloat16, torch.float32, torch.float64) or g.is_complex():
            raise ValueError(f"{name}: {arg} must hold integer geom ids; got a {g.dtype} tensor")
        if g.dim() > 1:
            raise ValueError(f"{name}: {arg} has shape {tuple(g.shape)}: the pairs are shared by every environment, pass one id or a 1-D list of ids")
        single, ids = g.dim() == 0, [int(v) for v in g.reshape(-1).tolist()]
    elif isinstance(g, (int, np.integer)) and not isinstance(g, bool):
        single, ids = True, [int(g)]
    else:
        arr = np.asarray(g)
        if arr.ndim == 0 and arr.dtype.kind in "iu":  # (a 0-d integer array: one id, like a 0-d tensor)
            return _ids(name, arg, int(arr), ngeom)
        if arr.ndim != 1 or (arr.size and arr.dtype.kind not in "iu"):
            raise ValueError(f"{name}: {arg} must be one geom id or a 1-D sequence of ids, shared by every environment; got shape {arr.shape}, dtype {arr.dtype}")
        single, ids = False, [int(v) for v in arr.tolist()]
    for v in ids:
        if not 0 <= v < ngeom:
            raise ValueError(f"{name}: {arg} holds geom id {v}, the Model has {ngeom} geoms")
    return ids, single


def pair_rows(name, m, geom1, geom2):
    """The pair table of one call, ``[P, 4]`` int32 (geom1, geom2, type1, type2), and whether both ids were single: every refusal about the ids is made here."""
    ngeom = int(m.ngeom)
    a, sa = _ids(name, "geom1", geom1, ngeom)
    b, sb = _ids(name, "geom2", geom2, ngeom)
    if len(a) != len(b):
        if sa:
            a = a * len(b)
        elif sb:
            b = b * len(a)
        else:
            raise ValueError(f"{name}: geom1 holds {len(a)} ids and geom2 {len(b)}: they do not broadcast")
    gtype = np.asarray(m.tables.ray["geom_type"])
    rows = np.zeros((len(a), 4), dtype=np.int32)
    for i, (g1, g2) in enumerate(zip(a, b)):
        if g1 == g2:
            raise ValueError(f"{name}: pair {i} is geom {g1} with itself")
        t1, t2 = int(gtype[g1]), int(gtype[g2])
        plane = int(GeomType.PLANE)
        ok = (t1 in _CORE and t2 in _CORE) or (t1 == plane and t2 in _ON_PLANE) or (t2 == plane and t1 in _ON_PLANE)
        if not ok:
            raise NotImplementedError(f"{name}: pair {i} (geoms {g1}, {g2}) is {GeomType(t1).name.lower()}-{GeomType(t2).name.lower()}: supported are sphere / "
                                      "capsule / box with each other and a plane with a sphere, capsule, box, ellipsoid or cylinder")
        rows[i] = (g1, g2, t1, t2)
    return rows, sa and sb


def geom_distance(m, d, geom1, geom2, distmax):
    """``(dist, fromto)``: the signed distance of geom pairs and their nearest points, ``S + (P,)`` / ``S + (P, 6)`` (``S`` / ``S + (6,)`` for two single ids);
    the module's docstring has the conventions."""
    name = "geom_distance"
    xpos, xmat = d.geom_xpos, d.geom_xmat
    refuse_tracing(name, xpos, xmat, geom1, geom2)
    ng = int(m.ngeom)
    batch, dtype, device = probe(name, m, "geom_xpos", xpos, (ng, 3))
    check_leaves(name, dict(geom_xmat=xmat), dict(geom_xmat=(ng, 3, 3)), batch, dtype, device, 3)
    rows, single = pair_rows(name, m, geom1, geom2)
    if isinstance(distmax, torch.Tensor) and distmax.numel() == 1:
        distmax = distmax.item()
    if not isinstance(distmax, (int, float, np.integer, np.floating)) or isinstance(distmax, bool) or not float(distmax) >= 0:
        raise ValueError(f"{name}: distmax must be a non-negative float; got {distmax!r}")
    if tuple(np.shape(m.geom_size)) != (ng, 3):
        raise ValueError(f"{name}: Model.geom_size has shape {tuple(np.shape(m.geom_size))}, expected {(ng, 3)}")
    require_device(device)
    P = int(rows.shape[0])
    B = int(math.prod(batch)) if batch else 1
    shape = batch if single else batch + (P,)
    if B == 0 or P == 0:
        return torch.zeros(shape, dtype=dtype, device=device), torch.zeros(shape + (6,), dtype=dtype, device=device)
    size = model_value(m, "geom_size", m.geom_size, dtype, device)
    table = cached(_DEV, (m.tables.uid, rows.tobytes(), device), lambda: torch.tensor(rows, dtype=torch.int32, device=device).contiguous())
    xpos_c, xmat_c = xpos.reshape(B, ng, 3).contiguous(), xmat.reshape(B, ng, 9).contiguous()
    dist = torch.empty((B, P), dtype=dtype, device=device)
    fromto = torch.empty((B, P, 6), dtype=dtype, device=device)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    call(name, m, "mjh_geom_distance", (ptr(xpos_c), ptr(xmat_c), ptr(size), ptr(table), P, ctypes.c_double(float(distmax)), ptr(dist), ptr(fromto), B), device,
         dtype)
    return dist.reshape(shape), fromto.reshape(shape + (6,))
