"""The rest of MuJoCo's Jacobian block on a finished forward pass: ``mj_jacBody`` / ``mj_jacBodyCom`` / ``mj_jacSite`` / ``mj_jacGeom``, ``mj_jacSubtreeCom``,
``mj_jacDot`` and ``mj_angmomMat`` (the reference has ``jac`` alone).  One native launch each (``mjh_jacobian``, ``csrc/mjh_jacobian.h``, whose header states the
definitions and the order of every sum).

``jac_body(m, d, body_id)``, ``jac_body_com(m, d, body_id)``, ``jac_site(m, d, site_id)``, ``jac_geom(m, d, geom_id)`` return ``(jacp, jacr)``: ``jac`` at the
object's ``xpos`` / ``xipos`` / ``site_xpos`` / ``geom_xpos`` on its body, bit for bit (the point is gathered on the device and ``jac`` is called).
``jac_subtree_com(m, d, body_id)`` returns the Jacobian of the subtree's centre of mass, ``jac_dot(m, d, point, body_id)`` the pair of time derivatives
``(jacp_dot, jacr_dot)`` of ``jac`` along the motion (``qpos`` flows with ``qvel``, the point is carried rigidly by the body), ``angmom_mat(m, d, body_id)`` the matrix
that maps ``qvel`` to the subtree's angular momentum about its centre of mass.

Conventions are ``support.py``'s: every leading dimension of a leaf is the batch (S); ids are an int or P ids shared by all environments, a listed id adds a P
dimension; points are ``(3,)``, ``S + (3,)`` or ``S + (P, 3)``; matrices come back as ``jac`` returns them, ``S + [P] + (nv, 3)``, world-oriented.

``vec=``: an ``S + (nv,)`` tensor.  The function then returns the products ``sum_i M[i, :] vec[i]``, summed in ascending dof order, as ``S + [P] + (3,)`` (or a
pair of them); the matrix is never written.  ``jac_body(..., vec=d.qvel)`` is the object's velocity, ``jac_dot(..., vec=d.qvel)`` the ``Jdot qvel`` bias term.

``body_mass``, ``body_subtreemass`` and ``body_inertia`` are read from the caller's ``Model`` at each call, so a value-only edit such as
``mx.replace(body_mass=...)`` takes effect without a new native model (``jac_subtree_com`` divides by the Model's ``body_subtreemass``: edit both).

The calls run on the caller's current stream, in the model's dtype; nothing is written to the input.  ``torch.vmap`` / ``torch.compile``: there is no operator for
these functions; they raise ``NotImplementedError``.
"""

from __future__ import annotations

import math

import numpy as np
import torch

from . import native
from ._postpass import bind, call, check_leaves, check_override, model_value, probe, refuse_tracing, require_device
from .support import _device_ids, _query_mode, _strides, body_ids

POINT, DOT, SUBTREE_COM, ANGMOM = range(4)  # include/mjhip.h MJH_JACOBIAN_*
_NAMES = ("jac_point", "jac_dot", "jac_subtree_com", "angmom_mat")
_MASS_OK = {}  # (tensor address, version, ids) -> the body_subtreemass tensor checked for these ids (kept, so that the address stays its own)


class _Resolved(tuple):
    """(ids, listed) already validated by the caller (the object functions hand their objects' bodies down)."""


def _host_ints(x):
    x = x.data if not isinstance(x, (torch.Tensor, np.ndarray)) and isinstance(getattr(x, "data", None), torch.Tensor) else x  # (an UnbatchedTensor)
    return np.asarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x).astype(np.int64)


def _ids(name, what, ident, count):
    """``support.body_ids`` with the object's own name in the messages."""
    try:
        return body_ids(ident, count)
    except ValueError as exc:
        raise ValueError(f"{name}: {str(exc).replace('body_id', what + '_id').replace('body ids', what + ' ids')}") from None


def plan(name: str, m, op: int, leaves: dict, point, vec, ids: tuple, listed: bool):
    """Shape, dtype and device checks of one call: (batch, dtype, device, P or None, the point's mode)."""
    nv, nb = int(m.nv), int(m.nbody)
    tails = dict(cdof=(nv, 6), cdof_dot=(nv, 6), cvel=(nb, 6), subtree_com=(nb, 3), xipos=(nb, 3), ximat=(nb, 3, 3))
    batch, dtype, device = probe(name, m, "cdof", leaves["cdof"], (nv, 6))
    check_leaves(name, leaves, tails, batch, dtype, device, 3)
    mode, P = None, (len(ids) if listed else None)
    if point is not None:
        if not isinstance(point, torch.Tensor):
            raise ValueError(f"{name}: point must be a tensor, got {type(point).__name__}")
        try:
            mode = _query_mode("point", tuple(point.shape), batch, 3)
        except ValueError as exc:
            raise ValueError(f"{name}: {exc}") from None
        if mode[1] is not None:
            if mode[1] == 0:
                raise ValueError(f"{name}: no query points")
            if listed and len(ids) != mode[1]:
                raise ValueError(f"{name}: {len(ids)} body ids for {mode[1]} points")
            P = mode[1]
    if vec is not None:
        check_override(name, "vec", vec, batch + (nv,), dtype, device, "one vector per environment")
    return batch, dtype, device, P, mode


def _values(name, m, op, ids, dtype, device):
    """The model values of one call, from the caller's Model: {argument name: device tensor}; a subtree of zero mass is refused."""
    nb = int(m.nbody)
    out = {}
    for n, shape in (("body_mass", (nb,)), ("body_subtreemass", (nb,))) + ((("body_inertia", (nb, 3)),) if op == ANGMOM else ()):
        v = getattr(m, n)
        if tuple(np.shape(v)) != shape:
            raise ValueError(f"{name}: Model.{n} has shape {tuple(np.shape(v))}, expected {shape}")
        out[n] = model_value(m, n, v, dtype, device)
    sm = m.body_subtreemass
    key = (sm.data_ptr(), sm._version, ids) if isinstance(sm, torch.Tensor) else None
    if key is None or _MASS_OK.get(key) is not sm:  # (one read of the P masses; a tensor is read again only after it was written or replaced)
        mass = np.asarray(sm.detach().cpu().numpy() if isinstance(sm, torch.Tensor) else sm, dtype=np.float64)
        zero = [b for b in ids if mass[b] == 0]
        if zero:
            raise ValueError(f"{name}: the subtree of body {zero[0]} has no mass (Model.body_subtreemass[{zero[0]}] == 0): its centre of mass is undefined")
        if key is not None:
            if len(_MASS_OK) > 256:
                _MASS_OK.clear()
            _MASS_OK[key] = sm
    return out


def jacobian_native(name, m, op: int, leaves: dict, values: dict, point, mode, vec, ids: tuple, listed: bool, batch, P, dtype, device):
    """One ``mjh_jacobian`` call on plain tensors."""
    nv = int(m.nv)
    count = P or 1
    tail = ((P,) if P is not None else ()) + ((nv, 3) if vec is None else (3,))
    outs = [torch.empty(batch + tail, dtype=dtype, device=device) for _ in range(2 if op in (POINT, DOT) else 1)]
    B = int(math.prod(batch)) if batch else 1
    if B == 0 or nv == 0:
        return [o.zero_() for o in outs]
    a = native.ARGS["mjh_jacobian"](op=op, P=count, B=B, body_stride=1 if listed else 0)
    tensors = dict(leaves, **values, body_id=_device_ids(ids, device), **{f"out{i}": o for i, o in enumerate(outs)})
    if point is not None:
        tensors["point"] = point.to(device=device, dtype=dtype)
        a.point_env, a.point_q = _strides(mode, count, 3)
    if vec is not None:
        tensors["vec"] = vec
    bind(a, tensors)
    call(name, m, "mjh_jacobian", a, device, dtype)
    return outs


def _call(name, m, d, op, point, body_id, vec):
    refuse_tracing(name, d.cdof, point, vec)
    ids, listed = body_id if isinstance(body_id, _Resolved) else _ids(name, "body", body_id, int(m.nbody))
    leaves = dict(cdof=d.cdof, subtree_com=d.subtree_com)
    if op == DOT:
        leaves.update(cdof_dot=d.cdof_dot, cvel=d.cvel)
    if op in (SUBTREE_COM, ANGMOM):
        leaves.update(xipos=d.xipos)
    if op == ANGMOM:
        leaves.update(ximat=d.ximat)
    batch, dtype, device, P, mode = plan(name, m, op, leaves, point, vec, ids, listed)
    values = _values(name, m, op, ids, dtype, device) if op in (SUBTREE_COM, ANGMOM) else {}
    require_device(device)
    return jacobian_native(name, m, op, leaves, values, point, mode, vec, ids, listed, batch, P, dtype, device)


def _object(name, m, d, what, ident, count, pos, bodyid, vec):
    """jac at the gathered position of an object, on its body."""
    from . import support

    refuse_tracing(name, d.cdof, pos, vec)
    ids, listed = _ids(name, what, ident, int(count))
    want = tuple(d.cdof.shape[:-2]) + (int(count), 3)
    if tuple(pos.shape) != want:
        raise ValueError(f"{name}: the {what} positions have shape {tuple(pos.shape)}, expected {want} for this Model and a Data of batch shape {want[:-2]}")
    bodies = ids if bodyid is None else tuple(int(b) for b in _host_ints(bodyid)[list(ids)])
    point = pos.index_select(-2, _device_ids(ids, pos.device).to(torch.int64)) if listed else pos[..., ids[0], :]
    if vec is None:
        return support.jac(m, d, point, list(bodies) if listed else bodies[0])
    return tuple(_call(name, m, d, POINT, point, _Resolved((bodies, listed)), vec))


# ---- public functions -------------------------------------------------------------------------------------------------------

def jac_body(m, d, body_id, vec=None):
    """``(jacp, jacr)`` of the body's frame origin ``d.xpos`` (MuJoCo's ``mj_jacBody``): ``jac`` at that point, bit for bit.  ``S + [P] + (nv, 3)`` each; with
    ``vec=`` (``S + (nv,)``) the products ``S + [P] + (3,)``: ``vec=d.qvel`` gives the origin's linear and the body's angular velocity."""
    return _object("jac_body", m, d, "body", body_id, m.nbody, d.xpos, None, vec)


def jac_body_com(m, d, body_id, vec=None):
    """``(jacp, jacr)`` of the body's centre of mass ``d.xipos`` (MuJoCo's ``mj_jacBodyCom``).  Shapes and ``vec=`` as for ``jac_body``."""
    return _object("jac_body_com", m, d, "body", body_id, m.nbody, d.xipos, None, vec)


def jac_site(m, d, site_id, vec=None):
    """``(jacp, jacr)`` of a site, ``d.site_xpos`` on ``site_bodyid`` (MuJoCo's ``mj_jacSite``).  Shapes and ``vec=`` as for ``jac_body``."""
    return _object("jac_site", m, d, "site", site_id, m.nsite, d.site_xpos, m.site_bodyid, vec)


def jac_geom(m, d, geom_id, vec=None):
    """``(jacp, jacr)`` of a geom, ``d.geom_xpos`` on ``geom_bodyid`` (MuJoCo's ``mj_jacGeom``).  Shapes and ``vec=`` as for ``jac_body``."""
    return _object("jac_geom", m, d, "geom", geom_id, m.ngeom, d.geom_xpos, m.geom_bodyid, vec)


def jac_subtree_com(m, d, body_id, vec=None):
    """The Jacobian of the centre of mass of the body's subtree, ``S + [P] + (nv, 3)`` (MuJoCo's ``mj_jacSubtreeCom``): the mass-weighted mean of ``jac`` at the
    ``xipos`` of every body of the subtree.  Body 0 is the whole model.  A subtree of zero mass is refused.  ``vec=d.qvel`` gives ``subtree_linvel``."""
    return _call("jac_subtree_com", m, d, SUBTREE_COM, None, body_id, vec)[0]


def jac_dot(m, d, point, body_id, vec=None):
    """``(jacp_dot, jacr_dot)``: the time derivatives of ``jac(m, d, point, body_id)`` along the motion, ``qpos`` flowing with ``qvel`` and the point carried
    rigidly by the body (MuJoCo's ``mj_jacDot``).  ``point`` / ``body_id`` and the shapes as for ``jac``; ``vec=d.qvel`` gives the ``Jdot qvel`` term of the point's
    acceleration.  Reads ``cdof``, ``cdof_dot``, ``cvel`` and ``subtree_com``: they belong to the velocity the pass ran on."""
    point = point if isinstance(point, torch.Tensor) else torch.as_tensor(point)
    return tuple(_call("jac_dot", m, d, DOT, point, body_id, vec))


def angmom_mat(m, d, body_id, vec=None):
    """The matrix that maps ``qvel`` to the angular momentum of the body's subtree about the subtree's centre of mass, ``S + [P] + (nv, 3)`` (MuJoCo's
    ``mj_angmomMat``).  ``vec=d.qvel`` gives ``subtree_angmom``."""
    return _call("angmom_mat", m, d, ANGMOM, None, body_id, vec)[0]
