"""The force of every contact and the sensors that sit on it and on ``cacc``: MuJoCo's ``mj_contactForce`` (MJX ``support.contact_force``) and its touch,
framelinacc and frameangacc sensors.  The reference evaluates none of them: ``step`` / ``forward`` leave their ``sensordata`` slots as the caller set them, here
too.  These functions run on a finished pass, beside ``fwd_postconstraint``, through one native launch of their own (``mjh_contact_sensors``,
``csrc/mjh_contact_sensors.h``, whose header states the definitions).

``contact_force(m, d, contact_id=None, to_world_frame=False)`` returns ``S + (ncon, 6)``: per contact slot ``[force(3), torque(3)]`` (MuJoCo's order, not the
rotational-first order of ``cfrc_ext``) in the contact frame -- ``force[0]`` is the normal force --, decoded from ``efc_force`` exactly as ``rne_postconstraint``
decodes it; ``to_world_frame=True`` rotates both halves by ``contact.frame^T``.  ``contact_id``: an int (``S + (6,)``) or a flat sequence of slots shared by all
environments (``S + (P, 6)``).  A slot whose geom ids are not in ``[0, ngeom)`` (an unused slot of a ``max_contact_points`` model), or whose rows do not lie
inside ``efc_force``, gives zeros.

``sensor_postconstraint(m, d, qvel=None)`` returns ``fwd_postconstraint(m, d, qvel, sensors=True)`` -- the five leaves and every slot it writes or copies, bit
for bit -- with, in addition, the slots of the touch, framelinacc and frameangacc sensors evaluated (the second launch reads ``cacc`` from the first one's
output).  A touch sensor sums the normal forces of the contacts of its site's body whose ray from the contact point along the normal, pointing out of that body,
meets the site's shape (sphere, capsule, ellipsoid, cylinder or box; ``Model.site_size`` is read at each call, so value edits take effect).  framelinacc / frameangacc are in the world
frame; a reference frame (``reftype`` / ``refname``) on these two types is ignored, as MuJoCo ignores it.  With ``DisableBit.SENSOR``, or a model without
these sensors, the result is ``fwd_postconstraint``'s.  ``all_sensors=True`` also writes the slots of the joint / tendon limit sensors and the energy sensors
(jointlimitpos / vel / frc, tendonlimitpos / vel / frc, e_potential, e_kinetic; ``energy.py``) by one more launch; every other slot is as without it.

Every leading dimension of a leaf is the batch (S); the input is never written and every other leaf of the result aliases it.  The calls run on the caller's
current stream.  ``torch.vmap`` / ``torch.compile``: there is no operator for these functions; they raise ``NotImplementedError``.
"""

from __future__ import annotations

import math

import numpy as np
import torch

from . import native
from ._postpass import bind, cached, call, check_leaves, probe, refuse_tracing, require_device, upload
from .postconstraint import CONTACT_INTS

FORCES, SENSORS, WORLD = 1, 2, 4  # include/mjhip.h MJH_CONSENS_*
TOUCH = 0
_ZONES = {2: "sphere", 3: "capsule", 4: "ellipsoid", 5: "cylinder", 6: "box"}  # the site shapes a touch zone can have (GeomType)
_DEV = {}  # (tables uid, dtype, device) -> the sensor rows and cutoffs on the device


def _tables(m, dtype, device):
    def make():
        cs = m.tables.contact_sensors
        counts = (int(m.nbody), int(m.nbody), int(m.ngeom), int(m.nsite), int(m.ncam))
        for r in cs["rows"]:  # (the kernel indexes with these unchecked)
            if not (0 <= r[1] and r[1] + (1 if r[0] == TOUCH else 3) <= int(m.nsensordata) and 0 <= r[3] < 5 and 0 <= r[2] < counts[r[3]] and 0 <= r[4] < counts[0]
                    and 0 <= r[5] < counts[0]):
                raise RuntimeError(f"contact-sensor table row {r.tolist()} does not address this Model")
        return dict(rows=torch.tensor(cs["rows"], dtype=torch.int32, device=device).contiguous(), cutoff=torch.tensor(cs["cutoff"], dtype=dtype, device=device).contiguous())

    return cached(_DEV, (m.tables.uid, dtype, device), make)


def _contact_leaves(m, d):
    _, _, _, ncon, nefc = m.constraint_sizes_py
    if ncon == 0 or nefc == 0:
        return {}, {}
    c = d.contact
    leaves = dict(efc_force=d.efc_force, contact_pos=c.pos, contact_frame=c.frame, contact_friction=c.friction, contact_dim=c.contact_dim, contact_geom=c.geom,
                  contact_efc_address=c.efc_address)
    tails = dict(efc_force=(nefc,), contact_pos=(ncon, 3), contact_frame=(ncon, 3, 3), contact_friction=(ncon, 5), contact_dim=(ncon,), contact_geom=(ncon, 2),
                 contact_efc_address=(ncon,))
    return leaves, tails


def _launch(name, m, device, dtype, B, flags, tensors, nsens=0):
    a = native.ARGS["mjh_contact_sensors"](flags=flags, nsens=nsens, B=B)
    bind(a, tensors)
    call(name, m, "mjh_contact_sensors", a, device, dtype)


def _slots(name, contact_id, ncon):
    """(list of slots, whether an int was given)."""
    if isinstance(contact_id, bool):
        raise ValueError(f"{name}: contact_id must be an int or a flat sequence of ints, got a bool")
    if isinstance(contact_id, (int, np.integer)):
        ids, one = [int(contact_id)], True
    else:
        arr = contact_id.detach().cpu().numpy() if isinstance(contact_id, torch.Tensor) else np.asarray(contact_id)
        if arr.ndim != 1 or (arr.size and not np.issubdtype(arr.dtype, np.integer)):
            raise ValueError(f"{name}: contact_id must be an int or a flat sequence of ints shared by all environments, got shape {arr.shape} of {arr.dtype}")
        ids, one = [int(i) for i in arr], False
    for i in ids:
        if not 0 <= i < ncon:
            raise ValueError(f"{name}: contact_id {i} is not a contact slot of this Model (ncon = {ncon})")
    return ids, one


def contact_force(m, d, contact_id=None, to_world_frame: bool = False):
    """The force of every contact slot of the finished pass ``d`` holds (MuJoCo's ``mj_contactForce``): ``S + (ncon, 6)``, each row ``[force(3), torque(3)]`` in
    the contact frame (``[..., 0]`` is the normal force), or in the world frame with ``to_world_frame=True``.  ``contact_id``: an int (``S + (6,)``) or a flat
    sequence of slots shared by all environments (``S + (P, 6)``).  An unused slot gives zeros; a model without contacts or constraint rows an empty / zero result."""
    name = "contact_force"
    refuse_tracing(name, d.qpos, d.efc_force)
    _, _, _, ncon, nefc = m.constraint_sizes_py
    batch, dtype, device = probe(name, m, "qpos", d.qpos, (int(m.nq),))
    leaves, tails = _contact_leaves(m, d)
    check_leaves(name, leaves, tails, batch, dtype, device, 3, CONTACT_INTS)
    ids, one = (None, False) if contact_id is None else _slots(name, contact_id, ncon)
    require_device(device)
    B = int(math.prod(batch)) if batch else 1
    if B == 0 or not leaves:
        out = torch.zeros(batch + (ncon, 6), dtype=dtype, device=device)
    else:
        out = torch.empty(batch + (ncon, 6), dtype=dtype, device=device)
        _launch(name, m, device, dtype, B, FORCES | (WORLD if to_world_frame else 0), dict(leaves, force=out))
    if ids is None:
        return out
    return out[..., ids[0], :] if one else out[..., torch.tensor(ids, dtype=torch.int64, device=device), :]


def _refuse_zones(name, m):
    rows = m.tables.contact_sensors["rows"]
    for r in rows:
        if int(r[0]) == TOUCH and int(r[7]) not in _ZONES:
            raise NotImplementedError(f"{name}: the touch sensor on site {int(r[2])} has a zone of geom type {int(r[7])}; a touch zone is a "
                                      f"{' / '.join(_ZONES.values())} site")


def sensor_postconstraint(m, d, qvel=None, *, all_sensors: bool = False):
    """``fwd_postconstraint(m, d, qvel, sensors=True)`` -- the five leaves and the ``sensordata`` slots it writes or copies, bit for bit -- plus the slots of the
    touch, framelinacc and frameangacc sensors, evaluated from the pass's contact forces and the fresh ``cacc`` by one more launch.  ``qvel``: as for
    ``rne_postconstraint``.  A reference frame on framelinacc / frameangacc is ignored, as MuJoCo ignores it.

    ``all_sensors=True``: the same ``Data`` with, in addition, the slots of the jointlimitpos / vel / frc, tendonlimitpos / vel / frc, e_potential and e_kinetic
    sensors written (``energy.py``: one more launch; ``qvel`` serves the limit velocities and the kinetic energy too)."""
    name = "sensor_postconstraint"
    refuse_tracing(name, d.qpos, qvel)
    _refuse_zones(name, m)
    if not all_sensors:
        return _sensor_postconstraint(name, m, d, qvel)
    from .energy import plan_sensors, write_sensors

    p = plan_sensors(name, m, d, qvel)  # (checked before the first launch: a refused call launches nothing)
    out = _sensor_postconstraint(name, m, d, qvel)
    if p is not None:
        write_sensors(name, m, p, out.sensordata)  # (fwd_postconstraint's own fresh sensordata)
    return out


def _sensor_postconstraint(name, m, d, qvel):
    from .postconstraint import RNE, SENSORS as PC_SENSORS, SUBTREE, _run

    rows = m.tables.contact_sensors["rows"]
    nsd = int(getattr(m, "nsensordata", 0) or 0)
    extra, tails = {}, {}
    if len(rows) and nsd > 0:  # (checked before the first launch: a refused call launches nothing)
        batch, dtype, device = probe(name, m, "qpos", d.qpos, (int(m.nq),))
        nb, ng, ns, nc = int(m.nbody), int(m.ngeom), int(m.nsite), int(m.ncam)
        extra, tails = _contact_leaves(m, d)
        extra.update(xpos=d.xpos, geom_xpos=d.geom_xpos, cam_xpos=d.cam_xpos)
        tails.update(xpos=(nb, 3), geom_xpos=(ng, 3), cam_xpos=(nc, 3))
        check_leaves(name, extra, tails, batch, dtype, device, 3, CONTACT_INTS)
        size = np.asarray(m.site_size.detach().cpu().numpy() if isinstance(m.site_size, torch.Tensor) else m.site_size, dtype=np.float64)
        if size.shape != (ns, 3):
            raise ValueError(f"{name}: Model.site_size has shape {size.shape}, expected ({ns}, 3)")
    out = _run(name, m, d, qvel, RNE | SUBTREE | PC_SENSORS)
    if not (len(rows) and nsd > 0):
        return out
    B = int(math.prod(batch)) if batch else 1
    if B == 0:
        return out
    t = _tables(m, dtype, device)
    leaves = dict(extra, site_xpos=d.site_xpos, site_xmat=d.site_xmat, cvel=d.cvel, cacc=out.cacc, subtree_com=d.subtree_com, xipos=d.xipos, site_size=upload(m, "site_size", size, dtype, device),
                  sns=t["rows"], sns_cutoff=t["cutoff"], sensordata=out.sensordata)
    _launch(name, m, device, dtype, B, SENSORS, leaves, nsens=int(t["rows"].shape[0]))
    return out
