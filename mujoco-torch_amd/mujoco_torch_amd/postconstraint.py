"""Body accelerations and forces behind a finished forward pass: MuJoCo's ``mj_rnePostConstraint`` and ``mj_subtreeVel`` (MJX
``smooth.rne_postconstraint`` / ``smooth.subtree_vel``; the reference has neither, so its ``Data`` keeps ``cacc``, ``cfrc_int``, ``cfrc_ext``,
``subtree_linvel`` and ``subtree_angmom`` as ``make_data`` or the caller left them).

``rne_postconstraint(m, d, qvel=None)`` returns a ``Data`` with ``cacc``, ``cfrc_int`` and ``cfrc_ext`` (``S + (nbody, 6)``) replaced,
``subtree_vel(m, d)`` one with ``subtree_linvel`` and ``subtree_angmom`` (``S + (nbody, 3)``) replaced, ``fwd_postconstraint(m, d, qvel=None,
sensors=False)`` both -- in ONE native launch (``mjh_postconstraint``, ``csrc/mjh_postcon.h``) -- and with ``sensors=True`` also a ``sensordata``
whose accelerometer, force, torque, subtreelinvel and subtreeangmom slots are recomputed from the fresh leaves (every other slot is copied).
Every leading dimension of a leaf is the batch (S), as for the support functions; the input is never written and every other leaf of the
result aliases it.  The calls run on the caller's current stream and read only leaves of a finished forward pass, so the caller runs
``forward`` / ``step`` first.

Spatial vectors are ``[rotational(3), translational(3)]`` in the world frame about ``subtree_com[body_rootid[b]]`` (the convention of ``cvel`` /
``cdof`` / ``cinert``).  ``cfrc_ext`` holds ``xfrc_applied`` and the contact forces; the forces of equality constraints (connect / weld), joint
and tendon limits and frictionloss are NOT added: they stay joint-space (``qfrc_constraint``).  ``cfrc_int[b]`` is the force the parent of ``b``
exerts on ``b``'s subtree (body 0 accumulates like any other body).

``qvel=``: ``cacc`` needs the velocity the pass ran on.  On the output of ``forward`` that is ``d.qvel`` (the default).  On the output of ``step``
``d.qvel`` is already advanced, so pass the pre-step velocity, ``S + (nv,)``; the derived leaves then belong to the PRE-step state, as in MuJoCo
(``mj_step`` leaves ``cacc`` / ``cfrc_*`` of the state it started from).

``torch.vmap`` / ``torch.compile``: there is no operator for these functions; they raise ``NotImplementedError``.
"""

from __future__ import annotations

import math

import torch

from . import native
from ._postpass import bind, call, check_leaves, check_override, probe, refuse_tracing, require_device

RNE, SUBTREE, SENSORS = 1, 2, 4  # include/mjhip.h MJH_POSTCON_*
CONTACT_INTS = dict(contact_dim=torch.int32, contact_geom=torch.int64, contact_efc_address=torch.int64)


def plan(name: str, m, leaves: dict, qvel, flags: int):
    """Shape, dtype and device checks of one call: ``leaves`` maps leaf names to tensors; returns (batch, dtype, device)."""
    nb, nv, nsite, nsd = int(m.nbody), int(m.nv), int(m.nsite), int(getattr(m, "nsensordata", 0) or 0)
    _, _, _, ncon, nefc = m.constraint_sizes_py
    tails = dict(qvel=(nv,), qacc=(nv,), cdof=(nv, 6), cdof_dot=(nv, 6), cvel=(nb, 6), cinert=(nb, 10), xipos=(nb, 3), ximat=(nb, 3, 3), subtree_com=(nb, 3),
                 xfrc_applied=(nb, 6), efc_force=(nefc,), contact_pos=(ncon, 3), contact_frame=(ncon, 3, 3), contact_friction=(ncon, 5), contact_dim=(ncon,),
                 contact_geom=(ncon, 2), contact_efc_address=(ncon,), site_xpos=(nsite, 3), site_xmat=(nsite, 3, 3), sensordata=(nsd,))
    batch, dtype, device = probe(name, m, "cvel", leaves["cvel"], (nb, 6))
    check_leaves(name, leaves, tails, batch, dtype, device, 3, CONTACT_INTS)
    if qvel is not None:
        check_override(name, "qvel", qvel, batch + (nv,), dtype, device, "the velocity the pass ran on, per environment")
    if flags & SUBTREE:
        sm = m.body_subtreemass
        if tuple(sm.shape) != (nb,) or sm.dtype != dtype or sm.device != device:
            raise ValueError(f"{name}: Model.body_subtreemass is {tuple(sm.shape)} {sm.dtype} on {sm.device}, expected ({nb},) {dtype} on {device}")
    return batch, dtype, device


def _run(name: str, m, d, qvel, flags: int):
    refuse_tracing(name, d.qpos, qvel)
    _, _, _, ncon, nefc = m.constraint_sizes_py
    nsd = int(getattr(m, "nsensordata", 0) or 0)
    leaves = dict(cvel=d.cvel, xipos=d.xipos, subtree_com=d.subtree_com)
    if flags & RNE:
        leaves.update(qvel=d.qvel, qacc=d.qacc, cdof=d.cdof, cdof_dot=d.cdof_dot, cinert=d.cinert, xfrc_applied=d.xfrc_applied)
        if ncon > 0 and nefc > 0:
            c = d.contact
            leaves.update(efc_force=d.efc_force, contact_pos=c.pos, contact_frame=c.frame, contact_friction=c.friction, contact_dim=c.contact_dim,
                          contact_geom=c.geom, contact_efc_address=c.efc_address)
    if flags & SUBTREE:
        leaves.update(ximat=d.ximat)
    if flags & SENSORS and nsd > 0:
        leaves.update(sensordata=d.sensordata)
        if int(m.nsite) > 0:
            leaves.update(site_xpos=d.site_xpos, site_xmat=d.site_xmat)
    else:
        flags &= ~SENSORS
    batch, dtype, device = plan(name, m, leaves, qvel, flags)
    require_device(device)
    if qvel is not None:
        leaves["qvel"] = qvel
    nb = int(m.nbody)
    B = int(math.prod(batch)) if batch else 1
    new = lambda *tail: torch.empty(batch + tail, dtype=dtype, device=device)
    out = {}
    if flags & RNE:
        out.update(cacc=new(nb, 6), cfrc_int=new(nb, 6), cfrc_ext=new(nb, 6))
    if flags & SUBTREE:
        out.update(subtree_linvel=new(nb, 3), subtree_angmom=new(nb, 3))
    if flags & SENSORS:
        out.update(sensordata=new(nsd))
    if B == 0 or nb == 0:
        return d.replace(**{k: v.zero_() for k, v in out.items()})
    a = native.ARGS["mjh_postconstraint"](flags=flags, B=B)
    if "sensordata" in leaves:
        leaves["sensordata_in"] = leaves.pop("sensordata")
    if flags & SUBTREE:
        leaves["body_subtreemass"] = m.body_subtreemass
    bind(a, dict(leaves, **out))
    call(name, m, "mjh_postconstraint", a, device, dtype)
    return d.replace(**out)


def rne_postconstraint(m, d, qvel=None):
    """``d`` with ``cacc``, ``cfrc_int`` and ``cfrc_ext`` (``S + (nbody, 6)``) computed from the finished forward pass ``d`` holds (MuJoCo's
    ``mj_rnePostConstraint``).  ``cfrc_ext``: ``xfrc_applied`` and the contact forces (from ``efc_force``) on each body; equality (connect / weld),
    limit and frictionloss forces are not added, they stay joint-space.  ``cacc[0] = [0, 0, 0, -gravity]``.

    ``qvel``: the velocity the pass ran on, ``S + (nv,)``; default ``d.qvel``, which is right for the output of ``forward``.  The output of
    ``step`` carries the ADVANCED velocity: pass the pre-step ``qvel`` there, and read the result as the leaves of the pre-step state, as in MuJoCo."""
    return _run("rne_postconstraint", m, d, qvel, RNE)


def subtree_vel(m, d):
    """``d`` with ``subtree_linvel`` (the velocity of each subtree's centre of mass) and ``subtree_angmom`` (its angular momentum about that centre),
    ``S + (nbody, 3)``, computed from ``cvel`` / ``xipos`` / ``ximat`` / ``subtree_com`` (MuJoCo's ``mj_subtreeVel``).  Like ``cvel``, they belong to the
    velocity the pass ran on."""
    return _run("subtree_vel", m, d, None, SUBTREE)


def fwd_postconstraint(m, d, qvel=None, sensors: bool = False):
    """``subtree_vel(m, rne_postconstraint(m, d, qvel))`` in one launch, bit for bit.  ``sensors=True`` also replaces ``sensordata``: the slots of
    accelerometer, force, torque, subtreelinvel and subtreeangmom sensors are evaluated from the fresh leaves (with their cutoff), every other slot
    keeps ``d.sensordata``.  ``qvel``: as for ``rne_postconstraint``."""
    return _run("fwd_postconstraint", m, d, qvel, RNE | SUBTREE | (SENSORS if sensors else 0))
