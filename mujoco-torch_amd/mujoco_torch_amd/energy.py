"""The potential and kinetic energy of a finished pass -- MuJoCo's ``mj_energyPos`` / ``mj_energyVel`` (``d.energy``), which the reference lacks -- and the
sensors no pass evaluates that read them or a limit's constraint row: jointlimitpos / vel / frc, tendonlimitpos / vel / frc, e_potential, e_kinetic.  One native
launch (``mjh_energy``, ``csrc/mjh_energy.h``, whose header states the definitions).

``energy(m, d, *, qpos=None, qvel=None)`` returns ``S + (2,)``, ``[potential, kinetic]``; ``energy_pos(m, d, *, qpos=None)`` and ``energy_vel(m, d, *,
qvel=None)`` return the halves, ``S``.  The potential is gravity (``-sum body_mass * dot(opt.gravity, xipos)``, unless ``DisableBit.GRAVITY``) plus the joint and
tendon springs (under the flags the step applies their forces under); the kinetic energy is ``1/2 qvel^T (qM qvel)`` with the pass's dense ``qM`` as stored.
Gravity compensation and fluid forces have no potential, as in MuJoCo.

``qpos=`` / ``qvel=``: the state the pass ran on.  On the output of ``forward`` that is ``d.qpos`` / ``d.qvel`` (the default).  On the output of ``step`` they are
already advanced while ``xipos``, ``ten_length`` and ``qM`` still belong to the pre-step state, so pass the pre-step values there (as for ``rne_postconstraint``).

The sensors are written by ``sensor_postconstraint(m, d, qvel, all_sensors=True)`` (``contact_sensors.py``).  A limit sensor whose joint or tendon has no
constraint row (not limited, or limits / constraints disabled) gives 0, as in MuJoCo.

The model VALUES the kernel uses -- ``opt.gravity``, ``body_mass``, ``jnt_stiffness``, ``qpos_spring``, ``jnt_range``, ``jnt_margin``, ``sensor_cutoff`` and the
tendons' ``tendon_stiffness`` / ``tendon_lengthspring`` / ``tendon_range`` / ``tendon_margin`` -- are read from the caller's ``Model`` at each call, so a value-only
edit such as ``mx.replace(body_mass=...)`` takes effect without a new native model (the tendon values are no ``Model`` fields: they come from the compiled model
the tables keep).

Every leading dimension of a leaf is the batch (S); nothing is written to the input.  The calls run on the caller's current stream.  ``torch.vmap`` /
``torch.compile``: there is no operator for these functions; they raise ``NotImplementedError``.
"""

from __future__ import annotations

import math

import numpy as np
import torch

from . import native
from ._enums import DisableBit
from ._postpass import bind, cached, call, check_leaves, check_override, model_value, probe, refuse_tracing, require_device, upload

POS, VEL, SENSORS = 1, 2, 4  # include/mjhip.h MJH_ENERGY_*
E_POTENTIAL, E_KINETIC = 43, 44
_DEV = {}   # (tables uid, device) -> the sensor rows on the device


def plan(name: str, m, leaves: dict, overrides: dict):
    """Shape, dtype and device checks of one call, as ``postconstraint.plan``: ``leaves`` maps leaf names to tensors, ``overrides`` the ``qpos=`` / ``qvel=``
    arguments; returns (batch, dtype, device)."""
    nq, nv, nb, nt, nsd = int(m.nq), int(m.nv), int(m.nbody), int(m.ntendon), int(getattr(m, "nsensordata", 0) or 0)
    nefc = int(m.constraint_sizes_py[4])
    tails = dict(qpos=(nq,), qvel=(nv,), xipos=(nb, 3), ten_length=(nt,), qM=(nv, nv), efc_J=(nefc, nv), efc_force=(nefc,), sensordata=(nsd,))
    batch, dtype, device = probe(name, m, "xipos", leaves["xipos"], (nb, 3))
    check_leaves(name, leaves, tails, batch, dtype, device, 2)
    for n, t in overrides.items():
        if t is not None:
            check_override(name, n, t, batch + tails[n], dtype, device, f"the {n} the pass ran on, per environment")
    return batch, dtype, device


def _values(name, m, dtype, device, cutoff_of=None):
    """The model values of one call, from the caller's Model: {argument name: device tensor}."""
    nq, nb, nj, nt = int(m.nq), int(m.nbody), int(m.njnt), int(m.ntendon)
    src = m.tables.source
    shapes = dict(gravity=(3,), body_mass=(nb,), jnt_stiffness=(nj,), qpos_spring=(nq,), jnt_range=(nj, 2), jnt_margin=(nj,), tendon_stiffness=(nt,),
                  tendon_lengthspring=(nt, 2), tendon_range=(nt, 2), tendon_margin=(nt,))
    out = {}
    for n, shape in shapes.items():
        if n.startswith("tendon_") and nt == 0:
            continue
        v = m.opt.gravity if n == "gravity" else (getattr(m, n) if hasattr(m, n) else getattr(src, n))
        if tuple(np.shape(v)) != shape:
            raise ValueError(f"{name}: Model.{'opt.' if n == 'gravity' else ''}{n} has shape {tuple(np.shape(v))}, expected {shape}")
        out[n] = model_value(m, n, v, dtype, device)
    if cutoff_of is not None:
        cut = m.sensor_cutoff
        if tuple(np.shape(cut)) != (int(m.nsensor),):
            raise ValueError(f"{name}: Model.sensor_cutoff has shape {tuple(np.shape(cut))}, expected ({int(m.nsensor)},)")
        if isinstance(cut, torch.Tensor):  # (gathered where it lives: no copy to the host)
            out["sns_cutoff"] = cut.detach()[torch.as_tensor(cutoff_of, dtype=torch.int64, device=cut.device)].to(device=device, dtype=dtype).contiguous()
        else:
            out["sns_cutoff"] = upload(m, "sensor_cutoff", np.asarray(cut, dtype=np.float64)[cutoff_of], dtype, device)
    return out


def _rows(name, m, device):
    def make():
        rows = m.tables.energy_sensors["rows"]
        nefc = int(m.constraint_sizes_py[4])
        for r in rows:  # (the kernel indexes with these unchecked)
            count = int(m.ntendon) if 23 <= r[0] <= 25 else (int(m.njnt) if 20 <= r[0] <= 22 else 1)
            if not (0 <= r[1] < int(m.nsensordata) and (r[0] in (E_POTENTIAL, E_KINETIC) or 0 <= r[2] < count) and -1 <= r[3] < nefc):
                raise RuntimeError(f"energy-sensor table row {r.tolist()} does not address this Model")
        return torch.tensor(rows, dtype=torch.int32, device=device).contiguous()

    return cached(_DEV, (m.tables.uid, device), make)


def _launch(name, m, device, dtype, B, flags, tensors, nsens=0):
    a = native.ARGS["mjh_energy"](flags=flags, nsens=nsens, B=B)
    bind(a, tensors)
    call(name, m, "mjh_energy", a, device, dtype)


def _springs(m):
    return not (int(m.opt.disableflags) & (DisableBit.SPRING | DisableBit.DAMPER))


def _run(name, m, d, flags, qpos, qvel):
    refuse_tracing(name, d.qpos, qpos, qvel)
    leaves = dict(xipos=d.xipos)
    if flags & POS:
        leaves.update(qpos=d.qpos)
        if int(m.ntendon) > 0:
            leaves.update(ten_length=d.ten_length)
    if flags & VEL:
        leaves.update(qvel=d.qvel, qM=d.qM)
    batch, dtype, device = plan(name, m, leaves, dict(qpos=qpos if flags & POS else None, qvel=qvel if flags & VEL else None))
    values = _values(name, m, dtype, device) if flags & POS else {}
    require_device(device)
    if qpos is not None and flags & POS:
        leaves["qpos"] = qpos
    if qvel is not None and flags & VEL:
        leaves["qvel"] = qvel
    B = int(math.prod(batch)) if batch else 1
    if B == 0:
        return torch.zeros(batch + (2,), dtype=dtype, device=device)
    out = torch.empty(batch + (2,), dtype=dtype, device=device)
    _launch(name, m, device, dtype, B, flags, dict(leaves, energy=out, **values), nsens=len(m.tables.energy_sensors["rows"]))  # (the table's size: it enters the lanes)
    return out


def energy(m, d, *, qpos=None, qvel=None):
    """``[potential, kinetic]`` of the finished forward pass ``d`` holds, ``S + (2,)`` (MuJoCo's ``mj_energyPos`` / ``mj_energyVel``).  ``qpos`` / ``qvel``: the
    state the pass ran on, ``S + (nq,)`` / ``S + (nv,)``; default ``d.qpos`` / ``d.qvel``, which is right for the output of ``forward``.  The output of ``step``
    carries the ADVANCED state: pass the pre-step values there."""
    return _run("energy", m, d, POS | VEL, qpos, qvel)


def energy_pos(m, d, *, qpos=None):
    """The potential energy, ``S``: gravity and the joint / tendon springs.  ``qpos``: as for ``energy``."""
    return _run("energy_pos", m, d, POS, qpos, None)[..., 0]


def energy_vel(m, d, *, qvel=None):
    """The kinetic energy ``1/2 qvel^T (qM qvel)``, ``S``.  ``qvel``: as for ``energy``."""
    return _run("energy_vel", m, d, VEL, None, qvel)[..., 1]


def plan_sensors(name, m, d, qvel):
    """The checks of ``sensor_postconstraint(all_sensors=True)``'s launch, made before anything is launched: None when the model has none of these sensors, else
    what ``write_sensors`` needs."""
    rows = m.tables.energy_sensors["rows"]
    nsd = int(getattr(m, "nsensordata", 0) or 0)
    if not len(rows) or nsd == 0:
        return None
    types = set(rows[:, 0].tolist())
    flags = SENSORS | (POS if E_POTENTIAL in types else 0) | (VEL if E_KINETIC in types else 0)
    leaves = dict(xipos=d.xipos, qpos=d.qpos, qvel=d.qvel)
    if int(m.ntendon) > 0:
        leaves.update(ten_length=d.ten_length)
    if flags & VEL:
        leaves.update(qM=d.qM)
    if int(m.constraint_sizes_py[4]) > 0 and int(m.nv) > 0:
        leaves.update(efc_J=d.efc_J, efc_force=d.efc_force)
    batch, dtype, device = plan(name, m, leaves, dict(qvel=qvel))
    if qvel is not None:
        leaves["qvel"] = qvel
    values = _values(name, m, dtype, device, cutoff_of=m.tables.energy_sensors["index"])
    return dict(flags=flags, leaves=leaves, values=values, batch=batch, dtype=dtype, device=device)


def write_sensors(name, m, p, sensordata):
    """Writes the slots of the joint / tendon limit and energy sensors into ``sensordata`` (``S + (nsensordata,)``, the caller's own fresh tensor)."""
    B = int(math.prod(p["batch"])) if p["batch"] else 1
    if B == 0:
        return
    dtype, device = p["dtype"], p["device"]
    rows = _rows(name, m, device)
    _launch(name, m, device, dtype, B, p["flags"], dict(p["leaves"], sns=rows, sensordata=sensordata, **p["values"]), nsens=int(rows.shape[0]))
