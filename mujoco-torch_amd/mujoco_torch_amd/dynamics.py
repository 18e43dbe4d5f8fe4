"""The reference's ``tendon`` / ``transmission`` (``_src/smooth.py:470-497, 535-591``), ``passive`` (``_src/passive.py``) and ``fwd_velocity`` / ``fwd_actuation`` /
``fwd_acceleration`` (``_src/forward.py:87-228``) as functions on a caller's ``Data``.  Each reads the leaves of ``d`` AS THEY ARE -- nothing is recomputed from
``qpos`` that the function does not itself compute from ``qpos`` -- and returns ``d.replace(...)`` with exactly its own leaves as fresh tensors; every other leaf of the
result is the caller's tensor object, and nothing is written to the input.  With the stages of ``smooth.py`` the calls

    kinematics -> com_pos -> tendon -> crb -> tendon_armature -> factor_m -> transmission -> fwd_velocity -> fwd_actuation -> fwd_acceleration

are ``forward`` up to ``qacc_smooth``, one stage at a time, with any leaf editable in between and no collision or constraint assembly.

====================  ==============================================================================  ===================================================
function              reads from ``d``                                                                leaves replaced
====================  ==============================================================================  ===================================================
``tendon``            ``qpos``                                                                        ``ten_length``, ``ten_J`` (dense ``(ntendon, nv)``);
                                                                                                      ``d`` itself without tendons
``transmission``      ``qpos``, ``ten_length``, ``ten_J``                                             ``actuator_length``, ``actuator_moment`` ``(nu, nv)``;
                                                                                                      ``d`` itself without actuators
``passive``           ``qpos``, ``qvel``, ``ten_length``, ``ten_velocity``, ``ten_J``; with gravcomp  ``qfrc_passive``, ``qfrc_gravcomp`` (the caller's
                      ``xipos``, ``subtree_com``, ``cdof``; with fluid also ``ximat``, ``cvel``       object on a model without gravcomp or with GRAVITY
                                                                                                      disabled)
``fwd_velocity``      ``actuator_moment``, ``ten_J``, ``qvel`` and what ``com_vel``, ``passive``,     ``actuator_velocity``, ``ten_velocity`` (with
                      ``rne`` read                                                                    tendons), ``cvel``, ``cdof_dot``, ``qfrc_passive``,
                                                                                                      ``qfrc_gravcomp``, ``qfrc_bias``
``fwd_actuation``     ``ctrl``, ``act``, ``actuator_length``, ``actuator_velocity``,                  ``act_dot``, ``qfrc_actuator``, ``actuator_force``
                      ``actuator_moment``, ``qfrc_gravcomp``                                          (the caller's with ``nu == 0`` or ACTUATION disabled)
``fwd_acceleration``  ``qfrc_applied``, ``xfrc_applied``, ``xipos``, ``subtree_com``, ``cdof``,       ``qfrc_smooth``, ``qacc_smooth``
                      ``qfrc_passive``, ``qfrc_bias``, ``qfrc_actuator``, ``qLD``
====================  ==============================================================================  ===================================================

Each is one native launch (``mjh_dynamics``, ``csrc/mjh_dynamics.h``, whose header states the definitions and the order of every sum); ``fwd_velocity`` is the launch of
the two products followed by ``com_vel``, ``passive`` and ``rne`` -- that sequence itself, so it equals calling them one after the other bit for bit.  The branches
that compute nothing launch nothing: ``passive`` with ``DisableBit.SPRING`` or ``DAMPER`` (both outputs zero), ``fwd_actuation`` with ``nu == 0`` or
``DisableBit.ACTUATION`` (``act_dot`` and ``qfrc_actuator`` zero), an empty leaf (``nv == 0``, no tendons, ``B == 0``).

The model VALUES are read from the caller's ``Model`` at each call (a field ``Model`` does not carry -- the tendons' stiffness, damping and ``lengthspring`` -- from the
compiled model the tables keep): ``jnt_stiffness``, ``qpos_spring``, ``dof_damping``, ``body_mass`` / ``body_inertia`` / ``body_gravcomp``, ``jnt_actgravcomp``,
``jnt_actfrcrange``, ``actuator_gainprm`` / ``biasprm`` / ``dynprm`` / ``ctrlrange`` / ``forcerange`` / ``gear`` / ``lengthrange`` / ``acc0``, ``has_gravcomp`` and
``opt.gravity`` / ``wind`` / ``viscosity`` / ``density`` / ``has_fluid_params`` / ``disableflags``.  So a value-only edit such as ``mx.replace(dof_damping=...)`` takes effect
without a new native model; the structure (which actuator drives what, the dyn / gain / bias types, the limited flags, the tendons' joint terms, the tree) is the
compiled model's.  A model one environment of which does not fit the LDS of a CU is refused with a ``RuntimeError`` naming the sizes (``plan``).

Every leading dimension of a leaf is the batch (S); matrices may come as ``(n, 3, 3)`` or ``(n, 9)``.  The calls run on the caller's current stream.  ``torch.vmap`` /
``torch.compile``: there is no operator for these functions; they raise ``NotImplementedError``.
"""

from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from . import native
from ._enums import DisableBit
from ._postpass import bind, call, check_leaves, model_value, probe, refuse_tracing, require_device
from .smooth import com_vel, rne

TENDON, TRANSMISSION, VELOCITY, PASSIVE, ACTUATION, ACCELERATION = range(6)  # include/mjhip.h MJH_DYNAMICS_*
OPS = dict(tendon=TENDON, transmission=TRANSMISSION, velocity=VELOCITY, passive=PASSIVE, actuation=ACTUATION, acceleration=ACCELERATION)
GAIN_MUSCLE = BIAS_MUSCLE = 2  # GainType.MUSCLE, BiasType.MUSCLE
DYN_NONE, DYN_MUSCLE = 0, 4    # DynType.NONE, DynType.MUSCLE


def _sizes(m):
    return dict(nq=int(m.nq), nv=int(m.nv), nu=int(m.nu), na=int(m.na), nb=int(m.nbody), nj=int(m.njnt), nt=int(m.ntendon))


def _tails(m):
    z = _sizes(m)
    nq, nv, nu, na, nb, nt = z["nq"], z["nv"], z["nu"], z["na"], z["nb"], z["nt"]
    return dict(qpos=(nq,), qvel=(nv,), ctrl=(nu,), act=(na,), ten_length=(nt,), ten_velocity=(nt,), ten_J=(nt, nv), actuator_length=(nu,), actuator_velocity=(nu,),
                actuator_moment=(nu, nv), xipos=(nb, 3), ximat=(nb, 3, 3), subtree_com=(nb, 3), cdof=(nv, 6), cvel=(nb, 6), qfrc_gravcomp=(nv,), qfrc_applied=(nv,),
                xfrc_applied=(nb, 6), qfrc_passive=(nv,), qfrc_bias=(nv,), qfrc_actuator=(nv,), qLD=(nv, nv))


# args field: (Model field, shape with size names; None: any row length)
VALUES = dict(jnt_stiffness=("jnt_stiffness", ("nj",)), qpos_spring=("qpos_spring", ("nq",)), dof_damping=("dof_damping", ("nv",)),
              tendon_stiffness=("tendon_stiffness", ("nt",)), tendon_damping=("tendon_damping", ("nt",)), tendon_lengthspring=("tendon_lengthspring", ("nt", 2)),
              body_mass=("body_mass", ("nb",)), body_inertia=("body_inertia", ("nb", 3)), body_gravcomp=("body_gravcomp", ("nb",)),
              jnt_actgravcomp=("jnt_actgravcomp", ("nj",)), jnt_actfrcrange=("jnt_actfrcrange", ("nj", 2)), gainprm=("actuator_gainprm", ("nu", None)),
              biasprm=("actuator_biasprm", ("nu", None)), dynprm=("actuator_dynprm", ("nu", None)), ctrlrange=("actuator_ctrlrange", ("nu", 2)),
              forcerange=("actuator_forcerange", ("nu", 2)), gear=("actuator_gear", ("nu", 6)), lengthrange=("actuator_lengthrange", ("nu", 2)),
              acc0=("actuator_acc0", ("nu",)))


def plan(op, m_or_sizes, dtype) -> tuple[int, int, int]:
    """(lanes per environment, environments per workgroup, reals of LDS per environment) of one call of ``op`` (``tendon``, ``transmission``, ``velocity``, ``passive``,
    ``actuation``, ``acceleration`` or its ``MJH_DYNAMICS_*`` number) on a Model, or on a dict of sizes ``nq, nv, nu, nb, nt``: the library's own plan
    (``mjh_dynamics_plan``, a host computation).  A model one environment of which exceeds the LDS of a CU is a ``RuntimeError`` naming the sizes."""
    op = OPS[op] if isinstance(op, str) else int(op)
    z = m_or_sizes if isinstance(m_or_sizes, dict) else _sizes(m_or_sizes)
    lib = native.load_library()
    fn = getattr(lib, "mjh_dynamics_plan", None)
    if fn is None:
        raise RuntimeError(f"{native.LIB_PATH} predates tendon .. fwd_acceleration (no mjh_dynamics_plan): rebuild the library")
    out = (ctypes.c_int * 3)()
    real = 8 if dtype == torch.float64 else 4
    rc = fn(op, int(z["nq"]), int(z["nv"]), int(z["nu"]), int(z["nb"]), int(z["nt"]), real, out)
    if rc == -12:
        raise RuntimeError(f"{list(OPS)[op]}: nq = {z['nq']}, nv = {z['nv']}, nu = {z['nu']}, nbody = {z['nb']}, ntendon = {z['nt']} in {dtype} need {out[2] * real} "
                           f"bytes of LDS per environment; a CU has {160 * 1024}")
    if rc != 0:
        raise RuntimeError(f"dynamics.plan failed ({rc}): {lib.mjh_last_error().decode()}")
    return tuple(out)


def _value(name, m, arg, z, dtype, device):
    """One model value of the caller's Model on the device: (tensor, row length)."""
    field, shape = VALUES[arg]
    v = getattr(m, field) if hasattr(m, field) else getattr(m.tables.source, field)
    got = tuple(np.shape(v))
    want = tuple(z[s] if isinstance(s, str) else s for s in shape)
    if len(got) != len(want) or any(w is not None and g != w for g, w in zip(got, want)):
        raise ValueError(f"{name}: Model.{field} has shape {got}, expected {tuple('any' if w is None else w for w in want)}")
    return model_value(m, field, v, dtype, device), (got[1] if len(got) == 2 else 1)


def _vec3(name, v, what):
    v = [float(x) for x in (v.detach().cpu().reshape(-1).tolist() if isinstance(v, torch.Tensor) else np.asarray(v, dtype=np.float64).reshape(-1))]
    if len(v) != 3:
        raise ValueError(f"{name}: Model.opt.{what} has {len(v)} entries, expected 3")
    return v


def _run(name, op, m, leaves: dict, probe_leaf: str, values: tuple, outs: dict, launch: bool = True, **scalars):
    """One ``mjh_dynamics`` call: the checks in the order of ``smooth._run`` (tracing, shapes / dtype / device, the model values, the CPU refusal), then the launch.
    ``outs``: {args field: trailing shape}; returns {args field: tensor}.  ``launch=False``: a branch that computes nothing -- the outputs are zeros."""
    refuse_tracing(name, *leaves.values())
    tails = _tails(m)
    batch, dtype, device = probe(name, m, probe_leaf, leaves[probe_leaf], tails[probe_leaf])
    check_leaves(name, leaves, tails, batch, dtype, device, 3)
    z = _sizes(m)
    vals, strides = {}, {}
    for arg in values:
        vals[arg], row = _value(name, m, arg, z, dtype, device)
        if arg in ("gainprm", "biasprm", "dynprm"):
            strides[arg[:-3] + "_stride"] = row
    require_device(device)
    B = int(math.prod(batch)) if batch else 1
    if not launch:
        return {n: torch.zeros(batch + tail, dtype=dtype, device=device) for n, tail in outs.items()}
    res = {n: torch.empty(batch + tail, dtype=dtype, device=device) for n, tail in outs.items()}
    if B > 0 and any(t.numel() for t in res.values()):
        plan(op, z, dtype)
        a = native.DynamicsArgs(op=op, B=B, disableflags=int(m.opt.disableflags), **strides, **scalars)
        bind(a, dict(leaves, **vals, **res))
        call(name, m, "mjh_dynamics", a, device, dtype, what="tendon .. fwd_acceleration")
    return res


def tendon(m, d):
    """``ten_length`` and the dense ``ten_J`` of the fixed tendons from ``d.qpos``: the reference's ``smooth.tendon``; ``d`` itself for a model without tendons, zeros for a
    model whose tendons have no joint terms."""
    z = _sizes(m)
    if z["nt"] == 0:
        return d
    r = _run("tendon", TENDON, m, dict(qpos=d.qpos), "qpos", (), dict(ten_length_out=(z["nt"],), ten_J_out=(z["nt"], z["nv"])))
    return d.replace(ten_length=r["ten_length_out"], ten_J=r["ten_J_out"])


def transmission(m, d):
    """``actuator_length`` and ``actuator_moment`` from the caller's ``qpos`` (joint transmissions; ball and free joints under JOINTINPARENT rotate the gear axis by the
    inverse joint quaternion) and ``ten_length`` / ``ten_J`` (tendon transmissions), with the Model's ``actuator_gear``: the reference's ``smooth.transmission``; ``d``
    itself for a model without actuators."""
    z = _sizes(m)
    if z["nu"] == 0:
        return d
    leaves = dict(qpos=d.qpos)
    if z["nt"] > 0:
        leaves.update(ten_length=d.ten_length, ten_J=d.ten_J)
    r = _run("transmission", TRANSMISSION, m, leaves, "qpos", ("gear",), dict(actuator_length_out=(z["nu"],), actuator_moment_out=(z["nu"], z["nv"])))
    return d.replace(actuator_length=r["actuator_length_out"], actuator_moment=r["actuator_moment_out"])


def _velocity_products(m, d):
    """``actuator_velocity = actuator_moment qvel`` and, with tendons, ``ten_velocity = ten_J qvel`` (forward.py:87-95): one launch."""
    z = _sizes(m)
    leaves = dict(qvel=d.qvel, actuator_moment=d.actuator_moment)
    outs = dict(actuator_velocity_out=(z["nu"],))
    if z["nt"] > 0:
        leaves.update(ten_J=d.ten_J)
        outs.update(ten_velocity_out=(z["nt"],))
    r = _run("fwd_velocity", VELOCITY, m, leaves, "qvel", (), outs)
    if z["nv"] == 0:  # (no dofs, no launch: the products are empty sums)
        for t in r.values():
            t.zero_()
    kw = dict(actuator_velocity=r["actuator_velocity_out"])
    if z["nt"] > 0:
        kw.update(ten_velocity=r["ten_velocity_out"])
    return d.replace(**kw)


def passive(m, d):
    """``qfrc_passive`` and ``qfrc_gravcomp``: joint springs (ball and free joints by the quaternion difference), dof dampers, tendon springs with their
    ``lengthspring`` dead band, tendon dampers through ``ten_J^T``, gravity compensation (``qfrc_gravcomp`` whole, ``qfrc_passive`` gets the part
    ``1 - jnt_actgravcomp`` of it) and the inertia-box fluid model -- the reference's ``passive.passive``.  With ``DisableBit.SPRING`` or ``DAMPER`` both are zero; a
    model without gravcomp (or with GRAVITY disabled) keeps the caller's ``qfrc_gravcomp`` object."""
    z = _sizes(m)
    flags = int(m.opt.disableflags)
    leaves = dict(qpos=d.qpos, qvel=d.qvel)
    if flags & (DisableBit.SPRING | DisableBit.DAMPER):
        r = _run("passive", PASSIVE, m, leaves, "qvel", (), dict(qfrc_passive_out=(z["nv"],), qfrc_gravcomp_out=(z["nv"],)), launch=False)
        return d.replace(qfrc_passive=r["qfrc_passive_out"], qfrc_gravcomp=r["qfrc_gravcomp_out"])
    gravcomp = bool(m.has_gravcomp) and not flags & DisableBit.GRAVITY
    fluid = bool(m.opt.has_fluid_params)
    values = ["jnt_stiffness", "qpos_spring", "dof_damping"]
    outs = dict(qfrc_passive_out=(z["nv"],))
    scalars = dict(has_gravcomp=int(gravcomp), has_fluid=int(fluid))
    if z["nt"] > 0:
        leaves.update(ten_length=d.ten_length, ten_velocity=d.ten_velocity, ten_J=d.ten_J)
        values += ["tendon_stiffness", "tendon_damping", "tendon_lengthspring"]
    if gravcomp or fluid:
        leaves.update(xipos=d.xipos, subtree_com=d.subtree_com, cdof=d.cdof)
        values += ["body_mass"]
    if gravcomp:
        values += ["body_gravcomp", "jnt_actgravcomp"]
        outs.update(qfrc_gravcomp_out=(z["nv"],))
        g = _vec3("passive", m.opt.gravity, "gravity")
        scalars.update(gravity_x=g[0], gravity_y=g[1], gravity_z=g[2])
    if fluid:
        leaves.update(ximat=d.ximat, cvel=d.cvel)
        values += ["body_inertia"]
        w = _vec3("passive", m.opt.wind, "wind")
        scalars.update(wind_x=w[0], wind_y=w[1], wind_z=w[2], density=float(m.opt.density), viscosity=float(m.opt.viscosity))
    r = _run("passive", PASSIVE, m, leaves, "qvel", tuple(values), outs, **scalars)
    kw = dict(qfrc_passive=r["qfrc_passive_out"])
    if gravcomp:
        kw.update(qfrc_gravcomp=r["qfrc_gravcomp_out"])
    return d.replace(**kw)


def fwd_velocity(m, d):
    """The velocity stage: ``actuator_velocity`` and ``ten_velocity`` (the two products), then ``com_vel``, ``passive`` and ``rne`` on the result -- the reference's
    ``forward._velocity``.  It IS that sequence (one launch for the products, then the three functions' own), so it equals calling them one after the other bit for bit."""
    return rne(m, passive(m, com_vel(m, _velocity_products(m, d))))


def _types(m, field):
    v = getattr(m, field)
    return np.asarray(v.data.detach().cpu().numpy() if hasattr(v, "data") and not isinstance(v, np.ndarray) else v).astype(np.int64).reshape(-1)


def fwd_actuation(m, d):
    """``act_dot``, ``actuator_force`` and ``qfrc_actuator``: the control clamp (unless CLAMPCTRL is disabled), the activation dynamics (NONE, INTEGRATOR, FILTER,
    FILTEREXACT, MUSCLE), gain (FIXED, AFFINE, MUSCLE) times the control -- for a stateful actuator its last activation -- plus bias (NONE, AFFINE, MUSCLE), the
    force-range clamp, ``actuator_moment^T force``, ``+ qfrc_gravcomp * jnt_actgravcomp`` on gravcomp models and the per-joint ``actfrcrange`` clamp: the reference's
    ``forward._actuation``.  With ``nu == 0`` or ``DisableBit.ACTUATION``, ``act_dot`` and ``qfrc_actuator`` are zero and ``actuator_force`` stays the caller's."""
    z = _sizes(m)
    name = "fwd_actuation"
    if z["nu"] == 0 or int(m.opt.disableflags) & DisableBit.ACTUATION:
        r = _run(name, ACTUATION, m, dict(qvel=d.qvel, ctrl=d.ctrl), "qvel", (), dict(act_dot_out=(z["na"],), qfrc_actuator_out=(z["nv"],)), launch=False)
        return d.replace(act_dot=r["act_dot_out"], qfrc_actuator=r["qfrc_actuator_out"])
    gravcomp = bool(m.has_gravcomp)
    leaves = dict(ctrl=d.ctrl, actuator_length=d.actuator_length, actuator_velocity=d.actuator_velocity, actuator_moment=d.actuator_moment)
    values = ["gainprm", "biasprm", "ctrlrange", "forcerange", "lengthrange", "acc0", "jnt_actfrcrange"]
    if z["na"] > 0:
        leaves.update(act=d.act)
        values += ["dynprm"]
    if gravcomp:
        leaves.update(qfrc_gravcomp=d.qfrc_gravcomp)
        values += ["jnt_actgravcomp"]
    need = dict(gainprm=9 if (_types(m, "actuator_gaintype") == GAIN_MUSCLE).any() else 3, biasprm=9 if (_types(m, "actuator_biastype") == BIAS_MUSCLE).any() else 3,
                dynprm=3 if (_types(m, "actuator_dyntype") == DYN_MUSCLE).any() else 1)
    for arg, least in need.items():
        if arg in values:
            field = VALUES[arg][0]
            got = tuple(np.shape(getattr(m, field)))
            if len(got) == 2 and got[1] < least:
                raise ValueError(f"{name}: Model.{field} has shape {got}, expected ({z['nu']}, >= {least}) for this model's actuators")
    r = _run(name, ACTUATION, m, leaves, "ctrl", tuple(values), dict(act_dot_out=(z["na"],), actuator_force_out=(z["nu"],), qfrc_actuator_out=(z["nv"],)),
             has_gravcomp=int(gravcomp))
    return d.replace(act_dot=r["act_dot_out"], actuator_force=r["actuator_force_out"], qfrc_actuator=r["qfrc_actuator_out"])


def fwd_acceleration(m, d):
    """``qfrc_smooth = qfrc_passive - qfrc_bias + qfrc_actuator + (qfrc_applied + xfrc_accumulate)`` and ``qacc_smooth = solve_m`` of it with the caller's ``qLD``: the
    reference's ``forward._acceleration``."""
    z = _sizes(m)
    leaves = dict(qfrc_applied=d.qfrc_applied, xfrc_applied=d.xfrc_applied, xipos=d.xipos, subtree_com=d.subtree_com, cdof=d.cdof, qfrc_passive=d.qfrc_passive,
                  qfrc_bias=d.qfrc_bias, qfrc_actuator=d.qfrc_actuator, qLD=d.qLD)
    r = _run("fwd_acceleration", ACCELERATION, m, leaves, "qfrc_applied", (), dict(qfrc_smooth_out=(z["nv"],), qacc_smooth_out=(z["nv"],)))
    return d.replace(qfrc_smooth=r["qfrc_smooth_out"], qacc_smooth=r["qacc_smooth_out"])
