"""The reference's integrators as a tail on a finished forward pass: ``deriv_smooth_vel`` (``_src/derivative.py:22-68``), ``implicit`` (``forward._implicit``,
``:404-416``: the implicitfast integrator) and ``euler`` (``forward._euler``, ``:313-328``), with the ``_advance`` they share (``:255-310``).  One native launch
(``mjh_integrate``, ``csrc/mjh_integrate.h``, whose header states the definitions and the order of every sum).

``device_put`` still refuses ``opt.integrator = IMPLICITFAST``: ``step`` does not run it.  Implicitfast is ``d = implicit(mx, forward(mx, d))`` on a model compiled
with the Euler integrator -- ``step`` with the integrator swapped, minus ``_check_state``: neither function here runs that check (``step`` does), so a state with a
non-finite or huge entry is advanced as it is.

``deriv_smooth_vel(m, d)`` returns ``S + (nv, nv)``, or ``None`` when no term applies: ``actuator_moment^T diag(vel) actuator_moment`` unless ``DisableBit.ACTUATION``
(``vel_i = biasprm[i, 2] [biastype AFFINE] + gainprm[i, 2] [gaintype AFFINE] * c_i``, ``c_i`` the raw ``ctrl[i]`` for a stateless actuator and
``act[actuator_actadr[i]]`` for a stateful one -- the reference's ``where(dyn_mask, act, ctrl)`` wherever that is well defined, ``na == 0`` or ``na == nu``; muscle
gains contribute nothing), ``- diag(dof_damping)`` unless ``DisableBit.DAMPER``, ``- ten_J^T diag(tendon_damping) ten_J`` whenever the model has tendons (the
reference does not put this term under the DAMPER flag).

``implicit(m, d, *, dt=None, return_qacc=False)``: ``qacc = chol_solve(qM - h qDeriv, qfrc_smooth + qfrc_constraint)`` (``d.qacc`` when ``qDeriv`` is ``None``), then
the advance: ``act`` (FILTEREXACT exactly, else ``act + h act_dot``, clamped to ``actuator_actrange`` where limited), ``qvel + h qacc``, ``qpos`` integrated with the new
``qvel``, ``time + h``.  ``euler(m, d, *, dt=None, return_qacc=False)``: ``qacc = chol_solve(qM + h diag(dof_damping), ...)`` unless ``DisableBit.EULERDAMP``
(then ``d.qacc``), then the same advance.  The factorisation is the reference's ``math.small_cholesky``: up to 16 dofs the scalar sequence with every pivot clamped
at 1e-12, above ``A + 1e-10 I``.  The result is ``d`` with exactly ``qpos``, ``qvel``, ``act`` and ``time`` replaced (fresh tensors); ``d.qacc`` stays the solver's, as
in the reference.  ``return_qacc=True`` returns ``(Data, qacc)`` with the acceleration the state was advanced with, ``S + (nv,)``.  ``dt=`` (a float or 0-d value; an
extension) is the ``h`` used in both places, default ``m.opt.timestep``: ``euler(m, forward(m, d), dt=h / n)`` is one substep of the reference's ``_adaptive``.

Both raise the reference's ``NotImplementedError`` for a model with fluid parameters unless DAMPER or SPRING is disabled, as ``deriv_smooth_vel`` does.

The model VALUES the kernel uses -- ``dof_damping``, ``actuator_gainprm`` / ``biasprm`` / ``dynprm`` / ``actrange``, ``opt.timestep``, ``opt.disableflags`` (and
``tendon_damping``, no ``Model`` field: from the compiled model the tables keep) -- are read from the caller's ``Model`` at each call, so a value-only edit such as
``mx.replace(dof_damping=...)`` takes effect without a new native model.  The structure (gain / bias / dyn types, ``actadr``, ``actlimited``, the joints) is the
compiled model's.

Every leading dimension of a leaf is the batch (S); nothing is written to the input.  The calls run on the caller's current stream.  ``torch.vmap`` /
``torch.compile``: there is no operator for these functions; they raise ``NotImplementedError``.
"""

from __future__ import annotations

import math

import numpy as np
import torch

from . import native
from ._enums import DisableBit
from ._postpass import bind, call, check_leaves, model_value, probe, refuse_tracing, require_device

QDERIV, IMPLICIT, EULER, STATE, WRITE_QDERIV, WRITE_QACC = 1, 2, 4, 8, 16, 32  # include/mjhip.h MJH_INTEGRATE_*
FLUID_MESSAGE = "fluid drag not supported for implicitfast"  # (the reference's, derivative.py:64)


def _sizes(m):
    return dict(nq=int(m.nq), nv=int(m.nv), nu=int(m.nu), na=int(m.na), nt=int(m.ntendon))


def plan(name: str, m, leaves: dict):
    """Shape, dtype and device checks of one call, as ``energy.plan``: ``leaves`` maps leaf names to tensors (``qvel`` is among them); returns (batch, dtype, device)."""
    z = _sizes(m)
    nq, nv, nu, na, nt = z["nq"], z["nv"], z["nu"], z["na"], z["nt"]
    tails = dict(qpos=(nq,), qvel=(nv,), act=(na,), act_dot=(na,), time=(), ctrl=(nu,), qacc=(nv,), qM=(nv, nv), qfrc_smooth=(nv,), qfrc_constraint=(nv,),
                 actuator_moment=(nu, nv), ten_J=(nt, nv))
    batch, dtype, device = probe(name, m, "qvel", leaves["qvel"], (nv,))
    check_leaves(name, leaves, tails, batch, dtype, device, 2)
    return batch, dtype, device


def _values(name, m, dtype, device, names):
    """The model values of one call, from the caller's Model: {argument name: (device tensor, row length)}."""
    z = _sizes(m)
    src = m.tables.source
    fields = dict(dof_damping=("dof_damping", (z["nv"],)), tendon_damping=("tendon_damping", (z["nt"],)), gainprm=("actuator_gainprm", (z["nu"], None)),
                  biasprm=("actuator_biasprm", (z["nu"], None)), dynprm=("actuator_dynprm", (z["nu"], None)), actrange=("actuator_actrange", (z["nu"], 2)))
    out = {}
    for n in names:
        field, shape = fields[n]
        v = getattr(m, field) if hasattr(m, field) else getattr(src, field)
        got = tuple(np.shape(v))
        least = {"gainprm": 3, "biasprm": 3, "dynprm": 1}.get(n)
        if len(got) != len(shape) or any(w is not None and g != w for g, w in zip(got, shape)) or (least is not None and got[1] < least):
            raise ValueError(f"{name}: Model.{field} has shape {got}, expected {tuple('>= %d' % least if w is None else w for w in shape)}")
        out[n] = (model_value(m, field, v, dtype, device), got[1] if len(got) == 2 else 1)
    return out


def _step_size(name, m, dt):
    h = m.opt.timestep if dt is None else dt
    if isinstance(h, (torch.Tensor, np.ndarray)) and int(np.prod(tuple(h.shape))) != 1:
        raise ValueError(f"{name}: dt= must be a float or a 0-d value; got shape {tuple(h.shape)}")
    try:
        h = float(h)
    except (TypeError, ValueError):
        raise ValueError(f"{name}: dt= must be a float or a 0-d value; got {type(dt).__name__}") from None
    if not math.isfinite(h):
        raise ValueError(f"{name}: dt= must be finite; got {h}")
    return h


def _terms(m):
    """(actuation, damper, tendons): the terms of qDeriv that apply to this Model (derivative.py:27, :54, :59)."""
    flags = int(m.opt.disableflags)
    return (not flags & DisableBit.ACTUATION, not flags & DisableBit.DAMPER, int(m.ntendon) > 0)


def _refuse_fluid(m):
    if not (int(m.opt.disableflags) & (DisableBit.DAMPER | DisableBit.SPRING)) and bool(m.opt.has_fluid_params):
        raise NotImplementedError(FLUID_MESSAGE)


def _launch(name, m, device, dtype, B, flags, h, tensors, values, outs):
    a = native.ARGS["mjh_integrate"](flags=flags, disableflags=int(m.opt.disableflags), B=B, h=h)
    tensors = dict(tensors, **outs)
    for n, (t, stride) in values.items():
        tensors[n] = t
        if n in ("gainprm", "biasprm", "dynprm"):
            setattr(a, n[:-3] + "_stride", stride)
    bind(a, tensors)
    call(name, m, "mjh_integrate", a, device, dtype)


def _build_leaves(m, d, actuation, tendons):
    z = _sizes(m)
    leaves = {}
    if actuation and z["nu"] > 0:
        leaves.update(ctrl=d.ctrl, actuator_moment=d.actuator_moment)
        if z["na"] > 0:
            leaves.update(act=d.act)
    if tendons:
        leaves.update(ten_J=d.ten_J)
    return leaves


def _build_values(actuation, damper, tendons, m):
    names = []
    if actuation and int(m.nu) > 0:
        names += ["gainprm", "biasprm"]
    if damper:
        names += ["dof_damping"]
    if tendons:
        names += ["tendon_damping"]
    return names


def deriv_smooth_vel(m, d):
    """The analytic derivative of the smooth forces with respect to ``qvel`` of the finished pass ``d`` holds, ``S + (nv, nv)`` (the full symmetric matrix), or
    ``None`` when no term applies (ACTUATION and DAMPER disabled, no tendons); the reference's ``derivative.deriv_smooth_vel``, its quirks included (the module
    docstring).  Raises the reference's ``NotImplementedError`` for fluid parameters unless DAMPER or SPRING is disabled."""
    name = "deriv_smooth_vel"
    refuse_tracing(name, d.qvel, d.ctrl)
    actuation, damper, tendons = _terms(m)
    leaves = dict(qvel=d.qvel, **_build_leaves(m, d, actuation, tendons))
    batch, dtype, device = plan(name, m, leaves)
    values = _values(name, m, dtype, device, _build_values(actuation, damper, tendons, m))
    if not (actuation or damper or tendons):
        return None
    _refuse_fluid(m)
    require_device(device)
    nv = int(m.nv)
    B = int(math.prod(batch)) if batch else 1
    out = torch.empty(batch + (nv, nv), dtype=dtype, device=device)
    if B == 0 or nv == 0:
        return out
    del leaves["qvel"]
    _launch(name, m, device, dtype, B, QDERIV | WRITE_QDERIV, 0.0, leaves, values, dict(qderiv_out=out))
    return out


def _integrate(name, m, d, dt, return_qacc, implicit):
    refuse_tracing(name, d.qpos, d.qvel, dt)
    h = _step_size(name, m, dt)
    z = _sizes(m)
    actuation, damper, tendons = _terms(m) if implicit else (False, False, False)
    if implicit:
        solve = actuation or damper or tendons
        value_names = _build_values(actuation, damper, tendons, m)
        flags = (QDERIV | IMPLICIT) if solve else 0
    else:
        solve = not int(m.opt.disableflags) & DisableBit.EULERDAMP
        value_names = ["dof_damping"] if solve else []
        flags = EULER if solve else 0
    leaves = dict(qpos=d.qpos, qvel=d.qvel, time=d.time, **_build_leaves(m, d, actuation, tendons))
    if z["na"] > 0:
        leaves.update(act=d.act, act_dot=d.act_dot)
        value_names += ["dynprm", "actrange"]
    if solve:
        leaves.update(qM=d.qM, qfrc_smooth=d.qfrc_smooth, qfrc_constraint=d.qfrc_constraint)
    else:
        leaves.update(qacc=d.qacc)
    batch, dtype, device = plan(name, m, leaves)
    values = _values(name, m, dtype, device, value_names)
    if implicit:
        _refuse_fluid(m)
    require_device(device)
    B = int(math.prod(batch)) if batch else 1
    new = lambda *tail: torch.empty(batch + tail, dtype=dtype, device=device)
    outs = dict(qpos_out=new(z["nq"]), qvel_out=new(z["nv"]), act_out=new(z["na"]), time_out=new())
    flags |= STATE
    if return_qacc:
        outs["qacc_out"] = new(z["nv"])
        flags |= WRITE_QACC
    if B > 0:
        _launch(name, m, device, dtype, B, flags, h, leaves, values, outs)
    out = d.replace(qpos=outs["qpos_out"], qvel=outs["qvel_out"], act=outs["act_out"], time=outs["time_out"])
    return (out, outs["qacc_out"]) if return_qacc else out


def implicit(m, d, *, dt=None, return_qacc=False):
    """One implicit-in-velocity (implicitfast) integration step of the finished pass ``d`` holds: the reference's ``forward._implicit``.  Returns ``d`` with ``qpos``,
    ``qvel``, ``act`` and ``time`` replaced; ``d.qacc`` stays the solver's.  ``dt``: the step, default ``m.opt.timestep``; ``return_qacc=True``: ``(Data, qacc)``
    with the implicit acceleration, ``S + (nv,)``.  ``implicit(m, forward(m, d))`` is ``step`` with the integrator swapped, minus ``_check_state``, which this
    function does not run."""
    return _integrate("implicit", m, d, dt, return_qacc, True)


def euler(m, d, *, dt=None, return_qacc=False):
    """One semi-implicit Euler integration step of the finished pass ``d`` holds, damping integrated implicitly unless ``DisableBit.EULERDAMP``: the reference's
    ``forward._euler``.  Arguments and result as for ``implicit``; with ``dt=`` a substep of the reference's ``_adaptive``.  ``_check_state`` is not run (``step``
    runs it)."""
    return _integrate("euler", m, d, dt, return_qacc, False)
