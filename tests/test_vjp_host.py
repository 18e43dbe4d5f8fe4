"""The numpy reference of the tangent maps (tests/_vjp_ref.py) against first principles, and the refusals of ``transition_vjp`` /
``differentiable_step`` that need no device."""
import numpy as np
import pytest
import torch

import _fd_ref as R
import _vjp_ref as V
import mujoco_torch_amd as mt
from _cases import seeded_batch

F64, F32 = torch.float64, torch.float32


def rig():
    """A free joint, a hinge, a ball joint and a slide: nq 13, nv 11."""
    return R.Joints([R.FREE, R.HINGE, R.BALL, R.SLIDE], [0, 7, 8, 12], [0, 6, 7, 10], 13, 11)


def unit_qpos(rng, jt, n, scale=None):
    q = rng.randn(n, jt.nq)
    for qa, _ in jt.quats:
        q[:, qa:qa + 4] /= np.linalg.norm(q[:, qa:qa + 4], axis=-1, keepdims=True)
        if scale is not None:
            q[:, qa:qa + 4] *= scale[:, None]
    return q


def test_pull_is_the_gradient_of_a_linear_functional_along_the_tangent():
    """L(delta) = <gq, integrate(qpos, delta, 1)>: pull(gq) against its float64 central difference at delta = 0.  With h = 1e-5 the truncation
    is h^2 / 24 |gq| (third derivative of exp(delta / 2): 1 / 8) ~ 4e-12 |gq| and the cancellation 2^-52 |gq| / h ~ 2e-11 |gq|: allowed 1e-9 |gq|."""
    rng = np.random.RandomState(0)
    jt = rig()
    qpos, gq = unit_qpos(rng, jt, 32), rng.randn(32, jt.nq)
    got = V.pull(jt, qpos, gq)
    h = 1e-5
    for k in range(jt.nv):
        e = np.zeros(jt.nv)
        e[k] = 1
        fd = ((gq * R.integrate(jt, qpos, e, h)).sum(-1) - (gq * R.integrate(jt, qpos, e, -h)).sum(-1)) / (2 * h)
        assert np.abs(got[:, k] - fd).max() <= 1e-9 * np.abs(gq).sum(-1).max(), k
    assert np.abs(got).max() > 0.5


def test_push_is_the_pseudo_inverse_of_pull():
    rng = np.random.RandomState(1)
    jt = rig()
    qpos, gt = unit_qpos(rng, jt, 32), rng.randn(32, jt.nv)
    gq = V.push(jt, qpos, gt)
    assert np.abs(V.pull(jt, qpos, gq) - gt).max() <= 32 * 2.0 ** -52 * np.abs(gt).max()
    for qa, _ in jt.quats:  # no radial component
        assert np.abs((gq[:, qa:qa + 4] * qpos[:, qa:qa + 4]).sum(-1)).max() <= 32 * 2.0 ** -52 * np.abs(gt).max()
    scaled = unit_qpos(np.random.RandomState(1), jt, 32, scale=np.linspace(0.5, 2.0, 32))  # the same rotations, other norms
    gs = V.push(jt, scaled, gt)
    assert np.abs(V.pull(jt, scaled, gs) - gt).max() <= 32 * 2.0 ** -52 * np.abs(gt).max()
    for qa, _ in jt.quats:
        assert np.abs((gs[:, qa:qa + 4] * scaled[:, qa:qa + 4]).sum(-1)).max() <= 64 * 2.0 ** -52 * np.abs(gt).max()


def test_bounds_hold_for_float32_evaluations():
    """The derived bounds of _vjp_ref against the reference itself run in float32."""
    rng = np.random.RandomState(2)
    jt = rig()
    qpos, gq, gt = unit_qpos(rng, jt, 64, scale=np.linspace(0.7, 1.4, 64)).astype(np.float32), rng.randn(64, jt.nq).astype(np.float32), rng.randn(64, jt.nv).astype(np.float32)
    u = 2.0 ** -24
    ep = np.abs(V.pull(jt, qpos, gq).astype(np.float64) - V.pull(jt, qpos.astype(np.float64), gq.astype(np.float64)))
    assert (ep <= V.pull_bound(u, jt, qpos, gq)).all() and ep.max() > 0
    es = np.abs(V.push(jt, qpos, gt).astype(np.float64) - V.push(jt, qpos.astype(np.float64), gt.astype(np.float64)))
    assert (es <= V.push_bound(u, jt, qpos, gt)).all() and es.max() > 0


def test_argument_refusals_without_a_device():
    mx, d = seeded_batch("ball_free_actuators", {}, F64, 3)
    ns, nu = 2 * int(mx.nv) + int(mx.na), int(mx.nu)
    g = torch.zeros(3, ns, dtype=F64)
    for bad in (0, -1e-6, float("inf"), "x"):
        with pytest.raises(ValueError, match="eps"):
            mt.transition_vjp(mx, d, g, eps=bad)
        with pytest.raises(ValueError, match="eps"):
            mt.differentiable_step(mx, d, eps=bad)
    with pytest.raises(ValueError, match="g_state has shape"):
        mt.transition_vjp(mx, d, torch.zeros(3, ns + 1, dtype=F64))
    with pytest.raises(ValueError, match="g_state has shape"):
        mt.transition_vjp(mx, d, torch.zeros(ns, dtype=F64))
    with pytest.raises(ValueError, match="g_sensor has shape"):
        mt.transition_vjp(mx, d, g, torch.zeros(3, 5, dtype=F64))
    with pytest.raises(ValueError, match="g_state is torch.float32"):
        mt.transition_vjp(mx, d, g.to(F32))
    with pytest.raises(ValueError, match="g_state must be a tensor"):
        mt.transition_vjp(mx, d, np.zeros((3, ns)))
    with pytest.raises(ValueError, match="float32"):  # Data / Model dtype mismatch
        mt.transition_vjp(mx, d.to(F32), g.to(F32))
    with pytest.raises(ValueError, match="float32"):
        mt.differentiable_step(mx, d.to(F32))
    with pytest.raises(ValueError, match="max_scratch_bytes"):
        mt.transition_vjp(mx, d, g, max_scratch_bytes=0)
    for name in ("qfrc_applied", "xfrc_applied", "mocap_pos"):
        leaf = getattr(d, name).clone().requires_grad_()
        with pytest.raises(ValueError, match=f"Data.{name} requires grad"):
            mt.differentiable_step(mx, d.replace(**{name: leaf}))
    # the four differentiated leaves pass the argument checks: the call gets as far as asking for a device
    ok = d.replace(qpos=d.qpos.clone().requires_grad_(), ctrl=d.ctrl.clone().requires_grad_())
    with pytest.raises(RuntimeError, match="HIP device"):
        mt.differentiable_step(mx, ok)
    with pytest.raises(RuntimeError, match="HIP device"):
        mt.transition_vjp(mx, d, g)
    assert nu > 0


def test_transition_fd_refusals_are_unchanged():
    """The shared validation keeps transition_fd's messages word for word."""
    mx, d = seeded_batch("cartpole", {}, F64, 2)
    with pytest.raises(ValueError, match="eps must be a positive finite number, got 0.0"):
        mt.transition_fd(mx, d, eps=0)
    with pytest.raises(ValueError, match="the Data is torch.float32, the Model torch.float64: transition_fd runs in the model's dtype"):
        mt.transition_fd(mx, d.to(F32))
    with pytest.raises(ValueError, match="max_scratch_bytes must be positive, got -1"):
        mt.transition_fd(mx, d, max_scratch_bytes=-1)
    with pytest.raises(RuntimeError, match="HIP device"):
        mt.transition_fd(mx, d)


def test_push_gives_zeros_for_an_all_zero_quaternion():
    rng = np.random.RandomState(3)
    jt = rig()
    qpos, gt = unit_qpos(rng, jt, 4), rng.randn(4, jt.nv)
    qpos[1, 3:7] = 0
    gq = V.push(jt, qpos, gt)
    assert np.isfinite(gq).all() and (gq[1, 3:7] == 0).all() and np.abs(gq[1, 8:12]).max() > 0
    assert (V.push_bound(2.0 ** -53, jt, qpos, gt)[1, 3:7] == 0).all() and (V.pull(jt, qpos, rng.randn(4, jt.nq))[1, 3:6] == 0).all()


def test_a_stepped_result_can_be_stepped_again():
    """sensordata of a differentiable_step result carries a graph: where the step computes sensors it does not read the incoming values and the
    leaf passes (the call gets as far as asking for a device); with sensors disabled the leaf is carried through the step and stays refused."""
    mx, d = seeded_batch("sensor_rig", {}, F64, 2)
    sens = (2.0 * d.sensordata.clone().requires_grad_())  # a non-leaf with a grad_fn, as a previous differentiable_step returns it
    assert sens.grad_fn is not None
    with pytest.raises(RuntimeError, match="HIP device"):
        mt.differentiable_step(mx, d.replace(sensordata=sens))
    off, d2 = seeded_batch("sensor_rig", {"disableflags": int(mt.DisableBit.SENSOR)}, F64, 2)
    with pytest.raises(ValueError, match="Data.sensordata requires grad"):
        mt.differentiable_step(off, d2.replace(sensordata=sens))
    plain, d3 = seeded_batch("cartpole", {}, F64, 2)  # no sensors at all: the (empty) leaf is not let through either
    with pytest.raises(RuntimeError, match="HIP device"):
        mt.differentiable_step(plain, d3)


def test_inside_a_fullgraph_compile_the_call_is_refused():
    """What is guaranteed under torch.compile: the call is kept out of Dynamo's graphs, so with fullgraph=True the tracer reports it as
    unsupported; without fullgraph it breaks the graph and runs the call eagerly (here: as far as asking for a device; tests/test_vjp.py has the
    same on the device)."""
    mx, d = seeded_batch("cartpole", {}, F64, 2)
    g = torch.zeros(2, 4, dtype=F64)
    f = torch.compile(lambda q: mt.transition_vjp(mx, d.replace(qpos=q), g)[0], fullgraph=True)
    with pytest.raises(Exception) as info:
        f(d.qpos)
    assert type(info.value).__name__ == "Unsupported", repr(info.value)
    with pytest.raises(RuntimeError, match="HIP device"):
        torch.compile(lambda q: mt.transition_vjp(mx, d.replace(qpos=q), g)[0])(d.qpos)
