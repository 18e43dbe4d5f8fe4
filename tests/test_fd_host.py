"""The numpy reference of transition_fd (tests/_fd_ref.py) pinned on its own, and transition_fd's refusals (CPU).

Tolerances are derived.  Add / subtract dofs: ``(x + eps) - x`` is off ``eps`` by at most one rounding of ``x + eps``, i.e. half an ulp of the
operand, ``2^-53 max(|x|, |x + eps|)``.  Rotational dofs of ball / free joints: ``_fd_ref.QUAT_INTEGRATE_OPS`` roundings of unit-magnitude
components for the rotated quaternion, carried into the rotation vector with the factor 2 of the angle, and ``_fd_ref.QUAT_SUB_OPS`` of the
difference itself (``bound`` below).

``tests/_hostsim.py`` (the CPU stand-in of the device library) answers ``mjh_step`` / ``mjh_forward`` only, so it cannot host the two new entry
points; what runs here without a device is what transition_fd decides before it needs one: argument validation and the refusals.
"""
import numpy as np
import pytest
import torch

import _fd_ref as R
import mujoco_torch_amd as mt
from _cases import seeded_batch
from _util import load_model

U = 2.0 ** -52


def joints(mx):
    return R.Joints(mx.jnt_type.data.cpu().numpy(), np.asarray(mx.jnt_qposadr), np.asarray(mx.jnt_dofadr), int(mx.nq), int(mx.nv))


def bound(scale):
    """|difference(q, integrate(q, v, 1)) - v| allowed on a rotational dof, in units of float64 machine epsilon: the integrated quaternion's roundings
    doubled into the angle, plus the difference's own (the part relative to the rotation vector taken at ``scale`` = |v| <= pi)."""
    return (2 * R.QUAT_INTEGRATE_OPS + 2 * 7 + 6 * scale) * U


def poses(mx, n, seed):
    """n random poses: qpos0 moved along random tangents (quaternions stay unit)."""
    jt = joints(mx)
    rng = np.random.RandomState(seed)
    q0 = np.broadcast_to(mx.qpos0.cpu().numpy().astype(np.float64), (n, jt.nq))
    return jt, R.integrate(jt, q0, rng.uniform(-1, 1, (n, jt.nv)), 1.0)


@pytest.mark.parametrize("xml", ["ball_free_actuators", "humanoid"])
def test_unit_tangent_nudge_differences_back_to_eps(xml):
    mx = load_model(xml)
    jt, q = poses(mx, 16, 1)
    assert len(jt.rot_dofs) >= 3
    eps = 1e-6
    for j in range(jt.nv):
        e = np.zeros(jt.nv)
        e[j] = 1
        for s in (eps, -eps):
            got = R.difference(jt, q, R.integrate(jt, q, e, s))
            err = np.abs(got - s * e)
            if jt.axis[j] < 0:
                assert (err[:, j] <= 0.5 * U * (np.abs(q[:, jt.adr[j]]) + eps)).all(), (xml, j)
                rot = jt.axis >= 0  # nothing else moves; an untouched quaternion differences to the roundings of q^-1 q's vector part
                assert (np.delete(err, j, axis=1)[:, ~np.delete(rot, j)] == 0).all() and (err[:, rot] <= 2 * 7 * U).all(), (xml, j)
            else:
                mine = (jt.axis >= 0) & (jt.adr == jt.adr[j])  # the three dofs of this quaternion
                assert (err[:, jt.axis < 0] == 0).all() and (err[:, (jt.axis >= 0) & ~mine] <= 2 * 7 * U).all(), (xml, j)
                assert (err[:, mine] <= bound(eps)).all(), (xml, j, err.max())


@pytest.mark.parametrize("xml", ["ball_free_actuators", "humanoid"])
def test_difference_inverts_integrate(xml):
    mx = load_model(xml)
    jt, q = poses(mx, 64, 2)
    rng = np.random.RandomState(3)
    v = rng.uniform(-1, 1, (64, jt.nv))
    for qa, da in jt.quats:  # rotation vectors of every length below pi
        w = rng.randn(64, 3)
        v[:, da:da + 3] = w / np.linalg.norm(w, axis=1, keepdims=True) * rng.uniform(0, 3.1, (64, 1))
    got = R.difference(jt, q, R.integrate(jt, q, v, 1.0))
    err = np.abs(got - v)
    add = jt.axis < 0
    assert (err[:, add] <= 0.5 * U * (np.abs(q[:, jt.adr[add]]) + np.abs(v[:, add]))).all()
    # near a half turn the angle 2 atan2(s, w) has the derivative 2 / |(s, w)| = 2 in both arguments: no amplification beyond the factor in bound()
    assert (err[:, ~add] <= bound(np.pi)).all(), err[:, ~add].max()
    q1 = R.integrate(jt, q, got, 1.0)
    for qa, _ in jt.quats:  # ... and lands on the same rotation (q and -q are one rotation)
        a, b = q1[:, qa:qa + 4], R.integrate(jt, q, v, 1.0)[:, qa:qa + 4]
        assert (np.minimum(np.abs(a - b).max(1), np.abs(a + b).max(1)) <= 4 * bound(np.pi)).all()


def test_ctrl_rule_on_a_hand_made_table():
    eps = 1e-6
    #            inside   at upper  at lower  narrow range      unlimited   outside
    u = np.array([[0.25,   1.0,      -1.0,     0.25e-6,          5.0,        1.5]])
    rng_ = np.array([[-1, 1], [-1, 1], [-1, 1], [0.0, 0.5e-6], [-1, 1], [-1, 1]], dtype=np.float64)
    lim = np.array([1, 1, 1, 1, 0, 1])
    f, b = R.ctrl_sides(u, eps, lim, rng_, centered=False)
    assert f.tolist() == [[True, False, True, False, True, False]] and b.tolist() == [[False, True, False, False, False, False]]
    f, b = R.ctrl_sides(u, eps, lim, rng_, centered=True)
    assert f.tolist() == [[True, False, True, False, True, False]] and b.tolist() == [[True, True, False, False, True, False]]
    # the columns that follow: y = 3 u (one state, no joints), so that every taken difference is 3 up to the rounding of u +- eps
    jt = R.Joints([], [], [], 0, 0)
    z = np.zeros((1, 0))
    for centered in (False, True):
        P, sides = R.perturbed(jt, z, z, np.zeros((1, 1)), u, eps, centered, lim, rng_)
        y0 = dict(qpos=z, qvel=z, act=3 * u.sum(-1, keepdims=True))
        y = dict(qpos=P["qpos"], qvel=P["qvel"], act=3 * P["ctrl"].sum(-1, keepdims=True))
        A, B = R.jacobians(jt, y0, y, eps, centered, sides)
        assert A.shape == (1, 1, 1) and B.shape == (1, 1, 6) and A[0, 0, 0] == 0
        taken = (sides[0] | sides[1])[0]
        assert (B[0, 0, ~taken] == 0).all() and taken.tolist() == [True, True, True, False, True, False]
        assert np.abs(B[0, 0, taken] - 3).max() <= 8 * U * np.abs(3 * u).sum() / eps
        nside = 2 if centered else 1
        assert P["ctrl"].shape == (1, 7, nside, 6)
        assert P["ctrl"][0, 2, 0, 1] == 1.0 - eps if not centered else P["ctrl"][0, 2, 1, 1] == 1.0 - eps  # at the upper bound: the backward nudge
        assert (P["ctrl"][0, 4] == u[0]).all() and (P["ctrl"][0, 6] == u[0]).all()  # refused both ways: untouched


def test_refusals_need_no_device():
    mx, d = seeded_batch("cartpole", {}, torch.float64, 4)
    for bad in (0, 0.0, -1e-6, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="eps"):
            mt.transition_fd(mx, d, eps=bad)
    with pytest.raises(ValueError, match="eps"):
        mt.transition_fd(mx, d, eps="small")
    with pytest.raises(ValueError, match="float32.*float64|dtype"):
        mt.transition_fd(mx, d.to(torch.float32))
    mx32, d32 = seeded_batch("cartpole", {}, torch.float32, 4)
    with pytest.raises(ValueError, match="rounds to zero"):
        mt.transition_fd(mx32, d32, eps=1e-60)
    with pytest.raises(ValueError, match="max_scratch_bytes"):
        mt.transition_fd(mx, d, max_scratch_bytes=0)
    with pytest.raises(NotImplementedError, match="vmap"):
        torch.vmap(lambda q: mt.transition_fd(mx, d[0].replace(qpos=q))[0])(d.qpos)
    with pytest.raises(RuntimeError, match="HIP device"):  # (every check above comes before this one)
        mt.transition_fd(mx, d)


def test_exported_next_to_inverse():
    assert mt.transition_fd.__module__ == "mujoco_torch_amd.derivative"
    import mujoco_torch_amd.derivative as dv

    assert dv.MAX_SCRATCH_BYTES > 0
