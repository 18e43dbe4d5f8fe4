"""The configuration arithmetic on the GPU (mjh_qpos_arith_kernel, csrc/mjh_qpos.h) against the numpy longdouble reference tests/_qpos_ref.py, which
tests/test_qpos_host.py pins on the recorded steps and on closed forms; and against the two things it must agree with: the step's own position update and the
coordinates of ``transition_fd``.

The bound is the project's pre-solver tolerance TOL_PRE[dtype] times max(1, the largest magnitude of the environment's reference output); the reference is
evaluated on the same (rounded) inputs as the kernel.
"""
import numpy as np
import pytest
import torch

import _qpos_ref as qr
import mujoco_torch_amd as mt
from _cases import F32, F64, TOL_PRE, TOL_SOL
from _util import load_model

pytestmark = pytest.mark.gpu

DEV = "cuda"
LD = qr.LD
DTYPES = [pytest.param(F64, id="f64"), pytest.param(F32, id="f32")]
B = 70  # one wave holds the tail of one environment's joints and the head of the next (10 and 22 joints per environment)
ANGLES = [0.0, 1e-9, np.pi - 1e-3, np.pi + 1e-3, 3.0, 0.5]  # of the rotation between qpos1 and qpos2, by environment (e % 6)
_MODELS = {}


def model(xml, dtype):
    if (xml, dtype) not in _MODELS:
        mx = load_model(xml, dtype=dtype)
        _MODELS[xml, dtype] = (mx, mx.to(DEV), qr.joints(mx))
    return _MODELS[xml, dtype]


def states(J, dtype, seed):
    """(qpos1, qvel, qpos2) [B, ...] numpy float64 holding values of the dtype: qpos1 seeded with unit quaternions, qvel seeded with the rotational part of
    environment e of length ANGLES[e % 6], qpos2 = qpos1 (+) qvel (rounded to the dtype; where the angle is 0, qpos2's quaternions are qpos1's, bit for bit)."""
    rng = np.random.RandomState(seed)
    rows, nq, nv = J
    rnd = lambda a: np.asarray(torch.tensor(np.asarray(a, dtype=np.float64)).to(dtype).double().numpy())
    q1 = rnd(qr.normalize_quat(J, rng.randn(B, nq)))
    v = rng.randn(B, nv)
    for t, qa, da in rows:
        if t in (qr.FREE, qr.BALL):
            k = da + (3 if t == qr.FREE else 0)
            axis = rng.randn(B, 3)
            v[:, k:k + 3] = axis / np.linalg.norm(axis, axis=-1, keepdims=True) * np.array([ANGLES[e % 6] for e in range(B)])[:, None]
    v = rnd(v)
    q2 = rnd(qr.integrate_pos(J, q1, v, 1.0))
    for t, qa, da in rows:
        if t in (qr.FREE, qr.BALL):
            k = qa + (3 if t == qr.FREE else 0)
            zero = np.array([ANGLES[e % 6] == 0.0 for e in range(B)])
            q2[zero, k:k + 4] = q1[zero, k:k + 4]
    return q1, v, q2


def worst_share(got, want, dtype):
    want = np.asarray(want, dtype=LD)
    scale = np.maximum(1, np.abs(want).max(-1, keepdims=True))
    assert np.isfinite(got).all()
    return float((np.abs(got.astype(LD) - want) / (TOL_PRE[dtype] * scale)).max())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("xml", ["ik_arm", "humanoid"])
def test_the_three_operations_against_the_reference(xml, dtype):
    mx, mdev, J = model(xml, dtype)
    q1, v, q2 = states(J, dtype, seed=7)
    dev = lambda a: torch.tensor(a).to(dtype).to(DEV)
    shares = {}
    for dt in (1.0, 0.002):
        got = mt.integrate_pos(mdev, dev(q1), dev(v), dt).cpu().numpy()
        shares[f"integrate dt={dt}"] = worst_share(got, qr.integrate_pos(J, q1, v, dt), dtype)
        for k in qr.quat_slices(J):
            assert np.abs(np.linalg.norm(got[:, k:k + 4].astype(np.float64), axis=-1) - 1).max() <= TOL_PRE[dtype]
        got = mt.differentiate_pos(mdev, dev(q1), dev(q2), dt).cpu().numpy()
        shares[f"differentiate dt={dt}"] = worst_share(got, qr.differentiate_pos(J, q1, q2, dt), dtype)
    # the round trip: qpos1 (+) (qpos2 (-) qpos1) is qpos2 as a configuration
    back = mt.integrate_pos(mdev, dev(q1), mt.differentiate_pos(mdev, dev(q1), dev(q2), 0.5), 0.5).cpu().numpy().astype(np.float64)
    for k in qr.quat_slices(J):
        sign = np.sign((back[:, k:k + 4] * q2[:, k:k + 4]).sum(-1, keepdims=True))
        back[:, k:k + 4] *= sign
    shares["round trip"] = worst_share(back, q2, dtype)
    # normalize_quat: non-unit quaternions, all zeros in environment 3, below 1e-15 in environment 4; everything else bit for bit
    raw = q1 * np.random.RandomState(8).uniform(0.1, 10.0, (B, 1))
    for k in qr.quat_slices(J):
        raw[3, k:k + 4] = 0
        raw[4, k:k + 4] = [0, 3e-16, -4e-16, 0]
    raw = torch.tensor(raw).to(dtype)
    got = mt.normalize_quat(mdev, raw.to(DEV)).cpu()
    want = qr.normalize_quat(J, raw.double().numpy())
    shares["normalize"] = worst_share(got.numpy(), want, dtype)
    rest = np.ones(J[1], dtype=bool)
    for k in qr.quat_slices(J):
        rest[k:k + 4] = False
        assert got[3, k:k + 4].tolist() == [1, 0, 0, 0] and got[4, k:k + 4].tolist() == [1, 0, 0, 0]
    assert torch.equal(got[:, rest], raw[:, rest])
    print(f"{xml} {dtype}: worst error over bound {({k: f'{s:.2e}' for k, s in shares.items()})}")
    assert max(shares.values()) <= 1, shares


@pytest.mark.parametrize("dtype", DTYPES)
def test_batch_shapes_views_and_an_empty_batch(dtype):
    mx, mdev, J = model("ik_arm", dtype)
    q1, v, q2 = states(J, dtype, seed=9)
    dev = lambda a: torch.tensor(a).to(dtype).to(DEV)
    flat = mt.integrate_pos(mdev, dev(q1), dev(v), 0.1)
    assert torch.equal(mt.integrate_pos(mdev, dev(q1).reshape(7, 10, -1), dev(v).reshape(7, 10, -1), 0.1).reshape(B, -1), flat)
    assert torch.equal(mt.integrate_pos(mdev, dev(q1)[5], dev(v)[5], 0.1), flat[5])
    wide = torch.zeros(B, 2 * J[1], dtype=dtype, device=DEV)
    wide[:, ::2] = dev(q1)
    assert torch.equal(mt.integrate_pos(mdev, wide[:, ::2], dev(v), 0.1), flat)  # (a non-contiguous view)
    assert tuple(mt.differentiate_pos(mdev, dev(q1)[:0], dev(q2)[:0]).shape) == (0, J[2])
    x1, x2 = torch.cat([dev(q1), dev(v)], -1), torch.cat([dev(q2), 2 * dev(v)], -1)
    dx = mt.state_sub(mdev, x2, x1)
    assert torch.equal(dx[:, :J[2]], mt.differentiate_pos(mdev, dev(q1), dev(q2))) and torch.equal(dx[:, J[2]:], dev(v))
    assert torch.equal(mt.state_add(mdev, x1, dx)[:, :J[1]], mt.integrate_pos(mdev, dev(q1), dx[:, :J[2]], 1.0))


@pytest.mark.parametrize("dtype", DTYPES)
def test_integrate_pos_agrees_with_the_step(dtype):
    """An Euler model: integrate_pos(qpos before, qvel after, timestep) against the step's own qpos after, at TOL_PRE max(1, |q|).  (Whether the two are
    bit-identical is printed, not asserted: DESIGN.md reports it.)"""
    mx, mdev, J = model("humanoid", dtype)
    assert int(mx.opt.integrator) == 0
    rng = np.random.RandomState(10)
    d0 = mt.make_data(mx)
    d0 = (d0 if dtype == F64 else d0.to(dtype)).expand(B).clone()
    d0 = d0.replace(qvel=torch.tensor(0.5 * rng.randn(B, J[2])).to(dtype)).to(DEV)
    d1 = mt.step(mdev, d0)
    got = mt.integrate_pos(mdev, d0.qpos, d1.qvel, float(mx.opt.timestep))
    same = torch.equal(got, d1.qpos)
    err = ((got - d1.qpos).abs() / d1.qpos.abs().clamp(min=1)).max().item()
    print(f"{dtype}: integrate_pos against the step's qpos: worst {err:.2e} (bound {TOL_PRE[dtype]:g}), bit-identical: {same}")
    assert err <= TOL_PRE[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("xml", ["humanoid", "muscle_arm"])
def test_state_arithmetic_agrees_with_transition_fd(xml, dtype):
    """fixed_iterations=True, no contact: a state of the humanoid lifted 1 m, its root quaternion the identity (na = 0: columns over the qpos block -- a free
    translation, the three free rotations, hinges -- and the qvel block), and a state of the muscle arm with activations inside (0, 1) (nv = 2, na = 3: every
    column of the qpos, qvel and act blocks).  state_sub(step(state_add(x, eps e_i)), step(x)) / eps against column i of transition_fd(eps=1e-6,
    centered=False), at TOL_SOL max(1, |column|)."""
    mx, mdev, J = model(xml, dtype)
    nq, nv, na, eps, nb = J[1], J[2], int(mx.na), 1e-6, 2
    ns = 2 * nv + na
    rng = np.random.RandomState(11)
    q = np.broadcast_to(mx.qpos0.numpy().astype(np.float64), (nb, nq)).copy()
    if xml == "humanoid":
        assert na == 0
        q[:, 2] += 1.0
        q[:, 7:] += 0.1 * rng.randn(nb, nq - 7)
        cols = (0, 3, 4, 5, 6, 13, nv - 1, nv + 2, nv + 4, nv + 9, 2 * nv - 1)
    else:
        assert na == 3 and len(mx.tables.pairs) == 0
        q += 0.1 * rng.randn(nb, nq)
        cols = tuple(range(ns))
    d = mt.make_data(mx)
    d = (d if dtype == F64 else d.to(dtype)).expand(nb).clone()
    d = d.replace(qpos=torch.tensor(q).to(dtype), qvel=torch.tensor(0.1 * rng.randn(nb, nv)).to(dtype))
    if na:
        d = d.replace(act=torch.tensor(rng.uniform(0.2, 0.6, (nb, na))).to(dtype), ctrl=torch.tensor(rng.uniform(0.2, 0.6, (nb, int(mx.nu)))).to(dtype))
    d = d.to(DEV)
    A, _ = mt.transition_fd(mdev, d, eps=eps, centered=False, fixed_iterations=True)
    state = lambda dd: torch.cat([dd.qpos, dd.qvel, dd.act], -1)
    x = state(d)
    y0 = state(mt.step(mdev, d, fixed_iterations=True))
    worst = {}
    for i in cols:
        dx = torch.zeros(nb, ns, dtype=dtype, device=DEV)
        dx[:, i] = eps
        xp = mt.state_add(mdev, x, dx)
        dp = d.replace(qpos=xp[:, :nq].contiguous(), qvel=xp[:, nq:nq + nv].contiguous(), act=xp[:, nq + nv:].contiguous())
        col = mt.state_sub(mdev, state(mt.step(mdev, dp, fixed_iterations=True)), y0) / eps
        want = A[:, :, i]
        worst[i] = ((col - want).abs().amax(-1) / want.abs().amax(-1).clamp(min=1)).max().item()
        assert torch.isfinite(col).all() and want.abs().max() > 0
    print(f"{xml} {dtype}: state_sub(step(state_add(x, eps e_i)), step(x)) / eps against transition_fd, error over max(1, |column|) by column: "
          f"{({i: f'{w:.1e}' for i, w in worst.items()})} (bound {TOL_SOL[dtype]:g})")
    assert max(worst.values()) <= TOL_SOL[dtype], worst
