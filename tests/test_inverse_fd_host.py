"""The numpy reference of inverse_fd (tests/_ifd_ref.py) pinned on its own, and inverse_fd's refusals (CPU).

Tolerances are derived, with ``u = 2^-53`` (half an ulp of 1 in float64).

* A ``qvel`` / ``qacc`` nudge: ``(x + s) - x`` is off ``s`` by at most one rounding of ``x + s``, ``u max(|x|, |x + s|) <= u (|x| + eps)`` (the
  subtraction of two numbers that close is exact).  The ``qpos`` columns are ``_fd_ref.integrate``, which tests/test_fd_host.py pins.
* The affine function of ``test_reference_recovers_the_matrices_of_an_affine_function``: see its docstring.

``tests/_hostsim.py`` answers ``mjh_step`` / ``mjh_forward`` only, so it cannot host the two new entry points; what runs here without a device is
what inverse_fd decides before it needs one: argument validation and the refusals.
"""
import os
import re

import numpy as np
import pytest
import torch

import _fd_ref as R
import _ifd_ref as I
import mujoco_torch_amd as mt
from _cases import seeded_batch
from _util import load_model
from mujoco_torch_amd import native

u = 2.0 ** -53
F64 = torch.float64
INVERSE_FD = mt.inverse_fd  # (everything here belongs to the feature: without it the module does not import)


def joints(mx):
    return R.Joints(mx.jnt_type.data.cpu().numpy(), np.asarray(mx.jnt_qposadr), np.asarray(mx.jnt_dofadr), int(mx.nq), int(mx.nv))


@pytest.mark.parametrize("centered", [False, True], ids=["one-sided", "centered"])
@pytest.mark.parametrize("xml", ["ball_free_actuators", "humanoid"])
def test_nudges_difference_back_to_eps(xml, centered):
    mx = load_model(xml)
    jt = joints(mx)
    nv, B, eps = jt.nv, 8, 1e-6
    rng = np.random.RandomState(1)
    q0 = np.broadcast_to(mx.qpos0.cpu().numpy().astype(np.float64), (B, jt.nq))
    qpos = R.integrate(jt, q0, rng.uniform(-1, 1, (B, nv)), 1.0)
    qvel, qacc = rng.randn(B, nv), 3.0 * rng.randn(B, nv)
    P = I.perturbed(jt, qpos, qvel, qacc, eps, centered)
    nside = 2 if centered else 1
    assert P["qpos"].shape == (B, 3 * nv, nside, jt.nq) and P["qvel"].shape == P["qacc"].shape == (B, 3 * nv, nside, nv)
    assert len(jt.rot_dofs) >= 3
    for side in range(nside):
        s = -eps if side else eps
        for j in range(nv):
            e = np.zeros(nv)
            e[j] = 1
            assert (P["qpos"][:, j, side] == R.integrate(jt, qpos, e, s)).all()  # the pinned integrate, called once per column
            assert (P["qvel"][:, j, side] == qvel).all() and (P["qacc"][:, j, side] == qacc).all()
            for k, (name, x) in enumerate((("qvel", qvel), ("qacc", qacc)), start=1):
                col = P[name][:, k * nv + j, side]
                assert (np.abs((col[:, j] - x[:, j]) - s) <= u * (np.abs(x[:, j]) + eps)).all(), (name, j, side)
                assert (np.delete(col, j, axis=1) == np.delete(x, j, axis=1)).all()  # nothing else moves
                other = "qacc" if name == "qvel" else "qvel"
                assert (P["qpos"][:, k * nv + j, side] == qpos).all() and (P[other][:, k * nv + j, side] == (qacc if name == "qvel" else qvel)).all()


@pytest.mark.parametrize("centered", [False, True], ids=["one-sided", "centered"])
def test_reference_recovers_the_matrices_of_an_affine_function(centered):
    """``f(q, v, a) = c + Aq q + Av v + Aa a`` on slide joints (``nq = nv = n``, the tangent space is ``qpos`` itself), rows ``[f; g]`` with ``g``
    a second affine function standing in for sensordata.  A finite difference of an affine function has no truncation error, so what separates
    the reference's Jacobian from the matrix is rounding alone:

    * one evaluation sums ``m = 3 n + 1`` terms (each product rounded once, at most ``m - 1`` additions whatever their order):
      ``|fl(f_i) - f_i| <= gamma_m T_i``, ``gamma_m = m u / (1 - m u)``, ``T_i = |c_i| + sum |A_ik| |x_k|`` (at the perturbed inputs, bounded with
      ``|x_k| + eps``);
    * the two evaluations of a difference contribute ``2 gamma_m T_i / eps`` one-sided and ``2 gamma_m T_i / (2 eps)`` centered;
    * the nudged operand ``x_j +- eps`` is off by ``u (|x_j| + eps)``, which the function carries with ``|A_ij|``: one nudge over ``eps``
      one-sided, two over ``2 eps`` centered -- ``u (|x_j| + eps) |A_ij| / eps`` either way;
    * the subtraction and the division add ``2 u`` relative to the entry (bounded with ``|A_ij|`` plus the above).
    """
    n, nsd, B, eps = 5, 3, 6, 1e-6
    jt = R.Joints([R.SLIDE] * n, np.arange(n), np.arange(n), n, n)
    rng = np.random.RandomState(7)
    A = rng.randn(3, n + nsd, n) * np.array([1.0, 10.0, 100.0])[:, None, None]
    c = rng.randn(n + nsd)
    x = [rng.randn(B, n), 2.0 * rng.randn(B, n), 5.0 * rng.randn(B, n)]
    fn = lambda q, v, a: c + np.einsum("ik,...k->...i", A[0], q) + np.einsum("ik,...k->...i", A[1], v) + np.einsum("ik,...k->...i", A[2], a)
    P = I.perturbed(jt, *x, eps, centered)
    y0, y = fn(*x), fn(P["qpos"], P["qvel"], P["qacc"])
    got = I.jacobians(n, y0[:, :n], y[..., :n], eps, centered, y0[:, n:], y[..., n:])
    assert [g.shape for g in got] == [(B, n, n)] * 3 + [(B, nsd, n)] * 3
    m = 3 * n + 1
    gamma = m * u / (1 - m * u)
    T = np.abs(c) + sum(np.einsum("ik,bk->bi", np.abs(A[k]), np.abs(x[k]) + eps) for k in range(3))  # [B, rows]
    worst = 0.0
    for k in range(3):
        for rows, g in ((slice(0, n), got[k]), (slice(n, n + nsd), got[3 + k])):
            want = np.broadcast_to(A[k][rows], g.shape)
            nudge = u * (np.abs(x[k])[:, None, :] + eps) * np.abs(want) / eps
            evals = 2 * gamma * T[:, rows, None] / ((2 if centered else 1) * eps)
            bound = (evals + nudge) * (1 + 2 * u) + 2 * u * np.abs(want)
            err = np.abs(g - want)
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), (k, float((err / bound).max()))
            assert np.abs(want).max() > 0.5
    print(f"affine function, centered={centered}: worst deviation / bound {worst:.3e}")
    three = I.jacobians(n, y0[:, :n], y[..., :n], eps, centered)
    assert len(three) == 3 and all((a == b).all() for a, b in zip(three, got))


def test_refusals_need_no_device():
    mx, d = seeded_batch("cartpole", {}, F64, 4)
    for bad in (0, 0.0, -1e-6, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="eps"):
            mt.inverse_fd(mx, d, eps=bad)
    with pytest.raises(ValueError, match="eps"):
        mt.inverse_fd(mx, d, eps="small")
    with pytest.raises(ValueError, match="float32.*float64|dtype"):
        mt.inverse_fd(mx, d.to(torch.float32))
    mx32, d32 = seeded_batch("cartpole", {}, torch.float32, 4)
    with pytest.raises(ValueError, match="rounds to zero"):
        mt.inverse_fd(mx32, d32, eps=1e-60)
    with pytest.raises(ValueError, match="max_scratch_bytes"):
        mt.inverse_fd(mx, d, max_scratch_bytes=0)
    with pytest.raises(NotImplementedError, match="vmap"):
        torch.vmap(lambda q: mt.inverse_fd(mx, d[0].replace(qpos=q))[0])(d.qpos)
    with pytest.raises(RuntimeError, match="HIP device"):  # (every check above comes before this one)
        mt.inverse_fd(mx, d)
    with pytest.raises(RuntimeError, match="HIP device"):
        mt.inverse_fd(mx, d, 1e-6, True, sensors=True)
    with pytest.raises(TypeError):  # sensors and max_scratch_bytes are keyword-only
        mt.inverse_fd(mx, d, 1e-6, False, True)


def test_inside_a_fullgraph_compile_the_call_is_refused():
    """Kept out of Dynamo's graphs like transition_vjp: refused as unsupported under fullgraph=True, run eagerly behind a graph break without."""
    mx, d = seeded_batch("cartpole", {}, F64, 2)
    f = torch.compile(lambda q: mt.inverse_fd(mx, d.replace(qpos=q))[0], fullgraph=True)
    with pytest.raises(Exception) as info:
        f(d.qpos)
    assert type(info.value).__name__ == "Unsupported", repr(info.value)
    with pytest.raises(RuntimeError, match="HIP device"):
        torch.compile(lambda q: mt.inverse_fd(mx, d.replace(qpos=q))[0])(d.qpos)


def test_exported_and_declared():
    import mujoco_torch_amd.derivative as dv

    assert mt.inverse_fd.__module__ == "mujoco_torch_amd.derivative" and "inverse_fd" in dv.__doc__ and "inverse_fd" in mt.__doc__
    assert set(dv._INVERSE_INPUT_LEAVES) == set(dv._INPUT_LEAVES) | {"qacc", "qfrc_actuator"}
    text = open(native.HEADER).read()
    assert re.search(r"#define MJH_KERNEL_IFD_PERTURB 45\b", text) and re.search(r"#define MJH_KERNEL_IFD_DIFFERENCE 46\b", text)
    assert "int mjh_ifd_perturb(" in text and "int mjh_ifd_difference(" in text
    lib = native.load_library()
    assert hasattr(lib, "mjh_ifd_perturb") and hasattr(lib, "mjh_ifd_difference")
    usage = open(os.path.join(os.path.dirname(native.LIB_PATH), "resource_usage.txt")).read().splitlines()
    mine = [ln for ln in usage if "mjh_ifd_" in ln]
    assert len(mine) == 4 and all("ScratchSize [bytes/lane]: 0" in ln for ln in mine)
