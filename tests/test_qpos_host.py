"""``integrate_pos`` / ``differentiate_pos`` / ``normalize_quat`` / ``state_sub`` / ``state_add`` without a GPU: the longdouble reference (tests/_qpos_ref.py) pinned
on the recorded steps and on closed forms, and the host API driven on a CPU stand-in of ``mjh_qpos_arith`` that evaluates that reference on the host pointers it
is handed.  tests/test_qpos.py runs the kernel."""
import ctypes
import re

import numpy as np
import pytest
import torch

import _hostsim
import _qpos_ref as qr
import mujoco_torch_amd as mt
from _cases import F32, F64, TOL_PRE
from _util import Golden, load_model
from mujoco_torch_amd import native

LD = qr.LD


# ---- 1. the reference -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["humanoid_cg_f64", "humanoid_newton_f64", "ant_euler_cg_ell_f64", "ant_euler_newton_pyr_f64"])
def test_the_reference_reproduces_the_recorded_euler_steps(case):
    """Euler models with a free joint: integrate(qpos before, qvel after, timestep) == the recorded qpos after, within TOL_PRE max(1, |q|), every environment
    and step."""
    g = Golden(case)
    assert int(g.model.opt.integrator) == 0 and 0 in qr.joints(g.model)[0][0]
    J, h = qr.joints(g.model), float(g.model.opt.timestep)
    worst = 0.0
    for e in range(g.nenv):
        q = g.z[f"in/{e}/qpos"]
        for s in range(g.nsteps):
            want = g.expected(e, s, "qpos")
            got = qr.integrate_pos(J, q, g.expected(e, s, "qvel"), h)
            err = np.abs(got - want) / np.maximum(1, np.abs(want))
            worst = max(worst, float(err.max()))
            q = want
    print(f"{case}: worst {worst:.2e} = {worst / TOL_PRE[g.dtype]:.2e} of TOL_PRE")
    assert worst <= TOL_PRE[g.dtype]


def _axis_angle(axis, angle):
    axis = np.asarray(axis, dtype=LD) / np.sqrt((np.asarray(axis, dtype=LD) ** 2).sum())
    return np.concatenate([[np.cos(LD(angle) / 2)], axis * np.sin(LD(angle) / 2)])


BALL_ONLY = ([(qr.BALL, 0, 0)], 4, 3)


def test_differentiate_pos_on_closed_forms():
    ident = np.array([1, 0, 0, 0], dtype=LD)
    axis = np.array([1, 2, -2], dtype=LD) / 3
    # a known angle about a known axis, from the identity and from another rotation (the difference is in the frame of q1: q2 = q1 * r)
    r = _axis_angle(axis, 0.7)
    assert np.abs(qr.differentiate_pos(BALL_ONLY, ident, r) - axis * LD(0.7)).max() < 1e-17
    q1 = _axis_angle([0.3, -1, 0.5], 1.9)
    assert np.abs(qr.differentiate_pos(BALL_ONLY, q1, qr.quat_mul(q1, r), 0.5) - axis * LD(0.7) / LD(0.5)).max() < 1e-17
    # either side of the wrap: pi - 1e-3 stays, pi + 1e-3 comes back as -(pi - 1e-3) about the same axis
    for ang, want in ((qr.PI - LD(1e-3), qr.PI - LD(1e-3)), (qr.PI + LD(1e-3), -(qr.PI - LD(1e-3)))):
        got = qr.differentiate_pos(BALL_ONLY, ident, _axis_angle(axis, ang))
        assert np.abs(got - axis * want).max() < 1e-17, (float(ang), got)
    # identical quaternions: exactly zero
    assert (qr.differentiate_pos(BALL_ONLY, q1, q1) == 0).all()
    many = np.random.RandomState(1).randn(200, 4)
    assert (qr.differentiate_pos(BALL_ONLY, many, many, 0.1) == 0).all() and (qr.differentiate_pos(BALL_ONLY, many, -many) == 0).all()
    # scalars and positions
    J = ([(qr.FREE, 0, 0), (3, 7, 6)], 8, 7)
    a, b = np.array([1, 2, 3, 1, 0, 0, 0, 0.5], dtype=LD), np.array([2, 0, 3.5, 1, 0, 0, 0, -0.25], dtype=LD)
    assert np.array_equal(qr.differentiate_pos(J, a, b, 0.5), np.array([2, -4, 1, 0, 0, 0, -1.5], dtype=LD))


def test_differentiate_then_integrate_is_a_round_trip_as_rotations():
    rng = np.random.RandomState(3)
    mx = load_model("ik_arm")
    J = qr.joints(mx)
    q1, q2 = (qr.normalize_quat(J, rng.randn(50, J[1])) for _ in range(2))
    for dt in (1.0, 0.01):
        back = qr.integrate_pos(J, q1, qr.differentiate_pos(J, q1, q2, dt), dt)
        quats = qr.quat_slices(J)
        assert len(quats) == 2
        for k in quats:
            assert np.abs(np.abs((back[:, k:k + 4] * q2[:, k:k + 4]).sum(-1)) - 1).max() < 1e-17
        rest = np.ones(J[1], dtype=bool)
        for k in quats:
            rest[k:k + 4] = False
        assert np.abs(back[:, rest] - q2[:, rest]).max() < 1e-17


def test_normalize_quat_reference():
    mx = load_model("ik_arm")
    J = qr.joints(mx)
    q = np.arange(1, J[1] + 1, dtype=LD)
    q[8:12] = 0                   # the wrist: all zeros
    q[15:19] = [0, 3e-16, 4e-16, 0]  # the probe: norm 5e-16 < 1e-15
    out = qr.normalize_quat(J, q)
    assert np.array_equal(out[:8], q[:8]) and np.array_equal(out[12:15], q[12:15])
    assert out[8:12].tolist() == [1, 0, 0, 0] and out[15:19].tolist() == [1, 0, 0, 0]
    q[15:19] = [0, 3, 4, 0]
    assert np.abs(qr.normalize_quat(J, q)[15:19] - np.array([0, 3, 4, 0], dtype=LD) / 5).max() < 1e-18


# ---- 2. the host API on a stand-in -----------------------------------------------------------------------------------------------------------------

class StandIn:
    """``mjh_qpos_arith`` of the CPU stand-in library: the numpy reference on the host pointers it is handed."""

    def __init__(self):
        self.calls = []

    def install(self, monkeypatch):
        _hostsim.install(monkeypatch)
        monkeypatch.setattr(_hostsim._Lib, "mjh_qpos_arith", self, raising=False)
        return self

    def __get__(self, lib, owner=None):
        return lambda *args: self.run(lib, *args)

    def run(self, lib, handle, op, a, b, dt, out, B, stream):
        d = lib.o.desc
        nq, nv, nj = int(d.nq), int(d.nv), int(d.njnt)
        ct, npdt = (ctypes.c_double, np.float64) if lib.o.dt == 0 else (ctypes.c_float, np.float32)
        view = lambda p, n, c=ct: np.ctypeslib.as_array((c * n).from_address(p.value))
        ints = lambda p: np.ctypeslib.as_array((ctypes.c_int32 * nj).from_address(p)).tolist()
        J = (list(zip(ints(d.jnt_type), ints(d.jnt_qposadr), ints(d.jnt_dofadr))), nq, nv)
        self.calls.append(dict(op=op, B=B, dt=dt.value))
        qa = view(a, B * nq).reshape(B, nq)
        if op == 0:
            view(out, B * nq)[:] = qr.integrate_pos(J, qa, view(b, B * nv).reshape(B, nv), dt.value).astype(npdt).reshape(-1)
        elif op == 1:
            view(out, B * nv)[:] = qr.differentiate_pos(J, qa, view(b, B * nq).reshape(B, nq), dt.value).astype(npdt).reshape(-1)
        else:
            assert b.value is None
            view(out, B * nq)[:] = qr.normalize_quat(J, qa).astype(npdt).reshape(-1)
        return 0


@pytest.fixture
def stand_in(monkeypatch):
    return StandIn().install(monkeypatch)


@pytest.fixture(scope="module")
def models():
    return {F64: load_model("ik_arm"), F32: load_model("ik_arm", dtype=F32)}


def test_the_functions_and_the_entry_point_are_public():
    for n in ("integrate_pos", "differentiate_pos", "normalize_quat", "state_sub", "state_add"):
        assert callable(getattr(mt, n)), n
    assert native.ABI_VERSION >= 22
    text = open(native.HEADER).read()
    assert re.search(r"\bint mjh_qpos_arith\s*\(const mjhModel\* m, int op, const void\* a, const void\* b, double dt, void\* out, int64_t B, void\* hip_stream\);", text)
    assert re.search(r"#define MJH_KERNEL_QPOS_ARITH 48\b", text)
    for i, n in enumerate(("INTEGRATE", "DIFFERENTIATE", "NORMALIZE")):
        assert re.search(rf"#define MJH_QPOS_{n} {i}\b", text)
    assert len(native.ARGS) == 6 and "mjh_qpos_arith" not in native.ARGS
    assert "state_sub" in mt.transition_fd.__doc__ and "state_add" in mt.transition_fd.__doc__


def test_the_fixture_has_what_it_is_meant_to_have(models):
    mx = models[F64]
    types = [t for t, _, _ in qr.joints(mx)[0]]
    assert types.count(3) >= 7 and types.count(2) == 1 and types.count(qr.BALL) == 1 and types.count(qr.FREE) == 1
    assert int(mx.nsite) == 2 and len(mx.tables.pairs) == 0 and (int(mx.nq), int(mx.nv), int(mx.na)) == (19, 17, 0)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("batch", [(), (3,), (2, 3)], ids=["unbatched", "b3", "b2x3"])
def test_shapes_dtypes_and_values(stand_in, models, batch, dtype):
    mx = models[dtype]
    J = qr.joints(mx)
    rng = np.random.RandomState(4)
    q1, q2 = (torch.tensor(qr.normalize_quat(J, rng.randn(*batch, J[1])).astype(np.float64)).to(dtype) for _ in range(2))
    v = torch.tensor(rng.randn(*batch, J[2])).to(dtype)
    npdt = q1.numpy().dtype
    out = mt.integrate_pos(mx, q1, v, 0.01)
    assert tuple(out.shape) == batch + (J[1],) and out.dtype == dtype
    assert np.array_equal(out.numpy(), qr.integrate_pos(J, q1.numpy(), v.numpy(), 0.01).astype(npdt))
    assert torch.equal(mt.integrate_pos(mx, q1, v, torch.tensor(0.01, dtype=F64)), out) and torch.equal(mt.integrate_pos(mx, q1, v, np.float64(0.01)), out)
    dq = mt.differentiate_pos(mx, q1, q2, 0.5)
    assert tuple(dq.shape) == batch + (J[2],) and dq.dtype == dtype
    assert np.array_equal(dq.numpy(), qr.differentiate_pos(J, q1.numpy(), q2.numpy(), 0.5).astype(npdt))
    assert np.array_equal(mt.differentiate_pos(mx, q1, q2).numpy(), qr.differentiate_pos(J, q1.numpy(), q2.numpy(), 1.0).astype(npdt))
    nq = mt.normalize_quat(mx, 3 * q1)
    assert tuple(nq.shape) == batch + (J[1],) and np.array_equal(nq.numpy(), qr.normalize_quat(J, (3 * q1).numpy()).astype(npdt))
    assert [c["op"] for c in stand_in.calls] == [0, 0, 0, 1, 1, 2] and all(c["B"] == (int(np.prod(batch)) if batch else 1) for c in stand_in.calls)
    # states: na = 0 here, x = [qpos, qvel]
    x1, x2 = torch.cat([q1, v], -1), torch.cat([q2, 2 * v], -1)
    dx = mt.state_sub(mx, x2, x1)
    assert tuple(dx.shape) == batch + (2 * J[2],)
    assert torch.equal(dx[..., :J[2]], mt.differentiate_pos(mx, q1, q2)) and torch.equal(dx[..., J[2]:], 2 * v - v)
    back = mt.state_add(mx, x1, dx)
    assert tuple(back.shape) == batch + (J[1] + J[2],) and torch.equal(back[..., :J[1]], mt.integrate_pos(mx, q1, dx[..., :J[2]], 1.0))
    assert torch.equal(back[..., J[1]:], v + (2 * v - v))


def test_states_with_activations(stand_in):
    mx = load_model("muscle_arm")
    nq, nv, na = int(mx.nq), int(mx.nv), int(mx.na)
    assert na > 0
    rng = np.random.RandomState(5)
    x, dx = torch.tensor(rng.randn(4, nq + nv + na)), torch.tensor(rng.randn(4, 2 * nv + na))
    y = mt.state_add(mx, x, dx)
    assert tuple(y.shape) == (4, nq + nv + na) and torch.equal(y[:, nq:], x[:, nq:] + dx[:, nv:])
    assert torch.allclose(mt.state_sub(mx, y, x), dx, rtol=0, atol=1e-12)


def test_refusals_come_before_any_call(stand_in, models):
    mx = models[F64]
    nq, nv = int(mx.nq), int(mx.nv)
    q, v = torch.zeros(3, nq, dtype=F64), torch.zeros(3, nv, dtype=F64)
    bad = [
        (ValueError, "qpos has shape", lambda: mt.integrate_pos(mx, q[:, :-1], v, 0.1)),
        (ValueError, "qvel= must have shape", lambda: mt.integrate_pos(mx, q, v[:, :-1], 0.1)),
        (ValueError, "qvel= must have shape", lambda: mt.integrate_pos(mx, q, v[:2], 0.1)),
        (ValueError, "qvel= is torch.float32", lambda: mt.integrate_pos(mx, q, v.float(), 0.1)),
        (ValueError, "runs in the model's dtype", lambda: mt.integrate_pos(mx, q.float(), v.float(), 0.1)),
        (ValueError, "unsupported Data dtype", lambda: mt.integrate_pos(mx, q.half(), v.half(), 0.1)),
        (ValueError, "qpos has shape", lambda: mt.integrate_pos(mx, q.numpy(), v, 0.1)),
        (ValueError, "dt must be", lambda: mt.integrate_pos(mx, q, v, None)),
        (ValueError, "dt must be", lambda: mt.integrate_pos(mx, q, v, float("nan"))),
        (ValueError, "dt must be", lambda: mt.integrate_pos(mx, q, v, torch.tensor([0.1, 0.2]))),
        (ValueError, "non-zero", lambda: mt.differentiate_pos(mx, q, q, 0.0)),
        (ValueError, "qpos2= must have shape", lambda: mt.differentiate_pos(mx, q, v)),
        (ValueError, "qpos1 has shape", lambda: mt.differentiate_pos(mx, v, q)),
        (ValueError, "qpos has shape", lambda: mt.normalize_quat(mx, v)),
        (ValueError, "x2 must have shape", lambda: mt.state_sub(mx, q, torch.zeros(3, nq + nv, dtype=F64))),
        (ValueError, "x1", lambda: mt.state_sub(mx, torch.zeros(3, nq + nv, dtype=F64), torch.zeros(2, nq + nv, dtype=F64))),
        (ValueError, "dx must have shape", lambda: mt.state_add(mx, torch.zeros(3, nq + nv, dtype=F64), torch.zeros(3, nq + nv, dtype=F64))),
        (NotImplementedError, "integrate_pos cannot be used under torch.vmap", lambda: torch.vmap(lambda a: mt.integrate_pos(mx, a, v[0], 0.1))(q)),
        (NotImplementedError, "differentiate_pos cannot be used under torch.vmap", lambda: torch.vmap(lambda a: mt.differentiate_pos(mx, a, q[0]))(q)),
        (NotImplementedError, "normalize_quat cannot be used under torch.vmap", lambda: torch.vmap(lambda a: mt.normalize_quat(mx, a))(q)),
        (NotImplementedError, "state_add cannot be used under torch.vmap",
         lambda: torch.vmap(lambda a: mt.state_add(mx, a, torch.zeros(2 * nv, dtype=F64)))(torch.zeros(3, nq + nv, dtype=F64))),
    ]
    for exc, match, run in bad:
        with pytest.raises(exc, match=match):
            run()
    assert not stand_in.calls


def test_compile_is_refused(stand_in, models):
    mx = models[F64]
    q, v = torch.zeros(3, int(mx.nq), dtype=F64), torch.zeros(3, int(mx.nv), dtype=F64)
    with pytest.raises(Exception, match="integrate_pos cannot be used under torch.vmap / torch.compile"):
        torch.compile(lambda a, b: mt.integrate_pos(mx, a, b, 0.1), backend="eager", fullgraph=True)(q, v)
    assert not stand_in.calls


def test_without_the_stand_in_cpu_tensors_are_refused(models):
    mx = models[F64]
    with pytest.raises(RuntimeError, match="HIP device"):
        mt.normalize_quat(mx, torch.zeros(2, int(mx.nq), dtype=F64))


def test_an_empty_batch_returns_without_a_call(stand_in, models):
    mx = models[F64]
    out = mt.integrate_pos(mx, torch.zeros(0, int(mx.nq), dtype=F64), torch.zeros(0, int(mx.nv), dtype=F64), 0.1)
    assert tuple(out.shape) == (0, int(mx.nq)) and not stand_in.calls
