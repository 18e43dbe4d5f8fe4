"""deriv_smooth_vel / implicit / euler on the GPU (csrc/mjh_integrate.h) against the tests' longdouble reference (tests/_integrator_ref.py, pinned on the
reference's recordings by tests/test_integrator_host.py) and against those recordings (tests/golden/integrator/, tools/gen_integrator_golden.py).

Bounds, none taken from what the kernel gives: qDeriv entrywise |got - ref| <= 4 k u S (k = nu + ntendon + 1 terms, S the sum of the absolute terms); the returned
qacc by residual, |A x - b|inf <= 4 n u (|A|inf |x|inf + |b|inf) with A as the reference's factorisation rule defines it; with the returned qacc taken as given, the
four advanced leaves against the longdouble formulas at TOL_PRE[dtype] of the leaf's largest magnitude; against the recording, a leaf may be off the longdouble
solution by 4 x the reference's own recorded distance plus 4 n u max|leaf| (two backward-stable solves with different summation orders, LAPACK's for nv > 16, can sit on
opposite sides of the exact result).  u = 2^-53 / 2^-24.  Batches of 1, 5 and 67 (the last workgroup partly filled), inputs both ways: the recorded pass's leaves
(only the tail is under test) and a live mt.forward."""
import numpy as np
import pytest
import torch

import _integrator_ref as ir
import mujoco_torch_amd as mt
from _cases import TOL_PRE

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64, F32 = torch.float64, torch.float32
CASES = ["integrator_rig_f64", "integrator_rig_f32", "integrator_ctrl_rig_f64", "integrator_ctrl_rig_f32", "ant_f64", "satellite_small_f64", "pendula_f64", "humanoid_f64", "humanoid_f32", "centipede_f64"]
BATCHES = (1, 5, 67)
_DEVICE_MODELS = {}


def device_model(c):
    if c.name not in _DEVICE_MODELS:
        _DEVICE_MODELS[c.name] = c.model.to(DEV)
    return _DEVICE_MODELS[c.name]


def host(t):
    return t.detach().cpu().numpy()


def state_of(d, e=None):
    return {n: host(getattr(d, n)) if e is None else host(getattr(d, n))[e] for n in ir.STATE}


def check_tail(V, leaves, dtype, mx, d, what, h=None, recorded=None, distance=None, nenv=None, hp=None):
    """Runs the three functions on the device Data ``d`` (its leaves on the host: ``leaves[e]``) and holds every environment to the derived bounds; returns the
    worst ratios (and, with a recording, the worst share of the recording's bound and whether qacc is the recording's bits)."""
    u, tol = ir.U[str(dtype)[6:]], TOL_PRE[dtype]
    B, nv = d.qvel.shape[0], V["nv"]
    kw = {} if h is None else dict(dt=h)
    worst = dict(qderiv=0.0, solve=0.0, advance=0.0, recording=0.0)
    Q = mt.deriv_smooth_vel(mx, d)
    Qr = ir.qderiv(V, leaves[0])[0]
    assert (Q is None) == (Qr is None)
    if Q is not None:
        assert tuple(Q.shape) == (B, nv, nv) and Q.dtype == dtype and Q.device.type == "cuda"
        Qh = host(Q)
        assert np.array_equal(Qh, Qh.transpose(0, 2, 1))
        for e in range(B):
            worst["qderiv"] = max(worst["qderiv"], ir.qderiv_excess(V, leaves[e], Qh[e], u))
    same_bits = True
    for which in ("implicit", "euler"):
        out, qacc = getattr(mt, which)(mx, d, return_qacc=True, **kw)
        assert tuple(qacc.shape) == (B, nv) and qacc.dtype == dtype
        plain = getattr(mt, which)(mx, d, **kw)
        got, qa = state_of(out), host(qacc)
        for n in ir.STATE:
            assert torch.equal(getattr(plain, n), getattr(out, n)), (which, n)
        assert out.qacc.data_ptr() == d.qacc.data_ptr()  # (the solver's, as in the reference)
        for e in range(B):
            r = ir.solve_excess(V, leaves[e], which, qa[e], u, h)
            worst["solve"] = max(worst["solve"], r or 0.0)
            worst["advance"] = max(worst["advance"], ir.advance_excess(V, leaves[e], qa[e], {n: got[n][e] for n in ir.STATE}, tol, h))
            if recorded is not None:
                rec, ref = recorded[e % nenv], hp(e % nenv, which)
                for n in ir.STATE + ("qacc",):
                    g = (qa[e] if n == "qacc" else got[n][e]).astype(ir.HP).reshape(-1)
                    if g.size == 0:
                        continue
                    w = np.asarray(ref[n], dtype=ir.HP).reshape(-1)
                    allowed = 4 * distance[which][n][e % nenv] + 4 * max(nv, 1) * u * float(np.abs(w).max())
                    worst["recording"] = max(worst["recording"], float(np.abs(g - w).max()) / allowed)
                same_bits = same_bits and np.array_equal(qa[e], rec[which + "/qacc"])
    print(f"{what}: worst qDeriv / (4 k u S) {worst['qderiv']:.3g}, residual / bound {worst['solve']:.3g}, advance / TOL_PRE {worst['advance']:.3g}" +
          (f", off longdouble / (4 x the reference's distance + 4 n u max) {worst['recording']:.3g}, qacc the recording's bits: {same_bits}" if recorded is not None else ""))
    assert worst["qderiv"] <= 1 and worst["solve"] <= 1 and worst["advance"] <= 1 and worst["recording"] <= 1, worst
    return worst, same_bits


@pytest.mark.parametrize("name", CASES)
def test_the_recorded_pass_against_the_reference_and_the_recording(name):
    """Only the tail is under test: the leaves are the recorded forward pass's, so no solver branch enters."""
    c = ir.case(name)
    mx = device_model(c)
    for B in BATCHES:
        d = c.data(B, DEV)
        leaves = [c.leaves[e % c.nenv] for e in range(B)]
        check_tail(c.V, leaves, c.dtype, mx, d, f"{name} B = {B}", recorded=c.recorded, distance=c.distance, nenv=c.nenv, hp=c.hp)
        if B == 5:  # qDeriv against the recording too: two sums of the same terms
            Q = mt.deriv_smooth_vel(mx, d)
            for e in range(B):
                if Q is not None:
                    _, S, k = ir.qderiv(c.V, leaves[e])
                    err = np.abs(host(Q)[e].astype(ir.HP) - c.recorded[e % c.nenv]["qderiv"].astype(ir.HP))
                    assert (err <= 8 * k * c.u * S).all()


_LIVE = {}


def live(name, B=67):
    """(case, device model, the device's own forward pass of B states: the recorded states, repeated with seeded noise on qvel / ctrl / act)."""
    if name not in _LIVE:
        c = ir.case(name)
        mx = device_model(c)
        d = c.data(B)
        rng = np.random.RandomState(23)
        jitter = lambda t, s: t + torch.tensor(s * rng.randn(*t.shape) * (np.arange(B) >= c.nenv).reshape((B,) + (1,) * (t.dim() - 1)), dtype=t.dtype)
        ctrl = jitter(d.ctrl, 0.3)
        if "ctrl_rig" in name:  # (a damper's control is not negative; above every ctrlrange of the rig, as in its recordings)
            ctrl = ctrl.abs() + 0.15
        d = mt.make_data(c.model).to(c.dtype).expand(B).clone().replace(qpos=d.qpos, qvel=jitter(d.qvel, 0.3), ctrl=ctrl, act=jitter(d.act, 0.1), time=d.time)
        _LIVE[name] = (c, mx, mt.forward(mx, d.to(DEV)))
    return _LIVE[name]


@pytest.mark.parametrize("name", CASES)
def test_a_live_forward_pass_against_the_reference(name):
    c, mx, f = live(name)
    L = ir.leaves_of(f)
    for B in BATCHES:
        check_tail(c.V, [ir.env(L, e) for e in range(B)], c.dtype, mx, f[:B], f"{name} live B = {B}")


@pytest.mark.parametrize("name", ["integrator_rig_f64", "integrator_rig_f32", "integrator_ctrl_rig_f64", "humanoid_f64", "centipede_f64"])
def test_an_environment_of_a_batch_equals_the_same_state_alone(name):
    """lanes, envs and chunk follow from the model alone: environment i of 67 is, bit for bit, the call on it alone and on a slice [i : i + 3]."""
    _, mx, f = live(name)
    full = {w: getattr(mt, w)(mx, f, return_qacc=True) for w in ("implicit", "euler")}
    Q = mt.deriv_smooth_vel(mx, f)
    for i in (0, 1, 7, 8, 31, 64):
        for lo, hi in ((i, i + 1), (i, i + 3)):
            for w, (out, qacc) in full.items():
                o, qa = getattr(mt, w)(mx, f[lo:hi], return_qacc=True)
                assert torch.equal(qa, qacc[lo:hi]), (w, i)
                for n in ir.STATE:
                    assert torch.equal(getattr(o, n), getattr(out, n)[lo:hi]), (w, n, i)
            if Q is not None:
                assert torch.equal(mt.deriv_smooth_vel(mx, f[lo:hi]), Q[lo:hi]), i
    out23 = mt.implicit(mx, torch.stack([f[7:10], f[10:13]]))
    assert tuple(out23.qvel.shape[:2]) == (2, 3) and torch.equal(out23.qvel.reshape(6, -1), full["implicit"][0].qvel[7:13])


@pytest.mark.parametrize("name", ["integrator_ctrl_rig_f64", "integrator_ctrl_rig_f32"])
def test_a_stateless_actuator_reads_the_raw_control(name):
    """dyntype NONE: c_i is d.ctrl[i] as the caller left it, not the control the forward pass clamps to ctrlrange.  Every limited actuator of the rig has a
    vel_i that depends on ctrl and a control beyond its range, in the recorded and in the live pass: the bounds of the two tests above hold for the raw control, and
    here the clamped control is shown to miss them (so would a kernel that clamped, or read another slot)."""
    c, mx, f = live(name)
    lim = np.nonzero(ir._np(c.model.actuator_ctrllimited))[0]
    hi = ir._np(c.model.actuator_ctrlrange)[lim, 1]
    gain_vel = np.asarray(c.V["gainprm"][:, 2] * (c.V["gaintype"] == ir.AFFINE), dtype=np.float64)
    assert c.V["na"] == 0 and len(lim) == 3 and (gain_vel[lim] != 0).all()
    for d, B in ((c.data(5, DEV), 5), (f, 67)):
        L = ir.leaves_of(d)
        assert (L["ctrl"][:, lim] > hi).all()
        Q = host(mt.deriv_smooth_vel(mx, d))
        lo_hi = torch.tensor(ir._np(c.model.actuator_ctrlrange), dtype=c.dtype, device=DEV)
        limited = torch.tensor(ir._np(c.model.actuator_ctrllimited), device=DEV)
        clamped = torch.where(limited, torch.minimum(torch.maximum(d.ctrl, lo_hi[:, 0]), lo_hi[:, 1]), d.ctrl)
        Qc = host(mt.deriv_smooth_vel(mx, d.replace(ctrl=clamped)))
        for e in range(B):
            Le = ir.env(L, e)
            assert ir.qderiv_excess(c.V, Le, Q[e], c.u) <= 1
            assert ir.qderiv_excess(c.V, Le, Qc[e], c.u) > 1e3 and ir.qderiv_excess(c.V, dict(Le, ctrl=host(clamped)[e]), Qc[e], c.u) <= 1
        # ... and it reaches the step: the implicit qvel moves with the raw control
        assert not torch.equal(mt.implicit(mx, d).qvel, mt.implicit(mx, d.replace(ctrl=clamped)).qvel)


ACTUATION, DAMPER, EULERDAMP = 1 << 11, 1 << 6, 1 << 15


def flagged(mx, flags):
    return mx.replace(opt=mx.opt.replace(disableflags=type(mx.opt.disableflags)(int(mx.opt.disableflags) | flags)))


@pytest.mark.parametrize("name,flags", [("integrator_rig_f64", ACTUATION), ("integrator_rig_f64", DAMPER), ("satellite_small_f64", ACTUATION), ("ant_f64", DAMPER),
                                         ("integrator_rig_f64", EULERDAMP)], ids=["rig-actuation", "rig-damper", "satellite-actuation", "ant-damper", "rig-eulerdamp"])
def test_the_disable_flags_are_the_callers(name, flags):
    """The flags are read from the caller's Model at each call (the pass itself is the unflagged model's: the tail reads its leaves as they are)."""
    c, mx, f = live(name)
    L = ir.leaves_of(f[:5])
    V = dict(c.V, disableflags=c.V["disableflags"] | flags)
    check_tail(V, [ir.env(L, e) for e in range(5)], c.dtype, flagged(mx, flags), f[:5], f"{name} flags {flags:#x}")
    if flags == DAMPER and c.V["nt"]:  # the tendon term stays in: the reference's quirk
        Q = host(mt.deriv_smooth_vel(flagged(mx, flags | ACTUATION), f[:5]))
        ball = int(c.V["jnt_dofadr"][1])  # (no tendon reaches the ball joint: its damping is gone, the tendons' is not)
        assert np.abs(Q).max() > 0 and not Q[:, ball:ball + 3].any()


def test_without_any_term_implicit_advances_with_the_pass_qacc():
    """ACTUATION and DAMPER off on a model without tendons: deriv_smooth_vel is None and implicit is, bit for bit, euler under EULERDAMP off."""
    c, mx, f = live("ant_f64")
    none = flagged(mx, ACTUATION | DAMPER)
    assert mt.deriv_smooth_vel(none, f) is None
    a, qa = mt.implicit(none, f, return_qacc=True)
    b, qb = mt.euler(flagged(mx, EULERDAMP), f, return_qacc=True)
    assert torch.equal(qa, f.qacc) and torch.equal(qb, f.qacc)
    for n in ir.STATE:
        assert torch.equal(getattr(a, n), getattr(b, n)), n
    assert not torch.equal(a.qvel, mt.implicit(mx, f).qvel)


def test_value_only_edits_are_honoured_without_a_new_native_model():
    from mujoco_torch_amd._postpass import handle as _handle

    c, mx, f = live("integrator_rig_f64")
    nm = _handle(mx, f.qpos.device, F64)
    L = ir.leaves_of(f[:5])
    leaves = [ir.env(L, e) for e in range(5)]
    base = mt.implicit(mx, f[:5]).qvel
    gain = mx.actuator_gainprm.clone()
    gain[:, 2] *= 3
    h = float(mx.opt.timestep)
    edits = [(mx.replace(dof_damping=5 * mx.dof_damping), dict(dof_damping=5 * c.V["dof_damping"]), None),
             (mx.replace(actuator_gainprm=gain), dict(gainprm=ir._np(gain).astype(ir.HP)), None),
             (mx.replace(opt=mx.opt.replace(timestep=2 * mx.opt.timestep)), dict(timestep=ir.HP(2 * h)), None),
             (mx, {}, h / 2)]
    for i, (edited, values, dt) in enumerate(edits):
        check_tail(dict(c.V, **values), leaves, F64, edited, f[:5], f"edit {i}", h=dt)
        assert _handle(edited, f.qpos.device, F64) is nm  # (the same native model serves the edited one)
        assert not torch.equal(mt.implicit(edited, f[:5], **({} if dt is None else dict(dt=dt))).qvel, base), i
    assert torch.equal(mt.euler(mx, f[:5], dt=torch.tensor(h / 2, dtype=F64)).qvel, mt.euler(mx, f[:5], dt=h / 2).qvel)


@pytest.mark.parametrize("name", ["ant_f64", "humanoid_f64", "humanoid_f32", "integrator_rig_f64", "integrator_rig_f32"])
def test_euler_on_a_forward_pass_agrees_with_step(name):
    """Euler models, states _check_state leaves alone: the state leaves of euler(mx, forward(mx, d)) agree with step(mx, d) within TOL_PRE."""
    c, mx, f = live(name)
    d = mt.make_data(c.model).to(c.dtype).expand(f.qpos.shape[0]).clone().to(DEV).replace(qpos=f.qpos, qvel=f.qvel, ctrl=f.ctrl, act=f.act, time=f.time)
    s, e = mt.step(mx, d), mt.euler(mx, f)
    same = True
    for n in ir.STATE:
        a, b = host(getattr(s, n)).astype(np.float64), host(getattr(e, n)).astype(np.float64)
        if a.size:
            assert np.abs(a - b).max() <= TOL_PRE[c.dtype] * max(float(np.abs(a).max()), 1e-30), n
        same = same and np.array_equal(a, b)
    print(f"{name}: euler(forward) and step bit-identical: {same}")


_HINGE = """<mujoco><compiler angle="radian"/><option timestep="0.01" gravity="0 0 0"/><worldbody>
  <body><joint name="h" type="hinge" axis="0 1 0"/><geom type="sphere" size="0.1" mass="1"/></body>
</worldbody><actuator><velocity joint="h" kv="{kv}"/></actuator></mujoco>"""


def test_the_point_of_it_all():
    """One hinge with a velocity servo, h kv / I = 4: explicit Euler multiplies qvel by |1 - 4| = 3 a step, the implicit tail by 1 / (1 + 4)."""
    probe = mt.device_put(mt.mjcf.from_xml_string(_HINGE.format(kv=1.0))).to(DEV)
    fp = mt.forward(probe, mt.make_data(probe).expand(1).clone().to(DEV))
    I = float(mt.full_m(probe, fp).reshape(-1)[0])
    h = 0.01
    lite = mt.mjcf.from_xml_string(_HINGE.format(kv=repr(4 * I / h)))
    lite.opt.disableflags = EULERDAMP
    mx = mt.device_put(lite).to(DEV)
    d0 = mt.make_data(mx).expand(8).clone().to(DEV)
    d0 = d0.replace(qvel=torch.linspace(0.1, 0.8, 8, dtype=F64, device=DEV).reshape(8, 1))
    de, di = d0, d0
    norms = [di.qvel.abs().clone()]
    for _ in range(20):
        de = mt.step(mx, de)
        di = mt.implicit(mx, mt.forward(mx, di))
        norms.append(di.qvel.abs().clone())
    grow = (de.qvel.abs() / d0.qvel.abs()).min().item()
    print(f"I = {I:.6g}; after 20 steps |qvel| / start: step (Euler) {grow:.3g} (3^20 = {3.0 ** 20:.3g}), implicit {(norms[-1] / norms[0]).max().item():.3g} (5^-20 = {5.0 ** -20:.3g})")
    assert grow > 1e6
    assert all((b < a).all() for a, b in zip(norms, norms[1:]))
    assert torch.allclose(norms[1] / norms[0], torch.full_like(norms[0], 0.2), rtol=1e-9, atol=0)


def test_inputs_are_not_modified_and_outputs_own_their_storage():
    c, mx, f = live("integrator_rig_f64")
    before = {n: getattr(f, n).clone() for n in ir.LEAVES}
    ptrs = {getattr(f, n).untyped_storage().data_ptr() for n in ir.LEAVES}
    for w in ("implicit", "euler"):
        out, qacc = getattr(mt, w)(mx, f, return_qacc=True)
        for n in ir.STATE:
            assert getattr(out, n).untyped_storage().data_ptr() not in ptrs, (w, n)
        assert qacc.untyped_storage().data_ptr() not in ptrs
        assert out.qM is f.qM
    mt.deriv_smooth_vel(mx, f)
    torch.cuda.synchronize()
    for n, t in before.items():
        assert torch.equal(getattr(f, n), t), n
