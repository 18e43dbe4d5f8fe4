"""deriv_smooth_vel / implicit / euler without a GPU: the public functions and their refusals, and the tests' own longdouble reference (tests/_integrator_ref.py)
-- the yardstick of tests/test_integrator.py -- pinned on every recording of the reference (tests/golden/integrator/, tools/gen_integrator_golden.py) and on
closed forms.

Bounds: the recorded qDeriv within 4 k u S per entry of the longdouble one (k = nu + ntendon + 1 terms, S the sum of the absolute terms, u the unit roundoff of the
recording's dtype); the recorded qacc by residual against the matrix the reference's factorisation rule defines, |A x - b|inf <= 4 n u (|A|inf |x|inf + |b|inf) (the
generator records qacc, so nothing is recovered from qvel); the recorded advanced leaves, with the recorded qacc taken as given, at TOL_PRE[dtype] of the leaf's
largest magnitude."""
import re

import numpy as np
import pytest
import torch

import _integrator_ref as ir
import mujoco_torch_amd as mt
import pyoracle
from _cases import TOL_PRE
from _util import load_model

CASES = sorted(f[:-4] for f in __import__("os").listdir(ir.GOLD) if f.endswith(".npz"))
DAMPER, ACTUATION, EULERDAMP = 1 << 6, 1 << 11, 1 << 15


# ---- the reference pinned on the recordings ----------------------------------------------------------------------------------------------------------

def test_every_case_of_the_issue_is_recorded():
    assert set(CASES) >= {"integrator_rig_f64", "integrator_rig_f32", "integrator_ctrl_rig_f64", "integrator_ctrl_rig_f32", "integrator_rig_nodamper_f64", "ant_f64", "satellite_small_f64", "pendula_f64", "humanoid_f64",
                          "humanoid_f32", "centipede_f64"}
    sizes = {n: ir.case(n).meta["sizes"] for n in CASES}
    # (the bundled ant is the legs alone, 8 hinges: the free joint under the inline Cholesky is the rig's)
    assert sizes["ant_f64"]["nv"] == 8 and sizes["humanoid_f64"]["nv"] == 27 and sizes["centipede_f64"]["nv"] == 72
    rig = sizes["integrator_rig_f64"]
    assert rig["nv"] == 12 and 0 in ir.case("integrator_rig_f64").V["jnt_type"] and rig["na"] == rig["nu"] == 6 and rig["ntendon"] == 2 and sizes["pendula_f64"]["ntendon"] > 0


@pytest.mark.parametrize("name", CASES)
def test_the_reference_is_pinned_on_the_recording(name):
    c = ir.case(name)
    tol = TOL_PRE[c.dtype]
    worst = dict(qderiv=0.0, solve=0.0, advance=0.0)
    for e in range(c.nenv):
        L, rec = c.leaves[e], c.recorded[e]
        Q = ir.qderiv(c.V, L)[0]
        assert (Q is None) == ("qderiv" not in rec)
        if Q is not None:
            worst["qderiv"] = max(worst["qderiv"], ir.qderiv_excess(c.V, L, rec["qderiv"], c.u))
        for which in ("implicit", "euler"):
            r = ir.solve_excess(c.V, L, which, rec[which + "/qacc"], c.u)
            worst["solve"] = max(worst["solve"], r or 0.0)
            worst["advance"] = max(worst["advance"], ir.advance_excess(c.V, L, rec[which + "/qacc"], {n: rec[f"{which}/{n}"] for n in ir.STATE}, tol))
            # the meta's distances are the recording's distances from this reference
            hp = c.hp(e, which)
            for n in ir.STATE + ("qacc",):
                d = float(np.abs(rec[f"{which}/{n}"].astype(ir.HP) - hp[n]).max(initial=0))
                assert d == pytest.approx(c.distance[which][n][e], rel=1e-6, abs=1e-300), (which, n)
    print(f"{name}: recorded qDeriv / (4 k u S) {worst['qderiv']:.3g}, residual / bound {worst['solve']:.3g}, advance / TOL_PRE {worst['advance']:.3g}")
    assert worst["qderiv"] <= 1 and worst["solve"] <= 1 and worst["advance"] <= 1, worst


@pytest.mark.parametrize("name", ["integrator_ctrl_rig_f64", "integrator_ctrl_rig_f32"])
def test_the_reference_reads_the_raw_control_of_a_stateless_actuator(name):
    """na == 0: the dampers and the affine-gain general actuator of integrator_ctrl_rig have vel_i = gainprm[2] ctrl, every recorded control lies above its ctrlrange,
    and the reference's recorded qDeriv is the raw control's: the longdouble qDeriv of the clamped control misses it by far more than the bound."""
    c = ir.case(name)
    lim = np.nonzero(ir._np(c.model.actuator_ctrllimited))[0]
    rng = ir._np(c.model.actuator_ctrlrange)
    gain_vel = np.asarray(c.V["gainprm"][:, 2] * (c.V["gaintype"] == ir.AFFINE), dtype=np.float64)
    assert c.V["na"] == 0 and (c.V["dyntype"] == ir.DYN_NONE).all() and lim.tolist() == [0, 1, 2] and (gain_vel[lim] != 0).all() and not gain_vel[3:].any()
    for e in range(c.nenv):
        L = c.leaves[e]
        assert (L["ctrl"][lim] > rng[lim, 1]).all()
        clamped = np.where(ir._np(c.model.actuator_ctrllimited), np.clip(L["ctrl"], rng[:, 0], rng[:, 1]), L["ctrl"]).astype(L["ctrl"].dtype)
        assert ir.qderiv_excess(c.V, L, c.recorded[e]["qderiv"], c.u) <= 1
        assert ir.qderiv_excess(c.V, dict(L, ctrl=clamped), c.recorded[e]["qderiv"], c.u) > 1e3


def test_the_tendon_term_stays_in_under_the_damper_flag():
    """The reference's quirk, on the recording made with DisableBit.DAMPER: the dof damping is gone from the recorded qDeriv, the tendons' damping is not."""
    c, full = ir.case("integrator_rig_nodamper_f64"), ir.case("integrator_rig_f64")
    assert c.V["disableflags"] & DAMPER and c.V["nt"] == 2 and c.V["tendon_damping"].min() > 0
    for e in range(c.nenv):
        Q = c.recorded[e]["qderiv"].astype(ir.HP)
        J = c.leaves[e]["ten_J"].astype(ir.HP)
        tend = -sum(c.V["tendon_damping"][t] * np.outer(J[t], J[t]) for t in range(2))
        acts = ir.qderiv(dict(c.V, nt=0), c.leaves[e])[0]  # (DAMPER set: the actuator term alone)
        assert np.abs(tend).max() > 0.1 and np.abs(Q - (acts + tend)).max() < 1e-14
        ball = int(c.V["jnt_dofadr"][1])
        assert not Q[ball:ball + 3, ball:ball + 3].any() or np.allclose(np.asarray(Q[ball:ball + 3, ball:ball + 3], dtype=float), np.asarray(acts[ball:ball + 3, ball:ball + 3], dtype=float))
    # ... and with the flag clear the diagonal carries the dof damping too
    Q0 = full.recorded[0]["qderiv"].astype(ir.HP)
    free = int(full.V["jnt_dofadr"][-1])
    assert np.allclose(np.asarray(np.diag(Q0)[free:free + 6], dtype=float), -0.02)


# ---- closed forms ------------------------------------------------------------------------------------------------------------------------------------------

_HINGE = """<mujoco><compiler angle="radian"/><option timestep="0.01" gravity="0 0 0"/><worldbody>
  <body><joint name="h" type="hinge" axis="0 1 0" damping="0.3"/><geom type="sphere" size="0.1" mass="1"/></body>
</worldbody><actuator><velocity joint="h" kv="2.5"/></actuator></mujoco>"""


def oracle_leaves(mx, d):
    out = dict(pyoracle.run(mx, d, step=False))
    B = d.qpos.shape[0]
    for n in ("qpos", "qvel", "act", "ctrl", "time"):
        out[n] = getattr(d, n).numpy().copy()
    nv = int(mx.nv)
    L = {n: np.asarray(out[n]) for n in ir.LEAVES}
    L["qM"], L["actuator_moment"], L["ten_J"] = L["qM"].reshape(B, nv, nv), L["actuator_moment"].reshape(B, -1, nv), L["ten_J"].reshape(B, -1, nv)
    L["time"] = L["time"].reshape(B)
    return L


def test_a_hinge_with_a_velocity_servo_by_hand():
    """qDeriv = -kv - damping; the implicit qvel' = (I v + h f) / (I + h (kv + damping)), f the force that does not depend on the velocity (kv ctrl)."""
    mx = mt.device_put(mt.mjcf.from_xml_string(_HINGE))
    v0, u0 = 0.7, 0.4
    d = mt.make_data(mx).expand(1).clone().replace(qvel=torch.tensor([[v0]], dtype=torch.float64), ctrl=torch.tensor([[u0]], dtype=torch.float64))
    L = ir.env(oracle_leaves(mx, d), 0)
    V = ir.model_values(mx)
    Q, S, k = ir.qderiv(V, L)
    assert Q.shape == (1, 1) and abs(float(Q[0, 0]) - (-2.5 - 0.3)) < 1e-15 and k == 2
    I, h = float(L["qM"][0, 0]), 0.01
    f = float(L["qfrc_smooth"][0] + L["qfrc_constraint"][0])
    assert abs(f - (2.5 * u0 - 2.5 * v0 - 0.3 * v0)) < 1e-12  # (the servo and the damper are all that pushes)
    r = ir.integrate(V, L, "implicit")
    assert abs(float(r["qvel"][0]) - (I * v0 + h * 2.5 * u0) / (I + h * (2.5 + 0.3))) < 1e-14
    assert abs(float(r["qpos"][0]) - h * float(r["qvel"][0])) < 1e-15 and abs(float(r["time"]) - h) < 1e-18
    e = ir.integrate(V, L, "euler")
    assert abs(float(e["qvel"][0]) - (I * v0 + h * (2.5 * u0 - 2.5 * v0)) / (I + h * 0.3)) < 1e-14  # (Euler: the dof damping alone is implicit)


def test_the_none_cases():
    mx = mt.device_put(mt.mjcf.from_xml_string(_HINGE))
    d = mt.make_data(mx).expand(1).clone()
    L = ir.env(oracle_leaves(mx, d), 0)
    V = ir.model_values(mx)
    assert ir.qderiv(dict(V, disableflags=ACTUATION | DAMPER), L)[0] is None
    assert ir.system(dict(V, disableflags=ACTUATION | DAMPER), L, "implicit") == (None, None)
    assert ir.system(dict(V, disableflags=EULERDAMP), L, "euler") == (None, None)
    assert float(ir.qderiv(dict(V, disableflags=ACTUATION), L)[0][0, 0]) == -0.3 and float(ir.qderiv(dict(V, disableflags=DAMPER), L)[0][0, 0]) == -2.5
    # the public function, which needs no device to say so
    lite = mt.mjcf.from_xml_string(_HINGE)
    lite.opt.disableflags = ACTUATION | DAMPER
    assert mt.deriv_smooth_vel(mt.device_put(lite), d) is None


# ---- the host API --------------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def rig():
    mx = load_model("integrator_rig")
    return mx, mt.make_data(mx).expand(3).clone()


def test_the_functions_and_the_entry_point_are_public():
    from mujoco_torch_amd import native

    for n in ("deriv_smooth_vel", "implicit", "euler"):
        assert callable(getattr(mt, n)), n
    assert hasattr(native, "IntegrateArgs") and native.ABI_VERSION >= 19
    text = open(native.HEADER).read()
    assert re.search(r"\bint mjh_integrate\s*\(const mjhModel\* m, const mjhIntegrateArgs\* args, void\* hip_stream\);", text)
    assert re.search(r"#define MJH_KERNEL_INTEGRATE 35\b", text)
    for i, n in enumerate(("QDERIV", "IMPLICIT", "EULER", "STATE", "WRITE_QDERIV", "WRITE_QACC")):
        assert re.search(rf"#define MJH_INTEGRATE_{n} {1 << i}\b", text)
    body = text[text.index("typedef struct mjhIntegrateArgs {"):text.index("} mjhIntegrateArgs;")]
    fields = re.findall(r"[*\s,](\w+)(?=[,;])", body.split("{", 1)[1])
    assert fields == [f[0] for f in native.IntegrateArgs._fields_], fields


def test_the_launch_plan_serves_every_model_one_environment_fits():
    """mjh_integrate_plan (the plan mjh_integrate launches with, a host computation) over nv, nu and both dtypes: whenever one environment -- the triangle, the
    right-hand side, the new qvel, vel_i and one row -- fits the 64 KB a workgroup may take, the plan holds at least one row (the call is not refused), and every
    plan stays inside its budget with whole environments in a 256-lane workgroup."""
    import ctypes

    from mujoco_torch_amd import native

    lib = native.load_library()
    r4 = lambda n: (n + 3) & ~3
    out = (ctypes.c_int * 4)()
    served = refused = 0
    for real_bytes in (8, 4):
        for nv in range(1, 200):
            for nu in sorted({0, 1, 2, 3, 4, 5, 8, nv // 2, nv - 8, nv - 7, nv - 6, nv - 5, nv - 4, nv - 3, nv - 2, nv - 1, nv, nv + 3} - set(range(-9, 0))):
                fixed = r4(nv * (nv + 1) // 2) + 2 * r4(nv) + r4(nu)
                fits = (r4(fixed + nv) + 4) * real_bytes <= 64 * 1024
                rc = lib.mjh_integrate_plan(nv, nu, 0, real_bytes, out)
                if not fits:
                    refused += rc != 0
                    continue
                assert rc == 0, (nv, nu, real_bytes)
                lanes, envs, chunk, lds_env = list(out)
                served += 1
                assert lanes == (16 if nv <= 16 else 32 if nv <= 32 else 64) and envs >= 1 and envs * lanes <= 256 and 256 // lanes % envs == 0
                assert 1 <= chunk <= max(nv, nu, 1) and lds_env == r4(fixed + chunk * nv) and envs * lds_env * real_bytes <= (52 * 1024 if envs > 1 else 64 * 1024)
    assert served > 3000 and refused > 100
    # the models the first plan refused although they fit with fewer environments
    for nv, nu, rb in ((54, 5, 8), (54, 8, 8), (78, 1, 8), (78, 4, 4), (111, 101, 4), (111, 104, 4)):
        assert lib.mjh_integrate_plan(nv, nu, 0, rb, out) == 0 and out[2] >= 1, (nv, nu, rb)
    assert lib.mjh_integrate_plan(-1, 0, 0, 8, out) == -22 and lib.mjh_integrate_plan(5, 0, 0, 2, out) == -22


def test_device_put_still_refuses_the_implicit_integrators():
    for integrator in (2, 3):
        lite = mt.mjcf.from_xml_string(_HINGE)
        lite.opt.integrator = integrator
        with pytest.raises(NotImplementedError):
            mt.device_put(lite)


def test_cpu_data_is_refused(rig):
    mx, d = rig
    for call in (lambda: mt.deriv_smooth_vel(mx, d), lambda: mt.implicit(mx, d), lambda: mt.euler(mx, d, dt=0.001, return_qacc=True)):
        with pytest.raises(RuntimeError, match="HIP device"):
            call()


def test_arguments_are_validated(rig):
    mx, d = rig
    with pytest.raises(ValueError, match="qM"):
        mt.implicit(mx, d.replace(qM=d.qM[:, :-1]))
    with pytest.raises(ValueError, match="actuator_moment"):
        mt.deriv_smooth_vel(mx, d.replace(actuator_moment=d.actuator_moment[:, :-1]))
    with pytest.raises(ValueError, match="ten_J"):
        mt.implicit(mx, d.replace(ten_J=d.ten_J.to(torch.float32)))
    with pytest.raises(ValueError, match="qvel"):
        mt.euler(mx, d.replace(qvel=d.qvel[:, :-1]))
    with pytest.raises(ValueError, match="act_dot"):
        mt.euler(mx, d.replace(act_dot=d.act_dot[:1]))
    with pytest.raises(ValueError, match="dtype"):
        mt.implicit(mx, d.to(torch.float32))
    with pytest.raises(ValueError, match="dof_damping"):
        mt.implicit(mx.replace(dof_damping=mx.dof_damping[:-1]), d)
    with pytest.raises(ValueError, match="actuator_gainprm"):
        mt.deriv_smooth_vel(mx.replace(actuator_gainprm=mx.actuator_gainprm[:, :2]), d)
    for bad in (torch.zeros(2), "fast", float("nan")):
        with pytest.raises(ValueError, match="dt="):
            mt.implicit(mx, d, dt=bad)
    with pytest.raises(TypeError):
        mt.implicit(mx, d, 0.001)  # (keyword only)


def test_fluid_parameters_are_refused_as_in_the_reference():
    def swimmer(flags=0):
        lite = mt.mjcf.from_xml_path(mt.test_data_path("swimmer.xml"))
        lite.opt.viscosity, lite.opt.disableflags = 0.1, flags
        return mt.device_put(lite)

    mx = swimmer()
    assert bool(mx.opt.has_fluid_params)
    d = mt.make_data(mx).expand(2).clone()
    for call in (lambda m: mt.deriv_smooth_vel(m, d), lambda m: mt.implicit(m, d)):
        with pytest.raises(NotImplementedError, match="fluid drag not supported for implicitfast"):
            call(mx)
    for flag in (DAMPER, 1 << 5):  # with DAMPER or SPRING disabled the reference goes on: here, on to the device check
        with pytest.raises(RuntimeError, match="HIP device"):
            mt.implicit(swimmer(flag), d)
    with pytest.raises(RuntimeError, match="HIP device"):  # (euler never asks)
        mt.euler(mx, d)


@pytest.mark.parametrize("name", ["deriv_smooth_vel", "implicit", "euler"])
def test_vmap_is_refused_by_name(rig, name):
    mx, d = rig
    fn = lambda q: (lambda r: r if isinstance(r, torch.Tensor) else r.qpos)(getattr(mt, name)(mx, d.replace(qvel=q)))
    with pytest.raises(NotImplementedError, match=name):
        torch.vmap(fn)(d.qvel)


@pytest.mark.parametrize("name", ["deriv_smooth_vel", "implicit", "euler"])
def test_compile_is_refused_by_name(rig, name):
    mx, d = rig
    fn = torch.compile(lambda q: (lambda r: r if isinstance(r, torch.Tensor) else r.qpos)(getattr(mt, name)(mx, d.replace(qvel=q))), fullgraph=True)
    with pytest.raises(Exception, match=name) as info:
        fn(d.qvel)
    assert isinstance(info.value, NotImplementedError) or "NotImplementedError" in str(info.value) or isinstance(getattr(info.value, "__cause__", None), NotImplementedError)


def test_the_values_are_the_callers(rig):
    """dof_damping and the actuator parameters are read from the caller's Model, tendon_damping (no Model field) from the compiled model the tables keep."""
    from mujoco_torch_amd.integrate import _values

    mx, _ = rig
    assert not hasattr(mx, "tendon_damping")
    edited = mx.replace(dof_damping=3 * mx.dof_damping, actuator_dynprm=mx.actuator_dynprm + 1)
    assert edited.tables is mx.tables
    for dtype in (torch.float64, torch.float32):
        v = _values("implicit", edited, dtype, torch.device("cpu"), ["dof_damping", "tendon_damping", "gainprm", "biasprm", "dynprm", "actrange"])
        assert torch.equal(v["dof_damping"][0], (3 * mx.dof_damping).to(dtype)) and torch.equal(v["dynprm"][0], (mx.actuator_dynprm + 1).to(dtype))
        assert v["tendon_damping"][0].tolist() == torch.tensor([0.7, 0.25], dtype=torch.float64).to(dtype).tolist()
        assert v["gainprm"][1] == mx.actuator_gainprm.shape[1] and v["dynprm"][1] == mx.actuator_dynprm.shape[1] and v["actrange"][1] == 2
