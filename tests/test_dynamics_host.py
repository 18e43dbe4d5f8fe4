"""The host side of tendon / transmission / passive / fwd_velocity / fwd_actuation / fwd_acceleration (mujoco_torch_amd/dynamics.py) and the tests' longdouble
reference (tests/_dynamics_ref.py) against the reference's recordings (tests/golden/dynamics/, tools/gen_dynamics_golden.py).  No GPU.

The bound is ``TOL_PRE[dtype]`` (tests/_cases.py) as ``_util.rel_err`` measures, the one the GPU tests hold the kernels to; the recordings carry the reference's own
distance from the longdouble evaluation (``ref_distance``), which must lie inside it for the bound to mean anything."""
import ctypes
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import _dynamics_ref as dr
import mujoco_torch_amd as mt
from _cases import TOL_PRE
from _util import rel_err
from mujoco_torch_amd import dynamics, native
from mujoco_torch_amd._enums import DisableBit

F64, F32 = torch.float64, torch.float32
OPS = ("TENDON", "TRANSMISSION", "VELOCITY", "PASSIVE", "ACTUATION", "ACCELERATION")


def f64(a):
    return np.asarray(a, dtype=np.float64)


def test_the_six_names_exist_with_the_recorded_signatures():
    api = json.load(open(os.path.join(dr.GOLD, "reference_api.json")))["signatures"]
    assert sorted(api) == sorted(dr.FUNCTIONS)
    for n, params in api.items():
        assert callable(getattr(mt, n)) and getattr(mt, n) is getattr(dynamics, n) and list(inspect.signature(getattr(mt, n)).parameters) == params, n


def test_the_header_declares_the_entry_points_the_ops_and_the_ids():
    from test_abi import header_fields

    text = open(native.HEADER).read()
    assert native.ABI_VERSION >= 28 and list(native.DynamicsArgs._fields_) == header_fields(text, "mjhDynamicsArgs")
    assert "mjh_dynamics" not in native.ARGS and len(native.ARGS) == 6  # bound beside the table, not in it
    assert re.search(r"\bint mjh_dynamics\s*\(const mjhModel\* m, const mjhDynamicsArgs\* args, void\* hip_stream\);", text)
    assert re.search(r"\bint mjh_dynamics_plan\s*\(int op, int nq, int nv, int nu, int nbody, int ntendon, int real_bytes, int\* lanes_envs_lds\);", text)
    for op, n in enumerate(OPS):
        assert re.search(rf"#define MJH_DYNAMICS_{n} {op}\b", text) and re.search(rf"#define MJH_KERNEL_DYNAMICS_{n} {63 + op}\b", text), n
        assert dynamics.OPS[n.lower()] == op
    usage = open(native.LIB_PATH.replace("libmjhip.so", "resource_usage.txt")).read().splitlines()
    mine = [ln for ln in usage if "mjh_dynamics_kernel" in ln]
    assert len(mine) == 12 and all("ScratchSize [bytes/lane]: 0 " in ln for ln in mine)  # six ops, two dtypes, no scratch


def test_every_case_of_the_issue_is_recorded_and_every_branch_is_covered():
    have = {n: dr.case(n) for n in dr.CASES}
    got = {(c.meta["xml"], c.meta["dtype"]) for c in have.values()}
    assert got >= {("pendula", "float64"), ("pendula", "float32"), ("muscle_arm", "float64"), ("muscle_arm", "float32"), ("ball_free_actuators", "float64"),
                   ("gravcomp_arm", "float64"), ("tendon_fixed", "float64"), ("swimmer", "float64"), ("humanoid", "float64"), ("humanoid", "float32"),
                   ("centipede", "float64"), ("hopper", "float64"), ("halfcheetah", "float64"), ("ant", "float64")}
    assert {0, 1, 2, 3} <= set(have["pendula_f64"].V["jnt_type"].tolist()) and have["pendula_f64"].V["nt"] > 0 and have["pendula_f64"].V["has_gravcomp"]
    assert (have["muscle_arm_f64"].V["actuator_gaintype"] == 2).all() and (have["muscle_arm_f64"].V["actuator_dyntype"] == 4).all()
    assert have["centipede_f64"].V["nb"] == 74 and have["centipede_f64"].V["nv"] == 72
    sw = have["swimmer_fluid_f64"]
    assert sw.V["has_fluid"] and float(sw.V["viscosity"]) == 0.05 and np.allclose(f64(sw.V["wind"]), [0.3, -0.2, 0.1])
    assert have["hopper_nograv_noact_f64"].V["disableflags"] & int(DisableBit.GRAVITY) and have["hopper_nograv_noact_f64"].V["disableflags"] & int(DisableBit.ACTUATION)
    assert have["halfcheetah_nospring_f64"].V["disableflags"] & int(DisableBit.SPRING)
    z = have["ant_zero_mass_fluid_f64"]
    body = int(next(iter(z.meta["model_edits"]["body_mass"])))
    assert z.V["has_fluid"] and z.V["body_mass"][body] == 0 and float(z.compiled.body_mass[body]) > 0 and z.model.tables.uid == z.compiled.tables.uid  # a value-only edit
    assert not (z.V["body_parentid"] == body).any()  # a leaf body
    g = have["gravcomp_arm_f64"]
    assert set(f64(g.V["jnt_actgravcomp"]).tolist()) == {0.0, 1.0} and g.V["jnt_actfrclimited"].any()
    # every branch is taken and not taken in some case's environments
    taken = lambda c, k: min(have[c].branches[k]) > 0
    assert taken("humanoid_f64", "ctrl_clamp") and taken("dynamics_actuators_f64", "ctrl_clamp")
    assert taken("dynamics_actuators_f64", "force_clamp") and taken("dynamics_actuators_f64", "dof_clamp") and taken("dynamics_actuators_f64", "stateful")
    for c in ("pendula_f64", "pendula_f32", "tendon_fixed_f64"):
        assert all(taken(c, k) for k in ("band_below", "band_inside", "band_above")), c
    assert taken("ball_free_actuators_f64", "inparent_ball") and taken("ball_free_actuators_f64", "inparent_free") and taken("gravcomp_arm_f64", "actgravcomp")
    dyn = set(have["dynamics_actuators_f64"].V["actuator_dyntype"].tolist())
    assert dyn == {0, 1, 2, 3} and set(have["dynamics_actuators_f64"].V["actuator_gaintype"].tolist()) == {0, 1}  # NONE, INTEGRATOR, FILTER, FILTEREXACT; FIXED, AFFINE
    for c in have.values():
        assert 2 <= c.nenv <= 3
        for fn, leaves in c.distance.items():
            for n, per_env in leaves.items():
                assert len(per_env) == c.nenv and max(per_env, default=0.0) <= TOL_PRE[c.dtype], (c.name, fn, n)
        for e in range(c.nenv):  # the inputs are edited: no function's inputs are the pass's own
            for fn, L in c.ins[e].items():
                assert all(a.size == 0 or not a.any() or not np.array_equal(a, c.passes[e][n]) for n, a in L.items()), (c.name, fn)
    for f in os.listdir(dr.GOLD):
        assert os.path.getsize(os.path.join(dr.GOLD, f)) < 1 << 20, f


@pytest.mark.parametrize("name", dr.CASES)
def test_the_reference_is_pinned_on_the_recording(name):
    """The longdouble restatement matches every recorded output of the reference, on the edited inputs, within TOL_PRE."""
    c = dr.case(name)
    worst = 0.0
    for e in range(c.nenv):
        for fn in dr.functions(c.V):
            want = dr.FN[fn](c.V, dict(c.passes[e], **c.ins[e][fn]))
            assert set(dr.writes(c.V, fn)) <= set(want), fn
            for n in dr.writes(c.V, fn):
                rec = c.outs[e][fn][n]
                worst = max(worst, rel_err(f64(want[n]).astype(rec.dtype).reshape(rec.shape), rec) / TOL_PRE[c.dtype])
    assert worst <= 1, worst


@pytest.mark.parametrize("name", dr.CASES)
def test_the_reference_chain_reproduces_the_recorded_pass(name):
    """On the recorded UNEDITED pass, each function of the reference module reproduces the pass's own leaves."""
    c = dr.case(name)
    tol = TOL_PRE[c.dtype]
    for e in range(c.nenv):
        P = c.passes[e]
        for fn in dr.functions(c.V):
            out = dr.FN[fn](c.V, P)
            for n in dr.writes(c.V, fn):
                assert rel_err(f64(out[n]).astype(P[n].dtype).reshape(P[n].shape), P[n]) <= tol, (fn, n, e)


def test_the_launch_plan():
    """mjh_dynamics_plan: lanes from nv (TENDON, PASSIVE, ACCELERATION) or nu (TRANSMISSION, VELOCITY, ACTUATION), whole environments in a 256-lane workgroup, the
    reals per environment the header states; a model past a CU's LDS is refused with the sizes."""
    r4 = lambda n: max(4, (n + 3) & ~3)
    table = ((1, 0, 0, 3, 0, F64), (9, 8, 0, 14, 0, F32), (28, 27, 21, 17, 0, F64), (72, 72, 6, 74, 0, F64), (40, 36, 11, 21, 2, F32), (12, 11, 4, 6, 4, F64),
             (2, 2, 3, 3, 0, F32), (124, 121, 40, 123, 0, F32))
    for nq, nv, nu, nb, nt, dtype in table:
        z = dict(nq=nq, nv=nv, nu=nu, nb=nb, nt=nt)
        want = dict(tendon=(nv, nq), transmission=(nu, nq + nt + 3 * nu), velocity=(nu, nv + (nu + nt) * (nv | 1)), passive=(nv, nv + nt + 12 * nb), actuation=(nu, nu),
                    acceleration=(nv, ((nv * (nv + 1) // 2 + 3) & ~3) + nv + 6 * nb))
        for op, (n, reals) in want.items():
            lanes, envs, lds = dynamics.plan(op, z, dtype)
            real = 8 if dtype == F64 else 4
            assert lanes == (16 if n <= 16 else 32 if n <= 32 else 64) and lds == r4(reals), (op, z)
            assert envs == max(1, min(256 // lanes, 64 * 1024 // (lds * real))) and lds * real <= 160 * 1024
            assert dynamics.plan(dynamics.OPS[op], z, dtype) == (lanes, envs, lds)
    with pytest.raises(RuntimeError, match=r"velocity: nq = 257, nv = 256, nu = 256, nbody = 200, ntendon = 0 .* need \d+ bytes of LDS"):
        dynamics.plan("velocity", dict(nq=257, nv=256, nu=256, nb=200, nt=0), F32)
    lib, out = native.load_library(), (ctypes.c_int * 3)()
    assert lib.mjh_dynamics_plan(6, 3, 3, 1, 2, 0, 8, out) == -22 and lib.mjh_dynamics_plan(0, 3, 3, 1, 2, 0, 2, out) == -22
    assert lib.mjh_dynamics_plan(0, 3, 3, 1, 0, 0, 8, out) == -22 and lib.mjh_dynamics_plan(2, 257, 256, 256, 200, 0, 4, out) == -12 and out[2] == 256 + 256 * 257
    for name in ("humanoid_f64", "centipede_f64", "pendula_f32"):
        c = dr.case(name)
        for op in dynamics.OPS:
            assert dynamics.plan(op, c.model, c.dtype)[1] >= 1


@pytest.fixture(scope="module")
def rig():
    c = dr.case("pendula_f64")
    return c.model, c.data(2)


CALLS = {n: getattr(mt, n) for n in dr.FUNCTIONS}
WRONG = dict(tendon="qpos", transmission="ten_J", passive="ten_velocity", fwd_velocity="actuator_moment", fwd_actuation="actuator_length", fwd_acceleration="qLD")


@pytest.mark.parametrize("name", list(CALLS))
def test_cpu_data_is_refused(rig, name):
    mx, d = rig
    with pytest.raises(RuntimeError, match="HIP device"):
        CALLS[name](mx, d)


@pytest.mark.parametrize("name", list(CALLS))
def test_a_float32_data_on_a_float64_model_is_refused(rig, name):
    mx, d = rig
    with pytest.raises(ValueError, match=name + ".*dtype"):
        CALLS[name](mx, d.to(F32))


@pytest.mark.parametrize("name", list(CALLS))
def test_a_wrong_trailing_shape_names_the_function_and_the_leaf(rig, name):
    mx, d = rig
    leaf = WRONG[name]
    with pytest.raises(ValueError, match=rf"{name}: {leaf} has shape"):
        CALLS[name](mx, d.replace(**{leaf: getattr(d, leaf)[..., :-1]}))
    if name == "passive":
        with pytest.raises(ValueError, match="passive: Model.dof_damping has shape"):
            mt.passive(mx.replace(dof_damping=mx.dof_damping[:-1]), d)
    if name == "fwd_actuation":
        with pytest.raises(ValueError, match="fwd_actuation: Model.actuator_gainprm has shape"):
            mt.fwd_actuation(mx.replace(actuator_gainprm=mx.actuator_gainprm[:, :2]), d)


@pytest.mark.parametrize("name", list(CALLS))
def test_a_leaf_of_another_dtype_or_device_is_refused(rig, name):
    """One leaf in float32 beside float64 ones, and one on the meta device beside CPU ones: refused by name before anything else runs."""
    mx, d = rig
    leaf = WRONG[name]
    if leaf != {"tendon": "qpos", "transmission": "qpos", "passive": "qvel", "fwd_velocity": "qvel", "fwd_actuation": "ctrl", "fwd_acceleration": "qfrc_applied"}[name]:
        with pytest.raises(ValueError, match=rf"{name}: {leaf} is torch.float32"):
            CALLS[name](mx, d.replace(**{leaf: getattr(d, leaf).to(F32)}))
        with pytest.raises(ValueError, match=rf"{name}: {leaf} is torch.float64 on meta"):
            CALLS[name](mx, d.replace(**{leaf: getattr(d, leaf).to("meta")}))


@pytest.mark.parametrize("name", list(CALLS))
def test_vmap_is_refused_by_name(rig, name):
    mx, d = rig
    leaf = WRONG[name]
    fn = lambda t: getattr(CALLS[name](mx, d.replace(**{leaf: t})), dr.WRITES[name][0])
    with pytest.raises(NotImplementedError, match=name):
        torch.vmap(fn)(getattr(d, leaf))


def test_the_no_launch_branches_return_what_the_reference_returns():
    c = dr.case("humanoid_f64")
    d = c.data(2)
    assert c.V["nt"] == 0 and mt.tendon(c.model, d) is d
    xml = '<mujoco><worldbody><body pos="0 0 1"><joint type="hinge" axis="0 1 0"/><geom type="sphere" size="0.1" mass="2"/></body></worldbody></mujoco>'
    mc = mt.device_put(mt.mjcf.from_xml_string(xml))
    d1 = mt.make_data(mc).expand(2).clone()
    assert int(mc.nu) == 0 and mt.transmission(mc, d1) is d1 and mt.tendon(mc, d1) is d1
    # the zero branches are decided before the device check: they launch nothing, but a CPU Data is still refused like every other call
    for name, fn in (("hopper_nograv_noact_f64", mt.fwd_actuation), ("halfcheetah_nospring_f64", mt.passive)):
        c = dr.case(name)
        with pytest.raises(RuntimeError, match="HIP device"):
            fn(c.model, c.data(2))
    for name in ("hopper_nograv_noact_f64", "halfcheetah_nospring_f64"):  # ... and the restatement gives the reference's zeros there
        c = dr.case(name)
        fn = "fwd_actuation" if "noact" in name else "passive"
        for e in range(c.nenv):
            for n in dr.writes(c.V, fn):
                assert not c.outs[e][fn][n].any() and not f64(dr.FN[fn](c.V, dict(c.passes[e], **c.ins[e][fn]))[n]).any(), (name, n)
    assert "actuator_force" not in dr.writes(dr.case("hopper_nograv_noact_f64").V, "fwd_actuation")
    assert "qfrc_gravcomp" in dr.writes(dr.case("halfcheetah_nospring_f64").V, "passive") and "qfrc_gravcomp" not in dr.writes(dr.case("humanoid_f64").V, "passive")
