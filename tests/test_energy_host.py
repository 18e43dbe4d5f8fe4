"""energy / the limit and energy sensors without a GPU: the public functions and their refusals, and the tests' own numpy reference (tests/_energy_ref.py) -- the
yardstick of tests/test_energy.py -- held to closed forms, to the forces the step applies (the potential's finite differences against qfrc_bias - qfrc_passive), to
the bodies' kinetic energies and to hand-placed limit states, all on forward passes of the CPU oracle.

Measured here (printed by the tests): finite differences, worst |dV/2h - (bias - passive)| / (1 + |dV/2h|): tendon_fixed 3.2e-9, tendon_armature 3.2e-9,
hopper 6.7e-10, cartpole 2.1e-10, halfcheetah 1.5e-9, pendula (ball / free dofs) 2.1e-9, limit_energy_rig (every dof) 1.1e-9; kinetic energy against the bodies,
worst share of the bound: humanoid 2.5e-4, pendula 9.2e-5."""
import re

import numpy as np
import pytest
import torch

import _energy_ref as er
import _fd_ref as fr
import _postcon_ref as pr
import mujoco_torch_amd as mt
import pyoracle
from _energy_ref import HP
from _util import load_model

U64 = 2.0 ** -53
G = 9.81


def oracle_pass(mx, d):
    """{leaf: array [B, ...]} of the CPU oracle's forward pass on the batched Data `d`, with the state it ran on."""
    out = dict(pyoracle.run(mx, d, step=False))
    out["qpos"], out["qvel"] = d.qpos.numpy().copy(), d.qvel.numpy().copy()
    return out


def leaves(out):
    B = out["qpos"].shape[0]
    return {n: np.asarray(out[n]).reshape(B, -1) if n != "xipos" else np.asarray(out[n]).reshape(B, -1, 3) for n in er.LEAVES}


def data(mx, qpos=None, qvel=None, B=1):
    d = mt.make_data(mx).expand(B).clone()
    kw = {}
    if qpos is not None:
        kw["qpos"] = torch.tensor(np.asarray(qpos, dtype=np.float64)).reshape(B, -1)
    if qvel is not None:
        kw["qvel"] = torch.tensor(np.asarray(qvel, dtype=np.float64)).reshape(B, -1)
    return d.replace(**kw)


@pytest.fixture(scope="module")
def rig():
    mx = load_model("limit_energy_rig")
    return mx, mt.make_data(mx).expand(3).clone()


# ---- the public functions ----------------------------------------------------------------------------------------------------------------

def test_the_functions_and_the_entry_point_are_public():
    from mujoco_torch_amd import native

    for n in ("energy", "energy_pos", "energy_vel", "sensor_postconstraint"):
        assert callable(getattr(mt, n)), n
    assert hasattr(native, "EnergyArgs") and native.ABI_VERSION >= 18
    text = open(native.HEADER).read()
    assert re.search(r"\bint mjh_energy\s*\(const mjhModel\* m, const mjhEnergyArgs\* args, void\* hip_stream\);", text)
    assert re.search(r"#define MJH_KERNEL_ENERGY 34\b", text)
    for i, n in enumerate(("POS", "VEL", "SENSORS")):
        assert re.search(rf"#define MJH_ENERGY_{n} {1 << i}\b", text)
    body = text[text.index("typedef struct mjhEnergyArgs {"):text.index("} mjhEnergyArgs;")]
    fields = re.findall(r"[*\s,](\w+)(?=[,;])", body.split("{", 1)[1])
    assert fields == [f[0] for f in native.EnergyArgs._fields_], fields


def test_the_sensors_have_a_table_of_their_own(rig):
    mx, _ = rig
    T = mx.tables.energy_sensors
    rows = np.asarray(T["rows"])
    assert sorted(set(rows[:, 0].tolist())) == list(er.TYPES)
    assert not set(np.asarray(mx.tables.sensors["type"]).tolist()) & set(er.TYPES)  # (no pass evaluates them)
    V = er.model_values(mx)
    want = er.limit_rows(V)
    ref = [(t, adr, obj, -1 if t in (er.EPOT, er.EKIN) else want.get(("tendon" if t >= er.TLPOS else "jnt", obj), -1), dt) for t, adr, obj, dt, _ in V["sensors"]]
    assert [tuple(r[:5]) for r in rows.tolist()] == ref and T["index"].tolist() == list(range(len(ref)))
    assert {r[3] for r in rows.tolist() if r[0] in (er.JLPOS, er.TLPOS)} == {-1, 0, 1, 2, 3}  # ball, hinge, slide, tendon and the two unlimited objects
    for flag in (1 << 13, ):  # DisableBit.SENSOR
        assert len(load_model("limit_energy_rig", {"disableflags": flag}).tables.energy_sensors["rows"]) == 0
    off = load_model("limit_energy_rig", {"disableflags": 1 << 3})  # DisableBit.LIMIT: no rows, the sensors give 0
    assert set(np.asarray(off.tables.energy_sensors["rows"])[:, 3].tolist()) == {-1}
    two = np.asarray(load_model("sensor_rig2").tables.energy_sensors["rows"])
    assert two[:, 0].tolist() == [er.JLPOS, er.EPOT]


def test_cpu_data_is_refused(rig):
    mx, d = rig
    for call in (lambda: mt.energy(mx, d), lambda: mt.energy_pos(mx, d, qpos=d.qpos.clone()), lambda: mt.energy_vel(mx, d, qvel=d.qvel.clone()),
                 lambda: mt.sensor_postconstraint(mx, d, all_sensors=True)):
        with pytest.raises(RuntimeError, match="HIP device"):
            call()


def test_shapes_and_dtypes_are_validated(rig):
    mx, d = rig
    with pytest.raises(ValueError, match="xipos"):
        mt.energy(mx, d.replace(xipos=d.xipos[:, :-1]))
    with pytest.raises(ValueError, match="qM"):
        mt.energy(mx, d.replace(qM=d.qM[:, :-1]))
    with pytest.raises(ValueError, match="ten_length"):
        mt.energy_pos(mx, d.replace(ten_length=d.ten_length.to(torch.float32)))
    with pytest.raises(ValueError, match="dtype"):
        mt.energy(mx, d.to(torch.float32))
    with pytest.raises(ValueError, match="qpos="):
        mt.energy(mx, d, qpos=torch.zeros(int(mx.nq), dtype=torch.float64))
    with pytest.raises(ValueError, match="qvel="):
        mt.energy_vel(mx, d, qvel=d.qvel.to(torch.float32))
    with pytest.raises(ValueError, match="efc_J"):
        mt.sensor_postconstraint(mx, d.replace(efc_J=d.efc_J[:, :-1]), all_sensors=True)
    with pytest.raises(ValueError, match="body_mass"):
        mt.energy(mx.replace(body_mass=mx.body_mass[:-1]), d)
    with pytest.raises(TypeError):
        mt.sensor_postconstraint(mx, d, None, True)  # (keyword only)


@pytest.mark.parametrize("name", ["energy", "energy_pos", "energy_vel", "sensor_postconstraint"])
def test_vmap_is_refused_by_name(rig, name):
    mx, d = rig
    fn = (lambda q: mt.sensor_postconstraint(mx, d.replace(qpos=q), all_sensors=True).qpos) if name == "sensor_postconstraint" else (
        lambda q: getattr(mt, name)(mx, d.replace(qpos=q)))
    with pytest.raises(NotImplementedError, match=name):
        torch.vmap(fn)(d.qpos)


def test_the_tendon_values_come_from_the_compiled_model(rig):
    """Model carries no tendon_stiffness / tendon_lengthspring / tendon_range / tendon_margin, so these four cannot be edited with mx.replace: a call takes them
    from the compiled model the tables keep (shared by every value-only copy), in the model's dtype; the Model's own fields are taken from the caller's Model."""
    from mujoco_torch_amd.energy import _values

    mx, _ = rig
    names = ("tendon_stiffness", "tendon_lengthspring", "tendon_range", "tendon_margin")
    assert not any(hasattr(mx, n) for n in names)
    edited = mx.replace(body_mass=2 * mx.body_mass, jnt_margin=mx.jnt_margin + 0.5)
    assert edited.tables is mx.tables
    for dtype in (torch.float64, torch.float32):
        v = _values("energy", edited, dtype, torch.device("cpu"), cutoff_of=mx.tables.energy_sensors["index"])
        for n in names:
            want = torch.tensor(np.asarray(getattr(mx.tables.source, n), dtype=np.float64)).to(dtype)
            assert v[n].dtype == dtype and torch.equal(v[n], want), n
        assert float(v["tendon_stiffness"][0]) == 8 and v["tendon_lengthspring"].tolist()[0] == torch.tensor([-0.02, 0.05], dtype=torch.float64).to(dtype).tolist()
        assert torch.equal(v["body_mass"], (2 * mx.body_mass).to(dtype)) and torch.equal(v["jnt_margin"], (mx.jnt_margin + 0.5).to(dtype))
        assert torch.equal(v["sns_cutoff"], torch.tensor(np.asarray(mx.sensor_cutoff)[mx.tables.energy_sensors["index"]]).to(dtype))
    # a sensor_cutoff held as a tensor is gathered as it is
    v = _values("energy", mx.replace(sensor_cutoff=torch.tensor(np.asarray(mx.sensor_cutoff)) * 2), torch.float64, torch.device("cpu"), cutoff_of=mx.tables.energy_sensors["index"])
    assert v["sns_cutoff"].tolist()[:3] == [0.0, 0.5, 3.0]


def test_limit_sensors_compile_on_a_ball_joint():
    """MuJoCo accepts jointlimitpos / vel / frc on any joint; jointpos / jointvel stay slide / hinge only."""
    xml = """<mujoco><worldbody><body><joint name="b" type="ball" range="0 1"/><geom size="0.1"/></body></worldbody>
             <sensor><{tag} joint="b"/></sensor></mujoco>"""
    for tag in ("jointlimitpos", "jointlimitvel", "jointlimitfrc"):
        assert int(mt.mjcf.from_xml_string(xml.format(tag=tag)).nsensordata) == 1
    with pytest.raises(ValueError, match="slide or hinge"):
        mt.mjcf.from_xml_string(xml.format(tag="jointpos"))


# ---- 1. closed forms ---------------------------------------------------------------------------------------------------------------------------

def test_cartpole_energies_by_hand():
    """cart 1 kg on a slide along x, pole 0.1 kg with its centre 0.3 m from the hinge (tests/test_host_api.py): V = -sum m g . c, T = the two bodies' translation
    plus the pole's rotation about its centre."""
    mx = load_model("cartpole")
    x, th, vx, w = 0.1, 0.7, 0.4, -1.3
    out = oracle_pass(mx, data(mx, [x, th], [vx, w]))
    (en, A, n) = er.evaluate(mx, leaves(out))["energy"]
    xi = out["xipos"].reshape(-1, 3)
    mass = np.asarray(mx.body_mass)
    assert abs(mass[1] - 1.0) < 1e-12 and abs(mass[2] - 0.1) < 1e-12
    V = mass[1] * G * xi[1, 2] + mass[2] * G * xi[2, 2]
    assert abs(float(en[0, 0]) - V) <= er.bound(n[0, 0], U64, A[0, 0]) + 8 * U64 * abs(V)
    # the pole's centre sits 0.3 from the hinge: its height follows the angle (about the y axis, from the upright pose)
    assert abs((xi[2, 2] - xi[1, 2]) - 0.3 * np.cos(th)) < 1e-12
    M, _ = mt.mjcf.mass_matrix0(mx.tables.source, np.array([x, th]))
    l, m = 0.3, 0.1
    T = 0.5 * 1.1 * vx * vx + m * l * np.cos(th) * vx * w + 0.5 * M[1, 1] * w * w
    print(f"cartpole: V {float(en[0, 0]):.12f} by hand {V:.12f}; T {float(en[0, 1]):.12f} by hand {T:.12f}")
    assert abs(float(en[0, 1]) - T) <= er.bound(n[0, 1], U64, A[0, 1]) + 64 * U64 * abs(T)  # (+ the oracle's own mass matrix)
    assert n[0, 0] == 6 and n[0, 1] == 4


_PENDULUM = """<mujoco><compiler angle="radian"/><option timestep="0.002"/><worldbody>
  <body pos="0 0 2"><joint name="h" type="hinge" axis="0 1 0" stiffness="4" springref="0.3" armature="0.05"/>
    <geom type="sphere" size="0.05" pos="0 0 -0.5" mass="2"/></body>
</worldbody></mujoco>"""


def test_a_hinge_pendulum_by_hand():
    """A point-like bob (sphere, mass 2, inertia 2/5 m r^2) 0.5 below a y hinge at height 2, spring 4 about 0.3 rad, armature 0.05."""
    mx = mt.device_put(mt.mjcf.from_xml_string(_PENDULUM))
    q, w = 0.9, 1.7
    out = oracle_pass(mx, data(mx, [q], [w]))
    (en, A, n) = er.evaluate(mx, leaves(out))["energy"]
    m, l, r = 2.0, 0.5, 0.05
    V = m * G * (2 - l * np.cos(q)) + 0.5 * 4 * (q - 0.3) ** 2
    T = 0.5 * (m * l * l + 0.4 * m * r * r + 0.05) * w * w
    print(f"pendulum: V {float(en[0, 0]):.12f} by hand {V:.12f}; T {float(en[0, 1]):.12f} by hand {T:.12f}")
    assert abs(float(en[0, 0]) - V) <= er.bound(n[0, 0], U64, A[0, 0]) + 64 * U64 * abs(V)  # (+ the oracle's kinematics)
    assert abs(float(en[0, 1]) - T) <= er.bound(n[0, 1], U64, A[0, 1]) + 64 * U64 * abs(T)
    assert n[0, 0] == 4 and n[0, 1] == 1
    # gravity off: the spring alone; springs off (either flag, as the step): gravity alone
    for flag, want in ((1 << 7, 0.5 * 4 * (q - 0.3) ** 2), (1 << 5, m * G * (2 - l * np.cos(q))), (1 << 6, m * G * (2 - l * np.cos(q)))):
        lite = mt.mjcf.from_xml_string(_PENDULUM)
        lite.opt.disableflags = flag
        mo = mt.device_put(lite)
        v = er.evaluate(mo, leaves(oracle_pass(mo, data(mo, [q], [w]))))["energy"][0][0, 0]
        assert abs(float(v) - want) < 1e-12 * (1 + abs(want)), (flag, float(v), want)


# ---- 2. the potential is the potential of the forces the step applies ------------------------------------------------------------------------------

FD_H, FD_TOL = 1e-6, 1e-7
FD_MODELS = [("tendon_fixed", "hinge_slide"), ("tendon_armature", "hinge_slide"), ("hopper", "hinge_slide"), ("cartpole", "hinge_slide"), ("halfcheetah", "hinge_slide"),
             ("pendula", "ball_free"), ("limit_energy_rig", "all")]


@pytest.mark.parametrize("xml,which", FD_MODELS, ids=[c[0] for c in FD_MODELS])
def test_the_potential_differentiates_to_the_applied_forces(xml, which):
    """qvel = 0, ctrl = 0: along every tangent direction, (V(q + h e) - V(q - h e)) / 2h = qfrc_bias - qfrc_passive at that dof (h = 1e-6, float64; the floor of
    the difference itself -- truncation and eps / h rounding -- is what 1e-7 allows).  Models with gravity compensation or fluid forces are left out (those
    forces have no potential here); pendula's gravity-compensated chain is, too: its ball and free dofs are checked."""
    mx = load_model(xml)
    jt = fr.Joints(er._np(mx.jnt_type), er._np(mx.jnt_qposadr), er._np(mx.jnt_dofadr), mx.nq, mx.nv)
    dof_type = np.concatenate([[t] * {er.FREE: 6, er.BALL: 3}.get(int(t), 1) for t in jt.type]).astype(np.int64)
    dofs = [i for i in range(jt.nv) if which == "all" or (dof_type[i] in (er.SLIDE, er.HINGE)) == (which == "hinge_slide")]
    assert dofs
    rng = np.random.RandomState(3)
    q0 = fr.integrate(jt, np.asarray(mx.qpos0, dtype=np.float64), 0.3 * rng.randn(jt.nv), 1.0)
    steps = np.zeros((2 * len(dofs), jt.nv))
    for i, dof in enumerate(dofs):
        steps[2 * i, dof], steps[2 * i + 1, dof] = FD_H, -FD_H
    qs = np.concatenate([q0[None], fr.integrate(jt, np.broadcast_to(q0, (len(steps), jt.nq)), steps, 1.0)])
    out = oracle_pass(mx, data(mx, qs, B=len(qs)))
    V = np.asarray(er.evaluate(mx, leaves(out))["energy"][0][:, 0], dtype=np.float64)
    dV = (V[1::2] - V[2::2]) / (2 * FD_H)
    force = (out["qfrc_bias"][0] - out["qfrc_passive"][0])[dofs]
    err = np.abs(dV - force) / (1 + np.abs(dV))
    print(f"{xml}: {len(dofs)} dofs, worst |dV/2h - (bias - passive)| / (1 + |dV/2h|) = {err.max():.2e}; |force| up to {np.abs(force).max():.3g}")
    assert np.abs(force).max() > 1e-3  # (something pulls)
    assert err.max() <= FD_TOL, (dofs, err)


# ---- 3. kinetic energy against the bodies ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("xml", ["humanoid", "pendula"])
def test_kinetic_energy_is_the_sum_over_the_bodies(xml):
    """1/2 qvel^T qM qvel = 1/2 sum_b cvel_b^T I_b cvel_b (cinert) + 1/2 sum dof_armature qvel^2, within 4 n u A of the reference."""
    mx = load_model(xml)
    rng = np.random.RandomState(11)
    B = 3
    d = mt.make_data(mx).expand(B).clone()
    jt = fr.Joints(er._np(mx.jnt_type), er._np(mx.jnt_qposadr), er._np(mx.jnt_dofadr), mx.nq, mx.nv)
    q = fr.integrate(jt, np.broadcast_to(np.asarray(mx.qpos0, dtype=np.float64), (B, jt.nq)), 0.4 * rng.randn(B, jt.nv), 1.0)
    out = oracle_pass(mx, data(mx, q, rng.randn(B, jt.nv), B=B))
    (en, A, n) = er.evaluate(mx, leaves(out))["energy"]
    arm = np.asarray(mx.dof_armature, dtype=np.float64).astype(HP)
    tarm = np.asarray(getattr(mx.tables.source, "tendon_armature", np.zeros(0)), dtype=np.float64).astype(HP) if int(mx.ntendon) else np.zeros(0, dtype=HP)
    for e in range(B):
        cvel, cin = out["cvel"][e].reshape(-1, 6).astype(HP), out["cinert"][e].reshape(-1, 10).astype(HP)
        T = sum(cvel[b] @ pr._inert_mul(cin[b], cvel[b], -1) for b in range(1, int(mx.nbody))) / 2 + (arm * out["qvel"][e].astype(HP) ** 2).sum() / 2
        T = T + (tarm * out["ten_velocity"][e].astype(HP) ** 2).sum() / 2  # (tendon armature sits in qM too)
        allowed = er.bound(n[e, 1], U64, A[e, 1])
        print(f"{xml} env {e}: T {float(en[e, 1]):.12f}, over the bodies {float(T):.12f}, |difference| / bound {abs(float(en[e, 1] - T)) / allowed:.2e}")
        assert n[e, 1] == int(mx.nv) ** 2 and abs(float(en[e, 1] - T)) <= allowed


# ---- 4. the limit rules ----------------------------------------------------------------------------------------------------------------------------

RIG_SENSORS = ("hinge_pos", "hinge_vel", "hinge_frc", "ball_pos", "ball_vel", "ball_frc", "slide_pos", "slide_vel", "slide_frc", "swing_pos", "swing_frc",
               "couple_pos", "couple_vel", "couple_frc", "loose_pos", "loose_vel", "epot", "ekin")  # tests/golden/limit_energy_rig.xml, in order


def _rig_states(mx):
    """Three states placed by hand: beyond every range, inside the margins only, well inside."""
    q0 = np.asarray(mx.qpos0, dtype=np.float64)
    adr = {n: int(er._np(mx.jnt_qposadr)[i]) for i, n in enumerate(mx.tables.source.names_jnt)}
    axis = np.array([0.0, 0.6, 0.8])
    states = []
    for hinge, ball, slide, swing in ((0.6, 0.8, 0.25, 0.0), (0.47, 0.69, -0.195, 1.675), (0.0, 0.2, 0.0, 0.0)):
        q = q0.copy()
        q[adr["hinge"]], q[adr["slide"]], q[adr["swing"]] = hinge, slide, swing
        q[adr["ball"]:adr["ball"] + 4] = np.concatenate([[np.cos(ball / 2)], np.sin(ball / 2) * axis])
        states.append(q)
    return np.array(states), adr


def test_the_limit_rules_on_states_placed_by_hand(rig):
    mx, _ = rig
    qs, adr = _rig_states(mx)
    dof = {n: int(er._np(mx.jnt_dofadr)[i]) for i, n in enumerate(mx.tables.source.names_jnt)}
    qvel = np.zeros((3, int(mx.nv)))
    qvel[:, dof["hinge"]], qvel[:, dof["slide"]], qvel[:, dof["swing"]] = 1.0, 0.3, -0.5
    qvel[:, dof["ball"]:dof["ball"] + 3] = [0.2, -0.1, 0.4]
    out = oracle_pass(mx, data(mx, qs, qvel, B=3))
    res = er.evaluate(mx, leaves(out))
    names = RIG_SENSORS
    assert len(names) == len(res["sensors"]) == int(mx.nsensor)
    S = {n: np.asarray(s["value"], dtype=np.float64) for n, s in zip(names, res["sensors"])}
    row = {n: s["row"] for n, s in zip(names, res["sensors"])}
    print({n: v.tolist() for n, v in S.items()})
    close = lambda got, want: np.allclose(got, want, rtol=0, atol=1e-12)
    # positions: dist - margin beyond the range and inside the margin, 0 well inside
    assert close(S["hinge_pos"], [-0.1 - 0.05, 0.03 - 0.05, 0]) and close(S["slide_pos"], [-0.05 - 0.01, 0.005 - 0.01, 0])
    assert close(S["ball_pos"], [-0.1 - 0.02, 0.01 - 0.02, 0])
    assert close(S["couple_pos"], [(0.15 - 0.25) - 0.02, (0.15 - 0.14) - 0.02, 0])
    # an object without a row gives 0: the unlimited joint and tendon
    assert row["swing_pos"] == row["loose_pos"] == -1
    for n in ("swing_pos", "swing_frc", "loose_pos", "loose_vel"):
        assert not S[n].any(), n
    # velocities: the row's sign times the velocity where the limit is active, 0 where the pass zeroed the row; the cutoff clamps a real sensor
    assert close(S["hinge_vel"], [-0.25, -0.25, 0])  # -qvel = -1 at the upper side, clamped to the cutoff 0.25
    assert close(S["slide_vel"], [-0.3, 0.3, 0])    # upper side, lower side
    ax = np.array([0.0, 0.6, 0.8])
    assert close(S["ball_vel"], [-(ax @ [0.2, -0.1, 0.4])] * 2 + [0])
    assert close(S["couple_vel"], [-(0.3 + 0.2 * -0.5)] * 2 + [0])
    # forces: efc_force[row]; the cutoff bounds a positive-typed sensor from above only
    f = out["efc_force"].reshape(3, -1)
    assert f[0, row["hinge_frc"]] > 1.5 and S["hinge_frc"][0] == 1.5 and S["hinge_frc"][2] == 0
    assert 0 < f[1, row["hinge_frc"]] and S["hinge_frc"][1] == min(f[1, row["hinge_frc"]], 1.5)
    for n in ("ball_frc", "slide_frc", "couple_frc"):
        assert np.array_equal(S[n], f[:, row[n]]) and S[n][0] > 0 and S[n][1] >= 0 and S[n][2] == 0, n  # (beyond the range it pushes back)
    # the energy sensors are the energies
    assert np.array_equal(S["epot"], np.asarray(res["energy"][0][:, 0], dtype=np.float64)) and np.array_equal(S["ekin"], np.asarray(res["energy"][0][:, 1], dtype=np.float64))
    # limits disabled: every limit sensor gives 0
    off = load_model("limit_energy_rig", {"disableflags": 1 << 3})
    res = er.evaluate(off, leaves(oracle_pass(off, data(off, qs, qvel, B=3))))
    assert all(not np.asarray(s["value"]).any() for s in res["sensors"] if s["type"] not in (er.EPOT, er.EKIN))
