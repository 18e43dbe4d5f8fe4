"""energy / energy_pos / energy_vel and sensor_postconstraint(all_sensors=True) on the GPU against the tests' numpy reference (tests/_energy_ref.py, pinned on the
CPU by tests/test_energy_host.py).  The leaves come from the product's own forward pass on the device, so the reference and the kernel read the same bits; the
tolerance is derived, |got - ref| <= 4 n u A with n and A from the reference (u = 2^-53 / 2^-24); jointlimitfrc / tendonlimitfrc are efc_force[row] bit for bit.
Batches of 67 (no multiple of any environments-per-workgroup), 3, 1 and the batch shape (2, 3); environment i of the 67 equals the same state run alone, bit for
bit; every slot outside the eight sensor types is all_sensors=False's; a value-only edit of body_mass is honoured without a new native model; qpos= / qvel= on a
step output reproduce the pre-step forward's values.

Measured on an MI355X (printed by the tests), worst |got - ref| / (4 n u A) over the 67 environments, (V, T): cartpole (0.036, 0.119), humanoid float64
(0.024, 0.0009), float32 (0.014, 0.0013), tendon_fixed (0.029, 0.0064), pendula (0.0033, 0.0005), sensor_rig2 (0.031, 0.0060), limit_energy_rig float64
(0.017, 0.0051), float32 (0.017, 0.0043), centipede_83 (0.0041, 0.00007).  limit_energy_rig, environments of 67 with a non-zero value: hinge pos / vel / frc
18 / 18 / 17, ball 29 / 29 / 19, slide 42 / 42 / 40, tendon 49 / 49 / 19, the unlimited joint and tendon 0; sensor_rig2's jointlimitpos 11."""
import numpy as np
import pytest
import torch

import _energy_ref as er
import _fd_ref as fr
import mujoco_torch_amd as mt
from _cases import seeded_batch
from _util import load_model

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64, F32 = torch.float64, torch.float32
B = 67
FIVE = ("cacc", "cfrc_int", "cfrc_ext", "subtree_linvel", "subtree_angmom")
_PASSES = {}

CASES = [("cartpole", F64), ("humanoid", F64), ("humanoid", F32), ("tendon_fixed", F64), ("pendula", F64), ("sensor_rig2", F64), ("limit_energy_rig", F64),
         ("limit_energy_rig", F32), ("centipede_83", F64)]
_SPREAD = {"cartpole": 0.5, "humanoid": 0.3, "tendon_fixed": 0.4, "pendula": 0.5, "limit_energy_rig": 0.4, "centipede_83": 0.3}
_ids = lambda cases: [f"{c[0]}-{str(c[1])[11:]}" for c in cases]


def a_pass(xml, dtype):
    """(host model, device model, the device's forward pass of B = 67 seeded states; shared by the tests of this module, never written).  sensor_rig2: the seeded
    batch (it sets the sensordata the caller owns); every other model: qpos0 moved along a random tangent (joints pass their ranges, springs and tendons stretch),
    random velocities."""
    key = (xml, dtype)
    if key not in _PASSES:
        if xml == "sensor_rig2":
            mc, d = seeded_batch(xml, {}, dtype, B)
        else:
            mc = load_model(xml, {}, dtype)
            rng = np.random.RandomState(17)
            jt = fr.Joints(er._np(mc.jnt_type), er._np(mc.jnt_qposadr), er._np(mc.jnt_dofadr), mc.nq, mc.nv)
            q = fr.integrate(jt, np.broadcast_to(np.asarray(mc.qpos0, dtype=np.float64), (B, jt.nq)), _SPREAD[xml] * rng.randn(B, jt.nv), 1.0)
            d = mt.make_data(mc).expand(B).clone()
            d = d.replace(qpos=torch.tensor(q), qvel=torch.tensor(0.8 * rng.randn(B, jt.nv)), sensordata=torch.tensor(rng.randn(B, int(mc.nsensordata))))
            d = d if dtype == F64 else d.to(dtype)
        mx = mc.to(DEV)
        _PASSES[key] = (mc, mx, mt.forward(mx, d.to(DEV)))
    return _PASSES[key]


_REFS = {}


def reference(xml, dtype):
    if (xml, dtype) not in _REFS:
        mc, _, f = a_pass(xml, dtype)
        _REFS[(xml, dtype)] = er.evaluate(mc, er.leaves_of(f))
    return _REFS[(xml, dtype)]


def _worst(got, val, A, n, u):
    """The largest |got - ref| / (4 n u A) (0 / 0 = 0), asserting nothing."""
    err = np.abs(np.asarray(got, dtype=er.HP) - val).astype(np.float64)
    allowed = er.bound(n, u, A)
    return float(np.max(np.where(err == 0, 0.0, err / np.where(allowed > 0, allowed, np.finfo(np.float64).tiny)))), err, allowed


# ---- the energies ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("xml,dtype", CASES, ids=_ids(CASES))
def test_energy_against_the_reference(xml, dtype):
    mc, mx, f = a_pass(xml, dtype)
    val, A, n = reference(xml, dtype)["energy"]
    u = er.U[dtype]
    got = mt.energy(mx, f)
    assert tuple(got.shape) == (B, 2) and got.dtype == dtype and got.device.type == "cuda"
    ratio, err, allowed = _worst(got.cpu().numpy(), val, A, n, u)
    print(f"{xml} {dtype}: V in [{float(val[:, 0].min()):.4g}, {float(val[:, 0].max()):.4g}], T up to {float(val[:, 1].max()):.4g}; n = {n[0].tolist()}; "
          f"worst |got - ref| / (4 n u A) = {ratio:.3g} (V {float((err[:, 0] / np.maximum(allowed[:, 0], 1e-300)).max()):.3g}, "
          f"T {float((err[:, 1] / np.maximum(allowed[:, 1], 1e-300)).max()):.3g})")
    assert float(np.abs(val[:, 1]).min()) > 0 and np.abs(np.asarray(val[:, 0], dtype=np.float64)).max() > 0
    assert (err <= allowed).all(), (err / np.maximum(allowed, 1e-300)).max(0)
    # the halves, and the other batches: the same bits
    assert torch.equal(mt.energy_pos(mx, f), got[:, 0]) and torch.equal(mt.energy_vel(mx, f), got[:, 1])
    assert torch.equal(mt.energy(mx, f[:3]), got[:3]) and torch.equal(mt.energy(mx, f[5:6]), got[5:6])
    f23 = torch.stack([f[7:10], f[10:13]])
    six = mt.energy(mx, f23)
    assert tuple(six.shape) == (2, 3, 2) and torch.equal(six.reshape(6, 2), got[7:13])
    assert tuple(mt.energy_pos(mx, f23).shape) == (2, 3)


@pytest.mark.parametrize("xml,dtype", [("humanoid", F64), ("limit_energy_rig", F32), ("centipede_83", F64), ("pendula", F64)], ids=["humanoid", "rig-f32", "centipede_83", "pendula"])
def test_an_environment_of_a_batch_equals_the_same_state_alone(xml, dtype):
    """Fixed summation order, no dependence on B, on the slot in the workgroup or on how the batch is cut: bit for bit."""
    _, mx, f = a_pass(xml, dtype)
    full = mt.energy(mx, f)
    sens = mt.sensor_postconstraint(mx, f, all_sensors=True).sensordata if int(mx.nsensordata) else None
    for i in (0, 1, 15, 16, 33, 66):
        assert torch.equal(mt.energy(mx, f[i:i + 1]), full[i:i + 1]), i
        if sens is not None:
            assert torch.equal(mt.sensor_postconstraint(mx, f[i:i + 1], all_sensors=True).sensordata, sens[i:i + 1]), i
    assert torch.equal(mt.energy(mx, f[3:64]), full[3:64])


def test_a_value_only_edit_is_honoured_without_a_new_native_model():
    from mujoco_torch_amd._postpass import handle as _handle

    mc, mx, f = a_pass("humanoid", F64)
    nm = _handle(mx, f.qpos.device, F64)
    base = mt.energy_pos(mx, f)
    heavy = mx.replace(body_mass=2 * mx.body_mass)
    got = mt.energy_pos(heavy, f)
    assert _handle(heavy, f.qpos.device, F64) is nm  # (the same native model serves the edited one)
    V = er.model_values(mc)
    heavy_ref = [er.potential(dict(V, body_mass=2 * V["body_mass"]), q, x, np.zeros(0)) for q, x in
                 zip(f.qpos.cpu().numpy().astype(er.HP), f.xipos.cpu().numpy().astype(er.HP))]
    val, A, n = (np.array([r[k] for r in heavy_ref]) for k in range(3))  # (the edited model's own terms)
    err = np.abs(got.cpu().numpy().astype(er.HP) - val).astype(np.float64)
    assert (err <= er.bound(n, er.U[F64], A)).all()
    # the gravity part alone (the joint springs taken out of both models): doubling the masses doubles it to the last bit
    assert V["jnt_stiffness"].any() and not torch.equal(got, 2 * base)
    zero = torch.zeros_like(mx.jnt_stiffness)
    g1, g2 = mt.energy_pos(mx.replace(jnt_stiffness=zero), f), mt.energy_pos(heavy.replace(jnt_stiffness=zero), f)
    assert torch.equal(g2, 2 * g1) and float(g1.abs().min()) > 0
    assert torch.allclose(got - base, g1, rtol=1e-12, atol=0)  # (what the edit added is the gravity part once more)
    # gravity and the spring values are the caller's too
    nograv = mx.opt.replace(gravity=torch.zeros_like(mx.opt.gravity))
    assert not mt.energy_pos(mx.replace(jnt_stiffness=zero, opt=nograv), f).any()
    springs = mt.energy_pos(mx.replace(opt=nograv), f)
    assert float(springs.min()) > 0 and torch.allclose(springs + g1, base, rtol=1e-12, atol=0)
    _, rx, rf = a_pass("limit_energy_rig", F64)
    stiff = rx.replace(jnt_stiffness=3 * rx.jnt_stiffness, opt=rx.opt.replace(gravity=torch.zeros_like(rx.opt.gravity)))
    soft = rx.replace(opt=rx.opt.replace(gravity=torch.zeros_like(rx.opt.gravity)))
    tend = rx.replace(jnt_stiffness=0 * rx.jnt_stiffness, opt=rx.opt.replace(gravity=torch.zeros_like(rx.opt.gravity)))
    a, b, c = mt.energy_pos(stiff, rf), mt.energy_pos(soft, rf), mt.energy_pos(tend, rf)
    assert torch.allclose(a - c, 3 * (b - c), rtol=1e-12, atol=0) and float((b - c).min()) > 0 and float(c.max()) > 0


def test_qpos_and_qvel_on_a_step_output_reproduce_the_pre_step_values():
    for xml in ("limit_energy_rig", "humanoid"):
        _, mx, f = a_pass(xml, F64)
        s = mt.step(mx, f)
        want = mt.energy(mx, f)
        assert not torch.equal(s.qpos, f.qpos) and not torch.equal(s.qvel, f.qvel)
        assert torch.equal(mt.energy(mx, s, qpos=f.qpos, qvel=f.qvel), want)
        assert torch.equal(mt.energy_pos(mx, s, qpos=f.qpos), want[:, 0]) and torch.equal(mt.energy_vel(mx, s, qvel=f.qvel), want[:, 1])
        assert not torch.equal(mt.energy(mx, s), want)  # (the advanced state is another one)
        if int(mx.nsensordata):
            ws, gs = mt.sensor_postconstraint(mx, f, all_sensors=True).sensordata, mt.sensor_postconstraint(mx, s, qvel=f.qvel, all_sensors=True).sensordata
            rows = np.asarray(mx.tables.energy_sensors["rows"])
            vel = torch.tensor([int(r[1]) for r in rows if r[0] in (er.JLVEL, er.TLVEL, er.EKIN)], device=DEV)
            assert torch.equal(gs[:, vel], ws[:, vel])  # (the limit velocities and the kinetic energy are the pre-step state's)
            assert not torch.equal(mt.sensor_postconstraint(mx, s, all_sensors=True).sensordata[:, vel], ws[:, vel])
            for r in rows:  # the forces are the step's own solve (its warm start is another one): efc_force[row] of the step output, bit for bit
                if r[0] in (er.JLFRC, er.TLFRC) and r[3] >= 0 and float(mx.sensor_cutoff[int(mx.tables.energy_sensors["index"][list(rows[:, 1]).index(r[1])])]) == 0:
                    assert torch.equal(gs[:, int(r[1])], s.efc_force[:, int(r[3])]), r.tolist()


# ---- the sensors -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("xml,dtype", [("limit_energy_rig", F64), ("limit_energy_rig", F32), ("sensor_rig2", F64)], ids=["rig-f64", "rig-f32", "sensor_rig2"])
def test_the_energy_sensors_are_energy_bit_for_bit(xml, dtype):
    """The lanes per environment follow from the model and the size of its sensor table in both kinds of call (the rig: 7 bodies, 12 dofs, 18 sensors -> 32 lanes),
    so the partial sums are the same ones: the e_potential / e_kinetic slots (no cutoff on them in these models) are energy's bits."""
    mc, mx, f = a_pass(xml, dtype)
    en, sd = mt.energy(mx, f), mt.sensor_postconstraint(mx, f, all_sensors=True).sensordata
    rows, index = np.asarray(mc.tables.energy_sensors["rows"]), np.asarray(mc.tables.energy_sensors["index"])
    seen = 0
    for r, i in zip(rows, index):
        if r[0] in (er.EPOT, er.EKIN):
            assert float(mc.sensor_cutoff[i]) == 0
            assert torch.equal(sd[:, int(r[1])], en[:, 0 if r[0] == er.EPOT else 1]), r.tolist()
            seen += 1
    assert seen == (2 if xml == "limit_energy_rig" else 1)


def _slots(mx):
    rows = np.asarray(mx.tables.energy_sensors["rows"])
    mask = np.zeros(int(mx.nsensordata), dtype=bool)
    mask[rows[:, 1]] = True
    return torch.tensor(mask, device=DEV)


SENSOR_CASES = [("limit_energy_rig", F64), ("limit_energy_rig", F32), ("sensor_rig2", F64)]


@pytest.mark.parametrize("xml,dtype", SENSOR_CASES, ids=_ids(SENSOR_CASES))
def test_all_sensors_against_the_reference(xml, dtype):
    mc, mx, f = a_pass(xml, dtype)
    ref = reference(xml, dtype)
    u = er.U[dtype]
    plain, got = mt.sensor_postconstraint(mx, f), mt.sensor_postconstraint(mx, f, all_sensors=True)
    new = _slots(mx)
    assert new.any() and int(new.sum()) == len(ref["sensors"]) and (xml == "limit_energy_rig") == bool(new.all())  # (the rig declares these sensors only)
    # every other slot and leaf: all_sensors=False's, bit for bit; its slots of these types stay the caller's
    assert torch.equal(got.sensordata[:, ~new], plain.sensordata[:, ~new])
    for n in FIVE:
        assert torch.equal(getattr(got, n), getattr(plain, n)), n
    assert torch.equal(plain.sensordata[:, new], f.sensordata[:, new]) and not torch.equal(got.sensordata[:, new], f.sensordata[:, new])
    assert torch.equal(mt.sensor_postconstraint(mx, f, all_sensors=False).sensordata, plain.sensordata)
    sd, force = got.sensordata.cpu().numpy(), f.efc_force.cpu().numpy()
    active = {}
    for s in ref["sensors"]:
        g = sd[:, s["adr"]]
        if s["type"] in (er.JLFRC, er.TLFRC):
            assert np.array_equal(g, np.asarray(s["value"], dtype=sd.dtype)), s  # efc_force[row] after the cutoff, bit for bit
            if s["row"] >= 0 and not any(c[4] > 0 for c in er.model_values(mc)["sensors"] if c[1] == s["adr"]):
                assert np.array_equal(g, force[:, s["row"]])
        else:
            ratio, err, allowed = _worst(g, s["value"], s["A"], s["n"], u)
            assert (err <= allowed).all(), (s["type"], s["adr"], ratio)
        active[(s["type"], s["adr"])] = int(np.count_nonzero(g))
    print(f"{xml} {dtype}: environments (of {B}) with a non-zero value per (type, slot): {active}")
    if xml == "limit_energy_rig":  # every kind of limit is met and missed, an object without a row reads 0
        rows = np.asarray(mc.tables.energy_sensors["rows"])
        for r in rows:
            k = active[(int(r[0]), int(r[1]))]
            assert (k == 0) if (r[3] < 0 and r[0] not in (er.EPOT, er.EKIN)) else (0 < k < B or r[0] in (er.EPOT, er.EKIN)), (r.tolist(), k)
    # other batches: the same bits
    assert torch.equal(mt.sensor_postconstraint(mx, f[:3], all_sensors=True).sensordata, got.sensordata[:3])
    assert torch.equal(mt.sensor_postconstraint(mx, torch.stack([f[7:10], f[10:13]]), all_sensors=True).sensordata.reshape(6, -1), got.sensordata[7:13])


def test_limits_disabled_and_models_without_these_sensors():
    mc = load_model("limit_energy_rig", {"disableflags": 1 << 3})  # DisableBit.LIMIT: no rows, every limit sensor reads 0
    _, _, f0 = a_pass("limit_energy_rig", F64)
    mx = mc.to(DEV)
    d = mt.make_data(mc).expand(5).clone().to(DEV).replace(qpos=f0.qpos[:5].clone(), qvel=f0.qvel[:5].clone())
    f = mt.forward(mx, d)
    got = mt.sensor_postconstraint(mx, f, all_sensors=True).sensordata
    rows = np.asarray(mc.tables.energy_sensors["rows"])
    lim = torch.tensor([int(r[1]) for r in rows if r[0] not in (er.EPOT, er.EKIN)], device=DEV)
    assert not got[:, lim].any() and got[:, [int(r[1]) for r in rows if r[0] == er.EKIN]].abs().min() > 0
    _, hx, hf = a_pass("humanoid", F64)  # no such sensors: the call is all_sensors=False's
    assert torch.equal(mt.sensor_postconstraint(hx, hf[:4], all_sensors=True).sensordata, mt.sensor_postconstraint(hx, hf[:4]).sensordata)


def test_the_input_is_not_written_and_refusals_on_the_device():
    _, mx, f = a_pass("limit_energy_rig", F64)
    names = er.LEAVES + ("sensordata",)
    before = {n: getattr(f, n).clone() for n in names}
    mt.energy(mx, f), mt.sensor_postconstraint(mx, f, all_sensors=True)
    for n, t in before.items():
        assert torch.equal(getattr(f, n), t), n
    with pytest.raises(ValueError, match="qM"):
        mt.energy(mx, f.replace(qM=f.qM.float()))
    with pytest.raises(ValueError, match="qpos="):
        mt.energy(mx, f, qpos=f.qpos.cpu())
    with pytest.raises(NotImplementedError, match="energy"):
        torch.vmap(lambda q: mt.energy(mx, f.replace(qpos=q)))(f.qpos)
    with pytest.raises(RuntimeError, match="HIP device"):
        mt.energy(mx.to("cpu"), f.to("cpu"))
    assert tuple(mt.energy(mx, f[:0]).shape) == (0, 2)
