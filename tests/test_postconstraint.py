"""rne_postconstraint / subtree_vel / fwd_postconstraint on the GPU: the five leaves against the tests' numpy reference (tests/_postcon_ref.py, fed the GPU
pass's own leaves) within its derived bound, the joint-projection identity on device outputs alone, independence of packing and batch cuts, the sensors
against the sensor kernel, the qvel= override, and input safety."""
import numpy as np
import pytest
import torch

import _postcon_ref as pr
import mujoco_torch_amd as mt
from _cases import seeded_batch
from _postcon_ref import IDENTITY_C, within

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64, F32 = torch.float64, torch.float32
_PASSES = {}


def loaded_pass(xml, ov=None, dtype=F64, B=8, steps=3):
    """A forward pass on the GPU a few steps after the seeded pose, with random xfrc_applied (shared by the tests of this module; never written)."""
    key = (xml, tuple(sorted((ov or {}).items())), dtype, B, steps)
    if key not in _PASSES:
        mc, d = seeded_batch(xml, ov or {}, dtype, B)
        rng = np.random.RandomState(5)
        d = d.replace(xfrc_applied=torch.tensor(2.0 * rng.randn(B, int(mc.nbody), 6), dtype=dtype))
        mx, d = mc.to(DEV), d.to(DEV)
        for _ in range(steps):
            d = mt.step(mx, d)
        _PASSES[key] = (mx, mt.forward(mx, d))
    return _PASSES[key]


# condim 4 and 6 with both cones: convex_primitives (condim 4 and 6 pairs), mesh_contact (condim 6)
REF_CASES = [("humanoid", {}, F64, 8), ("ant", {"cone": 1}, F32, 8), ("capsules_topk", {}, F64, 8), ("boxes_topk", {}, F64, 6), ("boxes_topk", {"cone": 1}, F32, 5),
             ("mesh_contact", {}, F64, 4), ("mesh_contact", {"cone": 1}, F32, 4), ("convex_primitives", {}, F64, 4), ("convex_primitives", {"cone": 1}, F64, 3),
             ("cartpole", {}, F64, 8), ("mocap_chain", {}, F64, 5), ("centipede_83", {}, F64, 3), ("centipede_154", {}, F32, 2)]


@pytest.mark.parametrize("xml,ov,dtype,B", REF_CASES, ids=[f"{x}-{'-'.join(f'{k}{v}' for k, v in o.items()) or 'default'}-{str(t)[11:]}" for x, o, t, _ in REF_CASES])
def test_the_five_leaves_against_the_reference(xml, ov, dtype, B):
    mx, f = loaded_pass(xml, ov, dtype, B)
    out = mt.fwd_postconstraint(mx, f)
    ref = pr.evaluate(pr.tables(mx), pr.leaves_of(f))
    eps = torch.finfo(dtype).eps
    nb = int(mx.nbody)
    for k, (v, S, n) in ref.items():
        got = getattr(out, k)
        assert tuple(got.shape) == (B, nb, v.shape[-1]) and got.dtype == dtype, k
        worst = float((np.abs(got.cpu().numpy().astype(pr.HP) - v).astype(np.float64) / np.maximum(pr.bound(n, eps, S), 1e-300)).max())
        print(f"{xml} {k}: worst error {worst:.3f} of its bound; max |value| {float(np.abs(v).max()):.3e}")
        within(got.cpu().numpy(), v, pr.bound(n, eps, S), f"{xml} {k}")
    if xml in ("humanoid", "ant", "capsules_topk", "boxes_topk", "mesh_contact", "convex_primitives", "centipede_83", "centipede_154"):
        assert float(out.cfrc_ext.abs().max()) > 0 and float(f.efc_force.abs().max()) > 0, "the pass carries no contact force"
    if xml == "cartpole":
        assert f.efc_force.numel() == 0


def _jt_ext_on_device(mx, f, L, T):
    """J^T cfrc_ext with the library's own support functions: xfrc_accumulate + apply_ft of every contact's wrench (environment by environment: max_contact_points
    models pick their slots, hence the body ids, per environment)."""
    jt = mt.xfrc_accumulate(mx, f).clone()
    dt = L["cdof"].dtype
    for e in range(jt.shape[0]):
        pts, fo, to, ids = pr.contact_queries(T, L, e, dt)
        if len(ids):
            t = lambda a: torch.tensor(a[None], device=DEV)
            jt[e] += mt.apply_ft(mx, f[e:e + 1], t(fo), t(to), t(pts), [int(i) for i in ids])[0].sum(0)
    return jt


IDENTITY_CASES = [("humanoid", {}, F64, 8), ("ant", {"cone": 1}, F32, 8), ("capsules_topk", {}, F64, 8), ("equality", {}, F64, 4), ("cartpole", {}, F64, 8)]


@pytest.mark.parametrize("xml,ov,dtype,B", IDENTITY_CASES, ids=[c[0] for c in IDENTITY_CASES])
def test_joint_projection_identity_on_device_outputs(xml, ov, dtype, B):
    """cdof[i] . cfrc_int[b] = (qM qacc)[i] - armature[i] qacc[i] + qfrc_bias[i] - (J^T cfrc_ext)[i] for every dof, every side computed on the device
    (rne_postconstraint, mul_m, xfrc_accumulate, apply_ft); the host only forms the contacts' wrenches and the sum of |terms| the constant multiplies."""
    mx, f = loaded_pass(xml, ov, dtype, B)
    out = mt.rne_postconstraint(mx, f)
    L, T = pr.leaves_of(f), pr.tables(mx)
    Mq, jt = mt.mul_m(mx, f, f.qacc), _jt_ext_on_device(mx, f, L, T)
    ratio, lhs, _ = pr.identity_ratio(mx, L, out.cfrc_int.cpu().numpy(), Mq.cpu().numpy(), f.qfrc_bias.cpu().numpy(), jt.cpu().numpy(),
                                      pr.identity_scale(mx, L, f.qM.cpu().numpy()), torch.finfo(dtype).eps)
    print(f"{xml}: identity ratio {ratio:.3f} of eps * sum|terms| over {lhs.size} dofs")
    assert ratio <= IDENTITY_C, (xml, ratio)


def _equal(a, b, names):
    for n in names:
        assert torch.equal(getattr(a, n), getattr(b, n)), n


FIVE = ("cacc", "cfrc_int", "cfrc_ext", "subtree_linvel", "subtree_angmom")


@pytest.mark.parametrize("xml,ov,dtype", [("humanoid", {}, F64), ("ant", {"cone": 1}, F32), ("centipede_83", {}, F64)], ids=["humanoid", "ant", "centipede_83"])
def test_results_do_not_depend_on_packing_or_cuts(xml, ov, dtype):
    B = 70
    mx, f = loaded_pass(xml, ov, dtype, B, steps=2)
    full = mt.fwd_postconstraint(mx, f)
    for sl in (slice(4, 5), slice(9, 12), slice(2, 69)):  # 1, 3 and 67 environments
        part = mt.fwd_postconstraint(mx, f[sl])
        for n in FIVE:
            assert torch.equal(getattr(part, n), getattr(full, n)[sl]), (n, sl)
    two = mt.subtree_vel(mx, mt.rne_postconstraint(mx, f))
    _equal(two, full, FIVE)


def _dependent_slots(mx):
    s = mx.tables.sensors
    slot = np.asarray(s["slot"])
    types = np.asarray(s["type"])
    return np.array([k >= 0 and int(types[k]) in (pr.ACCELEROMETER, pr.FORCE, pr.TORQUE, pr.SUBTREELINVEL, pr.SUBTREEANGMOM) for k in slot])


@pytest.mark.parametrize("xml,dtype", [("sensor_rig", F64), ("sensor_rig2", F64), ("sensor_rig2", F32)])
def test_sensors_match_the_sensor_kernel_on_the_fresh_leaves(xml, dtype):
    """forward() evaluates the same sensors from the leaves its INPUT carries, so the yardstick is a second pass from the same input state with the fresh leaves
    handed in: both passes start from the same state, hence hold the same kinematic leaves bit for bit (asserted; a pass over its own output would renormalise
    qpos again, which moves last bits in float32), and every bit of difference would be the new kernel's."""
    mx, state = loaded_pass(xml, {}, dtype, 9, steps=2)
    KIN = ("qpos", "cvel", "site_xpos", "site_xmat", "subtree_com", "qacc", "efc_force")
    f = mt.forward(mx, state)
    dep = torch.tensor(_dependent_slots(mx), device=DEV)
    assert dep.any() and not dep.all()
    out = mt.fwd_postconstraint(mx, f, sensors=True)
    _equal(out, mt.fwd_postconstraint(mx, f), FIVE)
    again = mt.forward(mx, state.replace(**{n: getattr(out, n) for n in FIVE}))
    _equal(again, f, KIN)
    diff = (out.sensordata != again.sensordata) & dep
    print(f"{xml} {dtype}: {int(dep.sum())} dependent slots, differing: {diff.any(0).nonzero().flatten().tolist()}")
    assert torch.equal(out.sensordata[:, dep], again.sensordata[:, dep])
    assert torch.equal(out.sensordata[:, ~dep], f.sensordata[:, ~dep])
    if xml == "sensor_rig2":  # (the pass itself read the caller's leaves, which the seeded batch randomises)
        assert not torch.equal(out.sensordata[:, dep], f.sensordata[:, dep])
    if xml == "sensor_rig":  # the accelerometer's cutoff of 0.05 clamps
        assert float(out.sensordata[:, dep].abs().max()) == 0.05


def test_a_resting_rover_is_held_by_its_contact_force():
    """sensor_rig with the hull pressed into the floor, at rest: the bodies' m (classical acceleration + g), summed over the rover's subtree, is the contact force --
    Newton's law for the free root.  A pass obeys it as far as its solver converged, so the check has two parts: the difference equals the solver's own residual
    M qacc - qfrc_smooth - qfrc_constraint on the root's translational dofs (from the pass's leaves, on the device) within C eps sum|terms| -- nothing else is
    applied to those dofs --, and that residual is below what the solver's gradient test lets through, opt.tolerance * meaninertia * nv.  Then the accelerometer
    slot holds the formula's value under the sensor's cutoff."""
    from _util import load_model

    mc = load_model("sensor_rig")
    mx = mc.to(DEV)
    d = mt.make_data(mc).expand(2).clone()
    q = d.qpos.clone()
    q[:, 2] = torch.tensor([0.195, 0.19])
    f = mt.forward(mx, d.replace(qpos=q).to(DEV))
    out = mt.fwd_postconstraint(mx, f, sensors=True)
    g = lambda t: t.cpu().numpy().astype(np.float64)
    cacc, ext, xip, com, mass = g(out.cacc), g(out.cfrc_ext), g(f.xipos), g(f.subtree_com), g(mx.body_mass)
    assert (ext[:, 1, 5] > 1.0).all(), "no contact force on the hull"
    total, scale = np.zeros((2, 3)), np.zeros((2, 3))
    for b in (1, 2):
        r = xip[:, b] - com[:, 1]
        total += mass[b] * (cacc[:, b, 3:] + np.cross(cacc[:, b, :3], r))
        scale += mass[b] * (np.abs(cacc[:, b, 3:]) + np.abs(cacc[:, b, [1, 2, 0]] * r[:, [2, 0, 1]]) + np.abs(cacc[:, b, [2, 0, 1]] * r[:, [1, 2, 0]]))
    force = ext[:, 1, 3:] + ext[:, 2, 3:]
    resid = g(mt.mul_m(mx, f, f.qacc) - f.qfrc_smooth - f.qfrc_constraint)[:, :3]
    eps = np.finfo(np.float64).eps
    S = scale + np.abs(force) + pr.identity_scale(mx, pr.leaves_of(f), g(f.qM))[:, :3] + np.abs(g(f.qfrc_smooth))[:, :3] + np.abs(g(f.qfrc_constraint))[:, :3]
    print(f"rover: |m (a + g) - F| {np.abs(total - force).max():.3e}, solver residual {np.abs(resid).max():.3e}, difference {np.abs(total - force - resid).max():.3e}")
    within(total - force, resid, IDENTITY_C * eps * S, "m (a + g) - contact force against the solver's residual")
    assert np.abs(resid).max() <= float(mc.opt.tolerance) * float(mc.stat.meaninertia) * int(mc.nv)
    types, adr = list(np.asarray(mx.tables.sensors["type"])), np.asarray(mx.tables.sensors["adr"])
    k = types.index(pr.ACCELEROMETER)
    slot, site = int(adr[k]), int(np.asarray(mx.tables.sensors["objid"])[k])
    for e in range(2):  # the slot holds the formula's value under the sensor's cutoff of 0.05
        a = pr.site_sensor(pr.ACCELEROMETER, g(f.site_xmat)[e, site], g(f.site_xpos)[e, site], com[e, 1], g(f.cvel)[e, 1], cacc=cacc[e, 1])
        within(g(out.sensordata)[e, slot:slot + 3], np.clip(np.asarray(a, dtype=np.float64), -0.05, 0.05), 64 * np.finfo(np.float64).eps * np.abs(cacc[e, 1]).max(), "accelerometer")


def test_the_qvel_override_gives_the_pre_step_leaves():
    mx, f = loaded_pass("humanoid", {}, F64, 8)
    s = mt.step(mx, f)
    assert not torch.equal(s.qvel, f.qvel)
    got = mt.rne_postconstraint(mx, s, qvel=f.qvel)
    # step ran the same pass on the same state, warm-started differently: with its qacc / efc_force copied over, f is the pre-step pass bit for bit
    want = mt.rne_postconstraint(mx, f.replace(qacc=s.qacc, efc_force=s.efc_force))
    _equal(got, want, ("cacc", "cfrc_int", "cfrc_ext"))
    _equal(mt.fwd_postconstraint(mx, s, qvel=f.qvel), got, ("cacc", "cfrc_int", "cfrc_ext"))
    plain = mt.rne_postconstraint(mx, s)
    assert not torch.equal(plain.cacc, got.cacc) and not torch.equal(plain.cfrc_int, got.cfrc_int)


def test_the_input_is_not_written_and_the_other_leaves_alias_it():
    mx, f = loaded_pass("sensor_rig2", {}, F64, 9, steps=2)
    names = [n for n in pr.LEAVES if not n.startswith("contact_")] + ["sensordata", "site_xpos", "site_xmat"] + list(FIVE)
    before = {n: getattr(f, n).clone() for n in names}
    out = mt.fwd_postconstraint(mx, f, sensors=True)
    for n, t in before.items():
        assert torch.equal(getattr(f, n), t), n
    for n in ("qpos", "qvel", "cvel", "qM", "efc_force", "xfrc_applied"):
        assert getattr(out, n).data_ptr() == getattr(f, n).data_ptr(), n
    assert out.contact.pos.data_ptr() == f.contact.pos.data_ptr()
    for n in FIVE + ("sensordata",):
        assert getattr(out, n).data_ptr() != getattr(f, n).data_ptr(), n
    only = mt.subtree_vel(mx, f)
    assert only.cacc.data_ptr() == f.cacc.data_ptr() and only.sensordata.data_ptr() == f.sensordata.data_ptr()


def test_refusals_on_the_device():
    mx, f = loaded_pass("humanoid", {}, F64, 8)
    nv = int(mx.nv)
    with pytest.raises(ValueError, match="qvel="):
        mt.rne_postconstraint(mx, f, qvel=torch.zeros(nv, dtype=F64, device=DEV))
    with pytest.raises(ValueError, match="qvel="):
        mt.fwd_postconstraint(mx, f, qvel=f.qvel.cpu())
    with pytest.raises(ValueError, match="cvel"):
        mt.subtree_vel(mx, f.replace(cvel=f.cvel[:, :, :5]))
    with pytest.raises(ValueError, match="cinert"):
        mt.rne_postconstraint(mx, f.replace(cinert=f.cinert.float()))
    with pytest.raises(NotImplementedError, match="subtree_vel"):
        torch.vmap(lambda q: mt.subtree_vel(mx, f.replace(qpos=q)).qpos)(f.qpos)
    with pytest.raises(RuntimeError, match="HIP device"):
        mt.subtree_vel(mx.to("cpu"), f.to("cpu"))
