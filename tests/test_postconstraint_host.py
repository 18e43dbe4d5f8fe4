"""rne_postconstraint / subtree_vel / fwd_postconstraint without a GPU: the public functions and their refusals, and the tests' own numpy reference
(tests/_postcon_ref.py) held to closed forms and to the joint-projection identity on forward passes of the CPU oracle (tests/_hostsim.py)."""
import numpy as np
import pytest
import torch

import _hostsim
import _postcon_ref as pr
import _support_ref as sr
import mujoco_torch_amd as mt
from _postcon_ref import IDENTITY_C, within
from _util import load_model

EPS = float(np.finfo(np.float64).eps)
G = 9.81
IDENTITY_MODELS = [("humanoid", {}), ("ant", {"cone": 1}), ("capsules_topk", {}), ("equality", {}), ("cartpole", {})]


@pytest.fixture
def hostsim(monkeypatch):
    return _hostsim.install(monkeypatch)


_PASSES = {}


def loaded_pass(xml, overrides=None, B=4, steps=3):
    """A forward pass of the oracle a few steps after a perturbed pose, with random xfrc_applied (contacts loaded).  Needs the hostsim fixture installed."""
    key = (xml, tuple(sorted((overrides or {}).items())), B, steps)
    if key not in _PASSES:
        mx = load_model(xml, overrides)
        rng = np.random.RandomState(7)
        d = mt.make_data(mx).expand(B).clone()
        d = d.replace(qpos=d.qpos + torch.tensor(0.05 * rng.randn(B, mx.nq)), qvel=torch.tensor(0.3 * rng.randn(B, mx.nv)),
                      xfrc_applied=torch.tensor(2.0 * rng.randn(B, mx.nbody, 6)), ctrl=torch.tensor(0.3 * rng.randn(B, mx.nu)))
        for _ in range(steps):
            d = mt.step(mx, d)
        _PASSES[key] = (mx, mt.forward(mx, d))
    return _PASSES[key]


def xml_pass(xml, qpos=None, qvel=None):
    mx = mt.device_put(mt.mjcf.from_xml_string(xml))
    d = mt.make_data(mx).expand(1).clone()
    if qpos is not None:
        d = d.replace(qpos=torch.tensor([qpos], dtype=torch.float64))
    if qvel is not None:
        d = d.replace(qvel=torch.tensor([qvel], dtype=torch.float64))
    return mx, mt.forward(mx, d)


# ---- the public functions ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def hum():
    mx = load_model("humanoid")
    return mx, mt.make_data(mx).expand(4).clone()


def test_the_three_functions_are_public():
    for n in ("rne_postconstraint", "subtree_vel", "fwd_postconstraint"):
        assert callable(getattr(mt, n)), n
    from mujoco_torch_amd import native

    assert hasattr(native, "PostconArgs") and native.ABI_VERSION >= 16


def test_cpu_data_is_refused(hum):
    mx, d = hum
    for call in (lambda: mt.rne_postconstraint(mx, d), lambda: mt.subtree_vel(mx, d), lambda: mt.fwd_postconstraint(mx, d, sensors=True),
                 lambda: mt.rne_postconstraint(mx, d, qvel=d.qvel.clone())):
        with pytest.raises(RuntimeError, match="HIP device"):
            call()


def test_shapes_dtypes_and_qvel_are_validated(hum):
    mx, d = hum
    nb, nv = int(mx.nbody), int(mx.nv)
    with pytest.raises(ValueError, match="qvel="):
        mt.rne_postconstraint(mx, d, qvel=torch.zeros(nv, dtype=torch.float64))
    with pytest.raises(ValueError, match="qvel="):
        mt.fwd_postconstraint(mx, d, qvel=torch.zeros(4, nv + 1, dtype=torch.float64))
    with pytest.raises(ValueError, match="qvel="):
        mt.rne_postconstraint(mx, d, qvel=torch.zeros(4, nv, dtype=torch.float32))
    with pytest.raises(ValueError, match="qvel="):
        mt.rne_postconstraint(mx, d, qvel=[0.0] * nv)
    with pytest.raises(ValueError, match="cvel"):
        mt.subtree_vel(mx, d.replace(cvel=torch.zeros(4, nb, 5, dtype=torch.float64)))
    with pytest.raises(ValueError, match="cinert"):
        mt.rne_postconstraint(mx, d.replace(cinert=torch.zeros(4, nb, 9, dtype=torch.float64)))
    with pytest.raises(ValueError, match="xipos"):
        mt.fwd_postconstraint(mx, d.replace(xipos=torch.zeros(3, nb, 3, dtype=torch.float64)))
    with pytest.raises(ValueError, match="ximat"):
        mt.subtree_vel(mx, d.replace(ximat=d.ximat.to(torch.float32)))
    with pytest.raises(ValueError, match="dtype"):
        mt.subtree_vel(mx, d.to(torch.float32))


@pytest.mark.parametrize("name", ["rne_postconstraint", "subtree_vel", "fwd_postconstraint"])
def test_vmap_is_refused_by_name(hum, name):
    mx, d = hum
    with pytest.raises(NotImplementedError, match=name):
        torch.vmap(lambda q: getattr(mt, name)(mx, d.replace(qpos=q)).qpos)(d.qpos)
    if name != "subtree_vel":
        with pytest.raises(NotImplementedError, match=name):
            torch.vmap(lambda v: getattr(mt, name)(mx, d, qvel=v).qpos)(d.qvel)


# ---- closed forms on the reference -----------------------------------------------------------------------------------------------------------

_FREE = """<mujoco><option timestep="0.002"/><worldbody>
  <body name="b" pos="0 0 2"><joint type="free"/><geom type="sphere" size="0.1" mass="1.5"/><site name="s" pos="0.03 0.02 0.01" euler="10 20 30"/></body>
</worldbody></mujoco>"""
_FIXED = """<mujoco><worldbody>
  <body name="fixed" pos="0.3 0.2 1"><geom type="box" size="0.1 0.2 0.3" mass="2.5"/><site name="s" pos="0.05 0 0.1"/></body>
  <body name="swing" pos="2 0 1"><joint type="hinge" axis="0 1 0"/><geom type="sphere" size="0.1" pos="0.2 0 0" mass="1"/></body>
</worldbody></mujoco>"""
_ARM = """<mujoco><option gravity="0 0 0"/><worldbody>
  <body name="arm" pos="0 0 1"><joint type="hinge" axis="0 0 1"/><geom type="sphere" size="0.05" pos="0.4 0 0" mass="1"/><site name="s" pos="0.7 0 0"/></body>
</worldbody></mujoco>"""


def _ref(mx, f, **kw):
    return pr.evaluate(pr.tables(mx), pr.leaves_of(f), **kw)


def _accelerometer(mx, f, r, site=0):
    body = int(np.asarray(mx.site_bodyid)[site])
    root = int(np.asarray(mx.body_rootid)[body])
    g = lambda t: t.detach().numpy()[0]
    return pr.site_sensor(pr.ACCELEROMETER, g(f.site_xmat)[site], g(f.site_xpos)[site], g(f.subtree_com)[root], g(f.cvel)[body], cacc=r["cacc"][0][0, body])


@pytest.mark.parametrize("spin", [False, True])
def test_free_fall_has_no_acceleration_and_no_internal_force(hostsim, spin):
    """(cacc is the spatial acceleration: its translational part is the classical acceleration minus omega x v, so it vanishes in free fall only without spin;
    the internal force vanishes either way.)"""
    mx, f = xml_pass(_FREE, qvel=[0.3, -0.2, 0.1] + ([0.5, 0.4, -0.6] if spin else [0, 0, 0]))
    r = _ref(mx, f)
    for k in ("cfrc_int",) if spin else ("cacc", "cfrc_int"):
        v, S, n = r[k]
        sel = (slice(None), 1, slice(3, 6)) if k == "cacc" else (slice(None), 1)
        within(v[sel], 0.0, pr.bound(n, EPS, S)[sel], k)  # (the oracle's qacc carries a few roundings of its own: the same order as one term of S)
    assert np.abs(np.asarray(r["cfrc_ext"][0], dtype=np.float64)).max() == 0
    # the accelerometer: R^T (cacc_lin - dif x cacc_ang) + ang x lin, a few products of quantities bounded by |cvel| (|omega| < 1, |v| < 1) and S(cacc)
    # the site sits off the centre of mass, so under spin it reads the centripetal omega x (omega x r) in its own frame (a sphere's spin is steady), else zero
    om, R = np.array([0.5, 0.4, -0.6]) * spin, f.site_xmat.numpy()[0, 0].reshape(3, 3)
    want = R.T @ np.cross(om, np.cross(om, f.site_xpos.numpy()[0, 0] - f.xipos.numpy()[0, 1]))
    within(_accelerometer(mx, f, r), want, 64 * EPS * (float(r["cacc"][1][0, 1].max()) + 1.0), "accelerometer")


def test_a_body_fixed_to_the_world_feels_gravity(hostsim):
    mx, f = xml_pass(_FIXED)
    r = _ref(mx, f)
    v, S, n = r["cacc"]
    within(v[0, 1], [0, 0, 0, 0, 0, G], pr.bound(n, EPS, S)[0, 1], "cacc")
    v, S, n = r["cfrc_int"]
    within(v[0, 1, 3:], [0, 0, 2.5 * G], pr.bound(n, EPS, S)[0, 1, 3:], "cfrc_int force")
    within(_accelerometer(mx, f, r), [0, 0, G], 64 * EPS * G, "accelerometer")


def test_a_spinning_arm_reads_the_centripetal_acceleration(hostsim):
    w, rad = 3.0, 0.7
    mx, f = xml_pass(_ARM, qvel=[w])
    assert float(f.qacc.abs().max()) < 1e-13  # nothing accelerates the joint
    a = _accelerometer(mx, f, _ref(mx, f))
    within(a, [-w * w * rad, 0, 0], 64 * EPS * w * w * rad, "accelerometer")  # (a dozen roundings in the oracle's kinematics and the reference's formula)


def test_subtree_momenta_of_a_free_sphere(hostsim):
    v, om = [0.3, -0.2, 0.1], [0.5, 0.4, -0.6]
    mx, f = xml_pass(_FREE, qvel=v + om)
    r = _ref(mx, f)
    I = 0.4 * 1.5 * 0.1 ** 2
    for k, want in (("subtree_linvel", v), ("subtree_angmom", [I * x for x in om])):
        val, S, n = r[k]
        within(val[0, 1], want, pr.bound(n, EPS, S)[0, 1] + 16 * EPS * np.abs(want).max(), k)  # (+ the rounding of the oracle's cvel and of I itself)


def test_humanoid_subtree_momentum_is_the_sum_of_body_momenta(hostsim):
    mx, f = loaded_pass("humanoid")
    L = pr.leaves_of(f)
    val, S, n = _ref(mx, f)["subtree_linvel"]
    T = pr.tables(mx)
    mask, root = sr.ancestor_mask(mx.body_parentid, mx.dof_bodyid), np.asarray(mx.body_rootid)
    ids = np.arange(1, T["nbody"])
    (pv, ps), _ = sr.point_velocity_hp(L["cdof"], L["subtree_com"], root, mask, L["xipos"][:, 1:], ids, L["qvel"])
    want, ws = (T["mass"][None, 1:, None] * pv).sum(1), (T["mass"][None, 1:, None] * ps).sum(1)
    sm = T["subtreemass"][1]
    # the left side's bound scaled by the mass, the right side's own: nbody bodies of nv + JACP_ROUNDINGS terms each; cvel itself is the oracle's rounding of the same sums
    allowed = pr.bound(n, EPS, S)[:, 1] * float(sm) + sr.bound(T["nbody"] + int(mx.nv) + sr.JACP_ROUNDINGS, EPS, ws) + sr.bound(int(mx.nv) + sr.JACP_ROUNDINGS, EPS, ws)
    within(val[:, 1] * sm, want, allowed, "subtree momentum")


# ---- the joint-projection identity and the zero-force assumption ---------------------------------------------------------------------------------

def _identity_inputs(mx, f):
    L = pr.leaves_of(f)
    T = pr.tables(mx)
    mask, root = sr.ancestor_mask(mx.body_parentid, mx.dof_bodyid), np.asarray(mx.body_rootid)
    qM = f.qM.numpy()
    jt = np.asarray(sr.xfrc_hp(L["cdof"], L["subtree_com"], L["xipos"], L["xfrc_applied"], root, mask)[0], dtype=np.float64)
    for e in range(qM.shape[0]):
        pts, fo, to, ids = pr.contact_queries(T, L, e, np.float64)
        if len(ids):
            jt[e] += np.asarray(sr.apply_ft_hp(L["cdof"][e:e + 1], L["subtree_com"][e:e + 1], root, mask, pts[None], fo[None], to[None], ids)[0][0].sum(0), dtype=np.float64)
    return L, T, qM, (qM * L["qacc"][:, None, :]).sum(-1), jt


@pytest.mark.parametrize("xml,ov", IDENTITY_MODELS, ids=[m for m, _ in IDENTITY_MODELS])
def test_joint_projection_identity_on_the_reference(hostsim, xml, ov):
    mx, f = loaded_pass(xml, ov)
    assert not np.asarray(mx.tables.source.tendon_armature if int(mx.ntendon) else np.zeros(0)).any()
    L, T, qM, Mq, jt = _identity_inputs(mx, f)
    cint = pr.evaluate(T, L, subtree=False, dtype=np.float64)["cfrc_int"][0]  # the reference evaluated in float64: the rounding the constant is taken from
    ratio, lhs, rhs = pr.identity_ratio(mx, L, cint, Mq, f.qfrc_bias.numpy(), jt, pr.identity_scale(mx, L, qM), EPS)
    print(f"{xml}: identity ratio {ratio:.3f} of eps * sum|terms| over {lhs.size} dofs; largest |lhs| {np.abs(lhs).max():.3e}")
    assert ratio <= IDENTITY_C, (xml, ratio)
    if xml in ("humanoid", "ant", "capsules_topk"):  # the pass is one with loaded contacts
        assert np.abs(np.asarray(pr.evaluate(T, L, subtree=False)["cfrc_ext"][0], dtype=np.float64)).max() > 1e-3


@pytest.mark.parametrize("xml,ov", IDENTITY_MODELS[:4], ids=[m for m, _ in IDENTITY_MODELS[:4]])
def test_slots_without_penetration_carry_no_force(hostsim, xml, ov):
    """What lets cfrc_ext gather every slot without an activity test: the rows of a contact slot whose distance is not below its margin hold zero efc_force."""
    mx, f = loaded_pass(xml, ov)
    L = pr.leaves_of(f)
    dist, margin = f.contact.dist.numpy(), f.contact.includemargin.numpy()
    pyr, seen = int(mx.opt.cone) == 0, 0
    for e in range(dist.shape[0]):
        for c in range(dist.shape[1]):
            dim, adr = int(L["contact_dim"][e, c]), int(L["contact_efc_address"][e, c])
            rows = 2 * (dim - 1) if pyr and dim > 1 else dim
            if L["contact_geom"][e, c, 0] >= 0 and dist[e, c] - margin[e, c] >= 0:
                seen += 1
                assert not L["efc_force"][e, adr:adr + rows].any(), (xml, e, c)
    assert seen > 0
