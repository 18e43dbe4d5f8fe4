"""jac_dot / jac_subtree_com / angmom_mat and the body / site / geom Jacobians without a GPU: the public functions and their refusals, and the tests' own numpy
reference (tests/_jacobian_ref.py) -- the yardstick of tests/test_jacobian.py -- held to the definition of jac_dot by finite differences of jac along the motion, to
subtree_vel's definitions (tests/_postcon_ref.py) and to closed forms, all on forward passes of the CPU oracle.

Measured here (printed by the tests): jac_dot against the Richardson-combined centred differences of jac (eps = 1e-3), worst error / allowed error: pendula 1.7e-3,
ball_limits 1.9e-6, humanoid 2.8e-4.  With the stored cdof_dot on the ball joints' dofs instead of the motion cross product with the body's own velocity the same
check misses its bound on ball_limits (test_the_stored_cdof_dot_of_a_ball_joint_is_not_the_derivative)."""
import re

import numpy as np
import pytest
import torch

import _fd_ref as fr
import _jacobian_ref as jr
import _postcon_ref as pr
import _support_ref as sr
import mujoco_torch_amd as mt
import pyoracle
from _jacobian_ref import HP
from _util import load_model

U64 = 2.0 ** -53
FD_EPS = 1e-3
NAMES = ("jac_body", "jac_body_com", "jac_site", "jac_geom", "jac_subtree_com", "jac_dot", "angmom_mat")


def oracle_pass(mx, qpos, qvel):
    """{leaf: array [B, ...]} of the CPU oracle's forward pass on the states (qpos [B, nq], qvel [B, nv])."""
    B = qpos.shape[0]
    d = mt.make_data(mx).expand(B).clone().replace(qpos=torch.tensor(np.asarray(qpos, dtype=np.float64)), qvel=torch.tensor(np.asarray(qvel, dtype=np.float64)))
    out = dict(pyoracle.run(mx, d, step=False))
    out["qvel"] = np.asarray(qvel, dtype=np.float64)
    return out


def joints(mx):
    return fr.Joints(jr._np(mx.jnt_type), jr._np(mx.jnt_qposadr), jr._np(mx.jnt_dofadr), mx.nq, mx.nv)


def moved_state(mx, seed, B=1, scale=0.4):
    jt = joints(mx)
    rng = np.random.RandomState(seed)
    q = fr.integrate(jt, np.broadcast_to(np.asarray(mx.qpos0, dtype=np.float64), (B, jt.nq)), scale * rng.randn(B, jt.nv), 1.0)
    return q, rng.randn(B, jt.nv), rng


@pytest.fixture(scope="module")
def pendula():
    mx = load_model("pendula")
    return mx, mt.make_data(mx).expand(3).clone()


# ---- the public functions ----------------------------------------------------------------------------------------------------------------

def test_the_functions_and_the_entry_point_are_public():
    import inspect

    from mujoco_torch_amd import jacobian, native

    for n in NAMES:
        assert callable(getattr(mt, n)) and getattr(mt, n) is getattr(jacobian, n), n
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(mt.jac_body) == sig(mt.jac_body_com) == ["m", "d", "body_id", "vec"] and sig(mt.jac_site) == ["m", "d", "site_id", "vec"]
    assert sig(mt.jac_geom) == ["m", "d", "geom_id", "vec"] and sig(mt.jac_subtree_com) == sig(mt.angmom_mat) == ["m", "d", "body_id", "vec"]
    assert sig(mt.jac_dot) == ["m", "d", "point", "body_id", "vec"]
    assert all(inspect.signature(getattr(mt, n)).parameters["vec"].default is None for n in NAMES)
    assert hasattr(native, "JacobianArgs") and native.ABI_VERSION >= 20
    text = open(native.HEADER).read()
    assert re.search(r"\bint mjh_jacobian\s*\(const mjhModel\* m, const mjhJacobianArgs\* args, void\* hip_stream\);", text)
    for i, n in enumerate(("POINT", "DOT", "SUBTREE_COM", "ANGMOM")):
        assert re.search(rf"#define MJH_JACOBIAN_{n} {i}\b", text) and re.search(rf"#define MJH_KERNEL_JACOBIAN_{n} {36 + i}\b", text)
        assert re.search(rf"#define MJH_KERNEL_JACOBIAN_{n}_VEC {40 + i}\b", text)
    assert (jacobian.POINT, jacobian.DOT, jacobian.SUBTREE_COM, jacobian.ANGMOM) == (0, 1, 2, 3)
    assert re.search(r"#define MJH_KERNEL_INTEGRATE 35\b", text)
    body = text[text.index("typedef struct mjhJacobianArgs {"):text.index("} mjhJacobianArgs;")]
    fields = re.findall(r"[*\s,](\w+)(?=[,;])", body.split("{", 1)[1])
    assert fields == [f[0] for f in native.JacobianArgs._fields_], fields


def test_cpu_data_is_refused(pendula):
    mx, d = pendula
    pt = torch.zeros(3, dtype=torch.float64)
    calls = [lambda: mt.jac_body(mx, d, 1), lambda: mt.jac_body_com(mx, d, [1, 2]), lambda: mt.jac_geom(mx, d, 0), lambda: mt.jac_body(mx, d, 1, vec=d.qvel),
             lambda: mt.jac_subtree_com(mx, d, 0), lambda: mt.jac_subtree_com(mx, d, [0, 1], vec=d.qvel), lambda: mt.jac_dot(mx, d, pt, 1),
             lambda: mt.jac_dot(mx, d, pt, 1, vec=d.qvel), lambda: mt.angmom_mat(mx, d, 1), lambda: mt.angmom_mat(mx, d, 1, vec=d.qvel)]
    if int(mx.nsite):
        calls.append(lambda: mt.jac_site(mx, d, 0))
    for call in calls:
        with pytest.raises(RuntimeError, match="HIP device"):
            call()


def test_arguments_and_shapes_are_validated(pendula):
    mx, d = pendula
    nb, nv, ng = int(mx.nbody), int(mx.nv), int(mx.ngeom)
    pt = torch.zeros(3, dtype=torch.float64)
    for call in (lambda: mt.jac_body(mx, d, nb), lambda: mt.jac_body_com(mx, d, -1), lambda: mt.jac_subtree_com(mx, d, [0, nb]), lambda: mt.angmom_mat(mx, d, nb),
                 lambda: mt.jac_dot(mx, d, pt, nb)):
        with pytest.raises(ValueError, match=rf"outside \[0, {nb}\)"):
            call()
    with pytest.raises(ValueError, match=rf"jac_geom: geom ids \[{ng}\] are outside \[0, {ng}\)"):
        mt.jac_geom(mx, d, ng)
    with pytest.raises(ValueError, match=r"jac_site: site ids .* are outside"):
        mt.jac_site(mx, d, int(mx.nsite))
    with pytest.raises(ValueError, match="per-environment"):
        mt.jac_subtree_com(mx, d, torch.zeros(3, 2, dtype=torch.int64))
    with pytest.raises(ValueError, match="integers"):
        mt.angmom_mat(mx, d, torch.zeros(2))
    with pytest.raises(ValueError, match="point must have shape"):
        mt.jac_dot(mx, d, torch.zeros(4, dtype=torch.float64), 1)
    with pytest.raises(ValueError, match="2 body ids for 3 points"):
        mt.jac_dot(mx, d, torch.zeros(3, 3, 3, dtype=torch.float64), [1, 2])
    with pytest.raises(ValueError, match="vec="):
        mt.jac_subtree_com(mx, d, 1, vec=torch.zeros(nv, dtype=torch.float64))
    with pytest.raises(ValueError, match="vec="):
        mt.jac_dot(mx, d, pt, 1, vec=d.qvel.to(torch.float32))
    with pytest.raises(ValueError, match="vec="):
        mt.jac_body(mx, d, 1, vec=d.qvel[:, :-1])
    with pytest.raises(ValueError, match="cdof_dot"):
        mt.jac_dot(mx, d.replace(cdof_dot=d.cdof_dot[:, :-1]), pt, 1)
    with pytest.raises(ValueError, match="ximat"):
        mt.angmom_mat(mx, d.replace(ximat=d.ximat.to(torch.float32)), 1)
    with pytest.raises(ValueError, match="xipos"):
        mt.jac_subtree_com(mx, d.replace(xipos=d.xipos[:, :-1]), 1)
    with pytest.raises(ValueError, match="dtype"):
        mt.jac_subtree_com(mx, d.to(torch.float32), 1)
    with pytest.raises(ValueError, match="body_mass"):
        mt.jac_subtree_com(mx.replace(body_mass=mx.body_mass[:-1]), d, 1)
    with pytest.raises(ValueError, match="body_inertia"):
        mt.angmom_mat(mx.replace(body_inertia=mx.body_inertia[:-1]), d, 1)
    with pytest.raises(ValueError, match="positions have shape"):
        mt.jac_body(mx, d.replace(xpos=d.xpos[:, :-1]), 1)


def test_a_subtree_without_mass_is_refused(pendula):
    mx, d = pendula
    sm = jr._np(mx.body_subtreemass).copy()
    sm[2] = 0
    empty = mx.replace(body_subtreemass=torch.tensor(sm))
    for fn in (mt.jac_subtree_com, mt.angmom_mat):
        with pytest.raises(ValueError, match=r"subtree of body 2 has no mass"):
            fn(empty, d, [1, 2])
        with pytest.raises(ValueError, match=r"subtree of body 2 has no mass"):
            fn(empty, d, 2, vec=d.qvel)
        with pytest.raises(RuntimeError, match="HIP device"):  # (the other bodies pass the check)
            fn(empty, d, 1)


@pytest.mark.parametrize("name", NAMES)
def test_vmap_is_refused_by_name(pendula, name):
    mx, d = pendula
    pt = torch.zeros(3, dtype=torch.float64)
    if name == "jac_dot":
        fn = lambda c: mt.jac_dot(mx, d.replace(cdof=c), pt, 1)[0]
    elif name in ("jac_subtree_com", "angmom_mat"):
        fn = lambda c: getattr(mt, name)(mx, d.replace(cdof=c), 1)
    else:
        fn = lambda c: getattr(mt, name)(mx, d.replace(cdof=c), 0)[0]
    with pytest.raises(NotImplementedError, match=name):
        torch.vmap(fn)(d.cdof)


# ---- 1. jac_dot is the time derivative of jac --------------------------------------------------------------------------------------------------------

def _fd_case(xml, seed=5):
    """The state, the oracle passes at qpos (+) eps' qvel for eps' = 0, +-eps, +-eps / 2 (qvel kept), one point per body carried by the body's frame."""
    mx = load_model(xml)
    T = jr.tables(mx)
    jt = joints(mx)
    q0, v, rng = moved_state(mx, seed)
    steps = np.array([0, FD_EPS, -FD_EPS, FD_EPS / 2, -FD_EPS / 2])
    qs = np.stack([fr.integrate(jt, q0[0], v[0], h) for h in steps])
    out = oracle_pass(mx, qs, np.broadcast_to(v, (5, jt.nv)).copy())
    L = jr.leaves_of(out)
    nb = T["nbody"]
    xpos, xmat = np.asarray(out["xpos"]).reshape(5, nb, 3), np.asarray(out["xmat"]).reshape(5, nb, 3, 3)
    pts = xpos + np.einsum("ebrc,bc->ebr", xmat, 0.3 * rng.randn(nb, 3))
    return T, L, pts, np.arange(nb)


def _fd_ratio(T, L, pts, ids, dot):
    """Worst |dot - Richardson| / allowed over jacp and jacr; allowed = 4 |FD(eps) - FD(eps / 2)| + eps_machine |J| / eps: the difference's own measured error."""
    J = sr.jac_same(L["cdof"], L["subtree_com"], T["root"], T["mask"], pts, ids)
    worst = 0.0
    for Jk, D in zip(J, dot):
        f1, f2 = (Jk[1] - Jk[2]) / (2 * FD_EPS), (Jk[3] - Jk[4]) / FD_EPS
        rich = (4 * f2 - f1) / 3
        allowed = 4 * np.abs(f1 - f2) + 2 * U64 * np.abs(Jk[0]) / FD_EPS
        err = np.abs(np.asarray(D[0], dtype=np.float64) - rich)
        assert np.abs(rich).max() > 1e-2  # (something moves)
        ratio = np.where(err > allowed, np.inf, err / np.where(allowed > 0, allowed, 1.0))
        assert not (err[allowed == 0] > 0).any()
        worst = max(worst, float(ratio.max()))
    return worst


@pytest.mark.parametrize("xml", ["pendula", "ball_limits", "humanoid"])
def test_jac_dot_is_the_time_derivative_of_jac(xml):
    T, L, pts, ids = _fd_case(xml)
    assert T["rot"].any()  # (ball or free rotations are among the dofs)
    (dp, _, _), (dr, _, _) = jr.dot_hp(T, {k: a[:1] for k, a in L.items()}, pts[:1], ids)
    worst = _fd_ratio(T, L, pts, ids, (dp, dr))
    print(f"{xml}: jac_dot against the Richardson-combined centred differences of jac (eps {FD_EPS}), worst error / allowed error {worst:.2e}")
    assert worst <= 1.0


def test_the_stored_cdof_dot_of_a_ball_joint_is_not_the_derivative():
    """The check has the power to tell: with cdof_dot as stored on every dof (formed with the velocity in front of the joint) ball_limits misses the bound."""
    T, L, pts, ids = _fd_case("ball_limits")
    plain = dict(T, rot=np.zeros_like(T["rot"]))
    (dp, _, _), (dr, _, _) = jr.dot_hp(plain, {k: a[:1] for k, a in L.items()}, pts[:1], ids)
    with pytest.raises(AssertionError):
        assert _fd_ratio(T, L, pts, ids, (dp, dr)) <= 1.0


# ---- 2. identities ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("xml", ["pendula", "ball_limits", "humanoid"])
def test_the_products_with_qvel_are_subtree_vel(xml):
    """jac_subtree_com . qvel = subtree_linvel and angmom_mat . qvel = subtree_angmom (tests/_postcon_ref.py, MuJoCo's mj_subtreeVel), for every body.  Both sides
    are evaluated in HP from the same float64 leaves; they differ through the leaves' own rounding (cvel against cdof . qvel, subtree_com against the bodies), which
    each side's magnitude sum bounds at the float64 unit: allowed = bound(n, u, S) of the one + bound(n, u, S) of the other."""
    mx = load_model(xml)
    T = jr.tables(mx)
    q, v, _ = moved_state(mx, 7, B=2)
    out = oracle_pass(mx, q, v)
    L = jr.leaves_of(out)
    ids = np.arange(T["nbody"])
    P = pr.tables(mx)
    want = pr.evaluate(P, dict(cvel=L["cvel"], xipos=L["xipos"], ximat=L["ximat"], subtree_com=L["subtree_com"]), rne=False, subtree=True)
    for name, fn in (("subtree_linvel", jr.subtree_com_hp), ("subtree_angmom", jr.angmom_hp)):
        got, S, n = jr.product(fn(T, L, ids), v)
        ref, Sr, nr = want[name]
        allowed = jr.bound(n, U64, S) + pr.bound(nr, U64, Sr)
        ratio = float((np.abs(got - ref) / np.where(allowed > 0, allowed, 1)).max())
        print(f"{xml}: {name}, worst |product - subtree_vel| / allowed {ratio:.2e}; largest entry {float(np.abs(ref).max()):.3g}")
        assert np.abs(ref).max() > 1e-2 and (np.abs(got - ref) <= allowed).all()


@pytest.mark.parametrize("xml", ["pendula", "humanoid"])
def test_the_subtree_of_a_leaf_body_is_the_body(xml):
    """jac_subtree_com of a body without children is jac at its xipos (its mass cancels: body_subtreemass = body_mass there)."""
    mx = load_model(xml)
    T = jr.tables(mx)
    q, v, _ = moved_state(mx, 9, B=2)
    L = jr.leaves_of(oracle_pass(mx, q, v))
    leaves = [b for b in range(1, T["nbody"]) if T["sub"][b].sum() == 1 and T["mass"][b] > 0]
    assert leaves
    got, S, n = jr.subtree_com_hp(T, L, leaves)
    (jp, ap), _ = sr.jac_hp(L["cdof"], L["subtree_com"], T["root"], T["mask"], L["xipos"][:, leaves], leaves)
    assert np.abs(jp).max() > 1e-2 and (np.abs(got - jp) <= jr.bound(n, U64, S)).all()


# ---- 3. closed forms -------------------------------------------------------------------------------------------------------------------------------

_PENDULUM = """<mujoco><compiler angle="radian"/><option timestep="0.002"/><worldbody>
  <body pos="0 0 2"><joint name="h" type="hinge" axis="0 1 0"/>
    <geom type="sphere" size="0.05" pos="0 0 -0.5" mass="2"/></body>
</worldbody></mujoco>"""


def test_a_hinge_pendulum_by_hand():
    """A bob (sphere, mass 2, radius 0.05) 0.5 below a y hinge at height 2: its centre is (-l sin q, 0, 2 - l cos q)."""
    mx = mt.device_put(mt.mjcf.from_xml_string(_PENDULUM))
    T = jr.tables(mx)
    q, w, m, l, r = 0.9, 1.7, 2.0, 0.5, 0.05
    out = oracle_pass(mx, np.array([[q]]), np.array([[w]]))
    L = jr.leaves_of(out)
    close = lambda got, want: np.allclose(np.asarray(got, dtype=np.float64), want, rtol=0, atol=1e-13)
    assert close(L["xipos"][0, 1], [-l * np.sin(q), 0, 2 - l * np.cos(q)])
    for body in (0, 1):
        assert close(jr.subtree_com_hp(T, L, [body])[0][0, 0], [[-l * np.cos(q), 0, l * np.sin(q)]])
        assert close(jr.angmom_hp(T, L, [body])[0][0, 0], [[0, 0.4 * m * r * r, 0]])
    (dp, _, _), (dr, _, _) = jr.dot_hp(T, L, L["xipos"][:, 1], [1])
    assert close(dp[0, 0], [[l * np.sin(q) * w, 0, l * np.cos(q) * w]]) and close(dr[0, 0], np.zeros((1, 3)))
    # on the world body nothing moves
    (dp, _, _), (dr, _, _) = jr.dot_hp(T, L, L["xipos"][:, 1], [0])
    assert not dp.any() and not dr.any()


def test_the_cartpole_by_hand():
    """cart 1 kg on a slide along x, pole 0.1 kg with its centre l = 0.3 from the hinge (about y): the whole model's centre moves with the cart, and by m / M of
    the pole's centre with the hinge; about that centre the hinge's angular momentum is the pole's own inertia plus the reduced mass times l^2, the slide's none."""
    mx = load_model("cartpole")
    T = jr.tables(mx)
    x, th, vx, w = 0.1, 0.7, 0.4, -1.3
    out = oracle_pass(mx, np.array([[x, th]]), np.array([[vx, w]]))
    L = jr.leaves_of(out)
    mc, mp, l = 1.0, 0.1, 0.3
    r = np.asarray(L["xipos"][0, 2] - L["xipos"][0, 1], dtype=np.float64)
    assert abs(np.linalg.norm(r) - l) < 1e-12 and abs(r[2] - l * np.cos(th)) < 1e-12 and abs(r[1]) < 1e-15
    u = np.cross([0.0, 1.0, 0.0], r)  # the pole centre's velocity at unit hinge rate
    close = lambda got, want: np.allclose(np.asarray(got, dtype=np.float64), want, rtol=0, atol=1e-13)
    assert close(jr.subtree_com_hp(T, L, [0])[0][0, 0], [[1, 0, 0], mp / (mc + mp) * u])
    assert close(jr.subtree_com_hp(T, L, [2])[0][0, 0], [[1, 0, 0], u])
    M0, _ = mt.mjcf.mass_matrix0(mx.tables.source, np.array([x, th]))
    Ip = M0[1, 1] - mp * l * l  # the pole's own inertia about y (+ the joint's armature, none here)
    assert float(np.asarray(jr._np(mx.dof_armature))[1]) == 0
    assert close(jr.angmom_hp(T, L, [0])[0][0, 0], [[0, 0, 0], [0, Ip + mp * mc / (mc + mp) * l * l, 0]])
    assert close(jr.angmom_hp(T, L, [2])[0][0, 0], [[0, 0, 0], [0, Ip, 0]])
    # the pole centre's acceleration at constant rates: Jdot qvel = -w^2 r
    (dp, Sp, n), _ = jr.dot_hp(T, L, L["xipos"][:, 2], [2])
    got, _, _ = jr.product((dp, Sp, n), np.array([[vx, w]]))
    assert close(got[0, 0], -w * w * r)
