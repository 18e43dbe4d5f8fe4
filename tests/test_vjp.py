"""transition_vjp, the tangent maps and differentiable_step on the device.

1. the contraction against the dense Jacobians of ``transition_fd`` (the same entries, bit for bit: only the order of the additions differs);
2. chunking and repetition change no bit;
3. the tangent kernels against tests/_vjp_ref.py;
4. the autograd wiring of ``differentiable_step``, through one step and through two chained ones;
5. its gradient against the reference's own autograd gradient through its float64 CPU step (tests/golden/vjp, tools/gen_vjp_golden.py);
6. refusals.
"""
import json
import os

import numpy as np
import pytest
import torch

import _vjp_ref as V
import mujoco_torch_amd as mt
from _cases import seeded_batch
from _util import GOLD, INT_LEAVES, REAL_LEAVES, leaf
from test_fd import joints, on_gpu

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
UNIT = {F64: 2.0 ** -53, F32: 2.0 ** -24}  # unit roundoff
EPS = {F64: 1e-6, F32: 1e-3}               # (float32: an eps its 2^-23 can resolve, as in test_fd)
NU_BFA = 8
# ball_free_actuators ships without control ranges: limit every second actuator to [-1, 1] so that the control rule has something to refuse
LIMITED = {"model.actuator_ctrllimited": [1, 0] * (NU_BFA // 2), "model.actuator_ctrlrange": [[-1.0, 1.0]] * NU_BFA}


def sizes(mx):
    nv, na, nu, nsd = int(mx.nv), int(mx.na), int(mx.nu), int(getattr(mx, "nsensordata", 0) or 0)
    return nv, na, nu, nsd, 2 * nv + na


def cotangents(mx, B, dtype, seed=5):
    nv, na, nu, nsd, ns = sizes(mx)
    rng = np.random.RandomState(seed)
    return torch.tensor(rng.randn(B, ns), dtype=dtype, device="cuda"), torch.tensor(rng.randn(B, nsd), dtype=dtype, device="cuda")


def edge_controls(mx, dg, eps):
    """Environment 0: inside the range (forward; centered: both sides, 3); 1: at the upper edge (backward only, 2); 2: at the lower edge (forward
    only, also when centered, 1); 3: inside but closer to the upper edge than eps (2); 4: outside the range (none, 0)."""
    assert int(mx.nu) == NU_BFA and dg.ctrl.shape[0] == 5
    ctrl = dg.ctrl.clone().clamp_(-0.5, 0.5)
    ctrl[1] = 1.0
    ctrl[2] = -1.0
    ctrl[3] = 1.0 - 0.5 * eps
    ctrl[4] = 1.5
    return dg.replace(ctrl=ctrl)


def case(xml, dtype):
    """(mx, mg, dg) of the smallest batch that reaches every branch for this model."""
    if xml == "ball_free_actuators":
        mx, mg, dg = on_gpu(xml, dtype, 5, LIMITED)
        assert np.asarray(mx.actuator_ctrllimited).reshape(-1).tolist() == LIMITED["model.actuator_ctrllimited"]
        return mx, mg, edge_controls(mx, dg, EPS[dtype])
    return on_gpu(xml, dtype, {"sensor_rig": 3, "cartpole": 1, "humanoid": 3, "muscle_arm": 2, "sensor_rig2": 3}[xml])


def check_contraction(what, mx, got, jac, g, gs, dtype):
    """|gx - A^T g - C^T g_s| <= 2 nrow u sum_row |g_row J[row, c]|: nrow - 1 additions and nrow products, each rounding relative to a partial
    sum of magnitude <= sum |g J| (u per operation, first order), once for the kernel and once more for slack on the float64 yardstick's own."""
    nv, na, nu, nsd, ns = sizes(mx)
    A, Bm, C, D = (j.detach().cpu().numpy().astype(np.float64) for j in jac)
    g = g.cpu().numpy().astype(np.float64)
    gs = None if gs is None else gs.cpu().numpy().astype(np.float64)
    nrow = ns + (nsd if gs is not None else 0)
    for name, out, Js, Jc in (("gx", got[0], A, C), ("gu", got[1], Bm, D)):
        ref = np.einsum("br,brc->bc", g, Js)
        mag = np.einsum("br,brc->bc", np.abs(g), np.abs(Js))
        if gs is not None:
            ref = ref + np.einsum("br,brc->bc", gs, Jc)
            mag = mag + np.einsum("br,brc->bc", np.abs(gs), np.abs(Jc))
        out = out.cpu().numpy().astype(np.float64)
        assert out.shape == ref.shape, (what, name, out.shape, ref.shape)
        assert np.isfinite(out).all(), (what, name)
        err, tol = np.abs(out - ref), 2 * nrow * UNIT[dtype] * mag
        print(f"{what} {name}{out.shape}: max |entry| {np.abs(ref).max() if ref.size else 0:.3e}, worst error {err.max() if err.size else 0:.3e}, "
              f"worst error / bound {(err[tol > 0] / tol[tol > 0]).max() if (tol > 0).any() else 0:.3e}, zero-bound entries {int((tol == 0).sum())}")
        assert (err <= tol).all(), (what, name, float(err.max()))
        if ref.size:
            assert np.abs(ref).max() > 0, (what, name)


@pytest.mark.parametrize("centered", [False, True], ids=["one-sided", "centered"])
@pytest.mark.parametrize("dtype", [F64, F32], ids=["float64", "float32"])
@pytest.mark.parametrize("xml", ["ball_free_actuators", "sensor_rig", "cartpole", "humanoid", "muscle_arm", "sensor_rig2"])
def test_contraction_equals_the_dense_jacobians(xml, dtype, centered):
    """Beside the four models the feature was specified with: muscle_arm, the one with activations (na > 0), and sensor_rig2, whose 22 state and
    141 sensor rows make a lane loop over three rows (the humanoid has 54 state rows and no sensors: one row per lane)."""
    mx, mg, dg = case(xml, dtype)
    nv, na, nu, nsd, ns = sizes(mx)
    B, eps = dg.qpos.shape[0], EPS[dtype]
    g, gs = cotangents(mx, B, dtype)
    jac = mt.transition_fd(mg, dg, eps=eps, centered=centered, sensors=True)
    what = f"{xml} {dtype} centered={centered}"
    got = mt.transition_vjp(mg, dg, g, gs, eps=eps, centered=centered)
    assert tuple(got[0].shape) == (B, ns) and tuple(got[1].shape) == (B, nu) and got[0].dtype == dtype and got[1].dtype == dtype
    check_contraction(what + " with g_sensor", mx, got, jac, g, gs, dtype)
    bare = mt.transition_vjp(mg, dg, g, eps=eps, centered=centered)
    check_contraction(what + " without g_sensor", mx, bare, jac, g, None, dtype)
    if xml == "sensor_rig":
        assert nsd > 0 and not torch.equal(bare[0], got[0])
    if xml == "ball_free_actuators":  # the control rule took every branch: columns of refused controls are exactly zero
        Bm = jac[1].cpu().numpy()
        lim = np.array(LIMITED["model.actuator_ctrllimited"], dtype=bool)
        assert (Bm[4][:, lim] == 0).all() and (got[1][4].cpu().numpy()[lim] == 0).all() and np.abs(got[1][4].cpu().numpy()[~lim]).max() > 0
        assert np.abs(Bm[:4]).max(axis=1).min() > 0  # ... and every control that could be nudged moves some entry of the next state
    if xml == "humanoid":
        assert (B * (ns + nu)) % 4 != 0  # the last workgroup is not full
    if xml == "sensor_rig2":
        assert ns + nsd > 128 and ns < 64  # with g_sensor the lanes loop over the rows, without it some lanes have none


def test_unbatched_and_nested_batches():
    mx, mg, dg = case("ball_free_actuators", F64)
    g, _ = cotangents(mx, 5, F64)
    gx, gu = mt.transition_vjp(mg, dg, g)
    a, b = mt.transition_vjp(mg, dg[1], g[1])
    assert a.shape == gx.shape[1:] and torch.equal(a, gx[1]) and torch.equal(b, gu[1])
    a2, b2 = mt.transition_vjp(mg, dg[torch.arange(5).reshape(5, 1)], g.reshape(5, 1, -1))
    assert a2.shape == (5, 1) + gx.shape[1:] and torch.equal(a2[:, 0], gx) and torch.equal(b2[:, 0], gu)


def test_chunking_and_repetition_change_no_bit():
    mx, mg, dg = case("humanoid", F64)
    nv, na, nu, nsd, ns = sizes(mx)
    ncol, B = ns + nu, dg.qpos.shape[0]
    g, gs = cotangents(mx, B, F64)
    pool = lambda: list(mg.tables.__dict__["_fd_scratch"].values())[-1]
    for centered in (False, True):
        nside = 2 if centered else 1
        run = lambda budget: mt.transition_vjp(mg, dg, g, gs, centered=centered, max_scratch_bytes=budget)
        whole = run(1 << 40)
        scr = pool()
        assert scr.slots == B * ncol * nside  # one chunk
        per_col = scr.slab.numel() / ncol
        ragged = []
        for k in (7.5, 10.5):
            cut = run(int(k * per_col))
            cols = pool().slots // (B * nside)
            assert 1 < cols < ncol, (cols, ncol)
            ragged.append(ncol % cols != 0)
            assert all(torch.equal(a, b) for a, b in zip(whole, cut)), (centered, cols)
        assert any(ragged), "no cut left a last chunk shorter than the others"
        single = run(1)  # one column per chunk
        assert pool().slots == B * nside
        again = run(1 << 40)
        for a, b, c in zip(whole, single, again):
            assert torch.equal(a, b) and torch.equal(a, c)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["float64", "float32"])
@pytest.mark.parametrize("xml", ["ball_free_actuators", "humanoid"])
def test_tangent_kernels_match_the_reference(xml, dtype):
    """Copied entries exactly; quaternion entries within twice the op-count bound of _vjp_ref (two correct evaluations of the same expression)."""
    B = 70  # more than one wavefront of (environment, dof) lanes in the smaller model too
    mx, mg, dg = on_gpu(xml, dtype, B)
    jt = joints(mx)
    assert len(jt.quats) >= 1
    rng = np.random.RandomState(11)
    qpos = dg.qpos.cpu().numpy().copy()
    qpos += (0.3 * rng.randn(*qpos.shape)).astype(qpos.dtype)
    for qa, _ in jt.quats:  # half the environments keep unit quaternions, the others get norms in [0.5, 2]
        q = qpos[:, qa:qa + 4]
        q /= np.linalg.norm(q, axis=-1, keepdims=True)
        q[1::2] *= rng.uniform(0.5, 2.0, (len(q[1::2]), 1)).astype(qpos.dtype)
        q[4] = 0  # ... and one is all zero: pull and push give exact zeros there
    gq, gt = rng.randn(B, jt.nq).astype(qpos.dtype), rng.randn(B, jt.nv).astype(qpos.dtype)
    dev = lambda x: torch.tensor(x, device="cuda")
    f64 = lambda x: x.astype(np.float64)
    mach = UNIT[dtype]
    for name, got, ref, tol in (
            ("pull", mt.tangent_pull(mg, dev(qpos), dev(gq)), V.pull(jt, f64(qpos), f64(gq)), 2 * V.pull_bound(mach, jt, qpos, gq)),
            ("push", mt.tangent_push(mg, dev(qpos), dev(gt)), V.push(jt, f64(qpos), f64(gt)), 2 * V.push_bound(mach, jt, qpos, gt))):
        got = got.cpu().numpy()
        assert got.dtype == qpos.dtype and got.shape == ref.shape
        err, exact = np.abs(got - ref), tol == 0
        print(f"{xml} {dtype} {name}: exact entries {int(exact.sum())}, bounded {int((~exact).sum())}, worst error / bound {(err[~exact] / tol[~exact]).max():.3e}")
        assert (err[exact] == 0).all() and (err[~exact] <= tol[~exact]).all(), (name, float(err.max()))
        assert exact.any() and (~exact).any() and np.abs(ref[~exact]).max() > 0.1
        qa, da = jt.quats[0]
        assert (got[4, qa:qa + 4] == 0).all() if name == "push" else (got[4, da:da + 3] == 0).all()


def with_grad(dg):
    leaves = {k: getattr(dg, k).clone().requires_grad_() for k in ("qpos", "qvel", "act", "ctrl")}
    return dg.replace(**leaves), leaves


def functional(mx, d1, B, dtype, seed=21):
    """A seeded linear functional of (qpos, qvel, act, sensordata) and its weights."""
    rng = np.random.RandomState(seed)
    w = {k: torch.tensor(rng.randn(B, getattr(d1, k).shape[-1]), dtype=dtype, device="cuda") for k in ("qpos", "qvel", "act", "sensordata")}
    return sum((w[k] * getattr(d1, k)).sum() for k in w), w


@pytest.mark.parametrize("xml", ["ball_free_actuators", "sensor_rig"])
def test_autograd_wiring(xml):
    mx, mg, dg = case(xml, F64)
    nv, na, nu, nsd, ns = sizes(mx)
    B = dg.qpos.shape[0]
    names = [n for n in REAL_LEAVES + INT_LEAVES if isinstance(leaf(dg, n), torch.Tensor)]
    before = {n: leaf(dg, n).clone() for n in names}
    d, leaves = with_grad(dg)
    d1 = mt.differentiable_step(mg, d)
    plain = mt.step(mg, dg, fixed_iterations=True)
    for n in names:  # every leaf is the step's, bit for bit
        assert torch.equal(leaf(d1, n).detach(), leaf(plain, n)), n
    tracked = ("qpos", "qvel", "act") + (("sensordata",) if nsd else ())
    for n in names:
        t = leaf(d1, n)
        if n in tracked:
            assert t.grad_fn is not None and t.requires_grad, n
        elif t.is_floating_point() and n not in ("ctrl",):
            assert not t.requires_grad, n
    L, w = functional(mx, d1, B, F64)
    first = torch.autograd.grad(L, [leaves[k] for k in ("qpos", "qvel", "act", "ctrl")], retain_graph=True)
    # ... composed by hand
    g_state = torch.cat([mt.tangent_pull(mg, plain.qpos, w["qpos"]), w["qvel"], w["act"]], dim=-1)
    gx, gu = mt.transition_vjp(mg, dg, g_state, w["sensordata"] if nsd else None, eps=1e-6, centered=True, fixed_iterations=True)
    hand = (mt.tangent_push(mg, dg.qpos, gx[:, :nv].contiguous()), gx[:, nv:2 * nv], gx[:, 2 * nv:], gu)
    for k, a, b in zip(("qpos", "qvel", "act", "ctrl"), first, hand):
        assert a.shape == leaves[k].shape and torch.equal(a, b), k
        assert a.numel() == 0 or float(a.abs().max()) > 0, k
    L.backward()  # a second backward through the retained graph repeats the bits, and gradients arrive at exactly the four leaves
    for k, a in zip(("qpos", "qvel", "act", "ctrl"), first):
        assert torch.equal(leaves[k].grad, a), k
    for n in names:
        t = leaf(d, n)
        if n not in ("qpos", "qvel", "act", "ctrl"):
            assert t.grad is None and not t.requires_grad, n
    for n in names:  # the inputs are unmodified
        assert torch.equal(leaf(dg, n), before[n]) and torch.equal(leaf(d, n).detach(), before[n]), n
    # without any input requiring grad the result carries no graph
    assert mt.differentiable_step(mg, dg).qpos.grad_fn is None


# test_gradient_matches_the_reference_autograd: measured on an MI355X (cartpole, B = 4, eps = 1e-6, centered): the largest |difference| to the
# reference's autograd gradient is 5.2e-12 (qpos 4.4e-12, qvel 2.0e-12, ctrl 5.2e-12; gradients of magnitude 0.3 .. 2).  The bound is 10 x that:
# finite-difference truncation plus cancellation, whose constants depend on the model.
MEASURED_GAP = 5.2e-12
GAP_BOUND = 10 * MEASURED_GAP


def test_gradient_matches_the_reference_autograd():
    z = np.load(os.path.join(GOLD, "vjp", "cartpole.npz"))
    meta = json.loads(str(z["meta"]))
    B = meta["nenv"]
    mx, dg = seeded_batch("cartpole", {}, F64, B)
    for k in ("qpos", "qvel", "act", "ctrl"):  # the recording was made on these very inputs
        assert np.array_equal(getattr(dg, k).numpy(), z[f"in/{k}"]), k
    mg, dg = mx.to("cuda"), dg.to("cuda")
    assert tuple(mx.constraint_sizes_py)[-1] == 0  # no constraint rows: a smooth step
    d, leaves = with_grad(dg)
    d1 = mt.differentiable_step(mg, d, eps=1e-6, centered=True)
    L = sum((torch.tensor(z[f"w/{k}"], device="cuda") * getattr(d1, k)).sum() for k in ("qpos", "qvel", "act"))
    got = torch.autograd.grad(L, [leaves[k] for k in ("qpos", "qvel", "act", "ctrl")])
    gap = 0.0
    for k, g in zip(("qpos", "qvel", "act", "ctrl"), got):
        ref = z[f"grad/{k}"]
        assert g.shape == ref.shape, k
        if ref.size:
            gap = max(gap, float(np.abs(g.cpu().numpy() - ref).max()))
            assert np.abs(ref).max() > 0.1, k
    print(f"cartpole: largest |differentiable_step gradient - reference autograd gradient| {gap:.3e}, bound {GAP_BOUND:.1e}")
    assert gap <= GAP_BOUND, (gap, GAP_BOUND)


@pytest.mark.parametrize("xml", ["sensor_rig", "ball_free_actuators"])
def test_two_chained_steps_backpropagate(xml):
    """d2 = differentiable_step(differentiable_step(d)): the gradient of a functional of d2 equals the two vector-Jacobian products composed by
    hand, bit for bit.  The first result's sensordata carries a graph and is accepted by the second call; the second step does not read it, so
    the first step's sensor cotangent is zero.  ctrl feeds both steps: its gradient is the sum of the two."""
    mx, mg, dg = case(xml, F64)
    nv, na, nu, nsd, ns = sizes(mx)
    B = dg.qpos.shape[0]
    d, leaves = with_grad(dg)
    d1 = mt.differentiable_step(mg, d)
    d2 = mt.differentiable_step(mg, d1)
    p1 = mt.step(mg, dg, fixed_iterations=True)
    p2 = mt.step(mg, p1, fixed_iterations=True)
    for n in ("qpos", "qvel", "act", "sensordata"):
        assert torch.equal(getattr(d2, n).detach(), getattr(p2, n)), n
    L, w = functional(mx, d2, B, F64)
    got = torch.autograd.grad(L, [leaves[k] for k in ("qpos", "qvel", "act", "ctrl")], retain_graph=True)
    kw = dict(eps=1e-6, centered=True, fixed_iterations=True)
    g2 = torch.cat([mt.tangent_pull(mg, p2.qpos, w["qpos"]), w["qvel"], w["act"]], dim=-1)
    gx2, gu2 = mt.transition_vjp(mg, p1, g2, w["sensordata"] if nsd else None, **kw)
    gq_mid = mt.tangent_push(mg, p1.qpos, gx2[:, :nv].contiguous())
    g1 = torch.cat([mt.tangent_pull(mg, p1.qpos, gq_mid), gx2[:, nv:2 * nv], gx2[:, 2 * nv:]], dim=-1)
    gx1, gu1 = mt.transition_vjp(mg, dg, g1, torch.zeros_like(w["sensordata"]) if nsd else None, **kw)
    hand = (mt.tangent_push(mg, dg.qpos, gx1[:, :nv].contiguous()), gx1[:, nv:2 * nv], gx1[:, 2 * nv:], gu1 + gu2)
    for k, a, b in zip(("qpos", "qvel", "act", "ctrl"), got, hand):
        assert a.shape == leaves[k].shape and torch.equal(a, b), (k, float((a - b).abs().max()) if a.numel() else 0)
        assert a.numel() == 0 or float(a.abs().max()) > 0, k
    if nu:
        assert float(gu1.abs().max()) > 0 and float(gu2.abs().max()) > 0
    # backward is native launches: differentiating it again is an error, not a gradient without a graph
    (gq,) = torch.autograd.grad(L, [leaves["qpos"]], create_graph=True)
    assert not gq.requires_grad
    with pytest.raises(RuntimeError, match="once_differentiable|does not require grad"):
        gq.sum().backward()


def test_torch_compile_breaks_the_graph_and_runs_the_call_eagerly():
    """Without fullgraph Dynamo breaks the graph at the call, which is kept out of its graphs, and runs it eagerly: the same bits as outside
    torch.compile.  (With fullgraph=True it is refused: tests/test_vjp_host.py.)"""
    mx, mg, dg = on_gpu("cartpole", F64, 4)
    g, _ = cotangents(mx, 4, F64)
    want = mt.transition_vjp(mg, dg, g)
    got = torch.compile(lambda q: mt.transition_vjp(mg, dg.replace(qpos=q), g))(dg.qpos)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_refusals_on_the_device():
    mx, mg, dg = on_gpu("cartpole", F64, 4)
    g, _ = cotangents(mx, 4, F64)
    with pytest.raises(NotImplementedError, match="transition_vjp cannot be used under torch.vmap"):
        torch.vmap(lambda q: mt.transition_vjp(mg, dg[0].replace(qpos=q), g[0])[0])(dg.qpos)
    with pytest.raises(NotImplementedError, match="differentiable_step cannot be used under torch.vmap"):
        torch.vmap(lambda q: mt.differentiable_step(mg, dg[0].replace(qpos=q)).qpos)(dg.qpos)
    with pytest.raises(ValueError, match="float32"):
        mt.transition_vjp(mg, dg.to(F32), g.to(F32))
    with pytest.raises(ValueError, match="float32"):
        mt.differentiable_step(mg, dg.to(F32))
    with pytest.raises(ValueError, match="g_state is on cpu"):
        mt.transition_vjp(mg, dg, g.cpu())
    with pytest.raises(ValueError, match="requires grad"):
        mt.differentiable_step(mg, dg.replace(qfrc_applied=dg.qfrc_applied.clone().requires_grad_()))
