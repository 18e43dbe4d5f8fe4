"""The support functions on the GPU: ``jac`` / ``apply_ft`` / ``xfrc_accumulate`` / ``mul_m`` / ``solve_m`` against the reference's own
(tests/golden/support/, tools/gen_support_golden.py; the recorded leaves are fed in), their shape forms, consistency between them, zero rows,
batch shapes, value edits, no mutation of the input, and the vmap / compile operator.  tests/test_support_edges.py goes past the goldens: launches cut on
the host, more vectors / rows than an LDS chunk, every body of the float32 and the large models, derived error bounds (tests/_support_ref.py)."""
import json
import os

import numpy as np
import pytest
import torch

import mujoco_torch_amd as mt
from _util import GOLD, load_model

pytestmark = pytest.mark.gpu

SUP_GOLD = os.path.join(GOLD, "support")
CASES = sorted(f[:-4] for f in os.listdir(SUP_GOLD) if f.endswith(".npz"))
DEV = "cuda"
LEAVES = ("cdof", "subtree_com", "xipos", "xfrc_applied", "qM", "qLD")


def _load(case):
    z = np.load(os.path.join(SUP_GOLD, case + ".npz"))
    meta = json.loads(str(z["meta"]))
    g = lambda k: np.stack([z[f"{e}/{k}"] for e in range(meta["nenv"])])
    keys = LEAVES + ("point", "force", "torque", "vec", "jacp", "jacr", "apply_ft", "xfrc_accumulate", "mul_m", "solve_m")
    return meta, {k: g(k) for k in keys}


def _golden_data(meta, a):
    dtype = getattr(torch, meta["dtype"])
    mx = load_model(meta["xml"], dtype=dtype).to(DEV)
    d = mt.make_data(mx).expand(meta["nenv"]).clone().to(DEV)
    return mx, d.replace(**{k: torch.tensor(a[k], device=DEV) for k in LEAVES})


def _close(got, want, tol, what):
    got, want = got.double().cpu().numpy(), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got - want).max(initial=0) / max(np.abs(want).max(initial=0), 1e-300)
    assert err <= tol, f"{what}: rel err {err:.3e}"


@pytest.mark.parametrize("case", CASES)
def test_matches_the_reference(case):
    meta, a = _load(case)
    mx, d = _golden_data(meta, a)
    tol = 1e-12 if meta["dtype"] == "float64" else 1e-5
    t = lambda k: torch.tensor(a[k], device=DEV)
    ids = meta["body_id"]
    # jac: the reference's per-element arithmetic, bit for bit, one point at a time and all P at once
    jp, jr = mt.jac(mx, d, t("point"), ids)
    assert torch.equal(jp.cpu(), torch.tensor(a["jacp"])) and torch.equal(jr.cpu(), torch.tensor(a["jacr"])), case
    for i, b in enumerate(ids):
        p1, r1 = mt.jac(mx, d, t("point")[:, i], torch.tensor(b))
        assert torch.equal(p1, jp[:, i]) and torch.equal(r1, jr[:, i])
    _close(mt.apply_ft(mx, d, t("force"), t("torque"), t("point"), ids), a["apply_ft"], tol, f"{case} apply_ft")
    _close(mt.xfrc_accumulate(mx, d), a["xfrc_accumulate"], tol, f"{case} xfrc_accumulate")
    _close(mt.mul_m(mx, d, t("vec")), a["mul_m"], tol, f"{case} mul_m")
    _close(mt.solve_m(mx, d, t("vec")), a["solve_m"], tol, f"{case} solve_m")


@pytest.fixture(scope="module")
def posed():
    """Humanoid float64, 8 environments after forward(), with random xfrc_applied."""
    mc = load_model("humanoid")
    mx = mc.to(DEV)
    B = 8
    rng = np.random.RandomState(11)
    d = mt.make_data(mc).expand(B).clone()
    d = d.replace(qpos=d.qpos + torch.tensor(0.1 * rng.randn(*d.qpos.shape)), qvel=torch.tensor(0.3 * rng.randn(B, mx.nv)))
    d = mt.forward(mx, d.to(DEV))
    return mx, d.replace(xfrc_applied=torch.tensor(rng.randn(B, mx.nbody, 6), device=DEV))


def _rand(*shape, seed=0):
    return torch.tensor(np.random.RandomState(seed).randn(*shape), device=DEV)


def test_point_shape_forms_agree_bit_for_bit(posed):
    mx, d = posed
    B, P = d.qpos.shape[0], 4
    ids = [0, 1, 7, 16]
    pts = _rand(B, P, 3, seed=1)
    jp, jr = mt.jac(mx, d, pts, ids)
    assert jp.shape == (B, P, mx.nv, 3) == jr.shape
    for i, b in enumerate(ids):
        pe, re = mt.jac(mx, d, pts[:, i], b)  # batch + (3,)
        assert torch.equal(pe, jp[:, i]) and torch.equal(re, jr[:, i])
        ps, rs = mt.jac(mx, d, pts[0, i], b)  # (3,): shared
        assert ps.shape == (B, mx.nv, 3)
        assert torch.equal(ps[0], jp[0, i]) and torch.equal(rs, jr[:, i])
    f, tq = _rand(B, P, 3, seed=2), _rand(3, seed=3)
    q = mt.apply_ft(mx, d, f, tq, pts, ids)
    assert q.shape == (B, P, mx.nv)
    for i, b in enumerate(ids):
        assert torch.equal(mt.apply_ft(mx, d, f[:, i], tq, pts[:, i], b), q[:, i])
        assert torch.equal(mt.apply_ft(mx, d, f[:, i], tq.expand(B, 3), pts[:, i], torch.tensor(b)), q[:, i])


@pytest.mark.parametrize("fn", ["mul_m", "solve_m"])
def test_k_vectors_agree_with_k_calls(posed, fn):
    mx, d = posed
    B, K = d.qpos.shape[0], 5
    v = _rand(B, K, mx.nv, seed=4)
    f = getattr(mt, fn)
    out = f(mx, d, v)
    assert out.shape == (B, K, mx.nv)
    for j in range(K):
        assert torch.equal(f(mx, d, v[:, j]), out[:, j])
    assert torch.equal(f(mx, d, v[0, 0]), f(mx, d, v[0, 0].expand(B, mx.nv)))


def test_consistency(posed):
    mx, d = posed
    B, P = d.qpos.shape[0], 6
    ids = [0, 1, 3, 9, 12, 16]
    pts, f, tq = _rand(B, P, 3, seed=5), _rand(B, P, 3, seed=6), _rand(B, P, 3, seed=7)
    jp, jr = mt.jac(mx, d, pts, ids)
    want = torch.einsum("bpvk,bpk->bpv", jp, f) + torch.einsum("bpvk,bpk->bpv", jr, tq)
    _close(mt.apply_ft(mx, d, f, tq, pts, ids), want.cpu().numpy(), 1e-13, "apply_ft vs einsum of jac")
    x = d.xfrc_applied
    per = mt.apply_ft(mx, d, x[:, :, :3], x[:, :, 3:], d.xipos, list(range(mx.nbody)))
    _close(mt.xfrc_accumulate(mx, d), per.sum(1).cpu().numpy(), 1e-12, "xfrc_accumulate vs summed apply_ft")
    v = _rand(B, 2, mx.nv, seed=8)
    _close(mt.mul_m(mx, d, v), torch.einsum("bij,bkj->bki", d.qM, v).cpu().numpy(), 1e-13, "mul_m vs einsum")
    _close(mt.solve_m(mx, d, v), torch.cholesky_solve(v.transpose(1, 2), torch.tril(d.qLD)).transpose(1, 2).cpu().numpy(), 1e-11, "solve_m vs cholesky_solve")


def test_world_and_mocap_bodies_have_zero_jacobians():
    mc = load_model("mocap_child")
    mx = mc.to(DEV)
    d = mt.forward(mx, mt.make_data(mc).expand(3).clone().to(DEV))
    dofnum, parent = np.asarray(mc.body_dofnum), np.asarray(mc.body_parentid)
    nodof = [b for b in range(mx.nbody) if b == 0 or (dofnum[b] == 0 and parent[b] == 0)]
    assert len(nodof) >= 2
    jp, jr = mt.jac(mx, d, _rand(3, len(nodof), 3, seed=9), nodof)
    assert not jp.any() and not jr.any()
    jp, jr = mt.jac(mx, d, _rand(3, 3, seed=9), mx.nbody - 1)
    assert jp.any() and jr.any()


@pytest.mark.parametrize("batch", [(2, 3), (1,), (300,)])
def test_batch_shapes(posed, batch):
    """Two batch dimensions, B = 1 and a B that is no multiple of a workgroup's environments: each environment's result equals a B = 1 call."""
    mx, d8 = posed
    n = int(np.prod(batch))
    idx = torch.arange(n, device=DEV) % d8.qpos.shape[0]
    d = mt.make_data(mx).expand(*batch).clone().to(DEV)
    d = d.replace(**{k: getattr(d8, k)[idx].reshape(batch + getattr(d8, k).shape[1:]) for k in LEAVES})
    pts, v = _rand(*batch, 2, 3, seed=10), _rand(*batch, mx.nv, seed=11)
    outs = {"jac": mt.jac(mx, d, pts, [4, 16])[0], "mul_m": mt.mul_m(mx, d, v), "solve_m": mt.solve_m(mx, d, v), "xfrc": mt.xfrc_accumulate(mx, d),
            "apply_ft": mt.apply_ft(mx, d, _rand(3), _rand(3), pts[..., 0, :], 5)}
    assert outs["jac"].shape == batch + (2, mx.nv, 3)
    assert outs["mul_m"].shape == outs["solve_m"].shape == outs["xfrc"].shape == outs["apply_ft"].shape == batch + (mx.nv,)
    flat = {k: o.reshape((n,) + o.shape[len(batch):]) for k, o in outs.items()}
    P, V = pts.reshape(n, 2, 3), v.reshape(n, mx.nv)
    for e in sorted({0, n // 2, n - 1}):
        one = mt.make_data(mx).expand(1).clone().to(DEV)
        one = one.replace(**{k: getattr(d8, k)[idx[e] : idx[e] + 1] for k in LEAVES})
        assert torch.equal(flat["jac"][e], mt.jac(mx, one, P[e : e + 1], [4, 16])[0][0])
        assert torch.equal(flat["mul_m"][e], mt.mul_m(mx, one, V[e : e + 1])[0])
        assert torch.equal(flat["solve_m"][e], mt.solve_m(mx, one, V[e : e + 1])[0])
        assert torch.equal(flat["xfrc"][e], mt.xfrc_accumulate(mx, one)[0])


def test_value_edits_take_effect_and_the_input_is_not_mutated(posed):
    mx, d = posed
    before = {k: getattr(d, k).clone() for k in LEAVES}
    pts, v = _rand(3, seed=12), _rand(mx.nv, seed=13)
    outs = (mt.jac(mx, d, pts, 7)[0], mt.xfrc_accumulate(mx, d), mt.mul_m(mx, d, v), mt.solve_m(mx, d, v))
    for k in LEAVES:
        assert torch.equal(getattr(d, k), before[k]), k
    d2 = d.replace(cdof=d.cdof * 2, xfrc_applied=d.xfrc_applied * 3, qM=d.qM * 2, qLD=d.qLD * 2)
    outs2 = (mt.jac(mx, d2, pts, 7)[0], mt.xfrc_accumulate(mx, d2), mt.mul_m(mx, d2, v), mt.solve_m(mx, d2, v))
    assert torch.equal(outs2[0], outs[0] * 2)
    _close(outs2[1], (outs[1] * 6).cpu().numpy(), 1e-14, "xfrc edited")
    assert torch.equal(outs2[2], outs[2] * 2)
    _close(outs2[3], (outs[3] / 4).cpu().numpy(), 1e-14, "solve_m edited")


def test_vmap_and_compile_are_bit_identical(posed):
    mx, d = posed
    B = d.qpos.shape[0]
    pts, f, v = _rand(B, 3, seed=14), _rand(B, 3, seed=15), _rand(B, 2, mx.nv, seed=16)
    direct = (mt.jac(mx, d, pts, 9), mt.apply_ft(mx, d, f, f, pts, [9]), mt.xfrc_accumulate(mx, d), mt.mul_m(mx, d, v), mt.solve_m(mx, d, v))

    def fn(d, pts, f, v):
        return (mt.jac(mx, d, pts, 9), mt.apply_ft(mx, d, f, f, pts, [9]), mt.xfrc_accumulate(mx, d), mt.mul_m(mx, d, v), mt.solve_m(mx, d, v))

    mapped = torch.vmap(fn)(d, pts, f, v)
    compiled = torch.compile(fn, fullgraph=True)(d, pts, f, v)
    for got in (mapped, compiled):
        assert torch.equal(got[0][0], direct[0][0]) and torch.equal(got[0][1], direct[0][1])
        for a, b in zip(got[1:], direct[1:]):
            assert torch.equal(a, b)
    # one operator call per function
    from torch._dynamo.testing import CompileCounterWithBackend

    cnt = CompileCounterWithBackend("eager")
    torch.compile(fn, fullgraph=True, backend=cnt)(d, pts, f, v)
    calls = [n for g in cnt.graphs for n in g.graph.nodes if n.op == "call_function" and "support_leaves" in str(n.target)]
    assert len(cnt.graphs) == 1 and len(calls) == 5
