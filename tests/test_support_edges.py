"""The support kernels past their goldens (tests/test_support.py checks them on 6 bodies, 3 vectors and at most 3 environments per case):

* launches cut on the host (``MJH_MAX_GRID_LOG2``), boundaries inside an environment and inside a query, against the uncut run;
* ``solve_m`` with more vectors than its LDS chunk holds and ``mul_m`` with three row chunks, in both dtypes;
* every body of small, float32 and large (two and three mask words) models on this library's own ``forward`` output: ``jac`` bit for bit against
  tests/_support_ref.py (whose ancestor mask is walked from ``body_parentid``, so every row of the library's ``body_dofmask`` is checked), the four
  sums against its high-precision evaluation, and J^T qvel against the ``cvel`` leaf, which involves no mask table at all;
* query forms without a test so far: P = 1 and K = 1 with their dimension kept, a shared point with listed ids, non-contiguous and
  float64 queries, a side stream, an empty batch.

No tolerance here is read off the kernels.  Where the kernel's arithmetic order is that of another same-dtype evaluation the results must be
``torch.equal``.  A sum of n products is held to ``(n + 2) eps S_abs`` per element (``_support_ref.bound``; S_abs: the sum of the absolute
elementary terms in high precision), n counting the terms plus the roundings their inputs have taken; ``solve_m`` to the componentwise
residual bound of two substitutions (``_support_ref.solve_m_factor``).  The model tables the reference needs are read from the host model.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import _support_ref as ref
import mujoco_torch_amd as mt
from _util import load_model
from test_big_models import ENVELOPE

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64, F32 = torch.float64, torch.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _overrides(xml, dtype):
    """The option overrides test_big_models.ENVELOPE lists for the model (the configuration whose largest model it is); none for the others."""
    for (dt, _, _), (big, _, ov) in ENVELOPE.items():
        if big == xml and dt == dtype:
            return ov
    return {}


def _forwarded(xml, dtype, B, seed):
    """(host model, device model, Data after forward on the device): a seeded perturbed pose, non-zero qvel, random xfrc_applied on every body."""
    mc = load_model(xml, _overrides(xml, dtype), dtype)
    mx = mc.to(DEV)
    rng = np.random.RandomState(seed)
    d = mt.make_data(mc).expand(B).clone()
    d = d.replace(qpos=d.qpos + torch.tensor(0.1 * rng.randn(*d.qpos.shape)), qvel=torch.tensor(0.3 * rng.randn(B, int(mc.nv))))
    if dtype != F64:
        d = d.to(dtype)
    d = mt.forward(mx, d.to(DEV))
    return mc, mx, d.replace(xfrc_applied=torch.tensor(rng.randn(B, int(mc.nbody), 6), dtype=dtype, device=DEV))


def _rand(rng, *shape, dtype=F64):
    return torch.tensor(rng.randn(*shape), dtype=dtype, device=DEV)


def _host(t):
    return t.detach().cpu().numpy()


def _within(got, want, allowed, what):
    """|got - want| <= allowed per element (the difference in the reference's high precision); prints the worst ratio before it asserts."""
    err = np.abs(np.asarray(got, dtype=ref.HP) - np.asarray(want, dtype=ref.HP)).astype(np.float64)
    allowed = np.asarray(allowed, dtype=np.float64)
    assert err.shape == allowed.shape, (what, err.shape, allowed.shape)
    assert np.isfinite(err).all(), what
    ratio = float((err / np.maximum(allowed, 1e-300)).max(initial=0.0))
    print(f"{what}: worst error / bound {ratio:.3f} over {err.size} elements")
    over = err > allowed
    i = np.unravel_index(np.argmax(err - allowed), err.shape) if err.size else ()
    assert not over.any(), f"{what}: {int(over.sum())} of {err.size} elements beyond their bound; worst at {i}: error {err[i]:.3e}, bound {allowed[i]:.3e}"


# ---- a. launch cuts ---------------------------------------------------------------------------------------------------------------

CUT_MODELS = (("humanoid", "float64"), ("ant", "float32"), ("centipede_83", "float64"))
CUT_B, CUT_P, CUT_K, CUT_LOG2 = 203, 5, 3, 2

_CUT_CHILD = r'''
import sys
sys.path.insert(0, "tests"); sys.path.insert(0, "mujoco-torch_amd"); sys.path.insert(0, "oracle")
import numpy as np, torch, mujoco_torch_amd as mt
from _util import load_model
B, P, K = int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
res = {}
for spec in sys.argv[5:]:
    xml, dts = spec.split(":")
    dt = getattr(torch, dts)
    mc = load_model(xml, dtype=dt)
    mx = mc.to("cuda")
    nv, nb = int(mc.nv), int(mc.nbody)
    rng = np.random.RandomState(3)
    d = mt.make_data(mc).expand(B).clone()
    d = d.replace(qpos=d.qpos + torch.tensor(0.05 * rng.randn(*d.qpos.shape)), qvel=torch.tensor(0.2 * rng.randn(B, nv)))
    if dt != torch.float64: d = d.to(dt)
    d = mt.forward(mx, d.to("cuda"))
    d = d.replace(xfrc_applied=torch.tensor(rng.randn(B, nb, 6), dtype=dt, device="cuda"))
    t = lambda *s: torch.tensor(rng.randn(*s), dtype=dt, device="cuda")
    ids = [0, 1, nb // 2, nb - 2, nb - 1]
    assert len(ids) == P
    pts, f, tq, v, p1 = t(B, P, 3), t(B, P, 3), t(B, P, 3), t(B, K, nv), t(3)
    out = {k: getattr(d, k) for k in ("cdof", "subtree_com", "xipos", "qM", "qLD")}  # the leaves: a difference there is forward's, not support's
    out["jacp"], out["jacr"] = mt.jac(mx, d, pts, ids)
    out["apply_ft"] = mt.apply_ft(mx, d, f, tq, pts, ids)
    out["xfrc_accumulate"] = mt.xfrc_accumulate(mx, d)
    out["mul_m"] = mt.mul_m(mx, d, v)
    out["solve_m"] = mt.solve_m(mx, d, v)
    out["jacp_one_body"], out["jacr_one_body"] = mt.jac(mx, d, p1, nb - 1)  # body_stride 0, a shared (3,) point
    out["apply_ft_one_body"] = mt.apply_ft(mx, d, f[0, 0], tq[:, 0], p1, nb - 1)
    res[spec] = {k: o.cpu() for k, o in out.items()}
torch.save(res, sys.argv[1])
print("ran")
'''


def test_batches_past_one_launch_are_cut_on_the_host():
    """MJH_MAX_GRID_LOG2=2 caps a launch at 4 workgroups: 1024 elements of the point and xfrc kernels, 4 environments of mul_m / solve_m.  All five
    functions on 203 environments of three models then run in several launches whose (env_base, r_base, count) the launcher rebuilds, boundaries
    falling inside an environment and inside a query, and must be bit-identical to the single launch of the default.

    Which boundaries are aligned is asserted as a set: the ant's 8 dofs divide 1024, so its nv-sized units (an environment of xfrc_accumulate and of
    the one-body apply_ft, a query of apply_ft) start launches on their own boundaries; every other call of every model, and all of the
    humanoid's (27 dofs) and the centipede's (83), get a launch that starts inside an environment and inside a query."""
    launch = 256 << CUT_LOG2  # MJH_SUP_WG lanes per workgroup
    aligned = set()
    for xml, dts in CUT_MODELS:
        nv = int(load_model(xml, dtype=getattr(torch, dts)).nv)
        # function: (elements per environment, elements per query)
        sizes = {"jac": (CUT_P * nv * 3, nv * 3), "apply_ft": (CUT_P * nv, nv), "jac one body": (nv * 3, nv * 3), "apply_ft one body": (nv, nv),
                 "xfrc_accumulate": (nv, nv)}
        for what, (per_env, per_q) in sizes.items():
            assert CUT_B * per_env > launch, (xml, what)  # at least two launches
            if launch % per_env == 0:
                aligned.add((xml, what))  # every launch starts on an environment boundary: r_base stays 0
            elif launch % per_q == 0:
                aligned.add((xml, what + " (query)"))  # inside an environment, on a query boundary
        assert launch % sizes["jac"][0] != 0 and launch % sizes["apply_ft"][0] != 0, xml  # the P = 5 calls: inside an environment, every model
    # the ant's 8 dofs divide 1024: its nv-sized elements are the aligned cases; everything else starts inside an environment AND inside a query
    assert aligned == {("ant", "apply_ft one body"), ("ant", "xfrc_accumulate"), ("ant", "apply_ft (query)")}, aligned
    assert CUT_B > (1 << CUT_LOG2) and CUT_B % (1 << CUT_LOG2) != 0  # mul_m / solve_m: several launches, the last one short
    with tempfile.TemporaryDirectory() as td:
        res = {}
        for tag, env in (("one", {}), ("cut", {"MJH_MAX_GRID_LOG2": str(CUT_LOG2)})):
            f = os.path.join(td, tag + ".pt")
            base = {k: v for k, v in os.environ.items() if k != "MJH_MAX_GRID_LOG2"}
            r = subprocess.run([sys.executable, "-c", _CUT_CHILD, f, str(CUT_B), str(CUT_P), str(CUT_K)] + [f"{x}:{t}" for x, t in CUT_MODELS],
                               cwd=ROOT, env=dict(base, **env), capture_output=True, text=True, timeout=900)
            assert r.returncode == 0 and "ran" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
            res[tag] = torch.load(f)
    assert len(res["one"]) == len(CUT_MODELS)
    for case, outs in res["one"].items():
        assert len(outs) == 14
        for k, a in outs.items():
            assert a.shape[0] == CUT_B and torch.isfinite(a).all() and a.any(), (case, k)
            assert torch.equal(a, res["cut"][case][k]), (case, k)


# ---- b. LDS chunk edges -----------------------------------------------------------------------------------------------------------

SOLVE_CHUNK_BYTES, MULM_CHUNK_BYTES = 16384, 32768  # run_support (csrc/mjhip.hip): kVecBytes, kChunkBytes


def _itemsize(dtype):
    return torch.finfo(dtype).bits // 8


def _check_solve_m(mc, d, v, out, what):
    """solve_m's result on vectors v [B, K, nv] by its residual and by the forward error the residual bound implies (against the high-precision solve)."""
    nv, eps = int(mc.nv), torch.finfo(out.dtype).eps
    qLD, vh, xh = _host(d.qLD), _host(v), _host(out)
    res, scale = ref.solve_m_residual(qLD, vh, xh)
    _within(res, np.zeros_like(res), ref.solve_m_factor(nv, eps) * scale, f"{what} solve_m residual")
    _within(xh, ref.solve_m_hp(qLD, vh)[0], ref.solve_m_forward_bound(qLD, xh, eps), f"{what} solve_m")


def _check_mul_m(mc, d, v, out, what):
    val, s = ref.mul_m_hp(_host(d.qM), _host(v))
    _within(_host(out), val, ref.bound(int(mc.nv), torch.finfo(out.dtype).eps, s), f"{what} mul_m")


@pytest.mark.parametrize("xml,dtype,chunk", [("humanoid", F64, 75), ("centipede_83", F64, 24), ("centipede_154", F32, 26)], ids=lambda v: str(v).replace("torch.", ""))
def test_solve_m_with_more_vectors_than_an_lds_chunk(xml, dtype, chunk):
    """The kernel keeps ``chunk`` = 16 KiB / (nv reals) vectors in LDS at a time: K = chunk - 1, chunk, chunk + 1 (a last chunk of one vector) and
    2 chunk + 3 (three chunks, the last partial).  Row j of the K-vector call is bit-identical to the call on vector j alone, for every j, and the
    largest call is held to the residual bound.  (Past 64 KiB of LDS the launcher raises the kernel's LDS limit; no model the library accepts reaches
    that -- the largest, 106 dofs in float64 and 154 in float32, need 61 and 62 KiB -- so that branch is out of reach of a test.)"""
    B = 3
    mc, mx, d = _forwarded(xml, dtype, B, seed=21)
    nv = int(mc.nv)
    assert chunk == SOLVE_CHUNK_BYTES // (nv * _itemsize(dtype)) and chunk > 1
    assert (nv * (nv + 1) // 2 + chunk * nv) * _itemsize(dtype) <= 64 * 1024
    Ks = (chunk - 1, chunk, chunk + 1, 2 * chunk + 3)
    assert Ks[1] <= chunk < Ks[2] and Ks[3] > 2 * chunk and Ks[3] % chunk != 0  # the j0 loop runs once, once, twice, three times
    v = _rand(np.random.RandomState(22), B, Ks[-1], nv, dtype=dtype)
    single = torch.stack([mt.solve_m(mx, d, v[:, j]) for j in range(Ks[-1])], dim=1)
    assert single.shape == (B, Ks[-1], nv)
    for K in Ks:
        out = mt.solve_m(mx, d, v[:, :K])
        assert out.shape == (B, K, nv)
        bad = [j for j in range(K) if not torch.equal(out[:, j], single[:, j])]
        assert not bad, f"{xml} K = {K} (chunk {chunk}): vectors {bad[:8]} differ from their single-vector call"
    _check_solve_m(mc, d, v, out, f"{xml} K = {Ks[-1]}")


@pytest.mark.parametrize("xml,dtype,chunk", [("centipede_154", F32, 53), ("centipede_106", F64, 38)], ids=lambda v: str(v).replace("torch.", ""))
def test_mul_m_with_three_row_chunks(xml, dtype, chunk):
    """qM streams through LDS in chunks of 32 KiB / (nv reals) rows: three chunks with a short last one in both models.  K = 1, 2, 7 and 70 vectors share
    each chunk (K rows-of-the-chunk lanes' worth of work: 70 x 53 is 58 passes of the wavefront); every vector's result is bit-identical to its
    single-vector call and within the summation bound of the high-precision product."""
    B = 3
    mc, mx, d = _forwarded(xml, dtype, B, seed=23)
    nv = int(mc.nv)
    assert chunk == MULM_CHUNK_BYTES // (nv * _itemsize(dtype))
    assert nv > 2 * chunk and nv < 3 * chunk and nv % chunk != 0  # three row chunks, the last one short
    Ks = (1, 2, 7, 70)
    assert Ks[-1] * chunk > 10 * 64
    v = _rand(np.random.RandomState(24), B, Ks[-1], nv, dtype=dtype)
    single = torch.stack([mt.mul_m(mx, d, v[:, j]) for j in range(Ks[-1])], dim=1)
    for K in Ks:
        out = mt.mul_m(mx, d, v[:, :K])
        assert out.shape == (B, K, nv)
        bad = [j for j in range(K) if not torch.equal(out[:, j], single[:, j])]
        assert not bad, f"{xml} K = {K}: vectors {bad[:8]} differ from their single-vector call"
        _check_mul_m(mc, d, v[:, :K], out, f"{xml} K = {K}")


# ---- c. every body, small / float32 / large models, on forward's own output ---------------------------------------------------------

# (xml, dtype, nv, nbody, 64-bit mask words)
ALL_BODY_CASES = [("humanoid", F64, 27, 17, 1), ("humanoid", F32, 27, 17, 1), ("ant", F64, 8, 14, 1), ("ant", F32, 8, 14, 1), ("cartpole", F64, 2, 3, 1),
                  ("mocap_child", F64, 11, 6, 1), ("ball_limits", F64, 11, 6, 1), ("walker2d", F64, 9, 8, 1), ("walker2d", F32, 9, 8, 1),
                  ("centipede_83", F64, 83, 85, 2), ("centipede_121", F32, 121, 123, 2), ("centipede_129", F32, 129, 131, 3), ("centipede_154", F32, 154, 156, 3)]


@pytest.fixture(scope="module", params=ALL_BODY_CASES, ids=[f"{c[0]}-{str(c[1])[6:]}" for c in ALL_BODY_CASES])
def all_bodies(request):
    """5 seeded environments after forward, every body queried at once at xipos + a seeded offset; the host tables and the walked mask."""
    xml, dtype, nv, nb, words = request.param
    B = 5
    mc, mx, d = _forwarded(xml, dtype, B, seed=31)
    assert (int(mc.nv), int(mc.nbody), (int(mc.nv) + 63) // 64) == (nv, nb, words)
    rng = np.random.RandomState(32)
    ids = list(range(nb))
    assert sorted(set(ids)) == list(range(int(mx.nbody)))  # every body is queried
    pts = d.xipos + _rand(rng, B, nb, 3, dtype=dtype) * 0.1
    mask = ref.ancestor_mask(mc.body_parentid, mc.dof_bodyid)
    assert mask.shape == (nb, nv) and not mask[0].any()
    assert ((mask.any(1)) & (~mask.all(1))).any(), f"{xml}: no body has a partial mask"
    geo = (_host(d.cdof), _host(d.subtree_com), np.asarray(mc.body_rootid), mask)
    assert np.abs(_host(d.qvel)).min() > 0 and np.abs(geo[0]).max() > 0
    return dict(xml=f"{xml} {str(dtype)[6:]}", mc=mc, mx=mx, d=d, ids=ids, pts=pts, geo=geo, mask=mask, eps=torch.finfo(dtype).eps, rng=rng, dtype=dtype)


def test_jac_of_every_body_is_bit_identical_to_the_walked_mask_reference(all_bodies):
    """jacp / jacr of all nbody bodies in one call against _support_ref.jac_same on the device's own leaves: the same per-element arithmetic in the
    same dtype, with the ancestor mask walked from body_parentid on the host.  A wrong bit anywhere in the library's body_dofmask, in any of its
    mask words, zeroes or frees an entry, so this checks the whole table."""
    c = all_bodies
    jp, jr = mt.jac(c["mx"], c["d"], c["pts"], c["ids"])
    wp, wr = ref.jac_same(*c["geo"], _host(c["pts"]), c["ids"])
    assert jp.shape == wp.shape == (5, len(c["ids"])) + c["mask"].shape[1:] + (3,)
    for got, want, name in ((jp, wp, "jacp"), (jr, wr, "jacr")):
        got = _host(got)
        assert got.dtype == want.dtype
        bad = np.argwhere(got != want)
        assert bad.size == 0, f"{c['xml']} {name}: {len(bad)} entries differ, first (env, body, dof, k) = {bad[0].tolist()}: {got[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}"
    # the zero pattern is the mask's: an entry of jacr is non-zero exactly where the dof is an ancestor's and its cdof entry is not zero
    assert np.array_equal(_host(jr) != 0, (c["geo"][0][:, None, :, :3] != 0) & c["mask"][None, :, :, None])


def test_the_sums_of_every_body_are_within_their_bounds_of_high_precision(all_bodies):
    """apply_ft on every body, xfrc_accumulate, mul_m and solve_m on forward's own leaves against the high-precision evaluation.  n per element:
    apply_ft 6 products of entries carrying JACP_ROUNDINGS = 4 roundings, n = 10; xfrc_accumulate the same over all bodies, n = 6 nbody + 4
    (the world body's terms are all masked: its row of S_abs is zero, and skipping it changes nothing -- which is why the reference may skip
    it); mul_m nv products of exact inputs, n = nv.  S_abs is formed from the unrounded high-precision elementary terms."""
    c = all_bodies
    mc, mx, d, eps, rng, dtype = c["mc"], c["mx"], c["d"], c["eps"], c["rng"], c["dtype"]
    B, nb, nv = 5, int(mc.nbody), int(mc.nv)
    f, tq = _rand(rng, B, nb, 3, dtype=dtype), _rand(rng, B, nb, 3, dtype=dtype)
    got = mt.apply_ft(mx, d, f, tq, c["pts"], c["ids"])
    val, s = ref.apply_ft_hp(*c["geo"], _host(c["pts"]), _host(f), _host(tq), c["ids"])
    assert got.shape == (B, nb, nv) and (s[:, 1:].max() > 0)
    _within(_host(got), val, ref.bound(6 + ref.JACP_ROUNDINGS, eps, s), f"{c['xml']} apply_ft")
    assert np.array_equal(_host(got) != 0, np.broadcast_to(c["mask"], got.shape) & (_host(got) != 0))  # nothing outside the mask
    val, s = ref.xfrc_hp(c["geo"][0], c["geo"][1], _host(d.xipos), _host(d.xfrc_applied), c["geo"][2], c["mask"])
    _within(_host(mt.xfrc_accumulate(mx, d)), val, ref.bound(6 * nb + ref.JACP_ROUNDINGS, eps, s), f"{c['xml']} xfrc_accumulate")
    v = _rand(rng, B, 4, nv, dtype=dtype)
    _check_mul_m(mc, d, v, mt.mul_m(mx, d, v), c["xml"])
    _check_solve_m(mc, d, v, mt.solve_m(mx, d, v), c["xml"])


def test_jacobians_times_qvel_give_the_cvel_leaf(all_bodies):
    """Physics that uses no mask table: for every body, jacp^T qvel and jacr^T qvel are the velocity of the point, which the ``cvel`` leaf of the same
    forward pass gives as omega = cvel[b, :3], v = cvel[b, 3:] + omega x (point - subtree_com[root[b]]).  Both sides are sums of the same
    cdof * qvel products over the body's ancestor dofs (na of them); the device's jac and cvel are taken to the host and both sides are
    formed there in high precision, so the error is that of their roundings.  Angular: cvel's sum of na products, n = na.  Linear: the issue's
    count of 2 na terms (a dof's cross term is two products; cvel's own sum of na products and its use in the cross product stay below it), plus
    the JACP_ROUNDINGS = 4 of a jacp entry, n = 2 na + 4.  S_abs is formed from the unrounded high-precision terms |cdof| |offset| |qvel|."""
    c = all_bodies
    d, eps = c["d"], c["eps"]
    jp, jr = mt.jac(c["mx"], d, c["pts"], c["ids"])
    q = np.asarray(_host(d.qvel), dtype=ref.HP)[:, None, :, None]
    v_jac, w_jac = (np.asarray(_host(jp), dtype=ref.HP) * q).sum(2), (np.asarray(_host(jr), dtype=ref.HP) * q).sum(2)
    (_, sv), (_, sw) = ref.point_velocity_hp(*c["geo"], _host(c["pts"]), c["ids"], _host(d.qvel))
    cvel = np.asarray(_host(d.cvel), dtype=ref.HP)
    off = np.asarray(_host(c["pts"]), dtype=ref.HP) - np.asarray(c["geo"][1], dtype=ref.HP)[:, c["geo"][2]]
    w, v = cvel[..., :3], cvel[..., 3:] + np.cross(cvel[..., :3], off)
    na = c["mask"].sum(1)[None, :, None]
    assert na.max() >= 2 and (sw[:, 1:].max() > 0) and np.abs(w).max() > 0
    _within(w_jac, w, ref.bound(na, eps, sw), f"{c['xml']} jacr^T qvel vs cvel")
    _within(v_jac, v, ref.bound(2 * na + ref.JACP_ROUNDINGS, eps, sv), f"{c['xml']} jacp^T qvel vs cvel")


# ---- d. query forms without a test so far ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ant32():
    return _forwarded("ant", F32, 6, seed=41)


def test_one_query_and_one_vector_keep_their_dimension(ant32):
    """P = 1 given as a one-element id list and K = 1 given as S + (1, nv): the result keeps the dimension (the query stride takes the n == 1 branch)."""
    mc, mx, d = ant32
    B, nv, rng = 6, int(mc.nv), np.random.RandomState(42)
    pts, f, tq, v = _rand(rng, B, 1, 3, dtype=F32), _rand(rng, B, 1, 3, dtype=F32), _rand(rng, B, 1, 3, dtype=F32), _rand(rng, B, 1, nv, dtype=F32)
    jp, jr = mt.jac(mx, d, pts, [7])
    wp, wr = mt.jac(mx, d, pts[:, 0], 7)
    assert jp.shape == (B, 1, nv, 3) == jr.shape and wp.shape == (B, nv, 3)
    assert torch.equal(jp[:, 0], wp) and torch.equal(jr[:, 0], wr) and wp.any()
    assert torch.equal(mt.jac(mx, d, pts[:, 0], torch.tensor([7]))[0], jp)  # (3,) points per environment with a one-element list
    q = mt.apply_ft(mx, d, f, tq, pts, [7])
    assert q.shape == (B, 1, nv) and torch.equal(q[:, 0], mt.apply_ft(mx, d, f[:, 0], tq[:, 0], pts[:, 0], 7)) and q.any()
    for fn in (mt.mul_m, mt.solve_m):
        out = fn(mx, d, v)
        assert out.shape == (B, 1, nv) and torch.equal(out[:, 0], fn(mx, d, v[:, 0])) and out.any()


def test_a_shared_point_with_listed_ids(ant32):
    mc, mx, d = ant32
    B, nv, rng = 6, int(mc.nv), np.random.RandomState(43)
    ids = [0, 3, 7, 13]
    p, f, tq = _rand(rng, 3, dtype=F32), _rand(rng, 3, dtype=F32), _rand(rng, B, len(ids), 3, dtype=F32)
    jp, jr = mt.jac(mx, d, p, ids)
    wp, wr = mt.jac(mx, d, p.expand(B, len(ids), 3), ids)
    assert jp.shape == (B, len(ids), nv, 3) and torch.equal(jp, wp) and torch.equal(jr, wr) and jp[:, 1:].any() and not jp[:, 0].any()
    q = mt.apply_ft(mx, d, f, tq, p, ids)
    assert q.shape == (B, len(ids), nv) and torch.equal(q, mt.apply_ft(mx, d, f.expand(B, len(ids), 3), tq, p.expand(B, len(ids), 3), ids))


def test_non_contiguous_and_float64_queries(ant32):
    """Queries given as strided views, and as float64 tensors to a float32 Data, equal the contiguous float32 call bit for bit (a float64 query
    is rounded to the Data's dtype once, as ``.to`` does)."""
    mc, mx, d = ant32
    B, nv, rng = 6, int(mc.nv), np.random.RandomState(44)
    ids = [1, 5, 13]
    big = _rand(rng, B, 2 * len(ids), 6, dtype=F64)
    views = [big[:, ::2, :3], big[:, 1::2, 3:], big[:, ::2, 3:]]  # point, force, torque
    assert not any(t.is_contiguous() for t in views)
    same = [t.to(F32).contiguous() for t in views]
    vbig = _rand(rng, B, nv, 4, dtype=F64)
    vview, vsame = vbig.transpose(1, 2)[:, ::2], vbig.transpose(1, 2)[:, ::2].to(F32).contiguous()
    assert not vview.is_contiguous() and vview.shape == (B, 2, nv)
    for pick in (lambda t64, t32: t64, lambda t64, t32: t64.to(F32), lambda t64, t32: t32.double()):  # float64 view, float32 view, float64 contiguous
        p, f, tq = (pick(a, b) for a, b in zip(views, same))
        jp, jr = mt.jac(mx, d, p, ids)
        wp, wr = mt.jac(mx, d, same[0], ids)
        assert jp.dtype == F32 and torch.equal(jp, wp) and torch.equal(jr, wr) and jp.any()
        assert torch.equal(mt.apply_ft(mx, d, f, tq, p, ids), mt.apply_ft(mx, d, same[1], same[2], same[0], ids))
        for fn in (mt.mul_m, mt.solve_m):
            out = fn(mx, d, pick(vview, vsame))
            assert out.dtype == F32 and torch.equal(out, fn(mx, d, vsame)) and out.any()


def test_a_side_stream_runs_the_kernels_in_its_own_order(ant32):
    """A call on a non-default stream whose query is still being produced on that stream, read on that stream: the launch is ordered after the
    producer only if it went to the caller's current stream."""
    mc, mx, d = ant32
    B, nv, rng = 6, int(mc.nv), np.random.RandomState(45)
    v, pts = _rand(rng, B, 2, nv, dtype=F32), _rand(rng, B, 3, dtype=F32)
    want = (mt.mul_m(mx, d, v), mt.solve_m(mx, d, v), mt.xfrc_accumulate(mx, d)) + mt.jac(mx, d, pts, 9)
    ones = torch.ones(1 << 24, dtype=F64, device=DEV)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        one = torch.ones((), dtype=F64, device=DEV)
        for _ in range(40):  # exactly 1.0, after some milliseconds of queued work
            one = one * (ones.sum() / ones.numel())
        v2, p2 = (v * one).to(F32), (pts * one).to(F32)
        got = (mt.mul_m(mx, d, v2), mt.solve_m(mx, d, v2), mt.xfrc_accumulate(mx, d)) + mt.jac(mx, d, p2, 9)
        got = [g.cpu() for g in got]  # the read, on the same stream
    s.synchronize()
    for g, w in zip(got, want):
        assert torch.equal(g, w.cpu())


def test_an_empty_batch_returns_empty_outputs(ant32):
    mc, mx, d = ant32
    nv = int(mc.nv)
    d0 = d[:0]
    assert d0.qpos.shape == (0, int(mc.nq))
    e = lambda *s: torch.zeros(*s, dtype=F32, device=DEV)
    jp, jr = mt.jac(mx, d0, e(0, 2, 3), [1, 2])
    assert jp.shape == (0, 2, nv, 3) == jr.shape and jp.dtype == F32 and jp.device.type == "cuda"
    assert mt.jac(mx, d0, e(3), 4)[0].shape == (0, nv, 3)
    assert mt.apply_ft(mx, d0, e(3), e(0, 3), e(0, 2, 3), [1, 2]).shape == (0, 2, nv)
    assert mt.xfrc_accumulate(mx, d0).shape == (0, nv)
    assert mt.mul_m(mx, d0, e(0, 3, nv)).shape == (0, 3, nv) and mt.solve_m(mx, d0, e(nv)).shape == (0, nv)
