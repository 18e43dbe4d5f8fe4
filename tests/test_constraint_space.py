"""The constraint-space functions on the device (mul_jac_vec, mul_jac_t_vec, constraint_update, efc_ar; csrc/mjh_efc.h) against the numpy longdouble reference
tests/_efc_ref.py -- which tests/test_constraint_space_host.py pins on the recordings -- evaluated on the SAME rounded inputs: the leaves of this library's own
``forward`` on the seeded batches of tests/_cases.py, B in {1, 3, 70}.

No bound here is read off the kernels.  Values are held to ``TOL_PRE[dtype]`` by ``_util.rel_err``; ``AR`` to ``max(TOL_PRE, 4 x the error of the composition
torch.bmm(J, solve_m(J)^T) + diag R`` of kernels that existed before, on the same inputs) -- a triangular solve's error scales with cond(M), and the factor 4
covers another summation order of the same condition-limited computation; the pass's own ``efc_force`` / ``qfrc_constraint`` to ``TOL_SOL[dtype]``; states on the rows ``_efc_ref.comparable`` keeps, with at most 1 % left out.  The dual identity is read on the scale
of its terms: every entry of ``AR`` and of ``efc_force`` carries one rounding of the dtype, so the residual is a rounding of ``sum_j |AR_ij f_j|``, not of the
``jar`` those terms cancel to.

Measured (one MI355X), worst over the batch sizes: the values 1.3e-14 (float64, equality loops) and 1.6e-6 (float32, centipede_154) by ``rel_err``; ``AR`` 3.7e-16 /
2.4e-7 against the composition's 3.4e-16 / 1.3e-7, never past 2.0 x it; the pass's own forces 7.4e-14 / 9.4e-6; the dual identity 6.0e-16 / 3.0e-7 of its terms; no
row's state had to be left out.
"""
import ctypes
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import _efc_ref as er
import mujoco_torch_amd as mt
from _cases import F32, F64, TOL_PRE, TOL_SOL, seeded_batch
from _util import rel_err
from mujoco_torch_amd import constraint_space as cs
from mujoco_torch_amd import native

pytestmark = pytest.mark.gpu

DEV = "cuda"
LD = er.LD
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = [("humanoid", F64), ("ant_frictionloss", F64), ("ant_frictionloss", F32), ("equality_loops", F64), ("centipede_83", F64), ("centipede_154", F32)]
BATCHES = (1, 3, 70)
IDS = [f"{x}-{str(t)[6:]}" for x, t in MODELS]
K = 3
STATE_CAP = 0.01
LEAVES = ("efc_J", "efc_D", "efc_aref", "efc_frictionloss", "efc_force", "qfrc_constraint", "qacc", "qM", "qLD", "qfrc_smooth", "qacc_smooth")
PERTURB = 0.25  # of the largest |qacc| of the environment: moves rows across their zone boundaries


def sizes(m):
    ne, nf, _, _, nefc = m.constraint_sizes_py
    floss = nf > 0 and not (int(m.opt.disableflags) & mt.DisableBit.FRICTIONLOSS)
    return int(ne + nf), bool(floss), int(nefc), int(m.nv), float(m.stat.meaninertia) * max(1, int(m.nv))


def host(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def passed(xml, dtype, B):
    """(host model, device model, Data after forward on the device, its leaves on the host [B, ...], query tensors): computed once and shared."""
    mc, d = seeded_batch(xml, {}, dtype, B)
    mx = mc.to(DEV)
    d = mt.forward(mx, d.to(DEV))
    _, _, nefc, nv, _ = sizes(mc)
    tail = dict(efc_J=(nefc, nv), qM=(nv, nv), qLD=(nv, nv))
    A = {n: host(getattr(d, n)).reshape((B,) + tail.get(n, (-1,))) for n in LEAVES}
    rng = np.random.RandomState(11)
    q = dict(v=torch.tensor(rng.randn(B, K, nv), dtype=dtype, device=DEV), f=torch.tensor(rng.randn(B, K, nefc), dtype=dtype, device=DEV))
    q["qacc2"] = d.qacc + PERTURB * d.qacc.abs().amax(-1, keepdim=True) * torch.tensor(rng.randn(B, nv), dtype=dtype, device=DEV)
    return mc, mx, d, A, q


def reference_update(mc, A, qacc):
    ne_nf, floss, _, _, scale = sizes(mc)
    return er.constraint_update(A["efc_J"], A["efc_D"], A["efc_aref"], A["efc_frictionloss"], ne_nf, floss, qacc=qacc, qM=A["qM"], qfrc_smooth=A["qfrc_smooth"],
                                qacc_smooth=A["qacc_smooth"], inertia_scale=scale)


def check(what, got, want, tol, floor=None):
    e = rel_err(host(got) if isinstance(got, torch.Tensor) else got, np.asarray(want, dtype=np.float64), *(() if floor is None else (floor,)))
    print(f"  {what}: rel_err {e:.3g} ({e / tol:.2g} of {tol:g})")
    assert np.isfinite(e) and e <= tol, (what, e, tol)
    return e


def check_states(what, mc, A, qacc, got, eps):
    ne_nf, floss, _, _, _ = sizes(mc)
    want = reference_update(mc, A, qacc)["efc_state"]
    dist, bound = er.state_margin(A["efc_J"], qacc, A["efc_aref"], A["efc_D"], A["efc_frictionloss"], ne_nf, floss, eps)
    keep = er.comparable(dist, bound)
    out = 1 - keep.mean()
    hist = np.bincount(want.reshape(-1), minlength=4).tolist()
    print(f"  {what}: states (satisfied, quadratic, linear-neg, linear-pos) {hist}; {int((~keep).sum())} of {keep.size} rows left out ({out:.2%})")
    assert out <= STATE_CAP
    assert (host(got) == want)[keep].all(), what
    return hist


# ---- the plan --------------------------------------------------------------------------------------------------------------------------------

def test_the_large_models_reach_three_chunks_with_a_short_last_one():
    for xml, dtype in (("centipede_83", F64), ("centipede_154", F32)):
        mc = passed(xml, dtype, 1)[0]
        _, _, nefc, nv, _ = sizes(mc)
        for op in (cs.MUL_J, cs.MUL_JT, cs.UPDATE, cs.AR):
            chunk, nchunk, last, lds = cs.plan(op, nv, nefc, dtype)
            assert nchunk >= 3 and 0 < last < chunk and (nchunk - 1) * chunk + last == nefc, (xml, op, chunk, nchunk, last)
            assert lds <= 160 * 1024
    mc = passed("humanoid", F64, 1)[0]
    assert sizes(mc)[2] % 64 != 0 and cs.plan(cs.AR, int(mc.nv), sizes(mc)[2], F64)[1] == 1  # one chunk, rows not a multiple of the wavefront
    assert cs.plan(cs.UPDATE, 8, 256, F64)[1] == 2  # the ant in float64: two chunks


# ---- the kernels against the reference -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("xml,dtype", MODELS, ids=IDS)
def test_kernels_against_the_reference(xml, dtype, B):
    mc, mx, d, A, q = passed(xml, dtype, B)
    ne_nf, floss, nefc, nv, scale = sizes(mc)
    tol, eps = TOL_PRE[dtype], float(torch.finfo(dtype).eps)
    print(f"{xml} {dtype} B={B}: nv {nv}, nefc {nefc}")
    check("mul_jac_vec", mt.mul_jac_vec(mx, d, q["v"]), er.mul_jac_vec(A["efc_J"], host(q["v"])), tol)
    check("mul_jac_t_vec", mt.mul_jac_t_vec(mx, d, q["f"]), er.mul_jac_t_vec(A["efc_J"], host(q["f"])), tol)
    seen = np.zeros(4, dtype=np.int64)
    for what, qacc in (("qacc", None), ("perturbed qacc", q["qacc2"])):
        u = mt.constraint_update(mx, d, qacc)
        qh = A["qacc"] if qacc is None else host(qacc)
        want = reference_update(mc, A, qh)
        for n in ("jar", "efc_force", "qfrc_constraint", "gauss", "cost"):
            check(f"{what}: {n}", getattr(u, n), want[n], tol)
        # grad = M qacc - qfrc_smooth - qfrc_constraint.  At a general qacc it is read like the rest.  At the pass's own qacc the three terms cancel to the solver's
        # residual, thousands of times smaller than they are, and the result of ANY evaluation in the dtype is a rounding of the terms: there the scale is the
        # largest term (plain float32 numpy on the 154-dof centipede: 1.3e-3 of the largest |grad|, 1e-7 of the largest term)
        terms = max(float(np.abs(x).max()) for x in (want["grad"] + A["qfrc_smooth"] + want["qfrc_constraint"], A["qfrc_smooth"], want["qfrc_constraint"]))
        floor = terms if qacc is None else None
        check(f"{what}: grad" + (" (on the scale of its terms)" if qacc is None else ""), u.grad, want["grad"], tol, floor)
        # |grad_norm error| <= |grad error|_2 / scale <= sqrt(nv) x the bound on grad's entries, relative to a largest grad_norm no smaller than max|grad| / scale
        check(f"{what}: grad_norm", u.grad_norm, want["grad_norm"], tol * np.sqrt(nv), None if floor is None else floor / scale)
        seen += check_states(what, mc, A, qh, u.efc_state, eps)
        uj = mt.constraint_update(mx, d, jar=u.jar)  # the mj_constraintUpdate form on the kernel's own jar: the same decisions and forces, bit for bit
        assert uj.gauss is None and torch.equal(uj.efc_state, u.efc_state) and torch.equal(uj.efc_force, u.efc_force) and torch.equal(uj.qfrc_constraint, u.qfrc_constraint)
        check(f"{what}: cost without gauss", uj.cost, np.asarray(want["cost"] - want["gauss"], dtype=np.float64), tol)
    assert seen[er.QUADRATIC] > 0 and seen[er.SATISFIED] > 0
    if floss and B >= 3:
        assert seen[er.LINEAR_NEG] > 0 and seen[er.LINEAR_POS] > 0, seen
    dual = mt.efc_ar(mx, d)
    AR, b = er.efc_ar(A["efc_J"], A["efc_D"], A["efc_aref"], A["qLD"], A["qacc_smooth"])
    check("b", dual.b, b, tol)
    assert torch.equal(dual.AR, dual.AR.transpose(-1, -2).contiguous())
    J = d.efc_J.reshape(B, nefc, nv)
    Dd = d.efc_D.reshape(B, nefc)
    comp = torch.bmm(J, mt.solve_m(mx, d, J).transpose(-1, -2)) + torch.diag_embed(torch.where(Dd > 0, 1 / Dd, torch.zeros_like(Dd)))
    want = np.asarray(AR, dtype=np.float64)
    e_comp, e_new = rel_err(host(comp), want), rel_err(host(dual.AR), want)
    print(f"  AR: rel_err {e_new:.3g}, the composition bmm(J, solve_m(J)^T) {e_comp:.3g}, bound {max(tol, 4 * e_comp):.3g}")
    assert e_new <= max(tol, 4 * e_comp)
    # ... and with the diagonal left out: R = 1 / D of an inactive contact's row is the largest entry by orders of magnitude, and would be the scale of the above
    off = ~np.eye(nefc, dtype=bool)
    o_comp, o_new = rel_err(host(comp)[:, off], want[:, off]), rel_err(host(dual.AR)[:, off], want[:, off])
    print(f"  AR off the diagonal: rel_err {o_new:.3g}, the composition {o_comp:.3g}, bound {max(tol, 4 * o_comp):.3g}; largest |AR| {np.abs(want).max():.3g}, off the diagonal {np.abs(want[:, off]).max():.3g}")
    assert o_new <= max(tol, 4 * o_comp)


@pytest.mark.parametrize("xml,dtype", MODELS, ids=IDS)
def test_the_pass_itself_is_reproduced(xml, dtype):
    """After ``forward``, ``constraint_update(m, d)`` gives the pass's own ``efc_force`` and ``qfrc_constraint`` at TOL_SOL[dtype] by ``_util.rel_err``, per
    environment; ``grad_norm`` then says how far from converged each environment was left."""
    mc, mx, d, A, _ = passed(xml, dtype, 70)
    u = mt.constraint_update(mx, d)
    got = dict(efc_force=host(u.efc_force), qfrc_constraint=host(u.qfrc_constraint))
    worst = {n: max(rel_err(got[n][e], A[n][e]) for e in range(70)) for n in got}
    print(f"{xml} {dtype}: efc_force {worst['efc_force']:.3g}, qfrc_constraint {worst['qfrc_constraint']:.3g}; "
          f"grad_norm median {float(u.grad_norm.median()):.3g}, max {float(u.grad_norm.max()):.3g} (opt.tolerance {float(mc.opt.tolerance):g})")
    assert max(worst.values()) <= TOL_SOL[dtype], worst


@pytest.mark.parametrize("xml,dtype", MODELS, ids=IDS)
def test_the_dual_identity_on_device_outputs(xml, dtype):
    """``jar - ((AR - diag R) f + b) = J M^-1 grad`` with ``M^-1`` by the ``solve_m`` kernel, M the matrix ``qLD`` factors (``qM + 1e-10 I`` past 16 dofs:
    ``grad`` takes ``1e-10 qacc`` there, tests/test_constraint_space_host.py).  The combination runs in longdouble on the host from the device's outputs; the
    residual is held to TOL_PRE on the scale of the identity's terms, |jar| + sum_j |AR_ij f_j| + |R_i f_i| + |b| + |J| |M^-1 grad|."""
    mc, mx, d, A, q = passed(xml, dtype, 70)
    _, _, nefc, nv, _ = sizes(mc)
    u = mt.constraint_update(mx, d, q["qacc2"])
    dual = mt.efc_ar(mx, d)
    grad = u.grad + (1e-10 * q["qacc2"] if nv > 16 else 0)
    x = er.ld(host(mt.solve_m(mx, d, grad)))
    AR, b, f, jar, J = (er.ld(host(t)) for t in (dual.AR, dual.b, u.efc_force, u.jar, d.efc_J.reshape(70, nefc, nv)))
    R = er.efc_R(A["efc_D"])
    lhs = jar - (np.einsum("bij,bj->bi", AR, f) - R * f + b)
    rhs = np.einsum("bnv,bv->bn", J, x)
    terms = np.abs(jar) + np.einsum("bij,bj->bi", np.abs(AR), np.abs(f)) + np.abs(R * f) + np.abs(b) + np.einsum("bnv,bv->bn", np.abs(J), np.abs(x))
    floor = 1e-6 if dtype == F64 else 1e-3  # (_util.rel_err's: an environment without a single active row has nothing but zeros here)
    err = float((np.abs(lhs - rhs).max(-1) / np.maximum(terms.max(-1), floor)).max())
    print(f"{xml} {dtype}: residual / terms {err:.3g} ({err / TOL_PRE[dtype]:.2g} of the bound); residual / max|jar| {float(np.abs(lhs - rhs).max() / np.abs(jar).max()):.3g}")
    assert err <= TOL_PRE[dtype]


# ---- bit identities --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("xml,dtype", MODELS, ids=IDS)
def test_rows_vectors_and_environments_are_independent(xml, dtype):
    mc, mx, d, A, q = passed(xml, dtype, 70)
    _, _, nefc, nv, _ = sizes(mc)
    many = mt.mul_jac_vec(mx, d, q["v"]), mt.mul_jac_t_vec(mx, d, q["f"])
    for j in range(K):  # row j of a K-vector call is the single-vector call
        assert torch.equal(many[0][:, j], mt.mul_jac_vec(mx, d, q["v"][:, j].contiguous()))
        assert torch.equal(many[1][:, j], mt.mul_jac_t_vec(mx, d, q["f"][:, j].contiguous()))
    assert torch.equal(mt.mul_jac_vec(mx, d, q["v"][:, :1].contiguous()), many[0][:, :1])  # (K = 1 with its dimension kept)
    for fn, shared in ((mt.mul_jac_vec, q["v"][0, 0].contiguous()), (mt.mul_jac_t_vec, q["f"][0, 0].contiguous())):  # a shared vector is that vector repeated
        assert torch.equal(fn(mx, d, shared), fn(mx, d, shared.expand(70, -1).contiguous()))
    u, dual = mt.constraint_update(mx, d, q["qacc2"]), mt.efc_ar(mx, d)
    for e in (0, 37, 69):  # environment e of the batch is the call on environment e alone
        one = d[e:e + 1]
        assert torch.equal(mt.mul_jac_vec(mx, one, q["v"][e:e + 1]), many[0][e:e + 1]) and torch.equal(mt.mul_jac_t_vec(mx, one, q["f"][e:e + 1]), many[1][e:e + 1])
        u1, dual1 = mt.constraint_update(mx, one, q["qacc2"][e:e + 1]), mt.efc_ar(mx, one)
        for a, b in zip(tuple(u1) + tuple(dual1), tuple(u) + tuple(dual)):
            assert torch.equal(a, b[e:e + 1])
    assert torch.equal(dual.AR, dual.AR.transpose(-1, -2).contiguous())


_CUT_CHILD = r'''
import sys
sys.path.insert(0, "tests"); sys.path.insert(0, "mujoco-torch_amd"); sys.path.insert(0, "oracle")
import torch, mujoco_torch_amd as mt
import test_constraint_space as t
res = {}
for spec in sys.argv[2:]:
    xml, dts = spec.split(":")
    mc, mx, d, A, q = t.passed(xml, getattr(torch, dts), 70)
    out = {k: getattr(d, k) for k in ("efc_J", "efc_D", "qM", "qLD", "qacc")}  # the leaves: a difference there is forward's
    out["mul_jac_vec"], out["mul_jac_t_vec"] = mt.mul_jac_vec(mx, d, q["v"]), mt.mul_jac_t_vec(mx, d, q["f"])
    out.update({"update_" + k: v for k, v in mt.constraint_update(mx, d, q["qacc2"])._asdict().items()})
    out.update(mt.efc_ar(mx, d)._asdict())
    res[spec] = {k: o.cpu() for k, o in out.items()}
torch.save(res, sys.argv[1])
print("ran")
'''
CUT_MODELS = (("humanoid", "float64"), ("ant_frictionloss", "float32"), ("centipede_83", "float64"))


def test_a_batch_cut_into_several_launches_is_bit_identical():
    """MJH_MAX_GRID_LOG2=2 caps a launch at 4 workgroups, one environment each: 70 environments go out as 18 launches, the last one of 2, and every output must
    equal the single launch of the default bit for bit (fresh child processes: the library reads the switch once)."""
    with tempfile.TemporaryDirectory() as td:
        res = {}
        for tag, env in (("one", {}), ("cut", {"MJH_MAX_GRID_LOG2": "2"})):
            f = os.path.join(td, tag + ".pt")
            base = {k: v for k, v in os.environ.items() if k != "MJH_MAX_GRID_LOG2"}
            r = subprocess.run([sys.executable, "-c", _CUT_CHILD, f] + [f"{x}:{t}" for x, t in CUT_MODELS], cwd=ROOT, env=dict(base, **env), capture_output=True,
                               text=True, timeout=600)
            assert r.returncode == 0 and "ran" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
            res[tag] = torch.load(f)
    assert len(res["one"]) == len(CUT_MODELS)
    for case, outs in res["one"].items():
        assert len(outs) == 5 + 2 + 8 + 2
        for k, a in outs.items():
            assert a.shape[0] == 70 and a.any() and (a.dtype == torch.int32 or torch.isfinite(a).all()), (case, k)
            assert torch.equal(a, res["cut"][case][k]), (case, k)


# ---- edges ------------------------------------------------------------------------------------------------------------------------------------

def test_a_model_without_rows():
    mc, d = seeded_batch("humanoid", {"disableflags": 1}, F64, 3)
    mx = mc.to(DEV)
    d = mt.forward(mx, d.to(DEV))
    nv = int(mc.nv)
    assert sizes(mc)[2] == 0
    assert tuple(mt.mul_jac_vec(mx, d, d.qacc).shape) == (3, 0) and tuple(mt.efc_ar(mx, d).AR.shape) == (3, 0, 0)
    u = mt.constraint_update(mx, d)
    assert tuple(u.jar.shape) == (3, 0) and tuple(u.qfrc_constraint.shape) == (3, nv) and not u.qfrc_constraint.any()
    # without constraints the pass's qacc IS qacc_smooth = (qM + 1e-10 I)^-1 qfrc_smooth (27 dofs: the regularised factor): no cost, and a gradient
    # qM qacc - qfrc_smooth = -1e-10 qacc, read on the scale of qfrc_smooth
    assert torch.equal(d.qacc, d.qacc_smooth) and not u.cost.any() and not u.gauss.any()
    e = rel_err(host(u.grad), -1e-10 * host(d.qacc), float(d.qfrc_smooth.abs().max()))
    print(f"no rows: grad against -1e-10 qacc on the scale of qfrc_smooth {e:.3g}; grad_norm {host(u.grad_norm)}")
    assert e <= TOL_PRE[F64]
    assert torch.allclose(u.grad_norm, u.grad.norm(dim=-1) / sizes(mc)[4], rtol=1e-12, atol=0)


def test_kernel_ids_and_byte_accounts():
    """The four kernels report under their timing ids (50 .. 53), one launch a call, and ``mjh_model_kernel_io`` accounts them per environment."""
    mc, mx, d, A, q = passed("humanoid", F64, 3)
    _, _, n, nv, _ = sizes(mc)
    nm = native.get_native_model(mx, torch.device("cuda", 0), F64)
    rw = (ctypes.c_int64 * 2)()
    want = {50: ((n * nv + nv) * 8, n * 8), 51: ((n * nv + n) * 8, nv * 8), 52: ((n * nv + 3 * n + nv * nv + 3 * nv) * 8, (2 * n + 2 * nv + 3) * 8 + 4 * n),
            53: ((n * nv + nv * nv + 2 * n + nv) * 8, (n * n + n) * 8)}
    calls = {50: lambda: mt.mul_jac_vec(mx, d, d.qacc), 51: lambda: mt.mul_jac_t_vec(mx, d, d.efc_force), 52: lambda: mt.constraint_update(mx, d), 53: lambda: mt.efc_ar(mx, d)}
    for kid, call in calls.items():
        assert nm.lib.mjh_model_kernel_io(nm.handle, kid, rw) == 0 and (rw[0], rw[1]) == want[kid], kid
        nm.lib.mjh_debug_phase_timing(1)
        try:
            call()
            ms, ids = (ctypes.c_float * 16)(), (ctypes.c_int * 16)()
            k = nm.lib.mjh_debug_phase_times(ms, ids, 16)
        finally:
            nm.lib.mjh_debug_phase_timing(0)
        assert [ids[i] for i in range(k)] == [kid] and ms[0] > 0, kid


def test_a_side_stream_and_non_contiguous_queries():
    mc, mx, d, A, q = passed("ant_frictionloss", F32, 3)
    want = mt.mul_jac_vec(mx, d, q["v"])
    wide = torch.zeros(3, K, 2 * int(mc.nv), dtype=F32, device=DEV)
    wide[..., ::2] = q["v"]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = mt.mul_jac_vec(mx, d, wide[..., ::2])
    s.synchronize()
    assert torch.equal(got, want)
