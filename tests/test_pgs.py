"""``solve_pgs`` on the device (csrc/mjh_pgs.h) against the numpy longdouble reference tests/_pgs_ref.py -- the definitions in the ``AR`` form, which
tests/test_pgs_host.py pins on a hand-worked problem and on the recordings -- evaluated on the SAME rounded inputs: the leaves of this library's own ``forward`` on the
seeded batches of tests/_cases.py, B in {1, 3, 70}.  The large models are the largest centipedes that both pass ``forward`` in the dtype and fit the solver's plan:
``centipede_106`` in float64 (5 staging steps of 19 rows and a last one of 4; 106 dofs) and ``centipede_154`` in float32 (26 + 26 + 26 + 22; 154 dofs).

No bound here is read off the kernel.  Values are held to ``max(TOL_PRE[dtype], 4 x the error of _pgs_ref run in the same dtype on the same inputs)`` by
``_util.rel_err``, the rule tests/test_constraint_space.py uses for ``AR``: the factor 4 covers another summation order of a computation limited by the condition
of ``M``.  (Where a sweep finds nothing left to improve -- the ant's ``AR`` is diagonal, its second sweep starts at the fixed point -- ``improvement`` is the
rounding residue ``1/2 delta^2 AR_ii`` of the last bits of ``f`` in ANY arithmetic of the dtype, the reference's own included: that is what the second term of the
bound measures.)  Feasibility and the bit identities carry no tolerance.  The slacks of the cost inequalities are written down where they are used.

Measured (one MI355X), worst over B, the sweep counts and both starts: ``efc_force`` 8.2e-15 (float64, humanoid) / 5.0e-7 (float32, centipede_154), ``qacc`` 1.1e-14 /
8.3e-7, ``cost`` 1.7e-14 / 3.2e-7, ``improvement`` 6.4e-13 / 3.2e-6 by ``rel_err`` -- at most 1.7e-5 (float64) and 1.6e-2 (float32) of the bound, which is its
``TOL_PRE`` term everywhere but for the ant's ``improvement`` from ``force0`` in float32 (the parenthesis above): 1.8e5 of the 1e-3 floor from the kernel and from
the reference in float32 alike, 0.25 of the bound.  Stopping: 3 to 10 sweeps on the humanoid, 1 to 12 on the equality loops and centipede_154, 2 to 12 on
centipede_106, 2 on the ant.  The dual cost never rose; ``cost + primal`` reaches -0.49 of its slack at worst (centipede_106, an environment without an active row).
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
import _pgs_ref as pr
import mujoco_torch_amd as mt
from _cases import F32, F64, TOL_PRE, seeded_batch
from _util import rel_err
from mujoco_torch_amd import native
from mujoco_torch_amd import pgs

pytestmark = pytest.mark.gpu

DEV = "cuda"
LD = er.LD
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = [("humanoid", F64), ("ant_frictionloss", F64), ("ant_frictionloss", F32), ("equality_loops", F64), ("centipede_106", F64), ("centipede_154", F32)]
IDS = [f"{x}-{str(t)[6:]}" for x, t in MODELS]
BATCHES = (1, 3, 70)
SWEEPS = (1, 2, 7)
LEAVES = ("efc_J", "efc_D", "efc_aref", "efc_frictionloss", "efc_force", "qLD", "qM", "qacc_smooth", "qfrc_smooth", "qacc")
NAMES = ("efc_force", "qfrc_constraint", "qacc", "cost", "improvement")
NPDT = {F64: np.float64, F32: np.float32}


def sizes(m):
    ne, nf, _, _, nefc = (int(x) for x in m.constraint_sizes_py)
    return ne, nf, nefc, int(m.nv), float(m.stat.meaninertia) * max(1, int(m.nv))


def host(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def passed(xml, dtype, B):
    """(host model, device model, Data after forward on the device, its leaves on the host [B, ...], an infeasible start on the device): computed once and shared."""
    mc, d = seeded_batch(xml, {}, dtype, B)
    mx = mc.to(DEV)
    d = mt.forward(mx, d.to(DEV))
    ne, nf, nefc, nv, _ = sizes(mc)
    tail = dict(efc_J=(nefc, nv), qM=(nv, nv), qLD=(nv, nv))
    A = {n: host(getattr(d, n)).reshape((B,) + tail.get(n, (-1,))) for n in LEAVES}
    # a start of the size of the pass's forces with both signs everywhere: negative on unilateral rows, past the bounds on the friction rows
    rng = np.random.RandomState(5)
    f0 = torch.tensor(rng.randn(B, nefc) * max(float(np.abs(A["efc_force"]).max()), 1.0), dtype=dtype, device=DEV)
    return mc, mx, d, A, f0


@functools.lru_cache(maxsize=None)
def reference(xml, dtype, B, warm, sweeps=max(SWEEPS)):
    """(the longdouble reference, the reference in the dtype) of ``sweeps`` sweeps with ``tolerance = 0``: every sweep's force, improvement and cost."""
    mc, _, _, A, f0 = passed(xml, dtype, B)
    ne, nf, _, _, scale = sizes(mc)
    args = (A["efc_J"], A["efc_D"], A["efc_aref"], A["efc_frictionloss"], A["qLD"], A["qacc_smooth"], ne, nf, scale, sweeps)
    start = host(f0) if warm else None
    return pr.solve_pgs(*args, force0=start), pr.solve_pgs(*args, force0=start, dtype=NPDT[dtype])


def at_sweep(A, ref, k, dtype=LD):
    qfrc, qacc = pr.finish(A["efc_J"], A["qLD"], A["qacc_smooth"], ref["forces"][k], dtype)
    imp = ref["improvements"][k - 1] if k else np.zeros(len(qfrc))
    return dict(efc_force=ref["forces"][k], qfrc_constraint=qfrc, qacc=qacc, cost=ref["costs"][k], improvement=imp)


def f64(x):
    return np.asarray(x, dtype=np.float64)


# ---- fixed sweeps against the reference -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("warm", [False, True], ids=["cold", "force0"])
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("xml,dtype", MODELS, ids=IDS)
def test_fixed_sweeps_against_the_reference(xml, dtype, B, warm):
    """``tolerance = 0``, 1, 2 and 7 sweeps, from zeros and from a random infeasible ``force0``: force, ``J^T f``, ``qacc``, cost and improvement against longdouble,
    each within ``max(TOL_PRE, 4 x the same-dtype reference's error)``; ``niter == iterations``.

    Measured (one MI355X), worst error / bound over B, the sweep counts and both starts (the kernel's ``rel_err`` / the same-dtype reference's, by output, are the
    table of ``solve_pgs`` in DESIGN.md): humanoid float64 1.7e-5, ant-frictionloss float64 6.4e-4 and float32 0.25 (``improvement`` at the fixed point: rounding in
    both, the same figure), equality loops 1.1e-5, centipede_106 float64 6.6e-6, centipede_154 float32 1.6e-2."""
    mc, mx, d, A, f0 = passed(xml, dtype, B)
    ref, same = reference(xml, dtype, B, warm)
    worst = 0.0
    print(f"{xml} {dtype} B={B} {'force0' if warm else 'cold'}: nv {sizes(mc)[3]}, nefc {sizes(mc)[2]}")
    for k in SWEEPS:
        res = mt.solve_pgs(mx, d, iterations=k, tolerance=0.0, force0=f0 if warm else None)
        assert (res.niter == k).all() and res.niter.dtype == torch.int32
        want, other = at_sweep(A, ref, k), at_sweep(A, same, k, NPDT[dtype])
        for n in NAMES:
            e_same, e_new = rel_err(f64(other[n]), f64(want[n])), rel_err(host(getattr(res, n)), f64(want[n]))
            bound = max(TOL_PRE[dtype], 4 * e_same)
            worst = max(worst, e_new / bound)
            print(f"  {k} sweeps: {n}: rel_err {e_new:.3g}, the reference in the dtype {e_same:.3g}, bound {bound:.3g} ({e_new / bound:.2g} of it)")
            assert np.isfinite(e_new) and e_new <= bound, (n, k, e_new, bound)
    print(f"  worst error / bound {worst:.3g}")


@pytest.mark.parametrize("xml,dtype", MODELS, ids=IDS)
def test_no_sweep_returns_the_projected_start(xml, dtype):
    mc, mx, d, A, f0 = passed(xml, dtype, 3)
    ne, nf, nefc, nv, _ = sizes(mc)
    res = mt.solve_pgs(mx, d, iterations=0, force0=f0)
    want = pr.project(host(f0), A["efc_frictionloss"], ne, nf)
    assert np.array_equal(host(res.efc_force), want) and not res.niter.any() and not res.improvement.any()
    ref = pr.solve_pgs(A["efc_J"], A["efc_D"], A["efc_aref"], A["efc_frictionloss"], A["qLD"], A["qacc_smooth"], ne, nf, sizes(mc)[4], 0, force0=host(f0))
    for n in ("qfrc_constraint", "qacc", "cost"):
        assert rel_err(host(getattr(res, n)), f64(ref[n])) <= TOL_PRE[dtype], n
    cold = mt.solve_pgs(mx, d, iterations=0)
    assert not cold.efc_force.any() and not cold.qfrc_constraint.any() and not cold.cost.any() and torch.equal(cold.qacc, d.qacc_smooth)
    shared = mt.solve_pgs(mx, d, iterations=2, tolerance=0.0, force0=f0[1].contiguous())  # a shared start is that start repeated
    assert all(torch.equal(a, b) for a, b in zip(shared, mt.solve_pgs(mx, d, iterations=2, tolerance=0.0, force0=f0[1].expand(3, -1).contiguous())))


# ---- feasibility ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("xml,dtype", MODELS, ids=IDS)
def test_feasibility_is_exact(xml, dtype):
    """After every number of sweeps, from either start: ``|f| <= efc_frictionloss`` on the friction rows and ``f >= 0`` on the later rows, exactly; from zeros the
    rows of inactive contacts (``J = 0``, ``aref = 0``) are exact zeros."""
    mc, mx, d, A, f0 = passed(xml, dtype, 70)
    ne, nf, nefc, nv, _ = sizes(mc)
    dead = ~A["efc_J"].any(-1) & (A["efc_aref"] == 0)
    dead[:, :ne + nf] = False
    print(f"{xml} {dtype}: {ne} equality, {nf} friction rows, {int(dead.sum())} of {dead.size} rows are inactive contacts'")
    for start in (None, f0):
        for k in (0, 1, 3, 16):
            f = host(mt.solve_pgs(mx, d, iterations=k, tolerance=0.0, force0=start).efc_force)
            assert np.isfinite(f).all()
            assert (np.abs(f[:, ne:ne + nf]) <= A["efc_frictionloss"][:, ne:ne + nf]).all()
            assert (f[:, ne + nf:] >= 0).all()
            if start is None:
                assert not f[dead].any()
    if nf:
        f = host(mt.solve_pgs(mx, d, iterations=1, tolerance=0.0, force0=f0).efc_force)
        assert (np.abs(f[:, ne:ne + nf]) == A["efc_frictionloss"][:, ne:ne + nf]).any()  # (some friction row sits on its bound)
    if xml == "ant_frictionloss":
        assert dead.any()


# ---- stopping ---------------------------------------------------------------------------------------------------------------------------------

STOP_SWEEPS = 12


@pytest.mark.parametrize("xml,dtype", MODELS, ids=IDS)
def test_environments_stop_on_their_own(xml, dtype):
    """``tolerance`` is the median over the environments of the reference's improvement at the fifth sweep, so that about half of them have stopped by then and
    the rest go on (the ant: its ``AR`` is diagonal, every environment is at the fixed point after one sweep and finds an improvement of rounding size at the
    second -- no tolerance separates environments there; with ``tolerance = 1``, seven orders of magnitude from either improvement, all stop at sweep 2).  Nothing
    is compared with the reference's stopping sweep: an improvement next to the tolerance may fall on either side of it.  What holds on the device's own numbers:
    ``niter <= iterations``; ``improvement < tolerance`` wherever ``niter < iterations``; the environments that stopped last had ``improvement >= tolerance`` one
    sweep earlier; and an environment's force is the force of ``niter`` sweeps at ``tolerance = 0``, bit for bit."""
    mc, mx, d, A, _ = passed(xml, dtype, 70)
    ref, _ = reference(xml, dtype, 70, False, STOP_SWEEPS)
    ant = xml == "ant_frictionloss"
    tol = 1.0 if ant else float(np.median(f64(ref["improvements"][4])))
    res = mt.solve_pgs(mx, d, iterations=STOP_SWEEPS, tolerance=tol)
    niter = host(res.niter)
    print(f"{xml} {dtype}: tolerance {tol:.3g}; niter histogram {np.bincount(niter, minlength=STOP_SWEEPS + 1).tolist()}")
    assert (niter >= 1).all() and (niter <= STOP_SWEEPS).all()
    early = niter < STOP_SWEEPS
    assert (host(res.improvement)[early] < tol).all()
    if ant:
        assert (niter == 2).all()
    else:
        assert len(np.unique(niter)) >= 2, niter
    last = int(niter.max())
    if last > 1:
        before = mt.solve_pgs(mx, d, iterations=last - 1, tolerance=0.0)
        assert (before.niter == last - 1).all()
        assert (host(before.improvement)[niter == last] >= tol).all()
    for k in np.unique(niter):
        fixed = mt.solve_pgs(mx, d, iterations=int(k), tolerance=0.0)
        assert (fixed.niter == int(k)).all()
        rows = torch.tensor(niter == k, device=DEV)
        for a, b in zip(res, fixed):
            assert torch.equal(a[rows], b[rows]), k


# ---- monotone and dual ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("xml,dtype", MODELS, ids=IDS)
def test_the_cost_falls_and_stays_above_minus_the_primal(xml, dtype):
    """The dual cost after 1, 4 and 16 sweeps is non-increasing, and ``cost + constraint_update(m, d).cost >= 0`` (weak duality: the primal cost of ANY ``qacc``,
    here the pass's, is at least minus the dual cost of any feasible force) -- each up to what the dtype can hold:

    * rounding: an evaluation of the cost in the dtype is off by ``TOL_PRE`` of the sum S of the magnitudes of its terms
      (``1/2 sum |f_i AR_ij f_j| + sum |f_i b_i|``, longdouble from the device's force; the primal's: ``|cost|`` itself, its terms are all of one sign but for the
      linear zones') -- the bound the fixed-sweep test holds ``cost`` to; two costs are compared, so ``2 TOL_PRE S``;
    * the factor: ``AR`` is made from ``qLD``, the dtype's factor of ``qM``, the primal from ``qM`` itself: ``10 nv eps cond(M)`` of the dual's quadratic term
      (the bound of tests/test_constraint_space_host.py for ``AR`` against ``J M^-1 J^T``);
    * past 16 dofs ``qLD`` factors ``qM + 1e-10 I``: the primal of that matrix is larger by ``1/2 1e-10 qacc . (qacc - qacc_smooth)``, which the slack carries,
      as tests/test_constraint_space.py documents for the dual identity.

    ``grad_norm`` of ``constraint_update`` at the solver's ``qacc`` after 64 sweeps is below its value after 4, per environment -- unless the value after 4 is
    already at the rounding floor of ``grad``'s cancelling terms, ``(nefc + nv) eps max(|M qacc|, |qfrc_smooth|, |qfrc_constraint|) / scale``, or the four sweeps had
    reached the solver's fixed point (the force after 64 is the same bits: then so is ``grad_norm``)."""
    mc, mx, d, A, _ = passed(xml, dtype, 70)
    ne, nf, nefc, nv, scale = sizes(mc)
    eps, tol = float(torch.finfo(dtype).eps), TOL_PRE[dtype]
    AR, b, R = pr.dual(A["efc_J"], A["efc_D"], A["efc_aref"], A["qLD"], A["qacc_smooth"])
    runs = {k: mt.solve_pgs(mx, d, iterations=k, tolerance=0.0) for k in (1, 4, 16, 64)}
    S = {k: f64(np.einsum("bi,bij,bj->b", np.abs(er.ld(host(r.efc_force))), np.abs(AR), np.abs(er.ld(host(r.efc_force)))) / 2
                + (np.abs(er.ld(host(r.efc_force))) * np.abs(b)).sum(-1)) for k, r in runs.items()}
    cost = {k: host(r.cost).astype(np.float64) for k, r in runs.items()}
    for a, c in ((1, 4), (4, 16)):
        slack = 2 * tol * np.maximum(S[a], S[c])
        print(f"{xml} {dtype}: cost after {c} sweeps - after {a}: max {float((cost[c] - cost[a]).max()):.3g}, largest (difference / slack) {float(((cost[c] - cost[a]) / np.maximum(slack, 1e-300)).max()):.3g}")
        assert (cost[c] <= cost[a] + slack).all()
    primal = mt.constraint_update(mx, d)
    P = host(primal.cost).astype(np.float64)
    cond = np.array([np.linalg.cond(M) for M in A["qM"].astype(np.float64)])
    reg = 0.5e-10 * np.abs((A["qacc"].astype(np.float64) * (A["qacc"].astype(np.float64) - A["qacc_smooth"])).sum(-1)) if nv > 16 else 0.0
    for k in (1, 4, 16, 64):
        f = er.ld(host(runs[k].efc_force))
        quad = f64(np.einsum("bi,bij,bj->b", f, AR, f) / 2)
        slack = 2 * tol * (S[k] + np.abs(P)) + 10 * nv * eps * cond * np.abs(quad) + reg
        gap = cost[k] + P
        print(f"  {k} sweeps: dual + primal: min {float(gap.min()):.3g}, median {float(np.median(gap)):.3g}; smallest (gap / slack) {float((gap / np.maximum(slack, 1e-300)).min()):.3g}")
        assert (gap >= -slack).all()
    g = {k: mt.constraint_update(mx, d, runs[k].qacc) for k in (4, 64)}
    g4, g64 = host(g[4].grad_norm).astype(np.float64), host(g[64].grad_norm).astype(np.float64)
    terms = np.maximum.reduce([np.abs(host(g[4].grad + g[4].qfrc_constraint) + A["qfrc_smooth"]).max(-1), np.abs(A["qfrc_smooth"]).max(-1),
                               np.abs(host(g[4].qfrc_constraint)).max(-1)]).astype(np.float64)
    floor = (nefc + nv) * eps * terms / scale
    settled_n = int((host(runs[4].efc_force) == host(runs[64].efc_force)).all(-1).sum())
    print(f"  grad_norm after 4 sweeps: median {np.median(g4):.3g}, after 64: {np.median(g64):.3g}; {int((g4 <= floor).sum())} of 70 environments at the floor after 4, "
          f"{settled_n} at the fixed point; not below and neither: {np.flatnonzero(~((g64 < g4) | (g4 <= floor))).tolist()}")
    settled = (host(runs[4].efc_force) == host(runs[64].efc_force)).all(-1)  # (e.g. an environment none of whose rows is active: f = 0 from the first sweep on)
    assert ((g64 < g4) | (g4 <= floor) | settled).all() and (g64[settled] == g4[settled]).all()


# ---- bit identities ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("xml,dtype", MODELS, ids=IDS)
def test_an_environment_alone_is_its_row_of_the_batch(xml, dtype):
    mc, mx, d, A, f0 = passed(xml, dtype, 70)
    whole = mt.solve_pgs(mx, d, iterations=7, tolerance=0.0, force0=f0)
    for e in (0, 37, 69):
        one = mt.solve_pgs(mx, d[e:e + 1], iterations=7, tolerance=0.0, force0=f0[e:e + 1])
        for a, b in zip(one, whole):
            assert torch.equal(a, b[e:e + 1])


_CUT_CHILD = r'''
import sys
sys.path.insert(0, "tests"); sys.path.insert(0, "mujoco-torch_amd"); sys.path.insert(0, "oracle")
import torch, mujoco_torch_amd as mt
import test_pgs as t
res = {}
for spec in sys.argv[2:]:
    xml, dts = spec.split(":")
    mc, mx, d, A, f0 = t.passed(xml, getattr(torch, dts), 70)
    out = {k: getattr(d, k) for k in ("efc_J", "efc_D", "qLD", "qacc_smooth")}  # the leaves: a difference there is forward's
    out.update(mt.solve_pgs(mx, d, iterations=7, tolerance=0.0, force0=f0)._asdict())
    res[spec] = {k: o.cpu() for k, o in out.items()}
torch.save(res, sys.argv[1])
print("ran")
'''
CUT_MODELS = (("humanoid", "float64"), ("ant_frictionloss", "float32"), ("centipede_106", "float64"))


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
        assert len(outs) == 4 + 6
        for k, a in outs.items():
            assert a.shape[0] == 70 and a.any() and (a.dtype == torch.int32 or torch.isfinite(a).all()), (case, k)
            assert torch.equal(a, res["cut"][case][k]), (case, k)


# ---- the plan, the refusals, the bookkeeping -----------------------------------------------------------------------------------------------------

def test_the_large_models_stage_several_chunks_with_a_short_last_one():
    for xml, dtype in (("centipede_106", F64), ("centipede_154", F32)):
        mc = passed(xml, dtype, 1)[0]
        _, _, nefc, nv, _ = sizes(mc)
        chunk, nchunk, last, lds = pgs.plan(nv, nefc, dtype)
        assert nv > 32 and nchunk >= 3 and 0 < last < chunk and (nchunk - 1) * chunk + last == nefc and 64 * 1024 < lds <= 160 * 1024, (xml, chunk, nchunk, last, lds)
    for xml, dtype, over in (("centipede_121", F64, False), ("centipede_129", F64, False), ("centipede_154", F64, True)):  # (float64 forward stops at 106 dofs)
        mc, _ = seeded_batch(xml, {}, dtype, 1)
        _, _, nefc, nv, _ = sizes(mc)
        if over:
            with pytest.raises(RuntimeError, match=rf"nv = {nv}, nefc = {nefc} .* need \d+ bytes of LDS"):
                pgs.plan(nv, nefc, dtype)
        else:
            assert pgs.plan(nv, nefc, dtype)[3] <= 160 * 1024


def test_elliptic_cones_are_refused_before_any_launch(monkeypatch):
    mc, d = seeded_batch("ant", {"cone": 1}, F64, 3)
    mx = mc.to(DEV)
    d = mt.forward(mx, d.to(DEV))
    calls = []
    monkeypatch.setattr(pgs, "call", lambda *a, **k: calls.append(a))
    with pytest.raises(NotImplementedError, match="ELLIPTIC"):
        mt.solve_pgs(mx, d)
    assert not calls


def test_a_model_without_rows():
    mc, d = seeded_batch("humanoid", {"disableflags": 1}, F64, 3)
    mx = mc.to(DEV)
    d = mt.forward(mx, d.to(DEV))
    res = mt.solve_pgs(mx, d)
    assert tuple(res.efc_force.shape) == (3, 0) and tuple(res.qfrc_constraint.shape) == (3, int(mc.nv)) and not res.qfrc_constraint.any()
    assert torch.equal(res.qacc, d.qacc_smooth) and not res.cost.any() and not res.niter.any() and res.niter.dtype == torch.int32


def test_kernel_id_and_byte_account():
    """The kernel reports under timing id 54, one launch a call, and ``mjh_model_kernel_io`` accounts it per environment."""
    mc, mx, d, A, f0 = passed("humanoid", F64, 3)
    _, _, n, nv, _ = sizes(mc)
    nm = native.get_native_model(mx, torch.device("cuda", 0), F64)
    rw = (ctypes.c_int64 * 2)()
    assert nm.lib.mjh_model_kernel_io(nm.handle, 54, rw) == 0
    assert (rw[0], rw[1]) == ((2 * n * nv + nv * nv + 3 * n + nv) * 8, (n + 2 * nv + 2) * 8 + 4)
    nm.lib.mjh_debug_phase_timing(1)
    try:
        mt.solve_pgs(mx, d, iterations=3, force0=f0)
        ms, ids = (ctypes.c_float * 16)(), (ctypes.c_int * 16)()
        k = nm.lib.mjh_debug_phase_times(ms, ids, 16)
    finally:
        nm.lib.mjh_debug_phase_timing(0)
    assert [ids[i] for i in range(k)] == [54] and ms[0] > 0


def test_defaults_and_a_side_stream():
    """``iterations`` / ``tolerance`` default to the model's options; the call runs on the caller's stream; the input is not written."""
    mc, mx, d, A, f0 = passed("ant_frictionloss", F32, 3)
    before = {n: getattr(d, n).clone() for n in ("efc_J", "efc_D", "efc_aref", "efc_frictionloss", "qLD", "qacc_smooth", "efc_force", "qacc")}
    want = mt.solve_pgs(mx, d, iterations=int(mc.opt.iterations), tolerance=float(mc.opt.tolerance), force0=f0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = mt.solve_pgs(mx, d, force0=f0)
    s.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert all(torch.equal(getattr(d, n), t) for n, t in before.items())
