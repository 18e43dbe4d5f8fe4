"""The constraint-space, PGS and no-slip kernels (csrc/mjh_efc.h, mjh_dual.h, mjh_pgs.h, mjh_noslip.h) off their models' shapes and values: the family and the synthetic
leaves of tests/_efc_synth.py against the longdouble references tests/_efc_ref.py, _pgs_ref.py and _noslip_ref.py on the SAME rounded inputs, B = 3.  No ``forward``
runs here: the kernels under test are the only device code.  tests/test_constraint_shapes_host.py pins the family's sizes, the table's conditions and the
references on these inputs without a device.

The table (``_efc_synth.TABLE``) walks the dof counts 1 .. 65 -- every ``P`` of ``efc_jt_accumulate`` with ``nv == P`` and ``nv < P``, the one-lane-per-dof path with
fewer dofs than lanes and at 64 and 65, where one lane makes the second trip of the ``k += 64`` loops -- and the row counts against the staging chunk: chunks of 66,
65, 63 and 62 rows, ``nefc`` an exact multiple of the chunk, a last chunk of one row, 1, 7, 8 and 9 rows around ``AR``'s 8 x 8 tile, and all four row classes
at once.  ``test_the_table_meets_its_conditions`` proves from the library's own plans that each of these is reached.

No bound is read off a kernel.  Values: ``TOL_PRE[dtype]`` by ``_util.rel_err`` (``grad_norm``: ``x sqrt(nv)``); ``AR``, ``solve_pgs`` and ``solve_noslip``:
``max(TOL_PRE, 4 x the error of the reference run in the dtype)``, the rule of tests/test_pgs.py; states: every row ``_efc_ref.comparable`` keeps, at most 1 % left
out -- and none at all in the zone-boundary test, whose inputs are exact in every precision.  Feasibility, untouched rows and the bit identities carry no tolerance.

Measured (one MI355X), worst error over bound per function, float64 / float32, and the case that gave it:
  mul_jac_vec, mul_jac_t_vec   8.7e-7 (nv33, J^T: 8.7e-16) / 1.4e-3 (nv33-f32, J^T: 2.7e-7)
  constraint_update            6.8e-7 (nv33, jar=: qfrc_constraint 6.8e-16) / 1.7e-3 (nv64-f32, qfrc_constraint 3.5e-7); no row's state left out in any case
  efc_ar: b                    6.1e-7 (nv64: 6.1e-16) / 1.2e-3 (nv64-f32: 2.3e-7)
  efc_ar: AR                   6.9e-7 (nv64, off the diagonal: 6.9e-16) / 2.0e-3 (nv65-f32-last-one, off the diagonal: 4.0e-7)
  solve_pgs                    1.0e-5 (nv5 cold, 3 sweeps, improvement: 1.0e-14) / 9.3e-3 (nv33-f32 force0, 3 sweeps, qfrc_constraint: 1.9e-6)
  solve_noslip                 0.67 (nv5 elliptic, 3 sweeps, improvement: the sweep starts at the fixed point, the exact figure is 3e-20 and
                               any float64 evaluation leaves a rounding residue -- 1.1e-9 of rel_err's floor here, 4.2e-10 from the float64 reference) / 2.0e-2 (nv65-f32-last-one pyramidal, 3 sweeps, improvement: 4.0e-6)
  cost(pgs) - cost(noslip)     6.2e-6 (nv33: 6.2e-15) / 1.7e-2 (nv33-f32: 3.4e-6), without a sweep; every other output of the two the same bits
The first no-slip sweep's blocks over the table [no normal force, inside, boundary, put back, degenerate]: pyramidal [0, 942, 913, 0, 125], elliptic
[0, 42, 129, 48, 183]; friction-loss rows [skipped, inside, on a bound] [0, 42, 30].  The zone-boundary test sees all four states on every model.
"""
import functools

import numpy as np
import pytest
import torch

import _efc_ref as er
import _efc_synth as sy
import _noslip_ref as nr
import _pgs_ref as pr
import mujoco_torch_amd as mt
from _cases import F32, F64, TOL_PRE
from _util import rel_err

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, K, SWEEPS, NPDT = sy.B, sy.K, sy.SWEEPS, sy.NPDT
NAMES = ("efc_force", "qfrc_constraint", "qacc", "cost", "improvement")
ALL = [c.name for c in sy.TABLE]
PGS_CASES = ALL
NOSLIP_CASES = sy.noslip_cases()
NOSLIP_IDS = [f"{n}-{'elliptic' if c else 'pyramidal'}" for n, c in NOSLIP_CASES]
MIXED = ("mixed12", "mixed12-f32")


def host(t):
    return t.detach().cpu().numpy()


def f64(x):
    return np.asarray(x, dtype=np.float64)


def dev(x, dtype):
    return torch.tensor(np.ascontiguousarray(x), dtype=dtype, device=DEV)


@functools.lru_cache(maxsize=None)
def placed(name, cone=0):
    """(host Model, device Model, device Data, host arrays, queries) of a table entry."""
    m, d, A, q = sy.problem(name, cone)
    return m, m.to(DEV), d.to(DEV), A, q


def check(what, got, want, tol, floor=None):
    e = rel_err(host(got) if isinstance(got, torch.Tensor) else got, f64(want), *(() if floor is None else (floor,)))
    print(f"  {what}: rel_err {e:.3g} ({e / tol:.2g} of {tol:g})")
    assert np.isfinite(e) and e <= tol, (what, e, tol)
    return e / tol


def against_same(what, got, want, same, tol):
    """``got`` against the longdouble ``want`` within max(tol, 4 x the error of ``same``, the reference run in the dtype)."""
    e_same, e_new = rel_err(f64(same), f64(want)), rel_err(host(got) if isinstance(got, torch.Tensor) else got, f64(want))
    bound = max(tol, 4 * e_same)
    print(f"  {what}: rel_err {e_new:.3g}, the reference in the dtype {e_same:.3g}, bound {bound:.3g} ({e_new / bound:.2g} of it)")
    assert np.isfinite(e_new) and e_new <= bound, (what, e_new, bound)
    return e_new / bound


# ---- the checks, on any (Model, Data, arrays) -------------------------------------------------------------------------------------------------------

def check_mul(mx, d, A, q, dtype):
    tol = TOL_PRE[dtype]
    return max(check("mul_jac_vec", mt.mul_jac_vec(mx, d, dev(q["v"], dtype)), er.mul_jac_vec(A["efc_J"], q["v"]), tol),
               check("mul_jac_t_vec", mt.mul_jac_t_vec(mx, d, dev(q["f"], dtype)), er.mul_jac_t_vec(A["efc_J"], q["f"]), tol))


def check_update(m, mx, d, A, q, dtype, cap=sy.STATE_CAP):
    """``constraint_update`` at the Data's ``qacc`` and at ``jar=``: values, ``grad_norm`` at ``TOL_PRE sqrt(nv)``, states on the comparable rows."""
    tol, eps, nv = TOL_PRE[dtype], float(torch.finfo(dtype).eps), int(m.nv)
    worst = 0.0
    u = mt.constraint_update(mx, d)
    want = sy.ref_update(m, A, qacc=A["qacc"])
    for n in ("jar", "efc_force", "qfrc_constraint", "gauss", "cost", "grad"):
        worst = max(worst, check(f"qacc: {n}", getattr(u, n), want[n], tol))
    worst = max(worst, check("qacc: grad_norm", u.grad_norm, want["grad_norm"], tol * np.sqrt(nv)))
    uj = mt.constraint_update(mx, d, jar=dev(q["jar"], dtype))
    wantj = sy.ref_update(m, A, jar=q["jar"])
    assert uj.gauss is None and uj.grad is None and uj.grad_norm is None
    for n in ("efc_force", "qfrc_constraint", "cost"):
        worst = max(worst, check(f"jar=: {n}", getattr(uj, n), wantj[n], tol))
    hist = np.zeros(4, dtype=np.int64)
    for what, got, ref, keep in (("qacc", u, want, sy.state_keep(m, A, eps, qacc=A["qacc"])), ("jar=", uj, wantj, sy.state_keep(m, A, eps, jar=q["jar"]))):
        out = 1 - keep.mean()
        h = np.bincount(ref["efc_state"].reshape(-1), minlength=4)
        hist += h
        print(f"  {what}: states (satisfied, quadratic, linear-neg, linear-pos) {h.tolist()}; {int((~keep).sum())} of {keep.size} rows left out ({out:.2%})")
        assert out <= cap and got.efc_state.dtype == torch.int32
        assert (host(got.efc_state) == ref["efc_state"])[keep].all(), what
    return worst, hist


def check_ar(mx, d, A, dtype):
    """``efc_ar``: ``b`` at TOL_PRE; ``AR``, whole and off the diagonal, at max(TOL_PRE, 4 x the error of ``_pgs_ref.dual`` in the dtype); symmetric bit for bit."""
    tol = TOL_PRE[dtype]
    dual = mt.efc_ar(mx, d)
    AR, b = er.efc_ar(A["efc_J"], A["efc_D"], A["efc_aref"], A["qLD"], A["qacc_smooth"])
    same = pr.dual(A["efc_J"], A["efc_D"], A["efc_aref"], A["qLD"], A["qacc_smooth"], NPDT[dtype])[0]
    worst = check("b", dual.b, b, tol)
    assert torch.equal(dual.AR, dual.AR.transpose(-1, -2).contiguous())
    worst = max(worst, against_same("AR", dual.AR, AR, same, tol))
    n = AR.shape[-1]
    if n > 1:
        off = ~np.eye(n, dtype=bool)
        worst = max(worst, against_same("AR off the diagonal", host(dual.AR)[:, off], AR[:, off], same[:, off], tol))
    return worst


def feasible(m, A, f):
    _, ne, nf, _, _, _ = sy.sizes(m)
    return bool((np.abs(f[:, ne:ne + nf]) <= A["efc_frictionloss"][:, ne:ne + nf]).all() and (f[:, ne + nf:] >= 0).all() and np.isfinite(f).all())


def check_pgs(m, mx, d, A, dtype, start, refs, sweeps=SWEEPS):
    """``solve_pgs`` at ``tolerance=0`` after each of ``sweeps``, from ``start`` (None: cold): the five outputs at max(TOL_PRE, 4 x the same-dtype reference's
    error); exact feasibility; ``niter == iterations``."""
    ref, same = refs
    worst = 0.0
    for k in sweeps:
        res = mt.solve_pgs(mx, d, iterations=k, tolerance=0.0, force0=None if start is None else dev(start, dtype))
        assert (res.niter == k).all() and res.niter.dtype == torch.int32
        assert feasible(m, A, host(res.efc_force))
        want, other = sy.pgs_at(A, ref, k), sy.pgs_at(A, same, k, NPDT[dtype])
        for n in NAMES:
            worst = max(worst, against_same(f"{k} sweeps: {n}", getattr(res, n), want[n], other[n], TOL_PRE[dtype]))
    return worst


def with_friction(d, mu, dtype):
    return d.replace(contact=d.contact.replace(friction=dev(mu, dtype).reshape(d.contact.friction.shape)))


def check_noslip(m, mx, d, A, dtype, start, mu, refs, sweeps=SWEEPS):
    """``solve_noslip`` at ``tolerance=0`` after each of ``sweeps``: tests/test_noslip.py's tolerance rule and per-environment ``niter``; rows that are not friction
    dimensions come back bit for bit; friction-loss rows within their bounds, pyramid edges ``>= 0``."""
    ref, same = refs
    assert ref["qcqp_converged"]
    _, ne, nf, _, _, _ = sy.sizes(m)
    touched = sy.touched_rows(m)
    d = with_friction(d, mu, dtype)
    worst = 0.0
    for k in sweeps:
        res = mt.solve_noslip(mx, d, iterations=k, tolerance=0.0, force0=dev(start, dtype))
        niter, f = host(res.niter), host(res.efc_force)
        assert res.niter.dtype == torch.int32 and (niter >= 1).all() and ((niter == k) | ((niter < k) & (host(res.improvement) < 0))).all()
        assert np.isfinite(f).all() and np.array_equal(f[:, ~touched], start[:, ~touched])
        assert (np.abs(f[:, ne:ne + nf]) <= A["efc_frictionloss"][:, ne:ne + nf]).all()
        if int(m.opt.cone) == 0:
            assert (f[:, ne + nf:] >= 0).all()
        want, other = sy.noslip_at(A, ref, niter), sy.noslip_at(A, same, niter, NPDT[dtype])
        for n in NAMES:
            worst = max(worst, against_same(f"{k} sweeps: {n}", getattr(res, n), want[n], other[n], TOL_PRE[dtype]))
    return worst


# ---- the table -----------------------------------------------------------------------------------------------------------------------------------

def test_the_table_meets_its_conditions():
    """Sizes, staged rows and ``efc_ar``'s second buffer of every entry, from ``constraint_space.plan``, ``pgs.plan`` and ``noslip.plan``: the conditions are
    ``_efc_synth.table_conditions``'s asserts (the host test runs the same)."""
    got = sy.table_conditions()
    print(f"efc_ar stages a second buffer on {len(got['second_buffer'])} entries: {got['second_buffer']}")
    for name, st in got["staged"].items():
        print(f"  {name}: {sy.BY_NAME[name].want}, staged {st}")


# ---- the shape sweep -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ALL)
def test_constraint_space_against_the_reference(name):
    m, mx, d, A, q = placed(name)
    dtype = sy.BY_NAME[name].dtype
    print(f"{name} {dtype}: (nv, ne, nf, nl, ncon, nefc) {sy.sizes(m)}")
    w1 = check_mul(mx, d, A, q, dtype)
    w2, hist = check_update(m, mx, d, A, q, dtype)
    w3 = check_ar(mx, d, A, dtype)
    if sy.sizes(m)[5] >= 7:
        assert hist[er.QUADRATIC] > 0 and hist[er.SATISFIED] > 0, hist
    if sy.floss_of(m):
        assert hist[er.LINEAR_NEG] > 0 and hist[er.LINEAR_POS] > 0, hist
    print(f"  worst error / bound: mul {w1:.3g}, constraint_update {w2:.3g}, efc_ar {w3:.3g}")


@pytest.mark.parametrize("warm", [False, True], ids=["cold", "force0"])
@pytest.mark.parametrize("name", PGS_CASES)
def test_pgs_against_the_reference(name, warm):
    m, mx, d, A, q = placed(name)
    dtype = sy.BY_NAME[name].dtype
    start = q["pgs0"] if warm else None
    if warm:
        assert not feasible(m, A, start)  # (negative on unilateral rows, past the bounds on friction rows)
    print(f"{name} {dtype} {'force0' if warm else 'cold'}: (nv, ne, nf, nl, ncon, nefc) {sy.sizes(m)}")
    w = check_pgs(m, mx, d, A, dtype, start, sy.pgs_refs(name, warm))
    print(f"  worst error / bound {w:.3g}")


@pytest.mark.parametrize("name,cone", NOSLIP_CASES, ids=NOSLIP_IDS)
def test_noslip_against_the_reference(name, cone):
    m, mx, d, A, _ = placed(name, cone)
    dtype = sy.BY_NAME[name].dtype
    start, mu, ref, same = sy.noslip_refs(name, cone)
    print(f"{name} {dtype} {'elliptic' if cone else 'pyramidal'}: (nv, ne, nf, nl, ncon, nefc) {sy.sizes(m)}")
    w = check_noslip(m, mx, d, A, dtype, start, mu, (ref, same))
    print(f"  worst error / bound {w:.3g}")


def test_the_noslip_inputs_exercise_the_code():
    """Counted with the reference on the first sweep, over the table: per cone type at least one block ends strictly inside its cone and one on the boundary;
    friction-loss rows end inside and on their bounds."""
    total = {0: np.zeros(5, dtype=int), 1: np.zeros(5, dtype=int)}
    fl = np.zeros(3, dtype=int)
    for name, cone in NOSLIP_CASES:
        ref = sy.noslip_refs(name, cone)[2]
        for k, s in ref["status"][0].items():
            if k == "fl":
                fl += np.bincount(s.ravel(), minlength=3)
            else:
                total[cone] += np.bincount(s, minlength=5)
    print(f"first sweep [no normal force, inside, boundary, put back, degenerate]: pyramidal {total[0].tolist()}, elliptic {total[1].tolist()}; "
          f"friction-loss rows [skipped, inside, on a bound] {fl.tolist()}")
    for cone in (0, 1):
        assert total[cone][nr.INTERIOR] >= 1 and total[cone][nr.BOUNDARY] >= 1, (cone, total[cone])
    assert fl[nr.INTERIOR] >= 1 and fl[nr.BOUNDARY] >= 1


# ---- bit identities ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sy.BIT_CASES)
def test_vectors_and_environments_are_independent(name):
    """Column j of a K-vector call is the single-vector call; environment 1 alone is row 1 of the batch, for every function."""
    m, mx, d, A, q = placed(name)
    dtype = sy.BY_NAME[name].dtype
    v, f, jar, f0 = (dev(q[n], dtype) for n in ("v", "f", "jar", "pgs0"))
    many = mt.mul_jac_vec(mx, d, v), mt.mul_jac_t_vec(mx, d, f)
    for j in range(K):
        assert torch.equal(many[0][:, j], mt.mul_jac_vec(mx, d, v[:, j].contiguous()))
        assert torch.equal(many[1][:, j], mt.mul_jac_t_vec(mx, d, f[:, j].contiguous()))
    start, mu = sy.noslip_start(m, dtype), sy.noslip_friction(m, dtype)
    dn, s0 = with_friction(d, mu, dtype), dev(start, dtype)

    def everything(dd, e):
        out = [mt.mul_jac_vec(mx, dd, v[e]), mt.mul_jac_t_vec(mx, dd, f[e])]
        out += [t for t in mt.constraint_update(mx, dd) if t is not None] + [t for t in mt.constraint_update(mx, dd, jar=jar[e]) if t is not None]
        out += list(mt.efc_ar(mx, dd)) + list(mt.solve_pgs(mx, dd, iterations=3, tolerance=0.0, force0=f0[e]))
        return out

    one = everything(d[1:2], slice(1, 2)) + list(mt.solve_noslip(mx, dn[1:2], iterations=3, tolerance=0.0, force0=s0[1:2]))
    whole = everything(d, slice(None)) + list(mt.solve_noslip(mx, dn, iterations=3, tolerance=0.0, force0=s0))
    assert len(one) == len(whole) == 2 + 8 + 5 + 2 + 6 + 6
    for i, (a, b) in enumerate(zip(one, whole)):
        assert torch.equal(a, b[1:2]), i


@pytest.mark.parametrize("name", ("nv5", "nv33", "nv33-f32", "nv65-f32-last-one"))
def test_the_two_solvers_share_their_staging_and_ending(name):
    """Without a sweep, from one feasible ``force0`` (the table's random start, projected by ``_pgs_ref.project``: ``solve_pgs`` projects it onto itself),
    ``solve_pgs`` and ``solve_noslip`` run csrc/mjh_dual.h's staging and ending alone: ``efc_force``, ``qfrc_constraint`` and ``qacc`` come back with the same bits,
    ``qfrc_constraint`` with the bits of ``mul_jac_t_vec(force0)`` as well (``efc_jt_accumulate`` over the same chunks), and the costs differ by the regulariser's
    ``1/2 sum_i R_i f_i^2`` at TOL_PRE.  The entries: both paths of ``efc_jt_accumulate`` (5 and 33 / 65 dofs), three staging chunks and a last chunk of one row."""
    m, mx, d, A, q = placed(name)
    dtype = sy.BY_NAME[name].dtype
    _, ne, nf, _, _, _ = sy.sizes(m)
    f = pr.project(q["pgs0"], A["efc_frictionloss"], ne, nf)
    assert feasible(m, A, f) and not np.array_equal(f, q["pgs0"]) and f.any()
    f0 = dev(f, dtype)
    p, n = mt.solve_pgs(mx, d, iterations=0, force0=f0), mt.solve_noslip(mx, d, iterations=0, force0=f0)
    assert not p.niter.any() and not n.niter.any() and not p.improvement.any() and not n.improvement.any()
    assert np.array_equal(host(p.efc_force), f)
    for what in ("efc_force", "qfrc_constraint", "qacc"):
        assert torch.equal(getattr(p, what), getattr(n, what)), what
    assert torch.equal(p.qfrc_constraint, mt.mul_jac_t_vec(mx, d, f0))
    R = np.where(A["efc_D"] > 0, 1 / np.where(A["efc_D"] > 0, er.ld(A["efc_D"]), 1), 0)
    check("cost(pgs) - cost(noslip)", f64(host(p.cost)) - f64(host(n.cost)), (R * er.ld(f) ** 2).sum(-1) / 2, TOL_PRE[dtype])


# ---- the value edges -------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", MIXED)
def test_zone_boundaries_with_no_row_left_out(name):
    """``constraint_update(jar=...)`` with ``jar`` exactly on, and one step to each side of, ``+- r fl`` (``efc_D = 4``, ``fl`` in {0.5, 3}: exact in every
    precision) and 0 (+-0, +-the smallest subnormal, +-the smallest normal), on friction rows and later rows, rows below ``ne + nf`` and inequality rows: states and
    forces equal ``_efc_ref`` on EVERY row; the cost at TOL_PRE."""
    m, mx, d, _, _ = placed(name)
    dtype = sy.BY_NAME[name].dtype
    A, jar = sy.zone_edge_inputs(name)
    dd = sy.with_arrays(sy.problem(name)[1], A).to(DEV)
    u = mt.constraint_update(mx, dd, jar=dev(jar, dtype))
    want = sy.ref_update(m, A, jar=jar)
    hist = np.bincount(want["efc_state"].reshape(-1), minlength=4)
    print(f"{name}: states (satisfied, quadratic, linear-neg, linear-pos) {hist.tolist()}")
    assert (hist > 0).all()
    bad = np.argwhere(host(u.efc_state) != want["efc_state"])
    assert not len(bad), [(int(e), int(i), float(jar[e, i]), float(A["efc_frictionloss"][e, i]), int(host(u.efc_state)[e, i]), int(want["efc_state"][e, i])) for e, i in bad]
    assert np.array_equal(host(u.efc_force), f64(want["efc_force"]))  # (-4 jar and +- fl: no rounding in any precision)
    check("cost", u.cost, want["cost"], TOL_PRE[dtype])
    check("qfrc_constraint", u.qfrc_constraint, want["qfrc_constraint"], TOL_PRE[dtype])


@pytest.mark.parametrize("name,cone", [("mixed12", 0), ("mixed12-f32", 0), ("mixed33", 0), ("mixed33", 1)], ids=["mixed12", "mixed12-f32", "mixed33", "mixed33-elliptic"])
def test_rows_with_efc_D_zero(name, cone):
    """``efc_D == 0`` on every third row, with ``fl > 0`` and ``fl == 0``: ``constraint_update`` takes ``r = 1 / mjMINVAL`` (both forms), ``efc_ar``, ``solve_pgs`` and
    ``solve_noslip`` take ``R = 0``; everything against the references by the rules of the sweep."""
    m, mx, _, _, q = placed(name, cone)
    dtype = sy.BY_NAME[name].dtype
    A = sy.zero_d_inputs(name, cone)
    _, ne, nf, _, _, _ = sy.sizes(m)
    z = A["efc_D"] == 0
    assert z[:, :ne].any() and z[:, ne:ne + nf].any() and z[:, ne + nf:].any() and (A["efc_frictionloss"][z] > 0).any() and (A["efc_frictionloss"][z] == 0).any()
    dd = sy.with_arrays(sy.problem(name, cone)[1], A).to(DEV)
    if not cone:
        check_update(m, mx, dd, A, q, dtype)
        check_ar(mx, dd, A, dtype)
        for start in (None, q["pgs0"]):
            check_pgs(m, mx, dd, A, dtype, start, (sy.ref_pgs(m, A, start), sy.ref_pgs(m, A, start, dtype=NPDT[dtype])))
    start, mu = sy.noslip_start(m, dtype), sy.noslip_friction(m, dtype)
    check_noslip(m, mx, dd, A, dtype, start, mu, (sy.ref_noslip(m, A, start, mu), sy.ref_noslip(m, A, start, mu, dtype=NPDT[dtype])))


@pytest.mark.parametrize("name", ("nv8", "nv8-f32", "nv33"))
def test_a_frictionloss_leaf_without_friction_rows_is_not_read(name):
    """``nfric = 0``: ``floss`` is false and there are no friction rows, so a random positive ``efc_frictionloss`` leaf gives the bits of a zeroed one."""
    m, mx, d, A, q = placed(name)
    dtype = sy.BY_NAME[name].dtype
    assert sy.sizes(m)[2] == 0 and not sy.floss_of(m) and not A["efc_frictionloss"].any()
    loud = d.replace(efc_frictionloss=dev(np.random.RandomState(3).uniform(0.1, 2.0, A["efc_frictionloss"].shape), dtype))
    jar, f0 = dev(q["jar"], dtype), dev(q["pgs0"], dtype)
    s0 = dev(sy.noslip_start(m, dtype), dtype)

    def everything(dd):
        out = [t for t in mt.constraint_update(mx, dd) if t is not None] + [t for t in mt.constraint_update(mx, dd, jar=jar) if t is not None]
        return out + list(mt.solve_pgs(mx, dd, iterations=3, tolerance=0.0, force0=f0)) + list(mt.solve_noslip(mx, dd, iterations=3, tolerance=0.0, force0=s0))

    a, b = everything(d), everything(loud)
    assert len(a) == len(b) == 8 + 5 + 6 + 6
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), i


@pytest.mark.parametrize("name", MIXED)
def test_pgs_edge_rows(name):
    """The row classes of ``_efc_synth.pgs_edge_inputs`` after 0, 1 and 3 sweeps, cold and from ``force0``: everything against ``_pgs_ref`` by the rule of the sweep,
    and the exact outcomes -- a row with ``AR_ii = 0`` keeps its projected start bit for bit; a ``J = 0`` row with ``aref != 0`` sits on ``project(-b / R)`` (cold: from
    the first sweep; from ``force0``: from the second -- ``pgs_edge_inputs`` says why); a ``J = 0``, ``b = 0`` row is an exact 0 after the first sweep; a friction row
    with bound 0 is an exact 0 always; a ``force0`` on its bounds comes back from ``iterations=0`` unchanged."""
    m, mx, _, _, _ = placed(name)
    dtype = sy.BY_NAME[name].dtype
    dt = NPDT[dtype]
    A, f0, rows = sy.pgs_edge_inputs(name)
    _, ne, nf, _, _, nefc = sy.sizes(m)
    dd = sy.with_arrays(sy.problem(name)[1], A).to(DEV)
    fl = A["efc_frictionloss"]
    R = np.where(A["efc_D"] > 0, dt(1) / np.where(A["efc_D"] > 0, A["efc_D"], dt(1)), dt(0))
    target = pr.project((A["efc_aref"] / np.where(R > 0, R, dt(1))).astype(dt), fl, ne, nf)  # -b / R = aref / R: exact, D is a power of two there
    for start in (None, f0):
        refs = sy.ref_pgs(m, A, start), sy.ref_pgs(m, A, start, dtype=dt)
        check_pgs(m, mx, dd, A, dtype, start, refs, sweeps=(0, 1, 3))
        p0 = pr.project(np.zeros((B, nefc), dtype=dt) if start is None else start, fl, ne, nf)
        for k in (0, 1, 3):
            f = host(mt.solve_pgs(mx, dd, iterations=k, tolerance=0.0, force0=None if start is None else dev(start, dtype)).efc_force)
            assert np.array_equal(f[:, rows["skipped"]], p0[:, rows["skipped"]]), k
            assert not f[:, rows["bound0"]].any(), k
            if k == 0:
                assert np.array_equal(f, p0)
                assert start is None or p0[:, rows["vanishes"]].all()  # (the start is not zero there)
            else:
                assert not f[:, rows["vanishes"]].any(), k
            if k >= (1 if start is None else 2):
                assert np.array_equal(f[:, rows["moves"]], target[:, rows["moves"]]), k
            for want in (refs[0]["forces"][k],):  # the reference agrees with every exact outcome (pinned on the host as well)
                assert np.array_equal(f64(want)[:, rows["skipped"]], p0[:, rows["skipped"]]) and not f64(want)[:, rows["bound0"]].any()
    mv = target[:, rows["moves"]]
    assert (mv != 0).any() and (mv == 0).any() and (np.abs(mv[:, 1]) == fl[:, rows["moves"]][:, 1]).any()  # (free, clamped to a bound, clamped to 0)
    edge = sy.on_bounds_start(m, A, dtype)
    res = mt.solve_pgs(mx, dd, iterations=0, force0=dev(edge, dtype))
    assert np.array_equal(host(res.efc_force), edge) and not res.niter.any() and not res.improvement.any()
    assert (np.abs(edge[:, ne:ne + nf]) == fl[:, ne:ne + nf]).all() and (edge[:, ne + nf::2] == 0).all()
