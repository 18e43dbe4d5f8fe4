"""What tests/test_constraint_shapes.py rests on, without a device: the family's sizes, the table's conditions from the library's own plans, and the three
longdouble references (tests/_efc_ref.py, _pgs_ref.py, _noslip_ref.py) on the synthetic leaves of tests/_efc_synth.py -- well conditioned (longdouble against
the same definitions in float64 within TOL_PRE[F64]), within the state cap on their own, and with the stated outcome on every PGS edge row."""
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

B, NPDT = sy.B, sy.NPDT
ALL = [c.name for c in sy.TABLE]
NOSLIP_CASES = sy.noslip_cases()
NOSLIP_IDS = [f"{n}-{'elliptic' if c else 'pyramidal'}" for n, c in NOSLIP_CASES]
MIXED = ("mixed12", "mixed12-f32")


def f64(x):
    return np.asarray(x, dtype=np.float64)


# ---- the family --------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ALL)
def test_the_family_has_the_sizes_of_the_table(name):
    c = sy.BY_NAME[name]
    m = c.model()
    nv, ne, nf, nl, ncon, nefc = sy.sizes(m)
    assert (nv, ne, nf, nl, ncon, nefc) == c.want and nv == sum(c.legs) and m.qpos0.dtype == c.dtype
    opts = dict(c.opts)
    assert ne == opts.get("neq", 0) and nf == opts.get("nfric", 0)
    assert nl == sum((n > 0) + (n > 6) for n in c.legs)  # links 0 and 6 of every leg are limited
    assert ncon == (2 * len(c.legs) if c.contacts else 0) and nefc == ne + nf + nl + 4 * ncon  # a capsule on a plane: two contacts of four pyramid edges
    if c.contacts:
        assert (np.asarray(m.tables.con_dim)[:ncon] == 3).all() and int(m.tables.con_efc_address[0]) == ne + nf + nl
    if c.elliptic:
        me = c.model(1)
        assert int(me.opt.cone) == 1 and sy.sizes(me) == (nv, ne, nf, nl, ncon, ne + nf + nl + 3 * ncon)


def test_the_knobs_of_the_family():
    """``limited=`` chooses the limited links; ``contacts=False`` leaves the limit rows; the generated text is deterministic and nothing is read from disk."""
    assert sy.sizes(sy.family([3, 3], limited=(0, 1, 2)))[3] == 6 and sy.sizes(sy.family([3, 3], limited=()))[3] == 0
    assert sy.sizes(sy.family([8, 8], contacts=False)) == (16, 0, 0, 4, 0, 4)
    assert sy.sizes(sy.family([8, 8])) == (16, 0, 0, 4, 4, 20)          # the three sizes the issue quotes
    assert sy.sizes(sy.family([2] * 15 + [1]))[::5] == (31, 144) and sy.sizes(sy.family([7] * 9))[::5] == (63, 90)
    assert sy.family_xml([2, 1], nfric=2, neq=1) == sy.family_xml([2, 1], nfric=2, neq=1) and 'jacobian="dense"' in sy.family_xml([1])
    m = sy.family([2, 2], nfric=3, neq=1, dtype=F32)
    assert sy.sizes(m) == (4, 1, 3, 2, 4, 22) and m.qpos0.dtype == F32


def test_the_table_meets_its_conditions():
    got = sy.table_conditions()
    assert len(got["second_buffer"]) >= 4


# ---- the synthetic leaves ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ("mixed12-f32", "nv65", "mixed33"))
def test_the_leaves_follow_the_recipe(name):
    m, d, A, q = sy.problem(name)
    nv, ne, nf, _, _, nefc = sy.sizes(m)
    dt = NPDT[sy.BY_NAME[name].dtype]
    for n in sy.SYNTH_LEAVES:
        assert A[n].dtype == dt and getattr(d, n).shape[0] == B and np.isfinite(A[n]).all(), n
    again = sy.arrays_of(m, sy.leaves(m, B, sy.BY_NAME[name].dtype, sy.BY_NAME[name].seed))
    assert all(np.array_equal(A[n], again[n]) for n in sy.SYNTH_LEAVES)  # seeded
    assert np.array_equal(A["qM"], A["qM"].transpose(0, 2, 1)) and not np.triu(A["qLD"], 1).any()
    L = er.ld(A["qLD"])
    assert rel_err(f64(np.einsum("bik,bjk->bij", L, L)), f64(A["qM"])) <= 4 * np.finfo(dt).eps
    assert np.linalg.cond(f64(A["qM"])).max() < 100
    assert (A["efc_D"] >= 0.5).all() and (A["efc_D"] <= 50).all()
    fl = A["efc_frictionloss"]
    assert not fl[:, :ne].any() and not fl[:, ne + nf:].any() and (fl[:, ne:ne + nf] >= dt(0.1)).all() and (fl[:, ne:ne + nf] <= 2).all()
    dead = ~A["efc_J"].any(-1)
    assert not dead[:, :ne + nf].any() and not A["efc_aref"][dead].any() and 0.1 < dead[:, ne + nf:].mean() < 0.4


# ---- the references on them -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ALL)
def test_the_constraint_space_reference_is_well_conditioned_and_within_the_state_cap(name):
    """Longdouble against plain float64 numpy of the same definitions within TOL_PRE[F64]; the rows ``comparable`` leaves out at the dtype's eps: at most 1 %."""
    m, _, A, q = sy.problem(name)
    dtype = sy.BY_NAME[name].dtype
    tol = TOL_PRE[F64]
    D = {n: f64(v) for n, v in A.items()}
    assert rel_err(np.einsum("bnv,bkv->bkn", D["efc_J"], f64(q["v"])), f64(er.mul_jac_vec(A["efc_J"], q["v"]))) <= tol
    assert rel_err(np.einsum("bnv,bkn->bkv", D["efc_J"], f64(q["f"])), f64(er.mul_jac_t_vec(A["efc_J"], q["f"]))) <= tol
    want = sy.ref_update(m, A, qacc=A["qacc"])
    jar = np.einsum("bnv,bv->bn", D["efc_J"], D["qacc"]) - D["efc_aref"]
    ms = np.einsum("bij,bj->bi", D["qM"], D["qacc"]) - D["qfrc_smooth"]
    assert rel_err(jar, f64(want["jar"])) <= tol and rel_err(ms - np.einsum("bnv,bn->bv", D["efc_J"], f64(want["efc_force"])), f64(want["grad"])) <= tol
    AR, b = er.efc_ar(A["efc_J"], A["efc_D"], A["efc_aref"], A["qLD"], A["qacc_smooth"])
    AR64, b64, _ = pr.dual(A["efc_J"], A["efc_D"], A["efc_aref"], A["qLD"], A["qacc_smooth"], np.float64)
    assert rel_err(AR64, f64(AR)) <= tol and rel_err(b64, f64(b)) <= tol
    eps = float(torch.finfo(dtype).eps)
    for keep in (sy.state_keep(m, A, eps, qacc=A["qacc"]), sy.state_keep(m, A, eps, jar=q["jar"])):
        assert 1 - keep.mean() <= sy.STATE_CAP, (name, int((~keep).sum()), keep.size)
    hist = np.bincount(want["efc_state"].reshape(-1), minlength=4) + np.bincount(sy.ref_update(m, A, jar=q["jar"])["efc_state"].reshape(-1), minlength=4)
    if sy.sizes(m)[5] >= 7:
        assert hist[er.QUADRATIC] > 0 and hist[er.SATISFIED] > 0, hist
    if sy.floss_of(m):
        assert hist[er.LINEAR_NEG] > 0 and hist[er.LINEAR_POS] > 0, hist


@pytest.mark.parametrize("warm", [False, True], ids=["cold", "force0"])
@pytest.mark.parametrize("name", ALL)
def test_the_pgs_reference_is_well_conditioned(name, warm):
    m, _, A, q = sy.problem(name)
    start = q["pgs0"] if warm else None
    ref, r64 = sy.ref_pgs(m, A, start), sy.ref_pgs(m, A, start, dtype=np.float64)
    for k in (0,) + sy.SWEEPS:
        want, other = sy.pgs_at(A, ref, k), sy.pgs_at(A, r64, k, np.float64)
        for n in ("efc_force", "qfrc_constraint", "qacc", "cost", "improvement"):
            assert rel_err(f64(other[n]), f64(want[n])) <= TOL_PRE[F64], (name, k, n)
    assert (ref["niter"] == max(sy.SWEEPS)).all()


@pytest.mark.parametrize("name,cone", NOSLIP_CASES, ids=NOSLIP_IDS)
def test_the_noslip_reference_is_well_conditioned(name, cone):
    m, _, A, _ = sy.problem(name, cone)
    start, mu, ref, _ = sy.noslip_refs(name, cone)
    r64 = sy.ref_noslip(m, A, start, mu, dtype=np.float64)
    assert ref["qcqp_converged"]
    for k in (0,) + sy.SWEEPS:
        niter = np.full(B, k)
        want, other = sy.noslip_at(A, ref, niter), sy.noslip_at(A, r64, niter, np.float64)
        for n in ("efc_force", "qfrc_constraint", "qacc", "cost", "improvement"):
            assert rel_err(f64(other[n]), f64(want[n])) <= TOL_PRE[F64], (name, cone, k, n)
    touched = sy.touched_rows(m)
    assert touched.any() and not touched.all() and np.array_equal(f64(ref["efc_force"])[:, ~touched], f64(start)[:, ~touched])
    assert (start[:, ~touched][:, sy.sizes(m)[1] + sy.sizes(m)[2]:] > 0).all()  # positive normals: the blocks are live


def test_the_noslip_inputs_exercise_the_reference():
    total = {0: np.zeros(5, dtype=int), 1: np.zeros(5, dtype=int)}
    for name, cone in NOSLIP_CASES:
        for k, s in sy.noslip_refs(name, cone)[2]["status"][0].items():
            if k != "fl":
                total[cone] += np.bincount(s, minlength=5)
    for cone in (0, 1):
        assert total[cone][nr.INTERIOR] >= 1 and total[cone][nr.BOUNDARY] >= 1, (cone, total[cone])


# ---- the value edges on the references ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", MIXED)
def test_the_zone_boundaries_by_the_definitions(name):
    """On the boundary and beyond it a row with a friction loss is linear, one step inside it is not; ``jar = +-0`` and anything positive are satisfied on an
    inequality row, anything negative -- the smallest subnormal included -- is quadratic; below ``ne + nf`` every row that is not linear is quadratic."""
    m, _, _, _ = sy.problem(name)
    _, ne, nf, _, _, nefc = sy.sizes(m)
    A, jar = sy.zone_edge_inputs(name)
    st = sy.ref_update(m, A, jar=jar)["efc_state"]
    fl, r = er.ld(A["efc_frictionloss"]), er.LD(0.25)
    j = er.ld(jar)
    row = np.broadcast_to(np.arange(nefc), st.shape)
    assert (A["efc_D"] == 4).all() and set(np.unique(fl[fl > 0]).tolist()) == {0.5, 3.0}
    has = fl > 0
    assert (st[has & (j <= -r * fl)] == er.LINEAR_NEG).all() and (st[has & (j >= r * fl)] == er.LINEAR_POS).all()
    inside = ~(has & ((j <= -r * fl) | (j >= r * fl)))
    assert (st[inside & (row < ne + nf)] == er.QUADRATIC).all()
    assert (st[inside & (row >= ne + nf) & (j < 0)] == er.QUADRATIC).all() and (st[inside & (row >= ne + nf) & ~(j < 0)] == er.SATISFIED).all()
    on = has & ((j == -r * fl) | (j == r * fl))
    step = has & ~on & (np.abs(np.abs(j) - r * fl) <= 2 * np.finfo(jar.dtype).eps * r * fl)
    assert on[:, ne:ne + nf].sum() == 4 and on[:, ne + nf:].sum() == 4 and step[:, ne:ne + nf].sum() == 8 and step[:, ne + nf:].sum() == 8
    zero = j == 0
    tiny = (j != 0) & (np.abs(j) <= np.finfo(jar.dtype).tiny)
    assert zero[:, :ne].sum() == 2 and zero[:, ne + nf:].sum() == 4 and np.signbit(jar[zero]).sum() == 3
    assert tiny[:, :ne].sum() == 4 and tiny[:, ne + nf:].sum() == 8 and (np.abs(jar[tiny]) < np.finfo(jar.dtype).tiny).sum() == 6  # (half of them subnormal)
    assert (np.bincount(st.reshape(-1), minlength=4) > 0).all()
    assert np.array_equal(f64(sy.ref_update(m, A, jar=jar)["efc_force"]), np.where(st == er.QUADRATIC, -4 * f64(jar), np.where(st == er.LINEAR_NEG, f64(fl), np.where(st == er.LINEAR_POS, -f64(fl), 0))))


@pytest.mark.parametrize("name", MIXED)
def test_the_pgs_edge_rows_on_the_reference(name):
    """The outcomes tests/test_constraint_shapes.py asserts on the device, on ``_pgs_ref`` in longdouble and in the dtype: a row with ``AR_ii <= 0`` is skipped (the
    reference's rule ``diag > 0``) and keeps its projected start; a ``J = 0`` row goes to ``project(-b / R)`` -- exactly so in the dtype, where ``D`` is a power of two:
    from the first sweep cold, from the second from ``force0``; with ``b = 0`` to an exact 0; a friction row with bound 0 is 0 after the projection and stays."""
    m, _, _, _ = sy.problem(name)
    dt = NPDT[sy.BY_NAME[name].dtype]
    _, ne, nf, _, _, nefc = sy.sizes(m)
    A, f0, rows = sy.pgs_edge_inputs(name)
    fl = A["efc_frictionloss"]
    assert not A["efc_J"][:, rows["skipped"] | rows["moves"] | rows["vanishes"]].any() and A["efc_J"][:, rows["bound0"]].any()
    assert (A["efc_D"][:, rows["skipped"]] <= 0).all() and (A["efc_D"][:, rows["skipped"]] < 0).any() and (A["efc_D"][:, rows["skipped"]] == 0).any()
    assert rows["skipped"][:ne].any() and rows["skipped"][ne:ne + nf].any() and rows["skipped"][ne + nf:].any()
    assert rows["moves"][:ne].any() and rows["moves"][ne:ne + nf].any() and rows["moves"][ne + nf:].any()
    AR, b, R = pr.dual(A["efc_J"], A["efc_D"], A["efc_aref"], A["qLD"], A["qacc_smooth"])
    diag = AR[:, np.arange(nefc), np.arange(nefc)]
    assert not diag[:, rows["skipped"]].any() and (diag[:, rows["moves"] | rows["vanishes"]] > 0).all() and not b[:, rows["vanishes"]].any() and b[:, rows["moves"]].all()
    target = pr.project(-b / np.where(R > 0, R, 1), er.ld(fl), ne, nf)
    for start in (None, f0):
        p0 = pr.project(np.zeros((B, nefc), dtype=dt) if start is None else start, fl, ne, nf)
        for dtype in (er.LD, dt):
            ref = sy.ref_pgs(m, A, start, dtype=dtype)
            for k in (0, 1, 3):
                f = f64(ref["forces"][k])
                assert np.array_equal(f[:, rows["skipped"]], p0[:, rows["skipped"]]) and not f[:, rows["bound0"]].any()
                if k == 0:
                    assert np.array_equal(f, p0)
                else:
                    assert not f[:, rows["vanishes"]].any()
                if dtype != er.LD and k >= (1 if start is None else 2):
                    assert np.array_equal(f[:, rows["moves"]], f64(target)[:, rows["moves"]])
                elif k:  # (from force0 the dtype's first sweep lands within a few roundings of |force0| + |target|)
                    assert rel_err(f[:, rows["moves"]], f64(target)[:, rows["moves"]]) <= (1e-15 if dtype == er.LD else 8 * np.finfo(dt).eps)
    assert p0[:, rows["vanishes"]].all() and p0[:, rows["skipped"]].any()
    edge = sy.on_bounds_start(m, A, sy.BY_NAME[name].dtype)
    assert np.array_equal(pr.project(edge, fl, ne, nf), edge)
    assert np.array_equal(f64(sy.ref_pgs(m, A, edge, sweeps=0)["efc_force"]), edge)


@pytest.mark.parametrize("name", ("mixed12", "mixed33"))
def test_efc_D_zero_by_the_definitions(name):
    """``efc_D == 0``: ``constraint_update`` takes ``r = 1 / mjMINVAL`` -- no ``jar`` of order one reaches ``r fl = 1e15 fl``, so the row is never linear and its force
    ``-D jar`` is 0 --, the dual side ``R = 0``."""
    m, _, _, q = sy.problem(name)
    A = sy.zero_d_inputs(name)
    z = A["efc_D"] == 0
    assert 0.3 < z.mean() < 0.36
    for u in (sy.ref_update(m, A, qacc=A["qacc"]), sy.ref_update(m, A, jar=q["jar"])):
        assert not f64(u["efc_force"])[z].any() and np.isin(u["efc_state"][z], (er.SATISFIED, er.QUADRATIC)).all() and np.isfinite(f64(u["cost"])).all()
    assert not f64(er.efc_R(A["efc_D"]))[z].any()
