"""The constraint-space functions without a GPU: the tests' numpy longdouble reference (tests/_efc_ref.py, the yardstick of tests/test_constraint_space.py) pinned on the
recorded solver outputs of the goldens and on a factorisation of its own, and the public functions with the launch replaced by that reference.

Measured here (printed by the tests), worst over every environment and step of a case.  ``constraint_update`` of the recorded ``qacc`` against the recorded
leaves: |difference| of efc_force 1.5e-14 on forces of 32 (humanoid CG), 5.4e-12 on 5.9e3 (humanoid Newton), 6.8e-12 on 8.8e4 (ant frictionloss, Newton and CG),
5.8e-12 on 3.7e3 (equality loops); of qfrc_constraint 8.4e-12 at worst; by ``_util.rel_err`` 2.4e-14 / 5.7e-14 at worst, against a bound of 1e-8.  ``AR`` against
``J M^-1 J^T`` by a longdouble factorisation of the recorded ``qM``: 2.8e-15 of the largest entry at worst, at most 1.1 % of the bound ``10 nv eps cond(M)``
(cond(M) 4.5e3 on the humanoid, 1.1 on the ant).  The dual identity: 1.2e-14 of the largest |jar| at worst.  State decisions: no row of any case is left out,
at float64 and at float32 roundoff.
"""
import ctypes
import functools
import re

import numpy as np
import pytest
import torch

import _efc_ref as er
import _hostsim
import mujoco_torch_amd as mt
from _cases import F32, F64, TOL_PRE, TOL_SOL, seeded_batch
from _util import Golden, rel_err
from mujoco_torch_amd import constraint_space as cs
from mujoco_torch_amd import native
from test_abi import header_fields

LD = er.LD
CASES = ["humanoid_cg_f64", "humanoid_newton_f64", "ant_frictionloss_newton_f64", "ant_frictionloss_cg_f64", "equality_loops_f64"]
LEAVES = ("efc_J", "efc_D", "efc_aref", "efc_frictionloss", "efc_force", "qfrc_constraint", "qacc", "qM", "qLD", "qfrc_smooth", "qacc_smooth")
STATE_CAP = 0.01  # share of rows whose state may be left out of a comparison, per case


def sizes(m):
    """(ne + nf, frictionloss zones on?, nefc, nv, meaninertia * max(1, nv)) of a model."""
    ne, nf, _, _, nefc = m.constraint_sizes_py
    floss = nf > 0 and not (int(m.opt.disableflags) & mt.DisableBit.FRICTIONLOSS)
    return int(ne + nf), bool(floss), int(nefc), int(m.nv), float(m.stat.meaninertia) * max(1, int(m.nv))


@functools.lru_cache(maxsize=None)
def recorded(case):
    """(model, {leaf: [environments * steps, ...]}) of a recording."""
    g = Golden(case)
    _, _, nefc, nv, _ = sizes(g.model)
    tail = dict(efc_J=(nefc, nv), qM=(nv, nv), qLD=(nv, nv))
    rec = {n: np.stack([g.expected(e, s, n).reshape(tail.get(n, (-1,))) for e in range(g.nenv) for s in range(g.nsteps)]) for n in LEAVES}
    return g.model, rec


def update_of(m, r, **kw):
    ne_nf, floss, _, _, scale = sizes(m)
    return er.constraint_update(r["efc_J"], r["efc_D"], r["efc_aref"], r["efc_frictionloss"], ne_nf, floss, qM=r["qM"], qfrc_smooth=r["qfrc_smooth"],
                                qacc_smooth=r["qacc_smooth"], inertia_scale=scale, **kw)


# ---- 1. the reference on the recordings -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES)
def test_the_reference_reproduces_the_recorded_forces(case):
    """``constraint_update`` of the recorded ``qacc`` gives the recorded ``efc_force`` and ``qfrc_constraint`` at TOL_SOL[float64] by ``_util.rel_err``, per
    environment and step."""
    m, r = recorded(case)
    got = update_of(m, r, qacc=r["qacc"])
    N = len(r["qacc"])
    worst = {n: max(rel_err(got[n][i], r[n][i]) for i in range(N)) for n in ("efc_force", "qfrc_constraint")}
    absolute = {n: float(np.abs(got[n] - r[n]).max()) for n in ("efc_force", "qfrc_constraint")}
    print(f"{case}: {N} environment-steps, worst rel_err {worst}, worst |difference| {absolute}, largest |efc_force| {np.abs(r['efc_force']).max():.3g}")
    assert N >= 2 and np.abs(r["efc_force"]).max() > 0
    assert worst["efc_force"] <= TOL_SOL[F64] and worst["qfrc_constraint"] <= TOL_SOL[F64], worst


def test_the_recordings_cover_equality_and_friction_rows():
    assert sizes(recorded("equality_loops_f64")[0])[0] > 0 and not sizes(recorded("equality_loops_f64")[0])[1]
    m, r = recorded("ant_frictionloss_newton_f64")
    ne_nf, floss, _, _, _ = sizes(m)
    assert floss and ne_nf > 0 and (r["efc_frictionloss"][:, :ne_nf] > 0).all() and not r["efc_frictionloss"][:, ne_nf:].any()
    states = update_of(m, r, qacc=r["qacc"])["efc_state"]
    assert {er.QUADRATIC, er.SATISFIED} <= set(np.unique(states).tolist())


# ---- 2. AR and b on something independent ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES)
def test_ar_agrees_with_a_factorisation_of_the_recorded_mass_matrix(case):
    """``AR - diag(R) = J X`` with ``X = M^-1 J^T`` from a longdouble Cholesky factorisation of the recorded ``qM`` -- not of ``qLD``, the float64 factor the
    reference made of it (of ``qM + 1e-10 I`` for more than 16 dofs, math.py:108-113: the same regularisation is applied here).  The recorded factor
    carries the rounding of a float64 factorisation, which a solve amplifies by cond(M): the bound is 10 nv eps cond(M) relative to the largest entry."""
    m, r = recorded(case)
    _, _, nefc, nv, _ = sizes(m)
    AR, b = er.efc_ar(r["efc_J"], r["efc_D"], r["efc_aref"], r["qLD"], r["qacc_smooth"])
    assert (AR == AR.transpose(0, 2, 1)).all()
    M = er.ld(r["qM"]) + (LD(1e-10) * np.eye(nv, dtype=LD) if nv > 16 else 0)
    X = er.cholesky_solve(M, r["efc_J"])  # rows M^-1 J_r^T
    want = np.einsum("bik,bjk->bij", er.ld(r["efc_J"]), X)
    R = er.efc_R(r["efc_D"])
    got = AR - R[:, :, None] * np.eye(nefc, dtype=LD)
    cond = max(float(np.linalg.cond(np.asarray(Mi, dtype=np.float64))) for Mi in M)
    bound = 10 * nv * np.finfo(np.float64).eps * cond
    err = float(np.abs(got - want).max() / np.abs(want).max())
    print(f"{case}: cond(M) {cond:.3g}, |AR - diag R - J M^-1 J^T| / max {err:.3g}, bound {bound:.3g} ({err / bound:.2g} of it)")
    assert err <= bound
    assert float(np.abs(b - (np.einsum('bnv,bv->bn', er.ld(r['efc_J']), er.ld(r['qacc_smooth'])) - r['efc_aref'])).max()) == 0


@pytest.mark.parametrize("case", CASES)
def test_the_dual_identity_holds_whatever_the_convergence(case):
    """``jar - ((AR - diag R) f + b) = J M^-1 grad`` for the recorded ``qacc`` (f = efc_force): algebra, so it holds to rounding -- TOL_PRE[float64] relative
    to the largest |jar| -- whether or not the solver had converged.  The M of the identity is the matrix ``qLD`` factors, through which ``AR`` and
    ``qacc_smooth`` are made: ``qM + 1e-10 I`` for more than 16 dofs (math.py:108-113), so there ``grad`` takes the term ``1e-10 qacc`` that
    ``(M + 1e-10 I) qacc`` has over ``qM qacc`` (without it the two sides differ by ``1e-10 J M^-1 qacc``: 4.8e-9 on the humanoid)."""
    m, r = recorded(case)
    _, _, nefc, nv, _ = sizes(m)
    u = update_of(m, r, qacc=r["qacc"])
    AR, b = er.efc_ar(r["efc_J"], r["efc_D"], r["efc_aref"], r["qLD"], r["qacc_smooth"])
    A0 = AR - er.efc_R(r["efc_D"])[:, :, None] * np.eye(nefc, dtype=LD)
    lhs = u["jar"] - (np.einsum("bij,bj->bi", A0, u["efc_force"]) + b)
    grad = u["grad"] + (LD(1e-10) * er.ld(r["qacc"]) if nv > 16 else 0)
    W = er.forward_substitute(r["qLD"], r["efc_J"])
    wg = er.forward_substitute(r["qLD"], grad[:, None, :])[:, 0]
    rhs = np.einsum("bnk,bk->bn", W, wg)
    err = float(np.abs(lhs - rhs).max() / max(float(np.abs(u["jar"]).max()), 1e-6))
    print(f"{case}: worst grad_norm {float(u['grad_norm'].max()):.3g}, |lhs - rhs| / max|jar| {err:.3g}")
    assert err <= TOL_PRE[F64]


# ---- 3. state decisions -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES)
def test_states_are_decided_away_from_the_zone_boundaries(case):
    """``efc_state`` is compared only on rows whose ``jar`` lies further from every zone boundary than the propagated rounding bound of ``jar``
    (``_efc_ref.state_margin``).  On the recordings, at float64 and at float32 roundoff, the rows left out stay under 1 % -- the reference alone; and the states
    of the rows kept do not change when ``jar`` moves by that bound either way."""
    m, r = recorded(case)
    ne_nf, floss, _, _, _ = sizes(m)
    u = update_of(m, r, qacc=r["qacc"])
    for eps in (np.finfo(np.float64).eps, np.finfo(np.float32).eps):
        dist, bound = er.state_margin(r["efc_J"], r["qacc"], r["efc_aref"], r["efc_D"], r["efc_frictionloss"], ne_nf, floss, eps)
        keep = er.comparable(dist, bound)
        out = 1 - keep.mean()
        print(f"{case}: eps {eps:.1e}: {int((~keep).sum())} of {keep.size} rows left out ({out:.2%})")
        assert out <= STATE_CAP
        for sign in (-1, 1):
            moved = er.constraint_update(r["efc_J"], r["efc_D"], r["efc_aref"], r["efc_frictionloss"], ne_nf, floss, jar=u["jar"] + sign * bound)["efc_state"]
            assert (moved == u["efc_state"])[keep].all()


# ---- 4. the public functions on a stand-in --------------------------------------------------------------------------------------------------------

class StandIn:
    """``mjh_constraint_space`` of the CPU stand-in library: the numpy reference on the host pointers it is handed."""

    def __init__(self):
        self.calls = []

    def install(self, monkeypatch):
        _hostsim.install(monkeypatch)
        monkeypatch.setattr(_hostsim._Lib, "mjh_constraint_space", self, raising=False)
        return self

    def __get__(self, lib, owner=None):
        return lambda *args: self.run(lib, *args)

    def run(self, lib, handle, args, stream):
        a = args._obj
        nv, n, B = int(lib.o.desc.nv), int(lib.o.desc.nefc), int(a.B)
        ct, dt = (ctypes.c_double, np.float64) if lib.o.dt == 0 else (ctypes.c_float, np.float32)
        view = lambda p, count, c=ct: np.ctypeslib.as_array((c * count).from_address(p))
        leaf = lambda name, *shape: view(getattr(a, name), B * int(np.prod(shape))).reshape((B,) + shape)
        put = lambda name, value, c=ct, t=dt: view(getattr(a, name), value.size, c).__setitem__(slice(None), np.asarray(value, dtype=t).reshape(-1))
        self.calls.append(dict(op=int(a.op), B=B, K=int(a.K), ne_nf=int(a.ne_nf), floss=int(a.floss), vec_env=int(a.vec_env), vec_k=int(a.vec_k),
                               with_qacc=bool(a.qacc), with_jar=bool(a.jar_in)))
        if a.op in (cs.MUL_J, cs.MUL_JT):
            w, K = (nv, n)[a.op], int(a.K)
            span = (B - 1) * a.vec_env + (K - 1) * a.vec_k + w
            idx = np.arange(B)[:, None, None] * a.vec_env + np.arange(K)[None, :, None] * a.vec_k + np.arange(w)
            vec = view(a.vec, span)[idx]
            put("out", (er.mul_jac_vec if a.op == cs.MUL_J else er.mul_jac_t_vec)(leaf("efc_J", n, nv), vec))
        elif a.op == cs.UPDATE:
            kw = dict(qacc=leaf("qacc", nv), qM=leaf("qM", nv, nv), qfrc_smooth=leaf("qfrc_smooth", nv), qacc_smooth=leaf("qacc_smooth", nv),
                      inertia_scale=a.meaninertia * max(1, nv)) if a.qacc else dict(jar=leaf("jar_in", n))
            u = er.constraint_update(leaf("efc_J", n, nv), leaf("efc_D", n), leaf("efc_aref", n) if a.qacc else None, leaf("efc_frictionloss", n), int(a.ne_nf),
                                     bool(a.floss), **kw)
            for name in ("efc_force", "qfrc_constraint", "cost") + (("jar", "gauss", "grad", "grad_norm") if a.qacc else ()):
                put(name, u[name])
            put("efc_state", u["efc_state"], ctypes.c_int32, np.int32)
        else:
            AR, b = er.efc_ar(leaf("efc_J", n, nv), leaf("efc_D", n), leaf("efc_aref", n), leaf("qLD", nv, nv), leaf("qacc_smooth", nv))
            put("AR", AR)
            put("b", b)
        return 0


@pytest.fixture
def stand_in(monkeypatch):
    return StandIn().install(monkeypatch)


def forwarded(xml, dtype, batch, overrides=None):
    """(model, Data after forward) on the CPU stand-in (the oracle runs the pass), of batch shape ``batch``."""
    B = int(np.prod(batch)) if batch else 1
    mx, d = seeded_batch(xml, overrides or {}, dtype, B)
    d = mt.forward(mx, d)
    if len(batch) == 2:
        d = torch.stack([d[i * batch[1]:(i + 1) * batch[1]] for i in range(batch[0])])
    return mx, d if batch else d[0]


def arrays(mx, d):
    """The leaves of a Data as [B, ...] numpy arrays."""
    _, _, nefc, nv, _ = sizes(mx)
    tail = dict(efc_J=(nefc, nv), qM=(nv, nv), qLD=(nv, nv))
    B = int(d.qacc.numel()) // nv
    return {n: getattr(d, n).detach().cpu().numpy().reshape((B,) + tail.get(n, (nefc if n.startswith("efc") else nv,))) for n in LEAVES}


def test_the_functions_and_the_entry_point_are_public():
    assert all(callable(getattr(mt, n)) for n in ("mul_jac_vec", "mul_jac_t_vec", "constraint_update", "efc_ar")) and native.ABI_VERSION >= 23
    assert mt.ConstraintUpdate._fields == ("jar", "efc_force", "efc_state", "qfrc_constraint", "cost", "gauss", "grad", "grad_norm")
    assert mt.EfcDual._fields == ("AR", "b")
    text = open(native.HEADER).read()
    assert re.search(r"int mjh_constraint_space\(const mjhModel\* m, const mjhConstraintSpaceArgs\* args, void\* hip_stream\);", text)
    assert re.search(r"int mjh_constraint_space_plan\(int op, int nv, int nefc, int real_bytes, int\* chunk_nchunk_last_lds\);", text)
    for i, n in enumerate(("MUL_J", "MUL_JT", "UPDATE", "AR")):
        assert re.search(rf"#define MJH_EFC_{n} {i}\b", text) and re.search(rf"#define MJH_KERNEL_EFC_{n} {50 + i}\b", text) and getattr(cs, n) == i
    assert list(native.ConstraintSpaceArgs._fields_) == header_fields(text, "mjhConstraintSpaceArgs")
    assert len(native.ARGS) == 6 and "mjh_constraint_space" not in native.ARGS  # (bound beside the table, like mjh_ray)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("batch", [(), (3,), (2, 2)], ids=["unbatched", "b3", "b2x2"])
def test_products_take_every_vector_form(stand_in, batch, dtype):
    mx, d = forwarded("ant_frictionloss", dtype, batch)
    _, _, nefc, nv, _ = sizes(mx)
    B = int(np.prod(batch)) if batch else 1
    A = arrays(mx, d)
    rng = np.random.RandomState(1)
    for fn, w, o, ref in ((mt.mul_jac_vec, nv, nefc, er.mul_jac_vec), (mt.mul_jac_t_vec, nefc, nv, er.mul_jac_t_vec)):
        for K in (None, 1, 4):
            v = torch.tensor(rng.randn(*(batch + ((K,) if K else ()) + (w,))), dtype=dtype)
            got = fn(mx, d, v)
            assert tuple(got.shape) == batch + ((K,) if K else ()) + (o,) and got.dtype == dtype
            want = ref(A["efc_J"], v.numpy().reshape(B, K or 1, w)).astype(got.numpy().dtype)
            assert np.array_equal(got.numpy().reshape(B, K or 1, o), want)
            c = stand_in.calls[-1]
            shared = batch == () and K is None  # (a lone (w,) vector is the shared form)
            assert (c["K"], c["vec_env"], c["vec_k"]) == (K or 1, 0 if shared else (K or 1) * w, w if K and K > 1 else 0)
        shared = torch.tensor(rng.randn(w), dtype=dtype)
        got = fn(mx, d, shared)
        assert tuple(got.shape) == batch + (o,) and (stand_in.calls[-1]["vec_env"], stand_in.calls[-1]["vec_k"]) == (0, 0)
        assert torch.equal(got, fn(mx, d, shared.expand(batch + (w,)).contiguous()))


@pytest.mark.parametrize("xml", ["ant_frictionloss", "equality_loops"])
def test_update_and_dual_return_the_reference(stand_in, xml):
    mx, d = forwarded(xml, F64, (3,))
    ne_nf, floss, nefc, nv, scale = sizes(mx)
    A = arrays(mx, d)
    u = mt.constraint_update(mx, d)
    assert isinstance(u, mt.ConstraintUpdate) and stand_in.calls[-1] == dict(op=cs.UPDATE, B=3, K=0, ne_nf=ne_nf, floss=int(floss), vec_env=0, vec_k=0,
                                                                            with_qacc=True, with_jar=False)
    want = update_of(mx, A, qacc=A["qacc"])
    shapes = dict(jar=(3, nefc), efc_force=(3, nefc), efc_state=(3, nefc), qfrc_constraint=(3, nv), cost=(3,), gauss=(3,), grad=(3, nv), grad_norm=(3,))
    for n, s in shapes.items():
        got = getattr(u, n)
        assert tuple(got.shape) == s and got.dtype == (torch.int32 if n == "efc_state" else F64), n
        assert np.array_equal(got.numpy(), want[n].astype(got.numpy().dtype)), n
    # the pass's own solution: the forces and the constraint force of the Data (the stand-in's pass is the oracle's)
    assert rel_err(u.efc_force.numpy(), A["efc_force"]) <= TOL_SOL[F64]
    # qacc= evaluates another acceleration; jar= classifies a given jar and computes nothing that needs qacc
    q2 = d.qacc + 0.5
    u2 = mt.constraint_update(mx, d, q2)
    assert np.array_equal(u2.cost.numpy(), update_of(mx, A, qacc=q2.numpy())["cost"].astype(np.float64)) and not torch.equal(u2.cost, u.cost)
    uj = mt.constraint_update(mx, d, jar=u2.jar)
    assert stand_in.calls[-1]["with_jar"] and not stand_in.calls[-1]["with_qacc"]
    assert uj.gauss is None and uj.grad is None and uj.grad_norm is None and uj.jar is u2.jar
    # (the stand-in rounds a longdouble jar to float64 before it is handed back: the forces agree to that rounding, not bit for bit as on the device)
    assert torch.equal(uj.efc_state, u2.efc_state) and rel_err(uj.efc_force.numpy(), u2.efc_force.numpy()) < 1e-14
    assert rel_err(uj.qfrc_constraint.numpy(), u2.qfrc_constraint.numpy()) < 1e-14
    assert torch.allclose(uj.cost + u2.gauss, u2.cost, rtol=1e-12, atol=0)
    with pytest.raises(ValueError, match="not both"):
        mt.constraint_update(mx, d, q2, jar=u2.jar)
    dual = mt.efc_ar(mx, d)
    AR, b = er.efc_ar(A["efc_J"], A["efc_D"], A["efc_aref"], A["qLD"], A["qacc_smooth"])
    assert isinstance(dual, mt.EfcDual) and tuple(dual.AR.shape) == (3, nefc, nefc) and tuple(dual.b.shape) == (3, nefc)
    assert np.array_equal(dual.AR.numpy(), AR.astype(np.float64)) and np.array_equal(dual.b.numpy(), b.astype(np.float64))
    assert torch.equal(dual.AR, dual.AR.transpose(-1, -2))


def test_unbatched_and_nested_batches(stand_in):
    for batch in ((), (2, 2)):
        mx, d = forwarded("ant_frictionloss", F32, batch)
        _, _, nefc, nv, _ = sizes(mx)
        u, dual = mt.constraint_update(mx, d), mt.efc_ar(mx, d)
        assert tuple(u.jar.shape) == batch + (nefc,) and tuple(u.cost.shape) == batch and tuple(u.grad.shape) == batch + (nv,) and u.cost.dtype == F32
        assert tuple(dual.AR.shape) == batch + (nefc, nefc) and tuple(dual.b.shape) == batch + (nefc,)


def test_a_model_without_rows_returns_without_a_call(stand_in):
    mx, d = forwarded("humanoid", F64, (3,), {"disableflags": 1})
    _, _, nefc, nv, scale = sizes(mx)
    assert nefc == 0
    n0 = len(stand_in.calls)
    assert tuple(mt.mul_jac_vec(mx, d, torch.zeros(3, 2, nv, dtype=F64)).shape) == (3, 2, 0)
    out = mt.mul_jac_t_vec(mx, d, torch.zeros(3, 0, dtype=F64))
    assert tuple(out.shape) == (3, nv) and not out.any()
    u = mt.constraint_update(mx, d)
    assert tuple(u.jar.shape) == tuple(u.efc_force.shape) == tuple(u.efc_state.shape) == (3, 0) and u.efc_state.dtype == torch.int32
    assert tuple(u.qfrc_constraint.shape) == (3, nv) and not u.qfrc_constraint.any()
    A = arrays(mx, d)
    want = er.constraint_update(A["efc_J"], A["efc_D"], A["efc_aref"], A["efc_frictionloss"], 0, False, qacc=A["qacc"] + 1, qM=A["qM"], qfrc_smooth=A["qfrc_smooth"],
                                qacc_smooth=A["qacc_smooth"], inertia_scale=scale)
    u1 = mt.constraint_update(mx, d, d.qacc + 1)  # (no rows: the Gauss term is the whole cost)
    for n in ("cost", "gauss", "grad", "grad_norm"):
        assert rel_err(getattr(u1, n).numpy(), want[n]) <= TOL_PRE[F64], n
    uj = mt.constraint_update(mx, d, jar=torch.zeros(3, 0, dtype=F64))
    assert tuple(uj.cost.shape) == (3,) and not uj.cost.any() and uj.gauss is None
    dual = mt.efc_ar(mx, d)
    assert tuple(dual.AR.shape) == (3, 0, 0) and tuple(dual.b.shape) == (3, 0)
    assert len(stand_in.calls) == n0


def test_refusals_come_before_any_call(stand_in):
    mx, d = forwarded("ant_frictionloss", F64, (3,))
    _, _, nefc, nv, _ = sizes(mx)
    n0 = len(stand_in.calls)
    v, f = torch.zeros(3, nv, dtype=F64), torch.zeros(3, nefc, dtype=F64)
    bad = [
        (ValueError, "vec must have shape", lambda: mt.mul_jac_vec(mx, d, torch.zeros(3, nv + 1, dtype=F64))),
        (ValueError, "vec must have shape", lambda: mt.mul_jac_vec(mx, d, torch.zeros(2, nv, dtype=F64))),
        (ValueError, "vec must have shape", lambda: mt.mul_jac_t_vec(mx, d, v)),
        (ValueError, "no vectors", lambda: mt.mul_jac_vec(mx, d, torch.zeros(3, 0, nv, dtype=F64))),
        (ValueError, "float32", lambda: mt.mul_jac_vec(mx, d, v.float())),
        (ValueError, "must be a tensor", lambda: mt.mul_jac_vec(mx, d, [0.0] * nv)),
        (ValueError, "qacc= must have shape", lambda: mt.constraint_update(mx, d, torch.zeros(nv, dtype=F64))),
        (ValueError, "qacc= is torch.float32", lambda: mt.constraint_update(mx, d, v.float())),
        (ValueError, "jar= must have shape", lambda: mt.constraint_update(mx, d, jar=v)),
        (ValueError, "efc_J has shape", lambda: mt.efc_ar(mx, d.replace(efc_J=d.efc_J[:, :-1]))),
        (ValueError, "efc_D", lambda: mt.constraint_update(mx, d.replace(efc_D=d.efc_D[:1]))),
        (ValueError, "qLD", lambda: mt.efc_ar(mx, d.replace(qLD=d.qLD.float()))),
        (ValueError, "dtype|float32", lambda: mt.constraint_update(mx, d.to(F32))),
        (NotImplementedError, "constraint_update cannot be used under torch.vmap", lambda: torch.vmap(lambda q: mt.constraint_update(mx, d, q).cost)(torch.zeros(2, 3, nv, dtype=F64))),
        (NotImplementedError, "mul_jac_vec cannot be used under torch.vmap", lambda: torch.vmap(lambda q: mt.mul_jac_vec(mx, d, q))(torch.zeros(2, 3, nv, dtype=F64))),
        (NotImplementedError, "efc_ar cannot be used under torch.vmap", lambda: torch.vmap(lambda j: mt.efc_ar(mx, d.replace(efc_J=j)).b)(d.efc_J[None])),
    ]
    for exc, match, run in bad:
        with pytest.raises(exc, match=match):
            run()
    with pytest.raises(Exception, match="mul_jac_t_vec cannot be used under torch.vmap / torch.compile"):
        torch.compile(lambda x: mt.mul_jac_t_vec(mx, d, x), backend="eager", fullgraph=True)(f)
    assert len(stand_in.calls) == n0


def test_without_the_stand_in_cpu_data_is_refused(monkeypatch):
    _hostsim.install(monkeypatch)
    mx, d = forwarded("ant_frictionloss", F64, (2,))
    monkeypatch.undo()
    with pytest.raises(RuntimeError, match="HIP device"):
        mt.efc_ar(mx, d)


def test_a_library_from_before_the_functions_is_named(monkeypatch):
    _hostsim.install(monkeypatch)  # (its library has no mjh_constraint_space)
    mx, d = forwarded("ant_frictionloss", F64, (2,))
    for run in (lambda: mt.efc_ar(mx, d), lambda: mt.constraint_update(mx, d), lambda: mt.mul_jac_vec(mx, d, d.qacc)):
        with pytest.raises(RuntimeError, match=r"predates the constraint-space functions \(no mjh_constraint_space\): rebuild the library"):
            run()


def test_the_plan_is_the_librarys():
    """(rows per chunk, chunks, rows of the last chunk, LDS bytes): a staged row takes nv | 1 reals; every chunk but the last is full."""
    for op in (cs.MUL_J, cs.MUL_JT, cs.UPDATE, cs.AR):
        for nv, nefc, dtype in ((27, 53, F64), (8, 256, F64), (83, 60, F64), (154, 100, F32), (1, 1, F32)):
            chunk, nchunk, last, lds = cs.plan(op, nv, nefc, dtype)
            assert 1 <= last <= chunk and (nchunk - 1) * chunk + last == nefc and lds <= 160 * 1024 and lds >= chunk * (nv | 1) * (8 if dtype == F64 else 4)
    assert cs.plan(cs.AR, 83, 60, F64)[1] >= 3 and cs.plan(cs.UPDATE, 154, 100, F32)[1] >= 3
    with pytest.raises(RuntimeError, match="plan failed"):
        cs.plan(cs.AR, 256, 300, F64)  # (the triangle alone is 263 KB)
