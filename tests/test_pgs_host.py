"""``solve_pgs`` without a GPU: the tests' numpy reference (tests/_pgs_ref.py, the yardstick of tests/test_pgs.py) pinned on a hand-worked problem and on the recorded
solver outputs of the goldens, the library's plan, and the public function with the launch replaced by that reference.

Measured here (printed by the tests).  On the recordings (pyramidal cones), longdouble, 24 sweeps from zeros: the dual cost falls on every sweep but for rises of
rounding size once an environment has converged (1.4e-14 on a cost of 1e5 on the humanoid, 5.8e-11 on 3.5e8 on the ant: at most 1.5e-4 of the slack); weak duality
holds with gaps of 212 (humanoid, CG), 1608 (humanoid, Newton) and 4e4 (equality loops) where 24 sweeps have not converged, and -2.9e-11, 2e-6 of the slack, on the
ant, which has.  Convergence to the recorded ``efc_force`` at TOL_SOL[float64] = 1e-8 by ``_util.rel_err``: the ant with friction loss after 1 sweep (its ``AR`` is
diagonal to rounding: one sweep is the exact solve, error 0) and the equality loops after 1024 sweeps (3.9e-11 on the two environment-steps the test runs, 1.1e-9
over all nine; 512 sweeps leave 2.4e-6).  The humanoid recordings are not converged solves (its model is configured for ONE solver iteration; ``grad_norm`` 5 to
11), so there the recorded force is not the optimum and only monotonicity and duality apply.
"""
import ctypes
import re
import time

import numpy as np
import pytest
import torch

import _efc_ref as er
import _hostsim
import _pgs_ref as pr
import mujoco_torch_amd as mt
from _cases import F32, F64, TOL_SOL, seeded_batch
from _util import rel_err
from mujoco_torch_amd import native
from mujoco_torch_amd import pgs
from test_abi import header_fields
from test_constraint_space_host import CASES, forwarded, recorded, update_of

LD = er.LD
EPS_LD = float(np.finfo(LD).eps)


def sizes(m):
    ne, nf, _, _, nefc = (int(x) for x in m.constraint_sizes_py)
    return ne, nf, nefc, int(m.nv), float(m.stat.meaninertia) * max(1, int(m.nv))


def solve_recorded(case, sweeps, dtype=LD, rows=slice(None), **kw):
    m, r = recorded(case)
    ne, nf, _, _, scale = sizes(m)
    return pr.solve_pgs(r["efc_J"][rows], r["efc_D"][rows], r["efc_aref"][rows], r["efc_frictionloss"][rows], r["qLD"][rows], r["qacc_smooth"][rows], ne, nf, scale,
                        sweeps, dtype=dtype, **kw)


# ---- 1. the reference on a problem worked by hand ------------------------------------------------------------------------------------------

def hand(b):
    """nv = 2, ``qLD = I``, ``J = [[1, 0], [1, 1]]``, ``D = [1, 1]``, ``qacc_smooth = 0``, ``aref = -b``: ``AR = J J^T + I = [[2, 1], [1, 3]]``.  Row 0 is an
    equality row (free), row 1 unilateral; ``inertia_scale = 2``."""
    J = np.array([[[1.0, 0.0], [1.0, 1.0]]])
    return dict(J=J, D=np.ones((1, 2)), aref=-np.asarray(b, dtype=np.float64)[None], fl=np.zeros((1, 2)), qLD=np.eye(2)[None], qacc_smooth=np.zeros((1, 2)), ne=1, nf=0,
                inertia_scale=2.0)


def test_the_reference_on_a_hand_worked_problem():
    """``AR = [[2, 1], [1, 3]]``, ``b = (-2, -4)``, from ``f = 0``.  First sweep: row 0 (free): ``res = -2``, ``f_0 = 0 + 2 / 2 = 1``, ``delta = 1``,
    ``improvement = -1 (1/2 . 1 . 2 - 2) = 1``; row 1 (``f >= 0``): ``res = 1 . 1 + 3 . 0 - 4 = -3``, ``f_1 = max(0, 0 + 3 / 3) = 1``, ``delta = 1``,
    ``improvement += -1 (1/2 . 1 . 3 - 3) = 1.5``: 2.5 in all, ``/ 2 = 1.25`` scaled; the cost is ``1/2 (2 + 1 + 1 + 3) - 2 - 4 = -2.5``: what the sweep gained.
    Fixed point: ``AR f = -b`` has the feasible solution ``f = (0.4, 1.2)`` (``2 (0.4) + 1.2 = 2``, ``0.4 + 3 (1.2) = 4``), cost ``1/2 f . b = -2.8``; Gauss-Seidel
    on this matrix contracts by ``1 . 1 / (2 . 3) = 1/6`` a sweep.  ``qfrc_constraint = J^T f = (f_0 + f_1, f_1)`` and, with ``qLD = I``, ``qacc`` is the same.

    With ``b = (-2, 4)`` the unilateral row binds: row 1 has ``res = 1 + 4 = 5 > 0`` and stays at 0, ``f = (1, 0)`` is the fixed point after one sweep, cost -1,
    and the second sweep improves nothing.  A start of ``(0, -3)`` is projected to ``(0, 0)``: the same sweeps."""
    p = hand((-2.0, -4.0))
    out = pr.solve_pgs(p["J"], p["D"], p["aref"], p["fl"], p["qLD"], p["qacc_smooth"], p["ne"], p["nf"], p["inertia_scale"], 40)
    assert np.array_equal(out["AR"][0], [[2, 1], [1, 3]]) and np.array_equal(out["b"][0], [-2, -4])
    assert np.array_equal(out["forces"][0][0], [0, 0]) and np.array_equal(out["forces"][1][0], [1, 1])
    assert out["improvements"][0][0] == 1.25 and out["costs"][0][0] == 0 and out["costs"][1][0] == -2.5
    assert np.abs(out["efc_force"][0] - np.array([LD(4) / 10, LD(12) / 10])).max() < 1e-17 and abs(out["cost"][0] + LD(28) / 10) < 1e-17
    assert np.abs(out["qfrc_constraint"][0] - np.array([LD(16) / 10, LD(12) / 10])).max() < 1e-17 and np.array_equal(out["qacc"], out["qfrc_constraint"])
    ratio = f64(np.abs(out["forces"][3][0] - out["efc_force"][0]) / np.abs(out["forces"][2][0] - out["efc_force"][0]))
    assert np.allclose(ratio, 1 / 6, rtol=1e-9), ratio
    assert (out["niter"] == 40).all() and (np.diff(f64(out["costs"][:, 0])) <= 0).all()
    p = hand((-2.0, 4.0))
    for start in (None, np.array([[0.0, -3.0]])):
        out = pr.solve_pgs(p["J"], p["D"], p["aref"], p["fl"], p["qLD"], p["qacc_smooth"], p["ne"], p["nf"], p["inertia_scale"], 3, force0=start)
        assert np.array_equal(out["forces"][0][0], [0, 0]) and all(np.array_equal(out["forces"][k][0], [1, 0]) for k in (1, 2, 3))
        assert out["improvements"][0][0] == 0.5 and out["improvements"][1][0] == 0 and out["costs"][1][0] == -1
    # the stopping rule: improvement < tolerance ends an environment, the one that goes on is not touched by it
    p2 = {k: (np.concatenate([v, v]) if isinstance(v, np.ndarray) else v) for k, v in hand((-2.0, -4.0)).items()}
    p2["aref"][1] = [2.0, -4.0]  # (environment 1: the binding problem)
    out = pr.solve_pgs(p2["J"], p2["D"], p2["aref"], p2["fl"], p2["qLD"], p2["qacc_smooth"], p2["ne"], p2["nf"], p2["inertia_scale"], 6, tolerance=1e-3)
    # (environment 0: the improvements 1.25, 0.1458, then 1/36 of the last one a sweep: 4.05e-3, 1.1e-4 -- the fourth sweep is the first below 1e-3)
    assert out["niter"].tolist() == [4, 2] and out["improvement"][1] == 0 and out["improvement"][0] < 1e-3 <= out["improvements"][2][0]
    assert abs(out["improvements"][1][0] - LD(7) / 48) < 1e-18 and np.isnan(f64(out["improvements"][4:, 0])).all()
    assert np.array_equal(out["forces"][6][0], out["forces"][4][0]) and not np.array_equal(out["forces"][4][0], out["forces"][3][0])
    # a friction row: |f| <= fl
    p = hand((-2.0, -4.0))
    out = pr.solve_pgs(p["J"], p["D"], p["aref"], np.array([[0.25, 0.0]]), p["qLD"], p["qacc_smooth"], 0, 1, p["inertia_scale"], 30)
    assert out["efc_force"][0][0] == 0.25 and abs(out["efc_force"][0][1] - LD(3.75) / 3) < 1e-17  # (row 0 on its bound: f_1 = (4 - 0.25) / 3)


def f64(x):
    return np.asarray(x, dtype=np.float64)


# ---- 2. the reference on the recordings ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES)
def test_the_dual_cost_falls_and_weak_duality_holds_on_the_recordings(case):
    """In longdouble, 24 sweeps from zeros.  The dual cost is non-increasing sweep by sweep up to the rounding of its terms, ``(n^2 + n) eps_LD S`` with ``S`` the
    sum of the magnitudes of the terms of ``1/2 f^T AR f + f^T b``.  Weak duality: with ``P`` the primal cost (``_efc_ref.constraint_update``) of the recorded
    ``qacc``, ``cost_k + P >= -slack`` after every sweep; the slack is that rounding, plus ``10 nv eps_64 cond(M)`` of the quadratic term for the float64
    factor ``qLD`` the dual is made from while the primal reads ``qM`` (the bound of tests/test_constraint_space_host.py for ``AR``), plus, past 16 dofs where
    ``qLD`` factors ``qM + 1e-10 I``, the ``1/2 1e-10 qacc . (qacc - qacc_smooth)`` the primal of that matrix has over the primal of ``qM``."""
    m, r = recorded(case)
    ne, nf, nefc, nv, _ = sizes(m)
    assert int(m.opt.cone) == 0  # pyramidal
    out = solve_recorded(case, 24)
    AR, b, forces, costs = out["AR"], out["b"], out["forces"], out["costs"]
    S = np.stack([np.einsum("bi,bij,bj->b", np.abs(f), np.abs(AR), np.abs(f)) / 2 + (np.abs(f) * np.abs(b)).sum(-1) for f in forces])
    rounding = (nefc * nefc + nefc) * EPS_LD * S
    rise = costs[1:] - costs[:-1]
    print(f"{case}: cost {f64(costs[0]).max():.4g} -> {f64(costs[-1]).min():.6g}; largest rise {float(rise.max()):.3g}, largest rise / slack "
          f"{float((rise / np.maximum(rounding[1:], 1e-4000)).max()):.3g}")
    assert (rise <= np.maximum(rounding[1:], rounding[:-1])).all()
    assert (costs[-1] < costs[0]).all()
    P = update_of(m, r, qacc=r["qacc"])["cost"]
    cond = np.array([np.linalg.cond(M) for M in r["qM"]])
    quad = np.stack([np.einsum("bi,bij,bj->b", f, AR, f) / 2 for f in forces])
    reg = 0.5e-10 * np.abs((er.ld(r["qacc"]) * (er.ld(r["qacc"]) - er.ld(r["qacc_smooth"]))).sum(-1)) if nv > 16 else 0
    slack = rounding + (nefc + nv) * EPS_LD * np.abs(P) + 10 * nv * np.finfo(np.float64).eps * cond * np.abs(quad) + reg
    gap = costs + P
    print(f"  dual + primal after 24 sweeps: min {float(gap[-1].min()):.4g} (of a primal cost of {float(P.min()):.4g} .. {float(P.max()):.4g}); smallest gap / slack "
          f"{float((gap[1:] / slack[1:]).min()):.3g}")
    assert (gap >= -slack).all()


def test_one_sweep_solves_the_ant_whose_ar_is_diagonal():
    """The recorded ``efc_force`` of the ant with friction loss at TOL_SOL after ONE sweep: no two of its active rows share a dof (the contact rows are inactive),
    ``AR`` is diagonal (its largest off-diagonal entry is 1e-16, the last bits of the float64 factor ``qLD``: ``|AR_ij| <= 10 nv eps sqrt(AR_ii AR_jj)``, measured 1.3e-15) and a sweep
    is the exact solve of every row, bounds included (friction rows end on their bounds)."""
    for case in ("ant_frictionloss_newton_f64", "ant_frictionloss_cg_f64"):
        m, r = recorded(case)
        out = solve_recorded(case, 2)
        off = out["AR"] * (1 - np.eye(out["AR"].shape[-1]))
        err = [max(rel_err(f64(out["forces"][k][i]), r["efc_force"][i]) for i in range(len(r["qacc"]))) for k in (1, 2)]
        print(f"{case}: largest off-diagonal |AR| {float(np.abs(off).max()):.3g}; force against the recording after 1, 2 sweeps {err}")
        dg = np.einsum("bii->bi", out["AR"])
        coupling = np.abs(off) / np.sqrt(dg[:, :, None] * dg[:, None, :])
        print(f"  largest |AR_ij| / sqrt(AR_ii AR_jj) {float(coupling.max()):.3g}")
        assert (dg > 0).all() and coupling.max() <= 10 * sizes(m)[3] * np.finfo(np.float64).eps and max(err) <= TOL_SOL[F64]  # (diagonal to the last bits of the float64 factor qLD)
        ne, nf = sizes(m)[:2]
        assert (np.abs(out["efc_force"][:, ne:ne + nf]) == r["efc_frictionloss"][:, ne:ne + nf]).any()


SWEEPS_EQUALITY = 1024  # picked on the CPU: 512 sweeps leave 2.4e-6 (3.9e-6 over all nine environment-steps), 1024 reach 3.9e-11 (1.1e-9)


def test_the_reference_converges_to_the_recorded_forces():
    """The equality loops (14 equality rows coupled through 17 dofs, 180 contact rows): the reference reaches the recorded Newton solve's ``efc_force`` at
    TOL_SOL[float64] after 1024 sweeps.  Run in float64 -- the iteration contracts, so rounding does not accumulate over the sweeps -- on the first two
    recorded environment-steps: longdouble, the yardstick elsewhere, takes twice as long here for the same figure."""
    m, r = recorded("equality_loops_f64")
    t = time.time()
    out = solve_recorded("equality_loops_f64", SWEEPS_EQUALITY, dtype=np.float64, rows=slice(0, 2))
    err = {k: max(rel_err(out["forces"][k][i], r["efc_force"][i]) for i in range(2)) for k in (SWEEPS_EQUALITY // 2, SWEEPS_EQUALITY)}
    print(f"equality_loops_f64: force against the recording {err} ({time.time() - t:.1f} s)")
    assert err[SWEEPS_EQUALITY] <= TOL_SOL[F64] < err[SWEEPS_EQUALITY // 2]


# ---- 3. the plan -----------------------------------------------------------------------------------------------------------------------------

def test_the_plan_is_the_librarys():
    """(rows per staging step, steps, rows of the last step, LDS bytes): a staged row takes nv | 1 reals, every step but the last is full, and the LDS holds the
    packed triangle of qLD, all nefc rows, five reals a row, two dof vectors and 64 partial sums."""
    for nv, nefc, dtype in ((27, 53, F64), (8, 256, F64), (8, 256, F32), (17, 194, F64), (106, 80, F64), (129, 80, F64), (154, 100, F32), (1, 1, F32)):
        size = 8 if dtype == F64 else 4
        chunk, nchunk, last, lds = pgs.plan(nv, nefc, dtype)
        assert 1 <= last <= chunk and (nchunk - 1) * chunk + last == nefc
        assert chunk == max(1, min(16 * 1024 // ((nv | 1) * size), nefc))
        assert lds == ((nv * (nv + 1) // 2 + nefc * (nv | 1) + 5 * nefc + 2 * nv + 64) * size + 15) // 16 * 16 <= 160 * 1024
    assert pgs.plan(27, 53, F64)[1] == 1 and pgs.plan(8, 256, F64)[:3] == (227, 2, 29) and pgs.plan(106, 80, F64)[:3] == (19, 5, 4) and pgs.plan(154, 100, F32)[:3] == (26, 4, 22)
    with pytest.raises(RuntimeError, match=r"nv = 154, nefc = 100 in torch.float64 need 226464 bytes of LDS .* a workgroup has 163840"):
        pgs.plan(154, 100, F64)
    lib = native.load_library()
    out = (ctypes.c_int * 4)()
    assert lib.mjh_pgs_plan(154, 100, 8, out) == -12 and out[3] == 226464 and lib.mjh_pgs_plan(-1, 1, 8, out) == -22 and lib.mjh_pgs_plan(1, 1, 2, out) == -22


# ---- 4. the public function on a stand-in ----------------------------------------------------------------------------------------------------------

class StandIn:
    """``mjh_pgs`` of the CPU stand-in library: the numpy reference on the host pointers it is handed."""

    def __init__(self):
        self.calls = []

    def install(self, monkeypatch):
        _hostsim.install(monkeypatch)
        monkeypatch.setattr(_hostsim._Lib, "mjh_pgs", self, raising=False)
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
        self.calls.append(dict(B=B, ne=int(a.ne), nf=int(a.nf), iterations=int(a.iterations), tolerance=float(a.tolerance), meaninertia=float(a.meaninertia),
                               force0=bool(a.force0), force0_env=int(a.force0_env)))
        f0 = None
        if a.force0:
            f0 = view(a.force0, (B - 1) * a.force0_env + n)[np.arange(B)[:, None] * a.force0_env + np.arange(n)]
        out = pr.solve_pgs(leaf("efc_J", n, nv), leaf("efc_D", n), leaf("efc_aref", n), leaf("efc_frictionloss", n), leaf("qLD", nv, nv), leaf("qacc_smooth", nv),
                           int(a.ne), int(a.nf), a.meaninertia * max(1, nv), int(a.iterations), tolerance=a.tolerance, force0=f0)
        for name in ("efc_force", "qfrc_constraint", "qacc", "cost", "improvement"):
            put(name, out[name])
        put("niter", out["niter"], ctypes.c_int32, np.int32)
        return 0


@pytest.fixture
def stand_in(monkeypatch):
    return StandIn().install(monkeypatch)


def reference_of(mx, d, B, sweeps, **kw):
    ne, nf, nefc, nv, scale = sizes(mx)
    h = lambda n, *s: getattr(d, n).detach().numpy().reshape((B,) + s)
    return pr.solve_pgs(h("efc_J", nefc, nv), h("efc_D", nefc), h("efc_aref", nefc), h("efc_frictionloss", nefc), h("qLD", nv, nv), h("qacc_smooth", nv), ne, nf, scale,
                        sweeps, **kw)


def test_the_function_and_the_entry_point_are_public():
    assert callable(mt.solve_pgs) and mt.PGSResult._fields == ("efc_force", "qfrc_constraint", "qacc", "cost", "improvement", "niter")
    assert native.ABI_VERSION >= 24
    text = open(native.HEADER).read()
    assert re.search(r"int mjh_pgs\(const mjhModel\* m, const mjhPgsArgs\* args, void\* hip_stream\);", text)
    assert re.search(r"int mjh_pgs_plan\(int nv, int nefc, int real_bytes, int\* chunk_nchunk_last_lds\);", text)
    assert re.search(r"#define MJH_KERNEL_PGS 54\b", text)
    assert list(native.PgsArgs._fields_) == header_fields(text, "mjhPgsArgs")
    assert len(native.ARGS) == 6 and "mjh_pgs" not in native.ARGS  # (bound beside the table, like mjh_constraint_space)
    lib = native.load_library()
    assert lib.mjh_pgs.argtypes[1]._type_ is native.PgsArgs and "solve_pgs" in mt.__doc__


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("batch", [(), (3,), (2, 2)], ids=["unbatched", "b3", "b2x2"])
def test_the_function_returns_the_reference(stand_in, batch, dtype):
    mx, d = forwarded("ant_frictionloss", dtype, batch)
    ne, nf, nefc, nv, scale = sizes(mx)
    B = int(np.prod(batch)) if batch else 1
    before = {n: getattr(d, n).clone() for n in ("efc_J", "efc_D", "efc_aref", "efc_frictionloss", "qLD", "qacc_smooth", "efc_force", "qacc")}
    res = mt.solve_pgs(mx, d)
    assert isinstance(res, mt.PGSResult)
    assert stand_in.calls[-1] == dict(B=B, ne=ne, nf=nf, iterations=int(mx.opt.iterations), tolerance=float(mx.opt.tolerance), meaninertia=float(mx.stat.meaninertia),
                                      force0=False, force0_env=0)
    want = reference_of(mx, d, B, int(mx.opt.iterations), tolerance=float(mx.opt.tolerance))
    shapes = dict(efc_force=batch + (nefc,), qfrc_constraint=batch + (nv,), qacc=batch + (nv,), cost=batch, improvement=batch, niter=batch)
    for n, s in shapes.items():
        got = getattr(res, n)
        assert tuple(got.shape) == s and got.dtype == (torch.int32 if n == "niter" else dtype), n
        assert np.array_equal(got.numpy().reshape(-1), np.asarray(want[n]).astype(got.numpy().dtype).reshape(-1)), n
    assert all(torch.equal(getattr(d, n), t) for n, t in before.items())  # nothing is written to d
    rng = np.random.RandomState(2)
    per_env, shared = torch.tensor(rng.randn(*(batch + (nefc,))) * 50, dtype=dtype), torch.tensor(rng.randn(nefc) * 50, dtype=dtype)
    for f0, stride in ((per_env, nefc if batch else 0), (shared, 0)):
        res = mt.solve_pgs(mx, d, iterations=3, tolerance=0.0, force0=f0)
        c = stand_in.calls[-1]
        assert (c["iterations"], c["tolerance"], c["force0"], c["force0_env"]) == (3, 0.0, True, stride)
        want = reference_of(mx, d, B, 3, force0=np.broadcast_to(f0.numpy().reshape((-1, nefc)), (B, nefc)))
        assert np.array_equal(res.efc_force.numpy().reshape(B, nefc), want["efc_force"].astype(res.efc_force.numpy().dtype))
        assert (res.niter == 3).all()
    zero = mt.solve_pgs(mx, d, iterations=0, force0=per_env)
    assert stand_in.calls[-1]["iterations"] == 0 and not zero.niter.any() and not zero.improvement.any()
    assert np.array_equal(zero.efc_force.numpy().reshape(B, nefc), pr.project(per_env.numpy().reshape(B, nefc), d.efc_frictionloss.numpy().reshape(B, nefc), ne, nf))


def test_the_output_of_step_is_valid_input(stand_in):
    mx, d = seeded_batch("ant_frictionloss", {}, F64, 2)
    d = mt.step(mx, d)
    res = mt.solve_pgs(mx, d, iterations=2, tolerance=0.0)
    assert rel_err(res.efc_force.numpy(), d.efc_force.numpy()) <= TOL_SOL[F64]  # (the leaves of the pass step integrated; the ant is solved by one sweep)


def test_empty_cases_are_answered_on_the_host(stand_in):
    mx, d = forwarded("ant_frictionloss", F64, (3,))
    ne, nf, nefc, nv, _ = sizes(mx)
    n0 = len(stand_in.calls)
    res = mt.solve_pgs(mx, d[:0])
    assert tuple(res.efc_force.shape) == (0, nefc) and tuple(res.qacc.shape) == (0, nv) and tuple(res.cost.shape) == (0,) and res.niter.dtype == torch.int32
    mx, d = forwarded("humanoid", F64, (3,), {"disableflags": 1})
    assert sizes(mx)[2] == 0
    res = mt.solve_pgs(mx, d, force0=torch.zeros(3, 0, dtype=F64))
    assert tuple(res.efc_force.shape) == (3, 0) and tuple(res.qfrc_constraint.shape) == (3, int(mx.nv)) and not res.qfrc_constraint.any()
    assert torch.equal(res.qacc, d.qacc_smooth) and not res.cost.any() and not res.improvement.any() and not res.niter.any()
    assert len(stand_in.calls) == n0


def test_refusals_come_before_any_call(stand_in):
    mx, d = forwarded("ant_frictionloss", F64, (3,))
    ne, nf, nefc, nv, _ = sizes(mx)
    n0 = len(stand_in.calls)
    f = torch.zeros(3, nefc, dtype=F64)
    bad = [
        (ValueError, "force0= must have shape", lambda: mt.solve_pgs(mx, d, force0=torch.zeros(2, nefc, dtype=F64))),
        (ValueError, "force0= must have shape", lambda: mt.solve_pgs(mx, d, force0=torch.zeros(3, nefc + 1, dtype=F64))),
        (ValueError, "force0= must have shape", lambda: mt.solve_pgs(mx, d, force0=[0.0] * nefc)),
        (ValueError, "force0= is torch.float32", lambda: mt.solve_pgs(mx, d, force0=f.float())),
        (ValueError, "iterations must be an integer >= 0", lambda: mt.solve_pgs(mx, d, iterations=-1)),
        (ValueError, "iterations must be an integer >= 0", lambda: mt.solve_pgs(mx, d, iterations=2.5)),
        (ValueError, "tolerance must be >= 0", lambda: mt.solve_pgs(mx, d, tolerance=-1e-9)),
        (ValueError, "tolerance must be >= 0", lambda: mt.solve_pgs(mx, d, tolerance=float("nan"))),
        (ValueError, "efc_J has shape", lambda: mt.solve_pgs(mx, d.replace(efc_J=d.efc_J[:, :-1]))),
        (ValueError, "efc_D", lambda: mt.solve_pgs(mx, d.replace(efc_D=d.efc_D[:1]))),
        (ValueError, "qLD", lambda: mt.solve_pgs(mx, d.replace(qLD=d.qLD.float()))),
        (ValueError, "dtype|float32", lambda: mt.solve_pgs(mx, d.to(F32))),
        (NotImplementedError, "solve_pgs cannot be used under torch.vmap", lambda: torch.vmap(lambda x: mt.solve_pgs(mx, d, force0=x).cost)(torch.zeros(2, 3, nefc, dtype=F64))),
    ]
    for exc, match, run in bad:
        with pytest.raises(exc, match=match):
            run()
    with pytest.raises(Exception, match="solve_pgs cannot be used under torch.vmap / torch.compile"):
        torch.compile(lambda x: mt.solve_pgs(mx, d, force0=x).cost, backend="eager", fullgraph=True)(f)
    assert len(stand_in.calls) == n0


_FRICTIONLESS = """
<mujoco>
  <option cone="{cone}"/>
  <worldbody>
    <geom type="plane" size="2 2 .01" condim="1"/>
    <body pos="0 0 .09"><freejoint/><geom type="sphere" size=".1" condim="1"/></body>
    <body pos=".19 0 .09"><freejoint/><geom type="sphere" size=".1" condim="1"/></body>
  </worldbody>
</mujoco>
"""


def test_elliptic_cones_with_friction_are_refused(stand_in):
    mx, d = seeded_batch("ant", {"cone": 1}, F64, 2)
    n0 = len(stand_in.calls)
    with pytest.raises(NotImplementedError, match="ELLIPTIC .* condim"):
        mt.solve_pgs(mx, d)  # (before any leaf is looked at: the Data need not even hold a pass)
    assert len(stand_in.calls) == n0
    # a frictionless elliptic model has rows of dimension one only: served, and the same problem as its pyramidal twin
    res = {}
    for cone in ("pyramidal", "elliptic"):
        mx = mt.device_put(mt.mjcf.from_xml_string(_FRICTIONLESS.format(cone=cone)))
        d = mt.forward(mx, mt.make_data(mx).expand(2).clone())
        assert int(mx.opt.cone) == (cone == "elliptic") and tuple(mx.constraint_sizes_py) == (0, 0, 0, 3, 3)
        res[cone] = mt.solve_pgs(mx, d, iterations=5, tolerance=0.0)
        assert stand_in.calls[-1]["B"] == 2
    assert res["elliptic"].efc_force.abs().min() > 0 and torch.equal(res["pyramidal"].efc_force, res["elliptic"].efc_force)
    with pytest.raises(NotImplementedError, match="solver PGS not implemented"):  # device_put refuses opt.solver = PGS as before
        seeded_batch("ant", {"solver": 0}, F64, 1)


def test_without_the_stand_in_cpu_data_is_refused(monkeypatch):
    _hostsim.install(monkeypatch)
    mx, d = forwarded("ant_frictionloss", F64, (2,))
    monkeypatch.undo()
    with pytest.raises(RuntimeError, match="HIP device"):
        mt.solve_pgs(mx, d)


def test_a_library_from_before_the_function_is_named(monkeypatch):
    _hostsim.install(monkeypatch)  # (its library has no mjh_pgs)
    mx, d = forwarded("ant_frictionloss", F64, (2,))
    with pytest.raises(RuntimeError, match=r"predates solve_pgs \(no mjh_pgs\): rebuild the library"):
        mt.solve_pgs(mx, d)
