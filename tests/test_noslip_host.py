"""``solve_noslip`` without a GPU: the tests' numpy reference (tests/_noslip_ref.py, the yardstick of tests/test_noslip.py) pinned on problems worked by hand, the
library's plan, and the public function with the launch replaced by that reference.
"""
import ctypes
import re

import numpy as np
import pytest
import torch

import _hostsim
import _noslip_ref as nr
import mujoco_torch_amd as mt
from _cases import F32, F64, seeded_batch
from mujoco_torch_amd import native
from mujoco_torch_amd import noslip
from test_abi import header_fields
from test_constraint_space_host import forwarded

LD = nr.LD


def sizes(m):
    ne, nf, _, ncon, nefc = (int(x) for x in m.constraint_sizes_py)
    return ne, nf, nefc, int(m.nv), float(m.stat.meaninertia) * max(1, int(m.nv)), ncon


def f64(x):
    return np.asarray(x, dtype=np.float64)


# ---- 1. the reference on problems worked by hand ---------------------------------------------------------------------------------------------

def pair_problem(f0, b):
    """nv = 2, ``qLD = I``, ``J = [[1, 0], [0, 2]]``: ``A = diag(1, 4)``; ``qacc_smooth = 0``, ``aref = -b``; one pyramidal contact of condim 2 -- a single pair,
    rows (0, 1) -- and ``D = 1`` (``R = 1``); ``inertia_scale = 2``."""
    J = np.array([[[1.0, 0.0], [0.0, 2.0]]])
    return dict(J=J, D=np.ones((1, 2)), aref=-np.asarray(b, dtype=np.float64)[None], fl=np.zeros((1, 2)), qLD=np.eye(2)[None], qacc_smooth=np.zeros((1, 2)),
                force0=np.asarray(f0, dtype=np.float64)[None], mu=np.ones((1, 1, 5)), ne=0, nf=0, con=[(0, 2)], elliptic=False, inertia_scale=2.0)


def run(p, sweeps, **kw):
    return nr.solve_noslip(p["J"], p["D"], p["aref"], p["fl"], p["qLD"], p["qacc_smooth"], p["force0"], p["mu"], p["ne"], p["nf"], p["con"], p["elliptic"],
                           p["inertia_scale"], sweeps, **kw)


def test_a_pyramid_pair_interior_and_clamped():
    """``A = diag(1, 4)``, the pair ``(f_0, f_1)`` with ``f_0 + f_1 = 2 mid`` kept.  On the line ``f = (mid + y, mid - y)`` the cost
    ``1/2 (mid + y)^2 + 2 (mid - y)^2 + b_0 (mid + y) + b_1 (mid - y)`` has ``d/dy = 5 y - 3 mid + b_0 - b_1``: ``K1 = 1 + 4 = 5``,
    ``K0 = mid (1 - 4) + bc_0 - bc_1`` with ``bc = res - A f_old = b``.

    Interior: ``f = (3, 1)``, ``b = (0, 1)``: ``mid = 2``, ``y = (6 + 1) / 5 = 1.4`` inside ``+-2``: ``f = (3.4, 0.6)``.  ``res = A f + b = (3, 5)``,
    ``delta = (0.4, -0.4)``: ``change = 1/2 (0.16 + 0.64) + (1.2 - 2) = -0.4``; the first sweep adds ``1/2 sum R f^2 = 1/2 (9 + 1) = 5``:
    ``improvement = (5 + 0.4) / 2 = 2.7``.  A second sweep finds the same optimum: ``improvement = 0``.
    Clamped: ``b = (0, 11)``: ``y = (6 + 11) / 5 = 3.4 > mid``: ``f = (4, 0)``, and with ``b = (11, 0)``: ``y = (6 - 11) / 5 = -1``, interior again: ``(1, 3)``;
    ``b = (30, 0)``: ``y = -4.8 < -mid``: ``f = (0, 4)``."""
    out = run(pair_problem((3.0, 1.0), (0.0, 1.0)), 2)
    assert np.array_equal(out["A"][0], [[1, 0], [0, 4]]) and np.array_equal(out["b"][0], [0, 1])
    assert np.abs(out["forces"][1][0] - np.array([LD(34) / 10, LD(6) / 10])).max() < 1e-18
    assert abs(out["improvements"][0][0] - LD(27) / 10) < 1e-18 and abs(out["improvements"][1][0]) < 1e-18
    assert out["status"][0][(0, 0)][0] == nr.INTERIOR
    assert abs(out["costs"][1][0] - out["costs"][0][0] + LD(4) / 10) < 1e-17  # (the cost fell by what the block reported)
    for b, want, st in (((0.0, 11.0), (4, 0), nr.BOUNDARY), ((11.0, 0.0), (1, 3), nr.INTERIOR), ((30.0, 0.0), (0, 4), nr.BOUNDARY)):
        out = run(pair_problem((3.0, 1.0), b), 1)
        assert np.array_equal(out["forces"][1][0], want) and out["status"][0][(0, 0)][0] == st, b
        assert out["forces"][1][0].sum() == 4
    # float64 runs the same rules; iterations = 0 returns the start with its cost and no improvement
    out = run(pair_problem((3.0, 1.0), (0.0, 1.0)), 0, dtype=np.float64)
    assert np.array_equal(out["efc_force"][0], [3, 1]) and out["improvement"][0] == 0 and out["niter"][0] == 0 and out["cost"][0] == 0.5 * (9 + 4) + 1
    assert np.array_equal(out["qfrc_constraint"][0], [3, 2]) and np.array_equal(out["qacc"][0], [3, 2])


def ellipse_problem(bc, mu, fn, A=None):
    """The QCQP alone: ``A_c`` (default ``I``), ``bc``, ``mu`` [2], the normal force."""
    A = np.eye(len(bc)) if A is None else np.asarray(A, dtype=np.float64)
    return np.asarray(A, dtype=LD)[None], np.asarray(bc, dtype=LD)[None], np.asarray(mu, dtype=LD)[None], np.asarray([fn], dtype=LD)


def test_a_qcqp_with_identity_block_is_the_scaled_projection():
    """``A_c = I``: ``v`` minimises ``1/2 |v + bc|^2`` over the ellipse ``sum (v_k / mu_k)^2 <= f_n^2``: the unconstrained minimum ``-bc`` when it lies inside; else
    the point of the ellipse nearest to ``-bc``.  With ``mu = (m, m)`` (a circle of radius ``m f_n``) that is ``-bc`` scaled onto the circle:
    ``v = -bc m f_n / |bc|``.  With ``mu = (2, 1)``, ``f_n = 1`` and ``bc = (-4, 0)`` it is the vertex ``(2, 0)``; in general the nearest point satisfies
    ``v_k = -bc_k mu_k^2 / (mu_k^2 + lambda)`` for the multiplier that puts it on the ellipse, checked here through its stationarity:
    ``(v + bc)_k`` parallel to the ellipse's normal ``v_k / mu_k^2``."""
    v, active, la, bad = nr.qcqp(*ellipse_problem((-0.25, 0.5), (1.0, 1.0), 1.0))
    assert not active[0] and not bad[0] and la[0] == 0 and np.array_equal(v[0], [0.25, -0.5])
    v, active, la, bad = nr.qcqp(*ellipse_problem((-3.0, 4.0), (0.5, 0.5), 2.0))
    assert active[0] and not bad[0] and np.abs(v[0] - np.array([LD(3) / 5, LD(-4) / 5])).max() < 1e-17  # radius 1: -bc / 5
    assert abs(la[0] - (LD(5) - 1) * LD(0.25)) < 1e-16  # (u = -b_s / (mu^2 + lambda), |u| = f_n: lambda = |b_s| / f_n - mu^2 = 1.25 - 0.25)
    v, active, _, _ = nr.qcqp(*ellipse_problem((-4.0, 0.0), (2.0, 1.0), 1.0))
    assert active[0] and np.abs(v[0] - np.array([2, 0])).max() < 1e-17
    bc, mu = np.array([-3.0, -2.0]), np.array([2.0, 1.0])
    v, active, _, _ = nr.qcqp(*ellipse_problem(bc, mu, 1.0))
    g, nrm = f64(v[0]) + bc, f64(v[0]) / mu ** 2
    assert active[0] and abs(((f64(v[0]) / mu) ** 2).sum() - 1) < 1e-15 and abs(g[0] * nrm[1] - g[1] * nrm[0]) < 1e-14 and (g * nrm).sum() < 0
    # the same rules in float32 reach the same point to float32
    A, b, m, r = ellipse_problem(bc, mu, 1.0)
    v32, *_ = nr.qcqp(A.astype(np.float32), b.astype(np.float32), m.astype(np.float32), r.astype(np.float32))
    assert v32.dtype == np.float32 and np.abs(v32[0] - f64(v[0])).max() < 1e-6


def test_a_singular_block_gives_zero():
    """``A_c = [[1, 1], [1, 1]]`` has the pivots 1 and 0: not positive, ``v = 0`` and the constraint counts as inactive; a zero ``mu`` does the same (``A_s`` has a
    zero row), and so does an inactive contact's block ``A_c = 0``.  In a sweep the block then becomes 0 -- unless that raises the cost by more than 1e-10, which
    puts it back."""
    for A, mu in (([[1.0, 1.0], [1.0, 1.0]], (1.0, 1.0)), (np.eye(2), (0.5, 0.0)), (np.zeros((2, 2)), (1.0, 1.0))):
        v, active, la, bad = nr.qcqp(*ellipse_problem((-3.0, 4.0), mu, 2.0, A))
        assert bad[0] and not active[0] and not v.any()
    # an elliptic contact of condim 3 with J rows (normal, t1, t2) = (e0, e1, e1): the friction block is [[1, 1], [1, 1]]
    J = np.array([[[1.0, 0.0], [0.0, 1.0], [0.0, 1.0]]])
    p = dict(J=J, D=np.ones((1, 3)), qLD=np.eye(2)[None], qacc_smooth=np.zeros((1, 2)), fl=np.zeros((1, 3)), mu=np.ones((1, 1, 5)), ne=0, nf=0, con=[(0, 3)],
             elliptic=True, inertia_scale=2.0)
    out = run(dict(p, aref=np.array([[0.0, 5.0, 5.0]]), force0=np.array([[2.0, 0.5, 0.25]])), 1)  # b = (0, -5, -5): zeroing the friction raises the cost: put back
    assert out["status"][0][(0, 0)][0] == nr.DEGENERATE and np.array_equal(out["forces"][1][0], [2, 0.5, 0.25])
    assert out["improvements"][0][0] == (4 + 0.25 + 0.0625) / 4  # (only the regulariser's term, 1/2 sum R f^2, scaled by 1 / 2)
    out = run(dict(p, aref=np.array([[0.0, -5.0, -5.0]]), force0=np.array([[2.0, 0.5, 0.25]])), 1)  # b = (0, 5, 5): zeroing lowers it
    assert np.array_equal(out["forces"][1][0], [2, 0, 0])
    out = run(dict(p, aref=np.array([[0.0, -5.0, -5.0]]), force0=np.array([[0.0, 0.5, 0.25]])), 1)  # no normal force: the friction rows become 0
    assert out["status"][0][(0, 0)][0] == nr.NONE and np.array_equal(out["forces"][1][0], [0, 0, 0])


def test_a_friction_loss_row_and_the_untouched_rows():
    """Rows: 0 equality, 1 friction loss (bound 0.25), 2 a limit row; ``J = I`` (nv = 3), ``qLD = I``: ``A = I``.  From ``f = (7, 0, 3)``, ``b = (1, -2, 1)``: only
    row 1 moves, to ``clamp(0 + 2, +-0.25) = 0.25``: ``res = -2``, ``delta = 0.25``, ``improvement -= 0.25 (0.125 - 2)``: 0.46875 on top of
    ``1/2 (49 + 0 + 9) = 29``; rows 0 and 2 are the start's bits although their own residuals are far from zero."""
    J = np.eye(3)[None]
    out = nr.solve_noslip(J, np.ones((1, 3)), -np.array([[1.0, -2.0, 1.0]]), np.array([[0.0, 0.25, 0.0]]), np.eye(3)[None], np.zeros((1, 3)), np.array([[7.0, 0.0, 3.0]]),
                          np.zeros((1, 0, 5)), 1, 1, [], False, 3.0, 2)
    assert np.array_equal(out["forces"][1][0], [7, 0.25, 3]) and np.array_equal(out["forces"][2][0], [7, 0.25, 3])
    assert abs(out["improvements"][0][0] - (LD(29) + LD(0.46875)) / 3) < 1e-18 and out["improvements"][1][0] == 0 and out["status"][0]["fl"][0, 0] == nr.BOUNDARY


# ---- 2. the plan -----------------------------------------------------------------------------------------------------------------------------

def test_the_plan_is_the_librarys():
    """``solve_pgs``'s staging and arrays plus 22 reals a contact slot: the blocks of ``A`` (15), ``mu`` (5), the table entry (2)."""
    for nv, nefc, ncon, dtype in ((27, 53, 8, F64), (8, 188, 60, F64), (8, 188, 60, F32), (30, 174, 30, F64), (106, 80, 16, F64), (1, 1, 0, F32)):
        size = 8 if dtype == F64 else 4
        chunk, nchunk, last, lds = noslip.plan(nv, nefc, ncon, dtype)
        assert 1 <= last <= chunk and (nchunk - 1) * chunk + last == nefc
        assert chunk == max(1, min(16 * 1024 // ((nv | 1) * size), nefc))
        assert lds == ((nv * (nv + 1) // 2 + nefc * (nv | 1) + 5 * nefc + 2 * nv + 64 + 22 * ncon) * size + 15) // 16 * 16 <= 160 * 1024
    assert noslip.plan(106, 80, 16, F64)[:3] == (19, 5, 4)
    with pytest.raises(RuntimeError, match=r"nv = 154, nefc = 100, ncon = 20 in torch.float64 need 229984 bytes of LDS .* a workgroup has 163840"):
        noslip.plan(154, 100, 20, F64)
    lib = native.load_library()
    out = (ctypes.c_int * 4)()
    assert lib.mjh_noslip_plan(154, 100, 20, 8, out) == -12 and out[3] == 229984 and lib.mjh_noslip_plan(-1, 1, 0, 8, out) == -22
    assert lib.mjh_noslip_plan(1, 1, -1, 8, out) == -22 and lib.mjh_noslip_plan(1, 1, 0, 2, out) == -22


# ---- 3. the public function on a stand-in ----------------------------------------------------------------------------------------------------

class StandIn:
    """``mjh_noslip`` of the CPU stand-in library: the numpy reference, in the model's dtype, on the host pointers it is handed."""

    def __init__(self):
        self.calls = []

    def install(self, monkeypatch):
        _hostsim.install(monkeypatch)
        monkeypatch.setattr(_hostsim._Lib, "mjh_noslip", self, raising=False)
        return self

    def __get__(self, lib, owner=None):
        return lambda *args: self.run(lib, *args)

    def run(self, lib, handle, args, stream):
        a = args._obj
        desc = lib.o.desc
        nv, n, ncon, B = int(desc.nv), int(desc.nefc), int(desc.ncon), int(a.B)
        ct, dt = (ctypes.c_double, np.float64) if lib.o.dt == 0 else (ctypes.c_float, np.float32)
        view = lambda p, count, c=ct: np.ctypeslib.as_array((c * count).from_address(p))
        leaf = lambda name, *shape: view(getattr(a, name), B * int(np.prod(shape))).reshape((B,) + shape)
        put = lambda name, value, c=ct, t=dt: view(getattr(a, name), value.size, c).__setitem__(slice(None), np.asarray(value, dtype=t).reshape(-1))
        self.calls.append(dict(B=B, ne=int(a.ne), nf=int(a.nf), iterations=int(a.iterations), tolerance=float(a.tolerance), meaninertia=float(a.meaninertia),
                               force0=int(a.force0 or 0), force0_env=int(a.force0_env), friction=bool(a.contact_friction)))
        f0 = view(a.force0, (B - 1) * a.force0_env + n)[np.arange(B)[:, None] * a.force0_env + np.arange(n)]
        table = lambda p: np.array((ctypes.c_int32 * ncon).from_address(ctypes.cast(p, ctypes.c_void_p).value)) if ncon else np.zeros(0, dtype=np.int32)
        dims, adr = table(desc.con_dim), table(desc.con_efc_address)
        elliptic = int(desc.cone) == 1
        con = nr.contacts(dims, adr, ncon)
        slots = [i for i, x in enumerate(dims) if x > 1]
        mu = leaf("contact_friction", ncon, 5)[:, slots] if elliptic and ncon else np.ones((B, len(con), 5), dtype=dt)
        out = nr.solve_noslip(leaf("efc_J", n, nv), leaf("efc_D", n), leaf("efc_aref", n), leaf("efc_frictionloss", n), leaf("qLD", nv, nv), leaf("qacc_smooth", nv),
                              f0, mu, int(a.ne), int(a.nf), con, elliptic, a.meaninertia * max(1, nv), int(a.iterations), tolerance=a.tolerance, dtype=dt)
        for name in ("efc_force", "qfrc_constraint", "qacc", "cost", "improvement"):
            put(name, out[name])
        put("niter", out["niter"], ctypes.c_int32, np.int32)
        return 0


@pytest.fixture
def stand_in(monkeypatch):
    return StandIn().install(monkeypatch)


def test_the_function_and_the_entry_point_are_public():
    assert callable(mt.solve_noslip) and mt.NoslipResult._fields == ("efc_force", "qfrc_constraint", "qacc", "cost", "improvement", "niter")
    assert native.ABI_VERSION >= 25
    text = open(native.HEADER).read()
    assert re.search(r"int mjh_noslip\(const mjhModel\* m, const mjhNoslipArgs\* args, void\* hip_stream\);", text)
    assert re.search(r"int mjh_noslip_plan\(int nv, int nefc, int ncon, int real_bytes, int\* chunk_nchunk_last_lds\);", text)
    assert re.search(r"#define MJH_KERNEL_NOSLIP 55\b", text)
    assert list(native.NoslipArgs._fields_) == header_fields(text, "mjhNoslipArgs")
    assert "mjh_noslip" not in native.ARGS  # (bound beside the table, like mjh_pgs)
    lib = native.load_library()
    assert lib.mjh_noslip.argtypes[1]._type_ is native.NoslipArgs and "solve_noslip" in mt.__doc__
    usage = open(native.LIB_PATH.replace("libmjhip.so", "resource_usage.txt")).read().splitlines()
    mine = [ln for ln in usage if "mjh_noslip_kernel" in ln]
    assert len(mine) == 2 and all("ScratchSize [bytes/lane]: 0" in ln for ln in mine)


@pytest.mark.parametrize("xml,ov,dtype", [("ant_frictionloss", {}, F64), ("ant", {"cone": 1}, F32), ("humanoid", {}, F64)], ids=["pyramidal-fl", "elliptic-f32", "humanoid"])
@pytest.mark.parametrize("batch", [(), (3,), (2, 2)], ids=["unbatched", "b3", "b2x2"])
def test_the_function_returns_the_reference(stand_in, batch, xml, ov, dtype):
    mx, d = forwarded(xml, dtype, batch, ov)
    ne, nf, nefc, nv, scale, ncon = sizes(mx)
    B = int(np.prod(batch)) if batch else 1
    before = {n: getattr(d, n).clone() for n in ("efc_J", "efc_D", "efc_aref", "efc_frictionloss", "qLD", "qacc_smooth", "efc_force", "qacc")}
    res = mt.solve_noslip(mx, d, iterations=3)
    assert isinstance(res, mt.NoslipResult)
    c = stand_in.calls[-1]
    assert {k: c[k] for k in ("B", "ne", "nf", "iterations", "tolerance", "meaninertia", "force0_env", "friction")} == dict(
        B=B, ne=ne, nf=nf, iterations=3, tolerance=1e-6, meaninertia=float(mx.stat.meaninertia), force0_env=nefc if batch else 0, friction=bool(ov))
    assert c["force0"] == d.efc_force.data_ptr()  # the default start is the pass's own force
    shapes = dict(efc_force=batch + (nefc,), qfrc_constraint=batch + (nv,), qacc=batch + (nv,), cost=batch, improvement=batch, niter=batch)
    for n, s in shapes.items():
        got = getattr(res, n)
        assert tuple(got.shape) == s and got.dtype == (torch.int32 if n == "niter" else dtype), n
    assert all(torch.equal(getattr(d, n), t) for n, t in before.items())  # nothing is written to d
    rng = np.random.RandomState(2)
    per_env, shared = torch.tensor(rng.randn(*(batch + (nefc,))) * 50, dtype=dtype).abs(), torch.tensor(rng.randn(nefc) * 50, dtype=dtype).abs()
    for f0, stride in ((per_env, nefc if batch else 0), (shared, 0)):
        res = mt.solve_noslip(mx, d, iterations=2, tolerance=0.0, force0=f0)
        c = stand_in.calls[-1]
        assert (c["iterations"], c["tolerance"], c["force0"], c["force0_env"]) == (2, 0.0, f0.data_ptr(), stride)
        assert (res.niter == 2).all() and torch.isfinite(res.efc_force).all()
    zero = mt.solve_noslip(mx, d, iterations=0, force0=per_env)
    assert stand_in.calls[-1]["iterations"] == 0 and not zero.niter.any() and not zero.improvement.any() and torch.equal(zero.efc_force, per_env)


def test_iterations_default_to_the_models_option_or_must_be_given(stand_in):
    """``iterations=None``: ``m.opt.noslip_iterations`` where the Model's options carry it; this library's ``Option`` does not, so the call is a ``ValueError``
    that says so -- and an options object that does carry it is used."""
    mx, d = forwarded("ant_frictionloss", F64, (2,))
    n0 = len(stand_in.calls)
    assert not hasattr(mx.opt, "noslip_iterations")
    with pytest.raises(ValueError, match="iterations must be given: .* no noslip_iterations"):
        mt.solve_noslip(mx, d)
    assert len(stand_in.calls) == n0

    class Opt:
        def __init__(self, opt):
            self._opt = opt
            self.noslip_iterations = 4

        def __getattr__(self, n):
            return getattr(self._opt, n)

    class Model:
        def __init__(self, m):
            self._m = m
            self.opt = Opt(m.opt)

        def __getattr__(self, n):
            return getattr(self._m, n)

    res = mt.solve_noslip(Model(mx), d, tolerance=0.0)
    assert stand_in.calls[-1]["iterations"] == 4 and (res.niter == 4).all()


def test_empty_cases_are_answered_on_the_host(stand_in):
    mx, d = forwarded("ant_frictionloss", F64, (3,))
    ne, nf, nefc, nv, _, _ = sizes(mx)
    n0 = len(stand_in.calls)
    res = mt.solve_noslip(mx, d[:0], iterations=2)
    assert tuple(res.efc_force.shape) == (0, nefc) and tuple(res.qacc.shape) == (0, nv) and tuple(res.cost.shape) == (0,) and res.niter.dtype == torch.int32
    mx, d = forwarded("humanoid", F64, (3,), {"disableflags": 1})
    assert sizes(mx)[2] == 0
    res = mt.solve_noslip(mx, d, iterations=2, force0=torch.zeros(3, 0, dtype=F64))
    assert tuple(res.efc_force.shape) == (3, 0) and tuple(res.qfrc_constraint.shape) == (3, int(mx.nv)) and not res.qfrc_constraint.any()
    assert torch.equal(res.qacc, d.qacc_smooth) and not res.cost.any() and not res.improvement.any() and not res.niter.any()
    assert len(stand_in.calls) == n0


def test_refusals_come_before_any_call(stand_in):
    mx, d = forwarded("ant_frictionloss", F64, (3,))
    ne, nf, nefc, nv, _, _ = sizes(mx)
    n0 = len(stand_in.calls)
    f = torch.zeros(3, nefc, dtype=F64)
    go = lambda *a, **k: mt.solve_noslip(*a, **dict(dict(iterations=2), **k))
    bad = [
        (ValueError, "force0= must have shape", lambda: go(mx, d, force0=torch.zeros(2, nefc, dtype=F64))),
        (ValueError, "force0= must have shape", lambda: go(mx, d, force0=torch.zeros(3, nefc + 1, dtype=F64))),
        (ValueError, "force0= must have shape", lambda: go(mx, d, force0=[0.0] * nefc)),
        (ValueError, "force0= is torch.float32", lambda: go(mx, d, force0=f.float())),
        (ValueError, "iterations must be an integer >= 0", lambda: go(mx, d, iterations=-1)),
        (ValueError, "iterations must be an integer >= 0", lambda: go(mx, d, iterations=2.5)),
        (ValueError, "tolerance must be >= 0", lambda: go(mx, d, tolerance=-1e-9)),
        (ValueError, "tolerance must be >= 0", lambda: go(mx, d, tolerance=float("nan"))),
        (ValueError, "efc_J has shape", lambda: go(mx, d.replace(efc_J=d.efc_J[:, :-1]))),
        (ValueError, "efc_D", lambda: go(mx, d.replace(efc_D=d.efc_D[:1]))),
        (ValueError, "efc_force", lambda: go(mx, d.replace(efc_force=d.efc_force[:, :-1]))),
        (ValueError, "qLD", lambda: go(mx, d.replace(qLD=d.qLD.float()))),
        (ValueError, "dtype|float32", lambda: go(mx, d.to(F32))),
        (NotImplementedError, "solve_noslip cannot be used under torch.vmap", lambda: torch.vmap(lambda x: go(mx, d, force0=x).cost)(torch.zeros(2, 3, nefc, dtype=F64))),
    ]
    for exc, match, fn in bad:
        with pytest.raises(exc, match=match):
            fn()
    with pytest.raises(Exception, match="solve_noslip cannot be used under torch.vmap / torch.compile"):
        torch.compile(lambda x: go(mx, d, force0=x).cost, backend="eager", fullgraph=True)(f)
    me, de = forwarded("ant", F64, (2,), {"cone": 1})
    with pytest.raises(ValueError, match="contact_friction"):
        go(me, de.replace(contact=de.contact.replace(friction=de.contact.friction[:, :-1])))
    assert len(stand_in.calls) == n0


def test_without_the_stand_in_cpu_data_is_refused(monkeypatch):
    _hostsim.install(monkeypatch)
    mx, d = forwarded("ant_frictionloss", F64, (2,))
    monkeypatch.undo()
    with pytest.raises(RuntimeError, match="HIP device"):
        mt.solve_noslip(mx, d, iterations=1)


def test_a_library_from_before_the_function_is_named(monkeypatch):
    _hostsim.install(monkeypatch)  # (its library has no mjh_noslip)
    mx, d = forwarded("ant_frictionloss", F64, (2,))
    with pytest.raises(RuntimeError, match=r"predates solve_noslip \(no mjh_noslip\): rebuild the library"):
        mt.solve_noslip(mx, d, iterations=1)
