"""``ik_site`` without a GPU: the longdouble reference of one iteration (tests/_ik_ref.py) pinned on its normal equations and on the Jacobian reference, the
committed targets (tests/_ik_cases.py) chosen and checked, and the host loop driven on CPU stand-ins -- the oracle's forward pass for the kinematics
(tests/_hostsim.py) and the reference iteration for ``mjh_ik_site_step``.  tests/test_ik.py runs the kernel."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import _hostsim
import _ik_cases as ic
import _ik_ref as ir
import _jacobian_ref as jr
import mujoco_torch_amd as mt
from _cases import F32, F64
from mujoco_torch_amd import native

LD = ir.LD


# ---- 1. the reference -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", list(ic.CASES))
def test_the_reference_iteration_solves_its_normal_equations_on_the_reference_jacobian(case):
    """At the first iteration of every case: J equals what tests/_jacobian_ref.py gives for the site (selected columns; the others are zero), and the update
    satisfies (J^T J + damping I) delta = J^T e to longdouble rounding (the dual form the iteration solves gives the same delta)."""
    t = ic.targets(case, "f64")
    mx = ic.model()
    T = ir.tables(mx, t["site"], t["joints"])
    leaves = ic.kinematics(mx)(t["qpos0"])
    B = t["qpos0"].shape[0]
    r = ir.iteration(T, leaves, t["qpos0"], t["target_pos"], t["target_quat"], max_update_norm=1e30, **t["kw"])
    L = {n: np.zeros((B, 1)) for n in jr.LEAVES}
    L.update(cdof=leaves["cdof"].reshape(B, -1, 6), subtree_com=leaves["subtree_com"].reshape(B, -1, 3))
    (jp, _, _), (jrot, _, _) = jr.point_hp(jr.tables(mx), L, leaves["site_xpos"].reshape(B, -1, 3)[:, t["site"]], [T["body"]])
    rows = ([jp[:, 0]] if t["target_pos"] is not None else []) + ([jrot[:, 0]] if t["target_quat"] is not None else [])
    want = np.swapaxes(np.concatenate(rows, -1), -1, -2) * T["sel"].astype(LD)
    assert np.abs(r["J"] - want).max() <= 4 * np.finfo(LD).eps * max(1, float(np.abs(want).max()))
    assert np.abs(r["J"][:, :, ~T["sel"]]).max(initial=0) == 0 and np.abs(r["J"]).max() > 0.05
    lam = LD(t["kw"].get("damping", 1e-6))
    J, nv = r["J"], want.shape[-1]
    lhs = (np.swapaxes(J, -1, -2) @ J + lam * np.eye(nv, dtype=LD)) @ r["delta"][..., None]
    rhs = np.swapaxes(J, -1, -2) @ r["e"][..., None]
    # conditioning: the dual system's is at most (|J|^2 + damping) / damping
    scale = float(np.abs(rhs).max()) * float((np.abs(J) ** 2).sum() / B / lam + 1)
    assert np.abs(lhs - rhs).max() <= 64 * np.finfo(LD).eps * scale, (float(np.abs(lhs - rhs).max()), scale)
    assert np.abs(r["delta"][:, ~T["sel"]]).max(initial=0) == 0


def test_the_reference_rotation_vector():
    rng = np.random.RandomState(0)
    for ang in (0.0, 1e-9, 0.3, 2.0, np.pi - 1e-6):
        axis = rng.randn(5, 3)
        axis /= np.linalg.norm(axis, axis=-1, keepdims=True)
        q = np.concatenate([np.full((5, 1), np.cos(LD(ang) / 2)), axis.astype(LD) * np.sin(LD(ang) / 2)], -1)
        got = ir.rotvec(ir.quat_to_mat(q))
        assert np.abs(got - axis.astype(LD) * LD(ang)).max() < 1e-12, ang


@pytest.mark.parametrize("key", ["f64", "f32"])
def test_the_committed_targets_converge_and_are_clear(key):
    """On every committed target the reference loop converges within max_steps = 20; at least 90 % of them are clear (tests/_ik_cases.py)."""
    n = clear = 0
    for case in ic.CASES:
        r = ic.reference(case, key)
        print(f"{key} {case}: reference steps {r['steps'].tolist()}, clear {r['clear'].astype(int).tolist()}, worst err_norm {float(r['err_norm'].max()):.2e}")
        assert r["success"].all() and (r["steps"] <= ic.MAX_STEPS).all() and (r["steps"] > 0).all(), case
        assert (r["err_norm"] < ic.TOL[key]).all()
        n, clear = n + r["steps"].size, clear + int(r["clear"].sum())
    print(f"{key}: {clear} of {n} targets clear")
    assert clear >= 0.9 * n


# ---- 2. the host API on stand-ins ------------------------------------------------------------------------------------------------------------------

class StandIn:
    """``mjh_ik_site_step`` of the CPU stand-in library: the reference iteration on the host pointers it is handed."""

    def __init__(self):
        self.calls = []

    def install(self, monkeypatch):
        _hostsim.install(monkeypatch)
        monkeypatch.setattr(_hostsim._Lib, "mjh_ik_site_step", self, raising=False)
        return self

    def __get__(self, lib, owner=None):
        return lambda *args: self.run(lib, *args)

    def run(self, lib, handle, cdof, com, sx, sm, site, body, tp, tps, tq, tqs, sel, params, last, qpos, err, steps, done, B, stream):
        d = lib.o.desc
        nq, nv, nb, ns = int(d.nq), int(d.nv), int(d.nbody), int(d.nsite)
        ct, npdt = (ctypes.c_double, np.float64) if lib.o.dt == 0 else (ctypes.c_float, np.float32)
        view = lambda p, n, c=ct: np.ctypeslib.as_array((c * n).from_address(p.value))
        mx = ic.model()
        selv = view(sel, nv, ctypes.c_int32).astype(bool)
        T = ir.tables(mx, site, None)
        assert T["body"] == body
        T["sel"] = selv
        T["moved"] = [bool(selv[da]) for t, qa, da in T["J"][0]]
        tol, damping, mun, rw = (params[i] for i in range(4))
        self.calls.append(dict(site=site, B=B, last=last, params=(tol, damping, mun, rw), sel=selv.copy(), pos_stride=tps, quat_stride=tqs,
                               has_pos=tp.value is not None, has_quat=tq.value is not None))
        leaves = dict(cdof=view(cdof, B * nv * 6).reshape(B, nv * 6), subtree_com=view(com, B * nb * 3), site_xpos=view(sx, B * ns * 3), site_xmat=view(sm, B * ns * 9))
        tgt = lambda p, n, stride: None if p.value is None else (view(p, n * B).reshape(B, n) if stride else view(p, n))
        q, dn, st, er = view(qpos, B * nq).reshape(B, nq), view(done, B, ctypes.c_uint8), view(steps, B, ctypes.c_int32), view(err, B)
        r = ir.iteration(T, leaves, q, tgt(tp, 3, tps), tgt(tq, 4, tqs), tol=tol, damping=damping, max_update_norm=mun, rot_weight=rw)
        live = dn == 0
        er[live] = r["err_norm"].astype(npdt)[live]
        dn[live & r["done"]] = 1
        go = live & ~r["done"] & (last == 0)
        q[go] = r["qpos"].astype(npdt)[go]
        st[go] += 1
        return 0


@pytest.fixture
def stand_in(monkeypatch):
    return StandIn().install(monkeypatch)


def _call(case, key, dtype=F64, **kw):
    t = ic.targets(case, key)
    mx = ic.model(dtype)
    B = t["qpos0"].shape[0]
    d = mt.make_data(mx)
    d = (d if dtype == F64 else d.to(dtype)).expand(B).clone()
    tens = lambda a: None if a is None else torch.tensor(a).to(dtype)
    args = dict(joints=t["joints"], tol=ic.TOL[key], max_steps=ic.MAX_STEPS, **t["kw"])
    args.update(kw)
    return mt.ik_site(mx, d, t["site"], tens(t["target_pos"]), tens(t["target_quat"]), **args), d, mx


def test_the_function_and_the_entry_point_are_public():
    assert callable(mt.ik_site) and mt.IKResult._fields == ("qpos", "err_norm", "steps", "success") and native.ABI_VERSION >= 22
    p = inspect.signature(mt.ik_site).parameters
    assert list(p) == ["m", "d", "site_id", "target_pos", "target_quat", "joints", "tol", "max_steps", "damping", "max_update_norm", "rot_weight"]
    assert [p[n].default for n in list(p)[3:]] == [None, None, None, None, 20, 1e-6, 2.0, 1.0] and p["joints"].kind == p["joints"].KEYWORD_ONLY
    text = open(native.HEADER).read()
    assert re.search(r"\bint mjh_ik_site_step\s*\(const mjhModel\* m, const void\* cdof, const void\* subtree_com, const void\* site_xpos, const void\* site_xmat, int site,"
                     r" int body,\s*const void\* target_pos, int64_t pos_stride, const void\* target_quat, int64_t quat_stride, const int32_t\* dof_sel,"
                     r" const double\* params,\s*int last, void\* qpos, void\* err_norm, int32_t\* steps, unsigned char\* done, int64_t B, void\* hip_stream\);", text)
    assert re.search(r"#define MJH_KERNEL_IK_SITE 49\b", text)
    assert len(native.ARGS) == 6 and "mjh_ik_site_step" not in native.ARGS


def test_the_library_has_both_entry_points_without_scratch():
    """The built library exports the two entry points, refuses a null model with -22 and a message, and the build's register report shows no scratch in
    any of the eight new kernel instantiations."""
    lib = native.load_library()
    assert hasattr(lib, "mjh_qpos_arith") and hasattr(lib, "mjh_ik_site_step")
    assert lib.mjh_qpos_arith(None, 0, None, None, 0.0, None, 0, None) == -22 and b"null" in lib.mjh_last_error()
    assert lib.mjh_ik_site_step(None, None, None, None, None, 0, 0, None, 0, None, 0, None, None, 0, None, None, None, None, 0, None) == -22
    usage = open(os.path.join(os.path.dirname(native.LIB_PATH), "resource_usage.txt")).read().splitlines()
    mine = [ln for ln in usage if "mjh_qpos_arith_kernel" in ln or "mjh_ik_site_kernel" in ln]
    assert len(mine) == 8 and all("ScratchSize [bytes/lane]: 0" in ln for ln in mine)


@pytest.mark.parametrize("case", ["tip_both", "tip_both_subset", "probe_both", "tip_pos", "tip_quat"])
def test_the_host_loop_reproduces_the_reference_loop(stand_in, case):
    """max_steps + 1 passes and calls, the last one flagged; the results are those of the reference loop (the stand-in rounds qpos to float64 between
    iterations, the reference loop does not: the step counts agree on the clear targets, the configurations to 1e-9)."""
    res, d, mx = _call(case, "f64")
    ref = ic.reference(case, "f64")
    t = ic.targets(case, "f64")
    B = t["qpos0"].shape[0]
    assert len(stand_in.calls) == ic.MAX_STEPS + 1 and [c["last"] for c in stand_in.calls] == [0] * ic.MAX_STEPS + [1]
    c = stand_in.calls[0]
    assert c["has_pos"] == (t["target_pos"] is not None) and c["has_quat"] == (t["target_quat"] is not None) and c["B"] == B
    assert c["pos_stride"] == (3 if c["has_pos"] else 0) and c["quat_stride"] == (4 if c["has_quat"] else 0)
    assert np.array_equal(c["sel"], ir.tables(mx, t["site"], t["joints"])["sel"])
    assert res.success.all() and res.success.dtype == torch.bool and res.steps.dtype == torch.int32 and tuple(res.qpos.shape) == (B, int(mx.nq))
    clear = ref["clear"]
    assert np.array_equal(res.steps.numpy()[clear], ref["steps"][clear])
    assert np.abs(res.qpos.numpy()[clear] - np.asarray(ref["qpos"], dtype=np.float64)[clear]).max() < 1e-9
    assert (res.err_norm.numpy() < 1e-9).all()
    moved = np.zeros(int(mx.nq), dtype=bool)
    for (ty, qa, da), m in zip(ir.tables(mx, t["site"], t["joints"])["J"][0], ir.tables(mx, t["site"], t["joints"])["moved"]):
        moved[qa:qa + {0: 7, 1: 4}.get(ty, 1)] = m
    assert torch.equal(res.qpos[:, ~moved], d.qpos[:, ~moved]) and torch.equal(d.qpos, torch.tensor(t["qpos0"]))  # (nothing is written to d)


def test_shared_targets_batch_shapes_and_max_steps_zero(stand_in):
    mx = ic.model()
    t = ic.targets("tip_both", "f64")
    d = mt.make_data(mx).expand(2, 3).clone()
    tp, tq = torch.tensor(t["target_pos"][0]), torch.tensor(t["target_quat"][0])
    res = mt.ik_site(mx, d, 0, tp, tq)
    assert tuple(res.qpos.shape) == (2, 3, int(mx.nq)) and tuple(res.err_norm.shape) == tuple(res.steps.shape) == tuple(res.success.shape) == (2, 3)
    assert stand_in.calls[0]["pos_stride"] == stand_in.calls[0]["quat_stride"] == 0 and stand_in.calls[0]["params"] == (1e-9, 1e-6, 2.0, 1.0)
    assert res.success.all() and (res.steps == int(ic.reference("tip_both", "f64")["steps"][0])).all()
    assert all(torch.equal(res.qpos[i, j], res.qpos[0, 0]) for i in range(2) for j in range(3))
    one = mt.ik_site(mx, mt.make_data(mx), 0, tp, tq)  # an unbatched Data
    assert tuple(one.qpos.shape) == (int(mx.nq),) and one.success.shape == () and torch.equal(one.qpos, res.qpos[0, 0])
    n = len(stand_in.calls)
    zero = mt.ik_site(mx, d, 0, tp, max_steps=0)
    assert len(stand_in.calls) == n + 1 and stand_in.calls[-1]["last"] == 1 and not stand_in.calls[-1]["has_quat"]
    assert not zero.success.any() and (zero.steps == 0).all() and torch.equal(zero.qpos, d.qpos) and (zero.err_norm > 0.1).all()
    n = len(stand_in.calls)
    w = mt.ik_site(mx, d, 0, tp, tq, max_steps=0, rot_weight=0.25, damping=1e-3, max_update_norm=0.5, tol=1e-3)
    assert stand_in.calls[n]["params"] == (1e-3, 1e-3, 0.5, 0.25)
    only = [mt.ik_site(mx, d, 0, a, b, max_steps=0).err_norm for a, b in ((tp, None), (None, tq))]
    assert torch.allclose(w.err_norm, only[0] + 0.25 * only[1], rtol=0, atol=1e-14)  # (rot_weight scales the orientation part of the error)
    f32 = mt.ik_site(ic.model(F32), mt.make_data(ic.model(F32)).to(F32).expand(2).clone(), 0, tp.float())
    assert stand_in.calls[-1]["params"][0] == 2e-4 and f32.qpos.dtype == F32 and f32.success.all()


def test_refusals_come_before_any_call(stand_in):
    mx = ic.model()
    d = mt.make_data(mx).expand(3).clone()
    tp, tq = torch.zeros(3, dtype=F64), torch.tensor([1.0, 0, 0, 0], dtype=F64)
    ns, nj = int(mx.nsite), int(mx.njnt)
    bad = [
        (ValueError, "neither target", lambda: mt.ik_site(mx, d, 0)),
        (ValueError, "target_pos must be a tensor of shape", lambda: mt.ik_site(mx, d, 0, torch.zeros(2, 3, dtype=F64))),
        (ValueError, "target_pos must be a tensor of shape", lambda: mt.ik_site(mx, d, 0, [0.0, 0.0, 0.0])),
        (ValueError, "target_quat must be a tensor of shape", lambda: mt.ik_site(mx, d, 0, tp, torch.zeros(3, 3, dtype=F64))),
        (ValueError, "target_pos= is torch.float32", lambda: mt.ik_site(mx, d, 0, tp.float())),
        (ValueError, "target_quat= is torch.float32", lambda: mt.ik_site(mx, d, 0, tp, tq.float())),
        (ValueError, "target_pos= is torch.float64 on meta", lambda: mt.ik_site(mx, d, 0, tp.to("meta"))),
        (ValueError, "qpos has shape", lambda: mt.ik_site(mx, d.replace(qpos=d.qpos[:, :-1]), 0, tp)),
        (ValueError, "runs in the model's dtype", lambda: mt.ik_site(mx, d.replace(qpos=d.qpos.float()), 0, tp.float())),
        (ValueError, "shared by every environment", lambda: mt.ik_site(mx, d, torch.zeros(3, dtype=torch.int64), tp)),
        (ValueError, "shared by every environment", lambda: mt.ik_site(mx, d, [0, 0, 0], tp)),
        (ValueError, "one integer site id", lambda: mt.ik_site(mx, d, 0.0, tp)),
        (ValueError, f"site id {ns}", lambda: mt.ik_site(mx, d, ns, tp)),
        (ValueError, "site id -1", lambda: mt.ik_site(mx, d, -1, tp)),
        (ValueError, "shared by every environment", lambda: mt.ik_site(mx, d, 0, tp, joints=[[0, 1], [0, 1], [0, 1]])),
        (ValueError, "shared by every environment", lambda: mt.ik_site(mx, d, 0, tp, joints=torch.zeros((3, 2), dtype=torch.int64))),
        (ValueError, "integer joint ids", lambda: mt.ik_site(mx, d, 0, tp, joints=torch.tensor([0.0, 1.0]))),
        (ValueError, "integer joint ids", lambda: mt.ik_site(mx, d, 0, tp, joints=[0.5])),
        (ValueError, f"joint id {nj}", lambda: mt.ik_site(mx, d, 0, tp, joints=[0, nj])),
        (ValueError, "joint id -1", lambda: mt.ik_site(mx, d, 0, tp, joints=[-1])),
        (ValueError, "damping must be a finite float > 0", lambda: mt.ik_site(mx, d, 0, tp, damping=0.0)),
        (ValueError, "damping must be a finite float > 0", lambda: mt.ik_site(mx, d, 0, tp, damping=-1e-6)),
        (ValueError, "damping", lambda: mt.ik_site(mx, d, 0, tp, damping=float("nan"))),
        (ValueError, "max_steps must be an integer >= 0", lambda: mt.ik_site(mx, d, 0, tp, max_steps=-1)),
        (ValueError, "max_steps must be an integer >= 0", lambda: mt.ik_site(mx, d, 0, tp, max_steps=2.5)),
        (ValueError, "tol must be", lambda: mt.ik_site(mx, d, 0, tp, tol=-1.0)),
        (ValueError, "max_update_norm must be", lambda: mt.ik_site(mx, d, 0, tp, max_update_norm=None)),
        (ValueError, "rot_weight must be", lambda: mt.ik_site(mx, d, 0, tp, rot_weight=-2.0)),
        (NotImplementedError, "ik_site cannot be used under torch.vmap", lambda: torch.vmap(lambda q: mt.ik_site(mx, d.replace(qpos=q), 0, tp).qpos)(d.qpos[None])),
        (NotImplementedError, "ik_site cannot be used under torch.vmap", lambda: torch.vmap(lambda t: mt.ik_site(mx, d, 0, t).qpos)(torch.zeros(2, 3, dtype=F64))),
    ]
    for exc, match, run in bad:
        with pytest.raises(exc, match=match):
            run()
    with pytest.raises(Exception, match="ik_site cannot be used under torch.vmap / torch.compile"):
        torch.compile(lambda t: mt.ik_site(mx, d, 0, t).qpos, backend="eager", fullgraph=True)(tp)
    assert not stand_in.calls


def test_without_the_stand_in_cpu_data_is_refused():
    mx = ic.model()
    with pytest.raises(RuntimeError, match="HIP device"):
        mt.ik_site(mx, mt.make_data(mx), 0, torch.zeros(3, dtype=F64))


def test_an_empty_batch_returns_without_a_call(stand_in):
    mx = ic.model()
    res = mt.ik_site(mx, mt.make_data(mx).expand(0).clone(), 0, torch.zeros(3, dtype=F64))
    assert tuple(res.qpos.shape) == (0, int(mx.nq)) and tuple(res.success.shape) == (0,) and not stand_in.calls
