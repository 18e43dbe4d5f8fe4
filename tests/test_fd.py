"""transition_fd on the device against the host composition: tests/_fd_ref.py around the library's own ``step``.

The yardstick of tests 1-3 uses the same step kernel on host-built perturbed inputs, so the solver's own tolerance cancels and only the two new
kernels are judged.  That needs ``step`` not to depend on where in a batch an environment sits, or how large the batch is:
``test_step_does_not_depend_on_placement`` establishes it (one environment replicated at batch sizes 1 .. 150: bit-identical next states, sensors
included; the stepping kernels are those of the parent commit, byte for byte in lib/resource_usage.txt).  Measured placement spread on an MI355X: 0 in all five models.  Hence:

* entries whose row and column are add / subtract quantities (slide / hinge / free-translation dofs, qvel, act, ctrl, sensordata): EXACT equality;
* rows that are rotational dofs of ball / free joints: ``_fd_ref.bound`` (two correct evaluations of the rotation vector of q0^-1 q1);
* columns that are such dofs: ``_fd_ref.column_bound`` (the two perturbed quaternions differ by roundings, which the step carries to every output
  with the yardstick's own derivative); an entry in both gets the sum.
"""
import math

import numpy as np
import pytest
import torch

import _fd_ref as R
import mujoco_torch_amd as mt
from _cases import seeded_batch
from _util import INT_LEAVES, REAL_LEAVES, leaf
from mujoco_torch_amd import derivative

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
MACH = {F64: 2.0 ** -52, F32: 2.0 ** -23}
CASES = [("cartpole", F64, 64), ("ball_free_actuators", F64, 32), ("muscle_arm", F64, 64), ("ant", F64, 32), ("ant", F32, 32), ("humanoid", F64, 16),
         ("sensor_rig", F64, 16)]  # (sensor_rig: a free joint WITH sensors, so that C's quaternion columns are covered too)


def joints(mx):
    return R.Joints(mx.jnt_type.data.cpu().numpy(), np.asarray(mx.jnt_qposadr), np.asarray(mx.jnt_dofadr), int(mx.nq), int(mx.nv))


def on_gpu(xml, dtype, B, overrides=None):
    mx, d = seeded_batch(xml, overrides or {}, dtype, B)
    return mx, mx.to("cuda"), d.to("cuda")


def state(y, sensors):
    names = ("qpos", "qvel", "act") + (("sensordata",) if sensors else ())
    return {n: getattr(y, n).detach().cpu().numpy() for n in names}


def composition(mx, mg, dg, eps, centered, sensors, fixed_iterations=False, stepper=None):
    """A, B (C, D) by _fd_ref around ``step`` (one call over all perturbed environments); also the perturbed inputs and the control flags."""
    jt = joints(mx)
    B = dg.qpos.shape[0]
    np_ = lambda t: t.detach().cpu().numpy()
    P, sides = R.perturbed(jt, np_(dg.qpos), np_(dg.qvel), np_(dg.act), np_(dg.ctrl), eps, centered, np.asarray(mx.actuator_ctrllimited),
                           np.asarray(mx.actuator_ctrlrange).reshape(-1, 2))
    ncol, nside = P["qpos"].shape[1:3]
    rep = dg[torch.arange(B).repeat_interleave(ncol * nside)]
    rep = rep.replace(**{k: torch.tensor(v.reshape(B * ncol * nside, v.shape[-1]), device=dg.qpos.device) for k, v in P.items()})
    step = stepper or (lambda d: mt.step(mg, d, fixed_iterations))
    y0, y = state(step(dg), sensors), state(step(rep), sensors)
    y = {k: v.reshape(B, ncol, nside, v.shape[-1]) for k, v in y.items()}
    return R.jacobians(jt, y0, y, eps, centered, sides, sensors), rep, sides


def tolerances(jt, ref, dtype, eps):
    """Per entry of each of A, B, C, D: 0, or the derived bound of the module docstring."""
    out = []
    for k, J in enumerate(ref):
        tol = np.zeros(J.shape)
        if k in (0, 1) and len(jt.rot_dofs):  # rows of A, B
            tol[:, jt.rot_dofs, :] += R.bound(MACH[dtype], eps)
        if k in (0, 2):                       # columns of A, C
            for _, da in jt.quats:
                tol[:, :, da:da + 3] += R.column_bound(MACH[dtype], eps, J[:, :, da:da + 3])[:, :, None]
        out.append(tol)
    return out


def compare(what, got, ref, tol):
    for name, g, r, t in zip("ABCD", got, ref, tol):
        g = g.detach().cpu().numpy()
        assert g.shape == r.shape, (what, name, g.shape, r.shape)
        err = np.abs(g - r)
        exact = t == 0
        print(f"{what} {name}{g.shape}: max |entry| {np.abs(r).max() if r.size else 0:.3e}; exact entries: {int(exact.sum())}, worst deviation "
              f"{err[exact].max() if exact.any() else 0:.3e}; bounded entries: {int((~exact).sum())}, worst deviation / bound "
              f"{(err[~exact] / t[~exact]).max() if (~exact).any() else 0:.3e}")
        assert np.isfinite(g).all(), (what, name)
        assert (err[exact] == 0).all(), (what, name, "add / subtract entries must be bit-identical", float(err[exact].max()))
        assert (err[~exact] <= t[~exact]).all(), (what, name, float((err[~exact] / t[~exact]).max()))


@pytest.mark.parametrize("xml", ["cartpole", "ant", "humanoid", "ball_free_actuators", "sensor_rig"])
def test_step_does_not_depend_on_placement(xml):
    mx, mg, dg = on_gpu(xml, F64, 4)
    one = dg[torch.tensor([2])]
    want = state(mt.step(mg, one), int(getattr(mx, "nsensordata", 0) or 0) > 0)
    for B in (2, 7, 64, 150):
        got = state(mt.step(mg, dg[torch.full((B,), 2)]), "sensordata" in want)
        for k, v in want.items():
            assert (got[k] == v).all(), (xml, B, k, float(np.abs(got[k] - v).max()))


@pytest.mark.parametrize("centered", [False, True], ids=["one-sided", "centered"])
@pytest.mark.parametrize("xml,dtype,B", CASES, ids=[f"{x}-{str(t)[6:]}" for x, t, _ in CASES])
def test_machinery_matches_the_host_composition(xml, dtype, B, centered):
    mx, mg, dg = on_gpu(xml, dtype, B)
    eps = 1e-6 if dtype == F64 else 1e-3  # (float32: an eps its 2^-23 can resolve; the comparison is exact either way)
    got = mt.transition_fd(mg, dg, eps=eps, centered=centered, sensors=True)
    ref, _, _ = composition(mx, mg, dg, eps, centered, True)
    nv, na, nu, nsd = int(mx.nv), int(mx.na), int(mx.nu), int(getattr(mx, "nsensordata", 0) or 0)
    ns = 2 * nv + na
    assert [tuple(g.shape) for g in got] == [(B, ns, ns), (B, ns, nu), (B, nsd, ns), (B, nsd, nu)] and all(g.dtype == dtype for g in got)
    compare(f"{xml} {dtype} centered={centered}", got, ref, tolerances(joints(mx), ref, dtype, eps))
    two = mt.transition_fd(mg, dg, eps=eps, centered=centered)
    assert len(two) == 2 and all(torch.equal(a, b) for a, b in zip(two, got))


def test_unbatched_data_is_the_batch_of_one():
    mx, mg, dg = on_gpu("ball_free_actuators", F64, 3)
    A, Bm = mt.transition_fd(mg, dg)
    a, b = mt.transition_fd(mg, dg[1])
    assert a.shape == A.shape[1:] and b.shape == Bm.shape[1:] and torch.equal(a, A[1]) and torch.equal(b, Bm[1])
    A2, B2 = mt.transition_fd(mg, dg[torch.arange(3).reshape(3, 1)])  # batch shape (3, 1)
    assert A2.shape == (3, 1) + A.shape[1:] and torch.equal(A2[:, 0], A) and torch.equal(B2[:, 0], Bm)


def test_chunking_changes_nothing():
    mx, mg, dg = on_gpu("humanoid", F64, 8)
    ncol = 2 * int(mx.nv) + int(mx.na) + int(mx.nu)
    pool = lambda: list(mg.tables.__dict__["_fd_scratch"].values())[-1]
    for centered in (False, True):
        nside = 2 if centered else 1
        whole = mt.transition_fd(mg, dg, centered=centered, max_scratch_bytes=1 << 40)
        scr = pool()
        assert scr.slots == 8 * ncol * nside  # one chunk
        cut = mt.transition_fd(mg, dg, centered=centered, max_scratch_bytes=scr.slab.numel() * 30 // ncol)
        cols = pool().slots // (8 * nside)
        assert math.ceil(ncol / cols) >= 3 and ncol % cols != 0, (ncol, cols)  # three chunks or more, the last one ragged
        single = mt.transition_fd(mg, dg, centered=centered, max_scratch_bytes=1)  # one column per chunk
        assert pool().slots == 8 * nside
        for a, b, c in zip(whole, cut, single):
            assert torch.equal(a, b) and torch.equal(a, c)


def test_control_rule_on_the_device():
    mx, mg, dg = on_gpu("ant", F64, 30)
    nu, ns = int(mx.nu), 2 * int(mx.nv) + int(mx.na)
    assert np.asarray(mx.actuator_ctrllimited).all() and (np.asarray(mx.actuator_ctrlrange).reshape(-1, 2) == [-1, 1]).all()
    ctrl = dg.ctrl.clone().clamp_(-0.9, 0.9)
    ctrl[1::3] = 1.0    # at the upper bound
    ctrl[2::3] = -1.0   # at the lower bound
    ctrl[3, 0] = 1.0 - 0.5e-6  # inside, but closer to the bound than eps: forward refused
    dg = dg.replace(ctrl=ctrl)
    eps = 1e-6
    for centered in (False, True):
        got = mt.transition_fd(mg, dg, eps=eps, centered=centered, sensors=True)
        ref, rep, (fwd, bwd) = composition(mx, mg, dg, eps, centered, True)
        compare(f"ant ctrl rule centered={centered}", got, ref, tolerances(joints(mx), ref, F64, eps))
        assert fwd[0].all() and (bwd[0] == centered).all() and not fwd[1].any() and bwd[1].all() and fwd[2].all() and not bwd[2].any()
        assert not fwd[3, 0] and bwd[3, 0]
    # one-sided, a control at its upper bound yields the backward difference -- not zero
    Bm = mt.transition_fd(mg, dg, eps=eps)[1].cpu().numpy()
    y0 = state(mt.step(mg, dg), False)
    back = state(mt.step(mg, dg.replace(ctrl=torch.where(torch.arange(nu, device="cuda") == 0, ctrl - eps, ctrl))), False)
    want = np.concatenate([y0["qpos"] - back["qpos"], y0["qvel"] - back["qvel"]], axis=-1) / eps  # (the ant here has slide / hinge joints only)
    assert Bm.shape[1] == ns == want.shape[1]
    assert (Bm[1::3, :, 0] == want[1::3]).all() and np.abs(Bm[1::3, :, 0]).max() > 0


def test_it_is_a_derivative_of_the_oracle_step():
    """Cartpole (no constraint rows, a smooth step): A, B centered at eps = 1e-6 against centered differences of the CPU oracle's step on the same
    perturbed inputs.  Allowed: 4 x the largest elementwise difference between the oracle's and the device's next states on these very inputs,
    over 2 eps (rounding only: nothing iterates).  Measured on an MI355X: spread 4.2e-17, hence allowed 8.3e-11; worst deviation of A, B 2.1e-11."""
    import pyoracle

    mx, mg, dg = on_gpu("cartpole", F64, 64)
    eps = 1e-6
    spread = [0.0]

    def both(d):  # the device's step, and beside it the oracle's on the same inputs
        y = mt.step(mg, d)
        o = pyoracle.run(mx, d.to("cpu"), step=True)
        spread[0] = max([spread[0]] + [float(np.abs(o[k] - getattr(y, k).cpu().numpy()).max()) for k in ("qpos", "qvel")])
        B_ = d.qpos.shape[0]
        return y.replace(qpos=torch.tensor(np.asarray(o["qpos"]).reshape(B_, -1), device="cuda"), qvel=torch.tensor(np.asarray(o["qvel"]).reshape(B_, -1), device="cuda"))

    ref, _, _ = composition(mx, mg, dg, eps, True, False, stepper=both)
    got = mt.transition_fd(mg, dg, eps=eps, centered=True)
    allowed = 4 * spread[0] / (2 * eps)
    worst = max(float(np.abs(g.cpu().numpy() - r).max()) for g, r in zip(got, ref))
    print(f"cartpole: oracle / device step spread on the perturbed inputs {spread[0]:.3e}, allowed {allowed:.3e}, worst deviation of A, B {worst:.3e}")
    assert np.abs(ref[0]).max() > 0.5 and np.abs(ref[1]).max() > 0
    assert worst <= allowed, (worst, allowed, spread[0])


def test_inputs_are_untouched_and_calls_repeat():
    mx, mg, dg = on_gpu("humanoid", F64, 8)
    names = [n for n in REAL_LEAVES + INT_LEAVES if isinstance(leaf(dg, n), torch.Tensor)]
    before = {n: leaf(dg, n).clone() for n in names}
    first = mt.transition_fd(mg, dg, centered=True, sensors=True)
    second = mt.transition_fd(mg, dg, centered=True, sensors=True)
    assert len(names) > 60 and all(torch.equal(leaf(dg, n), before[n]) for n in names)
    assert all(torch.equal(a, b) for a, b in zip(first, second))


def test_large_batch_completes_within_its_scratch():
    mx, mg, dg = on_gpu("humanoid", F64, 4096)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    out = mt.transition_fd(mg, dg, centered=True)  # 150 columns x 4096 environments, default budget
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(o).all()) for o in out)
    scr = list(mg.tables.__dict__["_fd_scratch"].values())[-1]
    assert scr.slab.numel() <= derivative.MAX_SCRATCH_BYTES and scr.slots < 4096 * 150  # chunked
    del out
    warm = torch.cuda.memory_allocated()
    out = mt.transition_fd(mg, dg, centered=True)
    torch.cuda.synchronize()
    del out
    again = torch.cuda.memory_allocated()
    print(f"humanoid B=4096 centered: scratch {scr.slab.numel() / 2**20:.0f} MiB in chunks of {scr.slots // 8192} columns; allocated before {base / 2**20:.0f} MiB, "
          f"after the first call {warm / 2**20:.0f} MiB, after the second {again / 2**20:.0f} MiB")
    assert again <= warm and warm - base <= scr.slab.numel() + (64 << 20)  # nothing but the kept scratch (and the model's device tables) stays


def test_refusals():
    mx, mg, dg = on_gpu("cartpole", F64, 4)
    with pytest.raises(ValueError, match="eps"):
        mt.transition_fd(mg, dg, eps=0)
    with pytest.raises(ValueError, match="float32"):
        mt.transition_fd(mg, dg.to(F32))
    with pytest.raises(NotImplementedError, match="vmap"):
        torch.vmap(lambda q: mt.transition_fd(mg, dg[0].replace(qpos=q))[0])(dg.qpos)
    A, Bm, C, D = mt.transition_fd(mg, dg, sensors=True)  # no sensors: C, D with a zero first dimension
    assert C.shape == (4, 0, 4) and D.shape == (4, 0, 1)


def test_native_refusals_of_the_fd_family():
    """The seven entry points of the finite-difference family, called straight through the bindings with one defect each: the return code and the
    text ``mjh_last_error`` is left with.  Every row is refused, or answered with 0, before anything is launched (all other pointers are real ones
    of a stepped cartpole batch).  Before each row the error text is set to "null argument" by a call without a model: a row that returns 0 leaves
    it there.  The two families order their early returns differently -- ``mjh_ifd_*`` answers ``B == 0`` before it looks at ``eps`` or the
    columns, ``mjh_fd_*`` after -- and the rows with ``B = 0`` and ``eps = 0`` pin that.  The expected values were recorded from the library of the
    commit before the perturb kernels were folded into one."""
    import ctypes
    import sys

    from mujoco_torch_amd import native

    fw = sys.modules["mujoco_torch_amd.forward"]
    B = 2
    mx, mg, dg = on_gpu("cartpole", F64, B)
    _, mg32, _ = on_gpu("cartpole", F32, B)
    dev = dg.qpos.device
    nv, ns, nu = int(mx.nv), 2 * int(mx.nv) + int(mx.na), int(mx.nu)
    assert (nv, ns, nu, int(mx.nq), int(getattr(mx, "nsensordata", 0) or 0)) == (2, 4, 1, 2, 0)
    y0 = mt.step(mg, dg)
    nm, nm32 = native.get_native_model(mg, dev, F64), native.get_native_model(mg32, dev, F32)
    lib = nm.lib
    derivative._bind(lib)
    tab = fw._table(dg, (mg.tables.uid, F64, dev, B), nm.leaf_counts, B, F64, dev)
    leaf_bytes = derivative._leaf_bytes(fw, nm.leaf_counts, F64)
    slots = B * 3 * nv * 2  # room for every column of either family, centered
    out_idx = tuple(fw._IDX[n] for n in fw._written_names(mg, True))
    scratch = lambda names: derivative._make_scratch(fw, tuple(fw._IDX[n] for n in names if tab.arr[fw._IDX[n]] != 0), (), (), out_idx, leaf_bytes, slots, dev)
    scr, iscr = scratch(derivative._INPUT_LEAVES), scratch(derivative._INVERSE_INPUT_LEAVES)
    for s in (scr, iscr):
        s.slab.zero_()
    buf = lambda *shape: torch.zeros(shape, dtype=F64, device=dev)
    bufs = {k: buf(*shape) for k, shape in dict(A=(B, ns, ns), Bm=(B, ns, nu), C=(64,), D=(64,), g=(B, ns), gx=(B, ns), gu=(B, nu), gq=(B, 2), gt=(B, nv), f0=(B, nv),
                                                f=(slots, nv), Dq=(B, nv, nv), Dv=(B, nv, nv), Da=(B, nv, nv), S0=(64,), S1=(64,), S2=(64,)).items()}
    P = {k: ctypes.c_void_p(t.data_ptr()) for k, t in bufs.items()}
    keep = []

    def without(struct, *names):  # the pointer struct with these leaves NULL
        s = native.DataPtrs.from_buffer_copy(struct)
        for n in names:
            setattr(s, n, None)
        keep.append(s)
        return ctypes.byref(s)

    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    h, h32 = nm.handle, nm32.handle
    pin, py0, pout = ctypes.byref(tab.struct), ctypes.byref(y0.__dict__["_ptab"].struct), ctypes.byref(scr.out)
    eps = 1e-6
    ORDER = {"fd_perturb": "m in scratch B col0 ncol eps centered", "fd_difference": "m in nominal stepped B col0 ncol eps centered A Bm C D",
             "fd_vjp": "m in nominal stepped B col0 ncol eps centered g_state g_sens gx gu", "fd_tangent": "m qpos g_in g_out B mode",
             "ifd_perturb": "m in scratch B col0 ncol eps centered",
             "ifd_difference": "m f0 s0 f s B col0 ncol eps centered DfDq DfDv DfDa DsDq DsDv DsDa"}
    common = {"m": h, "in": pin, "B": B, "col0": 0, "ncol": 1, "eps": eps, "centered": 0}
    BASE = {"fd_perturb": dict(common, scratch=ctypes.byref(scr.inp)),
            "fd_difference": dict(common, nominal=py0, stepped=pout, A=P["A"], Bm=P["Bm"], C=None, D=None),
            "fd_vjp": dict(common, nominal=py0, stepped=pout, g_state=P["g"], g_sens=None, gx=P["gx"], gu=P["gu"]),
            "fd_tangent": {"m": h, "qpos": ctypes.c_void_p(dg.qpos.data_ptr()), "g_in": P["gq"], "g_out": P["gt"], "B": B, "mode": 0},
            "ifd_perturb": dict(common, scratch=ctypes.byref(iscr.inp)),
            "ifd_difference": dict(common, f0=P["f0"], s0=None, f=P["f"], s=None, DfDq=P["Dq"], DfDv=P["Dv"], DfDa=P["Da"], DsDq=None, DsDv=None, DsDa=None)}
    NAN, BIG = float("nan"), 1 << 30
    E_B, E_EPS, E_COL, E_CTRL = "fd: B must be >= 0", "fd: eps must be positive in the model's dtype", "fd: columns outside [0, 2 nv + na + nu)", \
        "fd: in.ctrl is required for the ctrl columns"
    I_B, I_EPS, I_COL = "ifd: B must be >= 0", "ifd: eps must be positive in the model's dtype", "ifd: columns outside [0, 3 nv)"
    E_PERT, I_PERT = "fd_perturb: qpos, qvel, act and ctrl are required in both Data", "ifd_perturb: qpos, qvel and qacc are required in both Data"
    E_DIFF = "fd_difference: qpos, qvel, act (and sensordata for C, D) are required in both stepped Data"
    E_VJP = "fd_vjp: qpos, qvel, act (and sensordata with g_sens) are required in both stepped Data"
    I_F = "ifd_difference: qfrc_inverse of the perturbed passes (and, one-sided, of the nominal pass) is required"
    NONE = "null argument"  # (what the priming call leaves: the row left nothing)
    no_ctrl = without(tab.struct, "ctrl")
    ROWS = [
        ("fd_perturb", dict(B=-1), -22, E_B), ("fd_perturb", dict(eps=0.0), -22, E_EPS), ("fd_perturb", dict(eps=NAN), -22, E_EPS),
        ("fd_perturb", dict(m=h32, eps=1e-60), -22, E_EPS), ("fd_perturb", dict(col0=-1), -22, E_COL), ("fd_perturb", dict(ncol=0), -22, E_COL),
        ("fd_perturb", dict(ncol=ns + nu + 1), -22, E_COL), ("fd_perturb", dict(col0=ns + nu, ncol=1), -22, E_COL), ("fd_perturb", dict(ncol=BIG), -22, E_COL),
        ("fd_perturb", {"in": no_ctrl, "col0": ns}, -22, E_CTRL), ("fd_perturb", dict(scratch=without(scr.inp, "qpos")), -22, E_PERT),
        ("fd_perturb", {"in": without(tab.struct, "qvel")}, -22, E_PERT), ("fd_perturb", dict(B=0, eps=0.0), -22, E_EPS), ("fd_perturb", dict(B=0), 0, NONE),
        ("fd_perturb", dict(B=0, scratch=without(scr.inp, "qpos")), 0, NONE),
        ("fd_difference", dict(B=-1), -22, E_B), ("fd_difference", dict(eps=0.0), -22, E_EPS), ("fd_difference", dict(m=h32, eps=1e-60), -22, E_EPS),
        ("fd_difference", dict(col0=-1), -22, E_COL), ("fd_difference", dict(ncol=0), -22, E_COL), ("fd_difference", dict(ncol=ns + nu + 1), -22, E_COL),
        ("fd_difference", dict(ncol=BIG), -22, E_COL), ("fd_difference", {"in": no_ctrl, "col0": ns}, -22, E_CTRL),
        ("fd_difference", dict(C=P["C"]), -22, "fd_difference: C and D go together"), ("fd_difference", dict(D=P["D"]), -22, "fd_difference: C and D go together"),
        ("fd_difference", dict(A=None), -22, "fd_difference: A and Bm are required"), ("fd_difference", dict(Bm=None), -22, "fd_difference: A and Bm are required"),
        ("fd_difference", dict(stepped=without(scr.out, "qpos")), -22, E_DIFF), ("fd_difference", dict(nominal=without(y0.__dict__["_ptab"].struct, "qvel")), -22, E_DIFF),
        ("fd_difference", dict(B=0, eps=0.0), -22, E_EPS), ("fd_difference", dict(B=0), 0, NONE), ("fd_difference", dict(B=0, A=None), 0, NONE),
        ("fd_vjp", dict(B=-1), -22, E_B), ("fd_vjp", dict(eps=NAN), -22, E_EPS), ("fd_vjp", dict(col0=ns + nu, ncol=1), -22, E_COL),
        ("fd_vjp", {"in": no_ctrl, "col0": ns}, -22, E_CTRL), ("fd_vjp", dict(g_state=None), -22, "fd_vjp: g_state, gx and gu are required"),
        ("fd_vjp", dict(gu=None), -22, "fd_vjp: g_state, gx and gu are required"), ("fd_vjp", dict(stepped=without(scr.out, "qvel")), -22, E_VJP),
        ("fd_vjp", dict(B=0, eps=0.0), -22, E_EPS), ("fd_vjp", dict(B=0), 0, NONE), ("fd_vjp", dict(B=0, g_state=None), 0, NONE),
        ("fd_tangent", dict(B=-1), -22, "fd_tangent: B must be >= 0"),
        ("fd_tangent", dict(mode=2), -22, "fd_tangent: mode must be MJH_FD_TANGENT_PULL or MJH_FD_TANGENT_PUSH"),
        ("fd_tangent", dict(B=0, mode=2), -22, "fd_tangent: mode must be MJH_FD_TANGENT_PULL or MJH_FD_TANGENT_PUSH"),
        ("fd_tangent", dict(g_in=None), -22, "fd_tangent: qpos, g_in and g_out are required"), ("fd_tangent", dict(mode=1, qpos=None), -22, "fd_tangent: qpos, g_in and g_out are required"),
        ("fd_tangent", dict(B=0), 0, NONE), ("fd_tangent", dict(B=0, g_out=None), 0, NONE),
        ("ifd_perturb", dict(B=-1), -22, I_B), ("ifd_perturb", dict(eps=0.0), -22, I_EPS), ("ifd_perturb", dict(eps=NAN), -22, I_EPS),
        ("ifd_perturb", dict(m=h32, eps=1e-60), -22, I_EPS), ("ifd_perturb", dict(col0=-1), -22, I_COL), ("ifd_perturb", dict(ncol=0), -22, I_COL),
        ("ifd_perturb", dict(ncol=3 * nv + 1), -22, I_COL), ("ifd_perturb", dict(col0=3 * nv, ncol=1), -22, I_COL), ("ifd_perturb", dict(ncol=BIG), -22, I_COL),
        ("ifd_perturb", dict(scratch=without(iscr.inp, "qpos")), -22, I_PERT), ("ifd_perturb", {"in": without(tab.struct, "qacc")}, -22, I_PERT),
        ("ifd_perturb", dict(B=0, eps=0.0), 0, NONE), ("ifd_perturb", dict(B=0, ncol=0), 0, NONE), ("ifd_perturb", dict(B=0), 0, NONE),
        ("ifd_difference", dict(B=-1), -22, I_B), ("ifd_difference", dict(eps=0.0), -22, I_EPS), ("ifd_difference", dict(m=h32, eps=1e-60), -22, I_EPS),
        ("ifd_difference", dict(col0=-1), -22, I_COL), ("ifd_difference", dict(ncol=0), -22, I_COL), ("ifd_difference", dict(ncol=3 * nv + 1), -22, I_COL),
        ("ifd_difference", dict(ncol=BIG), -22, I_COL),
        ("ifd_difference", dict(DsDq=P["S0"], DsDv=P["S1"]), -22, "ifd_difference: DsDq, DsDv and DsDa go together"),
        ("ifd_difference", dict(DsDa=P["S2"]), -22, "ifd_difference: DsDq, DsDv and DsDa go together"),
        ("ifd_difference", dict(DfDv=None), -22, "ifd_difference: DfDq, DfDv and DfDa are required"), ("ifd_difference", dict(f0=None), -22, I_F),
        ("ifd_difference", dict(f=None, centered=1), -22, I_F), ("ifd_difference", dict(B=0, eps=0.0), 0, NONE), ("ifd_difference", dict(B=0, col0=-1), 0, NONE),
        ("ifd_difference", dict(B=0), 0, NONE),
    ]
    assert {r[0] for r in ROWS} == set(ORDER)
    got = []
    for name, over, _, _ in ROWS:
        assert lib.mjh_fd_tangent(None, None, None, None, 0, 0, st) == -22 and lib.mjh_last_error() == b"null argument"
        a = dict(BASE[name], **over)
        rc = getattr(lib, "mjh_" + name)(*[a[k] for k in ORDER[name].split()], st)
        got.append((rc, lib.mjh_last_error().decode()))
    torch.cuda.synchronize()
    for (name, over, rc, text), g in zip(ROWS, got):
        shown = {k: v for k, v in over.items() if isinstance(v, (int, float))}
        print(f"{name} {shown} {sorted(set(over) - set(shown))}: {g}")
    wrong = [(name, sorted(over), g, (rc, text)) for (name, over, rc, text), g in zip(ROWS, got) if g != (rc, text)]
    assert not wrong, wrong
