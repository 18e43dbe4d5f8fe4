"""inverse_fd on the device against the host composition: tests/_ifd_ref.py around the library's own ``inverse``.

The yardstick of test 2 runs the same inverse pass on host-built perturbed inputs, so only the two new kernels are judged.  That needs ``inverse``
not to depend on where in a batch an environment sits, or how large the batch is: ``test_inverse_does_not_depend_on_placement`` establishes it (one
environment replicated at batch sizes 2 .. 150: bit-identical ``qfrc_inverse`` and ``sensordata``).  ``placement_spread`` measures it per model and
test 2 uses the measurement: with a spread of zero (measured on an MI355X: 0 in every model below) its allowance is zero; a spread ``s`` would allow ``2 s / eps``
(centered: ``s / eps``) instead.  Hence:

* entries whose column is an add / subtract quantity (slide / hinge / free-translation dofs, qvel, qacc): EXACT equality -- no output row is a
  quaternion, so there are no row bounds;
* columns that are rotational dofs of ball / free joints: ``_fd_ref.column_bound`` (the two perturbed quaternions differ by roundings, which the
  pass carries to every output with the yardstick's own derivative).
"""
import functools
import math

import numpy as np
import pytest
import torch

import _fd_ref as R
import _ifd_ref as I
import mujoco_torch_amd as mt
from _cases import seeded_batch
from _util import INT_LEAVES, REAL_LEAVES, leaf, load_model

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
MACH = {F64: 2.0 ** -52, F32: 2.0 ** -23}
INVDISCRETE = int(mt.EnableBit.INVDISCRETE)
DISCRETE = {"enableflags": INVDISCRETE}
CASES = [("cartpole", F64, 64, {}), ("ball_free_actuators", F64, 32, {}), ("ant", F64, 32, {}), ("ant", F32, 32, {}), ("humanoid", F64, 16, {}),
         ("sensor_rig", F64, 16, {}), ("halfcheetah", F64, 16, DISCRETE)]
INVERSE_FD = mt.inverse_fd  # (everything here belongs to the feature: without it the module does not import)


def joints(mx):
    return R.Joints(mx.jnt_type.data.cpu().numpy(), np.asarray(mx.jnt_qposadr), np.asarray(mx.jnt_dofadr), int(mx.nq), int(mx.nv))


def on_gpu(xml, dtype, B, overrides=None):
    """``seeded_batch`` with a seeded non-zero ``qacc`` (of the size of a gravity-driven acceleration)."""
    mx, d = seeded_batch(xml, overrides or {}, dtype, B)
    qacc = torch.tensor(3.0 * np.random.RandomState(7).randn(B, int(mx.nv))).to(dtype)
    d = d.replace(qacc=qacc)
    return mx, mx.to("cuda"), d.to("cuda")


def outputs(y, sensors):
    out = {"qfrc_inverse": y.qfrc_inverse.detach().cpu().numpy()}
    if sensors:
        out["sensordata"] = y.sensordata.detach().cpu().numpy()
    return out


def has_sensors(mx):
    return int(getattr(mx, "nsensordata", 0) or 0) > 0


@functools.lru_cache(maxsize=None)
def placement_spread(xml, dtype, discrete=False):
    """{output: the largest |difference| between one environment evaluated alone and replicated at batch sizes 2, 7, 64 and 150}."""
    mx, mg, dg = on_gpu(xml, dtype, 4, DISCRETE if discrete else {})
    sens = has_sensors(mx)
    want = outputs(mt.inverse(mg, dg[torch.tensor([2])]), sens)
    assert np.abs(want["qfrc_inverse"]).max() > 0
    spread = {k: 0.0 for k in want}
    for B in (2, 7, 64, 150):
        got = outputs(mt.inverse(mg, dg[torch.full((B,), 2)]), sens)
        for k, v in want.items():
            assert np.isfinite(got[k]).all(), (xml, B, k)
            spread[k] = max(spread[k], float(np.abs(got[k] - v).max()))
    return spread


def composition(mx, mg, dg, eps, centered):
    """The six Jacobians by _ifd_ref around ``inverse`` (one call over all perturbed environments)."""
    jt = joints(mx)
    B, nv = dg.qpos.shape[0], int(mx.nv)
    np_ = lambda t: t.detach().cpu().numpy()
    P = I.perturbed(jt, np_(dg.qpos), np_(dg.qvel), np_(dg.qacc), eps, centered)
    ncol, nside = P["qpos"].shape[1:3]
    rep = dg[torch.arange(B).repeat_interleave(ncol * nside)]
    rep = rep.replace(**{k: torch.tensor(v.reshape(B * ncol * nside, v.shape[-1]), device=dg.qpos.device) for k, v in P.items()})
    sens = has_sensors(mx)
    y0, y = outputs(mt.inverse(mg, dg), sens), outputs(mt.inverse(mg, rep), sens)
    y = {k: v.reshape(B, ncol, nside, v.shape[-1]) for k, v in y.items()}
    if not sens:
        y0["sensordata"], y["sensordata"] = np.zeros((B, 0), dtype=y0["qfrc_inverse"].dtype), np.zeros((B, ncol, nside, 0), dtype=y0["qfrc_inverse"].dtype)
    return I.jacobians(nv, y0["qfrc_inverse"], y["qfrc_inverse"], eps, centered, y0["sensordata"], y["sensordata"])


def tolerances(jt, ref, dtype, eps, centered, spread):
    """Per entry of each of the six: the placement allowance (zero on a placement-independent ``inverse``), plus ``column_bound`` on the
    rotational columns of DfDq / DsDq."""
    out = []
    for k, J in enumerate(ref):
        s = spread["qfrc_inverse" if k < 3 else "sensordata"] if J.shape[1] else 0.0
        tol = np.full(J.shape, (1.0 if centered else 2.0) * s / eps)
        if k in (0, 3):
            for _, da in jt.quats:
                tol[:, :, da:da + 3] += R.column_bound(MACH[dtype], eps, J[:, :, da:da + 3])[:, :, None]
        out.append(tol)
    return out


NAMES = ("DfDq", "DfDv", "DfDa", "DsDq", "DsDv", "DsDa")


def compare(what, got, ref, tol):
    for name, g, r, t in zip(NAMES, got, ref, tol):
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
def test_inverse_does_not_depend_on_placement(xml):
    spread = placement_spread(xml, F64)
    print(f"{xml}: placement spread of inverse {spread}")
    assert all(v == 0 for v in spread.values()), (xml, spread)


@pytest.mark.parametrize("centered", [False, True], ids=["one-sided", "centered"])
@pytest.mark.parametrize("xml,dtype,B,overrides", CASES, ids=[f"{x}-{str(t)[6:]}{'-discrete' if o else ''}" for x, t, _, o in CASES])
def test_machinery_matches_the_host_composition(xml, dtype, B, overrides, centered):
    mx, mg, dg = on_gpu(xml, dtype, B, overrides)
    if overrides:
        assert int(mx.opt.enableflags) & INVDISCRETE and int(mx.opt.integrator) == 0 and float(mx.dof_damping.abs().max()) > 0  # the discrete form runs
    eps = 1e-6 if dtype == F64 else 1e-3  # (float32: an eps its 2^-23 can resolve; the comparison is exact either way)
    got = mt.inverse_fd(mg, dg, eps=eps, centered=centered, sensors=True)
    ref = composition(mx, mg, dg, eps, centered)
    nv, nsd = int(mx.nv), int(getattr(mx, "nsensordata", 0) or 0)
    assert [tuple(g.shape) for g in got] == [(B, nv, nv)] * 3 + [(B, nsd, nv)] * 3 and all(g.dtype == dtype for g in got)
    spread = placement_spread(xml, dtype, bool(overrides))
    print(f"{xml} {dtype}: placement spread {spread}, allowance in place of zero {(1.0 if centered else 2.0) * max(spread.values()) / eps:.3e}")
    compare(f"{xml} {dtype} centered={centered}", got, ref, tolerances(joints(mx), ref, dtype, eps, centered, spread))
    assert np.abs(ref[0]).max() > 0 and np.abs(ref[2]).max() > 0.5  # (DfDv is exactly zero on an upright cartpole without damping)
    three = mt.inverse_fd(mg, dg, eps=eps, centered=centered)
    assert len(three) == 3 and all(torch.equal(a, b) for a, b in zip(three, got))


def test_it_is_a_derivative_the_acceleration_columns_are_the_mass_matrix():
    """Cartpole in float64 has no constraint rows, so ``qfrc_inverse = qfrc_bias + M qacc - qfrc_passive`` is affine in ``qacc`` with matrix ``qM``:
    centered ``DfDa`` at ``eps = 1e-6`` against the dense ``qM`` of the nominal pass.  A centered difference of an affine function has no
    truncation error; the bound counts roundings, with ``u = 2^-53``, in the order ``csrc/mjh_inverse.h`` documents.  The position and velocity
    stages see the same inputs in both slots of an acceleration column, so ``qM``, ``qfrc_bias`` and ``qfrc_passive`` are the same bits there
    (test 1) and only the tail differs:

    * ``y_i = sum_k M_ik x_k`` from ``s = 0`` in ``k`` order: ``nv`` products and ``nv - 1`` inexact additions (``0 + p`` is exact), each at most
      ``u Y_i``, ``Y_i = sum_k |M_ik| (|qacc_k| + eps)``: ``(2 nv - 1) u Y_i``;
    * ``(qfrc_bias_i + y_i)``: ``u (|b_i| + Y_i)``;  ``- qfrc_passive_i``: ``u (|b_i| + Y_i + |p_i|)``;  ``- qfrc_constraint_i``, which is an
      exact zero without constraint rows: no rounding.  Together ``E_i = u ((2 nv + 1) Y_i + 2 |b_i| + |p_i|)``, inflated by ``(1 + 2^-40)`` for the
      second-order terms;
    * the two passes of a column: ``2 E_i / (2 eps)``;
    * the operand: ``qacc_j +- eps`` is rounded, half an ulp ``u (|qacc_j| + eps)`` on each side, carried by ``|M_ij|`` and divided by ``2 eps``:
      ``u (|qacc_j| + eps) |M_ij| / eps``;
    * the subtraction ``f+ - f-`` and the division by ``2 eps``: ``2 u`` relative to the entry, bounded with ``|M_ij|`` plus the terms above.

    Measured on an MI355X: max |qM| 1.10, worst deviation 4.2e-10, worst deviation / bound 0.25, largest bound 5.0e-9.
    """
    mx, mg, dg = on_gpu("cartpole", F64, 64)
    eps, u = 1e-6, 2.0 ** -53
    nv = int(mx.nv)
    y0 = mt.inverse(mg, dg)
    assert int(y0.nefc) == 0 and float(y0.qfrc_constraint.abs().max()) == 0
    M = mt.full_m(mg, y0).cpu().numpy()
    assert M.shape == (64, nv, nv) and np.abs(M).max() > 0.5
    b, p, a = (t.cpu().numpy() for t in (y0.qfrc_bias, y0.qfrc_passive, dg.qacc))
    assert np.abs(a).max() > 1.0
    DfDa = mt.inverse_fd(mg, dg, eps=eps, centered=True)[2].cpu().numpy()
    Y = np.einsum("bik,bk->bi", np.abs(M), np.abs(a) + eps)
    E = u * ((2 * nv + 1) * Y + 2 * np.abs(b) + np.abs(p)) * (1 + 2.0 ** -40)
    first = 2 * E[:, :, None] / (2 * eps) + u * (np.abs(a)[:, None, :] + eps) * np.abs(M) / eps
    bound = first * (1 + 2 * u) + 2 * u * np.abs(M)
    err = np.abs(DfDa - M)
    print(f"cartpole DfDa against qM: max |qM| {np.abs(M).max():.3e}, worst deviation {err.max():.3e}, worst deviation / bound {(err / bound).max():.3e}, "
          f"largest bound {bound.max():.3e}")
    assert (err <= bound).all(), float((err / bound).max())


def test_chunking_changes_nothing():
    mx, mg, dg = on_gpu("humanoid", F64, 8)
    ncol = 3 * int(mx.nv)
    pool = lambda: list(mg.tables.__dict__["_fd_scratch"].values())[-1]
    for centered in (False, True):
        nside = 2 if centered else 1
        whole = mt.inverse_fd(mg, dg, centered=centered, sensors=True, max_scratch_bytes=1 << 40)
        scr = pool()
        assert scr.slots == 8 * ncol * nside  # one chunk
        cut = mt.inverse_fd(mg, dg, centered=centered, sensors=True, max_scratch_bytes=scr.slab.numel() * 30 // ncol)
        cols = pool().slots // (8 * nside)
        assert math.ceil(ncol / cols) >= 3 and ncol % cols != 0, (ncol, cols)  # three chunks or more, the last one ragged
        single = mt.inverse_fd(mg, dg, centered=centered, sensors=True, max_scratch_bytes=1)  # one column per chunk
        assert pool().slots == 8 * nside
        for a, b, c in zip(whole, cut, single):
            assert torch.equal(a, b) and torch.equal(a, c)
    # the scratch pool is shared with transition_fd: a call of one between two of the other changes neither
    before = mt.inverse_fd(mg, dg, sensors=True)
    A0 = mt.transition_fd(mg, dg)
    A1 = mt.transition_fd(mg, dg)
    after = mt.inverse_fd(mg, dg, sensors=True)
    A2 = mt.transition_fd(mg, dg)
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    assert all(torch.equal(a, b) and torch.equal(a, c) for a, b, c in zip(A0, A1, A2))


def test_unbatched_data_is_the_batch_of_one():
    mx, mg, dg = on_gpu("ball_free_actuators", F64, 3)
    whole = mt.inverse_fd(mg, dg)
    one = mt.inverse_fd(mg, dg[1])
    nv = int(mx.nv)
    assert all(o.shape == (nv, nv) and torch.equal(o, w[1]) for o, w in zip(one, whole))
    two = mt.inverse_fd(mg, dg[torch.arange(3).reshape(3, 1)])  # batch shape (3, 1)
    assert all(t.shape == (3, 1, nv, nv) and torch.equal(t[:, 0], w) for t, w in zip(two, whole))


def test_inputs_are_untouched_and_calls_repeat():
    mx, mg, dg = on_gpu("humanoid", F64, 8)
    names = [n for n in REAL_LEAVES + INT_LEAVES if isinstance(leaf(dg, n), torch.Tensor)]
    before = {n: leaf(dg, n).clone() for n in names}
    qinv = dg.qfrc_inverse.clone()
    first = mt.inverse_fd(mg, dg, centered=True, sensors=True)
    second = mt.inverse_fd(mg, dg, centered=True, sensors=True)
    assert len(names) > 60 and all(torch.equal(leaf(dg, n), before[n]) for n in names) and torch.equal(dg.qfrc_inverse, qinv)
    assert all(torch.equal(a, b) for a, b in zip(first, second))


def test_kernel_ids_and_byte_accounts():
    """The two kernels report under their timing ids (45, 46), and ``mjh_model_kernel_io`` accounts them per slot: the perturb kernel reads and
    writes the input leaves of an inverse pass -- an upper bound that also counts the four input-only sensor leaves (18 reals per body) this
    Data does not carry -- and the difference kernel one slot's ``qfrc_inverse`` and ``sensordata`` in, one column of ``DfD*`` / ``DsD*`` out."""
    import ctypes

    from mujoco_torch_amd import derivative, native

    for xml in ("humanoid", "sensor_rig"):
        mx, mg, dg = on_gpu(xml, F64, 4)
        nm = native.get_native_model(mg, torch.device("cuda", 0), F64)
        rw = (ctypes.c_int64 * 2)()
        assert nm.lib.mjh_model_kernel_io(nm.handle, 45, rw) == 0
        carried = sum(leaf(dg, n).numel() // 4 * leaf(dg, n).element_size() for n in derivative._INVERSE_INPUT_LEAVES if isinstance(leaf(dg, n), torch.Tensor))
        assert rw[0] == rw[1] and carried <= rw[0] <= carried + 18 * int(mx.nbody) * 8, (xml, carried, rw[0])
        assert nm.lib.mjh_model_kernel_io(nm.handle, 46, rw) == 0
        assert rw[0] == rw[1] == (int(mx.nv) + int(getattr(mx, "nsensordata", 0) or 0)) * 8, (xml, rw[0], rw[1])
        nm.lib.mjh_debug_phase_timing(1)
        try:
            mt.inverse_fd(mg, dg, sensors=True)
            ms, ids = (ctypes.c_float * 96)(), (ctypes.c_int * 96)()
            n = nm.lib.mjh_debug_phase_times(ms, ids, 96)  # (the launches of the most recent native call: the difference kernel's)
        finally:
            nm.lib.mjh_debug_phase_timing(0)
        assert [ids[i] for i in range(n)] == [46] and ms[0] > 0


def test_refusals():
    mx, mg, dg = on_gpu("cartpole", F64, 4)
    with pytest.raises(ValueError, match="eps"):
        mt.inverse_fd(mg, dg, eps=0)
    with pytest.raises(ValueError, match="eps"):
        mt.inverse_fd(mg, dg, eps=float("inf"))
    with pytest.raises(ValueError, match="float32"):
        mt.inverse_fd(mg, dg.to(F32))
    with pytest.raises(RuntimeError, match="HIP device"):
        mt.inverse_fd(mx, dg.to("cpu"))
    with pytest.raises(NotImplementedError, match="vmap"):
        torch.vmap(lambda q: mt.inverse_fd(mg, dg[0].replace(qpos=q))[0])(dg.qpos)
    six = mt.inverse_fd(mg, dg, sensors=True)  # no sensors: DsD* with a zero first dimension
    assert [tuple(t.shape) for t in six] == [(4, 2, 2)] * 3 + [(4, 0, 2)] * 3
    # RK4 with INVDISCRETE: inverse's own error
    rk = load_model("ant", {"integrator": 1})
    d = mt.make_data(rk).expand(4).clone().to("cuda")
    rkdev = rk.to("cuda")
    disc = rkdev.replace(opt=rkdev.opt.replace(enableflags=INVDISCRETE))
    with pytest.raises(RuntimeError, match="discrete inverse dynamics is not supported by RK4 integrator"):
        mt.inverse_fd(disc, d)
    assert all(t.shape == (4, rk.nv, rk.nv) for t in mt.inverse_fd(rkdev, d))  # the continuous form of the same RK4 model
    # sensors disabled: sensordata is the caller's in every pass, DsD* are zeros
    off, mgo, dgo = on_gpu("sensor_rig", F64, 2, {"disableflags": int(mt.DisableBit.SENSOR)})
    six = mt.inverse_fd(mgo, dgo, sensors=True)
    nsd = int(off.nsensordata)
    assert nsd > 0 and all(t.shape == (2, nsd, off.nv) and not bool(t.any()) for t in six[3:]) and all(bool(t.any()) for t in six[:3])


def test_the_two_perturb_entry_points_agree_where_their_columns_coincide():
    """Columns [0, 2 nv) mean the same to ``mjh_fd_perturb`` and ``mjh_ifd_perturb``: a nudge of qpos in tangent space, then of qvel.  Over the
    same input leaves, the leaves both scratch batches carry come out equal bit for bit -- in a model with a ball joint, a free joint and ctrl
    (it has no act: that leaf is empty in both batches), for windows whose slot counts are no multiple of a workgroup's 64 lanes (leaves of 1, nq and nv words end inside the streaming loop's
    last trip)."""
    import ctypes
    import sys

    from mujoco_torch_amd import derivative, native

    fw = sys.modules["mujoco_torch_amd.forward"]
    B, eps = 3, 1e-6
    mx, mg, dg = on_gpu("ball_free_actuators", F64, B)
    dev = dg.qpos.device
    nq, nv, na, nu = int(mx.nq), int(mx.nv), int(mx.na), int(mx.nu)
    types, qadr = mx.jnt_type.data.cpu().numpy(), np.asarray(mx.jnt_qposadr)
    quat = np.zeros(nq, dtype=bool)
    for t, a in zip(types, qadr):
        if t == 0:    # free: the quaternion follows the translation
            quat[a + 3:a + 7] = True
        elif t == 1:  # ball
            quat[a:a + 4] = True
    assert nu > 0 and (types == 0).any() and (types == 1).any()
    nm = native.get_native_model(mg, dev, F64)
    lib, h = nm.lib, nm.handle
    derivative._bind(lib)
    tab = fw._table(dg, (mg.tables.uid, F64, dev, B), nm.leaf_counts, B, F64, dev)
    leaf_bytes = derivative._leaf_bytes(fw, nm.leaf_counts, F64)
    slots = B * 2 * nv * 2
    scratch = lambda names: derivative._make_scratch(fw, tuple(fw._IDX[n] for n in names if tab.arr[fw._IDX[n]] != 0), (), (), (), leaf_bytes, slots, dev)
    fd, ifd = scratch(derivative._INPUT_LEAVES), scratch(derivative._INVERSE_INPUT_LEAVES)

    def view(scr, name, n):
        off = int(np.frombuffer(scr.inp, dtype=np.uint64)[fw._IDX[name]]) - scr.slab.data_ptr()
        assert 0 <= off and off + slots * n * 8 <= scr.slab.numel()
        return scr.slab[off:off + slots * n * 8].view(F64).reshape(slots, n)

    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for centered in (False, True):
        nside = 2 if centered else 1
        for c0, n in ((0, 2 * nv), (1, 2 * nv - 2)):
            used = B * n * nside
            assert used % 64 != 0
            fd.slab.zero_()
            ifd.slab.zero_()
            for fn, scr in ((lib.mjh_fd_perturb, fd), (lib.mjh_ifd_perturb, ifd)):
                rc = fn(h, ctypes.byref(tab.struct), ctypes.byref(scr.inp), B, c0, n, eps, int(centered), st)
                assert rc == 0, lib.mjh_last_error().decode()
            for name, w in (("qpos", nq), ("qvel", nv), ("act", na), ("ctrl", nu), ("qacc_warmstart", nv)):
                if w == 0:
                    assert tab.arr[fw._IDX[name]] == 0
                    continue
                assert torch.equal(view(fd, name, w), view(ifd, name, w)), (centered, c0, name)
            qpos = view(ifd, "qpos", nq)[:used].reshape(B, n * nside, nq)
            qvel = view(ifd, "qvel", nv)[:used].reshape(B, n * nside, nv)
            assert bool((qpos != dg.qpos[:, None, :])[..., torch.tensor(quat, device=dev)].any()) and bool((qvel != dg.qvel[:, None, :]).any())
            assert not bool(view(ifd, "qpos", nq)[used:].any())  # nothing past the call's slots
