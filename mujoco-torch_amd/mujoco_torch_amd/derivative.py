"""``transition_fd``: finite-difference Jacobians of one ``step`` with respect to state and control (MuJoCo's ``mjd_transitionFD``);
``transition_vjp``: their product with a cotangent, without forming them; ``differentiable_step``: ``step`` with an autograd graph built on that;
``inverse_fd``: finite-difference Jacobians of ``inverse`` with respect to position, velocity and acceleration (MuJoCo's ``mjd_inverseFD``).

The step is one opaque native launch sequence, so there is no autograd graph to differentiate; what the library can do cheaply is step many
environments at once.  The ``P`` perturbed steps of an environment are ``P`` more environments of a scratch batch:

* ``mjh_fd_perturb`` (``csrc/mjh_fd.h``) writes the input leaves of a chunk of perturbed environments from the caller's ``Data``, each with one
  entry of ``qpos`` (in tangent space: quaternions are rotated, not added to), ``qvel``, ``act`` or ``ctrl`` nudged by ``eps``;
* ``mjh_step`` -- the library's ordinary step, unchanged -- advances the chunk;
* ``mjh_fd_difference`` differences the chunk's next states (``qpos`` back in tangent space) against the nominal step, or against each other, and
  writes the chunk's columns of ``A``, ``B`` (``C``, ``D``) in place.

The nominal step runs once.  The scratch batch is bounded by ``max_scratch_bytes``: the columns are processed in chunks sized to it, the scratch is
reused between chunks and kept per (model, batch, dtype, stream) for the next call.  Host work per call is a few ctypes calls per chunk; nothing
synchronises, everything runs on the caller's current stream.

``inverse_fd`` goes through the same chunk loop with another native pass between its two kernels: ``mjh_ifd_perturb`` (``csrc/mjh_ifd.h``) nudges
``qpos`` (tangent space), ``qvel`` or ``qacc``, ``mjh_inverse`` -- the library's ordinary inverse pass, unchanged -- runs on the chunk, and
``mjh_ifd_difference`` differences ``qfrc_inverse`` and ``sensordata``.
"""

from __future__ import annotations

import ctypes
import functools
import math
import sys

import numpy as np
import torch

from . import native
from .types import Data, Model

MAX_SCRATCH_BYTES = 2 << 30  # default budget of the scratch batch (its input leaves, its step outputs and the step's workspace)
_ALIGN = 256
_SCRATCH_KEPT = 2            # scratch batches kept per model for later calls (most recently used)

# every leaf a step can read from its input Data (csrc/mjh_kernels.h, mjh_sensor.h): the state, the caller's forces and targets, and the leaves
# a step carries over where a stage is disabled or absent (tracking cameras read subtree_com; qfrc_gravcomp with gravity off; actuator_force with
# actuation off; qfrc_constraint without constraint rows; sensordata slots no sensor fills).  Those the caller's Data holds are replicated.
_INPUT_LEAVES = ("time qpos qvel act qacc_warmstart ctrl qfrc_applied xfrc_applied mocap_pos mocap_quat subtree_com qfrc_gravcomp actuator_force "
                 "qfrc_constraint sensordata eq_active").split()
# ... and an inverse pass (mjh_inverse's contract, include/mjhip.h): it runs the stages of a step up to the velocity stage, then the tail, which reads
# the caller's qacc, and the sensors, which read the caller's actuator_force / qfrc_actuator because the pass evaluates no actuation.
_INVERSE_INPUT_LEAVES = _INPUT_LEAVES + ["qacc", "qfrc_actuator"]


def _bind(lib):
    if not hasattr(lib, "mjh_fd_perturb"):
        raise RuntimeError(f"{native.LIB_PATH} predates transition_fd (no mjh_fd_perturb): rebuild the library")
    if getattr(lib, "_fd_bound", False):
        return
    P, V = ctypes.POINTER(native.DataPtrs), ctypes.c_void_p
    lib.mjh_fd_perturb.argtypes = [V, P, P, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int, V]
    lib.mjh_fd_perturb.restype = ctypes.c_int
    lib.mjh_fd_difference.argtypes = [V, P, P, P, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int, V, V, V, V, V]
    lib.mjh_fd_difference.restype = ctypes.c_int
    if not hasattr(lib, "mjh_fd_vjp"):
        raise RuntimeError(f"{native.LIB_PATH} predates transition_vjp (no mjh_fd_vjp): rebuild the library")
    lib.mjh_fd_vjp.argtypes = [V, P, P, P, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int, V, V, V, V, V]
    lib.mjh_fd_vjp.restype = ctypes.c_int
    lib.mjh_fd_tangent.argtypes = [V, V, V, V, ctypes.c_int64, ctypes.c_int, V]
    lib.mjh_fd_tangent.restype = ctypes.c_int
    if not hasattr(lib, "mjh_ifd_perturb"):
        raise RuntimeError(f"{native.LIB_PATH} predates inverse_fd (no mjh_ifd_perturb): rebuild the library")
    lib.mjh_ifd_perturb.argtypes = [V, P, P, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int, V]
    lib.mjh_ifd_perturb.restype = ctypes.c_int
    lib.mjh_ifd_difference.argtypes = [V, V, V, V, V, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int, V, V, V, V, V, V, V]
    lib.mjh_ifd_difference.restype = ctypes.c_int
    lib._fd_bound = True


class _Scratch:
    """The scratch batch of ``slots`` environments: one allocation, and the two pointer structs (inputs, the pass's outputs) into it; ``tail``:
    the address of ``tail_bytes`` more per slot, for an output that is no ABI leaf (``qfrc_inverse``), or 0."""

    __slots__ = ("slab", "inp", "out", "slots", "tail")


def _leaf_bytes(fw, counts, dtype):
    """Bytes per environment of every ABI leaf."""
    esize = torch.empty((), dtype=dtype).element_size()
    size = np.full(fw._NLEAF, esize, dtype=np.int64)
    for n, dt in fw._INT_DTYPE.items():
        size[fw._IDX[n]] = 4 if dt == torch.int32 else 8
    return np.asarray(counts, dtype=np.int64) * size


def _make_scratch(fw, in_idx, extra_idx, extra_bytes, out_idx, leaf_bytes, slots, device, tail_bytes=0) -> _Scratch:
    s = _Scratch()
    s.slots = slots
    s.inp, s.out = native.DataPtrs(), native.DataPtrs()
    inp = np.frombuffer(s.inp, dtype=np.uint64)
    out = np.frombuffer(s.out, dtype=np.uint64)
    off, where = 0, []
    for arr, idx, nbytes in [(inp, i, leaf_bytes[i]) for i in in_idx] + [(inp, fw._NLEAF + k, b) for k, b in zip(extra_idx, extra_bytes)] + \
                            [(out, i, leaf_bytes[i]) for i in out_idx]:
        if nbytes == 0:
            continue
        where.append((arr, idx, off))
        off += (int(nbytes) * slots + _ALIGN - 1) // _ALIGN * _ALIGN
    tail_off = off
    off += (int(tail_bytes) * slots + _ALIGN - 1) // _ALIGN * _ALIGN
    s.slab = torch.empty(off, dtype=torch.uint8, device=device)
    base = s.slab.data_ptr()
    for arr, idx, o in where:
        arr[idx] = base + o
    s.tail = base + tail_off if tail_bytes else 0
    return s


def _outside_graphs(fn):
    """``fn`` kept out of Dynamo: a ``torch.compile`` region that calls it breaks its graph there and runs it eagerly, or refuses it under
    ``fullgraph=True``.  Without this Dynamo goes on to compile the frames below the call one by one and fails on the raw pointers they handle.
    The marking is made at the first call that finds the tracer loaded: importing it costs a second that a plain ``import`` should not pay."""
    marked = []

    @functools.wraps(fn)
    def call(*args, **kwargs):
        if "torch._dynamo" not in sys.modules:
            return fn(*args, **kwargs)
        if not marked:
            marked.append(torch.compiler.disable(fn))
        return marked[0](*args, **kwargs)

    return call


class _Call:
    """What ``_validate`` established about a call: the sizes, the dtype and device, the batch shape and the scratch budget."""

    __slots__ = ("fw", "eps", "dtype", "device", "batch", "B", "nv", "na", "nu", "nsd", "ns", "budget", "sens_written")


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None and t.numel() else None)


def _validate(name, m: Model, d: Data, eps, max_scratch_bytes) -> _Call:
    """The refusals every entry point of this module shares, in the order ``transition_fd`` has always made them."""
    c = _Call()
    c.fw = fw = sys.modules[__package__ + ".forward"]  # (the package attribute `forward` is the function)
    try:
        eps = float(eps)
    except (TypeError, ValueError):
        raise ValueError(f"eps must be a positive number, got {eps!r}") from None
    if not eps > 0 or math.isinf(eps):
        raise ValueError(f"eps must be a positive finite number, got {eps}")
    qpos = d.qpos
    if torch.compiler.is_compiling() or not fw._plain(qpos):
        raise NotImplementedError(f"{name} cannot be used under torch.vmap / torch.compile: there is no operator for it.  Call it on a "
                                  "batched Data directly (every leading dimension of a leaf is the batch).")
    dtype = qpos.dtype
    mdtype = m.qpos0.dtype
    if dtype != mdtype:
        raise ValueError(f"the Data is {dtype}, the Model {mdtype}: {name} runs in the model's dtype")
    if dtype not in (torch.float64, torch.float32):
        raise ValueError(f"unsupported dtype {dtype}: {name} runs in float64 or float32")
    if not float(torch.tensor(eps, dtype=dtype)) > 0:
        raise ValueError(f"eps = {eps} rounds to zero in {dtype}")
    c.budget = MAX_SCRATCH_BYTES if max_scratch_bytes is None else int(max_scratch_bytes)
    if c.budget <= 0:
        raise ValueError(f"max_scratch_bytes must be positive, got {max_scratch_bytes}")
    c.eps, c.dtype, c.device = eps, dtype, qpos.device
    c.batch = tuple(qpos.shape[:-1])
    c.B = int(math.prod(c.batch)) if c.batch else 1
    c.nv, c.na, c.nu, c.nsd = int(m.nv), int(m.na), int(m.nu), int(getattr(m, "nsensordata", 0) or 0)
    c.ns = 2 * c.nv + c.na
    c.sens_written = c.nsd > 0 and "sensordata" in fw._written_names(m, True)  # (else sensordata is the caller's in every step)
    return c


def _on_device(c: _Call, m: Model):
    """... and the one that needs the tensors on a device (after the argument refusals, which do not)."""
    c.fw._require_device(c.device)


def _drive(name, c: _Call, m: Model, d: Data, centered, fixed_iterations, consume, nominal=None, inverse=False):
    """The chunk loop: perturb, step, ``consume(lib, handle, in, nominal, stepped, col0, ncol, stream)`` (``mjh_fd_difference`` or ``mjh_fd_vjp``)
    for every chunk of columns, after the nominal step -- or with ``nominal``, the pointer struct of one that has already run.

    ``inverse``: the native pass between perturb and consume is ``mjh_inverse`` instead of ``mjh_step`` -- the call ``inverse(m, d)`` makes, with
    its flags -- around it ``mjh_ifd_perturb`` over the 3 nv columns of qpos / qvel / qacc, and
    ``consume(lib, handle, nominal_f, nominal_sens, stepped_f, stepped_sens, col0, ncol, stream)`` on the raw pointers of qfrc_inverse (which is
    no ABI leaf: the scratch batch carries it behind its leaves) and sensordata."""
    fw, dtype, device, B = c.fw, c.dtype, c.device, c.B
    nside = 2 if centered else 1
    ncol = 3 * c.nv if inverse else c.ns + c.nu
    written = fw._inverse_names(m) if inverse else fw._written_names(m, True)

    # ---- the nominal pass; the caller's pointer table ----
    if inverse:
        y0 = fw._run_native(m, d, False, False, None, 0x1F, inverse=True)  # exactly the launches of inverse(m, d)
    else:
        y0 = fw._run_native(m, d, bool(fixed_iterations), True) if nominal is None else None
    nm = native.get_native_model(m, device, dtype)
    _bind(nm.lib)
    T = m.tables
    tab = fw._table(d, (T.uid, dtype, device, B), nm.leaf_counts, B, dtype, device)
    extra = T.sensors["extra_leaves"]
    keep = fw._extra_inputs(tab, d, extra, B, int(m.nbody), dtype, device) if extra else None  # noqa: F841  (contiguous copies live until the launches are enqueued)
    if nominal is None:
        nominal = y0.__dict__["_ptab"].struct

    # ---- the scratch batch ----
    stream, prev = fw._stream_and_guard(device)
    try:
        in_idx = tuple(fw._IDX[n] for n in (_INVERSE_INPUT_LEAVES if inverse else _INPUT_LEAVES) if tab.arr[fw._IDX[n]] != 0)
        esize = torch.empty((), dtype=dtype).element_size()
        extra_idx = tuple(k for k, n in enumerate(fw._EXTRA_NAMES) if extra and n in extra and tab.xarr[k] != 0)
        extra_bytes = tuple(int(m.nbody) * fw._EXTRA_WIDTH[fw._EXTRA_NAMES[k]] * esize for k in extra_idx)
        out_idx = tuple(fw._IDX[n] for n in written)
        leaf_bytes = _leaf_bytes(fw, nm.leaf_counts, dtype)
        tail_bytes = c.nv * esize if inverse else 0
        per_slot = int(leaf_bytes[list(in_idx)].sum() + sum(extra_bytes) + leaf_bytes[list(out_idx)].sum()) + int(nm.work_bytes) + tail_bytes
        cols = int(max(1, min(ncol, c.budget // max(1, per_slot * B * nside))))
        slots = B * cols * nside
        pool = T.__dict__.setdefault("_fd_scratch", {})
        key = (device, dtype, stream, slots, in_idx, extra_idx) + (("inverse",) if inverse else ())
        scr = pool.pop(key, None)
        if scr is None:
            while len(pool) >= _SCRATCH_KEPT:
                pool.pop(next(iter(pool)))
            scr = _make_scratch(fw, in_idx, extra_idx, extra_bytes, out_idx, leaf_bytes, slots, device, tail_bytes)
        pool[key] = scr  # (most recently used last)
        work = nm.workspace(slots, stream)
        wptr = ctypes.c_void_p(work.data_ptr() if work is not None else None)
        flags = fw._inverse_flags(m) if inverse else (native.FLAG_FIXED_ITERATIONS if fixed_iterations else 0)
        lib, h, st = nm.lib, nm.handle, ctypes.c_void_p(stream)
        pin, pscr_in, pscr_out, py0 = ctypes.byref(tab.struct), ctypes.byref(scr.inp), ctypes.byref(scr.out), ctypes.byref(nominal)
        if inverse:
            sens = fw._IDX["sensordata"]
            f0, s0 = _ptr(y0.qfrc_inverse), ctypes.c_void_p(int(y0.__dict__["_ptab"].arr[sens]) or None)
            f1, s1 = ctypes.c_void_p(scr.tail), ctypes.c_void_p(int(np.frombuffer(scr.out, dtype=np.uint64)[sens]) or None)
        for c0 in range(0, ncol, cols):
            n = min(cols, ncol - c0)
            if inverse:
                rc = lib.mjh_ifd_perturb(h, pin, pscr_in, B, c0, n, c.eps, int(bool(centered)), st)
                if rc == 0:
                    rc = lib.mjh_inverse(h, pscr_in, pscr_out, f1, wptr, B * n * nside, flags, st)
                if rc == 0:
                    rc = consume(lib, h, f0, s0, f1, s1, c0, n, st)
            else:
                rc = lib.mjh_fd_perturb(h, pin, pscr_in, B, c0, n, c.eps, int(bool(centered)), st)
                if rc == 0:
                    rc = lib.mjh_step(h, pscr_in, pscr_out, wptr, B * n * nside, flags, st)
                if rc == 0:
                    rc = consume(lib, h, pin, py0, pscr_out, c0, n, st)
            if rc != 0:
                raise RuntimeError(f"native {name} failed ({rc}): {lib.mjh_last_error().decode()}")
    finally:
        if prev is not None:
            torch.cuda.set_device(prev)


def transition_fd(m: Model, d: Data, eps: float = 1e-6, centered: bool = False, sensors: bool = False, fixed_iterations: bool = False, *,
                  max_scratch_bytes: int | None = None):
    """Finite-difference Jacobians of ``step`` (MuJoCo's ``mjd_transitionFD``): ``A, B`` or, with ``sensors=True``, ``A, B, C, D``.

    With the state ``x = [dq (nv, tangent space), qvel (nv), act (na)]``, ``ns = 2 nv + na``, ``u = ctrl`` and ``y`` the state after one step:
    ``A = dy/dx``: ``S + (ns, ns)``, ``B = dy/du``: ``S + (ns, nu)``, ``C = dsensordata/dx``: ``S + (nsensordata, ns)``, ``D = dsensordata/du``:
    ``S + (nsensordata, nu)``, ``S`` being the batch shape of ``d``.  Rows are outputs, columns what was perturbed: ``A[..., i, j] = dy_i / dx_j``.
    A model without sensors returns ``C``, ``D`` with a zero first dimension.  ``state_sub`` / ``state_add`` (``qpos.py``) form differences and sums of physics
    states ``[qpos, qvel, act]`` in these coordinates: ``state_sub(m, step(state_add(m, x, dx)), step(x))`` is ``A dx`` to first order.

    Every other input of the step (``time``, ``qacc_warmstart``, ``mocap_*``, ``qfrc_applied``, ``xfrc_applied``, ``eq_active`` ...) is the caller's,
    in the nominal and in every perturbed step.  ``qpos`` is perturbed and differenced in tangent space: slide / hinge joints and free translations
    add and subtract, ball joints and the rotation of free joints rotate the quaternion by ``eps`` about the dof's local axis and take the rotation
    vector of ``q0^-1 q1``.  One-sided differences ``(y+ - y0) / eps`` by default, ``(y+ - y-) / (2 eps)`` with ``centered``.  A control with
    ``actuator_ctrllimited`` is nudged only where ``ctrl`` and the nudged ``ctrl`` both lie inside ``actuator_ctrlrange``: forward if it can be,
    backward if ``centered`` or if forward was refused; the column is the mean of the one-sided differences taken, zero if there was none.

    ``fixed_iterations`` is passed to every step.  With early termination the solver may stop after a different number of iterations in two of the
    steps, and their difference over ``eps`` is then solver tolerance over ``eps`` rather than a derivative (as in MuJoCo): for models in contact use
    ``fixed_iterations=True`` or a tight ``opt.tolerance``.

    The perturbed steps run as a scratch batch of ``B x columns x (2 if centered else 1)`` environments, in chunks of columns sized so that the
    scratch stays under ``max_scratch_bytes`` (default ``MAX_SCRATCH_BYTES``; one column at least).  The scratch is kept for the next call.
    """
    c = _validate("transition_fd", m, d, eps, max_scratch_bytes)
    _on_device(c, m)
    batch, dtype, device, ns, nu, nsd = c.batch, c.dtype, c.device, c.ns, c.nu, c.nsd
    A = torch.empty(batch + (ns, ns), dtype=dtype, device=device)
    Bm = torch.empty(batch + (ns, nu), dtype=dtype, device=device)
    C = D = None
    with_sens = bool(sensors) and c.sens_written
    if sensors:
        C = torch.empty(batch + (nsd, ns), dtype=dtype, device=device)
        D = torch.empty(batch + (nsd, nu), dtype=dtype, device=device)
        if not with_sens:  # (sensors disabled: sensordata is the caller's in every step)
            C.zero_()
            D.zero_()
    if c.B == 0 or ns == 0:
        return (A.zero_(), Bm.zero_()) + ((C, D) if sensors else ())
    pA, pB, pC, pD = _ptr(A), _ptr(Bm), _ptr(C if with_sens else None), _ptr(D if with_sens else None)
    cen = int(bool(centered))

    def difference(lib, h, pin, py0, pscr_out, c0, n, st):
        return lib.mjh_fd_difference(h, pin, py0, pscr_out, c.B, c0, n, c.eps, cen, pA, pB, pC, pD, st)

    _drive("transition_fd", c, m, d, centered, fixed_iterations, difference)
    return (A, Bm) + ((C, D) if sensors else ())


@_outside_graphs
def inverse_fd(m: Model, d: Data, eps: float = 1e-6, centered: bool = False, *, sensors: bool = False, max_scratch_bytes: int | None = None):
    """Finite-difference Jacobians of ``inverse`` (MuJoCo's ``mjd_inverseFD``): ``DfDq, DfDv, DfDa`` or, with ``sensors=True``,
    ``DfDq, DfDv, DfDa, DsDq, DsDv, DsDa``.

    ``DfD*``: ``S + (nv, nv)``, the derivatives of ``qfrc_inverse`` with respect to ``dq`` (``qpos`` in tangent space), ``qvel`` and ``qacc``;
    ``DsD*``: ``S + (nsensordata, nv)``, those of ``sensordata``; ``S`` is the batch shape of ``d``.  Rows are outputs, columns what was perturbed,
    as in ``transition_fd``: ``DfDq[..., i, j] = d qfrc_inverse_i / d dq_j``.  MuJoCo's ``mjd_inverseFD`` stores the transposes.  A model without
    sensors returns ``DsD*`` with a zero first dimension; with sensors disabled they are zeros (``sensordata`` is then the caller's in every pass).

    Column ``j`` of ``DfDq`` / ``DsDq`` nudges ``qpos`` along dof ``j`` by ``transition_fd``'s rule: slide / hinge joints and free translations add
    ``eps``, ball joints and the rotation of free joints rotate the quaternion by ``eps`` about the dof's local axis.  Column ``j`` of ``DfDv`` /
    ``DsDv`` adds ``eps`` to ``qvel[j]``, of ``DfDa`` / ``DsDa`` to ``qacc[j]``.  Nothing else is perturbed: ``act``, ``ctrl``, ``qfrc_applied``,
    ``xfrc_applied``, ``mocap_*``, ``eq_active``, ``time`` and the leaves an inverse pass carries over are the caller's in every pass.  One-sided
    differences ``(f+ - f0) / eps`` by default, ``(f+ - f-) / (2 eps)`` with ``centered`` (an extension, as in ``transition_fd``).  Outputs are
    subtracted plainly: neither ``qfrc_inverse`` nor ``sensordata`` has quaternion rows.

    Every pass, the nominal and the perturbed ones, is exactly what ``inverse(m, d)`` runs -- the same native call with the same flags, the discrete
    form under ``EnableBit.INVDISCRETE`` included (an RK4 model then raises ``inverse``'s error before anything is launched).  No iterative solver
    runs in an inverse pass, so the differences carry rounding error only, not the solver tolerance ``transition_fd`` warns about.

    The perturbed passes run as a scratch batch of ``B x columns x (2 if centered else 1)`` environments, in chunks of columns sized so that the
    scratch stays under ``max_scratch_bytes`` (default ``MAX_SCRATCH_BYTES``; one column at least); it comes from the pool ``transition_fd`` keeps
    its own in.  Nothing synchronises, everything runs on the caller's current stream, ``d`` is not written.  Under ``torch.vmap`` the call raises
    ``NotImplementedError``; it is kept out of ``torch.compile`` graphs like ``transition_vjp``.

    Out of scope: MuJoCo's ``flg_actuation`` (the library's inverse pass does not evaluate actuation: ``qfrc_inverse`` is the total force, whatever
    ``ctrl`` is); ``DmDq``, the derivative of the mass matrix; a vector-Jacobian product or an autograd wrapper; and MuJoCo's stage skipping -- the
    acceleration columns run whole inverse passes although only the tail depends on ``qacc``.
    """
    c = _validate("inverse_fd", m, d, eps, max_scratch_bytes)
    _on_device(c, m)
    batch, dtype, device, nv, nsd = c.batch, c.dtype, c.device, c.nv, c.nsd
    Df = [torch.empty(batch + (nv, nv), dtype=dtype, device=device) for _ in range(3)]
    Ds = []
    with_sens = bool(sensors) and c.nsd > 0 and "sensordata" in c.fw._inverse_names(m)
    if sensors:
        Ds = [torch.empty(batch + (nsd, nv), dtype=dtype, device=device) for _ in range(3)]
        if not with_sens:  # (sensors disabled: sensordata is the caller's in every pass)
            for t in Ds:
                t.zero_()
    if c.B == 0 or nv == 0:
        return tuple(t.zero_() for t in Df) + tuple(Ds)
    pf = [_ptr(t) for t in Df]
    ps = [_ptr(t if with_sens else None) for t in (Ds or [None] * 3)]
    cen = int(bool(centered))

    def difference(lib, h, f0, s0, f1, s1, c0, n, st):
        return lib.mjh_ifd_difference(h, f0, s0, f1, s1, c.B, c0, n, c.eps, cen, *pf, *ps, st)

    _drive("inverse_fd", c, m, d, centered, False, difference, inverse=True)
    return tuple(Df) + tuple(Ds)


def _cotangent(name, what, g, batch, n, dtype, device):
    """``g`` checked against ``batch + (n,)`` in the call's dtype and on its device, and made contiguous."""
    if not isinstance(g, torch.Tensor):
        raise ValueError(f"{name}: {what} must be a tensor of shape {batch + (n,)}, got {type(g).__name__}")
    if tuple(g.shape) != batch + (n,):
        raise ValueError(f"{name}: {what} has shape {tuple(g.shape)}, expected {batch + (n,)} (the batch shape of the Data, then {n})")
    if g.dtype != dtype:
        raise ValueError(f"{name}: {what} is {g.dtype}, the Data {dtype}")
    if g.device != device:
        raise ValueError(f"{name}: {what} is on {g.device}, the Data on {device}")
    return g.detach().contiguous()


def _vjp(name, c: _Call, m, d, g_state, g_sensor, centered, fixed_iterations, nominal=None):
    """``gx``, ``gu`` of validated, contiguous cotangents (``g_sensor`` may be None)."""
    gx = torch.empty(c.batch + (c.ns,), dtype=c.dtype, device=c.device)
    gu = torch.empty(c.batch + (c.nu,), dtype=c.dtype, device=c.device)
    if c.B == 0 or c.ns == 0:
        return gx.zero_(), gu.zero_()
    pg, pgs, pgx, pgu = _ptr(g_state), _ptr(g_sensor if c.sens_written else None), _ptr(gx), _ptr(gu)
    cen = int(bool(centered))

    def contract(lib, h, pin, py0, pscr_out, c0, n, st):
        return lib.mjh_fd_vjp(h, pin, py0, pscr_out, c.B, c0, n, c.eps, cen, pg, pgs, pgx, pgu, st)

    _drive(name, c, m, d, centered, fixed_iterations, contract, nominal)
    return gx, gu


@_outside_graphs
def transition_vjp(m: Model, d: Data, g_state: torch.Tensor, g_sensor: torch.Tensor | None = None, eps: float = 1e-6, centered: bool = False,
                   fixed_iterations: bool = False, *, max_scratch_bytes: int | None = None):
    """The vector-Jacobian product of ``transition_fd``'s Jacobians, without forming them: ``gx = A^T g_state + C^T g_sensor``: ``S + (ns,)`` and
    ``gu = B^T g_state + D^T g_sensor``: ``S + (nu,)``.

    ``g_state``: ``S + (ns,)``, the cotangent of the next state in the order of ``x``: ``[dq (nv, tangent space), qvel (nv), act (na)]``;
    ``g_sensor``: ``S + (nsensordata,)`` or None.  ``gx`` is in the same tangent-space order (``tangent_pull`` / ``tangent_push`` map the ``qpos``
    part from and to ``qpos`` coordinates).  ``eps``, ``centered``, ``fixed_iterations`` and ``max_scratch_bytes`` are ``transition_fd``'s, and
    so are the perturbed steps, the control-range rule and the caveat on ``fixed_iterations``: ``mjh_fd_vjp`` (``csrc/mjh_fd.h``) takes the place of
    ``mjh_fd_difference`` and contracts each entry with the cotangent where that one stores it.  One wavefront sums a column, in an order that
    depends on the number of rows alone: the result is the same bits from call to call and for every ``max_scratch_bytes``.  With sensors disabled
    ``g_sensor`` contributes nothing (``C = D = 0``).
    """
    name = "transition_vjp"
    c = _validate(name, m, d, eps, max_scratch_bytes)
    g_state = _cotangent(name, "g_state", g_state, c.batch, c.ns, c.dtype, c.device)
    if g_sensor is not None:
        g_sensor = _cotangent(name, "g_sensor", g_sensor, c.batch, c.nsd, c.dtype, c.device)
    _on_device(c, m)
    return _vjp(name, c, m, d, g_state, g_sensor, centered, fixed_iterations)


def _tangent(name, m: Model, qpos: torch.Tensor, g: torch.Tensor, mode: int) -> torch.Tensor:
    fw = sys.modules[__package__ + ".forward"]
    if torch.compiler.is_compiling() or not fw._plain(qpos) or not fw._plain(g):
        raise NotImplementedError(f"{name} cannot be used under torch.vmap / torch.compile: there is no operator for it.")
    nq, nv = int(m.nq), int(m.nv)
    if qpos.shape[-1:] != (nq,):
        raise ValueError(f"{name}: qpos has shape {tuple(qpos.shape)}, expected (..., {nq})")
    batch, dtype, device = tuple(qpos.shape[:-1]), qpos.dtype, qpos.device
    if dtype != m.qpos0.dtype or dtype not in (torch.float64, torch.float32):
        raise ValueError(f"{name}: qpos is {dtype}, the Model {m.qpos0.dtype}: it runs in the model's dtype, float64 or float32")
    n_in, n_out = (nq, nv) if mode == 0 else (nv, nq)
    g = _cotangent(name, "the cotangent", g, batch, n_in, dtype, device)
    fw._require_device(device)
    out = torch.empty(batch + (n_out,), dtype=dtype, device=device)
    B = int(math.prod(batch)) if batch else 1
    if B == 0 or nv == 0:
        return out.zero_()
    nm = native.get_native_model(m, device, dtype)
    _bind(nm.lib)
    qpos = qpos.detach().contiguous()
    stream, prev = fw._stream_and_guard(device)
    try:
        rc = nm.lib.mjh_fd_tangent(nm.handle, _ptr(qpos), _ptr(g), _ptr(out), B, mode, ctypes.c_void_p(stream))
    finally:
        if prev is not None:
            torch.cuda.set_device(prev)
    if rc != 0:
        raise RuntimeError(f"native {name} failed ({rc}): {nm.lib.mjh_last_error().decode()}")
    return out


@_outside_graphs
def tangent_pull(m: Model, qpos: torch.Tensor, g_qpos: torch.Tensor) -> torch.Tensor:
    """A cotangent of ``qpos`` (``S + (nq,)``) brought to the tangent space at ``qpos`` (``S + (nv,)``): the entry itself for slide / hinge joints
    and free translations; for the rotational dof ``k`` of a ball / free joint with quaternion ``q``, ``<g_qpos[quaternion], q (x) (0, e_k)> / 2``:
    the adjoint of ``delta -> q (x) exp(delta / 2)``, the convention ``transition_fd`` perturbs and differences in."""
    return _tangent("tangent_pull", m, qpos, g_qpos, 0)


@_outside_graphs
def tangent_push(m: Model, qpos: torch.Tensor, g_tangent: torch.Tensor) -> torch.Tensor:
    """A tangent-space cotangent at ``qpos`` (``S + (nv,)``) in ``qpos`` coordinates (``S + (nq,)``): the entry itself, or for a quaternion ``q``
    ``2 sum_k g_k q (x) (0, e_k) / |q|^2``.  That is the cotangent whose ``tangent_pull`` is ``g_tangent`` and whose component along ``q`` -- the
    radial one -- is zero by definition: how a step depends on the norm of a quaternion is not differentiated.  An all-zero quaternion, which the
    library's normalisation leaves at zero and no perturbation moves, receives zeros."""
    return _tangent("tangent_push", m, qpos, g_tangent, 1)


_DIFFERENTIATED = ("qpos", "qvel", "act", "ctrl")


def _refuse_other_leaves(d: Data, sens_written: bool):
    """A floating leaf other than qpos / qvel / act / ctrl that requires grad would silently receive none.  ``sensordata`` is let through where
    the step computes it: the step does not read the incoming values then, so their gradient is zero and that zero is right -- which is what lets
    ``differentiable_step`` be applied to its own result, whose ``sensordata`` carries a graph.  With sensors disabled the leaf is carried through
    the step, and stays refused."""
    def scan(obj, prefix):
        for k, v in obj._fields.items():  # (leaves still lazy belong to a step's output slab and carry no graph)
            if isinstance(v, torch.Tensor):
                if not prefix and k == "sensordata" and sens_written:
                    continue
                if v.requires_grad and v.is_floating_point() and (prefix or k not in _DIFFERENTIATED):
                    raise ValueError(f"differentiable_step: Data.{prefix}{k} requires grad, but gradients are computed for "
                                     f"{', '.join(_DIFFERENTIATED)} only; detach it (a silent zero gradient would be wrong)")
            elif hasattr(v, "_fields"):
                scan(v, f"{prefix}{k}.")
    scan(d, "")


class _Job:
    """One ``differentiable_step`` call, handed through ``torch.autograd.Function.apply`` as a single opaque argument."""

    __slots__ = ("m", "d", "c", "centered", "fixed_iterations", "out", "names")


class _Step(torch.autograd.Function):
    @staticmethod
    def forward(ctx, job, qpos, qvel, act, ctrl):
        job.out = y0 = job.c.fw._run_native(job.m, job.d, job.fixed_iterations, True)  # exactly the launches of step
        outs = tuple(getattr(y0, n) for n in job.names)
        ctx.job = job
        ctx.save_for_backward(qpos, qvel, act, ctrl, *outs)  # (the saved-tensor checks refuse a backward after an in-place write to any of them)
        return outs

    @staticmethod
    @torch.autograd.function.once_differentiable  # native launches: a second-order request is an error, not a gradient without a graph
    def backward(ctx, *grads):
        job, saved = ctx.job, ctx.saved_tensors
        c, m = job.c, job.m
        qpos, y = saved[0], dict(zip(job.names, saved[4:]))
        g = [gr if gr is not None else torch.zeros_like(y[n]) for n, gr in zip(job.names, grads)]
        g = dict(zip(job.names, g))
        nv = c.nv
        g_state = torch.cat([tangent_pull(m, y["qpos"], g["qpos"].contiguous()), g["qvel"], g["act"]], dim=-1)
        g_sens = g["sensordata"].contiguous() if "sensordata" in g else None
        nominal = native.DataPtrs()
        arr = np.frombuffer(nominal, dtype=np.uint64)
        for n in job.names:
            arr[c.fw._IDX[n]] = y[n].data_ptr() if y[n].numel() else 0
        gx, gu = _vjp("differentiable_step", c, m, job.d, g_state, g_sens, job.centered, job.fixed_iterations, nominal)
        gq = tangent_push(m, qpos, gx[..., :nv].contiguous())
        return None, gq, gx[..., nv:2 * nv], gx[..., 2 * nv:], gu


@_outside_graphs
def differentiable_step(m: Model, d: Data, eps: float = 1e-6, centered: bool = True, fixed_iterations: bool = True, *,
                        max_scratch_bytes: int | None = None) -> Data:
    """``step`` with a ``torch.autograd`` graph: ``loss.backward()`` through the native step (the reference's ``differentiable_mode`` use case).

    Forward runs exactly the launches of ``step(m, d, fixed_iterations)``: every leaf of the result is that step's, bit for bit.  ``qpos``,
    ``qvel``, ``act`` and (where the model computes sensors) ``sensordata`` of the result carry a ``grad_fn``; no other leaf is differentiable.
    Backward returns gradients for ``d.qpos``, ``d.qvel``, ``d.act`` and ``d.ctrl`` -- nothing else: if any other floating leaf of ``d``
    (``qfrc_applied``, ``xfrc_applied``, ``mocap_pos`` ...) requires grad, the call raises ``ValueError`` rather than hand it a silent zero.  The
    Model's parameters are not differentiated either.

    The gradients are FINITE-DIFFERENCE derivatives, not analytic ones: backward is ``tangent_pull`` of the ``qpos`` cotangent at the stepped
    ``qpos``, the chunk loop of ``transition_vjp`` (reusing the forward's result as the nominal step) and ``tangent_push`` at ``d.qpos``, i.e.
    ``ns + nu`` extra environment-steps per environment and backward, twice that when ``centered`` (the default here: the truncation error is then
    ``O(eps^2)``).  The gradient of ``d.qpos`` has no component along a quaternion (see ``tangent_push``).  A control at the edge of its
    ``actuator_ctrlrange`` gets the one-sided difference ``transition_fd`` documents, or zero when neither side can be taken.

    ``fixed_iterations`` is passed to the forward step and to every perturbed one.  With early termination the solver may stop after a different
    number of iterations in two of the steps, and their difference over ``eps`` is then solver tolerance over ``eps`` rather than a derivative:
    that is why it defaults to ``True`` here (``step`` defaults to ``False``; for a model without constraint rows the two agree bit for bit).
    ``step`` itself stays as it is, without a graph.

    The result can be stepped again (``for _ in range(T): d = differentiable_step(m, d)``) and a loss on the last state backpropagates through
    every step.  Backward runs once per graph: ``create_graph=True`` through it raises.  It re-steps from ``d``: ``d.qpos``, ``d.qvel``, ``d.act``,
    ``d.ctrl`` and the stepped state are saved tensors, and autograd refuses a backward after an in-place write to one of them, but the other
    leaves the step reads (``qfrc_applied``, ``xfrc_applied``, ``mocap_*``, ``qacc_warmstart``, ``time``, ``eq_active`` ...) are held by reference
    and are NOT checked: do not write to them in place between forward and backward (``replace`` makes a new Data and is safe).

    Under ``torch.vmap`` the call raises ``NotImplementedError``.  It is kept out of ``torch.compile`` graphs: inside a ``fullgraph=True`` region
    Dynamo refuses it as an unsupported call; without ``fullgraph`` Dynamo breaks the graph at the call and runs it eagerly, with the same result
    as outside ``torch.compile``.  The same holds for ``transition_vjp``, ``tangent_pull`` and ``tangent_push``.
    """
    name = "differentiable_step"
    c = _validate(name, m, d, eps, max_scratch_bytes)
    _refuse_other_leaves(d, c.sens_written)
    _on_device(c, m)
    job = _Job()
    job.m, job.d, job.c, job.centered, job.fixed_iterations, job.out = m, d, c, bool(centered), bool(fixed_iterations), None
    job.names = ("qpos", "qvel", "act") + (("sensordata",) if c.sens_written else ())
    outs = _Step.apply(job, d.qpos, d.qvel, d.act, d.ctrl)
    y0, job.out = job.out, None
    return y0.replace(**dict(zip(job.names, outs)))
