"""``transition_fd``: finite-difference Jacobians of one ``step`` with respect to state and control (MuJoCo's ``mjd_transitionFD``).

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
"""

from __future__ import annotations

import ctypes
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
    lib._fd_bound = True


class _Scratch:
    """The scratch batch of ``slots`` environments: one allocation, and the two pointer structs (inputs, step outputs) into it."""

    __slots__ = ("slab", "inp", "out", "slots")


def _leaf_bytes(fw, counts, dtype):
    """Bytes per environment of every ABI leaf."""
    esize = torch.empty((), dtype=dtype).element_size()
    size = np.full(fw._NLEAF, esize, dtype=np.int64)
    for n, dt in fw._INT_DTYPE.items():
        size[fw._IDX[n]] = 4 if dt == torch.int32 else 8
    return np.asarray(counts, dtype=np.int64) * size


def _make_scratch(fw, in_idx, extra_idx, extra_bytes, out_idx, leaf_bytes, slots, device) -> _Scratch:
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
    s.slab = torch.empty(off, dtype=torch.uint8, device=device)
    base = s.slab.data_ptr()
    for arr, idx, o in where:
        arr[idx] = base + o
    return s


def transition_fd(m: Model, d: Data, eps: float = 1e-6, centered: bool = False, sensors: bool = False, fixed_iterations: bool = False, *,
                  max_scratch_bytes: int | None = None):
    """Finite-difference Jacobians of ``step`` (MuJoCo's ``mjd_transitionFD``): ``A, B`` or, with ``sensors=True``, ``A, B, C, D``.

    With the state ``x = [dq (nv, tangent space), qvel (nv), act (na)]``, ``ns = 2 nv + na``, ``u = ctrl`` and ``y`` the state after one step:
    ``A = dy/dx``: ``S + (ns, ns)``, ``B = dy/du``: ``S + (ns, nu)``, ``C = dsensordata/dx``: ``S + (nsensordata, ns)``, ``D = dsensordata/du``:
    ``S + (nsensordata, nu)``, ``S`` being the batch shape of ``d``.  Rows are outputs, columns what was perturbed: ``A[..., i, j] = dy_i / dx_j``.
    A model without sensors returns ``C``, ``D`` with a zero first dimension.

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
    fw = sys.modules[__package__ + ".forward"]  # (the package attribute `forward` is the function)
    try:
        eps = float(eps)
    except (TypeError, ValueError):
        raise ValueError(f"eps must be a positive number, got {eps!r}") from None
    if not eps > 0 or math.isinf(eps):
        raise ValueError(f"eps must be a positive finite number, got {eps}")
    qpos = d.qpos
    if torch.compiler.is_compiling() or not fw._plain(qpos):
        raise NotImplementedError("transition_fd cannot be used under torch.vmap / torch.compile: there is no operator for it.  Call it on a "
                                  "batched Data directly (every leading dimension of a leaf is the batch).")
    dtype = qpos.dtype
    mdtype = m.qpos0.dtype
    if dtype != mdtype:
        raise ValueError(f"the Data is {dtype}, the Model {mdtype}: transition_fd runs in the model's dtype")
    if dtype not in (torch.float64, torch.float32):
        raise ValueError(f"unsupported dtype {dtype}: transition_fd runs in float64 or float32")
    if not float(torch.tensor(eps, dtype=dtype)) > 0:
        raise ValueError(f"eps = {eps} rounds to zero in {dtype}")
    budget = MAX_SCRATCH_BYTES if max_scratch_bytes is None else int(max_scratch_bytes)
    if budget <= 0:
        raise ValueError(f"max_scratch_bytes must be positive, got {max_scratch_bytes}")
    device = qpos.device
    fw._require_device(device)
    batch = tuple(qpos.shape[:-1])
    B = int(math.prod(batch)) if batch else 1
    nv, na, nu, nsd = int(m.nv), int(m.na), int(m.nu), int(getattr(m, "nsensordata", 0) or 0)
    ns, nside = 2 * nv + na, 2 if centered else 1
    ncol = ns + nu
    A = torch.empty(batch + (ns, ns), dtype=dtype, device=device)
    Bm = torch.empty(batch + (ns, nu), dtype=dtype, device=device)
    C = D = None
    written = fw._written_names(m, True)
    with_sens = bool(sensors) and nsd > 0 and "sensordata" in written
    if sensors:
        C = torch.empty(batch + (nsd, ns), dtype=dtype, device=device)
        D = torch.empty(batch + (nsd, nu), dtype=dtype, device=device)
        if not with_sens:  # (sensors disabled: sensordata is the caller's in every step)
            C.zero_()
            D.zero_()
    if B == 0 or ns == 0:
        return (A.zero_(), Bm.zero_()) + ((C, D) if sensors else ())

    # ---- the nominal step; the caller's pointer table ----
    y0 = fw._run_native(m, d, bool(fixed_iterations), True)
    nm = native.get_native_model(m, device, dtype)
    _bind(nm.lib)
    T = m.tables
    tab = fw._table(d, (T.uid, dtype, device, B), nm.leaf_counts, B, dtype, device)
    extra = T.sensors["extra_leaves"]
    keep = fw._extra_inputs(tab, d, extra, B, int(m.nbody), dtype, device) if extra else None  # noqa: F841  (contiguous copies live until the launches are enqueued)
    y0tab = y0.__dict__["_ptab"]

    # ---- the scratch batch ----
    stream, prev = fw._stream_and_guard(device)
    try:
        in_idx = tuple(fw._IDX[n] for n in _INPUT_LEAVES if tab.arr[fw._IDX[n]] != 0)
        esize = torch.empty((), dtype=dtype).element_size()
        extra_idx = tuple(k for k, n in enumerate(fw._EXTRA_NAMES) if extra and n in extra and tab.xarr[k] != 0)
        extra_bytes = tuple(int(m.nbody) * fw._EXTRA_WIDTH[fw._EXTRA_NAMES[k]] * esize for k in extra_idx)
        out_idx = tuple(fw._IDX[n] for n in written)
        leaf_bytes = _leaf_bytes(fw, nm.leaf_counts, dtype)
        per_slot = int(leaf_bytes[list(in_idx)].sum() + sum(extra_bytes) + leaf_bytes[list(out_idx)].sum()) + int(nm.work_bytes)
        cols = int(max(1, min(ncol, budget // max(1, per_slot * B * nside))))
        slots = B * cols * nside
        pool = T.__dict__.setdefault("_fd_scratch", {})
        key = (device, dtype, stream, slots, in_idx, extra_idx)
        scr = pool.pop(key, None)
        if scr is None:
            while len(pool) >= _SCRATCH_KEPT:
                pool.pop(next(iter(pool)))
            scr = _make_scratch(fw, in_idx, extra_idx, extra_bytes, out_idx, leaf_bytes, slots, device)
        pool[key] = scr  # (most recently used last)
        work = nm.workspace(slots, stream)
        wptr = ctypes.c_void_p(work.data_ptr() if work is not None else None)
        flags = native.FLAG_FIXED_ITERATIONS if fixed_iterations else 0
        lib, h, st = nm.lib, nm.handle, ctypes.c_void_p(stream)
        pin, pscr_in, pscr_out, py0 = ctypes.byref(tab.struct), ctypes.byref(scr.inp), ctypes.byref(scr.out), ctypes.byref(y0tab.struct)
        ptr = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None and t.numel() else None)
        pA, pB, pC, pD = ptr(A), ptr(Bm), ptr(C if with_sens else None), ptr(D if with_sens else None)
        for c0 in range(0, ncol, cols):
            n = min(cols, ncol - c0)
            rc = lib.mjh_fd_perturb(h, pin, pscr_in, B, c0, n, eps, int(bool(centered)), st)
            if rc == 0:
                rc = lib.mjh_step(h, pscr_in, pscr_out, wptr, B * n * nside, flags, st)
            if rc == 0:
                rc = lib.mjh_fd_difference(h, pin, py0, pscr_out, B, c0, n, eps, int(bool(centered)), pA, pB, pC, pD, st)
            if rc != 0:
                raise RuntimeError(f"native transition_fd failed ({rc}): {lib.mjh_last_error().decode()}")
    finally:
        if prev is not None:
            torch.cuda.set_device(prev)
    return (A, Bm) + ((C, D) if sensors else ())
