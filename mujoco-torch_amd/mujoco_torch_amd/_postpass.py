"""The host side every function on a finished pass shares (``support``, ``postconstraint``, ``contact_sensors``, ``energy``, ``integrate``, ``jacobian``; ``ray`` and
``render`` use the handle, the caches and the call): the native model of a call, the refusal under ``torch.vmap`` / ``torch.compile``, the batch / dtype / device /
shape checks of the Data's leaves, host values kept on the device, and the call into the library.  Which leaves a call reads, what it returns and in which order
it checks stay with each module.

``forward._require_device`` / ``_stream_and_guard`` and ``native.get_native_model`` are looked up on their modules when a function runs, never bound at import:
the host tests replace them.  The two modules themselves are imported once, at first use (``_module``): an import statement inside a function costs more than
the checks around it, and at import time they cannot load yet (``device`` imports ``ray``, and with it this module, while ``native`` is waiting for ``device``).
"""

from __future__ import annotations

import ctypes
import importlib

import numpy as np
import torch

_MODULES = {}
_HANDLES = {}  # (tables uid, device, dtype) -> a NativeModel of that structure: these entry points read the structure from it, the values come with each call
_HOST = {}  # (tables uid, name, dtype, device) -> (the bytes of a host value, its device copy)


def _module(name):
    mod = _MODULES.get(name)
    if mod is None:
        mod = _MODULES[name] = importlib.import_module("." + name, __package__)  # (``forward``: the module; the package's attribute of that name is the function)
    return mod


def cached(cache: dict, key, make, valid=None, limit: int = 256):
    """``cache[key]``, made by ``make()`` when it is missing or ``valid(entry)`` is false; a cache past ``limit`` entries is emptied first."""
    hit = cache.get(key)
    if hit is None or (valid is not None and not valid(hit)):
        if len(cache) > limit:
            cache.clear()
        hit = cache[key] = make()
    return hit


def handle(m, device, dtype):
    return cached(_HANDLES, (m.tables.uid, device, dtype), lambda: _module("native").get_native_model(m, device, dtype), limit=64)


def refuse_tracing(name, *tensors):
    plain = _module("forward")._plain
    if torch.compiler.is_compiling() or not all(plain(t) for t in tensors if isinstance(t, torch.Tensor)):
        raise NotImplementedError(f"{name} cannot be used under torch.vmap / torch.compile: there is no operator for it.  Call it on a "
                                  "batched Data directly (every leading dimension of a leaf is the batch).")


def require_device(device):
    _module("forward")._require_device(device)


# ---- checks -----------------------------------------------------------------------------------------------------------------

def probe(name: str, m, n: str, leaf, tail: tuple):
    """(batch, dtype, device) of a Data from the leaf ``n`` of trailing shape ``tail``; the dtype is float64 or float32 and the Model's."""
    shape = tuple(getattr(leaf, "shape", ()))
    if not isinstance(leaf, torch.Tensor) or len(shape) < len(tail) or shape[-len(tail):] != tail:
        raise ValueError(f"{name}: {n} has shape {shape}, expected (..., {', '.join(str(s) for s in tail)}) for this Model")
    dtype = leaf.dtype
    if dtype not in (torch.float64, torch.float32):
        raise ValueError(f"{name}: unsupported Data dtype {dtype}")
    if dtype != m.qpos0.dtype:
        raise ValueError(f"{name}: the Data is {dtype}, the Model {m.qpos0.dtype}: it runs in the model's dtype")
    return shape[:-len(tail)], dtype, leaf.device


def check_leaves(name: str, leaves: dict, tails: dict, batch: tuple, dtype, device, flat: int, ints: dict = {}):
    """Every leaf is ``batch + tails[n]`` -- a tail of ``flat`` dimensions may come with its last two merged (``flat=3``: matrices as ``(n, 9)``; ``flat=2``:
    ``(n, m)`` as ``(n * m,)``) -- of ``dtype`` (``ints[n]`` for an integer leaf) on ``device``."""
    for n, t in leaves.items():
        tail = tails[n]
        want = batch + tail
        if tuple(t.shape) != want and not (len(tail) == flat and tuple(t.shape) == batch + tail[:-2] + (tail[-2] * tail[-1],)):
            raise ValueError(f"{name}: {n} has shape {tuple(t.shape)}, expected {want} for a Data of batch shape {batch}")
        if t.dtype != ints.get(n, dtype) or t.device != device:
            raise ValueError(f"{name}: {n} is {t.dtype} on {t.device}, expected {ints.get(n, dtype)} on {device}")


def check_override(name: str, n: str, t, shape: tuple, dtype, device, what: str):
    """An ``n=`` argument that stands in for a leaf (``qpos=``, ``qvel=``, ``vec=``): a tensor of ``shape`` in the Data's dtype on its device."""
    if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape:
        raise ValueError(f"{name}: {n}= must have shape {shape} ({what}); got {tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
    if t.dtype != dtype or t.device != device:
        raise ValueError(f"{name}: {n}= is {t.dtype} on {t.device}, the Data is {dtype} on {device}")


# ---- values -----------------------------------------------------------------------------------------------------------------

def upload(m, name, value, dtype, device):
    """A host value of the Model (read at each call) on the device: uploaded again only when its values changed."""
    arr = np.ascontiguousarray(np.asarray(value, dtype=np.float64))
    key = arr.tobytes()
    return cached(_HOST, (m.tables.uid, name, dtype, device), lambda: (key, torch.tensor(arr, dtype=dtype, device=device).contiguous()),
                  valid=lambda hit: hit[0] == key, limit=1024)[1]


def model_value(m, name, value, dtype, device):
    """A value of the caller's Model on the device: a tensor is converted where it lives, a host value goes through ``upload``."""
    return value.detach().to(device=device, dtype=dtype).contiguous() if isinstance(value, torch.Tensor) else upload(m, name, value, dtype, device)


# ---- the call ---------------------------------------------------------------------------------------------------------------

def bind(args, tensors: dict):
    """Sets the pointer fields of ``args`` from ``{field: tensor}``.  An empty tensor is skipped (its field stays NULL); one that is not contiguous is passed as a
    contiguous copy.  ``args`` keeps every tensor it points to alive, so they last as long as the struct does."""
    keep = args.__dict__.setdefault("_keep", [])
    for n, t in tensors.items():
        if t.numel() == 0:
            continue
        if not t.is_contiguous():
            t = t.contiguous()
        keep.append(t)
        setattr(args, n, t.data_ptr())


def call(name: str, m, symbol: str, args, device, dtype, what: str | None = None):
    """``symbol(handle, args, stream)`` on the caller's current stream: ``args`` is a filled args struct (``native.ARGS[symbol]``), or the tuple of positional
    arguments between the handle and the stream.  A library without the symbol and a non-zero return are ``RuntimeError``s."""
    nm = handle(m, device, dtype)
    fn = getattr(nm.lib, symbol, None)
    if fn is None:
        raise RuntimeError(f"{_module('native').LIB_PATH} predates {what or name} (no {symbol}): rebuild the library")
    argv = args if isinstance(args, tuple) else (ctypes.byref(args),)
    stream, prev = _module("forward")._stream_and_guard(device)
    try:
        rc = fn(nm.handle, *argv, ctypes.c_void_p(stream))
    finally:
        if prev is not None:
            torch.cuda.set_device(prev)
    if rc != 0:
        raise RuntimeError(f"native {name} failed ({rc}): {nm.lib.mjh_last_error().decode()}")
