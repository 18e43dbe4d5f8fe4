"""The host side ``solve_pgs`` and ``solve_noslip`` share (``csrc/mjh_dual.h`` has what their kernels share): the checks of ``iterations``, ``tolerance``, ``force0``
and ``Model.stat.meaninertia``, the six outputs, and the library's plan of a call.  Which leaves a call reads, its defaults, the cone / condim refusals, the order of
the checks and what an empty problem returns stay with each module.
"""

from __future__ import annotations

import ctypes
import operator

import torch

from . import native


def check_sweeps(name: str, iterations, tolerance) -> tuple[int, float]:
    """``iterations`` as an int in [0, 2^31) and ``tolerance`` as a float >= 0."""
    try:
        iterations = operator.index(iterations)
    except TypeError:
        raise ValueError(f"{name}: iterations must be an integer >= 0; got {iterations!r}") from None
    if iterations < 0 or iterations >= 2 ** 31:
        raise ValueError(f"{name}: iterations must be an integer >= 0; got {iterations!r}")
    tolerance = float(tolerance)
    if not tolerance >= 0:
        raise ValueError(f"{name}: tolerance must be >= 0; got {tolerance!r}")
    return iterations, tolerance


def check_force0(name: str, force0, batch: tuple, nefc: int, dtype, device) -> int:
    """A ``force0=`` argument: ``batch + (nefc,)`` or ``(nefc,)`` (shared) in the Data's dtype on its device; returns its element stride per environment (0: shared)."""
    if not isinstance(force0, torch.Tensor) or tuple(force0.shape) not in (batch + (nefc,), (nefc,)):
        got = tuple(force0.shape) if isinstance(force0, torch.Tensor) else type(force0).__name__
        raise ValueError(f"{name}: force0= must have shape {batch + (nefc,)} (per environment) or {(nefc,)} (shared); got {got}")
    if force0.dtype != dtype or force0.device != device:
        raise ValueError(f"{name}: force0= is {force0.dtype} on {force0.device}, the Data is {dtype} on {device}")
    return nefc if tuple(force0.shape) == batch + (nefc,) and batch else 0


def check_meaninertia(name: str, m) -> float:
    meaninertia = float(m.stat.meaninertia)
    if not meaninertia > 0:
        raise ValueError(f"{name}: Model.stat.meaninertia is {meaninertia}, expected a positive number")
    return meaninertia


def new_outputs(batch: tuple, nefc: int, nv: int, dtype, device) -> dict:
    """The six outputs of a call, uninitialised, in the order of the result tuples."""
    new = lambda *tail, dt=dtype: torch.empty(batch + tail, dtype=dt, device=device)
    return dict(efc_force=new(nefc), qfrc_constraint=new(nv), qacc=new(nv), cost=new(), improvement=new(), niter=new(dt=torch.int32))


def plan(what: str, symbol: str, sizes: dict, dtype, holds: str) -> tuple[int, int, int, int]:
    """``symbol(*sizes.values(), bytes of a real, out)``, the library's plan of one ``what`` call (a host computation).  A library without the symbol and a model
    that does not fit a workgroup's LDS (``holds``: what has to fit) are ``RuntimeError``s; the latter names the sizes."""
    lib = native.load_library()
    fn = getattr(lib, symbol, None)
    if fn is None:
        raise RuntimeError(f"{native.LIB_PATH} predates {what} (no {symbol}): rebuild the library")
    out = (ctypes.c_int * 4)()
    rc = fn(*(int(v) for v in sizes.values()), 8 if dtype == torch.float64 else 4, out)
    if rc == -12:
        raise RuntimeError(f"{what}: {', '.join(f'{k} = {v}' for k, v in sizes.items())} in {dtype} need {out[3]} bytes of LDS ({holds}); "
                           f"a workgroup has {160 * 1024}")
    if rc != 0:
        raise RuntimeError(f"{what.removeprefix('solve_')}.plan failed ({rc}): {lib.mjh_last_error().decode()}")
    return tuple(out)
