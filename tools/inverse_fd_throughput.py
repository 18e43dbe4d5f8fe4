"""What ``mujoco_torch_amd.inverse_fd`` costs beyond the inverse passes it runs.

Humanoid, float64, ``B`` environments (default 256), one-sided: ``3 nv = 81`` columns, ``B * 81`` perturbed environments in one chunk under the default
scratch budget.  After a warm-up, one ``inverse_fd`` call and the same number of environments through ``inverse`` alone (the nominal batch, then
one batch of ``B * 81``: the way ``inverse_fd`` cuts them) alternate, each timed with HIP events on the current stream.  The bytes are the library's
own account (``mjh_model_kernel_io``): per slot for the two kernels of ``inverse_fd`` (ids 45, 46), per environment for the kernels an ``inverse``
call launches (their ids come from the library's per-launch events).  Prints one JSON line.

Kernel times come from a profiler run of its own: ``rocprofv3 --kernel-trace --stats -- python tools/inverse_fd_throughput.py --calls 20`` runs
nothing but ``--calls`` calls of ``inverse_fd`` after one warm-up call; read ``mjh_ifd_perturb_kernel``, ``mjh_ifd_difference_kernel`` and the
others in the kernel stats.

    python tools/inverse_fd_throughput.py [--batch 256] [--steps 20] [--warmup 5] [--calls 0]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mujoco-torch_amd"))

import mujoco_torch_amd as mt  # noqa: E402
from mujoco_torch_amd import native  # noqa: E402

IFD_PERTURB, IFD_DIFFERENCE = 45, 46


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=0, help="profiler mode: run this many inverse_fd calls and nothing else")
    args = ap.parse_args()
    B = args.batch
    lib = native.load_library()
    mx = mt.device_put(mt.mjcf.from_xml_path(mt.test_data_path("humanoid.xml")))
    mdev = mx.to("cuda")
    rng = np.random.RandomState(0)
    d0 = mt.make_data(mx).expand(B).clone().replace(qvel=torch.tensor(0.05 * rng.randn(B, mx.nv)))
    d = mt.forward(mdev, d0.to("cuda"))  # a consistent qacc
    ncol = 3 * int(mx.nv)
    if args.calls:
        mt.inverse_fd(mdev, d)
        torch.cuda.synchronize()
        for _ in range(args.calls):
            mt.inverse_fd(mdev, d)
        torch.cuda.synchronize()
        print(json.dumps(dict(tool="inverse_fd_throughput", mode="profile", B=B, columns=ncol, calls=args.calls)))
        return
    rep = d[torch.arange(B).repeat_interleave(ncol)]  # as many environments as the scratch batch holds
    for _ in range(args.warmup):
        mt.inverse_fd(mdev, d)
        mt.inverse(mdev, d)
        mt.inverse(mdev, rep)
    torch.cuda.synchronize()
    scr = list(mdev.tables.__dict__["_fd_scratch"].values())[-1]
    assert scr.slots == B * ncol, "one chunk expected: lower --batch or raise the budget"
    fd_ms, inv_ms = [], []
    for _ in range(args.steps):  # alternating: both see the same clocks
        fd_ms.append(timed(lambda: mt.inverse_fd(mdev, d)))
        inv_ms.append(timed(lambda: (mt.inverse(mdev, d), mt.inverse(mdev, rep))))
    # bytes: the two new kernels per slot, the kernels of one inverse call per environment
    nm = native.get_native_model(mdev, torch.device("cuda", torch.cuda.current_device()), torch.float64)
    rw = (ctypes.c_int64 * 2)()

    def io(k):  # (None: the library keeps no account of that kernel on its own for this model)
        return (int(rw[0]), int(rw[1])) if lib.mjh_model_kernel_io(nm.handle, k, rw) == 0 else None

    lib.mjh_debug_phase_timing(1)
    mt.inverse(mdev, rep)
    ms, ids = (ctypes.c_float * 96)(), (ctypes.c_int * 96)()
    n = lib.mjh_debug_phase_times(ms, ids, 96)
    lib.mjh_debug_phase_timing(0)
    launched = [int(ids[i]) for i in range(n)]
    pass_io = {k: io(k) for k in sorted(set(launched))}
    pass_bytes = sum(sum(v) for v in pass_io.values() if v is not None)
    pert, diff = io(IFD_PERTURB), io(IFD_DIFFERENCE)
    fd, inv = float(np.median(fd_ms)), float(np.median(inv_ms))
    print(json.dumps(dict(tool="inverse_fd_throughput", device=torch.cuda.get_device_name(), model="humanoid", dtype="float64", B=B, columns=ncol,
                          slots=B * ncol, steps=args.steps, warmup=args.warmup, scratch_bytes=int(scr.slab.numel()),
                          inverse_fd_ms=fd, inverse_fd_ms_min_max=[min(fd_ms), max(fd_ms)], inverse_alone_ms=inv, inverse_alone_ms_min_max=[min(inv_ms), max(inv_ms)],
                          beyond_the_passes_frac=(fd - inv) / inv, inverse_pass_kernel_ids=launched, inverse_pass_kernel_ms=[float(ms[i]) for i in range(n)],
                          inverse_pass_io_bytes_per_env={str(k): v for k, v in pass_io.items()}, inverse_pass_bytes_per_env=pass_bytes,
                          inverse_pass_kernels_without_account=[k for k, v in pass_io.items() if v is None],
                          ifd_perturb_bytes_per_slot=pert, ifd_difference_bytes_per_slot=diff,
                          new_kernels_byte_ratio=(sum(pert) + sum(diff)) / pass_bytes if pass_bytes else None)))


if __name__ == "__main__":
    main()
