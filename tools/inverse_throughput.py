"""Throughput of ``mujoco_torch_amd.inverse`` against ``forward`` on the same batch, and the inverse tail's share of the HBM roofline.

For each (model, batch): one forward pass gives a consistent qacc; after a warm-up, ``inverse`` and ``forward`` calls alternate, each timed with HIP
events on the current stream.  The inverse-tail kernel (timing id 20) is timed on its own through the library's per-launch events
(mjh_debug_phase_timing), and its algorithmic bytes come from mjh_model_kernel_io(20).  Prints one JSON line.  Kernel times from a profiler:
run this under ``rocprofv3 --kernel-trace --stats -- python tools/inverse_throughput.py`` and read mjh_inverse_kernel in the stats.

    python tools/inverse_throughput.py [--steps 20] [--warmup 5]
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

HBM_BYTES_PER_S = 8e12
CONFIGS = [("humanoid", 4096), ("humanoid", 32768), ("ant", 4096), ("ant", 32768)]


def state(mx, B, seed):
    rng = np.random.RandomState(seed)
    return mt.make_data(mx).expand(B).clone().replace(qvel=torch.tensor(0.05 * rng.randn(B, mx.nv)))


def timed(fn, steps):
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    lib = native.load_library()
    res = []
    for xml, B in CONFIGS:
        mx = mt.device_put(mt.mjcf.from_xml_path(mt.test_data_path(xml + ".xml")))
        mdev = mx.to("cuda")
        d = mt.forward(mdev, state(mx, B, 0).to("cuda"))
        for _ in range(args.warmup):
            mt.inverse(mdev, d)
            mt.forward(mdev, d)
        torch.cuda.synchronize()
        inv_ms, fwd_ms = [], []
        for _ in range(args.steps):  # alternating: both see the same clocks and the same L2 state
            inv_ms += timed(lambda: mt.inverse(mdev, d), 1)
            fwd_ms += timed(lambda: mt.forward(mdev, d), 1)
        lib.mjh_debug_phase_timing(1)
        kern = []
        for _ in range(args.steps):
            mt.inverse(mdev, d)
            ms, ids = (ctypes.c_float * 96)(), (ctypes.c_int * 96)()
            n = lib.mjh_debug_phase_times(ms, ids, 96)
            kern += [ms[i] for i in range(n) if ids[i] == 20]
        lib.mjh_debug_phase_timing(0)
        nm = native.get_native_model(mdev, torch.device("cuda", torch.cuda.current_device()), torch.float64)
        rw = (ctypes.c_int64 * 2)()
        assert lib.mjh_model_kernel_io(nm.handle, 20, rw) == 0
        per_env = int(rw[0] + rw[1])
        k_ms = float(np.median(kern))
        res.append(dict(model=xml, dtype="float64", B=B, nefc=int(mx.constraint_sizes_py[4]), nv=int(mx.nv),
                        inverse_ms=float(np.median(inv_ms)), forward_ms=float(np.median(fwd_ms)),
                        inverse_env_steps_per_s=B / (float(np.median(inv_ms)) * 1e-3), forward_env_steps_per_s=B / (float(np.median(fwd_ms)) * 1e-3),
                        tail_kernel_ms=k_ms, tail_bytes_per_env=per_env, tail_bytes=per_env * B,
                        tail_roofline_share=per_env * B / (k_ms * 1e-3) / HBM_BYTES_PER_S))
    print(json.dumps(dict(tool="inverse_throughput", device=torch.cuda.get_device_name(), steps=args.steps, warmup=args.warmup, results=res)))


if __name__ == "__main__":
    main()
