"""The workload behind the measured time of the plane-ellipsoid / plane-cylinder narrow phase (mjh_quadric_kernel).

Steps the test scene tests/golden/quadric.xml (five plane-cylinder and two plane-ellipsoid pairs per environment: 7 items, 17 contacts) at a user-sized
batch from jittered poses.  Meant to run under the profiler, in a run of its own:

    rocprofv3 --kernel-trace --stats -d OUT -o quadric -- python tools/quadric_profile.py [--batch 4096] [--steps 50] [--dtype float64]

and read the rows of ``mjh_quadric_kernel`` in what the profiler wrote under OUT (its kernel statistics: a csv file with ``--output-format csv``, else the
``kernels`` view of its database).  With or without a profiler it prints the library's own per-launch events (mjh_debug_phase_timing) for the
kernel's id (MJH_KERNEL_QUADRIC = 44) as one JSON line.
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

QUADRIC = 44


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--dtype", default="float64", choices=["float64", "float32"])
    args = ap.parse_args()
    dtype = getattr(torch, args.dtype)
    lib = native.load_library()
    mx = mt.device_put(mt.mjcf.from_xml_path(os.path.join(ROOT, "tests", "golden", "quadric.xml")), dtype=None if dtype == torch.float64 else dtype)
    mdev = mx.to("cuda")
    B = args.batch
    rng = np.random.RandomState(0)
    d = mt.make_data(mx).expand(B).clone()
    q = d.qpos.clone()
    for j in range(mx.njnt):
        a = int(mx.jnt_qposadr[j])
        if int(mx.jnt_type.data[j]) == 0:
            q[:, a : a + 3] += torch.tensor(0.01 * rng.randn(B, 3))
            q[:, a + 3 : a + 7] += torch.tensor(0.05 * rng.randn(B, 4))
        else:
            q[:, a] += torch.tensor(0.5 * rng.randn(B))
    d = d.replace(qpos=q, qvel=torch.tensor(0.3 * rng.randn(B, mx.nv)))
    d = (d.to(dtype) if dtype != torch.float64 else d).to("cuda")
    for _ in range(args.warmup):
        d = mt.step(mdev, d)
    torch.cuda.synchronize()
    lib.mjh_debug_phase_timing(1)
    us = []
    for _ in range(args.steps):
        d = mt.step(mdev, d)
        ms, kid = (ctypes.c_float * 96)(), (ctypes.c_int * 96)()
        n = lib.mjh_debug_phase_times(ms, kid, 96)
        us += [1e3 * ms[i] for i in range(n) if kid[i] == QUADRIC]
    lib.mjh_debug_phase_timing(0)
    assert us, "the step launched no quadric kernel"
    rw = (ctypes.c_int64 * 2)()
    assert lib.mjh_model_kernel_io(native.get_native_model(mdev, torch.device("cuda"), dtype).handle, QUADRIC, rw) == 0
    print(json.dumps({"model": "quadric", "dtype": args.dtype, "batch": B, "launches": len(us), "quadric_event_us_median": float(np.median(us)),
                      "quadric_event_us_min": float(np.min(us)), "bytes_per_env": [int(rw[0]), int(rw[1])]}))


if __name__ == "__main__":
    main()
