"""Kernel time of one ``fwd_postconstraint`` launch next to the forward pass that produced its inputs, and the HBM bound.

For each (model, dtype, B): a few steps load the contacts, then ``forward`` and ``fwd_postconstraint(sensors=False)`` are timed through the library's
per-launch events (mjh_debug_phase_timing): the forward pass as the sum of its launches, the new kernel by its id (MJH_KERNEL_POSTCON = 32).  The bytes
are the library's own account per environment (mjh_model_kernel_io).  Prints one JSON line.

    python tools/postcon_throughput.py [--steps 30] [--warmup 5]
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
from mujoco_torch_amd._postpass import handle as _handle  # noqa: E402

HBM_BYTES_PER_S = 8e12
POSTCON = 32
CONFIGS = [("humanoid", torch.float64, 4096), ("ant", torch.float32, 16384)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    lib = native.load_library()
    res = []
    for xml, dtype, B in CONFIGS:
        mx = mt.device_put(mt.mjcf.from_xml_path(mt.test_data_path(xml + ".xml")), dtype=None if dtype == torch.float64 else dtype)
        mdev = mx.to("cuda")
        rng = np.random.RandomState(0)
        d = mt.make_data(mx).expand(B).clone()
        d = d.replace(qvel=torch.tensor(0.05 * rng.randn(B, mx.nv)), xfrc_applied=torch.tensor(rng.randn(B, mx.nbody, 6)))
        d = (d.to(dtype) if dtype != torch.float64 else d).to("cuda")
        for _ in range(3):
            d = mt.step(mdev, d)
        f = mt.forward(mdev, d)
        for _ in range(args.warmup):
            mt.forward(mdev, d), mt.fwd_postconstraint(mdev, f)
        torch.cuda.synchronize()

        def launches(fn):
            per_call = []
            for _ in range(args.steps):
                fn()
                ms, kid = (ctypes.c_float * 96)(), (ctypes.c_int * 96)()
                n = lib.mjh_debug_phase_times(ms, kid, 96)
                per_call.append([(kid[i], ms[i]) for i in range(n)])
            return per_call

        lib.mjh_debug_phase_timing(1)
        fwd = launches(lambda: mt.forward(mdev, d))
        post = launches(lambda: mt.fwd_postconstraint(mdev, f))
        fwd2 = launches(lambda: mt.forward(mdev, d))  # (again, behind the other: the spread of the yardstick itself)
        lib.mjh_debug_phase_timing(0)
        med = lambda calls: float(np.median([sum(t for _, t in c) for c in calls]))
        assert all(len(c) == 1 and c[0][0] == POSTCON for c in post), post[0]
        io = (ctypes.c_int64 * 2)()
        rc = lib.mjh_model_kernel_io(_handle(mdev, torch.device("cuda", torch.cuda.current_device()), dtype).handle, POSTCON, io)
        assert rc == 0, rc
        nbytes = B * (io[0] + io[1])
        k_ms = med(post)
        res.append(dict(model=xml, dtype=str(dtype).split(".")[-1], B=B, forward_ms=med(fwd), forward_again_ms=med(fwd2), forward_launches=[k for k, _ in fwd[0]],
                        postcon_ms=k_ms, postcon_min_ms=float(min(sum(t for _, t in c) for c in post)), read_bytes_per_env=int(io[0]), written_bytes_per_env=int(io[1]),
                        hbm_bound_ms=nbytes / HBM_BYTES_PER_S * 1e3, hbm_share=nbytes / (k_ms * 1e-3) / HBM_BYTES_PER_S))
    print(json.dumps(dict(tool="postcon_throughput", device=torch.cuda.get_device_name(), steps=args.steps, warmup=args.warmup, results=res)))


if __name__ == "__main__":
    main()
