"""Throughput of ``mujoco_torch_amd.ray`` (rays/s), its kernel time and HBM share, against ``forward`` on the same batch as a scale reference.

For each (model, dtype, B, R): one forward pass poses the batch; after a warm-up, ``ray`` and ``forward`` calls alternate, each timed with HIP events
on the current stream.  The ray kernel (timing id 21) is timed on its own through the library's per-launch events (mjh_debug_phase_timing).  Its
bytes are counted here from what the kernel touches: the candidates' geom_xpos / geom_xmat (12 reals each per environment), the rays (pnt / vec
as passed) and the outputs (dist + int64 geomid per ray); the triangle table and the sizes are shared by every lane (cache-resident).
Prints one JSON line.

    python tools/ray_throughput.py [--steps 20] [--warmup 5]
"""
import argparse
import ctypes
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mujoco-torch_amd"))

import mujoco_torch_amd as mt  # noqa: E402
from mujoco_torch_amd import native  # noqa: E402

R_ = importlib.import_module("mujoco_torch_amd.ray")
HBM_BYTES_PER_S = 8e12
# (model, dtype, B, rays per environment)
CONFIGS = [("humanoid", torch.float64, 4096, 64), ("ant", torch.float32, 16384, 32), ("mesh_contact", torch.float32, 8192, 64)]


def rays(B, R, dtype, seed=0):
    """An 8 x 8 (or fewer) downward height scan around the origin, the rest a horizontal ring at 0.5 m."""
    rng = np.random.RandomState(seed)
    n_scan = min(64, R // 2) if R < 64 else 64
    side = int(np.sqrt(n_scan))
    n_scan = side * side
    xy = np.stack(np.meshgrid(np.linspace(-1, 1, side), np.linspace(-1, 1, side)), -1).reshape(-1, 2)
    P = np.zeros((B, R, 3))
    V = np.zeros((B, R, 3))
    P[:, :n_scan, :2] = xy + 0.05 * rng.randn(B, n_scan, 2)
    P[:, :n_scan, 2] = 2.0
    V[:, :n_scan, 2] = -1.0
    k = R - n_scan
    if k:
        a = np.linspace(0, 2 * np.pi, k, endpoint=False)
        P[:, n_scan:, 2] = 0.5
        V[:, n_scan:, 0], V[:, n_scan:, 1] = np.cos(a), np.sin(a)
    return torch.tensor(P, dtype=dtype, device="cuda"), torch.tensor(V, dtype=dtype, device="cuda")


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
    for xml, dtype, B, R in CONFIGS:
        mx = mt.device_put(mt.mjcf.from_xml_path(mt.test_data_path(xml + ".xml")), dtype=None if dtype == torch.float64 else dtype)
        mdev = mx.to("cuda")
        rng = np.random.RandomState(0)
        d = mt.make_data(mx).expand(B).clone()
        d = d.replace(qvel=torch.tensor(0.05 * rng.randn(B, mx.nv)))
        d = mt.forward(mdev, (d.to(dtype) if dtype != torch.float64 else d).to("cuda"))
        P, V = rays(B, R, dtype)
        for _ in range(args.warmup):
            mt.ray(mdev, d, P, V)
            mt.forward(mdev, d)
        torch.cuda.synchronize()
        ray_ms, fwd_ms = [], []
        for _ in range(args.steps):
            ray_ms += timed(lambda: mt.ray(mdev, d, P, V), 1)
            fwd_ms += timed(lambda: mt.forward(mdev, d), 1)
        lib.mjh_debug_phase_timing(1)
        kern = []
        for _ in range(args.steps):
            mt.ray(mdev, d, P, V)
            ms, ids = (ctypes.c_float * 96)(), (ctypes.c_int * 96)()
            n = lib.mjh_debug_phase_times(ms, ids, 96)
            kern += [ms[i] for i in range(n) if ids[i] == 21]
        lib.mjh_debug_phase_timing(0)
        c = R_.candidates(mx.tables.ray, R_.filter_key(mx.tables.ray, (), True, -1))
        rb = torch.empty((), dtype=dtype).element_size()
        nbytes = B * (len(c["geom"]) * 12 * rb + 2 * R * 3 * rb + R * (rb + 8))
        k_ms = float(np.median(kern))
        r_ms = float(np.median(ray_ms))
        res.append(dict(model=xml, dtype=str(dtype).split(".")[-1], B=B, R=R, ncand=int(len(c["geom"])), ntri=int(len(c["tri"])),
                        ray_ms=r_ms, rays_per_s=B * R / (r_ms * 1e-3), forward_ms=float(np.median(fwd_ms)),
                        kernel_ms=k_ms, kernel_rays_per_s=B * R / (k_ms * 1e-3), kernel_bytes=nbytes,
                        kernel_roofline_share=nbytes / (k_ms * 1e-3) / HBM_BYTES_PER_S))
    print(json.dumps(dict(tool="ray_throughput", device=torch.cuda.get_device_name(), steps=args.steps, warmup=args.warmup, results=res)))


if __name__ == "__main__":
    main()
