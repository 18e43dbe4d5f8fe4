"""Pair evaluations per second of ``geom_distance`` per type pair, and which limit each one runs against.

The scene is the tests' (tests/golden/geom_distance.xml), its geoms at seeded random poses within their own sizes of a common point (about half of the pairs
overlap), B = 4096 environments, both dtypes.  For each type pair the call is timed twice: with the pair listed once (4096 items: one call as a user makes it)
and listed ``--repeat`` times (the same work over and over: enough items to fill the device).  Times are HIP events around the call on a synchronised device,
after a warm-up, and the kernel alone through the library's per-launch events (mjh_debug_phase_timing, kernel id MJH_KERNEL_GEOM_DISTANCE = 47).

An item reads two geom frames and sizes and its table row and writes 7 reals (mjh_model_kernel_io's account: 30 reals + 16 bytes in, 7 reals out).  ``bound``
says which limit the long list runs against: "bandwidth" when those bytes move at more than half of the HBM rate (the list repeats one pair, so the caches
serve most of the reads: the rate is the kernel's demand, not HBM traffic), "launch" when even the long list takes less than twice the one-pair call, else
"compute"; ``single_call_bound`` is
"launch" (the launch and one wave's latency: 4096 items are 64 waves, a quarter of the device's compute units) when an item of the one-pair call costs more than
four times what it costs in the long list.  Prints one JSON line.

    python tools/geom_distance_throughput.py [--steps 30] [--warmup 5] [--repeat 64]
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

PLANE, SPHERE, CAPSULE, ELLIPSOID, CYLINDER, BOX = 0, 2, 3, 4, 5, 6  # mjtGeom
HBM_BYTES_PER_S = 8e12
GEOM_DISTANCE = 47
B = 4096
# geom ids of the scene: plane 0, spheres 1 2, capsules 3 4, boxes 5 6, ellipsoid 7, cylinder 8
PAIRS = {"sphere-sphere": (1, 2), "sphere-capsule": (2, 4), "capsule-capsule": (3, 4), "sphere-box": (2, 6), "capsule-box": (4, 6), "box-box": (5, 6),
         "plane-sphere": (0, 2), "plane-capsule": (0, 4), "plane-box": (0, 6), "plane-ellipsoid": (0, 7), "plane-cylinder": (0, 8)}


def reach(gtype, size):
    """Radius of a ball about the geom's centre that holds it (the plane: anywhere among the large geoms)."""
    return {PLANE: 10.0, SPHERE: size[0], CAPSULE: size[0] + size[1], BOX: float(np.linalg.norm(size)), ELLIPSOID: float(size.max()), CYLINDER: float(np.hypot(size[0], size[1]))}[int(gtype)]


def random_rotations(rng, n):
    """n rotation matrices [n, 3, 3] from seeded unit quaternions."""
    q = rng.randn(n, 4)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeat", type=int, default=64)
    args = ap.parse_args()
    lib = native.load_library()
    res = []
    for dtype in (torch.float64, torch.float32):
        mx = mt.device_put(mt.mjcf.from_xml_path(os.path.join(ROOT, "tests", "golden", "geom_distance.xml")), dtype=None if dtype == torch.float64 else dtype)
        mdev = mx.to("cuda")
        gtype, size = np.asarray(mx.tables.ray["geom_type"]).astype(int), mx.geom_size.numpy()
        rng = np.random.RandomState(0)
        radius = np.array([reach(t, s) for t, s in zip(gtype, size)])
        xpos = rng.randn(B, 1, 3) + 0.3 * radius[None, :, None] * rng.randn(B, len(gtype), 3)
        xmat = random_rotations(rng, B * len(gtype)).reshape(B, len(gtype), 3, 3)
        d = mt.make_data(mx).expand(B).clone()
        d = (d.to(dtype) if dtype != torch.float64 else d).replace(geom_xpos=torch.tensor(xpos).to(dtype), geom_xmat=torch.tensor(xmat).to(dtype)).to("cuda")
        io = (ctypes.c_int64 * 2)()
        assert lib.mjh_model_kernel_io(_handle(mdev, torch.device("cuda", torch.cuda.current_device()), dtype).handle, GEOM_DISTANCE, io) == 0
        for name, (g1, g2) in PAIRS.items():
            row = dict(pair=name, dtype=str(dtype).split(".")[-1], B=B, read_bytes_per_item=int(io[0]), written_bytes_per_item=int(io[1]))
            for label, P in (("single", 1), ("list", args.repeat)):
                call = lambda: mt.geom_distance(mdev, d, [g1] * P, [g2] * P, 1e9)
                for _ in range(args.warmup):
                    call()
                torch.cuda.synchronize()
                wall = []
                for _ in range(args.steps):
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    call()
                    t1.record()
                    t1.synchronize()
                    wall.append(t0.elapsed_time(t1))
                lib.mjh_debug_phase_timing(1)
                kern = []
                for _ in range(args.steps):
                    call()
                    ms, kid = (ctypes.c_float * 96)(), (ctypes.c_int * 96)()
                    n = lib.mjh_debug_phase_times(ms, kid, 96)
                    assert n == 1 and kid[0] == GEOM_DISTANCE, [(kid[i], ms[i]) for i in range(n)]
                    kern.append(ms[0])
                lib.mjh_debug_phase_timing(0)
                k_s, items = 1e-3 * float(np.median(kern)), B * P
                row.update({f"{label}_pairs": P, f"{label}_kernel_us": 1e6 * k_s, f"{label}_kernel_min_us": 1e3 * float(min(kern)),
                            f"{label}_call_us": 1e3 * float(np.median(wall)), f"{label}_evaluations_per_s": items / k_s,
                            f"{label}_bytes_per_s": items * (io[0] + io[1]) / k_s})
            row["hbm_share"] = row["list_bytes_per_s"] / HBM_BYTES_PER_S
            row["hbm_bound_us"] = 1e6 * B * args.repeat * (io[0] + io[1]) / HBM_BYTES_PER_S
            row["bound"] = "bandwidth" if row["hbm_share"] > 0.5 else ("launch" if row["list_kernel_us"] < 2 * row["single_kernel_us"] else "compute")
            row["single_efficiency"] = row["list_kernel_us"] / args.repeat / row["single_kernel_us"]  # an item's time in the long list over its time in the one-pair call
            row["single_call_bound"] = "launch" if row["single_efficiency"] < 0.25 else row["bound"]
            res.append(row)
    print(json.dumps(dict(tool="geom_distance_throughput", device=torch.cuda.get_device_name(), steps=args.steps, warmup=args.warmup, repeat=args.repeat,
                          results=res)))


if __name__ == "__main__":
    main()
