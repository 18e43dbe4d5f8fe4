"""Throughput of ``mujoco_torch_amd.render`` (pixels/s), its kernel time and HBM share, against ``step`` on the same batch as a scale reference.

For each (model, dtype, B, image, shadows): one forward pass poses the batch; after a warm-up, ``render`` and ``step`` calls alternate, each timed
with HIP events on the current stream.  The render kernel (timing id 22) is timed on its own through the library's per-launch events
(mjh_debug_phase_timing).  Its bytes are counted from what the kernel touches: the candidates' geom_xpos / geom_xmat (12 reals each per environment),
the camera and light poses, and the outputs (rgb in the call's dtype, depth, int64 seg per pixel); the triangle table, sizes, colours and light rows
are shared by every lane (cache-resident).  Models without a camera get one looking at the origin.  Prints one JSON line.

    python tools/render_throughput.py [--steps 20] [--warmup 5]
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

R_ = importlib.import_module("mujoco_torch_amd.render")
RAY = importlib.import_module("mujoco_torch_amd.ray")
HBM_BYTES_PER_S = 8e12
DATA = os.path.dirname(mt.test_data_path("ant.xml"))
CAM = '<camera name="look" pos="0.1 -1.0 0.6" xyaxes="1 0 0 0 0.3 1" fovy="45"/>'
# (model, dtype, B, width, height, camera, shadows)
CONFIGS = [("humanoid", torch.float64, 4096, 64, 64, 1, False), ("humanoid", torch.float64, 4096, 64, 64, 1, True),
           ("ant", torch.float32, 16384, 64, 64, 2, False), ("mesh_contact", torch.float32, 8192, 64, 64, 0, False)]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    lib = native.load_library()
    res = []
    for xml, dtype, B, W, H, cam, shadows in CONFIGS:
        text = open(os.path.join(DATA, xml + ".xml")).read()
        if "<camera" not in text:
            text = text.replace("<worldbody>", "<worldbody>\n    " + CAM, 1)
        mx = mt.device_put(mt.mjcf.from_xml_string(text, base_dir=DATA), dtype=None if dtype == torch.float64 else dtype)
        mdev = mx.to("cuda")
        rng = np.random.RandomState(0)
        d = mt.make_data(mx).expand(B).clone()
        d = d.replace(qvel=torch.tensor(0.05 * rng.randn(B, mx.nv)))
        d = mt.forward(mdev, (d.to(dtype) if dtype != torch.float64 else d).to("cuda"))
        kw = dict(camera_id=cam, width=W, height=H, shadows=shadows)
        for _ in range(args.warmup):
            mt.render(mdev, d, **kw)
            mt.step(mdev, d)
        torch.cuda.synchronize()
        ren_ms, step_ms = [], []
        for _ in range(args.steps):
            ren_ms.append(timed(lambda: mt.render(mdev, d, **kw)))
            step_ms.append(timed(lambda: mt.step(mdev, d)))
        lib.mjh_debug_phase_timing(1)
        kern = []
        for _ in range(args.steps):
            rgb, _, _ = mt.render(mdev, d, **kw)
            ms, ids = (ctypes.c_float * 96)(), (ctypes.c_int * 96)()
            n = lib.mjh_debug_phase_times(ms, ids, 96)
            kern += [ms[i] for i in range(n) if ids[i] == 22]
        lib.mjh_debug_phase_timing(0)
        c = RAY.candidates(mx.tables.ray, (True, (), ()))
        rb = torch.empty((), dtype=dtype).element_size()
        nl = int(mx.nlight)
        pix = B * W * H
        nbytes = B * (len(c["geom"]) * 12 + 12 + 6 * nl) * rb + pix * (3 * rgb.element_size() + rb + 8)
        k_ms, r_ms = float(np.median(kern)), float(np.median(ren_ms))
        res.append(dict(model=xml, dtype=str(dtype).split(".")[-1], B=B, width=W, height=H, shadows=shadows, ncand=int(len(c["geom"])),
                        ntri=int(len(c["tri"])), nlight=nl, render_ms=r_ms, pixels_per_s=pix / (r_ms * 1e-3), step_ms=float(np.median(step_ms)),
                        kernel_ms=k_ms, kernel_pixels_per_s=pix / (k_ms * 1e-3), kernel_bytes=nbytes,
                        kernel_roofline_share=nbytes / (k_ms * 1e-3) / HBM_BYTES_PER_S))
    print(json.dumps(dict(tool="render_throughput", device=torch.cuda.get_device_name(), steps=args.steps, warmup=args.warmup, results=res)))


if __name__ == "__main__":
    main()
