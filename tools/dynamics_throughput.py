"""Kernel time of ``tendon`` / ``transmission`` / ``passive`` / ``fwd_velocity`` / ``fwd_actuation`` / ``fwd_acceleration`` next to the kernels of the whole pass.

Two workloads on the benchmark's input recipe (small random velocities and controls): the humanoid at B = 4096 in float64 and the ant at B = 16384 in float32, each
with the model's own options.  ``forward`` makes the pass; each function then runs on that Data as it is (a function that returns ``d`` itself for the model --
``tendon`` without tendons -- is reported as ``null``).  The kernels are timed through the library's per-launch events (mjh_debug_phase_timing; kernel ids 63 + op, and
61 / 62 for the ``com_vel`` / ``rne`` launches inside ``fwd_velocity``), read after every native call, ``--steps`` times after ``--warmup`` warm-up calls, every
function inside one loop; medians and minima are reported per launch, with the kernels of one ``forward`` at the same batch (ids and times) beside them and the
launch plan (lanes, environments per workgroup, reals of LDS per environment).  There is no threshold: these functions re-run a part of a pass and are not a faster
step; the figures are the record.  Prints one JSON line.

    python tools/dynamics_throughput.py [--steps 20] [--warmup 3]
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
from mujoco_torch_amd import dynamics, native, smooth  # noqa: E402

WORKLOADS = (("humanoid", torch.float64, 4096), ("ant", torch.float32, 16384))
FUNCTIONS = ("tendon", "transmission", "passive", "fwd_velocity", "fwd_actuation", "fwd_acceleration")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    lib = native.load_library()
    seen = []

    def recording(real):  # the timing aid keeps the launches of the most recent native call: read them after each one
        def call(*a, **k):
            real(*a, **k)
            ms, kid = (ctypes.c_float * 64)(), (ctypes.c_int * 64)()
            n = lib.mjh_debug_phase_times(ms, kid, 64)
            seen.extend((int(kid[i]), float(ms[i])) for i in range(n))
        return call

    real_calls = dynamics.call, smooth.call
    res = []
    for xml, dtype, B in WORKLOADS:
        mc = mt.device_put(mt.mjcf.from_xml_path(mt.test_data_path(xml + ".xml")), dtype=None if dtype == torch.float64 else dtype)
        mx = mc.to("cuda")
        rng = np.random.RandomState(42)
        d0 = mt.make_data(mc).expand(B).clone()
        d0 = d0.replace(qvel=torch.tensor(0.01 * rng.randn(B, mc.nv)), ctrl=torch.tensor(0.3 * rng.randn(B, mc.nu)))
        d0 = (d0.to(dtype) if dtype != torch.float64 else d0).to("cuda")
        d = mt.forward(mx, d0)
        for _ in range(args.warmup):
            mt.forward(mx, d0)
            for fn in FUNCTIONS:
                getattr(mt, fn)(mx, d)
        torch.cuda.synchronize()
        t = {fn: [] for fn in FUNCTIONS + ("forward",)}
        lib.mjh_debug_phase_timing(1)
        dynamics.call, smooth.call = recording(real_calls[0]), recording(real_calls[1])
        try:
            for _ in range(args.steps):
                for fn in FUNCTIONS:
                    del seen[:]
                    out = getattr(mt, fn)(mx, d)
                    t[fn].append(None if out is d else list(seen))
                mt.forward(mx, d0)
                ms, kid = (ctypes.c_float * 64)(), (ctypes.c_int * 64)()
                n = lib.mjh_debug_phase_times(ms, kid, 64)
                t["forward"].append([(int(kid[i]), float(ms[i])) for i in range(n)])
        finally:
            dynamics.call, smooth.call = real_calls
            lib.mjh_debug_phase_timing(0)
        rows = {}
        for fn in FUNCTIONS + ("forward",):
            if t[fn][0] is None:
                rows[fn] = None
                continue
            ids = [kid for kid, _ in t[fn][0]]
            assert all([kid for kid, _ in x] == ids for x in t[fn]), (fn, t[fn][0])
            per = [dict(kernel=kid, us=1e3 * float(np.median([x[i][1] for x in t[fn]])), min_us=1e3 * float(min(x[i][1] for x in t[fn]))) for i, kid in enumerate(ids)]
            rows[fn] = dict(launches=per, us=sum(p["us"] for p in per))
        plans = {op: list(dynamics.plan(op, mc, dtype)) for op in dynamics.OPS}
        res.append(dict(model=xml, dtype=str(dtype).split(".")[-1], B=B, nv=int(mc.nv), nu=int(mc.nu), nbody=int(mc.nbody), plans=plans, kernels=rows))
    print(json.dumps(dict(tool="dynamics_throughput", device=torch.cuda.get_device_name(), steps=args.steps, warmup=args.warmup, results=res)))


if __name__ == "__main__":
    main()
