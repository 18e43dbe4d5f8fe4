"""Kernel time of ``solve`` next to the kernels of the pass that made its inputs, and the largest centipede it serves.

Two workloads on the benchmark's input recipe (small random velocities and controls): the humanoid at B = 4096 in float64 with CG and the ant at B = 16384 in float32
with Newton, each with the model's own options.  ``forward`` makes the pass; ``solve`` then runs (a) on that Data as it is -- its warm start is the pass's own
solution, what a re-solve of a finished pass costs -- and (b) from a cold start, ``qacc_warmstart = qacc_smooth``, the work the pass's own solver phase does after a
reset.  The kernels are timed through the library's per-launch events (mjh_debug_phase_timing; ``solve``: kernel id 56), ``--steps`` times after ``--warmup`` warm-up
calls, every variant inside one loop; medians and minima are reported, with the kernels of one ``forward`` at the same batch (ids and times) beside them and the
library's own account of the bytes (``mjh_model_kernel_io``) with the time they take at 8 TB/s.  ``fits`` lists, per solver and dtype, the largest bundled
``centipede_*`` model whose working set fits the plan (``solver.plan``; dofs, rows, LDS bytes).  No ratio is asserted: the figures are the record.  Prints one JSON line.

    python tools/solve_throughput.py [--steps 20] [--warmup 3]
"""
import argparse
import ctypes
import glob
import json
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mujoco-torch_amd"))

import mujoco_torch_amd as mt  # noqa: E402
from mujoco_torch_amd import native  # noqa: E402
from mujoco_torch_amd import solver  # noqa: E402

WORKLOADS = (("humanoid", {"solver": 1}, torch.float64, 4096), ("ant", {"solver": 2}, torch.float32, 16384))
KERNEL_SOLVE = 56
HBM_BYTES_PER_S = 8e12


def launches(lib, call):
    call()
    ms, kid = (ctypes.c_float * 64)(), (ctypes.c_int * 64)()
    n = lib.mjh_debug_phase_times(ms, kid, 64)
    return [(int(kid[i]), float(ms[i])) for i in range(n)]


def fits():
    """{solver: {dtype: (model, nv, nefc, LDS bytes)}}: the largest bundled centipede the plan admits."""
    out = {}
    names = sorted(glob.glob(mt.test_data_path("centipede*.xml")), key=lambda p: int((re.findall(r"_(\d+)\.xml$", p) or ["72"])[0]))
    sizes = []
    for p in names:
        mc = mt.device_put(mt.mjcf.from_xml_path(p))
        sizes.append((os.path.basename(p)[:-4], int(mc.nv), int(mc.constraint_sizes_py[4])))
    for s in (mt.SolverType.CG, mt.SolverType.NEWTON):
        for dtype in (torch.float64, torch.float32):
            best = None
            for name, nv, nefc in sizes:
                try:
                    best = (name, nv, nefc, solver.plan(s, nv, nefc, dtype)[3])
                except RuntimeError:
                    pass
            out.setdefault(s.name, {})[str(dtype).split(".")[-1]] = best
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    lib = native.load_library()
    res = []
    for xml, ov, dtype, B in WORKLOADS:
        spec = mt.mjcf.from_xml_path(mt.test_data_path(xml + ".xml"))
        for k, v in ov.items():
            setattr(spec.opt, k, v)
        mc = mt.device_put(spec, dtype=None if dtype == torch.float64 else dtype)
        mx = mc.to("cuda")
        rng = np.random.RandomState(42)
        d0 = mt.make_data(mc).expand(B).clone()
        d0 = d0.replace(qvel=torch.tensor(0.01 * rng.randn(B, mc.nv)), ctrl=torch.tensor(0.3 * rng.randn(B, mc.nu)))
        d0 = (d0.to(dtype) if dtype != torch.float64 else d0).to("cuda")
        d = mt.forward(mx, d0)
        cold = d.replace(qacc_warmstart=d.qacc_smooth.clone())
        nv, nefc = int(mc.nv), int(mc.constraint_sizes_py[4])
        nm = native.get_native_model(mx, torch.device("cuda", 0), dtype)
        rw = (ctypes.c_int64 * 2)()
        assert lib.mjh_model_kernel_io(nm.handle, KERNEL_SOLVE, rw) == 0
        calls = {"warm": lambda: mt.solve(mx, d), "cold": lambda: mt.solve(mx, cold), "forward": lambda: mt.forward(mx, d0)}
        for _ in range(args.warmup):
            for c in calls.values():
                c()
        torch.cuda.synchronize()
        t = {k: [] for k in calls}
        lib.mjh_debug_phase_timing(1)
        for _ in range(args.steps):
            for k, c in calls.items():
                t[k].append(launches(lib, c))
        lib.mjh_debug_phase_timing(0)
        rows = {}
        for k in ("warm", "cold"):
            assert all(len(x) == 1 and x[0][0] == KERNEL_SOLVE for x in t[k]), t[k][0]
            ks = [x[0][1] for x in t[k]]
            _, st = mt.solve(mx, d if k == "warm" else cold, stats=True)
            rows[k] = dict(kernel_us=1e3 * float(np.median(ks)), kernel_min_us=1e3 * float(min(ks)), mean_niter=float(st.niter.float().mean()), max_niter=int(st.niter.max()))
        ids = [kid for kid, _ in t["forward"][0]]
        fwd = [dict(kernel=kid, us=1e3 * float(np.median([x[i][1] for x in t["forward"]]))) for i, kid in enumerate(ids)]
        res.append(dict(model=xml, solver=mt.SolverType(int(mc.opt.solver)).name, dtype=str(dtype).split(".")[-1], B=B, nv=nv, nefc=nefc, iterations=int(mc.opt.iterations),
                        ls_iterations=int(mc.opt.ls_iterations), plan=list(solver.plan(mc.opt.solver, nv, nefc, dtype)), bytes_per_env=int(rw[0] + rw[1]),
                        hbm_bound_us=(rw[0] + rw[1]) * B / HBM_BYTES_PER_S * 1e6, solve=rows, forward_kernels=fwd))
    print(json.dumps(dict(tool="solve_throughput", device=torch.cuda.get_device_name(), steps=args.steps, warmup=args.warmup, fits=fits(), results=res)))


if __name__ == "__main__":
    main()
