"""Environment-sweeps per second of ``solve_pgs`` and what it costs against the composition a user could write before it: ``efc_ar`` (the Delassus matrix in
global memory) followed by the projected Gauss-Seidel row loop in torch, one row of every environment at a time.

Two workloads: the humanoid at B = 4096 in float64 and the ant with frictionloss rows at B = 16384 in float32, on the leaves of this library's own ``forward`` on
the benchmark's input recipe (small random velocities and controls), ``tolerance = 0`` and a fixed number of sweeps (``--sweeps``), from zeros.  Both are timed the
same way: HIP events around the call on the current stream, ``--steps`` times after ``--warmup`` warm-up calls, alternating the new call and the composition inside
one loop so that a drift of the machine hits both; the median and the minimum are reported.  The kernel is also timed alone through the library's per-launch
events (mjh_debug_phase_timing, kernel id 54), at ``--sweeps`` sweeps and at none: the difference is the sweeps themselves, the rest is staging ``efc_J``, the
forward substitution and the tail.  ``ratio`` is the composition's median time over the new call's: below 1 the composition is faster, and it is printed as it
comes out.  The two forces are compared (they solve the same problem in another summation order).  Prints one JSON line.

    python tools/pgs_throughput.py [--sweeps 8] [--steps 20] [--warmup 3]
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

WORKLOADS = (("humanoid", torch.float64, 4096), ("ant_frictionloss", torch.float32, 16384))
KERNEL_ID = 54


def timed(call):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    call()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def composition(mx, d, sweeps):
    """``efc_ar`` and the row loop in torch: the force after ``sweeps`` sweeps from zeros."""
    ne, nf, _, _, nefc = (int(x) for x in mx.constraint_sizes_py)
    fl = d.efc_frictionloss

    def run():
        AR, b = mt.efc_ar(mx, d)
        f = torch.zeros_like(b)
        diag = torch.diagonal(AR, dim1=-2, dim2=-1)
        for _ in range(sweeps):
            for i in range(nefc):
                res = (AR[:, i, :] * f).sum(-1) + b[:, i]
                ok = diag[:, i] > 0
                new = f[:, i] - res / torch.where(ok, diag[:, i], torch.ones_like(res))
                if ne <= i < ne + nf:
                    new = torch.minimum(torch.maximum(new, -fl[:, i]), fl[:, i])
                elif i >= ne + nf:
                    new = new.clamp_min(0)
                f[:, i] = torch.where(ok, new, f[:, i])
        return f

    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweeps", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    lib = native.load_library()
    res = []
    for xml, dtype, B in WORKLOADS:
        mc = mt.device_put(mt.mjcf.from_xml_path(mt.test_data_path(xml + ".xml")), dtype=None if dtype == torch.float64 else dtype)
        mx = mc.to("cuda")
        rng = np.random.RandomState(42)
        d = mt.make_data(mc).expand(B).clone()
        d = d.replace(qvel=torch.tensor(0.01 * rng.randn(B, mc.nv)), ctrl=torch.tensor(0.3 * rng.randn(B, mc.nu)))
        d = mt.forward(mx, (d.to(dtype) if dtype != torch.float64 else d).to("cuda"))
        nefc, nv = int(mc.constraint_sizes_py[4]), int(mc.nv)
        new = lambda k=args.sweeps: mt.solve_pgs(mx, d, iterations=k, tolerance=0.0)
        old = composition(mx, d, args.sweeps)
        for _ in range(args.warmup):
            got, want = new().efc_force, old()
        torch.cuda.synchronize()
        diff = float((got - want).abs().max() / want.abs().max().clamp_min(1e-30))
        t_new, t_old = [], []
        for _ in range(args.steps):  # alternating: a drift of the machine hits both
            t_new.append(timed(new))
            t_old.append(timed(old))
        kern = {}
        lib.mjh_debug_phase_timing(1)
        for k in (args.sweeps, 0):
            kern[k] = []
            for _ in range(args.steps):
                assert (new(k).niter == k).all()
                ms, kid = (ctypes.c_float * 16)(), (ctypes.c_int * 16)()
                n = lib.mjh_debug_phase_times(ms, kid, 16)
                assert n == 1 and kid[0] == KERNEL_ID, [(kid[i], ms[i]) for i in range(n)]
                kern[k].append(ms[0])
        lib.mjh_debug_phase_timing(0)
        k_s, k0_s = 1e-3 * float(np.median(kern[args.sweeps])), 1e-3 * float(np.median(kern[0]))
        call_s, comp_s = 1e-3 * float(np.median(t_new)), 1e-3 * float(np.median(t_old))
        res.append(dict(model=xml, dtype=str(dtype).split(".")[-1], B=B, nv=nv, nefc=nefc, sweeps=args.sweeps, call_us=1e6 * call_s, call_min_us=1e3 * float(min(t_new)),
                        composition_us=1e6 * comp_s, composition_min_us=1e3 * float(min(t_old)), ratio=comp_s / call_s,
                        env_sweeps_per_s=B * args.sweeps / call_s, composition_env_sweeps_per_s=B * args.sweeps / comp_s,
                        kernel_us=1e6 * k_s, kernel_no_sweep_us=1e6 * k0_s, sweep_us=1e6 * (k_s - k0_s) / args.sweeps,
                        kernel_env_sweeps_per_s=B * args.sweeps / max(k_s - k0_s, 1e-12), force_difference=diff, plan=list(mt.pgs.plan(nv, nefc, dtype))))
    print(json.dumps(dict(tool="pgs_throughput", device=torch.cuda.get_device_name(), sweeps=args.sweeps, steps=args.steps, warmup=args.warmup, results=res)))


if __name__ == "__main__":
    main()
