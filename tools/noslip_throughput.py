"""Kernel time of ``solve_noslip`` next to the bytes it moves, and ``solve_pgs`` at the same sweep count for context.

Two workloads: the humanoid at B = 4096 in float64 (pyramidal cones: 16 pairs a sweep) and the ant with elliptic cones at B = 16384 in float32 (60 contact slots, a
QCQP of two rows each where the normal force is positive), on the leaves of this library's own ``forward``.  The humanoid starts from the benchmark's input recipe
(small random velocities and controls).  The ant has no floor and at that recipe's pose only contacts between geoms that cannot move against each other, whose
QCQPs are refused at the first pivot; its joints are therefore thrown far past their ranges (``qpos`` +- 2.5 rad, joint velocities from 5e-5 to 5 rad/s over the
batch: the recipe of tests/test_noslip.py) so that legs meet and the Cholesky / Newton path runs: ``qcqp_contacts_per_env`` counts the contacts with a positive
normal force and a block that moves.  ``tolerance = 0``, from the pass's own force, at 1 and 10 sweeps (``--sweeps``).  The call is timed by HIP events around it on the
current stream, ``--steps`` times after ``--warmup`` warm-up calls, every variant inside one loop so that a drift of the machine hits all of them; the kernel alone
through the library's per-launch events (mjh_debug_phase_timing, kernel id 55; ``solve_pgs``: 54).  Medians and minima are reported.  ``bytes_per_env`` is the
library's own account (``mjh_model_kernel_io``), ``hbm_bound_us`` the time those bytes take at 8 TB/s.  ``solve_pgs`` runs on the humanoid alone (it refuses
elliptic cones) from zeros.  No ratio is asserted: the figures are the record.  Prints one JSON line.

    python tools/noslip_throughput.py [--sweeps 1 10] [--steps 20] [--warmup 3]
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
from mujoco_torch_amd import noslip  # noqa: E402

WORKLOADS = (("humanoid", {}, torch.float64, 4096), ("ant", {"cone": 1}, torch.float32, 16384))
KERNEL_NOSLIP, KERNEL_PGS = 55, 54
HBM_BYTES_PER_S = 8e12


def timed(call):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    call()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def kernel_ms(lib, call, kernel_id):
    call()
    ms, kid = (ctypes.c_float * 16)(), (ctypes.c_int * 16)()
    n = lib.mjh_debug_phase_times(ms, kid, 16)
    assert n == 1 and kid[0] == kernel_id, [(kid[i], ms[i]) for i in range(n)]
    return ms[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweeps", type=int, nargs="+", default=[1, 10])
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
        d = mt.make_data(mc).expand(B).clone()
        d = d.replace(qvel=torch.tensor(0.01 * rng.randn(B, mc.nv)), ctrl=torch.tensor(0.3 * rng.randn(B, mc.nu)))
        if xml == "ant":
            s = 10.0 ** np.linspace(-5, 0, B)
            d = d.replace(qpos=d.qpos + torch.tensor(2.5 * rng.uniform(-1, 1, (B, mc.nq))), qvel=torch.tensor(5.0 * s[:, None] * rng.randn(B, mc.nv)))
        d = mt.forward(mx, (d.to(dtype) if dtype != torch.float64 else d).to("cuda"))
        ne, nf, _, ncon, nefc = (int(x) for x in mc.constraint_sizes_py)
        nv = int(mc.nv)
        nm = native.get_native_model(mx, torch.device("cuda", 0), dtype)
        rw = (ctypes.c_int64 * 2)()
        assert lib.mjh_model_kernel_io(nm.handle, KERNEL_NOSLIP, rw) == 0
        nbytes = (rw[0] + rw[1]) * B
        calls = {("noslip", k): (lambda k=k: mt.solve_noslip(mx, d, iterations=k, tolerance=0.0)) for k in args.sweeps}
        if not ov:
            calls.update({("pgs", k): (lambda k=k: mt.solve_pgs(mx, d, iterations=k, tolerance=0.0)) for k in args.sweeps})
        for _ in range(args.warmup):
            for c in calls.values():
                c()
        torch.cuda.synchronize()
        t_call = {key: [] for key in calls}
        for _ in range(args.steps):  # every variant inside one loop: a drift of the machine hits all of them
            for key, c in calls.items():
                t_call[key].append(timed(c))
        t_kern = {key: [] for key in calls}
        lib.mjh_debug_phase_timing(1)
        for _ in range(args.steps):
            for key, c in calls.items():
                t_kern[key].append(kernel_ms(lib, c, KERNEL_NOSLIP if key[0] == "noslip" else KERNEL_PGS))
        lib.mjh_debug_phase_timing(0)
        moved = mt.solve_noslip(mx, d, iterations=max(args.sweeps), tolerance=0.0)
        dims, adr = np.asarray(mc.tables.con_dim)[:ncon], np.asarray(mc.tables.con_efc_address)[:ncon]
        changed = (moved.efc_force != d.efc_force)
        live = sum(int(changed[:, a + 1:a + k].any(-1).sum()) for k, a in zip(dims, adr) if k > 1) if ov else 0
        rows = []
        for (what, k), ts in t_call.items():
            ks = t_kern[(what, k)]
            rows.append(dict(function="solve_" + what, sweeps=k, call_us=1e3 * float(np.median(ts)), call_min_us=1e3 * float(min(ts)),
                             kernel_us=1e3 * float(np.median(ks)), kernel_min_us=1e3 * float(min(ks))))
        res.append(dict(model=xml, overrides=ov, dtype=str(dtype).split(".")[-1], B=B, nv=nv, nefc=nefc, ncon=ncon, bytes_per_env=int(rw[0] + rw[1]),
                        read_bytes_per_env=int(rw[0]), written_bytes_per_env=int(rw[1]), hbm_bound_us=nbytes / HBM_BYTES_PER_S * 1e6,
                        plan=list(noslip.plan(nv, nefc, ncon, dtype)), rows_changed=int(changed.sum()), qcqp_contacts_per_env=live / B,
                        mean_niter=float(moved.niter.float().mean()), timings=rows))
    print(json.dumps(dict(tool="noslip_throughput", device=torch.cuda.get_device_name(), steps=args.steps, warmup=args.warmup, results=res)))


if __name__ == "__main__":
    main()
