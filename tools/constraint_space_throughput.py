"""Calls per second of the constraint-space functions (mul_jac_vec, mul_jac_t_vec, constraint_update, efc_ar) and what they cost against the compositions a
user could write before them from torch and the kernels that existed: ``torch.bmm`` for the products, ``bmm`` + ``where`` + ``mul_m`` for the update,
``torch.bmm(J, solve_m(J)^T) + diag R`` for ``AR``.

Two workloads: the humanoid at B = 4096 in float64 and the ant with frictionloss rows at B = 16384 in float32, on the leaves of this library's own ``forward``
on the benchmark's input recipe (small random velocities and controls).  Every call and every composition is timed the same way: HIP events around the call on
the current stream, ``--steps`` times after ``--warmup`` warm-up calls, alternating the new call and its composition inside one loop so that a drift of the
machine hits both; the median and the minimum are reported.  The new kernels are also timed alone through the library's per-launch events
(mjh_debug_phase_timing, kernel ids 50 .. 53), with the bytes ``mjh_model_kernel_io`` accounts per environment, as bytes per second.  ``ratio`` is the
composition's median time over the new call's: below 1 the composition is faster, and it is printed as it comes out.  Prints one JSON line.

    python tools/constraint_space_throughput.py [--steps 50] [--warmup 10]
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

WORKLOADS = (("humanoid", torch.float64, 4096), ("ant_frictionloss", torch.float32, 16384))
KERNEL_IDS = dict(mul_jac_vec=50, mul_jac_t_vec=51, constraint_update=52, efc_ar=53)
MINVAL = 1e-15


def timed(call):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    call()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def compositions(mx, d, B):
    """{function: the same result from torch and the kernels that existed before} on the Data's leaves."""
    ne, nf, _, _, nefc = mx.constraint_sizes_py
    nv = int(mx.nv)
    J, D, aref, fl = d.efc_J.reshape(B, nefc, nv), d.efc_D, d.efc_aref, d.efc_frictionloss
    floss = nf > 0 and not (int(mx.opt.disableflags) & mt.DisableBit.FRICTIONLOSS)
    always = torch.arange(nefc, device=J.device) < ne + nf
    scale = float(mx.stat.meaninertia) * max(1, nv)

    def update():
        q = d.qacc
        jar = torch.bmm(J, q.unsqueeze(-1)).squeeze(-1) - aref
        r = 1 / (D + (D == 0) * MINVAL)
        neg = (fl > 0) & (jar <= -r * fl) if floss else torch.zeros_like(jar, dtype=torch.bool)
        pos = (fl > 0) & (jar >= r * fl) if floss else neg
        quad = (always | (jar < 0)) & ~neg & ~pos
        force = torch.where(quad, -D * jar, torch.where(neg, fl, torch.where(pos, -fl, torch.zeros_like(fl))))
        state = quad.int() + 2 * neg.int() + 3 * pos.int()
        qc = torch.bmm(force.unsqueeze(1), J).squeeze(1)
        ms = mt.mul_m(mx, d, q) - d.qfrc_smooth
        gauss = 0.5 * (ms * (q - d.qacc_smooth)).sum(-1)
        cost = 0.5 * (quad * D * jar * jar).sum(-1) + (neg * (-0.5 * r * fl * fl - fl * jar)).sum(-1) + (pos * (-0.5 * r * fl * fl + fl * jar)).sum(-1) + gauss
        grad = ms - qc
        return jar, force, state, qc, cost, gauss, grad, grad.norm(dim=-1) / scale

    def ar():
        return (torch.bmm(J, mt.solve_m(mx, d, J).transpose(-1, -2)) + torch.diag_embed(torch.where(D > 0, 1 / D, torch.zeros_like(D))),
                torch.bmm(J, d.qacc_smooth.unsqueeze(-1)).squeeze(-1) - aref)

    return dict(mul_jac_vec=lambda: torch.bmm(J, d.qacc.unsqueeze(-1)).squeeze(-1), mul_jac_t_vec=lambda: torch.bmm(d.efc_force.unsqueeze(1), J).squeeze(1),
                constraint_update=update, efc_ar=ar)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
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
        new = dict(mul_jac_vec=lambda: mt.mul_jac_vec(mx, d, d.qacc), mul_jac_t_vec=lambda: mt.mul_jac_t_vec(mx, d, d.efc_force),
                   constraint_update=lambda: mt.constraint_update(mx, d), efc_ar=lambda: mt.efc_ar(mx, d))
        old = compositions(mx, d, B)
        h = _handle(mx, torch.device("cuda", torch.cuda.current_device()), dtype).handle
        for name, call in new.items():
            for _ in range(args.warmup):
                call()
                old[name]()
            torch.cuda.synchronize()
            t_new, t_old = [], []
            for _ in range(args.steps):  # alternating: a drift of the machine hits both
                t_new.append(timed(call))
                t_old.append(timed(old[name]))
            lib.mjh_debug_phase_timing(1)
            kern = []
            for _ in range(args.steps):
                call()
                ms, kid = (ctypes.c_float * 16)(), (ctypes.c_int * 16)()
                n = lib.mjh_debug_phase_times(ms, kid, 16)
                assert n == 1 and kid[0] == KERNEL_IDS[name], [(kid[i], ms[i]) for i in range(n)]
                kern.append(ms[0])
            lib.mjh_debug_phase_timing(0)
            io = (ctypes.c_int64 * 2)()
            assert lib.mjh_model_kernel_io(h, KERNEL_IDS[name], io) == 0
            k_s = 1e-3 * float(np.median(kern))
            res.append(dict(function=name, model=xml, dtype=str(dtype).split(".")[-1], B=B, nv=nv, nefc=nefc, call_us=1e3 * float(np.median(t_new)),
                            call_min_us=1e3 * float(min(t_new)), composition_us=1e3 * float(np.median(t_old)), composition_min_us=1e3 * float(min(t_old)),
                            ratio=float(np.median(t_old) / np.median(t_new)), kernel_us=1e6 * k_s, kernel_min_us=1e3 * float(min(kern)),
                            environments_per_s=B / k_s, read_bytes_per_env=int(io[0]), written_bytes_per_env=int(io[1]),
                            kernel_bytes_per_s=B * (io[0] + io[1]) / k_s))
    print(json.dumps(dict(tool="constraint_space_throughput", device=torch.cuda.get_device_name(), steps=args.steps, warmup=args.warmup, results=res)))


if __name__ == "__main__":
    main()
