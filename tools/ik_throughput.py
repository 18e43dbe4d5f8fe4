"""``ik_site`` solves per second and ``mjh_qpos_arith`` items per second at B = 4096, and where an ``ik_site`` call spends its time.

The model is the tests' arm (tests/golden/ik_arm.xml); every environment starts at a seeded configuration and is sent to the tip position of another one and to a seeded
orientation, all dofs, the defaults (``max_steps = 20``), both dtypes.  A solve is one environment of one call; the call is timed ``--repeats`` times by HIP events
on a synchronised device after a warm-up, and the figure is the median with the spread (max - min) / median.
A call makes 21 kinematics passes and 21 launches of the IK kernel (id MJH_KERNEL_IK_SITE = 49).  The split is by the library's per-launch events
(mjh_debug_phase_timing) over one call: the kernels of the passes, the IK launches (the first updates every environment, the last ones find most of them done),
and what is left of the call's wall time, which is the host's (Python between the launches).

``mjh_qpos_arith``: one ``integrate_pos`` call at B = 4096 (40960 (environment, joint) items), the call by events and the kernel alone by the library's events
(id MJH_KERNEL_QPOS_ARITH = 48): at this size the kernel is launch-bound, so the kernel time is the floor of one call.  Prints one JSON line.

    python tools/ik_throughput.py [--repeats 10] [--warmup 3]
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

QPOS_ARITH, IK_SITE = 48, 49
B = 4096
TIP = 0


def timed(call, repeats, warmup):
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        call()
        t1.record()
        t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    med = float(np.median(ms))
    return med, (max(ms) - min(ms)) / med


def _events(lib, cap=64):
    """[(kernel id, ms)] of the launches of the most recent library call (the library waits for it)."""
    ms, kid = (ctypes.c_float * cap)(), (ctypes.c_int * cap)()
    n = lib.mjh_debug_phase_times(ms, kid, cap)
    return [(kid[i], ms[i]) for i in range(n)]


def launches(lib, call):
    """[(kernel id, ms)] of the launches of the last library call that ``call`` makes."""
    lib.mjh_debug_phase_timing(1)
    try:
        call()
        return _events(lib)
    finally:
        lib.mjh_debug_phase_timing(0)


def kernel_split(lib, solve):
    """(ms of the kinematics kernels, ms of the IK kernel) per iteration of one ``ik_site`` call, from the library's per-launch events: the events of a library
    call are read right after it, so ``ik_site``'s call into ``mjh_ik_site_step`` is wrapped -- what is pending before it is the kinematics pass."""
    import mujoco_torch_amd.ik as ikmod

    kin, ik, orig = [], [], ikmod.call

    def wrapped(*a, **k):
        kin.append(sum(ms for _, ms in _events(lib)))
        orig(*a, **k)
        ev = _events(lib)
        assert ev and all(kid == IK_SITE for kid, _ in ev), ev
        ik.append(sum(ms for _, ms in ev))

    ikmod.call = wrapped
    lib.mjh_debug_phase_timing(1)
    try:
        solve()
    finally:
        ikmod.call = orig
        lib.mjh_debug_phase_timing(0)
    return kin, ik


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    lib = native.load_library()
    res = []
    for dtype in (torch.float64, torch.float32):
        mx = mt.device_put(mt.mjcf.from_xml_path(os.path.join(ROOT, "tests", "golden", "ik_arm.xml")), dtype=None if dtype == torch.float64 else dtype)
        mdev = mx.to("cuda")
        nv, njnt = int(mx.nv), int(mx.njnt)
        rng = np.random.RandomState(0)
        d = mt.make_data(mx).expand(B).clone()
        d = (d.to(dtype) if dtype != torch.float64 else d).to("cuda")
        zero = d.qpos.contiguous()
        start = mt.integrate_pos(mdev, zero, torch.tensor(0.3 * rng.uniform(-1, 1, (B, nv))).to(dtype).to("cuda"), 1.0)
        goal = mt.integrate_pos(mdev, zero, torch.tensor(0.3 * rng.uniform(-1, 1, (B, nv))).to(dtype).to("cuda"), 1.0)
        p = mt.forward(mdev, d.replace(qpos=goal), stages=1)
        tp = p.site_xpos[:, TIP].contiguous()
        rv = rng.uniform(-1, 1, (B, 3)) * 0.5 / np.sqrt(3)  # the target orientation: a seeded rotation vector of at most 0.5 rad (the ball-joint wrist reaches any)
        ang = np.linalg.norm(rv, axis=-1, keepdims=True)
        tq = torch.tensor(np.concatenate([np.cos(ang / 2), rv / ang * np.sin(ang / 2)], -1)).to(dtype).to("cuda")
        ds = d.replace(qpos=start)
        solve = lambda: mt.ik_site(mdev, ds, TIP, tp, tq)
        r = solve()
        call_ms, spread = timed(solve, args.repeats, args.warmup)
        row = dict(dtype=str(dtype).split(".")[-1], B=B, max_steps=20, success=float(r.success.double().mean().item()), mean_steps=float(r.steps.double().mean().item()),
                   call_ms=call_ms, call_spread=spread, solves_per_s=B / (1e-3 * call_ms))
        # the split of one call: the kernels of its 21 kinematics passes, its 21 IK launches, and the rest -- the host between the launches
        kin, ik = kernel_split(lib, solve)
        assert len(kin) == len(ik) == 21
        row.update(passes=21, kinematics_kernels_ms=float(sum(kin)), kinematics_pass_first_us=1e3 * float(kin[0]), ik_kernels_ms=float(sum(ik)),
                   ik_kernel_first_us=1e3 * float(ik[0]), ik_kernel_last_us=1e3 * float(ik[-1]), kinematics_share=float(sum(kin)) / call_ms,
                   ik_kernel_share=float(sum(ik)) / call_ms, host_share=1 - float(sum(kin) + sum(ik)) / call_ms)
        # mjh_qpos_arith
        v = torch.tensor(rng.randn(B, nv)).to(dtype).to("cuda")
        arith = lambda: mt.integrate_pos(mdev, start, v, 0.002)
        a_ms, a_spread = timed(arith, 10 * args.repeats, args.warmup)
        ks = []
        for _ in range(10 * args.repeats):
            ev = launches(lib, arith)
            assert len(ev) == 1 and ev[0][0] == QPOS_ARITH, ev
            ks.append(ev[0][1])
        k_ms = float(np.median(ks))
        row.update(qpos_arith_items=B * njnt, qpos_arith_call_us=1e3 * a_ms, qpos_arith_call_spread=a_spread, qpos_arith_kernel_us=1e3 * k_ms,
                   qpos_arith_kernel_spread=(max(ks) - min(ks)) / k_ms, qpos_arith_items_per_s=B * njnt / (1e-3 * k_ms))
        res.append(row)
    print(json.dumps(dict(tool="ik_throughput", device=torch.cuda.get_device_name(), repeats=args.repeats, warmup=args.warmup, results=res)))


if __name__ == "__main__":
    main()
