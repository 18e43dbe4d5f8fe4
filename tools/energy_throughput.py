"""Kernel time of one ``energy`` launch, the bytes it moves per second, and what the same two numbers cost when written with torch ops on the same leaves.

For each (model, dtype, B): a few steps and a forward pass give the leaves; ``energy`` is timed through the library's per-launch events
(mjh_debug_phase_timing), the kernel by its id (MJH_KERNEL_ENERGY = 34), and -- like the torch expression -- end to end with HIP events around the call.  The
bytes are the library's own account per environment (mjh_model_kernel_io).  The torch expression is what a user can write today: ``0.5 * einsum('bi,bij,bj')``
for the kinetic energy plus the gathers and sums of the potential (gravity over the bodies, the slide / hinge springs; models with ball / free or tendon springs
are not timed this way).  Prints one JSON line.

    python tools/energy_throughput.py [--steps 30] [--warmup 5]
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
ENERGY = 34
CONFIGS = [("humanoid", torch.float64, 4096), ("ant", torch.float32, 16384)]


def torch_energy(m, f, hinge_slide, qadr):
    """[potential, kinetic] with torch ops on the leaves of the pass (gravity and slide / hinge springs; the kinetic energy as one einsum)."""
    V = -(m.body_mass[1:] * (f.xipos[:, 1:] * m.opt.gravity).sum(-1)).sum(-1)
    d = f.qpos[:, qadr] - m.qpos_spring[qadr]
    V = V + (0.5 * m.jnt_stiffness[hinge_slide] * d * d).sum(-1)
    T = 0.5 * torch.einsum("bi,bij,bj->b", f.qvel, f.qM, f.qvel)
    return torch.stack([V, T], dim=-1)


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
        d = d.replace(qvel=torch.tensor(0.05 * rng.randn(B, mx.nv)))
        d = (d.to(dtype) if dtype != torch.float64 else d).to("cuda")
        for _ in range(3):
            d = mt.step(mdev, d)
        f = mt.forward(mdev, d)
        jt = np.asarray(mx.jnt_type.data)
        assert not np.asarray(mx.jnt_stiffness)[jt < 2].any() and not int(mx.ntendon), "the torch expression covers slide / hinge springs only"
        hs = torch.tensor(np.nonzero(jt >= 2)[0], device="cuda")
        qadr = torch.tensor(np.asarray(mx.jnt_qposadr)[jt >= 2], device="cuda")
        ours, theirs = (lambda: mt.energy(mdev, f)), (lambda: torch_energy(mdev, f, hs, qadr))
        a, b = ours(), theirs()
        scale = b.abs().max().item()
        assert (a - b).abs().max().item() <= (1e-10 if dtype == torch.float64 else 1e-3) * scale, ((a - b).abs().max().item(), scale)
        for _ in range(args.warmup):
            ours(), theirs()
        torch.cuda.synchronize()

        def wall(fn):
            out = []
            for _ in range(args.steps):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                fn()
                t1.record()
                t1.synchronize()
                out.append(t0.elapsed_time(t1))
            return float(np.median(out)), float(min(out))

        wall_ours, wall_theirs = wall(ours), wall(theirs)
        lib.mjh_debug_phase_timing(1)
        per_call = []
        for _ in range(args.steps):
            ours()
            ms, kid = (ctypes.c_float * 96)(), (ctypes.c_int * 96)()
            n = lib.mjh_debug_phase_times(ms, kid, 96)
            per_call.append([(kid[i], ms[i]) for i in range(n)])
        lib.mjh_debug_phase_timing(0)
        assert all(len(c) == 1 and c[0][0] == ENERGY for c in per_call), per_call[0]
        k_ms = float(np.median([c[0][1] for c in per_call]))
        io = (ctypes.c_int64 * 2)()
        rc = lib.mjh_model_kernel_io(_handle(mdev, torch.device("cuda", torch.cuda.current_device()), dtype).handle, ENERGY, io)
        assert rc == 0, rc
        nbytes = B * (io[0] + io[1])
        res.append(dict(model=xml, dtype=str(dtype).split(".")[-1], B=B, kernel_us=1e3 * k_ms, kernel_min_us=1e3 * float(min(c[0][1] for c in per_call)),
                        call_us=1e3 * wall_ours[0], call_min_us=1e3 * wall_ours[1], torch_ops_us=1e3 * wall_theirs[0], torch_ops_min_us=1e3 * wall_theirs[1],
                        read_bytes_per_env=int(io[0]), written_bytes_per_env=int(io[1]), bytes_per_s=nbytes / (k_ms * 1e-3),
                        hbm_bound_us=nbytes / HBM_BYTES_PER_S * 1e6, hbm_share=nbytes / (k_ms * 1e-3) / HBM_BYTES_PER_S))
    print(json.dumps(dict(tool="energy_throughput", device=torch.cuda.get_device_name(), steps=args.steps, warmup=args.warmup, results=res)))


if __name__ == "__main__":
    main()
