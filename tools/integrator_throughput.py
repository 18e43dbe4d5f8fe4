"""Kernel time of one ``implicit`` launch against the same computation written with torch ops, and what the implicit integrator costs per step:
``implicit(mx, forward(mx, d))`` against ``step(mx, d)`` on the model's own Euler path.

For each (model, dtype, B): a few steps and a forward pass give the leaves; ``implicit`` is timed through the library's per-launch events
(mjh_debug_phase_timing), the kernel by its id (MJH_KERNEL_INTEGRATE = 35), and -- like the torch expression -- end to end with HIP events around the call.  The
bytes are the library's own account per environment (mjh_model_kernel_io).  The torch expression is what a user can write today: qDeriv by two einsums and a
diagonal, ``torch.linalg.cholesky`` / ``cholesky_solve`` of ``qM - h qDeriv`` (+ 1e-10 I above 16 dofs), the velocity update, the slide / hinge positions by a
gather and the quaternions of free / ball joints one joint at a time (models with activations are not timed this way).  Prints one JSON line.

    python tools/integrator_throughput.py [--steps 30] [--warmup 5]
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
INTEGRATE = 35
CONFIGS = [("humanoid", torch.float64, 4096), ("ant", torch.float32, 16384)]


def _quat_integrate(q, w, h):
    n = w.norm(dim=-1, keepdim=True)
    axis = w / torch.where(n > 0, n, torch.ones_like(n))
    half = 0.5 * h * n
    r = torch.cat([torch.cos(half), axis * torch.sin(half)], dim=-1)
    a, b = q, r
    out = torch.stack([a[:, 0] * b[:, 0] - a[:, 1] * b[:, 1] - a[:, 2] * b[:, 2] - a[:, 3] * b[:, 3], a[:, 0] * b[:, 1] + a[:, 1] * b[:, 0] + a[:, 2] * b[:, 3] - a[:, 3] * b[:, 2],
                       a[:, 0] * b[:, 2] - a[:, 1] * b[:, 3] + a[:, 2] * b[:, 0] + a[:, 3] * b[:, 1], a[:, 0] * b[:, 3] + a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1] + a[:, 3] * b[:, 0]], dim=-1)
    return out / out.norm(dim=-1, keepdim=True)


def torch_implicit(m, f, h, tab):
    """(qpos, qvel, time) of the implicit step with torch ops on the leaves of the pass (stateless actuators)."""
    vel = tab["bias_vel"] + tab["gain_vel"] * f.ctrl
    Q = torch.einsum("bur,bu,buc->brc", f.actuator_moment, vel, f.actuator_moment) - torch.diag(m.dof_damping)
    A = f.qM - h * Q
    if A.shape[-1] > 16:
        A = A + 1e-10 * torch.eye(A.shape[-1], dtype=A.dtype, device=A.device)
    qacc = torch.cholesky_solve((f.qfrc_smooth + f.qfrc_constraint).unsqueeze(-1), torch.linalg.cholesky(A)).squeeze(-1)
    qvel = f.qvel + h * qacc
    qpos = f.qpos.clone()
    qpos[:, tab["hs_q"]] = f.qpos[:, tab["hs_q"]] + h * qvel[:, tab["hs_v"]]
    for kind, qa, da in tab["quats"]:
        if kind == 0:
            qpos[:, qa:qa + 3] = f.qpos[:, qa:qa + 3] + h * qvel[:, da:da + 3]
            qa, da = qa + 3, da + 3
        qpos[:, qa:qa + 4] = _quat_integrate(f.qpos[:, qa:qa + 4], qvel[:, da:da + 3], h)
    return qpos, qvel, f.time + h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    lib = native.load_library()
    res = []
    for xml, dtype, B in CONFIGS:
        mx = mt.device_put(mt.mjcf.from_xml_path(mt.test_data_path(xml + ".xml")), dtype=None if dtype == torch.float64 else dtype)
        assert int(mx.na) == 0 and int(mx.ntendon) == 0 and int(mx.opt.integrator) == 0, "the torch expression covers stateless actuators, no tendons; step must be Euler"
        mdev = mx.to("cuda")
        rng = np.random.RandomState(0)
        d = mt.make_data(mx).expand(B).clone()
        d = d.replace(qvel=torch.tensor(0.05 * rng.randn(B, mx.nv)), ctrl=torch.tensor(0.3 * rng.randn(B, mx.nu)))
        d = (d.to(dtype) if dtype != torch.float64 else d).to("cuda")
        for _ in range(3):
            d = mt.step(mdev, d)
        f = mt.forward(mdev, d)
        jt, qadr, dadr = np.asarray(mx.jnt_type.data), np.asarray(mx.jnt_qposadr), np.asarray(mx.jnt_dofadr)
        affine = lambda t: torch.tensor(np.asarray(t.data) == 1, device="cuda")
        tab = dict(bias_vel=mdev.actuator_biasprm[:, 2] * affine(mx.actuator_biastype), gain_vel=mdev.actuator_gainprm[:, 2] * affine(mx.actuator_gaintype),
                   hs_q=torch.tensor(qadr[jt >= 2], device="cuda"), hs_v=torch.tensor(dadr[jt >= 2], device="cuda"),
                   quats=[(int(t), int(q), int(v)) for t, q, v in zip(jt, qadr, dadr) if t < 2])
        h = float(mx.opt.timestep)
        ours, theirs = (lambda: mt.implicit(mdev, f)), (lambda: torch_implicit(mdev, f, h, tab))
        a, b = ours(), theirs()
        for got, want in ((a.qpos, b[0]), (a.qvel, b[1]), (a.time, b[2])):
            scale = want.abs().max().item()
            assert (got - want).abs().max().item() <= (1e-9 if dtype == torch.float64 else 2e-4) * scale, ((got - want).abs().max().item(), scale)
        stepped, tail = (lambda: mt.step(mdev, d)), (lambda: mt.implicit(mdev, mt.forward(mdev, d)))
        for _ in range(args.warmup):
            ours(), theirs(), stepped(), tail()
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

        wall_ours, wall_theirs, wall_step, wall_tail = wall(ours), wall(theirs), wall(stepped), wall(tail)
        lib.mjh_debug_phase_timing(1)
        per_call = []
        for _ in range(args.steps):
            ours()
            ms, kid = (ctypes.c_float * 96)(), (ctypes.c_int * 96)()
            n = lib.mjh_debug_phase_times(ms, kid, 96)
            per_call.append([(kid[i], ms[i]) for i in range(n)])
        lib.mjh_debug_phase_timing(0)
        assert all(len(c) == 1 and c[0][0] == INTEGRATE for c in per_call), per_call[0]
        k_ms = float(np.median([c[0][1] for c in per_call]))
        io = (ctypes.c_int64 * 2)()
        rc = lib.mjh_model_kernel_io(_handle(mdev, torch.device("cuda", torch.cuda.current_device()), dtype).handle, INTEGRATE, io)
        assert rc == 0, rc
        nbytes = B * (io[0] + io[1])
        res.append(dict(model=xml, dtype=str(dtype).split(".")[-1], B=B, kernel_us=1e3 * k_ms, kernel_min_us=1e3 * float(min(c[0][1] for c in per_call)),
                        call_us=1e3 * wall_ours[0], call_min_us=1e3 * wall_ours[1], torch_ops_us=1e3 * wall_theirs[0], torch_ops_min_us=1e3 * wall_theirs[1],
                        step_euler_us=1e3 * wall_step[0], forward_plus_implicit_us=1e3 * wall_tail[0],
                        read_bytes_per_env=int(io[0]), written_bytes_per_env=int(io[1]), bytes_per_s=nbytes / (k_ms * 1e-3),
                        hbm_bound_us=nbytes / HBM_BYTES_PER_S * 1e6, hbm_share=nbytes / (k_ms * 1e-3) / HBM_BYTES_PER_S))
    print(json.dumps(dict(tool="integrator_throughput", device=torch.cuda.get_device_name(), steps=args.steps, warmup=args.warmup, results=res)))


if __name__ == "__main__":
    main()
