"""Kernel times of the support functions (``jac``, ``apply_ft``, ``xfrc_accumulate``, ``mul_m``, ``solve_m``) next to the torch formulation of
each and the HBM bound.

For each (model, dtype, B): one forward pass poses the batch, with a random ``xfrc_applied``; P = 6 query points and K = 3 vectors per environment.
Each op's kernel is timed through the library's per-launch events (mjh_debug_phase_timing, ids 23..27); the whole call (Python included) and the
torch formulation are timed with HIP events: an ``einsum`` Jacobian from ``cdof`` / ``subtree_com`` and a mask table (jac), the einsum of that
Jacobian with force / torque (apply_ft), the same over every body (xfrc_accumulate), ``torch.bmm`` with ``qM`` (mul_m) and ``torch.cholesky_solve``
with ``qLD`` (solve_m).  The bytes are what each kernel must move: its leaves once and its outputs.  Prints one JSON line.

    python tools/support_throughput.py [--steps 20] [--warmup 5]
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

HBM_BYTES_PER_S = 8e12
CONFIGS = [("humanoid", torch.float64, 4096), ("ant", torch.float32, 16384), ("mesh_contact", torch.float32, 8192)]
P, K = 6, 3


def timed(fn, steps):
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
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
        d = mt.forward(mdev, (d.to(dtype) if dtype != torch.float64 else d).to("cuda"))
        d = d.replace(xfrc_applied=torch.randn(B, mx.nbody, 6, dtype=dtype, device="cuda"))
        nv, nb = mx.nv, mx.nbody
        ids = [int(b) for b in np.linspace(0, nb - 1, P).round()]
        pts = torch.randn(B, P, 3, dtype=dtype, device="cuda")
        f, t = torch.randn(B, P, 3, dtype=dtype, device="cuda"), torch.randn(B, P, 3, dtype=dtype, device="cuda")
        v = torch.randn(B, K, nv, dtype=dtype, device="cuda")
        # the torch formulation: mask[b, dof] = dof's body is an ancestor-or-self of b
        parent, dofbody = np.asarray(mx.body_parentid), np.asarray(mx.dof_bodyid)
        anc = np.eye(nb, dtype=bool)
        for b in range(1, nb):
            anc[b] |= anc[parent[b]]
        mask = torch.tensor(anc[:, dofbody], dtype=dtype, device="cuda")  # [nbody, nv]
        root = torch.tensor(np.asarray(mx.body_rootid), device="cuda")
        idt = torch.tensor(ids, device="cuda")

        def t_jac(pts, idt):
            off = pts - d.subtree_com[:, root[idt]]                                    # [B, P, 3]
            cd = d.cdof
            cr = torch.linalg.cross(cd[:, None, :, :3].expand(B, len(idt), nv, 3), off[:, :, None, :].expand(B, len(idt), nv, 3), dim=-1)
            m = mask[idt][None, :, :, None]
            return (cd[:, None, :, 3:] + cr) * m, cd[:, None, :, :3] * m

        def t_apply(f, t, pts, idt):
            jp, jr = t_jac(pts, idt)
            return torch.einsum("bpvk,bpk->bpv", jp, f) + torch.einsum("bpvk,bpk->bpv", jr, t)

        all_b = torch.arange(nb, device="cuda")
        ops = {
            "jac": (lambda: mt.jac(mdev, d, pts, ids), lambda: t_jac(pts, idt), B * (6 * nv + 6 * P * nv * 2)),
            "apply_ft": (lambda: mt.apply_ft(mdev, d, f, t, pts, ids), lambda: t_apply(f, t, pts, idt), B * (6 * nv + 9 * P + P * nv)),
            "xfrc_accumulate": (lambda: mt.xfrc_accumulate(mdev, d), lambda: t_apply(d.xfrc_applied[..., :3], d.xfrc_applied[..., 3:], d.xipos, all_b).sum(1),
                                B * (6 * nv + 12 * nb + nv)),
            "mul_m": (lambda: mt.mul_m(mdev, d, v), lambda: torch.bmm(v, d.qM.transpose(1, 2)), B * (nv * nv + 2 * K * nv)),
            "solve_m": (lambda: mt.solve_m(mdev, d, v), lambda: torch.cholesky_solve(v.transpose(1, 2), d.qLD).transpose(1, 2), B * (nv * nv + 2 * K * nv)),
        }
        rb = torch.empty((), dtype=dtype).element_size()
        for k, (ours, theirs, nreal) in ops.items():
            for _ in range(args.warmup):
                ours(), theirs()
            torch.cuda.synchronize()
            call_ms, torch_ms = timed(ours, args.steps), timed(theirs, args.steps)
            lib.mjh_debug_phase_timing(1)
            kern = []
            for _ in range(args.steps):
                ours()
                ms, kid = (ctypes.c_float * 96)(), (ctypes.c_int * 96)()
                n = lib.mjh_debug_phase_times(ms, kid, 96)
                kern += [ms[i] for i in range(n) if 23 <= kid[i] <= 27]
            lib.mjh_debug_phase_timing(0)
            k_ms = float(np.median(kern))
            nbytes = nreal * rb
            res.append(dict(model=xml, dtype=str(dtype).split(".")[-1], B=B, nv=nv, op=k, P=P, K=K, kernel_ms=k_ms, call_ms=call_ms, torch_ms=torch_ms,
                            bytes=nbytes, hbm_bound_ms=nbytes / HBM_BYTES_PER_S * 1e3, roofline_share=nbytes / (k_ms * 1e-3) / HBM_BYTES_PER_S))
    print(json.dumps(dict(tool="support_throughput", device=torch.cuda.get_device_name(), steps=args.steps, warmup=args.warmup, results=res)))


if __name__ == "__main__":
    main()
