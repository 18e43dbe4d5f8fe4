"""Kernel time of ``jac_subtree_com``, ``jac_dot`` and ``angmom_mat``, matrix and product form, the bytes they move per second, and what the torch composition a user
can write today costs on the same leaves.

For each (model, dtype, B): a few steps and a forward pass give the leaves.  Each call is timed through the library's per-launch events (mjh_debug_phase_timing),
the kernel by its id (MJH_KERNEL_JACOBIAN_POINT + op = 36 + op for a matrix, 40 + op for a product with ``vec``), and end to end with HIP events around the call.
The bytes are the library's own account per environment and query (mjh_model_kernel_io).  Queries: the whole model (body 0) for the two subtree functions, the last
body's ``xipos`` on that body for ``jac_dot``.  Beside each product form: its matrix form followed by ``einsum``.  The torch composition of the subtree functions is
one ``jac`` per body at its ``xipos``, stacked, then ``einsum`` with the masses (and, for the angular momentum, with ``ximat`` / ``body_inertia`` and cross products);
``jac_dot`` has none: nothing else exposes the derivative.  Prints one JSON line.

    python tools/jacobian_throughput.py [--steps 30] [--warmup 5]
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
MATRIX, PRODUCT = 36, 40  # MJH_KERNEL_JACOBIAN_POINT, MJH_KERNEL_JACOBIAN_POINT_VEC
DOT, SUBTREE_COM, ANGMOM = 1, 2, 3
CONFIGS = [("humanoid", torch.float64, 4096), ("ant", torch.float32, 16384)]


def torch_subtree(m, f, want_angmom):
    """jac_subtree_com / angmom_mat of body 0 composed from one jac per body and torch ops: [B, nv, 3]."""
    nb = int(m.nbody)
    J = [mt.jac(m, f, f.xipos[:, b], b) for b in range(nb)]
    jp, jr = torch.stack([j[0] for j in J], 1), torch.stack([j[1] for j in J], 1)  # [B, nb, nv, 3]
    sc = torch.einsum("n,bnik->bik", m.body_mass, jp) / m.body_subtreemass[0]
    if not want_angmom:
        return sc
    R = f.ximat.reshape(f.ximat.shape[0], nb, 3, 3)
    rot = torch.einsum("bnrc,nc,bnsc,bnis->bnir", R, m.body_inertia, R, jr)
    d = (f.xipos - f.subtree_com[:, :1])[:, :, None, :].expand_as(jp)
    return (rot + m.body_mass[None, :, None, None] * torch.linalg.cross(d, jp - sc[:, None], dim=-1)).sum(1)


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
        last = int(mx.nbody) - 1
        pt, v = f.xipos[:, last].contiguous(), f.qvel
        handle = _handle(mdev, torch.device("cuda", torch.cuda.current_device()), dtype).handle
        tol = 1e-9 if dtype == torch.float64 else 1e-3

        def wall(fn):
            for _ in range(args.warmup):
                fn()
            torch.cuda.synchronize()
            out = []
            for _ in range(args.steps):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                fn()
                t1.record()
                t1.synchronize()
                out.append(t0.elapsed_time(t1))
            return float(np.median(out)), float(min(out))

        def kernel(fn, kid_want):
            lib.mjh_debug_phase_timing(1)
            per_call = []
            for _ in range(args.steps):
                fn()
                ms, kid = (ctypes.c_float * 96)(), (ctypes.c_int * 96)()
                n = lib.mjh_debug_phase_times(ms, kid, 96)
                per_call.append([(kid[i], ms[i]) for i in range(n)])
            lib.mjh_debug_phase_timing(0)
            assert all(len(c) == 1 and c[0][0] == kid_want for c in per_call), (per_call[0], kid_want)
            io = (ctypes.c_int64 * 2)()
            rc = lib.mjh_model_kernel_io(handle, kid_want, io)
            assert rc == 0, rc
            k_ms = float(np.median([c[0][1] for c in per_call]))
            nbytes = B * (io[0] + io[1])
            return dict(kernel_us=1e3 * k_ms, kernel_min_us=1e3 * float(min(c[0][1] for c in per_call)), read_bytes_per_env=int(io[0]),
                        written_bytes_per_env=int(io[1]), bytes_per_s=nbytes / (k_ms * 1e-3), hbm_bound_us=nbytes / HBM_BYTES_PER_S * 1e6)

        ops = {"jac_subtree_com": (SUBTREE_COM, lambda **k: mt.jac_subtree_com(mdev, f, 0, **k), lambda: torch_subtree(mdev, f, False)),
               "angmom_mat": (ANGMOM, lambda **k: mt.angmom_mat(mdev, f, 0, **k), lambda: torch_subtree(mdev, f, True)),
               "jac_dot": (DOT, lambda **k: mt.jac_dot(mdev, f, pt, last, **k)[0], None)}
        for name, (op, ours, theirs) in ops.items():
            mat, prod = ours(), ours(vec=v)
            via = torch.einsum("bik,bi->bk", mat, v)
            scale = max(via.abs().max().item(), 1e-30)
            assert (prod - via).abs().max().item() <= tol * scale, (name, (prod - via).abs().max().item(), scale)
            row = dict(model=xml, dtype=str(dtype).split(".")[-1], B=B, function=name)
            row["matrix"] = dict(kernel(ours, MATRIX + op), call_us=1e3 * wall(ours)[0])
            row["product"] = dict(kernel(lambda: ours(vec=v), PRODUCT + op), call_us=1e3 * wall(lambda: ours(vec=v))[0])
            row["matrix_then_einsum_us"] = 1e3 * wall(lambda: torch.einsum("bik,bi->bk", ours(), v))[0]
            if theirs is not None:
                ref = theirs()
                assert (ref - mat).abs().max().item() <= tol * max(mat.abs().max().item(), 1e-30), (name, (ref - mat).abs().max().item())
                row["torch_composition_us"] = 1e3 * wall(theirs)[0]
            res.append(row)
    print(json.dumps(dict(tool="jacobian_throughput", device=torch.cuda.get_device_name(), steps=args.steps, warmup=args.warmup, results=res)))


if __name__ == "__main__":
    main()
