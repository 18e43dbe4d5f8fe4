"""Generate tests/golden/vjp/<case>.npz: the REFERENCE's own ``torch.autograd`` gradient of a seeded linear functional of the next state through
its float64 CPU ``step`` -- what tests/test_vjp.py holds ``differentiable_step`` to.

TEST INFRASTRUCTURE, container-only (needs the reference tree; imports oracle/ref_harness.py and tools/gen_inverse_golden.put unchanged).  For
every environment of ``tests/_cases.seeded_batch(xml, {}, float64, NENV)``:  L = <w_qpos, qpos'> + <w_qvel, qvel'> + <w_act, act'> with the weights
of RandomState(900) (standard normal), and dL / d(qpos, qvel, act, ctrl) by ``torch.autograd.grad``.  Inputs, weights and gradients are recorded.

Only models whose step the reference can differentiate are listed: cartpole (no constraint rows).  gravcomp_arm has 68 constraint rows in the seeded
state and the reference's passive forces call numpy on a tensor that requires grad there, so it is left out.

Run:  python tools/gen_vjp_golden.py
"""

import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for p in (os.path.join(REPO, "oracle"), os.path.join(REPO, "mujoco-torch_amd"), os.path.join(REPO, "tests"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import ref_harness  # noqa: E402
from _cases import seeded_batch  # noqa: E402
from gen_inverse_golden import load_lite, put  # noqa: E402

GOLD = os.path.join(REPO, "tests", "golden", "vjp")
NENV = 4
CASES = ("cartpole",)
STATE = ("qpos", "qvel", "act")
INPUTS = ("qpos", "qvel", "act", "ctrl")


def main():
    ref = ref_harness.load()
    os.makedirs(GOLD, exist_ok=True)
    for xml in CASES:
        mref, _ = put(ref, load_lite(xml, {}), torch.float64)
        mx, d = seeded_batch(xml, {}, torch.float64, NENV)
        rng = np.random.RandomState(900)
        w = {k: rng.randn(NENV, getattr(d, k).shape[-1]) for k in STATE}
        store = {f"w/{k}": v for k, v in w.items()}
        grads = {k: [] for k in INPUTS}
        for e in range(NENV):
            leaves = {k: getattr(d, k)[e].clone().requires_grad_() for k in INPUTS}
            out = ref.forward.step(mref, ref.io.make_data(mref).replace(**leaves))
            L = sum((torch.tensor(w[k][e]) * getattr(out, k)).sum() for k in STATE)
            g = torch.autograd.grad(L, [leaves[k] for k in INPUTS], allow_unused=True)
            for k, gk in zip(INPUTS, g):
                grads[k].append(np.zeros(leaves[k].shape) if gk is None else gk.numpy())
        for k in INPUTS:
            store[f"in/{k}"] = getattr(d, k).numpy()
            store[f"grad/{k}"] = np.stack(grads[k])
        store["meta"] = np.array(json.dumps(dict(xml=xml, nenv=NENV, dtype="float64", weights="RandomState(900).randn per state leaf, in the order qpos, qvel, act",
                                                 functional="sum_k <w_k, k'> over the next qpos, qvel, act", torch=torch.__version__)))
        path = os.path.join(GOLD, xml + ".npz")
        np.savez_compressed(path, **store)
        print(f"{xml}: {os.path.getsize(path)} bytes;", {k: float(np.abs(store['grad/' + k]).max()) for k in INPUTS if store['grad/' + k].size})


if __name__ == "__main__":
    main()
