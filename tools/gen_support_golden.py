"""Generate tests/golden/support/<case>.npz from the REFERENCE's own support functions (mujoco_torch/_src/support.py, smooth.py), in the build
container, and tests/golden/support/reference_api.json (the reference's signatures and enums).

TEST INFRASTRUCTURE, container-only (needs the reference tree; see oracle/ref_harness.py, which this script imports unchanged, as it does
oracle/gen_golden.make_inputs and tools/gen_inverse_golden.put).  For each case and environment:
  1. the seeded inputs of ``make_inputs(recipe)`` and one reference ``forward`` in the case's dtype; the leaves the functions read
     (cdof, subtree_com, xipos, qM, qLD) are recorded, with a random ``xfrc_applied`` on every body (RandomState(700 + env));
  2. queries: NPT points (near the bodies' xipos) on bodies that include the world body 0, the first root body and a leaf body (and a
     body without dofs when the model has one), a force and a torque per point, and K vectors -- recorded in the case's dtype;
  3. outputs: the reference ``support.jac`` / ``apply_ft`` per point, ``support.xfrc_accumulate``, ``smooth.mul_m`` / ``smooth.solve_m`` per
     vector, all on the recorded leaves.
The GPU tests feed the recorded leaves in, so the comparison does not depend on forward parity.

Run:  python tools/gen_support_golden.py [case ...]
"""

import inspect
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for p in (os.path.join(REPO, "oracle"), os.path.join(REPO, "mujoco-torch_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import ref_harness  # noqa: E402
from gen_golden import make_inputs  # noqa: E402
from gen_inverse_golden import load_lite, put  # noqa: E402

GOLD = os.path.join(REPO, "tests", "golden", "support")
NPT, K = 6, 3

# case: (xml, dtype, environments, make_inputs recipe)
CASES = {
    "humanoid_f64": ("humanoid", "float64", 3, "perturbed"),      # nv 27: the cholesky_solve branch; free root
    "humanoid_f32": ("humanoid", "float32", 3, "perturbed"),
    "ant_f64": ("ant", "float64", 3, "bench_ctrl"),               # nv 8: the inline substitution
    "ant_f32": ("ant", "float32", 3, "bench_ctrl"),
    "cartpole_f64": ("cartpole", "float64", 3, "cartpole"),       # nv 2
    "mocap_child_f64": ("mocap_child", "float64", 3, "mocap"),    # bodies without dofs
    "centipede_83_f64": ("centipede_83", "float64", 2, "centipede"),  # nv > 64: two mask words
}


def pick_bodies(lite, rng):
    nb = int(lite.nbody)
    parent = np.asarray(lite.body_parentid)
    leaves = [b for b in range(1, nb) if b not in set(parent[1:].tolist())]
    roots = [b for b in range(1, nb) if parent[b] == 0]
    nodof = [b for b in range(1, nb) if int(np.asarray(lite.body_dofnum)[b]) == 0]
    ids = [0, roots[0], leaves[-1]] + nodof[:1]
    while len(ids) < NPT:
        ids.append(int(rng.randint(nb)))
    return ids


def main(only=None, out_dir=GOLD):
    ref = ref_harness.load()
    os.makedirs(out_dir, exist_ok=True)
    for case, (xml, dtype_s, nenv, recipe) in CASES.items():
        if only and case not in only:
            continue
        dtype = getattr(torch, dtype_s)
        lite = load_lite(xml, {})
        mref, _ = put(ref, lite, dtype)
        nb, nv = int(lite.nbody), int(lite.nv)
        store = {}
        bodies = pick_bodies(lite, np.random.RandomState(7))
        for env in range(nenv):
            inp = make_inputs(recipe, lite, env)
            d = ref.io.make_data(mref)
            d = d.replace(**{k: torch.tensor(np.asarray(v, dtype=np.float64)) for k, v in inp.items()})
            if dtype != torch.float64:
                d = d.to(dtype)
            d = ref.forward.forward(mref, d)
            rng = np.random.RandomState(700 + env)
            xfrc = torch.tensor(rng.randn(nb, 6)).to(dtype)
            d = d.replace(xfrc_applied=xfrc)
            xipos = d.xipos.detach()
            pts = torch.stack([xipos[b] + torch.tensor(0.1 * rng.randn(3)).to(dtype) for b in bodies])
            frc = torch.tensor(rng.randn(NPT, 3)).to(dtype)
            trq = torch.tensor(rng.randn(NPT, 3)).to(dtype)
            vec = torch.tensor(rng.randn(K, nv)).to(dtype)
            jp, jr, ft = [], [], []
            for i, b in enumerate(bodies):
                p, r = ref.support.jac(mref, d, pts[i], torch.tensor(b))
                jp.append(p.detach()); jr.append(r.detach())
                ft.append(ref.support.apply_ft(mref, d, frc[i], trq[i], pts[i], torch.tensor(b)).detach())
            for k in ("cdof", "subtree_com", "xipos", "xfrc_applied", "qM", "qLD"):
                store[f"{env}/{k}"] = getattr(d, k).detach().numpy()
            store[f"{env}/point"], store[f"{env}/force"], store[f"{env}/torque"], store[f"{env}/vec"] = pts.numpy(), frc.numpy(), trq.numpy(), vec.numpy()
            store[f"{env}/jacp"], store[f"{env}/jacr"] = torch.stack(jp).numpy(), torch.stack(jr).numpy()
            store[f"{env}/apply_ft"] = torch.stack(ft).numpy()
            store[f"{env}/xfrc_accumulate"] = ref.support.xfrc_accumulate(mref, d).detach().numpy()
            store[f"{env}/mul_m"] = torch.stack([ref.smooth.mul_m(mref, d, vec[j]) for j in range(K)]).detach().numpy()
            store[f"{env}/solve_m"] = torch.stack([ref.smooth.solve_m(mref, d, vec[j]) for j in range(K)]).detach().numpy()
        meta = dict(xml=xml, dtype=dtype_s, nenv=nenv, recipe=recipe, nv=nv, nbody=nb, body_id=bodies, npt=NPT, K=K,
                    queries="RandomState(700 + env): xfrc_applied randn (nbody, 6); points xipos[body] + 0.1 randn; force, torque, vectors randn",
                    torch=torch.__version__)
        store["meta"] = np.array(json.dumps(meta))
        path = os.path.join(out_dir, case + ".npz")
        np.savez_compressed(path, **store)
        print(f"{case}: {os.path.getsize(path) / 1024:.0f} KB, nv {nv}, bodies {bodies}")
    api(ref, out_dir)


def api(ref, out_dir):
    """The reference's parameter names of the six functions and the members / values of four enums."""
    fns = {"jac": ref.support.jac, "apply_ft": ref.support.apply_ft, "xfrc_accumulate": ref.support.xfrc_accumulate,
           "full_m": ref.support.full_m, "mul_m": ref.smooth.mul_m, "solve_m": ref.smooth.solve_m}
    out = dict(signatures={k: list(inspect.signature(f).parameters) for k, f in fns.items()},
               enums={n: {e.name: int(e.value) for e in getattr(ref.types, n)} for n in ("SensorType", "ObjType", "ConstraintType", "WrapType")})
    with open(os.path.join(out_dir, "reference_api.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("reference_api.json:", {k: len(v) for k, v in out["enums"].items()})


if __name__ == "__main__":
    main(sys.argv[1:] or None)
