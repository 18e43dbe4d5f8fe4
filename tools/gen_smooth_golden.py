"""Generate tests/golden/smooth/<case>.npz from the REFERENCE's own ``kinematics`` / ``com_pos`` / ``crb`` / ``tendon_armature`` / ``factor_m`` / ``com_vel`` / ``rne``
(mujoco_torch/_src/smooth.py), in the build container, and tests/golden/smooth/reference_api.json (the seven names with their parameter lists).

TEST INFRASTRUCTURE, container-only (needs the reference tree; see oracle/ref_harness.py, which this script imports unchanged, as it does
oracle/gen_golden.make_inputs and tools/gen_inverse_golden.put).  For each case and environment: the seeded inputs of ``make_inputs(recipe)``, then
  pass/<env>/<leaf>             the leaves one reference ``forward`` produced on those inputs (tests/_smooth_ref.PASS_LEAVES), unedited,
  kin/<env>/<leaf>              the inputs of ``kinematics`` (qpos, mocap_pos, mocap_quat) and out/<env>/kinematics/<leaf> what the reference's ``kinematics`` made of them
                                on the pass's Data (its subtree_com is what trackcom / targetbodycom cameras read),
  in/<env>/<function>/<leaf>    for the six other functions, the leaves the function reads, EDITED: each perturbed by a relative 0.1 U(-1, 1), element by element
                                (RandomState(9000 + 16 env + the function's index)); for ``factor_m``, ``qM + G G^T`` with
                                ``G = 0.1 sqrt(mean diag qM) randn(nv, nv) / sqrt(nv)`` -- so that no output can be had by recomputing from qpos,
  out/<env>/<function>/<leaf>   the reference's outputs on those edited leaves (``rne_acc``: ``rne`` with ``flg_acc=True``).
A case with ``zero_mass`` sets ``body_mass`` of that (leaf) body to 0 through the reference Model's ``replace``: the mjMINVAL branch of ``com_pos``.
The meta records, per function and leaf, the reference's own distance from the longdouble evaluation of the same inputs (tests/_smooth_ref.py), per environment,
measured as tests/_util.rel_err measures: ``ref_distance[function][leaf][env]``.  Every one must lie within ``TOL_PRE[dtype]`` (tests/_cases.py), which is the bound the
GPU tests hold the kernels to: the script asserts it; a case that misses is replaced by another model, not by a wider bound.
Only recorded arrays and settings are stored.

Run:  python tools/gen_smooth_golden.py [case ...]
"""

import inspect
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
from gen_golden import make_inputs  # noqa: E402
from gen_integrator_golden import _keep_integer_tables, load_lite  # noqa: E402
from gen_inverse_golden import put  # noqa: E402

import _smooth_ref as sr  # noqa: E402
import mujoco_torch_amd as mt  # noqa: E402
from _cases import TOL_PRE  # noqa: E402
from _util import rel_err  # noqa: E402

GOLD = os.path.join(REPO, "tests", "golden", "smooth")

# case: (xml, dtype, environments, make_inputs recipe, zero-mass body or None)
CASES = {
    "pendula_f64": ("pendula", "float64", 3, "pendula", None),            # every joint type, mocap, tendons
    "pendula_f32": ("pendula", "float32", 3, "pendula", None),
    "ant_f64": ("ant", "float64", 3, "bench_ctrl", None),                  # nv 14: the clamped-pivot factorisation
    "humanoid_f64": ("humanoid", "float64", 3, "perturbed", None),        # nv 27: + 1e-10 I
    "humanoid_f32": ("humanoid", "float32", 3, "perturbed", None),
    "tendon_armature_f64": ("tendon_armature", "float64", 3, "generic", None),
    "centipede_f64": ("centipede", "float64", 2, "centipede", None),      # 74 bodies, 72 dofs: more bodies than lanes
    "ant_zero_mass_f64": ("ant", "float64", 2, "bench_ctrl", -1),          # body_mass of the last (a leaf) body = 0 through replace
}
SIX = ("com_pos", "crb", "tendon_armature", "factor_m", "com_vel", "rne")
KIN_IN = ("qpos", "mocap_pos", "mocap_quat")


def _edited(fn, L, env, nv):
    rng = np.random.RandomState(9000 + 16 * env + SIX.index(fn))
    out = {}
    for n in sr.READS[fn]:
        a = np.array(L[n])
        if fn == "factor_m":
            G = 0.1 * np.sqrt(np.mean(np.diag(a.astype(np.float64)))) * rng.randn(nv, nv) / np.sqrt(max(nv, 1))
            out[n] = (a.astype(np.float64) + G @ G.T).astype(a.dtype)
        else:
            out[n] = (a.astype(np.float64) * (1 + 0.1 * rng.uniform(-1, 1, a.shape))).astype(a.dtype)
    return out


def main(only=None, out_dir=GOLD):
    ref = ref_harness.load()
    _keep_integer_tables()
    os.makedirs(out_dir, exist_ok=True)
    fns = {n: getattr(ref.smooth, n) for n in sr.FUNCTIONS}
    for case, (xml, dtype_s, nenv, recipe, zero_mass) in CASES.items():
        if only and case not in only:
            continue
        torch.manual_seed(0)
        dtype = getattr(torch, dtype_s)
        lite = load_lite(xml, {})
        mref, keep_sensors = put(ref, lite, dtype)
        mx = mt.device_put(load_lite(xml, {}), dtype=None if dtype == torch.float64 else dtype)
        edit = None
        if zero_mass is not None:
            body = int(zero_mass) % int(lite.nbody)
            mass = mref.body_mass.clone()
            mass[body] = 0
            mref = mref.replace(body_mass=mass)
            mass2 = mx.body_mass.clone()
            mass2[body] = 0
            mx = mx.replace(body_mass=mass2)
            edit = dict(body=body, value=0.0)
        V = sr.model_values(mx)
        assert not ref.support.is_sparse(mref), "the functions are recorded on the dense path"
        store = {}
        dist = {f: {n: [] for n in sr.WRITES["rne" if f == "rne_acc" else f]} for f in SIX + ("rne_acc",)}
        for env in range(nenv):
            inp = make_inputs(recipe, lite, env)
            d = ref.io.make_data(mref)
            d = d.replace(**{k: torch.tensor(np.asarray(v, dtype=np.float64)) for k, v in inp.items()})
            if dtype != torch.float64:
                d = d.to(dtype)
            for n in KIN_IN:
                store[f"kin/{env}/{n}"] = getattr(d, n).detach().numpy().copy()
            f = ref.forward.forward(mref, d.clone())
            k = fns["kinematics"](mref, f.clone().replace(**{n: getattr(d, n).clone() for n in KIN_IN}))  # (the caller's subtree_com -- trackcom cameras read it -- is the pass's)
            for n in sr.WRITES["kinematics"]:
                store[f"out/{env}/kinematics/{n}"] = getattr(k, n).detach().numpy().copy()
            P = {n: sr.shaped(V, n, getattr(f, n).detach().numpy().copy()) for n in sr.PASS_LEAVES}
            for n, a in P.items():
                store[f"pass/{env}/{n}"] = a
            for fn in SIX:
                if fn == "tendon_armature" and V["nt"] == 0:
                    continue
                E = _edited(fn, P, env, V["nv"])
                for n, a in E.items():
                    store[f"in/{env}/{fn}/{n}"] = a
                de = f.clone().replace(**{n: torch.from_numpy(a.copy()).reshape(getattr(f, n).shape) for n, a in E.items()})
                for tag, kw in ((fn, {}),) + ((("rne_acc", dict(flg_acc=True)),) if fn == "rne" else ()):
                    o = fns[fn](mref, de.clone(), **kw)
                    want = sr.FN[fn](V, E, **kw)
                    for n in sr.WRITES[fn]:
                        a = sr.shaped(V, n, getattr(o, n).detach().numpy().copy())
                        store[f"out/{env}/{tag}/{n}"] = a
                        e = rel_err(a, np.asarray(want[n], dtype=np.float64).astype(a.dtype))
                        dist[tag][n].append(e)
                        assert e <= TOL_PRE[dtype], f"{case} env {env} {tag}.{n}: the reference is {e:.3g} from the longdouble evaluation, TOL_PRE is {TOL_PRE[dtype]}"
        meta = dict(xml=xml, overrides={}, dtype=dtype_s, nenv=nenv, recipe=recipe, keep_sensors=keep_sensors, zero_mass=edit, ref_distance=dist,
                    sizes=dict(nbody=V["nb"], nv=V["nv"], njnt=V["nj"], ntendon=V["nt"]), torch=torch.__version__)
        store["meta"] = np.array(json.dumps(meta))
        path = os.path.join(out_dir, case + ".npz")
        np.savez_compressed(path, **store)
        print(f"{case}: {os.path.getsize(path) / 1024:.0f} KB; the reference's distance from longdouble (rel_err): " +
              ", ".join(f"{t} {max((max(v, default=0) for v in dist[t].values()), default=0):.1e}" for t in dist))
    if not only:
        with open(os.path.join(out_dir, "reference_api.json"), "w") as fh:
            json.dump(dict(signatures={n: list(inspect.signature(f).parameters) for n, f in fns.items()}), fh, indent=1, sort_keys=True)
            fh.write("\n")


if __name__ == "__main__":
    main(sys.argv[1:] or None)
