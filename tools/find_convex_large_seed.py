"""The rule by which oracle/gen_golden.py's CONVEX_LARGE_SEED was chosen: the FIRST seed of 0, 1, 2, ... for which

1. on the CPU oracle's narrow phase, every pair of tests/golden/convex_large.xml is in contact (dist < includemargin) in at least two and apart in
   at least one of the recorded environments, in float64 (five environments) and float32 (six);
2. neither recording is larger than the largest golden that was there before (centipede_83_f64.npz);
3. hinted with the reference's recorded contacts, the float64 oracle keeps its natural narrow-phase outcome on every pair of every recorded
   environment-step (`tie_pairs` == 0: no index selection of the poses is decided by rounding noise).

Criterion 1 needs the oracle only; 2 and 3 need the reference (container-only, oracle/ref_harness.py): a seed that passes 1 is recorded into a scratch
directory and examined.  Prints one line per examined seed -- sizes, float64 tie pairs per environment-step, the float32 environment-steps with a
tie outcome -- and stops at the first seed that passes all three.

    python tools/find_convex_large_seed.py [first seed] [last seed]
"""
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("mujoco-torch_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import gen_golden  # noqa: E402
import pyoracle  # noqa: E402
import _util  # noqa: E402
import mujoco_torch_amd as mt  # noqa: E402
from _convex_large import PAIRS, pair_slots  # noqa: E402
from test_convex_large_host import teacher_forced, tie_outcomes  # noqa: E402

NENV = {"float64": 5, "float32": 6}
SIZE_CAP = os.path.getsize(os.path.join(ROOT, "tests", "golden", "centipede_83_f64.npz"))


def pairs_in_and_out(seed, dtype):
    """Criterion 1 for one dtype."""
    gen_golden.CONVEX_LARGE_SEED = seed
    mx = _util.load_model("convex_large", {}, dtype)
    lite = mt.mjcf.from_xml_path(_util.model_path("convex_large"))
    ds = []
    for e in range(NENV[str(dtype)[6:]]):
        inp = gen_golden.make_inputs("convex_large", lite, e)
        d = mt.make_data(mx).replace(**{k: torch.tensor(np.asarray(v, dtype=np.float64)) for k, v in inp.items()})
        ds.append(d if dtype == torch.float64 else d.to(dtype))
    out = pyoracle.run(mx, torch.stack(ds), step=False, stages=0x07)
    for pair in PAIRS:
        sl = pair_slots(out, pair)
        gap = (out["contact_dist"][:, sl] - out["contact_includemargin"][:, sl]).min(1)
        if not ((gap < 0).sum() >= 2 and (gap > 0).sum() >= 1):
            return False
    return True


def examine(seed, scratch):
    """Records both cases with the reference into `scratch`; returns (sizes, float64 tie pairs per env-step, float32 env-steps with a tie outcome)."""
    gen_golden.CONVEX_LARGE_SEED = seed
    gen_golden.GOLD = _util.GOLD = scratch
    gen_golden.main(["convex_large_f64", "convex_large_f32"])
    sizes = [os.path.getsize(os.path.join(scratch, f"convex_large_{t}.npz")) for t in ("f64", "f32")]
    g = _util.Golden("convex_large_f64")
    ties64 = [tie_outcomes(g, e, s, d)[1] for e, s, d in teacher_forced(g)]
    g = _util.Golden("convex_large_f32")
    flagged32 = [(e, s) for e, s, d in teacher_forced(g) if tie_outcomes(g, e, s, d)[1]]
    return sizes, ties64, flagged32


def main(first=0, last=200):
    real_gold = _util.GOLD
    with tempfile.TemporaryDirectory() as scratch:
        os.symlink(os.path.join(real_gold, "meshes"), os.path.join(scratch, "meshes"))
        os.symlink(os.path.join(real_gold, "convex_large.xml"), os.path.join(scratch, "convex_large.xml"))
        for seed in range(first, last + 1):
            _util.GOLD = real_gold
            if not (pairs_in_and_out(seed, torch.float64) and pairs_in_and_out(seed, torch.float32)):
                continue
            sizes, ties64, flagged32 = examine(seed, scratch)
            ok = max(sizes) <= SIZE_CAP and sum(ties64) == 0
            print(f"seed {seed}: sizes {sizes} (cap {SIZE_CAP}), float64 tie pairs {ties64}, float32 tie env-steps {flagged32} -> {'KEEP' if ok else 'next'}", flush=True)
            if ok:
                return seed
    return None


if __name__ == "__main__":
    a = [int(x) for x in sys.argv[1:3]]
    main(*a)
