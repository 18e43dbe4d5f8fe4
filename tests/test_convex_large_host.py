"""The convex narrow phase on hulls larger than one wavefront, CPU part (tests/test_convex_large.py is the GPU part).

convex_large.xml carries hulls with more than 64 vertices, faces and edges (blob100), 18 vertices per face (prism18) and caps past the 20-vertex face limit
(prism44), in eleven pairs that cover every convex pair function.  Here: the hull tables keep those sizes; the reference's recordings
(tests/golden/convex_large_{f64,f32}.npz, oracle/gen_golden.py) really put every pair in and out of contact; the CPU oracle -- which the GPU tests lean on for
ties -- reproduces them without a single narrow-phase tie outcome in float64; and two properties of the contacts that need neither (tests/_convex_large.py)
hold on the recordings and on the oracle.  The oracle against every recorded leaf, and convex.py's tables against the reference's mesh.get, are
tests/test_oracle_golden.py's: both take the new recordings from the directory listing.

The refusal of a hull too large for the pair kernel's LDS scratch is decided by the device library at model creation; the CPU stand-in (tests/_hostsim.py)
never reaches it, so that test is in the GPU file.
"""
import numpy as np
import pytest
import torch

import pyoracle
from _cases import TOL_PRE
from _convex_large import PAIRS, TABLE_SIZES, PropertyTally, check_properties, pair_slots
from _util import GOLDEN_CASES, HINT_LEAVES, INT_LEAVES, PRE_SOLVER, REAL_LEAVES, Golden, rel_err  # noqa: I001

CASES = ["convex_large_f64", "convex_large_f32"]
# environment-steps of the float32 recording on which the oracle, given the recorded contacts as its hint, keeps a narrow-phase tie outcome other than its natural
# one (`tie_pairs` > 0) -- counted here on the CPU; tests/test_convex_large.py admits the oracle route for the float32 GPU comparison on no more than this share
F32_TIE_FLAGGED = [(2, 1), (5, 1)]  # (environment, step)
F32_TIE_ENV_STEPS = len(F32_TIE_FLAGGED)
CONTACT_LEAVES = ["contact_dist", "contact_pos", "contact_frame"]


def recorded(g, e, s):
    return {n: g.expected(e, s, n) for n in REAL_LEAVES + INT_LEAVES}


def tie_outcomes(g, e, s, d):
    """(oracle outputs hinted with the recorded contacts, number of pairs that kept a non-natural tie outcome) for one recorded environment-step."""
    ties = np.zeros(1, dtype=np.int32)
    out = pyoracle.run(g.model, d, step=False, stages=0x07, contact_hint={n: g.expected(e, s, n) for n in HINT_LEAVES}, tie_pairs=ties)
    return out, int(ties[0])


def teacher_forced(g):
    """(env, step, input Data of that step) over a recording: each step starts from the reference's own previous output."""
    for e in range(g.nenv):
        d = g.input_data(e)
        for s in range(g.nsteps):
            yield e, s, d
            d = pyoracle.apply(d, recorded(g, e, s))


def test_new_recordings_are_in_the_golden_listing():
    assert set(CASES) <= set(GOLDEN_CASES)  # test_oracle_matches_reference_golden, test_convex_tables_match_reference and test_step_matches_reference_golden run on them


def test_hull_tables_are_larger_than_a_wavefront():
    """A change to the hull builder (or to the STL files) cannot quietly shrink the case back under 64: vertices, faces, edges, vertices per face."""
    g = Golden("convex_large_f64")
    T = g.model.tables.convex
    for geom, (nv, nf, ne, nfv) in TABLE_SIZES.items():
        t = T[geom]
        assert (len(t["vert"]), len(t["face"]), len(t["edge"]), t["face"].shape[1]) == (nv, nf, ne, nfv), geom
        assert t["facenormal"].shape == (nf, 3)
    assert all(T[geom] is None for geom in range(len(T)) if geom not in TABLE_SIZES)
    blob, p18, p44 = T[1], T[3], T[4]
    assert min(len(blob["vert"]), len(blob["face"]), len(blob["edge"])) > 64 and len(p44["vert"]) > 64
    assert not np.array_equal(T[1]["vert"], T[2]["vert"])  # the two blobs carry different vertex data (different scales)
    # prism18: two 18-gons and 18 quads padded 4 -> 18 with their last id
    pads = [f for f in p18["face"] if len(set(f.tolist())) == 4]
    assert len(pads) == 18 and all((f[3:] == f[3]).all() for f in pads) and sum(len(set(f.tolist())) == 18 for f in p18["face"]) == 2
    # prism44: the caps are subsampled (44 // 20 + 1 = 3 -> 15 of 44), so the faces' cap rings name 30 of the 88 vertices and every vertex is still on a side face
    caps = [f for f in p44["face"] if len(set(f.tolist())) == 15]
    assert len(caps) == 2 and len(set(np.concatenate(caps).tolist())) == 30 and len(set(p44["face"].reshape(-1).tolist())) == 88


def test_pair_list():
    g = Golden("convex_large_f64")
    out = recorded(g, 0, 0)
    got = sorted(set(zip(out["contact_geom1"].tolist(), out["contact_geom2"].tolist())))
    assert got == sorted(PAIRS)
    fns = sorted(p[0] for p in g.model.tables.pairs)
    assert fns == [5, 5, 6, 6, 7, 7, 8, 8, 8, 8, 8]  # plane / sphere / capsule - convex twice each, convex-convex five times
    assert g.model.constraint_sizes_py[3] == 2 * 4 + 2 * 1 + 2 * 2 + 5 * 4


@pytest.mark.parametrize("case", CASES)
def test_every_pair_is_in_and_out_of_contact(case):
    """On the recording itself (first step, the drawn poses): every pair has dist < includemargin in at least two environments and dist > includemargin in at least one."""
    g = Golden(case)
    for pair in PAIRS:
        sl = pair_slots(recorded(g, 0, 0), pair)
        gap = np.array([(g.expected(e, 0, "contact_dist")[sl] - g.expected(e, 0, "contact_includemargin")[sl]).min() for e in range(g.nenv)])
        assert (gap < 0).sum() >= 2 and (gap > 0).sum() >= 1, (pair, gap)


def test_float64_oracle_meets_no_tie_on_the_recordings(oracle_lib):
    """Contact leaves and every other pre-solver leaf of the natural oracle run against the recording at TOL_PRE, every environment and step; and hinted with the
    recorded contacts, the oracle keeps its natural narrow-phase outcome on every pair: no index selection of these poses is decided by rounding noise.  This is what
    lets the GPU float64 comparison run against the recording with no oracle alternative admitted."""
    g = Golden("convex_large_f64")
    worst = 0.0
    for e, s, d in teacher_forced(g):
        nat = pyoracle.run(g.model, d, step=True)
        for n in PRE_SOLVER:
            err = rel_err(nat[n], g.expected(e, s, n))
            assert err <= TOL_PRE[g.dtype], (e, s, n, err)
            worst = max(worst, err if n in CONTACT_LEAVES else 0.0)
        hinted, ties = tie_outcomes(g, e, s, d)
        assert ties == 0, (e, s, ties)
        assert all(np.array_equal(hinted[n], nat[n]) for n in CONTACT_LEAVES)
    print(f"convex_large_f64: worst contact leaf {worst:.2e} = {worst / TOL_PRE[g.dtype]:.2e} of TOL_PRE")


def test_float32_tie_count_is_the_recorded_one(oracle_lib):
    g = Golden("convex_large_f32")
    flagged, worst = [], 0.0
    for e, s, d in teacher_forced(g):
        hinted, ties = tie_outcomes(g, e, s, d)
        if ties:
            flagged.append((e, s))
        worst = max(worst, max(rel_err(hinted[n], g.expected(e, s, n)) for n in CONTACT_LEAVES))
    print(f"convex_large_f32: tie env-steps {flagged}, worst contact leaf {worst:.2e} = {worst / TOL_PRE[g.dtype]:.2e} of TOL_PRE")
    assert flagged == F32_TIE_FLAGGED, flagged
    assert len(flagged) <= g.nenv * g.nsteps / 4  # more than a quarter would mean the poses are bad: another seed, not a wider cap
    assert worst <= TOL_PRE[g.dtype]


@pytest.mark.parametrize("case", CASES)
def test_contact_properties_on_recording_and_oracle(case, oracle_lib):
    """tests/_convex_large.py's plane-convex and sphere-convex properties (numpy longdouble, no reference and no oracle in the expected values) on the reference's
    recording and on the oracle's output of the same inputs; the poses must exercise them (PropertyTally.assert_covered)."""
    g = Golden(case)
    eps = float(torch.finfo(g.dtype).eps)
    for source in ("recording", "oracle"):
        tally = PropertyTally()
        for e, s, d in teacher_forced(g):
            tally.add(check_properties(recorded(g, e, s) if source == "recording" else pyoracle.run(g.model, d, step=True), g.model, eps))
        print(f"{case} {source}: {tally}")
        tally.assert_covered()
