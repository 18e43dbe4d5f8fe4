"""The primitive narrow phase's yardstick and family without a device: tests/_prim_ref.py against the reference's recordings and against the CPU oracle, and the
conditions of tests/_prim_scenes.py's table.  tests/test_primitive_contacts.py runs the same rules (``_prim_scenes.check_*``) on the HIP kernels.

The restatement is tied to the reference by the recordings: for every golden of tests/golden/ whose model has in-kernel pairs, ``_prim_ref`` on the RECORDED ``geom_xpos`` /
``geom_xmat`` gives the recorded ``contact_dist / pos / frame`` at ``TOL_PRE[dtype]`` on the comparable rows -- without importing the reference.
"""
import numpy as np
import pytest
import torch

import _prim_ref as ref
import _prim_scenes as ps
import pyoracle
from _cases import TOL_PRE
from _util import GOLDEN_CASES, Golden, rel_err

STAGES_COLLISION = 0x07  # kinematics, com_pos / crb prefix, collision


def oracle_run(mx, d, **kw):
    return pyoracle.run(mx, d, step=False, stages=STAGES_COLLISION, **kw)


# ---- the restatement against the reference's recordings -------------------------------------------------------------------------------------------------------------

SEEN = {}


@pytest.mark.parametrize("case", GOLDEN_CASES)
def test_the_restatement_gives_the_recorded_contacts(case):
    g = Golden(case)
    mx = g.model
    T = mx.tables
    pairs = ref.pairs_of(T)
    if not any(p[0] < ref.FN_IN_KERNEL for p in pairs):
        SEEN[case] = 0
        return  # (no sphere / capsule pair in this model: nothing of it is this module's business)
    dtype, eps = g.dtype, float(torch.finfo(g.dtype).eps)
    ncon, nslot = mx.constraint_sizes_py[3], len(T.contact_perm)
    nrows = 0
    for env in range(g.nenv):
        for step in range(g.nsteps):
            ex = lambda n: np.asarray(g.expected(env, step, n))
            C = ref.reference(pairs, T.pair_dst, nslot, ex("geom_xpos")[None], ex("geom_xmat").reshape(1, -1, 9), np.asarray(mx.geom_size, dtype=np.float64))
            rec = ps.contact_leaves({k: ex(k) for k in ("contact_dist", "contact_pos", "contact_frame")}, 1, ncon)
            want, keep = (ps._as_leaves(C), C.comparable(eps)) if T.topk else C.against(rec["pos"], eps)
            live = (C.fn >= 0)[None]
            if T.topk:  # the recorded contacts are the ncon closest candidates: each one of an in-kernel pair against that pair's candidate, and (no other pairs) the multiset
                cand = np.where(live[0], ps.f64(C.dist[0]), np.inf)
                if live.all():
                    assert rel_err(np.sort(rec["dist"][0]), np.sort(cand)[:ncon]) <= TOL_PRE[dtype], (case, env, step)
                g1, g2 = ex("contact_geom1").reshape(-1), ex("contact_geom2").reshape(-1)
                for c in range(ncon):
                    own = [int(T.pair_dst[p][q]) for p, (fn, k, a, b) in enumerate(pairs) if fn < ref.FN_IN_KERNEL and (a, b) == (int(g1[c]), int(g2[c])) for q in range(k)]
                    if not own:
                        continue
                    q = own[int(np.argmin(np.abs(cand[own] - rec["dist"][0, c])))]
                    for leaf in ps.LEAVES:
                        if keep[leaf][0, q]:
                            assert rel_err(rec[leaf][0, c], ps.f64(want[leaf][0, q])) <= TOL_PRE[dtype], (case, env, step, c, leaf)
                    nrows += 1
                continue
            for leaf in ps.LEAVES:
                rows = keep[leaf] & live
                err = rel_err(rec[leaf][rows], ps.f64(want[leaf][rows]))
                assert err <= TOL_PRE[dtype], (case, env, step, leaf, err)
            nrows += int(live.sum())
    SEEN[case] = nrows
    print(f"{case}: {nrows} recorded contacts of in-kernel pairs compared")


def test_the_recordings_cover_the_bundled_primitive_models():
    """The ant, humanoid, hopper, capsules_topk and centipede recordings were all compared, each on some contacts."""
    for case in GOLDEN_CASES:
        if case not in SEEN:
            test_the_restatement_gives_the_recorded_contacts(case)
    for model in ("ant", "humanoid", "hopper", "capsules_topk", "centipede"):
        hits = {c: n for c, n in SEEN.items() if c.startswith(model) and n > 0}
        assert hits, model


# ---- the family -----------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [e.name for e in ps.TABLE])
def test_the_table_meets_its_conditions(name, oracle_lib):
    """Each entry's condition, proved from ``mx.tables`` and the reference's margins on the oracle's geom frames (float64)."""
    mx, d = ps.placed(name)
    out = oracle_run(mx, d)
    ps.conditions(name, (out["geom_xpos"], out["geom_xmat"]))
    e = ps.BY_NAME[name]
    assert e.B % 4 != 0
    print(f"{name}: B = {e.B}, {len(mx.tables.pairs)} pairs, {ps.slots(mx)} slots, nefc {mx.constraint_sizes_py[4]}: {e.why}")


def test_the_exact_entries_take_every_clamp_and_both_picks(oracle_lib):
    """Over the exact and either-side entries: sphere-capsule's t below, inside and above its range; each of capsule-capsule's four parameters below and above its range
    (the eight clamp outcomes); d1 < d2 true and false; make_frame's b = y and b = z; plane-capsule's fallback with both of its n[1] outcomes; coincident centres."""
    seen = {k: set() for k in ref.SIDES}
    for e in ps.TABLE:
        if e.kind not in ("exact", "side"):
            continue
        mx, d = ps.placed(e.name)
        out = oracle_run(mx, d)
        C = ps.reference_of(mx, out["geom_xpos"], out["geom_xmat"])
        for k in ("t_side",):
            seen[k] |= set(np.unique(C.side[k][:, C.fn == ref.FN_SPHERE_CAPSULE]).tolist())
        for k in ("ota_side", "otb_side", "in1_side", "in2_side", "pick"):
            seen[k] |= set(np.unique(C.side[k][:, C.fn == ref.FN_CAPSULE_CAPSULE]).tolist())
        seen["frame_y"] |= set(np.unique(C.side["frame_y"][:, C.fn != ref.FN_PLANE_CAPSULE]).tolist())
        fb = C.side["pc_fallback"].astype(bool)
        seen["pc_fallback"] |= set(np.unique(C.side["pc_fallback"][:, C.fn == ref.FN_PLANE_CAPSULE]).tolist())
        seen["pc_fb_y"] |= set(np.unique(C.side["pc_fb_y"][fb]).tolist())
        seen["coincident"] |= set(np.unique(C.side["coincident"]).tolist())
    print(seen)
    for k in ("t_side", "ota_side", "otb_side", "in1_side", "in2_side"):
        assert seen[k] == {-1, 0, 1}, (k, seen[k])
    for k in ("pick", "frame_y", "pc_fallback", "pc_fb_y", "coincident"):
        assert seen[k] == {0, 1}, (k, seen[k])


@pytest.mark.parametrize("name,dtype", ps.CASES, ids=ps.CASE_IDS)
def test_the_oracle_against_the_restatement(name, dtype, oracle_lib):
    """``pyoracle.run(..., step=False, stages=0x07)`` on the whole family by the rules of the GPU test: values, properties, constants, max_contact_points."""
    mx, d = ps.placed(name, dtype)
    out = oracle_run(mx, d)
    e = ps.BY_NAME[name]
    print(f"{name} {dtype}: {e.why}")
    if mx.tables.topk:
        twin, dt = ps.placed(name, dtype, uncapped=True)
        tout = oracle_run(twin, dt)
        C, _, _ = ps.check_values(name, dtype, twin, tout)
        ps.check_properties(dtype, ps.contact_leaves(tout, e.B, ps.slots(twin)), C)
        ps.check_topk(name, dtype, mx, out, twin, tout)
        return
    C, _, _ = ps.check_values(name, dtype, mx, out)
    ps.check_properties(dtype, ps.contact_leaves(out, e.B, ps.slots(mx)), C)
    ps.check_constants(dtype, mx, out, e.B)


def test_the_known_answer_scenes_through_the_restatement(oracle_lib):
    """The primitive pair among the seven scenes of tests/test_collision_kat.py (the parallel capsules) by the restatement: its own check, and the oracle's output."""
    import mujoco_torch_amd as mt
    from test_collision_kat import KATS

    n = 0
    for kat, (xml, check) in sorted(KATS.items()):
        mx = mt.device_put(mt.mjcf.from_xml_string(xml))
        pairs = ref.pairs_of(mx.tables)
        if not pairs or any(p[0] >= ref.FN_IN_KERNEL for p in pairs):
            continue
        out = oracle_run(mx, mt.make_data(mx))
        ncon = mx.constraint_sizes_py[3]
        C = ref.reference(pairs, mx.tables.pair_dst, ncon, out["geom_xpos"].reshape(1, -1, 3), out["geom_xmat"].reshape(1, -1, 9), np.asarray(mx.geom_size, dtype=np.float64))
        check(ps.f64(C.dist[0]), ps.f64(C.pos[0]), ps.f64(C.frame[0]))
        got = ps.contact_leaves(out, 1, ncon)
        for leaf in ps.LEAVES:
            assert rel_err(got[leaf], ps.f64(ps._as_leaves(C)[leaf])) <= TOL_PRE[ps.F64], (kat, leaf)
        n += 1
    assert n >= 1


@pytest.mark.parametrize("dtype", [ps.F64, ps.F32], ids=["f64", "f32"])
def test_comparable_leaves_little_out(dtype, oracle_lib):
    """With the reference alone: at most 1 % of a drawn entry's contacts left out, nothing of an exact or either-side entry."""
    eps = float(torch.finfo(dtype).eps)
    total, gone, near = 0, 0, 0
    for e in ps.TABLE:
        if dtype not in e.dtypes or e.kind in ("nearpar", "topk"):
            continue
        mx, d = ps.placed(e.name, dtype)
        out = oracle_run(mx, d)
        C = ps.reference_of(mx, out["geom_xpos"], out["geom_xmat"])
        keep = C.against(C.pos, eps)[1]
        left = max(int((~keep[k]).sum()) for k in ps.LEAVES)
        if e.kind in ("exact", "side"):
            assert left == 0, (e.name, left)
            continue
        assert left <= 0.01 * keep["pos"].size, (e.name, left, keep["pos"].size)
        total, gone = total + keep["pos"].size, gone + left
        sw = np.stack([C.margin[k] for k in ("frame_sw", "pc_bn", "pc_n1")])
        near += int((np.nan_to_num(sw, nan=1.0).min(0) < 1e-3).sum())
    print(f"{dtype}: {gone} of {total} drawn contacts left out; {near} within 1e-3 of a 0.5 switch")
