"""Plane-cylinder / plane-ellipsoid collisions, CPU part (tests/test_quadric.py is the GPU part).

The recordings tests/golden/quadric/*.npz are the reference's own steps with its own plane_ellipsoid / plane_cylinder registered in its driver table
(tools/gen_quadric_golden.py).  They sit in a directory of their own: the CPU oracle does not know the two pair functions, so these models cannot go through
the tests that run it on every tests/golden/*.npz.  Here: the static tables against the recorded integer leaves, the numpy longdouble restatement
(tests/_quadric_ref.py) against the recorded contacts -- which pins the yardstick of the GPU tests -- and the refusals that stay.
"""
import re

import numpy as np
import pytest
import torch

import mujoco_torch_amd as mt
from mujoco_torch_amd import collision_tables as ct
from mujoco_torch_amd import native
from mujoco_torch_amd._enums import GeomType
from _cases import TOL_PRE
from _quadric_ref import FN_PLANE_CYLINDER, FN_PLANE_ELLIPSOID, pair_contacts
from _util import Golden, leaf, rel_err

CASES = ["quadric/euler_newton_pyr_f64", "quadric/euler_cg_ell_f64", "quadric/rk4_newton_ell_f32", "quadric/topk_f64"]
MIN_LEN, PAR_BAND = 0.05, (0.9e-3, 1.1e-3)  # what tools/gen_quadric_golden.py keeps every recorded plane-cylinder pair clear of

_GOLDEN = {}


def golden(case):
    if case not in _GOLDEN:
        _GOLDEN[case] = Golden(case)
    return _GOLDEN[case]


def test_tables_and_header_name_the_same_ids():
    text = open(native.HEADER).read()
    assert re.search(r"#define MJH_FN_PLANE_ELLIPSOID 9\b", text) and re.search(r"#define MJH_FN_PLANE_CYLINDER 10\b", text)
    assert re.search(r"#define MJH_KERNEL_QUADRIC 44\b", text) and re.search(r"#define MJH_MAX_PAIR_CONTACTS 4\b", text)
    assert ct.COLLISION_FN[(GeomType.PLANE, GeomType.ELLIPSOID)] == (ct.FN_PLANE_ELLIPSOID, 1) == (FN_PLANE_ELLIPSOID, 1)
    assert ct.COLLISION_FN[(GeomType.PLANE, GeomType.CYLINDER)] == (ct.FN_PLANE_CYLINDER, 3) == (FN_PLANE_CYLINDER, 3)
    others = [k for k in ct.COLLISION_FN if (GeomType.ELLIPSOID in k or GeomType.CYLINDER in k) and k[0] != GeomType.PLANE]
    assert not others  # every other cylinder / ellipsoid key stays refused


def test_scene_has_what_it_is_meant_to_have():
    """Both new pair functions beside an in-kernel primitive pair, two planes, and all three parameter sources (pair / priority / dynamic)."""
    mx = golden(CASES[0]).model
    fns = [p[0] for p in mx.tables.pairs]
    assert fns.count(FN_PLANE_CYLINDER) == 5 and fns.count(FN_PLANE_ELLIPSOID) == 2 and fns.count(1) == 1 and len(fns) == 8
    assert [p[1] for p in mx.tables.pairs] == [3, 3, 3, 3, 3, 1, 1, 2]  # contacts per pair; the cylinder group comes first
    assert {p[2].geom1 for p in mx.tables.pairs} == {0, 1}
    sources = {(p[2].ipair > -1, p[2].geomp > -1) for p in mx.tables.pairs}
    assert sources == {(True, False), (False, True), (False, False)}
    assert sorted({p[2].dim for p in mx.tables.pairs}) == [3, 4, 6]
    assert golden("quadric/topk_f64").model.tables.topk and not mx.tables.topk


@pytest.mark.parametrize("case", CASES)
def test_static_tables_match_the_recorded_integer_leaves(case):
    g = golden(case)
    assert tuple(g.model.constraint_sizes_py) == tuple(g.meta["constraint_sizes"])
    d = mt.make_data(g.model)
    ncon = g.model.constraint_sizes_py[3]
    for e in range(g.nenv):
        for s in range(g.nsteps):
            for n in ("contact_dim", "contact_efc_address"):
                assert np.array_equal(leaf(d, n).numpy(), g.expected(e, s, n)), (n, e, s)
            if not g.model.tables.topk:
                for n in ("contact_geom1", "contact_geom2", "contact_geom"):
                    assert np.array_equal(leaf(d, n).numpy(), g.expected(e, s, n)), (n, e, s)
            else:  # max_contact_points: which candidates are kept is decided per step -- every kept contact is one of the model's pairs
                pairs = {(p[2].geom1, p[2].geom2) for p in g.model.tables.pairs}
                got = list(zip(g.expected(e, s, "contact_geom1").tolist(), g.expected(e, s, "contact_geom2").tolist()))
                assert len(got) == ncon and set(got) <= pairs


def _compare(g, e, s, tol):
    """The restatement on the recorded geom frames against the recorded contacts of the new pairs: (worst error, contacts compared)."""
    xpos, xmat = g.expected(e, s, "geom_xpos"), g.expected(e, s, "geom_xmat")
    dist, pos, frame = g.expected(e, s, "contact_dist"), g.expected(e, s, "contact_pos").reshape(-1, 3), g.expected(e, s, "contact_frame").reshape(-1, 9)
    g1, g2 = g.expected(e, s, "contact_geom1"), g.expected(e, s, "contact_geom2")
    want_d, want_p, want_f, slots = np.array(dist, dtype=np.float64), np.array(pos, dtype=np.float64), np.array(frame, dtype=np.float64), []
    for c in pair_contacts(g.model, xpos, xmat):
        if c["fn"] == FN_PLANE_CYLINDER:
            assert c["info"]["len"] >= MIN_LEN and not PAR_BAND[0] <= c["info"]["prj_half"] <= PAR_BAND[1], (e, s, c["pair"], c["info"])
        if not g.model.tables.topk:
            dst = c["dst"]
            use = range(len(dst))
        else:  # the kept contacts of this pair, each matched to the nearest of its candidates (two rim contacts share a distance: position decides)
            dst = np.nonzero((g1 == c["geom1"]) & (g2 == c["geom2"]))[0]
            cd, cp = np.asarray(c["dist"], dtype=np.float64), np.asarray(c["pos"], dtype=np.float64)
            use = [int(np.argmin(np.maximum(np.abs(cd - dist[t]), np.abs(cp - pos[t]).max(1)))) for t in dst]
            assert len(set(use)) == len(use)
        for t, k in zip(dst, use):
            want_d[t], want_p[t], want_f[t] = c["dist"][k], c["pos"][k], c["frame"][k].reshape(-1)
            slots.append(int(t))
    assert len(set(slots)) == len(slots)
    err = max(rel_err(dist, want_d), rel_err(pos, want_p), rel_err(frame, want_f))
    assert err <= tol, (e, s, err)
    return err, len(slots)


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_the_recorded_contacts(case):
    """tests/_quadric_ref.py on the recorded geom_xpos / geom_xmat == the reference's recorded contact_dist / pos / frame of the new pairs at TOL_PRE, every
    environment and step, both dtypes; every recorded plane-cylinder pair is clear of the function's two discontinuities (asserted, no case left out)."""
    g = golden(case)
    worst, n = 0.0, 0
    for e in range(g.nenv):
        for s in range(g.nsteps):
            err, k = _compare(g, e, s, TOL_PRE[g.dtype])
            worst, n = max(worst, err), n + k
    print(f"{case}: {n} contacts, worst {worst:.2e} = {worst / TOL_PRE[g.dtype]:.2e} of TOL_PRE")
    assert n >= (g.nenv * g.nsteps * 17 if not g.model.tables.topk else g.nenv * g.nsteps)


def test_recordings_cover_the_par_branch_and_both_contact_states():
    g = golden(CASES[0])
    par = disk = active = apart = 0
    for e in range(g.nenv):
        for s in range(g.nsteps):
            cs = pair_contacts(g.model, g.expected(e, s, "geom_xpos"), g.expected(e, s, "geom_xmat"))
            par += sum(c["info"].get("par", False) for c in cs)
            disk += sum(c["fn"] == FN_PLANE_CYLINDER and not c["info"]["par"] for c in cs)
            gap = g.expected(e, s, "contact_dist") - g.expected(e, s, "contact_includemargin")
            active, apart = active + int((gap < 0).sum()), apart + int((gap > 0).sum())
    assert par > 0 and disk > 0 and active > 0 and apart > 0, (par, disk, active, apart)


_REFUSED = {
    "sphere-cylinder": ('<geom type="sphere" size="0.1"/>', '<geom type="cylinder" size="0.1 0.1"/>', "(SPHERE, CYLINDER)"),
    "box-ellipsoid": ('<geom type="box" size="0.1 0.1 0.1"/>', '<geom type="ellipsoid" size="0.1 0.08 0.05"/>', "(ELLIPSOID, BOX)"),
    "cylinder-cylinder": ('<geom type="cylinder" size="0.1 0.1"/>', '<geom type="cylinder" size="0.1 0.1"/>', "(CYLINDER, CYLINDER)"),
}


@pytest.mark.parametrize("name", list(_REFUSED))
def test_other_cylinder_and_ellipsoid_pairs_are_still_refused(name):
    a, b, key = _REFUSED[name]
    xml = f"""<mujoco><worldbody><geom type="plane" size="1 1 .01"/>
      <body pos="0 0 0.2"><joint type="free"/>{a}</body><body pos="0.3 0 0.2"><joint type="free"/>{b}</body></worldbody></mujoco>"""
    with pytest.raises(NotImplementedError, match="collisions not implemented") as ei:
        mt.device_put(mt.mjcf.from_xml_string(xml))
    assert key in str(ei.value)


def test_plane_only_models_are_accepted_in_both_dtypes():
    xml = """<mujoco><worldbody><geom type="plane" size="1 1 .01"/>
      <body pos="0 0 0.2"><joint type="free"/><geom type="cylinder" size="0.1 0.1"/></body>
      <body pos="0.5 0 0.2"><joint type="free"/><geom type="ellipsoid" size="0.1 0.08 0.05" contype="2" conaffinity="2"/></body></worldbody></mujoco>"""
    for dtype in (None, torch.float32):
        mx = mt.device_put(mt.mjcf.from_xml_string(xml), dtype=dtype)
        assert mx.constraint_sizes_py[3] == 3  # the ellipsoid (contype 2) meets nothing, the cylinder meets the plane: three contacts
