"""The convex narrow phase (csrc/mjh_convex.h: one wavefront per environment and pair) on hulls larger than that wavefront.

Every selection of the kernel is a loop `for (i = lane; i < n; i += 64)` with a per-lane running best and a wave-wide arg-best after it; the hulls of the other
tests (at most 20 vertices, 12 faces, 5 vertices per face) never take such a loop past its first trip.  convex_large.xml does: 100 vertices / 196 faces / 294 edges
(blob100), 18 vertices per face with 4 -> 18 padding (prism18), 88 vertices with subsampled caps (prism44), in all four pair functions.  The poses are the ones
recorded from the reference (tests/golden/convex_large_*.npz); tests/test_convex_large_host.py shows on the CPU that float64 meets no narrow-phase tie on them
and counts the float32 ones.  The full step on the same recordings is tests/test_gpu_parity.py::test_step_matches_reference_golden's (directory listing).

The refusal of a hull whose pair needs more LDS scratch than a workgroup has is decided by the device library at model creation, which the CPU stand-in of the
host tests never reaches: it is tested here.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mujoco_torch_amd as mt
import pyoracle
from _cases import TOL_PRE
from _convex_large import PropertyTally, check_properties
from _util import GOLD, INT_LEAVES, REAL_LEAVES, Golden, assert_leaves_close, gpu_out_to_numpy, rel_err
from mujoco_torch_amd import native
from test_convex_large_host import CONTACT_LEAVES, F32_TIE_FLAGGED

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
NARROW = 0x07  # kinematics, inertia, collision


def step_inputs(g, s):
    """Batched input Data of recorded step s (teacher-forced: the reference's own output of step s - 1)."""
    d = g.input_data()
    for t in range(s):
        d = pyoracle.apply(d, {n: np.stack([g.expected(e, t, n) for e in range(g.nenv)]) for n in REAL_LEAVES + INT_LEAVES})
    return d


def contact_bits(out):
    return {n: out[n] for n in CONTACT_LEAVES + ["geom_xpos", "geom_xmat"]}


@pytest.mark.parametrize("case", ["convex_large_f64", "convex_large_f32"])
def test_narrow_phase_matches_the_reference_and_the_properties(case, oracle_lib):
    """forward(stages = kinematics + inertia + collision) on the recorded inputs: contact_dist / contact_pos / contact_frame against the recording at TOL_PRE, every
    environment and step.  Float64 admits no oracle alternative (no tie on these poses, shown on the CPU); float32 may verify an environment through the oracle with
    tie hints, only on the env-steps the CPU count flagged.  The longdouble properties of tests/_convex_large.py hold on the same output at the dtype's eps."""
    g = Golden(case)
    mdev = g.model.to("cuda")
    tol, eps = TOL_PRE[g.dtype], float(torch.finfo(g.dtype).eps)
    worst, via_oracle, tally = 0.0, 0, PropertyTally()
    for s in range(g.nsteps):
        d = step_inputs(g, s)
        out = gpu_out_to_numpy(mt.forward(mdev, d.to("cuda"), stages=NARROW))
        for e in range(g.nenv):
            err = max(rel_err(out[n][e], g.expected(e, s, n)) for n in CONTACT_LEAVES)
            print(f"{case} step{s} env{e}: contact leaves {err:.2e} ({err / tol:.2e} of TOL_PRE)")
            if err > tol and g.dtype == torch.float32 and (e, s) in F32_TIE_FLAGGED:  # only where the CPU count found a tie outcome
                via_oracle += 1
                want = pyoracle.run(g.model, d[e], step=False, stages=NARROW, contact_hint={n: out[n][e] for n in CONTACT_LEAVES})
                assert_leaves_close(lambda n: out[n][e], lambda n: want[n], tol, names=CONTACT_LEAVES, what=f"{case} step{s} env{e} (oracle, tie hints)")
            else:
                assert err <= tol, f"{case} step{s} env{e}: contact leaves {err:.3e} beyond {tol:g}"
                worst = max(worst, err)
            tally.add(check_properties({n: out[n][e] for n in out}, g.model, eps))
    print(f"{case}: worst contact leaf {worst / tol:.2e} of TOL_PRE, {via_oracle} env-steps through the oracle; {tally}")
    tally.assert_covered()
    assert via_oracle <= (len(F32_TIE_FLAGGED) if g.dtype == torch.float32 else 0)


@pytest.mark.parametrize("case", ["convex_large_f64", "convex_large_f32"])
def test_contacts_do_not_depend_on_placement_in_the_batch(case):
    """The recorded environments tiled to B = 24 in a shuffled order, and each one alone (B = 1), give the bits of the B = nenv run: no lane, wave or workgroup of
    the pair grid reads another environment's scratch."""
    g = Golden(case)
    mdev = g.model.to("cuda")
    d = g.input_data()
    base = contact_bits(gpu_out_to_numpy(mt.forward(mdev, d.to("cuda"), stages=NARROW)))
    order = np.random.RandomState(24).permutation(np.arange(24) % g.nenv)
    assert set(order.tolist()) == set(range(g.nenv))
    tiled = contact_bits(gpu_out_to_numpy(mt.forward(mdev, d[torch.as_tensor(order)].to("cuda"), stages=NARROW)))
    for n in base:
        assert np.array_equal(tiled[n], base[n][order]), n
    for e in range(g.nenv):
        one = contact_bits(gpu_out_to_numpy(mt.forward(mdev, d[e : e + 1].to("cuda"), stages=NARROW)))
        for n in base:
            assert np.array_equal(one[n][0], base[n][e]), (n, e)


_CUT_CHILD = r'''
import sys
sys.path.insert(0, "tests"); sys.path.insert(0, "mujoco-torch_amd"); sys.path.insert(0, "oracle")
import numpy as np, torch, mujoco_torch_amd as mt
from mujoco_torch_amd import native
from _util import Golden
out = {}
for case in ("convex_large_f64", "convex_large_f32"):
    g = Golden(case)
    got = mt.forward(g.model.to("cuda"), g.input_data().to("cuda"), stages=0x07)
    out[case] = {n: native.data_field_tensor(got, n).cpu() for n in ("contact_dist", "contact_pos", "contact_frame")}
torch.save(out, sys.argv[1])
print("ran")
'''


def test_cut_launches_give_the_same_bits(tmp_path):
    """MJH_MAX_GRID_LOG2=2 caps a launch at 4 workgroups: the convex launcher takes four times that, 16 workgroups, so the 11 pairs x 5 (6) environments
    go out as 4 (5) launches whose boundaries fall inside an environment (16 is no multiple of 11).
    The switch is read once per process, so each setting runs in a fresh child."""
    res = {}
    for tag, env in (("one", {}), ("cut", {"MJH_MAX_GRID_LOG2": "2"})):
        f = str(tmp_path / (tag + ".pt"))
        base = {k: v for k, v in os.environ.items() if k != "MJH_MAX_GRID_LOG2"}
        r = subprocess.run([sys.executable, "-c", _CUT_CHILD, f], cwd=ROOT, env=dict(base, **env), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "ran" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
        res[tag] = torch.load(f)
    for case in res["one"]:
        for n, t in res["one"][case].items():
            assert torch.equal(t, res["cut"][case][n]), (case, n)


_MIXED_K = """<mujoco model="mixed_k">
  <compiler meshdir="{meshdir}"/>
  <asset><mesh name="prism18" file="prism18.stl"/></asset>
  <worldbody>
    <geom name="floor" type="plane" size="40 40 40" contype="0" conaffinity="0"/>
    <body name="box" pos="0 0 0.2"><joint type="free"/><geom type="box" size="0.05 0.04 0.03"/></body>
    <body name="prism18" pos="0.158 0 0.2"><joint type="free"/><geom type="mesh" mesh="prism18"/></body>
  </worldbody>
</mujoco>
"""


def test_mixed_face_widths_box_against_prism18(tmp_path, oracle_lib):
    """Plane + box + prism18 with the box-prism18 pair alone (K = 18 against the box's 4): fv()'s replicate padding 4 -> 18 and the 43 K part of the scratch, away
    from the paths only many vertices reach.  Eight seeded poses, float64, against the oracle at TOL_PRE with no tie outcome admitted."""
    xml = tmp_path / "mixed_k.xml"
    xml.write_text(_MIXED_K.format(meshdir=os.path.join(GOLD, "meshes")))
    mx = mt.device_put(mt.mjcf.from_xml_path(str(xml)))
    assert [p[0] for p in mx.tables.pairs] == [8] and mx.tables.convex[1]["face"].shape[1] == 4 and mx.tables.convex[2]["face"].shape[1] == 18
    B, rng = 8, np.random.RandomState(18)
    q = mt.make_data(mx).qpos.expand(B, -1).clone()
    for a in (0, 7):
        q[:, a : a + 3] += torch.tensor(0.012 * rng.randn(B, 3))
        q[:, a + 3 : a + 7] = torch.tensor(rng.randn(B, 4))
    d = mt.make_data(mx).expand(B).clone().replace(qpos=q)
    out = gpu_out_to_numpy(mt.forward(mx.to("cuda"), d.to("cuda"), stages=NARROW))
    ties = np.zeros(B, dtype=np.int32)
    want = pyoracle.run(mx, d, step=False, stages=NARROW, contact_hint={n: out[n] for n in CONTACT_LEAVES}, tie_pairs=ties)
    touching = int((out["contact_dist"].min(1) < 0).sum())
    worst = max(rel_err(out[n], want[n]) for n in CONTACT_LEAVES)
    print(f"mixed K: {touching}/{B} poses in contact, worst contact leaf {worst:.2e} ({worst / TOL_PRE[torch.float64]:.2e} of TOL_PRE), tie outcomes {ties.tolist()}")
    assert 2 <= touching < B
    assert int(ties.sum()) == 0 and worst <= TOL_PRE[torch.float64]


def test_hull_too_large_for_the_scratch_is_refused_in_float64_only(tmp_path):
    """A convex-convex pair of two 700-vertex hulls needs 3 (V1 + F1 + V2 + F2) + 43 K + 8 reals of LDS scratch: past a workgroup's 64 KiB in float64, inside it in
    float32.  The float64 model is refused at creation with the library's -12 message, the float32 one is accepted.  The models are only built, never stepped."""
    import make_convex_large as mk

    mk.write_stl(str(tmp_path / "blob700.stl"), mk.hull_triangles(mk.ellipsoid_points(700, seed=700)))
    xml = tmp_path / "too_large.xml"
    xml.write_text(f"""<mujoco model="too_large">
  <compiler meshdir="{tmp_path}"/>
  <asset><mesh name="a" file="blob700.stl"/><mesh name="b" file="blob700.stl" scale="0.9 0.8 0.7"/></asset>
  <worldbody>
    <body pos="0 0 0.2"><joint type="free"/><geom type="mesh" mesh="a"/></body>
    <body pos="0.2 0 0.2"><joint type="free"/><geom type="mesh" mesh="b"/></body>
  </worldbody>
</mujoco>
""")
    lite = mt.mjcf.from_xml_path(str(xml))
    dev = torch.device("cuda:0")
    for dtype, size in ((torch.float64, 8), (torch.float32, 4)):
        mx = mt.device_put(lite, dtype=None if dtype == torch.float64 else dtype)
        t1, t2 = mx.tables.convex[0], mx.tables.convex[1]
        need = 3 * (len(t1["vert"]) + len(t1["face"]) + len(t2["vert"]) + len(t2["face"])) + 43 * max(t1["face"].shape[1], t2["face"].shape[1])
        bytes_needed = (need + 8) * size
        print(f"{dtype}: {len(t1['vert'])} vertices, {len(t1['face'])} faces, scratch {bytes_needed} B of {64 * 1024}")
        if dtype == torch.float64:
            assert bytes_needed > 64 * 1024
            with pytest.raises(RuntimeError, match=r"mjh_model_create failed \(-12\): convex hull too large for the pair kernel's LDS scratch"):
                native.get_native_model(mx.to("cuda"), dev, dtype)
        else:
            assert bytes_needed <= 64 * 1024
            assert native.get_native_model(mx.to("cuda"), dev, dtype).handle
