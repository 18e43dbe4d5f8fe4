"""contact_force / sensor_postconstraint without a GPU: the public functions and their refusals, the tests' own numpy reference (tests/_contact_sensors_ref.py)
held to closed forms on forward passes of the CPU oracle (tests/_hostsim.py), and the hit / miss / fragile counts of the touch_rig fixture the GPU tests rely on."""
import re

import numpy as np
import pytest
import torch

import _contact_sensors_ref as cr
import _hostsim
import _postcon_ref as pr
import mujoco_torch_amd as mt
from _postcon_ref import within
from _util import load_model

EPS = float(np.finfo(np.float64).eps)
G = 9.81


@pytest.fixture
def hostsim(monkeypatch):
    return _hostsim.install(monkeypatch)


@pytest.fixture(scope="module")
def rig():
    mx = load_model("touch_rig")
    return mx, mt.make_data(mx).expand(4).clone()


# ---- the public functions ----------------------------------------------------------------------------------------------------------------

def test_the_functions_and_the_entry_point_are_public():
    from mujoco_torch_amd import native

    for n in ("contact_force", "sensor_postconstraint"):
        assert callable(getattr(mt, n)), n
    assert hasattr(native, "ContactSensorArgs") and native.ABI_VERSION >= 17
    text = open(native.HEADER).read()
    assert re.search(r"\bint mjh_contact_sensors\s*\(const mjhModel\* m, const mjhContactSensorArgs\* args, void\* hip_stream\);", text)
    for i, n in enumerate(("FORCES", "SENSORS", "WORLD")):
        assert re.search(rf"#define MJH_CONSENS_{n} {1 << i}\b", text)
    # the ctypes struct names the header's fields, in order
    body = text[text.index("typedef struct mjhContactSensorArgs {"):text.index("} mjhContactSensorArgs;")]
    fields = re.findall(r"[*\s,](\w+)(?=[,;])", body.split("{", 1)[1])
    assert fields == [f[0] for f in native.ContactSensorArgs._fields_], fields


def test_the_new_sensors_have_a_table_of_their_own(rig):
    mx, _ = rig
    rows = np.asarray(mx.tables.contact_sensors["rows"])
    assert sorted(set(rows[:, 0].tolist())) == [cr.TOUCH, cr.FRAMELINACC, cr.FRAMEANGACC]
    assert sorted(set(rows[rows[:, 0] != cr.TOUCH, 3].tolist())) == [0, 1, 2, 3, 4]  # body, xbody, geom, site, camera
    assert sorted(set(np.asarray(mx.tables.source.sensor_objtype).tolist())) == [1, 2, 5, 6, 7]
    assert set(rows[rows[:, 0] == cr.TOUCH, 7].tolist()) == {cr.SPHERE, cr.CAPSULE, cr.ELLIPSOID, cr.CYLINDER, cr.BOX}
    assert not set(np.asarray(mx.tables.sensors["type"]).tolist()) & {cr.TOUCH, cr.FRAMELINACC, cr.FRAMEANGACC}  # (no pass evaluates them)
    ref = cr.sensor_rows(mx)
    assert [tuple(r) for r in rows.tolist()] == [r[:8] for r in ref] and list(mx.tables.contact_sensors["cutoff"]) == [r[8] for r in ref]
    off = load_model("touch_rig", {"disableflags": 1 << 13})  # DisableBit.SENSOR
    assert len(off.tables.contact_sensors["rows"]) == 0


def test_cpu_data_is_refused(rig):
    mx, d = rig
    for call in (lambda: mt.contact_force(mx, d), lambda: mt.contact_force(mx, d, contact_id=0, to_world_frame=True), lambda: mt.sensor_postconstraint(mx, d),
                 lambda: mt.sensor_postconstraint(mx, d, qvel=d.qvel.clone())):
        with pytest.raises(RuntimeError, match="HIP device"):
            call()


def test_shapes_dtypes_and_contact_ids_are_validated(rig):
    mx, d = rig
    ncon = int(mx.constraint_sizes_py[3])
    assert ncon > 2
    for bad in (ncon, -1, [0, ncon], [[0, 1]], 1.5, [0.5], True):
        with pytest.raises(ValueError, match="contact_id"):
            mt.contact_force(mx, d, contact_id=bad)
    with pytest.raises(ValueError, match="efc_force"):
        mt.contact_force(mx, d.replace(efc_force=d.efc_force[:, :-1]))
    with pytest.raises(ValueError, match="efc_force"):
        mt.contact_force(mx, d.replace(efc_force=d.efc_force.to(torch.float32)))
    with pytest.raises(ValueError, match="qpos"):
        mt.contact_force(mx, d.replace(qpos=d.qpos[:, :-1]))
    with pytest.raises(ValueError, match="dtype"):
        mt.contact_force(mx, d.to(torch.float32))
    with pytest.raises(ValueError, match="geom_xpos"):
        mt.sensor_postconstraint(mx, d.replace(geom_xpos=d.geom_xpos[:, :-1]))
    with pytest.raises(ValueError, match="cam_xpos"):
        mt.sensor_postconstraint(mx, d.replace(cam_xpos=d.cam_xpos.to(torch.float32)))
    with pytest.raises(ValueError, match="site_size"):
        mt.sensor_postconstraint(mx.replace(site_size=mx.site_size[:-1]), d)
    with pytest.raises(ValueError, match="qvel="):
        mt.sensor_postconstraint(mx, d, qvel=torch.zeros(int(mx.nv), dtype=torch.float64))


@pytest.mark.parametrize("name", ["contact_force", "sensor_postconstraint"])
def test_vmap_is_refused_by_name(rig, name):
    mx, d = rig
    pick = (lambda o: o) if name == "contact_force" else (lambda o: o.qpos)
    with pytest.raises(NotImplementedError, match=name):
        torch.vmap(lambda q: pick(getattr(mt, name)(mx, d.replace(qpos=q))))(d.qpos)


def test_a_touch_zone_of_an_unsupported_shape_is_refused(rig):
    _, d = rig
    types = np.asarray(load_model("touch_rig").site_type).tolist()
    types[0] = 7  # a mesh: no site shape
    mx = load_model("touch_rig", {"model.site_type": types})
    with pytest.raises(NotImplementedError, match="touch sensor on site 0"):
        mt.sensor_postconstraint(mx, d)


# ---- closed forms on the reference -----------------------------------------------------------------------------------------------------------

_BOX = """<mujoco><option timestep="0.002"/><worldbody>
  <geom type="plane" size="2 2 0.1"/>
  <body name="box" pos="0 0 0.0995"><joint type="free"/><geom type="box" size="0.15 0.1 0.1" mass="2.5"/><site name="whole" type="box" size="0.2 0.2 0.2"/></body>
</worldbody><sensor><touch site="whole"/></sensor></mujoco>"""
_FIXED = """<mujoco><worldbody>
  <body name="fixed" pos="0.3 0.2 1"><geom type="box" size="0.1 0.2 0.3" mass="2.5"/><site name="s" pos="0.05 0 0.1"/></body>
  <body name="swing" pos="2 0 1"><joint type="hinge" axis="0 1 0"/><geom type="sphere" size="0.1" pos="0.2 0 0" mass="1"/></body>
</worldbody><sensor><framelinacc objtype="site" objname="s"/><frameangacc objtype="site" objname="s"/></sensor></mujoco>"""
_ARM = """<mujoco><option gravity="0 0 0"/><worldbody>
  <body name="arm" pos="0 0 1"><joint type="hinge" axis="0 0 1"/><geom type="sphere" size="0.05" pos="0.4 0 0" mass="1"/><site name="s" pos="0.7 0 0"/></body>
</worldbody><sensor><framelinacc objtype="site" objname="s"/><frameangacc objtype="xbody" objname="arm"/></sensor></mujoco>"""


def _xml_pass(xml, qvel=None, steps=0):
    mx = mt.device_put(mt.mjcf.from_xml_string(xml))
    d = mt.make_data(mx).expand(1).clone()
    if qvel is not None:
        d = d.replace(qvel=torch.tensor([qvel], dtype=torch.float64))
    for _ in range(steps):
        d = mt.step(mx, d)
    return mx, mt.forward(mx, d)


def _sensors(mx, f):
    """The reference's sensors on an oracle pass, with the reference's own cacc."""
    cacc = np.asarray(pr.evaluate(pr.tables(mx), pr.leaves_of(f), subtree=False)["cacc"][0], dtype=np.float64)
    L = cr.leaves_of(f, cacc=torch.tensor(cacc))
    return cr.evaluate(mx, L, np.asarray(mx.site_size)), L


def test_a_box_at_rest_is_carried_by_its_touch_zone(hostsim):
    """Newton's law for the free box: the normal forces sum to m (g + a_z).  The pass obeys it as far as its solver converged -- the residual
    M qacc - qfrc_smooth - qfrc_constraint is below opt.tolerance * meaninertia * nv, what the solver's gradient test lets through -- and after settling a_z is
    small, so `whole` = m g within m |a_z| + that residual (+ the rounding of the sum)."""
    mx, f = _xml_pass(_BOX, steps=300)
    (touch,), L = _sensors(mx, f)
    m, az = 2.5, float(f.qacc[0, 2])
    tol = float(mx.opt.tolerance) * float(mx.stat.meaninertia) * int(mx.nv)
    assert abs(az) < 1e-3 * G, az  # at rest
    dec = touch["decisions"][0]
    assert len(dec) >= 3 and all(d[3] and not d[4] for d in dec)  # the loaded corners, all inside the zone
    print(f"box: whole {float(touch['value'][0, 0]):.9f}, m g {m * G:.9f}, m a_z {m * az:.3e}, solver allowance {tol:.3e}")
    within(touch["value"][0, 0], m * (G + az), tol + pr.bound(touch["n"][0, 0], EPS, touch["S"][0, 0]), "whole against m (g + a_z)")
    within(touch["value"][0, 0], m * G, m * abs(az) + tol + pr.bound(touch["n"][0, 0], EPS, touch["S"][0, 0]), "whole against m g")
    # contact_force of the reference: the normal forces are the touch terms; a condim-3 contact carries no torque
    val, S, n = cr.contact_force(pr.tables(mx), L)
    assert float(val[0, :, 0].sum()) == float(touch["raw"][0, 0]) and not val[0, :, 3:].any()


def test_a_body_fixed_to_the_world_feels_gravity(hostsim):
    mx, f = _xml_pass(_FIXED)
    (lin, ang), _ = _sensors(mx, f)
    within(lin["value"][0], [0, 0, G], pr.bound(lin["n"][0], EPS, lin["S"][0]) + 16 * EPS * G, "framelinacc")
    assert not np.asarray(ang["value"][0], dtype=np.float64).any()


def test_a_spinning_arm_reads_the_centripetal_acceleration(hostsim):
    w, rad = 3.0, 0.7
    mx, f = _xml_pass(_ARM, qvel=[w])
    assert float(f.qacc.abs().max()) < 1e-13  # nothing accelerates the joint
    (lin, ang), _ = _sensors(mx, f)
    within(lin["value"][0], [-w * w * rad, 0, 0], pr.bound(lin["n"][0], EPS, lin["S"][0]) + 64 * EPS * w * w * rad, "framelinacc")  # (+ the oracle's kinematics)
    assert np.abs(np.asarray(ang["value"][0], dtype=np.float64)).max() < 1e-12


# ---- the fixture -----------------------------------------------------------------------------------------------------------------------------

ISSUE_ZONES = ("whole", "half", "corner", "below", "above", "top", "rodskin", "rodtip")
ADDED_ZONES = ("edge", "pad", "rodfoot")  # capsule, ellipsoid, cylinder


def rig_counts(mx, leaves):
    """Per zone (hits, misses, fragile, direction-dependent) over all environments, and the number of (contact, sensor) pairs."""
    rows = [r for r in cr.evaluate(mx, leaves, np.asarray(mx.site_size)) if r["row"][0] == cr.TOUCH]
    names = [mx.tables.source.names_site[r["row"][2]] for r in rows]
    out, pairs = {}, 0
    for name, r in zip(names, rows):
        dec = [d for env in r["decisions"] for d in env]
        pairs += len(dec)
        out[name] = (sum(d[3] for d in dec), sum(not d[3] for d in dec), sum(d[4] for d in dec), sum(d[5] for d in dec))
    return out, pairs


@pytest.mark.parametrize("cone", [0, 1])
@pytest.mark.parametrize("steps", [3, 25])
def test_touch_rig_decides_robustly(hostsim, cone, steps):
    """B = 16, seed 7, qpos0 + 0.02 randn, qvel = 0.3 randn: every zone but `above` is hit, every zone but `whole` / `rodskin` is missed, `below` is hit
    from outside the zone (the direction rule decides), and no decision flips under a scaling of the zone by 1 +- 1e-3."""
    mx = load_model("touch_rig", {"cone": cone})
    rng = np.random.RandomState(7)
    d = mt.make_data(mx).expand(16).clone()
    d = d.replace(qpos=d.qpos + torch.tensor(0.02 * rng.randn(16, mx.nq)), qvel=torch.tensor(0.3 * rng.randn(16, mx.nv)))
    for _ in range(steps):
        d = mt.step(mx, d)
    f = mt.forward(mx, d)
    counts, pairs = rig_counts(mx, cr.leaves_of(f))
    print(f"touch_rig cone {cone}, {steps} steps: {pairs} pairs; (hits, misses, fragile, direction-dependent) per zone: {counts}")
    issue_pairs = sum(sum(counts[z][:2]) for z in ISSUE_ZONES)
    # measured on this fixture: 298 / 276 / 268 / 292 pairs over the eight zones the fixture's description names (it leaves the masses open), 19 - 24 of them
    # decided by the direction rule; per zone 3 - 45 hits and 6 - 45 misses
    assert 260 <= issue_pairs <= 300, issue_pairs
    for z in ISSUE_ZONES + ADDED_ZONES:
        hits, misses, fragile, _ = counts[z]
        assert fragile == 0, z
        assert (hits == 0) if z == "above" else (3 <= hits <= 45), (z, hits)
        assert (misses == 0) if z in ("whole", "rodskin") else (6 <= misses <= 45), (z, misses)
    assert 19 <= sum(counts[z][3] for z in ISSUE_ZONES) <= 25
    assert counts["below"][3] == counts["below"][0] > 0  # every hit of `below` is one from outside the zone
    # what the GPU tests ask of a case (tests/test_contact_sensors.py): at least 20 hits, 20 misses, 5 direction-dependent decisions
    assert sum(c[0] for c in counts.values()) >= 20 and sum(c[1] for c in counts.values()) >= 20 and sum(c[3] for c in counts.values()) >= 5
