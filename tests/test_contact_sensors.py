"""contact_force / sensor_postconstraint on the GPU: the contact forces against the tests' numpy reference (tests/_contact_sensors_ref.py, fed the GPU pass's own
leaves) in both frames, the Jacobian identity J^T f = sum of efc_J rows times efc_force (independent of the decode), the touch and frame-acceleration sensors
against the reference, the siblings' results bit for bit, the qvel= override, input safety, and independence of packing and batch cuts.

Measured on an MI355X (printed by the tests):
  Jacobian identity, worst |lhs - rhs| / allowance: capsules_topk 0.011, ant cone 1 float32 0.0002, touch_rig 0.006, convex_primitives 0.002.
  touch, (hits, misses, excluded, direction-dependent) of the (contact, sensor) pairs per case: touch_rig cone 0 float64 (139, 263, 0, 29) of 402, cone 1 float64
  (127, 245, 0, 25) of 372, cone 0 float32 (140, 262, 0, 30) of 402, cone 1 float32 (125, 247, 0, 25) of 372; ant (32, 0, 0, 0) of 32.  rodtip is clipped at its
  cutoff in 6 (cone 0) / 5 (cone 1) of 16 environments.  contact_force: at most 0.041 of its bound in either frame on every case."""
import numpy as np
import pytest
import torch

import _contact_sensors_ref as cr
import _postcon_ref as pr
import _support_ref as sr
import mujoco_torch_amd as mt
from _cases import seeded_batch
from _postcon_ref import HP, within
from _util import load_model

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64, F32 = torch.float64, torch.float32
FIVE = ("cacc", "cfrc_int", "cfrc_ext", "subtree_linvel", "subtree_angmom")
_PASSES = {}


def _id(c):
    return f"{c[0]}-{'-'.join(f'{k}{v}' for k, v in c[1].items()) or 'default'}-{str(c[2])[11:]}"


def loaded_pass(xml, ov=None, dtype=F64, B=8, steps=3):
    """A forward pass on the GPU a few steps after the seeded pose (shared by the tests of this module; never written).  touch_rig: the recipe of
    tests/test_contact_sensors_host.py (seed 7, qpos0 + 0.02 randn, qvel = 0.3 randn); every other model: the seeded batch with random xfrc_applied."""
    key = (xml, tuple(sorted((ov or {}).items())), dtype, B, steps)
    if key not in _PASSES:
        if xml == "touch_rig":
            mc = load_model(xml, ov or {}, dtype)
            rng = np.random.RandomState(7)
            d = mt.make_data(mc).expand(B).clone()
            d = d.replace(qpos=d.qpos + torch.tensor(0.02 * rng.randn(B, mc.nq)), qvel=torch.tensor(0.3 * rng.randn(B, mc.nv)))
            d = d if dtype == F64 else d.to(dtype)
        else:
            mc, d = seeded_batch(xml, ov or {}, dtype, B)
            rng = np.random.RandomState(5)
            d = d.replace(xfrc_applied=torch.tensor(2.0 * rng.randn(B, int(mc.nbody), 6), dtype=dtype))
        mx, d = mc.to(DEV), d.to(DEV)
        for _ in range(steps):
            d = mt.step(mx, d)
        _PASSES[key] = (mx, mt.forward(mx, d))
    return _PASSES[key]


# ---- contact_force against the reference ---------------------------------------------------------------------------------------------------------------

FORCE_CASES = [("touch_rig", {"cone": 0}, F64, 16), ("touch_rig", {"cone": 1}, F64, 16), ("touch_rig", {"cone": 0}, F32, 16), ("touch_rig", {"cone": 1}, F32, 16),
               ("ant", {"cone": 0}, F64, 8), ("ant", {"cone": 1}, F32, 8), ("capsules_topk", {}, F64, 8), ("boxes_topk", {}, F64, 8),
               ("convex_primitives", {"cone": 0}, F64, 4), ("convex_primitives", {"cone": 1}, F64, 4), ("mesh_contact", {}, F32, 4), ("humanoid", {}, F64, 8),
               ("centipede_154", {}, F32, 2), ("cartpole", {}, F64, 8)]


@pytest.mark.parametrize("xml,ov,dtype,B", FORCE_CASES, ids=[_id(c) for c in FORCE_CASES])
def test_contact_force_against_the_reference(xml, ov, dtype, B):
    mx, f = loaded_pass(xml, ov, dtype, B)
    ncon = int(mx.constraint_sizes_py[3])
    local, world = mt.contact_force(mx, f), mt.contact_force(mx, f, to_world_frame=True)
    assert tuple(local.shape) == tuple(world.shape) == (B, ncon, 6) and local.dtype == world.dtype == dtype and local.device == f.qpos.device
    if xml == "cartpole":  # no contacts: an empty result
        assert ncon == 0 and local.numel() == 0
        return
    T, L = pr.tables(mx), pr.leaves_of(f)
    eps = torch.finfo(dtype).eps
    for got, to_world in ((local, False), (world, True)):
        val, S, n = cr.contact_force(T, L, to_world)
        g = got.cpu().numpy()
        worst = float((np.abs(g.astype(HP) - val).astype(np.float64) / np.maximum(pr.bound(n, eps, S), 1e-300)).max())
        print(f"{xml} {'world' if to_world else 'contact'} frame: worst error {worst:.3f} of its bound; max |w| {float(np.abs(val).max()):.3e}")
        within(g, val, pr.bound(n, eps, S), f"{xml} contact_force to_world={to_world}")
        assert float(np.abs(g).max()) > 0, "every force is zero"
        if not to_world:  # pure copies (elliptic cone, dim 1, skipped slots) are the same bits
            cp = cr.copies(T, L)
            assert cp.any() or T["pyramidal"]
            assert np.array_equal(g[cp], np.asarray(val, dtype=g.dtype)[cp])
    if xml.endswith("_topk"):  # run-time slots: a slot without geoms (-1), or whose rows do not lie inside efc_force, gives zeros; the other slots do not move
        geom, adr = f.contact.geom.clone(), f.contact.efc_address.clone()
        geom[0::4, 0, 0], geom[1::4, 0, 1], geom[2::4, 0, 1] = -1, -1, int(mx.ngeom)  # (slot 0 is the loaded one in these passes)
        adr[3::4, 0] = int(mx.constraint_sizes_py[4]) - 1
        edited = f.replace(contact=f.contact.replace(geom=geom, efc_address=adr))
        for frame, full in ((False, local), (True, world)):
            got = mt.contact_force(mx, edited, to_world_frame=frame)
            assert not bool(got[:, 0].any()) and torch.equal(got[:, 1:], full[:, 1:]) and int(full[:, 0].any(-1).sum()) >= 4
    if xml == "convex_primitives":
        assert {4, 6} <= set(np.unique(L["contact_dim"]).tolist()) and float(local[..., 3:].abs().max()) > 0  # torsional / rolling rows are decoded
    # contact_id: an int, a flat sequence
    assert torch.equal(mt.contact_force(mx, f, contact_id=ncon - 1), local[:, ncon - 1])
    assert torch.equal(mt.contact_force(mx, f, contact_id=[ncon - 1, 0], to_world_frame=True), world[:, [ncon - 1, 0]])
    assert tuple(mt.contact_force(mx, f[0], contact_id=0).shape) == (6,) and torch.equal(mt.contact_force(mx, f[0]), local[0])  # no batch dimension


# ---- the Jacobian identity -----------------------------------------------------------------------------------------------------------------------------

IDENTITY_CASES = [("capsules_topk", {}, F64, 8), ("ant", {"cone": 1}, F32, 8), ("touch_rig", {"cone": 0}, F64, 16), ("convex_primitives", {"cone": 0}, F64, 4)]


@pytest.mark.parametrize("xml,ov,dtype,B", IDENTITY_CASES, ids=[_id(c) for c in IDENTITY_CASES])
def test_contact_forces_project_like_the_constraint_rows(xml, ov, dtype, B):
    """For every environment: sum_c [apply_ft(f, tau, pos, b2) - apply_ft(f, tau, pos, b1)], with (f, tau) = contact_force(..., to_world_frame=True), equals
    sum over the contacts' rows of efc_J[row] efc_force[row] from the pass's own leaves.  It does not use the decode: a pyramid's rows enter the right side
    one by one.  Allowance: _support_ref.bound of both sides -- the left one's terms are the 6 products per query and dof (evaluated here in HP from the
    device's forces, which carry the decode's and the rotation's roundings: + 16), the right one's the rows -- plus one such term for the rounding of efc_J
    itself, whose entries are sums of nv + JACP_ROUNDINGS rounded terms."""
    mx, f = loaded_pass(xml, ov, dtype, B)
    T, L = pr.tables(mx), pr.leaves_of(f)
    ncon, nefc, nv = int(mx.constraint_sizes_py[3]), int(mx.constraint_sizes_py[4]), int(mx.nv)
    world = mt.contact_force(mx, f, to_world_frame=True).cpu().numpy().astype(HP)
    J, p = f.efc_J.cpu().numpy().reshape(B, nefc, nv).astype(HP), L["efc_force"].astype(HP)
    mask, root = sr.ancestor_mask(mx.body_parentid, mx.dof_bodyid), np.asarray(mx.body_rootid)
    eps = torch.finfo(dtype).eps
    worst, loaded = 0.0, 0
    for e in range(B):
        lhs, s_lhs, rhs, s_rhs, nq, nrow = np.zeros(nv, dtype=HP), np.zeros(nv, dtype=HP), np.zeros(nv, dtype=HP), np.zeros(nv, dtype=HP), 0, 0
        for c in range(ncon):
            g1, g2 = int(L["contact_geom"][e, c, 0]), int(L["contact_geom"][e, c, 1])
            if g1 < 0 or g2 < 0:
                continue
            dim, adr = int(L["contact_dim"][e, c]), int(L["contact_efc_address"][e, c])
            rows = 2 * (dim - 1) if T["pyramidal"] and dim > 1 else dim
            rhs += (J[e, adr:adr + rows] * p[e, adr:adr + rows, None]).sum(0)
            s_rhs += np.abs(J[e, adr:adr + rows] * p[e, adr:adr + rows, None]).sum(0)
            nrow += rows
            ids = [int(T["geom_bodyid"][g1]), int(T["geom_bodyid"][g2])]
            pts = np.broadcast_to(L["contact_pos"][e, c], (1, 2, 3))
            v, s = sr.apply_ft_hp(L["cdof"][e:e + 1], L["subtree_com"][e:e + 1], root, mask, pts, np.stack([-world[e, c, :3], world[e, c, :3]])[None],
                                  np.stack([-world[e, c, 3:], world[e, c, 3:]])[None], ids)
            lhs += v[0].sum(0)
            s_lhs += s[0].sum(0)
            nq += 2
        allowed = sr.bound(6 * nq + 16, eps, s_lhs) + sr.bound(nrow, eps, s_rhs) + sr.bound(nv + sr.JACP_ROUNDINGS, eps, s_rhs)
        err = np.abs(lhs - rhs).astype(np.float64)
        worst = max(worst, float((err / np.maximum(allowed, 1e-300)).max()))
        loaded += int(np.abs(rhs).max() > 0)
        within(lhs, rhs, allowed, f"{xml} environment {e}")
    print(f"{xml}: Jacobian identity, worst |lhs - rhs| / allowance {worst:.4f} over {B} environments ({loaded} with contact forces)")
    assert loaded > 0


# ---- touch ---------------------------------------------------------------------------------------------------------------------------------------------

def _names(mx):
    return mx.tables.source.names_site


def _touch_check(mx, f, out, what, eps, misses_exist=True):
    """The touch slots of `out` against the reference, with the cap on excluded decisions: at most 5 % of the (contact, sensor) pairs, and at least 20 hits, 20
    misses and 5 direction-dependent decisions left (misses_exist=False: a model whose zones enclose their bodies, where every decision is a hit)."""
    L = cr.leaves_of(f, cacc=out.cacc)
    sens = [r for r in cr.evaluate(mx, L, np.asarray(mx.site_size)) if r["row"][0] == cr.TOUCH]
    sd = out.sensordata.cpu().numpy()
    hits = misses = excluded = direction = 0
    for r in sens:
        adr = r["row"][1]
        slack = np.zeros(sd.shape[0])
        for e, dec in enumerate(r["decisions"]):
            for (_, w0, _, hit, fragile, dirdep) in dec:
                if fragile:  # an excluded decision: the slot may or may not hold its term
                    excluded += 1
                    slack[e] += float(w0)
                    continue
                hits, misses, direction = hits + bool(hit), misses + (not hit), direction + bool(dirdep)
        within(sd[:, adr], r["value"][:, 0], pr.bound(r["n"][:, 0], eps, r["S"][:, 0]) + slack, f"{what} touch on site {_names(mx)[r['row'][2]]}")
    pairs = hits + misses + excluded
    print(f"{what}: touch (hits, misses, excluded, direction-dependent) = ({hits}, {misses}, {excluded}, {direction}) of {pairs} (contact, sensor) pairs")
    assert excluded <= 0.05 * pairs and hits >= 20, (hits, misses, excluded, direction)
    assert (misses >= 20 and direction >= 5) if misses_exist else misses == 0, (hits, misses, excluded, direction)
    return sens, sd


RIG_CASES = [({"cone": 0}, F64), ({"cone": 1}, F64), ({"cone": 0}, F32), ({"cone": 1}, F32)]


@pytest.mark.parametrize("ov,dtype", RIG_CASES, ids=[_id(("touch_rig",) + c) for c in RIG_CASES])
def test_touch_on_the_rig_against_the_reference(ov, dtype):
    B = 16
    mx, f = loaded_pass("touch_rig", ov, dtype, B)
    out = mt.sensor_postconstraint(mx, f)
    eps = torch.finfo(dtype).eps
    sens, sd = _touch_check(mx, f, out, f"touch_rig {ov} {dtype}", eps)
    by = {_names(mx)[r["row"][2]]: r for r in sens}
    # `whole` is the sum of the positive normal forces of the slab's slots, in slot order
    w0 = mt.contact_force(mx, f)[..., 0].cpu().numpy().astype(HP)
    slab = int(by["whole"]["row"][4])
    bodies = pr.tables(mx)["geom_bodyid"][np.maximum(f.contact.geom.cpu().numpy(), 0)]
    on = (bodies == slab).any(-1) & (f.contact.geom.cpu().numpy() >= 0).all(-1) & (w0 > 0)
    assert on.any(1).all()
    within(sd[:, by["whole"]["row"][1]], (w0 * on).sum(1), pr.bound(on.sum(1), eps, (np.abs(w0) * on).sum(1)), "whole against contact_force")
    assert not sd[:, by["above"]["row"][1]].any()  # exactly 0
    tip = by["rodtip"]
    clipped = np.asarray(tip["raw"][:, 0] > 1.5 + pr.bound(tip["n"][:, 0], eps, tip["S"][:, 0]))
    print(f"rodtip: {int(clipped.sum())} of {B} environments clipped at 1.5; largest unclipped value {float(tip['raw'].max()):.3f}")
    assert clipped.any() and (sd[clipped, tip["row"][1]] == 1.5).all() and (sd[:, tip["row"][1]] <= 1.5).all()
    # Model.site_size is read at each call: `above` grown tenfold reaches the slab's contacts
    size = np.array(mx.site_size)
    size[_names(mx).index("above")] *= 10
    grown = mt.sensor_postconstraint(mx.replace(site_size=size), f).sensordata[:, by["above"]["row"][1]]
    assert bool((grown > 0).any())
    assert torch.equal(mt.sensor_postconstraint(mx, f).sensordata, out.sensordata)  # ... and the original sizes are back with the original Model


def test_touch_on_the_ant_against_the_reference():
    """The ant's nine zones enclose the geoms of their bodies, and its loaded contacts (the four aux / leg capsule pairs) lie on the zones' axes: all 32 decisions
    at B = 8 are hits from inside the zone, whatever the pose (checked on the CPU oracle at 3, 40 and 120 steps).  So this case holds the values, the cap on
    exclusions and the floor on hits; misses and the direction rule are held on touch_rig, where they exist."""
    mx, f = loaded_pass("ant", {"cone": 0}, F64, 8)
    out = mt.sensor_postconstraint(mx, f)
    sens, sd = _touch_check(mx, f, out, "ant", torch.finfo(F64).eps, misses_exist=False)
    assert sum(float(np.abs(sd[:, r["row"][1]]).max()) > 0 for r in sens) == 4  # the four leg zones read a force


# ---- framelinacc / frameangacc -------------------------------------------------------------------------------------------------------------------------

FRAME_CASES = [("touch_rig", {"cone": 0}, F64, 16), ("touch_rig", {"cone": 1}, F32, 16), ("sensor_rig2", {}, F64, 9), ("sensor_rig2", {}, F32, 9)]


@pytest.mark.parametrize("xml,ov,dtype,B", FRAME_CASES, ids=[_id(c) for c in FRAME_CASES])
def test_frame_accelerations_against_the_reference(xml, ov, dtype, B):
    mx, f = loaded_pass(xml, ov, dtype, B)
    out = mt.sensor_postconstraint(mx, f)
    eps = torch.finfo(dtype).eps
    L = cr.leaves_of(f, cacc=out.cacc)
    sens = [r for r in cr.evaluate(mx, L, np.asarray(mx.site_size)) if r["row"][0] != cr.TOUCH]
    sd = out.sensordata.cpu().numpy()
    kinds = set()
    for r in sens:
        t, adr, _, kind, body = r["row"][:5]
        kinds.add((t, kind))
        got = sd[:, adr:adr + 3]
        if t == cr.FRAMEANGACC:
            assert r["row"][8] == 0 and np.array_equal(got, out.cacc[:, body, :3].cpu().numpy()), r["row"]  # a copy: the same bits
        else:
            assert float(np.abs(got).max()) > 0
            within(got, r["value"], pr.bound(r["n"], eps, r["S"]), f"{xml} framelinacc {r['row']}")
    if xml == "touch_rig":
        assert kinds == {(33, 3), (34, 3), (33, 0), (33, 1), (33, 2), (34, 4)}  # site, body, xbody, geom; site, camera
        # the accelerometer on the same site is the same vector in the site's frame (its arithmetic is pinned to the reference's by tests/test_postconstraint.py)
        src = mx.tables.source
        acc = [int(a) for a, t in zip(np.asarray(src.sensor_adr), np.asarray(src.sensor_type)) if int(t) == pr.ACCELEROMETER][0]
        lin = [r for r in sens if r["row"][0] == cr.FRAMELINACC and r["row"][3] == 3][0]
        R = L["site_xmat"][:, lin["row"][2]].reshape(B, 3, 3).astype(HP)
        rot = np.einsum("bji,bj->bi", R, sd[:, lin["row"][1]:lin["row"][1] + 3].astype(HP))
        S = np.einsum("bji,bj->bi", np.abs(R), np.asarray(lin["S"], dtype=HP))
        within(rot, sd[:, acc:acc + 3], 16 * eps * S.astype(np.float64), "site_xmat^T framelinacc against the accelerometer")
    else:
        assert kinds == {(33, 3)}


# ---- the siblings' results, the override, input safety -------------------------------------------------------------------------------------------------

def _new_slots(mx):
    rows = np.asarray(mx.tables.contact_sensors["rows"])
    mask = np.zeros(int(mx.nsensordata), dtype=bool)
    for r in rows:
        mask[r[1]:r[1] + (1 if r[0] == cr.TOUCH else 3)] = True
    return torch.tensor(mask, device=DEV)


@pytest.mark.parametrize("xml,ov,dtype,B", [("touch_rig", {"cone": 0}, F64, 16), ("sensor_rig2", {}, F64, 9), ("sensor_rig2", {}, F32, 9), ("ant", {"cone": 1}, F32, 8)],
                         ids=["touch_rig", "sensor_rig2-f64", "sensor_rig2-f32", "ant"])
def test_everything_else_is_fwd_postconstraint_bit_for_bit(xml, ov, dtype, B):
    mx, f = loaded_pass(xml, ov, dtype, B)
    new = _new_slots(mx)
    assert new.any() and not new.all()
    want, got = mt.fwd_postconstraint(mx, f, sensors=True), mt.sensor_postconstraint(mx, f)
    for n in FIVE:
        assert torch.equal(getattr(got, n), getattr(want, n)), n
    assert torch.equal(got.sensordata[:, ~new], want.sensordata[:, ~new])
    assert torch.equal(want.sensordata[:, new], f.sensordata[:, new]) and not torch.equal(got.sensordata[:, new], f.sensordata[:, new])  # only the new call evaluates them
    # the qvel= override after step: the same relation on the pre-step state
    s = mt.step(mx, f)
    want, got = mt.fwd_postconstraint(mx, s, qvel=f.qvel, sensors=True), mt.sensor_postconstraint(mx, s, qvel=f.qvel)
    for n in FIVE:
        assert torch.equal(getattr(got, n), getattr(want, n)), n
    assert torch.equal(got.sensordata[:, ~new], want.sensordata[:, ~new])
    assert not torch.equal(got.cacc, mt.sensor_postconstraint(mx, s).cacc)


def test_models_without_these_sensors_degrade_to_the_sibling():
    for xml, ov in (("touch_rig", {"disableflags": 1 << 13}), ("cartpole", {})):  # DisableBit.SENSOR; a model without sensors
        mx, f = loaded_pass(xml, ov, F64, 4, steps=1)
        assert len(mx.tables.contact_sensors["rows"]) == 0
        want, got = mt.fwd_postconstraint(mx, f, sensors=True), mt.sensor_postconstraint(mx, f)
        for n in FIVE + ("sensordata",):
            assert torch.equal(getattr(got, n), getattr(want, n)), (xml, n)


def test_the_input_is_not_written_and_the_other_leaves_alias_it():
    mx, f = loaded_pass("touch_rig", {"cone": 0}, F64, 16)
    names = [n for n in cr.LEAVES if not n.startswith("contact_")] + list(FIVE)
    before = {n: getattr(f, n).clone() for n in names}
    con = {n: getattr(f.contact, n).clone() for n in ("pos", "frame", "friction", "contact_dim", "geom", "efc_address")}
    out, force = mt.sensor_postconstraint(mx, f), mt.contact_force(mx, f, to_world_frame=True)
    for n, t in before.items():
        assert torch.equal(getattr(f, n), t), n
    for n, t in con.items():
        assert torch.equal(getattr(f.contact, n), t), n
    for n in ("qpos", "qvel", "cvel", "qM", "efc_force", "xfrc_applied", "site_xpos"):
        assert getattr(out, n).data_ptr() == getattr(f, n).data_ptr(), n
    assert out.contact.pos.data_ptr() == f.contact.pos.data_ptr()
    for n in FIVE + ("sensordata",):
        assert getattr(out, n).data_ptr() != getattr(f, n).data_ptr(), n
    assert force.data_ptr() not in (f.efc_force.data_ptr(), f.contact.frame.data_ptr())


def test_refusals_on_the_device():
    mx, f = loaded_pass("touch_rig", {"cone": 0}, F64, 16)
    ncon = int(mx.constraint_sizes_py[3])
    with pytest.raises(ValueError, match="contact_id"):
        mt.contact_force(mx, f, contact_id=ncon)
    with pytest.raises(ValueError, match="efc_force"):
        mt.contact_force(mx, f.replace(efc_force=f.efc_force.float()))
    with pytest.raises(ValueError, match="efc_force"):
        mt.contact_force(mx, f.replace(efc_force=f.efc_force.cpu()))
    with pytest.raises(ValueError, match="geom_xpos"):
        mt.sensor_postconstraint(mx, f.replace(geom_xpos=f.geom_xpos[:, :-1]))
    with pytest.raises(NotImplementedError, match="contact_force"):
        torch.vmap(lambda q: mt.contact_force(mx, f.replace(qpos=q)))(f.qpos)
    with pytest.raises(RuntimeError, match="HIP device"):
        mt.contact_force(mx.to("cpu"), f.to("cpu"))


# ---- packing and cuts ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("xml,ov,dtype", [("ant", {"cone": 1}, F32), ("humanoid", {}, F64), ("touch_rig", {"cone": 0}, F64)], ids=["ant", "humanoid", "touch_rig"])
def test_results_do_not_depend_on_packing_or_cuts(xml, ov, dtype):
    B = 70
    mx, f = loaded_pass(xml, ov, dtype, B, steps=2)
    full = (mt.contact_force(mx, f), mt.contact_force(mx, f, to_world_frame=True), mt.sensor_postconstraint(mx, f).sensordata)
    assert float(full[0].abs().max()) > 0
    for sl in (slice(4, 5), slice(9, 12), slice(2, 69)):  # 1, 3 and 67 environments
        part = (mt.contact_force(mx, f[sl]), mt.contact_force(mx, f[sl], to_world_frame=True), mt.sensor_postconstraint(mx, f[sl]).sensordata)
        for a, b in zip(part, full):
            assert torch.equal(a, b[sl]), sl
