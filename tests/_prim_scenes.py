"""The family of scenes of tests/test_primitive_contacts.py and its host twin: MJCF built in code, one free body of sphere / capsule geoms (two where the arrangement needs
two movers) over static spheres, capsules and a plane in the world, poses set through ``qpos``, a different pose per environment.

Every entry states the CONDITION it exists for (``Entry.why``); ``conditions(entry)`` proves it from the placed model's tables and the reference's margins, not from the name.
The batch is 5 (not a multiple of the four environments of a packed wavefront) for every entry whose poses are drawn; an entry of exact arrangements has one environment
per arrangement (7, 5, 5, 11; ``side-capsules`` 9: none a multiple of four); ``n15`` runs at B = 1.

Pair counts.  A body geom collides with every world geom, a ``plane-only`` one (contype = conaffinity = 2, the plane has 3) with the plane alone; the world geoms come
spheres, capsules, plane, so the pair groups come sphere-sphere, sphere-capsule, capsule-capsule, plane-sphere, plane-capsule and the layouts below -- the fewest geoms a
search over (static spheres, static capsules, body spheres, body capsules, plane-only spheres and capsules, their order) found -- give exactly 1, 15, 16, 17, 32, 33, 64, 65
and 135 in-kernel pairs, with a two-contact plane-capsule pair as the LAST pair of a trip of 16, 32 and 64 lanes (pair W - 1, and pair W is none) or as the FIRST pair of
the next trip (pair W, and pair W - 1 is none).
"""
import functools
from dataclasses import dataclass, field

import numpy as np
import torch

import _prim_ref as ref
import mujoco_torch_amd as mt

F64, F32 = torch.float64, torch.float32
NPDT = {F64: np.float64, F32: np.float32}
B = 5
QI = (1.0, 0.0, 0.0, 0.0)
QX = (0.5, 0.5, 0.5, 0.5)      # z -> x (x -> y, y -> z): exact in every precision
QY = (0.5, -0.5, -0.5, -0.5)   # z -> y
QFLIP = (0.0, 1.0, 0.0, 0.0)   # z -> -z


def _fmt(v):
    return " ".join(repr(float(x)) for x in np.atleast_1d(v))


def quat_z_to(v):
    """Unit quaternion (w first) rotating +z onto ``v``."""
    v = np.asarray(v, dtype=np.float64) / np.linalg.norm(v)
    ax = np.cross([0.0, 0.0, 1.0], v)
    s, c = np.linalg.norm(ax), v[2]
    if s < 1e-12:
        return np.array(QI if c > 0 else QFLIP)
    ang = np.arctan2(s, c)
    return np.concatenate([[np.cos(ang / 2)], np.sin(ang / 2) * ax / s])


def sphere(r, pos=(0, 0, 0), **kw):
    return dict(type="sphere", size=(r,), pos=pos, quat=QI, **kw)


def capsule(r, hl, pos=(0, 0, 0), quat=QI, **kw):
    return dict(type="capsule", size=(r, hl), pos=pos, quat=quat, **kw)


def plane(pos=(0, 0, 0), quat=QI, **kw):
    return dict(type="plane", size=(5, 5, 0.1), pos=pos, quat=quat, **kw)


def _geom_xml(g):
    extra = "".join(f' {k}="{v}"' for k, v in g.items() if k not in ("type", "size", "pos", "quat"))
    return f'<geom type="{g["type"]}" size="{_fmt(g["size"])}" pos="{_fmt(g["pos"])}" quat="{_fmt(g["quat"])}"{extra}/>'


@dataclass
class Entry:
    name: str
    kind: str            # random | mixed | params | exact | side | nearpar | topk
    why: str
    world: list
    bodies: list         # one list of geoms per free body
    poses: np.ndarray    # [B, 7 * len(bodies)] qpos of the free bodies
    dtypes: tuple = (F64, F32)
    option: dict = field(default_factory=dict)
    max_contact_points: int = -1
    contact_xml: str = ""
    want: dict = field(default_factory=dict)  # what conditions() must find

    @property
    def B(self):
        return self.poses.shape[0]


def xml_of(e, dummies=0, floss=False, uncapped=False, **option):
    """The entry's MJCF.  ``uncapped``: without its max_contact_points (the twin whose contacts are the capped model's candidates).  ``dummies``: further free bodies whose geom collides with nothing (they only add dofs: 2 take a one-body scene to nv = 18); ``floss``: one more body on a
    hinge with frictionloss (one friction row: the general constraint phase); ``option``: attributes of <option> over the entry's own."""
    opt = dict(e.option, **option)
    out = ["<mujoco>", "<option " + " ".join(f'{k}="{v}"' for k, v in opt.items()) + "/>"]
    if e.max_contact_points > -1 and not uncapped:
        out.append(f'<custom><numeric name="max_contact_points" data="{e.max_contact_points}"/></custom>')
    out.append('<default><geom condim="1"/></default><worldbody>')
    out += [_geom_xml(g) for g in e.world]
    for geoms in e.bodies:
        out.append('<body pos="0 0 1"><joint type="free"/>' + "".join(_geom_xml(g) for g in geoms) + "</body>")
    for i in range(dummies):
        out.append(f'<body pos="{3 + i} 0 1"><joint type="free"/><geom type="sphere" size="0.1" contype="0" conaffinity="0"/></body>')
    if floss:
        out.append('<body pos="-3 0 1"><joint type="hinge" axis="0 0 1" frictionloss="0.1"/><geom type="sphere" size="0.1" pos="0.2 0 0" contype="0" conaffinity="0"/></body>')
    out.append("</worldbody>" + e.contact_xml + "</mujoco>")
    return "\n".join(out)


@functools.lru_cache(maxsize=None)
def _placed(name, dtype, dummies, floss, uncapped, option):
    e = BY_NAME[name]
    mx = mt.device_put(mt.mjcf.from_xml_string(xml_of(e, dummies, floss, uncapped, **dict(option))), dtype=None if dtype == F64 else dtype)
    d0 = mt.make_data(mx)
    q = np.repeat(np.asarray(d0.qpos, dtype=np.float64)[None], e.B, 0)
    q[:, : e.poses.shape[1]] = e.poses
    d = d0.expand(e.B).clone().replace(qpos=torch.tensor(q))
    return mx, (d if dtype == F64 else d.to(dtype))


def placed(name, dtype=F64, dummies=0, floss=False, uncapped=False, **option):
    """(host Model, host Data [B]) of an entry or one of its variants, cached."""
    return _placed(name, dtype, dummies, floss, uncapped, tuple(sorted(option.items())))


def slots(mx):
    """Slots of the narrow phase's own arrays: the contacts, or with max_contact_points the candidates."""
    return len(mx.tables.contact_perm)


def reference_of(mx, geom_xpos, geom_xmat):
    return ref.reference(ref.pairs_of(mx.tables), mx.tables.pair_dst, slots(mx), geom_xpos, geom_xmat, np.asarray(mx.geom_size, dtype=np.float64))


def same_dtype_of(mx, geom_xpos, geom_xmat, dtype):
    return ref.evaluate(ref.pairs_of(mx.tables), mx.tables.pair_dst, slots(mx), geom_xpos, geom_xmat, np.asarray(mx.geom_size, dtype=np.float64), NPDT[dtype])


# ---- drawn poses ---------------------------------------------------------------------------------------------------------------------------------------

def _unit_quats(rng, n):
    q = rng.randn(n, 4)
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def _drawn_geom(rng, kind, box, **kw):
    pos = rng.uniform(-1, 1, 3) * box
    if kind == "S":
        return sphere(round(rng.uniform(0.05, 0.12), 3), pos, **kw)
    return capsule(round(rng.uniform(0.04, 0.09), 3), round(rng.uniform(0.1, 0.25), 3), pos, _unit_quats(rng, 1)[0], **kw)


TILT = quat_z_to([0.12, -0.2, 1.0])  # the plane: tilted and off the origin


def drawn(name, why, ws, wc, order, counts, seed, batch=B, want=None, **kw):
    """``ws`` / ``wc`` static spheres / capsules and the plane in the world; the body's geoms in ``order`` over S, C (every world geom) and XS, XC (the plane only)."""
    rng = np.random.RandomState(seed)
    world = [_drawn_geom(rng, "S", (0.35, 0.35, 0.25)) for _ in range(ws)] + [_drawn_geom(rng, "C", (0.35, 0.35, 0.25)) for _ in range(wc)]
    for g in world:
        g["pos"] = np.asarray(g["pos"]) + [0, 0, 0.45]
    world.append(plane((0.1, -0.2, 0.05), TILT, contype=3, conaffinity=3))
    body = []
    for k in order:
        po = dict(contype=2, conaffinity=2) if k[0] == "X" else {}
        body += [_drawn_geom(rng, k[-1], (0.25, 0.25, 0.25), **po) for _ in range(counts[k])]
    poses = np.concatenate([rng.uniform(-0.1, 0.1, (batch, 2)), rng.uniform(0.35, 0.55, (batch, 1)), _unit_quats(rng, batch)], 1)
    return Entry(name, kw.pop("kind", "random"), why, world, [body], poses, want=want or {}, **kw)


def _counts(a, c, xs=0, xc=0):
    return dict(S=a, C=c, XS=xs, XC=xc)


SCXX, CSXX = ("S", "C", "XS", "XC"), ("C", "S", "XS", "XC")
PC = ref.FN_PLANE_CAPSULE
TABLE = [
    drawn("n1", "one pair: a single lane works", 0, 0, SCXX, _counts(0, 0, 1), 1, want=dict(npair=1)),
    drawn("n15", "15 pairs: one short of the 16 lanes of a packed environment; the B = 1 case", 1, 1, SCXX, _counts(1, 4), 15, batch=1, want=dict(npair=15)),
    drawn("n16-last", "16 pairs, pair 15 a plane-capsule pair: a trip of 16 lanes exactly full", 1, 2, SCXX, _counts(1, 3), 16, want=dict(npair=16, pc=[15])),
    drawn("n17-last", "17 pairs, the two-contact pair last in the first trip of 16", 1, 2, CSXX, _counts(1, 3, 0, 1), 17, want=dict(npair=17, pc=[15], not_pc=[16])),
    drawn("n17-first", "17 pairs, the two-contact pair first in the second trip of 16", 1, 2, SCXX, _counts(3, 1, 1, 0), 18, want=dict(npair=17, pc=[16], not_pc=[15])),
    drawn("n32-last", "32 pairs, pair 31 a plane-capsule pair: a trip of 32 lanes exactly full", 1, 2, SCXX, _counts(1, 7), 32, want=dict(npair=32, pc=[31])),
    drawn("n33-last", "33 pairs, the two-contact pair last in the first trip of 32", 1, 2, CSXX, _counts(1, 7, 0, 1), 33, want=dict(npair=33, pc=[31], not_pc=[32])),
    drawn("n33-first", "33 pairs, the two-contact pair first in the second trip of 32", 1, 2, SCXX, _counts(7, 1, 1, 0), 34, want=dict(npair=33, pc=[32], not_pc=[31])),
    drawn("n64-last", "64 pairs, pair 63 a plane-capsule pair: a trip of 64 lanes exactly full", 3, 4, SCXX, _counts(1, 7), 64, want=dict(npair=64, pc=[63])),
    drawn("n65-last", "65 pairs, the two-contact pair last in the first trip of 64", 3, 4, CSXX, _counts(1, 7, 0, 1), 65, want=dict(npair=65, pc=[63], not_pc=[64])),
    drawn("n65-first", "65 pairs, the two-contact pair first in the second trip of 64", 3, 4, SCXX, _counts(7, 1, 1, 0), 66, want=dict(npair=65, pc=[64], not_pc=[63])),
    drawn("n135", "at least 129 pairs: a third trip of 64 lanes, a ninth of 16", 4, 4, SCXX, _counts(6, 9), 135, want=dict(npair_min=129)),
]


# ---- mixed condims, parameter sources ------------------------------------------------------------------------------------------------------------------------

def _mixed(name, cone):
    e = drawn(name, f"condims 1, 3, 4 and 6 on primitives in an order where contact_order is not the identity, {cone}", 1, 1, ("S", "C"), dict(S=2, C=2), 77, kind="mixed",
              option=dict(cone=cone), want=dict(condims={1, 3, 4, 6}, permuted=True))
    e.world[0]["condim"], e.world[1]["condim"], e.world[2]["condim"] = 3, 1, 1
    for g, c in zip(e.bodies[0], (1, 4, 6, 3)):
        g["condim"] = c
    return e


def _params():
    e = drawn("params", "an explicit <pair>, a higher-priority geom and the dynamic mix with unequal solmix, margin and gap", 1, 1, ("S", "C"), dict(S=2, C=2), 78, kind="params",
              want=dict(sources={(True, False), (False, True), (False, False)}))
    e.world[0].update(name="ws", solmix=2.0, margin=0.02, gap=0.005, friction="0.8 0.01 0.002", solref="0.03 0.9", solimp="0.8 0.9 0.002 0.5 2", condim=3)
    e.world[1].update(solmix=0.5, margin=0.035, gap=0.01, friction="1.1 0.02 0.001", solref="0.015 1.1", condim=4)
    e.world[2].update(margin=0.01, solmix=1.5)
    b = e.bodies[0]
    b[0].update(name="b0", solmix=0.25, margin=0.05, gap=0.02, friction="0.6 0.03 0.004", solimp="0.85 0.97 0.003 0.4 3", condim=3)
    b[1].update(priority=1, margin=0.03, gap=0.004, friction="1.3 0.04 0.003", solref="0.025 0.8", condim=6)
    b[2].update(solmix=3.0, margin=0.015, friction="0.9 0.005 0.0001", solref="0.02 1.0")
    b[3].update(solmix=0.75, gap=0.012, solimp="0.7 0.92 0.004 0.6 2")
    e.contact_xml = ('<contact><pair geom1="ws" geom2="b0" condim="4" friction="0.7 0.65 0.01 0.002 0.003" solref="0.035 0.95" solreffriction="0.04 1.2" '
                     'solimp="0.75 0.93 0.002 0.5 2" margin="0.04" gap="0.0125"/></contact>')
    return e


TABLE += [_mixed("mixed-pyramidal", "pyramidal"), _mixed("mixed-elliptic", "elliptic"), _params()]


# ---- exact arrangements: every coordinate is a small dyadic number, every rotation a signed permutation ---------------------------------------------------------

def _pose(*bodies):
    return np.concatenate([np.concatenate([np.asarray(p, dtype=np.float64), np.asarray(q, dtype=np.float64)]) for p, q in bodies])


def _exact_entries():
    out = []
    c0 = np.array([0.5, -0.25, 1.0])
    deltas = [(0, 0, 0), (0.5, 0, 0), (-0.5, 0, 0), (0, 0.5, 0), (0, -0.5, 0), (0, 0, 0.5), (0, 0, -0.5)]
    out.append(Entry("exact-spheres", "exact", "two spheres with bit-identical centres, and with normals along +-x, +-y, +-z", [], [[sphere(0.25)], [sphere(0.125)]],
                     np.stack([_pose((c0, QI), (c0 + np.array(dl), QI)) for dl in deltas]), want=dict(coincident=1, axis_normals=6)))
    # capsule (r 0.125, half-length 0.25) and sphere (r 0.25) over the z-plane: standing (b = y), flipped, lying along x and y, a sphere touching the plane (dist == 0), the
    # sphere beyond the a-cap, beyond the b-cap and abreast of the middle of the capsule
    out.append(Entry("exact-plane-z", "exact", "a capsule standing along the normal of a z-plane (b = y), lying in it, a sphere exactly touching it; sphere-capsule beyond each cap and abreast",
                     [plane()], [[capsule(0.125, 0.25)], [sphere(0.25)]],
                     np.stack([_pose(((0, 0, 0.75), QI), ((0.5, 0, 0.25), QI)), _pose(((0, 0, 0.75), QFLIP), ((0.5, 0, 0.25), QI)), _pose(((0, 0, 0.125), QX), ((0, 0.5, 0.25), QI)),
                               _pose(((0.25, 0, 0.25), QY), ((0.25, 1.0, 0.5), QI)), _pose(((1, 1, 0.375), QI), ((1, 1, 1.25), QI))]),
                     want=dict(pc_fb_y=1, pc_lying=1, touching=1, t_sides={-1, 0, 1})))
    out.append(Entry("exact-plane-y", "exact", "the same over a plane whose normal is y: |n[1]| > 0.5, the fallback takes b = z", [plane((0, -0.5, 0), QY)], [[capsule(0.125, 0.25)], [sphere(0.25)]],
                     np.stack([_pose(((0, 0.25, 0), QY), ((0.5, -0.25, 0.25), QI)), _pose(((0, 0.25, 0.5), QX), ((1, 0, 0), QI)), _pose(((0.5, -0.375, 0), QI), ((0, 0.5, 2), QI)),
                               _pose(((0, -0.125, 1), QY), ((0, 1, 1), QI)), _pose(((1, 0, 1), QX), ((1, 0.5, 1), QI))]),
                     want=dict(pc_fb_z=1, pc_lying=1, touching=1)))
    ax, bx, by = ((0, 0, 0.5), QX), lambda p: (p, QX), lambda p: (p, QY)
    arr = [bx((0, 0, 1.0)), bx((0.5, 0, 1.0)), bx((-0.5, 0, 1.0)), bx((2.0, 0, 1.0)), by((-0.5, 0.5, 0.5)), bx((1.5, 0, 0.5)), bx((-1.5, 0, 0.5)), by((1.0, 0, 0.5)), by((-1.0, 0, 0.5)),
           by((2.0, -2.0, 1.0)), by((-2.0, 2.0, 1.0))]
    poses = np.stack([_pose(ax, b) for b in arr])
    poses[2, :3] = (0.5, 0, 0.5)   # the partial overlap mirrored: the other capsule is the one that overhangs (d1 < d2)
    poses[2, 7:10] = (0, 0, 1.0)
    out.append(Entry("exact-capsules", "exact", "capsule-capsule axis-aligned: parallel with full, partial and no overlap, crossing at one point, end to end, end to middle, both clamped",
                     [], [[capsule(0.125, 0.5)], [capsule(0.125, 0.5)]], poses,
                     want=dict(coincident=1, clamps={"ota_side", "otb_side", "in1_side", "in2_side"}, picks={0, 1}, exact_tie=1)))
    return out


TABLE += _exact_entries()


# ---- either side of each switch, 5 % either way -----------------------------------------------------------------------------------------------------------------

def _side_entries():
    out = []
    c0 = np.array([0.2, 0.1, 0.8])
    out.append(Entry("side-frame", "side", "make_frame's |a[1]| < 0.5 switch: a[1] = +-0.45 and +-0.55 (and 0)", [], [[sphere(0.2)], [sphere(0.15)]],
                     np.stack([_pose((c0, QI), (c0 + 0.5 * np.array([np.sqrt(1 - a * a) * 0.6, a, np.sqrt(1 - a * a) * 0.8]), QI)) for a in (0.45, -0.45, 0.55, -0.55, 0.0)]),
                     want=dict(frame_y={0, 1}, frame_sw=0.0499)))
    for n1 in (0.45, 0.55):
        n = np.array([0.0, n1, np.sqrt(1 - n1 * n1)])
        u, w = np.array([1.0, 0, 0]), np.cross(n, [1.0, 0, 0])
        poses = []
        for deg, t in ((28, u), (32, u), (28, w), (32, -w), (32, -u)):
            axis = np.cos(np.radians(deg)) * n + np.sin(np.radians(deg)) * t
            poses.append(_pose((0.6 * n + 0.1 * u, quat_z_to(axis))))
        out.append(Entry(f"side-plane-capsule-n{int(100 * n1)}", "side", f"plane-capsule's bn < 0.5 fallback: the axis 28 and 32 degrees off a normal with n[1] = {n1}",
                         [plane((0, 0, 0), quat_z_to(n))], [[capsule(0.08, 0.2)]], np.stack(poses), want=dict(pc_fallback={0, 1}, pc_fb_y={int(n1 < 0.5)}, pc_bn=0.02, pc_n1=0.04)))
    # sphere-capsule: the sphere's foot on the segment at t = -0.05, 0.05, 0.95, 1.05 (and 0.5); the capsule lies along (0.6, 0, 0.8)
    axis, cpos, hl = np.array([0.6, 0.0, 0.8]), np.array([0.1, -0.2, 0.7]), 0.3
    a = cpos - hl * axis
    out.append(Entry("side-sphere-capsule", "side", "closest_segment_point's clamps: t just inside and just outside 0 and 1", [], [[sphere(0.1)], [capsule(0.07, hl)]],
                     np.stack([_pose((a + t * 2 * hl * axis + 0.3 * np.array([0, 1.0, 0]), QI), (cpos, quat_z_to(axis))) for t in (-0.05, 0.05, 0.95, 1.05, 0.5)]),
                     want=dict(t_sides={-1, 0, 1}, t=0.04)))
    # capsule-capsule: A along x (half-length 0.5), B along y (half-length 0.2) 0.25 above it: the feet of the common perpendicular 5 % inside / outside each end of A, then of B
    A = ((0, 0, 0.5), quat_z_to([1, 0, 0]))
    feet = [(s * 0.5 * f, 0.0) for s in (1, -1) for f in (0.95, 1.05)] + [(0.0, s * 0.2 * f) for s in (1, -1) for f in (0.95, 1.05)] + [(0.1, 0.05)]
    out.append(Entry("side-capsules", "side", "closest_segment_to_segment's four clamps: each line parameter just inside and just outside its end", [], [[capsule(0.1, 0.5)], [capsule(0.08, 0.2)]],
                     np.stack([_pose(A, ((x, -y, 0.75), quat_z_to([0, 1, 0]))) for x, y in feet]), want=dict(ota_sides={-1, 0, 1}, otb_sides={-1, 0, 1}, ota=0.02, otb=0.009)))
    return out


TABLE += _side_entries()


# ---- near-parallel capsules ---------------------------------------------------------------------------------------------------------------------------------------

def _nearpar(denom, dtypes):
    rng = np.random.RandomState(int(-np.log10(denom)))
    th = np.arcsin(np.sqrt(denom))
    poses = []
    for e in range(B):
        s = 1 if e % 2 == 0 else -1
        axis_b = np.array([np.cos(s * th), np.sin(s * th), 0.0])
        poses.append(_pose(((0, 0, 0.5), quat_z_to([1, 0, 0])), ((rng.uniform(-0.3, 0.3), rng.uniform(-0.05, 0.05), 0.5 + rng.uniform(0.25, 0.4)), quat_z_to(axis_b))))
    return Entry(f"near-parallel-{denom:g}", "nearpar", f"the 1e-6 regulariser of closest_segment_to_segment: denom about {denom:g}", [], [[capsule(0.1, 0.5)], [capsule(0.08, 0.4)]],
                 np.stack(poses), dtypes=dtypes, want=dict(denom=denom))


TABLE += [_nearpar(1e-2, (F64, F32)), _nearpar(1e-4, (F64,)), _nearpar(1e-8, (F64,))]


# ---- max_contact_points -------------------------------------------------------------------------------------------------------------------------------------------

def _topk_entries():
    many = drawn("topk-many", "max_contact_points: more candidates than lanes (71), the 24 closest kept", 3, 4, SCXX, _counts(1, 7), 64, kind="topk", max_contact_points=24,
                 want=dict(ncand_min=65, keep=24))
    # six spheres of one radius on one body, at three local heights (1, 3 and 2 of them): over a z-plane, the body upright, equal heights are bit-equal distances; the three
    # closest are kept, so the cut falls inside the tie of three.  Environments 0 and 3 have the same pose.
    body = [sphere(0.125, (x, y, z)) for x, y, z in ((0, 0, 0), (0.5, 0, 0.25), (0, 0.5, 0.25), (-0.5, 0, 0.25), (0, -0.5, 0.5), (0.5, 0.5, 0.5))]
    poses = np.stack([_pose((p, QI)) for p in ((0, 0, 0.25), (0.5, -1, 0.125), (-0.25, 0.75, 1.0), (0, 0, 0.25), (2, 2, 0.5))])
    ties = Entry("topk-ties", "topk", "max_contact_points: bit-equal distances, the cut in the middle of a tie of three; two environments with one pose", [plane()], [body], poses,
                 max_contact_points=3, want=dict(ncand=6, keep=3, tie_across_cut=True, same_envs=(0, 3)))
    plus1 = drawn("topk-plus-one", "max_contact_points: one candidate more than the cap", 0, 0, SCXX, _counts(3, 1), 91, kind="topk", max_contact_points=4, want=dict(ncand=5, keep=4))
    return [many, ties, plus1]


TABLE += _topk_entries()
BY_NAME = {e.name: e for e in TABLE}
assert len(BY_NAME) == len(TABLE)
CASES = [(e.name, dt) for e in TABLE for dt in e.dtypes]
CASE_IDS = [f"{n}-{'f64' if dt == F64 else 'f32'}" for n, dt in CASES]
INSTANTIATION_ENTRIES = ("n17-first", "n65-first", "mixed-pyramidal")


# ---- the conditions, from the tables and the margins ------------------------------------------------------------------------------------------------------------------

def conditions(name, xpos_xmat):
    """Asserts what ``Entry.want`` states, from ``mx.tables`` and the reference's margins on ``xpos_xmat`` (geom frames of the entry's poses, from whichever run).  Returns the
    reference evaluation."""
    e = BY_NAME[name]
    mx, _ = placed(name)
    T, w = mx.tables, e.want
    pairs = ref.pairs_of(T)
    fns = [p[0] for p in pairs]
    assert all(f < ref.FN_IN_KERNEL for f in fns), fns
    C = reference_of(mx, *xpos_xmat)
    M, S = C.margin, C.side
    if "npair" in w:
        assert len(pairs) == w["npair"], (name, len(pairs))
    if "npair_min" in w:
        assert len(pairs) >= w["npair_min"], (name, len(pairs))
    for p in w.get("pc", []):
        assert fns[p] == PC and pairs[p][1] == 2, (name, p, fns[p])
    for p in w.get("not_pc", []):
        assert fns[p] != PC and pairs[p][1] == 1, (name, p, fns[p])
    if e.kind == "random" and len(pairs) >= 15:
        assert set(fns) == set(range(5)), (name, sorted(set(fns)))  # all five pair functions
    if "condims" in w:
        assert set(int(x) for x in T.con_dim) == w["condims"] and not np.array_equal(T.contact_perm, np.arange(len(T.contact_perm))), (name, T.con_dim, T.contact_perm)
    if "sources" in w:
        assert {(c.ipair > -1, c.geomp > -1) for _, _, c, _ in T.pairs} == w["sources"], name
    if "ncand" in w or "ncand_min" in w:
        ncand, ncon = len(T.contact_perm), mx.constraint_sizes_py[3]
        assert T.topk and ncon == w["keep"] and (ncand == w["ncand"] if "ncand" in w else ncand >= w["ncand_min"]), (name, ncand, ncon)
    if w.get("tie_across_cut"):
        srt = np.sort(C.dist, axis=1)
        k = w["keep"]
        assert (srt[:, k - 1] == srt[:, k]).all() and (srt[:, k - 2] == srt[:, k - 1]).all() and (srt[:, k - 3] < srt[:, k - 2]).all(), name
    if "same_envs" in w:
        i, j = w["same_envs"]
        assert np.array_equal(e.poses[i], e.poses[j])
    if "coincident" in w:
        assert S["coincident"].sum() >= w["coincident"], name
    if "axis_normals" in w:
        n = C.frame[:, :, 0].astype(np.float64)
        axis = (np.abs(n) == 1).sum(-1) == 1
        assert axis.sum() >= w["axis_normals"] and {tuple(v) for v in n[axis & ~S["coincident"].astype(bool)].reshape(-1, 3)} == {(s * (i == 0), s * (i == 1), s * (i == 2)) for i in range(3) for s in (1.0, -1.0)}, name
    if "pc_fb_y" in w and isinstance(w["pc_fb_y"], int) and e.kind == "exact":
        assert (S["pc_fallback"] & S["pc_fb_y"]).sum() >= 1, name
    if "pc_fb_z" in w:
        assert (S["pc_fallback"] & ~S["pc_fb_y"].astype(bool) & (C.fn == PC)).sum() >= 1, name
    if "pc_lying" in w:
        assert ((C.fn == PC) & (np.abs(M["pc_bn"] - 0.5) < 1e-15)).sum() >= 1, name  # bn == 1
    if "touching" in w:
        assert (C.dist == 0).sum() >= 1, name
    if "t_sides" in w:
        assert set(np.unique(S["t_side"][:, C.fn == ref.FN_SPHERE_CAPSULE])) == w["t_sides"], name
    if "clamps" in w:
        cc = C.fn == ref.FN_CAPSULE_CAPSULE
        for k in w["clamps"]:  # the eight clamp outcomes: each of the four parameters below and above its range
            assert {-1, 1} <= set(np.unique(S[k][:, cc])), (name, k, np.unique(S[k][:, cc]))
        assert set(np.unique(S["pick"][:, cc])) == w["picks"], name
        assert C.exact_tie.sum() >= w["exact_tie"], name
    if e.kind == "side":
        for k in ("frame_sw", "pc_bn", "pc_n1", "t", "ota", "otb"):
            if k in w:
                m = M[k][~np.isnan(M[k])]
                assert m.size and m.min() >= w[k], (name, k, m.min())
        for k, sk in (("frame_y", "frame_y"), ("pc_fallback", "pc_fallback"), ("ota_sides", "ota_side"), ("otb_sides", "otb_side")):
            if k in w:
                assert set(np.unique(S[sk])) == w[k], (name, k, np.unique(S[sk]))
        if "pc_fb_y" in w:
            assert set(np.unique(S["pc_fb_y"][S["pc_fallback"].astype(bool)])) == w["pc_fb_y"], name
    if "denom" in w:
        dn = M["denom"][~np.isnan(M["denom"])]
        assert (dn > 0.5 * w["denom"]).all() and (dn < 2 * w["denom"]).all(), (name, dn)
    return C


# ---- the rules, on the leaves of any run ({abi leaf: numpy}, batched) ---------------------------------------------------------------------------------------------------

CC = ref.FN_CAPSULE_CAPSULE
LEAVES = ("dist", "pos", "normal", "frame")
CONST_REALS = ("includemargin", "friction", "solref", "solreffriction", "solimp")
CONST_INTS = ("dim", "geom1", "geom2", "geom", "efc_address")


def f64(x):
    return np.asarray(x, dtype=np.float64)


def contact_leaves(out, nb, n):
    fr = np.asarray(out["contact_frame"]).reshape(nb, n, 3, 3)
    return dict(dist=np.asarray(out["contact_dist"]).reshape(nb, n), pos=np.asarray(out["contact_pos"]).reshape(nb, n, 3), normal=fr[:, :, 0], frame=fr)


def _as_leaves(C):
    return dict(dist=C.dist, pos=C.pos, normal=C.frame[:, :, 0], frame=C.frame)


def check_values(name, dtype, mx, out, log=print):
    """``contact_dist / pos / frame`` of a run against ``_prim_ref`` on that run's own ``geom_xpos`` / ``geom_xmat``: the comparable rows of every leaf at ``TOL_PRE[dtype]`` by
    ``_util.rel_err`` (``_prim_ref.Contacts.against``: a near-tie of the d1 < d2 pick is held to the nearer of the two picks); capsule-capsule contacts with ``denom < 1e-2`` at max(TOL_PRE, 4 x the error of the same-dtype numpy evaluation), ``dist`` alone where ``denom < 1e-6``.
    Entries of exact arrangements and of the either-side kind leave nothing out, a drawn one at most 1 %.  -> (reference, {(pair function, leaf): error / bound}, rows left out per leaf)."""
    from _cases import TOL_PRE
    from _util import rel_err

    e = BY_NAME[name]
    tol, eps = TOL_PRE[dtype], float(torch.finfo(dtype).eps)
    C = reference_of(mx, out["geom_xpos"], out["geom_xmat"])
    same = _as_leaves(same_dtype_of(mx, out["geom_xpos"], out["geom_xmat"], dtype))
    got = contact_leaves(out, e.B, slots(mx))
    want, keep = C.against(got["pos"], eps)
    strict = C.comparable(eps)
    assert (C.fn >= 0).all()  # every slot belongs to an in-kernel pair
    denom = C.margin["denom"]
    ill = (C.fn == CC)[None] & (denom < 1e-2)
    vague = ill & (denom < 1e-6)
    share = {}
    floor = (1e-3,) if dtype == F32 else ()  # (_util.rel_err's own floor for float32 leaves; the reference values arrive here as float64)
    for leaf in LEAVES:
        assert np.isfinite(got[leaf]).all(), (name, leaf)
        for fn in range(ref.FN_IN_KERNEL):  # reported, not asserted: the same figure per pair function
            rows = keep[leaf] & ~ill & (C.fn == fn)[None]
            if rows.any():
                share[(ref.FN_NAMES[fn], leaf)] = rel_err(got[leaf][rows], f64(want[leaf][rows]), *floor) / tol
        rows = keep[leaf] & ~ill
        if rows.any():
            err = rel_err(got[leaf][rows], f64(want[leaf][rows]), *floor)
            log(f"  {leaf}: rel_err {err:.3g} over {int(rows.sum())} contacts ({err / tol:.2g} of {tol:g})")
            assert err <= tol, (name, leaf, err, tol)
        rows = keep[leaf] & ill & (np.ones_like(vague) if leaf == "dist" else ~vague)
        if rows.any():
            e_same, err = rel_err(f64(same[leaf][rows]), f64(want[leaf][rows]), *floor), rel_err(got[leaf][rows], f64(want[leaf][rows]), *floor)
            bound = max(tol, 4 * e_same)
            log(f"  {leaf}, denom < 1e-2: rel_err {err:.3g}, numpy in the dtype {e_same:.3g}, bound {bound:.3g} ({err / bound:.2g} of it)")
            assert err <= bound, (name, leaf, err, bound)
            share[("capsule_capsule, denom < 1e-2", leaf)] = err / bound
    left = {leaf: int((~keep[leaf]).sum()) for leaf in LEAVES}
    log(f"  left out of {keep['pos'].size}: {left}; held to either d1 < d2 pick: {int((keep['pos'] & ~strict['pos']).sum())}")
    if e.kind in ("exact", "side"):
        assert not any(left.values()), (name, left)
    elif e.kind != "nearpar":
        assert max(left.values()) <= 0.01 * keep["pos"].size, (name, left)
    if e.kind == "exact" and dtype == F64:  # frames of axis-aligned normals: exactly the expected 0 / +-1 entries
        rows = ((np.abs(C.frame) == 1) | (C.frame == 0)).all((-1, -2))
        assert rows.sum() >= e.B // 2 and np.array_equal(got["frame"][rows], f64(C.frame[rows])), name
    return C, share, left


def check_properties(dtype, got, C):
    """No tolerance beyond 64 eps, on every contact: |frame[0]| = 1 (except where make_frame was given a zero vector), the rows mutually orthogonal (except plane-capsule's
    fallback, whose b is not orthogonalised), everything finite."""
    tol = 64 * float(torch.finfo(dtype).eps)
    fr = f64(got["frame"])
    assert np.isfinite(fr).all() and np.isfinite(got["dist"]).all() and np.isfinite(got["pos"]).all()
    n, b, c = fr[:, :, 0], fr[:, :, 1], fr[:, :, 2]
    unit = (C.fn == PC)[None] | C.side["any_a"].astype(bool)
    assert unit.all()  # (no pair of the family hands make_frame a zero vector: a coincident pair gets x)
    assert (np.abs(np.linalg.norm(n, axis=-1) - 1)[unit] <= tol).all()
    ortho = ~C.side["pc_fallback"].astype(bool)
    for u, v in ((n, b), (n, c), (b, c)):
        assert (np.abs((u * v).sum(-1))[ortho] <= tol).all()


def expected_constants(mx, dtype):
    """The model-constant contact leaves per slot, from ``collision_tables.static_contact_params`` through ``pair_dst`` (models without max_contact_points)."""
    from mujoco_torch_amd import collision_tables as ct
    from mujoco_torch_amd.io import model_float_leaves

    T = mx.tables
    n = slots(mx)
    per_pair = ct.static_contact_params(model_float_leaves(mx, dtype), T.pairs, dtype)
    want = dict(includemargin=torch.zeros(n, dtype=dtype), friction=torch.zeros(n, 5, dtype=dtype), solref=torch.zeros(n, 2, dtype=dtype),
                solreffriction=torch.zeros(n, 2, dtype=dtype), solimp=torch.zeros(n, 5, dtype=dtype), dim=torch.zeros(n, dtype=torch.int32),
                geom1=torch.zeros(n, dtype=torch.int32), geom2=torch.zeros(n, dtype=torch.int32))
    for p, (fn, k, c, _) in enumerate(T.pairs):
        for q in range(k):
            s = int(T.pair_dst[p][q])
            want["friction"][s], want["solref"][s], want["solreffriction"][s], want["solimp"][s], want["includemargin"][s] = per_pair[p]
            want["dim"][s], want["geom1"][s], want["geom2"][s] = c.dim, c.geom1, c.geom2
    want["geom"] = torch.stack([want["geom1"], want["geom2"]], -1)
    elliptic = int(mx.opt.cone) == 1
    rows = torch.tensor([1 if d == 1 else (d if elliptic else 2 * (d - 1)) for d in want["dim"].tolist()], dtype=torch.int64)
    ne, nf, nl = mx.constraint_sizes_py[:3]
    want["efc_address"] = (ne + nf + nl + torch.cumsum(rows, 0) - rows).to(torch.int32)
    return want


def check_constants(dtype, mx, out, nb, skip=()):
    """Integers equal, reals ``torch.equal`` in the dtype, in every environment."""
    want = expected_constants(mx, dtype)
    for k in CONST_REALS + CONST_INTS:
        if k in skip:
            continue
        got = torch.as_tensor(np.asarray(out["contact_" + k])).reshape((nb,) + tuple(want[k].shape))
        assert got.dtype == want[k].dtype or not got.is_floating_point(), (k, got.dtype)
        assert torch.equal(got.to(want[k].dtype), want[k].expand(got.shape).contiguous()), k


def check_topk(name, dtype, mx, out, twin_mx, twin_out, log=print):
    """max_contact_points against the uncapped twin, whose contacts are the candidates: the kept distances are the ``ncon`` smallest as a multiset, bit for bit; each kept
    contact's pos, frame, geom ids and constants belong to ONE candidate with that distance; no candidate is kept twice; environments with one pose give one result.  And
    against ``_prim_ref``: the sorted kept distances at TOL_PRE.  Which of two tied candidates survives is not asserted."""
    from _cases import TOL_PRE
    from _util import rel_err

    e = BY_NAME[name]
    ncon, ncand = mx.constraint_sizes_py[3], slots(mx)
    assert slots(twin_mx) == ncand and twin_mx.constraint_sizes_py[3] == ncand and not twin_mx.tables.topk
    names = ("contact_dist", "contact_pos", "contact_frame", "contact_geom1", "contact_geom2", "contact_dim") + tuple("contact_" + k for k in CONST_REALS)
    kept = {k: np.asarray(out[k]).reshape(e.B, ncon, -1) for k in names}
    cand = {k: np.asarray(twin_out[k]).reshape(e.B, ncand, -1) for k in names}
    assert kept["contact_dist"].dtype == cand["contact_dist"].dtype == NPDT[dtype]
    assert np.array_equal(np.sort(kept["contact_dist"][:, :, 0], 1), np.sort(cand["contact_dist"][:, :, 0], 1)[:, :ncon]), name
    for env in range(e.B):
        used = set()
        for c in range(ncon):
            hit = [q for q in range(ncand) if q not in used and all(np.array_equal(kept[k][env, c], cand[k][env, q]) for k in names)]
            assert hit, (name, env, c)
            used.add(hit[0])
    if "same_envs" in e.want:
        i, j = e.want["same_envs"]
        for k in names:
            assert np.array_equal(kept[k][i], kept[k][j]), (name, k)
    C = reference_of(mx, out["geom_xpos"], out["geom_xmat"])
    err = rel_err(np.sort(kept["contact_dist"][:, :, 0], 1), f64(ref.topk_smallest(C.dist, ncon)))
    log(f"  kept distances against the reference's {ncon} smallest of {ncand}: rel_err {err:.3g} ({err / TOL_PRE[dtype]:.2g} of {TOL_PRE[dtype]:g})")
    assert err <= TOL_PRE[dtype]
    return err / TOL_PRE[dtype]
