"""Models of chosen sizes and leaves of chosen values for the constraint-space, PGS and no-slip kernels (tests/test_constraint_shapes.py and its host companion).

``family`` writes the text of a member of tools/gen_big_models.py's family -- a hub over a floor, legs that are chains of hinges, ``jacobian="dense"``, chosen links
limited, every tip colliding with the floor at condim 3 -- in the test process and compiles it with ``mt.mjcf.from_xml_string``: nothing is committed, and the sizes
(nv, ne, nf, nl, ncon, nefc) are the caller's choice.  With the default ``limited=(0, 6)`` a pyramidal leg gives 9 rows (1 limit, two capsule-plane contacts of 4
edges), 10 with seven or more links; an elliptic leg 7 or 8.

``leaves`` fills a ``make_data`` batch with seeded synthetic leaves, created in float64 and rounded to the dtype: no ``forward`` runs, the functions under test
read leaves and nothing else.  ``TABLE`` is the one table of cases both test files walk.
"""
import functools
import math
from typing import NamedTuple

import numpy as np
import torch

import _efc_ref as er
import _noslip_ref as nr
import _pgs_ref as pr
import mujoco_torch_amd as mt

F64, F32 = torch.float64, torch.float32
LD = er.LD
NPDT = {F64: np.float64, F32: np.float32}
SYNTH_LEAVES = ("efc_J", "efc_D", "efc_aref", "efc_frictionloss", "qM", "qLD", "qfrc_smooth", "qacc_smooth", "qacc")


def _leg(k, nleg, links, limited, nfric_left):
    a = 2 * math.pi * k / nleg
    out = [f'<body name="l{k}_0" pos="{0.12 * math.cos(a):.5f} {0.12 * math.sin(a):.5f} 0" euler="0 0 {math.degrees(a):.4f}">']
    for i in range(links):
        if i > 0:
            out.append(f'<body name="l{k}_{i}" pos="0.1 0 0">')
        axis = "0 1 0" if i % 2 == 0 else "0 0 1"
        lim = ' limited="true" range="-40 55"' if i in limited else ""
        fric = ' frictionloss="0.4"' if i < nfric_left else ""
        out.append(f'<joint name="j{k}_{i}" type="hinge" axis="{axis}"{lim}{fric}/>')
        tip = ' contype="1" conaffinity="0" condim="3"' if i == links - 1 else ""
        out.append(f'<geom name="g{k}_{i}" type="capsule" fromto="0 0 0 0.1 0 0" size="0.02"{tip}/>')
    return out + ["</body>"] * links


def family_xml(legs, *, nfric=0, neq=0, limited=(0, 6)):
    """The MJCF text.  ``nfric``: ``frictionloss`` on the first ``nfric`` joints, in dof order; ``neq``: joint equalities between the first joints of legs k and
    k + 1, k < neq; ``limited``: the links of every leg whose joint is limited."""
    assert 0 <= nfric <= sum(legs) and 0 <= neq < max(len(legs), 1)
    out = ['<mujoco model="efc_synth">', '<option timestep="0.002" jacobian="dense" solver="CG" iterations="50" tolerance="1e-10"><flag eulerdamp="disable"/></option>',
           '<default><joint damping="0.2" armature="0.01"/><geom contype="0" conaffinity="0" density="500"/></default>', "<worldbody>",
           '<geom name="floor" type="plane" size="5 5 0.1" contype="0" conaffinity="1" condim="3"/>', '<body name="hub" pos="0 0 0.3">',
           '<geom name="hub" type="sphere" size="0.12"/>']
    left = nfric
    for k, n in enumerate(legs):
        out += _leg(k, len(legs), n, limited, left)
        left = max(0, left - n)
    out += ["</body>", "</worldbody>"]
    if neq:
        out += ["<equality>"] + [f'<joint name="e{k}" joint1="j{k}_0" joint2="j{k + 1}_0" polycoef="0 1"/>' for k in range(neq)] + ["</equality>"]
    return "\n".join(out + ["</mujoco>", ""])


def family(legs, *, cone=0, contacts=True, nfric=0, neq=0, limited=(0, 6), dtype=F64):
    """The Model (host) of the family member: nv = sum(legs).  ``cone``: 0 pyramidal, 1 elliptic; ``contacts=False`` sets ``DisableBit.CONTACT``."""
    lite = mt.mjcf.from_xml_string(family_xml(legs, nfric=nfric, neq=neq, limited=limited))
    lite.opt.cone = int(cone)
    if not contacts:
        lite.opt.disableflags = int(lite.opt.disableflags) | int(mt.DisableBit.CONTACT)
    return mt.device_put(lite, dtype=None if dtype == F64 else dtype)


def sizes(m):
    """(nv, ne, nf, nl, ncon, nefc)."""
    ne, nf, nl, ncon, nefc = (int(x) for x in m.constraint_sizes_py)
    return int(m.nv), ne, nf, nl, ncon, nefc


def inertia_scale(m):
    return float(m.stat.meaninertia) * max(1, int(m.nv))


def cholesky_lower(M):
    """The lower Cholesky factor of M [B, n, n] in longdouble."""
    M = er.ld(M)
    n = M.shape[-1]
    L = np.zeros_like(M)
    for j in range(n):
        L[:, j, j] = np.sqrt(M[:, j, j] - (L[:, j, :j] ** 2).sum(-1))
        for i in range(j + 1, n):
            L[:, i, j] = (M[:, i, j] - (L[:, i, :j] * L[:, j, :j]).sum(-1)) / L[:, j, j]
    return L


def synth_arrays(nv, ne, nf, nefc, B, dtype, seed):
    """{leaf: [B, ...] numpy array in the dtype}: the issue's recipe.  ``qM = A A^T / nv + I`` (A standard normal), rounded; ``qLD`` the lower Cholesky factor of
    that rounded ``qM`` in longdouble, rounded (zeros above the diagonal); ``efc_J`` standard normal with about a quarter of the rows past ``ne + nf`` exact zeros
    whose ``aref`` is 0 (inactive contacts), chosen per environment; ``efc_D`` log-uniform in [0.5, 50]; ``efc_frictionloss`` uniform in [0.1, 2] on the friction
    rows, 0 elsewhere; ``aref``, ``qfrc_smooth``, ``qacc_smooth``, ``qacc`` standard normal."""
    rng = np.random.RandomState(seed)
    dt = NPDT[dtype]
    A = rng.randn(B, nv, nv)
    qM = (np.einsum("bik,bjk->bij", A, A) / nv + np.eye(nv)).astype(dt)
    qM = np.maximum(qM, qM.transpose(0, 2, 1))  # (symmetric bit for bit after the rounding: a max of two roundings of the same sums)
    qLD = np.asarray(cholesky_lower(qM), dtype=dt)
    J = rng.randn(B, nefc, nv)
    aref = rng.randn(B, nefc)
    dead = rng.rand(B, nefc) < 0.25
    dead[:, :ne + nf] = False
    J[dead] = 0
    aref[dead] = 0
    D = 0.5 * 100.0 ** rng.rand(B, nefc)
    fl = np.zeros((B, nefc))
    fl[:, ne:ne + nf] = rng.uniform(0.1, 2.0, (B, nf))
    out = dict(efc_J=J, efc_D=D, efc_aref=aref, efc_frictionloss=fl, qM=qM, qLD=qLD, qfrc_smooth=rng.randn(B, nv), qacc_smooth=rng.randn(B, nv),
               qacc=rng.randn(B, nv))
    return {n: np.ascontiguousarray(v.astype(dt)) for n, v in out.items()}


def leaves(m, B, dtype, seed):
    """A Data of batch B from ``mt.make_data(m)`` whose SYNTH_LEAVES are ``synth_arrays`` of the Model's sizes (host tensors in the dtype)."""
    nv, ne, nf, _, _, nefc = sizes(m)
    d = mt.make_data(m).expand(B).clone()
    if dtype != F64:
        d = d.to(dtype)
    return d.replace(**{n: torch.from_numpy(v) for n, v in synth_arrays(nv, ne, nf, nefc, B, dtype, seed).items()})


def arrays_of(m, d):
    """The SYNTH_LEAVES of a Data as host arrays [B, ...] (matrices unflattened)."""
    nv, _, _, _, _, nefc = sizes(m)
    B = d.efc_D.shape[0]
    tail = dict(efc_J=(nefc, nv), qM=(nv, nv), qLD=(nv, nv))
    return {n: getattr(d, n).detach().cpu().numpy().reshape((B,) + tail.get(n, (-1,))) for n in SYNTH_LEAVES}


class Case(NamedTuple):
    name: str
    legs: tuple
    dtype: torch.dtype
    opts: tuple = ()        # family's keywords, as sorted items
    want: tuple = ()        # (nv, ne, nf, nl, ncon, nefc): pinned by the host test
    stage: tuple = ()       # the rows of every staging step the plans must report, () where the table sets no condition
    elliptic: bool = False  # solve_noslip runs on the elliptic twin too
    seed: int = 1

    def model(self, cone=0):
        return _model(self.legs, self.dtype, self.opts, cone)

    @property
    def contacts(self):
        return dict(self.opts).get("contacts", True)


_MODELS = {}


def _model(legs, dtype, opts, cone):
    key = (legs, dtype, opts, cone)
    if key not in _MODELS:
        _MODELS[key] = family(list(legs), cone=cone, dtype=dtype, **dict(opts))
    return _MODELS[key]


def _c(name, legs, dtype, want, stage=(), elliptic=False, seed=1, **opts):
    return Case(name, tuple(legs), dtype, tuple(sorted(opts.items())), tuple(want), tuple(stage), elliptic, seed)


B = 3
MIXED12 = dict(neq=2, nfric=5)
MIXED33 = dict(neq=3, nfric=7)
TABLE = [
    # the dof counts, float64: every P of efc_jt_accumulate (1 .. 32) with nv == P and nv < P, one lane per dof with fewer dofs than lanes, 64 and 65
    _c("nv1", [1], F64, (1, 0, 0, 1, 2, 9)),
    _c("nv2", [2], F64, (2, 0, 0, 1, 2, 9)),
    _c("nv3", [3], F64, (3, 0, 0, 1, 2, 9)),
    _c("nv4", [2, 2], F64, (4, 0, 0, 2, 4, 18)),
    _c("nv5", [5], F64, (5, 0, 0, 1, 2, 9), elliptic=True),
    _c("nv8", [4, 4], F64, (8, 0, 0, 2, 4, 18)),
    _c("nv16", [8, 8], F64, (16, 0, 0, 4, 4, 20)),
    _c("nv17", [8, 9], F64, (17, 0, 0, 4, 4, 20)),
    _c("nv31", [2] * 15 + [1], F64, (31, 0, 0, 16, 32, 144), (66, 66, 12)),
    _c("nv32", [2] * 16, F64, (32, 0, 0, 16, 32, 144), (62, 62, 20), elliptic=True),
    _c("nv33", [2] * 15 + [3], F64, (33, 0, 0, 16, 32, 144), (62, 62, 20), elliptic=True),
    _c("nv63-whole-chunks", [6] * 6 + [27], F64, (63, 0, 0, 8, 14, 64), (32, 32)),
    _c("nv64", [8] * 8, F64, (64, 0, 0, 16, 16, 80), (31, 31, 18), elliptic=True),
    _c("nv65", [7] * 9 + [2], F64, (65, 0, 0, 19, 20, 99), (31, 31, 31, 6), elliptic=True),
    # float32
    _c("nv8-f32", [4, 4], F32, (8, 0, 0, 2, 4, 18)),
    _c("nv32-f32", [2] * 16, F32, (32, 0, 0, 16, 32, 144), (124, 20)),
    _c("nv33-f32", [2] * 15 + [3], F32, (33, 0, 0, 16, 32, 144), (124, 20)),
    _c("nv63-f32", [7] * 9, F32, (63, 0, 0, 18, 18, 90), (65, 25)),
    _c("nv64-f32", [8] * 8, F32, (64, 0, 0, 16, 16, 80), (63, 17)),
    _c("nv65-f32-last-one", [6] * 6 + [29], F32, (65, 0, 0, 8, 14, 64), (63, 1)),
    # limit rows alone, around AR's 8 x 8 tile
    _c("rows1", [1], F64, (1, 0, 0, 1, 0, 1), contacts=False),
    _c("rows1-nv3", [3], F64, (3, 0, 0, 1, 0, 1), contacts=False),
    _c("rows7", [1] * 7, F64, (7, 0, 0, 7, 0, 7), contacts=False),
    _c("rows8", [1] * 8, F64, (8, 0, 0, 8, 0, 8), contacts=False),
    _c("rows9", [1] * 9, F64, (9, 0, 0, 9, 0, 9), contacts=False),
    # equality, friction-loss, limit and contact rows at once: both row-class boundaries inside the matrix
    _c("mixed12", [5, 4, 3], F64, (12, 2, 5, 3, 6, 34), **MIXED12),
    _c("mixed12-f32", [5, 4, 3], F32, (12, 2, 5, 3, 6, 34), **MIXED12),
    _c("mixed33", [2] * 15 + [3], F64, (33, 3, 7, 16, 32, 154), (62, 62, 30), elliptic=True, **MIXED33),
]
BY_NAME = {c.name: c for c in TABLE}
BIT_CASES = ("nv33", "nv64", "nv65", "nv33-f32", "nv64-f32", "nv65-f32-last-one")


# ---- the problems and their references (host, computed once and shared) ---------------------------------------------------------------------------

K = 3           # vectors of a mul_jac_vec / mul_jac_t_vec call
SWEEPS = (1, 3)
STATE_CAP = 0.01


@functools.lru_cache(maxsize=None)
def problem(name, cone=0):
    """(host Model, host Data of batch B, its SYNTH_LEAVES as arrays, queries) of a table entry; ``cone=1``: its elliptic twin (other row counts: other leaves)."""
    c = BY_NAME[name]
    m = c.model(cone)
    d = leaves(m, B, c.dtype, c.seed + 100 * cone)
    nv, _, _, _, _, nefc = sizes(m)
    rng = np.random.RandomState(11)
    dt = NPDT[c.dtype]
    q = dict(v=rng.randn(B, K, nv).astype(dt), f=rng.randn(B, K, nefc).astype(dt), jar=rng.randn(B, nefc).astype(dt), pgs0=(2 * rng.randn(B, nefc)).astype(dt))
    return m, d, arrays_of(m, d), q


def floss_of(m):
    return sizes(m)[2] > 0 and not (int(m.opt.disableflags) & int(mt.DisableBit.FRICTIONLOSS))


def ref_update(m, A, qacc=None, jar=None):
    _, ne, nf, _, _, _ = sizes(m)
    return er.constraint_update(A["efc_J"], A["efc_D"], A["efc_aref"], A["efc_frictionloss"], ne + nf, floss_of(m), qacc=qacc, jar=jar, qM=A["qM"],
                                qfrc_smooth=A["qfrc_smooth"], qacc_smooth=A["qacc_smooth"], inertia_scale=inertia_scale(m))


def state_keep(m, A, eps, qacc=None, jar=None):
    """The rows whose state is compared (``_efc_ref.comparable``).  In the ``jar=`` form ``jar`` itself carries no rounding: what is left of the bound is the two
    roundings of a friction row's boundary ``r fl`` (``state_margin`` with ``J = 0`` and ``aref = -jar``, less the ulp of that ``aref``)."""
    _, ne, nf, _, _, _ = sizes(m)
    if jar is None:
        dist, bound = er.state_margin(A["efc_J"], qacc, A["efc_aref"], A["efc_D"], A["efc_frictionloss"], ne + nf, floss_of(m), eps)
    else:
        dist, bound = er.state_margin(np.zeros_like(A["efc_J"]), np.zeros_like(A["qacc"]), -er.ld(jar), A["efc_D"], A["efc_frictionloss"], ne + nf, floss_of(m), eps)
        bound = bound - LD(eps) * np.abs(er.ld(jar))
    return er.comparable(dist, bound)


def ref_pgs(m, A, force0, sweeps=max(SWEEPS), dtype=LD):
    _, ne, nf, _, _, _ = sizes(m)
    return pr.solve_pgs(A["efc_J"], A["efc_D"], A["efc_aref"], A["efc_frictionloss"], A["qLD"], A["qacc_smooth"], ne, nf, inertia_scale(m), sweeps, force0=force0,
                        dtype=dtype)


def pgs_at(A, ref, k, dtype=LD):
    qfrc, qacc = pr.finish(A["efc_J"], A["qLD"], A["qacc_smooth"], ref["forces"][k], dtype)
    imp = ref["improvements"][k - 1] if k else np.zeros(len(qfrc))
    return dict(efc_force=ref["forces"][k], qfrc_constraint=qfrc, qacc=qacc, cost=ref["costs"][k], improvement=imp)


def con_of(m):
    _, _, _, _, ncon, _ = sizes(m)
    return nr.contacts(np.asarray(m.tables.con_dim)[:ncon], m.tables.con_efc_address, ncon)


def noslip_friction(m, dtype, seed=7):
    """``contact.friction`` [B, ncon, 5] as tests/test_noslip.py sets it: the pass's leaf (here ``make_data``'s) edited afterwards -- every third environment keeps the
    model's coefficients, the others get sliding coefficients between 0.3 and 1.5, per contact and direction."""
    _, _, _, _, ncon, _ = sizes(m)
    fr = mt.make_data(m).contact.friction.detach().cpu().numpy().astype(np.float64).reshape(1, ncon, 5).repeat(B, 0)
    rng = np.random.RandomState(seed)
    new = rng.uniform(0.3, 1.5, (B, ncon, 2))
    e = np.arange(B) % 3 != 0
    fr[e, :, :2] = new[e]
    return fr.astype(NPDT[dtype])


def touched_rows(m):
    """The rows a no-slip sweep may change: friction-loss rows, the rows of pyramidal contacts of condim > 1, the friction rows of elliptic ones."""
    _, ne, nf, _, _, nefc = sizes(m)
    t = np.zeros(nefc, dtype=bool)
    t[ne:ne + nf] = True
    for adr, dim in con_of(m):
        if int(m.opt.cone) == 1:
            t[adr + 1:adr + dim] = True
        else:
            t[adr:adr + 2 * (dim - 1)] = True
    return t


def noslip_start(m, dtype, seed=5):
    """A random start of unit size: both signs on the equality and friction-loss rows and on the friction rows of elliptic contacts, positive on every other row
    (limit rows, normals, pyramid edges), so that every block is live."""
    _, ne, nf, _, _, nefc = sizes(m)
    f0 = np.random.RandomState(seed).randn(B, nefc)
    signed = np.zeros(nefc, dtype=bool)
    signed[:ne + nf] = True
    if int(m.opt.cone) == 1:
        for adr, dim in con_of(m):
            signed[adr + 1:adr + dim] = True
    f0[:, ~signed] = np.abs(f0[:, ~signed])
    return f0.astype(NPDT[dtype])


def ref_noslip(m, A, start, mu, sweeps=max(SWEEPS), dtype=LD):
    _, ne, nf, _, _, _ = sizes(m)
    return nr.solve_noslip(A["efc_J"], A["efc_D"], A["efc_aref"], A["efc_frictionloss"], A["qLD"], A["qacc_smooth"], start, mu, ne, nf, con_of(m),
                           int(m.opt.cone) == 1, inertia_scale(m), sweeps, tolerance=-np.inf, dtype=dtype)


def noslip_at(A, ref, niter, dtype=LD):
    """The reference's outputs with environment e taken after ``niter[e]`` sweeps."""
    e = np.arange(len(niter))
    f = ref["forces"][niter, e]
    qfrc, qacc = pr.finish(A["efc_J"], A["qLD"], A["qacc_smooth"], f, dtype)
    imp = np.where(niter > 0, ref["improvements"][np.maximum(niter, 1) - 1, e], 0)
    return dict(efc_force=f, qfrc_constraint=qfrc, qacc=qacc, cost=ref["costs"][niter, e], improvement=imp)


@functools.lru_cache(maxsize=None)
def pgs_refs(name, warm):
    """(longdouble, same dtype) references of max(SWEEPS) PGS sweeps of a table entry, cold or from the infeasible start ``pgs0``."""
    m, _, A, q = problem(name)
    start = q["pgs0"] if warm else None
    return ref_pgs(m, A, start), ref_pgs(m, A, start, dtype=NPDT[BY_NAME[name].dtype])


@functools.lru_cache(maxsize=None)
def noslip_refs(name, cone):
    """(start, friction, longdouble reference, same-dtype reference) of max(SWEEPS) no-slip sweeps of a table entry."""
    m, _, A, _ = problem(name, cone)
    dtype = BY_NAME[name].dtype
    start, mu = noslip_start(m, dtype), noslip_friction(m, dtype)
    return start, mu, ref_noslip(m, A, start, mu), ref_noslip(m, A, start, mu, dtype=NPDT[dtype])


def noslip_cases():
    """[(name, cone)]: every entry with contacts under the pyramidal cone, the ``elliptic`` ones under the elliptic cone as well."""
    return [(c.name, 0) for c in TABLE if c.contacts] + [(c.name, 1) for c in TABLE if c.elliptic]


# ---- the table's conditions ---------------------------------------------------------------------------------------------------------------------

def plans(c, cone=0):
    """{what: (chunk, nchunk, last, lds)} of the six plans of an entry, from the library."""
    from mujoco_torch_amd import constraint_space as cs, noslip, pgs
    nv, _, _, _, ncon, nefc = sizes(c.model(cone))
    out = {op: cs.plan(op, nv, nefc, c.dtype) for op in (cs.MUL_J, cs.MUL_JT, cs.UPDATE, cs.AR)}
    out["pgs"] = pgs.plan(nv, nefc, c.dtype)
    out["noslip"] = noslip.plan(nv, nefc, ncon, c.dtype)
    return out


def staged(plan):
    chunk, nchunk, last, _ = plan
    return (chunk,) * (nchunk - 1) + (last,)


def table_conditions():
    """Asserts what the issue asks of the table, from the library's own plans; returns a summary for the log."""
    from mujoco_torch_amd import constraint_space as cs
    size = {F64: 8, F32: 4}
    got = {c.name: (sizes(c.model()), plans(c)) for c in TABLE}
    for c in TABLE:
        s, p = got[c.name]
        assert s == c.want, (c.name, s)
        for what, pl in p.items():
            if c.stage:
                assert staged(pl) == c.stage, (c.name, what, pl)
            assert sum(staged(pl)) == s[5] and pl[3] <= 160 * 1024, (c.name, what, pl)
    with_rows = [c for c in TABLE if c.contacts]
    for dtype, dofs in ((F64, (1, 2, 3, 4, 5, 8, 16, 17, 31, 32, 33, 63, 64, 65)), (F32, (8, 32, 33, 64, 65))):
        have = {c.want[0] for c in with_rows if c.dtype == dtype and c.want[3] >= 1 and c.want[4] >= 1}
        assert set(dofs) <= have, (dtype, sorted(set(dofs) - have))
    st = {c.name: staged(got[c.name][1][cs.AR]) for c in TABLE}
    assert st["nv31"] == (66, 66, 12) and BY_NAME["nv31"].dtype == F64                      # a chunk of 66 rows, three chunks
    assert st["nv63-f32"] == (65, 25) and st["nv64-f32"] == (63, 17)                        # chunks of 65 and of 63 rows
    assert st["nv32"] == (62, 62, 20) and st["nv33"] == (62, 62, 20)                        # 62 rows at 32 and 33 dofs
    assert st["nv63-whole-chunks"] == (32, 32)                                              # nefc an exact multiple of the chunk: last == chunk
    assert any(len(s) > 1 and s[-1] == 1 for s in st.values())                              # a last chunk of one row
    bare = sorted((c.want[0], c.want[5]) for c in TABLE if not c.contacts)
    assert bare == [(1, 1), (3, 1), (7, 7), (8, 8), (9, 9)], bare                            # limit rows alone: nefc 1, 7, 8, 9, and nv 3 with nefc 1
    mixed = [c for c in TABLE if c.want[1] > 0 and c.want[2] > 0 and c.want[4] > 0]
    assert len(mixed) >= 2 and any(c.elliptic for c in mixed)
    ell = {c.want[0] for c in TABLE if c.elliptic}
    assert {5, 32, 33, 64, 65} <= ell
    second = []
    for c in TABLE:  # efc_ar's second buffer: more than one chunk, and the plan's LDS holds qLD's triangle and two chunks
        nv = c.want[0]
        chunk, nchunk, _, lds = got[c.name][1][cs.AR]
        tri, ld = nv * (nv + 1) // 2, nv | 1
        one, two = [((tri + k * chunk * ld) * size[c.dtype] + 15) & ~15 for k in (1, 2)]
        assert lds == (two if nchunk > 1 else one), (c.name, lds, one, two)
        if nchunk > 1:
            second.append(c.name)
    assert len(second) >= 4, second
    return dict(second_buffer=second, staged=st)


# ---- the value edges' inputs ------------------------------------------------------------------------------------------------------------------------

def _tiny(dt):
    """(smallest positive subnormal = nextafter(0, 1), smallest positive normal) of the dtype."""
    return np.nextafter(dt(0), dt(1)), np.finfo(dt).tiny


def zone_edge_inputs(name):
    """The leaves and the ``jar`` of the zone-boundary test on a mixed entry: (arrays with ``efc_D = 4`` everywhere and a new ``efc_frictionloss``, jar [B, nefc]).
    ``r = 0.25`` and ``fl`` in {0.5, 3} make ``r fl`` exact in every precision.  Slots are (environment, row) pairs in environment-major order, per row class:

    * friction rows, then the rows past ``ne + nf``: the 12 pairs (fl, jar) with jar in {-r fl, +r fl, one step to each side of both};
    * equality rows (fl = 0), then later rows with fl = 0, then later rows with fl = 0.5: jar in {0, -0, +-the smallest subnormal (nextafter(0, +-1)), +-the smallest normal};
    * every other slot: the seeded jar, fl = 0 (friction rows: fl = 0.5)."""
    m, _, A, q = problem(name)
    _, ne, nf, _, _, nefc = sizes(m)
    dt = NPDT[BY_NAME[name].dtype]
    A = dict(A)
    A["efc_D"] = np.full((B, nefc), 4, dtype=dt)
    fl = np.zeros((B, nefc), dtype=dt)
    fl[:, ne:ne + nf] = 0.5
    jar = q["jar"].copy()
    edges = []
    for f in (0.5, 3.0):
        for s in (-1, 1):
            x = dt(s * 0.25 * f)
            edges += [(f, x), (f, np.nextafter(x, dt(-np.inf))), (f, np.nextafter(x, dt(np.inf)))]
    sub, tiny = _tiny(dt)
    zeros = [dt(0.0), dt(-0.0), sub, -sub, tiny, -tiny]
    fric = [(e, i) for e in range(B) for i in range(ne, ne + nf)]
    eq = [(e, i) for e in range(B) for i in range(ne)]
    late = [(e, i) for e in range(B) for i in range(ne + nf, nefc)]
    assert len(fric) >= len(edges) and len(eq) >= len(zeros) and len(late) >= len(edges) + 2 * len(zeros)
    for (e, i), (f, x) in zip(fric, edges):
        fl[e, i], jar[e, i] = f, x
    for (e, i), (f, x) in zip(late, edges):
        fl[e, i], jar[e, i] = f, x
    for (e, i), x in zip(eq, zeros):
        jar[e, i] = x
    for (e, i), x in zip(late[len(edges):], zeros):
        jar[e, i] = x
    for (e, i), x in zip(late[len(edges) + len(zeros):], zeros):
        fl[e, i], jar[e, i] = 0.5, x
    A["efc_frictionloss"] = fl
    return A, jar


def zero_d_inputs(name, cone=0):
    """The leaves of an entry with ``efc_D = 0`` on every third row, counted from row 1 in environment 0, row 2 in environment 1, ...: equality, friction
    (``fl > 0``), limit and contact rows (``fl == 0``) alike."""
    m, _, A, _ = problem(name, cone)
    A = dict(A)
    D = A["efc_D"].copy()
    for e in range(B):
        D[e, (1 + e) % 3::3] = 0
    A["efc_D"] = D
    return A


PGS_EDGE_CLASSES = ("skipped", "moves", "vanishes", "bound0")


def pgs_edge_inputs(name):
    """(arrays, force0 [B, nefc], {class: bool [nefc]}) of the PGS edge rows on a mixed entry, one row of each class among the equality, the friction and the later
    rows where the class exists there:

    * ``skipped``: ``J = 0`` and ``D <= 0`` (0 and -1 in turn), so ``AR_ii = 0``: the row keeps its projected start bit for bit;
    * ``moves``: ``J = 0``, ``aref != 0``, ``D > 0``: the row goes to ``project(-b / R)``, ``b = -aref``;
    * ``vanishes``: ``J = 0``, ``aref = 0`` (``b = 0``), ``force0 != 0``: the row goes to an exact 0;
    * ``bound0``: a friction row (``J != 0``) whose ``efc_frictionloss`` is 0: an exact 0 from any start.

    ``D`` is a power of two on the ``moves`` and ``vanishes`` rows: then ``R f`` and ``res / R`` carry no rounding, and ``f - (R f + b) / R`` is ``-b / R`` exactly
    once ``f`` is near it (the subtraction of neighbours is exact) -- in general ``fl(fl(R f) / R) != f`` and the outcome is exact only up to an ulp.
    ``force0`` is positive on the later rows' ``vanishes`` row and inside the bound on the friction rows' one, so that the projection leaves it non-zero."""
    m, _, A, q = problem(name)
    _, ne, nf, _, _, nefc = sizes(m)
    assert ne >= 2 and nf >= 5 and nefc - ne - nf >= 6
    dt = NPDT[BY_NAME[name].dtype]
    A = {n: v.copy() for n, v in A.items()}
    f0 = q["pgs0"].copy()
    rows = {k: np.zeros(nefc, dtype=bool) for k in PGS_EDGE_CLASSES}
    lo, late = ne, ne + nf
    plan = dict(skipped=(0, lo, late, late + 3), moves=(1, lo + 1, late + 1), vanishes=(lo + 2, late + 2), bound0=(lo + 3,))
    for k, idx in plan.items():
        rows[k][list(idx)] = True
    for n, i in enumerate(plan["skipped"]):
        A["efc_J"][:, i] = 0
        A["efc_D"][:, i] = 0 if n % 2 == 0 else -1
        A["efc_aref"][:, i] = dt(0.75)
    for n, i in enumerate(plan["moves"]):
        A["efc_J"][:, i] = 0
        A["efc_D"][:, i] = dt(2.0 ** (n - 1))
        A["efc_aref"][:, i] = np.array(([0.3, -0.7, 1.1] if n != 1 else [0.03, -4.0, 4.0])[:B], dtype=dt)  # (the friction row: inside its bound, then past either)
    for i in plan["vanishes"]:
        A["efc_J"][:, i] = 0
        A["efc_D"][:, i] = dt(8.0)
        A["efc_aref"][:, i] = 0
    f0[:, lo + 2] = (0.5 * A["efc_frictionloss"][:, lo + 2]).astype(dt)
    f0[:, late + 2] = np.abs(f0[:, late + 2]) + dt(0.125)
    A["efc_frictionloss"][:, lo + 3] = 0
    return A, f0, rows


def on_bounds_start(m, A, dtype):
    """A ``force0`` exactly on its bounds: +- ``efc_frictionloss`` in turn on the friction rows, 0 on every second later row and positive on the others, free on
    the equality rows."""
    _, ne, nf, _, _, nefc = sizes(m)
    f0 = np.abs(np.random.RandomState(9).randn(B, nefc)).astype(NPDT[dtype])
    f0[:, :ne] *= -1
    fl = A["efc_frictionloss"][:, ne:ne + nf]
    f0[:, ne:ne + nf] = fl * np.where(np.arange(nf) % 2 == 0, 1, -1).astype(fl.dtype)
    f0[:, ne + nf::2] = 0
    return f0


def with_arrays(d, A):
    """The Data ``d`` with the leaves of ``A`` in place of its own (host tensors)."""
    return d.replace(**{n: torch.from_numpy(np.ascontiguousarray(A[n])) for n in SYNTH_LEAVES})
