"""jac_body / jac_body_com / jac_site / jac_geom, jac_subtree_com, jac_dot and angmom_mat on the GPU (mujoco_torch_amd/jacobian.py, csrc/mjh_jacobian.h), matrix and
product form, against the tests' own numpy reference (tests/_jacobian_ref.py, pinned without a GPU by tests/test_jacobian_host.py) evaluated in high precision on the
very leaves the kernels read (this library's own ``forward`` output).

No tolerance here is read off the kernels.  An element is held to ``(n + 2)(eps + EPS_HP) S_abs`` (``_support_ref.bound``): S_abs the sum of the absolute elementary
products it is made of, n their number plus the roundings one takes on its way (the reference's docstring counts them), eps the unit of the Data's dtype.  Where
two same-dtype evaluations run the same operations in the same order -- the object Jacobians and ``jac``, a slice of the batch and the whole batch, a cut launch and
an uncut one -- the results must be ``torch.equal``.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import _fd_ref as fr
import _jacobian_ref as jr
import _postcon_ref as pr
import mujoco_torch_amd as mt
from _util import load_model

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64, F32 = torch.float64, torch.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 5
CASES = [("pendula", F64), ("ball_limits", F64), ("humanoid", F64), ("humanoid", F32), ("centipede", F64)]
_ids = lambda cases: [f"{x}-{str(t).replace('torch.', '')}" for x, t in cases]
_PASSES = {}


def a_pass(xml, dtype):
    """(host model, device model, Data after forward on the device, the reference's tables and host leaves): B states moved off qpos0, non-zero qvel."""
    key = (xml, dtype)
    if key not in _PASSES:
        mc = load_model(xml, dtype=dtype)
        mx = mc.to(DEV)
        jt = fr.Joints(jr._np(mc.jnt_type), jr._np(mc.jnt_qposadr), jr._np(mc.jnt_dofadr), mc.nq, mc.nv)
        rng = np.random.RandomState(17)
        q = fr.integrate(jt, np.broadcast_to(np.asarray(jr._np(mc.qpos0), dtype=np.float64), (B, jt.nq)), 0.3 * rng.randn(B, jt.nv), 1.0)
        d = mt.make_data(mc).expand(B).clone()
        d = d.replace(qpos=torch.tensor(q), qvel=torch.tensor(0.5 * rng.randn(B, jt.nv)))
        if dtype != F64:
            d = d.to(dtype)
        f = mt.forward(mx, d.to(DEV))
        _PASSES[key] = (mc, mx, f, jr.tables(mc), jr.leaves_of(f))
    return _PASSES[key]


def _host(t):
    return t.detach().cpu().numpy()


def _within(got, triple, eps, what, nonzero=True):
    """|got - value| <= bound(n, eps, S_abs) per element; prints the worst ratio before it asserts."""
    val, S, n = triple
    got = np.asarray(_host(got), dtype=jr.HP).reshape(val.shape)
    err = np.abs(got - val).astype(np.float64)
    allowed = jr.bound(n, eps, S)
    assert np.isfinite(err).all(), what
    ratio = float((err / np.maximum(allowed, 1e-300)).max())
    print(f"{what}: worst error / bound {ratio:.3f} over {err.size} elements; largest entry {float(np.abs(val).max()):.3g}")
    assert not nonzero or np.abs(val).max() > 0, what  # (something to compare)
    over = err > allowed
    assert not over.any(), f"{what}: {int(over.sum())} of {err.size} elements beyond their bound (worst ratio {ratio:.3g})"


def _listed(T):
    """Three body ids: the world (the whole model), a leaf body that some dof moves, and a moving body of another tree than the leaf's where the model has
    several (else a middle body)."""
    nb, root = T["nbody"], T["root"]
    leaf = max(b for b in range(1, nb) if T["sub"][b].sum() == 1 and T["mask"][b].any())
    other = [b for b in range(1, nb) if root[b] != root[leaf] and T["mask"][b].any()]
    third = other[0] if other else next(b for b in range(1, nb) if T["sub"][b].sum() > 1 and T["parent"][b] != 0)
    return [0, leaf, third]


def _points(rng, f, P, mode, dtype):
    base = f.xipos.mean(1)  # near the model, per environment
    if mode == "shared":
        return torch.tensor(rng.randn(3), dtype=dtype, device=DEV)
    if mode == "env":
        return base + torch.tensor(0.3 * rng.randn(B, 3), dtype=dtype, device=DEV)
    return base[:, None, :] + torch.tensor(0.3 * rng.randn(B, P, 3), dtype=dtype, device=DEV)


# ---- 1. every function, both forms, against the reference --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("listed", [False, True], ids=["P1", "P3"])
@pytest.mark.parametrize("xml,dtype", CASES, ids=_ids(CASES))
def test_every_function_against_the_reference(xml, dtype, listed):
    mc, mx, f, T, L = a_pass(xml, dtype)
    eps = torch.finfo(dtype).eps
    rng = np.random.RandomState(23)
    three = _listed(T)
    ids = three if listed else three[1]
    idl = three if listed else [three[1]]
    P = len(idl)
    vec = f.qvel
    what = f"{xml} {str(dtype)[6:]} P={P}"
    # the subtree functions
    for name, fn, ref in (("jac_subtree_com", mt.jac_subtree_com, jr.subtree_com_hp), ("angmom_mat", mt.angmom_mat, jr.angmom_hp)):
        want = ref(T, L, idl)
        got = fn(mx, f, ids)
        assert tuple(got.shape) == (B,) + ((P,) if listed else ()) + (int(mc.nv), 3) and got.dtype == dtype
        _within(got, want, eps, f"{what} {name}")
        gv = fn(mx, f, ids, vec=vec)
        assert tuple(gv.shape) == (B,) + ((P,) if listed else ()) + (3,)
        _within(gv, jr.product(want, _host(vec)), eps, f"{what} {name} vec")
    # jac_dot, with the three point forms
    for mode in ("shared", "env") + (("query",) if listed else ()):
        pt = _points(rng, f, P, mode, dtype)
        wp, wr = jr.dot_hp(T, L, _host(pt), idl)
        gp, gr = mt.jac_dot(mx, f, pt, ids)
        assert tuple(gp.shape) == tuple(gr.shape) == (B,) + ((P,) if listed else ()) + (int(mc.nv), 3)
        _within(gp, wp, eps, f"{what} jacp_dot ({mode} point)")
        _within(gr, wr, eps, f"{what} jacr_dot ({mode} point)", nonzero=xml == "humanoid")  # (the axis of a hinge on the world does not turn)
        vp, vr = mt.jac_dot(mx, f, pt, ids, vec=vec)
        assert tuple(vp.shape) == tuple(vr.shape) == (B,) + ((P,) if listed else ()) + (3,)
        _within(vp, jr.product(wp, _host(vec)), eps, f"{what} jacp_dot vec ({mode} point)")
        _within(vr, jr.product(wr, _host(vec)), eps, f"{what} jacr_dot vec ({mode} point)", nonzero=xml == "humanoid")
    # the object Jacobians times a vector (the matrices themselves: test_the_object_jacobians_are_jac_bit_for_bit)
    objects = [("jac_body", mt.jac_body, f.xpos, None, idl), ("jac_body_com", mt.jac_body_com, f.xipos, None, idl)]
    ng, ns = int(mc.ngeom), int(mc.nsite)
    moving = lambda bodyid: [i for i in range(len(bodyid)) if T["mask"][int(bodyid[i])].any()]  # (objects some dof moves)
    gm = moving(jr._np(mc.geom_bodyid))
    objects.append(("jac_geom", mt.jac_geom, f.geom_xpos, jr._np(mc.geom_bodyid), [gm[-1], gm[len(gm) // 2], 0][:P]))
    if ns:
        sm = moving(jr._np(mc.site_bodyid))
        objects.append(("jac_site", mt.jac_site, f.site_xpos, jr._np(mc.site_bodyid), [sm[-1], sm[len(sm) // 2], 0][:P]))
    for name, fn, pos, bodyid, oid in objects:
        bodies = oid if bodyid is None else [int(bodyid[i]) for i in oid]
        wp, wr = jr.point_hp(T, L, _host(pos)[:, oid], bodies)
        vp, vr = fn(mx, f, oid if listed else oid[0], vec=vec)
        assert tuple(vp.shape) == tuple(vr.shape) == (B,) + ((P,) if listed else ()) + (3,)
        _within(vp, jr.product(wp, _host(vec)), eps, f"{what} {name} vec (linear)")
        _within(vr, jr.product(wr, _host(vec)), eps, f"{what} {name} vec (angular)")


def test_a_model_with_sites_is_among_the_cases():
    assert int(a_pass("pendula", F64)[0].nsite) > 0 and a_pass("centipede", F64)[0].nv > 64 and len(set(a_pass("pendula", F64)[3]["root"][1:].tolist())) > 1


# ---- 2. agreement with the existing kernels ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("xml,dtype", [("pendula", F64), ("humanoid", F32)], ids=["pendula-float64", "humanoid-float32"])
def test_the_object_jacobians_are_jac_bit_for_bit(xml, dtype):
    mc, mx, f, T, _ = a_pass(xml, dtype)
    nb, ng, ns = int(mc.nbody), int(mc.ngeom), int(mc.nsite)
    gb, sb = jr._np(mc.geom_bodyid), jr._np(mc.site_bodyid)
    cases = [(mt.jac_body, f.xpos, None, [0, 1, nb - 1]), (mt.jac_body_com, f.xipos, None, [nb - 1, 2, 0]), (mt.jac_geom, f.geom_xpos, gb, [0, ng - 1, ng // 2])]
    if ns:
        cases.append((mt.jac_site, f.site_xpos, sb, [ns - 1, 0, ns // 2]))
    for fn, pos, bodyid, oid in cases:
        bodies = oid if bodyid is None else [int(bodyid[i]) for i in oid]
        jp, jrot = fn(mx, f, oid)
        wp, wr = mt.jac(mx, f, pos[:, oid], bodies)
        assert torch.equal(jp, wp) and torch.equal(jrot, wr) and tuple(jp.shape) == (B, 3, int(mc.nv), 3), fn.__name__
        one = fn(mx, f, oid[1])
        w1 = mt.jac(mx, f, pos[:, oid[1]], bodies[1])
        assert torch.equal(one[0], w1[0]) and torch.equal(one[1], w1[1]) and torch.equal(one[0], jp[:, 1]), fn.__name__
        assert jp.any() or bodies == [0, 0, 0]


@pytest.mark.parametrize("xml,dtype", [("pendula", F64), ("humanoid", F64), ("humanoid", F32), ("centipede", F64)], ids=_ids([("pendula", F64), ("humanoid", F64), ("humanoid", F32), ("centipede", F64)]))
def test_the_products_with_qvel_are_subtree_vel_and_the_matrix_times_qvel(xml, dtype):
    """``vec = qvel``: the product forms against ``subtree_vel``'s leaves and against the matrix form contracted on the host in high precision.  With b_j the
    product's bound and b_p ``_postcon_ref``'s (both at the dtype's eps), each kernel lies within its own bound of its own reference and the two references differ
    by the leaves' rounding, which b_j + b_p bounds (tests/test_jacobian_host.py): allowed = 2 (b_j + b_p).  The matrix form: the product's bound plus the
    elements' own bounds weighted by |qvel|."""
    mc, mx, f, T, L = a_pass(xml, dtype)
    eps = torch.finfo(dtype).eps
    ids = list(range(T["nbody"]))
    sv = mt.subtree_vel(mx, f)
    ref = pr.evaluate(pr.tables(mc), dict(cvel=L["cvel"], xipos=L["xipos"], ximat=L["ximat"], subtree_com=L["subtree_com"]), rne=False, subtree=True)
    q = np.asarray(_host(f.qvel), dtype=jr.HP)
    for name, fn, hp, leaf in (("jac_subtree_com", mt.jac_subtree_com, jr.subtree_com_hp, "subtree_linvel"), ("angmom_mat", mt.angmom_mat, jr.angmom_hp, "subtree_angmom")):
        want = hp(T, L, ids)
        pv, pS, pn = jr.product(want, q)
        got = np.asarray(_host(fn(mx, f, ids, vec=f.qvel)), dtype=jr.HP)
        _, Sr, nr = ref[leaf]
        allowed = 2 * (jr.bound(pn, eps, pS) + pr.bound(nr, eps, Sr))
        err = np.abs(got - np.asarray(_host(getattr(sv, leaf)), dtype=jr.HP)).astype(np.float64)
        print(f"{xml} {name} . qvel against {leaf}: worst error / allowed {float((err / np.maximum(allowed, 1e-300)).max()):.3f}")
        assert (err <= allowed).all() and np.abs(got).max() > 1e-3
        mat = np.asarray(_host(fn(mx, f, ids)), dtype=jr.HP)
        allowed = jr.bound(pn, eps, pS) + (jr.bound(want[2], eps, want[1]) * np.abs(q)[:, None, :, None].astype(np.float64)).sum(2)
        err = np.abs((mat * q[:, None, :, None]).sum(2) - got).astype(np.float64)
        print(f"{xml} {name}: product form against the matrix form times qvel: worst error / allowed {float((err / np.maximum(allowed, 1e-300)).max()):.3f}")
        assert (err <= allowed).all()


# ---- 3. slices and cuts ------------------------------------------------------------------------------------------------------------------------------

def _all_calls(mx, f, ids, pt, vec):
    out = {}
    out["sc"], out["am"] = mt.jac_subtree_com(mx, f, ids), mt.angmom_mat(mx, f, ids)
    out["dp"], out["dr"] = mt.jac_dot(mx, f, pt, ids)
    out["sc_v"], out["am_v"] = mt.jac_subtree_com(mx, f, ids, vec=vec), mt.angmom_mat(mx, f, ids, vec=vec)
    out["dp_v"], out["dr_v"] = mt.jac_dot(mx, f, pt, ids, vec=vec)
    out["bp_v"], out["br_v"] = mt.jac_body_com(mx, f, ids, vec=vec)
    return out


@pytest.mark.parametrize("xml,dtype", [("pendula", F64), ("humanoid", F32), ("centipede", F64)], ids=["pendula-float64", "humanoid-float32", "centipede-float64"])
def test_a_slice_of_the_batch_equals_the_rows_of_the_full_call(xml, dtype):
    mc, mx, f, T, _ = a_pass(xml, dtype)
    ids = _listed(T)
    pt = _points(np.random.RandomState(5), f, 3, "query", dtype)
    full = _all_calls(mx, f, ids, pt, f.qvel)
    part = _all_calls(mx, f[1:4], ids, pt[1:4], f.qvel[1:4])
    for k, a in full.items():
        assert a.any() and torch.equal(part[k], a[1:4]), k


CUT_B, CUT_P, CUT_LOG2 = 70, 5, 2
CUT_MODELS = (("humanoid", "float64"), ("pendula", "float64"))

_CUT_CHILD = r'''
import sys
sys.path.insert(0, "tests"); sys.path.insert(0, "mujoco-torch_amd"); sys.path.insert(0, "oracle")
import numpy as np, torch, mujoco_torch_amd as mt
from _util import load_model
B, P = int(sys.argv[2]), int(sys.argv[3])
res = {}
for spec in sys.argv[4:]:
    xml, dts = spec.split(":")
    dt = getattr(torch, dts)
    mc = load_model(xml, dtype=dt)
    mx = mc.to("cuda")
    nv, nb = int(mc.nv), int(mc.nbody)
    rng = np.random.RandomState(3)
    d = mt.make_data(mc).expand(B).clone()
    d = d.replace(qpos=d.qpos + torch.tensor(0.05 * rng.randn(*d.qpos.shape)), qvel=torch.tensor(0.2 * rng.randn(B, nv)))
    if dt != torch.float64: d = d.to(dt)
    d = mt.forward(mx, d.to("cuda"))
    ids = [0, 1, nb // 2, nb - 2, nb - 1]
    assert len(ids) == P
    pts = torch.tensor(rng.randn(B, P, 3), dtype=dt, device="cuda")
    out = {k: getattr(d, k) for k in ("cdof", "cdof_dot", "cvel", "subtree_com", "xipos", "ximat")}  # the leaves: a difference there is forward's
    out["sc"], out["am"] = mt.jac_subtree_com(mx, d, ids), mt.angmom_mat(mx, d, ids)
    out["dp"], out["dr"] = mt.jac_dot(mx, d, pts, ids)
    out["sc_v"], out["am_v"] = mt.jac_subtree_com(mx, d, ids, vec=d.qvel), mt.angmom_mat(mx, d, ids, vec=d.qvel)
    out["dp_v"], out["dr_v"] = mt.jac_dot(mx, d, pts, ids, vec=d.qvel)
    out["bp_v"], out["br_v"] = mt.jac_body(mx, d, ids, vec=d.qvel)
    out["sc_one"] = mt.jac_subtree_com(mx, d, 1)  # body_stride 0
    res[spec] = {k: o.cpu() for k, o in out.items()}
torch.save(res, sys.argv[1])
print("ran")
'''


def test_batches_past_one_launch_are_cut_on_the_host():
    """MJH_MAX_GRID_LOG2=2 caps a launch at 4 workgroups: 1024 elements of the matrix kernel, 64 or 32 environments of the product kernel (16 a workgroup, 8 where
    an environment's 13 nv reals -- 19 nv for jac_dot -- would pass 48 KB).  70 environments with 5 queries then run in several launches, whose boundaries fall inside an environment
    and inside a query for the matrix form (neither 3 nv P nor 3 nv divides 1024) and leave a short last launch for the product form; everything must be
    bit-identical to the uncut run."""
    launch = 256 << CUT_LOG2
    for xml, dts in CUT_MODELS:
        nv = int(load_model(xml, dtype=getattr(torch, dts)).nv)
        assert CUT_B * CUT_P * nv * 3 > launch and launch % (CUT_P * nv * 3) != 0 and launch % (nv * 3) != 0, xml
    for envs in (16, 8):
        assert CUT_B > envs << CUT_LOG2 and CUT_B % (envs << CUT_LOG2) != 0
    with tempfile.TemporaryDirectory() as td:
        res = {}
        for tag, env in (("one", {}), ("cut", {"MJH_MAX_GRID_LOG2": str(CUT_LOG2)})):
            out = os.path.join(td, tag + ".pt")
            base = {k: v for k, v in os.environ.items() if k != "MJH_MAX_GRID_LOG2"}
            r = subprocess.run([sys.executable, "-c", _CUT_CHILD, out, str(CUT_B), str(CUT_P)] + [f"{x}:{t}" for x, t in CUT_MODELS],
                               cwd=ROOT, env=dict(base, **env), capture_output=True, text=True, timeout=600)
            assert r.returncode == 0 and "ran" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
            res[tag] = torch.load(out)
    assert len(res["one"]) == len(CUT_MODELS)
    for case, outs in res["one"].items():
        assert len(outs) == 17
        for k, a in outs.items():
            assert a.shape[0] == CUT_B and torch.isfinite(a).all() and a.any(), (case, k)
            assert torch.equal(a, res["cut"][case][k]), (case, k)


# ---- 4. the model values are the caller's; the input is the caller's ---------------------------------------------------------------------------------

def test_a_value_only_edit_is_honoured_without_a_new_native_model():
    from mujoco_torch_amd._postpass import handle as _handle

    mc, mx, f, T, L = a_pass("humanoid", F64)
    nm = _handle(mx, f.qpos.device, F64)
    base = mt.jac_subtree_com(mx, f, 0)
    scale = torch.ones_like(mx.body_mass)
    scale[1:4] = 3.0  # the torso's end gets heavier: the centre of mass moves towards it
    heavy = mx.replace(body_mass=mx.body_mass * scale)
    got = mt.jac_subtree_com(heavy, f, 0)
    assert _handle(heavy, f.qpos.device, F64) is nm  # (the same native model serves the edited one)
    assert not torch.equal(got, base)
    Th = dict(T, mass=T["mass"] * np.asarray(_host(scale), dtype=jr.HP))  # (body_subtreemass kept, as in the edited Model: the definition divides by it)
    _within(got, jr.subtree_com_hp(Th, L, [0]), torch.finfo(F64).eps, "humanoid jac_subtree_com, body_mass edited")
    am = mt.angmom_mat(heavy.replace(body_inertia=2 * mx.body_inertia), f, [0, 1])
    _within(am, jr.angmom_hp(dict(Th, inertia=2 * T["inertia"]), L, [0, 1]), torch.finfo(F64).eps, "humanoid angmom_mat, body_mass and body_inertia edited")
    # all masses doubled together with body_subtreemass: the centre's Jacobian is unchanged but for the rounding of the division
    both = mx.replace(body_mass=2 * mx.body_mass, body_subtreemass=2 * mx.body_subtreemass)
    assert torch.equal(mt.jac_subtree_com(both, f, 0), base)  # (powers of two: exactly)


def test_the_input_is_not_written():
    mc, mx, f, T, _ = a_pass("pendula", F64)
    before = {n: getattr(f, n).clone() for n in jr.LEAVES + ("qvel", "xpos", "geom_xpos", "site_xpos")}
    ids = _listed(T)
    pt = _points(np.random.RandomState(2), f, 3, "query", F64)
    keep = pt.clone()
    _all_calls(mx, f, ids, pt, f.qvel)
    mt.jac_site(mx, f, [0, 1], vec=f.qvel)
    mt.jac_geom(mx, f, 0)
    torch.cuda.synchronize()
    for n, t in before.items():
        assert torch.equal(getattr(f, n), t), n
    assert torch.equal(pt, keep)
    # a side stream and an empty batch
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        side = mt.angmom_mat(mx, f, ids, vec=f.qvel)
    s.synchronize()
    assert torch.equal(side, mt.angmom_mat(mx, f, ids, vec=f.qvel))
    assert tuple(mt.jac_subtree_com(mx, f[:0], ids).shape) == (0, 3, int(mc.nv), 3) and tuple(mt.jac_dot(mx, f[:0], pt[:0], ids, vec=f.qvel[:0])[0].shape) == (0, 3, 3)
