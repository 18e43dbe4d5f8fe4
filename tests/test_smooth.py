"""kinematics / com_pos / crb / tendon_armature / factor_m / com_vel / rne on the GPU (mujoco_torch_amd/smooth.py, csrc/mjh_smooth.h) against the reference's
recordings on EDITED leaves (tests/golden/smooth/, tools/gen_smooth_golden.py), against ``forward`` and against themselves.

The bound is the project's own for pre-solver leaves, ``TOL_PRE[dtype]`` (tests/_cases.py: 1e-9 / 2e-4) as ``_util.rel_err`` measures; the generator asserts that the
reference's recorded outputs lie within it of the longdouble evaluation (tests/_smooth_ref.py, pinned by tests/test_smooth_host.py).  Nothing is read off the kernels.
Measured on one MI355X, worst error / bound over the recorded cases: see DESIGN.md section 4."""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import _smooth_ref as sr
import _support_ref as sup
import mujoco_torch_amd as mt
from _cases import TOL_PRE
from _util import load_model, rel_err
from mujoco_torch_amd import native
from mujoco_torch_amd._enums import DisableBit

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
F64, F32 = torch.float64, torch.float32
SIX = ("com_pos", "crb", "tendon_armature", "factor_m", "com_vel", "rne")
_DEVICE = {}


def device_model(c):
    if c.name not in _DEVICE:
        _DEVICE[c.name] = c.model.to(DEV)
    return _DEVICE[c.name]


def host(t):
    return t.detach().cpu().numpy()


def run(tag, mx, d):
    return mt.rne(mx, d, flg_acc=True) if tag == "rne_acc" else getattr(mt, tag)(mx, d)


def writes(tag):
    return sr.WRITES[tag.replace("_acc", "")]


@pytest.mark.parametrize("name", sr.CASES)
def test_every_function_on_the_recorded_edited_leaves(name):
    """Every function on every recorded environment, stacked into one batch, on the recorded (edited) inputs: each replaced leaf within TOL_PRE of the recording.
    ``kinematics`` is the kinematics stage of the pass, bit for bit, and within TOL_PRE of the reference's."""
    c = sr.case(name)
    mx, tol = device_model(c), TOL_PRE[c.dtype]
    worst = {}
    for tag in sr.tags(c.V):
        d = c.data(c.nenv, DEV, tag.replace("_acc", ""))
        out = run(tag, mx, d)
        for n in writes(tag):
            got = host(getattr(out, n))
            assert got.shape == tuple(getattr(d, n).shape) and getattr(out, n).dtype == c.dtype, (tag, n)
            for e in range(c.nenv):
                worst[tag] = max(worst.get(tag, 0.0), rel_err(got[e], c.outs[e][tag][n]) / tol)
        if tag == "crb":
            qM = host(out.qM)
            assert np.array_equal(qM, qM.transpose(0, 2, 1)) and not host(out.crb)[:, 0].any()
        if tag == "factor_m":
            assert not np.triu(host(out.qLD), 1).any()
    d = c.data(c.nenv, DEV, "kinematics")
    k, f = mt.kinematics(mx, d), mt.forward(mx, d, stages=1)
    for n in sr.WRITES["kinematics"]:
        assert torch.equal(getattr(k, n), getattr(f, n)), n
        for e in range(c.nenv):
            r = rel_err(host(getattr(k, n))[e], c.outs[e]["kinematics"][n].reshape(host(getattr(k, n))[e].shape)) / tol
            assert r <= 1, ("kinematics", n, e, r)
            worst["kinematics"] = max(worst.get("kinematics", 0.0), r)
    print(f"{name}: worst error / TOL_PRE " + ", ".join(f"{t} {v:.3g}" for t, v in worst.items()))
    assert max(worst.values()) <= 1, worst


@pytest.mark.parametrize("name", ["pendula_f64", "humanoid_f32"])
def test_only_the_listed_leaves_are_replaced_and_the_input_is_not_written(name):
    c = sr.case(name)
    mx = device_model(c)
    for tag in ("kinematics",) + sr.tags(c.V):
        d = c.data(3, DEV, tag.replace("_acc", ""))
        before = {n: t.clone() for n, t in d.items() if isinstance(t, torch.Tensor)}
        out = run(tag, mx, d)
        for n, t in before.items():
            assert torch.equal(getattr(d, n), t), (tag, n)
            if n in writes(tag):
                assert getattr(out, n).data_ptr() != getattr(d, n).data_ptr() or t.numel() == 0, (tag, n)
            else:
                assert getattr(out, n) is getattr(d, n), (tag, n)


_CHAIN = {}


def chain(xml, dtype=F64, B=5):
    """(model, forward's Data, the Data of the seven functions run one after the other from the same qpos, qvel and forward's ten_J)."""
    if (xml, dtype, B) not in _CHAIN:
        mc = load_model(xml, dtype=dtype)
        mx = mc.to(DEV)
        rng = np.random.RandomState(11)
        d = mt.make_data(mc).expand(B).clone()
        d = d.replace(qpos=d.qpos + torch.tensor(0.2 * rng.randn(*d.qpos.shape)), qvel=torch.tensor(0.5 * rng.randn(B, int(mc.nv))))
        d = (d if dtype == F64 else d.to(dtype)).to(DEV)
        f = mt.forward(mx, d)
        s = d.replace(ten_J=f.ten_J)
        for fn in (mt.kinematics, mt.com_pos, mt.crb, mt.tendon_armature, mt.factor_m, mt.com_vel, mt.rne):
            s = fn(mx, s)
        _CHAIN[(xml, dtype, B)] = (mc, mx, f, s)
    return _CHAIN[(xml, dtype, B)]


@pytest.mark.parametrize("xml", ["pendula", "humanoid", "tendon_armature", "centipede"])
def test_the_chain_reproduces_forward_and_its_factor_solves(xml):
    mc, mx, f, s = chain(xml)
    worst = 0.0
    for n in ("qpos", "xpos", "xmat", "xipos", "ximat", "xanchor", "xaxis", "subtree_com", "cinert", "cdof", "crb", "qM", "qLD", "cvel", "cdof_dot", "qfrc_bias"):
        for e in range(f.qpos.shape[0]):
            worst = max(worst, rel_err(host(getattr(s, n))[e], host(getattr(f, n))[e]) / TOL_PRE[F64])
    print(f"{xml}: the chain against forward, worst error / TOL_PRE {worst:.3g}")
    assert worst <= 1
    nv, B = int(mc.nv), f.qpos.shape[0]
    v = torch.tensor(np.random.RandomState(5).randn(B, 1, nv), device=DEV)
    x = mt.solve_m(mx, s, v)
    res, s_abs = sup.solve_m_residual(host(s.qLD).reshape(B, nv, nv), host(v), host(x).reshape(B, 1, nv))
    assert (res <= sup.solve_m_factor(nv, 2.0 ** -53) * s_abs).all()  # x solves (L L^T) x = v for the new factor ...
    A = np.stack([sr.factored_matrix(dict(nv=nv), host(s.qM)[e].reshape(nv, nv)) for e in range(B)])
    g, clamp = sr.factor_bound(dict(nv=nv), A, 2.0 ** -53)
    L = np.tril(host(s.qLD).reshape(B, nv, nv)).astype(sr.HP)
    back = np.abs(L @ L.transpose(0, 2, 1) - A)  # ... and the factor is qM's (+ 1e-10 I above 16 dofs) within the factorisation's backward error
    assert (back <= g * (np.abs(L) @ np.abs(L).transpose(0, 2, 1)) + clamp).all()


@pytest.mark.parametrize("name", ["pendula_f64", "humanoid_f32", "centipede_f64"])
def test_an_environment_of_a_batch_equals_itself_alone_and_batch_shapes_agree(name):
    """Lanes, environments per workgroup and LDS follow from the model alone: environment e of 70 is the call on it alone, bit for bit; batch shape (2, 3) is the flat 6;
    B = 1 and B = 3 (partly filled workgroups) are slices of the 70."""
    c = sr.case(name)
    mx = device_model(c)
    for tag in sr.tags(c.V):
        d = c.data(70, DEV, tag.replace("_acc", ""))
        rng = np.random.RandomState(3)
        if tag == "factor_m":  # 70 different matrices that stay positive definite: the diagonal grows by up to 5 %
            grow = torch.tensor(1 + 0.05 * rng.uniform(0, 1, (70, c.V["nv"])), dtype=c.dtype, device=DEV)
            d = d.replace(qM=d.qM + torch.diag_embed(torch.diagonal(d.qM, dim1=-2, dim2=-1) * (grow - 1)))
        else:
            d = d.replace(**{n: getattr(d, n) * torch.tensor(1 + 0.05 * rng.uniform(-1, 1, tuple(getattr(d, n).shape)), dtype=c.dtype, device=DEV)
                             for n in sr.READS[tag.replace("_acc", "")]})
        full = run(tag, mx, d)
        for n in writes(tag):
            assert torch.isfinite(getattr(full, n)).all() and not torch.equal(getattr(full, n)[:3], getattr(full, n)[3:6]), (tag, n)
        for lo, hi in ((0, 1), (7, 8), (33, 34), (69, 70), (0, 3), (64, 67)):
            part = run(tag, mx, d[lo:hi])
            for n in writes(tag):
                assert torch.equal(getattr(part, n), getattr(full, n)[lo:hi]), (tag, n, lo, hi)
        flat = d[:6]
        six = run(tag, mx, flat.replace(**{n: t.reshape((2, 3) + tuple(t.shape[1:])) for n, t in flat.items() if isinstance(t, torch.Tensor)}))
        for n in writes(tag):
            assert tuple(getattr(six, n).shape[:2]) == (2, 3) and torch.equal(getattr(six, n).reshape(getattr(full, n)[:6].shape), getattr(full, n)[:6]), (tag, n)


def test_value_edits_of_the_callers_model_take_effect():
    c = sr.case("humanoid_f64")
    mx = device_model(c)
    d = c.data(3, DEV)
    base = mt.com_pos(mx, d)
    mass = mx.body_mass.clone()
    mass[3] = mass[3] * 2
    heavy = mt.com_pos(mx.replace(body_mass=mass), d)
    assert not torch.equal(heavy.subtree_com, base.subtree_com) and not torch.equal(heavy.cinert[:, 3], base.cinert[:, 3])
    q0 = mt.crb(mx, d)
    arm = mx.dof_armature + torch.linspace(0.1, 0.5, int(mx.nv), dtype=F64, device=DEV)
    q1 = mt.crb(mx.replace(dof_armature=arm), d)
    assert torch.equal(q1.crb, q0.crb)
    diff = q1.qM - q0.qM
    off = diff - torch.diag_embed(torch.diagonal(diff, dim1=-2, dim2=-1))
    assert not off.any() and (torch.diagonal(diff, dim1=-2, dim2=-1) > 0.05).all()
    b0 = mt.rne(mx, d)
    b1 = mt.rne(mx.replace(opt=mx.opt.replace(disableflags=int(mx.opt.disableflags) | int(DisableBit.GRAVITY))), d)
    b2 = mt.rne(mx.replace(opt=mx.opt.replace(gravity=torch.zeros(3, dtype=F64))), d)
    assert not torch.equal(b0.qfrc_bias, b1.qfrc_bias) and torch.equal(b1.qfrc_bias, b2.qfrc_bias)
    want = np.stack([sr.rne(sr.model_values(c.model, disableflags=int(DisableBit.GRAVITY)), c.passes[e])["qfrc_bias"] for e in range(3)])
    assert rel_err(host(b1.qfrc_bias), want.astype(np.float64)) <= TOL_PRE[F64]


def test_a_model_without_dofs_returns_empty_leaves_without_a_launch():
    xml = '<mujoco><worldbody><body pos="0 0 1"><geom type="sphere" size="0.1" mass="2"/><body pos="0.3 0 0"><geom type="box" size="0.1 0.2 0.3" mass="1"/></body></body></worldbody></mujoco>'
    mc = mt.device_put(mt.mjcf.from_xml_string(xml))
    mx = mc.to(DEV)
    assert int(mc.nv) == 0 and int(mc.nbody) == 3
    rng = np.random.RandomState(2)
    d = mt.make_data(mc).expand(2).clone()
    d = d.replace(xipos=torch.tensor(rng.randn(2, 3, 3)), ximat=torch.tensor(np.linalg.qr(rng.randn(2, 3, 3, 3))[0]), xmat=torch.tensor(np.linalg.qr(rng.randn(2, 3, 3, 3))[0])).to(DEV)
    V = sr.model_values(mc)
    nm = native.get_native_model(mx, torch.device("cuda", 0), F64)

    def launches(call):
        nm.lib.mjh_debug_phase_timing(1)
        try:
            out = call()
            ms, ids = (ctypes.c_float * 16)(), (ctypes.c_int * 16)()
            k = nm.lib.mjh_debug_phase_times(ms, ids, 16)
        finally:
            nm.lib.mjh_debug_phase_timing(0)
        return out, [ids[i] for i in range(k)]

    cp, ran = launches(lambda: mt.com_pos(mx, d))
    assert ran == [57] and tuple(cp.cdof.shape) == (2, 0, 6)
    for e in range(2):
        want = sr.com_pos(V, {n: host(getattr(d, n))[e] for n in sr.READS["com_pos"]})
        assert rel_err(host(cp.subtree_com)[e], want["subtree_com"].astype(np.float64)) <= TOL_PRE[F64]
        assert rel_err(host(cp.cinert)[e], want["cinert"].astype(np.float64)) <= TOL_PRE[F64]
    mt.com_pos(mx, d)  # (the timing aid keeps the launches of the most recent native call: a call that launches nothing leaves this one's)
    for fn, leaves in ((mt.factor_m, ("qLD",)), (mt.com_vel, ("cdof_dot",)), (mt.rne, ("qfrc_bias",))):
        out, ran = launches(lambda: fn(mx, d))
        assert ran in ([], [57]), fn.__name__
        for n in leaves:
            assert getattr(out, n).numel() == 0 and getattr(out, n).shape[0] == 2
    assert mt.crb(mx, d).qM.numel() == 0 and tuple(mt.crb(mx, d).crb.shape) == (2, 3, 10) and not mt.com_vel(mx, d).cvel.any()
    assert mt.tendon_armature(mx, d) is d


_CUT_CHILD = r'''
import sys
sys.path.insert(0, "tests"); sys.path.insert(0, "mujoco-torch_amd"); sys.path.insert(0, "oracle")
import torch, mujoco_torch_amd as mt
import _smooth_ref as sr
res = {}
for name in sys.argv[3:]:
    c = sr.case(name)
    mx = c.model.to("cuda")
    for tag in sr.tags(c.V):
        d = c.data(int(sys.argv[2]), "cuda", tag.replace("_acc", ""))
        out = mt.rne(mx, d, flg_acc=True) if tag == "rne_acc" else getattr(mt, tag)(mx, d)
        for n in sr.WRITES[tag.replace("_acc", "")]:
            res[f"{name}/{tag}/{n}"] = getattr(out, n).cpu()
torch.save(res, sys.argv[1])
print("ran", len(res))
'''


def test_batches_past_one_launch_are_cut_on_the_host():
    """MJH_MAX_GRID_LOG2=2 caps a launch at 4 workgroups of at most 16 environments: 70 environments go out in several launches with a short last one.  All six
    kernels must give the bits of the uncut run, in a fresh process each (the library reads the switch once)."""
    names = ["pendula_f64", "tendon_armature_f64"]
    with tempfile.TemporaryDirectory() as td:
        res = {}
        for tag, env in (("one", {}), ("cut", {"MJH_MAX_GRID_LOG2": "2"})):
            out = os.path.join(td, tag + ".pt")
            base = {k: v for k, v in os.environ.items() if k != "MJH_MAX_GRID_LOG2"}
            r = subprocess.run([sys.executable, "-c", _CUT_CHILD, out, "70"] + names, cwd=ROOT, env=dict(base, **env), capture_output=True, text=True, timeout=300)
            assert r.returncode == 0 and "ran" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
            res[tag] = torch.load(out)
    assert {k.split("/")[1] for k in res["one"]} == set(SIX) | {"rne_acc"}
    for k, a in res["one"].items():
        assert a.shape[0] == 70 and torch.isfinite(a).all() and bool(a.any()), k
        assert torch.equal(a, res["cut"][k]), k


def test_every_op_is_timed_under_its_id_and_accounted_for():
    c = sr.case("tendon_armature_f64")
    mx = device_model(c)
    nb, nv, nj, nt = (c.V[k] for k in ("nb", "nv", "nj", "nt"))
    assert nt > 0
    nm = native.get_native_model(mx, torch.device("cuda", 0), F64)
    rw = (ctypes.c_int64 * 2)()
    want = {57: (21 * nb + 6 * nj, 13 * nb + 6 * nv), 58: (10 * nb + 6 * nv, 10 * nb + nv * nv), 59: (nv * nv + nt * nv, nv * nv), 60: (nv * (nv + 1) // 2, nv * nv),
            61: (7 * nv, 6 * nb + 6 * nv), 62: (14 * nv + 16 * nb, nv)}
    for op, fn in enumerate(SIX):
        kid = 57 + op
        d = c.data(3, DEV, fn)
        assert nm.lib.mjh_model_kernel_io(nm.handle, kid, rw) == 0 and (rw[0], rw[1]) == tuple(8 * x for x in want[kid]), fn
        nm.lib.mjh_debug_phase_timing(1)
        try:
            getattr(mt, fn)(mx, d)
            ms, ids = (ctypes.c_float * 16)(), (ctypes.c_int * 16)()
            k = nm.lib.mjh_debug_phase_times(ms, ids, 16)
        finally:
            nm.lib.mjh_debug_phase_timing(0)
        assert [ids[i] for i in range(k)] == [kid] and ms[0] > 0, fn
