"""The host side of kinematics / com_pos / crb / tendon_armature / factor_m / com_vel / rne (mujoco_torch_amd/smooth.py) and the tests' longdouble reference
(tests/_smooth_ref.py) against the reference's recordings (tests/golden/smooth/, tools/gen_smooth_golden.py).  No GPU.

The bound is ``TOL_PRE[dtype]`` (tests/_cases.py) as ``_util.rel_err`` measures, the one the GPU tests hold the kernels to; the recordings carry the reference's own
distance from the longdouble evaluation (``ref_distance``), which must lie inside it for the bound to mean anything."""
import ctypes
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import _smooth_ref as sr
import mujoco_torch_amd as mt
from _cases import TOL_PRE
from _util import rel_err
from mujoco_torch_amd import native, smooth

F64, F32 = torch.float64, torch.float32
U = {F64: 2.0 ** -53, F32: 2.0 ** -24}
SIX = ("com_pos", "crb", "tendon_armature", "factor_m", "com_vel", "rne")


def f64(a):
    return np.asarray(a, dtype=np.float64)


def test_the_seven_names_exist_with_the_recorded_signatures():
    api = json.load(open(os.path.join(sr.GOLD, "reference_api.json")))["signatures"]
    assert sorted(api) == sorted(sr.FUNCTIONS)
    for n, params in api.items():
        assert getattr(mt, n) is getattr(smooth, n) and list(inspect.signature(getattr(mt, n)).parameters) == params, n
    assert inspect.signature(mt.rne).parameters["flg_acc"].default is False


def test_the_header_declares_the_entry_point_the_ops_and_the_ids():
    from test_abi import header_fields

    text = open(native.HEADER).read()
    assert native.ABI_VERSION >= 27 and list(native.SmoothArgs._fields_) == header_fields(text, "mjhSmoothArgs")
    assert re.search(r"\bint mjh_smooth\s*\(const mjhModel\* m, const mjhSmoothArgs\* args, void\* hip_stream\);", text)
    for op, n in enumerate(("COM_POS", "CRB", "TENDON_ARMATURE", "FACTOR_M", "COM_VEL", "RNE")):
        assert re.search(rf"#define MJH_SMOOTH_{n} {op}\b", text) and re.search(rf"#define MJH_KERNEL_SMOOTH_{n} {57 + op}\b", text), n
        assert smooth.OPS[n.lower()] == op
    usage = open(native.LIB_PATH.replace("libmjhip.so", "resource_usage.txt")).read().splitlines()
    mine = [ln for ln in usage if "mjh_smooth_kernel" in ln]
    assert len(mine) == 12 and all("ScratchSize [bytes/lane]: 0 " in ln for ln in mine)  # six ops, two dtypes, no scratch


def test_every_case_of_the_issue_is_recorded():
    have = {n: sr.case(n) for n in sr.CASES}
    assert {(c.meta["xml"], c.meta["dtype"]) for c in have.values()} >= {("pendula", "float64"), ("pendula", "float32"), ("ant", "float64"), ("humanoid", "float64"),
                                                                          ("humanoid", "float32"), ("tendon_armature", "float64"), ("centipede", "float64")}
    assert have["ant_f64"].V["nv"] <= 16 < have["humanoid_f64"].V["nv"] and have["centipede_f64"].V["nb"] > 64 and have["centipede_f64"].V["nv"] > 64
    assert have["tendon_armature_f64"].V["tendon_armature"].any() and have["pendula_f64"].V["nt"] > 0
    assert {0, 1, 2, 3} <= set(have["pendula_f64"].V["jnt_type"].tolist())
    z = have["ant_zero_mass_f64"]
    body = z.meta["zero_mass"]["body"]
    assert z.V["body_mass"][body] == 0 and float(z.compiled.body_mass[body]) > 0 and z.model.tables.uid == z.compiled.tables.uid  # a value-only edit
    assert not (z.V["body_parentid"] == body).any()  # a leaf body: its subtree mass is below mjMINVAL
    for c in have.values():
        assert 2 <= c.nenv <= 4
        for tag, leaves in c.distance.items():
            for n, per_env in leaves.items():
                assert max(per_env, default=0.0) <= TOL_PRE[c.dtype], (c.name, tag, n)
        for e in range(c.nenv):  # the inputs are edited: no function's inputs are the pass's own
            for fn, L in c.ins[e].items():
                assert all(a.size == 0 or not np.array_equal(a, c.passes[e][n]) for n, a in L.items()), (c.name, fn)
    for f in os.listdir(sr.GOLD):
        assert os.path.getsize(os.path.join(sr.GOLD, f)) < 1 << 20, f


@pytest.mark.parametrize("name", sr.CASES)
def test_the_reference_is_pinned_on_the_recording(name):
    """The longdouble restatement matches every recorded output of the reference, on the edited inputs, within TOL_PRE."""
    c = sr.case(name)
    worst = 0.0
    for e in range(c.nenv):
        for tag in sr.tags(c.V):
            fn = tag.replace("_acc", "")
            want = sr.FN[fn](c.V, c.ins[e][fn], **(dict(flg_acc=True) if tag == "rne_acc" else {}))
            for n in sr.WRITES[fn]:
                worst = max(worst, rel_err(f64(want[n]).astype(c.outs[e][tag][n].dtype), c.outs[e][tag][n]) / TOL_PRE[c.dtype])
    assert worst <= 1, worst
    if name == "ant_zero_mass_f64":  # the mjMINVAL branch: the massless leaf body's subtree_com is its xipos
        body = c.meta["zero_mass"]["body"]
        for e in range(c.nenv):
            assert np.array_equal(c.outs[e]["com_pos"]["subtree_com"][body], c.ins[e]["com_pos"]["xipos"][body])


@pytest.mark.parametrize("name", sr.CASES)
def test_the_reference_chain_reproduces_the_recorded_pass(name):
    """On the recorded UNEDITED pass, com_pos -> crb -> tendon_armature -> factor_m and com_vel -> rne of the reference module reproduce the pass's own leaves."""
    c = sr.case(name)
    tol = TOL_PRE[c.dtype]
    for e in range(c.nenv):
        P = c.passes[e]
        L = dict(P)
        for fn in SIX:
            if fn == "tendon_armature" and c.V["nt"] == 0:
                continue
            out = sr.FN[fn](c.V, L)
            for n, a in out.items():
                if (fn, n) == ("crb", "qM") and c.V["nt"] > 0:
                    continue  # (the pass's qM is tendon_armature's)
                assert rel_err(f64(a).astype(P[n].dtype), P[n]) <= tol, (fn, n, e)
            L.update(out)


@pytest.mark.parametrize("name", ["ant_f64", "humanoid_f64", "humanoid_f32", "centipede_f64"])
def test_the_factor_times_its_transpose_is_the_matrix(name):
    """In longdouble, L L^T equals qM (+ 1e-10 I above 16 dofs) within the factorisation's backward error, for the recorded factor of the edited matrix."""
    c = sr.case(name)
    for e in range(c.nenv):
        A = sr.factored_matrix(c.V, c.ins[e]["factor_m"]["qM"])
        for L in (sr.factor_m(c.V, c.ins[e]["factor_m"])["qLD"], np.asarray(c.outs[e]["factor_m"]["qLD"], dtype=sr.HP)):
            assert not np.triu(L, 1).any()
            g, clamp = sr.factor_bound(c.V, A, U[c.dtype])
            assert (np.abs(L @ L.T - A) <= g * (np.abs(L) @ np.abs(L).T) + clamp).all()


@pytest.mark.parametrize("name", ["pendula_f64", "humanoid_f64", "centipede_f64"])
def test_rne_with_accelerations_adds_the_mass_matrix_product(name):
    """rne(flg_acc=True) - rne() = (qM - diag(dof_armature)) qacc for the crb of the same leaves."""
    c = sr.case(name)
    for e in range(c.nenv):
        L = c.ins[e]["rne"]
        diff = sr.rne(c.V, L, True)["qfrc_bias"] - sr.rne(c.V, L)["qfrc_bias"]
        qM = sr.crb(c.V, L)["qM"] - np.diag(c.V["dof_armature"])
        want = qM @ np.asarray(L["qacc"], dtype=sr.HP)
        assert rel_err(f64(diff), f64(want)) <= TOL_PRE[c.dtype]
        got = f64(c.outs[e]["rne_acc"]["qfrc_bias"]) - f64(c.outs[e]["rne"]["qfrc_bias"])  # ... and so do the reference's recordings
        scale = max(np.abs(f64(c.outs[e]["rne_acc"]["qfrc_bias"])).max(), np.abs(f64(want)).max())
        assert np.abs(got - f64(want)).max() <= TOL_PRE[c.dtype] * scale


def test_the_launch_plan():
    """mjh_smooth_plan: lanes from nbody (factor_m: nv), whole environments in a 256-lane workgroup, the stated reals per environment; every model the goldens cover
    fits, centipede_83 in float64 and centipede_121 in float32 among them; a matrix past a CU's LDS is refused with the sizes."""
    r4 = lambda n: max(4, (n + 3) & ~3)
    for nb, nv, nt, dtype in ((3, 0, 0, F64), (14, 8, 0, F32), (20, 27, 0, F64), (74, 72, 0, F64), (85, 83, 0, F64), (123, 121, 0, F32), (6, 5, 2, F64), (200, 256, 3, F32)):
        want = dict(com_pos=10 * nb, crb=20 * nb + 12 * nv, tendon_armature=nt * nv, factor_m=((nv * (nv + 1) // 2 + 3) & ~3) + nv, com_vel=13 * nv, rne=24 * nb + 6 * nv)
        for op, reals in want.items():
            lanes, envs, lds = smooth.plan(op, nb, nv, nt, dtype)
            n = nv if op == "factor_m" else nb
            assert lanes == (16 if n <= 16 else 32 if n <= 32 else 64) and lds == r4(reals) and 1 <= envs <= 256 // lanes, (op, nb, nv)
            real = 8 if dtype == F64 else 4
            assert envs == max(1, min(256 // lanes, 64 * 1024 // (lds * real))) and lds * real <= 160 * 1024
            assert smooth.plan(smooth.OPS[op], nb, nv, nt, dtype) == (lanes, envs, lds)
    with pytest.raises(RuntimeError, match=r"factor_m: nbody = 300, nv = 256, ntendon = 0 .* need \d+ bytes of LDS"):
        smooth.plan("factor_m", 300, 256, 0, F64)
    lib, out = native.load_library(), (ctypes.c_int * 3)()
    assert lib.mjh_smooth_plan(6, 3, 3, 0, 8, out) == -22 and lib.mjh_smooth_plan(0, 3, 3, 0, 2, out) == -22 and lib.mjh_smooth_plan(0, 0, 3, 0, 8, out) == -22
    for xml, dtype in (("centipede_83", F64), ("centipede_121", F32)):
        lite = mt.mjcf.from_xml_path(mt.test_data_path(xml + ".xml"))
        for op in SIX:
            smooth.plan(op, int(lite.nbody), int(lite.nv), int(lite.ntendon), dtype)


@pytest.fixture(scope="module")
def rig():
    c = sr.case("pendula_f64")
    return c.model, c.data(2)


CALLS = dict(kinematics=mt.kinematics, com_pos=mt.com_pos, crb=mt.crb, tendon_armature=mt.tendon_armature, factor_m=mt.factor_m, com_vel=mt.com_vel, rne=mt.rne,
             rne_acc=lambda m, d: mt.rne(m, d, flg_acc=True))


@pytest.mark.parametrize("name", list(CALLS))
def test_cpu_data_is_refused(rig, name):
    mx, d = rig
    with pytest.raises(RuntimeError, match="HIP device"):
        CALLS[name](mx, d)


@pytest.mark.parametrize("name", list(CALLS))
def test_a_float32_data_on_a_float64_model_is_refused(rig, name):
    mx, d = rig
    with pytest.raises(ValueError, match=name.replace("_acc", "") + ".*dtype"):
        CALLS[name](mx, d.to(F32))


WRONG = dict(kinematics="qpos", com_pos="xanchor", crb="cdof", tendon_armature="ten_J", factor_m="qM", com_vel="cdof", rne="cvel", rne_acc="qacc")


@pytest.mark.parametrize("name", list(CALLS))
def test_a_wrong_trailing_shape_names_the_function_and_the_leaf(rig, name):
    mx, d = rig
    leaf = WRONG[name]
    with pytest.raises(ValueError, match=rf"{name.replace('_acc', '')}: {leaf} has shape"):
        CALLS[name](mx, d.replace(**{leaf: getattr(d, leaf)[:, :-1]}))
    if name == "com_pos":  # matrices may come flattened: the check passes, the device check refuses
        with pytest.raises(RuntimeError, match="HIP device"):
            mt.com_pos(mx, d.replace(ximat=d.ximat.reshape(2, -1, 9), xmat=d.xmat.reshape(2, -1, 9)))
        with pytest.raises(ValueError, match="com_pos: Model.body_mass has shape"):
            mt.com_pos(mx.replace(body_mass=mx.body_mass[:-1]), d)


@pytest.mark.parametrize("name", list(CALLS))
def test_vmap_is_refused_by_name(rig, name):
    mx, d = rig
    leaf = WRONG[name]
    fn = lambda t: getattr(CALLS[name](mx, d.replace(**{leaf: t})), sr.WRITES[name.replace("_acc", "")][0])
    with pytest.raises(NotImplementedError, match=name.replace("_acc", "")):
        torch.vmap(fn)(getattr(d, leaf))


def test_a_model_without_tendons_is_returned_as_it_is():
    c = sr.case("ant_f64")
    d = c.data(2)
    assert c.V["nt"] == 0 and mt.tendon_armature(c.model, d) is d
