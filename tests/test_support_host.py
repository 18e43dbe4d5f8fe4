"""The support functions without a GPU: names, signatures and enums against the reference's (tests/golden/support/reference_api.json,
tools/gen_support_golden.py), shape and argument validation, the CPU refusal, full_m, and the C entry point."""
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import mujoco_torch_amd as mt
from _util import GOLD, load_model
from mujoco_torch_amd import native

API = json.load(open(os.path.join(GOLD, "support", "reference_api.json")))
FNS = ("jac", "apply_ft", "xfrc_accumulate", "full_m", "mul_m", "solve_m")


@pytest.mark.parametrize("name", FNS)
def test_public_with_the_reference_signature(name):
    assert hasattr(mt, name)
    assert list(inspect.signature(getattr(mt, name)).parameters) == API["signatures"][name]


@pytest.mark.parametrize("enum", ["SensorType", "ObjType", "ConstraintType", "WrapType"])
def test_enums_are_exported_with_the_reference_values(enum):
    E = getattr(mt, enum)
    for name, value in API["enums"][enum].items():
        assert int(E[name]) == value, (enum, name)
    if enum in ("ConstraintType", "WrapType"):
        assert {e.name: int(e) for e in E} == API["enums"][enum]


def test_entry_point_is_declared_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(native.HEADER).read(), flags=re.S)
    assert re.search(r"\bint mjh_support\s*\(const mjhModel\* m, const mjhSupportArgs\* args, void\* hip_stream\);", text)
    for i, n in enumerate(("JAC", "APPLY_FT", "XFRC", "MUL_M", "SOLVE_M")):
        assert re.search(rf"#define MJH_SUPPORT_{n} {i}\b", text) and re.search(rf"#define MJH_KERNEL_{n} {23 + i}\b", text)
    assert re.search(r"#define MJH_KERNEL_RENDER 22\b", text)
    if os.path.exists(native.LIB_PATH):
        assert hasattr(native.load_library(), "mjh_support")


@pytest.fixture(scope="module")
def hum():
    mx = load_model("humanoid")
    return mx, mt.make_data(mx).expand(4).clone()


def test_full_m_is_qM(hum):
    mx, d = hum
    assert mt.full_m(mx, d) is d.qM


def test_cpu_data_is_refused(hum):
    mx, d = hum
    with pytest.raises(RuntimeError, match="HIP device"):
        mt.jac(mx, d, torch.zeros(3, dtype=torch.float64), 3)
    with pytest.raises(RuntimeError, match="HIP device"):
        mt.apply_ft(mx, d, torch.ones(3), torch.ones(3), torch.zeros(3), [1, 2])
    with pytest.raises(RuntimeError, match="HIP device"):
        mt.xfrc_accumulate(mx, d)
    with pytest.raises(RuntimeError, match="HIP device"):
        mt.mul_m(mx, d, torch.ones(mx.nv, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="HIP device"):
        mt.solve_m(mx, d, torch.ones(4, 3, mx.nv, dtype=torch.float64))


@pytest.mark.parametrize("body_id", [-1, 17, [0, 17], torch.tensor(99), np.array([3, -2])])
def test_body_ids_out_of_range(hum, body_id):
    mx, d = hum
    with pytest.raises(ValueError, match="outside"):
        mt.jac(mx, d, torch.zeros(3), body_id)


@pytest.mark.parametrize("body_id", [torch.zeros(4, 1, dtype=torch.int64), [[1], [2], [3], [4]], torch.tensor(1.0), "torso", [], 2.0])
def test_per_environment_or_malformed_body_ids(hum, body_id):
    mx, d = hum
    with pytest.raises(ValueError):
        mt.jac(mx, d, torch.zeros(3), body_id)


def test_mapped_body_ids_are_refused(hum):
    mx, d = hum
    with pytest.raises(ValueError, match="vmap"):
        torch.vmap(lambda b: mt.jac(mx, d, torch.zeros(3), b)[0])(torch.tensor([1, 2]))


@pytest.mark.parametrize("shape", [(2,), (4, 2), (3, 3), (4, 2, 2), (5, 3), (4, 1, 1, 3)])
def test_bad_point_shapes(hum, shape):
    mx, d = hum
    with pytest.raises(ValueError, match="point"):
        mt.jac(mx, d, torch.zeros(shape), 1)


def test_query_counts_must_agree(hum):
    mx, d = hum
    with pytest.raises(ValueError, match="agree"):
        mt.jac(mx, d, torch.zeros(4, 5, 3), [1, 2])
    with pytest.raises(ValueError, match="agree"):
        mt.apply_ft(mx, d, torch.zeros(4, 2, 3), torch.zeros(4, 3, 3), torch.zeros(3), 1)
    with pytest.raises(ValueError, match="force"):
        mt.apply_ft(mx, d, torch.zeros(2), torch.zeros(3), torch.zeros(3), 1)


@pytest.mark.parametrize("fn", ["mul_m", "solve_m"])
@pytest.mark.parametrize("shape", [(26,), (4, 26), (27, 3), (4, 3, 27, 1), (3, 27)])
def test_bad_vector_shapes(hum, fn, shape):
    mx, d = hum
    with pytest.raises(ValueError):
        getattr(mt, fn)(mx, d, torch.zeros(shape, dtype=torch.float64))


def test_the_support_operator_traces_to_its_output_shapes(hum):
    """The fake implementation of support_leaves (what torch.compile traces) gives the shapes the docstrings state."""
    from torch._subclasses.fake_tensor import FakeTensorMode

    from mujoco_torch_amd import compile_op  # noqa: F401
    from mujoco_torch_amd.support import plan

    mx, d = hum
    nv = mx.nv
    with FakeTensorMode() as fm:
        cdof, com = fm.from_tensor(d.cdof), fm.from_tensor(d.subtree_com)
        assert plan(0, [cdof, com], [torch.zeros(3)], (1,), False)[3] == [(4, nv, 3)] * 2
        assert plan(0, [cdof, com], [torch.zeros(4, 3)], (1, 2, 3), True)[3] == [(4, 3, nv, 3)] * 2
        assert plan(1, [cdof, com], [torch.zeros(3), torch.zeros(4, 2, 3), torch.zeros(4, 3)], (5,), False)[3] == [(4, 2, nv)]
        assert plan(3, [fm.from_tensor(d.qM)], [torch.zeros(4, 3, nv)], (0,), False)[3] == [(4, 3, nv)]
        assert plan(4, [fm.from_tensor(d.qLD)], [torch.zeros(nv)], (0,), False)[3] == [(4, nv)]


# ---- the tests' own numpy reference (tests/_support_ref.py), pinned on the reference project's recorded outputs -----------------------

SUP_GOLD = os.path.join(GOLD, "support")
SUP_CASES = sorted(f[:-4] for f in os.listdir(SUP_GOLD) if f.endswith(".npz"))


def _within(got, want, allowed, what):
    """|got - want| <= allowed per element, the difference taken in the reference module's high precision."""
    import _support_ref as ref

    err = np.abs(np.asarray(got, dtype=ref.HP) - np.asarray(want, dtype=ref.HP)).astype(np.float64)
    allowed = np.asarray(allowed, dtype=np.float64)
    assert err.shape == allowed.shape, (what, err.shape, allowed.shape)
    over = err > allowed
    i = np.unravel_index(np.argmax(err - allowed), err.shape) if err.size else ()
    assert not over.any(), f"{what}: {int(over.sum())} of {err.size} elements beyond their bound; worst at {i}: error {err[i]:.3e}, bound {allowed[i]:.3e}"
    return float((err / np.maximum(allowed, 1e-300)).max(initial=0.0))


@pytest.mark.parametrize("case", SUP_CASES)
def test_the_numpy_reference_matches_the_recorded_outputs(case):
    """tests/_support_ref.py against the 7 goldens of the reference project, before it is trusted on the device.  jac_same (the same-dtype
    evaluation with the mask walked from body_parentid) reproduces the recorded jacp / jacr exactly; the high-precision functions agree with the
    recorded apply_ft / xfrc_accumulate / mul_m within (n + 2) eps S_abs, where n counts the terms of the element's sum plus the roundings its
    inputs have taken (apply_ft: 6 products of entries that carry JACP_ROUNDINGS = 4 roundings each, n = 10; xfrc_accumulate: the same over
    all bodies, n = 6 nbody + 4; mul_m: nv products of exact inputs, n = nv; jacp itself: 3 terms and the offset's rounding, n = 4; S_abs is
    formed from the unrounded high-precision elementary terms), and the recorded solve_m within the two-substitution residual bound and
    the forward bound it implies.  That the reference's own float32 and float64 results stay inside them is what makes the bounds usable on the device."""
    import _support_ref as ref

    assert len(SUP_CASES) == 7
    z = np.load(os.path.join(SUP_GOLD, case + ".npz"))
    meta = json.loads(str(z["meta"]))
    a = {k: np.stack([z[f"{e}/{k}"] for e in range(meta["nenv"])]) for k in sorted({f.split("/", 1)[1] for f in z.files if "/" in f})}
    dtype = getattr(torch, meta["dtype"])
    eps = torch.finfo(dtype).eps
    mx = load_model(meta["xml"], dtype=dtype)
    nv, nb, ids = int(mx.nv), int(mx.nbody), meta["body_id"]
    assert (nv, nb) == (meta["nv"], meta["nbody"]) and a["cdof"].dtype == np.dtype(meta["dtype"])
    root = np.asarray(mx.body_rootid)
    mask = ref.ancestor_mask(mx.body_parentid, mx.dof_bodyid)
    assert mask.shape == (nb, nv) and not mask[0].any()
    geo = (a["cdof"], a["subtree_com"], root, mask)

    jp, jr = ref.jac_same(*geo, a["point"], ids)
    assert jp.dtype == a["jacp"].dtype and np.array_equal(jp, a["jacp"]) and np.array_equal(jr, a["jacr"]), case
    (hp, ap), (hr, ar) = ref.jac_hp(*geo, a["point"], ids)
    _within(a["jacp"], hp, ref.bound(4, eps, ap), f"{case} jacp")
    assert np.array_equal(np.asarray(a["jacr"], dtype=ref.HP), hr)  # a copy of cdof or zero: no rounding at all

    val, s = ref.apply_ft_hp(*geo, a["point"], a["force"], a["torque"], ids)
    _within(a["apply_ft"], val, ref.bound(6 + ref.JACP_ROUNDINGS, eps, s), f"{case} apply_ft")
    val, s = ref.xfrc_hp(a["cdof"], a["subtree_com"], a["xipos"], a["xfrc_applied"], root, mask)
    _within(a["xfrc_accumulate"], val, ref.bound(6 * nb + ref.JACP_ROUNDINGS, eps, s), f"{case} xfrc_accumulate")
    val, s = ref.mul_m_hp(a["qM"], a["vec"])
    _within(a["mul_m"], val, ref.bound(nv, eps, s), f"{case} mul_m")

    res, scale = ref.solve_m_residual(a["qLD"], a["vec"], a["solve_m"])
    _within(res, np.zeros_like(res), ref.solve_m_factor(nv, eps) * scale, f"{case} solve_m residual")
    x, _ = ref.solve_m_hp(a["qLD"], a["vec"])
    _within(a["solve_m"], x, ref.solve_m_forward_bound(a["qLD"], a["solve_m"], eps), f"{case} solve_m")
    res, scale = ref.solve_m_residual(a["qLD"], a["vec"], x)  # ... and the substitution of the reference module solves the system it states
    _within(res, np.zeros_like(res), ref.solve_m_factor(nv, ref.EPS_HP) * scale, f"{case} solve_m_hp residual")
