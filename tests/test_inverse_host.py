"""Inverse dynamics without a GPU: the public API and the C entry point exist, the written-leaf set follows the reference, and the golden fixtures
(tests/golden/inverse/) are what their generator (tools/gen_inverse_golden.py) makes."""
import inspect
import json
import os
import re
import sys

import numpy as np
import pytest

import mujoco_torch_amd as mt
from _util import GOLD, load_model
from mujoco_torch_amd import native
from mujoco_torch_amd.forward import _inverse_names

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV_GOLD = os.path.join(GOLD, "inverse")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_inverse_golden as gen  # noqa: E402


def test_inverse_is_public_with_the_reference_signature():
    assert callable(mt.inverse)
    assert list(inspect.signature(mt.inverse).parameters) == ["m", "d"]


def test_entry_point_and_flag_are_declared():
    text = re.sub(r"/\*.*?\*/", "", open(native.HEADER).read(), flags=re.S)
    assert re.search(r"\bint mjh_inverse\s*\(const mjhModel\* m, const mjhData\* in, mjhData\* out, void\* qfrc_inverse, void\* work, int64_t B, int flags,", text)
    assert int(re.search(r"#define MJH_FLAG_INV_DISCRETE (\d+)", text).group(1)) == native.FLAG_INV_DISCRETE
    if os.path.exists(native.LIB_PATH):
        assert hasattr(native.load_library(), "mjh_inverse")


def test_written_leaves_follow_the_reference():
    """inverse() runs _position, _velocity, the sensors and inv_constraint: no actuation, acceleration or solver leaf, qfrc_constraint always."""
    skip = {"actuator_force", "qfrc_actuator", "qfrc_smooth", "qacc_smooth", "qacc", "act_dot", "qacc_warmstart"}
    ant = _inverse_names(load_model("ant"))
    assert not skip & set(ant)
    assert {"efc_J", "efc_D", "efc_aref", "efc_force", "efc_frictionloss", "qfrc_constraint", "qfrc_bias", "qfrc_passive", "qM", "qLD", "contact_dist"} <= set(ant)
    cartpole = _inverse_names(load_model("cartpole"))
    assert "qfrc_constraint" in cartpole and "efc_force" not in cartpole and not skip & set(cartpole)


def test_golden_meta_matches_the_generator():
    files = sorted(f[:-4] for f in os.listdir(INV_GOLD) if f.endswith(".npz"))
    assert files == sorted(gen.CASES)
    for case, (xml, overrides, dtype, nenv, recipe) in gen.CASES.items():
        path = os.path.join(INV_GOLD, case + ".npz")
        assert os.path.getsize(path) < 1 << 20, case
        meta = json.loads(str(np.load(path)["meta"]))
        assert (meta["xml"], meta["overrides"], meta["dtype"], meta["nenv"], meta["recipe"], meta["noise"]) == (xml, overrides, dtype, nenv, recipe, gen.NOISE), case
        assert 4 <= nenv <= 8


def test_generator_reproduces_the_fixtures(tmp_path):
    """The reference's inverse, run again here, gives the committed arrays bit for bit."""
    import ref_harness

    if not ref_harness.available():
        pytest.skip("the reference tree is not present")
    gen.main(out_dir=str(tmp_path))
    for case in gen.CASES:
        a, b = np.load(os.path.join(INV_GOLD, case + ".npz")), np.load(os.path.join(tmp_path, case + ".npz"))
        assert sorted(a.files) == sorted(b.files), case
        for k in a.files:
            if k == "meta":
                ma, mb = json.loads(str(a[k])), json.loads(str(b[k]))
                ma.pop("torch"), mb.pop("torch")
                assert ma == mb, case
            else:
                assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), (case, k)
