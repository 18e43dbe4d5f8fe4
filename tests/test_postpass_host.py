"""The host path the functions on a finished pass share (``mujoco_torch_amd/_postpass.py``), without a GPU: the caches, ``bind``, and the order of events of the
six entry points that take an args struct, on the CPU stand-in of the device library (tests/_hostsim.py), which exports none of them.

What each module refuses, message by message, is asserted by its own host suite (test_support_host.py, test_postconstraint_host.py,
test_contact_sensors_host.py, test_energy_host.py, test_integrator_host.py, test_jacobian_host.py); none of them reaches the library lookup, which is what
``test_a_valid_call_reaches_the_library_lookup`` adds."""
import ctypes
import types

import numpy as np
import pytest
import torch

import _hostsim
import mujoco_torch_amd as mt
from _util import load_model
from mujoco_torch_amd import _postpass as pp
from mujoco_torch_amd import native

CPU, META = torch.device("cpu"), torch.device("meta")


@pytest.fixture
def hostsim(monkeypatch):
    return _hostsim.install(monkeypatch)


@pytest.fixture(scope="module")
def hum():
    mx = load_model("humanoid")
    return mx, mt.make_data(mx).expand(2).clone()


def model(uid):
    return types.SimpleNamespace(tables=types.SimpleNamespace(uid=uid))


# ---- the caches --------------------------------------------------------------------------------------------------------------------------

def test_cached_makes_once_and_is_bounded():
    cache, made = {}, []
    make = lambda: made.append(1) or object()
    first = pp.cached(cache, "a", make, limit=2)
    assert pp.cached(cache, "a", make, limit=2) is first and len(made) == 1
    assert pp.cached(cache, "a", make, valid=lambda hit: False, limit=2) is not first and len(made) == 2
    pp.cached(cache, "b", make, limit=2)
    pp.cached(cache, "c", make, limit=2)
    assert sorted(cache) == ["a", "b", "c"]
    pp.cached(cache, "d", make, limit=2)  # (past the limit: emptied, then filled)
    assert sorted(cache) == ["d"]


def test_upload_keeps_a_value_until_its_bytes_change():
    m = model("upload-test-1")
    a = pp.upload(m, "body_mass", np.array([1.0, 2.0, 3.0]), torch.float64, CPU)
    assert a.dtype == torch.float64 and a.device == CPU and a.is_contiguous() and a.tolist() == [1.0, 2.0, 3.0]
    assert pp.upload(m, "body_mass", [1.0, 2.0, 3.0], torch.float64, CPU) is a  # (the same values, another container)
    assert pp.upload(m, "body_mass", np.array([1, 2, 3], dtype=np.int32), torch.float64, CPU) is a
    b = pp.upload(m, "body_mass", np.array([1.0, 2.5, 3.0]), torch.float64, CPU)
    assert b is not a and b.tolist() == [1.0, 2.5, 3.0] and a.tolist() == [1.0, 2.0, 3.0]
    assert pp.upload(m, "body_mass", np.array([1.0, 2.5, 3.0]), torch.float64, CPU) is b


def test_upload_keys_do_not_collide():
    m, other = model("upload-test-2"), model("upload-test-3")
    v = np.array([4.0, 5.0])
    base = pp.upload(m, "jnt_margin", v, torch.float64, CPU)
    by_name = pp.upload(m, "jnt_stiffness", v + 1, torch.float64, CPU)
    by_dtype = pp.upload(m, "jnt_margin", v + 2, torch.float32, CPU)
    by_device = pp.upload(m, "jnt_margin", v + 3, torch.float64, META)
    by_model = pp.upload(other, "jnt_margin", v + 4, torch.float64, CPU)
    assert by_dtype.dtype == torch.float32 and by_device.device == META
    assert len({id(t) for t in (base, by_name, by_dtype, by_device, by_model)}) == 5
    assert pp.upload(m, "jnt_margin", v, torch.float64, CPU) is base and base.tolist() == [4.0, 5.0]  # (none of them replaced it)
    assert pp.upload(m, "jnt_stiffness", v + 1, torch.float64, CPU) is by_name and by_name.tolist() == [5.0, 6.0]
    assert pp.upload(m, "jnt_margin", v + 2, torch.float32, CPU) is by_dtype and by_dtype.tolist() == [6.0, 7.0]
    assert pp.upload(m, "jnt_margin", v + 3, torch.float64, META) is by_device
    assert pp.upload(other, "jnt_margin", v + 4, torch.float64, CPU) is by_model and by_model.tolist() == [8.0, 9.0]


def test_model_value_converts_a_tensor_and_uploads_a_host_value():
    m = model("upload-test-4")
    t = torch.arange(6, dtype=torch.float32).reshape(2, 3).t().requires_grad_()
    got = pp.model_value(m, "x", t, torch.float64, CPU)
    assert got.dtype == torch.float64 and got.is_contiguous() and not got.requires_grad and torch.equal(got, t.detach().double())
    host = pp.model_value(m, "x", [1.0, 2.0], torch.float64, CPU)
    assert pp.model_value(m, "x", (1.0, 2.0), torch.float64, CPU) is host


# ---- bind --------------------------------------------------------------------------------------------------------------------------------

def test_bind_skips_empty_tensors_and_keeps_contiguous_copies():
    a = native.ARGS["mjh_energy"](flags=3, B=2)
    plain = torch.arange(6.0)
    strided = torch.arange(12.0).reshape(3, 4).t()
    assert not strided.is_contiguous()
    pp.bind(a, dict(qpos=torch.empty(0), xipos=plain, qM=strided, sns=torch.empty((0, 4), dtype=torch.int32)))
    assert a.qpos is None and a.sns is None  # (NULL)
    assert a.xipos == plain.data_ptr()
    assert a.qM not in (None, strided.data_ptr())
    copies = [t for t in a._keep if t.data_ptr() == a.qM]  # (the struct itself holds what it points to)
    assert len(copies) == 1 and copies[0].is_contiguous() and torch.equal(copies[0], strided)
    assert any(t is plain for t in a._keep)
    assert (a.flags, a.B) == (3, 2) and a.qvel is None
    pp.bind(a, dict(qvel=plain))  # (a second call adds to what is kept)
    assert a.qvel == plain.data_ptr() and any(t.data_ptr() == a.qM for t in a._keep)


# ---- the order of events on the stand-in library -----------------------------------------------------------------------------------------

CALLS = {
    "mjh_support": (lambda m, d: mt.jac(m, d, torch.zeros(3, dtype=torch.float64), 1), lambda d: d.replace(cdof=d.cdof[..., :5]),
                    "predates the support functions", "cdof / subtree_com have shapes"),
    "mjh_postconstraint": (lambda m, d: mt.fwd_postconstraint(m, d), lambda d: d.replace(cinert=d.cinert[..., :9]), "predates fwd_postconstraint",
                           "fwd_postconstraint: cinert has shape"),
    "mjh_contact_sensors": (lambda m, d: mt.contact_force(m, d), lambda d: d.replace(efc_force=d.efc_force[..., :-1]), "predates contact_force",
                            "contact_force: efc_force has shape"),
    "mjh_energy": (lambda m, d: mt.energy(m, d), lambda d: d.replace(qM=d.qM[..., :-1]), "predates energy", "energy: qM has shape"),
    "mjh_integrate": (lambda m, d: mt.implicit(m, d), lambda d: d.replace(qfrc_smooth=d.qfrc_smooth[..., :-1]), "predates implicit",
                      "implicit: qfrc_smooth has shape"),
    "mjh_jacobian": (lambda m, d: mt.angmom_mat(m, d, 1), lambda d: d.replace(ximat=d.ximat[..., :2, :]), "predates angmom_mat", "angmom_mat: ximat has shape"),
}


def test_the_table_covers_every_args_struct_entry_point():
    assert sorted(CALLS) == sorted(native.ARGS)


@pytest.mark.parametrize("symbol", sorted(CALLS))
def test_a_valid_call_reaches_the_library_lookup(hostsim, hum, symbol):
    """Past every check and ``_require_device``, a call on a library without its entry point says which one is missing."""
    mx, d = hum
    run, _, what, _ = CALLS[symbol]
    with pytest.raises(RuntimeError, match=rf"{what} \(no {symbol}\): rebuild the library") as exc:
        run(mx, d)
    assert str(exc.value).startswith(native.LIB_PATH)


@pytest.mark.parametrize("symbol", sorted(CALLS))
def test_a_wrong_leaf_shape_is_refused_before_the_library_lookup(hostsim, hum, symbol):
    mx, d = hum
    run, spoil, _, message = CALLS[symbol]
    with pytest.raises(ValueError, match=message):
        run(mx, spoil(d))


def test_without_the_stand_in_the_device_check_comes_before_the_library(hum):
    mx, d = hum
    with pytest.raises(RuntimeError, match="run only on a HIP device"):
        mt.energy(mx, d)


def test_an_empty_batch_touches_no_library(hostsim, hum):
    mx, d = hum
    empty = mt.make_data(mx).expand(0).clone()
    out = mt.energy(mx, empty)
    assert tuple(out.shape) == (0, 2)
    assert tuple(mt.contact_force(mx, empty).shape) == (0, int(mx.constraint_sizes_py[3]), 6)


def test_call_passes_the_struct_and_reports_a_failure(hostsim, hum, monkeypatch):
    """``call`` on a stand-in that does export the symbol: the handle, the filled struct and the stream arrive; a non-zero return is today's RuntimeError."""
    mx, d = hum
    seen = []

    def mjh_energy(self, handle, args, stream):
        a = ctypes.cast(args, ctypes.POINTER(native.EnergyArgs)).contents
        seen.append((a.flags, a.B, a.xipos, a.energy, stream.value))
        return 0

    monkeypatch.setattr(_hostsim._Lib, "mjh_energy", mjh_energy, raising=False)
    out = mt.energy(mx, d)
    assert tuple(out.shape) == (2, 2)
    assert seen == [(3, 2, d.xipos.data_ptr(), out.data_ptr(), None)]  # (a CPU tensor's stream is the null stream)
    monkeypatch.setattr(_hostsim._Lib, "mjh_energy", lambda self, handle, args, stream: -22, raising=False)
    with pytest.raises(RuntimeError, match=r"native energy_vel failed \(-22\): hostsim"):
        mt.energy_vel(mx, d)
