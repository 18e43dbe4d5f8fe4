"""Dense models past 64 dofs (tools/gen_big_models.py): the code paths only they take are really taken, and the size envelope the LDS carve
allows is what the documentation states -- the largest model of each (dtype, solver, eulerdamp) steps and matches the oracle, one dof more is refused
on the host by ``mjh_model_create`` before anything launches, and the process keeps stepping valid models afterwards.

The family: a fixed hub with legs of hinge chains (centipede.xml's layout), nbody = nv + 2, 2 limit rows and 2 contacts per leg."""
import numpy as np
import pytest
import torch

import mujoco_torch_amd as mt
from _cases import TOL_PRE, TOL_SOL, seeded_batch, seeded_tol_sol
from _util import check_against_oracle, gpu_out_to_numpy, load_model
from mujoco_torch_amd import native

pytestmark = pytest.mark.gpu

LDS = 160 * 1024  # one CU
F64, F32 = torch.float64, torch.float32
EULERDAMP = 1 << 15  # a DisableBit
# (dtype, solver, eulerdamp) -> (largest model that builds, the next size up, option overrides that select the configuration).  Newton, and CG
# with eulerdamp on, keep the Hessian images H / HL (~1.5 nv^2 reals) in the solver arena (phase 4, qM already left in global memory), which binds
# first: 163008 B of 163840 at 83 dofs in float64, 163016 B at 121 in float32.  CG without eulerdamp drops them and the crb arena (phase 1:
# qMp + qLD + 20 nbody + 12 nv reals) binds instead: 106 dofs in float64, 154 in float32 (three 64-bit mask words from 129 on).
ENVELOPE = {
    (F64, "CG", True): ("centipede_83", "centipede_84", {"solver": 1}),
    (F64, "CG", False): ("centipede_106", "centipede_107", {}),
    (F64, "Newton", True): ("centipede_83", "centipede_84", {}),
    (F64, "Newton", False): ("centipede_83", "centipede_84", {"disableflags": EULERDAMP}),
    (F32, "CG", True): ("centipede_121", "centipede_122", {}),
    (F32, "CG", False): ("centipede_154", "centipede_155", {}),
    (F32, "Newton", True): ("centipede_121", "centipede_122", {"solver": 2}),
    (F32, "Newton", False): ("centipede_121", "centipede_122", {"solver": 2, "disableflags": EULERDAMP}),
}


def _lds(xml, dtype, overrides=None):
    mx = load_model(xml, overrides or {}, dtype)
    return mx, native.get_native_model(mx.to("cuda"), torch.device("cuda:0"), dtype).lds_bytes


# (xml, dtype, 64-bit mask words, the phase whose arena is within 4 KiB of 160 KiB or None)
PATH_CASES = [("centipede", F64, 2, None), ("centipede_83", F64, 2, 4), ("centipede_106", F64, 2, 1), ("centipede_84", F32, 2, None),
              ("centipede_121", F32, 2, 4), ("centipede_128", F32, 2, None), ("centipede_129", F32, 3, None), ("centipede_154", F32, 3, 1)]


@pytest.mark.parametrize("xml,dtype,words,binding", PATH_CASES, ids=[f"{c[0]}-{str(c[1])[6:]}" for c in PATH_CASES])
def test_large_models_take_the_paths_under_test(xml, dtype, words, binding):
    """The largest models sit within a few KB of a CU's 160 KiB in the arena that binds them (so the documented envelope is this carve's), the
    mask-word count nv implies is the one the model is meant to exercise (two up to dof 127, three from dof 128 on), whether the solver keeps
    an nv x nv copy of qM in LDS is what the carve's rule says, and a seeded batch carries active limit AND contact rows on each of three steps."""
    mx, lds = _lds(xml, dtype)
    nv, size = int(mx.nv), torch.finfo(dtype).bits // 8
    assert nv > 64 and (nv + 63) // 64 == words  # mask_words (mjhip.hip build())
    print(f"{xml} {str(dtype)[6:]}: nv {nv}, lds_bytes per phase {lds[:5]}, register solver {lds[5]}")
    assert max(lds[:5]) <= LDS
    if binding is not None:
        assert max(lds[:5]) == lds[binding] > LDS - 4 * 1024, lds
    ne, nf, nl, ncon, nefc = mx.constraint_sizes_py
    # sol_qm_lds: wanted whenever the solver iterates more than 4 times over rows, dropped when the arena with qMs would pass 160 KiB.  With
    # iterations = 4 it is off by rule, so the two arenas are equal exactly when the 50-iteration model dropped its copy too.
    assert int(mx.opt.iterations) > 4 and nefc > 0
    _, lds4 = _lds(xml, dtype, {"iterations": 4})
    qms = ((nv * nv + 1) & ~1) * size  # the carve's size of qMs (arrays padded to an even count of reals)
    kept = lds4[4] + qms <= LDS
    assert lds[4] == lds4[4] + (qms if kept else 0), (lds[4], lds4[4])
    if binding == 4 or xml == "centipede":
        assert not kept  # these models' solvers read qM from global memory
    if xml == "centipede_84":
        assert kept  # ... and this one's from LDS: the rule is not vacuous
    mx, d = seeded_batch(xml, {}, dtype, 7)
    mdev, dg = mx.to("cuda"), d.to("cuda")
    for s in range(3):
        dg = mt.step(mdev, dg)
        f = native.data_field_tensor(dg, "efc_force").cpu().numpy().reshape(7, -1)
        assert f.shape[1] == nefc and nl > 0 and ncon > 0
        assert np.abs(f[:, ne + nf: ne + nf + nl]).max() > 0, f"{xml} step{s}: no active limit row"
        assert np.abs(f[:, ne + nf + nl:]).max() > 0, f"{xml} step{s}: no active contact row"
        assert np.isfinite(native.data_field_tensor(dg, "qacc").cpu().numpy()).all()


@pytest.mark.parametrize("config", list(ENVELOPE), ids=[f"{str(c[0])[6:]}-{c[1]}-eulerdamp{'on' if c[2] else 'off'}" for c in ENVELOPE])
def test_size_envelope_and_its_refusal(config, oracle_lib):
    """The largest model of the configuration steps and matches the oracle; one dof more raises the host-side -12 refusal; a valid model still
    steps correctly afterwards."""
    dtype, solver, eulerdamp = config
    big, over, ov = ENVELOPE[config]
    mx, d = seeded_batch(big, ov, dtype, 3)
    assert int(mx.opt.solver) == (1 if solver == "CG" else 2) and bool(int(mx.opt.disableflags) & EULERDAMP) != eulerdamp
    out = mt.step(mx.to("cuda"), d.to("cuda"))
    check_against_oracle(mx, d, gpu_out_to_numpy(out), TOL_PRE[dtype], seeded_tol_sol(big, ov, dtype), what=f"{big} {config}", nthreads=4)
    mo = load_model(over, {"solver": int(mx.opt.solver), "disableflags": int(mx.opt.disableflags)}, dtype)
    assert int(mo.nv) == int(mx.nv) + 1
    with pytest.raises(RuntimeError, match=r"mjh_model_create failed \(-12\): model does not fit the 160 KiB LDS of one CU"):
        mt.step(mo.to("cuda"), mt.make_data(mo).expand(3).clone().to(dtype).to("cuda"))
    # the refusal leaves the process usable: a fresh model (centipede, Newton as its XML has it) builds, steps and matches
    mx, d = seeded_batch("centipede", {}, dtype, 3)
    out = mt.step(mx.to("cuda"), d.to("cuda"))
    check_against_oracle(mx, d, gpu_out_to_numpy(out), TOL_PRE[dtype], TOL_SOL[dtype], what=f"centipede after the refusal of {over}", nthreads=4)
