"""Inverse dynamics on the GPU: ``mujoco_torch_amd.inverse`` against the reference's own ``inverse`` (tests/golden/inverse/, tools/gen_inverse_golden.py)
and the properties that hold without a reference: forward-then-inverse gives back the applied forces, the discrete round trip of an Euler step, the
vmap / compile operator, batch shapes, no mutation of the input, and batches cut into several launches."""
import json
import os

import numpy as np
import pytest
import torch

import mujoco_torch_amd as mt
from _cases import TOL_PRE
from _util import GOLD, INT_LEAVES, REAL_LEAVES, load_model, rel_err, solver_floor
from mujoco_torch_amd import native
from mujoco_torch_amd.forward import _inverse_names

pytestmark = pytest.mark.gpu

INV_GOLD = os.path.join(GOLD, "inverse")
INV_CASES = sorted(f[:-4] for f in os.listdir(INV_GOLD) if f.endswith(".npz"))
INVDISCRETE = int(mt.EnableBit.INVDISCRETE)


def _leaf(d, n):
    return d.qfrc_inverse if n == "qfrc_inverse" else native.data_field_tensor(d, n)


def _load(case):
    z = np.load(os.path.join(INV_GOLD, case + ".npz"))
    meta = json.loads(str(z["meta"]))
    dtype = getattr(torch, meta["dtype"])
    mx = load_model(meta["xml"], meta["overrides"], dtype, keep_sensors=meta["keep_sensors"])
    return z, meta, dtype, mx


def _input(z, mx, dtype, env):
    """The recorded input Data of one environment: every ABI leaf and the input-only sensor leaves."""
    d = mt.make_data(mx)
    if dtype != torch.float64:
        d = d.to(dtype)
    top, con = {}, {}
    for n in REAL_LEAVES + INT_LEAVES:
        path = native.DATA_PATH[n]
        t = torch.from_numpy(z[f"in/{env}/{n}"].copy())  # (dtypes as the Data schema has them: the reference's forward leaves some all-zero leaves of models without actuators in float32)
        t = t.to(torch.int32 if n in native.LISTS["MJH_DATA_I32"] else (torch.int64 if n in INT_LEAVES else dtype))
        (con if len(path) == 2 else top)[path[-1]] = t
    for n in native.LISTS["MJH_DATA_EXTRA_IN"]:
        top[n] = torch.from_numpy(z[f"in/{env}/{n}"].copy())
    return d.replace(contact=d.contact.replace(**con), **top)


def _batch(z, meta, mx, dtype):
    return torch.stack([_input(z, mx, dtype, e) for e in range(meta["nenv"])])


TAIL = ("efc_force", "qfrc_constraint", "qfrc_inverse")


def _err(n, got, want, efc_force):
    # qfrc_constraint = J^T efc_force, and qfrc_inverse with it, can cancel to rounding residue: read on the scale of the forces they are made of (_util.solver_floor)
    return rel_err(got, want, solver_floor("qfrc_constraint", {"efc_force": efc_force}) if n in ("qfrc_constraint", "qfrc_inverse") else 1e-6)


def _tail_of(mx, g, qacc, discrete):
    """inverse.py's tail in numpy (float64) on a result's own position / velocity leaves: what the kernel must compute from them."""
    nv = int(mx.nv)
    ne, nf = mx.constraint_sizes_py[:2]
    qM = g["qM"].reshape(nv, nv).astype(np.float64)
    q = qacc.astype(np.float64)
    if discrete:
        L = g["qLD"].reshape(nv, nv).astype(np.float64)
        rhs = qM @ q + float(mx.opt.timestep) * mx.dof_damping.double().cpu().numpy() * q
        q = np.linalg.solve(L.T, np.linalg.solve(L, rhs))
    J = g["efc_J"].reshape(-1, nv).astype(np.float64)
    jaref = J @ q - g["efc_aref"].astype(np.float64)
    active = (jaref < 0) | (np.arange(J.shape[0]) < ne + nf)
    f = g["efc_D"].astype(np.float64) * -jaref * active
    qc = J.T @ f
    return {"efc_force": f, "qfrc_constraint": qc, "qfrc_inverse": g["qfrc_bias"] + qM @ q - g["qfrc_passive"] - qc}


@pytest.mark.parametrize("case", INV_CASES)
def test_inverse_matches_reference_golden(case, oracle_lib):
    """Every leaf the reference's inverse writes, qfrc_inverse included, per environment; integer contact leaves bit for bit; every other leaf is the
    caller's tensor itself.  An environment whose narrow phase meets a degenerate pair (coincident capsule axes: an index tie the implementation's
    rounding decides) is checked the way the step goldens are: its position / velocity leaves against the oracle's admissible outcome, its inverse tail
    against inverse.py's formulas on its own leaves."""
    import pyoracle

    z, meta, dtype, mx = _load(case)
    dg = _batch(z, meta, mx, dtype).to("cuda")
    out = mt.inverse(mx.to("cuda"), dg)
    written = _inverse_names(mx) + ["qfrc_inverse"]
    tol = TOL_PRE[dtype]
    discrete = bool(int(mx.opt.enableflags) & INVDISCRETE) and int(mx.opt.integrator) == 0 and not (int(mx.opt.disableflags) & (1 << 15))
    via_oracle = 0
    for e in range(meta["nenv"]):
        got = {n: _leaf(out, n)[e].cpu().numpy() for n in written}
        for n in written:
            if n in INT_LEAVES:
                assert np.array_equal(got[n], z[f"out/{e}/{n}"]), (case, e, n)
        bad = [n for n in written if n not in INT_LEAVES and not _err(n, got[n], z[f"out/{e}/{n}"], z[f"out/{e}/efc_force"]) <= tol]
        if not bad:
            continue
        via_oracle += 1
        d1 = _input(z, mx, dtype, e)
        hint = {k: got[k] for k in ("contact_dist", "contact_pos", "contact_frame")} if mx.constraint_sizes_py[3] > 0 else None
        o = pyoracle.run(mx, d1, step=False, stages=0x1F, **({"contact_hint": hint} if hint else {}))
        pre = [n for n in written if n not in TAIL and n not in INT_LEAVES and n != "sensordata"]
        worst = max(rel_err(got[n], o[n]) for n in pre)
        assert worst <= tol, (case, e, bad, worst)
        tail = _tail_of(mx, got, z[f"in/{e}/qacc"], discrete)
        for n in TAIL:
            if got[n].size:
                err = _err(n, got[n], tail[n], got["efc_force"] if "efc_force" in got else np.zeros(0))
                assert err <= tol, (case, e, n, err)
    assert via_oracle <= meta["nenv"] // 2, (case, via_oracle)
    for n in REAL_LEAVES + INT_LEAVES:
        if n in written:
            continue
        t_in, t_out = native.data_field_tensor(dg, n), native.data_field_tensor(out, n)
        assert t_out.data_ptr() == t_in.data_ptr() or t_in.numel() == 0, n
        for e in range(meta["nenv"]):
            assert np.array_equal(t_out[e].cpu().numpy(), z[f"out/{e}/{n}"]), (case, e, n)  # ... and what the reference left there


def _random_state(mx, B, seed, push=0.0):
    rng = np.random.RandomState(seed)
    q = np.tile(mx.qpos0.cpu().numpy(), (B, 1))
    q[:, 7:] += 0.3 * rng.randn(B, mx.nq - 7)
    q[:, 2] -= push * rng.rand(B)
    return mt.make_data(mx).expand(B).clone().replace(
        qpos=torch.tensor(q), qvel=torch.tensor(0.5 * rng.randn(B, mx.nv)), ctrl=torch.tensor(np.clip(0.7 * rng.randn(B, mx.nu), -1, 1)),
        qfrc_applied=torch.tensor(0.5 * rng.randn(B, mx.nv)))


def _per_env_err(got, want):
    got, want = got.double().cpu().numpy(), want.double().cpu().numpy()
    return np.array([rel_err(g, w, floor=1.0) for g, w in zip(got, want)])


def test_forward_then_inverse_gives_back_the_applied_forces():
    """A converged Newton solve (100 iterations, tight tolerance): inverse(forward(d)) = qfrc_applied + qfrc_actuator (xfrc_applied = 0), every environment."""
    mx = load_model("humanoid", {"solver": 2, "iterations": 100, "ls_iterations": 50, "tolerance": 1e-12})
    B = 4096
    d = _random_state(mx, B, 11, push=0.08)
    mdev = mx.to("cuda")
    f = mt.forward(mdev, d.to("cuda"))
    inv = mt.inverse(mdev, f)
    err = _per_env_err(inv.qfrc_inverse, f.qfrc_applied + f.qfrc_actuator)
    assert int(f.nefc) > 0 and float(f.efc_force.abs().max()) > 0
    assert err.max() <= 1e-6, (err.max(), int(err.argmax()))


def test_discrete_round_trip_of_an_euler_step():
    """step, then qacc = (qvel' - qvel) / h, then inverse with INVDISCRETE gives back qfrc_applied + qfrc_actuator; without the flag it does not."""
    mx = load_model("halfcheetah")
    assert int(mx.opt.integrator) == 0 and float(mx.dof_damping.abs().max()) > 0
    B = 4096
    rng = np.random.RandomState(12)
    d = mt.make_data(mx).expand(B).clone().replace(
        qpos=torch.tensor(mx.qpos0.cpu().numpy() + 0.1 * rng.randn(B, mx.nq)), qvel=torch.tensor(0.5 * rng.randn(B, mx.nv)),
        ctrl=torch.tensor(np.clip(0.7 * rng.randn(B, mx.nu), -1, 1)), qfrc_applied=torch.tensor(0.5 * rng.randn(B, mx.nv)))
    mdev = mx.to("cuda")
    dg = d.to("cuda")
    s = mt.step(mdev, dg)
    h = float(mx.opt.timestep)
    dq = dg.replace(qacc=(s.qvel - dg.qvel) / h)
    want = dg.qfrc_applied + s.qfrc_actuator
    mdisc = mdev.replace(opt=mdev.opt.replace(enableflags=int(mdev.opt.enableflags) | INVDISCRETE))
    err = _per_env_err(mt.inverse(mdisc, dq).qfrc_inverse, want)
    assert err.max() <= 1e-9, err.max()
    err_cont = _per_env_err(mt.inverse(mdev, dq).qfrc_inverse, want)
    assert err_cont.max() > 1e-2, err_cont.max()


def _golden_batch(case):
    z, meta, dtype, mx = _load(case)
    return mx, _batch(z, meta, mx, dtype).to("cuda"), (z, dtype)


@pytest.mark.parametrize("case", ["humanoid_newton_f64", "sensor_rig2_f64", "halfcheetah_discrete_f64"])
def test_vmap_and_compile_are_the_direct_batch(case):
    """``torch.vmap(mt.inverse, in_dims=(None, 0))`` and its ``torch.compile`` go through ONE ``inverse_leaves`` call: bit-identical to the direct batched call."""
    mx, dg, _ = _golden_batch(case)
    mdev = mx.to("cuda")
    want = mt.inverse(mdev, dg)
    names = _inverse_names(mx) + ["qfrc_inverse"]
    mapped = torch.vmap(mt.inverse, in_dims=(None, 0))(mdev, dg)
    compiled = torch.compile(torch.vmap(lambda y: mt.inverse(mdev, y)), fullgraph=True)(dg)
    for got in (mapped, compiled):
        for n in names:
            assert torch.equal(_leaf(got, n), _leaf(want, n)), n
        assert torch.equal(got.qacc, dg.qacc)


def test_batch_shapes_agree():
    """Unbatched (one environment), (B,) and (2, B / 2) give the same numbers."""
    mx, dg, (z, dtype) = _golden_batch("ant_ell_f64")
    mdev = mx.to("cuda")
    B = dg.qpos.shape[0]
    want = mt.inverse(mdev, dg)
    two = mt.inverse(mdev, torch.stack([dg[: B // 2], dg[B // 2:]]))
    assert tuple(two.qfrc_inverse.shape) == (2, B // 2, mx.nv)
    names = _inverse_names(mx) + ["qfrc_inverse"]
    for n in names:
        assert torch.equal(_leaf(two, n).reshape(_leaf(want, n).shape), _leaf(want, n)), n
    for e in (0, B - 1):
        one = mt.inverse(mdev, _input(z, mx, dtype, e).to("cuda"))
        assert tuple(one.qfrc_inverse.shape) == (mx.nv,)
        for n in names:
            assert torch.equal(_leaf(one, n), _leaf(want, n)[e]), (e, n)


def test_the_input_is_not_mutated():
    mx, dg, _ = _golden_batch("sensor_rig2_f64")
    before = {n: native.data_field_tensor(dg, n).clone() for n in REAL_LEAVES + INT_LEAVES}
    qinv = dg.qfrc_inverse.clone()
    out = mt.inverse(mx.to("cuda"), dg)
    for n, t in before.items():
        assert torch.equal(native.data_field_tensor(dg, n), t), n
    assert torch.equal(dg.qfrc_inverse, qinv)
    assert out.qfrc_inverse.data_ptr() != dg.qfrc_inverse.data_ptr()


def test_rk4_discrete_raises_and_cpu_tensors_are_rejected():
    mx = load_model("ant", {"integrator": 1})
    d = mt.make_data(mx).expand(4).clone()
    mdev = mx.to("cuda")
    mdisc = mdev.replace(opt=mdev.opt.replace(enableflags=INVDISCRETE))
    with pytest.raises(RuntimeError, match="discrete inverse dynamics is not supported by RK4 integrator"):
        mt.inverse(mdisc, d.to("cuda"))
    assert mt.inverse(mdev, d.to("cuda")).qfrc_inverse.shape == (4, mx.nv)  # continuous inverse of the same RK4 model
    with pytest.raises(RuntimeError, match="HIP device"):
        mt.inverse(mx, d)


def test_batches_past_one_launch_are_cut_on_the_host():
    """MJH_MAX_GRID_LOG2=3 caps a launch at 8 workgroups: a batch of 203 environments runs the inverse tail (and the forward prefix and sensors before it) in
    several launches, bit-identical to one launch -- including the largest bundled model (centipede, 72 dofs: 64 lanes per environment)."""
    import subprocess
    import sys
    import tempfile

    code = r'''
import sys
sys.path.insert(0, "tests"); sys.path.insert(0, "mujoco-torch_amd"); sys.path.insert(0, "oracle")
import numpy as np, torch, mujoco_torch_amd as mt
from mujoco_torch_amd import native
from mujoco_torch_amd.forward import _inverse_names
from _util import load_model
out = {}
for xml, ov, dt in (("humanoid", {}, torch.float64), ("ant", {"cone": 1}, torch.float32), ("sensor_rig2", {}, torch.float64), ("halfcheetah", {"enableflags": 8}, torch.float64),
                    ("centipede", {}, torch.float64), ("mesh_contact", {}, torch.float32)):
    mx = load_model(xml, ov, dt)
    B = 203
    rng = np.random.RandomState(0)
    d = mt.make_data(mx).expand(B).clone().replace(qvel=torch.tensor(0.05 * rng.randn(B, mx.nv)), qacc=torch.tensor(rng.randn(B, mx.nv)))
    if dt != torch.float64: d = d.to(dt)
    got = mt.inverse(mx.to("cuda"), d.to("cuda"))
    out[xml] = {n: (got.qfrc_inverse if n == "qfrc_inverse" else native.data_field_tensor(got, n)).cpu() for n in _inverse_names(mx) + ["qfrc_inverse"]}
torch.save(out, sys.argv[1])
print("ran")
'''
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as td:
        res = {}
        for tag, env in (("one", {}), ("cut", {"MJH_MAX_GRID_LOG2": "3"})):
            f = os.path.join(td, tag + ".pt")
            r = subprocess.run([sys.executable, "-c", code, f], cwd=root, env=dict(os.environ, **env), capture_output=True, text=True, timeout=900)
            assert r.returncode == 0 and "ran" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
            res[tag] = torch.load(f)
    for case in res["one"]:
        for n, t in res["one"][case].items():
            assert torch.equal(t, res["cut"][case][n]) or (t.is_floating_point() and torch.equal(torch.nan_to_num(t), torch.nan_to_num(res["cut"][case][n]))), (case, n)


LARGE_INV = [("centipede_83", torch.float64, False), ("centipede_83", torch.float64, True), ("centipede_121", torch.float32, False), ("centipede_121", torch.float32, True),
             ("centipede_106", torch.float64, False), ("centipede_154", torch.float32, False)]


@pytest.mark.parametrize("xml,dtype,discrete", LARGE_INV, ids=[f"{x[10:]}-{str(t)[6:]}-{'discrete' if dc else 'continuous'}" for x, t, dc in LARGE_INV])
def test_large_models_against_the_oracle_and_the_tail_formulas(xml, dtype, discrete, oracle_lib):
    """The largest dense models that build (tests/test_big_models.py): 64 lanes per environment and an LDS chunk of far fewer rows than nv
    (16 of 83 and 12 of 106 in float64, 24 of 121 and 18 of 154 in float32).  The forward prefix (stages 0x1F) against the oracle; efc_force,
    qfrc_constraint and qfrc_inverse against inverse.py's formulas in float64 on the kernel's own leaves, with and without the discrete re-solve
    (Euler, eulerdamp on, damped joints: the two largest models disable eulerdamp, the discrete case runs on their eulerdamp twins)."""
    import pyoracle

    mx = load_model(xml, {"enableflags": INVDISCRETE} if discrete else {}, dtype)
    assert int(mx.opt.integrator) == 0 and float(mx.dof_damping.abs().min()) > 0
    assert not discrete or not (int(mx.opt.disableflags) & (1 << 15))
    B = 5
    rng = np.random.RandomState(7)
    d = mt.make_data(mx).expand(B).clone().replace(
        qpos=torch.tensor(mx.qpos0.cpu().numpy() + 0.5 * rng.randn(B, mx.nq)), qvel=torch.tensor(0.5 * rng.randn(B, mx.nv)),
        qacc=torch.tensor(5.0 * rng.randn(B, mx.nv)), ctrl=torch.tensor(np.clip(0.5 * rng.randn(B, mx.nu), -1, 1)))
    d = d.to(dtype)
    out = mt.inverse(mx.to("cuda"), d.to("cuda"))
    written = _inverse_names(mx) + ["qfrc_inverse"]
    tol = TOL_PRE[dtype]
    ne, nf, nl = mx.constraint_sizes_py[:3]
    active = 0
    for e in range(B):
        got = {n: _leaf(out, n)[e].cpu().numpy() for n in written}
        hint = {k: got[k] for k in ("contact_dist", "contact_pos", "contact_frame")}
        o = pyoracle.run(mx, d[e], step=False, stages=0x1F, contact_hint=hint)
        pre = [n for n in written if n not in TAIL and n not in INT_LEAVES and n != "sensordata"]
        worst = max(rel_err(got[n], o[n]) for n in pre)
        assert worst <= tol, (xml, e, worst, max(pre, key=lambda n: rel_err(got[n], o[n])))
        tail = _tail_of(mx, got, d[e].qacc.cpu().numpy(), discrete)
        for n in TAIL:
            err = _err(n, got[n], tail[n], got["efc_force"])
            assert err <= tol, (xml, e, n, err)
        active += int(np.count_nonzero(got["efc_force"][ne + nf + nl:]))
    assert active > 0  # contact rows take part
