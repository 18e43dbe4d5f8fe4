"""Ray casting on the GPU: ``mujoco_torch_amd.ray`` against the reference's own ray casting (tests/golden/ray/, tools/gen_ray_golden.py), bit for
bit against the rangefinder sensor, its batch shapes and filters, the vmap / compile operator, no mutation of the input, batches cut into
several launches and value edits of the geom sizes."""
import json
import os

import numpy as np
import pytest
import torch

import mujoco_torch_amd as mt
from _util import GOLD, load_model
from mujoco_torch_amd._enums import SensorType

pytestmark = pytest.mark.gpu

RAY_GOLD = os.path.join(GOLD, "ray")
RAY_CASES = sorted(f[:-4] for f in os.listdir(RAY_GOLD) if f.endswith(".npz") and f != "ray_geom.npz")
DEV = "cuda"


def _load(case):
    z = np.load(os.path.join(RAY_GOLD, case + ".npz"))
    meta = json.loads(str(z["meta"]))
    n = meta["nenv"]
    g = lambda k: np.stack([z[f"{e}/{k}"] for e in range(n)])
    return meta, {k: g(k) for k in ("geom_xpos", "geom_xmat", "pnt", "vec", "dist", "geomid", "runner_up")}


def _posed(mx, n, seed=0, scale=0.05):
    """A batch of n environments after forward(), every qpos entry jittered by scale * randn (quaternions are normalised by the kinematics)."""
    d = mt.make_data(mx).expand(n).clone()
    rng = np.random.RandomState(seed)
    q = d.qpos.clone()
    q += torch.tensor(scale * rng.randn(*q.shape), dtype=q.dtype)
    d = d.replace(qpos=q)
    return mt.forward(mx.to(DEV), d.to(DEV))


@pytest.mark.parametrize("case", RAY_CASES)
def test_matches_the_reference(case):
    meta, a = _load(case)
    dtype = getattr(torch, meta["dtype"])
    mx = load_model(meta["xml"], dtype=dtype).to(DEV)
    d = mt.make_data(mx).expand(meta["nenv"]).clone().to(DEV)
    d = d.replace(geom_xpos=torch.tensor(a["geom_xpos"], device=DEV), geom_xmat=torch.tensor(a["geom_xmat"], device=DEV))
    dist, gid = mt.ray(mx, d, torch.tensor(a["pnt"], device=DEV), torch.tensor(a["vec"], device=DEV),
                       geomgroup=tuple(meta["geomgroup"]), flg_static=meta["flg_static"], bodyexclude=meta["bodyexclude"])
    assert dist.dtype == dtype and gid.dtype == torch.int64 and dist.shape == a["dist"].shape == gid.shape
    dist, gid = dist.double().cpu().numpy(), gid.cpu().numpy()
    tol = 1e-9 if dtype == torch.float64 else 1e-4
    miss = a["geomid"] < 0
    assert np.all(dist[miss] == -1) and np.all(gid[miss] == -1), f"{case}: {np.sum(gid[miss] != -1)} recorded misses hit"
    hit = ~miss
    rel = np.abs(dist[hit] - a["dist"][hit]) / np.maximum(1.0, np.abs(a["dist"][hit]))
    assert rel.max(initial=0) <= tol, f"{case}: dist rel err {rel.max():.3e}"
    tie = np.abs(a["runner_up"] - a["dist"]) <= tol * np.maximum(1.0, np.abs(a["dist"]))
    bad = hit & (gid != a["geomid"]) & ~tie
    assert not bad.any(), f"{case}: geomid differs on {int(bad.sum())} rays without a tie"


def test_bit_identical_to_the_rangefinder():
    """The ant's 8 rangefinders: ray() along each site's z axis, excluding the site's body, is the sensor's value bit for bit."""
    mx = load_model("ant").to(DEV)
    d = _posed(mx, 64, seed=3, scale=0.6)  # tilted torsos and bent legs: the horizontal rays hit the floor and the legs
    st = np.asarray(mx.sensor_type)
    sid = [i for i in range(len(st)) if int(st[i]) == int(SensorType.RANGEFINDER)]
    assert len(sid) == 8
    adr, obj = np.asarray(mx.sensor_adr), np.asarray(mx.sensor_objid)
    site_body = np.asarray(mx.site_bodyid)
    n_hit = 0
    for i in sid:
        s = int(obj[i])
        dist, gid = mt.ray(mx, d, d.site_xpos[:, s], d.site_xmat[:, s, :, 2], bodyexclude=int(site_body[s]))
        want = d.sensordata[:, int(adr[i])]
        assert torch.equal(dist, want), (i, (dist - want).abs().max())
        n_hit += int((gid >= 0).sum())
    assert n_hit > 0


def test_shapes_and_broadcast():
    mx = load_model("ray_scene").to(DEV)
    B, Rn = 6, 5
    d = _posed(mx, B, seed=1)
    rng = np.random.RandomState(0)
    P = torch.tensor(rng.uniform(-1, 1, (B, Rn, 3)) + [0, 0, 1.5], device=DEV)
    V = torch.tensor(rng.randn(B, Rn, 3) - [0, 0, 1.0], device=DEV)
    dist, gid = mt.ray(mx, d, P, V)
    assert dist.shape == (B, Rn) and gid.shape == (B, Rn)
    assert (gid >= 0).any() and (gid < 0).any() or (gid >= 0).all()
    for r in range(Rn):  # an R-ray call is R one-ray calls, bit for bit
        d1, g1 = mt.ray(mx, d, P[:, r], V[:, r])
        assert d1.shape == (B,) and torch.equal(d1, dist[:, r]) and torch.equal(g1, gid[:, r])
    e1, h1 = mt.ray(mx, d, P[0, 0], V[0, 0])  # (3,): the same ray everywhere
    e2, h2 = mt.ray(mx, d, P[0, 0].expand(B, 3), V[0, 0].expand(B, 3))
    assert e1.shape == (B,) and torch.equal(e1, e2) and torch.equal(h1, h2)
    e3, h3 = mt.ray(mx, d, P[:, 0], V)  # pnt per environment, vec per ray
    e4, h4 = mt.ray(mx, d, P[:, :1].expand(B, Rn, 3), V)
    assert e3.shape == (B, Rn) and torch.equal(e3, e4) and torch.equal(h3, h4)
    e5, _ = mt.ray(mx, d, P[0, 0], V)
    e6, _ = mt.ray(mx, d, P[0, 0].expand(B, Rn, 3), V)
    assert torch.equal(e5, e6)
    # two batch dimensions and B = 1
    d2 = mt.make_data(mx).expand(2, 3).clone().to(DEV)
    d2 = d2.replace(geom_xpos=d.geom_xpos.reshape(2, 3, -1, 3), geom_xmat=d.geom_xmat.reshape(2, 3, -1, 3, 3))
    f, h = mt.ray(mx, d2, P.reshape(2, 3, Rn, 3), V.reshape(2, 3, Rn, 3))
    assert f.shape == (2, 3, Rn) and torch.equal(f.reshape(B, Rn), dist) and torch.equal(h.reshape(B, Rn), gid)
    d1 = mt.make_data(mx).expand(1).clone().to(DEV).replace(geom_xpos=d.geom_xpos[2:3], geom_xmat=d.geom_xmat[2:3])
    f, h = mt.ray(mx, d1, P[2:3], V[2:3])
    assert f.shape == (1, Rn) and torch.equal(f[0], dist[2]) and torch.equal(h[0], gid[2])


def test_filters_change_the_answer():
    mx = load_model("ray_scene").to(DEV)
    d = _posed(mx, 4, seed=2)
    names = ["floor", "pillar", "ghost", "ball", "arm", "egg", "crate", "can", "gem", "spike"]
    down = torch.tensor([0.0, 0.0, -1.0], dtype=torch.float64, device=DEV)
    far = torch.tensor([3.0, 3.0, 1.0], dtype=torch.float64, device=DEV)  # over the floor, nothing else below
    dist, gid = mt.ray(mx, d, far, down)
    assert (gid == names.index("floor")).all() and torch.allclose(dist, torch.ones_like(dist))
    dist, gid = mt.ray(mx, d, far, down, flg_static=False)
    assert (gid == -1).all() and (dist == -1).all()
    top = d.geom_xpos[:, names.index("ball")] + torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64, device=DEV)
    _, gid = mt.ray(mx, d, top, down)
    assert (gid == names.index("ball")).all()
    _, gid = mt.ray(mx, d, top, down, bodyexclude=1)  # torso excluded: the floor below
    assert not (gid == names.index("ball")).any() and not (gid == names.index("arm")).any() and not (gid == names.index("egg")).any()
    ghost = torch.tensor([-1.2, 0.0, 2.0], dtype=torch.float64, device=DEV)  # the transparent box over the floor
    dist, gid = mt.ray(mx, d, ghost, down)
    assert (gid == names.index("floor")).all() and torch.allclose(dist, torch.full_like(dist, 2.0))
    _, gid = mt.ray(mx, d, top, down, geomgroup=(1, 1, 0, 0, 0, 0))
    assert (gid == names.index("ball")).all()
    _, gid = mt.ray(mx, d, top, down, geomgroup=(0, 1, 1, 1, 0, 0))
    assert not (gid == names.index("ball")).any()


def test_vmap_and_compile_match_the_direct_call():
    mx = load_model("ray_scene").to(DEV)
    B, Rn = 5, 4
    d = _posed(mx, B, seed=4)
    rng = np.random.RandomState(1)
    P = torch.tensor(rng.uniform(-1, 1, (B, Rn, 3)) + [0, 0, 1.5], device=DEV)
    V = torch.tensor(rng.randn(B, Rn, 3) - [0, 0, 1.0], device=DEV)
    want = mt.ray(mx, d, P, V, bodyexclude=[2])
    got = torch.vmap(lambda dd, p, v: mt.ray(mx, dd, p, v, bodyexclude=[2]))(d, P, V)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    one = mt.ray(mx, d, P[0, 0], V[:, 0])
    got = torch.vmap(lambda dd, v: mt.ray(mx, dd, P[0, 0], v))(d, V[:, 0])
    assert torch.equal(got[0], one[0]) and torch.equal(got[1], one[1])
    f = torch.compile(lambda dd, p, v: mt.ray(mx, dd, p, v, bodyexclude=[2]), fullgraph=True)
    got = f(d, P, V)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_input_data_is_not_mutated():
    mx = load_model("mesh_contact").to(DEV)
    d = _posed(mx, 8, seed=5)
    before = {k: getattr(d, k).clone() for k in ("geom_xpos", "geom_xmat", "qpos", "xpos")}
    p = torch.tensor([0.0, 0.0, 2.0], dtype=torch.float64, device=DEV)
    v = torch.tensor([0.01, 0.02, -1.0], dtype=torch.float64, device=DEV)
    mt.ray(mx, d, p, v)
    for k, t in before.items():
        assert torch.equal(getattr(d, k), t), k


def test_batches_past_one_launch_are_cut_on_the_host():
    """MJH_MAX_GRID_LOG2=2 caps a launch at 4 workgroups (1024 pairs): 203 environments x 7 rays run in several launches, a launch boundary falling
    inside an environment, bit-identical to one launch."""
    import subprocess
    import sys
    import tempfile

    code = r'''
import sys
sys.path.insert(0, "tests"); sys.path.insert(0, "mujoco-torch_amd"); sys.path.insert(0, "oracle")
import numpy as np, torch, mujoco_torch_amd as mt
from _util import load_model
res = {}
for xml, dt in (("ray_scene", torch.float64), ("mesh_contact", torch.float32), ("humanoid", torch.float64)):
    mx = load_model(xml, dtype=dt).to("cuda")
    B = 203
    d = mt.make_data(mx).expand(B).clone()
    q = d.qpos.clone(); q += torch.tensor(0.05 * np.random.RandomState(0).randn(*q.shape), dtype=q.dtype); d = d.replace(qpos=q)
    if dt != torch.float64: d = d.to(dt)
    d = mt.forward(mx, d.to("cuda"))
    rng = np.random.RandomState(1)
    P = torch.tensor(rng.uniform(-1, 1, (B, 7, 3)) + [0, 0, 1.5], dtype=dt, device="cuda")
    V = torch.tensor(rng.randn(B, 7, 3) - [0, 0, 1.0], dtype=dt, device="cuda")
    res[xml] = [t.cpu() for t in mt.ray(mx, d, P, V)] + [t.cpu() for t in mt.ray(mx, d, P[:, 0], V[:, 0])]
torch.save(res, sys.argv[1])
print("ran")
'''
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as td:
        res = {}
        for tag, env in (("one", {}), ("cut", {"MJH_MAX_GRID_LOG2": "2"})):
            f = os.path.join(td, tag + ".pt")
            r = subprocess.run([sys.executable, "-c", code, f], cwd=root, env=dict(os.environ, **env), capture_output=True, text=True, timeout=900)
            assert r.returncode == 0 and "ran" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
            res[tag] = torch.load(f)
    for case in res["one"]:
        for a, b in zip(res["one"][case], res["cut"][case]):
            assert torch.equal(a, b), case


def test_geom_size_edit_takes_effect_without_a_rebuild():
    mx = load_model("ray_scene").to(DEV)
    d = _posed(mx, 4, seed=6)
    ball = 3
    top = d.geom_xpos[:, ball] + torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64, device=DEV)
    down = torch.tensor([0.0, 0.0, -1.0], dtype=torch.float64, device=DEV)
    d0, g0 = mt.ray(mx, d, top, down)
    assert (g0 == ball).all()
    size = mx.geom_size.clone()
    size[ball, 0] = 0.3
    mx2 = mx.replace(geom_size=size)
    d1, g1 = mt.ray(mx2, d, top, down)
    assert (g1 == ball).all()
    assert torch.allclose(d1, d0 - 0.15, atol=1e-12)
    d2, _ = mt.ray(mx, d, top, down)  # the original model still has its own sizes
    assert torch.equal(d2, d0)
