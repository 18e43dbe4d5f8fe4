"""The committed targets of the ``ik_site`` tests (tests/test_ik_host.py chooses and checks them on the CPU, tests/test_ik.py runs them on the GPU), for the tests only.

A case is a site of tests/golden/ik_arm.xml, which parts of the pose are asked for and a joint selection.  Its targets are the site poses of
``qpos* = qpos0 (+) 0.3 U(-1, 1)`` on the selected dofs (seeded), so they are reachable by construction; the kinematics come from the oracle's forward pass.
``reference(case, key)`` runs the longdouble loop (tests/_ik_ref.py) on them once per process: per target the reference's step count, and whether the target is
CLEAR -- the error after the last update below ``tol / 10`` and the error before it above ``10 tol``, so that a correct implementation in the working precision
takes the same number of updates.
"""
import functools

import numpy as np
import torch

import _ik_ref as ir
import _qpos_ref as qr
import mujoco_torch_amd as mt
import pyoracle
from _util import load_model

STAGE_KINEMATICS = 1
TIP, PROBE = 0, 1
# name: (site, position?, orientation?, joints, keyword arguments).  Joints 0-6: the hinges, 7: the slide, 8: the ball-joint wrist, 9: the probe's free joint.
# (The free body's Jacobian is square and well conditioned, so with the default damping its error falls by 1e-6 per update and lands within a decade of
#  tol = 1e-9 however the target is drawn: that case runs with damping = 1e-9.)
CASES = {
    "tip_pos": (TIP, True, False, None, {}),
    "tip_quat": (TIP, False, True, None, {}),
    "tip_both": (TIP, True, True, None, {}),
    "tip_both_subset": (TIP, True, True, [1, 2, 3, 5, 7, 8], {}),
    "probe_both": (PROBE, True, True, [9], {"damping": 1e-9}),
}
TOL = {"f64": 1e-9, "f32": 2e-4}
# one seed per target: RandomState(seed).uniform(-1, 1, nv) is its draw.  Chosen on the CPU among seeds 1000 .. 1059 by the longdouble loop alone.
SEEDS = {
    ("tip_pos", "f64"): [1000, 1001, 1002, 1003, 1004, 1005, 1006, 1008, 1009, 1010],
    ("tip_quat", "f64"): [1000, 1001, 1002, 1003, 1004, 1005, 1006, 1007, 1008, 1009],
    ("tip_both", "f64"): [1000, 1001, 1002, 1003, 1005, 1006, 1007, 1008, 1009, 1010],
    ("tip_both_subset", "f64"): [1000, 1002, 1003, 1005, 1006, 1007, 1008, 1010, 1013, 1015],
    ("tip_pos", "f32"): [1000, 1001, 1002, 1003, 1005, 1008, 1009, 1011, 1012, 1015],
    ("tip_quat", "f32"): [1000, 1001, 1002, 1003, 1004, 1005, 1006, 1007, 1009, 1010],
    ("tip_both", "f32"): [1000, 1001, 1002, 1003, 1005, 1008, 1009, 1011, 1012, 1013],
    ("tip_both_subset", "f32"): [1000, 1001, 1005, 1008, 1011, 1012, 1014, 1018, 1019, 1026],
    ("probe_both", "f64"): [1000, 1001, 1002, 1003, 1004, 1005, 1006, 1007, 1008, 1009],
    ("probe_both", "f32"): [1000, 1004, 1006, 1007, 1008, 1009, 1011, 1014, 1017, 1019],
}
MAX_STEPS = 20


@functools.lru_cache(maxsize=None)
def model(dtype=torch.float64):
    return load_model("ik_arm", dtype=dtype)


def kinematics(mx):
    """qpos [B, nq] float64 -> the leaves of the oracle's kinematics pass."""
    d0 = mt.make_data(mx)

    def run(q):
        q = torch.tensor(np.asarray(q, dtype=np.float64))
        out = pyoracle.run(mx, d0.expand(q.shape[0]).clone().replace(qpos=q), step=False, stages=STAGE_KINEMATICS)
        return {n: out[n] for n in ("cdof", "subtree_com", "site_xpos", "site_xmat")}

    return run


def mat_to_quat(M):
    """Unit quaternions of the rotation matrices M [B, 3, 3] (float64), w >= 0."""
    v = ir.rotvec(M)
    a = np.sqrt((v * v).sum(-1, keepdims=True))
    q = np.concatenate([np.cos(a / 2), np.where(a == 0, 0, v / np.where(a == 0, 1, a)) * np.sin(a / 2)], -1)
    return np.asarray(q, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def targets(case, key, seeds=None):
    """dict(site, joints, kw, qpos0 [B, nq], qpos_star, target_pos or None, target_quat or None), float64; ``key``: "f64" / "f32" (the committed seeds of that
    tolerance), or ``seeds`` given as a tuple."""
    site, pos, rot, joints, kw = CASES[case]
    seeds = SEEDS[case, key] if seeds is None else list(seeds)
    mx, n = model(), len(seeds)
    T = ir.tables(mx, site, joints)
    q0 = np.broadcast_to(mx.qpos0.numpy().astype(np.float64), (n, int(mx.nq)))
    dq = np.stack([0.3 * np.random.RandomState(s).uniform(-1, 1, int(mx.nv)) for s in seeds]) * T["sel"]
    star = qr.integrate_pos(T["J"], q0, dq, 1.0).astype(np.float64)
    L = kinematics(mx)(star)
    return dict(site=site, joints=joints, kw=kw, qpos0=np.array(q0), qpos_star=star,
                target_pos=L["site_xpos"].reshape(n, -1, 3)[:, site].copy() if pos else None,
                target_quat=mat_to_quat(L["site_xmat"].reshape(n, -1, 3, 3)[:, site]) if rot else None)


@functools.lru_cache(maxsize=None)
def reference(case, key, seeds=None):
    """The longdouble loop on the case's targets at ``TOL[key]``: dict(steps, success, clear, history, qpos, err_norm)."""
    t, tol = targets(case, key, seeds), TOL[key]
    mx, n = model(), t["qpos0"].shape[0]
    r = ir.loop(ir.tables(mx, t["site"], t["joints"]), kinematics(mx), t["qpos0"], t["target_pos"], t["target_quat"], tol=tol, max_steps=MAX_STEPS, **t["kw"])
    h, s = r["history"], r["steps"]
    idx = np.arange(n)
    last = h[s, idx]                          # the evaluation that found the environment done: the error after its last update
    before = h[np.maximum(s - 1, 0), idx]     # ... and the error that last update started from
    r["clear"] = r["success"] & (s > 0) & (last < tol / 10) & (before > 10 * tol)
    return r
