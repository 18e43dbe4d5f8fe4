"""A numpy longdouble reference of one iteration of ``ik_site`` (mujoco_torch_amd/ik.py, csrc/mjh_ik.h), for the tests only, and the loop around it with the
kinematics supplied by the caller (on the CPU: the oracle's forward pass).

One iteration, per environment, given the leaves of the kinematics pass at the current ``qpos``:

* ``e_pos = target_pos - site_xpos``; ``e_rot`` = the rotation vector (axis times angle, angle in [0, pi]) of ``R(target_quat) site_xmat^T``;
  ``e`` stacks the parts asked for; ``err_norm = |e_pos| + rot_weight |e_rot|``; ``err_norm < tol``: done.
* ``J`` = the rows of (jacp | jacr) of the site asked for, ``jacp[d] = (cdof[d, 3:] + cdof[d, :3] x (site_xpos - subtree_com[root])) mask[d]``,
  ``jacr[d] = cdof[d, :3] mask[d]``, the columns of unselected dofs zeroed; ``(J J^T + damping I) y = e`` by Cholesky, every pivot clamped at 1e-12; ``delta = J^T y``, scaled to ``max_update_norm`` when longer;
  ``qpos <- integrate_pos(qpos, delta, 1)`` (tests/_qpos_ref.py) on the joints with a selected dof, the others copied.

The ancestor mask is walked from ``body_parentid`` (``_support_ref.ancestor_mask``); the library's tables are never read.
"""
import numpy as np

import _qpos_ref as qr
from _support_ref import ancestor_mask

LD = np.longdouble


def tables(mx, site, joints=None):
    """What one site and one joint selection need of the model, as host arrays."""
    J = qr.joints(mx)
    body = int(qr._np(mx.site_bodyid).reshape(-1)[site])
    mask = ancestor_mask(qr._np(mx.body_parentid), qr._np(mx.dof_bodyid))[body]
    sel = np.zeros(J[2], dtype=bool)
    width = {qr.FREE: 6, qr.BALL: 3}
    for j, (t, qa, da) in enumerate(J[0]):
        if joints is None or j in list(joints):
            sel[da:da + width.get(t, 1)] = True
    moved = [any(sel[da:da + width.get(t, 1)]) for t, qa, da in J[0]]
    return dict(J=J, site=int(site), body=body, root=int(qr._np(mx.body_rootid).reshape(-1)[body]), mask=mask, sel=sel, moved=moved)


def quat_to_mat(q):
    w, x, y, z = (q[..., i] for i in range(4))
    return np.stack([np.stack([w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                     np.stack([2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)], -1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z], -1)], -2)


def rotvec(E):
    """The rotation vector of the rotation matrices E [..., 3, 3], angle in [0, pi]: through the quaternion, by the branch of Shepperd's method with the
    largest pivot."""
    E = np.asarray(E, dtype=LD)
    out = np.empty(E.shape[:-2] + (3,), dtype=LD)
    for idx in np.ndindex(*E.shape[:-2]):
        M = E[idx]
        piv = [M[0, 0] + M[1, 1] + M[2, 2], M[0, 0], M[1, 1], M[2, 2]]
        k = int(np.argmax(piv))
        if k == 0:
            s = 2 * np.sqrt(1 + piv[0])
            q = [s / 4, (M[2, 1] - M[1, 2]) / s, (M[0, 2] - M[2, 0]) / s, (M[1, 0] - M[0, 1]) / s]
        elif k == 1:
            s = 2 * np.sqrt(1 + M[0, 0] - M[1, 1] - M[2, 2])
            q = [(M[2, 1] - M[1, 2]) / s, s / 4, (M[0, 1] + M[1, 0]) / s, (M[0, 2] + M[2, 0]) / s]
        elif k == 2:
            s = 2 * np.sqrt(1 + M[1, 1] - M[0, 0] - M[2, 2])
            q = [(M[0, 2] - M[2, 0]) / s, (M[0, 1] + M[1, 0]) / s, s / 4, (M[1, 2] + M[2, 1]) / s]
        else:
            s = 2 * np.sqrt(1 + M[2, 2] - M[0, 0] - M[1, 1])
            q = [(M[1, 0] - M[0, 1]) / s, (M[0, 2] + M[2, 0]) / s, (M[1, 2] + M[2, 1]) / s, s / 4]
        q = np.array(q, dtype=LD) * (-1 if q[0] < 0 else 1)
        sn = np.sqrt((q[1:] ** 2).sum())
        out[idx] = 0 if sn == 0 else q[1:] / sn * (2 * np.arctan2(sn, q[0]))
    return out


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def error(T, leaves, target_pos, target_quat, rot_weight=1.0):
    """(e [B, 3 or 6], err_norm [B])."""
    s, B = T["site"], leaves["cdof"].shape[0]
    parts, norm = [], 0
    if target_pos is not None:
        e = np.asarray(target_pos, dtype=LD) - np.asarray(leaves["site_xpos"], dtype=LD).reshape(B, -1, 3)[:, s]
        parts.append(e)
        norm = norm + np.sqrt((e * e).sum(-1))
    if target_quat is not None:
        S = np.asarray(leaves["site_xmat"], dtype=LD).reshape(B, -1, 3, 3)[:, s]
        R = quat_to_mat(np.broadcast_to(np.asarray(target_quat, dtype=LD), (B, 4)))
        e = rotvec(R @ np.swapaxes(S, -1, -2))
        parts.append(e)
        norm = norm + LD(rot_weight) * np.sqrt((e * e).sum(-1))
    return np.concatenate(parts, -1), norm


def jacobian(T, leaves, with_pos, with_rot):
    """J [B, 3 or 6, nv]: the rows asked for, unselected columns zero."""
    B = leaves["cdof"].shape[0]
    cd = np.asarray(leaves["cdof"], dtype=LD).reshape(B, -1, 6)
    com = np.asarray(leaves["subtree_com"], dtype=LD).reshape(B, -1, 3)[:, T["root"]]
    pt = np.asarray(leaves["site_xpos"], dtype=LD).reshape(B, -1, 3)[:, T["site"]]
    on = (T["mask"] & T["sel"]).astype(LD)[None, :, None]
    rows = []
    if with_pos:
        rows.append((cd[..., 3:] + _cross(cd[..., :3], (pt - com)[:, None, :])) * on)
    if with_rot:
        rows.append(cd[..., :3] * on)
    return np.swapaxes(np.concatenate(rows, -1), -1, -2)


def iteration(T, leaves, qpos, target_pos=None, target_quat=None, tol=1e-9, damping=1e-6, max_update_norm=2.0, rot_weight=1.0):
    """One iteration on every environment: dict(e, err_norm, done, J, y, delta, qpos) -- ``qpos`` advanced where the environment is not done."""
    q = np.asarray(qpos, dtype=LD)
    e, norm = error(T, leaves, target_pos, target_quat, rot_weight)
    done = norm < LD(tol)
    J = jacobian(T, leaves, target_pos is not None, target_quat is not None)
    n = J.shape[1]
    G = J @ np.swapaxes(J, -1, -2) + LD(damping) * np.eye(n, dtype=LD)
    y = np.empty(e.shape, dtype=LD)
    for b in range(G.shape[0]):  # Cholesky and two substitutions in longdouble (numpy.linalg has no longdouble)
        L = np.zeros((n, n), dtype=LD)
        for i in range(n):
            for j in range(i + 1):
                s = G[b, i, j] - (L[i, :j] * L[j, :j]).sum()
                L[i, j] = np.sqrt(max(s, LD(1e-12))) if i == j else s / L[j, j]  # (the kernel's pivot clamp: never active on a positive definite G)
        z = np.zeros(n, dtype=LD)
        for i in range(n):
            z[i] = (e[b, i] - (L[i, :i] * z[:i]).sum()) / L[i, i]
        for i in reversed(range(n)):
            z[i] = (z[i] - (L[i + 1:, i] * z[i + 1:]).sum()) / L[i, i]
        y[b] = z
    delta = (np.swapaxes(J, -1, -2) @ y[..., None])[..., 0]
    dn = np.sqrt((delta * delta).sum(-1, keepdims=True))
    delta = np.where(dn > LD(max_update_norm), delta * (LD(max_update_norm) / np.where(dn == 0, LD(1), dn)), delta)
    new = qr.integrate_pos(T["J"], q, delta, 1.0)
    for (t, qa, da), moved in zip(T["J"][0], T["moved"]):
        if not moved:
            w = {qr.FREE: 7, qr.BALL: 4}.get(t, 1)
            new[..., qa:qa + w] = q[..., qa:qa + w]
    new = np.where(done[:, None], q, new)
    return dict(e=e, err_norm=norm, done=done, J=J, y=y, delta=delta, qpos=new)


def loop(T, kinematics, qpos, target_pos=None, target_quat=None, tol=1e-9, max_steps=20, **kw):
    """The whole loop: ``kinematics(qpos [B, nq] float64) -> leaves``.  Returns dict(qpos, err_norm, steps, success, history): ``history[k]`` is the err_norm of
    evaluation k ([B]; a done environment keeps its last value)."""
    q = np.asarray(qpos, dtype=LD).copy()
    B = q.shape[0]
    done, steps, err, hist = np.zeros(B, dtype=bool), np.zeros(B, dtype=np.int32), np.zeros(B, dtype=LD), []
    for k in range(max_steps + 1):
        r = iteration(T, kinematics(q.astype(np.float64)), q, target_pos, target_quat, tol=tol, **kw)
        live = ~done
        err = np.where(live, r["err_norm"], err)
        done = done | (live & r["done"])
        hist.append(err.copy())
        if k < max_steps:
            go = ~done
            q = np.where(go[:, None], r["qpos"], q)
            steps = steps + go.astype(np.int32)
    return dict(qpos=q, err_norm=err, steps=steps, success=done, history=np.stack(hist))
