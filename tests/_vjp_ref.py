"""A plain numpy reference of the two coordinate maps of ``differentiable_step`` (``tangent_pull``, ``tangent_push``), for the tests only.

Like ``_fd_ref`` it knows nothing of the library: it takes host arrays and a ``_fd_ref.Joints`` and works in the dtype it is given.

The tangent convention is ``_fd_ref.integrate``'s: a quaternion ``q`` moved along ``delta`` is ``q (x) exp(delta / 2)``, to first order
``q + sum_k delta_k b_k / 2`` with ``b_k = q (x) (0, e_k)``.

* ``pull(jt, qpos, gq)``: the cotangent of ``qpos`` seen from the tangent space: ``gt_k = <gq[quaternion], b_k> / 2``, the entry itself elsewhere.
* ``push(jt, qpos, gt)``: the cotangent of ``qpos`` whose pull is ``gt`` and which has no component along ``q``: ``2 sum_k gt_k b_k / |q|^2``
  (zeros for an all-zero quaternion).

``pull_bound`` / ``push_bound``: how far a correct evaluation in a dtype may lie from the exact value (see there).
"""
import numpy as np

import _fd_ref as R


def directions(q):
    """b_k = q (x) (0, e_k), k = 0..2: [..., 3, 4]."""
    e = np.zeros((3, 4), dtype=q.dtype)
    e[0, 1] = e[1, 2] = e[2, 3] = 1
    return np.stack([R.quat_mul(q, np.broadcast_to(e[k], q.shape)) for k in range(3)], axis=-2)


def pull(jt, qpos, gq):
    qpos, gq = np.asarray(qpos), np.asarray(gq)
    out = np.zeros(qpos.shape[:-1] + (jt.nv,), dtype=qpos.dtype)
    add = np.nonzero(jt.axis < 0)[0]
    out[..., add] = gq[..., jt.adr[add]]
    for qa, da in jt.quats:
        b = directions(qpos[..., qa:qa + 4])
        out[..., da:da + 3] = qpos.dtype.type(0.5) * (gq[..., None, qa:qa + 4] * b).sum(-1)
    return out


def push(jt, qpos, gt):
    qpos, gt = np.asarray(qpos), np.asarray(gt)
    out = np.zeros(qpos.shape, dtype=qpos.dtype)
    add = np.nonzero(jt.axis < 0)[0]
    out[..., jt.adr[add]] = gt[..., add]
    for qa, da in jt.quats:
        q = qpos[..., qa:qa + 4]
        b = directions(q)
        n2 = (q * q).sum(-1, keepdims=True)
        out[..., qa:qa + 4] = 2 * (gt[..., da:da + 3, None] * b).sum(-2) / (n2 + (n2 == 0))  # (an all-zero quaternion receives zeros)
    return out


# pull, a rotational dof: 4 products and 3 additions (the halving is exact) -- each of the 7 roundings is relative to a partial sum no larger than
# sum_i |gq_i b_i|, the entries of b being entries of q up to sign
PULL_OPS = 7
# push, one entry of a quaternion: 3 products, 2 additions and the doubling's division (6 roundings) on sum_k |gt_k b_k[i]| / |q|^2, and the 4 products
# and 3 additions of |q|^2 (7 roundings, all terms positive: relative), which the division carries over
PUSH_OPS = 6 + 7


def pull_bound(machine_eps, jt, qpos, gq):
    """[..., nv]: 0 for the copied dofs (exact), else ``PULL_OPS`` roundings of ``sum_i |gq_i| |b_k[i]| / 2``."""
    qpos, gq = np.abs(np.asarray(qpos, dtype=np.float64)), np.abs(np.asarray(gq, dtype=np.float64))
    out = np.zeros(qpos.shape[:-1] + (jt.nv,))
    perm = [[1, 0, 3, 2], [2, 3, 0, 1], [3, 2, 1, 0]]  # |b_k[i]| = |q[perm[k][i]]|
    for qa, da in jt.quats:
        for k in range(3):
            out[..., da + k] = PULL_OPS * float(machine_eps) * 0.5 * (gq[..., qa:qa + 4] * qpos[..., qa:qa + 4][..., perm[k]]).sum(-1)
    return out


def push_bound(machine_eps, jt, qpos, gt):
    """[..., nq]: 0 for the copied entries, else ``PUSH_OPS`` roundings of ``2 sum_k |gt_k| |b_k[i]| / |q|^2``."""
    qpos, gt = np.abs(np.asarray(qpos, dtype=np.float64)), np.abs(np.asarray(gt, dtype=np.float64))
    out = np.zeros(qpos.shape)
    perm = [[1, 0, 3, 2], [2, 3, 0, 1], [3, 2, 1, 0]]
    for qa, da in jt.quats:
        q = qpos[..., qa:qa + 4]
        n2 = (q * q).sum(-1)
        n2 = n2 + (n2 == 0)
        for i in range(4):
            mag = sum(gt[..., da + k] * q[..., perm[k][i]] for k in range(3))
            out[..., qa + i] = PUSH_OPS * float(machine_eps) * 2 * mag / n2
    return out
