"""A plain numpy reference of what ``inverse_fd`` does around the inverse passes (MuJoCo's ``mjd_inverseFD``), for the tests only.

Like ``_fd_ref`` it knows nothing of the library: host arrays and ``_fd_ref.Joints`` in, host arrays out, in the dtype of the arrays it is given.

Column ``c`` in ``[0, nv)`` nudges ``qpos`` along dof ``c`` in tangent space (``_fd_ref.integrate``: addition, or the quaternion rotated about the
dof's local axis), ``[nv, 2 nv)`` adds to ``qvel``, ``[2 nv, 3 nv)`` to ``qacc``; side 0 by ``+eps``, side 1 (centered only) by ``-eps``.

* ``perturbed`` builds ``qpos`` / ``qvel`` / ``qacc`` of every (environment, column, side);
* ``jacobians`` forms ``DfDq, DfDv, DfDa`` (``DsDq, DsDv, DsDa``) from the nominal and the perturbed ``qfrc_inverse`` (``sensordata``):
  ``(y+ - y0) / eps`` one-sided, ``(y+ - y-) / (2 eps)`` centered, in the arrays' dtype -- the expression of ``mjh_ifd_difference_kernel``
  (``csrc/mjh_ifd.h``), so that equal inputs give equal bits.  Rows are outputs, columns what was perturbed.
"""
import numpy as np

import _fd_ref as R


def perturbed(jt, qpos, qvel, qacc, eps, centered):
    """{qpos, qvel, qacc}, each [B, 3 nv, nside, n]."""
    qpos, qvel, qacc = (np.asarray(x) for x in (qpos, qvel, qacc))
    B, nv = qpos.shape[0], jt.nv
    nside = 2 if centered else 1
    h = qpos.dtype.type(eps)
    rep = lambda x: np.array(np.broadcast_to(x[:, None, None, :], (B, 3 * nv, nside, x.shape[-1])))
    P = dict(qpos=rep(qpos), qvel=rep(qvel), qacc=rep(qacc))
    for side in range(nside):
        s = -h if side else h
        for j in range(nv):
            e = np.zeros(nv, dtype=qpos.dtype)
            e[j] = 1
            P["qpos"][:, j, side] = R.integrate(jt, qpos, e, s)
            P["qvel"][:, nv + j, side, j] = qvel[:, j] + s
            P["qacc"][:, 2 * nv + j, side, j] = qacc[:, j] + s
    return P


def difference(y0, y, eps, centered):
    """[B, rows, 3 nv] from the nominal ``y0`` [B, rows] and the perturbed ``y`` [B, 3 nv, nside, rows]."""
    y0, y = np.asarray(y0), np.asarray(y)
    h = y.dtype.type(eps)
    J = (y[:, :, 0] - y[:, :, 1]) / (2 * h) if centered else (y[:, :, 0] - y0[:, None, :]) / h
    assert J.dtype == y.dtype
    return np.swapaxes(J, 1, 2)


def jacobians(nv, f0, f, eps, centered, s0=None, s=None):
    """DfDq, DfDv, DfDa (and DsDq, DsDv, DsDa when ``s`` is given): [B, nv, nv] ([B, nsensordata, nv])."""
    Jf = difference(f0, f, eps, centered)
    out = tuple(Jf[:, :, k * nv:(k + 1) * nv] for k in range(3))
    if s is not None:
        Js = difference(s0, s, eps, centered)
        out += tuple(Js[:, :, k * nv:(k + 1) * nv] for k in range(3))
    return out
