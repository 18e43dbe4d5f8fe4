"""A numpy reference of ``solve_pgs`` (mujoco_torch_amd/pgs.py) in the ``AR`` form, vectorised over environments and written from the definitions of the issue /
the module's docstring (MuJoCo's ``mj_solPGS`` for rows of dimension one), not from the kernel -- which never forms ``AR``: the yardstick of tests/test_pgs.py,
pinned on a hand-worked problem and on the recordings by tests/test_pgs_host.py.

``dtype=longdouble`` is the yardstick (``AR`` and ``b`` from ``_efc_ref.efc_ar``).  ``dtype=float64 / float32`` run the same definitions -- the forward
substitution, ``AR = W W^T + diag R``, every row residual ``sum_j AR_ij f_j + b_i`` -- in that precision: the "same precision, other formulation" error that
bounds the kernel's.  Arrays are ``[B, ...]``; inputs are taken as they are (the "same rounded inputs").
"""
import numpy as np

import _efc_ref as er

LD = er.LD


def dual(J, D, aref, qLD, qacc_smooth, dtype=LD):
    """(AR [B, n, n], b [B, n], R [B, n]) in ``dtype``; longdouble: ``_efc_ref.efc_ar`` itself."""
    if dtype == LD:
        AR, b = er.efc_ar(J, D, aref, qLD, qacc_smooth)
        return AR, b, er.efc_R(D)
    c = lambda x: np.asarray(x, dtype=dtype)
    J, D, aref, L, qs = c(J), c(D), c(aref), c(qLD), c(qacc_smooth)
    W = J.copy()
    for i in range(L.shape[-1]):
        W[:, :, i] = (W[:, :, i] - np.einsum("bk,bnk->bn", L[:, i, :i], W[:, :, :i])) / L[:, i, i][:, None]
    R = np.where(D > 0, 1 / np.where(D > 0, D, dtype(1)), dtype(0)).astype(dtype)
    AR = np.einsum("bik,bjk->bij", W, W)
    n = AR.shape[-1]
    AR[:, np.arange(n), np.arange(n)] += R
    return AR.astype(dtype), (np.einsum("bnv,bv->bn", J, qs) - aref).astype(dtype), R


def project(f, fl, ne, nf):
    """The feasible set: rows < ne free, the next nf rows |f| <= fl, later rows f >= 0."""
    out = f.copy()
    fr = slice(ne, ne + nf)
    out[..., fr] = np.clip(f[..., fr], -fl[..., fr], fl[..., fr])
    out[..., ne + nf:] = np.maximum(f[..., ne + nf:], 0)
    return out


def project_row(v, i, fl_i, ne, nf):
    if i < ne:
        return v
    if i < ne + nf:
        return np.clip(v, -fl_i, fl_i)
    return np.maximum(v, 0)


def cost_of(AR, b, f):
    return np.einsum("bi,bij,bj->b", f, AR, f) / 2 + (f * b).sum(-1)


def chol_solve(L, rhs, dtype=LD):
    """(L L^T)^-1 rhs: L [B, nv, nv] (lower triangle read), rhs [B, nv]."""
    L, x = np.asarray(L, dtype=dtype), np.asarray(rhs, dtype=dtype).copy()
    nv = L.shape[-1]
    for i in range(nv):
        x[:, i] = (x[:, i] - (L[:, i, :i] * x[:, :i]).sum(-1)) / L[:, i, i]
    for i in range(nv - 1, -1, -1):
        x[:, i] = (x[:, i] - (L[:, i + 1:, i] * x[:, i + 1:]).sum(-1)) / L[:, i, i]
    return x


def finish(J, qLD, qacc_smooth, f, dtype=LD):
    """(qfrc_constraint = J^T f, qacc = qacc_smooth + (L L^T)^-1 J^T f) of a force [B, n]."""
    qfrc = np.einsum("bnv,bn->bv", np.asarray(J, dtype=dtype), np.asarray(f, dtype=dtype))
    return qfrc, np.asarray(qacc_smooth, dtype=dtype) + chol_solve(qLD, qfrc, dtype)


def solve_pgs(J, D, aref, fl, qLD, qacc_smooth, ne, nf, inertia_scale, iterations, tolerance=0.0, force0=None, dtype=LD, problem=None):
    """``iterations`` sweeps at most, every environment stopping on its own once a sweep's scaled improvement is below ``tolerance``.  A dict:
    ``forces`` [iterations + 1, B, n] (entry 0: the projected ``force0``; an environment that has stopped repeats its last force), ``improvements`` [iterations, B]
    (NaN once stopped), ``costs`` [iterations + 1, B], ``niter`` [B], and of the final force ``efc_force``, ``qfrc_constraint``, ``qacc``, ``cost``,
    ``improvement`` (of the environment's last sweep; 0 without one).  ``inertia_scale``: meaninertia * max(1, nv); ``problem``: ``dual(...)`` of the same inputs and
    dtype, when the caller shares it between runs."""
    AR, b, R = dual(J, D, aref, qLD, qacc_smooth, dtype) if problem is None else problem
    c = lambda x: np.asarray(x, dtype=dtype)
    B, n = b.shape
    fl = c(fl)
    f = project(np.zeros((B, n), dtype=dtype) if force0 is None else np.broadcast_to(c(force0), (B, n)).copy(), fl, ne, nf)
    diag = AR[:, np.arange(n), np.arange(n)]
    live = np.ones(B, dtype=bool)
    niter = np.zeros(B, dtype=np.int32)
    last = np.zeros(B, dtype=dtype)
    forces, imps, costs = [f.copy()], [], [cost_of(AR, b, f)]
    half, inv = dtype(0.5), dtype(1) / dtype(inertia_scale)
    for _ in range(iterations):
        imp = np.zeros(B, dtype=dtype)
        new = f.copy()
        for i in range(n):
            res = (AR[:, i, :] * new).sum(-1) + b[:, i]
            ok = diag[:, i] > 0
            d = np.where(ok, diag[:, i], dtype(1))
            old = new[:, i]
            fi = np.where(ok, project_row(old - res / d, i, fl[:, i], ne, nf), old)
            delta = fi - old
            imp = imp - delta * (half * delta * diag[:, i] + res)
            new[:, i] = fi
        imp = imp * inv
        f = np.where(live[:, None], new, f)
        niter += live
        last = np.where(live, imp, last)
        imps.append(np.where(live, imp, np.nan))
        live = live & ~(imp < dtype(tolerance))
        forces.append(f.copy())
        costs.append(cost_of(AR, b, f))
    qfrc, qacc = finish(J, qLD, qacc_smooth, f, dtype)
    return dict(forces=np.stack(forces), improvements=np.stack(imps) if imps else np.zeros((0, B), dtype=dtype), costs=np.stack(costs), niter=niter, efc_force=f,
                qfrc_constraint=qfrc, qacc=qacc, cost=costs[-1], improvement=last, AR=AR, b=b)
