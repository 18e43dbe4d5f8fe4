"""A numpy longdouble reference of the constraint-space functions (mujoco_torch_amd/constraint_space.py), vectorised over environments and written from the
definitions of the issue / the module's docstring (the reference solver's, _src/solver.py:293-357, 501-508), not from the kernels: the yardstick of
tests/test_constraint_space.py, pinned on the recordings by tests/test_constraint_space_host.py.

Arrays are ``[B, ...]``; inputs of any float dtype are taken as they are (the "same rounded inputs") and every operation runs in longdouble.
"""
import numpy as np

LD = np.longdouble
MINVAL = LD(1e-15)  # mujoco.mjMINVAL
SATISFIED, QUADRATIC, LINEAR_NEG, LINEAR_POS = 0, 1, 2, 3


def ld(x):
    return np.asarray(x, dtype=LD)


def mul_jac_vec(J, vec):
    """J [B, n, nv], vec [B, K, nv] -> [B, K, n]."""
    return np.einsum("bnv,bkv->bkn", ld(J), ld(vec))


def mul_jac_t_vec(J, vec):
    """J [B, n, nv], vec [B, K, n] -> [B, K, nv]."""
    return np.einsum("bnv,bkn->bkv", ld(J), ld(vec))


def zones(jar, D, fl, ne_nf, floss):
    """(linear_neg, linear_pos, quadratic, r) of rows [B, n]."""
    jar, D, fl = ld(jar), ld(D), ld(fl)
    r = 1 / (D + (D == 0) * MINVAL)
    if floss:
        neg = (fl > 0) & (jar <= -r * fl)
        pos = (fl > 0) & (jar >= r * fl)
    else:
        neg = pos = np.zeros(jar.shape, dtype=bool)
    always = np.arange(jar.shape[-1]) < ne_nf
    quad = (always | (jar < 0)) & ~neg & ~pos
    return neg, pos, quad, r


def constraint_update(J, D, aref, fl, ne_nf, floss, qacc=None, jar=None, qM=None, qfrc_smooth=None, qacc_smooth=None, inertia_scale=None):
    """The outputs of ``constraint_update`` as a dict; with ``jar`` (and no ``qacc``) ``gauss`` / ``grad`` / ``grad_norm`` are absent and the cost has no Gauss term.
    ``inertia_scale``: meaninertia * max(1, nv)."""
    J, D, fl = ld(J), ld(D), ld(fl)
    assert (qacc is None) != (jar is None)
    out = {}
    if qacc is not None:
        qacc = ld(qacc)
        jar = np.einsum("bnv,bv->bn", J, qacc) - ld(aref)
    jar = ld(jar)
    neg, pos, quad, r = zones(jar, D, fl, ne_nf, floss)
    force = np.where(quad, -D * jar, np.where(neg, fl, np.where(pos, -fl, LD(0))))
    state = np.where(neg, LINEAR_NEG, np.where(pos, LINEAR_POS, np.where(quad, QUADRATIC, SATISFIED))).astype(np.int32)
    cost = (quad * D * jar * jar).sum(-1) / 2 + (neg * (-r * fl * fl / 2 - fl * jar)).sum(-1) + (pos * (-r * fl * fl / 2 + fl * jar)).sum(-1)
    out.update(jar=jar, efc_force=force, efc_state=state, qfrc_constraint=np.einsum("bnv,bn->bv", J, force))
    if qacc is not None:
        ms = np.einsum("bij,bj->bi", ld(qM), qacc) - ld(qfrc_smooth)
        gauss = (ms * (qacc - ld(qacc_smooth))).sum(-1) / 2
        grad = ms - out["qfrc_constraint"]
        out.update(gauss=gauss, grad=grad, grad_norm=np.sqrt((grad * grad).sum(-1)) / LD(inertia_scale))
        cost = cost + gauss
    out["cost"] = cost
    return out


def state_margin(J, qacc, aref, D, fl, ne_nf, floss, eps):
    """(distance of jar from its nearest zone boundary, the propagated rounding bound of jar) per row [B, n], for arithmetic of unit roundoff ``eps``: a state is
    compared only where the distance exceeds the bound.  Bound: gamma_nv sum_j |J_ij qacc_j| + ulp(aref), gamma_nv = (nv + 1) eps, plus two roundings of a
    friction row's boundary r fl.  Boundaries: 0 for the rows past the equality and friction rows, +- r fl for rows with a friction loss; a row with neither
    has no boundary (distance inf)."""
    J, qacc, aref, D, fl = ld(J), ld(qacc), ld(aref), ld(D), ld(fl)
    nv = J.shape[-1]
    jar = np.einsum("bnv,bv->bn", J, qacc) - aref
    spread = np.einsum("bnv,bv->bn", np.abs(J), np.abs(qacc))
    r = 1 / (D + (D == 0) * MINVAL)
    edge = r * fl
    bound = (nv + 1) * LD(eps) * spread + LD(eps) * np.abs(aref)
    dist = np.full(jar.shape, np.inf, dtype=LD)
    free = np.arange(jar.shape[-1]) >= ne_nf
    dist = np.where(free, np.minimum(dist, np.abs(jar)), dist)
    if floss:
        has = fl > 0
        dist = np.where(has, np.minimum(dist, np.minimum(np.abs(jar - edge), np.abs(jar + edge))), dist)
        bound = bound + has * 2 * LD(eps) * np.abs(edge)
    return dist, bound


def comparable(dist, bound):
    """The rows whose state is compared: further from every boundary than the bound -- or with a bound of zero: such a ``jar`` has no rounding in any
    arithmetic (the rows of inactive contacts, J = 0 and aref = 0, whose ``jar`` is an exact zero on its boundary and which are satisfied)."""
    return (dist > bound) | (bound == 0)


def forward_substitute(L, rhs):
    """W with L W^T = rhs^T row by row: L [B, nv, nv] (lower triangle read), rhs [B, n, nv] -> [B, n, nv] = rows (L^-1 rhs_r)."""
    L, W = ld(L), ld(rhs).copy()
    for i in range(L.shape[-1]):
        W[:, :, i] = (W[:, :, i] - np.einsum("bk,bnk->bn", L[:, i, :i], W[:, :, :i])) / L[:, i, i][:, None]
    return W


def efc_R(D):
    D = ld(D)
    return np.where(D > 0, 1 / np.where(D > 0, D, LD(1)), LD(0))


def efc_ar(J, D, aref, qLD, qacc_smooth):
    """(AR [B, n, n], b [B, n]): AR = J (L L^T)^-1 J^T + diag(R), L = qLD's lower triangle, R = 1 / D where D > 0 else 0; b = J qacc_smooth - aref."""
    W = forward_substitute(qLD, J)
    AR = np.einsum("bik,bjk->bij", W, W)
    n = AR.shape[-1]
    AR[:, np.arange(n), np.arange(n)] += efc_R(D)
    return AR, np.einsum("bnv,bv->bn", ld(J), ld(qacc_smooth)) - ld(aref)


def cholesky_solve(M, rhs):
    """M^-1 rhs by a longdouble Cholesky factorisation of M itself (not of a recorded factor): M [B, nv, nv] symmetric positive definite, rhs [B, n, nv] -> [B, n, nv]."""
    M = ld(M)
    nv = M.shape[-1]
    L = np.zeros_like(M)
    for j in range(nv):
        L[:, j, j] = np.sqrt(M[:, j, j] - (L[:, j, :j] ** 2).sum(-1))
        for i in range(j + 1, nv):
            L[:, i, j] = (M[:, i, j] - (L[:, i, :j] * L[:, j, :j]).sum(-1)) / L[:, j, j]
    Y = forward_substitute(L, rhs)
    for i in range(nv - 1, -1, -1):  # L^T x = y
        Y[:, :, i] = (Y[:, :, i] - np.einsum("bk,bnk->bn", L[:, i + 1:, i], Y[:, :, i + 1:])) / L[:, i, i][:, None]
    return Y
