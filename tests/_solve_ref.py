"""A numpy statement of ``solve`` (mujoco_torch_amd/solver.py), vectorised over environments and written from the definitions of the issue / the module's docstring
(the reference solver's, _src/solver.py:244-553, and math.small_cholesky's, math.py:87-168), not from the kernel and without importing the reference: the yardstick of
tests/test_solve.py, pinned on a hand-worked problem and on the recordings by tests/test_solve_host.py.

Arrays are ``[B, ...]``.  ``dtype`` (longdouble, float64, float32) is the arithmetic of EVERY operation: inputs are cast to it first, sums are numpy's.  An environment
that has stopped keeps its state; ``solve`` returns the state after every body (``qaccs[k]``: after ``min(k, niter)`` bodies).
"""
import numpy as np

LD = np.longdouble
CG, NEWTON = 1, 2  # mjtSolver


def _dot(a, b):
    return (a * b).sum(-1)


def cholesky(A):
    """math.small_cholesky: up to 16 dofs every pivot is clamped at 1e-12, above that ``A + 1e-10 I`` is factored; [B, n, n] -> the lower factor."""
    n = A.shape[-1]
    small = n <= 16
    if not small:
        A = A + A.dtype.type(1e-10) * np.eye(n, dtype=A.dtype)
    L = np.zeros_like(A)
    for j in range(n):
        s = A[:, j, j] - (L[:, j, :j] ** 2).sum(-1)
        L[:, j, j] = np.sqrt(np.maximum(s, A.dtype.type(1e-12)) if small else s)
        for i in range(j + 1, n):
            L[:, i, j] = (A[:, i, j] - (L[:, i, :j] * L[:, j, :j]).sum(-1)) / L[:, j, j]
    return L


def cholesky_solve(L, x):
    """(L L^T)^-1 x: L [B, n, n] (lower triangle read), x [B, n]."""
    n = L.shape[-1]
    y = x.copy()
    for i in range(n):
        y[:, i] = (y[:, i] - (L[:, i, :i] * y[:, :i]).sum(-1)) / L[:, i, i]
    for i in range(n - 1, -1, -1):
        y[:, i] = (y[:, i] - (L[:, i + 1:, i] * y[:, i + 1:]).sum(-1)) / L[:, i, i]
    return y


class Problem:
    """The leaves of B environments in ``dtype`` and the model's constants."""

    def __init__(self, J, D, aref, fl, qM, qLD, qfrc_smooth, qacc_smooth, ne_nf, floss, scale, dtype=LD):
        c = lambda x: np.array(x, dtype=dtype)
        self.J, self.D, self.aref, self.fl, self.M, self.L, self.fs, self.qs = (c(x) for x in (J, D, aref, fl, qM, qLD, qfrc_smooth, qacc_smooth))
        self.dtype, self.t = dtype, np.dtype(dtype).type
        self.ne_nf, self.floss, self.scale = int(ne_nf), bool(floss), self.t(scale)
        self.always = np.arange(self.D.shape[-1]) < self.ne_nf
        self.r = 1 / (self.D + (self.D == 0) * self.t(1e-15))
        self.rf = self.r * self.fl
        self.has = self.fl > 0

    def zones(self, x):
        """(linear_neg, linear_pos, quadratic) of rows at ``x = jar``: [B, n], or [B, K, n] for K points an environment."""
        if self.floss:
            rf, has = (self.rf, self.has) if x.ndim == 2 else (self.rf[:, None, :], self.has[:, None, :])
            neg, pos = (x <= -rf) & has, (x >= rf) & has
        else:
            neg = pos = np.zeros(x.shape, dtype=bool)
        return neg, pos, (self.always | (x < 0)) & ~neg & ~pos

    def evaluate(self, qacc, jar=None, Ma=None):
        """The state at ``qacc``: jar, Ma, force, active rows, J^T force, gauss, cost, grad."""
        qacc = np.array(qacc, dtype=self.dtype)
        jar = np.einsum("bnv,bv->bn", self.J, qacc) - self.aref if jar is None else jar
        Ma = np.einsum("bij,bj->bi", self.M, qacc) if Ma is None else Ma
        neg, pos, quad = self.zones(jar)
        force = self.D * -jar * quad + np.where(neg, self.fl, np.where(pos, -self.fl, self.t(0)))
        qfrc = np.einsum("bnv,bn->bv", self.J, force)
        gauss = self.t(0.5) * _dot(Ma - self.fs, qacc - self.qs)
        half = self.t(0.5)
        floss = (neg * (-half * self.r * self.fl * self.fl - self.fl * jar)).sum(-1) + (pos * (-half * self.r * self.fl * self.fl + self.fl * jar)).sum(-1)
        cost = half * (self.D * jar * jar * quad).sum(-1) + gauss + floss
        return dict(qacc=qacc, jar=jar, Ma=Ma, force=force, active=quad, qfrc=qfrc, gauss=gauss, cost=cost, grad=Ma - self.fs - qfrc)

    def mgrad(self, st, solver):
        if solver == CG:
            return cholesky_solve(self.L, st["grad"])
        H = self.M + np.matmul((self.J * (self.D * st["active"])[:, :, None]).transpose(0, 2, 1), self.J)  # M + J^T diag(D active) J
        return cholesky_solve(cholesky(H), st["grad"])

    def grad_norm(self, st):
        return np.sqrt(_dot(st["grad"], st["grad"])) / self.scale


def _points(P, st, jv, qg, alpha):
    """The line-search points at alpha [B, K]: (cost, deriv_0, deriv_1), each [B, K]."""
    t = P.t
    jar = st["jar"][:, None, :]
    x = jar + alpha[:, :, None] * jv[:, None, :]
    neg, pos, quad = P.zones(x)
    D, fl, rf = P.D[:, None, :], P.fl[:, None, :], P.rf[:, None, :]
    q = [t(0.5) * jar * jar * D, jv[:, None, :] * jar * D, t(0.5) * jv[:, None, :] * jv[:, None, :] * D]
    tot = [qg[k][:, None] + (q[k] * quad).sum(-1) for k in range(3)]
    if P.floss:
        tot[0] = tot[0] + (neg * fl * (-t(0.5) * rf - jar)).sum(-1) + (pos * fl * (-t(0.5) * rf + jar)).sum(-1)
        tot[1] = tot[1] + (neg * (-fl * jv[:, None, :])).sum(-1) + (pos * (fl * jv[:, None, :])).sum(-1)
    cost = alpha * alpha * tot[2] + alpha * tot[1] + tot[0]
    return cost, 2 * alpha * tot[2] + tot[1], 2 * tot[2] + (tot[2] == 0) * t(1e-15)


def _where(c, a, b):
    return tuple(np.where(c, x, y) for x, y in zip(a, b))


def linesearch(P, st, search, tolerance, ls_tolerance, ls_iterations, fixed):
    """The exact line search along ``search`` [B, nv]: (improved [B], alpha [B], mv, jv)."""
    t = P.t
    with np.errstate(all="ignore"):
        gtol = t(tolerance) * t(ls_tolerance) * (np.sqrt(_dot(search, search)) * P.scale)
        mv = np.einsum("bij,bj->bi", P.M, search)
        jv = np.einsum("bnv,bv->bn", P.J, search)
        qg = (st["gauss"], _dot(search, st["Ma"]) - _dot(search, P.fs), t(0.5) * _dot(search, mv))
        point = lambda alpha: tuple(x[:, 0] for x in (alpha[:, None],) + _points(P, st, jv, qg, alpha[:, None]))  # (alpha, cost, d0, d1)
        p0 = point(np.zeros_like(gtol))
        p1 = point(p0[0] - p0[2] / p0[3])
        lesser = p1[2] < p0[2]
        lo, hi = _where(lesser, p1, p0), _where(lesser, p0, p1)
        swap = ~(np.abs(p1[2]) < gtol)
        for _ in range(ls_iterations):
            go = np.ones_like(swap) if fixed else swap & ~((lo[2] < 0) & (lo[2] > -gtol)) & ~((hi[2] > 0) & (hi[2] < gtol))
            if not go.any():
                break
            alpha = np.stack([lo[0] - lo[2] / lo[3], hi[0] - hi[2] / hi[3], t(0.5) * (lo[0] + hi[0])], axis=1)
            c, d0, d1 = _points(P, st, jv, qg, alpha)
            lo_next, hi_next, mid = ((alpha[:, k], c[:, k], d0[:, k], d1[:, k]) for k in range(3))
            nb = (lo[2] < 0) == (hi[2] < 0)
            take = lambda cur, cand: ((cur[2] < cand[2]) & (cand[2] < 0)) | ((cur[2] > cand[2]) & (cand[2] > 0)) | (nb & (np.abs(cand[2]) < np.abs(cur[2])))
            new_lo, new_hi, any_swap = lo, hi, np.zeros_like(swap)
            for cand in (lo_next, mid, hi_next):
                s = take(new_lo, cand)
                new_lo, any_swap = _where(s, cand, new_lo), any_swap | s
            for cand in (hi_next, mid, lo_next):
                s = take(new_hi, cand)
                new_hi, any_swap = _where(s, cand, new_hi), any_swap | s
            lo, hi, swap = _where(go, new_lo, lo), _where(go, new_hi, hi), np.where(go, any_swap, swap)
        improved = (lo[1] < p0[1]) | (hi[1] < p0[1])
        return improved, np.where(lo[1] < hi[1], lo[0], hi[0]), mv, jv


def solve(J, D, aref, fl, qM, qLD, qfrc_smooth, qacc_smooth, qacc_warmstart, ne_nf, floss, scale, solver, iterations, tolerance=0.0, ls_iterations=50,
          ls_tolerance=0.01, fixed=False, warmstart=True, dtype=LD):
    """The solve of B environments as a dict: ``qacc``, ``efc_force``, ``qfrc_constraint``, ``cost``, ``improvement``, ``grad_norm``, ``niter`` at the end, and the
    per-body histories ``qaccs`` [K + 1, B, nv], ``costs``, ``improvements``, ``grad_norms`` [K + 1, B], ``niters`` [K + 1, B] (K: the bodies of the longest
    environment; entry k: the state after min(k, niter) bodies)."""
    P = Problem(J, D, aref, fl, qM, qLD, qfrc_smooth, qacc_smooth, ne_nf, floss, scale, dtype)
    t = P.t
    start = P.qs
    if warmstart:
        warm = np.array(qacc_warmstart, dtype=dtype)
        start = np.where((P.evaluate(warm)["cost"] < P.evaluate(P.qs)["cost"])[:, None], warm, P.qs)
    st = P.evaluate(start)
    B = len(start)
    mg = P.mgrad(st, solver)
    search = -mg
    prev = np.full(B, np.inf, dtype=dtype)
    niter = np.zeros(B, dtype=np.int32)
    hist = dict(qaccs=[], costs=[], improvements=[], grad_norms=[], niters=[])

    def record():
        with np.errstate(all="ignore"):
            for k, v in (("qaccs", st["qacc"]), ("costs", st["cost"]), ("improvements", (prev - st["cost"]) / P.scale), ("grad_norms", P.grad_norm(st)), ("niters", niter)):
                hist[k].append(np.array(v))

    record()
    while True:
        if iterations == 1:
            run = niter < 1
        elif fixed:
            run = niter < iterations
        else:
            with np.errstate(all="ignore"):
                run = ~((niter >= iterations) | ((prev - st["cost"]) / P.scale < t(tolerance)) | (P.grad_norm(st) < t(tolerance)))
        if not run.any():
            break
        improved, alpha, mv, jv = linesearch(P, st, search, tolerance, ls_tolerance, ls_iterations, fixed)
        step = np.where(improved, alpha, t(0))
        new = P.evaluate(st["qacc"] + search * step[:, None], jar=st["jar"] + jv * step[:, None], Ma=st["Ma"] + mv * step[:, None])
        new_mg = P.mgrad(new, solver)
        if solver == NEWTON:
            new_search = -new_mg
        else:
            beta = _dot(new["grad"], new_mg - mg) / np.maximum(_dot(st["grad"], mg), t(1e-15))
            new_search = -new_mg + np.maximum(beta, t(0))[:, None] * search
        pick = lambda a, b: np.where(run.reshape((B,) + (1,) * (a.ndim - 1)), a, b)
        prev = pick(st["cost"], prev)
        st = {k: pick(new[k], st[k]) for k in st}
        mg, search, niter = pick(new_mg, mg), pick(new_search, search), niter + run
        record()
    out = {k: np.stack(v) for k, v in hist.items()}
    with np.errstate(all="ignore"):
        out.update(qacc=st["qacc"], efc_force=st["force"], qfrc_constraint=st["qfrc"], cost=st["cost"], improvement=(prev - st["cost"]) / P.scale,
                   grad_norm=P.grad_norm(st), niter=niter.astype(np.int32))
    return out
