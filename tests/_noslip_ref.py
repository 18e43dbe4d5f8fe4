"""A numpy reference of ``solve_noslip`` (mujoco_torch_amd/noslip.py) in the ``A`` / ``b`` form, vectorised over environments and written from the definitions of
the module's docstring (MuJoCo's ``mj_solNoSlip``), not from the kernel -- which never forms ``A``: the yardstick of tests/test_noslip.py, pinned on hand-worked
problems by tests/test_noslip_host.py.

``dtype=longdouble`` is the yardstick (``A = AR - diag R`` and ``b`` from ``_pgs_ref.dual``).  ``dtype=float64 / float32`` run the same rules -- the forward
substitution, ``A = W W^T``, every residual ``sum_j A_ij f_j + b_i``, the QCQP -- in that precision: the "same precision, other formulation" error that bounds the
kernel's.  Arrays are ``[B, ...]``; inputs are taken as they are (the "same rounded inputs").  The QCQP's Newton iteration runs until the step no longer changes
``lambda`` in the dtype; float32 / float64 keep the definition's cap of 30 factorisations, longdouble is not capped there (200, and the result says whether every
iteration had stopped by itself: the yardstick is the converged QCQP, so a device iteration that the cap cut short would show).
"""
import numpy as np

import _pgs_ref as pr

LD = pr.LD
MINVAL = 1e-15
QCQP_ITERATIONS = 30   # the definition's cap, what the same-dtype runs keep
QCQP_CONVERGED = 200   # longdouble: the iteration runs until it stops by itself; that it did is recorded (``qcqp_converged``)
# status of a block after a sweep: the normal force (pair: the mean) is not positive / the update ended strictly inside / on the boundary / was put back /
# the block is degenerate (a pair with K1 < MINVAL, an elliptic block with a pivot that is not positive: v = 0)
NONE, INTERIOR, BOUNDARY, PUT_BACK, DEGENERATE = 0, 1, 2, 3, 4


def contacts(con_dim, con_efc_address, ncon):
    """[(first row, condim)] of the contacts with friction (condim > 1), in slot order."""
    return [(int(a), int(d)) for d, a in zip(np.asarray(con_dim)[:ncon], np.asarray(con_efc_address)[:ncon]) if d > 1]


def problem(J, D, aref, qLD, qacc_smooth, dtype=LD):
    """(A [B, n, n] = W W^T, b [B, n], R [B, n]) in ``dtype``: ``_pgs_ref.dual`` with the regulariser taken off the diagonal again (longdouble) or never added."""
    AR, b, R = pr.dual(J, D, aref, qLD, qacc_smooth, dtype)
    A = AR.copy()
    n = A.shape[-1]
    if dtype == LD:
        A[:, np.arange(n), np.arange(n)] -= R
    else:  # (the same-dtype run must not round A_ii + R_i - R_i: W W^T itself)
        c = lambda x: np.asarray(x, dtype=dtype)
        W = c(J).copy()
        L = c(qLD)
        for i in range(L.shape[-1]):
            W[:, :, i] = (W[:, :, i] - np.einsum("bk,bnk->bn", L[:, i, :i], W[:, :, :i])) / L[:, i, i][:, None]
        A = np.einsum("bik,bjk->bij", W, W).astype(dtype)
    return A, b, R


def cost_of(A, b, f):
    return np.einsum("bi,bij,bj->b", f, A, f) / 2 + (f * b).sum(-1)


def _chol(M):
    """(L, ok): the Cholesky factor of M [B, N, N] by rows and whether every pivot was positive and finite."""
    B, N, _ = M.shape
    L = np.zeros_like(M)
    ok = np.ones(B, dtype=bool)
    one = M.dtype.type(1)
    with np.errstate(all="ignore"):
        for i in range(N):
            for j in range(i + 1):
                s = M[:, i, j].copy()
                for k in range(j):
                    s = s - L[:, i, k] * L[:, j, k]
                if i == j:
                    ok &= np.isfinite(s) & (s > 0)
                    L[:, i, i] = np.sqrt(np.where(ok, s, one))
                else:
                    L[:, i, j] = s / L[:, j, j]
    return L, ok


def _lower_solve(L, x):
    out = np.zeros_like(x)
    for i in range(x.shape[-1]):
        s = x[:, i].copy()
        for k in range(i):
            s = s - L[:, i, k] * out[:, k]
        out[:, i] = s / L[:, i, i]
    return out


def _upper_solve(L, x):
    """L^T out = x."""
    N = x.shape[-1]
    out = np.zeros_like(x)
    for i in range(N - 1, -1, -1):
        s = x[:, i].copy()
        for k in range(i + 1, N):
            s = s - L[:, k, i] * out[:, k]
        out[:, i] = s / L[:, i, i]
    return out


def qcqp(Ac, bc, mu, r, iterations=None):
    """``argmin 1/2 v^T Ac v + v . bc`` subject to ``sum (v_k / mu_k)^2 <= r^2``: (v [B, N], active [B], lambda [B], singular [B]).  With ``v_k = mu_k u_k``: Newton on the
    multiplier of ``|u|^2 <= r^2`` from 0, ``u = -(A_s + lambda I)^-1 b_s``; a non-positive or non-finite pivot gives ``v = 0``; an active constraint
    (``lambda > 0``) is rescaled onto the surface."""
    dt = Ac.dtype.type
    if iterations is None:
        iterations = QCQP_CONVERGED if Ac.dtype == LD else QCQP_ITERATIONS
    B, N = bc.shape
    As = Ac * mu[:, :, None] * mu[:, None, :]
    bs = bc * mu
    la = np.zeros(B, dtype=Ac.dtype)
    u = np.zeros((B, N), dtype=Ac.dtype)
    done = np.zeros(B, dtype=bool)
    bad = np.zeros(B, dtype=bool)
    eye = np.eye(N, dtype=Ac.dtype)
    with np.errstate(all="ignore"):
        for _ in range(iterations):
            L, ok = _chol(As + la[:, None, None] * eye)
            live = ~done
            bad |= live & ~ok
            done |= bad
            go = live & ok
            un = _upper_solve(L, _lower_solve(L, -bs))
            u = np.where(go[:, None], un, u)
            val = (u * u).sum(-1) - r * r
            w = _lower_solve(L, u)
            step = val / (dt(2) * (w * w).sum(-1))
            new = la + step
            stop = (val <= 0) | ~(step > 0) | (new == la)
            la = np.where(go & ~stop, new, la)
            done |= go & stop
            if done.all():
                break
        active = (la > 0) & ~bad
        s = (u * u).sum(-1)
        scale = np.where(active & (s > 0), r / np.sqrt(np.where(s > 0, s, dt(1))), dt(1))
        v = np.where(bad[:, None], dt(0), u * mu * scale[:, None])
    qcqp.done = done
    return v, active, la, bad


def solve_noslip(J, D, aref, fl, qLD, qacc_smooth, force0, mu, ne, nf, con, elliptic, inertia_scale, iterations, tolerance=0.0, dtype=LD, prob=None):
    """``iterations`` sweeps at most from ``force0`` [B, n] (NOT projected), every environment stopping on its own once a sweep's scaled improvement is below
    ``tolerance``.  ``con``: ``contacts(...)``; ``mu`` [B, len(con), 5]: ``contact.friction`` of the contacts of ``con``, in that order.  A dict: ``forces`` [iterations + 1, B, n], ``improvements`` [iterations, B] (NaN once stopped), ``costs``
    [iterations + 1, B], ``niter``, ``status`` (per sweep: {(contact, pair or 0): [B] codes} and {"fl": [B, nf]}), and of the final force ``efc_force``,
    ``qfrc_constraint``, ``qacc``, ``cost``, ``improvement`` (0 without a sweep); ``qcqp_converged``: every QCQP's iteration stopped by itself."""
    A, b, R = problem(J, D, aref, qLD, qacc_smooth, dtype) if prob is None else prob
    c = lambda x: np.asarray(x, dtype=dtype)
    dt = np.dtype(dtype).type
    B, n = b.shape
    fl, mu = c(fl), c(mu)
    f = np.broadcast_to(c(force0), (B, n)).copy()
    live = np.ones(B, dtype=bool)
    niter = np.zeros(B, dtype=np.int32)
    last = np.zeros(B, dtype=dtype)
    forces, imps, costs, statuses = [f.copy()], [], [cost_of(A, b, f)], []
    converged = True
    half, inv, minval, thresh = dt(0.5), dt(1) / dt(inertia_scale), dt(MINVAL), dt(1e-10)

    def finish_block(new, rows, old, res, Ac):
        """The block's cost change; a rise above 1e-10 puts the block back.  Returns (change [B], put back [B])."""
        delta = new[:, rows] - old
        change = half * np.einsum("bi,bij,bj->b", delta, Ac, delta) + (delta * res).sum(-1)
        back = change > thresh
        new[:, rows] = np.where(back[:, None], old, new[:, rows])
        return np.where(back, dt(0), change), back

    with np.errstate(all="ignore"):
        for it in range(iterations):
            imp = (half * (R.astype(dtype) * f * f).sum(-1)).astype(dtype) if it == 0 else np.zeros(B, dtype=dtype)
            new = f.copy()
            status = {}
            flst = np.zeros((B, nf), dtype=np.int8)
            for i in range(ne, ne + nf):
                res = (A[:, i, :] * new).sum(-1) + b[:, i]
                aii = A[:, i, i]
                ok = ~(aii < minval)
                old = new[:, i].copy()
                x = old - res / np.where(ok, aii, dt(1))
                x = np.where(x < -fl[:, i], -fl[:, i], np.where(x > fl[:, i], fl[:, i], x))
                fi = np.where(ok, x, old)
                delta = fi - old
                imp = imp - delta * (half * delta * aii + res)
                new[:, i] = fi
                flst[:, i - ne] = np.where(ok, np.where(np.abs(fi) < fl[:, i], INTERIOR, BOUNDARY), NONE)
            status["fl"] = flst
            for ci, (adr, dim) in enumerate(con):
                if elliptic:
                    rows = np.arange(adr + 1, adr + dim)
                    res = np.einsum("bij,bj->bi", A[:, rows, :], new) + b[:, rows]
                    Ac = A[:, rows[:, None], rows[None, :]]
                    old = new[:, rows].copy()
                    bc = res - np.einsum("bij,bj->bi", Ac, old)
                    fn = new[:, adr]
                    small = fn < minval
                    v, active, _, bad = qcqp(Ac, bc, mu[:, ci, :dim - 1], fn)
                    converged = converged and bool((qcqp.done | small).all())  # (without a normal force the block is zeroed whatever the QCQP gives)
                    new[:, rows] = np.where(small[:, None], dt(0), v)
                    change, back = finish_block(new, rows, old, res, Ac)
                    imp = imp - change
                    status[(ci, 0)] = np.where(small, NONE, np.where(bad, DEGENERATE, np.where(back, PUT_BACK, np.where(active, BOUNDARY, INTERIOR))))
                else:
                    for p in range(dim - 1):
                        rows = np.array([adr + 2 * p, adr + 2 * p + 1])
                        res = np.einsum("bij,bj->bi", A[:, rows, :], new) + b[:, rows]
                        Ac = A[:, rows[:, None], rows[None, :]]
                        old = new[:, rows].copy()
                        bc = res - np.einsum("bij,bj->bi", Ac, old)
                        mid = half * (old[:, 0] + old[:, 1])
                        K1 = Ac[:, 0, 0] + Ac[:, 1, 1] - Ac[:, 0, 1] - Ac[:, 1, 0]
                        K0 = mid * (Ac[:, 0, 0] - Ac[:, 1, 1]) + bc[:, 0] - bc[:, 1]
                        flat = K1 < minval
                        yy = -K0 / np.where(flat, dt(1), K1)
                        clamped = (yy < -mid) | (yy > mid)
                        yy = np.where(yy < -mid, -mid, np.where(yy > mid, mid, yy))
                        yy = np.where(flat, dt(0), yy)
                        new[:, rows[0]] = np.where(flat, mid, mid + yy)
                        new[:, rows[1]] = np.where(flat, mid, mid - yy)
                        change, back = finish_block(new, rows, old, res, Ac)
                        imp = imp - change
                        inside = ~flat & ~clamped & (np.abs(yy) < mid)
                        status[(ci, p)] = np.where(~(mid > 0), NONE, np.where(flat, DEGENERATE, np.where(back, PUT_BACK, np.where(inside, INTERIOR, BOUNDARY))))
            imp = imp * inv
            f = np.where(live[:, None], new, f)
            niter += live
            last = np.where(live, imp, last)
            imps.append(np.where(live, imp, np.nan))
            live = live & ~(imp < dt(tolerance))
            forces.append(f.copy())
            costs.append(cost_of(A, b, f))
            statuses.append(status)
    qfrc, qacc = pr.finish(J, qLD, qacc_smooth, f, dtype)
    return dict(forces=np.stack(forces), improvements=np.stack(imps) if imps else np.zeros((0, B), dtype=dtype), costs=np.stack(costs), niter=niter, efc_force=f,
                qfrc_constraint=qfrc, qacc=qacc, cost=costs[-1], improvement=last, status=statuses, A=A, b=b, R=R, qcqp_converged=converged)
