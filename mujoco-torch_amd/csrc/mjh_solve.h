// mjh_solve.h -- the kernel behind mjh_solve: the reference's primal constraint solver (CG and Newton with an exact line search, mujoco_torch/_src/solver.py:244-553) on the
// leaves of a finished pass.  Dense models only; one wavefront (the whole workgroup) per environment, so an environment stops on its own and every branch on a reduced
// scalar is wave-uniform (wave_sum leaves the same bits in every lane).  Every constraint row is a scalar row, whatever the cone: the cost minimised is the one
// mjh_efc_update_kernel evaluates (mjh_efc.h), with its zones, forces and order of sums.
//
// LDS (solve_lds), in this order: the packed lower triangle of qM (Mp); a second packed triangle (Lp: qLD for CG; for Newton H = qM + J^T diag(D active) J, factored in
// place); ALL of efc_J (nefc rows of ld = nv | 1 reals, staged once by efc_load_rows in the plan's chunks and read three ways afterwards: J search a row per lane, J^T force
// by efc_jt_accumulate, Newton's J^T D J an entry of the triangle per lane); the row vectors D, frictionloss, jar (= J qacc - aref), jv (= J search), force and, Newton
// only, da (= D where the row is quadratic, else 0); the dof vectors qacc, Ma, grad, Mgrad, the previous Mgrad (CG's Polak-Ribiere), search, mv, qfrc_smooth, qacc_smooth
// and J^T force; red, the 64 partial sums of efc_jt_accumulate.  qM is held, not re-read: a product with it is taken on every iteration.
//
// One evaluation (solve_update), at the jar and Ma in LDS: zones, forces and the cost of mjh_efc_update_kernel -- r = 1 / (D + (D == 0) mjMINVAL); linear-neg: fl > 0 and
// jar <= -r fl; linear-pos: fl > 0 and jar >= r fl (both only with `floss`); quadratic: (row < ne + nf or jar < 0) and not linear; force = -D jar, +fl, -fl or 0;
// cost = (1/2 sum_quadratic D jar^2 + gauss) + sum_linear (-1/2 r fl^2 -/+ fl jar), gauss = 1/2 (Ma - qfrc_smooth) . (qacc - qacc_smooth) -- then J^T force.
// Gradient (solve_gradient): grad = Ma - qfrc_smooth - J^T force; Mgrad = (Lp Lp^T)^-1 grad by a forward substitution whose element k subtracts in column order (as
// math.small_cholesky_solve does) and a column-oriented back substitution.  Newton builds H first and factors it by math.small_cholesky's rule: up to 16 dofs every pivot is
// clamped at 1e-12, above that H + 1e-10 I is factored; a column's diagonal is computed by every lane, its entries below one per lane, each sum in k order.
// Start: qacc_smooth, or -- with `warmstart` -- qacc_warmstart when its cost is strictly below qacc_smooth's.  The cost before the first body is +inf.
// One body: the line search, the evaluation, the gradient; search = -Mgrad (Newton) or -Mgrad + max(0, grad . (Mgrad - Mgrad_prev) / max(grad_prev . Mgrad_prev, mjMINVAL))
// search (CG).  iterations == 1: one body, unconditionally; `fixed`: exactly `iterations` bodies; otherwise bodies while not (niter >= iterations or
// (prev_cost - cost) / scale < tolerance or |grad| / scale < tolerance), scale = meaninertia max(1, nv).
// Line search (solve_linesearch), the reference's :378-497: gtol = tolerance ls_tolerance |search| scale; a point at alpha sums, over the rows quadratic at
// jar + alpha jv, the row's (1/2 jar^2 D, jv jar D, 1/2 jv^2 D) and, over the linear ones, fl (-1/2 r fl -/+ jar) and -/+ fl jv -- a lane's rows in ascending order into one
// partial sum per coefficient, wave_sum, plus (gauss, search . Ma - search . qfrc_smooth, 1/2 search . mv); cost, deriv_0 and deriv_1 (guarded by mjMINVAL) from the three
// totals.  p0 at 0, p1 at its Newton step, lo / hi by their derivatives, no iteration when |p1.deriv_0| < gtol; an iteration evaluates lo's and hi's Newton steps and the
// midpoint in ONE pass over the rows and applies the six swap tests in the reference's order with its not_bracketed acceptance; `fixed` runs exactly ls_iterations of
// them.  qacc, Ma and jar move by alpha of the cheaper end only if an end's cost is below p0's.
//
// Sums over k < nv or i < nefc: lane l sums l, l + 64, ... in ascending order, wave_sum adds the lanes in its fixed order -- an order that depends on nv (nefc) alone, never
// on the batch, the launch cut or the position in the grid.
//
// Per environment: efc_J, qM and qLD (CG) once, D, aref (once per start candidate, at most three times), frictionloss, qfrc_smooth, qacc_smooth, qacc_warmstart in;
// qacc, qacc_warmstart, qfrc_constraint, efc_force, cost, improvement, grad_norm, niter out (the account of mjh_model_kernel_io).
#pragma once
#include "mjh_efc.h"

#define MJH_SOLVER_CG 1      /* mjtSolver */
#define MJH_SOLVER_NEWTON 2
#define MJH_SOLVE_DOF_VECTORS 10

template <typename REAL>
struct SolveArgs {
  const REAL *J, *D, *aref, *fl, *qM, *qLD, *qfrc_smooth, *qacc_smooth, *qacc_warmstart;  // [B, ...] leaves
  REAL *qacc, *qacc_warmstart_out, *qfrc_constraint, *force, *cost, *improvement, *grad_norm;
  int* niter;
  int64_t env_base;  // first environment of this launch
  REAL tolerance, ls_gtol, scale;  // ls_gtol = tolerance * ls_tolerance; scale = meaninertia * max(1, nv)
  int nv, nefc, ne_nf, floss, newton, iterations, ls_iterations, fixed, warmstart;
  int chunk;  // rows of J per staging step
};

template <typename REAL>
struct SolveLds {
  REAL *Mp, *Lp, *J, *D, *fl, *jar, *jv, *f, *da, *x, *Ma, *grad, *Mgrad, *Mprev, *search, *mv, *fs, *as, *c, *red;
};

template <typename REAL>
__device__ __forceinline__ SolveLds<REAL> solve_lds(REAL* base, int nv, int n, bool newton) {
  SolveLds<REAL> s;
  const int tri = nv * (nv + 1) / 2;
  s.Mp = base;
  s.Lp = s.Mp + tri;
  s.J = s.Lp + tri;
  s.D = s.J + n * (nv | 1);
  s.fl = s.D + n;
  s.jar = s.fl + n;
  s.jv = s.jar + n;
  s.f = s.jv + n;
  s.da = s.f + n;  // (Newton only: CG's layout has no such array)
  s.x = s.da + (newton ? n : 0);
  s.Ma = s.x + nv;
  s.grad = s.Ma + nv;
  s.Mgrad = s.grad + nv;
  s.Mprev = s.Mgrad + nv;
  s.search = s.Mprev + nv;
  s.mv = s.search + nv;
  s.fs = s.mv + nv;
  s.as = s.fs + nv;
  s.c = s.as + nv;
  s.red = s.c + nv;  // 64 reals
  return s;
}

template <typename REAL>
struct LsPoint {
  REAL alpha, cost, d0, d1;
};

// y = M v from the packed lower triangle, a dof per lane, the sum in column order
template <typename REAL>
__device__ __forceinline__ void solve_mul_m(REAL* y, const REAL* Mp, const REAL* v, int nv, int l) {
  for (int i = l; i < nv; i += MJH_WAVE) {
    const REAL* Mi = Mp + i * (i + 1) / 2;
    REAL s = 0;
    for (int k = 0; k <= i; k++) s += Mi[k] * v[k];
    for (int k = i + 1; k < nv; k++) s += Mp[k * (k + 1) / 2 + i] * v[k];
    y[i] = s;
  }
}

// y = J v, a row per lane, the sum in column order
template <typename REAL>
__device__ __forceinline__ void solve_mul_j(REAL* y, const REAL* J, int ld, const REAL* v, int n, int nv, int l) {
  for (int r = l; r < n; r += MJH_WAVE) {
    const REAL* m = J + r * ld;
    REAL s = 0;
    for (int k = 0; k < nv; k++) s += m[k] * v[k];
    y[r] = s;
  }
}

// y <- (L L^T)^-1 y in place, Lp the packed lower triangle; the caller has synced, and syncs before it reads y
template <typename REAL>
__device__ __forceinline__ void solve_factored(REAL* y, const REAL* Lp, int nv, int l) {
  for (int i = 0; i < nv; i++) {  // L z = y: element k subtracts L[k][i] z[i] in i order
    const REAL zi = y[i] / Lp[i * (i + 1) / 2 + i];
    wave_sync();  // (every lane has read y[i] before it is overwritten)
    for (int k = i + 1 + l; k < nv; k += MJH_WAVE) y[k] = y[k] - Lp[k * (k + 1) / 2 + i] * zi;
    if (l == 0) y[i] = zi;
    wave_sync();
  }
  for (int i = nv - 1; i >= 0; i--) {  // L^T x = z
    const REAL* Li = Lp + i * (i + 1) / 2;
    const REAL xi = y[i] / Li[i];
    wave_sync();
    for (int k = l; k < i; k += MJH_WAVE) y[k] = y[k] - Li[k] * xi;
    if (l == 0) y[i] = xi;
    wave_sync();
  }
}

// Hp = Mp + J^T diag(da) J (packed lower triangles), an entry per lane, the sum in row order; a row of weight zero adds a zero and is passed over
template <typename REAL>
__device__ __forceinline__ void solve_hessian(REAL* Hp, const REAL* Mp, const REAL* J, int ld, const REAL* da, int n, int nv, int l) {
  const int tri = nv * (nv + 1) / 2;
  for (int t = l; t < tri; t += MJH_WAVE) {
    int i = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
    while ((i + 1) * (i + 2) / 2 <= t) i++;
    while (i * (i + 1) / 2 > t) i--;
    const int k = t - i * (i + 1) / 2;
    REAL s = 0;
    for (int r = 0; r < n; r++) {
      const REAL w = da[r];
      if (w == (REAL)0) continue;
      s += J[r * ld + i] * w * J[r * ld + k];
    }
    Hp[t] = Mp[t] + s;
  }
}

// the packed lower triangle Hp -> its Cholesky factor in place (math.small_cholesky's rule); the caller has synced
template <typename REAL>
__device__ __forceinline__ void solve_cholesky(REAL* Hp, int nv, int l) {
  const bool small = nv <= 16;
  for (int j = 0; j < nv; j++) {
    REAL* Hj = Hp + j * (j + 1) / 2;
    REAL s = small ? Hj[j] : Hj[j] + (REAL)1e-10;
    for (int k = 0; k < j; k++) s = s - Hj[k] * Hj[k];
    const REAL dj = r_sqrt<REAL>(small && s < (REAL)1e-12 ? (REAL)1e-12 : s);
    for (int i = j + 1 + l; i < nv; i += MJH_WAVE) {
      REAL* Hi = Hp + i * (i + 1) / 2;
      REAL t = Hi[j];
      for (int k = 0; k < j; k++) t = t - Hi[k] * Hj[k];
      Hi[j] = t / dj;
    }
    wave_sync();  // (every lane has read H[j][j] before it is overwritten)
    if (l == 0) Hj[j] = dj;
    wave_sync();
  }
}

// zones, forces (s.f; Newton: s.da) and J^T force (s.c) at s.jar; returns the cost, with `gauss` from s.Ma and s.x.  The caller has synced.
template <typename REAL>
__device__ __forceinline__ REAL solve_update(const SolveArgs<REAL>& a, const SolveLds<REAL>& s, int l, REAL& gauss) {
  const int nv = a.nv, n = a.nefc, ld = nv | 1;
  REAL quad = 0, lin = 0;
  for (int r = l; r < n; r += MJH_WAVE) {
    const REAL jar = s.jar[r], d = s.D[r], fr = s.fl[r];
    bool neg = false, pos = false;
    REAL rr = 0;
    if (a.floss && fr > 0) {
      rr = (REAL)1 / (d + (d == (REAL)0 ? (REAL)mjMINVAL : (REAL)0));
      neg = jar <= -rr * fr;
      pos = jar >= rr * fr;
    }
    const bool active = (r < a.ne_nf || jar < 0) && !neg && !pos;
    if (active) quad += d * jar * jar;
    if (neg) lin += (REAL)-0.5 * rr * fr * fr - fr * jar;
    if (pos) lin += (REAL)-0.5 * rr * fr * fr + fr * jar;
    s.f[r] = neg ? fr : (pos ? -fr : (active ? d * -jar : (REAL)0));
    if (a.newton) s.da[r] = active ? d : (REAL)0;
  }
  wave_sync();
  efc_jt_accumulate<REAL>(s.c, true, s.J, ld, s.f, n, nv, s.red, l);
  REAL g = 0;
  for (int k = l; k < nv; k += MJH_WAVE) g += (s.Ma[k] - s.fs[k]) * (s.x[k] - s.as[k]);
  gauss = (REAL)0.5 * wave_sum(g);
  REAL cost = (REAL)0.5 * wave_sum(quad);
  cost += gauss;
  cost += wave_sum(lin);
  wave_sync();  // (s.c is whole)
  return cost;
}

// s.x = src, s.jar = J x - aref, s.Ma = M x, then solve_update
template <typename REAL>
__device__ __forceinline__ REAL solve_context(const SolveArgs<REAL>& a, const SolveLds<REAL>& s, int l, const REAL* src, const REAL* aref, REAL& gauss) {
  const int nv = a.nv, n = a.nefc, ld = nv | 1;
  wave_sync();
  for (int k = l; k < nv; k += MJH_WAVE) s.x[k] = src[k];
  wave_sync();
  solve_mul_j<REAL>(s.jar, s.J, ld, s.x, n, nv, l);
  for (int r = l; r < n; r += MJH_WAVE) s.jar[r] = s.jar[r] - aref[r];  // (a lane's own rows)
  solve_mul_m<REAL>(s.Ma, s.Mp, s.x, nv, l);
  wave_sync();
  return solve_update<REAL>(a, s, l, gauss);
}

// s.grad, s.Mgrad from s.Ma and s.c (Newton: H and its factor in s.Lp first); returns |grad|^2.  The caller has synced.
template <typename REAL>
__device__ __forceinline__ REAL solve_gradient(const SolveArgs<REAL>& a, const SolveLds<REAL>& s, int l) {
  const int nv = a.nv, n = a.nefc, ld = nv | 1;
  REAL g2 = 0;
  for (int k = l; k < nv; k += MJH_WAVE) {
    const REAL g = s.Ma[k] - s.fs[k] - s.c[k];
    s.grad[k] = g;
    s.Mgrad[k] = g;
    g2 += g * g;
  }
  if (a.newton) {
    solve_hessian<REAL>(s.Lp, s.Mp, s.J, ld, s.da, n, nv, l);
    wave_sync();
    solve_cholesky<REAL>(s.Lp, nv, l);
  }
  wave_sync();
  solve_factored<REAL>(s.Mgrad, s.Lp, nv, l);
  return wave_sum(g2);
}

// N points of the line search in one pass over the rows; qg: (gauss, search . Ma - search . qfrc_smooth, 1/2 search . mv)
template <typename REAL, int N>
__device__ __forceinline__ void solve_points(const SolveArgs<REAL>& a, const SolveLds<REAL>& s, int l, REAL qg0, REAL qg1, REAL qg2, const REAL (&alpha)[N],
                                             LsPoint<REAL> (&out)[N]) {
  const int n = a.nefc;
  REAL s0[N], s1[N], s2[N];
#pragma unroll
  for (int p = 0; p < N; p++) s0[p] = s1[p] = s2[p] = 0;
  for (int r = l; r < n; r += MJH_WAVE) {
    const REAL jr = s.jar[r], v = s.jv[r], d = s.D[r];
    const REAL q0 = (REAL)0.5 * jr * jr * d, q1 = v * jr * d, q2 = (REAL)0.5 * v * v * d;
    REAL fr = 0, rf = 0;
    bool has = false;
    if (a.floss) {
      fr = s.fl[r];
      has = fr > 0;
      rf = (REAL)1 / (d + (d == (REAL)0 ? (REAL)mjMINVAL : (REAL)0)) * fr;
    }
#pragma unroll
    for (int p = 0; p < N; p++) {
      const REAL x = jr + alpha[p] * v;
      bool active = r < a.ne_nf || x < 0;
      if (has) {
        const bool ln = x <= -rf, lp = x >= rf;
        if (ln) { s0[p] += fr * ((REAL)-0.5 * rf - jr); s1[p] += -fr * v; }
        if (lp) { s0[p] += fr * ((REAL)-0.5 * rf + jr); s1[p] += fr * v; }
        active = active && !ln && !lp;
      }
      if (active) { s0[p] += q0; s1[p] += q1; s2[p] += q2; }
    }
  }
#pragma unroll
  for (int p = 0; p < N; p++) {
    const REAL t0 = qg0 + wave_sum(s0[p]), t1 = qg1 + wave_sum(s1[p]), t2 = qg2 + wave_sum(s2[p]), al = alpha[p];
    out[p].alpha = al;
    out[p].cost = al * al * t2 + al * t1 + t0;
    out[p].d0 = (REAL)2 * al * t2 + t1;
    out[p].d1 = (REAL)2 * t2 + (t2 == (REAL)0 ? (REAL)mjMINVAL : (REAL)0);
  }
}

// the candidate replaces the end when it narrows the bracket towards a zero derivative, or, while both ends' derivatives have one sign, when it is nearer to zero
template <typename REAL>
__device__ __forceinline__ bool solve_swap(LsPoint<REAL>& end, const LsPoint<REAL>& cand, bool not_bracketed) {
  const REAL x = end.d0, y = cand.d0;
  const bool take = (x < y && y < 0) || (x > y && y > 0) || (not_bracketed && r_abs<REAL>(y) < r_abs<REAL>(x));
  if (take) end = cand;
  return take;
}

// one exact line search along s.search: s.x, s.Ma, s.jar move (s.mv, s.jv are left behind).  The caller has synced.
template <typename REAL>
__device__ __forceinline__ void solve_linesearch(const SolveArgs<REAL>& a, const SolveLds<REAL>& s, int l, REAL gauss) {
  const int nv = a.nv, n = a.nefc, ld = nv | 1;
  solve_mul_m<REAL>(s.mv, s.Mp, s.search, nv, l);
  solve_mul_j<REAL>(s.jv, s.J, ld, s.search, n, nv, l);
  wave_sync();
  REAL ss = 0, sma = 0, sfs = 0, smv = 0;
  for (int k = l; k < nv; k += MJH_WAVE) {
    const REAL v = s.search[k];
    ss += v * v;
    sma += v * s.Ma[k];
    sfs += v * s.fs[k];
    smv += v * s.mv[k];
  }
  const REAL gtol = a.ls_gtol * (r_sqrt<REAL>(wave_sum(ss)) * a.scale);
  const REAL qg1 = wave_sum(sma) - wave_sum(sfs), qg2 = (REAL)0.5 * wave_sum(smv);
  LsPoint<REAL> one[1];
  const REAL zero[1] = {(REAL)0};
  solve_points<REAL, 1>(a, s, l, gauss, qg1, qg2, zero, one);
  const LsPoint<REAL> p0 = one[0];
  const REAL first[1] = {p0.alpha - p0.d0 / p0.d1};
  solve_points<REAL, 1>(a, s, l, gauss, qg1, qg2, first, one);
  const LsPoint<REAL> p1 = one[0];
  const bool lesser = p1.d0 < p0.d0;
  LsPoint<REAL> lo = lesser ? p1 : p0, hi = lesser ? p0 : p1;
  bool swap = !(r_abs<REAL>(p1.d0) < gtol);
  for (int it = 0; it < a.ls_iterations; it++) {
    if (!a.fixed && (!swap || (lo.d0 < 0 && lo.d0 > -gtol) || (hi.d0 > 0 && hi.d0 < gtol))) break;
    const REAL at[3] = {lo.alpha - lo.d0 / lo.d1, hi.alpha - hi.d0 / hi.d1, (REAL)0.5 * (lo.alpha + hi.alpha)};
    LsPoint<REAL> c[3];  // lo_next, hi_next, mid
    solve_points<REAL, 3>(a, s, l, gauss, qg1, qg2, at, c);
    const bool nb = (lo.d0 < 0) == (hi.d0 < 0);
    swap = solve_swap<REAL>(lo, c[0], nb);
    swap |= solve_swap<REAL>(lo, c[2], nb);
    swap |= solve_swap<REAL>(lo, c[1], nb);
    swap |= solve_swap<REAL>(hi, c[1], nb);
    swap |= solve_swap<REAL>(hi, c[2], nb);
    swap |= solve_swap<REAL>(hi, c[0], nb);
  }
  if (lo.cost < p0.cost || hi.cost < p0.cost) {
    const REAL alpha = lo.cost < hi.cost ? lo.alpha : hi.alpha;
    for (int k = l; k < nv; k += MJH_WAVE) {
      s.x[k] = s.x[k] + s.search[k] * alpha;
      s.Ma[k] = s.Ma[k] + s.mv[k] * alpha;
    }
    for (int r = l; r < n; r += MJH_WAVE) s.jar[r] = s.jar[r] + s.jv[r] * alpha;
  }
  wave_sync();
}

template <typename REAL>
__global__ __launch_bounds__(MJH_WAVE) void mjh_solve_kernel(SolveArgs<REAL> a) {
  extern __shared__ double solve_lds_raw[];
  const int l = (int)threadIdx.x, nv = a.nv, n = a.nefc, ld = nv | 1;
  const SolveLds<REAL> s = solve_lds<REAL>(reinterpret_cast<REAL*>(solve_lds_raw), nv, n, a.newton != 0);
  const int64_t e = a.env_base + blockIdx.x;
  const REAL* J = a.J + e * n * nv;
  const REAL* aref = a.aref + e * n;

  efc_load_triangle<REAL>(s.Mp, a.qM + e * nv * nv, nv, l);
  if (!a.newton) efc_load_triangle<REAL>(s.Lp, a.qLD + e * nv * nv, nv, l);
  for (int r0 = 0; r0 < n; r0 += a.chunk) {
    const int rows = n - r0 < a.chunk ? n - r0 : a.chunk;
    efc_load_rows<REAL>(s.J + r0 * ld, ld, J + (int64_t)r0 * nv, rows, nv, l);
  }
  for (int r = l; r < n; r += MJH_WAVE) { s.D[r] = a.D[e * n + r]; s.fl[r] = a.fl[e * n + r]; }
  for (int k = l; k < nv; k += MJH_WAVE) { s.fs[k] = a.qfrc_smooth[e * nv + k]; s.as[k] = a.qacc_smooth[e * nv + k]; }

  // the start: the smooth acceleration, or the warm start when its cost is strictly lower
  REAL gauss, cost;
  if (a.warmstart) {
    const REAL smooth = solve_context<REAL>(a, s, l, s.as, aref, gauss);
    cost = solve_context<REAL>(a, s, l, a.qacc_warmstart + e * nv, aref, gauss);
    if (!(cost < smooth)) cost = solve_context<REAL>(a, s, l, s.as, aref, gauss);
  } else {
    cost = solve_context<REAL>(a, s, l, s.as, aref, gauss);
  }
  REAL prev = (REAL)__builtin_huge_val();
  REAL g2 = solve_gradient<REAL>(a, s, l);
  wave_sync();
  for (int k = l; k < nv; k += MJH_WAVE) s.search[k] = -s.Mgrad[k];
  wave_sync();

  int niter = 0;
  for (;;) {
    if (a.iterations == 1) {
      if (niter >= 1) break;
    } else if (a.fixed) {
      if (niter >= a.iterations) break;
    } else if (niter >= a.iterations || (prev - cost) / a.scale < a.tolerance || r_sqrt<REAL>(g2) / a.scale < a.tolerance) {
      break;
    }
    solve_linesearch<REAL>(a, s, l, gauss);
    REAL pg = 0;  // grad_prev . Mgrad_prev
    for (int k = l; k < nv; k += MJH_WAVE) {
      const REAL mg = s.Mgrad[k];
      pg += s.grad[k] * mg;
      s.Mprev[k] = mg;
    }
    prev = cost;
    cost = solve_update<REAL>(a, s, l, gauss);
    g2 = solve_gradient<REAL>(a, s, l);
    wave_sync();
    if (a.newton) {
      for (int k = l; k < nv; k += MJH_WAVE) s.search[k] = -s.Mgrad[k];
    } else {
      REAL num = 0;
      for (int k = l; k < nv; k += MJH_WAVE) num += s.grad[k] * (s.Mgrad[k] - s.Mprev[k]);
      const REAL den = wave_sum(pg);
      REAL beta = wave_sum(num) / (den > (REAL)mjMINVAL ? den : (REAL)mjMINVAL);
      beta = beta > (REAL)0 ? beta : (REAL)0;
      for (int k = l; k < nv; k += MJH_WAVE) s.search[k] = -s.Mgrad[k] + beta * s.search[k];
    }
    wave_sync();
    niter++;
  }

  for (int k = l; k < nv; k += MJH_WAVE) {
    const REAL q = s.x[k];
    a.qacc[e * nv + k] = q;
    a.qacc_warmstart_out[e * nv + k] = q;
    a.qfrc_constraint[e * nv + k] = s.c[k];
  }
  for (int r = l; r < n; r += MJH_WAVE) a.force[e * n + r] = s.f[r];
  if (l == 0) {
    a.cost[e] = cost;
    a.improvement[e] = (prev - cost) / a.scale;
    a.grad_norm[e] = r_sqrt<REAL>(g2) / a.scale;
    a.niter[e] = niter;
  }
}
