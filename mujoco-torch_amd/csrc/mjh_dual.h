// mjh_dual.h -- what the two dual solvers of a finished pass share, mjh_pgs_kernel (mjh_pgs.h) and mjh_noslip_kernel (mjh_noslip.h): their arguments, their LDS layout,
// their staging and their ending.  The sweeps between staging and ending are each kernel's own.  Dense models only; one wavefront (the whole workgroup) per environment.
//
// Definitions, as mjh_efc_ar_kernel has them (mjh_efc.h): W = rows of (L^-1 J^T)^T, L = qLD -- what mjh_efc_ar_kernel forms chunk by chunk --, R = 1 / D where D > 0 else 0,
// b = J qacc_smooth - aref, A = W W^T and AR = A + diag(R).  Neither matrix is ever formed: with y = sum_j f_j w_j, row i of A f is w_i . y (of AR f: w_i . y + R_i f_i), and
// a change of f_i by delta is y += delta w_i: O(nv) per row where a row of AR costs O(nefc), and nothing of size nefc x nv or nefc x nefc leaves the chip.
//
// LDS (dual_lds), in this order: the packed lower triangle of qLD, ALL of W (nefc rows of ld = nv | 1 reals -- an odd stride, so the lanes that walk down a column of rows in
// efc_forward_rows hit different banks, while the sweeps read rows along k, consecutive lanes consecutive reals --), R, b, the friction bounds, w_i . w_i (A_ii; AR_ii =
// w_i . w_i + R_i), f, y, c = J^T f and red, the 64 partial sums of efc_jt_accumulate; `end`: where a kernel's own arrays start (mjh_noslip.h's blocks, mu and table).
//
// Staging (dual_stage): qLD's triangle (efc_load_triangle); then efc_J in chunks of `chunk` rows by efc_load_rows, straight into the chunk's place in W, where efc_rows_b takes
// b_i of them first and efc_forward_rows then substitutes them in place (all mjh_efc.h's); then, a row per lane, R_i, w_i . w_i (columns in order), the
// bound and the start force f_i = start(i, bound_i), the caller's (mjh_pgs.h: force0 or zeros, projected; mjh_noslip.h: force0 as it is); then y = sum_j f_j w_j by
// efc_jt_accumulate.  The caller syncs before it reads y.
//
// Ending (dual_finish), after the caller's last sync: cost = 1/2 (y . y + sum_i R_i f_i^2) + f . b, the R term only WITH_R; efc_force = f; cost, improvement and niter from
// lane 0; qfrc_constraint = J^T f, J streamed once more through the chunks by efc_jt_accumulate (W is no longer needed: its first chunk stages them);
// qacc = qacc_smooth + L^-T y by a column-oriented back substitution (x_i = y_i / L_ii, then y_k -= L_ik x_i for k < i, one k per lane).
//
// Sums over k < nv or i < nefc, here and in the sweeps: lane l sums k = l, l + 64, ... in ascending order, wave_sum adds the lanes in its fixed order -- an order that depends
// on nv (nefc) alone.  Every lane carries the same scalars (wave_sum leaves the same bits in all of them), so branches on them are wave-uniform; a lane updates the y_k it owns.
//
// Per environment: efc_J twice (W, then J^T f), qLD, D, aref, frictionloss, qacc_smooth and what the start reads in; efc_force, qfrc_constraint, qacc, cost, improvement,
// niter out: read (2 nefc nv + nv^2 + 3 nefc + nv) reals and the start's, written (nefc + 2 nv + 2) reals + 4 bytes (the account of mjh_model_kernel_io).
#pragma once
#include "mjh_efc.h"

template <typename REAL>
struct DualArgs {
  const REAL *J, *D, *aref, *fl, *qLD, *qacc_smooth;  // [B, ...] leaves
  const REAL* force0;                                 // [nefc] per environment at element stride force0_env (0: shared); NULL (mjh_pgs alone): zeros
  REAL *force, *qfrc_constraint, *qacc, *cost, *improvement;
  int* niter;
  int64_t force0_env;
  int64_t env_base;  // first environment of this launch
  REAL tolerance, inv_scale;
  int nv, nefc, ne, nf, iterations;
  int chunk;  // rows of J per staging step
};

template <typename REAL>
struct DualLds {
  REAL *Lp, *W, *R, *b, *bound, *ww, *f, *y, *c, *red, *end;
};

template <typename REAL>
__device__ __forceinline__ DualLds<REAL> dual_lds(REAL* base, int nv, int n) {
  DualLds<REAL> s;
  s.Lp = base;
  s.W = s.Lp + nv * (nv + 1) / 2;
  s.R = s.W + n * (nv | 1);
  s.b = s.R + n;
  s.bound = s.b + n;
  s.ww = s.bound + n;  // w_i . w_i
  s.f = s.ww + n;
  s.y = s.f + n;
  s.c = s.y + nv;
  s.red = s.c + nv;  // 64 reals
  s.end = s.red + MJH_WAVE;
  return s;
}

template <typename REAL, typename START>
__device__ __forceinline__ void dual_stage(const DualArgs<REAL>& a, const DualLds<REAL>& s, int64_t e, const REAL* J, const REAL* as, int l, START start) {
  const int nv = a.nv, n = a.nefc, ld = nv | 1;
  efc_load_triangle<REAL>(s.Lp, a.qLD + e * nv * nv, nv, l);
  const REAL *D = a.D + e * n, *aref = a.aref + e * n, *fl = a.fl + e * n;
  for (int r0 = 0; r0 < n; r0 += a.chunk) {
    const int rows = n - r0 < a.chunk ? n - r0 : a.chunk;
    REAL* w = s.W + r0 * ld;
    efc_load_rows<REAL>(w, ld, J + (int64_t)r0 * nv, rows, nv, l);
    wave_sync();
    efc_rows_b<REAL>(s.b + r0, w, ld, as, aref + r0, rows, nv, l);
    efc_forward_rows<REAL>(w, ld, s.Lp, rows, nv, l);  // (a lane reads and writes its own rows only)
    for (int r = l; r < rows; r += MJH_WAVE) {
      const int row = r0 + r;
      const REAL* m = w + r * ld;
      REAL ss = 0;
      for (int k = 0; k < nv; k++) ss += m[k] * m[k];
      const REAL d = D[row], bd = fl[row];
      s.R[row] = d > 0 ? (REAL)1 / d : (REAL)0;
      s.ww[row] = ss;
      s.bound[row] = bd;
      s.f[row] = start(row, bd);
    }
  }
  wave_sync();
  efc_jt_accumulate<REAL>(s.y, true, s.W, ld, s.f, n, nv, s.red, l);  // y = sum_j f_j w_j
}

template <typename REAL, bool WITH_R>
__device__ __forceinline__ void dual_finish(const DualArgs<REAL>& a, const DualLds<REAL>& s, int64_t e, const REAL* J, const REAL* as, int l, int niter, REAL improvement) {
  const int nv = a.nv, n = a.nefc, ld = nv | 1;
  REAL yy = 0, rff = 0, fb = 0;
  for (int k = l; k < nv; k += MJH_WAVE) yy += s.y[k] * s.y[k];
  for (int i = l; i < n; i += MJH_WAVE) {
    const REAL fi = s.f[i];
    if constexpr (WITH_R) rff += s.R[i] * fi * fi;
    fb += fi * s.b[i];
    a.force[e * n + i] = fi;
  }
  REAL cost;
  if constexpr (WITH_R) cost = (REAL)0.5 * (wave_sum(yy) + wave_sum(rff)) + wave_sum(fb);
  else cost = (REAL)0.5 * wave_sum(yy) + wave_sum(fb);
  if (l == 0) { a.cost[e] = cost; a.improvement[e] = improvement; a.niter[e] = niter; }

  for (int r0 = 0; r0 < n; r0 += a.chunk) {  // J^T f: W is no longer needed, its first chunk stages J again
    const int rows = n - r0 < a.chunk ? n - r0 : a.chunk;
    wave_sync();
    efc_load_rows<REAL>(s.W, ld, J + (int64_t)r0 * nv, rows, nv, l);
    wave_sync();
    efc_jt_accumulate<REAL>(s.c, r0 == 0, s.W, ld, s.f + r0, rows, nv, s.red, l);
  }
  for (int k = l; k < nv; k += MJH_WAVE) a.qfrc_constraint[e * nv + k] = s.c[k];

  for (int i = nv - 1; i >= 0; i--) {  // L^T x = y in place
    const REAL* Li = s.Lp + i * (i + 1) / 2;
    wave_sync();
    const REAL xi = s.y[i] / Li[i];
    wave_sync();  // (every lane has read y[i] before it is overwritten)
    for (int k = l; k < i; k += MJH_WAVE) s.y[k] = s.y[k] - Li[k] * xi;
    if (l == 0) s.y[i] = xi;
  }
  wave_sync();
  for (int k = l; k < nv; k += MJH_WAVE) a.qacc[e * nv + k] = as[k] + s.y[k];
}
