// mjh_pgs.h -- the kernel behind mjh_pgs: a projected Gauss-Seidel solver of the dual problem of a finished pass (MuJoCo's mj_solPGS for rows of dimension
// one), min_f 1/2 f^T AR f + f^T b over the feasible set, AR = J (L L^T)^-1 J^T + diag(R) and b = J qacc_smooth - aref as mjh_efc_ar_kernel defines them -- without
// ever forming AR.  W, y, the LDS arrays, the staging, the ending (cost with its R term, qfrc_constraint, qacc), the order of every sum and what is uniform across
// the lanes: mjh_dual.h.  Here: the feasible set and the sweep.
//
// Feasible set: rows i < ne free; ne <= i < ne + nf: |f_i| <= frictionloss_i; later rows: f_i >= 0.  force0 (or zeros) is projected onto it first.  One sweep, rows in
// order, improvement = 0 at its start:
//     res = (w_i . y + R_i f_i) + b_i;  AR_ii <= 0: the row is skipped;  f_i <- project_i(f_i - res / AR_ii);  delta = the change;
//     improvement -= delta (1/2 delta AR_ii + res);  y += delta w_i
// then improvement *= inv_scale = 1 / (meaninertia max(1, nv)), niter += 1, and the environment stops when improvement < tolerance or niter == iterations: the loop
// is bounded by the argument.
// A row with w_i = 0 (w_i . w_i == 0: an inactive contact's) has nothing to sum and nothing to add to y; with f_i = 0 and b_i = 0 as well it cannot move and is
// passed over -- the same bits as visiting it.
#pragma once
#include "mjh_dual.h"

template <typename REAL>
struct PgsArgs : DualArgs<REAL> {};

template <typename REAL>
__device__ __forceinline__ REAL pgs_project(REAL v, int row, int ne, int ne_nf, REAL bound) {
  if (row < ne) return v;
  if (row < ne_nf) return v < -bound ? -bound : (v > bound ? bound : v);
  return v > (REAL)0 ? v : (REAL)0;
}

template <typename REAL>
__global__ __launch_bounds__(MJH_WAVE) void mjh_pgs_kernel(PgsArgs<REAL> a) {
  extern __shared__ double pgs_lds_raw[];
  const int l = (int)threadIdx.x, nv = a.nv, n = a.nefc, ld = nv | 1, ne = a.ne, ne_nf = a.ne + a.nf;
  const DualLds<REAL> s = dual_lds<REAL>(reinterpret_cast<REAL*>(pgs_lds_raw), nv, n);
  REAL *W = s.W, *R = s.R, *bb = s.b, *bound = s.bound, *ww = s.ww, *f = s.f, *y = s.y;
  const int64_t e = a.env_base + blockIdx.x;
  const REAL *J = a.J + e * n * nv, *as = a.qacc_smooth + e * nv;  // this environment's efc_J and qacc_smooth
  const REAL* f0 = a.force0 ? a.force0 + e * a.force0_env : nullptr;
  dual_stage<REAL>(a, s, e, J, as, l, [=](int row, REAL bd) { return pgs_project<REAL>(f0 ? f0[row] : (REAL)0, row, ne, ne_nf, bd); });
  wave_sync();

  int niter = 0;
  REAL improvement = 0;
  for (int it = 0; it < a.iterations; it++) {
    REAL imp = 0;
    for (int i = 0; i < n; i++) {
      const REAL wn = ww[i], ri = R[i], dg = wn + ri;
      if (!(dg > (REAL)0)) continue;
      const REAL old = f[i], bi = bb[i];
      const bool coupled = wn != (REAL)0;
      if (!coupled && old == (REAL)0 && bi == (REAL)0) continue;  // res = 0 and f stays 0: the rows of inactive contacts (J = 0, aref = 0)
      const REAL* wi = W + i * ld;
      REAL dot = 0;
      if (coupled) {  // (w_i = 0: the sum is a zero)
        REAL p = 0;
        for (int k = l; k < nv; k += MJH_WAVE) p += wi[k] * y[k];
        dot = wave_sum(p);
      }
      const REAL res = (dot + ri * old) + bi;
      const REAL fn = pgs_project<REAL>(old - res / dg, i, ne, ne_nf, bound[i]);
      const REAL delta = fn - old;
      imp -= delta * ((REAL)0.5 * delta * dg + res);
      if (delta != (REAL)0) {
        if (coupled)
          for (int k = l; k < nv; k += MJH_WAVE) y[k] += delta * wi[k];
        f[i] = fn;  // (every lane stores the same bits)
      }
    }
    wave_sync();
    niter++;
    improvement = imp * a.inv_scale;
    if (improvement < a.tolerance) break;
  }

  dual_finish<REAL, true>(a, s, e, J, as, l, niter, improvement);
}
