// mjh_pgs.h -- the kernel behind mjh_pgs: a projected Gauss-Seidel solver of the dual problem of a finished pass (MuJoCo's mj_solPGS for rows of dimension
// one), min_f 1/2 f^T AR f + f^T b over the feasible set, AR = J (L L^T)^-1 J^T + diag(R) and b = J qacc_smooth - aref as mjh_efc_ar_kernel defines them -- without
// ever forming AR.  Dense models only; one wavefront (the whole workgroup) per environment.
//
// With W = rows of (L^-1 J^T)^T -- what mjh_efc_ar_kernel forms chunk by chunk -- and y = sum_j f_j w_j, row i of AR f is w_i . y + R_i f_i, and a change of f_i
// by delta is y += delta w_i: O(nv) per row where a row of AR costs O(nefc), and nothing of size nefc x nv or nefc x nefc leaves the chip.
//
// LDS: the packed lower triangle of qLD, ALL of W (nefc rows of ld = nv | 1 reals), R, b, the friction bounds, w_i . w_i (AR_ii = w_i . w_i + R_i), f, y, J^T f
// and the 64 partial sums of efc_jt_accumulate.  efc_J is staged in chunks of `chunk` rows by efc_load_rows, straight into the chunk's place in W, where
// efc_forward_rows substitutes it in place (both are mjh_efc.h's); b_i is taken while the rows are still J's.
//
// Feasible set: rows i < ne free; ne <= i < ne + nf: |f_i| <= frictionloss_i; later rows: f_i >= 0.  force0 (or zeros) is projected onto it first.  One sweep, rows in
// order, improvement = 0 at its start:
//     res = (w_i . y + R_i f_i) + b_i;  AR_ii <= 0: the row is skipped;  f_i <- project_i(f_i - res / AR_ii);  delta = the change;
//     improvement -= delta (1/2 delta AR_ii + res);  y += delta w_i
// then improvement *= inv_scale = 1 / (meaninertia max(1, nv)), niter += 1, and the environment stops when improvement < tolerance or niter == iterations: the loop
// is bounded by the argument.  w_i . y: lane l sums k = l, l + 64, ... in ascending order, wave_sum adds the lanes in its fixed order -- an order that depends on nv
// alone.  Every lane carries the same scalars (wave_sum leaves the same bits in all of them), so the branches are wave-uniform; a lane updates the y_k it owns.
// A row with w_i = 0 (w_i . w_i == 0: an inactive contact's) has nothing to sum and nothing to add to y; with f_i = 0 and b_i = 0 as well it cannot move and is
// passed over -- the same bits as visiting it.
//
// Then: cost = 1/2 (y . y + sum_i R_i f_i^2) + f . b;  qfrc_constraint = J^T f, J streamed once more through the chunks by efc_jt_accumulate;
// qacc = qacc_smooth + L^-T y by a column-oriented back substitution (x_i = y_i / L_ii, then y_k -= L_ik x_i for k < i, one k per lane).
#pragma once
#include "mjh_efc.h"

template <typename REAL>
struct PgsArgs {
  const REAL *J, *D, *aref, *fl, *qLD, *qacc_smooth;  // [B, ...] leaves
  const REAL* force0;                                 // [nefc] per environment at element stride force0_env (0: shared); NULL: zeros
  REAL *force, *qfrc_constraint, *qacc, *cost, *improvement;
  int* niter;
  int64_t force0_env;
  int64_t env_base;  // first environment of this launch
  REAL tolerance, inv_scale;
  int nv, nefc, ne, nf, iterations;
  int chunk;  // rows of J per staging step
};

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
  REAL* Lp = reinterpret_cast<REAL*>(pgs_lds_raw);
  REAL* W = Lp + nv * (nv + 1) / 2;
  REAL* R = W + n * ld;
  REAL* bb = R + n;
  REAL* bound = bb + n;
  REAL* ww = bound + n;  // w_i . w_i: AR_ii = ww_i + R_i
  REAL* f = ww + n;
  REAL* y = f + n;
  REAL* c = y + nv;
  REAL* red = c + nv;  // 64 reals
  const int64_t e = a.env_base + blockIdx.x;
  const REAL* src = a.qLD + e * nv * nv;
  for (int t = l; t < nv * nv; t += MJH_WAVE) {  // every row whole (coalesced), its upper part dropped
    const int i = t / nv, k = t - i * nv;
    const REAL v = src[t];
    if (k <= i) Lp[i * (i + 1) / 2 + k] = v;
  }
  const REAL* J = a.J + e * n * nv;
  const REAL *D = a.D + e * n, *aref = a.aref + e * n, *fl = a.fl + e * n, *as = a.qacc_smooth + e * nv;
  const REAL* f0 = a.force0 ? a.force0 + e * a.force0_env : nullptr;
  for (int r0 = 0; r0 < n; r0 += a.chunk) {
    const int rows = n - r0 < a.chunk ? n - r0 : a.chunk;
    REAL* w = W + r0 * ld;
    efc_load_rows<REAL>(w, ld, J + (int64_t)r0 * nv, rows, nv, l);
    wave_sync();
    for (int r = l; r < rows; r += MJH_WAVE) {  // b, while the rows are still J's
      const REAL* m = w + r * ld;
      REAL s = 0;
      for (int k = 0; k < nv; k++) s += m[k] * as[k];
      bb[r0 + r] = s - aref[r0 + r];
    }
    efc_forward_rows<REAL>(w, ld, Lp, rows, nv, l);  // (a lane reads and writes its own rows only)
    for (int r = l; r < rows; r += MJH_WAVE) {
      const int row = r0 + r;
      const REAL* m = w + r * ld;
      REAL s = 0;
      for (int k = 0; k < nv; k++) s += m[k] * m[k];
      const REAL d = D[row], rr = d > 0 ? (REAL)1 / d : (REAL)0, bd = fl[row];
      R[row] = rr;
      ww[row] = s;
      bound[row] = bd;
      f[row] = pgs_project<REAL>(f0 ? f0[row] : (REAL)0, row, ne, ne_nf, bd);
    }
  }
  wave_sync();
  efc_jt_accumulate<REAL>(y, true, W, ld, f, n, nv, red, l);  // y = sum_j f_j w_j
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

  REAL yy = 0, rff = 0, fb = 0;
  for (int k = l; k < nv; k += MJH_WAVE) yy += y[k] * y[k];
  for (int i = l; i < n; i += MJH_WAVE) {
    const REAL fi = f[i];
    rff += R[i] * fi * fi;
    fb += fi * bb[i];
    a.force[e * n + i] = fi;
  }
  const REAL cost = (REAL)0.5 * (wave_sum(yy) + wave_sum(rff)) + wave_sum(fb);
  if (l == 0) { a.cost[e] = cost; a.improvement[e] = improvement; a.niter[e] = niter; }

  for (int r0 = 0; r0 < n; r0 += a.chunk) {  // J^T f: W is no longer needed, its first chunk stages J again
    const int rows = n - r0 < a.chunk ? n - r0 : a.chunk;
    wave_sync();
    efc_load_rows<REAL>(W, ld, J + (int64_t)r0 * nv, rows, nv, l);
    wave_sync();
    efc_jt_accumulate<REAL>(c, r0 == 0, W, ld, f + r0, rows, nv, red, l);
  }
  for (int k = l; k < nv; k += MJH_WAVE) a.qfrc_constraint[e * nv + k] = c[k];

  for (int i = nv - 1; i >= 0; i--) {  // L^T x = y in place
    const REAL* Li = Lp + i * (i + 1) / 2;
    wave_sync();
    const REAL xi = y[i] / Li[i];
    wave_sync();  // (every lane has read y[i] before it is overwritten)
    for (int k = l; k < i; k += MJH_WAVE) y[k] = y[k] - Li[k] * xi;
    if (l == 0) y[i] = xi;
  }
  wave_sync();
  for (int k = l; k < nv; k += MJH_WAVE) a.qacc[e * nv + k] = as[k] + y[k];
}
