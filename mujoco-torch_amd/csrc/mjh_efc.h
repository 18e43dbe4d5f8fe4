// mjh_efc.h -- the kernels behind mjh_constraint_space: the constraint problem of a finished pass in constraint space (MuJoCo's mj_mulJacVec,
// mj_mulJacTVec, mj_constraintUpdate and the Delassus matrix efc_AR; the definitions are the reference solver's, mujoco_torch/_src/solver.py:293-357, 501-508).
// Dense models only.  Every kernel runs one wavefront (the whole workgroup) per environment and streams efc_J from global memory through LDS in chunks of
// `chunk` rows, by flat coalesced loads; a staged row takes ld = nv | 1 reals, so that lanes walking down a column of rows hit different banks.
//
// mjh_efc_mulj_kernel:  y_j = J x_j for the K vectors of the environment.  Lanes take (vector, row) pairs row-fastest; a row's sum runs in column order.
// mjh_efc_muljt_kernel: y_j = J^T f_j, vector by vector through efc_jt_accumulate: up to 32 dofs the rows of a chunk are split over lane groups whose partial
//   sums are added in a fixed order; the partial sum of the chunks so far is the output element itself.
// mjh_efc_update_kernel: one pass over J.  While a chunk is staged: jar = J qacc - aref of its rows (or the caller's jar), the zone of every row
//     r = 1 / (D + (D == 0) mjMINVAL);  linear-neg: fl > 0 and jar <= -r fl;  linear-pos: fl > 0 and jar >= r fl   (both only with `floss`)
//     quadratic: (row < ne_nf or jar < 0) and not linear;  satisfied otherwise                       state 2 / 3 / 1 / 0 (MuJoCo's mjtConstraintState)
//   its force (-D jar, +fl, -fl, 0), the row's cost term, and J^T force accumulated in LDS (efc_jt_accumulate).  Then, with qacc: M qacc through the same staging
//   buffer, gauss = 1/2 (M qacc - qfrc_smooth) . (qacc - qacc_smooth), grad = M qacc - qfrc_smooth - J^T force, grad_norm = |grad| * inv_scale.
//   cost = (1/2 sum_quadratic D jar^2 + gauss) + sum_linear (-1/2 r fl^2 -/+ fl jar): lane-partial sums over the lane's rows in ascending order, then wave_sum.
// mjh_efc_ar_kernel: AR = J (L L^T)^-1 J^T + diag(R), R = 1 / D where D > 0 else 0, and b = J qacc_smooth - aref.  The packed lower triangle of qLD stays in
//   LDS.  A chunk of rows of J is turned into W = rows of (L^-1 J^T)^T in place, one row per lane by forward substitution (element i subtracts L[i][k] w[k] in
//   k order, as math.small_cholesky_solve does), so that AR[i][j] = w_i . w_j.  Chunk a against itself gives the diagonal block, against every later chunk b
//   (staged and substituted into the second buffer) the off-diagonal blocks: each entry is computed once and stored to both triangles.  Neither W nor any
//   other (nefc, nv) intermediate goes to global memory; chunk b's rows of J are read again for every a < b.  Its triangle load, its b and its substitution (efc_load_triangle, efc_rows_b,
//   efc_forward_rows) are also the staging of the dual solvers, which keep ALL of W on chip (mjh_dual.h).
#pragma once
#include "mjh_device.h"

template <typename REAL>
struct EfcArgs {
  const REAL *J, *D, *aref, *fl, *qM, *qLD, *qfrc_smooth, *qacc_smooth, *qacc, *jar_in;  // [B, ...] leaves and overrides (jar_in: UPDATE without qacc)
  const REAL* vec;                                                                    // MUL_J / MUL_JT queries, addressed by vec_env / vec_k (0: shared)
  REAL *out, *jar, *force, *qfrc_constraint, *cost, *gauss, *grad, *grad_norm, *AR, *b;
  int* state;
  int64_t vec_env, vec_k;
  int64_t env_base;  // first environment of this launch
  REAL inv_scale;    // 1 / (meaninertia * max(1, nv))
  int nv, nefc, K, ne_nf, floss;
  int chunk;         // rows of J (UPDATE: and of qM) per LDS chunk
};

// rows [0, rows) x nv of a contiguous row-major matrix -> LDS rows of ld reals; consecutive lanes read consecutive addresses
template <typename REAL>
__device__ __forceinline__ void efc_load_rows(REAL* dst, int ld, const REAL* src, int rows, int nv, int l) {
  const int n = rows * nv;
  int i = l / nv, k = l - i * nv;
  for (int t = l; t < n; t += MJH_WAVE) {
    dst[i * ld + k] = src[t];
    k += MJH_WAVE;
    while (k >= nv) { k -= nv; i++; }
  }
}

// acc[k] += sum_r rows[r][k] f[r], k < nv, for `rows` staged rows (acc may be global memory: the lane that stores an element is the one that reads it back; `first`:
// nothing to read back yet).  Up to 32 dofs the wavefront is split into G = 64 / P groups of P lanes (P: nv rounded up to a power of two), group g sums the
// rows r = g, g + G, ... in ascending order and the G partial sums are added in group order through `red` (64 reals of LDS); past 32 dofs a lane owns a dof and
// sums every row in order.  Either way the order depends on nv and the chunk alone: not on the batch, the launch cut or the number of vectors.
template <typename REAL>
__device__ __forceinline__ void efc_jt_accumulate(REAL* acc, bool first, const REAL* buf, int ld, const REAL* f, int rows, int nv, REAL* red, int l) {
  if (nv > 32) {
    for (int k = l; k < nv; k += MJH_WAVE) {
      REAL s = first ? (REAL)0 : acc[k];
      for (int r = 0; r < rows; r++) s += buf[r * ld + k] * f[r];
      acc[k] = s;
    }
    return;
  }
  int P = 1;
  while (P < nv) P <<= 1;
  const int G = MJH_WAVE / P, g = l / P, k = l - g * P;
  REAL s = 0;
  if (k < nv)
    for (int r = g; r < rows; r += G) s += buf[r * ld + k] * f[r];
  red[l] = s;
  wave_sync();
  if (l < nv) {
    REAL t = first ? (REAL)0 : acc[l];
    for (int q = 0; q < G; q++) t += red[q * P + l];
    acc[l] = t;
  }
  wave_sync();  // (red is free again)
}

template <typename REAL>
__global__ __launch_bounds__(MJH_WAVE) void mjh_efc_mulj_kernel(EfcArgs<REAL> a) {
  extern __shared__ double efc_lds_raw[];
  REAL* buf = reinterpret_cast<REAL*>(efc_lds_raw);
  const int l = (int)threadIdx.x, nv = a.nv, n = a.nefc, K = a.K, ld = nv | 1;
  const int64_t e = a.env_base + blockIdx.x;
  const REAL* J = a.J + e * n * nv;
  const REAL* x0 = a.vec + e * a.vec_env;
  REAL* y = a.out + e * K * n;
  for (int r0 = 0; r0 < n; r0 += a.chunk) {
    const int rows = n - r0 < a.chunk ? n - r0 : a.chunk;
    efc_load_rows<REAL>(buf, ld, J + (int64_t)r0 * nv, rows, nv, l);
    wave_sync();
    for (int t = l; t < K * rows; t += MJH_WAVE) {
      const int j = t / rows, r = t - j * rows;
      const REAL* x = x0 + j * a.vec_k;
      const REAL* m = buf + r * ld;
      REAL s = 0;
      for (int k = 0; k < nv; k++) s += m[k] * x[k];
      y[(int64_t)j * n + r0 + r] = s;
    }
    wave_sync();
  }
}

template <typename REAL>
__global__ __launch_bounds__(MJH_WAVE) void mjh_efc_muljt_kernel(EfcArgs<REAL> a) {
  extern __shared__ double efc_lds_raw[];
  REAL* buf = reinterpret_cast<REAL*>(efc_lds_raw);
  const int l = (int)threadIdx.x, nv = a.nv, n = a.nefc, K = a.K, ld = nv | 1;
  const int64_t e = a.env_base + blockIdx.x;
  const REAL* J = a.J + e * n * nv;
  const REAL* f0 = a.vec + e * a.vec_env;
  REAL* y = a.out + e * K * nv;
  REAL* red = buf + a.chunk * ld;  // 64 reals
  for (int r0 = 0; r0 < n; r0 += a.chunk) {
    const int rows = n - r0 < a.chunk ? n - r0 : a.chunk;
    efc_load_rows<REAL>(buf, ld, J + (int64_t)r0 * nv, rows, nv, l);
    wave_sync();
    for (int j = 0; j < K; j++) efc_jt_accumulate<REAL>(y + (int64_t)j * nv, r0 == 0, buf, ld, f0 + j * a.vec_k + r0, rows, nv, red, l);
    wave_sync();
  }
}

template <typename REAL>
__global__ __launch_bounds__(MJH_WAVE) void mjh_efc_update_kernel(EfcArgs<REAL> a) {
  extern __shared__ double efc_lds_raw[];
  const int l = (int)threadIdx.x, nv = a.nv, n = a.nefc, ld = nv | 1;
  REAL* x = reinterpret_cast<REAL*>(efc_lds_raw);  // qacc
  REAL* c = x + nv;                                // J^T force
  REAL* y = c + nv;                                // M qacc
  REAL* f = y + nv;                                // the forces of the current chunk
  REAL* buf = f + a.chunk;                         // chunk rows of J, then of qM
  REAL* red = buf + a.chunk * ld;                  // 64 reals: the partial sums of efc_jt_accumulate
  const int64_t e = a.env_base + blockIdx.x;
  const bool with_qacc = a.qacc != nullptr;
  for (int i = l; i < nv; i += MJH_WAVE) { x[i] = with_qacc ? a.qacc[e * nv + i] : (REAL)0; c[i] = 0; }
  wave_sync();

  const REAL* J = a.J + e * n * nv;
  const REAL *D = a.D + e * n, *aref = a.aref + e * n, *fl = a.fl + e * n;
  REAL quad = 0, lin = 0;  // this lane's rows: sum D jar^2 over the quadratic ones, the cost terms of the linear ones
  for (int r0 = 0; r0 < n; r0 += a.chunk) {
    const int rows = n - r0 < a.chunk ? n - r0 : a.chunk;
    efc_load_rows<REAL>(buf, ld, J + (int64_t)r0 * nv, rows, nv, l);
    wave_sync();
    for (int r = l; r < rows; r += MJH_WAVE) {
      const int row = r0 + r;
      REAL jar;
      if (with_qacc) {
        const REAL* m = buf + r * ld;
        REAL s = 0;
        for (int k = 0; k < nv; k++) s += m[k] * x[k];
        jar = s - aref[row];
        a.jar[e * n + row] = jar;
      } else {
        jar = a.jar_in[e * n + row];
      }
      const REAL d = D[row], fr = fl[row];
      bool neg = false, pos = false;
      REAL rr = 0;
      if (a.floss && fr > 0) {
        rr = (REAL)1 / (d + (d == (REAL)0 ? (REAL)1e-15 : (REAL)0));  // mjMINVAL
        neg = jar <= -rr * fr;
        pos = jar >= rr * fr;
      }
      const bool active = (row < a.ne_nf || jar < 0) && !neg && !pos;
      const REAL force = neg ? fr : (pos ? -fr : (active ? d * -jar : (REAL)0));
      if (active) quad += d * jar * jar;
      if (neg) lin += (REAL)-0.5 * rr * fr * fr - fr * jar;
      if (pos) lin += (REAL)-0.5 * rr * fr * fr + fr * jar;
      f[r] = force;
      a.force[e * n + row] = force;
      a.state[e * n + row] = neg ? 2 : (pos ? 3 : (active ? 1 : 0));
    }
    wave_sync();
    efc_jt_accumulate<REAL>(c, false, buf, ld, f, rows, nv, red, l);
    wave_sync();
  }
  for (int k = l; k < nv; k += MJH_WAVE) a.qfrc_constraint[e * nv + k] = c[k];
  REAL cost = (REAL)0.5 * wave_sum(quad);
  const REAL lin_all = wave_sum(lin);

  if (with_qacc) {
    const REAL* qM = a.qM + e * nv * nv;
    for (int r0 = 0; r0 < nv; r0 += a.chunk) {
      const int rows = nv - r0 < a.chunk ? nv - r0 : a.chunk;
      efc_load_rows<REAL>(buf, ld, qM + (int64_t)r0 * nv, rows, nv, l);
      wave_sync();
      for (int r = l; r < rows; r += MJH_WAVE) {
        const REAL* m = buf + r * ld;
        REAL s = 0;
        for (int k = 0; k < nv; k++) s += m[k] * x[k];
        y[r0 + r] = s;
      }
      wave_sync();
    }
    REAL g = 0, g2 = 0;
    for (int k = l; k < nv; k += MJH_WAVE) {
      const REAL ms = y[k] - a.qfrc_smooth[e * nv + k];
      g += ms * (x[k] - a.qacc_smooth[e * nv + k]);
      const REAL gr = ms - c[k];
      a.grad[e * nv + k] = gr;
      g2 += gr * gr;
    }
    const REAL gauss = (REAL)0.5 * wave_sum(g);
    const REAL norm = r_sqrt<REAL>(wave_sum(g2)) * a.inv_scale;
    cost += gauss;
    if (l == 0) { a.gauss[e] = gauss; a.grad_norm[e] = norm; }
  }
  cost += lin_all;
  if (l == 0) a.cost[e] = cost;
}

// qLD (nv x nv, row-major) -> its packed lower triangle in LDS, row i at i (i + 1) / 2: every row is read whole (coalesced), its upper part dropped
template <typename REAL>
__device__ __forceinline__ void efc_load_triangle(REAL* Lp, const REAL* src, int nv, int l) {
  for (int t = l; t < nv * nv; t += MJH_WAVE) {
    const int i = t / nv, k = t - i * nv;
    const REAL v = src[t];
    if (k <= i) Lp[i * (i + 1) / 2 + k] = v;
  }
}

// b[r] = w_r . qacc_smooth - aref[r] of the staged rows while the rows are still J's (before efc_forward_rows), one row per lane, its sum in column order; b may
// be LDS or global memory
template <typename REAL>
__device__ __forceinline__ void efc_rows_b(REAL* b, const REAL* w, int ld, const REAL* as, const REAL* aref, int rows, int nv, int l) {
  for (int r = l; r < rows; r += MJH_WAVE) {
    const REAL* m = w + r * ld;
    REAL s = 0;
    for (int k = 0; k < nv; k++) s += m[k] * as[k];
    b[r] = s - aref[r];
  }
}

// the rows of `w` (rows x ld, J's rows on entry) -> L^-1 J_r^T, one row per lane; Lp: the packed lower triangle, row i at i (i + 1) / 2
template <typename REAL>
__device__ __forceinline__ void efc_forward_rows(REAL* w, int ld, const REAL* Lp, int rows, int nv, int l) {
  for (int r = l; r < rows; r += MJH_WAVE) {
    REAL* wr = w + r * ld;
    for (int i = 0; i < nv; i++) {
      const REAL* Li = Lp + i * (i + 1) / 2;
      REAL s = wr[i];
      for (int k = 0; k < i; k++) s = s - Li[k] * wr[k];
      wr[i] = s / Li[i];
    }
  }
}

template <typename REAL>
__global__ __launch_bounds__(MJH_WAVE) void mjh_efc_ar_kernel(EfcArgs<REAL> a) {
  extern __shared__ double efc_lds_raw[];
  const int l = (int)threadIdx.x, nv = a.nv, n = a.nefc, ld = nv | 1;
  REAL* Lp = reinterpret_cast<REAL*>(efc_lds_raw);
  REAL* wa = Lp + nv * (nv + 1) / 2;
  REAL* wb = wa + a.chunk * ld;  // (used, and allocated, only when there is more than one chunk)
  const int64_t e = a.env_base + blockIdx.x;
  efc_load_triangle<REAL>(Lp, a.qLD + e * nv * nv, nv, l);
  const REAL* J = a.J + e * n * nv;
  const REAL *D = a.D + e * n, *aref = a.aref + e * n, *as = a.qacc_smooth + e * nv;
  REAL* AR = a.AR + e * n * n;
  for (int a0 = 0; a0 < n; a0 += a.chunk) {
    const int ra = n - a0 < a.chunk ? n - a0 : a.chunk;
    efc_load_rows<REAL>(wa, ld, J + (int64_t)a0 * nv, ra, nv, l);
    wave_sync();
    efc_rows_b<REAL>(a.b + e * n + a0, wa, ld, as, aref + a0, ra, nv, l);
    efc_forward_rows<REAL>(wa, ld, Lp, ra, nv, l);  // (a lane reads and writes its own rows only)
    wave_sync();
    // Blocks go out in tiles of 8 x 8 entries, one entry per lane: the store of an entry and the store of its mirror image then both cover runs of 8
    // consecutive reals.  The diagonal block: the tiles on and above the diagonal, entries j >= i.
    const int ta = (ra + 7) >> 3;
    for (int ti = 0; ti < ta; ti++)
      for (int tj = ti; tj < ta; tj++) {
        const int i = ti * 8 + (l >> 3), j = tj * 8 + (l & 7);
        if (i >= ra || j >= ra || j < i) continue;
        const REAL *wi = wa + i * ld, *wj = wa + j * ld;
        REAL s = 0;
        for (int k = 0; k < nv; k++) s += wi[k] * wj[k];
        if (i == j) {
          const REAL d = D[a0 + i];
          s += d > 0 ? (REAL)1 / d : (REAL)0;
        }
        AR[(int64_t)(a0 + i) * n + a0 + j] = s;
        if (i != j) AR[(int64_t)(a0 + j) * n + a0 + i] = s;
      }
    for (int b0 = a0 + a.chunk; b0 < n; b0 += a.chunk) {
      const int rb = n - b0 < a.chunk ? n - b0 : a.chunk;
      wave_sync();  // (the previous block's reads of wb are done)
      efc_load_rows<REAL>(wb, ld, J + (int64_t)b0 * nv, rb, nv, l);
      wave_sync();
      efc_forward_rows<REAL>(wb, ld, Lp, rb, nv, l);
      wave_sync();
      const int tb = (rb + 7) >> 3;
      for (int t = 0; t < ta * tb; t++) {
        const int ti = t / tb, i = ti * 8 + (l >> 3), j = (t - ti * tb) * 8 + (l & 7);
        if (i >= ra || j >= rb) continue;
        const REAL *wi = wa + i * ld, *wj = wb + j * ld;
        REAL s = 0;
        for (int k = 0; k < nv; k++) s += wi[k] * wj[k];
        AR[(int64_t)(a0 + i) * n + b0 + j] = s;
        AR[(int64_t)(b0 + j) * n + a0 + i] = s;
      }
    }
    wave_sync();
  }
}
