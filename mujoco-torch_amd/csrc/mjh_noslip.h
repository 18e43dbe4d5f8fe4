// mjh_noslip.h -- the kernel behind mjh_noslip: MuJoCo's no-slip post-solver (mj_solNoSlip, `noslip_iterations`) on a finished pass: Gauss-Seidel sweeps on
// the UNREGULARISED matrix A = J (L L^T)^-1 J^T over the friction dimensions only -- friction-loss rows, the opposing edge pairs of pyramidal contacts, the
// tangential / torsional / rolling rows of elliptic contacts -- from the force the main solver left.  Every other row (equality, limit, frictionless contact rows,
// elliptic normals) is returned bit for bit.  Dense models only; one wavefront (the whole workgroup) per environment; the arguments, the LDS arrays,
// the staging and the ending are mjh_dual.h's.
//
// With W = rows of (L^-1 J^T)^T, y = sum_j f_j w_j, b = J qacc_smooth - aref, R = 1 / D where D > 0 else 0 as mjh_dual.h defines them: A_ij = w_i . w_j, the row
// residual is res_i = w_i . y + b_i, scale = 1 / (meaninertia max(1, nv)), MINVAL = 1e-15.  force0 is NOT projected.  One sweep, improvement = 0 at its start (the
// first sweep: 1/2 sum_i R_i f_i^2 over all rows, the cost of dropping the regulariser):
//   1. friction-loss rows ne <= i < ne + nf: A_ii < MINVAL: skipped; f_i <- clamp(f_i - res_i / A_ii, +-frictionloss_i); improvement -= delta (1/2 delta A_ii + res_i)
//   2. every contact of condim > 1 in slot order, block by block (a pyramidal contact: its dim - 1 pairs of opposing edges, rows (j, j + 1), one after the other; an
//      elliptic contact: its dim - 1 friction rows, the normal row i = first row untouched).  A_c: the block of A, bc = res - A_c f_old.
//        pair:     mid = (f_j + f_j+1) / 2, K1 = A_00 + A_11 - A_01 - A_10, K0 = mid (A_00 - A_11) + bc_0 - bc_1;  K1 < MINVAL: both become mid;  otherwise
//                  yy = -K0 / K1, yy < -mid -> -mid, yy > mid -> mid;  f_j = mid + yy, f_j+1 = mid - yy  (the pair's sum, the contact's normal force, is kept)
//        elliptic: f_i < MINVAL: the friction forces become 0;  otherwise v = argmin 1/2 v^T A_c v + v . bc subject to sum_k (v_k / mu_k)^2 <= f_i^2,
//                  mu = contact.friction[:dim - 1]: with v_k = mu_k u_k (A_s = mu_k A_c,km mu_m, b_s = mu_k bc_k) Newton on the multiplier lambda >= 0 of
//                  |u|^2 <= f_i^2 from lambda = 0, u = -(A_s + lambda I)^-1 b_s by a Cholesky factor, step = (|u|^2 - f_i^2) / (2 u . (A_s + lambda I)^-1 u), until
//                  |u|^2 <= f_i^2, or the step is not > 0, or lambda + step == lambda; at most 30 factorisations; a pivot that is not positive and finite gives
//                  v = 0; lambda > 0 (the constraint is active): v is put on the surface, v = mu u f_i / |u|
//      then change = 1/2 delta^T A_c delta + delta . res; change > 1e-10: the block is put back (change = 0); improvement -= change; y += sum_k delta_k w_k
// then improvement *= scale, niter += 1, and the environment stops when improvement < tolerance or niter == iterations: the loop is bounded by the argument.
// Outputs: cost = 1/2 y . y + f . b (no R term), qfrc_constraint = J^T f, qacc = qacc_smooth + L^-T y.
//
// LDS: mjh_dual.h's arrays, then per contact slot: the block(s) A_c, 15 reals (an elliptic contact: the packed lower triangle of its up to 5 x 5 block; a pyramidal
// one: A_00, A_01, A_11 of each pair), mu (5 reals), and the table (first row, condim) as two ints.  The blocks are constant over the sweeps: formed once, after W.
// The dot products of a block -- up to five residuals, or the i + 1 entries of row i of A_c -- go through ONE multi-value wave reduction (noslip_wave_sums: the DPP stages
// of wave_sum, every value at each stage before the next, so the chains overlap), lane l summing as mjh_dual.h has it.
// Every lane carries the same scalars; the pair update and the QCQP are scalar code on them, their branches go through noslip_uniform and the contact table's entries through readfirstlane
// (one lane's value, read as a scalar: no divergence); a lane updates the y_k it owns.
//
// Per environment, on top of mjh_dual.h's account: force0 and, with an elliptic cone, the friction of every contact slot in: read (2 nefc nv + nv^2 + 4 nefc + nv
// [+ 5 ncon]) reals (the account of mjh_model_kernel_io).
#pragma once
#include "mjh_dual.h"

#define MJH_NOSLIP_BLOCK 15       // reals of A_c per contact slot
#define MJH_NOSLIP_QCQP_ITERS 30  // factorisations of the multiplier's Newton iteration

template <typename REAL>
struct NoslipArgs : DualArgs<REAL> {  // (force0 is required)
  const REAL* friction;          // [B, ncon, 5] contact.friction (read for elliptic cones)
  const int *con_dim, *con_adr;  // the model's static contact tables (ncon)
  int ncon, elliptic;
};

// a condition every lane holds alike, as a scalar: the branch on it is uniform by construction
__device__ __forceinline__ bool noslip_uniform(bool c) { return __builtin_amdgcn_readfirstlane((int)c) != 0; }

// p[j] <- the sum over the lanes of p[j], j < N, the same bits in every lane and the bits wave_sum gives each value
template <typename REAL, int N>
__device__ __forceinline__ void noslip_wave_sums(REAL (&p)[N]) {
#ifdef MJH_NO_DPP
#pragma unroll
  for (int j = 0; j < N; j++) p[j] = wave_sum(p[j]);
#else
#pragma unroll
  for (int j = 0; j < N; j++) p[j] += dpp_move<0xB1>(p[j]);  // quad_perm [1,0,3,2]
#pragma unroll
  for (int j = 0; j < N; j++) p[j] += dpp_move<0x4E>(p[j]);  // quad_perm [2,3,0,1]
#pragma unroll
  for (int j = 0; j < N; j++) p[j] += dpp_move<0x141>(p[j]);  // row_half_mirror
#pragma unroll
  for (int j = 0; j < N; j++) p[j] += dpp_move<0x140>(p[j]);  // row_mirror
#pragma unroll
  for (int j = 0; j < N; j++) p[j] = ((read_lane(p[j], 0) + read_lane(p[j], 16)) + read_lane(p[j], 32)) + read_lane(p[j], 48);
#endif
}

// res[j] = w_(row0 + j) . y + b_(row0 + j), j < N: one reduction for the block
template <typename REAL, int N>
__device__ __forceinline__ void noslip_residuals(REAL (&res)[N], const REAL* W, int ld, const REAL* y, const REAL* bb, int row0, int nv, int l) {
#pragma unroll
  for (int j = 0; j < N; j++) res[j] = 0;
  const REAL* w0 = W + row0 * ld;
  for (int k = l; k < nv; k += MJH_WAVE) {
    const REAL yk = y[k];
#pragma unroll
    for (int j = 0; j < N; j++) res[j] += w0[j * ld + k] * yk;
  }
  noslip_wave_sums<REAL, N>(res);
#pragma unroll
  for (int j = 0; j < N; j++) res[j] += bb[row0 + j];
}

// y += sum_j delta_j w_(row0 + j), a lane its own y_k, j ascending; f_(row0 + j) = v_j (every lane stores the same bits)
template <typename REAL, int N>
__device__ __forceinline__ void noslip_accept(const REAL (&v)[N], const REAL (&delta)[N], const REAL* W, int ld, REAL* y, REAL* f, int row0, int nv, int l) {
#pragma unroll
  for (int j = 0; j < N; j++) {
    if (noslip_uniform(delta[j] != (REAL)0)) {
      const REAL* wj = W + (row0 + j) * ld;
      for (int k = l; k < nv; k += MJH_WAVE) y[k] += delta[j] * wj[k];
      f[row0 + j] = v[j];
    }
  }
}

// row I of the packed lower triangle of the N x N block of A at rows row0 ..: its I + 1 entries in one reduction, then the rows below it
template <typename REAL, int N, int I>
__device__ __forceinline__ void noslip_form_rows(REAL* blk, const REAL* w0, int ld, int nv, int l) {
  REAL p[I + 1];
#pragma unroll
  for (int j = 0; j <= I; j++) p[j] = 0;
  for (int k = l; k < nv; k += MJH_WAVE) {
    const REAL wik = w0[I * ld + k];
#pragma unroll
    for (int j = 0; j <= I; j++) p[j] += wik * w0[j * ld + k];
  }
  noslip_wave_sums<REAL, I + 1>(p);
  if (l == 0) {
#pragma unroll
    for (int j = 0; j <= I; j++) blk[I * (I + 1) / 2 + j] = p[j];
  }
  if constexpr (I + 1 < N) noslip_form_rows<REAL, N, I + 1>(blk, w0, ld, nv, l);
}

// the packed lower triangle (row i at i (i + 1) / 2) of the N x N block of A at rows row0 ..
template <typename REAL, int N>
__device__ __forceinline__ void noslip_form_block(REAL* blk, const REAL* W, int ld, int row0, int nv, int l) {
  noslip_form_rows<REAL, N, 0>(blk, W + row0 * ld, ld, nv, l);
}

// change = 1/2 delta^T A_c delta + delta . res, A_c the packed lower triangle
template <typename REAL, int N>
__device__ __forceinline__ REAL noslip_change(const REAL* blk, const REAL (&delta)[N], const REAL (&res)[N]) {
  REAL q = 0, lin = 0;
#pragma unroll
  for (int i = 0; i < N; i++) {
    REAL s = 0;
#pragma unroll
    for (int j = 0; j < N; j++) s += blk[i >= j ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i] * delta[j];
    q += delta[i] * s;
    lin += delta[i] * res[i];
  }
  return (REAL)0.5 * q + lin;
}

// the Cholesky factor (packed lower rows) of A_s + lambda I; false: a pivot was not positive and finite
template <typename REAL, int N>
__device__ __forceinline__ bool noslip_chol(const REAL (&As)[N * (N + 1) / 2], REAL la, REAL (&L)[N * (N + 1) / 2]) {
  bool ok = true;
#pragma unroll
  for (int i = 0; i < N; i++) {
#pragma unroll
    for (int j = 0; j <= i; j++) {
      REAL s = As[i * (i + 1) / 2 + j];
      if (i == j) s = s + la;
#pragma unroll
      for (int k = 0; k < j; k++) s = s - L[i * (i + 1) / 2 + k] * L[j * (j + 1) / 2 + k];
      if (i == j) {
        ok = ok && s > (REAL)0 && s < (REAL)INFINITY;
        L[i * (i + 1) / 2 + i] = r_sqrt<REAL>(ok ? s : (REAL)1);
      } else {
        L[i * (i + 1) / 2 + j] = s / L[j * (j + 1) / 2 + j];
      }
    }
  }
  return ok;
}

template <typename REAL, int N>
__device__ __forceinline__ void noslip_lower_solve(const REAL (&L)[N * (N + 1) / 2], const REAL (&x)[N], REAL (&out)[N]) {
#pragma unroll
  for (int i = 0; i < N; i++) {
    REAL s = x[i];
#pragma unroll
    for (int k = 0; k < i; k++) s = s - L[i * (i + 1) / 2 + k] * out[k];
    out[i] = s / L[i * (i + 1) / 2 + i];
  }
}

template <typename REAL, int N>
__device__ __forceinline__ void noslip_upper_solve(const REAL (&L)[N * (N + 1) / 2], const REAL (&x)[N], REAL (&out)[N]) {
#pragma unroll
  for (int i = N - 1; i >= 0; i--) {
    REAL s = x[i];
#pragma unroll
    for (int k = i + 1; k < N; k++) s = s - L[k * (k + 1) / 2 + i] * out[k];
    out[i] = s / L[i * (i + 1) / 2 + i];
  }
}

// v = argmin 1/2 v^T A_c v + v . bc subject to sum (v_k / mu_k)^2 <= r^2 (the header has the iteration); blk: A_c, packed
template <typename REAL, int N>
__device__ __forceinline__ void noslip_qcqp(REAL (&v)[N], const REAL* blk, const REAL (&bc)[N], const REAL* mu, REAL r) {
  REAL As[N * (N + 1) / 2], L[N * (N + 1) / 2], m[N], nbs[N], u[N], z[N];
#pragma unroll
  for (int i = 0; i < N; i++) {
    m[i] = mu[i];
    nbs[i] = -(bc[i] * m[i]);
    u[i] = 0;
  }
#pragma unroll
  for (int i = 0; i < N; i++)
#pragma unroll
    for (int j = 0; j <= i; j++) As[i * (i + 1) / 2 + j] = blk[i * (i + 1) / 2 + j] * m[i] * m[j];
  REAL la = 0;
  bool bad = false;
  for (int it = 0; it < MJH_NOSLIP_QCQP_ITERS; it++) {
    if (noslip_uniform(!noslip_chol<REAL, N>(As, la, L))) { bad = true; break; }
    noslip_lower_solve<REAL, N>(L, nbs, z);
    noslip_upper_solve<REAL, N>(L, z, u);
    REAL uu = 0, ww = 0;
#pragma unroll
    for (int i = 0; i < N; i++) uu += u[i] * u[i];
    const REAL val = uu - r * r;
    noslip_lower_solve<REAL, N>(L, u, z);
#pragma unroll
    for (int i = 0; i < N; i++) ww += z[i] * z[i];
    const REAL step = val / ((REAL)2 * ww), nw = la + step;
    if (noslip_uniform(val <= (REAL)0 || !(step > (REAL)0) || nw == la)) break;
    la = nw;
  }
  REAL uu = 0;
#pragma unroll
  for (int i = 0; i < N; i++) uu += u[i] * u[i];
  const REAL scale = (la > (REAL)0 && uu > (REAL)0) ? r / r_sqrt<REAL>(uu) : (REAL)1;
#pragma unroll
  for (int i = 0; i < N; i++) v[i] = bad ? (REAL)0 : u[i] * m[i] * scale;
}

// the dim - 1 = N friction rows of an elliptic contact whose normal row is `adr`; returns the accepted cost change
template <typename REAL, int N>
__device__ __forceinline__ REAL noslip_elliptic(const REAL* blk, const REAL* mu, const REAL* W, int ld, REAL* y, REAL* f, const REAL* bb, int adr, int nv, int l) {
  REAL res[N], old[N], bc[N], v[N], delta[N];
  noslip_residuals<REAL, N>(res, W, ld, y, bb, adr + 1, nv, l);
#pragma unroll
  for (int j = 0; j < N; j++) old[j] = f[adr + 1 + j];
#pragma unroll
  for (int i = 0; i < N; i++) {
    REAL s = 0;
#pragma unroll
    for (int j = 0; j < N; j++) s += blk[i >= j ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i] * old[j];
    bc[i] = res[i] - s;
  }
  const REAL fn = f[adr];
  if (noslip_uniform(fn < (REAL)1e-15)) {
#pragma unroll
    for (int j = 0; j < N; j++) v[j] = 0;
  } else {
    noslip_qcqp<REAL, N>(v, blk, bc, mu, fn);
  }
#pragma unroll
  for (int j = 0; j < N; j++) delta[j] = v[j] - old[j];
  const REAL change = noslip_change<REAL, N>(blk, delta, res);
  if (noslip_uniform(change > (REAL)1e-10)) return (REAL)0;  // put back: nothing was stored
  noslip_accept<REAL, N>(v, delta, W, ld, y, f, adr + 1, nv, l);
  return change;
}

// one pair of opposing pyramid edges, rows (j, j + 1); blk: A_00, A_01, A_11; returns the accepted cost change
template <typename REAL>
__device__ __forceinline__ REAL noslip_pair(const REAL* blk, const REAL* W, int ld, REAL* y, REAL* f, const REAL* bb, int j, int nv, int l) {
  REAL res[2], v[2], delta[2];
  noslip_residuals<REAL, 2>(res, W, ld, y, bb, j, nv, l);
  const REAL o0 = f[j], o1 = f[j + 1], a00 = blk[0], a01 = blk[1], a11 = blk[2];
  const REAL bc0 = res[0] - (a00 * o0 + a01 * o1), bc1 = res[1] - (a01 * o0 + a11 * o1);
  const REAL mid = (REAL)0.5 * (o0 + o1);
  const REAL K1 = a00 + a11 - a01 - a01, K0 = mid * (a00 - a11) + bc0 - bc1;
  if (K1 < (REAL)1e-15) {
    v[0] = mid;
    v[1] = mid;
  } else {
    REAL yy = -K0 / K1;
    yy = yy < -mid ? -mid : (yy > mid ? mid : yy);
    v[0] = mid + yy;
    v[1] = mid - yy;
  }
  delta[0] = v[0] - o0;
  delta[1] = v[1] - o1;
  const REAL q = delta[0] * (a00 * delta[0] + a01 * delta[1]) + delta[1] * (a01 * delta[0] + a11 * delta[1]);
  const REAL change = (REAL)0.5 * q + (delta[0] * res[0] + delta[1] * res[1]);
  if (noslip_uniform(change > (REAL)1e-10)) return (REAL)0;
  noslip_accept<REAL, 2>(v, delta, W, ld, y, f, j, nv, l);
  return change;
}

template <typename REAL>
__global__ __launch_bounds__(MJH_WAVE) void mjh_noslip_kernel(NoslipArgs<REAL> a) {
  extern __shared__ double noslip_lds_raw[];
  const int l = (int)threadIdx.x, nv = a.nv, n = a.nefc, ld = nv | 1, ne = a.ne, ne_nf = a.ne + a.nf, nc = a.ncon;
  const DualLds<REAL> s = dual_lds<REAL>(reinterpret_cast<REAL*>(noslip_lds_raw), nv, n);
  REAL *W = s.W, *R = s.R, *bb = s.b, *bound = s.bound, *ww = s.ww, *f = s.f, *y = s.y;  // (ww_i = A_ii)
  REAL* blk = s.end;                               // MJH_NOSLIP_BLOCK reals per contact slot
  REAL* mu = blk + MJH_NOSLIP_BLOCK * nc;          // 5 reals per contact slot
  int* tab = reinterpret_cast<int*>(mu + 5 * nc);  // (first row, condim) per contact slot
  const int64_t e = a.env_base + blockIdx.x;
  for (int t = l; t < nc; t += MJH_WAVE) {
    tab[2 * t] = a.con_adr[t];
    tab[2 * t + 1] = a.con_dim[t];
  }
  if (a.elliptic)
    for (int t = l; t < 5 * nc; t += MJH_WAVE) mu[t] = a.friction[e * 5 * nc + t];
  const REAL *J = a.J + e * n * nv, *as = a.qacc_smooth + e * nv;  // this environment's efc_J and qacc_smooth
  const REAL* f0 = a.force0 + e * a.force0_env;
  dual_stage<REAL>(a, s, e, J, as, l, [=](int row, REAL) { return f0[row]; });
  for (int ci = 0; ci < nc; ci++) {  // the blocks of A: constant over the sweeps
    const int adr = __builtin_amdgcn_readfirstlane(tab[2 * ci]), dim = __builtin_amdgcn_readfirstlane(tab[2 * ci + 1]);  // (scalars: the dispatch below is uniform)
    REAL* bk = blk + MJH_NOSLIP_BLOCK * ci;
    if (dim < 2 || dim > 6) continue;  // (condim is 1, 3, 4 or 6: 15 reals hold the block(s) of any of them)
    if (a.elliptic) {
      if (dim == 3) noslip_form_block<REAL, 2>(bk, W, ld, adr + 1, nv, l);
      else if (dim == 4) noslip_form_block<REAL, 3>(bk, W, ld, adr + 1, nv, l);
      else if (dim == 6) noslip_form_block<REAL, 5>(bk, W, ld, adr + 1, nv, l);
    } else {
      for (int p = 0; p < dim - 1; p++) noslip_form_block<REAL, 2>(bk + 3 * p, W, ld, adr + 2 * p, nv, l);
    }
  }
  wave_sync();

  int niter = 0;
  REAL improvement = 0;
  for (int it = 0; it < a.iterations; it++) {
    REAL imp = 0;
    if (it == 0) {  // the cost of dropping the regulariser
      REAL rff = 0;
      for (int i = l; i < n; i += MJH_WAVE) rff += R[i] * f[i] * f[i];
      imp = (REAL)0.5 * wave_sum(rff);
    }
    for (int i = ne; i < ne_nf; i++) {
      const REAL aii = ww[i];
      if (aii < (REAL)1e-15) continue;
      const REAL* wi = W + i * ld;
      REAL p = 0;
      for (int k = l; k < nv; k += MJH_WAVE) p += wi[k] * y[k];
      const REAL res = wave_sum(p) + bb[i], old = f[i], bd = bound[i];
      REAL fn = old - res / aii;
      fn = fn < -bd ? -bd : (fn > bd ? bd : fn);
      const REAL delta = fn - old;
      imp -= delta * ((REAL)0.5 * delta * aii + res);
      if (noslip_uniform(delta != (REAL)0)) {
        for (int k = l; k < nv; k += MJH_WAVE) y[k] += delta * wi[k];
        f[i] = fn;  // (every lane stores the same bits)
      }
    }
    for (int ci = 0; ci < nc; ci++) {
      const int adr = __builtin_amdgcn_readfirstlane(tab[2 * ci]), dim = __builtin_amdgcn_readfirstlane(tab[2 * ci + 1]);
      const REAL* bk = blk + MJH_NOSLIP_BLOCK * ci;
      if (dim < 2 || dim > 6) continue;
      if (a.elliptic) {
        const REAL* m = mu + 5 * ci;
        if (dim == 3) imp -= noslip_elliptic<REAL, 2>(bk, m, W, ld, y, f, bb, adr, nv, l);
        else if (dim == 4) imp -= noslip_elliptic<REAL, 3>(bk, m, W, ld, y, f, bb, adr, nv, l);
        else if (dim == 6) imp -= noslip_elliptic<REAL, 5>(bk, m, W, ld, y, f, bb, adr, nv, l);
      } else {
        for (int p = 0; p < dim - 1; p++) imp -= noslip_pair<REAL>(bk + 3 * p, W, ld, y, f, bb, adr + 2 * p, nv, l);
      }
    }
    wave_sync();
    niter++;
    improvement = imp * a.inv_scale;
    if (improvement < a.tolerance) break;
  }
  wave_sync();

  dual_finish<REAL, false>(a, s, e, J, as, l, niter, improvement);
}
