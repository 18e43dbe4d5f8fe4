// mjh_support.h -- the kernels behind mjh_support: functions that read a finished forward pass and return a tensor
// (reference mujoco_torch/_src/support.py: jac :138-153, apply_ft :169-181, xfrc_accumulate :184-194; smooth.py: mul_m :370-374, solve_m :335-338
// with math.small_cholesky_solve :132-168).  Dense models only.
//
// mjh_sup_point_kernel<REAL, JAC>: one lane per output element, environment-major, 256 lanes per workgroup.  JAC: element (env, query, dof, k) of
//   jacp / jacr ([B, P, nv, 3] each), so consecutive lanes store consecutive addresses of both outputs.  !JAC (apply_ft): element (env, query, dof);
//   the lane forms its dof's three jacp / jacr entries in registers and stores jacp . force + jacr . torque: J is never written.
// mjh_sup_xfrc_kernel: one lane per (env, dof); the body loop runs in body order, as the whole-pass kernel's xfrc_accumulate does.
// mjh_sup_mulm_kernel / mjh_sup_solvem_kernel: one wavefront (the whole workgroup) per environment.  qM (row chunks) or qLD (its lower triangle,
//   packed) is loaded from HBM once, by flat coalesced loads into LDS, and serves all K vectors of the environment.
// Per element, jac is the reference's arithmetic: offset = point - subtree_com[root], cross (math.py:63-76), (cdof[3:] + cross) * mask, cdof[:3] * mask.
#pragma once
#include "mjh_device.h"
#include "mjh_inverse.h"

#define MJH_SUP_WG 256

template <typename REAL>
struct SupArgs {
  const REAL *cdof, *subtree_com, *xipos, *xfrc, *mat;   // [B, ...] leaves (mat: qM for mul_m, qLD for solve_m)
  const REAL *point, *force, *torque, *vec;              // queries, addressed by the strides below (0: shared)
  const int* body;                                       // query body ids (body_stride 1), or one id (0)
  const unsigned long long* body_dofmask;                // model: nbody * mask_words
  const int* body_rootid;                                // model: nbody
  REAL *out0, *out1;
  int64_t point_env, point_q, force_env, force_q, torque_env, torque_q, vec_env, vec_k;
  int64_t env_base;   // first environment of this launch
  int r_base;         // (point / xfrc kernels) element of env_base the launch starts at
  int count;          // (point / xfrc kernels) elements of this launch
  int body_stride, nv, nbody, mask_words, P, K;
  int chunk;          // mul_m: qM rows per LDS chunk; solve_m: vectors per LDS chunk
};

// the ancestor mask of `body` at `dof` as the reference's 0 / 1 multiplier
template <typename REAL>
__device__ __forceinline__ REAL sup_mask(const SupArgs<REAL>& a, int body, int dof) {
  return (REAL)((a.body_dofmask[(int64_t)body * a.mask_words + (dof >> 6)] >> (dof & 63)) & 1ull);
}

// jacp / jacr of `point` on `body` at one dof of environment e
template <typename REAL>
__device__ __forceinline__ void sup_jac_dof(const SupArgs<REAL>& a, int64_t e, const REAL* point, int body, int dof, REAL* jp, REAL* jr) {
  const REAL on = sup_mask(a, body, dof);
  const REAL* rc = a.subtree_com + (e * a.nbody + a.body_rootid[body]) * 3;
  const REAL off[3] = {point[0] - rc[0], point[1] - rc[1], point[2] - rc[2]};
  const REAL* cd = a.cdof + (e * a.nv + dof) * 6;
  REAL c[3];
  cross3(cd, off, c);
#pragma unroll
  for (int i = 0; i < 3; i++) { jp[i] = (cd[3 + i] + c[i]) * on; jr[i] = cd[i] * on; }
}

template <typename REAL, bool JAC>
__global__ __launch_bounds__(MJH_SUP_WG) void mjh_sup_point_kernel(SupArgs<REAL> a) {
  const unsigned l = blockIdx.x * MJH_SUP_WG + threadIdx.x;
  if (l >= (unsigned)a.count) return;
  const unsigned per_q = JAC ? 3u * a.nv : (unsigned)a.nv, per_env = per_q * a.P;
  const unsigned lr = (unsigned)a.r_base + l;
  const unsigned er = lr / per_env, r = lr - er * per_env;
  const unsigned p = r / per_q, rq = r - p * per_q;
  const int64_t e = a.env_base + er;
  const int body = a.body[p * a.body_stride];
  const REAL* pt = a.point + e * a.point_env + p * a.point_q;
  const int64_t o = (e * a.P + p) * per_q + rq;  // output index
  if (JAC) {
    const unsigned dof = rq / 3, k = rq - dof * 3;
    const REAL on = sup_mask(a, body, (int)dof);
    const REAL* rc = a.subtree_com + (e * a.nbody + a.body_rootid[body]) * 3;
    const REAL off[3] = {pt[0] - rc[0], pt[1] - rc[1], pt[2] - rc[2]};
    const REAL* cd = a.cdof + (e * a.nv + dof) * 6;
    const unsigned k1 = k == 2 ? 0 : k + 1, k2 = k == 0 ? 2 : k - 1;
    const REAL c = cd[k1] * off[k2] - cd[k2] * off[k1];  // math.cross, component k
    a.out0[o] = (cd[3 + k] + c) * on;
    a.out1[o] = cd[k] * on;
  } else {
    REAL jp[3], jr[3];
    sup_jac_dof(a, e, pt, body, (int)rq, jp, jr);
    const REAL* f = a.force + e * a.force_env + p * a.force_q;
    const REAL* t = a.torque + e * a.torque_env + p * a.torque_q;
    a.out0[o] = (jp[0] * f[0] + jp[1] * f[1] + jp[2] * f[2]) + (jr[0] * t[0] + jr[1] * t[1] + jr[2] * t[2]);
  }
}

template <typename REAL>
__global__ __launch_bounds__(MJH_SUP_WG) void mjh_sup_xfrc_kernel(SupArgs<REAL> a) {
  const unsigned l = blockIdx.x * MJH_SUP_WG + threadIdx.x;
  if (l >= (unsigned)a.count) return;
  const unsigned lr = (unsigned)a.r_base + l;
  const unsigned er = lr / (unsigned)a.nv, dof = lr - er * (unsigned)a.nv;
  const int64_t e = a.env_base + er;
  REAL acc = 0;
  for (int b = 0; b < a.nbody; b++) {
    const REAL* f = a.xfrc + (e * a.nbody + b) * 6;
    REAL jp[3], jr[3];
    sup_jac_dof(a, e, a.xipos + (e * a.nbody + b) * 3, b, (int)dof, jp, jr);
    acc += (jp[0] * f[0] + jp[1] * f[1] + jp[2] * f[2]) + (jr[0] * f[3] + jr[1] * f[4] + jr[2] * f[5]);
  }
  a.out0[e * a.nv + dof] = acc;
}

// y_j = qM x_j for the K vectors of one environment; qM streams through LDS in chunks of `chunk` rows, each chunk serving every vector.
// Lanes take (vector, row) pairs row-fastest, so the stores of a pass are consecutive; a row's sum runs in column order.
template <typename REAL>
__global__ __launch_bounds__(MJH_WAVE) void mjh_sup_mulm_kernel(SupArgs<REAL> a) {
  extern __shared__ double sup_lds_raw[];
  REAL* buf = reinterpret_cast<REAL*>(sup_lds_raw);
  const int l = (int)threadIdx.x, nv = a.nv, K = a.K;
  const int64_t e = a.env_base + blockIdx.x;
  const REAL* qM = a.mat + e * nv * nv;
  const REAL* x0 = a.vec + e * a.vec_env;
  REAL* y = a.out0 + e * K * nv;
  for (int r0 = 0; r0 < nv; r0 += a.chunk) {
    const int rows = nv - r0 < a.chunk ? nv - r0 : a.chunk;
    inv_load<REAL>(buf, qM + (int64_t)r0 * nv, rows * nv, l, MJH_WAVE);
    wave_sync();
    for (int t = l; t < K * rows; t += MJH_WAVE) {
      const int j = t / rows, r = t - j * rows;
      const REAL* x = x0 + j * a.vec_k;
      const REAL* m = buf + r * nv;
      REAL s = 0;
      for (int k = 0; k < nv; k++) s += m[k] * x[k];
      y[(int64_t)j * nv + r0 + r] = s;
    }
    wave_sync();
  }
}

// x_j = (L L^T)^-1 b_j (math.small_cholesky_solve) for the K vectors of one environment, L = qLD's lower triangle, packed in LDS.  Column-oriented
// substitution over `chunk` vectors at a time held in LDS: step k divides entry k of every vector by L[k][k], then every lane subtracts L[i][k] times it
// from its entries i > k (forward) or L[k][i] times it from its entries i < k (backward).  Forward, an entry's subtractions run in the reference's
// order (k ascending); backward they run k descending, where the reference's row loop runs ascending.
template <typename REAL>
__global__ __launch_bounds__(MJH_WAVE) void mjh_sup_solvem_kernel(SupArgs<REAL> a) {
  extern __shared__ double sup_lds_raw[];
  REAL* Lp = reinterpret_cast<REAL*>(sup_lds_raw);  // row i at i (i + 1) / 2
  const int l = (int)threadIdx.x, nv = a.nv, K = a.K;
  REAL* w = Lp + nv * (nv + 1) / 2;                 // chunk vectors of nv
  const int64_t e = a.env_base + blockIdx.x;
  const REAL* src = a.mat + e * nv * nv;
  for (int t = l; t < nv * nv; t += MJH_WAVE) {     // every row whole (coalesced), its upper part dropped
    const int i = t / nv, k = t - i * nv;
    const REAL v = src[t];
    if (k <= i) Lp[i * (i + 1) / 2 + k] = v;
  }
  const REAL* b0 = a.vec + e * a.vec_env;
  REAL* y = a.out0 + e * K * nv;
  for (int j0 = 0; j0 < K; j0 += a.chunk) {
    const int nj = K - j0 < a.chunk ? K - j0 : a.chunk, n = nj * nv;
    for (int t = l; t < n; t += MJH_WAVE) {
      const int j = t / nv, i = t - j * nv;
      w[t] = b0[(int64_t)(j0 + j) * a.vec_k + i];
    }
    wave_sync();
    for (int k = 0; k < nv; k++) {  // L y = b
      const REAL dk = Lp[k * (k + 1) / 2 + k];
      for (int j = l; j < nj; j += MJH_WAVE) w[j * nv + k] = w[j * nv + k] / dk;
      wave_sync();
      for (int t = l; t < n; t += MJH_WAVE) {
        const int j = t / nv, i = t - j * nv;
        if (i > k) w[t] = w[t] - Lp[i * (i + 1) / 2 + k] * w[j * nv + k];
      }
      wave_sync();
    }
    for (int k = nv - 1; k >= 0; k--) {  // L^T x = y
      const REAL dk = Lp[k * (k + 1) / 2 + k];
      for (int j = l; j < nj; j += MJH_WAVE) w[j * nv + k] = w[j * nv + k] / dk;
      wave_sync();
      const REAL* row = Lp + k * (k + 1) / 2;
      for (int t = l; t < n; t += MJH_WAVE) {
        const int j = t / nv, i = t - j * nv;
        if (i < k) w[t] = w[t] - row[i] * w[j * nv + k];
      }
      wave_sync();
    }
    for (int t = l; t < n; t += MJH_WAVE) y[(int64_t)j0 * nv + t] = w[t];
    wave_sync();
  }
}
