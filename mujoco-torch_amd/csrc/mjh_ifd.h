// mjh_ifd.h -- the kernels around the passes of a finite-difference Jacobian of inverse dynamics (mjh_ifd_perturb, mjh_ifd_difference; MuJoCo's
// mjd_inverseFD).  The passes themselves are plain mjh_inverse calls over the perturbed environments.
//
// Columns: c in [0, nv) nudges qpos along dof c (tangent space), [nv, 2 nv) qvel, [2 nv, 3 nv) qacc.  Nothing else is perturbed.  A call serves the
// columns [col0, col0 + ncol) of every environment, in the slot layout of mjh_fd.h:  w = (e * ncol + (c - col0)) * nside + side,  nside = 1
// (centered: 2), side 0 nudged by +eps, side 1 by -eps.  The column is decoded from w: there is no column list in memory.
//
// mjh_ifd_perturb_kernel: one workgroup per slot.  It streams every listed input leaf of environment e into slot w (4-byte words, consecutive lanes on
//   consecutive addresses), then one lane nudges the slot's entry by mjh_fd_perturb_kernel's rule: x + h for qvel / qacc and slide / hinge /
//   free-translation dofs, quat_integrate(q, e_k, h) for the rotational dofs of ball / free joints.
// mjh_ifd_difference_kernel: one lane per (environment, row, column of the chunk), column fastest, so that a wave's stores run along a row of
//   DfDq / DfDv / DfDa (DsDq / DsDv / DsDa) for as many columns as the chunk holds.  Rows [0, nv): qfrc_inverse, then, with the sensor matrices,
//   sensordata.  No row is a quaternion: every entry is  (y+ - y0) / eps  or, centered,  (y+ - y-) / (2 eps).
// Both move far fewer bytes than the passes between them: a slot's input leaves, and nv + nsensordata outputs per slot.
#pragma once
#include "mjh_fd.h"

#define MJH_IFD_PERTURB_WG 64
#define MJH_IFD_DIFF_WG 256

template <typename REAL>
struct IfdPerturbArgs {
  const int *dof_jntid, *jnt_type, *jnt_qposadr, *jnt_dofadr;
  const REAL *qpos, *qvel, *qacc;       // the caller's [B, nq], [B, nv], [B, nv]
  REAL *p_qpos, *p_qvel, *p_qacc;       // the scratch batch's [slots, ...]
  REAL eps;
  int nq, nv;
  int centered, col0, ncol;
  int nleaf;
  int64_t first;                        // first slot of this launch
  int64_t total;                        // slots of the call
  FdLeaf leaf[MJH_FD_MAX_LEAVES];
};

template <typename REAL>
struct IfdDiffArgs {
  const REAL *f0, *s0;                  // the nominal pass: qfrc_inverse [B, nv], sensordata [B, nsd]
  const REAL *f, *s;                    // the perturbed passes: [slots, nv], [slots, nsd]
  REAL *DfDq, *DfDv, *DfDa;             // [B, nv, nv]
  REAL *DsDq, *DsDv, *DsDa;             // [B, nsd, nv]
  REAL eps;
  int nv, nsd;                          // nsd: 0 when the sensor matrices are not asked for
  int centered, col0, ncol;
  int64_t first;                        // first entry of this launch
  int64_t total;                        // entries of the call: B * (nv + nsd) * ncol
};

template <typename REAL>
__global__ __launch_bounds__(MJH_IFD_PERTURB_WG) void mjh_ifd_perturb_kernel(IfdPerturbArgs<REAL> a) {
  const int64_t w = a.first + blockIdx.x;
  if (w >= a.total) return;
  const int nside = a.centered ? 2 : 1, nslot = a.ncol * nside;
  const int64_t e = w / nslot;
  const int sl = (int)(w - e * nslot);
  for (int l = 0; l < a.nleaf; l++) {
    const FdLeaf L = a.leaf[l];
    unsigned* dst = L.dst + w * L.words;
    const unsigned* src = L.src + e * L.words;
    for (int i = threadIdx.x; i < L.words; i += MJH_IFD_PERTURB_WG) dst[i] = src[i];
  }
  __syncthreads();  // the nudged entry is stored over its copy
  if (threadIdx.x != 0) return;
  const int col = a.col0 + sl / nside, side = sl - (sl / nside) * nside;
  const int nv = a.nv;
  const REAL h = side ? -a.eps : a.eps;
  if (col < nv) {
    int adr, axis;
    fd_dof(a.dof_jntid, a.jnt_type, a.jnt_qposadr, a.jnt_dofadr, col, adr, axis);
    const REAL* q = a.qpos + e * a.nq + adr;
    REAL* o = a.p_qpos + w * a.nq + adr;
    if (axis < 0) {
      o[0] = q[0] + h;
    } else {
      const REAL q4[4] = {q[0], q[1], q[2], q[3]}, t[3] = {(REAL)(axis == 0), (REAL)(axis == 1), (REAL)(axis == 2)};
      REAL r[4];
      quat_integrate(q4, t, h, r);
#pragma unroll
      for (int i = 0; i < 4; i++) o[i] = r[i];
    }
  } else if (col < 2 * nv) {
    const int d = col - nv;
    a.p_qvel[w * nv + d] = a.qvel[e * nv + d] + h;
  } else {
    const int d = col - 2 * nv;
    a.p_qacc[w * nv + d] = a.qacc[e * nv + d] + h;
  }
}

template <typename REAL>
__global__ __launch_bounds__(MJH_IFD_DIFF_WG) void mjh_ifd_difference_kernel(IfdDiffArgs<REAL> a) {
  const int64_t g = a.first + (int64_t)blockIdx.x * MJH_IFD_DIFF_WG + threadIdx.x;
  if (g >= a.total) return;
  const int nv = a.nv, nsd = a.nsd, nrow = nv + nsd, nside = a.centered ? 2 : 1;
  const int64_t t = g / a.ncol;
  const int cl = (int)(g - t * a.ncol);
  const int64_t e = t / nrow;
  const int row = (int)(t - e * nrow), col = a.col0 + cl;
  const int64_t wp = (e * a.ncol + cl) * nside, wm = wp + nside - 1;  // the slots of the forward and of the backward nudge
  const bool sens = row >= nv;
  const int r = sens ? row - nv : row, n = sens ? nsd : nv;
  const REAL* y = sens ? a.s : a.f;
  const REAL* y0 = sens ? a.s0 : a.f0;
  const REAL h = a.eps;
  const REAL v = a.centered ? (y[wp * n + r] - y[wm * n + r]) / (2 * h) : (y[wp * n + r] - y0[e * n + r]) / h;
  const int blk = col / nv;  // 0: qpos, 1: qvel, 2: qacc
  REAL* D = sens ? (blk == 0 ? a.DsDq : (blk == 1 ? a.DsDv : a.DsDa)) : (blk == 0 ? a.DfDq : (blk == 1 ? a.DfDv : a.DfDa));
  D[(e * n + r) * nv + (col - blk * nv)] = v;
}
