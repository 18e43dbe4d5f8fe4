// mjh_ifd.h -- what a finite-difference Jacobian of inverse dynamics (mjh_ifd_perturb, mjh_ifd_difference; MuJoCo's mjd_inverseFD) adds to
// mjh_fd.h.  The passes themselves are plain mjh_inverse calls over the perturbed environments.
//
// Columns: c in [0, nv) nudges qpos along dof c (tangent space), [nv, 2 nv) qvel, [2 nv, 3 nv) qacc.  Nothing else is perturbed.  A call serves the
// columns [col0, col0 + ncol) of every environment, in the slot layout of mjh_fd.h.
//
// mjh_ifd_perturb_kernel: mjh_fd.h's fd_perturb_slot with INVERSE -- the same workgroup as mjh_fd_perturb_kernel's up to column 2 nv, where it
//   nudges qacc (x + h) instead of act / ctrl.  It takes FdPerturbArgs, with qacc / p_qacc set and na = nu = 0.
// mjh_ifd_difference_kernel: one lane per (environment, row, column of the chunk) by mjh_fd.h's fd_unit, column fastest, so that a wave's stores run
//   along a row of DfDq / DfDv / DfDa (DsDq / DsDv / DsDa) for as many columns as the chunk holds.  Rows [0, nv): qfrc_inverse, then, with the
//   sensor matrices, sensordata.  No row is a quaternion, so the entry is this file's own: (y+ - y0) / eps  or, centered,  (y+ - y-) / (2 eps), with
//   no fd_sub and no control rule.
// Both move far fewer bytes than the passes between them: a slot's input leaves, and nv + nsensordata outputs per slot.
#pragma once
#include "mjh_fd.h"

#define MJH_IFD_PERTURB_WG MJH_FD_PERTURB_WG
#define MJH_IFD_DIFF_WG 256

template <typename REAL>
struct IfdDiffArgs {
  FdCommon<REAL> c;                     // na = nu = 0, no ctrl; nsd: 0 when the sensor matrices are not asked for; units: B * (nv + nsd) * ncol entries
  const REAL *f0, *s0;                  // the nominal pass: qfrc_inverse [B, nv], sensordata [B, nsd]
  const REAL *f, *s;                    // the perturbed passes: [slots, nv], [slots, nsd]
  REAL *DfDq, *DfDv, *DfDa;             // [B, nv, nv]
  REAL *DsDq, *DsDv, *DsDa;             // [B, nsd, nv]
};

template <typename REAL>
__global__ __launch_bounds__(MJH_IFD_PERTURB_WG) void mjh_ifd_perturb_kernel(FdPerturbArgs<REAL> a) { fd_perturb_slot<REAL, true>(a); }

template <typename REAL>
__global__ __launch_bounds__(MJH_IFD_DIFF_WG) void mjh_ifd_difference_kernel(IfdDiffArgs<REAL> a) {
  const FdCommon<REAL>& c = a.c;
  const int64_t g = c.span.first + (int64_t)blockIdx.x * MJH_IFD_DIFF_WG + threadIdx.x;
  if (g >= c.span.total) return;
  const int nv = c.nv, nsd = c.nsd;
  int64_t e, wp, wm;
  int row, cl;
  fd_unit(c, g, nv + nsd, e, row, cl);
  fd_slots(c, e, cl, wp, wm);
  const int col = c.col0 + cl;
  const bool sens = row >= nv;
  const int r = sens ? row - nv : row, n = sens ? nsd : nv;
  const REAL* y = sens ? a.s : a.f;
  const REAL* y0 = sens ? a.s0 : a.f0;
  const REAL h = c.eps;
  const REAL v = c.centered ? (y[wp * n + r] - y[wm * n + r]) / (2 * h) : (y[wp * n + r] - y0[e * n + r]) / h;
  const int blk = col / nv;  // 0: qpos, 1: qvel, 2: qacc
  REAL* D = sens ? (blk == 0 ? a.DsDq : (blk == 1 ? a.DsDv : a.DsDa)) : (blk == 0 ? a.DfDq : (blk == 1 ? a.DfDv : a.DfDa));
  D[(e * n + r) * nv + (col - blk * nv)] = v;
}
