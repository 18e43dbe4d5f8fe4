// mjh_fd.h -- the kernels around the steps of a finite-difference transition Jacobian (mjh_fd_perturb, mjh_fd_difference; MuJoCo's
// mjd_transitionFD) and of its vector-Jacobian product (mjh_fd_vjp, mjh_fd_tangent).  The steps themselves are plain mjh_step calls over the
// perturbed environments.  What the family shares with the Jacobians of inverse dynamics (mjh_ifd.h) lives here too: FdCommon, the slot layout
// (fd_unit, fd_slots) and the whole of a perturb workgroup (fd_perturb_slot, which mjh_ifd_perturb_kernel instantiates with INVERSE).
//
// Columns: c in [0, nv) nudges qpos along dof c (tangent space), [nv, 2 nv) qvel, [2 nv, ns) act, ns = 2 nv + na, and [ns, ns + nu) ctrl.  A call
// serves the columns [col0, col0 + ncol) of every environment.  Column c of environment e owns nside (1, centered: 2) perturbed environments,
// "slots", at index  w = (e * ncol + (c - col0)) * nside + side  of the scratch batch: environment-major, so every leaf of the scratch batch is
// written and read in address order.  Which column a slot is, and which way it is nudged, is decoded from w here: there is no column list in memory.
//
// mjh_fd_perturb_kernel (fd_perturb_slot): one workgroup per slot.  It streams every listed input leaf of environment e into slot w (4-byte words, consecutive lanes on
//   consecutive addresses), then one lane nudges the slot's entry: x + h for qvel / act / ctrl and slide / hinge / free-translation dofs;
//   quat_integrate(q, e_k, h) (mjh_device.h, forward.py:231-252) for the rotational dofs of ball / free joints; h = +eps on side 0, -eps on side 1.
//   INVERSE changes what the columns from 2 nv on are: qacc (x + h) in place of act and ctrl.
// ctrl (fd_ctrl_sides): with actuator_ctrllimited, a nudge is taken only when ctrl and the nudged ctrl both lie inside actuator_ctrlrange; the
//   backward nudge only when centered or when the forward one was refused.  One-sided, the single slot carries the forward nudge, else the backward
//   one, else the caller's ctrl unchanged; centered, a refused side carries it unchanged.  The flags depend on each environment's own ctrl and are
//   formed again, from the same values by the same function, in the difference kernel.
// mjh_fd_difference_kernel: one lane per (environment, row, column of the chunk), column fastest, so that a wave's stores run along a row of A / B /
//   C / D for as many columns as the chunk holds.  Rows [0, nv): qpos differenced in tangent space -- subtraction, or quat_sub(q1, q0), the rotation
//   vector of q0^-1 q1 -- then qvel, act and, with C / D, sensordata.  Forward (y+ - y0) / eps, backward (y0 - y-) / eps, centered state columns
//   (y+ - y-) / (2 eps); a ctrl column with both sides taken is the mean of its forward and backward difference; with none, zero.
// mjh_fd_vjp_kernel: the same entries contracted with a cotangent instead of stored: one wavefront per (environment, column of the chunk), lane l
//   sums g[row] * v(row, column) over row = l, l + 64, ... in ascending order, one xor butterfly adds the 64 partial sums, lane 0 stores.  The order
//   of the additions depends on the number of rows alone: the result is the same bits from run to run and whatever the chunking.  fd_entry is the
//   expression both kernels share.
// mjh_fd_tangent_kernel: the two coordinate maps between a cotangent of qpos (nq) and one of the tangent space (nv); see there.
// The first two move far fewer bytes than the steps between them (a slot's inputs and four of its output leaves against the ~50 KB a humanoid step writes).
#pragma once
#include "mjh_device.h"

#define MJH_FD_PERTURB_WG 64
#define MJH_FD_DIFF_WG 256
#define MJH_FD_VJP_WG 256      // four wavefronts, one (environment, column) each
#define MJH_FD_TANGENT_WG 256
#define MJH_FD_MAX_LEAVES 24

struct FdLeaf {
  unsigned* dst;        // [slots, words]
  const unsigned* src;  // [B, words]
  int words;            // 4-byte words per environment
  int pad_;
};

// the units (slots / output elements / dofs) of a call, and where this launch starts among them (the host's launch_fd sets both)
struct FdSpan {
  int64_t first, total;
};

// what the kernels of the family read of the model and of the call; mjh_ifd.h: no act or ctrl columns, so na = nu = 0 and the ctrl fields are null
template <typename REAL>
struct FdCommon {
  const int *dof_jntid, *jnt_type, *jnt_qposadr, *jnt_dofadr, *act_ctrllimited;
  const REAL* act_ctrlrange;
  const REAL* ctrl;     // the caller's [B, nu]
  REAL eps;
  int nq, nv, na, nu, nsd;
  int centered, col0, ncol;
  FdSpan span;
};

// INVERSE reads qacc / p_qacc and leaves act / p_act / p_ctrl null; the transition kernel the other way round
template <typename REAL>
struct FdPerturbArgs {
  FdCommon<REAL> c;
  const REAL *qpos, *qvel, *act, *qacc;            // the caller's
  REAL *p_qpos, *p_qvel, *p_act, *p_ctrl, *p_qacc; // the scratch batch's
  int nleaf, pad_;
  FdLeaf leaf[MJH_FD_MAX_LEAVES];
};

template <typename REAL>
struct FdState {
  const REAL *qpos, *qvel, *act, *sens;
};

template <typename REAL>
struct FdDiffArgs {
  FdCommon<REAL> c;
  FdState<REAL> y0;  // the nominal step's result [B, ...]
  FdState<REAL> y;   // the perturbed steps' results [slots, ...]
  REAL *A, *Bm, *C, *D;
};

template <typename REAL>
struct FdVjpArgs {
  FdCommon<REAL> c;
  FdState<REAL> y0, y;        // as in FdDiffArgs
  const REAL *g_state;        // [B, ns]  cotangent of the next state, tangent-space order
  const REAL *g_sens;         // [B, nsd] cotangent of sensordata, or null
  REAL *gx, *gu;              // [B, ns], [B, nu]
};

template <typename REAL>
struct FdTangentArgs {
  const int *dof_jntid, *jnt_type, *jnt_qposadr, *jnt_dofadr;
  const REAL *qpos;           // [B, nq]
  const REAL *g_in;           // pull: [B, nq], push: [B, nv]
  REAL *g_out;                // pull: [B, nv], push: [B, nq]
  int nq, nv, mode, pad_;
  FdSpan span;                // units: (environment, dof)
};

// bit 0: the forward nudge is taken, bit 1: the backward one
template <typename REAL>
__device__ __forceinline__ int fd_ctrl_sides(const FdCommon<REAL>& c, int64_t e, int i) {
  const bool lim = c.act_ctrllimited[i] != 0;
  const REAL u = c.ctrl[e * c.nu + i], lo = c.act_ctrlrange[2 * i], hi = c.act_ctrlrange[2 * i + 1];
  const REAL up = u + c.eps, um = u - c.eps;
  const bool in0 = u >= lo && u <= hi;
  const bool fwd = !lim || (in0 && up >= lo && up <= hi);
  const bool bwd = (c.centered || !fwd) && (!lim || (in0 && um >= lo && um <= hi));
  return (fwd ? 1 : 0) | (bwd ? 2 : 0);
}

// where dof d lives in qpos: its joint's type, the address of the entry (or of the quaternion) and, for a rotational dof, its axis (else -1)
__device__ __forceinline__ void fd_dof(const int* dof_jntid, const int* jnt_type, const int* jnt_qposadr, const int* jnt_dofadr, int d, int& adr, int& axis) {
  const int j = dof_jntid[d], t = jnt_type[j], qa = jnt_qposadr[j], k = d - jnt_dofadr[j];
  if (t == JNT_FREE && k >= 3) { adr = qa + 3; axis = k - 3; }
  else if (t == JNT_BALL) { adr = qa; axis = k; }
  else { adr = qa + k; axis = -1; }
}

// The slots of column cl of the chunk in environment e: wp carries the forward nudge, wm the backward one (the same slot when not centered)
template <typename REAL>
__device__ __forceinline__ void fd_slots(const FdCommon<REAL>& c, int64_t e, int cl, int64_t& wp, int64_t& wm) {
  const int nside = c.centered ? 2 : 1;
  wp = (e * c.ncol + cl) * nside;
  wm = wp + nside - 1;
}

// Unit g of a difference call, column fastest: environment e, row of nrow, column cl of the chunk
template <typename REAL>
__device__ __forceinline__ void fd_unit(const FdCommon<REAL>& c, int64_t g, int nrow, int64_t& e, int& row, int& cl) {
  const int64_t t = g / c.ncol;
  cl = (int)(g - t * c.ncol);
  e = t / nrow;
  row = (int)(t - e * nrow);
}

// One workgroup of a perturb kernel: slot w of the scratch batch, copied from its environment and nudged in its column
template <typename REAL, bool INVERSE>
__device__ __forceinline__ void fd_perturb_slot(const FdPerturbArgs<REAL>& a) {
  const FdCommon<REAL>& c = a.c;
  const int64_t w = c.span.first + blockIdx.x;
  if (w >= c.span.total) return;
  const int nside = c.centered ? 2 : 1, nslot = c.ncol * nside;
  const int64_t e = w / nslot;
  const int sl = (int)(w - e * nslot);
  for (int l = 0; l < a.nleaf; l++) {
    const FdLeaf L = a.leaf[l];
    unsigned* dst = L.dst + w * L.words;
    const unsigned* src = L.src + e * L.words;
    for (int i = threadIdx.x; i < L.words; i += MJH_FD_PERTURB_WG) dst[i] = src[i];
  }
  __syncthreads();  // the nudged entry is stored over its copy
  if (threadIdx.x != 0) return;
  const int col = c.col0 + sl / nside, side = sl - (sl / nside) * nside;
  const int nv = c.nv, ns = 2 * nv + c.na;
  REAL h = side ? -c.eps : c.eps;
  if (col < nv) {
    int adr, axis;
    fd_dof(c.dof_jntid, c.jnt_type, c.jnt_qposadr, c.jnt_dofadr, col, adr, axis);
    const REAL* q = a.qpos + e * c.nq + adr;
    REAL* o = a.p_qpos + w * c.nq + adr;
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
  } else if constexpr (INVERSE) {
    const int d = col - 2 * nv;
    a.p_qacc[w * nv + d] = a.qacc[e * nv + d] + h;
  } else if (col < ns) {
    const int i = col - 2 * nv;
    a.p_act[w * c.na + i] = a.act[e * c.na + i] + h;
  } else {
    const int i = col - ns, sides = fd_ctrl_sides(c, e, i);
    bool take;
    if (c.centered) take = side ? (sides & 2) != 0 : (sides & 1) != 0;
    else { take = sides != 0; if (!(sides & 1)) h = -c.eps; }
    if (take) a.p_ctrl[w * c.nu + i] = c.ctrl[e * c.nu + i] + h;
  }
}

template <typename REAL>
__global__ __launch_bounds__(MJH_FD_PERTURB_WG) void mjh_fd_perturb_kernel(FdPerturbArgs<REAL> a) { fd_perturb_slot<REAL, false>(a); }

// element `row` of  y1 - y0  in tangent space
template <typename REAL>
__device__ __forceinline__ REAL fd_sub(const FdCommon<REAL>& c, const FdState<REAL>& s1, int64_t e1, const FdState<REAL>& s0, int64_t e0, int row) {
  const int nv = c.nv, ns = 2 * nv + c.na;
  if (row < nv) {
    int adr, axis;
    fd_dof(c.dof_jntid, c.jnt_type, c.jnt_qposadr, c.jnt_dofadr, row, adr, axis);
    const REAL *q1 = s1.qpos + e1 * c.nq + adr, *q0 = s0.qpos + e0 * c.nq + adr;
    if (axis < 0) return q1[0] - q0[0];
    const REAL u[4] = {q1[0], q1[1], q1[2], q1[3]}, v[4] = {q0[0], q0[1], q0[2], q0[3]};
    REAL r[3];
    quat_sub(u, v, r);
    return axis == 0 ? r[0] : (axis == 1 ? r[1] : r[2]);
  }
  if (row < 2 * nv) return s1.qvel[e1 * nv + (row - nv)] - s0.qvel[e0 * nv + (row - nv)];
  if (row < ns) return s1.act[e1 * c.na + (row - 2 * nv)] - s0.act[e0 * c.na + (row - 2 * nv)];
  return s1.sens[e1 * c.nsd + (row - ns)] - s0.sens[e0 * c.nsd + (row - ns)];
}

// entry (row, col0 + cl) of environment e's A / B / C / D: `sides` is fd_ctrl_sides of a ctrl column, else 3 when centered and 1 when not
template <typename REAL>
__device__ __forceinline__ REAL fd_entry(const FdCommon<REAL>& c, const FdState<REAL>& y0, const FdState<REAL>& y, int64_t e, int cl, int row, bool is_ctrl, int sides) {
  int64_t wp, wm;
  fd_slots(c, e, cl, wp, wm);
  const REAL h = c.eps;
  REAL v = 0;
  if (sides == 1) v = fd_sub(c, y, wp, y0, e, row) / h;
  else if (sides == 2) v = fd_sub(c, y0, e, y, wm, row) / h;
  else if (sides == 3 && !is_ctrl) v = fd_sub(c, y, wp, y, wm, row) / (2 * h);
  else if (sides == 3) v = (fd_sub(c, y, wp, y0, e, row) / h + fd_sub(c, y0, e, y, wm, row) / h) * (REAL)0.5;
  return v;
}

template <typename REAL>
__global__ __launch_bounds__(MJH_FD_DIFF_WG) void mjh_fd_difference_kernel(FdDiffArgs<REAL> a) {
  const FdCommon<REAL>& c = a.c;
  const int64_t g = c.span.first + (int64_t)blockIdx.x * MJH_FD_DIFF_WG + threadIdx.x;
  if (g >= c.span.total) return;
  const int nv = c.nv, ns = 2 * nv + c.na, nrow = ns + (a.C ? c.nsd : 0);
  int64_t e;
  int row, cl;
  fd_unit(c, g, nrow, e, row, cl);
  const int col = c.col0 + cl;
  const bool is_ctrl = col >= ns;
  const int sides = is_ctrl ? fd_ctrl_sides(c, e, col - ns) : (c.centered ? 3 : 1);
  const REAL v = fd_entry(c, a.y0, a.y, e, cl, row, is_ctrl, sides);
  if (row < ns) {
    if (!is_ctrl) a.A[(e * ns + row) * ns + col] = v;
    else a.Bm[(e * ns + row) * c.nu + (col - ns)] = v;
  } else {
    if (!is_ctrl) a.C[(e * c.nsd + (row - ns)) * ns + col] = v;
    else a.D[(e * c.nsd + (row - ns)) * c.nu + (col - ns)] = v;
  }
}

template <typename REAL>
__global__ __launch_bounds__(MJH_FD_VJP_WG) void mjh_fd_vjp_kernel(FdVjpArgs<REAL> a) {
  const FdCommon<REAL>& c = a.c;
  const int lane = threadIdx.x & (MJH_WAVE - 1);
  const int64_t u = c.span.first + (int64_t)blockIdx.x * (MJH_FD_VJP_WG / MJH_WAVE) + threadIdx.x / MJH_WAVE;  // the same for all lanes of a wavefront
  if (u >= c.span.total) return;
  const int nv = c.nv, ns = 2 * nv + c.na, nrow = ns + (a.g_sens ? c.nsd : 0);
  const int64_t e = u / c.ncol;
  const int cl = (int)(u - e * c.ncol), col = c.col0 + cl;
  const bool is_ctrl = col >= ns;
  const int sides = is_ctrl ? fd_ctrl_sides(c, e, col - ns) : (c.centered ? 3 : 1);
  REAL acc = 0;
  for (int row = lane; row < nrow; row += MJH_WAVE) {
    const REAL g = row < ns ? a.g_state[e * ns + row] : a.g_sens[e * c.nsd + (row - ns)];
    acc = acc + g * fd_entry(c, a.y0, a.y, e, cl, row, is_ctrl, sides);
  }
#pragma unroll
  for (int m = MJH_WAVE / 2; m >= 1; m >>= 1) acc = acc + __shfl_xor(acc, m, MJH_WAVE);  // (every lane ends with the same sum: a + b == b + a)
  if (lane != 0) return;
  if (!is_ctrl) a.gx[e * ns + col] = acc;
  else a.gu[e * c.nu + (col - ns)] = acc;
}

// b = q (x) (0, e_k): the direction qpos moves in when the quaternion q turns about its local axis k (q (x) exp(d / 2) = q + b d / 2 + ...)
template <typename REAL>
__device__ __forceinline__ void fd_quat_dir(const REAL* q, int k, REAL* b) {
  if (k == 0) { b[0] = -q[1]; b[1] = q[0]; b[2] = q[3]; b[3] = -q[2]; }
  else if (k == 1) { b[0] = -q[2]; b[1] = -q[3]; b[2] = q[0]; b[3] = q[1]; }
  else { b[0] = -q[3]; b[1] = q[2]; b[2] = -q[1]; b[3] = q[0]; }
}

// One lane per (environment, dof).  mode 0, pull: the cotangent g_in of qpos [B, nq] to the tangent space at qpos, g_out [B, nv]: the entry itself
// for slide / hinge / free-translation dofs, <g_in[quaternion], b_k> / 2 for the rotational dof k of a ball / free joint (the adjoint of
// d -> q (x) exp(d / 2)).  mode 1, push: a tangent cotangent g_in [B, nv] to qpos coordinates, g_out [B, nq]: the entry itself, or for a quaternion
// 2 sum_k g_in[k] b_k / |q|^2 (zero for an all-zero quaternion) -- the cotangent with no component along q (a step's dependence on a quaternion's norm is not differentiated) whose
// pull is g_in.  The lane of a quaternion's first rotational dof writes all four entries; every entry of qpos belongs to exactly one joint.
template <typename REAL>
__global__ __launch_bounds__(MJH_FD_TANGENT_WG) void mjh_fd_tangent_kernel(FdTangentArgs<REAL> a) {
  const int64_t g = a.span.first + (int64_t)blockIdx.x * MJH_FD_TANGENT_WG + threadIdx.x;
  if (g >= a.span.total) return;
  const int64_t e = g / a.nv;
  const int d = (int)(g - e * a.nv);
  int adr, axis;
  fd_dof(a.dof_jntid, a.jnt_type, a.jnt_qposadr, a.jnt_dofadr, d, adr, axis);
  const REAL* q = a.qpos + e * a.nq + adr;
  if (a.mode == 0) {
    const REAL* gq = a.g_in + e * a.nq + adr;
    if (axis < 0) { a.g_out[e * a.nv + d] = gq[0]; return; }
    const REAL q4[4] = {q[0], q[1], q[2], q[3]};
    REAL b[4];
    fd_quat_dir(q4, axis, b);
    a.g_out[e * a.nv + d] = (REAL)0.5 * (((gq[0] * b[0] + gq[1] * b[1]) + gq[2] * b[2]) + gq[3] * b[3]);
  } else {
    const REAL* gt = a.g_in + e * a.nv + d;
    REAL* o = a.g_out + e * a.nq + adr;
    if (axis < 0) { o[0] = gt[0]; return; }
    if (axis != 0) return;
    const REAL q4[4] = {q[0], q[1], q[2], q[3]};
    REAL n2 = ((q4[0] * q4[0] + q4[1] * q4[1]) + q4[2] * q4[2]) + q4[3] * q4[3];
    n2 = n2 + (REAL)(n2 == 0);  // an all-zero quaternion stays zero under normalize_n and quat_integrate: no rotation changes the step, the cotangent is zero
    REAL b0[4], b1[4], b2[4];
    fd_quat_dir(q4, 0, b0);
    fd_quat_dir(q4, 1, b1);
    fd_quat_dir(q4, 2, b2);
#pragma unroll
    for (int i = 0; i < 4; i++) o[i] = (REAL)2 * ((gt[0] * b0[i] + gt[1] * b1[i]) + gt[2] * b2[i]) / n2;
  }
}
