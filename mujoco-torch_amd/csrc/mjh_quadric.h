// mjh_quadric.h -- narrow phase of the plane-ellipsoid and plane-cylinder pairs: ONE LANE PER (environment, pair).
//
// Restates reference mujoco_torch/_src/collision_primitive.py, hard-selection branch (smooth_collisions off): plane_ellipsoid :77-85 (one contact) and
// plane_cylinder :88-169 (three contacts), operation by operation: math.sign is +1 at 0, math.norm is zero-safe, normalize divides by n + 1e-6 (n == 0),
// the flat disc (len_ < 1e-12) takes mat[:, 0] * radius, the `par` test is made on prjaxis AFTER its scaling by the half-length, and the sideways
// vector is scaled by torch.sqrt(torch.full((), 3.0)) * 0.5 -- a float32 0-d tensor whatever the model's dtype, so a float64 model multiplies by
// the float32-rounded value, widened.
//
// A pair is a few dozen flops between 24 reals in and 13 per contact out: a wave per pair (as the convex narrow phase has it) would leave 63 lanes
// idle, so the (environment, pair) items are spread over the lanes, environment-major -- the lanes of a wave read the geom frames of a handful of
// neighbouring environments and write neighbouring contact slots.  No LDS, no cross-lane traffic, every load of an item issued up front.
//
// The hand-over is the convex narrow phase's (mjh_convex.h): the kernel runs behind the kinematics, once per RK4 stage, reads geom_xpos / geom_xmat of
// the pass and writes dist / pos / frame into the pair's contact slots (pair_dst) -- or, with max_contact_points, into the candidate arrays of the
// workspace; the constraint stage skips every pair function from MJH_FN_PLANE_CONVEX up and loads what was written here.
// The host launches the kernel with DevModel::cvx_pairs / ncvxpair narrowed to ITS pairs (mjhip.hip: launch_quadric).
#pragma once
#include "mjh_kernels.h"

#define M (kargs<REAL>().M)
#define out (kargs<REAL>().cur)
#define KA (kargs<REAL>())

template <typename REAL>
struct QuadricPair {
  int64_t e;
  int p;
  REAL frame[9];  // make_frame(plane normal): shared by the contacts of the pair

  __device__ __forceinline__ QuadricPair(int64_t env, int pair) : e(env), p(pair) {}

  // contact q of the pair to its slot (CvxPair::emit, with the frame made once)
  __device__ __forceinline__ void emit(int q, REAL dist, const REAL* pos) const {
    const int c = M.pair_dst[p * MJH_MAX_PAIR_CONTACTS + q];
    const bool cand = M.topk != 0;  // max_contact_points: `c` is a CANDIDATE index, the arrays are the workspace's (the constraint phase selects)
    const int64_t nc = cand ? M.ncand : M.ncon, B = KA.B;
    if (c < 0 || c >= nc) return;
    REAL* const gd = cand ? KA.cand : out.contact_dist;
    REAL* const gp = cand ? KA.cand + B * nc : out.contact_pos;
    REAL* const gf = cand ? KA.cand + 4 * B * nc : out.contact_frame;
    gd[e * nc + c] = dist;
#pragma unroll
    for (int i = 0; i < 3; i++) gp[(e * nc + c) * 3 + i] = pos[i];
#pragma unroll
    for (int i = 0; i < 9; i++) gf[(e * nc + c) * 9 + i] = frame[i];
  }

  // ---- plane_ellipsoid :77-85 -------------------------------------------------------------------------------------------
  __device__ __forceinline__ void plane_ellipsoid(const REAL* ppos, const REAL* n, const REAL* epos, const REAL* emat, const REAL* size) const {
    REAL s[3];
#pragma unroll
    for (int i = 0; i < 3; i++) s[i] = (emat[i] * n[0] + emat[3 + i] * n[1] + emat[6 + i] * n[2]) * size[i];  // (mat.T * n).sum(-1) * size
    normalize_n<REAL, 3>(s);
#pragma unroll
    for (int i = 0; i < 3; i++) s[i] = -s[i] * size[i];  // sphere_support * size
    REAL pos[3], rel[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
      pos[i] = epos[i] + (emat[3 * i] * s[0] + emat[3 * i + 1] * s[1] + emat[3 * i + 2] * s[2]);
      rel[i] = pos[i] - ppos[i];
    }
    const REAL dist = dot3(n, rel);
#pragma unroll
    for (int i = 0; i < 3; i++) pos[i] = pos[i] - n[i] * dist * (REAL)0.5;
    emit(0, dist, pos);
  }

  // ---- plane_cylinder :88-169 -------------------------------------------------------------------------------------------
  __device__ __forceinline__ void plane_cylinder(const REAL* ppos, const REAL* n, const REAL* cpos, const REAL* cmat, const REAL* size) const {
    const REAL radius = size[0], half = size[1];
    REAL axis[3] = {cmat[2], cmat[5], cmat[8]};
    // make sure axis points towards plane (-math.sign: +1 for prjaxis < 0, -1 otherwise, zero included)
    REAL prjaxis = dot3(n, axis);
    const REAL sign = prjaxis < 0 ? (REAL)1 : (REAL)-1;
#pragma unroll
    for (int i = 0; i < 3; i++) axis[i] = axis[i] * sign;
    prjaxis = prjaxis * sign;
    // normal distance to the cylinder's centre
    const REAL rel[3] = {cpos[0] - ppos[0], cpos[1] - ppos[1], cpos[2] - ppos[2]};
    const REAL dist0 = dot3(rel, n);
    // remove the component of -normal along the axis
    REAL vec[3];
#pragma unroll
    for (int i = 0; i < 3; i++) vec[i] = axis[i] * prjaxis - n[i];
    const REAL len = norm_n<REAL, 3>(vec);
    if (len < (REAL)1e-12) {  // disc flat on the plane
#pragma unroll
      for (int i = 0; i < 3; i++) vec[i] = cmat[3 * i] * radius;
    } else {  // safe_div (math.py:79-81): len != 0 here
#pragma unroll
      for (int i = 0; i < 3; i++) vec[i] = vec[i] / len * radius;
    }
    const REAL prjvec = dot3(vec, n);
    // scale axis by the half-length
#pragma unroll
    for (int i = 0; i < 3; i++) axis[i] = axis[i] * half;
    prjaxis = prjaxis * half;
    // sideways vector
    const REAL prjvec1 = -prjvec * (REAL)0.5;
    REAL vec1[3];
    cross3(vec, axis, vec1);
    normalize_n<REAL, 3>(vec1);
    const REAL k = (REAL)(1.7320508075688772f * 0.5f);  // torch.sqrt(torch.full((), 3.0)) * 0.5: float32 in every model dtype
#pragma unroll
    for (int i = 0; i < 3; i++) vec1[i] = vec1[i] * radius * k;
    // disc parallel to the plane ...
    const REAL d1 = dist0 + prjaxis + prjvec, d2 = dist0 + prjaxis + prjvec1;
    // ... or the cylinder's side (|prjaxis| after the scaling)
    const REAL d3 = dist0 - prjaxis + prjvec;
    const bool par = r_abs(prjaxis) < (REAL)1e-3;
    REAL pos[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
      const REAL base = cpos[i] + axis[i], hv = vec[i] * (REAL)-0.5;
      pos[0][i] = base + (vec[i] - n[i] * d1 * (REAL)0.5);
      pos[1][i] = par ? (cpos[i] + vec[i] - axis[i] - n[i] * d3 * (REAL)0.5) : (base + (vec1[i] + hv - n[i] * d2 * (REAL)0.5));
      pos[2][i] = base + (-vec1[i] + hv - n[i] * d2 * (REAL)0.5);
    }
    emit(0, d1, pos[0]);
    emit(1, par ? d3 : d2, pos[1]);
    emit(2, d2, pos[2]);
  }

  __device__ __forceinline__ void run() {
    const int g1 = M.pair_geom1[p], g2 = M.pair_geom2[p], fn = M.pair_fn[p];
    const int64_t ng = M.ngeom;
    const REAL *gp = out.geom_xpos + e * ng * 3, *gm = out.geom_xmat + e * ng * 9;
    REAL p1[3], n[3], p2[3], m2[9];
#pragma unroll
    for (int i = 0; i < 3; i++) { p1[i] = gp[3 * g1 + i]; p2[i] = gp[3 * g2 + i]; n[i] = gm[9 * g1 + 3 * i + 2]; }
#pragma unroll
    for (int i = 0; i < 9; i++) m2[i] = gm[9 * g2 + i];
    const REAL size[3] = {M.geom_size[3 * g2], M.geom_size[3 * g2 + 1], M.geom_size[3 * g2 + 2]};
    make_frame(n, frame);
    if (fn == MJH_FN_PLANE_ELLIPSOID) plane_ellipsoid(p1, n, p2, m2, size);
    else if (fn == MJH_FN_PLANE_CYLINDER) plane_cylinder(p1, n, p2, m2, size);
  }
};

// grid: ceil(items / 64) one-wave workgroups over the items [env_begin, env_begin + env_count) of B * ncvxpair (environment-major); no grid-stride loop
template <typename REAL>
__global__ __launch_bounds__(MJH_WAVE) void mjh_quadric_kernel(KArgs<REAL> args) {
  const int npc = M.ncvxpair;
  const int64_t item = KA.env_begin + (int64_t)blockIdx.x * MJH_WAVE + lane_id();
  if (item >= KA.env_begin + KA.env_count) return;
  const int64_t env = item / npc;
  const int pair = M.cvx_pairs[(int)(item - env * npc)];
  QuadricPair<REAL>(env, pair).run();
}

#undef M
#undef out
#undef KA
