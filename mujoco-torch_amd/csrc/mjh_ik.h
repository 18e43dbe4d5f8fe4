// mjh_ik.h -- one damped-least-squares iteration of site-pose inverse kinematics (the scheme of dm_control's qpos_from_site_pose with constant regularisation),
// on the leaves of a kinematics pass: ONE WAVEFRONT PER ENVIRONMENT, MODE (1: position, 2: orientation, 3: both) a template argument so that the N = 3 or 6 rows
// are compile-time loops over registers.  No LDS, no scratch; an environment's result depends on nothing but its own rows.
//
// Per environment that is not done:
//  1. e_pos = target_pos - site_xpos;  e_rot = the rotation vector (axis times angle, angle in [0, pi], world frame like jacr) of E = R_target site_xmat^T,
//     R_target = quat_to_mat(target_quat): E goes to a quaternion by the branch of Shepperd's method with the largest pivot, its sign chosen so that
//     w >= 0, and e_rot = axis * 2 atan2(|xyz|, w).  e stacks the parts asked for;  err_norm = |e_pos| + rot_weight |e_rot|, stored.
//  2. err_norm < tol: done = 1 and nothing else is touched.  Otherwise, on the last evaluation, nothing else is touched either.
//  3. J[:, d] = (jacp | jacr)(site)[d] * sel[d]: the arithmetic of mjh_support.h's JAC on cdof and subtree_com[body_rootid[site body]], columns of dofs outside
//     the selection zeroed.  G = J J^T + damping I: every entry a lane-partial sum over the lane's dofs in ascending order, then wave_sum (a fixed order).
//     G = L L^T (Cholesky, every pivot clamped at 1e-12 as math.small_cholesky does), L L^T y = e, redundantly in every lane.  delta_d = J[:, d] . y;  |delta| > max_update_norm: delta *= max_update_norm / |delta|.
//  4. one lane per joint with a selected dof: qpos <- qpos_integrate_joint(qpos, delta, 1) (mjh_qpos.h), in place; the lane forms its joint's (<= 6) entries of
//     delta itself, by the expression of step 3.  A joint without a selected dof is not written.  steps += 1.
#pragma once
#include "mjh_device.h"
#include "mjh_qpos.h"

template <typename REAL>
struct IkSiteArgs {
  const REAL *cdof, *subtree_com, *site_xpos, *site_xmat;  // [B, nv, 6], [B, nbody, 3], [B, nsite, 3], [B, nsite, 9]: the pass at the current qpos
  const REAL *target_pos, *target_quat;                    // [B or 1, 3] / [B or 1, 4], NULL: absent (then MODE lacks that bit)
  const int* sel;                                          // [nv]: 1 = the dof takes part
  REAL* qpos;                                              // [B, nq], in place
  REAL* err_norm;                                          // [B]
  int* steps;                                              // [B]
  unsigned char* done;                                     // [B]
  const unsigned long long* body_dofmask;
  const int *body_rootid, *jnt_type, *jnt_qposadr, *jnt_dofadr;
  int64_t pos_stride, quat_stride;                         // elements between the targets of consecutive environments (0: shared)
  int64_t env_begin;
  int nv, nq, njnt, nbody, nsite, mask_words, site, body, last;
  REAL tol, damping, max_update_norm, rot_weight;
};

// rotation vector of the rotation matrix E (row-major), angle in [0, pi]
template <typename REAL>
__device__ __forceinline__ void ik_rotvec(const REAL* E, REAL* o) {
  const REAL tr = (E[0] + E[4]) + E[8];
  REAL q[4];
  if (tr >= E[0] && tr >= E[4] && tr >= E[8]) {
    const REAL s = 2 * r_sqrt<REAL>(1 + tr);  // 4 w
    q[0] = s / 4; q[1] = (E[7] - E[5]) / s; q[2] = (E[2] - E[6]) / s; q[3] = (E[3] - E[1]) / s;
  } else if (E[0] >= E[4] && E[0] >= E[8]) {
    const REAL s = 2 * r_sqrt<REAL>(((1 + E[0]) - E[4]) - E[8]);  // 4 x
    q[0] = (E[7] - E[5]) / s; q[1] = s / 4; q[2] = (E[1] + E[3]) / s; q[3] = (E[2] + E[6]) / s;
  } else if (E[4] >= E[8]) {
    const REAL s = 2 * r_sqrt<REAL>(((1 + E[4]) - E[0]) - E[8]);  // 4 y
    q[0] = (E[2] - E[6]) / s; q[1] = (E[1] + E[3]) / s; q[2] = s / 4; q[3] = (E[5] + E[7]) / s;
  } else {
    const REAL s = 2 * r_sqrt<REAL>(((1 + E[8]) - E[0]) - E[4]);  // 4 z
    q[0] = (E[3] - E[1]) / s; q[1] = (E[2] + E[6]) / s; q[2] = (E[5] + E[7]) / s; q[3] = s / 4;
  }
  const REAL sg = q[0] < 0 ? (REAL)-1 : (REAL)1;
  REAL axis[3] = {sg * q[1], sg * q[2], sg * q[3]};
  const REAL sn = normalize_n<REAL, 3>(axis);
  const REAL ang = 2 * r_atan2<REAL>(sn, sg * q[0]);
#pragma unroll
  for (int i = 0; i < 3; i++) o[i] = axis[i] * ang;
}

// column `dof` of J: the rows MODE asks for of (jacp | jacr) at the site, zero for a dof outside the selection (mjh_support.h: sup_jac_dof)
template <typename REAL, int MODE>
__device__ __forceinline__ void ik_column(const IkSiteArgs<REAL>& a, int64_t e, const REAL* off, int dof, REAL* col) {
  const REAL on = (REAL)((a.body_dofmask[(int64_t)a.body * a.mask_words + (dof >> 6)] >> (dof & 63)) & 1ull);
  const REAL use = (REAL)(a.sel[dof] != 0);
  const REAL* cd = a.cdof + (e * a.nv + dof) * 6;
  int r = 0;
  if (MODE & 1) {
    REAL c[3];
    cross3(cd, off, c);
#pragma unroll
    for (int i = 0; i < 3; i++) col[r++] = ((cd[3 + i] + c[i]) * on) * use;
  }
  if (MODE & 2) {
#pragma unroll
    for (int i = 0; i < 3; i++) col[r++] = (cd[i] * on) * use;
  }
}

// grid: one one-wave workgroup per environment of the launch
template <typename REAL, int MODE>
__global__ __launch_bounds__(MJH_WAVE) void mjh_ik_site_kernel(IkSiteArgs<REAL> a) {
  constexpr int N = MODE == 3 ? 6 : 3;
  const int64_t e = a.env_begin + blockIdx.x;
  const int l = lane_id();
  if (a.done[e]) return;  // (wave-uniform)

  // 1. the error
  const REAL* sp = a.site_xpos + (e * a.nsite + a.site) * 3;
  REAL err[N], en = 0;
  if (MODE & 1) {
    const REAL* tp = a.target_pos + e * a.pos_stride;
#pragma unroll
    for (int i = 0; i < 3; i++) err[i] = tp[i] - sp[i];
    en = norm_n<REAL, 3>(err);
  }
  if (MODE & 2) {
    const REAL* tq = a.target_quat + e * a.quat_stride;
    const REAL* S = a.site_xmat + (e * a.nsite + a.site) * 9;
    const REAL q[4] = {tq[0], tq[1], tq[2], tq[3]};
    REAL T[9], E[9];
    quat_to_mat(q, T);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) E[3 * i + j] = (T[3 * i] * S[3 * j] + T[3 * i + 1] * S[3 * j + 1]) + T[3 * i + 2] * S[3 * j + 2];
    REAL* er = err + (N - 3);
    ik_rotvec(E, er);
    en = en + a.rot_weight * norm_n<REAL, 3>(er);
  }
  if (l == 0) a.err_norm[e] = en;
  if (en < a.tol) {
    if (l == 0) a.done[e] = 1;
    return;
  }
  if (a.last) return;

  // 3. G = J J^T + damping I
  const REAL* rc = a.subtree_com + (e * a.nbody + a.body_rootid[a.body]) * 3;
  const REAL off[3] = {sp[0] - rc[0], sp[1] - rc[1], sp[2] - rc[2]};
  REAL G[N * (N + 1) / 2];
#pragma unroll
  for (int i = 0; i < N * (N + 1) / 2; i++) G[i] = 0;
  for (int d = l; d < a.nv; d += MJH_WAVE) {
    REAL col[N];
    ik_column<REAL, MODE>(a, e, off, d, col);
#pragma unroll
    for (int i = 0, k = 0; i < N; i++)
#pragma unroll
      for (int j = 0; j <= i; j++, k++) G[k] = G[k] + col[i] * col[j];
  }
#pragma unroll
  for (int i = 0, k = 0; i < N; i++)
#pragma unroll
    for (int j = 0; j <= i; j++, k++) G[k] = wave_sum(G[k]) + (i == j ? a.damping : (REAL)0);
  // Cholesky in place (packed lower rows), then the two substitutions
  REAL y[N];
#pragma unroll
  for (int i = 0; i < N; i++) {
#pragma unroll
    for (int j = 0; j <= i; j++) {
      REAL s = G[i * (i + 1) / 2 + j];
#pragma unroll
      for (int k = 0; k < j; k++) s = s - G[i * (i + 1) / 2 + k] * G[j * (j + 1) / 2 + k];
      if (i == j) s = s > (REAL)1e-12 ? s : (REAL)1e-12;  // (a pivot that rounding took to zero or below -- a rank-deficient selection with a damping near the rounding of G -- gives a large finite step, capped below, never a NaN)
      G[i * (i + 1) / 2 + j] = i == j ? r_sqrt<REAL>(s) : s / G[j * (j + 1) / 2 + j];
    }
  }
#pragma unroll
  for (int i = 0; i < N; i++) {
    REAL s = err[i];
#pragma unroll
    for (int k = 0; k < i; k++) s = s - G[i * (i + 1) / 2 + k] * y[k];
    y[i] = s / G[i * (i + 1) / 2 + i];
  }
#pragma unroll
  for (int i = N - 1; i >= 0; i--) {
    REAL s = y[i];
#pragma unroll
    for (int k = i + 1; k < N; k++) s = s - G[k * (k + 1) / 2 + i] * y[k];
    y[i] = s / G[i * (i + 1) / 2 + i];
  }
  // |delta|
  REAL n2 = 0;
  for (int d = l; d < a.nv; d += MJH_WAVE) {
    REAL col[N], dd = 0;
    ik_column<REAL, MODE>(a, e, off, d, col);
#pragma unroll
    for (int i = 0; i < N; i++) dd = dd + col[i] * y[i];
    n2 = n2 + dd * dd;
  }
  const REAL dn = r_sqrt<REAL>(wave_sum(n2));
  const REAL scale = dn > a.max_update_norm ? a.max_update_norm / dn : (REAL)1;

  // 4. the update, one lane per joint
  for (int j = l; j < a.njnt; j += MJH_WAVE) {
    const int t = a.jnt_type[j], qa = a.jnt_qposadr[j], da = a.jnt_dofadr[j];
    const int nd = t == JNT_FREE ? 6 : (t == JNT_BALL ? 3 : 1), nqj = t == JNT_FREE ? 7 : (t == JNT_BALL ? 4 : 1);
    bool any = false;
    for (int k = 0; k < nd; k++) any = any || a.sel[da + k] != 0;
    if (!any) continue;
    REAL v[6] = {0, 0, 0, 0, 0, 0}, q[7] = {0, 0, 0, 0, 0, 0, 0}, o[7];
#pragma unroll
    for (int k = 0; k < 6; k++) {
      if (k < nd) {
        REAL col[N], dd = 0;
        ik_column<REAL, MODE>(a, e, off, da + k, col);
#pragma unroll
        for (int i = 0; i < N; i++) dd = dd + col[i] * y[i];
        v[k] = dd * scale;
      }
    }
    REAL* qp = a.qpos + e * a.nq + qa;
#pragma unroll
    for (int k = 0; k < 7; k++)
      if (k < nqj) q[k] = qp[k];
    qpos_integrate_joint<REAL>(t, q, v, (REAL)1, o);
#pragma unroll
    for (int k = 0; k < 7; k++)
      if (k < nqj) qp[k] = o[k];
  }
  if (l == 0) a.steps[e] = a.steps[e] + 1;
}
