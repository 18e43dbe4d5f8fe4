// mjh_qpos.h -- configuration arithmetic on plain qpos / qvel rows (MuJoCo's mj_integratePos, mj_differentiatePos, mj_normalizeQuat): ONE LANE PER
// (environment, joint), environment-major.  Joint type and addresses are the model's; no LDS, no cross-lane traffic, nothing kept between items.
//
// Definitions, per joint (qa = jnt_qposadr, da = jnt_dofadr):
//  * INTEGRATE      out[qa..] = a ⊕ dt b, a = qpos, b = qvel: the step's integrate_pos (mjh_kernels.h; reference forward.py:231-252) -- slide / hinge q + dt v, a free
//                   joint's position p + dt v, every quaternion quat_integrate(q, w, dt) (mjh_device.h) = normalize(q ⊗ [cos(dt|w|/2), â sin(dt|w|/2)]),
//                   â = w / (|w| + 1e-6 [|w| == 0]).  Same device functions, same expression order as the step.
//  * DIFFERENTIATE  out[da..] = (b ⊖ a) / dt, a = qpos1, b = qpos2: scalars and positions (b - a) / dt, every quaternion quat_sub(b, a) / dt (mjh_device.h;
//                   reference math.py:276-280, 354-360): axis times angle of a^-1 ⊗ b, angle = 2 atan2(|xyz|, w) taken into (-pi, pi], the zero vector when |xyz| == 0.
//                   The difference is in the frame INTEGRATE advances in: INTEGRATE(a, DIFFERENTIATE(a, b, dt), dt) is b as a rotation (possibly -b).
//  * NORMALIZE      out[qa..] = a with every ball / free quaternion divided by its norm, (1, 0, 0, 0) where the norm is below 1e-15 (mjMINVAL); every other
//                   entry is copied bit for bit.
// qpos_integrate_joint is what mjh_ik.h applies its update with.
#pragma once
#include "mjh_device.h"  // (MJH_QPOS_*: include/mjhip.h)

template <typename REAL>
struct QposArithArgs {
  const REAL *a, *b;  // INTEGRATE: qpos [B, nq], qvel [B, nv]; DIFFERENTIATE: qpos1, qpos2 [B, nq]; NORMALIZE: qpos [B, nq], b unused
  REAL* out;          // [B, nq]; DIFFERENTIATE: [B, nv]
  const int *jnt_type, *jnt_qposadr, *jnt_dofadr;
  int64_t item_begin, item_count;  // this launch: items [item_begin, item_begin + item_count) of B * njnt, item = environment * njnt + joint
  int njnt, nq, nv, op;
  REAL dt;
};

// one joint of integrate_pos: q -> o (its qpos entries), v its dofs
template <typename REAL>
__device__ __forceinline__ void qpos_integrate_joint(int t, const REAL* q, const REAL* v, REAL dt, REAL* o) {
  if (t == JNT_FREE) {
    for (int i = 0; i < 3; i++) o[i] = q[i] + dt * v[i];
    REAL q4[4] = {q[3], q[4], q[5], q[6]}, w[3] = {v[3], v[4], v[5]}, r[4];
    quat_integrate(q4, w, dt, r);
    for (int i = 0; i < 4; i++) o[3 + i] = r[i];
  } else if (t == JNT_BALL) {
    REAL q4[4] = {q[0], q[1], q[2], q[3]}, w[3] = {v[0], v[1], v[2]}, r[4];
    quat_integrate(q4, w, dt, r);
    for (int i = 0; i < 4; i++) o[i] = r[i];
  } else {
    o[0] = q[0] + dt * v[0];
  }
}

template <typename REAL>
__device__ __forceinline__ void qpos_normalize_quat(const REAL* q, REAL* o) {
  const REAL n = norm_n<REAL, 4>(q);
  const bool tiny = n < (REAL)1e-15;
  o[0] = tiny ? (REAL)1 : q[0] / n;
#pragma unroll
  for (int i = 1; i < 4; i++) o[i] = tiny ? (REAL)0 : q[i] / n;
}

// grid: ceil(item_count / 64) one-wave workgroups; no grid-stride loop
template <typename REAL>
__global__ __launch_bounds__(MJH_WAVE) void mjh_qpos_arith_kernel(QposArithArgs<REAL> a) {
  const int64_t local = (int64_t)blockIdx.x * MJH_WAVE + threadIdx.x;
  if (local >= a.item_count) return;
  const int64_t item = a.item_begin + local;
  const int64_t e = item / a.njnt;
  const int j = (int)(item - e * a.njnt);
  const int t = a.jnt_type[j], qa = a.jnt_qposadr[j], da = a.jnt_dofadr[j];
  if (a.op == MJH_QPOS_INTEGRATE) {
    qpos_integrate_joint<REAL>(t, a.a + e * a.nq + qa, a.b + e * a.nv + da, a.dt, a.out + e * a.nq + qa);
  } else if (a.op == MJH_QPOS_DIFFERENTIATE) {
    const REAL *q1 = a.a + e * a.nq + qa, *q2 = a.b + e * a.nq + qa;
    REAL* o = a.out + e * a.nv + da;
    if (t == JNT_FREE || t == JNT_BALL) {
      const int k = t == JNT_FREE ? 3 : 0;
      if (t == JNT_FREE)
        for (int i = 0; i < 3; i++) o[i] = (q2[i] - q1[i]) / a.dt;
      const REAL u[4] = {q2[k], q2[k + 1], q2[k + 2], q2[k + 3]}, v[4] = {q1[k], q1[k + 1], q1[k + 2], q1[k + 3]};
      REAL r[3];
      quat_sub(u, v, r);
      for (int i = 0; i < 3; i++) o[k + i] = r[i] / a.dt;
    } else {
      o[0] = (q2[0] - q1[0]) / a.dt;
    }
  } else {
    const REAL* q = a.a + e * a.nq + qa;
    REAL* o = a.out + e * a.nq + qa;
    if (t == JNT_FREE || t == JNT_BALL) {
      const int k = t == JNT_FREE ? 3 : 0;
      if (t == JNT_FREE)
        for (int i = 0; i < 3; i++) o[i] = q[i];
      const REAL q4[4] = {q[k], q[k + 1], q[k + 2], q[k + 3]};
      REAL r[4];
      qpos_normalize_quat(q4, r);
      for (int i = 0; i < 4; i++) o[k + i] = r[i];
    } else {
      o[0] = q[0];
    }
  }
}
