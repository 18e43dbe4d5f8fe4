// mjh_dynamics.h -- the reference's tendon / transmission (_src/smooth.py:470-497, 535-591), passive (_src/passive.py) and the stages of forward.py:87-228
// (_velocity's two products, _actuation, _acceleration) as functions on a caller's Data: each reads the leaves it is handed AS THEY ARE (nothing is recomputed from
// qpos that the function does not itself compute from qpos) and writes fresh ones.  Six operations (DynArgs.op), one kernel each.
//
// Sums over k (a vector's components), over a tendon's joint terms, over tendons, over actuators and over dofs run in ascending index order from 0 (s = 0; s += term).
// "bodies(d)" is the range [dof_bodyid[d], body_subtree_end[dof_bodyid[d]]) -- bodies are in depth-first order, so these are exactly the bodies whose dof chain holds
// d -- taken in ascending order: the reference's sum over ALL bodies with the terms its 0 / 1 ancestor mask makes exact zeros left out.  jacp / jacr of a point on
// body b at dof d are support.jac's: off = point - subtree_com[body_rootid[b]], jacp = cdof[d][3:] + cdof[d][:3] x off, jacr = cdof[d][:3] (mjh_support.h's sup_jac_dof
// with the mask known to be 1).
//
// TENDON        (smooth.py:470-497)  ten_length[t] = sum over the tendon's joint terms of coef * qpos[qposadr];  ten_J[t][d] = the term's coef at its dof (the last term
//               of a dof wins), 0 elsewhere -- the compiled model's constant matrix.  A model whose tendons have no joint terms: zeros.
// TRANSMISSION  (smooth.py:535-591)  per actuator i with gear g:  TENDON: length = ten_length[id] g[0], moment row = ten_J[id] g[0].  SLIDE / HINGE: length = qpos g[0],
//               moment = g[0] at the dof.  BALL: axis, angle = quat_to_axis_angle(q); a = g[:3], under JOINTINPARENT rotate(g[:3], q^-1); length = (axis[0] angle) a[0] +
//               (axis[1] angle) a[1] + (axis[2] angle) a[2]; moment = a at the three dofs.  FREE: length 0, moment = g[:6], under JOINTINPARENT [g[:3], rotate(g[3:], q^-1)].
// VELOCITY      (forward.py:87-95)   actuator_velocity[i] = sum_d actuator_moment[i][d] qvel[d];  ten_velocity[t] = sum_d ten_J[t][d] qvel[d].
// PASSIVE       (passive.py:80-200)  (SPRING or DAMPER disabled: zeros, no launch.)  q[d] = -stiffness (qpos - qpos_spring) for slide / hinge and a free joint's
//               translations, -stiffness quat_sub(q, q_spring) for ball joints and a free joint's rotations;  q[d] = (0 + q[d]) - dof_damping[d] qvel[d];
//               f[t] = stiffness (lo - len) where lo - len > 0, stiffness (hi - len) where hi - len < 0 (this side wins), else 0, [lo, hi] = tendon_lengthspring;
//               f[t] = f[t] + (-tendon_damping[t] ten_velocity[t]);  q[d] += sum_t ten_J[t][d] f[t].
//               gravcomp (the model has it and GRAVITY is not disabled): qfrc_gravcomp[d] = sum over bodies(d) of jacp(xipos[b]) . (-gravity (mass gravcomp)[b]);
//               q[d] += qfrc_gravcomp[d] (1 - jnt_actgravcomp[dof_jntid[d]]).
//               fluid (the options carry fluid parameters): per body the inertia-box wrench of passive.py:31-78 (wind, viscosity, density, the mass > 0 guard, the 1e-12
//               clamps) from ximat, cvel, xipos, subtree_com;  q[d] += sum over bodies(d) of (jacp . force + jacr . torque).
// ACTUATION     (forward.py:102-219) (no actuators or ACTUATION disabled: zeros, no launch.)  ctrl clamped to ctrlrange where limited unless CLAMPCTRL is disabled;
//               act_dot by dyntype (NONE: none; INTEGRATOR: ctrl; FILTER / FILTEREXACT: (ctrl - act) / max(dynprm[0], mjMINVAL); MUSCLE: support.muscle_dynamics);
//               the control the gain sees: ctrl, for a stateful actuator act[actadr + actnum - 1];  force = gain * that + bias (FIXED / AFFINE / MUSCLE, NONE / AFFINE / MUSCLE),
//               clamped to forcerange where limited;  qfrc_actuator[d] = sum_i actuator_moment[i][d] force[i], + qfrc_gravcomp[d] jnt_actgravcomp[dof_jntid[d]] on gravcomp
//               models, clamped to jnt_actfrcrange of the dof's joint where limited.
// ACCELERATION  (forward.py:222-228) applied[d] = qfrc_applied[d] + sum over bodies(d) of (jacp(xipos[b]) . xfrc[b][:3] + jacr . xfrc[b][3:]);
//               qfrc_smooth = ((qfrc_passive - qfrc_bias) + qfrc_actuator) + applied;  qacc_smooth = small_cholesky_solve(qfrc_smooth, qLD): itg_chol_solve of
//               mjh_integrate.h on the packed lower triangle of the caller's qLD in LDS.
//
// The packing of mjh_smooth.h: `lanes` (16 / 32 / 64, from nv for TENDON, PASSIVE and ACCELERATION, from nu for TRANSMISSION, VELOCITY and ACTUATION) lanes serve one
// environment, up to 256 / lanes environments share a workgroup, an environment's lanes lie inside one wavefront (wave barriers only).  A leaf several lanes need goes
// to LDS in one flat coalesced pass (qpos, qvel, the matrices of VELOCITY, xipos / subtree_com, qLD); a matrix read once (ten_J in PASSIVE, actuator_moment in ACTUATION)
// is read column by column, consecutive lanes consecutive addresses.  LDS per environment, in reals: TENDON nq; TRANSMISSION nq + ntendon + 3 nu; VELOCITY
// nv + (nu + ntendon) (nv | 1) (an odd row stride); PASSIVE nv + ntendon + 12 nbody; ACTUATION nu; ACCELERATION nv (nv + 1) / 2 (rounded up to 4) + nv + 6 nbody.
// No atomics: every sum has one fixed order, so a result depends neither on the lanes, nor on B, nor on the environment's slot, nor on how the host cut the batch.
// The model VALUES are arguments of the call (the caller's Model's), not the blob's; the structure (which actuator drives what, the types, the limited flags, the
// tendons' joint terms, the tree) is the blob's.  The muscle functions restate those of the pass kernel (mjh_kernels.h, members of its stage class), support.py:197-296.
#pragma once
#include "mjh_device.h"
#include "mjh_integrate.h"

#define MJH_DYNAMICS_WG 256

template <typename REAL>
struct DynArgs {
  // [B, ...] leaves of the caller's Data
  const REAL *qpos, *qvel, *ctrl, *act, *ten_length, *ten_velocity, *ten_J, *actuator_length, *actuator_velocity, *actuator_moment, *xipos, *ximat, *subtree_com, *cdof,
      *cvel, *qfrc_gravcomp, *qfrc_applied, *xfrc_applied, *qfrc_passive, *qfrc_bias, *qfrc_actuator, *qLD;
  // the caller's model values; gainprm / biasprm / dynprm are [nu, *_stride]
  const REAL *jnt_stiffness, *qpos_spring, *dof_damping, *tendon_stiffness, *tendon_damping, *tendon_lengthspring, *body_mass, *body_inertia, *body_gravcomp,
      *jnt_actgravcomp, *jnt_actfrcrange, *gainprm, *biasprm, *dynprm, *ctrlrange, *forcerange, *gear, *lengthrange, *acc0;
  // structure (the blob)
  const int *body_rootid, *body_subtree_end, *jnt_type, *jnt_qposadr, *jnt_dofadr, *jnt_actfrclimited, *dof_bodyid, *dof_jntid, *ten_adr, *ten_qposadr, *act_trntype,
      *act_trnid, *act_jnttype, *act_dofadr, *act_qposadr, *act_gaintype, *act_biastype, *act_dyntype, *act_ctrllimited, *act_forcelimited, *act_actadr, *act_actnum;
  const REAL *ten_coef, *ten_J0;
  // outputs
  REAL *ten_length_out, *ten_J_out, *actuator_length_out, *actuator_moment_out, *actuator_velocity_out, *ten_velocity_out, *qfrc_passive_out, *qfrc_gravcomp_out,
      *act_dot_out, *qfrc_actuator_out, *actuator_force_out, *qfrc_smooth_out, *qacc_smooth_out;
  REAL gravity[3], wind[3], density, viscosity;
  int nq, nv, nu, na, nbody, njnt, ntendon;
  int gain_stride, bias_stride, dyn_stride;
  int gravcomp, fluid, clampctrl;  // gravcomp: the term is computed (the model has it, GRAVITY on; ACTUATION: the model has it); fluid: the options carry fluid parameters
  int lanes, envs;                 // lanes per environment, environments per workgroup
  int lds_env;                     // REALs of LDS per environment (a multiple of 4)
  int64_t env_begin, env_count;
};

// n reals of one environment's leaf into LDS, flat: consecutive lanes read consecutive elements
template <typename REAL>
__device__ __forceinline__ void dyn_load(REAL* dst, const REAL* src, int n, int l, int L) {
  for (int w = l; w < n; w += L) dst[w] = src[w];
}

// jacp / jacr (support.jac :138-153) of `point` at a dof whose body is an ancestor-or-self of the point's body: cd the dof's cdof row, rc subtree_com of the body's root
template <typename REAL>
__device__ __forceinline__ void dyn_jac_dof(const REAL* cd, const REAL* rc, const REAL* point, REAL* jp, REAL* jr) {
  const REAL off[3] = {point[0] - rc[0], point[1] - rc[1], point[2] - rc[2]};
  REAL c[3];
  cross3(cd, off, c);
#pragma unroll
  for (int i = 0; i < 3; i++) { jp[i] = cd[3 + i] + c[i]; jr[i] = cd[i]; }
}

// ---- muscle actuators (support.py:197-296), as in the pass kernel ----
template <typename REAL> __device__ __forceinline__ REAL dyn_clamp_min(REAL x, REAL lo) { return x > lo ? x : lo; }
template <typename REAL> __device__ __forceinline__ REAL dyn_sq(REAL x) { return x * x; }
template <typename REAL>
__device__ __forceinline__ REAL dyn_muscle_sigmoid(REAL x) {  // :197-202
  REAL sol = x * x * x * (3 * x * (2 * x - 5) + 10);
  sol = x <= 0 ? (REAL)0 : sol;
  return x >= 1 ? (REAL)1 : sol;
}
template <typename REAL>
__device__ __forceinline__ REAL dyn_muscle_dynamics(REAL ctrl, REAL act, const REAL* prm) {  // :205-232
  const REAL ctrlclamp = ctrl < 0 ? (REAL)0 : (ctrl > 1 ? (REAL)1 : ctrl), actclamp = act < 0 ? (REAL)0 : (act > 1 ? (REAL)1 : act);
  const REAL tau_act = prm[0] * ((REAL)0.5 + (REAL)1.5 * actclamp), tau_deact = prm[1] / ((REAL)0.5 + (REAL)1.5 * actclamp), width = prm[2];
  const REAL dctrl = ctrlclamp - act;
  const REAL tau_hard = dctrl > 0 ? tau_act : tau_deact;
  const REAL q = dctrl / (width + (width == 0 ? (REAL)(float)mjMINVAL : (REAL)0));  // math.safe_div
  const REAL tau_smooth = tau_deact + (tau_act - tau_deact) * dyn_muscle_sigmoid<REAL>(q + (REAL)0.5);
  const REAL tau = width < (REAL)mjMINVAL ? tau_hard : tau_smooth;
  return dctrl / dyn_clamp_min<REAL>(tau, (REAL)mjMINVAL);
}
template <typename REAL>
__device__ __forceinline__ REAL dyn_muscle_gain_length(REAL len, REAL lmin, REAL lmax) {  // :235-249
  const REAL a = (REAL)0.5 * (lmin + 1), b = (REAL)0.5 * (1 + lmax);
  const REAL out0 = (REAL)0.5 * dyn_sq<REAL>((len - lmin) / dyn_clamp_min<REAL>(a - lmin, (REAL)mjMINVAL));
  const REAL out1 = 1 - (REAL)0.5 * dyn_sq<REAL>((1 - len) / dyn_clamp_min<REAL>(1 - a, (REAL)mjMINVAL));
  const REAL out2 = 1 - (REAL)0.5 * dyn_sq<REAL>((len - 1) / dyn_clamp_min<REAL>(b - 1, (REAL)mjMINVAL));
  const REAL out3 = (REAL)0.5 * dyn_sq<REAL>((lmax - len) / dyn_clamp_min<REAL>(lmax - b, (REAL)mjMINVAL));
  REAL o = len <= b ? out2 : out3;
  o = len <= 1 ? out1 : o;
  o = len <= a ? out0 : o;
  return (lmin <= len && len <= lmax) ? o : (REAL)0;
}
template <typename REAL>
__device__ __forceinline__ REAL dyn_muscle_gain(REAL len, REAL vel, const REAL* lr, REAL acc0, const REAL* prm) {  // :252-278
  REAL force = prm[2];
  const REAL scale = prm[3], lmin = prm[4], lmax = prm[5], vmax = prm[6], fvmax = prm[8];
  force = force < 0 ? scale / dyn_clamp_min<REAL>(acc0, (REAL)mjMINVAL) : force;
  const REAL L0 = (lr[1] - lr[0]) / dyn_clamp_min<REAL>(prm[1] - prm[0], (REAL)mjMINVAL);
  const REAL L = prm[0] + (len - lr[0]) / dyn_clamp_min<REAL>(L0, (REAL)mjMINVAL);
  const REAL V = vel / dyn_clamp_min<REAL>(L0 * vmax, (REAL)mjMINVAL);
  const REAL FL = dyn_muscle_gain_length<REAL>(L, lmin, lmax);
  const REAL y = fvmax - 1;
  REAL FV = V <= y ? fvmax - dyn_sq<REAL>(y - V) / dyn_clamp_min<REAL>(y, (REAL)mjMINVAL) : fvmax;
  FV = V <= 0 ? dyn_sq<REAL>(V + 1) : FV;
  FV = V <= -1 ? (REAL)0 : FV;
  return -force * FL * FV;
}
template <typename REAL>
__device__ __forceinline__ REAL dyn_muscle_bias(REAL len, const REAL* lr, REAL acc0, const REAL* prm) {  // :281-296
  REAL force = prm[2];
  const REAL scale = prm[3], lmax = prm[5], fpmax = prm[7];
  force = force < 0 ? scale / dyn_clamp_min<REAL>(acc0, (REAL)mjMINVAL) : force;
  const REAL L0 = (lr[1] - lr[0]) / dyn_clamp_min<REAL>(prm[1] - prm[0], (REAL)mjMINVAL);
  const REAL L = prm[0] + (len - lr[0]) / dyn_clamp_min<REAL>(L0, (REAL)mjMINVAL);
  const REAL b = (REAL)0.5 * (1 + lmax);
  const REAL out1 = -force * fpmax * (REAL)0.5 * dyn_sq<REAL>((L - 1) / dyn_clamp_min<REAL>(b - 1, (REAL)mjMINVAL));
  const REAL out2 = -force * fpmax * ((REAL)0.5 + (L - b) / dyn_clamp_min<REAL>(b - 1, (REAL)mjMINVAL));
  const REAL o = L <= b ? out1 : out2;
  return L <= 1 ? (REAL)0 : o;
}

template <typename REAL, int OP>
__global__ __launch_bounds__(MJH_DYNAMICS_WG) void mjh_dynamics_kernel(DynArgs<REAL> a) {
  extern __shared__ __attribute__((aligned(16))) double dyn_lds_raw[];
  const int L = a.lanes;
  const int slot = (int)threadIdx.x / L, l = (int)threadIdx.x - slot * L;
  const int64_t e = a.env_begin + (int64_t)blockIdx.x * a.envs + slot;
  if (slot >= a.envs || e >= a.env_begin + a.env_count) return;  // (whole environments only: an environment's lanes all return or none do)
  const int nq = a.nq, nv = a.nv, nu = a.nu, nb = a.nbody, nt = a.ntendon;
  REAL* lds = reinterpret_cast<REAL*>(dyn_lds_raw) + (int64_t)slot * a.lds_env;

  if constexpr (OP == MJH_DYNAMICS_TENDON) {
    REAL* qp = lds;  // nq: qpos
    dyn_load<REAL>(qp, a.qpos + e * nq, nq, l, L);
    wave_sync();
    for (int t = l; t < nt; t += L) {
      REAL len = 0;
      for (int q = a.ten_adr[t]; q < a.ten_adr[t + 1]; q++) len += a.ten_coef[q] * qp[a.ten_qposadr[q]];
      a.ten_length_out[e * nt + t] = len;
    }
    REAL* J = a.ten_J_out + e * nt * nv;
    for (int w = l; w < nt * nv; w += L) J[w] = a.ten_J0[w];
  }

  if constexpr (OP == MJH_DYNAMICS_TRANSMISSION) {
    REAL* qp = lds;        // nq: qpos
    REAL* tl = qp + nq;    // ntendon: ten_length
    REAL* ga = tl + nt;    // 3 nu: the gear axis of a ball / free joint's rotations
    dyn_load<REAL>(qp, a.qpos + e * nq, nq, l, L);
    dyn_load<REAL>(tl, a.ten_length + e * nt, nt, l, L);
    wave_sync();
    for (int i = l; i < nu; i += L) {
      const REAL* gear = a.gear + 6 * i;
      const int jt = a.act_jnttype[i], qa = a.act_qposadr[i], trn = a.act_trntype[i];
      REAL len = 0;
      if (trn == 3) {
        len = tl[a.act_trnid[i]] * gear[0];
      } else if (jt == JNT_SLIDE || jt == JNT_HINGE) {
        len = qp[qa] * gear[0];
      } else {
        const int go = jt == JNT_FREE ? 3 : 0;
        const REAL* q4 = qp + qa + go;
        REAL g3[3] = {gear[go], gear[go + 1], gear[go + 2]};
        if (trn == 1) {  // JOINTINPARENT: the gear axis in the child frame
          const REAL qn[4] = {q4[0], q4[1] * (REAL)-1, q4[2] * (REAL)-1, q4[3] * (REAL)-1};
          const REAL gv[3] = {g3[0], g3[1], g3[2]};
          rotate(gv, qn, g3);
        }
        ga[3 * i] = g3[0]; ga[3 * i + 1] = g3[1]; ga[3 * i + 2] = g3[2];
        if (jt == JNT_BALL) {
          const REAL q[4] = {q4[0], q4[1], q4[2], q4[3]};
          REAL axis[3], angle;
          quat_to_axis_angle(q, axis, angle);
          len = ((axis[0] * angle) * g3[0] + (axis[1] * angle) * g3[1]) + (axis[2] * angle) * g3[2];
        }
      }
      a.actuator_length_out[e * nu + i] = len;
    }
    wave_sync();
    REAL* mom = a.actuator_moment_out + e * nu * nv;
    for (int w = l; w < nu * nv; w += L) {
      const int i = w / nv, d = w - i * nv;
      const int jt = a.act_jnttype[i], k = d - a.act_dofadr[i];
      REAL v = 0;
      if (a.act_trntype[i] == 3) v = a.ten_J[(e * nt + a.act_trnid[i]) * nv + d] * a.gear[6 * i];
      else if (jt == JNT_SLIDE || jt == JNT_HINGE) v = k == 0 ? a.gear[6 * i] : (REAL)0;
      else if (jt == JNT_BALL) v = (k >= 0 && k < 3) ? ga[3 * i + k] : (REAL)0;
      else v = (k >= 0 && k < 3) ? a.gear[6 * i + k] : ((k >= 3 && k < 6) ? ga[3 * i + k - 3] : (REAL)0);
      mom[w] = v;
    }
  }

  if constexpr (OP == MJH_DYNAMICS_VELOCITY) {
    const int ld = nv | 1;       // odd row stride: the lanes of a pass read one column of different rows, on different banks
    REAL* qv = lds;              // nv: qvel
    REAL* M = qv + nv;           // (nu + ntendon) ld: the rows of actuator_moment, then of ten_J
    dyn_load<REAL>(qv, a.qvel + e * nv, nv, l, L);
    const REAL* mom = a.actuator_moment + e * nu * nv;
    for (int w = l; w < nu * nv; w += L) { const int r = w / nv; M[r * ld + (w - r * nv)] = mom[w]; }
    const REAL* tj = a.ten_J + e * nt * nv;
    for (int w = l; w < nt * nv; w += L) { const int r = w / nv; M[(nu + r) * ld + (w - r * nv)] = tj[w]; }
    wave_sync();
    for (int r = l; r < nu + nt; r += L) {
      REAL s = 0;
      for (int d = 0; d < nv; d++) s += M[r * ld + d] * qv[d];
      if (r < nu) a.actuator_velocity_out[e * nu + r] = s;
      else a.ten_velocity_out[e * nt + r - nu] = s;
    }
  }

  if constexpr (OP == MJH_DYNAMICS_PASSIVE) {
    REAL* qf = lds;              // nv: the joint springs, by dof
    REAL* tf = qf + nv;          // ntendon: the tendons' spring + damper force
    REAL* xip = tf + nt;         // 3 nbody: xipos
    REAL* com = xip + 3 * nb;    // 3 nbody: subtree_com
    REAL* wr = com + 3 * nb;     // 6 nbody: the fluid wrench [force, torque]
    const bool bodies = a.gravcomp || a.fluid;
    if (bodies) {
      dyn_load<REAL>(xip, a.xipos + e * nb * 3, nb * 3, l, L);
      dyn_load<REAL>(com, a.subtree_com + e * nb * 3, nb * 3, l, L);
    }
    const REAL* qpos = a.qpos + e * nq;
    for (int j = l; j < a.njnt; j += L) {
      const int t = a.jnt_type[j], qa = a.jnt_qposadr[j], da = a.jnt_dofadr[j];
      const REAL k = a.jnt_stiffness[j];
      if (t == JNT_FREE || t == JNT_BALL) {
        int qo = qa, dd = da;
        if (t == JNT_FREE) {
          for (int i = 0; i < 3; i++) qf[da + i] = -k * (qpos[qa + i] - a.qpos_spring[qa + i]);
          qo = qa + 3; dd = da + 3;
        }
        const REAL q[4] = {qpos[qo], qpos[qo + 1], qpos[qo + 2], qpos[qo + 3]};
        const REAL qs[4] = {a.qpos_spring[qo], a.qpos_spring[qo + 1], a.qpos_spring[qo + 2], a.qpos_spring[qo + 3]};
        REAL r[3];
        quat_sub(q, qs, r);
        for (int i = 0; i < 3; i++) qf[dd + i] = -k * r[i];
      } else {
        qf[da] = -k * (qpos[qa] - a.qpos_spring[qa]);
      }
    }
    for (int t = l; t < nt; t += L) {
      const REAL len = a.ten_length[e * nt + t];
      const REAL below = a.tendon_lengthspring[2 * t] - len, above = a.tendon_lengthspring[2 * t + 1] - len;
      REAL fs = below > 0 ? a.tendon_stiffness[t] * below : (REAL)0;
      fs = above < 0 ? a.tendon_stiffness[t] * above : fs;
      tf[t] = fs + (-a.tendon_damping[t] * a.ten_velocity[e * nt + t]);
    }
    if (a.fluid) {  // passive._inertia_box_fluid_model :31-78, one lane per body
      for (int b = l; b < nb; b += L) {
        const REAL pi = (REAL)3.14159265358979323846;
        const REAL* inr = a.body_inertia + 3 * b;
        const REAL mass = a.body_mass[b];
        REAL box[3];
#pragma unroll
        for (int i = 0; i < 3; i++) {
          REAL s3 = (inr[0] * (i == 0 ? (REAL)-1 : (REAL)1) + inr[1] * (i == 1 ? (REAL)-1 : (REAL)1)) + inr[2] * (i == 2 ? (REAL)-1 : (REAL)1);
          s3 = s3 > (REAL)1e-12 ? s3 : (REAL)1e-12;
          const REAL mm = mass > (REAL)(float)1e-12 ? mass : (REAL)(float)1e-12;
          box[i] = r_sqrt<REAL>(((REAL)6.0 * s3) / mm) * (REAL)(mass > 0);
        }
        REAL xi[9], cv[6];
#pragma unroll
        for (int i = 0; i < 9; i++) xi[i] = a.ximat[(e * nb + b) * 9 + i];
#pragma unroll
        for (int i = 0; i < 6; i++) cv[i] = a.cvel[(e * nb + b) * 6 + i];
        const REAL* rc = com + 3 * a.body_rootid[b];
        const REAL off[3] = {xip[3 * b] - rc[0], xip[3 * b + 1] - rc[1], xip[3 * b + 2] - rc[2]};
        REAL c[3], v3[3], lvel[6], lwind[3];
        cross3(off, cv, c);  // math.transform_motion :437-452
#pragma unroll
        for (int i = 0; i < 3; i++) v3[i] = cv[3 + i] - c[i];
#pragma unroll
        for (int i = 0; i < 3; i++) {
          lvel[3 + i] = xi[i] * v3[0] + xi[3 + i] * v3[1] + xi[6 + i] * v3[2];
          lvel[i] = xi[i] * cv[0] + xi[3 + i] * cv[1] + xi[6 + i] * cv[2];
          lwind[i] = xi[i] * a.wind[0] + xi[3 + i] * a.wind[1] + xi[6 + i] * a.wind[2];
        }
#pragma unroll
        for (int i = 0; i < 3; i++) lvel[3 + i] = lvel[3 + i] + (-lwind[i]);
        const REAL diam = ((box[0] + box[1]) + box[2]) / 3;
        const REAL d3 = diam * diam * diam;
        REAL fa[3], fv[3];
#pragma unroll
        for (int i = 0; i < 3; i++) {
          fa[i] = lvel[i] * -pi * d3 * a.viscosity;
          fv[i] = lvel[3 + i] * (REAL)-3.0 * pi * diam * a.viscosity;
        }
        const REAL sv[3] = {box[1] * box[2], box[0] * box[2], box[0] * box[1]};
        const REAL b4[3] = {r_pow<REAL>(box[0], (REAL)4), r_pow<REAL>(box[1], (REAL)4), r_pow<REAL>(box[2], (REAL)4)};
        const REAL sa[3] = {box[0] * (b4[1] + b4[2]), box[1] * (b4[0] + b4[2]), box[2] * (b4[0] + b4[1])};
#pragma unroll
        for (int i = 0; i < 3; i++) {
          fv[i] = fv[i] - (REAL)0.5 * a.density * sv[i] * r_abs(lvel[3 + i]) * lvel[3 + i];
          fa[i] = fa[i] - ((REAL)1.0 * a.density * sa[i] * r_abs(lvel[i]) * lvel[i] / (REAL)64.0);
        }
#pragma unroll
        for (int i = 0; i < 3; i++) {
          wr[6 * b + i] = xi[3 * i] * fv[0] + xi[3 * i + 1] * fv[1] + xi[3 * i + 2] * fv[2];        // force
          wr[6 * b + 3 + i] = xi[3 * i] * fa[0] + xi[3 * i + 1] * fa[1] + xi[3 * i + 2] * fa[2];    // torque
        }
      }
    }
    wave_sync();
    for (int d = l; d < nv; d += L) {
      REAL q = ((REAL)0 + qf[d]) - a.dof_damping[d] * a.qvel[e * nv + d];
      if (nt > 0) {
        REAL acc = 0;
        for (int t = 0; t < nt; t++) acc += a.ten_J[(e * nt + t) * nv + d] * tf[t];
        q = q + acc;
      }
      if (bodies) {
        REAL cd[6];
#pragma unroll
        for (int k = 0; k < 6; k++) cd[k] = a.cdof[(e * nv + d) * 6 + k];
        const int b0 = a.dof_bodyid[d], b1 = a.body_subtree_end[b0];
        if (a.gravcomp) {
          REAL acc = 0;
          for (int b = b0; b < b1; b++) {
            const REAL mg = a.body_mass[b] * a.body_gravcomp[b];
            const REAL f[3] = {-a.gravity[0] * mg, -a.gravity[1] * mg, -a.gravity[2] * mg};
            REAL jp[3], jr[3];
            dyn_jac_dof<REAL>(cd, com + 3 * a.body_rootid[b], xip + 3 * b, jp, jr);
            acc += (jp[0] * f[0] + jp[1] * f[1]) + jp[2] * f[2];
          }
          a.qfrc_gravcomp_out[e * nv + d] = acc;
          q = q + acc * ((REAL)1 - a.jnt_actgravcomp[a.dof_jntid[d]]);
        }
        if (a.fluid) {
          REAL acc = 0;
          for (int b = b0; b < b1; b++) {
            REAL jp[3], jr[3];
            dyn_jac_dof<REAL>(cd, com + 3 * a.body_rootid[b], xip + 3 * b, jp, jr);
            const REAL* w6 = wr + 6 * b;
            acc += ((jp[0] * w6[0] + jp[1] * w6[1]) + jp[2] * w6[2]) + ((jr[0] * w6[3] + jr[1] * w6[4]) + jr[2] * w6[5]);
          }
          q = q + acc;
        }
      }
      a.qfrc_passive_out[e * nv + d] = q;
    }
  }

  if constexpr (OP == MJH_DYNAMICS_ACTUATION) {
    REAL* frc = lds;  // nu: the actuator forces
    for (int i = l; i < nu; i += L) {
      REAL ctrl = a.ctrl[e * nu + i];
      const int dyn = a.act_dyntype[i], gt = a.act_gaintype[i], bt = a.act_biastype[i];
      const REAL* gp = a.gainprm + (int64_t)i * a.gain_stride;
      const REAL* bp = a.biasprm + (int64_t)i * a.bias_stride;
      if (a.clampctrl && a.act_ctrllimited[i]) {
        const REAL clo = a.ctrlrange[2 * i], chi = a.ctrlrange[2 * i + 1];
        ctrl = ctrl > clo ? ctrl : clo;
        ctrl = ctrl < chi ? ctrl : chi;
      }
      REAL ctrl_act = ctrl;
      if (dyn != DYN_NONE) {
        const int ad = a.act_actadr[i];
        const REAL act = a.act[e * a.na + ad];
        REAL dot;
        if (dyn == DYN_INTEGRATOR) dot = ctrl;
        else if (dyn == DYN_MUSCLE) dot = dyn_muscle_dynamics<REAL>(ctrl, act, a.dynprm + (int64_t)i * a.dyn_stride);
        else {
          REAL tau = a.dynprm[(int64_t)i * a.dyn_stride];
          tau = tau > (REAL)mjMINVAL ? tau : (REAL)mjMINVAL;
          dot = (ctrl - act) / tau;
        }
        a.act_dot_out[e * a.na + ad] = dot;
        ctrl_act = a.act[e * a.na + ad + a.act_actnum[i] - 1];
      }
      const REAL len = a.actuator_length[e * nu + i], vel = a.actuator_velocity[e * nu + i];
      REAL gain = (gt == GAIN_FIXED) ? gp[0] : gp[0] + gp[1] * len + gp[2] * vel;
      REAL bias = (bt == BIAS_AFFINE) ? bp[0] + bp[1] * len + bp[2] * vel : (REAL)0;
      if (gt == GAIN_MUSCLE) gain = dyn_muscle_gain<REAL>(len, vel, a.lengthrange + 2 * i, a.acc0[i], gp);
      if (bt == BIAS_MUSCLE) bias = dyn_muscle_bias<REAL>(len, a.lengthrange + 2 * i, a.acc0[i], bp);
      REAL force = gain * ctrl_act + bias;
      if (a.act_forcelimited[i]) {
        const REAL flo = a.forcerange[2 * i], fhi = a.forcerange[2 * i + 1];
        force = force < flo ? flo : (force > fhi ? fhi : force);
      }
      frc[i] = force;
      a.actuator_force_out[e * nu + i] = force;
    }
    wave_sync();
    const REAL* mom = a.actuator_moment + e * nu * nv;
    for (int d = l; d < nv; d += L) {
      REAL s = 0;
      for (int i = 0; i < nu; i++) s += mom[i * nv + d] * frc[i];
      const int j = a.dof_jntid[d];
      if (a.gravcomp) s = s + a.qfrc_gravcomp[e * nv + d] * a.jnt_actgravcomp[j];
      if (a.jnt_actfrclimited[j]) {
        const REAL flo = a.jnt_actfrcrange[2 * j], fhi = a.jnt_actfrcrange[2 * j + 1];
        s = s < flo ? flo : (s > fhi ? fhi : s);
      }
      a.qfrc_actuator_out[e * nv + d] = s;
    }
  }

  if constexpr (OP == MJH_DYNAMICS_ACCELERATION) {
    const int ntri = (nv * (nv + 1)) / 2;
    REAL* A = lds;                      // the packed lower triangle of qLD
    REAL* x = A + ((ntri + 3) & ~3);    // nv: qfrc_smooth -> qacc_smooth
    REAL* xip = x + nv;                 // 3 nbody: xipos
    REAL* com = xip + 3 * nb;           // 3 nbody: subtree_com
    const REAL* qLD = a.qLD + e * nv * nv;
    for (int w = l; w < nv * nv; w += L) {
      const int r = w / nv, c = w - r * nv;
      const REAL v = qLD[w];
      if (c <= r) A[itg_tri(r, c)] = v;
    }
    dyn_load<REAL>(xip, a.xipos + e * nb * 3, nb * 3, l, L);
    dyn_load<REAL>(com, a.subtree_com + e * nb * 3, nb * 3, l, L);
    wave_sync();
    for (int d = l; d < nv; d += L) {
      REAL cd[6];
#pragma unroll
      for (int k = 0; k < 6; k++) cd[k] = a.cdof[(e * nv + d) * 6 + k];
      const int b0 = a.dof_bodyid[d], b1 = a.body_subtree_end[b0];
      REAL acc = 0;
      for (int b = b0; b < b1; b++) {
        const REAL* f = a.xfrc_applied + (e * nb + b) * 6;
        REAL jp[3], jr[3];
        dyn_jac_dof<REAL>(cd, com + 3 * a.body_rootid[b], xip + 3 * b, jp, jr);
        acc += ((jp[0] * f[0] + jp[1] * f[1]) + jp[2] * f[2]) + ((jr[0] * f[3] + jr[1] * f[4]) + jr[2] * f[5]);
      }
      const REAL applied = a.qfrc_applied[e * nv + d] + acc;
      const REAL s = ((a.qfrc_passive[e * nv + d] - a.qfrc_bias[e * nv + d]) + a.qfrc_actuator[e * nv + d]) + applied;
      x[d] = s;
      a.qfrc_smooth_out[e * nv + d] = s;
    }
    wave_sync();
    itg_chol_solve<REAL>(A, x, nv, l, L);
    for (int d = l; d < nv; d += L) a.qacc_smooth_out[e * nv + d] = x[d];
  }
}
