// mjh_integrate.h -- the integrators of the reference as a tail on a finished forward pass: deriv_smooth_vel (_src/derivative.py:22-68), _implicit
// (_src/forward.py:404-416, the implicitfast integrator), _euler (:313-328) and the _advance they share (:255-310).
//
// qDeriv (build):   sum_i moment[i, r] * (moment[i, c] * vel_i), actuators in index order                            unless DisableBit.ACTUATION
//                     vel_i = biasprm[i, 2] [biastype AFFINE] + gainprm[i, 2] [gaintype AFFINE] * c_i,  c_i = ctrl[i] (dyntype NONE, not clamped) or act[actadr[i]]
//                   - dof_damping[r] on the diagonal                                                                   unless DisableBit.DAMPER
//                   - sum_t (ten_J[t, r] * tendon_damping[t]) * ten_J[t, c], tendons in index order                    whenever ntendon > 0 (not under DAMPER: the reference's rule)
// implicit:         A = qM - h * qDeriv;  qacc = chol_solve(A, qfrc_smooth + qfrc_constraint)
// euler:            A = qM + diag(h * dof_damping);  qacc likewise
// neither:          qacc = the pass's (the caller's qacc leaf)
// factorisation:    math.small_cholesky (math.py:87-129): nv <= 16 the column-by-column scalar sequence, every pivot clamped at 1e-12; nv > 16 cholesky(A + 1e-10 I), no
//                   clamp (the 1e-10 is added to each pivot as its column is reached: the same factor in exact arithmetic, any order being allowed there).  Only the lower triangle of A is read, as there.  With contraction off, the right-looking sweep below subtracts the products L[i][k] L[j][k] from
//                   entry (i, j) in k order, i.e. the reference's sequence; the forward substitution likewise; the backward substitution sums k ascending for nv <= 16
//                   (:160-166; a serial chain, so every lane runs it) and column by column above (LAPACK there: any order).
// advance (state):  act: FILTEREXACT act + act_dot * tau * (1 - exp(-h / tau)), tau = max(dynprm[0], mjMINVAL), else act + act_dot * h, clamped to actrange where actlimited;
//                   qvel' = qvel + qacc * h;  qpos integrated with qvel' (quat_integrate renormalises);  time + h.
//
// The packing of mjh_energy_kernel / mjh_inverse_kernel: `lanes` (16 / 32 / 64, from nv) lanes serve one environment, up to 256 / lanes environments share a workgroup (fewer
// where the matrix of a large model needs the LDS), an environment's lanes lie inside one wavefront (wave barriers only).  No atomics, no scratch.  Per environment the LDS
// holds the packed lower triangle of A (nv (nv + 1) / 2 reals), the right-hand side, the new qvel, the actuators' vel_i and one buffer of `chunk` rows of nv reals, through
// which qM (read from global memory ONCE, its lower triangle used), actuator_moment and ten_J stream by flat coalesced loads (inv_load of mjh_inverse.h).
// qDeriv is built FIRST, in the triangle (zeroed), each entry by its own lane (lane l owns rows l, l + lanes, ..) in the order above; then qM streams in and the entry becomes
// qM - h * qDeriv -- the reference's association (it sums qDeriv before it scales by h), and deriv_smooth_vel returns exactly the matrix implicit uses.  (Tendons: the sum
// over t is formed per chunk of ten_J rows and then subtracted, the reference's `qderiv - J^T D J`; with more tendons than a chunk holds, chunk by chunk.)
// lanes, envs and chunk follow from the model alone, so a result depends neither on B nor on the environment's slot nor on how the host cut the batch.
// The model VALUES (dof_damping, tendon_damping, gainprm / biasprm / dynprm / actrange, the timestep, the disable flags) are arguments of the call, not the blob's.
#pragma once
#include "mjh_device.h"
#include "mjh_inverse.h"

#define MJH_INTEGRATE_WG 256

template <typename REAL>
struct IntegrateArgs {
  // [B, ...] leaves of a finished forward pass
  const REAL *qpos, *qvel, *act, *act_dot, *time, *ctrl, *qacc, *qM, *qfrc_smooth, *qfrc_constraint, *actuator_moment, *ten_J;
  // the caller's model values; gainprm / biasprm / dynprm are [nu, prm_stride[k]]
  const REAL *dof_damping, *tendon_damping, *gainprm, *biasprm, *dynprm, *actrange;
  // structure (the blob)
  const int *act_gaintype, *act_biastype, *act_dyntype, *act_actadr, *act_actlimited, *jnt_type, *jnt_qposadr, *jnt_dofadr;
  // outputs
  REAL *qpos_out, *qvel_out, *act_out, *time_out, *qderiv_out, *qacc_out;
  REAL h;
  int nq, nv, nu, na, njnt, ntendon;
  int gain_stride, bias_stride, dyn_stride;
  int flags;                     // MJH_INTEGRATE_*
  int actuation_on, damper_on;   // from the caller's disable flags
  int lanes, envs, chunk;        // lanes per environment, environments per workgroup, rows of nv reals per LDS chunk
  int lds_env;                   // REALs of LDS per environment (a multiple of 4)
  int64_t env_begin, env_count;
};

__device__ __forceinline__ int itg_tri(int r, int c) { return (r * (r + 1)) / 2 + c; }  // packed lower rows, c <= r

// math.small_cholesky (math.py:87-129) in place on the packed lower triangle A of an environment in LDS, by the environment's L lanes (lane l owns rows l, l + L, ..);
// v: nv reals of LDS for the scaled column.  Right-looking: column j is scaled by its pivot (clamped at 1e-12 up to INLINE_CHOL_MAX dofs, + 1e-10 above), then every
// later entry (r, c) loses L[r][j] L[c][j], i.e. the products leave an entry in j order.  Shared by mjh_integrate_kernel (qM - h qDeriv) and mjh_smooth.h's factor_m (qM).
template <typename REAL>
__device__ __forceinline__ void itg_cholesky(REAL* A, REAL* v, int nv, int l, int L) {
  const bool big = nv > INLINE_CHOL_MAX;
  for (int j = 0; j < nv; j++) {
    REAL s = A[itg_tri(j, j)];
    if (big) s = s + (REAL)1e-10;  // (A + 1e-10 I, applied at the pivot)
    else s = s > (REAL)1e-12 ? s : (REAL)1e-12;
    const REAL d = r_sqrt<REAL>(s);
    wave_sync();  // every lane has read the pivot before its owner overwrites it
    for (int r = l; r < nv; r += L) {  // (the scaled column also goes to v, a buffer of its own: the sweep below then reads no entry of A another lane writes)
      if (r > j) { const REAL q = A[itg_tri(r, j)] / d; A[itg_tri(r, j)] = q; v[r] = q; }
      else if (r == j) A[itg_tri(j, j)] = d;
    }
    wave_sync();
    for (int r = l; r < nv; r += L) {
      if (r <= j) continue;
      const REAL* __restrict__ col = v;
      REAL* __restrict__ Ar = A + itg_tri(r, 0);
      const REAL lr = col[r];
      for (int c = j + 1; c <= r; c++) Ar[c] = Ar[c] - lr * col[c];
    }
    wave_sync();
  }
}

// math.small_cholesky_solve (math.py:132-168) in place on x, nv reals of an environment in LDS, with the packed factor A that itg_cholesky left (or a caller's qLD packed
// the same way): L y = b by columns, then L^T z = y as the reference's row loop up to INLINE_CHOL_MAX dofs and by columns above.  Shared by mjh_integrate_kernel and
// mjh_dynamics.h's ACCELERATION (qacc_smooth from the caller's qLD).
template <typename REAL>
__device__ __forceinline__ void itg_chol_solve(REAL* A, REAL* x, int nv, int l, int L) {
  const bool big = nv > INLINE_CHOL_MAX;
  // L y = b, column by column: element r loses L[r][k] y[k] in k order, as the reference's row loop does
  // (every lane reads x[k] and its owner overwrites it in the same trip with no barrier between: an environment's lanes share a wavefront, which issues the read
  // for all of them before the write, and LDS operations complete in issue order.  The same holds for the column-wise backward substitution below.)
  for (int k = 0; k < nv; k++) {
    const REAL yk = x[k] / A[itg_tri(k, k)];
    for (int r = l; r < nv; r += L) {
      if (r > k) x[r] = x[r] - A[itg_tri(r, k)] * yk;
      else if (r == k) x[k] = yk;
    }
    wave_sync();
  }
  if (!big) {  // L^T z = y, the reference's row loop: k ascending inside a row, rows descending -- a serial chain, run by every lane alike
    for (int i = nv - 1; i >= 0; i--) {
      REAL s = x[i];
      for (int k = i + 1; k < nv; k++) s = s - A[itg_tri(k, i)] * x[k];
      s = s / A[itg_tri(i, i)];
      wave_sync();
      if (l == 0) x[i] = s;
      wave_sync();
    }
  } else {
    for (int k = nv - 1; k >= 0; k--) {
      const REAL zk = x[k] / A[itg_tri(k, k)];
      for (int r = l; r < nv; r += L) {
        if (r < k) x[r] = x[r] - A[itg_tri(k, r)] * zk;
        else if (r == k) x[k] = zk;
      }
      wave_sync();
    }
  }
}

template <typename REAL>
__global__ __launch_bounds__(MJH_INTEGRATE_WG) void mjh_integrate_kernel(IntegrateArgs<REAL> a) {
  extern __shared__ __attribute__((aligned(16))) double itg_lds_raw[];
  const int L = a.lanes;
  const int slot = (int)threadIdx.x / L, l = (int)threadIdx.x - slot * L;
  const int64_t e = a.env_begin + (int64_t)blockIdx.x * a.envs + slot;
  if (slot >= a.envs || e >= a.env_begin + a.env_count) return;  // (whole environments only: an environment's lanes all return or none do)
  const int nv = a.nv, nu = a.nu, nt = a.ntendon, ntri = (nv * (nv + 1)) / 2;
  REAL* A = reinterpret_cast<REAL*>(itg_lds_raw) + (int64_t)slot * a.lds_env;  // packed lower triangle: qDeriv, then A, then its factor
  REAL* x = A + ((ntri + 3) & ~3);                                            // right-hand side -> qacc
  REAL* v = x + ((nv + 3) & ~3);                                              // the new qvel
  REAL* vel = v + ((nv + 3) & ~3);                                            // vel_i of the actuators
  REAL* buf = vel + ((nu + 3) & ~3);                                          // chunk rows of qM / actuator_moment / ten_J
  const REAL h = a.h;
  const bool build = a.flags & MJH_INTEGRATE_QDERIV, implicit = (a.flags & MJH_INTEGRATE_IMPLICIT) && build, euler = !implicit && (a.flags & MJH_INTEGRATE_EULER);

  if (build) {
    for (int w = l; w < ntri; w += L) A[w] = 0;
    if (a.actuation_on) {
      for (int i = l; i < nu; i += L) {
        const REAL bias_vel = a.act_biastype[i] == BIAS_AFFINE ? a.biasprm[i * a.bias_stride + 2] : (REAL)0;
        const REAL gain_vel = a.act_gaintype[i] == GAIN_AFFINE ? a.gainprm[i * a.gain_stride + 2] : (REAL)0;
        const REAL c = a.act_dyntype[i] == DYN_NONE ? a.ctrl[e * nu + i] : a.act[e * a.na + a.act_actadr[i]];
        vel[i] = bias_vel + gain_vel * c;
      }
    }
    wave_sync();
    if (a.actuation_on) {
      const REAL* mom = a.actuator_moment + e * nu * nv;
      for (int i0 = 0; i0 < nu; i0 += a.chunk) {
        const int rows = nu - i0 < a.chunk ? nu - i0 : a.chunk;
        inv_load<REAL>(buf, mom + (int64_t)i0 * nv, rows * nv, l, L);
        wave_sync();
        for (int ii = 0; ii < rows; ii++) {
          const REAL vi = vel[i0 + ii];
          if (vi == 0) continue;  // (adds exact zeros)
          const REAL* m = buf + ii * nv;
          for (int r = l; r < nv; r += L) {
            const REAL mr = m[r];
            if (mr == 0) continue;
            REAL* Ar = A + itg_tri(r, 0);
            for (int c = 0; c <= r; c++) Ar[c] = Ar[c] + mr * (m[c] * vi);
          }
        }
        wave_sync();
      }
    }
    if (a.damper_on)
      for (int r = l; r < nv; r += L) A[itg_tri(r, r)] = A[itg_tri(r, r)] - a.dof_damping[r];
    if (nt > 0) {
      const REAL* J = a.ten_J + e * nt * nv;
      for (int t0 = 0; t0 < nt; t0 += a.chunk) {
        const int rows = nt - t0 < a.chunk ? nt - t0 : a.chunk;
        inv_load<REAL>(buf, J + (int64_t)t0 * nv, rows * nv, l, L);
        wave_sync();
        for (int r = l; r < nv; r += L) {
          bool any = false;
          for (int t = 0; t < rows; t++) any = any || buf[t * nv + r] != 0;
          if (!any) continue;
          REAL* Ar = A + itg_tri(r, 0);
          for (int c = 0; c <= r; c++) {
            REAL s = 0;
            for (int t = 0; t < rows; t++) s = s + (buf[t * nv + r] * a.tendon_damping[t0 + t]) * buf[t * nv + c];
            Ar[c] = Ar[c] - s;
          }
        }
        wave_sync();
      }
    }
    wave_sync();
    if (a.flags & MJH_INTEGRATE_WRITE_QDERIV) {  // the full symmetric matrix, flat
      REAL* out = a.qderiv_out + e * nv * nv;
      for (int w = l; w < nv * nv; w += L) {
        const int r = w / nv, c = w - r * nv;
        out[w] = c <= r ? A[itg_tri(r, c)] : A[itg_tri(c, r)];
      }
    }
  }

  if (implicit || euler) {
    // A: the lower triangle of qM streams through buf once
    const REAL* qM = a.qM + e * nv * nv;
    for (int r0 = 0; r0 < nv; r0 += a.chunk) {
      const int rows = nv - r0 < a.chunk ? nv - r0 : a.chunk;
      inv_load<REAL>(buf, qM + (int64_t)r0 * nv, rows * nv, l, L);
      wave_sync();
      for (int w = l; w < rows * nv; w += L) {
        const int rr = w / nv, c = w - rr * nv, r = r0 + rr;
        if (c > r) continue;
        const int k = itg_tri(r, c);
        if (implicit) A[k] = buf[w] - h * A[k];
        else A[k] = r == c ? buf[w] + h * a.dof_damping[r] : buf[w];
      }
      wave_sync();
    }
    for (int i = l; i < nv; i += L) x[i] = a.qfrc_smooth[e * nv + i] + a.qfrc_constraint[e * nv + i];
    wave_sync();

    itg_cholesky<REAL>(A, v, nv, l, L);
    itg_chol_solve<REAL>(A, x, nv, l, L);
  } else if (a.flags & (MJH_INTEGRATE_STATE | MJH_INTEGRATE_WRITE_QACC)) {
    for (int i = l; i < nv; i += L) x[i] = a.qacc[e * nv + i];
    wave_sync();
  }

  if (a.flags & MJH_INTEGRATE_WRITE_QACC)
    for (int i = l; i < nv; i += L) a.qacc_out[e * nv + i] = x[i];

  if (a.flags & MJH_INTEGRATE_STATE) {
    for (int i = l; i < nu; i += L) {  // one lane per actuator
      const int dyn = a.act_dyntype[i];
      if (dyn == DYN_NONE) continue;
      const int ad = a.act_actadr[i];
      REAL act = a.act[e * a.na + ad];
      const REAL ad_dot = a.act_dot[e * a.na + ad];
      if (dyn == DYN_FILTEREXACT) {
        REAL tau = a.dynprm[i * a.dyn_stride];
        tau = tau > (REAL)mjMINVAL ? tau : (REAL)mjMINVAL;
        act = act + ad_dot * tau * (1 - r_exp<REAL>(-h / tau));
      } else {
        act = act + ad_dot * h;
      }
      if (a.act_actlimited[i]) {
        const REAL lo = a.actrange[2 * i], hi = a.actrange[2 * i + 1];
        act = act < lo ? lo : (act > hi ? hi : act);
      }
      a.act_out[e * a.na + ad] = act;
    }
    for (int i = l; i < nv; i += L) {  // one lane per dof
      const REAL nvl = a.qvel[e * nv + i] + x[i] * h;
      v[i] = nvl;
      a.qvel_out[e * nv + i] = nvl;
    }
    wave_sync();
    const REAL* qpos = a.qpos + e * a.nq;
    REAL* o = a.qpos_out + e * a.nq;
    for (int j = l; j < a.njnt; j += L) {  // one lane per joint (forward.py:231-252)
      const int t = a.jnt_type[j], qa = a.jnt_qposadr[j], da = a.jnt_dofadr[j];
      if (t == JNT_FREE) {
        for (int i = 0; i < 3; i++) o[qa + i] = qpos[qa + i] + h * v[da + i];
        REAL q[4] = {qpos[qa + 3], qpos[qa + 4], qpos[qa + 5], qpos[qa + 6]}, w[3] = {v[da + 3], v[da + 4], v[da + 5]}, r[4];
        quat_integrate(q, w, h, r);
        for (int i = 0; i < 4; i++) o[qa + 3 + i] = r[i];
      } else if (t == JNT_BALL) {
        REAL q[4] = {qpos[qa], qpos[qa + 1], qpos[qa + 2], qpos[qa + 3]}, w[3] = {v[da], v[da + 1], v[da + 2]}, r[4];
        quat_integrate(q, w, h, r);
        for (int i = 0; i < 4; i++) o[qa + i] = r[i];
      } else {
        o[qa] = qpos[qa] + h * v[da];
      }
    }
    if (l == 0) a.time_out[e] = a.time[e] + h;
  }
}
