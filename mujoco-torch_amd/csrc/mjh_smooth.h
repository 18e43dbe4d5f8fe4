// mjh_smooth.h -- the smooth-dynamics stages of the reference (_src/smooth.py:210-467, 500-521, support.make_m's dense path, math.small_cholesky) as functions on
// a caller's Data: each reads the leaves it is handed AS THEY ARE (nothing is recomputed from qpos) and writes fresh ones.  Six operations (SmoothArgs.op), one kernel each.
//
// Spatial vectors are [rotational(3), translational(3)] in the world frame about subtree_com[body_rootid[b]]; bodies are in depth-first order, so the subtree of b is
// the bodies [b, body_subtree_end[b]).  "sub(x)[b]" below is the sum of x over that range LAST BODY FIRST (s = 0; s += x[end - 1]; ..; s += x[b]), the order postcon's
// cfrc_int uses; "chain(b)" is the path world -> b (body_chain, the world left out, b itself last).  Sums over k (a vector's components), over a joint's or a body's
// dofs and over tendons run in ascending index order from the first term (or from 0 where stated).
//
// COM_POS    (smooth.py:210-288)  pos = sub(xipos * body_mass), mass = sub(body_mass);  subtree_com[b] = xipos[b] where mass < mjMINVAL, else pos / max(mass, mjMINVAL).
//            off = xipos[b] - subtree_com[root(b)];  I = (ximat diag(inertia)) ximat^T + (h h^T) mass, h row i = off x (-e_i), both products summed over k ascending;
//            cinert[b] = [I00, I11, I22, I01, I02, I12, off * mass, mass].
//            cdof, per joint j of body b, o = subtree_com[root(b)] - xanchor[j]:  FREE: [0, e_0], [0, e_1], [0, e_2], then [a_k, a_k x o] for the rows a_k of xmat[b]^T
//            (the columns of xmat);  BALL: those three;  HINGE: [xaxis, xaxis x o];  SLIDE: [0, xaxis].
// CRB        (smooth.py:291-308)  crb = sub(cinert), crb[0] = 0;  f_i = inert_mul(crb[dof_bodyid[i]], cdof[i]);  qM[i][j] = qM[j][i] = sum_k f_i[k] cdof[j][k] for j = i
//            or an ancestor dof of i (body_dofmask of i's body, j <= i), 0 elsewhere;  + dof_armature[i] on the diagonal.
// TENDON_ARMATURE (smooth.py:500-521)  qM[r][c] + sum_t ten_J[t][r] * (ten_J[t][c] * tendon_armature[t]), the sum from 0.
// FACTOR_M   (smooth.py:311-319, math.py:87-129)  qLD = L, the lower triangle, zeros above the diagonal: nv <= 16 the column-by-column scalar sequence with every pivot
//            clamped at 1e-12, above cholesky(qM + 1e-10 I).  Only the lower triangle of qM is read.  The factorisation is itg_cholesky of mjh_integrate.h.
// COM_VEL    (smooth.py:385-424)  per joint part p (a joint; a free joint is two parts, its translations and its rotations) s_p = sum over the part's dofs of
//            cdof[i] * qvel[i].  cvel[b]: from 0, along chain(b), each body's parts in order: cvel += s_p.  cdof_dot of a joint's dofs = motion_cross(cvel, cdof[i]) with
//            the cvel from BEFORE that joint's parts are added -- except the free joint: its three translational rows are 0 and its rotational rows use the cvel that
//            already holds s of the translations.
// RNE        (smooth.py:427-467)  A[b] = sum over b's dofs of cdof_dot[i] * qvel[i], Q[b] = sum of cdof[i] * qacc[i] (flg_acc only; 0 for a body without dofs).
//            cacc: from [0, -gravity] (0 under DisableBit.GRAVITY), along chain(b): cacc = cacc + A[anc], then (flg_acc) cacc = cacc + Q[anc].
//            loc[b] = inert_mul(cinert[b], cacc[b]) + motion_cross_force(cvel[b], inert_mul(cinert[b], cvel[b]));  cfrc = sub(loc);
//            qfrc_bias[i] = sum_k cdof[i][k] cfrc[dof_bodyid[i]][k].
//
// The packing of mjh_postcon_kernel for the five tree operations: `lanes` (16 / 32 / 64, from nbody) lanes serve one environment, up to 256 / lanes environments share a
// workgroup, an environment's lanes lie inside one wavefront (wave barriers only).  Every leaf element is read from global memory once: a per-body or per-joint row by
// the lane that owns the body or joint, a leaf several lanes need (cdof, cinert in CRB, qvel in COM_VEL, ten_J) by one flat coalesced pass into LDS.  LDS holds only what
// crosses lanes.  Bodies, joints, dofs and matrix entries beyond the lane count take several trips.  FACTOR_M takes its lanes from nv and keeps the packed lower triangle
// of the environment's matrix and one column in LDS; several environments share a workgroup where they fit, else an environment has the workgroup -- one wavefront -- alone.
// No atomics: every sum has one fixed order, so a result depends neither on the lanes, nor on B, nor on the environment's slot, nor on how the host cut the batch.
// The model VALUES (body_mass, body_inertia, dof_armature, the tendons' armature, gravity, the GRAVITY flag) are arguments of the call, not the blob's.
#pragma once
#include "mjh_device.h"
#include "mjh_integrate.h"

#define MJH_SMOOTH_WG 256

template <typename REAL>
struct SmoothArgs {
  // [B, ...] leaves of the caller's Data
  const REAL *xipos, *ximat, *xmat, *xanchor, *xaxis, *cinert, *cdof, *cdof_dot, *cvel, *qvel, *qacc, *qM, *ten_J;
  // the caller's model values
  const REAL *body_mass, *body_inertia, *dof_armature, *tendon_armature;
  // structure (the blob)
  const int *body_rootid, *body_jntadr, *body_jntnum, *body_dofadr, *body_dofnum, *body_depth, *body_chain, *body_subtree_end, *jnt_type, *jnt_dofadr, *jnt_bodyid, *dof_bodyid;
  const unsigned long long* body_dofmask;
  // outputs
  REAL *subtree_com, *cinert_out, *cdof_out, *crb, *qM_out, *qLD, *cvel_out, *cdof_dot_out, *qfrc_bias;
  REAL cacc0[3];  // translational part of cacc[world]: -gravity, or zero under DisableBit.GRAVITY
  int nbody, njnt, nv, ntendon, max_depth, mask_words, flg_acc;
  int lanes, envs;  // lanes per environment, environments per workgroup
  int lds_env;      // REALs of LDS per environment (a multiple of 4)
  int64_t env_begin, env_count;
};

// n reals of one environment's leaf into LDS, flat: consecutive lanes read consecutive elements
template <typename REAL>
__device__ __forceinline__ void sm_load(REAL* dst, const REAL* src, int n, int l, int L) {
  for (int w = l; w < n; w += L) dst[w] = src[w];
}

// sub(x)[b] for component k of rows of `stride` reals
template <typename REAL>
__device__ __forceinline__ REAL sm_subtree(const REAL* x, int stride, int k, int b, int end) {
  REAL s = 0;
  for (int d = end - 1; d >= b; d--) s += x[stride * d + k];
  return s;
}

template <typename REAL, int OP>
__global__ __launch_bounds__(MJH_SMOOTH_WG) void mjh_smooth_kernel(SmoothArgs<REAL> a) {
  extern __shared__ __attribute__((aligned(16))) double sm_lds_raw[];
  const int L = a.lanes;
  const int slot = (int)threadIdx.x / L, l = (int)threadIdx.x - slot * L;
  const int64_t e = a.env_begin + (int64_t)blockIdx.x * a.envs + slot;
  if (slot >= a.envs || e >= a.env_begin + a.env_count) return;  // (whole environments only: an environment's lanes all return or none do)
  const int nb = a.nbody, nv = a.nv, md = a.max_depth;
  REAL* lds = reinterpret_cast<REAL*>(sm_lds_raw) + (int64_t)slot * a.lds_env;

  if constexpr (OP == MJH_SMOOTH_COM_POS) {
    REAL* xip = lds;           // 3 nb: xipos
    REAL* mp = xip + 3 * nb;   // 4 nb: xipos * mass, mass
    REAL* com = mp + 4 * nb;   // 3 nb: subtree_com
    for (int b = l; b < nb; b += L) {
      const REAL* x = a.xipos + (e * nb + b) * 3;
      const REAL mass = a.body_mass[b];
#pragma unroll
      for (int k = 0; k < 3; k++) { const REAL xk = x[k]; xip[3 * b + k] = xk; mp[4 * b + k] = xk * mass; }
      mp[4 * b + 3] = mass;
    }
    wave_sync();
    for (int b = l; b < nb; b += L) {
      const int end = a.body_subtree_end[b];
      const REAL mass = sm_subtree(mp, 4, 3, b, end);
      const REAL den = mass > (REAL)mjMINVAL ? mass : (REAL)mjMINVAL;
#pragma unroll
      for (int k = 0; k < 3; k++) {
        const REAL c = mass < (REAL)mjMINVAL ? xip[3 * b + k] : sm_subtree(mp, 4, k, b, end) / den;
        com[3 * b + k] = c;
        a.subtree_com[(e * nb + b) * 3 + k] = c;
      }
    }
    wave_sync();
    for (int b = l; b < nb; b += L) {
      const int root = a.body_rootid[b];
      const REAL* xm = a.ximat + (e * nb + b) * 9;
      REAL R[9], off[3], h[9], I[9];
#pragma unroll
      for (int i = 0; i < 9; i++) R[i] = xm[i];
#pragma unroll
      for (int k = 0; k < 3; k++) off[k] = xip[3 * b + k] - com[3 * root + k];
      const REAL mass = a.body_mass[b];
      const REAL in[3] = {a.body_inertia[3 * b], a.body_inertia[3 * b + 1], a.body_inertia[3 * b + 2]};
#pragma unroll
      for (int i = 0; i < 3; i++) {
        REAL ne[3] = {0, 0, 0};
        ne[i] = -1;
        cross3(off, ne, h + 3 * i);
      }
#pragma unroll
      for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) {
          const REAL rot = ((R[3 * i] * in[0]) * R[3 * j] + (R[3 * i + 1] * in[1]) * R[3 * j + 1]) + (R[3 * i + 2] * in[2]) * R[3 * j + 2];
          const REAL hh = (h[3 * i] * h[3 * j] + h[3 * i + 1] * h[3 * j + 1]) + h[3 * i + 2] * h[3 * j + 2];
          I[3 * i + j] = rot + hh * mass;
        }
      }
      REAL* o = a.cinert_out + (e * nb + b) * 10;
      o[0] = I[0]; o[1] = I[4]; o[2] = I[8]; o[3] = I[1]; o[4] = I[2]; o[5] = I[5];
#pragma unroll
      for (int k = 0; k < 3; k++) o[6 + k] = off[k] * mass;
      o[9] = mass;
    }
    for (int j = l; j < a.njnt; j += L) {  // one lane per joint: its dofs' rows
      const int t = a.jnt_type[j], b = a.jnt_bodyid[j], da = a.jnt_dofadr[j];
      const REAL* rc = com + 3 * a.body_rootid[b];
      REAL* o = a.cdof_out + (e * nv + da) * 6;
      if (t == JNT_SLIDE) {
        const REAL* ax = a.xaxis + (e * a.njnt + j) * 3;
#pragma unroll
        for (int k = 0; k < 3; k++) { o[k] = 0; o[3 + k] = ax[k]; }
        continue;
      }
      const REAL* an = a.xanchor + (e * a.njnt + j) * 3;
      const REAL off[3] = {rc[0] - an[0], rc[1] - an[1], rc[2] - an[2]};
      if (t == JNT_HINGE) {
        const REAL* ax = a.xaxis + (e * a.njnt + j) * 3;
        const REAL x[3] = {ax[0], ax[1], ax[2]};
        REAL c[3];
        cross3(x, off, c);
#pragma unroll
        for (int k = 0; k < 3; k++) { o[k] = x[k]; o[3 + k] = c[k]; }
        continue;
      }
      if (t == JNT_FREE) {
#pragma unroll
        for (int r = 0; r < 3; r++) {
#pragma unroll
          for (int k = 0; k < 6; k++) o[6 * r + k] = (k == 3 + r) ? (REAL)1 : (REAL)0;
        }
        o += 18;
      }
      const REAL* xm = a.xmat + (e * nb + b) * 9;
      REAL R[9];
#pragma unroll
      for (int i = 0; i < 9; i++) R[i] = xm[i];
#pragma unroll
      for (int r = 0; r < 3; r++) {
        const REAL x[3] = {R[r], R[3 + r], R[6 + r]};
        REAL c[3];
        cross3(x, off, c);
#pragma unroll
        for (int k = 0; k < 3; k++) { o[6 * r + k] = x[k]; o[6 * r + 3 + k] = c[k]; }
      }
    }
  }

  if constexpr (OP == MJH_SMOOTH_CRB) {
    REAL* ci = lds;             // 10 nb: cinert
    REAL* cr = ci + 10 * nb;    // 10 nb: crb
    REAL* cd = cr + 10 * nb;    // 6 nv: cdof
    REAL* f = cd + 6 * nv;      // 6 nv: inert_mul(crb of the dof's body, cdof)
    sm_load<REAL>(ci, a.cinert + e * nb * 10, nb * 10, l, L);
    sm_load<REAL>(cd, a.cdof + e * nv * 6, nv * 6, l, L);
    wave_sync();
    for (int w = l; w < nb * 10; w += L) {
      const int b = w / 10, k = w - 10 * b;
      const REAL s = b == 0 ? (REAL)0 : sm_subtree(ci, 10, k, b, a.body_subtree_end[b]);
      cr[w] = s;
      a.crb[e * nb * 10 + w] = s;
    }
    wave_sync();
    for (int i = l; i < nv; i += L) {
      REAL c[10], v[6], o[6];
      const int b = a.dof_bodyid[i];
#pragma unroll
      for (int k = 0; k < 10; k++) c[k] = cr[10 * b + k];
#pragma unroll
      for (int k = 0; k < 6; k++) v[k] = cd[6 * i + k];
      inert_mul(c, v, o);
#pragma unroll
      for (int k = 0; k < 6; k++) f[6 * i + k] = o[k];
    }
    wave_sync();
    REAL* out = a.qM_out + e * nv * nv;
    for (int w = l; w < nv * nv; w += L) {
      const int r = w / nv, c = w - r * nv;
      const int i = r > c ? r : c, j = r > c ? c : r;
      const unsigned long long word = a.body_dofmask[(int64_t)a.dof_bodyid[i] * a.mask_words + (j >> 6)];
      REAL s = 0;
      if ((word >> (j & 63)) & 1ull) {
        s = f[6 * i] * cd[6 * j];
#pragma unroll
        for (int k = 1; k < 6; k++) s = s + f[6 * i + k] * cd[6 * j + k];
      }
      if (r == c) s = s + a.dof_armature[r];
      out[w] = s;
    }
  }

  if constexpr (OP == MJH_SMOOTH_TENDON_ARMATURE) {
    const int nt = a.ntendon;
    REAL* J = lds;  // nt nv: ten_J
    sm_load<REAL>(J, a.ten_J + e * nt * nv, nt * nv, l, L);
    wave_sync();
    const REAL* qM = a.qM + e * nv * nv;
    REAL* out = a.qM_out + e * nv * nv;
    for (int w = l; w < nv * nv; w += L) {
      const int r = w / nv, c = w - r * nv;
      REAL s = 0;
      for (int t = 0; t < nt; t++) s = s + J[t * nv + r] * (J[t * nv + c] * a.tendon_armature[t]);
      out[w] = qM[w] + s;
    }
  }

  if constexpr (OP == MJH_SMOOTH_FACTOR_M) {
    const int ntri = (nv * (nv + 1)) / 2;
    REAL* A = lds;                      // the packed lower triangle: qM, then its factor
    REAL* v = A + ((ntri + 3) & ~3);    // nv: the scaled column
    const REAL* qM = a.qM + e * nv * nv;
    for (int w = l; w < nv * nv; w += L) {
      const int r = w / nv, c = w - r * nv;
      if (c <= r) A[itg_tri(r, c)] = qM[w];
    }
    wave_sync();
    itg_cholesky<REAL>(A, v, nv, l, L);
    REAL* out = a.qLD + e * nv * nv;
    for (int w = l; w < nv * nv; w += L) {
      const int r = w / nv, c = w - r * nv;
      out[w] = c <= r ? A[itg_tri(r, c)] : (REAL)0;
    }
  }

  if constexpr (OP == MJH_SMOOTH_COM_VEL) {
    REAL* cd = lds;            // 6 nv: cdof
    REAL* S = cd + 6 * nv;     // 6 nv: the part sums, at the part's first dof
    REAL* qv = S + 6 * nv;     // nv: qvel
    sm_load<REAL>(cd, a.cdof + e * nv * 6, nv * 6, l, L);
    sm_load<REAL>(qv, a.qvel + e * nv, nv, l, L);
    wave_sync();
    for (int j = l; j < a.njnt; j += L) {
      const int t = a.jnt_type[j], da = a.jnt_dofadr[j];
      const int parts = t == JNT_FREE ? 2 : 1, width = (t == JNT_FREE || t == JNT_BALL) ? 3 : 1;
      for (int p = 0; p < parts; p++) {
        const int i0 = da + 3 * p;
#pragma unroll
        for (int k = 0; k < 6; k++) {
          REAL s = cd[6 * i0 + k] * qv[i0];
          for (int r = 1; r < width; r++) s = s + cd[6 * (i0 + r) + k] * qv[i0 + r];
          S[6 * i0 + k] = s;
        }
      }
    }
    wave_sync();
    for (int b = l; b < nb; b += L) {
      REAL cv[6] = {0, 0, 0, 0, 0, 0};
      const int depth = a.body_depth[b];
      for (int kk = 0; kk < depth; kk++) {
        const int anc = a.body_chain[b * md + kk];
        const int j0 = a.body_jntadr[anc], nj = a.body_jntnum[anc];
        const bool own = anc == b;
        for (int jj = 0; jj < nj; jj++) {
          const int j = j0 + jj, t = a.jnt_type[j], da = a.jnt_dofadr[j];
          int i0 = da;
          if (t == JNT_FREE) {
#pragma unroll
            for (int k = 0; k < 6; k++) cv[k] = cv[k] + S[6 * da + k];
            if (own) {
              REAL* o = a.cdof_dot_out + (e * nv + da) * 6;
#pragma unroll
              for (int k = 0; k < 18; k++) o[k] = 0;
            }
            i0 = da + 3;
          }
          if (own) {
            const int width = t == JNT_HINGE || t == JNT_SLIDE ? 1 : 3;
            for (int r = 0; r < width; r++) {
              REAL v[6], o[6];
#pragma unroll
              for (int k = 0; k < 6; k++) v[k] = cd[6 * (i0 + r) + k];
              motion_cross(cv, v, o);
              REAL* out = a.cdof_dot_out + (e * nv + i0 + r) * 6;
#pragma unroll
              for (int k = 0; k < 6; k++) out[k] = o[k];
            }
          }
#pragma unroll
          for (int k = 0; k < 6; k++) cv[k] = cv[k] + S[6 * i0 + k];
        }
      }
      REAL* out = a.cvel_out + (e * nb + b) * 6;
#pragma unroll
      for (int k = 0; k < 6; k++) out[k] = cv[k];
    }
  }

  if constexpr (OP == MJH_SMOOTH_RNE) {
    REAL* cd = lds;             // 6 nv: cdof
    REAL* A = cd + 6 * nv;      // 6 nb: the body's sum of cdof_dot * qvel
    REAL* Q = A + 6 * nb;       // 6 nb: ... of cdof * qacc
    REAL* loc = Q + 6 * nb;     // 6 nb: the local force
    REAL* cf = loc + 6 * nb;    // 6 nb: cfrc
    sm_load<REAL>(cd, a.cdof + e * nv * 6, nv * 6, l, L);
    wave_sync();
    for (int b = l; b < nb; b += L) {
      const int d0 = a.body_dofadr[b], nd = b > 0 ? a.body_dofnum[b] : 0;
      REAL s[6] = {0, 0, 0, 0, 0, 0}, q[6] = {0, 0, 0, 0, 0, 0};
      for (int r = 0; r < nd; r++) {
        const int i = d0 + r;
        const REAL qv = a.qvel[e * nv + i];
        const REAL* cdd = a.cdof_dot + (e * nv + i) * 6;
#pragma unroll
        for (int k = 0; k < 6; k++) { const REAL term = cdd[k] * qv; s[k] = r == 0 ? term : s[k] + term; }
        if (a.flg_acc) {
          const REAL qa = a.qacc[e * nv + i];
#pragma unroll
          for (int k = 0; k < 6; k++) { const REAL term = cd[6 * i + k] * qa; q[k] = r == 0 ? term : q[k] + term; }
        }
      }
#pragma unroll
      for (int k = 0; k < 6; k++) { A[6 * b + k] = s[k]; Q[6 * b + k] = q[k]; }
    }
    wave_sync();
    for (int b = l; b < nb; b += L) {
      REAL ca[6] = {0, 0, 0, a.cacc0[0], a.cacc0[1], a.cacc0[2]};
      const int depth = a.body_depth[b];
      for (int kk = 0; kk < depth; kk++) {
        const int anc = a.body_chain[b * md + kk];
#pragma unroll
        for (int k = 0; k < 6; k++) ca[k] = ca[k] + A[6 * anc + k];
        if (a.flg_acc) {
#pragma unroll
          for (int k = 0; k < 6; k++) ca[k] = ca[k] + Q[6 * anc + k];
        }
      }
      const REAL* cip = a.cinert + (e * nb + b) * 10;
      const REAL* cvp = a.cvel + (e * nb + b) * 6;
      REAL ci[10], cv[6], f1[6], f2[6], f3[6];
#pragma unroll
      for (int k = 0; k < 10; k++) ci[k] = cip[k];
#pragma unroll
      for (int k = 0; k < 6; k++) cv[k] = cvp[k];
      inert_mul(ci, ca, f1);
      inert_mul(ci, cv, f2);
      motion_cross_force(cv, f2, f3);
#pragma unroll
      for (int k = 0; k < 6; k++) loc[6 * b + k] = f1[k] + f3[k];
    }
    wave_sync();
    for (int w = l; w < nb * 6; w += L) {
      const int b = w / 6, k = w - 6 * b;
      cf[w] = sm_subtree(loc, 6, k, b, a.body_subtree_end[b]);
    }
    wave_sync();
    for (int i = l; i < nv; i += L) {
      const int b = a.dof_bodyid[i];
      REAL s = cd[6 * i] * cf[6 * b];
#pragma unroll
      for (int k = 1; k < 6; k++) s = s + cd[6 * i + k] * cf[6 * b + k];
      a.qfrc_bias[e * nv + i] = s;
    }
  }
}
