// mjh_jacobian.h -- the kernels behind mjh_jacobian: the rest of MuJoCo's Jacobian block on a finished forward pass (mj_jacBody .. mj_jacGeom with a vector,
// mj_jacDot, mj_jacSubtreeCom, mj_angmomMat; the reference has jac alone).  Dense models only.  Matrices are (nv, 3) per query, as the reference's jac returns them.
//
// Per environment, c(b) = subtree_com[body_rootid[b]], (w_i, v_i) = cdof[i], mask(b, i) = dof i sits on b or an ancestor of b (body_dofmask), subtree(body) = the
// bodies [body, body_subtree_end[body]) (bodies are in DFS order), J_b(x)[i] = v_i + w_i x (x - c(b)) where mask(b, i), else 0:
//   POINT        jacp[i] = J_body(point)[i], jacr[i] = w_i mask(body, i): mjh_support's jac, operation by operation
//   DOT          jacr_dot[i] = wd_i mask, jacp_dot[i] = ((vd_i + wd_i x (point - c)) + w_i x pdot) mask, pdot = U + W x (point - c), (W, U) = cvel[body];
//                (wd_i, vd_i) = cdof_dot[i] for slide and hinge dofs and a free joint's translations.  The dofs of a ball joint and a free joint's rotations:
//                wd_i = Wb x w_i, vd_i = Wb x v_i + Ub x w_i with (Wb, Ub) = cvel[dof_bodyid[i]]: the stored cdof_dot of those is formed with the velocity in
//                front of the joint (smooth.py:400-407), the column's derivative needs the body's own (MuJoCo's mj_jacDot)
//   SUBTREE_COM  out[i] = (sum_{b in subtree(body)} body_mass[b] J_b(xipos[b])[i]) / body_subtreemass[body], bodies in ascending order
//   ANGMOM       out[i] = sum_{b in subtree(body)} (R_b (body_inertia[b] * (R_b^T w_i)) mask(b, i) + body_mass[b] (xipos[b] - C) x (J_b(xipos[b])[i] - SUBTREE_COM[i])),
//                R_b = ximat[b], C = subtree_com[body], bodies in ascending order
// SUBTREE_COM and ANGMOM evaluate their sums.  The closed forms through subtree_com / body_subtreemass / crb read no body_mass at all, so a caller's value-only edit
// (mx.replace(body_mass=...), taken from the call's arguments like mjh_energy's) would not reach them; a sum costs nbody short steps per element on models of tens of bodies.
//
// Two forms.  mjh_jac_matrix_kernel: one lane per output element (env, query, dof, k), environment-major, 256 lanes per workgroup, so consecutive lanes store
//   consecutive addresses (the shape of mjh_sup_point_kernel); a lane forms its dof's 3-vector in registers and stores component k.  The kernel is bound by its
//   stores (6 nv or 3 nv reals per query against 6 or 12 nv + a few bodies read, all of it L1 / L2 hits after the first lane of the environment).
// mjh_jac_product_kernel (vec given): out = sum_i column[i] vec[i], the matrix never written.  16 lanes serve one environment, up to 16 environments share a
//   256-lane workgroup, an environment's lanes lie inside one wavefront (wave barriers only).  The rows every query re-reads -- cdof, cdof_dot (DOT), vec -- are
//   staged in LDS once per environment by flat coalesced loads and serve all P queries.  Query by query, lane l forms the columns of dofs l, l + 16, ... (the
//   costly part: a subtree operation walks the bodies for every dof) and leaves column[i] * vec[i] in LDS; then lane k < 3 (6 for POINT / DOT) sums component k
//   over the dofs in ascending order from 0: no atomics, no tree, so a result depends on nothing but its environment.  16 lanes: the dofs of these models are a
//   few tens, 64 lanes per environment would leave most of a wavefront idle in the column pass, one lane per query (P is often 1) nearly all of it; 16
//   environments per workgroup keep the stage loads wide.  LDS per environment: 13 nv reals (19 nv for DOT), rounded to multiples of 4 reals (16-byte carve
//   offsets); the workgroup's share is held to 48 KB (three workgroups per CU of 160 KB) by halving the environments per workgroup -- humanoid float64: 2.8 KB an
//   environment (DOT 4.1 KB), 16 (8) fit; 72 dofs: 7.5 KB (10.9 KB), 4 fit.  Both LDS passes are linear in the lane (stride 6 reals between lanes in the column
//   pass, stride 1 in the sum): no bank conflicts worth a padding.
// Neither form uses scratch (3-vectors are selected with ?:, never indexed at run time) and neither depends on how the host cut or sliced the batch.
#pragma once
#include "mjh_device.h"

#define MJH_JAC_WG 256
#define MJH_JAC_LANES 16

template <typename REAL>
struct JacArgs {
  const REAL *cdof, *cdof_dot, *cvel, *subtree_com, *xipos, *ximat;  // [B, ...] leaves
  const REAL *body_mass, *body_subtreemass, *body_inertia;           // the caller's model values
  const REAL *point, *vec;
  const int* body;                                                   // query body ids (body_stride 1), or one id (0)
  const unsigned long long* body_dofmask;                            // model: nbody * mask_words
  const int *body_rootid, *body_subtree_end, *dof_bodyid, *dof_jntid, *jnt_type, *jnt_dofadr;
  REAL *out0, *out1;
  int64_t point_env, point_q;
  int64_t env_base;   // first environment of this launch
  int64_t env_count;  // (product form) environments of this launch
  int r_base;         // (matrix form) element of env_base the launch starts at
  int count;          // (matrix form) elements of this launch
  int op, body_stride, nv, nbody, mask_words, P;
  int envs, lds_env;  // (product form) environments per workgroup, REALs of LDS per environment (a multiple of 4)
};

template <typename REAL>
__device__ __forceinline__ bool jac_on(const JacArgs<REAL>& a, int body, int dof) {
  return (a.body_dofmask[(int64_t)body * a.mask_words + (dof >> 6)] >> (dof & 63)) & 1ull;
}

// v + w x (x - c(b)) of one dof: cd = its cdof row
template <typename REAL>
__device__ __forceinline__ void jac_lin(const JacArgs<REAL>& a, int64_t e, const REAL* cd, const REAL* x, int b, REAL* o) {
  const REAL* rc = a.subtree_com + (e * a.nbody + a.body_rootid[b]) * 3;
  const REAL off[3] = {x[0] - rc[0], x[1] - rc[1], x[2] - rc[2]};
  REAL c[3];
  cross3(cd, off, c);
  o[0] = cd[3] + c[0]; o[1] = cd[4] + c[1]; o[2] = cd[5] + c[2];
}

// SUBTREE_COM's 3-vector of one dof
template <typename REAL>
__device__ __forceinline__ void jac_subtree(const JacArgs<REAL>& a, int64_t e, const REAL* cd, int body, int dof, REAL* o) {
  REAL s0 = 0, s1 = 0, s2 = 0;
  const int end = a.body_subtree_end[body];
  for (int b = body; b < end; b++) {
    if (!jac_on(a, b, dof)) continue;
    REAL j[3];
    jac_lin(a, e, cd, a.xipos + (e * a.nbody + b) * 3, b, j);
    const REAL m = a.body_mass[b];
    s0 = s0 + m * j[0]; s1 = s1 + m * j[1]; s2 = s2 + m * j[2];
  }
  const REAL M = a.body_subtreemass[body];
  o[0] = s0 / M; o[1] = s1 / M; o[2] = s2 / M;
}

// the column(s) of one dof: o0 (jacp, jacp_dot, the subtree matrices' row), o1 (jacr, jacr_dot; POINT and DOT only).  cd / cdd: the dof's cdof / cdof_dot rows.
template <typename REAL>
__device__ __forceinline__ void jac_column(const JacArgs<REAL>& a, int64_t e, int p, int dof, const REAL* cd, const REAL* cdd, REAL* o0, REAL* o1) {
  const int body = a.body[p * a.body_stride];
  o0[0] = o0[1] = o0[2] = 0;
  o1[0] = o1[1] = o1[2] = 0;
  if (a.op == MJH_JACOBIAN_POINT || a.op == MJH_JACOBIAN_DOT) {
    if (!jac_on(a, body, dof)) return;
    const REAL* pt = a.point + e * a.point_env + p * a.point_q;
    if (a.op == MJH_JACOBIAN_POINT) {
      jac_lin(a, e, cd, pt, body, o0);
      o1[0] = cd[0]; o1[1] = cd[1]; o1[2] = cd[2];
      return;
    }
    const REAL* rc = a.subtree_com + (e * a.nbody + a.body_rootid[body]) * 3;
    const REAL off[3] = {pt[0] - rc[0], pt[1] - rc[1], pt[2] - rc[2]};
    const REAL* V = a.cvel + (e * a.nbody + body) * 6;
    REAL t[3], pd[3];
    cross3(V, off, t);
    pd[0] = V[3] + t[0]; pd[1] = V[4] + t[1]; pd[2] = V[5] + t[2];
    REAL wd[3], vd[3];
    const int j = a.dof_jntid[dof], jt = a.jnt_type[j];
    if (jt == JNT_BALL || (jt == JNT_FREE && dof - a.jnt_dofadr[j] >= 3)) {
      const REAL* Vb = a.cvel + (e * a.nbody + a.dof_bodyid[dof]) * 6;
      REAL u[3];
      cross3(Vb, cd, wd);
      cross3(Vb, cd + 3, vd);
      cross3(Vb + 3, cd, u);
      vd[0] = vd[0] + u[0]; vd[1] = vd[1] + u[1]; vd[2] = vd[2] + u[2];
    } else {
      wd[0] = cdd[0]; wd[1] = cdd[1]; wd[2] = cdd[2];
      vd[0] = cdd[3]; vd[1] = cdd[4]; vd[2] = cdd[5];
    }
    REAL c1[3], c2[3];
    cross3(wd, off, c1);
    cross3(cd, pd, c2);
    o0[0] = (vd[0] + c1[0]) + c2[0]; o0[1] = (vd[1] + c1[1]) + c2[1]; o0[2] = (vd[2] + c1[2]) + c2[2];
    o1[0] = wd[0]; o1[1] = wd[1]; o1[2] = wd[2];
    return;
  }
  REAL sc[3];
  jac_subtree(a, e, cd, body, dof, sc);
  if (a.op == MJH_JACOBIAN_SUBTREE_COM) {
    o0[0] = sc[0]; o0[1] = sc[1]; o0[2] = sc[2];
    return;
  }
  const REAL* C = a.subtree_com + (e * a.nbody + body) * 3;
  const int end = a.body_subtree_end[body];
  REAL s0 = 0, s1 = 0, s2 = 0;
  for (int b = body; b < end; b++) {
    const REAL* x = a.xipos + (e * a.nbody + b) * 3;
    const REAL d[3] = {x[0] - C[0], x[1] - C[1], x[2] - C[2]};
    const bool on = jac_on(a, b, dof);
    REAL j[3] = {0, 0, 0};
    if (on) jac_lin(a, e, cd, x, b, j);
    const REAL w[3] = {j[0] - sc[0], j[1] - sc[1], j[2] - sc[2]};
    REAL c[3];
    cross3(d, w, c);
    const REAL m = a.body_mass[b];
    REAL t0 = m * c[0], t1 = m * c[1], t2 = m * c[2];
    if (on) {
      const REAL* R = a.ximat + (e * a.nbody + b) * 9;
      const REAL* I = a.body_inertia + b * 3;
      const REAL l0 = I[0] * ((R[0] * cd[0] + R[3] * cd[1]) + R[6] * cd[2]);  // inertia * (R^T w)
      const REAL l1 = I[1] * ((R[1] * cd[0] + R[4] * cd[1]) + R[7] * cd[2]);
      const REAL l2 = I[2] * ((R[2] * cd[0] + R[5] * cd[1]) + R[8] * cd[2]);
      t0 = ((R[0] * l0 + R[1] * l1) + R[2] * l2) + t0;
      t1 = ((R[3] * l0 + R[4] * l1) + R[5] * l2) + t1;
      t2 = ((R[6] * l0 + R[7] * l1) + R[8] * l2) + t2;
    }
    s0 = s0 + t0; s1 = s1 + t1; s2 = s2 + t2;
  }
  o0[0] = s0; o0[1] = s1; o0[2] = s2;
}

template <typename REAL>
__global__ __launch_bounds__(MJH_JAC_WG) void mjh_jac_matrix_kernel(JacArgs<REAL> a) {
  const unsigned l = blockIdx.x * MJH_JAC_WG + threadIdx.x;
  if (l >= (unsigned)a.count) return;
  const unsigned per_q = 3u * a.nv, per_env = per_q * a.P;
  const unsigned lr = (unsigned)a.r_base + l;
  const unsigned er = lr / per_env, r = lr - er * per_env;
  const unsigned p = r / per_q, rq = r - p * per_q;
  const unsigned dof = rq / 3, k = rq - dof * 3;
  const int64_t e = a.env_base + er;
  const REAL* cd = a.cdof + (e * a.nv + dof) * 6;
  const REAL* cdd = a.op == MJH_JACOBIAN_DOT ? a.cdof_dot + (e * a.nv + dof) * 6 : cd;
  REAL o0[3], o1[3];
  jac_column(a, e, (int)p, (int)dof, cd, cdd, o0, o1);
  const int64_t o = (e * a.P + p) * per_q + rq;
  a.out0[o] = k == 0 ? o0[0] : (k == 1 ? o0[1] : o0[2]);
  if (a.op == MJH_JACOBIAN_POINT || a.op == MJH_JACOBIAN_DOT) a.out1[o] = k == 0 ? o1[0] : (k == 1 ? o1[1] : o1[2]);
}

template <typename REAL>
__global__ __launch_bounds__(MJH_JAC_WG) void mjh_jac_product_kernel(JacArgs<REAL> a) {
  extern __shared__ __attribute__((aligned(16))) double jac_lds_raw[];
  constexpr int L = MJH_JAC_LANES;
  const int slot = (int)threadIdx.x / L, l = (int)threadIdx.x - slot * L;
  const int64_t er = (int64_t)blockIdx.x * a.envs + slot;
  if (slot >= a.envs || er >= a.env_count) return;  // (whole environments only: an environment's lanes all return or none do)
  const int64_t e = a.env_base + er;
  const int nv = a.nv, n6 = 6 * nv;
  const bool dot = a.op == MJH_JACOBIAN_DOT;
  REAL* cd = reinterpret_cast<REAL*>(jac_lds_raw) + (int64_t)slot * a.lds_env;  // cdof (6 nv, rounded up to a multiple of 4)
  REAL* x = cd + ((n6 + 3) & ~3);                                                // vec (nv, rounded likewise)
  REAL* term = x + ((nv + 3) & ~3);                                              // the dofs' terms of the query at hand (6 nv, rounded likewise)
  REAL* cdd = term + ((n6 + 3) & ~3);                                            // cdof_dot (DOT)
  const REAL* g = a.cdof + e * n6;
  for (int t = l; t < n6; t += L) cd[t] = g[t];
  g = a.vec + e * nv;
  for (int t = l; t < nv; t += L) x[t] = g[t];
  if (dot) {
    g = a.cdof_dot + e * n6;
    for (int t = l; t < n6; t += L) cdd[t] = g[t];
  }
  wave_sync();
  // a query at a time: the lanes form the columns of dofs l, l + 16, ... and leave column[i] * vec[i] in LDS; then lane k sums component k over the dofs in
  // ascending order (components 3..5: the rotational part of POINT / DOT)
  const int nout = (dot || a.op == MJH_JACOBIAN_POINT) ? 6 : 3;
  for (int p = 0; p < a.P; p++) {
    for (int i = l; i < nv; i += L) {
      REAL o0[3], o1[3];
      jac_column(a, e, p, i, cd + 6 * i, dot ? cdd + 6 * i : cd + 6 * i, o0, o1);
      const REAL xi = x[i];
      REAL* t = term + 6 * i;
      t[0] = o0[0] * xi; t[1] = o0[1] * xi; t[2] = o0[2] * xi;
      t[3] = o1[0] * xi; t[4] = o1[1] * xi; t[5] = o1[2] * xi;
    }
    wave_sync();
    if (l < nout) {
      REAL s = 0;
      for (int i = 0; i < nv; i++) s = s + term[6 * i + l];
      if (l < 3) a.out0[(e * a.P + p) * 3 + l] = s;
      else a.out1[(e * a.P + p) * 3 + (l - 3)] = s;
    }
    wave_sync();
  }
}
