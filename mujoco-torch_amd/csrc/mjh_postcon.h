// mjh_postcon.h -- the body accelerations and forces behind a finished forward pass: MuJoCo's mj_rnePostConstraint and mj_subtreeVel (MJX: smooth.rne_postconstraint /
// smooth.subtree_vel).  The reference has neither, so the Data leaves cacc, cfrc_int, cfrc_ext, subtree_linvel and subtree_angmom stay what the caller put there; this
// kernel is what writes them.
//
// Spatial vectors are [rotational(3), translational(3)] in the world frame about subtree_com[body_rootid[b]] (the convention of cvel / cdof / cinert); xfrc_applied[b] is
// [force(3), torque(3)] at xipos[b].  move(w, from, to) of a wrench [t, f]: t' = t - (to - from) x f, f' = f.
//   cfrc_ext[0] = 0;  cfrc_ext[b] = move([xfrc[3:6], xfrc[0:3]], xipos[b], com[root(b)]);  per contact slot c in slot order (geom ids >= 0): w = the contact-frame wrench
//     from efc_force at contact.efc_address[c] (elliptic cone or dim 1: the dim rows; pyramidal: w[0] = the sum of the 2 (dim - 1) rows, w[k] = (p[2 (k - 1)] -
//     p[2 (k - 1) + 1]) * friction[k - 1]), rotated to the world by contact.frame^T, W = [torque, force] at contact.pos:  cfrc_ext[b1] -= move(W, pos, com[root(b1)]) when
//     b1 != 0, cfrc_ext[b2] += move(W, pos, com[root(b2)]) when b2 != 0.  Equality (connect / weld), limit and frictionloss forces are NOT added: they stay joint-space.
//   cacc[0] = [0, 0, 0, -gravity] (zero under DisableBit.GRAVITY);  cacc[b] = cacc[parent] + sum over b's dofs, in order, of (cdof_dot[i] qvel[i] + cdof[i] qacc[i])
//   local[b] = (cinert[b] cacc[b] + cvel[b] x* (cinert[b] cvel[b])) - cfrc_ext[b];  cfrc_int[b] = the sum of local over b's subtree (last body first, as the rne stage sums)
//   v[b] = cvel[b][3:6] - (xipos[b] - com[root(b)]) x cvel[b][0:3];  subtree_linvel[b] = (sum of mass v over b's subtree, last body first) / max(mjMINVAL, subtreemass[b])
//   subtree_angmom: L[b] = ximat (inertia o (ximat^T omega)); bodies from last to first: L[b] += (xipos[b] - com[b]) x (mass[b] (v[b] - linvel[b])), then for b >= 1
//     L[parent] += L[b] + (com[b] - com[parent]) x (subtreemass[b] (linvel[b] - linvel[parent])).
//   sensors (flag bit 4): the slots of accelerometer, force, torque, subtreelinvel and subtreeangmom sensors from the fresh leaves, with sensor_value's arithmetic
//     (mjh_sensor.h) and its cutoff; every other slot is copied from the input sensordata.
//
// A streaming kernel in the packing of mjh_inverse_kernel: `lanes` (16 / 32 / 64, from nbody) lanes serve one environment, up to 256 / lanes environments share a
// workgroup, an environment's lanes lie inside one wavefront (wave barriers only).  Every leaf element is read from global memory once, by the lane that owns its body,
// dof, contact or sensor slot; LDS holds what crosses lanes: the contacts' moved wrenches, the per-body sums and the results the later stages (and the sensors) read.
// One lane per contact forms its two moved wrenches once; one lane per body gathers cfrc_ext scanning the slots in slot order against the runtime contact_geom leaf
// (max_contact_points models choose the slots at run time).  cacc[b] is the sum along b's ancestor chain from the world down -- the additions of the recursion, in its order.
// No atomics: every sum has one fixed order, so the results do not depend on lanes, packing or how the host cut the batch.  Bodies, contacts and slots beyond the lane
// count take several trips.
#pragma once
#include "mjh_device.h"

#define MJH_POSTCON_WG 256

template <typename REAL>
struct PostconArgs {
  // [B, ...] leaves of a finished forward pass
  const REAL *qvel, *qacc, *cdof, *cdof_dot, *cvel, *cinert, *xipos, *ximat, *subtree_com, *xfrc, *efc_force;
  const REAL *contact_pos, *contact_frame, *contact_friction;
  const int* contact_dim;
  const int64_t *contact_geom, *contact_efc_address;
  const REAL *site_xpos, *site_xmat, *sensordata_in;
  // model tables (the blob) and the caller's body_subtreemass
  const int *body_parentid, *body_rootid, *body_dofadr, *body_dofnum, *body_depth, *body_chain, *body_subtree_end, *geom_bodyid;
  const int *sns_type, *sns_adr, *sns_objid, *sns_bodyid, *sns_rootid, *sns_datatype, *slot_sensor;
  const REAL *body_mass, *body_inertia, *body_subtreemass, *sns_cutoff;
  // outputs
  REAL *cacc, *cfrc_int, *cfrc_ext, *subtree_linvel, *subtree_angmom, *sensordata;
  REAL cacc0[3];  // translational part of cacc[0]: -gravity, or zero under DisableBit.GRAVITY
  int nbody, nv, ncon, nefc, ngeom, nsite, nsensordata, max_depth;
  int pyramidal;  // opt.cone
  int flags;      // MJH_POSTCON_*
  int lanes, envs;  // lanes per environment, environments per workgroup
  int lds_env;      // REALs of LDS per environment
  int64_t env_begin, env_count;
};

// t' = t - (to - from) x f
template <typename REAL>
__device__ __forceinline__ void pc_move(const REAL* t, const REAL* f, const REAL* from, const REAL* to, REAL* o) {
  const REAL d[3] = {to[0] - from[0], to[1] - from[1], to[2] - from[2]};
  REAL c[3];
  cross3(d, f, c);
#pragma unroll
  for (int i = 0; i < 3; i++) { o[i] = t[i] - c[i]; o[3 + i] = f[i]; }
}

#define PC_ROT_T(R_, v, o) for (int i_ = 0; i_ < 3; i_++) (o)[i_] = (R_)[i_] * (v)[0] + (R_)[3 + i_] * (v)[1] + (R_)[6 + i_] * (v)[2];

// the value of slot component `comp` of sensor s (accelerometer 1, force 4, torque 5, subtreelinvel 36, subtreeangmom 37) from the environment's fresh leaves in LDS:
// sensor_value's arithmetic (mjh_sensor.h), operation by operation
template <typename REAL>
__device__ __forceinline__ REAL pc_sensor(const PostconArgs<REAL>& a, int64_t e, int type, int s, int comp, const REAL* cacc_l, const REAL* cint_l, const REAL* lin_l,
                                          const REAL* am_l) {
  const int obj = a.sns_objid[s], body = a.sns_bodyid[s], root = a.sns_rootid[s];
  if (type == 36) return lin_l[3 * obj + comp];
  if (type == 37) return am_l[3 * obj + comp];
  const REAL* rot = a.site_xmat + (e * a.nsite + obj) * 9;
  const REAL* posp = a.site_xpos + (e * a.nsite + obj) * 3;
  const REAL pos[3] = {posp[0], posp[1], posp[2]};
  REAL R[9];
#pragma unroll
  for (int i = 0; i < 9; i++) R[i] = rot[i];
  const REAL* sc = a.subtree_com + (e * a.nbody + root) * 3;
  const REAL dif[3] = {pos[0] - sc[0], pos[1] - sc[1], pos[2] - sc[2]};
  if (type == 4 || type == 5) {
    REAL cf[6], o[3];
#pragma unroll
    for (int i = 0; i < 6; i++) cf[i] = cint_l[6 * body + i];
    if (type == 4) { PC_ROT_T(R, cf + 3, o) return o[comp]; }
    REAL c[3], v[3];
    cross3(dif, cf + 3, c);
#pragma unroll
    for (int i = 0; i < 3; i++) v[i] = cf[i] - c[i];
    PC_ROT_T(R, v, o)
    return o[comp];
  }
  const REAL* cv = a.cvel + (e * a.nbody + body) * 6;
  const REAL cvel[6] = {cv[0], cv[1], cv[2], cv[3], cv[4], cv[5]};
  REAL c[3], v[3], lin[3];
  cross3(dif, cvel, c);
#pragma unroll
  for (int i = 0; i < 3; i++) v[i] = cvel[3 + i] - c[i];
  PC_ROT_T(R, v, lin)
  REAL ang[3], ca[3], av[3], acc[3], corr[3], cacc[6];
#pragma unroll
  for (int i = 0; i < 6; i++) cacc[i] = cacc_l[6 * body + i];
  PC_ROT_T(R, cvel, ang)
  cross3(dif, cacc, ca);
#pragma unroll
  for (int i = 0; i < 3; i++) av[i] = cacc[3 + i] - ca[i];
  PC_ROT_T(R, av, acc)
  cross3(ang, lin, corr);
  return (acc[comp] + corr[comp]) + 0;
}

template <typename REAL>
__global__ __launch_bounds__(MJH_POSTCON_WG) void mjh_postcon_kernel(PostconArgs<REAL> a) {
  extern __shared__ double pc_lds_raw[];
  const int L = a.lanes;
  const int slot = (int)threadIdx.x / L, l = (int)threadIdx.x - slot * L;
  const int64_t e = a.env_begin + (int64_t)blockIdx.x * a.envs + slot;
  if (slot >= a.envs || e >= a.env_begin + a.env_count) return;  // (whole environments only: an environment's lanes all return or none do)
  const int nb = a.nbody, nv = a.nv, ncon = a.ncon, md = a.max_depth;
  REAL* ext = reinterpret_cast<REAL*>(pc_lds_raw) + (int64_t)slot * a.lds_env;  // 6 nb: cfrc_ext, then (same lane) the local force
  REAL* acc_l = ext + 6 * nb;    // 6 nb: cacc
  REAL* int_l = acc_l + 6 * nb;  // 6 nb: the per-body dof sums, then cfrc_int
  REAL* lin_l = int_l + 6 * nb;  // 3 nb: subtree_linvel
  REAL* am_l = lin_l + 3 * nb;   // 3 nb: subtree_angmom
  REAL* v_l = am_l + 3 * nb;     // 3 nb: com velocity of the body
  REAL* mv_l = v_l + 3 * nb;     // 3 nb: mass * v, then what the body hands to its parent's angular momentum
  REAL* cw = mv_l + 3 * nb;      // 12 ncon: the contact wrench moved to root(b1), to root(b2)
  REAL* cb = cw + 12 * ncon;     // 2 ncon: b1, b2 (as reals; -1: the slot is skipped)
  const REAL* com = a.subtree_com + e * nb * 3;
  const REAL* xip = a.xipos + e * nb * 3;
  const REAL* cvl = a.cvel + e * nb * 6;

  if (a.flags & MJH_POSTCON_RNE) {
    // one lane per contact: the world wrench, moved to the two bodies' reference points
    for (int c = l; c < ncon; c += L) {
      const int64_t g1 = a.contact_geom[(e * ncon + c) * 2], g2 = a.contact_geom[(e * ncon + c) * 2 + 1];
      const int dim = a.contact_dim[e * ncon + c];
      const int64_t adr = a.contact_efc_address[e * ncon + c];
      const bool pyr = a.pyramidal && dim > 1;
      const int rows = pyr ? 2 * (dim - 1) : dim;
      const bool ok = g1 >= 0 && g2 >= 0 && g1 < a.ngeom && g2 < a.ngeom && dim >= 1 && dim <= 6 && adr >= 0 && adr + rows <= a.nefc;
      REAL m1[6] = {0, 0, 0, 0, 0, 0}, m2[6] = {0, 0, 0, 0, 0, 0};
      int b1 = -1, b2 = -1;
      if (ok) {
        b1 = a.geom_bodyid[g1]; b2 = a.geom_bodyid[g2];
        const REAL* p = a.efc_force + e * a.nefc + adr;
        REAL w[6] = {0, 0, 0, 0, 0, 0};
        if (!pyr) {
          for (int k = 0; k < dim; k++) w[k] = p[k];
        } else {
          const REAL* fr = a.contact_friction + (e * ncon + c) * 5;
          REAL s = p[0];
          for (int k = 1; k < rows; k++) s = s + p[k];
          w[0] = s;
          for (int k = 1; k < dim; k++) w[k] = (p[2 * (k - 1)] - p[2 * (k - 1) + 1]) * fr[k - 1];
        }
        const REAL* fp = a.contact_frame + (e * ncon + c) * 9;
        REAL F[9], force[3], torque[3];
#pragma unroll
        for (int i = 0; i < 9; i++) F[i] = fp[i];
        PC_ROT_T(F, w, force)
        PC_ROT_T(F, w + 3, torque)
        const REAL* pp = a.contact_pos + (e * ncon + c) * 3;
        const REAL pos[3] = {pp[0], pp[1], pp[2]};
        pc_move(torque, force, pos, com + 3 * a.body_rootid[b1], m1);
        pc_move(torque, force, pos, com + 3 * a.body_rootid[b2], m2);
      }
#pragma unroll
      for (int k = 0; k < 6; k++) { cw[12 * c + k] = m1[k]; cw[12 * c + 6 + k] = m2[k]; }
      cb[2 * c] = (REAL)b1; cb[2 * c + 1] = (REAL)b2;
    }
    wave_sync();
    // one lane per body: cfrc_ext (xfrc_applied, then the contact slots in slot order) and the body's dof sum
    for (int b = l; b < nb; b += L) {
      REAL x[6] = {0, 0, 0, 0, 0, 0};
      if (b > 0) {
        const REAL* xf = a.xfrc + (e * nb + b) * 6;
        const REAL f[3] = {xf[0], xf[1], xf[2]}, t[3] = {xf[3], xf[4], xf[5]};
        pc_move(t, f, xip + 3 * b, com + 3 * a.body_rootid[b], x);
        for (int c = 0; c < ncon; c++) {
          const int b1 = (int)cb[2 * c], b2 = (int)cb[2 * c + 1];
          if (b1 == b) {
#pragma unroll
            for (int k = 0; k < 6; k++) x[k] = x[k] - cw[12 * c + k];
          }
          if (b2 == b) {
#pragma unroll
            for (int k = 0; k < 6; k++) x[k] = x[k] + cw[12 * c + 6 + k];
          }
        }
      }
      const int d0 = a.body_dofadr[b], nd = b > 0 ? a.body_dofnum[b] : 0;
      REAL vm[6] = {0, 0, 0, 0, 0, 0};
      for (int r = 0; r < nd; r++) {
        const int i = d0 + r;
        const REAL qv = a.qvel[e * nv + i], qa = a.qacc[e * nv + i];
        const REAL *cdd = a.cdof_dot + (e * nv + i) * 6, *cd = a.cdof + (e * nv + i) * 6;
#pragma unroll
        for (int k = 0; k < 6; k++) {
          const REAL term = cdd[k] * qv + cd[k] * qa;
          vm[k] = r == 0 ? term : vm[k] + term;
        }
      }
#pragma unroll
      for (int k = 0; k < 6; k++) { ext[6 * b + k] = x[k]; int_l[6 * b + k] = vm[k]; a.cfrc_ext[(e * nb + b) * 6 + k] = x[k]; }
    }
    wave_sync();
    // cacc along the ancestor chain from the world down, then the local force
    for (int b = l; b < nb; b += L) {
      REAL ca[6] = {0, 0, 0, a.cacc0[0], a.cacc0[1], a.cacc0[2]};
      const int depth = a.body_depth[b];
      for (int kk = 0; kk < depth; kk++) {
        const int anc = a.body_chain[b * md + kk];
        if (a.body_dofnum[anc] > 0) {
#pragma unroll
          for (int k = 0; k < 6; k++) ca[k] = ca[k] + int_l[6 * anc + k];
        }
      }
      const REAL* cip = a.cinert + (e * nb + b) * 10;
      REAL ci[10], cv[6], f1[6], f2[6], f3[6];
#pragma unroll
      for (int k = 0; k < 10; k++) ci[k] = cip[k];
#pragma unroll
      for (int k = 0; k < 6; k++) cv[k] = cvl[6 * b + k];
      inert_mul(ci, ca, f1);
      inert_mul(ci, cv, f2);
      motion_cross_force(cv, f2, f3);
#pragma unroll
      for (int k = 0; k < 6; k++) {
        acc_l[6 * b + k] = ca[k];
        a.cacc[(e * nb + b) * 6 + k] = ca[k];
        ext[6 * b + k] = (f1[k] + f3[k]) - ext[6 * b + k];
      }
    }
    wave_sync();
    // subtree sums of the local forces
    for (int w = l; w < nb * 6; w += L) {
      const int b = w / 6, k = w - 6 * b;
      const int end = a.body_subtree_end[b];
      REAL s = 0;
      for (int d = end - 1; d >= b; d--) s += ext[6 * d + k];
      int_l[w] = s;
      a.cfrc_int[e * nb * 6 + w] = s;
    }
    wave_sync();
  }

  if (a.flags & MJH_POSTCON_SUBTREE) {
    for (int b = l; b < nb; b += L) {
      const REAL om[3] = {cvl[6 * b], cvl[6 * b + 1], cvl[6 * b + 2]};
      const REAL* rc = com + 3 * a.body_rootid[b];
      const REAL r[3] = {xip[3 * b] - rc[0], xip[3 * b + 1] - rc[1], xip[3 * b + 2] - rc[2]};
      REAL c[3];
      cross3(r, om, c);
      const REAL mass = a.body_mass[b];
      const REAL* xm = a.ximat + (e * nb + b) * 9;
      REAL R[9], loc[3], wl[3];
#pragma unroll
      for (int i = 0; i < 9; i++) R[i] = xm[i];
      PC_ROT_T(R, om, loc)  // ximat^T omega
#pragma unroll
      for (int i = 0; i < 3; i++) loc[i] = a.body_inertia[3 * b + i] * loc[i];
#pragma unroll
      for (int i = 0; i < 3; i++) wl[i] = R[3 * i] * loc[0] + R[3 * i + 1] * loc[1] + R[3 * i + 2] * loc[2];
#pragma unroll
      for (int i = 0; i < 3; i++) {
        const REAL v = cvl[6 * b + 3 + i] - c[i];
        v_l[3 * b + i] = v;
        mv_l[3 * b + i] = mass * v;
        am_l[3 * b + i] = wl[i];
      }
    }
    wave_sync();
    for (int w = l; w < nb * 3; w += L) {
      const int b = w / 3, k = w - 3 * b;
      const int end = a.body_subtree_end[b];
      REAL s = 0;
      for (int d = end - 1; d >= b; d--) s += mv_l[3 * d + k];
      const REAL sm = a.body_subtreemass[b];
      const REAL lv = s / (sm > (REAL)mjMINVAL ? sm : (REAL)mjMINVAL);
      lin_l[w] = lv;
      a.subtree_linvel[e * nb * 3 + w] = lv;
    }
    wave_sync();
    // angular momentum: the walk from the last body to the first, one tree level per trip.  A body first takes what its children (later bodies, last first) hand up, then its own term.
    for (int lev = md; lev >= 0; lev--) {
      for (int b = l; b < nb; b += L) {
        if (a.body_depth[b] != lev) continue;
        REAL Lb[3] = {am_l[3 * b], am_l[3 * b + 1], am_l[3 * b + 2]};
        const int end = a.body_subtree_end[b];
        for (int d = end - 1; d > b; d--) {
          if (a.body_parentid[d] != b) continue;
#pragma unroll
          for (int k = 0; k < 3; k++) Lb[k] = Lb[k] + mv_l[3 * d + k];
        }
        const REAL mass = a.body_mass[b];
        REAL dx[3], dp[3], dL[3];
#pragma unroll
        for (int k = 0; k < 3; k++) { dx[k] = xip[3 * b + k] - com[3 * b + k]; dp[k] = mass * (v_l[3 * b + k] - lin_l[3 * b + k]); }
        cross3(dx, dp, dL);
#pragma unroll
        for (int k = 0; k < 3; k++) Lb[k] = Lb[k] + dL[k];
        const int par = a.body_parentid[b];
        const REAL sm = a.body_subtreemass[b];
#pragma unroll
        for (int k = 0; k < 3; k++) { dx[k] = com[3 * b + k] - com[3 * par + k]; dp[k] = sm * (lin_l[3 * b + k] - lin_l[3 * par + k]); }
        cross3(dx, dp, dL);
#pragma unroll
        for (int k = 0; k < 3; k++) {
          am_l[3 * b + k] = Lb[k];
          mv_l[3 * b + k] = Lb[k] + dL[k];  // (mass * v of this body is dead: its level is done with it)
          a.subtree_angmom[(e * nb + b) * 3 + k] = Lb[k];
        }
      }
      wave_sync();
    }
  }

  if (a.flags & MJH_POSTCON_SENSORS) {
    const int nsd = a.nsensordata;
    for (int k = l; k < nsd; k += L) {
      const int s = a.slot_sensor[k];
      const int type = s >= 0 ? a.sns_type[s] : -1;
      REAL v;
      if (type == 1 || type == 4 || type == 5 || type == 36 || type == 37) {
        v = pc_sensor<REAL>(a, e, type, s, k - a.sns_adr[s], acc_l, int_l, lin_l, am_l);
        const REAL cutoff = a.sns_cutoff[s];
        const int dt = a.sns_datatype[s];
        if (cutoff > 0) {
          if (dt == 0) v = v < -cutoff ? -cutoff : (v > cutoff ? cutoff : v);
          else if (dt == 1) v = v < cutoff ? v : cutoff;
        }
      } else {
        v = a.sensordata_in[e * nsd + k];
      }
      a.sensordata[e * nsd + k] = v;
    }
  }
}
#undef PC_ROT_T
