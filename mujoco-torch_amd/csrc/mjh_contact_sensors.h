// mjh_contact_sensors.h -- the force of every contact (MuJoCo's mj_contactForce, MJX support.contact_force) and the sensors that sit on it and on cacc: touch,
// framelinacc, frameangacc.  No pass of the reference evaluates them (their sensordata slots keep the caller's values through step / forward, here too); this kernel
// runs on a finished pass, after mjh_postcon_kernel has written cacc.
//
// contact force, per slot c: w = the contact-frame wrench from efc_force at contact.efc_address[c], the decode of mjh_postcon.h: elliptic cone or dim 1: w[:dim] = the
//   dim rows, the rest 0; pyramidal with dim > 1: w[0] = the sum of the 2 (dim - 1) rows in row order, w[k] = (p[2 (k - 1)] - p[2 (k - 1) + 1]) * friction[k - 1].  A slot
//   whose geom ids are not in [0, ngeom), or whose rows do not lie inside efc_force, gives zeros.  The row is [force(3), torque(3)] (MuJoCo's order, not the
//   rotational-first order of cfrc_ext), in the contact frame, or with to_world as [frame^T w[0:3], frame^T w[3:6]].
// touch on site s, b = site_bodyid[s]: the sum of w[0] over the slots c, in slot order, that are valid as above, have b in {geom_bodyid[g1], geom_bodyid[g2]}, w[0] > 0,
//   and whose ray from contact.pos[c] along v meets the site's shape (site_type, site_size, site_xpos, site_xmat; ray_geom of mjh_ray.h after ray_to_geom) at a distance
//   >= 0.  v = +frame[c][0] when b is geom 1's body, -frame[c][0] when it is geom 2's: the ray points out of the sensor's body, so a contact point inside the zone
//   always counts.  Site shapes: sphere, capsule, ellipsoid, cylinder, box.
// framelinacc / frameangacc of a body (its point: xipos), xbody (xpos), geom (geom_xpos), site (site_xpos) or camera (cam_xpos) riding on `body`, root = body_rootid[body]:
//   dif = pos - subtree_com[root], omega = cvel[body][0:3], alpha = cacc[body][0:3], vlin = cvel[body][3:6] - dif x omega;
//   frameangacc = alpha;  framelinacc = (cacc[body][3:6] - dif x alpha) + omega x vlin.  Both in the world frame; a reference frame (reftype / refid) on these two types
//   is ignored, as MuJoCo ignores it.
// cutoff: mjh_sensor.h's rule by sensor_datatype (real: clamp to +-cutoff, positive: min(v, cutoff), when cutoff > 0); touch is positive.
//
// The packing of mjh_postcon_kernel: `lanes` (16 / 32 / 64, from the larger of ncon and the number of these sensors) lanes serve one environment, up to 256 / lanes
// environments share a workgroup, an environment's lanes lie inside one wavefront (wave barriers only).  One lane per contact slot decodes w once, writes the slot's
// contact_force row (rows of consecutive (environment, slot) pairs are consecutive in memory) and leaves what the touch sensors need in LDS: w[0], the two bodies, the
// contact point and the normal.  One lane per sensor then walks the slots in slot order, or evaluates its frame object, and writes the sensor's slots of sensordata
// (every other slot is left as it is).  No atomics: every sum has one fixed order, so the results do not depend on lanes, packing or how the host cut the batch.
// Contacts and sensors beyond the lane count take several trips.  Every leaf element is read once, by the lane that owns its contact slot or sensor.
#pragma once
#include "mjh_device.h"
#include "mjh_ray.h"

#define MJH_CONSENS_WG 256
#define MJH_CONSENS_LDS_CONTACT 12  // REALs of LDS per contact slot: w[0], body 1, body 2, pos(3), normal(3), padding (a multiple of 4: 16-byte carve offsets)
#define MJH_CONSENS_COLS 8          // ints per sensor row: type, adr, objid, kind, bodyid, rootid, datatype, sitetype

template <typename REAL>
struct ConSensArgs {
  // [B, ...] leaves of a finished forward pass (cacc: mjh_postconstraint's)
  const REAL *efc_force, *contact_pos, *contact_frame, *contact_friction;
  const int* contact_dim;
  const int64_t *contact_geom, *contact_efc_address;
  const REAL *site_xmat, *cvel, *cacc, *subtree_com;
  const REAL *xipos, *xpos, *geom_xpos, *site_xpos, *cam_xpos;  // the frame objects' points by leaf kind 0 .. 4: [B, nbody | nbody | ngeom | nsite | ncam, 3]
  // tables: the model's geom_bodyid (the blob) and site_size (the caller's Model), the sensor rows and cutoffs (device arrays of the caller's)
  const int *geom_bodyid, *sns;
  const REAL *site_size, *sns_cutoff;
  // outputs
  REAL *force;       // [B, ncon, 6]
  REAL *sensordata;  // [B, nsensordata]: only the slots of these sensors are written
  int nbody, ncon, nefc, ngeom, nsite, ncam, nsensordata, nsens;
  int pyramidal;  // opt.cone
  int flags;      // MJH_CONSENS_*
  int contacts;   // the contact stage runs (forces asked for, or a touch sensor present)
  int lanes, envs;  // lanes per environment, environments per workgroup
  int lds_env;      // REALs of LDS per environment (a multiple of 4)
  int64_t env_begin, env_count;
};

#define CS_ROT_T(R_, v, o) for (int i_ = 0; i_ < 3; i_++) (o)[i_] = (R_)[i_] * (v)[0] + (R_)[3 + i_] * (v)[1] + (R_)[6 + i_] * (v)[2];

template <typename REAL>
__global__ __launch_bounds__(MJH_CONSENS_WG) void mjh_consens_kernel(ConSensArgs<REAL> a) {
  extern __shared__ __attribute__((aligned(16))) double cs_lds_raw[];
  const int L = a.lanes;
  const int slot = (int)threadIdx.x / L, l = (int)threadIdx.x - slot * L;
  const int64_t e = a.env_begin + (int64_t)blockIdx.x * a.envs + slot;
  if (slot >= a.envs || e >= a.env_begin + a.env_count) return;  // (whole environments only: an environment's lanes all return or none do)
  const int ncon = a.ncon, nb = a.nbody;
  REAL* cl = reinterpret_cast<REAL*>(cs_lds_raw) + (int64_t)slot * a.lds_env;  // MJH_CONSENS_LDS_CONTACT per contact slot

  if (a.contacts) {
    // one lane per contact slot: the wrench, once
    for (int c = l; c < ncon; c += L) {
      const int64_t g1 = a.contact_geom[(e * ncon + c) * 2], g2 = a.contact_geom[(e * ncon + c) * 2 + 1];
      const int dim = a.contact_dim[e * ncon + c];
      const int64_t adr = a.contact_efc_address[e * ncon + c];
      const bool pyr = a.pyramidal && dim > 1;
      const int rows = pyr ? 2 * (dim - 1) : dim;
      const bool ok = g1 >= 0 && g2 >= 0 && g1 < a.ngeom && g2 < a.ngeom && dim >= 1 && dim <= 6 && adr >= 0 && adr + rows <= a.nefc;
      REAL w[6] = {0, 0, 0, 0, 0, 0};
      int b1 = -1, b2 = -1;
      if (ok) {
        b1 = a.geom_bodyid[g1]; b2 = a.geom_bodyid[g2];
        const REAL* p = a.efc_force + e * a.nefc + adr;
        if (!pyr) {
          for (int k = 0; k < dim; k++) w[k] = p[k];
        } else {
          const REAL* fr = a.contact_friction + (e * ncon + c) * 5;
          REAL s = p[0];
          for (int k = 1; k < rows; k++) s = s + p[k];
          w[0] = s;
          for (int k = 1; k < dim; k++) w[k] = (p[2 * (k - 1)] - p[2 * (k - 1) + 1]) * fr[k - 1];
        }
      }
      const REAL* fp = a.contact_frame + (e * ncon + c) * 9;
      REAL F[9];
#pragma unroll
      for (int i = 0; i < 9; i++) F[i] = fp[i];
      if (a.flags & MJH_CONSENS_FORCES) {
        REAL o[6];
        if (a.flags & MJH_CONSENS_WORLD) {
          CS_ROT_T(F, w, o)
          CS_ROT_T(F, w + 3, o + 3)
        } else {
#pragma unroll
          for (int k = 0; k < 6; k++) o[k] = w[k];
        }
        REAL* dst = a.force + (e * ncon + c) * 6;
#pragma unroll
        for (int k = 0; k < 6; k++) dst[k] = o[k];
      }
      const REAL* pp = a.contact_pos + (e * ncon + c) * 3;
      REAL* q = cl + MJH_CONSENS_LDS_CONTACT * c;
      q[0] = w[0]; q[1] = (REAL)b1; q[2] = (REAL)b2;
#pragma unroll
      for (int i = 0; i < 3; i++) { q[3 + i] = pp[i]; q[6 + i] = F[i]; }
    }
    wave_sync();
  }

  if (a.flags & MJH_CONSENS_SENSORS) {
    const int nsd = a.nsensordata;
    for (int s = l; s < a.nsens; s += L) {
      const int* row = a.sns + MJH_CONSENS_COLS * s;
      const int type = row[0], adr = row[1], obj = row[2], kind = row[3], body = row[4], root = row[5], dt = row[6], stype = row[7];
      const REAL cutoff = a.sns_cutoff[s];
      const REAL* leaf = kind == 0 ? a.xipos : (kind == 1 ? a.xpos : (kind == 2 ? a.geom_xpos : (kind == 3 ? a.site_xpos : a.cam_xpos)));
      const int count = kind <= 1 ? nb : (kind == 2 ? a.ngeom : (kind == 3 ? a.nsite : a.ncam));
      const REAL* posp = leaf + (e * count + obj) * 3;
      const REAL pos[3] = {posp[0], posp[1], posp[2]};
      REAL v[3] = {0, 0, 0};
      const int n = type == 0 ? 1 : 3;
      if (type == 0) {  // touch
        const REAL* xm = a.site_xmat + (e * a.nsite + obj) * 9;
        REAL R[9];
#pragma unroll
        for (int i = 0; i < 9; i++) R[i] = xm[i];
        const REAL size[3] = {a.site_size[3 * obj], a.site_size[3 * obj + 1], a.site_size[3 * obj + 2]};
        REAL sum = 0;
        for (int c = 0; c < ncon; c++) {
          const REAL* q = cl + MJH_CONSENS_LDS_CONTACT * c;
          const int b1 = (int)q[1], b2 = (int)q[2];
          const REAL w0 = q[0];
          if (b1 < 0 || !(w0 > 0) || (b1 != body && b2 != body)) continue;
          const REAL sgn = b1 == body ? (REAL)1 : (REAL)-1;
          const REAL pnt[3] = {q[3], q[4], q[5]}, vec[3] = {sgn * q[6], sgn * q[7], sgn * q[8]};
          REAL dp[3], dv[3];
          ray_to_geom<REAL>(R, pos, pnt, vec, dp, dv);
          const REAL x = ray_geom<REAL>(stype, size, dp, dv);
          if (x >= 0 && !isinf(x)) sum = sum + w0;
        }
        v[0] = sum;
      } else {
        const REAL* sc = a.subtree_com + (e * nb + root) * 3;
        const REAL* cap = a.cacc + (e * nb + body) * 6;
        const REAL ca[6] = {cap[0], cap[1], cap[2], cap[3], cap[4], cap[5]};
        if (type == 34) {  // frameangacc
#pragma unroll
          for (int i = 0; i < 3; i++) v[i] = ca[i];
        } else {  // framelinacc
          const REAL* cvp = a.cvel + (e * nb + body) * 6;
          const REAL cv[6] = {cvp[0], cvp[1], cvp[2], cvp[3], cvp[4], cvp[5]};
          const REAL dif[3] = {pos[0] - sc[0], pos[1] - sc[1], pos[2] - sc[2]};
          REAL c1[3], c2[3], c3[3], vlin[3];
          cross3(dif, cv, c1);
#pragma unroll
          for (int i = 0; i < 3; i++) vlin[i] = cv[3 + i] - c1[i];
          cross3(dif, ca, c2);
          cross3(cv, vlin, c3);
#pragma unroll
          for (int i = 0; i < 3; i++) v[i] = (ca[3 + i] - c2[i]) + c3[i];
        }
      }
#pragma unroll
      for (int i = 0; i < 3; i++) {
        if (i >= n) break;
        REAL x = v[i];
        if (cutoff > 0) {
          if (dt == 0) x = x < -cutoff ? -cutoff : (x > cutoff ? cutoff : x);
          else if (dt == 1) x = x < cutoff ? x : cutoff;
        }
        a.sensordata[e * nsd + adr + i] = x;
      }
    }
  }
}
#undef CS_ROT_T
