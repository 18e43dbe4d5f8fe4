// mjh_energy.h -- the potential and kinetic energy of a finished pass (MuJoCo's mj_energyPos / mj_energyVel, d.energy; the reference has no counterpart) and the
// sensors no pass evaluates that read them or a limit's constraint row: jointlimitpos / vel / frc, tendonlimitpos / vel / frc, e_potential, e_kinetic.
//
// potential:  V = - sum_{b = 1 .. nbody - 1} body_mass[b] * dot(gravity, xipos[b])                         unless DisableBit.GRAVITY
//               + sum_joints 1/2 k (q - qpos_spring)^2                                                      slide / hinge
//                            1/2 k |pos - pos_spring|^2 + 1/2 k |phi|^2                                     free (phi: of its quaternion)
//                            1/2 k |phi|^2,  phi = quat_sub(normalize(quat), quat_spring)                   ball: the rotation vector the step's spring force uses
//               + sum_tendons 1/2 k disp^2, disp = how far ten_length lies outside tendon_lengthspring      (the force's rule: `above` wins over `below`)
//             the spring terms under the flags the step applies the spring forces under: neither DisableBit.SPRING nor DisableBit.DAMPER set (passive.py:178).
// kinetic:    T = 1/2 qvel^T (qM qvel), qM the pass's dense matrix as stored (armature and tendon armature are in it).
// Gravity compensation and fluid forces have no potential here, as in MuJoCo.
// sensors, one row of `sns` each (type, sensordata address, object id, the limit's row in efc_J / efc_force or -1, datatype, the joint's type):
//   jointlimitpos / tendonlimitpos:  dist - margin if dist < margin else 0;  dist = min(q - range[0], range[1] - q) for a hinge / slide joint or a tendon's ten_length,
//                                    max(range) - angle for a ball joint (constraint.py:302-405)
//   jointlimitvel / tendonlimitvel:  efc_J[row] . qvel, columns in order (the pass has zeroed the row of an inactive limit)
//   jointlimitfrc / tendonlimitfrc:  efc_force[row]
//   e_potential / e_kinetic:         V / T above (the call computes them: MJH_ENERGY_POS / MJH_ENERGY_VEL)
//   A limit sensor whose object has no row (row < 0: not limited, or limits / constraints disabled) gives 0.  Then mjh_sensor.h's cutoff rule by datatype.
//
// The packing of mjh_postcon_kernel / mjh_consens_kernel: `lanes` (16 / 32 / 64, from the largest of nbody, nv and the sensor count) lanes serve one environment, up to
// 256 / lanes environments share a workgroup, an environment's lanes lie inside one wavefront (wave barriers only).  qM, the only large read, comes from global memory
// once, by flat coalesced loads through an LDS chunk of `chunk` rows (inv_load of mjh_inverse.h), so any nv the library accepts fits the same footprint.  No atomics:
// a lane accumulates its strided terms in index order (bodies, then joints, then tendons; matrix rows in row order), lane 0 adds the per-lane partials in lane order
// through LDS.  lanes and chunk follow from the model and the size of its sensor table alone (every call passes that size), so a result
// does not depend on B, on the environment's slot in its workgroup or on how the host cut the batch, and the energy sensors' slots are the energies' bits.
// The model VALUES (gravity, body_mass, jnt_stiffness, qpos_spring, the tendon springs, ranges, margins, cutoffs) are arguments of the call, not the blob's.
#pragma once
#include "mjh_device.h"
#include "mjh_inverse.h"

#define MJH_ENERGY_WG 256
#define MJH_ENERGY_COLS 6  // ints per sensor row: type, adr, objid, efc row, datatype, joint type

template <typename REAL>
struct EnergyArgs {
  // [B, ...] leaves of a finished forward pass (qpos / qvel: the state the pass ran on)
  const REAL *qpos, *qvel, *xipos, *ten_length, *qM, *efc_J, *efc_force;
  // the caller's model values
  const REAL *gravity, *body_mass, *jnt_stiffness, *qpos_spring, *jnt_range, *jnt_margin, *tendon_stiffness, *tendon_lengthspring, *tendon_range, *tendon_margin, *sns_cutoff;
  // tables: the model's jnt_type / jnt_qposadr (the blob), the sensor rows (a device array of the caller's)
  const int *jnt_type, *jnt_qposadr, *sns;
  // outputs
  REAL* energy;      // [B, 2]: [potential, kinetic]; the halves the flags ask for are written (may be null in a call for the sensors)
  REAL* sensordata;  // [B, nsensordata]: only the slots of these sensors are written
  int nq, nv, nbody, njnt, ntendon, nefc, nsensordata, nsens;
  int flags;                  // MJH_ENERGY_*
  int gravity_on, spring_on;  // from opt.disableflags
  int lanes, envs, chunk;     // lanes per environment, environments per workgroup, rows of qM per LDS chunk
  int lds_env;                // REALs of LDS per environment (a multiple of 4)
  int64_t env_begin, env_count;
};

template <typename REAL>
__global__ __launch_bounds__(MJH_ENERGY_WG) void mjh_energy_kernel(EnergyArgs<REAL> a) {
  extern __shared__ __attribute__((aligned(16))) double en_lds_raw[];
  const int L = a.lanes;
  const int slot = (int)threadIdx.x / L, l = (int)threadIdx.x - slot * L;
  const int64_t e = a.env_begin + (int64_t)blockIdx.x * a.envs + slot;
  if (slot >= a.envs || e >= a.env_begin + a.env_count) return;  // (whole environments only: an environment's lanes all return or none do)
  const int nv = a.nv, nq = a.nq, nb = a.nbody, nt = a.ntendon;
  REAL* x = reinterpret_cast<REAL*>(en_lds_raw) + (int64_t)slot * a.lds_env;  // qvel (nv, rounded up to a multiple of 4)
  REAL* pv = x + ((nv + 3) & ~3);                                             // the lanes' partial sums of V ...
  REAL* pk = pv + L;                                                          // ... and of qvel^T qM qvel
  REAL* res = pk + L;                                                         // [V, T, -, -]
  REAL* buf = res + 4;                                                        // chunk rows of qM
  const REAL* qpos = a.qpos + e * nq;

  if (a.flags & MJH_ENERGY_POS) {
    REAL p = 0;
    if (a.gravity_on) {
      const REAL g0 = a.gravity[0], g1 = a.gravity[1], g2 = a.gravity[2];
      for (int b = 1 + l; b < nb; b += L) {
        const REAL* xp = a.xipos + (e * nb + b) * 3;
        p = p - a.body_mass[b] * ((g0 * xp[0] + g1 * xp[1]) + g2 * xp[2]);
      }
    }
    if (a.spring_on) {
      for (int j = l; j < a.njnt; j += L) {
        const REAL k = a.jnt_stiffness[j];
        if (k == 0) continue;
        const int t = a.jnt_type[j];
        const REAL* q = qpos + a.jnt_qposadr[j];
        const REAL* qs = a.qpos_spring + a.jnt_qposadr[j];
        if (t == JNT_FREE || t == JNT_BALL) {
          if (t == JNT_FREE) {
            const REAL d0 = q[0] - qs[0], d1 = q[1] - qs[1], d2 = q[2] - qs[2];
            p = p + ((REAL)0.5 * k) * ((d0 * d0 + d1 * d1) + d2 * d2);
            q += 3; qs += 3;
          }
          REAL u[4] = {q[0], q[1], q[2], q[3]}, r[3];
          normalize_n<REAL, 4>(u);
          quat_sub(u, qs, r);
          p = p + ((REAL)0.5 * k) * ((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]);
        } else {
          const REAL d = q[0] - qs[0];
          p = p + ((REAL)0.5 * k) * (d * d);
        }
      }
      for (int t = l; t < nt; t += L) {
        const REAL k = a.tendon_stiffness[t];
        if (k == 0) continue;
        const REAL len = a.ten_length[e * nt + t];
        const REAL below = a.tendon_lengthspring[2 * t] - len, above = a.tendon_lengthspring[2 * t + 1] - len;
        const REAL disp = above < 0 ? above : (below > 0 ? below : (REAL)0);
        p = p + ((REAL)0.5 * k) * (disp * disp);
      }
    }
    pv[l] = p;
  }

  if (a.flags & MJH_ENERGY_VEL) {
    for (int i = l; i < nv; i += L) x[i] = a.qvel[e * nv + i];
    wave_sync();
    const REAL* qM = a.qM + e * nv * nv;
    REAL p = 0;
    for (int r0 = 0; r0 < nv; r0 += a.chunk) {
      const int rows = nv - r0 < a.chunk ? nv - r0 : a.chunk;
      inv_load<REAL>(buf, qM + (int64_t)r0 * nv, rows * nv, l, L);
      wave_sync();
      for (int r = l; r < rows; r += L) {
        REAL s = 0;
        for (int k = 0; k < nv; k++) s += buf[r * nv + k] * x[k];
        p = p + x[r0 + r] * s;
      }
      wave_sync();
    }
    pk[l] = p;
  }
  wave_sync();
  if (l == 0) {  // the partials in lane order
    REAL V = 0, T = 0;
    if (a.flags & MJH_ENERGY_POS) {
      for (int i = 0; i < L; i++) V = V + pv[i];
      if (a.energy) a.energy[e * 2] = V;
    }
    if (a.flags & MJH_ENERGY_VEL) {
      for (int i = 0; i < L; i++) T = T + pk[i];
      T = (REAL)0.5 * T;
      if (a.energy) a.energy[e * 2 + 1] = T;
    }
    res[0] = V; res[1] = T;
  }
  wave_sync();

  if (a.flags & MJH_ENERGY_SENSORS) {
    const int nsd = a.nsensordata, nefc = a.nefc;
    for (int s = l; s < a.nsens; s += L) {
      const int* row = a.sns + MJH_ENERGY_COLS * s;
      const int type = row[0], adr = row[1], obj = row[2], er = row[3], dt = row[4], jt = row[5];
      const REAL cutoff = a.sns_cutoff[s];
      REAL v = 0;
      if (type == 43) v = res[0];       // e_potential
      else if (type == 44) v = res[1];  // e_kinetic
      else if (er >= 0) {
        if (type == 20 || type == 23) {  // jointlimitpos, tendonlimitpos
          REAL dist, margin;
          if (type == 23) {
            const REAL len = a.ten_length[e * nt + obj];
            const REAL dmin = len - a.tendon_range[2 * obj], dmax = a.tendon_range[2 * obj + 1] - len;
            dist = dmin < dmax ? dmin : dmax;
            margin = a.tendon_margin[obj];
          } else {
            const REAL* q = qpos + a.jnt_qposadr[obj];
            const REAL r0 = a.jnt_range[2 * obj], r1 = a.jnt_range[2 * obj + 1];
            if (jt == JNT_BALL) {
              const REAL u[4] = {q[0], q[1], q[2], q[3]};
              REAL axis[3], angle;
              quat_to_axis_angle(u, axis, angle);
              dist = (r0 > r1 ? r0 : r1) - angle;
            } else {
              const REAL dmin = q[0] - r0, dmax = r1 - q[0];
              dist = dmin < dmax ? dmin : dmax;
            }
            margin = a.jnt_margin[obj];
          }
          v = dist < margin ? dist - margin : (REAL)0;
        } else if (type == 21 || type == 24) {  // jointlimitvel, tendonlimitvel
          const REAL* J = a.efc_J + (e * nefc + er) * nv;
          const REAL* qv = a.qvel + e * nv;
          REAL acc = 0;
          for (int k = 0; k < nv; k++) acc += J[k] * qv[k];
          v = acc;
        } else {  // jointlimitfrc, tendonlimitfrc
          v = a.efc_force[e * nefc + er];
        }
      }
      if (cutoff > 0) {
        if (dt == 0) v = v < -cutoff ? -cutoff : (v > cutoff ? cutoff : v);
        else if (dt == 1) v = v < cutoff ? v : cutoff;
      }
      a.sensordata[e * nsd + adr] = v;
    }
  }
}
