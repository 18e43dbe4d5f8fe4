// mjh_inverse.h -- the tail of inverse dynamics (reference mujoco_torch/_src/inverse.py: discrete_acc, inv_constraint, the qfrc_inverse sum).
//
// Runs behind a forward pass of stages 0x1F (kinematics .. velocity: efc_J / efc_D / efc_aref, qM / qLD, qfrc_bias, qfrc_passive are in `out`).
// Per environment, with the caller's qacc:
//   discrete (Euler, eulerdamp on, some dof_damping != 0):  qacc <- solve_m(M qacc + h * dof_damping o qacc)     inverse.py:24-40, 57-60
//   jaref = efc_J qacc - efc_aref;  efc_force = efc_D * -jaref * (jaref < 0 || row < ne + nf);  qfrc_constraint = efc_J^T efc_force   :63-83
//   qfrc_inverse = qfrc_bias + M qacc - qfrc_passive - qfrc_constraint                                                                 :97
// A streaming kernel: its bytes are efc_J and qM, each read from HBM ONCE.  `lanes` (16 / 32 / 64) lanes serve one environment, 256 / lanes environments share a
// workgroup; an environment's lanes lie inside one wavefront, so its LDS is synchronised by wave barriers only.  Both matrices stream through one LDS buffer of
// `chunk` rows per environment (flat, coalesced loads of consecutive rows): a chunk of efc_J serves J qacc (one row per lane) and then J^T f (one column per lane)
// before the next chunk is loaded, so any nefc / nv the library accepts fits the same footprint.  Sums run in row / column order whatever the chunk, so the
// result does not depend on the packing or on how the host cut the batch.
#pragma once
#include "mjh_device.h"

template <typename REAL>
struct InvArgs {
  const REAL *efc_J, *efc_D, *efc_aref, *qM, *qLD, *qfrc_bias, *qfrc_passive, *qacc;  // [B, ...] leaves (qacc: the caller's)
  const REAL* dof_damping;                                                            // model constant (nv)
  REAL *efc_force, *qfrc_constraint, *qfrc_inverse;                                   // outputs
  REAL timestep;
  int nv, nefc, nalways;   // nalways = ne + nf: equality and friction rows are always active
  int discrete;            // 1: the eulerdamp re-solve of discrete_acc applies
  int lanes, envs, chunk;  // lanes per environment, environments per workgroup, matrix rows per LDS chunk
  int lds_env;             // REALs of LDS per environment
  int64_t env_begin, env_count;
};

// rows [0, n) x nv of a contiguous row-major matrix -> LDS, four requests per lane in flight per trip
template <typename REAL>
__device__ __forceinline__ void inv_load(REAL* dst, const REAL* src, int n, int l, int L) {
  int i = l;
  for (; i + 3 * L < n; i += 4 * L) {
    const REAL a = src[i], b = src[i + L], c = src[i + 2 * L], d = src[i + 3 * L];
    dst[i] = a; dst[i + L] = b; dst[i + 2 * L] = c; dst[i + 3 * L] = d;
  }
  for (; i < n; i += L) dst[i] = src[i];
}

// y = M x (qM: [nv, nv] row-major, global), streamed through `buf` in chunks of `chunk` rows; one row per lane
template <typename REAL>
__device__ __forceinline__ void inv_mul_m(const InvArgs<REAL>& a, const REAL* qM, const REAL* x, REAL* y, REAL* buf, int l, int L) {
  const int nv = a.nv;
  for (int r0 = 0; r0 < nv; r0 += a.chunk) {
    const int rows = nv - r0 < a.chunk ? nv - r0 : a.chunk;
    inv_load<REAL>(buf, qM + (int64_t)r0 * nv, rows * nv, l, L);
    wave_sync();
    for (int r = l; r < rows; r += L) {
      REAL s = 0;
      for (int k = 0; k < nv; k++) s += buf[r * nv + k] * x[k];
      y[r0 + r] = s;
    }
    wave_sync();
  }
}

template <typename REAL>
__global__ __launch_bounds__(256) void mjh_inverse_kernel(InvArgs<REAL> a) {
  extern __shared__ double inv_lds_raw[];
  const int L = a.lanes;
  const int slot = (int)threadIdx.x / L, l = (int)threadIdx.x - slot * L;
  const int64_t e = a.env_begin + (int64_t)blockIdx.x * a.envs + slot;
  if (slot >= a.envs || e >= a.env_begin + a.env_count) return;  // (whole environments only: an environment's lanes all return or none do)
  const int nv = a.nv, nefc = a.nefc;
  REAL* x = reinterpret_cast<REAL*>(inv_lds_raw) + (int64_t)slot * a.lds_env;  // qacc (after discrete_acc)
  REAL* y = x + nv;            // M qacc (the right-hand side of discrete_acc first)
  REAL* c = y + nv;            // qfrc_constraint
  REAL* f = c + nv;            // efc_force of the current chunk
  REAL* buf = f + a.chunk;     // chunk rows of efc_J / qM

  const REAL* qM = a.qM + e * nv * nv;
  for (int i = l; i < nv; i += L) { x[i] = a.qacc[e * nv + i]; c[i] = 0; }
  wave_sync();

  if (a.discrete) {  // discrete_acc, Euler: qfrc = M qacc + h * dof_damping o qacc; qacc = solve_m(qfrc) (math.small_cholesky_solve :152-166)
    inv_mul_m<REAL>(a, qM, x, y, buf, l, L);
    for (int i = l; i < nv; i += L) y[i] = y[i] + a.timestep * a.dof_damping[i] * x[i];
    wave_sync();
    const REAL* Ld = a.qLD + e * nv * nv;
    // forward substitution L z = qfrc, column by column: element i subtracts L[i][k] z[k] in k order, as the reference's row loop does
    for (int k = 0; k < nv; k++) {
      const REAL zk = y[k] / Ld[k * nv + k];
      for (int i = k + 1 + l; i < nv; i += L) y[i] = y[i] - Ld[i * nv + k] * zk;
      wave_sync();
      if (l == 0) y[k] = zk;
      wave_sync();
    }
    // backward substitution L^T x = z
    for (int k = nv - 1; k >= 0; k--) {
      const REAL xk = y[k] / Ld[k * nv + k];
      for (int i = l; i < k; i += L) y[i] = y[i] - Ld[k * nv + i] * xk;
      wave_sync();
      if (l == 0) y[k] = xk;
      wave_sync();
    }
    for (int i = l; i < nv; i += L) x[i] = y[i];
    wave_sync();
  }

  inv_mul_m<REAL>(a, qM, x, y, buf, l, L);

  // inv_constraint: one pass over efc_J, chunk by chunk
  const REAL* J = a.efc_J + e * nefc * nv;
  for (int r0 = 0; r0 < nefc; r0 += a.chunk) {
    const int rows = nefc - r0 < a.chunk ? nefc - r0 : a.chunk;
    inv_load<REAL>(buf, J + (int64_t)r0 * nv, rows * nv, l, L);
    wave_sync();
    for (int r = l; r < rows; r += L) {
      const int row = r0 + r;
      REAL s = 0;
      for (int k = 0; k < nv; k++) s += buf[r * nv + k] * x[k];
      const REAL jaref = s - a.efc_aref[e * nefc + row];
      const bool active = jaref < 0 || row < a.nalways;
      const REAL force = a.efc_D[e * nefc + row] * -jaref * (REAL)(active ? 1 : 0);
      f[r] = force;
      a.efc_force[e * nefc + row] = force;
    }
    wave_sync();
    for (int k = l; k < nv; k += L) {
      REAL s = c[k];
      for (int r = 0; r < rows; r++) s += buf[r * nv + k] * f[r];
      c[k] = s;
    }
    wave_sync();
  }

  for (int i = l; i < nv; i += L) {
    const REAL qc = c[i];
    a.qfrc_constraint[e * nv + i] = qc;
    a.qfrc_inverse[e * nv + i] = ((a.qfrc_bias[e * nv + i] + y[i]) - a.qfrc_passive[e * nv + i]) - qc;
  }
}
