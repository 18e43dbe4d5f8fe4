// mjhip.hip -- C ABI of the MI355X-native stepper (see include/mjhip.h) and the host side of the launches.
//
// Host work per call: fill the kernarg struct of each pipeline phase and enqueue it on the caller's stream
// (5 launches per forward pass; 20 for an RK4 step).  No allocation, no synchronisation, no PyTorch types:
// the binding (ctypes) passes raw device pointers.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "mjh_kernels.h"
#include "mjh_convex.h"
#include "mjh_sensor.h"
#include "mjh_reset.h"
#include "mjh_io.h"
#include "mjh_inverse.h"
#include "mjh_ray.h"
#include "mjh_render.h"
#include "mjh_support.h"
#include "mjh_fd.h"
#include "mjh_ifd.h"
#include "mjh_postcon.h"
#include "mjh_contact_sensors.h"
#include "mjh_energy.h"
#include "mjh_jacobian.h"
#include "mjh_integrate.h"
#include "mjh_smooth.h"
#include "mjh_dynamics.h"
#include "mjh_quadric.h"
#include "mjh_geomdist.h"
#include "mjh_qpos.h"
#include "mjh_ik.h"
#include "mjh_efc.h"
#include "mjh_pgs.h"
#include "mjh_solve.h"
#include "mjh_noslip.h"
#include "mjh_instances.h"

// the kernels are compiled in their own translation units (mjh_inst.hip, one per build group): this file is the host side only
#define X_(R, P, W) extern template __global__ void mjh_phase_kernel<R, P, W>(KArgs<R>);
#define S_(R, N, RPL, W) extern template __global__ void mjh_sol2_kernel<R, N, RPL, W>(KArgs<R>);
#define C_(R) extern template __global__ void mjh_convex_kernel<R>(KArgs<R>);
#define N_(R) extern template __global__ void mjh_sensor_kernel<R, 0>(KArgs<R>); extern template __global__ void mjh_sensor_kernel<R, 1>(KArgs<R>);
MJH_INST_ALL(X_, S_, C_, N_, double)
MJH_INST_ALL(X_, S_, C_, N_, float)
extern template __global__ void mjh_inverse_kernel<double>(InvArgs<double>);  // (build group 19)
extern template __global__ void mjh_inverse_kernel<float>(InvArgs<float>);
extern template __global__ void mjh_ray_kernel<double>(RayArgs<double>);  // (build group 20)
extern template __global__ void mjh_ray_kernel<float>(RayArgs<float>);
extern template __global__ void mjh_render_kernel<double>(RenderArgs<double>);  // (build group 21)
extern template __global__ void mjh_render_kernel<float>(RenderArgs<float>);
#define SUP_(R)                                                                                                    \
  extern template __global__ void mjh_sup_point_kernel<R, true>(SupArgs<R>);                                       \
  extern template __global__ void mjh_sup_point_kernel<R, false>(SupArgs<R>);                                      \
  extern template __global__ void mjh_sup_xfrc_kernel<R>(SupArgs<R>);                                              \
  extern template __global__ void mjh_sup_mulm_kernel<R>(SupArgs<R>);                                              \
  extern template __global__ void mjh_sup_solvem_kernel<R>(SupArgs<R>);
SUP_(double)  // (build group 22)
SUP_(float)
#undef SUP_
extern template __global__ void mjh_fd_perturb_kernel<double>(FdPerturbArgs<double>);  // (build group 23)
extern template __global__ void mjh_fd_perturb_kernel<float>(FdPerturbArgs<float>);
extern template __global__ void mjh_fd_difference_kernel<double>(FdDiffArgs<double>);
extern template __global__ void mjh_fd_difference_kernel<float>(FdDiffArgs<float>);
extern template __global__ void mjh_fd_vjp_kernel<double>(FdVjpArgs<double>);
extern template __global__ void mjh_fd_vjp_kernel<float>(FdVjpArgs<float>);
extern template __global__ void mjh_fd_tangent_kernel<double>(FdTangentArgs<double>);
extern template __global__ void mjh_fd_tangent_kernel<float>(FdTangentArgs<float>);
extern template __global__ void mjh_postcon_kernel<double>(PostconArgs<double>);  // (build group 24)
extern template __global__ void mjh_postcon_kernel<float>(PostconArgs<float>);
extern template __global__ void mjh_consens_kernel<double>(ConSensArgs<double>);  // (build group 25)
extern template __global__ void mjh_consens_kernel<float>(ConSensArgs<float>);
extern template __global__ void mjh_energy_kernel<double>(EnergyArgs<double>);  // (build group 26)
extern template __global__ void mjh_energy_kernel<float>(EnergyArgs<float>);
extern template __global__ void mjh_jac_matrix_kernel<double>(JacArgs<double>);  // (build group 28)
extern template __global__ void mjh_jac_matrix_kernel<float>(JacArgs<float>);
extern template __global__ void mjh_jac_product_kernel<double>(JacArgs<double>);
extern template __global__ void mjh_jac_product_kernel<float>(JacArgs<float>);
extern template __global__ void mjh_integrate_kernel<double>(IntegrateArgs<double>);  // (build group 27)
extern template __global__ void mjh_integrate_kernel<float>(IntegrateArgs<float>);
#define SM_(R)                                                                                  \
  extern template __global__ void mjh_smooth_kernel<R, MJH_SMOOTH_COM_POS>(SmoothArgs<R>);         \
  extern template __global__ void mjh_smooth_kernel<R, MJH_SMOOTH_CRB>(SmoothArgs<R>);             \
  extern template __global__ void mjh_smooth_kernel<R, MJH_SMOOTH_TENDON_ARMATURE>(SmoothArgs<R>); \
  extern template __global__ void mjh_smooth_kernel<R, MJH_SMOOTH_FACTOR_M>(SmoothArgs<R>);        \
  extern template __global__ void mjh_smooth_kernel<R, MJH_SMOOTH_COM_VEL>(SmoothArgs<R>);         \
  extern template __global__ void mjh_smooth_kernel<R, MJH_SMOOTH_RNE>(SmoothArgs<R>);
SM_(double)  // (build group 37)
SM_(float)
#undef SM_
#define DY_(R)                                                                                    \
  extern template __global__ void mjh_dynamics_kernel<R, MJH_DYNAMICS_TENDON>(DynArgs<R>);        \
  extern template __global__ void mjh_dynamics_kernel<R, MJH_DYNAMICS_TRANSMISSION>(DynArgs<R>);  \
  extern template __global__ void mjh_dynamics_kernel<R, MJH_DYNAMICS_VELOCITY>(DynArgs<R>);      \
  extern template __global__ void mjh_dynamics_kernel<R, MJH_DYNAMICS_PASSIVE>(DynArgs<R>);       \
  extern template __global__ void mjh_dynamics_kernel<R, MJH_DYNAMICS_ACTUATION>(DynArgs<R>);     \
  extern template __global__ void mjh_dynamics_kernel<R, MJH_DYNAMICS_ACCELERATION>(DynArgs<R>);
DY_(double)  // (build group 38)
DY_(float)
#undef DY_
extern template __global__ void mjh_quadric_kernel<double>(KArgs<double>);  // (build group 29)
extern template __global__ void mjh_quadric_kernel<float>(KArgs<float>);
extern template __global__ void mjh_ifd_perturb_kernel<double>(FdPerturbArgs<double>);  // (build group 30)
extern template __global__ void mjh_ifd_perturb_kernel<float>(FdPerturbArgs<float>);
extern template __global__ void mjh_ifd_difference_kernel<double>(IfdDiffArgs<double>);
extern template __global__ void mjh_ifd_difference_kernel<float>(IfdDiffArgs<float>);
extern template __global__ void mjh_geomdist_kernel<double>(GeomDistArgs<double>);  // (build group 31)
extern template __global__ void mjh_geomdist_kernel<float>(GeomDistArgs<float>);
extern template __global__ void mjh_qpos_arith_kernel<double>(QposArithArgs<double>);  // (build group 32)
extern template __global__ void mjh_qpos_arith_kernel<float>(QposArithArgs<float>);
#define IK_(R)                                                                  \
  extern template __global__ void mjh_ik_site_kernel<R, 1>(IkSiteArgs<R>);      \
  extern template __global__ void mjh_ik_site_kernel<R, 2>(IkSiteArgs<R>);      \
  extern template __global__ void mjh_ik_site_kernel<R, 3>(IkSiteArgs<R>);
IK_(double)
IK_(float)
#undef IK_
#define EFC_(R)                                                               \
  extern template __global__ void mjh_efc_mulj_kernel<R>(EfcArgs<R>);         \
  extern template __global__ void mjh_efc_muljt_kernel<R>(EfcArgs<R>);        \
  extern template __global__ void mjh_efc_update_kernel<R>(EfcArgs<R>);       \
  extern template __global__ void mjh_efc_ar_kernel<R>(EfcArgs<R>);
EFC_(double)  // (build group 33)
EFC_(float)
#undef EFC_
extern template __global__ void mjh_pgs_kernel<double>(PgsArgs<double>);  // (build group 34)
extern template __global__ void mjh_pgs_kernel<float>(PgsArgs<float>);
extern template __global__ void mjh_solve_kernel<double>(SolveArgs<double>);  // (build group 36)
extern template __global__ void mjh_solve_kernel<float>(SolveArgs<float>);
extern template __global__ void mjh_noslip_kernel<double>(NoslipArgs<double>);  // (build group 35)
extern template __global__ void mjh_noslip_kernel<float>(NoslipArgs<float>);
#undef X_
#undef S_
#undef C_
#undef N_

template <typename REAL> using Kernel = void (*)(KArgs<REAL>);
// the register solver's instantiations (mjh_instances.h): NMAX, RPL, form (sol2_form), kernel
template <typename REAL> struct Sol2Kernel { int nmax, rpl, wt; Kernel<REAL> fn; };
#define NONE_(...)
#define S_(R, N, RPL, WT) {N, RPL, WT, &mjh_sol2_kernel<R, N, RPL, WT>},
template <typename REAL> const Sol2Kernel<REAL> kSol2Kernels[] = {MJH_INST_ALL(NONE_, S_, NONE_, NONE_, REAL)};
#undef NONE_
#undef S_
template <typename REAL>
Kernel<REAL> sol2_kernel(int nmax, int rpl, int wt) {
  for (const Sol2Kernel<REAL>& k : kSol2Kernels<REAL>) if (k.nmax == nmax && k.rpl == rpl && k.wt == wt) return k.fn;
  return nullptr;
}

static thread_local std::string g_err;
static unsigned long long* g_stamps = nullptr;  // diagnostic builds only (mjh_debug_set_stamps)
static int fail(int code, const std::string& msg) { g_err = msg; return code; }

// ---- per-launch timing (mjh_debug_phase_timing): HIP events on the launch stream around every kernel of a call ----------------
#define MJH_TIMING_MAX 96
static struct {
  bool on = false;
  int n = 0;                          // launches recorded by the last call
  int id[MJH_TIMING_MAX];             // MJH_KERNEL_* (include/mjhip.h)
  hipEvent_t ev[MJH_TIMING_MAX + 1];  // ev[i] .. ev[i + 1] brackets launch i
} g_timing;
static inline void timing_begin(hipStream_t s) { if (g_timing.on) { g_timing.n = 0; (void)hipEventRecord(g_timing.ev[0], s); } }
static inline void timing_mark(hipStream_t s, int id) {
  if (g_timing.on && g_timing.n < MJH_TIMING_MAX) { g_timing.id[g_timing.n] = id; g_timing.n++; (void)hipEventRecord(g_timing.ev[g_timing.n], s); }
}
#define HIP_TRY(x)                                                                                         \
  do {                                                                                                     \
    hipError_t e_ = (x);                                                                                   \
    if (e_ != hipSuccess) return fail(-5, std::string(#x) + ": " + hipGetErrorString(e_));                 \
  } while (0)

// The LDS arenas of a model: the five pipeline phases and the register solver (carved as lds_carve(M, 1 << arena)), then those of the fused kernels and of the
// register solver's first tier.
enum Arena { AR_KIN, AR_CRB, AR_CON, AR_VEL, AR_SOL, AR_SOL2, AR_KV, AR_KCV, AR_KCV2, AR_TIER, AR_CS, AR_COUNT };
static_assert(AR_SOL2 + 1 == MJH_NARENA, "the arenas carved per model come first");
struct ArenaLds {
  LdsOff off;  // offsets of the arena's arrays
  int bytes;   // ... and its size per environment
};

// A real Data leaf in the RK4 stage workspace: not there, there with its slot in the stage Data, or there with the slot left NULL (the space is still taken)
enum StageLeaf : unsigned char { STAGE_NONE, STAGE_SLOT, STAGE_SPACE };

struct mjhModel {
  int dtype;
  void* blob;          // device allocation holding every table
  size_t blob_bytes;
  ArenaLds arena[AR_COUNT] = {};
  int lds(Arena a) const { return arena[a].bytes; }
  int pack2[AR_COUNT] = {};                // the phase kernels on an arena (phase_kernel) run two environments per wavefront
  int pack4[AR_COUNT] = {};                // ... or four (16 lanes each): small models only
  int sol2_nmax = 0, sol2_rpl = 0;         // register solver (mjh_sol2_kernel) instantiation serving this model, 0 = not eligible
  int fuse_kv = 0;                         // kinematics + velocity phases run as ONE kernel (MJH_KERNEL_KV) from an arena of their own
  int fuse_kcv = 0;                        // ... and the crb / factor stage between them: ONE kernel (MJH_KERNEL_KCV) for the three (models whose crb stage packs like the other two)
  int kcv2 = 0;                            // a step launches the two-wave form (MJH_KERNEL_KCV2) instead of MJH_KERNEL_KCV ...
  int64_t kcv2_max_envs = 0;               // ... forced on (MJH_KCV2=1): any batch; otherwise 0 and the limit is kcv2_limit() of the LAUNCH's device
  int kcv2_per_wg = 0, kcv2_envs_per_wg = 0; // arena bytes and environments of one of its workgroups
  int sol2_tiers = 0;                      // 1: a first launch with ONE row slot per lane serves the environments whose active contacts fit 32 dense rows
  int sol2_w16_rpl = 0;                    // > 0: that first launch runs FOUR environments per wavefront (16 lanes each, nv <= 16) with this many row slots per lane
  int sol2_w16_nmax = 0;                   // ... instantiated for 8, 12 or 16 dofs; the first tier runs from an arena of its own (AR_TIER: 32 rows of efc_J instead of all of them)
  int fuse_all = 0;                        // ... and the whole pass as ONE kernel (SOL2_PASS, MJH_KERNEL_PASS): kernel 13's stages in front of kernel 14's, one arena of max(AR_KCV, AR_CS)
  int lds_all = 0;
  int inv_lanes = 0, inv_envs = 0, inv_chunk = 0, inv_lds_env = 0;  // inverse-dynamics tail (mjh_inverse_kernel): lanes per environment, environments per workgroup, rows per LDS chunk, REALs per environment
  int pc_lanes = 0, pc_envs = 0, pc_lds_env = 0;  // body accelerations and forces (mjh_postcon_kernel): lanes per environment, environments per workgroup, REALs per environment; pc_envs == 0: the model does not fit
  int cs_lds_env = 0, cs_ok = 0;  // contact forces and their sensors (mjh_consens_kernel): REALs per environment (a multiple of 4); cs_ok == 0: the model's contacts do not fit
  int any_damping = 0;                     // some dof_damping != 0 (discrete_acc's eulerdamp re-solve applies)
  int fuse_stage = 0;                      // every RK4 stage of a small Newton model runs as ONE launch (SOL2_STAGE, MJH_KERNEL_STAGE; stage 0 too unless MJH_FUSE_STAGE0=0): kernel 13's stages, the constraint phase (kernel 8) and the register solver's first tier
  int lds_stage = 0;                       // ... dynamic LDS of one of its four-environment workgroups
  int fuse_tail = 0;                       // the tail of a pass -- constraint phase + the solver's first tier + integrator -- as ONE launch of the same kernel (parts 2 | 4): small Newton models whose pass cannot be one launch (convex narrow phase or sensors between the parts, Euler)
  int lds_tail = 0;
  int fuse_cs = 0;                         // constraint stage + register solver + integrator run as ONE kernel (SOL2_CS, MJH_KERNEL_CS) from an arena of its own
  int cvx_lds_bytes;                       // LDS scratch of one (environment, convex pair) wave
  int ncvx = 0, nquad = 0;                 // DevModel::cvx_pairs lists every pair narrow-phased outside the pass kernels (ncvxpair of them): first the ncvx box / mesh pairs of mjh_convex_kernel, then the nquad plane-ellipsoid / plane-cylinder pairs of mjh_quadric_kernel
  int64_t work_reals;                      // per-environment REALs of workspace: RK4 stage Data and sums + the convex candidates of max_contact_points (0 for most Euler models)
  int64_t hs_reals = 0;                    // ... of which the constraint phase's hand-over to the register solver (KArgs::hs): small models with one contact condim
  int64_t cand_reals = 0;                  // ... of which the candidate contacts (at the HEAD of the workspace: its first B * cand_reals reals; the RK4 stage Data and sums follow)
  std::vector<int64_t> leaf_count;         // per-env element count of every real Data leaf, ABI order
  std::vector<StageLeaf> stage_leaf;       // ... and its part in the RK4 stage workspace (RK4 models)
  DevModel<double> m64;
  DevModel<float> m32;
};

namespace {

// What the host knows of each phase kernel (mjh_phase_kernel<REAL, id, W>): the arena it runs from, the arena whose packing flags (mjhModel::pack2 / pack4) say
// whether it runs two / four environments per wavefront, and the most environments per wavefront it is instantiated for (mjh_instances.h).  Its threads per
// workgroup: phase_threads (mjh_kernels.h).
struct PhaseKernel { Arena arena, pack; int max_envs; };
constexpr PhaseKernel phase_kernel(int id) {
  switch (id) {
    case MJH_KERNEL_KIN: return {AR_KIN, AR_KIN, 4};
    case MJH_KERNEL_CRB: return {AR_CRB, AR_CRB, 4};
    case MJH_KERNEL_CON: return {AR_CON, AR_CON, 1};
    case MJH_KERNEL_VEL: return {AR_VEL, AR_VEL, 4};
    case MJH_KERNEL_SOL: return {AR_SOL, AR_SOL, 1};
    case MJH_KERNEL_VEL_OPT: return {AR_VEL, AR_VEL, 4};           // (the velocity phase's arena and packing)
    case MJH_KERNEL_SOL_GEN: return {AR_SOL, AR_SOL, 1};
    case MJH_KERNEL_CON_GEN: return {AR_CON, AR_CON, 1};
    case MJH_KERNEL_CON_DIRECT: return {AR_CON, AR_CON, 2};        // never four per wavefront
    case MJH_KERNEL_KV: return {AR_KV, AR_KV, 4};
    case MJH_KERNEL_KCV: return {AR_KCV, AR_CRB, 4};               // (fuse_kcv holds only when the crb stage packs like the other two)
    case MJH_KERNEL_KCV2: return {AR_KCV2, AR_CRB, 4};
  }
  return {AR_COUNT, AR_COUNT, 0};
}

// lets launches of `kernel` take `bytes` of dynamic LDS
template <typename F>
hipError_t allow_lds(F* kernel, int bytes) {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
}
// ... for a phase kernel at W lanes per environment: its arena for each of the MJH_WAVE / W environments of a workgroup
template <typename REAL, int P, int W>
hipError_t allow_phase_lds(const mjhModel* m) {
  return allow_lds(&mjh_phase_kernel<REAL, P, W>, MJH_WAVE / W * m->lds(phase_kernel(P).arena));
}
// ... at every width launch_phase runs it at: one environment per wavefront, and two / four where the packing flags of its arena say so
template <typename REAL, int P>
hipError_t allow_phase_lds_packed(const mjhModel* m) {
  constexpr PhaseKernel K = phase_kernel(P);
  hipError_t e = allow_phase_lds<REAL, P, MJH_WAVE>(m);
  if constexpr (K.max_envs > 1) if (!e && m->pack2[K.pack]) e = allow_phase_lds<REAL, P, 32>(m);
  if constexpr (K.max_envs == 4) if (!e && m->pack4[K.pack]) e = allow_phase_lds<REAL, P, 16>(m);
  return e;
}
// ... for every instantiation of register-solver form `wt`
template <typename REAL>
hipError_t allow_sol2_lds(int wt, int bytes) {
  for (const Sol2Kernel<REAL>& k : kSol2Kernels<REAL>)
    if (k.wt == wt)
      if (const hipError_t e = allow_lds(k.fn, bytes)) return e;
  return hipSuccess;
}

struct BlobBuilder {
  std::vector<unsigned char> host;
  size_t add(const void* p, size_t bytes) {
    size_t off = (host.size() + 15) & ~size_t(15);
    host.resize(off + bytes);
    if (bytes) memcpy(host.data() + off, p, bytes);
    return off;
  }
};

std::vector<int64_t> leaf_counts(const mjhModelDesc* m) {
  const int64_t nq = m->nq, nv = m->nv, nu = m->nu, na = m->na, nb = m->nbody, nj = m->njnt, ng = m->ngeom;
  const int64_t ncon = m->ncon, nefc = m->nefc;
  std::vector<int64_t> v;
#define F(n, c) v.push_back(c);
  F(time, 1) F(qpos, nq) F(qvel, nv) F(act, na) F(qacc_warmstart, nv) F(ctrl, nu) F(qfrc_applied, nv)
  F(xfrc_applied, nb * 6) F(mocap_pos, m->nmocap * 3) F(mocap_quat, m->nmocap * 4) F(qacc, nv) F(act_dot, na)
  F(xpos, nb * 3) F(xquat, nb * 4) F(xmat, nb * 9) F(xipos, nb * 3) F(ximat, nb * 9) F(xanchor, nj * 3) F(xaxis, nj * 3)
  F(geom_xpos, ng * 3) F(geom_xmat, ng * 9) F(site_xpos, m->nsite * 3) F(site_xmat, m->nsite * 9)
  F(cam_xpos, m->ncam * 3) F(cam_xmat, m->ncam * 9) F(light_xpos, m->nlight * 3) F(light_xdir, m->nlight * 3)
  F(subtree_com, nb * 3) F(cdof, nv * 6) F(cinert, nb * 10) F(crb, nb * 10) F(ten_length, m->ntendon) F(ten_J, m->ntendon * nv) F(ten_velocity, m->ntendon) F(actuator_length, nu)
  F(actuator_moment, nu * nv) F(qM, nv * nv) F(qLD, nv * nv) F(contact_dist, ncon) F(contact_pos, ncon * 3)
  F(contact_frame, ncon * 9) F(contact_includemargin, ncon) F(contact_friction, ncon * 5) F(contact_solref, ncon * 2)
  F(contact_solreffriction, ncon * 2) F(contact_solimp, ncon * 5) F(sensordata, m->nsensordata) F(efc_J, nefc * nv) F(efc_frictionloss, nefc)
  F(efc_D, nefc) F(efc_aref, nefc) F(efc_force, nefc) F(actuator_velocity, nu) F(cvel, nb * 6) F(cdof_dot, nv * 6)
  F(qfrc_bias, nv) F(qfrc_passive, nv) F(qfrc_gravcomp, nv) F(actuator_force, nu) F(qfrc_actuator, nv) F(qfrc_smooth, nv)
  F(qacc_smooth, nv) F(qfrc_constraint, nv)
#undef F
  return v;
}

// leaves an RK stage pass needs as storage between its phases (everything a forward pass writes except
// frames that no later phase reads)
const char* const kStageLeaves[] = {
    "qpos", "qvel", "act", "qacc_warmstart", "qacc", "act_dot", "xipos", "geom_xpos", "geom_xmat", "subtree_com", "cdof",
    "cinert", "qM", "qLD", "efc_J", "efc_D", "efc_aref", "qfrc_smooth", "qacc_smooth", "qfrc_constraint",
    "contact_dist" /* the solver phase picks the active contacts' rows by it */};
// ... plus, for models with convex pairs, the contact leaves the convex kernel hands to the constraint phase
const char* const kConvexStageLeaves[] = {"contact_dist", "contact_pos", "contact_frame"};
const char* const kEqStageLeaves[] = {"xpos", "xquat", "xmat"};  // body frames read by the equality rows (constraint.py:116-212)
bool is_stage_leaf(const char* name, bool has_convex, bool has_fluid, bool has_eq, bool topk) {
  if (topk && !strcmp(name, "contact_includemargin")) return true;  // per environment once max_contact_points selects: the solver phase reads it
  if (!strcmp(name, "qfrc_gravcomp") || !strncmp(name, "ten_", 4)) return false;  // tendon quantities are recomputed from qpos where they are used  // staged in LDS inside the velocity phase; the leaf itself is written by stage 0 only
  if (has_eq) for (const char* s : kEqStageLeaves) if (!strcmp(s, name)) return true;
  for (const char* s : kStageLeaves) if (!strcmp(s, name)) return true;
  if (has_convex) for (const char* s : kConvexStageLeaves) if (!strcmp(s, name)) return true;
  if (has_fluid && !strcmp(name, "ximat")) return true;  // the fluid model needs the inertial frames of the stage (passive.py:31-78)
  return false;
}

// The library's environment switches: measurement aids, each turning a measured default the other way.  Read once, at the first model creation.
bool on(const char* e) { return !(e && e[0] == '0'); }                              // unset, or anything but "0...": on
int tri(const char* e) { return !e ? -1 : (e[0] == '1' ? 1 : 0); }                  // -1: unset (the default), 1: forced on, 0: off
int mask12(const char* e) { return e ? (int)(strtol(e, nullptr, 0) & 0xfff) : -1; }  // 12 bits of the workgroup index; -1: unset
int num(const char* e, int unset) { return e ? atoi(e) : unset; }
struct Switches {
  bool all_handoff = on(getenv("MJH_ALL_HANDOFF"));
  bool lds_diet = on(getenv("MJH_LDS_DIET"));
  bool pair_cull = on(getenv("MJH_PAIR_CULL"));
  bool kin_level = on(getenv("MJH_KIN_LEVEL"));
  bool sol2_mfma = on(getenv("MJH_SOL2_MFMA"));
  bool sol2_incr = on(getenv("MJH_SOL2_INCR"));
  bool handover = on(getenv("MJH_HANDOVER"));
  int kcv2 = tri(getenv("MJH_KCV2"));
  int fuse_all = tri(getenv("MJH_FUSE_ALL"));
  bool fuse_stage = on(getenv("MJH_FUSE_STAGE"));
  bool fuse_stage0 = on(getenv("MJH_FUSE_STAGE0"));
  bool fuse_tail = on(getenv("MJH_FUSE_TAIL"));
  bool cs_one = on(getenv("MJH_CS_ONE"));
  int xswap = mask12(getenv("MJH_XSWAP"));  // (an explicit mask applies at every launch size: the bit-identity tests)
  int xswap_k = mask12(getenv("MJH_XSWAP_K"));
  int xswap_c = mask12(getenv("MJH_XSWAP_C"));
  int sensor_epw = num(getenv("MJH_SENSOR_EPW"), 0);  // 0: auto
  int max_grid_log2 = std::min(std::max(num(getenv("MJH_MAX_GRID_LOG2"), 20), 0), 20);
};
const Switches& switches() {
  static const Switches s;
  return s;
}

constexpr int kLdsCu = 160 * 1024;  // the LDS of one CU: the most one workgroup can take (a phase keeps 160 KB / arena environments of a CU in flight: profiles/r01/notes.md)
constexpr int kLdsWg = 64 * 1024;   // the most dynamic LDS per workgroup the packed, fused and solver forms are planned for (each form's test of whether it serves a model)

// carves `arena` for phase bit `phase_bit` from the flags of M (the model's DevModel, or a copy of it with the register solver's first-tier row cap); returns its bytes per environment
template <typename REAL>
int carve(mjhModel* out, Arena arena, const DevModel<REAL>& M, int phase_bit, int* kv_defer_ok = nullptr) {
  ArenaLds& ar = out->arena[arena];
  return ar.bytes = lds_carve(M, phase_bit, ar.off, kv_defer_ok) * (int)sizeof(REAL);
}

using Fixups = std::vector<std::pair<const void**, size_t>>;  // (pointer slot of DevModel, offset in the blob)

// ---- tables: the model copied into DevModel and the blob, and the topology, row, transmission and sensor tables derived from it (no kernel choice) ----
template <typename REAL>
int tables(const mjhModelDesc* d, mjhModel* out, DevModel<REAL>& M, BlobBuilder& bb, Fixups& fix) {
  memset(&M, 0, sizeof(M));
#define X(n) M.n = d->n;
  MJH_MODEL_INTS(X)
#undef X
  M.timestep = (REAL)d->timestep;
  M.impratio = (REAL)d->impratio;
  M.density = (REAL)d->density; M.viscosity = (REAL)d->viscosity;
  M.wind[0] = (REAL)d->wind_x; M.wind[1] = (REAL)d->wind_y; M.wind[2] = (REAL)d->wind_z;
  M.magnetic[0] = (REAL)d->magnetic_x; M.magnetic[1] = (REAL)d->magnetic_y; M.magnetic[2] = (REAL)d->magnetic_z;
  M.has_fluid = (d->density > 0) || (d->viscosity > 0) || (d->wind_x != 0) || (d->wind_y != 0) || (d->wind_z != 0);
  M.con_general = (d->nf > 0 || d->nft > 0 || d->ne > 0 || d->nlb > 0 || d->nlt > 0 || d->topk) ? 1 : 0;
  if (d->nft > 0 && d->nf + d->nl + d->nft > 64) return fail(-38, "frictionloss rows beyond the first 64 solver rows are not supported");
  for (int b = 0; b < d->nbody; b++) if (d->body_gravcomp[b] != 0) M.has_gravcomp = 1;
  M.gravity[0] = (REAL)d->gravity_x; M.gravity[1] = (REAL)d->gravity_y; M.gravity[2] = (REAL)d->gravity_z;
  M.meaninertia = d->meaninertia; M.tolerance = d->tolerance; M.ls_tolerance = d->ls_tolerance;
#define X(n) fix.push_back({(const void**)&M.n, bb.add(d->n, sizeof(int32_t) * (size_t)d->len_##n)});
  MJH_MODEL_INT_ARRAYS(X)
#undef X
#define X(n)                                                                                   \
  {                                                                                            \
    std::vector<REAL> tmp((size_t)d->len_##n);                                                 \
    for (size_t i = 0; i < tmp.size(); i++) tmp[i] = (REAL)d->n[i];                            \
    fix.push_back({(const void**)&M.n, bb.add(tmp.data(), sizeof(REAL) * tmp.size())});        \
  }
  MJH_MODEL_REAL_ARRAYS(X)
#undef X
  // ---- derived topology tables ----
  const int nb = d->nbody, nv = d->nv;
  if (nv > 256) return fail(-22, "nv must be <= 256 (inertia-matrix pair table packs two 8-bit dof indices)");
  const int NW = nv > 64 ? (nv + 63) / 64 : 1;  // 64-bit words per dof mask
  M.mask_words = NW;
  M.big = nv > 64 ? 1 : 0;
  if (M.big) M.con_general = 1;  // the general constraint kernel (7) reads multi-word masks; so does the optional-physics velocity kernel (5)
  std::vector<int> depth(nb, 0), sub_end(nb, 0);
  int max_depth = 1;
  for (int b = 1; b < nb; b++) {
    if (d->body_parentid[b] >= b) return fail(-22, "bodies must be ordered parent-before-child");
    depth[b] = depth[d->body_parentid[b]] + 1;
    if (depth[b] > max_depth) max_depth = depth[b];
  }
  if (max_depth > MJH_MAX_DEPTH) return fail(-22, "kinematic tree deeper than MJH_MAX_DEPTH");
  std::vector<int> chain((size_t)nb * max_depth, 0);
  for (int b = 1; b < nb; b++) {
    int c = b;
    for (int k = depth[b] - 1; k >= 0; k--) { chain[(size_t)b * max_depth + k] = c; c = d->body_parentid[c]; }
  }
  for (int b = nb - 1; b >= 0; b--) {
    if (sub_end[b] < b + 1) sub_end[b] = b + 1;
    if (b > 0) { int p = d->body_parentid[b]; if (sub_end[p] < sub_end[b]) sub_end[p] = sub_end[b]; }
  }
  for (int b = 1; b < nb; b++)  // DFS order check: every body in [b, sub_end[b]) must descend from b
    for (int c = b + 1; c < sub_end[b]; c++) {
      int a = c;
      while (a > b) a = d->body_parentid[a];
      if (a != b) return fail(-22, "bodies are not in depth-first order");
    }
  std::vector<unsigned long long> body_dofmask((size_t)nb * NW, 0ull), dof_ancmask((size_t)nv * NW, 0ull);
  auto anc = [&](int i, int j) { return (dof_ancmask[(size_t)i * NW + (j >> 6)] >> (j & 63)) & 1ull; };
  for (int dd = 0; dd < nv; dd++) {
    int a = dd;
    while (a >= 0) { dof_ancmask[(size_t)dd * NW + (a >> 6)] |= 1ull << (a & 63); a = d->dof_parentid[a]; }
  }
  for (int b = 0; b < nb; b++) {
    int a = b;
    while (a > 0) {
      for (int dd = 0; dd < nv; dd++) if (d->dof_bodyid[dd] == a) body_dofmask[(size_t)b * NW + (dd >> 6)] |= 1ull << (dd & 63);
      a = d->body_parentid[a];
    }
  }
  {  // lower-triangle entries (i, j) of qM whose dofs are on one ancestor path (support.make_m :50-80 masks the rest to zero)
    std::vector<int> pairs;
    for (int i = 0; i < nv; i++)
      for (int j = 0; j <= i; j++)
        if (anc(i, j)) pairs.push_back((i << 8) | j);
    M.nqmpair = (int)pairs.size();
    std::vector<int> slot((size_t)nv * nv, -1);
    for (int pk : pairs) {
      const int i = pk >> 8, j = pk & 0xff, sl = (i * (i + 1)) / 2 + j;
      slot[(size_t)i * nv + j] = sl;
      slot[(size_t)j * nv + i] = sl;
    }
    {  // tendon armature couples dofs of different branches: every entry of qM can be non-zero then
      bool arm = false;
      for (int t = 0; t < d->ntendon; t++) arm = arm || d->tendon_armature[t] != 0;
      if (arm)
        for (int i = 0; i < nv; i++)
          for (int j = 0; j <= i; j++) { slot[(size_t)i * nv + j] = (i * (i + 1)) / 2 + j; slot[(size_t)j * nv + i] = (i * (i + 1)) / 2 + j; }
    }
    fix.push_back({(const void**)&M.qm_slot, bb.add(slot.data(), sizeof(int) * slot.size())});
    fix.push_back({(const void**)&M.qm_pair, bb.add(pairs.data(), sizeof(int) * pairs.size())});
  }
  std::vector<int> row_con((size_t)d->nefc, -1);
  for (int c = 0; c < d->ncon; c++) {
    int dim = d->con_dim[c];
    int rows = dim == 1 ? 1 : (d->cone == CONE_ELLIPTIC ? dim : 2 * (dim - 1));
    for (int r = 0; r < rows; r++) {
      int row = d->con_efc_address[c] + r;
      if (row < 0 || row >= d->nefc) return fail(-22, "contact row address out of range");
      row_con[row] = c;
    }
  }
  {  // per-row / per-contact tables of the plain constraint phase (DevModel::crow_par ...).  The arithmetic is the kernel's own, in REAL, in
     // the same order (constraint.py:440-451, 480-487, 547-561): the values are bit-identical to what each lane used to recompute.
    const int first = d->nefc - [&] { int n = 0; for (int r = 0; r < d->nefc; r++) n += row_con[r] >= 0; return n; }();
    int ncrow = d->nefc - first;
    for (int r = first; r < d->nefc; r++) if (row_con[r] < 0) ncrow = -1;  // contact rows must close the row order
    if (ncrow < 0 || d->topk) ncrow = 0;
    M.ncrow = ncrow;
    M.con_rows = 0;
    for (int c = 0; c < d->ncon; c++) {
      const int dim = d->con_dim[c], rows = dim == 1 ? 1 : (d->cone == CONE_ELLIPTIC ? dim : 2 * (dim - 1));
      if (c == 0) M.con_rows = rows; else if (rows != M.con_rows) { M.con_rows = 0; break; }
    }
    M.crow_by_con = (M.con_rows > 0 && ncrow == d->ncon * M.con_rows) ? 1 : 0;
    for (int c = 0; c < d->ncon && M.crow_by_con; c++) if (d->con_efc_address[c] != first + c * M.con_rows) M.crow_by_con = 0;
    const bool elliptic = d->cone == CONE_ELLIPTIC;
    std::vector<REAL> par((size_t)9 * (ncrow > 0 ? ncrow : 1), (REAL)0);
    std::vector<int> info((size_t)(ncrow > 0 ? ncrow : 1), 0);
    for (int q = 0; q < ncrow; q++) {
      const int c = row_con[first + q], sub = first + q - d->con_efc_address[c], dim = d->con_dim[c];
      REAL sr0 = (REAL)d->con_solref[2 * c], sr1 = (REAL)d->con_solref[2 * c + 1];
      if (elliptic && dim > 1 && sub > 0) {
        const REAL sf0 = (REAL)d->con_solreffriction[2 * c], sf1 = (REAL)d->con_solreffriction[2 * c + 1];
        const REAL none = (REAL)(!((sf0 != 0) || (sf1 != 0)));
        sr0 = sf0 + sr0 * none; sr1 = sf1 + sr1 * none;
      }
      REAL fric[5];
      for (int i = 0; i < 5; i++) fric[i] = (REAL)d->con_friction[5 * c + i];
      const REAL t = (REAL)d->body_invweight0[d->geom_bodyid[d->con_geom1[c]]] + (REAL)d->body_invweight0[d->geom_bodyid[d->con_geom2[c]]];
      REAL invweight;
      if (dim == 1) invweight = t;
      else if (!elliptic) { const REAL mu = fric[0]; invweight = (t + mu * mu * t) * 2 * mu * mu / M.impratio; }
      else { const REAL iwf = t / M.impratio; invweight = (sub == 0) ? t : (sub == 1 ? iwf : iwf * ((fric[0] * fric[0]) / (fric[sub - 1] * fric[sub - 1]))); }
      par[(size_t)0 * ncrow + q] = sr0; par[(size_t)1 * ncrow + q] = sr1;
      for (int i = 0; i < 5; i++) par[(size_t)(2 + i) * ncrow + q] = (REAL)d->con_solimp[5 * c + i];
      par[(size_t)7 * ncrow + q] = invweight;
      par[(size_t)8 * ncrow + q] = (REAL)d->con_includemargin[c];
      info[q] = c | (sub << 16) | ((elliptic && dim > 1) ? (1 << 24) : 0);
    }
    fix.push_back({(const void**)&M.crow_par, bb.add(par.data(), sizeof(REAL) * par.size())});
    fix.push_back({(const void**)&M.crow_info, bb.add(info.data(), sizeof(int) * info.size())});
    std::vector<int> cbody((size_t)4 * (d->ncon > 0 ? d->ncon : 1), 0);
    std::vector<unsigned long long> cmask((size_t)2 * (d->ncon > 0 ? d->ncon : 1), 0ull);
    for (int c = 0; c < d->ncon; c++) {
      const int b1 = d->geom_bodyid[d->con_geom1[c]], b2 = d->geom_bodyid[d->con_geom2[c]];
      cbody[4 * c] = b1; cbody[4 * c + 1] = b2; cbody[4 * c + 2] = d->body_rootid[b1]; cbody[4 * c + 3] = d->body_rootid[b2];
      cmask[2 * c] = body_dofmask[(size_t)b1 * NW]; cmask[2 * c + 1] = body_dofmask[(size_t)b2 * NW];  // (first word: the table serves the small-model kernel only)
    }
    fix.push_back({(const void**)&M.con_body, bb.add(cbody.data(), sizeof(int) * cbody.size())});
    fix.push_back({(const void**)&M.con_dmask, bb.add(cmask.data(), sizeof(unsigned long long) * cmask.size())});
    // bounding-sphere reach of the sphere / capsule pairs (collision(): the cull ahead of the narrow phase in RK4 stages 1..3)
    std::vector<REAL> pcull((size_t)2 * (d->npair > 0 ? d->npair : 1), (REAL)-1);
    for (int p = 0; p < d->npair; p++) {
      const int fn = d->pair_fn[p], g1 = d->pair_geom1[p], g2 = d->pair_geom2[p];
      if (fn != MJH_FN_SPHERE_SPHERE && fn != MJH_FN_SPHERE_CAPSULE && fn != MJH_FN_CAPSULE_CAPSULE) continue;
      const double r1 = d->geom_size[3 * g1] + (fn == MJH_FN_CAPSULE_CAPSULE ? d->geom_size[3 * g1 + 1] : 0.0);
      const double r2 = d->geom_size[3 * g2] + (fn == MJH_FN_SPHERE_SPHERE ? 0.0 : d->geom_size[3 * g2 + 1]);
      double margin = 0;
      for (int q = 0; q < d->pair_ncon[p] && q < MJH_MAX_PAIR_CONTACTS; q++) margin = std::max(margin, (double)d->con_includemargin[d->pair_dst[p * MJH_MAX_PAIR_CONTACTS + q]]);
      const double reach = (r1 + r2 + margin) * 1.01 + 1e-3;
      pcull[2 * p] = (REAL)(reach * reach); pcull[2 * p + 1] = (REAL)(r1 + r2);
    }
    fix.push_back({(const void**)&M.pair_cull, bb.add(pcull.data(), sizeof(REAL) * pcull.size())});
  }
  {
    int max_jnt = 1;
    for (int b = 0; b < nb; b++) if (d->body_jntnum[b] > max_jnt) max_jnt = d->body_jntnum[b];
    std::vector<int> chain_dof((size_t)nb * max_depth, 0), chain_jnt((size_t)nb * max_depth * max_jnt, 0);
    for (int b = 1; b < nb; b++)
      for (int k = 0; k < depth[b]; k++) {
        const int c = chain[(size_t)b * max_depth + k];
        chain_dof[(size_t)b * max_depth + k] = d->body_dofadr[c] < 0 ? 0 : (d->body_dofadr[c] | (d->body_dofnum[c] << 16));
        for (int jj = 0; jj < d->body_jntnum[c]; jj++) {
          const int j = d->body_jntadr[c] + jj;
          chain_jnt[((size_t)b * max_depth + k) * max_jnt + jj] = (d->jnt_type[j] + 1) | (d->jnt_dofadr[j] << 8);
        }
      }
    M.max_jnt = max_jnt;
    fix.push_back({(const void**)&M.chain_dof, bb.add(chain_dof.data(), sizeof(int) * chain_dof.size())});
    fix.push_back({(const void**)&M.chain_jnt, bb.add(chain_jnt.data(), sizeof(int) * chain_jnt.size())});
  }
  fix.push_back({(const void**)&M.body_depth, bb.add(depth.data(), sizeof(int) * nb)});
  fix.push_back({(const void**)&M.body_chain, bb.add(chain.data(), sizeof(int) * chain.size())});
  fix.push_back({(const void**)&M.body_subtree_end, bb.add(sub_end.data(), sizeof(int) * nb)});
  fix.push_back({(const void**)&M.body_dofmask, bb.add(body_dofmask.data(), sizeof(unsigned long long) * body_dofmask.size())});
  fix.push_back({(const void**)&M.efc_row_con, bb.add(row_con.data(), sizeof(int) * row_con.size())});
  {
    const int nrf = d->nsensor > 0 ? d->sns_rfadr[d->nsensor] : 0;
    std::vector<int> owner((size_t)nrf + 1, 0);
    for (int sidx = 0; sidx < d->nsensor; sidx++)
      for (int q = d->sns_rfadr[sidx]; q < d->sns_rfadr[sidx + 1]; q++) owner[q] = sidx;
    M.nrfq = nrf;
    fix.push_back({(const void**)&M.rf_sensor, bb.add(owner.data(), sizeof(int) * owner.size())});
    std::vector<int> rsite((size_t)nrf + 1, 0), rtype((size_t)nrf + 1, 0);
    std::vector<REAL> rsize((size_t)3 * nrf + 3, (REAL)0);
    for (int q = 0; q < nrf; q++) {
      const int g = d->rf_geom[q];
      rsite[q] = d->sns_objid[owner[q]]; rtype[q] = d->geom_type[g];
      for (int i = 0; i < 3; i++) rsize[3 * q + i] = (REAL)d->geom_size[3 * g + i];
    }
    fix.push_back({(const void**)&M.rf_site, bb.add(rsite.data(), sizeof(int) * rsite.size())});
    fix.push_back({(const void**)&M.rf_gtype, bb.add(rtype.data(), sizeof(int) * rtype.size())});
    fix.push_back({(const void**)&M.rf_gsize, bb.add(rsize.data(), sizeof(REAL) * rsize.size())});
    M.sns_full = 0;
    for (int sidx = 0; sidx < d->nsensor; sidx++) { const int t = d->sns_type[sidx]; if (!(t == 1 || t == 2 || t == 3 || t == 7 || t == 9 || t == 10)) M.sns_full = 1; }
  }
  {
    std::vector<int> row_eq((size_t)d->ne + 1, 0);
    for (int q = 0; q < d->neqtab; q++) {
      const int width = d->eq_kind[q] == 0 ? 3 : (d->eq_kind[q] == 1 ? 6 : 1);
      for (int k = 0; k < width && d->eq_row[q] + k < d->ne; k++) row_eq[d->eq_row[q] + k] = q;
    }
    fix.push_back({(const void**)&M.efc_row_eq, bb.add(row_eq.data(), sizeof(int) * row_eq.size())});
  }
  {
    // transmission tables (smooth.transmission :535-591): the non-zeros of every actuator's moment row, actuator-major (length /
    // velocity of an actuator) and dof-major (qfrc_actuator of a dof).  A coefficient is a model constant (gear component) except
    // for JOINTINPARENT on ball / free joints, where it is a component of the gear axis rotated into the child frame (rot >= 0).
    std::vector<REAL> tenJ((size_t)d->ntendon * nv + 1, (REAL)0);
    for (int t = 0; t < d->ntendon; t++)
      for (int q = d->ten_adr[t]; q < d->ten_adr[t + 1]; q++) tenJ[(size_t)t * nv + d->ten_dof[q]] = (REAL)d->ten_coef[q];
    fix.push_back({(const void**)&M.ten_J0, bb.add(tenJ.data(), sizeof(REAL) * tenJ.size())});
    {  // tendon armature: J^T diag(armature) J (products and sums in REAL, tendons in index order)
      std::vector<REAL> jtaj((size_t)(nv * (nv + 1)) / 2 + 1, (REAL)0);
      M.has_ten_armature = 0;
      for (int t = 0; t < d->ntendon; t++) if (d->tendon_armature[t] != 0) M.has_ten_armature = 1;
      if (M.has_ten_armature)
        for (int i = 0; i < nv; i++)
          for (int j = 0; j <= i; j++) {
            REAL sacc = 0;
            for (int t = 0; t < d->ntendon; t++) sacc += tenJ[(size_t)t * nv + i] * (tenJ[(size_t)t * nv + j] * (REAL)d->tendon_armature[t]);
            jtaj[(size_t)(i * (i + 1)) / 2 + j] = sacc;
          }
      fix.push_back({(const void**)&M.ten_JTAJ, bb.add(jtaj.data(), sizeof(REAL) * jtaj.size())});
    }
    std::vector<REAL> moment((size_t)d->nu * nv, (REAL)0);
    std::vector<int> a_adr((size_t)d->nu + 1, 0), a_dof, a_rot;
    std::vector<REAL> a_coef;
    int has_rot = 0;
    for (int i = 0; i < d->nu; i++) {
      a_adr[i] = (int)a_dof.size();
      const int jt = d->act_jnttype[i], da = d->act_dofadr[i];
      const bool inparent = d->act_trntype[i] == 1;
      if (d->act_trntype[i] == 3) {  // tendon transmission: moment row = ten_J[t] * gear[0] (smooth.py:558-561), dense row in dof order
        const int t = d->act_trnid[i];
        for (int dd = 0; dd < nv; dd++) {
          const REAL c = tenJ[(size_t)t * nv + dd] * (REAL)d->act_gear[6 * i];
          moment[(size_t)i * nv + dd] = c;
          if (tenJ[(size_t)t * nv + dd] != 0) { a_dof.push_back(dd); a_coef.push_back(c); a_rot.push_back(-1); }
        }
        continue;
      }
      const int width = jt == JNT_FREE ? 6 : (jt == JNT_BALL ? 3 : 1);
      for (int k = 0; k < width; k++) {
        const bool rot = inparent && ((jt == JNT_BALL) || (jt == JNT_FREE && k >= 3));
        a_dof.push_back(da + k);
        a_coef.push_back((REAL)d->act_gear[6 * i + k]);
        a_rot.push_back(rot ? (jt == JNT_FREE ? k - 3 : k) : -1);
        if (rot) has_rot = 1; else moment[(size_t)i * nv + da + k] = (REAL)d->act_gear[6 * i + k];
      }
    }
    a_adr[d->nu] = (int)a_dof.size();
    std::vector<int> adr((size_t)nv + 1, 0), ids, d_rot;
    std::vector<REAL> d_coef;
    for (int dd = 0; dd < nv; dd++) {
      adr[dd] = (int)ids.size();
      for (int i = 0; i < d->nu; i++)
        for (int q = a_adr[i]; q < a_adr[i + 1]; q++)
          if (a_dof[q] == dd) { ids.push_back(i); d_coef.push_back(a_coef[q]); d_rot.push_back(a_rot[q]); }
    }
    adr[nv] = (int)ids.size();
    M.act_has_rot = has_rot;
    M.act_simple = 1;
    for (int i = 0; i < d->nu; i++) if ((d->act_jnttype[i] != JNT_SLIDE && d->act_jnttype[i] != JNT_HINGE) || d->act_trntype[i] == 3) M.act_simple = 0;
    a_dof.push_back(0); a_rot.push_back(-1); a_coef.push_back(0); ids.push_back(0); d_rot.push_back(-1); d_coef.push_back(0);  // never empty
    fix.push_back({(const void**)&M.act_moment, bb.add(moment.data(), sizeof(REAL) * moment.size())});
    fix.push_back({(const void**)&M.dof_act_adr, bb.add(adr.data(), sizeof(int) * adr.size())});
    fix.push_back({(const void**)&M.dof_act_id, bb.add(ids.data(), sizeof(int) * ids.size())});
    fix.push_back({(const void**)&M.dof_act_coef, bb.add(d_coef.data(), sizeof(REAL) * d_coef.size())});
    fix.push_back({(const void**)&M.dof_act_rot, bb.add(d_rot.data(), sizeof(int) * d_rot.size())});
    fix.push_back({(const void**)&M.act_ent_adr, bb.add(a_adr.data(), sizeof(int) * a_adr.size())});
    fix.push_back({(const void**)&M.act_ent_dof, bb.add(a_dof.data(), sizeof(int) * a_dof.size())});
    fix.push_back({(const void**)&M.act_ent_coef, bb.add(a_coef.data(), sizeof(REAL) * a_coef.size())});
    fix.push_back({(const void**)&M.act_ent_rot, bb.add(a_rot.data(), sizeof(int) * a_rot.size())});
    {
      std::vector<int> flim((size_t)nv + 1, 0);
      std::vector<REAL> frange((size_t)2 * nv + 2, (REAL)0);
      for (int dd = 0; dd < nv; dd++) {
        const int j = d->dof_jntid[dd];
        flim[dd] = d->jnt_actfrclimited[j];
        frange[2 * dd] = (REAL)d->jnt_actfrcrange[2 * j]; frange[2 * dd + 1] = (REAL)d->jnt_actfrcrange[2 * j + 1];
      }
      fix.push_back({(const void**)&M.dof_frc_lim, bb.add(flim.data(), sizeof(int) * flim.size())});
      fix.push_back({(const void**)&M.dof_frc_range, bb.add(frange.data(), sizeof(REAL) * frange.size())});
    }
    M.inv_nv = nv > 0 ? 1.0f / (float)nv : 0.0f;
  }
  // single-column rows: dof-frictionloss rows (J = e_dof) first, then slide/hinge limit rows (J = +-e_dof or 0)
  const int ncr = d->nf + d->nl;
  std::vector<int> lim_dof((size_t)ncr, 0);
  for (int r = 0; r < d->nf; r++) lim_dof[r] = d->fric_dof[r];
  for (int r = 0; r < d->nl; r++) lim_dof[d->nf + r] = d->jnt_dofadr[d->lim_jnt[r]];
  fix.push_back({(const void**)&M.lim_dof, bb.add(lim_dof.data(), sizeof(int) * lim_dof.size())});
  std::vector<int> dof_limrow((size_t)2 * nv, -1);
  for (int r = 0; r < ncr; r++) {
    const int dd = lim_dof[r];
    if (dof_limrow[2 * dd] < 0) dof_limrow[2 * dd] = r;
    else if (dof_limrow[2 * dd + 1] < 0) dof_limrow[2 * dd + 1] = r;
    else return fail(-22, "more than two single-column rows on one dof");
  }
  fix.push_back({(const void**)&M.dof_limrow, bb.add(dof_limrow.data(), sizeof(int) * dof_limrow.size())});
  M.max_depth = max_depth;
  // convex pairs and the LDS scratch their wave needs (layout in mjh_convex.h)
  std::vector<int> cvx_pairs, quad_pairs;
  int cvx_reals = 0;
  for (int p = 0; p < d->npair; p++) {
    const int fn = d->pair_fn[p];
    if (fn < MJH_FN_PLANE_CONVEX) continue;
    if (fn == MJH_FN_PLANE_ELLIPSOID || fn == MJH_FN_PLANE_CYLINDER) {  // mjh_quadric_kernel (mjh_quadric.h): no tables, no LDS
      if (d->pair_ncon[p] != (fn == MJH_FN_PLANE_CYLINDER ? 3 : 1)) return fail(-22, "plane-ellipsoid pairs have one contact, plane-cylinder pairs three");
      quad_pairs.push_back(p);
      continue;
    }
    if (fn > MJH_FN_PLANE_CYLINDER) return fail(-38, "pair function not implemented");
    const int c2 = d->geom_convexid[d->pair_geom2[p]], c1 = d->geom_convexid[d->pair_geom1[p]];
    if (c2 < 0 || c2 >= d->nconvex || (fn == MJH_FN_CONVEX_CONVEX && (c1 < 0 || c1 >= d->nconvex))) return fail(-22, "convex pair without convex tables");
    int need = 0;
    if (fn == MJH_FN_PLANE_CONVEX) need = 5 * d->convex_nvert[c2];
    else if (fn == MJH_FN_CAPSULE_CONVEX) need = 6 * d->convex_nfv[c2];
    else if (fn == MJH_FN_CONVEX_CONVEX) {
      const int K = d->convex_nfv[c1] > d->convex_nfv[c2] ? d->convex_nfv[c1] : d->convex_nfv[c2];
      need = 3 * (d->convex_nvert[c1] + d->convex_nface[c1] + d->convex_nvert[c2] + d->convex_nface[c2]) + 43 * K;
    }
    if (need > cvx_reals) cvx_reals = need;
    cvx_pairs.push_back(p);
  }
  out->ncvx = (int)cvx_pairs.size();
  out->nquad = (int)quad_pairs.size();
  cvx_pairs.insert(cvx_pairs.end(), quad_pairs.begin(), quad_pairs.end());
  fix.push_back({(const void**)&M.cvx_pairs, bb.add(cvx_pairs.data(), sizeof(int) * cvx_pairs.size())});
  M.ncvxpair = (int)cvx_pairs.size();  // what the pass kernels test: contacts handed over through the contact leaves (or the candidate arrays)
  out->cvx_lds_bytes = (cvx_reals + 8) * (int)sizeof(REAL);
  if (out->cvx_lds_bytes > kLdsWg) return fail(-12, "convex hull too large for the pair kernel's LDS scratch");
  for (int i = 0; i < nv; i++) if (d->dof_damping[i] != 0) out->any_damping = 1;
  out->leaf_count = leaf_counts(d);
  return 0;
}

// ---- plan: every choice of path, arena, packing, solver tier and fusion that serves the model, and the workspace they need (no HIP call) ----
template <typename REAL>
int plan(const mjhModelDesc* d, mjhModel* out, DevModel<REAL>& M) {
  const Switches& sw = switches();
  const int nv = d->nv;
  // measured on MI355X (profiles/r02/notes.md): ant (nv 8) constraint phase 127 -> 112 us, mesh scene 58 -> 54 us; the humanoid (nv 27) is
  // slower that way (43 -> 59 us: every (contact, dof) lane re-reads 27-wide rows through L2) and keeps the dense copy in LDS
  M.con_direct = (nv <= 16 && !M.con_general) ? 1 : 0;
  M.all_handoff = (sw.all_handoff && d->ngeom <= 32 && d->nbody <= 32 && nv <= 32) ? 1 : 0;
  // small plain models (the ones that run four environments per wavefront, no optional physics): a leaner arena (DevModel::lds_diet).  MJH_LDS_DIET=0: off
  M.lds_diet = (sw.lds_diet && d->nbody <= 16 && d->njnt <= 16 && nv <= 16 && !M.has_fluid && !M.has_gravcomp && d->ntendon == 0) ? 1 : 0;
  M.pair_cull_on = sw.pair_cull ? 1 : 0;  // MJH_PAIR_CULL=0: RK4 stages 1..3 narrow-phase every pair like stage 0
  // the level sweep (Env::kinematics): same operations per body as the walk, bit-identical; MJH_KIN_LEVEL=0 keeps the walk (A / B runs)
  M.kin_lvl = (sw.kin_level && d->nbody > 1 && d->nbody <= 32) ? 1 : 0;  // (nb <= 32: one body per lane in EVERY instantiation the model can run at -- 16 lanes per environment only with nbody <= 16, else 32 or 64 -- so that which kernel a batch size or an odd tail selects never changes a bit)
  M.sol_qm_lds = (d->nefc > 0 && d->iterations > 4) ? 1 : 0;  // one pass over qM per solver iteration: from LDS when there are many
  // register solver, Newton, float32: J^T diag(w) J on the matrix cores (v_mfma_f32_4x4x1, 16 independent 4 x 4 blocks: each environment's lanes feed only their own blocks).  MJH_SOL2_MFMA=0: vector path
  M.sol2_hs = (sw.sol2_mfma && sizeof(REAL) == 4 && d->solver == SOL_NEWTON && nv <= 16 && d->nefc > 0) ? 1 : 0;
  M.sol2_incr = (sw.sol2_incr && d->solver == SOL_NEWTON && nv <= 16 && d->nefc > 0) ? 1 : 0;

  for (int p = 0; p < MJH_NARENA; p++) {
    carve(out, (Arena)p, M, 1 << p);
    if (p == AR_SOL && out->lds(AR_SOL) > kLdsCu && M.sol_qm_lds) {  // a large model: qM stays in global memory (L2) for the solver's products
      M.sol_qm_lds = 0;
      carve(out, AR_SOL, M, 1 << p);
    }
    if (p < MJH_NPHASE && out->lds((Arena)p) > kLdsCu) return fail(-12, "model does not fit the 160 KiB LDS of one CU");
  }
  {  // register solver: CG, slide / hinge limit rows + contact rows only, one dof per lane of a 32-lane half
    const int nd = d->nefc - d->nf - d->nl;
    const bool general = d->nf > 0 || d->nft > 0 || d->ne > 0 || d->nlb > 0 || d->nlt > 0;
    const int nmax = nv <= 8 ? 8 : (nv <= 16 ? 16 : 28), rpl = nd <= 32 ? 1 : (nd <= 64 ? 2 : (nd <= 128 ? 4 : 8));
    // Newton (Hessian built and factorised in registers): two environments per wavefront run until BOTH have converged, which pays
    // when the solves are short -- measured on MI355X: ant (nv 8, 1 - 3 iterations) solver phase 229 -> 175 us, mesh scene (nv 12, up to
    // 100 iterations x 50 line-search steps, very uneven across environments) 548 -> 691 us.
    // (... with FOUR environments per wavefront -- the first tier of models whose nv, na and single-column rows fit 16 lanes, see below -- the shared
    // nv-sized work outweighs the wait: the mesh scene's solver phase 338 -> see profiles/r03/notes.md)
    const bool w16 = nv <= 16 && d->na <= 16 && d->nl <= 16;
    const bool solver_ok = d->solver == SOL_CG || (d->solver == SOL_NEWTON && (nv <= 8 || w16));
    if (solver_ok && !general && nv <= 28 && nd <= 32 * (nmax <= 16 ? 8 : 2) && d->nl <= 32 && d->na <= 32 && d->nq <= 64 && 2 * out->lds(AR_SOL2) <= kLdsWg) {
      out->sol2_nmax = nmax;
      out->sol2_rpl = rpl;
      // measured on MI355X (profiles/r02/notes.md): ant solver phase 124 -> 114 us (the narrow tier runs three waves per SIMD).
      // Small models (nv, na and the single-column rows fit 16 lanes): the first tier packs FOUR environments per wavefront.  The solver's nv-sized
      // work (substitutions, Cholesky of the Newton Hessian, M products) costs a wave the same whatever it carries, so its cost per environment
      // halves, and a CU keeps twice the environments in flight.  Row slots of that tier: 2 per lane (32 rows) for contacts of up to 4 rows,
      // 5 (80 rows) for wider ones (condim 6 pyramidal: 10 rows per contact).
      const int w16_rpl = ((M.con_rows > 0 && M.con_rows <= 4) || nd <= 32) ? 2 : 5;
      DevModel<REAL> Mc = M;
      if (w16) {
        Mc.sol2_row_cap = 16 * w16_rpl;
        if (4 * carve(out, AR_TIER, Mc, PH_SOL2) <= kLdsWg) {
          out->sol2_tiers = 1; out->sol2_w16_rpl = w16_rpl;
          out->sol2_w16_nmax = nv <= 8 ? 8 : (nv <= 12 ? 12 : 16);
        }
      }
      if (!out->sol2_tiers && rpl > 1) {
        Mc.sol2_row_cap = 32;
        carve(out, AR_TIER, Mc, PH_SOL2);
        out->sol2_tiers = 1;
      }
    }
  }
  {  // constraint stage + register solver in one kernel: plain rows, one dense-row slot per lane, no tiers, nv in (16, 28] (the instantiation that is built).
     // Measured on the humanoid (MI355X, B = 4096): profiles/r04/notes.md.
    bool mono = true;  // contact rows in contact order (the in-place row compaction walks them upwards)
    for (int c = 1; c < d->ncon; c++) mono = mono && d->con_efc_address[c] > d->con_efc_address[c - 1];
    if (out->sol2_nmax == 28 && out->sol2_rpl == 1 && !out->sol2_tiers && !M.con_direct && !M.con_general && !M.topk && d->ncon > 0 && d->nefc > 0 && mono &&
        M.con_rows > 0 && M.ncrow == d->nefc - d->nl && d->nf == 0 && nv <= 32 && d->nq <= 64 && d->nl <= 32 && d->na <= 32) {
      if (carve(out, AR_CS, M, PH_CS) > 0 && 2 * out->lds(AR_CS) <= kLdsWg) out->fuse_cs = 1;
      else out->arena[AR_CS].bytes = 0;  // (the carve is negative when the overlays do not work out)
    }
  }
  {  // inverse-dynamics tail (mjh_inverse.h): one environment per 16 / 32 / 64 lanes, 256 lanes per workgroup, LDS_BUDGET bytes per workgroup shared by its environments.
     // The chunk of matrix rows an environment streams through LDS is what is left of its share after qacc, M qacc, qfrc_constraint and the chunk's forces.
    constexpr int LDS_BUDGET = 52 * 1024;  // three workgroups per CU (160 KB)
    out->inv_lanes = nv <= 16 ? 16 : (nv <= 32 ? 32 : 64);
    out->inv_envs = 256 / out->inv_lanes;
    const int reals = LDS_BUDGET / out->inv_envs / (int)sizeof(REAL);
    const int rows_max = d->nefc > nv ? d->nefc : (nv > 0 ? nv : 1);
    int chunk = (reals - 3 * nv) / (nv + 1);
    if (chunk > rows_max) chunk = rows_max;
    if (chunk < 1) return fail(-12, "inverse dynamics: nv too large for the LDS chunk of one environment");
    out->inv_chunk = chunk;
    out->inv_lds_env = (3 * nv + chunk + chunk * nv + 1) & ~1;
  }
  {  // body accelerations and forces (mjh_postcon.h): one environment per 16 / 32 / 64 lanes (from nbody), up to 256 lanes per workgroup; an environment keeps seven
     // per-body arrays (30 reals a body) and the contacts' moved wrenches (14 reals a contact) in LDS.  A workgroup is planned for kLdsWg bytes; an environment that
     // needs more than that runs alone, and one that does not fit a CU's LDS is refused by mjh_postconstraint (the rest of the library still serves the model).
    const int nb = d->nbody;
    out->pc_lanes = nb <= 16 ? 16 : (nb <= 32 ? 32 : 64);
    out->pc_lds_env = (30 * nb + 14 * d->ncon + 1) & ~1;
    const int64_t env_bytes = (int64_t)out->pc_lds_env * (int64_t)sizeof(REAL);
    const int fit = (int)std::min<int64_t>(MJH_POSTCON_WG / out->pc_lanes, kLdsWg / std::max<int64_t>(env_bytes, 1));
    out->pc_envs = env_bytes > kLdsCu ? 0 : std::max(fit, 1);
  }
  {  // contact forces and their sensors (mjh_contact_sensors.h): an environment keeps MJH_CONSENS_LDS_CONTACT reals a contact slot in LDS; the lanes per environment
     // and the environments per workgroup follow from the call's sensor count (run_consens)
    out->cs_lds_env = std::max(4, (MJH_CONSENS_LDS_CONTACT * d->ncon + 3) & ~3);
    out->cs_ok = (int64_t)out->cs_lds_env * (int64_t)sizeof(REAL) <= kLdsCu;
  }
  // phases that are register-bound (not LDS-bound) run two environments per wavefront, 32 lanes each: the same
  // VGPR budget then keeps twice as many environments in flight (mjh_kernels.h, Env<REAL, W>)
  out->pack2[AR_KIN] = 2 * out->lds(AR_KIN) <= kLdsWg;
  out->pack2[AR_VEL] = 2 * out->lds(AR_VEL) <= kLdsWg;
  {  // fused kinematics + velocity kernel (plain velocity phase only).  Measured on MI355X: profiles/r02/notes.md.
    int defer_ok = 0;
    carve(out, AR_KV, M, PH_KINVEL, &defer_ok);
    M.kv_defer = defer_ok;
    out->fuse_kv = (!(M.has_fluid || M.has_gravcomp || M.ntendon > 0 || M.big) && out->lds(AR_KV) <= kLdsCu) ? 1 : 0;
  }
  out->pack2[AR_CON] = M.con_direct && 2 * out->lds(AR_CON) <= kLdsWg;  // plain constraint phase: its contact rows go straight to the leaf, the arena is small enough for two per wavefront
  // CRB: the register Cholesky keeps one matrix row per lane, so nv <= 32 would fit a 32-lane half too; measured on the float64
  // humanoid (nv 27) two per wavefront is SLOWER, 50.2 vs 39.9 us (132 VGPRs: 3 waves / SIMD instead of 4, and every broadcast of the
  // factorisation becomes two v_readlane + a select).  float32 small models: +13 % on the ant (round 1).
  // (round 4, after the register work of round 3: 35.1 vs 36.5 us, and it is what lets kernel 13 serve the humanoid)
  out->pack2[AR_CRB] = ((sizeof(REAL) == 4 && nv <= 16) || (nv <= 32 && nv > 16)) && 2 * out->lds(AR_CRB) <= kLdsWg;
  // small models (every per-body / per-joint / per-dof loop fits 16 lanes): FOUR environments per wavefront in the packed phases.
  // These phases are bound by the number of dependent chains a SIMD can interleave (registers cap the waves), so the same waves
  // carrying twice the environments is close to twice the throughput -- measured on the ant (B = 16384, 64 environments per CU):
  // see profiles/r02/notes.md.
  if (d->nbody <= 16 && d->njnt <= 16 && nv <= 16)
    for (const Arena a : {AR_KIN, AR_CRB, AR_VEL}) out->pack4[a] = out->pack2[a] && 4 * out->lds(a) <= kLdsWg;
  // the fused kinematics + velocity kernel packs where both of its phases do and its own arena fits
  out->pack2[AR_KV] = out->pack2[AR_KIN] && out->pack2[AR_VEL] && 2 * out->lds(AR_KV) <= kLdsWg;
  out->pack4[AR_KV] = out->pack4[AR_KIN] && out->pack4[AR_VEL] && 4 * out->lds(AR_KV) <= kLdsWg;
  {  // kinematics + crb / factor + velocity as ONE kernel (13): when the crb stage packs environments per wavefront the way the other two do (float32 models with
     // nv <= 16, and every model with 16 < nv <= 32).  Saves the crb kernel's loads of cinert / cdof, its launch and the wait between the launches.
     // At every batch size (round 4; round 3 had kept the separate launches past one round of waves): the humanoid (two per wavefront) at B = 32768: 652 us against 452 + 218;
     // the ant (four per wavefront) at B = 16384, two rounds: 93.6 us against 75.8 + 21.8 (profiles/r04/notes.md)
    carve(out, AR_KCV, M, PH_KCV);
    const bool same_pack = out->pack2[AR_CRB] == out->pack2[AR_KV] && out->pack4[AR_CRB] == out->pack4[AR_KV];
    out->fuse_kcv = (out->fuse_kv && same_pack && out->pack2[AR_CRB] && out->lds(AR_KCV) <= kLdsCu && 2 * out->lds(AR_KCV) <= kLdsWg &&
                     (!out->pack4[AR_CRB] || 4 * out->lds(AR_KCV) <= kLdsWg)) ? 1 : 0;
  }
  // kernel 13 on two wavefronts per workgroup (velocity beside crb / factor): packed float32 models.  MJH_KCV2=0 / 1 forces it off / on (also for float64, two per wavefront).
  if (out->fuse_kcv && sw.kcv2 != 0 && (sw.kcv2 == 1 || (sizeof(REAL) == 4 && out->pack4[AR_CRB]))) {
    const int per_wg = (out->pack4[AR_CRB] ? 4 : 2) * carve(out, AR_KCV2, M, PH_KCV2);
    if (per_wg <= kLdsWg) {
      out->kcv2 = 1;
      // The two-wave form pays while the whole batch is resident at once: two wavefronts per workgroup at four per SIMD are 8 workgroups per CU (and their arenas must fit the
      // CU's 160 KB).  Past that it runs more rounds of waves than kernel 13 (which fits 16 one-wave workgroups) and loses.  Measured (MI355X, profiles/r05/notes.md): mesh scene
      // B = 8192 37.5 us against 46.0; ant B = 8192 46.1 against 54.5; ant B = 16384 (two rounds against one) 101 against 62.
      // The limit belongs to the device a LAUNCH runs on, not to the one that was current when the model was built: kcv2_limit() below, cached per device.
      out->kcv2_per_wg = per_wg;
      out->kcv2_envs_per_wg = out->pack4[AR_CRB] ? 4 : 2;
      out->kcv2_max_envs = sw.kcv2 == 1 ? ((int64_t)1 << 62) : 0;
    }
  }
  // the whole pass in one kernel: models both fused kernels serve at two environments per wavefront, without convex pairs or sensors (their kernels sit between the two halves).
  // Measured (MI355X, humanoid B = 4096, three A / B pairs in one call, profiles/r04/notes.md): 166.8 - 170.5 us in one launch against 91.7 - 93.1 + 76.4 - 76.7 in two
  // (23.5 - 24.3 M against 24.1 - 24.6 M env-steps/s): the one function is allocated 256 VGPRs + 304 B of scratch where the halves take 198 + 0 and 256 + 120 B, and that
  // costs what the missing device-wide barrier saves.  Opt-in (MJH_FUSE_ALL=1).
  // Round 5: for models with opt.iterations == 1 (the humanoid benchmark) the one-iteration instantiation (W = 36: the solver loop is straight-line code, the factor of M
  // dies behind its one preconditioning step) takes 256 VGPRs + 52 B where the generic one takes 256 + 304 B, and the single launch wins at every batch size: B = 4096
  // 155.0 - 155.9 us against 91.0 + 71.0 - 71.6 in two launches (25.5 - 25.7 M against 25.0 - 25.2 M env-steps/s), B = 32768 1162 us against 657 + 577 (27.8 - 28.1 M against
  // 26.4 M; profiles/r05/notes.md).  Default on for those models (MJH_FUSE_ALL=0: off); still opt-in (MJH_FUSE_ALL=1) for the others.
  // (round 5, second half: without the kernels' grid-stride loops the generic instantiation takes 228 VGPRs and no scratch either: default on for every model both fused kernels serve)
  if (sw.fuse_all != 0 && out->fuse_cs && out->fuse_kcv && out->pack2[AR_CRB] && !out->pack4[AR_CRB] && M.ncvxpair == 0 && d->nsensor == 0) {
    out->lds_all = std::max(out->lds(AR_KCV), out->lds(AR_CS));
    if (2 * out->lds_all <= kLdsWg) {
      out->fuse_all = 1;
      M.nt_all = M.all_handoff;
    }
  }
  // One launch per RK4 stage (stage 0 too, unless MJH_FUSE_STAGE0=0) for small Newton models: kernel 13 at four environments per wavefront, the direct constraint phase (kernel 8, two
  // per wavefront: run twice per wave) and the solver's packed Newton tier at four, behind one another in mjh_sol2_kernel<.., 18>.  MJH_FUSE_STAGE=0: the three launches.
  if (sw.fuse_stage && d->integrator == INT_RK4 && d->solver == SOL_NEWTON && out->fuse_kcv && out->pack4[AR_CRB] && M.con_direct && out->pack2[AR_CON] && out->sol2_tiers &&
      out->sol2_w16_nmax == 8 && (out->sol2_w16_rpl == 2 || out->sol2_w16_rpl == 5) && M.ncvxpair == 0 && d->nefc > 0) {
    const int need = std::max({4 * out->lds(AR_KCV), 2 * out->lds(AR_CON), 4 * out->lds(AR_TIER)});
    if (need <= kLdsWg) { out->fuse_stage = 1; out->lds_stage = need; }
  }
  // ... and the tail of a pass alone (MJH_FUSE_TAIL=0: the two launches)
  // Measured (MI355X, profiles/r06/notes.md): mesh scene (12 dofs: the tier's instantiation takes 227 VGPRs, two waves per SIMD, and the constraint phase inherits that) 219.6 us
  // against 167.9 + 49.2 in two launches -- 8-dof tiers only (the one instantiation that is built), whose kernel sits at the constraint phase's own four waves per SIMD.
  if (sw.fuse_tail && d->solver == SOL_NEWTON && M.con_direct && out->pack2[AR_CON] && out->sol2_tiers && out->sol2_w16_nmax == 8 && d->nefc > 0 && !M.topk) {
    const int need = std::max(2 * out->lds(AR_CON), 4 * out->lds(AR_TIER));
    if (need <= kLdsWg) { out->fuse_tail = 1; out->lds_tail = need; }
  }

  // workspace per environment (run()): [hand-over | candidates | RK4 stage Data | RK4 sums]
  if (d->integrator == INT_RK4) {
    const char* names[] = {
#define X(n) #n,
        MJH_DATA_REALS(X)
#undef X
    };
    out->stage_leaf.assign(out->leaf_count.size(), STAGE_NONE);
    for (size_t i = 0; i < out->leaf_count.size(); i++)
      if (is_stage_leaf(names[i], M.ncvxpair > 0, M.has_fluid != 0, M.ne > 0, M.topk != 0)) {
        // (kernel 13 keeps cinert / xipos in its arena from the kinematics to the crb and velocity stages: no later LAUNCH of a stage reads their workspace copies -- left NULL, the stores are skipped)
        out->stage_leaf[i] = (out->fuse_kcv && (!strcmp(names[i], "cinert") || !strcmp(names[i], "xipos"))) ? STAGE_SPACE : STAGE_SLOT;
        out->work_reals += out->leaf_count[i];
      }
    out->work_reals += 4 * (int64_t)d->nv + 2 * (int64_t)d->na;  // qvel0, kqvel(unused), sum_qvel, sum_qacc, act0, sum_actdot
  }
  {  // hand-over of the small-model constraint phase (kernel 8) to the register solver: [count | contact -> slot | D | aref | rows] of the active contacts' rows, compact.  MJH_HANDOVER=0: off
    const int64_t nd = (int64_t)d->nefc - d->nl;
    // Measured (MI355X, profiles/r05/notes.md): ant (RK4: stages 1..3 write the hand-over INSTEAD of their workspace leaves) solver phase 44.7 -> 42.3 us per stage, constraint phase unchanged;
    // mesh scene (Euler: the leaves AND the hand-over) solver 197.9 -> 194.4 us but constraint phase 47.2 -> 52.0: RK4 models only.
    out->hs_reals = (sw.handover && d->integrator == INT_RK4 && M.con_direct && M.crow_by_con && out->sol2_nmax && !out->fuse_cs && nd > 0) ? ((1 + (int64_t)d->ncon + 2 * nd + nd * d->nv + 3) & ~(int64_t)3) : 0;
    out->work_reals += out->hs_reals;
  }
  out->cand_reals = (d->topk && M.ncvxpair > 0) ? 13 * (int64_t)d->ncand : 0;  // candidate contacts of the convex / quadric narrow phases (dist, pos, frame)
  out->work_reals += out->cand_reals;
  return 0;
}

// ---- grants: the dynamic LDS of every kernel the plan can launch, from the plan's fields (hipFuncSetAttribute is per function: the last model built sets it) ----
template <typename REAL>
int grant_lds(const mjhModel* m) {
  HIP_TRY((allow_phase_lds_packed<REAL, MJH_KERNEL_KIN>(m)));
  HIP_TRY((allow_phase_lds_packed<REAL, MJH_KERNEL_CRB>(m)));
  HIP_TRY((allow_phase_lds_packed<REAL, MJH_KERNEL_CON>(m)));
  HIP_TRY((allow_phase_lds_packed<REAL, MJH_KERNEL_VEL>(m)));
  HIP_TRY((allow_phase_lds_packed<REAL, MJH_KERNEL_SOL>(m)));
  HIP_TRY((allow_phase_lds_packed<REAL, MJH_KERNEL_SOL_GEN>(m)));
  HIP_TRY((allow_phase_lds_packed<REAL, MJH_KERNEL_CON_GEN>(m)));
  HIP_TRY((allow_phase_lds_packed<REAL, MJH_KERNEL_CON_DIRECT>(m)));
  HIP_TRY((allow_phase_lds_packed<REAL, MJH_KERNEL_VEL_OPT>(m)));
  if (m->fuse_kcv) HIP_TRY((allow_phase_lds_packed<REAL, MJH_KERNEL_KCV>(m)));  // (fuse_kcv: the crb arena packs two per wavefront)
  if (m->fuse_kv) {  // (its packed forms by its own arena alone: pack2 / pack4 of AR_KV also need both phases packed)
    HIP_TRY((allow_phase_lds<REAL, MJH_KERNEL_KV, MJH_WAVE>(m)));
    if (2 * m->lds(AR_KV) <= kLdsWg) HIP_TRY((allow_phase_lds<REAL, MJH_KERNEL_KV, 32>(m)));
    if (4 * m->lds(AR_KV) <= kLdsWg) HIP_TRY((allow_phase_lds<REAL, MJH_KERNEL_KV, 16>(m)));
  }
  if (m->kcv2) {  // (the two-wave form only exists packed)
    HIP_TRY((allow_phase_lds<REAL, MJH_KERNEL_KCV2, 32>(m)));
    if (m->pack4[AR_CRB]) HIP_TRY((allow_phase_lds<REAL, MJH_KERNEL_KCV2, 16>(m)));
  }
  HIP_TRY(allow_lds(&mjh_convex_kernel<REAL>, m->cvx_lds_bytes));
  if (m->sol2_nmax) HIP_TRY(allow_sol2_lds<REAL>(SOL2_PAIR, 2 * m->lds(AR_SOL2)));
  if (m->sol2_w16_rpl) {
    HIP_TRY(allow_sol2_lds<REAL>(SOL2_QUAD, 4 * m->lds(AR_TIER)));
    HIP_TRY(allow_sol2_lds<REAL>(SOL2_QUAD_NEWTON, 4 * m->lds(AR_TIER)));
  }
  if (m->fuse_cs) {
    HIP_TRY(allow_sol2_lds<REAL>(SOL2_CS, 2 * m->lds(AR_CS)));
    HIP_TRY(allow_sol2_lds<REAL>(SOL2_CS_ONE, 2 * m->lds(AR_CS)));
  }
  if (m->fuse_all) {
    HIP_TRY(allow_sol2_lds<REAL>(SOL2_PASS, 2 * m->lds_all));
    HIP_TRY(allow_sol2_lds<REAL>(SOL2_PASS_ONE, 2 * m->lds_all));
  }
  if (m->fuse_stage || m->fuse_tail) HIP_TRY(allow_sol2_lds<REAL>(SOL2_STAGE, std::max(m->lds_stage, m->lds_tail)));
  HIP_TRY(allow_lds(&mjh_inverse_kernel<REAL>, kLdsWg));  // (the inverse tail's LDS_BUDGET plus the rounding of lds_env)
  if (m->pc_envs > 0) HIP_TRY(allow_lds(&mjh_postcon_kernel<REAL>, std::max(kLdsWg, m->pc_envs * m->pc_lds_env * (int)sizeof(REAL))));
  if (m->cs_ok) HIP_TRY(allow_lds(&mjh_consens_kernel<REAL>, std::max(kLdsWg, m->cs_lds_env * (int)sizeof(REAL))));
  HIP_TRY(allow_lds(&mjh_energy_kernel<REAL>, kLdsWg));  // (run_energy's LDS_BUDGET plus the rounding of lds_env)
  HIP_TRY(allow_lds(&mjh_integrate_kernel<REAL>, kLdsWg));  // (run_integrate never asks for more)
  return 0;
}

// ---- upload: the blob to the device, DevModel's table pointers into it ----
int upload(mjhModel* out, const BlobBuilder& bb, const Fixups& fix) {
  void* dev = nullptr;
  HIP_TRY(hipMalloc(&dev, bb.host.size() + 16));
  out->blob = dev;  // (mjh_model_create releases it if what follows fails)
  out->blob_bytes = bb.host.size();
  HIP_TRY(hipMemcpy(dev, bb.host.data(), bb.host.size(), hipMemcpyHostToDevice));
  for (auto& f : fix) *f.first = (const unsigned char*)dev + f.second;
  return 0;
}

template <typename REAL>
int build(const mjhModelDesc* d, mjhModel* out, DevModel<REAL>& M) {
  BlobBuilder bb;
  Fixups fix;
  if (const int rc = tables(d, out, M, bb, fix)) return rc;
  if (const int rc = plan(d, out, M)) return rc;
  if (const int rc = grant_lds<REAL>(out)) return rc;
  return upload(out, bb, fix);
}

// Workgroups per launch.  The kernels run ONE unit of work per workgroup (no grid-stride loop), so a batch past this many is cut into several launches.  2^20 by default;
// MJH_MAX_GRID_LOG2 lowers it so that the tests reach the multi-launch paths at small batches.
static int64_t max_grid() { return (int64_t)1 << switches().max_grid_log2; }

// The kernels run ONE unit of work per workgroup, `per_wg` units each (no grid-stride loop): `count` units go out as launches of at most `max_wg` workgroups.
// launch(first, n, workgroups) enqueues the one of units [first, first + n).
template <typename F>
int launch_cut(int64_t count, int64_t per_wg, F&& launch, int64_t max_wg = max_grid()) {
  for (int64_t first = 0; first < count; first += per_wg * max_wg) {
    const int64_t n = count - first < per_wg * max_wg ? count - first : per_wg * max_wg;
    launch(first, n, (unsigned)((n + per_wg - 1) / per_wg));
    HIP_TRY(hipGetLastError());
  }
  return 0;
}

template <typename REAL, int P, int W>
int launch_range(const mjhModel* m, KArgs<REAL>& a, int64_t begin, int64_t count, hipStream_t stream) {
  if (count <= 0) return 0;
  constexpr int NSUB = MJH_WAVE / W;
  const ArenaLds& ar = m->arena[phase_kernel(P).arena];
  a.off = ar.off;
  a.lds_reals = ar.bytes / (int)sizeof(REAL);
  const int rc = launch_cut(count, NSUB, [&](int64_t first, int64_t n, unsigned grid) {
    a.env_begin = begin + first; a.env_count = n;
    hipLaunchKernelGGL((mjh_phase_kernel<REAL, P, W>), dim3(grid), dim3(phase_threads(P)), (size_t)(NSUB * ar.bytes), stream, a);
  });
  if (rc) return rc;
  timing_mark(stream, P);
  return 0;
}
template <typename REAL, int P>
int launch_phase(const mjhModel* m, KArgs<REAL>& a, hipStream_t stream) {
  constexpr PhaseKernel K = phase_kernel(P);
  int64_t done = 0;
  int rc = 0;
  if constexpr (K.max_envs > 1) {
    if (m->pack2[K.pack] && a.B >= 2) {  // groups of four / pairs of environments, then the odd one on its own
      if constexpr (K.max_envs == 4) {
        if (m->pack4[K.pack] && a.B >= 4) {
          done = a.B & ~(int64_t)3;
          if ((rc = launch_range<REAL, P, 16>(m, a, 0, done, stream))) return rc;
        }
      }
      const int64_t even = (a.B - done) & ~(int64_t)1;
      if ((rc = launch_range<REAL, P, 32>(m, a, done, even, stream))) return rc;
      done += even;
    }
  }
  // (one environment per wavefront: the two-wave form only exists packed, kernel 13 serves the odd environment)
  return launch_range<REAL, (P == MJH_KERNEL_KCV2 ? MJH_KERNEL_KCV : P), MJH_WAVE>(m, a, done, a.B - done, stream);
}

// MJH_XSWAP=mask (12 bits of the workgroup index; 0: off): in the whole-pass kernel and the stage kernel, workgroups of odd parity under the mask run the velocity stage before
// crb / factor (mjh_sol2_kernel: "out of lockstep").  Default 0x100: workgroups 256 apart, i.e. different wave slots of the same CUs under the round-robin placement.  Measured
// (MI355X, humanoid B = 4096, profiles/r06/notes.md): 141.5 - 144.0 us -> 137.0 - 137.6 us whatever the mask (0x1 .. 0xfff); B = 32768 (eight rounds: the waves drift apart by themselves) unchanged.
// Launches of more than 4096 workgroups keep one order: B = 32768 (eight rounds, the waves drift apart by themselves) measured 1015 us in one order against 1033 us with the swap.
// MJH_XSWAP_K=mask (default 0x200; 0: off): the same idea inside the kinematics stage -- workgroups of odd parity under this mask run com_pos before the geom / site / camera frames
// (Env::kinematics, com_first).  Measured (MI355X, humanoid B = 4096, profiles/r06/notes.md): 138.8 -> 136.0 us on top of MJH_XSWAP; bit-identical.
// A mask that is set applies at every launch size; the defaults at launches of at most 4096 workgroups.
static int xswap_mask(int set, int default_mask, int64_t workgroups) { return set >= 0 ? set : (workgroups <= 4096 ? default_mask : 0); }

// the out-of-lockstep masks of a launcher of `workgroups` workgroups: a.flags carries MJH_XSWAP's for the launcher's scope, a.xswap_k MJH_XSWAP_K's
template <typename REAL>
struct OutOfLockstep {
  KArgs<REAL>& a;
  const int flags;
  OutOfLockstep(KArgs<REAL>& args, int64_t workgroups) : a(args), flags(args.flags) {
    a.flags |= xswap_mask(switches().xswap, 0x100, workgroups) << 16;
    a.xswap_k = xswap_mask(switches().xswap_k, 0x200, workgroups);
  }
  ~OutOfLockstep() { a.flags = flags; }
};

// register-solver instantiation (NMAX, RPL, form WT) over the batch, MJH_WAVE / lanes environments per workgroup
template <typename REAL>
int launch_sol2_kernel(KArgs<REAL>& a, int nmax, int rpl, int wt, int lds, hipStream_t stream) {
  const Kernel<REAL> fn = sol2_kernel<REAL>(nmax, rpl, wt);
  if (!fn) return fail(-5, "no register-solver instantiation for this model");
  if (a.scan_marks) {  // the marks-scanning second tier walks the batch itself: one grid of at most 4096 waves (env_begin = 0, env_count = B)
    const int64_t waves = (a.B + MJH_WAVE - 1) / MJH_WAVE;
    hipLaunchKernelGGL(fn, dim3((unsigned)(waves < 4096 ? waves : 4096)), dim3(MJH_WAVE), (size_t)lds, stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
  }
  const int rc = launch_cut(a.B, MJH_WAVE / sol2_form(wt).lanes, [&](int64_t first, int64_t n, unsigned grid) {
    a.env_begin = first; a.env_count = n;
    hipLaunchKernelGGL(fn, dim3(grid), dim3(MJH_WAVE), (size_t)lds, stream, a);
  });
  a.env_begin = 0; a.env_count = a.B;
  return rc;
}

// the solver phase through the register solver: two (or, first tier of a small model, four) environments per wavefront
template <typename REAL>
int launch_sol2(const mjhModel* m, KArgs<REAL>& a, hipStream_t stream, bool first_done = false) {  // first_done: the stage kernel has run the first tier (and marked what it left): only the second tier is launched
  a.env_begin = 0; a.env_count = a.B;
  const int nd = a.M.nefc - a.M.nf - a.M.nl;
  bool second = true;
  const bool marks = m->sol2_tiers && a.cur.qacc != nullptr;  // the first tier marks what it leaves, the second scans the marks (needs the qacc leaf)
  a.mark_leftover = marks ? 1 : 0;
  int rc = 0;
  a.row_lo = -1;
  if (m->sol2_tiers) {  // first tier: fewer row slots per lane, its own (smaller) arena
    a.off = m->arena[AR_TIER].off;
    a.lds_reals = m->lds(AR_TIER) / (int)sizeof(REAL);
    if (m->sol2_w16_rpl) {
      a.row_hi = 16 * m->sol2_w16_rpl;
      const int wt = a.M.solver == SOL_NEWTON ? SOL2_QUAD_NEWTON : SOL2_QUAD;
      if (!first_done && (rc = launch_sol2_kernel(a, m->sol2_w16_nmax, m->sol2_w16_rpl, wt, 4 * m->lds(AR_TIER), stream))) return rc;
      second = nd > a.row_hi;  // every environment fits the first tier otherwise
    } else {
      a.row_hi = 32;
      if ((rc = launch_sol2_kernel(a, m->sol2_nmax, 1, SOL2_PAIR, 2 * m->lds(AR_TIER), stream))) return rc;
    }
    a.row_lo = a.row_hi;
  }
  a.mark_leftover = 0;
  if (second) {
    a.row_hi = 0x7fffffff;
    a.off = m->arena[AR_SOL2].off;
    a.lds_reals = m->lds(AR_SOL2) / (int)sizeof(REAL);
    a.scan_marks = marks ? 1 : 0;
    if ((rc = launch_sol2_kernel(a, m->sol2_nmax, m->sol2_rpl, SOL2_PAIR, 2 * m->lds(AR_SOL2), stream))) return rc;
    a.scan_marks = 0;
  }
  if (!(first_done && !second)) timing_mark(stream, MJH_KERNEL_SOL2);  // both tiers under one mark: the solver phase (behind the stage kernel: the second tier alone, when there is one)
  return 0;
}

// one RK4 stage of a small Newton model in one launch (mjhModel::fuse_stage), then the solver's second tier for what the first left
template <typename REAL>
int launch_stage(const mjhModel* m, KArgs<REAL>& a, hipStream_t stream, int parts = 7) {  // parts 6: the tail of a pass (constraint phase + first solver tier) behind launches of its own for the rest
  a.stage_parts = parts;
  const OutOfLockstep<REAL> swap(a, a.B / 4);
  const int xswap_c = switches().xswap_c;  // MJH_XSWAP_C=mask (default 0x400, 0: off; see KArgs::xswap_c): measured ant 30.9 -> 31.1 M env-steps/s
  a.xswap_c = a.rk_stage == 0 ? (xswap_c >= 0 ? xswap_c : 0x400) : 0;
  a.off = m->arena[AR_KCV].off; a.lds_reals = m->lds(AR_KCV) / (int)sizeof(REAL);
  a.off2 = m->arena[AR_CON].off; a.lds_reals2 = m->lds(AR_CON) / (int)sizeof(REAL);
  a.off3 = m->arena[AR_TIER].off; a.lds_reals3 = m->lds(AR_TIER) / (int)sizeof(REAL);
  a.row_lo = -1; a.row_hi = 16 * m->sol2_w16_rpl;
  a.mark_leftover = (m->sol2_tiers && a.cur.qacc != nullptr) ? 1 : 0;
  a.scan_marks = 0;
  // (fuse_stage / fuse_tail: 8-dof tiers only)
  if (const int rc = launch_sol2_kernel(a, 8, m->sol2_w16_rpl, SOL2_STAGE, parts == 7 ? m->lds_stage : m->lds_tail, stream)) return rc;
  timing_mark(stream, parts == 7 ? MJH_KERNEL_STAGE : MJH_KERNEL_TAIL);
  return launch_sol2<REAL>(m, a, stream, true);
}

// constraint stage + register solver + integrator in one launch (mjhModel::fuse_cs)
template <typename REAL>
int launch_cs(const mjhModel* m, KArgs<REAL>& a, hipStream_t stream) {
  a.off = m->arena[AR_CS].off;
  a.lds_reals = m->lds(AR_CS) / (int)sizeof(REAL);
  a.row_lo = -1; a.row_hi = 0x7fffffff;
  a.mark_leftover = 0; a.scan_marks = 0;
  // opt.iterations == 1 (solver.py:534-535: the loop body runs exactly once): straight-line solver code
  // (A / B switch: MJH_CS_ONE=0 launches the generic instantiation for one-iteration models too)
  const int wt = a.M.iterations == 1 && switches().cs_one ? SOL2_CS_ONE : SOL2_CS;
  if (const int rc = launch_sol2_kernel(a, 28, 1, wt, 2 * m->lds(AR_CS), stream)) return rc;
  timing_mark(stream, MJH_KERNEL_CS);
  return 0;
}

// the whole pass in one launch (mjhModel::fuse_all).  The caller bounds B to one launch.
template <typename REAL>
int launch_all(const mjhModel* m, KArgs<REAL>& a, hipStream_t stream) {
  a.off = m->arena[AR_KCV].off; a.off2 = m->arena[AR_CS].off;
  a.lds_reals = m->lds_all / (int)sizeof(REAL);
  a.row_lo = -1; a.row_hi = 0x7fffffff;
  a.mark_leftover = 0; a.scan_marks = 0;
  const int64_t blocks = (a.B + 1) / 2;
  const OutOfLockstep<REAL> swap(a, blocks < (int64_t)1 << 20 ? blocks : (int64_t)1 << 20);
  if (const int rc = launch_sol2_kernel(a, 28, 1, a.M.iterations == 1 ? SOL2_PASS_ONE : SOL2_PASS, 2 * m->lds_all, stream)) return rc;
  timing_mark(stream, MJH_KERNEL_PASS);
  return 0;
}

// convex narrow phase: one wavefront per (environment, pair), one launch per 2^22 of them; sensors: one per environment
// (a launch of either narrow-phase kernel sees DevModel::cvx_pairs / ncvxpair narrowed to its own pairs: NarrowedPairs)
template <typename REAL>
struct NarrowedPairs {
  DevModel<REAL>& M;
  const int* const pairs;
  const int n;
  NarrowedPairs(DevModel<REAL>& M_, int first, int count) : M(M_), pairs(M_.cvx_pairs), n(M_.ncvxpair) { M.cvx_pairs = pairs + first; M.ncvxpair = count; }
  ~NarrowedPairs() { M.cvx_pairs = pairs; M.ncvxpair = n; }
};
template <typename REAL>
int launch_convex(const mjhModel* m, KArgs<REAL>& a, hipStream_t stream) {
  const NarrowedPairs<REAL> own(a.M, 0, m->ncvx);
  const int rc = launch_cut(a.B * a.M.ncvxpair, 1, [&](int64_t first, int64_t, unsigned grid) {
    a.env_begin = first;  // (first ITEM of this launch)
    hipLaunchKernelGGL((mjh_convex_kernel<REAL>), dim3(grid), dim3(MJH_WAVE), (size_t)m->cvx_lds_bytes, stream, a);
  }, 4 * max_grid());
  a.env_begin = 0;
  if (rc) return rc;
  timing_mark(stream, MJH_KERNEL_CONVEX);
  return 0;
}
// plane-ellipsoid / plane-cylinder narrow phase: one LANE per (environment, pair), 64 items per one-wave workgroup
template <typename REAL>
int launch_quadric(const mjhModel* m, KArgs<REAL>& a, hipStream_t stream) {
  const NarrowedPairs<REAL> own(a.M, m->ncvx, m->nquad);
  const int rc = launch_cut(a.B * a.M.ncvxpair, MJH_WAVE, [&](int64_t first, int64_t n, unsigned grid) {
    a.env_begin = first; a.env_count = n;  // (ITEMS of this launch)
    hipLaunchKernelGGL((mjh_quadric_kernel<REAL>), dim3(grid), dim3(MJH_WAVE), 0, stream, a);
  });
  a.env_begin = 0; a.env_count = a.B;
  if (rc) return rc;
  timing_mark(stream, MJH_KERNEL_QUADRIC);
  return 0;
}
template <typename REAL>
int launch_sensor_kernel(const mjhModel* m, KArgs<REAL>& a, hipStream_t stream) {
  (void)m;
  // environments per wavefront: two when their slots fit the 64 lanes of the slot phase (MJH_SENSOR_EPW overrides).  Measured (MI355X, ant B = 16384, 27 slots and 104 ray tests per environment):
  // one 36.8 - 37.1 us, two 28.8 - 29.0, four 35.6 - 35.7 (a quarter of the workgroups: too few waves to hide the kernel's two dependent load chains) -- profiles/r05/notes.md
  const int epw_env = switches().sensor_epw;
  int epw = epw_env > 0 ? epw_env : (a.M.nsensordata > 0 ? MJH_WAVE / a.M.nsensordata : 1);
  epw = epw < 1 ? 1 : (epw_env > 0 ? (epw > 8 ? 8 : epw) : (epw > 2 ? 2 : epw));
  a.sns_epw = epw;
  const size_t lds = sizeof(double) * (size_t)(a.M.nrfq + 1) * (size_t)epw;
  const int rc = launch_cut(a.B, epw, [&](int64_t first, int64_t n, unsigned grid) {
    a.env_begin = first; a.env_count = n;
    if (a.M.sns_full) hipLaunchKernelGGL((mjh_sensor_kernel<REAL, 1>), dim3(grid), dim3(MJH_WAVE), lds, stream, a);
    else hipLaunchKernelGGL((mjh_sensor_kernel<REAL, 0>), dim3(grid), dim3(MJH_WAVE), lds, stream, a);
  });
  a.env_begin = 0; a.env_count = a.B;
  if (rc) return rc;
  timing_mark(stream, MJH_KERNEL_SENSOR);
  return 0;
}

// Largest batch the two-wave form of kernel 13 serves in ONE round of its workgroups on the device `stream` belongs to: two wavefronts per workgroup at four per SIMD are 8
// workgroups per CU, and their arenas must fit the CU's LDS.  (CUs, LDS per CU) are read once per device (a model built while another device was current, or stepped
// under bench --gpus N before device selection, kept the wrong one-round threshold: 101 us against 62 for the ant).
static int64_t kcv2_limit(const mjhModel* m, hipStream_t stream) {
  if (m->kcv2_max_envs) return m->kcv2_max_envs;
  static int cus_of[64], lds_of[64];  // 0 = not read yet (plain ints: a race writes the same values twice)
  int dev = 0;
  if (hipStreamGetDevice(stream, &dev) != hipSuccess && hipGetDevice(&dev) != hipSuccess) dev = 0;
  if (dev < 0 || dev >= 64) dev = 0;
  if (!cus_of[dev]) {
    int cus = 256, lds = kLdsCu;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, dev) != hipSuccess || lds < kLdsWg) lds = kLdsCu;
    lds_of[dev] = lds;
    cus_of[dev] = cus > 0 ? cus : 256;
  }
  int wgs = lds_of[dev] / (m->kcv2_per_wg > 0 ? m->kcv2_per_wg : 1);
  if (wgs > 8) wgs = 8;
  return (int64_t)cus_of[dev] * wgs * m->kcv2_envs_per_wg;
}

// Stage masks: mjh_forward runs the pipeline up to and including the highest stage bit asked for, so a phase runs when any stage at or past its own is.
constexpr int kFromCrb = MJH_STAGE_ALL & ~MJH_STAGE_KINEMATICS;
constexpr int kFromCollision = kFromCrb & ~MJH_STAGE_CRB;
constexpr int kFromVelocity = MJH_STAGE_VELOCITY | MJH_STAGE_ACTUATION | MJH_STAGE_SOLVE;
constexpr int kFromActuation = MJH_STAGE_ACTUATION | MJH_STAGE_SOLVE;
constexpr int kUpToVelocity = MJH_STAGE_ALL & ~kFromActuation;

// one forward pass = the phases selected by `stages`
template <typename REAL>
int forward_pass(const mjhModel* m, KArgs<REAL>& a, hipStream_t stream) {
  int rc = 0;
  const int st = a.stages;
  if (m->fuse_all && (st & MJH_STAGE_ALL) == MJH_STAGE_ALL && a.B >= 2 && (a.B & 1) == 0 && a.B <= 2 * max_grid() /* one workgroup per pair: the kernel has no grid-stride loop */ && a.cur.efc_J && a.cur.efc_D && a.cur.efc_aref && a.cur.qM && a.cur.qLD) return launch_all<REAL>(m, a, stream);
  // MJH_FUSE_STAGE0=0: stage 0 (which writes the returned Data in full) keeps its three launches.  Its sensors (they read leaves of the kinematics and velocity stages only) follow the
  // stage kernel: in an RK4 step nothing of stage 0 writes the returned state -- the final advance is stage 3's -- so the jointpos / ballquat readers of out.qpos race nothing.
  if (m->fuse_stage && a.rk_stage >= (switches().fuse_stage0 ? 0 : 1) && (st & MJH_STAGE_ALL) == MJH_STAGE_ALL && a.B >= 4 && (a.B & 3) == 0 && a.cur.qM && a.cur.qLD && a.cur.qfrc_smooth && a.cur.contact_dist &&
      a.cur.efc_J && a.cur.efc_D && a.cur.efc_aref) {
    if ((rc = launch_stage<REAL>(m, a, stream))) return rc;
    if (a.M.nsensor > 0 && a.rk_stage == 0 && a.cur.sensordata) {
      if ((rc = launch_sensor_kernel<REAL>(m, a, stream))) return rc;
    }
    return 0;
  }
  const bool fused_kv = m->fuse_kv && (st & kFromVelocity);  // the velocity phase is asked for: it rides with the kinematics (it needs nothing of CRB / CON)
  const bool fused_kcv = fused_kv && m->fuse_kcv && (st & kFromCrb);  // ... and so does the crb / factor stage (small models)
  if ((st & MJH_STAGE_ALL) && (rc = fused_kcv ? ((m->kcv2 && a.B <= kcv2_limit(m, stream)) ? launch_phase<REAL, MJH_KERNEL_KCV2>(m, a, stream) : launch_phase<REAL, MJH_KERNEL_KCV>(m, a, stream)) : (fused_kv ? launch_phase<REAL, MJH_KERNEL_KV>(m, a, stream) : launch_phase<REAL, MJH_KERNEL_KIN>(m, a, stream)))) return rc;
  if ((st & kFromCollision) && m->ncvx > 0) {  // convex narrow phase: one wave per (environment, pair); needs only the geom frames of PH_KIN
    if ((rc = launch_convex<REAL>(m, a, stream))) return rc;
  }
  if ((st & kFromCollision) && m->nquad > 0) {  // ... and the plane-ellipsoid / plane-cylinder pairs, one lane each
    if ((rc = launch_quadric<REAL>(m, a, stream))) return rc;
  }
  if ((st & kFromCrb) && !fused_kcv && (rc = launch_phase<REAL, MJH_KERNEL_CRB>(m, a, stream))) return rc;
  const bool fused_cs = m->fuse_cs && (st & kFromCollision) && (st & MJH_STAGE_SOLVE) && a.cur.efc_J && a.cur.efc_D && a.cur.efc_aref;  // the whole tail of the pass is asked for: constraint stage and solve share a kernel
  const bool fused_tail = !fused_cs && m->fuse_tail && (st & kFromCollision) == kFromCollision && a.B >= 4 && (a.B & 3) == 0 && a.cur.qM && a.cur.qLD && a.cur.qfrc_smooth && a.cur.contact_dist &&
                          a.cur.efc_J && a.cur.efc_D && a.cur.efc_aref && !(a.M.has_fluid || a.M.has_gravcomp || a.M.ntendon > 0 || a.M.big) && fused_kv;  // (the velocity stage has run: it rode with the kinematics)
  if (fused_tail) {  // small Newton models: constraint phase + first solver tier + integrator in one launch (their sensors read leaves of the kinematics / velocity stages only: first)
    if ((st & MJH_STAGE_SOLVE) && a.M.nsensor > 0 && a.rk_stage <= 0 && a.cur.sensordata) {
      if ((rc = launch_sensor_kernel<REAL>(m, a, stream))) return rc;
    }
    return launch_stage<REAL>(m, a, stream, 6);
  }
  if (!fused_cs && (st & kFromCollision) && (a.M.ncon > 0 || a.M.nefc > 0) &&
      (rc = a.M.con_general ? launch_phase<REAL, MJH_KERNEL_CON_GEN>(m, a, stream) : (a.M.con_direct ? launch_phase<REAL, MJH_KERNEL_CON_DIRECT>(m, a, stream) : launch_phase<REAL, MJH_KERNEL_CON>(m, a, stream)))) return rc;
  if ((st & kFromVelocity) && !fused_kv && (rc = (a.M.has_fluid || a.M.has_gravcomp || a.M.ntendon > 0 || a.M.big) ? launch_phase<REAL, MJH_KERNEL_VEL_OPT>(m, a, stream) : launch_phase<REAL, MJH_KERNEL_VEL>(m, a, stream))) return rc;
  const bool want_sensors = (st & MJH_STAGE_SOLVE) && a.M.nsensor > 0 && a.rk_stage <= 0 && a.cur.sensordata;  // needs only the leaves of KIN and VEL
  if (want_sensors) {  // (round 4's opt-in side stream for this launch is gone: it raced the integrator tail's write of out.qpos, which jointpos / ballquat sensors read, and measured no gain -- profiles/r04/notes.md)
    if ((rc = launch_sensor_kernel<REAL>(m, a, stream))) return rc;
  }
  if (fused_cs) return launch_cs<REAL>(m, a, stream);
  if ((st & kFromActuation) && m->sol2_nmax) return launch_sol2<REAL>(m, a, stream);
  if ((st & kFromActuation) && (rc = (a.M.nf > 0 || a.M.nft > 0 || a.M.ne > 0 || a.M.nlb > 0 || a.M.nlt > 0) ? launch_phase<REAL, MJH_KERNEL_SOL_GEN>(m, a, stream) : launch_phase<REAL, MJH_KERNEL_SOL>(m, a, stream))) return rc;  // (MJH_STAGE_ACTUATION: _acceleration's solve lives at the head of the solver phase)
  return 0;
}

template <typename REAL>
int run(const mjhModel* m, const DevModel<REAL>& M, const mjhData* in, mjhData* out, void* work, int64_t B, int flags, int do_step, int stages, void* stream) {
  if (B <= 0) return 0;
  static_assert(sizeof(DevData<REAL>) == sizeof(mjhData), "DevData must mirror mjhData");
  static_assert(sizeof(KArgs<REAL>) <= 4096, "kernel arguments exceed the 4 KiB kernarg segment");
  KArgs<REAL> a;
  memset(&a, 0, sizeof(a));
  timing_begin((hipStream_t)stream);
  a.M = M;
  memcpy(&a.in, in, sizeof(a.in));
  DevData<REAL> fin;
  memcpy(&fin, out, sizeof(fin));
  a.fin = state_of(fin);
  a.cur = fin;
  a.B = B; a.flags = flags; a.do_step = do_step; a.stages = do_step ? MJH_STAGE_ALL : stages;
  a.rk_stage = -1; a.state_from_cur = 0;
  a.warm_src = a.in.qacc_warmstart;
  a.stamps = g_stamps;
  if (!a.in.qpos || !a.in.qvel) return fail(-22, "in.qpos and in.qvel are required");
  if ((a.stages & kFromActuation) && !(fin.qM && fin.qLD && fin.qfrc_smooth)) return fail(-22, "the solver phase reads out.qM / out.qLD: both leaves are required");
  if (M.ncon > 0 && M.nefc > 0 && (a.stages & MJH_STAGE_SOLVE) && !fin.contact_dist) return fail(-22, "the solver phase reads out.contact_dist (active-contact row compaction): the leaf is required");
  if (M.ncvxpair > 0 && (a.stages & kFromCollision) && !(fin.contact_dist && fin.contact_pos && fin.contact_frame && fin.geom_xpos && fin.geom_xmat))
    return fail(-22, "models with convex or plane-ellipsoid / plane-cylinder pairs need out.geom_xpos/geom_xmat and out.contact_dist/pos/frame");
  hipStream_t s = (hipStream_t)stream;
  REAL* w = (REAL*)work;
  if (m->hs_reals > 0) {  // (without a workspace the solver reads the leaves, as it always did)
    if (work) { a.hs = w; a.hs_reals = (int)m->hs_reals; }
    w += m->hs_reals * B;
  }
  if (m->cand_reals > 0 && (a.stages & kFromCollision)) {  // max_contact_points over pairs narrow-phased outside the pass (box / mesh, ellipsoid / cylinder): the candidates live at the head of the workspace
    if (!work) return fail(-22, "max_contact_points with box / mesh / ellipsoid / cylinder pairs needs a workspace of mjh_model_work_bytes(m) * B bytes");
    a.cand = w;
    w += m->cand_reals * B;
  }
  if (!do_step || M.integrator == INT_EULER) return forward_pass<REAL>(m, a, s);

  // ---- RK4 (forward.py:331-370): stage 0 computes the returned Data; stages 1..3 run in the workspace Data ----
  if (!work) return fail(-22, "RK4 needs a workspace of mjh_model_work_bytes(m) * B bytes");
  DevData<REAL> scr;
  memset(&scr, 0, sizeof(scr));
  REAL** slots = reinterpret_cast<REAL**>(&scr);
  for (size_t i = 0; i < m->stage_leaf.size(); i++)
    if (m->stage_leaf[i] != STAGE_NONE) {
      if (m->stage_leaf[i] == STAGE_SLOT) slots[i] = w;
      w += m->leaf_count[i] * B;
    }
  a.W.qvel0 = w; w += (int64_t)M.nv * B;
  a.W.kqvel = w; w += (int64_t)M.nv * B;
  a.W.sum_qvel = w; w += (int64_t)M.nv * B;
  a.W.sum_qacc = w; w += (int64_t)M.nv * B;
  a.W.act0 = w; w += (int64_t)M.na * B;
  a.W.sum_actdot = w; w += (int64_t)M.na * B;
  a.nxt = state_of(scr);
  int rc = 0;
  for (int stage = 0; stage < 4; stage++) {
    a.rk_stage = stage;
    if (stage == 0) {
      a.cur = fin; a.state_from_cur = 0; a.warm_src = a.in.qacc_warmstart;
    } else {
      a.cur = scr; a.state_from_cur = 1;
      a.warm_src = (stage == 1) ? fin.qacc_warmstart : scr.qacc_warmstart;  // solver.py:547-552 writes it every pass
    }
    if ((rc = forward_pass<REAL>(m, a, s))) return rc;
  }
  return 0;
}

// inverse dynamics (inverse.py:86-102): the forward pass up to and including the velocity stage, the inverse tail, then the sensors
template <typename REAL>
int run_inverse(const mjhModel* m, const DevModel<REAL>& M, const mjhData* in, mjhData* out, void* qfrc_inverse, void* work, int64_t B, int flags, void* stream) {
  if (B <= 0) return 0;
  const bool discrete = (flags & MJH_FLAG_INV_DISCRETE) != 0;
  if (discrete && M.integrator == INT_RK4) return fail(-22, "discrete inverse dynamics is not supported by RK4 integrator");
  DevData<REAL> o;
  memcpy(&o, out, sizeof(o));
  const REAL* qacc = reinterpret_cast<const REAL*>(in->qacc);
  if (!qacc) return fail(-22, "in.qacc is required");
  if (!qfrc_inverse || !o.qfrc_constraint || !o.qM || !o.qLD || !o.qfrc_bias || !o.qfrc_passive) return fail(-22, "inverse: qfrc_inverse and out.qfrc_constraint / qM / qLD / qfrc_bias / qfrc_passive are required");
  if (M.nefc > 0 && !(o.efc_J && o.efc_D && o.efc_aref && o.efc_force)) return fail(-22, "inverse: out.efc_J / efc_D / efc_aref / efc_force are required");
  // (the hand-over workspace of the register solver is not used: no solver runs.  A workspace is needed only for the max_contact_points candidates, which it holds at its head)
  int rc = run<REAL>(m, M, in, out, m->cand_reals > 0 ? work : nullptr, B, flags & MJH_FLAG_FIXED_ITERATIONS, 0, kUpToVelocity, stream);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  InvArgs<REAL> ia;
  memset(&ia, 0, sizeof(ia));
  ia.efc_J = o.efc_J; ia.efc_D = o.efc_D; ia.efc_aref = o.efc_aref; ia.qM = o.qM; ia.qLD = o.qLD; ia.qfrc_bias = o.qfrc_bias; ia.qfrc_passive = o.qfrc_passive;
  ia.qacc = qacc; ia.dof_damping = M.dof_damping;
  ia.efc_force = o.efc_force; ia.qfrc_constraint = o.qfrc_constraint; ia.qfrc_inverse = reinterpret_cast<REAL*>(qfrc_inverse);
  ia.timestep = M.timestep;
  ia.nv = M.nv; ia.nefc = M.nefc; ia.nalways = M.ne + M.nf + M.nft;
  ia.discrete = (discrete && M.integrator == INT_EULER && !(M.disableflags & DSBL_EULERDAMP) && m->any_damping) ? 1 : 0;
  ia.lanes = m->inv_lanes; ia.envs = m->inv_envs; ia.chunk = m->inv_chunk; ia.lds_env = m->inv_lds_env;
  const size_t lds = (size_t)ia.envs * ia.lds_env * sizeof(REAL);
  if ((rc = launch_cut(B, ia.envs, [&](int64_t first, int64_t n, unsigned grid) {
         ia.env_begin = first; ia.env_count = n;
         hipLaunchKernelGGL((mjh_inverse_kernel<REAL>), dim3(grid), dim3(256), lds, s, ia);
       })))
    return rc;
  timing_mark(s, MJH_KERNEL_INVERSE);
  if (M.nsensor > 0 && o.sensordata) {  // sensor_pos / sensor_vel / sensor_acc: leaves this call does not write (actuator_force, qfrc_actuator) are the caller's
    KArgs<REAL> a;
    memset(&a, 0, sizeof(a));
    a.M = M;
    memcpy(&a.in, in, sizeof(a.in));
    a.cur = o;
    if (!a.cur.actuator_force) a.cur.actuator_force = a.in.actuator_force;
    if (!a.cur.qfrc_actuator) a.cur.qfrc_actuator = a.in.qfrc_actuator;
    a.fin = state_of(o);
    a.B = B; a.flags = flags; a.do_step = 0; a.stages = kUpToVelocity; a.rk_stage = -1; a.state_from_cur = 0;
    a.warm_src = a.in.qacc_warmstart;
    if ((rc = launch_sensor_kernel<REAL>(m, a, s))) return rc;
  }
  return 0;
}

// ray casting (ray.py:375-452): one lane per (environment, ray) pair, the candidates' geom frames staged in LDS chunk by chunk (mjh_ray.h)
template <typename REAL>
int run_ray(const mjhModel* m, const DevModel<REAL>& M, const void* geom_xpos, const void* geom_xmat, const void* pnt, int64_t pnt_env, int64_t pnt_ray,
            const void* vec, int64_t vec_env, int64_t vec_ray, int64_t B, int64_t R, const mjhRayCands* c, void* dist, int64_t* geomid, void* stream) {
  (void)m;
  if (B <= 0 || R <= 0) return B < 0 || R < 0 ? fail(-22, "ray: B and R must be >= 0") : 0;
  if (R > (1 << 30)) return fail(-22, "ray: more than 2^30 rays per environment");
  if (c->ncand < 0 || c->ncand > (1 << 30)) return fail(-22, "ray: bad candidate count");
  if (!geom_xpos || !geom_xmat || !pnt || !vec || !dist || !geomid || (c->ncand > 0 && (!c->cand || !c->geom_size))) return fail(-22, "ray: null pointer");
  hipStream_t s = (hipStream_t)stream;
  timing_begin(s);
  RayArgs<REAL> a;
  memset(&a, 0, sizeof(a));
  a.geom_xpos = reinterpret_cast<const REAL*>(geom_xpos); a.geom_xmat = reinterpret_cast<const REAL*>(geom_xmat);
  a.pnt = reinterpret_cast<const REAL*>(pnt); a.vec = reinterpret_cast<const REAL*>(vec);
  a.pnt_env = pnt_env; a.pnt_ray = pnt_ray; a.vec_env = vec_env; a.vec_ray = vec_ray;
  a.cand = c->cand; a.tri = reinterpret_cast<const REAL*>(c->tri); a.geom_size = reinterpret_cast<const REAL*>(c->geom_size);
  a.dist = reinterpret_cast<REAL*>(dist); a.geomid = geomid;
  a.ngeom = M.ngeom; a.ncand = (int)c->ncand; a.R = (int)R;
  // LDS: the environments one workgroup's 256 consecutive pairs can touch (<= 255 / R + 2, at most 256) x a chunk of candidates x 12 reals, within
  // LDS_BUDGET per workgroup (three workgroups per CU at the worst); a chunk never holds more candidates than there are
  constexpr int LDS_BUDGET = 48 * 1024;
  const int64_t span = R >= 256 ? 2 : (255 / R + 2 < 256 ? 255 / R + 2 : 256);
  int64_t chunk = LDS_BUDGET / (span * 12 * (int64_t)sizeof(REAL));
  if (chunk > c->ncand) chunk = c->ncand;
  if (chunk < 1) chunk = 1;
  a.chunk = (int)chunk;
  const size_t lds = c->ncand > 0 ? (size_t)(span * chunk * 12 * (int64_t)sizeof(REAL)) : 0;
  if (const int rc = launch_cut(B * R, MJH_RAY_WG, [&](int64_t first, int64_t n, unsigned grid) {
        a.env_base = first / R; a.r_base = (int)(first % R); a.npairs = (int)n;
        hipLaunchKernelGGL((mjh_ray_kernel<REAL>), dim3(grid), dim3(MJH_RAY_WG), lds, s, a);
      }))
    return rc;
  timing_mark(s, MJH_KERNEL_RAY);
  return 0;
}

// signed distance and nearest points of geom pairs (mjh_geomdist.h): one lane per (pair, environment), items pair-major, one-wave workgroups
template <typename REAL>
int run_geom_distance(const DevModel<REAL>& M, const void* geom_xpos, const void* geom_xmat, const void* geom_size, const int32_t* pairs, int64_t npair,
                      double distmax, void* dist, void* fromto, int64_t B, void* stream) {
  if (B < 0 || npair < 0) return fail(-22, "geom_distance: B and npair must be >= 0");
  if (!(distmax >= 0)) return fail(-22, "geom_distance: distmax must be >= 0");
  if (B == 0 || npair == 0) return 0;
  if (npair > (1 << 30)) return fail(-22, "geom_distance: more than 2^30 pairs");
  if (M.ngeom <= 0) return fail(-22, "geom_distance: the model has no geoms");
  if (!geom_xpos || !geom_xmat || !geom_size || !pairs || !dist || !fromto) return fail(-22, "geom_distance: null pointer");
  hipStream_t s = (hipStream_t)stream;
  timing_begin(s);
  GeomDistArgs<REAL> a;
  memset(&a, 0, sizeof(a));
  a.geom_xpos = reinterpret_cast<const REAL*>(geom_xpos); a.geom_xmat = reinterpret_cast<const REAL*>(geom_xmat);
  a.geom_size = reinterpret_cast<const REAL*>(geom_size); a.pairs = pairs;
  a.dist = reinterpret_cast<REAL*>(dist); a.fromto = reinterpret_cast<REAL*>(fromto);
  a.B = B; a.ngeom = M.ngeom; a.npair = (int)npair; a.distmax = (REAL)distmax;
  if (const int rc = launch_cut(B * npair, MJH_WAVE, [&](int64_t first, int64_t n, unsigned grid) {
        a.item_begin = first; a.item_count = n;
        hipLaunchKernelGGL((mjh_geomdist_kernel<REAL>), dim3(grid), dim3(MJH_WAVE), 0, s, a);
      }))
    return rc;
  timing_mark(s, MJH_KERNEL_GEOM_DISTANCE);
  return 0;
}

// configuration arithmetic (mjh_qpos.h): one lane per (environment, joint), environment-major, one-wave workgroups
template <typename REAL>
int run_qpos_arith(const DevModel<REAL>& M, int op, const void* qa, const void* qb, double dt, void* out, int64_t B, void* stream) {
  if (op != MJH_QPOS_INTEGRATE && op != MJH_QPOS_DIFFERENTIATE && op != MJH_QPOS_NORMALIZE) return fail(-22, "qpos_arith: unknown op");
  if (B < 0) return fail(-22, "qpos_arith: B must be >= 0");
  if (op == MJH_QPOS_DIFFERENTIATE && !(dt != 0)) return fail(-22, "qpos_arith: differentiate needs dt != 0");
  if (op != MJH_QPOS_NORMALIZE && !(dt == dt)) return fail(-22, "qpos_arith: dt is NaN");
  if (B == 0 || M.njnt == 0) return 0;
  if (B > ((int64_t)1 << 40)) return fail(-22, "qpos_arith: more than 2^40 environments");
  if (!qa || !out || (op != MJH_QPOS_NORMALIZE && !qb)) return fail(-22, "qpos_arith: null pointer");
  hipStream_t s = (hipStream_t)stream;
  timing_begin(s);
  QposArithArgs<REAL> a;
  memset(&a, 0, sizeof(a));
  a.a = reinterpret_cast<const REAL*>(qa); a.b = reinterpret_cast<const REAL*>(qb); a.out = reinterpret_cast<REAL*>(out);
  a.jnt_type = M.jnt_type; a.jnt_qposadr = M.jnt_qposadr; a.jnt_dofadr = M.jnt_dofadr;
  a.njnt = M.njnt; a.nq = M.nq; a.nv = M.nv; a.op = op; a.dt = (REAL)dt;
  if (const int rc = launch_cut(B * M.njnt, MJH_WAVE, [&](int64_t first, int64_t n, unsigned grid) {
        a.item_begin = first; a.item_count = n;
        hipLaunchKernelGGL((mjh_qpos_arith_kernel<REAL>), dim3(grid), dim3(MJH_WAVE), 0, s, a);
      }))
    return rc;
  timing_mark(s, MJH_KERNEL_QPOS_ARITH);
  return 0;
}

// one iteration of site-pose inverse kinematics (mjh_ik.h): one one-wave workgroup per environment
template <typename REAL>
int run_ik_site_step(const DevModel<REAL>& M, const void* cdof, const void* subtree_com, const void* site_xpos, const void* site_xmat, int site, int body,
                     const void* target_pos, int64_t pos_stride, const void* target_quat, int64_t quat_stride, const int32_t* dof_sel, const double* params,
                     int last, void* qpos, void* err_norm, int32_t* steps, unsigned char* done, int64_t B, void* stream) {
  if (B < 0) return fail(-22, "ik_site_step: B must be >= 0");
  if (M.nv <= 0 || M.nsite <= 0) return fail(-22, "ik_site_step: the model has no dofs or no sites");
  if (site < 0 || site >= M.nsite || body < 0 || body >= M.nbody) return fail(-22, "ik_site_step: site or body outside the model");
  if (!target_pos && !target_quat) return fail(-22, "ik_site_step: neither target given");
  if ((pos_stride != 0 && pos_stride != 3) || (quat_stride != 0 && quat_stride != 4)) return fail(-22, "ik_site_step: a target stride is 0 (shared) or the target's length");
  if (!params) return fail(-22, "ik_site_step: null pointer");
  if (!(params[1] > 0)) return fail(-22, "ik_site_step: damping must be > 0");
  if (!(params[2] >= 0) || !(params[3] >= 0) || !(params[0] == params[0])) return fail(-22, "ik_site_step: tol, max_update_norm, rot_weight");
  if (B == 0) return 0;
  if (!cdof || !subtree_com || !site_xpos || !site_xmat || !dof_sel || !qpos || !err_norm || !steps || !done) return fail(-22, "ik_site_step: null pointer");
  hipStream_t s = (hipStream_t)stream;
  timing_begin(s);
  IkSiteArgs<REAL> a;
  memset(&a, 0, sizeof(a));
  a.cdof = reinterpret_cast<const REAL*>(cdof); a.subtree_com = reinterpret_cast<const REAL*>(subtree_com);
  a.site_xpos = reinterpret_cast<const REAL*>(site_xpos); a.site_xmat = reinterpret_cast<const REAL*>(site_xmat);
  a.target_pos = reinterpret_cast<const REAL*>(target_pos); a.target_quat = reinterpret_cast<const REAL*>(target_quat);
  a.sel = dof_sel; a.qpos = reinterpret_cast<REAL*>(qpos); a.err_norm = reinterpret_cast<REAL*>(err_norm); a.steps = steps; a.done = done;
  a.body_dofmask = M.body_dofmask; a.body_rootid = M.body_rootid; a.jnt_type = M.jnt_type; a.jnt_qposadr = M.jnt_qposadr; a.jnt_dofadr = M.jnt_dofadr;
  a.pos_stride = pos_stride; a.quat_stride = quat_stride;
  a.nv = M.nv; a.nq = M.nq; a.njnt = M.njnt; a.nbody = M.nbody; a.nsite = M.nsite; a.mask_words = M.mask_words; a.site = site; a.body = body; a.last = last != 0;
  a.tol = (REAL)params[0]; a.damping = (REAL)params[1]; a.max_update_norm = (REAL)params[2]; a.rot_weight = (REAL)params[3];
  const int mode = (target_pos ? 1 : 0) | (target_quat ? 2 : 0);
  if (const int rc = launch_cut(B, 1, [&](int64_t first, int64_t, unsigned grid) {
        a.env_begin = first;
        if (mode == 1) hipLaunchKernelGGL((mjh_ik_site_kernel<REAL, 1>), dim3(grid), dim3(MJH_WAVE), 0, s, a);
        else if (mode == 2) hipLaunchKernelGGL((mjh_ik_site_kernel<REAL, 2>), dim3(grid), dim3(MJH_WAVE), 0, s, a);
        else hipLaunchKernelGGL((mjh_ik_site_kernel<REAL, 3>), dim3(grid), dim3(MJH_WAVE), 0, s, a);
      }))
    return rc;
  timing_mark(s, MJH_KERNEL_IK_SITE);
  return 0;
}

// the ray-cast renderer (render.py:719-861): one lane per (environment, output pixel), the candidates' geom frames staged in LDS (mjh_render.h)
template <typename REAL>
int run_render(const DevModel<REAL>& M, const void* geom_xpos, const void* geom_xmat, const void* cam_xpos, const void* cam_xmat, const void* light_xpos,
               const void* light_xdir, int64_t B, const mjhRenderScene* sc, const mjhRenderParams* p, void* rgb, void* depth, int64_t* seg, void* stream) {
  if (B < 0) return fail(-22, "render: B must be >= 0");
  if (p->width < 1 || p->height < 1 || p->ssaa < 1) return fail(-22, "render: width, height and ssaa must be >= 1");
  if ((int64_t)p->width * p->height > (1 << 24) || (int64_t)p->ssaa * p->ssaa > 4096) return fail(-22, "render: image or super-sampling too large");
  if (p->camera < 0 || p->camera >= M.ncam) return fail(-22, "render: camera id out of range");
  if (sc->nlight != M.nlight) return fail(-22, "render: the light table does not match the model's nlight");
  if (sc->ncand < 0 || sc->ncand > (1 << 30) || sc->nprim < 0 || sc->nprim > sc->ncand) return fail(-22, "render: bad candidate count");
  if (B == 0) return 0;
  if (!geom_xpos || !geom_xmat || !cam_xpos || !cam_xmat || !rgb || !depth || !seg || (M.nlight > 0 && (!light_xpos || !light_xdir || !sc->light)) ||
      (sc->ncand > 0 && (!sc->cand || !sc->geom_size || !sc->geom_rgba || !sc->geom_matid)))
    return fail(-22, "render: null pointer");
  hipStream_t s = (hipStream_t)stream;
  timing_begin(s);
  RenderArgs<REAL> a;
  memset(&a, 0, sizeof(a));
  a.geom_xpos = reinterpret_cast<const REAL*>(geom_xpos); a.geom_xmat = reinterpret_cast<const REAL*>(geom_xmat);
  a.cam_xpos = reinterpret_cast<const REAL*>(cam_xpos); a.cam_xmat = reinterpret_cast<const REAL*>(cam_xmat);
  a.light_xpos = reinterpret_cast<const REAL*>(light_xpos); a.light_xdir = reinterpret_cast<const REAL*>(light_xdir);
  a.cand = sc->cand; a.tri = reinterpret_cast<const REAL*>(sc->tri); a.geom_size = reinterpret_cast<const REAL*>(sc->geom_size);
  a.geom_rgba = reinterpret_cast<const REAL*>(sc->geom_rgba); a.geom_matid = sc->geom_matid; a.mat_rgba = sc->mat_rgba;
  a.light = reinterpret_cast<const REAL*>(sc->light);
  a.rgb = rgb; a.depth = reinterpret_cast<REAL*>(depth); a.seg = seg;
  a.half_w = (REAL)p->half_w; a.half_h = (REAL)p->half_h; a.fog_start = (REAL)p->fog_start; a.fog_range = (REAL)p->fog_range;
  for (int k = 0; k < 3; k++) { a.fog_color[k] = (REAL)p->fog_color[k]; a.bg[k] = (float)p->background[k]; }
  a.ngeom = M.ngeom; a.ncam = M.ncam; a.nlight = M.nlight; a.cam = p->camera; a.ncand = (int)sc->ncand; a.nprim = (int)sc->nprim;
  a.W = p->width; a.H = p->height; a.ssaa = p->ssaa;
  a.shade = p->shading && M.nlight > 0; a.shadows = p->shadows != 0; a.fog = p->fog != 0; a.rgb_f32 = p->rgb_f32 != 0; a.u8 = p->u8 != 0;
  // LDS: as run_ray, with R = the output pixels of one image
  const int64_t P = (int64_t)p->width * p->height;
  constexpr int LDS_BUDGET = 48 * 1024;
  const int64_t span = P >= 256 ? 2 : (255 / P + 2 < 256 ? 255 / P + 2 : 256);
  int64_t chunk = LDS_BUDGET / (span * 12 * (int64_t)sizeof(REAL));
  if (chunk > sc->ncand) chunk = sc->ncand;
  if (chunk < 1) chunk = 1;
  a.chunk = (int)chunk;
  const size_t lds = sc->ncand > 0 ? (size_t)(span * chunk * 12 * (int64_t)sizeof(REAL)) : 0;
  if (const int rc = launch_cut(B * P, MJH_RENDER_WG, [&](int64_t first, int64_t n, unsigned grid) {
        a.env_base = first / P; a.r_base = (int)(first % P); a.npairs = (int)n;
        hipLaunchKernelGGL((mjh_render_kernel<REAL>), dim3(grid), dim3(MJH_RENDER_WG), lds, s, a);
      }))
    return rc;
  timing_mark(s, MJH_KERNEL_RENDER);
  return 0;
}

// the support functions (support.py:138-194, smooth.py:335-374) on a finished forward pass' leaves (mjh_support.h)
template <typename REAL>
int run_support(const mjhModel* m, const DevModel<REAL>& M, const mjhSupportArgs* x, void* stream) {
  (void)m;
  const int op = x->op, nv = M.nv;
  if (op < MJH_SUPPORT_JAC || op > MJH_SUPPORT_SOLVE_M) return fail(-22, "support: unknown op");
  if (x->B < 0) return fail(-22, "support: B must be >= 0");
  const bool pt = op == MJH_SUPPORT_JAC || op == MJH_SUPPORT_APPLY_FT, mv = op == MJH_SUPPORT_MUL_M || op == MJH_SUPPORT_SOLVE_M;
  if (pt && (x->P < 1 || (int64_t)x->P * nv * 3 >= (1 << 30))) return fail(-22, "support: bad query count P");
  if (mv && (x->K < 1 || (int64_t)x->K * nv >= (1 << 30))) return fail(-22, "support: bad vector count K");
  if (pt && x->body_stride != 0 && x->body_stride != 1) return fail(-22, "support: body_stride must be 0 or 1");
  if (x->B == 0 || nv == 0) return 0;
  if (!x->out0 || (op == MJH_SUPPORT_JAC && !x->out1) || ((pt || op == MJH_SUPPORT_XFRC) && (!x->cdof || !x->subtree_com)) ||
      (pt && (!x->body_id || !x->point)) || (op == MJH_SUPPORT_APPLY_FT && (!x->force || !x->torque)) ||
      (op == MJH_SUPPORT_XFRC && (!x->xipos || !x->xfrc_applied)) || (op == MJH_SUPPORT_MUL_M && !x->qM) || (op == MJH_SUPPORT_SOLVE_M && !x->qLD) ||
      (mv && !x->vec))
    return fail(-22, "support: null pointer");
  hipStream_t s = (hipStream_t)stream;
  timing_begin(s);
  SupArgs<REAL> a;
  memset(&a, 0, sizeof(a));
  a.cdof = reinterpret_cast<const REAL*>(x->cdof); a.subtree_com = reinterpret_cast<const REAL*>(x->subtree_com);
  a.xipos = reinterpret_cast<const REAL*>(x->xipos); a.xfrc = reinterpret_cast<const REAL*>(x->xfrc_applied);
  a.mat = reinterpret_cast<const REAL*>(op == MJH_SUPPORT_MUL_M ? x->qM : x->qLD);
  a.point = reinterpret_cast<const REAL*>(x->point); a.force = reinterpret_cast<const REAL*>(x->force);
  a.torque = reinterpret_cast<const REAL*>(x->torque); a.vec = reinterpret_cast<const REAL*>(x->vec);
  a.body = x->body_id; a.body_stride = (int)x->body_stride;
  a.body_dofmask = M.body_dofmask; a.body_rootid = M.body_rootid;
  a.out0 = reinterpret_cast<REAL*>(x->out0); a.out1 = reinterpret_cast<REAL*>(x->out1);
  a.point_env = x->point_env; a.point_q = x->point_q; a.force_env = x->force_env; a.force_q = x->force_q;
  a.torque_env = x->torque_env; a.torque_q = x->torque_q; a.vec_env = x->vec_env; a.vec_k = x->vec_k;
  a.nv = nv; a.nbody = M.nbody; a.mask_words = M.mask_words; a.P = x->P; a.K = x->K;
  if (pt || op == MJH_SUPPORT_XFRC) {  // one lane per output element; a launch starts at (env_base, r_base) so that the lanes index in 32 bits
    const int64_t per_env = op == MJH_SUPPORT_JAC ? (int64_t)x->P * nv * 3 : op == MJH_SUPPORT_APPLY_FT ? (int64_t)x->P * nv : nv;
    const int rc = launch_cut(x->B * per_env, MJH_SUP_WG, [&](int64_t first, int64_t n, unsigned grid) {
      a.env_base = first / per_env; a.r_base = (int)(first % per_env); a.count = (int)n;
      if (op == MJH_SUPPORT_JAC) hipLaunchKernelGGL((mjh_sup_point_kernel<REAL, true>), dim3(grid), dim3(MJH_SUP_WG), 0, s, a);
      else if (op == MJH_SUPPORT_APPLY_FT) hipLaunchKernelGGL((mjh_sup_point_kernel<REAL, false>), dim3(grid), dim3(MJH_SUP_WG), 0, s, a);
      else hipLaunchKernelGGL((mjh_sup_xfrc_kernel<REAL>), dim3(grid), dim3(MJH_SUP_WG), 0, s, a);
    });
    if (rc) return rc;
  } else {  // one wavefront per environment, the matrix staged in LDS
    constexpr int64_t kChunkBytes = 32 * 1024, kVecBytes = 16 * 1024, kMaxLds = 160 * 1024;
    const int64_t rb = (int64_t)nv * sizeof(REAL);
    int64_t lds;
    if (op == MJH_SUPPORT_MUL_M) {  // qM rows per chunk
      int64_t c = kChunkBytes / rb;
      a.chunk = (int)(c < 1 ? 1 : (c > nv ? nv : c));
      lds = a.chunk * rb;
    } else {  // the packed triangle + vectors per chunk
      int64_t c = kVecBytes / rb;
      a.chunk = (int)(c < 1 ? 1 : (c > x->K ? x->K : c));
      lds = ((int64_t)nv * (nv + 1) / 2 + (int64_t)a.chunk * nv) * sizeof(REAL);
      if (lds > kMaxLds) return fail(-22, "support: solve_m needs more LDS than a workgroup has (nv too large)");
      if (lds > 64 * 1024) HIP_TRY(allow_lds(&mjh_sup_solvem_kernel<REAL>, (int)lds));
    }
    const int rc = launch_cut(x->B, 1, [&](int64_t first, int64_t, unsigned grid) {
      a.env_base = first;
      if (op == MJH_SUPPORT_MUL_M) hipLaunchKernelGGL((mjh_sup_mulm_kernel<REAL>), dim3(grid), dim3(MJH_WAVE), (size_t)lds, s, a);
      else hipLaunchKernelGGL((mjh_sup_solvem_kernel<REAL>), dim3(grid), dim3(MJH_WAVE), (size_t)lds, s, a);
    });
    if (rc) return rc;
  }
  timing_mark(s, MJH_KERNEL_JAC + op);
  return 0;
}

// The kernels that stage efc_J in LDS (mjh_efc.h, mjh_dual.h): a workgroup is one wavefront, and small chunks keep many of them on a compute unit.
constexpr int64_t kChunkBytes = 16 * 1024, kMaxLds = 160 * 1024;

// out[0 .. 2] = rows of efc_J per LDS chunk (a staged row takes nv | 1 reals; never more than `most`, the rows worth holding at once), the number of chunks and
// the rows of the last one; returns the chunk.
static int64_t efc_chunks(int nv, int nefc, int64_t most, int real_bytes, int* out) {
  const int64_t rb = (int64_t)(nv | 1) * real_bytes;
  const int64_t chunk = std::max<int64_t>(1, std::min(kChunkBytes / rb, std::max<int64_t>(most, 1)));
  const int64_t nchunk = nefc > 0 ? (nefc + chunk - 1) / chunk : 0, last = nefc > 0 ? nefc - (nchunk - 1) * chunk : 0;
  out[0] = (int)chunk; out[1] = (int)nchunk; out[2] = (int)last;
  return chunk;
}

// out[3] = the bytes of LDS that hold `reals`; returns 0, or -12 when they do not fit kMaxLds
static int efc_lds(int64_t reals, int real_bytes, int* out) {
  const int64_t lds = (reals * real_bytes + 15) & ~(int64_t)15;
  out[3] = (int)std::min<int64_t>(lds, INT32_MAX);
  return lds > kMaxLds ? -12 : 0;
}

// The chunk plan of mjh_constraint_space (mjh_efc.h): rows of efc_J per LDS chunk (a staged row takes nv | 1 reals), the number of chunks, the rows of the last
// one and the LDS of a workgroup.  MUL_J: the chunk alone; MUL_JT: and 64 partial sums.  UPDATE: qacc, J^T force, M qacc, the chunk's forces, the chunk, which also stages qM, and 64 partial sums.
// AR: the packed triangle of qLD and one chunk, two when there is more than one.  Returns 0, or -12 when AR does not fit kMaxLds.
static int efc_plan(int op, int nv, int nefc, int real_bytes, int* out) {
  const int64_t ld = nv | 1;
  int plan[4];
  const int64_t chunk = efc_chunks(nv, nefc, op == MJH_EFC_UPDATE ? std::max(nefc, nv) : nefc, real_bytes, plan);
  int64_t reals = chunk * ld;
  if (op == MJH_EFC_UPDATE) reals += 3 * (int64_t)nv + chunk;
  if (op == MJH_EFC_UPDATE || op == MJH_EFC_MUL_JT) reals += MJH_WAVE;  // the partial sums of efc_jt_accumulate
  if (op == MJH_EFC_AR) reals = (int64_t)nv * (nv + 1) / 2 + (plan[1] > 1 ? 2 : 1) * chunk * ld;
  if (efc_lds(reals, real_bytes, plan)) return -12;  // (out stays as it came)
  std::copy(plan, plan + 4, out);
  return 0;
}

// the constraint-space functions on a finished pass' leaves (mjh_efc.h): one wavefront per environment
template <typename REAL>
int run_constraint_space(const DevModel<REAL>& M, const mjhConstraintSpaceArgs* x, void* stream) {
  const int op = x->op, nv = M.nv, n = M.nefc;
  if (op < MJH_EFC_MUL_J || op > MJH_EFC_AR) return fail(-22, "constraint_space: unknown op");
  if (x->B < 0) return fail(-22, "constraint_space: B must be >= 0");
  const bool mv = op == MJH_EFC_MUL_J || op == MJH_EFC_MUL_JT;
  if (mv && (x->K < 1 || (int64_t)x->K * std::max(nv, n) >= (1 << 30))) return fail(-22, "constraint_space: bad vector count K");
  if (op == MJH_EFC_UPDATE && (x->ne_nf < 0 || x->ne_nf > n)) return fail(-22, "constraint_space: ne_nf outside [0, nefc]");
  if (op == MJH_EFC_UPDATE && x->qacc && !(x->meaninertia > 0)) return fail(-22, "constraint_space: meaninertia must be > 0");
  if (x->B == 0 || nv == 0 || n == 0) return 0;
  if (!x->efc_J || (mv && (!x->vec || !x->out))) return fail(-22, "constraint_space: null pointer");
  if (op == MJH_EFC_UPDATE) {
    if (!x->efc_D || !x->efc_frictionloss || !x->efc_force || !x->efc_state || !x->qfrc_constraint || !x->cost)
      return fail(-22, "constraint_space: null pointer (update leaves)");
    if (x->qacc ? (x->jar_in || !x->efc_aref || !x->qM || !x->qfrc_smooth || !x->qacc_smooth || !x->jar || !x->gauss || !x->grad || !x->grad_norm) : !x->jar_in)
      return fail(-22, "constraint_space: update takes qacc with efc_aref, qM, qfrc_smooth, qacc_smooth and its outputs, or jar_in alone");
  }
  if (op == MJH_EFC_AR && (!x->efc_D || !x->efc_aref || !x->qLD || !x->qacc_smooth || !x->AR || !x->b)) return fail(-22, "constraint_space: null pointer (AR leaves)");
  int plan[4];
  if (efc_plan(op, nv, n, (int)sizeof(REAL), plan)) return fail(-12, "constraint_space: qLD's triangle and two row chunks do not fit the LDS of a workgroup (nv too large)");
  hipStream_t s = (hipStream_t)stream;
  timing_begin(s);
  EfcArgs<REAL> a;
  memset(&a, 0, sizeof(a));
  a.J = reinterpret_cast<const REAL*>(x->efc_J); a.D = reinterpret_cast<const REAL*>(x->efc_D); a.aref = reinterpret_cast<const REAL*>(x->efc_aref);
  a.fl = reinterpret_cast<const REAL*>(x->efc_frictionloss); a.qM = reinterpret_cast<const REAL*>(x->qM); a.qLD = reinterpret_cast<const REAL*>(x->qLD);
  a.qfrc_smooth = reinterpret_cast<const REAL*>(x->qfrc_smooth); a.qacc_smooth = reinterpret_cast<const REAL*>(x->qacc_smooth);
  a.qacc = reinterpret_cast<const REAL*>(x->qacc); a.jar_in = reinterpret_cast<const REAL*>(x->jar_in); a.vec = reinterpret_cast<const REAL*>(x->vec);
  a.out = reinterpret_cast<REAL*>(x->out); a.jar = reinterpret_cast<REAL*>(x->jar); a.force = reinterpret_cast<REAL*>(x->efc_force); a.state = x->efc_state;
  a.qfrc_constraint = reinterpret_cast<REAL*>(x->qfrc_constraint); a.cost = reinterpret_cast<REAL*>(x->cost); a.gauss = reinterpret_cast<REAL*>(x->gauss);
  a.grad = reinterpret_cast<REAL*>(x->grad); a.grad_norm = reinterpret_cast<REAL*>(x->grad_norm); a.AR = reinterpret_cast<REAL*>(x->AR); a.b = reinterpret_cast<REAL*>(x->b);
  a.vec_env = x->vec_env; a.vec_k = x->vec_k;
  a.nv = nv; a.nefc = n; a.K = x->K; a.ne_nf = x->ne_nf; a.floss = x->floss != 0; a.chunk = plan[0];
  a.inv_scale = (REAL)(1.0 / (x->meaninertia * std::max(1, nv)));
  const size_t lds = (size_t)plan[3];
  void (*kernel)(EfcArgs<REAL>) = op == MJH_EFC_MUL_J ? &mjh_efc_mulj_kernel<REAL> : op == MJH_EFC_MUL_JT ? &mjh_efc_muljt_kernel<REAL>
                                  : op == MJH_EFC_UPDATE ? &mjh_efc_update_kernel<REAL> : &mjh_efc_ar_kernel<REAL>;
  if (lds > 64 * 1024) HIP_TRY(allow_lds(kernel, (int)lds));
  if (const int rc = launch_cut(x->B, 1, [&](int64_t first, int64_t, unsigned grid) {
        a.env_base = first;
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(MJH_WAVE), lds, s, a);
      }))
    return rc;
  timing_mark(s, MJH_KERNEL_EFC_MUL_J + op);
  return 0;
}

// The plan of mjh_pgs (ncon = 0) and mjh_noslip (mjh_dual.h): rows of efc_J per staging step (as mjh_constraint_space stages them), the number of steps, the rows of
// the last one and the LDS of a workgroup: the packed triangle of qLD, all nefc rows of W, five reals a row (R, b, the friction bound, w_i . w_i, f), y and J^T f,
// 64 partial sums, and per contact slot the block(s) of A (15 reals), mu (5 reals) and the table entry (two ints, counted as two reals).  Returns 0, or -12 when
// that does not fit kMaxLds (out is filled all the same).
static int dual_plan(int nv, int nefc, int ncon, int real_bytes, int* out) {
  efc_chunks(nv, nefc, nefc, real_bytes, out);
  return efc_lds((int64_t)nv * (nv + 1) / 2 + (int64_t)nefc * (nv | 1) + 5 * (int64_t)nefc + 2 * (int64_t)nv + MJH_WAVE + (MJH_NOSLIP_BLOCK + 5 + 2) * (int64_t)ncon,
                 real_bytes, out);
}

// mjh_pgs and mjh_noslip on a finished pass' leaves (mjh_pgs.h, mjh_noslip.h; X: mjhPgsArgs or mjhNoslipArgs): one wavefront per environment.  `noslip`: force0 is
// required, the model's contact tables and cone go along with `friction` (x->contact_friction), and the kernel is mjh_noslip_kernel.
template <typename REAL, typename X>
int run_dual(const DevModel<REAL>& M, const X* x, void* stream, bool noslip, const void* friction) {
  const std::string who = noslip ? "noslip" : "pgs";
  const int nv = M.nv, n = M.nefc, ncon = noslip ? M.ncon : 0;
  if (x->B < 0) return fail(-22, who + ": B must be >= 0");
  if (x->iterations < 0) return fail(-22, who + ": iterations must be >= 0");
  if (x->ne < 0 || x->nf < 0 || x->ne + x->nf > n) return fail(-22, who + ": ne + nf outside [0, nefc]");
  if (!(x->meaninertia > 0)) return fail(-22, who + ": meaninertia must be > 0");
  if (!(x->tolerance >= 0)) return fail(-22, who + ": tolerance must be >= 0");
  if (x->force0_env != 0 && x->force0_env < n) return fail(-22, who + ": force0_env must be 0 (shared) or at least nefc");
  if (x->B == 0 || nv == 0 || n == 0) return 0;
  const bool elliptic = noslip && M.cone == CONE_ELLIPTIC;
  if (!x->efc_J || !x->efc_D || !x->efc_aref || !x->efc_frictionloss || !x->qLD || !x->qacc_smooth || !x->efc_force || !x->qfrc_constraint || !x->qacc || !x->cost ||
      !x->improvement || !x->niter || (noslip && !x->force0) || (elliptic && ncon > 0 && !friction))
    return fail(-22, who + ": null pointer");
  int plan[4];
  if (dual_plan(nv, n, ncon, (int)sizeof(REAL), plan)) {
    char msg[240];
    if (noslip)
      snprintf(msg, sizeof(msg), "noslip: nv = %d, nefc = %d, ncon = %d need %d bytes of LDS (qLD's triangle, all nefc rows of nv | 1 reals, 22 reals a contact); a workgroup has %d",
               nv, n, ncon, plan[3], (int)kMaxLds);
    else
      snprintf(msg, sizeof(msg), "pgs: nv = %d, nefc = %d need %d bytes of LDS (qLD's triangle and all nefc rows of nv | 1 reals); a workgroup has %d", nv, n, plan[3],
               (int)kMaxLds);
    return fail(-12, msg);
  }
  hipStream_t s = (hipStream_t)stream;
  timing_begin(s);
  NoslipArgs<REAL> a;  // (mjh_pgs launches its DualArgs part)
  memset(&a, 0, sizeof(a));
  a.J = reinterpret_cast<const REAL*>(x->efc_J); a.D = reinterpret_cast<const REAL*>(x->efc_D); a.aref = reinterpret_cast<const REAL*>(x->efc_aref);
  a.fl = reinterpret_cast<const REAL*>(x->efc_frictionloss); a.qLD = reinterpret_cast<const REAL*>(x->qLD); a.qacc_smooth = reinterpret_cast<const REAL*>(x->qacc_smooth);
  a.force0 = reinterpret_cast<const REAL*>(x->force0); a.force0_env = x->force0_env;
  a.force = reinterpret_cast<REAL*>(x->efc_force); a.qfrc_constraint = reinterpret_cast<REAL*>(x->qfrc_constraint); a.qacc = reinterpret_cast<REAL*>(x->qacc);
  a.cost = reinterpret_cast<REAL*>(x->cost); a.improvement = reinterpret_cast<REAL*>(x->improvement); a.niter = x->niter;
  a.tolerance = (REAL)x->tolerance; a.inv_scale = (REAL)(1.0 / (x->meaninertia * std::max(1, nv)));
  a.nv = nv; a.nefc = n; a.ne = x->ne; a.nf = x->nf; a.iterations = x->iterations; a.chunk = plan[0];
  if (noslip) {
    a.friction = reinterpret_cast<const REAL*>(friction); a.con_dim = M.con_dim; a.con_adr = M.con_efc_address; a.ncon = ncon; a.elliptic = elliptic ? 1 : 0;
  }
  const size_t lds = (size_t)plan[3];
  if (lds > 64 * 1024 && noslip) HIP_TRY(allow_lds(&mjh_noslip_kernel<REAL>, (int)lds));
  if (lds > 64 * 1024 && !noslip) HIP_TRY(allow_lds(&mjh_pgs_kernel<REAL>, (int)lds));
  if (const int rc = launch_cut(x->B, 1, [&](int64_t first, int64_t, unsigned grid) {
        a.env_base = first;
        PgsArgs<REAL> p;
        static_cast<DualArgs<REAL>&>(p) = a;
        if (noslip) hipLaunchKernelGGL(mjh_noslip_kernel<REAL>, dim3(grid), dim3(MJH_WAVE), lds, s, a);
        else hipLaunchKernelGGL(mjh_pgs_kernel<REAL>, dim3(grid), dim3(MJH_WAVE), lds, s, p);
      }))
    return rc;
  timing_mark(s, noslip ? MJH_KERNEL_NOSLIP : MJH_KERNEL_PGS);
  return 0;
}

// The plan of mjh_solve (mjh_solve.h): rows of efc_J per staging step (as mjh_constraint_space stages them), the number of steps, the rows of the last one and the LDS of
// a workgroup: two packed triangles (qM; qLD, or Newton's H and its factor), all nefc rows of J, five reals a row (D, frictionloss, jar, jv, force; Newton: and D active),
// MJH_SOLVE_DOF_VECTORS dof vectors and 64 partial sums.  Returns 0, or -12 when that does not fit kMaxLds (out is filled all the same).
static int solve_plan(int solver, int nv, int nefc, int real_bytes, int* out) {
  efc_chunks(nv, nefc, nefc, real_bytes, out);
  return efc_lds((int64_t)nv * (nv + 1) + (int64_t)nefc * (nv | 1) + (solver == MJH_SOLVER_NEWTON ? 6 : 5) * (int64_t)nefc + MJH_SOLVE_DOF_VECTORS * (int64_t)nv + MJH_WAVE,
                 real_bytes, out);
}

// mjh_solve on a finished pass' leaves (mjh_solve.h): one wavefront per environment
template <typename REAL>
int run_solve(const DevModel<REAL>& M, const mjhSolveArgs* x, void* stream) {
  const int nv = M.nv, n = M.nefc;
  if (x->B < 0) return fail(-22, "solve: B must be >= 0");
  if (x->solver != MJH_SOLVER_CG && x->solver != MJH_SOLVER_NEWTON) return fail(-22, "solve: solver must be 1 (CG) or 2 (Newton)");
  if (x->iterations < 0 || x->ls_iterations < 0) return fail(-22, "solve: iterations and ls_iterations must be >= 0");
  if (x->ne < 0 || x->nf < 0 || x->ne + x->nf > n) return fail(-22, "solve: ne + nf outside [0, nefc]");
  if (!(x->meaninertia > 0)) return fail(-22, "solve: meaninertia must be > 0");
  if (!(x->tolerance >= 0) || !(x->ls_tolerance >= 0)) return fail(-22, "solve: tolerance and ls_tolerance must be >= 0");
  if (x->B == 0 || nv == 0 || n == 0) return 0;
  const bool newton = x->solver == MJH_SOLVER_NEWTON;
  if (!x->efc_J || !x->efc_D || !x->efc_aref || !x->efc_frictionloss || !x->qM || (!newton && !x->qLD) || !x->qfrc_smooth || !x->qacc_smooth ||
      (x->warmstart && !x->qacc_warmstart) || !x->qacc_out || !x->qacc_warmstart_out || !x->qfrc_constraint_out || !x->efc_force_out || !x->cost || !x->improvement ||
      !x->grad_norm || !x->niter)
    return fail(-22, "solve: null pointer");
  int plan[4];
  if (solve_plan(x->solver, nv, n, (int)sizeof(REAL), plan)) {
    char msg[240];
    snprintf(msg, sizeof(msg), "solve: nv = %d, nefc = %d, solver = %s need %d bytes of LDS (two packed triangles and all nefc rows of nv | 1 reals); a workgroup has %d", nv, n,
             newton ? "NEWTON" : "CG", plan[3], (int)kMaxLds);
    return fail(-12, msg);
  }
  hipStream_t s = (hipStream_t)stream;
  timing_begin(s);
  SolveArgs<REAL> a;
  memset(&a, 0, sizeof(a));
  a.J = reinterpret_cast<const REAL*>(x->efc_J); a.D = reinterpret_cast<const REAL*>(x->efc_D); a.aref = reinterpret_cast<const REAL*>(x->efc_aref);
  a.fl = reinterpret_cast<const REAL*>(x->efc_frictionloss); a.qM = reinterpret_cast<const REAL*>(x->qM); a.qLD = reinterpret_cast<const REAL*>(x->qLD);
  a.qfrc_smooth = reinterpret_cast<const REAL*>(x->qfrc_smooth); a.qacc_smooth = reinterpret_cast<const REAL*>(x->qacc_smooth);
  a.qacc_warmstart = reinterpret_cast<const REAL*>(x->qacc_warmstart);
  a.qacc = reinterpret_cast<REAL*>(x->qacc_out); a.qacc_warmstart_out = reinterpret_cast<REAL*>(x->qacc_warmstart_out);
  a.qfrc_constraint = reinterpret_cast<REAL*>(x->qfrc_constraint_out); a.force = reinterpret_cast<REAL*>(x->efc_force_out); a.cost = reinterpret_cast<REAL*>(x->cost);
  a.improvement = reinterpret_cast<REAL*>(x->improvement); a.grad_norm = reinterpret_cast<REAL*>(x->grad_norm); a.niter = x->niter;
  a.tolerance = (REAL)x->tolerance; a.ls_gtol = (REAL)(x->tolerance * x->ls_tolerance); a.scale = (REAL)(x->meaninertia * std::max(1, nv));
  a.nv = nv; a.nefc = n; a.ne_nf = x->ne + x->nf; a.floss = x->floss != 0; a.newton = newton; a.iterations = x->iterations; a.ls_iterations = x->ls_iterations;
  a.fixed = x->fixed != 0; a.warmstart = x->warmstart != 0; a.chunk = plan[0];
  const size_t lds = (size_t)plan[3];
  if (lds > 64 * 1024) HIP_TRY(allow_lds(&mjh_solve_kernel<REAL>, (int)lds));
  if (const int rc = launch_cut(x->B, 1, [&](int64_t first, int64_t, unsigned grid) {
        a.env_base = first;
        hipLaunchKernelGGL(mjh_solve_kernel<REAL>, dim3(grid), dim3(MJH_WAVE), lds, s, a);
      }))
    return rc;
  timing_mark(s, MJH_KERNEL_SOLVE);
  return 0;
}

// The tail of the kernels that give every workgroup a.envs environments of a.lanes lanes and a.lds_env reals of LDS each (postcon, consens, energy, integrate): the
// batch goes out in cuts of environments [env_begin, env_begin + env_count), timed as kernel `id`.  The caller has made its last refusal.
template <typename REAL, template <typename> class Args>
int launch_envs(void (*kernel)(Args<REAL>), Args<REAL>& a, int64_t B, hipStream_t s, int id) {
  const size_t lds = (size_t)a.envs * a.lds_env * sizeof(REAL);
  timing_begin(s);
  if (const int rc = launch_cut(B, a.envs, [&](int64_t first, int64_t n, unsigned grid) {
        a.env_begin = first; a.env_count = n;
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(a.envs * a.lanes), lds, s, a);
      }))
    return rc;
  timing_mark(s, id);
  return 0;
}

// a.n = x->n as a pointer to (const) REAL: how the run_* functions from here to run_integrate copy the leaves of an ABI args struct into a kernel's
#define P_(n) a.n = reinterpret_cast<const REAL*>(x->n);
#define O_(n) a.n = reinterpret_cast<REAL*>(x->n);

// body accelerations and forces of a finished forward pass (mjh_postcon.h): MuJoCo's mj_rnePostConstraint / mj_subtreeVel and the sensors that read them, one launch
template <typename REAL>
int run_postcon(const mjhModel* m, const DevModel<REAL>& M, const mjhPostconArgs* x, void* stream) {
  const int f = x->flags;
  if (f <= 0 || f > (MJH_POSTCON_RNE | MJH_POSTCON_SUBTREE | MJH_POSTCON_SENSORS)) return fail(-22, "postconstraint: unknown flags");
  if ((f & MJH_POSTCON_SENSORS) && (f & (MJH_POSTCON_RNE | MJH_POSTCON_SUBTREE)) != (MJH_POSTCON_RNE | MJH_POSTCON_SUBTREE))
    return fail(-22, "postconstraint: the sensors need both the rne and the subtree part");
  if (x->B < 0) return fail(-22, "postconstraint: B must be >= 0");
  if (x->B == 0) return 0;
  if (m->pc_envs == 0) return fail(-12, "postconstraint: the model's bodies and contacts do not fit the LDS of one workgroup");
  const bool rne = f & MJH_POSTCON_RNE, sub = f & MJH_POSTCON_SUBTREE, sns = (f & MJH_POSTCON_SENSORS) && M.nsensordata > 0;
  if (!x->cvel || !x->xipos || !x->subtree_com) return fail(-22, "postconstraint: null pointer (cvel / xipos / subtree_com)");
  if (rne && (!x->cinert || !x->xfrc_applied || !x->cacc || !x->cfrc_int || !x->cfrc_ext || (M.nv > 0 && (!x->qvel || !x->qacc || !x->cdof || !x->cdof_dot)) ||
              (M.ncon > 0 && M.nefc > 0 && (!x->efc_force || !x->contact_pos || !x->contact_frame || !x->contact_friction || !x->contact_dim || !x->contact_geom || !x->contact_efc_address))))
    return fail(-22, "postconstraint: null pointer (rne leaves)");
  if (sub && (!x->ximat || !x->body_subtreemass || !x->subtree_linvel || !x->subtree_angmom)) return fail(-22, "postconstraint: null pointer (subtree leaves)");
  if (sns && (!x->sensordata_in || !x->sensordata || (M.nsite > 0 && (!x->site_xpos || !x->site_xmat)))) return fail(-22, "postconstraint: null pointer (sensor leaves)");
  PostconArgs<REAL> a;
  memset(&a, 0, sizeof(a));
  P_(qvel) P_(qacc) P_(cdof) P_(cdof_dot) P_(cvel) P_(cinert) P_(xipos) P_(ximat) P_(subtree_com) P_(efc_force) P_(contact_pos) P_(contact_frame) P_(contact_friction)
  P_(site_xpos) P_(site_xmat) P_(sensordata_in) P_(body_subtreemass)
  a.xfrc = reinterpret_cast<const REAL*>(x->xfrc_applied);
  a.contact_dim = x->contact_dim; a.contact_geom = x->contact_geom; a.contact_efc_address = x->contact_efc_address;
  a.body_parentid = M.body_parentid; a.body_rootid = M.body_rootid; a.body_dofadr = M.body_dofadr; a.body_dofnum = M.body_dofnum; a.body_depth = M.body_depth;
  a.body_chain = M.body_chain; a.body_subtree_end = M.body_subtree_end; a.geom_bodyid = M.geom_bodyid;
  a.sns_type = M.sns_type; a.sns_adr = M.sns_adr; a.sns_objid = M.sns_objid; a.sns_bodyid = M.sns_bodyid; a.sns_rootid = M.sns_rootid; a.sns_datatype = M.sns_datatype;
  a.slot_sensor = M.slot_sensor; a.body_mass = M.body_mass; a.body_inertia = M.body_inertia; a.sns_cutoff = M.sns_cutoff;
  O_(cacc) O_(cfrc_int) O_(cfrc_ext) O_(subtree_linvel) O_(subtree_angmom) O_(sensordata)
  const bool nograv = M.disableflags & DSBL_GRAVITY;
  for (int k = 0; k < 3; k++) a.cacc0[k] = nograv ? (REAL)0 : -M.gravity[k];
  a.nbody = M.nbody; a.nv = M.nv; a.nefc = M.nefc; a.ngeom = M.ngeom; a.nsite = M.nsite; a.nsensordata = M.nsensordata; a.max_depth = M.max_depth;
  a.ncon = M.nefc > 0 ? M.ncon : 0;  // (without constraint rows there is no force to gather)
  a.pyramidal = M.cone != CONE_ELLIPTIC;
  a.flags = (rne ? MJH_POSTCON_RNE : 0) | (sub ? MJH_POSTCON_SUBTREE : 0) | (sns ? MJH_POSTCON_SENSORS : 0);
  a.lanes = m->pc_lanes; a.envs = m->pc_envs; a.lds_env = m->pc_lds_env;
  return launch_envs(mjh_postcon_kernel<REAL>, a, x->B, (hipStream_t)stream, MJH_KERNEL_POSTCON);
}

// contact forces and the touch / framelinacc / frameangacc sensors of a finished forward pass (mjh_contact_sensors.h), one launch
template <typename REAL>
int run_consens(const mjhModel* m, const DevModel<REAL>& M, const mjhContactSensorArgs* x, void* stream) {
  const int f = x->flags;
  if (f <= 0 || f > (MJH_CONSENS_FORCES | MJH_CONSENS_SENSORS | MJH_CONSENS_WORLD) || !(f & (MJH_CONSENS_FORCES | MJH_CONSENS_SENSORS)))
    return fail(-22, "contact_sensors: unknown flags");
  if ((f & MJH_CONSENS_WORLD) && !(f & MJH_CONSENS_FORCES)) return fail(-22, "contact_sensors: the world frame applies to the forces");
  if (x->B < 0 || x->nsens < 0) return fail(-22, "contact_sensors: B and nsens must be >= 0");
  if (x->B == 0) return 0;
  if (!m->cs_ok) return fail(-12, "contact_sensors: the model's contacts do not fit the LDS of one workgroup");
  const int ncon = M.nefc > 0 ? M.ncon : 0;  // (without constraint rows there is no force to decode)
  const bool forces = (f & MJH_CONSENS_FORCES) && ncon > 0, sns = (f & MJH_CONSENS_SENSORS) && x->nsens > 0 && M.nsensordata > 0;
  if (!forces && !sns) return 0;
  if (ncon > 0 && (!x->efc_force || !x->contact_pos || !x->contact_frame || !x->contact_friction || !x->contact_dim || !x->contact_geom || !x->contact_efc_address))
    return fail(-22, "contact_sensors: null pointer (contact leaves)");
  if (forces && !x->force) return fail(-22, "contact_sensors: null pointer (force)");
  if (sns && (!x->sns || !x->sns_cutoff || !x->sensordata || !x->cvel || !x->cacc || !x->subtree_com || !x->xipos || !x->xpos || (M.ngeom > 0 && !x->geom_xpos) ||
              (M.nsite > 0 && (!x->site_xpos || !x->site_xmat || !x->site_size)) || (M.ncam > 0 && !x->cam_xpos)))
    return fail(-22, "contact_sensors: null pointer (sensor leaves)");
  ConSensArgs<REAL> a;
  memset(&a, 0, sizeof(a));
  P_(efc_force) P_(contact_pos) P_(contact_frame) P_(contact_friction) P_(site_xpos) P_(site_xmat) P_(cvel) P_(cacc) P_(subtree_com) P_(xipos) P_(xpos) P_(geom_xpos)
  P_(cam_xpos) P_(site_size) P_(sns_cutoff)
  a.contact_dim = x->contact_dim; a.contact_geom = x->contact_geom; a.contact_efc_address = x->contact_efc_address;
  a.geom_bodyid = M.geom_bodyid; a.sns = x->sns;
  a.force = reinterpret_cast<REAL*>(x->force); a.sensordata = reinterpret_cast<REAL*>(x->sensordata);
  a.nbody = M.nbody; a.ncon = ncon; a.nefc = M.nefc; a.ngeom = M.ngeom; a.nsite = M.nsite; a.ncam = M.ncam; a.nsensordata = M.nsensordata;
  a.nsens = sns ? x->nsens : 0;
  a.pyramidal = M.cone != CONE_ELLIPTIC;
  a.flags = (forces ? (f & (MJH_CONSENS_FORCES | MJH_CONSENS_WORLD)) : 0) | (sns ? MJH_CONSENS_SENSORS : 0);
  a.contacts = ncon > 0;
  const int widest = std::max(ncon, a.nsens);
  a.lanes = widest <= 16 ? 16 : (widest <= 32 ? 32 : 64);
  a.lds_env = m->cs_lds_env;
  const int64_t env_bytes = (int64_t)a.lds_env * (int64_t)sizeof(REAL);
  a.envs = (int)std::max<int64_t>(1, std::min<int64_t>(MJH_CONSENS_WG / a.lanes, kLdsWg / env_bytes));
  return launch_envs(mjh_consens_kernel<REAL>, a, x->B, (hipStream_t)stream, MJH_KERNEL_CONSENS);
}

// the energies and the joint / tendon limit and energy sensors of a finished forward pass (mjh_energy.h), one launch
template <typename REAL>
int run_energy(const mjhModel* m, const DevModel<REAL>& M, const mjhEnergyArgs* x, void* stream) {
  const int f = x->flags;
  if (f <= 0 || f > (MJH_ENERGY_POS | MJH_ENERGY_VEL | MJH_ENERGY_SENSORS)) return fail(-22, "energy: unknown flags");
  if (x->B < 0 || x->nsens < 0) return fail(-22, "energy: B and nsens must be >= 0");
  if (x->B == 0) return 0;
  const bool pos = f & MJH_ENERGY_POS, vel = f & MJH_ENERGY_VEL, sns = (f & MJH_ENERGY_SENSORS) && x->nsens > 0 && M.nsensordata > 0;
  if (!(f & MJH_ENERGY_SENSORS) && !x->energy) return fail(-22, "energy: null pointer (energy)");
  if (!x->energy && !sns) return 0;
  const bool springs = !(M.disableflags & (DSBL_SPRING | DSBL_DAMPER));
  if (pos && (!x->gravity || !x->body_mass || !x->xipos || (springs && M.njnt > 0 && (!x->qpos || !x->jnt_stiffness || !x->qpos_spring)) ||
              (springs && M.ntendon > 0 && (!x->ten_length || !x->tendon_stiffness || !x->tendon_lengthspring))))
    return fail(-22, "energy: null pointer (potential leaves)");
  if (vel && M.nv > 0 && (!x->qvel || !x->qM)) return fail(-22, "energy: null pointer (kinetic leaves)");
  if (sns && (!x->sns || !x->sns_cutoff || !x->sensordata || (M.nq > 0 && !x->qpos) || (M.nv > 0 && !x->qvel) || (M.njnt > 0 && (!x->jnt_range || !x->jnt_margin)) ||
              (M.ntendon > 0 && (!x->ten_length || !x->tendon_range || !x->tendon_margin)) || (M.nefc > 0 && M.nv > 0 && (!x->efc_J || !x->efc_force))))
    return fail(-22, "energy: null pointer (sensor leaves)");
  EnergyArgs<REAL> a;
  memset(&a, 0, sizeof(a));
  P_(qpos) P_(qvel) P_(xipos) P_(ten_length) P_(qM) P_(efc_J) P_(efc_force) P_(gravity) P_(body_mass) P_(jnt_stiffness) P_(qpos_spring) P_(jnt_range) P_(jnt_margin)
  P_(tendon_stiffness) P_(tendon_lengthspring) P_(tendon_range) P_(tendon_margin) P_(sns_cutoff)
  a.jnt_type = M.jnt_type; a.jnt_qposadr = M.jnt_qposadr; a.sns = x->sns;
  a.energy = reinterpret_cast<REAL*>(x->energy); a.sensordata = reinterpret_cast<REAL*>(x->sensordata);
  a.nq = M.nq; a.nv = M.nv; a.nbody = M.nbody; a.njnt = M.njnt; a.ntendon = M.ntendon; a.nefc = M.nefc; a.nsensordata = M.nsensordata;
  a.nsens = sns ? x->nsens : 0;
  a.flags = (pos ? MJH_ENERGY_POS : 0) | (vel ? MJH_ENERGY_VEL : 0) | (sns ? MJH_ENERGY_SENSORS : 0);
  a.gravity_on = !(M.disableflags & DSBL_GRAVITY);
  a.spring_on = springs;
  // lanes, environments per workgroup and the chunk of qM rows follow from the model and the size of its sensor table alone (nsens is that size in EVERY call, with
  // or without MJH_ENERGY_SENSORS, so the energies of the two kinds of call are the same bits): LDS_BUDGET bytes per workgroup shared by its environments, an
  // environment's share holding qvel, the lanes' partial sums, the two results and the chunk
  constexpr int LDS_BUDGET = 52 * 1024;  // three workgroups per CU (160 KB)
  const int nv = M.nv, widest = std::max(std::max(M.nbody, nv), x->nsens);
  a.lanes = widest <= 16 ? 16 : (widest <= 32 ? 32 : 64);
  a.envs = MJH_ENERGY_WG / a.lanes;
  const int reals = LDS_BUDGET / a.envs / (int)sizeof(REAL), fixed = ((nv + 3) & ~3) + 2 * a.lanes + 4;
  int chunk = (reals - fixed) / std::max(nv, 1);
  if (chunk > nv) chunk = std::max(nv, 1);
  if (chunk < 1) return fail(-12, "energy: nv too large for the LDS chunk of one environment");
  a.chunk = chunk;
  a.lds_env = (fixed + chunk * nv + 3) & ~3;
  return launch_envs(mjh_energy_kernel<REAL>, a, x->B, (hipStream_t)stream, MJH_KERNEL_ENERGY);
}

// the Jacobian block on a finished forward pass (mjh_jacobian.h): matrices by one lane per element, products (vec given) by 16 lanes per environment
template <typename REAL>
int run_jacobian(const mjhModel* m, const DevModel<REAL>& M, const mjhJacobianArgs* x, void* stream) {
  (void)m;
  const int op = x->op, nv = M.nv;
  if (op < MJH_JACOBIAN_POINT || op > MJH_JACOBIAN_ANGMOM) return fail(-22, "jacobian: unknown op");
  if (x->B < 0) return fail(-22, "jacobian: B must be >= 0");
  if (x->P < 1 || (int64_t)x->P * nv * 3 >= (1 << 30)) return fail(-22, "jacobian: bad query count P");
  if (x->body_stride != 0 && x->body_stride != 1) return fail(-22, "jacobian: body_stride must be 0 or 1");
  if (x->B == 0 || nv == 0) return 0;
  const bool pt = op == MJH_JACOBIAN_POINT || op == MJH_JACOBIAN_DOT, product = x->vec != nullptr;
  if (!x->out0 || (pt && !x->out1) || !x->cdof || !x->subtree_com || !x->body_id || (pt && !x->point) || (op == MJH_JACOBIAN_DOT && (!x->cdof_dot || !x->cvel)) ||
      (!pt && (!x->xipos || !x->body_mass || !x->body_subtreemass)) || (op == MJH_JACOBIAN_ANGMOM && (!x->ximat || !x->body_inertia)))
    return fail(-22, "jacobian: null pointer");
  JacArgs<REAL> a;
  memset(&a, 0, sizeof(a));
  P_(cdof) P_(cdof_dot) P_(cvel) P_(subtree_com) P_(xipos) P_(ximat) P_(body_mass) P_(body_subtreemass) P_(body_inertia) P_(point) P_(vec)
  a.body = x->body_id; a.body_stride = (int)x->body_stride;
  a.body_dofmask = M.body_dofmask; a.body_rootid = M.body_rootid; a.body_subtree_end = M.body_subtree_end;
  a.dof_bodyid = M.dof_bodyid; a.dof_jntid = M.dof_jntid; a.jnt_type = M.jnt_type; a.jnt_dofadr = M.jnt_dofadr;
  a.out0 = reinterpret_cast<REAL*>(x->out0); a.out1 = reinterpret_cast<REAL*>(x->out1);
  a.point_env = x->point_env; a.point_q = x->point_q;
  a.op = op; a.nv = nv; a.nbody = M.nbody; a.mask_words = M.mask_words; a.P = x->P;
  hipStream_t s = (hipStream_t)stream;
  if (!product) {  // one lane per output element; a launch starts at (env_base, r_base) so that the lanes index in 32 bits
    timing_begin(s);
    const int64_t per_env = (int64_t)x->P * nv * 3;
    if (const int rc = launch_cut(x->B * per_env, MJH_JAC_WG, [&](int64_t first, int64_t n, unsigned grid) {
          a.env_base = first / per_env; a.r_base = (int)(first % per_env); a.count = (int)n;
          hipLaunchKernelGGL((mjh_jac_matrix_kernel<REAL>), dim3(grid), dim3(MJH_JAC_WG), 0, s, a);
        }))
      return rc;
    timing_mark(s, MJH_KERNEL_JACOBIAN_POINT + op);
    return 0;
  }
  // the product form: an environment's LDS holds cdof, vec, the terms of one query and (DOT) cdof_dot; LDS_BUDGET bytes per workgroup are shared by at most 256 / 16 environments, halved
  // until they fit; a single environment may take up to 64 KB (the limit a kernel has without a grant)
  constexpr int LDS_BUDGET = 48 * 1024, LDS_MAX = 64 * 1024;
  a.lds_env = 2 * ((6 * nv + 3) & ~3) + ((nv + 3) & ~3) + (op == MJH_JACOBIAN_DOT ? ((6 * nv + 3) & ~3) : 0);
  a.envs = MJH_JAC_WG / MJH_JAC_LANES;
  while (a.envs > 1 && (int64_t)a.envs * a.lds_env * (int64_t)sizeof(REAL) > LDS_BUDGET) a.envs >>= 1;
  const size_t lds = (size_t)a.envs * a.lds_env * sizeof(REAL);
  if (lds > (size_t)LDS_MAX) return fail(-12, "jacobian: nv too large for the LDS rows of one environment");
  timing_begin(s);  // (behind the last refusal)
  if (const int rc = launch_cut(x->B, a.envs, [&](int64_t first, int64_t n, unsigned grid) {
        a.env_base = first; a.env_count = n;
        hipLaunchKernelGGL((mjh_jac_product_kernel<REAL>), dim3(grid), dim3(a.envs * MJH_JAC_LANES), lds, s, a);
      }))
    return rc;
  timing_mark(s, MJH_KERNEL_JACOBIAN_POINT_VEC + op);
  return 0;
}

// mjh_integrate's launch plan, from the model alone: lanes per environment, environments per workgroup, rows of nv reals per LDS chunk, reals of LDS per
// environment.  An environment's LDS: the packed triangle, the right-hand side, the new qvel, vel_i (`fixed`) and chunk rows.  LDS_BUDGET bytes per workgroup are
// shared by 256 / lanes environments, halved until one environment's share holds the fixed part, one row and the rounding of lds_env to a multiple of 4; a single
// environment may take all of kLdsWg.  Returns 0, or -12 when one environment does not fit kLdsWg.
static int integrate_plan(int nv, int nu, int nt, int real_bytes, int* out) {
  constexpr int LDS_BUDGET = 52 * 1024;  // three workgroups per CU (160 KB)
  const int lanes = nv <= 16 ? 16 : (nv <= 32 ? 32 : 64);
  const int fixed = (((nv * (nv + 1)) / 2 + 3) & ~3) + 2 * ((nv + 3) & ~3) + ((nu + 3) & ~3), row = std::max(nv, 1);
  const int most = std::max(std::max(nv, nu), std::max(nt, 1));  // rows worth holding at once
  int envs = MJH_INTEGRATE_WG / lanes;
  while (envs > 1 && LDS_BUDGET / envs / real_bytes - 4 < fixed + row) envs >>= 1;
  const int reals = (envs > 1 ? LDS_BUDGET / envs : kLdsWg) / real_bytes - 4;
  int chunk = (reals - fixed) / row;
  if (chunk > most) chunk = most;
  if (chunk < 1) return -12;
  const int lds_env = (fixed + chunk * row + 3) & ~3;
  if ((int64_t)envs * lds_env * real_bytes > (int64_t)kLdsWg) return -12;
  out[0] = lanes; out[1] = envs; out[2] = chunk; out[3] = lds_env;
  return 0;
}

// deriv_smooth_vel and the implicit / Euler integrators on a finished forward pass (mjh_integrate.h), one launch
template <typename REAL>
int run_integrate(const mjhModel* m, const DevModel<REAL>& M, const mjhIntegrateArgs* x, void* stream) {
  const int f = x->flags;
  constexpr int ALL = MJH_INTEGRATE_QDERIV | MJH_INTEGRATE_IMPLICIT | MJH_INTEGRATE_EULER | MJH_INTEGRATE_STATE | MJH_INTEGRATE_WRITE_QDERIV | MJH_INTEGRATE_WRITE_QACC;
  if (f <= 0 || f > ALL) return fail(-22, "integrate: unknown flags");
  const bool build = f & MJH_INTEGRATE_QDERIV, implicit = f & MJH_INTEGRATE_IMPLICIT, euler = f & MJH_INTEGRATE_EULER, state = f & MJH_INTEGRATE_STATE;
  const bool wqd = f & MJH_INTEGRATE_WRITE_QDERIV, wqa = f & MJH_INTEGRATE_WRITE_QACC;
  if ((implicit && !build) || (implicit && euler) || (wqd && !build)) return fail(-22, "integrate: IMPLICIT and WRITE_QDERIV need QDERIV, IMPLICIT excludes EULER");
  if (!state && !wqd && !wqa) return fail(-22, "integrate: the flags ask for no output");
  if (x->B < 0) return fail(-22, "integrate: B must be >= 0");
  if (x->B == 0) return 0;
  if (!(x->h == x->h)) return fail(-22, "integrate: h is not a number");
  const int nv = M.nv, nu = M.nu, na = M.na, nt = M.ntendon;
  const bool actuation = !(x->disableflags & DSBL_ACTUATION) && nu > 0, damper = !(x->disableflags & DSBL_DAMPER);
  const bool solve = (implicit || euler) && nv > 0;
  if (build && nv > 0) {
    if (actuation && (!x->actuator_moment || !x->ctrl || !x->gainprm || !x->biasprm || (na > 0 && !x->act))) return fail(-22, "integrate: null pointer (actuator leaves)");
    if (actuation && (x->gain_stride < 3 || x->bias_stride < 3)) return fail(-22, "integrate: gainprm / biasprm rows need at least 3 entries");
    if (damper && !x->dof_damping) return fail(-22, "integrate: null pointer (dof_damping)");
    if (nt > 0 && (!x->ten_J || !x->tendon_damping)) return fail(-22, "integrate: null pointer (tendon leaves)");
    if (wqd && !x->qderiv_out) return fail(-22, "integrate: null pointer (qderiv_out)");
  }
  if (solve && (!x->qM || !x->qfrc_smooth || !x->qfrc_constraint || (euler && !implicit && !x->dof_damping))) return fail(-22, "integrate: null pointer (qM, qfrc_smooth, qfrc_constraint, dof_damping)");
  if (!solve && (state || wqa) && nv > 0 && !x->qacc) return fail(-22, "integrate: null pointer (qacc)");
  if (wqa && nv > 0 && !x->qacc_out) return fail(-22, "integrate: null pointer (qacc_out)");
  if (state) {
    if ((M.nq > 0 && (!x->qpos || !x->qpos_out)) || (nv > 0 && (!x->qvel || !x->qvel_out)) || !x->time || !x->time_out) return fail(-22, "integrate: null pointer (state leaves)");
    if (na > 0 && (!x->act || !x->act_dot || !x->act_out || !x->dynprm || !x->actrange || x->dyn_stride < 1)) return fail(-22, "integrate: null pointer (activation leaves)");
  }
  IntegrateArgs<REAL> a;
  memset(&a, 0, sizeof(a));
  P_(qpos) P_(qvel) P_(act) P_(act_dot) P_(time) P_(ctrl) P_(qacc) P_(qM) P_(qfrc_smooth) P_(qfrc_constraint) P_(actuator_moment) P_(ten_J)
  P_(dof_damping) P_(tendon_damping) P_(gainprm) P_(biasprm) P_(dynprm) P_(actrange)
  O_(qpos_out) O_(qvel_out) O_(act_out) O_(time_out) O_(qderiv_out) O_(qacc_out)
  a.act_gaintype = M.act_gaintype; a.act_biastype = M.act_biastype; a.act_dyntype = M.act_dyntype; a.act_actadr = M.act_actadr; a.act_actlimited = M.act_actlimited;
  a.jnt_type = M.jnt_type; a.jnt_qposadr = M.jnt_qposadr; a.jnt_dofadr = M.jnt_dofadr;
  a.h = (REAL)x->h;
  a.nq = M.nq; a.nv = nv; a.nu = nu; a.na = na; a.njnt = M.njnt; a.ntendon = nt;
  a.gain_stride = x->gain_stride; a.bias_stride = x->bias_stride; a.dyn_stride = x->dyn_stride;
  a.flags = f;
  a.actuation_on = actuation; a.damper_on = damper;
  int plan[4];
  if (integrate_plan(nv, nu, nt, (int)sizeof(REAL), plan)) return fail(-12, "integrate: nv too large for the LDS of one workgroup");
  a.lanes = plan[0]; a.envs = plan[1]; a.chunk = plan[2]; a.lds_env = plan[3];
  return launch_envs(mjh_integrate_kernel<REAL>, a, x->B, (hipStream_t)stream, MJH_KERNEL_INTEGRATE);
}

// mjh_smooth's launch plan, from the model alone: lanes per environment (from nbody; FACTOR_M: from nv), environments per workgroup, reals of LDS per environment
// (mjh_smooth.h names the arrays).  A workgroup is planned for kLdsWg bytes; an environment that needs more runs alone.  Returns 0, or -12 when one environment does
// not fit kLdsCu (out is filled all the same).
static int smooth_plan(int op, int nb, int nv, int nt, int real_bytes, int* out) {
  const int n = op == MJH_SMOOTH_FACTOR_M ? nv : nb;
  const int lanes = n <= 16 ? 16 : (n <= 32 ? 32 : 64);
  const int64_t reals[6] = {10 * (int64_t)nb, 20 * (int64_t)nb + 12 * (int64_t)nv, (int64_t)nt * nv, ((((int64_t)nv * (nv + 1)) / 2 + 3) & ~(int64_t)3) + nv,
                            13 * (int64_t)nv, 24 * (int64_t)nb + 6 * (int64_t)nv};
  const int64_t lds_env = std::max<int64_t>(4, (reals[op] + 3) & ~(int64_t)3), env_bytes = lds_env * real_bytes;
  out[0] = lanes;
  out[1] = (int)std::max<int64_t>(1, std::min<int64_t>(MJH_SMOOTH_WG / lanes, kLdsWg / env_bytes));
  out[2] = (int)std::min<int64_t>(lds_env, INT32_MAX);
  return env_bytes > kLdsCu ? -12 : 0;
}

template <typename REAL, int OP>
int launch_smooth(SmoothArgs<REAL>& a, int64_t B, hipStream_t s) {
  const size_t lds = (size_t)a.envs * a.lds_env * sizeof(REAL);
  if (lds > (size_t)kLdsWg) HIP_TRY(allow_lds(&mjh_smooth_kernel<REAL, OP>, (int)lds));
  return launch_envs(mjh_smooth_kernel<REAL, OP>, a, B, s, MJH_KERNEL_SMOOTH_COM_POS + OP);
}

// the smooth-dynamics stages on a caller's Data (mjh_smooth.h), one launch
template <typename REAL>
int run_smooth(const mjhModel* m, const DevModel<REAL>& M, const mjhSmoothArgs* x, void* stream) {
  const int op = x->op;
  if (op < MJH_SMOOTH_COM_POS || op > MJH_SMOOTH_RNE) return fail(-22, "smooth: unknown op");
  if (x->B < 0) return fail(-22, "smooth: B must be >= 0");
  const int nb = M.nbody, nv = M.nv, nj = M.njnt, nt = M.ntendon;
  if (x->B == 0 || (op != MJH_SMOOTH_COM_POS && op != MJH_SMOOTH_CRB && nv == 0) || (op == MJH_SMOOTH_TENDON_ARMATURE && nt == 0)) return 0;  // (crb is per body)
  switch (op) {
    case MJH_SMOOTH_COM_POS:
      if (!x->xipos || !x->ximat || !x->xmat || !x->body_mass || !x->body_inertia || !x->subtree_com_out || !x->cinert_out || (nj > 0 && (!x->xanchor || !x->xaxis)) ||
          (nv > 0 && !x->cdof_out))
        return fail(-22, "smooth: null pointer (com_pos)");
      break;
    case MJH_SMOOTH_CRB:
      if (!x->cinert || !x->crb_out || (nv > 0 && (!x->cdof || !x->dof_armature || !x->qM_out))) return fail(-22, "smooth: null pointer (crb)");
      break;
    case MJH_SMOOTH_TENDON_ARMATURE:
      if (!x->qM || !x->ten_J || !x->tendon_armature || !x->qM_out) return fail(-22, "smooth: null pointer (tendon_armature)");
      break;
    case MJH_SMOOTH_FACTOR_M:
      if (!x->qM || !x->qLD_out) return fail(-22, "smooth: null pointer (factor_m)");
      break;
    case MJH_SMOOTH_COM_VEL:
      if (!x->cdof || !x->qvel || !x->cvel_out || !x->cdof_dot_out) return fail(-22, "smooth: null pointer (com_vel)");
      break;
    default:
      if (!x->cdof || !x->cdof_dot || !x->cvel || !x->cinert || !x->qvel || (x->flg_acc && !x->qacc) || !x->qfrc_bias_out) return fail(-22, "smooth: null pointer (rne)");
  }
  int plan[3];
  if (smooth_plan(op, nb, nv, nt, (int)sizeof(REAL), plan)) {
    char msg[200];
    snprintf(msg, sizeof(msg), "smooth: op %d with nbody = %d, nv = %d, ntendon = %d needs %lld bytes of LDS per environment; a CU has %d", op, nb, nv, nt,
             (long long)plan[2] * (long long)sizeof(REAL), (int)kLdsCu);
    return fail(-12, msg);
  }
  SmoothArgs<REAL> a;
  memset(&a, 0, sizeof(a));
  P_(xipos) P_(ximat) P_(xmat) P_(xanchor) P_(xaxis) P_(cinert) P_(cdof) P_(cdof_dot) P_(cvel) P_(qvel) P_(qacc) P_(qM) P_(ten_J)
  P_(body_mass) P_(body_inertia) P_(dof_armature) P_(tendon_armature)
  a.subtree_com = reinterpret_cast<REAL*>(x->subtree_com_out); a.cinert_out = reinterpret_cast<REAL*>(x->cinert_out); a.cdof_out = reinterpret_cast<REAL*>(x->cdof_out);
  a.crb = reinterpret_cast<REAL*>(x->crb_out); a.qM_out = reinterpret_cast<REAL*>(x->qM_out); a.qLD = reinterpret_cast<REAL*>(x->qLD_out);
  a.cvel_out = reinterpret_cast<REAL*>(x->cvel_out); a.cdof_dot_out = reinterpret_cast<REAL*>(x->cdof_dot_out); a.qfrc_bias = reinterpret_cast<REAL*>(x->qfrc_bias_out);
  a.body_rootid = M.body_rootid; a.body_jntadr = M.body_jntadr; a.body_jntnum = M.body_jntnum; a.body_dofadr = M.body_dofadr; a.body_dofnum = M.body_dofnum;
  a.body_depth = M.body_depth; a.body_chain = M.body_chain; a.body_subtree_end = M.body_subtree_end; a.jnt_type = M.jnt_type; a.jnt_dofadr = M.jnt_dofadr;
  a.jnt_bodyid = M.jnt_bodyid; a.dof_bodyid = M.dof_bodyid; a.body_dofmask = M.body_dofmask;
  const bool nograv = x->disableflags & DSBL_GRAVITY;
  a.cacc0[0] = nograv ? (REAL)0 : -(REAL)x->gravity_x; a.cacc0[1] = nograv ? (REAL)0 : -(REAL)x->gravity_y; a.cacc0[2] = nograv ? (REAL)0 : -(REAL)x->gravity_z;
  a.nbody = nb; a.njnt = nj; a.nv = nv; a.ntendon = nt; a.max_depth = M.max_depth; a.mask_words = M.mask_words; a.flg_acc = x->flg_acc != 0;
  a.lanes = plan[0]; a.envs = plan[1]; a.lds_env = plan[2];
  hipStream_t s = (hipStream_t)stream;
  switch (op) {
    case MJH_SMOOTH_COM_POS: return launch_smooth<REAL, MJH_SMOOTH_COM_POS>(a, x->B, s);
    case MJH_SMOOTH_CRB: return launch_smooth<REAL, MJH_SMOOTH_CRB>(a, x->B, s);
    case MJH_SMOOTH_TENDON_ARMATURE: return launch_smooth<REAL, MJH_SMOOTH_TENDON_ARMATURE>(a, x->B, s);
    case MJH_SMOOTH_FACTOR_M: return launch_smooth<REAL, MJH_SMOOTH_FACTOR_M>(a, x->B, s);
    case MJH_SMOOTH_COM_VEL: return launch_smooth<REAL, MJH_SMOOTH_COM_VEL>(a, x->B, s);
    default: return launch_smooth<REAL, MJH_SMOOTH_RNE>(a, x->B, s);
  }
}

// mjh_dynamics's launch plan, from the model alone: lanes per environment (from nv: TENDON, PASSIVE, ACCELERATION; from nu: TRANSMISSION, VELOCITY, ACTUATION),
// environments per workgroup, reals of LDS per environment (mjh_dynamics.h names the arrays).  A workgroup is planned for kLdsWg bytes; an environment that needs more
// runs alone.  Returns 0, or -12 when one environment does not fit kLdsCu (out is filled all the same).
static int dynamics_plan(int op, int nq, int nv, int nu, int nb, int nt, int real_bytes, int* out) {
  const int n = (op == MJH_DYNAMICS_TENDON || op == MJH_DYNAMICS_PASSIVE || op == MJH_DYNAMICS_ACCELERATION) ? nv : nu;
  const int lanes = n <= 16 ? 16 : (n <= 32 ? 32 : 64);
  const int64_t reals[6] = {(int64_t)nq, (int64_t)nq + nt + 3 * (int64_t)nu, (int64_t)nv + ((int64_t)nu + nt) * (nv | 1), (int64_t)nv + nt + 12 * (int64_t)nb, (int64_t)nu,
                            ((((int64_t)nv * (nv + 1)) / 2 + 3) & ~(int64_t)3) + nv + 6 * (int64_t)nb};
  const int64_t lds_env = std::max<int64_t>(4, (reals[op] + 3) & ~(int64_t)3), env_bytes = lds_env * real_bytes;
  out[0] = lanes;
  out[1] = (int)std::max<int64_t>(1, std::min<int64_t>(MJH_DYNAMICS_WG / lanes, kLdsWg / env_bytes));
  out[2] = (int)std::min<int64_t>(lds_env, INT32_MAX);
  return env_bytes > kLdsCu ? -12 : 0;
}

template <typename REAL, int OP>
int launch_dynamics(DynArgs<REAL>& a, int64_t B, hipStream_t s) {
  const size_t lds = (size_t)a.envs * a.lds_env * sizeof(REAL);
  if (lds > (size_t)kLdsWg) HIP_TRY(allow_lds(&mjh_dynamics_kernel<REAL, OP>, (int)lds));
  return launch_envs(mjh_dynamics_kernel<REAL, OP>, a, B, s, MJH_KERNEL_DYNAMICS_TENDON + OP);
}

// tendon, transmission, passive and the forward stages on a caller's Data (mjh_dynamics.h), one launch
template <typename REAL>
int run_dynamics(const mjhModel* m, const DevModel<REAL>& M, const mjhDynamicsArgs* x, void* stream) {
  const int op = x->op;
  if (op < MJH_DYNAMICS_TENDON || op > MJH_DYNAMICS_ACCELERATION) return fail(-22, "dynamics: unknown op");
  if (x->B < 0) return fail(-22, "dynamics: B must be >= 0");
  const int nq = M.nq, nv = M.nv, nu = M.nu, na = M.na, nb = M.nbody, nj = M.njnt, nt = M.ntendon;
  const int flags = x->disableflags;
  if (x->B == 0) return 0;
  switch (op) {
    case MJH_DYNAMICS_TENDON:
      if (nt == 0) return 0;
      if (!x->qpos || !x->ten_length_out || (nv > 0 && !x->ten_J_out)) return fail(-22, "dynamics: null pointer (tendon)");
      break;
    case MJH_DYNAMICS_TRANSMISSION:
      if (nu == 0) return 0;
      if (!x->qpos || !x->gear || !x->actuator_length_out || (nv > 0 && !x->actuator_moment_out) || (nt > 0 && (!x->ten_length || (nv > 0 && !x->ten_J))))
        return fail(-22, "dynamics: null pointer (transmission)");
      break;
    case MJH_DYNAMICS_VELOCITY:
      if (nu + nt == 0 || nv == 0) return 0;
      if (!x->qvel || (nu > 0 && (!x->actuator_moment || !x->actuator_velocity_out)) || (nt > 0 && (!x->ten_J || !x->ten_velocity_out)))
        return fail(-22, "dynamics: null pointer (velocity)");
      break;
    case MJH_DYNAMICS_PASSIVE:
      if (flags & (DSBL_SPRING | DSBL_DAMPER)) return fail(-22, "dynamics: passive with SPRING or DAMPER disabled is all zeros: nothing to launch");
      if (nv == 0) return 0;
      if (!x->qpos || !x->qvel || !x->jnt_stiffness || !x->qpos_spring || !x->dof_damping || !x->qfrc_passive_out ||
          (nt > 0 && (!x->ten_length || !x->ten_velocity || !x->ten_J || !x->tendon_stiffness || !x->tendon_damping || !x->tendon_lengthspring)) ||
          ((x->has_gravcomp || x->has_fluid) && (!x->xipos || !x->subtree_com || !x->cdof || !x->body_mass)) ||
          (x->has_gravcomp && (!x->body_gravcomp || !x->jnt_actgravcomp || !x->qfrc_gravcomp_out)) || (x->has_fluid && (!x->ximat || !x->cvel || !x->body_inertia)))
        return fail(-22, "dynamics: null pointer (passive)");
      break;
    case MJH_DYNAMICS_ACTUATION:
      if (nu == 0 || (flags & DSBL_ACTUATION)) return fail(-22, "dynamics: actuation without actuators or with ACTUATION disabled is all zeros: nothing to launch");
      if (!x->ctrl || (na > 0 && (!x->act || !x->act_dot_out || !x->dynprm)) || !x->actuator_length || !x->actuator_velocity || !x->gainprm || !x->biasprm ||
          !x->ctrlrange || !x->forcerange || !x->lengthrange || !x->acc0 || !x->actuator_force_out ||
          (nv > 0 && (!x->actuator_moment || !x->qfrc_actuator_out || !x->jnt_actfrcrange || (x->has_gravcomp && (!x->qfrc_gravcomp || !x->jnt_actgravcomp)))))
        return fail(-22, "dynamics: null pointer (actuation)");
      if (x->gain_stride < 3 || x->bias_stride < 3 || (na > 0 && x->dyn_stride < 1))  // (9 / 9 / 3 for muscle gains, biases and dynamics: the Python layer's check)
        return fail(-22, "dynamics: gainprm / biasprm rows need 3 entries, dynprm rows 1");
      break;
    default:
      if (nv == 0) return 0;
      if (!x->qfrc_applied || !x->xfrc_applied || !x->xipos || !x->subtree_com || !x->cdof || !x->qfrc_passive || !x->qfrc_bias || !x->qfrc_actuator || !x->qLD ||
          !x->qfrc_smooth_out || !x->qacc_smooth_out)
        return fail(-22, "dynamics: null pointer (acceleration)");
  }
  int plan[3];
  if (dynamics_plan(op, nq, nv, nu, nb, nt, (int)sizeof(REAL), plan)) {
    char msg[240];
    snprintf(msg, sizeof(msg), "dynamics: op %d with nq = %d, nv = %d, nu = %d, nbody = %d, ntendon = %d needs %lld bytes of LDS per environment; a CU has %d", op, nq, nv,
             nu, nb, nt, (long long)plan[2] * (long long)sizeof(REAL), (int)kLdsCu);
    return fail(-12, msg);
  }
  DynArgs<REAL> a;
  memset(&a, 0, sizeof(a));
  P_(qpos) P_(qvel) P_(ctrl) P_(act) P_(ten_length) P_(ten_velocity) P_(ten_J) P_(actuator_length) P_(actuator_velocity) P_(actuator_moment) P_(xipos) P_(ximat)
  P_(subtree_com) P_(cdof) P_(cvel) P_(qfrc_gravcomp) P_(qfrc_applied) P_(xfrc_applied) P_(qfrc_passive) P_(qfrc_bias) P_(qfrc_actuator) P_(qLD)
  P_(jnt_stiffness) P_(qpos_spring) P_(dof_damping) P_(tendon_stiffness) P_(tendon_damping) P_(tendon_lengthspring) P_(body_mass) P_(body_inertia) P_(body_gravcomp)
  P_(jnt_actgravcomp) P_(jnt_actfrcrange) P_(gainprm) P_(biasprm) P_(dynprm) P_(ctrlrange) P_(forcerange) P_(gear) P_(lengthrange) P_(acc0)
  O_(ten_length_out) O_(ten_J_out) O_(actuator_length_out) O_(actuator_moment_out) O_(actuator_velocity_out) O_(ten_velocity_out) O_(qfrc_passive_out)
  O_(qfrc_gravcomp_out) O_(act_dot_out) O_(qfrc_actuator_out) O_(actuator_force_out) O_(qfrc_smooth_out) O_(qacc_smooth_out)
  a.body_rootid = M.body_rootid; a.body_subtree_end = M.body_subtree_end; a.jnt_type = M.jnt_type; a.jnt_qposadr = M.jnt_qposadr; a.jnt_dofadr = M.jnt_dofadr;
  a.jnt_actfrclimited = M.jnt_actfrclimited; a.dof_bodyid = M.dof_bodyid; a.dof_jntid = M.dof_jntid; a.ten_adr = M.ten_adr; a.ten_qposadr = M.ten_qposadr;
  a.act_trntype = M.act_trntype; a.act_trnid = M.act_trnid; a.act_jnttype = M.act_jnttype; a.act_dofadr = M.act_dofadr; a.act_qposadr = M.act_qposadr;
  a.act_gaintype = M.act_gaintype; a.act_biastype = M.act_biastype; a.act_dyntype = M.act_dyntype; a.act_ctrllimited = M.act_ctrllimited;
  a.act_forcelimited = M.act_forcelimited; a.act_actadr = M.act_actadr; a.act_actnum = M.act_actnum; a.ten_coef = M.ten_coef; a.ten_J0 = M.ten_J0;
  a.gravity[0] = (REAL)x->gravity_x; a.gravity[1] = (REAL)x->gravity_y; a.gravity[2] = (REAL)x->gravity_z;
  a.wind[0] = (REAL)x->wind_x; a.wind[1] = (REAL)x->wind_y; a.wind[2] = (REAL)x->wind_z; a.density = (REAL)x->density; a.viscosity = (REAL)x->viscosity;
  a.nq = nq; a.nv = nv; a.nu = nu; a.na = na; a.nbody = nb; a.njnt = nj; a.ntendon = nt;
  a.gain_stride = x->gain_stride; a.bias_stride = x->bias_stride; a.dyn_stride = x->dyn_stride;
  a.gravcomp = x->has_gravcomp != 0; a.fluid = x->has_fluid != 0; a.clampctrl = !(flags & DSBL_CLAMPCTRL);
  a.lanes = plan[0]; a.envs = plan[1]; a.lds_env = plan[2];
  hipStream_t s = (hipStream_t)stream;
  switch (op) {
    case MJH_DYNAMICS_TENDON: return launch_dynamics<REAL, MJH_DYNAMICS_TENDON>(a, x->B, s);
    case MJH_DYNAMICS_TRANSMISSION: return launch_dynamics<REAL, MJH_DYNAMICS_TRANSMISSION>(a, x->B, s);
    case MJH_DYNAMICS_VELOCITY: return launch_dynamics<REAL, MJH_DYNAMICS_VELOCITY>(a, x->B, s);
    case MJH_DYNAMICS_PASSIVE: return launch_dynamics<REAL, MJH_DYNAMICS_PASSIVE>(a, x->B, s);
    case MJH_DYNAMICS_ACTUATION: return launch_dynamics<REAL, MJH_DYNAMICS_ACTUATION>(a, x->B, s);
    default: return launch_dynamics<REAL, MJH_DYNAMICS_ACCELERATION>(a, x->B, s);
  }
}

#undef P_
#undef O_

// ---- finite-difference Jacobians of a step (mjh_fd.h) and of inverse dynamics (mjh_ifd.h): the launches on either side of the caller's mjh_step / mjh_inverse
// over the perturbed environments.  One check (fd_common), one perturb (run_fd_perturb) and one launch tail (launch_fd) serve both. ----

// 4-byte words per environment of every mjhData slot, in struct order: reals, int32, int64, then the trailing input-only leaves
template <typename REAL>
std::vector<int64_t> data_words(const mjhModel* m, const DevModel<REAL>& M) {
  const int64_t rw = sizeof(REAL) / 4, ncon = M.ncon, nb = M.nbody;
  std::vector<int64_t> w;
  for (int64_t c : m->leaf_count) w.push_back(c * rw);
  const int64_t tail[] = {ncon /* contact_dim */, M.neq /* eq_active */, 2 * ncon, 2 * ncon, 4 * ncon, 2 * ncon /* geom1, geom2, geom, efc_address (int64) */,
                          6 * nb * rw, 6 * nb * rw, 3 * nb * rw, 3 * nb * rw /* cacc, cfrc_int, subtree_linvel, subtree_angmom */};
  w.insert(w.end(), tail, tail + 10);
  return w;
}

// The refusals the family's entry points share, then what its kernels read of the model and of the call.  `inverse`: the columns are the 3 nv of
// mjh_ifd.h (no act, no ctrl: na = nu = 0 in `c`), the rows counted against 2^31 its nv, and the messages say "ifd".
template <typename REAL>
int fd_common(const DevModel<REAL>& M, bool inverse, const void* ctrl, int64_t B, int col0, int ncol, double eps, int centered, FdCommon<REAL>& c) {
  const std::string fam = inverse ? "ifd" : "fd";
  const int ns = 2 * M.nv + M.na;
  const int64_t cols = inverse ? 3 * (int64_t)M.nv : (int64_t)ns + M.nu, rows = inverse ? M.nv : ns;
  if (B < 0) return fail(-22, fam + ": B must be >= 0");
  if (!(eps > 0) || !((REAL)eps > 0)) return fail(-22, fam + ": eps must be positive in the model's dtype");
  if (col0 < 0 || ncol < 1 || (int64_t)col0 + ncol > cols) return fail(-22, fam + ": columns outside [0, " + (inverse ? "3 nv)" : "2 nv + na + nu)"));
  if ((int64_t)ncol * 2 * (rows + M.nsensordata + 1) >= ((int64_t)1 << 31)) return fail(-22, fam + ": too many columns in one call");
  if (!inverse && col0 + ncol > ns && !ctrl) return fail(-22, "fd: in.ctrl is required for the ctrl columns");
  c.dof_jntid = M.dof_jntid; c.jnt_type = M.jnt_type; c.jnt_qposadr = M.jnt_qposadr; c.jnt_dofadr = M.jnt_dofadr;
  if (!inverse) { c.act_ctrllimited = M.act_ctrllimited; c.act_ctrlrange = M.act_ctrlrange; c.ctrl = reinterpret_cast<const REAL*>(ctrl); }
  c.eps = (REAL)eps;
  c.nq = M.nq; c.nv = M.nv; c.na = inverse ? 0 : M.na; c.nu = inverse ? 0 : M.nu; c.nsd = M.nsensordata;
  c.centered = centered ? 1 : 0; c.col0 = col0; c.ncol = ncol;
  return 0;
}

// The tail of the family's run_* functions, after launch_envs: `units` units of the call go out `per_wg` to a workgroup of `wg` lanes, in cuts that
// start at span.first (`span` lies inside `a`), timed as kernel `id`.  The caller has made its last refusal.
template <typename Args>
int launch_fd(void (*kernel)(Args), Args& a, FdSpan& span, int64_t units, int per_wg, int wg, void* stream, int id) {
  hipStream_t s = (hipStream_t)stream;
  span.total = units;
  timing_begin(s);
  if (const int rc = launch_cut(units, per_wg, [&](int64_t first, int64_t, unsigned grid) {
        span.first = first;
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(wg), 0, s, a);
      }))
    return rc;
  timing_mark(s, id);
  return 0;
}

// INVERSE: mjh_ifd_perturb, whose columns from 2 nv on are qacc; else mjh_fd_perturb (act, ctrl)
template <typename REAL, bool INVERSE>
int run_fd_perturb(const mjhModel* m, const DevModel<REAL>& M, const mjhData* in, mjhData* scratch, int64_t B, int col0, int ncol, double eps, int centered, void* stream) {
  static_assert(sizeof(FdPerturbArgs<REAL>) <= 4096, "kernel arguments exceed the 4 KiB kernarg segment");
  const std::string fn = INVERSE ? "ifd_perturb" : "fd_perturb";
  if (INVERSE && (B == 0 || M.nv == 0)) return B < 0 ? fail(-22, "ifd: B must be >= 0") : 0;
  FdPerturbArgs<REAL> a;
  memset(&a, 0, sizeof(a));
  if (const int rc = fd_common(M, INVERSE, in->ctrl, B, col0, ncol, eps, centered, a.c)) return rc;
  if (B == 0) return 0;
  if (INVERSE) {
    if (!in->qpos || !in->qvel || !in->qacc || !scratch->qpos || !scratch->qvel || !scratch->qacc)
      return fail(-22, "ifd_perturb: qpos, qvel and qacc are required in both Data");
  } else if (!in->qpos || !in->qvel || !scratch->qpos || !scratch->qvel || (M.na > 0 && !(in->act && scratch->act)) || (M.nu > 0 && !(in->ctrl && scratch->ctrl))) {
    return fail(-22, "fd_perturb: qpos, qvel, act and ctrl are required in both Data");
  }
  const std::vector<int64_t> words = data_words(m, M);
  if (words.size() * sizeof(void*) != sizeof(mjhData)) return fail(-22, fn + ": leaf table out of sync with mjhData");
  void* const* dp = reinterpret_cast<void* const*>(scratch);
  void* const* sp = reinterpret_cast<void* const*>(in);
  for (size_t i = 0; i < words.size(); i++) {
    if (!dp[i] || words[i] == 0) continue;
    if (!sp[i]) return fail(-22, fn + ": a leaf of the scratch Data is missing from the input Data");
    if (a.nleaf == MJH_FD_MAX_LEAVES) return fail(-22, fn + ": too many leaves in the scratch Data (input leaves only)");
    FdLeaf& L = a.leaf[a.nleaf++];
    L.dst = (unsigned*)dp[i]; L.src = (const unsigned*)sp[i]; L.words = (int)words[i];
  }
  a.qpos = reinterpret_cast<const REAL*>(in->qpos); a.qvel = reinterpret_cast<const REAL*>(in->qvel);
  a.p_qpos = reinterpret_cast<REAL*>(scratch->qpos); a.p_qvel = reinterpret_cast<REAL*>(scratch->qvel);
  if (INVERSE) {
    a.qacc = reinterpret_cast<const REAL*>(in->qacc); a.p_qacc = reinterpret_cast<REAL*>(scratch->qacc);
  } else {
    a.act = reinterpret_cast<const REAL*>(in->act); a.p_act = reinterpret_cast<REAL*>(scratch->act); a.p_ctrl = reinterpret_cast<REAL*>(scratch->ctrl);
  }
  return launch_fd(INVERSE ? mjh_ifd_perturb_kernel<REAL> : mjh_fd_perturb_kernel<REAL>, a, a.c.span, B * ncol * (centered ? 2 : 1), 1, MJH_FD_PERTURB_WG, stream,
                   INVERSE ? MJH_KERNEL_IFD_PERTURB : MJH_KERNEL_FD_PERTURB);
}

// the state (and, with `sens`, the sensordata) of a stepped Data as the difference and vjp kernels read it; false: a leaf they need is missing
template <typename REAL>
bool fd_state(const DevModel<REAL>& M, const mjhData* d, bool sens, FdState<REAL>& y) {
  y.qpos = reinterpret_cast<const REAL*>(d->qpos); y.qvel = reinterpret_cast<const REAL*>(d->qvel);
  y.act = reinterpret_cast<const REAL*>(d->act); y.sens = reinterpret_cast<const REAL*>(d->sensordata);
  return y.qpos && y.qvel && (M.na == 0 || y.act) && (!sens || y.sens);
}

template <typename REAL>
int run_fd_difference(const DevModel<REAL>& M, const mjhData* in, const mjhData* nominal, const mjhData* stepped, int64_t B, int col0, int ncol, double eps,
                      int centered, void* A, void* Bm, void* C, void* D, void* stream) {
  FdDiffArgs<REAL> a;
  memset(&a, 0, sizeof(a));
  if (const int rc = fd_common(M, false, in->ctrl, B, col0, ncol, eps, centered, a.c)) return rc;
  const int ns = 2 * M.nv + M.na;
  if (B == 0 || ns == 0) return 0;
  const bool sens = C != nullptr && M.nsensordata > 0;
  if ((C && !D && M.nu > 0) || (!C && D)) return fail(-22, "fd_difference: C and D go together");
  if (!A || (M.nu > 0 && !Bm)) return fail(-22, "fd_difference: A and Bm are required");
  if (!fd_state(M, nominal, sens, a.y0) || !fd_state(M, stepped, sens, a.y))
    return fail(-22, "fd_difference: qpos, qvel, act (and sensordata for C, D) are required in both stepped Data");
  a.A = reinterpret_cast<REAL*>(A); a.Bm = reinterpret_cast<REAL*>(Bm);
  a.C = sens ? reinterpret_cast<REAL*>(C) : nullptr; a.D = sens ? reinterpret_cast<REAL*>(D) : nullptr;
  return launch_fd(mjh_fd_difference_kernel<REAL>, a, a.c.span, B * (ns + (sens ? M.nsensordata : 0)) * ncol, MJH_FD_DIFF_WG, MJH_FD_DIFF_WG, stream,
                   MJH_KERNEL_FD_DIFFERENCE);
}

template <typename REAL>
int run_fd_vjp(const DevModel<REAL>& M, const mjhData* in, const mjhData* nominal, const mjhData* stepped, int64_t B, int col0, int ncol, double eps,
               int centered, const void* g_state, const void* g_sens, void* gx, void* gu, void* stream) {
  FdVjpArgs<REAL> a;
  memset(&a, 0, sizeof(a));
  if (const int rc = fd_common(M, false, in->ctrl, B, col0, ncol, eps, centered, a.c)) return rc;
  const int ns = 2 * M.nv + M.na;
  if (B == 0 || ns == 0) return 0;
  const bool sens = g_sens != nullptr && M.nsensordata > 0;
  if (!g_state || !gx || (M.nu > 0 && !gu)) return fail(-22, "fd_vjp: g_state, gx and gu are required");
  if (!fd_state(M, nominal, sens, a.y0) || !fd_state(M, stepped, sens, a.y))
    return fail(-22, "fd_vjp: qpos, qvel, act (and sensordata with g_sens) are required in both stepped Data");
  a.g_state = reinterpret_cast<const REAL*>(g_state); a.g_sens = sens ? reinterpret_cast<const REAL*>(g_sens) : nullptr;
  a.gx = reinterpret_cast<REAL*>(gx); a.gu = reinterpret_cast<REAL*>(gu);
  return launch_fd(mjh_fd_vjp_kernel<REAL>, a, a.c.span, B * ncol, MJH_FD_VJP_WG / MJH_WAVE, MJH_FD_VJP_WG, stream, MJH_KERNEL_FD_VJP);
}

template <typename REAL>
int run_fd_tangent(const DevModel<REAL>& M, const void* qpos, const void* g_in, void* g_out, int64_t B, int mode, void* stream) {
  if (B < 0) return fail(-22, "fd_tangent: B must be >= 0");
  if (mode != MJH_FD_TANGENT_PULL && mode != MJH_FD_TANGENT_PUSH) return fail(-22, "fd_tangent: mode must be MJH_FD_TANGENT_PULL or MJH_FD_TANGENT_PUSH");
  if (B == 0 || M.nv == 0) return 0;
  if (!qpos || !g_in || !g_out) return fail(-22, "fd_tangent: qpos, g_in and g_out are required");
  FdTangentArgs<REAL> a;
  memset(&a, 0, sizeof(a));
  a.dof_jntid = M.dof_jntid; a.jnt_type = M.jnt_type; a.jnt_qposadr = M.jnt_qposadr; a.jnt_dofadr = M.jnt_dofadr;
  a.qpos = reinterpret_cast<const REAL*>(qpos); a.g_in = reinterpret_cast<const REAL*>(g_in); a.g_out = reinterpret_cast<REAL*>(g_out);
  a.nq = M.nq; a.nv = M.nv; a.mode = mode;
  return launch_fd(mjh_fd_tangent_kernel<REAL>, a, a.span, B * M.nv, MJH_FD_TANGENT_WG, MJH_FD_TANGENT_WG, stream, MJH_KERNEL_FD_TANGENT);
}

// the other end of mjh_ifd_perturb (run_fd_perturb<REAL, true>): qfrc_inverse and sensordata of the caller's mjh_inverse over the perturbed environments (mjh_ifd.h)
template <typename REAL>
int run_ifd_difference(const DevModel<REAL>& M, const void* f0, const void* s0, const void* f, const void* sd, int64_t B, int col0, int ncol, double eps,
                       int centered, void* DfDq, void* DfDv, void* DfDa, void* DsDq, void* DsDv, void* DsDa, void* stream) {
  if (B == 0 || M.nv == 0) return B < 0 ? fail(-22, "ifd: B must be >= 0") : 0;
  IfdDiffArgs<REAL> a;
  memset(&a, 0, sizeof(a));
  if (const int rc = fd_common(M, true, nullptr, B, col0, ncol, eps, centered, a.c)) return rc;
  const int given = (DsDq != nullptr) + (DsDv != nullptr) + (DsDa != nullptr);
  if (given != 0 && given != 3) return fail(-22, "ifd_difference: DsDq, DsDv and DsDa go together");
  const bool sens = given == 3 && M.nsensordata > 0;
  if (!DfDq || !DfDv || !DfDa) return fail(-22, "ifd_difference: DfDq, DfDv and DfDa are required");
  if (!f || (!centered && !f0)) return fail(-22, "ifd_difference: qfrc_inverse of the perturbed passes (and, one-sided, of the nominal pass) is required");
  if (sens && (!sd || (!centered && !s0))) return fail(-22, "ifd_difference: sensordata of the perturbed passes (and, one-sided, of the nominal pass) is required for DsD*");
  a.f0 = reinterpret_cast<const REAL*>(f0); a.s0 = reinterpret_cast<const REAL*>(s0);
  a.f = reinterpret_cast<const REAL*>(f); a.s = reinterpret_cast<const REAL*>(sd);
  a.DfDq = reinterpret_cast<REAL*>(DfDq); a.DfDv = reinterpret_cast<REAL*>(DfDv); a.DfDa = reinterpret_cast<REAL*>(DfDa);
  if (sens) { a.DsDq = reinterpret_cast<REAL*>(DsDq); a.DsDv = reinterpret_cast<REAL*>(DsDv); a.DsDa = reinterpret_cast<REAL*>(DsDa); }
  a.c.nsd = sens ? M.nsensordata : 0;
  return launch_fd(mjh_ifd_difference_kernel<REAL>, a, a.c.span, B * (a.c.nv + a.c.nsd) * ncol, MJH_IFD_DIFF_WG, MJH_IFD_DIFF_WG, stream, MJH_KERNEL_IFD_DIFFERENCE);
}

}  // namespace

extern "C" {

int mjh_model_create(const mjhModelDesc* desc, int dtype, mjhModel** out) {
  if (!desc || !out) return fail(-22, "null argument");
  if (desc->abi_version != MJH_ABI_VERSION) return fail(-22, "mjhModelDesc.abi_version mismatch");
  if (dtype != MJH_F64 && dtype != MJH_F32) return fail(-22, "dtype must be MJH_F64 or MJH_F32");
  if (desc->integrator != INT_EULER && desc->integrator != INT_RK4) return fail(-38, "integrator not implemented");
  if (desc->solver != SOL_CG && desc->solver != SOL_NEWTON) return fail(-38, "solver not implemented");
  mjhModel* m = new mjhModel();
  m->dtype = dtype;
  int rc = dtype == MJH_F64 ? build<double>(desc, m, m->m64) : build<float>(desc, m, m->m32);
  if (rc != 0) { mjh_model_destroy(m); return rc; }
  *out = m;
  return 0;
}

void mjh_model_destroy(mjhModel* m) {
  if (!m) return;
  if (m->blob) (void)hipFree(m->blob);
  delete m;
}

int mjh_forward(const mjhModel* m, const mjhData* in, mjhData* out, void* work, int64_t B, int stages, int flags, void* stream) {
  if (!m || !in || !out) return fail(-22, "null argument");
  return m->dtype == MJH_F64 ? run<double>(m, m->m64, in, out, work, B, flags, 0, stages, stream)
                             : run<float>(m, m->m32, in, out, work, B, flags, 0, stages, stream);
}

int mjh_step(const mjhModel* m, const mjhData* in, mjhData* out, void* work, int64_t B, int flags, void* stream) {
  if (!m || !in || !out) return fail(-22, "null argument");
  return m->dtype == MJH_F64 ? run<double>(m, m->m64, in, out, work, B, flags, 1, MJH_STAGE_ALL, stream)
                             : run<float>(m, m->m32, in, out, work, B, flags, 1, MJH_STAGE_ALL, stream);
}

int mjh_inverse(const mjhModel* m, const mjhData* in, mjhData* out, void* qfrc_inverse, void* work, int64_t B, int flags, void* stream) {
  if (!m || !in || !out) return fail(-22, "null argument");
  return m->dtype == MJH_F64 ? run_inverse<double>(m, m->m64, in, out, qfrc_inverse, work, B, flags, stream)
                             : run_inverse<float>(m, m->m32, in, out, qfrc_inverse, work, B, flags, stream);
}

int mjh_ray(const mjhModel* m, const void* geom_xpos, const void* geom_xmat, const void* pnt, int64_t pnt_env, int64_t pnt_ray, const void* vec,
            int64_t vec_env, int64_t vec_ray, int64_t B, int64_t R, const mjhRayCands* cands, void* dist, int64_t* geomid, void* stream) {
  if (!m || !cands) return fail(-22, "null argument");
  return m->dtype == MJH_F64 ? run_ray<double>(m, m->m64, geom_xpos, geom_xmat, pnt, pnt_env, pnt_ray, vec, vec_env, vec_ray, B, R, cands, dist, geomid, stream)
                             : run_ray<float>(m, m->m32, geom_xpos, geom_xmat, pnt, pnt_env, pnt_ray, vec, vec_env, vec_ray, B, R, cands, dist, geomid, stream);
}

int mjh_geom_distance(const mjhModel* m, const void* geom_xpos, const void* geom_xmat, const void* geom_size, const int32_t* pairs, int64_t npair, double distmax,
                      void* dist, void* fromto, int64_t B, void* stream) {
  if (!m) return fail(-22, "null argument");
  return m->dtype == MJH_F64 ? run_geom_distance<double>(m->m64, geom_xpos, geom_xmat, geom_size, pairs, npair, distmax, dist, fromto, B, stream)
                             : run_geom_distance<float>(m->m32, geom_xpos, geom_xmat, geom_size, pairs, npair, distmax, dist, fromto, B, stream);
}

int mjh_qpos_arith(const mjhModel* m, int op, const void* a, const void* b, double dt, void* out, int64_t B, void* stream) {
  if (!m) return fail(-22, "null argument");
  return m->dtype == MJH_F64 ? run_qpos_arith<double>(m->m64, op, a, b, dt, out, B, stream) : run_qpos_arith<float>(m->m32, op, a, b, dt, out, B, stream);
}

int mjh_ik_site_step(const mjhModel* m, const void* cdof, const void* subtree_com, const void* site_xpos, const void* site_xmat, int site, int body,
                     const void* target_pos, int64_t pos_stride, const void* target_quat, int64_t quat_stride, const int32_t* dof_sel, const double* params,
                     int last, void* qpos, void* err_norm, int32_t* steps, unsigned char* done, int64_t B, void* stream) {
  if (!m) return fail(-22, "null argument");
  return m->dtype == MJH_F64 ? run_ik_site_step<double>(m->m64, cdof, subtree_com, site_xpos, site_xmat, site, body, target_pos, pos_stride, target_quat, quat_stride,
                                                        dof_sel, params, last, qpos, err_norm, steps, done, B, stream)
                             : run_ik_site_step<float>(m->m32, cdof, subtree_com, site_xpos, site_xmat, site, body, target_pos, pos_stride, target_quat, quat_stride,
                                                       dof_sel, params, last, qpos, err_norm, steps, done, B, stream);
}

int mjh_render(const mjhModel* m, const void* geom_xpos, const void* geom_xmat, const void* cam_xpos, const void* cam_xmat, const void* light_xpos,
               const void* light_xdir, int64_t B, const mjhRenderScene* scene, const mjhRenderParams* params, void* rgb, void* depth, int64_t* seg,
               void* stream) {
  if (!m || !scene || !params) return fail(-22, "null argument");
  return m->dtype == MJH_F64 ? run_render<double>(m->m64, geom_xpos, geom_xmat, cam_xpos, cam_xmat, light_xpos, light_xdir, B, scene, params, rgb, depth, seg, stream)
                             : run_render<float>(m->m32, geom_xpos, geom_xmat, cam_xpos, cam_xmat, light_xpos, light_xdir, B, scene, params, rgb, depth, seg, stream);
}

int mjh_support(const mjhModel* m, const mjhSupportArgs* args, void* stream) {
  if (!m || !args) return fail(-22, "null argument");
  return m->dtype == MJH_F64 ? run_support<double>(m, m->m64, args, stream) : run_support<float>(m, m->m32, args, stream);
}

int mjh_constraint_space(const mjhModel* m, const mjhConstraintSpaceArgs* args, void* stream) {
  if (!m || !args) return fail(-22, "null argument");
  return m->dtype == MJH_F64 ? run_constraint_space<double>(m->m64, args, stream) : run_constraint_space<float>(m->m32, args, stream);
}

int mjh_constraint_space_plan(int op, int nv, int nefc, int real_bytes, int* chunk_nchunk_last_lds) {
  if (op < MJH_EFC_MUL_J || op > MJH_EFC_AR || nv < 0 || nefc < 0 || (real_bytes != 4 && real_bytes != 8) || !chunk_nchunk_last_lds)
    return fail(-22, "constraint_space_plan: bad argument");
  if (efc_plan(op, nv, nefc, real_bytes, chunk_nchunk_last_lds)) return fail(-12, "constraint_space_plan: the operation does not fit the LDS of a workgroup");
  return 0;
}

int mjh_pgs(const mjhModel* m, const mjhPgsArgs* args, void* stream) {
  if (!m || !args) return fail(-22, "null argument");
  return m->dtype == MJH_F64 ? run_dual<double>(m->m64, args, stream, false, nullptr) : run_dual<float>(m->m32, args, stream, false, nullptr);
}

int mjh_pgs_plan(int nv, int nefc, int real_bytes, int* chunk_nchunk_last_lds) {
  if (nv < 0 || nefc < 0 || (real_bytes != 4 && real_bytes != 8) || !chunk_nchunk_last_lds) return fail(-22, "pgs_plan: bad argument");
  if (dual_plan(nv, nefc, 0, real_bytes, chunk_nchunk_last_lds)) return fail(-12, "pgs_plan: the model does not fit the LDS of a workgroup");
  return 0;
}

int mjh_solve(const mjhModel* m, const mjhSolveArgs* args, void* stream) {
  if (!m || !args) return fail(-22, "null argument");
  return m->dtype == MJH_F64 ? run_solve<double>(m->m64, args, stream) : run_solve<float>(m->m32, args, stream);
}

int mjh_solve_plan(int solver, int nv, int nefc, int real_bytes, int* chunk_nchunk_last_lds) {
  if ((solver != MJH_SOLVER_CG && solver != MJH_SOLVER_NEWTON) || nv < 0 || nefc < 0 || (real_bytes != 4 && real_bytes != 8) || !chunk_nchunk_last_lds)
    return fail(-22, "solve_plan: bad argument");
  if (solve_plan(solver, nv, nefc, real_bytes, chunk_nchunk_last_lds)) return fail(-12, "solve_plan: the model does not fit the LDS of a workgroup");
  return 0;
}

int mjh_noslip(const mjhModel* m, const mjhNoslipArgs* args, void* stream) {
  if (!m || !args) return fail(-22, "null argument");
  return m->dtype == MJH_F64 ? run_dual<double>(m->m64, args, stream, true, args->contact_friction) : run_dual<float>(m->m32, args, stream, true, args->contact_friction);
}

int mjh_noslip_plan(int nv, int nefc, int ncon, int real_bytes, int* chunk_nchunk_last_lds) {
  if (nv < 0 || nefc < 0 || ncon < 0 || (real_bytes != 4 && real_bytes != 8) || !chunk_nchunk_last_lds) return fail(-22, "noslip_plan: bad argument");
  if (dual_plan(nv, nefc, ncon, real_bytes, chunk_nchunk_last_lds)) return fail(-12, "noslip_plan: the model does not fit the LDS of a workgroup");
  return 0;
}

int mjh_postconstraint(const mjhModel* m, const mjhPostconArgs* args, void* stream) {
  if (!m || !args) return fail(-22, "null argument");
  return m->dtype == MJH_F64 ? run_postcon<double>(m, m->m64, args, stream) : run_postcon<float>(m, m->m32, args, stream);
}

int mjh_contact_sensors(const mjhModel* m, const mjhContactSensorArgs* args, void* stream) {
  if (!m || !args) return fail(-22, "null argument");
  return m->dtype == MJH_F64 ? run_consens<double>(m, m->m64, args, stream) : run_consens<float>(m, m->m32, args, stream);
}

int mjh_energy(const mjhModel* m, const mjhEnergyArgs* args, void* stream) {
  if (!m || !args) return fail(-22, "null argument");
  return m->dtype == MJH_F64 ? run_energy<double>(m, m->m64, args, stream) : run_energy<float>(m, m->m32, args, stream);
}

int mjh_jacobian(const mjhModel* m, const mjhJacobianArgs* args, void* stream) {
  if (!m || !args) return fail(-22, "null argument");
  return m->dtype == MJH_F64 ? run_jacobian<double>(m, m->m64, args, stream) : run_jacobian<float>(m, m->m32, args, stream);
}

int mjh_integrate(const mjhModel* m, const mjhIntegrateArgs* args, void* stream) {
  if (!m || !args) return fail(-22, "null argument");
  return m->dtype == MJH_F64 ? run_integrate<double>(m, m->m64, args, stream) : run_integrate<float>(m, m->m32, args, stream);
}

int mjh_smooth(const mjhModel* m, const mjhSmoothArgs* args, void* stream) {
  if (!m || !args) return fail(-22, "null argument");
  return m->dtype == MJH_F64 ? run_smooth<double>(m, m->m64, args, stream) : run_smooth<float>(m, m->m32, args, stream);
}

int mjh_dynamics(const mjhModel* m, const mjhDynamicsArgs* args, void* stream) {
  if (!m || !args) return fail(-22, "null argument");
  return m->dtype == MJH_F64 ? run_dynamics<double>(m, m->m64, args, stream) : run_dynamics<float>(m, m->m32, args, stream);
}

int mjh_dynamics_plan(int op, int nq, int nv, int nu, int nbody, int ntendon, int real_bytes, int* lanes_envs_lds) {
  if (op < MJH_DYNAMICS_TENDON || op > MJH_DYNAMICS_ACCELERATION || nq < 0 || nv < 0 || nu < 0 || nbody < 1 || ntendon < 0 || (real_bytes != 4 && real_bytes != 8) ||
      !lanes_envs_lds)
    return fail(-22, "dynamics_plan: bad argument");
  if (dynamics_plan(op, nq, nv, nu, nbody, ntendon, real_bytes, lanes_envs_lds)) return fail(-12, "dynamics_plan: one environment does not fit the LDS of a CU");
  return 0;
}

int mjh_smooth_plan(int op, int nbody, int nv, int ntendon, int real_bytes, int* lanes_envs_lds) {
  if (op < MJH_SMOOTH_COM_POS || op > MJH_SMOOTH_RNE || nbody < 1 || nv < 0 || ntendon < 0 || (real_bytes != 4 && real_bytes != 8) || !lanes_envs_lds)
    return fail(-22, "smooth_plan: bad argument");
  if (smooth_plan(op, nbody, nv, ntendon, real_bytes, lanes_envs_lds)) return fail(-12, "smooth_plan: one environment does not fit the LDS of a CU");
  return 0;
}

int mjh_integrate_plan(int nv, int nu, int ntendon, int real_bytes, int* lanes_envs_chunk_lds) {
  if (nv < 0 || nu < 0 || ntendon < 0 || (real_bytes != 4 && real_bytes != 8) || !lanes_envs_chunk_lds) return fail(-22, "integrate_plan: bad argument");
  return integrate_plan(nv, nu, ntendon, real_bytes, lanes_envs_chunk_lds);
}

int mjh_fd_perturb(const mjhModel* m, const mjhData* in, mjhData* scratch, int64_t B, int col0, int ncol, double eps, int centered, void* stream) {
  if (!m || !in || !scratch) return fail(-22, "null argument");
  return m->dtype == MJH_F64 ? run_fd_perturb<double, false>(m, m->m64, in, scratch, B, col0, ncol, eps, centered, stream)
                             : run_fd_perturb<float, false>(m, m->m32, in, scratch, B, col0, ncol, eps, centered, stream);
}

int mjh_fd_difference(const mjhModel* m, const mjhData* in, const mjhData* nominal, const mjhData* stepped, int64_t B, int col0, int ncol, double eps,
                      int centered, void* A, void* Bm, void* C, void* D, void* stream) {
  if (!m || !in || !nominal || !stepped) return fail(-22, "null argument");
  return m->dtype == MJH_F64 ? run_fd_difference<double>(m->m64, in, nominal, stepped, B, col0, ncol, eps, centered, A, Bm, C, D, stream)
                             : run_fd_difference<float>(m->m32, in, nominal, stepped, B, col0, ncol, eps, centered, A, Bm, C, D, stream);
}

int mjh_fd_vjp(const mjhModel* m, const mjhData* in, const mjhData* nominal, const mjhData* stepped, int64_t B, int col0, int ncol, double eps, int centered,
               const void* g_state, const void* g_sens, void* gx, void* gu, void* stream) {
  if (!m || !in || !nominal || !stepped) return fail(-22, "null argument");
  return m->dtype == MJH_F64 ? run_fd_vjp<double>(m->m64, in, nominal, stepped, B, col0, ncol, eps, centered, g_state, g_sens, gx, gu, stream)
                             : run_fd_vjp<float>(m->m32, in, nominal, stepped, B, col0, ncol, eps, centered, g_state, g_sens, gx, gu, stream);
}

int mjh_fd_tangent(const mjhModel* m, const void* qpos, const void* g_in, void* g_out, int64_t B, int mode, void* stream) {
  if (!m) return fail(-22, "null argument");
  return m->dtype == MJH_F64 ? run_fd_tangent<double>(m->m64, qpos, g_in, g_out, B, mode, stream)
                             : run_fd_tangent<float>(m->m32, qpos, g_in, g_out, B, mode, stream);
}

int mjh_ifd_perturb(const mjhModel* m, const mjhData* in, mjhData* scratch, int64_t B, int col0, int ncol, double eps, int centered, void* stream) {
  if (!m || !in || !scratch) return fail(-22, "null argument");
  return m->dtype == MJH_F64 ? run_fd_perturb<double, true>(m, m->m64, in, scratch, B, col0, ncol, eps, centered, stream)
                             : run_fd_perturb<float, true>(m, m->m32, in, scratch, B, col0, ncol, eps, centered, stream);
}

int mjh_ifd_difference(const mjhModel* m, const void* nominal_f, const void* nominal_sens, const void* stepped_f, const void* stepped_sens, int64_t B,
                       int col0, int ncol, double eps, int centered, void* DfDq, void* DfDv, void* DfDa, void* DsDq, void* DsDv, void* DsDa, void* stream) {
  if (!m) return fail(-22, "null argument");
  return m->dtype == MJH_F64
             ? run_ifd_difference<double>(m->m64, nominal_f, nominal_sens, stepped_f, stepped_sens, B, col0, ncol, eps, centered, DfDq, DfDv, DfDa, DsDq, DsDv, DsDa, stream)
             : run_ifd_difference<float>(m->m32, nominal_f, nominal_sens, stepped_f, stepped_sens, B, col0, ncol, eps, centered, DfDq, DfDv, DfDa, DsDq, DsDv, DsDa, stream);
}

int mjh_reset_where(const mjhModel* m, mjhData* d, const mjhData* d0, const unsigned char* mask, const void* qpos_rows,
                    const void* qvel_rows, int64_t B, void* stream) {
  if (!m || !d || !d0 || !mask) return fail(-22, "null argument");
  if (B <= 0) return 0;
  const int rw = m->dtype == MJH_F64 ? 2 : 1;  // 4-byte words per real
  ResetArgs a;
  memset(&a, 0, sizeof(a));
  a.mask = mask;
  void* const* dp = reinterpret_cast<void* const*>(d);
  void* const* sp = reinterpret_cast<void* const*>(d0);
  const char* names[] = {
#define X(n) #n,
      MJH_DATA_REALS(X) MJH_DATA_I32(X) MJH_DATA_I64(X)
#undef X
  };
  const size_t nreal = m->leaf_count.size();
  const int64_t ncon = m->dtype == MJH_F64 ? m->m64.ncon : m->m32.ncon;
  const int64_t neq = m->dtype == MJH_F64 ? m->m64.neq : m->m32.neq;
  const int64_t int_words[] = {ncon /* contact_dim */, neq /* eq_active */, 2 * ncon, 2 * ncon, 4 * ncon, 2 * ncon /* geom1, geom2, geom, efc_address (int64) */};
  const size_t nall = sizeof(names) / sizeof(names[0]);
  if (nall != nreal + 6 || nall > MJH_RESET_MAX_LEAVES) return fail(-22, "mjh_reset_where: leaf table out of sync with mjhData");
  for (size_t i = 0; i < nall; i++) {
    const int64_t words = i < nreal ? m->leaf_count[i] * rw : int_words[i - nreal];
    if (!dp[i] || words == 0) continue;  // leaf not carried by the caller's Data
    if (!sp[i]) return fail(-22, std::string("mjh_reset_where: d0.") + names[i] + " is null but d." + names[i] + " is not");
    ResetLeaf& L = a.leaf[a.nleaf++];
    L.dst = (unsigned*)dp[i]; L.src = (const unsigned*)sp[i]; L.words = (int)words;
    const void* rows = !strcmp(names[i], "qpos") ? qpos_rows : !strcmp(names[i], "qvel") ? qvel_rows : nullptr;
    if (rows) { L.src = (const unsigned*)rows; L.src_stride = (int)words; }
  }
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(mjh_reset_kernel, dim3((unsigned)B), dim3(256), 0, s, a);
  HIP_TRY(hipGetLastError());
  return 0;
}

/* measurement aid (bench.py): while enabled, every kernel launch of mjh_step / mjh_forward is bracketed by HIP events recorded
 * on the launch stream; mjh_debug_phase_times() waits for the last call and returns the elapsed time of each of its launches.
 * Not for concurrent callers; costs one hipEventRecord per launch while on. */
int mjh_debug_phase_timing(int enable) {
  if (enable && !g_timing.on) {
    for (int i = 0; i <= MJH_TIMING_MAX; i++) HIP_TRY(hipEventCreate(&g_timing.ev[i]));
    g_timing.on = true; g_timing.n = 0;
  } else if (!enable && g_timing.on) {
    for (int i = 0; i <= MJH_TIMING_MAX; i++) (void)hipEventDestroy(g_timing.ev[i]);
    g_timing.on = false; g_timing.n = 0;
  }
  return 0;
}
int mjh_debug_phase_times(float* ms, int* ids, int max) {
  if (!g_timing.on) return fail(-22, "mjh_debug_phase_timing(1) has not been called");
  const int n = g_timing.n < max ? g_timing.n : max;
  if (n > 0) HIP_TRY(hipEventSynchronize(g_timing.ev[g_timing.n]));
  for (int i = 0; i < n; i++) { HIP_TRY(hipEventElapsedTime(&ms[i], g_timing.ev[i], g_timing.ev[i + 1])); ids[i] = g_timing.id[i]; }
  return n;
}

/* diagnostic (-DMJH_STAMPS builds): device buffer [B, 128] of uint64 receiving in-kernel clock stamps */
void mjh_debug_set_stamps(void* dev_ptr) { g_stamps = (unsigned long long*)dev_ptr; }

int mjh_model_leaf_counts(const mjhModel* m, int64_t* counts, int max) {
  if (!m || !counts) return fail(-22, "null argument");
  const int64_t ncon = m->dtype == MJH_F64 ? m->m64.ncon : m->m32.ncon, neq = m->dtype == MJH_F64 ? m->m64.neq : m->m32.neq;
  std::vector<int64_t> all(m->leaf_count);
  const int64_t ints[] = {ncon /* contact_dim */, neq /* eq_active */, ncon, ncon, 2 * ncon, ncon /* geom1, geom2, geom, efc_address */};
  all.insert(all.end(), ints, ints + 6);
  for (int i = 0; i < (int)all.size() && i < max; i++) counts[i] = all[i];
  return (int)all.size();
}

// mjh_model_kernel_io's account of `kernel` in a scope: `inner` -- asked for as a part of another kernel's account (kernels 13 / 14 of a model with the whole-pass kernel
// are accounted inside it only); `stages13` -- the accounts of RK4 stages 1..3 alone (the stage kernel's parts)
static int kernel_io(const mjhModel* m, int kernel, int64_t* read_write_bytes, bool inner, bool stages13) {
  if ((kernel == MJH_KERNEL_SOL2) != (m->sol2_nmax != 0) && (kernel == MJH_KERNEL_SOL2 || kernel == MJH_KERNEL_SOL || kernel == MJH_KERNEL_SOL_GEN)) return -2;  // the solver phase runs as ONE of kernels 4 / 6 / 9
  if (kernel == MJH_KERNEL_KCV2) return m->kcv2 ? kernel_io(m, MJH_KERNEL_KCV, read_write_bytes, true, stages13) : -2;  // the two-wave form of kernel 13 moves the same bytes
  if (kernel == MJH_KERNEL_KCV && !m->fuse_kcv) return -2;  // (a model with kernel 13 reports both accounts: which one a step launches depends on the batch)
  if ((kernel == MJH_KERNEL_KV) != (m->fuse_kv != 0) && (kernel == MJH_KERNEL_KV || kernel == MJH_KERNEL_KIN || kernel == MJH_KERNEL_VEL)) return -2;  // kinematics + velocity: ONE kernel (12) or two (0, 3)
  const bool f64 = m->dtype == MJH_F64;
  const bool rk4 = (f64 ? m->m64.integrator : m->m32.integrator) == INT_RK4;
  auto io_of = [&](int k, int64_t* a) -> int {  // RK4: the mean over the four stage launches of a step (the sensor kernel runs once)
    int64_t b[2] = {0, 0};
    DevModel<double> m64 = m->m64;
    DevModel<float> m32 = m->m32;
    if (k == MJH_KERNEL_CONVEX || k == MJH_KERNEL_QUADRIC) m64.ncvxpair = m32.ncvxpair = k == MJH_KERNEL_CONVEX ? m->ncvx : m->nquad;  // (as their launches: the kernel's own pairs, NarrowedPairs)
    int rc = f64 ? mjh_kernel_io<double>(m64, k, 1, &a[0], &a[1]) : mjh_kernel_io<float>(m32, k, 1, &a[0], &a[1]);
    if (rc == 0 && rk4 && k != MJH_KERNEL_SENSOR) {
      rc = f64 ? mjh_kernel_io<double>(m64, k, 2, &b[0], &b[1]) : mjh_kernel_io<float>(m32, k, 2, &b[0], &b[1]);
      if (stages13) { a[0] = b[0]; a[1] = b[1]; }                             // the stage kernel: launches of stages 1..3 only
      else if (m->fuse_stage) {}                                               // ... whose model launches kernels 13 / 8 / 9 in stage 0 only
      else { a[0] = (a[0] + 3 * b[0]) / 4; a[1] = (a[1] + 3 * b[1]) / 4; }
    }
    return rc;
  };
  int64_t a[2] = {0, 0};
  if (kernel == MJH_KERNEL_RENDER) {  // the renderer (mjh_render), per environment and per output pixel: see include/mjhip.h
    const int64_t R = f64 ? 8 : 4, ng = f64 ? m->m64.ngeom : m->m32.ngeom, nc = f64 ? m->m64.ncam : m->m32.ncam, nl = f64 ? m->m64.nlight : m->m32.nlight;
    if (nc == 0) return -2;
    read_write_bytes[0] = (12 * ng + 12 + 6 * nl) * R;
    read_write_bytes[1] = (3 * R + R + 8);
    return 0;
  }
  if (kernel >= MJH_KERNEL_JAC && kernel <= MJH_KERNEL_SOLVE_M) {  // the support kernels (mjh_support), per environment: see include/mjhip.h
    const int64_t R = f64 ? 8 : 4, nv = f64 ? m->m64.nv : m->m32.nv, nb = f64 ? m->m64.nbody : m->m32.nbody;
    if (nv == 0) return -2;
    const int64_t io[5][2] = {{6 * nv + 3 + 3, 6 * nv}, {6 * nv + 3 + 9, nv}, {6 * nv + 3 * nb + 3 * nb + 6 * nb, nv}, {nv * nv + nv, nv}, {nv * nv + nv, nv}};
    read_write_bytes[0] = io[kernel - MJH_KERNEL_JAC][0] * R;
    read_write_bytes[1] = io[kernel - MJH_KERNEL_JAC][1] * R;
    return 0;
  }
  if (kernel == MJH_KERNEL_FD_PERTURB || kernel == MJH_KERNEL_FD_DIFFERENCE) {  // the finite-difference kernels (mjh_fd.h), per slot: see include/mjhip.h
    const int64_t R = f64 ? 8 : 4, nq = f64 ? m->m64.nq : m->m32.nq, nv = f64 ? m->m64.nv : m->m32.nv, na = f64 ? m->m64.na : m->m32.na, nu = f64 ? m->m64.nu : m->m32.nu;
    const int64_t nb = f64 ? m->m64.nbody : m->m32.nbody, nmo = f64 ? m->m64.nmocap : m->m32.nmocap, nsd = f64 ? m->m64.nsensordata : m->m32.nsensordata, neq = f64 ? m->m64.neq : m->m32.neq;
    if (kernel == MJH_KERNEL_FD_PERTURB) {  // time qpos qvel act qacc_warmstart ctrl qfrc_applied xfrc_applied mocap_* subtree_com qfrc_gravcomp actuator_force qfrc_constraint sensordata, the four trailing leaves, eq_active
      read_write_bytes[0] = read_write_bytes[1] = (1 + nq + 5 * nv + na + 2 * nu + 6 * nb + 7 * nmo + 3 * nb + nsd + 18 * nb) * R + 4 * neq;
    } else {
      read_write_bytes[0] = (nq + nv + na + nsd) * R;
      read_write_bytes[1] = (2 * nv + na + nsd) * R;
    }
    return 0;
  }
  if (kernel == MJH_KERNEL_IFD_PERTURB || kernel == MJH_KERNEL_IFD_DIFFERENCE) {  // the inverse-dynamics finite-difference kernels (mjh_ifd.h), per slot: see include/mjhip.h
    const int64_t R = f64 ? 8 : 4, nq = f64 ? m->m64.nq : m->m32.nq, nv = f64 ? m->m64.nv : m->m32.nv, na = f64 ? m->m64.na : m->m32.na, nu = f64 ? m->m64.nu : m->m32.nu;
    const int64_t nb = f64 ? m->m64.nbody : m->m32.nbody, nmo = f64 ? m->m64.nmocap : m->m32.nmocap, nsd = f64 ? m->m64.nsensordata : m->m32.nsensordata, neq = f64 ? m->m64.neq : m->m32.neq;
    if (nv == 0) return -2;
    if (kernel == MJH_KERNEL_IFD_PERTURB) {  // the leaves of MJH_KERNEL_FD_PERTURB, and qacc and qfrc_actuator
      read_write_bytes[0] = read_write_bytes[1] = (1 + nq + 7 * nv + na + 2 * nu + 6 * nb + 7 * nmo + 3 * nb + nsd + 18 * nb) * R + 4 * neq;
    } else {
      read_write_bytes[0] = read_write_bytes[1] = (nv + nsd) * R;
    }
    return 0;
  }
  if (kernel == MJH_KERNEL_FD_VJP || kernel == MJH_KERNEL_FD_TANGENT) {  // per (environment, column) and per environment: see include/mjhip.h
    const int64_t R = f64 ? 8 : 4, nq = f64 ? m->m64.nq : m->m32.nq, nv = f64 ? m->m64.nv : m->m32.nv, na = f64 ? m->m64.na : m->m32.na;
    const int64_t nsd = f64 ? m->m64.nsensordata : m->m32.nsensordata;
    if (nv == 0) return -2;
    if (kernel == MJH_KERNEL_FD_VJP) {
      read_write_bytes[0] = ((nq + nv + na + nsd) + (2 * nv + na + nsd)) * R;
      read_write_bytes[1] = R;
    } else {
      read_write_bytes[0] = 2 * nq * R;
      read_write_bytes[1] = nq * R;
    }
    return 0;
  }
  if (kernel == MJH_KERNEL_POSTCON) {  // body accelerations and forces (mjh_postconstraint, all three flags): every input leaf once, the six outputs
    const int64_t R = f64 ? 8 : 4, nv = f64 ? m->m64.nv : m->m32.nv, nb = f64 ? m->m64.nbody : m->m32.nbody, nefc = f64 ? m->m64.nefc : m->m32.nefc;
    const int64_t ncon = nefc > 0 ? (f64 ? m->m64.ncon : m->m32.ncon) : 0, ns = f64 ? m->m64.nsite : m->m32.nsite, nsd = f64 ? m->m64.nsensordata : m->m32.nsensordata;
    if (m->pc_envs == 0) return -2;
    // qvel qacc cdof cdof_dot | cvel cinert xipos ximat subtree_com xfrc_applied | efc_force | contact pos frame friction | dim, geom, efc_address | sites, sensordata
    read_write_bytes[0] = (14 * nv + (6 + 10 + 3 + 9 + 3 + 6) * nb + nefc + 17 * ncon + 12 * ns + nsd) * R + ncon * (4 + 16 + 8);
    read_write_bytes[1] = (24 * nb + nsd) * R;
    return 0;
  }
  if (kernel == MJH_KERNEL_ENERGY) {  // both energies (mjh_energy, MJH_ENERGY_POS | MJH_ENERGY_VEL): qpos, qvel, xipos, ten_length and qM once, two reals out
    const int64_t R = f64 ? 8 : 4, nq = f64 ? m->m64.nq : m->m32.nq, nv = f64 ? m->m64.nv : m->m32.nv, nb = f64 ? m->m64.nbody : m->m32.nbody, nt = f64 ? m->m64.ntendon : m->m32.ntendon;
    read_write_bytes[0] = (nq + nv + 3 * nb + nt + nv * nv) * R;
    read_write_bytes[1] = 2 * R;
    return 0;
  }
  if (kernel == MJH_KERNEL_GEOM_DISTANCE) {  // one (pair, environment) item of mjh_geom_distance: two frames and sizes and the pair's row in, dist and fromto out
    const int64_t R = f64 ? 8 : 4;
    if ((f64 ? m->m64.ngeom : m->m32.ngeom) == 0) return -2;
    read_write_bytes[0] = 30 * R + 16;
    read_write_bytes[1] = 7 * R;
    return 0;
  }
  if (kernel == MJH_KERNEL_QPOS_ARITH) {  // one environment of an integrate call of mjh_qpos_arith: qpos and qvel in, qpos out
    const int64_t R = f64 ? 8 : 4, nq = f64 ? m->m64.nq : m->m32.nq, nv = f64 ? m->m64.nv : m->m32.nv;
    if (nq == 0) return -2;
    read_write_bytes[0] = (nq + nv) * R;
    read_write_bytes[1] = nq * R;
    return 0;
  }
  if (kernel == MJH_KERNEL_IK_SITE) {  // one environment of an updating mjh_ik_site_step call with both targets
    const int64_t R = f64 ? 8 : 4, nq = f64 ? m->m64.nq : m->m32.nq, nv = f64 ? m->m64.nv : m->m32.nv;
    if (nv == 0 || (f64 ? m->m64.nsite : m->m32.nsite) == 0) return -2;
    read_write_bytes[0] = (6 * nv + 12 + 3 + 7 + nq + 1) * R + 4 + 1;
    read_write_bytes[1] = (nq + 1) * R + 4 + 1;
    return 0;
  }
  if (kernel >= MJH_KERNEL_EFC_MUL_J && kernel <= MJH_KERNEL_EFC_AR) {  // mjh_constraint_space, per environment: see include/mjhip.h
    const int64_t R = f64 ? 8 : 4, nv = f64 ? m->m64.nv : m->m32.nv, n = f64 ? m->m64.nefc : m->m32.nefc;
    if (nv == 0 || n == 0) return -2;
    const int64_t io[4][2] = {{n * nv + nv, n}, {n * nv + n, nv}, {n * nv + 3 * n + nv * nv + 3 * nv, 2 * n + 2 * nv + 3}, {n * nv + nv * nv + 2 * n + nv, n * n + n}};
    read_write_bytes[0] = io[kernel - MJH_KERNEL_EFC_MUL_J][0] * R;
    read_write_bytes[1] = io[kernel - MJH_KERNEL_EFC_MUL_J][1] * R + (kernel == MJH_KERNEL_EFC_UPDATE ? 4 * n : 0);
    return 0;
  }
  if (kernel == MJH_KERNEL_PGS || kernel == MJH_KERNEL_NOSLIP) {  // mjh_pgs / mjh_noslip, per environment: see include/mjhip.h
    const int64_t R = f64 ? 8 : 4, nv = f64 ? m->m64.nv : m->m32.nv, n = f64 ? m->m64.nefc : m->m32.nefc, ncon = f64 ? m->m64.ncon : m->m32.ncon;
    const bool elliptic = (f64 ? m->m64.cone : m->m32.cone) == CONE_ELLIPTIC;
    if (nv == 0 || n == 0) return -2;
    const int64_t start = kernel == MJH_KERNEL_PGS ? 0 : n + (elliptic ? 5 * ncon : 0);  // (no-slip: force0 and, with an elliptic cone, the friction)
    read_write_bytes[0] = (2 * n * nv + nv * nv + 3 * n + nv + start) * R;
    read_write_bytes[1] = (n + 2 * nv + 2) * R + 4;
    return 0;
  }
  if (kernel == MJH_KERNEL_SOLVE) {  // mjh_solve with the warm start on, per environment: see include/mjhip.h
    const int64_t R = f64 ? 8 : 4, nv = f64 ? m->m64.nv : m->m32.nv, n = f64 ? m->m64.nefc : m->m32.nefc;
    if (nv == 0 || n == 0) return -2;
    read_write_bytes[0] = (n * nv + 2 * nv * nv + 4 * n + 3 * nv) * R;
    read_write_bytes[1] = (n + 3 * nv + 3) * R + 4;
    return 0;
  }
  if (kernel >= MJH_KERNEL_JACOBIAN_POINT && kernel <= MJH_KERNEL_JACOBIAN_ANGMOM_VEC) {  // mjh_jacobian, per environment for one query: see include/mjhip.h
    const int64_t R = f64 ? 8 : 4, nv = f64 ? m->m64.nv : m->m32.nv, nb = f64 ? m->m64.nbody : m->m32.nbody;
    if (nv == 0) return -2;
    const bool vec = kernel >= MJH_KERNEL_JACOBIAN_POINT_VEC;
    const int op = kernel - (vec ? MJH_KERNEL_JACOBIAN_POINT_VEC : MJH_KERNEL_JACOBIAN_POINT);
    // POINT: cdof, the root's subtree_com, the point; DOT: cdof_dot and cvel too; SUBTREE_COM: cdof, subtree_com, xipos; ANGMOM: ximat too
    const int64_t rd[4] = {6 * nv + 3 + 3, 12 * nv + 3 + 3 + 6 * nb, 6 * nv + 6 * nb, 6 * nv + 15 * nb}, wr[4] = {6 * nv, 6 * nv, 3 * nv, 3 * nv};
    read_write_bytes[0] = (rd[op] + (vec ? nv : 0)) * R;
    read_write_bytes[1] = (vec ? wr[op] / nv : wr[op]) * R;
    return 0;
  }
  if (kernel >= MJH_KERNEL_SMOOTH_COM_POS && kernel <= MJH_KERNEL_SMOOTH_RNE) {  // mjh_smooth, per environment: see include/mjhip.h
    const int64_t R = f64 ? 8 : 4, nb = f64 ? m->m64.nbody : m->m32.nbody, nv = f64 ? m->m64.nv : m->m32.nv, nj = f64 ? m->m64.njnt : m->m32.njnt,
                  nt = f64 ? m->m64.ntendon : m->m32.ntendon;
    const int op = kernel - MJH_KERNEL_SMOOTH_COM_POS;
    if ((op != MJH_SMOOTH_COM_POS && op != MJH_SMOOTH_CRB && nv == 0) || (op == MJH_SMOOTH_TENDON_ARMATURE && nt == 0)) return -2;
    const int64_t rd[6] = {21 * nb + 6 * nj, 10 * nb + 6 * nv, nv * nv + nt * nv, (nv * (nv + 1)) / 2, 7 * nv, 14 * nv + 16 * nb};
    const int64_t wr[6] = {13 * nb + 6 * nv, 10 * nb + nv * nv, nv * nv, nv * nv, 6 * nb + 6 * nv, nv};
    read_write_bytes[0] = rd[op] * R;
    read_write_bytes[1] = wr[op] * R;
    return 0;
  }
  if (kernel >= MJH_KERNEL_DYNAMICS_TENDON && kernel <= MJH_KERNEL_DYNAMICS_ACCELERATION) return -2;  // mjh_dynamics: not accounted (include/mjhip.h)
  if (kernel == MJH_KERNEL_INTEGRATE) {  // an implicit step (mjh_integrate, QDERIV | IMPLICIT | STATE): the leaves it reads once (qM in full), the four state leaves out
    const int64_t R = f64 ? 8 : 4, nq = f64 ? m->m64.nq : m->m32.nq, nv = f64 ? m->m64.nv : m->m32.nv, nu = f64 ? m->m64.nu : m->m32.nu, na = f64 ? m->m64.na : m->m32.na,
                  nt = f64 ? m->m64.ntendon : m->m32.ntendon;
    read_write_bytes[0] = (nq + 3 * nv + 2 * na + 1 + nu + nv * nv + nu * nv + nt * nv) * R;
    read_write_bytes[1] = (nq + nv + na + 1) * R;
    return 0;
  }
  if (kernel == MJH_KERNEL_INVERSE) {  // the inverse-dynamics tail (mjh_inverse): efc_J and qM once, efc_D / efc_aref, qacc, qfrc_bias / passive in; efc_force, qfrc_constraint, qfrc_inverse out.
    // (the discrete branch reads qM a second time and the factor's lower triangle: not counted, it depends on the call's flags)
    const int64_t R = f64 ? 8 : 4, nv = f64 ? m->m64.nv : m->m32.nv, nefc = f64 ? m->m64.nefc : m->m32.nefc;
    read_write_bytes[0] = (nefc * nv + 2 * nefc + nv * nv + 3 * nv) * R;
    read_write_bytes[1] = (nefc + 2 * nv) * R;
    return 0;
  }
  if (kernel == MJH_KERNEL_PASS) {  // the whole pass in one launch: the accounts of kernels 13 and 14 (what the second half reads of the first it still reads from the leaves)
    if (!m->fuse_all) return -2;
    int64_t a13[2] = {0, 0}, a14[2] = {0, 0};
    if (kernel_io(m, MJH_KERNEL_KCV, a13, true, stages13) != 0 || kernel_io(m, MJH_KERNEL_CS, a14, true, stages13) != 0) return -2;
    read_write_bytes[0] = a13[0] + a14[0]; read_write_bytes[1] = a13[1] + a14[1];
    return 0;
  }
  if (kernel == MJH_KERNEL_STAGE) {  // one RK4 stage in one launch: the stage accounts of kernel 13, the constraint phase and the register solver (what a part reads of the previous one it still reads from the workspace leaves)
    if (!m->fuse_stage) return -2;
    int64_t a13[2] = {0, 0}, a8[2] = {0, 0}, a9[2] = {0, 0};
    if (kernel_io(m, MJH_KERNEL_KCV, a13, true, true) != 0 || kernel_io(m, MJH_KERNEL_CON_DIRECT, a8, true, true) != 0 || kernel_io(m, MJH_KERNEL_SOL2, a9, true, true) != 0) return -2;
    read_write_bytes[0] = a13[0] + a8[0] + a9[0]; read_write_bytes[1] = a13[1] + a8[1] + a9[1];
    return 0;
  }
  if (kernel == MJH_KERNEL_TAIL) {  // the tail of a pass in one launch: the accounts of the constraint phase and the register solver
    if (!m->fuse_tail) return -2;
    int64_t a8[2] = {0, 0}, a9[2] = {0, 0};
    if (kernel_io(m, MJH_KERNEL_CON_DIRECT, a8, true, stages13) != 0 || kernel_io(m, MJH_KERNEL_SOL2, a9, true, stages13) != 0) return -2;
    read_write_bytes[0] = a8[0] + a9[0]; read_write_bytes[1] = a8[1] + a9[1];
    return 0;
  }
  if ((kernel == MJH_KERNEL_KCV || kernel == MJH_KERNEL_CS) && m->fuse_all && !inner) return -2;
  if (kernel == MJH_KERNEL_CS) {  // constraint stage + register solver: the two accounts minus what stays in the arena between them -- the dense rows of efc_J, efc_D / efc_aref, one entry per single-column row, qvel
    if (!m->fuse_cs) return -2;
    int64_t k2[2] = {0, 0}, k4[2] = {0, 0};
    if (io_of(MJH_KERNEL_CON, k2) != 0 || io_of(MJH_KERNEL_SOL, k4) != 0) return -2;
    const int64_t R = f64 ? 8 : 4, nv = f64 ? m->m64.nv : m->m32.nv, nefc = f64 ? m->m64.nefc : m->m32.nefc, nl = f64 ? m->m64.nl : m->m32.nl;
    read_write_bytes[0] = k2[0] + k4[0] - ((nefc - nl) * nv + 2 * nefc + nl + nv) * R;
    read_write_bytes[1] = k2[1] + k4[1];
    return 0;
  }
  if ((kernel == MJH_KERNEL_CON || kernel == MJH_KERNEL_SOL2) && m->fuse_cs) return -2;  // (a full pass of this model launches kernel 14 instead)
  if (kernel == MJH_KERNEL_KV || kernel == MJH_KERNEL_KCV) {  // the accounts of the fused stages minus what stays in the arena between them: qpos, cdof, cinert, subtree_com, xipos are not read back (13: nor cinert, cdof by the crb stage)
    int64_t k0[2] = {0, 0}, k3[2] = {0, 0}, k1[2] = {0, 0};
    if (io_of(MJH_KERNEL_KIN, k0) != 0 || io_of(MJH_KERNEL_VEL, k3) != 0 || (kernel == MJH_KERNEL_KCV && io_of(MJH_KERNEL_CRB, k1) != 0)) return -2;
    const int64_t R = f64 ? 8 : 4, nq = f64 ? m->m64.nq : m->m32.nq, nv = f64 ? m->m64.nv : m->m32.nv, nb = f64 ? m->m64.nbody : m->m32.nbody;
    read_write_bytes[0] = k0[0] + k3[0] - (nq + 6 * nv + 10 * nb + 3 * nb + 3 * nb) * R + (kernel == MJH_KERNEL_KCV ? k1[0] - (10 * nb + 6 * nv) * R : 0);
    read_write_bytes[1] = k0[1] + k3[1] + (kernel == MJH_KERNEL_KCV ? k1[1] : 0);
    return 0;
  }
  const int k = kernel == MJH_KERNEL_SOL2 ? MJH_KERNEL_SOL : kernel;  // the register solver moves the same leaves as the plain LDS solver
  if (io_of(k, a) != 0) return -2;  // -2: this model's step does not launch that kernel
  read_write_bytes[0] = a[0]; read_write_bytes[1] = a[1];
  return 0;
}
int mjh_model_kernel_io(const mjhModel* m, int kernel, int64_t* read_write_bytes) {
  if (!m || !read_write_bytes) return fail(-22, "null argument");
  return kernel_io(m, kernel, read_write_bytes, false, false);
}

int64_t mjh_model_work_bytes(const mjhModel* m) { return m ? m->work_reals * (m->dtype == MJH_F64 ? 8 : 4) : 0; }
int mjh_model_lds_bytes(const mjhModel* m, int arena) {  // the query numbers of include/mjhip.h: 0..5 the arenas carved per model, 16..19 the others
  if (!m) return 0;
  if (arena >= 0 && arena < MJH_NARENA) return m->lds((Arena)arena);
  if (arena == 16) return m->lds(AR_TIER);
  if (arena == 17) return m->lds(AR_KCV);
  if (arena == 18) return m->lds(AR_CS);
  if (arena == 19) return m->lds(AR_KCV2);
  return 0;
}
const char* mjh_last_error(void) { return g_err.c_str(); }
int mjh_abi_version(void) { return MJH_ABI_VERSION; }

#define STR_(x) #x
const char* mjh_data_fields(void) {
  static const char s[] =
#define X(n) STR_(n) ","
      MJH_DATA_REALS(X) MJH_DATA_I32(X) MJH_DATA_I64(X)
#undef X
      ;
  static std::string t = std::string(s).substr(0, sizeof(s) - 2);
  return t.c_str();
}
const char* mjh_data_extra_fields(void) {  // the input-only leaves that trail mjhData (MJH_DATA_EXTRA_IN)
  static const char s[] =
#define X(n) STR_(n) ","
      MJH_DATA_EXTRA_IN(X)
#undef X
      ;
  static std::string t = std::string(s).substr(0, sizeof(s) - 2);
  return t.c_str();
}
int mjh_sizeof_data(void) { return (int)sizeof(mjhData); }
const char* mjh_model_fields(void) {
  static const char s[] =
#define X(n) STR_(n) ","
      MJH_MODEL_INTS(X) MJH_MODEL_REALS(X) MJH_MODEL_INT_ARRAYS(X) MJH_MODEL_REAL_ARRAYS(X)
#undef X
      ;
  static std::string t = std::string(s).substr(0, sizeof(s) - 2);
  return t.c_str();
}

}  // extern "C"
