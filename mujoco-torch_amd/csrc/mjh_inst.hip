// mjh_inst.hip -- one build group of kernel instantiations (mjh_instances.h).  Compiled once per (group, dtype) by build.sh:
//   hipcc -c -DMJH_INST_GROUP=<g> -DMJH_INST_REAL=<double|float> mjh_inst.hip
#include <hip/hip_runtime.h>

#include "mjh_kernels.h"
#include "mjh_convex.h"
#include "mjh_sensor.h"
#include "mjh_inverse.h"
#include "mjh_ray.h"
#include "mjh_render.h"
#include "mjh_support.h"
#include "mjh_fd.h"
#include "mjh_ifd.h"
#include "mjh_postcon.h"
#include "mjh_contact_sensors.h"
#include "mjh_energy.h"
#include "mjh_integrate.h"
#include "mjh_jacobian.h"
#include "mjh_quadric.h"
#include "mjh_geomdist.h"
#include "mjh_qpos.h"
#include "mjh_ik.h"
#include "mjh_efc.h"
#include "mjh_pgs.h"
#include "mjh_noslip.h"
#include "mjh_solve.h"
#include "mjh_smooth.h"
#include "mjh_dynamics.h"
#include "mjh_instances.h"

#define MJH_CAT_(a, b) a##b
#define MJH_CAT(a, b) MJH_CAT_(a, b)
#define X_(R, P, W) template __global__ void mjh_phase_kernel<R, P, W>(KArgs<R>);
#define S_(R, N, RPL, W) template __global__ void mjh_sol2_kernel<R, N, RPL, W>(KArgs<R>);
#define C_(R) template __global__ void mjh_convex_kernel<R>(KArgs<R>);
#define N_(R) template __global__ void mjh_sensor_kernel<R, 0>(KArgs<R>); template __global__ void mjh_sensor_kernel<R, 1>(KArgs<R>);
MJH_CAT(MJH_INST_G, MJH_INST_GROUP)(X_, S_, C_, N_, MJH_INST_REAL)
#if MJH_INST_GROUP == 19
template __global__ void mjh_inverse_kernel<MJH_INST_REAL>(InvArgs<MJH_INST_REAL>);
#endif
#if MJH_INST_GROUP == 20
template __global__ void mjh_ray_kernel<MJH_INST_REAL>(RayArgs<MJH_INST_REAL>);
#endif
#if MJH_INST_GROUP == 21
template __global__ void mjh_render_kernel<MJH_INST_REAL>(RenderArgs<MJH_INST_REAL>);
#endif
#if MJH_INST_GROUP == 22
template __global__ void mjh_sup_point_kernel<MJH_INST_REAL, true>(SupArgs<MJH_INST_REAL>);
template __global__ void mjh_sup_point_kernel<MJH_INST_REAL, false>(SupArgs<MJH_INST_REAL>);
template __global__ void mjh_sup_xfrc_kernel<MJH_INST_REAL>(SupArgs<MJH_INST_REAL>);
template __global__ void mjh_sup_mulm_kernel<MJH_INST_REAL>(SupArgs<MJH_INST_REAL>);
template __global__ void mjh_sup_solvem_kernel<MJH_INST_REAL>(SupArgs<MJH_INST_REAL>);
#endif
#if MJH_INST_GROUP == 23
template __global__ void mjh_fd_perturb_kernel<MJH_INST_REAL>(FdPerturbArgs<MJH_INST_REAL>);
template __global__ void mjh_fd_difference_kernel<MJH_INST_REAL>(FdDiffArgs<MJH_INST_REAL>);
template __global__ void mjh_fd_vjp_kernel<MJH_INST_REAL>(FdVjpArgs<MJH_INST_REAL>);
template __global__ void mjh_fd_tangent_kernel<MJH_INST_REAL>(FdTangentArgs<MJH_INST_REAL>);
#endif
#if MJH_INST_GROUP == 24
template __global__ void mjh_postcon_kernel<MJH_INST_REAL>(PostconArgs<MJH_INST_REAL>);
#endif
#if MJH_INST_GROUP == 25
template __global__ void mjh_consens_kernel<MJH_INST_REAL>(ConSensArgs<MJH_INST_REAL>);
#endif
#if MJH_INST_GROUP == 26
template __global__ void mjh_energy_kernel<MJH_INST_REAL>(EnergyArgs<MJH_INST_REAL>);
#endif
#if MJH_INST_GROUP == 27
template __global__ void mjh_integrate_kernel<MJH_INST_REAL>(IntegrateArgs<MJH_INST_REAL>);
#endif
#if MJH_INST_GROUP == 28
template __global__ void mjh_jac_matrix_kernel<MJH_INST_REAL>(JacArgs<MJH_INST_REAL>);
template __global__ void mjh_jac_product_kernel<MJH_INST_REAL>(JacArgs<MJH_INST_REAL>);
#endif
#if MJH_INST_GROUP == 29
template __global__ void mjh_quadric_kernel<MJH_INST_REAL>(KArgs<MJH_INST_REAL>);
#endif
#if MJH_INST_GROUP == 30
template __global__ void mjh_ifd_perturb_kernel<MJH_INST_REAL>(FdPerturbArgs<MJH_INST_REAL>);
template __global__ void mjh_ifd_difference_kernel<MJH_INST_REAL>(IfdDiffArgs<MJH_INST_REAL>);
#endif
#if MJH_INST_GROUP == 31
template __global__ void mjh_geomdist_kernel<MJH_INST_REAL>(GeomDistArgs<MJH_INST_REAL>);
#endif
#if MJH_INST_GROUP == 32
template __global__ void mjh_qpos_arith_kernel<MJH_INST_REAL>(QposArithArgs<MJH_INST_REAL>);
template __global__ void mjh_ik_site_kernel<MJH_INST_REAL, 1>(IkSiteArgs<MJH_INST_REAL>);
template __global__ void mjh_ik_site_kernel<MJH_INST_REAL, 2>(IkSiteArgs<MJH_INST_REAL>);
template __global__ void mjh_ik_site_kernel<MJH_INST_REAL, 3>(IkSiteArgs<MJH_INST_REAL>);
#endif
#if MJH_INST_GROUP == 33
template __global__ void mjh_efc_mulj_kernel<MJH_INST_REAL>(EfcArgs<MJH_INST_REAL>);
template __global__ void mjh_efc_muljt_kernel<MJH_INST_REAL>(EfcArgs<MJH_INST_REAL>);
template __global__ void mjh_efc_update_kernel<MJH_INST_REAL>(EfcArgs<MJH_INST_REAL>);
template __global__ void mjh_efc_ar_kernel<MJH_INST_REAL>(EfcArgs<MJH_INST_REAL>);
#endif
#if MJH_INST_GROUP == 34
template __global__ void mjh_pgs_kernel<MJH_INST_REAL>(PgsArgs<MJH_INST_REAL>);
#endif
#if MJH_INST_GROUP == 35
template __global__ void mjh_noslip_kernel<MJH_INST_REAL>(NoslipArgs<MJH_INST_REAL>);
#endif
#if MJH_INST_GROUP == 36
template __global__ void mjh_solve_kernel<MJH_INST_REAL>(SolveArgs<MJH_INST_REAL>);
#endif
#if MJH_INST_GROUP == 37
template __global__ void mjh_smooth_kernel<MJH_INST_REAL, MJH_SMOOTH_COM_POS>(SmoothArgs<MJH_INST_REAL>);
template __global__ void mjh_smooth_kernel<MJH_INST_REAL, MJH_SMOOTH_CRB>(SmoothArgs<MJH_INST_REAL>);
template __global__ void mjh_smooth_kernel<MJH_INST_REAL, MJH_SMOOTH_TENDON_ARMATURE>(SmoothArgs<MJH_INST_REAL>);
template __global__ void mjh_smooth_kernel<MJH_INST_REAL, MJH_SMOOTH_FACTOR_M>(SmoothArgs<MJH_INST_REAL>);
template __global__ void mjh_smooth_kernel<MJH_INST_REAL, MJH_SMOOTH_COM_VEL>(SmoothArgs<MJH_INST_REAL>);
template __global__ void mjh_smooth_kernel<MJH_INST_REAL, MJH_SMOOTH_RNE>(SmoothArgs<MJH_INST_REAL>);
#endif
#if MJH_INST_GROUP == 38
template __global__ void mjh_dynamics_kernel<MJH_INST_REAL, MJH_DYNAMICS_TENDON>(DynArgs<MJH_INST_REAL>);
template __global__ void mjh_dynamics_kernel<MJH_INST_REAL, MJH_DYNAMICS_TRANSMISSION>(DynArgs<MJH_INST_REAL>);
template __global__ void mjh_dynamics_kernel<MJH_INST_REAL, MJH_DYNAMICS_VELOCITY>(DynArgs<MJH_INST_REAL>);
template __global__ void mjh_dynamics_kernel<MJH_INST_REAL, MJH_DYNAMICS_PASSIVE>(DynArgs<MJH_INST_REAL>);
template __global__ void mjh_dynamics_kernel<MJH_INST_REAL, MJH_DYNAMICS_ACTUATION>(DynArgs<MJH_INST_REAL>);
template __global__ void mjh_dynamics_kernel<MJH_INST_REAL, MJH_DYNAMICS_ACCELERATION>(DynArgs<MJH_INST_REAL>);
#endif
