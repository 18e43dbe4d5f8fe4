// mjh_instances.h -- the list of kernel instantiations the library ships, cut into build groups.
//
// Every kernel is one fully inlined function of several thousand lines; compiled in one translation unit the library took four minutes.
// Each group below is compiled by its own hipcc process (mjh_inst.hip with -DMJH_INST_GROUP=g -DMJH_INST_REAL=double|float, build.sh runs
// them in parallel); mjhip.hip sees the same list as `extern template` declarations, so it holds the host side only.
// X(REAL, PHASE, W) for mjh_phase_kernel (PHASE: an MJH_KERNEL_* id, W: lanes per environment), S(REAL, NMAX, RPL, WT) for mjh_sol2_kernel (WT: a SOL2_* form,
// mjh_kernels.h), C(REAL) / N(REAL) for the convex and sensor kernels.
#pragma once

#define MJH_INST_G0(X, S, C, N, R) X(R, MJH_KERNEL_KIN, 64) X(R, MJH_KERNEL_KIN, 32) X(R, MJH_KERNEL_KIN, 16)
#define MJH_INST_G1(X, S, C, N, R) X(R, MJH_KERNEL_CRB, 64) X(R, MJH_KERNEL_CRB, 32) X(R, MJH_KERNEL_CRB, 16) X(R, MJH_KERNEL_CON, 64)
#define MJH_INST_G2(X, S, C, N, R) X(R, MJH_KERNEL_VEL, 64) X(R, MJH_KERNEL_VEL, 32) X(R, MJH_KERNEL_VEL, 16)
#define MJH_INST_G3(X, S, C, N, R) X(R, MJH_KERNEL_KV, 64) X(R, MJH_KERNEL_KV, 32) X(R, MJH_KERNEL_KV, 16)
#define MJH_INST_G4(X, S, C, N, R) X(R, MJH_KERNEL_VEL_OPT, 64) X(R, MJH_KERNEL_VEL_OPT, 32) X(R, MJH_KERNEL_VEL_OPT, 16)
#define MJH_INST_G5(X, S, C, N, R) X(R, MJH_KERNEL_SOL, 64) X(R, MJH_KERNEL_SOL_GEN, 64) X(R, MJH_KERNEL_CON_GEN, 64)
#define MJH_INST_G6(X, S, C, N, R) X(R, MJH_KERNEL_CON_DIRECT, 64) X(R, MJH_KERNEL_CON_DIRECT, 32) C(R) N(R)
#define MJH_INST_G7(X, S, C, N, R) S(R, 8, 1, SOL2_PAIR) S(R, 8, 2, SOL2_PAIR) S(R, 8, 4, SOL2_PAIR) S(R, 8, 8, SOL2_PAIR)
#define MJH_INST_G8(X, S, C, N, R) S(R, 16, 1, SOL2_PAIR) S(R, 16, 2, SOL2_PAIR) S(R, 16, 4, SOL2_PAIR) S(R, 16, 8, SOL2_PAIR)
#define MJH_INST_G9(X, S, C, N, R) S(R, 28, 1, SOL2_PAIR) S(R, 28, 2, SOL2_PAIR)
#define MJH_INST_G10(X, S, C, N, R) S(R, 8, 2, SOL2_QUAD) S(R, 8, 5, SOL2_QUAD) S(R, 12, 2, SOL2_QUAD) S(R, 12, 5, SOL2_QUAD)  /* four environments per wavefront (nv <= 16) */
#define MJH_INST_G11(X, S, C, N, R) S(R, 16, 2, SOL2_QUAD) S(R, 16, 5, SOL2_QUAD)
#define MJH_INST_G13(X, S, C, N, R) S(R, 8, 2, SOL2_QUAD_NEWTON) S(R, 8, 5, SOL2_QUAD_NEWTON) S(R, 12, 2, SOL2_QUAD_NEWTON) S(R, 12, 5, SOL2_QUAD_NEWTON)  /* ... the same for Newton models (Newton-only code) */
#define MJH_INST_G14(X, S, C, N, R) S(R, 16, 2, SOL2_QUAD_NEWTON) S(R, 16, 5, SOL2_QUAD_NEWTON)
#define MJH_INST_G12(X, S, C, N, R) X(R, MJH_KERNEL_KCV, 64) X(R, MJH_KERNEL_KCV, 32) X(R, MJH_KERNEL_KCV, 16)  /* kinematics + crb + velocity in one launch */
#define MJH_INST_G15(X, S, C, N, R) S(R, 28, 1, SOL2_CS) S(R, 28, 1, SOL2_CS_ONE)  /* constraint stage + register solver + integrator in one kernel (generic; opt.iterations == 1) */
#define MJH_INST_G16(X, S, C, N, R) S(R, 28, 1, SOL2_PASS) S(R, 28, 1, SOL2_PASS_ONE)  /* the whole pass -- kinematics + crb + velocity + constraint stage + register solver + integrator -- in one kernel */
#define MJH_INST_G17(X, S, C, N, R) X(R, MJH_KERNEL_KCV2, 32) X(R, MJH_KERNEL_KCV2, 16)  /* kernel 13 on two wavefronts per workgroup: kinematics, then velocity beside crb / factor */
#define MJH_INST_G18(X, S, C, N, R) S(R, 8, 2, SOL2_STAGE) S(R, 8, 5, SOL2_STAGE)  /* one RK4 stage of a small Newton model in one launch: kernel 13's stages + constraint phase + the solver's first tier */
#define MJH_INST_G19(X, S, C, N, R)  /* the inverse-dynamics tail (mjh_inverse_kernel, mjh_inverse.h): instantiated by mjh_inst.hip for this group */
#define MJH_INST_G20(X, S, C, N, R)  /* the ray-casting kernel (mjh_ray_kernel, mjh_ray.h): instantiated by mjh_inst.hip for this group */
#define MJH_INST_G21(X, S, C, N, R)  /* the ray-cast renderer (mjh_render_kernel, mjh_render.h): instantiated by mjh_inst.hip for this group */
#define MJH_INST_G22(X, S, C, N, R)  /* the support kernels (mjh_sup_*_kernel, mjh_support.h): instantiated by mjh_inst.hip for this group */
#define MJH_INST_G23(X, S, C, N, R)  /* the finite-difference kernels (mjh_fd_*_kernel, mjh_fd.h): instantiated by mjh_inst.hip for this group */
#define MJH_INST_G24(X, S, C, N, R)  /* body accelerations and forces (mjh_postcon_kernel, mjh_postcon.h): instantiated by mjh_inst.hip for this group */
#define MJH_INST_G25(X, S, C, N, R)  /* contact forces and their sensors (mjh_consens_kernel, mjh_contact_sensors.h): instantiated by mjh_inst.hip for this group */
#define MJH_INST_G26(X, S, C, N, R)  /* energies and the limit / energy sensors (mjh_energy_kernel, mjh_energy.h): instantiated by mjh_inst.hip for this group */
#define MJH_INST_G27(X, S, C, N, R)  /* deriv_smooth_vel and the implicit / Euler integrators (mjh_integrate_kernel, mjh_integrate.h): instantiated by mjh_inst.hip for this group */
#define MJH_INST_G28(X, S, C, N, R)  /* the Jacobian block (mjh_jac_matrix_kernel / mjh_jac_product_kernel, mjh_jacobian.h): instantiated by mjh_inst.hip for this group */
#define MJH_INST_G29(X, S, C, N, R)  /* the plane-ellipsoid / plane-cylinder narrow phase (mjh_quadric_kernel, mjh_quadric.h): instantiated by mjh_inst.hip for this group */
#define MJH_INST_G30(X, S, C, N, R)  /* the inverse-dynamics finite-difference kernels (mjh_ifd_*_kernel, mjh_ifd.h): instantiated by mjh_inst.hip for this group */
#define MJH_INST_G31(X, S, C, N, R)  /* geom-pair distances (mjh_geomdist_kernel, mjh_geomdist.h): instantiated by mjh_inst.hip for this group */
#define MJH_INST_G32(X, S, C, N, R)  /* configuration arithmetic and the site-pose IK iteration (mjh_qpos_arith_kernel, mjh_qpos.h; mjh_ik_site_kernel, mjh_ik.h): instantiated by mjh_inst.hip for this group */
#define MJH_INST_G33(X, S, C, N, R)  /* the constraint-space kernels (mjh_efc_*_kernel, mjh_efc.h): instantiated by mjh_inst.hip for this group */
#define MJH_INST_G34(X, S, C, N, R)  /* projected Gauss-Seidel on the dual problem (mjh_pgs_kernel, mjh_pgs.h): instantiated by mjh_inst.hip for this group */
#define MJH_INST_G35(X, S, C, N, R)  /* the no-slip friction post-solver (mjh_noslip_kernel, mjh_noslip.h): instantiated by mjh_inst.hip for this group */
#define MJH_INST_G36(X, S, C, N, R)  /* the CG / Newton primal solver on a finished pass (mjh_solve_kernel, mjh_solve.h): instantiated by mjh_inst.hip for this group */
#define MJH_INST_G37(X, S, C, N, R)  /* the smooth-dynamics stages on a caller's Data (mjh_smooth_kernel, mjh_smooth.h): instantiated by mjh_inst.hip for this group */
#define MJH_INST_G38(X, S, C, N, R)  /* tendon, transmission, passive and the forward stages on a caller's Data (mjh_dynamics_kernel, mjh_dynamics.h): instantiated by mjh_inst.hip for this group */
#define MJH_INST_NGROUPS 39

#define MJH_INST_ALL(X, S, C, N, R)                                                                                            \
  MJH_INST_G0(X, S, C, N, R) MJH_INST_G1(X, S, C, N, R) MJH_INST_G2(X, S, C, N, R) MJH_INST_G3(X, S, C, N, R) MJH_INST_G4(X, S, C, N, R) \
  MJH_INST_G5(X, S, C, N, R) MJH_INST_G6(X, S, C, N, R) MJH_INST_G7(X, S, C, N, R) MJH_INST_G8(X, S, C, N, R) MJH_INST_G9(X, S, C, N, R) MJH_INST_G10(X, S, C, N, R) MJH_INST_G11(X, S, C, N, R) MJH_INST_G12(X, S, C, N, R) MJH_INST_G13(X, S, C, N, R) MJH_INST_G14(X, S, C, N, R) MJH_INST_G15(X, S, C, N, R) MJH_INST_G16(X, S, C, N, R) MJH_INST_G17(X, S, C, N, R) MJH_INST_G18(X, S, C, N, R) MJH_INST_G19(X, S, C, N, R) MJH_INST_G20(X, S, C, N, R) MJH_INST_G21(X, S, C, N, R) MJH_INST_G22(X, S, C, N, R) MJH_INST_G23(X, S, C, N, R) MJH_INST_G24(X, S, C, N, R) MJH_INST_G25(X, S, C, N, R) MJH_INST_G26(X, S, C, N, R) MJH_INST_G27(X, S, C, N, R) MJH_INST_G28(X, S, C, N, R) MJH_INST_G29(X, S, C, N, R) MJH_INST_G30(X, S, C, N, R) MJH_INST_G31(X, S, C, N, R) MJH_INST_G32(X, S, C, N, R) MJH_INST_G33(X, S, C, N, R) MJH_INST_G34(X, S, C, N, R) MJH_INST_G35(X, S, C, N, R) MJH_INST_G36(X, S, C, N, R) MJH_INST_G37(X, S, C, N, R) MJH_INST_G38(X, S, C, N, R)
