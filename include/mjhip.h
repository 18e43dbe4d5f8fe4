/*
 * mjhip.h -- C ABI of the MI355X-native batched stepper behind mujoco_torch.step().
 *
 * The reference (vmoens/mujoco-torch) has NO native boundary: its step is pure Python
 * (mujoco_torch/_src/forward.py:463-496) vectorised with torch.vmap.  This header is the
 * boundary a maintainer binds instead; each entry point names the reference call it replaces:
 *
 *   mjh_model_create   <- Model.to(device) + _build_device_precomp   (_src/types.py:949-1013)
 *   mjh_forward        <- forward.forward(m, d)                       (_src/forward.py:373-401)
 *   mjh_step           <- forward.step(m, d, fixed_iterations)        (_src/forward.py:463-496)
 *   mjh_inverse        <- inverse.inverse(m, d)                       (_src/inverse.py:86-102)
 *   mjh_ray            <- ray.ray(m, d, pnt, vec, ...)               (_src/ray.py:375-452)
 *   mjh_render         <- render.render_batch(m, d, camera_id, ...)   (_src/render.py:719-907)
 *   mjh_fd_perturb / mjh_fd_difference <- the two ends of a finite-difference transition Jacobian (MuJoCo's mjd_transitionFD; the reference has no counterpart)
 *   mjh_fd_vjp / mjh_fd_tangent        <- its vector-Jacobian product and the quaternion coordinate maps of a gradient through one step
 *   mjh_ifd_perturb / mjh_ifd_difference <- the two ends of a finite-difference Jacobian of inverse dynamics (MuJoCo's mjd_inverseFD; the reference has no counterpart)
 *   mjh_support        <- support.jac / apply_ft / xfrc_accumulate, smooth.mul_m / solve_m (_src/support.py:138-194, smooth.py:335-374)
 *   mjh_postconstraint <- MuJoCo's mj_rnePostConstraint / mj_subtreeVel (MJX smooth.rne_postconstraint / subtree_vel; the reference has no counterpart)
 *   mjh_contact_sensors <- MuJoCo's mj_contactForce (MJX support.contact_force) and its touch / framelinacc / frameangacc sensors (the reference evaluates none of them)
 *   mjh_energy         <- MuJoCo's mj_energyPos / mj_energyVel and its joint / tendon limit and energy sensors (the reference evaluates none of them)
 *   mjh_geom_distance  <- MuJoCo's mj_geomDistance: signed distance and nearest points of geom pairs (the reference has no counterpart)
 *   mjh_qpos_arith     <- MuJoCo's mj_integratePos / mj_differentiatePos / mj_normalizeQuat on plain rows (forward._integrate_pos, math.quat_sub: _src/forward.py:231-252, math.py:276-280)
 *   mjh_ik_site_step   <- one damped-least-squares iteration of site-pose inverse kinematics (dm_control's qpos_from_site_pose; the reference has no counterpart)
 *   mjh_constraint_space <- MuJoCo's mj_mulJacVec / mj_mulJacTVec / mj_constraintUpdate and the Delassus matrix efc_AR, by the reference solver's definitions (_src/solver.py:293-357, 501-508)
 *   mjh_pgs            <- MuJoCo's mj_solPGS for rows of dimension one, on the dual problem of a finished pass (the reference's solvers are CG and Newton alone)
 *   mjh_noslip         <- MuJoCo's mj_solNoSlip (noslip_iterations): Gauss-Seidel on the friction dimensions with the unregularised matrix, after the main solver (the reference has no counterpart)
 *   mjh_solve          <- solver.solve(m, d, fixed_iterations) on a caller's Data: the CG / Newton primal solver with its exact line search (_src/solver.py:244-553)
 *   mjh_smooth         <- smooth.com_pos, crb, tendon_armature, factor_m, com_vel and rne on a caller's Data (_src/smooth.py:210-332, 385-467, 500-521)
 *   mjh_dynamics       <- smooth.tendon, transmission, passive.passive and forward's _velocity products, _actuation, _acceleration on a caller's Data (_src/smooth.py:470-497, 535-591, passive.py, forward.py:87-228)
 *   mjh_jacobian       <- MuJoCo's mj_jacBody .. mj_jacGeom (as products), mj_jacDot, mj_jacSubtreeCom, mj_angmomMat (the reference has support.jac alone)
 *   mjh_integrate      <- derivative.deriv_smooth_vel, forward._implicit (implicitfast), forward._euler and their _advance, on a finished pass (_src/derivative.py:22-68, forward.py:255-328, 404-416)
 *
 * Conventions
 *  - every Data leaf is batch-major contiguous: shape [B, ...] exactly as
 *    make_data(mx).expand(B).clone() lays it out (reference benchmarks/_helpers.py:37-41);
 *  - all pointers in mjhData are DEVICE pointers for the mjh_* entry points and HOST pointers
 *    for the oracle twin (oracle/mjoracle.c: mjo_forward / mjo_step, same structs);
 *  - "real" fields are double (dtype 0) or float (dtype 1) for the whole call;
 *  - functions return 0 on success or a negative errno-style code; they never throw, never
 *    allocate, never synchronise: work is enqueued on the given hipStream_t (passed as void*);
 *  - the caller owns every buffer.  `in` and `out` may alias field-by-field only for fields
 *    the step does not write (qacc/qacc_warmstart outputs must be distinct storage, mirroring
 *    reference solver.py:541-548).
 *
 * The X-macro lists below are the single source of truth for field order; the Python host
 * side (mujoco_torch_amd/native.py) parses them to build its ctypes structures.
 */
#ifndef MJHIP_H_
#define MJHIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MJH_ABI_VERSION 28

/* ---- dtype / flags ------------------------------------------------------------------- */
#define MJH_F64 0
#define MJH_F32 1

#define MJH_FLAG_FIXED_ITERATIONS 1 /* step(..., fixed_iterations=True), forward.py:463 */
#define MJH_FLAG_INV_DISCRETE 2     /* mjh_inverse: opt.enableflags & mjENBL_INVDISCRETE (discrete_acc, inverse.py:92-93) */

/* stage bits for mjh_forward(stages): run the pipeline up to and including the highest bit */
#define MJH_STAGE_KINEMATICS 0x001 /* smooth.kinematics + com_pos        smooth.py:34-288   */
#define MJH_STAGE_CRB 0x002        /* smooth.crb + factor_m              smooth.py:291-332  */
#define MJH_STAGE_COLLISION 0x004  /* collision_driver.collision         :800-875           */
#define MJH_STAGE_CONSTRAINT 0x008 /* constraint.make_constraint         :600-768           */
#define MJH_STAGE_VELOCITY 0x010   /* transmission, _velocity, passive, rne                  */
#define MJH_STAGE_ACTUATION 0x020  /* forward._actuation + _acceleration :102-228           */
#define MJH_STAGE_SOLVE 0x040      /* solver.solve                       solver.py:244-553  */
#define MJH_STAGE_ALL 0x07f

/* kernel ids: the kernels a call launches, as mjh_debug_phase_times() reports them and mjh_model_kernel_io() accounts for them */
#define MJH_KERNEL_KIN 0         /* kinematics + com_pos                                                              */
#define MJH_KERNEL_CRB 1         /* crb + factor_m                                                                    */
#define MJH_KERNEL_CON 2         /* collision + constraint rows                                                       */
#define MJH_KERNEL_VEL 3         /* transmission, velocity, passive, rne, actuation                                   */
#define MJH_KERNEL_SOL 4         /* solve + integrator                                                                */
#define MJH_KERNEL_VEL_OPT 5     /* MJH_KERNEL_VEL with fluid forces, gravity compensation, tendons or nv > 64         */
#define MJH_KERNEL_SOL_GEN 6     /* MJH_KERNEL_SOL with frictionloss / equality / dense limit rows                     */
#define MJH_KERNEL_CON_GEN 7     /* MJH_KERNEL_CON with those rows, max_contact_points or nv > 64                      */
#define MJH_KERNEL_CON_DIRECT 8  /* MJH_KERNEL_CON of small models: contact rows straight to the leaf                  */
#define MJH_KERNEL_SOL2 9        /* the solver phase as the register solver (two or four environments per wavefront)   */
#define MJH_KERNEL_CONVEX 10     /* convex narrow phase                                                               */
#define MJH_KERNEL_SENSOR 11     /* sensors                                                                           */
#define MJH_KERNEL_KV 12         /* kinematics + velocity as one kernel: then 0 and 3 do not appear                   */
#define MJH_KERNEL_KCV 13        /* kinematics + crb / factor + velocity as one kernel: then 12 and 1 do not appear    */
#define MJH_KERNEL_CS 14         /* constraint stage + register solver + integrator as one kernel                     */
/* 15 is unassigned */
#define MJH_KERNEL_PASS 16       /* the whole pass as one kernel (humanoid-class models)                              */
#define MJH_KERNEL_KCV2 17       /* MJH_KERNEL_KCV on two wavefronts per workgroup                                    */
#define MJH_KERNEL_STAGE 18      /* one RK4 stage of a small Newton model as one kernel                               */
#define MJH_KERNEL_TAIL 19       /* that kernel running the constraint phase + the solver's first tier only           */
#define MJH_KERNEL_INVERSE 20    /* the inverse-dynamics tail of mjh_inverse                                          */
#define MJH_KERNEL_RAY 21        /* the ray kernel of mjh_ray                                                         */
#define MJH_KERNEL_RENDER 22     /* the ray-cast renderer of mjh_render                                               */
#define MJH_KERNEL_JAC 23        /* mjh_support, MJH_SUPPORT_JAC: point Jacobians                                      */
#define MJH_KERNEL_APPLY_FT 24   /* mjh_support, MJH_SUPPORT_APPLY_FT: Cartesian force to generalized force            */
#define MJH_KERNEL_XFRC 25       /* mjh_support, MJH_SUPPORT_XFRC: xfrc_applied summed into a generalized force        */
#define MJH_KERNEL_MUL_M 26      /* mjh_support, MJH_SUPPORT_MUL_M: qM products                                       */
#define MJH_KERNEL_SOLVE_M 27    /* mjh_support, MJH_SUPPORT_SOLVE_M: solves with the factor qLD                       */
#define MJH_KERNEL_FD_PERTURB 28 /* mjh_fd_perturb: the perturbed input leaves of a chunk of finite-difference columns */
#define MJH_KERNEL_FD_DIFFERENCE 29 /* mjh_fd_difference: the columns of A, B, C, D from the stepped chunk            */
#define MJH_KERNEL_FD_VJP 30     /* mjh_fd_vjp: those columns contracted with a cotangent instead of stored            */
#define MJH_KERNEL_FD_TANGENT 31 /* mjh_fd_tangent: cotangents between qpos coordinates and the tangent space          */
#define MJH_KERNEL_POSTCON 32    /* mjh_postconstraint: cacc, cfrc_int, cfrc_ext, subtree_linvel, subtree_angmom       */
#define MJH_KERNEL_CONSENS 33    /* mjh_contact_sensors: contact forces, touch / framelinacc / frameangacc sensors     */
#define MJH_KERNEL_ENERGY 34     /* mjh_energy: potential / kinetic energy, joint / tendon limit and energy sensors     */
#define MJH_KERNEL_INTEGRATE 35  /* mjh_integrate: deriv_smooth_vel, the implicit (implicitfast) and Euler integrators   */
#define MJH_KERNEL_JACOBIAN_POINT 36       /* mjh_jacobian, matrix form (36 + op): MJH_JACOBIAN_POINT                   */
#define MJH_KERNEL_JACOBIAN_DOT 37         /* ... MJH_JACOBIAN_DOT: the time derivative of a point Jacobian              */
#define MJH_KERNEL_JACOBIAN_SUBTREE_COM 38 /* ... MJH_JACOBIAN_SUBTREE_COM: the Jacobian of a subtree's centre of mass  */
#define MJH_KERNEL_JACOBIAN_ANGMOM 39      /* ... MJH_JACOBIAN_ANGMOM: the angular-momentum matrix of a subtree         */
#define MJH_KERNEL_JACOBIAN_POINT_VEC 40   /* mjh_jacobian, product form (40 + op): the same four times a vector          */
#define MJH_KERNEL_JACOBIAN_DOT_VEC 41
#define MJH_KERNEL_JACOBIAN_SUBTREE_COM_VEC 42
#define MJH_KERNEL_JACOBIAN_ANGMOM_VEC 43
#define MJH_KERNEL_QUADRIC 44    /* plane-ellipsoid / plane-cylinder narrow phase (one lane per (environment, pair))   */
#define MJH_KERNEL_IFD_PERTURB 45 /* mjh_ifd_perturb: the perturbed input leaves of a chunk of inverse-dynamics columns */
#define MJH_KERNEL_IFD_DIFFERENCE 46 /* mjh_ifd_difference: the columns of DfDq, DfDv, DfDa (DsDq, DsDv, DsDa) from the chunk */
#define MJH_KERNEL_GEOM_DISTANCE 47 /* mjh_geom_distance: signed distance and nearest points of geom pairs (one lane per (pair, environment)) */
#define MJH_KERNEL_QPOS_ARITH 48 /* mjh_qpos_arith: qpos (+) dt qvel, (qpos2 (-) qpos1) / dt, quaternion normalisation (one lane per (environment, joint)) */
#define MJH_KERNEL_IK_SITE 49    /* mjh_ik_site_step: one iteration of site-pose inverse kinematics (one wavefront per environment) */
#define MJH_KERNEL_EFC_MUL_J 50  /* mjh_constraint_space (50 + op), MJH_EFC_MUL_J: efc_J products                        */
#define MJH_KERNEL_EFC_MUL_JT 51 /* ... MJH_EFC_MUL_JT: products with its transpose                                      */
#define MJH_KERNEL_EFC_UPDATE 52 /* ... MJH_EFC_UPDATE: jar, states, forces, cost and gradient of a qacc (one fused kernel) */
#define MJH_KERNEL_EFC_AR 53     /* ... MJH_EFC_AR: the Delassus matrix J M^-1 J^T + R and b                              */
#define MJH_KERNEL_PGS 54        /* mjh_pgs: projected Gauss-Seidel sweeps on the dual problem (one wavefront per environment) */
#define MJH_KERNEL_NOSLIP 55     /* mjh_noslip: no-slip sweeps on the friction dimensions, pyramidal pairs and elliptic QCQPs (one wavefront per environment) */
#define MJH_KERNEL_SOLVE 56      /* mjh_solve: the CG / Newton primal solver with its exact line search on a finished pass (one wavefront per environment) */
#define MJH_KERNEL_SMOOTH_COM_POS 57          /* mjh_smooth, MJH_SMOOTH_COM_POS: subtree_com, cinert, cdof (the ids are 57 + op)       */
#define MJH_KERNEL_SMOOTH_CRB 58              /* ... MJH_SMOOTH_CRB: crb and the dense qM                                              */
#define MJH_KERNEL_SMOOTH_TENDON_ARMATURE 59  /* ... MJH_SMOOTH_TENDON_ARMATURE: qM + ten_J^T diag(armature) ten_J                     */
#define MJH_KERNEL_SMOOTH_FACTOR_M 60         /* ... MJH_SMOOTH_FACTOR_M: qLD, the Cholesky factor of qM                               */
#define MJH_KERNEL_SMOOTH_COM_VEL 61          /* ... MJH_SMOOTH_COM_VEL: cvel, cdof_dot                                                */
#define MJH_KERNEL_SMOOTH_RNE 62              /* ... MJH_SMOOTH_RNE: qfrc_bias                                                         */
#define MJH_KERNEL_DYNAMICS_TENDON 63        /* mjh_dynamics, MJH_DYNAMICS_TENDON: ten_length, ten_J (the ids are 63 + op)            */
#define MJH_KERNEL_DYNAMICS_TRANSMISSION 64  /* ... MJH_DYNAMICS_TRANSMISSION: actuator_length, actuator_moment                       */
#define MJH_KERNEL_DYNAMICS_VELOCITY 65      /* ... MJH_DYNAMICS_VELOCITY: actuator_velocity, ten_velocity                            */
#define MJH_KERNEL_DYNAMICS_PASSIVE 66       /* ... MJH_DYNAMICS_PASSIVE: qfrc_passive, qfrc_gravcomp                                 */
#define MJH_KERNEL_DYNAMICS_ACTUATION 67     /* ... MJH_DYNAMICS_ACTUATION: act_dot, actuator_force, qfrc_actuator                    */
#define MJH_KERNEL_DYNAMICS_ACCELERATION 68  /* ... MJH_DYNAMICS_ACCELERATION: qfrc_smooth, qacc_smooth                               */

/* pair-function ids of the static collision table (collision_driver.py:106-125) */
#define MJH_FN_PLANE_SPHERE 0
#define MJH_FN_PLANE_CAPSULE 1
#define MJH_FN_SPHERE_SPHERE 2
#define MJH_FN_SPHERE_CAPSULE 3
#define MJH_FN_CAPSULE_CAPSULE 4
#define MJH_FN_PLANE_CONVEX 5
#define MJH_FN_SPHERE_CONVEX 6
#define MJH_FN_CAPSULE_CONVEX 7
#define MJH_FN_CONVEX_CONVEX 8
/* ids from MJH_FN_PLANE_CONVEX up are narrow-phased by kernels of their own between the kinematics and the constraint stage, which picks their
 * contacts up from the contact leaves (or, with max_contact_points, from the candidate arrays of the workspace): 5..8 by MJH_KERNEL_CONVEX, 9..10
 * by MJH_KERNEL_QUADRIC.  The reference has no cylinder / ellipsoid pair beyond these two outside its gradient-descent SDF functions. */
#define MJH_FN_PLANE_ELLIPSOID 9 /* collision_primitive.py:77-85, 1 contact   */
#define MJH_FN_PLANE_CYLINDER 10 /* collision_primitive.py:88-169, 3 contacts */
#define MJH_MAX_PAIR_CONTACTS 4

/* ---- model description (host arrays; copied into a device blob by mjh_model_create) ---- */

/* int32 scalars */
#define MJH_MODEL_INTS(X)                                                                        \
  X(nq) X(nv) X(nu) X(na) X(nbody) X(njnt) X(ngeom) X(nsite) X(ncam) X(nlight) X(nmocap)         \
  X(ne) X(nf) /* dof-frictionloss rows */ X(nft) /* tendon-frictionloss rows (dense; they follow the dof ones) */ X(nl) /* slide / hinge limit rows (single-column) */ X(nlb) /* ball-joint limit rows */ X(nlt) /* tendon limit rows */ X(ncon) X(ncand) /* candidate contacts the narrow phase computes: == ncon unless max_contact_points keeps the ncon closest (collision_driver.py:822-840) */ X(topk) /* 1: that selection is on; the con_* tables are then in candidate order, ncand long */ X(nefc) X(npair) X(nconvex) \
  X(ntendon) /* fixed tendons = length of the ten_length / ten_velocity leaves */ X(nwrapj) /* joint terms of all tendons (entries of ten_dof / ten_qposadr / ten_coef) */ \
  X(neq) /* equality constraints of the model = length of the eq_active leaf */ X(neqtab) /* entries of the eq_* tables (0 when equality rows are disabled) */ \
  X(nsensor) /* sensors the stepper computes (sns_* tables) */ X(nsensordata) /* length of the sensordata leaf */ \
  X(integrator) X(solver) X(cone) X(disableflags) X(iterations) X(ls_iterations)

/* double scalars */
#define MJH_MODEL_REALS(X)                                                                       \
  X(timestep) X(impratio) X(tolerance) X(ls_tolerance) X(meaninertia)                            \
  X(gravity_x) X(gravity_y) X(gravity_z)                                                         \
  X(density) X(viscosity) X(wind_x) X(wind_y) X(wind_z) /* fluid model of passive.py:31-78; all zero = no fluid forces */ \
  X(magnetic_x) X(magnetic_y) X(magnetic_z) /* opt.magnetic: magnetometer sensors (sensor.py:92-94) */

/* const int32_t* arrays (length in comment) */
#define MJH_MODEL_INT_ARRAYS(X)                                                                  \
  X(body_parentid)  /* nbody */                                                                  \
  X(body_rootid)    /* nbody */                                                                  \
  X(body_jntadr)    /* nbody */                                                                  \
  X(body_jntnum)    /* nbody */                                                                  \
  X(body_dofadr)    /* nbody */                                                                  \
  X(body_dofnum)    /* nbody */                                                                  \
  X(body_mocapid)   /* nbody */                                                                  \
  X(jnt_type)       /* njnt */                                                                   \
  X(jnt_qposadr)    /* njnt */                                                                   \
  X(jnt_dofadr)     /* njnt */                                                                   \
  X(jnt_bodyid)     /* njnt */                                                                   \
  X(jnt_actfrclimited) /* njnt */                                                                \
  X(jnt_actgravcomp) /* njnt: gravity compensation of the joint's dofs is applied as an actuator force (forward.py:206-207) */ \
  X(dof_bodyid)     /* nv */                                                                     \
  X(dof_jntid)      /* nv */                                                                     \
  X(dof_parentid)   /* nv */                                                                     \
  X(geom_type)      /* ngeom */                                                                  \
  X(geom_bodyid)    /* ngeom */                                                                  \
  X(geom_convexid)  /* ngeom: index into convex_* tables or -1 */                                \
  X(site_bodyid)    /* nsite */                                                                  \
  X(cam_bodyid)     /* ncam */                                                                   \
  X(cam_mode)       /* ncam */                                                                   \
  X(cam_targetbodyid) /* ncam */                                                                 \
  X(light_bodyid)   /* nlight */                                                                 \
  X(act_trntype)    /* nu */                                                                     \
  X(act_jnttype)    /* nu */                                                                     \
  X(act_dofadr)     /* nu */                                                                     \
  X(act_qposadr)    /* nu */                                                                     \
  X(act_gaintype)   /* nu */                                                                     \
  X(act_biastype)   /* nu */                                                                     \
  X(act_dyntype)    /* nu */                                                                     \
  X(act_ctrllimited)  /* nu */                                                                   \
  X(act_forcelimited) /* nu */                                                                   \
  X(act_actlimited)   /* nu */                                                                   \
  X(act_actadr)     /* nu */                                                                     \
  X(act_actnum)     /* nu */                                                                     \
  X(sns_type)       /* nsensor: mjtSensor of the sensors sensor.py evaluates (every type of its three stage functions; the others keep their slots: slot_sensor) */ \
  X(sns_adr)        /* nsensor: first slot in sensordata */                                      \
  X(sns_objid)      /* nsensor: id of the object -- site / body / geom / camera / tendon / actuator id; the qpos address (jointpos, ballquat) or dof address (jointvel, ballangvel, jointactuatorfrc) of a joint */ \
  X(sns_bodyid)     /* nsensor: body the object rides on (site sensors, frame sensors) */       \
  X(sns_rootid)     /* nsensor: root body of that body */                                        \
  X(sns_objtype)    /* nsensor: mjtObj of the object: 0 unknown, 1 body (inertial frame), 2 xbody, 5 geom, 6 site, 7 camera (frame sensors, sensor.py:62-74) */ \
  X(sns_reftype)    /* nsensor: mjtObj of the reference frame of a frame sensor (0 = none) */   \
  X(sns_refid)      /* nsensor: its id, -1 = none (the value is reported in the world frame) */ \
  X(sns_refbodyid)  /* nsensor: body of the reference object */                                  \
  X(sns_refrootid)  /* nsensor: root body of that body */                                        \
  X(sns_datatype)   /* nsensor: mjtDataType (0 real, 1 positive) for the cutoff rule */          \
  X(sns_rfadr)      /* nsensor+1: rangefinders, range into rf_geom; geoms in the reference's evaluation order */ \
  X(rf_geom)        /* geom ids a rangefinder ray is tested against (ray.py:292-325: site's own body excluded, invisible geoms dropped) */ \
  X(slot_sensor)    /* nsensordata: sns_* index that produces the slot, -1 = the slot keeps the caller's value */ \
  X(eq_kind)        /* neqtab: 0 connect (3 rows), 1 weld (6 rows), 2 joint coupling (1 row); reference ROW order = all connects, all welds, all joint couplings (constraint.py:651-656) */ \
  X(eq_id)          /* neqtab: index of the constraint in the model (eq_active / eq_data / eq_solref / eq_solimp) */ \
  X(eq_obj1)        /* neqtab: body ids (connect, weld) or joint id (joint coupling) */          \
  X(eq_obj2)        /* neqtab: second body / joint (-1 = none for a joint coupling) */           \
  X(eq_row)         /* neqtab: first efc row */                                                  \
  X(eq_jadr)        /* neqtab*4: joint couplings: dofadr1, dofadr2, qposadr1, qposadr2 (device.py:310-314; a missing second joint reads the LAST joint, as the reference's jnt_dofadr[-1] does) */ \
  X(fric_dof)       /* nf: dof of each dof-frictionloss row, reference row order (constraint.py:215-251) */ \
  X(topk_slot)      /* ncon (top-k only): final contact slot of the t-th closest candidate (the unstable argsort of the kept contacts' equal condims, collision_driver.py:828) */ \
  X(fric_tendon)    /* nft: tendon id of each tendon-frictionloss row (constraint.py:230-234) */ \
  X(ten_adr)        /* ntendon+1: CSR of the joint terms of each fixed tendon (smooth.py:470-497) */ \
  X(ten_dof)        /* nwrapj: dof of the term */                                                \
  X(ten_qposadr)    /* nwrapj: qpos address of the term */                                       \
  X(lim_tendon)     /* nlt: tendon id of each tendon limit row (constraint.py:375-405); these rows follow the slide / hinge ones */ \
  X(act_trnid)      /* nu: joint id, or tendon id for tendon transmissions (act_trntype 3) */    \
  X(lim_ball_jnt)   /* nlb: joint id of each ball-joint limit row (constraint.py:299-335); these rows precede the slide / hinge ones */ \
  X(lim_jnt)        /* nl: joint id of each slide/hinge limit row, reference row order */        \
  X(pair_fn)        /* npair: MJH_FN_* (0..10) */                                                \
  X(pair_geom1)     /* npair */                                                                  \
  X(pair_geom2)     /* npair */                                                                  \
  X(pair_ncon)      /* npair */                                                                  \
  X(pair_dst)       /* npair*MJH_MAX_PAIR_CONTACTS: contact slot of each contact of the pair */  \
  X(con_dim)        /* ncon */                                                                   \
  X(con_geom1)      /* ncon */                                                                   \
  X(con_geom2)      /* ncon */                                                                   \
  X(con_efc_address) /* ncon: cone-aware first row (constraint.py:636-646) */                    \
  X(convex_nvert)   /* nconvex */                                                                \
  X(convex_nface)   /* nconvex */                                                                \
  X(convex_nfv)     /* nconvex: vertices per (padded) face */                                    \
  X(convex_nedge)   /* nconvex */                                                                \
  X(convex_vertadr) /* nconvex: offset (in vec3) into convex_vert */                             \
  X(convex_faceadr) /* nconvex: offset (in ints) into convex_face */                             \
  X(convex_normadr) /* nconvex: offset (in vec3) into convex_facenormal */                       \
  X(convex_edgeadr) /* nconvex: offset (in int pairs) into convex_edge */                        \
  X(convex_face)    /* sum(nface*nfv): vertex ids */                                             \
  X(convex_edge)    /* sum(nedge)*2 */

/* const double* arrays */
#define MJH_MODEL_REAL_ARRAYS(X)                                                                 \
  X(qpos0)          /* nq */                                                                     \
  X(qpos_spring)    /* nq */                                                                     \
  X(body_pos)       /* nbody*3 */                                                                \
  X(body_quat)      /* nbody*4 */                                                                \
  X(body_ipos)      /* nbody*3 */                                                                \
  X(body_iquat)     /* nbody*4 */                                                                \
  X(body_mass)      /* nbody */                                                                  \
  X(body_inertia)   /* nbody*3 */                                                                \
  X(body_invweight0) /* nbody (translational component) */                                       \
  X(jnt_pos)        /* njnt*3 */                                                                 \
  X(jnt_axis)       /* njnt*3 */                                                                 \
  X(jnt_stiffness)  /* njnt */                                                                   \
  X(jnt_range)      /* njnt*2 */                                                                 \
  X(jnt_margin)     /* njnt */                                                                   \
  X(jnt_solref)     /* njnt*2 */                                                                 \
  X(jnt_solimp)     /* njnt*5 */                                                                 \
  X(jnt_actfrcrange) /* njnt*2 */                                                                \
  X(dof_armature)   /* nv */                                                                     \
  X(dof_damping)    /* nv */                                                                     \
  X(dof_invweight0) /* nv */                                                                     \
  X(sns_cutoff)     /* nsensor */                                                                \
  X(dof_frictionloss) /* nv */                                                                   \
  X(dof_solref)     /* nv*2 */                                                                   \
  X(dof_solimp)     /* nv*5 */                                                                   \
  X(ten_coef)       /* nwrapj: coefficient of the term */                                        \
  X(tendon_range)   /* ntendon*2 */                                                              \
  X(tendon_margin)  /* ntendon */                                                                \
  X(tendon_invweight0) /* ntendon */                                                             \
  X(tendon_solref_lim) /* ntendon*2 */                                                           \
  X(tendon_solimp_lim) /* ntendon*5 */                                                           \
  X(tendon_stiffness) /* ntendon */                                                              \
  X(tendon_damping) /* ntendon */                                                                \
  X(tendon_frictionloss) /* ntendon */ X(tendon_solref_fri) /* ntendon*2 */ X(tendon_solimp_fri) /* ntendon*5 */ \
  X(tendon_lengthspring) /* ntendon*2: the spring is slack between the two lengths (passive.py:121-127) */ \
  X(tendon_armature) /* ntendon: qM += J^T diag(armature) J (smooth.py:500-522) */ \
  X(body_gravcomp)  /* nbody: fraction of the body's weight compensated (passive.py:148-156); all zero = none */ \
  X(body_invweight0_rot) /* nbody (rotational component; weld rows 3..5, constraint.py:193-194) */         \
  X(eq_data)        /* neq*11 (MuJoCo layout: connect anchors; weld anchors, relpose, torquescale; joint polycoef) */ \
  X(eq_solref)      /* neq*2 */                                                                  \
  X(eq_solimp)      /* neq*5 */                                                                  \
  X(geom_pos)       /* ngeom*3 */                                                                \
  X(geom_quat)      /* ngeom*4 */                                                                \
  X(geom_size)      /* ngeom*3 */                                                                \
  X(site_pos)       /* nsite*3 */                                                                \
  X(site_quat)      /* nsite*4 */                                                                \
  X(cam_pos)        /* ncam*3 */                                                                 \
  X(cam_quat)       /* ncam*4 */                                                                 \
  X(cam_pos0)       /* ncam*3 */                                                                 \
  X(cam_mat0)       /* ncam*9 */                                                                 \
  X(light_pos)      /* nlight*3 */                                                               \
  X(light_dir)      /* nlight*3 */                                                               \
  X(act_gear)       /* nu*6 */                                                                   \
  X(act_gainprm)    /* nu*9 (muscle gains read all nine, support.py:246-272; fixed / affine the first three) */ \
  X(act_biasprm)    /* nu*9 */                                                                   \
  X(act_lengthrange) /* nu*2 (muscles) */                                                        \
  X(act_acc0)       /* nu (muscles: force = scale / acc0 when gainprm[2] < 0) */                  \
  X(act_dynprm)     /* nu*3 */                                                                   \
  X(act_ctrlrange)  /* nu*2 */                                                                   \
  X(act_forcerange) /* nu*2 */                                                                   \
  X(act_actrange)   /* nu*2 */                                                                   \
  X(con_includemargin)  /* ncon */                                                               \
  X(con_friction)       /* ncon*5 */                                                             \
  X(con_solref)         /* ncon*2 */                                                             \
  X(con_solreffriction) /* ncon*2 */                                                             \
  X(con_solimp)         /* ncon*5 */                                                             \
  X(convex_vert)        /* sum(nvert)*3 */                                                       \
  X(convex_facenormal)  /* sum(nface)*3 */

typedef struct mjhModelDesc {
  int32_t abi_version;
#define X(n) int32_t n;
  MJH_MODEL_INTS(X)
#undef X
#define X(n) double n;
  MJH_MODEL_REALS(X)
#undef X
#define X(n) const int32_t* n;
  MJH_MODEL_INT_ARRAYS(X)
#undef X
#define X(n) const double* n;
  MJH_MODEL_REAL_ARRAYS(X)
#undef X
#define X(n) int64_t len_##n;
  MJH_MODEL_INT_ARRAYS(X)
  MJH_MODEL_REAL_ARRAYS(X)
#undef X
} mjhModelDesc;

/* ---- Data leaves (reference _src/types.py:1091-1261, Contact :1036-1088) --------------- */

/* real leaves; per-env element count in the comment */
#define MJH_DATA_REALS(X)                                                                        \
  X(time)             /* 1 */                                                                    \
  X(qpos)             /* nq */                                                                   \
  X(qvel)             /* nv */                                                                   \
  X(act)              /* na */                                                                   \
  X(qacc_warmstart)   /* nv */                                                                   \
  X(ctrl)             /* nu */                                                                   \
  X(qfrc_applied)     /* nv */                                                                   \
  X(xfrc_applied)     /* nbody*6 */                                                              \
  X(mocap_pos)        /* nmocap*3 */                                                             \
  X(mocap_quat)       /* nmocap*4 */                                                             \
  X(qacc)             /* nv */                                                                   \
  X(act_dot)          /* na */                                                                   \
  X(xpos)             /* nbody*3 */                                                              \
  X(xquat)            /* nbody*4 */                                                              \
  X(xmat)             /* nbody*9 */                                                              \
  X(xipos)            /* nbody*3 */                                                              \
  X(ximat)            /* nbody*9 */                                                              \
  X(xanchor)          /* njnt*3 */                                                               \
  X(xaxis)            /* njnt*3 */                                                               \
  X(geom_xpos)        /* ngeom*3 */                                                              \
  X(geom_xmat)        /* ngeom*9 */                                                              \
  X(site_xpos)        /* nsite*3 */                                                              \
  X(site_xmat)        /* nsite*9 */                                                              \
  X(cam_xpos)         /* ncam*3 */                                                               \
  X(cam_xmat)         /* ncam*9 */                                                               \
  X(light_xpos)       /* nlight*3 */                                                             \
  X(light_xdir)       /* nlight*3 */                                                             \
  X(subtree_com)      /* nbody*3 */                                                              \
  X(cdof)             /* nv*6 */                                                                 \
  X(cinert)           /* nbody*10 */                                                             \
  X(crb)              /* nbody*10 */                                                             \
  X(ten_length)       /* ntendon */                                                              \
  X(ten_J)            /* ntendon*nv (dense; constant for fixed tendons) */                       \
  X(ten_velocity)     /* ntendon */                                                              \
  X(actuator_length)  /* nu */                                                                   \
  X(actuator_moment)  /* nu*nv */                                                                \
  X(qM)               /* nv*nv (dense) */                                                        \
  X(qLD)              /* nv*nv (dense Cholesky L) */                                             \
  X(contact_dist)           /* ncon */                                                           \
  X(contact_pos)            /* ncon*3 */                                                         \
  X(contact_frame)          /* ncon*9 */                                                         \
  X(contact_includemargin)  /* ncon */                                                           \
  X(contact_friction)       /* ncon*5 */                                                         \
  X(contact_solref)         /* ncon*2 */                                                         \
  X(contact_solreffriction) /* ncon*2 */                                                         \
  X(contact_solimp)         /* ncon*5 */                                                         \
  X(sensordata)       /* nsensordata (sensor.py:56-440; written by forward passes that include the solver stage) */ \
  X(efc_J)            /* nefc*nv */                                                              \
  X(efc_frictionloss) /* nefc */                                                                 \
  X(efc_D)            /* nefc */                                                                 \
  X(efc_aref)         /* nefc */                                                                 \
  X(efc_force)        /* nefc */                                                                 \
  X(actuator_velocity) /* nu */                                                                  \
  X(cvel)             /* nbody*6 */                                                              \
  X(cdof_dot)         /* nv*6 */                                                                 \
  X(qfrc_bias)        /* nv */                                                                   \
  X(qfrc_passive)     /* nv */                                                                   \
  X(qfrc_gravcomp)    /* nv (written only by models with gravity compensation; otherwise the caller's value stays, passive.py:190-194) */ \
  X(actuator_force)   /* nu */                                                                   \
  X(qfrc_actuator)    /* nv */                                                                   \
  X(qfrc_smooth)      /* nv */                                                                   \
  X(qacc_smooth)      /* nv */                                                                   \
  X(qfrc_constraint)  /* nv */

/* Input-only real leaves that NO stage of the reference writes -- they hold what make_data put there (zeros) or what the caller did -- but its sensor functions
 * read: cacc (accelerometer, sensor.py:383-392), cfrc_int (force / torque, :399-416), subtree_linvel / subtree_angmom (:261-266).  They trail the struct, outside
 * the leaf lists above (no kernel of a pass writes them, the goldens' key sets do not change); NULL = zeros.  [B, nbody*6], [B, nbody*6], [B, nbody*3], [B, nbody*3].
 * mjh_postconstraint computes them from a finished pass, into buffers of the caller's. */
#define MJH_DATA_EXTRA_IN(X) X(cacc) X(cfrc_int) X(subtree_linvel) X(subtree_angmom)

#define MJH_DATA_I32(X) X(contact_dim) /* ncon */ X(eq_active) /* neq: input, enable / disable each equality constraint (types.py:1103) */

#define MJH_DATA_I64(X)                                                                          \
  X(contact_geom1)       /* ncon */                                                              \
  X(contact_geom2)       /* ncon */                                                              \
  X(contact_geom)        /* ncon*2 */                                                            \
  X(contact_efc_address) /* ncon */

typedef struct mjhData {
#define X(n) void* n;
  MJH_DATA_REALS(X)
#undef X
#define X(n) int32_t* n;
  MJH_DATA_I32(X)
#undef X
#define X(n) int64_t* n;
  MJH_DATA_I64(X)
#undef X
#define X(n) const void* n;
  MJH_DATA_EXTRA_IN(X)
#undef X
} mjhData;

/* ---- entry points ------------------------------------------------------------------------ */

typedef struct mjhModel mjhModel; /* opaque: device-resident constant blob + launch geometry */

/* Builds the device blob for one dtype.  replaces Model.to(device) (types.py:991-1013). */
int mjh_model_create(const mjhModelDesc* desc, int dtype, mjhModel** out);
void mjh_model_destroy(mjhModel* m);

/* forward dynamics for B environments (forward.py:373-401), optionally only a prefix of stages.
 * `work`: as for mjh_step; a forward pass needs it only for models whose max_contact_points selection runs over box / mesh candidates
 * (the convex narrow phase hands its candidate contacts to the constraint phase there), NULL otherwise. */
int mjh_forward(const mjhModel* m, const mjhData* in, mjhData* out, void* work, int64_t B, int stages, int flags,
                void* hip_stream);

/* one simulation step for B environments (forward.py:463-496): _check_state, forward, Euler/RK4.
 * `work`: caller-owned device scratch of mjh_model_work_bytes(m) * B bytes (contents undefined, may be
 * NULL when that is 0).  RK4 keeps its stage Data (stages 1..3 of forward.py:356-367) and the running
 * sums there; max_contact_points over box / mesh pairs keeps the candidate contacts of the convex narrow phase there
 * (collision_driver.py:822-840: every candidate is computed, the closest are kept); other Euler models need none. */
int mjh_step(const mjhModel* m, const mjhData* in, mjhData* out, void* work, int64_t B, int flags, void* hip_stream);
int64_t mjh_model_work_bytes(const mjhModel* m);

/* inverse dynamics for B environments (inverse.py:86-102): the forward pass up to and including the velocity stage (stages 0x1F of
 * mjh_forward: _position + _velocity), then -- with the caller's in.qacc -- discrete_acc when MJH_FLAG_INV_DISCRETE is set (Euler with eulerdamp
 * and some dof damping: qacc <- solve_m(M qacc + h * dof_damping o qacc); RK4 returns an error), inv_constraint and
 *   qfrc_inverse = qfrc_bias + M qacc - qfrc_passive - qfrc_constraint,
 * then the sensors when the model has some and out.sensordata is given.  Writes the leaves of those stages, efc_force (nefc > 0), qfrc_constraint
 * (zeros when nefc == 0) and `qfrc_inverse` ([B, nv], a pointer of its own: qfrc_inverse is not one of the mjhData leaves).  It does NOT write
 * actuator_force, qfrc_actuator, qfrc_smooth, qacc_smooth, qacc, act_dot or qacc_warmstart (NULL in `out` is fine); sensors that read
 * actuator_force / qfrc_actuator read the caller's (in).  `work`: as for mjh_forward. */
int mjh_inverse(const mjhModel* m, const mjhData* in, mjhData* out, void* qfrc_inverse, void* work, int64_t B, int flags, void* hip_stream);

/* the geoms one mjh_ray call tests, built by the caller from the model and its filters (ray.py:400-415: flg_static, bodyexclude, geomgroup, alpha).
 * Every pointer is device memory.  `cand` holds ncand rows of four int32: geom id, geom type (mjtGeom: plane 0, sphere 2, capsule 3, ellipsoid 4,
 * cylinder 5, box 6, mesh 7), first and end triangle in `tri` (meshes; anything for the primitives).  The rows are in tie-break order -- the reference's
 * type-major order (plane, sphere, capsule, ellipsoid, cylinder, box, mesh), ascending geom id within a type -- and the first minimum wins.
 * `tri`: [ntri][9] reals of the call's dtype, a triangle's three vertices in the geom frame.  `geom_size`: [ngeom][3] reals, the sizes to use (read
 * on the device by every call, so value edits of the Model need no new table).  The library does not validate the rows: ids must be < ngeom and
 * triangle ranges inside `tri`. */
typedef struct mjhRayCands {
  int64_t ncand;
  const int32_t* cand;
  const void* tri;
  const void* geom_size;
} mjhRayCands;

/* batched ray casting (ray.py:375-452): R rays in each of B environments against the candidate geoms.  geom_xpos [B, ngeom, 3] / geom_xmat
 * [B, ngeom, 9] are the environments' geom frames (a forward pass's leaves).  Ray r of environment e starts at pnt[e * pnt_env + r * pnt_ray + k]
 * and runs along vec[e * vec_env + r * vec_ray + k], k = 0..2, in element strides (0: shared); vec is not normalised.  Writes
 * dist [B * R] (the ray parameter of the nearest hit, -1 for none; the model's dtype) and geomid [B * R] (int64, -1 for none), environment-major.
 * Returns 0 or a negative code; B == 0 is a no-op. */
int mjh_ray(const mjhModel* m, const void* geom_xpos, const void* geom_xmat, const void* pnt, int64_t pnt_env, int64_t pnt_ray, const void* vec,
            int64_t vec_env, int64_t vec_ray, int64_t B, int64_t R, const mjhRayCands* cands, void* dist, int64_t* geomid, void* hip_stream);

/* signed distance and nearest points of geom pairs on a finished pass (MuJoCo's mj_geomDistance; definitions: csrc/mjh_geomdist.h).  geom_xpos [B, ngeom, 3] /
 * geom_xmat [B, ngeom, 9]: the environments' geom frames; geom_size [ngeom][3]: the sizes to use (read on the device by every call, so value edits of the Model
 * need no new table); reals are of the model's dtype.  `pairs`: npair rows of four int32 on the device, shared by every environment: geom1, geom2 and their types
 * (mjtGeom: plane 0, sphere 2, capsule 3, ellipsoid 4, cylinder 5, box 6), written by the caller as the ray candidate table is.  Supported: sphere / capsule / box with each
 * other, a plane with any of those five; the library does not validate the rows (a geom id outside the model or another type pair gives NaN).  Writes
 * dist [B, npair] and fromto [B, npair, 6] (the nearest point on geom1, then on geom2: to - from = dist * n, n the unit vector from geom1 towards geom2, dist < 0 when
 * they overlap); where dist > distmax (>= 0), dist = distmax and fromto = 0.  Returns 0 or a negative code; B == 0 or npair == 0 is a no-op. */
int mjh_geom_distance(const mjhModel* m, const void* geom_xpos, const void* geom_xmat, const void* geom_size, const int32_t* pairs, int64_t npair, double distmax,
                      void* dist, void* fromto, int64_t B, void* hip_stream);

/* configuration arithmetic on plain rows (definitions: csrc/mjh_qpos.h); joint types and addresses are the model's, reals of the model's dtype, every pointer device
 * memory.  op MJH_QPOS_INTEGRATE: out [B, nq] = a (+) dt b, a = qpos [B, nq], b = qvel [B, nv] (the step's integrate_pos: quaternions renormalised).
 * MJH_QPOS_DIFFERENTIATE: out [B, nv] = (b (-) a) / dt, a = qpos1, b = qpos2 [B, nq] (MuJoCo's mj_differentiatePos; dt != 0).  MJH_QPOS_NORMALIZE: out [B, nq] = a with
 * every ball / free quaternion divided by its norm, (1, 0, 0, 0) where the norm is below 1e-15; b and dt are ignored.  out may not overlap a or b.  Returns 0 or
 * a negative code; B == 0 is a no-op. */
#define MJH_QPOS_INTEGRATE 0
#define MJH_QPOS_DIFFERENTIATE 1
#define MJH_QPOS_NORMALIZE 2
int mjh_qpos_arith(const mjhModel* m, int op, const void* a, const void* b, double dt, void* out, int64_t B, void* hip_stream);

/* one damped-least-squares iteration of site-pose inverse kinematics for every environment that is not done (definitions: csrc/mjh_ik.h).  cdof [B, nv, 6],
 * subtree_com [B, nbody, 3], site_xpos [B, nsite, 3], site_xmat [B, nsite, 9]: the kinematics pass at the current qpos.  `site`: the site, `body` its body (the
 * caller's site_bodyid[site]).  target_pos (3 reals per environment) / target_quat (4, unit): NULL = absent, not both; pos_stride / quat_stride: elements between
 * the targets of consecutive environments, 0 for one shared target.  dof_sel [nv] int32 on the device: non-zero = the dof takes part.  params: tol, damping (> 0),
 * max_update_norm, rot_weight.  In / out: qpos [B, nq]; err_norm [B] reals; steps [B] int32; done [B] bytes (non-zero: the environment is skipped and none of its
 * entries is touched).  Per environment: err_norm is stored; err_norm < tol sets done; otherwise, unless `last` is non-zero, qpos is advanced by the update and
 * steps incremented.  Returns 0 or a negative code; B == 0 is a no-op. */
int mjh_ik_site_step(const mjhModel* m, const void* cdof, const void* subtree_com, const void* site_xpos, const void* site_xmat, int site, int body,
                     const void* target_pos, int64_t pos_stride, const void* target_quat, int64_t quat_stride, const int32_t* dof_sel, const double* params,
                     int last, void* qpos, void* err_norm, int32_t* steps, unsigned char* done, int64_t B, void* hip_stream);

/* the scene one mjh_render call draws, built by the caller from the model (render.py:33-114 precompute_render_data).  Every pointer is device memory.
 * `cand`, `tri`, `geom_size`: as mjhRayCands, the VISIBLE geoms ((matid != -1 or rgba alpha != 0) and (matid == -1 or the material's alpha != 0)) in the
 * reference's type-major order; the `nprim` primitive rows come first, the mesh rows (ascending geom id) after them.  Shadow rays test the primitive
 * rows only, as the reference does.  `geom_rgba`: [ngeom][4] reals of the call's dtype holding float32 values (MuJoCo's type); `geom_matid`: [ngeom]
 * int32, -1 for none; `mat_rgba`: [nmat][4] float32.  A hit geom's colour is mat_rgba[matid] when matid >= 0, else geom_rgba (first three channels).
 * `light`: [nlight][16] reals of the call's dtype, one row per light: diffuse (3), ambient (3), specular (3), attenuation (3), cos(cutoff) of a
 * spotlight (cutoff < 180 degrees; 2 for none), directional (1 / 0), castshadow (1 / 0), unused.  nlight must equal the model's. */
typedef struct mjhRenderScene {
  int64_t ncand;
  int64_t nprim;
  const int32_t* cand;
  const void* tri;
  const void* geom_size;
  const void* geom_rgba;
  const int32_t* geom_matid;
  const float* mat_rgba;
  int64_t nlight;
  const void* light;
} mjhRenderScene;

/* one mjh_render call's settings.  camera: 0 <= camera < ncam; width, height, ssaa >= 1 (the output image is width x height, rendered at ssaa times
 * that and averaged); half_w / half_h: the tangents of the half view angles (render.py:196-198, in the call's dtype); shading: Lambert + Phong per
 * light when the model has lights (else the flat colour); shadows: shadow rays for the castshadow lights; background: the colour of a miss (float32
 * values); fog: linear fog on hit samples, factor clamp((depth - fog_start) / fog_range, 0, 1) toward fog_color; rgb_f32: write rgb as float32 (else
 * in the call's dtype); u8: write rgb as uint8, (rgb * 255) clamped to [0, 255] and truncated, from the rgb rgb_f32 selects. */
typedef struct mjhRenderParams {
  int32_t camera, width, height, ssaa;
  int32_t shading, shadows, fog, rgb_f32, u8, reserved;
  double half_w, half_h;
  double background[3];
  double fog_color[3];
  double fog_start, fog_range;
} mjhRenderParams;

/* batched ray-cast rendering (render.py:719-907): one image per environment from camera `camera`.  geom_xpos [B, ngeom, 3], geom_xmat [B, ngeom, 9],
 * cam_xpos [B, ncam, 3], cam_xmat [B, ncam, 9], light_xpos / light_xdir [B, nlight, 3]: the environments' poses (a forward pass's leaves).  Writes
 * rgb [B, height, width, 3] (the dtype params->rgb_f32 / u8 select), depth [B, height, width] (the model's dtype; the ray distance of the nearest hit,
 * -1 for a miss, averaged over the super-samples), seg [B, height, width] (int64 geom id of the centre super-sample, -1 for a miss).  Row 0 is the top of
 * the image.  Returns 0 or a negative code; B == 0 is a no-op. */
int mjh_render(const mjhModel* m, const void* geom_xpos, const void* geom_xmat, const void* cam_xpos, const void* cam_xmat, const void* light_xpos,
               const void* light_xdir, int64_t B, const mjhRenderScene* scene, const mjhRenderParams* params, void* rgb, void* depth, int64_t* seg,
               void* hip_stream);

/* mjh_support operations (mjhSupportArgs.op); op + MJH_KERNEL_JAC is the kernel id the timing aid reports */
#define MJH_SUPPORT_JAC 0
#define MJH_SUPPORT_APPLY_FT 1
#define MJH_SUPPORT_XFRC 2
#define MJH_SUPPORT_MUL_M 3
#define MJH_SUPPORT_SOLVE_M 4

/* one mjh_support call.  Every pointer is device memory holding reals of the model's dtype, batch-major over B environments; the leaves are a finished
 * forward pass's: cdof [B, nv, 6], subtree_com / xipos [B, nbody, 3], xfrc_applied [B, nbody, 6], qM / qLD [B, nv, nv].  Queries are addressed in element
 * strides (0: shared by every environment or query): query p of environment e reads point[e * point_env + p * point_q + k], k = 0..2, and likewise force /
 * torque; vector j of environment e reads vec[e * vec_env + j * vec_k + i], i = 0..nv-1.  body_id: P body ids in [0, nbody) (body_stride 1) or one id
 * for every query (0); the library does not validate them.  Per op, what is read and written (outputs environment-major, contiguous):
 *   JAC       cdof, subtree_com, point, body_id  -> out0 = jacp, out1 = jacr [B, P, nv, 3]   (support.py:138-153)
 *   APPLY_FT  the same, force, torque            -> out0 = jacp force + jacr torque [B, P, nv] (J is not formed)   (support.py:169-181)
 *   XFRC      cdof, subtree_com, xipos, xfrc_applied -> out0 [B, nv]: apply_ft of every body's xfrc_applied at its xipos, summed in body order (:184-194)
 *   MUL_M     qM, vec                            -> out0 [B, K, nv] = qM vec_j                  (smooth.py:370-374)
 *   SOLVE_M   qLD (lower triangle), vec          -> out0 [B, K, nv] = (L L^T)^-1 vec_j          (smooth.py:335-338, math.py:132-168)
 * P (JAC, APPLY_FT) and K (MUL_M, SOLVE_M) are >= 1; P * nv * 3 and K * nv must stay below 2^30. */
typedef struct mjhSupportArgs {
  int32_t op;
  int32_t P, K, reserved;
  int64_t B;
  const void* cdof;
  const void* subtree_com;
  const void* xipos;
  const void* xfrc_applied;
  const void* qM;
  const void* qLD;
  const int32_t* body_id;
  int64_t body_stride;
  const void* point;
  int64_t point_env, point_q;
  const void* force;
  int64_t force_env, force_q;
  const void* torque;
  int64_t torque_env, torque_q;
  const void* vec;
  int64_t vec_env, vec_k;
  void* out0;
  void* out1;
} mjhSupportArgs;

/* the support functions on a finished forward pass (see mjhSupportArgs).  Runs on hip_stream without host synchronisation.  Returns 0 or a negative
 * code; B == 0 is a no-op. */
int mjh_support(const mjhModel* m, const mjhSupportArgs* args, void* hip_stream);

/* mjh_postconstraint flags: what one launch computes */
#define MJH_POSTCON_RNE 1     /* cacc, cfrc_int, cfrc_ext (MuJoCo's mj_rnePostConstraint)                                        */
#define MJH_POSTCON_SUBTREE 2 /* subtree_linvel, subtree_angmom (mj_subtreeVel)                                                  */
#define MJH_POSTCON_SENSORS 4 /* ... and the sensordata slots that read those leaves; needs both bits above                     */

/* one mjh_postconstraint call.  Every pointer is device memory, batch-major over B environments; reals are of the model's dtype.  The inputs are the leaves of a
 * finished forward pass: qvel (the velocity the pass ran on) / qacc [B, nv], cdof / cdof_dot [B, nv, 6], cvel / xfrc_applied [B, nbody, 6], cinert [B, nbody, 10],
 * xipos / subtree_com [B, nbody, 3], ximat [B, nbody, 9], efc_force [B, nefc], contact_pos [B, ncon, 3], contact_frame [B, ncon, 9], contact_friction [B, ncon, 5],
 * contact_dim [B, ncon] (int32), contact_geom [B, ncon, 2] / contact_efc_address [B, ncon] (int64), site_xpos [B, nsite, 3], site_xmat [B, nsite, 9], sensordata_in
 * [B, nsensordata]; body_subtreemass [nbody] is the model's.  RNE reads qvel .. cinert, xipos, subtree_com, xfrc_applied, efc_force (nefc > 0) and the contact leaves
 * (ncon > 0) and writes cacc, cfrc_int, cfrc_ext [B, nbody, 6]; SUBTREE reads cvel, xipos, ximat, subtree_com, body_subtreemass and writes subtree_linvel,
 * subtree_angmom [B, nbody, 3]; SENSORS also reads site_xpos / site_xmat and sensordata_in and writes sensordata [B, nsensordata]: the slots of accelerometer, force,
 * torque, subtreelinvel and subtreeangmom sensors from the fresh leaves, every other slot copied.  Spatial vectors are [rotational, translational] in the world frame
 * about subtree_com[body_rootid[b]]; cfrc_ext holds xfrc_applied and the contact forces only (equality, limit and frictionloss forces stay joint-space).  A contact slot
 * whose geom ids are not in [0, ngeom), or whose rows do not lie inside efc_force, is skipped.  No output may alias an input. */
typedef struct mjhPostconArgs {
  int32_t flags, reserved;
  int64_t B;
  const void *qvel, *qacc, *cdof, *cdof_dot, *cvel, *cinert, *xipos, *ximat, *subtree_com, *xfrc_applied, *efc_force;
  const void *contact_pos, *contact_frame, *contact_friction;
  const int32_t* contact_dim;
  const int64_t *contact_geom, *contact_efc_address;
  const void *site_xpos, *site_xmat, *sensordata_in;
  const void* body_subtreemass;
  void *cacc, *cfrc_int, *cfrc_ext, *subtree_linvel, *subtree_angmom, *sensordata;
} mjhPostconArgs;

/* body accelerations and forces of a finished forward pass (see mjhPostconArgs) as ONE launch.  Runs on hip_stream without host synchronisation.  Returns 0 or a
 * negative code (a model whose bodies and contacts do not fit the LDS of a workgroup is refused); B == 0 is a no-op. */
int mjh_postconstraint(const mjhModel* m, const mjhPostconArgs* args, void* hip_stream);

/* mjh_contact_sensors flags: what one launch computes */
#define MJH_CONSENS_FORCES 1  /* the force of every contact slot, [B, ncon, 6] (MuJoCo's mj_contactForce)                          */
#define MJH_CONSENS_SENSORS 2 /* the sensordata slots of the touch, framelinacc and frameangacc sensors listed in sns                */
#define MJH_CONSENS_WORLD 4   /* with FORCES: rows in the world frame, [frame^T w[0:3], frame^T w[3:6]], instead of the contact frame */

/* one mjh_contact_sensors call.  Every pointer is device memory; the leaves are batch-major over B environments, reals are of the model's dtype.  FORCES reads
 * efc_force [B, nefc], contact_pos [B, ncon, 3], contact_frame [B, ncon, 9], contact_friction [B, ncon, 5], contact_dim [B, ncon] (int32), contact_geom [B, ncon, 2] /
 * contact_efc_address [B, ncon] (int64) and writes force [B, ncon, 6]: per slot [force(3), torque(3)] in the contact frame, decoded from efc_force as mjh_postconstraint
 * decodes it; a slot whose geom ids are not in [0, ngeom), or whose rows do not lie inside efc_force, gives zeros.  SENSORS evaluates the nsens sensors of sns
 * ([nsens, 8] int32: sensor type (0 touch, 33 framelinacc, 34 frameangacc), sensordata address, object id, leaf kind of the object's point (0 xipos, 1 xpos, 2 geom_xpos,
 * 3 site_xpos, 4 cam_xpos), the body the object rides on, that body's root, datatype, the site's geom type for touch) with sns_cutoff [nsens] (reals) and writes ONLY their
 * slots of sensordata [B, nsensordata]: touch reads the contact leaves above, site_xpos [B, nsite, 3], site_xmat [B, nsite, 9] and site_size [nsite, 3] (the caller's
 * Model); the frame sensors read cvel / cacc [B, nbody, 6] (cacc: mjh_postconstraint's), subtree_com [B, nbody, 3] and the leaf of their kind (xipos, xpos [B, nbody, 3],
 * geom_xpos [B, ngeom, 3], site_xpos, cam_xpos [B, ncam, 3]).  The definitions are in csrc/mjh_contact_sensors.h.  sns rows must address this model (the kernel does not
 * check them).  No output may alias an input. */
typedef struct mjhContactSensorArgs {
  int32_t flags, nsens;
  int64_t B;
  const void *efc_force, *contact_pos, *contact_frame, *contact_friction;
  const int32_t* contact_dim;
  const int64_t *contact_geom, *contact_efc_address;
  const void *site_xpos, *site_xmat, *cvel, *cacc, *subtree_com, *xipos, *xpos, *geom_xpos, *cam_xpos;
  const void* site_size;
  const int32_t* sns;
  const void* sns_cutoff;
  void *force, *sensordata;
} mjhContactSensorArgs;

/* contact forces and / or the touch, framelinacc and frameangacc sensors of a finished forward pass (see mjhContactSensorArgs) as ONE launch.  Runs on hip_stream
 * without host synchronisation.  Returns 0 or a negative code (a model whose contacts do not fit the LDS of a workgroup is refused); B == 0 is a no-op. */
int mjh_contact_sensors(const mjhModel* m, const mjhContactSensorArgs* args, void* hip_stream);

/* mjh_energy flags: what one launch computes */
#define MJH_ENERGY_POS 1     /* the potential energy, energy[:, 0] (MuJoCo's mj_energyPos)                                                   */
#define MJH_ENERGY_VEL 2     /* the kinetic energy, energy[:, 1] (mj_energyVel)                                                             */
#define MJH_ENERGY_SENSORS 4 /* the sensordata slots of the joint / tendon limit and energy sensors listed in sns                            */

/* one mjh_energy call.  Every pointer is device memory; the leaves are batch-major over B environments, reals are of the model's dtype.  The MODEL VALUES are
 * arguments of the call (the caller's Model, not the blob): gravity [3], body_mass [nbody], jnt_stiffness [njnt], qpos_spring [nq], jnt_range [njnt, 2],
 * jnt_margin [njnt], tendon_stiffness [ntendon], tendon_lengthspring [ntendon, 2], tendon_range [ntendon, 2], tendon_margin [ntendon], sns_cutoff [nsens].
 * POS reads xipos [B, nbody, 3], qpos [B, nq] and ten_length [B, ntendon] -- the state the pass ran on -- and writes energy[:, 0]; VEL reads qvel [B, nv] and the
 * pass's dense qM [B, nv, nv] and writes energy[:, 1] = 1/2 qvel^T (qM qvel); energy is [B, 2] and may be NULL in a call for the sensors.  SENSORS evaluates the
 * nsens sensors of sns -- nsens is the size of the model's table in EVERY call, also one without SENSORS: it enters the lanes per environment, so that the energies of
 * the two kinds of call are the same bits -- ([nsens, 6] int32: sensor type (20 .. 25 jointlimitpos / vel / frc, tendonlimitpos / vel / frc, 43 e_potential, 44 e_kinetic), sensordata
 * address, object id, the row of the object's limit in efc_J / efc_force or -1, datatype, the joint's type) and writes ONLY their slots of sensordata
 * [B, nsensordata]; it reads qpos, qvel, ten_length, efc_J [B, nefc, nv] and efc_force [B, nefc]; an e_potential / e_kinetic row needs POS / VEL in the same call
 * (0 without).  The definitions are in csrc/mjh_energy.h.  sns rows must address this model (the kernel does not check them).  No output may alias an input. */
typedef struct mjhEnergyArgs {
  int32_t flags, nsens;
  int64_t B;
  const void *qpos, *qvel, *xipos, *ten_length, *qM, *efc_J, *efc_force;
  const void *gravity, *body_mass, *jnt_stiffness, *qpos_spring, *jnt_range, *jnt_margin, *tendon_stiffness, *tendon_lengthspring, *tendon_range, *tendon_margin;
  const int32_t* sns;
  const void* sns_cutoff;
  void *energy, *sensordata;
} mjhEnergyArgs;

/* the energies and / or the joint / tendon limit and energy sensors of a finished forward pass (see mjhEnergyArgs) as ONE launch.  Runs on hip_stream without host
 * synchronisation.  Returns 0 or a negative code; B == 0 is a no-op. */
int mjh_energy(const mjhModel* m, const mjhEnergyArgs* args, void* hip_stream);

/* mjh_integrate flags: what one launch computes */
#define MJH_INTEGRATE_QDERIV 1        /* build qDeriv = d(qfrc_smooth) / d(qvel): actuators, dof damping, tendon damping (derivative.py:22-68)        */
#define MJH_INTEGRATE_IMPLICIT 2      /* with QDERIV: qacc = chol_solve(qM - h qDeriv, qfrc_smooth + qfrc_constraint) (forward.py:404-416)            */
#define MJH_INTEGRATE_EULER 4         /* qacc = chol_solve(qM + h diag(dof_damping), qfrc_smooth + qfrc_constraint) (forward.py:313-328)              */
#define MJH_INTEGRATE_STATE 8         /* advance: qpos_out, qvel_out, act_out, time_out (forward.py:255-310), with the qacc above or else the qacc leaf */
#define MJH_INTEGRATE_WRITE_QDERIV 16 /* with QDERIV: qderiv_out [B, nv, nv], the full symmetric matrix                                               */
#define MJH_INTEGRATE_WRITE_QACC 32   /* qacc_out [B, nv]: the acceleration the state is advanced with                                                */

/* one mjh_integrate call.  Every pointer is device memory; the leaves are batch-major over B environments, reals are of the model's dtype.  The MODEL VALUES are
 * arguments of the call (the caller's Model, not the blob): dof_damping [nv], tendon_damping [ntendon], gainprm [nu, gain_stride], biasprm [nu, bias_stride] (entry 2 of a
 * row is read), dynprm [nu, dyn_stride] (entry 0), actrange [nu, 2], the step h and the disable flags (ACTUATION 1 << 11, DAMPER 1 << 6 are read).  The structure (gain /
 * bias / dyn types, actadr, actlimited, jnt_type / qposadr / dofadr) is the compiled model's.  QDERIV reads ctrl [B, nu], act [B, na], actuator_moment [B, nu, nv], ten_J
 * [B, ntendon, nv]; IMPLICIT / EULER read qM [B, nv, nv] (its lower triangle), qfrc_smooth and qfrc_constraint [B, nv]; a call with neither reads qacc [B, nv]; STATE reads
 * qpos [B, nq], qvel [B, nv], act, act_dot [B, na], time [B].  The definitions, the factorisation rule (the reference's math.small_cholesky) and the order of every sum
 * are in csrc/mjh_integrate.h.  No output may alias an input. */
typedef struct mjhIntegrateArgs {
  int32_t flags, disableflags;
  int64_t B;
  double h;
  int32_t gain_stride, bias_stride, dyn_stride, reserved;
  const void *qpos, *qvel, *act, *act_dot, *time, *ctrl, *qacc, *qM, *qfrc_smooth, *qfrc_constraint, *actuator_moment, *ten_J;
  const void *dof_damping, *tendon_damping, *gainprm, *biasprm, *dynprm, *actrange;
  void *qpos_out, *qvel_out, *act_out, *time_out, *qderiv_out, *qacc_out;
} mjhIntegrateArgs;

/* deriv_smooth_vel and / or one implicit or Euler integration step on a finished forward pass (see mjhIntegrateArgs) as ONE launch.  Runs on hip_stream without host
 * synchronisation.  Returns 0 or a negative code (a model whose matrix does not fit the LDS of a workgroup is refused); B == 0 is a no-op. */
int mjh_integrate(const mjhModel* m, const mjhIntegrateArgs* args, void* hip_stream);

/* the launch plan mjh_integrate uses for a model of nv dofs, nu actuators and ntendon tendons in reals of real_bytes (4 / 8) bytes, a host computation (no device is
 * touched): out = {lanes per environment, environments per workgroup, rows per LDS chunk, reals of LDS per environment}.  Returns 0, -12 when one environment does not
 * fit a workgroup's LDS (mjh_integrate refuses such a model), -22 for a bad argument. */
int mjh_integrate_plan(int nv, int nu, int ntendon, int real_bytes, int* lanes_envs_chunk_lds);

/* mjh_smooth operations (mjhSmoothArgs.op); MJH_KERNEL_SMOOTH_COM_POS + op is the kernel id the timing aid reports */
#define MJH_SMOOTH_COM_POS 0
#define MJH_SMOOTH_CRB 1
#define MJH_SMOOTH_TENDON_ARMATURE 2
#define MJH_SMOOTH_FACTOR_M 3
#define MJH_SMOOTH_COM_VEL 4
#define MJH_SMOOTH_RNE 5

/* one mjh_smooth call (definitions and the order of every sum: csrc/mjh_smooth.h; the functions are the reference's smooth.com_pos, crb, tendon_armature, factor_m,
 * com_vel and rne).  Every pointer is device memory, reals of the model's dtype, batch-major over B environments; the leaves are the caller's, read as they are.
 * Read / written per op (everything else may be NULL):
 *   COM_POS          xipos [B, nbody, 3], ximat, xmat [B, nbody, 9], xanchor, xaxis [B, njnt, 3], body_mass [nbody], body_inertia [nbody, 3]
 *                    -> subtree_com_out [B, nbody, 3], cinert_out [B, nbody, 10], cdof_out [B, nv, 6]
 *   CRB              cinert [B, nbody, 10], cdof [B, nv, 6], dof_armature [nv] -> crb_out [B, nbody, 10] (row 0 zero), qM_out [B, nv, nv] (dense, symmetric)
 *   TENDON_ARMATURE  qM [B, nv, nv], ten_J [B, ntendon, nv], tendon_armature [ntendon] -> qM_out
 *   FACTOR_M         qM (its lower triangle) -> qLD_out [B, nv, nv] (the lower triangle L, zeros above the diagonal)
 *   COM_VEL          cdof, qvel [B, nv] -> cvel_out [B, nbody, 6], cdof_dot_out [B, nv, 6]
 *   RNE              cdof, cdof_dot, cvel [B, nbody, 6], cinert, qvel, qacc [B, nv] (flg_acc only) -> qfrc_bias_out [B, nv]
 * gravity_x .. z and disableflags (DisableBit.GRAVITY) are the caller's options, read by RNE.  No output may alias an input. */
typedef struct mjhSmoothArgs {
  int32_t op, flg_acc, disableflags, reserved;
  int64_t B;
  double gravity_x, gravity_y, gravity_z;
  const void* xipos;
  const void* ximat;
  const void* xmat;
  const void* xanchor;
  const void* xaxis;
  const void* cinert;
  const void* cdof;
  const void* cdof_dot;
  const void* cvel;
  const void* qvel;
  const void* qacc;
  const void* qM;
  const void* ten_J;
  const void* body_mass;
  const void* body_inertia;
  const void* dof_armature;
  const void* tendon_armature;
  void* subtree_com_out;
  void* cinert_out;
  void* cdof_out;
  void* crb_out;
  void* qM_out;
  void* qLD_out;
  void* cvel_out;
  void* cdof_dot_out;
  void* qfrc_bias_out;
} mjhSmoothArgs;

/* one smooth-dynamics stage on a caller's Data (see mjhSmoothArgs).  One launch of the op's kernel (timing id MJH_KERNEL_SMOOTH_COM_POS + op), several environments per
 * workgroup, cut at the launch cap like mjh_postconstraint; runs on hip_stream without host synchronisation.  Returns 0 or a negative code (-12 when one environment
 * does not fit the LDS of a CU: mjh_last_error names the sizes; -22 for an unknown op, a null pointer or B < 0, before anything is launched).  B == 0 is a no-op, and
 * so is an op whose outputs are all empty for this model (nv == 0 for TENDON_ARMATURE .. RNE; ntendon == 0 for TENDON_ARMATURE). */
int mjh_smooth(const mjhModel* m, const mjhSmoothArgs* args, void* hip_stream);

/* the plan mjh_smooth uses for `op` on a model of nbody bodies, nv dofs and ntendon tendons in reals of real_bytes (4 / 8) bytes, a host computation (no device is
 * touched): out = {lanes per environment (16 / 32 / 64: from nbody, FACTOR_M from nv), environments per workgroup, reals of LDS per environment}.  Per environment the
 * LDS holds 10 nbody (COM_POS), 20 nbody + 12 nv (CRB), ntendon nv (TENDON_ARMATURE), nv (nv + 1) / 2 + nv (FACTOR_M), 13 nv (COM_VEL), 24 nbody + 6 nv (RNE) reals,
 * rounded up to a multiple of 4.  Returns 0, -12 when one environment does not fit the LDS of a CU (out is filled all the same), -22 for a bad argument. */
int mjh_smooth_plan(int op, int nbody, int nv, int ntendon, int real_bytes, int* lanes_envs_lds);

/* mjh_dynamics operations (mjhDynamicsArgs.op); MJH_KERNEL_DYNAMICS_TENDON + op is the kernel id the timing aid reports */
#define MJH_DYNAMICS_TENDON 0
#define MJH_DYNAMICS_TRANSMISSION 1
#define MJH_DYNAMICS_VELOCITY 2
#define MJH_DYNAMICS_PASSIVE 3
#define MJH_DYNAMICS_ACTUATION 4
#define MJH_DYNAMICS_ACCELERATION 5

/* one mjh_dynamics call (definitions and the order of every sum: csrc/mjh_dynamics.h; the functions are the reference's smooth.tendon, smooth.transmission, the two
 * products of forward._velocity, passive.passive, forward._actuation and forward._acceleration).  Every pointer is device memory, reals of the model's dtype; the leaves
 * are batch-major over B environments and the caller's, read as they are; the model values are the caller's Model's.  Read / written per op (everything else may be NULL):
 *   TENDON        qpos [B, nq] -> ten_length_out [B, ntendon], ten_J_out [B, ntendon, nv] (the joint terms and their coefficients are the compiled model's)
 *   TRANSMISSION  qpos, ten_length, ten_J (tendon transmissions), gear [nu, 6] -> actuator_length_out [B, nu], actuator_moment_out [B, nu, nv]
 *   VELOCITY      qvel [B, nv], actuator_moment [B, nu, nv], ten_J -> actuator_velocity_out [B, nu], ten_velocity_out [B, ntendon]
 *   PASSIVE       qpos, qvel, jnt_stiffness [njnt], qpos_spring [nq], dof_damping [nv]; with tendons ten_length, ten_velocity, ten_J, tendon_stiffness, tendon_damping
 *                 [ntendon], tendon_lengthspring [ntendon, 2]; with has_gravcomp or has_fluid xipos [B, nbody, 3], subtree_com, cdof [B, nv, 6], body_mass [nbody]; with
 *                 has_gravcomp body_gravcomp [nbody], jnt_actgravcomp [njnt] (reals, 0 / 1), gravity_x .. z; with has_fluid ximat [B, nbody, 9], cvel [B, nbody, 6],
 *                 body_inertia [nbody, 3], wind_x .. z, density, viscosity -> qfrc_passive_out [B, nv], with has_gravcomp qfrc_gravcomp_out [B, nv].
 *                 has_gravcomp here: the term is computed (the model has it and GRAVITY is not disabled).  SPRING or DAMPER disabled: -22 (both outputs are zero;
 *                 the caller makes them).
 *   ACTUATION     ctrl [B, nu], act [B, na] (stateful actuators), actuator_length, actuator_velocity, actuator_moment, gainprm [nu, gain_stride >= 3; 9 for a muscle
 *                 gain], biasprm [nu, bias_stride], dynprm [nu, dyn_stride >= 1; 3 for muscle dynamics], ctrlrange, forcerange, lengthrange [nu, 2], acc0 [nu],
 *                 jnt_actfrcrange [njnt, 2]; with has_gravcomp (the model has it) qfrc_gravcomp [B, nv], jnt_actgravcomp
 *                 -> act_dot_out [B, na], actuator_force_out [B, nu], qfrc_actuator_out [B, nv].  nu == 0 or ACTUATION disabled: -22 (the caller makes the zeros).
 *   ACCELERATION  qfrc_applied [B, nv], xfrc_applied [B, nbody, 6], xipos, subtree_com, cdof, qfrc_passive, qfrc_bias, qfrc_actuator [B, nv], qLD [B, nv, nv] (its lower
 *                 triangle) -> qfrc_smooth_out, qacc_smooth_out [B, nv]
 * disableflags are the caller's (SPRING, DAMPER, CLAMPCTRL, ACTUATION are read).  No output may alias an input. */
typedef struct mjhDynamicsArgs {
  int32_t op, disableflags, has_gravcomp, has_fluid;
  int32_t gain_stride, bias_stride, dyn_stride, reserved;
  int64_t B;
  double gravity_x, gravity_y, gravity_z;
  double wind_x, wind_y, wind_z;
  double density, viscosity;
  const void* qpos;
  const void* qvel;
  const void* ctrl;
  const void* act;
  const void* ten_length;
  const void* ten_velocity;
  const void* ten_J;
  const void* actuator_length;
  const void* actuator_velocity;
  const void* actuator_moment;
  const void* xipos;
  const void* ximat;
  const void* subtree_com;
  const void* cdof;
  const void* cvel;
  const void* qfrc_gravcomp;
  const void* qfrc_applied;
  const void* xfrc_applied;
  const void* qfrc_passive;
  const void* qfrc_bias;
  const void* qfrc_actuator;
  const void* qLD;
  const void* jnt_stiffness;
  const void* qpos_spring;
  const void* dof_damping;
  const void* tendon_stiffness;
  const void* tendon_damping;
  const void* tendon_lengthspring;
  const void* body_mass;
  const void* body_inertia;
  const void* body_gravcomp;
  const void* jnt_actgravcomp;
  const void* jnt_actfrcrange;
  const void* gainprm;
  const void* biasprm;
  const void* dynprm;
  const void* ctrlrange;
  const void* forcerange;
  const void* gear;
  const void* lengthrange;
  const void* acc0;
  void* ten_length_out;
  void* ten_J_out;
  void* actuator_length_out;
  void* actuator_moment_out;
  void* actuator_velocity_out;
  void* ten_velocity_out;
  void* qfrc_passive_out;
  void* qfrc_gravcomp_out;
  void* act_dot_out;
  void* qfrc_actuator_out;
  void* actuator_force_out;
  void* qfrc_smooth_out;
  void* qacc_smooth_out;
} mjhDynamicsArgs;

/* one stage of the smooth dynamics on a caller's Data (see mjhDynamicsArgs).  One launch of the op's kernel (timing id MJH_KERNEL_DYNAMICS_TENDON + op), several
 * environments per workgroup, cut at the launch cap like mjh_smooth; runs on hip_stream without host synchronisation.  Returns 0 or a negative code (-12 when one
 * environment does not fit the LDS of a CU: mjh_last_error names the sizes; -22 for an unknown op, a null pointer, a parameter row that is too short, B < 0 or a
 * branch that launches nothing (see the struct), before anything is launched).  B == 0 is a no-op, and so is an op whose outputs are all empty for this model
 * (ntendon == 0 for TENDON; nu == 0 for TRANSMISSION; nu == 0 and ntendon == 0, or nv == 0, for VELOCITY; nv == 0 for PASSIVE and ACCELERATION). */
int mjh_dynamics(const mjhModel* m, const mjhDynamicsArgs* args, void* hip_stream);

/* the plan mjh_dynamics uses for `op` on a model of nq positions, nv dofs, nu actuators, nbody bodies and ntendon tendons in reals of real_bytes (4 / 8) bytes, a host
 * computation (no device is touched): out = {lanes per environment (16 / 32 / 64: from nv for TENDON, PASSIVE and ACCELERATION, from nu for TRANSMISSION, VELOCITY and
 * ACTUATION), environments per workgroup, reals of LDS per environment}.  Per environment the LDS holds nq (TENDON), nq + ntendon + 3 nu (TRANSMISSION),
 * nv + (nu + ntendon) (nv | 1) (VELOCITY: an odd row stride), nv + ntendon + 12 nbody (PASSIVE), nu (ACTUATION), nv (nv + 1) / 2 rounded up to a multiple of 4 + nv + 6 nbody (ACCELERATION)
 * reals, rounded up to a multiple of 4, at least 4.  Returns 0, -12 when one environment does not fit the LDS of a CU (out is filled all the same), -22 for a bad
 * argument. */
int mjh_dynamics_plan(int op, int nq, int nv, int nu, int nbody, int ntendon, int real_bytes, int* lanes_envs_lds);

/* mjh_constraint_space operations (mjhConstraintSpaceArgs.op); MJH_KERNEL_EFC_MUL_J + op is the kernel id the timing aid reports */
#define MJH_EFC_MUL_J 0
#define MJH_EFC_MUL_JT 1
#define MJH_EFC_UPDATE 2
#define MJH_EFC_AR 3

/* one mjh_constraint_space call (definitions: csrc/mjh_efc.h).  Every pointer is device memory, reals of the model's dtype unless stated, batch-major over B
 * environments; the leaves are a finished pass's: efc_J [B, nefc, nv], efc_D / efc_aref / efc_frictionloss [B, nefc], qM / qLD [B, nv, nv], qfrc_smooth /
 * qacc_smooth [B, nv].  Vector j of environment e reads vec[e * vec_env + j * vec_k + i] (element strides; 0: shared).  A NULL output is not an option: every
 * output of the op is written.  Per op (outputs environment-major, contiguous):
 *   MUL_J   efc_J, vec (nv entries each)   -> out [B, K, nefc] = J vec_j
 *   MUL_JT  efc_J, vec (nefc entries each) -> out [B, K, nv] = J^T vec_j
 *   UPDATE  efc_J, efc_D, efc_frictionloss and either
 *           qacc [B, nv] with efc_aref, qM, qfrc_smooth, qacc_smooth -> jar = J qacc - aref, efc_force [B, nefc], efc_state [B, nefc] int32 (0 satisfied, 1 quadratic,
 *             2 linear-neg, 3 linear-pos), qfrc_constraint [B, nv] = J^T efc_force, cost / gauss / grad_norm [B], grad [B, nv]; or
 *           jar_in [B, nefc] with qacc NULL (MuJoCo's mj_constraintUpdate) -> efc_force, efc_state, qfrc_constraint, cost (without the Gauss term)
 *           ne_nf: the equality and friction rows, always quadratic unless linear; floss != 0: the friction rows have their linear zones; grad_norm =
 *           |grad| / (meaninertia * max(1, nv))
 *   AR      efc_J, efc_D, efc_aref, qLD (lower triangle), qacc_smooth -> AR [B, nefc, nefc] = J (L L^T)^-1 J^T + diag(D > 0 ? 1 / D : 0), both triangles
 *             from one computed value; b [B, nefc] = J qacc_smooth - aref
 * K >= 1 (MUL_J, MUL_JT); K * max(nv, nefc) must stay below 2^30. */
typedef struct mjhConstraintSpaceArgs {
  int32_t op;
  int32_t K, ne_nf, floss;
  int64_t B;
  double meaninertia;
  const void* efc_J;
  const void* efc_D;
  const void* efc_aref;
  const void* efc_frictionloss;
  const void* qM;
  const void* qLD;
  const void* qfrc_smooth;
  const void* qacc_smooth;
  const void* qacc;
  const void* jar_in;
  const void* vec;
  int64_t vec_env, vec_k;
  void* out;
  void* jar;
  void* efc_force;
  int32_t* efc_state;
  void* qfrc_constraint;
  void* cost;
  void* gauss;
  void* grad;
  void* grad_norm;
  void* AR;
  void* b;
} mjhConstraintSpaceArgs;

/* the constraint-space functions on a finished pass (see mjhConstraintSpaceArgs).  Runs on hip_stream without host synchronisation.  Returns 0 or a negative
 * code (AR: -12 when qLD's triangle and two row chunks do not fit the LDS of a workgroup); B == 0, nv == 0 and nefc == 0 are no-ops. */
int mjh_constraint_space(const mjhModel* m, const mjhConstraintSpaceArgs* args, void* hip_stream);

/* the chunk plan mjh_constraint_space uses for operation op on a model of nv dofs and nefc rows in reals of real_bytes (4 / 8) bytes, a host computation (no
 * device is touched): out = {rows of efc_J per LDS chunk, number of chunks, rows of the last chunk, bytes of LDS per workgroup}.  Returns 0, -12 when the
 * operation does not fit a workgroup's LDS, -22 for a bad argument. */
int mjh_constraint_space_plan(int op, int nv, int nefc, int real_bytes, int* chunk_nchunk_last_lds);

/* one mjh_pgs call (definitions: csrc/mjh_pgs.h).  Every pointer is device memory, reals of the model's dtype unless stated, batch-major over B environments; the
 * leaves are a finished pass's, as for mjhConstraintSpaceArgs: efc_J [B, nefc, nv], efc_D / efc_aref / efc_frictionloss [B, nefc], qLD [B, nv, nv] (lower triangle),
 * qacc_smooth [B, nv].  The problem: min_f 1/2 f^T AR f + f^T b with AR = J (L L^T)^-1 J^T + diag(D > 0 ? 1 / D : 0), b = J qacc_smooth - aref, over: rows
 * i < ne free, ne <= i < ne + nf with |f_i| <= efc_frictionloss_i, later rows f_i >= 0.  force0 (NULL: zeros; environment e reads force0[e * force0_env + i],
 * force0_env 0: shared) is projected onto that set; then at most `iterations` sweeps over the rows in order, each followed by
 * improvement *= 1 / (meaninertia * max(1, nv)); an environment stops when improvement < tolerance.  Outputs, every one written: efc_force [B, nefc] = f,
 * qfrc_constraint [B, nv] = J^T f, qacc [B, nv] = qacc_smooth + (L L^T)^-1 J^T f, cost [B] (the dual cost), improvement [B] (of the last sweep; 0 without one),
 * niter [B] int32 (the sweeps run). */
typedef struct mjhPgsArgs {
  int32_t ne, nf, iterations, pad_;
  int64_t B;
  double meaninertia, tolerance;
  const void* efc_J;
  const void* efc_D;
  const void* efc_aref;
  const void* efc_frictionloss;
  const void* qLD;
  const void* qacc_smooth;
  const void* force0;
  int64_t force0_env;
  void* efc_force;
  void* qfrc_constraint;
  void* qacc;
  void* cost;
  void* improvement;
  int32_t* niter;
} mjhPgsArgs;

/* projected Gauss-Seidel on the dual problem of a finished pass (see mjhPgsArgs; MuJoCo's mj_solPGS for rows of dimension one).  One launch, one wavefront per
 * environment, cut at the launch cap like mjh_constraint_space; runs on hip_stream without host synchronisation.  Returns 0 or a negative code (-12 when qLD's
 * triangle and all nefc rows of nv | 1 reals do not fit the LDS of a workgroup: mjh_last_error names the sizes); B == 0, nv == 0 and nefc == 0 are no-ops. */
int mjh_pgs(const mjhModel* m, const mjhPgsArgs* args, void* hip_stream);

/* the plan mjh_pgs uses for a model of nv dofs and nefc rows in reals of real_bytes (4 / 8) bytes, a host computation (no device is touched): out = {rows of
 * efc_J per staging step, number of steps, rows of the last step, bytes of LDS per workgroup}.  Returns 0, -12 when the model does not fit a workgroup's LDS
 * (out is filled all the same: the bytes it would need), -22 for a bad argument. */
int mjh_pgs_plan(int nv, int nefc, int real_bytes, int* chunk_nchunk_last_lds);

/* one mjh_noslip call (definitions: csrc/mjh_noslip.h).  Every pointer is device memory, reals of the model's dtype unless stated, batch-major over B environments;
 * the leaves are a finished pass's, as for mjhPgsArgs, and contact_friction [B, ncon, 5] (read when the model's cone is elliptic; may be NULL otherwise).  The
 * sweeps run on A = J (L L^T)^-1 J^T (no regulariser) over the friction dimensions only: the friction-loss rows ne <= i < ne + nf, then every contact of
 * condim > 1 in slot order (the model's static contact tables and cone) -- the pairs of opposing edges of a pyramidal contact, or the dim - 1 friction rows of an
 * elliptic one through a QCQP in its normal force.  force0 (required; environment e reads force0[e * force0_env + i], force0_env 0: shared) is NOT projected;
 * every other row leaves as it came.  At most `iterations` sweeps, each followed by improvement *= 1 / (meaninertia * max(1, nv)); an environment stops when
 * improvement < tolerance.  Outputs, every one written: efc_force [B, nefc], qfrc_constraint [B, nv] = J^T f, qacc [B, nv] = qacc_smooth + (L L^T)^-1 J^T f,
 * cost [B] = 1/2 f^T A f + f . b, improvement [B] (of the last sweep; 0 without one), niter [B] int32 (the sweeps run). */
typedef struct mjhNoslipArgs {
  int32_t ne, nf, iterations, pad_;
  int64_t B;
  double meaninertia, tolerance;
  const void* efc_J;
  const void* efc_D;
  const void* efc_aref;
  const void* efc_frictionloss;
  const void* qLD;
  const void* qacc_smooth;
  const void* force0;
  const void* contact_friction;
  int64_t force0_env;
  void* efc_force;
  void* qfrc_constraint;
  void* qacc;
  void* cost;
  void* improvement;
  int32_t* niter;
} mjhNoslipArgs;

/* the no-slip friction post-solver on a finished pass (see mjhNoslipArgs; MuJoCo's mj_solNoSlip).  One launch, one wavefront per environment, cut at the launch cap
 * like mjh_pgs; runs on hip_stream without host synchronisation.  Returns 0 or a negative code (-12 when the model does not fit the LDS of a workgroup:
 * mjh_last_error names the sizes); B == 0, nv == 0 and nefc == 0 are no-ops. */
int mjh_noslip(const mjhModel* m, const mjhNoslipArgs* args, void* hip_stream);

/* the plan mjh_noslip uses for a model of nv dofs, nefc rows and ncon contact slots in reals of real_bytes (4 / 8) bytes, a host computation (no device is
 * touched): out = {rows of efc_J per staging step, number of steps, rows of the last step, bytes of LDS per workgroup}: mjh_pgs_plan's, plus 22 reals a contact
 * slot (the blocks of A, 15; mu, 5; the table entry, 2).  Returns 0, -12 when the model does not fit a workgroup's LDS (out is filled all the same: the bytes it
 * would need), -22 for a bad argument. */
int mjh_noslip_plan(int nv, int nefc, int ncon, int real_bytes, int* chunk_nchunk_last_lds);

/* one mjh_solve call (definitions: csrc/mjh_solve.h; the algorithm is the reference's solver.solve, _src/solver.py:244-553).  Every pointer is device memory, reals of
 * the model's dtype unless stated, batch-major over B environments; the leaves are a finished pass's: efc_J [B, nefc, nv], efc_D / efc_aref / efc_frictionloss
 * [B, nefc], qM [B, nv, nv] (dense; the lower triangle is read), qLD [B, nv, nv] (lower triangle; CG only, may be NULL for Newton), qfrc_smooth / qacc_smooth /
 * qacc_warmstart [B, nv] (qacc_warmstart: read when `warmstart`, may be NULL otherwise).  ne, nf: the model's equality and friction row counts; floss: the
 * friction-loss linear zones apply (nf > 0 and DisableBit.FRICTIONLOSS clear); solver: 1 (CG) or 2 (Newton), mjtSolver's values; fixed: exactly `iterations` bodies
 * and `ls_iterations` line-search bodies; warmstart: the start is qacc_warmstart when its cost is strictly below qacc_smooth's (0: qacc_smooth).  iterations == 1
 * runs one body unconditionally; otherwise an environment stops when niter >= iterations, (prev_cost - cost) / scale < tolerance or |grad| / scale < tolerance,
 * scale = meaninertia * max(1, nv).  Outputs, every one written: qacc_out and qacc_warmstart_out [B, nv] (the same values), qfrc_constraint_out [B, nv],
 * efc_force_out [B, nefc], cost [B] (at the returned qacc), improvement [B] ((prev_cost - cost) / scale of the last body; +inf without one), grad_norm [B]
 * (|grad| / scale at the returned qacc), niter [B] int32 (the bodies run).  No output may alias an input. */
typedef struct mjhSolveArgs {
  int32_t ne, nf, floss, solver, iterations, ls_iterations, fixed, warmstart;
  int64_t B;
  double tolerance, ls_tolerance, meaninertia;
  const void* efc_J;
  const void* efc_D;
  const void* efc_aref;
  const void* efc_frictionloss;
  const void* qM;
  const void* qLD;
  const void* qfrc_smooth;
  const void* qacc_smooth;
  const void* qacc_warmstart;
  void* qacc_out;
  void* qacc_warmstart_out;
  void* qfrc_constraint_out;
  void* efc_force_out;
  void* cost;
  void* improvement;
  void* grad_norm;
  int32_t* niter;
} mjhSolveArgs;

/* the reference's constraint solver on a finished pass (see mjhSolveArgs).  One launch, one wavefront per environment, cut at the launch cap like mjh_pgs; runs on
 * hip_stream without host synchronisation.  Returns 0 or a negative code (-12 when the working set does not fit the LDS of a workgroup: mjh_last_error names nv,
 * nefc, the solver and the bytes; -22 for a null pointer or a bad size, before anything is launched); B == 0, nv == 0 and nefc == 0 are no-ops. */
int mjh_solve(const mjhModel* m, const mjhSolveArgs* args, void* hip_stream);

/* the plan mjh_solve uses for `solver` (1: CG, 2: Newton) on a model of nv dofs and nefc rows in reals of real_bytes (4 / 8) bytes, a host computation (no device is
 * touched): out = {rows of efc_J per staging step, number of steps, rows of the last step, bytes of LDS per workgroup}.  The LDS holds two packed triangles (qM; qLD
 * or Newton's H and its factor), all nefc rows of nv | 1 reals, five reals a row (six for Newton), ten dof vectors and 64 partial sums:
 * nv (nv + 1) + nefc (nv | 1) + (5 | 6) nefc + 10 nv + 64 reals.  Returns 0, -12 when that does not fit a workgroup's LDS (out is filled all the same: the bytes
 * it would need), -22 for a bad argument. */
int mjh_solve_plan(int solver, int nv, int nefc, int real_bytes, int* chunk_nchunk_last_lds);

/* mjh_jacobian operations (mjhJacobianArgs.op); MJH_KERNEL_JACOBIAN_POINT + op (matrix form) or MJH_KERNEL_JACOBIAN_POINT_VEC + op (product form) is the kernel id
 * the timing aid reports */
#define MJH_JACOBIAN_POINT 0
#define MJH_JACOBIAN_DOT 1
#define MJH_JACOBIAN_SUBTREE_COM 2
#define MJH_JACOBIAN_ANGMOM 3

/* one mjh_jacobian call.  Every pointer is device memory holding reals of the model's dtype, batch-major over B environments; the leaves are a finished forward
 * pass's: cdof / cdof_dot [B, nv, 6], cvel [B, nbody, 6], subtree_com / xipos [B, nbody, 3], ximat [B, nbody, 9].  The MODEL VALUES body_mass [nbody],
 * body_subtreemass [nbody] and body_inertia [nbody, 3] are arguments of the call (the caller's Model, not the blob).  body_id: P body ids in [0, nbody)
 * (body_stride 1) or one id for every query (0); the library does not validate them, nor that body_subtreemass[body] != 0.  point is addressed as in mjhSupportArgs.
 * Per op, what is read and written (outputs environment-major, contiguous; the definitions and the order of every sum are in csrc/mjh_jacobian.h):
 *   POINT        cdof, subtree_com, point                   -> out0 = jacp, out1 = jacr [B, P, nv, 3] (mjh_support's JAC)
 *   DOT          the same, cdof_dot, cvel                   -> out0 = jacp_dot, out1 = jacr_dot [B, P, nv, 3]
 *   SUBTREE_COM  cdof, subtree_com, xipos, body_mass, body_subtreemass            -> out0 [B, P, nv, 3]
 *   ANGMOM       the same, ximat, body_inertia                                    -> out0 [B, P, nv, 3]
 * vec != NULL ([B, nv]) selects the product form: out0 (and out1) are [B, P, 3] = sum_i matrix[i, :] vec[i] in ascending dof order, the matrix is not written.
 * P >= 1 and P * nv * 3 must stay below 2^30.  No output may alias an input. */
typedef struct mjhJacobianArgs {
  int32_t op, P;
  int64_t B;
  const void *cdof, *cdof_dot, *cvel, *subtree_com, *xipos, *ximat;
  const void *body_mass, *body_subtreemass, *body_inertia;
  const int32_t* body_id;
  int64_t body_stride;
  const void* point;
  int64_t point_env, point_q;
  const void* vec;
  void *out0, *out1;
} mjhJacobianArgs;

/* the Jacobian block on a finished forward pass (see mjhJacobianArgs).  Runs on hip_stream without host synchronisation.  Returns 0 or a negative code (-12: one
 * environment's rows do not fit a workgroup's LDS in the product form); B == 0 is a no-op. */
int mjh_jacobian(const mjhModel* m, const mjhJacobianArgs* args, void* hip_stream);

/* Finite-difference transition Jacobians (MuJoCo's mjd_transitionFD), as two launches around an mjh_step of the caller's own.  State x = (qpos in
 * tangent space: nv, qvel: nv, act: na), ns = 2 nv + na; column c in [0, ns) nudges entry c of x, column ns + i nudges ctrl[i].  A call serves the
 * columns [col0, col0 + ncol) of all B environments.  Each column of an environment owns nside = (centered ? 2 : 1) environments ("slots") of a
 * scratch batch of B * ncol * nside environments, slot (e * ncol + (c - col0)) * nside + side; side 0 carries the nudge +eps, side 1 the nudge -eps.
 * A ctrl nudge is taken only if ctrl and the nudged ctrl both lie inside actuator_ctrlrange when actuator_ctrllimited; the backward one only when
 * centered or when the forward one was refused.  One-sided, the single slot of a ctrl column carries the forward nudge if taken, else the backward
 * one, else ctrl unchanged; centered, a refused side carries ctrl unchanged.
 *
 * mjh_fd_perturb: for every slot, copies every leaf that is non-NULL in `scratch` from environment e of `in` (which must carry it) and applies the
 * slot's nudge: addition, or for the rotational dofs of ball / free joints the rotation of the quaternion by eps about the dof's local axis
 * (quat_integrate, math.py:377).  scratch.qpos / qvel must be non-NULL, act / ctrl when na / nu > 0.
 * mjh_fd_difference: reads qpos / qvel / act (and sensordata when C, D are given) of `nominal` (the step of `in`, B environments) and of `stepped`
 * (the step of the scratch batch) and in.ctrl, and writes the columns [col0, col0 + ncol) of A [B, ns, ns] and Bm [B, ns, nu] (C [B, nsensordata, ns],
 * D [B, nsensordata, nu]; both NULL or both given): rows = next state, qpos rows differenced in tangent space (subtraction, or the rotation vector
 * of q0^-1 q1, math.py:276).  One side: (y+ - y0) / eps or (y0 - y-) / eps; centered state columns: (y+ - y-) / (2 eps); a ctrl column with both
 * sides: the mean of the two one-sided differences; with neither: zeros.  Bm / D may be NULL when nu == 0.
 * Both run on hip_stream without host synchronisation; eps is rounded to the model's dtype.  Return 0 or a negative code; B == 0 is a no-op. */
int mjh_fd_perturb(const mjhModel* m, const mjhData* in, mjhData* scratch, int64_t B, int col0, int ncol, double eps, int centered, void* hip_stream);
int mjh_fd_difference(const mjhModel* m, const mjhData* in, const mjhData* nominal, const mjhData* stepped, int64_t B, int col0, int ncol, double eps,
                      int centered, void* A, void* Bm, void* C, void* D, void* hip_stream);

/* The vector-Jacobian product of those Jacobians, in place of mjh_fd_difference after the same mjh_fd_perturb and mjh_step: for the columns
 * [col0, col0 + ncol),  out[e, c] = sum_row g[e, row] * J[e, row, c]  with J[e, row, c] exactly the value mjh_fd_difference would store and
 * g = g_state [B, ns] (cotangent of the next state in the order of x) followed, when g_sens is given, by g_sens [B, nsensordata]: gx [B, ns] receives
 * the columns c < ns (A^T g_state + C^T g_sens), gu [B, nu] the ctrl columns (B^T g_state + D^T g_sens; may be NULL when nu == 0).  Only the columns
 * of the call are written.  The additions of one sum happen in an order that depends on the number of rows alone: a result is the same bits from run
 * to run and for every way of cutting the columns into calls. */
int mjh_fd_vjp(const mjhModel* m, const mjhData* in, const mjhData* nominal, const mjhData* stepped, int64_t B, int col0, int ncol, double eps, int centered,
               const void* g_state, const void* g_sens, void* gx, void* gu, void* hip_stream);

/* Cotangents between qpos coordinates (nq) and the tangent space (nv) at `qpos` [B, nq], under q(d) = q (x) exp(d / 2) for the quaternions of ball / free
 * joints (the convention of mjh_fd_perturb / mjh_fd_difference) and the identity elsewhere.
 * MJH_FD_TANGENT_PULL: g_in [B, nq] -> g_out [B, nv]; a rotational dof k gives <g_in[quaternion], q (x) (0, e_k)> / 2.
 * MJH_FD_TANGENT_PUSH: g_in [B, nv] -> g_out [B, nq]; a quaternion receives 2 sum_k g_in[k] q (x) (0, e_k) / |q|^2: the cotangent whose pull is g_in and
 * whose component along q is zero (how a step depends on a quaternion's norm is not differentiated); zeros for an all-zero quaternion, which no
 * perturbation of mjh_fd_perturb moves.  Every entry of g_out is written. */
#define MJH_FD_TANGENT_PULL 0
#define MJH_FD_TANGENT_PUSH 1
int mjh_fd_tangent(const mjhModel* m, const void* qpos, const void* g_in, void* g_out, int64_t B, int mode, void* hip_stream);

/* Finite-difference Jacobians of inverse dynamics (MuJoCo's mjd_inverseFD), as two launches around an mjh_inverse of the caller's own.  Column c in
 * [0, nv) nudges qpos along dof c (tangent space), [nv, 2 nv) qvel, [2 nv, 3 nv) qacc; nothing else is perturbed.  A call serves the columns
 * [col0, col0 + ncol) of all B environments, in the slot layout of mjh_fd_perturb: each column of an environment owns nside = (centered ? 2 : 1)
 * environments of a scratch batch of B * ncol * nside, slot (e * ncol + (c - col0)) * nside + side; side 0 carries the nudge +eps, side 1 -eps.
 *
 * mjh_ifd_perturb: for every slot, copies every leaf that is non-NULL in `scratch` from environment e of `in` (which must carry it) and applies the
 * slot's nudge by the rule of mjh_fd_perturb: addition, or for the rotational dofs of ball / free joints the rotation of the quaternion by eps about
 * the dof's local axis.  scratch.qpos / qvel / qacc must be non-NULL (mjh_inverse reads in.qacc).  The leaves an mjh_inverse call can read from its
 * input are those a step can read, qacc, and -- for the sensors -- the caller's actuator_force / qfrc_actuator.
 * mjh_ifd_difference: from the nominal pass's qfrc_inverse `nominal_f` [B, nv] and sensordata `nominal_sens` [B, nsensordata], and those of the
 * scratch batch (`stepped_f`, `stepped_sens`: [slots, ...]), writes the columns of the call into DfDq, DfDv, DfDa [B, nv, nv] and -- when all three
 * are given -- DsDq, DsDv, DsDa [B, nsensordata, nv]: column c < nv of DfDq / DsDq, c - nv of DfDv / DsDv, c - 2 nv of DfDa / DsDa.  Rows are outputs
 * (MuJoCo stores the transposes).  Every entry is (y+ - y0) / eps or, centered, (y+ - y-) / (2 eps): no output is a quaternion.  nominal_* are not
 * read when centered and may then be NULL; the sensor pointers may be NULL when the sensor matrices are.
 * Both run on hip_stream without host synchronisation; eps is rounded to the model's dtype.  Return 0 or a negative code; B == 0 is a no-op. */
int mjh_ifd_perturb(const mjhModel* m, const mjhData* in, mjhData* scratch, int64_t B, int col0, int ncol, double eps, int centered, void* hip_stream);
int mjh_ifd_difference(const mjhModel* m, const void* nominal_f, const void* nominal_sens, const void* stepped_f, const void* stepped_sens, int64_t B,
                       int col0, int ncol, double eps, int centered, void* DfDq, void* DfDv, void* DfDa, void* DsDq, void* DsDv, void* DsDa,
                       void* hip_stream);

/* per-environment ELEMENT count of every mjhData leaf in ABI order (reals, then int32, then int64 leaves): a leaf handed to
 * mjh_forward / mjh_step / mjh_reset_where must hold exactly B * count elements.  The binding validates tensor sizes against
 * this before it passes raw pointers (the kernels index `ptr + env * count` unchecked).  Writes min(n, max) entries, returns n. */
int mjh_model_leaf_counts(const mjhModel* m, int64_t* counts, int max);

/* masked in-place reset of environments -- the env caller's `self._dx[mask] = self._make_batch(n)` (zoo/base.py:266-273,
 * :289-293 partial reset, :327-331 fused auto-reset) as ONE launch without a host sync.  For every environment e with
 * mask[e] != 0, every leaf that is non-NULL in `d` is overwritten with that leaf of `d0` (ONE environment, same dtype; the
 * leaf must be non-NULL there too), except qpos / qvel, which take row e of qpos_rows [B, nq] / qvel_rows [B, nv] when those
 * are non-NULL (the caller's dx0 + reset noise).  Environments with mask[e] == 0 are untouched.  `mask`: B bytes (torch.bool). */
int mjh_reset_where(const mjhModel* m, mjhData* d, const mjhData* d0, const unsigned char* mask, const void* qpos_rows,
                    const void* qvel_rows, int64_t B, void* hip_stream);

/* bytes of dynamic LDS one environment occupies in arena `arena`: 0..4 the pipeline phases (kinematics, crb/factor,
 * collision/constraint, velocity/acceleration, solve/integrate), 5 the register solver, 16 its first tier, 17 the fused
 * kinematics + crb + velocity kernel (MJH_KERNEL_KCV), 18 the fused constraint + solver kernel (MJH_KERNEL_CS), 19 the
 * two-wave form of MJH_KERNEL_KCV (MJH_KERNEL_KCV2).  0 for any other number. */
int mjh_model_lds_bytes(const mjhModel* m, int arena);

/* measurement aid used by bench.py for the per-kernel roofline: while enabled, every kernel launch of mjh_step / mjh_forward is
 * bracketed by HIP events on the launch stream (mjh_inverse, mjh_ray, mjh_render, mjh_support, mjh_fd_perturb, mjh_fd_difference, mjh_fd_vjp, mjh_fd_tangent, mjh_ifd_perturb, mjh_ifd_difference, mjh_postconstraint, mjh_contact_sensors, mjh_energy, mjh_integrate, mjh_jacobian, mjh_geom_distance, mjh_qpos_arith, mjh_ik_site_step, mjh_constraint_space, mjh_pgs, mjh_noslip, mjh_solve, mjh_smooth and mjh_dynamics too); mjh_debug_phase_times() waits for the most recent call and returns, per launch,
 * the elapsed milliseconds and the kernel id (MJH_KERNEL_*).  Returns the number of launches (<= max) or a negative code. */
int mjh_debug_phase_timing(int enable);
int mjh_debug_phase_times(float* ms, int* kernel_ids, int max);

/* diagnostic builds only (-DMJH_STAMPS, tools/stamps.py): device buffer the kernels write their s_memtime section stamps into; NULL turns
 * them off.  The shipped library is built without MJH_STAMPS: the pointer is stored and nothing reads it. */
void mjh_debug_set_stamps(void* dev_ptr);

/* global-memory bytes ONE launch of kernel `kernel` (MJH_KERNEL_*) reads and writes per environment in a step (MJH_KERNEL_INVERSE: in an mjh_inverse call): the library's own
 * account of its loads / stores through the Data leaves (csrc/mjh_io.h) -- the per-kernel "algorithmic bytes" of the roofline.
 * read_write_bytes[0] = read, [1] = written.  RK4 models: the mean over the four stage launches of a step (stages 1..3 write a private
 * workspace holding only the leaves a later phase reads).  MJH_KERNEL_RENDER (an mjh_render call): [0] = bytes read per environment at most (the frames
 * of every geom, one camera's pose, the light poses), [1] = bytes written per output pixel with rgb in the model's dtype (rgb, depth, seg); -2 for a
 * model without cameras.  MJH_KERNEL_JAC .. MJH_KERNEL_SOLVE_M (an mjh_support call): per environment for one query point (JAC, APPLY_FT: the dof
 * rows, the root's subtree_com, the point, force and torque; jacp + jacr or the product), the whole sum (XFRC) or one vector (MUL_M, SOLVE_M: the matrix
 * loaded whole, the vector, the result).  MJH_KERNEL_FD_PERTURB / MJH_KERNEL_FD_DIFFERENCE: per slot, the input leaves a step of this model can read,
 * read and written (an upper bound: the caller's Data may lack some), and one slot's qpos, qvel, act and sensordata read, with [1] = one column of A and C.  MJH_KERNEL_FD_VJP: per (environment, column), one slot's and the nominal
 * qpos, qvel, act and sensordata (an upper bound: a one-sided column reads the nominal, a centered state column its two slots) and the cotangent, with
 * [1] = one entry of gx / gu; MJH_KERNEL_FD_TANGENT: per environment, qpos and a cotangent of at most nq entries read, one written.  MJH_KERNEL_POSTCON (an
 * mjh_postconstraint call with all three flags): per environment, every input leaf of mjhPostconArgs once, from the leaf extents, and the six outputs.  MJH_KERNEL_ENERGY
 * (an mjh_energy call with MJH_ENERGY_POS | MJH_ENERGY_VEL): per environment, qpos, qvel, xipos, ten_length and qM once, the two energies written.  MJH_KERNEL_INTEGRATE
 * (an mjh_integrate call for implicit: QDERIV | IMPLICIT | STATE): per environment, the leaves that call reads once (qM in full), qpos, qvel, act and time written.  MJH_KERNEL_JACOBIAN_* (an mjh_jacobian call): per environment
 * for one query, the dof rows and the body rows the operation reads (DOT: cvel and cdof_dot too; the subtree operations: xipos, ximat for ANGMOM) and the matrices,
 * or, for the *_VEC ids, vec and the 3-vectors.  MJH_KERNEL_QUADRIC: like MJH_KERNEL_CONVEX, the two geom frames of each of its pairs and the pair's contacts.  MJH_KERNEL_IFD_PERTURB / MJH_KERNEL_IFD_DIFFERENCE:
 * per slot, the input leaves an mjh_inverse call of this model can read, read and written (an upper bound: the caller's Data may lack some), and one slot's qfrc_inverse and
 * sensordata read, with [1] = one column of DfD* and DsD*.  MJH_KERNEL_GEOM_DISTANCE (an mjh_geom_distance call): per (pair, environment), the two geom frames and sizes
 * and the pair's row read, dist and fromto written.  MJH_KERNEL_QPOS_ARITH (an integrate call of mjh_qpos_arith): per environment, qpos and qvel read, qpos written.
 * MJH_KERNEL_IK_SITE (an updating mjh_ik_site_step call with both targets): per environment, cdof, the site's frame, its root's subtree_com, the targets, qpos and the
 * three state words read, qpos and the state words written.  MJH_KERNEL_EFC_MUL_J .. MJH_KERNEL_EFC_AR (an mjh_constraint_space call): per environment, efc_J once and
 * one vector in, one out (MUL_J, MUL_JT); efc_J, the three row leaves, qM and the three dof vectors in, the outputs of the qacc form out (UPDATE); efc_J once (a model of one
 * chunk), qLD, efc_D, efc_aref and qacc_smooth in, AR and b out (AR); -2 for a model without dofs or rows.  MJH_KERNEL_PGS (an mjh_pgs call
 * from zeros, without force0): per environment, efc_J twice (W, then J^T f), qLD, the three row leaves and qacc_smooth in, efc_force, qfrc_constraint, qacc and the
 * three scalars out; -2 for a model without dofs or rows.  MJH_KERNEL_NOSLIP (an mjh_noslip call): per environment, efc_J twice, qLD, the three row leaves, force0,
 * qacc_smooth and, with an elliptic cone, the friction of every contact slot in -- (2 nefc nv + nv^2 + 4 nefc + nv [+ 5 ncon]) reals --, efc_force, qfrc_constraint,
 * qacc and the three scalars out -- (nefc + 2 nv + 2) reals + 4 bytes; -2 for a model without dofs or rows.  MJH_KERNEL_SOLVE (an mjh_solve call with the warm start
 * on): per environment, efc_J, qM and qLD once (qLD: counted for both solvers, Newton does not read it), efc_D and efc_frictionloss once, efc_aref twice (once per start
 * candidate; a third time when the smooth start wins), qfrc_smooth, qacc_smooth and qacc_warmstart in -- (nefc nv + 2 nv^2 + 4 nefc + 3 nv) reals --, qacc,
 * qacc_warmstart, qfrc_constraint, efc_force and the three scalars out -- (nefc + 3 nv + 3) reals + 4 bytes; -2 for a model without dofs or rows.  MJH_KERNEL_SMOOTH_COM_POS + op (an mjh_smooth call), per environment, every leaf the op
 * reads once, from the leaf extents, and what it writes, in reals: COM_POS 21 nbody + 6 njnt in, 13 nbody + 6 nv out; CRB 10 nbody + 6 nv in, 10 nbody + nv^2 out;
 * TENDON_ARMATURE nv^2 + ntendon nv in, nv^2 out (-2 without tendons); FACTOR_M nv (nv + 1) / 2 in, nv^2 out; COM_VEL 7 nv in, 6 nbody + 6 nv out; RNE (with flg_acc)
 * 14 nv + 16 nbody in, nv out; -2 for a model without dofs, COM_POS and CRB apart.  MJH_KERNEL_DYNAMICS_TENDON + op (an mjh_dynamics call) is not accounted: -2.
 * Returns 0, or -2 when this model's step does not launch that kernel. */
int mjh_model_kernel_io(const mjhModel* m, int kernel, int64_t* read_write_bytes);

/* last error message of the calling thread ("" if none) */
const char* mjh_last_error(void);

/* comma-separated field lists in ABI order (lets the binding assert it is in sync) */
const char* mjh_data_fields(void);
const char* mjh_data_extra_fields(void); /* ... of the input-only leaves that trail mjhData (MJH_DATA_EXTRA_IN) */
int mjh_sizeof_data(void);               /* sizeof(mjhData) as the library was built */
const char* mjh_model_fields(void);
int mjh_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MJHIP_H_ */
