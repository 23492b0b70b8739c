/*
 * a1mpc.h -- C ABI of the MI355X batched convex-MPC QP engine (liba1mpc.so).
 *
 * Drop-in boundary for the ONE hot path of ShuoYangRobotics/A1-QP-MPC-Controller: QP formation +
 * OSQP solve inside A1RobotControl::compute_grf.  Citations are reference file:line with
 * S/ = src/a1_cpp/src/.  The reference has no FFI; the C++ call sites this ABI replaces are
 *
 *   a1mpc_config                <- compile-time dims S/A1Params.h:26-34, ConvexMpc ctor constants
 *                                  S/ConvexMpc.cpp:8-44,223-224, A1CtrlStates fields S/A1CtrlStates.h:358-366,
 *                                  mpc_dt S/A1RobotControl.cpp:462, OSQP settings S/A1RobotControl.cpp:523-524
 *   a1mpc_create / _destroy     <- `OsqpEigen::Solver solver` member (S/A1RobotControl.h:67) + per-tick
 *                                  `ConvexMpc mpc_solver(q, r); reset()` (S/A1RobotControl.cpp:447-448)
 *   a1mpc_solve_batch           <- MPC branch of compute_grf, S/A1RobotControl.cpp:446-562:
 *                                  calculate_A_mat_c / calculate_B_mat_c / state_space_discretization /
 *                                  calculate_qp_mats (S/ConvexMpc.cpp:110-260), solver.update*()/solve()
 *                                  (:522-540), R' * solution[0:12] (:555-561)          -- n ticks at once
 *   a1mpc_balance_solve_batch   <- balance-QP branch of compute_grf, S/A1RobotControl.cpp:377-444 (+ ctor :11-48)
 *   a1mpc_reset_warm_start      <- destroying / re-creating the persistent OSQP workspace
 *
 * Plain pointers and sizes only.  All matrices use the reference's (Eigen) storage: 3x4 GRF / foot
 * matrices are column-major (leg-major, 12 doubles), root_rot_mat is passed ROW-major (9 doubles).
 * Streams: the *_device entry points launch on the stream the caller passes (NULL = the handle's own).  The handle owns scratch that
 * every launch uses, so consecutive calls on DIFFERENT streams are ordered by the library (the later call waits on the device for the
 * earlier one; calls on the same stream are ordered by the stream) -- a handle never runs two launches concurrently; use one handle
 * per stream for that.
 * Caller owns every host array (pageable is fine; the library snapshots inputs at entry because the
 * surrounding control program mutates A1CtrlStates without locks, S/MainGazebo.cpp:47-121).  A handle is
 * used by one thread at a time (the reference's thread 1); different handles are independent.
 * Nothing throws across this boundary.  There is NO CPU fallback: without a working HIP device every
 * entry point returns an error.
 */
#ifndef A1MPC_H_
#define A1MPC_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define A1MPC_STATE_DIM 13      /* MPC_STATE_DIM      S/A1Params.h:27 */
#define A1MPC_NUM_DOF 12        /* NUM_DOF            S/A1Params.h:34 */
#define A1MPC_CONSTRAINT_DIM 20 /* MPC_CONSTRAINT_DIM S/A1Params.h:28 */
#define A1MPC_NUM_LEG 4         /* NUM_LEG            S/A1Params.h:31 */

typedef enum a1mpc_status {
    A1MPC_OK = 0,
    A1MPC_ERR_INVALID_ARGUMENT = 1,
    A1MPC_ERR_UNSUPPORTED_HORIZON = 2, /* horizons compiled in: 1, 4, 6, 8, 10, 12, 14, 16, 20 (a1mpc_config.horizon) */
    A1MPC_ERR_NO_DEVICE = 3,
    A1MPC_ERR_HIP = 4,
    A1MPC_ERR_BATCH_TOO_LARGE = 5
} a1mpc_status;

/* per-problem solver status written to status_out[] -- OSQP's numbering, which the reference ignores
 * (S/A1RobotControl.cpp:540); on A1MPC_QP_NON_CVX the GRFs are zeros (replaces the reference's
 * uninitialised-matrix behaviour, S/A1RobotControl.cpp:322,559) */
#define A1MPC_QP_SOLVED 1
#define A1MPC_QP_SOLVED_INACCURATE 2
#define A1MPC_QP_MAX_ITER_REACHED (-2)
#define A1MPC_QP_NON_CVX (-7)
/* OSQP's other outcomes -- PRIMAL_INFEASIBLE (-3), PRIMAL_INFEASIBLE_INACCURATE (3), DUAL_INFEASIBLE (-4), DUAL_INFEASIBLE_INACCURATE (4) -- are UNREACHABLE here by
 * construction, and the kernels do not evaluate OSQP's infeasibility certificates (auxil.c is_primal_infeasible / is_dual_infeasible):
 *   * every configuration on which they could fire is refused with A1MPC_ERR_INVALID_ARGUMENT by a1mpc_create / a1mpc_update_config / a1mpc_sharded_create /
 *     a1mpc_pipeline_create (and the balance-QP constants by a1mpc_balance_solve_batch): mu < 0, fz_min > fz_max, fz_max < 0, a negative or non-finite weight,
 *     mass / dt <= 0, a singular body inertia, and every OSQP setting osqp_setup itself refuses (auxil.c validate_settings: rho, sigma <= 0, alpha outside (0, 2),
 *     negative tolerances, ...).  OSQP refuses the same data in osqp_setup (validate_data: l <= u); the reference ignores that return code
 *     (S/A1RobotControl.cpp:532,540) and goes on to read an uninitialised solution (:559) -- a deliberate deviation: the bad configuration is reported where it is given.
 *   * on every accepted configuration the per-problem inputs (states, feet, contacts) cannot make the QP infeasible or unbounded: the bounds come from the
 *     configuration and the contact flags only, (0, 0, max(fz_min, 0) c) is always feasible, the feasible set is compact and P = B'QB + R is positive semi-definite.
 * Non-finite INPUTS surface as A1MPC_QP_NON_CVX + zero forces (OSQP: a NaN residual ends the solve as OSQP_NON_CVX). */

typedef struct a1mpc_config {
    int32_t horizon; /* PLAN_HORIZON (S/A1Params.h:26 fixes 10; a run-time value here).  1, 10, 16, 20: the tuned horizons (the balance-QP analogue, the reference's own,
                        BASELINE's h = 16 / 20 configurations).  4, 6, 8, 12, 14: the same kernel families -- fast path and general path -- as they instantiate for them
                        (every entry point: all warm-start modes, contact schedules, tick records, per-step feet / yaw_A, pipelines, sharding), not tuned beyond that.  Anything
                        else -- odd horizons, 2, 18, > 20 -- is refused by a1mpc_create with A1MPC_ERR_UNSUPPORTED_HORIZON */
    double dt;       /* mpc_dt, S/A1RobotControl.cpp:462 */
    double mu;       /* S/ConvexMpc.cpp:8 */
    double fz_min;   /* S/ConvexMpc.cpp:223 */
    double fz_max;   /* S/ConvexMpc.cpp:224 */
    double q[A1MPC_STATE_DIM]; /* q_weights, S/A1CtrlStates.h:365 */
    double r[A1MPC_NUM_DOF];   /* r_weights, S/A1CtrlStates.h:366 */
    double mass;               /* robot_mass, S/A1CtrlStates.h:358 */
    double inertia_body[9];    /* a1_trunk_inertia, row-major, S/A1CtrlStates.h:359-360 */
    /* OSQP 0.6 settings; the reference only sets verbosity and warm start, everything else is the default */
    double rho, sigma, alpha, eps_abs, eps_rel, adaptive_rho_tolerance;
    int32_t max_iter;
    int32_t check_termination;     /* iterations between termination checks (25) */
    int32_t adaptive_rho;          /* 1 */
    int32_t adaptive_rho_interval; /* > 0: rho is re-estimated every that many iterations.  0 = OSQP's default "automatic", the
                                      setting the reference runs with: OSQP derives the period from measured wall-clock set-up time
                                      (non-reproducible); here 0 resolves deterministically to the outcome of OSQP's rule for these QP
                                      sizes, max(check_termination, 25-multiple) = check_termination (25).  a1mpc_default_config: 25 */
    int32_t scaling;               /* Ruiz passes (10) */
    int32_t warm_start;            /* 0: cold start every solve (the reference's balance-QP path and S/test/test_mpc.cpp).
                                      1: every tick is a fresh OSQP set-up warm-started from the previous tick's (x, y, rho) as osqp_warm_start defines it.
                                      2: the reference's UPDATE path on ticks >= 2 (S/A1RobotControl.cpp:533-538: updateHessianMatrix / updateGradient /
                                         update*Bound on the persistent OsqpEigen workspace, then solve()): OSQP re-equilibrates with the PREVIOUS tick's
                                         gradient still in the workspace and starts from the previous solve's SCALED (x, z, y) as they are.  The handle then
                                         also carries the previous scalings, gradient and z of every problem.  Restated from OSQP 0.6's update functions
                                         (oracle: orc_mpc_solve_update); every horizon > 1, on the fast path and on (round 5; round 6: at every batch size) the general
                                         path (per-step feet / contact schedules / its own A_c yaw: a1mpc_solve_batch_strided).  Horizon 1 (the balance QP, which the
                                         reference cold-starts anyway) behaves like 1: a1mpc_last_warm_start_mode reports which semantics a solve actually ran.
                                         When the sparsity pattern of the reference's Hessian (dense.sparseView(), S/ConvexMpc.cpp:211: exact zeros are not stored)
                                         changes from one tick to the next, osqp-eigen cannot take osqp_update_P: updateHessianMatrix clears the solver, initialises
                                         it again (rho back to cfg.rho, fresh scaling) and warm-starts it with the workspace's scaled iterates -- reproduced per
                                         problem.  The decision is the same on both paths and across a switch between them: an entry of the dense Hessian is
                                         stored exactly when a state row with a non-zero weight meets both of its columns of B_qp, so the entries are compared
                                         as that rule gives them -- a zero of B~ that appears or vanishes under a zero weight, or where another weighted row
                                         keeps the entry, is no change (tests/test_gpu_update_reinit.py, tests/test_update_reinit_host.py).  A tick solved
                                         in another mode or through the general path's split pipeline drops the carried workspace: the next tick is a fresh set-up
                                         warm-started from (x, y, rho).  (An a1mpc_warm_start injection does NOT drop it since round 4: see there.) */
} a1mpc_config;

/* balance-QP constants, A1RobotControl ctor S/A1RobotControl.cpp:11-15 */
typedef struct a1mpc_balance_config {
    double Q[6];         /* diag(1,1,1,400,400,100) */
    double R;            /* 1e-3 */
    double mu;           /* 0.7 */
    double F_min, F_max; /* 0, 180 */
} a1mpc_balance_config;

typedef struct a1mpc_handle_s* a1mpc_handle;

/* Reference constants (mu 0.3, fz in [0,180], dt 0.0025, horizon 10), OSQP defaults, warm start on;
 * q, r, mass, inertia are left zero for the caller (they come from the rosparam YAML). */
void a1mpc_default_config(a1mpc_config* cfg);
void a1mpc_default_balance_config(a1mpc_balance_config* cfg);

/* device: HIP device ordinal (>= 0).  max_batch: largest n any later call will pass.  The configuration is validated first (see the status
 * values above for what is refused and why): A1MPC_ERR_INVALID_ARGUMENT + a1mpc_last_error() naming the field, whether or not a GPU is present. */
a1mpc_status a1mpc_create(const a1mpc_config* cfg, int32_t max_batch, int32_t device, a1mpc_handle* out);
void a1mpc_destroy(a1mpc_handle h);

/*
 * n independent MPC ticks.  Host pointers.
 *   x0      n x 13   mpc_states                    (S/A1RobotControl.cpp:452-456)
 *   x_ref   n x 13H  mpc_states_d                  (S/A1RobotControl.cpp:470-488)
 *   R_world n x 9    root_rot_mat, row-major
 *   foot    n x 12   foot_pos_abs, 3x4 column-major (same feet for all H steps, S/A1RobotControl.cpp:498-514)
 *   contact n x 4    contacts[], broadcast over the horizon (S/ConvexMpc.cpp:228-245)
 * out:
 *   grf_body_out n x 12  3x4 column-major, body frame (the value compute_grf returns)
 *   u_full_out   n x 12H world-frame forces of every horizon step, or NULL
 *   iters_out, status_out  n each, or NULL
 * With cfg.warm_start the handle keeps (x, y, rho) of problem i between calls, like the reference's
 * persistent OSQP workspace.
 * A handful of QPs (n <= 8: the reference's own call is n = 1) are read from and written to the handle's pinned block by the
 * kernel itself, and the call returns as soon as the last output word has arrived (polled; round 6) -- the handle's stream may
 * still be retiring the launch for a few microseconds, which later calls and every a1mpc_last_* query order themselves behind.
 */
a1mpc_status a1mpc_solve_batch(a1mpc_handle h, int32_t n, const double* x0, const double* x_ref, const double* R_world,
                               const double* foot_abs, const uint8_t* contact, double* grf_body_out, double* u_full_out,
                               int32_t* iters_out, int32_t* status_out);

/* Same, but every pointer is DEVICE memory of the handle's device and the launch is asynchronous on
 * `hip_stream` (a hipStream_t, NULL = the handle's own stream).  No host synchronisation. */
a1mpc_status a1mpc_solve_batch_device(a1mpc_handle h, int32_t n, const double* d_x0, const double* d_x_ref,
                                      const double* d_R_world, const double* d_foot_abs, const uint8_t* d_contact,
                                      double* d_grf_body_out, double* d_u_full_out, int32_t* d_iters_out,
                                      int32_t* d_status_out, void* hip_stream);

/*
 * The general case of the reference's ConvexMpc INTERFACE: a different B_d at every horizon step (public member B_mat_d_list,
 * S/ConvexMpc.h:74, filled per step by S/test/test_mpc.cpp:106-122 -- feet shifted by root_lin_vel_d * dt -- and by the commented
 * lines S/A1RobotControl.cpp:504-507) and a per-step contact schedule (a superset: calculate_qp_mats broadcasts the current contacts,
 * S/ConvexMpc.cpp:228-245).
 *   foot_stride    0: foot is n x 12, the same feet at every step       12: foot is n x 12H, step t of problem i at foot[(i*H + t)*12]
 *   contact_stride 0: contact is n x 4, broadcast over the horizon       4: contact is n x 4H, step t of problem i at contact[(i*H + t)*4]
 *   yaw_A          NULL: A_c is built from mpc_states[2] (S/A1RobotControl.cpp:452,492)      else n yaws, one per problem
 *                  (calculate_A_mat_c takes its own euler argument, S/ConvexMpc.h:28; S/test/test_mpc.cpp:94-104 passes an average)
 * Everything else as a1mpc_solve_batch.  (0, 0, NULL) IS a1mpc_solve_batch (same kernels, same bits).  (0, 4, NULL) -- a gait schedule over the
 * horizon with step-invariant feet, the case a controller with a contact plan has -- also runs the fast kernels at their speed: contacts only
 * change the bounds and which rows are equalities (any horizon a1mpc_create accepts).  Per-step feet and / or a yaw_A run the general kernels:
 * same OSQP iterates as the reference's formation with those inputs, with a bigger LDS image per QP (B~_t of every step), i.e.
 * fewer QPs in flight -- 1.7-2.5x slower by design (round 6; with two batches in flight 3.6 M / 1.5 M / 1.07 M first solves/s at 4096 x h10 / 8192 x h16 / 8192 x h20).
 * Every horizon > 1 that a1mpc_create accepts (10, 16, 20 tuned; 4, 6, 8, 12, 14 as the kernels instantiate).
 */
a1mpc_status a1mpc_solve_batch_strided(a1mpc_handle h, int32_t n, const double* x0, const double* x_ref, const double* R_world,
                                       const double* foot_abs, int32_t foot_stride, const uint8_t* contact, int32_t contact_stride,
                                       const double* yaw_A, double* grf_body_out, double* u_full_out, int32_t* iters_out,
                                       int32_t* status_out);
a1mpc_status a1mpc_solve_batch_strided_device(a1mpc_handle h, int32_t n, const double* d_x0, const double* d_x_ref,
                                              const double* d_R_world, const double* d_foot_abs, int32_t foot_stride,
                                              const uint8_t* d_contact, int32_t contact_stride, const double* d_yaw_A,
                                              double* d_grf_body_out, double* d_u_full_out, int32_t* d_iters_out,
                                              int32_t* d_status_out, void* hip_stream);

/*
 * N1 (the caller side of the path, S/A1RobotControl.cpp:452-488): the same solve from the COMPACT tick record; x0 (mpc_states)
 * and x_ref (mpc_states_d) are built on the device exactly as compute_grf builds them.  tick is n x 22 doubles:
 *   [0:3] root_euler  [3:6] root_pos  [6:9] root_ang_vel  [9:12] root_lin_vel          (world frame, as in mpc_states)
 *   [12:15] root_euler_d  [15:18] root_lin_vel_d (BODY frame; rotated by R_world as at :470)  [18:21] root_ang_vel_d  [21] root_pos_d[2]
 * Input per QP drops from (13 + 13H) to 22 doubles.  Host pointers; a1mpc_solve_batch_ticks_device takes device pointers + a stream.
 * A handful of ticks (n <= 8; the drop-in's compute_grf is n = 1) take the pinned-block path of a1mpc_solve_batch (see there).
 */
a1mpc_status a1mpc_solve_batch_ticks(a1mpc_handle h, int32_t n, const double* tick, const double* R_world, const double* foot_abs,
                                     const uint8_t* contact, double* grf_body_out, double* u_full_out, int32_t* iters_out,
                                     int32_t* status_out);
a1mpc_status a1mpc_solve_batch_ticks_device(a1mpc_handle h, int32_t n, const double* d_tick, const double* d_R_world,
                                            const double* d_foot_abs, const uint8_t* d_contact, double* d_grf_body_out,
                                            double* d_u_full_out, int32_t* d_iters_out, int32_t* d_status_out, void* hip_stream);

/*
 * n independent balance-QP ticks (12 variables, 20 constraints), cold-started like the reference.
 *   root_acc n x 6   desired wrench incl. m*9.8 (S/A1RobotControl.cpp:379-391)
 *   R_world  n x 9   root_rot_mat (output rotation), R_z n x 9 root_rot_mat_z (lever arms, :397), row-major
 *   foot     n x 12, contact n x 4
 * The handle's horizon is irrelevant for this call; its OSQP settings are used with warm_start forced off.
 */
a1mpc_status a1mpc_balance_solve_batch(a1mpc_handle h, const a1mpc_balance_config* qp, int32_t n, const double* root_acc,
                                       const double* R_world, const double* R_z, const double* foot_abs,
                                       const uint8_t* contact, double* grf_body_out, double* f_world_out,
                                       int32_t* iters_out, int32_t* status_out);

/*
 * N2a (the caller side of the path): A1RobotControl::update_plan, S/A1RobotControl.cpp:148-202, for n robots -- gait counters,
 * planned contacts and the Raibert foothold.  Element-wise, HBM-bound; results are bit-identical to the reference arithmetic.
 *   movement_mode      n          0 = stand (all feet planned in contact, counters reset), 1 = walk
 *   gait_counter       n x 4      in/out
 *   gait_counter_speed n x 4
 *   root_lin_vel n x 3 (world), R_z n x 9 (root_rot_mat_z), R_world n x 9 (root_rot_mat), root_pos n x 3, root_lin_vel_d n x 3 (body)
 * out: plan_contacts n x 4, foot_pos_target_rel / _abs / _world n x 12 each (3x4 column-major); any of the three may be NULL.
 * Host pointers.
 */
typedef struct a1mpc_gait_config {
    double counter_per_gait, counter_per_swing; /* S/A1CtrlStates.h:24-25 */
    double control_dt;                          /* S/A1CtrlStates.h:332 */
    double foot_delta_x_limit, foot_delta_y_limit; /* S/A1Params.h:44-45 */
    double default_foot_pos[12];                /* 3x4 column-major, S/A1CtrlStates.h:45 */
    double gait_counter_reset[4];               /* S/A1CtrlStates.h:322-326 */
} a1mpc_gait_config;
void a1mpc_default_gait_config(a1mpc_gait_config* cfg);
a1mpc_status a1mpc_update_plan_batch(a1mpc_handle h, const a1mpc_gait_config* gait, int32_t n, const uint8_t* movement_mode,
                                     double* gait_counter, const double* gait_counter_speed, const double* root_lin_vel,
                                     const double* R_z, const double* R_world, const double* root_pos, const double* root_lin_vel_d,
                                     uint8_t* plan_contacts_out, double* foot_pos_target_rel_out, double* foot_pos_target_abs_out,
                                     double* foot_pos_target_world_out);

/*
 * N3 (the step right after the path): A1RobotControl::compute_joint_torques, S/A1RobotControl.cpp:289-319, for n robots.
 *   active          n        0 while the reference's mpc_init_counter < 10 (:294): all torques zero
 *   contacts        n x 4
 *   j_foot_blocks   n x 4 x 9  the four diagonal 3x3 blocks of j_foot (S/A1CtrlStates.h), column-major each
 *   grf, f_kin      n x 12     foot_forces_grf / foot_forces_kin, 3x4 column-major
 *   km_foot         3, torques_gravity n x 12
 *   joint_torques   n x 12     in/out: NaN results keep the previous value (:314-317)
 * stance: tau = J'(-f_grf); swing: tau = J^-1 (km .* f_kin) by partial-pivot LU in Eigen's operation order.  Host pointers.
 */
a1mpc_status a1mpc_joint_torques_batch(a1mpc_handle h, int32_t n, const uint8_t* active, const uint8_t* contacts, const double* j_foot_blocks,
                                       const double* grf, const double* f_kin, const double* km_foot, const double* torques_gravity,
                                       double* joint_torques);

/*
 * N2b (caller side of the path): actual contacts, recent-contact positions and terrain pitch for n robots, one tick --
 * the contact block of generate_swing_legs_ctrl (S/A1RobotControl.cpp:256-282), compute_walking_surface (:566-582) and the
 * terrain adaptation of compute_grf (:335-376), including their MovingWindowFilters (S/utils/filter.hpp; windows 60 / 100).
 * The filter state of every robot (13 filters, early_contacts, foot_pos_recent_contact) lives on the device inside the handle,
 * indexed by the robot's position in the batch; a1mpc_reset_contact_state zeroes it (= constructing A1RobotControl).
 *   gait_counter n x 4, plan_contacts n x 4, foot_force n x 4, foot_pos_abs n x 12 (3x4 column-major), root_pos_z n
 *   root_euler_d_pitch n   in/out: overwritten with +-terrain_angle when use_terrain_adapt (:358-364)
 * out: contacts n x 4, foot_pos_recent_contact n x 12, terrain_angle n (= state.terrain_pitch_angle).  Host pointers.
 * Filter arithmetic is bit-identical to the reference's; the plane fit uses a Jacobi eigen-decomposition in place of Eigen's
 * JacobiSVD (same pseudo-inverse up to rounding), acos comes from the device math library.
 */
typedef struct a1mpc_contact_config {
    double counter_per_swing;   /* S/A1CtrlStates.h:25 */
    double foot_force_low;      /* FOOT_FORCE_LOW, S/A1Params.h:38 */
    int32_t use_terrain_adapt;  /* S/A1CtrlStates.h:22 */
} a1mpc_contact_config;
void a1mpc_default_contact_config(a1mpc_contact_config* cfg);
a1mpc_status a1mpc_contact_terrain_batch(a1mpc_handle h, const a1mpc_contact_config* cfg, int32_t n, const double* gait_counter,
                                         const uint8_t* plan_contacts, const double* foot_force, const double* foot_pos_abs,
                                         const double* root_pos_z, double* root_euler_d_pitch, uint8_t* contacts_out,
                                         double* foot_pos_recent_contact_out, double* terrain_angle_out);
a1mpc_status a1mpc_reset_contact_state(a1mpc_handle h);
/* The terrain block of compute_grf on its own (S/A1RobotControl.cpp:335-376 with compute_walking_surface :566-582) for callers that keep
 * the reference's generate_swing_legs_ctrl: foot_pos_recent_contact (n x 12, 3x4 column-major) comes from the caller's A1CtrlStates,
 * the terrain-angle filter (window 100) of robot i lives in the handle (the same state a1mpc_contact_terrain_batch uses and
 * a1mpc_reset_contact_state clears).  root_euler_d_pitch n in/out, terrain_angle_out n (= state.terrain_pitch_angle).  Host pointers. */
a1mpc_status a1mpc_terrain_batch(a1mpc_handle h, int32_t use_terrain_adapt, int32_t n, const double* foot_pos_recent_contact,
                                 const double* root_pos_z, double* root_euler_d_pitch, double* terrain_angle_out);

/*
 * N4a (caller side): swing-leg targets and the foot PD force -- the first block of generate_swing_legs_ctrl,
 * S/A1RobotControl.cpp:204-254, with the Bezier curve of S/utils/Utils.cpp:64-104 -- for n robots.
 *   R_z n x 9 (root_rot_mat_z), foot_pos_abs / foot_pos_target_rel n x 12, gait_counter n x 4, kp_foot / kd_foot 3 (per axis)
 *   foot_pos_start, foot_pos_rel_last_time, foot_pos_target_last_time n x 12  in/out (state carried by the caller)
 * out: foot_pos_cur n x 12, foot_forces_kin n x 12.  Host pointers.  Integer powers of the curve are products here (std::pow there):
 * agreement to a few ulp, everything else bit-identical arithmetic.
 */
a1mpc_status a1mpc_swing_legs_batch(a1mpc_handle h, int32_t n, double counter_per_swing, double dt, const double* R_z,
                                    const double* foot_pos_abs, const double* gait_counter, const double* foot_pos_target_rel,
                                    const double* kp_foot, const double* kd_foot, double* foot_pos_start, double* foot_pos_rel_last_time,
                                    double* foot_pos_target_last_time, double* foot_pos_cur_out, double* foot_forces_kin_out);

/*
 * N4b (caller side): leg kinematics of n robots -- the per-leg block of the joint-state callback, S/GazeboA1ROS.cpp:264-279, with
 * A1Kinematics::fk / jac (S/legKinematics/A1Kinematics.cpp) restated from the leg model (hip offset, abduction, thigh, calf).
 *   joint_pos, joint_vel n x 12; R_world n x 9; root_pos, root_lin_vel n x 3; rho_fix 4 x 5 = [ox, oy, d, lt, lc] per leg, rho_opt 4 x 3
 * out (each may be NULL except foot_pos_rel and j_foot_blocks): foot_pos_rel n x 12, j_foot_blocks n x 4 x 9 (column-major 3x3 per leg,
 * the layout a1mpc_joint_torques_batch takes), foot_vel_rel, foot_pos_abs, foot_vel_abs, foot_pos_world, foot_vel_world n x 12.
 * Host pointers.  sin / cos come from the device math library: agreement with the reference to a few ulp.
 */
a1mpc_status a1mpc_leg_state_batch(a1mpc_handle h, int32_t n, const double* joint_pos, const double* joint_vel, const double* R_world,
                                   const double* root_pos, const double* root_lin_vel, const double* rho_fix, const double* rho_opt,
                                   double* foot_pos_rel_out, double* j_foot_blocks_out, double* foot_vel_rel_out, double* foot_pos_abs_out,
                                   double* foot_vel_abs_out, double* foot_pos_world_out, double* foot_vel_world_out);

/*
 * N4c (caller side, the step before the path): A1BasicEKF, S/A1BasicEKF.cpp:7-163 -- the 18-state / 28-measurement Kalman filter that
 * provides root_pos and root_lin_vel -- for n robots, one tick.  The filter state of every robot (x 18, P 18x18, initialised flag) lives
 * on the device inside the handle; the first call for a robot performs init_state (:54-68), later calls update_estimation (:70-163), like
 * the reference's callers (S/GazeboA1ROS.cpp:194-198).  a1mpc_reset_ekf_state = constructing the filter anew.
 *   movement_mode n, foot_force n x 4, R_world n x 9, imu_acc n x 3, imu_ang_vel n x 3, foot_pos_rel / foot_vel_rel n x 12
 * out: root_pos n x 3, root_lin_vel n x 3, estimated_contacts n x 4.  Host pointers.
 * The two fullPivHouseholderQr solves with S are one Gauss-Jordan elimination of [S | error_y | C] here (S is symmetric positive definite).
 */
a1mpc_status a1mpc_ekf_update_batch(a1mpc_handle h, int32_t n, double dt, int32_t assume_flat_ground, const uint8_t* movement_mode,
                                    const double* foot_force, const double* R_world, const double* imu_acc, const double* imu_ang_vel,
                                    const double* foot_pos_rel, const double* foot_vel_rel, double* root_pos_out, double* root_lin_vel_out,
                                    uint8_t* estimated_contacts_out);
a1mpc_status a1mpc_reset_ekf_state(a1mpc_handle h);

/*
 * Device-pointer variants of the caller-side entry points above: every array argument is a device pointer (the small per-call constant
 * arrays kp / kd / km / rho_fix / rho_opt stay host pointers, they travel as kernel arguments), the call is asynchronous on `hip_stream`
 * (NULL = the handle's stream).  Together with a1mpc_solve_batch_ticks_device a whole control tick chains on the GPU without a PCIe hop.
 */
a1mpc_status a1mpc_update_plan_batch_device(a1mpc_handle h, const a1mpc_gait_config* gait, int32_t n, const uint8_t* d_movement_mode,
                                            double* d_gait_counter, const double* d_gait_counter_speed, const double* d_root_lin_vel,
                                            const double* d_R_z, const double* d_R_world, const double* d_root_pos, const double* d_root_lin_vel_d,
                                            uint8_t* d_plan_contacts_out, double* d_rel_out, double* d_abs_out, double* d_world_out, void* hip_stream);
a1mpc_status a1mpc_swing_legs_batch_device(a1mpc_handle h, int32_t n, double counter_per_swing, double dt, const double* d_R_z,
                                           const double* d_foot_pos_abs, const double* d_gait_counter, const double* d_foot_pos_target_rel,
                                           const double* kp_foot, const double* kd_foot, double* d_foot_pos_start, double* d_foot_pos_rel_last_time,
                                           double* d_foot_pos_target_last_time, double* d_foot_pos_cur_out, double* d_foot_forces_kin_out, void* hip_stream);
a1mpc_status a1mpc_contact_terrain_batch_device(a1mpc_handle h, const a1mpc_contact_config* cfg, int32_t n, const double* d_gait_counter,
                                                const uint8_t* d_plan_contacts, const double* d_foot_force, const double* d_foot_pos_abs,
                                                const double* d_root_pos_z, double* d_root_euler_d_pitch, uint8_t* d_contacts_out,
                                                double* d_foot_pos_recent_contact_out, double* d_terrain_angle_out, void* hip_stream);
a1mpc_status a1mpc_leg_state_batch_device(a1mpc_handle h, int32_t n, const double* d_joint_pos, const double* d_joint_vel, const double* d_R_world,
                                          const double* d_root_pos, const double* d_root_lin_vel, const double* rho_fix, const double* rho_opt,
                                          double* d_foot_pos_rel_out, double* d_j_foot_blocks_out, double* d_foot_vel_rel_out, double* d_foot_pos_abs_out,
                                          double* d_foot_vel_abs_out, double* d_foot_pos_world_out, double* d_foot_vel_world_out, void* hip_stream);
a1mpc_status a1mpc_ekf_update_batch_device(a1mpc_handle h, int32_t n, double dt, int32_t assume_flat_ground, const uint8_t* d_movement_mode,
                                           const double* d_foot_force, const double* d_R_world, const double* d_imu_acc, const double* d_imu_ang_vel,
                                           const double* d_foot_pos_rel, const double* d_foot_vel_rel, double* d_root_pos_out, double* d_root_lin_vel_out,
                                           uint8_t* d_estimated_contacts_out, void* hip_stream);
a1mpc_status a1mpc_joint_torques_batch_device(a1mpc_handle h, int32_t n, const uint8_t* d_active, const uint8_t* d_contacts, const double* d_j_foot_blocks,
                                              const double* d_grf, const double* d_f_kin, const double* km_foot, const double* d_torques_gravity,
                                              double* d_joint_torques, void* hip_stream);

/*
 * One control tick of n robots in ONE call, device-resident (round 5; SURVEY 8(f) N1-N4 chained): what the reference runs per robot every 2.5 ms --
 *   joint-state callback: leg FK / Jacobians (S/GazeboA1ROS.cpp:264-279)  ->  A1BasicEKF::update_estimation (S/A1BasicEKF.cpp:70-163)  ->  update_plan
 *   (S/A1RobotControl.cpp:148-202)  ->  generate_swing_legs_ctrl (:204-287; its contact logic together with the terrain fit of compute_grf, :335-376, :566-582)  ->
 *   compute_grf (:446-562: state packing, reference trajectory, QP formation, OSQP)  ->  compute_joint_torques (:289-319), driven by S/MainGazebo.cpp:47-119
 * -- as six element-wise / filter kernels, a tick-record pack and the MPC launch back to back on `hip_stream` (NULL = the handle's), no host round trip.
 * compute_joint_torques (N3) runs INSIDE the MPC kernel's output stage whenever the tick goes through the fused / latency kernel (every warm-started tick of a
 * known batch, every batch of <= 256 robots): the lanes that have just written a leg's GRF evaluate tau = J'(-f) (stance) or J^-1 (km .* f_kin) (swing) for that leg;
 * otherwise (a first tick, a batch beyond the fused kernel's range) it is one more launch.  Results are bit-identical to chaining the seven *_device entry points
 * (a1mpc_leg_state_batch_device, a1mpc_ekf_update_batch_device, a1mpc_update_plan_batch_device, a1mpc_swing_legs_batch_device, a1mpc_contact_terrain_batch_device,
 * a1mpc_solve_batch_ticks_device, a1mpc_joint_torques_batch_device) with root_pos[.][2] as root_pos_z and root_euler_d[.][1] as the terrain pitch.
 * The filter states (EKF, contact / terrain windows) and the carried OSQP workspace live in the handle, indexed by the robot's position in the batch.
 */
typedef struct a1mpc_tick_params {
    a1mpc_gait_config gait;           /* update_plan + counter_per_swing of the swing legs */
    a1mpc_contact_config contact;     /* contact logic, terrain adaptation */
    double control_dt;                /* EKF dt and the swing legs' velocity dt (2.5 ms, S/A1CtrlStates.h:332) */
    int32_t assume_flat_ground;       /* A1BasicEKF ctor argument, S/A1BasicEKF.cpp:42-53 */
    double kp_foot[3], kd_foot[3];    /* swing-leg PD, per axis (S/A1CtrlStates.h: kp_foot / kd_foot) */
    double km_foot[3];                /* S/A1CtrlStates.h: km_foot */
    double rho_fix[20], rho_opt[12];  /* leg geometry: 4 x [ox, oy, d, lt, lc] and 4 x 3 (S/GazeboA1ROS.cpp:20-50) */
} a1mpc_tick_params;
typedef struct a1mpc_tick_buffers {   /* DEVICE pointers, n robots each; layouts as in the per-stage entry points above */
    /* inputs of this tick: sensors, attitude (the reference takes it from the IMU / simulator), commands */
    const double *joint_pos, *joint_vel;                 /* n x 12 */
    const double *R_world, *R_z;                         /* n x 9 row-major: root_rot_mat, root_rot_mat_z */
    const double *root_euler, *root_ang_vel;             /* n x 3 (world frame), the tick record's [0:3] and [6:9] */
    const double *imu_acc, *imu_ang_vel;                 /* n x 3 (the EKF's inputs) */
    const double* foot_force;                            /* n x 4 */
    const uint8_t* movement_mode;                        /* n */
    const uint8_t* mpc_active;                           /* n: 0 while the reference's mpc_init_counter < 10 (S/A1RobotControl.cpp:294) */
    const double *root_lin_vel_d, *root_ang_vel_d;       /* n x 3: commanded velocities (lin: body frame, rotated at S/A1RobotControl.cpp:470) */
    const double* root_pos_d_z;                          /* n: commanded body height, root_pos_d[2] */
    const double* gait_counter_speed;                    /* n x 4 */
    const double* torques_gravity;                       /* n x 12 */
    /* state carried from tick to tick by the caller (in/out) */
    double* gait_counter;                                /* n x 4 */
    double *foot_pos_start, *foot_pos_rel_last_time, *foot_pos_target_last_time;   /* n x 12 */
    double* root_euler_d;                                /* n x 3: [1] is overwritten with +-terrain_angle when use_terrain_adapt (S/A1RobotControl.cpp:358-364) */
    double* joint_torques;                               /* n x 12: NaN results keep the previous value (:314-317) */
    double *root_pos, *root_lin_vel;                     /* n x 3: the estimate (in: the previous tick's, read by the leg stage's world-frame outputs; out: this tick's) */
    /* outputs */
    uint8_t *estimated_contacts, *plan_contacts, *contacts;   /* n x 4 */
    double *foot_pos_rel, *j_foot_blocks, *foot_vel_rel, *foot_pos_abs;   /* n x 12 / n x 36 / n x 12 / n x 12 */
    double *foot_vel_abs, *foot_pos_world, *foot_vel_world;               /* n x 12, each may be NULL */
    double* foot_pos_target_rel;                                          /* n x 12 */
    double *foot_pos_target_abs, *foot_pos_target_world;                  /* n x 12, each may be NULL */
    double *foot_pos_cur, *foot_forces_kin;              /* n x 12 */
    double* foot_pos_recent_contact;                     /* n x 12 */
    double* terrain_angle;                               /* n */
    double* grf;                                         /* n x 12: foot_forces_grf, body frame */
    int32_t *iters, *status;                             /* n each, or NULL */
} a1mpc_tick_buffers;
void a1mpc_default_tick_params(a1mpc_tick_params* p);   /* the reference's Gazebo parameter set and the A1's leg geometry */
a1mpc_status a1mpc_control_tick_device(a1mpc_handle h, const a1mpc_tick_params* params, const a1mpc_tick_buffers* buffers, int32_t n, void* hip_stream);
/* duration of the handle's last a1mpc_control_tick_device on the device (HIP events around the whole tick; synchronises it) and whether its joint torques were
 * written by the MPC kernel's output stage (1) or by a launch of their own (0) */
a1mpc_status a1mpc_last_control_tick_ms(a1mpc_handle h, float* ms_out, int32_t* torques_fused_out);

/*
 * The balance-QP stance controller on the device (stance_leg_control_type 0 of the reference's rosparam sets): what compute_grf runs instead of the convex MPC,
 * S/A1RobotControl.cpp:325-332, 377-444 -- a PD wrench on the body, then the 12-variable QP of a1mpc_balance_solve_batch.
 *
 * a1mpc_balance_wrench_batch(_device): root_acc, the desired wrench (S/A1RobotControl.cpp:379-391) from the euler error with its yaw wrap at +-3.1415926 * 1.5
 * (:325-332), for n robots.  kp_linear .* (root_pos_d - root_pos) + R (kd_linear .* (root_lin_vel_d - R' root_lin_vel)) on the first three elements (+ mass * 9.8 on
 * the third, the handle's cfg.mass), kp_angular .* euler_error + kd_angular .* (root_ang_vel_d - R' root_ang_vel) on the last three.
 *   root_pos_d, root_pos n x 3; root_lin_vel_d n x 3 (body frame), root_lin_vel n x 3 (world); root_euler_d, root_euler n x 3;
 *   root_ang_vel_d n x 3 (body frame), root_ang_vel n x 3 (world); R_world n x 9 row-major (root_rot_mat)
 * out: root_acc n x 6, the layout a1mpc_balance_solve_batch takes.  Element-wise, HBM-bound (27 doubles in, 6 out per robot); IEEE add / subtract / multiply in the
 * reference's order, not contracted: bit-identical to the reference arithmetic.  A null handle, gains or array, a non-finite gain or n < 0 is
 * A1MPC_ERR_INVALID_ARGUMENT, n > max_batch A1MPC_ERR_BATCH_TOO_LARGE (a1mpc_last_error names the argument), all before any device call; n == 0 launches nothing.
 * The _device entry takes device pointers and is asynchronous on `hip_stream` (NULL = the handle's stream); the host entry stages through device memory.
 */
typedef struct a1mpc_balance_gains { double kp_linear[3], kd_linear[3], kp_angular[3], kd_angular[3]; } a1mpc_balance_gains;
void a1mpc_default_balance_gains(a1mpc_balance_gains* gains);   /* S/A1CtrlStates.h:117-120: 1000 x3 | 200, 70, 120 | 650, 35, 1 | 4.5, 4.5, 30 */
a1mpc_status a1mpc_balance_wrench_batch(a1mpc_handle h, const a1mpc_balance_gains* gains, int32_t n, const double* root_pos_d, const double* root_pos,
                                        const double* root_lin_vel_d, const double* root_lin_vel, const double* root_euler_d, const double* root_euler,
                                        const double* root_ang_vel_d, const double* root_ang_vel, const double* R_world, double* root_acc_out);
a1mpc_status a1mpc_balance_wrench_batch_device(a1mpc_handle h, const a1mpc_balance_gains* gains, int32_t n, const double* d_root_pos_d, const double* d_root_pos,
                                               const double* d_root_lin_vel_d, const double* d_root_lin_vel, const double* d_root_euler_d, const double* d_root_euler,
                                               const double* d_root_ang_vel_d, const double* d_root_ang_vel, const double* d_R_world, double* d_root_acc_out,
                                               void* hip_stream);
/* a1mpc_balance_solve_batch (S/A1RobotControl.cpp:393-444) on device pointers: asynchronous on `hip_stream` (NULL = the handle's stream), no host synchronisation and no
 * pinned small-batch block; the same validation, the same kernel launch and the same bits as the host entry.  d_f_world_out, d_iters_out, d_status_out may be NULL.
 * a1mpc_last_kernel_ms and a1mpc_last_nfact report it. */
a1mpc_status a1mpc_balance_solve_batch_device(a1mpc_handle h, const a1mpc_balance_config* qp, int32_t n, const double* d_root_acc, const double* d_R_world,
                                              const double* d_R_z, const double* d_foot_abs, const uint8_t* d_contact, double* d_grf_body_out, double* d_f_world_out,
                                              int32_t* d_iters_out, int32_t* d_status_out, void* hip_stream);
/* The contact block of generate_swing_legs_ctrl on its own (S/A1RobotControl.cpp:256-282) -- a1mpc_contact_terrain_batch without the terrain fit, which the reference
 * skips for this controller (:335, "only do terrain adaptation in MPC").  The early-contact flags and the recent-contact filters are the handle's contact state, the
 * same a1mpc_contact_terrain_batch uses and a1mpc_reset_contact_state clears; the terrain-angle filter, root_euler_d and the terrain outputs are neither read nor
 * written (cfg->use_terrain_adapt is ignored).  gait_counter n x 4, plan_contacts n x 4, foot_force n x 4, foot_pos_abs n x 12;
 * out: contacts n x 4, foot_pos_recent_contact n x 12 -- bit for bit what a1mpc_contact_terrain_batch gives. */
a1mpc_status a1mpc_contacts_batch(a1mpc_handle h, const a1mpc_contact_config* cfg, int32_t n, const double* gait_counter, const uint8_t* plan_contacts,
                                  const double* foot_force, const double* foot_pos_abs, uint8_t* contacts_out, double* foot_pos_recent_contact_out);
a1mpc_status a1mpc_contacts_batch_device(a1mpc_handle h, const a1mpc_contact_config* cfg, int32_t n, const double* d_gait_counter, const uint8_t* d_plan_contacts,
                                         const double* d_foot_force, const double* d_foot_pos_abs, uint8_t* d_contacts_out, double* d_foot_pos_recent_contact_out,
                                         void* hip_stream);
/* One control tick of n robots on the balance-QP controller in ONE call: the leg state, EKF, plan and swing-leg stages of a1mpc_control_tick_device, the contact block
 * alone, then compute_grf's type-0 branch (S/A1RobotControl.cpp:325-332, 377-444) -- the wrench from this tick's root_pos / root_lin_vel, root_euler(_d), the commanded
 * velocities and R_world, the balance QP on R_world, R_z, foot_pos_abs and contacts -- and compute_joint_torques (:289-319) as a launch of its own
 * (a1mpc_last_control_tick_ms reports this tick with torques_fused = 0), back to back on `hip_stream`, no host round trip.  Bit-identical to chaining
 * a1mpc_leg_state_batch_device, a1mpc_ekf_update_batch_device, a1mpc_update_plan_batch_device, a1mpc_swing_legs_batch_device, a1mpc_contacts_batch_device,
 * a1mpc_balance_wrench_batch_device, a1mpc_balance_solve_batch_device and a1mpc_joint_torques_batch_device.  Of a1mpc_tick_buffers, root_pos_d_z and terrain_angle are
 * not used and may be NULL, root_euler_d is read and never written; grf / iters / status are the QP's.  The handle's horizon is irrelevant; its OSQP settings are used
 * with the warm start forced off, as in a1mpc_balance_solve_batch. */
typedef struct a1mpc_balance_tick {
    a1mpc_balance_gains gains; a1mpc_balance_config qp;
    const double* root_pos_d;   /* device, n x 3 */
    double* root_acc;           /* device, n x 6 out, or NULL: a handle-owned buffer, allocated once */
    double* f_world;            /* device, n x 12 out, or NULL */
} a1mpc_balance_tick;
a1mpc_status a1mpc_control_tick_balance_device(a1mpc_handle h, const a1mpc_tick_params* params, const a1mpc_balance_tick* balance, const a1mpc_tick_buffers* buffers,
                                               int32_t n, void* hip_stream);

/* a1mpc_balance_wrench_batch(_device) with kp_linear[0:2] PER ROBOT: kp_linear_xy (n x 2) replaces gains->kp_linear[0:2], gains->kp_linear[2] and the nine other gains
 * stay the batch's.  The reference switches kp_linear(0), kp_linear(1) of every robot between 0 (walking with a velocity command: the position target follows the robot)
 * and kp_linear_lock_x / _y (S/GazeboA1ROS.cpp:172-173, 183-186) -- a1mpc_command_batch's kp_linear_xy, of which this entry is the consumer: with the batch-wide gains
 * a walking robot on the balance controller is pulled back to its lock point.  A kernel of its own around the wrench kernel's per-robot body; bit-identical to
 * a1mpc_balance_wrench_batch when every row holds gains->kp_linear[0:2].  Refusals as there, and a null kp_linear_xy. */
a1mpc_status a1mpc_balance_wrench_kp_batch(a1mpc_handle h, const a1mpc_balance_gains* gains, int32_t n, const double* kp_linear_xy, const double* root_pos_d,
                                           const double* root_pos, const double* root_lin_vel_d, const double* root_lin_vel, const double* root_euler_d,
                                           const double* root_euler, const double* root_ang_vel_d, const double* root_ang_vel, const double* R_world, double* root_acc_out);
a1mpc_status a1mpc_balance_wrench_kp_batch_device(a1mpc_handle h, const a1mpc_balance_gains* gains, int32_t n, const double* d_kp_linear_xy, const double* d_root_pos_d,
                                                  const double* d_root_pos, const double* d_root_lin_vel_d, const double* d_root_lin_vel, const double* d_root_euler_d,
                                                  const double* d_root_euler, const double* d_root_ang_vel_d, const double* d_root_ang_vel, const double* d_R_world,
                                                  double* d_root_acc_out, void* hip_stream);

/*
 * The sensor and command front end: what the reference's adapter makes of what a simulator or robot provides -- a quaternion, raw IMU samples, a stick command --
 * BEFORE the chain of a1mpc_control_tick_device starts.  The ROS publishers and subscribers of S/GazeboA1ROS.cpp stay out of scope; the arithmetic inside its
 * callbacks is a per-robot function of arrays, and is this.
 *
 * a1mpc_sensor_frontend_batch(_device), n robots:
 *   in   quat n x 4 (w, x, y, z; NOT normalised, as in the reference), imu_acc_raw n x 3, imu_gyro_raw n x 3
 *   out  R_world n x 9 row-major = root_quat.toRotationMatrix() (gt_pose_callback, S/GazeboA1ROS.cpp:258; Eigen's operation order: tx = 2x, twx = tx * w, ...,
 *        R00 = 1 - (tyy + tzz)); root_euler n x 3 = Utils::quat_to_euler (:259, S/utils/Utils.cpp:7-33, the clamp of t2 included); R_z n x 9 =
 *        AngleAxisd(yaw, UnitZ) as a matrix (:262); imu_acc, imu_ang_vel n x 3 = the six MovingWindowFilter(5) of imu_callback (:289-298, S/utils/filter.hpp:26-62:
 *        Neumaier sums, divided by the window length from the first sample on); root_ang_vel n x 3 = R_world * imu_ang_vel (:299) on this call's matrix and filtered
 *        value, every row sum of three terms left to right.
 *   Not contracted: everything except atan2, asin, sin and cos is the reference's arithmetic bit for bit (those four are the device library's, their arguments
 *   bit-identical).  ONE UNPINNED CHOICE: R_z follows Eigen's AngleAxis::toRotationMatrix as published (sin_axis = s * axis, cos1_axis = (1 - c) * axis, the
 *   off-diagonal pairs tmp -+ sin_axis, the diagonal cos1_axis .* axis + c -- element (2,2) is (1 - c) + c, not a literal 1); no Eigen is at hand where this
 *   project is built to pin that order against, the two rotation matrices are held to a restatement written from Eigen's source text (tests/frontend_ref.py).
 *   The filter state lives in the handle, indexed by the robot's position in the batch, allocated on first use; a1mpc_reset_sensor_state clears it (= constructing
 *   the adapter).  cfg->imu_window runs from 1 to 64 (A1MPC_IMU_WINDOW_MAX); a window other than the one the state was built with, without a reset in between, is
 *   A1MPC_ERR_INVALID_ARGUMENT.
 *
 * a1mpc_command_batch(_device): the first half of main_update, S/GazeboA1ROS.cpp:124-188, branch for branch, and the gate of compute_joint_torques
 * (S/A1RobotControl.cpp:292-294).
 *   in   cmd n x 6 = joy_cmd_velx, vely, velz, roll_rate, pitch_rate, yaw_rate after joy_callback's scaling (the axis mapping differs between the Gazebo and the
 *        hardware adapter and stays with the caller); mode_toggle n (joy_cmd_ctrl_state_change_request); root_pos n x 3 (the previous tick's estimate); dt
 *   in/out, carried by the caller like gait_counter (A1CtrlStates / adapter members): body_height n (joy_cmd_body_height, initially 0.3, S/GazeboA1ROS.h:130),
 *        ctrl_state n (joy_cmd_ctrl_state), root_euler_d n x 3, root_pos_d n x 3, kp_linear_xy n x 2 (kp_linear(0), kp_linear(1)), mpc_init_counter n
 *   out  root_lin_vel_d, root_ang_vel_d n x 3; movement_mode n; mpc_active n: 1 from the call on which the incremented counter reaches mpc_init_ticks;
 *        root_pos_d_z n: the contiguous copy of root_pos_d[.][2] the tick takes
 *   body_height += velz * dt (the product rounded first), clamped with >= max / <= min (:124-130); the toggle (:142-147); root_euler_d += rate * dt (:158-160);
 *   movement_mode 1 in state 1; on the ONE tick that leaves state 1 the xy target is locked to root_pos and kp_linear_xy set to the lock values (:167-173); otherwise
 *   (:174-176) kp_linear_xy is left as it is; in mode 1, sqrt(vx * vx + vy * vy) > lock_speed refreshes the xy target and zeroes kp_linear_xy, else the lock values (:179-188).
 *
 * Both: a null handle, config or array, a non-finite config value or dt, body_height_min > body_height_max, a window out of range or n < 0 is
 * A1MPC_ERR_INVALID_ARGUMENT (a1mpc_last_error names the argument), n > max_batch A1MPC_ERR_BATCH_TOO_LARGE, all before any device call; n == 0 launches nothing.  The
 * _device entries take device pointers and are asynchronous on `hip_stream` (NULL = the handle's stream); the host entries stage through device memory.
 */
#define A1MPC_IMU_WINDOW_MAX 64
typedef struct a1mpc_sensor_config { int32_t imu_window; } a1mpc_sensor_config;   /* default 5, S/GazeboA1ROS.cpp:99-104 */
typedef struct a1mpc_command_config {
    double body_height_max, body_height_min;      /* 0.32, 0.1: JOY_CMD_BODY_HEIGHT_MAX / _MIN, S/A1Params.h:16-17 */
    double kp_linear_lock_x, kp_linear_lock_y;    /* 120, 120: S/A1CtrlStates.h:273-274, 298-299 */
    double lock_speed;                            /* 0.05: S/GazeboA1ROS.cpp:180 */
    int32_t mpc_init_ticks;                       /* 10: S/A1RobotControl.cpp:294 */
} a1mpc_command_config;
void a1mpc_default_sensor_config(a1mpc_sensor_config* cfg);
void a1mpc_default_command_config(a1mpc_command_config* cfg);
a1mpc_status a1mpc_reset_sensor_state(a1mpc_handle h);
a1mpc_status a1mpc_sensor_frontend_batch(a1mpc_handle h, const a1mpc_sensor_config* cfg, int32_t n, const double* quat, const double* imu_acc_raw, const double* imu_gyro_raw,
                                         double* R_world_out, double* R_z_out, double* root_euler_out, double* imu_acc_out, double* imu_ang_vel_out, double* root_ang_vel_out);
a1mpc_status a1mpc_sensor_frontend_batch_device(a1mpc_handle h, const a1mpc_sensor_config* cfg, int32_t n, const double* d_quat, const double* d_imu_acc_raw,
                                                const double* d_imu_gyro_raw, double* d_R_world_out, double* d_R_z_out, double* d_root_euler_out, double* d_imu_acc_out,
                                                double* d_imu_ang_vel_out, double* d_root_ang_vel_out, void* hip_stream);
a1mpc_status a1mpc_command_batch(a1mpc_handle h, const a1mpc_command_config* cfg, int32_t n, const double* cmd, const uint8_t* mode_toggle, const double* root_pos, double dt,
                                 double* body_height, uint8_t* ctrl_state, double* root_euler_d, double* root_pos_d, double* kp_linear_xy, int32_t* mpc_init_counter,
                                 double* root_lin_vel_d_out, double* root_ang_vel_d_out, uint8_t* movement_mode_out, uint8_t* mpc_active_out, double* root_pos_d_z_out);
a1mpc_status a1mpc_command_batch_device(a1mpc_handle h, const a1mpc_command_config* cfg, int32_t n, const double* d_cmd, const uint8_t* d_mode_toggle, const double* d_root_pos,
                                        double dt, double* d_body_height, uint8_t* d_ctrl_state, double* d_root_euler_d, double* d_root_pos_d, double* d_kp_linear_xy,
                                        int32_t* d_mpc_init_counter, double* d_root_lin_vel_d_out, double* d_root_ang_vel_d_out, uint8_t* d_movement_mode_out,
                                        uint8_t* d_mpc_active_out, double* d_root_pos_d_z_out, void* hip_stream);
/* The control tick from RAW inputs in one call: the sensor stage, the command stage (dt = params->control_dt, root_pos = buffers->root_pos, root_euler_d =
 * buffers->root_euler_d), then exactly a1mpc_control_tick_device, back to back on `hip_stream` with no host round trip; bit-identical to calling
 * a1mpc_sensor_frontend_batch_device, a1mpc_command_batch_device and a1mpc_control_tick_device by hand.  Of a1mpc_tick_buffers, ELEVEN input fields become outputs of
 * the call -- R_world, R_z, root_euler, root_ang_vel, imu_acc, imu_ang_vel, movement_mode, mpc_active, root_lin_vel_d, root_ang_vel_d, root_pos_d_z: the caller
 * supplies the storage, the front end writes it, the tick reads it -- and root_euler_d is integrated by the command stage before the terrain stage overwrites its
 * pitch.  Every refusal of the three entries is made before the first launch.  a1mpc_last_control_tick_ms reports the tick behind the front end.
 * Out of scope: the preview / foothold ticks, and the balance tick (which would also need a1mpc_balance_wrench_kp_batch inside it). */
typedef struct a1mpc_tick_sensors {   /* DEVICE pointers, n robots each */
    a1mpc_sensor_config sensor; a1mpc_command_config command;
    const double *quat, *imu_acc_raw, *imu_gyro_raw;   /* n x 4, n x 3, n x 3 */
    const double* cmd;                                 /* n x 6 */
    const uint8_t* mode_toggle;                        /* n */
    double* body_height;                               /* in/out from here on: n */
    uint8_t* ctrl_state;                               /* n */
    double *root_pos_d, *kp_linear_xy;                 /* n x 3, n x 2 */
    int32_t* mpc_init_counter;                         /* n */
} a1mpc_tick_sensors;
a1mpc_status a1mpc_control_tick_sensors_device(a1mpc_handle h, const a1mpc_tick_params* params, const a1mpc_tick_sensors* sensors, const a1mpc_tick_buffers* buffers,
                                               int32_t n, void* hip_stream);

/*
 * Gait-aware horizon: the device-side PRODUCER of the two inputs a1mpc_solve_batch_strided takes beyond the reference controller's -- a contact schedule over the
 * horizon and per-step feet -- from the state a control tick already holds on the device (gait counters, contacts, feet, the velocity command).
 * NOT the reference controller's behaviour unless switched off: calculate_qp_mats broadcasts the current contacts[] over all H steps (S/ConvexMpc.cpp:228-245) and
 * compute_grf passes the current feet at every step (S/A1RobotControl.cpp:498-514; the per-step shift is commented out there, :496,:504-507).  What IS the
 * reference's: the counter rule that is run forward (update_plan, S/A1RobotControl.cpp:156-164), the per-step interface that takes the result (B_mat_d_list,
 * S/ConvexMpc.h:74) and the foot recurrence (S/test/test_mpc.cpp:105-122, S/A1RobotControl.cpp:504-507).
 *   contact_schedule  0: no schedule is produced; the solve broadcasts contacts[] (the reference).
 *                     1: step 0 = the robot's ACTUAL contacts[] (planned or early contact, S/A1RobotControl.cpp:271 -- the value the reference broadcasts); step t >= 1 =
 *                        update_plan's rule run forward from the CURRENT gait_counter (already advanced by this tick's update_plan): t * ticks_per_step times
 *                        c = fmod(c + speed, counter_per_gait), then contact = (c <= counter_per_swing) (:158-164).  The update is iterated, not a closed form, so step t
 *                        is bit for bit the plan_contacts update_plan itself produces t * ticks_per_step ticks later at constant speed.  movement_mode == 0: every
 *                        step is 1 (:150-153).  Early contacts and the foot-force test (:256-282) are not predicted: beyond step 0 the schedule is the PLAN.
 *   foot_preview      0: no per-step feet are produced; the solve uses the current feet at every step (the reference controller).
 *                     1: the reference's lines as written: f_0 = foot_pos_abs, f_(t+1) = f_t - root_lin_vel_d * dt with root_lin_vel_d the BODY-frame command exactly
 *                        as S/test/test_mpc.cpp:112-115 and S/A1RobotControl.cpp:504-507 have it, dt = the handle's cfg.dt.
 *                     2: the same recurrence with R_world * root_lin_vel_d, the world-frame command root_lin_vel_d_world of S/A1RobotControl.cpp:470 -- foot_pos_abs is
 *                        world-aligned, so this is the physically consistent variant (not in the reference).
 *                     The product is rounded first and then subtracted (no FMA contraction): bit-identical to the C++ loop.
 *   ticks_per_step    1..64: control ticks per horizon step (mpc_dt / control period).  The reference runs 1: mpc_dt equals the control period (S/A1RobotControl.cpp:462).
 * a1mpc_default_preview_config: {1, 0, 1}.
 */
typedef struct a1mpc_preview_config {
    int32_t contact_schedule;  /* 0: broadcast contacts (the reference), 1: gait-predicted schedule */
    int32_t foot_preview;      /* 0 / 1 / 2 as above */
    int32_t ticks_per_step;    /* 1..64 */
} a1mpc_preview_config;
void a1mpc_default_preview_config(a1mpc_preview_config* cfg);
/*
 * The preview on its own, n robots, horizon H = the handle's (>= 2).  Of `gait` only counter_per_gait (> 0) and counter_per_swing are read.
 *   movement_mode n, gait_counter n x 4, gait_counter_speed n x 4, contacts n x 4, foot_pos_abs n x 12 (3x4 column-major), R_world n x 9 (row-major; read by
 *   foot_preview 2 only, may be NULL otherwise), root_lin_vel_d n x 3 (body frame)
 * out: contact_sched_out n x 4H bytes, step t of robot i at [(i*H + t)*4]; foot_steps_out n x 12H doubles, step t of robot i at [(i*H + t)*12] -- the layouts
 * a1mpc_solve_batch_strided takes with contact_stride = 4 / foot_stride = 12.  Either may be NULL (not produced).  With contact_schedule 0 a schedule that is asked for is
 * contacts[] at every step, the reference's broadcast written out (same solve as contact_stride = 0); the feet need foot_preview 1 or 2.  The inputs of an output
 * that is not produced may be NULL (the schedule reads movement_mode, gait_counter, gait_counter_speed, contacts; the feet foot_pos_abs, root_lin_vel_d, R_world).  Refused with A1MPC_ERR_INVALID_ARGUMENT (a1mpc_last_error names the field): a null config, ticks_per_step outside 1..64, foot_preview outside
 * 0..2, contact_schedule outside 0..1, horizon 1, counter_per_gait <= 0, foot_steps_out with foot_preview 0.
 * Host pointers; a1mpc_horizon_preview_batch_device: device pointers, asynchronous on hip_stream (NULL = the handle's).
 */
a1mpc_status a1mpc_horizon_preview_batch(a1mpc_handle h, const a1mpc_preview_config* cfg, const a1mpc_gait_config* gait, int32_t n,
                                         const uint8_t* movement_mode, const double* gait_counter, const double* gait_counter_speed, const uint8_t* contacts,
                                         const double* foot_pos_abs, const double* R_world, const double* root_lin_vel_d, uint8_t* contact_sched_out,
                                         double* foot_steps_out);
a1mpc_status a1mpc_horizon_preview_batch_device(a1mpc_handle h, const a1mpc_preview_config* cfg, const a1mpc_gait_config* gait, int32_t n,
                                                const uint8_t* d_movement_mode, const double* d_gait_counter, const double* d_gait_counter_speed,
                                                const uint8_t* d_contacts, const double* d_foot_pos_abs, const double* d_R_world, const double* d_root_lin_vel_d,
                                                uint8_t* d_contact_sched_out, double* d_foot_steps_out, void* hip_stream);
/*
 * The preview with FOOTHOLDS: a leg that the schedule lifts and puts down again inside the horizon stands, from its touchdown on, where update_plan has just planned it
 * (the Raibert foothold foot_pos_target_abs, S/A1RobotControl.cpp:166-199, the third output of a1mpc_update_plan_batch), not at the place it left.  The QP then knows
 * where a swing leg lands as well as when.  Not in the reference (which uses the current feet at every step, S/A1RobotControl.cpp:498-514).
 * For robot i, leg l, steps t = 0 .. H-1, with c_t the contact bit of the schedule the same a1mpc_preview_config produces (c_0 = contacts[]; contact_schedule 0:
 * contacts[] at every step), s = v * dt rounded once (v, dt as for foot_preview 1 / 2 above) and T = foot_pos_target_abs[i][3l .. 3l+2]:
 *   f_0 = foot_pos_abs
 *   f_t = T             if c_t == 1 and c_(t-1) == 0   (a touchdown: the words of T, copied)
 *   f_t = f_(t-1) - s   otherwise                      (the recurrence of S/test/test_mpc.cpp:112-115, continued from whatever f_(t-1) is)
 * A second touchdown of the leg inside the horizon is T again; swing steps carry the shifted value (their forces are bound to zero); with contact_schedule 0 there is
 * no touchdown and the feet are a1mpc_horizon_preview_batch's.  Not predicted: the target of a LATER touchdown is today's (constant velocity and command), and there is
 * no terrain height at the foothold.  Bit-identical to the plain C++ loop of these lines (no FMA contraction).
 * Arguments, layouts and validation of a1mpc_horizon_preview_batch(_device), with foot_pos_target_abs n x 12 (3x4 column-major, a1mpc_update_plan_batch's layout) after
 * root_lin_vel_d.  Refused in addition, with A1MPC_ERR_INVALID_ARGUMENT and a1mpc_last_error naming the argument: foot_steps_out with a null foot_pos_target_abs; with
 * contact_schedule 1, foot_steps_out with a null movement_mode, gait_counter, gait_counter_speed or contacts even when contact_sched_out is NULL (the footholds read the
 * schedule).  With foot_steps_out == NULL the call IS a1mpc_horizon_preview_batch(_device).  a1mpc_preview_config is unchanged: foot_preview 3 stays refused.
 */
a1mpc_status a1mpc_horizon_preview_footholds_batch(a1mpc_handle h, const a1mpc_preview_config* cfg, const a1mpc_gait_config* gait, int32_t n,
                                                   const uint8_t* movement_mode, const double* gait_counter, const double* gait_counter_speed,
                                                   const uint8_t* contacts, const double* foot_pos_abs, const double* R_world, const double* root_lin_vel_d,
                                                   const double* foot_pos_target_abs, uint8_t* contact_sched_out, double* foot_steps_out);
a1mpc_status a1mpc_horizon_preview_footholds_batch_device(a1mpc_handle h, const a1mpc_preview_config* cfg, const a1mpc_gait_config* gait, int32_t n,
                                                          const uint8_t* d_movement_mode, const double* d_gait_counter, const double* d_gait_counter_speed,
                                                          const uint8_t* d_contacts, const double* d_foot_pos_abs, const double* d_R_world,
                                                          const double* d_root_lin_vel_d, const double* d_foot_pos_target_abs, uint8_t* d_contact_sched_out,
                                                          double* d_foot_steps_out, void* hip_stream);
/*
 * Tick records (a1mpc_solve_batch_ticks: x0 / x_ref built on the device, S/A1RobotControl.cpp:452-488) joined with the strides of a1mpc_solve_batch_strided.
 * (foot_stride, contact_stride, yaw_A) = (0, 0, NULL) IS a1mpc_solve_batch_ticks(_device): same kernels, same bits.  (0, 4, NULL) runs the fast kernels at their speed
 * (contacts only change bounds and equality rows).  Per-step feet and / or a yaw_A run the general kernels, whose set-up builds x0 / x_ref from the record exactly as
 * the fast path's does; with yaw_A = NULL the A_c yaw is the record's root_euler[2] (= mpc_states[2], S/A1RobotControl.cpp:452,492).  Same iterates as
 * a1mpc_solve_batch_strided on the explicit x0 / x_ref up to the rounding of x_ref (base + (slope * dt) * (i + 1) here as in compute_grf).  All warm-start modes as on
 * the underlying entries.  The host-pointer entry stages through device memory at every n (no pinned small-batch transport).  Horizon >= 2.
 */
a1mpc_status a1mpc_solve_batch_ticks_strided(a1mpc_handle h, int32_t n, const double* tick, const double* R_world, const double* foot_abs, int32_t foot_stride,
                                             const uint8_t* contact, int32_t contact_stride, const double* yaw_A, double* grf_body_out, double* u_full_out,
                                             int32_t* iters_out, int32_t* status_out);
a1mpc_status a1mpc_solve_batch_ticks_strided_device(a1mpc_handle h, int32_t n, const double* d_tick, const double* d_R_world, const double* d_foot_abs,
                                                    int32_t foot_stride, const uint8_t* d_contact, int32_t contact_stride, const double* d_yaw_A,
                                                    double* d_grf_body_out, double* d_u_full_out, int32_t* d_iters_out, int32_t* d_status_out, void* hip_stream);
/*
 * a1mpc_control_tick_device with the preview between the contacts / terrain stage and the MPC launch: the chain of a1mpc_control_tick_device in which
 * a1mpc_horizon_preview_batch_device (schedule and / or feet into handle-owned device buffers, allocated once) + a1mpc_solve_batch_ticks_strided_device +
 * a1mpc_joint_torques_batch_device replace the ticks solve -- bit-identical to chaining those entries by hand.
 *   {0, 0, *}                      IS a1mpc_control_tick_device: same launches (no preview kernel), same bits, same torques_fused.
 *   contact_schedule 1, feet 0     the tick stays on the fast kernels; compute_joint_torques (N3) stays in the MPC kernel's output stage wherever it is today -- that
 *                                  stage reads step 0 of the schedule, the actual contacts[], so the torques keep their meaning.
 *   foot_preview 1 / 2             the general kernels solve the tick (1.7-2.5x the fast path's first solves, see a1mpc_solve_batch_strided); they have no torque stage, so
 *                                  the joint torques are a1mpc_torque_kernel as a launch of its own and a1mpc_last_control_tick_ms reports torques_fused = 0.
 * cfg.warm_start 0 / 1 / 2 behave as on the underlying solve entries (a1mpc_last_warm_start_mode stays truthful).  a1mpc_last_control_tick_ms reports this tick too.
 * Validation as a1mpc_horizon_preview_batch (params->gait.counter_per_gait <= 0 is refused whenever a preview is on).
 */
a1mpc_status a1mpc_control_tick_preview_device(a1mpc_handle h, const a1mpc_tick_params* params, const a1mpc_preview_config* preview,
                                               const a1mpc_tick_buffers* buffers, int32_t n, void* hip_stream);
/*
 * a1mpc_control_tick_preview_device with the foothold rule of a1mpc_horizon_preview_footholds_batch_device fed from buffers->foot_pos_target_abs, which update_plan
 * (stage 3 of the same tick, S/A1RobotControl.cpp:198) has just written: bit-identical to the chain with that entry in the preview's place.  buffers->foot_pos_target_abs,
 * an optional output elsewhere, is mandatory here whenever preview->foot_preview != 0 (a null one is refused, A1MPC_ERR_INVALID_ARGUMENT).  With foot_preview 0 the call
 * IS a1mpc_control_tick_preview_device: same launches, same bits.  torques_fused = 0 with feet on, as there; a1mpc_last_control_tick_ms reports this tick too.
 */
a1mpc_status a1mpc_control_tick_preview_footholds_device(a1mpc_handle h, const a1mpc_tick_params* params, const a1mpc_preview_config* preview,
                                                         const a1mpc_tick_buffers* buffers, int32_t n, void* hip_stream);

/*
 * What the model does with a force plan: the predicted states over the horizon and the cost of the plan, n problems, on the device.  The reference keeps A_qp and B_qp
 * as public members of ConvexMpc (S/ConvexMpc.h, filled by calculate_qp_mats, S/ConvexMpc.cpp:181-202); its caller gets the predicted trajectory A_qp x0 + B_qp u and the
 * tracking cost with one Eigen product each.  These entries replace that use of the two members (the solver here never forms them): x_pred IS A_qp x0 + B_qp u.
 * The model is exactly the reference's: A_d = I + dt A_c, B_d,t = dt B_c,t (forward Euler, S/ConvexMpc.cpp:110-151), with R_world and the yaw of A_c FROZEN over the
 * horizon (one A_d for all steps, one world inertia; only the feet may change per step).  With x_0 = x0[i], for t = 0 .. H-1 (H = the handle's horizon, >= 2), every
 * x_t read before x_(t+1) is written:
 *   rpy_(t+1) = rpy_t + dt T w_t                         T = [c s 0; -s c 0; 0 0 1], c, s = cos / sin(yaw), yaw = yaw_A[i] or x0[i][2]
 *   pos_(t+1) = pos_t + dt v_t
 *   w_(t+1)   = w_t + dt Iw^-1 sum_leg r_(t,leg) x f_(t,leg)     Iw = R I_b R', r = foot_abs (step t with foot_stride 12), f = u_full; legs summed in the order 0 .. 3
 *   v_(t+1)   = v_t + (dt / m) sum_leg f_(t,leg) + dt [0, 0, x_t[12]]
 *   x_(t+1)[12] = x_t[12]
 * Layouts are those of a1mpc_solve_batch_strided / a1mpc_solve_batch_ticks_strided (x0 n x 13, x_ref n x 13H, R_world n x 9 row-major, foot_abs n x 12 or n x 12H,
 * foot_stride 0 / 12, yaw_A NULL or n, u_full n x 12H world-frame forces = u_full_out of a solve): the inputs and outputs of a solve are passed on unchanged.
 * dt, q, r, mass, inertia_body and the horizon are the handle's configuration.  u_full == NULL means zero forces: the free response A_qp x0.
 * out, each may be NULL (not both):
 *   x_pred_out  n x 13H   step t of problem i at [(i*H + t)*13] holds x_(t+1) -- the index convention of x_ref / mpc_states_d, whose block t is compared with A_d^(t+1) x0
 *   cost_out    n x 2     [0] = sum_t sum_(k<12) q_k (x_(t+1),k - x_ref_t,k)^2        [1] = sum_t sum_j r_j u_(t,j)^2
 * With the reference's Q = 2 diag(q), R = 2 diag(r) (S/ConvexMpc.cpp:12-44) these are 1/2 e'Qe and 1/2 u'Ru, so
 *   cost[0](u) + cost[1](u) - cost[0](0) = 1/2 u'Pu + g'u,
 * OSQP's objective on the reference's hessian / gradient (S/ConvexMpc.cpp:204-215); cost[0](0) is what a call with u_full == NULL returns.  cost_out needs x_ref.
 * The _ticks entries take the compact tick record of a1mpc_solve_batch_ticks instead of (x0, x_ref): x0 = [tick[0:12], -9.8] and x_ref_t = base + (slope dt)(t + 1),
 * built as S/A1RobotControl.cpp:470-488 builds mpc_states_d, with the expressions the solve's set-up uses.
 * Refused with A1MPC_ERR_INVALID_ARGUMENT (a1mpc_last_error names the argument), whether or not a GPU is present: a null handle, n < 0 or n > max_batch, a foot_stride
 * other than 0 / 12, both outputs NULL, cost_out without x_ref, a null x0 / tick, R_world or foot_abs, a handle of horizon < 2.  n == 0 is A1MPC_OK and launches nothing.
 * Host pointers; the _device entries take device pointers and are asynchronous on hip_stream (NULL = the handle's): a call on the stream of the preceding
 * a1mpc_solve_batch_*_device sees its d_u_full_out, so solve -> predicted state -> next tick's x0 chains without a host copy.
 */
a1mpc_status a1mpc_horizon_states_batch(a1mpc_handle h, int32_t n, const double* x0, const double* x_ref, const double* R_world,
                                        const double* foot_abs, int32_t foot_stride, const double* yaw_A, const double* u_full,
                                        double* x_pred_out, double* cost_out);
a1mpc_status a1mpc_horizon_states_batch_device(a1mpc_handle h, int32_t n, const double* d_x0, const double* d_x_ref, const double* d_R_world,
                                               const double* d_foot_abs, int32_t foot_stride, const double* d_yaw_A, const double* d_u_full,
                                               double* d_x_pred_out, double* d_cost_out, void* hip_stream);
a1mpc_status a1mpc_horizon_states_ticks_batch(a1mpc_handle h, int32_t n, const double* tick, const double* R_world, const double* foot_abs,
                                              int32_t foot_stride, const double* yaw_A, const double* u_full, double* x_pred_out, double* cost_out);
a1mpc_status a1mpc_horizon_states_ticks_batch_device(a1mpc_handle h, int32_t n, const double* d_tick, const double* d_R_world, const double* d_foot_abs,
                                                     int32_t foot_stride, const double* d_yaw_A, const double* d_u_full, double* d_x_pred_out,
                                                     double* d_cost_out, void* hip_stream);

/*
 * The plant that closes the loop on the device: one control period of the NONLINEAR single rigid body under the forces a solve returned, n robots.  The reference gets
 * its plant from a simulator or the robot; a1mpc_horizon_states_* is the MPC's own linear model (R_world and the yaw of A_c frozen, no gyroscopic term, feet that do not
 * move with the body).  This is the body that model linearises:  a1mpc_solve_batch_ticks_device -> a1mpc_plant_step_batch_device -> a1mpc_solve_batch_ticks_device on one
 * stream, in place on the tick records, R_world and the feet, with no host copy.
 *   state      n x state_stride, state_stride = 12, 13 or 22: [0:3] euler  [3:6] pos  [6:9] omega (WORLD frame)  [9:12] v (world) -- the head of an x0 row (13) or of a
 *              tick record (22).  The input euler is NOT read (the attitude state is R_world); words [12:state_stride) of state_out are never written: the gravity word
 *              of an x0 row and the command half of a tick record survive a step in place
 *   R_world    n x 9 row-major, body -> world        foot_abs  n x 12, leg l at [3l:3l+3]: the world-oriented lever from the COM (foot_pos_abs)
 *   grf_body   n x 12 BODY-frame forces, grf_body_out of a solve        contacts  n x 4, non-zero = stance
 *   ext_wrench NULL, or n x 6: [0:3] force, [3:6] torque about the COM, world frame
 * mass and inertia_body are the handle's configuration; a1mpc_plant_config holds dt (one call advances by dt), substeps (1 .. 64) and gravity_z (default -9.8, the
 * constant of mpc_states[12]).  Forces and contacts are held over the call.  Before the first sub-step:
 *   0. R <- R - R (R^T R - I) / 2, the first-order step to the nearest orthogonal matrix.  L is carried INSIDE a call only (the handle keeps no state); the next call
 *      rebuilds it from omega through R_world, and R^T R - I enters that rebuild times the condition number of the inertia.  Without this step the rounding of every
 *      Cayley product so far piles up in R^T R (a random walk, 5e-15 after 400 calls) and the world angular momentum of a torque-free body moves by 2e-12 .. 4e-12
 *      relative over 400 calls; with it R^T R - I stays at 4e-16 and the momentum within 8e-14.  An R_world that is orthogonal to rounding is changed by an ulp at most
 *   then L = R (I_b (R^T omega)) and I_b^-1 by cofactors; then `substeps` times, with h = dt / substeps:
 *   1. fw_l = R f_l for a stance leg, exactly +0 for a swing leg (selected, not multiplied: a NaN in a swing leg's force does not reach the body)
 *   2. F = ((fw_0 + fw_1) + (fw_2 + fw_3)) + f_ext,  tau = ((r_0 x fw_0 + r_1 x fw_1) + (r_2 x fw_2 + r_3 x fw_3)) + tau_ext
 *   3. v' = v + h (F / m + g e_z),  dp = h v',  pos' = pos + dp                                   (semi-implicit Euler)
 *   4. a = (h / 2) omega,  R' = cay(a) R,  cay(a) = I + s ([a]x + [a]x^2),  s = 2 / (1 + a.a)     (the Cayley map: orthogonal in exact arithmetic, no sin / cos)
 *   5. L' = L + h tau,  omega' = R' (I_b^-1 (R'^T L'))                                            (omega from the NEW attitude: L is kept to rounding over the call)
 *   6. a stance foot is pinned in the world, r' = r - dp; a swing foot keeps its body-frame position, r' = R' (R^T r)
 * After the last sub-step the angles are read off R in the rot_zyx convention: roll = atan2(R[7], R[8]), pitch = asin(clamp(-R[6], -1, 1)), yaw = atan2(R[3], R[0]).
 * They are an output only and never feed back.
 * Arithmetic: IEEE add, subtract, multiply and divide alone (no fused multiply-add, contraction off, three-term sums left to right) up to the three inverse
 * trigonometric calls, so pos, R, v, omega and the feet are a pure function of the robot's own inputs -- the same bits at every batch size, position in the batch and
 * entry -- and an elementwise restatement reproduces them bit for bit.  f64 division in this build is correctly rounded (the compiler's IEEE expansion: the library is
 * built without any fast-math or unsafe-math flag) and f64 subnormals are kept.
 * What it is not: first order in h (rotational energy drifts, about 2 % over 5 s at |omega| = 5 rad/s with substeps = 1); no ground, no contact or friction model --
 * the forces are taken as given, a stance foot does not slip and nothing stops a body below its feet; massless legs.
 * out: state_out n x state_stride, R_world_out n x 9, foot_abs_out n x 12, all required.  Each may be its input exactly (in place); any other overlap is the
 * caller's error.  Non-finite inputs of one robot give non-finite outputs of that robot alone.
 * Refused with A1MPC_ERR_INVALID_ARGUMENT (a1mpc_last_error names the field) before any launch: a null handle or config, substeps outside 1 .. 64, dt <= 0 or not
 * finite, a gravity_z that is not finite, a state_stride other than 12 / 13 / 22, n < 0 or n > max_batch, a null required pointer.  n == 0 is A1MPC_OK and launches
 * nothing.  The handle gets no state.  Host pointers (staged like the other caller-side entries); the _device entry takes device pointers and is asynchronous on
 * hip_stream (NULL = the handle's), ordered like every other _device entry: on the stream of the preceding a1mpc_solve_batch_*_device it reads that solve's
 * d_grf_body_out.
 */
typedef struct a1mpc_plant_config { double dt; int32_t substeps; double gravity_z; } a1mpc_plant_config;
void a1mpc_default_plant_config(a1mpc_plant_config* cfg);   /* 0.0025 (the control tick), 1, -9.8 */
a1mpc_status a1mpc_plant_step_batch(a1mpc_handle h, const a1mpc_plant_config* cfg, int32_t n, const double* state_in, int32_t state_stride, const double* R_world,
                                    const double* foot_abs, const double* grf_body, const uint8_t* contacts, const double* ext_wrench, double* state_out,
                                    double* R_world_out, double* foot_abs_out);
a1mpc_status a1mpc_plant_step_batch_device(a1mpc_handle h, const a1mpc_plant_config* cfg, int32_t n, const double* d_state_in, int32_t state_stride,
                                           const double* d_R_world, const double* d_foot_abs, const double* d_grf_body, const uint8_t* d_contacts,
                                           const double* d_ext_wrench, double* d_state_out, double* d_R_world_out, double* d_foot_abs_out, void* hip_stream);

/*
 * Sensor synthesis: what a robot's sensors read on the body a1mpc_plant_step_batch advances -- the inverse of the front stages of a1mpc_control_tick_sensors_device
 * (quaternion -> R, joint angles -> feet, the EKF's accelerometer and foot-velocity relations), n robots.  With it  a1mpc_sensor_synthesis_batch_device ->
 * a1mpc_control_tick_sensors_device -> a1mpc_plant_step_batch_device  runs on one stream with no host copy, and the estimator, the leg kinematics, the contact logic and
 * the sensor front end are inside the loop.
 * in: the layouts of a1mpc_plant_step_batch.  state n x state_stride (12, 13 or 22), of which only [6:9] omega and [9:12] v are read, both world frame; R_world n x 9
 * row-major; foot_abs n x 12, r_l the lever of leg l; grf_body n x 12 and contacts n x 4: the forces that were applied; ext_wrench NULL or n x 6 (its force half is
 * read); rho_fix (20) and rho_opt (12): HOST arrays in both entries, the leg geometry of a1mpc_leg_state_batch.  The mass is the handle's cfg.mass.
 * Per robot, R row-major, every three-term sum left to right:
 *   gyro        imu_gyro_raw = R^T omega
 *   accelerometer  the specific force in the body frame:  imu_acc_raw = ((f_0 + f_1) + (f_2 + f_3)) / m,  then + (R^T f_ext) / m when a wrench is given; a swing leg
 *               contributes exactly +0, selected and not multiplied, as in the plant.  This is R^T (a - g e_z) of the plant's step 3: no differencing and no gravity
 *               constant (the EKF adds its own (0, 0, -9.81), A1BasicEKF.cpp:76)
 *   foot force  foot_force_l = the world z component of R f_l,  (R20 f0 + R21 f1) + R22 f2,  for a stance leg; +0 for a swing leg
 *   quaternion  (w, x, y, z) by Eigen's matrix-to-quaternion algorithm.  tr = (R00 + R11) + R22 > 0:  t = sqrt(tr + 1), w = t / 2, t = 0.5 / t, x = (R21 - R12) t,
 *               y = (R02 - R20) t, z = (R10 - R01) t.  Otherwise i = the largest diagonal (0; 1 if R11 > R00; 2 if R22 > Rii), j = (i + 1) % 3, k = (j + 1) % 3:
 *               t = sqrt(((Rii - Rjj) - Rkk) + 1), q_i = t / 2, t = 0.5 / t, w = (Rkj - Rjk) t, q_j = (Rji + Rij) t, q_k = (Rki + Rik) t
 *   foot position  foot_pos_rel_l = p = R^T r_l
 *   joint angles   the closed-form inverse of the leg model of a1mpc_leg_state_batch, with its ox = f[0], oy = f[1], L = f[2] + o[1], lt = f[3], al = f[4] - o[2],
 *               r0 = o[0] (f = rho_fix + 5 l, o = rho_opt + 3 l):
 *                 dx = p0 - ox,  dy = p1 - oy,  Zp = -sqrt(max((dy dy + p2 p2) - L L, 0)),  q0 = atan2(p2, dy) - atan2(Zp, L)
 *                 ell = sqrt(al al + r0 r0),  phi = atan2(r0, al),  c = (((dx dx + Zp Zp) - lt lt) - ell ell) / ((2 lt) ell)
 *                 k = -acos(clamp(c, -1, 1))   (the knee bends back, as the A1's does)
 *                 q1 = atan2(-dx, -Zp) - atan2(ell sin k, lt + ell cos k),  q2 = k + phi
 *   foot velocity  stance leg: foot_vel_rel_l = -(R^T (v + omega x r_l)), the foot at rest in the world (the relation A1BasicEKF.cpp:122 inverts); swing leg: exactly
 *               +0, the foot fixed in the body (the plant's step 6)
 *   joint rates    joint_vel_l = J(q)^-1 foot_vel_rel_l, J the leg model's Jacobian evaluated at the synthesised angles, the inverse by cofactors like the plant's I_b^-1
 *   reach flags    reach_l bit 0: dy dy + p2 p2 < L L was clamped; bit 1: c was clamped.  Any bit set: this leg's joint_vel is exactly +0
 * Arithmetic: contraction off, no fused multiply-add; IEEE +, -, *, / and sqrt, the device library's atan2, acos, sin and cos.  Each robot's outputs are a pure function
 * of that robot's inputs alone: the same bits at every batch size, position in the batch and entry.
 * What it is not: no sensor noise or bias of its own (a1mpc_sensor_noise_batch below adds them to these outputs), no ground or contact model (foot_force is the
 * applied force, not a measured one); a swing foot is fixed in the body, as the
 * plant keeps it, so the loop this closes is the standing robot.
 * out: quat_out n x 4, imu_acc_raw_out and imu_gyro_raw_out n x 3, joint_pos_out and joint_vel_out n x 12, foot_force_out n x 4 doubles and reach_out n x 4 bytes, all
 * required; foot_pos_rel_out and foot_vel_rel_out n x 12, optional (NULL = not wanted).  No output may alias an input.  Non-finite inputs of one robot stay with that robot.
 * Refused with A1MPC_ERR_INVALID_ARGUMENT (a1mpc_last_error names the argument) before any launch: a null handle or required pointer, a state_stride other than
 * 12 / 13 / 22, n < 0, a geometry value that is not finite, lt <= 0, al al + r0 r0 == 0; n > max_batch is A1MPC_ERR_BATCH_TOO_LARGE.  n == 0 is A1MPC_OK and launches
 * nothing.  The handle gets no state.  Host pointers (staged like the other caller-side entries); the _device entry takes device pointers and is asynchronous on
 * hip_stream (NULL = the handle's), ordered like every other _device entry.
 */
a1mpc_status a1mpc_sensor_synthesis_batch(a1mpc_handle h, int32_t n, const double* state, int32_t state_stride, const double* R_world, const double* foot_abs,
                                          const double* grf_body, const uint8_t* contacts, const double* ext_wrench, const double* rho_fix, const double* rho_opt,
                                          double* quat_out, double* imu_acc_raw_out, double* imu_gyro_raw_out, double* joint_pos_out, double* joint_vel_out,
                                          double* foot_force_out, uint8_t* reach_out, double* foot_pos_rel_out, double* foot_vel_rel_out);
a1mpc_status a1mpc_sensor_synthesis_batch_device(a1mpc_handle h, int32_t n, const double* d_state, int32_t state_stride, const double* d_R_world,
                                                 const double* d_foot_abs, const double* d_grf_body, const uint8_t* d_contacts, const double* d_ext_wrench,
                                                 const double* rho_fix, const double* rho_opt, double* d_quat_out, double* d_imu_acc_raw_out,
                                                 double* d_imu_gyro_raw_out, double* d_joint_pos_out, double* d_joint_vel_out, double* d_foot_force_out,
                                                 uint8_t* d_reach_out, double* d_foot_pos_rel_out, double* d_foot_vel_rel_out, void* hip_stream);

/*
 * The walking plant: a1mpc_plant_step_batch with swing feet that MOVE in the body frame and a flat rigid ground, and the sensors that know the swing feet move.  With
 * them  a1mpc_walk_sensors_batch_device -> a1mpc_control_tick_sensors_device -> a1mpc_walk_step_batch_device  runs on one stream with no host copy while the gait layer
 * (update_plan, the Bezier swing legs, the contact logic) walks the body: in movement_mode 1 the loop this closes is the trotting robot.  The plant step and the sensor
 * synthesis above are unchanged and stay the standing robot's.
 *
 * a1mpc_walk_step_batch.  Layouts, strides 12 / 13 / 22, the in-place rule of state / R_world / foot_abs, mass and inertia (the handle's) are those of
 * a1mpc_plant_step_batch; cfg->plant is its configuration.  Step 0 (the polish of R) and steps 1 - 5 of every sub-step are its steps, in its operation order.  New:
 *   in   R_z          n x 9 row-major: the tick's root_rot_mat_z (a1mpc_tick_buffers.R_z)
 *        foot_target  n x 12: the tick's foot_pos_target_last_time, y_l = the Bezier point the swing-leg stage asked leg l to be at on this tick, in the frame of
 *                     foot_pos_cur = R_z^T foot_pos_abs.  Both are device-resident outputs / carried state of a1mpc_control_tick_device
 *   before the sub-steps, with R the polished attitude, for every leg:  p0 = R^T r,  p_t = R^T (R_z y),  d = (swing_track (p_t - p0)) / substeps,
 *        vel = (swing_track (p_t - p0)) / dt.  swing_track == 0: d and vel are exactly +0, selected and not multiplied; R_z and foot_target are not read and may be NULL
 *   step 6 of a sub-step:  a stance foot keeps r' = r - dp;  a swing foot does p = R^T r, p' = p + d, r' = R' p'  (swing_track == 0: p' = p, the sum is skipped, so the
 *        step is a1mpc_plant_step_batch's bit for bit)
 *   after the last sub-step, when flat_ground != 0, with gz = ground_z - pos_z':  a stance foot gets r'_z = gz (ON the plane z = ground_z of the world);  a swing foot
 *        gets r'_z = (r'_z < gz) ? gz : r'_z (not below it; a NaN stays a NaN)
 *   out  foot_vel_body_out n x 12, required: a swing leg writes vel, the COMMANDED body-frame velocity of its foot over this call; a stance leg writes +0.  It is the
 *        commanded velocity: on a tick where the ground stops the foot it overstates the z motion.  a1mpc_walk_sensors_batch reads it
 * A stance leg's foot_target reaches no output (selected away, like a swing leg's force): a NaN there changes no bit.  swing_track in (0, 1) moves the foot that
 * fraction of the way per call.  The default configuration is a1mpc_default_plant_config, swing_track 1, flat_ground 0, ground_z 0.
 * What it is not: a kinematic swing over a flat rigid plane.  Legs are massless; there is no impact and no slip; no friction cone is applied to the given forces;
 * nothing stops the BODY itself at the plane; and the foot-force sensor of a1mpc_walk_sensors_batch is still the applied force, not a measured touchdown, so the
 * reference's early-contact branch never fires.
 * Refused with A1MPC_ERR_INVALID_ARGUMENT (a1mpc_last_error names the field) before any launch: everything a1mpc_plant_step_batch refuses (on cfg->plant), a null
 * foot_vel_body_out, a swing_track outside [0, 1] or not finite, flat_ground set with a ground_z that is not finite, swing_track > 0 with a NULL R_z or foot_target.
 * n == 0 is A1MPC_OK and launches nothing.  The handle gets no state.  Host pointers, or (_device) device pointers, asynchronous on hip_stream.
 *
 * a1mpc_walk_sensors_batch is a1mpc_sensor_synthesis_batch with one more input, foot_vel_body (n x 12, optional) after ext_wrench: on a SWING leg foot_vel_rel_l is
 * foot_vel_body_l (selected) instead of +0, and joint_vel_l = J(q)^-1 of it by the same cofactor inverse; the reach-flag rule (any bit set: joint_vel_l = +0) is
 * unchanged; a stance leg's foot_vel_body reaches no output.  Everything else is the synthesis's arithmetic, layouts and refusals; with foot_vel_body NULL or all +0
 * every output is a1mpc_sensor_synthesis_batch's bit for bit.
 */
typedef struct a1mpc_walk_config { a1mpc_plant_config plant; double swing_track; int32_t flat_ground; double ground_z; } a1mpc_walk_config;
void a1mpc_default_walk_config(a1mpc_walk_config* cfg);   /* a1mpc_default_plant_config, 1.0, 0, 0.0 */
a1mpc_status a1mpc_walk_step_batch(a1mpc_handle h, const a1mpc_walk_config* cfg, int32_t n, const double* state_in, int32_t state_stride, const double* R_world,
                                   const double* foot_abs, const double* grf_body, const uint8_t* contacts, const double* ext_wrench, const double* R_z,
                                   const double* foot_target, double* state_out, double* R_world_out, double* foot_abs_out, double* foot_vel_body_out);
a1mpc_status a1mpc_walk_step_batch_device(a1mpc_handle h, const a1mpc_walk_config* cfg, int32_t n, const double* d_state_in, int32_t state_stride,
                                          const double* d_R_world, const double* d_foot_abs, const double* d_grf_body, const uint8_t* d_contacts,
                                          const double* d_ext_wrench, const double* d_R_z, const double* d_foot_target, double* d_state_out, double* d_R_world_out,
                                          double* d_foot_abs_out, double* d_foot_vel_body_out, void* hip_stream);
a1mpc_status a1mpc_walk_sensors_batch(a1mpc_handle h, int32_t n, const double* state, int32_t state_stride, const double* R_world, const double* foot_abs,
                                      const double* grf_body, const uint8_t* contacts, const double* ext_wrench, const double* foot_vel_body, const double* rho_fix,
                                      const double* rho_opt, double* quat_out, double* imu_acc_raw_out, double* imu_gyro_raw_out, double* joint_pos_out,
                                      double* joint_vel_out, double* foot_force_out, uint8_t* reach_out, double* foot_pos_rel_out, double* foot_vel_rel_out);
a1mpc_status a1mpc_walk_sensors_batch_device(a1mpc_handle h, int32_t n, const double* d_state, int32_t state_stride, const double* d_R_world, const double* d_foot_abs,
                                             const double* d_grf_body, const uint8_t* d_contacts, const double* d_ext_wrench, const double* d_foot_vel_body,
                                             const double* rho_fix, const double* rho_opt, double* d_quat_out, double* d_imu_acc_raw_out, double* d_imu_gyro_raw_out,
                                             double* d_joint_pos_out, double* d_joint_vel_out, double* d_foot_force_out, uint8_t* d_reach_out,
                                             double* d_foot_pos_rel_out, double* d_foot_vel_rel_out, void* hip_stream);

/*
 * Sloped ground and sensed touchdowns for the walking plant: a ground plane PER ROBOT under a1mpc_walk_step_batch, and a touch sensor on the feet of
 * a1mpc_walk_sensors_batch.  With them  a1mpc_touch_sensors_batch_device -> a1mpc_control_tick_sensors_device -> a1mpc_ground_step_batch_device  runs on one
 * stream with no host copy, and the gait layer's terrain fit (compute_walking_surface, use_terrain_adapt) and its early-contact latch meet a slope and a touchdown they
 * can be held to.  Kernels of their own (a1mpc_walk_step_ground_kernel, a1mpc_walk_sensors_touch_kernel): the four entries above are unchanged, and the walk family's
 * exported symbols stay the five of its block -- these four are a family of their own, a1mpc_ground_* / a1mpc_touch_*.
 *
 * a1mpc_ground_step_batch is a1mpc_walk_step_batch with one more input after foot_target and one more output after foot_vel_body_out:
 *   in   ground       n x 3, optional: (z0, sx, sy) of robot b; its ground is the plane hz(X, Y) = (z0 + sx X) + sy Y of the world, in that operation order, no FMA
 *   after the last sub-step, for every leg, with ground given:  X = pos'_x + r'_x,  Y = pos'_y + r'_y,  gz = hz(X, Y) - pos'_z;  a stance foot gets r'_z = gz;  a swing
 *        foot gets r'_z = (r'_z < gz) ? gz : r'_z.  The projection is VERTICAL: x and y of every foot and of the body do not change.  cfg->flat_ground and
 *        cfg->ground_z are not read.  ground NULL: the rule of a1mpc_walk_step_batch with cfg's plane, or none
 *   out  touch_out    n x 4 bytes, required: 1 for a stance leg; for a swing leg 1 exactly when the comparison above lifted the foot (the same comparison: a NaN
 *                     gives 0); 0 for every swing leg when there is no ground at all (ground NULL and flat_ground == 0)
 * Reductions: with ground NULL every other output is a1mpc_walk_step_batch's bit for bit; with ground = (ground_z, 0, 0) and finite inputs every other output is
 * a1mpc_walk_step_batch's with flat_ground = 1, bit for bit.  A row of ground that is not finite stays with its robot (the z of its feet).
 * Refused: everything a1mpc_walk_step_batch refuses (the ground_z check only with ground NULL), and a null touch_out.  In-place use of state, R_world and foot_abs
 * follows a1mpc_walk_step_batch's rule.
 *
 * a1mpc_touch_sensors_batch is a1mpc_walk_sensors_batch with two more inputs after foot_vel_body: touch (n x 4 bytes, optional: the step's touch_out) and
 * touch_force (by value).  On a SWING leg whose touch byte is non-zero foot_force_l = touch_force, selected and not added; a stance leg's byte reaches no output.
 * Nothing else changes: legs are massless and there is no impact, so the accelerometer is a1mpc_walk_sensors_batch's.  With touch NULL or touch_force == 0 every
 * output is a1mpc_walk_sensors_batch's bit for bit.  Refused: everything a1mpc_walk_sensors_batch refuses, and a touch_force that is negative or not finite.
 *
 * What it is not: ONE plane per robot -- no steps, no height field; the projection is vertical, so a stance foot on a slope neither slips nor feels a friction cone;
 * the touch force is a constant, not a contact model; nothing stops the BODY itself at the plane; and the tick's foot preview still plans flat-ground footholds.
 */
a1mpc_status a1mpc_ground_step_batch(a1mpc_handle h, const a1mpc_walk_config* cfg, int32_t n, const double* state_in, int32_t state_stride, const double* R_world,
                                          const double* foot_abs, const double* grf_body, const uint8_t* contacts, const double* ext_wrench, const double* R_z,
                                          const double* foot_target, const double* ground, double* state_out, double* R_world_out, double* foot_abs_out,
                                          double* foot_vel_body_out, uint8_t* touch_out);
a1mpc_status a1mpc_ground_step_batch_device(a1mpc_handle h, const a1mpc_walk_config* cfg, int32_t n, const double* d_state_in, int32_t state_stride,
                                                 const double* d_R_world, const double* d_foot_abs, const double* d_grf_body, const uint8_t* d_contacts,
                                                 const double* d_ext_wrench, const double* d_R_z, const double* d_foot_target, const double* d_ground,
                                                 double* d_state_out, double* d_R_world_out, double* d_foot_abs_out, double* d_foot_vel_body_out, uint8_t* d_touch_out,
                                                 void* hip_stream);
a1mpc_status a1mpc_touch_sensors_batch(a1mpc_handle h, int32_t n, const double* state, int32_t state_stride, const double* R_world, const double* foot_abs,
                                            const double* grf_body, const uint8_t* contacts, const double* ext_wrench, const double* foot_vel_body, const uint8_t* touch,
                                            double touch_force, const double* rho_fix, const double* rho_opt, double* quat_out, double* imu_acc_raw_out,
                                            double* imu_gyro_raw_out, double* joint_pos_out, double* joint_vel_out, double* foot_force_out, uint8_t* reach_out,
                                            double* foot_pos_rel_out, double* foot_vel_rel_out);
a1mpc_status a1mpc_touch_sensors_batch_device(a1mpc_handle h, int32_t n, const double* d_state, int32_t state_stride, const double* d_R_world, const double* d_foot_abs,
                                                   const double* d_grf_body, const uint8_t* d_contacts, const double* d_ext_wrench, const double* d_foot_vel_body,
                                                   const uint8_t* d_touch, double touch_force, const double* rho_fix, const double* rho_opt, double* d_quat_out,
                                                   double* d_imu_acc_raw_out, double* d_imu_gyro_raw_out, double* d_joint_pos_out, double* d_joint_vel_out,
                                                   double* d_foot_force_out, uint8_t* d_reach_out, double* d_foot_pos_rel_out, double* d_foot_vel_rel_out,
                                                   void* hip_stream);

/*
 * Height-field terrain for the walking plant: ONE gridded field of heights under a1mpc_walk_step_batch in place of a1mpc_ground_step_batch's plane per robot -- stairs,
 * kerbs, rough ground.  With it  a1mpc_touch_sensors_batch_device -> a1mpc_control_tick_sensors_device -> a1mpc_heightfield_step_batch_device  runs on one stream
 * with no host copy; the step's touch bytes feed the touch sensors, its ground_out rows feed a1mpc_episode_update_batch, and a1mpc_heightfield_sample_batch places
 * spawn templates on the terrain in front of a1mpc_respawn_rows_device.  Kernels of their own (a1mpc_walk_step_heightfield_kernel, a1mpc_heightfield_sample_kernel):
 * every entry above is unchanged, and these five symbols are a family of their own, a1mpc_*heightfield*.  The handle gets no state.
 *
 * The field.  height is ny x nx doubles, row-major, x fastest: H[j * nx + i] is the height of node (i, j) at the world position (x0 + i dx, y0 + j dy).  It is a DEVICE
 * pointer in the _device entries and a host pointer in the host entries; the struct itself is always host memory, read during the call.
 *
 * The sampling rule hf(X, Y), one IEEE operation per step in exactly this order, no FMA:
 *   inv_dx = 1.0 / dx, inv_dy = 1.0 / dy          once on the host, passed to the kernels by value
 *   with a per-robot origin row (ox, oy, oz):     ux = ((X - ox) - x0) * inv_dx,   uy = ((Y - oy) - y0) * inv_dy
 *   with origin NULL:                             ux = (X - x0) * inv_dx,          uy = (Y - y0) * inv_dy        (the subtraction is skipped, not done with 0)
 *   valid = (ux == ux) && (uy == uy)
 *   cx = ux > 0.0 ? ux : 0.0;  cx = cx < (double)(nx - 1) ? cx : (double)(nx - 1);   cy likewise with ny    (a NaN goes to 0: the index is always in range)
 *        only cx and cy are ever converted to an integer; they are finite and lie in [0, nx - 1] and [0, ny - 1]
 *   interp == 0 (cell-constant: steps):  i = (int)cx, j = (int)cy, h = H[j * nx + i].  Cell (i, j) spans [x0 + i dx, x0 + (i + 1) dx) x [y0 + j dy, y0 + (j + 1) dy);
 *        the last node of an axis owns only its own line
 *   interp == 1 (bilinear):  i = (int)cx; i = i < nx - 1 ? i : nx - 2;  tx = cx - (double)i;  j and ty likewise;
 *        h00 = H[j * nx + i], h10 = H[j * nx + i + 1], h01 = H[(j + 1) * nx + i], h11 = H[(j + 1) * nx + i + 1];
 *        a = h00 + tx * (h10 - h00);  b = h01 + tx * (h11 - h01);  h = a + ty * (b - a)
 *   top = valid ? h : NaN, selected;  with origin given, top = top + oz;  hf(X, Y) = top
 * Outside the grid the field continues with its edge values (+-inf is clamped like any other value and gives a finite height); a NaN coordinate gives a NaN height.
 * The index arithmetic is 64-bit.  Several terrains in one batch are tiles of one field: robot b's origin row moves the field's frame to (ox, oy) and lifts it by oz.
 *
 * a1mpc_heightfield_step_batch is a1mpc_ground_step_batch with (field, origin) in place of ground and one more optional output, ground_out, after touch_out:
 *   in   field        the descriptor above
 *        origin       n x 3, optional: (ox, oy, oz) of robot b
 *   after the last sub-step, for every leg:  X = pos'_x + r'_x,  Y = pos'_y + r'_y,  gz = hf(X, Y) - pos'_z;  then the ground step's rule unchanged: a stance foot gets
 *        r'_z = gz;  a swing foot gets r'_z = (r'_z < gz) ? gz : r'_z;  touch_out (n x 4 bytes, required) is 1 for a stance leg, and for a swing leg 1 exactly when
 *        that comparison lifted the foot (a NaN keeps the foot and gives 0).  The projection is VERTICAL.  cfg->flat_ground and cfg->ground_z are not read
 *   out  ground_out   n x 3, optional: (hf(pos'_x, pos'_y), +0, +0) -- the row a1mpc_episode_update_batch takes as `ground`: its hz = (z0 + sx X) + sy Y is then the
 *                     terrain height under the body, bit for bit for a finite position; it is also the height condition of the closed loops
 * Reductions: with a constant field of a finite value c (either interp) and origin NULL every other output is a1mpc_ground_step_batch's with ground = (c, 0, 0), bit for
 * bit on finite inputs.  A robot's outputs do not depend on its position in the batch, on the batch size, or on the other robots.
 * In-place use of state, R_world and foot_abs follows a1mpc_ground_step_batch's rule.  n == 0 is A1MPC_OK and launches nothing.
 *
 * a1mpc_heightfield_sample_batch is the rule on its own, one point per lane: xy n x 2 (X, Y), origin n x 3 optional, height_out n.
 *
 * Refused with A1MPC_ERR_INVALID_ARGUMENT (a1mpc_last_error names the field) before any launch, every array left untouched.  The field is checked FIRST, in front of
 * the handle, so whether or not a GPU is present: a null descriptor or a null height; interp other than 0 or 1; nx or ny below 1 with interp == 0 or below 2 with
 * interp == 1; nx or ny above 32768; dx or dy not finite or not positive; x0 or y0 not finite; an inv_dx or inv_dy that is not finite.  Then, of the step, everything
 * a1mpc_ground_step_batch refuses (cfg's own plane is never checked); of the sample entry a null handle, n < 0, a null xy or height_out.  The host-pointer entries
 * stage the WHOLE field on every call, as every host-pointer entry stages its inputs: they are for tests and small fields, and refuse a field of more than 2^20 nodes
 * with A1MPC_ERR_BATCH_TOO_LARGE (a stated condition, not a measurement).  Their copy of the field is a device allocation that lives for the call (the handle gets no
 * state): unlike the other host-pointer entries, which use the handle's staging alone, they allocate and free device memory on every call, and the free synchronises the
 * WHOLE device, so they disturb work on other streams -- keep them out of a loop that shares the device, and use the _device entries there.
 * n > max_batch is A1MPC_ERR_BATCH_TOO_LARGE.  The _device entries are asynchronous on
 * hip_stream (NULL = the handle's); the field's heights must stay valid until the stream has passed the call.
 *
 * What it is not: the projection is vertical, so a swing foot that meets a riser is lifted onto the tread and reports a touch, not a collision; there is no slip and no
 * friction cone; nothing stops the BODY itself at the field; there is ONE field per call -- several terrains in one batch are tiles of one field, reached through
 * origin; and the tick's foot preview still plans flat-ground footholds.
 */
typedef struct a1mpc_heightfield {
    int32_t nx, ny;         /* nodes along world x / y */
    double x0, y0;          /* world position of node (0, 0) */
    double dx, dy;          /* node spacing, > 0 */
    int32_t interp;         /* 0: cell-constant (steps), 1: bilinear */
    const double* height;   /* ny x nx, row-major, x fastest: H[j * nx + i]; a DEVICE pointer in the _device entries, a host pointer in the host entries */
} a1mpc_heightfield;
void a1mpc_default_heightfield(a1mpc_heightfield* field);   /* 0, 0, 0.0, 0.0, 1.0, 1.0, 0, NULL */
a1mpc_status a1mpc_heightfield_step_batch(a1mpc_handle h, const a1mpc_walk_config* cfg, int32_t n, const double* state_in, int32_t state_stride, const double* R_world,
                                          const double* foot_abs, const double* grf_body, const uint8_t* contacts, const double* ext_wrench, const double* R_z,
                                          const double* foot_target, const a1mpc_heightfield* field, const double* origin, double* state_out, double* R_world_out,
                                          double* foot_abs_out, double* foot_vel_body_out, uint8_t* touch_out, double* ground_out);
a1mpc_status a1mpc_heightfield_step_batch_device(a1mpc_handle h, const a1mpc_walk_config* cfg, int32_t n, const double* d_state_in, int32_t state_stride,
                                                 const double* d_R_world, const double* d_foot_abs, const double* d_grf_body, const uint8_t* d_contacts,
                                                 const double* d_ext_wrench, const double* d_R_z, const double* d_foot_target, const a1mpc_heightfield* field,
                                                 const double* d_origin, double* d_state_out, double* d_R_world_out, double* d_foot_abs_out, double* d_foot_vel_body_out,
                                                 uint8_t* d_touch_out, double* d_ground_out, void* hip_stream);
a1mpc_status a1mpc_heightfield_sample_batch(a1mpc_handle h, const a1mpc_heightfield* field, int32_t n, const double* xy, const double* origin, double* height_out);
a1mpc_status a1mpc_heightfield_sample_batch_device(a1mpc_handle h, const a1mpc_heightfield* field, int32_t n, const double* d_xy, const double* d_origin,
                                                   double* d_height_out, void* hip_stream);

/*
 * Sensor noise and IMU bias on the device, reproducible per robot and tick: white Gaussian noise on the six sensor arrays that a1mpc_sensor_synthesis_batch,
 * a1mpc_walk_sensors_batch and a1mpc_touch_sensors_batch write, and a random-walk bias on the IMU.  With it  a1mpc_walk_sensors_batch_device ->
 * a1mpc_sensor_noise_batch_device -> a1mpc_control_tick_sensors_device -> a1mpc_walk_step_batch_device  runs on one stream with no host copy, and the EKF's
 * covariances, the contact logic's force thresholds and the IMU window meet inputs that are not exact.  A kernel of its own (a1mpc_sensor_noise_kernel) and a family
 * of its own, a1mpc_*noise*: the entries above are unchanged.
 *
 * in / out (all optional, NULL = that sensor is left alone), modified IN PLACE, in the synthesis entries' layouts: quat n x 4 (w first), imu_acc_raw and imu_gyro_raw
 *        n x 3, joint_pos and joint_vel n x 12, foot_force n x 4
 *        imu_bias  n x 6, optional: (gyro bias, acc bias) of robot b, carried by the caller from call to call (start it at zero); the handle gets no state
 * out    z_out     n x 44, optional: the unit normals drawn for robot b, the injected noise's truth
 * by value: robot0, the global index of row 0 (robot b of the call is robot g = robot0 + b of the experiment), and tick
 * Generator, per robot: draw j = 0 .. 21 is Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85) with the key (seed low word,
 * seed high word) on the counter (j, g, tick low word, tick high word).  Of its four words x0 .. x3:
 *        k1 = (x0 >> 6) 2^26 + (x1 >> 6),  k2 = (x2 >> 6) 2^26 + (x3 >> 6),  u = (k + 0.5) 2^-52   (exact, in (0, 1))
 *        r = sqrt(-2 log u1),  a = 6.283185307179586 u2,  z[2 j] = r cos a,  z[2 j + 1] = r sin a
 * Channels: z[0:3) gyro, z[3:6) acc, z[6:9) gyro bias step, z[9:12) acc bias step, z[12:15) attitude, z[15] unused, z[16:28) joint_pos, z[28:40) joint_vel,
 * z[40:44) foot_force.  A robot's normals are a function of (seed, g, tick) alone: the same bits at every batch size, position in the batch, shard and entry, and the
 * same whatever the sigmas are.
 * Arithmetic (contraction off, no fused multiply-add, sums left to right):
 *   bias      b' = b + walk z, stored back; a walk of 0 leaves b's bits alone and still applies it
 *   IMU       gyro' = (gyro + b'_gyro) + gyro_sigma z, acc likewise; without imu_bias there is no bias term
 *   attitude  theta = att_sigma z[12:15),  dq = (1, theta / 2),  q' = q (x) dq (Hamilton product, w first: a small rotation in the body frame), every component
 *             divided by sqrt(((w w + x x) + y y) + z z)
 *   joints and forces  x' = x + sigma z, on every leg, stance or swing
 * A sigma of 0 SELECTS the input: nothing is added (-0 and NaN payloads keep their bits; the quaternion is not renormalised) and that channel's draws are skipped
 * unless z_out asks for them.  A non-finite input of one robot stays with that robot.
 * What it is not: white Gaussian noise and a random-walk bias only -- no quantisation, no latency, no dropout, no temperature or scale-factor model, no correlation
 * between channels or in time; and the bias is not estimated by anything: the tick's EKF has no bias states, so it sees the bias as a constant error.
 * Refused with A1MPC_ERR_INVALID_ARGUMENT (a1mpc_last_error names the field) before any launch, every array left untouched: a null handle or cfg, n < 0, a sigma or
 * walk that is negative or not finite, a walk > 0 with imu_bias NULL, robot0 + n > 2^32, two arrays that overlap.  n > max_batch is A1MPC_ERR_BATCH_TOO_LARGE.
 * n == 0 is A1MPC_OK and launches nothing.  Host pointers (staged like the other caller-side entries), or (_device) device pointers, asynchronous on hip_stream
 * (NULL = the handle's) and ordered like every other _device entry.
 */
typedef struct a1mpc_noise_config {
    uint64_t seed;
    double gyro_sigma, acc_sigma;            /* rad/s, m/s^2: white, per sample */
    double gyro_bias_walk, acc_bias_walk;    /* std of the bias increment per call */
    double att_sigma;                        /* rad: a small body-frame rotation on the quaternion */
    double joint_pos_sigma, joint_vel_sigma; /* rad, rad/s */
    double foot_force_sigma;                 /* N */
} a1mpc_noise_config;
void a1mpc_default_noise_config(a1mpc_noise_config* cfg);   /* seed 0, every sigma 0: off */
a1mpc_status a1mpc_sensor_noise_batch(a1mpc_handle h, const a1mpc_noise_config* cfg, int32_t n, uint64_t robot0, uint64_t tick, double* quat, double* imu_acc_raw,
                                      double* imu_gyro_raw, double* joint_pos, double* joint_vel, double* foot_force, double* imu_bias, double* z_out);
a1mpc_status a1mpc_sensor_noise_batch_device(a1mpc_handle h, const a1mpc_noise_config* cfg, int32_t n, uint64_t robot0, uint64_t tick, double* d_quat,
                                             double* d_imu_acc_raw, double* d_imu_gyro_raw, double* d_joint_pos, double* d_joint_vel, double* d_foot_force,
                                             double* d_imu_bias, double* d_z_out, void* hip_stream);

/*
 * Episode record and batch summary for closed-loop runs, on the device.  The loop  sensors -> noise -> control tick -> plant step  never leaves the GPU; this is its
 * last stage: a1mpc_episode_update_batch_device, called once per tick behind the plant step on the loop's stream, keeps 16 doubles per robot -- whether it stayed up and
 * until when, how well it tracked its command, how well the estimator tracked the plant -- and a1mpc_episode_summary_batch_device reduces n records to 20 numbers, so
 * that a run of 65 536 robots is read with one small copy at its end.  Two kernels and a family of their own, a1mpc_episode_*: the entries above are unchanged.
 *
 * UPDATE.  in (all device pointers in the _device entry, host pointers staged like the other caller-side entries otherwise):
 *        state, state_stride   n x 12 / 13 / 22, the plant's truth: pos = state[3:6) and v = state[9:12) are read
 *        R_world               n x 9 row-major, the truth attitude
 *        root_pos, root_lin_vel   n x 3 each, the tick's estimate (a1mpc_tick_buffers); optional, as a pair
 *        root_lin_vel_d        n x 3, the body-frame command (x and y are read); optional
 *        root_pos_d_z          n; optional
 *        ground                n x 3, z0, sx, sy as in a1mpc_ground_step_batch; optional (NULL: the plane z = 0)
 *        grf_body, contacts    n x 12 doubles, n x 4 bytes; optional, as a pair
 *        status                n int32, the solver's; optional        reach   n x 4 bytes; optional
 *        tick                  by value, below 2^53 - 1               cfg     min_up, min_height (a1mpc_default_episode_config: 0.5, 0.12)
 * in / out  episode  n x 16 doubles, owned by the caller; the handle gets no state.  An all-zero record is the start of an episode: a memset is a reset.
 *   word  0 ticks            updates accumulated            1 end_tick_p1   0 while alive, else tick + 1 of the update that ended the episode
 *         2 end_code         0 alive, 1 non-finite input, 2 tilt, 3 height
 *         3 vel_err_sum      += ex ex + ey ey;  vb_k = (R0k v0 + R1k v1) + R2k v2 (vb = R^T v),  e = vb - root_lin_vel_d
 *         4 height_err_sum   += ez ez;  ez = (pos_z - hz) - root_pos_d_z,  hz = (z0 + sx pos_x) + sy pos_y, or +0 without ground
 *         5 tilt_max         max of 1 - R22
 *         6 est_pos_err_sum  += (dx dx + dy dy) + dz dz, d = root_pos - pos      7 est_vel_err_sum  the same on root_lin_vel - v      8 est_vel_err_max  max of 7's term
 *         9 effort_sum       += (s0 + s1) + (s2 + s3);  s_l = (fx fx + fy fy) + fz fz on a stance leg, +0 selected on a swing leg
 *        10 fz_max           max over stance legs of the body-frame fz           11 solver_bad  += 1 when status != 1       12 reach_bad  += legs with reach != 0
 *        13, 14 x0, y0       pos_x, pos_y of the first accumulated update (the one that finds ticks == 0)
 *        15 dist2            (pos_x - x0)^2 + (pos_y - y0)^2 of the latest accumulated update
 * Per robot, in this order: (1) a record with end_code != 0 keeps every bit: it is frozen.  (2) If any value this robot's rules read is not finite -- pos, v, R, the
 * estimate, the command's x and y, root_pos_d_z, its ground row, the forces of its STANCE legs (a swing leg's force is selected away and not tested, as in the plant)
 * -- end_code = 1, end_tick_p1 = tick + 1, and nothing else changes.  (3) R22 < min_up ends with code 2.  (4) pos_z - hz < min_height ends with code 3.  (5) Otherwise
 * every word whose inputs are given is accumulated; a word whose input is NULL keeps its bits.  A maximum is (x > m) ? x : m.  The update that ends an episode
 * accumulates nothing.
 * Arithmetic: IEEE + - * and comparisons only, contraction off, no fused multiply-add, sums in the order written.  A robot's record is a pure function of its own
 * inputs: the same bits at every batch size, position in the batch and entry.
 *
 * SUMMARY.  summary_out, 20 doubles (device-resident in the _device entry):
 *   word  0 n       1 .. 4 records with end_code 0 / 1 / 2 / 3       5 the smallest end_tick_p1 - 1 over ended records, -1 when none ended
 *         6 sum of ticks   7 of vel_err_sum   8 of height_err_sum   9 max of tilt_max   10 the LOWEST row that attains word 9   11 sum of est_pos_err_sum
 *        12 sum of est_vel_err_sum   13 max of est_vel_err_max   14 sum of effort_sum   15 max of fz_max   16 sum of solver_bad   17 of reach_bad   18 sum of dist2
 *        19 max of dist2
 * Every sum is over all n rows, frozen records included, and is DEFINED by a balanced tree: the column padded to the next power of two with +0, then x'[i] = x[2i] +
 * x[2i + 1] until one value is left.  It does not depend on the launch geometry (every summed word of a record is at least +0, so the + (+0) of the radix-64 levels
 * the kernel uses is exact).  No atomics: a1mpc_episode_reduce_kernel runs level by level, 64 rows per wavefront, the levels separated by launches on the stream; the
 * partials live in a workspace sized from max_batch at a1mpc_create.
 * What it is not: no reset of the handle's state (EKF, contact filters) for a robot that fell -- a fallen robot's record freezes, its loop goes on (a1mpc_respawn_batch below starts it again); no quantiles or
 * histograms; sums, not means (divide by word 6 or word 0 yourself); one batch, not merged across shards or handles.
 * Refused with A1MPC_ERR_INVALID_ARGUMENT (a1mpc_last_error names the field) before any launch, every array left untouched: a null handle (first), cfg, state, R_world
 * or episode; a stride other than 12 / 13 / 22; n < 0; min_up outside [-1, 1] or not finite; min_height not finite; tick >= 2^53 - 1; half of a pair (root_pos /
 * root_lin_vel, grf_body / contacts); episode overlapping an input; for the summary a null handle, episode or summary_out, n < 0, summary_out overlapping episode.
 * n > max_batch is A1MPC_ERR_BATCH_TOO_LARGE.  n == 0 is A1MPC_OK, launches nothing and writes nothing.  The _device entries are asynchronous on hip_stream (NULL = the
 * handle's) and ordered like every other _device entry.
 */
typedef struct a1mpc_episode_config {
    double min_up;      /* the episode ends (code 2) when R22 falls below it: 0.5 is a tilt of 60 degrees */
    double min_height;  /* ... (code 3) when the body is less than this above its ground, m */
} a1mpc_episode_config;
void a1mpc_default_episode_config(a1mpc_episode_config* cfg);   /* 0.5, 0.12 */
a1mpc_status a1mpc_episode_update_batch(a1mpc_handle h, const a1mpc_episode_config* cfg, int32_t n, uint64_t tick, const double* state, int32_t state_stride,
                                        const double* R_world, const double* root_pos, const double* root_lin_vel, const double* root_lin_vel_d, const double* root_pos_d_z,
                                        const double* ground, const double* grf_body, const uint8_t* contacts, const int32_t* status, const uint8_t* reach, double* episode);
a1mpc_status a1mpc_episode_update_batch_device(a1mpc_handle h, const a1mpc_episode_config* cfg, int32_t n, uint64_t tick, const double* d_state, int32_t state_stride,
                                               const double* d_R_world, const double* d_root_pos, const double* d_root_lin_vel, const double* d_root_lin_vel_d,
                                               const double* d_root_pos_d_z, const double* d_ground, const double* d_grf_body, const uint8_t* d_contacts,
                                               const int32_t* d_status, const uint8_t* d_reach, double* d_episode, void* hip_stream);
a1mpc_status a1mpc_episode_summary_batch(a1mpc_handle h, int32_t n, const double* episode, double* summary_out);
a1mpc_status a1mpc_episode_summary_batch_device(a1mpc_handle h, int32_t n, const double* d_episode, double* d_summary_out, void* hip_stream);

/*
 * Respawn: a robot whose episode is over gets its lane back, on the device.  Behind the episode update of a closed loop, a1mpc_respawn_batch_device decides per robot
 * whether its episode is to start again, clears that robot's state in the handle and holds it for a few ticks while its estimator is primed;
 * a1mpc_respawn_rows_device then puts the caller's own rows back.  Every robot is on its own episode clock (word 0 of its record) and nothing is read back per tick.
 * A family of its own, a1mpc_respawn_*, two kernels (a1mpc_respawn_kernel, a1mpc_respawn_rows_kernel): the entries above are unchanged.
 *
 * MASKED RESET.  a1mpc_respawn_reset_batch(_device): for every robot b < n with mask[b] & 1, every byte of that robot's state that the whole-handle reset of each bit
 * of `what` zeroes is zeroed, and no other byte of the handle changes:
 *   A1MPC_RESPAWN_EKF      a1mpc_reset_ekf_state: the robot's row of the filter state (x, P and the flag word; a zero flag word is a new filter, which the init kernel
 *                          takes on the next EKF launch).  With n > 0 the handle forgets which robots have been initialised, so that the next EKF launch runs its init
 *                          kernel again: that kernel returns at once for every robot whose flag word is not zero
 *   A1MPC_RESPAWN_CONTACT  a1mpc_reset_contact_state: its contact record, its leg windows and its word of every slot of the terrain window
 *   A1MPC_RESPAWN_SENSOR   a1mpc_reset_sensor_state: its word of every slot, sum and correction of the six IMU filters, its count and cursor.  The window the state was
 *                          built with stays: a masked reset does not license another imu_window
 *   A1MPC_RESPAWN_WARM     a1mpc_reset_warm_start: its carried iterates and rho and, once allocated, its record of the update path's carry.  The queue order of the next
 *                          solve stays (it is scheduling only: results do not depend on it)
 * A block that is not allocated yet is skipped.  From the call on a reset robot gives, bit for bit in every output of every entry, what the same batch position gives on
 * a handle on which the whole-handle resets were called at that point; every other robot gives what it gives on a handle that saw no reset.  The _device entry is
 * asynchronous on hip_stream (NULL = the handle's), ordered like every other _device entry, and does not synchronise -- the whole-handle resets do.
 *
 * DECISION.  a1mpc_respawn_batch(_device), once per tick behind a1mpc_episode_update_batch(_device):
 *   in / out  episode       n x 16 doubles, the records of the episode update
 *             life          n x 2 int32, owned by the caller: [hold, episodes_done]; all zero = nobody held, nothing finished
 *   out       finished_out  n x 16 doubles, optional: the record an episode ended with, taken when its robot is respawned; a row the call does not write keeps its bits
 *             mask_out      n bytes: 0 left alone, 1 respawned, 2 held
 * Per robot, in this order:  (1) hold > 0: HELD -- every word of the record becomes +0, hold -= 1, mask_out = 2.  The record is not consulted: a held robot is stepped
 * and then put back (rows, below), so whatever the step made of it, a NaN included, ends no episode.  (2) Otherwise, if end_code == c for a c of 1 .. 3 with bit c of
 * cfg->codes set, or end_code == 0, cfg->max_ticks > 0 and ticks >= max_ticks: RESPAWNED -- the 16 words go to finished_out[b] when given, the record becomes +0, hold =
 * cfg->hold_ticks, episodes_done += 1, mask_out = 1, and the robot's state in the handle is cleared as by the masked reset with cfg->what, in the same launch.
 * (3) Otherwise mask_out = 0 and nothing else is written.  Copies, comparisons and integer arithmetic only.
 * With life[b][0] = hold_ticks at the start of a run the first hold_ticks ticks are held: the priming of a fresh estimator on an unstepped plant, per robot.  After a
 * respawn the robot is held for exactly hold_ticks ticks and its record starts from zero on the first free tick.
 *
 * ROWS.  a1mpc_respawn_rows_device: the loop's other state (the plant's rows, the tick's carried arrays, the command state, imu_bias) is the caller's, and only the
 * caller knows its spawn values.  For each of n_rows <= A1MPC_RESPAWN_ROWS_MAX table entries and every robot b < n whose mask value selects the entry (`when` bit 0: on
 * mask 1, bit 1: on mask 2; any other mask value selects nothing), row b of dst becomes row b of src (src_rows >= n) or its row 0 (src_rows == 1): copied, never
 * computed; every other byte is untouched.  8-byte words where row_bytes and both pointers are multiples of 8, bytes otherwise.  Typically the plant's rows carry when =
 * 3 (put back on every held tick: an unstepped plant) and the rest when = 1.  There is no host-pointer variant: a host caller has mask_out and its own arrays.
 *
 * What it is not: one handle only, not the pipeline or the sharded handles (a1mpc_sharded_handle gives a shard's handle for the masked reset); spawn poses are the
 * caller's templates, nothing is randomised; finished_out keeps only a robot's latest finished record; a held robot's plant step is computed and discarded.
 * Refused with A1MPC_ERR_INVALID_ARGUMENT (a1mpc_last_error names the field) before any launch, every array left untouched: a null handle (first), cfg, episode, life,
 * mask_out, mask or rows; n < 0; `what` or codes with unknown bits (bit 0 of codes included); hold_ticks < 0; max_ticks >= 2^53; n_rows outside 0 .. 16; a null dst or
 * src; row_bytes outside 1 .. 4096; src_rows neither 1 nor >= n; `when` 0 or with unknown bits; dst overlapping its src; finished_out or mask_out overlapping episode.
 * n > max_batch is A1MPC_ERR_BATCH_TOO_LARGE.  n == 0 is A1MPC_OK and launches nothing.
 */
#define A1MPC_RESPAWN_EKF 1u
#define A1MPC_RESPAWN_CONTACT 2u
#define A1MPC_RESPAWN_SENSOR 4u
#define A1MPC_RESPAWN_WARM 8u
#define A1MPC_RESPAWN_ROWS_MAX 16
typedef struct a1mpc_respawn_config {
    uint32_t codes;      /* bit c: an episode that ended with end_code c (1 non-finite, 2 tilt, 3 height) is respawned */
    uint64_t max_ticks;  /* > 0: a live episode whose ticks has reached it is respawned too (a time limit); 0: none */
    int32_t hold_ticks;  /* ticks a respawned robot is held at its spawn rows while its estimator is primed */
    uint32_t what;       /* A1MPC_RESPAWN_* bits cleared for a respawned robot */
} a1mpc_respawn_config;
typedef struct a1mpc_respawn_rows {
    void* dst;
    const void* src;
    int32_t row_bytes;
    int32_t src_rows;    /* 1: one template row for every robot; >= n: row b */
    uint32_t when;       /* bit 0: on mask 1 (respawned), bit 1: on mask 2 (held) */
} a1mpc_respawn_rows;
void a1mpc_default_respawn_config(a1mpc_respawn_config* cfg);   /* codes 0xE, max_ticks 0, hold_ticks 10, what 0xF */
a1mpc_status a1mpc_respawn_reset_batch(a1mpc_handle h, int32_t n, const uint8_t* mask, uint32_t what);
a1mpc_status a1mpc_respawn_reset_batch_device(a1mpc_handle h, int32_t n, const uint8_t* d_mask, uint32_t what, void* hip_stream);
a1mpc_status a1mpc_respawn_batch(a1mpc_handle h, const a1mpc_respawn_config* cfg, int32_t n, double* episode, int32_t* life, double* finished_out, uint8_t* mask_out);
a1mpc_status a1mpc_respawn_batch_device(a1mpc_handle h, const a1mpc_respawn_config* cfg, int32_t n, double* d_episode, int32_t* d_life, double* d_finished_out,
                                        uint8_t* d_mask_out, void* hip_stream);
a1mpc_status a1mpc_respawn_rows_device(a1mpc_handle h, int32_t n, const uint8_t* d_mask, const a1mpc_respawn_rows* rows, int32_t n_rows, void* hip_stream);

/*
 * Debug / verification: the dense QP data the reference's ConvexMpc keeps in its public members after calculate_qp_mats
 * (hessian, gradient, lb, ub: S/ConvexMpc.h:84-93, S/ConvexMpc.cpp:158-245) for n problems, formed on the GPU from the same inputs as
 * a1mpc_solve_batch_strided.  P_out n x (12H)^2 (row-major, symmetric), g_out n x 12H, l_out / u_out n x 20H (the constraint matrix is
 * the constant stencil of S/ConvexMpc.cpp:46-58).  The solver itself never forms these; callers that poke the members
 * (S/A1RobotControl.cpp:527-537, S/test/test_mpc.cpp:136-140) get them through include/a1mpc_dropin.hpp.  Host pointers; allocates
 * and frees its own device buffers; not a per-tick call.
 */
a1mpc_status a1mpc_form_qp_batch(a1mpc_handle h, int32_t n, const double* x0, const double* x_ref, const double* R_world,
                                 const double* foot_abs, int32_t foot_stride, const uint8_t* contact, int32_t contact_stride,
                                 const double* yaw_A, double* P_out, double* g_out, double* l_out, double* u_out);

/* Work-queue order of batches larger than the resident set: history = 1 (default) issues the QPs longest-first by the cost
 * (iterations + factor passes) each one had in the previous solve of this handle with the same n -- the same robots tick after
 * tick; history = 0 is plain index order.  The first solve of a batch size, the solve after a1mpc_reset_warm_start and the solve after
 * this call have no history: their queue is ordered by a cost guess the set-up kernel derives from each QP's velocity error.
 * Scheduling only: no returned number depends on it.  Environment override at create: A1MPC_SCHEDULE=index. */
a1mpc_status a1mpc_set_schedule(a1mpc_handle h, int32_t history);

/* forget the carried (x, y, rho) of every problem: next solve is a cold start */
a1mpc_status a1mpc_reset_warm_start(a1mpc_handle h);

/* Read / write the carried OSQP workspace of problems 0..n-1 (the reference keeps it inside its persistent
 * OsqpEigen::Solver member, S/A1RobotControl.h:67): x n x 12H (world-frame forces), y n x 20H (reference row order), rho n
 * (0 = "start from settings.rho").  Any pointer may be NULL.  Host pointers; synchronises the handle's stream.  A solve whose
 * solution is not finite leaves x = y = 0 behind, i.e. the next tick of that problem starts from cold iterates (OSQP's store_solution()
 * cold-starts its iterates after a failed solve), so one bad tick cannot poison the ticks after it -- and, since round 4, the rho the
 * solver had reached, exactly as OSQP's cold_start() leaves the adapted rho in settings->rho (the reference ignores the solver's return
 * code, S/A1RobotControl.cpp:540, so its next tick does run with that rho; engine and oracle used to restart from the configured rho).
 * With warm_start = 2 an injected state is re-expressed on the update path's workspace the way osqp_warm_start_x / _y do it on the
 * reference's persistent solver (round 4): x and y replace the carried iterates, z becomes A x, the previous tick's scalings and gradient
 * stay, and the next tick follows the update path from there (until round 4 an injected state cleared the carry and the next tick was a
 * fresh set-up). */
a1mpc_status a1mpc_warm_start(a1mpc_handle h, int32_t n, const double* x, const double* y, const double* rho);
a1mpc_status a1mpc_get_warm_start(a1mpc_handle h, int32_t n, double* x_out, double* y_out, double* rho_out);
/* warm_start = 2 only: the unscaled z = Pi(w) of problems 0..n-1 that the update path keeps beside (x, y, rho) -- what OSQP leaves in work->z, n x 20H in the
 * reference's row order (S/ConvexMpc.cpp:46-58).  With x and y it is everything OSQP's own termination test reads (auxil.c check_termination: ||Ax - z||,
 * ||Px + q + A'y||), so a caller -- the parity tests do, on the ticks where engine and oracle stop at different iterations -- can verify that a returned point is
 * one OSQP would have stopped at.  A1MPC_ERR_INVALID_ARGUMENT when the handle has no update-path carry (another warm-start mode, horizon 1, no tick yet).
 * Host pointer; synchronises the handle's stream.  Problems without a previous update-path tick read as zeros. */
a1mpc_status a1mpc_get_workspace_z(a1mpc_handle h, int32_t n, double* z_out);
/* warm_start = 2 only: the equilibration of the handle's last update-path tick as OSQP's workspace holds it -- D (n x 12H, variable scaling), E (n x 20H,
 * constraint scaling, reference row order) and the cost scaling c (n; 0 = no previous tick).  Together with a1mpc_get_warm_start (unscaled x, y, rho) and
 * a1mpc_get_workspace_z this is the complete state the reference's persistent OsqpEigen solver carries from tick to tick (scaled iterates x_s = x / D,
 * z_s = E z, y_s = c y / E): a second implementation of the update path can be started from it (the parity tests re-seed the oracle that way).
 * Any pointer may be NULL.  Host pointers; synchronises the handle's stream. */
a1mpc_status a1mpc_get_workspace_scaling(a1mpc_handle h, int32_t n, double* D_out, double* E_out, double* c_out);
/* Stage counters of the solve (the reference brackets its tick with stopwatches t1..t6, S/A1RobotControl.cpp:491-553; a1mpc_last_stage_ms gives
 * set-up | solve by HIP events).  a1mpc_set_profiling(h, 1): batches that go through the split pipeline (more QPs than the resident rows; horizon > 1,
 * warm_start != 2, contacts broadcast) run a clock-stamped instantiation of the persistent ADMM kernel -- the same arithmetic, the same results bit for bit,
 * shader-clock stamps around every factor pass, iteration segment and residual check (outside the hot loop).  a1mpc_last_stage_cycles then returns the cycles
 * summed over the QPs of the last profiled solve: [0] Riccati factor passes, [1] ADMM iterations, [2] residual checks + rho updates; *qps_out = the number of
 * QPs summed (0: the last solve was not profiled).  A QP's cycles include the time its wavefront spent on its wave-mate's divergent stages; the three sums'
 * ratio splits a1mpc_last_stage_ms' solve stage.  Host call; synchronises the handle's stream. */
a1mpc_status a1mpc_set_profiling(a1mpc_handle h, int32_t on);
a1mpc_status a1mpc_last_stage_cycles(a1mpc_handle h, double* cycles3_out, int32_t* qps_out);
/* The same stopwatches for the tick the reference actually runs (round 5): with profiling on, a solve that goes through the fused or the latency kernel at horizon 10
 * -- every warm-started closed-loop tick of a known batch up to 8192 robots, every batch of <= 256 QPs, i.e. the batch-1 control tick, in all three warm-start
 * semantics -- runs a clock-stamped instantiation of that kernel (same arithmetic, same results bit for bit) and this call returns the shader-clock cycles summed over
 * its QPs, in the order of the reference's tick (S/A1RobotControl.cpp:446-562):
 *   [0] formation: inputs, B~, gradient roll-out + adjoint, the two 12x12 Hessian blocks        (calculate_A/B_mat_c .. calculate_qp_mats, :491-520)
 *   [1] the Ruiz equilibration passes + cost scaling                                            (osqp_setup / osqp_update_P: scale_data)
 *   [2] hot state (rho vector, warm-start iterates, update-path carry) + set-up -> solver hand-off
 *   [3] Riccati factor passes   [4] ADMM iterations (OSQP's first iteration included)   [5] residual checks + rho updates        (solver.solve(), :540)
 *   [6] outputs: R' f, the carried workspace (x, y, rho; update path: z, scalings)                (:555-561, store_solution)
 *   [7] the whole tick, entry to exit (= the sum of [0..6])
 * A wavefront's QPs share its instruction stream: a QP's cycles include its wave-mate's.  *qps_out = QPs summed (0: the last solve was not such a tick -- a
 * split-pipeline solve reports through a1mpc_last_stage_cycles).  Host call; synchronises the handle's stream. */
a1mpc_status a1mpc_last_tick_stage_cycles(a1mpc_handle h, double* cycles8_out, int32_t* qps_out);
/* Which warm-start semantics the handle's last MPC solve actually ran: 0 (cold), 1 (fresh set-up + osqp_warm_start) or 2 (the reference's update path).
 * warm_start = 2 exists at every horizon > 1 on the fast path and on the general path (per-step feet, a separate A_c yaw: its latency and fused kernels -- round 6:
 * at every batch size, an update-path batch beyond the resident rows runs the fused kernel in several rounds); a solve at horizon 1, or a general-path batch forced onto
 * its split pipeline by A1MPC_PIPELINE=split, runs mode 1 instead (documented at a1mpc_config.warm_start) -- this call makes that visible to the caller.  -1 before the
 * first solve. */
a1mpc_status a1mpc_last_warm_start_mode(a1mpc_handle h, int32_t* mode_out);

/* Replace the configuration of a live handle -- everything except the horizon: dt (the reference uses the measured loop dt when
 * use_sim_time is "true", S/A1RobotControl.cpp:465), weights, mass / inertia, friction and force limits, OSQP settings.  The constants
 * travel to the kernels by value with every launch, so this costs nothing, keeps the carried warm start and takes effect with the
 * next call.  Validated like a1mpc_create; a refused configuration leaves the handle's configuration as it was. */
a1mpc_status a1mpc_update_config(a1mpc_handle h, const a1mpc_config* cfg);

/* The handle's HIP timing events (around every launch: a1mpc_last_kernel_ms, a1mpc_last_stage_ms, a1mpc_last_control_tick_ms read them) on (default) / off.  An event
 * record is a packet of its own on the GPU's queue; a 400 Hz control loop that never reads the instrumentation can turn it off -- three records less per MPC tick, four
 * per control tick (batch-1 p50 -5 us; a chained control tick -15..-18 us at 4096 robots: each record is a marker packet in front of which the command processor drains
 * the queue, 5-6 us -- kernel trace and the round-5 "timing off is slower" artefact explained in profiles/r06_control_tick_timeline.md).  With timing off the three calls
 * above return A1MPC_ERR_INVALID_ARGUMENT ("no kernel has been launched ...").  No result depends on it. */
a1mpc_status a1mpc_set_timing(a1mpc_handle h, int32_t on);

/* instrumentation: duration of the last kernel launched through this handle (HIP events on its stream;
 * synchronises that stream), bytes of dynamic LDS per workgroup and QPs per workgroup of the horizon's kernel */
a1mpc_status a1mpc_last_kernel_ms(a1mpc_handle h, float* ms_out);
a1mpc_status a1mpc_kernel_info(a1mpc_handle h, int32_t* lds_bytes_per_workgroup, int32_t* qps_per_workgroup,
                               int32_t* threads_per_workgroup);

/* Stage split of the last MPC launch, the engine's counterpart of the reference's t1..t6 stopwatches (S/A1RobotControl.cpp:491-553;
 * "form" = calculate_A/B_mat_c + discretisation + calculate_qp_mats + OSQP set-up, "solve" = solver.solve()): form_ms = the set-up kernel
 * (formation + Ruiz equilibration, + the queue-order kernel), solve_ms = the persistent ADMM kernel (factorisations + iterations + output).
 * Batches that run the fused / latency kernel are one launch: form_ms = 0, solve_ms = the whole launch.  Per-QP iteration counts come with
 * every solve (iters_out), factorisation counts from a1mpc_last_nfact.  Synchronises the launch. */
a1mpc_status a1mpc_last_stage_ms(a1mpc_handle h, float* form_ms_out, float* solve_ms_out);

/* number of KKT (Riccati) factorisations each QP of the last MPC / balance launch performed (1 + rho updates);
 * synchronises the handle's stream; instrumentation for the work model of bench.py */
a1mpc_status a1mpc_last_nfact(a1mpc_handle h, int32_t n, int32_t* nfact_out);

/*
 * The batch sharded over the GPUs of one node behind ONE handle and one host thread (SURVEY 8b "device = -1 = all", 8e): shard g solves a
 * contiguous slice (sizes differ by at most one, remainder to the low shards) on devices[g] with its own engine handle and stream; the QPs
 * are independent, so there is no data-path collective -- only scatter-inputs / gather-results, by one of two transports:
 *   transport 0  pinned host memory, one asynchronous copy fan-out per device each way (every GPU over its own PCIe link)
 *   transport 1  RCCL over xGMI: one copy of the whole batch to devices[0], grouped ncclSend / ncclRecv to the other devices and back
 *                (librccl.so is dlopen()ed by this call; distinct devices required)
 * devices NULL or n_devices <= 0 = every visible device.  A device may be listed twice with transport 0 (two shards on one GPU).
 * max_batch is the TOTAL batch.  Warm start, if configured, is carried per shard, i.e. per position in the batch as long as n stays the same.
 * Host pointers; layouts as a1mpc_solve_batch.
 */
typedef struct a1mpc_sharded_s* a1mpc_sharded;
a1mpc_status a1mpc_sharded_create(const a1mpc_config* cfg, int32_t max_batch, const int32_t* devices, int32_t n_devices, int32_t transport,
                                  a1mpc_sharded* out);
a1mpc_status a1mpc_sharded_solve_batch(a1mpc_sharded s, int32_t n, const double* x0, const double* x_ref, const double* R_world,
                                       const double* foot_abs, const uint8_t* contact, double* grf_body_out, int32_t* iters_out,
                                       int32_t* status_out);
/* Round 6: the closed loop on all GPUs.  The same sharded solve for the compact tick records (a1mpc_solve_batch_ticks: S/A1RobotControl.cpp:452-488 on the device), and for a batch that
 * is RESIDENT ON SHARD 0's GPU (device pointers of that device; layouts of a1mpc_solve_batch_device / _ticks_device): the root feeds the other shards over xGMI -- peer copies
 * with transport 0, grouped ncclSend / ncclRecv with transport 1 -- solves its own shard in place and collects every shard's GRFs / iterations / status in the caller's output
 * arrays on the root ("RCCL over xGMI only to scatter inputs / gather GRFs", the north_star).  hip_stream: a stream of the root device the inputs were produced on (the shards
 * start behind it; NULL: the inputs are ready).  The calls return when the outputs are complete.  Every shard's engine handle carries its own warm start: with
 * cfg.warm_start = 1 or 2 and a constant n, tick after tick through any of these entries is the closed loop of the single-GPU handle, shard by shard (a1mpc_sharded_handle
 * gives a shard's handle for a1mpc_reset_warm_start / a1mpc_get_warm_start / the instrumentation calls).  a1mpc_sharded_last_transfer: the bytes the last solve moved from the
 * root to the other shards and back (1968 B + 104 B per QP at h = 16). */
a1mpc_status a1mpc_sharded_solve_batch_ticks(a1mpc_sharded s, int32_t n, const double* tick, const double* R_world, const double* foot_abs,
                                             const uint8_t* contact, double* grf_body_out, int32_t* iters_out, int32_t* status_out);
a1mpc_status a1mpc_sharded_solve_batch_device(a1mpc_sharded s, int32_t n, const double* d_x0, const double* d_x_ref, const double* d_R_world,
                                              const double* d_foot_abs, const uint8_t* d_contact, double* d_grf_body_out, int32_t* d_iters_out,
                                              int32_t* d_status_out, void* hip_stream);
a1mpc_status a1mpc_sharded_solve_batch_ticks_device(a1mpc_sharded s, int32_t n, const double* d_tick, const double* d_R_world, const double* d_foot_abs,
                                                    const uint8_t* d_contact, double* d_grf_body_out, int32_t* d_iters_out, int32_t* d_status_out,
                                                    void* hip_stream);
a1mpc_status a1mpc_sharded_handle(a1mpc_sharded s, int32_t shard, a1mpc_handle* out);
a1mpc_status a1mpc_sharded_last_transfer(a1mpc_sharded s, int64_t* scatter_bytes, int64_t* gather_bytes);
a1mpc_status a1mpc_sharded_info(a1mpc_sharded s, int32_t* n_shards, int32_t* devices_out, int32_t* transport);
void a1mpc_sharded_destroy(a1mpc_sharded s);

/*
 * Batch pipeline: consecutive batches in flight together on ONE device (north_star: "HIP streams"; the reference has no counterpart -- it
 * solves one QP per tick on one thread, S/MainGazebo.cpp:57-68).  A launch of a few thousand QPs ends in a tail: its few 150-225-iteration
 * QPs keep a handful of wavefronts busy while the rest of the chip idles (the last 0.15-0.25 ms of a 0.85 ms launch at 4096 x h10).  The
 * pipeline owns `depth` complete engine handles (0 = the default: 2) on `depth` HIP streams and hands batches to them round-robin, so the
 * next batch's set-up kernel and persistent rows are dispatched onto the SIMDs the tail has left.  Batches in flight share nothing
 * (prepared-state records, queue, warm start are per slot): results are bit-identical to a lone handle's.  Measured on one MI355X, first
 * solves of distinct batches (profiles/r03_bench_default_run.json, r03_bench_depth1_run.json): 4096 x h10 4.2-5.0 M -> 6.35-6.44 M solves/s,
 * 8192 x h16 2.23 -> 2.47 M; depth 3 no longer pays (profiles/r03_pcie_probe_4096_h10.json); 16 384 x h10 neutral; a batch of 65 536 QPs
 * fills the chip on its own and loses 7 % when pipelined -- submit those through a plain handle.
 * Round 6 (kernel traces of the slots, profiles/r06_setup_ahead.md): what is left between two slots and one 65 536-QP launch (0.60-0.61 against 0.57-0.58 ms per 4096 x h10
 * batch) is the chain set-up kernel -> queue-order kernel -> persistent kernel of every batch, each of which finds the chip full; a third slot is worth 3-4 % when the
 * caller submits in a free-running loop and loses 11-19 % when it starts its slots behind one event, so the default stays two.  A slot of a two-slot pipeline runs the
 * general path's one-wave persistent kernel at horizon 10 (six QPs per CU) instead of the CU-wide one (seven): the other slot's set-up then runs beside it (+6 % at
 * 4096 QPs, +12 % at 2560; same bits).
 *   submit   device pointers, layouts of a1mpc_solve_batch_device.  slot = -1: next slot round-robin (returned in *slot_out), or a fixed
 *            slot (a robot population that is warm-started must stay on its slot: the carried OSQP workspace lives there).
 *            fresh_batch != 0: these QPs are new to the slot, order its queue by the set-up kernel's cost guess instead of the slot's
 *            previous batch (a1mpc_set_schedule).  inputs_ready_stream: the slot starts after everything queued on that stream so far
 *            (NULL = the inputs are ready now).  Returns at once; the outputs of a slot are valid after a1mpc_pipeline_wait / _join, and
 *            its output buffers must not be handed to another submit before that.
 *   submit (host pointers)  a1mpc_pipeline_submit: the arrays of a1mpc_solve_batch -- what a caller on the reference's side of the boundary has
 *            (S/A1RobotControl.h:44: A1CtrlStates in, a 3x4 matrix out).  Inputs are snapshotted into the slot's pinned block before the call
 *            returns (the caller may overwrite them at once); H2D copy, launches and D2H copy are queued on the slot's stream.  The OUTPUT arrays
 *            are written by the a1mpc_pipeline_wait (or by the next submit) that retires the slot: they must stay valid until then.  The
 *            caller's thread snapshots batch k + 1 while the GPU solves batch k.
 *   wait     the host waits for the slot's last submit (slot -1 = every slot) and hands a host-pointer batch to its output arrays;
 *            join: a caller's stream waits for it instead (device-pointer submits only).
 *   handle   the slot's engine handle, for warm-start I/O, a1mpc_update_config and the instrumentation calls.
 * One host thread per pipeline.
 */
typedef struct a1mpc_pipeline_s* a1mpc_pipeline;
a1mpc_status a1mpc_pipeline_create(const a1mpc_config* cfg, int32_t max_batch, int32_t device, int32_t depth, a1mpc_pipeline* out);
a1mpc_status a1mpc_pipeline_submit_device(a1mpc_pipeline p, int32_t slot, int32_t fresh_batch, int32_t n, const double* d_x0,
                                          const double* d_x_ref, const double* d_R_world, const double* d_foot_abs, const uint8_t* d_contact,
                                          double* d_grf_body_out, double* d_u_full_out, int32_t* d_iters_out, int32_t* d_status_out,
                                          void* inputs_ready_stream, int32_t* slot_out);
a1mpc_status a1mpc_pipeline_submit(a1mpc_pipeline p, int32_t slot, int32_t fresh_batch, int32_t n, const double* x0, const double* x_ref,
                                   const double* R_world, const double* foot_abs, const uint8_t* contact, double* grf_body_out,
                                   double* u_full_out, int32_t* iters_out, int32_t* status_out, int32_t* slot_out);
/* Round 6: the other two input forms of the MPC entry with batches in flight together -- per-step feet / contact schedules / an A_c yaw of its own (the general path of
 * the reference's INTERFACE: B_mat_d_list, S/ConvexMpc.h:74, driven by S/test/test_mpc.cpp:106-122; arguments of a1mpc_solve_batch_strided(_device)) and the compact tick
 * records (S/A1RobotControl.cpp:452-488; arguments of a1mpc_solve_batch_ticks_device).  A first solve of the general path is bounded by its longest QPs and no feature of
 * the inputs predicts them (profiles/r05_general_path_order.txt): the tail is what a second batch in flight fills.  Slots, events, fresh_batch, inputs_ready_stream and
 * the life time of the output arrays are those of a1mpc_pipeline_submit_device / a1mpc_pipeline_submit; results are bit-identical to the lone handle's entry points.
 * (foot_stride, contact_stride, yaw_A) = (0, 0, NULL) IS a1mpc_pipeline_submit(_device). */
a1mpc_status a1mpc_pipeline_submit_strided_device(a1mpc_pipeline p, int32_t slot, int32_t fresh_batch, int32_t n, const double* d_x0,
                                                  const double* d_x_ref, const double* d_R_world, const double* d_foot_abs, int32_t foot_stride,
                                                  const uint8_t* d_contact, int32_t contact_stride, const double* d_yaw_A, double* d_grf_body_out,
                                                  double* d_u_full_out, int32_t* d_iters_out, int32_t* d_status_out, void* inputs_ready_stream,
                                                  int32_t* slot_out);
a1mpc_status a1mpc_pipeline_submit_strided(a1mpc_pipeline p, int32_t slot, int32_t fresh_batch, int32_t n, const double* x0, const double* x_ref,
                                           const double* R_world, const double* foot_abs, int32_t foot_stride, const uint8_t* contact,
                                           int32_t contact_stride, const double* yaw_A, double* grf_body_out, double* u_full_out,
                                           int32_t* iters_out, int32_t* status_out, int32_t* slot_out);
a1mpc_status a1mpc_pipeline_submit_ticks_device(a1mpc_pipeline p, int32_t slot, int32_t fresh_batch, int32_t n, const double* d_tick,
                                                const double* d_R_world, const double* d_foot_abs, const uint8_t* d_contact, double* d_grf_body_out,
                                                double* d_u_full_out, int32_t* d_iters_out, int32_t* d_status_out, void* inputs_ready_stream,
                                                int32_t* slot_out);
/* The tick records joined with the strides (arguments of a1mpc_solve_batch_ticks_strided_device: the outputs of the gait-aware horizon as per-step inputs) with batches
 * in flight together.  Per-step feet always solve on the general kernels, whose first solves are the ones a second batch in flight helps.  Slots, fresh_batch,
 * inputs_ready_stream and output life times as for a1mpc_pipeline_submit_strided_device; (foot_stride, contact_stride, yaw_A) = (0, 0, NULL) IS
 * a1mpc_pipeline_submit_ticks_device; a foot_stride other than 0 / 12 or a contact_stride other than 0 / 4 is refused.  Bit-identical to the lone handle's entry. */
a1mpc_status a1mpc_pipeline_submit_ticks_strided_device(a1mpc_pipeline p, int32_t slot, int32_t fresh_batch, int32_t n, const double* d_tick,
                                                        const double* d_R_world, const double* d_foot_abs, int32_t foot_stride, const uint8_t* d_contact,
                                                        int32_t contact_stride, const double* d_yaw_A, double* d_grf_body_out, double* d_u_full_out,
                                                        int32_t* d_iters_out, int32_t* d_status_out, void* inputs_ready_stream, int32_t* slot_out);
a1mpc_status a1mpc_pipeline_wait(a1mpc_pipeline p, int32_t slot);
a1mpc_status a1mpc_pipeline_join(a1mpc_pipeline p, int32_t slot, void* hip_stream);
/* a1mpc_pipeline_handle: a host-pointer batch still in flight on the slot is waited for and handed to its caller's output arrays first (its results live in
 * the handle's one pinned mirror, which any host-pointer call on the handle would overwrite).  a1mpc_pipeline_destroy does the same for every slot: the output
 * arrays of submitted batches must stay valid until wait / the next submit to the slot / destroy has returned. */
a1mpc_status a1mpc_pipeline_handle(a1mpc_pipeline p, int32_t slot, a1mpc_handle* out);
a1mpc_status a1mpc_pipeline_depth(a1mpc_pipeline p, int32_t* depth_out);
void a1mpc_pipeline_destroy(a1mpc_pipeline p);

const char* a1mpc_status_string(a1mpc_status s);
const char* a1mpc_last_error(void); /* thread-local detail of the last non-OK return (e.g. the HIP error string) */
const char* a1mpc_build_info(void); /* "sources <sha256/16 of csrc + this header> arch gfx950": which sources the library was compiled from */

#ifdef __cplusplus
}
#endif
#endif /* A1MPC_H_ */
