/*
 * cmpc_solver.h — C ABI of the MI355X-native batched convex-MPC solver (libcmpc_hip.so).
 *
 * Two surfaces live here:
 *
 *  1. The reference's single-instance SolverMPC interface, unchanged, so the be2r_cmpc_unitree
 *     FSM links against this library instead of SolverMPC.cpp + convexMPC_interface.cpp +
 *     RobotState.cpp (reference: be2r_cmpc_unitree/src/controllers/convexMPC/convexMPC_interface.h:44-52).
 *     Same names, same argument meaning, same call protocol
 *       setup_problem -> update_x_drag -> update_solver_settings -> update_problem_data_floats
 *       -> get_solution(0..11)
 *     (ConvexMPCLocomotion.cpp:807-836). The solve runs on the GPU through the batched path with
 *     batch = 1.
 *
 *  2. A new reentrant batched API (cmpc_batch_*): one handle per stream, a batch of independent
 *     MPC instances packed as fixed-stride fp32 records (layout below), forces + status out.
 *
 * No torch types cross this boundary: plain pointers and sizes only.
 */
#ifndef CMPC_SOLVER_H
#define CMPC_SOLVER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
#define CMPC_EXTERNC extern "C"
#else
#define CMPC_EXTERNC
#endif

/* ------------------------------------------------------------------------------------------ */
/* Instance record layout (fp32 words).                                                       */
/* One record = one solve_mpc() call's per-instance data (SolverMPC.cpp:566-655).             */
/* ------------------------------------------------------------------------------------------ */
#define CMPC_REC_P        0   /* p[3]      body position (world)          update_data_t.p      */
#define CMPC_REC_V        3   /* v[3]      body velocity (world)          update_data_t.v      */
#define CMPC_REC_Q        6   /* q[4]      orientation quaternion w,x,y,z update_data_t.q      */
#define CMPC_REC_W        10  /* w[3]      angular velocity (world)       update_data_t.w      */
#define CMPC_REC_R        13  /* r[12]     foot offsets, axis-major 3x4:  r[axis*4 + leg]      */
#define CMPC_REC_RPY      25  /* roll, pitch, yaw (stored, unused by the solve, as reference)  */
#define CMPC_REC_XDRAG    28  /* x_drag    A(11,9) coefficient            update_x_drag()      */
#define CMPC_REC_FEST3    29  /* f_est(3): compensation force fed into qg (config 5)           */
#define CMPC_REC_FLAGS    30  /* bit-cast uint32: bit0 = use f_est in qg (history > 500)       */
#define CMPC_REC_HDR      32  /* header words; traj follows                                    */
/* traj[12*N] fp32 at CMPC_REC_HDR, then gait[4*N] uint8 (step-major, leg-minor) packed into
 * N words, then padding to a 16-byte multiple. */
#define CMPC_REC_TRAJ(N)   (CMPC_REC_HDR)
#define CMPC_REC_GAIT(N)   (CMPC_REC_HDR + 12 * (N))
#define CMPC_REC_WORDS(N)  ((CMPC_REC_HDR + 13 * (N) + 3) & ~3)

/* Compact record (cmpc_batch_expand): what the caller computes trajAll from
 * (ConvexMPCLocomotion.cpp:554-585) instead of trajAll itself — the header as above, trajAll's
 * step-0 row (12 words: trajInitial with [2] = the measured yaw), the gait words, padding to a
 * 16-byte multiple. 56 words (224 B) at N = 10 against 164 (656 B): what a root GPU sends each
 * peer per instance in the config-4 sharding (parallel.RootPipeline record_format="compact"). */
#define CMPC_CREC_TRAJ0    (CMPC_REC_HDR)
#define CMPC_CREC_GAIT     (CMPC_REC_HDR + 12)
#define CMPC_CREC_WORDS(N) ((CMPC_REC_HDR + 12 + (N) + 3) & ~3)

#define CMPC_MAX_HORIZON  20  /* reference caps at 19 (SolverMPC.cpp:113-116); lifted to 20 for config 5;
                                 longer horizons are rejected (cmpc_batch_create / set_params -2) */

/* ------------------------------------------------------------------------------------------ */
/* Config 5: periodic-disturbance estimation (fp32 words).                                    */
/* LogData record: the previous step's logged state, forces and model, as the caller receives */
/* it from /log_data (unitree_legged_msgs/msg/LogData.msg; read at                            */
/* ConvexMPCLocomotion.cpp:639-771). geometry_msgs doubles are stored as fp32, the precision */
/* the reference casts them to.                                                               */
/* ------------------------------------------------------------------------------------------ */
#define CMPC_LOG_POS      0   /* pos_act x,y,z                                                  */
#define CMPC_LOG_EUL      3   /* euler_act x,y,z (roll, pitch, yaw)                             */
#define CMPC_LOG_ANG      6   /* vel_act.angular x,y,z                                          */
#define CMPC_LOG_LIN      9   /* vel_act.linear x,y,z                                           */
#define CMPC_LOG_FORCE    12  /* foot_force{0..3}_{x,y,z}, leg-major                            */
#define CMPC_LOG_XDRAG    24  /* x_drag                                                         */
#define CMPC_LOG_R        25  /* r_{x,y,z}_{1..4}, axis-major 3x4                               */
#define CMPC_LOG_ROT      37  /* R_00 .. R_22, row-major                                        */
#define CMPC_LOG_WORDS    48
/* Estimator state of one instance: the reference's globals time_history / diff_history /
 * est_* / f_est (SolverMPC.cpp:390-398, 555-563), with the unbounded histories replaced by a
 * ring of the last CMPC_EST_WINDOW samples (only that window is ever read). */
#define CMPC_EST_WINDOW   400 /* window_size (SolverMPC.cpp:704)                                */
#define CMPC_EST_STOP     500 /* re-estimation stops above this count (SolverMPC.cpp:707)       */
#define CMPC_EST_F        0   /* f_ext[3] samples, ring [400]                                   */
#define CMPC_EST_T        400 /* simulation_time samples, ring [400]                            */
#define CMPC_EST_COUNT    800 /* int32: samples pushed so far (= time_history.size(), capped)   */
#define CMPC_EST_HEAD     801 /* int32: ring slot of the next sample (= the oldest one)         */
#define CMPC_EST_FEST3    802 /* f_est(3), the compensation force                               */
#define CMPC_EST_PARAMS   804 /* double[4]: est_stat, est_amp, est_freq, est_phase              */
#define CMPC_EST_WORDS    816

/* ------------------------------------------------------------------------------------------ */
/* Batched input assembly: locomotion-controller state (fp32 words).  */
/* The inputs and persistent state of ConvexMPCLocomotion::run's MPC side                     */
/* (ConvexMPCLocomotion.cpp:100-123, 204-257, 334-339, 511-586, 612-633, 786-818).            */
/* Words marked "state" are read and written back by cmpc_batch_assemble; int32 words are     */
/* bit-cast into the fp32 array.                                                               */
/* ------------------------------------------------------------------------------------------ */
#define CMPC_LOCO_POS      0   /* seResult.position[3]                                         */
#define CMPC_LOCO_ZGT      3   /* ground_truth_position[2]: p[2] of the solve (:628)           */
#define CMPC_LOCO_Q        4   /* seResult.orientation (w,x,y,z)                               */
#define CMPC_LOCO_RPY      8   /* seResult.rpy[3]                                              */
#define CMPC_LOCO_VW       11  /* seResult.vWorld[3]                                           */
#define CMPC_LOCO_WW       14  /* seResult.omegaWorld[3]                                       */
#define CMPC_LOCO_PFOOT    17  /* pFoot[4][3], world frame, leg-major (:234)                   */
#define CMPC_LOCO_CMD      29  /* x_vel_cmd, y_vel_cmd, _yaw_turn_rate (scaled sticks, :108-114)*/
#define CMPC_LOCO_HEIGHT   32  /* _body_height                                                 */
#define CMPC_LOCO_VDES     33  /* state: filtered _x_vel_des, _y_vel_des (:116-117)            */
#define CMPC_LOCO_WPD      35  /* state: world_position_desired x, y (:239, :537-552)          */
#define CMPC_LOCO_RPYINT   37  /* state: rpy_int[0], rpy_int[1] (:218-228)                     */
#define CMPC_LOCO_XCI      39  /* state: x_comp_integral (:809-818)                            */
#define CMPC_LOCO_COUNTER  40  /* state, int32: iterationCounter                               */
#define CMPC_LOCO_GAIT     41  /* int32: OffsetDurationGait P, offsets[4], durations[4]        */
#define CMPC_LOCO_FLAGS    50  /* state, uint32: CMPC_LOCO_OMNI | STANDING | PRONK | FIRST     */
#define CMPC_LOCO_STAND    51  /* stand_traj x, y, yaw (:146-151; stand_traj[0], [1], [5])     */
/* foot placement and swing (:276-331, :350-402; FootSwingTrajectory.cpp:17-42)                  */
#define CMPC_LOCO_SWREM    56  /* state: swingTimeRemaining[4] (:287-296)                       */
#define CMPC_LOCO_SWST     60  /* out: gait->getSwingState() of the tick (Gait.cpp:102-135)      */
#define CMPC_LOCO_P0       64  /* state: footSwingTrajectories[l]._p0 [4][3] (:262, :378)       */
#define CMPC_LOCO_PF       76  /* state: footSwingTrajectories[l]._pf [4][3], the foothold Pf   */
#define CMPC_LOCO_PDES     88  /* state: footSwingTrajectories[l]._p [4][3] = pDesFootWorld     */
#define CMPC_LOCO_WORDS    104
#define CMPC_LOCO_OMNI     1u  /* omniMode: v_des is already in the world frame (:211)         */
#define CMPC_LOCO_STANDING 2u  /* current_gait == 4: stand trajectory (:527-533)               */
#define CMPC_LOCO_PRONK    4u  /* gaitNumber == 8 (pacing): roll compensation off (:230)      */
#define CMPC_LOCO_FIRST    8u  /* firstRun: world_position_desired = position (:249-256)       */
#define CMPC_LOCO_SIMFEET  16u /* simulator feet (not in the reference): after each tick a     */
                               /* swinging foot is at its pDesFootWorld, a foot entering stance */
                               /* touches down (z = 0) and stance feet stay fixed in the world; */
                               /* cmpc_batch_rollout then leaves the feet alone                 */
#define CMPC_LOCO_FSWING0  256u/* firstSwing[l] is bit (8 + l) (:75, :289, :376, :413)          */

/* Batch-shared controller constants. */
typedef struct cmpc_loco_params {
  float dt;               /* control tick (s); dtMPC = dt * iters_between_mpc                   */
  int   iters_between_mpc;/* _iterationsBetweenMPC                                             */
  float x_drag_gain;      /* _dyn_params->cmpc_x_drag                                          */
  int   pad;
  float hip_x, hip_y;     /* quadruped._abadLocation x, y: getHipLocation(l) = (+-x, +-y, 0)    */
                          /* (Quadruped.h:95-102; A1: 0.1805, 0.047, MiniCheetah.h:30-31)       */
  float abad_link;        /* quadruped._abadLinkLength (A1: 0.0838)                             */
  float swing_height;     /* _dyn_params->Swing_traj_height (ros_config.yaml:62: 0.17)          */
  float bonus_swing;      /* _dyn_params->cmpc_bonus_swing (ros_config.yaml:70: 0)              */
  float pad2[3];
} cmpc_loco_params;

/* Per-instance status (batched API). The reference has no status: on qpOASES failure it prints
 * "failed to solve!" and leaves stale forces (SolverMPC.cpp:964-968). Documented deviation:
 * every force of the instance is +0.0 when status != CMPC_OK, and an instance with CMPC_OK has
 * finite forces inside its friction pyramids. A failed instance changes nothing of any other
 * instance, in the same call or in a later one on the same handle (tests/test_gpu_status.py).
 *
 * Non-finite input: a record word that the solve reads (p, v, q, omega, r of a leg with a stance
 * step, x_drag, the trajectory, f_est(3) while the flag bit is set) and that is NaN, +-Inf or
 * >= 3e38 in magnitude. Where the word reaches only the gradient (p, v, omega, trajectory,
 * f_est) the status is CMPC_BAD_INPUT. Where it reaches the Hessian (q, r, x_drag) the NaN meets
 * a Cholesky pivot first and the status is CMPC_NOT_PD or CMPC_BAD_INPUT: the kernels do not tell
 * the two apart. Words the solve does not read (the stored roll / pitch / yaw, f_est(3) while the
 * flag is clear) are without effect. A trajectory row ahead of the record's first stance step
 * reaches no force: non-finite there, the instance is either solved as if the word were finite
 * (n <= 64, and 65..72 at N <= 10) or refused with CMPC_BAD_INPUT (the larger size classes).
 * The shared parameters (cmpc_params) are not validated:
 * with valid ones, 0 is always feasible and the cap is max_iter + 2n trips (n = reduced
 * variables), so CMPC_INFEASIBLE and CMPC_MAX_ITER need invalid parameters (f_max < 0) or a
 * lowered max_iter, and CMPC_NOT_PD needs alpha <= -diag(B'SB) or non-finite input. */
enum {
  CMPC_OK = 0,
  CMPC_MAX_ITER = 1,      /* more than max_iter + 2n active-set trips (reference nWSR = 100)   */
  CMPC_INFEASIBLE = 2,    /* friction-pyramid QP infeasible                                    */
  CMPC_NOT_PD = 3,        /* Hessian factorisation failed (a pivot <= 0 or NaN)                */
  CMPC_BAD_INPUT = 4      /* non-finite input that left the Hessian finite: the solution would */
                          /* not be a number (horizon out of range is refused by the host API) */
};

/* Batch-shared problem parameters (problem_setup + the update_data_t scalars that the caller
 * keeps constant across instances: ConvexMPCLocomotion.cpp:617,623,807). */
typedef struct cmpc_params {
  float dt;           /* dtMPC (s)                                                              */
  float mu;           /* friction coefficient; fmat uses 1/mu (SolverMPC.cpp:657-660)           */
  float f_max;        /* ub(fz) = gait * f_max                                                  */
  int   horizon;      /* N, 1..CMPC_MAX_HORIZON                                                 */
  float weights[12];  /* diagonal state weights (13th = 0)                                      */
  float alpha;        /* force regularisation: qH = 2(B'SB + alpha I)                          */
  int   max_iter;     /* active-set iteration cap (reference: nWSR = 100)                       */
} cmpc_params;

/* The robot: the single rigid body of the prediction model. The reference hard-codes the A1's
 * m = 12, I_body = diag(.07, .26, .242) (RobotState.h:25-26), which is the default here; another
 * robot, a payload or a randomised mass is set per handle (cmpc_batch_set_model) or for the
 * single-instance surface (cmpc_set_model). The fields are double: the fp32 kernels use (float)
 * of each field, the fp64 paths (the refinement of the wide classes, cmpc_batch_evaluate) the
 * doubles themselves, so the default model gives bit for bit what the literals gave.
 * Not part of the model: gravity (the reference's -9.8 in x0[12] and -9.81 in the config-5
 * residual both stay) and off-diagonal body inertia (principal moments only). The handle's model
 * is batch-shared, as cmpc_params is; a batch whose robots differ sets a per-instance table
 * (cmpc_batch_set_instance_params below). */
typedef struct cmpc_model {
  double mass;        /* kg, > 0 */
  double inertia[3];  /* principal body-frame moments Ixx, Iyy, Izz (kg m^2), each > 0;
                         I_world = R diag(.) R' */
} cmpc_model;

typedef struct cmpc_batch cmpc_batch;

/* ------------------------------------------------------------------------------------------ */
/* 1. Reference single-instance interface (convexMPC_interface.h:44-52)                       */
/* ------------------------------------------------------------------------------------------ */
/* Replaces convexMPC_interface.cpp:44-67 (+ resize_qp_mats, SolverMPC.cpp:149-250). */
CMPC_EXTERNC void setup_problem(double dt, int horizon, double mu, double f_max);
/* Replaces convexMPC_interface.cpp:96-107 (double-precision variant, yaw only). */
CMPC_EXTERNC void update_problem_data(double* p, double* v, double* q, double* w, double* r,
                                      double yaw, double* weights, double* state_trajectory,
                                      double alpha, int* gait);
/* Replaces convexMPC_interface.cpp:156-162: q_soln[index], 0 before the first solve. */
CMPC_EXTERNC double get_solution(int index);
/* Replaces convexMPC_interface.cpp:109-130 (use_jcqp thresholds >1.5 -> 2, >0.5 -> 1). */
CMPC_EXTERNC void update_solver_settings(int max_iter, double rho, double sigma,
                                         double solver_alpha, double terminate, double use_jcqp);
/* Replaces convexMPC_interface.cpp:132-149 -> solve_mpc (SolverMPC.cpp:566-1089). */
CMPC_EXTERNC void update_problem_data_floats(float* p, float* v, float* q, float* w, float* r,
                                             float roll, float pitch, float yaw, float* weights,
                                             float* state_trajectory, float alpha, int* gait);
#ifdef __cplusplus
/* C++ linkage, as the reference (convexMPC_interface.h:52; symbol _Z13update_x_dragf). */
void update_x_drag(float x_drag);
#endif

/* Globals the reference solver reads but its caller defines (ConvexMPCLocomotion.cpp:610,
 * be2r_cmpc_unitree_node.cpp:6). Weak definitions in the library; the host program's strong
 * definitions take precedence. f_ext has Eigen::Matrix<float,6,1> layout (6 floats). */
CMPC_EXTERNC float f_ext[6];
CMPC_EXTERNC float simulation_time;
/* The solver's own estimator globals (SolverMPC.h:72-74, SolverMPC.cpp:390-392, 772-798):
 * f_est(3) = the compensation force of the last update_problem_data* call (fed into qg once more
 * than 500 samples were pushed), f_est_smoothed = 0.95 f_est_smoothed + 0.05 f_est, and
 * f_est_static(3) = 0.97 f_est_static(3) + 0.03 f_ext(3). Eigen::Matrix<float,6,1> layout. The
 * estimator step itself runs on the device (the kernel of cmpc_batch_estimate, one instance). */
CMPC_EXTERNC float f_est[6];
CMPC_EXTERNC float f_est_smoothed[6];
CMPC_EXTERNC float f_est_static[6];

/* ------------------------------------------------------------------------------------------ */
/* 2. Batched, reentrant API                                                                   */
/* ------------------------------------------------------------------------------------------ */
CMPC_EXTERNC int cmpc_record_words(int horizon);
/* Create a handle bound to the current HIP device; stream may be NULL (a private stream is
 * created). Scratch for max_batch instances is allocated here, never inside solve. */
CMPC_EXTERNC int cmpc_batch_create(cmpc_batch** out, const cmpc_params* prm, int max_batch,
                                   void* hip_stream);
CMPC_EXTERNC int cmpc_batch_set_params(cmpc_batch* h, const cmpc_params* prm);
CMPC_EXTERNC void cmpc_batch_destroy(cmpc_batch* h);
/* The handle's robot model (cmpc_model above); m == NULL sets the default. Handle state of its
 * own: it survives cmpc_batch_set_params, in either order of the two calls, and applies to every
 * call made after it (solve, solve_due, condense, evaluate, rollout, and the residual of
 * cmpc_batch_estimate when d_logs is given; cmpc_batch_admm follows through the H and g it is
 * given). No allocation and no synchronisation. A non-finite or non-positive field returns -2
 * (the bad-value error of cmpc_batch_set_params) and leaves the handle unchanged. New API. */
CMPC_EXTERNC int cmpc_batch_set_model(cmpc_batch* h, const cmpc_model* m);
CMPC_EXTERNC int cmpc_batch_get_model(const cmpc_batch* h, cmpc_model* out);
/* Per-instance robot mass, inertia, friction coefficient and force limit: one row of
 * CMPC_INST_WORDS doubles per instance (payload and inertia randomisation per environment, a
 * friction coefficient per terrain patch, a weakened actuator on some robots). New API. */
#define CMPC_INST_MASS     0   /* kg, > 0                                    */
#define CMPC_INST_INERTIA  1   /* Ixx, Iyy, Izz (kg m^2), each > 0           */
#define CMPC_INST_MU       4   /* friction coefficient, > 0                  */
#define CMPC_INST_FMAX     5   /* force limit (N)                            */
#define CMPC_INST_WORDS    6
/* d_inst: device pointer to count * CMPC_INST_WORDS doubles, 1 <= count <= max_batch. Row i belongs
 * to instance i of every later call: the index of its record, with or without a due mask. The call
 * snapshots the rows (later writes to d_inst have no effect until the next call) into a
 * handle-owned table of kernel-side values, the first 64-byte line of an entry per instance
 * (the second line is cmpc_batch_set_instance_costs'), derived by the
 * expressions the handle's own model and parameters go through ((float) inertia, 1.f / (float)
 * mass, 1.0 / inertia, 1.0 / mass, 1.f / (float) mu, (float) f_max), so a row equal to a handle's
 * model, mu and f_max gives that handle's bits; beside it the rows themselves (48 bytes per
 * instance: cmpc_batch_evaluate uses the inertia doubles). Both are allocated for max_batch
 * instances by the first call (make it outside stream capture) and freed by cmpc_batch_destroy; no
 * solve allocates. A set-up call: it synchronises the handle's stream (a validation kernel counts
 * the bad rows, the host reads the count, a conversion kernel fills the table).
 * A row is bad when its mass or inertia breaks the rules of cmpc_batch_set_model (overflowing
 * reciprocals included), when mu is not positive or 1.f / (float) mu is not finite, when (float)
 * f_max is not finite, or when any word is non-finite. With any bad row the call returns -2 and the
 * handle keeps its previous table, or none. d_inst == NULL clears the table: the handle is then bit
 * for bit the handle it was before (shared model, mu and f_max).
 * While a table is set, instance i uses row i in place of the handle's model, mu and f_max in
 * cmpc_batch_solve, _solve_due, _solve_host, _condense, _condense_rows, _evaluate(_host),
 * _sensitivity(_host), _rollout, _estimate(_due) (the residual, when d_logs is given) and _admm
 * (fmat and U_b); a row whose |gait x f_max| < 0.01 eliminates every foot-step of that instance
 * alone. Each of these calls with
 * batch > count returns its bad-arguments error and writes nothing. cmpc_batch_get_model still
 * returns the handle's shared model; cmpc_batch_set_model and _set_params still work and the table
 * survives both: their model, mu and f_max become visible again when the table is cleared. The
 * weights and alpha have a table of their own (cmpc_batch_set_instance_costs below); dt, horizon,
 * max_iter, refine and output steps stay batch-shared. The single-instance
 * surface and libcmpc_multi.so take no table. */
CMPC_EXTERNC int cmpc_batch_set_instance_params(cmpc_batch* h, const double* d_inst, int count);
CMPC_EXTERNC int cmpc_batch_instance_count(const cmpc_batch* h);   /* 0: none set */
/* Per-instance cost: one row of CMPC_COST_WORDS floats per instance, the twelve state weights and the
 * force regularisation alpha (many candidate costs tuned in one batch, gait-dependent weights in a
 * mixed batch). The reference takes both on every update_problem_data call and so does the
 * single-instance surface here; this call gives the batched surface the same freedom. New API. */
#define CMPC_COST_WEIGHTS 0    /* 12 fp32 state weights, each finite and >= 0 (cmpc_params.weights) */
#define CMPC_COST_ALPHA   12   /* fp32, finite, > 0, 2.f * alpha finite                              */
#define CMPC_COST_WORDS   16   /* words 13..15 reserved: never read, any bit pattern                 */
/* d_cost: device pointer to count * CMPC_COST_WORDS floats, 1 <= count <= max_batch. Row i belongs
 * to instance i of every later call: the index of its record, with or without a due mask. The call
 * snapshots the rows (later writes to d_cost have no effect until the next call) into the second
 * 64-byte line of the handle-owned table of kernel-side entries (128 bytes per instance: the first
 * line is cmpc_batch_set_instance_params'), 2.f * alpha formed by the expression the handle's own
 * alpha goes through, so a row equal to a handle's weights and alpha gives that handle's bits. The
 * table's buffers are allocated for max_batch instances by the first call of either table (make it
 * outside stream capture) and freed by cmpc_batch_destroy; no solve allocates. A set-up call: it
 * synchronises the handle's stream (a validation kernel counts the bad rows, the host reads the
 * count, a conversion kernel fills the table).
 * A row is bad when a weight is negative or non-finite, when alpha is non-finite or <= 0, or when
 * 2.f * alpha is not finite. (cmpc_params itself validates none of these; the table is stricter
 * because a bad alpha in one row would otherwise show only as that instance's CMPC_NOT_PD.) With
 * any bad row the call returns -2 and the handle keeps its previous table, or none. d_cost == NULL
 * clears the table: the handle is then bit for bit the handle it was before (shared weights, alpha).
 * While a table is set, instance i uses row i in place of the handle's weights and alpha in
 * cmpc_batch_solve, _solve_due, _solve_host, _condense, _condense_rows, _evaluate(_host) and
 * _sensitivity(_host); _admm follows through the H and g it is given; _rollout, _estimate(_due),
 * _assemble and _expand read neither value. Each call that takes a batch returns its
 * bad-arguments error and writes nothing when batch > count.
 * The cost table and the parameter table are independent: either, both or neither may be set, in
 * any order, and each is cleared on its own; with both set, batch must not exceed either count.
 * Both survive cmpc_batch_set_params and cmpc_batch_set_model; of the shared values a table does
 * not cover, the newest apply to every instance (with only a cost table, a later set_model or a new
 * mu reaches every row; with only a parameter table, new shared weights do), refreshed by a kernel
 * on the handle's stream without allocation or host synchronisation.
 * Out of scope: per-instance dt, horizon and max_iter; the single-instance surface, which already
 * takes weights and alpha per call; libcmpc_multi.so and parallel.RootPipeline. */
CMPC_EXTERNC int cmpc_batch_set_instance_costs(cmpc_batch* h, const float* d_cost, int count);
CMPC_EXTERNC int cmpc_batch_instance_cost_count(const cmpc_batch* h);   /* 0: none set */
/* Device-resident solve: d_records [batch * cmpc_record_words(N)] fp32, d_forces
 * [batch * 12N] fp32 (step-major, leg*3+axis), d_status [batch] uint8, d_iters [batch] int32
 * (may be NULL). Asynchronous on the handle's stream. Returns 0 or a negative error. */
CMPC_EXTERNC int cmpc_batch_solve(cmpc_batch* h, const float* d_records, int batch,
                                  float* d_forces, uint8_t* d_status, int32_t* d_iters);
/* The same solve for the instances with an MPC step due this tick, for batches whose
 * iterationCounters are not in lockstep. d_due: `batch` bytes, the array cmpc_batch_assemble
 * writes; instance i is due iff d_due[i] != 0 (the test of cmpc_batch_rollout); bytes at index
 * `batch` and beyond are never read. d_due == NULL is exactly cmpc_batch_solve (the same launch
 * sequence, not a mask of ones).
 *   due:     forces, status and iters are bit for bit what cmpc_batch_solve writes for the same
 *            record, in every size class, launch form and batch size, with the same
 *            cmpc_batch_set_output_steps stride and cmpc_batch_set_refine setting;
 *   not due: the record is never read (it may hold anything, NaN words and arbitrary gait bytes
 *            included), and the instance's rows of d_forces, d_status and d_iters are not
 *            written: they keep the caller's previous values, so a robot holds its last forces
 *            until its next MPC step.
 * Asynchronous on the handle's stream, joined as cmpc_batch_solve is: when the handle's stream
 * reaches the end of the call every size class has finished. No allocation and no host
 * synchronisation inside. Argument checks and error returns of cmpc_batch_solve. The timing hooks
 * below record around it as well; class1_overflow then counts due instances only. New API. */
CMPC_EXTERNC int cmpc_batch_solve_due(cmpc_batch* h, const float* d_records, const uint8_t* d_due,
                                      int batch, float* d_forces, uint8_t* d_status, int32_t* d_iters);
/* Forces kept per instance: the first `steps` horizon steps (12 x steps floats per instance,
 * stride of d_forces / forces of the two solves below and of cmpc_batch_rollout), 0 = every step
 * (12N, the default). A caller that reads only get_solution(0..11) as ConvexMPCLocomotion.cpp:
 * 832-845 does can keep step 0 (48 B instead of 480 B per instance at N = 10). New API. */
CMPC_EXTERNC int cmpc_batch_set_output_steps(cmpc_batch* h, int steps);
/* The fp64 refinement of the converged working set in the wide size classes:
 * 1 (default) from N = 11, 0 off (every horizon solved in fp32 only, as the reference's own fp32
 * condensation: ~11 % faster at N = 16, but at N >= 16 a few all-stance instances then miss
 * qpOASES by more than 1e-4). New API. */
CMPC_EXTERNC int cmpc_batch_set_refine(cmpc_batch* h, int on);
/* Compact records (CMPC_CREC_*) -> solve records for the handle's horizon: trajAll[12 k + j] =
 * the step-0 row, except j = 2, 3, 4 (yaw, x, y) = the previous step's + dtMPC x (yaw rate, v_x,
 * v_y) of the step-0 row, in fp32 as updateMPCIfNeeded computes it (ConvexMPCLocomotion.cpp:
 * 554-585, dtMPC = the handle's dt). Bit for bit the records a caller builds itself. d_compact
 * [batch * CMPC_CREC_WORDS(N)], d_records [batch * cmpc_record_words(N)]. Asynchronous on the
 * handle's stream. New API. */
CMPC_EXTERNC int cmpc_batch_expand(cmpc_batch* h, const float* d_compact, float* d_records, int batch);
/* Same, host buffers in and out (H2D + solve + D2H on the handle's stream, synchronous). */
CMPC_EXTERNC int cmpc_batch_solve_host(cmpc_batch* h, const float* records, int batch,
                                       float* forces, uint8_t* status, int32_t* iters);
/* Prediction, cost and optimality gap of given forces U [batch * 12N] (this solver's, qpOASES's,
 * ADMM's or the caller's own), in fp64, against the exact QP the fp32 record defines: the model
 * matrices in fp64 from the record's fp32 words, Adt / Bdt / Qdt = the exact exponential (A_c^3 =
 * 0), no H or g formed. New API.
 *   x_k+1 = Adt x_k + Bdt u_k + Qdt f,  x_0 = [rpy, p, w, v, -9.8] (rpy = quat_to_rpy of q rounded
 *           to fp32, SolverMPC.cpp:352-361, 592), f = (0,0,0,f_est3,0,0) if flag bit 0, else 0
 *   cost  = sum_k (x_k - xd_k)' W (x_k - xd_k) + alpha |U|^2,  W = diag(weights, 0), k = 1..N
 *   cost0 = the same at U = 0;  cost - cost0 = 1/2 U'HU + g'U, the reference's QP objective
 *   grad  = HU + g by the adjoint: lambda <- Adt' lambda + 2 W e_k, grad_k = Bdt' lambda + 2 alpha u_k
 *   gap   = sum over stance foot-steps of  grad_fs . f_fs - min(0, ub (grad_z - mu |grad_x| - mu |grad_y|))
 * with ub = gait x f_max and 1/mu as fmat holds it in fp32 (SolverMPC.cpp:657-665); a foot-step is
 * stance unless |ub| < 0.01 (SolverMPC.cpp:869-894). The feasible set is a product of truncated
 * pyramids {|fx| <= mu fz, |fy| <= mu fz, 0 <= fz <= ub} with vertices 0 and (+-mu ub, +-mu ub, ub),
 * so gap is the Frank-Wolfe gap in closed form: for feasible U, cost(U) - cost(U*) <= gap, and
 * gap = 0 at the optimum; no active-set tolerance, no multipliers. (Strong convexity also gives
 * |U - U*|_2 <= sqrt(gap / alpha), which at alpha ~ 4e-5 is newtons wide: not a useful distance.)
 * Outputs, either may be NULL (not both):
 *   d_xpred [batch * 12N] fp32: x_1 .. x_N rounded from fp64, step-major, components in the order
 *           of the record's traj rows (rpy, p, w, v);
 *   d_cert  [batch * CMPC_CERT_WORDS] fp64, indexed by CMPC_CERT_*.
 * Non-finite input gives NaN words. Asynchronous on the handle's stream. Returns 0 or a negative
 * error: bad batch, both outputs NULL, or a handle that keeps fewer than N output steps
 * (cmpc_batch_set_output_steps: its forces are not a full solution). */
#define CMPC_CERT_COST    0   /* cost(U)                                                         */
#define CMPC_CERT_COST0   1   /* cost(0)                                                         */
#define CMPC_CERT_GAP     2   /* Frank-Wolfe gap (>= cost(U) - cost(U*) for feasible U)         */
#define CMPC_CERT_VIOL    3   /* max over stance foot-steps of the negative slack of the rows   */
                              /* (+-fx/mu + fz)/sqrt(1/mu^2 + 1), (+-fy/mu + fz)/sqrt(1/mu^2 + 1), */
                              /* fz, ub - fz; clamped at 0                                        */
#define CMPC_CERT_SWING   4   /* max |f| over swing foot-steps                                   */
#define CMPC_CERT_GRADMAX 5   /* max |grad| over stance columns                                  */
#define CMPC_CERT_WORDS   8   /* words 6, 7: padding, written as 0                               */
CMPC_EXTERNC int cmpc_batch_evaluate(cmpc_batch* h, const float* d_records, const float* d_forces,
                                     int batch, float* d_xpred, double* d_cert);
/* Same, host buffers in and out (H2D + kernel + D2H on the handle's stream, synchronous). */
CMPC_EXTERNC int cmpc_batch_evaluate_host(cmpc_batch* h, const float* records, const float* forces,
                                          int batch, float* xpred, double* cert);
/* Single-instance surface: cmpc_batch_evaluate of the record and the solution of the last
 * update_problem_data* call (x_pred [12N] fp32, cert [CMPC_CERT_WORDS] fp64; either may be NULL).
 * Runs on request only, so the reference protocol's latency is untouched. Returns a negative
 * error before the first solve. New API. */
CMPC_EXTERNC int cmpc_evaluate_last(float* x_pred, double* cert);
/* Gradients of a loss L through the solve, by an fp64 Riccati adjoint: given forces U [batch * 12N]
 * (any source, as for cmpc_batch_evaluate) and the upstream gradient V = dL/dU [batch * 12N], how L
 * moves with the weights, alpha, the initial state, the reference trajectory and f_est(3). The QP,
 * x_0, 1/mu, ub and the stance test are cmpc_batch_evaluate's, all in fp64. New API.
 *   face:   a row of a stance foot-step is active when its normalised slack (the six expressions of
 *           CMPC_CERT_VIOL, not negated) is <= act_tol newtons. The foot-step's free subspace Z_s is
 *           the null space of its active rows' normals: interior (dimension 3), one friction side
 *           (2), an x side and a y side (1), the cap fz = ub (2), cap and one side (1), cap and two
 *           sides (0). A foot-step with fz at 0, or on both sides of one axis, is at the apex: all of
 *           it is pinned (0). Swing foot-steps are pinned. Z = diag(Z_s), m = sum of the dimensions.
 *   w     = -Z (Z'HZ)^-1 Z'V,  H = 2 (B_qp' S B_qp + alpha I): dL/dg of the minimiser over the face
 *   dx    : the rollout of w from a zero state, dx_k+1 = Adt dx_k + Bdt w_k; x_k(U) as evaluate's
 *   dL/dxd_k[j] = -2 W_j dx_k[j]                       (word j of traj row k)
 *   dL/dx_0     = the first 12 components of lambda_0,  lambda <- Adt' lambda + 2 W dx_k backwards
 *   dL/dW_j     = 2 sum_k dx_k[j] (x_k(U) - xd_k)[j]    (through H and g together)
 *   dL/dalpha   = 2 w.U
 *   dL/df_est(3) = sum_k lambda_k+1' Qdt e_3 when flag bit 0 is set, otherwise 0
 * w solves an LQ problem over the 12 dynamic states with at most 12 inputs per step, by a Riccati
 * recursion: O(N 12^3) operations at any horizon, no H formed.
 * Out of scope: the rpy part of dL/dx_0 is the partial derivative at a fixed rotation matrix (the
 * quaternion also forms R); nothing is returned for the derivative through R, the foot offsets r,
 * x_drag, mass, inertia, mu, f_max or dt.
 * Validity: the quantity is defined for any U: it is the derivative of the minimiser over the face
 * U lies on. It equals the derivative of the solve when U is the optimum and no active row has a
 * zero multiplier. At a weakly active row the solution map is only directionally differentiable;
 * what is returned there is the derivative of one side, and this is not detected (CMPC_SENS_SLACK
 * tells how near an inactive row is, nothing tells how near a multiplier is to 0). An instance whose
 * forces are all zero (a failed status) has m = 0 and zero gradients. Non-finite forces, V or
 * trajectory words give NaN in every word of d_sens but CMPC_SENS_FREE (d_dtraj and d_dg hold NaN
 * only where the arithmetic carries it: they do not depend on the trajectory, for one); other
 * non-finite record words give NaN in the words they reach.
 * Outputs: d_sens [batch * CMPC_SENS_WORDS] fp64; d_dtraj [batch * 12N] fp64 = dL/dxd, step-major in
 * the order of the traj rows, may be NULL; d_dg [batch * 12N] fp64 = w, may be NULL.
 * Honours the handle's model and both per-instance tables as cmpc_batch_evaluate does. Asynchronous
 * on the handle's stream; neither allocates nor synchronises. Returns 0 or a negative error: those
 * of cmpc_batch_evaluate (bad batch, a NULL input, a NULL d_sens, a handle that keeps fewer than N
 * output steps), and -2 for an act_tol that is negative or not finite. */
#define CMPC_SENS_X0       0   /* 12: dL/dx_0 in the order of the traj rows (rpy, p, w, v)      */
#define CMPC_SENS_WEIGHTS  12  /* 12: dL/dweights                                               */
#define CMPC_SENS_ALPHA    24
#define CMPC_SENS_FEST3    25
#define CMPC_SENS_FREE     26  /* m, the face's dimension, as a double                          */
#define CMPC_SENS_SLACK    27  /* smallest normalised slack of an inactive row of a stance      */
                               /* foot-step (+inf when there is none): how near the face is to   */
                               /* changing                                                       */
#define CMPC_SENS_WORDS    32  /* 28..31 written as 0 */
CMPC_EXTERNC int cmpc_batch_sensitivity(cmpc_batch* h, const float* d_records, const float* d_forces,
                                        const float* d_grad_forces, int batch, double act_tol,
                                        double* d_sens, double* d_dtraj, double* d_dg);
/* Same, host buffers in and out (H2D + kernel + D2H on the handle's stream, synchronous). */
CMPC_EXTERNC int cmpc_batch_sensitivity_host(cmpc_batch* h, const float* records, const float* forces,
                                             const float* grad_forces, int batch, double act_tol,
                                             double* sens, double* dtraj, double* dg);
/* Single-instance surface: cmpc_batch_sensitivity of the record, the solution and the model of the
 * last update_problem_data* call (grad_forces [12N]; sens [CMPC_SENS_WORDS]; dtraj, dg [12N] or
 * NULL). Runs on request only. Returns a negative error before the first solve. New API. */
CMPC_EXTERNC int cmpc_sensitivity_last(const float* grad_forces, double act_tol, double* sens,
                                       double* dtraj, double* dg);
/* The step-0 feedback gain of the solve: given forces U [batch * 12N] (any source, as for
 * cmpc_batch_evaluate), G = d u_0* / d x_0 [12 x 12], with which a controller that holds the solved
 * forces for iters_between_mpc ticks corrects them for the state's drift, u = u_0 + G (x - x_0)
 * (cmpc_batch_feedback below). The QP, x_0, 1/mu, ub and the stance test are cmpc_batch_evaluate's;
 * the face, Z_k, the apex rule and the pinned swing foot-steps are cmpc_batch_sensitivity's, word for
 * word, with act_tol in newtons. New API.
 * Backwards from P = 0 over the 12 dynamic states, with Pn = P_k+1 + W and G_k = Bdt Z_k:
 *   R   = alpha Z_k'Z_k + G_k'Pn G_k
 *   P_k = Adt'Pn Adt - (Adt'Pn G_k) R^-1 (G_k'Pn Adt)
 *   at k = 0:  K_0 = R^-1 G_0'Pn Adt,  G = -Z_0 K_0
 * (the backward half of cmpc_batch_sensitivity's recursion, without its upstream gradient, forward
 * pass or trajectory; one vector-Jacobian product of that call gives one row's worth of G). G is
 * row-major: row = force component leg*3+axis of step 0, column = component of x_0 in the order of
 * the traj rows (rpy, p, w, v). G is the derivative of the step-0 forces of the minimiser over U's
 * face with respect to x_0.
 *   Validity: as for cmpc_batch_sensitivity: G equals the derivative of the solve where U is the
 *     optimum and no active row has a zero multiplier; at a weakly active row it is one side's
 *     derivative, undetected (CMPC_GAIN_SLACK tells how near an inactive row is).
 *   rpy columns: the partial derivative at a fixed rotation matrix and fixed foot offsets r.
 *   Rows of swing or pinned foot-steps are exactly +0.0. For an active row with normal n of a step-0
 *     foot-step, n'G_foot = 0 to rounding.
 *   G does not depend on the trajectory, p, v, w, f_est(3) or the flag word: those words are not
 *     read, so NaN there changes no bit.
 *   Non-finite forces give NaN in words 0..143 and CMPC_GAIN_SLACK, with FREE and FREE0 as
 *     classified. An instance whose forces are all zero (a failed status) has G = 0 and FREE = 0.
 * Output: d_gain [batch * CMPC_GAIN_WORDS] fp64. Honours the handle's model and both per-instance
 * tables as cmpc_batch_evaluate does. Asynchronous on the handle's stream; neither allocates nor
 * synchronises. Returns 0 or a negative error, those of cmpc_batch_sensitivity: bad batch (beyond
 * max_batch or a table's count), a NULL argument, a handle that keeps fewer than N output steps
 * (-3), and -2 for an act_tol that is negative or not finite.
 * Out of scope: d u_k / d x_0 for k >= 1; gains with respect to the trajectory or f_est; the
 * derivative through R, r, x_drag, mass, inertia, mu, f_max or dt. */
#define CMPC_GAIN_K        0    /* 144: G, row-major [force component of step 0][component of x_0] */
#define CMPC_GAIN_FREE     144  /* m, the face's dimension over all steps, as CMPC_SENS_FREE        */
#define CMPC_GAIN_FREE0    145  /* the dimension of step 0's face, 0..12                             */
#define CMPC_GAIN_SLACK    146  /* as CMPC_SENS_SLACK                                                */
#define CMPC_GAIN_WORDS    148  /* 147 written as 0 */
CMPC_EXTERNC int cmpc_batch_gain(cmpc_batch* h, const float* d_records, const float* d_forces, int batch,
                                 double act_tol, double* d_gain);
/* Same, host buffers in and out (H2D + kernel + D2H on the handle's stream, synchronous). */
CMPC_EXTERNC int cmpc_batch_gain_host(cmpc_batch* h, const float* records, const float* forces, int batch,
                                      double act_tol, double* gain);
/* Single-instance surface: cmpc_batch_gain of the record, the solution and the model of the last
 * update_problem_data* call (gain [CMPC_GAIN_WORDS]). Runs on request only. Returns a negative error
 * before the first solve. New API. */
CMPC_EXTERNC int cmpc_gain_last(double act_tol, double* gain);
/* The held forces corrected for the present state. d_forces: the solved forces at the handle's
 * output stride (cmpc_batch_set_output_steps; step 0 alone is read); d_gain: cmpc_batch_gain's
 * output for them, 16-byte aligned (the rows of G are read by 16-byte loads; the 1184-byte stride of an
 * instance keeps every row so); d_states [batch * 12] fp32: the present state in the order of the traj rows (what
 * CMPC_LOCO_RPY / POS / WW / VW hold); d_due [batch] bytes or NULL; d_u [batch * 12] fp32. For
 * instance i with d_due == NULL or d_due[i] == 0, all in fp64:
 *   delta = x - x_0 (x_0 as the solve forms it from the record), the three rpy differences wrapped
 *           by delta - 2 pi rint(delta / 2 pi);
 *   u     = u_0 + G delta, summed over the columns 0..11 in order;
 *   guard, per foot of step 0: stance (|ub| >= 0.01): fz <- min(max(fz, 0), ub), then fx, fy clamped
 *           to +-mu fz with mu = 1 / (the fp32 1/mu); swing: +0.0;
 *   and one rounding to fp32.
 * An instance with d_due[i] != 0 has just been solved: its row of d_u is not written and nothing
 * of it but the due byte is read, so cmpc_batch_assemble's due mask can be passed as it is. Honours
 * the per-instance parameter table (mu, f_max) as cmpc_batch_evaluate does. Asynchronous on the
 * handle's stream; neither allocates nor synchronises. Returns 0 or a negative error: bad batch, a
 * NULL argument other than d_due, a d_gain that is not 16-byte aligned. New API. */
CMPC_EXTERNC int cmpc_batch_feedback(cmpc_batch* h, const float* d_records, const float* d_forces,
                                     const double* d_gain, const float* d_states, const uint8_t* d_due,
                                     int batch, float* d_u);
/* Single-instance surface: the robot model from the next update_problem_data* call on, as
 * update_solver_settings sets its settings (m == NULL: the default; -2 and no change for a
 * non-finite or non-positive field). cmpc_evaluate_last evaluates under the model of the solve it
 * evaluates. New API. */
CMPC_EXTERNC int cmpc_set_model(const cmpc_model* m);
/* Parity hook for the condensation rows (SolverMPC.cpp:96-146, 806-814): full 12N x 12N qH
 * (row-major) and qg per instance, all variables kept (no swing elimination). */
CMPC_EXTERNC int cmpc_batch_condense(cmpc_batch* h, const float* d_records, int batch,
                                     float* d_H, float* d_g);
/* The same in row-owner mode: every row of qH carries its own recursion on down to step 0 and
 * writes its entries on both sides of the diagonal, none mirrored from the row above, so qH is
 * symmetric to fp32 rounding only. This is how the class-1 solver condenses tables with two
 * stance feet at every step; qg as above. New API. */
CMPC_EXTERNC int cmpc_batch_condense_rows(cmpc_batch* h, const float* d_records, int batch,
                                          float* d_H, float* d_g);
/* JCQP ADMM settings: update_solver_settings(max_iter, rho, sigma, solver_alpha, terminate, .)
 * (convexMPC_interface.cpp:109-129 -> QpProblemSettings, JCQP/QpProblem.h:15-28). */
typedef struct cmpc_admm_settings {
  int    max_iter;    /* maxIterations (ros_config.yaml jcqp_max_iter: 10000)                   */
  double rho;         /* jcqp_rho 1e-7                                                           */
  double sigma;       /* jcqp_sigma 1e-8                                                         */
  double alpha;       /* over-relaxation, jcqp_alpha 1.5                                         */
  double terminate;   /* (|Ax - z|_inf + |Px + q + A'y|_inf) / 4 threshold, jcqp_terminate 0.1  */
  int    reduced;     /* 0: use_jcqp == 1 (full QP); 1: use_jcqp == 2 (swing legs eliminated)    */
} cmpc_admm_settings;
/* use_jcqp == 1 (SolverMPC.cpp:818-838, 1057-1062): the full QP (P = qH, q = qg from
 * cmpc_batch_condense, A = fmat, l = 0, u = U_b) solved by JCQP's ADMM in fp64, one workgroup
 * per instance, any horizon. With s->reduced (use_jcqp == 2, SolverMPC.cpp:984-1053) the swing
 * legs are eliminated first. QPs of up to 120 variables keep the inverted KKT Schur complement in
 * LDS; larger ones (N > 10) in per-workgroup fp64 global slabs (min(max_batch, 512) x (12N)^2
 * doubles: 151 MB at N = 16, 236 MB at N = 20), allocated by the handle's FIRST cmpc_batch_admm
 * call and kept from then on (handles that never run ADMM never pay for them): make that first
 * call outside stream capture, and expect an allocation failure to surface there. d_forces
 * [batch * out_cols] = the solution as float (0 for eliminated variables), the leading steps the
 * handle keeps (cmpc_batch_set_output_steps; 12N by default), so cmpc_batch_rollout reads ADMM
 * forces with the same stride as the active-set solve's; d_status 0 = residual
 * below terminate, 1 = max_iter reached; d_iters (may be NULL). */
CMPC_EXTERNC int cmpc_batch_admm(cmpc_batch* h, const float* d_records, const float* d_H,
                                 const float* d_g, int batch, const cmpc_admm_settings* s,
                                 float* d_forces, uint8_t* d_status, int32_t* d_iters);
/* Config 5, one estimator step for every instance (SolverMPC.cpp:688-811 per instance, the
 * residual of ConvexMPCLocomotion.cpp:639-771 first when d_logs is given):
 *   f_ext  = residual(d_logs[i], d_records[i])          if d_logs  (written to d_fext6 if set)
 *            (0, 0, 0, d_fext3[i], 0, 0)                 otherwise
 *   push (f_ext[3], t_i) into d_est[i], t_i = d_time ? d_time[i] : sim_time;
 *   400 <= count <= 500: band-pass (Gaussian sigma 7 minus sigma 27), DFT peak, sine fit;
 *   count >= 400: f_est(3) = est_amp + sin(2 pi t_i est_freq + est_phase);
 *   d_records[i]: CMPC_REC_FEST3 = f_est(3), CMPC_REC_FLAGS bit 0 = (count > 500).
 * d_est: batch * CMPC_EST_WORDS words, zero-initialised by the caller before the first step.
 * Asynchronous on the handle's stream; run it before cmpc_batch_solve on the same records. */
CMPC_EXTERNC int cmpc_batch_estimate(cmpc_batch* h, float* d_est, const float* d_logs,
                                     const float* d_fext3, const float* d_time, float sim_time,
                                     float* d_records, float* d_fext6, int batch);
/* The same step for the due instances only (d_due as for cmpc_batch_solve_due; NULL is exactly
 * cmpc_batch_estimate): the reference runs its estimator inside solve_mpc, i.e. on MPC ticks. A
 * due instance gets bit for bit the step of cmpc_batch_estimate; of an instance that is not due
 * neither the d_est state, nor the record's CMPC_REC_FEST3 / CMPC_REC_FLAGS words, nor the
 * d_fext6 row is touched. Argument checks and error returns of cmpc_batch_estimate. New API. */
CMPC_EXTERNC int cmpc_batch_estimate_due(cmpc_batch* h, float* d_est, const float* d_logs,
                                         const float* d_fext3, const float* d_time, float sim_time,
                                         float* d_records, float* d_fext6, const uint8_t* d_due,
                                         int batch);
/* One control tick of every instance's locomotion controller (batched
 * ConvexMPCLocomotion::run MPC side): updates the state words of d_loco [batch *
 * CMPC_LOCO_WORDS]; where an MPC step is due (iterationCounter % iters_between_mpc == 0 after
 * the increment) writes the instance's solve record d_records[i] (the arguments the reference
 * passes to update_problem_data_floats: p, v, q, w, r, rpy, trajAll, gait table, x_drag) and
 * d_due[i] = 1, else leaves the record and sets d_due[i] = 0. Gait rows i < N use
 * (i + _iteration + 1) mod P, i.e. the table repeats for N > P where the reference would read
 * past its P-row table. Asynchronous on the handle's stream. */
CMPC_EXTERNC int cmpc_batch_assemble(cmpc_batch* h, float* d_loco, const cmpc_loco_params* lp,
                                     float* d_records, uint8_t* d_due, int batch);
/* Closes the loop of a batched MPC simulator: for every instance with d_due[i] != 0 (all when
 * d_due is NULL), advances the single-rigid-body state of its record by one MPC step with its
 * own prediction model and the step-0 forces of the solve (d_forces[i][0..11]), plus an
 * optional disturbance d_xi6[i] = [tau(3), f(3)] through Qdt (Q_ct of SolverMPC.cpp:607-615):
 *   x+ = Adt x0 + Bdt u0 + Qdt xi   (the discretisation of c2qp, SolverMPC.cpp:96-146)
 * and writes rpy / p / w / v (+ the quaternion, z_groundtruth = p_z) into d_loco[i]; the feet
 * move with the body in x, y (footstep relocation is not simulated). The step is the handle's
 * dt (dtMPC). Asynchronous on the handle's stream. */
CMPC_EXTERNC int cmpc_batch_rollout(cmpc_batch* h, float* d_loco, const float* d_records,
                                    const float* d_forces, const float* d_xi6,
                                    const uint8_t* d_due, int batch);
/* Measurement hooks: record HIP events on the handle's stream around the next `steps` solves;
 * read back per-solve ms pairs [class 1's launch, the time after it until the wide size classes
 * have joined] and the number of instances the last solve listed for the wide classes
 * (n > 64). Synchronises. cmpc_batch_solve_due is recorded the same way (its classify pass
 * precedes the first event); the count is then of due instances only. */
CMPC_EXTERNC int cmpc_batch_enable_timing(cmpc_batch* h, int steps);
/* The same on every `every`-th solve only (the first of each group of `every`), `steps` of them:
 * a timed loop then pays the event packets on a fraction of its solves. */
CMPC_EXTERNC int cmpc_batch_enable_timing_every(cmpc_batch* h, int steps, int every);
CMPC_EXTERNC int cmpc_batch_read_timing(cmpc_batch* h, float* ms, int* steps_recorded,
                                        int* class1_overflow);
/* Stream the handle runs on (hipStream_t). */
CMPC_EXTERNC void* cmpc_batch_stream(cmpc_batch* h);
/* Last HIP error string for this thread (diagnostics). */
CMPC_EXTERNC const char* cmpc_last_error(void);

#endif /* CMPC_SOLVER_H */
