/*
 * se3mpc.h -- C ABI of libse3mpc.so, the MI355X (gfx950) SE(3) MPC inner solver.
 *
 * Drop-in boundary for the hot path of DART-Planner's SE3MPCPlanner
 * (reference: src/dart_planner/planning/se3_mpc_planner.py, "planner.py" below).  The
 * reference has no FFI of its own (it is pure Python on NumPy/SciPy); these entry points are
 * what a ctypes binding inside that file would call instead of its NumPy/SciPy arithmetic.
 * INTEGRATION.md shows that binding.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++/torch types.  Every function returns an
 *     int status (SE3MPC_OK == 0, negative = error); nothing throws across the ABI.
 *   - All data pointers are DEVICE pointers (HBM) owned by the caller; the library never
 *     allocates or frees device memory and never synchronises the stream (graph-capturable).
 *     `stream` is a hipStream_t passed as void* (NULL = the default stream).
 *   - Two arithmetic types per entry point: `_f32` (production) and `_f64` (the tolerance
 *     check of BASELINE.json config 5).  Parameters are always doubles on the host side.
 *   - Two data layouts:
 *       "lane layout"  (evaluation kernels): row-major [row][b], b fastest, leading dimension
 *         `ld` >= B elements -- one trajectory per lane, every (row) access of a wavefront is
 *         one coalesced 256-B line.  Rows of a decision vector follow the reference packing
 *         (planner.py:361-376): P block rows 3k+a, V block rows 3N+3k+a, T block rows
 *         6N+3k+a (k = step, a = axis).
 *       "problem layout" (solver): [b][row], row fastest -- the reference's own packing of one
 *         decision vector per problem; one 64-lane wavefront owns one problem.
 *     se3mpc_transpose_* converts between the two.
 *   - B == 0 is legal everywhere and is a no-op.  1 <= horizon <= SE3MPC_MAX_HORIZON.
 */
#ifndef SE3MPC_H
#define SE3MPC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SE3MPC_ABI_VERSION 1
#define SE3MPC_MAX_HORIZON 64      /* 9*N <= 576 decision variables per problem            */
#define SE3MPC_MAX_CORRECTIONS 10  /* L-BFGS memory m (SciPy default maxcor = 10)          */
#define SE3MPC_MAX_SPHERES 256     /* obstacle table staged in LDS (4 KB)                  */
#define SE3MPC_MAX_SWARM 1024      /* drones per swarm (se3mpc_mppi_closed_loop_swarm_*)   */
#define SE3MPC_MAX_TRACKS 16       /* tracked spheres (se3mpc_mppi_tracks_*): an LDS slab [N][Kt][4] */

enum se3mpc_status {
  SE3MPC_OK = 0,
  SE3MPC_ERR_NULL = -1,        /* a required pointer is NULL                               */
  SE3MPC_ERR_HORIZON = -2,     /* horizon outside [1, SE3MPC_MAX_HORIZON]                  */
  SE3MPC_ERR_SHAPE = -3,       /* B < 0, ld < B, K out of range, ...                       */
  SE3MPC_ERR_PARAM = -4,       /* non-finite / non-positive mass, dt, ...                  */
  SE3MPC_ERR_WORKSPACE = -5,   /* workspace too small                                      */
  SE3MPC_ERR_LAUNCH = -6,      /* HIP reported a launch error (see se3mpc_last_error)      */
  SE3MPC_ERR_NO_DEVICE = -7    /* no gfx950 device visible                                 */
};

/* SE3MPCConfig (planner.py:36-79) + constructor constants (planner.py:149-151), unit-stripped
 * to SI magnitudes.  se3mpc_default_params() fills the reference defaults. */
typedef struct se3mpc_params {
  int32_t horizon;              /* prediction_horizon N            (planner.py:41, default 6) */
  int32_t has_goal;             /* 0: goal_position is None -> goal terms skipped (:524,:546,:567) */
  double dt;                    /* planner.py:99-105 (timing manager: 1/400 s)                */
  double mass;                  /* 1.5 kg  (planner.py:149)                                   */
  double gravity;               /* 9.81    (planner.py:150)                                   */
  double position_weight;       /* 100     (planner.py:56)                                    */
  double velocity_weight;       /* 10      (planner.py:57)                                    */
  double acceleration_weight;   /* 1       (planner.py:58)                                    */
  double thrust_weight;         /* 0.1     (planner.py:59)                                    */
  double terminal_factor;       /* 10      (planner.py:548)                                   */
  double position_bound;        /* 100 m   (planner.py:384)                                   */
  double max_velocity;          /* 10 m/s  (planner.py:45, :388)                              */
  double max_acceleration;      /* 15      (planner.py:46, :489)                              */
  double max_thrust;            /* 25 N    (planner.py:48)                                    */
  double min_thrust;            /* 2 N     (planner.py:49)                                    */
  double max_tilt_angle;        /* pi/4    (planner.py:52, :393)                              */
  double safety_margin;         /* 1.5 m   (planner.py:64, :509)                              */
  /* scipy.optimize.minimize(method="L-BFGS-B") options as the reference sets them (:256-268) */
  int32_t max_iterations;       /* maxiter = 15 (planner.py:67)                               */
  int32_t max_corrections;      /* maxcor  = 10 (SciPy default)                               */
  int32_t max_linesearch;       /* maxls   = 20 (SciPy default)                               */
  int32_t max_fun;              /* maxfun  = 15000 (SciPy default)                            */
  double pgtol;                 /* gtol = convergence_tolerance = 0.05 (planner.py:264)       */
  double ftol;                  /* ftol = 10*convergence_tolerance = 0.5 (planner.py:265)     */
} se3mpc_params;

/* Per-problem result of the solver, mirroring scipy's OptimizeResult fields the reference
 * reads (planner.py:271-278): status 0 = converged, 1 = iteration/evaluation limit,
 * 2 = abnormal termination in line search.  `task` is the L-BFGS-B stop reason.  As in SciPy
 * the limits win: a line search that ends abnormally after nfev has passed max_fun (or nit has
 * reached max_iterations) reports status 1 with task SE3MPC_TASK_ABNORMAL. */
typedef struct se3mpc_solve_info {
  double fun;        /* f at the returned x                                              */
  int32_t nit;       /* iterations                                                       */
  int32_t nfev;      /* objective/gradient evaluations                                   */
  int32_t status;    /* scipy status: 0, 1 or 2                                          */
  int32_t task;      /* enum se3mpc_task                                                 */
} se3mpc_solve_info;

enum se3mpc_task {
  SE3MPC_TASK_CONV_PGTOL = 1,    /* CONVERGENCE: NORM OF PROJECTED GRADIENT <= PGTOL      */
  SE3MPC_TASK_CONV_FTOL = 2,     /* CONVERGENCE: REL_REDUCTION_OF_F <= FACTR*EPSMCH       */
  SE3MPC_TASK_STOP_MAXITER = 3,  /* STOP: TOTAL NO. OF ITERATIONS REACHED LIMIT           */
  SE3MPC_TASK_STOP_MAXFUN = 4,   /* STOP: TOTAL NO. OF F,G EVALUATIONS EXCEEDS LIMIT      */
  SE3MPC_TASK_ABNORMAL = 5,      /* ABNORMAL TERMINATION IN LNSRCH                        */
  SE3MPC_TASK_OVERFLOW = 6       /* internal: first-tier LDS too small, re-solved by the second launch; never returned */
};

/* ------------------------------------------------------------------ library / params */
int se3mpc_abi_version(void);
/* 0-terminated message of the last failing HIP call on this thread ("" if none). */
const char* se3mpc_last_error(void);
/* Number of visible gfx950 devices (0 if none / HIP not usable); never fails. */
int se3mpc_device_count(void);
/* Reference defaults (planner.py:36-79, :149-151); horizon 6, dt 1/400, has_goal 1. */
int se3mpc_default_params(se3mpc_params* out);
/* SE3MPC_OK or the error a kernel entry point would return for these params. */
int se3mpc_check_params(const se3mpc_params* p);

/* ------------------------------------------------------------------ lane layout: [row][b]
 * Common arguments: B trajectories, leading dimension ld (elements), device pointers.
 * p0, v0, goal: [3][ld].   X: [9N][ld].   T: [3N][ld].
 */

/* Cold start, replaces _create_straight_line_initialization (planner.py:329-359); with
 * project != 0 also clips into the box of _setup_optimization_bounds (planner.py:378-402),
 * which is what L-BFGS-B does to x0 before its first evaluation.  X0: [9N][ld]. */
int se3mpc_init_f32(const se3mpc_params* p, int B, int ld, const float* p0, const float* v0,
                    const float* goal, int project, float* X0, void* stream);
int se3mpc_init_f64(const se3mpc_params* p, int B, int ld, const double* p0, const double* v0,
                    const double* goal, int project, double* X0, void* stream);

/* Objective and the reference's gradient on the full decision vector, replaces
 * _objective_function (planner.py:516-550) and _objective_gradient (planner.py:552-580,
 * reproduced as is -- it is not the derivative of the objective).  f: [B]; g: [9N][ld] or NULL. */
int se3mpc_cost_grad_f32(const se3mpc_params* p, int B, int ld, const float* X, const float* goal,
                         float* f, float* g, void* stream);
int se3mpc_cost_grad_f64(const se3mpc_params* p, int B, int ld, const double* X, const double* goal,
                         double* f, double* g, void* stream);

/* Equality residuals of the translational dynamics, replaces _dynamics_constraints
 * (planner.py:426-462).  R: [6N][ld], row order as the reference: P0-p0 (3), V0-v0 (3), then
 * per k = 0..N-2 the position residual (3) and the velocity residual (3). */
int se3mpc_dynamics_residual_f32(const se3mpc_params* p, int B, int ld, const float* X, const float* p0,
                                 const float* v0, float* R, void* stream);
int se3mpc_dynamics_residual_f64(const se3mpc_params* p, int B, int ld, const double* X, const double* p0,
                                 const double* v0, double* R, void* stream);

/* Sphere-obstacle inequality residuals, replaces _obstacle_constraints (planner.py:499-514).
 * spheres: device [K][4] = (cx, cy, cz, radius), 0 <= K <= SE3MPC_MAX_SPHERES, staged in LDS.
 * C: [N*K][ld] (row k*K + j) or NULL; cmin: [B] = min over (k,j) or NULL;
 * viol: [B] = sum over (k,j) of max(0, -c) or NULL (the in-kernel reduced forms). */
int se3mpc_obstacle_residual_f32(const se3mpc_params* p, int B, int ld, const float* X, const float* spheres,
                                 int K, float* C, float* cmin, float* viol, void* stream);
int se3mpc_obstacle_residual_f64(const se3mpc_params* p, int B, int ld, const double* X, const double* spheres,
                                 int K, double* C, double* cmin, double* viol, void* stream);

/* Replaces _physical_constraints (planner.py:472-497).  C: [4N][ld]: N velocity rows,
 * N acceleration rows, then per k (max_thrust^2 - |T|^2, |T|^2 - min_thrust^2). */
int se3mpc_physical_constraints_f32(const se3mpc_params* p, int B, int ld, const float* X, float* C, void* stream);
int se3mpc_physical_constraints_f64(const se3mpc_params* p, int B, int ld, const double* X, double* C, void* stream);

/* Replaces _extract_solution_from_result + _compute_attitudes_and_rates (planner.py:582-654).
 * T: [3N][ld] (the T block of X).  acc, att, rates: [3N][ld]; thrust: [N][ld]; any may be NULL. */
int se3mpc_extract_f32(const se3mpc_params* p, int B, int ld, const float* T, float* acc, float* att,
                       float* rates, float* thrust, void* stream);
int se3mpc_extract_f64(const se3mpc_params* p, int B, int ld, const double* T, double* acc, double* att,
                       double* rates, double* thrust, void* stream);

/* Shooting form (the build's canonical "rollout"): forward rollout of the
 * recurrence that planner.py:449-460 writes as residuals, the objective of planner.py:516-550
 * on the rolled-out states, and its exact gradient wrt the thrust sequence by the reverse
 * sweep.  cost: [B]; gradT: [3N][ld] or NULL; P, V: [3N][ld] or both NULL (rolled-out states).
 * wave_keys: NULL, or [ceil(B/64)] device words: the kernel WRITES slot w = min over trajectories
 * 64w..64w+63 of (orderable(cost[b]) << 32 | (index_base + b)) -- the batch argmin fused into the
 * rollout, one plain store per wavefront, no atomics, no pre-initialisation; se3mpc_reduce_keys folds
 * the slots into one key per batch (same packed key as se3mpc_argmin_*). */
int se3mpc_rollout_cost_grad_f32(const se3mpc_params* p, int B, int ld, const float* p0, const float* v0,
                                 const float* goal, const float* T, float* cost, float* gradT, float* P,
                                 float* V, uint64_t* wave_keys, uint32_t index_base, void* stream);
int se3mpc_rollout_cost_grad_f64(const se3mpc_params* p, int B, int ld, const double* p0, const double* v0,
                                 const double* goal, const double* T, double* cost, double* gradT, double* P,
                                 double* V, uint64_t* wave_keys, uint32_t index_base, void* stream);

/* Multi-batch launch of the same kernel: `nbatch` independent batches in ONE launch (grid.y), laid out as
 * consecutive blocks -- p0, v0, goal: [nbatch][3][ld]; T, gradT: [nbatch][3N][ld]; cost: [nbatch][ld];
 * wave_keys: NULL or [nbatch][ceil(B/64)].  For callers that hold many independent sample
 * batches (Monte-Carlo sweeps, several planners): one launch amortises the launch latency that
 * dominates a single 8192-rollout batch.  1 <= nbatch <= 65535. */
int se3mpc_rollout_cost_grad_batched_f32(const se3mpc_params* p, int B, int ld, int nbatch, const float* p0,
                                         const float* v0, const float* goal, const float* T, float* cost,
                                         float* gradT, uint64_t* wave_keys, uint32_t index_base, void* stream);
int se3mpc_rollout_cost_grad_batched_f64(const se3mpc_params* p, int B, int ld, int nbatch, const double* p0,
                                         const double* v0, const double* goal, const double* T, double* cost,
                                         double* gradT, uint64_t* wave_keys, uint32_t index_base, void* stream);

/* The same rollout fused with the sphere-obstacle residuals of planner.py:499-514 evaluated on the ROLLED-OUT
 * positions (BASELINE.json config 3): per-step positions staged in LDS, sphere table in LDS, cmin[b] = min over
 * (k, j) of |P_k - c_j|^2 - (r_j + margin)^2 and viol[b] = sum of max(0, -residual); neither the states nor the
 * N*K residuals are written to HBM.  spheres: [K][4]; cmin, viol: [B] (either may be NULL); gradT may be NULL. */
int se3mpc_rollout_obstacles_f32(const se3mpc_params* p, int B, int ld, const float* p0, const float* v0,
                                 const float* goal, const float* T, float* cost, float* gradT, const float* spheres,
                                 int K, float* cmin, float* viol, uint64_t* wave_keys, uint32_t index_base, void* stream);
int se3mpc_rollout_obstacles_f64(const se3mpc_params* p, int B, int ld, const double* p0, const double* v0,
                                 const double* goal, const double* T, double* cost, double* gradT, const double* spheres,
                                 int K, double* cmin, double* viol, uint64_t* wave_keys, uint32_t index_base, void* stream);

/* Multi-batch launch of the fused kernel (grid.y = batch), operands laid out as in se3mpc_rollout_cost_grad_batched_*:
 * p0, v0, goal: [nbatch][3][ld]; T, gradT: [nbatch][3N][ld]; cost, cmin, viol: [nbatch][ld]; wave_keys: NULL or
 * [nbatch][ceil(B/64)]; ONE sphere table [K][4] shared by all batches.  1 <= nbatch <= 65535. */
int se3mpc_rollout_obstacles_batched_f32(const se3mpc_params* p, int B, int ld, int nbatch, const float* p0,
                                         const float* v0, const float* goal, const float* T, float* cost, float* gradT,
                                         const float* spheres, int K, float* cmin, float* viol, uint64_t* wave_keys,
                                         uint32_t index_base, void* stream);
int se3mpc_rollout_obstacles_batched_f64(const se3mpc_params* p, int B, int ld, int nbatch, const double* p0,
                                         const double* v0, const double* goal, const double* T, double* cost, double* gradT,
                                         const double* spheres, int K, double* cmin, double* viol, uint64_t* wave_keys,
                                         uint32_t index_base, void* stream);

/* `iters` iterations of the shooting form in ONE launch -- the on-device replacement of a host-driven optimisation loop over the
 * rollout (north_star: "replacing DART-Planner's ... optimisation loop"; reference loop site planner.py:256-268): projected gradient
 * descent on every trajectory's thrust sequence,  T <- clip(T - step * dcost/dT, thrust box of planner.py:390-400),  `iters` times,
 * then one last evaluation at the final T.  The thrust sequence stays in registers between iterations: only iteration 0 reads T_in
 * and only the last evaluation writes (T_out, cost, gradT) -- HBM traffic per launch is that of ONE rollout whatever `iters` is.
 * iters = 0 is se3mpc_rollout_cost_grad_* plus a copy of T.  T_out may alias T_in.  cost_first: NULL or [B] = the cost at T_in;
 * cost: [B] = the cost at T_out; gradT: NULL or [3N][ld] = the gradient at T_out; wave_keys as in se3mpc_rollout_cost_grad_*.
 * Multi-batch (grid.y): operands as in se3mpc_rollout_cost_grad_batched_* with T_out / cost_first laid out like T / cost.
 * se3mpc_projected_step_* is one descent step as its own launch (T_out = clip(T - step * gradT)): iterating
 * se3mpc_rollout_cost_grad_* + se3mpc_projected_step_* from the host is what this entry point replaces. */
int se3mpc_rollout_iterate_f32(const se3mpc_params* p, int B, int ld, int nbatch, int iters, double step, const float* p0,
                               const float* v0, const float* goal, const float* T_in, float* T_out, float* cost_first, float* cost,
                               float* gradT, uint64_t* wave_keys, uint32_t index_base, void* stream);
int se3mpc_rollout_iterate_f64(const se3mpc_params* p, int B, int ld, int nbatch, int iters, double step, const double* p0,
                               const double* v0, const double* goal, const double* T_in, double* T_out, double* cost_first, double* cost,
                               double* gradT, uint64_t* wave_keys, uint32_t index_base, void* stream);
/* The obstacle-aware iteration loop (BASELINE config 3 inside the loop): se3mpc_rollout_iterate_* on the objective
 *     running cost (planner.py:516-550 on the rolled-out states) + obstacle_weight * sum_k sum_j max(0, -c_kj)^2,
 *     c_kj = |P_k - c_j|^2 - (r_j + safety_margin)^2      (the reference's sphere residual, planner.py:499-514)
 * -- the BUILD'S EXTENSION: the reference forms these residuals and never hands them to its solver (:250 vs :256-268; its
 * obstacle_weight, :63 = 1000, is never read).  The exact gradient of the penalty reaches the thrust sequence through the same
 * adjoint sweep.  spheres: [K][4] rows (cx, cy, cz, r) as se3mpc_rollout_obstacles_* (0 <= K <= SE3MPC_MAX_SPHERES; K = 0 is the
 * plain loop's numbers at the obstacle form's speed).  cost / cost_first include the penalty; penalty: NULL or [B] = the penalty
 * alone at T_out (0: the plan keeps the margin of every sphere at every step).  Everything else as se3mpc_rollout_iterate_*.
 * wave_keys: written inside the launch (the library presets the [nbatch][ceil(B/64)] slots itself: workgroups of 32 trajectories fold
 * pairwise into a slot). */
int se3mpc_rollout_iterate_obstacles_f32(const se3mpc_params* p, int B, int ld, int nbatch, int iters, double step, const float* p0,
                                         const float* v0, const float* goal, const float* T_in, float* T_out, float* cost_first,
                                         float* cost, float* gradT, const float* spheres, int K, double obstacle_weight,
                                         float* penalty, uint64_t* wave_keys, uint32_t index_base, void* stream);
int se3mpc_rollout_iterate_obstacles_f64(const se3mpc_params* p, int B, int ld, int nbatch, int iters, double step, const double* p0,
                                         const double* v0, const double* goal, const double* T_in, double* T_out, double* cost_first,
                                         double* cost, double* gradT, const double* spheres, int K, double obstacle_weight,
                                         double* penalty, uint64_t* wave_keys, uint32_t index_base, void* stream);
int se3mpc_projected_step_f32(const se3mpc_params* p, int B, int ld, double step, const float* T, const float* gradT, float* T_out,
                              void* stream);
int se3mpc_projected_step_f64(const se3mpc_params* p, int B, int ld, double step, const double* T, const double* gradT, double* T_out,
                              void* stream);

/* The tail of a shooting-form plan in ONE launch of one wavefront (the caller side of se3mpc_rollout_iterate_* / _obstacles_*, i.e. what
 * _solve_se3_mpc does after its optimiser returns, planner.py:270-280 -> _extract_solution_from_result :582-602 -> _compute_attitudes_and_rates
 * :604-654): fold the descent launch's wave_keys[n_slots] to the winning key (stored to key_out if not NULL), take column
 * (key & 0xffffffff) - index_base of T ([3N][ld], the descent's T_out) as doubles, roll it out from state = (p0, v0, goal) [9 doubles; goal ignored
 * when has_goal == 0] with the recurrence of planner.py:449-460 and the objective of :516-550, extract accelerations, attitudes, body rates and
 * thrust magnitudes, and -- K > 0 -- the sphere penalty obstacle_weight * sum max(0, -c_kj)^2 left at that plan (spheres: [K][4] doubles, rows
 * (cx, cy, cz, r) before the safety margin).  out: 19 N + 3 doubles = [P | V | T | acc | att | rates (N x 3 each) | thrust (N) | cost | penalty |
 * cost + penalty]; out, key_out and state may be pinned host memory (the kernel's loads / stores then are the copies).  B >= 1. */
int se3mpc_shooting_finish_f32(const se3mpc_params* p, int B, int ld, const float* T, const uint64_t* wave_keys, int n_slots,
                               uint32_t index_base, const double* state, const double* spheres, int K, double obstacle_weight, double* out,
                               uint64_t* key_out, void* stream);
int se3mpc_shooting_finish_f64(const se3mpc_params* p, int B, int ld, const double* T, const uint64_t* wave_keys, int n_slots,
                               uint32_t index_base, const double* state, const double* spheres, int K, double obstacle_weight, double* out,
                               uint64_t* key_out, void* stream);

/* keys_out[i] = min over wave_keys[i][0..per_batch) for i < nbatch (one small workgroup per batch). */
int se3mpc_reduce_keys(const uint64_t* wave_keys, int per_batch, int nbatch, uint64_t* keys_out, void* stream);

/* Tuning knob for measurements: which implementation of the rollout the entry point above
 * launches.  0 = auto (default), 1 = exact-N register arrays (N in {6,20,30,50}; falls back to
 * 3 otherwise), 2 = per-step state tiles staged in LDS, 3 = register-light reversible sweep, 4 / 5 = 1 / 3
 * with one wavefront looping over the three axes, 6 = 32-step register bucket with guarded steps (f32, horizons 17..32;
 * else 3).  variant + 8 * (flags + 1) forces the memory-policy
 * flags of the benchmarked instantiation (horizon 30, f32, gradient): bit 0 nt loads, bit 1 nt stores,
 * bit 2 XCD-contiguous block order; the default is all three (7).  + 128 / + 256 / + 384 forces the workgroup of
 * se3mpc_rollout_obstacles_* to 3 / 8 / 4 wavefronts (default: 8 while 8 x workgroups <= 1024, else 4 for the exact-N = 50 register
 * sweep -- three axis wavefronts and a helper -- and 3 otherwise); + 128 also forces
 * se3mpc_rollout_iterate_obstacles_* to its narrow shape (3 wavefronts on 64 trajectories, sphere table in LDS; default: 7 wavefronts on
 * 32 trajectories, four of them helpers with the table in registers).  + 512 / + 1024: the
 * write-heavy float32 lane kernels never / always take their 16-byte-per-lane form (four trajectories per lane; needs B and ld
 * multiples of 4 and 16-byte aligned operands; default: from 262144 trajectories up).
 * + 2048: se3mpc_rollout_obstacles_f32 forms its residuals on the matrix core (v_mfma_f32_16x16x4_f32 on the expanded form |P|^2 - 2 P.c + |c|^2 - R^2:
 * measured evidence for DESIGN.md 5.3, no faster than the default packed-VALU difference form and four digits less precise next to a sphere's surface).
 * All compute the same quantities. */
int se3mpc_set_rollout_variant(int variant);

/* Replaces is_plan_valid (planner.py:717-737): valid[b] = 1 iff all positions finite,
 * z >= 0.1 and |v| <= 20.  P, V: [3N][ld] (V may be NULL). */
int se3mpc_is_plan_valid_f32(const se3mpc_params* p, int B, int ld, const float* P, const float* V,
                             int32_t* valid, void* stream);
int se3mpc_is_plan_valid_f64(const se3mpc_params* p, int B, int ld, const double* P, const double* V,
                             int32_t* valid, void* stream);

/* Batch argmin: *key = min over b of (orderable(cost[b]) << 32 | (index_base + b)); the packed
 * 64-bit key is what the multi-GPU path all-reduces with MIN.
 * The function resets *key itself (stream-ordered).  Decode with se3mpc_key_*. */
int se3mpc_argmin_f32(int B, const float* cost, uint32_t index_base, uint64_t* key, void* stream);
int se3mpc_argmin_f64(int B, const double* cost, uint32_t index_base, uint64_t* key, void* stream);
uint32_t se3mpc_key_index(uint64_t key);
float se3mpc_key_cost(uint64_t key);   /* f64 costs are ordered through their float rounding */

/* Population sums of a lane-layout block -- the other exchange of the multi-GPU path ("for an
 * MPPI-style averaged gradient: all-reduce(SUM) of 3N floats"): out[r] = sum_b w_b * X[r][b] for r < rows and
 * out[rows] = sum_b w_b, accumulated in float64 with a fixed summation tree.  w_b = 1 when cost == NULL (plain
 * mean of, e.g., the rollout's thrust gradient), else the MPPI weight exp(-(cost[b] - cost_ref) / temperature),
 * where cost_ref is the host argument, or -- when ref_key != NULL -- the cost held in that device key (the fused /
 * all-reduced argmin key: the global minimum, so every rank weighs on the same scale).  One all-reduce(SUM) of the
 * rows + 1 doubles, then out[r] / out[rows], gives the population mean over all ranks.
 * workspace: device double[se3mpc_population_workspace(rows, B)]. */
int se3mpc_population_workspace(int rows, int B);
int se3mpc_population_sums_f32(int rows, int B, int ld, const float* X, const float* cost, double cost_ref,
                               const uint64_t* ref_key, double temperature, double* out, double* workspace, void* stream);
int se3mpc_population_sums_f64(int rows, int B, int ld, const double* X, const double* cost, double cost_ref,
                               const uint64_t* ref_key, double temperature, double* out, double* workspace, void* stream);

/* MPPI (model-predictive path integral) on the shooting form, `iters` iterations of `nprob` independent problems in ONE launch (one
 * workgroup per problem; nothing per sample touches HBM).  Lane layout over problems: p0, v0, goal: [3][ld]; U_in, U_out: [3N][ld] (the
 * nominal thrust sequence, rows 3k+a as the T block; U_out may alias U_in); cost: [ld]; trace: NULL or [iters][ld]; keys: NULL or [ld].
 * Iteration i (g = iter_base + *iter_offset + i; iter_offset: NULL or a device word, so that a captured graph can advance it) of problem
 * q = index_base + p:
 *   noise   x0..x3 = Philox4x32-10(counter (q, s, g, k), key (seed & 0xffffffff, seed >> 32)), u_j = (x_j + 0.5) * 2^-32 in the entry
 *           point's type, n = (sqrt(-2 ln u0) cos 2 pi u1, sqrt(-2 ln u0) sin 2 pi u1, sqrt(-2 ln u2) cos 2 pi u3); sample s = 0 has none
 *   sample  T_s[k][a] = clip(U[k][a] + sigma * n_a) into the thrust box of se3mpc_projected_step_* (+-txy for x, y; [min, max] for z)
 *   cost    c_s = the cost of se3mpc_rollout_cost_grad_* at T_s + obstacle_weight * sum_k sum_j max(0, -(|P_k - c_j|^2 - (r_j + margin)^2))^2
 *           (the penalty of se3mpc_rollout_iterate_obstacles_*; spheres: [K][4] rows (cx, cy, cz, r) shared by all problems, K = 0: none)
 *   update  m = min_s c_s, w_s = exp(-(c_s - m) / temperature), U <- sum_s w_s T_s / sum_s w_s, accumulated in float64 in a fixed order
 *           (results are identical run to run); trace[i][p] = m.
 * cost[p] = the cost (with the penalty) of U_out, evaluated once after the last update; keys[p] = orderable(cost) << 32 | q, the key of
 * se3mpc_argmin_* (se3mpc_shooting_finish_*(B = 1, n_slots = 1) takes it as is).  iters = 0 evaluates and copies U_in.  nprob = 0 is a
 * no-op.  64 <= S <= 65536, S a multiple of 64 (SE3MPC_ERR_SHAPE otherwise, as K outside [0, SE3MPC_MAX_SPHERES]); sigma >= 0, temperature
 * > 0 and obstacle_weight >= 0 finite (SE3MPC_ERR_PARAM).  Every rejected call sets se3mpc_last_error and launches nothing.
 * temperature is absolute, in cost units. */
int se3mpc_mppi_f32(const se3mpc_params* p, int nprob, int ld, int S, int iters, double sigma, double temperature, uint64_t seed,
                    uint32_t iter_base, const uint32_t* iter_offset, uint32_t index_base, const float* p0, const float* v0, const float* goal,
                    const float* U_in, float* U_out, const float* spheres, int K, double obstacle_weight, float* cost, float* trace,
                    uint64_t* keys, void* stream);
int se3mpc_mppi_f64(const se3mpc_params* p, int nprob, int ld, int S, int iters, double sigma, double temperature, uint64_t seed,
                    uint32_t iter_base, const uint32_t* iter_offset, uint32_t index_base, const double* p0, const double* v0, const double* goal,
                    const double* U_in, double* U_out, const double* spheres, int K, double obstacle_weight, double* cost, double* trace,
                    uint64_t* keys, void* stream);
/* se3mpc_mppi_* around spheres that MOVE with constant velocity.  The operands of se3mpc_mppi_*, and after `spheres`:
 * sphere_vel [K][3] rows (vx, vy, vz) in m/s, same type, shared by all problems; sphere_t0: the time of step 0 on the table's clock, i.e.
 * the centres of `spheres` hold at time 0 of that clock and the plan starts sphere_t0 seconds later.  The penalty of step k (on the state
 * before step k, as in se3mpc_mppi_*) is taken against the centres at
 *   tau_k = sphere_t0 + (double)k * dt,     tR = tau_k rounded to the kernel's type,     centre_a = c_a + v_a * tR   (may be one FMA)
 * and is then se3mpc_mppi_*'s expression dz^2 + (dy^2 + (dx^2 - (r + margin)^2)).  With sphere_vel = 0 the centre is exactly c for every
 * finite tau and every output equals se3mpc_mppi_*'s bit for bit.  tR is tau in the KERNEL's type: keep sphere_t0 and the span of a run
 * small (seconds since the table was made, not epoch time) -- a float32 kernel at tau = 1.7e9 has an ulp of 128 s.  Rebase the centres
 * on the host in float64 instead (c + v * (now - t_table), sphere_t0 = 0).
 * Checks: those of se3mpc_mppi_*, then a non-finite sphere_t0: SE3MPC_ERR_PARAM; sphere_vel NULL with K > 0: SE3MPC_ERR_NULL.  K = 0 is
 * allowed and reads neither table.  There is no split form. */
int se3mpc_mppi_moving_f32(const se3mpc_params* p, int nprob, int ld, int S, int iters, double sigma, double temperature, uint64_t seed,
                           uint32_t iter_base, const uint32_t* iter_offset, uint32_t index_base, const float* p0, const float* v0,
                           const float* goal, const float* U_in, float* U_out, const float* spheres, const float* sphere_vel, double sphere_t0,
                           int K, double obstacle_weight, float* cost, float* trace, uint64_t* keys, void* stream);
int se3mpc_mppi_moving_f64(const se3mpc_params* p, int nprob, int ld, int S, int iters, double sigma, double temperature, uint64_t seed,
                           uint32_t iter_base, const uint32_t* iter_offset, uint32_t index_base, const double* p0, const double* v0,
                           const double* goal, const double* U_in, double* U_out, const double* spheres, const double* sphere_vel,
                           double sphere_t0, int K, double obstacle_weight, double* cost, double* trace, uint64_t* keys, void* stream);
/* se3mpc_mppi_moving_* around spheres with a PREDICTED PATH as well: an obstacle whose centre is given per step of the
 * horizon -- a pedestrian track, another vehicle's published trajectory -- not as c + v t.  The operands of se3mpc_mppi_moving_*, and
 * after K: tracks, device [N][Kt][4] = (x, y, z, radius) per problem, same type; Kt in [0, SE3MPC_MAX_TRACKS] with K + Kt <=
 * SE3MPC_MAX_SPHERES; track_stride, in elements between the slabs of consecutive problems (0: one slab for all; otherwise >= 4 N Kt).
 * Row [k][j] is tracked sphere j at the time of the state before step k -- the instant tau_k of se3mpc_mppi_moving_* -- so the penalty of
 * step k walks the K moving rows exactly as se3mpc_mppi_moving_* does and then the Kt rows [k][.] in rising j with the same expression
 * dz^2 + (dy^2 + (dx^2 - (r + margin)^2)) and no time arithmetic; the penalties add up in that order.  The slab is staged once per launch
 * (N = 64, Kt = 16 in float64: 32 KB of LDS).  Kt = 0 reads no slab and gives se3mpc_mppi_moving_*'s outputs bit for bit; Kt tracks that
 * hold one centre at every step give those of se3mpc_mppi_moving_* on K + Kt rows whose last Kt velocities are zero.
 * Checks: those of se3mpc_mppi_moving_* with the same codes, then Kt outside [0, SE3MPC_MAX_TRACKS], K + Kt > SE3MPC_MAX_SPHERES or a
 * track_stride that is neither 0 nor >= 4 N Kt: SE3MPC_ERR_SHAPE; tracks NULL with Kt > 0: SE3MPC_ERR_NULL.  There is no split form. */
int se3mpc_mppi_tracks_f32(const se3mpc_params* p, int nprob, int ld, int S, int iters, double sigma, double temperature, uint64_t seed,
                           uint32_t iter_base, const uint32_t* iter_offset, uint32_t index_base, const float* p0, const float* v0,
                           const float* goal, const float* U_in, float* U_out, const float* spheres, const float* sphere_vel, double sphere_t0,
                           int K, const float* tracks, int Kt, long long track_stride, double obstacle_weight, float* cost, float* trace,
                           uint64_t* keys, void* stream);
int se3mpc_mppi_tracks_f64(const se3mpc_params* p, int nprob, int ld, int S, int iters, double sigma, double temperature, uint64_t seed,
                           uint32_t iter_base, const uint32_t* iter_offset, uint32_t index_base, const double* p0, const double* v0,
                           const double* goal, const double* U_in, double* U_out, const double* spheres, const double* sphere_vel,
                           double sphere_t0, int K, const double* tracks, int Kt, long long track_stride, double obstacle_weight, double* cost,
                           double* trace, uint64_t* keys, void* stream);
/* se3mpc_mppi_* with ONE problem's samples split over `splits` workgroups (split j owns samples [j S / splits, (j + 1) S / splits)), for
 * the call that plans one or a few problems and would otherwise run on one or a few compute units.  Same operands, same noise (the
 * counter (q, s, g, k) does not depend on who draws a sample), same cost, same update, same outputs as se3mpc_mppi_*; only the order of
 * the float64 sums differs: each split sums its own samples as se3mpc_mppi_* does, and the splits' partial sums are folded in split
 * order j = 0 .. splits - 1 against the running minimum.  splits = 1 gives the bytes of se3mpc_mppi_*.  Results are identical run to run
 * and do not depend on how the device schedules the workgroups.
 * The call enqueues iters + 1 launches on `stream` (one per iteration over a grid of splits x nprob workgroups, then one that writes
 * U_out, cost, keys and the last trace row): the kernel boundary hands the partial sums of an iteration to the next.  It allocates
 * nothing and synchronises nothing, so it can be captured into a graph; every launch reads *iter_offset and adds its own iteration
 * number, so a replay advances as se3mpc_mppi_* does.  U_out may alias U_in.
 * workspace: device memory of at least se3mpc_mppi_split_workspace_bytes(p->horizon, nprob, splits) bytes, 8-byte aligned.  It needs no
 * initialisation and holds nothing between calls; two calls in flight at once need a workspace each.  iters = 0 does not touch it.
 * Argument rules: everything se3mpc_mppi_* rejects, with the same codes; also SE3MPC_ERR_SHAPE for splits < 1, S not a multiple of
 * 64 * splits (every split owns whole wavefronts), S / splits < 64, nprob > 65535 and workspace_bytes too small, and SE3MPC_ERR_NULL
 * for workspace == NULL (the last two when iters > 0).  Every rejected call sets se3mpc_last_error and launches nothing.
 * se3mpc_mppi_split_workspace_bytes returns 0 for arguments outside these rules. */
size_t se3mpc_mppi_split_workspace_bytes(int horizon, int nprob, int splits);
int se3mpc_mppi_split_f32(const se3mpc_params* p, int nprob, int ld, int S, int iters, double sigma, double temperature, uint64_t seed,
                          uint32_t iter_base, const uint32_t* iter_offset, uint32_t index_base, const float* p0, const float* v0,
                          const float* goal, const float* U_in, float* U_out, const float* spheres, int K, double obstacle_weight, float* cost,
                          float* trace, uint64_t* keys, int splits, void* workspace, size_t workspace_bytes, void* stream);
int se3mpc_mppi_split_f64(const se3mpc_params* p, int nprob, int ld, int S, int iters, double sigma, double temperature, uint64_t seed,
                          uint32_t iter_base, const uint32_t* iter_offset, uint32_t index_base, const double* p0, const double* v0,
                          const double* goal, const double* U_in, double* U_out, const double* spheres, int K, double obstacle_weight,
                          double* cost, double* trace, uint64_t* keys, int splits, void* workspace, size_t workspace_bytes, void* stream);
/* The samples of ONE iteration (g = iter_base) of se3mpc_mppi_*, materialised for inspection: column p * S + s of T_out [3N][ld_out]
 * (ld_out >= S * nprob) is T_s of problem p; noise: NULL or [3N][ld_out] = the normals n of that column (drawn for s = 0 too, where the
 * sample does not use them); raw: NULL or [4N][ld_out] = the Philox words, row 4k + j = x_j of step k.  Same argument rules. */
int se3mpc_mppi_samples_f32(const se3mpc_params* p, int nprob, int ld, int S, double sigma, uint64_t seed, uint32_t iter_base,
                            uint32_t index_base, const float* U_in, float* T_out, int ld_out, float* noise, uint32_t* raw, void* stream);
int se3mpc_mppi_samples_f64(const se3mpc_params* p, int nprob, int ld, int S, double sigma, uint64_t seed, uint32_t iter_base,
                            uint32_t index_base, const double* U_in, double* T_out, int ld_out, double* noise, uint32_t* raw, void* stream);

/* Obstacle source: the sphere table of se3mpc_obstacle_residual_* straight from a local
 * occupancy grid, replacing the host loop of cloud/main_improved_threelayer.py:387-398 (target 20) and
 * tests/test_se3_mpc_with_mapper.py:29-33 (target 10): occupied = cells with occupancy > threshold in grid
 * order, step = max(1, n_occupied // target), spheres = every step-th occupied cell, all with `radius`.
 * positions: [M][3] (grid order of ExplicitGeometricMapper.get_local_occupancy_grid,
 * perception/explicit_geometric_mapper.py:221-248), occupancy: [M]; spheres: [cap][4] (at most 2*target-1
 * are produced; extra ones are dropped at cap), *count = number written. */
int se3mpc_spheres_from_grid_f32(const float* positions, const float* occupancy, int M, double threshold, int target,
                                 double radius, float* spheres, int cap, int32_t* count, void* stream);
int se3mpc_spheres_from_grid_f64(const double* positions, const double* occupancy, int M, double threshold, int target,
                                 double radius, double* spheres, int cap, int32_t* count, void* stream);

/* [rows][ld_in] <-> [cols][ld_out] tiled transpose through LDS (layout conversion). */
int se3mpc_transpose_f32(int rows, int cols, const float* in, int ld_in, float* out, int ld_out, void* stream);
int se3mpc_transpose_f64(int rows, int cols, const double* in, int ld_in, double* out, int ld_out, void* stream);

/* ------------------------------------------------------------------ voxel map (obstacle source)
 * Device-resident counterpart of ExplicitGeometricMapper (src/dart_planner/perception/explicit_geometric_mapper.py,
 * "mapper.py" below): the sparse voxel dict (mapper.py:74-76) becomes an open-addressing hash table in HBM owned by
 * the caller.  A voxel index (ix, iy, iz) = floor(position / resolution) (mapper.py:93-96, float64) is packed as
 * three 21-bit fields (|index| < 2^20: +-200 km at 0.2 m); SE3MPC_VOXEL_EMPTY marks a free slot.  Positions outside
 * that range read as unknown (prior).  All entry points are stream-ordered and allocate nothing. */
#define SE3MPC_VOXEL_EMPTY 0xFFFFFFFFFFFFFFFFull
#define SE3MPC_VOXEL_MAX_CELLS 1024   /* cells per axis of a local grid (axis tables staged in LDS) */

typedef struct se3mpc_voxel_map {
  uint64_t* keys;      /* [capacity] packed voxel index                                   */
  double* prob;        /* [capacity] occupancy_probability (mapper.py:31)                 */
  int32_t* count;      /* [capacity] observation_count     (mapper.py:33)                 */
  int32_t capacity;    /* power of two, >= 64; keep the load factor under ~0.7            */
  int32_t reserved;
  double resolution;   /* voxel edge in metres (mapper.py:66, default 0.2)                */
  double prior;        /* occupancy of unknown space: prob_prior = 0.5 (mapper.py:83)     */
} se3mpc_voxel_map;

/* keys = EMPTY, prob = prior, count = 0. */
int se3mpc_voxel_clear(const se3mpc_voxel_map* m, void* stream);
/* Create-or-overwrite M voxels (ijk: [M][3] voxel indices; prob: [M], or NULL for `value` everywhere; count_in:
 * [M] observation counts, or NULL to leave counts untouched) -- what add_obstacle does with 0.9
 * (mapper.py:424-447), how a host-built map is uploaded and how a table is re-hashed into a larger one.
 * failed: device int32[2], incremented (not reset): [0] per voxel that could not be stored (table full / index
 * out of range), [1] per voxel that did not exist before. */
int se3mpc_voxel_insert(const se3mpc_voxel_map* m, const int32_t* ijk, const double* prob, double value,
                        const int32_t* count_in, int M, int32_t* failed, void* stream);
/* update_map (mapper.py:102-153) for M <= SE3MPC_VOXEL_MAX_RAYS observations in their order (longer scans: call
 * again with the next chunk): origin [M][3], direction [M][3] (UNIT vectors: the caller normalises, as
 * mapper.py:265 does), distance [M] = min(hit_distance or max_range, map max_range) (:111-112), hit [M] = 1 when the
 * observation carries a hit distance (the ray's last voxel is then updated with like_hit = prob_hit, every other
 * voxel with like_miss = 1 - prob_miss, :319-323).  Voxels are walked with the reference's DDA (:251-312); the
 * clamped Bayesian update (:325-337) does not commute, so every voxel applies its observations in ray order (voxels
 * are independent of each other and proceed in parallel).
 * Workspace (device): ray_keys uint64 [M][max_len] and ray_len int32 [M] (max_len >= 3 * ceil(distance /
 * resolution) + 8 never truncates); slot_rows int32 [capacity] and row_bits uint64
 * [se3mpc_voxel_update_row_words(M, max_len)], both ALL ZERO on entry and left all zero on return.
 * stats: device int32[4] = {voxels walked, walked voxels that could not be stored, truncated rays, voxels created}
 * (reset by the call). */
#define SE3MPC_VOXEL_MAX_RAYS 1024
int se3mpc_voxel_update_rays(const se3mpc_voxel_map* m, const double* origin, const double* direction,
                             const double* distance, const int32_t* hit, int M, double like_hit, double like_miss,
                             uint64_t* ray_keys, int32_t* ray_len, int max_len, int32_t* slot_rows, uint64_t* row_bits,
                             int32_t* stats, void* stream);
long long se3mpc_voxel_update_row_words(int M, int max_len);
/* _trace_ray (mapper.py:251-312) alone, for M rays: ray_keys[ray][0 .. ray_len[ray]) = the packed indices of the
 * walked voxels in walk order (index a = ((key >> (42 - 21 a)) & 0x1FFFFF) - 2^20 for a = 0, 1, 2; SE3MPC_VOXEL_EMPTY
 * for a voxel outside the packable range).  The table is not touched (only m->resolution is used).  stats as in
 * se3mpc_voxel_update_rays ([0] voxels walked, [1] rays dropped, [2] rays truncated). */
int se3mpc_voxel_trace_rays(const se3mpc_voxel_map* m, const double* origin, const double* direction,
                            const double* distance, int M, uint64_t* ray_keys, int32_t* ray_len, int max_len,
                            int32_t* stats, void* stream);
/* Compact the occupied slots (order unspecified): ijk_out [capacity][3], prob_out / count_out [capacity] (may be
 * NULL), *n_out = number of voxels (the caller zeroes nothing: the function resets *n_out itself). */
int se3mpc_voxel_export(const se3mpc_voxel_map* m, int32_t* ijk_out, double* prob_out, int32_t* count_out,
                        int32_t* n_out, void* stream);
/* query_occupancy_batch (mapper.py:155-183): positions [M][3] -> occupancy [M] (float64 as stored). */
int se3mpc_voxel_query_f32(const se3mpc_voxel_map* m, const float* positions, int M, double* occupancy, void* stream);
int se3mpc_voxel_query_f64(const se3mpc_voxel_map* m, const double* positions, int M, double* occupancy, void* stream);
/* is_trajectory_safe (mapper.py:185-219, :339-353) for B trajectories at once: trajectory b = N rows of 3 at
 * P + b * stride (elements; stride = 9N reads the P block of se3mpc_solve_*'s X directly).  Each position is
 * checked with its 6 axis neighbours at +-margin; safe[b] = 1/0, first[b] = index of the first colliding
 * position or -1.  One wavefront per trajectory. */
int se3mpc_voxel_trajectory_safe_f32(const se3mpc_voxel_map* m, const float* P, int B, int N, long long stride,
                                     double margin, double threshold, int32_t* safe, int32_t* first, void* stream);
int se3mpc_voxel_trajectory_safe_f64(const se3mpc_voxel_map* m, const double* P, int B, int N, long long stride,
                                     double margin, double threshold, int32_t* safe, int32_t* first, void* stream);
/* get_local_occupancy_grid (mapper.py:221-248) fused with the grid -> sphere selection of
 * cloud/main_improved_threelayer.py:387-398 / tests/test_se3_mpc_with_mapper.py:29-33, without materialising the
 * grid: n = int(size / resolution) cells per axis at linspace(centre - size/2, centre + size/2, n) (numpy's
 * i * step + start, last = stop), cell order (iz, ix, iy) with iy fastest, occupied = occupancy > threshold,
 * step = max(1, n_occupied // target), every step-th occupied cell becomes (x, y, z, radius).
 * centre: HOST pointer to 3 doubles.  spheres: [cap][4]; count: device int32[2] = {spheres written, n_occupied};
 * workspace: device int32[se3mpc_voxel_local_workspace(n)]. */
int se3mpc_voxel_local_workspace(int cells_per_axis);
int se3mpc_voxel_local_spheres_f32(const se3mpc_voxel_map* m, const double* centre, double size, double threshold,
                                   int target, double radius, float* spheres, int cap, int32_t* count,
                                   int32_t* workspace, void* stream);
int se3mpc_voxel_local_spheres_f64(const se3mpc_voxel_map* m, const double* centre, double size, double threshold,
                                   int target, double radius, double* spheres, int cap, int32_t* count,
                                   int32_t* workspace, void* stream);

/* ------------------------------------------------------------------ uncertainty field (mission layer)
 * Device-resident counterpart of UncertaintyField (src/dart_planner/neural_scene/uncertainty_field.py, "field.py" below): the
 * two dense float64 grids of field.py:58-59 in HBM, owned by the caller, C order with k fastest.  n = ceil((max - min) /
 * resolution) is computed by the caller as field.py:53-55 does.  Float64 only: every number is the reference's.  All entry
 * points are stream-ordered and allocate nothing.
 *
 * Argument rules of this section: a NULL descriptor, grid or required operand: SE3MPC_ERR_NULL; a grid size < 1, more than 2^30
 * voxels, a count (S, N, B) outside [0, 2^30], max_regions outside [1, 2^30], num_targets outside [0, 1024]: SE3MPC_ERR_SHAPE; a resolution that is not finite
 * and positive, a non-finite origin or alpha: SE3MPC_ERR_PARAM; a workspace of fewer words than needed or not 8-byte aligned:
 * SE3MPC_ERR_WORKSPACE.  A count of 0 is a no-op.  Every rejected call sets se3mpc_last_error and launches nothing. */
typedef struct se3mpc_ufield {
  double* uncertainty;        /* [n0][n1][n2] uncertainty_grid   (field.py:58)                  */
  double* observation_count;  /* [n0][n1][n2] observation_count  (field.py:59)                  */
  int32_t n[3];               /* grid_size                       (field.py:53-55)               */
  int32_t reserved;
  double origin[3];           /* scene_bounds[0]                                                */
  double resolution;          /* voxel edge in metres                                           */
} se3mpc_ufield;

/* Words of int32 workspace that every entry point of this section accepts for a grid of nx * ny * nz voxels and max_regions
 * rows (7 words per voxel, 2 per 1024 voxels and 27 per row, at least 2048); negative: SE3MPC_ERR_SHAPE.  The workspace may be
 * dirty: every word a call reads was written by that call. */
long long se3mpc_ufield_workspace(int nx, int ny, int nz, int max_regions);
/* uncertainty = 1, observation_count = 0 (field.py:58-59). */
int se3mpc_ufield_fill(const se3mpc_ufield* f, void* stream);
/* reduce_uncertainty_around_position (field.py:221-260) S times in ONE launch, in index order: centres [S][3], radius [S],
 * radius_voxels [S] = int(radius / resolution) as the caller's float64 gives it (field.py:234), factor [S] = reduction_factor.
 * The bytes of the two grids equal those of S sequential calls. */
int se3mpc_ufield_stamp(const se3mpc_ufield* f, const double* centres, const double* radius, const int32_t* radius_voxels,
                        const double* factor, int S, void* stream);
/* update_uncertainty_field (field.py:90-108): positions [N][3], uncertainty [N], weights [N] or NULL (1.0), alpha = 0.1 in
 * the reference.  Points outside the grid are ignored; points of one voxel are applied in input order.  keys: device
 * int32[N] scratch; workspace: 2 words per voxel. */
int se3mpc_ufield_update_points(const se3mpc_ufield* f, const double* positions, const double* uncertainty,
                                const double* weights, int N, double alpha, int32_t* keys, int32_t* workspace,
                                long long workspace_words, void* stream);
/* get_uncertainty_at_position (field.py:110-125) for B positions [B][3]: out [B], 1.0 outside the bounds. */
int se3mpc_ufield_query(const se3mpc_ufield* f, const double* positions, int B, double* out, void* stream);
/* The sums of get_statistics (field.py:262-289): counts int32[2] = {voxels with observation_count > 0, voxels with
 * uncertainty > threshold}, values [3] = {sum, min, max of the uncertainty}.  A fold in a fixed order: two runs give the
 * same bytes.  workspace: 2048 words. */
int se3mpc_ufield_statistics(const se3mpc_ufield* f, double threshold, int32_t* counts, double* values, int32_t* workspace,
                             long long workspace_words, void* stream);
/* identify_high_uncertainty_regions (field.py:154-182, :308-405): the 6-connected components of uncertainty > threshold.
 * labels int32 [n0][n1][n2]: the smallest raster index of the voxel's component, -1 outside the mask.  Components with
 * voxels * resolution^3 >= min_volume are kept in ascending order of that index (the reference's discovery order), at most
 * max_regions of them; counts int32[2] = {rows written, regions that qualify}.  regions [max_regions][12] = centre 3, min
 * 3, max 3, uncertainty_value, volume, priority, sorted by priority descending as Python's stable sort does; region_roots
 * int32[max_regions] or NULL: the label of each row.  Eight launches, no host round trip; two runs give the same bytes. */
int se3mpc_ufield_regions(const se3mpc_ufield* f, double threshold, double min_volume, int max_regions, int32_t* labels,
                          double* regions, int32_t* region_roots, int32_t* counts, int32_t* workspace,
                          long long workspace_words, void* stream);
/* The target list of get_exploration_targets (field.py:204-219) from the rows and counts of se3mpc_ufield_regions (device):
 * the centres of the first min(num_targets, counts[0]) rows with z = max(z, 2.0); position: HOST pointer to 3 doubles or
 * NULL; with it the targets are stably sorted by distance.  targets [num_targets][3], n_out int32[1]. */
int se3mpc_ufield_targets(const double* regions, const int32_t* counts, int num_targets, const double* position,
                          double* targets, int32_t* n_out, void* stream);

/* ------------------------------------------------------------------ consumer side of the contract
 * Plan sample -> geometric controller -> simulator, one drone per lane.  Reference ("controller.py" =
 * src/dart_planner/control/geometric_controller.py, "onboard.py" = src/dart_planner/control/onboard_controller.py,
 * "simulator.py" = src/dart_planner/utils/drone_simulator.py), unit-stripped and reproduced with its quirks.
 * All arrays are per-drone rows: pos, vel, att (roll, pitch, yaw), omega: [B][3]; time: double [B] (DroneState.timestamp).
 */

/* GeometricControllerConfig (controller.py:26-77) after _apply_tuning_profile (:140-158).  se3mpc_controller_default_params
 * fills the "sitl_optimized" profile (control_config.py:95-111) with the vehicle constants the reference instantiates. */
typedef struct se3mpc_controller_params {
  double kp_pos[3], ki_pos[3], kd_pos[3];      /* position PID gains                     (controller.py:38-42)   */
  double kp_att[3], kd_att[3];                 /* attitude PD gains                      (:45-47)                */
  double inertia[3];                           /* diagonal inertia, kg m^2               (:49)                   */
  double max_torque_xyz[3];                    /* per-axis torque limits, N m            (:51)                   */
  double max_integral_per_axis[3];             /* per-axis integral limits               (:68)                   */
  double max_integral_pos;                     /* norm limit of the integral             (:56)                   */
  double max_tilt_angle;                       /* rad                                    (:57)                   */
  double mass, gravity;                        /* (:59-60)                                                       */
  double max_thrust, min_thrust;               /* N; lower limit = min_thrust*mass*gravity (:61-62, :469)        */
  double tracking_error_threshold, velocity_error_threshold;   /* (:64-65, _check_tracking_performance :650-658) */
  double back_calculation_gain;                /* Kb                                     (:69)                   */
  double integral_decay_factor;                /* (:70)                                                          */
  double saturation_threshold;                 /* (:71)                                                          */
  double yaw_singularity_threshold;            /* |yaw_vector . b3| at or above which yaw is singular (:73)      */
  double default_heading_yaw;                  /* rad, for yaw_fallback_method 1         (:75)                   */
  int32_t anti_windup_method;                  /* 0 "clamping", 1 "back_calculation", 2 none of them (:67)       */
  int32_t yaw_fallback_method;                 /* 0 "skip_yaw", 1 "default_heading", 2 "maintain_current", 3 any other string (:74) */
} se3mpc_controller_params;

/* DroneSimulator.__init__ (simulator.py:41-50). */
typedef struct se3mpc_simulator_params {
  double mass, gravity, inertia[3], max_thrust, max_torque;
} se3mpc_simulator_params;

/* Mutable controller members (controller.py:87-105), SE3MPC_CONTROLLER_STATE_WORDS doubles per drone:
 * [0..2] integral_vel_error, [3] last_time (NaN = None), [4] last_valid_thrust, [5] unsaturated_thrust, [6..8] unsaturated_torque,
 * [9] failsafe_count, [10] number of failsafe gain halvings (:817-821), [11] bit set: 1 failsafe_active, 2 last_thrust_saturated,
 * 4 / 8 / 16 last_torque_saturated x / y / z. */
#define SE3MPC_CONTROLLER_STATE_WORDS 12

int se3mpc_controller_default_params(se3mpc_controller_params* out);
int se3mpc_simulator_default_params(se3mpc_simulator_params* out);
/* GeometricController.__init__ / reset() (controller.py:87-105, :840-860) for B drones: state = device double[B][12]. */
int se3mpc_controller_reset(const se3mpc_controller_params* cp, int B, double* state, void* stream);

/* compute_control (controller.py:413-512) and, when body_thrust / body_rates are given, compute_body_rate_command (:706-726) for B
 * drones: desired position / velocity / acceleration dpos, dvel, dacc [B][3] (dacc NULL = 0), yaw, yaw_rate [B] (NULL = 0).
 * Outputs (any may be NULL): thrust [B], torque [B][3], body_thrust [B] (normalised), body_rates [B][3], flags int32 [B] (bit 0
 * failsafe command returned, 1 invalid dt, 2 thrust saturated, 3 yaw singularity, 4 tilt limited, 5..7 torque saturated x/y/z).
 * `state` is read and updated. */
int se3mpc_control_f32(const se3mpc_controller_params* cp, int B, const double* time, const float* pos, const float* vel,
                       const float* att, const float* omega, const float* dpos, const float* dvel, const float* dacc,
                       const float* yaw, const float* yaw_rate, double* state, float* thrust, float* torque, float* body_thrust,
                       float* body_rates, int32_t* flags, void* stream);
int se3mpc_control_f64(const se3mpc_controller_params* cp, int B, const double* time, const double* pos, const double* vel,
                       const double* att, const double* omega, const double* dpos, const double* dvel, const double* dacc,
                       const double* yaw, const double* yaw_rate, double* state, double* thrust, double* torque, double* body_thrust,
                       double* body_rates, int32_t* flags, void* stream);

/* compute_control_fast / compute_control_from_fast_state (controller.py:253-411, :728-768), the unit-free path of the reference's
 * 400 Hz hardware loop (hardware/pixhawk_interface.py:401), for B drones: dt (seconds) is an argument; an invalid one (dt <= 0 or
 * dt > 0.1) returns vehicle_mass * vehicle_gravity and zero torque and changes nothing (flag bit 1; no failsafe).  Gravity and the
 * lower thrust limit (min_thrust * vehicle_mass * vehicle_gravity) come from the vehicle constants (common/vehicle_params.py:19-23:
 * 1.0 kg, 9.80665 m/s^2), not from cp->mass / cp->gravity.  Same `state` record as se3mpc_control_* (the two paths share integral,
 * halved gains and saturation flags); last_time, last_valid_thrust, failsafe_active and failsafe_count are not written.  flags as
 * se3mpc_control_* (bits 2, 5..7 are what the reference adds to its _thrust_saturation_count / _torque_saturation_count). */
int se3mpc_control_fast_f32(const se3mpc_controller_params* cp, double vehicle_mass, double vehicle_gravity, int B, double dt,
                            const float* pos, const float* vel, const float* att, const float* omega, const float* dpos,
                            const float* dvel, const float* dacc, const float* yaw, const float* yaw_rate, double* state, float* thrust,
                            float* torque, int32_t* flags, void* stream);
int se3mpc_control_fast_f64(const se3mpc_controller_params* cp, double vehicle_mass, double vehicle_gravity, int B, double dt,
                            const double* pos, const double* vel, const double* att, const double* omega, const double* dpos,
                            const double* dvel, const double* dacc, const double* yaw, const double* yaw_rate, double* state,
                            double* thrust, double* torque, int32_t* flags, void* stream);

/* The controller's building blocks, as the reference's own controller tests call them (tests/control/
 * test_geometric_controller_anti_windup.py, test_geometric_controller_yaw_singularity.py, tests/test_controller_torque_calculation.py),
 * for B drones on the same `state` record:
 *  - integral_update = _update_integral_error(vel_error, dt, thrust_saturated, torque_saturated) (controller.py:536-564) with its
 *    anti-windup method and _clamp_integral_per_axis: vel_error [B][3]; saturation int32 [B] (bit 0 thrust, bits 1..3 torque x/y/z;
 *    NULL = none); the unsaturated thrust / torques of the back-calculation are read from the record;
 *  - attitude_torque = _geometric_attitude_control / _fast_geometric_attitude_control(att, ang_vel, b3_des, yaw_des, yaw_rate_des)
 *    (:643-704, :348-411): torque [B][3], flags as se3mpc_control_* (bits 3, 5..7); writes the record's unsaturated torques and torque
 *    saturation flags.  inertia: NULL = diag(cp->inertia), or host double[9] row-major (the tests assign a full matrix to _fast_inertia);
 *  - desired_frame = _detect_yaw_singularity(yaw_vector, b3_des) (:160-189) -> cos_angle [B], singular int32 [B], and frame [B][9] =
 *    (b1, b2, b3): method < 0 what _geometric_attitude_control builds (cp's fallback only when singular); method 0..3 =
 *    _handle_yaw_singularity(yaw_vector, b3_des, current_yaw, method) (:191-252) unconditionally.  Any output may be NULL. */
int se3mpc_controller_integral_update_f32(const se3mpc_controller_params* cp, int B, const float* vel_error, double dt,
                                          const int32_t* saturation, double* state, void* stream);
int se3mpc_controller_integral_update_f64(const se3mpc_controller_params* cp, int B, const double* vel_error, double dt,
                                          const int32_t* saturation, double* state, void* stream);
int se3mpc_controller_attitude_torque_f32(const se3mpc_controller_params* cp, int B, const float* att, const float* omega,
                                          const float* b3_des, const float* yaw, const float* yaw_rate, const double* inertia,
                                          double* state, float* torque, int32_t* flags, void* stream);
int se3mpc_controller_attitude_torque_f64(const se3mpc_controller_params* cp, int B, const double* att, const double* omega,
                                          const double* b3_des, const double* yaw, const double* yaw_rate, const double* inertia,
                                          double* state, double* torque, int32_t* flags, void* stream);
int se3mpc_controller_desired_frame_f32(const se3mpc_controller_params* cp, int B, int method, const float* yaw_vector,
                                        const float* b3_des, const float* current_yaw, float* frame, float* cos_angle,
                                        int32_t* singular, void* stream);
int se3mpc_controller_desired_frame_f64(const se3mpc_controller_params* cp, int B, int method, const double* yaw_vector,
                                        const double* b3_des, const double* current_yaw, double* frame, double* cos_angle,
                                        int32_t* singular, void* stream);

/* compute_control_from_trajectory(state, trajectory, t) / compute_body_rate_from_trajectory -- stubs in the reference
 * (controller.py:873-875; the second does not exist), the glue its contract test calls: target = the plan sampled at sample_time[b]
 * with OnboardController._interpolate_trajectory (onboard.py:43-93), then compute_control(state, target, yaw 0, yaw rate 0).
 * Plans as in se3mpc_closed_loop_*.  target: NULL or [B][9] = the sampled (position, velocity, acceleration). */
int se3mpc_control_plan_f32(const se3mpc_controller_params* cp, int B, const double* time, const double* sample_time, const float* pos,
                            const float* vel, const float* att, const float* omega, int N, const double* timestamps, long long ts_stride,
                            const float* P, long long strideP, const float* V, long long strideV, const float* A, long long strideA,
                            double* state, float* thrust, float* torque, float* body_thrust, float* body_rates, int32_t* flags,
                            float* target, void* stream);
int se3mpc_control_plan_f64(const se3mpc_controller_params* cp, int B, const double* time, const double* sample_time, const double* pos,
                            const double* vel, const double* att, const double* omega, int N, const double* timestamps, long long ts_stride,
                            const double* P, long long strideP, const double* V, long long strideV, const double* A, long long strideA,
                            double* state, double* thrust, double* torque, double* body_thrust, double* body_rates, int32_t* flags,
                            double* target, void* stream);

/* DroneSimulator.step (simulator.py:52-72) for B drones with given commands: thrust [B] (newtons), torque [B][3]; wind as in
 * se3mpc_closed_loop_*; time, pos, vel, att, omega are advanced in place by dt. */
int se3mpc_simulator_step_f32(const se3mpc_simulator_params* sp, int B, double dt, const float* thrust, const float* torque,
                              const float* wind, long long wind_stride, double* time, float* pos, float* vel, float* att,
                              float* omega, void* stream);
int se3mpc_simulator_step_f64(const se3mpc_simulator_params* sp, int B, double dt, const double* thrust, const double* torque,
                              const double* wind, long long wind_stride, double* time, double* pos, double* vel, double* att,
                              double* omega, void* stream);

/* The closed loop of the reference's contract tests (tests/test_planner_controller_contract.py:115-162, :255-316), `nsteps` times per
 * drone in ONE launch:  t = state.timestamp;  [stop_at_plan_end: a drone whose t > timestamps[N-1] stops for good (`break`)];
 * target = plan sampled at t (onboard.py:43-93);  cmd = compute_control(state, target, yaw 0);  [step == gust_step: the wind becomes
 * gust_wind, host double[3]];  state = DroneSimulator.step(state, cmd, sim_dt) (simulator.py:52-72).
 * Plan of drone b: timestamps + b*ts_stride (double [N]), P + b*strideP, V + b*strideV, A + b*strideA ([N][3] rows; V, A may be
 * NULL = zeros; stride 0 = one plan shared by all drones; strideP = strideV = 9N on X / X + 3N and strideA = 3N on `acc` read the
 * outputs of se3mpc_solve_* in place).  wind: NULL, or newtons at wind + b*wind_stride (stride 0 = one vector).
 * time, pos, vel, att, omega, state are updated in place.  Logs (any may be NULL): log_state [nsteps][B][12] = (pos, vel, att, omega)
 * BEFORE each step, log_cmd [nsteps][B][4] = (thrust, torque) (NaN for a stopped drone), log_time double [nsteps][B],
 * steps_taken int32 [B]. */
int se3mpc_closed_loop_f32(const se3mpc_controller_params* cp, const se3mpc_simulator_params* sp, int B, int nsteps, double sim_dt,
                           int N, const double* timestamps, long long ts_stride, const float* P, long long strideP, const float* V,
                           long long strideV, const float* A, long long strideA, double* time, float* pos, float* vel, float* att,
                           float* omega, double* state, const float* wind, long long wind_stride, int gust_step,
                           const double* gust_wind, int stop_at_plan_end, float* log_state, float* log_cmd, double* log_time,
                           int32_t* steps_taken, void* stream);
int se3mpc_closed_loop_f64(const se3mpc_controller_params* cp, const se3mpc_simulator_params* sp, int B, int nsteps, double sim_dt,
                           int N, const double* timestamps, long long ts_stride, const double* P, long long strideP, const double* V,
                           long long strideV, const double* A, long long strideA, double* time, double* pos, double* vel, double* att,
                           double* omega, double* state, const double* wind, long long wind_stride, int gust_step,
                           const double* gust_wind, int stop_at_plan_end, double* log_state, double* log_cmd, double* log_time,
                           int32_t* steps_taken, void* stream);

/* ------------------------------------------------------------------ TrajectorySmoother
 * The stage of the reference's edge loop between planner and controller (edge/main_improved.py:96-152; "smoother.py" =
 * src/dart_planner/control/trajectory_smoother.py), one drone per lane, reproduced with its quirks: its own plan sampler (:215-278:
 * stamps relative to timestamps[0], blend (1 - alpha) * row[i] + alpha * row[i + 1], an empty plan samples as zeros), the minimum-jerk
 * transition (:280-319), the per-call limits (:64-92), the exponential filter that a filtered position at the exact origin bypasses
 * (:94-113) and the decaying-velocity hover after `timeout` seconds without a plan (:321-338).  All clock arithmetic is double. */

/* The class's constants (smoother.py:19-26, :151, :176-179, :101, :329-331). */
typedef struct se3mpc_smoother_params {
  double transition_time;                      /* s, > 0                                 (:19)                   */
  double velocity_limit, acceleration_limit, jerk_limit;   /* (:24-26)                                           */
  double update_dt;                            /* the fixed dt of get_desired_state, > 0 (:179)                  */
  double smoothing_window;                     /* alpha = min(1, update_dt / window), > 0 (:101)                 */
  double pos_diff_threshold, vel_diff_threshold;   /* a new plan further away starts a transition (:151)         */
  double timeout;                              /* s without a plan before the failsafe   (:176, :331)            */
  double decay_rate, decay_cap;                /* failsafe velocity decay, 1/s and s     (:329-331)              */
} se3mpc_smoother_params;

/* Mutable smoother members (smoother.py:28-46), SE3MPC_SMOOTHER_STATE_WORDS doubles per drone: [0..8] last_filtered_pos, _vel, _acc;
 * [9..20] transition_start_pos, transition_start_vel, transition_target_pos, transition_target_vel; [21] transition_start_time;
 * [22] last_cloud_update; [23] trajectory_start_time; [24] bit set: 1 current_trajectory is not None, 2 in_transition.
 * The plan itself (current_trajectory) stays the caller's and is passed per call. */
#define SE3MPC_SMOOTHER_STATE_WORDS 25

int se3mpc_smoother_default_params(se3mpc_smoother_params* out);
/* TrajectorySmoother.__init__ (smoother.py:28-46) for B drones: state = device double[B][25], all zero (no trajectory). */
int se3mpc_smoother_reset(int B, double* state, void* stream);

/* update_trajectory (smoother.py:115-165) for B drones at the clocks now [B] (where the reference reads time.time()).  Plans as in
 * se3mpc_closed_loop_* (timestamps, P, V, A and their strides; V, A may be NULL = zeros), N_old / N_new >= 0 rows (0 = an empty plan,
 * which samples as zeros; its pointers are not read).  The old plan is read only for drones that have a trajectory and may be NULL
 * when none does (a drone that has one then samples zeros).  `state` is read and updated.
 * Argument rules of the four entry points: a NULL required operand: SE3MPC_ERR_NULL; B < 0, nsteps < 0, a negative N or stride, N >
 * 4096: SE3MPC_ERR_SHAPE; transition_time / update_dt / smoothing_window not finite or not positive, non-finite sim_dt:
 * SE3MPC_ERR_PARAM (a limit or threshold may be infinite: it then never fires).  B = 0 and nsteps = 0 are no-ops.  Every rejected call sets se3mpc_last_error and launches nothing. */
int se3mpc_smoother_update_f32(const se3mpc_smoother_params* mp, int B, const double* now, int N_old, const double* ts_old,
                               long long ts_old_stride, const float* P_old, long long strideP_old, const float* V_old,
                               long long strideV_old, const float* A_old, long long strideA_old, int N_new, const double* ts_new,
                               long long ts_new_stride, const float* P_new, long long strideP_new, const float* V_new,
                               long long strideV_new, const float* A_new, long long strideA_new, double* state, void* stream);
int se3mpc_smoother_update_f64(const se3mpc_smoother_params* mp, int B, const double* now, int N_old, const double* ts_old,
                               long long ts_old_stride, const double* P_old, long long strideP_old, const double* V_old,
                               long long strideV_old, const double* A_old, long long strideA_old, int N_new, const double* ts_new,
                               long long ts_new_stride, const double* P_new, long long strideP_new, const double* V_new,
                               long long strideV_new, const double* A_new, long long strideA_new, double* state, void* stream);

/* get_desired_state (smoother.py:167-213) for B drones at the clocks now [B]: pos, vel [B][3] = the drone's own state (the failsafe
 * and the no-trajectory hover return it), the current plan of N >= 0 rows.  Outputs (any may be NULL): target [B][9] = (position,
 * velocity, acceleration), branch int32 [B]: 0 failsafe, 1 transition point, 2 transition just completed (then normal following),
 * 3 normal following, 4 no trajectory.  `state` is read and updated. */
int se3mpc_smoother_desired_f32(const se3mpc_smoother_params* mp, int B, const double* now, const float* pos, const float* vel, int N,
                                const double* timestamps, long long ts_stride, const float* P, long long strideP, const float* V,
                                long long strideV, const float* A, long long strideA, double* state, float* target, int32_t* branch,
                                void* stream);
int se3mpc_smoother_desired_f64(const se3mpc_smoother_params* mp, int B, const double* now, const double* pos, const double* vel, int N,
                                const double* timestamps, long long ts_stride, const double* P, long long strideP, const double* V,
                                long long strideV, const double* A, long long strideA, double* state, double* target, int32_t* branch,
                                void* stream);

/* The control-rate part of the reference's edge loop between two plans (edge/main_improved.py:125-152), `nsteps` times per drone in ONE
 * launch:  t = state.timestamp;  target = get_desired_state(t, state);  cmd = compute_control(state, target, yaw 0);  [step ==
 * gust_step: the wind becomes gust_wind];  state = DroneSimulator.step(state, cmd, sim_dt).  Arguments as se3mpc_closed_loop_* (no
 * stop_at_plan_end: the smoother holds the plan's last row, and no steps_taken: every drone takes nsteps), plus the smoother's
 * parameters, its records smoother_state [B][25] (in / out) and log_target [nsteps][B][9] (NULL or the targets handed to the
 * controller).  The same bits as nsteps chained se3mpc_smoother_desired_* -> se3mpc_control_* -> se3mpc_simulator_step_* launches. */
int se3mpc_closed_loop_smoothed_f32(const se3mpc_smoother_params* mp, const se3mpc_controller_params* cp,
                                    const se3mpc_simulator_params* sp, int B, int nsteps, double sim_dt, int N, const double* timestamps,
                                    long long ts_stride, const float* P, long long strideP, const float* V, long long strideV,
                                    const float* A, long long strideA, double* time, float* pos, float* vel, float* att, float* omega,
                                    double* state, double* smoother_state, const float* wind, long long wind_stride, int gust_step,
                                    const double* gust_wind, float* log_state, float* log_cmd, double* log_time, float* log_target,
                                    void* stream);
int se3mpc_closed_loop_smoothed_f64(const se3mpc_smoother_params* mp, const se3mpc_controller_params* cp,
                                    const se3mpc_simulator_params* sp, int B, int nsteps, double sim_dt, int N, const double* timestamps,
                                    long long ts_stride, const double* P, long long strideP, const double* V, long long strideV,
                                    const double* A, long long strideA, double* time, double* pos, double* vel, double* att,
                                    double* omega, double* state, double* smoother_state, const double* wind, long long wind_stride,
                                    int gust_step, const double* gust_wind, double* log_state, double* log_cmd, double* log_time,
                                    double* log_target, void* stream);

/* ------------------------------------------------------------------ MotorMixer and motor model
 * The last arithmetic stage between the controller's (thrust, torque) and the actuators in both hardware back ends of the reference
 * (hardware/pixhawk_interface.py:451-492, hardware/airsim_interface.py:157-191; "mixer.py" = src/dart_planner/hardware/motor_mixer.py,
 * "model.py" = src/dart_planner/hardware/motor_model.py), one drone per lane, reproduced with its quirks: a motor thrust below the
 * thrust curve's minimum asks for FULL PWM (model.py:250-252), the model clips to the MOTOR's limits before the mixer clips to the
 * CONFIG's, so the saturation counter (mixer.py:213, np.allclose with rtol 1e-6) sees only what the second clip and the idle floor
 * move, and get_control_allocation applies the INVERSE matrix to the motor thrusts (mixer.py:279). */

/* MotorMixer.mixing_matrix / inverse_matrix (mixer.py:379-398, :152-166), the QuadraticMotorModel's MotorParameters of motors 0..3
 * (model.py:33-48), MotorMixingConfig's PWM limits (mixer.py:64-66) and the constants of the Pixhawk loop.  All doubles. */
typedef struct se3mpc_mixer_params {
  double inverse[16];                          /* inverse_matrix, row-major: motor thrusts = inverse @ (T, tx, ty, tz)  (mixer.py:195) */
  double mixing[16];                           /* B, row-major: (T, tx, ty, tz) = B @ motor thrusts; column i = (1, y_i, x_i, direction_i * k_drag_i) */
  double thrust_a[4], thrust_b[4], thrust_c[4];   /* thrust = a pwm^2 + b pwm + c, newtons        (model.py:34-36) */
  double pwm_min[4], pwm_max[4], pwm_idle[4];  /* each MOTOR's limits                             (model.py:46-48) */
  double torque_coefficient[4];                /* torque = kQ rpm^2                               (model.py:39)    */
  double rpm_coefficient[4], rpm_offset[4];    /* rpm = k pwm + offset                            (model.py:42-43) */
  double config_pwm_min, config_pwm_max, config_pwm_idle;   /* the CONFIG's limits                (mixer.py:64-66) */
  double max_thrust;                           /* normalised thrust = clip(thrust / max_thrust, 0, 1)   (pixhawk_interface.py:473) */
  double body_rate_scale;                      /* rad/s per PWM unit                              (pixhawk_interface.py:482) */
  double watchdog_threshold;                   /* saturation_events > this trips the watchdog     (pixhawk_interface.py:413) */
} se3mpc_mixer_params;

/* Mutable mixer members (mixer.py:144-145), SE3MPC_MIXER_STATE_WORDS doubles per drone: [0] saturation_events, [1..4]
 * last_motor_commands. */
#define SE3MPC_MIXER_STATE_WORDS 5

/* Flag bits of se3mpc_mixer_mix_*: negative thrust clamped to 0 (mixer.py:187-189); a non-finite motor thrust (:198-199, the
 * reference raises RuntimeError); a raw PWM above 1.1 * config_pwm_max (:205-206); saturation_events was incremented (:213-214); all
 * motors at the config's idle although thrust > 0.2 (:218); saturation_events > watchdog_threshold after this call. */
#define SE3MPC_MIXER_NEGATIVE_THRUST 1
#define SE3MPC_MIXER_NON_FINITE 2
#define SE3MPC_MIXER_OVERRUN 4
#define SE3MPC_MIXER_SATURATION_EVENT 8
#define SE3MPC_MIXER_ALL_IDLE 16
#define SE3MPC_MIXER_WATCHDOG 32

/* create_x_configuration_mixer(0.15) (mixer.py:401-423) with create_default_motor_model() (model.py:386-437) and the Pixhawk constants
 * (max_thrust 10, rate scale 2, watchdog 5): B as mixer.py:379-398, its inverse by LU with partial pivoting on the host. */
int se3mpc_mixer_default_params(se3mpc_mixer_params* out);
/* MotorMixer.__init__ (mixer.py:144-145) for B drones: state = device double[B][5], all zero. */
int se3mpc_mixer_reset(int B, double* state, void* stream);

/* mix_commands (mixer.py:168-222, with _thrust_to_pwm :224-242, pwm_from_thrust model.py:219-258 and _saturate_pwm :244-260) for B
 * drones: thrust [B] newtons, torque [B][3] -> pwm [B][4].  state: NULL or the records [B][5], read and updated (a drone with the
 * non-finite flag gets NaN PWMs and its record is left as it is).  flags: NULL or int32 [B], the bits above (the watchdog bit needs
 * `state`).  body_rate: NULL or [B][4] = _convert_to_body_rate_cmd (pixhawk_interface.py:473-487): (normalised thrust, roll, pitch,
 * yaw rate).
 * Argument rules of the mixer's entry points: NULL parameters or a NULL required operand: SE3MPC_ERR_NULL; B < 0, nsteps < 0, a
 * negative stride, a plan se3mpc_closed_loop_smoothed_* rejects: SE3MPC_ERR_SHAPE; a non-finite field outside the two matrices
 * (which may hold whatever the host's linear algebra gave for a singular B), non-finite sim_dt: SE3MPC_ERR_PARAM.  B = 0 and nsteps = 0 are no-ops.  Every rejected
 * call sets se3mpc_last_error and launches nothing. */
int se3mpc_mixer_mix_f32(const se3mpc_mixer_params* mp, int B, const float* thrust, const float* torque, double* state, float* pwm,
                         int32_t* flags, float* body_rate, void* stream);
int se3mpc_mixer_mix_f64(const se3mpc_mixer_params* mp, int B, const double* thrust, const double* torque, double* state, double* pwm,
                         int32_t* flags, double* body_rate, void* stream);

/* What the motors do under pwm [B][4] (any output may be NULL, each [B][4]): motor_thrust = thrust_from_pwm (model.py:166-190) times
 * the motor's health, motor_torque = torque_from_pwm (:192-217), motor_rpm = rpm_from_pwm (:260-282), allocation =
 * get_control_allocation (mixer.py:262-279: the INVERSE matrix on the motor thrusts, as the reference has it), wrench = B @ motor
 * thrusts = the (thrust, torque) the vehicle receives -- the reference never forms it; a simulator behind the mixer needs it.
 * motor_health: NULL (= 1) or rows of 4 factors at motor_health + b * health_stride (stride 0 = one row for all drones): the
 * fault-injection operand; the mixer does not see it. */
int se3mpc_mixer_readback_f32(const se3mpc_mixer_params* mp, int B, const float* pwm, const float* motor_health, long long health_stride,
                              float* motor_thrust, float* motor_torque, float* motor_rpm, float* allocation, float* wrench,
                              void* stream);
int se3mpc_mixer_readback_f64(const se3mpc_mixer_params* mp, int B, const double* pwm, const double* motor_health,
                              long long health_stride, double* motor_thrust, double* motor_torque, double* motor_rpm, double* allocation,
                              double* wrench, void* stream);

/* se3mpc_closed_loop_smoothed_* with the actuators behind the controller, `nsteps` times per drone in ONE launch:  target =
 * get_desired_state(t, state) -- or, with smp and smoother_state BOTH NULL, the raw plan sample of se3mpc_closed_loop_* (then N >= 1);
 * one of the two alone is SE3MPC_ERR_NULL --;  cmd = compute_control(state, target, yaw 0);  pwm = mix_commands(cmd);  wrench = B @
 * (motor_health * thrust_from_pwm(pwm));  state = DroneSimulator.step(state, wrench, sim_dt).  mixer_state [B][5] in / out;
 * motor_health, health_stride as se3mpc_mixer_readback_*.  log_cmd keeps the COMMANDED (thrust, torque); log_pwm, log_wrench
 * [nsteps][B][4]: NULL or the PWMs and the realised (thrust, torque); log_target as se3mpc_closed_loop_smoothed_* in both forms.  The same
 * bits as nsteps chained (se3mpc_smoother_desired_* + se3mpc_control_*, or se3mpc_control_plan_*) -> se3mpc_mixer_mix_* ->
 * se3mpc_mixer_readback_* -> se3mpc_simulator_step_* launches. */
int se3mpc_closed_loop_actuated_f32(const se3mpc_smoother_params* smp, const se3mpc_controller_params* cp,
                                    const se3mpc_simulator_params* sp, const se3mpc_mixer_params* mp, int B, int nsteps, double sim_dt,
                                    int N, const double* timestamps, long long ts_stride, const float* P, long long strideP,
                                    const float* V, long long strideV, const float* A, long long strideA, double* time, float* pos,
                                    float* vel, float* att, float* omega, double* state, double* smoother_state, double* mixer_state,
                                    const float* motor_health, long long health_stride, const float* wind, long long wind_stride,
                                    int gust_step, const double* gust_wind, float* log_state, float* log_cmd, double* log_time,
                                    float* log_target, float* log_pwm, float* log_wrench, void* stream);
int se3mpc_closed_loop_actuated_f64(const se3mpc_smoother_params* smp, const se3mpc_controller_params* cp,
                                    const se3mpc_simulator_params* sp, const se3mpc_mixer_params* mp, int B, int nsteps, double sim_dt,
                                    int N, const double* timestamps, long long ts_stride, const double* P, long long strideP,
                                    const double* V, long long strideV, const double* A, long long strideA, double* time, double* pos,
                                    double* vel, double* att, double* omega, double* state, double* smoother_state, double* mixer_state,
                                    const double* motor_health, long long health_stride, const double* wind, long long wind_stride,
                                    int gust_step, const double* gust_wind, double* log_state, double* log_cmd, double* log_time,
                                    double* log_target, double* log_pwm, double* log_wrench, void* stream);

/* The receding-horizon closed-loop Monte-Carlo of BASELINE config 5's named test shape (tests/test_monte_carlo_sim.py:24-72) in ONE
 * launch: for each of B drones, `cycles` times { se3mpc_solve_* from the drone's own (pos, vel) with the reference's cold start;
 * `substeps` x se3mpc_closed_loop_*'s step (plan sample -> compute_control -> DroneSimulator.step at sim_dt) against the fresh plan,
 * whose row k is stamped (cycle * substeps * sim_dt) + k * params->dt }.  The same code as the two entry points it fuses, hence the
 * same bits as alternating them (dart_planner_amd/control/closed_loop.py) -- without 2 x cycles kernel boundaries at each of which every
 * drone waits for the slowest one.  goal [B][3]; wind NULL or rows of wind_stride (0 = one shared row); time [B], pos / vel / att /
 * omega [B][3], state [B][SE3MPC_CONTROLLER_STATE_WORDS]: in / out as se3mpc_closed_loop_*; X_last [B][9N], acc_last [B][3N],
 * info_last [B] (each may be NULL): the last cycle's plan; overflowed: device int32, set to the number of solves that needed more
 * L-BFGS pairs than this launch's LDS image holds (never with the reference's options) -- when it is not 0 the run must be repeated
 * with the two-launch form. */
int se3mpc_monte_carlo_f32(const se3mpc_params* p, const se3mpc_controller_params* cp, const se3mpc_simulator_params* sp, int B, int cycles,
                           int substeps, double sim_dt, const float* goal, const float* wind, long long wind_stride, double* time,
                           float* pos, float* vel, float* att, float* omega, double* state, float* X_last, float* acc_last,
                           se3mpc_solve_info* info_last, int32_t* overflowed, void* stream);
int se3mpc_monte_carlo_f64(const se3mpc_params* p, const se3mpc_controller_params* cp, const se3mpc_simulator_params* sp, int B, int cycles,
                           int substeps, double sim_dt, const double* goal, const double* wind, long long wind_stride, double* time,
                           double* pos, double* vel, double* att, double* omega, double* state, double* X_last, double* acc_last,
                           se3mpc_solve_info* info_last, int32_t* overflowed, void* stream);

/* se3mpc_monte_carlo_* with the reference's full edge loop per drone (edge/main_improved.py:96-152: plan -> TrajectorySmoother ->
 * GeometricController -> MotorMixer and motors -> DroneSimulator), still in ONE launch: for each of B drones, `cycles` times { se3mpc_solve_*
 * from the drone's own (pos, vel); with smp, se3mpc_smoother_update_* at the drone's clock against the plan of the cycle before (none in the
 * first cycle, also for a record that says it has a trajectory: as old = NULL there); `substeps` x the step of
 * se3mpc_closed_loop_actuated_* (with mp: desired state or raw plan sample -> compute_control -> mix_commands -> the motors' wrench under
 * motor_health -> DroneSimulator.step) or of se3mpc_closed_loop_smoothed_* (without mp) }.  The same code as the entry points it fuses, hence
 * the same bits as launching them in turn (dart_planner_amd/control/closed_loop.py, run with smoother= / mixer=).  Arguments as
 * se3mpc_monte_carlo_*, and: smp, mp: each may be NULL = the stage is absent (both NULL: this IS se3mpc_monte_carlo_*); smoother_state
 * [B][SE3MPC_SMOOTHER_STATE_WORDS], mixer_state [B][SE3MPC_MIXER_STATE_WORDS]: in / out; motor_health NULL (exactly 1) or rows of
 * health_stride (0 = one shared row) of four factors on the motors' thrusts, as se3mpc_closed_loop_actuated_*.  The plan being followed
 * does not leave the chip: a run cannot be continued by a second call.
 * Argument rules, before the B == 0 no-op: everything se3mpc_monte_carlo_* rejects, with the same codes; smp and smoother_state come
 * together, mp and mixer_state come together, motor_health needs mp (SE3MPC_ERR_NULL); health_stride < 0 (SE3MPC_ERR_SHAPE); smoother /
 * mixer parameters that se3mpc_smoother_update_* / se3mpc_mixer_mix_* reject (SE3MPC_ERR_PARAM). */
int se3mpc_monte_carlo_staged_f32(const se3mpc_params* p, const se3mpc_controller_params* cp, const se3mpc_simulator_params* sp,
                                  const se3mpc_smoother_params* smp, const se3mpc_mixer_params* mp, int B, int cycles, int substeps,
                                  double sim_dt, const float* goal, const float* wind, long long wind_stride, double* time, float* pos,
                                  float* vel, float* att, float* omega, double* state, double* smoother_state, double* mixer_state,
                                  const float* motor_health, long long health_stride, float* X_last, float* acc_last,
                                  se3mpc_solve_info* info_last, int32_t* overflowed, void* stream);
int se3mpc_monte_carlo_staged_f64(const se3mpc_params* p, const se3mpc_controller_params* cp, const se3mpc_simulator_params* sp,
                                  const se3mpc_smoother_params* smp, const se3mpc_mixer_params* mp, int B, int cycles, int substeps,
                                  double sim_dt, const double* goal, const double* wind, long long wind_stride, double* time, double* pos,
                                  double* vel, double* att, double* omega, double* state, double* smoother_state, double* mixer_state,
                                  const double* motor_health, long long health_stride, double* X_last, double* acc_last,
                                  se3mpc_solve_info* info_last, int32_t* overflowed, void* stream);

/* The receding-horizon closed-loop Monte-Carlo with se3mpc_mppi_* as its planner, in ONE launch (one workgroup of min(S, 256) lanes per
 * drone; no atomics, no workspace, no allocation, no synchronise).  Everything is in problem layout: goal [B][3] (input); time [B],
 * pos / vel / att / omega [B][3], state [B][SE3MPC_CONTROLLER_STATE_WORDS]: in / out as se3mpc_monte_carlo_*; wind, wind_stride as
 * se3mpc_monte_carlo_*; spheres [K][4] rows (cx, cy, cz, r) shared by all drones as se3mpc_mppi_*; U [B][N][3]: in / out, each drone's
 * nominal thrust sequence.  Cycle c = 0 .. cycles - 1 of drone b, with C = cycle_base + c and q = index_base + b:
 *   plan       `iters` iterations of se3mpc_mppi_* (same noise, clip, cost, sphere penalty and float64 update in the same order, hence the
 *              same bits) from the drone's current (pos, vel) on U, iteration number g = iter_base + C * iters + i (uint32 wrap);
 *              trace[b][c][i] = the minimum sample cost; in the last cycle cost[b] = the cost (with the penalty) of the updated U
 *   hand over  the updated U rolled out in the entry point's type: plan row k = the state BEFORE step k (row 0 = the drone's state),
 *              A_k = U_k / mass - (0, 0, g), stamped (C * substeps * sim_dt) + k * params->dt.  The plan stays on the chip; the last
 *              cycle's goes to plan_last [B][3][N][3] (P, V, A) when given
 *   act        `substeps` x the step of se3mpc_closed_loop_* (plan sample -> compute_control with yaw 0 -> DroneSimulator.step at
 *              sim_dt; no gust, no stop at the plan's end) -- the same code, hence the same bits
 *   clearance  (clearance != NULL and K > 0) after every simulator step clearance[b] = min(clearance[b], min_j(|pos - c_j| - r_j)),
 *              raw radii, no margin; the caller initialises the array (normally +inf)
 *   warm start U[k] <- U[k + shift] for k < N - shift, (0, 0, mass * gravity) for the rows behind; 0 <= shift <= N (0 keeps U, N resets it)
 * so U on return is the next cycle's starting nominal, and one call with cycles = C equals C calls with cycles = 1 and cycle_base =
 * 0 .. C - 1, bit for bit.  trace: NULL or [B][cycles][iters]; plan_last, clearance: NULL or as above.
 * Argument rules: everything se3mpc_mppi_* and se3mpc_monte_carlo_* reject, with the same codes (S a multiple of 64 in [64, 65536], K in
 * [0, SE3MPC_MAX_SPHERES]: SE3MPC_ERR_SHAPE; sigma >= 0, temperature > 0, obstacle_weight >= 0 and sim_dt finite: SE3MPC_ERR_PARAM);
 * shift outside [0, N], iters < 0, cycles < 0, substeps < 0, B < 0: SE3MPC_ERR_SHAPE; a NULL required operand: SE3MPC_ERR_NULL.  B = 0
 * and cycles = 0 are no-ops.  Every rejected call sets se3mpc_last_error and launches nothing. */
int se3mpc_mppi_closed_loop_f32(const se3mpc_params* p, const se3mpc_controller_params* cp, const se3mpc_simulator_params* sp, int B,
                                int cycles, int substeps, double sim_dt, uint32_t cycle_base, int shift, int S, int iters, double sigma,
                                double temperature, uint64_t seed, uint32_t iter_base, uint32_t index_base, const float* goal,
                                const float* spheres, int K, double obstacle_weight, const float* wind, long long wind_stride, double* time,
                                float* pos, float* vel, float* att, float* omega, double* state, float* U, float* cost, float* trace,
                                float* plan_last, float* clearance, void* stream);
int se3mpc_mppi_closed_loop_f64(const se3mpc_params* p, const se3mpc_controller_params* cp, const se3mpc_simulator_params* sp, int B,
                                int cycles, int substeps, double sim_dt, uint32_t cycle_base, int shift, int S, int iters, double sigma,
                                double temperature, uint64_t seed, uint32_t iter_base, uint32_t index_base, const double* goal,
                                const double* spheres, int K, double obstacle_weight, const double* wind, long long wind_stride, double* time,
                                double* pos, double* vel, double* att, double* omega, double* state, double* U, double* cost, double* trace,
                                double* plan_last, double* clearance, void* stream);

/* se3mpc_mppi_closed_loop_* around spheres that MOVE with constant velocity: the operands of se3mpc_mppi_closed_loop_*,
 * and after `spheres` the sphere_vel [K][3] and sphere_t0 of se3mpc_mppi_moving_*.  sphere_t0 is the time of the RUN's start (cycle 0,
 * simulator step 0) on the table's clock, the same in every chained call; the table advances with the run:
 *   plan       cycle C = cycle_base + c, step k:   tau_k = sphere_t0 + plan_stamp, plan_stamp = (double)(C * substeps) * sim_dt + (double)k * dt
 *              (the double the plan row's stamp is), the penalty then as in se3mpc_mppi_moving_*
 *   clearance  simulator step s (0-based) of cycle C: the position the step produced against the centres at
 *              tau = sphere_t0 + (double)(C * substeps + s + 1) * sim_dt; the form stays |pos - centre| - r with the raw radii
 * each tau rounded to the kernel's type (tR) and centre_a = c_a + v_a * tR, so the advice of se3mpc_mppi_moving_* on small times holds.
 * With sphere_vel = 0 every output equals se3mpc_mppi_closed_loop_*'s bit for bit.  Checks: those of se3mpc_mppi_closed_loop_*, then a
 * non-finite sphere_t0: SE3MPC_ERR_PARAM; sphere_vel NULL with K > 0: SE3MPC_ERR_NULL.  K = 0 is allowed and reads neither table.  There is
 * no staged or edge form. */
int se3mpc_mppi_closed_loop_moving_f32(const se3mpc_params* p, const se3mpc_controller_params* cp, const se3mpc_simulator_params* sp, int B,
                                       int cycles, int substeps, double sim_dt, uint32_t cycle_base, int shift, int S, int iters, double sigma,
                                       double temperature, uint64_t seed, uint32_t iter_base, uint32_t index_base, const float* goal,
                                       const float* spheres, const float* sphere_vel, double sphere_t0, int K, double obstacle_weight,
                                       const float* wind, long long wind_stride, double* time, float* pos, float* vel, float* att, float* omega,
                                       double* state, float* U, float* cost, float* trace, float* plan_last, float* clearance, void* stream);
int se3mpc_mppi_closed_loop_moving_f64(const se3mpc_params* p, const se3mpc_controller_params* cp, const se3mpc_simulator_params* sp, int B,
                                       int cycles, int substeps, double sim_dt, uint32_t cycle_base, int shift, int S, int iters, double sigma,
                                       double temperature, uint64_t seed, uint32_t iter_base, uint32_t index_base, const double* goal,
                                       const double* spheres, const double* sphere_vel, double sphere_t0, int K, double obstacle_weight,
                                       const double* wind, long long wind_stride, double* time, double* pos, double* vel, double* att,
                                       double* omega, double* state, double* U, double* cost, double* trace, double* plan_last,
                                       double* clearance, void* stream);

/* se3mpc_mppi_closed_loop_moving_* with the tracked spheres of se3mpc_mppi_tracks_* (DESIGN.md 5.8h): the operands of
 * se3mpc_mppi_closed_loop_moving_*, and after K: tracks, device [cycles][B][N][Kt][4] = (x, y, z, radius), and Kt.  Predictions are renewed
 * every cycle: cycle c of the CALL (0 <= c < cycles, whatever cycle_base is) of drone b plans around slab [c][b], whose row [k][j] is
 * sphere j at the time of the state before step k of that cycle's plan.  The in-flight clearance is measured against the K moving rows
 * only: a track is a prediction at plan steps, not a surface at simulator steps.  Kt = 0 gives se3mpc_mppi_closed_loop_moving_*'s
 * outputs bit for bit.  Checks: those of se3mpc_mppi_closed_loop_moving_*, then Kt outside [0, SE3MPC_MAX_TRACKS] or K + Kt >
 * SE3MPC_MAX_SPHERES: SE3MPC_ERR_SHAPE; tracks NULL with Kt > 0: SE3MPC_ERR_NULL. */
int se3mpc_mppi_closed_loop_tracks_f32(const se3mpc_params* p, const se3mpc_controller_params* cp, const se3mpc_simulator_params* sp, int B,
                                       int cycles, int substeps, double sim_dt, uint32_t cycle_base, int shift, int S, int iters, double sigma,
                                       double temperature, uint64_t seed, uint32_t iter_base, uint32_t index_base, const float* goal,
                                       const float* spheres, const float* sphere_vel, double sphere_t0, int K, const float* tracks, int Kt,
                                       double obstacle_weight, const float* wind, long long wind_stride, double* time, float* pos, float* vel,
                                       float* att, float* omega, double* state, float* U, float* cost, float* trace, float* plan_last,
                                       float* clearance, void* stream);
int se3mpc_mppi_closed_loop_tracks_f64(const se3mpc_params* p, const se3mpc_controller_params* cp, const se3mpc_simulator_params* sp, int B,
                                       int cycles, int substeps, double sim_dt, uint32_t cycle_base, int shift, int S, int iters, double sigma,
                                       double temperature, uint64_t seed, uint32_t iter_base, uint32_t index_base, const double* goal,
                                       const double* spheres, const double* sphere_vel, double sphere_t0, int K, const double* tracks, int Kt,
                                       double obstacle_weight, const double* wind, long long wind_stride, double* time, double* pos, double* vel,
                                       double* att, double* omega, double* state, double* U, double* cost, double* trace, double* plan_last,
                                       double* clearance, void* stream);

/* se3mpc_mppi_closed_loop_moving_* for SWARMS: the B drones of a call are B / swarm_size swarms of M = swarm_size drones
 * (drone b belongs to swarm b / M; its mates are the other drones of that swarm), and every drone plans around its nearest mates as
 * spheres of radius mate_radius that move with constant velocity.  The operands are those of se3mpc_mppi_closed_loop_moving_*, same
 * order and meaning, with K = the rows of the SHARED table (spheres, sphere_vel) every drone sees; in front of them swarm_size,
 * neighbours_k = Kn and mate_radius, behind them separation, neighbours and the workspace.  One planning cycle is one launch (one
 * workgroup of min(S, 256) lanes per drone), a call with cycles = C enqueues C + 1 launches on the stream (a seed and the cycles),
 * allocates nothing and synchronises nothing.  Cycle C = cycle_base + c of drone b:
 *   snapshot   (pos, vel) of every drone as they stand when the cycle starts ([B][6] in the workspace, written by the launch before)
 *   d2         for mate i of the drone, in float64 without contraction, summed left to right:  d2_i = dx*dx + dy*dy + dz*dz,
 *              dx = (double)snap_pos[i].x - (double)own.x and likewise y and z, own = the drone's own snapshot row
 *   eligible   a mate whose six snapshot values are finite; E = their number (E = 0 when the drone's own row is not finite)
 *   selection  the Kn_eff = min(Kn, E) eligible mates with the smallest (d2, drone index): equal d2 resolves to the lower index
 *   table      rows [0, K) the shared spheres; row K + r the mate a of rank r: velocity vel_a, radius mate_radius (so the penalty sees
 *              (mate_radius + margin)^2 by the expression of the shared rows), centre c'_a = pos_a - (vel_a * tR0), two roundings in the
 *              entry point's type without contraction, tR0 = (R)(sphere_t0 + (double)(C * substeps) * sim_dt): the time of the cycle's
 *              start on the table's clock, so centre = c' + v * tR_k puts the mate where it is at the cycle's start and extrapolates it
 *              along the horizon
 *   plan ... warm start   the cycle of se3mpc_mppi_closed_loop_moving_* on that table of K + Kn_eff rows; the in-flight clearance is
 *              measured against rows [0, K) only (the mates' extrapolated positions are predictions)
 * separation [B]: in / out, normally +inf: separation[b] = min(separation[b], (R)sqrt(min over the eligible mates of d2)) at every
 * cycle's start, on the snapshot: the true distance at the cycle boundaries; untouched when E = 0.  se3mpc_swarm_separation_* folds in
 * the same quantity of (pos, vel) as they stand (call it after the last cycle, so that the final positions count).  neighbours: NULL or
 * [B][Kn] int32: the drones chosen in the call's last cycle, as indices into the call's B drones in rank order, -1 in unused slots.
 * workspace: device memory of at least se3mpc_mppi_swarm_workspace_bytes(B, sizeof(R)) bytes = two [B][6] images, aligned to R; it
 * needs no initialisation and carries nothing from call to call.  Guarantees:
 *   reduces to the moving loop   with swarm_size = 1 or neighbours_k = 0 every output shared with se3mpc_mppi_closed_loop_moving_*
 *                                equals that entry point's, bit for bit
 *   continuation                 one call with cycles = C equals C calls with cycles = 1 and cycle_base = 0 .. C - 1, bit for bit,
 *                                separation and the neighbours of the last cycle included
 *   trace layout                 trace stays [B][cycles][iters]
 *   schedule independence        every workgroup reads one image of the snapshot and writes the other, the images swap between launches
 *                                and the kernel boundary is the only synchronisation (no atomics, no flags): results are identical run
 *                                to run and do not depend on how the device schedules workgroups
 * Argument rules: everything se3mpc_mppi_closed_loop_moving_* rejects, with the same codes; swarm_size outside [1, SE3MPC_MAX_SWARM],
 * B not a multiple of swarm_size, neighbours_k < 0, K + neighbours_k > SE3MPC_MAX_SPHERES, workspace_bytes too small (swarm_size > 1,
 * workspace given): SE3MPC_ERR_SHAPE; mate_radius negative or not finite: SE3MPC_ERR_PARAM; a NULL workspace or a NULL separation
 * when swarm_size > 1, neighbours_k > 0, B > 0 and cycles > 0: SE3MPC_ERR_NULL.  (With neighbours_k = 0 the snapshot serves the
 * separation alone: a NULL workspace or separation then leaves separation untouched.)  se3mpc_mppi_swarm_workspace_bytes returns 0
 * for arguments outside these rules (B < 0, elem_size not 4 or 8).  Every rejected call sets se3mpc_last_error and launches nothing.
 * There is no staged or edge form. */
size_t se3mpc_mppi_swarm_workspace_bytes(int B, int elem_size);
int se3mpc_mppi_closed_loop_swarm_f32(const se3mpc_params* p, const se3mpc_controller_params* cp, const se3mpc_simulator_params* sp, int B,
                                      int swarm_size, int neighbours_k, double mate_radius, int cycles, int substeps, double sim_dt,
                                      uint32_t cycle_base, int shift, int S, int iters, double sigma, double temperature, uint64_t seed,
                                      uint32_t iter_base, uint32_t index_base, const float* goal, const float* spheres, const float* sphere_vel,
                                      double sphere_t0, int K, double obstacle_weight, const float* wind, long long wind_stride, double* time,
                                      float* pos, float* vel, float* att, float* omega, double* state, float* U, float* cost, float* trace,
                                      float* plan_last, float* clearance, float* separation, int32_t* neighbours, void* workspace,
                                      size_t workspace_bytes, void* stream);
int se3mpc_mppi_closed_loop_swarm_f64(const se3mpc_params* p, const se3mpc_controller_params* cp, const se3mpc_simulator_params* sp, int B,
                                      int swarm_size, int neighbours_k, double mate_radius, int cycles, int substeps, double sim_dt,
                                      uint32_t cycle_base, int shift, int S, int iters, double sigma, double temperature, uint64_t seed,
                                      uint32_t iter_base, uint32_t index_base, const double* goal, const double* spheres,
                                      const double* sphere_vel, double sphere_t0, int K, double obstacle_weight, const double* wind,
                                      long long wind_stride, double* time, double* pos, double* vel, double* att, double* omega, double* state,
                                      double* U, double* cost, double* trace, double* plan_last, double* clearance, double* separation,
                                      int32_t* neighbours, void* workspace, size_t workspace_bytes, void* stream);

/* se3mpc_mppi_closed_loop_swarm_* with SHARED PLANS: a drone sees where its mates intend to go, not where their
 * velocities point.  The operands, the selection (d2, eligibility, ranks), separation, neighbours and every guarantee are those of
 * se3mpc_mppi_closed_loop_swarm_*; what differs is the table.  A drone's INTENT at a cycle's start is its nominal U as the cycle finds it
 * (shifted by the cycle before) rolled out from its (pos, vel) with the plan's recurrence: N rows, row k = the position before step k,
 * the instants the penalty of that cycle looks at.  The mate of rank r fills tracked row r of se3mpc_mppi_closed_loop_tracks_* -- centre
 * [k][r] = row k of its intent, radius mate_radius -- instead of moving row K + r, so one call equals, per cycle and per drone,
 * se3mpc_swarm_intent_* on the call's (pos, vel, U), then se3mpc_mppi_closed_loop_tracks_* with B = 1, index_base = b, cycle_base = C, one
 * cycle, the shared table as its K moving rows and Kt = Kn_eff, bit for bit.  The snapshot carries the intents: every workgroup reads one
 * image and writes its new (pos, vel) and its new intent to the other; the kernel boundary stays the only synchronisation.  The call
 * seeds the first image from (pos, vel, U) itself (two small launches, then one per cycle), so chained calls need nothing carried over.
 * workspace: at least se3mpc_mppi_swarm_intent_workspace_bytes(B, params->horizon, sizeof(R)) bytes = 2 x B x (6 + 3 N) elements (0 for
 * B < 0, a horizon outside [1, SE3MPC_MAX_HORIZON] or an elem_size that is not 4 or 8).  Argument rules: those of
 * se3mpc_mppi_closed_loop_swarm_* with the same codes, and neighbours_k > SE3MPC_MAX_TRACKS: SE3MPC_ERR_SHAPE. */
size_t se3mpc_mppi_swarm_intent_workspace_bytes(int B, int horizon, int elem_size);
int se3mpc_mppi_closed_loop_swarm_intent_f32(const se3mpc_params* p, const se3mpc_controller_params* cp, const se3mpc_simulator_params* sp, int B,
                                             int swarm_size, int neighbours_k, double mate_radius, int cycles, int substeps, double sim_dt,
                                             uint32_t cycle_base, int shift, int S, int iters, double sigma, double temperature, uint64_t seed,
                                             uint32_t iter_base, uint32_t index_base, const float* goal, const float* spheres,
                                             const float* sphere_vel, double sphere_t0, int K, double obstacle_weight, const float* wind,
                                             long long wind_stride, double* time, float* pos, float* vel, float* att, float* omega, double* state,
                                             float* U, float* cost, float* trace, float* plan_last, float* clearance, float* separation,
                                             int32_t* neighbours, void* workspace, size_t workspace_bytes, void* stream);
int se3mpc_mppi_closed_loop_swarm_intent_f64(const se3mpc_params* p, const se3mpc_controller_params* cp, const se3mpc_simulator_params* sp, int B,
                                             int swarm_size, int neighbours_k, double mate_radius, int cycles, int substeps, double sim_dt,
                                             uint32_t cycle_base, int shift, int S, int iters, double sigma, double temperature, uint64_t seed,
                                             uint32_t iter_base, uint32_t index_base, const double* goal, const double* spheres,
                                             const double* sphere_vel, double sphere_t0, int K, double obstacle_weight, const double* wind,
                                             long long wind_stride, double* time, double* pos, double* vel, double* att, double* omega,
                                             double* state, double* U, double* cost, double* trace, double* plan_last, double* clearance,
                                             double* separation, int32_t* neighbours, void* workspace, size_t workspace_bytes, void* stream);
/* The intent of every drone (one lane each): intent [B][N][3], row [b][k] = the position before step k of the nominal U [B][N][3] rolled
 * out from (pos, vel) [B][3] with the plan's recurrence (the P rows of plan_last of se3mpc_mppi_closed_loop_* at that U, bit for bit).
 * The seed of a run of se3mpc_mppi_closed_loop_swarm_intent_*.  params NULL or a NULL operand with B > 0: SE3MPC_ERR_NULL; invalid
 * params: the code of se3mpc_check_params; B < 0: SE3MPC_ERR_SHAPE; B = 0 is a no-op. */
int se3mpc_swarm_intent_f32(const se3mpc_params* p, int B, const float* pos, const float* vel, const float* U, float* intent, void* stream);
int se3mpc_swarm_intent_f64(const se3mpc_params* p, int B, const double* pos, const double* vel, const double* U, double* intent, void* stream);

/* The distance of every drone to its nearest eligible swarm-mate as (pos, vel) [B][3] stand: separation[b] = min(separation[b],
 * (R)sqrt(min d2)) with d2, eligibility and the E = 0 rule of se3mpc_mppi_closed_loop_swarm_*.  Reads pos and vel, writes separation only.
 * swarm_size outside [1, SE3MPC_MAX_SWARM], B < 0 or not a multiple of swarm_size: SE3MPC_ERR_SHAPE; a NULL operand with B > 0:
 * SE3MPC_ERR_NULL.  swarm_size = 1 and B = 0 are no-ops. */
int se3mpc_swarm_separation_f32(int B, int swarm_size, const float* pos, const float* vel, float* separation, void* stream);
int se3mpc_swarm_separation_f64(int B, int swarm_size, const double* pos, const double* vel, double* separation, void* stream);

/* se3mpc_mppi_closed_loop_* with the reference's full edge loop per drone (edge/main_improved.py:96-152: plan -> TrajectorySmoother
 * (control/trajectory_smoother.py:115-213) -> GeometricController (control/geometric_controller.py:413-512) -> MotorMixer and motors
 * (hardware/motor_mixer.py:168-222, hardware/motor_model.py:166-282) -> DroneSimulator (utils/drone_simulator.py:52-72)), still in ONE launch
 * and still with the clearance: for each of B drones, `cycles` times { plan and hand over as se3mpc_mppi_closed_loop_*; with smp,
 * se3mpc_smoother_update_* at the drone's clock against the plan of the cycle before; `substeps` x the step of se3mpc_closed_loop_actuated_*
 * (with mp: desired state or raw plan sample -> compute_control -> mix_commands -> the motors' wrench under motor_health ->
 * DroneSimulator.step) or of se3mpc_closed_loop_smoothed_* (without mp); clearance after every simulator step; warm start }.  The same code
 * as the entry points it fuses, hence the same bits as launching them in turn (dart_planner_amd/control/closed_loop.py, run_mppi with
 * smoother= / mixer=).  Arguments as se3mpc_mppi_closed_loop_*, and: smp, mp: each may be NULL = the stage is absent (both NULL: this IS
 * se3mpc_mppi_closed_loop_*); smoother_state [B][SE3MPC_SMOOTHER_STATE_WORDS], mixer_state [B][SE3MPC_MIXER_STATE_WORDS]: in / out;
 * motor_health NULL (exactly 1) or rows of health_stride (0 = one shared row) of four factors on the motors' thrusts, as
 * se3mpc_closed_loop_actuated_*; followed [B][9] (with smp), in / out: (pos, vel, acc) of the plan each drone follows, sampled at the clock
 * the next update_trajectory runs at -- the one value update_trajectory reads of the previous plan (trajectory_smoother.py:134-140), which
 * stays on the chip.  Zeros = nothing followed yet (what se3mpc_smoother_update_* reads through old = NULL); the sample is stored after the
 * last cycle too, so one call with cycles = C equals C calls with cycles = 1 and cycle_base = 0 .. C - 1 that carry followed, the records, U
 * and clearance along, bit for bit.
 * Argument rules: everything se3mpc_mppi_closed_loop_* rejects, with the same codes; smp and smoother_state come together, mp and
 * mixer_state come together, motor_health needs mp (SE3MPC_ERR_NULL); health_stride < 0 (SE3MPC_ERR_SHAPE); smoother / mixer parameters that
 * se3mpc_smoother_update_* / se3mpc_mixer_mix_* reject (SE3MPC_ERR_PARAM); after the B = 0 / cycles = 0 no-op: followed NULL with smp
 * (SE3MPC_ERR_NULL). */
int se3mpc_mppi_closed_loop_staged_f32(const se3mpc_params* p, const se3mpc_controller_params* cp, const se3mpc_simulator_params* sp,
                                       const se3mpc_smoother_params* smp, const se3mpc_mixer_params* mp, int B, int cycles, int substeps,
                                       double sim_dt, uint32_t cycle_base, int shift, int S, int iters, double sigma, double temperature,
                                       uint64_t seed, uint32_t iter_base, uint32_t index_base, const float* goal, const float* spheres, int K,
                                       double obstacle_weight, const float* wind, long long wind_stride, double* time, float* pos, float* vel,
                                       float* att, float* omega, double* state, double* smoother_state, double* mixer_state,
                                       const float* motor_health, long long health_stride, float* followed, float* U, float* cost, float* trace,
                                       float* plan_last, float* clearance, void* stream);
int se3mpc_mppi_closed_loop_staged_f64(const se3mpc_params* p, const se3mpc_controller_params* cp, const se3mpc_simulator_params* sp,
                                       const se3mpc_smoother_params* smp, const se3mpc_mixer_params* mp, int B, int cycles, int substeps,
                                       double sim_dt, uint32_t cycle_base, int shift, int S, int iters, double sigma, double temperature,
                                       uint64_t seed, uint32_t iter_base, uint32_t index_base, const double* goal, const double* spheres, int K,
                                       double obstacle_weight, const double* wind, long long wind_stride, double* time, double* pos, double* vel,
                                       double* att, double* omega, double* state, double* smoother_state, double* mixer_state,
                                       const double* motor_health, long long health_stride, double* followed, double* U, double* cost,
                                       double* trace, double* plan_last, double* clearance, void* stream);

/* ------------------------------------------------------------------ latency buffer and OnboardController
 * The reference's edge loop (edge/main.py:21-112; "latency.py" = src/dart_planner/utils/latency_buffer.py, "pid.py" =
 * src/dart_planner/utils/pid_controller.py, "onboard.py" = src/dart_planner/control/onboard_controller.py), one drone per lane, reproduced
 * with its quirks: while the buffer fills, push returns the CURRENT state (latency.py:68-73), so the first delayed state the controller
 * sees carries a timestamp that is not later than its last_time and compute_control_command answers thrust 0, torque 0, target (0, 0, 0)
 * for that one step (onboard.py:176-177, with last_time already moved by sense, :139-140).  All clock arithmetic is double. */

/* OnboardController.__init__ (onboard.py:25-35) and the first dt of sense (:139). */
typedef struct se3mpc_onboard_params {
  double mass, g;                              /* mass > 0                                                  (onboard.py:25-27) */
  double pid[6][4];                            /* rows pos_x, pos_y, pos_z, roll, pitch, yaw_rate; columns Kp, Ki, Kd, integral_limit
                                                  (0 = no clamp: `if self.integral_limit:`, pid.py:37)     (onboard.py:30-35) */
  double first_dt;                             /* dt of the first call, when last_time is None              (onboard.py:139)   */
} se3mpc_onboard_params;

/* Mutable OnboardController members, SE3MPC_ONBOARD_STATE_WORDS doubles per drone: [0..5] integral of pos_x, pos_y, pos_z, roll, pitch,
 * yaw_rate; [6..11] last_error, same order; [12] last_time; [13] 1 if last_time is not None.  (The setpoints are overwritten on every
 * call and are not state.) */
#define SE3MPC_ONBOARD_STATE_WORDS 14
/* LatencyBuffer members (latency.py:45-52), SE3MPC_LATENCY_STATE_WORDS doubles per drone: [0] len(buffer); [1] the ring slot of the oldest
 * entry; [2] total_samples; [3] actual_delay_s.  missed_samples = min(total_samples, depth), fill_percentage and is_ready follow. */
#define SE3MPC_LATENCY_STATE_WORDS 4
/* The reference's max_buffer_size (latency.py:34). */
#define SE3MPC_LATENCY_MAX_DEPTH 1000

int se3mpc_onboard_default_params(se3mpc_onboard_params* out);
/* LatencyBuffer.reset (latency.py:104-111) for B drones of a buffer of `depth` slots: state = device double[B][4], all zero.  The ring
 * itself needs no clearing: a slot is written before it is read. */
int se3mpc_latency_reset(int B, int depth, double* state, void* stream);
/* OnboardController.reset (onboard.py:186-193) for B drones: state = device double[B][14], all zero (last_time None). */
int se3mpc_onboard_reset(int B, double* state, void* stream);

/* DroneStateLatencyBuffer.push(state, state.timestamp) (latency.py:54-82) for B drones: time [B], pos, vel, att, omega [B][3] in; the
 * delayed state d_time [B], d_pos, d_vel, d_att, d_omega [B][3] out (the current state while the buffer fills, :68-73).  The buffer is
 * the caller's: ring [depth][12][B] (pos, vel, att, omega; field-major, drone innermost), ring_time double [depth][B], state [B][4];
 * all three in / out.  1 <= depth <= SE3MPC_LATENCY_MAX_DEPTH.  A record whose length or slot lies outside the ring reads as empty.
 * Argument rules of the entry points of this section: a NULL required operand: SE3MPC_ERR_NULL; B < 0, nsteps < 0, a negative stride,
 * a plan of more than 4096 rows, depth outside its range: SE3MPC_ERR_SHAPE; non-finite gains, limits, g, first_dt or sim_dt, mass not
 * positive: SE3MPC_ERR_PARAM.  B = 0 and nsteps = 0 are no-ops.  Every rejected call sets se3mpc_last_error and launches nothing. */
int se3mpc_latency_push_f32(int B, int depth, const double* time, const float* pos, const float* vel, const float* att,
                            const float* omega, float* ring, double* ring_time, double* state, double* d_time, float* d_pos, float* d_vel,
                            float* d_att, float* d_omega, void* stream);
int se3mpc_latency_push_f64(int B, int depth, const double* time, const double* pos, const double* vel, const double* att,
                            const double* omega, double* ring, double* ring_time, double* state, double* d_time, double* d_pos,
                            double* d_vel, double* d_att, double* d_omega, void* stream);

/* OnboardController.compute_control_command(state, trajectory) (onboard.py:172-180: sense :136-142, plan :144-161, act :163-170, the six
 * PIDController.update calls pid.py:25-51 term by term) for B drones: time [B] = state.timestamp, pos, att, omega [B][3] (the velocity is
 * not read by the control law), plans as in se3mpc_closed_loop_* (N >= 0 rows).  Outputs (any may be NULL): thrust [B], torque [B][3],
 * target_pos [B][3].  dt <= 0 gives thrust 0, torque 0, target (0, 0, 0) with last_time moved and the PIDs untouched (:176-177).
 * N = 0 (no plan) gives get_fallback_command (:182-184): thrust mass * g, torque 0, target = pos, and the record is untouched
 * (edge/main.py:91-94).  `state` [B][14] is read and updated. */
int se3mpc_onboard_control_f32(const se3mpc_onboard_params* op, int B, const double* time, const float* pos, const float* att,
                               const float* omega, int N, const double* timestamps, long long ts_stride, const float* P, long long strideP,
                               const float* V, long long strideV, const float* A, long long strideA, double* state, float* thrust,
                               float* torque, float* target_pos, void* stream);
int se3mpc_onboard_control_f64(const se3mpc_onboard_params* op, int B, const double* time, const double* pos, const double* att,
                               const double* omega, int N, const double* timestamps, long long ts_stride, const double* P,
                               long long strideP, const double* V, long long strideV, const double* A, long long strideA, double* state,
                               double* thrust, double* torque, double* target_pos, void* stream);

/* The body of the reference's edge loop (edge/main.py:80-95), `nsteps` times per drone in ONE launch:  delayed = latency_buffer.push(state)
 * [depth = 0: no buffer, delayed = state];  cmd, target = compute_control_command(delayed, plan) [N = 0: get_fallback_command, target =
 * delayed.position];  [step == gust_step: the wind becomes gust_wind];  state = DroneSimulator.step(state, cmd, sim_dt).  Arguments as
 * se3mpc_closed_loop_* (no stop_at_plan_end: every drone takes nsteps), plus the onboard parameters and records onboard_state [B][14],
 * the buffer (depth, ring, ring_time, latency_state as se3mpc_latency_push_*; with depth = 0 the three may be NULL) and the logs
 * log_target [nsteps][B][3], log_delayed_time double [nsteps][B] (each NULL or kept) next to log_state / log_cmd / log_time of
 * se3mpc_closed_loop_*; zero_thrust_steps: NULL, or int32 [B] counters (in / out) of the steps whose commanded thrust was exactly 0.
 * The same bits as nsteps chained se3mpc_latency_push_* -> se3mpc_onboard_control_* -> se3mpc_simulator_step_* launches. */
int se3mpc_edge_loop_f32(const se3mpc_onboard_params* op, const se3mpc_simulator_params* sp, int B, int nsteps, double sim_dt, int N,
                         const double* timestamps, long long ts_stride, const float* P, long long strideP, const float* V,
                         long long strideV, const float* A, long long strideA, double* time, float* pos, float* vel, float* att,
                         float* omega, double* onboard_state, int depth, float* ring, double* ring_time, double* latency_state,
                         const float* wind, long long wind_stride, int gust_step, const double* gust_wind, float* log_state,
                         float* log_cmd, double* log_time, float* log_target, double* log_delayed_time, int32_t* zero_thrust_steps,
                         void* stream);
int se3mpc_edge_loop_f64(const se3mpc_onboard_params* op, const se3mpc_simulator_params* sp, int B, int nsteps, double sim_dt, int N,
                         const double* timestamps, long long ts_stride, const double* P, long long strideP, const double* V,
                         long long strideV, const double* A, long long strideA, double* time, double* pos, double* vel, double* att,
                         double* omega, double* onboard_state, int depth, double* ring, double* ring_time, double* latency_state,
                         const double* wind, long long wind_stride, int gust_step, const double* gust_wind, double* log_state,
                         double* log_cmd, double* log_time, double* log_target, double* log_delayed_time, int32_t* zero_thrust_steps,
                         void* stream);

/* MEASUREMENT KNOB, not part of the interface a caller should build on (as se3mpc_set_rollout_variant): when se3mpc_edge_loop_* loads the ring
 * entry a push pops.  0 (default): one step ahead, before the previous step's controller and simulator arithmetic (depth >= 2; DESIGN.md
 * 5.7f).  1: in the push that pops it.  Same bits either way; 1 exists only so that tools/gpu_probe_edge_loop.py can time the difference.
 * The setting is one process-wide word read at launch time: it is not per stream or per thread, so leave it alone outside a measurement.
 * Any other value: SE3MPC_ERR_PARAM. */
int se3mpc_set_edge_loop_variant(int variant);

/* The receding-horizon Monte-Carlo on the edge loop in ONE launch: for each of B drones, `cycles` times { se3mpc_solve_*
 * from the drone's own (pos, vel) with the reference's cold start; `substeps` x the step of se3mpc_edge_loop_* (latency push ->
 * compute_control_command -> DroneSimulator.step at sim_dt) against the fresh plan, whose row k is stamped ((first_cycle + cycle) * substeps
 * * sim_dt) + k * params->dt }.  The same code as the two entry points it fuses, hence the same bits as alternating them
 * (ClosedLoopMonteCarlo.run_edge) -- without 2 x cycles kernel boundaries.  All cross-cycle state is the caller's, so a second call with
 * first_cycle = the cycles already flown continues a run bit for bit.  goal, wind, wind_stride, time, pos, vel, att, omega, X_last, acc_last,
 * info_last, overflowed as se3mpc_monte_carlo_*; onboard_state [B][SE3MPC_ONBOARD_STATE_WORDS], depth, ring, ring_time, latency_state and
 * zero_thrust_steps (NULL, or int32 [B] counters that are incremented) as se3mpc_edge_loop_* (depth = 0: no buffer, the three may be NULL).
 * Argument rules, in this order: a NULL parameter struct: SE3MPC_ERR_NULL; parameters that se3mpc_check_params, se3mpc_edge_loop_* (onboard,
 * simulator) reject: their codes; B, cycles, substeps or first_cycle < 0, horizon > 64, depth outside [0, SE3MPC_LATENCY_MAX_DEPTH],
 * (first_cycle + cycles) * substeps beyond an int: SE3MPC_ERR_SHAPE; a non-finite sim_dt: SE3MPC_ERR_PARAM; wind with a wind_stride that is
 * neither 0 nor >= 3: SE3MPC_ERR_SHAPE; B = 0: a no-op; then a NULL time, pos, vel, att, omega, onboard_state or overflowed, a NULL goal when
 * the parameters have one, a NULL ring, ring_time or latency_state when depth > 0: SE3MPC_ERR_NULL.  A rejected call launches nothing;
 * overflowed is zeroed on the stream before the launch. */
int se3mpc_monte_carlo_edge_f32(const se3mpc_params* p, const se3mpc_onboard_params* op, const se3mpc_simulator_params* sp, int B, int cycles,
                                int substeps, double sim_dt, int first_cycle, const float* goal, const float* wind, long long wind_stride,
                                double* time, float* pos, float* vel, float* att, float* omega, double* onboard_state, int depth, float* ring,
                                double* ring_time, double* latency_state, int32_t* zero_thrust_steps, float* X_last, float* acc_last,
                                se3mpc_solve_info* info_last, int32_t* overflowed, void* stream);
int se3mpc_monte_carlo_edge_f64(const se3mpc_params* p, const se3mpc_onboard_params* op, const se3mpc_simulator_params* sp, int B, int cycles,
                                int substeps, double sim_dt, int first_cycle, const double* goal, const double* wind, long long wind_stride,
                                double* time, double* pos, double* vel, double* att, double* omega, double* onboard_state, int depth,
                                double* ring, double* ring_time, double* latency_state, int32_t* zero_thrust_steps, double* X_last,
                                double* acc_last, se3mpc_solve_info* info_last, int32_t* overflowed, void* stream);

/* ------------------------------------------------------------------ mission layer: the goal source
 * GlobalMissionPlanner.get_current_goal (src/dart_planner/planning/global_mission_planner.py:182-224, "mission.py" below), the call that
 * produces the goal of every plan: a phase machine per drone -- phase, waypoint index, time of the last global plan -- unit-stripped and
 * reproduced with its quirks.  The wall clock the class reads (time.time(), :195) is the operand `now`.  Not reproduced: the np.random
 * parts (the simulated regions of :433-442 and the placeholder of :462-465, read only by the non-empty branch of _plan_exploration_goal)
 * and PlaceholderNeuralScene. */
typedef struct se3mpc_mission_params {
  double safe_altitude;          /* takeoff goal altitude, 5.0                                  (mission.py:256)   */
  double takeoff_band;           /* takeoff complete at z >= safe_altitude - band, 0.5          (:261)             */
  double waypoint_reach;         /* a waypoint is reached at distance < this, 2.0               (:322)             */
  double safety_margin;          /* GlobalMissionConfig.safety_margin, 2.0                      (:48, :376)        */
  double landing_pad_lift;       /* approach a landing pad from this far above, 3.0             (:380)             */
  double landing_step;           /* LANDING: goal z = max(floor, z - step), 1.0 and 0.5         (:347)             */
  double landing_floor;
  double emergency_step;         /* EMERGENCY: goal z = max(floor, z - step), 2.0 and 0.0       (:358)             */
  double emergency_floor;
  double emergency_altitude;     /* a global plan below this altitude outside LANDING: EMERGENCY, 0.5   (:454)     */
  double global_replan_period;   /* 1 / global_replan_frequency, 1.0                            (:60, :198)        */
  double exploration_base;       /* radius of the first exploration goal, 10.0                  (:284)             */
  double exploration_radius;     /* GlobalMissionConfig.exploration_radius, 50.0                (:46)              */
  double stamp_radius;           /* reduce_uncertainty_around_position of a global plan: 3.0, 0.2   (:411-413)     */
  double stamp_factor;
  int32_t use_neural_scene;      /* GlobalMissionConfig.use_neural_scene                        (:51)              */
  int32_t reserved;
} se3mpc_mission_params;

/* MissionPhase (mission.py:17-25) in its order; the semantic labels _apply_semantic_reasoning tells apart (:370-384). */
enum { SE3MPC_MISSION_TAKEOFF = 0, SE3MPC_MISSION_EXPLORATION = 1, SE3MPC_MISSION_MAPPING = 2, SE3MPC_MISSION_NAVIGATION = 3,
       SE3MPC_MISSION_LANDING = 4, SE3MPC_MISSION_EMERGENCY = 5 };
enum { SE3MPC_LABEL_OTHER = 0, SE3MPC_LABEL_OBSTACLE = 1, SE3MPC_LABEL_LANDING_PAD = 2, SE3MPC_LABEL_DOORWAY = 3 };

/* Mutable planner members (mission.py:95-97, :156), SE3MPC_MISSION_STATE_WORDS doubles per drone: [0] current_phase (a code above), [1]
 * current_waypoint_index, [2] last_global_plan_time, [3] global plans made (= the scene's update count with use_neural_scene).  The caller
 * may write EXPLORATION or MAPPING into [0]: nothing in the reference enters them either.  A phase word outside [0, 5] returns the position
 * as the goal (:222-224); an index below 0 or NaN reads as 0. */
#define SE3MPC_MISSION_STATE_WORDS 4

/* The reference's literals. */
int se3mpc_mission_default_params(se3mpc_mission_params* out);
/* SE3MPC_ERR_NULL; a non-finite value or a period that is not positive: SE3MPC_ERR_PARAM. */
int se3mpc_check_mission_params(const se3mpc_mission_params* mp);
/* TAKEOFF, index 0, last_global_plan_time 0.0, no plan made (mission.py:95-97, :156) for B drones. */
int se3mpc_mission_reset(int B, double* mission_state, void* stream);

/* get_current_goal for B drones, one per lane.  now [B]: the wall clock of each call; pos [B][3]; mission_state [B][SE3MPC_MISSION_STATE_WORDS]
 * in / out.  waypoints: float64 [W][3] rows shared by all drones (wp_stride 0) or per drone (wp_stride >= 3 W doubles from drone to drone);
 * labels int32 [W] under the same rule (label_stride 0 or >= W); W = 0: no waypoints (both may be NULL).  In order (mission.py:195-220): if
 * now - last_global_plan_time > global_replan_period, the global planning step -- below emergency_altitude and outside LANDING the phase
 * becomes EMERGENCY (:450-458), the plan count goes up, last_global_plan_time = now -- then the goal of the phase: TAKEOFF :254-265,
 * NAVIGATION and MAPPING :302-341 with _apply_semantic_reasoning :362-386, LANDING :343-353, EMERGENCY :355-360, EXPLORATION on its
 * empty-region branch :279-294 with nothing explored yet.  Every decision and all arithmetic in double on (double)pos; goal [B][3] is rounded
 * to the IO type once, on the store.  The stamp of the global planning step (:409-413) is row b of a table in the operand form of
 * se3mpc_ufield_stamp: stamp_centres [B][3] = the position, stamp_radius [B], stamp_radius_voxels [B] = (int)(stamp_radius / resolution),
 * stamp_factor [B]; a drone that made no global plan, and every drone without use_neural_scene, gets radius = -1 and radius_voxels = -1,
 * which se3mpc_ufield_stamp skips.
 * Argument rules: NULL params: SE3MPC_ERR_NULL; params se3mpc_check_mission_params rejects: its code; B outside [0, 2^30], W outside
 * [0, 2^20], a stride that is neither 0 nor at least a table: SE3MPC_ERR_SHAPE; with use_neural_scene a resolution that is not finite and
 * positive: SE3MPC_ERR_PARAM; B = 0: a no-op; then any NULL operand (the two tables only when W > 0): SE3MPC_ERR_NULL.  A rejected call sets
 * se3mpc_last_error and launches nothing. */
int se3mpc_mission_goal_f32(const se3mpc_mission_params* mp, int B, const double* now, const float* pos, double* mission_state,
                            const double* waypoints, long long wp_stride, const int32_t* labels, long long label_stride, int W,
                            double resolution, float* goal, double* stamp_centres, double* stamp_radius, int32_t* stamp_radius_voxels,
                            double* stamp_factor, void* stream);
int se3mpc_mission_goal_f64(const se3mpc_mission_params* mp, int B, const double* now, const double* pos, double* mission_state,
                            const double* waypoints, long long wp_stride, const int32_t* labels, long long label_stride, int W,
                            double resolution, double* goal, double* stamp_centres, double* stamp_radius, int32_t* stamp_radius_voxels,
                            double* stamp_factor, void* stream);

/* se3mpc_monte_carlo_* flying waypoint missions in ONE launch: for each of B drones, `cycles` times { se3mpc_mission_goal_*
 * on the drone's position with now = its clock + epoch; se3mpc_solve_* towards that goal; `substeps` x the step of se3mpc_closed_loop_*
 * against the fresh plan, whose row k is stamped ((first_cycle + cycle) * substeps * sim_dt) + k * params->dt }.  The same code as the three
 * entry points it fuses, hence the same bits as alternating them (ClosedLoopMonteCarlo.run_mission).  All cross-cycle state is the caller's,
 * so a second call with first_cycle = the cycles already flown continues a run bit for bit.  mp, waypoints .. resolution and mission_state
 * as se3mpc_mission_goal_*; wind .. state, X_last, acc_last, info_last and overflowed as se3mpc_monte_carlo_*; goal [B][3]: out, the last
 * cycle's goal (with cycles = 0 it stays as it is).  The stamps of the global planning steps are not applied -- they are ordered writes to
 * a grid all drones share, and the phase machine never reads it -- but logged: log_centres [cycles][B][3], log_radius, log_radius_voxels,
 * log_factor [cycles][B], rows as se3mpc_mission_goal_* writes them, cycle-major as the chain makes them; one se3mpc_ufield_stamp call with
 * S = cycles * B applies them.  All four NULL: no log.
 * Argument rules, in this order: a NULL parameter struct: SE3MPC_ERR_NULL; parameters that se3mpc_check_params, se3mpc_closed_loop_* or
 * se3mpc_check_mission_params reject: their codes; parameters without a goal (has_goal == 0): SE3MPC_ERR_PARAM; B, cycles, substeps or
 * first_cycle < 0, horizon > 64, (first_cycle + cycles) * substeps beyond an int, cycles * B beyond 2^30: SE3MPC_ERR_SHAPE; a non-finite
 * sim_dt or epoch: SE3MPC_ERR_PARAM; the wind and table rules of the entry points above; B = 0: a no-op; then a NULL time, pos, vel, att,
 * omega, state, mission_state, goal or overflowed, a NULL table when W > 0, a log of which only a part is there: SE3MPC_ERR_NULL.  A rejected
 * call launches nothing; overflowed is zeroed on the stream before the launch. */
int se3mpc_monte_carlo_mission_f32(const se3mpc_params* p, const se3mpc_controller_params* cp, const se3mpc_simulator_params* sp,
                                   const se3mpc_mission_params* mp, int B, int cycles, int substeps, double sim_dt, int first_cycle,
                                   double epoch, const double* waypoints, long long wp_stride, const int32_t* labels, long long label_stride,
                                   int W, double resolution, const float* wind, long long wind_stride, double* time, float* pos, float* vel,
                                   float* att, float* omega, double* state, double* mission_state, float* goal, double* log_centres,
                                   double* log_radius, int32_t* log_radius_voxels, double* log_factor, float* X_last, float* acc_last,
                                   se3mpc_solve_info* info_last, int32_t* overflowed, void* stream);
int se3mpc_monte_carlo_mission_f64(const se3mpc_params* p, const se3mpc_controller_params* cp, const se3mpc_simulator_params* sp,
                                   const se3mpc_mission_params* mp, int B, int cycles, int substeps, double sim_dt, int first_cycle,
                                   double epoch, const double* waypoints, long long wp_stride, const int32_t* labels, long long label_stride,
                                   int W, double resolution, const double* wind, long long wind_stride, double* time, double* pos,
                                   double* vel, double* att, double* omega, double* state, double* mission_state, double* goal,
                                   double* log_centres, double* log_radius, int32_t* log_radius_voxels, double* log_factor, double* X_last,
                                   double* acc_last, se3mpc_solve_info* info_last, int32_t* overflowed, void* stream);

/* The closed-loop MPPI Monte-Carlo on the edge loop in ONE launch: se3mpc_mppi_closed_loop_* with the act phase of
 * se3mpc_monte_carlo_edge_*.  One workgroup of min(S, 256) lanes per drone; for each of B drones, `cycles` times { plan, hand over, clearance
 * and warm start as se3mpc_mppi_closed_loop_* (the same code, hence the same bits: Philox stream index_base + b, iteration number iter_base +
 * C * iters + i with C = cycle_base + cycle, plan row k stamped (C * substeps * sim_dt) + k * params->dt); act: `substeps` x the step of
 * se3mpc_edge_loop_* (latency push -> compute_control_command -> the zero-thrust count -> DroneSimulator.step at sim_dt) against the plan on
 * the chip }.  The same code as the two entry points it fuses, hence the same bits as se3mpc_mppi_closed_loop_* with substeps = 0 followed by
 * se3mpc_edge_loop_* on plan_last, cycle by cycle (ClosedLoopMonteCarlo.run_mppi_edge) -- and with the clearance, which that chain cannot
 * measure.  substeps = 0: no act phase, no record, ring or counter is touched.
 * Operands: goal, spheres, K, wind, wind_stride, time, pos, vel, att, omega, U, cost, trace, plan_last and clearance as
 * se3mpc_mppi_closed_loop_*; onboard_state [B][SE3MPC_ONBOARD_STATE_WORDS], depth, ring [depth][12][B], ring_time [depth][B], latency_state
 * [B][SE3MPC_LATENCY_STATE_WORDS] and zero_thrust_steps (NULL, or int32 [B] counters that are added to) as se3mpc_edge_loop_*, the ring's row
 * width being this call's B (depth = 0: no buffer, the three may be NULL).  There is no geometric controller and no controller record.  All
 * cross-cycle state is the caller's, so one call with cycles = C equals C calls with cycles = 1 and cycle_base = 0 .. C - 1 on the same
 * operands, and a second call continues a run, bit for bit.  No atomics, no workspace, no allocation, no synchronise.
 * Argument rules: a NULL parameter struct: SE3MPC_ERR_NULL; parameters that se3mpc_check_params, se3mpc_edge_loop_* (onboard, simulator)
 * reject: their codes; cycles or substeps < 0, shift outside [0, N], depth outside [0, SE3MPC_LATENCY_MAX_DEPTH], (cycle_base + cycles) *
 * substeps beyond an int, wind with a wind_stride that is neither 0 nor >= 3: SE3MPC_ERR_SHAPE; everything se3mpc_mppi_* rejects (B < 0, S, iters,
 * K: SE3MPC_ERR_SHAPE; sigma, temperature, obstacle_weight: SE3MPC_ERR_PARAM); a non-finite sim_dt: SE3MPC_ERR_PARAM; B = 0 and cycles = 0 are
 * no-ops; then a NULL time, pos, vel, att, omega, onboard_state, U or cost, a NULL goal when the parameters have one, NULL spheres when K > 0, a
 * NULL ring, ring_time or latency_state when depth > 0: SE3MPC_ERR_NULL.  Every rejected call sets se3mpc_last_error and launches nothing. */
int se3mpc_mppi_closed_loop_edge_f32(const se3mpc_params* p, const se3mpc_onboard_params* op, const se3mpc_simulator_params* sp, int B, int cycles,
                                     int substeps, double sim_dt, uint32_t cycle_base, int shift, int S, int iters, double sigma,
                                     double temperature, uint64_t seed, uint32_t iter_base, uint32_t index_base, const float* goal,
                                     const float* spheres, int K, double obstacle_weight, const float* wind, long long wind_stride, double* time,
                                     float* pos, float* vel, float* att, float* omega, double* onboard_state, int depth, float* ring,
                                     double* ring_time, double* latency_state, int32_t* zero_thrust_steps, float* U, float* cost, float* trace,
                                     float* plan_last, float* clearance, void* stream);
int se3mpc_mppi_closed_loop_edge_f64(const se3mpc_params* p, const se3mpc_onboard_params* op, const se3mpc_simulator_params* sp, int B, int cycles,
                                     int substeps, double sim_dt, uint32_t cycle_base, int shift, int S, int iters, double sigma,
                                     double temperature, uint64_t seed, uint32_t iter_base, uint32_t index_base, const double* goal,
                                     const double* spheres, int K, double obstacle_weight, const double* wind, long long wind_stride,
                                     double* time, double* pos, double* vel, double* att, double* omega, double* onboard_state, int depth,
                                     double* ring, double* ring_time, double* latency_state, int32_t* zero_thrust_steps, double* U, double* cost,
                                     double* trace, double* plan_last, double* clearance, void* stream);

/* ------------------------------------------------------------------ problem layout: [b][row]
 * The batched solve: replaces _solve_se3_mpc (planner.py:230-280) = cold start (or a caller
 * x0), box, scipy.optimize.minimize(method="L-BFGS-B", jac=..., bounds=..., maxiter, gtol,
 * ftol) and _extract_solution_from_result, for B independent problems, one wavefront each.
 *   p0, v0, goal : [B][3]
 *   x0           : [B][9N] warm start, or NULL for the reference cold start
 *   X            : [B][9N] solution (result.x)
 *   info         : [B] se3mpc_solve_info
 *   acc, att, rates : [B][N][3], thrust : [B][N]   (any may be NULL)
 * All accumulations that feed a branch of L-BFGS-B run in double; `_f32` keeps the vectors in
 * float. */
/* Which generalized-Cauchy-point search se3mpc_solve_* runs while the L-BFGS memory is empty (B = theta I: the first iterate of every
 * solve and every iterate after a memory refresh).  0 (default): the closed form -- with B = theta I the published search crosses
 * exactly the breakpoints t_i <= 1/theta and stops at t = 1/theta, so the point is the projected step P(x - g/theta), one parallel
 * pass.  1: the published sequential breakpoint search (Byrd-Lu-Nocedal-Zhu 1995, algorithm CP) everywhere, as SciPy's L-BFGS-B
 * runs it: same iterates up to the rounding of its accumulated dtm = -f1/f2 (1e-8 N on thrust entries when nearly all of sum g^2
 * sits on variables that reach their bounds), ~5x slower on the first iterate.  With 1 the f64 solve reproduces the reference's
 * thrust block to 1e-9. */
int se3mpc_set_solver_variant(int variant);

int se3mpc_solve_f32(const se3mpc_params* p, int B, const float* p0, const float* v0, const float* goal,
                     const float* x0, float* X, se3mpc_solve_info* info, float* acc, float* att,
                     float* rates, float* thrust, void* stream);
int se3mpc_solve_f64(const se3mpc_params* p, int B, const double* p0, const double* v0, const double* goal,
                     const double* x0, double* X, se3mpc_solve_info* info, double* acc, double* att,
                     double* rates, double* thrust, void* stream);

/* Host-latency form of the solve: what SE3MPCPlanner.plan_trajectory (planner.py:215-228, one problem, the caller blocks until the
 * plan exists) binds.  ONE call = launch + wait: the same arguments as se3mpc_solve_* -- all of them HOST-PINNED, DEVICE-MAPPED
 * buffers (hipHostMalloc / torch pin_memory): the kernel reads its 72 bytes of input and writes its results in place -- plus
 *   done    : 8-byte aligned word in host-pinned, device-mapped memory
 *   ticket  : any value other than *done's current one (a per-call counter)
 *   timeout_us : after this long the wait falls back to hipStreamSynchronize
 * The kernel's last act is a system-scope fence and a store of `ticket` into *done; this function spins on that word instead of
 * paying hipStreamSynchronize's wake-up.  The batch must fit ONE wavefront (B <= 64 / lanes-per-problem: 8 problems at horizon <= 8,
 * 2 at horizon <= 32, 1 beyond; SE3MPC_ERR_SHAPE otherwise -- use se3mpc_solve_* then).  Returns when the results are in the buffers. */
int se3mpc_plan_host_f32(const se3mpc_params* p, int B, const float* p0, const float* v0, const float* goal,
                         const float* x0, float* X, se3mpc_solve_info* info, float* acc, float* att, float* rates,
                         float* thrust, unsigned long long* done, unsigned long long ticket, double timeout_us, void* stream);
int se3mpc_plan_host_f64(const se3mpc_params* p, int B, const double* p0, const double* v0, const double* goal,
                         const double* x0, double* X, se3mpc_solve_info* info, double* acc, double* att, double* rates,
                         double* thrust, unsigned long long* done, unsigned long long ticket, double timeout_us, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SE3MPC_H */
