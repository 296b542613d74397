// smoother.hip -- the reference's TrajectorySmoother on the device, one drone per lane: the stage of its edge loop
// (edge/main_improved.py:96-152) between planner and controller.
//
// Reference arithmetic ("smoother.py" = src/dart_planner/control/trajectory_smoother.py), unit-stripped and reproduced with its quirks:
//   * update_trajectory       smoother.py:115-165   se3mpc_smoother_update_*
//   * get_desired_state       smoother.py:167-213   se3mpc_smoother_desired_*  (and :64-113, :215-338, everything it calls)
//   * the control-rate loop   get_desired_state -> GeometricController.compute_control -> DroneSimulator.step, `nsteps` times in ONE
//                             launch: se3mpc_closed_loop_smoothed_* (lane_loop / control_step / simulator_step of closed_loop_device.hpp)
// The Butterworth filters the class builds (:56-62) are never applied by it and are not built here.
//
// Contraction is off in this file for the reason it is off in closed_loop.hip: the transition thresholds, the three per-call clamps, the
// two norm clamps of the transition and the `norm(last_filtered_pos) > 0` filter bypass compare against values NumPy forms without FMA.
#pragma clang fp contract(off)
#include "smoother_device.hpp"

namespace se3mpc {

__global__ void __launch_bounds__(64)
smoother_reset_kernel(int B, double* __restrict__ state) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  double* s = state + (size_t)b * SE3MPC_SMOOTHER_STATE_WORDS;
  for (int i = 0; i < SE3MPC_SMOOTHER_STATE_WORDS; ++i) s[i] = 0.0;               // smoother.py:28-46
}

template <typename R>
__global__ void __launch_bounds__(64)
smoother_update_kernel(SmoothDev<R> d, int B, const double* __restrict__ now, PlanView<R> old_plan, PlanView<R> new_plan, double* __restrict__ state) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  SmoothRegs<R> s = load_smooth<R>(state + (size_t)b * SE3MPC_SMOOTHER_STATE_WORDS);
  const PlanView<R> o = old_plan.of(b), n = new_plan.of(b);
  smoother_update<R>(d, s, now[b], old_plan.N, o.ts, o.P, o.V, o.A, new_plan.N, n.ts, n.P, n.V, n.A, state + (size_t)b * SE3MPC_SMOOTHER_STATE_WORDS + 9);
  store_smooth<R>(state + (size_t)b * SE3MPC_SMOOTHER_STATE_WORDS, s);
}

template <typename R>
__global__ void __launch_bounds__(64)
smoother_desired_kernel(SmoothDev<R> d, int B, const double* __restrict__ now, const R* __restrict__ pos, const R* __restrict__ vel, PlanView<R> plan,
                        double* __restrict__ state, R* __restrict__ target, int32_t* __restrict__ branch) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  SmoothRegs<R> s = load_smooth<R>(state + (size_t)b * SE3MPC_SMOOTHER_STATE_WORDS);
  const R p[3] = {pos[3 * b], pos[3 * b + 1], pos[3 * b + 2]}, v[3] = {vel[3 * b], vel[3 * b + 1], vel[3 * b + 2]};
  const PlanView<R> rows = plan.of(b);
  R x[9];
  PlanCursor<R> cur;
  cursor_reset(cur);
  const int br = smoother_desired<R>(d, s, state + (size_t)b * SE3MPC_SMOOTHER_STATE_WORDS + 9, now[b], p, v, plan.N, rows.ts, rows.P, rows.V, rows.A, cur, x);
  store_smooth<R>(state + (size_t)b * SE3MPC_SMOOTHER_STATE_WORDS, s);
  if (target != nullptr) for (int i = 0; i < 9; ++i) target[9 * b + i] = x[i];
  if (branch != nullptr) branch[b] = br;
}

// ---- nsteps x (get_desired_state, compute_control, DroneSimulator.step) per drone in one launch: lane_loop, as se3mpc_closed_loop_*, with
// this step in place of flight_step and no stop rule
template <typename R>
__global__ void __launch_bounds__(64)
closed_loop_smoothed_kernel(SmoothDev<R> d, CtrlDev<R> c, SimDev<R> m, int B, int nsteps, double sim_dt, PlanView<R> plan, double* __restrict__ time,
                            R* __restrict__ pos, R* __restrict__ vel, R* __restrict__ att, R* __restrict__ omega, double* __restrict__ state,
                            double* __restrict__ smoother_state, const R* __restrict__ wind, long long wind_stride, int gust_step, R gx, R gy, R gz,
                            R* __restrict__ log_state, R* __restrict__ log_cmd, double* __restrict__ log_time, R* __restrict__ log_target) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  CtrlRegs<R> s = load_ctrl<R>(state + (size_t)b * SE3MPC_CONTROLLER_STATE_WORDS);
  SmoothRegs<R> sm = load_smooth<R>(smoother_state + (size_t)b * SE3MPC_SMOOTHER_STATE_WORDS);
  DroneRegs<R> dr;
  dr.load(b, pos, vel, att, omega, wind, wind_stride, time);
  const int N = plan.N;
  const PlanView<R> rows = plan.of(b);
  const double* __restrict__ ts = rows.ts;
  const R* __restrict__ Pb = rows.P;
  const R* __restrict__ Vb = rows.V;
  const R* __restrict__ Ab = rows.A;
  const R dt = (R)sim_dt;
  PlanCursor<R> cur;
  cursor_reset(cur);
  lane_loop<R>(dr, b, B, nsteps, gust_step, gx, gy, gz, false, 0.0, log_state, log_cmd, log_time, [&](int step, R& th, R* tq) {
    smoothed_step<R>(d, c, m, sm, smoother_state + (size_t)b * SE3MPC_SMOOTHER_STATE_WORDS + 9, s, cur, N, ts, Pb, Vb, Ab, dr.p, dr.v, dr.a, dr.w,
                     dr.t, dt, sim_dt, dr.wd, th, tq, log_target != nullptr ? log_target + ((size_t)step * B + b) * 9 : nullptr);
  });
  dr.store(b, pos, vel, att, omega, time);
  store_ctrl<R>(state + (size_t)b * SE3MPC_CONTROLLER_STATE_WORDS, s);
  store_smooth<R>(smoother_state + (size_t)b * SE3MPC_SMOOTHER_STATE_WORDS, sm);
}

// a plan operand of the smoother's entry points (closed_loop_device.hpp: plan_shape_ok with no minimum, plan_present where `required`), both
// parts before the caller's no-op return
template <typename R>
static int check_plan(const PlanView<R>& plan, bool required, const char* what) {
  if (!plan_shape_ok(plan, 0)) return reject(SE3MPC_ERR_SHAPE, what);
  if (required && !plan_present(plan)) return reject(SE3MPC_ERR_NULL, what);
  return SE3MPC_OK;
}

template <typename R>
int smoother_update_impl(const se3mpc_smoother_params* mp, int B, const double* now, const PlanView<R>& old_plan, const PlanView<R>& new_plan,
                         double* state, void* stream) {
  int rc = check_smoother_params(mp);
  if (rc) return reject(rc, "se3mpc_smoother_update: smoother parameters");
  if (B < 0) return reject(SE3MPC_ERR_SHAPE, "se3mpc_smoother_update: B < 0");
  rc = check_plan(old_plan, false, "se3mpc_smoother_update: old plan");
  if (rc) return rc;
  rc = check_plan(new_plan, true, "se3mpc_smoother_update: new plan");
  if (rc) return rc;
  if (B == 0) return SE3MPC_OK;
  if (!now || !state) return reject(SE3MPC_ERR_NULL, "se3mpc_smoother_update: now / state");
  hipLaunchKernelGGL(smoother_update_kernel<R>, dim3(grid_for(B, 64)), dim3(64), 0, (hipStream_t)stream, make_smooth_dev<R>(*mp), B, now, old_plan,
                     new_plan, state);
  return launch_status("se3mpc_smoother_update");
}

template <typename R>
int smoother_desired_impl(const se3mpc_smoother_params* mp, int B, const double* now, const R* pos, const R* vel, const PlanView<R>& plan,
                          double* state, R* target, int32_t* branch, void* stream) {
  int rc = check_smoother_params(mp);
  if (rc) return reject(rc, "se3mpc_smoother_desired: smoother parameters");
  if (B < 0) return reject(SE3MPC_ERR_SHAPE, "se3mpc_smoother_desired: B < 0");
  rc = check_plan(plan, true, "se3mpc_smoother_desired: plan");
  if (rc) return rc;
  if (B == 0) return SE3MPC_OK;
  if (!now || !pos || !vel || !state) return reject(SE3MPC_ERR_NULL, "se3mpc_smoother_desired: now / pos / vel / state");
  hipLaunchKernelGGL(smoother_desired_kernel<R>, dim3(grid_for(B, 64)), dim3(64), 0, (hipStream_t)stream, make_smooth_dev<R>(*mp), B, now, pos, vel,
                     plan, state, target, branch);
  return launch_status("se3mpc_smoother_desired");
}

template <typename R>
int closed_loop_smoothed_impl(const se3mpc_smoother_params* mp, const se3mpc_controller_params* cp, const se3mpc_simulator_params* sp, int B,
                              int nsteps, double sim_dt, const PlanView<R>& plan, double* time, R* pos, R* vel, R* att, R* omega,
                              double* state, double* smoother_state, const R* wind, long long wind_stride, int gust_step,
                              const double* gust_wind, R* log_state, R* log_cmd, double* log_time, R* log_target, void* stream) {
  int rc = check_smoother_params(mp);
  if (rc) return reject(rc, "se3mpc_closed_loop_smoothed: smoother parameters");
  rc = check_controller_params(cp);
  if (rc) return reject(rc, "se3mpc_closed_loop_smoothed: controller parameters");
  rc = check_simulator_params(sp);
  if (rc) return reject(rc, "se3mpc_closed_loop_smoothed: simulator parameters");
  if (!std::isfinite(sim_dt)) return reject(SE3MPC_ERR_PARAM, "se3mpc_closed_loop_smoothed: sim_dt");
  if (B < 0 || nsteps < 0 || wind_stride < 0) return reject(SE3MPC_ERR_SHAPE, "se3mpc_closed_loop_smoothed: B / nsteps / wind_stride < 0");
  rc = check_plan(plan, true, "se3mpc_closed_loop_smoothed: plan");
  if (rc) return rc;
  if (B == 0 || nsteps == 0) return SE3MPC_OK;
  if (!time || !pos || !vel || !att || !omega || !state || !smoother_state || (gust_step >= 0 && !gust_wind))
    return reject(SE3MPC_ERR_NULL, "se3mpc_closed_loop_smoothed: a required operand is NULL");
  const R gx = gust_step >= 0 ? (R)gust_wind[0] : (R)0, gy = gust_step >= 0 ? (R)gust_wind[1] : (R)0, gz = gust_step >= 0 ? (R)gust_wind[2] : (R)0;
  hipLaunchKernelGGL(closed_loop_smoothed_kernel<R>, dim3(grid_for(B, 64)), dim3(64), 0, (hipStream_t)stream, make_smooth_dev<R>(*mp),
                     make_ctrl_dev<R>(*cp), make_sim_dev<R>(*sp), B, nsteps, sim_dt, plan, time, pos, vel, att, omega, state, smoother_state, wind,
                     wind_stride, gust_step, gx, gy, gz, log_state, log_cmd, log_time, log_target);
  return launch_status("se3mpc_closed_loop_smoothed");
}

}  // namespace se3mpc

using namespace se3mpc;

extern "C" int se3mpc_smoother_default_params(se3mpc_smoother_params* out) {
  if (out == nullptr) return SE3MPC_ERR_NULL;
  // smoother.py:19 (transition_time), :24-26 (limits), :179 (dt), :101 (window), :151 (thresholds), :176 (timeout), :329-331 (decay)
  const se3mpc_smoother_params d = {0.5, 5.0, 3.0, 10.0, 0.01, 0.1, 0.5, 1.0, 2.0, 2.0, 5.0};
  *out = d;
  return SE3MPC_OK;
}

extern "C" int se3mpc_smoother_reset(int B, double* state, void* stream) {
  if (B < 0) return reject(SE3MPC_ERR_SHAPE, "se3mpc_smoother_reset: B < 0");
  if (B == 0) return SE3MPC_OK;
  if (!state) return reject(SE3MPC_ERR_NULL, "se3mpc_smoother_reset: state");
  hipLaunchKernelGGL(smoother_reset_kernel, dim3(grid_for(B, 64)), dim3(64), 0, (hipStream_t)stream, B, state);
  return launch_status("se3mpc_smoother_reset");
}

#define SE3MPC_DEFINE_SMOOTHER_API(SUF, R)                                                                                          \
  extern "C" int se3mpc_smoother_update_##SUF(const se3mpc_smoother_params* mp, int B, const double* now, int N_old, const double* ts_old, \
                                              long long ts_old_stride, const R* P_old, long long strideP_old, const R* V_old,          \
                                              long long strideV_old, const R* A_old, long long strideA_old, int N_new,                 \
                                              const double* ts_new, long long ts_new_stride, const R* P_new, long long strideP_new,    \
                                              const R* V_new, long long strideV_new, const R* A_new, long long strideA_new,            \
                                              double* state, void* stream) {                                                          \
    return smoother_update_impl<R>(mp, B, now, PlanView<R>{N_old, ts_old, ts_old_stride, P_old, strideP_old, V_old, strideV_old, A_old, strideA_old}, \
                                   PlanView<R>{N_new, ts_new, ts_new_stride, P_new, strideP_new, V_new, strideV_new, A_new, strideA_new}, state, \
                                   stream);                                                                                         \
  }                                                                                                                                 \
  extern "C" int se3mpc_smoother_desired_##SUF(const se3mpc_smoother_params* mp, int B, const double* now, const R* pos, const R* vel, \
                                               int N, const double* timestamps, long long ts_stride, const R* P, long long strideP,    \
                                               const R* V, long long strideV, const R* A, long long strideA, double* state, R* target, \
                                               int32_t* branch, void* stream) {                                                       \
    return smoother_desired_impl<R>(mp, B, now, pos, vel, PlanView<R>{N, timestamps, ts_stride, P, strideP, V, strideV, A, strideA}, state, \
                                    target, branch, stream);                                                                        \
  }                                                                                                                                 \
  extern "C" int se3mpc_closed_loop_smoothed_##SUF(const se3mpc_smoother_params* mp, const se3mpc_controller_params* cp,               \
                                                   const se3mpc_simulator_params* sp, int B, int nsteps, double sim_dt, int N,         \
                                                   const double* timestamps, long long ts_stride, const R* P, long long strideP,       \
                                                   const R* V, long long strideV, const R* A, long long strideA, double* time, R* pos, \
                                                   R* vel, R* att, R* omega, double* state, double* smoother_state, const R* wind,     \
                                                   long long wind_stride, int gust_step, const double* gust_wind, R* log_state,        \
                                                   R* log_cmd, double* log_time, R* log_target, void* stream) {                        \
    return closed_loop_smoothed_impl<R>(mp, cp, sp, B, nsteps, sim_dt, PlanView<R>{N, timestamps, ts_stride, P, strideP, V, strideV, A, strideA}, \
                                        time, pos, vel, att, omega, state, smoother_state, wind, wind_stride, gust_step, gust_wind,    \
                                        log_state, log_cmd, log_time, log_target, stream);                                          \
  }

SE3MPC_DEFINE_SMOOTHER_API(f32, float)
SE3MPC_DEFINE_SMOOTHER_API(f64, double)
