// edge_loop.hip -- the reference's edge loop on the device, one drone per lane: the loop of edge/main.py:21-112, the only
// place where the reference models estimator -> controller transport delay.
//
// Reference arithmetic ("latency.py" = src/dart_planner/utils/latency_buffer.py, "pid.py" = src/dart_planner/utils/pid_controller.py,
// "onboard.py" = src/dart_planner/control/onboard_controller.py), unit-stripped and reproduced with its quirks:
//   * LatencyBuffer.push / reset            latency.py:54-82, :104-111     se3mpc_latency_push_*, se3mpc_latency_reset
//   * compute_control_command / fallback    onboard.py:95-184, pid.py:25-51 se3mpc_onboard_control_*, se3mpc_onboard_reset
//   * the 100 Hz loop body                  edge/main.py:80-95             se3mpc_edge_loop_*: push -> control or fallback -> [gust] ->
//                                           DroneSimulator.step, `nsteps` times in ONE launch (lane_loop / simulator_step / sample_plan of
//                                           closed_loop_device.hpp)
// The buffer is a ring in HBM that the caller owns, so a run continues across launches; it is NOT staged in LDS (at f64 one slot of one
// wavefront is 6.5 KiB: 64 KiB at depth 10, and the depth limit would depend on the precision) -- the loop loads the slot the next step pops
// before the current step's arithmetic instead (LatencyLane, edge_device.hpp).
//
// Contraction is off in this file for the reason it is off in closed_loop.hip: the integral clamps, the thrust clip and the dt <= 0 rule
// compare against values NumPy forms without FMA.
#pragma clang fp contract(off)
#include "edge_device.hpp"

namespace se3mpc {

static int g_edge_loop_variant = 0;   // se3mpc_set_edge_loop_variant

__global__ void __launch_bounds__(64)
words_reset_kernel(int B, int words, double* __restrict__ state) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  for (int i = 0; i < words; ++i) state[(size_t)b * words + i] = 0.0;             // latency.py:104-111 / onboard.py:186-193
}

template <typename R>
__global__ void __launch_bounds__(64)
latency_push_kernel(int B, int depth, const double* __restrict__ time, const R* __restrict__ pos, const R* __restrict__ vel,
                    const R* __restrict__ att, const R* __restrict__ omega, R* ring, double* ring_time, double* __restrict__ state,
                    double* __restrict__ d_time, R* __restrict__ d_pos, R* __restrict__ d_vel, R* __restrict__ d_att, R* __restrict__ d_omega) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  DroneRegs<R> cur, del;
  cur.load(b, pos, vel, att, omega, (const R*)nullptr, 0, time);
  LatencyLane<R> lat;
  lat.ring = LatRing<R>{ring, ring_time, depth, B, b};
  lat.begin(state + (size_t)b * SE3MPC_LATENCY_STATE_WORDS);
  lat.push(cur, del, false);
  lat.end(state + (size_t)b * SE3MPC_LATENCY_STATE_WORDS);
  del.store(b, d_pos, d_vel, d_att, d_omega, d_time);
}

template <typename R>
__global__ void __launch_bounds__(64)
onboard_control_kernel(OnboardDev<R> c, int B, const double* __restrict__ time, const R* __restrict__ pos, const R* __restrict__ att,
                       const R* __restrict__ omega, PlanView<R> plan, double* __restrict__ state, R* __restrict__ thrust, R* __restrict__ torque,
                       R* __restrict__ target_pos) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const R p[3] = {pos[3 * b], pos[3 * b + 1], pos[3 * b + 2]}, a[3] = {att[3 * b], att[3 * b + 1], att[3 * b + 2]},
          w[3] = {omega[3 * b], omega[3 * b + 1], omega[3 * b + 2]};
  R th, tq[3], tg[3];
  if (plan.N > 0) {
    OnboardRegs<R> s = load_onboard<R>(state + (size_t)b * SE3MPC_ONBOARD_STATE_WORDS);
    const PlanView<R> rows = plan.of(b);
    PlanCursor<R> cur;
    cursor_reset(cur);
    onboard_step<R>(c, s, cur, plan.N, rows.ts, rows.P, rows.V, rows.A, time[b], p, a, w, th, tq, tg);
    store_onboard<R>(state + (size_t)b * SE3MPC_ONBOARD_STATE_WORDS, s);
  } else {
    onboard_fallback<R>(c, p, th, tq, tg);
  }
  if (thrust != nullptr) thrust[b] = th;
  if (torque != nullptr) for (int i = 0; i < 3; ++i) torque[3 * b + i] = tq[i];
  if (target_pos != nullptr) for (int i = 0; i < 3; ++i) target_pos[3 * b + i] = tg[i];
}

// ---- nsteps x (push, control or fallback, [gust], simulate) per drone in one launch: lane_loop, as se3mpc_closed_loop_*, with no stop rule
template <typename R>
__global__ void __launch_bounds__(64)
edge_loop_kernel(OnboardDev<R> c, SimDev<R> m, int B, int nsteps, double sim_dt, PlanView<R> plan, double* __restrict__ time,
                 R* __restrict__ pos, R* __restrict__ vel, R* __restrict__ att, R* __restrict__ omega, double* __restrict__ onboard_state,
                 int depth, R* ring, double* ring_time, double* __restrict__ latency_state, const R* __restrict__ wind, long long wind_stride,
                 int gust_step, R gx, R gy, R gz, R* __restrict__ log_state, R* __restrict__ log_cmd, double* __restrict__ log_time,
                 R* __restrict__ log_target, double* __restrict__ log_delayed_time, int32_t* __restrict__ zero_thrust_steps, int early_load) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  OnboardRegs<R> s = load_onboard<R>(onboard_state + (size_t)b * SE3MPC_ONBOARD_STATE_WORDS);
  DroneRegs<R> d;
  d.load(b, pos, vel, att, omega, wind, wind_stride, time);
  const int N = plan.N;
  const PlanView<R> rows = plan.of(b);
  const double* __restrict__ ts = rows.ts;
  const R* __restrict__ Pb = rows.P;
  const R* __restrict__ Vb = rows.V;
  const R* __restrict__ Ab = rows.A;
  const R dt = (R)sim_dt;
  PlanCursor<R> cur;
  cursor_reset(cur);
  LatencyLane<R> lat;
  lat.ring = LatRing<R>{ring, ring_time, depth, B, b};
  if (depth > 0) lat.begin(latency_state + (size_t)b * SE3MPC_LATENCY_STATE_WORDS);
  int zeros = 0;
  lane_loop<R>(d, b, B, nsteps, gust_step, gx, gy, gz, false, 0.0, log_state, log_cmd, log_time, [&](int step, R& th, R* tq) {
    edge_step<R>(c, m, s, cur, lat, depth, early_load != 0 && step + 1 < nsteps, N, ts, Pb, Vb, Ab, d, dt, sim_dt, zeros, th, tq,
                 [&](const R* tg, double delayed_t) {
                   if (log_target != nullptr) for (int i = 0; i < 3; ++i) log_target[((size_t)step * B + b) * 3 + i] = tg[i];
                   if (log_delayed_time != nullptr) log_delayed_time[(size_t)step * B + b] = delayed_t;
                 });
  });
  d.store(b, pos, vel, att, omega, time);
  store_onboard<R>(onboard_state + (size_t)b * SE3MPC_ONBOARD_STATE_WORDS, s);
  if (depth > 0) lat.end(latency_state + (size_t)b * SE3MPC_LATENCY_STATE_WORDS);
  if (zero_thrust_steps != nullptr) zero_thrust_steps[b] += zeros;
}

static int words_reset(const char* what, int B, int words, double* state, void* stream) {
  if (B < 0) return reject(SE3MPC_ERR_SHAPE, what);
  if (B == 0) return SE3MPC_OK;
  if (!state) return reject(SE3MPC_ERR_NULL, what);
  hipLaunchKernelGGL(words_reset_kernel, dim3(grid_for(B, 64)), dim3(64), 0, (hipStream_t)stream, B, words, state);
  return launch_status(what);
}

// a plan operand of this file's entry points: N >= 0 rows (0 = no plan: the fallback), both parts before the caller's no-op return
template <typename R>
static int check_edge_plan(const PlanView<R>& plan, const char* what) {
  if (!plan_shape_ok(plan, 0)) return reject(SE3MPC_ERR_SHAPE, what);
  if (!plan_present(plan)) return reject(SE3MPC_ERR_NULL, what);
  return SE3MPC_OK;
}

template <typename R>
int latency_push_impl(int B, int depth, const double* time, const R* pos, const R* vel, const R* att, const R* omega, R* ring,
                      double* ring_time, double* state, double* d_time, R* d_pos, R* d_vel, R* d_att, R* d_omega, void* stream) {
  if (B < 0 || depth < 1 || depth > SE3MPC_LATENCY_MAX_DEPTH) return reject(SE3MPC_ERR_SHAPE, "se3mpc_latency_push: B < 0 or depth outside [1, 1000]");
  if (B == 0) return SE3MPC_OK;
  if (!time || !pos || !vel || !att || !omega || !ring || !ring_time || !state || !d_time || !d_pos || !d_vel || !d_att || !d_omega)
    return reject(SE3MPC_ERR_NULL, "se3mpc_latency_push: a required operand is NULL");
  hipLaunchKernelGGL(latency_push_kernel<R>, dim3(grid_for(B, 64)), dim3(64), 0, (hipStream_t)stream, B, depth, time, pos, vel, att, omega, ring,
                     ring_time, state, d_time, d_pos, d_vel, d_att, d_omega);
  return launch_status("se3mpc_latency_push");
}

template <typename R>
int onboard_control_impl(const se3mpc_onboard_params* op, int B, const double* time, const R* pos, const R* att, const R* omega,
                         const PlanView<R>& plan, double* state, R* thrust, R* torque, R* target_pos, void* stream) {
  int rc = check_onboard_params(op);
  if (rc) return reject(rc, "se3mpc_onboard_control: onboard parameters");
  if (B < 0) return reject(SE3MPC_ERR_SHAPE, "se3mpc_onboard_control: B < 0");
  rc = check_edge_plan(plan, "se3mpc_onboard_control: plan");
  if (rc) return rc;
  if (B == 0) return SE3MPC_OK;
  if (!time || !pos || !att || !omega || !state) return reject(SE3MPC_ERR_NULL, "se3mpc_onboard_control: time / pos / att / omega / state");
  hipLaunchKernelGGL(onboard_control_kernel<R>, dim3(grid_for(B, 64)), dim3(64), 0, (hipStream_t)stream, make_onboard_dev<R>(*op), B, time, pos,
                     att, omega, plan, state, thrust, torque, target_pos);
  return launch_status("se3mpc_onboard_control");
}

template <typename R>
int edge_loop_impl(const se3mpc_onboard_params* op, const se3mpc_simulator_params* sp, int B, int nsteps, double sim_dt, const PlanView<R>& plan,
                   double* time, R* pos, R* vel, R* att, R* omega, double* onboard_state, int depth, R* ring, double* ring_time,
                   double* latency_state, const R* wind, long long wind_stride, int gust_step, const double* gust_wind, R* log_state,
                   R* log_cmd, double* log_time, R* log_target, double* log_delayed_time, int32_t* zero_thrust_steps, void* stream) {
  int rc = check_onboard_params(op);
  if (rc) return reject(rc, "se3mpc_edge_loop: onboard parameters");
  rc = check_simulator_params(sp);
  if (rc) return reject(rc, "se3mpc_edge_loop: simulator parameters");
  if (!std::isfinite(sim_dt)) return reject(SE3MPC_ERR_PARAM, "se3mpc_edge_loop: sim_dt");
  if (B < 0 || nsteps < 0 || wind_stride < 0 || depth < 0 || depth > SE3MPC_LATENCY_MAX_DEPTH)
    return reject(SE3MPC_ERR_SHAPE, "se3mpc_edge_loop: B / nsteps / wind_stride < 0 or depth outside [0, 1000]");
  rc = check_edge_plan(plan, "se3mpc_edge_loop: plan");
  if (rc) return rc;
  if (B == 0 || nsteps == 0) return SE3MPC_OK;
  if (!time || !pos || !vel || !att || !omega || !onboard_state || (depth > 0 && (!ring || !ring_time || !latency_state)) ||
      (gust_step >= 0 && !gust_wind))
    return reject(SE3MPC_ERR_NULL, "se3mpc_edge_loop: a required operand is NULL");
  const R gx = gust_step >= 0 ? (R)gust_wind[0] : (R)0, gy = gust_step >= 0 ? (R)gust_wind[1] : (R)0, gz = gust_step >= 0 ? (R)gust_wind[2] : (R)0;
  hipLaunchKernelGGL(edge_loop_kernel<R>, dim3(grid_for(B, 64)), dim3(64), 0, (hipStream_t)stream, make_onboard_dev<R>(*op), make_sim_dev<R>(*sp), B,
                     nsteps, sim_dt, plan, time, pos, vel, att, omega, onboard_state, depth, ring, ring_time, latency_state, wind, wind_stride,
                     gust_step, gx, gy, gz, log_state, log_cmd, log_time, log_target, log_delayed_time, zero_thrust_steps, g_edge_loop_variant == 0 ? 1 : 0);
  return launch_status("se3mpc_edge_loop");
}

}  // namespace se3mpc

using namespace se3mpc;

extern "C" int se3mpc_onboard_default_params(se3mpc_onboard_params* out) {
  if (out == nullptr) return SE3MPC_ERR_NULL;
  // onboard.py:25 (mass, g), :30-35 (the six PIDController's), :139 (the first dt)
  const se3mpc_onboard_params d = {1.0, 9.81, {{10.0, 1.0, 5.0, 2.0}, {10.0, 1.0, 5.0, 2.0}, {12.0, 1.5, 6.0, 2.0}, {8.0, 0.0, 2.0, 1.0},
                                               {8.0, 0.0, 2.0, 1.0}, {4.0, 0.0, 1.0, 0.5}}, 0.01};
  *out = d;
  return SE3MPC_OK;
}

extern "C" int se3mpc_set_edge_loop_variant(int variant) {
  if (variant < 0 || variant > 1) return reject(SE3MPC_ERR_PARAM, "se3mpc_set_edge_loop_variant: 0 or 1");
  g_edge_loop_variant = variant;
  return SE3MPC_OK;
}

extern "C" int se3mpc_latency_reset(int B, int depth, double* state, void* stream) {
  if (depth < 1 || depth > SE3MPC_LATENCY_MAX_DEPTH) return reject(SE3MPC_ERR_SHAPE, "se3mpc_latency_reset: depth outside [1, 1000]");
  return words_reset("se3mpc_latency_reset", B, SE3MPC_LATENCY_STATE_WORDS, state, stream);
}

extern "C" int se3mpc_onboard_reset(int B, double* state, void* stream) {
  return words_reset("se3mpc_onboard_reset", B, SE3MPC_ONBOARD_STATE_WORDS, state, stream);
}

#define SE3MPC_DEFINE_EDGE_API(SUF, R)                                                                                              \
  extern "C" int se3mpc_latency_push_##SUF(int B, int depth, const double* time, const R* pos, const R* vel, const R* att,             \
                                           const R* omega, R* ring, double* ring_time, double* state, double* d_time, R* d_pos,        \
                                           R* d_vel, R* d_att, R* d_omega, void* stream) {                                             \
    return latency_push_impl<R>(B, depth, time, pos, vel, att, omega, ring, ring_time, state, d_time, d_pos, d_vel, d_att, d_omega,    \
                                stream);                                                                                            \
  }                                                                                                                                 \
  extern "C" int se3mpc_onboard_control_##SUF(const se3mpc_onboard_params* op, int B, const double* time, const R* pos, const R* att,  \
                                              const R* omega, int N, const double* timestamps, long long ts_stride, const R* P,        \
                                              long long strideP, const R* V, long long strideV, const R* A, long long strideA,         \
                                              double* state, R* thrust, R* torque, R* target_pos, void* stream) {                      \
    return onboard_control_impl<R>(op, B, time, pos, att, omega, PlanView<R>{N, timestamps, ts_stride, P, strideP, V, strideV, A, strideA}, \
                                   state, thrust, torque, target_pos, stream);                                                      \
  }                                                                                                                                 \
  extern "C" int se3mpc_edge_loop_##SUF(const se3mpc_onboard_params* op, const se3mpc_simulator_params* sp, int B, int nsteps,          \
                                        double sim_dt, int N, const double* timestamps, long long ts_stride, const R* P,               \
                                        long long strideP, const R* V, long long strideV, const R* A, long long strideA, double* time, \
                                        R* pos, R* vel, R* att, R* omega, double* onboard_state, int depth, R* ring, double* ring_time, \
                                        double* latency_state, const R* wind, long long wind_stride, int gust_step,                    \
                                        const double* gust_wind, R* log_state, R* log_cmd, double* log_time, R* log_target,            \
                                        double* log_delayed_time, int32_t* zero_thrust_steps, void* stream) {                          \
    return edge_loop_impl<R>(op, sp, B, nsteps, sim_dt, PlanView<R>{N, timestamps, ts_stride, P, strideP, V, strideV, A, strideA}, time, \
                             pos, vel, att, omega, onboard_state, depth, ring, ring_time, latency_state, wind, wind_stride, gust_step, \
                             gust_wind, log_state, log_cmd, log_time, log_target, log_delayed_time, zero_thrust_steps, stream);      \
  }

SE3MPC_DEFINE_EDGE_API(f32, float)
SE3MPC_DEFINE_EDGE_API(f64, double)
