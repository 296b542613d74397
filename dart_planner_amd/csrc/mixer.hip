// mixer.hip -- the reference's MotorMixer and motor model on the device, one drone per lane: the stage between the
// controller's (thrust, torque) and the actuators in both of its hardware back ends (hardware/pixhawk_interface.py:451-492,
// hardware/airsim_interface.py:157-191).
//
// Reference arithmetic ("mixer.py" = src/dart_planner/hardware/motor_mixer.py, "model.py" = src/dart_planner/hardware/motor_model.py),
// reproduced with its quirks:
//   * mix_commands             mixer.py:168-260, model.py:219-258      se3mpc_mixer_mix_*  (and pixhawk_interface.py:473-487, :413)
//   * the forward model        model.py:166-217, :260-282              se3mpc_mixer_readback_*
//   * get_control_allocation   mixer.py:262-279 (the INVERSE matrix on the motor thrusts)
//   * the actuated loop        desired state -> compute_control -> mix_commands -> the motors' wrench B @ F -> DroneSimulator.step, `nsteps`
//                              times in ONE launch: se3mpc_closed_loop_actuated_* (lane_loop / control_step / simulator_step)
//
// Contraction is off in this file for the reason it is off in closed_loop.hip: `thrust <= 0`, `disc < 0`, the allclose threshold of the
// saturation counter, the 1.1 overrun and the all-idle test compare against values NumPy forms without FMA.
#pragma clang fp contract(off)
#include <limits>

#include "smoother_device.hpp"
#include "mixer_device.hpp"

namespace se3mpc {

__global__ void __launch_bounds__(64)
mixer_reset_kernel(int B, double* __restrict__ state) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  double* s = state + (size_t)b * SE3MPC_MIXER_STATE_WORDS;
  for (int i = 0; i < SE3MPC_MIXER_STATE_WORDS; ++i) s[i] = 0.0;                  // mixer.py:144-145
}

template <typename R>
__global__ void __launch_bounds__(64)
mixer_mix_kernel(MixDev<R> d, int B, const R* __restrict__ thrust, const R* __restrict__ torque, double* __restrict__ state,
                 R* __restrict__ pwm, int32_t* __restrict__ flags, R* __restrict__ body_rate) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  MixRegs<R> s;
  if (state != nullptr) s = load_mix<R>(state + (size_t)b * SE3MPC_MIXER_STATE_WORDS);
  else { s.events = 0; s.last[0] = s.last[1] = s.last[2] = s.last[3] = (R)0; }
  const R th = thrust[b], tq[3] = {torque[3 * b], torque[3 * b + 1], torque[3 * b + 2]};
  R p[4];
  const int fl = mix_step<R>(d, s, th, tq, p);
  if (state != nullptr && !(fl & MF_NON_FINITE)) store_mix<R>(state + (size_t)b * SE3MPC_MIXER_STATE_WORDS, s);
  for (int i = 0; i < 4; ++i) pwm[4 * b + i] = p[i];
  if (flags != nullptr) flags[b] = fl;
  if (body_rate != nullptr) {
    R br[4];
    body_rate_command<R>(d, th, p, br);
    for (int i = 0; i < 4; ++i) body_rate[4 * b + i] = br[i];
  }
}

template <typename R>
__global__ void __launch_bounds__(64)
mixer_readback_kernel(MixDev<R> d, int B, const R* __restrict__ pwm, const R* __restrict__ motor_health, long long health_stride,
                      R* __restrict__ motor_thrust, R* __restrict__ motor_torque, R* __restrict__ motor_rpm, R* __restrict__ allocation,
                      R* __restrict__ wrench) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const R p[4] = {pwm[4 * b], pwm[4 * b + 1], pwm[4 * b + 2], pwm[4 * b + 3]};
  R F[4], Q[4], rpm[4], o[4];
  motors_realised<R>(d, p, motor_health != nullptr ? motor_health + (size_t)b * health_stride : nullptr, F, Q, rpm);
  if (motor_thrust != nullptr) for (int i = 0; i < 4; ++i) motor_thrust[4 * b + i] = F[i];
  if (motor_torque != nullptr) for (int i = 0; i < 4; ++i) motor_torque[4 * b + i] = Q[i];
  if (motor_rpm != nullptr) for (int i = 0; i < 4; ++i) motor_rpm[4 * b + i] = rpm[i];
  if (allocation != nullptr) {
    control_allocation<R>(d, F, o);
    for (int i = 0; i < 4; ++i) allocation[4 * b + i] = o[i];
  }
  if (wrench != nullptr) {
    realised_wrench<R>(d, F, o);
    for (int i = 0; i < 4; ++i) wrench[4 * b + i] = o[i];
  }
}

// ---- nsteps x (desired state, compute_control, mix_commands, the motors' wrench, DroneSimulator.step) per drone in one launch: lane_loop,
// as se3mpc_closed_loop_smoothed_*; SMOOTH = false: the raw plan sample of flight_step in place of get_desired_state.  log_cmd keeps the
// COMMAND; the simulator runs under what the motors deliver.
template <typename R, bool SMOOTH>
__global__ void __launch_bounds__(64)
closed_loop_actuated_kernel(SmoothDev<R> d, CtrlDev<R> c, SimDev<R> m, MixDev<R> x, int B, int nsteps, double sim_dt, PlanView<R> plan,
                            double* __restrict__ time, R* __restrict__ pos, R* __restrict__ vel, R* __restrict__ att, R* __restrict__ omega,
                            double* __restrict__ state, double* __restrict__ smoother_state, double* __restrict__ mixer_state,
                            const R* __restrict__ motor_health, long long health_stride, const R* __restrict__ wind, long long wind_stride,
                            int gust_step, R gx, R gy, R gz, R* __restrict__ log_state, R* __restrict__ log_cmd, double* __restrict__ log_time,
                            R* __restrict__ log_target, R* __restrict__ log_pwm, R* __restrict__ log_wrench) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  CtrlRegs<R> s = load_ctrl<R>(state + (size_t)b * SE3MPC_CONTROLLER_STATE_WORDS);
  MixRegs<R> mx = load_mix<R>(mixer_state + (size_t)b * SE3MPC_MIXER_STATE_WORDS);
  SmoothRegs<R> sm;
  if (SMOOTH) sm = load_smooth<R>(smoother_state + (size_t)b * SE3MPC_SMOOTHER_STATE_WORDS);
  R health[4] = {(R)1, (R)1, (R)1, (R)1};
  if (motor_health != nullptr) for (int i = 0; i < 4; ++i) health[i] = motor_health[(size_t)b * health_stride + i];
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
    const size_t row = (size_t)step * B + b;
    actuated_step<R, SMOOTH>(d, c, m, x, sm, SMOOTH ? smoother_state + (size_t)b * SE3MPC_SMOOTHER_STATE_WORDS + 9 : nullptr, s, mx,
                             motor_health != nullptr ? health : (const R*)nullptr, cur, N, ts, Pb, Vb, Ab, dr.p, dr.v, dr.a, dr.w, dr.t, dt, sim_dt,
                             dr.wd, th, tq, log_target != nullptr ? log_target + row * 9 : nullptr, log_pwm != nullptr ? log_pwm + row * 4 : nullptr,
                             log_wrench != nullptr ? log_wrench + row * 4 : nullptr);
  });
  dr.store(b, pos, vel, att, omega, time);
  store_ctrl<R>(state + (size_t)b * SE3MPC_CONTROLLER_STATE_WORDS, s);
  store_mix<R>(mixer_state + (size_t)b * SE3MPC_MIXER_STATE_WORDS, mx);
  if (SMOOTH) store_smooth<R>(smoother_state + (size_t)b * SE3MPC_SMOOTHER_STATE_WORDS, sm);
}

template <typename R>
int mixer_mix_impl(const se3mpc_mixer_params* mp, int B, const R* thrust, const R* torque, double* state, R* pwm, int32_t* flags,
                   R* body_rate, void* stream) {
  int rc = check_mixer_params(mp);
  if (rc) return reject(rc, "se3mpc_mixer_mix: mixer parameters");
  if (B < 0) return reject(SE3MPC_ERR_SHAPE, "se3mpc_mixer_mix: B < 0");
  if (B == 0) return SE3MPC_OK;
  if (!thrust || !torque || !pwm) return reject(SE3MPC_ERR_NULL, "se3mpc_mixer_mix: thrust / torque / pwm");
  hipLaunchKernelGGL(mixer_mix_kernel<R>, dim3(grid_for(B, 64)), dim3(64), 0, (hipStream_t)stream, make_mix_dev<R>(*mp), B, thrust, torque, state,
                     pwm, flags, body_rate);
  return launch_status("se3mpc_mixer_mix");
}

template <typename R>
int mixer_readback_impl(const se3mpc_mixer_params* mp, int B, const R* pwm, const R* motor_health, long long health_stride, R* motor_thrust,
                        R* motor_torque, R* motor_rpm, R* allocation, R* wrench, void* stream) {
  int rc = check_mixer_params(mp);
  if (rc) return reject(rc, "se3mpc_mixer_readback: mixer parameters");
  if (B < 0 || health_stride < 0) return reject(SE3MPC_ERR_SHAPE, "se3mpc_mixer_readback: B / health_stride < 0");
  if (B == 0) return SE3MPC_OK;
  if (!pwm) return reject(SE3MPC_ERR_NULL, "se3mpc_mixer_readback: pwm");
  hipLaunchKernelGGL(mixer_readback_kernel<R>, dim3(grid_for(B, 64)), dim3(64), 0, (hipStream_t)stream, make_mix_dev<R>(*mp), B, pwm, motor_health,
                     health_stride, motor_thrust, motor_torque, motor_rpm, allocation, wrench);
  return launch_status("se3mpc_mixer_readback");
}

template <typename R>
int closed_loop_actuated_impl(const se3mpc_smoother_params* sm, const se3mpc_controller_params* cp, const se3mpc_simulator_params* sp,
                              const se3mpc_mixer_params* mp, int B, int nsteps, double sim_dt, const PlanView<R>& plan, double* time, R* pos,
                              R* vel, R* att, R* omega, double* state, double* smoother_state, double* mixer_state, const R* motor_health,
                              long long health_stride, const R* wind, long long wind_stride, int gust_step, const double* gust_wind,
                              R* log_state, R* log_cmd, double* log_time, R* log_target, R* log_pwm, R* log_wrench, void* stream) {
  if ((sm == nullptr) != (smoother_state == nullptr))
    return reject(SE3MPC_ERR_NULL, "se3mpc_closed_loop_actuated: smoother parameters and smoother_state come together or not at all");
  const bool smooth = sm != nullptr;
  int rc = smooth ? check_smoother_params(sm) : SE3MPC_OK;
  if (rc) return reject(rc, "se3mpc_closed_loop_actuated: smoother parameters");
  rc = check_controller_params(cp);
  if (rc) return reject(rc, "se3mpc_closed_loop_actuated: controller parameters");
  rc = check_simulator_params(sp);
  if (rc) return reject(rc, "se3mpc_closed_loop_actuated: simulator parameters");
  rc = check_mixer_params(mp);
  if (rc) return reject(rc, "se3mpc_closed_loop_actuated: mixer parameters");
  if (!std::isfinite(sim_dt)) return reject(SE3MPC_ERR_PARAM, "se3mpc_closed_loop_actuated: sim_dt");
  if (B < 0 || nsteps < 0 || wind_stride < 0 || health_stride < 0)
    return reject(SE3MPC_ERR_SHAPE, "se3mpc_closed_loop_actuated: B / nsteps / wind_stride / health_stride < 0");
  // with the smoother a plan may be empty (it samples zeros); the raw sampler reads row N - 1
  if (!plan_shape_ok(plan, smooth ? 0 : 1)) return reject(SE3MPC_ERR_SHAPE, "se3mpc_closed_loop_actuated: plan");
  if (!plan_present(plan)) return reject(SE3MPC_ERR_NULL, "se3mpc_closed_loop_actuated: plan");
  if (B == 0 || nsteps == 0) return SE3MPC_OK;
  if (!time || !pos || !vel || !att || !omega || !state || !mixer_state || (gust_step >= 0 && !gust_wind))
    return reject(SE3MPC_ERR_NULL, "se3mpc_closed_loop_actuated: a required operand is NULL");
  const R gx = gust_step >= 0 ? (R)gust_wind[0] : (R)0, gy = gust_step >= 0 ? (R)gust_wind[1] : (R)0, gz = gust_step >= 0 ? (R)gust_wind[2] : (R)0;
  se3mpc_smoother_params none;
  se3mpc_smoother_default_params(&none);                                          // SMOOTH = false never reads it
  const SmoothDev<R> sd = make_smooth_dev<R>(smooth ? *sm : none);
  if (smooth)
    hipLaunchKernelGGL((closed_loop_actuated_kernel<R, true>), dim3(grid_for(B, 64)), dim3(64), 0, (hipStream_t)stream, sd, make_ctrl_dev<R>(*cp),
                       make_sim_dev<R>(*sp), make_mix_dev<R>(*mp), B, nsteps, sim_dt, plan, time, pos, vel, att, omega, state, smoother_state,
                       mixer_state, motor_health, health_stride, wind, wind_stride, gust_step, gx, gy, gz, log_state, log_cmd, log_time,
                       log_target, log_pwm, log_wrench);
  else
    hipLaunchKernelGGL((closed_loop_actuated_kernel<R, false>), dim3(grid_for(B, 64)), dim3(64), 0, (hipStream_t)stream, sd, make_ctrl_dev<R>(*cp),
                       make_sim_dev<R>(*sp), make_mix_dev<R>(*mp), B, nsteps, sim_dt, plan, time, pos, vel, att, omega, state, smoother_state,
                       mixer_state, motor_health, health_stride, wind, wind_stride, gust_step, gx, gy, gz, log_state, log_cmd, log_time,
                       log_target, log_pwm, log_wrench);
  return launch_status("se3mpc_closed_loop_actuated");
}

// B X = I by LU with partial pivoting (what np.linalg.solve does for the regular matrix of the X layout); false: a zero pivot
static bool invert4(const double* Bm, double* X) {
  double a[4][8];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) { a[i][j] = Bm[4 * i + j]; a[i][4 + j] = i == j ? 1.0 : 0.0; }
  int perm[4] = {0, 1, 2, 3};
  for (int k = 0; k < 4; ++k) {
    int piv = k;
    for (int i = k + 1; i < 4; ++i)
      if (std::fabs(a[perm[i]][k]) > std::fabs(a[perm[piv]][k])) piv = i;
    std::swap(perm[k], perm[piv]);
    const double p = a[perm[k]][k];
    if (p == 0.0) return false;
    for (int i = k + 1; i < 4; ++i) {
      const double l = a[perm[i]][k] / p;
      for (int j = k; j < 8; ++j) a[perm[i]][j] -= l * a[perm[k]][j];
    }
  }
  for (int c = 0; c < 4; ++c)
    for (int i = 3; i >= 0; --i) {
      double v = a[perm[i]][4 + c];
      for (int j = i + 1; j < 4; ++j) v -= a[perm[i]][j] * X[4 * j + c];
      X[4 * i + c] = v / a[perm[i]][i];
    }
  return true;
}

}  // namespace se3mpc

using namespace se3mpc;

extern "C" int se3mpc_mixer_default_params(se3mpc_mixer_params* out) {
  if (out == nullptr) return SE3MPC_ERR_NULL;
  se3mpc_mixer_params d;
  const double arm = 0.15, x = arm * 0.707;                                       // create_x_configuration_mixer(0.15), mixer.py:411-421
  const double px[4] = {x, x, -x, -x}, py[4] = {-x, x, x, -x}, dir[4] = {1.0, -1.0, 1.0, -1.0};
  for (int i = 0; i < 4; ++i) {                                                   // create_default_motor_model, model.py:394-435; limits :46-48
    d.thrust_a[i] = 2.5; d.thrust_b[i] = 1.2; d.thrust_c[i] = 0.1;
    d.pwm_min[i] = 0.0; d.pwm_max[i] = 1.0; d.pwm_idle[i] = 0.1;
    d.torque_coefficient[i] = 1e-7; d.rpm_coefficient[i] = 8000.0; d.rpm_offset[i] = 500.0;
  }
  d.config_pwm_min = 0.0; d.config_pwm_max = 1.0; d.config_pwm_idle = 0.1;        // mixer.py:64-66
  d.max_thrust = 10.0; d.body_rate_scale = 2.0; d.watchdog_threshold = 5.0;       // pixhawk_interface.py config, :482, :413
  for (int i = 0; i < 4; ++i) {                                                   // _compute_mixing_matrix, mixer.py:379-398, at config.pwm_max
    const double p = std::fmin(std::fmax(d.config_pwm_max, d.pwm_min[i]), d.pwm_max[i]);
    const double th = std::fmax(0.0, (d.thrust_a[i] * (p * p) + d.thrust_b[i] * p) + d.thrust_c[i]);
    const double rpm = std::fmax(0.0, d.rpm_coefficient[i] * p + d.rpm_offset[i]);
    const double tq = std::fmax(0.0, d.torque_coefficient[i] * (rpm * rpm));
    const double k_drag = th > 0.0 ? tq / th : 0.0;
    d.mixing[0 + i] = 1.0; d.mixing[4 + i] = py[i]; d.mixing[8 + i] = px[i]; d.mixing[12 + i] = dir[i] * k_drag;
  }
  if (!invert4(d.mixing, d.inverse)) return reject(SE3MPC_ERR_PARAM, "se3mpc_mixer_default_params: singular mixing matrix");
  *out = d;
  return SE3MPC_OK;
}

extern "C" int se3mpc_mixer_reset(int B, double* state, void* stream) {
  if (B < 0) return reject(SE3MPC_ERR_SHAPE, "se3mpc_mixer_reset: B < 0");
  if (B == 0) return SE3MPC_OK;
  if (!state) return reject(SE3MPC_ERR_NULL, "se3mpc_mixer_reset: state");
  hipLaunchKernelGGL(mixer_reset_kernel, dim3(grid_for(B, 64)), dim3(64), 0, (hipStream_t)stream, B, state);
  return launch_status("se3mpc_mixer_reset");
}

#define SE3MPC_DEFINE_MIXER_API(SUF, R)                                                                                             \
  extern "C" int se3mpc_mixer_mix_##SUF(const se3mpc_mixer_params* mp, int B, const R* thrust, const R* torque, double* state, R* pwm, \
                                        int32_t* flags, R* body_rate, void* stream) {                                               \
    return mixer_mix_impl<R>(mp, B, thrust, torque, state, pwm, flags, body_rate, stream);                                          \
  }                                                                                                                                 \
  extern "C" int se3mpc_mixer_readback_##SUF(const se3mpc_mixer_params* mp, int B, const R* pwm, const R* motor_health,               \
                                             long long health_stride, R* motor_thrust, R* motor_torque, R* motor_rpm, R* allocation, \
                                             R* wrench, void* stream) {                                                             \
    return mixer_readback_impl<R>(mp, B, pwm, motor_health, health_stride, motor_thrust, motor_torque, motor_rpm, allocation, wrench, \
                                  stream);                                                                                          \
  }                                                                                                                                 \
  extern "C" int se3mpc_closed_loop_actuated_##SUF(                                                                                 \
      const se3mpc_smoother_params* sm, const se3mpc_controller_params* cp, const se3mpc_simulator_params* sp,                        \
      const se3mpc_mixer_params* mp, int B, int nsteps, double sim_dt, int N, const double* timestamps, long long ts_stride, const R* P, \
      long long strideP, const R* V, long long strideV, const R* A, long long strideA, double* time, R* pos, R* vel, R* att, R* omega, \
      double* state, double* smoother_state, double* mixer_state, const R* motor_health, long long health_stride, const R* wind,    \
      long long wind_stride, int gust_step, const double* gust_wind, R* log_state, R* log_cmd, double* log_time, R* log_target,     \
      R* log_pwm, R* log_wrench, void* stream) {                                                                                    \
    return closed_loop_actuated_impl<R>(sm, cp, sp, mp, B, nsteps, sim_dt,                                                          \
                                        PlanView<R>{N, timestamps, ts_stride, P, strideP, V, strideV, A, strideA}, time, pos, vel,  \
                                        att, omega, state, smoother_state, mixer_state, motor_health, health_stride, wind,          \
                                        wind_stride, gust_step, gust_wind, log_state, log_cmd, log_time, log_target, log_pwm,       \
                                        log_wrench, stream);                                                                        \
  }

SE3MPC_DEFINE_MIXER_API(f32, float)
SE3MPC_DEFINE_MIXER_API(f64, double)
