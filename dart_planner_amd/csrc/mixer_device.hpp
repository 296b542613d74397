// mixer_device.hpp -- device code of the reference's MotorMixer and QuadraticMotorModel ("mixer.py" = src/dart_planner/hardware/motor_mixer.py,
// "model.py" = src/dart_planner/hardware/motor_model.py), one drone per lane: the last arithmetic stage between the controller's (thrust,
// torque) and the actuators (hardware/pixhawk_interface.py:451-492, hardware/airsim_interface.py:157-191).
// INCLUDE UNDER `#pragma clang fp contract(off)`: the `thrust <= 0` tests, the discriminant's sign, the allclose threshold of the saturation
// counter, the overrun and all-idle tests compare against values NumPy forms without FMA (see mixer.hip).
#pragma once
#include "smoother_device.hpp"

static_assert(sizeof(se3mpc_mixer_params) == 592, "se3mpc_mixer_params is part of the C ABI (capi.py mirrors it)");

namespace se3mpc {

// Per-motor branch of pwm_from_thrust, decided once on the host in double (model.py:243-245).
enum { MM_QUADRATIC = 0, MM_LINEAR = 1, MM_DEAD = 2 };
// Output flags of one mix_commands call.
enum { MF_NEGATIVE_THRUST = 1, MF_NON_FINITE = 2, MF_OVERRUN = 4, MF_SATURATION_EVENT = 8, MF_ALL_IDLE = 16, MF_WATCHDOG = 32 };

template <typename R>
struct MixDev {
  R inv[16], mix[16];                                   // inverse_matrix, mixing_matrix B (row-major)
  R a[4], b[4], c[4], pmin[4], pmax[4], pidle[4], kq[4], krpm[4], roff[4];   // the motors' own parameters
  R cmin, cmax, cidle, overrun, max_thrust, rate_scale; // the config's limits; overrun = 1.1 * config.pwm_max (mixer.py:205)
  int mode[4];
  int watchdog;                                         // saturation_events > watchdog trips (pixhawk_interface.py:413)
};

template <typename R>
static MixDev<R> make_mix_dev(const se3mpc_mixer_params& p) {
  MixDev<R> d;
  for (int i = 0; i < 16; ++i) { d.inv[i] = (R)p.inverse[i]; d.mix[i] = (R)p.mixing[i]; }
  for (int i = 0; i < 4; ++i) {
    d.a[i] = (R)p.thrust_a[i]; d.b[i] = (R)p.thrust_b[i]; d.c[i] = (R)p.thrust_c[i];
    d.pmin[i] = (R)p.pwm_min[i]; d.pmax[i] = (R)p.pwm_max[i]; d.pidle[i] = (R)p.pwm_idle[i];
    d.kq[i] = (R)p.torque_coefficient[i]; d.krpm[i] = (R)p.rpm_coefficient[i]; d.roff[i] = (R)p.rpm_offset[i];
    d.mode[i] = std::fabs(p.thrust_a[i]) < 1e-9 ? (std::fabs(p.thrust_b[i]) < 1e-9 ? MM_DEAD : MM_LINEAR) : MM_QUADRATIC;   // model.py:243-245
  }
  d.cmin = (R)p.config_pwm_min; d.cmax = (R)p.config_pwm_max; d.cidle = (R)p.config_pwm_idle;
  d.overrun = (R)(p.config_pwm_max * 1.1);                                        // mixer.py:205
  d.max_thrust = (R)p.max_thrust; d.rate_scale = (R)p.body_rate_scale;
  // events are whole numbers: events > threshold <=> events > floor(threshold)
  const double w = std::floor(p.watchdog_threshold);
  d.watchdog = w >= 2147483647.0 ? 2147483647 : (w < -1.0 ? -1 : (int)w);
  return d;
}

// The mutable members of MotorMixer (mixer.py:144-145) in registers.  In memory: double[SE3MPC_MIXER_STATE_WORDS] per drone.
template <typename R>
struct MixRegs {
  int events;
  R last[4];
};
template <typename R>
__device__ __forceinline__ MixRegs<R> load_mix(const double* __restrict__ s) {
  MixRegs<R> r;
  r.events = (int)s[0];
  for (int i = 0; i < 4; ++i) r.last[i] = (R)s[1 + i];
  return r;
}
template <typename R>
__device__ __forceinline__ void store_mix(double* __restrict__ s, const MixRegs<R>& r) {
  s[0] = (double)r.events;
  for (int i = 0; i < 4; ++i) s[1 + i] = (double)r.last[i];
}

// np.clip / np.maximum on a scalar: a NaN stays a NaN (fmin / fmax would drop it)
template <typename R>
__device__ __forceinline__ R clip_np(R x, R lo, R hi) { return x != x ? x : fmin(fmax(x, lo), hi); }
template <typename R>
__device__ __forceinline__ R maximum_np(R x, R lo) { return x != x ? x : fmax(x, lo); }
// Python's max(0.0, x) = x if x > 0.0 else 0.0: NaN -> 0.0, -0.0 -> 0.0 (model.py:190, :217, :282)
template <typename R>
__device__ __forceinline__ R max0_py(R x) { return x > (R)0 ? x : (R)0; }
// row j of a row-major 4 x 4 matrix times v, summed left to right
template <typename R>
__device__ __forceinline__ R row4(const R* __restrict__ M, int j, const R v[4]) {
  return ((M[4 * j] * v[0] + M[4 * j + 1] * v[1]) + M[4 * j + 2] * v[2]) + M[4 * j + 3] * v[3];
}

// QuadraticMotorModel.pwm_from_thrust (model.py:219-258) of motor i
template <typename R>
__device__ __forceinline__ R pwm_from_thrust(const MixDev<R>& d, int i, R thrust) {
  if (thrust <= (R)0) return d.pidle[i];                                          // :235-236 the MOTOR's idle
  R pwm;
  if (d.mode[i] != MM_QUADRATIC) {                                                // :243
    if (d.mode[i] == MM_DEAD) return d.pidle[i];                                  // :244-245
    pwm = (thrust - d.c[i]) / d.b[i];                                             // :246
  } else {
    const R disc = d.b[i] * d.b[i] - ((R)4 * d.a[i]) * (d.c[i] - thrust);         // :249
    if (disc < (R)0) return d.pmax[i];                                            // :250-252: a thrust below the curve's minimum asks for full PWM
    pwm = (-d.b[i] + sqrt(disc)) / ((R)2 * d.a[i]);                               // :255
  }
  return clip_np(pwm, d.pmin[i], d.pmax[i]);                                      // :258
}

// thrust_from_pwm, rpm_from_pwm, torque_from_pwm (model.py:166-217, :260-282) of motor i: an out-of-range PWM is clipped to the motor's limits
// (:182-183; the clip of an in-range value is the value, a NaN stays one and comes out as 0.0 through max(0.0, .))
template <typename R>
__device__ __forceinline__ void motor_forward(const MixDev<R>& d, int i, R pwm, R& thrust, R& torque, R& rpm) {
  const R p = clip_np(pwm, d.pmin[i], d.pmax[i]);
  thrust = max0_py((d.a[i] * (p * p) + d.b[i] * p) + d.c[i]);                     // :186-190
  rpm = max0_py(d.krpm[i] * p + d.roff[i]);                                       // :280-282
  torque = max0_py(d.kq[i] * (rpm * rpm));                                        // :215-217
}

// MotorMixer.mix_commands (mixer.py:168-222) for one drone -> the saturated PWMs and the call's flags.  thrust, torque: the command.
// A non-finite motor thrust (the reference raises RuntimeError, :198-199): NaN PWMs, MF_NON_FINITE, the record stays as it is.
template <typename R>
__device__ __forceinline__ int mix_step(const MixDev<R>& d, MixRegs<R>& s, R thrust, const R torque[3], R pwm[4]) {
  int flags = 0;
  if (thrust < (R)0) { thrust = (R)0; flags |= MF_NEGATIVE_THRUST; }              // :187-189
  const R cmd[4] = {thrust, torque[0], torque[1], torque[2]};                     // :192
  R F[4];
  bool finite = true;
  for (int i = 0; i < 4; ++i) {
    F[i] = row4(d.inv, i, cmd);                                                   // :195
    finite = finite && (fabs(F[i]) <= std::numeric_limits<R>::max());             // :198 (false for NaN and +-inf)
  }
  if (!finite) {
    for (int i = 0; i < 4; ++i) pwm[i] = (R)NAN;
    return flags | MF_NON_FINITE;
  }
  R raw[4], sat[4];
  bool overrun = false, event = false, all_idle = true;
  for (int i = 0; i < 4; ++i) {
    raw[i] = pwm_from_thrust(d, i, fmax(F[i], (R)0));                             // :235-240
    overrun = overrun || raw[i] > d.overrun;                                      // :205-206
    sat[i] = maximum_np(clip_np(raw[i], d.cmin, d.cmax), d.cidle);                // :255-258 the CONFIG's limits
    event = event || !(fabs(raw[i] - sat[i]) <= (R)1e-8 + (R)1e-6 * fabs(sat[i]));   // :213 not np.allclose(raw, sat, rtol=1e-6)
    all_idle = all_idle && sat[i] == d.cidle;                                     // :218
  }
  if (overrun) flags |= MF_OVERRUN;
  if (event) { s.events += 1; flags |= MF_SATURATION_EVENT; }                     // :214
  if (all_idle && thrust > (R)0.2) flags |= MF_ALL_IDLE;                          // :218-219
  for (int i = 0; i < 4; ++i) { s.last[i] = sat[i]; pwm[i] = sat[i]; }            // :221
  if (s.events > d.watchdog) flags |= MF_WATCHDOG;                                // pixhawk_interface.py:413
  return flags;
}

// _convert_to_body_rate_cmd (pixhawk_interface.py:473-487) from the command's thrust AS GIVEN and the PWMs -> (normalised thrust, body rates)
template <typename R>
__device__ __forceinline__ void body_rate_command(const MixDev<R>& d, R thrust, const R pwm[4], R out[4]) {
  out[0] = clip_np(thrust / d.max_thrust, (R)0, (R)1);                            // :473
  out[1] = ((pwm[1] + pwm[2]) - (pwm[0] + pwm[3])) * d.rate_scale;                // :477, :484
  out[2] = ((pwm[0] + pwm[1]) - (pwm[2] + pwm[3])) * d.rate_scale;                // :478, :485
  out[3] = ((pwm[0] + pwm[2]) - (pwm[1] + pwm[3])) * d.rate_scale;                // :479, :486
}

// What the motors do under the PWMs: each motor's thrust_from_pwm scaled by its health (null = 1: the fault-injection operand, which
// the mixer does not see), its torque and rpm.
template <typename R>
__device__ __forceinline__ void motors_realised(const MixDev<R>& d, const R pwm[4], const R* __restrict__ health, R F[4], R Q[4], R rpm[4]) {
  for (int i = 0; i < 4; ++i) {
    motor_forward(d, i, pwm[i], F[i], Q[i], rpm[i]);
    if (health != nullptr) F[i] = health[i] * F[i];
  }
}
// get_control_allocation (mixer.py:262-279): the INVERSE matrix on the motor thrusts, as the reference has it
template <typename R>
__device__ __forceinline__ void control_allocation(const MixDev<R>& d, const R F[4], R out[4]) {
  for (int j = 0; j < 4; ++j) out[j] = row4(d.inv, j, F);
}
// (thrust, torque) the motors deliver: B @ F.  The reference never forms it; a simulator behind the mixer needs it.
template <typename R>
__device__ __forceinline__ void realised_wrench(const MixDev<R>& d, const R F[4], R out[4]) {
  for (int j = 0; j < 4; ++j) out[j] = row4(d.mix, j, F);
}

// One actuated step of one drone: the command (smoothed_command, or SMOOTH = false: flight_command on the raw plan sample -- d, sm and tr are
// not read then), mix_commands (pixhawk_interface.py:464), what the motors deliver under the PWMs (health: null = 1), the simulator step under
// THAT wrench.  -> the COMMAND (th, tq); target_row [9], pwm_row [4], wrench_row [4]: null, or where the step's target, PWMs and delivered
// wrench are logged.
// The step of se3mpc_closed_loop_actuated_* (through lane_loop) and of se3mpc_monte_carlo_staged_* with the mixer: one definition, hence the
// same bits.  Left to the inliner, like control_step.
template <typename R, bool SMOOTH>
__device__ inline void actuated_step(const SmoothDev<R>& d, const CtrlDev<R>& c, const SimDev<R>& m, const MixDev<R>& x, SmoothRegs<R>& sm,
                                     const double* tr, CtrlRegs<R>& s, MixRegs<R>& mx, const R* health, PlanCursor<R>& cur, int N, const double* ts,
                                     const R* P, const R* V, const R* A, R p[3], R v[3], R a[3], R w[3], double& t, R dt, double sim_dt,
                                     const R wd[3], R& th, R tq[3], R* target_row, R* pwm_row, R* wrench_row) {
  if constexpr (SMOOTH) smoothed_command<R>(d, c, sm, tr, s, cur, N, ts, P, V, A, p, v, a, w, t, sim_dt, th, tq, target_row);
  else flight_command<R>(c, s, cur, N, ts, P, V, A, p, v, a, w, t, sim_dt, th, tq, target_row);
  R pw[4], F[4], Q[4], rpm[4], wr[4];
  const int mf = mix_step<R>(x, mx, th, tq, pw);                                  // pixhawk_interface.py:464
  (void)mf;
  motors_realised<R>(x, pw, health, F, Q, rpm);
  realised_wrench<R>(x, F, wr);
  if (pwm_row != nullptr) for (int i = 0; i < 4; ++i) pwm_row[i] = pw[i];
  if (wrench_row != nullptr) for (int i = 0; i < 4; ++i) wrench_row[i] = wr[i];
  simulator_step<R>(m, p, v, a, w, t, wr[0], wr + 1, dt, sim_dt, wd);
}

static inline int check_mixer_params(const se3mpc_mixer_params* p) {
  if (p == nullptr) return SE3MPC_ERR_NULL;
  const double* v = reinterpret_cast<const double*>(p);
  // the matrices may hold anything LAPACK returned for a singular B (the non-finite flag reports what comes of it); every other
  // field is finite and the watchdog threshold is no NaN
  for (size_t i = 32; i < sizeof(se3mpc_mixer_params) / sizeof(double) - 1; ++i)
    if (!std::isfinite(v[i])) return SE3MPC_ERR_PARAM;
  if (p->watchdog_threshold != p->watchdog_threshold) return SE3MPC_ERR_PARAM;
  return SE3MPC_OK;
}

}  // namespace se3mpc
