// smoother_device.hpp -- device code of the reference's TrajectorySmoother ("smoother.py" = src/dart_planner/control/trajectory_smoother.py),
// one drone per lane: the stage between planner and controller of the reference's edge loop (edge/main_improved.py:96-152).
// INCLUDE UNDER `#pragma clang fp contract(off)`: the transition thresholds, the clamps and the filter bypass compare against values NumPy
// forms without FMA (see smoother.hip).  All clock arithmetic is double in both precisions; everything per axis is R.
#pragma once
#include "closed_loop_device.hpp"

static_assert(sizeof(se3mpc_smoother_params) == 88, "se3mpc_smoother_params is part of the C ABI (capi.py mirrors it)");

namespace se3mpc {

template <typename R>
struct SmoothDev {
  double transition_time, timeout, decay_rate, decay_cap;   // clock side
  R velocity_limit, acceleration_limit, jerk_limit, dt, vel_step, acc_step, alpha, one_minus_alpha, trans_T, trans_T2, pos_thr, vel_thr;
};

template <typename R>
static SmoothDev<R> make_smooth_dev(const se3mpc_smoother_params& p) {
  SmoothDev<R> d;
  d.transition_time = p.transition_time; d.timeout = p.timeout; d.decay_rate = p.decay_rate; d.decay_cap = p.decay_cap;
  d.velocity_limit = (R)p.velocity_limit; d.acceleration_limit = (R)p.acceleration_limit; d.jerk_limit = (R)p.jerk_limit;
  d.dt = (R)p.update_dt;
  d.vel_step = (R)(p.velocity_limit * p.update_dt);                              // smoother.py:71 velocity_limit * dt
  d.acc_step = (R)(p.acceleration_limit * p.update_dt);                          // :79
  const double alpha = p.update_dt / p.smoothing_window < 1.0 ? p.update_dt / p.smoothing_window : 1.0;   // :101
  d.alpha = (R)alpha; d.one_minus_alpha = (R)(1.0 - alpha);
  d.trans_T = (R)p.transition_time; d.trans_T2 = (R)(p.transition_time * p.transition_time);   // :291, :293
  d.pos_thr = (R)p.pos_diff_threshold; d.vel_thr = (R)p.vel_diff_threshold;
  return d;
}

// The mutable members of TrajectorySmoother (smoother.py:28-46) in registers -- all but the four transition end points (words 9..20), which
// only update_trajectory writes and only a running transition reads: they stay in the drone's record and are read there (`tr`), which keeps
// 24 registers of the float64 loop free for the controller.  In memory: double[SE3MPC_SMOOTHER_STATE_WORDS] per drone.
enum { SM_HAS_TRAJECTORY = 1, SM_IN_TRANSITION = 2 };
enum { SB_FAILSAFE = 0, SB_TRANSITION = 1, SB_TRANSITION_DONE = 2, SB_NORMAL = 3, SB_NO_TRAJECTORY = 4 };

template <typename R>
struct SmoothRegs {
  R f[9];            // last_filtered_pos, _vel, _acc
  double transition_start, last_cloud_update, trajectory_start;
  int bits;
};

template <typename R>
__device__ __forceinline__ SmoothRegs<R> load_smooth(const double* __restrict__ s) {
  SmoothRegs<R> r;
  for (int i = 0; i < 9; ++i) r.f[i] = (R)s[i];
  r.transition_start = s[21]; r.last_cloud_update = s[22]; r.trajectory_start = s[23]; r.bits = (int)s[24];
  return r;
}
template <typename R>
__device__ __forceinline__ void store_smooth(double* __restrict__ s, const SmoothRegs<R>& r) {
  for (int i = 0; i < 9; ++i) s[i] = (double)r.f[i];
  s[21] = r.transition_start; s[22] = r.last_cloud_update; s[23] = r.trajectory_start; s[24] = (double)r.bits;
}

// TrajectorySmoother._interpolate_trajectory (smoother.py:215-278), NOT the onboard sampler: stamps relative to ts[0] (:225), tt =
// current_time - start_time (:219), the first / last row at or outside the ends (:228-253), else idx = searchsorted(.) - 1 and the blend
// (1 - alpha) * row[idx] + alpha * row[idx + 1] (:256-276) -- a different rounding from sample_plan's r1 + f * (r2 - r1).  PlanCursor as there:
// c.idx = searchsorted(ts - ts[0], tt) of an earlier tt of the same plan, c.t1 / c.t2 the RELATIVE stamps of the cached rows.
// N = 0, or a plan that is not there: zeros (:221-222).  out = (pos, vel, acc) [9].
template <typename R>
__device__ __forceinline__ void sample_plan_smoother(double tt, int N, const double* __restrict__ ts, const R* __restrict__ P,
                                                     const R* __restrict__ V, const R* __restrict__ A, R out[9], PlanCursor<R>& c) {
  if (N <= 0 || ts == nullptr || P == nullptr) {                                  // :221-222
    for (int i = 0; i < 9; ++i) out[i] = (R)0;
    return;
  }
  const double ts0 = ts[0];
  int idx = c.idx;                                                                // np.searchsorted(ts - ts[0], tt): first i with ts[i] - ts[0] >= tt
  while (idx < N && ts[idx] - ts0 < tt) ++idx;
  c.idx = idx;
  if (idx != c.rows_of) {
    const int i1 = idx == 0 ? 0 : (idx >= N ? N - 1 : idx - 1), i2 = idx >= N ? N - 1 : idx;
    c.t1 = ts[i1] - ts0; c.t2 = ts[i2] - ts0;                                     // :225
    for (int a = 0; a < 3; ++a) {
      c.r1[a] = P[3 * i1 + a]; c.r2[a] = P[3 * i2 + a];
      c.r1[3 + a] = V != nullptr ? V[3 * i1 + a] : (R)0; c.r2[3 + a] = V != nullptr ? V[3 * i2 + a] : (R)0;
      c.r1[6 + a] = A != nullptr ? A[3 * i1 + a] : (R)0; c.r2[6 + a] = A != nullptr ? A[3 * i2 + a] : (R)0;
    }
    c.rows_of = idx;
  }
  if (idx == 0) {                                                                 // :228-240 tt <= 0
    for (int i = 0; i < 9; ++i) out[i] = c.r1[i];
    return;
  }
  if (idx >= N - 1 && tt >= c.t2) {                                               // :241-253 tt >= the last stamp (r2 is the last row)
    for (int i = 0; i < 9; ++i) out[i] = c.r2[i];
    return;
  }
  const R al = (R)((tt - c.t1) / (c.t2 - c.t1));                                  // :257-258
  const R om = (R)1 - al;
  for (int i = 0; i < 9; ++i) out[i] = om * c.r1[i] + al * c.r2[i];               // :260-276
}

// _apply_trajectory_limits (smoother.py:64-92) then the exponential filter of _smooth_trajectory_point (:94-113); x = (pos, vel, acc) in / out.
template <typename R>
__device__ __forceinline__ void smooth_point(const SmoothDev<R>& d, SmoothRegs<R>& s, R x[9]) {
  R ch[3];
  for (int i = 0; i < 3; ++i) ch[i] = x[3 + i] - s.f[3 + i];                      // :68
  R mag = norm3(ch);                                                              // :69
  if (mag > d.vel_step)                                                           // :71
    for (int i = 0; i < 3; ++i) x[3 + i] = s.f[3 + i] + (ch[i] * d.vel_step) / mag;   // :72-73
  for (int i = 0; i < 3; ++i) ch[i] = x[6 + i] - s.f[6 + i];                      // :76
  mag = norm3(ch);                                                                // :77
  if (mag > d.acc_step)                                                           // :79
    for (int i = 0; i < 3; ++i) x[6 + i] = s.f[6 + i] + (ch[i] * d.acc_step) / mag;   // :80-81
  for (int i = 0; i < 3; ++i) ch[i] = (x[6 + i] - s.f[6 + i]) / d.dt;             // :84-85 (dt > 0: an argument rule)
  mag = norm3(ch);                                                                // :86
  if (mag > d.jerk_limit)                                                         // :88
    for (int i = 0; i < 3; ++i) x[6 + i] = s.f[6 + i] + ((ch[i] * d.jerk_limit) / mag) * d.dt;   // :89-90
  if (norm3(s.f) > (R)0)                                                          // :103 "not first iteration": a filtered position at the exact origin is not smoothed
    for (int i = 0; i < 9; ++i) x[i] = d.alpha * x[i] + d.one_minus_alpha * s.f[i];   // :104-106
  for (int i = 0; i < 9; ++i) s.f[i] = x[i];                                      // :109-111
}

// _generate_transition_state (smoother.py:280-319) at `progress` (double: a clock quantity; the polynomial is per-axis arithmetic in R).
// tr = words 9..20 of the drone's record: transition_start_pos, _start_vel, _target_pos, _target_vel.
template <typename R>
__device__ __forceinline__ void transition_state(const SmoothDev<R>& d, const double* __restrict__ tr, double progress, R x[9]) {
  const R t = (R)fmin(fmax(progress, 0.0), 1.0);                                  // :285
  const R t2 = t * t, t3 = t2 * t, t4 = t3 * t, t5 = t4 * t;
  const R sb = ((R)10 * t3 - (R)15 * t4) + (R)6 * t5;                             // :288
  const R sd = (((R)30 * t2 - (R)60 * t3) + (R)30 * t4) / d.trans_T;              // :289-291
  const R sdd = (((R)60 * t - (R)180 * t2) + (R)120 * t3) / d.trans_T2;           // :292-294
  const R om = (R)1 - sb;
  R v[3], a[3];
  for (int i = 0; i < 3; ++i) {
    const R sp = (R)tr[i], sv = (R)tr[3 + i], tp = (R)tr[6 + i], tv = (R)tr[9 + i];
    const R pd = tp - sp;                                                         // :300
    x[i] = om * sp + sb * tp;                                                     // :297
    v[i] = (om * sv + sb * tv) + sd * pd;                                         // :301-305
    a[i] = sdd * pd;                                                              // :308
  }
  const R vn = norm3(v);                                                          // :311
  if (vn > d.velocity_limit) { const R f = d.velocity_limit / vn; for (int i = 0; i < 3; ++i) v[i] = v[i] * f; }   // :312-313
  const R an = norm3(a);                                                          // :315
  if (an > d.acceleration_limit) { const R f = d.acceleration_limit / an; for (int i = 0; i < 3; ++i) a[i] = a[i] * f; }   // :316-317
  for (int i = 0; i < 3; ++i) { x[3 + i] = v[i]; x[6 + i] = a[i]; }
}

// update_trajectory (smoother.py:115-165) at the clock `now` in two parts, because its ONLY read of the plan being followed is one sample at
// (now, trajectory_start_time): a loop that keeps one plan per drone takes that sample before the planner overwrites the plan and hands the
// nine values to the second part (monte_carlo_staged.hip).
// (a) smoother.py:134-140: the plan being followed at the clock `now` -> cur = (pos, vel, acc) [9].  Reads the record, changes nothing.
template <typename R>
__device__ __forceinline__ void smoother_sample_followed(const SmoothRegs<R>& s, double now, int N_old, const double* ts_old, const R* P_old,
                                                         const R* V_old, const R* A_old, R cur[9]) {
  PlanCursor<R> c;
  cursor_reset(c);
  sample_plan_smoother<R>(now - s.trajectory_start, N_old, ts_old, P_old, V_old, A_old, cur, c);   // :134-140
}
// (b) the rest: the first-plan rule (`cur` is not read then), the new plan sampled at (now, now), the thresholds, the record.
template <typename R>
__device__ __forceinline__ void smoother_take_plan(const SmoothDev<R>& d, SmoothRegs<R>& s, double now, const R cur[9], int N_new,
                                                   const double* ts_new, const R* P_new, const R* V_new, const R* A_new,
                                                   double* __restrict__ tr) {
  s.last_cloud_update = now;                                                      // :123
  if (!(s.bits & SM_HAS_TRAJECTORY)) {                                            // :125-131 the first plan is taken as it stands
    s.bits = SM_HAS_TRAJECTORY;
    s.trajectory_start = now;
    return;
  }
  R nw[9];
  PlanCursor<R> c;
  cursor_reset(c);
  sample_plan_smoother<R>(now - now, N_new, ts_new, P_new, V_new, A_new, nw, c);                   // :143-145
  R dp[3], dv[3];
  for (int i = 0; i < 3; ++i) { dp[i] = nw[i] - cur[i]; dv[i] = nw[3 + i] - cur[3 + i]; }
  if (norm3(dp) > d.pos_thr || norm3(dv) > d.vel_thr) {                           // :148-151
    s.bits |= SM_IN_TRANSITION;                                                   // :153
    s.transition_start = now;                                                     // :154
    for (int i = 0; i < 6; ++i) { tr[i] = (double)cur[i]; tr[6 + i] = (double)nw[i]; }   // :155-158
  }                                                                               // (a small difference leaves a running transition running)
  s.trajectory_start = now;                                                       // :165
}
// update_trajectory with both plans in memory: (a) for a drone that follows a plan, then (b).
template <typename R>
__device__ __forceinline__ void smoother_update(const SmoothDev<R>& d, SmoothRegs<R>& s, double now, int N_old, const double* ts_old, const R* P_old,
                                                const R* V_old, const R* A_old, int N_new, const double* ts_new, const R* P_new,
                                                const R* V_new, const R* A_new, double* __restrict__ tr) {
  R cur[9];
  if (s.bits & SM_HAS_TRAJECTORY) smoother_sample_followed<R>(s, now, N_old, ts_old, P_old, V_old, A_old, cur);
  smoother_take_plan<R>(d, s, now, cur, N_new, ts_new, P_new, V_new, A_new, tr);
}

// get_desired_state (smoother.py:167-213) at the clock `now` for a drone at (pos, vel) -> x = (pos, vel, acc) and the branch code.
template <typename R>
__device__ __forceinline__ int smoother_desired(const SmoothDev<R>& d, SmoothRegs<R>& s, const double* __restrict__ tr, double now, const R pos[3], const R vel[3], int N,
                                                const double* ts, const R* P, const R* V, const R* A, PlanCursor<R>& cur, R x[9]) {
  const double age = now - s.last_cloud_update;
  if (age > d.timeout) {                                                          // :176 -> _get_failsafe_trajectory (:321-338): unfiltered
    const R decay = (R)exp(-d.decay_rate * fmin(age - d.timeout, d.decay_cap));   // :330-332
    const R neg_rate = (R)(-d.decay_rate);
    for (int i = 0; i < 3; ++i) {
      x[i] = pos[i];                                                              // :326
      x[3 + i] = vel[i] * decay;                                                  // :333
      x[6 + i] = neg_rate * x[3 + i];                                             // :336
    }
    return SB_FAILSAFE;
  }
  int branch = SB_NORMAL;
  if (s.bits & SM_IN_TRANSITION) {                                                // :182
    const double progress = (now - s.transition_start) / d.transition_time;       // :183-185
    if (progress >= 1.0) {                                                        // :187-189
      s.bits &= ~SM_IN_TRANSITION;
      branch = SB_TRANSITION_DONE;
    } else {
      transition_state<R>(d, tr, progress, x);                                    // :192
      smooth_point<R>(d, s, x);                                                   // :195
      return SB_TRANSITION;
    }
  }
  if (s.bits & SM_HAS_TRAJECTORY) {                                               // :201
    sample_plan_smoother<R>(now - s.trajectory_start, N, ts, P, V, A, x, cur);    // :202-204
    smooth_point<R>(d, s, x);                                                     // :207
    return branch;
  }
  for (int i = 0; i < 3; ++i) { x[i] = pos[i]; x[3 + i] = (R)0; x[6 + i] = (R)0; }   // :213
  return SB_NO_TRAJECTORY;
}

// The command of one smoothed step of one drone (edge/main_improved.py:129-136): get_desired_state at the drone's clock, the geometric
// controller on it with yaw = yaw rate = 0.  -> the command (th, tq); target_row: null, or where the desired state [9] is logged.
// flight_command (closed_loop_device.hpp) with the smoother in the sampler's place.  Left to the inliner, like control_step.
template <typename R>
__device__ inline void smoothed_command(const SmoothDev<R>& d, const CtrlDev<R>& c, SmoothRegs<R>& sm, const double* tr,
                                                 CtrlRegs<R>& s, PlanCursor<R>& cur, int N, const double* ts, const R* P, const R* V, const R* A,
                                                 const R p[3], const R v[3], const R a[3], const R w[3], double t, double sim_dt, R& th, R tq[3],
                                                 R* target_row) {
  R x[9];
  cursor_before_step(cur, sim_dt);
  smoother_desired<R>(d, sm, tr, t, p, v, N, ts, P, V, A, cur, x);                // main_improved.py:129
  if (target_row != nullptr) for (int i = 0; i < 9; ++i) target_row[i] = x[i];
  int fl;
  control_step<R>(c, s, t, p, v, a, w, x, x + 3, x + 6, (R)0, (R)0, th, tq, fl);  // main_improved.py:134-136
}

// One smoothed step of one drone: smoothed_command, the simulator step under the command (main_improved.py:139).
// The step of se3mpc_closed_loop_smoothed_* (through lane_loop) and of se3mpc_monte_carlo_staged_* with the smoother alone: one definition,
// hence the same bits.
template <typename R>
__device__ inline void smoothed_step(const SmoothDev<R>& d, const CtrlDev<R>& c, const SimDev<R>& m, SmoothRegs<R>& sm,
                                              const double* tr, CtrlRegs<R>& s, PlanCursor<R>& cur, int N, const double* ts,
                                              const R* P, const R* V, const R* A, R p[3], R v[3], R a[3], R w[3], double& t, R dt, double sim_dt,
                                              const R wd[3], R& th, R tq[3], R* target_row) {
  smoothed_command<R>(d, c, sm, tr, s, cur, N, ts, P, V, A, p, v, a, w, t, sim_dt, th, tq, target_row);
  simulator_step<R>(m, p, v, a, w, t, th, tq, dt, sim_dt, wd);
}

static inline int check_smoother_params(const se3mpc_smoother_params* p) {
  if (p == nullptr) return SE3MPC_ERR_NULL;
  // the three divisors; a limit or threshold may be infinite (it then never fires)
  if (!std::isfinite(p->transition_time) || !std::isfinite(p->update_dt) || !std::isfinite(p->smoothing_window) || !(p->transition_time > 0.0) ||
      !(p->update_dt > 0.0) || !(p->smoothing_window > 0.0))
    return SE3MPC_ERR_PARAM;
  return SE3MPC_OK;
}

}  // namespace se3mpc
