// edge_device.hpp -- device code of the reference's edge loop (edge/main.py:80-95): the latency buffer between estimator
// and controller (latency.py:34-82) and the cascaded-PID OnboardController (onboard.py:95-184, pid.py:25-51), one drone per lane.  The plan
// sampler, the simulator step, DroneRegs and lane_loop are those of closed_loop_device.hpp.
// INCLUDE UNDER `#pragma clang fp contract(off)`: the integral clamps, the thrust clip at 0 and the dt <= 0 rule compare against values
// NumPy forms without FMA.
#pragma once
#include "closed_loop_device.hpp"

static_assert(sizeof(se3mpc_onboard_params) == 216, "se3mpc_onboard_params is part of the C ABI (capi.py mirrors it)");

namespace se3mpc {

// PID rows of se3mpc_onboard_params / the record
enum { PID_X = 0, PID_Y, PID_Z, PID_ROLL, PID_PITCH, PID_YAW_RATE };

template <typename R>
struct OnboardDev {
  R mass, g, inv_g, hover;
  R kp[6], ki[6], kd[6], lim[6];
  double first_dt;
};

template <typename R>
static OnboardDev<R> make_onboard_dev(const se3mpc_onboard_params& p) {
  OnboardDev<R> c;
  c.mass = (R)p.mass; c.g = (R)p.g;
  c.inv_g = (R)1 / (R)p.g;                                                        // onboard.py:104 (1 / self.g), in the kernel's precision
  c.hover = (R)(p.mass * p.g);                                                    // :184
  for (int i = 0; i < 6; ++i) { c.kp[i] = (R)p.pid[i][0]; c.ki[i] = (R)p.pid[i][1]; c.kd[i] = (R)p.pid[i][2]; c.lim[i] = (R)p.pid[i][3]; }
  c.first_dt = p.first_dt;
  return c;
}

// The mutable members of OnboardController and its six PIDController's, in registers.  In memory: double[SE3MPC_ONBOARD_STATE_WORDS].
template <typename R>
struct OnboardRegs {
  R integral[6], last_error[6];
  double last_time;
  int has_time;          // last_time is not None
};

template <typename R>
__device__ __forceinline__ OnboardRegs<R> load_onboard(const double* __restrict__ s) {
  OnboardRegs<R> r;
  for (int i = 0; i < 6; ++i) { r.integral[i] = (R)s[i]; r.last_error[i] = (R)s[6 + i]; }
  r.last_time = s[12]; r.has_time = s[13] != 0.0;
  return r;
}
template <typename R>
__device__ __forceinline__ void store_onboard(double* __restrict__ s, const OnboardRegs<R>& r) {
  for (int i = 0; i < 6; ++i) { s[i] = (double)r.integral[i]; s[6 + i] = (double)r.last_error[i]; }
  s[12] = r.last_time; s[13] = r.has_time ? 1.0 : 0.0;
}

// PIDController.update (pid.py:25-51), term by term in its order
template <typename R>
__device__ __forceinline__ R pid_update(const OnboardDev<R>& c, OnboardRegs<R>& s, int i, R setpoint, R measured, R dt) {
  if (dt <= (R)0) return (R)0;                                                    // :27-28
  const R error = setpoint - measured;                                            // :30
  const R P_out = c.kp[i] * error;                                                // :33
  R I = s.integral[i] + error * dt;                                               // :36
  if (c.lim[i] != (R)0) {                                                         // :37 `if self.integral_limit:`
    I = I < -c.lim[i] ? -c.lim[i] : I;                                            // :38-40 np.clip = minimum(maximum(x, lo), hi); NaN stays NaN
    I = I > c.lim[i] ? c.lim[i] : I;
  }
  s.integral[i] = I;
  const R I_out = c.ki[i] * I;                                                    // :41
  const R derivative = (error - s.last_error[i]) / dt;                            // :44
  const R D_out = c.kd[i] * derivative;                                           // :45
  const R output = (P_out + I_out) + D_out;                                       // :48
  s.last_error[i] = error;                                                        // :50
  return output;
}

// OnboardController.compute_control_command (onboard.py:172-180) for one drone on the state (t, pos, att, omega): sense (:136-142; the
// sampler runs before the dt test and moves nothing but the cursor), the dt <= 0 command (:176-177), plan (:144-161), act (:163-170).
// The delayed clock can step BACK (the first popped state is older than the last pushed-through one): the cursor then searches from the start.
template <typename R>
__device__ __forceinline__ void onboard_step(const OnboardDev<R>& c, OnboardRegs<R>& s, PlanCursor<R>& cur, int N, const double* ts, const R* P,
                                             const R* V, const R* A, double t, const R pos[3], const R att[3], const R omega[3], R& th,
                                             R tq[3], R tgt[3]) {
  const double dt_d = s.has_time ? t - s.last_time : c.first_dt;                  // :139
  if (!s.has_time || !(dt_d >= 0.0)) cur.idx = 0;
  s.last_time = t; s.has_time = 1;                                                // :140
  R tp[3], tv[3], ta[3];
  sample_plan<R>(t, N, ts, P, V, A, tp, tv, ta, cur);                             // :141
  if (dt_d <= 0.0) {                                                              // :176-177
    th = (R)0; tq[0] = tq[1] = tq[2] = (R)0; tgt[0] = tgt[1] = tgt[2] = (R)0;
    return;
  }
  const R dt = (R)dt_d;
  R acc[3];
  for (int i = 0; i < 3; ++i) acc[i] = ta[i] + pid_update<R>(c, s, PID_X + i, tp[i], pos[i], dt);   // :147-157
  R thrust = c.mass * (acc[2] + c.g);                                             // :100
  thrust = thrust > (R)0 ? thrust : (R)0;                                         // :101 max(0.0, thrust): a NaN gives 0.0
  R sy, cy;
  sin_cos(att[2], sy, cy);
  const R roll_des = c.inv_g * (acc[0] * sy - acc[1] * cy);                       // :104-107
  const R pitch_des = c.inv_g * (acc[0] * cy + acc[1] * sy);                      // :108-111
  tq[0] = pid_update<R>(c, s, PID_ROLL, roll_des, att[0], dt);                    // :125-126
  tq[1] = pid_update<R>(c, s, PID_PITCH, pitch_des, att[1], dt);                  // :128-129
  tq[2] = pid_update<R>(c, s, PID_YAW_RATE, (R)0, omega[2], dt);                  // :131-132, :165
  th = thrust;
  for (int i = 0; i < 3; ++i) tgt[i] = tp[i];
}

// get_fallback_command (onboard.py:182-184) with edge/main.py:94's target
template <typename R>
__device__ __forceinline__ void onboard_fallback(const OnboardDev<R>& c, const R pos[3], R& th, R tq[3], R tgt[3]) {
  th = c.hover; tq[0] = tq[1] = tq[2] = (R)0;
  for (int i = 0; i < 3; ++i) tgt[i] = pos[i];
}

// ---- LatencyBuffer (latency.py:34-82) as a ring in HBM: ring [depth][12][B] (pos, vel, att, omega; drone innermost, so the 64 lanes of a
// wavefront whose drones share the slot read and write contiguous rows), ring_time [depth][B].
template <typename R>
struct LatRing {
  R* data;
  double* time;
  int depth, B, b;
  __device__ __forceinline__ void load(int slot, DroneRegs<R>& d) const {
    const R* q = data + (size_t)slot * 12 * B + b;
    for (int i = 0; i < 3; ++i) { d.p[i] = q[(size_t)i * B]; d.v[i] = q[(size_t)(3 + i) * B]; d.a[i] = q[(size_t)(6 + i) * B]; d.w[i] = q[(size_t)(9 + i) * B]; }
    d.t = time[(size_t)slot * B + b];
  }
  __device__ __forceinline__ void store(int slot, const DroneRegs<R>& d) const {
    R* q = data + (size_t)slot * 12 * B + b;
    for (int i = 0; i < 3; ++i) { q[(size_t)i * B] = d.p[i]; q[(size_t)(3 + i) * B] = d.v[i]; q[(size_t)(6 + i) * B] = d.a[i]; q[(size_t)(9 + i) * B] = d.w[i]; }
    time[(size_t)slot * B + b] = d.t;
  }
};

// The record (len(buffer), slot of the oldest entry, total_samples, actual_delay_s).  A length or slot outside the ring reads as an empty
// buffer: no record, whatever it holds, takes an access out of the ring.
struct LatRegs {
  int count, head;
  double total, actual_delay;
};
__device__ __forceinline__ LatRegs load_latency(const double* __restrict__ s, int depth) {
  LatRegs r;
  const double n = s[0], h = s[1];
  const bool ok = n >= 0.0 && n <= (double)depth && h >= 0.0 && h < (double)depth;
  r.count = ok ? (int)n : 0; r.head = ok ? (int)h : 0;
  r.total = s[2]; r.actual_delay = s[3];
  return r;
}
__device__ __forceinline__ void store_latency(double* __restrict__ s, const LatRegs& r) {
  s[0] = (double)r.count; s[1] = (double)r.head; s[2] = r.total; s[3] = r.actual_delay;
}

// One drone's buffer over a run of pushes.  `nxt` holds, in registers, the entry the NEXT push pops whenever the buffer is full (`have`):
// begin() loads it, push() hands it out and -- depth >= 2, early -- loads its successor at once, a slot other than the one this push writes
// and last written depth - 1 pushes ago by this lane, so the load's latency runs under the caller's controller and simulator arithmetic
// instead of in front of it.  Without `early` the entry is loaded by the push that pops it (the measurement variant, same bits).  Depth 1
// is "the previous state": it stays in registers and reaches the ring in end().
template <typename R>
struct LatencyLane {
  LatRing<R> ring;
  LatRegs L;
  DroneRegs<R> nxt;
  bool have;
  __device__ __forceinline__ void begin(const double* __restrict__ rec) {
    L = load_latency(rec, ring.depth);
    have = L.count == ring.depth;
    if (have) ring.load(L.head, nxt);
  }
  // push(cur) -> delayed; early: another push follows in this launch and may have its entry loaded now
  __device__ __forceinline__ void push(const DroneRegs<R>& cur, DroneRegs<R>& delayed, bool early) {
    const int depth = ring.depth;
    if (L.count < depth) {                                                        // latency.py:68-73
      int slot = L.head + L.count;
      slot = slot >= depth ? slot - depth : slot;
      if (depth > 1) ring.store(slot, cur);
      L.count += 1;
      delayed = cur;
    } else {                                                                      // :74-82
      if (!have) ring.load(L.head, nxt);
      delayed = nxt;
      L.actual_delay = cur.t - nxt.t;                                             // :81
      if (depth > 1) { ring.store(L.head, cur); L.head = L.head + 1 == depth ? 0 : L.head + 1; }
    }
    L.total += 1.0;                                                               // :71 / :78
    have = depth == 1;
    if (depth == 1) nxt = cur;
    else if (early && L.count == depth) { ring.load(L.head, nxt); have = true; }
  }
  __device__ __forceinline__ void end(double* __restrict__ rec) {
    if (ring.depth == 1 && L.count == 1) ring.store(0, nxt);
    store_latency(rec, L);
  }
};

// One step of the reference's edge loop (edge/main.py:81-95) for one drone: the push through its buffer (depth = 0: none, delayed = the
// state), the OnboardController on the delayed state against the N-row plan (N = 0: the fallback), the count of a commanded thrust of
// exactly 0, the simulator step under the command.  -> the command (th, tq); log(target [3], delayed clock) is called between command and
// simulator step.  The step of se3mpc_edge_loop_* (through lane_loop) and of se3mpc_monte_carlo_edge_*: one definition,
// hence the same bits.
template <typename R, typename F>
__device__ __forceinline__ void edge_step(const OnboardDev<R>& c, const SimDev<R>& m, OnboardRegs<R>& s, PlanCursor<R>& cur, LatencyLane<R>& lat,
                                          int depth, bool early, int N, const double* ts, const R* P, const R* V, const R* A, DroneRegs<R>& d,
                                          R dt, double sim_dt, int& zeros, R& th, R tq[3], F&& log) {
  DroneRegs<R> del;
  if (depth > 0) lat.push(d, del, early);                                         // edge/main.py:81-85
  else del = d;
  R tg[3];
  if (N > 0) onboard_step<R>(c, s, cur, N, ts, P, V, A, del.t, del.p, del.a, del.w, th, tq, tg);   // :87-90
  else onboard_fallback<R>(c, del.p, th, tq, tg);                                 // :91-94
  log(tg, del.t);
  if (th == (R)0) ++zeros;
  simulator_step<R>(m, d.p, d.v, d.a, d.w, d.t, th, tq, dt, sim_dt, d.wd);        // :95
}

static inline int check_onboard_params(const se3mpc_onboard_params* p) {
  if (p == nullptr) return SE3MPC_ERR_NULL;
  const double* d = reinterpret_cast<const double*>(p);
  for (int i = 0; i < 27; ++i)
    if (!std::isfinite(d[i])) return SE3MPC_ERR_PARAM;
  if (!(p->mass > 0.0)) return SE3MPC_ERR_PARAM;
  return SE3MPC_OK;
}

}  // namespace se3mpc
