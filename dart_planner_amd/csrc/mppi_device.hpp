// mppi_device.hpp -- code shared by the MPPI kernels: mppi.hip (one workgroup per problem, every iteration in one launch),
// mppi_split.hip (one problem's samples over several workgroups, one launch per iteration) and mppi_closed_loop.hip (the planner inside
// the closed loop).  The noise, the sample, the forward sweep, the weighted pass over a sample range and the
// update of the nominal are defined once, here, so the files agree bit for bit wherever their summation orders agree; so are the
// argument rules their entry points have in common (check_mppi_args).
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "se3mpc_common.hpp"
#include "closed_loop_device.hpp"
#include <se3mpc_wave_ops.hpp>

namespace se3mpc {
namespace mppi {

constexpr int kBlock = 256;                // workgroup width (samples per pass); S < 256 runs S lanes
constexpr int kMinS = 64, kMaxS = 65536;
constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;

// Philox4x32-10 (Salmon et al., SC'11): ten rounds, the key bumped between rounds.  The 32 x 32 -> 64 products are plain uint64_t
// arithmetic (v_mul_lo_u32 / v_mul_hi_u32); the first round's products of the uniform counter words q and g go to the scalar unit.
__device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    if (r) { k0 += kPhiloxW0; k1 += kPhiloxW1; }
    const uint64_t a = (uint64_t)kPhiloxM0 * c[0], b = (uint64_t)kPhiloxM1 * c[2];
    const uint32_t n0 = (uint32_t)(b >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(a >> 32) ^ c[3] ^ k1;
    c[0] = n0; c[1] = (uint32_t)b; c[2] = n2; c[3] = (uint32_t)a;
  }
}

// Box-Muller on the four words of one Philox block: three standard normals
template <typename R>
__device__ __forceinline__ void box_muller(const uint32_t x[4], R n[3]) {
  const R scale = (R)2.3283064365386962890625e-10;          // 2^-32
  const R two_pi = (R)6.283185307179586476925;
  const R u0 = ((R)x[0] + (R)0.5) * scale, u1 = ((R)x[1] + (R)0.5) * scale;
  const R u2 = ((R)x[2] + (R)0.5) * scale, u3 = ((R)x[3] + (R)0.5) * scale;
  const R r01 = sqrt((R)-2 * log(u0)), r23 = sqrt((R)-2 * log(u2));
  R s1, c1;
  sin_cos(two_pi * u1, s1, c1);
  n[0] = r01 * c1;
  n[1] = r01 * s1;
  n[2] = r23 * cos(two_pi * u3);
}

template <typename R>
__device__ __forceinline__ R box_clip(const DevParams<R>& q, int a, R t) {
  const R lo = (a == 2) ? q.tz_lo : -q.txy, hi = (a == 2) ? q.tz_hi : q.txy;
  return fmin(fmax(t, lo), hi);
}

// What a context of MOVING spheres adds (se3mpc_mppi_moving_*): the velocity table and the time of every step of the
// horizon in the kernel's type, both in LDS.  The static context holds neither: Ctx<R> is the struct it always was.
template <typename R, bool MOVING>
struct CtxMotion {};
template <typename R>
struct CtxMotion<R, true> {
  const R* svel;    // LDS [K][3] = (vx, vy, vz)
  const R* stime;   // LDS [N]: tR_k = (R)tau_k, the time of the state before step k on the table's clock
};

// What TRACKED spheres add behind the moving table (se3mpc_mppi_tracks_*): a slab of centres given per step of the horizon.
// Again through an empty base: Ctx<R> and Ctx<R, true> are the structs they were.
template <typename R, bool TRACKED>
struct CtxTracks {};
template <typename R>
struct CtxTracks<R, true> {
  const R* trk;     // LDS [N][Kt][4] = (x, y, z, (r + margin)^2): row [k][j] = tracked sphere j at the state before step k
  int Kt;
};

template <typename R, bool MOVING = false, bool TRACKED = false>
struct Ctx : CtxMotion<R, MOVING>, CtxTracks<R, TRACKED> {
  static_assert(MOVING || !TRACKED, "the tracked rows come behind a moving table");
  DevParams<R> q;
  uint32_t key0, key1, qi, g;
  const R* U;       // LDS [3N]
  const R* sph;     // LDS [K][4] = (cx, cy, cz, (r + margin)^2)
  int K;
  R w_obs;
  R p0[3], v0[3], gl[3];
};

// Sample s at step k: the noise (raw words / normals optional) and the clipped thrust.  The one expression mppi_samples_kernel and
// the fused kernel share, so the two agree bit for bit.
template <typename R, bool MOVING, bool TRACKED>
__device__ __forceinline__ void draw(const Ctx<R, MOVING, TRACKED>& c, const R* Uk, uint32_t s, int k, R sig, R t[3], uint32_t* raw = nullptr, R* nrm = nullptr) {
  uint32_t x[4] = {c.qi, s, c.g, (uint32_t)k};
  philox4x32_10(x, c.key0, c.key1);
  R n[3];
  box_muller<R>(x, n);
  if (raw != nullptr) { raw[0] = x[0]; raw[1] = x[1]; raw[2] = x[2]; raw[3] = x[3]; }
  if (nrm != nullptr) { nrm[0] = n[0]; nrm[1] = n[1]; nrm[2] = n[2]; }
#pragma unroll
  for (int a = 0; a < 3; ++a) t[a] = box_clip(c.q, a, Uk[a] + sig * n[a]);
}

template <typename R>
struct Roll {
  R p[3], v[3];
  R sp, sterm, sv, sa, st, pen;
};

// One step of the forward sweep (planner.py:449-460 solved forward, the objective of :516-550, the sphere penalty on P_k).  MOVING: sphere
// j's centre at step k is c_j + v_j * tR_k (one multiply-add per axis; v_j = 0 leaves c_j exactly), then the same expression.  TRACKED: behind
// the K moving rows the Kt rows of step k of the slab, their centres read as they stand (no time arithmetic), the same expression, pen
// summed on in rising index.
template <typename R, bool MOVING, bool TRACKED>
__device__ __forceinline__ void roll_step(const Ctx<R, MOVING, TRACKED>& c, Roll<R>& r, int k, const R t[3]) {
  const DevParams<R>& q = c.q;
  R acc[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    acc[a] = t[a] * q.inv_mass - ((a == 2) ? q.grav : (R)0);
    const R dev = t[a] - ((a == 2) ? q.hover : (R)0);
    const R e = r.p[a] - c.gl[a];
    if (k == q.N - 1) r.sterm += e * e; else r.sp += e * e;
    r.sv += r.v[a] * r.v[a];
    r.sa += acc[a] * acc[a];
    r.st += dev * dev;
  }
  [[maybe_unused]] R tR = (R)0;
  if constexpr (MOVING) tR = c.stime[k];
  for (int j = 0; j < c.K; ++j) {
    const R* s4 = c.sph + 4 * j;
    R cx = s4[0], cy = s4[1], cz = s4[2];
    if constexpr (MOVING) {
      const R* v3 = c.svel + 3 * j;
      cx = cx + v3[0] * tR; cy = cy + v3[1] * tR; cz = cz + v3[2] * tR;
    }
    const R dx = r.p[0] - cx, dy = r.p[1] - cy, dz = r.p[2] - cz;
    const R cc = dz * dz + (dy * dy + (dx * dx - s4[3]));
    const R h = fmax((R)0, -cc);
    r.pen += h * h;
  }
  if constexpr (TRACKED) {
    const R* row = c.trk + (size_t)4 * c.Kt * k;
    for (int j = 0; j < c.Kt; ++j) {
      const R* s4 = row + 4 * j;
      const R dx = r.p[0] - s4[0], dy = r.p[1] - s4[1], dz = r.p[2] - s4[2];
      const R cc = dz * dz + (dy * dy + (dx * dx - s4[3]));
      const R h = fmax((R)0, -cc);
      r.pen += h * h;
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    r.p[a] = r.p[a] + r.v[a] * q.dt + q.half_dt2 * acc[a];
    r.v[a] = r.v[a] + acc[a] * q.dt;
  }
}

// The state recurrence of roll_step alone, for a caller that wants the trajectory and not the cost: (p, v) advance by one step under
// thrust t, acc = the acceleration roll_step forms from t
template <typename R>
__device__ __forceinline__ void roll_state_step(const DevParams<R>& q, R p[3], R v[3], const R t[3], R acc[3]) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    acc[a] = t[a] * q.inv_mass - ((a == 2) ? q.grav : (R)0);
    p[a] = p[a] + v[a] * q.dt + q.half_dt2 * acc[a];
    v[a] = v[a] + acc[a] * q.dt;
  }
}

template <typename R, bool MOVING, bool TRACKED>
__device__ __forceinline__ Roll<R> roll_begin(const Ctx<R, MOVING, TRACKED>& c) {
  Roll<R> r;
#pragma unroll
  for (int a = 0; a < 3; ++a) { r.p[a] = c.p0[a]; r.v[a] = c.v0[a]; }
  r.sp = r.sterm = r.sv = r.sa = r.st = r.pen = (R)0;
  return r;
}

template <typename R, bool MOVING, bool TRACKED>
__device__ __forceinline__ R roll_total(const Ctx<R, MOVING, TRACKED>& c, const Roll<R>& r) {
  const DevParams<R>& q = c.q;
  R cost = q.wv * r.sv + q.wa * r.sa + q.wT * r.st;
  if (q.has_goal) cost += q.wp * (r.sp + r.sterm) + q.term * q.wp * r.sterm;
  return cost + c.w_obs * r.pen;
}

// Cost of sample s (NOISE) or of the nominal as it stands (!NOISE: no draw, no clip -- the final evaluation)
template <typename R, bool NOISE, bool MOVING, bool TRACKED>
__device__ __forceinline__ R sample_cost(const Ctx<R, MOVING, TRACKED>& c, uint32_t s, R sig) {
  Roll<R> r = roll_begin(c);
  for (int k = 0; k < c.q.N; ++k) {
    R t[3];
    if (NOISE) draw(c, c.U + 3 * k, s, k, sig, t); else { t[0] = c.U[3 * k]; t[1] = c.U[3 * k + 1]; t[2] = c.U[3 * k + 2]; }
    roll_step(c, r, k, t);
  }
  return roll_total(c, r);
}

// LDS carve-up of the fused kernel (bytes, every region 16-byte aligned): acc [3N + 1] double | part [W][3N + 1] double | red [W] double |
// U [3N] R | sph [K][4] R
struct Lds {
  size_t acc, part, red, U, sph, total;
};
__host__ __device__ inline size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }
__host__ __device__ inline Lds lds_layout(int N, int K, int W, size_t esz) {
  Lds l;
  const size_t rows1 = (size_t)3 * N + 1;
  l.acc = 0;
  l.part = align16(l.acc + rows1 * 8);
  l.red = align16(l.part + (size_t)W * rows1 * 8);
  l.U = align16(l.red + (size_t)W * 8);
  l.sph = align16(l.U + (size_t)3 * N * esz);
  l.total = align16(l.sph + (size_t)4 * K * esz);
  return l;
}

// Behind that image, the kernels of moving spheres keep: vel [K][3] R | step times [N] R
struct MovingLds {
  size_t vel, time, total;
};
__host__ __device__ inline MovingLds moving_lds_layout(int N, int K, int W, size_t esz) {
  MovingLds m;
  m.vel = lds_layout(N, K, W, esz).total;
  m.time = align16(m.vel + (size_t)3 * K * esz);
  m.total = align16(m.time + (size_t)N * esz);
  return m;
}

// Behind an image whose end the caller names (the planner's moving image, or a closed loop's), the kernels of tracked spheres keep
// (DESIGN.md 5.8h): trk [N][Kt][4] R
struct TrackLds {
  size_t trk, total;
};
__host__ __device__ inline TrackLds track_lds_layout(size_t behind, int N, int Kt, size_t esz) {
  TrackLds t;
  t.trk = align16(behind);
  t.total = align16(t.trk + (size_t)4 * N * Kt * esz);
  return t;
}

// The image as pointers
template <typename R>
struct LdsView {
  double *acc, *part, *red;
  R *U, *sph;
};
template <typename R>
__device__ __forceinline__ LdsView<R> lds_view(unsigned char* lds_raw, const Lds& L) {
  LdsView<R> v;
  v.acc = reinterpret_cast<double*>(lds_raw + L.acc);
  v.part = reinterpret_cast<double*>(lds_raw + L.part);
  v.red = reinterpret_cast<double*>(lds_raw + L.red);
  v.U = reinterpret_cast<R*>(lds_raw + L.U);
  v.sph = reinterpret_cast<R*>(lds_raw + L.sph);
  return v;
}

// The sphere table into LDS as (cx, cy, cz, (r + margin)^2); the caller's __syncthreads() publishes it.  (A slab of tracked spheres
// [N][Kt][4] is a table of N * Kt rows.)
template <typename R>
__device__ __forceinline__ void stage_spheres(const DevParams<R>& q, const R* __restrict__ spheres, int K, R* sph) {
  for (int i = (int)threadIdx.x; i < 4 * K; i += (int)blockDim.x) {
    const R v = spheres[i];
    sph[i] = ((i & 3) == 3) ? (v + q.margin) * (v + q.margin) : v;
  }
}

// (MOVING: the caller sets svel and stime; TRACKED: trk and Kt)
template <typename R, bool MOVING = false, bool TRACKED = false>
__device__ __forceinline__ Ctx<R, MOVING, TRACKED> load_ctx(const DevParams<R>& q, int ld, int p, uint32_t key0, uint32_t key1, uint32_t qi, const R* p0,
                                                   const R* v0, const R* goal, const R* U, const R* sph, int K, R w_obs) {
  Ctx<R, MOVING, TRACKED> c;
  c.q = q; c.key0 = key0; c.key1 = key1; c.qi = qi; c.g = 0; c.U = U; c.sph = sph; c.K = K; c.w_obs = w_obs;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    c.p0[a] = p0[(size_t)a * ld + p];
    c.v0[a] = v0[(size_t)a * ld + p];
    c.gl[a] = q.has_goal ? goal[(size_t)a * ld + p] : (R)0;
  }
  return c;
}

// The weighted pass of one workgroup over samples [s_lo, s_lo + count) of iteration c.g, in chunks of the workgroup's width: cost pass,
// chunk minimum (wavefront min, then the W partials in wavefront order), T_s regenerated, float64 weighted rows through wave_sum_n<3>,
// wavefront partials folded in wavefront order, chunks folded in chunk order with the streaming rescale.  Returns the minimum cost m of
// the range (+inf when every cost is NaN) and leaves acc[r] = sum_s w_s T_s[r] (r < 3N), acc[3N] = sum_s w_s, w_s = exp(-(c_s - m) / lambda),
// in LDS, visible to the whole workgroup.
template <typename R, bool MOVING, bool TRACKED>
__device__ __forceinline__ double weighted_pass(const Ctx<R, MOVING, TRACKED>& c, const R* U, int s_lo, int count, R sigma, double inv_lam, double* acc, double* part,
                                                double* red) {
  const int N = c.q.N, rows = 3 * N, NT = (int)blockDim.x, W = NT / kWave;
  const int tid = (int)threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const double kInf = __builtin_huge_val();
  double m = kInf;
  for (int c0 = 0; c0 < count; c0 += NT) {
    const uint32_t s = (uint32_t)(s_lo + c0 + tid);
    const bool live = c0 + tid < count;
    const R sig = s == 0 ? (R)0 : sigma;
    double cd = kInf;
    if (live) {
      const R cs = sample_cost<R, true>(c, s, sig);
      if (cs == cs) cd = (double)cs;                     // a NaN cost weighs nothing
    }
    // chunk minimum: wavefront min, then the W partials in wavefront order
    const double wm = wave_min(cd);
    if (lane == 0) red[wave] = wm;
    __syncthreads();
    double mc = red[0];
    for (int w = 1; w < W; ++w) mc = fmin(mc, red[w]);
    const double mn = fmin(m, mc);
    const double scale = (m < kInf) ? exp((mn - m) * inv_lam) : 0.0;     // earlier chunks re-expressed against the new minimum
    const double wgt = (cd < kInf) ? exp(-(cd - mn) * inv_lam) : 0.0;
    double* mine = part + (size_t)wave * (rows + 1);
    // weighted rows of this chunk (T_s regenerated): wavefront sums three rows at a time, one partial per wavefront in LDS
    for (int k = 0; k < N; ++k) {
      R t[3];
      draw(c, U + 3 * k, s, k, sig, t);
      double v3[3] = {wgt > 0.0 ? wgt * (double)t[0] : 0.0, wgt > 0.0 ? wgt * (double)t[1] : 0.0, wgt > 0.0 ? wgt * (double)t[2] : 0.0};
      wave_sum_n<3>(v3);
      if (lane == 0) { mine[3 * k] = v3[0]; mine[3 * k + 1] = v3[1]; mine[3 * k + 2] = v3[2]; }
    }
    const double ws = wave_sum(wgt);
    if (lane == 0) mine[rows] = ws;
    __syncthreads();
    for (int r = tid; r <= rows; r += NT) {
      double sum = part[r];
      for (int w = 1; w < W; ++w) sum += part[(size_t)w * (rows + 1) + r];
      acc[r] = (c0 == 0) ? sum : acc[r] * scale + sum;
    }
    m = mn;
    __syncthreads();
  }
  return m;
}

// The update after a weighted pass over ALL samples of an iteration: U <- the weighted mean acc / acc[3N] (the clip only guards the
// rounding of the division: a mean of in-box samples is in the box; no finite cost: U stays), the pass's minimum m to trace[at]
// (trace null: none).  Ends with the workgroup synchronised on U.
template <typename R>
__device__ __forceinline__ void nominal_update(const DevParams<R>& q, const double* acc, R* U, double m, R* trace, size_t at) {
  const int rows = 3 * q.N, NT = (int)blockDim.x, tid = (int)threadIdx.x;
  const double wsum = acc[rows];
  for (int r = tid; r < rows; r += NT)
    if (wsum > 0.0) U[r] = box_clip(q, r % 3, (R)(acc[r] / wsum));
  if (tid == 0 && trace != nullptr) trace[at] = (R)m;
  __syncthreads();
}

// The receding-horizon warm start of the nominal in LDS, by the whole workgroup: U[k] <- U[k + shift] for k < N - shift, (0, 0, hover) for
// the rows behind (shift = 0 keeps U, shift = N resets it).  tmp: LDS scratch of 3N values; U is visible to every lane on return.
template <typename R>
__device__ __forceinline__ void shift_nominal(const DevParams<R>& q, R* U, R* tmp, int shift) {
  const int rows = 3 * q.N;
  for (int r = (int)threadIdx.x; r < rows; r += (int)blockDim.x) {
    const int src = r + 3 * shift;
    tmp[r] = src < rows ? U[src] : ((r % 3 == 2) ? q.hover : (R)0);
  }
  __syncthreads();
  for (int r = (int)threadIdx.x; r < rows; r += (int)blockDim.x) U[r] = tmp[r];
  __syncthreads();
}

// Cost and argmin key of the nominal as it stands, written by lane 0 of the calling wavefront (the tail of every MPPI entry point)
template <typename R, bool MOVING, bool TRACKED>
__device__ __forceinline__ void write_nominal_cost(const Ctx<R, MOVING, TRACKED>& c, int p, uint32_t index_base, R* cost_out, uint64_t* keys) {
  const R cf = sample_cost<R, false>(c, 0u, (R)0);
  if ((threadIdx.x & (kWave - 1)) == 0) {
    cost_out[p] = cf;
    if (keys != nullptr) keys[p] = ((uint64_t)orderable_bits((float)cf) << 32) | (uint64_t)(index_base + (uint32_t)p);
  }
}

// ---- host side: the argument rules the MPPI entry points share -------------------------------------------------------------------------
// fn: the entry point's name, put in front of the message
static int fail(int rc, const char* what, const char* fn = nullptr) {
  char msg[160];
  if (fn != nullptr) {
    std::snprintf(msg, sizeof(msg), "%s: %s", fn, what);
    what = msg;
  }
  set_last_message(what);
  return rc;
}

// The batch and the sample set (every entry point)
static int check_mppi_batch(const char* fn, const se3mpc_params* p, int nprob, int ld, int S, double sigma) {
  if (p == nullptr) return fail(SE3MPC_ERR_NULL, "params is NULL", fn);
  const int rc = check_params_impl(p);
  if (rc != SE3MPC_OK) return fail(rc, "invalid params", fn);
  if (nprob < 0 || ld < nprob) return fail(SE3MPC_ERR_SHAPE, "batch size < 0 or leading dimension < batch size", fn);
  if (S < kMinS || S > kMaxS || S % kWave != 0) return fail(SE3MPC_ERR_SHAPE, "S outside [64, 65536] or not a multiple of 64", fn);
  if (!(sigma >= 0.0) || !std::isfinite(sigma)) return fail(SE3MPC_ERR_PARAM, "sigma must be finite and >= 0", fn);
  return SE3MPC_OK;
}

// ... and the planner's own (se3mpc_mppi_*, se3mpc_mppi_split_*, se3mpc_mppi_closed_loop_*), in the order se3mpc_mppi_* checks them
static int check_mppi_args(const char* fn, const se3mpc_params* p, int nprob, int ld, int S, int iters, double sigma, double temperature, int K,
                           double obstacle_weight) {
  const int rc = check_mppi_batch(fn, p, nprob, ld, S, sigma);
  if (rc) return rc;
  if (iters < 0) return fail(SE3MPC_ERR_SHAPE, "iters < 0", fn);
  if (K < 0 || K > SE3MPC_MAX_SPHERES) return fail(SE3MPC_ERR_SHAPE, "K outside [0, SE3MPC_MAX_SPHERES]", fn);
  if (!(temperature > 0.0) || !std::isfinite(temperature)) return fail(SE3MPC_ERR_PARAM, "temperature must be finite and > 0", fn);
  if (!(obstacle_weight >= 0.0) || !std::isfinite(obstacle_weight)) return fail(SE3MPC_ERR_PARAM, "obstacle_weight must be finite and >= 0", fn);
  return SE3MPC_OK;
}

// ... and what the entries of moving spheres add (se3mpc_mppi_moving_*, se3mpc_mppi_closed_loop_moving_*), after the rules above
static int check_moving_args(const char* fn, int K, const void* sphere_vel, double sphere_t0) {
  if (!std::isfinite(sphere_t0)) return fail(SE3MPC_ERR_PARAM, "sphere_t0 must be finite", fn);
  if (K > 0 && sphere_vel == nullptr) return fail(SE3MPC_ERR_NULL, "sphere_vel is NULL with K > 0", fn);
  return SE3MPC_OK;
}

// ... and what the entries of tracked spheres add (se3mpc_mppi_tracks_*, se3mpc_mppi_closed_loop_tracks_*), after the rules above
static int check_track_args(const char* fn, int K, int Kt, const void* tracks, long long track_stride, int N) {
  if (Kt < 0 || Kt > SE3MPC_MAX_TRACKS) return fail(SE3MPC_ERR_SHAPE, "Kt outside [0, SE3MPC_MAX_TRACKS]", fn);
  if (K + Kt > SE3MPC_MAX_SPHERES) return fail(SE3MPC_ERR_SHAPE, "K + Kt > SE3MPC_MAX_SPHERES", fn);
  if (Kt > 0 && track_stride != 0 && track_stride < (long long)4 * N * Kt)
    return fail(SE3MPC_ERR_SHAPE, "track_stride must be 0 or >= 4 * horizon * Kt", fn);
  if (Kt > 0 && tracks == nullptr) return fail(SE3MPC_ERR_NULL, "tracks is NULL with Kt > 0", fn);
  return SE3MPC_OK;
}

}  // namespace mppi
}  // namespace se3mpc
