// parity_kernels.hip -- lane-layout ([row][b]) parity forms of the SE(3) MPC path (a3..a16).
//
// One trajectory per lane: lane b of a wavefront reads element [row][b], so every load/store of
// a wavefront is one contiguous, fully used 256-B (f32) segment.  All of these kernels are
// HBM-streaming (1.7-10 flop/B, far below the fp32 ridge of ~20 flop/B); none has a dense
// contraction, so none uses MFMA (the "12x12 linearised dynamics" of the brief is
// a 2-FMA-per-axis LTI map).  Reference arithmetic: src/dart_planner/planning/se3_mpc_planner.py
// ("planner.py" in the comments), unit-stripped.
#include "lane_common.hpp"
#include <se3mpc_wave_ops.hpp>

namespace se3mpc {

// ------------------------------------------------------------------------------------------
// a3 + a4: cold start (planner.py:329-359) and optional projection into the box (:378-402)
// ------------------------------------------------------------------------------------------
template <typename R>
__global__ void __launch_bounds__(192)
init_kernel(DevParams<R> q, int B, int ld, const R* __restrict__ p0, const R* __restrict__ v0,
            const R* __restrict__ goal, int project, R* __restrict__ X) {
  // write-only stream: a 192-thread workgroup owns 64 trajectories, wavefront w writes axis w (3x the wavefronts in flight)
  int blk = blockIdx.x;
  if ((gridDim.x & 7) == 0) blk = (blk & 7) * (gridDim.x >> 3) + (blk >> 3);
  const int b0 = blk * kWave + (int)(threadIdx.x & (kWave - 1));
  if (b0 >= B) return;
  const unsigned voff = (unsigned)b0 * (unsigned)sizeof(R), rowb = (unsigned)ld * (unsigned)sizeof(R);
  const int a = wave_uniform((int)(threadIdx.x / kWave));
  const int N = q.N, N3 = 3 * q.N;
  const R denom = (R)(N - 1 > 1 ? N - 1 : 1);
  const R p = lane_ld<2>(lane_buf(p0), voff, (unsigned)(a) * rowb);
  const R v = lane_ld<2>(lane_buf(v0), voff, (unsigned)(a) * rowb);
  const R g = q.has_goal ? lane_ld<2>(lane_buf(goal), voff, (unsigned)(a) * rowb) : p;
  R prev = p;
#pragma unroll 4
  for (int i = 0; i < N; ++i) {
    R pi, vi;
    if (q.has_goal) {
      const R alpha = (R)i / denom;                       // planner.py:344
      pi = ((R)1 - alpha) * p + alpha * g;                // planner.py:345-347
      if constexpr (sizeof(R) == 4) {
        // float32: (P_i - P_{i-1})/dt loses ~|P| * 6e-8 / dt ~ 1e-3 m/s to cancellation; the
        // algebraically identical (alpha_i - alpha_{i-1}) (goal - p0) / dt does not
        vi = (i == 0) ? v : ((alpha - (R)(i - 1) / denom) * (g - p)) / q.dt;
      } else {
        vi = (i == 0) ? v : (pi - prev) / q.dt;           // planner.py:339, :350
      }
    } else {
      pi = p;                                             // planner.py:356
      vi = (i == 0) ? v : (R)0;
    }
    prev = pi;
    R ti = (a == 2) ? q.hover : (R)0;                     // planner.py:353
    if (project) {
      pi = fmin(fmax(pi, -q.pos_b), q.pos_b);
      vi = fmin(fmax(vi, -q.v_max), q.v_max);
      ti = (a == 2) ? fmin(fmax(ti, q.tz_lo), q.tz_hi) : ti;
    }
    lane_st<2>(lane_buf(X), voff, (unsigned)(3 * i + a) * rowb, (R)(pi));
    lane_st<2>(lane_buf(X), voff, (unsigned)(N3 + 3 * i + a) * rowb, (R)(vi));
    lane_st<2>(lane_buf(X), voff, (unsigned)(2 * N3 + 3 * i + a) * rowb, (R)(ti));
  }
}

// ------------------------------------------------------------------------------------------
// a5 + a6: objective (planner.py:516-550) and the reference's gradient (planner.py:552-580)
// ------------------------------------------------------------------------------------------
// Streaming shape shared by the parity-form kernels below: a 192-thread workgroup owns 64 trajectories and
// wavefront w works on axis w wherever the arithmetic is separable per axis; rows are taken in chunks of kChunk steps whose loads
// are ALL issued before the first use (3 * kChunk independent HBM requests in flight per lane, the same memory-level parallelism the
// benchmarked rollout kernel gets from its register arrays), then consumed and stored.  Per-row loops with a load -> use -> store
// dependence per step reached 55-63 % of the HBM peak; this shape reaches the copy ceiling of the part.
#ifndef SE3MPC_LANE_CHUNK
#define SE3MPC_LANE_CHUNK 16
#endif
constexpr int kChunk = SE3MPC_LANE_CHUNK;

template <typename R, bool WANT_G>
__global__ void __launch_bounds__(192)
cost_grad_kernel(DevParams<R> q, int B, int ld, const R* __restrict__ X, const R* __restrict__ goal,
                 R* __restrict__ f, R* __restrict__ g) {
  __shared__ R part[3][kWave];
  int blk = blockIdx.x;
  if ((gridDim.x & 7) == 0) blk = (blk & 7) * (gridDim.x >> 3) + (blk >> 3);
  const int lane = threadIdx.x & (kWave - 1);
  const int b0 = blk * kWave + lane;
  const bool live = b0 < B;
  const int b = live ? b0 : B - 1;                          // tail lanes shadow the last column (benign duplicate stores)
  const unsigned voff = (unsigned)b * (unsigned)sizeof(R), rowb = (unsigned)ld * (unsigned)sizeof(R);
  const int a = wave_uniform((int)(threadIdx.x / kWave));
  const int N = q.N, N3 = 3 * q.N;
  const LaneBuf<R> xb = lane_buf(X), gb = lane_buf(g);
  const R gl = q.has_goal ? lane_ld(lane_buf(goal), voff, (unsigned)a * rowb) : (R)0;
  const R grav = (a == 2) ? q.grav : (R)0;
  const R hov = (a == 2) ? q.hover : (R)0;
  const R two_wp = q.has_goal ? (R)2 * q.wp : (R)0, two_wv = (R)2 * q.wv, two_wT = (R)2 * q.wT;
  R sp = 0, sv = 0, sa = 0, st = 0, sterm = 0;
  for (int k0 = 0; k0 < N; k0 += kChunk) {
    R x[kChunk], v[kChunk], t[kChunk];
#pragma unroll
    for (int u = 0; u < kChunk; ++u) {
      if (k0 + u < N) {
        const unsigned r = (unsigned)(3 * (k0 + u) + a);
        x[u] = lane_ld<2>(xb, voff, r * rowb);
        v[u] = lane_ld<2>(xb, voff, (unsigned)(N3 + r) * rowb);
        t[u] = lane_ld<2>(xb, voff, (unsigned)(2 * N3 + r) * rowb);
      }
    }
#pragma unroll
    for (int u = 0; u < kChunk; ++u) {
      if (k0 + u < N) {
        const unsigned r = (unsigned)(3 * (k0 + u) + a);
        const R e = x[u] - gl;
        const R acc = t[u] * q.inv_mass - grav;             // planner.py:535-537
        const R dev = t[u] - hov;                           // planner.py:542
        sp += e * e; sv += v[u] * v[u]; sa += acc * acc; st += dev * dev;
        if (k0 + u == N - 1) sterm += e * e;                // planner.py:546-548
        if (WANT_G) {
          lane_st<2>(gb, voff, r * rowb, two_wp * e);                         // planner.py:567-570 (no terminal x10)
          lane_st<2>(gb, voff, (unsigned)(N3 + r) * rowb, two_wv * v[u]);     // planner.py:573-574
          lane_st<2>(gb, voff, (unsigned)(2 * N3 + r) * rowb, two_wT * t[u]); // planner.py:577-578 (no hover offset, no accel term)
        }
      }
    }
  }
  R c = q.wv * sv + q.wa * sa + q.wT * st;
  if (q.has_goal) c += q.wp * sp + q.term * q.wp * sterm;
  part[a][lane] = c;
  __syncthreads();
  if (a == 0 && live) f[b] = part[0][lane] + part[1][lane] + part[2][lane];
}

// ------------------------------------------------------------------------------------------
// a8: dynamics equality residuals (planner.py:426-462)
// ------------------------------------------------------------------------------------------
template <typename R>
__global__ void __launch_bounds__(192)
dynamics_residual_kernel(DevParams<R> q, int B, int ld, const R* __restrict__ X,
                         const R* __restrict__ p0, const R* __restrict__ v0, R* __restrict__ Rout) {
  // axis-split, chunked (see cost_grad_kernel): the residuals of one axis need only that axis' rows
  int blk = blockIdx.x;
  if ((gridDim.x & 7) == 0) blk = (blk & 7) * (gridDim.x >> 3) + (blk >> 3);
  const int b0 = blk * kWave + (int)(threadIdx.x & (kWave - 1));
  if (b0 >= B) return;
  const unsigned voff = (unsigned)b0 * (unsigned)sizeof(R), rowb = (unsigned)ld * (unsigned)sizeof(R);
  const int a = wave_uniform((int)(threadIdx.x / kWave));
  const int N = q.N, N3 = 3 * q.N;
  const LaneBuf<R> xb = lane_buf(X), rb = lane_buf(Rout);
  const R grav = (a == 2) ? q.grav : (R)0;
  const R dt2 = q.dt * q.dt;
  R pk = lane_ld<2>(xb, voff, (unsigned)(a) * rowb);
  R vk = lane_ld<2>(xb, voff, (unsigned)(N3 + a) * rowb);
  lane_st<2>(rb, voff, (unsigned)(a) * rowb, (R)(pk - lane_ld<2>(lane_buf(p0), voff, (unsigned)(a) * rowb)));        // planner.py:439
  lane_st<2>(rb, voff, (unsigned)(3 + a) * rowb, (R)(vk - lane_ld<2>(lane_buf(v0), voff, (unsigned)(a) * rowb)));    // planner.py:440
  for (int k0 = 0; k0 + 1 < N; k0 += kChunk) {
    R t[kChunk], pn[kChunk], vn[kChunk];
#pragma unroll
    for (int u = 0; u < kChunk; ++u) {
      if (k0 + u + 1 < N) {
        const int k = k0 + u;
        t[u] = lane_ld<2>(xb, voff, (unsigned)(2 * N3 + 3 * k + a) * rowb);
        pn[u] = lane_ld<2>(xb, voff, (unsigned)(3 * (k + 1) + a) * rowb);
        vn[u] = lane_ld<2>(xb, voff, (unsigned)(N3 + 3 * (k + 1) + a) * rowb);
      }
    }
#pragma unroll
    for (int u = 0; u < kChunk; ++u) {
      if (k0 + u + 1 < N) {
        const int k = k0 + u;
        const R acc = t[u] / q.mass - grav;                                                                // planner.py:445-447
        lane_st<2>(rb, voff, (unsigned)(6 + 6 * k + a) * rowb, (R)(pn[u] - pk - vk * q.dt - (R)0.5 * acc * dt2));   // :450-455
        lane_st<2>(rb, voff, (unsigned)(6 + 6 * k + 3 + a) * rowb, (R)(vn[u] - vk - acc * q.dt));                    // :459
        pk = pn[u]; vk = vn[u];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// a9: sphere-obstacle inequality residuals (planner.py:499-514); sphere table staged in LDS
// ------------------------------------------------------------------------------------------
template <typename R>
__global__ void obstacle_residual_kernel(DevParams<R> q, int B, int ld, const R* __restrict__ X,
                                         const R* __restrict__ spheres, int K, R* __restrict__ C,
                                         R* __restrict__ cmin, R* __restrict__ viol) {
  __shared__ R sph[SE3MPC_MAX_SPHERES * 4];   // (cx, cy, cz, (r + margin)^2)
  for (int i = threadIdx.x; i < K; i += blockDim.x) {
    sph[4 * i + 0] = spheres[4 * i + 0];
    sph[4 * i + 1] = spheres[4 * i + 1];
    sph[4 * i + 2] = spheres[4 * i + 2];
    const R s = spheres[4 * i + 3] + q.margin;              // planner.py:509
    sph[4 * i + 3] = s * s;
  }
  __syncthreads();
  const LaneIdx li = lane_index<R>(B);
  if (!li.live) return;
  const int b = li.b;
  (void)b;
  const unsigned voff = li.voff, rowb = (unsigned)ld * (unsigned)sizeof(R);
  const int N = q.N;
  R mn = INFINITY, vs = 0;
#pragma unroll 2
  for (int k = 0; k < N; ++k) {
    const R px = lane_ld<2>(lane_buf(X), voff, (unsigned)(3 * k + 0) * rowb);
    const R py = lane_ld<2>(lane_buf(X), voff, (unsigned)(3 * k + 1) * rowb);
    const R pz = lane_ld<2>(lane_buf(X), voff, (unsigned)(3 * k + 2) * rowb);
    for (int j = 0; j < K; ++j) {
      const R dx = px - sph[4 * j + 0], dy = py - sph[4 * j + 1], dz = pz - sph[4 * j + 2];
      const R c = (dx * dx + dy * dy + dz * dz) - sph[4 * j + 3];     // planner.py:508-512
      if (C != nullptr) lane_st<2>(lane_buf(C), voff, (unsigned)(k * K + j) * rowb, (R)(c));
      mn = fmin(mn, c);
      vs += fmax((R)0, -c);
    }
  }
  if (cmin != nullptr) cmin[b] = mn;
  if (viol != nullptr) viol[b] = vs;
}

// a9 reduced in-kernel (no N*K residuals written): min residual and summed violation per trajectory.  The N*K
// distance evaluations are the cost (VALU-bound, not HBM-bound): positions are held in registers four steps at a
// time, the sphere table is walked in pairs (two broadcast 16-B LDS reads per 8 evaluations) and f32 evaluates the
// pair with packed instructions.  The table is padded to an even count with a residual-+inf row; steps past the
// horizon are given a +inf position (residual +inf: neither the minimum nor the violation moves).
template <typename R>
__global__ void obstacle_reduce_kernel(DevParams<R> q, int B, int ld, const R* __restrict__ X, const R* __restrict__ spheres,
                                       int K, R* __restrict__ cmin, R* __restrict__ viol) {
  __shared__ R sph[(SE3MPC_MAX_SPHERES + 2) * 4];
  const int Kpad = (K + 1) & ~1;
  for (int i = threadIdx.x; i < Kpad; i += blockDim.x) {
    const bool real = i < K;
    const R s = real ? spheres[4 * i + 3] + q.margin : (R)0;
    sph[4 * i + 0] = real ? spheres[4 * i + 0] : (R)0;
    sph[4 * i + 1] = real ? spheres[4 * i + 1] : (R)0;
    sph[4 * i + 2] = real ? spheres[4 * i + 2] : (R)0;
    sph[4 * i + 3] = real ? s * s : (R)-INFINITY;
  }
  __syncthreads();
  const LaneIdx li = lane_index<R>(B);
  if (!li.live) return;
  const int b = li.b;
  const unsigned voff = li.voff, rowb = (unsigned)ld * (unsigned)sizeof(R);
  const int N = q.N;
  const LaneBuf<R> xb = lane_buf(X);
  constexpr int S = 4;
  R mn = INFINITY;
  if constexpr (sizeof(R) == 4) {
    typedef float f2 __attribute__((vector_size(8)));
    f2 vs2 = {0.0f, 0.0f};
    for (int k0 = 0; k0 < N; k0 += S) {
      float px[S], py[S], pz[S];
#pragma unroll
      for (int u = 0; u < S; ++u) {
        const int k = (k0 + u < N) ? k0 + u : N - 1;
        px[u] = lane_ld<2>(xb, voff, (unsigned)(3 * k + 0) * rowb);
        py[u] = lane_ld<2>(xb, voff, (unsigned)(3 * k + 1) * rowb);
        pz[u] = lane_ld<2>(xb, voff, (unsigned)(3 * k + 2) * rowb);
        if (k0 + u >= N) px[u] = INFINITY;
      }
      for (int j = 0; j < Kpad; j += 2) {
        const R* s0 = sph + 4 * j;
        const f2 cx = {s0[0], s0[4]}, cy = {s0[1], s0[5]}, cz = {s0[2], s0[6]}, r2 = {s0[3], s0[7]};
#pragma unroll
        for (int u = 0; u < S; ++u) {
          const f2 dx = f2{px[u], px[u]} - cx, dy = f2{py[u], py[u]} - cy, dz = f2{pz[u], pz[u]} - cz;
          const f2 cj = (dx * dx + dy * dy + dz * dz) - r2;                  // planner.py:508-512
          mn = fminf(mn, fminf(cj[0], cj[1]));
          vs2 += f2{fmaxf(0.0f, -cj[0]), fmaxf(0.0f, -cj[1])};
        }
      }
    }
    if (viol != nullptr) viol[b] = vs2[0] + vs2[1];
  } else {
    R vs = (R)0;
    for (int k0 = 0; k0 < N; k0 += S) {
      R px[S], py[S], pz[S];
#pragma unroll
      for (int u = 0; u < S; ++u) {
        const int k = (k0 + u < N) ? k0 + u : N - 1;
        px[u] = lane_ld<2>(xb, voff, (unsigned)(3 * k + 0) * rowb);
        py[u] = lane_ld<2>(xb, voff, (unsigned)(3 * k + 1) * rowb);
        pz[u] = lane_ld<2>(xb, voff, (unsigned)(3 * k + 2) * rowb);
        if (k0 + u >= N) px[u] = INFINITY;
      }
      for (int j = 0; j < Kpad; ++j) {
        const R cx = sph[4 * j], cy = sph[4 * j + 1], cz = sph[4 * j + 2], r2 = sph[4 * j + 3];
#pragma unroll
        for (int u = 0; u < S; ++u) {
          const R dx = px[u] - cx, dy = py[u] - cy, dz = pz[u] - cz;
          const R cj = (dx * dx + dy * dy + dz * dz) - r2;
          mn = fmin(mn, cj);
          vs += fmax((R)0, -cj);
        }
      }
    }
    if (viol != nullptr) viol[b] = vs;
  }
  if (cmin != nullptr) cmin[b] = mn;
}

// ------------------------------------------------------------------------------------------
// a10: physical feasibility constraints (planner.py:472-497)
// ------------------------------------------------------------------------------------------
template <typename R>
__global__ void __launch_bounds__(64)
physical_constraints_kernel(DevParams<R> q, int B, int ld, const R* __restrict__ X, R* __restrict__ C) {
  // every row of the result needs all three axes of a step, so one wavefront keeps whole steps; the six rows of each of
  // kPhysChunk steps are requested before the first use
  constexpr int kPhysChunk = 8;
  const LaneIdx li = lane_index<R>(B);
  if (!li.live) return;
  const unsigned voff = li.voff, rowb = (unsigned)ld * (unsigned)sizeof(R);
  const int N = q.N, N3 = 3 * q.N;
  const LaneBuf<R> xb = lane_buf(X), cb = lane_buf(C);
  for (int k0 = 0; k0 < N; k0 += kPhysChunk) {
    R v[kPhysChunk][3], t[kPhysChunk][3];
#pragma unroll
    for (int u = 0; u < kPhysChunk; ++u) {
      if (k0 + u < N) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          v[u][a] = lane_ld<2>(xb, voff, (unsigned)(N3 + 3 * (k0 + u) + a) * rowb);
          t[u][a] = lane_ld<2>(xb, voff, (unsigned)(2 * N3 + 3 * (k0 + u) + a) * rowb);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kPhysChunk; ++u) {
      if (k0 + u < N) {
        const int k = k0 + u;
        R v2 = 0, a2 = 0, t2 = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          const R acc = t[u][a] / q.mass - ((a == 2) ? q.grav : (R)0);
          v2 += v[u][a] * v[u][a]; a2 += acc * acc; t2 += t[u][a] * t[u][a];
        }
        lane_st<2>(cb, voff, (unsigned)(k) * rowb, (R)(q.v_max2 - v2));                             // planner.py:479-481
        lane_st<2>(cb, voff, (unsigned)(N + k) * rowb, (R)(q.a_max2 - a2));                       // planner.py:484-489
        lane_st<2>(cb, voff, (unsigned)(2 * N + 2 * k) * rowb, (R)(q.t_max2 - t2));               // planner.py:494
        lane_st<2>(cb, voff, (unsigned)(2 * N + 2 * k + 1) * rowb, (R)(t2 - q.t_min2));           // planner.py:495
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// a11 + a12: accelerations, thrust magnitudes, attitudes and body rates (planner.py:582-654)
// ------------------------------------------------------------------------------------------
// One step of planner.py:616-653 for one lane.  prev (b1,b2,b3 of the last valid R) lives in
// registers across the k loop; rows with |T| <= 1e-6 leave it untouched (planner.py:651-653).
template <typename R>
struct AttitudeState {
  R b1[3], b2[3], b3[3];
  bool valid;
};

template <typename R>
__device__ __forceinline__ void attitude_step(const R t[3], R inv_dt, AttitudeState<R>& prev, R att[3], R rate[3], R& mag) {
  mag = sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);                 // planner.py:618
  att[0] = att[1] = att[2] = (R)0;
  rate[0] = rate[1] = rate[2] = (R)0;
  if (!(mag > (R)1e-6)) return;                                        // planner.py:619, :651-653
  // float32: one reciprocal and three products per normalisation instead of three IEEE quotients (1 ulp; this kernel was VALU co-bound:
  // 273 instructions per step, 60 % VALU-busy at 1 M trajectories); float64 keeps the quotients
  R b3[3], b1[3];
  if constexpr (sizeof(R) == 4) { const R rm = rcp_approx(mag); b3[0] = t[0] * rm; b3[1] = t[1] * rm; b3[2] = t[2] * rm; }
  else { b3[0] = t[0] / mag; b3[1] = t[1] / mag; b3[2] = t[2] / mag; }   // planner.py:621
  // b1 = (1,0,0) x b3 = (0, -b3z, b3y)                                // planner.py:625-626
  b1[0] = (R)0; b1[1] = -b3[2]; b1[2] = b3[1];
  const R n1 = sqrt(b1[1] * b1[1] + b1[2] * b1[2]);                    // planner.py:627
  const bool regular = n1 > (R)1e-6;
  if (regular) {                                                       // planner.py:628-629
    if constexpr (sizeof(R) == 4) { const R rn = rcp_approx(n1); b1[1] *= rn; b1[2] *= rn; }
    else { b1[1] /= n1; b1[2] /= n1; }
  } else { b1[0] = (R)1; b1[1] = (R)0; b1[2] = (R)0; }                 // planner.py:630-631
  const R b2[3] = {b3[1] * b1[2] - b3[2] * b1[1],                      // planner.py:632
                   b3[2] * b1[0] - b3[0] * b1[2],
                   b3[0] * b1[1] - b3[1] * b1[0]};
  // R = [b1 b2 b3] (columns).  roll = atan2(R21, R22), pitch = asin(-R20), yaw = atan2(R10, R00)
  att[0] = atan2(b2[2], b3[2]);                                        // planner.py:636
  att[1] = asin(fmin(fmax(-b1[2], (R)-1), (R)1));                      // planner.py:637 (clamped: rounding can leave |R20| 1 ulp above 1)
  // yaw = atan2(b1y, b1x) (planner.py:638) with b1x exactly 0 (regular) or b1 = (1,0,0): +-pi/2 with the sign of b1y (a signed zero stays a
  // signed zero), or 0 -- what atan2 returns there, without evaluating it
  att[2] = regular ? (b1[1] == (R)0 ? b1[1] : copysign((R)1.5707963267948966, b1[1])) : (R)0;
  if (prev.valid) {                                                    // planner.py:641-649
    // omega = R^T (R - R_prev)/dt ; rates = (omega[2][1], omega[0][2], omega[1][0])
    R d1[3], d2[3], d3[3];
    for (int i = 0; i < 3; ++i) {
      d1[i] = (b1[i] - prev.b1[i]) * inv_dt;
      d2[i] = (b2[i] - prev.b2[i]) * inv_dt;
      d3[i] = (b3[i] - prev.b3[i]) * inv_dt;
    }
    rate[0] = b3[0] * d2[0] + b3[1] * d2[1] + b3[2] * d2[2];
    rate[1] = b1[0] * d3[0] + b1[1] * d3[1] + b1[2] * d3[2];
    rate[2] = b2[0] * d1[0] + b2[1] * d1[1] + b2[2] * d1[2];
  }
  for (int i = 0; i < 3; ++i) { prev.b1[i] = b1[i]; prev.b2[i] = b2[i]; prev.b3[i] = b3[i]; }
  prev.valid = true;                                                   // planner.py:650
}

template <typename R>
__global__ void __launch_bounds__(64)
extract_kernel(DevParams<R> q, int B, int ld, const R* __restrict__ T, R* __restrict__ acc,
               R* __restrict__ att, R* __restrict__ rates, R* __restrict__ thrust) {
  // write-heavy (3 rows in, 10 out per step); the thrust rows of kExtChunk steps are requested before the first use, the
  // attitude recurrence (prev_R) runs over them in order
  const LaneIdx li = lane_index<R>(B);
  if (!li.live) return;
  const unsigned voff = li.voff, rowb = (unsigned)ld * (unsigned)sizeof(R);
  const int N = q.N;
  const LaneBuf<R> tb = lane_buf(T);
  AttitudeState<R> prev;
  prev.valid = false;
  for (int i = 0; i < 3; ++i) prev.b1[i] = prev.b2[i] = prev.b3[i] = (R)0;
  constexpr int kExtChunk = 8;                             // fully unrolled below: register indices must be compile-time
  for (int k0 = 0; k0 < N; k0 += kExtChunk) {
    R tt[kExtChunk][3];
#pragma unroll
    for (int u = 0; u < kExtChunk; ++u) {
      if (k0 + u < N) {
#pragma unroll
        for (int a = 0; a < 3; ++a) tt[u][a] = lane_ld<2>(tb, voff, (unsigned)(3 * (k0 + u) + a) * rowb);
      }
    }
#pragma unroll
    for (int u = 0; u < kExtChunk; ++u) {
      if (k0 + u < N) {
        const int k = k0 + u;
        R t[3] = {tt[u][0], tt[u][1], tt[u][2]};
        R at[3], rt[3], mag;
        attitude_step<R>(t, q.inv_dt, prev, at, rt, mag);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          const unsigned r = (unsigned)(3 * k + a) * rowb;
          if (acc != nullptr) {                                                                                       // planner.py:589
            const R am = sizeof(R) == 4 ? t[a] * q.inv_mass : t[a] / q.mass;
            lane_st<2>(lane_buf(acc), voff, r, (R)(am - ((a == 2) ? q.grav : (R)0)));
          }
          if (att != nullptr) lane_st<2>(lane_buf(att), voff, r, at[a]);
          if (rates != nullptr) lane_st<2>(lane_buf(rates), voff, r, rt[a]);
        }
        if (thrust != nullptr) lane_st<2>(lane_buf(thrust), voff, (unsigned)(k) * rowb, (R)(mag));                  // planner.py:601
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// a16: is_plan_valid (planner.py:717-737)
// ------------------------------------------------------------------------------------------
template <typename R, bool HASV>
__global__ void is_plan_valid_kernel(DevParams<R> q, int B, int ld, const R* __restrict__ P, const R* __restrict__ V,
                                     int32_t* __restrict__ valid) {
  const LaneIdx li = lane_index<R>(B);
  if (!li.live) return;
  const int b = li.b;
  const unsigned voff = li.voff, rowb = (unsigned)ld * (unsigned)sizeof(R);
  const int N = q.N;
  const LaneBuf<R> pb = lane_buf(P), vb = lane_buf(HASV ? V : P);
  bool ok = true;
  // loads first, tests after, no data-dependent branch: a block of rows is in flight per lane
#pragma unroll 4
  for (int k = 0; k < N; ++k) {
    R x[3], v[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      x[a] = lane_ld<2>(pb, voff, (unsigned)(3 * k + a) * rowb);
      if constexpr (HASV) v[a] = lane_ld<2>(vb, voff, (unsigned)(3 * k + a) * rowb);
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      ok = ok & (fabs(x[a]) < (R)INFINITY);                            // planner.py:724 (NaN and +-Inf fail the comparison)
      if constexpr (HASV) ok = ok & !(fabs(v[a]) > (R)20.0);           // planner.py:734
    }
    ok = ok & !(x[2] < (R)0.1);                                        // planner.py:728
  }
  valid[b] = ok ? 1 : 0;
}

// ---- 16-byte accesses for the write-only / write-heavy streams at saturating batches: a lane owns FOUR consecutive trajectories, a wavefront
// row access is one contiguous 1 KB (tools/probes/probe_rows.hip: a bare write stream of this layout runs at 5.7-5.9 TB/s with 16 B per
// lane against 5.1-5.5 with a dword).  float only; taken when B and ld are multiples of 4, the operands 16-byte aligned and the batch fills
// the chip with a quarter of the wavefronts (kWideMinBatch); the arithmetic per trajectory is the dword kernel's, statement for statement.
__global__ void __launch_bounds__(192)
init4_kernel(DevParams<float> q, int B4, int ld4, const vf4* __restrict__ p0, const vf4* __restrict__ v0, const vf4* __restrict__ goal,
             int project, vf4* __restrict__ X) {
  int blk = blockIdx.x;
  if ((gridDim.x & 7) == 0) blk = (blk & 7) * (gridDim.x >> 3) + (blk >> 3);
  const int c = blk * kWave + (int)(threadIdx.x & (kWave - 1));       // column of four trajectories
  if (c >= B4) return;
  const int a = wave_uniform((int)(threadIdx.x / kWave));
  const int N = q.N, N3 = 3 * q.N;
  const float denom = (float)(N - 1 > 1 ? N - 1 : 1);
  const vf4 p = lane_ld4(p0 + (size_t)a * ld4 + c);
  const vf4 v = lane_ld4(v0 + (size_t)a * ld4 + c);
  const vf4 g = q.has_goal ? lane_ld4(goal + (size_t)a * ld4 + c) : p;
#pragma unroll 4
  for (int i = 0; i < N; ++i) {
    vf4 pi, vi;
    if (q.has_goal) {
      const float alpha = (float)i / denom;                                 // planner.py:344
      pi = (1.0f - alpha) * p + alpha * g;                                  // planner.py:345-347
      const vf4 dv = ((alpha - (float)(i - 1) / denom) * (g - p)) / q.dt;   // as init_kernel's float32 form
      vi = (i == 0) ? v : dv;
    } else {
      pi = p;
      vi = (i == 0) ? v : splat4(0.0f);
    }
    float ti = (a == 2) ? q.hover : 0.0f;
    if (project) {
      for (int w = 0; w < 4; ++w) { pi[w] = fminf(fmaxf(pi[w], -q.pos_b), q.pos_b); vi[w] = fminf(fmaxf(vi[w], -q.v_max), q.v_max); }
      ti = (a == 2) ? fminf(fmaxf(ti, q.tz_lo), q.tz_hi) : ti;
    }
    lane_st4(X + (size_t)(3 * i + a) * ld4 + c, pi);
    lane_st4(X + (size_t)(N3 + 3 * i + a) * ld4 + c, vi);
    lane_st4(X + (size_t)(2 * N3 + 3 * i + a) * ld4 + c, splat4(ti));
  }
}

// a9 materialised, four trajectories per lane: the N*K residual rows are the traffic (planner.py:499-514; arithmetic as obstacle_residual_kernel)
__global__ void __launch_bounds__(64)
obstacle_residual4_kernel(DevParams<float> q, int B4, int ld4, const vf4* __restrict__ X, const float* __restrict__ spheres, int K,
                          vf4* __restrict__ C, vf4* __restrict__ cmin, vf4* __restrict__ viol) {
  __shared__ float sph[SE3MPC_MAX_SPHERES * 4];
  for (int i = threadIdx.x; i < K; i += blockDim.x) {
    sph[4 * i + 0] = spheres[4 * i + 0]; sph[4 * i + 1] = spheres[4 * i + 1]; sph[4 * i + 2] = spheres[4 * i + 2];
    const float s = spheres[4 * i + 3] + q.margin;
    sph[4 * i + 3] = s * s;
  }
  __syncthreads();
  int blk = blockIdx.x;
  if ((gridDim.x & 7) == 0) blk = (blk & 7) * (gridDim.x >> 3) + (blk >> 3);
  const int c = blk * kWave + (int)threadIdx.x;
  if (c >= B4) return;
  const int N = q.N;
  vf4 mn = splat4(INFINITY), vs = splat4(0.0f);
#pragma unroll 2
  for (int k = 0; k < N; ++k) {
    const vf4 px = lane_ld4(X + (size_t)(3 * k + 0) * ld4 + c), py = lane_ld4(X + (size_t)(3 * k + 1) * ld4 + c),
              pz = lane_ld4(X + (size_t)(3 * k + 2) * ld4 + c);
    for (int j = 0; j < K; ++j) {
      const vf4 dx = px - sph[4 * j + 0], dy = py - sph[4 * j + 1], dz = pz - sph[4 * j + 2];
      const vf4 cj = (dx * dx + dy * dy + dz * dz) - sph[4 * j + 3];
      lane_st4(C + (size_t)(k * K + j) * ld4 + c, cj);
      for (int w = 0; w < 4; ++w) { mn[w] = fminf(mn[w], cj[w]); vs[w] += fmaxf(0.0f, -cj[w]); }
    }
  }
  if (cmin != nullptr) cmin[c] = mn;
  if (viol != nullptr) viol[c] = vs;
}

template <typename R>
int init_impl(const se3mpc_params* p, int B, int ld, const R* p0, const R* v0, const R* goal, int project, R* X0,
              void* stream) {
  int rc = check_lane_args(p, B, ld, 0, sizeof(R));
  if (rc) return rc;
  if (B == 0) return SE3MPC_OK;
  if (!p0 || !v0 || !X0 || (p->has_goal && !goal)) return SE3MPC_ERR_NULL;
  if constexpr (sizeof(R) == 4) {
    if (wide_ok(B, ld, {p0, v0, goal, X0})) {
      hipLaunchKernelGGL(init4_kernel, dim3(grid_for(B / 4, kWave)), dim3(192), 0, (hipStream_t)stream, make_dev_params<float>(*p), B / 4, ld / 4,
                         reinterpret_cast<const vf4*>(p0), reinterpret_cast<const vf4*>(v0), reinterpret_cast<const vf4*>(goal), project,
                         reinterpret_cast<vf4*>(X0));
      return launch_status("se3mpc_init");
    }
  }
  hipLaunchKernelGGL(init_kernel<R>, dim3(grid_for(B, kWave)), dim3(192), 0, (hipStream_t)stream,
                     make_dev_params<R>(*p), B, ld, p0, v0, goal, project, X0);
  return launch_status("se3mpc_init");
}

template <typename R>
int cost_grad_impl(const se3mpc_params* p, int B, int ld, const R* X, const R* goal, R* f, R* g, void* stream) {
  int rc = check_lane_args(p, B, ld, 0, sizeof(R));
  if (rc) return rc;
  if (B == 0) return SE3MPC_OK;
  if (!X || !f || (p->has_goal && !goal)) return SE3MPC_ERR_NULL;
  if ((uint64_t)9 * p->horizon * (uint64_t)ld * sizeof(R) >= (1ull << 32)) return SE3MPC_ERR_SHAPE;   // 32-bit buffer offsets
  if (g != nullptr)
    hipLaunchKernelGGL((cost_grad_kernel<R, true>), dim3(grid_for(B, kWave)), dim3(192), 0, (hipStream_t)stream, make_dev_params<R>(*p), B, ld, X,
                       goal, f, g);
  else
    hipLaunchKernelGGL((cost_grad_kernel<R, false>), dim3(grid_for(B, kWave)), dim3(192), 0, (hipStream_t)stream, make_dev_params<R>(*p), B, ld, X,
                       goal, f, g);
  return launch_status("se3mpc_cost_grad");
}

template <typename R>
int dynamics_residual_impl(const se3mpc_params* p, int B, int ld, const R* X, const R* p0, const R* v0, R* Rout,
                           void* stream) {
  int rc = check_lane_args(p, B, ld, 0, sizeof(R));
  if (rc) return rc;
  if (B == 0) return SE3MPC_OK;
  if (!X || !p0 || !v0 || !Rout) return SE3MPC_ERR_NULL;
  hipLaunchKernelGGL(dynamics_residual_kernel<R>, dim3(grid_for(B, kWave)), dim3(192), 0,
                     (hipStream_t)stream, make_dev_params<R>(*p), B, ld, X, p0, v0, Rout);
  return launch_status("se3mpc_dynamics_residual");
}

template <typename R>
int obstacle_residual_impl(const se3mpc_params* p, int B, int ld, const R* X, const R* spheres, int K, R* C, R* cmin,
                           R* viol, void* stream) {
  if (K < 0 || K > SE3MPC_MAX_SPHERES) return SE3MPC_ERR_SHAPE;
  int rc = check_lane_args(p, B, ld, p ? std::max(9LL * p->horizon, (long long)p->horizon * K) : 0, sizeof(R));
  if (rc) return rc;
  if (B == 0) return SE3MPC_OK;
  if (!X || (K > 0 && !spheres)) return SE3MPC_ERR_NULL;
  if (C == nullptr)
    hipLaunchKernelGGL(obstacle_reduce_kernel<R>, dim3(grid_for(B, kLaneBlock)), dim3(kLaneBlock), 0, (hipStream_t)stream,
                       make_dev_params<R>(*p), B, ld, X, spheres, K, cmin, viol);
  else {
    if constexpr (sizeof(R) == 4) {
      if (wide_ok(B, ld, {X, C, cmin, viol})) {
        hipLaunchKernelGGL(obstacle_residual4_kernel, dim3(grid_for(B / 4, kLaneBlock)), dim3(kLaneBlock), 0, (hipStream_t)stream,
                           make_dev_params<float>(*p), B / 4, ld / 4, reinterpret_cast<const vf4*>(X), spheres, K, reinterpret_cast<vf4*>(C),
                           reinterpret_cast<vf4*>(cmin), reinterpret_cast<vf4*>(viol));
        return launch_status("se3mpc_obstacle_residual");
      }
    }
    hipLaunchKernelGGL(obstacle_residual_kernel<R>, dim3(grid_for(B, kLaneBlock)), dim3(kLaneBlock), 0,
                       (hipStream_t)stream, make_dev_params<R>(*p), B, ld, X, spheres, K, C, cmin, viol);
  }
  return launch_status("se3mpc_obstacle_residual");
}

template <typename R>
int physical_constraints_impl(const se3mpc_params* p, int B, int ld, const R* X, R* C, void* stream) {
  int rc = check_lane_args(p, B, ld, 0, sizeof(R));
  if (rc) return rc;
  if (B == 0) return SE3MPC_OK;
  if (!X || !C) return SE3MPC_ERR_NULL;
  hipLaunchKernelGGL(physical_constraints_kernel<R>, dim3(grid_for(B, kLaneBlock)), dim3(kLaneBlock), 0,
                     (hipStream_t)stream, make_dev_params<R>(*p), B, ld, X, C);
  return launch_status("se3mpc_physical_constraints");
}

template <typename R>
int extract_impl(const se3mpc_params* p, int B, int ld, const R* T, R* acc, R* att, R* rates, R* thrust, void* stream) {
  int rc = check_lane_args(p, B, ld, 0, sizeof(R));
  if (rc) return rc;
  if (B == 0) return SE3MPC_OK;
  if (!T) return SE3MPC_ERR_NULL;
  hipLaunchKernelGGL(extract_kernel<R>, dim3(grid_for(B, kLaneBlock)), dim3(kLaneBlock), 0, (hipStream_t)stream,
                     make_dev_params<R>(*p), B, ld, T, acc, att, rates, thrust);
  return launch_status("se3mpc_extract");
}

template <typename R>
int is_plan_valid_impl(const se3mpc_params* p, int B, int ld, const R* P, const R* V, int32_t* valid, void* stream) {
  int rc = check_lane_args(p, B, ld, 0, sizeof(R));
  if (rc) return rc;
  if (B == 0) return SE3MPC_OK;
  if (!P || !valid) return SE3MPC_ERR_NULL;
  if (V != nullptr)
    hipLaunchKernelGGL((is_plan_valid_kernel<R, true>), dim3(grid_for(B, kLaneBlock)), dim3(kLaneBlock), 0, (hipStream_t)stream,
                       make_dev_params<R>(*p), B, ld, P, V, valid);
  else
    hipLaunchKernelGGL((is_plan_valid_kernel<R, false>), dim3(grid_for(B, kLaneBlock)), dim3(kLaneBlock), 0, (hipStream_t)stream,
                       make_dev_params<R>(*p), B, ld, P, V, valid);
  return launch_status("se3mpc_is_plan_valid");
}

}  // namespace se3mpc

using namespace se3mpc;   // C ABI (include/se3mpc.h)

extern "C" int se3mpc_init_f32(const se3mpc_params* p, int B, int ld, const float* p0, const float* v0, const float* goal, int project, float* X0,
                               void* stream) {
  return init_impl<float>(p, B, ld, p0, v0, goal, project, X0, stream);
}
extern "C" int se3mpc_init_f64(const se3mpc_params* p, int B, int ld, const double* p0, const double* v0, const double* goal, int project, double* X0,
                               void* stream) {
  return init_impl<double>(p, B, ld, p0, v0, goal, project, X0, stream);
}
extern "C" int se3mpc_cost_grad_f32(const se3mpc_params* p, int B, int ld, const float* X, const float* goal, float* f, float* g, void* stream) {
  return cost_grad_impl<float>(p, B, ld, X, goal, f, g, stream);
}
extern "C" int se3mpc_cost_grad_f64(const se3mpc_params* p, int B, int ld, const double* X, const double* goal, double* f, double* g, void* stream) {
  return cost_grad_impl<double>(p, B, ld, X, goal, f, g, stream);
}
extern "C" int se3mpc_dynamics_residual_f32(const se3mpc_params* p, int B, int ld, const float* X, const float* p0, const float* v0, float* Rout,
                                            void* stream) {
  return dynamics_residual_impl<float>(p, B, ld, X, p0, v0, Rout, stream);
}
extern "C" int se3mpc_dynamics_residual_f64(const se3mpc_params* p, int B, int ld, const double* X, const double* p0, const double* v0, double* Rout,
                                            void* stream) {
  return dynamics_residual_impl<double>(p, B, ld, X, p0, v0, Rout, stream);
}
extern "C" int se3mpc_obstacle_residual_f32(const se3mpc_params* p, int B, int ld, const float* X, const float* spheres, int K, float* C, float* cmin,
                                            float* viol, void* stream) {
  return obstacle_residual_impl<float>(p, B, ld, X, spheres, K, C, cmin, viol, stream);
}
extern "C" int se3mpc_obstacle_residual_f64(const se3mpc_params* p, int B, int ld, const double* X, const double* spheres, int K, double* C,
                                            double* cmin, double* viol, void* stream) {
  return obstacle_residual_impl<double>(p, B, ld, X, spheres, K, C, cmin, viol, stream);
}
extern "C" int se3mpc_physical_constraints_f32(const se3mpc_params* p, int B, int ld, const float* X, float* C, void* stream) {
  return physical_constraints_impl<float>(p, B, ld, X, C, stream);
}
extern "C" int se3mpc_physical_constraints_f64(const se3mpc_params* p, int B, int ld, const double* X, double* C, void* stream) {
  return physical_constraints_impl<double>(p, B, ld, X, C, stream);
}
extern "C" int se3mpc_extract_f32(const se3mpc_params* p, int B, int ld, const float* T, float* acc, float* att, float* rates, float* thrust,
                                  void* stream) {
  return extract_impl<float>(p, B, ld, T, acc, att, rates, thrust, stream);
}
extern "C" int se3mpc_extract_f64(const se3mpc_params* p, int B, int ld, const double* T, double* acc, double* att, double* rates, double* thrust,
                                  void* stream) {
  return extract_impl<double>(p, B, ld, T, acc, att, rates, thrust, stream);
}
extern "C" int se3mpc_is_plan_valid_f32(const se3mpc_params* p, int B, int ld, const float* P, const float* V, int32_t* valid, void* stream) {
  return is_plan_valid_impl<float>(p, B, ld, P, V, valid, stream);
}
extern "C" int se3mpc_is_plan_valid_f64(const se3mpc_params* p, int B, int ld, const double* P, const double* V, int32_t* valid, void* stream) {
  return is_plan_valid_impl<double>(p, B, ld, P, V, valid, stream);
}
