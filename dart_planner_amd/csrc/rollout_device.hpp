// rollout_device.hpp -- device code shared by the shooting-form kernels: rollout.hip (the plain rollout), rollout_obstacles.hip (fused with
// the sphere residuals) and rollout_iterate.hip (the on-device iteration loops).  The per-axis sweeps and the epilogue are the same
// expressions in all three, so they agree bit for bit wherever they take the same sweep.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "se3mpc_common.hpp"
#include <se3mpc_wave_ops.hpp>

namespace se3mpc {

// ------------------------------------------------------------------------------------------
// Shooting form: forward rollout (the recurrence of planner.py:449-460), objective of
// planner.py:516-550 on the rolled-out states, exact gradient wrt T by the reverse sweep.
// The three axes are independent double integrators and the cost is separable in them, so a
// lane processes one axis at a time: only one axis' T_k, P_k, V_k are live.
//
// Three variants of the same arithmetic (selected by se3mpc_set_rollout_variant, default
// chosen from measurements):
//   REG  exact-N register arrays (t[N], ps[N], vs[N]); instantiated for the BASELINE horizons.
//   LDS  any N: per-step state tiles P_k,V_k staged in LDS as [k][lane] (bank = lane, conflict
//        free), re-read by the reverse sweep; T_k re-read from L1/L2.
//   REV  any N: O(1) registers; the reverse sweep re-reads T_k (L2) and inverts the recurrence
//        (V_k = V_{k+1} - a_k dt, P_k = P_{k+1} - V_k dt - a_k dt^2/2) instead of storing states.
// ------------------------------------------------------------------------------------------

// Epilogue shared by the variants: store the cost and, if `wave_keys` is given, this wavefront's best
// (cost, index) as a packed key -- a DPP min over the 64 lanes (wavefront-shuffle reduction, no LDS)
// and ONE plain 8-byte store per wavefront into its own slot.  No atomics: 128 wavefronts hammering
// one word (or 64 batches' words in four cache lines) serialise in L2 at ~11 ns each, which measured
// 2.8x on a 64-batch launch; se3mpc_reduce_keys folds the slots afterwards, once per bucket.
// Tail lanes (b >= B) stay active up to here so the cross-lane ops see all 64 lanes; they contribute
// the identity.
template <typename R, bool SHARED_SLOT = false>
__device__ __forceinline__ void rollout_epilogue(bool live, int b, R c, R* __restrict__ cost,
                                                 unsigned long long* __restrict__ wave_key_slot, uint32_t index_base) {
  if (live) cost[b] = c;
  const uint32_t bits = live ? orderable_bits((float)c) : 0xFFFFFFFFu;
  const uint32_t m = wave_min_u32(bits);
  const int src = first_lane(wave_ballot(live && bits == m));
  if (wave_key_slot != nullptr && src >= 0 && lane_id() == src) {
    const unsigned long long k = ((unsigned long long)m << 32) | (unsigned long long)(index_base + (uint32_t)b);
    if constexpr (SHARED_SLOT) atomicMin(wave_key_slot, k);   // several workgroups per slot (preset to ~0 by the launcher); min is order-free
    else *wave_key_slot = k;
  }
}

template <typename R>
struct RolloutSums {
  R sp, sv, sa, st, sterm;
};

template <typename R>
__device__ __forceinline__ R rollout_total(const DevParams<R>& q, const RolloutSums<R>& s) {
  R c = q.wv * s.sv + q.wa * s.sa + q.wT * s.st;
  if (q.has_goal) c += q.wp * s.sp + q.term * q.wp * s.sterm;
  return c;
}

// Per-axis constants of the sweeps, hoisted out of the k loops.
template <typename R>
struct AxisConsts {
  R gl, grav, hov, two_wp, two_wv, c_aa, c_tt, c_lp, c_lv;
};

template <typename R>
__device__ __forceinline__ AxisConsts<R> axis_consts(const DevParams<R>& q, int a, R gl) {
  AxisConsts<R> c;
  c.gl = gl;
  c.grav = (a == 2) ? q.grav : (R)0;
  c.hov = (a == 2) ? q.hover : (R)0;
  c.two_wp = q.has_goal ? (R)2 * q.wp : (R)0;
  c.two_wv = (R)2 * q.wv;
  c.c_aa = (R)2 * q.wa * q.inv_mass;        // d(wa*acc^2)/dT
  c.c_tt = (R)2 * q.wT;                     // d(wT*(T-hover)^2)/dT
  c.c_lp = q.half_dt2 * q.inv_mass;         // dP_{k+1}/dT_k
  c.c_lv = q.dt * q.inv_mass;               // dV_{k+1}/dT_k
  return c;
}

// Weighted cost of ONE axis from its five sums of squares.
template <typename R>
__device__ __forceinline__ R axis_cost(const DevParams<R>& q, const RolloutSums<R>& s) {
  R c = q.wv * s.sv + q.wa * s.sa + q.wT * s.st;
  if (q.has_goal) c += q.wp * (s.sp + q.term * s.sterm);
  return c;
}

// One axis of one trajectory with exact-N register arrays.  Loads of all N thrust rows are issued
// back to back (N independent HBM requests in flight per lane) before the first use.
template <typename R, int N, bool GRAD, bool STATES, int LDAUX = 0, int STAUX = 0, bool TILE = false, bool EXACT = true, bool MIDSYNC = false>
__device__ __forceinline__ R rollout_axis_reg(const DevParams<R>& q, int a, unsigned voff, unsigned rowb, const R* __restrict__ p0,
                                              const R* __restrict__ v0, const R* __restrict__ goal,
                                              const R* __restrict__ T, R* __restrict__ gradT, R* __restrict__ Pout,
                                              R* __restrict__ Vout, R* __restrict__ ptile = nullptr) {
  // N is the compile-time register bound.  EXACT: the horizon equals N (no guards).  !EXACT: the horizon is
  // q.N <= N and every step is guarded by a wave-uniform (scalar) branch -- the bucketed fallback
  // (N in {16, 32, 64}) that keeps exact states and all loads in flight for any horizon.
  const int Nn = EXACT ? N : q.N;
  R t[N], es[N], vs[N];
#pragma unroll
  for (int k = 0; k < N; ++k) {
    if (EXACT || k < Nn) t[k] = lane_ld<LDAUX>(lane_buf(T), voff, (unsigned)(3 * k + a) * rowb);
  }
  const AxisConsts<R> c = axis_consts<R>(q, a, q.has_goal ? lane_ld(lane_buf(goal), voff, (unsigned)(a) * rowb) : (R)0);
  R p = lane_ld(lane_buf(p0), voff, (unsigned)(a) * rowb);
  R v = lane_ld(lane_buf(v0), voff, (unsigned)(a) * rowb);
  RolloutSums<R> s = {0, 0, 0, 0, 0};
#pragma unroll
  for (int k = 0; k < N; ++k) {
    if (EXACT || k < Nn) {
      const R acc = t[k] * q.inv_mass - c.grav;
      const R dev = t[k] - c.hov;
      const R e = p - c.gl;
      es[k] = e; vs[k] = v;
      if (TILE) ptile[k * kWave] = p;                        // per-step position tile in LDS (obstacle fusion)
      if (k == Nn - 1) s.sterm = e * e; else s.sp += e * e;
      s.sv += v * v; s.sa += acc * acc; s.st += dev * dev;
      if (STATES) {
        lane_st(lane_buf(Pout), voff, (unsigned)(3 * k + a) * rowb, p);
        lane_st(lane_buf(Vout), voff, (unsigned)(3 * k + a) * rowb, v);
      }
      p = p + v * q.dt + q.half_dt2 * acc;                   // planner.py:450-455 solved for P_{k+1}
      v = v + acc * q.dt;                                    // planner.py:459 solved for V_{k+1}
    }
  }
  if (MIDSYNC) __syncthreads();                              // the position tile is complete: helper wavefronts start on it during the adjoint sweep
  s.sp += s.sterm;
  if (GRAD) {
    R lamP = (R)0, lamV = (R)0;
#pragma unroll
    for (int k = N - 1; k >= 0; --k) {
      if (EXACT || k < Nn) {
        const R acc = t[k] * q.inv_mass - c.grav;
        const R dev = t[k] - c.hov;
        if (k == Nn - 1) {
          lane_st<STAUX>(lane_buf(gradT), voff, (unsigned)(3 * k + a) * rowb, c.c_aa * acc + c.c_tt * dev);
          lamP = c.two_wp * ((R)1 + q.term) * es[k];
          lamV = c.two_wv * vs[k];
        } else {
          lane_st<STAUX>(lane_buf(gradT), voff, (unsigned)(3 * k + a) * rowb, c.c_aa * acc + c.c_tt * dev + c.c_lp * lamP + c.c_lv * lamV);
          lamV = c.two_wv * vs[k] + q.dt * lamP + lamV;
          lamP = c.two_wp * es[k] + lamP;
        }
      }
    }
  }
  return axis_cost(q, s);
}

// Any N, O(1) registers: the reverse sweep re-reads T_k (L2) and walks the states backwards
// through the inverted recurrence instead of storing them.
template <typename R, bool GRAD, bool STATES, int STAUX = 0, bool TILE = false, bool MIDSYNC = false>
__device__ __forceinline__ R rollout_axis_rev(const DevParams<R>& q, int a, unsigned voff, unsigned rowb, const R* __restrict__ p0,
                                              const R* __restrict__ v0, const R* __restrict__ goal,
                                              const R* __restrict__ T, R* __restrict__ gradT, R* __restrict__ Pout,
                                              R* __restrict__ Vout, R* __restrict__ ptile = nullptr) {
  const int N = q.N;
  const AxisConsts<R> c = axis_consts<R>(q, a, q.has_goal ? lane_ld(lane_buf(goal), voff, (unsigned)(a) * rowb) : (R)0);
  R p = lane_ld(lane_buf(p0), voff, (unsigned)(a) * rowb);
  R v = lane_ld(lane_buf(v0), voff, (unsigned)(a) * rowb);
  RolloutSums<R> s = {0, 0, 0, 0, 0};
  R tk = (R)0, pl = p, vl = v;
#pragma unroll 6
  for (int k = 0; k < N; ++k) {
    tk = lane_ld(lane_buf(T), voff, (unsigned)(3 * k + a) * rowb);
    const R acc = tk * q.inv_mass - c.grav;
    const R dev = tk - c.hov;
    const R e = p - c.gl;
    if (TILE) ptile[k * kWave] = p;
    if (k == N - 1) s.sterm = e * e; else s.sp += e * e;
    s.sv += v * v; s.sa += acc * acc; s.st += dev * dev;
    if (STATES) {
      lane_st(lane_buf(Pout), voff, (unsigned)(3 * k + a) * rowb, p);
      lane_st(lane_buf(Vout), voff, (unsigned)(3 * k + a) * rowb, v);
    }
    pl = p; vl = v;                                         // state at step k (P_{N-1}, V_{N-1} after the loop)
    p = p + v * q.dt + q.half_dt2 * acc;
    v = v + acc * q.dt;
  }
  if (MIDSYNC) __syncthreads();                             // as in rollout_axis_reg
  s.sp += s.sterm;
  if (GRAD) {
    R lamP = c.two_wp * ((R)1 + q.term) * (pl - c.gl);
    R lamV = c.two_wv * vl;
    lane_st<STAUX>(lane_buf(gradT), voff, (unsigned)(3 * (N - 1) + a) * rowb, c.c_aa * (tk * q.inv_mass - c.grav) + c.c_tt * (tk - c.hov));
    R pk = pl, vk = vl;
#pragma unroll 6
    for (int k = N - 2; k >= 0; --k) {
      const R t = lane_ld(lane_buf(T), voff, (unsigned)(3 * k + a) * rowb);
      const R acc = t * q.inv_mass - c.grav;
      const R dev = t - c.hov;
      vk = vk - acc * q.dt;                                 // V_k from V_{k+1}
      pk = pk - vk * q.dt - q.half_dt2 * acc;               // P_k from P_{k+1}
      lane_st<STAUX>(lane_buf(gradT), voff, (unsigned)(3 * k + a) * rowb, c.c_aa * acc + c.c_tt * dev + c.c_lp * lamP + c.c_lv * lamV);
      lamV = c.two_wv * vk + q.dt * lamP + lamV;
      lamP = c.two_wp * (pk - c.gl) + lamP;
    }
  }
  return axis_cost(q, s);
}

// float32 sphere sweeps evaluate two spheres per instruction (v_pk_add/mul/fma_f32)
typedef float obs_f2 __attribute__((vector_size(8)));
#ifndef SE3MPC_OBS_PACKED
#define SE3MPC_OBS_PACKED 1
#endif
template <typename R> constexpr bool kObsPacked = sizeof(R) == 4 && SE3MPC_OBS_PACKED;

}  // namespace se3mpc
