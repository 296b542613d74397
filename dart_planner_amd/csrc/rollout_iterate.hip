// rollout_iterate.hip -- K iterations of the shooting form in one launch (se3mpc_rollout_iterate_*, se3mpc_rollout_iterate_obstacles_*) and
// the stand-alone projected step (se3mpc_projected_step_*).  The rollout sums, constants and epilogue are rollout_device.hpp's.
#include "lane_common.hpp"
#include "rollout_device.hpp"

namespace se3mpc {

// ------------------------------------------------------------------------------------------
// K iterations of the shooting form in ONE launch: projected gradient descent on the thrust
// sequence of every trajectory,
//     T <- clip(T - step * dcost/dT, thrust box of planner.py:390-400),
// `iters` times, then one last evaluation of (cost, gradient) at the final T.  A launch of the plain rollout kernel costs
// ~4.4 us for an 8192-trajectory batch whatever it does (6 MB = 1 us of HBM time; the rest is launch + the load -> 60
// dependent steps -> store chain), so a sampling / descent loop driven from the host pays that per iteration.  Here the
// thrust sequence of a lane stays in REGISTERS between iterations: iteration 0 reads T (3N rows), the last one writes T and
// the gradient; the iterations in between touch no memory at all.  The three axes are independent double integrators, the
// cost is separable in them and the box is per axis, so the three axis wavefronts of a workgroup iterate without ever
// talking to each other; their partial costs meet in LDS once, for the final cost and the fused argmin key.
// The gradient of step k is consumed in place: once the reverse sweep has produced g_k it no longer needs T_k (the adjoint
// recurrences run on the stored states), so T_k is overwritten right there -- no gradient array, no second pass.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ float fma_r(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_r(double a, double b, double c) { return __builtin_fma(a, b, c); }
// clamp(x, lo, hi) for lo <= hi as ONE instruction (v_med3): the median of (x, lo, hi); a NaN x comes back as lo or hi like fmin(fmax())
__device__ __forceinline__ float clamp_r(float x, float lo, float hi) { return __builtin_amdgcn_fmed3f(x, lo, hi); }
__device__ __forceinline__ double clamp_r(double x, double lo, double hi) { return fmin(fmax(x, lo), hi); }
// the same expression in the stand-alone step kernel and in the memory-resident fallback: one fused multiply-add, then the box
template <typename R>
__device__ __forceinline__ R projected_update(R t, R g, R step, R lo, R hi) {
  return fmin(fmax(fma_r(-step, g, t), lo), hi);
}

// ---- obstacle-aware iterations (BASELINE config 3 inside the iteration loop) ---------------------------------------------
// The build's EXTENSION of the shooting objective (the reference builds the sphere residuals c_kj = |P_k - c_j|^2 - (r_j + margin)^2,
// planner.py:499-514, and never hands them to its solver, :250 vs :256-268; its obstacle_weight, :63, is never read):
//     penalty = w_obs * sum_k sum_j max(0, -c_kj)^2          on the rolled-out positions,
// whose gradient wrt P_k, -4 w_obs sum_j max(0, -c_kj) (P_k - c_j), joins the adjoint of the position in the reverse sweep.
// The penalty couples the three axes, so an iteration becomes: axis wavefronts roll out and stage P_k in the LDS tile
// [axis][k][lane] -> barrier -> ALL W wavefronts of the workgroup split the steps (k = w, w + W, ...), evaluate the N*K
// distances against the LDS-resident sphere table and overwrite P_k IN PLACE with dpenalty/dP_k -> barrier -> axis wavefronts
// run the adjoint sweep reading their component back.  Thrusts, states and the per-step obstacle gradients never touch HBM.
template <typename R>
struct ObsCtx {
  R* tile;            // [3][N][64]
  const R* sph;       // [Kpad][4] = (cx, cy, cz, (r + margin)^2), padding rows -inf
  R* pen;             // [W][64]: each wavefront's share of the penalty, last pass
  R* pen_first;       // [W][64]: the same at the first pass (cost at T_in)
  int Kpad;
  bool axis_sweeps;   // false: the axis wavefronts only meet the barriers, the helpers (wavefronts 3 .. W-1) take every step between them
  int slot, slots;    // this lane's share of the steps: k = slot, slot + slots, ...  (TS = 32 trajectories per workgroup: a wavefront's two
                      // halves take different steps of the same 32 trajectories)
  R w_obs;
};

// Two spheres against one position, both sweeps (table in LDS / table in registers) through this one expression so that they agree bit for bit.
// PEN = false (descent passes, whose penalty nobody reads): the gradient only.
template <bool PEN = true>
__device__ __forceinline__ void sphere_pair(obs_f2 px2, obs_f2 py2, obs_f2 pz2, obs_f2 cx, obs_f2 cy, obs_f2 cz, obs_f2 r2, obs_f2& pk, obs_f2& qx,
                                            obs_f2& qy, obs_f2& qz) {
  const obs_f2 dx = px2 - cx, dy = py2 - cy, dz = pz2 - cz;
  const obs_f2 c = dz * dz + (dy * dy + (dx * dx - r2));        // three fused multiply-adds (a padding row's r2 = -inf gives c = +inf, h = 0)
  const obs_f2 h = obs_f2{fmaxf(0.0f, -c[0]), fmaxf(0.0f, -c[1])};
  if constexpr (PEN) pk += h * h;
  qx += h * dx; qy += h * dy; qz += h * dz;
}
template <typename R, bool PEN = true>
__device__ __forceinline__ void sphere_one(R px, R py, R pz, R cx, R cy, R cz, R r2, R& pk, R& qx, R& qy, R& qz) {
  const R dx = px - cx, dy = py - cy, dz = pz - cz;
  const R c = dz * dz + (dy * dy + (dx * dx - r2));
  const R h = fmax((R)0, -c);
  if constexpr (PEN) pk += h * h;
  qx += h * dx; qy += h * dy; qz += h * dz;
}

// steps k = first, first + stride, ... of every lane's trajectory: tile holds P_k on entry and dpenalty/dP_k on exit; returns this
// wavefront's share of the penalty (already weighted)
template <typename R, int TS>
__device__ __forceinline__ R obstacle_penalty_sweep(R* __restrict__ tile, const R* __restrict__ sph, int Nn, int Kpad, int first, int stride, int lane,
                                                    R w_obs) {
  R pen = (R)0;
  const R scale = (R)-4 * w_obs;
  lane &= TS - 1;
  for (int k = first; k < Nn; k += stride) {
    R* tx = tile + ((size_t)0 * Nn + k) * kWave + lane;
    R* ty = tile + ((size_t)1 * Nn + k) * kWave + lane;
    R* tz = tile + ((size_t)2 * Nn + k) * kWave + lane;
    const R px = *tx, py = *ty, pz = *tz;
    if constexpr (kObsPacked<R>) {
      const obs_f2 px2 = {px, px}, py2 = {py, py}, pz2 = {pz, pz}, zero = {0.0f, 0.0f};
      obs_f2 qx = zero, qy = zero, qz = zero, pk = zero;
#pragma unroll 4
      for (int j = 0; j < Kpad; j += 2) {                      // two spheres per packed instruction (Kpad is a multiple of 8)
        const R* s0 = sph + 4 * j;
        sphere_pair(px2, py2, pz2, obs_f2{s0[0], s0[4]}, obs_f2{s0[1], s0[5]}, obs_f2{s0[2], s0[6]}, obs_f2{s0[3], s0[7]}, pk, qx, qy, qz);
      }
      pen += pk[0] + pk[1];
      *tx = scale * (qx[0] + qx[1]); *ty = scale * (qy[0] + qy[1]); *tz = scale * (qz[0] + qz[1]);
    } else {
      R qx = (R)0, qy = (R)0, qz = (R)0, pk = (R)0;
      for (int j = 0; j < Kpad; ++j) {
        const R* s0 = sph + 4 * j;
        sphere_one<R>(px, py, pz, s0[0], s0[1], s0[2], s0[3], pk, qx, qy, qz);
      }
      pen += pk;
      *tx = scale * qx; *ty = scale * qy; *tz = scale * qz;
    }
  }
  return w_obs * pen;
}

// The helpers' sweep: the 8 * KP spheres live in REGISTERS for the whole launch (a helper wavefront holds nothing else), so a step costs
// its 6.5 VALU instructions per sphere and no LDS broadcast reads (with one wavefront per SIMD nothing hides their latency: measured
// 1300 cycles per step with the table in LDS against 450 for the arithmetic); the next step's position is fetched under the current one's
// arithmetic.  Same expression, same order as obstacle_penalty_sweep.
template <typename R, int KP>
struct SphereRegs {
  static constexpr int kPairs = kObsPacked<R> ? 4 * KP : 1, kOnes = kObsPacked<R> ? 1 : 8 * KP;
  obs_f2 cx2[kPairs], cy2[kPairs], cz2[kPairs], r22[kPairs];
  R cx[kOnes], cy[kOnes], cz[kOnes], r2[kOnes];
  __device__ __forceinline__ void load(const R* __restrict__ sph) {
    if constexpr (kObsPacked<R>) {
#pragma unroll
      for (int i = 0; i < kPairs; ++i) {
        const R* s0 = sph + 8 * i;
        cx2[i] = obs_f2{s0[0], s0[4]}; cy2[i] = obs_f2{s0[1], s0[5]}; cz2[i] = obs_f2{s0[2], s0[6]}; r22[i] = obs_f2{s0[3], s0[7]};
      }
    } else {
#pragma unroll
      for (int i = 0; i < kOnes; ++i) { cx[i] = sph[4 * i]; cy[i] = sph[4 * i + 1]; cz[i] = sph[4 * i + 2]; r2[i] = sph[4 * i + 3]; }
    }
  }
};

template <typename R, int KP, int U, int TS, bool PEN>
__device__ __forceinline__ R obstacle_penalty_sweep_regs(R* __restrict__ tile, const SphereRegs<R, KP>& sr, int Nn, int first, int stride, int lane,
                                                         R w_obs) {
  // U steps in flight: a packed float instruction's result is ready for a dependent one only ~8 cycles after issue, and a helper has its
  // SIMD to itself -- the distance chains of U different steps interleave and fill those slots.
  R pen = (R)0;
  const R scale = (R)-4 * w_obs;
  lane &= TS - 1;
#pragma unroll 1
  for (int k0 = first; k0 < Nn; k0 += U * stride) {
    R px[U], py[U], pz[U];
    R* tx[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k = k0 + u * stride;
      tx[u] = tile + (size_t)(k < Nn ? k : k0) * kWave + lane;
      px[u] = tx[u][0]; py[u] = tx[u][(size_t)Nn * kWave]; pz[u] = tx[u][(size_t)2 * Nn * kWave];
    }
    if constexpr (kObsPacked<R>) {
      const obs_f2 zero = {0.0f, 0.0f};
      obs_f2 px2[U], py2[U], pz2[U], qx[U], qy[U], qz[U], pk[U];
#pragma unroll
      for (int u = 0; u < U; ++u) { px2[u] = obs_f2{px[u], px[u]}; py2[u] = obs_f2{py[u], py[u]}; pz2[u] = obs_f2{pz[u], pz[u]}; qx[u] = qy[u] = qz[u] = pk[u] = zero; }
#pragma unroll
      for (int i = 0; i < SphereRegs<R, KP>::kPairs; ++i) {
#pragma unroll
        for (int u = 0; u < U; ++u) sphere_pair<PEN>(px2[u], py2[u], pz2[u], sr.cx2[i], sr.cy2[i], sr.cz2[i], sr.r22[i], pk[u], qx[u], qy[u], qz[u]);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (k0 + u * stride < Nn) {
          pen += pk[u][0] + pk[u][1];
          tx[u][0] = scale * (qx[u][0] + qx[u][1]); tx[u][(size_t)Nn * kWave] = scale * (qy[u][0] + qy[u][1]);
          tx[u][(size_t)2 * Nn * kWave] = scale * (qz[u][0] + qz[u][1]);
        }
      }
    } else {
      R qx[U], qy[U], qz[U], pk[U];
#pragma unroll
      for (int u = 0; u < U; ++u) qx[u] = qy[u] = qz[u] = pk[u] = (R)0;
#pragma unroll
      for (int i = 0; i < SphereRegs<R, KP>::kOnes; ++i) {
#pragma unroll
        for (int u = 0; u < U; ++u) sphere_one<R, PEN>(px[u], py[u], pz[u], sr.cx[i], sr.cy[i], sr.cz[i], sr.r2[i], pk[u], qx[u], qy[u], qz[u]);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (k0 + u * stride < Nn) {
          pen += pk[u];
          tx[u][0] = scale * qx[u]; tx[u][(size_t)Nn * kWave] = scale * qy[u]; tx[u][(size_t)2 * Nn * kWave] = scale * qz[u];
        }
      }
    }
  }
  return w_obs * pen;
}

// one exchange of an obstacle-aware pass, executed by EVERY wavefront of the workgroup (axis wavefronts from inside their sweeps,
// the helper wavefronts from the kernel body): barrier, this wavefront's share of the sweep, barrier
template <typename R, int TS = kWave>
__device__ __forceinline__ void obstacle_exchange(const ObsCtx<R>& o, int Nn, int w, int lane, bool first) {
  __syncthreads();
  R pen = (R)0;
  if (o.axis_sweeps || w >= 3) pen = obstacle_penalty_sweep<R, TS>(o.tile, o.sph, Nn, o.Kpad, o.slot, o.slots, lane, o.w_obs);
  o.pen[w * kWave + lane] = pen;
  if (first) o.pen_first[w * kWave + lane] = pen;
  __syncthreads();
}

#ifndef SE3MPC_OBS_STEPS_IN_FLIGHT
#define SE3MPC_OBS_STEPS_IN_FLIGHT 2
#endif
// the helpers' passes with the sphere table in registers
template <typename R, int KP, int TS>
__device__ __forceinline__ void helper_passes_regs(const ObsCtx<R>& o, int Nn, int w, int lane, int passes) {
  SphereRegs<R, KP> sr;
  sr.load(o.sph);
#pragma unroll 1
  for (int ps = 0; ps < passes; ++ps) {
    __syncthreads();
    R pen = (R)0;                                             // (only the first and the last pass' penalties are ever read)
    if (ps == 0 || ps == passes - 1) pen = obstacle_penalty_sweep_regs<R, KP, SE3MPC_OBS_STEPS_IN_FLIGHT, TS, true>(o.tile, sr, Nn, o.slot, o.slots, lane, o.w_obs);
    else (void)obstacle_penalty_sweep_regs<R, KP, SE3MPC_OBS_STEPS_IN_FLIGHT, TS, false>(o.tile, sr, Nn, o.slot, o.slots, lane, o.w_obs);
    o.pen[w * kWave + lane] = pen;
    if (ps == 0) o.pen_first[w * kWave + lane] = pen;
    __syncthreads();
  }
}

template <typename R, int N, bool EXACT, int LDAUX, int STAUX, bool OBS = false, int TS = kWave>
__device__ __forceinline__ R iterate_axis_reg(const DevParams<R>& q, int a, unsigned voff, unsigned rowb, const R* __restrict__ p0,
                                              const R* __restrict__ v0, const R* __restrict__ goal, const R* __restrict__ Tin,
                                              R* __restrict__ Tout, R* __restrict__ gradT, int iters, R step, bool live, bool want_first,
                                              R& cost_first, const ObsCtx<R>* obs = nullptr) {
  // `live`: tail lanes shadow the last trajectory (identical loads) but must not store -- Tout may alias Tin.
  // The sweeps come in two flavours so that the iterations in between carry no dead weight: the descent iterations roll out the
  // states only (no cost sums) and consume the gradient in place; cost sums and gradient stores exist only in the evaluation
  // passes (the optional one at T_in and the last one).
  const int Nn = EXACT ? N : q.N;
  R t[N], es[N], vs[N];
#pragma unroll
  for (int k = 0; k < N; ++k) {
    if (EXACT || k < Nn) t[k] = lane_ld<LDAUX>(lane_buf(Tin), voff, (unsigned)(3 * k + a) * rowb);
  }
  const AxisConsts<R> c = axis_consts<R>(q, a, q.has_goal ? lane_ld(lane_buf(goal), voff, (unsigned)(a) * rowb) : (R)0);
  const R pinit = lane_ld(lane_buf(p0), voff, (unsigned)(a) * rowb);
  const R vinit = lane_ld(lane_buf(v0), voff, (unsigned)(a) * rowb);
  const R lo = (a == 2) ? q.tz_lo : -q.txy, hi = (a == 2) ? q.tz_hi : q.txy;      // planner.py:390-400
  const int lane_ = (int)(threadIdx.x & (kWave - 1));
  R* my_tile = nullptr;                                       // OBS: this axis' column of the position / obstacle-gradient tile
  if constexpr (OBS) my_tile = obs->tile + (size_t)a * Nn * kWave + lane_;
  // forward sweep with the cost sums (evaluation passes)
  auto forward_cost = [&]() -> R {
    R p = pinit, v = vinit;
    RolloutSums<R> s = {0, 0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < N; ++k) {
      if (EXACT || k < Nn) {
        const R acc = t[k] * q.inv_mass - c.grav;
        const R dev = t[k] - c.hov;
        const R e = p - c.gl;
        es[k] = e; vs[k] = v;
        if constexpr (OBS) my_tile[(size_t)k * kWave] = p;
        if (k == Nn - 1) s.sterm = e * e; else s.sp += e * e;
        s.sv += v * v; s.sa += acc * acc; s.st += dev * dev;
        p = p + v * q.dt + q.half_dt2 * acc;
        v = v + acc * q.dt;
      }
    }
    s.sp += s.sterm;
    return axis_cost(q, s);
  };
  cost_first = (R)0;
  bool first_exchange = true;
  if (want_first && iters > 0) {
    cost_first = forward_cost();
    if constexpr (OBS) { obstacle_exchange<R, TS>(*obs, Nn, a, lane_, first_exchange); first_exchange = false; }     // the penalty at T_in
  }
  // Descent iterations in their leanest algebraically equal form (11 VALU per step instead of 17): the position error e = P - goal is
  // rolled out directly (the goal is constant, so e obeys P's recurrence), the local part of the gradient is one fma
  //   d/dT_k [wa acc^2 + wT (T - hover)^2] = gA T_k - gB,   gA = 2 wa / m^2 + 2 wT,  gB = 2 wa g / m + 2 wT hover,
  // and the step is folded into the coefficients:  T <- clamp(T (1 - s gA) + s gB - s c_lp lamP - s c_lv lamV).
  // Rounding differs from the evaluation passes' expressions by a few ulp (documented in the parity check); the evaluation passes
  // -- the ones whose cost and gradient leave the kernel -- keep the stand-alone kernel's expressions.
  const R gA = c.c_aa * q.inv_mass + c.c_tt, gB = c.c_aa * c.grav + c.c_tt * c.hov;
  const R u1 = (R)1 - step * gA, u0 = step * gB, uP = -step * c.c_lp, uV = -step * c.c_lv;
  const R lamP_term = c.two_wp * ((R)1 + q.term);
#pragma unroll 1
  for (int it = 0; it < iters; ++it) {
    R e = pinit - c.gl, v = vinit;
#pragma unroll
    for (int k = 0; k < N; ++k) {                              // states only
      if (EXACT || k < Nn) {
        const R acc = fma_r(t[k], q.inv_mass, -c.grav);
        es[k] = e; vs[k] = v;
        if constexpr (OBS) my_tile[(size_t)k * kWave] = e + c.gl;
        e = fma_r(q.half_dt2, acc, fma_r(v, q.dt, e));
        v = fma_r(acc, q.dt, v);
      }
    }
    if constexpr (OBS) { obstacle_exchange<R, TS>(*obs, Nn, a, lane_, first_exchange); first_exchange = false; }
    R lamP = (R)0, lamV = (R)0;
#pragma unroll
    for (int k = N - 1; k >= 0; --k) {                          // adjoint sweep; T_k is overwritten as soon as its gradient exists
      if (EXACT || k < Nn) {
        R qk = (R)0;                                            // dpenalty/dP_k of this axis (OBS)
        if constexpr (OBS) qk = my_tile[(size_t)k * kWave];
        if (k == Nn - 1) {
          t[k] = clamp_r(fma_r(t[k], u1, u0), lo, hi);
          if constexpr (OBS) lamP = fma_r(lamP_term, es[k], qk); else lamP = lamP_term * es[k];
          lamV = c.two_wv * vs[k];
        } else {
          t[k] = clamp_r(fma_r(t[k], u1, fma_r(lamP, uP, fma_r(lamV, uV, u0))), lo, hi);
          lamV = fma_r(c.two_wv, vs[k], fma_r(q.dt, lamP, lamV));
          if constexpr (OBS) lamP = fma_r(c.two_wp, es[k], lamP + qk); else lamP = fma_r(c.two_wp, es[k], lamP);
        }
      }
    }
  }
  // the last evaluation: cost and gradient at the final T (the gradient parks in the state registers it has just consumed)
  const R cost = forward_cost();
  if (!(want_first && iters > 0)) cost_first = cost;
  if constexpr (OBS) obstacle_exchange<R, TS>(*obs, Nn, a, lane_, first_exchange);
  if (gradT != nullptr) {
    R lamP = (R)0, lamV = (R)0;
#pragma unroll
    for (int k = N - 1; k >= 0; --k) {
      if (EXACT || k < Nn) {
        const R acc = t[k] * q.inv_mass - c.grav;
        const R dev = t[k] - c.hov;
        R qk = (R)0;
        if constexpr (OBS) qk = my_tile[(size_t)k * kWave];
        R g;
        if (k == Nn - 1) {
          g = c.c_aa * acc + c.c_tt * dev;
          lamP = c.two_wp * ((R)1 + q.term) * es[k];
          if constexpr (OBS) lamP += qk;
          lamV = c.two_wv * vs[k];
        } else {
          g = c.c_aa * acc + c.c_tt * dev + c.c_lp * lamP + c.c_lv * lamV;
          lamV = c.two_wv * vs[k] + q.dt * lamP + lamV;
          if constexpr (OBS) lamP = c.two_wp * es[k] + (lamP + qk); else lamP = c.two_wp * es[k] + lamP;
        }
        es[k] = g;
      }
    }
  }
  if (live) {
    if (gradT != nullptr) {
#pragma unroll
      for (int k = 0; k < N; ++k) {
        if (EXACT || k < Nn) lane_st<STAUX>(lane_buf(gradT), voff, (unsigned)(3 * k + a) * rowb, es[k]);
      }
    }
#pragma unroll
    for (int k = 0; k < N; ++k) {
      if (EXACT || k < Nn) lane_st<STAUX>(lane_buf(Tout), voff, (unsigned)(3 * k + a) * rowb, t[k]);
    }
  }
  return cost;
}

// Any horizon: the working copy of T lives in Tout (the lane's own elements, L1/L2-resident between iterations); states are
// recovered by walking the recurrence backwards as in rollout_axis_rev.
template <typename R, bool OBS = false, int TS = kWave>
__device__ __forceinline__ R iterate_axis_mem(const DevParams<R>& q, int a, unsigned voff, unsigned rowb, const R* __restrict__ p0,
                                              const R* __restrict__ v0, const R* __restrict__ goal, const R* __restrict__ Tin,
                                              R* __restrict__ Tout, R* __restrict__ gradT, int iters, R step, bool live, bool want_first,
                                              R& cost_first, const ObsCtx<R>* obs = nullptr) {
  (void)want_first;
  const int N = q.N;
  const int lane_ = (int)(threadIdx.x & (kWave - 1));
  // the working copy lives in Tout, so a tail lane has nothing of its own to iterate on: it leaves (no cross-lane op below).  Not so in
  // the obstacle-aware form, whose passes meet at workgroup barriers: a barrier is an instruction of the WAVEFRONT, so tail lanes
  // must walk the same code as their wavefront's live lanes (a second copy of the loop in a divergent branch would make the wavefront
  // execute every barrier twice); there they compute on zeros and neither load nor store.
  if constexpr (!OBS) {
    if (!live) { cost_first = (R)0; return (R)0; }
  }
  R* my_tile = nullptr;
  if constexpr (OBS) my_tile = obs->tile + (size_t)a * N * kWave + lane_;
  const AxisConsts<R> c = axis_consts<R>(q, a, q.has_goal ? lane_ld(lane_buf(goal), voff, (unsigned)(a) * rowb) : (R)0);
  const R pinit = lane_ld(lane_buf(p0), voff, (unsigned)(a) * rowb);
  const R vinit = lane_ld(lane_buf(v0), voff, (unsigned)(a) * rowb);
  const R lo = (a == 2) ? q.tz_lo : -q.txy, hi = (a == 2) ? q.tz_hi : q.txy;
  if (Tin != Tout && live) {
    for (int k = 0; k < N; ++k) lane_st(lane_buf(Tout), voff, (unsigned)(3 * k + a) * rowb, lane_ld(lane_buf(Tin), voff, (unsigned)(3 * k + a) * rowb));
  }
  R cost = (R)0;
#pragma unroll 1
  for (int it = 0; it <= iters; ++it) {
    const bool last = it == iters;
    R p = pinit, v = vinit, pl = pinit, vl = vinit, tk = (R)0;
    RolloutSums<R> s = {0, 0, 0, 0, 0};
#pragma unroll 6
    for (int k = 0; k < N; ++k) {
      tk = (!OBS || live) ? lane_ld(lane_buf(Tout), voff, (unsigned)(3 * k + a) * rowb) : (R)0;
      const R acc = tk * q.inv_mass - c.grav;
      const R dev = tk - c.hov;
      const R e = p - c.gl;
      if (k == N - 1) s.sterm = e * e; else s.sp += e * e;
      s.sv += v * v; s.sa += acc * acc; s.st += dev * dev;
      if constexpr (OBS) my_tile[(size_t)k * kWave] = p;
      pl = p; vl = v;
      p = p + v * q.dt + q.half_dt2 * acc;
      v = v + acc * q.dt;
    }
    s.sp += s.sterm;
    cost = axis_cost(q, s);
    if (it == 0) cost_first = cost;
    if constexpr (OBS) obstacle_exchange<R, TS>(*obs, N, a, lane_, it == 0);
    R lamP = c.two_wp * ((R)1 + q.term) * (pl - c.gl);
    if constexpr (OBS) lamP += my_tile[(size_t)(N - 1) * kWave];
    R lamV = c.two_wv * vl;
    {
      const R g = c.c_aa * (tk * q.inv_mass - c.grav) + c.c_tt * (tk - c.hov);
      if (!OBS || live) {
        if (last) { if (gradT != nullptr) lane_st(lane_buf(gradT), voff, (unsigned)(3 * (N - 1) + a) * rowb, g); }
        else lane_st(lane_buf(Tout), voff, (unsigned)(3 * (N - 1) + a) * rowb, projected_update(tk, g, step, lo, hi));
      }
    }
    R pk = pl, vk = vl;
#pragma unroll 6
    for (int k = N - 2; k >= 0; --k) {
      const R tt = (!OBS || live) ? lane_ld(lane_buf(Tout), voff, (unsigned)(3 * k + a) * rowb) : (R)0;
      const R acc = tt * q.inv_mass - c.grav;
      const R dev = tt - c.hov;
      vk = vk - acc * q.dt;
      pk = pk - vk * q.dt - q.half_dt2 * acc;
      const R g = c.c_aa * acc + c.c_tt * dev + c.c_lp * lamP + c.c_lv * lamV;
      if (!OBS || live) {
        if (last) { if (gradT != nullptr) lane_st(lane_buf(gradT), voff, (unsigned)(3 * k + a) * rowb, g); }
        else lane_st(lane_buf(Tout), voff, (unsigned)(3 * k + a) * rowb, projected_update(tt, g, step, lo, hi));
      }
      lamV = c.two_wv * vk + q.dt * lamP + lamV;
      if constexpr (OBS) lamP = c.two_wp * (pk - c.gl) + (lamP + my_tile[(size_t)k * kWave]); else lamP = c.two_wp * (pk - c.gl) + lamP;
    }
  }
  return cost;
}

// FLAGS as rollout_kernel (bit 0 nt loads, bit 1 nt stores, bit 2 XCD-contiguous block order, bit 3 N is a register bucket).
// blockIdx.y = batch of a multi-batch launch.
template <typename R, int N, bool REG, int FLAGS>
__global__ void __launch_bounds__(192)
rollout_iterate_kernel(DevParams<R> q, int B, int ld, int iters, R step, const R* __restrict__ p0, const R* __restrict__ v0,
                       const R* __restrict__ goal, const R* __restrict__ Tin, R* __restrict__ Tout, R* __restrict__ cost_first,
                       R* __restrict__ cost, R* __restrict__ gradT, unsigned long long* __restrict__ key, uint32_t index_base) {
  {
    const size_t bi = blockIdx.y, ss = (size_t)3 * ld, st = (size_t)3 * q.N * ld;
    p0 += bi * ss; v0 += bi * ss; Tin += bi * st; Tout += bi * st; cost += bi * (size_t)ld;
    if (goal != nullptr) goal += bi * ss;
    if (gradT != nullptr) gradT += bi * st;
    if (cost_first != nullptr) cost_first += bi * (size_t)ld;
    if (key != nullptr) key += bi * (size_t)gridDim.x;
  }
  int blk = blockIdx.x;
  if ((FLAGS & 4) && (gridDim.x & 7) == 0) blk = (blk & 7) * (gridDim.x >> 3) + (blk >> 3);
  const int lane = threadIdx.x & (kWave - 1);
  const int b0 = blk * kWave + lane;
  const bool live = b0 < B;
  const int b = live ? b0 : B - 1;
  const unsigned voff = (unsigned)b * (unsigned)sizeof(R), rowb = (unsigned)ld * (unsigned)sizeof(R);
  __shared__ R part[2][3][kWave];
  const int a = wave_uniform((int)(threadIdx.x / kWave));
  R c0 = (R)0, c;
  if constexpr (REG) c = iterate_axis_reg<R, N, !(FLAGS & 8), (FLAGS & 1) ? 2 : 0, (FLAGS & 2) ? 2 : 0>(q, a, voff, rowb, p0, v0, goal, Tin, Tout, gradT, iters, step, live, cost_first != nullptr, c0);
  else c = iterate_axis_mem<R>(q, a, voff, rowb, p0, v0, goal, Tin, Tout, gradT, iters, step, live, cost_first != nullptr, c0);
  part[0][a][lane] = c; part[1][a][lane] = c0;
  __syncthreads();
  const R total = part[0][0][lane] + part[0][1][lane] + part[0][2][lane];
  if (a == 0 && live && cost_first != nullptr) cost_first[b] = part[1][0][lane] + part[1][1][lane] + part[1][2][lane];
  rollout_epilogue<R>(live && a == 0, b, total, cost, (a == 0 && key != nullptr) ? key + blk : nullptr, index_base);
}

#ifndef SE3MPC_OBS_WIDE_W
#define SE3MPC_OBS_WIDE_W 7
#endif
#ifndef SE3MPC_OBS_WIDE_TS
#define SE3MPC_OBS_WIDE_TS 32
#endif
constexpr int kObsWideW = SE3MPC_OBS_WIDE_W, kObsWideTS = SE3MPC_OBS_WIDE_TS;
// The obstacle-aware form of rollout_iterate_kernel (see ObsCtx above).  Two workgroup shapes:
//   <W = 3, TS = 64>: the three axis wavefronts of 64 trajectories, each sweeping a third of the steps against the LDS-resident sphere
//     table -- for launches with enough workgroups to keep every SIMD busy with several wavefronts (which hide the LDS latency);
//   <W = 7, TS = 32>: for launches that would leave compute units idle (8192 trajectories = 128 workgroups of 64 on 256 CUs).  A workgroup
//     takes 32 trajectories (twice the workgroups), its axis wavefronts only roll out / run the adjoint, and FOUR helper wavefronts -- one
//     per SIMD of the CU: a fifth would share a SIMD and become the critical path, measured -- take all the distance evaluations with the
//     sphere table in their registers; the two halves of a helper take different steps of the same 32 trajectories.
// cost = running cost + penalty at T_out; penalty: NULL or [B] = the penalty alone (0 = the plan keeps the margin of every sphere).
// key: one slot per 64 trajectories (the ABI's ceil(B/64)); with TS = 32 the two workgroups of a slot fold into it with atomicMin (the
// launcher presets the slots to the dead-lane sentinel).
template <typename R, int N, bool REG, int FLAGS, int W, int TS>
__global__ void __launch_bounds__(64 * W)
rollout_iterate_obstacles_kernel(DevParams<R> q, int B, int ld, int iters, R step, const R* __restrict__ p0, const R* __restrict__ v0,
                                 const R* __restrict__ goal, const R* __restrict__ Tin, R* __restrict__ Tout, R* __restrict__ cost_first,
                                 R* __restrict__ cost, R* __restrict__ gradT, const R* __restrict__ spheres, int K, R w_obs,
                                 R* __restrict__ penalty, unsigned long long* __restrict__ key, uint32_t index_base) {
  HIP_DYNAMIC_SHARED(unsigned char, lds_raw)
  constexpr int SUBS = kWave / TS;                            // halves of a wavefront that share a trajectory set
  {
    const size_t bi = blockIdx.y, ss = (size_t)3 * ld, st = (size_t)3 * q.N * ld;
    p0 += bi * ss; v0 += bi * ss; Tin += bi * st; Tout += bi * st; cost += bi * (size_t)ld;
    if (goal != nullptr) goal += bi * ss;
    if (gradT != nullptr) gradT += bi * st;
    if (cost_first != nullptr) cost_first += bi * (size_t)ld;
    if (penalty != nullptr) penalty += bi * (size_t)ld;
    if (key != nullptr) key += bi * (size_t)((B + kWave - 1) / kWave);
  }
  const int Kpad = (K + 7) / 8 * 8;
  R* tile = reinterpret_cast<R*>(lds_raw);                  // [3][N][64]: positions, then dpenalty/dP, of the pass in flight (TS = 32: the
                                                             // shadow half of an axis wavefront keeps columns 32..63 to itself; nobody reads them)
  R* sph = tile + (size_t)3 * q.N * kWave;                   // [Kpad][4]
  R* pcost = sph + (size_t)4 * Kpad;                         // [3][64] axis costs at T_out, [3][64] at T_in
  R* ppen = pcost + 6 * kWave;                               // [W][64] penalty shares at T_out, [W][64] at T_in
  for (int i = threadIdx.x; i < Kpad; i += 64 * W) {         // visible to every wavefront behind the first barrier
    if (i < K) {
      const R sm = spheres[4 * i + 3] + q.margin;
      sph[4 * i + 0] = spheres[4 * i + 0]; sph[4 * i + 1] = spheres[4 * i + 1]; sph[4 * i + 2] = spheres[4 * i + 2]; sph[4 * i + 3] = sm * sm;
    } else {
      sph[4 * i + 0] = (R)0; sph[4 * i + 1] = (R)0; sph[4 * i + 2] = (R)0; sph[4 * i + 3] = (R)-INFINITY;
    }
  }
  int blk = blockIdx.x;
  if ((FLAGS & 4) && (gridDim.x & 7) == 0) blk = (blk & 7) * (gridDim.x >> 3) + (blk >> 3);
  const int lane = threadIdx.x & (kWave - 1);
  const int tl = lane & (TS - 1), sub = lane / TS;
  const int b0 = blk * TS + tl;
  const bool live = b0 < B && sub == 0;                       // the second half of a TS = 32 axis wavefront shadows the first: same loads, no stores,
                                                             // and nothing it computes is used (its tile columns never receive an obstacle gradient)
  const int b = b0 < B ? b0 : B - 1;
  const unsigned voff = (unsigned)b * (unsigned)sizeof(R), rowb = (unsigned)ld * (unsigned)sizeof(R);
  const int a = wave_uniform((int)(threadIdx.x / kWave));
  ObsCtx<R> o;
  o.tile = tile; o.sph = sph; o.pen = ppen; o.pen_first = ppen + W * kWave; o.Kpad = Kpad; o.w_obs = w_obs;
  // (no table, or one too long for the helpers' registers: everyone sweeps from LDS)
  o.axis_sweeps = W <= 3 || Kpad == 0 || Kpad / 8 > (sizeof(R) == 4 ? 4 : 2);
  if (o.axis_sweeps) { o.slot = a * SUBS + sub; o.slots = W * SUBS; }
  else { o.slot = (a - 3) * SUBS + sub; o.slots = (W - 3) * SUBS; }       // (axis wavefronts never read theirs)
  if constexpr (W > 3) __syncthreads();                       // the helpers read the table into registers before the first exchange
  if (a < 3) {
    R c0 = (R)0, c;
    if constexpr (REG) c = iterate_axis_reg<R, N, !(FLAGS & 8), (FLAGS & 1) ? 2 : 0, (FLAGS & 2) ? 2 : 0, true, TS>(q, a, voff, rowb, p0, v0, goal, Tin, Tout, gradT, iters, step, live, cost_first != nullptr, c0, &o);
    else c = iterate_axis_mem<R, true, TS>(q, a, voff, rowb, p0, v0, goal, Tin, Tout, gradT, iters, step, live, cost_first != nullptr, c0, &o);
    pcost[a * kWave + lane] = c; pcost[(3 + a) * kWave + lane] = c0;
  } else {
    // as many exchanges as the axis wavefronts run: one per descent iteration, the last evaluation, and (register form) the
    // evaluation at T_in when its cost is asked for
    const int passes = iters + 1 + ((REG && cost_first != nullptr && iters > 0) ? 1 : 0);
    const int kp = Kpad / 8;
    if (o.axis_sweeps) {
      for (int ps = 0; ps < passes; ++ps) obstacle_exchange<R, TS>(o, q.N, a, lane, ps == 0);
    } else if (kp == 1) helper_passes_regs<R, 1, TS>(o, q.N, a, lane, passes);
    else if (kp == 2) helper_passes_regs<R, 2, TS>(o, q.N, a, lane, passes);
    else if constexpr (sizeof(R) == 4) {
      if (kp == 3) helper_passes_regs<R, 3, TS>(o, q.N, a, lane, passes);
      else helper_passes_regs<R, 4, TS>(o, q.N, a, lane, passes);
    }
  }
  __syncthreads();
  R total = pcost[0 * kWave + lane] + pcost[1 * kWave + lane] + pcost[2 * kWave + lane];
  R pen = (R)0, pen0 = (R)0;
#pragma unroll
  for (int w = 0; w < W; ++w) {
#pragma unroll
    for (int h = 0; h < SUBS; ++h) { pen += ppen[w * kWave + h * TS + tl]; pen0 += ppen[(W + w) * kWave + h * TS + tl]; }
  }
  total += pen;
  if (a == 0 && live) {
    if (cost_first != nullptr) cost_first[b] = pcost[3 * kWave + lane] + pcost[4 * kWave + lane] + pcost[5 * kWave + lane] + pen0;
    if (penalty != nullptr) penalty[b] = pen;
  }
  if constexpr (SUBS == 1) {
    rollout_epilogue<R>(live && a == 0, b, total, cost, (a == 0 && key != nullptr) ? key + blk : nullptr, index_base);
  } else {
    rollout_epilogue<R, true>(live && a == 0, b, total, cost, (a == 0 && key != nullptr) ? key + blk / SUBS : nullptr, index_base);
  }
}

// One projected gradient step as its own launch: T_out = clip(T - step * g, thrust box).  The host-chained counterpart of one
// iteration of rollout_iterate_kernel (rollout_cost_grad launch + this launch).
template <typename R>
__global__ void __launch_bounds__(64)
projected_step_kernel(DevParams<R> q, int B, int ld, R step, const R* __restrict__ T, const R* __restrict__ g, R* __restrict__ Tout) {
  const LaneIdx li = lane_index<R>(B);
  if (!li.live) return;
  const unsigned voff = li.voff, rowb = (unsigned)ld * (unsigned)sizeof(R);
  const int rows = 3 * q.N;
#pragma unroll 6
  for (int r = 0; r < rows; ++r) {
    const int a = r % 3;
    const R lo = (a == 2) ? q.tz_lo : -q.txy, hi = (a == 2) ? q.tz_hi : q.txy;
    const R t = lane_ld<2>(lane_buf(T), voff, (unsigned)r * rowb), gr = lane_ld<2>(lane_buf(g), voff, (unsigned)r * rowb);
    lane_st<2>(lane_buf(Tout), voff, (unsigned)r * rowb, projected_update(t, gr, step, lo, hi));
  }
}

template <typename R>
int rollout_iterate_impl(const se3mpc_params* p, int B, int ld, int nbatch, int iters, double step, const R* p0, const R* v0, const R* goal,
                         const R* Tin, R* Tout, R* cost_first, R* cost, R* gradT, uint64_t* key64, uint32_t index_base, void* stream) {
  if (nbatch < 1 || nbatch > 65535 || iters < 0 || iters > 1000000) return SE3MPC_ERR_SHAPE;
  int rc = check_lane_args(p, B, ld, p ? 3LL * p->horizon : 0, sizeof(R));
  if (rc) return rc;
  if (!std::isfinite(step)) return SE3MPC_ERR_PARAM;
  if (B == 0) return SE3MPC_OK;
  if (!p0 || !v0 || !Tin || !Tout || !cost || (p->has_goal && !goal)) return SE3MPC_ERR_NULL;
  unsigned long long* key = reinterpret_cast<unsigned long long*>(key64);
  const DevParams<R> q = make_dev_params<R>(*p);
  const int N = p->horizon, nblk = grid_for(B, kWave);
  hipStream_t s = (hipStream_t)stream;
  dispatch_horizon<R, true>(N, kSweepAuto, [&](auto sweep) {
    using S = decltype(sweep);
    hipLaunchKernelGGL((rollout_iterate_kernel<R, S::NN, S::REG, S::FLAGS>), dim3(nblk, nbatch), dim3(192), 0, s, q, B, ld, iters, (R)step, p0, v0,
                       goal, Tin, Tout, cost_first, cost, gradT, key, index_base);
  });
  return launch_status("se3mpc_rollout_iterate");
}

template <typename R>
int rollout_iterate_obstacles_impl(const se3mpc_params* p, int B, int ld, int nbatch, int iters, double step, const R* p0, const R* v0,
                                   const R* goal, const R* Tin, R* Tout, R* cost_first, R* cost, R* gradT, const R* spheres, int K,
                                   double obstacle_weight, R* penalty, uint64_t* key64, uint32_t index_base, void* stream) {
  if (nbatch < 1 || nbatch > 65535 || iters < 0 || iters > 1000000 || K < 0 || K > SE3MPC_MAX_SPHERES) return SE3MPC_ERR_SHAPE;
  int rc = check_lane_args(p, B, ld, p ? 3LL * p->horizon : 0, sizeof(R));
  if (rc) return rc;
  if (!std::isfinite(step) || !std::isfinite(obstacle_weight) || obstacle_weight < 0.0) return SE3MPC_ERR_PARAM;
  if (B == 0) return SE3MPC_OK;
  if (!p0 || !v0 || !Tin || !Tout || !cost || (p->has_goal && !goal) || (K > 0 && !spheres)) return SE3MPC_ERR_NULL;
  unsigned long long* key = reinterpret_cast<unsigned long long*>(key64);
  const DevParams<R> q = make_dev_params<R>(*p);
  const int N = p->horizon, nblk = grid_for(B, kWave);
  hipStream_t s = (hipStream_t)stream;
  // the wide shape (7 wavefronts on 32 trajectories) at every size: measured 2.2x the narrow one (3 wavefronts on 64, LDS-resident sphere
  // table) from 8192 to 262144 trajectories (profiles/r03_cfg3_loop_shapes.txt); se3mpc_set_rollout_variant(+128) forces the narrow one
  const int forced_w = (g_lane_tuning.rollout_variant >> 7) & 3;
  const bool wide = forced_w != 1;
  const int Kpad = (K + 7) / 8 * 8;
  if (wide && key != nullptr && kObsWideTS < kWave) {
    // two workgroups fold into each key slot with atomicMin: start from the dead-lane sentinel
    if (hipMemsetAsync(key, 0xFF, (size_t)nbatch * nblk * sizeof(unsigned long long), s) != hipSuccess) return SE3MPC_ERR_LAUNCH;
  }
  dispatch_horizon<R, true>(N, kSweepAuto, [&](auto sweep) {
    using S = decltype(sweep);
    auto launch = [&](auto w, auto ts) {
      constexpr int WW = decltype(w)::value, TT = decltype(ts)::value;
      const size_t lds = ((size_t)3 * N * kWave + (size_t)4 * Kpad + (size_t)(6 + 2 * WW) * kWave) * sizeof(R);
      if (lds > 64 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&rollout_iterate_obstacles_kernel<R, S::NN, S::REG, S::FLAGS, WW, TT>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      hipLaunchKernelGGL((rollout_iterate_obstacles_kernel<R, S::NN, S::REG, S::FLAGS, WW, TT>), dim3(grid_for(B, TT), nbatch), dim3(64 * WW),
                         lds, s, q, B, ld, iters, (R)step, p0, v0, goal, Tin, Tout, cost_first, cost, gradT, spheres, K,
                         (R)obstacle_weight, penalty, key, index_base);
    };
    if (wide) launch(std::integral_constant<int, kObsWideW>{}, std::integral_constant<int, kObsWideTS>{});
    else launch(std::integral_constant<int, 3>{}, std::integral_constant<int, kWave>{});
  });
  return launch_status("se3mpc_rollout_iterate_obstacles");
}

template <typename R>
int projected_step_impl(const se3mpc_params* p, int B, int ld, double step, const R* T, const R* g, R* Tout, void* stream) {
  int rc = check_lane_args(p, B, ld, p ? 3LL * p->horizon : 0, sizeof(R));
  if (rc) return rc;
  if (!std::isfinite(step)) return SE3MPC_ERR_PARAM;
  if (B == 0) return SE3MPC_OK;
  if (!T || !g || !Tout) return SE3MPC_ERR_NULL;
  hipLaunchKernelGGL(projected_step_kernel<R>, dim3(grid_for(B, kLaneBlock)), dim3(kLaneBlock), 0, (hipStream_t)stream, make_dev_params<R>(*p), B,
                     ld, (R)step, T, g, Tout);
  return launch_status("se3mpc_projected_step");
}

}  // namespace se3mpc

using namespace se3mpc;   // C ABI (include/se3mpc.h)

extern "C" int se3mpc_rollout_iterate_f32(const se3mpc_params* p, int B, int ld, int nbatch, int iters, double step, const float* p0, const float* v0,
                                          const float* goal, const float* T_in, float* T_out, float* cost_first, float* cost, float* gradT,
                                          uint64_t* wave_keys, uint32_t index_base, void* stream) {
  return rollout_iterate_impl<float>(p, B, ld, nbatch, iters, step, p0, v0, goal, T_in, T_out, cost_first, cost, gradT, wave_keys, index_base,
                                     stream);
}
extern "C" int se3mpc_rollout_iterate_f64(const se3mpc_params* p, int B, int ld, int nbatch, int iters, double step, const double* p0,
                                          const double* v0, const double* goal, const double* T_in, double* T_out, double* cost_first, double* cost,
                                          double* gradT, uint64_t* wave_keys, uint32_t index_base, void* stream) {
  return rollout_iterate_impl<double>(p, B, ld, nbatch, iters, step, p0, v0, goal, T_in, T_out, cost_first, cost, gradT, wave_keys, index_base,
                                      stream);
}
extern "C" int se3mpc_rollout_iterate_obstacles_f32(const se3mpc_params* p, int B, int ld, int nbatch, int iters, double step, const float* p0,
                                                    const float* v0, const float* goal, const float* T_in, float* T_out, float* cost_first,
                                                    float* cost, float* gradT, const float* spheres, int K, double obstacle_weight, float* penalty,
                                                    uint64_t* wave_keys, uint32_t index_base, void* stream) {
  return rollout_iterate_obstacles_impl<float>(p, B, ld, nbatch, iters, step, p0, v0, goal, T_in, T_out, cost_first, cost, gradT, spheres, K,
                                               obstacle_weight, penalty, wave_keys, index_base, stream);
}
extern "C" int se3mpc_rollout_iterate_obstacles_f64(const se3mpc_params* p, int B, int ld, int nbatch, int iters, double step, const double* p0,
                                                    const double* v0, const double* goal, const double* T_in, double* T_out, double* cost_first,
                                                    double* cost, double* gradT, const double* spheres, int K, double obstacle_weight,
                                                    double* penalty, uint64_t* wave_keys, uint32_t index_base, void* stream) {
  return rollout_iterate_obstacles_impl<double>(p, B, ld, nbatch, iters, step, p0, v0, goal, T_in, T_out, cost_first, cost, gradT, spheres, K,
                                                obstacle_weight, penalty, wave_keys, index_base, stream);
}
extern "C" int se3mpc_projected_step_f32(const se3mpc_params* p, int B, int ld, double step, const float* T, const float* gradT, float* T_out,
                                         void* stream) {
  return projected_step_impl<float>(p, B, ld, step, T, gradT, T_out, stream);
}
extern "C" int se3mpc_projected_step_f64(const se3mpc_params* p, int B, int ld, double step, const double* T, const double* gradT, double* T_out,
                                         void* stream) {
  return projected_step_impl<double>(p, B, ld, step, T, gradT, T_out, stream);
}
