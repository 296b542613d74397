// rollout.hip -- the shooting form in one launch: forward rollout, objective and exact gradient of a batch of thrust sequences
// (se3mpc_rollout_cost_grad_*), the flagship workload of bench.py.  The sweeps are in rollout_device.hpp; which horizon takes
// which is dispatch_horizon's table (lane_common.hpp).
#include "lane_common.hpp"
#include "rollout_device.hpp"

namespace se3mpc {

// Kernel shells.  SPLIT: a 192-thread workgroup owns 64 trajectories, wavefront w = axis w; the
// three partial costs meet in LDS ([3][64] values), then every wavefront runs the (uniform)
// epilogue and wavefront 0 commits it.  !SPLIT: one wavefront per 64 trajectories loops the axes.
// blockIdx.y = batch index of a multi-batch launch: consecutive batches are consecutive [rows][ld]
// blocks of every operand (keys: one word per batch).  FLAGS: bit 0 nt loads of T, bit 1 nt stores of
// the gradient, bit 2 XCD-contiguous block order (blocks that share an XCD stream adjacent columns), bit 3
// N is a register bucket (horizon q.N <= N, guarded steps) instead of the exact horizon.
template <typename R, int N, bool REG, bool SPLIT, bool GRAD, bool STATES, int FLAGS = 7>
__global__ void __launch_bounds__(SPLIT ? 192 : 64)
rollout_kernel(DevParams<R> q, int B, int ld, const R* __restrict__ p0, const R* __restrict__ v0,
               const R* __restrict__ goal, const R* __restrict__ T, R* __restrict__ cost, R* __restrict__ gradT,
               R* __restrict__ Pout, R* __restrict__ Vout, unsigned long long* __restrict__ key, uint32_t index_base) {
  {
    const size_t bi = blockIdx.y, ss = (size_t)3 * ld, st = (size_t)3 * q.N * ld;
    p0 += bi * ss; v0 += bi * ss; T += bi * st; cost += bi * (size_t)ld;
    if (goal != nullptr) goal += bi * ss;
    if (GRAD) gradT += bi * st;
    if (STATES) { Pout += bi * st; Vout += bi * st; }
    if (key != nullptr) key += bi * (size_t)gridDim.x;      // wave-key slots: [batch][block]
  }
  int blk = blockIdx.x;
  if ((FLAGS & 4) && (gridDim.x & 7) == 0) blk = (blk & 7) * (gridDim.x >> 3) + (blk >> 3);
  const int lane = threadIdx.x & (kWave - 1);
  const int b0 = blk * kWave + lane;
  const bool live = b0 < B;
  const int b = live ? b0 : B - 1;          // tail lanes shadow the last trajectory: identical loads, identical
                                            // (benign duplicate) stores, no contribution to cost/key
  const unsigned voff = (unsigned)b * (unsigned)sizeof(R);    // the lane's byte offset inside a row
  const unsigned rowb = (unsigned)ld * (unsigned)sizeof(R);   // bytes per row (wave-uniform)
  R total;
  if constexpr (SPLIT) {
    __shared__ R part[3][kWave];
    const int a = wave_uniform((int)(threadIdx.x / kWave));   // wave index -> SGPR, so row bases stay scalar
    R c;
    if constexpr (REG) c = rollout_axis_reg<R, N, GRAD, STATES, (FLAGS & 1) ? 2 : 0, (FLAGS & 2) ? 2 : 0, false, !(FLAGS & 8)>(q, a, voff, rowb, p0, v0, goal, T, gradT, Pout, Vout);
    else c = rollout_axis_rev<R, GRAD, STATES, (FLAGS & 2) ? 2 : 0>(q, a, voff, rowb, p0, v0, goal, T, gradT, Pout, Vout);
    part[a][lane] = c;
    __syncthreads();
    total = part[0][lane] + part[1][lane] + part[2][lane];
    rollout_epilogue<R>(live && a == 0, b, total, cost, (a == 0 && key != nullptr) ? key + blk : nullptr, index_base);
  } else {
    total = (R)0;
#pragma unroll 1
    for (int a = 0; a < 3; ++a) {
      if constexpr (REG) total += rollout_axis_reg<R, N, GRAD, STATES, (FLAGS & 1) ? 2 : 0, (FLAGS & 2) ? 2 : 0, false, !(FLAGS & 8)>(q, a, voff, rowb, p0, v0, goal, T, gradT, Pout, Vout);
      else total += rollout_axis_rev<R, GRAD, STATES, (FLAGS & 2) ? 2 : 0>(q, a, voff, rowb, p0, v0, goal, T, gradT, Pout, Vout);
    }
    rollout_epilogue<R>(live, b, total, cost, key != nullptr ? key + blk : nullptr, index_base);
  }
}

template <typename R, bool GRAD, bool STATES>
__global__ void __launch_bounds__(64)
rollout_lds_kernel(DevParams<R> q, int B, int ld, const R* __restrict__ p0, const R* __restrict__ v0,
                   const R* __restrict__ goal, const R* __restrict__ T, R* __restrict__ cost,
                   R* __restrict__ gradT, R* __restrict__ Pout, R* __restrict__ Vout,
                   unsigned long long* __restrict__ key, uint32_t index_base) {
  HIP_DYNAMIC_SHARED(unsigned char, lds_raw)
  R* tile = reinterpret_cast<R*>(lds_raw);                 // [2N][64]: P_k at row 2k, V_k at row 2k+1
  const int lane = threadIdx.x;                            // no barrier below: a wave only reads its own column
  const int b0 = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = b0 < B;
  const int b = live ? b0 : B - 1;
  const int N = q.N;
  RolloutSums<R> s = {0, 0, 0, 0, 0};
  const R two_wp = q.has_goal ? (R)2 * q.wp : (R)0;
  const size_t stride = (size_t)3 * ld;
#pragma unroll 1
  for (int a = 0; a < 3; ++a) {
    const R gl = q.has_goal ? goal[(size_t)a * ld + b] : (R)0;
    const R grav = (a == 2) ? q.grav : (R)0;
    const R hov = (a == 2) ? q.hover : (R)0;
    R p = p0[(size_t)a * ld + b];
    R v = v0[(size_t)a * ld + b];
    const R* tp = T + (size_t)a * ld + b;
    R* pp = STATES ? Pout + (size_t)a * ld + b : nullptr;
    R* vp = STATES ? Vout + (size_t)a * ld + b : nullptr;
    R tk = (R)0;
#pragma unroll 4
    for (int k = 0; k < N; ++k) {
      tk = *tp; tp += stride;
      tile[(2 * k) * kWave + lane] = p;
      tile[(2 * k + 1) * kWave + lane] = v;
      if (STATES) { if (live) { *pp = p; *vp = v; } pp += stride; vp += stride; }
      const R acc = tk * q.inv_mass - grav;
      const R e = p - gl;
      const R dev = tk - hov;
      s.sp += e * e; s.sv += v * v; s.sa += acc * acc; s.st += dev * dev;
      if (k == N - 1) s.sterm += e * e;
      p = p + v * q.dt + q.half_dt2 * acc;
      v = v + acc * q.dt;
    }
    if (GRAD) {
      const R pl = tile[(2 * (N - 1)) * kWave + lane], vl = tile[(2 * (N - 1) + 1) * kWave + lane];
      R lamP = two_wp * ((R)1 + q.term) * (pl - gl);
      R lamV = (R)2 * q.wv * vl;
      R* gp = gradT + (size_t)a * ld + b + (size_t)(N - 1) * stride;
      if (live) *gp = (R)2 * q.wa * (tk * q.inv_mass - grav) * q.inv_mass + (R)2 * q.wT * (tk - hov);
      tp -= stride;                                         // tp -> row N-1
#pragma unroll 4
      for (int k = N - 2; k >= 0; --k) {
        gp -= stride; tp -= stride;
        const R t = *tp;
        const R pk = tile[(2 * k) * kWave + lane], vk = tile[(2 * k + 1) * kWave + lane];
        const R acc = t * q.inv_mass - grav;
        if (live) *gp = (R)2 * q.wa * acc * q.inv_mass + (R)2 * q.wT * (t - hov) + (q.half_dt2 * lamP + q.dt * lamV) * q.inv_mass;
        lamV = (R)2 * q.wv * vk + q.dt * lamP + lamV;
        lamP = two_wp * (pk - gl) + lamP;
      }
    }
  }
  rollout_epilogue<R>(live, b, rollout_total(q, s), cost, key != nullptr ? key + blockIdx.x : nullptr, index_base);
}

LaneTuning g_lane_tuning;   // lane_common.hpp; written by se3mpc_set_rollout_variant below

// variant: as LaneTuning::rollout_variant (low 7 bits)
template <typename R, bool GRAD, bool STATES>
int rollout_launch(const se3mpc_params* p, int variant, int B, int ld, const R* p0, const R* v0, const R* goal,
                   const R* T, R* cost, R* gradT, R* P, R* V, unsigned long long* key, uint32_t index_base,
                   int nbatch, hipStream_t s) {
  const DevParams<R> q = make_dev_params<R>(*p);
  const int nblk = grid_for(B, kWave);
  const int flags = variant >> 3;
  variant &= 7;
  const int N = p->horizon;
  auto launch = [&](auto sweep, auto split) {
    using S = decltype(sweep);
    constexpr bool SPLIT = decltype(split)::value;
    hipLaunchKernelGGL((rollout_kernel<R, S::NN, S::REG, SPLIT, GRAD, STATES, S::FLAGS>), dim3(nblk, nbatch), dim3(SPLIT ? 192 : 64), 0,
                       s, q, B, ld, p0, v0, goal, T, cost, gradT, P, V, key, index_base);
  };
  if (variant == 2) {
    const size_t lds = (size_t)2 * N * kWave * sizeof(R);
    if (nbatch != 1) return SE3MPC_ERR_SHAPE;         // the LDS variant is single-batch (measurement only)
    hipLaunchKernelGGL((rollout_lds_kernel<R, GRAD, STATES>), dim3(nblk), dim3(kWave), lds, s, q, B, ld, p0, v0, goal,
                       T, cost, gradT, P, V, key, index_base);
    return launch_status("se3mpc_rollout_cost_grad");
  }
  if constexpr (sizeof(R) == 4 && GRAD && !STATES) {
    if (variant <= 1 && N == 30 && flags != 0) {      // tuning A/B on the benchmarked instantiation: FLAGS = flags - 1
#define SE3MPC_FLAG_CASE(F) case F: launch(Sweep<30, true, F>{}, std::true_type{}); break;
      switch (flags - 1) {
        SE3MPC_FLAG_CASE(0) SE3MPC_FLAG_CASE(1) SE3MPC_FLAG_CASE(2) SE3MPC_FLAG_CASE(3) SE3MPC_FLAG_CASE(4)
        SE3MPC_FLAG_CASE(5) SE3MPC_FLAG_CASE(6)
        default: launch(Sweep<30, true, 7>{}, std::true_type{});
      }
#undef SE3MPC_FLAG_CASE
      return launch_status("se3mpc_rollout_cost_grad");
    }
  }
  // a forced register form (1, 4, 6) falls back to the reversible sweep of the same workgroup shape where the horizon has none
  constexpr SweepRoute kRoute[7] = {kSweepAuto, kSweepExact, kSweepAuto, kSweepRev, kSweepExact, kSweepRev, kSweepBucket};
  if (variant == 4 || variant == 5) dispatch_horizon<R, false>(N, kRoute[variant], [&](auto sweep) { launch(sweep, std::false_type{}); });
  else dispatch_horizon<R, true>(N, kRoute[variant], [&](auto sweep) { launch(sweep, std::true_type{}); });
  return launch_status("se3mpc_rollout_cost_grad");
}

template <typename R>
int rollout_cost_grad_impl(const se3mpc_params* p, int B, int ld, const R* p0, const R* v0, const R* goal, const R* T,
                           R* cost, R* gradT, R* P, R* V, uint64_t* key64, uint32_t index_base, int nbatch,
                           void* stream) {
  unsigned long long* key = reinterpret_cast<unsigned long long*>(key64);
  if (nbatch < 1 || nbatch > 65535) return SE3MPC_ERR_SHAPE;
  int rc = check_lane_args(p, B, ld, p ? 3LL * p->horizon : 0, sizeof(R));   // tallest operand: 3N rows (32-bit buffer offsets)
  if (rc) return rc;
  if (B == 0) return SE3MPC_OK;
  if (!p0 || !v0 || !T || !cost || (p->has_goal && !goal)) return SE3MPC_ERR_NULL;
  if ((P == nullptr) != (V == nullptr)) return SE3MPC_ERR_NULL;   // states come as a pair
  hipStream_t s = (hipStream_t)stream;
  const int var = g_lane_tuning.rollout_variant & 127;
  const bool grad = gradT != nullptr, states = P != nullptr;
  if (grad && states) return rollout_launch<R, true, true>(p, var, B, ld, p0, v0, goal, T, cost, gradT, P, V, key, index_base, nbatch, s);
  if (grad) return rollout_launch<R, true, false>(p, var, B, ld, p0, v0, goal, T, cost, gradT, P, V, key, index_base, nbatch, s);
  if (states) return rollout_launch<R, false, true>(p, var, B, ld, p0, v0, goal, T, cost, gradT, P, V, key, index_base, nbatch, s);
  return rollout_launch<R, false, false>(p, var, B, ld, p0, v0, goal, T, cost, gradT, P, V, key, index_base, nbatch, s);
}

}  // namespace se3mpc

using namespace se3mpc;   // C ABI (include/se3mpc.h)

extern "C" int se3mpc_set_rollout_variant(int variant) {
  if (variant < 0 || variant >= 4096 || ((variant >> 9) & 3) == 3 || (variant & 127) > 71 || (variant & 7) > 6) return SE3MPC_ERR_SHAPE;
  g_lane_tuning.rollout_variant = variant & 511;
  g_lane_tuning.wide_select = (variant >> 9) & 3;
  g_lane_tuning.obs_mfma = (variant >> 11) & 1;
  return SE3MPC_OK;
}

extern "C" int se3mpc_rollout_cost_grad_f32(const se3mpc_params* p, int B, int ld, const float* p0, const float* v0, const float* goal,
                                            const float* T, float* cost, float* gradT, float* P, float* V, uint64_t* key, uint32_t index_base,
                                            void* stream) {
  return rollout_cost_grad_impl<float>(p, B, ld, p0, v0, goal, T, cost, gradT, P, V, key, index_base, 1, stream);
}
extern "C" int se3mpc_rollout_cost_grad_f64(const se3mpc_params* p, int B, int ld, const double* p0, const double* v0, const double* goal,
                                            const double* T, double* cost, double* gradT, double* P, double* V, uint64_t* key, uint32_t index_base,
                                            void* stream) {
  return rollout_cost_grad_impl<double>(p, B, ld, p0, v0, goal, T, cost, gradT, P, V, key, index_base, 1, stream);
}
extern "C" int se3mpc_rollout_cost_grad_batched_f32(const se3mpc_params* p, int B, int ld, int nbatch, const float* p0, const float* v0,
                                                    const float* goal, const float* T, float* cost, float* gradT, uint64_t* keys, uint32_t index_base,
                                                    void* stream) {
  return rollout_cost_grad_impl<float>(p, B, ld, p0, v0, goal, T, cost, gradT, (float*)nullptr, (float*)nullptr, keys, index_base, nbatch, stream);
}
extern "C" int se3mpc_rollout_cost_grad_batched_f64(const se3mpc_params* p, int B, int ld, int nbatch, const double* p0, const double* v0,
                                                    const double* goal, const double* T, double* cost, double* gradT, uint64_t* keys,
                                                    uint32_t index_base, void* stream) {
  return rollout_cost_grad_impl<double>(p, B, ld, p0, v0, goal, T, cost, gradT, (double*)nullptr, (double*)nullptr, keys, index_base, nbatch, stream);
}
