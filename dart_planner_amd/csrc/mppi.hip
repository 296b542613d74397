// mppi.hip -- MPPI (model-predictive path integral) on the shooting form: sample, roll out, weight and update in ONE launch.
//
// One workgroup per problem, all iterations in one launch.  Iteration i (global number g = iter_base + i) of
// problem q = index_base + p:
//   noise    x0..x3 = Philox4x32-10(counter (q, s, g, k), key (seed lo, seed hi)), u_j = (x_j + 1/2) 2^-32 (in the kernel's type),
//            n = (sqrt(-2 ln u0) cos 2 pi u1, sqrt(-2 ln u0) sin 2 pi u1, sqrt(-2 ln u2) cos 2 pi u3)      sample s = 0: no noise
//   sample   T_s[k][a] = clip(U[k][a] + sigma n_a, the thrust box of projected_step_kernel)
//   cost     c_s = the shooting-form cost of se3mpc_rollout_cost_grad_* + obstacle_weight * sum_k sum_j max(0, -c_kj)^2
//   update   m = min_s c_s, w_s = exp(-(c_s - m) / lambda), U <- sum_s w_s T_s / sum_s w_s   (float64, fixed order, no atomics)
// The nominal U lives in LDS, each lane owns one sample per pass (passes loop over chunks of the workgroup's width), and the
// forward sweep keeps the three axes and the noise in registers: no adjoint, no N-length arrays, nothing per sample in HBM.
// The weighted sum needs T_s after the chunk's minimum is known: it is regenerated from the counter (a second Philox + Box-Muller per
// step, no rollout) rather than held in 3N registers -- held, the kernel spills at every horizon where it would pay.
// Chunks fold into the running sums with a streaming rescale exp(-(m_new - m_old) / lambda), so S is not bounded by LDS.
#include "mppi_device.hpp"

namespace se3mpc {
namespace mppi {

// The fused planner: one workgroup of min(S, kBlock) lanes per problem, `iters` iterations, then one evaluation of the nominal.
template <typename R>
__global__ void __launch_bounds__(kBlock, 4)
mppi_kernel(DevParams<R> q, int ld, int S, int iters, R sigma, double inv_lam, uint32_t key0, uint32_t key1, uint32_t iter_base,
            const uint32_t* __restrict__ iter_offset, uint32_t index_base, const R* __restrict__ p0, const R* __restrict__ v0,
            const R* __restrict__ goal, const R* U_in, R* U_out, const R* __restrict__ spheres, int K, R w_obs, R* __restrict__ cost_out,
            R* __restrict__ trace, uint64_t* __restrict__ keys) {
  HIP_DYNAMIC_SHARED(unsigned char, lds_raw)
  const int N = q.N, rows = 3 * N, NT = (int)blockDim.x, W = NT / kWave;
  const int tid = (int)threadIdx.x, wave = tid / kWave;
  const int p = (int)blockIdx.x;
  const LdsView<R> l = lds_view<R>(lds_raw, lds_layout(N, K, W, sizeof(R)));
  R* U = l.U;
  for (int r = tid; r < rows; r += NT) U[r] = U_in[(size_t)r * ld + p];
  stage_spheres(q, spheres, K, l.sph);
  Ctx<R> c = load_ctx(q, ld, p, key0, key1, index_base + (uint32_t)p, p0, v0, goal, U, l.sph, K, w_obs);
  const uint32_t g0 = iter_base + (iter_offset != nullptr ? *iter_offset : 0u);
  __syncthreads();
  for (int it = 0; it < iters; ++it) {
    c.g = g0 + (uint32_t)it;
    const double m = weighted_pass<R>(c, U, 0, S, sigma, inv_lam, l.acc, l.part, l.red);
    nominal_update(q, l.acc, U, m, trace, (size_t)it * ld + p);
  }
  if (wave == 0) write_nominal_cost(c, p, index_base, cost_out, keys);
  for (int r = tid; r < rows; r += NT) U_out[(size_t)r * ld + p] = U[r];
}

// One iteration's samples materialised: column p * S + s of T_out [3N][ld_out]; noise [3N][ld_out] (normals) and raw [4N][ld_out]
// (Philox words, row 4k + j) when given.
template <typename R>
__global__ void __launch_bounds__(256)
mppi_samples_kernel(DevParams<R> q, int nprob, int ld, int S, R sigma, uint32_t key0, uint32_t key1, uint32_t g, uint32_t index_base,
                    const R* __restrict__ U_in, R* __restrict__ T_out, int ld_out, R* __restrict__ noise, uint32_t* __restrict__ raw) {
  const long long col = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (col >= (long long)S * nprob) return;
  const int p = (int)(col / S);
  const uint32_t s = (uint32_t)(col % S);
  Ctx<R> c;
  c.q = q; c.key0 = key0; c.key1 = key1; c.qi = index_base + (uint32_t)p; c.g = g; c.U = U_in; c.sph = nullptr; c.K = 0; c.w_obs = (R)0;
  const R sig = s == 0 ? (R)0 : sigma;
  for (int k = 0; k < q.N; ++k) {
    R Uk[3], t[3], n[3];
    for (int a = 0; a < 3; ++a) Uk[a] = U_in[(size_t)(3 * k + a) * ld + p];
    uint32_t x[4];
    draw(c, Uk, s, k, sig, t, x, n);
    for (int a = 0; a < 3; ++a) {
      T_out[(size_t)(3 * k + a) * ld_out + col] = t[a];
      if (noise != nullptr) noise[(size_t)(3 * k + a) * ld_out + col] = n[a];
    }
    if (raw != nullptr)
      for (int j = 0; j < 4; ++j) raw[(size_t)(4 * k + j) * ld_out + col] = x[j];
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
template <typename R>
static int mppi_impl(const se3mpc_params* p, int nprob, int ld, int S, int iters, double sigma, double temperature, uint64_t seed,
                     uint32_t iter_base, const uint32_t* iter_offset, uint32_t index_base, const R* p0, const R* v0, const R* goal,
                     const R* U_in, R* U_out, const R* spheres, int K, double obstacle_weight, R* cost, R* trace, uint64_t* keys,
                     void* stream) {
  const int rc = check_mppi_args("se3mpc_mppi", p, nprob, ld, S, iters, sigma, temperature, K, obstacle_weight);
  if (rc) return rc;
  if (nprob == 0) return SE3MPC_OK;
  if (!p0 || !v0 || (p->has_goal && !goal) || !U_in || !U_out || !cost || (K > 0 && !spheres)) return fail(SE3MPC_ERR_NULL, "se3mpc_mppi: NULL operand");
  const int NT = S < kBlock ? S : kBlock;
  const Lds L = lds_layout(p->horizon, K, NT / kWave, sizeof(R));
  const DevParams<R> q = make_dev_params<R>(*p);
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(mppi_kernel<R>, dim3(nprob), dim3(NT), L.total, st, q, ld, S, iters, (R)sigma, 1.0 / temperature, k0, k1, iter_base,
                     iter_offset, index_base, p0, v0, goal, U_in, U_out, spheres, K, (R)obstacle_weight, cost, trace, keys);
  return launch_status("se3mpc_mppi");
}

template <typename R>
static int mppi_samples_impl(const se3mpc_params* p, int nprob, int ld, int S, double sigma, uint64_t seed, uint32_t iter_base,
                             uint32_t index_base, const R* U_in, R* T_out, int ld_out, R* noise, uint32_t* raw, void* stream) {
  const int rc = check_mppi_batch("se3mpc_mppi_samples", p, nprob, ld, S, sigma);
  if (rc) return rc;
  if ((long long)S * nprob > (long long)ld_out || (long long)S * nprob > 0x7FFFFFFFLL) return fail(SE3MPC_ERR_SHAPE, "se3mpc_mppi_samples: ld_out < S * nprob");
  if (nprob == 0) return SE3MPC_OK;
  if (!U_in || !T_out) return fail(SE3MPC_ERR_NULL, "se3mpc_mppi_samples: NULL operand");
  const long long cols = (long long)S * nprob;
  hipLaunchKernelGGL(mppi_samples_kernel<R>, dim3((unsigned)((cols + 255) / 256)), dim3(256), 0, (hipStream_t)stream, make_dev_params<R>(*p), nprob,
                     ld, S, (R)sigma, (uint32_t)seed, (uint32_t)(seed >> 32), iter_base, index_base, U_in, T_out, ld_out, noise, raw);
  return launch_status("se3mpc_mppi_samples");
}

}  // namespace mppi
}  // namespace se3mpc

using se3mpc::mppi::mppi_impl;
using se3mpc::mppi::mppi_samples_impl;

extern "C" int se3mpc_mppi_f32(const se3mpc_params* p, int nprob, int ld, int S, int iters, double sigma, double temperature, uint64_t seed,
                               uint32_t iter_base, const uint32_t* iter_offset, uint32_t index_base, const float* p0, const float* v0,
                               const float* goal, const float* U_in, float* U_out, const float* spheres, int K, double obstacle_weight,
                               float* cost, float* trace, uint64_t* keys, void* stream) {
  return mppi_impl<float>(p, nprob, ld, S, iters, sigma, temperature, seed, iter_base, iter_offset, index_base, p0, v0, goal, U_in, U_out, spheres,
                          K, obstacle_weight, cost, trace, keys, stream);
}
extern "C" int se3mpc_mppi_f64(const se3mpc_params* p, int nprob, int ld, int S, int iters, double sigma, double temperature, uint64_t seed,
                               uint32_t iter_base, const uint32_t* iter_offset, uint32_t index_base, const double* p0, const double* v0,
                               const double* goal, const double* U_in, double* U_out, const double* spheres, int K, double obstacle_weight,
                               double* cost, double* trace, uint64_t* keys, void* stream) {
  return mppi_impl<double>(p, nprob, ld, S, iters, sigma, temperature, seed, iter_base, iter_offset, index_base, p0, v0, goal, U_in, U_out, spheres,
                           K, obstacle_weight, cost, trace, keys, stream);
}
extern "C" int se3mpc_mppi_samples_f32(const se3mpc_params* p, int nprob, int ld, int S, double sigma, uint64_t seed, uint32_t iter_base,
                                       uint32_t index_base, const float* U_in, float* T_out, int ld_out, float* noise, uint32_t* raw, void* stream) {
  return mppi_samples_impl<float>(p, nprob, ld, S, sigma, seed, iter_base, index_base, U_in, T_out, ld_out, noise, raw, stream);
}
extern "C" int se3mpc_mppi_samples_f64(const se3mpc_params* p, int nprob, int ld, int S, double sigma, uint64_t seed, uint32_t iter_base,
                                       uint32_t index_base, const double* U_in, double* T_out, int ld_out, double* noise, uint32_t* raw,
                                       void* stream) {
  return mppi_samples_impl<double>(p, nprob, ld, S, sigma, seed, iter_base, index_base, U_in, T_out, ld_out, noise, raw, stream);
}
