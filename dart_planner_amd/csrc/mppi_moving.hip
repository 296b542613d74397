// mppi_moving.hip -- the MPPI planner of mppi.hip around spheres that MOVE with constant velocity.
//
// The table's centres hold at a time origin and a second table [K][3] holds velocities.  The penalty of step k, on the state before step
// k as in mppi_kernel, is taken against the centres at
//   tau_k = sphere_t0 + (double)k * dt,        tR_k = (R)tau_k,        centre_j(k) = c_j + v_j * tR_k   (one multiply-add per axis)
// and is then roll_step's own expression.  The step times are filled once per launch into LDS behind the velocity table, so the sweep reads
// one uniform value per step and no float64 enters the float32 sweep.  Everything else is mppi_kernel: the functions of mppi_device.hpp
// with their MOVING switch on -- regenerated samples, nothing held per sample, no atomics, the same fold order -- so zero velocities give
// mppi_kernel's bits.
#include "mppi_device.hpp"

namespace se3mpc {
namespace mppi {

// The velocity table into LDS, by the whole workgroup; the caller's __syncthreads() publishes it
template <typename R>
__device__ __forceinline__ void stage_motion(const R* __restrict__ sphere_vel, int K, R* vel) {
  for (int i = (int)threadIdx.x; i < 3 * K; i += (int)blockDim.x) vel[i] = sphere_vel[i];
}

template <typename R>
__global__ void __launch_bounds__(kBlock, 4)
mppi_moving_kernel(DevParams<R> q, int ld, int S, int iters, R sigma, double inv_lam, uint32_t key0, uint32_t key1, uint32_t iter_base,
                   const uint32_t* __restrict__ iter_offset, uint32_t index_base, const R* __restrict__ p0, const R* __restrict__ v0,
                   const R* __restrict__ goal, const R* U_in, R* U_out, const R* __restrict__ spheres, const R* __restrict__ sphere_vel,
                   double sphere_t0, double plan_dt, int K, R w_obs, R* __restrict__ cost_out, R* __restrict__ trace,
                   uint64_t* __restrict__ keys) {
  HIP_DYNAMIC_SHARED(unsigned char, lds_raw)
  const int N = q.N, rows = 3 * N, NT = (int)blockDim.x, W = NT / kWave;
  const int tid = (int)threadIdx.x, wave = tid / kWave;
  const int p = (int)blockIdx.x;
  const LdsView<R> l = lds_view<R>(lds_raw, lds_layout(N, K, W, sizeof(R)));
  const MovingLds M = moving_lds_layout(N, K, W, sizeof(R));
  R* vel = reinterpret_cast<R*>(lds_raw + M.vel);
  R* stime = reinterpret_cast<R*>(lds_raw + M.time);
  R* U = l.U;
  for (int r = tid; r < rows; r += NT) U[r] = U_in[(size_t)r * ld + p];
  stage_spheres(q, spheres, K, l.sph);
  stage_motion(sphere_vel, K, vel);
  for (int k = tid; k < N; k += NT) stime[k] = (R)(sphere_t0 + (double)k * plan_dt);
  Ctx<R, true> c = load_ctx<R, true>(q, ld, p, key0, key1, index_base + (uint32_t)p, p0, v0, goal, U, l.sph, K, w_obs);
  c.svel = vel;
  c.stime = stime;
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

// ---- host side ------------------------------------------------------------------------------------------------------------------------
template <typename R>
static int mppi_moving_impl(const se3mpc_params* p, int nprob, int ld, int S, int iters, double sigma, double temperature, uint64_t seed,
                            uint32_t iter_base, const uint32_t* iter_offset, uint32_t index_base, const R* p0, const R* v0, const R* goal,
                            const R* U_in, R* U_out, const R* spheres, const R* sphere_vel, double sphere_t0, int K, double obstacle_weight,
                            R* cost, R* trace, uint64_t* keys, void* stream) {
  int rc = check_mppi_args("se3mpc_mppi_moving", p, nprob, ld, S, iters, sigma, temperature, K, obstacle_weight);
  if (rc) return rc;
  rc = check_moving_args("se3mpc_mppi_moving", K, sphere_vel, sphere_t0);
  if (rc) return rc;
  if (nprob == 0) return SE3MPC_OK;
  if (!p0 || !v0 || (p->has_goal && !goal) || !U_in || !U_out || !cost || (K > 0 && !spheres))
    return fail(SE3MPC_ERR_NULL, "se3mpc_mppi_moving: NULL operand");
  const int NT = S < kBlock ? S : kBlock;
  const MovingLds M = moving_lds_layout(p->horizon, K, NT / kWave, sizeof(R));
  const DevParams<R> q = make_dev_params<R>(*p);
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  hipLaunchKernelGGL(mppi_moving_kernel<R>, dim3(nprob), dim3(NT), M.total, (hipStream_t)stream, q, ld, S, iters, (R)sigma, 1.0 / temperature, k0,
                     k1, iter_base, iter_offset, index_base, p0, v0, goal, U_in, U_out, spheres, sphere_vel, sphere_t0, p->dt, K,
                     (R)obstacle_weight, cost, trace, keys);
  return launch_status("se3mpc_mppi_moving");
}

}  // namespace mppi
}  // namespace se3mpc

using se3mpc::mppi::mppi_moving_impl;

extern "C" int se3mpc_mppi_moving_f32(const se3mpc_params* p, int nprob, int ld, int S, int iters, double sigma, double temperature,
                                      uint64_t seed, uint32_t iter_base, const uint32_t* iter_offset, uint32_t index_base, const float* p0,
                                      const float* v0, const float* goal, const float* U_in, float* U_out, const float* spheres,
                                      const float* sphere_vel, double sphere_t0, int K, double obstacle_weight, float* cost, float* trace,
                                      uint64_t* keys, void* stream) {
  return mppi_moving_impl<float>(p, nprob, ld, S, iters, sigma, temperature, seed, iter_base, iter_offset, index_base, p0, v0, goal, U_in, U_out,
                                 spheres, sphere_vel, sphere_t0, K, obstacle_weight, cost, trace, keys, stream);
}
extern "C" int se3mpc_mppi_moving_f64(const se3mpc_params* p, int nprob, int ld, int S, int iters, double sigma, double temperature,
                                      uint64_t seed, uint32_t iter_base, const uint32_t* iter_offset, uint32_t index_base, const double* p0,
                                      const double* v0, const double* goal, const double* U_in, double* U_out, const double* spheres,
                                      const double* sphere_vel, double sphere_t0, int K, double obstacle_weight, double* cost, double* trace,
                                      uint64_t* keys, void* stream) {
  return mppi_moving_impl<double>(p, nprob, ld, S, iters, sigma, temperature, seed, iter_base, iter_offset, index_base, p0, v0, goal, U_in, U_out,
                                  spheres, sphere_vel, sphere_t0, K, obstacle_weight, cost, trace, keys, stream);
}
