// mppi_tracks.hip -- the MPPI planner of mppi_moving.hip around spheres with a PREDICTED PATH: behind the K rows of the
// moving table come Kt tracked rows whose centre is given per step of the horizon, not as c + v t.
//
// tracks [N][Kt][4] = (x, y, z, radius) per problem (track_stride elements apart; 0: one slab for all): row [k][j] is sphere j at the time of
// the state before step k, the instant stime[k] names.  The slab is staged into LDS once per launch behind the moving image, the radius folded
// to (r + margin)^2 as stage_spheres folds it, and roll_step walks the K moving rows as it always did and then the Kt rows of step k with the
// same expression and no time arithmetic.  Everything else is mppi_moving_kernel, through the functions of mppi_device.hpp with their TRACKED
// switch on: Kt = 0 gives mppi_moving_kernel's bits, and tracks that hold a constant centre give those of K + Kt moving rows whose last Kt
// velocities are zero.
#include "mppi_device.hpp"

namespace se3mpc {
namespace mppi {

template <typename R>
__global__ void __launch_bounds__(kBlock, 4)
mppi_tracks_kernel(DevParams<R> q, int ld, int S, int iters, R sigma, double inv_lam, uint32_t key0, uint32_t key1, uint32_t iter_base,
                   const uint32_t* __restrict__ iter_offset, uint32_t index_base, const R* __restrict__ p0, const R* __restrict__ v0,
                   const R* __restrict__ goal, const R* U_in, R* U_out, const R* __restrict__ spheres, const R* __restrict__ sphere_vel,
                   double sphere_t0, double plan_dt, int K, const R* __restrict__ tracks, int Kt, long long track_stride, R w_obs,
                   R* __restrict__ cost_out, R* __restrict__ trace, uint64_t* __restrict__ keys) {
  HIP_DYNAMIC_SHARED(unsigned char, lds_raw)
  const int N = q.N, rows = 3 * N, NT = (int)blockDim.x, W = NT / kWave;
  const int tid = (int)threadIdx.x, wave = tid / kWave;
  const int p = (int)blockIdx.x;
  const LdsView<R> l = lds_view<R>(lds_raw, lds_layout(N, K, W, sizeof(R)));
  const MovingLds M = moving_lds_layout(N, K, W, sizeof(R));
  const TrackLds T = track_lds_layout(M.total, N, Kt, sizeof(R));
  R* vel = reinterpret_cast<R*>(lds_raw + M.vel);
  R* stime = reinterpret_cast<R*>(lds_raw + M.time);
  R* trk = reinterpret_cast<R*>(lds_raw + T.trk);
  R* U = l.U;
  for (int r = tid; r < rows; r += NT) U[r] = U_in[(size_t)r * ld + p];
  stage_spheres(q, spheres, K, l.sph);
  for (int i = tid; i < 3 * K; i += NT) vel[i] = sphere_vel[i];
  for (int k = tid; k < N; k += NT) stime[k] = (R)(sphere_t0 + (double)k * plan_dt);
  if (Kt > 0) stage_spheres(q, tracks + (size_t)p * (size_t)track_stride, N * Kt, trk);
  Ctx<R, true, true> c = load_ctx<R, true, true>(q, ld, p, key0, key1, index_base + (uint32_t)p, p0, v0, goal, U, l.sph, K, w_obs);
  c.svel = vel;
  c.stime = stime;
  c.trk = trk;
  c.Kt = Kt;
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
static int mppi_tracks_impl(const se3mpc_params* p, int nprob, int ld, int S, int iters, double sigma, double temperature, uint64_t seed,
                            uint32_t iter_base, const uint32_t* iter_offset, uint32_t index_base, const R* p0, const R* v0, const R* goal,
                            const R* U_in, R* U_out, const R* spheres, const R* sphere_vel, double sphere_t0, int K, const R* tracks, int Kt,
                            long long track_stride, double obstacle_weight, R* cost, R* trace, uint64_t* keys, void* stream) {
  const char* fn = "se3mpc_mppi_tracks";
  int rc = check_mppi_args(fn, p, nprob, ld, S, iters, sigma, temperature, K, obstacle_weight);
  if (rc) return rc;
  rc = check_moving_args(fn, K, sphere_vel, sphere_t0);
  if (rc) return rc;
  rc = check_track_args(fn, K, Kt, tracks, track_stride, p->horizon);
  if (rc) return rc;
  if (nprob == 0) return SE3MPC_OK;
  if (!p0 || !v0 || (p->has_goal && !goal) || !U_in || !U_out || !cost || (K > 0 && !spheres)) return fail(SE3MPC_ERR_NULL, "NULL operand", fn);
  const int NT = S < kBlock ? S : kBlock;
  const TrackLds T = track_lds_layout(moving_lds_layout(p->horizon, K, NT / kWave, sizeof(R)).total, p->horizon, Kt, sizeof(R));
  const DevParams<R> q = make_dev_params<R>(*p);
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  hipLaunchKernelGGL(mppi_tracks_kernel<R>, dim3(nprob), dim3(NT), T.total, (hipStream_t)stream, q, ld, S, iters, (R)sigma, 1.0 / temperature, k0,
                     k1, iter_base, iter_offset, index_base, p0, v0, goal, U_in, U_out, spheres, sphere_vel, sphere_t0, p->dt, K, tracks, Kt,
                     track_stride, (R)obstacle_weight, cost, trace, keys);
  return launch_status(fn);
}

}  // namespace mppi
}  // namespace se3mpc

using se3mpc::mppi::mppi_tracks_impl;

extern "C" int se3mpc_mppi_tracks_f32(const se3mpc_params* p, int nprob, int ld, int S, int iters, double sigma, double temperature,
                                      uint64_t seed, uint32_t iter_base, const uint32_t* iter_offset, uint32_t index_base, const float* p0,
                                      const float* v0, const float* goal, const float* U_in, float* U_out, const float* spheres,
                                      const float* sphere_vel, double sphere_t0, int K, const float* tracks, int Kt, long long track_stride,
                                      double obstacle_weight, float* cost, float* trace, uint64_t* keys, void* stream) {
  return mppi_tracks_impl<float>(p, nprob, ld, S, iters, sigma, temperature, seed, iter_base, iter_offset, index_base, p0, v0, goal, U_in, U_out,
                                 spheres, sphere_vel, sphere_t0, K, tracks, Kt, track_stride, obstacle_weight, cost, trace, keys, stream);
}
extern "C" int se3mpc_mppi_tracks_f64(const se3mpc_params* p, int nprob, int ld, int S, int iters, double sigma, double temperature,
                                      uint64_t seed, uint32_t iter_base, const uint32_t* iter_offset, uint32_t index_base, const double* p0,
                                      const double* v0, const double* goal, const double* U_in, double* U_out, const double* spheres,
                                      const double* sphere_vel, double sphere_t0, int K, const double* tracks, int Kt, long long track_stride,
                                      double obstacle_weight, double* cost, double* trace, uint64_t* keys, void* stream) {
  return mppi_tracks_impl<double>(p, nprob, ld, S, iters, sigma, temperature, seed, iter_base, iter_offset, index_base, p0, v0, goal, U_in, U_out,
                                  spheres, sphere_vel, sphere_t0, K, tracks, Kt, track_stride, obstacle_weight, cost, trace, keys, stream);
}
