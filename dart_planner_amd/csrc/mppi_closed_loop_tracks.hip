// mppi_closed_loop_tracks.hip -- the closed-loop MPPI Monte-Carlo of mppi_closed_loop_moving.hip around spheres with a PREDICTED PATH
// (DESIGN.md 5.8h): every drone and every planning cycle in ONE launch, behind the K moving rows Kt tracked rows whose centres the caller
// gives per cycle, per drone and per step of the horizon -- tracks [cycles][B][N][Kt][4] = (x, y, z, radius), predictions renewed every
// cycle, so cycle c of the CALL plans around slab c (row [k][j] = sphere j at the state before step k of that cycle's plan).  The slab of a
// cycle is staged into LDS where the cycle's step times are refilled (one barrier publishes both).  The cycle is
// mppi_closed_loop_moving_kernel's, through the same functions with their TRACKED switch on.  The in-flight clearance sees the K moving
// rows only: a track is a prediction at plan steps, not a surface at simulator steps.  Kt = 0 gives mppi_closed_loop_moving_kernel's bits.
#pragma clang fp contract(off)
#include "closed_loop_device.hpp"
#pragma clang fp contract(fast)
#include "mppi_device.hpp"
#include "mppi_loop_device.hpp"

namespace se3mpc {
namespace mppi {

// Wavefronts per SIMD: those of mppi_closed_loop_moving_kernel
template <typename R>
struct TrackLoopWaves { static constexpr int value = 3; };
template <>
struct TrackLoopWaves<double> { static constexpr int value = 2; };

template <typename R>
__global__ void __launch_bounds__(kBlock, TrackLoopWaves<R>::value)
mppi_closed_loop_tracks_kernel(DevParams<R> q, CtrlDev<R> ctl, SimDev<R> sim, double plan_dt, int cycles, int substeps, double sim_dt,
                               uint32_t cycle_base, int shift, int S, int iters, R sigma, double inv_lam, uint32_t key0, uint32_t key1,
                               uint32_t iter_base, uint32_t index_base, const R* __restrict__ goalg, const R* __restrict__ spheres,
                               const R* __restrict__ sphere_vel, double sphere_t0, int K, const R* __restrict__ tracks, int Kt, R w_obs,
                               const R* __restrict__ windg, long long wind_stride, double* __restrict__ timeg, R* __restrict__ posg,
                               R* __restrict__ velg, R* __restrict__ attg, R* __restrict__ omegag, double* __restrict__ stateg,
                               R* __restrict__ Ug, R* __restrict__ cost_out, R* __restrict__ trace, R* __restrict__ plan_last,
                               R* __restrict__ clearance) {
  HIP_DYNAMIC_SHARED(unsigned char, lds_raw)
  const int N = q.N, rows = 3 * N, NT = (int)blockDim.x, W = NT / kWave;
  const int tid = (int)threadIdx.x, wave = tid / kWave;
  const int b = (int)blockIdx.x;
  const LoopLds X = loop_lds_layout(N, K, W, sizeof(R), true);
  const MovingLds M = moving_lds_layout(N, K, W, sizeof(R));
  const TrackLds TL = track_lds_layout(X.total, N, Kt, sizeof(R));
  const LdsView<R> l = lds_view<R>(lds_raw, lds_layout(N, K, W, sizeof(R)));
  R* U = l.U;
  R* sph = l.sph;
  R* svel = reinterpret_cast<R*>(lds_raw + M.vel);
  R* stime = reinterpret_cast<R*>(lds_raw + M.time);
  R* trk = reinterpret_cast<R*>(lds_raw + TL.trk);
  const DroneBlock<R> d = drone_block<R>(lds_raw + X.stamps, N, X.plan - X.stamps, X.vec - X.stamps);
  R* s_vec = d.vec;                                         // pos, vel, att, omega, wind | goal, running clearance
  R* rad = reinterpret_cast<R*>(lds_raw + X.rad);
  R* park = reinterpret_cast<R*>(lds_raw + X.park);         // [kPark][4] = (x, y, z, tR)
  const bool want_clear = clearance != nullptr && K > 0;

  for (int r = tid; r < rows; r += NT) U[r] = Ug[(size_t)b * rows + r];
  stage_spheres(q, spheres, K, sph);
  for (int i = tid; i < 3 * K; i += NT) svel[i] = sphere_vel[i];
  for (int j = tid; j < K; j += NT) rad[j] = spheres[4 * j + 3];
  if (tid == 0) {
    drone_load<R>(d, b, posg, velg, attg, omegag, windg, wind_stride, timeg, stateg);
    for (int i = 0; i < 3; ++i) s_vec[15 + i] = q.has_goal ? goalg[3 * b + i] : (R)0;
    s_vec[18] = want_clear ? clearance[b] : (R)0;
  }
  __syncthreads();
  // the planner's context as mppi_tracks_kernel builds it, from the LDS copies of the state and the goal (members named one by one: see
  // mppi_closed_loop.hip)
  Ctx<R, true, true> c = load_ctx<R, true, true>(q, 1, 0, key0, key1, index_base + (uint32_t)b, s_vec, s_vec + 3, s_vec + 15, U, sph, K, w_obs);
  c.svel = svel;
  c.stime = stime;
  c.trk = trk;
  c.Kt = Kt;
  c.gl[0] = wave_bcast(c.gl[0], 0); c.gl[1] = wave_bcast(c.gl[1], 0); c.gl[2] = wave_bcast(c.gl[2], 0);

  for (int cyc = 0; cyc < cycles; ++cyc) {
    const uint32_t C = cycle_base + (uint32_t)cyc;
    const bool last = cyc == cycles - 1;
    // ---- the step times and the slab of this cycle's plan (the previous cycle's last readers are behind shift_nominal's barriers)
    for (int k = tid; k < N; k += NT) stime[k] = (R)(sphere_t0 + plan_stamp((int)C, substeps, sim_dt, k, plan_dt));
    if (Kt > 0) stage_spheres(q, tracks + ((size_t)cyc * gridDim.x + b) * (size_t)(4 * N * Kt), N * Kt, trk);
    __syncthreads();
    // ---- plan
    c.p0[0] = wave_bcast(s_vec[0], 0); c.p0[1] = wave_bcast(s_vec[1], 0); c.p0[2] = wave_bcast(s_vec[2], 0);
    c.v0[0] = wave_bcast(s_vec[3], 0); c.v0[1] = wave_bcast(s_vec[4], 0); c.v0[2] = wave_bcast(s_vec[5], 0);
    const uint32_t g0 = iter_base + C * (uint32_t)iters;
    for (int it = 0; it < iters; ++it) {
      c.g = g0 + (uint32_t)it;
      const double m = weighted_pass<R>(c, U, 0, S, sigma, inv_lam, l.acc, l.part, l.red);
      nominal_update(q, l.acc, U, m, trace, ((size_t)b * cycles + cyc) * iters + it);
    }
    if (last && wave == 0) write_nominal_cost(c, b, index_base, cost_out, (uint64_t*)nullptr);
    // ---- hand over: the nominal's trajectory, row k = the state before step k
    if (tid == 0) {
      R p[3] = {c.p0[0], c.p0[1], c.p0[2]}, v[3] = {c.v0[0], c.v0[1], c.v0[2]};
      hand_over_plan(q, p, v, U, d, N, (int)C, substeps, sim_dt, plan_dt);
    }
    // ---- act, in chunks of kPark steps: the first lane flies and parks (position, time), then the workgroup measures the clearance
    int s0 = 0;
    do {
      const int n = substeps - s0 < kPark ? substeps - s0 : kPark;
      if (tid == 0 && n > 0)
        fly_steps<R>(ctl, sim, d, N, n, sim_dt, [&](int step, const R* p) {
          if (want_clear) {
            park[4 * step] = p[0]; park[4 * step + 1] = p[1]; park[4 * step + 2] = p[2];
            park[4 * step + 3] = (R)(sphere_t0 + (double)((int)C * substeps + s0 + step + 1) * sim_dt);
          }
        });
      __syncthreads();
      if (want_clear && n > 0) clearance_chunk<R, true>(park, sph, rad, n, K, l.red, s_vec + 18, svel);
      s0 += kPark;
    } while (s0 < substeps);
    if (last && plan_last != nullptr)
      for (int r = tid; r < 3 * rows; r += NT) plan_last[(size_t)b * 3 * rows + r] = d.planP[r];
    // ---- warm start of the next cycle
    shift_nominal(q, U, reinterpret_cast<R*>(l.acc), shift);
  }

  for (int r = tid; r < rows; r += NT) Ug[(size_t)b * rows + r] = U[r];
  if (tid == 0) {
    drone_store<R>(d, b, posg, velg, attg, omegag, timeg, stateg);
    if (want_clear) clearance[b] = s_vec[18];
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
template <typename R>
static int mppi_closed_loop_tracks_impl(const se3mpc_params* p, const se3mpc_controller_params* cp, const se3mpc_simulator_params* sp, int B,
                                        int cycles, int substeps, double sim_dt, uint32_t cycle_base, int shift, int S, int iters, double sigma,
                                        double temperature, uint64_t seed, uint32_t iter_base, uint32_t index_base, const R* goal,
                                        const R* spheres, const R* sphere_vel, double sphere_t0, int K, const R* tracks, int Kt,
                                        double obstacle_weight, const R* wind, long long wind_stride, double* time, R* pos, R* vel, R* att, R* omega, double* state, R* U, R* cost,
                                        R* trace, R* plan_last, R* clearance, void* stream) {
  const char* fn = "se3mpc_mppi_closed_loop_tracks";
  if (p == nullptr || cp == nullptr || sp == nullptr) return fail(SE3MPC_ERR_NULL, "NULL parameter struct", fn);
  int rc = check_params_impl(p);
  if (rc) return fail(rc, "invalid se3mpc_params", fn);
  rc = check_controller_params(cp);
  if (rc) return fail(rc, "invalid se3mpc_controller_params", fn);
  rc = check_simulator_params(sp);
  if (rc) return fail(rc, "invalid se3mpc_simulator_params", fn);
  if (cycles < 0 || substeps < 0) return fail(SE3MPC_ERR_SHAPE, "cycles or substeps < 0", fn);
  if (shift < 0 || shift > p->horizon) return fail(SE3MPC_ERR_SHAPE, "shift outside [0, horizon]", fn);
  if (wind != nullptr && !(wind_stride == 0 || wind_stride >= 3)) return fail(SE3MPC_ERR_SHAPE, "wind_stride must be 0 or >= 3", fn);
  rc = check_mppi_args(fn, p, B, B, S, iters, sigma, temperature, K, obstacle_weight);
  if (rc) return rc;
  if (!std::isfinite(sim_dt)) return fail(SE3MPC_ERR_PARAM, "sim_dt must be finite", fn);
  rc = check_moving_args(fn, K, sphere_vel, sphere_t0);
  if (rc) return rc;
  rc = check_track_args(fn, K, Kt, tracks, 0, p->horizon);
  if (rc) return rc;
  if (B == 0 || cycles == 0) return SE3MPC_OK;
  if (!time || !pos || !vel || !att || !omega || !state || !U || !cost || (p->has_goal && !goal) || (K > 0 && !spheres))
    return fail(SE3MPC_ERR_NULL, "NULL operand", fn);
  const int NT = S < kBlock ? S : kBlock;
  const LoopLds X = loop_lds_layout(p->horizon, K, NT / kWave, sizeof(R), true);
  const TrackLds TL = track_lds_layout(X.total, p->horizon, Kt, sizeof(R));
  hipLaunchKernelGGL(mppi_closed_loop_tracks_kernel<R>, dim3(B), dim3(NT), TL.total, (hipStream_t)stream, make_dev_params<R>(*p),
                     make_ctrl_dev<R>(*cp), make_sim_dev<R>(*sp), p->dt, cycles, substeps, sim_dt, cycle_base, shift, S, iters, (R)sigma,
                     1.0 / temperature, (uint32_t)seed, (uint32_t)(seed >> 32), iter_base, index_base, goal, spheres, sphere_vel, sphere_t0, K,
                     tracks, Kt, (R)obstacle_weight, wind, wind_stride, time, pos, vel, att, omega, state, U, cost, trace, plan_last, clearance);
  return launch_status(fn);
}

}  // namespace mppi
}  // namespace se3mpc

using se3mpc::mppi::mppi_closed_loop_tracks_impl;

extern "C" int se3mpc_mppi_closed_loop_tracks_f32(const se3mpc_params* p, const se3mpc_controller_params* cp, const se3mpc_simulator_params* sp,
                                                  int B, int cycles, int substeps, double sim_dt, uint32_t cycle_base, int shift, int S, int iters,
                                                  double sigma, double temperature, uint64_t seed, uint32_t iter_base, uint32_t index_base,
                                                  const float* goal, const float* spheres, const float* sphere_vel, double sphere_t0, int K, const float* tracks, int Kt,
                                                  double obstacle_weight, const float* wind, long long wind_stride, double* time, float* pos,
                                                  float* vel, float* att, float* omega, double* state, float* U, float* cost, float* trace,
                                                  float* plan_last, float* clearance, void* stream) {
  return mppi_closed_loop_tracks_impl<float>(p, cp, sp, B, cycles, substeps, sim_dt, cycle_base, shift, S, iters, sigma, temperature, seed, iter_base,
                                             index_base, goal, spheres, sphere_vel, sphere_t0, K, tracks, Kt, obstacle_weight, wind, wind_stride, time, pos, vel,
                                             att, omega, state, U, cost, trace, plan_last, clearance, stream);
}
extern "C" int se3mpc_mppi_closed_loop_tracks_f64(const se3mpc_params* p, const se3mpc_controller_params* cp, const se3mpc_simulator_params* sp,
                                                  int B, int cycles, int substeps, double sim_dt, uint32_t cycle_base, int shift, int S, int iters,
                                                  double sigma, double temperature, uint64_t seed, uint32_t iter_base, uint32_t index_base,
                                                  const double* goal, const double* spheres, const double* sphere_vel, double sphere_t0, int K, const double* tracks, int Kt,
                                                  double obstacle_weight, const double* wind, long long wind_stride, double* time, double* pos,
                                                  double* vel, double* att, double* omega, double* state, double* U, double* cost, double* trace,
                                                  double* plan_last, double* clearance, void* stream) {
  return mppi_closed_loop_tracks_impl<double>(p, cp, sp, B, cycles, substeps, sim_dt, cycle_base, shift, S, iters, sigma, temperature, seed, iter_base,
                                              index_base, goal, spheres, sphere_vel, sphere_t0, K, tracks, Kt, obstacle_weight, wind, wind_stride, time, pos, vel,
                                              att, omega, state, U, cost, trace, plan_last, clearance, stream);
}
