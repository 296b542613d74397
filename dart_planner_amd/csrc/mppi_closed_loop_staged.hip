// mppi_closed_loop_staged.hip -- the closed-loop MPPI Monte-Carlo of mppi_closed_loop.hip with the reference's full edge loop per drone
// (edge/main_improved.py:96-152): plan -> TrajectorySmoother -> GeometricController -> MotorMixer and motors -> DroneSimulator, every planning
// cycle of every drone inside ONE launch, the clearance to the spheres measured along the way.  Per cycle exactly what
// control/closed_loop.py's run_mppi launches with smoother= / mixer=: se3mpc_mppi_closed_loop_* as the planner alone,
// se3mpc_smoother_update_*, se3mpc_closed_loop_smoothed_* / se3mpc_closed_loop_actuated_* -- the same device functions (weighted_pass,
// nominal_update; smoother_take_plan, smoothed_step, actuated_step through staged_fly), hence the same bits.
//
// One workgroup of min(S, 256) lanes per drone, structured as mppi_closed_loop_kernel: plan, hand over (hand_over_plan), act on the first
// lane in chunks of kPark steps, the whole workgroup reducing the clearance of the positions each chunk parked (clearance_chunk), warm start.
// One plan per drone is enough, as in monte_carlo_staged.hip: update_trajectory reads the plan being followed once, at the drone's clock at
// the start of the cycle, which is its clock at the end of the act phase before -- so the first lane takes that sample at the end of every act
// phase and parks its nine values.  They come from `followed` at the start of a launch and go back at its end (the sample is taken after the
// last cycle too), so a run can be continued by a second launch with cycle_base.
// Between chunks the smoother's, the mixer's and the controller's registers go back to their LDS records; smoother_take_plan runs in the
// first chunk of a cycle only, smoother_sample_followed in the last.  Behind loop_lds_layout's image lie the records of the stages the
// variant has (StagedRecords).  All constants stay kernel arguments (parked in LDS they spill).  Without either stage the
// entry point IS se3mpc_mppi_closed_loop_*.
#pragma clang fp contract(off)
#include "staged_device.hpp"
#pragma clang fp contract(fast)
#include "mppi_device.hpp"
#include "mppi_loop_device.hpp"

namespace se3mpc {
namespace mppi {

// Wavefronts per SIMD each instantiation is compiled for, chosen from the ISA (tests/test_mppi_closed_loop_staged_isa.py):
// the most at which the act phase -- controller, smoother and mixer in one lane's registers -- spills nothing.  float: smoother 178 and both
// 195 registers (two wavefronts; at three they spill 3 / 17), mixer alone 156 (three).  double: 256 registers and 5 (mixer) / 28 (smoother) /
// 52 (both) accumulator registers (one wavefront; at two they spill 7 / 37 / 65).
template <typename R, bool SMOOTH, bool MIX>
struct StagedLoopWaves { static constexpr int value = 2; };
template <>
struct StagedLoopWaves<float, false, true> { static constexpr int value = 3; };
template <bool SMOOTH, bool MIX>
struct StagedLoopWaves<double, SMOOTH, MIX> { static constexpr int value = 1; };

template <typename R, bool SMOOTH, bool MIX>
__global__ void __launch_bounds__(kBlock, (StagedLoopWaves<R, SMOOTH, MIX>::value))
mppi_closed_loop_staged_kernel(DevParams<R> q, CtrlDev<R> ctl, SimDev<R> sim, SmoothDev<R> smd, MixDev<R> mxd, double plan_dt, int cycles, int substeps,
                               double sim_dt, uint32_t cycle_base, int shift, int S, int iters, R sigma, double inv_lam, uint32_t key0, uint32_t key1,
                               uint32_t iter_base, uint32_t index_base, const R* __restrict__ goalg, const R* __restrict__ spheres, int K, R w_obs,
                               const R* __restrict__ windg, long long wind_stride, double* __restrict__ timeg, R* __restrict__ posg,
                               R* __restrict__ velg, R* __restrict__ attg, R* __restrict__ omegag, double* __restrict__ stateg,
                               double* __restrict__ smootherg, double* __restrict__ mixerg, const R* __restrict__ healthg, long long health_stride,
                               R* __restrict__ followedg, R* __restrict__ Ug, R* __restrict__ cost_out, R* __restrict__ trace,
                               R* __restrict__ plan_last, R* __restrict__ clearance) {
  HIP_DYNAMIC_SHARED(unsigned char, lds_raw)
  const int N = q.N, rows = 3 * N, NT = (int)blockDim.x, W = NT / kWave;
  const int tid = (int)threadIdx.x, wave = tid / kWave;
  const int b = (int)blockIdx.x;
  const LoopLds X = loop_lds_layout(N, K, W, sizeof(R));
  const LdsView<R> l = lds_view<R>(lds_raw, lds_layout(N, K, W, sizeof(R)));
  R* U = l.U;
  R* sph = l.sph;
  const DroneBlock<R> d = drone_block<R>(lds_raw + X.stamps, N, X.plan - X.stamps, X.vec - X.stamps);
  const StagedBlock<R> sb = staged_block_at<R, SMOOTH, MIX>(d, lds_raw + X.total);      // the stages' records behind the loop's image
  R* s_vec = d.vec;                                         // pos, vel, att, omega, wind | goal, running clearance
  R* rad = reinterpret_cast<R*>(lds_raw + X.rad);
  R* park = reinterpret_cast<R*>(lds_raw + X.park);
  const bool want_clear = clearance != nullptr && K > 0;

  for (int r = tid; r < rows; r += NT) U[r] = Ug[(size_t)b * rows + r];
  stage_spheres(q, spheres, K, sph);
  for (int j = tid; j < K; j += NT) rad[j] = spheres[4 * j + 3];
  if (tid == 0) {
    drone_load<R>(d, b, posg, velg, attg, omegag, windg, wind_stride, timeg, stateg);
    staged_load<R, SMOOTH, MIX>(sb, b, smootherg, mixerg, healthg, health_stride, followedg);
    for (int i = 0; i < 3; ++i) s_vec[15 + i] = q.has_goal ? goalg[3 * b + i] : (R)0;
    s_vec[18] = want_clear ? clearance[b] : (R)0;
  }
  __syncthreads();
  // the planner's context as mppi_kernel builds it (load_ctx), from the LDS copies of the state and the goal
  Ctx<R> c = load_ctx(q, 1, 0, key0, key1, index_base + (uint32_t)b, s_vec, s_vec + 3, s_vec + 15, U, sph, K, w_obs);
  // (members of c are named one by one, as in mppi_closed_loop_kernel and for its reason: a loop over them would keep c in memory until the
  // loop is unrolled, which is after the pass that fixes the operand order of the cost's sums)
  c.gl[0] = wave_bcast(c.gl[0], 0); c.gl[1] = wave_bcast(c.gl[1], 0); c.gl[2] = wave_bcast(c.gl[2], 0);

  for (int cyc = 0; cyc < cycles; ++cyc) {
    const uint32_t C = cycle_base + (uint32_t)cyc;
    const bool last = cyc == cycles - 1;
    // ---- plan: the iterations of mppi_kernel from the drone's state as it stands
    c.p0[0] = wave_bcast(s_vec[0], 0); c.p0[1] = wave_bcast(s_vec[1], 0); c.p0[2] = wave_bcast(s_vec[2], 0);
    c.v0[0] = wave_bcast(s_vec[3], 0); c.v0[1] = wave_bcast(s_vec[4], 0); c.v0[2] = wave_bcast(s_vec[5], 0);
    const uint32_t g0 = iter_base + C * (uint32_t)iters;
    for (int it = 0; it < iters; ++it) {
      c.g = g0 + (uint32_t)it;
      const double m = weighted_pass<R>(c, U, 0, S, sigma, inv_lam, l.acc, l.part, l.red);
      nominal_update(q, l.acc, U, m, trace, ((size_t)b * cycles + cyc) * iters + it);
    }
    if (last && wave == 0) write_nominal_cost(c, b, index_base, cost_out, (uint64_t*)nullptr);
    // ---- hand over: the nominal's trajectory, row k = the state before step k; the plan of the cycle before is gone from here on -- its
    // one sample is parked
    if (tid == 0) {
      R p[3] = {c.p0[0], c.p0[1], c.p0[2]}, v[3] = {c.v0[0], c.v0[1], c.v0[2]};
      hand_over_plan(q, p, v, U, d, N, (int)C, substeps, sim_dt, plan_dt);
    }
    // ---- act, in chunks of kPark steps: the first lane flies, then the workgroup measures the clearance of the positions it left
    int s0 = 0;
    do {
      const int n = substeps - s0 < kPark ? substeps - s0 : kPark;
      if (tid == 0) {
        if (n > 0)
          staged_fly<R, SMOOTH, MIX>(sb, ctl, sim, smd, mxd, N, n, sim_dt, healthg != nullptr, s0 == 0, s0 + kPark >= substeps, [&](int step, const R* p) {
            if (want_clear) { park[3 * step] = p[0]; park[3 * step + 1] = p[1]; park[3 * step + 2] = p[2]; }
          });
        else if constexpr (SMOOTH)
          staged_take_only<R>(sb, smd, N);
      }
      __syncthreads();
      if (want_clear && n > 0) clearance_chunk(park, sph, rad, n, K, l.red, s_vec + 18);
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
    staged_store<R, SMOOTH, MIX>(sb, b, smootherg, mixerg, followedg);
    if (want_clear) clearance[b] = s_vec[18];
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
// se3mpc_mppi_closed_loop_* for R (the form without a stage)
static int mppi_closed_loop_plain(const se3mpc_params* p, const se3mpc_controller_params* cp, const se3mpc_simulator_params* sp, int B, int cycles,
                                  int substeps, double sim_dt, uint32_t cycle_base, int shift, int S, int iters, double sigma, double temperature,
                                  uint64_t seed, uint32_t iter_base, uint32_t index_base, const float* goal, const float* spheres, int K,
                                  double obstacle_weight, const float* wind, long long wind_stride, double* time, float* pos, float* vel, float* att,
                                  float* omega, double* state, float* U, float* cost, float* trace, float* plan_last, float* clearance, void* stream) {
  return se3mpc_mppi_closed_loop_f32(p, cp, sp, B, cycles, substeps, sim_dt, cycle_base, shift, S, iters, sigma, temperature, seed, iter_base,
                                     index_base, goal, spheres, K, obstacle_weight, wind, wind_stride, time, pos, vel, att, omega, state, U, cost, trace,
                                     plan_last, clearance, stream);
}
static int mppi_closed_loop_plain(const se3mpc_params* p, const se3mpc_controller_params* cp, const se3mpc_simulator_params* sp, int B, int cycles,
                                  int substeps, double sim_dt, uint32_t cycle_base, int shift, int S, int iters, double sigma, double temperature,
                                  uint64_t seed, uint32_t iter_base, uint32_t index_base, const double* goal, const double* spheres, int K,
                                  double obstacle_weight, const double* wind, long long wind_stride, double* time, double* pos, double* vel,
                                  double* att, double* omega, double* state, double* U, double* cost, double* trace, double* plan_last,
                                  double* clearance, void* stream) {
  return se3mpc_mppi_closed_loop_f64(p, cp, sp, B, cycles, substeps, sim_dt, cycle_base, shift, S, iters, sigma, temperature, seed, iter_base,
                                     index_base, goal, spheres, K, obstacle_weight, wind, wind_stride, time, pos, vel, att, omega, state, U, cost, trace,
                                     plan_last, clearance, stream);
}

template <typename R, bool SMOOTH, bool MIX>
static size_t staged_loop_lds_bytes(int N, int K, int W) {
  return loop_lds_layout(N, K, W, sizeof(R)).total + StagedRecords<R, SMOOTH, MIX>::bytes();
}

template <typename R>
static int mppi_closed_loop_staged_impl(const se3mpc_params* p, const se3mpc_controller_params* cp, const se3mpc_simulator_params* sp,
                                        const se3mpc_smoother_params* smp, const se3mpc_mixer_params* mp, int B, int cycles, int substeps,
                                        double sim_dt, uint32_t cycle_base, int shift, int S, int iters, double sigma, double temperature,
                                        uint64_t seed, uint32_t iter_base, uint32_t index_base, const R* goal, const R* spheres, int K,
                                        double obstacle_weight, const R* wind, long long wind_stride, double* time, R* pos, R* vel, R* att, R* omega,
                                        double* state, double* smoother_state, double* mixer_state, const R* motor_health, long long health_stride,
                                        R* followed, R* U, R* cost, R* trace, R* plan_last, R* clearance, void* stream) {
  // the rules of se3mpc_mppi_closed_loop_*, in its order, with the stages' rules where se3mpc_monte_carlo_staged_* has them
  if (p == nullptr || cp == nullptr || sp == nullptr) return fail(SE3MPC_ERR_NULL, "se3mpc_mppi_closed_loop_staged: NULL parameter struct");
  if ((smp == nullptr) != (smoother_state == nullptr))
    return fail(SE3MPC_ERR_NULL, "se3mpc_mppi_closed_loop_staged: smoother parameters and smoother_state come together or not at all");
  if ((mp == nullptr) != (mixer_state == nullptr))
    return fail(SE3MPC_ERR_NULL, "se3mpc_mppi_closed_loop_staged: mixer parameters and mixer_state come together or not at all");
  if (motor_health != nullptr && mp == nullptr) return fail(SE3MPC_ERR_NULL, "se3mpc_mppi_closed_loop_staged: motor_health needs the mixer");
  const bool smooth = smp != nullptr, mix = mp != nullptr;
  int rc = check_params_impl(p);
  if (rc) return fail(rc, "se3mpc_mppi_closed_loop_staged: invalid se3mpc_params");
  rc = check_controller_params(cp);
  if (rc) return fail(rc, "se3mpc_mppi_closed_loop_staged: invalid se3mpc_controller_params");
  rc = check_simulator_params(sp);
  if (rc) return fail(rc, "se3mpc_mppi_closed_loop_staged: invalid se3mpc_simulator_params");
  rc = smooth ? check_smoother_params(smp) : SE3MPC_OK;
  if (rc) return fail(rc, "se3mpc_mppi_closed_loop_staged: invalid se3mpc_smoother_params");
  rc = mix ? check_mixer_params(mp) : SE3MPC_OK;
  if (rc) return fail(rc, "se3mpc_mppi_closed_loop_staged: invalid se3mpc_mixer_params");
  if (cycles < 0 || substeps < 0) return fail(SE3MPC_ERR_SHAPE, "se3mpc_mppi_closed_loop_staged: cycles or substeps < 0");
  if (shift < 0 || shift > p->horizon) return fail(SE3MPC_ERR_SHAPE, "se3mpc_mppi_closed_loop_staged: shift outside [0, horizon]");
  if (wind != nullptr && !(wind_stride == 0 || wind_stride >= 3))
    return fail(SE3MPC_ERR_SHAPE, "se3mpc_mppi_closed_loop_staged: wind_stride must be 0 or >= 3");
  if (health_stride < 0) return fail(SE3MPC_ERR_SHAPE, "se3mpc_mppi_closed_loop_staged: health_stride < 0");
  rc = check_mppi_args("se3mpc_mppi_closed_loop_staged", p, B, B, S, iters, sigma, temperature, K, obstacle_weight);
  if (rc) return rc;
  if (!std::isfinite(sim_dt)) return fail(SE3MPC_ERR_PARAM, "se3mpc_mppi_closed_loop_staged: sim_dt must be finite");
  if (!smooth && !mix)
    return mppi_closed_loop_plain(p, cp, sp, B, cycles, substeps, sim_dt, cycle_base, shift, S, iters, sigma, temperature, seed, iter_base, index_base,
                                  goal, spheres, K, obstacle_weight, wind, wind_stride, time, pos, vel, att, omega, state, U, cost, trace, plan_last,
                                  clearance, stream);
  if (B == 0 || cycles == 0) return SE3MPC_OK;
  if (!time || !pos || !vel || !att || !omega || !state || !U || !cost || (p->has_goal && !goal) || (K > 0 && !spheres))
    return fail(SE3MPC_ERR_NULL, "se3mpc_mppi_closed_loop_staged: NULL operand");
  if (smooth && followed == nullptr) return fail(SE3MPC_ERR_NULL, "se3mpc_mppi_closed_loop_staged: followed is NULL with the smoother");
  const int NT = S < kBlock ? S : kBlock, W = NT / kWave, N = p->horizon;
  const CtrlDev<R> c = make_ctrl_dev<R>(*cp);
  const SimDev<R> m = make_sim_dev<R>(*sp);
  se3mpc_smoother_params no_smoother;
  se3mpc_smoother_default_params(&no_smoother);                                   // a variant without the stage never reads its constants
  const SmoothDev<R> sd = make_smooth_dev<R>(smooth ? *smp : no_smoother);
  const MixDev<R> xd = mix ? make_mix_dev<R>(*mp) : MixDev<R>{};
  auto go = [&](auto with_smoother, auto with_mixer) {
    constexpr bool SM = decltype(with_smoother)::value, MX = decltype(with_mixer)::value;
    const size_t lds = staged_loop_lds_bytes<R, SM, MX>(N, K, W);
    hipLaunchKernelGGL((mppi_closed_loop_staged_kernel<R, SM, MX>), dim3(B), dim3(NT), lds, (hipStream_t)stream,
                       make_dev_params<R>(*p), c, m, sd, xd, p->dt, cycles, substeps, sim_dt, cycle_base, shift, S, iters, (R)sigma, 1.0 / temperature,
                       (uint32_t)seed, (uint32_t)(seed >> 32), iter_base, index_base, goal, spheres, K, (R)obstacle_weight, wind, wind_stride, time,
                       pos, vel, att, omega, state, smoother_state, mixer_state, motor_health, health_stride, followed, U, cost, trace, plan_last,
                       clearance);
  };
  if (smooth && mix) go(std::true_type{}, std::true_type{});
  else if (smooth) go(std::true_type{}, std::false_type{});
  else go(std::false_type{}, std::true_type{});
  return launch_status("se3mpc_mppi_closed_loop_staged");
}

}  // namespace mppi
}  // namespace se3mpc

using se3mpc::mppi::mppi_closed_loop_staged_impl;

#define SE3MPC_DEFINE_MPPI_CLOSED_LOOP_STAGED(SUF, R)                                                                                        \
  extern "C" int se3mpc_mppi_closed_loop_staged_##SUF(                                                                                       \
      const se3mpc_params* p, const se3mpc_controller_params* cp, const se3mpc_simulator_params* sp, const se3mpc_smoother_params* smp,      \
      const se3mpc_mixer_params* mp, int B, int cycles, int substeps, double sim_dt, uint32_t cycle_base, int shift, int S, int iters,       \
      double sigma, double temperature, uint64_t seed, uint32_t iter_base, uint32_t index_base, const R* goal, const R* spheres, int K,      \
      double obstacle_weight, const R* wind, long long wind_stride, double* time, R* pos, R* vel, R* att, R* omega, double* state,           \
      double* smoother_state, double* mixer_state, const R* motor_health, long long health_stride, R* followed, R* U, R* cost, R* trace,     \
      R* plan_last, R* clearance, void* stream) {                                                                                            \
    return mppi_closed_loop_staged_impl<R>(p, cp, sp, smp, mp, B, cycles, substeps, sim_dt, cycle_base, shift, S, iters, sigma, temperature,  \
                                           seed, iter_base, index_base, goal, spheres, K, obstacle_weight, wind, wind_stride, time, pos, vel, \
                                           att, omega, state, smoother_state, mixer_state, motor_health, health_stride, followed, U, cost,    \
                                           trace, plan_last, clearance, stream);                                                              \
  }

SE3MPC_DEFINE_MPPI_CLOSED_LOOP_STAGED(f32, float)
SE3MPC_DEFINE_MPPI_CLOSED_LOOP_STAGED(f64, double)
