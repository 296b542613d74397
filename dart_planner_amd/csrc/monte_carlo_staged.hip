// monte_carlo_staged.hip -- the one-launch closed-loop Monte-Carlo of monte_carlo.hip with the reference's full edge loop per drone
// (edge/main_improved.py:96-152): plan -> TrajectorySmoother -> GeometricController -> MotorMixer and motors -> DroneSimulator, every
// planning cycle of every drone inside ONE kernel.  Per cycle exactly what control/closed_loop.py launches as
// se3mpc_solve_* + se3mpc_smoother_update_* + se3mpc_closed_loop_smoothed_* / se3mpc_closed_loop_actuated_*: the same device functions
// (solve_body.inc; smoother_take_plan, smoothed_step, actuated_step), hence the same bits -- without 3 x cycles kernel boundaries at each of
// which every drone waits for the batch's slowest solve.
//
// One plan per drone is enough: update_trajectory reads the plan being followed exactly once, at (now - trajectory_start), and `now` -- the
// drone's clock at the start of the cycle -- is its clock at the end of the act phase before.  So the first lane of the group takes that one
// sample (smoother_sample_followed) at the end of an act phase, while the plan it belongs to is still in LDS, and parks its nine values;
// the next cycle's solve then overwrites the plan and smoother_take_plan gets the nine values in place of the old plan.
//
// Mapping, LDS image and register budget as monte_carlo.hip; behind each drone's block lie the records of the stages the variant has
// (StagedLayout).  Without either stage the entry point IS se3mpc_monte_carlo_*.
#include "solve_device.hpp"
#pragma clang fp contract(off)
#include "staged_device.hpp"

namespace se3mpc {

// A drone's LDS block: the DroneBlock of monte_carlo.hip (stamps, clock, controller record, plan, state and wind) and behind it, at
// mc_consts_offset, the stages' share (StagedRecords, staged_device.hpp): the smoother's and the mixer's records (doubles, as in memory), the
// four health factors and the nine parked values of the plan being followed (IO).  A stage the variant does not have costs nothing.
// All constants -- controller, simulator, smoother, mixer: 1.1 KB in float64 -- stay kernel arguments here: the act phase reads them as
// scalars.  Parked in LDS as monte_carlo.hip parks the first two they come back as VECTOR registers that stay live across the step loop,
// and the float64 variants with the smoother spilled (8 registers with the two stages' constants as arguments, 89 - 113 with none).
template <typename IO, bool SMOOTH, bool MIX>
struct StagedLayout {
  __host__ __device__ static constexpr size_t records_offset(int G) { return mc_consts_offset<IO>(G); }
  __host__ __device__ static constexpr size_t group_bytes(int G) { return records_offset(G) + StagedRecords<IO, SMOOTH, MIX>::bytes(); }
};

// Group grp's block (pointers of a stage the variant does not have are null).  Built again inside each phase, as mc_block.
template <typename IO, int G, bool SMOOTH, bool MIX>
__device__ __forceinline__ StagedBlock<IO> staged_block(unsigned char* lds_raw, size_t solver_lds, int grp) {
  using L = StagedLayout<IO, SMOOTH, MIX>;
  unsigned char* gb = lds_raw + solver_lds + (size_t)grp * L::group_bytes(G);
  return staged_block_at<IO, SMOOTH, MIX>(drone_block<IO>(gb, G, mc_plan_offset<IO>(G), mc_plan_offset<IO>(G) + (size_t)9 * G * sizeof(IO)),
                                          gb + L::records_offset(G));
}

}  // namespace se3mpc
#pragma clang fp contract(fast)

namespace se3mpc {

// One wavefront per SIMD, as monte_carlo_kernel and for its reason: at the solver's 256-register budget the constants the compiler hoists
// out of the cycle loop spill.
template <typename IO, int G, bool SMOOTH, bool MIX>
__global__ void __launch_bounds__(64, SE3MPC_MC_WAVES)
monte_carlo_staged_kernel(SolveDev q, CtrlDev<IO> ctl, SimDev<IO> sim, SmoothDev<IO> smd, MixDev<IO> mxd, int B, int cycles, int substeps,
                          double sim_dt, size_t solver_lds, const IO* __restrict__ goalg, const IO* __restrict__ windg, long long wind_stride,
                          double* __restrict__ timeg, IO* __restrict__ posg, IO* __restrict__ velg, IO* __restrict__ attg,
                          IO* __restrict__ omegag, double* __restrict__ stateg, double* __restrict__ smootherg, double* __restrict__ mixerg,
                          const IO* __restrict__ healthg, long long health_stride, IO* __restrict__ Xg, IO* __restrict__ accg,
                          se3mpc_solve_info* __restrict__ infog, int* __restrict__ overflowed) {
  HIP_DYNAMIC_SHARED(unsigned char, lds_raw)
  constexpr int P = kWave / G, J = kSlots;
  const int lane = lane_id();
  const int k = lane & (G - 1);
  const int grp = lane / G;
  const int pb = blockIdx.x * P + grp;     // drone index
  if (pb >= B) return;                     // (a whole group leaves together)
  double goal[3] = {0.0, 0.0, 0.0};
  if (q.has_goal) {
#pragma unroll
    for (int a = 0; a < 3; ++a) goal[a] = (double)goalg[pb * 3 + a];
  }
  if (k == 0) {
    const StagedBlock<IO> blk = staged_block<IO, G, SMOOTH, MIX>(lds_raw, solver_lds, grp);
    drone_load<IO>(blk.d, pb, posg, velg, attg, omegag, windg, wind_stride, timeg, stateg);
    staged_load<IO, SMOOTH, MIX>(blk, pb, smootherg, mixerg, healthg, health_stride, nullptr);
  }
  group_sync<G>();
  const IO* x0row = nullptr;               // every cycle re-plans from the reference's cold start
  const bool cold = true;
  for (int cycle = 0; cycle < cycles; ++cycle) {
    // ---- plan: the batched solver's body on (pos, vel) as the solve kernel would read them from its [B][3] arrays
    double ps[3], vs[3];
    {
      const IO* s_vec = staged_block<IO, G, SMOOTH, MIX>(lds_raw, solver_lds, grp).d.vec;
#pragma unroll
      for (int a = 0; a < 3; ++a) { ps[a] = (double)s_vec[a]; vs[a] = (double)s_vec[3 + a]; }
    }
    double x[J];
    {
#include "solve_body.inc"
      if (task == SE3MPC_TASK_OVERFLOW && k == 0) atomicAdd(overflowed, 1);      // the LDS image was too small for this solve: the caller falls back
      const DroneBlock<IO> drone = staged_block<IO, G, SMOOTH, MIX>(lds_raw, solver_lds, grp).d;
      // the plan as se3mpc_solve_* stores it (rounded to the IO type) and as the act phase's launches read it; the plan of the cycle before
      // is gone from here on -- its one sample is parked
      if (live) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { drone.planP[3 * k + a] = (IO)x[a]; drone.planV[3 * k + a] = (IO)x[3 + a]; }
        drone.planA[3 * k + 0] = (IO)(x[6] / q.mass); drone.planA[3 * k + 1] = (IO)(x[7] / q.mass); drone.planA[3 * k + 2] = (IO)(x[8] / q.mass - q.grav);
        drone.stamps[k] = plan_stamp(cycle, substeps, sim_dt, k, q.dt);
      }
      if (cycle == cycles - 1 && live) {
        if (Xg != nullptr) {
#pragma unroll
          for (int j = 0; j < J; ++j) Xg[(size_t)pb * n + (j / 3) * n3 + 3 * k + (j % 3)] = (IO)x[j];
        }
        if (accg != nullptr) {
          const size_t o = (size_t)pb * n3 + 3 * k;
          accg[o] = drone.planA[3 * k + 0]; accg[o + 1] = drone.planA[3 * k + 1]; accg[o + 2] = drone.planA[3 * k + 2];
        }
        if (infog != nullptr && k == 0) {
          se3mpc_solve_info r;
          r.fun = f; r.nit = nit; r.nfev = nfev; r.status = status; r.task = task;
          infog[pb] = r;
        }
      }
    }
    group_sync<G>();
    // ---- act on the group's first lane
    if (k == 0)
      staged_act<IO, SMOOTH, MIX>(staged_block<IO, G, SMOOTH, MIX>(lds_raw, solver_lds, grp), ctl, sim, smd, mxd, q.N, substeps, sim_dt, healthg != nullptr,
                                  cycle + 1 < cycles);
    group_sync<G>();
  }
  if (k == 0) {
    const StagedBlock<IO> blk = staged_block<IO, G, SMOOTH, MIX>(lds_raw, solver_lds, grp);
    drone_store<IO>(blk.d, pb, posg, velg, attg, omegag, timeg, stateg);
    staged_store<IO, SMOOTH, MIX>(blk, pb, smootherg, mixerg, nullptr);
  }
}

template <typename IO, int G, bool SMOOTH, bool MIX, typename... Args>
static void launch_staged(int waves, size_t lds, hipStream_t s, Args... args) {
  if (lds > 64 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&monte_carlo_staged_kernel<IO, G, SMOOTH, MIX>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL((monte_carlo_staged_kernel<IO, G, SMOOTH, MIX>), dim3(waves), dim3(kWave), lds, s, args...);
}

template <typename IO, bool SMOOTH, bool MIX>
static size_t staged_group_bytes(int G) { return StagedLayout<IO, SMOOTH, MIX>::group_bytes(G); }

// se3mpc_monte_carlo_* for IO (the form without a stage)
static int monte_carlo_plain(const se3mpc_params* p, const se3mpc_controller_params* cp, const se3mpc_simulator_params* sp, int B, int cycles,
                             int substeps, double sim_dt, const float* goal, const float* wind, long long wind_stride, double* time, float* pos,
                             float* vel, float* att, float* omega, double* state, float* X_last, float* acc_last,
                             se3mpc_solve_info* info_last, int32_t* overflowed, void* stream) {
  return se3mpc_monte_carlo_f32(p, cp, sp, B, cycles, substeps, sim_dt, goal, wind, wind_stride, time, pos, vel, att, omega, state, X_last,
                                acc_last, info_last, overflowed, stream);
}
static int monte_carlo_plain(const se3mpc_params* p, const se3mpc_controller_params* cp, const se3mpc_simulator_params* sp, int B, int cycles,
                             int substeps, double sim_dt, const double* goal, const double* wind, long long wind_stride, double* time,
                             double* pos, double* vel, double* att, double* omega, double* state, double* X_last, double* acc_last,
                             se3mpc_solve_info* info_last, int32_t* overflowed, void* stream) {
  return se3mpc_monte_carlo_f64(p, cp, sp, B, cycles, substeps, sim_dt, goal, wind, wind_stride, time, pos, vel, att, omega, state, X_last,
                                acc_last, info_last, overflowed, stream);
}

template <typename IO>
int monte_carlo_staged_impl(const se3mpc_params* p, const se3mpc_controller_params* cp, const se3mpc_simulator_params* sp,
                            const se3mpc_smoother_params* smp, const se3mpc_mixer_params* mp, int B, int cycles, int substeps, double sim_dt,
                            const IO* goal, const IO* wind, long long wind_stride, double* time, IO* pos, IO* vel, IO* att, IO* omega,
                            double* state, double* smoother_state, double* mixer_state, const IO* motor_health, long long health_stride,
                            IO* X_last, IO* acc_last, se3mpc_solve_info* info_last, int32_t* overflowed, void* stream) {
  // the rules of se3mpc_monte_carlo_*, in its order, with the stages' rules where se3mpc_closed_loop_actuated_* has them
  if (p == nullptr || cp == nullptr || sp == nullptr) return SE3MPC_ERR_NULL;
  if ((smp == nullptr) != (smoother_state == nullptr))
    return reject(SE3MPC_ERR_NULL, "se3mpc_monte_carlo_staged: smoother parameters and smoother_state come together or not at all");
  if ((mp == nullptr) != (mixer_state == nullptr))
    return reject(SE3MPC_ERR_NULL, "se3mpc_monte_carlo_staged: mixer parameters and mixer_state come together or not at all");
  if (motor_health != nullptr && mp == nullptr) return reject(SE3MPC_ERR_NULL, "se3mpc_monte_carlo_staged: motor_health needs the mixer");
  const bool smooth = smp != nullptr, mix = mp != nullptr;
  int rc = check_params_impl(p);
  if (rc) return rc;
  rc = check_controller_params(cp);
  if (rc) return rc;
  rc = check_simulator_params(sp);
  if (rc) return rc;
  rc = smooth ? check_smoother_params(smp) : SE3MPC_OK;
  if (rc) return reject(rc, "se3mpc_monte_carlo_staged: smoother parameters");
  rc = mix ? check_mixer_params(mp) : SE3MPC_OK;
  if (rc) return reject(rc, "se3mpc_monte_carlo_staged: mixer parameters");
  if (B < 0 || cycles < 0 || substeps < 0 || p->horizon > kWave) return SE3MPC_ERR_SHAPE;
  if (health_stride < 0) return reject(SE3MPC_ERR_SHAPE, "se3mpc_monte_carlo_staged: health_stride < 0");
  if (!smooth && !mix)
    return monte_carlo_plain(p, cp, sp, B, cycles, substeps, sim_dt, goal, wind, wind_stride, time, pos, vel, att, omega, state, X_last, acc_last,
                             info_last, overflowed, stream);
  if (!std::isfinite(sim_dt)) return SE3MPC_ERR_PARAM;
  if (wind != nullptr && !(wind_stride == 0 || wind_stride >= 3)) return SE3MPC_ERR_SHAPE;
  if (B == 0) return SE3MPC_OK;
  if (!time || !pos || !vel || !att || !omega || !state || !overflowed || (p->has_goal && !goal)) return SE3MPC_ERR_NULL;
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(overflowed, 0, sizeof(int32_t), s) != hipSuccess) return launch_status("se3mpc_monte_carlo_staged(memset)");
  SolveDev q = make_solve_dev(*p);
  const int G = solve_group_for_horizon(p->horizon);
  const int waves = (int)(((long)B * G + kWave - 1) / kWave);
  // the L-BFGS pairs the LDS image holds: the rule of se3mpc_monte_carlo_*, with the stages' share of every drone's block in `extra`
  const size_t group = smooth ? (mix ? staged_group_bytes<IO, true, true>(G) : staged_group_bytes<IO, true, false>(G))
                              : staged_group_bytes<IO, false, true>(G);
  const size_t extra = (size_t)(kWave / G) * group;
  const size_t per_cu = (size_t)(waves + 255) / 256;                  // wavefronts a CU must hold for the whole launch to be resident
  const size_t budget = (size_t)160 * 1024 / (per_cu < 1 ? 1 : (per_cu > 8 ? 8 : per_cu));
  int mlds = q.m;
  while (mlds > 4 && solve_lds_bytes(mlds, G, sizeof(IO)) + extra > budget) --mlds;
  q.mlds = mlds;
  const size_t solver_lds = (solve_lds_bytes(mlds, G, sizeof(IO)) + 15) / 16 * 16;
  const size_t lds = solver_lds + extra;
  const CtrlDev<IO> c = make_ctrl_dev<IO>(*cp);
  const SimDev<IO> m = make_sim_dev<IO>(*sp);
  se3mpc_smoother_params no_smoother;
  se3mpc_smoother_default_params(&no_smoother);                                   // a variant without the stage never reads its constants
  const SmoothDev<IO> sd = make_smooth_dev<IO>(smooth ? *smp : no_smoother);
  const MixDev<IO> xd = mix ? make_mix_dev<IO>(*mp) : MixDev<IO>{};
  dispatch_group(G, [&](auto g) {
    constexpr int GG = decltype(g)::value;
    auto go = [&](auto with_smoother, auto with_mixer) {
      launch_staged<IO, GG, decltype(with_smoother)::value, decltype(with_mixer)::value>(
          waves, lds, s, q, c, m, sd, xd, B, cycles, substeps, sim_dt, solver_lds, goal, wind, wind_stride, time, pos, vel, att, omega, state,
          smoother_state, mixer_state, motor_health, health_stride, X_last, acc_last, info_last, overflowed);
    };
    if (smooth && mix) go(std::true_type{}, std::true_type{});
    else if (smooth) go(std::true_type{}, std::false_type{});
    else go(std::false_type{}, std::true_type{});
  });
  return launch_status("se3mpc_monte_carlo_staged");
}

}  // namespace se3mpc

using namespace se3mpc;

#define SE3MPC_DEFINE_MONTE_CARLO_STAGED(SUF, R)                                                                                    \
  extern "C" int se3mpc_monte_carlo_staged_##SUF(                                                                                   \
      const se3mpc_params* p, const se3mpc_controller_params* cp, const se3mpc_simulator_params* sp, const se3mpc_smoother_params* smp, \
      const se3mpc_mixer_params* mp, int B, int cycles, int substeps, double sim_dt, const R* goal, const R* wind, long long wind_stride, \
      double* time, R* pos, R* vel, R* att, R* omega, double* state, double* smoother_state, double* mixer_state, const R* motor_health, \
      long long health_stride, R* X_last, R* acc_last, se3mpc_solve_info* info_last, int32_t* overflowed, void* stream) {           \
    return monte_carlo_staged_impl<R>(p, cp, sp, smp, mp, B, cycles, substeps, sim_dt, goal, wind, wind_stride, time, pos, vel, att, omega, \
                                      state, smoother_state, mixer_state, motor_health, health_stride, X_last, acc_last, info_last,  \
                                      overflowed, stream);                                                                          \
  }

SE3MPC_DEFINE_MONTE_CARLO_STAGED(f32, float)
SE3MPC_DEFINE_MONTE_CARLO_STAGED(f64, double)
