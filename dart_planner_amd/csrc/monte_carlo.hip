// monte_carlo.hip -- the receding-horizon closed-loop Monte-Carlo of BASELINE config 5's named test shape
// (/root/reference/tests/test_monte_carlo_sim.py:24-72: `cycles` planning cycles of `substeps` control + simulator steps per drone) in
// ONE launch: every planning cycle of every drone runs inside the same kernel -- solve (solve_body.inc, the batched solver's own
// code: same bits as se3mpc_solve_*), plan handed to the controller through LDS, `substeps` x (plan sample -> geometric controller ->
// simulator step) (fly_steps of closed_loop_device.hpp, around the closed-loop kernel's own flight_step: same bits as
// se3mpc_closed_loop_*), next cycle.
//
// Why: driven as 2 x cycles launches (se3mpc_solve_* + se3mpc_closed_loop_* per cycle, control/closed_loop.py) every cycle waits at two
// kernel boundaries for its SLOWEST drone.  In the loop's own statistics 99.4 % of the solves stop after one L-BFGS-B iteration and a
// handful per cycle take three -- three times as long -- so each solve launch lasted ~30 us for ~11 us of typical work, 33 times in a
// row.  Drones are independent: here a wavefront's drones run their cycles back to back and only pay for their own slow solves.
//
// Mapping: the solver's (solve_device.hpp): G lanes per drone, lane k = horizon step k, 64 / G drones per wavefront.  The controller /
// simulator recurrence of a drone is strictly sequential scalar code: it runs on the group's first lane (the others wait at the
// group barrier), its 50 bytes of state parked in LDS while the solver has the registers.
#include "solve_device.hpp"
#pragma clang fp contract(off)
#include "closed_loop_device.hpp"
#pragma clang fp contract(fast)

namespace se3mpc {

// One wavefront per SIMD (SE3MPC_MC_WAVES, closed_loop_device.hpp)
template <typename IO, int G>
__global__ void __launch_bounds__(64, SE3MPC_MC_WAVES)
monte_carlo_kernel(SolveDev q, CtrlDev<IO> ctl, SimDev<IO> sim, int B, int cycles, int substeps, double sim_dt, size_t solver_lds,
                   const IO* __restrict__ goalg, const IO* __restrict__ windg, long long wind_stride, double* __restrict__ timeg,
                   IO* __restrict__ posg, IO* __restrict__ velg, IO* __restrict__ attg, IO* __restrict__ omegag,
                   double* __restrict__ stateg, IO* __restrict__ Xg, IO* __restrict__ accg, se3mpc_solve_info* __restrict__ infog,
                   int* __restrict__ overflowed) {
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
    const McBlock<IO> blk = mc_block<IO, G>(lds_raw, solver_lds, grp);
    *blk.ctl = ctl; *blk.sim = sim;
    drone_load<IO>(blk.d, pb, posg, velg, attg, omegag, windg, wind_stride, timeg, stateg);
  }
  group_sync<G>();
  const IO* x0row = nullptr;               // every cycle re-plans from the reference's cold start
  const bool cold = true;
  for (int cycle = 0; cycle < cycles; ++cycle) {
    // ---- plan: the batched solver's body on (pos, vel) as the solve kernel would read them from its [B][3] arrays
    double ps[3], vs[3];
    {
      const IO* s_vec = mc_block<IO, G>(lds_raw, solver_lds, grp).d.vec;
#pragma unroll
      for (int a = 0; a < 3; ++a) { ps[a] = (double)s_vec[a]; vs[a] = (double)s_vec[3 + a]; }
    }
    double x[J];
    {
#include "solve_body.inc"
      if (task == SE3MPC_TASK_OVERFLOW && k == 0) atomicAdd(overflowed, 1);      // the LDS image was too small for this solve: the caller falls back
      const DroneBlock<IO> drone = mc_block<IO, G>(lds_raw, solver_lds, grp).d;
      // the plan as se3mpc_solve_* stores it (rounded to the IO type) and as se3mpc_closed_loop_* reads it
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
    // ---- act: `substeps` flight steps (closed_loop_device.hpp: sample the plan, geometric controller, simulator step) on the group's first lane
    if (k == 0) {
      const McBlock<IO> blk = mc_block<IO, G>(lds_raw, solver_lds, grp);
      const CtrlDev<IO> c = *blk.ctl;
      const SimDev<IO> m = *blk.sim;
      fly_steps<IO>(c, m, blk.d, q.N, substeps, sim_dt, [](int, const IO*) {});
    }
    group_sync<G>();
  }
  if (k == 0) drone_store<IO>(mc_block<IO, G>(lds_raw, solver_lds, grp).d, pb, posg, velg, attg, omegag, timeg, stateg);
}

template <typename IO>
int monte_carlo_impl(const se3mpc_params* p, const se3mpc_controller_params* cp, const se3mpc_simulator_params* sp, int B, int cycles,
                     int substeps, double sim_dt, const IO* goal, const IO* wind, long long wind_stride, double* time, IO* pos, IO* vel,
                     IO* att, IO* omega, double* state, IO* X_last, IO* acc_last, se3mpc_solve_info* info_last, int32_t* overflowed,
                     void* stream) {
  if (p == nullptr || cp == nullptr || sp == nullptr) return SE3MPC_ERR_NULL;
  int rc = check_params_impl(p);
  if (rc) return rc;
  rc = check_controller_params(cp);
  if (rc) return rc;
  rc = check_simulator_params(sp);
  if (rc) return rc;
  if (B < 0 || cycles < 0 || substeps < 0 || p->horizon > kWave) return SE3MPC_ERR_SHAPE;
  if (!std::isfinite(sim_dt)) return SE3MPC_ERR_PARAM;
  if (wind != nullptr && !(wind_stride == 0 || wind_stride >= 3)) return SE3MPC_ERR_SHAPE;
  if (B == 0) return SE3MPC_OK;
  if (!time || !pos || !vel || !att || !omega || !state || !overflowed || (p->has_goal && !goal)) return SE3MPC_ERR_NULL;
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(overflowed, 0, sizeof(int32_t), s) != hipSuccess) return launch_status("se3mpc_monte_carlo(memset)");
  SolveDev q = make_solve_dev(*p);
  const int G = solve_group_for_horizon(p->horizon);
  const int waves = (int)(((long)B * G + kWave - 1) / kWave);
  // pairs of L-BFGS memory the LDS image holds: as many (<= maxcor) as still let every wavefront of the launch be resident at once,
  // at least 4 -- a solve with the reference's options stores at most two; a solve that needs more raises `overflowed`
  const size_t extra = (size_t)(kWave / G) * mc_group_bytes<IO>(G);
  const size_t per_cu = (size_t)(waves + 255) / 256;                  // wavefronts a CU must hold for the whole launch to be resident
  const size_t budget = (size_t)160 * 1024 / (per_cu < 1 ? 1 : (per_cu > 8 ? 8 : per_cu));
  int mlds = q.m;
  while (mlds > 4 && solve_lds_bytes(mlds, G, sizeof(IO)) + extra > budget) --mlds;
  q.mlds = mlds;
  const size_t solver_lds = (solve_lds_bytes(mlds, G, sizeof(IO)) + 15) / 16 * 16;
  const size_t lds = solver_lds + extra;
  const CtrlDev<IO> c = make_ctrl_dev<IO>(*cp);
  const SimDev<IO> m = make_sim_dev<IO>(*sp);
  dispatch_group(G, [&](auto g) {
    constexpr int GG = decltype(g)::value;
    if (lds > 64 * 1024)
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&monte_carlo_kernel<IO, GG>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((monte_carlo_kernel<IO, GG>), dim3(waves), dim3(kWave), lds, s, q, c, m, B, cycles, substeps, sim_dt, solver_lds, goal,
                       wind, wind_stride, time, pos, vel, att, omega, state, X_last, acc_last, info_last, overflowed);
  });
  return launch_status("se3mpc_monte_carlo");
}

}  // namespace se3mpc

using namespace se3mpc;

extern "C" int se3mpc_monte_carlo_f32(const se3mpc_params* p, const se3mpc_controller_params* cp, const se3mpc_simulator_params* sp, int B,
                                      int cycles, int substeps, double sim_dt, const float* goal, const float* wind, long long wind_stride,
                                      double* time, float* pos, float* vel, float* att, float* omega, double* state, float* X_last,
                                      float* acc_last, se3mpc_solve_info* info_last, int32_t* overflowed, void* stream) {
  return monte_carlo_impl<float>(p, cp, sp, B, cycles, substeps, sim_dt, goal, wind, wind_stride, time, pos, vel, att, omega, state, X_last,
                                 acc_last, info_last, overflowed, stream);
}
extern "C" int se3mpc_monte_carlo_f64(const se3mpc_params* p, const se3mpc_controller_params* cp, const se3mpc_simulator_params* sp, int B,
                                      int cycles, int substeps, double sim_dt, const double* goal, const double* wind, long long wind_stride,
                                      double* time, double* pos, double* vel, double* att, double* omega, double* state, double* X_last,
                                      double* acc_last, se3mpc_solve_info* info_last, int32_t* overflowed, void* stream) {
  return monte_carlo_impl<double>(p, cp, sp, B, cycles, substeps, sim_dt, goal, wind, wind_stride, time, pos, vel, att, omega, state, X_last,
                                  acc_last, info_last, overflowed, stream);
}
