// monte_carlo_mission.hip -- the one-launch closed-loop Monte-Carlo of monte_carlo.hip flying waypoint missions: at the head
// of every planning cycle the drone's goal comes from GlobalMissionPlanner.get_current_goal (mission_step of mission_device.hpp) on the drone's
// own position and clock, where monte_carlo_kernel reads one fixed goal.  Per cycle exactly what ClosedLoopMonteCarlo.run_mission launches as
// se3mpc_mission_goal_* + se3mpc_solve_* + se3mpc_closed_loop_*: the same device functions, hence the same bits.
//
// Mapping, LDS image and register budget as monte_carlo.hip.  The group's first lane runs the mission step on the LDS-resident position and
// clock and parks the goal, already rounded to the IO type as se3mpc_mission_goal_* stores it, behind the drone's block; after the group
// barrier every lane reads it.  The mission record lies there too, loaded at entry and stored at exit, and the plan's stamps count from
// `first_cycle`: a second launch continues the first.
//
// The stamps of the global planning step are ordered writes to a grid all drones share, and the phase machine never reads that grid: the
// kernel logs them as rows [cycle][drone] of the table se3mpc_ufield_stamp takes, and one call of it afterwards applies them in the chain's
// order.
#include "solve_device.hpp"
#pragma clang fp contract(off)
#include "closed_loop_device.hpp"
#include "mission_device.hpp"

namespace se3mpc {

// Behind each drone's block of monte_carlo.hip (mc_group_bytes, a multiple of 16): the mission record and the goal of the cycle [3] in the IO type
template <typename IO>
__host__ __device__ constexpr size_t mission_group_bytes(int G) { return mc_group_bytes<IO>(G) + SE3MPC_MISSION_STATE_WORDS * sizeof(double) + 32; }

template <typename IO>
struct MissionBlock {
  McBlock<IO> mc;
  double* rec;      // [SE3MPC_MISSION_STATE_WORDS]
  IO* goal;         // [3]
};
// Group grp's block.  Built again inside each phase, as mc_block.
template <typename IO, int G>
__device__ __forceinline__ MissionBlock<IO> mission_block(unsigned char* lds_raw, size_t solver_lds, int grp) {
  unsigned char* gb = lds_raw + solver_lds + (size_t)grp * mission_group_bytes<IO>(G);
  MissionBlock<IO> b;
  b.mc.d = drone_block<IO>(gb, G, mc_plan_offset<IO>(G), mc_plan_offset<IO>(G) + (size_t)9 * G * sizeof(IO));
  b.mc.ctl = reinterpret_cast<CtrlDev<IO>*>(gb + mc_consts_offset<IO>(G));
  b.mc.sim = reinterpret_cast<SimDev<IO>*>(b.mc.ctl + 1);
  b.rec = reinterpret_cast<double*>(gb + mc_group_bytes<IO>(G));
  b.goal = reinterpret_cast<IO*>(b.rec + SE3MPC_MISSION_STATE_WORDS);
  return b;
}

// The mission step of one cycle on the group's first lane: goal into the block, the stamp row into the log
template <typename IO>
__device__ __forceinline__ void mission_cycle(const se3mpc_mission_params& mp, int rv, double epoch, const MissionBlock<IO>& blk, const MissionTable& t,
                                              int pb, size_t row, double* __restrict__ centres, double* __restrict__ radius,
                                              int32_t* __restrict__ radius_voxels, double* __restrict__ factor) {
  const double p[3] = {(double)blk.mc.d.vec[0], (double)blk.mc.d.vec[1], (double)blk.mc.d.vec[2]};
  double g[3];
  MissionStamp st;
  mission_step(mp, rv, *blk.mc.d.time + epoch, p, blk.rec, mission_rows(t, pb), mission_labels(t, pb), t.W, g, st);
  for (int a = 0; a < 3; ++a) blk.goal[a] = (IO)g[a];
  if (centres != nullptr) {
    for (int a = 0; a < 3; ++a) centres[3 * row + a] = st.centre[a];
    radius[row] = st.radius;
    radius_voxels[row] = st.radius_voxels;
    factor[row] = st.factor;
  }
}

}  // namespace se3mpc
#pragma clang fp contract(fast)

namespace se3mpc {

template <typename IO, int G>
__global__ void __launch_bounds__(64, SE3MPC_MC_WAVES)
monte_carlo_mission_kernel(SolveDev q, CtrlDev<IO> ctl, SimDev<IO> sim, se3mpc_mission_params mp, int rv, double epoch, MissionTable table, int B,
                           int cycles, int substeps, double sim_dt, int first_cycle, size_t solver_lds, const IO* __restrict__ windg,
                           long long wind_stride, double* __restrict__ timeg, IO* __restrict__ posg, IO* __restrict__ velg, IO* __restrict__ attg,
                           IO* __restrict__ omegag, double* __restrict__ stateg, double* __restrict__ missiong, IO* __restrict__ goalg,
                           double* __restrict__ log_centres, double* __restrict__ log_radius, int32_t* __restrict__ log_radius_voxels,
                           double* __restrict__ log_factor, IO* __restrict__ Xg, IO* __restrict__ accg, se3mpc_solve_info* __restrict__ infog,
                           int* __restrict__ overflowed) {
  HIP_DYNAMIC_SHARED(unsigned char, lds_raw)
  constexpr int P = kWave / G, J = kSlots;
  const int lane = lane_id();
  const int k = lane & (G - 1);
  const int grp = lane / G;
  const int pb = blockIdx.x * P + grp;     // drone index
  if (pb >= B) return;                     // (a whole group leaves together)
  if (k == 0) {
    const MissionBlock<IO> blk = mission_block<IO, G>(lds_raw, solver_lds, grp);
    *blk.mc.ctl = ctl; *blk.mc.sim = sim;
    drone_load<IO>(blk.mc.d, pb, posg, velg, attg, omegag, windg, wind_stride, timeg, stateg);
    for (int i = 0; i < SE3MPC_MISSION_STATE_WORDS; ++i) blk.rec[i] = missiong[(size_t)pb * SE3MPC_MISSION_STATE_WORDS + i];
    for (int a = 0; a < 3; ++a) blk.goal[a] = goalg[3 * (size_t)pb + a];          // cycles == 0: the goal operand stays as it is
  }
  group_sync<G>();
  const IO* x0row = nullptr;               // every cycle re-plans from the reference's cold start
  const bool cold = true;
  for (int cycle = 0; cycle < cycles; ++cycle) {
    // ---- mission: get_current_goal on the drone's position and clock, on the group's first lane
    if (k == 0)
      mission_cycle<IO>(mp, rv, epoch, mission_block<IO, G>(lds_raw, solver_lds, grp), table, pb, (size_t)cycle * B + pb, log_centres, log_radius,
                        log_radius_voxels, log_factor);
    group_sync<G>();
    // ---- plan: the batched solver's body on (pos, vel, goal) as the solve kernel would read them from its [B][3] arrays
    double ps[3], vs[3], goal[3];
    {
      const MissionBlock<IO> blk = mission_block<IO, G>(lds_raw, solver_lds, grp);
      const IO* s_vec = blk.mc.d.vec;
#pragma unroll
      for (int a = 0; a < 3; ++a) { ps[a] = (double)s_vec[a]; vs[a] = (double)s_vec[3 + a]; goal[a] = (double)blk.goal[a]; }
    }
    double x[J];
    {
#include "solve_body.inc"
      if (task == SE3MPC_TASK_OVERFLOW && k == 0) atomicAdd(overflowed, 1);      // the LDS image was too small for this solve: the caller falls back
      const DroneBlock<IO> drone = mission_block<IO, G>(lds_raw, solver_lds, grp).mc.d;
      // the plan as se3mpc_solve_* stores it (rounded to the IO type) and as se3mpc_closed_loop_* reads it
      if (live) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { drone.planP[3 * k + a] = (IO)x[a]; drone.planV[3 * k + a] = (IO)x[3 + a]; }
        drone.planA[3 * k + 0] = (IO)(x[6] / q.mass); drone.planA[3 * k + 1] = (IO)(x[7] / q.mass); drone.planA[3 * k + 2] = (IO)(x[8] / q.mass - q.grav);
        drone.stamps[k] = plan_stamp(first_cycle + cycle, substeps, sim_dt, k, q.dt);
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
    // ---- act: `substeps` flight steps on the group's first lane, as monte_carlo_kernel
    if (k == 0) {
      const McBlock<IO> blk = mission_block<IO, G>(lds_raw, solver_lds, grp).mc;
      const CtrlDev<IO> c = *blk.ctl;
      const SimDev<IO> m = *blk.sim;
      fly_steps<IO>(c, m, blk.d, q.N, substeps, sim_dt, [](int, const IO*) {});
    }
    group_sync<G>();
  }
  if (k == 0) {
    const MissionBlock<IO> blk = mission_block<IO, G>(lds_raw, solver_lds, grp);
    drone_store<IO>(blk.mc.d, pb, posg, velg, attg, omegag, timeg, stateg);
    for (int i = 0; i < SE3MPC_MISSION_STATE_WORDS; ++i) missiong[(size_t)pb * SE3MPC_MISSION_STATE_WORDS + i] = blk.rec[i];
    for (int a = 0; a < 3; ++a) goalg[3 * (size_t)pb + a] = blk.goal[a];
  }
}

template <typename IO>
int monte_carlo_mission_impl(const se3mpc_params* p, const se3mpc_controller_params* cp, const se3mpc_simulator_params* sp,
                             const se3mpc_mission_params* mp, int B, int cycles, int substeps, double sim_dt, int first_cycle, double epoch,
                             const double* waypoints, long long wp_stride, const int32_t* labels, long long label_stride, int W, double resolution,
                             const IO* wind, long long wind_stride, double* time, IO* pos, IO* vel, IO* att, IO* omega, double* state,
                             double* mission_state, IO* goal, double* log_centres, double* log_radius, int32_t* log_radius_voxels,
                             double* log_factor, IO* X_last, IO* acc_last, se3mpc_solve_info* info_last, int32_t* overflowed, void* stream) {
  if (p == nullptr || cp == nullptr || sp == nullptr || mp == nullptr) return reject(SE3MPC_ERR_NULL, "se3mpc_monte_carlo_mission: a parameter struct");
  int rc = check_params_impl(p);
  if (rc) return rc;
  rc = check_controller_params(cp);
  if (rc) return reject(rc, "se3mpc_monte_carlo_mission: controller parameters");
  rc = check_simulator_params(sp);
  if (rc) return reject(rc, "se3mpc_monte_carlo_mission: simulator parameters");
  rc = check_mission_params(mp);
  if (rc) return reject(rc, "se3mpc_monte_carlo_mission: a non-finite mission parameter or a period <= 0");
  if (!p->has_goal) return reject(SE3MPC_ERR_PARAM, "se3mpc_monte_carlo_mission: the mission is the goal source, has_goal must be set");
  if (B < 0 || cycles < 0 || substeps < 0 || first_cycle < 0 || p->horizon > kWave)
    return reject(SE3MPC_ERR_SHAPE, "se3mpc_monte_carlo_mission: B / cycles / substeps / first_cycle < 0 or horizon > 64");
  if ((long long)(first_cycle + (long long)cycles) * substeps > 2147483647LL || (long long)cycles * B > (1LL << 30))
    return reject(SE3MPC_ERR_SHAPE, "se3mpc_monte_carlo_mission: (first_cycle + cycles) * substeps beyond an int, or cycles * B beyond 2^30");
  if (!std::isfinite(sim_dt) || !std::isfinite(epoch)) return reject(SE3MPC_ERR_PARAM, "se3mpc_monte_carlo_mission: sim_dt / epoch");
  if (wind != nullptr && !(wind_stride == 0 || wind_stride >= 3)) return reject(SE3MPC_ERR_SHAPE, "se3mpc_monte_carlo_mission: wind_stride");
  const MissionTable table = {waypoints, wp_stride, labels, label_stride, W};
  rc = check_mission_table(mp, table, resolution, "se3mpc_monte_carlo_mission: W < 0, a stride smaller than the table, or the resolution");
  if (rc) return rc;
  if (B == 0) return SE3MPC_OK;
  const int logs = (log_centres != nullptr) + (log_radius != nullptr) + (log_radius_voxels != nullptr) + (log_factor != nullptr);
  if (!time || !pos || !vel || !att || !omega || !state || !mission_state || !goal || !overflowed || (W > 0 && (!waypoints || !labels)) ||
      (logs != 0 && logs != 4))
    return reject(SE3MPC_ERR_NULL, "se3mpc_monte_carlo_mission: a state operand, the goal, the waypoint table, or a part of the stamp log");
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(overflowed, 0, sizeof(int32_t), s) != hipSuccess) return launch_status("se3mpc_monte_carlo_mission(memset)");
  SolveDev q = make_solve_dev(*p);
  const int G = solve_group_for_horizon(p->horizon);
  const int waves = (int)(((long)B * G + kWave - 1) / kWave);
  // the L-BFGS pairs of the LDS image: the rule of se3mpc_monte_carlo_*, on this kernel's wider group
  const size_t extra = (size_t)(kWave / G) * mission_group_bytes<IO>(G);
  const size_t per_cu = (size_t)(waves + 255) / 256;
  const size_t budget = (size_t)160 * 1024 / (per_cu < 1 ? 1 : (per_cu > 8 ? 8 : per_cu));
  int mlds = q.m;
  while (mlds > 4 && solve_lds_bytes(mlds, G, sizeof(IO)) + extra > budget) --mlds;
  q.mlds = mlds;
  const size_t solver_lds = (solve_lds_bytes(mlds, G, sizeof(IO)) + 15) / 16 * 16;
  const size_t lds = solver_lds + extra;
  const CtrlDev<IO> c = make_ctrl_dev<IO>(*cp);
  const SimDev<IO> m = make_sim_dev<IO>(*sp);
  const int rv = mission_radius_voxels(mp, resolution);
  dispatch_group(G, [&](auto g) {
    constexpr int GG = decltype(g)::value;
    if (lds > 64 * 1024)
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&monte_carlo_mission_kernel<IO, GG>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((monte_carlo_mission_kernel<IO, GG>), dim3(waves), dim3(kWave), lds, s, q, c, m, *mp, rv, epoch, table, B, cycles, substeps, sim_dt,
                       first_cycle, solver_lds, wind, wind_stride, time, pos, vel, att, omega, state, mission_state, goal, log_centres, log_radius,
                       log_radius_voxels, log_factor, X_last, acc_last, info_last, overflowed);
  });
  return launch_status("se3mpc_monte_carlo_mission");
}

}  // namespace se3mpc

using namespace se3mpc;

#define SE3MPC_MONTE_CARLO_MISSION(SUF, R)                                                                                                    \
  extern "C" int se3mpc_monte_carlo_mission_##SUF(                                                                                            \
      const se3mpc_params* p, const se3mpc_controller_params* cp, const se3mpc_simulator_params* sp, const se3mpc_mission_params* mp, int B,  \
      int cycles, int substeps, double sim_dt, int first_cycle, double epoch, const double* waypoints, long long wp_stride,                    \
      const int32_t* labels, long long label_stride, int W, double resolution, const R* wind, long long wind_stride, double* time, R* pos,    \
      R* vel, R* att, R* omega, double* state, double* mission_state, R* goal, double* log_centres, double* log_radius,                       \
      int32_t* log_radius_voxels, double* log_factor, R* X_last, R* acc_last, se3mpc_solve_info* info_last, int32_t* overflowed,              \
      void* stream) {                                                                                                                         \
    return monte_carlo_mission_impl<R>(p, cp, sp, mp, B, cycles, substeps, sim_dt, first_cycle, epoch, waypoints, wp_stride, labels,          \
                                       label_stride, W, resolution, wind, wind_stride, time, pos, vel, att, omega, state, mission_state,      \
                                       goal, log_centres, log_radius, log_radius_voxels, log_factor, X_last, acc_last, info_last, overflowed, \
                                       stream);                                                                                               \
  }
SE3MPC_MONTE_CARLO_MISSION(f32, float)
SE3MPC_MONTE_CARLO_MISSION(f64, double)
