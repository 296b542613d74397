// monte_carlo_edge.hip -- the one-launch closed-loop Monte-Carlo of monte_carlo.hip on the reference's OTHER edge loop (edge/main.py:21-112):
// plan -> latency buffer -> OnboardController -> DroneSimulator, every planning cycle of every drone inside ONE kernel.  Per
// cycle exactly what ClosedLoopMonteCarlo.run_edge launches as se3mpc_solve_* + se3mpc_edge_loop_*: the same device functions (solve_body.inc;
// edge_step of edge_device.hpp), hence the same bits -- without 2 x cycles kernel boundaries at each of which every drone waits for the
// batch's slowest solve.
//
// Every piece of cross-cycle state lives in operands the caller owns -- the onboard record, the latency record, the ring, the clocks -- and the
// plan's stamps count from `first_cycle`, so a second launch continues the first (unlike monte_carlo_staged.hip, whose followed plan stays on
// the chip).
//
// Mapping, LDS image and register budget as monte_carlo.hip; behind each drone's block lie the two records and the zero-thrust counter
// (EdgeRecords; the act phase is edge_act of edge_act_device.hpp, shared with mppi_closed_loop_edge.hip).  The ring stays the HBM operand of se3mpc_edge_loop_*, indexed by the drone: the act phase's one lane loads the entry a push
// pops one step ahead (LatencyLane), as every edge-loop launch does.
#include "solve_device.hpp"
#pragma clang fp contract(off)
#include "edge_act_device.hpp"

namespace se3mpc {

// Behind each drone's DroneBlock, at mc_consts_offset: its EdgeRecords (edge_act_device.hpp)
template <typename IO>
__host__ __device__ constexpr size_t edge_group_bytes(int G) { return mc_consts_offset<IO>(G) + EdgeRecords::bytes(); }

// Group grp's block.  Built again inside each phase, as mc_block.
template <typename IO, int G>
__device__ __forceinline__ EdgeBlock<IO> edge_block(unsigned char* lds_raw, size_t solver_lds, int grp) {
  unsigned char* gb = lds_raw + solver_lds + (size_t)grp * edge_group_bytes<IO>(G);
  return edge_block_at<IO>(drone_block<IO>(gb, G, mc_plan_offset<IO>(G), mc_plan_offset<IO>(G) + (size_t)9 * G * sizeof(IO)), gb + mc_consts_offset<IO>(G));
}

}  // namespace se3mpc
#pragma clang fp contract(fast)

namespace se3mpc {

// One wavefront per SIMD, as monte_carlo_kernel and for its reason.  The controller's and the simulator's constants are kernel arguments,
// as in monte_carlo_staged_kernel: the act phase reads them as scalars (DESIGN.md 5.7g has the register counts of both placements).
template <typename IO, int G>
__global__ void __launch_bounds__(64, SE3MPC_MC_WAVES)
monte_carlo_edge_kernel(SolveDev q, OnboardDev<IO> onb, SimDev<IO> sim, int B, int cycles, int substeps, double sim_dt, int first_cycle,
                        size_t solver_lds, const IO* __restrict__ goalg, const IO* __restrict__ windg, long long wind_stride,
                        double* __restrict__ timeg, IO* __restrict__ posg, IO* __restrict__ velg, IO* __restrict__ attg, IO* __restrict__ omegag,
                        double* __restrict__ onboardg, int depth, IO* ringg, double* ring_timeg, double* __restrict__ latencyg,
                        int32_t* __restrict__ zero_thrust_steps, IO* __restrict__ Xg, IO* __restrict__ accg,
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
  if (k == 0) edge_load<IO>(edge_block<IO, G>(lds_raw, solver_lds, grp), pb, posg, velg, attg, omegag, windg, wind_stride, timeg, onboardg, depth, latencyg);
  group_sync<G>();
  const IO* x0row = nullptr;               // every cycle re-plans from the reference's cold start
  const bool cold = true;
  for (int cycle = 0; cycle < cycles; ++cycle) {
    // ---- plan: the batched solver's body on (pos, vel) as the solve kernel would read them from its [B][3] arrays
    double ps[3], vs[3];
    {
      const IO* s_vec = edge_block<IO, G>(lds_raw, solver_lds, grp).d.vec;
#pragma unroll
      for (int a = 0; a < 3; ++a) { ps[a] = (double)s_vec[a]; vs[a] = (double)s_vec[3 + a]; }
    }
    double x[J];
    {
#include "solve_body.inc"
      if (task == SE3MPC_TASK_OVERFLOW && k == 0) atomicAdd(overflowed, 1);      // the LDS image was too small for this solve: the caller falls back
      const DroneBlock<IO> drone = edge_block<IO, G>(lds_raw, solver_lds, grp).d;
      // the plan as se3mpc_solve_* stores it (rounded to the IO type) and as se3mpc_edge_loop_* reads it
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
    // ---- act: `substeps` steps of the edge loop (latency push, OnboardController, simulator step) on the group's first lane
    if (k == 0 && substeps > 0)        // (no steps: the chain's edge-loop launch is a no-op that touches no record)
      edge_act<IO>(edge_block<IO, G>(lds_raw, solver_lds, grp), onb, sim, q.N, substeps, sim_dt, LatRing<IO>{ringg, ring_timeg, depth, B, pb},
                   [](int, const IO*) {});
    group_sync<G>();
  }
  if (k == 0)
    edge_store<IO>(edge_block<IO, G>(lds_raw, solver_lds, grp), pb, posg, velg, attg, omegag, timeg, onboardg, depth, latencyg, zero_thrust_steps);
}

template <typename IO>
int monte_carlo_edge_impl(const se3mpc_params* p, const se3mpc_onboard_params* op, const se3mpc_simulator_params* sp, int B, int cycles,
                          int substeps, double sim_dt, int first_cycle, const IO* goal, const IO* wind, long long wind_stride, double* time,
                          IO* pos, IO* vel, IO* att, IO* omega, double* onboard_state, int depth, IO* ring, double* ring_time,
                          double* latency_state, int32_t* zero_thrust_steps, IO* X_last, IO* acc_last, se3mpc_solve_info* info_last,
                          int32_t* overflowed, void* stream) {
  // the rules of se3mpc_monte_carlo_*, in its order, with the edge loop's where se3mpc_edge_loop_* has them
  if (p == nullptr || op == nullptr || sp == nullptr) return reject(SE3MPC_ERR_NULL, "se3mpc_monte_carlo_edge: a parameter struct is NULL");
  int rc = check_params_impl(p);
  if (rc) return rc;
  rc = check_onboard_params(op);
  if (rc) return reject(rc, "se3mpc_monte_carlo_edge: onboard parameters");
  rc = check_simulator_params(sp);
  if (rc) return reject(rc, "se3mpc_monte_carlo_edge: simulator parameters");
  if (B < 0 || cycles < 0 || substeps < 0 || first_cycle < 0 || p->horizon > kWave)
    return reject(SE3MPC_ERR_SHAPE, "se3mpc_monte_carlo_edge: B / cycles / substeps / first_cycle < 0 or horizon > 64");
  if (depth < 0 || depth > SE3MPC_LATENCY_MAX_DEPTH) return reject(SE3MPC_ERR_SHAPE, "se3mpc_monte_carlo_edge: depth outside [0, 1000]");
  if ((long long)(first_cycle + (long long)cycles) * substeps > 2147483647LL)
    return reject(SE3MPC_ERR_SHAPE, "se3mpc_monte_carlo_edge: (first_cycle + cycles) * substeps does not fit an int");
  if (!std::isfinite(sim_dt)) return reject(SE3MPC_ERR_PARAM, "se3mpc_monte_carlo_edge: sim_dt");
  if (wind != nullptr && !(wind_stride == 0 || wind_stride >= 3)) return reject(SE3MPC_ERR_SHAPE, "se3mpc_monte_carlo_edge: wind_stride is 0 or >= 3");
  if (B == 0) return SE3MPC_OK;
  if (!time || !pos || !vel || !att || !omega || !onboard_state || !overflowed || (p->has_goal && !goal) ||
      (depth > 0 && (!ring || !ring_time || !latency_state)))
    return reject(SE3MPC_ERR_NULL, "se3mpc_monte_carlo_edge: a required operand is NULL");
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(overflowed, 0, sizeof(int32_t), s) != hipSuccess) return launch_status("se3mpc_monte_carlo_edge(memset)");
  SolveDev q = make_solve_dev(*p);
  const int G = solve_group_for_horizon(p->horizon);
  const int waves = (int)(((long)B * G + kWave - 1) / kWave);
  // the L-BFGS pairs the LDS image holds: the rule of se3mpc_monte_carlo_*, with the records' share of every drone's block in `extra`
  const size_t extra = (size_t)(kWave / G) * edge_group_bytes<IO>(G);
  const size_t per_cu = (size_t)(waves + 255) / 256;                  // wavefronts a CU must hold for the whole launch to be resident
  const size_t budget = (size_t)160 * 1024 / (per_cu < 1 ? 1 : (per_cu > 8 ? 8 : per_cu));
  int mlds = q.m;
  while (mlds > 4 && solve_lds_bytes(mlds, G, sizeof(IO)) + extra > budget) --mlds;
  q.mlds = mlds;
  const size_t solver_lds = (solve_lds_bytes(mlds, G, sizeof(IO)) + 15) / 16 * 16;
  const size_t lds = solver_lds + extra;
  const OnboardDev<IO> c = make_onboard_dev<IO>(*op);
  const SimDev<IO> m = make_sim_dev<IO>(*sp);
  dispatch_group(G, [&](auto g) {
    constexpr int GG = decltype(g)::value;
    if (lds > 64 * 1024)
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&monte_carlo_edge_kernel<IO, GG>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((monte_carlo_edge_kernel<IO, GG>), dim3(waves), dim3(kWave), lds, s, q, c, m, B, cycles, substeps, sim_dt, first_cycle,
                       solver_lds, goal, wind, wind_stride, time, pos, vel, att, omega, onboard_state, depth, ring, ring_time, latency_state,
                       zero_thrust_steps, X_last, acc_last, info_last, overflowed);
  });
  return launch_status("se3mpc_monte_carlo_edge");
}

}  // namespace se3mpc

using namespace se3mpc;

#define SE3MPC_DEFINE_MONTE_CARLO_EDGE(SUF, R)                                                                                      \
  extern "C" int se3mpc_monte_carlo_edge_##SUF(                                                                                     \
      const se3mpc_params* p, const se3mpc_onboard_params* op, const se3mpc_simulator_params* sp, int B, int cycles, int substeps,  \
      double sim_dt, int first_cycle, const R* goal, const R* wind, long long wind_stride, double* time, R* pos, R* vel, R* att,    \
      R* omega, double* onboard_state, int depth, R* ring, double* ring_time, double* latency_state, int32_t* zero_thrust_steps,    \
      R* X_last, R* acc_last, se3mpc_solve_info* info_last, int32_t* overflowed, void* stream) {                                    \
    return monte_carlo_edge_impl<R>(p, op, sp, B, cycles, substeps, sim_dt, first_cycle, goal, wind, wind_stride, time, pos, vel,   \
                                    att, omega, onboard_state, depth, ring, ring_time, latency_state, zero_thrust_steps, X_last,    \
                                    acc_last, info_last, overflowed, stream);                                                       \
  }

SE3MPC_DEFINE_MONTE_CARLO_EDGE(f32, float)
SE3MPC_DEFINE_MONTE_CARLO_EDGE(f64, double)
