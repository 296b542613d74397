// mppi_closed_loop_edge.hip -- the one-launch closed-loop MPPI Monte-Carlo of mppi_closed_loop.hip on the reference's OTHER edge loop
// (edge/main.py:21-112): plan -> latency buffer -> OnboardController -> DroneSimulator, every planning cycle of every drone inside ONE kernel
// (DESIGN.md 5.8e).  One workgroup of min(S, 256) lanes per drone; cycle c (C = cycle_base + c) of drone b (q = index_base + b):
//   plan       the iterations of mppi_closed_loop_kernel, unchanged (weighted_pass and nominal_update of mppi_device.hpp), g = iter_base + C * iters + i
//   hand over  hand_over_plan of mppi_loop_device.hpp: the nominal's trajectory into LDS, stamped plan_stamp(C, substeps, sim_dt, k, dt)
//   act        `substeps` x edge_step (latency push -> onboard_step -> the zero-thrust count -> simulator_step) on the workgroup's first lane:
//              edge_act of edge_act_device.hpp, the act phase of monte_carlo_edge_kernel, around the step edge_loop_kernel itself calls -- hence
//              the bits of ClosedLoopMonteCarlo.run_mppi_edge (se3mpc_mppi_closed_loop_* with no steps + se3mpc_edge_loop_* per cycle)
//   clearance  the positions the simulator produced are parked in LDS and the whole workgroup reduces min_j(|pos - c_j| - r_j) over them
//   warm start U[k] <- U[k + shift], hover behind
// Every piece of cross-cycle state lives in operands the caller owns -- U, the onboard record, the latency record, the ring, the clocks, the
// zero-thrust counters, the clearance -- so a second launch continues the first.  The ring stays the HBM operand of se3mpc_edge_loop_*,
// [depth][12][B] / [depth][B], indexed by the drone.  No atomics, no workspace, no allocation, no synchronise.
#pragma clang fp contract(off)
#include "edge_act_device.hpp"
#pragma clang fp contract(fast)
#include "mppi_device.hpp"
#include "mppi_loop_device.hpp"

namespace se3mpc {
namespace mppi {

// Wavefronts per SIMD the kernel is compiled for, chosen from the ISA (DESIGN.md 5.8e has the counts at the rejected bounds): the highest at
// which the kernel spills nothing and uses no scratch.  The act phase holds the OnboardController, the plan cursor and the latency lane's
// prefetched entry in one lane's registers.
template <typename R>
struct EdgeLoopWaves { static constexpr int value = 3; };
template <>
struct EdgeLoopWaves<double> { static constexpr int value = 2; };

// LDS: the image of loop_lds_layout (its 12 controller words stay unused: the layout is shared with mppi_closed_loop_kernel) with the
// drone's EdgeRecords behind it
__host__ __device__ inline size_t edge_loop_lds_bytes(int N, int K, int W, size_t esz) { return loop_lds_layout(N, K, W, esz).total + EdgeRecords::bytes(); }

template <typename R>
__global__ void __launch_bounds__(kBlock, EdgeLoopWaves<R>::value)
mppi_closed_loop_edge_kernel(DevParams<R> q, OnboardDev<R> onb, SimDev<R> sim, double plan_dt, int B, int cycles, int substeps, double sim_dt,
                             uint32_t cycle_base, int shift, int S, int iters, R sigma, double inv_lam, uint32_t key0, uint32_t key1,
                             uint32_t iter_base, uint32_t index_base, const R* __restrict__ goalg, const R* __restrict__ spheres, int K, R w_obs,
                             const R* __restrict__ windg, long long wind_stride, double* __restrict__ timeg, R* __restrict__ posg,
                             R* __restrict__ velg, R* __restrict__ attg, R* __restrict__ omegag, double* __restrict__ onboardg, int depth, R* ringg,
                             double* ring_timeg, double* __restrict__ latencyg, int32_t* __restrict__ zero_thrust_steps, R* __restrict__ Ug,
                             R* __restrict__ cost_out, R* __restrict__ trace, R* __restrict__ plan_last, R* __restrict__ clearance) {
  HIP_DYNAMIC_SHARED(unsigned char, lds_raw)
  const int N = q.N, rows = 3 * N, NT = (int)blockDim.x, W = NT / kWave;
  const int tid = (int)threadIdx.x, wave = tid / kWave;
  const int b = (int)blockIdx.x;
  const LoopLds X = loop_lds_layout(N, K, W, sizeof(R));
  const LdsView<R> l = lds_view<R>(lds_raw, lds_layout(N, K, W, sizeof(R)));
  R* U = l.U;
  R* sph = l.sph;
  const EdgeBlock<R> eb = edge_block_at<R>(drone_block<R>(lds_raw + X.stamps, N, X.plan - X.stamps, X.vec - X.stamps), lds_raw + X.total);
  const DroneBlock<R>& d = eb.d;
  R* s_vec = d.vec;                                         // pos, vel, att, omega, wind | goal, running clearance
  R* rad = reinterpret_cast<R*>(lds_raw + X.rad);
  R* park = reinterpret_cast<R*>(lds_raw + X.park);
  const bool want_clear = clearance != nullptr && K > 0;

  for (int r = tid; r < rows; r += NT) U[r] = Ug[(size_t)b * rows + r];
  stage_spheres(q, spheres, K, sph);
  for (int j = tid; j < K; j += NT) rad[j] = spheres[4 * j + 3];
  if (tid == 0) {
    edge_load<R>(eb, b, posg, velg, attg, omegag, windg, wind_stride, timeg, onboardg, depth, latencyg);
    for (int i = 0; i < 3; ++i) s_vec[15 + i] = q.has_goal ? goalg[3 * b + i] : (R)0;
    s_vec[18] = want_clear ? clearance[b] : (R)0;
  }
  __syncthreads();
  // the planner's context as mppi_kernel builds it (load_ctx), from the LDS copies of the state and the goal
  Ctx<R> c = load_ctx(q, 1, 0, key0, key1, index_base + (uint32_t)b, s_vec, s_vec + 3, s_vec + 15, U, sph, K, w_obs);
  // (members of c are named one by one, as in mppi_closed_loop_kernel and for its reason: a loop over them would change the cost's rounding)
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
    // ---- hand over: the nominal's trajectory, row k = the state before step k
    if (tid == 0) {
      R p[3] = {c.p0[0], c.p0[1], c.p0[2]}, v[3] = {c.v0[0], c.v0[1], c.v0[2]};
      hand_over_plan(q, p, v, U, d, N, (int)C, substeps, sim_dt, plan_dt);
    }
    // ---- act, in chunks of kPark steps: the first lane flies the edge loop, then the workgroup measures the clearance of the positions it
    // left.  The lane's registers (onboard record, cursor, latency lane) are closed into the block at the end of a chunk and opened again by
    // the next: edge_act has the argument why that gives the bits of one run of `substeps` steps.  No steps: no act phase -- the chain's
    // edge-loop launch is then a no-op that touches no record.
    int s0 = 0;
    do {
      const int n = substeps - s0 < kPark ? substeps - s0 : kPark;
      if (tid == 0 && n > 0)
        edge_act<R>(eb, onb, sim, N, n, sim_dt, LatRing<R>{ringg, ring_timeg, depth, B, b}, [&](int step, const R* p) {
          if (want_clear) { park[3 * step] = p[0]; park[3 * step + 1] = p[1]; park[3 * step + 2] = p[2]; }
        });
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
    edge_store<R>(eb, b, posg, velg, attg, omegag, timeg, onboardg, depth, latencyg, zero_thrust_steps);
    if (want_clear) clearance[b] = s_vec[18];
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
template <typename R>
static int mppi_closed_loop_edge_impl(const se3mpc_params* p, const se3mpc_onboard_params* op, const se3mpc_simulator_params* sp, int B, int cycles,
                                      int substeps, double sim_dt, uint32_t cycle_base, int shift, int S, int iters, double sigma, double temperature,
                                      uint64_t seed, uint32_t iter_base, uint32_t index_base, const R* goal, const R* spheres, int K,
                                      double obstacle_weight, const R* wind, long long wind_stride, double* time, R* pos, R* vel, R* att, R* omega,
                                      double* onboard_state, int depth, R* ring, double* ring_time, double* latency_state,
                                      int32_t* zero_thrust_steps, R* U, R* cost, R* trace, R* plan_last, R* clearance, void* stream) {
  // the rules of se3mpc_mppi_closed_loop_*, in its order, with the edge loop's where se3mpc_monte_carlo_edge_* has them
  if (p == nullptr || op == nullptr || sp == nullptr) return fail(SE3MPC_ERR_NULL, "se3mpc_mppi_closed_loop_edge: NULL parameter struct");
  int rc = check_params_impl(p);
  if (rc) return fail(rc, "se3mpc_mppi_closed_loop_edge: invalid se3mpc_params");
  rc = check_onboard_params(op);
  if (rc) return fail(rc, "se3mpc_mppi_closed_loop_edge: invalid se3mpc_onboard_params");
  rc = check_simulator_params(sp);
  if (rc) return fail(rc, "se3mpc_mppi_closed_loop_edge: invalid se3mpc_simulator_params");
  if (cycles < 0 || substeps < 0) return fail(SE3MPC_ERR_SHAPE, "se3mpc_mppi_closed_loop_edge: cycles or substeps < 0");
  if (shift < 0 || shift > p->horizon) return fail(SE3MPC_ERR_SHAPE, "se3mpc_mppi_closed_loop_edge: shift outside [0, horizon]");
  if (depth < 0 || depth > SE3MPC_LATENCY_MAX_DEPTH) return fail(SE3MPC_ERR_SHAPE, "se3mpc_mppi_closed_loop_edge: depth outside [0, 1000]");
  if (substeps > 0 && (long long)cycle_base + cycles > 2147483647LL / substeps)
    return fail(SE3MPC_ERR_SHAPE, "se3mpc_mppi_closed_loop_edge: (cycle_base + cycles) * substeps does not fit an int");
  if (wind != nullptr && !(wind_stride == 0 || wind_stride >= 3)) return fail(SE3MPC_ERR_SHAPE, "se3mpc_mppi_closed_loop_edge: wind_stride must be 0 or >= 3");
  rc = check_mppi_args("se3mpc_mppi_closed_loop_edge", p, B, B, S, iters, sigma, temperature, K, obstacle_weight);
  if (rc) return rc;
  if (!std::isfinite(sim_dt)) return fail(SE3MPC_ERR_PARAM, "se3mpc_mppi_closed_loop_edge: sim_dt must be finite");
  if (B == 0 || cycles == 0) return SE3MPC_OK;
  if (!time || !pos || !vel || !att || !omega || !onboard_state || !U || !cost || (p->has_goal && !goal) || (K > 0 && !spheres) ||
      (depth > 0 && (!ring || !ring_time || !latency_state)))
    return fail(SE3MPC_ERR_NULL, "se3mpc_mppi_closed_loop_edge: NULL operand");
  const int NT = S < kBlock ? S : kBlock;
  const size_t lds = edge_loop_lds_bytes(p->horizon, K, NT / kWave, sizeof(R));
  hipLaunchKernelGGL(mppi_closed_loop_edge_kernel<R>, dim3(B), dim3(NT), lds, (hipStream_t)stream, make_dev_params<R>(*p), make_onboard_dev<R>(*op),
                     make_sim_dev<R>(*sp), p->dt, B, cycles, substeps, sim_dt, cycle_base, shift, S, iters, (R)sigma, 1.0 / temperature, (uint32_t)seed,
                     (uint32_t)(seed >> 32), iter_base, index_base, goal, spheres, K, (R)obstacle_weight, wind, wind_stride, time, pos, vel, att,
                     omega, onboard_state, depth, ring, ring_time, latency_state, zero_thrust_steps, U, cost, trace, plan_last, clearance);
  return launch_status("se3mpc_mppi_closed_loop_edge");
}

}  // namespace mppi
}  // namespace se3mpc

using se3mpc::mppi::mppi_closed_loop_edge_impl;

#define SE3MPC_DEFINE_MPPI_CLOSED_LOOP_EDGE(SUF, R)                                                                                   \
  extern "C" int se3mpc_mppi_closed_loop_edge_##SUF(                                                                                  \
      const se3mpc_params* p, const se3mpc_onboard_params* op, const se3mpc_simulator_params* sp, int B, int cycles, int substeps,    \
      double sim_dt, uint32_t cycle_base, int shift, int S, int iters, double sigma, double temperature, uint64_t seed,               \
      uint32_t iter_base, uint32_t index_base, const R* goal, const R* spheres, int K, double obstacle_weight, const R* wind,         \
      long long wind_stride, double* time, R* pos, R* vel, R* att, R* omega, double* onboard_state, int depth, R* ring,               \
      double* ring_time, double* latency_state, int32_t* zero_thrust_steps, R* U, R* cost, R* trace, R* plan_last, R* clearance,      \
      void* stream) {                                                                                                                 \
    return mppi_closed_loop_edge_impl<R>(p, op, sp, B, cycles, substeps, sim_dt, cycle_base, shift, S, iters, sigma, temperature,     \
                                         seed, iter_base, index_base, goal, spheres, K, obstacle_weight, wind, wind_stride, time,     \
                                         pos, vel, att, omega, onboard_state, depth, ring, ring_time, latency_state,                  \
                                         zero_thrust_steps, U, cost, trace, plan_last, clearance, stream);                            \
  }

SE3MPC_DEFINE_MPPI_CLOSED_LOOP_EDGE(f32, float)
SE3MPC_DEFINE_MPPI_CLOSED_LOOP_EDGE(f64, double)
