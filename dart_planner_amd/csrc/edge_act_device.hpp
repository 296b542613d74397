// edge_act_device.hpp -- the act phase of the one-launch Monte-Carlo kernels that fly the reference's edge loop (latency buffer ->
// OnboardController -> simulator; edge_device.hpp): monte_carlo_edge.hip and mppi_closed_loop_edge.hip (5.8e).  What a drone
// keeps in LDS beside its DroneBlock (EdgeRecords, EdgeBlock), the drone into its block and back (edge_load, edge_store), and the steps of one
// cycle by one lane (edge_act) -- one definition, hence the same bits in both kernels as in se3mpc_edge_loop_*.
// INCLUDE UNDER `#pragma clang fp contract(off)`, as edge_device.hpp.
#pragma once
#include "edge_device.hpp"

namespace se3mpc {

// What a kernel keeps per drone beside its DroneBlock: the onboard record and the latency record (doubles, as in memory) and the steps whose
// commanded thrust was exactly 0.  DroneBlock::ctrl (the geometric controller's 12 words) is not used by these kernels: the onboard record
// has 14.
struct EdgeRecords {
  __host__ __device__ static constexpr size_t counter_offset() { return (size_t)(SE3MPC_ONBOARD_STATE_WORDS + SE3MPC_LATENCY_STATE_WORDS) * sizeof(double); }
  __host__ __device__ static constexpr size_t bytes() { return (counter_offset() + sizeof(int) + 15) / 16 * 16; }
};

template <typename IO>
struct EdgeBlock {
  DroneBlock<IO> d;
  double *orec, *lrec;     // onboard record [SE3MPC_ONBOARD_STATE_WORDS], latency record [SE3MPC_LATENCY_STATE_WORDS]
  int* zeros;
};
// The block of the drone whose DroneBlock is d and whose EdgeRecords lie at `records` (8-byte aligned)
template <typename IO>
__device__ __forceinline__ EdgeBlock<IO> edge_block_at(const DroneBlock<IO>& d, unsigned char* records) {
  EdgeBlock<IO> b;
  b.d = d;
  b.orec = reinterpret_cast<double*>(records);
  b.lrec = b.orec + SE3MPC_ONBOARD_STATE_WORDS;
  b.zeros = reinterpret_cast<int*>(records + EdgeRecords::counter_offset());
  return b;
}

// Drone pb's state, wind, clock and records into its block (latencyg is read only with a buffer) ...
template <typename IO>
__device__ __forceinline__ void edge_load(const EdgeBlock<IO>& b, int pb, const IO* __restrict__ posg, const IO* __restrict__ velg,
                                          const IO* __restrict__ attg, const IO* __restrict__ omegag, const IO* __restrict__ windg,
                                          long long wind_stride, const double* __restrict__ timeg, const double* __restrict__ onboardg, int depth,
                                          const double* __restrict__ latencyg) {
  DroneRegs<IO> r;
  r.load(pb, posg, velg, attg, omegag, windg, wind_stride, timeg);
  r.store(b.d);
  for (int i = 0; i < 3; ++i) b.d.vec[12 + i] = r.wd[i];
  for (int i = 0; i < SE3MPC_ONBOARD_STATE_WORDS; ++i) b.orec[i] = onboardg[(size_t)pb * SE3MPC_ONBOARD_STATE_WORDS + i];
  for (int i = 0; i < SE3MPC_LATENCY_STATE_WORDS; ++i) b.lrec[i] = depth > 0 ? latencyg[(size_t)pb * SE3MPC_LATENCY_STATE_WORDS + i] : 0.0;
  *b.zeros = 0;
}
// ... and back; the counter is added to the caller's
template <typename IO>
__device__ __forceinline__ void edge_store(const EdgeBlock<IO>& b, int pb, IO* __restrict__ posg, IO* __restrict__ velg, IO* __restrict__ attg,
                                           IO* __restrict__ omegag, double* __restrict__ timeg, double* __restrict__ onboardg, int depth,
                                           double* __restrict__ latencyg, int32_t* __restrict__ zero_thrust_steps) {
  DroneRegs<IO> r;
  r.load(b.d);
  r.store(pb, posg, velg, attg, omegag, timeg);
  for (int i = 0; i < SE3MPC_ONBOARD_STATE_WORDS; ++i) onboardg[(size_t)pb * SE3MPC_ONBOARD_STATE_WORDS + i] = b.orec[i];
  if (depth > 0)
    for (int i = 0; i < SE3MPC_LATENCY_STATE_WORDS; ++i) latencyg[(size_t)pb * SE3MPC_LATENCY_STATE_WORDS + i] = b.lrec[i];
  if (zero_thrust_steps != nullptr) zero_thrust_steps[pb] += *b.zeros;
}

// `n` steps of the act phase of the drone in block b, by ONE lane, against the N-row plan the planner has handed over: what one
// se3mpc_edge_loop_* launch of `n` steps does to the drone -- the records from the block into registers, the cursor reset, the buffer's
// begin, the steps (each but the last with the next entry loaded ahead), the buffer's end (depth 1: the previous state reaches the ring), and
// back.  after_step(step, pos) is called behind every simulator step, as fly_steps' hook.  c and m by value, as fly_steps.
// Two calls of n1 and n2 steps leave what one call of n1 + n2 leaves, bit for bit: the records round-trip through the block exactly (the
// onboard record's R values through double, the latency record's integers through double), begin() loads back the entry end() or an earlier
// push stored, and the cursor is a search hint that a fresh search reproduces.
template <typename IO, typename F>
__device__ __forceinline__ void edge_act(const EdgeBlock<IO>& b, const OnboardDev<IO> c, const SimDev<IO> m, int N, int n, double sim_dt,
                                         const LatRing<IO>& ring, F&& after_step) {
  const DroneBlock<IO>& d = b.d;
  OnboardRegs<IO> s = load_onboard<IO>(b.orec);
  DroneRegs<IO> r;
  r.load(d);
  const IO dt = (IO)sim_dt;
  PlanCursor<IO> cur;
  cursor_reset(cur);
  const int depth = ring.depth;
  LatencyLane<IO> lat;
  lat.ring = ring;
  if (depth > 0) lat.begin(b.lrec);
  int zeros = 0;
  for (int step = 0; step < n; ++step) {
    IO th, tq[3];
    edge_step<IO>(c, m, s, cur, lat, depth, step + 1 < n, N, d.stamps, d.planP, d.planV, d.planA, r, dt, sim_dt, zeros, th, tq,
                  [](const IO*, double) {});
    after_step(step, r.p);
  }
  r.store(d);
  store_onboard<IO>(b.orec, s);
  if (depth > 0) lat.end(b.lrec);
  *b.zeros += zeros;
}

}  // namespace se3mpc
