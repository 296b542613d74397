// staged_device.hpp -- what the one-launch closed loops with the reference's full edge loop per drone share (monte_carlo_staged.hip, whose
// planner is the batched solver, and mppi_closed_loop_staged.hip, whose planner is MPPI): the stages' share of a
// drone's LDS block, its load and store, and the act phase of one lane -- update_trajectory's second part against the nine parked values of
// the plan being followed, the steps of se3mpc_closed_loop_actuated_* / _smoothed_*, the sample of this plan for the next update_trajectory.
// One definition, hence the same bits in both kernels and in the chain of launches they fuse.
// INCLUDE UNDER `#pragma clang fp contract(off)`, as the headers it is built from.
#pragma once
#include "mixer_device.hpp"

namespace se3mpc {

// What a variant keeps per drone behind its DroneBlock: the smoother's and the mixer's records (doubles, as in memory), then the four health
// factors and the nine parked values of the plan being followed (IO).  A stage the variant does not have costs nothing.
template <typename IO, bool SMOOTH, bool MIX>
struct StagedRecords {
  static constexpr size_t kRecordDoubles = (SMOOTH ? SE3MPC_SMOOTHER_STATE_WORDS : 0) + (MIX ? SE3MPC_MIXER_STATE_WORDS : 0);
  static constexpr size_t kValues = (MIX ? 4 : 0) + (SMOOTH ? 9 : 0);
  __host__ __device__ static constexpr size_t values_offset() { return kRecordDoubles * sizeof(double); }
  __host__ __device__ static constexpr size_t bytes() { return (values_offset() + kValues * sizeof(IO) + 15) / 16 * 16; }
};

template <typename IO>
struct StagedBlock {
  DroneBlock<IO> d;
  double *srec, *mrec;     // smoother record [SE3MPC_SMOOTHER_STATE_WORDS], mixer record [SE3MPC_MIXER_STATE_WORDS]
  IO *health, *parked;     // [4], [9]
};
// The block of the drone whose DroneBlock is d and whose stage records start at `records` (8-byte aligned; pointers of a stage the variant
// does not have are null)
template <typename IO, bool SMOOTH, bool MIX>
__device__ __forceinline__ StagedBlock<IO> staged_block_at(const DroneBlock<IO>& d, unsigned char* records) {
  StagedBlock<IO> b;
  b.d = d;
  double* rec = reinterpret_cast<double*>(records);
  b.srec = SMOOTH ? rec : nullptr;
  b.mrec = MIX ? rec + (SMOOTH ? SE3MPC_SMOOTHER_STATE_WORDS : 0) : nullptr;
  IO* val = reinterpret_cast<IO*>(records + StagedRecords<IO, SMOOTH, MIX>::values_offset());
  b.health = MIX ? val : nullptr;
  b.parked = SMOOTH ? val + (MIX ? 4 : 0) : nullptr;
  return b;
}

// Drone pb's stage records and health factors (null = 1) into its block, and the nine values of the plan it follows: followedg [B][9], or
// null = nothing is followed yet -- sample_plan_smoother's zeros for a plan that is not there, which is what se3mpc_smoother_update_* reads
// through old = NULL.
template <typename IO, bool SMOOTH, bool MIX>
__device__ __forceinline__ void staged_load(const StagedBlock<IO>& b, int pb, const double* __restrict__ smootherg,
                                            const double* __restrict__ mixerg, const IO* __restrict__ healthg, long long health_stride,
                                            const IO* __restrict__ followedg) {
  if constexpr (SMOOTH) {
    for (int i = 0; i < SE3MPC_SMOOTHER_STATE_WORDS; ++i) b.srec[i] = smootherg[(size_t)pb * SE3MPC_SMOOTHER_STATE_WORDS + i];
    for (int i = 0; i < 9; ++i) b.parked[i] = followedg != nullptr ? followedg[(size_t)pb * 9 + i] : (IO)0;
  }
  if constexpr (MIX) {
    for (int i = 0; i < SE3MPC_MIXER_STATE_WORDS; ++i) b.mrec[i] = mixerg[(size_t)pb * SE3MPC_MIXER_STATE_WORDS + i];
    for (int i = 0; i < 4; ++i) b.health[i] = healthg != nullptr ? healthg[(size_t)pb * health_stride + i] : (IO)1;
  }
}
// ... and the records back (followedg: null = the parked values are not kept)
template <typename IO, bool SMOOTH, bool MIX>
__device__ __forceinline__ void staged_store(const StagedBlock<IO>& b, int pb, double* __restrict__ smootherg, double* __restrict__ mixerg,
                                             IO* __restrict__ followedg) {
  if constexpr (SMOOTH) {
    for (int i = 0; i < SE3MPC_SMOOTHER_STATE_WORDS; ++i) smootherg[(size_t)pb * SE3MPC_SMOOTHER_STATE_WORDS + i] = b.srec[i];
    if (followedg != nullptr)
      for (int i = 0; i < 9; ++i) followedg[(size_t)pb * 9 + i] = b.parked[i];
  }
  if constexpr (MIX)
    for (int i = 0; i < SE3MPC_MIXER_STATE_WORDS; ++i) mixerg[(size_t)pb * SE3MPC_MIXER_STATE_WORDS + i] = b.mrec[i];
}

// `n` steps of the act phase of the drone in block b, by ONE lane, against the N-row plan the planner has handed over: with the smoother and
// `take`, first update_trajectory's second part at the drone's clock (the first part's nine values are parked in the block); then the steps
// -- actuated_step with the mixer, smoothed_step without --, after_step(step, pos) behind each; and with `sample` the sample of THIS plan at
// the clock the next update_trajectory will run at, into the parked values.  State and records come from LDS and go back there, so an act
// phase may be flown in several calls (take in the first, sample in the last).  has_health: false = the health operand was NULL (exactly 1,
// as se3mpc_closed_loop_actuated_*).
template <typename IO, bool SMOOTH, bool MIX, typename F>
__device__ __forceinline__ void staged_fly(const StagedBlock<IO>& b, const CtrlDev<IO>& c, const SimDev<IO>& m, const SmoothDev<IO>& sd, const MixDev<IO>& x, int N, int n,
                                           double sim_dt, bool has_health, bool take, bool sample, F&& after_step) {
  static_assert(SMOOTH || MIX, "without a stage the act phase is fly_steps (closed_loop_device.hpp)");
  const DroneBlock<IO>& d = b.d;
  SmoothRegs<IO> sm;
  MixRegs<IO> mx;
  CtrlRegs<IO> s = load_ctrl<IO>(d.ctrl);
  DroneRegs<IO> r;
  r.load(d);
  double* tr = SMOOTH ? b.srec + 9 : nullptr;
  if constexpr (SMOOTH) {
    sm = load_smooth<IO>(b.srec);
    if (take) smoother_take_plan<IO>(sd, sm, r.t, b.parked, N, d.stamps, d.planP, d.planV, d.planA, tr);   // the wall clock of update_trajectory = the drone's clock
  }
  if constexpr (MIX) mx = load_mix<IO>(b.mrec);
  const IO* health = MIX && has_health ? b.health : nullptr;
  const IO dt = (IO)sim_dt;
  PlanCursor<IO> cur;
  cursor_reset(cur);
  for (int step = 0; step < n; ++step) {
    IO th, tq[3];
    if constexpr (MIX)
      actuated_step<IO, SMOOTH>(sd, c, m, x, sm, tr, s, mx, health, cur, N, d.stamps, d.planP, d.planV, d.planA, r.p, r.v, r.a, r.w, r.t, dt, sim_dt,
                                r.wd, th, tq, nullptr, nullptr, nullptr);
    else
      smoothed_step<IO>(sd, c, m, sm, tr, s, cur, N, d.stamps, d.planP, d.planV, d.planA, r.p, r.v, r.a, r.w, r.t, dt, sim_dt, r.wd, th, tq, nullptr);
    after_step(step, r.p);
  }
  r.store(d);
  store_ctrl<IO>(d.ctrl, s);
  if constexpr (MIX) store_mix<IO>(b.mrec, mx);
  if constexpr (SMOOTH) {
    if (sample) smoother_sample_followed<IO>(sm, r.t, N, d.stamps, d.planP, d.planV, d.planA, b.parked);
    store_smooth<IO>(b.srec, sm);
  }
}

// The whole act phase of one cycle in one call; `again`: another cycle follows, so this plan is sampled for it.
template <typename IO, bool SMOOTH, bool MIX>
__device__ __forceinline__ void staged_act(const StagedBlock<IO>& b, const CtrlDev<IO>& c, const SimDev<IO>& m, const SmoothDev<IO>& sd, const MixDev<IO>& x, int N, int substeps,
                                           double sim_dt, bool has_health, bool again) {
  staged_fly<IO, SMOOTH, MIX>(b, c, m, sd, x, N, substeps, sim_dt, has_health, true, again, [](int, const IO*) {});
}

// A cycle without steps (what the chain does when its act launch is the nsteps == 0 no-op: se3mpc_smoother_update_* alone): the smoother takes
// the plan and samples it, nothing else of the block is touched.
template <typename IO>
__device__ __forceinline__ void staged_take_only(const StagedBlock<IO>& b, const SmoothDev<IO>& sd, int N) {
  const DroneBlock<IO>& d = b.d;
  const double now = *d.time;
  SmoothRegs<IO> sm = load_smooth<IO>(b.srec);
  smoother_take_plan<IO>(sd, sm, now, b.parked, N, d.stamps, d.planP, d.planV, d.planA, b.srec + 9);
  smoother_sample_followed<IO>(sm, now, N, d.stamps, d.planP, d.planV, d.planA, b.parked);
  store_smooth<IO>(b.srec, sm);
}

}  // namespace se3mpc
