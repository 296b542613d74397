// lane_common.hpp -- what the lane-layout ([row][b]) files share beside se3mpc_common.hpp: the lane bookkeeping of the one-trajectory-per-lane
// kernels, the argument check and tuning state of their launchers, and the ONE table that routes a horizon to a rollout sweep
// (parity_kernels.hip, rollout.hip, rollout_obstacles.hip, rollout_iterate.hip, reduce_kernels.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <initializer_list>
#include <type_traits>

#include "se3mpc_common.hpp"

namespace se3mpc {

// Lane bookkeeping shared by the one-trajectory-per-lane kernels (64-thread workgroups): blocks are taken
// in XCD-contiguous order (blocks that share an XCD -- dispatch is round-robin over the 8 XCDs -- stream
// adjacent columns: +5..10 % on the rollout kernel), rows are addressed through a buffer resource with a
// 32-bit lane offset, and once-streamed operands use the nt cache policy.
struct LaneIdx {
  int b;
  bool live;
  unsigned voff;
};
template <typename R>
__device__ __forceinline__ LaneIdx lane_index(int B) {
  int blk = blockIdx.x;
  if ((gridDim.x & 7) == 0) blk = (blk & 7) * (gridDim.x >> 3) + (blk >> 3);
  LaneIdx li;
  const int b0 = blk * (int)blockDim.x + (int)threadIdx.x;
  li.live = b0 < B;
  li.b = li.live ? b0 : B - 1;
  li.voff = (unsigned)li.b * (unsigned)sizeof(R);
  return li;
}

// ------------------------------------------------------------------------------------------
// host side: validation, tuning state, horizon routing
// ------------------------------------------------------------------------------------------
// `rows` = the tallest lane-layout operand of the call: buffer offsets (row * ld * sizeof) must stay 32-bit
inline int check_lane_args(const se3mpc_params* p, int B, int ld, long long rows = 0, size_t elem = 8) {
  if (p == nullptr) return SE3MPC_ERR_NULL;
  const int rc = check_params_impl(p);
  if (rc != SE3MPC_OK) return rc;
  if (B < 0 || ld < B || ld > (1 << 28)) return SE3MPC_ERR_SHAPE;   // lane byte offsets stay 32-bit
  if (rows == 0) rows = 9LL * p->horizon;
  if ((unsigned long long)rows * (unsigned long long)ld * elem >= (1ull << 32)) return SE3MPC_ERR_SHAPE;
  return SE3MPC_OK;
}

constexpr int kLaneBlock = 64;   // one wavefront per workgroup: small batches still spread over CUs

// What se3mpc_set_rollout_variant (rollout.hip, which defines the object) selects; every field 0 = the measured defaults.
struct LaneTuning {
  int rollout_variant = 0;   // 0 auto, 1 REG split, 2 LDS, 3 REV split, 4 REG mono, 5 REV mono, 6 REG bucket; +8*(FLAGS+1): explicit FLAGS (N = 30 f32 grad only); +128 / +256 / +384: workgroup shapes of the obstacle kernels
  int wide_select = 0;       // +512 / +1024: the 16-bytes-per-lane kernels never / whenever the shapes allow (default: from kWideMinBatch up)
  int obs_mfma = 0;          // +2048: se3mpc_rollout_obstacles_* forms its float32 residuals on the matrix core (expanded form; measured evidence, not the default)
};
extern LaneTuning g_lane_tuning;

// the 16-bytes-per-lane kernels (parity_kernels.hip) are taken when this holds
constexpr int kWideMinBatch = 1 << 18;
inline bool wide_ok(int B, int ld, std::initializer_list<const void*> ptrs) {
  const int sel = g_lane_tuning.wide_select;
  if (sel == 1 || (sel == 0 && B < kWideMinBatch) || B < 4 || (B & 3) || (ld & 3)) return false;
  for (const void* q : ptrs)
    if (q != nullptr && (reinterpret_cast<uintptr_t>(q) & 15u)) return false;
  return true;
}

// ---- horizon -> rollout sweep: the one routing table of the shooting-form kernels ----------------------------------------
// A sweep as a compile-time tag: NN = the register bound (0: none), REG = register arrays, FLAGS as rollout_kernel's (7, or 15 = N is a bucket).
template <int NN_, bool REG_, int FLAGS_>
struct Sweep {
  static constexpr int NN = NN_, FLAGS = FLAGS_;
  static constexpr bool REG = REG_;
};
enum SweepRoute { kSweepAuto, kSweepExact, kSweepBucket, kSweepRev };   // Exact / Bucket: that sweep or, where the horizon has none, the reversible one

// Calls launch(Sweep<...>{}) with the sweep of horizon N:
//   exact-N register kernels exist for the BASELINE horizons {6, 20} and, float32 only, {30, 50}: f64 arrays spill beyond N = 20;
//   any other horizon (measured at B = 1 M, tools/gpu_probe_horizons.py): 17..32 steps -> a 32-step register bucket
//   (guarded steps; 5.3-5.5 TB/s vs 4.5-4.7 for the reversible sweep); <= 16 or > 32 steps -> the reversible
//   sweep (6.0-6.5 TB/s on short horizons; a 64-step bucket needs 256 VGPRs and drops to 2.2 TB/s).  f32 only.
// BUCKET = false: the caller's kernel has no bucket form.  `launch` is instantiated for exactly the tags listed here.
template <typename R, bool BUCKET, typename F>
void dispatch_horizon(int N, SweepRoute want, F&& launch) {
  constexpr bool f32 = sizeof(R) == 4;
  if (want == kSweepAuto || want == kSweepExact) {
    if (N == 6) return launch(Sweep<6, true, 7>{});
    if (N == 20) return launch(Sweep<20, true, 7>{});
    if constexpr (f32) {
      if (N == 30) return launch(Sweep<30, true, 7>{});
      if (N == 50) return launch(Sweep<50, true, 7>{});
    }
  }
  if constexpr (f32 && BUCKET) {
    const bool has_bucket = N > 16 && N <= 32;
    if (has_bucket && (want == kSweepAuto || want == kSweepBucket)) return launch(Sweep<32, true, 15>{});
  }
  launch(Sweep<0, false, 7>{});
}

}  // namespace se3mpc
