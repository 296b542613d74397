// mppi_loop_device.hpp -- what the closed-loop MPPI kernels share beyond the planner (mppi_device.hpp) and the flight loop
// (closed_loop_device.hpp): mppi_closed_loop.hip and mppi_closed_loop_staged.hip.  The LDS image behind the planner's,
// the hand-over of the nominal's trajectory to the drone's block and the clearance reduction over the positions an act chunk parked.
// INCLUDE UNDER `#pragma clang fp contract(fast)`, behind mppi_device.hpp: the hand-over is roll_step's recurrence and the clearance a
// measurement; neither feeds a branch of the controller.
#pragma once
#include "mppi_device.hpp"

namespace se3mpc {
namespace mppi {

constexpr int kPark = 64;     // simulator positions parked per clearance reduction (longer act phases run in chunks of this many steps)

// LDS behind the planner's image (bytes, 16-byte aligned regions): stamps [N] double | time [1] double | controller record
// [SE3MPC_CONTROLLER_STATE_WORDS] double | plan P, V, A [3][N][3] R | pos, vel, att, omega, wind, goal, clearance [19] R | raw radii [K] R | parked positions
// [kPark][3] R.  moving (the kernel of moving spheres): the image lies behind moving_lds_layout's and a parked row is
// (x, y, z, tR) -- the position a simulator step produced and the time it is measured at, in the kernel's type.
struct LoopLds {
  size_t stamps, time, ctrl, plan, vec, rad, park, total;
};
__host__ __device__ inline LoopLds loop_lds_layout(int N, int K, int W, size_t esz, bool moving = false) {
  LoopLds x;
  x.stamps = moving ? moving_lds_layout(N, K, W, esz).total : lds_layout(N, K, W, esz).total;
  x.time = x.stamps + (size_t)N * 8;
  x.ctrl = x.time + 8;
  x.plan = align16(x.ctrl + (size_t)SE3MPC_CONTROLLER_STATE_WORDS * 8);
  x.vec = align16(x.plan + (size_t)9 * N * esz);
  x.rad = align16(x.vec + 19 * esz);
  x.park = align16(x.rad + (size_t)K * esz);
  x.total = align16(x.park + (size_t)(moving ? 4 : 3) * kPark * esz);
  return x;
}

// The hand-over, by ONE lane: the nominal U rolled out from (p, v) with roll_step's recurrence into the drone's block -- row k = the state
// BEFORE step k, A_k the acceleration of U_k, stamped plan_stamp(C, substeps, sim_dt, k, plan_dt).  p, v: the caller's copies (changed).
template <typename R>
__device__ __forceinline__ void hand_over_plan(const DevParams<R>& q, R p[3], R v[3], const R* U, const DroneBlock<R>& d, int N, int C, int substeps,
                                               double sim_dt, double plan_dt) {
  for (int k = 0; k < N; ++k) {
    R a3[3];
    const R t[3] = {U[3 * k], U[3 * k + 1], U[3 * k + 2]};
    for (int a = 0; a < 3; ++a) { d.planP[3 * k + a] = p[a]; d.planV[3 * k + a] = v[a]; }
    roll_state_step(q, p, v, t, a3);
    for (int a = 0; a < 3; ++a) d.planA[3 * k + a] = a3[a];
    d.stamps[k] = plan_stamp(C, substeps, sim_dt, k, plan_dt);
  }
}

// The clearance of the n positions an act chunk parked, by the whole workgroup: min over (step, j) of |pos - c_j| - r_j (sph rows (cx, cy,
// cz, .), raw radii rad) folded into *running by the first lane -- wavefront min, then the W partials in wavefront order through red [W].
// The positions are visible to every lane on entry; ends with the workgroup synchronised.  MOVING: park rows are (x, y, z, tR) and sphere j's
// centre is c_j + svel_j * tR (svel [K][3]); the distance keeps its form.
template <typename R, bool MOVING = false>
__device__ __forceinline__ void clearance_chunk(const R* park, const R* sph, const R* rad, int n, int K, double* red, R* running,
                                                const R* svel = nullptr) {
  const int NT = (int)blockDim.x, W = NT / kWave;
  const int tid = (int)threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  R ml = (R)__builtin_huge_val();
  for (int i = tid; i < n * K; i += NT) {
    const int step = i / K, j = i - step * K;
    R dx, dy, dz;
    if constexpr (MOVING) {
      const R tR = park[4 * step + 3];
      const R cx = sph[4 * j] + svel[3 * j] * tR, cy = sph[4 * j + 1] + svel[3 * j + 1] * tR, cz = sph[4 * j + 2] + svel[3 * j + 2] * tR;
      dx = park[4 * step] - cx; dy = park[4 * step + 1] - cy; dz = park[4 * step + 2] - cz;
    } else {
      dx = park[3 * step] - sph[4 * j]; dy = park[3 * step + 1] - sph[4 * j + 1]; dz = park[3 * step + 2] - sph[4 * j + 2];
    }
    ml = fmin(ml, sqrt(dx * dx + dy * dy + dz * dz) - rad[j]);
  }
  const double wm = wave_min((double)ml);
  if (lane == 0) red[wave] = wm;
  __syncthreads();
  double mc = red[0];
  for (int w = 1; w < W; ++w) mc = fmin(mc, red[w]);
  if (tid == 0) *running = fmin(*running, (R)mc);
  __syncthreads();
}

}  // namespace mppi
}  // namespace se3mpc
