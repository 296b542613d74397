// mppi_swarm.hip -- the closed-loop MPPI Monte-Carlo of mppi_closed_loop_moving.hip for SWARMS: the B drones of a call are B / M swarms of M
// drones, and every drone plans around its nearest swarm-mates as spheres that move with constant velocity.  One launch is
// ONE planning cycle of mppi_closed_loop_moving_kernel -- plan, hand over, act, clearance, warm start through the same functions with their
// MOVING switch on -- behind a prologue that builds the drone's own table in LDS:
//   rows [0, Ks)            the caller's shared spheres and velocities, staged as the moving kernel stages them
//   rows [Ks, Ks + Kn_eff)  the Kn_eff = min(Kn, E) eligible mates with the smallest (d2, index), d2 in float64 on the cycle's snapshot,
//                           row Ks + r = the mate of rank r: centre c' = pos - (vel * tR0) (so that the kernel's c' + vel * tR_k is the mate at
//                           the cycle's start, extrapolated), velocity, (mate_radius + margin)^2
// The mates are read from a SNAPSHOT of (pos, vel) that the launch before wrote (the seed kernel before the first cycle), never from pos / vel,
// which the workgroups of this launch are rewriting: every workgroup reads image A and writes its new (pos, vel) to image B, the host swaps the
// two between launches, and the kernel boundary is the only synchronisation.  The in-flight clearance is measured against rows [0, Ks) only.
#pragma clang fp contract(off)
#include "closed_loop_device.hpp"
#pragma clang fp contract(fast)
#include "mppi_device.hpp"
#include "mppi_loop_device.hpp"

namespace se3mpc {
namespace mppi {

#pragma clang fp contract(off)
// The squared distance of snapshot row a = (x, y, z, ...) from row own, in float64, summed left to right: a NumPy restatement has its bits
template <typename R>
__device__ __forceinline__ double mate_d2(const R* __restrict__ a, const R* __restrict__ own) {
  const double dx = (double)a[0] - (double)own[0];
  const double dy = (double)a[1] - (double)own[1];
  const double dz = (double)a[2] - (double)own[2];
  return dx * dx + dy * dy + dz * dz;
}

// Row ((x, y, z), (vx, vy, vz)) of a mate's table entry: the centre rebased to the table's time 0, c' = pos - (vel * tR0), two roundings
template <typename R>
__device__ __forceinline__ void mate_centre(const R* __restrict__ pos, const R* __restrict__ vel, R tR0, R c[3]) {
  for (int a = 0; a < 3; ++a) {
    const R back = vel[a] * tR0;
    c[a] = pos[a] - back;
  }
}
#pragma clang fp contract(fast)

// Eligible: the six values of a drone's (pos, vel) are finite
template <typename R>
__device__ __forceinline__ bool six_finite(const R* __restrict__ p3, const R* __restrict__ v3) {
  bool ok = true;
  for (int a = 0; a < 3; ++a) ok = ok && __builtin_isfinite(p3[a]) && __builtin_isfinite(v3[a]);
  return ok;
}

// LDS behind loop_lds_layout(N, Ks + Kn, W, esz, true): d2 [M] double (NaN = not eligible) | dmin [1] double | sel [Kn] int32 (-1 = empty)
struct SwarmLds {
  size_t d2, dmin, sel, total;
};
__host__ __device__ inline SwarmLds swarm_lds_layout(int N, int Kcap, int W, size_t esz, int M, int Kn) {
  SwarmLds s;
  s.d2 = loop_lds_layout(N, Kcap, W, esz, true).total;
  s.dmin = s.d2 + (size_t)M * 8;
  s.sel = s.dmin + 8;
  s.total = align16(s.sel + (size_t)Kn * 4);
  return s;
}

// Wavefronts per SIMD: those of mppi_closed_loop_moving_kernel
template <typename R>
struct SwarmWaves { static constexpr int value = 3; };
template <>
struct SwarmWaves<double> { static constexpr int value = 2; };

// (pos, vel) [B][3] -> snapshot [B][6], one value per lane
template <typename R>
__global__ void __launch_bounds__(kBlock)
swarm_seed_kernel(int B, const R* __restrict__ posg, const R* __restrict__ velg, R* __restrict__ snap) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= 6 * B) return;
  const int b = i / 6, a = i - 6 * b;
  snap[i] = a < 3 ? posg[3 * b + a] : velg[3 * b + a - 3];
}

// One drone per lane: the distance to the nearest eligible mate NOW, folded into separation[b]
template <typename R>
__global__ void __launch_bounds__(kBlock)
swarm_separation_kernel(int B, int M, const R* __restrict__ posg, const R* __restrict__ velg, R* __restrict__ separation) {
  const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (b >= B) return;
  if (!six_finite(posg + 3 * b, velg + 3 * b)) return;
  const int base = (b / M) * M;
  double dmin = 0.0;
  bool any = false;
  for (int i = 0; i < M; ++i) {
    const int o = base + i;
    if (o == b || !six_finite(posg + 3 * o, velg + 3 * o)) continue;
    const double d2 = mate_d2(posg + 3 * o, posg + 3 * b);
    dmin = any ? fmin(dmin, d2) : d2;
    any = true;
  }
  if (any) separation[b] = fmin(separation[b], (R)sqrt(dmin));
}

// cyc: this launch's cycle within the call's `cycles` (the trace row); last: the call's last cycle (cost, plan_last, neighbours).
// snapA NULL: no swarm (M = 1, or nothing wants the mates): the prologue's mate part and the snapshot write are skipped.
template <typename R>
__global__ void __launch_bounds__(kBlock, SwarmWaves<R>::value)
mppi_swarm_cycle_kernel(DevParams<R> q, CtrlDev<R> ctl, SimDev<R> sim, double plan_dt, int cycles, int cyc, bool last, int substeps, double sim_dt,
                        uint32_t C, int shift, int S, int iters, R sigma, double inv_lam, uint32_t key0, uint32_t key1, uint32_t iter_base,
                        uint32_t index_base, const R* __restrict__ goalg, const R* __restrict__ spheres, const R* __restrict__ sphere_vel,
                        double sphere_t0, int Ks, int Kn, int M, R mate_radius, R w_obs, const R* __restrict__ windg, long long wind_stride,
                        double* __restrict__ timeg, R* __restrict__ posg, R* __restrict__ velg, R* __restrict__ attg, R* __restrict__ omegag,
                        double* __restrict__ stateg, R* __restrict__ Ug, R* __restrict__ cost_out, R* __restrict__ trace,
                        R* __restrict__ plan_last, R* __restrict__ clearance, R* __restrict__ separation, int32_t* __restrict__ neighbours,
                        const R* __restrict__ snapA, R* __restrict__ snapB) {
  HIP_DYNAMIC_SHARED(unsigned char, lds_raw)
  const int N = q.N, rows = 3 * N, NT = (int)blockDim.x, W = NT / kWave;
  const int tid = (int)threadIdx.x, wave = tid / kWave;
  const int b = (int)blockIdx.x;
  const int Kcap = Ks + Kn;
  const LoopLds X = loop_lds_layout(N, Kcap, W, sizeof(R), true);
  const MovingLds ML = moving_lds_layout(N, Kcap, W, sizeof(R));
  const SwarmLds SL = swarm_lds_layout(N, Kcap, W, sizeof(R), M, Kn);
  const LdsView<R> l = lds_view<R>(lds_raw, lds_layout(N, Kcap, W, sizeof(R)));
  R* U = l.U;
  R* sph = l.sph;
  R* svel = reinterpret_cast<R*>(lds_raw + ML.vel);
  R* stime = reinterpret_cast<R*>(lds_raw + ML.time);
  const DroneBlock<R> d = drone_block<R>(lds_raw + X.stamps, N, X.plan - X.stamps, X.vec - X.stamps);
  R* s_vec = d.vec;                                         // pos, vel, att, omega, wind | goal, running clearance
  R* rad = reinterpret_cast<R*>(lds_raw + X.rad);           // raw radii of the shared rows (the clearance sees no others)
  R* park = reinterpret_cast<R*>(lds_raw + X.park);         // [kPark][4] = (x, y, z, tR)
  double* d2 = reinterpret_cast<double*>(lds_raw + SL.d2);
  double* dmin = reinterpret_cast<double*>(lds_raw + SL.dmin);
  int32_t* sel = reinterpret_cast<int32_t*>(lds_raw + SL.sel);
  const bool want_clear = clearance != nullptr && Ks > 0;
  const bool swarm = snapA != nullptr;
  const int base = (b / M) * M, self = b - base;

  // ---- prologue 1: the shared rows, as the moving kernel stages them
  for (int r = tid; r < rows; r += NT) U[r] = Ug[(size_t)b * rows + r];
  stage_spheres(q, spheres, Ks, sph);
  for (int i = tid; i < 3 * Ks; i += NT) svel[i] = sphere_vel[i];
  for (int j = tid; j < Ks; j += NT) rad[j] = spheres[4 * j + 3];
  for (int r = tid; r < Kn; r += NT) sel[r] = -1;
  if (tid == 0) {
    drone_load<R>(d, b, posg, velg, attg, omegag, windg, wind_stride, timeg, stateg);
    for (int i = 0; i < 3; ++i) s_vec[15 + i] = q.has_goal ? goalg[3 * b + i] : (R)0;
    s_vec[18] = want_clear ? clearance[b] : (R)0;
    *dmin = __builtin_nan("");
  }
  // ---- prologue 2, 3: d2 of every mate in float64 on the snapshot; NaN marks a mate that is not eligible (an eligible one's is never NaN)
  if (swarm) {
    const R* own = snapA + (size_t)6 * b;
    const bool own_ok = six_finite(own, own + 3);
    for (int i = tid; i < M; i += NT) {
      const R* row = snapA + (size_t)6 * (base + i);
      d2[i] = (own_ok && i != self && six_finite(row, row + 3)) ? mate_d2(row, own) : __builtin_nan("");
    }
  }
  __syncthreads();
  // ---- prologue 3, 4: rank by counting over (d2, index); the mate of rank r < Kn fills row Ks + r
  if (swarm) {
    const R tR0 = (R)(sphere_t0 + plan_stamp((int)C, substeps, sim_dt, 0, plan_dt));
    for (int i = tid; i < M; i += NT) {
      const double di = d2[i];
      if (!(di == di)) continue;
      int rank = 0;
      for (int j = 0; j < M; ++j) {
        const double dj = d2[j];
        rank += (dj < di || (dj == di && j < i)) ? 1 : 0;
      }
      if (rank == 0) *dmin = di;
      if (rank < Kn) {
        const R* row = snapA + (size_t)6 * (base + i);
        R c3[3];
        mate_centre(row, row + 3, tR0, c3);
        const int at = Ks + rank;
        for (int a = 0; a < 3; ++a) { sph[4 * at + a] = c3[a]; svel[3 * at + a] = row[3 + a]; }
        sph[4 * at + 3] = (mate_radius + q.margin) * (mate_radius + q.margin);
        sel[rank] = i;
      }
    }
    __syncthreads();
  }
  // ---- prologue 5: ranks are dense, so the filled slots are the first Kn_eff
  int K = Ks;
  for (int r = 0; r < Kn; ++r) K += sel[r] >= 0 ? 1 : 0;

  // the planner's context as mppi_closed_loop_moving_kernel builds it
  Ctx<R, true> c = load_ctx<R, true>(q, 1, 0, key0, key1, index_base + (uint32_t)b, s_vec, s_vec + 3, s_vec + 15, U, sph, K, w_obs);
  c.svel = svel;
  c.stime = stime;
  c.gl[0] = wave_bcast(c.gl[0], 0); c.gl[1] = wave_bcast(c.gl[1], 0); c.gl[2] = wave_bcast(c.gl[2], 0);

  // ---- the step times of this cycle's plan
  for (int k = tid; k < N; k += NT) stime[k] = (R)(sphere_t0 + plan_stamp((int)C, substeps, sim_dt, k, plan_dt));
  __syncthreads();
  // ---- plan
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
  // ---- act, in chunks of kPark steps; the clearance against the shared rows
  int s0 = 0;
  do {
    const int n = substeps - s0 < kPark ? substeps - s0 : kPark;
    if (tid == 0 && n > 0)
      fly_steps<R>(ctl, sim, d, N, n, sim_dt, [&](int step, const R* p) {
        if (want_clear) {
          park[4 * step] = p[0]; park[4 * step + 1] = p[1]; park[4 * step + 2] = p[2];
          park[4 * step + 3] = (R)(sphere_t0 + (double)((int)C * substeps + s0 + step + 1) * sim_dt);
        }
      });
    __syncthreads();
    if (want_clear && n > 0) clearance_chunk<R, true>(park, sph, rad, n, Ks, l.red, s_vec + 18, svel);
    s0 += kPark;
  } while (s0 < substeps);
  if (last && plan_last != nullptr)
    for (int r = tid; r < 3 * rows; r += NT) plan_last[(size_t)b * 3 * rows + r] = d.planP[r];
  if (last && neighbours != nullptr)
    for (int r = tid; r < Kn; r += NT) neighbours[(size_t)b * Kn + r] = sel[r] >= 0 ? base + sel[r] : -1;
  // ---- warm start of the next cycle
  shift_nominal(q, U, reinterpret_cast<R*>(l.acc), shift);

  for (int r = tid; r < rows; r += NT) Ug[(size_t)b * rows + r] = U[r];
  if (tid == 0) {
    drone_store<R>(d, b, posg, velg, attg, omegag, timeg, stateg);
    if (want_clear) clearance[b] = s_vec[18];
    if (swarm) {
      for (int i = 0; i < 6; ++i) snapB[(size_t)6 * b + i] = s_vec[i];
      const double dm = *dmin;
      if (separation != nullptr && dm == dm) separation[b] = fmin(separation[b], (R)sqrt(dm));
    }
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
static size_t swarm_workspace_bytes(int B, int elem_size) {
  if (B < 0 || (elem_size != 4 && elem_size != 8)) return 0;
  return (size_t)2 * 6 * (size_t)B * (size_t)elem_size;
}

template <typename R>
static int mppi_closed_loop_swarm_impl(const se3mpc_params* p, const se3mpc_controller_params* cp, const se3mpc_simulator_params* sp, int B,
                                       int swarm_size, int neighbours_k, double mate_radius, int cycles, int substeps, double sim_dt,
                                       uint32_t cycle_base, int shift, int S, int iters, double sigma, double temperature, uint64_t seed,
                                       uint32_t iter_base, uint32_t index_base, const R* goal, const R* spheres, const R* sphere_vel,
                                       double sphere_t0, int K, double obstacle_weight, const R* wind, long long wind_stride, double* time, R* pos,
                                       R* vel, R* att, R* omega, double* state, R* U, R* cost, R* trace, R* plan_last, R* clearance, R* separation,
                                       int32_t* neighbours, void* workspace, size_t workspace_bytes, void* stream) {
  const char* fn = "se3mpc_mppi_closed_loop_swarm";
  if (p == nullptr || cp == nullptr || sp == nullptr) return fail(SE3MPC_ERR_NULL, "NULL parameter struct", fn);
  int rc = check_params_impl(p);
  if (rc) return fail(rc, "invalid se3mpc_params", fn);
  rc = check_controller_params(cp);
  if (rc) return fail(rc, "invalid se3mpc_controller_params", fn);
  rc = check_simulator_params(sp);
  if (rc) return fail(rc, "invalid se3mpc_simulator_params", fn);
  if (cycles < 0 || substeps < 0) return fail(SE3MPC_ERR_SHAPE, "cycles or substeps < 0", fn);
  if (shift < 0 || shift > p->horizon) return fail(SE3MPC_ERR_SHAPE, "shift outside [0, horizon]", fn);
  if (wind != nullptr && !(wind_stride == 0 || wind_stride >= 3)) return fail(SE3MPC_ERR_SHAPE, "wind_stride must be 0 or >= 3", fn);
  rc = check_mppi_args(fn, p, B, B, S, iters, sigma, temperature, K, obstacle_weight);
  if (rc) return rc;
  if (!std::isfinite(sim_dt)) return fail(SE3MPC_ERR_PARAM, "sim_dt must be finite", fn);
  rc = check_moving_args(fn, K, sphere_vel, sphere_t0);
  if (rc) return rc;
  if (swarm_size < 1 || swarm_size > SE3MPC_MAX_SWARM) return fail(SE3MPC_ERR_SHAPE, "swarm_size outside [1, SE3MPC_MAX_SWARM]", fn);
  if (B % swarm_size != 0) return fail(SE3MPC_ERR_SHAPE, "B is not a multiple of swarm_size", fn);
  if (neighbours_k < 0) return fail(SE3MPC_ERR_SHAPE, "neighbours_k < 0", fn);
  if (K + neighbours_k > SE3MPC_MAX_SPHERES) return fail(SE3MPC_ERR_SHAPE, "K + neighbours_k > SE3MPC_MAX_SPHERES", fn);
  if (!(mate_radius >= 0.0) || !std::isfinite(mate_radius)) return fail(SE3MPC_ERR_PARAM, "mate_radius must be finite and >= 0", fn);
  if (swarm_size > 1 && workspace != nullptr && workspace_bytes < swarm_workspace_bytes(B, (int)sizeof(R)))
    return fail(SE3MPC_ERR_SHAPE, "workspace_bytes < se3mpc_mppi_swarm_workspace_bytes(B, elem_size)", fn);
  if (B == 0 || cycles == 0) return SE3MPC_OK;
  if (!time || !pos || !vel || !att || !omega || !state || !U || !cost || (p->has_goal && !goal) || (K > 0 && !spheres))
    return fail(SE3MPC_ERR_NULL, "NULL operand", fn);
  if (swarm_size > 1 && neighbours_k > 0 && (workspace == nullptr || separation == nullptr))
    return fail(SE3MPC_ERR_NULL, "NULL workspace or separation with swarm_size > 1 and neighbours_k > 0", fn);
  // the mates are looked at when there are any and something wants them: the table (neighbours_k > 0) or the separation
  const bool swarm = swarm_size > 1 && workspace != nullptr && (neighbours_k > 0 || separation != nullptr);
  R* snap[2] = {nullptr, nullptr};
  if (swarm) {
    snap[0] = static_cast<R*>(workspace);
    snap[1] = snap[0] + (size_t)6 * B;
    hipLaunchKernelGGL(swarm_seed_kernel<R>, dim3(grid_for(6 * B, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, B, (const R*)pos, (const R*)vel,
                       snap[0]);
  }
  const int NT = S < kBlock ? S : kBlock;
  const SwarmLds SL = swarm_lds_layout(p->horizon, K + neighbours_k, NT / kWave, sizeof(R), swarm_size, neighbours_k);
  for (int cyc = 0; cyc < cycles; ++cyc)
    hipLaunchKernelGGL(mppi_swarm_cycle_kernel<R>, dim3(B), dim3(NT), SL.total, (hipStream_t)stream, make_dev_params<R>(*p), make_ctrl_dev<R>(*cp),
                       make_sim_dev<R>(*sp), p->dt, cycles, cyc, cyc == cycles - 1, substeps, sim_dt, cycle_base + (uint32_t)cyc, shift, S, iters,
                       (R)sigma, 1.0 / temperature, (uint32_t)seed, (uint32_t)(seed >> 32), iter_base, index_base, goal, spheres, sphere_vel,
                       sphere_t0, K, neighbours_k, swarm_size, (R)mate_radius, (R)obstacle_weight, wind, wind_stride, time, pos, vel, att, omega,
                       state, U, cost, trace, plan_last, clearance, separation, neighbours, (const R*)snap[cyc & 1], snap[(cyc + 1) & 1]);
  return launch_status(fn);
}

template <typename R>
static int swarm_separation_impl(int B, int swarm_size, const R* pos, const R* vel, R* separation, void* stream) {
  const char* fn = "se3mpc_swarm_separation";
  if (B < 0) return fail(SE3MPC_ERR_SHAPE, "B < 0", fn);
  if (swarm_size < 1 || swarm_size > SE3MPC_MAX_SWARM) return fail(SE3MPC_ERR_SHAPE, "swarm_size outside [1, SE3MPC_MAX_SWARM]", fn);
  if (B % swarm_size != 0) return fail(SE3MPC_ERR_SHAPE, "B is not a multiple of swarm_size", fn);
  if (B == 0) return SE3MPC_OK;
  if (!pos || !vel || !separation) return fail(SE3MPC_ERR_NULL, "NULL operand", fn);
  if (swarm_size == 1) return SE3MPC_OK;
  hipLaunchKernelGGL(swarm_separation_kernel<R>, dim3(grid_for(B, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, B, swarm_size, pos, vel,
                     separation);
  return launch_status(fn);
}

}  // namespace mppi
}  // namespace se3mpc

using se3mpc::mppi::mppi_closed_loop_swarm_impl;
using se3mpc::mppi::swarm_separation_impl;

extern "C" size_t se3mpc_mppi_swarm_workspace_bytes(int B, int elem_size) { return se3mpc::mppi::swarm_workspace_bytes(B, elem_size); }

extern "C" int se3mpc_mppi_closed_loop_swarm_f32(const se3mpc_params* p, const se3mpc_controller_params* cp, const se3mpc_simulator_params* sp, int B,
                                                 int swarm_size, int neighbours_k, double mate_radius, int cycles, int substeps, double sim_dt,
                                                 uint32_t cycle_base, int shift, int S, int iters, double sigma, double temperature, uint64_t seed,
                                                 uint32_t iter_base, uint32_t index_base, const float* goal, const float* spheres,
                                                 const float* sphere_vel, double sphere_t0, int K, double obstacle_weight, const float* wind,
                                                 long long wind_stride, double* time, float* pos, float* vel, float* att, float* omega, double* state,
                                                 float* U, float* cost, float* trace, float* plan_last, float* clearance, float* separation,
                                                 int32_t* neighbours, void* workspace, size_t workspace_bytes, void* stream) {
  return mppi_closed_loop_swarm_impl<float>(p, cp, sp, B, swarm_size, neighbours_k, mate_radius, cycles, substeps, sim_dt, cycle_base, shift, S, iters,
                                            sigma, temperature, seed, iter_base, index_base, goal, spheres, sphere_vel, sphere_t0, K, obstacle_weight,
                                            wind, wind_stride, time, pos, vel, att, omega, state, U, cost, trace, plan_last, clearance, separation,
                                            neighbours, workspace, workspace_bytes, stream);
}
extern "C" int se3mpc_mppi_closed_loop_swarm_f64(const se3mpc_params* p, const se3mpc_controller_params* cp, const se3mpc_simulator_params* sp, int B,
                                                 int swarm_size, int neighbours_k, double mate_radius, int cycles, int substeps, double sim_dt,
                                                 uint32_t cycle_base, int shift, int S, int iters, double sigma, double temperature, uint64_t seed,
                                                 uint32_t iter_base, uint32_t index_base, const double* goal, const double* spheres,
                                                 const double* sphere_vel, double sphere_t0, int K, double obstacle_weight, const double* wind,
                                                 long long wind_stride, double* time, double* pos, double* vel, double* att, double* omega,
                                                 double* state, double* U, double* cost, double* trace, double* plan_last, double* clearance,
                                                 double* separation, int32_t* neighbours, void* workspace, size_t workspace_bytes, void* stream) {
  return mppi_closed_loop_swarm_impl<double>(p, cp, sp, B, swarm_size, neighbours_k, mate_radius, cycles, substeps, sim_dt, cycle_base, shift, S, iters,
                                             sigma, temperature, seed, iter_base, index_base, goal, spheres, sphere_vel, sphere_t0, K, obstacle_weight,
                                             wind, wind_stride, time, pos, vel, att, omega, state, U, cost, trace, plan_last, clearance, separation,
                                             neighbours, workspace, workspace_bytes, stream);
}

extern "C" int se3mpc_swarm_separation_f32(int B, int swarm_size, const float* pos, const float* vel, float* separation, void* stream) {
  return swarm_separation_impl<float>(B, swarm_size, pos, vel, separation, stream);
}
extern "C" int se3mpc_swarm_separation_f64(int B, int swarm_size, const double* pos, const double* vel, double* separation, void* stream) {
  return swarm_separation_impl<double>(B, swarm_size, pos, vel, separation, stream);
}

// ---- shared plans -----------------------------------------------------------------------------------------------------
// se3mpc_mppi_closed_loop_swarm_intent_*: the swarm cycle above with the mates handed over as their PLANS, not as (pos, vel) extrapolated.
// Beside its snapshot row every drone publishes its INTENT: its nominal, already shifted, rolled out from the state it is about to store --
// N rows, row k = the position before step k of the next cycle's plan, exactly the instants roll_step penalises in that cycle, so the reader
// needs no interpolation and no clock.  Selection is the cycle kernel's own (float64 d2 on the snapshot, ties to the lower index, six finite
// values); the mate of rank r then fills TRACKED row r of every step (mppi_device.hpp) instead of moving row Ks + r.  Images: [B][6]
// snapshot | [B][N][3] intent, two of them, read A / write B, swapped between launches: the kernel boundary stays the only synchronisation.
namespace se3mpc {
namespace mppi {

// The intent of one drone, by ONE lane: U [N][3] rolled out from (pos, vel) with roll_state_step, intent row k = the position BEFORE step k
template <typename R>
__device__ __forceinline__ void swarm_intent_rows(const DevParams<R>& q, const R* pos, const R* vel, const R* U, R* __restrict__ intent) {
  R p[3] = {pos[0], pos[1], pos[2]}, v[3] = {vel[0], vel[1], vel[2]};
  for (int k = 0; k < q.N; ++k) {
    R a3[3];
    const R t[3] = {U[3 * k], U[3 * k + 1], U[3 * k + 2]};
    for (int a = 0; a < 3; ++a) intent[3 * k + a] = p[a];
    roll_state_step(q, p, v, t, a3);
  }
}

// One drone per lane: the seed of a run (se3mpc_swarm_intent_*)
template <typename R>
__global__ void __launch_bounds__(kBlock)
swarm_intent_kernel(DevParams<R> q, int B, const R* __restrict__ posg, const R* __restrict__ velg, const R* __restrict__ Ug, R* __restrict__ intent) {
  const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (b >= B) return;
  swarm_intent_rows(q, posg + 3 * b, velg + 3 * b, Ug + (size_t)3 * q.N * b, intent + (size_t)3 * q.N * b);
}

// mppi_swarm_cycle_kernel with the mates in tracked rows.  snapA / snapB: the [B][6] snapshots of the two images, intentA / intentB their
// [B][N][3] intents.  LDS: swarm_lds_layout on the Ks shared rows, and behind it trk [N][Kn][4] (rows of Kt = Kn_eff entries are used).
template <typename R>
__global__ void __launch_bounds__(kBlock, SwarmWaves<R>::value)
mppi_swarm_intent_cycle_kernel(DevParams<R> q, CtrlDev<R> ctl, SimDev<R> sim, double plan_dt, int cycles, int cyc, bool last, int substeps,
                               double sim_dt, uint32_t C, int shift, int S, int iters, R sigma, double inv_lam, uint32_t key0, uint32_t key1,
                               uint32_t iter_base, uint32_t index_base, const R* __restrict__ goalg, const R* __restrict__ spheres,
                               const R* __restrict__ sphere_vel, double sphere_t0, int Ks, int Kn, int M, R mate_radius, R w_obs,
                               const R* __restrict__ windg, long long wind_stride, double* __restrict__ timeg, R* __restrict__ posg,
                               R* __restrict__ velg, R* __restrict__ attg, R* __restrict__ omegag, double* __restrict__ stateg, R* __restrict__ Ug,
                               R* __restrict__ cost_out, R* __restrict__ trace, R* __restrict__ plan_last, R* __restrict__ clearance,
                               R* __restrict__ separation, int32_t* __restrict__ neighbours, const R* __restrict__ snapA,
                               const R* __restrict__ intentA, R* __restrict__ snapB, R* __restrict__ intentB) {
  HIP_DYNAMIC_SHARED(unsigned char, lds_raw)
  const int N = q.N, rows = 3 * N, NT = (int)blockDim.x, W = NT / kWave;
  const int tid = (int)threadIdx.x, wave = tid / kWave;
  const int b = (int)blockIdx.x;
  const LoopLds X = loop_lds_layout(N, Ks, W, sizeof(R), true);
  const MovingLds ML = moving_lds_layout(N, Ks, W, sizeof(R));
  const SwarmLds SL = swarm_lds_layout(N, Ks, W, sizeof(R), M, Kn);
  const TrackLds TL = track_lds_layout(SL.total, N, Kn, sizeof(R));
  const LdsView<R> l = lds_view<R>(lds_raw, lds_layout(N, Ks, W, sizeof(R)));
  R* U = l.U;
  R* sph = l.sph;
  R* svel = reinterpret_cast<R*>(lds_raw + ML.vel);
  R* stime = reinterpret_cast<R*>(lds_raw + ML.time);
  R* trk = reinterpret_cast<R*>(lds_raw + TL.trk);
  const DroneBlock<R> d = drone_block<R>(lds_raw + X.stamps, N, X.plan - X.stamps, X.vec - X.stamps);
  R* s_vec = d.vec;                                         // pos, vel, att, omega, wind | goal, running clearance
  R* rad = reinterpret_cast<R*>(lds_raw + X.rad);
  R* park = reinterpret_cast<R*>(lds_raw + X.park);         // [kPark][4] = (x, y, z, tR)
  double* d2 = reinterpret_cast<double*>(lds_raw + SL.d2);
  double* dmin = reinterpret_cast<double*>(lds_raw + SL.dmin);
  int32_t* sel = reinterpret_cast<int32_t*>(lds_raw + SL.sel);
  const bool want_clear = clearance != nullptr && Ks > 0;
  const bool swarm = snapA != nullptr;
  const int base = (b / M) * M, self = b - base;

  // ---- prologue 1: the shared rows, as the moving kernel stages them
  for (int r = tid; r < rows; r += NT) U[r] = Ug[(size_t)b * rows + r];
  stage_spheres(q, spheres, Ks, sph);
  for (int i = tid; i < 3 * Ks; i += NT) svel[i] = sphere_vel[i];
  for (int j = tid; j < Ks; j += NT) rad[j] = spheres[4 * j + 3];
  for (int r = tid; r < Kn; r += NT) sel[r] = -1;
  if (tid == 0) {
    drone_load<R>(d, b, posg, velg, attg, omegag, windg, wind_stride, timeg, stateg);
    for (int i = 0; i < 3; ++i) s_vec[15 + i] = q.has_goal ? goalg[3 * b + i] : (R)0;
    s_vec[18] = want_clear ? clearance[b] : (R)0;
    *dmin = __builtin_nan("");
  }
  // ---- prologue 2, 3: the cycle kernel's d2 and eligibility
  if (swarm) {
    const R* own = snapA + (size_t)6 * b;
    const bool own_ok = six_finite(own, own + 3);
    for (int i = tid; i < M; i += NT) {
      const R* row = snapA + (size_t)6 * (base + i);
      d2[i] = (own_ok && i != self && six_finite(row, row + 3)) ? mate_d2(row, own) : __builtin_nan("");
    }
  }
  __syncthreads();
  // ---- prologue 3: rank by counting over (d2, index); sel[r] = the mate of rank r < Kn
  if (swarm) {
    for (int i = tid; i < M; i += NT) {
      const double di = d2[i];
      if (!(di == di)) continue;
      int rank = 0;
      for (int j = 0; j < M; ++j) {
        const double dj = d2[j];
        rank += (dj < di || (dj == di && j < i)) ? 1 : 0;
      }
      if (rank == 0) *dmin = di;
      if (rank < Kn) sel[rank] = i;
    }
    __syncthreads();
  }
  // ---- prologue 4: ranks are dense, so the filled slots are the first Kt; the whole workgroup copies the mates' intents into the slab
  int Kt = 0;
  for (int r = 0; r < Kn; ++r) Kt += sel[r] >= 0 ? 1 : 0;
  {
    const R r2 = (mate_radius + q.margin) * (mate_radius + q.margin);
    for (int i = tid; i < N * Kt; i += NT) {
      const int k = i / Kt, r = i - k * Kt;
      const R* src = intentA + ((size_t)(base + sel[r]) * N + k) * 3;
      R* dst = trk + (size_t)4 * i;
      dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2]; dst[3] = r2;
    }
  }

  // the planner's context as mppi_closed_loop_tracks_kernel builds it
  Ctx<R, true, true> c = load_ctx<R, true, true>(q, 1, 0, key0, key1, index_base + (uint32_t)b, s_vec, s_vec + 3, s_vec + 15, U, sph, Ks, w_obs);
  c.svel = svel;
  c.stime = stime;
  c.trk = trk;
  c.Kt = Kt;
  c.gl[0] = wave_bcast(c.gl[0], 0); c.gl[1] = wave_bcast(c.gl[1], 0); c.gl[2] = wave_bcast(c.gl[2], 0);

  // ---- the step times of this cycle's plan; the barrier publishes the slab too
  for (int k = tid; k < N; k += NT) stime[k] = (R)(sphere_t0 + plan_stamp((int)C, substeps, sim_dt, k, plan_dt));
  __syncthreads();
  // ---- plan
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
  // ---- act, in chunks of kPark steps; the clearance against the shared rows
  int s0 = 0;
  do {
    const int n = substeps - s0 < kPark ? substeps - s0 : kPark;
    if (tid == 0 && n > 0)
      fly_steps<R>(ctl, sim, d, N, n, sim_dt, [&](int step, const R* p) {
        if (want_clear) {
          park[4 * step] = p[0]; park[4 * step + 1] = p[1]; park[4 * step + 2] = p[2];
          park[4 * step + 3] = (R)(sphere_t0 + (double)((int)C * substeps + s0 + step + 1) * sim_dt);
        }
      });
    __syncthreads();
    if (want_clear && n > 0) clearance_chunk<R, true>(park, sph, rad, n, Ks, l.red, s_vec + 18, svel);
    s0 += kPark;
  } while (s0 < substeps);
  if (last && plan_last != nullptr)
    for (int r = tid; r < 3 * rows; r += NT) plan_last[(size_t)b * 3 * rows + r] = d.planP[r];
  if (last && neighbours != nullptr)
    for (int r = tid; r < Kn; r += NT) neighbours[(size_t)b * Kn + r] = sel[r] >= 0 ? base + sel[r] : -1;
  // ---- warm start of the next cycle
  shift_nominal(q, U, reinterpret_cast<R*>(l.acc), shift);

  for (int r = tid; r < rows; r += NT) Ug[(size_t)b * rows + r] = U[r];
  if (tid == 0) {
    drone_store<R>(d, b, posg, velg, attg, omegag, timeg, stateg);
    if (want_clear) clearance[b] = s_vec[18];
    if (swarm) {
      for (int i = 0; i < 6; ++i) snapB[(size_t)6 * b + i] = s_vec[i];
      // the intent of the next cycle: the shifted nominal from the state just stored
      swarm_intent_rows(q, s_vec, s_vec + 3, U, intentB + (size_t)b * rows);
      const double dm = *dmin;
      if (separation != nullptr && dm == dm) separation[b] = fmin(separation[b], (R)sqrt(dm));
    }
  }
}

// ---- host side
static size_t swarm_intent_workspace_bytes(int B, int horizon, int elem_size) {
  if (B < 0 || horizon < 1 || horizon > SE3MPC_MAX_HORIZON || (elem_size != 4 && elem_size != 8)) return 0;
  return (size_t)2 * (size_t)(6 + 3 * horizon) * (size_t)B * (size_t)elem_size;
}

template <typename R>
static int swarm_intent_impl(const se3mpc_params* p, int B, const R* pos, const R* vel, const R* U, R* intent, void* stream) {
  const char* fn = "se3mpc_swarm_intent";
  if (p == nullptr) return fail(SE3MPC_ERR_NULL, "params is NULL", fn);
  const int rc = check_params_impl(p);
  if (rc) return fail(rc, "invalid se3mpc_params", fn);
  if (B < 0) return fail(SE3MPC_ERR_SHAPE, "B < 0", fn);
  if (B == 0) return SE3MPC_OK;
  if (!pos || !vel || !U || !intent) return fail(SE3MPC_ERR_NULL, "NULL operand", fn);
  hipLaunchKernelGGL(swarm_intent_kernel<R>, dim3(grid_for(B, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, make_dev_params<R>(*p), B, pos, vel, U,
                     intent);
  return launch_status(fn);
}

template <typename R>
static int mppi_closed_loop_swarm_intent_impl(const se3mpc_params* p, const se3mpc_controller_params* cp, const se3mpc_simulator_params* sp, int B,
                                              int swarm_size, int neighbours_k, double mate_radius, int cycles, int substeps, double sim_dt,
                                              uint32_t cycle_base, int shift, int S, int iters, double sigma, double temperature, uint64_t seed,
                                              uint32_t iter_base, uint32_t index_base, const R* goal, const R* spheres, const R* sphere_vel,
                                              double sphere_t0, int K, double obstacle_weight, const R* wind, long long wind_stride, double* time,
                                              R* pos, R* vel, R* att, R* omega, double* state, R* U, R* cost, R* trace, R* plan_last, R* clearance,
                                              R* separation, int32_t* neighbours, void* workspace, size_t workspace_bytes, void* stream) {
  const char* fn = "se3mpc_mppi_closed_loop_swarm_intent";
  if (p == nullptr || cp == nullptr || sp == nullptr) return fail(SE3MPC_ERR_NULL, "NULL parameter struct", fn);
  int rc = check_params_impl(p);
  if (rc) return fail(rc, "invalid se3mpc_params", fn);
  rc = check_controller_params(cp);
  if (rc) return fail(rc, "invalid se3mpc_controller_params", fn);
  rc = check_simulator_params(sp);
  if (rc) return fail(rc, "invalid se3mpc_simulator_params", fn);
  if (cycles < 0 || substeps < 0) return fail(SE3MPC_ERR_SHAPE, "cycles or substeps < 0", fn);
  if (shift < 0 || shift > p->horizon) return fail(SE3MPC_ERR_SHAPE, "shift outside [0, horizon]", fn);
  if (wind != nullptr && !(wind_stride == 0 || wind_stride >= 3)) return fail(SE3MPC_ERR_SHAPE, "wind_stride must be 0 or >= 3", fn);
  rc = check_mppi_args(fn, p, B, B, S, iters, sigma, temperature, K, obstacle_weight);
  if (rc) return rc;
  if (!std::isfinite(sim_dt)) return fail(SE3MPC_ERR_PARAM, "sim_dt must be finite", fn);
  rc = check_moving_args(fn, K, sphere_vel, sphere_t0);
  if (rc) return rc;
  if (swarm_size < 1 || swarm_size > SE3MPC_MAX_SWARM) return fail(SE3MPC_ERR_SHAPE, "swarm_size outside [1, SE3MPC_MAX_SWARM]", fn);
  if (B % swarm_size != 0) return fail(SE3MPC_ERR_SHAPE, "B is not a multiple of swarm_size", fn);
  if (neighbours_k < 0 || neighbours_k > SE3MPC_MAX_TRACKS) return fail(SE3MPC_ERR_SHAPE, "neighbours_k outside [0, SE3MPC_MAX_TRACKS]", fn);
  if (K + neighbours_k > SE3MPC_MAX_SPHERES) return fail(SE3MPC_ERR_SHAPE, "K + neighbours_k > SE3MPC_MAX_SPHERES", fn);
  if (!(mate_radius >= 0.0) || !std::isfinite(mate_radius)) return fail(SE3MPC_ERR_PARAM, "mate_radius must be finite and >= 0", fn);
  if (swarm_size > 1 && workspace != nullptr && workspace_bytes < swarm_intent_workspace_bytes(B, p->horizon, (int)sizeof(R)))
    return fail(SE3MPC_ERR_SHAPE, "workspace_bytes < se3mpc_mppi_swarm_intent_workspace_bytes(B, horizon, elem_size)", fn);
  if (B == 0 || cycles == 0) return SE3MPC_OK;
  if (!time || !pos || !vel || !att || !omega || !state || !U || !cost || (p->has_goal && !goal) || (K > 0 && !spheres))
    return fail(SE3MPC_ERR_NULL, "NULL operand", fn);
  if (swarm_size > 1 && neighbours_k > 0 && (workspace == nullptr || separation == nullptr))
    return fail(SE3MPC_ERR_NULL, "NULL workspace or separation with swarm_size > 1 and neighbours_k > 0", fn);
  const bool swarm = swarm_size > 1 && workspace != nullptr && (neighbours_k > 0 || separation != nullptr);
  const int N = p->horizon;
  const DevParams<R> q = make_dev_params<R>(*p);
  R *snap[2] = {nullptr, nullptr}, *intent[2] = {nullptr, nullptr};
  if (swarm) {
    const size_t image = (size_t)(6 + 3 * N) * B;
    for (int i = 0; i < 2; ++i) {
      snap[i] = static_cast<R*>(workspace) + i * image;
      intent[i] = snap[i] + (size_t)6 * B;
    }
    hipLaunchKernelGGL(swarm_seed_kernel<R>, dim3(grid_for(6 * B, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, B, (const R*)pos, (const R*)vel,
                       snap[0]);
    hipLaunchKernelGGL(swarm_intent_kernel<R>, dim3(grid_for(B, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, q, B, (const R*)pos, (const R*)vel,
                       (const R*)U, intent[0]);
  }
  const int NT = S < kBlock ? S : kBlock;
  const TrackLds TL = track_lds_layout(swarm_lds_layout(N, K, NT / kWave, sizeof(R), swarm_size, neighbours_k).total, N, neighbours_k, sizeof(R));
  for (int cyc = 0; cyc < cycles; ++cyc)
    hipLaunchKernelGGL(mppi_swarm_intent_cycle_kernel<R>, dim3(B), dim3(NT), TL.total, (hipStream_t)stream, q, make_ctrl_dev<R>(*cp),
                       make_sim_dev<R>(*sp), p->dt, cycles, cyc, cyc == cycles - 1, substeps, sim_dt, cycle_base + (uint32_t)cyc, shift, S, iters,
                       (R)sigma, 1.0 / temperature, (uint32_t)seed, (uint32_t)(seed >> 32), iter_base, index_base, goal, spheres, sphere_vel,
                       sphere_t0, K, neighbours_k, swarm_size, (R)mate_radius, (R)obstacle_weight, wind, wind_stride, time, pos, vel, att, omega,
                       state, U, cost, trace, plan_last, clearance, separation, neighbours, (const R*)snap[cyc & 1], (const R*)intent[cyc & 1],
                       snap[(cyc + 1) & 1], intent[(cyc + 1) & 1]);
  return launch_status(fn);
}

}  // namespace mppi
}  // namespace se3mpc

using se3mpc::mppi::mppi_closed_loop_swarm_intent_impl;
using se3mpc::mppi::swarm_intent_impl;

extern "C" size_t se3mpc_mppi_swarm_intent_workspace_bytes(int B, int horizon, int elem_size) {
  return se3mpc::mppi::swarm_intent_workspace_bytes(B, horizon, elem_size);
}

extern "C" int se3mpc_swarm_intent_f32(const se3mpc_params* p, int B, const float* pos, const float* vel, const float* U, float* intent,
                                       void* stream) {
  return swarm_intent_impl<float>(p, B, pos, vel, U, intent, stream);
}
extern "C" int se3mpc_swarm_intent_f64(const se3mpc_params* p, int B, const double* pos, const double* vel, const double* U, double* intent,
                                       void* stream) {
  return swarm_intent_impl<double>(p, B, pos, vel, U, intent, stream);
}

extern "C" int se3mpc_mppi_closed_loop_swarm_intent_f32(const se3mpc_params* p, const se3mpc_controller_params* cp, const se3mpc_simulator_params* sp,
                                                        int B, int swarm_size, int neighbours_k, double mate_radius, int cycles, int substeps,
                                                        double sim_dt, uint32_t cycle_base, int shift, int S, int iters, double sigma,
                                                        double temperature, uint64_t seed, uint32_t iter_base, uint32_t index_base, const float* goal,
                                                        const float* spheres, const float* sphere_vel, double sphere_t0, int K,
                                                        double obstacle_weight, const float* wind, long long wind_stride, double* time, float* pos,
                                                        float* vel, float* att, float* omega, double* state, float* U, float* cost, float* trace,
                                                        float* plan_last, float* clearance, float* separation, int32_t* neighbours, void* workspace,
                                                        size_t workspace_bytes, void* stream) {
  return mppi_closed_loop_swarm_intent_impl<float>(p, cp, sp, B, swarm_size, neighbours_k, mate_radius, cycles, substeps, sim_dt, cycle_base, shift, S,
                                                   iters, sigma, temperature, seed, iter_base, index_base, goal, spheres, sphere_vel, sphere_t0, K,
                                                   obstacle_weight, wind, wind_stride, time, pos, vel, att, omega, state, U, cost, trace, plan_last,
                                                   clearance, separation, neighbours, workspace, workspace_bytes, stream);
}
extern "C" int se3mpc_mppi_closed_loop_swarm_intent_f64(const se3mpc_params* p, const se3mpc_controller_params* cp, const se3mpc_simulator_params* sp,
                                                        int B, int swarm_size, int neighbours_k, double mate_radius, int cycles, int substeps,
                                                        double sim_dt, uint32_t cycle_base, int shift, int S, int iters, double sigma,
                                                        double temperature, uint64_t seed, uint32_t iter_base, uint32_t index_base,
                                                        const double* goal, const double* spheres, const double* sphere_vel, double sphere_t0, int K,
                                                        double obstacle_weight, const double* wind, long long wind_stride, double* time, double* pos,
                                                        double* vel, double* att, double* omega, double* state, double* U, double* cost,
                                                        double* trace, double* plan_last, double* clearance, double* separation,
                                                        int32_t* neighbours, void* workspace, size_t workspace_bytes, void* stream) {
  return mppi_closed_loop_swarm_intent_impl<double>(p, cp, sp, B, swarm_size, neighbours_k, mate_radius, cycles, substeps, sim_dt, cycle_base, shift, S,
                                                    iters, sigma, temperature, seed, iter_base, index_base, goal, spheres, sphere_vel, sphere_t0, K,
                                                    obstacle_weight, wind, wind_stride, time, pos, vel, att, omega, state, U, cost, trace, plan_last,
                                                    clearance, separation, neighbours, workspace, workspace_bytes, stream);
}
