// rollout_obstacles.hip -- the rollout fused with the sphere-obstacle residuals on the rolled-out positions (se3mpc_rollout_obstacles_*,
// BASELINE config 3).  The per-axis sweeps are rollout_device.hpp's; the residual sweeps (packed VALU, matrix core) are here.
#include "lane_common.hpp"
#include "rollout_device.hpp"

namespace se3mpc {

// Sphere residuals of one wavefront's share of the steps (k = w, w+W, ...) against the LDS-resident table.
// The spheres are walked in register chunks of 8: one chunk is fetched once (broadcast LDS reads) and then
// swept over all of the wavefront's steps, so the inner loop costs 3 LDS reads per 8 evaluations instead of a
// 16-byte read per evaluation, and nothing in it waits on LDS.  f32 evaluates two spheres per instruction
// (v_pk_add/mul/fma_f32).  The table is padded to a multiple of 8 with (0, 0, 0, -inf): residual +inf.
constexpr int kSphereChunk = 8;

template <typename R>
__device__ __forceinline__ void obstacle_sweep(const R* __restrict__ tile, const R* __restrict__ sph, int Nn, int Kpad, int kbeg,
                                               int kend, int kstep, int lane, R& mn_io, R& vs_io) {
  // steps kbeg, kbeg + kstep, ... < kend; the minimum and the violation sum ACCUMULATE into mn_io / vs_io (start: +inf, 0)
  R mn = mn_io;
  if constexpr (kObsPacked<R>) {
    typedef float f2 __attribute__((vector_size(8)));
    f2 vs2 = {0.0f, 0.0f};
    for (int j0 = 0; j0 < Kpad; j0 += kSphereChunk) {
      f2 cx[kSphereChunk / 2], cy[kSphereChunk / 2], cz[kSphereChunk / 2], r2[kSphereChunk / 2];
#pragma unroll
      for (int jj = 0; jj < kSphereChunk / 2; ++jj) {
        const R* s0 = sph + 4 * (j0 + 2 * jj);
        cx[jj] = f2{s0[0], s0[4]}; cy[jj] = f2{s0[1], s0[5]}; cz[jj] = f2{s0[2], s0[6]}; r2[jj] = f2{s0[3], s0[7]};
      }
#pragma unroll 2
      for (int k = kbeg; k < kend; k += kstep) {
        const float px = tile[((size_t)0 * Nn + k) * kWave + lane], py = tile[((size_t)1 * Nn + k) * kWave + lane],
                    pz = tile[((size_t)2 * Nn + k) * kWave + lane];
        const f2 px2 = {px, px}, py2 = {py, py}, pz2 = {pz, pz};
#pragma unroll
        for (int jj = 0; jj < kSphereChunk / 2; ++jj) {
          const f2 dx = px2 - cx[jj], dy = py2 - cy[jj], dz = pz2 - cz[jj];
          const f2 cj = dz * dz + (dy * dy + (dx * dx - r2[jj]));          // three fused multiply-adds (padding rows: r2 = -inf, residual +inf)
          mn = __builtin_fminf(__builtin_fminf(mn, cj[0]), cj[1]);          // one v_min3_f32
          vs2 += f2{fmaxf(0.0f, -cj[0]), fmaxf(0.0f, -cj[1])};
        }
      }
    }
    vs_io += vs2[0] + vs2[1];
  } else {
    R vs = (R)0;
    for (int j0 = 0; j0 < Kpad; j0 += kSphereChunk) {
      R cx[kSphereChunk], cy[kSphereChunk], cz[kSphereChunk], r2[kSphereChunk];
#pragma unroll
      for (int jj = 0; jj < kSphereChunk; ++jj) {
        const R* s0 = sph + 4 * (j0 + jj);
        cx[jj] = s0[0]; cy[jj] = s0[1]; cz[jj] = s0[2]; r2[jj] = s0[3];
      }
      for (int k = kbeg; k < kend; k += kstep) {
        const R px = tile[((size_t)0 * Nn + k) * kWave + lane], py = tile[((size_t)1 * Nn + k) * kWave + lane],
                pz = tile[((size_t)2 * Nn + k) * kWave + lane];
#pragma unroll
        for (int jj = 0; jj < kSphereChunk; ++jj) {
          const R dx = px - cx[jj], dy = py - cy[jj], dz = pz - cz[jj];
          const R cj = dz * dz + (dy * dy + (dx * dx - r2[jj]));
          mn = fmin(mn, cj);
          vs += fmax((R)0, -cj);
        }
      }
    }
    vs_io += vs;
  }
  mn_io = mn;
}

// The same residuals on the matrix core (float32).  |P_k - c_j|^2 - R_j^2 = |P_k|^2 - 2 P_k.c_j + (|c_j|^2 - R_j^2) is a K = 4 contraction of
// (P_k, |P_k|^2) with (-2 c_j, 1) plus a per-sphere constant (P_k and c_j both taken about the table's mean centre, see obstacle_sweep_mfma): ONE v_mfma_f32_16x16x4_f32 forms the residuals of 16 spheres x 16 trajectories at a
// step, the constant riding in as the accumulator input.  A = the sphere chunk (one register per 16 spheres, loop-invariant), C-in = four
// constants per lane, B = a row of the position tile exactly as the forward sweep stored it ([axis][k][trajectory]: lanes 0-47 read x / y / z of
// 16 consecutive trajectories, lanes 48-63 the |P_k|^2 row this wavefront has just written behind the three axes) -- no transposed image.
// What is left for the VALU is the fold: two v_min3 and the violation sum per four residuals, running per lane = (trajectory l % 16 of the block,
// spheres 4 (l / 16) ... + 3) across all steps; the four lane groups meet once at the end (obstacle_mfma_fold).  Against the packed-VALU sweep
// (10 instructions per sphere pair) this issues 8 VALU instructions + 1 MFMA per 64 residuals-per-16-lanes, i.e. 2.25 instead of 5 per residual
// and lane, and the multiplies run beside them on the matrix pipe.  Price: the expanded form cancels, |P - o|^2 + |c - o|^2 (a few 1e2 m^2 for a
// table 15 m across) against a residual near 0 at an obstacle's surface: float32 absolute error ~ 2e-5 m^2 there where the difference form had
// 1e-6.  (Taken about the world's origin the same cancellation grew with the scene's distance from it: 2.4e-4 on a violation of 4.8 m^2 with
// positions 20 m out, past the suite's bound on the violation once a small safety margin made the violations shallow.)
// MEASURED (MI355X, profiles/r03g_cfg3_mfma_vs_valu.txt): 64 x 8192 x horizon 50 x 16 spheres 163.4 us against 166.0 us for the packed-VALU sweep,
// 1 M rollouts 330 against 336 us, the bench's ring of batches 164.4 against 161.9 us, one 8192-rollout launch 8.74 against 8.43 us -- the
// kernel is bound by its load latency at two workgroups per CU, not by VALU issue (64 % busy), so halving the evaluation's instructions buys
// nothing that pays for the precision.  The difference form on the VALU stays the default; se3mpc_set_rollout_variant(+2048) selects this one
// (float32 only; float64 always takes the VALU form).
// min(d, 0) through the integer minimum of the bit pattern (see obstacle_sweep_mfma)
__device__ __forceinline__ float relu_neg_bits(float d) {
  const int i = __float_as_int(d);
  return __int_as_float(i < 0 ? i : 0);
}
struct ObsMfmaAcc {
  float mn[4];
  obs_f2 vs[4];
};
__device__ __forceinline__ void obstacle_mfma_init(ObsMfmaAcc& acc) {
#pragma unroll
  for (int tb = 0; tb < 4; ++tb) { acc.mn[tb] = INFINITY; acc.vs[tb] = obs_f2{0.0f, 0.0f}; }
}
__device__ __forceinline__ void obstacle_sweep_mfma(float* __restrict__ tile, const float* __restrict__ sph, int Nn, int K, int Kpad, int kbeg,
                                                    int kend, int kstep, int lane, ObsMfmaAcc& acc) {
  const int li = lane & 15, lk = lane >> 4;
  if (Kpad <= 0 || K <= 0) return;
  float* pprow = tile + (size_t)3 * Nn * kWave;                                    // [Nn][64]: |P_k - o|^2, the tile's fourth "axis"
  // The expanded form cancels in proportion to |P|^2 + |c|^2, and |P - c| does not depend on the origin: positions and centres are taken
  // about o = the mean of the table's centres (padding rows are (0, 0, 0); every lane forms the same sums in the same order), so that what
  // cancels next to an obstacle is the table's own extent, not its distance from the world's origin.
  float ox = 0.0f, oy = 0.0f, oz = 0.0f;
  for (int j = 0; j < Kpad; ++j) { ox += sph[4 * j + 0]; oy += sph[4 * j + 1]; oz += sph[4 * j + 2]; }
  { const float inv = 1.0f / (float)K; ox *= inv; oy *= inv; oz *= inv; }
  const float ob = lk == 0 ? ox : (lk == 1 ? oy : (lk == 2 ? oz : 0.0f));         // this lane group's component of o (the |P - o|^2 row: none)
  // this wavefront owns steps kbeg, kbeg + kstep, ...: their |P_k|^2 rows first (read back across lanes below)
  for (int k = kbeg; k < kend; k += kstep) {
    const float px = tile[((size_t)0 * Nn + k) * kWave + lane] - ox, py = tile[((size_t)1 * Nn + k) * kWave + lane] - oy,
                pz = tile[((size_t)2 * Nn + k) * kWave + lane] - oz;
    pprow[(size_t)k * kWave + lane] = px * px + (py * py + pz * pz);
  }
  group_sync<kWave>();
  for (int j0 = 0; j0 < Kpad; j0 += 16) {
    const float* sa = sph + 4 * (j0 + li);
    const float a = lk < 3 ? -2.0f * (sa[lk] - ob) : 1.0f;                         // A[sphere li][component lk]
    vf4 w;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float* sw = sph + 4 * (j0 + 4 * lk + r);
      const float cx = sw[0] - ox, cy = sw[1] - oy, cz = sw[2] - oz;
      w[r] = (cx * cx + (cy * cy + cz * cz)) - sw[3];                             // |c - o|^2 - R^2; a padding row (0, 0, 0, -inf) gives +inf
    }
#pragma unroll 2
    for (int k = kbeg; k < kend; k += kstep) {
      const float* brow = tile + ((size_t)lk * Nn + k) * kWave + li;               // lk = 3: the |P_k|^2 row
      // the four trajectory blocks of a step: operands, then four independent matrix-core instructions, then the folds
      float b[4];
      vf4 d[4];
#pragma unroll
      for (int tb = 0; tb < 4; ++tb) b[tb] = brow[16 * tb] - ob;
#pragma unroll
      for (int tb = 0; tb < 4; ++tb) d[tb] = mfma_16x16x4_f32(a, b[tb], w);
#pragma unroll
      for (int tb = 0; tb < 4; ++tb) {
        acc.mn[tb] = __builtin_fminf(__builtin_fminf(acc.mn[tb], d[tb][0]), d[tb][1]);
        acc.mn[tb] = __builtin_fminf(__builtin_fminf(acc.mn[tb], d[tb][2]), d[tb][3]);
        // violation: max(0, -d) = -min(d, 0), the minimum taken on the bit patterns (a negative float is a negative integer, a positive one
        // positive): ONE v_min_i32 per residual, the sign folded into the packed add -- fmaxf on a matrix-core result costs a canonicalising
        // v_max first.  (A NaN residual -- non-finite positions -- with its sign bit set reaches the sum; with the bit clear it counts 0.)
        acc.vs[tb] -= obs_f2{relu_neg_bits(d[tb][0]), relu_neg_bits(d[tb][1])};
        acc.vs[tb] -= obs_f2{relu_neg_bits(d[tb][2]), relu_neg_bits(d[tb][3])};
      }
    }
  }
}
// the four lane groups (sphere quarters) of every trajectory meet; lane l leaves with the totals of trajectory l
__device__ __forceinline__ void obstacle_mfma_fold(const ObsMfmaAcc& acc, int lane, float& mn_out, float& vs_out) {
  const int lk = lane >> 4;
  float mn = INFINITY, vs = 0.0f;
#pragma unroll
  for (int tb = 0; tb < 4; ++tb) {
    float m = acc.mn[tb], v = acc.vs[tb][0] + acc.vs[tb][1];
    m = __builtin_fminf(m, wave_xor(m, 16)); v = v + wave_xor(v, 16);
    m = __builtin_fminf(m, wave_xor(m, 32)); v = v + wave_xor(v, 32);
    mn = lk == tb ? m : mn; vs = lk == tb ? v : vs;
  }
  mn_out = mn; vs_out = vs;
}

// Rollout fused with the sphere-obstacle residuals of planner.py:499-514 on the ROLLED-OUT positions
// (BASELINE.json config 3: horizon 50, K = 16 spheres from the mapper).  The forward sweep of each axis
// wavefront stages its positions as a per-step tile in LDS ([axis][k][lane], bank = lane: conflict free);
// after the barrier the W wavefronts of the workgroup split the steps (k = w, w+W, ...) and evaluate
// |P_k - c_j|^2 - (r_j + margin)^2 against the LDS-resident sphere table, keeping the minimum residual and
// the summed violation per trajectory.  Neither the states nor the N*K residuals ever touch HBM:
// 4*(6N+12) B per rollout instead of 4*(6N+10) + 4*(3N) written + 4*(3N) re-read for the unfused pair.
// W = 3: the axis wavefronts do everything (saturating batches).  W > 3: W - 3 helper wavefronts put the sphere table into
// LDS while the axis wavefronts roll out, all meet at a barrier BETWEEN the forward and the adjoint sweep (the position tile is
// complete there), and the helpers evaluate the first `kh` steps while the axis wavefronts run the adjoint sweep and store the
// gradient; the remaining steps are split over all W wavefronts.  kh balances the helpers' head start against the adjoint sweep
// (measured per-step costs, see where it is formed): with five helpers and 16 spheres they take most of the steps.  MF: the residuals on the
// matrix core (obstacle_sweep_mfma; float32, se3mpc_set_rollout_variant(+2048)) instead of the packed-VALU difference form.
// W = 8 for batches that leave SIMDs idle (8192 rollouts = 128 workgroups: the evaluation leaves the critical path), W = 4 where
// the register sweep leaves a CU's fourth pair of wavefront slots empty.
template <typename R, int N, bool REG, bool GRAD, int W, bool MF = false>
__global__ void __launch_bounds__(64 * W)
rollout_obstacles_kernel(DevParams<R> q, int B, int ld, const R* __restrict__ p0, const R* __restrict__ v0,
                         const R* __restrict__ goal, const R* __restrict__ T, R* __restrict__ cost,
                         R* __restrict__ gradT, const R* __restrict__ spheres, int K, R* __restrict__ cmin,
                         R* __restrict__ viol, unsigned long long* __restrict__ key, uint32_t index_base) {
  HIP_DYNAMIC_SHARED(unsigned char, lds_raw)
  {                                                         // blockIdx.y = batch of a multi-batch launch (as rollout_kernel)
    const size_t bi = blockIdx.y, ss = (size_t)3 * ld, st = (size_t)3 * q.N * ld;
    p0 += bi * ss; v0 += bi * ss; T += bi * st; cost += bi * (size_t)ld;
    if (goal != nullptr) goal += bi * ss;
    if (GRAD) gradT += bi * st;
    if (cmin != nullptr) cmin += bi * (size_t)ld;
    if (viol != nullptr) viol += bi * (size_t)ld;
    if (key != nullptr) key += bi * (size_t)gridDim.x;
  }
  static_assert(!MF || sizeof(R) == 4, "the matrix-core sweep is float32");
  constexpr int kChunk = MF ? 16 : kSphereChunk;            // MF: residuals on the matrix core, 16 spheres per instruction (obstacle_sweep_mfma)
  const int Kpad = (K + kChunk - 1) / kChunk * kChunk;
  R* tile = reinterpret_cast<R*>(lds_raw);                  // [3][N][64]; MF: [4][N][64], the fourth block = |P_k|^2
  R* sph = tile + (size_t)(MF ? 4 : 3) * q.N * kWave;        // [Kpad][4] = (cx, cy, cz, (r + margin)^2)
  R* part = sph + (size_t)4 * Kpad;                          // [3 + 2W][64]: axis costs, then min residual / violation per wave
  constexpr bool MID = W > 3;                               // helper wavefronts exist: barrier between the sweeps (see above)
  constexpr int NH = MID ? W - 3 : 1;
  // W = 3: the sphere table is fetched into registers now and written to LDS after the rollout: its HBM latency hides
  // behind the rollout's own loads instead of preceding them (K <= 256, 192 threads: at most two rows each)
  constexpr int kRowsPerThread = (SE3MPC_MAX_SPHERES + 64 * W - 1) / (64 * W);
  R srow[kRowsPerThread][4];
  if constexpr (!MID) {
#pragma unroll
    for (int t = 0; t < kRowsPerThread; ++t) {
      const int i = threadIdx.x + t * 64 * W;
      srow[t][0] = (R)0; srow[t][1] = (R)0; srow[t][2] = (R)0; srow[t][3] = (R)0;
      if (i < K) { srow[t][0] = spheres[4 * i + 0]; srow[t][1] = spheres[4 * i + 1]; srow[t][2] = spheres[4 * i + 2]; srow[t][3] = spheres[4 * i + 3]; }
    }
  }
  int blk = blockIdx.x;
  if ((gridDim.x & 7) == 0) blk = (blk & 7) * (gridDim.x >> 3) + (blk >> 3);
  const int lane = threadIdx.x & (kWave - 1);
  const int b0 = blk * kWave + lane;
  const bool live = b0 < B;
  const int b = live ? b0 : B - 1;
  const unsigned voff = (unsigned)b * (unsigned)sizeof(R), rowb = (unsigned)ld * (unsigned)sizeof(R);
  const int a = wave_uniform((int)(threadIdx.x / kWave));
  const int Nn = q.N;
  if (a < 3) {
    R* my_tile = tile + (size_t)a * Nn * kWave + lane;
    R c;
    if constexpr (REG) c = rollout_axis_reg<R, N, GRAD, false, 2, 2, true, true, MID>(q, a, voff, rowb, p0, v0, goal, T, gradT, nullptr, nullptr, my_tile);
    else c = rollout_axis_rev<R, GRAD, false, 2, true, MID>(q, a, voff, rowb, p0, v0, goal, T, gradT, nullptr, nullptr, my_tile);
    part[a * kWave + lane] = c;
  } else if constexpr (MID) {
    // helper wavefronts: the sphere table, then the barrier the axis wavefronts reach after their forward sweep
    for (int i = (int)threadIdx.x - 3 * kWave; i < Kpad; i += NH * kWave) {
      R s0 = (R)0, s1 = (R)0, s2 = (R)0, s3 = (R)-INFINITY;
      if (i < K) {
        s0 = spheres[4 * i + 0]; s1 = spheres[4 * i + 1]; s2 = spheres[4 * i + 2];
        const R sm = spheres[4 * i + 3] + q.margin;
        s3 = sm * sm;
      }
      sph[4 * i + 0] = s0; sph[4 * i + 1] = s1; sph[4 * i + 2] = s2; sph[4 * i + 3] = s3;
    }
    __syncthreads();
  }
  R mn = INFINITY, vs = (R)0;
  if constexpr (!MID) {
#pragma unroll
    for (int t = 0; t < kRowsPerThread; ++t) {
      const int i = threadIdx.x + t * 64 * W;
      if (i < Kpad) {
        const R sm = srow[t][3] + q.margin;
        sph[4 * i + 0] = srow[t][0]; sph[4 * i + 1] = srow[t][1]; sph[4 * i + 2] = srow[t][2];
        sph[4 * i + 3] = i < K ? sm * sm : (R)-INFINITY;
      }
    }
    __syncthreads();
    if constexpr (MF) {
      ObsMfmaAcc acc;
      obstacle_mfma_init(acc);
      obstacle_sweep_mfma(tile, sph, Nn, K, Kpad, a, Nn, W, lane, acc);
      obstacle_mfma_fold(acc, lane, mn, vs);
    } else {
      obstacle_sweep<R>(tile, sph, Nn, Kpad, a, Nn, W, lane, mn, vs);
    }
  } else {
    // steps [0, kh): the helpers alone, during the adjoint sweep; steps [kh, N): all W wavefronts.  The adjoint sweep costs an axis wavefront
    // ~48 cycles per step; a step's residuals cost ~9 cycles per sphere on the matrix core (150 per 16 spheres), ~20 on the VALU (320):
    // the head start covers 5 N / Kpad steps per helper there, 2.5 N / Kpad here
    const int khb = Kpad > 0 ? (NH * (MF ? 10 : 5) * Nn) / (2 * Kpad) : Nn;
    const int kh = khb < Nn ? khb : Nn;
    if constexpr (MF) {
      ObsMfmaAcc acc;
      obstacle_mfma_init(acc);
      if (a >= 3) obstacle_sweep_mfma(tile, sph, Nn, K, Kpad, a - 3, kh, NH, lane, acc);
      obstacle_sweep_mfma(tile, sph, Nn, K, Kpad, kh + a, Nn, W, lane, acc);
      obstacle_mfma_fold(acc, lane, mn, vs);
    } else {
      if (a >= 3) obstacle_sweep<R>(tile, sph, Nn, Kpad, a - 3, kh, NH, lane, mn, vs);
      obstacle_sweep<R>(tile, sph, Nn, Kpad, kh + a, Nn, W, lane, mn, vs);
    }
  }
  part[(3 + a) * kWave + lane] = mn;
  part[(3 + W + a) * kWave + lane] = vs;
  __syncthreads();
  if (a == 0) {
    const R total = part[0 * kWave + lane] + part[1 * kWave + lane] + part[2 * kWave + lane];
    if (live) {
      R m = part[3 * kWave + lane], v = part[(3 + W) * kWave + lane];
#pragma unroll
      for (int w = 1; w < W; ++w) { m = fmin(m, part[(3 + w) * kWave + lane]); v += part[(3 + W + w) * kWave + lane]; }
      if (cmin != nullptr) cmin[b] = m;
      if (viol != nullptr) viol[b] = v;
    }
    rollout_epilogue<R>(live, b, total, cost, key != nullptr ? key + blk : nullptr, index_base);
  }
}

template <typename R>
int rollout_obstacles_impl(const se3mpc_params* p, int B, int ld, const R* p0, const R* v0, const R* goal, const R* T,
                           R* cost, R* gradT, const R* spheres, int K, R* cmin, R* viol, uint64_t* key64, uint32_t index_base,
                           int nbatch, void* stream) {
  if (K < 0 || K > SE3MPC_MAX_SPHERES || nbatch < 1 || nbatch > 65535) return SE3MPC_ERR_SHAPE;
  int rc = check_lane_args(p, B, ld, p ? 3LL * p->horizon : 0, sizeof(R));
  if (rc) return rc;
  if (B == 0) return SE3MPC_OK;
  if (!p0 || !v0 || !T || !cost || (p->has_goal && !goal) || (K > 0 && !spheres)) return SE3MPC_ERR_NULL;
  unsigned long long* key = reinterpret_cast<unsigned long long*>(key64);
  const DevParams<R> q = make_dev_params<R>(*p);
  const int N = p->horizon, nblk = grid_for(B, kWave);
  const int Kpad = (K + kSphereChunk - 1) / kSphereChunk * kSphereChunk;
  // 8 wavefronts per workgroup while that still leaves SIMDs idle (the chip holds 1024 single-wave slots
  // before any wavefront has to share a SIMD), 3 otherwise; se3mpc_set_rollout_variant(+128 / +256) forces 3 / 8
  const int wsel = (g_lane_tuning.rollout_variant >> 7) & 3;
  const bool wide = wsel == 2 || (wsel == 0 && (long long)nblk * nbatch * 8 <= 1024);
  hipStream_t s = (hipStream_t)stream;
  // se3mpc_set_rollout_variant(3): the register-light reversible sweep, as for the plain rollout
  const SweepRoute route = (g_lane_tuning.rollout_variant & 127) == 3 ? kSweepRev : kSweepAuto;
  dispatch_horizon<R, false>(N, route, [&](auto sweep) {
    using S = decltype(sweep);
    // 3 axis wavefronts + 1 helper for the exact-N = 50 register sweep: at its 2 wavefronts per SIMD a CU has 8 slots, which two
    // 3-wavefront workgroups leave a quarter empty (64 x 8192, warm: 166 -> 161 us; shorter horizons hold 3 per SIMD and lose 3 % with
    // a helper: profiles/r03f_cfg3_workgroup_shapes.txt); se3mpc_set_rollout_variant(+384) forces it
    const bool four = wsel == 3 || (wsel == 0 && !wide && S::REG && N == 50);
    const int W = wide ? 8 : (four ? 4 : 3);
    // se3mpc_set_rollout_variant(+2048), float32: the residuals on the matrix core (obstacle_sweep_mfma: a fourth tile block for |P_k|^2, the
    // table padded to 16) unless the larger LDS image would pass 64 KiB.  Not the default: measured equal to the packed-VALU difference form
    // within 2 % either way (profiles/r03g_cfg3_mfma_vs_valu.txt) at four decimal digits less next to an obstacle's surface
    const int Kpad16 = (K + 15) / 16 * 16;
    const size_t lds_mf = ((size_t)4 * N * kWave + (size_t)4 * Kpad16 + (size_t)(3 + 2 * W) * kWave) * sizeof(R);
    const bool mf = sizeof(R) == 4 && g_lane_tuning.obs_mfma && K > 0 && lds_mf <= 64 * 1024;
    const size_t lds = mf ? lds_mf : ((size_t)3 * N * kWave + (size_t)4 * Kpad + (size_t)(3 + 2 * W) * kWave) * sizeof(R);
    auto launch = [&](auto grad, auto w, auto mfk) {
      constexpr int WW = decltype(w)::value;
      hipLaunchKernelGGL((rollout_obstacles_kernel<R, S::NN, S::REG, decltype(grad)::value, WW, decltype(mfk)::value>), dim3(nblk, nbatch),
                         dim3(64 * WW), lds, s, q, B, ld, p0, v0, goal, T, cost, gradT, spheres, K, cmin, viol, key, index_base);
    };
    auto by_mf = [&](auto grad, auto w) {
      if constexpr (sizeof(R) == 4) {
        if (mf) return launch(grad, w, std::true_type{});
      }
      launch(grad, w, std::false_type{});
    };
    auto by_w = [&](auto grad) {
      if (wide) by_mf(grad, std::integral_constant<int, 8>{});
      else if (four) by_mf(grad, std::integral_constant<int, 4>{});
      else by_mf(grad, std::integral_constant<int, 3>{});
    };
    if (gradT != nullptr) by_w(std::true_type{}); else by_w(std::false_type{});
  });
  return launch_status("se3mpc_rollout_obstacles");
}

}  // namespace se3mpc

using namespace se3mpc;   // C ABI (include/se3mpc.h)

extern "C" int se3mpc_rollout_obstacles_f32(const se3mpc_params* p, int B, int ld, const float* p0, const float* v0, const float* goal,
                                            const float* T, float* cost, float* gradT, const float* spheres, int K, float* cmin, float* viol,
                                            uint64_t* wave_keys, uint32_t index_base, void* stream) {
  return rollout_obstacles_impl<float>(p, B, ld, p0, v0, goal, T, cost, gradT, spheres, K, cmin, viol, wave_keys, index_base, 1, stream);
}
extern "C" int se3mpc_rollout_obstacles_f64(const se3mpc_params* p, int B, int ld, const double* p0, const double* v0, const double* goal,
                                            const double* T, double* cost, double* gradT, const double* spheres, int K, double* cmin, double* viol,
                                            uint64_t* wave_keys, uint32_t index_base, void* stream) {
  return rollout_obstacles_impl<double>(p, B, ld, p0, v0, goal, T, cost, gradT, spheres, K, cmin, viol, wave_keys, index_base, 1, stream);
}
extern "C" int se3mpc_rollout_obstacles_batched_f32(const se3mpc_params* p, int B, int ld, int nbatch, const float* p0, const float* v0,
                                                    const float* goal, const float* T, float* cost, float* gradT, const float* spheres, int K,
                                                    float* cmin, float* viol, uint64_t* wave_keys, uint32_t index_base, void* stream) {
  return rollout_obstacles_impl<float>(p, B, ld, p0, v0, goal, T, cost, gradT, spheres, K, cmin, viol, wave_keys, index_base, nbatch, stream);
}
extern "C" int se3mpc_rollout_obstacles_batched_f64(const se3mpc_params* p, int B, int ld, int nbatch, const double* p0, const double* v0,
                                                    const double* goal, const double* T, double* cost, double* gradT, const double* spheres, int K,
                                                    double* cmin, double* viol, uint64_t* wave_keys, uint32_t index_base, void* stream) {
  return rollout_obstacles_impl<double>(p, B, ld, p0, v0, goal, T, cost, gradT, spheres, K, cmin, viol, wave_keys, index_base, nbatch, stream);
}
