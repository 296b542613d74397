// reduce_kernels.hip -- reductions and utilities around the lane-layout kernels: batch argmin and wave-key fold, population sums, the
// one-wavefront tail of a shooting-form plan, occupancy grid -> sphere table, transposes.
#include "lane_common.hpp"
#include "rollout_device.hpp"   // shooting_finish_kernel rolls the winner out with the rollout's own sums and constants

namespace se3mpc {

// ------------------------------------------------------------------------------------------
// Batch argmin -> packed 64-bit key (orderable cost bits << 32 | global index)
// ------------------------------------------------------------------------------------------
template <typename R>
__global__ void __launch_bounds__(256)
argmin_kernel(int B, const R* __restrict__ cost, uint32_t index_base, unsigned long long* __restrict__ key) {
  __shared__ unsigned long long wave_min[4];
  unsigned long long best = ~0ull;
  for (int b = blockIdx.x * blockDim.x + threadIdx.x; b < B; b += gridDim.x * blockDim.x) {
    const unsigned long long k = ((unsigned long long)orderable_bits((float)cost[b]) << 32) | (unsigned long long)(index_base + (uint32_t)b);
    best = k < best ? k : best;
  }
  // wavefront shuffle reduction (64 lanes)
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_down(best, off, kWave);
    best = o < best ? o : best;
  }
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  if (lane == 0) wave_min[wave] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long m = wave_min[0];
    for (int w = 1; w < (int)(blockDim.x / kWave); ++w) m = wave_min[w] < m ? wave_min[w] : m;
    atomicMin(key, m);
  }
}

// Population sums of a lane-layout block: part[split][r] = sum over the split's trajectories of w_b * X[r][b]
// (r < rows) and part[split][rows] = sum of w_b, in float64.  w_b = 1, or the MPPI weight
// exp(-(cost_b - cost_ref) / temperature).  One workgroup per (row, split); a fixed summation tree (lane-strided
// partials, DPP wave sum, four wave totals in order), so the result does not depend on scheduling.
template <typename R>
__global__ void __launch_bounds__(256)
population_sums_kernel(int rows, int B, int ld, const R* __restrict__ X, const R* __restrict__ cost, double cost_ref,
                       const unsigned long long* __restrict__ ref_key, double inv_temperature, int per_split,
                       double* __restrict__ part) {
  __shared__ double wave_tot[4];
  const int r = blockIdx.x, split = blockIdx.y;
  const int lo = split * per_split, hi = (lo + per_split < B) ? lo + per_split : B;
  if (ref_key != nullptr) {
    uint32_t u = (uint32_t)(ref_key[0] >> 32);
    u = (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u;               // se3mpc_key_cost
    cost_ref = (double)__uint_as_float(u);
  }
  const R* row = r < rows ? X + (size_t)r * ld : nullptr;
  double acc = 0.0;
  for (int b = lo + threadIdx.x; b < hi; b += blockDim.x) {
    const double w = cost != nullptr ? exp(-((double)cost[b] - cost_ref) * inv_temperature) : 1.0;
    acc += row != nullptr ? w * (double)row[b] : w;
  }
  acc = wave_sum(acc);
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  if (lane == 0) wave_tot[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[(size_t)split * (rows + 1) + r] = ((wave_tot[0] + wave_tot[1]) + wave_tot[2]) + wave_tot[3];
}

__global__ void __launch_bounds__(256)
population_fold_kernel(int n, int nsplit, const double* __restrict__ part, double* __restrict__ out) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  double acc = 0.0;
  for (int sp = 0; sp < nsplit; ++sp) acc += part[(size_t)sp * n + r];
  out[r] = acc;
}

// keys_out[batch] = min over the batch's wave-key slots (one workgroup per batch, plain store)
__global__ void __launch_bounds__(256)
reduce_keys_kernel(const unsigned long long* __restrict__ wave_keys, int per_batch, unsigned long long* __restrict__ keys_out) {
  __shared__ unsigned long long wave_min[4];
  const unsigned long long* src = wave_keys + (size_t)blockIdx.x * per_batch;
  unsigned long long best = ~0ull;
  for (int i = threadIdx.x; i < per_batch; i += blockDim.x) best = src[i] < best ? src[i] : best;
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_down(best, off, kWave);
    best = o < best ? o : best;
  }
  if ((threadIdx.x & (kWave - 1)) == 0) wave_min[threadIdx.x / kWave] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long m = wave_min[0];
    for (int w = 1; w < 4; ++w) m = wave_min[w] < m ? wave_min[w] : m;
    keys_out[blockIdx.x] = m;
  }
}

// ------------------------------------------------------------------------------------------
// The tail of a shooting-form plan in ONE wavefront (what SE3MPCPlanner.plan_shooting did with reduce_keys -> index_select -> cast ->
// rollout with states -> extract -> pack -> two copies, a dozen graph nodes for ~10 us of work): fold the wave keys of the descent launch,
// take the winner's thrust column (IO type -> double), roll it out with states and cost (the recurrence of planner.py:449-460, the
// objective of :516-550), extract accelerations / attitudes / body rates / thrust magnitudes (:582-654, lane = step, the previous valid
// frame fetched from its lane as in the solver's epilogue), optionally the sphere penalty left at the winner, and write the packed
// result -- `out` may be host-mapped pinned memory, the stores then ARE the copy back.
// out: [P (N x 3) | V (N x 3) | T (N x 3) | acc (N x 3) | att (N x 3) | rates (N x 3) | thrust (N) | cost | penalty | cost + penalty].
// ------------------------------------------------------------------------------------------
template <typename IO>
__global__ void __launch_bounds__(64)
shooting_finish_kernel(DevParams<double> q, int B, int ld, const IO* __restrict__ T, const unsigned long long* __restrict__ wave_keys,
                       int n_slots, uint32_t index_base, const double* __restrict__ state, const double* __restrict__ spheres, int K,
                       double w_obs, double* __restrict__ out, unsigned long long* __restrict__ key_out) {
  __shared__ double sT[3][kWave], sP[3][kWave], sV[3][kWave], sC[3];
  const int lane = threadIdx.x, N = q.N;
  unsigned long long best = ~0ull;
  for (int i = lane; i < n_slots; i += kWave) best = wave_keys[i] < best ? wave_keys[i] : best;
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_down(best, off, kWave);
    best = o < best ? o : best;
  }
  best = __shfl(best, 0, kWave);
  if (lane == 0 && key_out != nullptr) *key_out = best;
  uint32_t idx = (uint32_t)(best & 0xFFFFFFFFull) - index_base;
  if (idx >= (uint32_t)B) idx = 0;                            // (every sample's cost was NaN / the slots were never written: still a defined read)
  const bool live = lane < N;
  double t0 = 0.0, t1 = 0.0, t2 = 0.0;
  if (live) {
    t0 = (double)T[(size_t)(3 * lane + 0) * ld + idx]; t1 = (double)T[(size_t)(3 * lane + 1) * ld + idx]; t2 = (double)T[(size_t)(3 * lane + 2) * ld + idx];
  }
  sT[0][lane] = t0; sT[1][lane] = t1; sT[2][lane] = t2;
  __syncthreads();
  if (lane < 3) {                                             // one axis per lane: the double integrator of planner.py:449-460, states and sums
    const int a = lane;
    const AxisConsts<double> c = axis_consts<double>(q, a, q.has_goal ? state[6 + a] : 0.0);
    double p = state[a], v = state[3 + a];
    RolloutSums<double> s = {0, 0, 0, 0, 0};
    for (int k = 0; k < N; ++k) {
      const double tk = sT[a][k];
      const double acc = tk * q.inv_mass - c.grav, dev = tk - c.hov, e = p - c.gl;
      sP[a][k] = p; sV[a][k] = v;
      if (k == N - 1) s.sterm = e * e; else s.sp += e * e;
      s.sv += v * v; s.sa += acc * acc; s.st += dev * dev;
      p = p + v * q.dt + q.half_dt2 * acc;
      v = v + acc * q.dt;
    }
    s.sp += s.sterm;
    sC[a] = axis_cost(q, s);
  }
  __syncthreads();
  const double cost = sC[0] + sC[1] + sC[2];
  // ---- extraction (planner.py:582-654), lane k = step k
  const double mag = sqrt(t0 * t0 + t1 * t1 + t2 * t2);
  const bool valid = live && mag > 1e-6;
  double b1[3] = {0, 0, 0}, b2[3] = {0, 0, 0}, b3[3] = {0, 0, 0};
  double roll = 0.0, pitch = 0.0, yaw = 0.0;
  double n1 = 0.0;
  if (valid) {
    b3[0] = t0 / mag; b3[1] = t1 / mag; b3[2] = t2 / mag;
    b1[0] = 0.0; b1[1] = -b3[2]; b1[2] = b3[1];
    n1 = sqrt(b1[1] * b1[1] + b1[2] * b1[2]);
    if (n1 > 1e-6) { b1[1] /= n1; b1[2] /= n1; } else { b1[0] = 1.0; b1[1] = 0.0; b1[2] = 0.0; }
    b2[0] = b3[1] * b1[2] - b3[2] * b1[1];
    b2[1] = b3[2] * b1[0] - b3[0] * b1[2];
    b2[2] = b3[0] * b1[1] - b3[1] * b1[0];
    roll = atan2(b2[2], b3[2]);
    pitch = asin(fmin(fmax(-b1[2], -1.0), 1.0));
    yaw = n1 > 1e-6 ? (b1[1] == 0.0 ? b1[1] : copysign(1.5707963267948966, b1[1])) : 0.0;   // atan2(b1y, b1x) with b1x exactly 0, or b1 = (1,0,0)
  }
  const uint64_t vmask = wave_ballot(valid);
  const uint64_t below = vmask & ((lane == 0) ? 0ull : (~0ull >> (64 - lane)));
  const bool has_prev = valid && below != 0ull;
  const int pk = has_prev ? 63 - __builtin_clzll(below) : lane;
  double q1[3], q2[3], q3[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) { q1[c] = group_gather<kWave>(b1[c], pk); q2[c] = group_gather<kWave>(b2[c], pk); q3[c] = group_gather<kWave>(b3[c], pk); }
  double w0 = 0.0, w1 = 0.0, w2 = 0.0;
  if (has_prev) {
    double d1[3], d2[3], d3[3];
    for (int c = 0; c < 3; ++c) {
      d1[c] = (b1[c] - q1[c]) / q.dt;
      d2[c] = (b2[c] - q2[c]) / q.dt;
      d3[c] = (b3[c] - q3[c]) / q.dt;
    }
    w0 = b3[0] * d2[0] + b3[1] * d2[1] + b3[2] * d2[2];
    w1 = b1[0] * d3[0] + b1[1] * d3[1] + b1[2] * d3[2];
    w2 = b2[0] * d1[0] + b2[1] * d1[1] + b2[2] * d1[2];
  }
  // ---- what is left of the sphere penalty at the winner (the objective of se3mpc_rollout_iterate_obstacles_*)
  double pen = 0.0;
  if (spheres != nullptr && K > 0) {
    double pl = 0.0;
    if (live) {
      const double px = sP[0][lane], py = sP[1][lane], pz = sP[2][lane];
      for (int j = 0; j < K; ++j) {
        const double dx = px - spheres[4 * j], dy = py - spheres[4 * j + 1], dz = pz - spheres[4 * j + 2], sm = spheres[4 * j + 3] + q.margin;
        const double h = fmax(0.0, -((dx * dx + dy * dy + dz * dz) - sm * sm));
        pl += h * h;
      }
    }
    pen = w_obs * wave_sum(pl);
  }
  if (live) {
    const int k = lane;
    double* o = out;
    o[3 * k] = sP[0][k]; o[3 * k + 1] = sP[1][k]; o[3 * k + 2] = sP[2][k]; o += 3 * N;
    o[3 * k] = sV[0][k]; o[3 * k + 1] = sV[1][k]; o[3 * k + 2] = sV[2][k]; o += 3 * N;
    o[3 * k] = t0; o[3 * k + 1] = t1; o[3 * k + 2] = t2; o += 3 * N;
    o[3 * k] = t0 / q.mass; o[3 * k + 1] = t1 / q.mass; o[3 * k + 2] = t2 / q.mass - q.grav; o += 3 * N;      // planner.py:589
    o[3 * k] = roll; o[3 * k + 1] = pitch; o[3 * k + 2] = yaw; o += 3 * N;
    o[3 * k] = w0; o[3 * k + 1] = w1; o[3 * k + 2] = w2; o += 3 * N;
    o[k] = mag;                                                                                                 // planner.py:601
  }
  if (lane == 0) { out[19 * N] = cost; out[19 * N + 1] = pen; out[19 * N + 2] = cost + pen; }
}

// ------------------------------------------------------------------------------------------
// Obstacle source: occupancy grid -> sphere table, on the device.
// Replaces the selection of cloud/main_improved_threelayer.py:387-398 (and of
// tests/test_se3_mpc_with_mapper.py:29-33): occupied = grid[occ > threshold] in grid order,
// step = max(1, n // target), spheres = occupied[::step] with a fixed radius.  One 256-thread workgroup;
// wavefront w owns a contiguous quarter of the grid and walks it 64 cells at a time (coalesced), ranking
// occupied cells with ballot + popcount; the four wavefront totals meet in LDS.  Deterministic order.
// ------------------------------------------------------------------------------------------
template <typename R>
__global__ void __launch_bounds__(256)
spheres_from_grid_kernel(const R* __restrict__ pos, const R* __restrict__ occ, int M, R threshold, int target, R radius,
                         R* __restrict__ spheres, int cap, int32_t* __restrict__ count) {
  __shared__ int wave_total[4];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int seg = ((M + 3) / 4 + kWave - 1) / kWave * kWave;          // per-wavefront segment, multiple of 64
  const int lo = wave * seg, hi = (lo + seg < M) ? lo + seg : M;
  int mine = 0;
  for (int i0 = lo; i0 < hi; i0 += kWave) {
    const int i = i0 + lane;
    const bool o = i < hi && occ[i] > threshold;
    mine += __builtin_popcountll(wave_ballot(o));
  }
  if (lane == 0) wave_total[wave] = mine;
  __syncthreads();
  int rank = 0, total = 0;
  for (int w = 0; w < 4; ++w) { if (w < wave) rank += wave_total[w]; total += wave_total[w]; }
  const int step = (target > 0 && total / target > 1) ? total / target : 1;
  for (int i0 = lo; i0 < hi; i0 += kWave) {
    const int i = i0 + lane;
    const bool o = i < hi && occ[i] > threshold;
    const uint64_t m = wave_ballot(o);
    if (o) {
      const int r = rank + __builtin_popcountll(m & ((lane == 0) ? 0ull : (~0ull >> (64 - lane))));
      if (r % step == 0 && r / step < cap) {
        R* s4 = spheres + (size_t)4 * (r / step);
        s4[0] = pos[(size_t)3 * i]; s4[1] = pos[(size_t)3 * i + 1]; s4[2] = pos[(size_t)3 * i + 2]; s4[3] = radius;
      }
    }
    rank += __builtin_popcountll(m);
  }
  if (threadIdx.x == 0) {
    const int k = total == 0 ? 0 : (total + step - 1) / step;
    *count = k < cap ? k : cap;
  }
}

// ------------------------------------------------------------------------------------------
// [rows][ld_in] -> [cols][ld_out] transpose through a padded LDS tile
// ------------------------------------------------------------------------------------------
template <typename R>
__global__ void __launch_bounds__(256)
transpose_kernel(int rows, int cols, const R* __restrict__ in, int ld_in, R* __restrict__ out, int ld_out) {
  __shared__ R tile[64][65];
  const int c0 = blockIdx.x * 64, r0 = blockIdx.y * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;   // 64 x 4
  for (int i = ty; i < 64; i += 4) {
    const int r = r0 + i, c = c0 + tx;
    if (r < rows && c < cols) tile[i][tx] = in[(size_t)r * ld_in + c];
  }
  __syncthreads();
  for (int i = ty; i < 64; i += 4) {
    const int c = c0 + i, r = r0 + tx;
    if (r < rows && c < cols) out[(size_t)c * ld_out + r] = tile[tx][i];
  }
}

// Transpose of a matrix with one SMALL dimension (a decision-vector block: 9N <= 576 against a batch of thousands to
// millions): out[c][r] = in[r][c].  The generic 64 x 64 tile reads or writes 256-B segments at a stride of 4 * 9N
// bytes (1080 B at N = 30): misaligned partial lines on the narrow side.  Here a workgroup owns a strip of TW
// consecutive indices of the LONG dimension and ALL indices of the short one, so the narrow side is one contiguous
// run of TW * small elements, moved with full lines; the strip is staged in LDS with an odd row pitch (conflict-free
// both ways).  ROWS_SMALL: in is [small][ld_in] (lane layout -> problem layout); else in is [long][ld_in].
template <typename R, bool ROWS_SMALL>
__global__ void __launch_bounds__(512)
transpose_strip_kernel(int small, int longn, const R* __restrict__ in, int ld_in, R* __restrict__ out, int ld_out, int TW) {
  HIP_DYNAMIC_SHARED(unsigned char, lds_raw)
  R* tile = reinterpret_cast<R*>(lds_raw);                  // [TW][pitch]: tile[t][s] = element (short index s, long index l0 + t)
  const int pitch = small | 1;
  const int l0 = blockIdx.x * TW;
  const int nt = (longn - l0 < TW) ? longn - l0 : TW;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave, nwave = blockDim.x / kWave;
  constexpr int U = 8;                                      // independent loads in flight per lane
  if constexpr (ROWS_SMALL) {
    // read: one wavefront per short-index row, lanes along the long dimension (coalesced), TW <= 64
    for (int s0 = wave * U; s0 < small; s0 += nwave * U) {
      R v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) v[u] = (s0 + u < small && lane < nt) ? in[(size_t)(s0 + u) * ld_in + l0 + lane] : (R)0;
#pragma unroll
      for (int u = 0; u < U; ++u) if (s0 + u < small && lane < nt) tile[lane * pitch + s0 + u] = v[u];
    }
    __syncthreads();
    // write: one wavefront per output row (long index), lanes along the short dimension: consecutive rows are adjacent
    for (int t = wave; t < nt; t += nwave)
      for (int sidx = lane; sidx < small; sidx += kWave) out[(size_t)(l0 + t) * ld_out + sidx] = tile[t * pitch + sidx];
  } else {
    for (int t = wave; t < nt; t += nwave) {
      const R* src = in + (size_t)(l0 + t) * ld_in;
      for (int s0 = lane; s0 < small; s0 += kWave * U) {
        R v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = (s0 + u * kWave < small) ? src[s0 + u * kWave] : (R)0;
#pragma unroll
        for (int u = 0; u < U; ++u) if (s0 + u * kWave < small) tile[t * pitch + s0 + u * kWave] = v[u];
      }
    }
    __syncthreads();
    for (int sidx = wave; sidx < small; sidx += nwave)
      if (lane < nt) out[(size_t)sidx * ld_out + l0 + lane] = tile[lane * pitch + sidx];
  }
}

template <typename R>
int argmin_impl(int B, const R* cost, uint32_t index_base, uint64_t* key, void* stream) {
  if (B < 0) return SE3MPC_ERR_SHAPE;
  if (!key) return SE3MPC_ERR_NULL;
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(key, 0xFF, sizeof(uint64_t), s) != hipSuccess) return launch_status("se3mpc_argmin(memset)");
  if (B == 0) return SE3MPC_OK;
  if (!cost) return SE3MPC_ERR_NULL;
  int grid = grid_for(B, 256);
  if (grid > 1024) grid = 1024;
  hipLaunchKernelGGL(argmin_kernel<R>, dim3(grid), dim3(256), 0, s, B, cost, index_base, (unsigned long long*)key);
  return launch_status("se3mpc_argmin");
}

static int population_splits(int B) {
  int n = B / 65536;
  return n < 1 ? 1 : (n > 16 ? 16 : n);
}

template <typename R>
int population_sums_impl(int rows, int B, int ld, const R* X, const R* cost, double cost_ref, const uint64_t* ref_key,
                         double temperature, double* out, double* workspace, void* stream) {
  if (rows < 0 || B < 0 || ld < B) return SE3MPC_ERR_SHAPE;
  if (!out) return SE3MPC_ERR_NULL;
  if (cost != nullptr && (!(temperature > 0.0) || !std::isfinite(temperature) || !std::isfinite(cost_ref))) return SE3MPC_ERR_PARAM;
  hipStream_t s = (hipStream_t)stream;
  if (B == 0) {
    if (hipMemsetAsync(out, 0, (size_t)(rows + 1) * sizeof(double), s) != hipSuccess) return launch_status("se3mpc_population_sums(memset)");
    return SE3MPC_OK;
  }
  if ((rows > 0 && !X) || !workspace) return SE3MPC_ERR_NULL;
  const int nsplit = population_splits(B);
  const int per_split = (B + nsplit - 1) / nsplit;
  hipLaunchKernelGGL(population_sums_kernel<R>, dim3(rows + 1, nsplit), dim3(256), 0, s, rows, B, ld, X, cost, cost_ref,
                     reinterpret_cast<const unsigned long long*>(ref_key), cost != nullptr ? 1.0 / temperature : 0.0, per_split,
                     workspace);
  int rc = launch_status("se3mpc_population_sums");
  if (rc) return rc;
  hipLaunchKernelGGL(population_fold_kernel, dim3(grid_for(rows + 1, 256)), dim3(256), 0, s, rows + 1, nsplit, workspace, out);
  return launch_status("se3mpc_population_sums(fold)");
}

template <typename R>
int spheres_from_grid_impl(const R* pos, const R* occ, int M, double threshold, int target, double radius, R* spheres, int cap,
                           int32_t* count, void* stream) {
  if (M < 0 || cap < 0 || target < 1) return SE3MPC_ERR_SHAPE;
  if (!count || (M > 0 && (!pos || !occ)) || (cap > 0 && !spheres)) return SE3MPC_ERR_NULL;
  hipLaunchKernelGGL(spheres_from_grid_kernel<R>, dim3(1), dim3(256), 0, (hipStream_t)stream, pos, occ, M, (R)threshold,
                     target, (R)radius, spheres, cap, count);
  return launch_status("se3mpc_spheres_from_grid");
}

template <typename R>
int transpose_impl(int rows, int cols, const R* in, int ld_in, R* out, int ld_out, void* stream) {
  if (rows < 0 || cols < 0 || ld_in < cols || ld_out < rows) return SE3MPC_ERR_SHAPE;
  if (rows == 0 || cols == 0) return SE3MPC_OK;
  if (!in || !out) return SE3MPC_ERR_NULL;
  // one small dimension (a decision-vector block against a batch): strip kernel with full-line traffic on both sides
  const int small = rows < cols ? rows : cols, longn = rows < cols ? cols : rows;
  if (small <= 9 * SE3MPC_MAX_HORIZON && longn >= 256) {
    int TW = 64;
    while (TW > 16 && (size_t)TW * (small | 1) * sizeof(R) > 72 * 1024) TW /= 2;
    const size_t lds = (size_t)TW * (small | 1) * sizeof(R);
    if (lds <= 72 * 1024) {
      if (rows < cols)
        hipLaunchKernelGGL((transpose_strip_kernel<R, true>), dim3(grid_for(longn, TW)), dim3(512), lds, (hipStream_t)stream, small,
                           longn, in, ld_in, out, ld_out, TW);
      else
        hipLaunchKernelGGL((transpose_strip_kernel<R, false>), dim3(grid_for(longn, TW)), dim3(512), lds, (hipStream_t)stream, small,
                           longn, in, ld_in, out, ld_out, TW);
      return launch_status("se3mpc_transpose(strip)");
    }
  }
  hipLaunchKernelGGL(transpose_kernel<R>, dim3(grid_for(cols, 64), grid_for(rows, 64)), dim3(256), 0,
                     (hipStream_t)stream, rows, cols, in, ld_in, out, ld_out);
  return launch_status("se3mpc_transpose");
}

template <typename IO>
int shooting_finish_impl(const se3mpc_params* p, int B, int ld, const IO* T, const uint64_t* wave_keys, int n_slots, uint32_t index_base,
                         const double* state, const double* spheres, int K, double obstacle_weight, double* out, uint64_t* key_out,
                         void* stream) {
  if (n_slots < 1 || K < 0 || K > SE3MPC_MAX_SPHERES) return SE3MPC_ERR_SHAPE;
  int rc = check_lane_args(p, B, ld, p ? 3LL * p->horizon : 0, sizeof(IO));
  if (rc) return rc;
  if (B < 1) return SE3MPC_ERR_SHAPE;                          // a plan needs a sample
  if (!std::isfinite(obstacle_weight) || obstacle_weight < 0.0) return SE3MPC_ERR_PARAM;
  if (!T || !wave_keys || !state || !out || (K > 0 && !spheres)) return SE3MPC_ERR_NULL;
  const DevParams<double> q = make_dev_params<double>(*p);
  hipLaunchKernelGGL(shooting_finish_kernel<IO>, dim3(1), dim3(kWave), 0, (hipStream_t)stream, q, B, ld, T,
                     reinterpret_cast<const unsigned long long*>(wave_keys), n_slots, index_base, state, K > 0 ? spheres : nullptr, K,
                     obstacle_weight, out, reinterpret_cast<unsigned long long*>(key_out));
  return launch_status("se3mpc_shooting_finish");
}

}  // namespace se3mpc

using namespace se3mpc;   // C ABI (include/se3mpc.h)

extern "C" int se3mpc_argmin_f32(int B, const float* cost, uint32_t index_base, uint64_t* key, void* stream) {
  return argmin_impl<float>(B, cost, index_base, key, stream);
}
extern "C" int se3mpc_argmin_f64(int B, const double* cost, uint32_t index_base, uint64_t* key, void* stream) {
  return argmin_impl<double>(B, cost, index_base, key, stream);
}

extern "C" int se3mpc_reduce_keys(const uint64_t* wave_keys, int per_batch, int nbatch, uint64_t* keys_out, void* stream) {
  if (per_batch < 1 || nbatch < 0) return SE3MPC_ERR_SHAPE;
  if (nbatch == 0) return SE3MPC_OK;
  if (!wave_keys || !keys_out) return SE3MPC_ERR_NULL;
  hipLaunchKernelGGL(reduce_keys_kernel, dim3(nbatch), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const unsigned long long*>(wave_keys), per_batch,
                     reinterpret_cast<unsigned long long*>(keys_out));
  return launch_status("se3mpc_reduce_keys");
}

extern "C" int se3mpc_shooting_finish_f32(const se3mpc_params* p, int B, int ld, const float* T, const uint64_t* wave_keys, int n_slots,
                                          uint32_t index_base, const double* state, const double* spheres, int K, double obstacle_weight,
                                          double* out, uint64_t* key_out, void* stream) {
  return se3mpc::shooting_finish_impl<float>(p, B, ld, T, wave_keys, n_slots, index_base, state, spheres, K, obstacle_weight, out, key_out, stream);
}
extern "C" int se3mpc_shooting_finish_f64(const se3mpc_params* p, int B, int ld, const double* T, const uint64_t* wave_keys, int n_slots,
                                          uint32_t index_base, const double* state, const double* spheres, int K, double obstacle_weight,
                                          double* out, uint64_t* key_out, void* stream) {
  return se3mpc::shooting_finish_impl<double>(p, B, ld, T, wave_keys, n_slots, index_base, state, spheres, K, obstacle_weight, out, key_out, stream);
}

extern "C" int se3mpc_population_workspace(int rows, int B) { return B < 1 ? 1 : (rows + 1) * population_splits(B); }
extern "C" int se3mpc_population_sums_f32(int rows, int B, int ld, const float* X, const float* cost, double cost_ref,
                                          const uint64_t* ref_key, double temperature, double* out, double* workspace,
                                          void* stream) {
  return population_sums_impl<float>(rows, B, ld, X, cost, cost_ref, ref_key, temperature, out, workspace, stream);
}
extern "C" int se3mpc_population_sums_f64(int rows, int B, int ld, const double* X, const double* cost, double cost_ref,
                                          const uint64_t* ref_key, double temperature, double* out, double* workspace,
                                          void* stream) {
  return population_sums_impl<double>(rows, B, ld, X, cost, cost_ref, ref_key, temperature, out, workspace, stream);
}

extern "C" int se3mpc_spheres_from_grid_f32(const float* positions, const float* occupancy, int M, double threshold, int target, double radius,
                                            float* spheres, int cap, int32_t* count, void* stream) {
  return spheres_from_grid_impl<float>(positions, occupancy, M, threshold, target, radius, spheres, cap, count, stream);
}
extern "C" int se3mpc_spheres_from_grid_f64(const double* positions, const double* occupancy, int M, double threshold, int target, double radius,
                                            double* spheres, int cap, int32_t* count, void* stream) {
  return spheres_from_grid_impl<double>(positions, occupancy, M, threshold, target, radius, spheres, cap, count, stream);
}
extern "C" int se3mpc_transpose_f32(int rows, int cols, const float* in, int ld_in, float* out, int ld_out, void* stream) {
  return transpose_impl<float>(rows, cols, in, ld_in, out, ld_out, stream);
}
extern "C" int se3mpc_transpose_f64(int rows, int cols, const double* in, int ld_in, double* out, int ld_out, void* stream) {
  return transpose_impl<double>(rows, cols, in, ld_in, out, ld_out, stream);
}
