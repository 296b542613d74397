// mppi_split.hip -- MPPI with ONE problem's samples split over several workgroups.
//
// se3mpc_mppi_* (mppi.hip) gives a problem one workgroup, which is right for thousands of problems and leaves 255 of 256 CUs idle for the
// single plan a drone asks for.  Here the S samples of a problem are split over G workgroups ("splits"): workgroup j owns samples
// [j S/G, (j + 1) S/G).  The noise counter is (q, s, g, k) per sample, so the sample set does not depend on who draws it.
//
// The iterations of a problem depend on each other through the nominal U, and all G workgroups need the new U.  The hand-off is the
// KERNEL BOUNDARY: one launch per iteration plus one finishing launch, no tickets, no flags, no spinning, no atomics.
//   launch it (mppi_split_iter_kernel, grid (G, nprob)):
//     prologue  it = 0: U <- U_in.  it > 0: every workgroup folds the G partials that launch it - 1 wrote, in split order j = 0 .. G-1 with
//               the streaming rescale exp(-(m_new - m_old) / lambda) of mppi_kernel's chunk fold, divides by the weight sum, rounds to R and
//               clips as mppi_kernel does.  The same arithmetic in the same order on the same bytes: all G workgroups hold the identical U.
//     body      mppi_kernel's weighted pass (mppi_device.hpp) over the workgroup's own sample range
//     epilogue  the partial (3N weighted rows, weight sum, local minimum; float64) to workspace slot (it & 1, problem, j)
//   finishing launch (mppi_split_finish_kernel, grid (nprob)): fold the last partials the same way, write U_out, the last trace row, cost, keys.
// Every partial is written by one launch and read by a later one, and every fold has a fixed order: results do not depend on dispatch
// order, placement or timing.  Two slots per problem and split, because launch it + 1 reads what launch it wrote while writing its own.
//
// Workspace, doubles, per parity x problem: G partials of 3N + 2 (rows | weight sum | minimum), then the 3N values of the nominal that
// parity's launch ran from (what U stays at when no sample of an iteration has a finite cost: mppi_kernel then leaves U alone).
#include "mppi_device.hpp"

namespace se3mpc {
namespace mppi {

constexpr int kFinishBlock = 256;

__host__ __device__ inline size_t split_partial_doubles(int N) { return (size_t)3 * N + 2; }
__host__ __device__ inline size_t split_problem_doubles(int N, int G) { return (size_t)G * split_partial_doubles(N) + (size_t)3 * N; }

// The nominal after the iteration whose partials `ws` holds (one parity, one problem), into U (LDS): folded in split order.  fs: LDS [2G].
// Returns the iteration's minimum sample cost.  Ends with the workgroup synchronised on U.
// Both kernels fold through this one function with contraction off, so an iteration folded by the next launch and one folded by the
// finishing launch give the same bits (iters = K in one call == K calls of one iteration).
template <typename R>
__device__ __forceinline__ double fold_partials(const DevParams<R>& q, const double* ws, int G, double inv_lam, double* fs, R* U) {
#pragma clang fp contract(off)
  const int rows = 3 * q.N, NT = (int)blockDim.x, tid = (int)threadIdx.x;
  const size_t pd = split_partial_doubles(q.N);
  const double kInf = __builtin_huge_val();
  // the two factors of fold step j: the running sums and partial j, both re-expressed against the minimum over partials 0 .. j
  for (int j = tid; j < G; j += NT) {
    double m_old = kInf;
    for (int i = 0; i < j; ++i) m_old = fmin(m_old, ws[(size_t)i * pd + rows + 1]);
    const double mj = ws[(size_t)j * pd + rows + 1];
    const double mn = fmin(m_old, mj);
    fs[2 * j] = (m_old < kInf) ? exp((mn - m_old) * inv_lam) : 0.0;
    fs[2 * j + 1] = (mj < kInf) ? exp((mn - mj) * inv_lam) : 0.0;
  }
  __syncthreads();
  double m = kInf, wsum = 0.0;
  for (int j = 0; j < G; ++j) {
    m = fmin(m, ws[(size_t)j * pd + rows + 1]);
    const double v = ws[(size_t)j * pd + rows] * fs[2 * j + 1];
    wsum = (j == 0) ? v : wsum * fs[2 * j] + v;
  }
  const double* prev = ws + (size_t)G * pd;
  for (int r = tid; r < rows; r += NT) {
    double a = 0.0;
    for (int j = 0; j < G; ++j) {
      const double v = ws[(size_t)j * pd + r] * fs[2 * j + 1];
      a = (j == 0) ? v : a * fs[2 * j] + v;
    }
    U[r] = (wsum > 0.0) ? box_clip(q, r % 3, (R)(a / wsum)) : (R)prev[r];
  }
  __syncthreads();
  return m;
}

// LDS of both kernels: the layout of mppi_kernel, then the 2G fold factors
__host__ __device__ inline size_t split_lds_bytes(const Lds& L, int G) { return L.total + (size_t)2 * G * 8; }

// One iteration of every problem: workgroup (j, p) runs samples [j S/G, (j + 1) S/G) of problem p with min(S/G, kBlock) lanes.
template <typename R>
__global__ void __launch_bounds__(kBlock, 4)
mppi_split_iter_kernel(DevParams<R> q, int ld, int Sg, int it, R sigma, double inv_lam, uint32_t key0, uint32_t key1, uint32_t iter_base,
                       const uint32_t* __restrict__ iter_offset, uint32_t index_base, const R* __restrict__ p0, const R* __restrict__ v0,
                       const R* __restrict__ goal, const R* __restrict__ U_in, const R* __restrict__ spheres, int K, R w_obs,
                       R* __restrict__ trace, double* workspace) {
  HIP_DYNAMIC_SHARED(unsigned char, lds_raw)
  const int N = q.N, rows = 3 * N, NT = (int)blockDim.x, W = NT / kWave;
  const int tid = (int)threadIdx.x;
  const int j = (int)blockIdx.x, G = (int)gridDim.x, p = (int)blockIdx.y, nprob = (int)gridDim.y;
  const Lds L = lds_layout(N, K, W, sizeof(R));
  const LdsView<R> l = lds_view<R>(lds_raw, L);
  R* U = l.U;
  double* fs = reinterpret_cast<double*>(lds_raw + L.total);
  const size_t prob = split_problem_doubles(N, G);
  double* mine = workspace + ((size_t)(it & 1) * nprob + p) * prob;                 // this launch writes here
  const double* theirs = workspace + ((size_t)((it & 1) ^ 1) * nprob + p) * prob;   // the previous launch wrote here
  stage_spheres(q, spheres, K, l.sph);
  if (it == 0) {
    for (int r = tid; r < rows; r += NT) U[r] = U_in[(size_t)r * ld + p];
    __syncthreads();
  } else {
    const double m = fold_partials<R>(q, theirs, G, inv_lam, fs, U);
    if (j == 0 && tid == 0 && trace != nullptr) trace[(size_t)(it - 1) * ld + p] = (R)m;
  }
  Ctx<R> c = load_ctx(q, ld, p, key0, key1, index_base + (uint32_t)p, p0, v0, goal, U, l.sph, K, w_obs);
  c.g = iter_base + (iter_offset != nullptr ? *iter_offset : 0u) + (uint32_t)it;
  const double m = weighted_pass<R>(c, U, j * Sg, Sg, sigma, inv_lam, l.acc, l.part, l.red);
  double* slot = mine + (size_t)j * split_partial_doubles(N);
  for (int r = tid; r <= rows; r += NT) slot[r] = l.acc[r];
  if (tid == 0) slot[rows + 1] = m;
  if (j == 0)
    for (int r = tid; r < rows; r += NT) mine[(size_t)G * split_partial_doubles(N) + r] = (double)U[r];
}

// After the last iteration: fold its partials, write U_out and the last trace row, evaluate the nominal once (cost, keys).
// iters = 0: evaluate and copy U_in.
template <typename R>
__global__ void __launch_bounds__(kFinishBlock)
mppi_split_finish_kernel(DevParams<R> q, int ld, int G, int iters, double inv_lam, uint32_t index_base, const R* __restrict__ p0,
                         const R* __restrict__ v0, const R* __restrict__ goal, const R* U_in, R* U_out, const R* __restrict__ spheres, int K,
                         R w_obs, R* __restrict__ cost_out, R* __restrict__ trace, uint64_t* __restrict__ keys, const double* workspace) {
  HIP_DYNAMIC_SHARED(unsigned char, lds_raw)
  const int N = q.N, rows = 3 * N, NT = (int)blockDim.x;
  const int tid = (int)threadIdx.x, wave = tid / kWave;
  const int p = (int)blockIdx.x, nprob = (int)gridDim.x;
  const Lds L = lds_layout(N, K, NT / kWave, sizeof(R));
  const LdsView<R> l = lds_view<R>(lds_raw, L);
  R* U = l.U;
  double* fs = reinterpret_cast<double*>(lds_raw + L.total);
  stage_spheres(q, spheres, K, l.sph);
  if (iters == 0) {
    for (int r = tid; r < rows; r += NT) U[r] = U_in[(size_t)r * ld + p];
    __syncthreads();
  } else {
    const double* theirs = workspace + ((size_t)((iters - 1) & 1) * nprob + p) * split_problem_doubles(N, G);
    const double m = fold_partials<R>(q, theirs, G, inv_lam, fs, U);
    if (tid == 0 && trace != nullptr) trace[(size_t)(iters - 1) * ld + p] = (R)m;
  }
  Ctx<R> c = load_ctx(q, ld, p, 0u, 0u, index_base + (uint32_t)p, p0, v0, goal, U, l.sph, K, w_obs);
  if (wave == 0) write_nominal_cost(c, p, index_base, cost_out, keys);
  for (int r = tid; r < rows; r += NT) U_out[(size_t)r * ld + p] = U[r];
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
static size_t workspace_bytes(int horizon, int nprob, int splits) {
  if (horizon < 1 || horizon > SE3MPC_MAX_HORIZON || nprob < 0 || splits < 1) return 0;
  return (size_t)2 * (size_t)nprob * split_problem_doubles(horizon, splits) * sizeof(double);
}

template <typename R>
static int mppi_split_impl(const se3mpc_params* p, int nprob, int ld, int S, int iters, double sigma, double temperature, uint64_t seed,
                           uint32_t iter_base, const uint32_t* iter_offset, uint32_t index_base, const R* p0, const R* v0, const R* goal,
                           const R* U_in, R* U_out, const R* spheres, int K, double obstacle_weight, R* cost, R* trace, uint64_t* keys,
                           int splits, void* workspace, size_t workspace_size, void* stream) {
  const int rc = check_mppi_args("se3mpc_mppi_split", p, nprob, ld, S, iters, sigma, temperature, K, obstacle_weight);
  if (rc) return rc;
  // the split's own
  if (splits < 1) return fail(SE3MPC_ERR_SHAPE, "se3mpc_mppi_split: splits < 1");
  if (S % (kWave * (long long)splits) != 0) return fail(SE3MPC_ERR_SHAPE, "se3mpc_mppi_split: S is not a multiple of 64 * splits");
  if (S / splits < kMinS) return fail(SE3MPC_ERR_SHAPE, "se3mpc_mppi_split: fewer than 64 samples per split");
  if (nprob > 65535) return fail(SE3MPC_ERR_SHAPE, "se3mpc_mppi_split: nprob > 65535 (the grid's second dimension)");
  if (nprob == 0) return SE3MPC_OK;
  if (!p0 || !v0 || (p->has_goal && !goal) || !U_in || !U_out || !cost || (K > 0 && !spheres)) return fail(SE3MPC_ERR_NULL, "se3mpc_mppi_split: NULL operand");
  if (iters > 0 && workspace == nullptr) return fail(SE3MPC_ERR_NULL, "se3mpc_mppi_split: workspace is NULL");
  if (iters > 0 && workspace_size < workspace_bytes(p->horizon, nprob, splits))
    return fail(SE3MPC_ERR_SHAPE, "se3mpc_mppi_split: workspace smaller than se3mpc_mppi_split_workspace_bytes");
  const int Sg = S / splits, NT = Sg < kBlock ? Sg : kBlock;
  const size_t lds_iter = split_lds_bytes(lds_layout(p->horizon, K, NT / kWave, sizeof(R)), splits);
  const size_t lds_fin = split_lds_bytes(lds_layout(p->horizon, K, kFinishBlock / kWave, sizeof(R)), splits);
  const DevParams<R> q = make_dev_params<R>(*p);
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  const double inv_lam = 1.0 / temperature;
  hipStream_t st = (hipStream_t)stream;
  for (int it = 0; it < iters; ++it) {
    hipLaunchKernelGGL(mppi_split_iter_kernel<R>, dim3(splits, nprob), dim3(NT), lds_iter, st, q, ld, Sg, it, (R)sigma, inv_lam, k0, k1, iter_base,
                       iter_offset, index_base, p0, v0, goal, U_in, spheres, K, (R)obstacle_weight, trace, (double*)workspace);
    const int lrc = launch_status("se3mpc_mppi_split");
    if (lrc) return lrc;
  }
  hipLaunchKernelGGL(mppi_split_finish_kernel<R>, dim3(nprob), dim3(kFinishBlock), lds_fin, st, q, ld, splits, iters, inv_lam, index_base, p0, v0,
                     goal, U_in, U_out, spheres, K, (R)obstacle_weight, cost, trace, keys, (const double*)workspace);
  return launch_status("se3mpc_mppi_split");
}

}  // namespace mppi
}  // namespace se3mpc

using se3mpc::mppi::mppi_split_impl;

extern "C" size_t se3mpc_mppi_split_workspace_bytes(int horizon, int nprob, int splits) {
  return se3mpc::mppi::workspace_bytes(horizon, nprob, splits);
}
extern "C" int se3mpc_mppi_split_f32(const se3mpc_params* p, int nprob, int ld, int S, int iters, double sigma, double temperature, uint64_t seed,
                                     uint32_t iter_base, const uint32_t* iter_offset, uint32_t index_base, const float* p0, const float* v0,
                                     const float* goal, const float* U_in, float* U_out, const float* spheres, int K, double obstacle_weight,
                                     float* cost, float* trace, uint64_t* keys, int splits, void* workspace, size_t workspace_bytes, void* stream) {
  return mppi_split_impl<float>(p, nprob, ld, S, iters, sigma, temperature, seed, iter_base, iter_offset, index_base, p0, v0, goal, U_in, U_out,
                                spheres, K, obstacle_weight, cost, trace, keys, splits, workspace, workspace_bytes, stream);
}
extern "C" int se3mpc_mppi_split_f64(const se3mpc_params* p, int nprob, int ld, int S, int iters, double sigma, double temperature, uint64_t seed,
                                     uint32_t iter_base, const uint32_t* iter_offset, uint32_t index_base, const double* p0, const double* v0,
                                     const double* goal, const double* U_in, double* U_out, const double* spheres, int K, double obstacle_weight,
                                     double* cost, double* trace, uint64_t* keys, int splits, void* workspace, size_t workspace_bytes,
                                     void* stream) {
  return mppi_split_impl<double>(p, nprob, ld, S, iters, sigma, temperature, seed, iter_base, iter_offset, index_base, p0, v0, goal, U_in, U_out,
                                 spheres, K, obstacle_weight, cost, trace, keys, splits, workspace, workspace_bytes, stream);
}
