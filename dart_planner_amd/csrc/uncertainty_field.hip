// uncertainty_field.hip -- the reference's UncertaintyField on the device: the dense grid of the mission layer (L4) that
// produces the goals plan_trajectory consumes.  Two float64 grids in HBM, C order with k fastest (uncertainty, observation_count).
//
// Reference arithmetic ("field.py" = src/dart_planner/neural_scene/uncertainty_field.py):
//   * reduce_uncertainty_around_position   field.py:221-260   se3mpc_ufield_stamp          (S stamps, one launch, gather form)
//   * update_uncertainty_field             field.py:66-108    se3mpc_ufield_update_points  (same-voxel points in input order)
//   * get_uncertainty_at_position          field.py:110-125   se3mpc_ufield_query
//   * get_statistics                       field.py:262-289   se3mpc_ufield_statistics     (fixed-shape fold, no float atomics)
//   * identify_high_uncertainty_regions    field.py:154-182, :308-405   se3mpc_ufield_regions
//   * get_exploration_targets              field.py:204-219   se3mpc_ufield_targets
//
// Contraction is off in this file: floor((p - b0) / res), the voxel centre (idx + 0.5) * res + b0, the distance, `distance <= radius`,
// `> threshold` and `volume >= min_volume` compare values that NumPy forms one rounded operation at a time.
#pragma clang fp contract(off)
#include <cmath>

#include "uncertainty_field_device.hpp"

namespace se3mpc {

static_assert(sizeof(se3mpc_ufield) == 64, "se3mpc_ufield is mirrored by capi.UFieldDesc");

// ------------------------------------------------------------------------------------------------ fill, query
__global__ void __launch_bounds__(256)
ufield_fill_kernel(UField f) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= f.V) return;
  f.u[v] = 1.0;                                                                    // field.py:58-59
  f.c[v] = 0.0;
}

__global__ void __launch_bounds__(256)
ufield_query_kernel(UField f, int B, const double* __restrict__ pos, double* __restrict__ out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int v = voxel_of(f, pos + 3 * (size_t)b);
  out[b] = v >= 0 ? f.u[v] : 1.0;                                                  // field.py:122-125
}

// ------------------------------------------------------------------------------------------------ stamps
// One lane per voxel; a workgroup owns kStampSpan consecutive raster voxels.  Stamps come in chunks of 256: lane t clips stamp chunk + t
// against the box that holds the workgroup's voxels and sets its bit, then every lane walks the set bits in index order and applies
// u = u * (1 - f) where `distance <= radius` (field.py:248-260).  A voxel is written by its own lane only: S stamps in one launch give
// the bytes of S sequential calls.
constexpr int kStampSpan = 256;

__global__ void __launch_bounds__(256)
ufield_stamp_kernel(UField f, int S, const double* __restrict__ centre, const double* __restrict__ radius, const int32_t* __restrict__ radius_voxels,
                    const double* __restrict__ factor) {
  __shared__ unsigned long long hit[4];
  __shared__ int win[256][6];
  const int t = threadIdx.x;
  const long long first = (long long)blockIdx.x * kStampSpan;
  const long long last = first + kStampSpan - 1 < (long long)f.V - 1 ? first + kStampSpan - 1 : (long long)f.V - 1;
  int lo[3], hi[3];                                                                // a box around voxels first .. last, inclusive
  {
    const int plane = f.n[1] * f.n[2];
    const int i0 = (int)(first / plane), i1 = (int)(last / plane);
    const int j0 = (int)(first % plane) / f.n[2], j1 = (int)(last % plane) / f.n[2];
    lo[0] = i0; hi[0] = i1;
    lo[1] = i0 == i1 ? j0 : 0; hi[1] = i0 == i1 ? j1 : f.n[1] - 1;
    lo[2] = 0; hi[2] = f.n[2] - 1;
  }
  const long long v = first + t;
  const bool live = v < f.V;
  int idx[3] = {0, 0, 0};
  double c[3] = {0.0, 0.0, 0.0}, u = 0.0, cnt = 0.0;
  if (live) {
    raster_to_index(f, (int)v, idx);
    for (int a = 0; a < 3; ++a) c[a] = ((double)idx[a] + 0.5) * f.res + f.b0[a];    // field.py:297-302
    u = f.u[v];
    cnt = f.c[v];
  }
  bool touched = false;
  for (int base = 0; base < S; base += 256) {
    if (t < 4) hit[t] = 0ull;
    __syncthreads();
    const int s = base + t;
    if (s < S) {
      int rv = radius_voxels[s];
      rv = rv < 0 ? -1 : (rv > kIndexClamp ? kIndexClamp : rv);                    // a negative radius: range() is empty
      bool overlap = rv >= 0;
      for (int a = 0; a < 3; ++a) {
        const int g = grid_index(f, centre[3 * (size_t)s + a], a);
        const int w0 = g - rv > 0 ? g - rv : 0;                                    // field.py:236-247
        const int w1 = g + rv + 1 < f.n[a] ? g + rv + 1 : f.n[a];
        win[t][a] = w0;
        win[t][3 + a] = w1;
        overlap = overlap && w0 <= hi[a] && w1 > lo[a];
      }
      if (overlap) atomicOr(&hit[t >> 6], 1ull << (t & 63));
    }
    __syncthreads();
    if (live) {
      for (int w = 0; w < 4; ++w) {
        unsigned long long bits = hit[w];
        while (bits != 0ull) {
          const int q = w * 64 + __builtin_ctzll(bits);
          bits &= bits - 1ull;
          const bool inside = idx[0] >= win[q][0] && idx[0] < win[q][3] && idx[1] >= win[q][1] && idx[1] < win[q][4] && idx[2] >= win[q][2] &&
                              idx[2] < win[q][5];
          if (!inside) continue;
          const size_t sq = (size_t)(base + q);
          const double dx = c[0] - centre[3 * sq], dy = c[1] - centre[3 * sq + 1], dz = c[2] - centre[3 * sq + 2];
          const double dist = sqrt((dx * dx + dy * dy) + dz * dz);                 // np.linalg.norm, field.py:251
          if (dist <= radius[sq]) {
            u = u * (1.0 - factor[sq]);                                            // field.py:256
            cnt = cnt + 1.0;
            touched = true;
          }
        }
      }
    }
    __syncthreads();
  }
  if (touched) {
    f.u[v] = u;
    f.c[v] = cnt;
  }
}

// ------------------------------------------------------------------------------------------------ point updates
// keys[i] = the raster index of point i (-1 outside the grid); the first point of every touched voxel is found with a 64-bit minimum in a
// table the first launch resets at exactly the touched voxels; that point then walks the later keys and applies its voxel's points in
// input order (field.py:77-88 in the loop of :107-108).
__global__ void __launch_bounds__(256)
ufield_point_keys_kernel(UField f, int N, const double* __restrict__ pos, int32_t* __restrict__ keys, unsigned long long* __restrict__ first) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int v = voxel_of(f, pos + 3 * (size_t)i);
  keys[i] = v;
  if (v >= 0) first[v] = ~0ull;
}

__global__ void __launch_bounds__(256)
ufield_point_first_kernel(int N, const int32_t* __restrict__ keys, unsigned long long* __restrict__ first) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int v = keys[i];
  if (v >= 0) atomicMin(&first[v], (unsigned long long)i);
}

__global__ void __launch_bounds__(256)
ufield_point_apply_kernel(UField f, int N, const int32_t* __restrict__ keys, const unsigned long long* __restrict__ first,
                          const double* __restrict__ unc, const double* __restrict__ weight, double alpha) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int v = keys[i];
  if (v < 0 || first[v] != (unsigned long long)i) return;
  double u = f.u[v], c = f.c[v];
  for (int j = i; j < N; ++j) {
    if (keys[j] != v) continue;
    u = alpha * unc[j] + (1.0 - alpha) * u;                                        // field.py:83-85
    c = c + (weight != nullptr ? weight[j] : 1.0);                                 // field.py:88
  }
  f.u[v] = u;
  f.c[v] = c;
}

// ------------------------------------------------------------------------------------------------ statistics
// kStatBlocks workgroups of 256 lanes stride over the grid, every lane folds its own voxels in raster order, a fixed tree folds the
// lanes, a second launch folds the workgroups with the same tree: the launch shape is fixed, so two runs add in the same order.
constexpr int kStatBlocks = 256;

struct StatPart {
  int observed, high;
  double sum, mn, mx;
};

__device__ __forceinline__ void stat_merge(StatPart& a, const StatPart& b) {
  a.observed += b.observed;
  a.high += b.high;
  a.sum = a.sum + b.sum;
  a.mn = nan_min(a.mn, b.mn);
  a.mx = nan_max(a.mx, b.mx);
}

// a fixed tree over the 256 lanes of the workgroup; the result is in lane 0
__device__ __forceinline__ void stat_tree(StatPart& p, int t) {
  __shared__ int si[2][256];
  __shared__ double sd[3][256];
  si[0][t] = p.observed; si[1][t] = p.high; sd[0][t] = p.sum; sd[1][t] = p.mn; sd[2][t] = p.mx;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (t < h) {
      StatPart o = {si[0][t + h], si[1][t + h], sd[0][t + h], sd[1][t + h], sd[2][t + h]};
      stat_merge(p, o);
      si[0][t] = p.observed; si[1][t] = p.high; sd[0][t] = p.sum; sd[1][t] = p.mn; sd[2][t] = p.mx;
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(256)
ufield_stat_partial_kernel(UField f, double threshold, int32_t* __restrict__ part_i, double* __restrict__ part_d) {
  const int t = threadIdx.x;
  const double inf = __builtin_huge_val();
  StatPart p = {0, 0, 0.0, inf, -inf};
  for (long long v = (long long)blockIdx.x * 256 + t; v < f.V; v += (long long)kStatBlocks * 256) {
    const double u = f.u[v];
    p.observed += f.c[v] > 0.0 ? 1 : 0;                                            // field.py:270
    p.high += u > threshold ? 1 : 0;                                               // field.py:271-273
    p.sum = p.sum + u;
    p.mn = nan_min(p.mn, u);
    p.mx = nan_max(p.mx, u);
  }
  stat_tree(p, t);
  if (t == 0) {
    const int b = blockIdx.x;
    part_i[2 * b] = p.observed; part_i[2 * b + 1] = p.high;
    part_d[3 * b] = p.sum; part_d[3 * b + 1] = p.mn; part_d[3 * b + 2] = p.mx;
  }
}

__global__ void __launch_bounds__(256)
ufield_stat_final_kernel(const int32_t* __restrict__ part_i, const double* __restrict__ part_d, int32_t* __restrict__ counts,
                         double* __restrict__ values) {
  const int t = threadIdx.x;                                                       // kStatBlocks == 256: one partial per lane
  StatPart p = {part_i[2 * t], part_i[2 * t + 1], part_d[3 * t], part_d[3 * t + 1], part_d[3 * t + 2]};
  stat_tree(p, t);
  if (t == 0) {
    counts[0] = p.observed; counts[1] = p.high;
    values[0] = p.sum; values[1] = p.mn; values[2] = p.mx;
  }
}

// ------------------------------------------------------------------------------------------------ regions: labelling
// The label of a component is the smallest raster index in it: the voxel at which the reference's raster scan (field.py:321-330) starts
// its flood fill, so ascending root label is the reference's discovery order whatever the schedule.
//
// Launch 1: a tile of kTile = 4 x 8 x 8 voxels (rows of 8 doubles along k) per workgroup, one lane per voxel.  Label equivalence in LDS:
// every voxel hands the smallest root among its six neighbours to its own root (an integer minimum), then all chains are shortened to
// their roots, until nothing changes.  Local indices order voxels of a tile as raster indices do.  The launch also resets the per-root
// facts of its voxels.
__global__ void __launch_bounds__(256)
ufield_label_tiles_kernel(UField f, double threshold, int tiles_j, int tiles_k, int32_t* __restrict__ labels, RegionFacts facts) {
  __shared__ int lab_s[kTileVoxels];
  __shared__ int changed;
  volatile int* lab = lab_s;
  const int t = threadIdx.x;
  const int tile = blockIdx.x;
  const int ti = tile / (tiles_j * tiles_k), tj = (tile / tiles_k) % tiles_j, tk = tile % tiles_k;
  const int li = t / (kTileJ * kTileK), lj = (t / kTileK) % kTileJ, lk = t % kTileK;
  const int i = ti * kTileI + li, j = tj * kTileJ + lj, k = tk * kTileK + lk;
  const bool inb = i < f.n[0] && j < f.n[1] && k < f.n[2];
  const int v = inb ? (i * f.n[1] + j) * f.n[2] + k : 0;
  const bool m = inb && f.u[v] > threshold;                                        // field.py:171
  lab[t] = m ? t : -1;
  if (inb) facts.reset(v);
  for (;;) {
    if (t == 0) changed = 0;
    __syncthreads();
    if (m) {
      const int r = lab[t];
      int best = r;
      if (li > 0) { const int o = lab[t - kTileJ * kTileK]; if (o >= 0 && o < best) best = o; }
      if (li < kTileI - 1) { const int o = lab[t + kTileJ * kTileK]; if (o >= 0 && o < best) best = o; }
      if (lj > 0) { const int o = lab[t - kTileK]; if (o >= 0 && o < best) best = o; }
      if (lj < kTileJ - 1) { const int o = lab[t + kTileK]; if (o >= 0 && o < best) best = o; }
      if (lk > 0) { const int o = lab[t - 1]; if (o >= 0 && o < best) best = o; }
      if (lk < kTileK - 1) { const int o = lab[t + 1]; if (o >= 0 && o < best) best = o; }
      if (best < r) {
        atomic_min_int(&lab_s[r], best);
        changed = 1;
      }
    }
    __syncthreads();
    if (m) {
      int l = lab[t];
      while (lab[l] != l) l = lab[l];
      lab[t] = l;
    }
    __syncthreads();
    const int again = changed;
    __syncthreads();
    if (!again) break;
  }
  if (inb) {
    int out = -1;
    if (m) {
      const int l = lab[t];
      const int ri = ti * kTileI + l / (kTileJ * kTileK), rj = tj * kTileJ + (l / kTileK) % kTileJ, rk = tk * kTileK + l % kTileK;
      out = (ri * f.n[1] + rj) * f.n[2] + rk;
    }
    labels[v] = out;
  }
}

// Launch 2: union-find across tile faces.  Only voxels on the low face of a tile along an axis do anything: the CAS traffic is that of the
// faces, not of the volume.  A union always links the larger root to the smaller, so the root of a component is its smallest index.
__global__ void __launch_bounds__(256)
ufield_merge_faces_kernel(UField f, int32_t* labels) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= f.V) return;
  int idx[3];
  raster_to_index(f, v, idx);
  const bool face[3] = {idx[0] > 0 && idx[0] % kTileI == 0, idx[1] > 0 && idx[1] % kTileJ == 0, idx[2] > 0 && idx[2] % kTileK == 0};
  if (!(face[0] || face[1] || face[2])) return;
  if (labels[v] < 0) return;                                                       // the sign of a label never changes
  const int stride[3] = {f.n[1] * f.n[2], f.n[2], 1};
  for (int a = 0; a < 3; ++a)
    if (face[a] && labels[v - stride[a]] >= 0) label_union(labels, v, v - stride[a]);
}

// Launch 3: every voxel ends at its root; voxel count and index bounding box per root, integer atomics only (order-free and exact).  A
// workgroup owns kFactSpan consecutive voxels; the voxels that share the workgroup's leading root are folded in LDS first, so a region of a
// million voxels costs seven atomics per workgroup.
constexpr int kFactSpan = 1024;

__global__ void __launch_bounds__(256)
ufield_flatten_facts_kernel(UField f, int32_t* labels, RegionFacts facts) {
  __shared__ int lead_s;
  __shared__ int acc[7][256];
  const int t = threadIdx.x;
  if (t == 0) lead_s = -1;
  __syncthreads();
  int root[kFactSpan / 256];
  for (int q = 0; q < kFactSpan / 256; ++q) {
    const long long v = (long long)blockIdx.x * kFactSpan + q * 256 + t;
    root[q] = -1;
    if (v < f.V && labels[v] >= 0) {
      int r = (int)v;
      for (int p = labels[r]; p != r; p = labels[r]) r = p;                        // roots are fixed in this launch; a chain read while
      labels[v] = r;                                                               // others shorten it still ends at the root
      root[q] = r;
      atomicCAS(&lead_s, -1, r);
    }
  }
  __syncthreads();
  const int lead = lead_s;
  int a[7] = {0, 0x7fffffff, 0x7fffffff, 0x7fffffff, -1, -1, -1};                  // count, min ijk, max ijk
  for (int q = 0; q < kFactSpan / 256; ++q) {
    if (root[q] < 0) continue;
    int idx[3];
    raster_to_index(f, (int)((long long)blockIdx.x * kFactSpan + q * 256 + t), idx);
    if (root[q] == lead) {
      a[0] += 1;
      for (int d = 0; d < 3; ++d) { a[1 + d] = idx[d] < a[1 + d] ? idx[d] : a[1 + d]; a[4 + d] = idx[d] > a[4 + d] ? idx[d] : a[4 + d]; }
    } else {
      facts.add(root[q], 1, idx, idx);
    }
  }
  for (int d = 0; d < 7; ++d) acc[d][t] = a[d];
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (t < h) {
      acc[0][t] += acc[0][t + h];
      for (int d = 1; d < 4; ++d) acc[d][t] = acc[d][t + h] < acc[d][t] ? acc[d][t + h] : acc[d][t];
      for (int d = 4; d < 7; ++d) acc[d][t] = acc[d][t + h] > acc[d][t] ? acc[d][t + h] : acc[d][t];
    }
    __syncthreads();
  }
  if (t == 0 && lead >= 0 && acc[0][0] > 0) {
    const int mn[3] = {acc[1][0], acc[2][0], acc[3][0]}, mx[3] = {acc[4][0], acc[5][0], acc[6][0]};
    facts.add(lead, acc[0][0], mn, mx);
  }
}

// ------------------------------------------------------------------------------------------------ regions: compaction
// Roots with count * res^3 >= min_volume (field.py:328) in ascending root order: a count per workgroup, a scan of the counts by one
// workgroup, a scatter -- three launches, nobody waits for a neighbour.  Lane t owns the four consecutive voxels 4t .. 4t + 3 of its span.
constexpr int kScanSpan = 1024;

__device__ __forceinline__ int qualifying(const UField& f, const int32_t* __restrict__ labels, const RegionFacts& facts, double cell, double min_volume,
                                          long long v) {
  if (v >= f.V || labels[v] != (int)v) return 0;
  return (double)facts.count[v] * cell >= min_volume ? 1 : 0;
}

// exclusive scan of one int per lane over the 256 lanes of a workgroup; *total = the sum
__device__ __forceinline__ int block_exclusive_scan(int x, int t, int* total) {
  __shared__ int s[2][256];
  int cur = 0;
  s[0][t] = x;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    s[1 - cur][t] = t >= d ? s[cur][t] + s[cur][t - d] : s[cur][t];
    cur = 1 - cur;
    __syncthreads();
  }
  const int incl = s[cur][t];
  *total = s[cur][255];
  __syncthreads();
  return incl - x;
}

__global__ void __launch_bounds__(256)
ufield_region_count_kernel(UField f, const int32_t* __restrict__ labels, RegionFacts facts, double cell, double min_volume, int32_t* __restrict__ span_count) {
  const int t = threadIdx.x;
  int n = 0;
  for (int q = 0; q < 4; ++q) n += qualifying(f, labels, facts, cell, min_volume, (long long)blockIdx.x * kScanSpan + 4 * t + q);
  int total;
  block_exclusive_scan(n, t, &total);
  if (t == 0) span_count[blockIdx.x] = total;
}

__global__ void __launch_bounds__(256)
ufield_region_scan_kernel(int spans, const int32_t* __restrict__ span_count, int32_t* __restrict__ span_offset, int max_regions, int32_t* __restrict__ counts) {
  const int t = threadIdx.x;
  int carry = 0;
  for (int base = 0; base < spans; base += 256) {
    const int x = base + t < spans ? span_count[base + t] : 0;
    int total;
    const int excl = block_exclusive_scan(x, t, &total);
    if (base + t < spans) span_offset[base + t] = carry + excl;
    carry += total;
  }
  if (t == 0) {
    counts[0] = carry < max_regions ? carry : max_regions;                         // rows written
    counts[1] = carry;                                                             // regions that qualify
  }
}

__global__ void __launch_bounds__(256)
ufield_region_scatter_kernel(UField f, const int32_t* __restrict__ labels, RegionFacts facts, double cell, double min_volume,
                             const int32_t* __restrict__ span_offset, int max_regions, int32_t* __restrict__ roots) {
  const int t = threadIdx.x;
  int flag[4], n = 0;
  for (int q = 0; q < 4; ++q) {
    flag[q] = qualifying(f, labels, facts, cell, min_volume, (long long)blockIdx.x * kScanSpan + 4 * t + q);
    n += flag[q];
  }
  int total;
  int rank = span_offset[blockIdx.x] + block_exclusive_scan(n, t, &total);
  for (int q = 0; q < 4; ++q) {
    if (!flag[q]) continue;
    if (rank < max_regions) roots[rank] = (int)((long long)blockIdx.x * kScanSpan + 4 * t + q);
    ++rank;
  }
}

// ------------------------------------------------------------------------------------------------ regions: float fold and finish
// One workgroup per kept region walks the region's bounding box in raster order, lanes strided, every lane adds its own voxels in that
// order, a fixed tree adds the lanes: no floating-point atomics, two runs give the same bytes.
__global__ void __launch_bounds__(256)
ufield_region_sum_kernel(UField f, const int32_t* __restrict__ labels, RegionFacts facts, const int32_t* __restrict__ counts,
                         const int32_t* __restrict__ roots, double* __restrict__ sums) {
  __shared__ double part[256];
  const int t = threadIdx.x, s = blockIdx.x;
  if (s >= counts[0]) return;
  const int root = roots[s];
  int lo[3], ext[3];
  for (int a = 0; a < 3; ++a) { lo[a] = facts.mn[3 * (size_t)root + a]; ext[a] = facts.mx[3 * (size_t)root + a] - lo[a] + 1; }
  const int total = ext[0] * ext[1] * ext[2];
  double acc = 0.0;
  for (int e = t; e < total; e += 256) {
    const int k = e % ext[2], j = (e / ext[2]) % ext[1], i = e / (ext[2] * ext[1]);
    const int v = ((lo[0] + i) * f.n[1] + lo[1] + j) * f.n[2] + lo[2] + k;
    if (labels[v] == root) acc = acc + f.u[v];
  }
  part[t] = acc;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (t < h) part[t] = part[t] + part[t + h];
    __syncthreads();
  }
  if (t == 0) sums[s] = part[0];
}

// One workgroup: the rows of field.py:385-405 in root order, then Python's stable sort(reverse=True) by priority (field.py:177) as a rank:
// the number of regions with a higher priority, or an equal one and a smaller root.  NaN priorities sort last, among themselves by root.
__global__ void __launch_bounds__(256)
ufield_region_finish_kernel(UField f, RegionFacts facts, double cell, const int32_t* __restrict__ counts, const int32_t* __restrict__ roots,
                            double* __restrict__ sums, double* __restrict__ rows, double* __restrict__ out, int32_t* __restrict__ out_roots) {
  const int t = threadIdx.x;
  const int n = counts[0];
  for (int s = t; s < n; s += 256) {
    const int root = roots[s];
    double* r = rows + 12 * (size_t)s;
    for (int a = 0; a < 3; ++a) {
      const double lo = ((double)facts.mn[3 * (size_t)root + a] + 0.5) * f.res + f.b0[a];
      const double hi = ((double)facts.mx[3 * (size_t)root + a] + 0.5) * f.res + f.b0[a];
      r[a] = (lo + hi) / 2.0;                                                      // field.py:388
      r[3 + a] = lo;
      r[6 + a] = hi;
    }
    const int count = facts.count[root];
    const double volume = (double)count * cell;                                    // field.py:389
    const double avg = sums[s] / (double)count;                                    // field.py:392-393
    const double priority = avg * log(1.0 + volume);                               // field.py:396
    r[9] = avg;
    r[10] = volume;
    r[11] = priority;
    sums[s] = priority;
  }
  __syncthreads();
  for (int s = t; s < n; s += 256) {
    const double p = sums[s];
    int rank = 0;
    for (int o = 0; o < n; ++o) {
      const double q = sums[o];
      const bool higher = q > p || (p != p && q == q);
      const bool equal = q == p || (p != p && q != q);
      rank += (higher || (equal && o < s)) ? 1 : 0;                                // roots[] ascends: o < s is "a smaller root"
    }
    for (int d = 0; d < 12; ++d) out[12 * (size_t)rank + d] = rows[12 * (size_t)s + d];
    if (out_roots != nullptr) out_roots[rank] = roots[s];
  }
}

// ------------------------------------------------------------------------------------------------ targets
// field.py:204-219: the centres of the first num_targets regions with z = max(z, 2.0); with a current position a stable sort by distance.
constexpr int kMaxTargets = 1024;

__global__ void __launch_bounds__(256)
ufield_targets_kernel(const double* __restrict__ regions, const int32_t* __restrict__ counts, int num_targets, bool have_position, double px,
                      double py, double pz, double* __restrict__ targets, int32_t* __restrict__ n_out) {
  __shared__ double dist[kMaxTargets];
  const int t = threadIdx.x;
  const int n = counts[0] < num_targets ? counts[0] : num_targets;
  for (int s = t; s < n; s += 256) {
    const double x = regions[12 * (size_t)s], y = regions[12 * (size_t)s + 1], z0 = regions[12 * (size_t)s + 2];
    const double z = 2.0 > z0 ? 2.0 : z0;                                          // Python's max(z, 2.0): a NaN z stays
    const double dx = x - px, dy = y - py, dz = z - pz;
    dist[s] = have_position ? sqrt((dx * dx + dy * dy) + dz * dz) : 0.0;
  }
  __syncthreads();
  for (int s = t; s < n; s += 256) {
    int rank = s;
    if (have_position) {
      rank = 0;
      const double p = dist[s];
      for (int o = 0; o < n; ++o) {
        const double q = dist[o];
        const bool lower = q < p || (p != p && q == q);
        const bool equal = q == p || (p != p && q != q);
        rank += (lower || (equal && o < s)) ? 1 : 0;
      }
    }
    const double z0 = regions[12 * (size_t)s + 2];
    targets[3 * (size_t)rank] = regions[12 * (size_t)s];
    targets[3 * (size_t)rank + 1] = regions[12 * (size_t)s + 1];
    targets[3 * (size_t)rank + 2] = 2.0 > z0 ? 2.0 : z0;
  }
  if (t == 0) n_out[0] = n;
}

// ------------------------------------------------------------------------------------------------ host side
// The int32 workspace of a grid of V voxels and max_regions rows, in words:
//   [0, 7V)            voxel count, min ijk, max ijk per root            (regions)
//   then 2 * spans     qualifying roots per span of 1024 voxels, their exclusive scan
//   then max_regions   the kept roots, ascending (padded to an even word)
//   then 2 * max_regions + 24 * max_regions      float64: sums / priorities, rows in root order
// The statistics partials (8 * kStatBlocks words) and the first-point table of the point updates (2V words) overlay its start.
struct UFieldLayout {
  long long spans, facts, span_count, span_offset, roots, sums, rows, words;
};

static UFieldLayout ufield_layout(long long V, long long max_regions) {
  UFieldLayout l;
  l.spans = (V + kScanSpan - 1) / kScanSpan;
  l.facts = 0;
  l.span_count = 7 * V;
  l.span_offset = l.span_count + l.spans;
  l.roots = l.span_offset + l.spans;
  l.sums = l.roots + max_regions;
  l.sums += l.sums & 1;
  l.rows = l.sums + 2 * max_regions;
  l.words = l.rows + 24 * max_regions;
  const long long stat_words = 8LL * kStatBlocks;
  if (l.words < stat_words) l.words = stat_words;
  return l;
}

// every factor and every partial product stays within kMaxVoxels, so nothing here can overflow
static bool grid_shape_ok(int nx, int ny, int nz) {
  if (nx < 1 || ny < 1 || nz < 1 || nx > kMaxVoxels || ny > kMaxVoxels || nz > kMaxVoxels) return false;
  const long long plane = (long long)nx * ny;
  return plane <= kMaxVoxels && plane * nz <= kMaxVoxels;
}

// stamps, points and positions per call: index + lane sums in the kernels and the launch grids stay ints
static bool count_ok(int n) { return n >= 0 && n <= kMaxCount; }

// NULL descriptor or grid: SE3MPC_ERR_NULL; sizes: SE3MPC_ERR_SHAPE; resolution / origin: SE3MPC_ERR_PARAM
static int check_field(const se3mpc_ufield* f, const char* what) {
  if (f == nullptr || f->uncertainty == nullptr || f->observation_count == nullptr) return reject(SE3MPC_ERR_NULL, what);
  if (!grid_shape_ok(f->n[0], f->n[1], f->n[2])) return reject(SE3MPC_ERR_SHAPE, what);
  if (!(f->resolution > 0.0) || !std::isfinite(f->resolution) || !std::isfinite(f->origin[0]) || !std::isfinite(f->origin[1]) ||
      !std::isfinite(f->origin[2]))
    return reject(SE3MPC_ERR_PARAM, what);
  return SE3MPC_OK;
}

static int check_workspace(const int32_t* workspace, long long have, long long need, const char* what) {
  if (workspace == nullptr) return reject(SE3MPC_ERR_NULL, what);
  if (have < need || ((uintptr_t)workspace & 7u) != 0) return reject(SE3MPC_ERR_WORKSPACE, what);
  return SE3MPC_OK;
}

}  // namespace se3mpc

using namespace se3mpc;

extern "C" long long se3mpc_ufield_workspace(int nx, int ny, int nz, int max_regions) {
  if (!grid_shape_ok(nx, ny, nz) || max_regions < 1 || !count_ok(max_regions)) return reject(SE3MPC_ERR_SHAPE, "se3mpc_ufield_workspace: grid sizes / max_regions");
  return ufield_layout((long long)nx * ny * nz, max_regions).words;
}

extern "C" int se3mpc_ufield_fill(const se3mpc_ufield* f, void* stream) {
  const int rc = check_field(f, "se3mpc_ufield_fill: field");
  if (rc) return rc;
  const UField d = make_ufield(*f);
  hipLaunchKernelGGL(ufield_fill_kernel, dim3(grid_for(d.V, 256)), dim3(256), 0, (hipStream_t)stream, d);
  return launch_status("se3mpc_ufield_fill");
}

extern "C" int se3mpc_ufield_stamp(const se3mpc_ufield* f, const double* centres, const double* radius, const int32_t* radius_voxels,
                                   const double* factor, int S, void* stream) {
  const int rc = check_field(f, "se3mpc_ufield_stamp: field");
  if (rc) return rc;
  if (!count_ok(S)) return reject(SE3MPC_ERR_SHAPE, "se3mpc_ufield_stamp: S outside [0, 2^30]");
  if (S == 0) return SE3MPC_OK;
  if (!centres || !radius || !radius_voxels || !factor) return reject(SE3MPC_ERR_NULL, "se3mpc_ufield_stamp: centres / radius / radius_voxels / factor");
  const UField d = make_ufield(*f);
  hipLaunchKernelGGL(ufield_stamp_kernel, dim3(grid_for(d.V, kStampSpan)), dim3(256), 0, (hipStream_t)stream, d, S, centres, radius, radius_voxels,
                     factor);
  return launch_status("se3mpc_ufield_stamp");
}

extern "C" int se3mpc_ufield_update_points(const se3mpc_ufield* f, const double* positions, const double* uncertainty, const double* weights, int N,
                                           double alpha, int32_t* keys, int32_t* workspace, long long workspace_words, void* stream) {
  const int rc = check_field(f, "se3mpc_ufield_update_points: field");
  if (rc) return rc;
  if (!count_ok(N)) return reject(SE3MPC_ERR_SHAPE, "se3mpc_ufield_update_points: N outside [0, 2^30]");
  if (!std::isfinite(alpha)) return reject(SE3MPC_ERR_PARAM, "se3mpc_ufield_update_points: alpha");
  if (N == 0) return SE3MPC_OK;
  if (!positions || !uncertainty || !keys) return reject(SE3MPC_ERR_NULL, "se3mpc_ufield_update_points: positions / uncertainty / keys");
  const UField d = make_ufield(*f);
  const int wrc = check_workspace(workspace, workspace_words, 2LL * d.V, "se3mpc_ufield_update_points: workspace");
  if (wrc) return wrc;
  unsigned long long* first = reinterpret_cast<unsigned long long*>(workspace);
  const dim3 grid(grid_for(N, 256)), block(256);
  hipLaunchKernelGGL(ufield_point_keys_kernel, grid, block, 0, (hipStream_t)stream, d, N, positions, keys, first);
  hipLaunchKernelGGL(ufield_point_first_kernel, grid, block, 0, (hipStream_t)stream, N, (const int32_t*)keys, first);
  hipLaunchKernelGGL(ufield_point_apply_kernel, grid, block, 0, (hipStream_t)stream, d, N, (const int32_t*)keys, (const unsigned long long*)first,
                     uncertainty, weights, alpha);
  return launch_status("se3mpc_ufield_update_points");
}

extern "C" int se3mpc_ufield_query(const se3mpc_ufield* f, const double* positions, int B, double* out, void* stream) {
  const int rc = check_field(f, "se3mpc_ufield_query: field");
  if (rc) return rc;
  if (!count_ok(B)) return reject(SE3MPC_ERR_SHAPE, "se3mpc_ufield_query: B outside [0, 2^30]");
  if (B == 0) return SE3MPC_OK;
  if (!positions || !out) return reject(SE3MPC_ERR_NULL, "se3mpc_ufield_query: positions / out");
  hipLaunchKernelGGL(ufield_query_kernel, dim3(grid_for(B, 256)), dim3(256), 0, (hipStream_t)stream, make_ufield(*f), B, positions, out);
  return launch_status("se3mpc_ufield_query");
}

extern "C" int se3mpc_ufield_statistics(const se3mpc_ufield* f, double threshold, int32_t* counts, double* values, int32_t* workspace,
                                        long long workspace_words, void* stream) {
  const int rc = check_field(f, "se3mpc_ufield_statistics: field");
  if (rc) return rc;
  if (!counts || !values) return reject(SE3MPC_ERR_NULL, "se3mpc_ufield_statistics: counts / values");
  const int wrc = check_workspace(workspace, workspace_words, 8LL * kStatBlocks, "se3mpc_ufield_statistics: workspace");
  if (wrc) return wrc;
  int32_t* part_i = workspace;
  double* part_d = reinterpret_cast<double*>(workspace + 2 * kStatBlocks);
  hipLaunchKernelGGL(ufield_stat_partial_kernel, dim3(kStatBlocks), dim3(256), 0, (hipStream_t)stream, make_ufield(*f), threshold, part_i, part_d);
  hipLaunchKernelGGL(ufield_stat_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const int32_t*)part_i, (const double*)part_d, counts, values);
  return launch_status("se3mpc_ufield_statistics");
}

extern "C" int se3mpc_ufield_regions(const se3mpc_ufield* f, double threshold, double min_volume, int max_regions, int32_t* labels, double* regions,
                                     int32_t* region_roots, int32_t* counts, int32_t* workspace, long long workspace_words, void* stream) {
  const int rc = check_field(f, "se3mpc_ufield_regions: field");
  if (rc) return rc;
  if (max_regions < 1 || !count_ok(max_regions)) return reject(SE3MPC_ERR_SHAPE, "se3mpc_ufield_regions: max_regions outside [1, 2^30]");
  if (!labels || !regions || !counts) return reject(SE3MPC_ERR_NULL, "se3mpc_ufield_regions: labels / regions / counts");
  const UField d = make_ufield(*f);
  const UFieldLayout l = ufield_layout(d.V, max_regions);
  const int wrc = check_workspace(workspace, workspace_words, l.words, "se3mpc_ufield_regions: workspace");
  if (wrc) return wrc;
  const RegionFacts facts = {workspace + l.facts, workspace + l.facts + d.V, workspace + l.facts + 4LL * d.V};
  int32_t* span_count = workspace + l.span_count;
  int32_t* span_offset = workspace + l.span_offset;
  int32_t* roots = workspace + l.roots;
  double* sums = reinterpret_cast<double*>(workspace + l.sums);
  double* rows = reinterpret_cast<double*>(workspace + l.rows);
  const double cell = std::pow(f->resolution, 3.0);                                // resolution ** 3, field.py:328, :389
  const int tiles[3] = {grid_for(d.n[0], kTileI), grid_for(d.n[1], kTileJ), grid_for(d.n[2], kTileK)};
  const int spans = (int)l.spans;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(ufield_label_tiles_kernel, dim3(tiles[0] * tiles[1] * tiles[2]), dim3(kTileVoxels), 0, st, d, threshold, tiles[1], tiles[2], labels,
                     facts);
  hipLaunchKernelGGL(ufield_merge_faces_kernel, dim3(grid_for(d.V, 256)), dim3(256), 0, st, d, labels);
  hipLaunchKernelGGL(ufield_flatten_facts_kernel, dim3(grid_for(d.V, kFactSpan)), dim3(256), 0, st, d, labels, facts);
  hipLaunchKernelGGL(ufield_region_count_kernel, dim3(spans), dim3(256), 0, st, d, (const int32_t*)labels, facts, cell, min_volume, span_count);
  hipLaunchKernelGGL(ufield_region_scan_kernel, dim3(1), dim3(256), 0, st, spans, (const int32_t*)span_count, span_offset, max_regions, counts);
  hipLaunchKernelGGL(ufield_region_scatter_kernel, dim3(spans), dim3(256), 0, st, d, (const int32_t*)labels, facts, cell, min_volume,
                     (const int32_t*)span_offset, max_regions, roots);
  hipLaunchKernelGGL(ufield_region_sum_kernel, dim3(max_regions), dim3(256), 0, st, d, (const int32_t*)labels, facts, (const int32_t*)counts,
                     (const int32_t*)roots, sums);
  hipLaunchKernelGGL(ufield_region_finish_kernel, dim3(1), dim3(256), 0, st, d, facts, cell, (const int32_t*)counts, (const int32_t*)roots, sums, rows,
                     regions, region_roots);
  return launch_status("se3mpc_ufield_regions");
}

extern "C" int se3mpc_ufield_targets(const double* regions, const int32_t* counts, int num_targets, const double* position, double* targets,
                                     int32_t* n_out, void* stream) {
  if (num_targets < 0 || num_targets > kMaxTargets) return reject(SE3MPC_ERR_SHAPE, "se3mpc_ufield_targets: num_targets outside [0, 1024]");
  if (!regions || !counts || !n_out || (num_targets > 0 && !targets)) return reject(SE3MPC_ERR_NULL, "se3mpc_ufield_targets: regions / counts / targets / n_out");
  const bool have = position != nullptr;
  hipLaunchKernelGGL(ufield_targets_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, regions, counts, num_targets, have, have ? position[0] : 0.0,
                     have ? position[1] : 0.0, have ? position[2] : 0.0, targets, n_out);
  return launch_status("se3mpc_ufield_targets");
}
