// uncertainty_field_device.hpp -- the grid view, the index arithmetic and the integer atomics of uncertainty_field.hip.
// Contraction is off wherever this header is included (the including file's pragma): every operation that feeds a comparison rounds as
// NumPy rounds it.
#pragma once
#pragma clang fp contract(off)

#include "se3mpc_common.hpp"

namespace se3mpc {

constexpr int kTileI = 4, kTileJ = 8, kTileK = 8;           // the labelling tile: rows of 8 doubles along k, one lane per voxel
constexpr int kTileVoxels = kTileI * kTileJ * kTileK;
constexpr long long kMaxVoxels = 1LL << 30;                 // labels are int32 raster indices
constexpr int kMaxCount = 1 << 30;                          // stamps / points / positions / region rows per call
constexpr int kIndexClamp = 1 << 29;                        // |grid index| <= 2 * kIndexClamp, radius_in_voxels <= kIndexClamp: sums fit an int

// se3mpc_ufield by value (kernel argument): V = n0 * n1 * n2
struct UField {
  double* u;
  double* c;
  int n[3];
  int V;
  double b0[3];
  double res;
};

inline UField make_ufield(const se3mpc_ufield& f) {
  UField d;
  d.u = f.uncertainty;
  d.c = f.observation_count;
  for (int a = 0; a < 3; ++a) { d.n[a] = f.n[a]; d.b0[a] = f.origin[a]; }
  d.V = f.n[0] * f.n[1] * f.n[2];
  d.res = f.resolution;
  return d;
}

// np.floor((x - b0) / res).astype(int) along axis a (field.py:291-295), clamped so that index +- radius stays an int; NaN: far below
__device__ __forceinline__ int grid_index(const UField& f, double x, int a) {
  const double g = floor((x - f.b0[a]) / f.res);
  const double big = (double)(2 * kIndexClamp);
  if (!(g >= -big)) return -2 * kIndexClamp;
  return g > big ? 2 * kIndexClamp : (int)g;
}

// the raster index of the voxel that holds position p[3], -1 outside the grid (field.py:304-306)
__device__ __forceinline__ int voxel_of(const UField& f, const double* __restrict__ p) {
  int idx[3];
  for (int a = 0; a < 3; ++a) {
    idx[a] = grid_index(f, p[a], a);
    if (idx[a] < 0 || idx[a] >= f.n[a]) return -1;
  }
  return (idx[0] * f.n[1] + idx[1]) * f.n[2] + idx[2];
}

__device__ __forceinline__ void raster_to_index(const UField& f, int v, int* idx) {
  idx[2] = v % f.n[2];
  idx[1] = (v / f.n[2]) % f.n[1];
  idx[0] = v / (f.n[2] * f.n[1]);
}

// np.min / np.max: a NaN on either side wins
__device__ __forceinline__ double nan_min(double a, double b) { return (a < b || a != a) ? a : b; }
__device__ __forceinline__ double nan_max(double a, double b) { return (a > b || a != a) ? a : b; }

// integer minimum / maximum as a compare-and-swap loop (LDS or HBM); never waits for another lane
__device__ __forceinline__ void atomic_min_int(int* p, int v) {
  int old = *p;
  while (v < old) {
    const int seen = atomicCAS(p, old, v);
    if (seen == old) break;
    old = seen;
  }
}

__device__ __forceinline__ void atomic_max_int(int* p, int v) {
  int old = *p;
  while (v > old) {
    const int seen = atomicCAS(p, old, v);
    if (seen == old) break;
    old = seen;
  }
}

// per-root integer facts, indexed by the root's raster index: voxel count, index bounding box
struct RegionFacts {
  int32_t* count;   // [V]
  int32_t* mn;      // [V][3]
  int32_t* mx;      // [V][3]

  __device__ __forceinline__ void reset(int v) const {
    count[v] = 0;
    for (int a = 0; a < 3; ++a) { mn[3 * (size_t)v + a] = 0x7fffffff; mx[3 * (size_t)v + a] = -1; }
  }

  __device__ __forceinline__ void add(int root, int n, const int* lo, const int* hi) const {
    atomicAdd(&count[root], n);
    for (int a = 0; a < 3; ++a) {
      atomic_min_int(&mn[3 * (size_t)root + a], lo[a]);
      atomic_max_int(&mx[3 * (size_t)root + a], hi[a]);
    }
  }
};

// Union-find over the label array: labels[x] <= x is x's parent, a root has labels[r] == r.  The loads bypass the reading CU's L1 (another
// CU's compare-and-swap may have moved the root since); a stale parent would still be an ancestor, the CAS decides.
__device__ __forceinline__ int label_find(int32_t* labels, int x) {
  for (;;) {
    const int p = __atomic_load_n(&labels[x], __ATOMIC_RELAXED);
    if (p == x) return x;
    x = p;
  }
}

// always links the larger root to the smaller: the root of a component is its smallest raster index
__device__ __forceinline__ void label_union(int32_t* labels, int a, int b) {
  for (;;) {
    a = label_find(labels, a);
    b = label_find(labels, b);
    if (a == b) return;
    if (a < b) { const int s = a; a = b; b = s; }
    const int seen = atomicCAS(&labels[a], a, b);
    if (seen == a) return;
    a = seen;                                               // a was linked meanwhile: go on from its new parent
  }
}

}  // namespace se3mpc
