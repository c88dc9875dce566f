// The sorted sparse grid that cloud_eval.hip and cloud_filter.hip search (the comment at the top of cloud_eval.hip describes
// it): 16-byte point records, 63-bit cell keys, the binary search that finds a z-run and the float32 distance, stated once.
// Everything sits in an anonymous namespace: each translation unit gets its own copy and the kernels keep their names.
#pragma once

#include "pf_common.h"

#include <math.h>

namespace {

struct __attribute__((aligned(16))) CloudPoint {
  float x, y, z;
  unsigned tag;
};

struct CloudGrid {
  float ox, oy, oz, edge;
  int nx, ny, nz;
};

constexpr int kCoordBits = 21;
constexpr int64_t kCoordMask = (1ll << kCoordBits) - 1;

__device__ __forceinline__ int64_t cell_key(int cx, int cy, int cz) {
  return ((int64_t)cx << (2 * kCoordBits)) | ((int64_t)cy << kCoordBits) | (int64_t)cz;
}

// floor((p - o) / edge) clamped to [lo, hi] (NaN goes to lo; the host rejects non-finite points)
__device__ __forceinline__ int cell_coord(float p, float o, float edge, int lo, int hi) {
  const float q = floorf((p - o) / edge);
  return (int)fminf(fmaxf(q, (float)lo), (float)hi);
}

// first j in [0, n] with keys[j] >= k
__device__ __forceinline__ int lower_bound(const int64_t* __restrict__ keys, int n, int64_t k) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < k) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ float dist2(float ax, float ay, float az, float bx, float by, float bz) {
  const float dx = ax - bx, dy = ay - by, dz = az - bz;
  return (dx * dx + dy * dy) + dz * dz;
}

inline bool grid_ok(int nx, int ny, int nz, float edge) {
  return nx >= 1 && ny >= 1 && nz >= 1 && nx <= PF_CLOUD_MAX_CELLS && ny <= PF_CLOUD_MAX_CELLS && nz <= PF_CLOUD_MAX_CELLS &&
         edge > 0.0f;
}

inline bool count_ok(int64_t n) { return n >= 0 && n <= PF_CLOUD_MAX_POINTS; }

inline unsigned blocks_of(int64_t n) { return (unsigned)pf_cdiv(n, 256); }

}  // namespace
