// The sorted sparse grid that cloud_eval.hip, cloud_filter.hip and mesh_distance.hip search (the comment at the top of
// cloud_eval.hip describes it): 16-byte point records, 63-bit cell keys, the binary search that finds a z-run, the float32
// distance, the walk over the cube of cells around a cell and the two passes of a nearest search, each stated once.
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

// the inverse of cell_key: a sorted record's cell is read from its key, never recomputed, so it cannot disagree with the sort
__device__ __forceinline__ void cell_of_key(int64_t key, int& cx, int& cy, int& cz) {
  cx = (int)(key >> (2 * kCoordBits));
  cy = (int)((key >> kCoordBits) & kCoordMask);
  cz = (int)(key & kCoordMask);
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

// ---- the walk ---------------------------------------------------------------------------------------------------------
// The cube of radius r cells around the cell (cx, cy, cz), clipped to the grid: per column (x, y) the cells z0 .. z1 are
// consecutive keys, so their records are one range of the sorted array -- one binary search, then a walk while the key stays
// inside the run.  (cx, cy, cz) may lie outside the grid (a query's clamped cell); a cube that misses the grid visits nothing.
// THE MARGIN every search on this grid keeps: cell arithmetic is float32 and can be off by rounding.  With at most 2^17 cells
// per axis (the host widens the cells of a larger cloud) a computed cell coordinate is within 2^-23 * 2^17 < 0.016 cells of
// the true quotient, so a record within (r - 0.05) cell edges of the query has its computed cell within r of the query's on
// every axis and the walk has met it.  Hence a best distance is trusted only when it is <= (r - 0.05) * edge, and a cube
// covers a radius R when (r - 0.05) * edge >= R.  (mesh_distance.hip adds the proof for a face listed by its box.)
// visit(j) is called for every record j of the cube, in key order; it returns false to end the whole walk.
template <class Visit>
__device__ __forceinline__ void walk_cube(const int64_t* __restrict__ keys, int n, int nx, int ny, int nz, int cx, int cy,
                                          int cz, int r, Visit visit) {
  const int z0 = max(cz - r, 0), z1 = min(cz + r, nz - 1);
  if (z0 > z1) return;
  for (int x = max(cx - r, 0); x <= min(cx + r, nx - 1); ++x) {
    for (int y = max(cy - r, 0); y <= min(cy + r, ny - 1); ++y) {
      const int64_t khi = cell_key(x, y, z1);
      for (int j = lower_bound(keys, n, cell_key(x, y, z0)); j < n && keys[j] <= khi; ++j) {
        if (!visit(j)) return;
      }
    }
  }
}

// The same columns for a whole wave: (cx, cy, cz, r) are uniform over the wave, a run is found by its two ends and lane
// `lane` visits every PF_WAVE-th record of it.  No early exit: the lanes merge what they found afterwards.
template <class Visit>
__device__ __forceinline__ void walk_cube_wave(const int64_t* __restrict__ keys, int n, int nx, int ny, int nz, int cx, int cy,
                                               int cz, int r, int lane, Visit visit) {
  const int z0 = max(cz - r, 0), z1 = min(cz + r, nz - 1);
  if (z0 > z1) return;
  for (int x = max(cx - r, 0); x <= min(cx + r, nx - 1); ++x) {
    for (int y = max(cy - r, 0); y <= min(cy + r, ny - 1); ++y) {
      const int j0 = lower_bound(keys, n, cell_key(x, y, z0));
      const int j1 = lower_bound(keys, n, cell_key(x, y, z1) + 1);
      for (int j = j0 + lane; j < j1; j += PF_WAVE) visit(j);
    }
  }
}

// ---- the nearest search in two passes ---------------------------------------------------------------------------------
// What is searched is a policy S passed by value with its pointers set (cloud_eval.hip: points, float32; mesh_distance.hip:
// faces, float64).  It holds the query and the running best: start(qx, qy, qz) takes the query and forgets the best,
// offer(j) holds record j against the best, within(reach) tells whether the best distance is <= the float32 length reach,
// merge(off) takes lane (lane ^ off)'s best where that is better, write(i, max_dist) stores query i's capped result.
//
// First pass, one thread per query on the fine grid: the cubes of radius 1, 3, .. `rings` cells around the query's cell;
// finished when the best lies inside the visited cube or the cube covers max_dist (the margin above).  The cell is clamped
// with rings + 1 cells of slack, so a query more than `rings` cells outside the grid meets no cell at all and stays
// unfinished.  done[i] tells the host which queries are left to the second pass.
template <class S>
__device__ __forceinline__ void nearest_cells_pass(S s, const float* __restrict__ query, int64_t nq,
                                                   const int64_t* __restrict__ keys, int n, const CloudGrid& g, int rings,
                                                   float max_dist, unsigned char* __restrict__ done) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nq) return;
  const float qx = query[i * 3 + 0], qy = query[i * 3 + 1], qz = query[i * 3 + 2];
  s.start(qx, qy, qz);
  const int cx = cell_coord(qx, g.ox, g.edge, -(rings + 1), g.nx + rings);
  const int cy = cell_coord(qy, g.oy, g.edge, -(rings + 1), g.ny + rings);
  const int cz = cell_coord(qz, g.oz, g.edge, -(rings + 1), g.nz + rings);
  bool finished = false;
  for (int r = 1; r <= rings && !finished; r += 2) {
    walk_cube(keys, n, g.nx, g.ny, g.nz, cx, cy, cz, r, [&](int j) {
      s.offer(j);
      return true;
    });
    const float reach = ((float)r - 0.05f) * g.edge;       // everything nearer than this has been visited
    finished = s.within(reach) || reach >= max_dist;
  }
  done[i] = finished ? 1 : 0;
  if (finished) s.write(i, max_dist);
}

// Second pass, one WAVE per unfinished query on a coarse grid whose edge the host has checked to be >= max_dist: the 27
// cells around the query's cell hold everything within max_dist, so the result is final.  The lanes stride over each run
// and merge their bests by xor shuffles; lane 0 writes.
template <class S>
__device__ __forceinline__ void nearest_wave_pass(S s, const float* __restrict__ query, const int64_t* __restrict__ todo,
                                                  int64_t ntodo, int64_t nq, const int64_t* __restrict__ keys, int n,
                                                  const CloudGrid& g, float max_dist) {
  const int64_t w = ((int64_t)blockIdx.x * 256 + threadIdx.x) / PF_WAVE;       // uniform over the wave
  const int lane = threadIdx.x & (PF_WAVE - 1);
  if (w >= ntodo) return;
  const int64_t i = todo[w];
  if (i < 0 || i >= nq) return;
  const float qx = query[i * 3 + 0], qy = query[i * 3 + 1], qz = query[i * 3 + 2];
  s.start(qx, qy, qz);
  const int cx = cell_coord(qx, g.ox, g.edge, -2, g.nx + 1);
  const int cy = cell_coord(qy, g.oy, g.edge, -2, g.ny + 1);
  const int cz = cell_coord(qz, g.oz, g.edge, -2, g.nz + 1);
  walk_cube_wave(keys, n, g.nx, g.ny, g.nz, cx, cy, cz, 1, lane, [&](int j) { s.offer(j); });
#pragma unroll
  for (int off = PF_WAVE / 2; off >= 1; off >>= 1) s.merge(off);
  if (lane == 0) s.write(i, max_dist);
}

inline bool grid_ok(int nx, int ny, int nz, float edge) {
  return nx >= 1 && ny >= 1 && nz >= 1 && nx <= PF_CLOUD_MAX_CELLS && ny <= PF_CLOUD_MAX_CELLS && nz <= PF_CLOUD_MAX_CELLS &&
         edge > 0.0f;
}

inline bool count_ok(int64_t n) { return n >= 0 && n <= PF_CLOUD_MAX_POINTS; }

inline unsigned blocks_of(int64_t n) { return (unsigned)pf_cdiv(n, 256); }

}  // namespace
