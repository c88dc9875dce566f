// Point-cloud evaluation (DTU accuracy / completeness, pointmvsnet_amd/evaluation.py): minimum-distance
// thinning of one cloud and nearest-neighbour distances between two unordered clouds of 10^6 .. 10^7 points.
//
// The data structure is a SPARSE uniform grid held as a sorted array.  A cloud's points get a 63-bit cell key
// (cx << 42 | cy << 21 | cz, cell = floor((p - origin) / edge) per axis in float32); the host sorts the keys (plumbing) and
// cloud_pack_kernel gathers the points into that order as 16-byte records (x, y, z, tag).  There is no cell table: the cells
// (cx, cy, z0 .. z1) of one grid column are CONSECUTIVE keys, so the points of a z-run are one contiguous range of the
// sorted array, found by one binary search on the per-point keys and walked until the key leaves the run.  A 3 x 3 x 3
// neighbourhood costs 9 searches.  That walk (walk_cube, walk_cube_wave), the margin every search keeps for the float32
// rounding of the cell coordinates (< 0.016 cells) and the two passes of the nearest search are stated in pf_cloud_grid.h.
// The thinning keeps the same margin through its grid's edge of 1.05 * min_dist: two points nearer than min_dist differ
// by < 0.99 in the quotient, so by at most 1 in the cell.
//
//   cloud_keys       one thread per point: the cell key.
//   cloud_pack       one thread per sorted slot: the point's record; tag = prio(original index) (thinning) or the index.
//   cloud_thin_round one round of the parallel form of the greedy thinning: an undecided point looks at its near
//                    neighbours of lower priority in the PREVIOUS round's states; it is removed if one is kept, kept if all
//                    are removed.  States are double-buffered, so the number of rounds is reproducible; the fixed point
//                    is the sequential greedy set whatever the order (a decision, once made, is the greedy walk's).
//   cloud_nn_cells / cloud_nn_wave   pf_cloud_grid.h's two passes over the point records (CloudNearest): a thread per query on
//                    the fine grid, a WAVE per unfinished query on the coarse grid (edge >= 1.05 * max_dist), minima by
//                    (distance, index).  The wave pass keeps the outliers (41^3 fine cells each) from setting the run time.
//   cloud_obs_mask / cloud_above_plane   the two DTU filters.
// No float atomics, no LDS, no scratch; every load is guarded by the array length.  Two runs give identical bytes.
#include "pf_cloud_grid.h"
#include "pf_hash.h"

namespace {

__global__ __launch_bounds__(256) void cloud_keys_kernel(const float* __restrict__ points, int64_t n, CloudGrid g,
                                                         int64_t* __restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int cx = cell_coord(points[i * 3 + 0], g.ox, g.edge, 0, g.nx - 1);
  const int cy = cell_coord(points[i * 3 + 1], g.oy, g.edge, 0, g.ny - 1);
  const int cz = cell_coord(points[i * 3 + 2], g.oz, g.edge, 0, g.nz - 1);
  keys[i] = cell_key(cx, cy, cz);
}

__global__ __launch_bounds__(256) void cloud_pack_kernel(const float* __restrict__ points, const int64_t* __restrict__ order,
                                                         int64_t n, int hashed, CloudPoint* __restrict__ packed) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t src = order[i];
  CloudPoint p;
  p.tag = hashed ? prio_hash((unsigned)src) : (unsigned)src;
  const bool ok = src >= 0 && src < n;
  p.x = ok ? points[src * 3 + 0] : 0.0f;
  p.y = ok ? points[src * 3 + 1] : 0.0f;
  p.z = ok ? points[src * 3 + 2] : 0.0f;
  packed[i] = p;
}

constexpr unsigned char kUndecided = 0, kKept = 1, kRemoved = 2;

__global__ __launch_bounds__(256) void cloud_thin_round_kernel(const CloudPoint* __restrict__ packed,
                                                               const int64_t* __restrict__ keys, int n, int nx, int ny, int nz,
                                                               float t, const unsigned char* __restrict__ state_in,
                                                               unsigned char* __restrict__ state_out, int* __restrict__ pending) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const unsigned char s = state_in[i];
  if (s != kUndecided) {
    state_out[i] = s;
    return;
  }
  const CloudPoint p = packed[i];
  int cx, cy, cz;
  cell_of_key(keys[i], cx, cy, cz);
  bool kept_near = false, undecided_near = false;
  walk_cube(keys, n, nx, ny, nz, cx, cy, cz, 1, [&](int j) {
    const CloudPoint q = packed[j];
    if (q.tag < p.tag && dist2(p.x, p.y, p.z, q.x, q.y, q.z) < t) {        // tags are a bijection of the index: j != i
      const unsigned char sj = state_in[j];
      kept_near |= sj == kKept;
      undecided_near |= sj == kUndecided;
    }
    return !kept_near;                                                     // one kept neighbour decides
  });
  const unsigned char out = kept_near ? kRemoved : (undecided_near ? kUndecided : kKept);
  state_out[i] = out;
  if (out == kUndecided) *pending = 1;                                     // every writer stores the same value
}

// nearest_distances' policy for pf_cloud_grid.h's two passes: float32 d2, ties to the lower tag (the original index)
struct CloudNearest {
  const CloudPoint* __restrict__ packed;
  float* __restrict__ dist;
  int* __restrict__ index;
  float qx, qy, qz, best;
  unsigned best_tag;

  __device__ __forceinline__ void start(float x, float y, float z) {
    qx = x, qy = y, qz = z;
    best = INFINITY;
    best_tag = 0xffffffffu;
  }
  __device__ __forceinline__ void take(float d2, unsigned tag) {
    if (d2 < best || (d2 == best && tag < best_tag)) {
      best = d2;
      best_tag = tag;
    }
  }
  __device__ __forceinline__ void offer(int j) {
    const CloudPoint p = packed[j];
    take(dist2(qx, qy, qz, p.x, p.y, p.z), p.tag);
  }
  __device__ __forceinline__ bool within(float reach) const { return best <= reach * reach; }
  __device__ __forceinline__ void merge(int off) {
    const float ob = __shfl_xor(best, off);
    const unsigned ot = __shfl_xor(best_tag, off);
    take(ob, ot);
  }
  __device__ __forceinline__ void write(int64_t i, float max_dist) const {
    const float d = fminf(sqrtf(best), max_dist);
    dist[i] = d;
    index[i] = d < max_dist ? (int)best_tag : -1;
  }
};

__global__ __launch_bounds__(256) void cloud_nn_cells_kernel(const float* __restrict__ query, int64_t nq,
                                                             const CloudPoint* __restrict__ packed,
                                                             const int64_t* __restrict__ keys, int nt, CloudGrid g, int rings,
                                                             float max_dist, float* __restrict__ dist, int* __restrict__ index,
                                                             unsigned char* __restrict__ done) {
  nearest_cells_pass(CloudNearest{packed, dist, index}, query, nq, keys, nt, g, rings, max_dist, done);
}

__global__ __launch_bounds__(256) void cloud_nn_wave_kernel(const float* __restrict__ query, const int64_t* __restrict__ todo,
                                                            int64_t ntodo, int64_t nq, const CloudPoint* __restrict__ packed,
                                                            const int64_t* __restrict__ keys, int nt, CloudGrid g,
                                                            float max_dist, float* __restrict__ dist,
                                                            int* __restrict__ index) {
  nearest_wave_pass(CloudNearest{packed, dist, index}, query, todo, ntodo, nq, keys, nt, g, max_dist);
}

__global__ __launch_bounds__(256) void cloud_obs_mask_kernel(const float* __restrict__ points, int64_t n,
                                                             const unsigned char* __restrict__ mask, int X, int Y, int Z,
                                                             float bx, float by, float bz, float res,
                                                             unsigned char* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float fx = floorf((points[i * 3 + 0] - bx) / res + 0.5f);
  const float fy = floorf((points[i * 3 + 1] - by) / res + 0.5f);
  const float fz = floorf((points[i * 3 + 2] - bz) / res + 0.5f);
  // the comparisons are false for NaN, so the conversions below are in range
  const bool inside = fx >= 0.0f && fx < (float)X && fy >= 0.0f && fy < (float)Y && fz >= 0.0f && fz < (float)Z;
  unsigned char v = 0;
  if (inside) v = mask[((int64_t)(int)fx * Y + (int)fy) * Z + (int)fz] != 0 ? 1 : 0;
  out[i] = v;
}

__global__ __launch_bounds__(256) void cloud_above_plane_kernel(const float* __restrict__ points, int64_t n, float a, float b,
                                                                float c, float d, unsigned char* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float s = ((a * points[i * 3 + 0] + b * points[i * 3 + 1]) + c * points[i * 3 + 2]) + d;
  out[i] = s > 0.0f ? 1 : 0;
}

}  // namespace

extern "C" {

int pf_cloud_cell_keys_f32(const float* points, int64_t n, float ox, float oy, float oz, float edge, int nx, int ny, int nz,
                           int64_t* keys, void* stream) {
  PF_REQUIRE(count_ok(n) && grid_ok(nx, ny, nz, edge));
  if (n == 0) return PF_OK;
  PF_REQUIRE(points && keys);
  const CloudGrid g = {ox, oy, oz, edge, nx, ny, nz};
  hipLaunchKernelGGL(cloud_keys_kernel, dim3(blocks_of(n)), dim3(256), 0, (hipStream_t)stream, points, n, g, keys);
  return pf_launch_status();
}

int pf_cloud_pack_f32(const float* points, const int64_t* order, int64_t n, int hashed, void* packed, void* stream) {
  PF_REQUIRE(count_ok(n));
  if (n == 0) return PF_OK;
  PF_REQUIRE(points && order && packed && ((uintptr_t)packed & 15) == 0);
  hipLaunchKernelGGL(cloud_pack_kernel, dim3(blocks_of(n)), dim3(256), 0, (hipStream_t)stream, points, order, n, hashed,
                     reinterpret_cast<CloudPoint*>(packed));
  return pf_launch_status();
}

int pf_cloud_thin_round(const void* packed, const int64_t* keys, int64_t n, int nx, int ny, int nz, float t,
                        const unsigned char* state_in, unsigned char* state_out, int* pending, void* stream) {
  PF_REQUIRE(count_ok(n) && grid_ok(nx, ny, nz, 1.0f));
  if (n == 0) return PF_OK;
  PF_REQUIRE(packed && keys && state_in && state_out && pending && state_in != state_out && ((uintptr_t)packed & 15) == 0);
  hipLaunchKernelGGL(cloud_thin_round_kernel, dim3(blocks_of(n)), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const CloudPoint*>(packed), keys, (int)n, nx, ny, nz, t, state_in, state_out, pending);
  return pf_launch_status();
}

int pf_cloud_nn_cells_f32(const float* query, int64_t nq, const void* packed, const int64_t* keys, int64_t nt, float ox,
                          float oy, float oz, float edge, int nx, int ny, int nz, int rings, float max_dist, float* dist,
                          int* index, unsigned char* done, void* stream) {
  PF_REQUIRE(count_ok(nq) && count_ok(nt) && nt >= 1 && grid_ok(nx, ny, nz, edge) && rings >= 1 && rings <= 15);
  if (nq == 0) return PF_OK;
  PF_REQUIRE(query && packed && keys && dist && index && done && ((uintptr_t)packed & 15) == 0);
  const CloudGrid g = {ox, oy, oz, edge, nx, ny, nz};
  hipLaunchKernelGGL(cloud_nn_cells_kernel, dim3(blocks_of(nq)), dim3(256), 0, (hipStream_t)stream, query, nq,
                     reinterpret_cast<const CloudPoint*>(packed), keys, (int)nt, g, rings, max_dist, dist, index, done);
  return pf_launch_status();
}

int pf_cloud_nn_wave_f32(const float* query, const int64_t* todo, int64_t ntodo, int64_t nq, const void* packed,
                         const int64_t* keys, int64_t nt, float ox, float oy, float oz, float edge, int nx, int ny, int nz,
                         float max_dist, float* dist, int* index, void* stream) {
  PF_REQUIRE(count_ok(nq) && count_ok(nt) && nt >= 1 && ntodo >= 0 && ntodo <= nq && grid_ok(nx, ny, nz, edge));
  PF_REQUIRE(edge >= max_dist);                     // the 27 cells must hold everything within max_dist
  if (ntodo == 0) return PF_OK;
  PF_REQUIRE(query && todo && packed && keys && dist && index && ((uintptr_t)packed & 15) == 0);
  const CloudGrid g = {ox, oy, oz, edge, nx, ny, nz};
  hipLaunchKernelGGL(cloud_nn_wave_kernel, dim3(blocks_of(ntodo * PF_WAVE)), dim3(256), 0, (hipStream_t)stream, query, todo,
                     ntodo, nq, reinterpret_cast<const CloudPoint*>(packed), keys, (int)nt, g, max_dist, dist, index);
  return pf_launch_status();
}

int pf_cloud_obs_mask_f32(const float* points, int64_t n, const unsigned char* mask, int X, int Y, int Z, float bx, float by,
                          float bz, float res, unsigned char* inside, void* stream) {
  PF_REQUIRE(count_ok(n) && X >= 1 && Y >= 1 && Z >= 1 && res > 0.0f);
  if (n == 0) return PF_OK;
  PF_REQUIRE(points && mask && inside);
  hipLaunchKernelGGL(cloud_obs_mask_kernel, dim3(blocks_of(n)), dim3(256), 0, (hipStream_t)stream, points, n, mask, X, Y, Z,
                     bx, by, bz, res, inside);
  return pf_launch_status();
}

int pf_cloud_above_plane_f32(const float* points, int64_t n, float a, float b, float c, float d, unsigned char* above,
                             void* stream) {
  PF_REQUIRE(count_ok(n));
  if (n == 0) return PF_OK;
  PF_REQUIRE(points && above);
  hipLaunchKernelGGL(cloud_above_plane_kernel, dim3(blocks_of(n)), dim3(256), 0, (hipStream_t)stream, points, n, a, b, c, d,
                     above);
  return pf_launch_status();
}

}  // extern "C"
