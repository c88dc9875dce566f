// Cleaning a fused cloud (pointmvsnet_amd/cloud_filter.py): k-nearest statistics inside a radius for the
// statistical and the radius outlier tests, and a voxel-grid merge.  The search runs on cloud_eval.hip's sorted sparse grid
// (pf_cloud_grid.h) built by pf_cloud_cell_keys_f32 / pf_cloud_pack_f32 over the cloud itself with plain index tags.
//
//   cloud_knn_stats<K>  one thread per point IN SORTED ORDER (neighbouring threads walk the same z-runs); the thread's own
//                       record and key come from the sorted arrays and its cell from the key.  It visits the cube of radius
//                       r cells around its cell (walk_cube), r = 1, 2, ..: the K smallest d2 < R2 among the other points
//                       (other by TAG, so an exact duplicate counts at distance 0) sit in K registers, ascending: a candidate
//                       below the current worst is passed down the array by min / max, every index static.  A ring is final
//                       when the k-th best is <= (r - 0.05) cells (pf_cloud_grid.h's margin: nothing outside the cube can
//                       be nearer) or when that reach covers R; every ring starts over, so nothing is inserted twice.  The
//                       result -- a multiset and a fixed summation order -- does not depend on the order the candidates
//                       arrive in, hence not on the grid.  Results scatter back through the tag.
//   cloud_radius_count  the same walk, counting only; its visitor ends the walk once `limit` neighbours are found.
//   cloud_voxel_keys    one thread per point: the voxel key from floor((p - o) * inv), inv made by the host.
//   cloud_voxel_reduce  one thread per voxel over its run of the (stably) sorted order: float64 sums in ascending input
//                       index, integer colour sums; writes the voxel's row and its members' inverse-map entries.
// No float atomics, no LDS, no scratch; every load is guarded by the array length.  Two runs give identical bytes.
#include "pf_cloud_grid.h"

namespace {

template <int K>
__global__ __launch_bounds__(256) void cloud_knn_stats_kernel(const CloudPoint* __restrict__ packed,
                                                              const int64_t* __restrict__ keys, int n, int nx, int ny, int nz,
                                                              float edge, int k, float R, float R2, float* __restrict__ mean,
                                                              int* __restrict__ count) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const CloudPoint p = packed[i];
  int cx, cy, cz;
  cell_of_key(keys[i], cx, cy, cz);
  const int whole = max(nx, max(ny, nz));                  // a cube of this radius is the whole grid
  float a[K];
  int found = 0;
  bool finished = false;
  for (int r = 1; !finished; ++r) {
#pragma unroll
    for (int s = 0; s < K; ++s) a[s] = INFINITY;
    found = 0;
    walk_cube(keys, n, nx, ny, nz, cx, cy, cz, r, [&](int j) {
      const CloudPoint q = packed[j];
      float d = dist2(p.x, p.y, p.z, q.x, q.y, q.z);
      if (q.tag == p.tag || !(d < R2)) return true;
      ++found;
      if (d < a[K - 1]) {
#pragma unroll
        for (int s = 0; s < K; ++s) {
          const float lo = fminf(a[s], d);
          d = fmaxf(a[s], d);
          a[s] = lo;
        }
      }
      return true;
    });
    const float reach = ((float)r - 0.05f) * edge;         // everything nearer than this has been visited
    float kth = INFINITY;                                  // the k-th best, INFINITY while fewer are found
#pragma unroll
    for (int s = 0; s < K; ++s) {
      if (s == k - 1) kth = a[s];
    }
    finished = kth <= reach * reach || reach >= R || r >= whole;
  }
  if (p.tag >= (unsigned)n) return;
  const int c = min(found, k);
  float sum = 0.0f;                                        // 0 + sqrt(a_1) is sqrt(a_1): the stated sum
#pragma unroll
  for (int s = 0; s < K; ++s) {
    if (s < c) sum += sqrtf(a[s]);
  }
  mean[p.tag] = c == 0 ? R : (sum + (float)(k - c) * R) / (float)k;    // (k * R) / k is R only up to rounding
  if (count != nullptr) count[p.tag] = c;
}

__global__ __launch_bounds__(256) void cloud_radius_count_kernel(const CloudPoint* __restrict__ packed,
                                                                 const int64_t* __restrict__ keys, int n, int nx, int ny,
                                                                 int nz, float edge, int limit, float R, float R2,
                                                                 int* __restrict__ count) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const CloudPoint p = packed[i];
  int cx, cy, cz;
  cell_of_key(keys[i], cx, cy, cz);
  const int whole = max(nx, max(ny, nz));
  int found = 0;
  bool finished = false;
  for (int r = 1; !finished; ++r) {
    found = 0;
    walk_cube(keys, n, nx, ny, nz, cx, cy, cz, r, [&](int j) {
      const CloudPoint q = packed[j];
      if (q.tag != p.tag && dist2(p.x, p.y, p.z, q.x, q.y, q.z) < R2) ++found;
      return found < limit;                                // the walk ends at the limit-th neighbour: found <= limit
    });
    finished = found >= limit || ((float)r - 0.05f) * edge >= R || r >= whole;
  }
  if (p.tag < (unsigned)n) count[p.tag] = found;
}

// floor((p - o) * inv) clamped to [0, hi] (the host has checked that no point lies beyond hi)
__device__ __forceinline__ int voxel_coord(float p, float o, float inv, int hi) {
  const float q = floorf((p - o) * inv);
  return (int)fminf(fmaxf(q, 0.0f), (float)hi);
}

__global__ __launch_bounds__(256) void cloud_voxel_keys_kernel(const float* __restrict__ points, int64_t n, float ox, float oy,
                                                               float oz, float inv, int nx, int ny, int nz,
                                                               int64_t* __restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int cx = voxel_coord(points[i * 3 + 0], ox, inv, nx - 1);
  const int cy = voxel_coord(points[i * 3 + 1], oy, inv, ny - 1);
  const int cz = voxel_coord(points[i * 3 + 2], oz, inv, nz - 1);
  keys[i] = cell_key(cx, cy, cz);
}

__global__ __launch_bounds__(256) void cloud_voxel_reduce_kernel(const float* __restrict__ points,
                                                                 const unsigned char* __restrict__ colors,
                                                                 const float* __restrict__ normals,
                                                                 const int64_t* __restrict__ order,
                                                                 const int64_t* __restrict__ starts, int64_t n, int64_t m,
                                                                 float* __restrict__ out_points,
                                                                 unsigned char* __restrict__ out_colors,
                                                                 float* __restrict__ out_normals, int* __restrict__ out_counts,
                                                                 int64_t* __restrict__ inverse) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= m) return;
  const int64_t t0 = min(max(starts[s], (int64_t)0), n), t1 = min(max(starts[s + 1], t0), n);
  double px = 0.0, py = 0.0, pz = 0.0, ux = 0.0, uy = 0.0, uz = 0.0;
  unsigned long long cr = 0, cg = 0, cb = 0, members = 0;
  for (int64_t t = t0; t < t1; ++t) {
    const int64_t src = order[t];
    if (src < 0 || src >= n) continue;
    ++members;
    px += (double)points[src * 3 + 0];
    py += (double)points[src * 3 + 1];
    pz += (double)points[src * 3 + 2];
    if (colors != nullptr) {
      cr += colors[src * 3 + 0];
      cg += colors[src * 3 + 1];
      cb += colors[src * 3 + 2];
    }
    if (normals != nullptr) {
      ux += (double)normals[src * 3 + 0];
      uy += (double)normals[src * 3 + 1];
      uz += (double)normals[src * 3 + 2];
    }
    if (inverse != nullptr) inverse[src] = s;
  }
  const unsigned long long cnt = members > 0 ? members : 1;   // (an empty run cannot come from the host's segment starts)
  out_points[s * 3 + 0] = (float)(px / (double)cnt);
  out_points[s * 3 + 1] = (float)(py / (double)cnt);
  out_points[s * 3 + 2] = (float)(pz / (double)cnt);
  if (out_colors != nullptr && colors != nullptr) {
    out_colors[s * 3 + 0] = (unsigned char)((2 * cr + cnt) / (2 * cnt));
    out_colors[s * 3 + 1] = (unsigned char)((2 * cg + cnt) / (2 * cnt));
    out_colors[s * 3 + 2] = (unsigned char)((2 * cb + cnt) / (2 * cnt));
  }
  if (out_normals != nullptr && normals != nullptr) {
    const double len = sqrt((ux * ux + uy * uy) + uz * uz);
    const bool ok = len > 0.0;
    out_normals[s * 3 + 0] = ok ? (float)(ux / len) : 0.0f;
    out_normals[s * 3 + 1] = ok ? (float)(uy / len) : 0.0f;
    out_normals[s * 3 + 2] = ok ? (float)(uz / len) : 0.0f;
  }
  if (out_counts != nullptr) out_counts[s] = (int)members;
}

}  // namespace

extern "C" {

int pf_cloud_knn_stats_f32(const void* packed, const int64_t* keys, int64_t n, int nx, int ny, int nz, float edge, int k,
                           float radius, float radius2, float* mean, int* count, void* stream) {
  PF_REQUIRE(count_ok(n) && grid_ok(nx, ny, nz, edge) && k >= 1 && k <= PF_CLOUD_MAX_K && radius > 0.0f && radius2 > 0.0f);
  if (n == 0) return PF_OK;
  PF_REQUIRE(packed && keys && mean && ((uintptr_t)packed & 15) == 0);
  const CloudPoint* pk = reinterpret_cast<const CloudPoint*>(packed);
  const dim3 grid(blocks_of(n)), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (k <= 8) {
    hipLaunchKernelGGL(cloud_knn_stats_kernel<8>, grid, block, 0, s, pk, keys, (int)n, nx, ny, nz, edge, k, radius, radius2,
                       mean, count);
  } else if (k <= 16) {
    hipLaunchKernelGGL(cloud_knn_stats_kernel<16>, grid, block, 0, s, pk, keys, (int)n, nx, ny, nz, edge, k, radius, radius2,
                       mean, count);
  } else {
    hipLaunchKernelGGL(cloud_knn_stats_kernel<32>, grid, block, 0, s, pk, keys, (int)n, nx, ny, nz, edge, k, radius, radius2,
                       mean, count);
  }
  return pf_launch_status();
}

int pf_cloud_radius_count_f32(const void* packed, const int64_t* keys, int64_t n, int nx, int ny, int nz, float edge,
                              int limit, float radius, float radius2, int* count, void* stream) {
  PF_REQUIRE(count_ok(n) && grid_ok(nx, ny, nz, edge) && limit >= 1 && limit <= PF_CLOUD_MAX_K && radius > 0.0f &&
             radius2 > 0.0f);
  if (n == 0) return PF_OK;
  PF_REQUIRE(packed && keys && count && ((uintptr_t)packed & 15) == 0);
  hipLaunchKernelGGL(cloud_radius_count_kernel, dim3(blocks_of(n)), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const CloudPoint*>(packed), keys, (int)n, nx, ny, nz, edge, limit, radius, radius2,
                     count);
  return pf_launch_status();
}

int pf_cloud_voxel_keys_f32(const float* points, int64_t n, float ox, float oy, float oz, float inv, int nx, int ny, int nz,
                            int64_t* keys, void* stream) {
  PF_REQUIRE(count_ok(n) && grid_ok(nx, ny, nz, inv));
  if (n == 0) return PF_OK;
  PF_REQUIRE(points && keys);
  hipLaunchKernelGGL(cloud_voxel_keys_kernel, dim3(blocks_of(n)), dim3(256), 0, (hipStream_t)stream, points, n, ox, oy, oz, inv,
                     nx, ny, nz, keys);
  return pf_launch_status();
}

int pf_cloud_voxel_reduce_f32(const float* points, const unsigned char* colors, const float* normals, const int64_t* order,
                              const int64_t* starts, int64_t n, int64_t m, float* out_points, unsigned char* out_colors,
                              float* out_normals, int* out_counts, int64_t* inverse, void* stream) {
  PF_REQUIRE(count_ok(n) && m >= 0 && m <= n);
  if (m == 0) return PF_OK;
  PF_REQUIRE(points && order && starts && out_points && (colors == nullptr) == (out_colors == nullptr) &&
             (normals == nullptr) == (out_normals == nullptr));
  hipLaunchKernelGGL(cloud_voxel_reduce_kernel, dim3(blocks_of(m)), dim3(256), 0, (hipStream_t)stream, points, colors, normals,
                     order, starts, n, m, out_points, out_colors, out_normals, out_counts, inverse);
  return pf_launch_status();
}

}  // extern "C"
