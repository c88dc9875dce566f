// Rendering a point cloud into the depth maps of V views: a z-buffer point splat, the inverse of the fusers' back-projection
// (specification: pointmvsnet_amd/render.py, include/pointflow_hip.h).  Pixel centres at
// (x + 0.5, y + 0.5) as in pf_camera.h, so the pixel that contains a projection (u, v) is (floor(u), floor(v)).
//
//   cloud_splat        one thread per point, 256 per block; the thread keeps its point in registers and walks ALL V views.
//                      The view index is the loop counter, so the 12 floats of a view's K [R | t] are wave-uniform and
//                      arrive by scalar loads into SGPRs; the only vector load is the point itself (12 bytes, once).  Per
//                      view: project (float32, the order written below, -ffp-contract=off), test depth and position as
//                      floats BEFORE any conversion to int (false for NaN, so every conversion is in range), then
//                      take the 64-bit unsigned minimum of (float_bits(z) << 32 | point index) on every cell of the
//                      (2 splat + 1)^2 footprint clamped to the map: z > 0, so the bit pattern orders like the value,
//                      the nearest point wins and among equal z the lowest index.  A minimum does not depend on the order
//                      of arrival: the result is a pure function of the input, and two runs give identical bytes.
//                      hipcc lowers atomicMin(unsigned long long*) to the no-return global_atomic_umin_x2; no float
//                      atomics, no compare-and-swap loop.
//                      A plain read of the cell before the atomic, skipping it when the key is not smaller, is safe only
//                      because the cell decreases monotonically: a stale read can cost an unnecessary atomic but can
//                      never cause a wrong skip.
//   cloud_zbuf_decode  one thread per cell: depth = the key's upper half as a float (0 where the cell is still all-ones),
//                      index = its lower half (-1 where empty; as a bit pattern for indices past 2^31, which is why a
//                      cloud stops at 2^32 - 2 points).
//
// Why the views are the inner loop and not blockIdx.y (UNMEASURED: chosen from the byte counts; tools/microbench_render.py
// times it).  With the view in blockIdx.y every view re-reads the cloud: 12 V bytes per point, 17.6 GB for 30 M points and
// 49 views, against 0.36 GB here -- the cloud is larger than the Infinity Cache, so those would be HBM bytes.  What is left
// either way is the scatter: up to (2 splat + 1)^2 8-byte atomics per (point, view) into V h w 8-byte cells (118 MB at 49
// views of 640 x 480: no XCD's 4 MB L2 holds it, whatever the order).  Neighbouring points of a fused or sampled cloud land
// in neighbouring pixels, so a wave's atomics of one view fall into few cache lines; the pre-read turns most of them into
// loads once a cell has seen a near point.  No rate is assumed for the 64-bit atomic minimum: none has been measured.
// No LDS, no scratch; every cell address is clamped into the map, whatever the matrices hold.
#include "pf_camera.h"

#include <math.h>

// (see scan_filter.hip: the host re-compilation of tests/hipemu reaches this file through eval_out.hip; its HIP shim has no
// 64-bit atomicMin, so there the two accesses are the host compiler's builtins)
#if defined(__HIP__)
#define PF_CR_PEEK(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define PF_CR_MIN(p, key) atomicMin((p), (key))
#else
#define PF_CR_PEEK(p) __atomic_load_n((p), __ATOMIC_RELAXED)
#define PF_CR_MIN(p, key) __atomic_fetch_min((p), (key), __ATOMIC_RELAXED)
#endif

namespace {

constexpr unsigned long long kCrEmpty = ~0ull;

__global__ __launch_bounds__(256) void cloud_splat_kernel(const float* __restrict__ points, int64_t N,
                                                          const float* __restrict__ proj, int V, int h, int w, int splat,
                                                          float depth_min, float depth_max,
                                                          unsigned long long* zbuf) {
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const float X = points[n * 3 + 0], Y = points[n * 3 + 1], Z = points[n * 3 + 2];
  const float s = (float)splat;
  const float ulim = (float)(w + splat), vlim = (float)(h + splat);
  const int64_t hw = (int64_t)h * w;
  for (int view = 0; view < V; ++view) {
    const float* __restrict__ p = proj + (int64_t)view * PF_RENDER_PROJ_FLOATS;      // wave-uniform: scalar loads
    const float qx = ((p[0] * X + p[1] * Y) + p[2] * Z) + p[3];
    const float qy = ((p[4] * X + p[5] * Y) + p[6] * Z) + p[7];
    const float z = ((p[8] * X + p[9] * Y) + p[10] * Z) + p[11];
    if (!(z > depth_min && z < depth_max)) continue;                               // false for NaN
    const float u = qx / z, v = qy / z;
    if (!(u >= -s && u < ulim && v >= -s && v < vlim)) continue;                   // as floats: the conversions are in range
    const int xc = (int)floorf(u), yc = (int)floorf(v);
    const int x0 = max(xc - splat, 0), x1 = min(xc + splat, w - 1);
    const int y0 = max(yc - splat, 0), y1 = min(yc + splat, h - 1);
    const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | (unsigned long long)(unsigned)n;
    unsigned long long* plane = zbuf + (int64_t)view * hw;
    for (int y = y0; y <= y1; ++y) {
      for (int x = x0; x <= x1; ++x) {
        unsigned long long* cell = plane + ((int64_t)y * w + x);
        if (key < PF_CR_PEEK(cell)) PF_CR_MIN(cell, key);
      }
    }
  }
}

__global__ __launch_bounds__(256) void cloud_zbuf_decode_kernel(const unsigned long long* __restrict__ zbuf, int64_t cells,
                                                                float* __restrict__ depth, int* __restrict__ index) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= cells) return;
  const unsigned long long key = zbuf[i];
  const bool empty = key == kCrEmpty;
  depth[i] = empty ? 0.0f : __uint_as_float((unsigned)(key >> 32));
  if (index != nullptr) index[i] = empty ? -1 : (int)(unsigned)key;
}

inline bool maps_ok(int V, int h, int w) {
  return V >= 0 && V <= 65535 && h >= 0 && w >= 0 && (int64_t)h * w <= INT32_MAX / 4 && pf_cdiv(h, kPfTile) <= 65535;
}

}  // namespace

extern "C" {

int pf_cloud_splat_f32(const float* points, int64_t N, const float* proj, int V, int h, int w, int splat, float depth_min,
                       float depth_max, uint64_t* zbuf, void* stream) {
  PF_REQUIRE(N >= 0 && N <= PF_RENDER_MAX_POINTS && maps_ok(V, h, w) && splat >= 0 && splat <= PF_RENDER_MAX_SPLAT);
  if (N == 0 || V == 0 || h == 0 || w == 0) return PF_OK;
  PF_REQUIRE(points && proj && zbuf);
  hipLaunchKernelGGL(cloud_splat_kernel, dim3((unsigned)pf_cdiv(N, 256)), dim3(256), 0, (hipStream_t)stream, points, N, proj,
                     V, h, w, splat, depth_min, depth_max, reinterpret_cast<unsigned long long*>(zbuf));
  return pf_launch_status();
}

int pf_cloud_zbuf_decode(const uint64_t* zbuf, int V, int h, int w, float* depth, int* index, void* stream) {
  PF_REQUIRE(maps_ok(V, h, w));
  const int64_t cells = (int64_t)V * h * w;
  if (cells == 0) return PF_OK;
  PF_REQUIRE(zbuf && depth && pf_cdiv(cells, 256) <= INT32_MAX);
  hipLaunchKernelGGL(cloud_zbuf_decode_kernel, dim3((unsigned)pf_cdiv(cells, 256)), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const unsigned long long*>(zbuf), cells, depth, index);
  return pf_launch_status();
}

}  // extern "C"
