// Round-trip geometric consistency filter: the filtered depth maps of V views -> per-view masks, averaged depth maps and
// points (the check of the PyTorch MVS code bases that replaced fusibile; specification: pointmvsnet_amd/geometric.py,
// include/pointflow_hip.h).  Pixel centres at (x + 0.5, y + 0.5) as in fusion.hip.
//
//   geo_filter   one thread per pixel of every view, 16 x 16 pixel tiles like Stage A of fusion.hip (a wavefront = 16 x 4
//                pixels, so the four taps of its lanes in a source view land in a few neighbouring cache lines).  Per
//                listed source view: project the pixel, read the 2 x 2 depths around the projection, interpolate, project
//                that point back, test the round trip, add the returned depth.  The view index is blockIdx.z and the
//                source slot the loop counter, so the source table and both matrices of a pair are wave-uniform and are
//                read by scalar loads into SGPRs; the only vector loads are the pixel's own depth and the four gathers per
//                source.  No match array, no LDS, no scratch, no atomics: per pixel 4 bytes in, 4 M gathers of 4 bytes,
//                21 bytes out.
// The ordered compaction of the masked points is pf_fuse_compact_f32 (fusion.hip) behind the host's prefix sum.
// The layout of view_maps and of a pair row, the tiling and the map itself: pf_camera.h.
#include "pf_camera.h"

namespace {

__global__ __launch_bounds__(kPfTile * kPfTile) void geo_filter_kernel(
    const float* __restrict__ depth, const float* __restrict__ view_maps, const int* __restrict__ sources,
    const float* __restrict__ pair_maps, int V, int M, int h, int w, float pix_threshold, float rel_depth_threshold,
    int num_consistent, float depth_min, float depth_max, int* __restrict__ count, float* __restrict__ depth_avg,
    float* __restrict__ point, unsigned char* __restrict__ emit) {
  int x, y, i;
  pf_tile_pixel(x, y, i);
  if (x >= w || y >= h) return;
  const int hw = h * w;
  const int64_t ip = (int64_t)i * hw + y * w + x;
  const float d = depth[ip];
  const bool valid = d > depth_min && d < depth_max;
  const float px = (float)x + 0.5f, py = (float)y + 0.5f;
  const float xlast = (float)(w - 1), ylast = (float)(h - 1);
  float sum = d;
  int n = 0;
  for (int m = 0; m < M; ++m) {
    const int j = sources[(int64_t)i * M + m];
    if (j < 0 || j >= V || j == i) continue;           // wave-uniform: a pad, or the view itself
    const float* __restrict__ f = pair_maps + ((int64_t)i * M + m) * (2 * PF_FUSE_PAIR_FLOATS);   // i -> j
    const float* __restrict__ b = f + PF_FUSE_PAIR_FLOATS;                                         // j -> i
    float qx, qy, z;
    pf_apply_map(f, px, py, d, qx, qy, z);
    const float u = qx / z, v = qy / z;
    const float fx = u - 0.5f, fy = v - 0.5f;
    const float x0 = floorf(fx), y0 = floorf(fy);
    // all four taps inside the map, no border replication; false for NaN, so the conversions below are in range
    const bool inside = valid && z > 0.0f && x0 >= 0.0f && x0 + 1.0f <= xlast && y0 >= 0.0f && y0 + 1.0f <= ylast;
    const int q = inside ? (int)y0 * w + (int)x0 : 0;
    const float* __restrict__ plane = depth + (int64_t)j * hw;
    const float t00 = inside ? plane[q] : 0.0f;
    const float t01 = inside ? plane[q + 1] : 0.0f;
    const float t10 = inside ? plane[q + w] : 0.0f;
    const float t11 = inside ? plane[q + w + 1] : 0.0f;
    const bool readable = inside && t00 > depth_min && t00 < depth_max && t01 > depth_min && t01 < depth_max &&
                          t10 > depth_min && t10 < depth_max && t11 > depth_min && t11 < depth_max;
    const float wx = fx - x0, wy = fy - y0;
    const float top = t00 * (1.0f - wx) + t01 * wx;
    const float bot = t10 * (1.0f - wx) + t11 * wx;
    const float ds = top * (1.0f - wy) + bot * wy;
    float rx, ry, dr;
    pf_apply_map(b, u, v, ds, rx, ry, dr);
    const float ex = rx / dr - px, ey = ry / dr - py;
    const bool consistent = readable && dr > 0.0f && sqrtf(ex * ex + ey * ey) < pix_threshold &&
                            fabsf(dr - d) / d < rel_depth_threshold;
    if (consistent) {
      sum += dr;
      ++n;
    }
  }
  const bool keep = valid && n >= num_consistent;
  const float avg = keep ? sum / (float)(n + 1) : 0.0f;
  float X, Y, Z;
  pf_apply_map(view_maps + i * PF_FUSE_VIEW_FLOATS, px, py, avg, X, Y, Z);
  count[ip] = n;                                        // 0 without a depth of its own: `inside` asks for it
  depth_avg[ip] = avg;
  point[ip * 3 + 0] = keep ? X : 0.0f;
  point[ip * 3 + 1] = keep ? Y : 0.0f;
  point[ip * 3 + 2] = keep ? Z : 0.0f;
  emit[ip] = keep ? 1 : 0;
}

}  // namespace

extern "C" {

int pf_geo_filter_f32(const float* depth, const float* view_maps, const int* sources, const float* pair_maps, int V, int M,
                      int h, int w, float pix_threshold, float rel_depth_threshold, int num_consistent, float depth_min,
                      float depth_max, int* count, float* depth_avg, float* point, unsigned char* emit, void* stream) {
  PF_REQUIRE(V >= 1 && M >= 0 && h >= 0 && w >= 0 && (int64_t)h * w <= INT32_MAX / 4);
  PF_REQUIRE((pf_cdiv(h, kPfTile) <= 65535) && V <= 65535);
  if (h == 0 || w == 0) return PF_OK;
  PF_REQUIRE(depth && view_maps && count && depth_avg && point && emit && ((sources && pair_maps) || M == 0));
  hipLaunchKernelGGL(geo_filter_kernel, dim3((unsigned)pf_cdiv(w, kPfTile), (unsigned)pf_cdiv(h, kPfTile), (unsigned)V),
                     dim3(kPfTile * kPfTile), 0, (hipStream_t)stream, depth, view_maps, sources, pair_maps, V, M, h, w,
                     pix_threshold, rel_depth_threshold, num_consistent, depth_min, depth_max, count, depth_avg, point,
                     emit);
  return pf_launch_status();
}

}  // extern "C"
