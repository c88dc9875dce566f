// Depth-map fusion: the filtered depth maps of V views -> one point cloud (the step reference tools/depthfusion.py:173-192
// hands to the external program fusibile; there is none for ROCm).  The specification is this project's own (DESIGN.md
// section 9, pointmvsnet_amd/fusion.py): pixel centres at (x + 0.5, y + 0.5) like get_pixel_grids, no normal test.
//
//   fuse_stage_a   one thread per pixel of every view, 16 x 16 pixel tiles (a wavefront = 16 x 4 pixels, so its gathers in
//                  a partner view land in a few neighbouring cache lines).  Back-projects the pixel, projects it into every
//                  other view in ascending order, reads the depth of the pixel that contains the projection, applies the
//                  disparity test and averages the consistent back-projections (and colours).  Gather-bound: per pixel and
//                  partner one 4-byte depth read at a data-dependent address, ~40 float operations.  The matrices of a view
//                  pair are wave-uniform (blockIdx.z and the loop counter index them), so they are read by scalar loads into
//                  SGPRs, not per lane.
//   fuse_mark      stage B for ONE view (the host launches the views in order): a pixel emits iff no earlier view has
//                  claimed it and it has enough consistent partners; an emitting pixel claims its matches.  used[view] is
//                  only read and used[other] only written (always 1) by a launch, so thread order cannot matter.
//   fuse_compact   ordered compaction: the host's inclusive prefix sum of the emit mask gives every emitting pixel its
//                  row; view-major, then row-major.  No atomics anywhere.
// The layout of view_maps and pair_maps, the tiling and the map itself: pf_camera.h.
#include "pf_camera.h"

namespace {

__global__ __launch_bounds__(kPfTile * kPfTile) void fuse_stage_a_kernel(
    const float* __restrict__ depth, const unsigned char* __restrict__ colour, const float* __restrict__ view_maps,
    const float* __restrict__ pair_maps, int V, int h, int w, float disp_threshold, float depth_min, float depth_max,
    int* __restrict__ count, float* __restrict__ point, unsigned char* __restrict__ colour_out, int* __restrict__ match) {
  int x, y, i;
  pf_tile_pixel(x, y, i);
  if (x >= w || y >= h) return;
  const int hw = h * w;
  const int p = y * w + x;
  const int64_t ip = (int64_t)i * hw + p;
  const float d = depth[ip];
  const bool valid = d > depth_min && d < depth_max;
  const float px = (float)x + 0.5f, py = (float)y + 0.5f;
  float sx = 0.0f, sy = 0.0f, sz = 0.0f, cr = 0.0f, cg = 0.0f, cb = 0.0f;
  if (valid) {
    pf_apply_map(view_maps + i * PF_FUSE_VIEW_FLOATS, px, py, d, sx, sy, sz);
    if (colour != nullptr) {
      cr = (float)colour[ip * 3 + 0];
      cg = (float)colour[ip * 3 + 1];
      cb = (float)colour[ip * 3 + 2];
    }
  }
  int n = 0, slot = 0;
  for (int j = 0; j < V; ++j) {
    if (j == i) continue;
    const float* __restrict__ m = pair_maps + ((int64_t)i * V + j) * PF_FUSE_PAIR_FLOATS;
    float qx, qy, z;
    pf_apply_map(m, px, py, d, qx, qy, z);
    const float u = qx / z, v = qy / z;
    // floor(u) in [0, w) <=> 0 <= u < w; the comparisons are false for NaN, so the conversions below are in range
    const bool inside = valid && z > 0.0f && u >= 0.0f && u < (float)w && v >= 0.0f && v < (float)h;
    const int xj = inside ? (int)u : 0, yj = inside ? (int)v : 0;
    const int q = yj * w + xj;
    const int64_t jq = (int64_t)j * hw + q;
    const float dj = inside ? depth[jq] : 0.0f;
    const float fb = m[12];
    const bool consistent = inside && dj > depth_min && dj < depth_max && fabsf(fb / z - fb / dj) < disp_threshold;
    match[((int64_t)i * (V - 1) + slot) * hw + p] = consistent ? q : -1;
    ++slot;
    if (consistent) {
      float X, Y, Z;
      pf_apply_map(view_maps + j * PF_FUSE_VIEW_FLOATS, (float)xj + 0.5f, (float)yj + 0.5f, dj, X, Y, Z);
      sx += X;
      sy += Y;
      sz += Z;
      if (colour != nullptr) {
        cr += (float)colour[jq * 3 + 0];
        cg += (float)colour[jq * 3 + 1];
        cb += (float)colour[jq * 3 + 2];
      }
      ++n;
    }
  }
  const float terms = (float)(n + 1);
  count[ip] = n;
  point[ip * 3 + 0] = sx / terms;
  point[ip * 3 + 1] = sy / terms;
  point[ip * 3 + 2] = sz / terms;
  if (colour_out != nullptr) {                       // sums of <= V bytes are exact; round to nearest (ties to even) once
    colour_out[ip * 3 + 0] = (unsigned char)rintf(cr / terms);
    colour_out[ip * 3 + 1] = (unsigned char)rintf(cg / terms);
    colour_out[ip * 3 + 2] = (unsigned char)rintf(cb / terms);
  }
}

__global__ __launch_bounds__(256) void fuse_mark_kernel(const int* __restrict__ count, const int* __restrict__ match,
                                                        unsigned char* __restrict__ used, unsigned char* __restrict__ emit,
                                                        int V, int view, int hw, int num_consistent) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= hw) return;
  const int64_t ip = (int64_t)view * hw + p;
  const bool e = used[ip] == 0 && count[ip] >= num_consistent;
  emit[ip] = e ? 1 : 0;
  if (!e) return;
  for (int slot = 0; slot < V - 1; ++slot) {
    const int q = match[((int64_t)view * (V - 1) + slot) * hw + p];
    const int j = slot < view ? slot : slot + 1;
    if (q >= 0 && q < hw) used[(int64_t)j * hw + q] = 1;
  }
}

__global__ __launch_bounds__(256) void fuse_compact_kernel(const unsigned char* __restrict__ emit,
                                                           const int64_t* __restrict__ rank, const float* __restrict__ point,
                                                           const unsigned char* __restrict__ colour, int64_t n, int64_t rows,
                                                           float* __restrict__ out_point,
                                                           unsigned char* __restrict__ out_colour) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || emit[i] == 0) return;
  const int64_t r = rank[i] - 1;                     // rank = inclusive prefix sum of emit
  if (r < 0 || r >= rows) return;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    out_point[r * 3 + c] = point[i * 3 + c];
    if (colour != nullptr) out_colour[r * 3 + c] = colour[i * 3 + c];
  }
}

}  // namespace

extern "C" {

int pf_fuse_stage_a_f32(const float* depth, const unsigned char* colour, const float* view_maps, const float* pair_maps,
                        int V, int h, int w, float disp_threshold, float depth_min, float depth_max, int* count,
                        float* point, unsigned char* colour_out, int* match, void* stream) {
  PF_REQUIRE(V >= 1 && h >= 0 && w >= 0 && (int64_t)h * w <= INT32_MAX / 4);
  PF_REQUIRE((pf_cdiv(h, kPfTile) <= 65535) && V <= 65535);
  if (h == 0 || w == 0) return PF_OK;
  PF_REQUIRE(depth && view_maps && pair_maps && count && point && (match || V == 1));
  PF_REQUIRE((colour == nullptr) == (colour_out == nullptr));
  hipLaunchKernelGGL(fuse_stage_a_kernel, dim3((unsigned)pf_cdiv(w, kPfTile), (unsigned)pf_cdiv(h, kPfTile), (unsigned)V),
                     dim3(kPfTile * kPfTile), 0, (hipStream_t)stream, depth, colour, view_maps, pair_maps, V, h, w,
                     disp_threshold, depth_min, depth_max, count, point, colour_out, match);
  return pf_launch_status();
}

int pf_fuse_mark(const int* count, const int* match, unsigned char* used, unsigned char* emit, int V, int view, int h,
                 int w, int num_consistent, void* stream) {
  PF_REQUIRE(V >= 1 && view >= 0 && view < V && h >= 0 && w >= 0 && (int64_t)h * w <= INT32_MAX / 4);
  if (h == 0 || w == 0) return PF_OK;
  PF_REQUIRE(count && used && emit && (match || V == 1));
  hipLaunchKernelGGL(fuse_mark_kernel, dim3((unsigned)pf_cdiv((int64_t)h * w, 256)), dim3(256), 0, (hipStream_t)stream,
                     count, match, used, emit, V, view, h * w, num_consistent);
  return pf_launch_status();
}

int pf_fuse_compact_f32(const unsigned char* emit, const int64_t* rank, const float* point, const unsigned char* colour,
                        int64_t n, int64_t rows, float* out_point, unsigned char* out_colour, void* stream) {
  PF_REQUIRE(n >= 0 && rows >= 0 && pf_cdiv(n, 256) <= INT32_MAX);
  if (n == 0 || rows == 0) return PF_OK;
  PF_REQUIRE(emit && rank && point && out_point && ((colour == nullptr) == (out_colour == nullptr)));
  hipLaunchKernelGGL(fuse_compact_kernel, dim3((unsigned)pf_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, emit, rank,
                     point, colour, n, rows, out_point, out_colour);
  return pf_launch_status();
}

}  // extern "C"
