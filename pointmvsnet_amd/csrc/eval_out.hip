// The step after the path: what reference utils/eval_file_logger.py:12-79 and
// tools/depthfusion.py:153-170 compute per depth map before files are written, on the device, so that the
// evaluation loop hands ONE staging buffer to an asynchronous D2H copy instead of stalling on .cpu().numpy()
// of every map (eval_file_logger.py:33-35,50,66).
//
//   eval_pack_map      a (h,w) map -> PFM row order (bottom row first: write_pfm's np.flipud, utils/io.py:124)
//   eval_flow_prob     (5,h,w) hypothesis probabilities -> the scalar confidence map of eval_file_logger.py:48-62:
//                      i = sum_d p_d*(d-2) + 2 in float64 (NumPy promotes: the offsets are a float64 array),
//                      conf = p[floor(i)] + p[min(floor(i)+1, 4)] in float32; PFM row order
//   eval_prob_filter   depth with pixels of low flow / initial confidence zeroed (depthfusion.py:166-167); the
//                      initial-confidence map may be smaller (nearest resize, cv2.INTER_NEAREST's index rule)
#include "pf_common.h"

namespace {

__global__ __launch_bounds__(256) void eval_pack_map_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                            int h, int w, int flip) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= h * w) return;
  const int y = i / w, x = i - y * w;
  dst[(flip ? h - 1 - y : y) * w + x] = src[i];
}

__global__ __launch_bounds__(256) void eval_flow_prob_kernel(const float* __restrict__ prob, float* __restrict__ dst,
                                                             int h, int w, int flip) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= h * w) return;
  const int y = i / w, x = i - y * w;
  dst[(flip ? h - 1 - y : y) * w + x] = pf_flow_confidence(prob, i, h * w);
}

__global__ __launch_bounds__(256) void eval_prob_filter_kernel(const float* __restrict__ depth,
                                                               const float* __restrict__ flow_conf,
                                                               const float* __restrict__ init_conf, int h, int w,
                                                               int ih, int iw, float flow_thr, float init_thr,
                                                               float* __restrict__ dst, int flip) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= h * w) return;
  const int y = i / w, x = i - y * w;
  // cv2.resize(..., INTER_NEAREST): src = min(floor(dst * src_size / dst_size), src_size - 1)
  int sy = y, sx = x;
  if (ih != h || iw != w) {
    sy = (int)floor((double)y * ((double)ih / (double)h));
    sx = (int)floor((double)x * ((double)iw / (double)w));
    sy = sy > ih - 1 ? ih - 1 : sy;
    sx = sx > iw - 1 ? iw - 1 : sx;
  }
  float d = depth[i];
  if (flow_conf[i] < flow_thr) d = 0.0f;
  if (init_conf[sy * iw + sx] < init_thr) d = 0.0f;
  dst[(flip ? h - 1 - y : y) * w + x] = d;
}

}  // namespace

extern "C" {

int pf_eval_pack_map_f32(const float* src, float* dst, int h, int w, int flip_rows, void* stream) {
  PF_REQUIRE(h >= 0 && w >= 0 && (int64_t)h * w <= INT32_MAX);
  if (h == 0 || w == 0) return PF_OK;
  PF_REQUIRE(src && dst && src != dst);
  hipLaunchKernelGGL(eval_pack_map_kernel, dim3((unsigned)pf_cdiv((int64_t)h * w, 256)), dim3(256), 0,
                     (hipStream_t)stream, src, dst, h, w, flip_rows);
  return pf_launch_status();
}

int pf_eval_flow_prob_f32(const float* prob, float* dst, int h, int w, int flip_rows, void* stream) {
  PF_REQUIRE(h >= 0 && w >= 0 && (int64_t)h * w <= INT32_MAX);
  if (h == 0 || w == 0) return PF_OK;
  PF_REQUIRE(prob && dst);
  hipLaunchKernelGGL(eval_flow_prob_kernel, dim3((unsigned)pf_cdiv((int64_t)h * w, 256)), dim3(256), 0,
                     (hipStream_t)stream, prob, dst, h, w, flip_rows);
  return pf_launch_status();
}

int pf_eval_prob_filter_f32(const float* depth, const float* flow_conf, const float* init_conf, int h, int w, int ih,
                            int iw, float flow_threshold, float init_threshold, float* dst, int flip_rows,
                            void* stream) {
  PF_REQUIRE(h >= 0 && w >= 0 && ih >= 1 && iw >= 1 && (int64_t)h * w <= INT32_MAX);
  if (h == 0 || w == 0) return PF_OK;
  PF_REQUIRE(depth && flow_conf && init_conf && dst && dst != depth);
  hipLaunchKernelGGL(eval_prob_filter_kernel, dim3((unsigned)pf_cdiv((int64_t)h * w, 256)), dim3(256), 0,
                     (hipStream_t)stream, depth, flow_conf, init_conf, h, w, ih, iw, flow_threshold, init_threshold, dst,
                     flip_rows);
  return pf_launch_status();
}

}  // extern "C"

// A build that is not hipcc's (no __HIP__: the host re-compilation of tests/hipemu, whose list of sources is fixed) gets
// the next stage of the evaluation output, the fusion kernels, the scene input (preprocess.hip), the point-cloud
// evaluation (cloud_eval.hip), the scan's confidence filter (scan_filter.hip), the round-trip consistency filter
// (geo_filter.hip), the point-cloud renderer (cloud_render.hip), the normal maps (depth_normals.hip), the guided depth
// upsampling (depth_refine.hip), the depth maps' segments (depth_segments.hip), the photometric check (photo_filter.hip), the cloud cleaning
// (cloud_filter.hip), the meshing (tsdf.hip, sparse_tsdf.hip), the mesh rasteriser (mesh_render.hip), the mesh clean-up (mesh_ops.hip) and the
// point-to-mesh distances (mesh_distance.hip) and the mesh simplification (mesh_simplify.hip) with this unit, so that such a library exports the whole C ABI.  hipcc
// compiles fusion.hip, preprocess.hip, cloud_eval.hip, scan_filter.hip, geo_filter.hip, cloud_render.hip,
// depth_normals.hip, depth_refine.hip, depth_segments.hip, photo_filter.hip, cloud_filter.hip, tsdf.hip, sparse_tsdf.hip, mesh_render.hip, mesh_ops.hip, mesh_distance.hip and mesh_simplify.hip as units of
// their own
// (build.SOURCES) and never takes this branch.
#if !defined(__HIP__)
#include "fusion.hip"
#include "preprocess.hip"
#include "cloud_eval.hip"
#include "scan_filter.hip"
#include "geo_filter.hip"
#include "cloud_render.hip"
#include "depth_normals.hip"
#include "depth_refine.hip"
#include "depth_segments.hip"
#include "photo_filter.hip"
#include "cloud_filter.hip"
#include "tsdf.hip"
#include "sparse_tsdf.hip"
#include "mesh_render.hip"
#include "mesh_ops.hip"
#include "mesh_distance.hip"
#include "mesh_simplify.hip"
#endif
