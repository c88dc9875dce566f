/*
 * pointflow_hip.h  --  C ABI of libpointflow_hip.so (MI355X / gfx950 native PointFlow hot path).
 *
 * Drop-in boundary for the reference's operator layer.  The reference binds
 * its one native op through a pybind module taking at::Tensor by value
 * (reference pointmvsnet/functions/csrc/main.cpp:3-6, gather_knn.h:7-13); everything else on the path
 * is a chain of ATen calls.  This library exposes the same operators -- and the fused forms the
 * MI355X pipeline uses -- as plain `extern "C"` functions over raw device pointers, sizes and a
 * hipStream_t, with no torch types in any signature.  The Python host side
 * (pointmvsnet_amd/_lib.py) binds them with ctypes; INTEGRATION.md shows the stub a reference
 * maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name ends in `_host`;
 *   - `stream` is a hipStream_t passed as void*; work is enqueued on it and the call returns
 *     without synchronising (the reference launches on the default stream,
 *     gather_knn_kernel.cu:138 -- a latent bug that is not reproduced);
 *   - tensors are dense row-major float32 unless stated; indices are int64 as the reference API
 *     mandates (functions/gather_knn.py:10-24, utils/torch_utils.py:16-22);
 *   - return value: PF_OK, a negative PF_ERR_* for argument errors (nothing was launched), or a
 *     positive hipError_t;
 *   - out-of-range neighbour indices never fault: the access is skipped / clamped and a sticky
 *     device status bit is raised, readable with pf_check_status() (the reference uses a device
 *     assert, gather_knn_kernel.cu:85).
 */
#ifndef POINTFLOW_HIP_H_
#define POINTFLOW_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PF_OK 0
#define PF_ERR_INVALID_ARG (-1)
#define PF_ERR_UNSUPPORTED (-2)

#define PF_STATUS_BAD_INDEX 1u

#define PF_MAX_VIEWS 8
#define PF_GEMM_TILE 64 /* points per GEMM / stats tile */

/* ---- packed camera block consumed by pf_flow_features_f32 (floats, device) -----------------
 *  [0..8]   inverse of the reference-view intrinsic, row-major      (model.py:168-169)
 *  [9..17]  inverse of the reference-view rotation                   (model.py:57,177)
 *  [18..20] reference-view translation                                (model.py:56)
 *  [21..23] world-point mean, [24..26] std                            (model.py:46-48)
 *  [27 + 21*v .. ] view v: intrinsic K (9, row-major) then extrinsic [R|t] (12, row-major 3x4)
 */
#define PF_CAM_KREF_INV 0
#define PF_CAM_RREF_INV 9
#define PF_CAM_TREF 18
#define PF_CAM_MEAN 21
#define PF_CAM_STD 24
#define PF_CAM_VIEWS 27
#define PF_CAM_VIEW_STRIDE 21
#define PF_CAM_FLOATS(V) (PF_CAM_VIEWS + PF_CAM_VIEW_STRIDE * (V))

const char* pf_version(void);
const char* pf_error_string(int code);
/* Number of compute units / LDS bytes of the current device, and its gcnArchName. */
int pf_device_info(int* cu_count, int* lds_bytes_per_block, char* arch_host, int arch_len);
/* Diagnostics: a one-thread kernel that writes the constant-rate device clock (100 MHz ticks) to *slot when it
 * runs on `stream` -- a timestamp that can sit INSIDE a captured hipGraph, where events cannot (PF_TIMELINE=1). */
int pf_debug_timestamp(long long* slot, void* stream);
/* Synchronises `stream`, returns the sticky status bits in *status_host and clears them. */
int pf_check_status(unsigned* status_host, void* stream);

/* ---- row G : gather_knn ------------------------------------------------------------------
 * Replaces dgcnn_ext.gather_knn_forward / gather_knn_backward
 * (reference functions/csrc/gather_knn_kernel.cu:25-47 and :97-148).
 *   forward : out[b,c,n,j] = feature[b,c,index[b,n,j]]      feature (B,C,N), index (B,N,K), out (B,C,N,K)
 *   backward: grad_in[b,c,index[b,n,j]] += grad_out[b,c,n,j]  (grad_in is zeroed by the call) -- float atomics in
 *             arrival order like the reference's kernel when inv_order / inv_start are NULL; with the inverted index
 *             lists of pf_knn_inverse(index, K, B, N, ...) (further down) every grad_in element is one thread's sum
 *             over the slots that name it, in ascending slot order: no atomics, bit-reproducible.
 * float32 and float64 like the reference's AT_DISPATCH_FLOATING_TYPES (:134). */
int pf_gather_knn_forward_f32(const float* feature, const int64_t* index, float* out,
                              int64_t B, int64_t C, int64_t N, int64_t K, void* stream);
int pf_gather_knn_forward_f64(const double* feature, const int64_t* index, double* out,
                              int64_t B, int64_t C, int64_t N, int64_t K, void* stream);
int pf_gather_knn_backward_f32(const float* grad_out, const int64_t* index, float* grad_in,
                               int64_t B, int64_t C, int64_t N, int64_t K, const uint32_t* inv_order,
                               const uint32_t* inv_start, void* stream);
int pf_gather_knn_backward_f64(const double* grad_out, const int64_t* index, double* grad_in,
                               int64_t B, int64_t C, int64_t N, int64_t K, const uint32_t* inv_order,
                               const uint32_t* inv_start, void* stream);

/* ---- row K : lattice kNN -------------------------------------------------------------------
 * Replaces get_knn_3d (reference utils/torch_utils.py:16-61).  xyz is (B,3,D,H,W) addressed through
 * `strides_host` (5 element strides, host array) so the strided sub-lattice views of
 * model.py:251-252 need no copy.  Candidates are the kernel_size^3 window, zero outside the lattice;
 * d2 = (dx*dx + dy*dy) + dz*dz in float32 without contraction; ranking: smaller d2 first, ties by
 * smaller candidate code (the reference's tie order is unspecified).
 *   idx_out  (B, D*H*W, knn) int64 or NULL: n + offsets, one global clamp to [0, DHW-1] (torch_utils.py:55-59)
 *   code_out (B, D*H*W, knn) uint8 or NULL: the window candidate code of each pick (kernel_size<=5);
 *            at least one of the two must be given
 * Limits: kernel_size odd, <= 7; knn <= min(32, kernel_size^3). */
int pf_knn_lattice_f32(const float* xyz, const int64_t* strides_host, int64_t B, int64_t D, int64_t H,
                       int64_t W, int kernel_size, int knn, int64_t* idx_out, uint8_t* code_out,
                       void* stream);

/* ---- row W : the warp ----------------------------------------------------------------------
 * Replaces FeatureFetcher.forward (reference utils/feature_fetcher.py:13-60): p = R X + t,
 * (x/z, y/z, 1) K^T, bilinear sample at pixel index (u-.5, v-.5), zero padding, legacy
 * align_corners=True.  maps (B,V,C,H,W), pts (B,3,N), K (B,V,3,3),
 * E (B,V,3,4) or NULL (identity), out (B,V,C,N).  V <= PF_MAX_VIEWS.
 * backward: gradient w.r.t. the maps only (the grid is built under no_grad, :29); grad_maps is
 * zeroed by the call. */
int pf_fetch_forward_f32(const float* maps, const float* pts, const float* K, const float* E, float* out,
                         int64_t B, int64_t V, int64_t C, int64_t H, int64_t W, int64_t N, void* stream);
int pf_fetch_backward_f32(const float* grad_out, const float* pts, const float* K, const float* E,
                          float* grad_maps, int64_t B, int64_t V, int64_t C, int64_t H, int64_t W,
                          int64_t N, void* stream);

/* ---- rows W+V : fetch + variance over views --------------------------------------------------
 * Fuses FeatureFetcher with E[x^2]-E[x]^2 over V (reference model.py:102-111, :187-190); never
 * materialises (B,V,C,N).  ref_override != 0 reproduces model.py:103-106: view 0 contributes the
 * un-warped reference feature maps[b,0,c, n mod (H*W)].  out (B,C,N). */
int pf_fetch_variance_f32(const float* maps, const float* pts, const float* K, const float* E, float* out,
                          int64_t B, int64_t V, int64_t C, int64_t H, int64_t W, int64_t N,
                          int ref_override, void* stream);
/* The coarse stage's use of it (reference model.py:79-111): the points are the frustum of the reference view,
 * generated in the kernel instead of read -- point n = d*H*W + y*W + x is
 *   world = rinv[b] (depths[b,d] * kinv[b] (x+0.5, y+0.5, 1)^T - t[b])
 * (kinv, rinv row-major 3x3: inverse coarse intrinsics and inverse rotation of view 0; t its translation),
 * with ref_override semantics.  world != NULL also receives the points (B, 3, D*H*W), the model's
 * "world_points" output.  out (B, C, D*H*W). */
int pf_frustum_variance_f32(const float* maps, const float* kinv, const float* rinv, const float* t,
                            const float* depths, const float* K, const float* E, float* out, float* world,
                            int64_t B, int64_t V, int64_t C, int64_t H, int64_t W, int64_t D, void* stream);

/* The same on CHANNEL-LAST maps (B, V, H, W, C), C % 4 == 0 (pf_nchw_to_nhwc_f32 converts; a convolution may
 * also write that layout directly): 16 lanes per point read every bilinear tap as one contiguous C-float run,
 * the (C, D*H*W) volume is written in 256-byte rows through an LDS transpose.  Bit-identical results. */
int pf_frustum_variance_cl_f32(const float* maps_cl, const float* kinv, const float* rinv, const float* t,
                               const float* depths, const float* K, const float* E, float* out, float* world,
                               int64_t B, int64_t V, int64_t C, int64_t H, int64_t W, int64_t D, void* stream);
/* in (P, C, S) -> out (P, S, C): planar to channel-last for P images of S pixels. */
int pf_nchw_to_nhwc_f32(const float* in, float* out, int64_t P, int64_t C, int64_t S, void* stream);

/* ---- bilinear resize (align_corners = False), the F.interpolate of model.py:184 -------------
 * in (P, IH, IW) -> out (P, OH, OW). */
int pf_resize_bilinear_f32(const float* in, float* out, int64_t P, int64_t IH, int64_t IW, int64_t OH,
                           int64_t OW, void* stream);

/* The three pyramid levels of one flow iteration (model.py:180-186) in one launch: in_l (V, c_l, h_l, w_l)
 * -> out_l (V, h, w, c_l) CHANNEL-LAST, bilinear align_corners = False (a level already at (h, w) is
 * transposed only).  c_l % 4 == 0 (else PF_ERR_UNSUPPORTED); c_l == 0 skips a level.  in_scale / in_shift (host
 * arrays of three device pointers, or NULL; an entry may be NULL): rows (V, c_l) of the pending BatchNorm + ReLU of
 * level l -- the tower's raw convolution output is normalised texel by texel BEFORE it is interpolated, i.e. the
 * F.interpolate of relu(bn(x)) without the normalised map ever being written (reference nn/conv.py:62-77 + model.py:184). */
int pf_flow_pyramid_f32(const float* in1, int c1, int h1, int w1, const float* in2, int c2, int h2, int w2,
                        const float* in3, int c3, int h3, int w3, int V, int h, int w, float* out1, float* out2,
                        float* out3, const float* const* in_scale, const float* const* in_shift, void* stream);

/* ---- row F (+U, +T ordering) : flow feature assembly ------------------------------------------
 * One launch builds what reference model.py:153-204 builds with ~100 ATen calls, for batch item 0..0
 * (one scene): for the 5 hypotheses depth + i*interval, i=-2..2: un-project the pixel centres of the
 * (h,w) flow grid, project into every view, bilinear-fetch the three (already resized to (h,w)) pyramid
 * levels maps1/2/3 -- CHANNEL-LAST (V,h,w,c_l), c_l % 4 == 0, as pf_flow_pyramid_f32 writes them --
 * variance over views, append (world-mean)/std repeated 8x.
 * depth_in (dh,dw) is nearest-resized to (h,w) on the fly (model.py:153-158).  `interval` is a DEVICE pointer
 * to the hypothesis spacing (one float): scene constants live in device memory so that a captured
 * hipGraph of the whole forward can be replayed on a new scene by refreshing small buffers.
 * Points are written in SUB-GRID-MAJOR order for the test-mode tiling of model.py:231-267
 * (ratio r, G = r*r groups, Ng = 5*(h/r)*(w/r) points each; group g=(y%r)*r+(x%r), local index
 * d*(h/r)*(w/r) + (y/r)*(w/r) + (x/r)); r = 1 gives the plain (5,h,w) lattice.
 *   feature (G*Ng, c1+c2+c3+24) POINT-major (the first EdgeConv GEMM's A operand)    xyz (G, 3, Ng) */
int pf_flow_features_f32(const float* maps1, const float* maps2, const float* maps3, int c1, int c2, int c3,
                         int V, int h, int w, const float* depth_in, int dh, int dw, const float* interval,
                         const float* cam, int ratio, float* feature, float* xyz, void* stream);

/* ---- rows E0/E1/E2/M building blocks ----------------------------------------------------------
 * Points are organised as G groups of Ng points; a "tile" is PF_GEMM_TILE consecutive points of one
 * group; a launch uses T = pf_stat_blocks(G, Ng) blocks per group, each reducing its tiles into one
 * float64 partial (sum, sum of squares) per column -> deterministic BatchNorm statistics. */
int pf_stat_blocks(int G, int Ng);
/* Blocks per group used by pf_pointwise_gemm_f32 (128-point tiles); its partials are (G, Tg, Nc, 2). */
int pf_gemm_blocks(int G, int Ng);

/* BatchNorm (training mode) statistics -> affine, one job.  Reduces partials (G, T, pcols, 2) over the T blocks
 * of `groups_per_stat` consecutive groups, columns [col0, col0+C):  mean = S/count,
 * var = SS/count - mean^2 (biased, used to normalise), scale = gamma*rsqrt(var+eps),
 * shift = beta - mean*scale; written to scale/shift[s*ld_affine + c].  When running_mean != NULL the
 * running statistics are updated S times in group order exactly like S successive nn.BatchNorm
 * calls (momentum, unbiased variance with n = unbias_n; reference runs BN in train mode at test time,
 * test.py:58).  count = elements per STAT group behind the sums.
 * pf_bn_finalize_jobs_f32 runs 1..32 independent jobs in one launch (e.g. the central and the difference half of an
 * EdgeConv BatchNorm, reference networks.py:33-36); the jobs must write disjoint scale/shift/running-stat ranges. */
typedef struct pf_bn_job {
  const double* partials;
  int32_t T, pcols, col0, C;
  double count, unbias_n;
  const float* gamma;
  const float* beta;
  float* running_mean;
  float* running_var;
  float momentum, eps;
  int32_t G, groups_per_stat;
  float* scale;
  float* shift;
  int32_t ld_affine;
  /* != 0: scale / shift are rows 0 / 1 of a rows tensor (4, S, ld_affine) = [scale | shift | mean | invstd] -- shift =
   * scale + S * ld_affine -- and pf_bn_finalize_jobs_f32 also writes rows 2 / 3, the batch statistics a BatchNorm
   * BACKWARD needs (the training step).  Consumers that resolve the job themselves (`in_bn`) ignore it.  (The field
   * sits in what was the struct's tail padding: size and offsets of everything else are unchanged.) */
  int32_t rows4;
} pf_bn_job;
int pf_bn_finalize_jobs_f32(const pf_bn_job* jobs, int njobs, void* stream);

/* The finalize FOLDED INTO THE CONSUMER (`in_bn`, host pointer, of pf_pointwise_gemm_f32 / pf_conv2d_wide_f32 /
 * pf_flow_head_f32; csrc/pf_bn_resolve.h): instead of (in_scale, in_shift) rows the consumer gets the pf_bn_job of
 * the pending BatchNorm -- finished statistics rows `partials` (G, T, pcols, 2) of the PRODUCER launch, count,
 * gamma, beta, eps -- and every block computes the (scale, shift) of its statistic group itself while its first
 * loads are in flight (fixed summation order: bit-reproducible).  The job's scale / shift rows and running
 * statistics are NOT written by such a consumer: pf_bn_finalize_jobs_f32 on the same job, any time later and off
 * the critical path, does that.  A consumer that cannot resolve (shape outside its fast path, more than 4096
 * rows behind a statistic) runs the finalize itself, without the running-statistics update, into job.scale /
 * job.shift (which must then be valid) and proceeds with those rows. */

/* Y[m, 0:Nc_store] = act(X[m, 0:K]) * Wt, m over G*Ng points.  Wt is (K, Nc) row-major, Nc in
 * {32, 64, 128}.  X is channel-major (G, K, Ng) when x_point_major == 0 (the reference (B,C,N) layout)
 * or point-major rows of ldx floats.  act = ReLU(x*in_scale[s,k] + in_shift[s,k]) when in_scale != NULL
 * (s = g / groups_per_stat) -- the previous layer's BatchNorm+ReLU fused into the load -- else identity.
 * col_partials (G, pf_gemm_blocks(G,Ng), Nc, 2) float64 or NULL receives per-block column sums of Y. */
int pf_pointwise_gemm_f32(const float* X, int x_point_major, int64_t ldx, const float* Wt, float* Y,
                          int64_t ldy, int G, int Ng, int K, int Nc, int Nc_store, const float* in_scale,
                          const float* in_shift, const pf_bn_job* in_bn, int groups_per_stat, double* col_partials,
                          void* stream);

/* Pass A of EdgeConv: for rows LE = [l (C) | e (C)] (point-major, ldle floats per point) and local
 * neighbour indices idx (G, Ng, k): partial sums over all (point, neighbour) pairs of
 * d = e[idx] - l and d*d per channel -> partials (G, T, C, 2) float64.   C in {32, 64, 128}.
 * Neighbourhood, two forms (both passes): `idx` (G, Ng, k) int64 group-local indices -- the reference's
 * tensor (functions/gather_knn.py:10-24) -- or, when `codes` != NULL (then idx may be NULL and k must be 16),
 * the window codes pf_knn_lattice_f32 wrote, (G, Ng, 16) uint8: neighbour j of point n is
 * clamp(n + (pd-hk)*lat_h*lat_w + (ph-hk)*lat_w + (pw-hk), 0, Ng-1) with code = (pd*lat_ks + ph)*lat_ks + pw,
 * hk = lat_ks/2 -- get_knn_3d's own index arithmetic (utils/torch_utils.py:51-59) done on the fly, so the six
 * gather passes of a PointFlow iteration read 16 instead of 128 index bytes per point.  lat_ks in {3, 5}. */
int pf_edge_stats_f32(const float* LE, int64_t ldle, int C, const int64_t* idx, int k, int G, int Ng,
                      double* partials, const uint8_t* codes, int lat_ks, int lat_h, int lat_w, void* stream);

/* Both passes have a lean form for the launches the flow stage makes, with the address work of a point done once and
 * shared by its lanes; it computes the same bits.  1 when a launch with these arguments takes it: window codes
 * (has_codes != 0), k == 16, C in {32, 64}, ldle == 2C, and Ng * ldle * 4 < 2^32 (a group's rows are addressed with
 * 32-bit byte offsets); 0 when it runs the general kernels. */
int pf_edge_lean_supported(int C, int k, int64_t ldle, int Ng, int has_codes);

/* Pass B of EdgeConv (reference networks.py:37-43 / :74-79):
 *   concat != 0: Y[m, 0:C]  = relu(l*scale[0:C] + shift[0:C])                       (central half)
 *                Y[m, C:2C] = mean_j relu((e[idx_j]-l)*scale[C:2C] + shift[C:2C])
 *   concat == 0: Y[m, 0:C]  = mean_j relu((e[idx_j]-l)*scale[0:C] + shift[0:C])
 * scale/shift are (S, ld_affine).  Y is point-major with ldy floats per point. */
int pf_edge_apply_f32(const float* LE, int64_t ldle, int C, const int64_t* idx, int k, int G, int Ng,
                      const float* scale, const float* shift, int ld_affine, int groups_per_stat,
                      int concat, float* Y, int64_t ldy, const uint8_t* codes, int lat_ks, int lat_h, int lat_w,
                      void* stream);

/* ---- EdgeConv backward (training, BASELINE config 4) ------------------------------------------------
 * Gradient of pf_edge_apply's output w.r.t. the rows LE = [l | e] through the train-mode BatchNorm, without
 * the (N, k, C) edge tensor the reference's autograd keeps (networks.py:18-45; its scatter is
 * functions/csrc/gather_knn_kernel.cu:50-89): both passes recompute d = e[idx] - l.
 * grad_y (G*Ng, ldg) point-major: [G_central C | G_diff C] (concat) or [G_diff C]; scale/shift/mean/invstd
 * rows (S, ld_affine) in the same column order (scale = gamma*invstd, shift = beta - mean*scale of the
 * forward; mean / invstd = its batch statistics).
 * Two walks over the neighbourhoods.  With g = [u > 0] * G / k (central half: [u > 0] * G), c1 = dbeta/M, c2 = dgamma/M
 * (M = elements behind the statistics of that column: gps*Ng*k for the difference half, gps*Ng for the central one),
 * dl = -sum_j dd_j is linear in (c1, c2): dl = -a * ((sum_j g_j - k * c1) - c2 * sum_j xhat_j), so the first walk can
 * leave every point's own sums behind and the forward lists are walked once.
 *   sums  : partials (G, pf_stat_blocks(G,Ng), cols, 2) float64, cols = 2C | C, per column (sum g, sum g*xhat)
 *           -> dbeta, dgamma; and grad_le (G*Ng, ldle): row n = [sum_j g_j (C) | sum_j xhat_j (C)].
 *           grad_acc (G*Ng, ld_acc) or NULL: a second upstream gradient in grad_y's column order (the next layer's data
 *           gradient, model.py:209-216's chain); the pass uses grad_y + grad_acc and stores that sum back into grad_acc,
 *           which the caller hands to `finish` as its grad_y (one element-wise launch less per layer).
 *   finish: (after pf_edge_backward_coeffs_f32: c1, c2 rows (S, ld_affine)) the gather over the inverted lists
 *           (inv_order / inv_start of pf_knn_inverse below) writes de -- point m sums dd over the pairs that gathered
 *           it, in ascending pair order -- AND turns the row's sums into dl (+ the central half of a concat layer):
 *           grad_le = [dl | de], columns [0, 2C) of every row written with plain stores, bit-reproducible (the
 *           reference's scatter uses float atomics).
 * C in {32, 64}.
 * plane: points per lattice plane (H*W of the D x H x W lattice the neighbours come from) or 0 = unknown -- a hint for
 * the XCD-aware block order only (each of the 8 L2s serves a band of pixel rows in every plane instead of every eighth
 * tile of the whole lattice); results do not depend on it.  pf_edge_stats_f32 / pf_edge_apply_f32 take the same hint as
 * (lat_ks 0, lat_h, lat_w) when they are given an index tensor instead of window codes. */
int pf_edge_backward_sums_f32(const float* LE, int64_t ldle, int C, const int64_t* idx, int k, int G, int Ng,
                              const float* grad_y, int64_t ldg, const float* scale, const float* shift,
                              const float* mean, const float* invstd, int ld_affine, int groups_per_stat, int concat,
                              double* partials, float* grad_le, float* grad_acc, int64_t ld_acc, int plane,
                              void* stream);
int pf_edge_backward_finish_f32(const float* LE, int64_t ldle, int C, int k, int G, int Ng, const float* grad_y,
                                int64_t ldg, const float* scale, const float* shift, const float* mean,
                                const float* invstd, const float* c1, const float* c2, int ld_affine,
                                int groups_per_stat, int concat, float* grad_le, const uint32_t* inv_order,
                                const uint32_t* inv_start, int plane, void* stream);

/* Between the two passes above: partials (G, pf_stat_blocks(G, Ng), cbn, 2) -> c1, c2 (G / groups_per_stat, cbn) =
 * the statistic set's (sum g', sum g' * xhat) / m in a fixed order (m = groups_per_stat * Ng points for the central
 * half [0, C) of a concat layer, * k pairs else), and dbeta / dgamma (cbn,) = the sums over the sets (NULL: not
 * wanted; accumulate != 0: added to what is there).  Replaces a dozen element-wise ATen launches per layer in the
 * training step (reference: autograd through networks.py:36-45). */
int pf_edge_backward_coeffs_f32(const double* partials, int G, int T, int cbn, int C, int concat, int groups_per_stat,
                                int Ng, int k, float* c1, float* c2, float* dgamma, float* dbeta, int accumulate,
                                void* stream);

/* The inverse of a neighbour index tensor idx (G, Ng, k) (csrc/knn_inverse.hip): order (G*Ng*k) = the pair ids
 * p = (g*Ng + n)*k + j grouped by their target row g*Ng + clamp(idx[p], 0, Ng-1); start (G*Ng + 1): the pairs
 * that gather row m are order[start[m] .. start[m+1]), in ascending p.  With (inv_order, inv_start)
 * pf_edge_backward_finish_f32 and pf_gather_knn_backward_* compute their scatter as a GATHER over those lists -- plain
 * stores in a fixed summation order, bit-reproducible -- instead of the float atomics of the reference's scatter
 * (functions/csrc/gather_knn_kernel.cu:50-89).  One inversion serves every layer that shares idx.  A counting sort in kernel launches only (no memset / memcpy nodes, no library call: capturable in a
 * hipGraph).  workspace: pf_knn_inverse_workspace(G, Ng, k) bytes of device scratch. */
int64_t pf_knn_inverse_workspace(int G, int Ng, int k);
int pf_knn_inverse(const int64_t* idx, int k, int G, int Ng, uint32_t* order, uint32_t* start, void* workspace,
                   int64_t workspace_bytes, void* stream);

/* ---- train-mode BatchNorm for the conv stacks around the path (ImageConv / VolumeConv) ----------
 * x (N, C, S) contiguous (NCHW / NCDHW with S = spatial size).  pf_channel_stats_f32 writes float64
 * partial (sum, sum of squares) per (sample, block, channel): partials (N, pf_norm_blocks(S), C, 2), the
 * layout pf_bn_finalize_jobs_f32 reduces (G = N samples; groups_per_stat samples pooled per statistic, e.g.
 * the batch of one reference conv call, nn/conv.py:29-35).  pf_channel_affine_f32 applies
 * y = x*scale[s,c] + shift[s,c] (s = n / samples_per_stat) with optional ReLU; y may alias x. */
int pf_norm_blocks(int64_t S);
int pf_channel_stats_f32(const float* x, int64_t N, int64_t C, int64_t S, double* partials, void* stream);
int pf_channel_affine_f32(const float* x, float* y, const float* scale, const float* shift, int64_t N, int64_t C,
                          int64_t S, int samples_per_stat, int relu, void* stream);
/* Finalize + normalise in one launch: every block reduces the partials (N, T, C, 2) of its own
 * (stat group, channel) in a fixed order, then streams y = act(gamma*(x-mean)*rsqrt(var+eps)+beta);
 * one block per channel applies the running-statistics recurrence over the N/samples_per_stat stat groups
 * in order.  count = elements per stat group (= samples_per_stat * S).  addend != NULL (same shape as x):
 * y = addend + act(...), the additive skip of VolumeConv's decoder (reference networks.py:166) in the same pass. */
int pf_channel_bn_apply_f32(const float* x, float* y, const double* partials, int T, int64_t N, int64_t C, int64_t S,
                            int samples_per_stat, double count, const float* gamma, const float* beta,
                            float* running_mean, float* running_var, float momentum, float eps, int relu,
                            const float* addend, void* stream);
/* The same for TWO convolution outputs at once: y = relu(bn2(x2)) + relu(bn1(x1)) (train-mode statistics from
 * partials1 / partials2, running statistics of both updated), y may alias x1 or x2 -- the last skip add of
 * VolumeConv's decoder (reference networks.py:166) as one pass over three streams. */
int pf_channel_bn_apply2_f32(const float* x1, const double* partials1, int T1, const float* gamma1, const float* beta1,
                             float* running_mean1, float* running_var1, float momentum1, float eps1, const float* x2,
                             const double* partials2, int T2, const float* gamma2, const float* beta2,
                             float* running_mean2, float* running_var2, float momentum2, float eps2, float* y, int64_t N,
                             int64_t C, int64_t S, int samples_per_stat, double count, void* stream);
/* Statistics + finalize + normalise in ONE launch for small tensors (one 1024-thread block per channel walks
 * the stat groups in order): y = act(BN_train(x)) with y == x allowed, and/or (y == NULL) only the affine
 * rows scale/shift (N/samples_per_stat, ld_affine) for a consumer that applies them itself.  Same
 * running-statistics semantics as pf_bn_finalize_jobs_f32. */
int pf_channel_bn_fused_f32(const float* x, float* y, int64_t N, int64_t C, int64_t S, int samples_per_stat,
                            const float* gamma, const float* beta, float* running_mean, float* running_var,
                            float momentum, float eps, int relu, float* scale, float* shift, int ld_affine,
                            void* stream);

/* ---- row R : 3x3x3 convolution of VolumeConv on the f32 matrix cores ---------------------------------
 * Replaces nn.Conv3d(k=3, padding=1, stride 1|2, bias=False) inside the Conv3d blocks of reference
 * networks.py:133-142 (nn/conv.py:108,115-121).  x (N,Cin,Di,Hi,Wi) NCDHW, Cin % 4 == 0, Cout <= 32;
 * wp = weights packed on the host as (Cin/4, 27 taps [kd][kh][kw], 4, 16*ceil(Cout/16)), zero padded:
 * wp[g][tap][k][co] = W[co][4g+k][kd][kh][kw];  y (N,Cout,Do,Ho,Wo).
 * partials (N, pf_conv3d_blocks(...), Cout, 2) float64 or NULL receives the per-block (sum, sum of
 * squares) of y per channel -- the BatchNorm batch statistics for free.
 * in_scale / in_shift (N / samples_per_stat, Cin) or in_bn: the pending BatchNorm + ReLU of x, applied while a
 * channel is staged (zero padding after it) -- rows, or resolved by the launch itself ("the finalize folded into
 * the consumer" above); all NULL: x is taken as it is. */
int pf_conv3d_blocks(int64_t Cin, int64_t Cout, int64_t Di, int64_t Hi, int64_t Wi, int stride);
/* The launch plan pf_conv3d_k3_f32 uses for a shape, for tests that pin it (a pure function of the shape, computed by
 * the function the launch itself calls): plan8 = {column tiles of 16 output channels NT, tile depth TD, tiles per
 * sample, tiles per block, blocks per sample, dynamic LDS bytes, 0, 0}. */
int pf_conv3d_plan(int64_t Cin, int64_t Cout, int64_t Di, int64_t Hi, int64_t Wi, int stride, int* plan8);
int pf_conv3d_k3_f32(const float* x, const float* wp, float* y, int64_t N, int64_t Cin, int64_t Cout, int64_t Di,
                     int64_t Hi, int64_t Wi, int stride, const float* in_scale, const float* in_shift,
                     const pf_bn_job* in_bn, int samples_per_stat, double* partials, void* stream);
/* The same convolution for stride 1 and Cout <= 8 (VolumeConv's conv0_1, networks.py:136: 64 -> 8 on the full cost
 * volume) without the half-empty 16-wide tile: N = 8 channels x 2 adjacent output rows, which read the same four
 * input rows, so K = 36 taps instead of 27 and 1.5x fewer MFMA cycles.  wp = weights packed as
 * (Cin/4, 36 taps [kd][kh'][kw], 4, 16): wp[g][tap][k][c + 8 s] = W[c][4g+k][kd][kh' - s][kw] (zero where kh' - s
 * is outside [0,2]).  partials (N, pf_conv3d_pair_blocks(...), Cout, 2) float64 or NULL as above. */
int pf_conv3d_pair_blocks(int64_t Cin, int64_t Cout, int64_t D, int64_t H, int64_t W);
int pf_conv3d_k3_pair_f32(const float* x, const float* wp, float* y, int64_t N, int64_t Cin, int64_t Cout, int64_t D,
                          int64_t H, int64_t W, double* partials, void* stream);
/* 3x3x3 / pad 1 / stride 1 conv3d with Cout <= 4 (VolumeConv's 8 -> 1 output layer, networks.py:147);
 * w is the unpacked (Cout, Cin, 3, 3, 3) weight. */
int pf_conv3d_k3_few_f32(const float* x, const float* w, float* y, int64_t N, int64_t Cin, int64_t Cout, int64_t D,
                         int64_t H, int64_t W, void* stream);

/* ConvTranspose3d 3x3x3, stride 2, padding 1, output_padding 1 (VolumeConv decoder, reference
 * networks.py:141-143 via nn/conv.py:189-216): y (N, Cout, 2D, 2H, 2W) from xa (+ xb when not NULL: the
 * decoder's skip add, networks.py:163-165) (N, Cin, D, H, W) and w (Cin, Cout, 3, 3, 3) in
 * nn.ConvTranspose3d's own layout.  partials != NULL: float64 (sum, sum of squares) per (sample, block,
 * channel), (N, pf_deconv3d_blocks(D, H, W), Cout, 2), the layout pf_channel_bn_apply_f32 consumes.
 * in_scale / in_shift (N / samples_per_stat, Cin) or in_bn: the pending BatchNorm + ReLU of xa (the previous
 * layer's raw output; Cin <= 64), applied to every loaded value BEFORE the skip add -- rows, or resolved by the
 * launch itself; all NULL: xa is taken as it is. */
int pf_deconv3d_blocks(int64_t D, int64_t H, int64_t W);
/* The form pf_deconv3d_k3s2_f32 takes for a shape, for tests that pin it (the launch's own selection, including the
 * environment switches PF_DECONV_MFMA / PF_DECONV_VALU): plan4 = {form (0 lane-per-cell, 1 matrix-core), output
 * channels per block CG, blocks of 128 input cells, 0}. */
int pf_deconv3d_plan(int64_t N, int64_t Cin, int64_t Cout, int64_t D, int64_t H, int64_t W, int* plan4);
int pf_deconv3d_k3s2_f32(const float* xa, const float* xb, const float* w, float* y, int64_t N, int64_t Cin,
                         int64_t Cout, int64_t D, int64_t H, int64_t W, const float* in_scale, const float* in_shift,
                         const pf_bn_job* in_bn, int samples_per_stat, double* partials, void* stream);

/* The bottom of VolumeConv's U-Net (reference networks.py:136-141) on volumes of a few thousand voxels, one launch
 * per layer (csrc/conv3d_bottom.hip): 3x3x3 / pad 1 convolutions 32 -> 64 stride 2 and 64 -> 64 stride 1, and the
 * ConvTranspose3d 64 -> 32 (3x3x3, stride 2, pad 1, output_padding 1: output = twice the input per dimension).
 * x (N, Cin, Di, Hi, Wi) -> y (N, Cout, Do, Ho, Wo); in_scale / in_shift / in_bn / samples_per_stat: the pending
 * BatchNorm + ReLU of the input as in pf_conv2d_wide_f32; partials (N, *_blocks(...), Cout, 2) float64 or NULL:
 * per-block sums of y and y*y.  Weights packed for the f32 matrix cores:
 *   conv   wp (3, 3, 3, Cin/16, 4, 64, 4):  wp[kd][kh][kw][kc][kq][co][j] = w[co][16 kc + 4 kq + j][kd][kh][kw]
 *   deconv wp (27, 4, 4, 32, 4):            wp[tap][kc][kq][co][j] = w[16 kc + 4 kq + j][co][tap]   (Cin-major
 *                                           weight of ConvTranspose3d, tap = (kd*3 + kh)*3 + kw)
 * PF_ERR_UNSUPPORTED for other channel counts (the *_supported functions tell). */
int pf_conv3d_bottom_supported(int64_t Cin, int64_t Cout, int stride);
int pf_conv3d_bottom_blocks(int64_t Di, int64_t Hi, int64_t Wi, int stride);
int pf_conv3d_bottom_f32(const float* x, const float* wp, float* y, int64_t N, int64_t Cin, int64_t Cout, int64_t Di,
                         int64_t Hi, int64_t Wi, int stride, const float* in_scale, const float* in_shift,
                         const pf_bn_job* in_bn, int samples_per_stat, double* partials, void* stream);
int pf_deconv3d_bottom_supported(int64_t Cin, int64_t Cout);
int pf_deconv3d_bottom_blocks(int64_t Di, int64_t Hi, int64_t Wi);
int pf_deconv3d_bottom_f32(const float* x, const float* wp, float* y, int64_t N, int64_t Cin, int64_t Cout, int64_t Di,
                           int64_t Hi, int64_t Wi, const float* in_scale, const float* in_shift, const pf_bn_job* in_bn,
                           int samples_per_stat, double* partials, void* stream);

/* ---- ImageConv: conv2d on the f32 matrix cores ------------------------
 * Replaces the nn.Conv2d of the Conv2d blocks of reference networks.py:89-110 (nn/conv.py:62-77) for the tower's
 * shapes: 3x3 / stride 1 / pad 1 (3->8, 3->16, 8->8, 16->16, 32->32, 64->64) and 5x5 / stride 2 / pad 2 (8->16, 16->32,
 * 32->64), bias-free (csrc/conv2d_wide.hip).  x (N,Cin,Hi,Wi) NCHW holds the RAW output of the previous conv when
 * in_scale / in_shift (N/sps, Cin) or in_bn (see "the finalize folded into the consumer" above) are given:
 * relu(x*scale+shift) -- the previous block's BatchNorm+ReLU -- is applied while staging, so that activation is
 * never written to memory; samples_per_stat consecutive samples share one affine row.  partials
 * (N, pf_conv2d_wide_blocks(...), Cout, 2) float64 or NULL receives the BatchNorm statistics of y (per-block sums
 * of y and y*y).  wp is the weight packed
 * (K, K, Cin/8, 2, Cout, 4): wp[kh][kw][kc][h][co][j] = w[co][8 kc + 4 h + j][kh][kw] for Cout 32 / 64, and
 * (K, K, 4, 16, Cin'/4), Cin' = Cin rounded up to 4: wp[kh][kw][kq][co][j] = w[co][(Cin'/4) kq + j][kh][kw] for
 * Cout 16 and the 3 -> 8 image layer (zero where co >= Cout or the channel does not exist), and for 8 -> 8 the PAIRED-ROWS
 * form (K + 1, K, 4, 16, Cin'/4): wp[kh'][kw][kq][co + 8 s][j] = w[co][(Cin'/4) kq + j][kh' - s][kw], zero where kh' - s
 * is outside [0, K): the 16 matrix columns are 8 channels x two adjacent output rows.
 * out_channel_last != 0 (Cout 32 / 64 only): y is written (N, Ho, Wo, Cout) -- the coarse tower's last layer
 * feeds pf_frustum_variance_cl_f32 directly, without the pf_nchw_to_nhwc_f32 pass.
 * PF_ERR_UNSUPPORTED for any other shape (pf_conv2d_wide_supported tells). */
int pf_conv2d_wide_supported(int64_t Cin, int64_t Cout, int kernel_size, int stride);
int pf_conv2d_wide_blocks(int64_t Cout, int64_t Hi, int64_t Wi, int stride);
int pf_conv2d_wide_f32(const float* x, const float* wp, float* y, int64_t N, int64_t Cin, int64_t Cout, int64_t Hi,
                       int64_t Wi, int kernel_size, int stride, const float* in_scale, const float* in_shift,
                       const pf_bn_job* in_bn, int samples_per_stat, double* partials, int out_channel_last,
                       void* stream);
/* The same launch over `sets` (1 or 2) PARAMETER SETS -- the model's two towers (coarse: model.py:71-77, flow:
 * model.py:140-148) have identical shapes and run on the same images, so each of their eleven layers is ONE launch:
 * samples [s*N/sets, (s+1)*N/sets) convolve with the packed weights at wp + s*wp_set_stride (floats, a multiple
 * of 4) and take their pending BatchNorm from in_bn[s] (an array of `sets` jobs; the (in_scale, in_shift) rows are
 * indexed by the global statistic group n / samples_per_stat as before).  x_layout says where sample
 * n = s*N/sets + i reads its input: 0 = sample n of x (N samples); 1 = sample i (x holds N/sets samples that
 * every set reads); 2 = sample i*sets + s (x is (N/sets, sets, Cin, Hi, Wi): what ONE convolution with the sets'
 * output channels stacked wrote -- the towers' first layer, 3 -> 8 + 8 on the same views, is a single
 * pf_conv2d_wide_f32 call with Cout = 16 and fills every column of the matrix tile).  Bit s of out_channel_last selects
 * the (Ho, Wo, Cout) layout for the samples of set s (each sample's region of y has the same size either way).
 * Per sample the arithmetic is that of pf_conv2d_wide_f32: results are bit-identical to `sets` separate calls. */
int pf_conv2d_wide_sets_f32(const float* x, int x_layout, const float* wp, int64_t wp_set_stride, int sets, float* y,
                            int64_t N, int64_t Cin, int64_t Cout, int64_t Hi, int64_t Wi, int kernel_size, int stride,
                            const float* in_scale, const float* in_shift, const pf_bn_job* in_bn, int samples_per_stat,
                            double* partials, int out_channel_last, void* stream);

/* ---- rows M (last layer) + H + T : flow head ---------------------------------------------------
 * Z (G*Ng, ldz) holds the pre-BN output of the 64->16 MLP layer.  Per pixel of the (h,w) grid:
 * a = relu(Z*scale+shift); flow_d = sum_c w_out[c]*a_c for the 5 hypotheses; p = softmax(-flow);
 * depth_out = nearest(depth_in) + sum_d p_d*(d-2)*interval  (reference model.py:218-227), written
 * back in image order (undoing the sub-grid-major point order, model.py:256-266).
 * flow_prob (5,h,w), depth_out (h,w). */
int pf_flow_head_f32(const float* Z, int64_t ldz, const float* scale, const float* shift, int ld_affine,
                     const pf_bn_job* in_bn, const float* w_out, const float* depth_in, int dh, int dw,
                     const float* interval, int h, int w, int ratio, float* flow_prob, float* depth_out,
                     void* stream);

/* ---- row S : soft-argmin + probability map -----------------------------------------------------
 * cost (B, D, HW) filtered cost volume; depth = sum_k linspace(start,end,D)[k] * softmax(-cost)[k]
 * (reference model.py:117-124); prob = p[floor(i)] + p[ceil(i)], i = (depth-start)/interval clamped
 * to [0, D-1] (functions/functions.py:141-175).  params (B,3) = (depth_start, depth_end, interval). */
int pf_softargmin_prob_f32(const float* cost, const float* params, float* depth, float* prob, int64_t B,
                           int64_t D, int64_t HW, void* stream);

/* ---- the step after the path: evaluation output + fusion pre-step -------------
 * Device-side halves of reference utils/eval_file_logger.py:12-79 and tools/depthfusion.py:153-170, writing into a
 * staging buffer in PFM row order (flip_rows != 0: bottom row first, the np.flipud of utils/io.py:124) so that one
 * asynchronous D2H copy per depth map feeds the file writer.
 *   pf_eval_pack_map_f32    src (h,w) -> dst (h,w) [row-flipped]
 *   pf_eval_flow_prob_f32   prob (5,h,w) -> confidence p[floor(i)] + p[min(floor(i)+1,4)], i = sum_d p_d (d-2) + 2
 *                           evaluated in float64 like NumPy does (eval_file_logger.py:48-62)
 *   pf_eval_prob_filter_f32 depth (h,w) with depth := 0 where flow_conf (h,w) < flow_threshold or
 *                           init_conf (ih,iw; nearest-resized, cv2.INTER_NEAREST's index rule) < init_threshold */
int pf_eval_pack_map_f32(const float* src, float* dst, int h, int w, int flip_rows, void* stream);
int pf_eval_flow_prob_f32(const float* prob, float* dst, int h, int w, int flip_rows, void* stream);
int pf_eval_prob_filter_f32(const float* depth, const float* flow_conf, const float* init_conf, int h, int w, int ih,
                            int iw, float flow_threshold, float init_threshold, float* dst, int flip_rows,
                            void* stream);

/* ---- depth-map fusion: filtered depth maps of V views -> one point cloud (csrc/fusion.hip) ---------------------
 * What reference tools/depthfusion.py:173-192 delegates to the external program fusibile.  The specification is this
 * project's own (pointmvsnet_amd/fusion.py): pixel (x, y) has its centre at (x + 0.5, y + 0.5),
 * no normal test.  All maps are (V, h, w) row-major, 0 = no depth; colours are (V, h, w, 3) bytes or NULL.
 * The host composes the matrices in float64 and passes them as float32:
 *   view_maps (V, PF_FUSE_VIEW_FLOATS): A = R^-1 K^-1 (3x3 row-major), C = -R^-1 t;  X = (A (x+.5, y+.5, 1)) d + C
 *   pair_maps (V, V, PF_FUSE_PAIR_FLOATS), entry [i][j]: M = K_j R_j R_i^-1 K_i^-1 (3x3), T = K_j (t_j - R_j R_i^-1 t_i),
 *             fb = K_j[0][0] |C_i - C_j|, 3 floats of padding;  q = (M (x+.5, y+.5, 1)) d + T
 * pf_fuse_stage_a_f32: per pixel p of view i with depth_min < d < depth_max and every other view j in ascending order:
 *   z = q.z, (xj, yj) = floor(q.xy / z); j is consistent iff z > 0, (xj, yj) is inside the map, d_j(xj, yj) is inside
 *   (depth_min, depth_max) and |fb / z - fb / d_j| < disp_threshold.  count (V,h,w) = consistent views; match
 *   (V, V-1, h, w) = yj * w + xj or -1 (slot = j, or j - 1 behind i); point (V,h,w,3) / colour_out (V,h,w,3) = mean of
 *   the pixel's own back-projection / colour and those of its matches (count + 1 terms; colour rounded to nearest).
 *   Pixels without depth: count 0, match -1, point 0.
 * pf_fuse_mark: stage B for view `view`, to be called for view = 0 .. V-1 in order on one stream with `used` (V,h,w)
 *   zeroed before the first call: emit[view][p] = (used[view][p] == 0 && count[view][p] >= num_consistent); an emitting
 *   pixel sets used[j][match] = 1 for each of its matches.
 * pf_fuse_compact_f32: rows of point / colour (n rows) whose emit byte is set -> out row rank[i] - 1, rank = the
 *   inclusive prefix sum of emit (int64); `rows` = rank[n-1] bounds the output. */
#define PF_FUSE_VIEW_FLOATS 12
#define PF_FUSE_PAIR_FLOATS 16
int pf_fuse_stage_a_f32(const float* depth, const unsigned char* colour, const float* view_maps, const float* pair_maps,
                        int V, int h, int w, float disp_threshold, float depth_min, float depth_max, int* count,
                        float* point, unsigned char* colour_out, int* match, void* stream);
int pf_fuse_mark(const int* count, const int* match, unsigned char* used, unsigned char* emit, int V, int view, int h,
                 int w, int num_consistent, void* stream);
int pf_fuse_compact_f32(const unsigned char* emit, const int64_t* rank, const float* point, const unsigned char* colour,
                        int64_t n, int64_t rows, float* out_point, unsigned char* out_colour, void* stream);

/* ---- round-trip geometric consistency filter (csrc/geo_filter.hip) ----------------------------------------------
 * The check of the PyTorch MVS code bases that followed the reference (MVSNet-pytorch, CasMVSNet): the reference has no
 * such step and OpenCV is not a dependency, so the specification is this project's own (pointmvsnet_amd/geometric.py,
 * DESIGN.md section 9).  Maps and pixel centres as above.  Only the listed pairs are composed:
 *   view_maps (V, PF_FUSE_VIEW_FLOATS) as above
 *   sources   (V, M) int32: the source views of view i in the order they are visited; -1 (a pad) and i itself are skipped
 *   pair_maps (V, M, 2, PF_FUSE_PAIR_FLOATS): entry [i][m][0] is the i -> j layout above for j = sources[i][m],
 *             entry [i][m][1] the same for j -> i (fb is not read)
 * pf_geo_filter_f32: per pixel p = (x, y) of view i with depth_min < d < depth_max, d = d_i(p), and listed source j:
 *   1. q = (M_ij (x+.5, y+.5, 1)) d + T_ij, (u, v) = q.xy / q.z; skip j if q.z <= 0
 *   2. (fx, fy) = (u - .5, v - .5), (x0, y0) = floor(fx, fy); skip j unless 0 <= x0, x0 + 1 <= w - 1, 0 <= y0,
 *      y0 + 1 <= h - 1 (no border replication) and the four taps d_j(y0.., x0..) are inside (depth_min, depth_max);
 *      ds = top (1 - wy) + bot wy, top = t00 (1 - wx) + t01 wx, bot = t10 (1 - wx) + t11 wx, wx = fx - x0, wy = fy - y0
 *   3. q' = (M_ji (u, v, 1)) ds + T_ji, d' = q'.z, (u', v') = q'.xy / d'
 *   4. j is consistent iff d' > 0, sqrt((u' - (x+.5))^2 + (v' - (y+.5))^2) < pix_threshold and
 *      |d' - d| / d < rel_depth_threshold
 *   count (V,h,w) = consistent sources; emit (V,h,w) = (count >= num_consistent); depth_avg (V,h,w) =
 *   (d + sum of the consistent d', in list order) / (count + 1) where emit, else 0; point (V,h,w,3) = the
 *   back-projection of p at depth_avg where emit, else 0.  Pixels without depth: count 0, emit 0.
 *   A pixel's colour is its own, so the colours do not pass through this call: pf_fuse_compact_f32 takes the images. */
int pf_geo_filter_f32(const float* depth, const float* view_maps, const int* sources, const float* pair_maps, int V, int M,
                      int h, int w, float pix_threshold, float rel_depth_threshold, int num_consistent, float depth_min,
                      float depth_max, int* count, float* depth_avg, float* point, unsigned char* emit, void* stream);

/* ---- normal maps of depth maps; normals of the fused points (csrc/depth_normals.hip) ------------------------------
 * What fusibile's clouds carry and the fusers above did not.  The specification is this project's own
 * (pointmvsnet_amd/normals.py).  Maps, pixel centres and view_maps as above; only A is read.
 * pf_depth_normals_f32: per pixel p = (x, y) of view i, in float32 in this order, with P(q) = (A_i (xq+.5, yq+.5, 1)) d_i(q)
 *   (the camera centre is not added), valid(q) = q inside the map and depth_min < d(q) < depth_max, linked(q) = valid(q) and
 *   |d(q) - d(p)| <= rel_jump * d(p):
 *   tangent along e = (step, 0): P(p+e) - P(p-e) if both are linked, else P(p+e) - P(p), else P(p) - P(p-e), else none;
 *   likewise along (0, step).  c = cross(tx, ty), n = c / |c|, negated if dot(n, P(p)) > 0 (it faces the camera).
 *   normal (V,h,w,3) = n, or (0, 0, 0) if p is not valid, a tangent is missing, |c| is 0 or not finite, or the dot
 *   product is exactly 0.  step >= 1.
 * pf_fuse_normals_f32: for every pixel p of view i with emit[i][p] set (pf_fuse_mark), out[i][p] = s / |s| with
 *   s = normal_maps[i][p] + the sum of normal_maps[j][match] over the slots of pf_fuse_stage_a_f32's match in ascending
 *   order with match >= 0 (slot = j, or j - 1 behind i), or (0, 0, 0) if |s| is 0 or not finite.  Other rows of out
 *   (V,h,w,3) are not written; pf_fuse_compact_f32 orders the rows like the points. */
int pf_depth_normals_f32(const float* depth, const float* view_maps, int V, int h, int w, int step, float rel_jump,
                         float depth_min, float depth_max, float* normal, void* stream);
int pf_fuse_normals_f32(const float* normal_maps, const int* match, const unsigned char* emit, int V, int h, int w,
                        float* out, void* stream);

/* ---- guided upsampling of depth maps by the views' images (csrc/depth_refine.hip) ----------------------------------
 * A joint bilateral upsampler between the confidence filter and the fusers.  The specification is this project's own
 * (pointmvsnet_amd/refine.py).  depth (V,h,w) float32, 0 = no depth; guide (V,H,W,3) uint8 with
 * H = s h, W = s w, 1 <= s <= 8; pixel centres as above.
 * pf_guide_pack_f32: records (V,h,w) of 8 bytes, per low-resolution pixel q: the bits of d(q), then r | g << 8 | b << 16 of
 *   guide[qy s + s/2][qx s + s/2], the guide pixel that contains q's centre.
 * pf_depth_upsample_f32: ws (s, 2 radius + 1) and wc (766) float32 as refine.spatial_table / refine.colour_table compose
 *   them.  Per output pixel (X, Y) of view i, in float32 in this order, with c = (X / s, Y / s), (px, py) = (X % s, Y % s),
 *   tap (tx, ty) the record q = c + (tx, ty) (a tap outside the map does not exist), valid(q) = depth_min < d(q) < depth_max,
 *   a = the sum of the three absolute channel differences between q's colour and guide[Y][X], and
 *   w(q) = (ws[py][ty + radius] * ws[px][tx + radius]) * wc[a]:
 *   c not valid: out = 0, count = 0.  Else the anchor starts at c; over |tx|, |ty| <= anchor_radius in row-major order a
 *   valid tap with a strictly larger w becomes the anchor; d0 = the anchor's depth.  linked(q) = valid(q) and
 *   |d(q) - d0| <= rel_jump * d0.  Over |tx|, |ty| <= radius in row-major order, linked taps only: Wsum += w,
 *   S += w * (d(q) - d0), count += 1.  out (V,H,W) = d0 + S / Wsum if Wsum > 0, else d0; count (V,H,W) int32, or NULL: not
 *   written.  0 <= radius <= 8, 0 <= anchor_radius <= min(radius, 2), 0 <= rel_jump <= 0.5. */
int pf_guide_pack_f32(const float* depth, const unsigned char* guide, int V, int h, int w, int s, void* records,
                      void* stream);
int pf_depth_upsample_f32(const void* records, const unsigned char* guide, const float* ws, const float* wc, int V, int h,
                          int w, int s, int radius, int anchor_radius, float rel_jump, float depth_min, float depth_max,
                          float* out, int* count, void* stream);

/* ---- segments of depth maps: speckle removal and gap filling (csrc/depth_segments.hip) ------------------------------
 * The specification is this project's own (pointmvsnet_amd/depth_segments.py).  depth (V,h,w) float32 with
 * V h w <= PF_DEPTH_SEGMENTS_MAX; valid(q) = depth_min < d(q) < depth_max (0 <= depth_min < depth_max); two 4-neighbours
 * p, q of one view are linked iff both are valid and |d(p) - d(q)| <= rel_jump * min(d(p), d(q)) in float32,
 * 0 <= rel_jump <= 0.5.  A segment is a connected component of the link graph; its root is its first pixel in row-major
 * order, as a flat index into (V,h,w).  n = V h w below.  No argument can make a kernel fault.
 * pf_depth_tile_size: the tile of pf_depth_tile_segments_f32 (the library's compile-time choice).
 * pf_depth_tile_segments_f32: label (V,h,w) int32 = the flat index of the root of the pixel's piece, the component of the
 *   links INSIDE the pixel's tile (tiles start at multiples of the tile size in every view); -1 for a pixel that is not
 *   valid.  piece (V,h,w) int32, or NULL: at a piece's root the number of its pixels, 0 elsewhere.
 * pf_depth_border_merge_f32: one hook launch over the pixel edges that cross tile borders, on the label array above: the
 *   roots of two linked pixels are united by atomicMin(label[larger root], smaller); *changed (the caller zeroes it) is
 *   raised by the number of edges that found two different roots.
 * pf_depth_label_compress: label[p] = the root of p's tree.  After a merge that left *changed at 0 -- on the labels as
 *   pf_depth_tile_segments_f32 or the last compress left them -- label[p] is the root of p's segment.
 * pf_depth_segment_sizes: size[label[p]] += piece[p] for every p (size (n) int32, zeroed by the caller): at a segment's
 *   root, its number of pixels.
 * pf_depth_speckle_mask_f32: s = size[label[p]] (0 for label -1); sizes (n) int32 = s; out (n) = d(p) if p is valid and
 *   s >= min_size, else 0; removed (n) uint8 = p is valid and s < min_size.  Each of the three may be NULL: not written.
 * pf_depth_gap_fill_f32: a valid pixel keeps its depth.  For a pixel (x, y) that is not valid the horizontal candidate
 *   exists iff the nearest valid pixels xl < x < xr of its row exist, xr - xl - 1 <= max_gap and |dl - dr| <= (rel_jump *
 *   float(xr - xl)) * min(dl, dr); its value is dl + (float(x - xl) / float(xr - xl)) * (dr - dl).  The vertical candidate
 *   likewise along the column.  out = 0.5f * (dh + dv) if both exist, the one that exists, else 0; filled (V,h,w) uint8 (or
 *   NULL) = a candidate exists.  All float32 in this order.  0 <= max_gap <= PF_DEPTH_GAP_MAX; out != depth. */
#define PF_DEPTH_SEGMENTS_MAX 2147483647LL
#define PF_DEPTH_GAP_MAX 32
int pf_depth_tile_size(int* tile_w, int* tile_h);
int pf_depth_tile_segments_f32(const float* depth, int V, int h, int w, float rel_jump, float depth_min, float depth_max,
                               int* label, int* piece, void* stream);
int pf_depth_border_merge_f32(const float* depth, int V, int h, int w, float rel_jump, float depth_min, float depth_max,
                              int* label, int* changed, void* stream);
int pf_depth_label_compress(int* label, int64_t n, void* stream);
int pf_depth_segment_sizes(const int* label, const int* piece, int64_t n, int* size, void* stream);
int pf_depth_speckle_mask_f32(const float* depth, const int* label, const int* size, int64_t n, int min_size,
                              float depth_min, float depth_max, int* sizes, float* out, unsigned char* removed,
                              void* stream);
int pf_depth_gap_fill_f32(const float* depth, int V, int h, int w, int max_gap, float rel_jump, float depth_min,
                          float depth_max, float* out, unsigned char* filled, void* stream);

/* ---- photometric consistency of depth maps: windowed ZNCC (csrc/photo_filter.hip) -----------------------------------
 * The one check of the chain that looks at the images again.  The specification is this project's own
 * (pointmvsnet_amd/photometric.py).  Maps, pixel centres, `sources` and `pair_maps` as for
 * pf_geo_filter_f32 (only entry [i][m][0], the i -> j row, is read).  All float32 operations in the stated order.
 * pf_grey_pack_u8: rgb (n, 3) uint8 -> grey (n) uint8, g = (77 R + 150 G + 29 B + 128) >> 8.
 * pf_grey_quads_u8: grey (V,h,w) uint8 -> quads (V,h,w) uint32, g(y, x) | g(y, x + 1) << 8 | g(y + 1, x) << 16 |
 *   g(y + 1, x + 1) << 24, a neighbour beyond the last column or row repeating the last one: the four bytes of a bilinear tap
 *   in one load.  g_i below is the low byte.
 * pf_photo_ncc_f32: quads (V,h,w) uint32 as above; 1 <= radius = r <= 5, n = (2 r + 1)^2, var_min >= 1.  Per pixel p = (x, y) of view
 *   i with d = d_i(p), c = g_i(p): over the taps (dx, dy) in [-r, r]^2, R = g_i(y + dy, x + dx) - c, SR = sum R,
 *   SRR = sum R^2, VR = n SRR - SR^2 (int32, exact).  p is scorable iff depth_min < d < depth_max, r <= x < w - r,
 *   r <= y < h - r and VR >= var_min.  Per listed source j (dy ascending outside, dx ascending inside):
 *   (qx, qy, z) = (M_ij (x + dx + .5, y + dy + .5, 1)) d + T_ij, rz = 1 / z, (u, v) = (qx rz, qy rz), (fx, fy) = (u - .5,
 *   v - .5), (x0, y0) = floor(fx, fy); the tap is inside iff z > 0, 0 <= x0, x0 + 1 <= w - 1, 0 <= y0, y0 + 1 <= h - 1;
 *   s = (top (1 - wy) + bot wy) - float(c) with top = t00 (1 - wx) + t01 wx, bot = t10 (1 - wx) + t11 wx over g_j as float;
 *   S1 += s, S2 += s s, SX += float(R) s.  VS = n S2 - S1 S1, COV = n SX - float(SR) S1.  j is usable iff p is scorable, every
 *   tap is inside and VS >= float(var_min); its ncc = fminf(1, fmaxf(-1, COV / sqrtf(float(VR) VS))).
 *   ncc (V,M,h,w), or NULL: the usable sources' ncc, a quiet NaN elsewhere (pads and i itself included).  usable (V,h,w)
 *   int32 = usable sources; count (V,h,w) int32 = those with ncc >= ncc_threshold; score (V,h,w) = the sum of the usable ncc
 *   in slot order / float(usable), 0 without one; mask (V,h,w) uint8: bit 0 = p is scorable and count >= num_consistent,
 *   bit 1 = p is scorable. */
int pf_grey_pack_u8(const unsigned char* rgb, int64_t n, unsigned char* grey, void* stream);
int pf_grey_quads_u8(const unsigned char* grey, int V, int h, int w, unsigned* quads, void* stream);
int pf_photo_ncc_f32(const float* depth, const unsigned* quads, const int* sources, const float* pair_maps, int V, int M,
                     int h, int w, int radius, int var_min, float ncc_threshold, int num_consistent, float depth_min,
                     float depth_max, float* ncc, float* score, int* count, int* usable, unsigned char* mask, void* stream);

/* ---- point-cloud evaluation: thinning and nearest distances between unordered clouds (csrc/cloud_eval.hip) -------
 * DTU's accuracy / completeness step, which the reference does not have (a separate MATLAB program).  The specification
 * is this project's own (pointmvsnet_amd/evaluation.py).  A cloud is searched through a sparse grid
 * kept as a sorted array: cell = floor((p - origin) / edge) per axis in float32, clamped to [0, n - 1];
 * key = cx << 42 | cy << 21 | cz.  The caller sorts the keys (ascending; any order inside a cell) and passes the sorted
 * keys together with the points gathered into that order.
 * pf_cloud_cell_keys_f32: keys (n) of points (n, 3).  nx, ny, nz <= PF_CLOUD_MAX_CELLS (so that float32 rounding moves a
 *   cell coordinate by < 0.016 cells, the margin every bound below keeps); n <= PF_CLOUD_MAX_POINTS everywhere.
 * pf_cloud_pack_f32: packed (n) 16-byte records (x, y, z, uint32 tag), 16-byte aligned: record i = point order[i]; tag =
 *   order[i], or with `hashed` prio(order[i]): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16.
 * pf_cloud_thin_round: one round of the greedy minimum-distance thinning in its parallel form on a grid whose edge is
 *   >= 1.05 * min_dist; t = float32(min_dist)^2.  States (n bytes, sorted order): 0 undecided, 1 kept, 2 removed.  An
 *   undecided point i looks at every j with tag(j) < tag(i) and dx*dx + dy*dy + dz*dz < t in state_in: state_out = removed
 *   if one of them is kept, kept if all are removed, else undecided, and then *pending is set to 1 (the caller clears it
 *   before the round and repeats with the buffers swapped while it is set).
 * pf_cloud_nn_cells_f32: per query (nq, 3) the nearest target point among the cubes of radius 1, 3, .. <= rings cells
 *   around the query's cell; done = 1 and dist = min(sqrt(min d^2), max_dist), index = that point's tag (-1 where dist ==
 *   max_dist) once the best distance is <= (radius - 0.05) * edge or that reach covers max_dist; else done = 0 and
 *   dist / index are left alone.
 * pf_cloud_nn_wave_f32: the same result for the queries todo[0 .. ntodo) (indices into query) from the 27 cells around
 *   the query on a grid with edge >= max_dist (the caller adds the rounding margin), one wavefront per query. */
#define PF_CLOUD_MAX_CELLS 131072
#define PF_CLOUD_MAX_POINTS 2000000000
int pf_cloud_cell_keys_f32(const float* points, int64_t n, float ox, float oy, float oz, float edge, int nx, int ny, int nz,
                           int64_t* keys, void* stream);
int pf_cloud_pack_f32(const float* points, const int64_t* order, int64_t n, int hashed, void* packed, void* stream);
int pf_cloud_thin_round(const void* packed, const int64_t* keys, int64_t n, int nx, int ny, int nz, float t,
                        const unsigned char* state_in, unsigned char* state_out, int* pending, void* stream);
int pf_cloud_nn_cells_f32(const float* query, int64_t nq, const void* packed, const int64_t* keys, int64_t nt, float ox,
                          float oy, float oz, float edge, int nx, int ny, int nz, int rings, float max_dist, float* dist,
                          int* index, unsigned char* done, void* stream);
int pf_cloud_nn_wave_f32(const float* query, const int64_t* todo, int64_t ntodo, int64_t nq, const void* packed,
                         const int64_t* keys, int64_t nt, float ox, float oy, float oz, float edge, int nx, int ny, int nz,
                         float max_dist, float* dist, int* index, void* stream);
/* The two DTU filters.  inside[i] = mask[idx] != 0 with idx = floor((p - bb_min) / res + 0.5) per axis (float32) when idx
 * lies in the (X, Y, Z) row-major byte grid, else 0.  above[i] = ((a x + b y) + c z) + d > 0. */
int pf_cloud_obs_mask_f32(const float* points, int64_t n, const unsigned char* mask, int X, int Y, int Z, float bx, float by,
                          float bz, float res, unsigned char* inside, void* stream);
int pf_cloud_above_plane_f32(const float* points, int64_t n, float a, float b, float c, float d, unsigned char* above,
                             void* stream);

/* ---- cleaning a fused cloud: k-nearest statistics and a voxel-grid merge (csrc/cloud_filter.hip) -------------------
 * The specification is this project's own (pointmvsnet_amd/cloud_filter.py).  The searches take the
 * sorted grid of pf_cloud_cell_keys_f32 / pf_cloud_pack_f32 above over the cloud itself, with plain index tags (hashed = 0)
 * and any edge.  d2(i, j) = (dx*dx + dy*dy) + dz*dz in float32; the neighbours of i are the points j != i by index (tag).
 * Both searches visit the cubes of radius r = 1, 2, .. cells around a point's cell until a ring is final: when it decides
 * the result -- see below -- or when (r - 0.05) * edge >= radius, the cube then holding everything within radius.
 * pf_cloud_knn_stats_f32: per point i, with a_1 <= a_2 <= ... the c = min(k, number of neighbours with d2 < radius2)
 *   smallest such d2: mean[i] = (((sqrtf(a_1) + sqrtf(a_2)) + ...) + float(k - c) * radius) / float(k), or radius itself
 *   when c = 0; count[i] = c (count may be NULL).  Final also when the k-th best is <= ((r - 0.05) * edge)^2.
 *   1 <= k <= PF_CLOUD_MAX_K; radius2 is the caller's float32 product radius * radius.
 * pf_cloud_radius_count_f32: count[i] = min(limit, number of neighbours with d2 < radius2); final also when limit are
 *   found.  1 <= limit <= PF_CLOUD_MAX_K.
 * pf_cloud_voxel_keys_f32: keys (n) = cx << 42 | cy << 21 | cz with c = floor((p - o) * inv) per axis in float32, clamped to
 *   [0, n_axis - 1]; inv is the caller's float32 reciprocal of the voxel edge, n_axis <= PF_CLOUD_MAX_CELLS.
 * pf_cloud_voxel_reduce_f32: the caller sorts the keys STABLY; order (n) is that permutation and starts (m + 1) the first
 *   sorted slot of each of the m voxels, starts[m] = n.  Row s of the outputs, from the points order[starts[s] ..
 *   starts[s+1]) in that (ascending index) order: out_points = float32(float64 sum / count); out_colors (uint8, with colors)
 *   = (2 * sum + count) / (2 * count) per channel in integers; out_normals (with normals) = the float64 sum divided by its
 *   float64 length, rounded to float32, (0, 0, 0) when the length is 0; out_counts (int32, may be NULL); inverse (n, may be
 *   NULL)[order[t]] = s.  colors / out_colors and normals / out_normals are given or NULL together. */
#define PF_CLOUD_MAX_K 32
int pf_cloud_knn_stats_f32(const void* packed, const int64_t* keys, int64_t n, int nx, int ny, int nz, float edge, int k,
                           float radius, float radius2, float* mean, int* count, void* stream);
int pf_cloud_radius_count_f32(const void* packed, const int64_t* keys, int64_t n, int nx, int ny, int nz, float edge,
                              int limit, float radius, float radius2, int* count, void* stream);
int pf_cloud_voxel_keys_f32(const float* points, int64_t n, float ox, float oy, float oz, float inv, int nx, int ny, int nz,
                            int64_t* keys, void* stream);
int pf_cloud_voxel_reduce_f32(const float* points, const unsigned char* colors, const float* normals, const int64_t* order,
                              const int64_t* starts, int64_t n, int64_t m, float* out_points, unsigned char* out_colors,
                              float* out_normals, int* out_counts, int64_t* inverse, void* stream);

/* ---- rendering a point cloud into depth maps: a z-buffer point splat (csrc/cloud_render.hip) -----------------------
 * The inverse of the fusers' back-projection, which the reference does not have (it scores depth maps against ground-truth
 * depth maps; DTU's test scans ship a ground-truth cloud).  The specification is this project's own
 * (pointmvsnet_amd/render.py).  Pixel centres at (x + 0.5, y + 0.5) as above.
 *   proj (V, PF_RENDER_PROJ_FLOATS): K [R | t] (3x4 row-major), composed in float64 by the host and passed as float32
 *   zbuf (V, h, w) 64-bit cells, set to all-ones by the caller on the same stream before the launch
 * pf_cloud_splat_f32: per point n = (X, Y, Z) of points (N, 3) and view v, in float32 in this order:
 *   qx = ((p0 X + p1 Y) + p2 Z) + p3, qy and z likewise from rows 1 and 2; skip unless depth_min < z < depth_max (false
 *   for NaN); u = qx / z, v = qy / z; skip unless -splat <= u < w + splat and -splat <= v < h + splat (compared as floats);
 *   (xc, yc) = floor(u, v); every pixel (x, y) of the map with |x - xc| <= splat and |y - yc| <= splat takes
 *   zbuf[v][y][x] = min(zbuf[v][y][x], float_bits(z) << 32 | n) by a 64-bit unsigned atomic minimum: the nearest point
 *   wins, among equal z the lowest index, whatever the order of arrival.  Non-finite coordinates are skipped by the tests.
 *   0 <= splat <= PF_RENDER_MAX_SPLAT, N <= PF_RENDER_MAX_POINTS, maps within the limits of pf_fuse_stage_a_f32.
 * pf_cloud_zbuf_decode: depth (V,h,w) = the float in a cell's upper half, 0 where the cell is all-ones; index (V,h,w) int32 =
 *   its lower half, -1 where empty (an index past 2^31 - 1 appears as its bit pattern); index may be NULL: not written. */
#define PF_RENDER_PROJ_FLOATS 12
#define PF_RENDER_MAX_SPLAT 8
#define PF_RENDER_MAX_POINTS 4294967294LL
int pf_cloud_splat_f32(const float* points, int64_t N, const float* proj, int V, int h, int w, int splat, float depth_min,
                       float depth_max, uint64_t* zbuf, void* stream);
int pf_cloud_zbuf_decode(const uint64_t* zbuf, int V, int h, int w, float* depth, int* index, void* stream);

/* ---- rasterising a triangle mesh into depth maps (csrc/mesh_render.hip) ----------------------------------------------
 * The z-buffer above with a face for a point.  The specification is this project's own (pointmvsnet_amd/render.py, "Mesh
 * rasterisation"); parity with OpenGL, Open3D or nvdiffrast is neither claimed nor tested.  proj and zbuf as above; h, w <=
 * PF_MESH_MAX_SIDE; faces (Nf, 3) int32 rows of vertices (Nv, 3), Nf <= PF_MESH_MAX_FACES, Nv <= 2^31 - 1.
 * Screen coordinates, per vertex and view in float32 in this order: qx, qy, z as in pf_cloud_splat_f32; u = qx / z,
 *   v = qy / z; valid iff depth_min < z < depth_max and -G <= u < w + G and -G <= v < h + G, G = PF_MESH_GUARD_BAND, compared
 *   as floats (false for NaN); xi = (int)rintf(u * 256.0f), yi = (int)rintf(v * 256.0f) (round half to even).  All that
 *   follows is exact in int64.
 * pf_mesh_screen_f32: that table: xy (V, Nv, 2) int32 (0, 0 where not valid), z (V, Nv) as computed, valid (V, Nv) 0 / 1.
 *   For tests and inspection; the rasteriser re-projects with the same device function.
 * pf_mesh_raster_f32: a face is rasterised in a view iff its three indices lie in [0, Nv) (another index is never read
 *   through), its three vertices are valid there and area2 = (bx-ax)(cy-ay) - (by-ay)(cx-ax) != 0; no clipping.  Front-facing
 *   iff area2 < 0; cull = PF_MESH_CULL_NONE renders both sides, PF_MESH_CULL_BACK only front-facing faces, PF_MESH_CULL_FRONT
 *   only the others.  For area2 < 0 b and c are swapped first.  Edge p -> q, d = q - p: E(s) = dx (sy - py) - dy (sx - px);
 *   pixel (x, y) with centre s = (256 x + 128, 256 y + 128) is covered iff for each of a -> b, b -> c, c -> a: E(s) > 0, or
 *   E(s) == 0 and (dy > 0 or (dy == 0 and dx < 0)).  With Ea, Eb, Ec the edge functions opposite a, b, c:
 *   ra = 1.0f / za (rb, rc likewise), inv = ((float)Ea * ra + (float)Eb * rb) + (float)Ec * rc, z = (float)area2 / inv;
 *   zbuf[v][y][x] = min(zbuf[v][y][x], float_bits(z) << 32 | face) by a 64-bit unsigned atomic minimum.  A face whose
 *   bounding box clamped to the map holds more than PF_MESH_LANE_PIXELS pixel centres is walked by its wave instead of its
 *   lane; the result does not depend on that.  Decode with pf_cloud_zbuf_decode.
 * pf_mesh_raster_tuned_f32: the same with that threshold as the argument lane_pixels >= 0 (tools/microbench_mesh_render.py).
 * pf_mesh_bary_f32: index (V, h, w) int32 from the decode; bary (V, h, w, 3) = ((float)Ea ra / inv, (float)Eb rb / inv,
 *   (float)Ec rc / inv) of the pixel's face in the face's STORED vertex order, zeros where index is -1. */
#define PF_MESH_GUARD_BAND 16384
#define PF_MESH_MAX_SIDE 16384
#define PF_MESH_MAX_FACES 4294967294LL
#define PF_MESH_LANE_PIXELS 64
#define PF_MESH_CULL_NONE 0
#define PF_MESH_CULL_BACK 1
#define PF_MESH_CULL_FRONT 2
int pf_mesh_screen_f32(const float* vertices, int64_t Nv, const float* proj, int V, int h, int w, float depth_min,
                       float depth_max, int* xy, float* z, unsigned char* valid, void* stream);
int pf_mesh_raster_f32(const float* vertices, int64_t Nv, const int* faces, int64_t Nf, const float* proj, int V, int h,
                       int w, float depth_min, float depth_max, int cull, uint64_t* zbuf, void* stream);
int pf_mesh_raster_tuned_f32(const float* vertices, int64_t Nv, const int* faces, int64_t Nf, const float* proj, int V, int h,
                             int w, float depth_min, float depth_max, int cull, int lane_pixels, uint64_t* zbuf,
                             void* stream);
int pf_mesh_bary_f32(const float* vertices, int64_t Nv, const int* faces, int64_t Nf, const float* proj, int V, int h, int w,
                     float depth_min, float depth_max, const int* index, float* bary, void* stream);

/* ---- meshing: TSDF integration of depth maps and marching tetrahedra (csrc/tsdf.hip) ----------------------------------
 * Volumetric fusion and iso-surface extraction, which the reference does not have.  The specification is this project's
 * own (pointmvsnet_amd/tsdf.py).  A volume has nx x ny x nz samples, indexed [k][j][i] (x fastest); sample (i, j, k) sits at
 * o + (float)i * voxel per coordinate; nx * ny * nz <= PF_TSDF_MAX_SAMPLES.  proj as for pf_cloud_splat_f32.
 * pf_tsdf_integrate_f32: per sample and view v in ascending order, in float32: qx, qy, z as in pf_cloud_splat_f32; skip
 *   unless depth_min < z < depth_max; u = qx / z, v = qy / z; skip unless 0 <= u < w and 0 <= v < h (compared as floats);
 *   d = depths[v][floor(v)][floor(u)]; skip unless depth_min < d < depth_max; sdf = d - z; skip if sdf < -trunc;
 *   S += fminf(sdf, trunc) / trunc, W += 1; with images (V, h, w, 3) uint8 and |sdf| <= trunc: CS (nz, ny, nx, 3) += rgb,
 *   CW += 1.  S, W (and CS, CW) are read and written: a call continues the sums of the calls before it.  images NULL: CS and
 *   CW are not touched.  One thread owns a sample: no atomics, one order of summation.
 * pf_tsdf_count_triangles: count ((nz-1)(ny-1)(nx-1)) int32, per cell (k (ny-1) + j)(nx-1) + i the number of triangles, 0..12:
 *   0 unless all 8 corners have weight >= min_weight; a corner is inside iff tsdf < 0; the cell is cut into the tetrahedra
 *   (0,1,3,7) (0,3,2,7) (0,2,6,7) (0,6,4,7) (0,4,5,7) (0,5,1,7) of its corners c = dx + 2 dy + 4 dz; a tetrahedron with 1 or 3
 *   inside corners gives one triangle, with 2 two.
 * pf_tsdf_emit_triangles: inclusive = the inclusive prefix sum of count, faces its last value; keys (faces, 3) int64: per
 *   triangle the keys of its three edges, (sample index of the lower end) * 8 + direction bits, in the order and winding of
 *   pointmvsnet_amd/tsdf.py (normals from inside to outside).
 * pf_tsdf_vertices_f32: per key the vertex p_a + t (p_b - p_a), t = f_a / (f_a - f_b), per coordinate in float32; with colour
 *   (nz, ny, nx, 3) uint8 also floor(c_a + t (c_b - c_a) + 0.5) clamped to 0..255 into colours (count, 3); both NULL or neither.
 *   A key that names no edge of the volume (direction bits 0, an end outside the grid, no such sample) gives (0, 0, 0). */
#define PF_TSDF_MAX_SAMPLES 2147483647LL
int pf_tsdf_integrate_f32(const float* depths, const unsigned char* images, const float* proj, int V, int h, int w, float ox,
                          float oy, float oz, float voxel, int nx, int ny, int nz, float trunc, float depth_min,
                          float depth_max, float* S, int* W, int* CS, int* CW, void* stream);
int pf_tsdf_count_triangles(const float* tsdf, const int* weight, int nx, int ny, int nz, int min_weight, int* count,
                            void* stream);
int pf_tsdf_emit_triangles(const float* tsdf, const int* weight, int nx, int ny, int nz, int min_weight,
                           const int64_t* inclusive, int64_t faces, int64_t* keys, void* stream);
int pf_tsdf_vertices_f32(const int64_t* keys, int64_t count, const float* tsdf, const unsigned char* colour, float ox, float oy,
                         float oz, float voxel, int nx, int ny, int nz, float* vertices, unsigned char* colours, void* stream);

/* ---- sparse TSDF volumes: brick allocation, integration, marching tetrahedra (csrc/sparse_tsdf.hip) ---------------------
 * The volume of the pf_tsdf_* block stored only near the surface (specification: pointmvsnet_amd/sparse_tsdf.py).  The
 * virtual grid has nx x ny x nz samples, at most PF_SPARSE_TSDF_MAX_AXIS per axis; a brick holds 8 x 8 x 8 of them, brick
 * (bi, bj, bk) = (i >> 3, j >> 3, k >> 3) has the key (bk NBy + bj) NBx + bi with NB* = ceil(n* / 8), and NBx NBy NBz < 2^31.
 * keys (bricks,) int64 are the allocated bricks, sorted and unique, bricks * 512 <= INT32_MAX; row b of S, W (bricks, 512), CS
 * (bricks, 512, 3) and CW belongs to keys[b], local index (lk * 8 + lj) * 8 + li.  proj, depths, images as for
 * pf_tsdf_integrate_f32.
 * pf_sparse_tsdf_touch: touched (NBx NBy NBz) uint8, one byte per virtual brick, set to 1 (never cleared, so calls
 *   accumulate) where some view passes the brick test: the brick's box grown by one sample per side is projected by its 8
 *   corners (qx, qy, z as in pf_tsdf_integrate_f32); m = 2^-20 (max |p8 X| + |p9 Y| + |p10 Z| + |p11| + trunc); the view is
 *   skipped if zhi + m <= depth_min or zlo - m >= depth_max; the pixel box is the whole image unless zlo - m > depth_min and
 *   2^-20 (max(|qx| terms, |qy| terms) + max(w, h) max |z| terms) < zlo / 4, else the corners' floor(u), floor(v) bounding
 *   box padded by one pixel and clipped; the brick is touched if a pixel of the box has depth_min < d < depth_max and
 *   (zlo - trunc) - m <= d <= (zhi + trunc) + m.  A NaN among the projections: the whole image and every valid d.
 * pf_sparse_tsdf_neighbours: rows (bricks, 7) int32: the rows of the +x, +y, +xy, +z, +xz, +yz, +xyz bricks of each brick
 *   (column c - 1 for c = dx + 2 dy + 4 dz), -1 where that brick is outside the grid or not among keys.
 * pf_sparse_tsdf_integrate_f32: pf_tsdf_integrate_f32 on the samples of the allocated bricks that lie inside the grid; the
 *   others are not touched.
 * pf_sparse_tsdf_count_triangles: count (bricks, 512) int32 per cell, owned by the brick of its corner 0, as
 *   pf_tsdf_count_triangles; a corner in a brick that is not allocated counts as weight 0; min_weight >= 1.  tsdf and weight
 *   are (bricks, 512).
 * pf_sparse_tsdf_emit_triangles: as pf_tsdf_emit_triangles in the order of count; the keys are those of the virtual grid,
 *   ((k ny + j) nx + i) * 8 + direction bits.
 * pf_sparse_tsdf_vertices_f32: as pf_tsdf_vertices_f32 for keys of the virtual grid, tsdf (bricks, 512) and colour
 *   (bricks, 512, 3) uint8; a key with an end in a brick that is not allocated gives (0, 0, 0) as well. */
#define PF_SPARSE_TSDF_MAX_AXIS 1048576
int pf_sparse_tsdf_touch(const float* depths, const float* proj, int V, int h, int w, float ox, float oy, float oz, float voxel,
                         int nx, int ny, int nz, float trunc, float depth_min, float depth_max, unsigned char* touched,
                         void* stream);
int pf_sparse_tsdf_neighbours(const int64_t* keys, int64_t bricks, int nx, int ny, int nz, int* rows, void* stream);
int pf_sparse_tsdf_integrate_f32(const int64_t* keys, int64_t bricks, const float* depths, const unsigned char* images,
                                 const float* proj, int V, int h, int w, float ox, float oy, float oz, float voxel, int nx, int ny,
                                 int nz, float trunc, float depth_min, float depth_max, float* S, int* W, int* CS, int* CW,
                                 void* stream);
int pf_sparse_tsdf_count_triangles(const float* tsdf, const int* weight, const int* rows, int64_t bricks, int min_weight,
                                   int* count, void* stream);
int pf_sparse_tsdf_emit_triangles(const int64_t* keys, int64_t bricks, const float* tsdf, const int* weight, const int* rows,
                                  int nx, int ny, int nz, int min_weight, const int64_t* inclusive, int64_t faces,
                                  int64_t* tri_keys, void* stream);
int pf_sparse_tsdf_vertices_f32(const int64_t* edge_keys, int64_t count, const int64_t* keys, int64_t bricks, const float* tsdf,
                                const unsigned char* colour, float ox, float oy, float oz, float voxel, int nx, int ny, int nz,
                                float* vertices, unsigned char* colours, void* stream);

/* ---- mesh clean-up and scoring: components, vertex normals, surface samples (csrc/mesh_ops.hip) -----------------------
 * The specification is this project's own (pointmvsnet_amd/mesh_ops.py).  vertices (Nv, 3) float32, faces (Nf, 3) int32,
 * Nv, Nf <= PF_MESH_OPS_MAX.  Every kernel skips a face with an index outside [0, Nv); no argument can make one fault.
 * pf_mesh_cc_hook: one hook launch of the hook-and-compress connected components on label (Nv) int32, which the caller
 *   initialises to label[v] = v: per face, the roots of (a, b) and of (a, c) are united by atomicMin(label[larger root],
 *   smaller); *changed is set to 1 iff some edge found two different roots (the caller zeroes it).
 * pf_mesh_cc_compress: label[v] = the root of v's tree, for every v.  After a round (hook, compress) whose hook left
 *   *changed at 0, label[v] is the smallest vertex index of v's connected component.
 * pf_mesh_face_labels: face_label[f] = label[faces[f][0]], -1 for a skipped face.
 * pf_mesh_vertex_normals_f32: offsets (Nv + 1) and corners (3 Nf) int64: vertex v owns the corners corners[offsets[v] ..
 *   offsets[v + 1]), corner 3 f + j is faces[f][j], in ascending order.  Per corner's face (a, b, c): e1 = p_b - p_a,
 *   e2 = p_c - p_a, n = e1 x e2 in float32 (each component a product, a product, a difference); skipped unless finite;
 *   else added to a float64 sum in that order.  normals (Nv, 3) = (float)(s / len), len = sqrt((sx sx + sy sy) + sz sz) in
 *   float64, (0, 0, 0) unless len is finite and positive.
 * pf_mesh_sample_count_f32: count (Nf) int32 = floorf(x + u_f) clamped to 2^31 - 1, x = (0.5f * sqrtf((nx nx + ny ny) + nz nz))
 *   * inv in float32 with n as above, u_f = (H(H(f ^ seed)) >> 8) * 2^-24, H = the hash of csrc/pf_hash.h; 0 unless x is finite.
 * pf_mesh_sample_emit_f32: inclusive (Nf) int64 = the inclusive prefix sum of count, N its last value (<= PF_MESH_OPS_MAX).
 *   Sample s belongs to the first face f with inclusive[f] > s, as its j-th (j = s - inclusive[f - 1]); i1 = H(H(f ^ seed) +
 *   2 j + 1) >> 8, i2 likewise with 2 j + 2 (mod 2^32); if i1 + i2 > 2^24 both become 2^24 - i; r = i * 2^-24; bary (N, 3) =
 *   ((2^24 - i1 - i2) * 2^-24, r1, r2); points (N, 3) = p_a + (r1 e1 + r2 e2) per coordinate in float32; face_index (N) = f.
 *   A sample whose face cannot be found or is skipped gets zeros and face_index -1. */
#define PF_MESH_OPS_MAX 2147483647LL
int pf_mesh_cc_hook(const int* faces, int64_t Nf, int64_t Nv, int* label, int* changed, void* stream);
int pf_mesh_cc_compress(int* label, int64_t Nv, void* stream);
int pf_mesh_face_labels(const int* faces, int64_t Nf, int64_t Nv, const int* label, int* face_label, void* stream);
int pf_mesh_vertex_normals_f32(const float* vertices, int64_t Nv, const int* faces, int64_t Nf, const int64_t* offsets,
                               const int64_t* corners, float* normals, void* stream);
int pf_mesh_sample_count_f32(const float* vertices, int64_t Nv, const int* faces, int64_t Nf, float inv, unsigned seed,
                             int* count, void* stream);
int pf_mesh_sample_emit_f32(const float* vertices, int64_t Nv, const int* faces, int64_t Nf, const int64_t* inclusive,
                            int64_t N, unsigned seed, float* points, int* face_index, float* bary, void* stream);

/* ---- mesh simplification: vertex clustering with quadric placement (csrc/mesh_simplify.hip) ---------------------------
 * The specification is this project's own (pointmvsnet_amd/mesh_simplify.py).  vertices (Nv, 3) float32, faces (Nf, 3) int32,
 * Nv, Nf <= PF_MESH_OPS_MAX; cluster (Nv) int64 is pf_cloud_voxel_reduce_f32's inverse map onto M <= Nv clusters.  No
 * argument can make a kernel fault: every index is checked where it is read.
 * pf_mesh_simplify_faces: triple (Nf, 3) int32 = (cluster[a], cluster[b], cluster[c]) in the face's own order, ascending
 *   (Nf, 3) int32 the same three numbers sorted, collapsed (Nf) = 1 iff two of them are equal; a face with an index outside
 *   [0, Nv) or a cluster outside [0, M) gets (-1, -1, -1) and collapsed = 1.
 * pf_mesh_simplify_keep_first: sorted_faces (K) int64 are face indices ordered by their ascending triple (by a stable sort,
 *   so ascending inside a run of equal triples); keep[sorted_faces[t]] = 1 iff t = 0 or the triple differs from that of
 *   sorted_faces[t - 1], else 0.  Other entries of keep (Nf) are not written.
 * pf_mesh_quadric_thread_f64 / _wave_f64: offsets (M + 1) and corners (3 Nf) int64: cluster s owns the list
 *   corners[offsets[s] .. offsets[s + 1]), corner 3 f + j being a corner of face f.  means (M, 3) float32.  In float64, per
 *   list entry with its face (a, b, c): p' = p - mean per coordinate, e1 = p_b' - p_a', e2 = p_c' - p_a', n = e1 x e2 (each
 *   component a product, a product, a difference), skipped unless finite; d = -((nx ax' + ny ay') + nz az'); the sums
 *   A += n n^T (six entries) and b += d n.  t = (A00 + A11) + A22; unless t is finite and positive the position is the mean;
 *   else lam = (regularisation * t) / 3, M = A + lam I is factored M = L D L^T (l10 = a01 / m00, l20 = a02 / m00,
 *   d1 = m11 - l10 a01, u21 = a12 - l20 a01, l21 = u21 / d1, d2 = m22 - (l20 a02 + l21 u21)) and M x = -b solved (y0 = -b0,
 *   y1 = -b1 - l10 y0, y2 = -b2 - (l20 y0 + l21 y1), x2 = y2 / d2, x1 = y1 / d1 - l21 x2, x0 = y0 / m00 - (l10 x1 + l20 x2));
 *   if some |x_k| <= (double)cell does not hold, fallback[s] = 1 and x = 0.  positions (M, 3) = (float)(mean + x), fallback
 *   (M) 0 / 1.  _thread: one thread per cluster, its list in ascending order; clusters whose list has `threshold` or more
 *   entries are not written.  _wave: one wave per cluster todo[0 .. ntodo): lane l adds entries l, l + 64, .., the lanes'
 *   sums are combined by the butterfly xor 32, 16, .. 1.  PF_MESH_SIMPLIFY_MIN_REG <= regularisation <= 1. */
#define PF_MESH_SIMPLIFY_MIN_REG 1e-6
int pf_mesh_simplify_faces(const int* faces, int64_t Nf, int64_t Nv, const int64_t* cluster, int64_t M, int* triple,
                           int* ascending, unsigned char* collapsed, void* stream);
int pf_mesh_simplify_keep_first(const int* ascending, int64_t Nf, const int64_t* sorted_faces, int64_t K,
                                unsigned char* keep, void* stream);
int pf_mesh_quadric_thread_f64(const float* vertices, int64_t Nv, const int* faces, int64_t Nf, const int64_t* offsets,
                               const int64_t* corners, const float* means, int64_t M, float cell, double regularisation,
                               int64_t threshold, float* positions, unsigned char* fallback, void* stream);
int pf_mesh_quadric_wave_f64(const float* vertices, int64_t Nv, const int* faces, int64_t Nf, const int64_t* offsets,
                             const int64_t* corners, const float* means, int64_t M, float cell, double regularisation,
                             const int64_t* todo, int64_t ntodo, float* positions, unsigned char* fallback, void* stream);

/* ---- exact point-to-mesh distances (csrc/mesh_distance.hip) -----------------------------------------------------------
 * The specification is this project's own (pointmvsnet_amd/mesh_distance.py): per query the lexicographic minimum of
 * (d2, face index) over the faces, d2 the squared distance to the triangle in float64 from the float32 coordinates.  The
 * search structure is the sorted sparse grid of the cloud kernels above with a (cell, face) pair for a point; ox .. nz are
 * its origin, cell edge and cell counts (nx, ny, nz <= PF_CLOUD_MAX_CELLS).  vertices (Nv, 3) float32, faces (Nf, 3) int32,
 * Nf <= PF_MESH_DIST_MAX_FACES.  A face with an index outside [0, Nv) or a non-finite vertex is skipped everywhere.
 * pf_mesh_dist_count_f32: count (Nf) int64 = min(limit, the number of cells the face is listed in): the box from
 *   cell(min - m) to cell(max + m) per axis over its vertices, cell(x) = floor((x - o) / edge) clamped to the grid, m =
 *   PF_MESH_DIST_BOX_MARGIN * edge, all in float32; 0 for a skipped face.  1 <= limit <= 2^32.
 * pf_mesh_dist_emit_f32: inclusive (Nf) int64 = the inclusive prefix sum of the UNCLAMPED counts, total its last value
 *   (<= PF_MESH_DIST_MAX_PAIRS).  Pair s belongs to the first face f with inclusive[f] > s, as its j-th; its cell is the
 *   j-th of the face's box, z fastest, then y.  keys (total) = cx << 42 | cy << 21 | cz, pair_face (total) = f.
 * pf_mesh_dist_pack_f32: the caller sorts the keys; order (total) is that permutation.  records (total) 48-byte rows, 16-byte
 *   aligned: (a.x, a.y, a.z, int32 face, b.x, b.y, b.z, 0, c.x, c.y, c.z, 0) of the face of pair order[i].
 * pf_mesh_dist_cells_f64: one thread per query walks the cubes of radius 1, 3, .. rings (<= 15) cells around its cell;
 *   done[i] = 1 and dist / face are final when the best distance is <= (r - 0.05) * edge or (r - 0.05) * edge >= max_dist;
 *   done[i] = 0 otherwise and dist / face are not written.  d = (float)sqrt(d2); dist = max_dist and face = -1 unless
 *   d < max_dist.
 * pf_mesh_dist_wave_f64: one wave per query todo[0 .. ntodo) on a grid with edge >= max_dist: the 27 cells around it. */
#define PF_MESH_DIST_MAX_FACES 134209536LL
#define PF_MESH_DIST_MAX_PAIRS 2147483647LL
#define PF_MESH_DIST_BOX_MARGIN 0.02f
int pf_mesh_dist_count_f32(const float* vertices, int64_t Nv, const int* faces, int64_t Nf, float ox, float oy, float oz,
                           float edge, int nx, int ny, int nz, int64_t limit, int64_t* count, void* stream);
int pf_mesh_dist_emit_f32(const float* vertices, int64_t Nv, const int* faces, int64_t Nf, float ox, float oy, float oz,
                          float edge, int nx, int ny, int nz, const int64_t* inclusive, int64_t total, int64_t* keys,
                          int* pair_face, void* stream);
int pf_mesh_dist_pack_f32(const float* vertices, int64_t Nv, const int* faces, int64_t Nf, const int* pair_face,
                          const int64_t* order, int64_t total, void* records, void* stream);
int pf_mesh_dist_cells_f64(const float* query, int64_t nq, const void* records, const int64_t* keys, int64_t total, float ox,
                           float oy, float oz, float edge, int nx, int ny, int nz, int rings, float max_dist, float* dist,
                           int* face, unsigned char* done, void* stream);
int pf_mesh_dist_wave_f64(const float* query, const int64_t* todo, int64_t ntodo, int64_t nq, const void* records,
                          const int64_t* keys, int64_t total, float ox, float oy, float oz, float edge, int nx, int ny, int nz,
                          float max_dist, float* dist, int* face, void* stream);

/* ---- image preprocessing from decoded uint8 views (csrc/preprocess.hip) -----------------------------------------
 * What reference dataset.py:269-287 does on the host before it uploads float32: cv2.resize, crop_dtu_input and
 * norm_image (utils/preprocess.py:6-11,56-85).  Specification: pointmvsnet_amd/utils/preprocess.py (the resize is this
 * project's own statement of bilinear interpolation with half-pixel centres, not OpenCV's fixed-point kernel).
 * pf_preprocess_resize_u8: src (V, h_src, w_src, 3) interleaved bytes, 16-byte aligned.  Output pixel (y, x) of the
 *   (H, W) cropped image blends the source pixels (yi[y] | yi[y]+1, xi[x] | xi[x]+1) (the +1 clamped to the last
 *   row / column) with the weights yw[y], xw[x] of the second one:
 *   (1-wy)*((1-wx)*p00 + wx*p01) + wy*((1-wx)*p10 + wx*p11) in float32, rounded half-to-even to a byte -> ref
 *   (V, H, W, 3).  The tables (the host composes them in float64, crop offset included) must be non-decreasing;
 *   span >= the largest number of source columns xi[last] + 2 - xi[first] that one tile of PF_PREPROCESS_TILE_X
 *   output columns samples.  sums (V, 3, 2) 64-bit integers receives, per view and channel, sum p and sum p*p over
 *   ref (zeroed by the call; integer atomics: exact, the same bits whatever the order).
 * pf_preprocess_standardise_f32: out (V, 3, H, W) planar = float32((p - mean) / (sqrt(var) + 1e-7)) evaluated in
 *   float64 with mean = S1 / N, var = (N S2 - S1^2) / N^2 (population variance) from the integers of `sums`. */
#define PF_PREPROCESS_TILE_X 256
int pf_preprocess_resize_u8(const unsigned char* src, int V, int h_src, int w_src, const int* xi, const float* xw,
                            const int* yi, const float* yw, int H, int W, int span, unsigned char* ref,
                            unsigned long long* sums, void* stream);
int pf_preprocess_standardise_f32(const unsigned char* ref, const unsigned long long* sums, int V, int H, int W,
                                  float* out, void* stream);

/* ---- the confidence filter of a whole scan, into the fusion (csrc/scan_filter.hip) -------------------------------
 * What reference tools/depthfusion.py:153-170 does per view on files, for all V views in one launch and in the four
 * interpolation modes of its -m/--inter_mode.  Specification: pointmvsnet_amd/scan.py (the resampling is this project's own
 * statement of what cv2.resize does to float32; bit parity with OpenCV is neither claimed nor tested).
 * pf_scan_filter_f32: filtered (V, h, w) = depth (V, h, w) where flow confidence >= flow_threshold and resized initial
 *   confidence >= init_threshold, else 0; the comparisons are NumPy's depth[conf < thr] = 0, so a NaN confidence keeps
 *   the depth.  kept (V) int32 receives the number of pixels per view that the filter did not zero (zeroed by the call,
 *   integer atomics).  The flow confidence is EITHER flow_prob (V, 5, h, w), turned into a confidence by the rule of
 *   pf_eval_flow_prob_f32, OR flow_conf (V, fh, fw); the other pointer is NULL.  init_conf is (V, ih, iw).  A confidence
 *   map of the depth map's size is read as it is; any other size is resampled to (h, w) with the tap tables of its axes:
 *   output row y reads the T source rows clamp(ys[y] + k, 0, s - 1), k = 0 .. T-1, with the weights yw[y * T + k]
 *   (columns alike, xs / xw); T = 1 (PF_SCAN_NEAREST: the value itself, no product), 2 (BILINEAR), 4 (CUBIC),
 *   8 (LANCZOS4).  The host composes the tables in float64 and passes the weights as float32; the kernel evaluates
 *   horizontally first, then vertically, in float32, each sum in ascending tap order.  The tables of a map that needs
 *   no resampling may be NULL.  flow_resized / init_resized: (V, h, w) or NULL, receive the confidences the comparisons
 *   saw.
 * pf_scan_filter_supported: 1 iff mode is one of the four, every size is >= 1, every map has at most 2^24 pixels,
 *   h <= 65535 * PF_SCAN_FILTER_TILE_Y and the LDS tile of each resampled map fits 48 KiB:
 *   4 * sy * (sx + PF_SCAN_FILTER_TILE_X) bytes with sy = (TILE_Y - 1) * s_h / h + T + 2 and
 *   sx = (TILE_X - 1) * s_w / w + T + 2 (integer division) -- upsampling by any factor, shrinking by up to ~9 x with
 *   LANCZOS4.  Anything else: PF_ERR_UNSUPPORTED.  V <= 65535. */
#define PF_SCAN_NEAREST 0
#define PF_SCAN_BILINEAR 1
#define PF_SCAN_CUBIC 2
#define PF_SCAN_LANCZOS4 4
#define PF_SCAN_FILTER_TILE_X 32
#define PF_SCAN_FILTER_TILE_Y 8
int pf_scan_filter_supported(int mode, int h, int w, int fh, int fw, int ih, int iw);
int pf_scan_filter_f32(const float* depth, const float* flow_prob, const float* flow_conf, int fh, int fw,
                       const float* init_conf, int ih, int iw, int V, int h, int w, int mode, const int* flow_ys,
                       const float* flow_yw, const int* flow_xs, const float* flow_xw, const int* init_ys,
                       const float* init_yw, const int* init_xs, const float* init_xw, float flow_threshold,
                       float init_threshold, float* filtered, int* kept, float* flow_resized, float* init_resized,
                       void* stream);

/* ==== Row Z : the training step (BASELINE config 4; reference train.py:72-82) ======================================
 * Hand-written backward for the convolution -> BatchNorm(batch statistics) -> ReLU blocks of ImageConv, VolumeConv
 * and the flow MLP (reference nn/conv.py:24-35,62-77,108-121,197-210; networks.py:84-167; model.py:40-43), replacing
 * ATen's convolution_backward / batch_norm backward (MIOpen / CK solvers) in the reference's loss.backward().
 * Everything below sums in a fixed order: gradients are bit-reproducible run to run.
 *
 * Forward finalize that keeps what the backward needs: like pf_bn_finalize_jobs_f32, but the result is ONE tensor
 * rows (4, S, ld_rows) = [scale | shift | mean | invstd], S = G / groups_per_stat; rows[0], rows[1] are the (S, ld)
 * in_scale / in_shift rows the forward kernels take.  The C channels of this call are channels [ch0, ch0 + C) of
 * gamma / beta / the running statistics and land in columns [col_out, col_out + C) of every row (EdgeConv's
 * BatchNorm covers [central | difference] halves with separate statistics, reference networks.py:33-36).  Running
 * statistics updated as by pf_bn_finalize_jobs_f32. */
int pf_bn_train_rows_f32(const double* partials, int T, int pcols, int col0, int C, double count, double unbias_n,
                         const float* gamma, const float* beta, float* running_mean, float* running_var,
                         float momentum, float eps, int G, int groups_per_stat, float* rows, int ld_rows, int col_out,
                         int ch0, void* stream);
/* BatchNorm(+ReLU) backward on planar tensors (N, C, S): g = dL/dz for z = act(y * scale + shift), y the raw
 * convolution output, rows as above (statistic group s = n / samples_per_stat).
 *   reduce : partials (N, pf_norm_blocks(S), C, 2) float64 = per-block (sum g', sum g' * xhat),
 *            g' = [y * scale + shift > 0] * g when relu != 0, else g;  xhat = (y - mean) * invstd
 *   coeffs : partials (G, T, pcols, 2) -> coef (2, S, C) = [scale * dbeta_s / count | scale * invstd * dgamma_s / count]
 *            and dgamma[c] / dbeta[c] = sum over the S statistic groups (accumulate != 0: added to what is there)
 *   apply  : dy = scale * g' - coef0 - coef1 * (y - mean)           (dy may alias g; the two entry points below) */
int pf_bn_bwd_reduce_f32(const float* g, const float* y, const float* rows, int64_t N, int64_t C, int64_t S,
                         int samples_per_stat, int relu, double* partials, void* stream);
int pf_bn_bwd_coeffs_f32(const double* partials, int T, int pcols, int col0, int C, double count, int G,
                         int groups_per_stat, const float* rows, float* coef, float* dgamma, float* dbeta,
                         int accumulate, void* stream);
/* coeffs + apply in one launch (the planar path of the training step): every block re-adds its statistic group's
 * partial rows (pf_norm_blocks(S) * samples_per_stat of them, the same order and bits as pf_bn_bwd_coeffs_f32), block
 * (0, c, 0) writes dgamma[c] / dbeta[c] (NULL: not wanted).  count = samples_per_stat * S. */
int pf_bn_bwd_apply_fused_f32(const float* g, const float* y, const float* rows, const double* partials, int T,
                              double count, float* dy, int64_t N, int64_t C, int64_t S, int samples_per_stat, int relu,
                              float* dgamma, float* dbeta, int accumulate, void* stream);
/* The whole BatchNorm(+ReLU) backward of planar tensors in ONE launch where a plane fits one block's registers (round 6):
 * samples_per_stat == 1 (every sample its own statistic group: the towers' per-view statistics, VolumeConv's one sample),
 * S % 4 == 0, S <= 32 768 (pf_bn_bwd_plane_supported), 16-byte aligned tensors.  rows (4, N, C) as pf_bn_train_rows_f32
 * writes them; dy (N, C, S); dgamma / dbeta (C) = the sums over the N samples in sample order (added when accumulate;
 * NULL: not wanted).  One block per channel loads a plane's (g, y) once, reduces, and writes dy from the registers:
 * 12 bytes per element and one launch where pf_bn_bwd_reduce_f32 + pf_bn_bwd_apply_fused_f32 are 20 and two. */
int pf_bn_bwd_plane_supported(int64_t S, int samples_per_stat);
int pf_bn_bwd_plane_f32(const float* g, const float* y, const float* rows, int64_t N, int64_t C, int64_t S, int relu,
                        float* dy, float* dgamma, float* dbeta, int accumulate, void* stream);
/* The same on point-major rows (G groups of Ng rows, ld floats per row; C in {16, 32, 64, 128} for reduce,
 * C % 4 == 0 for apply / affine): the flow MLP's BatchNorm1d.  reduce partials: (G, pf_rows_bn_blocks(G, Ng), C, 2).
 * pf_rows_affine_f32: z = act(y * scale + shift), the normalised activation handed on. */
int pf_rows_bn_blocks(int G, int Ng);
int pf_rows_bn_bwd_reduce_f32(const float* g, int64_t ldg, const float* y, int64_t ldy, const float* rows, int C, int G,
                              int Ng, int groups_per_stat, int relu, double* partials, void* stream);
int pf_rows_bn_bwd_apply_f32(const float* g, int64_t ldg, const float* y, int64_t ldy, const float* rows,
                             const float* coef, float* dy, int64_t ldo, int C, int G, int Ng, int groups_per_stat,
                             int relu, void* stream);
int pf_rows_affine_f32(const float* y, int64_t ldy, const float* rows, float* z, int64_t ldz, int C, int G, int Ng,
                       int groups_per_stat, int relu, void* stream);

/* Weight gradient of a convolution on the f32 matrix cores (csrc/conv_wgrad.hip), one formulation for nn.Conv2d /
 * nn.Conv3d / nn.ConvTranspose3d / the 1x1 convolutions over points:
 *     dw[cg][cx][kd][kh][kw] = sum_{n, o} gr[n, cg, o] * x[n, cx, o * stride + k - pad]           (zero outside x)
 * gr (N, Cg, Do, Ho, Wo) lives on the COARSE grid, x (N, Cx, Di, Hi, Wi) on the FINE one (2-D: Do = Di = KD = 1):
 *   convolution            gr = dL/dy, x = the layer input        -> dw in (Cout, Cin, k...) order;
 *   transposed convolution gr = the layer input, x = dL/dy (stride 2, pad 1) -> dw in (Cin, Cout, k...) order.
 * x_scale / x_shift (N / x_samples_per_stat, Cx) or NULL: x holds a RAW convolution output whose BatchNorm + ReLU is
 * pending; relu(x * scale + shift) is applied while x is staged (zero padding after it).
 * workspace: pf_conv_wgrad_workspace(...) bytes of device scratch (per-split partial gradients, added in split
 * order: no atomics).  accumulate != 0: dw += instead of dw =.  Limits: kernel extents <= 7, taps/16-channel block
 * <= 28 column tiles (27 taps x 16 channels, 25 x 16, ...); PF_ERR_UNSUPPORTED otherwise. */
int64_t pf_conv_wgrad_workspace(int64_t N, int64_t Cg, int64_t Cx, int64_t Do, int64_t Ho, int64_t Wo, int64_t Di,
                                int64_t Hi, int64_t Wi, int KD, int KH, int KW, int stride);
int pf_conv_wgrad_f32(const float* gr, const float* x, float* dw, int64_t N, int64_t Cg, int64_t Cx, int64_t Do,
                      int64_t Ho, int64_t Wo, int64_t Di, int64_t Hi, int64_t Wi, int KD, int KH, int KW, int stride,
                      int pd, int ph, int pw, const float* x_scale, const float* x_shift, int x_samples_per_stat,
                      void* workspace, int64_t workspace_bytes, int accumulate, void* stream);
/* The launch plan the two weight-gradient entry points use for a shape, for tests that pin it (the plan is a pure
 * function of the shape and of the device's occupancy for the chosen instantiation): plan12 = {row tiles per block MT,
 * tile TD, tile TH, channel sub-blocks per block, channels per sub-block, accumulator tiles per wave, position splits,
 * channel blocks, row blocks, LDS bytes, position tiles per block, stride}. */
int pf_conv_wgrad_plan(int64_t N, int64_t Cg, int64_t Cx, int64_t Do, int64_t Ho, int64_t Wo, int64_t Di, int64_t Hi,
                       int64_t Wi, int KD, int KH, int KW, int stride, int* plan12);
int pf_rows_wgrad_plan(int64_t P, int Cg, int Cx, int* plan12);
/* The same for a 1x1 convolution over point-major rows: dw[cg][cx] = sum_p gr[p, cg] * act(x[p, cx]);
 * gr (P, ldg), x (P, ldx), Cg % 4 == Cx % 4 == 0; x_scale / x_shift rows (P / x_rows_per_stat, Cx) or NULL. */
int64_t pf_rows_wgrad_workspace(int64_t P, int Cg, int Cx);
int pf_rows_wgrad_f32(const float* gr, int64_t ldg, const float* x, int64_t ldx, float* dw, int64_t P, int Cg, int Cx,
                      const float* x_scale, const float* x_shift, int64_t x_rows_per_stat, void* workspace,
                      int64_t workspace_bytes, int accumulate, void* stream);
/* Several layers' pf_conv_wgrad_f32 (partials only, as with dw == NULL) in as few launches as their kernel instantiations
 * allow (round 6): a training node queues the weight gradients of its layers -- nothing in the step waits for them -- and
 * issues them together once its data-gradient chain is done; layers that share an instantiation (VolumeConv's 96-384-block
 * layers below 24x32x40 beside conv1_0; the 25 600-point PointFlow iteration's 1x1 layers beside the 102 400-point one's)
 * ride in ONE grid.  Each item's arguments mean what pf_conv_wgrad_f32's mean; the
 * partials land in item.workspace (>= pf_conv_wgrad_workspace bytes) in the layout described below and are summed by
 * pf_wgrad_reduce_batch_f32.  n <= 64. */
typedef struct pf_wgrad_item {
  const float* gr;
  const float* x;
  int64_t N, Cg, Cx, Do, Ho, Wo, Di, Hi, Wi;
  int KD, KH, KW, stride, pd, ph, pw;
  int x_samples_per_stat;
  const float* x_scale;
  const float* x_shift;
  void* workspace;
  int64_t workspace_bytes;
  /* rows_P > 0: the item is a pf_rows_wgrad_f32 call instead -- gr (rows_P, ldg), x (rows_P, ldx) point-major rows, Cg / Cx
   * columns of them, x_rows_per_stat rows behind one (x_scale, x_shift) row; the grid / kernel / pad fields are unused
   * (stride must be 1). */
  int64_t rows_P, ldg, ldx, x_rows_per_stat;
} pf_wgrad_item;
int pf_conv_wgrad_batch_f32(const pf_wgrad_item* items, int n, void* stream);
/* dw == NULL in the two calls above: the split partials only.  The workspace then holds (splits, Cg, taps, Cx), splits =
 * workspace bytes / (4 * Cg * Cx * taps) -- the channel index fastest: what the kernel's lanes store as 64-byte runs
 * (round 6; it was (splits, Cg, Cx, taps)).  pf_wgrad_reduce_batch_f32 adds the partials of n layers in ONE launch, each
 * in the same fixed order as the single call (bit-identical results), and puts the sums into nn.ConvNd's order:
 * rows[i] = the Cg and taps[i] the KD * KH * KW (1 for pf_rows_wgrad_f32) of the call that wrote parts[i];
 *   swapped[i] == 0:  dws[i][(a * B + b) * T + t]         (+)= sum_k parts[i][k][(a * T + t) * B + b],  B = elems / (rows * T);
 *   swapped[i] != 0:  dws[i][(b * A + a) * T + T - 1 - t] (+)= the same sum,  A = rows[i].
 * SWAPPED: for a stride-1 'same' convolution the two operands of pf_conv_wgrad_f32 may change places -- gr' = x,
 * x' = dL/dy -- which gives dW'[cx][cg][k'] = dW[cg][cx][K-1-k'] per axis: the rows of the MFMA tile are then the layer's
 * INPUT channels and the patch staged with its halo is the (narrow) gradient tensor.  VolumeConv's conv0_1 (64 -> 8: 8 of
 * 16 MFMA rows used, a 64-channel halo patch per tile) and conv6_2 (8 -> 1: 1 of 16 rows) take it (reference
 * networks.py:134,147 under train.py:80; round 6: 185 -> 115 us and 38 -> 27 us at config 4). */
int pf_wgrad_reduce_batch_f32(const float* const* parts, float* const* dws, const int64_t* elems, const int* splits,
                              const int* rows, const int* taps, const int* swapped, int n, int accumulate, void* stream);


/* Data gradient of ImageConv's 5x5 / stride 2 / pad 2 convolutions (reference networks.py:93,98,103), i.e.
 * ConvTranspose2d(5, stride 2, pad 2, output_padding 1): dy (N, Cout, Ho, Wo) -> dx (N, Cin, 2 Ho, 2 Wo);
 * wp = the convolution's weight W (Cout, Cin, 5, 5) packed (Cout/4, 25 taps [kh][kw], 4, 16*ceil(Cin/16)):
 * wp[g][tap][k][ci] = W[4g + k][ci][kh][kw], zero padded.  Cout % 4 == 0, Cin <= 32.  (csrc/conv_dgrad.hip) */
int pf_deconv2d_k5s2_supported(int64_t Cout, int64_t Cin);
int pf_deconv2d_k5s2_f32(const float* dy, const float* wp, float* dx, int64_t N, int64_t Cout, int64_t Cin, int64_t Ho,
                         int64_t Wo, void* stream);
/* 3x3x3 / pad 1 / stride 1 conv3d of a ONE-channel volume x (N, 1, D, H, W) with w (Cout <= 8, 27): the data
 * gradient of VolumeConv's 8 -> 1 output layer (reference networks.py:147) when w holds the flipped kernels. */
int pf_conv3d_k3_c1_f32(const float* x, const float* w, float* y, int64_t N, int64_t Cout, int64_t D, int64_t H,
                        int64_t W, void* stream);


/* ---- Row Z : backward of the fused warp + variance stages without atomics (csrc/warp_bwd.hip) -------------------
 * Replaces, in the reference's loss.backward(), grid_sample's backward (a float-atomic scatter-add,
 * utils/feature_fetcher.py:55) and the element-wise chain of the variance (model.py:103-111, :187-190) for the coarse
 * cost volume and for the flow feature assembly.  One scene; maps channel-last (V, H, W, C) as the forward kernels
 * read them; points n = d * H * W + y * W + x.  Gradients never flow into the sampling positions
 * (utils/feature_fetcher.py:29).
 *
 * pf_sort_pairs_by_key: counting sort of `pairs` pair ids by keys[p] < nkeys (larger keys are dropped): start
 * (nkeys + 1), order = the ids grouped by key, ascending inside a group.  Kernel launches only (capturable). */
int64_t pf_sort_pairs_workspace(int64_t pairs, int64_t nkeys);
int pf_sort_pairs_by_key(const uint32_t* keys, int64_t pairs, int64_t nkeys, uint32_t* order, uint32_t* start,
                         void* workspace, int64_t workspace_bytes, void* stream);
/* taps: for every (view v, point n), pair id p = v * N + n: keys[p] = v * (H+1) * (W+1) + (yi+1) * (W+1) + (xi+1) for
 * the north-west tap (yi, xi) of its bilinear footprint (0xffffffff when no tap is inside the map) and
 * fxy[p] = (fx, fy), the fractional offsets.  flow: the points of pf_flow_features_f32 (depth (H, W) at the flow
 * resolution, ratio 1); frustum: the points of pf_frustum_variance_f32 (skip_view0 != 0: view 0 gets no keys, it
 * contributes its un-warped map, model.py:103-106). */
int pf_warp_taps_flow_f32(const float* depth, const float* interval, const float* cam, int V, int H, int W,
                          uint32_t* keys, float* fxy, void* stream);
int pf_warp_taps_frustum_f32(const float* kinv, const float* rinv, const float* t, const float* depths, const float* K,
                             const float* E, int V, int H, int W, int D, int skip_view0, uint32_t* keys, float* fxy,
                             void* stream);
/* gval (V, N, ctot) = (2 / V) * dvar[n, c] * (f_v[n, c] - mean_v f), ctot = c1 + c2 + c3 (levels concatenated, c_l % 4
 * == 0, c2 / c3 may be 0); dvar rows (N, ldv) point-major, or (ctot, N) channel-major with ldv = -1 (a cost volume's
 * gradient as it is). */
int pf_variance_grad_f32(const float* maps1, int c1, const float* maps2, int c2, const float* maps3, int c3, int V, int H,
                         int W, int64_t N, const uint32_t* keys, const float* fxy, const float* dvar, int64_t ldv,
                         int ref_override, float* gval, void* stream);
/* dmaps[v] (H, W, ctot) for v in [v0, V): every texel adds weight * gval over the sorted lists of the four cells whose
 * pairs have it as a tap -- plain stores, fixed order. */
int pf_warp_gather_f32(const float* gval, const float* fxy, const uint32_t* order, const uint32_t* start, int V, int v0,
                       int H, int W, int ctot, float* dmaps, void* stream);
/* ddepth (H, W): gradient w.r.t. the prior depth through the xyz features (24 columns from c0 of the point's
 * feature row; reference model.py:178-194). */
int pf_flow_depth_grad_f32(const float* dfeat, int64_t ld, int c0, const float* cam, int H, int W, float* ddepth,
                           void* stream);
/* Adjoint of the bilinear resize (align_corners = False) of pf_flow_pyramid_f32 for one level: dres (V, OH, OW, ld)
 * channel-last, columns [c0, c0 + C) -> dlevel (V, C, IH, IW). */
int pf_resize_bilinear_backward_f32(const float* dres, int ld, int c0, int C, int V, int OH, int OW, int IH, int IW,
                                    float* dlevel, void* stream);


/* Weight packing for a whole training step in ONE launch (csrc/norm_bwd.hip): `table` is a device array of `npacks`
 * descriptors (pf_pack_desc_bytes() bytes each; layout in pointmvsnet_amd/train_packs.py), each an affine gather
 *     dst[d_0 .. d_{n-1}] = src[sum_k a_k * sstride_k],  a_k = off_k + sum_i M[k][i] * d_i,  0 unless 0 <= a_k < lim_k
 * -- the MFMA operand layouts, zero paddings, flips and transpositions the forward and backward kernels of the step
 * read their weights in.  max_total: the largest destination element count in the table. */
int pf_pack_desc_bytes(void);
int pf_pack_gather_f32(const void* table, int npacks, long long max_total, void* stream);

/* ---- Row Z: the small differentiable heads of the training step (csrc/train_heads.hip) --------------------------
 * One or two launches each where autograd makes 15-25 element-wise ATen launches; float64 fixed-order reductions.
 *
 * pf_softargmin_backward_f32: backward of row S's depth (reference model.py:117-124): gcost[b,k,i] =
 *   -gdepth[b,i] * p_k * (z_k - depth[b,i]) with p = softmax(-cost) recomputed as pf_softargmin_prob_f32 rounds it and
 *   z_k - depth evaluated as step * (k - sum_j p_j j) (no difference of two numbers of the size of the depth; the
 *   `depth` argument must be valid and is not read).
 * pf_flow_head_train_f32: act (5*hw, ld >= 16) rows (row = d*hw + pixel) -> logit = act . w16 (channel order),
 *   prob (5, hw) = softmax(-logit) over d, offset (hw) = sum_d prob_d * (d - 2) * interval[0] (model.py:40-43,218-227).
 * pf_flow_head_backward_f32: gact (5*hw, 16) = d offset / d act * goffset, gw16 (16) (+)= its weight gradient;
 *   workspace: pf_flow_head_backward_workspace(hw) bytes.
 * pf_masked_mae_f32: loss[0] = weight * sum_b [ sum_{gt != 0} |pred - gt| / interval[b] / (count_b + 1e-7) ] with gt
 *   (B, H, W) read at the nearest-resized positions of pred (B, h, w) (networks.py:170-181, model.py:308-339);
 *   coef (B) = weight / (interval_b * (count_b + 1e-7)) for the backward: gpred = gloss[0] * coef_b * sign(pred - gt)
 *   on valid pixels, 0 elsewhere. */
int pf_softargmin_backward_f32(const float* cost, const float* params, const float* depth, const float* gdepth,
                               float* gcost, int64_t B, int64_t D, int64_t HW, void* stream);
int pf_flow_head_train_f32(const float* act, int64_t ld, const float* w16, const float* interval, int64_t hw,
                           float* offset, float* prob, void* stream);
int64_t pf_flow_head_backward_workspace(int64_t hw);
int pf_flow_head_backward_f32(const float* act, int64_t ld, const float* w16, const float* interval, const float* prob,
                              const float* goffset, int64_t hw, float* gact, float* gw16, int accumulate,
                              void* workspace, int64_t workspace_bytes, void* stream);
int pf_masked_mae_f32(const float* pred, const float* gt, const float* interval, int B, int h, int w, int H, int W,
                      float weight, float* loss, float* coef, void* stream);
int pf_masked_mae_backward_f32(const float* pred, const float* gt, const float* coef, const float* gloss, int B, int h,
                               int w, int H, int W, float* gpred, void* stream);
/* torch.optim.RMSprop's update (reference solver.py:17-52; no momentum, not centered) on flat float32 buffers of n
 * elements: g' = g + wd[i] * p (wd NULL: no weight decay); sq = alpha * sq + (1 - alpha) * g'^2;
 * p -= lr * g' / (sqrt(sq) + eps).  alpha is taken as the float nearest to the caller's double: pass (float)alpha. */
int pf_rmsprop_f32(float* p, const float* g, float* sq, const float* wd, int64_t n, float lr, float alpha, float eps,
                   void* stream);

#ifdef __cplusplus
}
#endif
#endif /* POINTFLOW_HIP_H_ */
