// Shared host/device helpers for libpointflow_hip.so (gfx950 only; no CUDA paths).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pointflow_hip.h"

#define PF_WAVE 64

// Per-device sticky status word (bad neighbour index etc.); allocated on first use.
unsigned* pf_status_ptr();

#define PF_REQUIRE(cond)                 \
  do {                                   \
    if (!(cond)) return PF_ERR_INVALID_ARG; \
  } while (0)

#define PF_HIP(expr)                        \
  do {                                      \
    hipError_t _e = (expr);                 \
    if (_e != hipSuccess) return (int)_e;   \
  } while (0)

static inline int pf_launch_status() {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? PF_OK : (int)e;
}

static inline int64_t pf_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is per DEVICE: `flags` is one bit per device ordinal, owned by the
// caller (one static word per kernel instantiation), so a process that drives several GPUs opts in on each of them.
#include <atomic>
static inline int pf_allow_big_lds(const void* kernel, int bytes, std::atomic<unsigned long long>& flags) {
  int dev = 0;
  PF_HIP(hipGetDevice(&dev));
  const unsigned long long bit = 1ull << (dev & 63);
  if (flags.load(std::memory_order_acquire) & bit) return PF_OK;
  PF_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
  flags.fetch_or(bit, std::memory_order_release);
  return PF_OK;
}

// Zero `bytes` bytes (a multiple of 4, 4-byte aligned) with a KERNEL.  The scatter-add backward passes need their output
// cleared first; hipMemsetAsync did that until the training step was captured in a hipGraph: memset nodes recorded
// from the autograd thread were not replayed reliably (the cleared buffers kept the previous replay's sums and the
// gradients grew from replay to replay, tools/dbg_train.py), a kernel node is.
#if defined(__HIPCC__)
static __global__ __launch_bounds__(256) void pf_zero_kernel(unsigned* __restrict__ p, size_t words) {
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < words; i += stride) p[i] = 0u;
}
static inline int pf_zero_async(void* p, size_t bytes, hipStream_t s) {
  if (bytes == 0) return PF_OK;
  const size_t words = bytes / 4;
  size_t blocks = (words + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(pf_zero_kernel, dim3((unsigned)blocks), dim3(256), 0, s, reinterpret_cast<unsigned*>(p), words);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? PF_OK : (int)e;
}
#endif

// ---- XCD-aware block order ------------------------------------------------------------------------
// Workgroups are dealt to the 8 XCDs round-robin in dispatch order (linear block id % 8) and every XCD has its own 4 MB
// L2.  With tile = block, the eight neighbours of a tile -- which read the same halo rows -- sit on eight different L2s.
// pf_xcd_xy relabels the blocks of a 2-D grid so that XCD x owns the x-th contiguous eighth of the launch's tiles:
// neighbours share an L2.  A pure relabelling (a bijection of the grid): results are bit-identical as long as everything
// a kernel derives from blockIdx -- the BatchNorm partial row included -- comes from the relabelled ids.  The tower
// convolutions (conv2d_wide.hip) take it: +1.0 % on the headline; the other kernel families measured showed nothing or
// lost (profiles/r06t_xcd_block_order.md).  (The EdgeConv gather passes use their own band order, edgeconv.hip: xcd_tile.)
#ifdef __HIPCC__
// the relabelled (blockIdx.x, blockIdx.y) of a 2-D grid (x fastest in dispatch order)
__device__ __forceinline__ void pf_xcd_xy(unsigned& bx, unsigned& by) {
  const unsigned gx = gridDim.x, total = gx * gridDim.y;
  const unsigned lin = blockIdx.y * gx + blockIdx.x;
  const unsigned per = total >> 3, rem = total & 7u;
  const unsigned x = lin & 7u, j = lin >> 3;
  const unsigned L = x * per + (x < rem ? x : rem) + j;
  by = L / gx;
  bx = L - by * gx;
}
#endif

// ---- projection + bilinear taps shared by the fetch kernels -------------------------------------
// Follows reference utils/feature_fetcher.py:36-55 on the arithmetic of ATen's CPU grid_sample with
// align_corners=True (the oracle): un-normalise with (g + 1) * ((size - 1) / 2), weights
// nw = (1-wy)(1-wx) ..., out = ((nw*a + ne*b) + sw*c) + se*d.  Compiled with -ffp-contract=off so the
// products/sums below stay separate unless written as fmaf.
struct PfTaps {
  int off[4];     // y*W + x of the nw, ne, sw, se taps; 0 (a valid address) when the tap is outside the map
  float wgt[4];   // bilinear weights; exactly 0 for a tap outside the map (zero padding)
  bool ok[4];     // tap inside the map (only the backward scatter needs it)
  int xi, yi;     // column / row of the nw tap (tap k sits at (xi + (k & 1), yi + (k >> 1)) when ok[k])
  float fx, fy;   // fractional parts: wgt = {(1-fy)(1-fx), (1-fy) fx, fy (1-fx), fy fx} where ok
};

__device__ __forceinline__ void pf_project_taps(float X, float Y, float Z, const float* __restrict__ Kv,
                                                const float* __restrict__ Ev, int H, int W, PfTaps& t) {
  float px = X, py = Y, pz = Z;
  if (Ev != nullptr) {
    px = fmaf(Ev[2], Z, fmaf(Ev[1], Y, Ev[0] * X)) + Ev[3];
    py = fmaf(Ev[6], Z, fmaf(Ev[5], Y, Ev[4] * X)) + Ev[7];
    pz = fmaf(Ev[10], Z, fmaf(Ev[9], Y, Ev[8] * X)) + Ev[11];
  }
  const float nx = px / pz;
  const float ny = py / pz;
  const float u = fmaf(Kv[2], 1.0f, fmaf(Kv[1], ny, Kv[0] * nx));
  const float v = fmaf(Kv[5], 1.0f, fmaf(Kv[4], ny, Kv[3] * nx));
  const float gx = ((u - 0.5f) / (float)(W - 1)) * 2.0f - 1.0f;
  const float gy = ((v - 0.5f) / (float)(H - 1)) * 2.0f - 1.0f;
  const float ix = (gx + 1.0f) * ((float)(W - 1) / 2.0f);
  const float iy = (gy + 1.0f) * ((float)(H - 1) / 2.0f);
  const float x0 = floorf(ix), y0 = floorf(iy);
  const float wx1 = ix - x0, wy1 = iy - y0;
  const float wx0 = 1.0f - wx1, wy0 = 1.0f - wy1;
  const float xmax = (float)(W - 1), ymax = (float)(H - 1);
  const bool vx0 = (x0 >= 0.0f) && (x0 <= xmax);
  const bool vx1 = (x0 + 1.0f >= 0.0f) && (x0 + 1.0f <= xmax);
  const bool vy0 = (y0 >= 0.0f) && (y0 <= ymax);
  const bool vy1 = (y0 + 1.0f >= 0.0f) && (y0 + 1.0f <= ymax);
  const int xi = (vx0 || vx1) ? (int)x0 : 0;
  const int yi = (vy0 || vy1) ? (int)y0 : 0;
  t.xi = xi;
  t.yi = yi;
  t.fx = wx1;
  t.fy = wy1;
  t.ok[0] = vy0 && vx0;
  t.ok[1] = vy0 && vx1;
  t.ok[2] = vy1 && vx0;
  t.ok[3] = vy1 && vx1;
  t.off[0] = t.ok[0] ? yi * W + xi : 0;
  t.off[1] = t.ok[1] ? yi * W + xi + 1 : 0;
  t.off[2] = t.ok[2] ? (yi + 1) * W + xi : 0;
  t.off[3] = t.ok[3] ? (yi + 1) * W + xi + 1 : 0;
  // zero weight == the reference's masked gather (value 0) times the weight: the term is +-0 either way.
  // (Feature maps are finite activations; 0 * inf is not a case the reference can produce a number for.)
  t.wgt[0] = t.ok[0] ? wy0 * wx0 : 0.0f;
  t.wgt[1] = t.ok[1] ? wy0 * wx1 : 0.0f;
  t.wgt[2] = t.ok[2] ? wy1 * wx0 : 0.0f;
  t.wgt[3] = t.ok[3] ? wy1 * wx1 : 0.0f;
}

// Unconditional loads (outside taps read element 0 with weight 0): the compiler can issue the taps of
// several views / channels back to back instead of one exec-masked branch per tap.
__device__ __forceinline__ float pf_sample(const float* __restrict__ plane, const PfTaps& t) {
  const float a = plane[t.off[0]];
  const float b = plane[t.off[1]];
  const float c = plane[t.off[2]];
  const float d = plane[t.off[3]];
  return ((a * t.wgt[0] + b * t.wgt[1]) + c * t.wgt[2]) + d * t.wgt[3];
}

// ---- flow confidence of reference utils/eval_file_logger.py:48-62, shared by eval_out.hip and scan_filter.hip ----
// prob (5, hw) hypothesis probabilities of one map -> p[floor(i)] + p[min(floor(i) + 1, 4)] at pixel i
__device__ __forceinline__ float pf_flow_confidence(const float* __restrict__ prob, int i, int hw) {
  float p[5];
#pragma unroll
  for (int d = 0; d < 5; ++d) p[d] = prob[(int64_t)d * hw + i];
  // np.sum(out_flow_prob_map * interval_list, axis=-1): float64 products, add.reduce = a0 + (((a1+a2)+a3)+a4)
  const double a0 = (double)p[0] * -2.0, a1 = (double)p[1] * -1.0, a2 = (double)p[2] * 0.0;
  const double a3 = (double)p[3] * 1.0, a4 = (double)p[4] * 2.0;
  const double idx = (a0 + (((a1 + a2) + a3) + a4)) + 2.0;
  int fl = (int)floor(idx);
  int ce = fl + 1;
  ce = ce < 0 ? 0 : (ce > 4 ? 4 : ce);                    // np.clip(pred_ceil, 0, 4)
  fl = fl < 0 ? fl + 5 : fl;                              // NumPy fancy indexing wraps a negative index
  fl = fl < 0 ? 0 : (fl > 4 ? 4 : fl);                    // (out of range would raise in NumPy; clamp, never fault)
  return p[fl] + p[ce];
}
