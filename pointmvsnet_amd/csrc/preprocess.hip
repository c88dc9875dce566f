// Image preprocessing from decoded uint8 views: bilinear resize -> centre crop -> per-view, per-channel standardisation
// (what reference dataset.py:269-287 does on the host with cv2.resize, crop_dtu_input and norm_image before it uploads
// float32).  The specification is pointmvsnet_amd/utils/preprocess.py; the resize part of it is this project's own.
//
//   resize_crop    one block = 256 output pixels of kRows consecutive output rows of one view.  Per output row the two
//                  source rows' segment that the tile samples is staged into LDS with aligned 16-byte loads (the source is
//                  3-byte interleaved: a lane's pixel starts at any byte), the blend reads bytes from LDS, the result goes
//                  through a 768-byte LDS line and leaves as aligned words.  The block sums p and p*p of its pixels per
//                  channel (exact in 32 bits for 256 x kRows bytes) and adds them to the view's six 64-bit INTEGER totals:
//                  integer addition is associative, so the totals are the same bits whatever the arrival order.
//   standardise    one block = 4096 pixels of one view.  A channel has only 256 possible inputs, so every block first
//                  evaluates the float64 expression (p - mean) / (sqrt(var) + 1e-7) for p = 0..255 into a 3 x 256 float
//                  table in LDS (3 divisions per thread) and then only looks up: 12 bytes in, three float4 out per lane,
//                  each plane written as full 1 KiB wave stores.
//
// Bytes (the algo_bytes of utils/preprocess.py): source 3 B/px read once, the uint8 image 3 B/px written and read back,
// 12 B/px of float32 written.  The second pass reads the intermediate image, not the source: 3 B/px instead of a second
// blend over up to four source pixels.
#include "pf_common.h"

// hipcc spells LDS `__shared__`.  The host re-compilation of tests/hipemu rewrites that spelling in the sources of its fixed
// list only; it reaches this file through eval_out.hip, so the emulator's spelling is chosen here.
#if defined(__HIP__)
#define PF_PRE_LDS __shared__
#define PF_PRE_LDS_DYNAMIC(name) extern __shared__ __attribute__((aligned(16))) unsigned char name[]
#else
#define PF_PRE_LDS static thread_local
#define PF_PRE_LDS_DYNAMIC(name) unsigned char* name = reinterpret_cast<unsigned char*>(::hipemu_shared_memory())
#endif

namespace {

constexpr int kTileX = PF_PREPROCESS_TILE_X;
constexpr int kRows = 8;
constexpr int kGroups = 4;                            // 4-pixel groups per thread of the standardise kernel

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// 16 bytes at byte offset `at` (a multiple of 16) of a buffer of `total` bytes; bytes behind the end read as 0
__device__ __forceinline__ uint4 load16(const unsigned char* __restrict__ base, int64_t at, int64_t total) {
  if (at + 16 <= total) return *reinterpret_cast<const uint4*>(base + at);
  unsigned w[4] = {0u, 0u, 0u, 0u};
  for (int b = 0; b < 16; ++b)
    if (at + b < total) w[b >> 2] |= (unsigned)base[at + b] << ((b & 3) * 8);
  return make_uint4(w[0], w[1], w[2], w[3]);
}

__global__ __launch_bounds__(kTileX) void resize_crop_kernel(
    const unsigned char* __restrict__ src, int h_src, int w_src, const int* __restrict__ xi, const float* __restrict__ xw,
    const int* __restrict__ yi, const float* __restrict__ yw, int H, int W, int span, int row_lds,
    unsigned char* __restrict__ ref, unsigned long long* __restrict__ sums) {
  PF_PRE_LDS_DYNAMIC(lds);                             // two source row segments of row_lds bytes, then the output line
  PF_PRE_LDS unsigned red[kTileX / PF_WAVE][6];
  uint4* lds4 = reinterpret_cast<uint4*>(lds);
  unsigned char* line = lds + 2 * row_lds;
  const int tid = threadIdx.x;
  const int v = blockIdx.z;
  const int x_first = blockIdx.x * kTileX;
  const int x_last = min(x_first + kTileX - 1, W - 1);
  const int x = x_first + tid;
  const bool active = x < W;
  const int64_t total = (int64_t)gridDim.z * h_src * w_src * 3;
  // the tile's source columns [xlo, xlo + npx): the tables are non-decreasing; everything is clamped so that a table that
  // is not can only give wrong pixels, never an address outside the buffers
  const int xlo = clampi(xi[x_first], 0, w_src - 1);
  const int xhi = min(clampi(xi[x_last], 0, w_src - 1) + 1, w_src - 1);
  const int npx = clampi(xhi - xlo + 1, 1, span);
  int o0 = 0, o1 = 0;
  float wx = 0.0f;
  if (active) {
    const int x0 = clampi(xi[x], 0, w_src - 1);
    o0 = clampi(x0 - xlo, 0, npx - 1) * 3;
    o1 = clampi(min(x0 + 1, w_src - 1) - xlo, 0, npx - 1) * 3;
    wx = xw[x];
  }
  const bool words = (W & 3) == 0;                     // then every tile's line starts and ends on a 4-byte boundary
  const int line_bytes = (x_last - x_first + 1) * 3;
  unsigned s1[3] = {0u, 0u, 0u}, s2[3] = {0u, 0u, 0u};
  const int y_first = blockIdx.y * kRows;
  for (int r = 0; r < kRows && y_first + r < H; ++r) {
    const int y = y_first + r;
    const int y0 = clampi(yi[y], 0, h_src - 1);
    const int y1 = min(y0 + 1, h_src - 1);
    const float wy = yw[y];
    int lead[2];                                       // bytes between the 16-byte boundary and the segment's first pixel
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int64_t g0 = (((int64_t)v * h_src + (k == 0 ? y0 : y1)) * w_src + xlo) * 3;
      const int64_t a0 = g0 & ~(int64_t)15;
      lead[k] = (int)(g0 - a0);
      const int chunks = (lead[k] + npx * 3 + 15) >> 4;            // <= row_lds / 16 because npx <= span
      for (int i = tid; i < chunks; i += kTileX) lds4[k * (row_lds >> 4) + i] = load16(src, a0 + 16 * (int64_t)i, total);
    }
    __syncthreads();
    if (active) {
      const unsigned char* __restrict__ r0 = lds + lead[0];
      const unsigned char* __restrict__ r1 = lds + row_lds + lead[1];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float p00 = (float)r0[o0 + c], p01 = (float)r0[o1 + c];
        const float p10 = (float)r1[o0 + c], p11 = (float)r1[o1 + c];
        const float top = (1.0f - wx) * p00 + wx * p01;
        const float bot = (1.0f - wx) * p10 + wx * p11;
        const unsigned q = (unsigned)rintf((1.0f - wy) * top + wy * bot);      // ties to even
        s1[c] += q;
        s2[c] += q * q;
        if (words)
          line[tid * 3 + c] = (unsigned char)q;
        else
          ref[(((int64_t)v * H + y) * W + x) * 3 + c] = (unsigned char)q;
      }
    }
    __syncthreads();
    if (words && tid * 4 < line_bytes) {
      unsigned* out = reinterpret_cast<unsigned*>(ref + (((int64_t)v * H + y) * W + x_first) * 3);
      out[tid] = reinterpret_cast<const unsigned*>(line)[tid];
    }
  }
  // block totals: 256 x kRows values of at most 255 (65 025 squared) fit 32 bits
  unsigned vals[6] = {s1[0], s1[1], s1[2], s2[0], s2[1], s2[2]};
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    unsigned a = vals[k];
    for (int off = PF_WAVE / 2; off > 0; off >>= 1) a += __shfl_down(a, off, PF_WAVE);
    if ((tid & (PF_WAVE - 1)) == 0) red[tid / PF_WAVE][k] = a;
  }
  __syncthreads();
  if (tid < 6) {
    unsigned long long t = 0;
    for (int wv = 0; wv < kTileX / PF_WAVE; ++wv) t += red[wv][tid];
    // sums (V, 3, 2): [.., 0] = sum p, [.., 1] = sum p*p
    atomicAdd(&sums[((int64_t)v * 3 + (tid % 3)) * 2 + tid / 3], t);
  }
}

__global__ __launch_bounds__(256) void standardise_kernel(const unsigned char* __restrict__ ref,
                                                          const unsigned long long* __restrict__ sums, int HW,
                                                          float* __restrict__ out) {
  PF_PRE_LDS float lut[3][256];
  const int tid = threadIdx.x;
  const int v = blockIdx.y;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const unsigned long long n = (unsigned long long)HW;
    const unsigned long long a = sums[((int64_t)v * 3 + c) * 2], b = sums[((int64_t)v * 3 + c) * 2 + 1];
    const double mean = (double)a / (double)n;
    const double var = (double)(n * b - a * a) / ((double)n * (double)n);      // the numerator is exact: HW <= 2^24
    lut[c][tid] = (float)(((double)tid - mean) / (sqrt(var) + 1e-7));
  }
  __syncthreads();
  const unsigned char* __restrict__ img = ref + (int64_t)v * HW * 3;
  float* __restrict__ planes = out + (int64_t)v * 3 * HW;
  if ((HW & 3) == 0) {
    for (int it = 0; it < kGroups; ++it) {
      const int g = (blockIdx.x * kGroups + it) * 256 + tid;               // pixels 4g .. 4g+3: 12 aligned bytes
      if (4 * (int64_t)g >= HW) break;
      const unsigned* __restrict__ in = reinterpret_cast<const unsigned*>(img + (int64_t)g * 12);
      const unsigned w0 = in[0], w1 = in[1], w2 = in[2];
      const unsigned px[4][3] = {{w0 & 255u, (w0 >> 8) & 255u, (w0 >> 16) & 255u},
                                 {w0 >> 24, w1 & 255u, (w1 >> 8) & 255u},
                                 {(w1 >> 16) & 255u, w1 >> 24, w2 & 255u},
                                 {(w2 >> 8) & 255u, (w2 >> 16) & 255u, w2 >> 24}};
#pragma unroll
      for (int c = 0; c < 3; ++c)
        *reinterpret_cast<float4*>(planes + (int64_t)c * HW + 4 * (int64_t)g) =
            make_float4(lut[c][px[0][c]], lut[c][px[1][c]], lut[c][px[2][c]], lut[c][px[3][c]]);
    }
  } else {
    for (int it = 0; it < 4 * kGroups; ++it) {
      const int64_t p = ((int64_t)blockIdx.x * 4 * kGroups + it) * 256 + tid;
      if (p >= HW) break;
#pragma unroll
      for (int c = 0; c < 3; ++c) planes[(int64_t)c * HW + p] = lut[c][img[p * 3 + c]];
    }
  }
}

}  // namespace

extern "C" {

int pf_preprocess_resize_u8(const unsigned char* src, int V, int h_src, int w_src, const int* xi, const float* xw,
                            const int* yi, const float* yw, int H, int W, int span, unsigned char* ref,
                            unsigned long long* sums, void* stream) {
  PF_REQUIRE(V >= 1 && V <= 65535 && h_src >= 1 && w_src >= 1 && H >= 1 && W >= 1 && span >= 1);
  PF_REQUIRE((int64_t)h_src * w_src <= (1 << 24) && (int64_t)H * W <= (1 << 24) && pf_cdiv(H, kRows) <= 65535);
  PF_REQUIRE(src && xi && xw && yi && yw && ref && sums);
  PF_REQUIRE(((uintptr_t)src & 15) == 0 && ((uintptr_t)ref & 3) == 0 && ((uintptr_t)sums & 7) == 0);
  const int row_lds = (int)(pf_cdiv((int64_t)span * 3 + 15, 16) * 16);
  const int lds = 2 * row_lds + kTileX * 3;
  PF_REQUIRE(lds <= 48 * 1024);                        // a tile may not span more than ~8000 source columns
  const int rc = pf_zero_async(sums, (size_t)V * 6 * sizeof(unsigned long long), (hipStream_t)stream);
  if (rc != PF_OK) return rc;
  hipLaunchKernelGGL(resize_crop_kernel, dim3((unsigned)pf_cdiv(W, kTileX), (unsigned)pf_cdiv(H, kRows), (unsigned)V),
                     dim3(kTileX), (size_t)lds, (hipStream_t)stream, src, h_src, w_src, xi, xw, yi, yw, H, W, span, row_lds,
                     ref, sums);
  return pf_launch_status();
}

int pf_preprocess_standardise_f32(const unsigned char* ref, const unsigned long long* sums, int V, int H, int W,
                                  float* out, void* stream) {
  PF_REQUIRE(V >= 1 && V <= 65535 && H >= 1 && W >= 1 && (int64_t)H * W <= (1 << 24));
  PF_REQUIRE(ref && sums && out);
  PF_REQUIRE(((uintptr_t)ref & 3) == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)sums & 7) == 0);
  const int HW = H * W;
  hipLaunchKernelGGL(standardise_kernel, dim3((unsigned)pf_cdiv(HW, 256 * 4 * kGroups), (unsigned)V), dim3(256), 0,
                     (hipStream_t)stream, ref, sums, HW, out);
  return pf_launch_status();
}

}  // extern "C"
