// The confidence filter of a whole scan in one launch: what reference tools/depthfusion.py:153-170 does per view on
// files (cv2.resize of the confidence maps, two comparisons), for all V views on the device, in the reference's four
// interpolation modes.  The specification is pointmvsnet_amd/scan.py; the resampling part of it is this project's own
// statement of what cv2.resize does to float32 (separable, replicate border, no prefilter).
//
//   scan_filter<T>   one block = a 32 x 8 tile of output pixels of one view, one lane per pixel; T = taps per axis
//                    (1 NEAREST, 2 BILINEAR, 4 CUBIC, 8 LANCZOS4), so the short modes are not padded to eight.
//                    Per confidence map that is not of the depth map's size: the tile's source footprint (the tile's
//                    share of the source plus up to T taps per axis; a few hundred floats at 2x / 4x upsampling) is
//                    staged into LDS once with clamped row / column ranges, the horizontal pass writes a strip of
//                    (footprint rows) x 32 floats, the vertical pass reads it.  Both sums run in ascending tap order in
//                    float32 (the unit is compiled with -ffp-contract=off).  A map of the depth map's size is read
//                    directly, as the reference does not resize it.  Raw flow probabilities go through
//                    pf_flow_confidence, the rule of
//                    pf_eval_flow_prob_f32.  Each lane then applies the two comparisons and stores one float; the block
//                    counts its kept pixels (wave shuffles, 4 LDS words) and adds ONE integer to the view's total.
//
// Every tap index is clamped into the source and then into the staged footprint, so tables that are not the
// non-decreasing ones of scan.resize_taps can only give wrong pixels, never an address outside a buffer.
//
// Bytes per output pixel (the algo_bytes of scan.py): 4 of depth, 20 of raw flow probability (or 4 fh fw / (h w) of a made
// confidence), 4 ih iw / (h w) of coarse confidence, 4 written.
#include "pf_common.h"

// (see preprocess.hip: the host re-compilation of tests/hipemu reaches this file through eval_out.hip)
#if defined(__HIP__)
#define PF_SF_LDS __shared__
#define PF_SF_LDS_DYNAMIC(name) extern __shared__ __attribute__((aligned(16))) float name[]
#else
#define PF_SF_LDS static thread_local
#define PF_SF_LDS_DYNAMIC(name) float* name = reinterpret_cast<float*>(::hipemu_shared_memory())
#endif

namespace {

constexpr int kSfTileX = PF_SCAN_FILTER_TILE_X;
constexpr int kSfTileY = PF_SCAN_FILTER_TILE_Y;
constexpr int kSfThreads = kSfTileX * kSfTileY;
constexpr int kSfMaxLds = 48 * 1024;

__device__ __forceinline__ int sf_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// one confidence input: maps (V, sh, sw) and the tap tables of its two axes for the (h, w) output
struct SfSource {
  const float* maps;
  int sh, sw;
  const int* ys;       // (h)     first tap's source row, before clamping
  const float* yw;     // (h, T)
  const int* xs;       // (w)
  const float* xw;     // (w, T)
  int span_y, span_x;  // the LDS footprint's rows / columns
  float* resized;      // (V, h, w) or NULL: the resampled map, for the tests
};

struct SfArgs {
  const float* depth;
  const float* flow_prob;      // (V, 5, h, w) or NULL
  SfSource flow, init;         // flow.maps is NULL when flow_prob is given
  int h, w;
  float flow_thr, init_thr;
  float* filtered;
  int* kept;
};

inline int sf_taps(int mode) {
  return mode == PF_SCAN_NEAREST ? 1 : mode == PF_SCAN_BILINEAR ? 2 : mode == PF_SCAN_CUBIC ? 4
         : mode == PF_SCAN_LANCZOS4 ? 8 : 0;
}

// rows / columns of source that a tile of `tile` outputs can touch: its first taps lie at most
// floor((tile - 1) * s / n) + 1 apart, plus the taps themselves
inline int64_t sf_span(int tile, int s, int n, int T) { return ((int64_t)(tile - 1) * s) / n + T + 2; }

inline int64_t sf_lds_floats(int sh, int sw, int h, int w, int T) {
  if (sh == h && sw == w) return 0;
  const int64_t sy = sf_span(kSfTileY, sh, h, T), sx = sf_span(kSfTileX, sw, w, T);
  return sy * sx + sy * kSfTileX;
}

// The resampled value of this lane's pixel (x0 + tx, y0 + ty); every lane of the block takes part.
template <int T>
__device__ __forceinline__ float sf_resample(const SfSource& s, int v, int x0, int y0, int h, int w, float* lds) {
  const int tid = threadIdx.x, tx = tid % kSfTileX, ty = tid / kSfTileX;
  const float* __restrict__ src = s.maps + (int64_t)v * s.sh * s.sw;
  float* tile = lds;                                  // (span_y, span_x)
  float* strip = lds + s.span_y * s.span_x;           // (span_y, kSfTileX)
  const int x_last = min(x0 + kSfTileX - 1, w - 1), y_last = min(y0 + kSfTileY - 1, h - 1);
  const int xlo = sf_clamp(s.xs[x0], 0, s.sw - 1), xhi = sf_clamp(s.xs[x_last] + T - 1, 0, s.sw - 1);
  const int ylo = sf_clamp(s.ys[y0], 0, s.sh - 1), yhi = sf_clamp(s.ys[y_last] + T - 1, 0, s.sh - 1);
  const int nx = sf_clamp(xhi - xlo + 1, 1, s.span_x), ny = sf_clamp(yhi - ylo + 1, 1, s.span_y);
  for (int i = tid; i < ny * nx; i += kSfThreads) {
    const int r = i / nx, c = i - r * nx;             // ylo + r <= yhi and xlo + c <= xhi: inside the map
    tile[r * s.span_x + c] = src[(int64_t)(ylo + r) * s.sw + xlo + c];
  }
  __syncthreads();
  const int x = min(x0 + tx, w - 1), y = min(y0 + ty, h - 1);
  {
    int cx[T];
    float wx[T];
    const int first = s.xs[x];
#pragma unroll
    for (int k = 0; k < T; ++k) {
      cx[k] = sf_clamp(sf_clamp(first + k, 0, s.sw - 1) - xlo, 0, nx - 1);
      wx[k] = s.xw[(int64_t)x * T + k];
    }
    for (int r = ty; r < ny; r += kSfTileY) {
      const float* __restrict__ row = tile + r * s.span_x;
      float acc = T == 1 ? row[cx[0]] : row[cx[0]] * wx[0];
#pragma unroll
      for (int k = 1; k < T; ++k) acc += row[cx[k]] * wx[k];
      strip[r * kSfTileX + tx] = acc;
    }
  }
  __syncthreads();
  const int first = s.ys[y];
  float acc = 0.0f;
#pragma unroll
  for (int k = 0; k < T; ++k) {
    const int r = sf_clamp(sf_clamp(first + k, 0, s.sh - 1) - ylo, 0, ny - 1);
    const float val = strip[r * kSfTileX + tx];
    if (T == 1)
      acc = val;
    else
      acc = k == 0 ? val * s.yw[(int64_t)y * T] : acc + val * s.yw[(int64_t)y * T + k];
  }
  __syncthreads();                                     // the next map re-uses the LDS
  return acc;
}

template <int T>
__global__ __launch_bounds__(kSfThreads) void scan_filter_kernel(SfArgs a) {
  PF_SF_LDS_DYNAMIC(lds);
  PF_SF_LDS int red[kSfThreads / PF_WAVE];
  const int tid = threadIdx.x, tx = tid % kSfTileX, ty = tid / kSfTileX;
  const int v = blockIdx.z;
  const int x0 = blockIdx.x * kSfTileX, y0 = blockIdx.y * kSfTileY;
  const int h = a.h, w = a.w;
  const int x = x0 + tx, y = y0 + ty;
  const bool active = x < w && y < h;
  const int hw = h * w;
  const int i = active ? y * w + x : 0;
  const int64_t at = (int64_t)v * hw + i;

  float ci;
  if (a.init.sh == h && a.init.sw == w)
    ci = a.init.maps[at];
  else
    ci = sf_resample<T>(a.init, v, x0, y0, h, w, lds);
  float cf;
  if (a.flow_prob != nullptr)
    cf = pf_flow_confidence(a.flow_prob + (int64_t)v * 5 * hw, i, hw);
  else if (a.flow.sh == h && a.flow.sw == w)
    cf = a.flow.maps[at];
  else
    cf = sf_resample<T>(a.flow, v, x0, y0, h, w, lds);

  // NumPy's depth[prob < thr] = 0: a NaN confidence compares false and keeps the depth
  const bool drop = (cf < a.flow_thr) || (ci < a.init_thr);
  if (active) {
    a.filtered[at] = drop ? 0.0f : a.depth[at];
    if (a.init.resized != nullptr) a.init.resized[at] = ci;
    if (a.flow.resized != nullptr) a.flow.resized[at] = cf;
  }
  int n = (active && !drop) ? 1 : 0;
  for (int off = PF_WAVE / 2; off > 0; off >>= 1) n += __shfl_down(n, off, PF_WAVE);
  if ((tid & (PF_WAVE - 1)) == 0) red[tid / PF_WAVE] = n;
  __syncthreads();
  if (tid == 0) {
    int t = 0;
    for (int wv = 0; wv < kSfThreads / PF_WAVE; ++wv) t += red[wv];
    if (t != 0) atomicAdd(&a.kept[v], t);              // integer: the same total whatever the arrival order
  }
}

template <int T>
int sf_launch(const SfArgs& a, int V, size_t lds_bytes, hipStream_t stream) {
  hipLaunchKernelGGL(scan_filter_kernel<T>,
                     dim3((unsigned)pf_cdiv(a.w, kSfTileX), (unsigned)pf_cdiv(a.h, kSfTileY), (unsigned)V),
                     dim3(kSfThreads), lds_bytes, stream, a);
  return pf_launch_status();
}

}  // namespace

extern "C" {

int pf_scan_filter_supported(int mode, int h, int w, int fh, int fw, int ih, int iw) {
  const int T = sf_taps(mode);
  if (T == 0 || h < 1 || w < 1 || fh < 1 || fw < 1 || ih < 1 || iw < 1) return 0;
  if ((int64_t)h * w > (1 << 24) || (int64_t)fh * fw > (1 << 24) || (int64_t)ih * iw > (1 << 24)) return 0;
  if (pf_cdiv(h, kSfTileY) > 65535) return 0;
  const int64_t a = sf_lds_floats(fh, fw, h, w, T), b = sf_lds_floats(ih, iw, h, w, T);
  return (a > b ? a : b) * 4 <= kSfMaxLds ? 1 : 0;
}

int pf_scan_filter_f32(const float* depth, const float* flow_prob, const float* flow_conf, int fh, int fw,
                       const float* init_conf, int ih, int iw, int V, int h, int w, int mode, const int* flow_ys,
                       const float* flow_yw, const int* flow_xs, const float* flow_xw, const int* init_ys,
                       const float* init_yw, const int* init_xs, const float* init_xw, float flow_threshold,
                       float init_threshold, float* filtered, int* kept, float* flow_resized, float* init_resized,
                       void* stream) {
  PF_REQUIRE(V >= 0 && V <= 65535 && h >= 0 && w >= 0);
  PF_REQUIRE(kept != nullptr || V == 0);
  if (V > 0) {
    const int rc = pf_zero_async(kept, (size_t)V * sizeof(int), (hipStream_t)stream);
    if (rc != PF_OK) return rc;
  }
  if (V == 0 || h == 0 || w == 0) return PF_OK;
  PF_REQUIRE(depth && init_conf && filtered && filtered != depth);
  PF_REQUIRE((flow_prob != nullptr) != (flow_conf != nullptr));            // exactly one form of flow confidence
  if (flow_prob != nullptr) fh = h, fw = w;
  if (!pf_scan_filter_supported(mode, h, w, fh, fw, ih, iw)) return PF_ERR_UNSUPPORTED;
  const bool flow_resample = flow_conf != nullptr && (fh != h || fw != w);
  const bool init_resample = ih != h || iw != w;
  PF_REQUIRE(!flow_resample || (flow_ys && flow_yw && flow_xs && flow_xw));
  PF_REQUIRE(!init_resample || (init_ys && init_yw && init_xs && init_xw));
  const int T = sf_taps(mode);
  SfArgs a;
  a.depth = depth;
  a.flow_prob = flow_prob;
  a.flow = SfSource{flow_conf, fh, fw, flow_ys, flow_yw, flow_xs, flow_xw, (int)sf_span(kSfTileY, fh, h, T),
                    (int)sf_span(kSfTileX, fw, w, T), flow_resized};
  a.init = SfSource{init_conf, ih, iw, init_ys, init_yw, init_xs, init_xw, (int)sf_span(kSfTileY, ih, h, T),
                    (int)sf_span(kSfTileX, iw, w, T), init_resized};
  a.h = h;
  a.w = w;
  a.flow_thr = flow_threshold;
  a.init_thr = init_threshold;
  a.filtered = filtered;
  a.kept = kept;
  const int64_t fa = flow_resample ? sf_lds_floats(fh, fw, h, w, T) : 0;
  const int64_t fb = init_resample ? sf_lds_floats(ih, iw, h, w, T) : 0;
  const size_t lds_bytes = (size_t)(fa > fb ? fa : fb) * sizeof(float);
  switch (T) {
    case 1: return sf_launch<1>(a, V, lds_bytes, (hipStream_t)stream);
    case 2: return sf_launch<2>(a, V, lds_bytes, (hipStream_t)stream);
    case 4: return sf_launch<4>(a, V, lds_bytes, (hipStream_t)stream);
    default: return sf_launch<8>(a, V, lds_bytes, (hipStream_t)stream);
  }
}

}  // extern "C"
