// Photometric consistency of depth maps: windowed zero-mean normalised cross-correlation (ZNCC) between a view's grey image
// and its source views' grey images, warped through the pixel's depth (specification: pointmvsnet_amd/photometric.py,
// include/pointflow_hip.h).  Pixel centres at (x + 0.5, y + 0.5) as in fusion.hip.
//
//   grey_pack   one thread per pixel: 3 bytes in, 1 out, g = (77 R + 150 G + 29 B + 128) >> 8.
//   grey_quads  one thread per pixel: the 2 x 2 grey bytes whose top-left corner is the pixel, as one dword
//               g(y, x) | g(y, x + 1) << 8 | g(y + 1, x) << 16 | g(y + 1, x + 1) << 24 (a neighbour beyond the last column or
//               row repeats the last one; no tap that is inside reads such a byte).  A bilinear tap is then ONE 32-bit
//               load instead of four byte loads.
//   photo_ncc   one thread per pixel of every view, pf_tile_pixel's 16 x 16 tiles, blockIdx.z the view.  A block stages the
//               (16 + 2 r)^2 grey bytes under its tile and r more on every side (the low bytes of the view's own quads) in
//               dynamic LDS (a byte outside the image is staged as 0: a pixel whose window leaves the image is decided by
//               its coordinates and never reads it), one barrier, then every thread forms its window's integer sums SR,
//               SRR and VR once.  A pixel that is not scorable writes its zeros and NaNs and leaves.  The mask byte
//               carries `scorable` in bit 1 for the report.  The source slot is the outer loop: the view is blockIdx.z
//               and the slot the loop counter, so the table entry and the pair row are wave-uniform and are read by scalar
//               loads into SGPRs, as in geo_filter_kernel.  Per tap: one LDS byte (the reference value is read again, not
//               kept: no per-thread array, no scratch), the full map, one division, one floor and one dword gather from
//               the source's quads (4 h w bytes per view, L2-resident).  A lane whose tap has left the source keeps the
//               clamped address 0 and goes on: its sums are dropped at the end of the slot.
//               The radius is a template argument for r = 1, 2, 3 (the tap loops unroll: the pixel coordinates, the LDS
//               offsets and m1 py + m2 become constants or are hoisted) and a runtime value for r = 4, 5.
//               Measured on an MI355X, 49 views of 640 x 480, 10 sources, r = 1 / 2 / 3: runtime
//               loop with byte loads 2.42 / 6.12 / 11.1 ms; this arm 2.16 / 5.54 / 10.0 ms; the template alone 2.20 / 5.70 /
//               19.7 ms (256 VGPRs at r = 3 with four byte loads in flight per tap); the quads alone 2.36 / 5.89 / 10.8 ms;
//               32 x 8 tiles 2.46 / 6.15 / 11.3 ms.
// No atomics: two runs give identical bytes.
#include "pf_camera.h"

// hipcc spells LDS `__shared__`.  The host re-compilation of tests/hipemu rewrites that spelling in the sources of its fixed
// list only; it reaches this file through eval_out.hip, so the emulator's spelling is chosen here (as in depth_refine.hip).
#if defined(__HIP__)
#define PF_PHOTO_LDS_DYNAMIC(name) extern __shared__ __attribute__((aligned(16))) unsigned char name[]
#else
#define PF_PHOTO_LDS_DYNAMIC(name) unsigned char* name = reinterpret_cast<unsigned char*>(::hipemu_shared_memory())
#endif

namespace {

constexpr unsigned kPhotoNoValue = 0x7fc00000u;      // the quiet NaN of a source that is not usable

__global__ __launch_bounds__(256) void photo_grey_pack_kernel(const unsigned char* __restrict__ rgb, int64_t n,
                                                              unsigned char* __restrict__ grey) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const unsigned char* __restrict__ c = rgb + p * 3;
  grey[p] = (unsigned char)((77u * c[0] + 150u * c[1] + 29u * c[2] + 128u) >> 8);
}

__global__ __launch_bounds__(256) void photo_grey_quads_kernel(const unsigned char* __restrict__ grey, int h, int w,
                                                               unsigned* __restrict__ quads) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= h * w) return;
  const int y = p / w, x = p - y * w;
  const int x1 = x + 1 < w ? x + 1 : x, y1 = y + 1 < h ? y + 1 : y;
  const unsigned char* __restrict__ g = grey + (int64_t)blockIdx.y * h * w;
  quads[(int64_t)blockIdx.y * h * w + p] = (unsigned)g[y * w + x] | ((unsigned)g[y * w + x1] << 8) |
                                           ((unsigned)g[y1 * w + x] << 16) | ((unsigned)g[y1 * w + x1] << 24);
}

template <int RT>                          // the radius, or 0: the radius is r_arg
__global__ __launch_bounds__(kPfTile * kPfTile) void photo_ncc_kernel(
    const float* __restrict__ depth, const unsigned* __restrict__ quads, const int* __restrict__ sources,
    const float* __restrict__ pair_maps, int V, int M, int h, int w, int r_arg, int var_min, float ncc_threshold,
    int num_consistent, float depth_min, float depth_max, float* __restrict__ ncc, float* __restrict__ score,
    int* __restrict__ count, int* __restrict__ usable, unsigned char* __restrict__ mask) {
  PF_PHOTO_LDS_DYNAMIC(win);                                  // F rows of F grey bytes
  const int r = RT > 0 ? RT : r_arg;
  const int F = kPfTile + 2 * r;
  const int i = blockIdx.z;
  const int hw = h * w;
  const unsigned* __restrict__ own = quads + (int64_t)i * hw;
  const int x_lo = (int)(blockIdx.x * kPfTile) - r, y_lo = (int)(blockIdx.y * kPfTile) - r;
  for (int k = threadIdx.x; k < F * F; k += kPfTile * kPfTile) {
    const int fy = k / F, fx = k - fy * F;
    const int gx = x_lo + fx, gy = y_lo + fy;
    const bool in_image = gx >= 0 && gx < w && gy >= 0 && gy < h;
    win[k] = in_image ? (unsigned char)(own[gy * w + gx] & 255u) : (unsigned char)0;
  }
  __syncthreads();

  int x, y, unused;
  pf_tile_pixel(x, y, unused);
  if (x >= w || y >= h) return;
  const int p = y * w + x;
  const int64_t ip = (int64_t)i * hw + p;
  const unsigned char* __restrict__ centre = win + (y - y_lo) * F + (x - x_lo);
  const int c = centre[0];
  const int n = (2 * r + 1) * (2 * r + 1);
  int SR = 0, SRR = 0;
  for (int dy = -r; dy <= r; ++dy)
    for (int dx = -r; dx <= r; ++dx) {
      const int R = (int)centre[dy * F + dx] - c;
      SR += R;
      SRR += R * R;
    }
  const int VR = n * SRR - SR * SR;
  const float d = depth[ip];
  const bool scorable = d > depth_min && d < depth_max && x >= r && x < w - r && y >= r && y < h - r && VR >= var_min;
  const float none = __uint_as_float(kPhotoNoValue);
  if (!scorable) {
    if (ncc)
      for (int m = 0; m < M; ++m) ncc[((int64_t)i * M + m) * hw + p] = none;
    score[ip] = 0.0f;
    count[ip] = 0;
    usable[ip] = 0;
    mask[ip] = 0;
    return;
  }
  const float cf = (float)c, nf = (float)n, SRf = (float)SR, VRf = (float)VR, var_min_f = (float)var_min;
  const float xlast = (float)(w - 1), ylast = (float)(h - 1);
  float total = 0.0f;
  int good = 0, used = 0;
  for (int m = 0; m < M; ++m) {
    const int j = sources[(int64_t)i * M + m];
    if (j < 0 || j >= V || j == i) {                        // wave-uniform: a pad, or the view itself
      if (ncc) ncc[((int64_t)i * M + m) * hw + p] = none;
      continue;
    }
    const float* __restrict__ f = pair_maps + ((int64_t)i * M + m) * (2 * PF_FUSE_PAIR_FLOATS);   // i -> j
    const unsigned* __restrict__ plane = quads + (int64_t)j * hw;
    float S1 = 0.0f, S2 = 0.0f, SX = 0.0f;
    bool all_inside = true;
    for (int dy = -r; dy <= r; ++dy) {
      const float py = (float)(y + dy) + 0.5f;
      for (int dx = -r; dx <= r; ++dx) {
        const int R = (int)centre[dy * F + dx] - c;
        const float px = (float)(x + dx) + 0.5f;
        float qx, qy, z;
        pf_apply_map(f, px, py, d, qx, qy, z);
        const float rz = 1.0f / z;
        const float u = qx * rz, v = qy * rz;
        const float fx = u - 0.5f, fy = v - 0.5f;
        const float x0 = floorf(fx), y0 = floorf(fy);
        // all four taps inside the image, no border replication; false for NaN, so the conversions below are in range
        const bool inside = z > 0.0f && x0 >= 0.0f && x0 + 1.0f <= xlast && y0 >= 0.0f && y0 + 1.0f <= ylast;
        all_inside = all_inside && inside;
        const int q = inside ? (int)y0 * w + (int)x0 : 0;
        const unsigned t = plane[q];
        const float t00 = (float)(t & 255u), t01 = (float)((t >> 8) & 255u);
        const float t10 = (float)((t >> 16) & 255u), t11 = (float)(t >> 24);
        const float wx = fx - x0, wy = fy - y0;
        const float top = t00 * (1.0f - wx) + t01 * wx;
        const float bot = t10 * (1.0f - wx) + t11 * wx;
        const float s = (top * (1.0f - wy) + bot * wy) - cf;
        S1 += s;
        S2 += s * s;
        SX += (float)R * s;
      }
    }
    const float VS = nf * S2 - S1 * S1;
    const float COV = nf * SX - SRf * S1;
    const bool ok = all_inside && VS >= var_min_f;
    const float val = fminf(1.0f, fmaxf(-1.0f, COV / sqrtf(VRf * VS)));
    if (ok) {
      total += val;
      ++used;
      good += val >= ncc_threshold ? 1 : 0;
    }
    if (ncc) ncc[((int64_t)i * M + m) * hw + p] = ok ? val : none;
  }
  score[ip] = used > 0 ? total / (float)used : 0.0f;
  count[ip] = good;
  usable[ip] = used;
  mask[ip] = (unsigned char)(2 | (good >= num_consistent ? 1 : 0));   // bit 1: scorable
}

}  // namespace

extern "C" {

int pf_grey_pack_u8(const unsigned char* rgb, int64_t n, unsigned char* grey, void* stream) {
  PF_REQUIRE(n >= 0 && pf_cdiv(n, 256) <= INT32_MAX);
  if (n == 0) return PF_OK;
  PF_REQUIRE(rgb && grey);
  hipLaunchKernelGGL(photo_grey_pack_kernel, dim3((unsigned)pf_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, rgb, n,
                     grey);
  return pf_launch_status();
}

int pf_grey_quads_u8(const unsigned char* grey, int V, int h, int w, unsigned* quads, void* stream) {
  PF_REQUIRE(V >= 1 && V <= 65535 && h >= 0 && w >= 0 && (int64_t)h * w <= INT32_MAX / 4);
  if (h == 0 || w == 0) return PF_OK;
  PF_REQUIRE(grey && quads);
  hipLaunchKernelGGL(photo_grey_quads_kernel, dim3((unsigned)pf_cdiv((int64_t)h * w, 256), (unsigned)V), dim3(256), 0,
                     (hipStream_t)stream, grey, h, w, quads);
  return pf_launch_status();
}

int pf_photo_ncc_f32(const float* depth, const unsigned* quads, const int* sources, const float* pair_maps, int V, int M,
                     int h, int w, int radius, int var_min, float ncc_threshold, int num_consistent, float depth_min,
                     float depth_max, float* ncc, float* score, int* count, int* usable, unsigned char* mask, void* stream) {
  PF_REQUIRE(V >= 1 && V <= 65535 && M >= 0 && h >= 0 && w >= 0 && (int64_t)h * w <= INT32_MAX / 4);
  PF_REQUIRE(radius >= 1 && radius <= 5 && var_min >= 1 && pf_cdiv(h, kPfTile) <= 65535);
  if (h == 0 || w == 0) return PF_OK;
  PF_REQUIRE(depth && quads && score && count && usable && mask && ((sources && pair_maps) || M == 0));
  const int F = kPfTile + 2 * radius;
  const dim3 grid((unsigned)pf_cdiv(w, kPfTile), (unsigned)pf_cdiv(h, kPfTile), (unsigned)V);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, dim3(kPfTile * kPfTile), (size_t)F * F, (hipStream_t)stream, depth, quads, sources,
                       pair_maps, V, M, h, w, radius, var_min, ncc_threshold, num_consistent, depth_min, depth_max, ncc, score,
                       count, usable, mask);
  };
  if (radius == 1) launch(photo_ncc_kernel<1>);
  else if (radius == 2) launch(photo_ncc_kernel<2>);
  else if (radius == 3) launch(photo_ncc_kernel<3>);
  else launch(photo_ncc_kernel<0>);
  return pf_launch_status();
}

}  // extern "C"
