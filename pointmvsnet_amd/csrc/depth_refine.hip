// Guided (joint bilateral) upsampling of depth maps by the image the network saw (specification: pointmvsnet_amd/refine.py,
// include/pointflow_hip.h).  Pixel centres at (x + 0.5, y + 0.5) as in fusion.hip.
//
//   guide_pack      one thread per LOW-resolution pixel q of every view: an 8-byte record {bits of d(q), r | g << 8 | b << 16}
//                   of the guide pixel that contains q's centre, guide[qy s + s/2][qx s + s/2].  The strided 3-byte gathers
//                   happen once per low-resolution pixel here, not once per block that has the pixel in its halo.
//   depth_upsample  one thread per OUTPUT pixel, 16 x 16 output tiles, blockIdx.z the view.  A block stages the records of
//                   its footprint -- the low-resolution pixels under the tile and `radius` more on every side, F x F with
//                   F = (16 / s if s divides 16, else 16 / s + 2) + 2 radius <= 32 -- in dynamic LDS, then the colour table wc
//                   (766 floats) and the whole spatial table ws (s rows of 2 radius + 1); one barrier.  valid(q) is decided
//                   ONCE per staged record, by the thread that stages it: the depth of an entry that is outside the map or
//                   not inside (depth_min, depth_max) is stored as NaN.  A NaN fails `|d - d0| <= jump` by itself, so the
//                   mean's tap loop has no validity test and no in-map test at all, and the anchor's has one (d == d).
//                   Per tap: one ds_read_b64 of the record, v_sad_u8 against the pixel's own colour, one read of wc and
//                   one of ws[px][tx] (ws[py][ty] is read once per tap row).
//                   LDS layout: records row-major with a pitch of P records = 2 P dwords.  ds_read_b64 is served in two
//                   groups of 32 lanes = two output rows of the tile, over 64 banks of 4 bytes.  For s = 2, 4, 8 both rows
//                   lie in one low-resolution row: 16 / s consecutive records, the s lanes of a record on ONE address
//                   (a broadcast), no conflict.  For s = 3, 5, 6, 7 the two rows can lie in adjacent record rows of at
//                   most 6 records (12 dwords) each; 2 P is 10 .. 46 for those s, so the two runs never meet on a bank.
//                   For s = 1 the rows are 16 records = 32 dwords each and P = F = 16 + 2 radius would put them 2 F mod 64
//                   banks apart (40 at radius 2: a 2-way conflict on 8 banks); there P is raised to the next value with
//                   P mod 32 == 16 (16 or 48), which puts the second row exactly on the other 32 banks.
//                   The tap loops have runtime bounds and no per-thread arrays: no scratch.  The count map has its own
//                   template arm.
// No atomics: two runs give identical bytes.
#include "pf_camera.h"

// hipcc spells LDS `__shared__`.  The host re-compilation of tests/hipemu rewrites that spelling in the sources of its fixed
// list only; it reaches this file through eval_out.hip, so the emulator's spelling is chosen here (as in preprocess.hip).
#if defined(__HIP__)
#define PF_REFINE_LDS_DYNAMIC(name) extern __shared__ __attribute__((aligned(16))) unsigned char name[]
#else
#define PF_REFINE_LDS_DYNAMIC(name) unsigned char* name = reinterpret_cast<unsigned char*>(::hipemu_shared_memory())
#endif

namespace {

constexpr int kWcEntries = 766;        // a = |dr| + |dg| + |db| in [0, 765]
constexpr int kWcFloats = 768;
constexpr unsigned kNoDepth = 0x7fc00000u;      // a quiet NaN in LDS: a tap that is outside the map or not valid

__device__ __forceinline__ unsigned pack_rgb(const unsigned char* __restrict__ p) {
  return (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16);
}

// |r - r'| + |g - g'| + |b - b'| of two packed colours (their top bytes are both 0)
__device__ __forceinline__ int colour_distance(unsigned a, unsigned b) {
#if defined(__HIP__)
  return (int)__builtin_amdgcn_sad_u8(a, b, 0u);               // v_sad_u8: the sum over the four bytes
#else
  int sum = 0;
  for (int k = 0; k < 24; k += 8) {
    const int d = (int)((a >> k) & 255u) - (int)((b >> k) & 255u);
    sum += d < 0 ? -d : d;
  }
  return sum;
#endif
}

__global__ __launch_bounds__(256) void guide_pack_kernel(const float* __restrict__ depth,
                                                         const unsigned char* __restrict__ guide, int h, int w, int s,
                                                         uint2* __restrict__ records) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  const int view = blockIdx.y;
  if (p >= h * w) return;
  const int qy = p / w, qx = p - qy * w;
  const int64_t W = (int64_t)w * s;
  const int64_t g = ((int64_t)view * h * s + (qy * s + s / 2)) * W + (qx * s + s / 2);
  const int64_t ip = (int64_t)view * h * w + p;
  records[ip] = make_uint2(__float_as_uint(depth[ip]), pack_rgb(guide + g * 3));
}

template <bool COUNT>
__global__ __launch_bounds__(kPfTile * kPfTile) void depth_upsample_kernel(
    const uint2* __restrict__ records, const unsigned char* __restrict__ guide, const float* __restrict__ ws,
    const float* __restrict__ wc, int h, int w, int s, int radius, int anchor_radius, int F, int P, float rel_jump,
    float depth_min, float depth_max, float* __restrict__ out, int* __restrict__ count) {
  PF_REFINE_LDS_DYNAMIC(lds);
  uint2* __restrict__ rec_s = reinterpret_cast<uint2*>(lds);                      // F rows of P records
  float* __restrict__ wc_s = reinterpret_cast<float*>(lds + (size_t)F * P * 8);   // kWcFloats
  float* __restrict__ ws_s = wc_s + kWcFloats;                                    // s * (2 radius + 1)
  const int taps = 2 * radius + 1;
  const int tid = threadIdx.x;
  const int view = blockIdx.z;
  const int x_lo = (int)(blockIdx.x * kPfTile) / s - radius;     // the footprint's first low-resolution column and row
  const int y_lo = (int)(blockIdx.y * kPfTile) / s - radius;
  const uint2* __restrict__ plane = records + (int64_t)view * h * w;
  for (int i = tid; i < F * F; i += kPfTile * kPfTile) {
    const int fy = i / F, fx = i - fy * F;
    const int qx = x_lo + fx, qy = y_lo + fy;
    const bool inside = qx >= 0 && qx < w && qy >= 0 && qy < h;
    uint2 r = inside ? plane[qy * w + qx] : make_uint2(kNoDepth, 0u);
    const float d = __uint_as_float(r.x);
    if (!(d > depth_min && d < depth_max)) r.x = kNoDepth;
    rec_s[fy * P + fx] = r;
  }
  for (int i = tid; i < kWcEntries; i += kPfTile * kPfTile) wc_s[i] = wc[i];
  for (int i = tid; i < s * taps; i += kPfTile * kPfTile) ws_s[i] = ws[i];
  __syncthreads();

  int X, Y, unused;
  pf_tile_pixel(X, Y, unused);
  const int H = h * s, W = w * s;
  if (X >= W || Y >= H) return;
  const int cx = X / s, cy = Y / s;
  const int px = X - cx * s, py = Y - cy * s;
  const int64_t o = ((int64_t)view * H + Y) * W + X;
  const unsigned own = pack_rgb(guide + o * 3);
  const uint2* __restrict__ centre = rec_s + (cy - y_lo) * P + (cx - x_lo);
  const float* __restrict__ wsx = ws_s + px * taps + radius;     // indexed by tx in [-radius, radius]
  const float* __restrict__ wsy = ws_s + py * taps + radius;
  const uint2 c = centre[0];
  const float dc = __uint_as_float(c.x);
  if (dc != dc) {                                                // not valid: holes stay holes
    out[o] = 0.0f;
    if (COUNT) count[o] = 0;
    return;
  }
  // the anchor: the valid tap of the inner window with the largest weight, the containing pixel unless one is strictly larger
  float d0 = dc;
  float w_best = (wsy[0] * wsx[0]) * wc_s[colour_distance(c.y, own)];
  for (int ty = -anchor_radius; ty <= anchor_radius; ++ty) {
    const float wy = wsy[ty];
    for (int tx = -anchor_radius; tx <= anchor_radius; ++tx) {
      const uint2 r = centre[ty * P + tx];
      const float d = __uint_as_float(r.x);
      const float wt = (wy * wsx[tx]) * wc_s[colour_distance(r.y, own)];
      const bool better = d == d && wt > w_best;
      w_best = better ? wt : w_best;
      d0 = better ? d : d0;
    }
  }
  // the mean of the linked taps, as offsets from d0
  const float jump = rel_jump * d0;
  float wsum = 0.0f, ssum = 0.0f;
  int n = 0;
  for (int ty = -radius; ty <= radius; ++ty) {
    const float wy = wsy[ty];
    for (int tx = -radius; tx <= radius; ++tx) {
      const uint2 r = centre[ty * P + tx];
      const float d = __uint_as_float(r.x);
      const float diff = d - d0;
      const bool linked = fabsf(diff) <= jump;                   // false for a tap without depth: its diff is NaN
      const float wt = (wy * wsx[tx]) * wc_s[colour_distance(r.y, own)];
      wsum += linked ? wt : 0.0f;
      ssum += linked ? wt * diff : 0.0f;
      if (COUNT) n += linked ? 1 : 0;
    }
  }
  out[o] = wsum > 0.0f ? d0 + ssum / wsum : d0;
  if (COUNT) count[o] = n;
}

// the footprint's side for scale s and its LDS pitch (the file comment)
inline int refine_footprint(int s, int radius) { return (16 % s == 0 ? 16 / s : 16 / s + 2) + 2 * radius; }
inline int refine_pitch(int s, int F) { return s == 1 ? ((F + 15) / 32) * 32 + 16 : F; }

}  // namespace

extern "C" {

int pf_guide_pack_f32(const float* depth, const unsigned char* guide, int V, int h, int w, int s, void* records,
                      void* stream) {
  PF_REQUIRE(V >= 1 && V <= 65535 && h >= 0 && w >= 0 && s >= 1 && s <= 8);
  PF_REQUIRE((int64_t)h * s * w * s <= INT32_MAX / 4);
  if (h == 0 || w == 0) return PF_OK;
  PF_REQUIRE(depth && guide && records);
  hipLaunchKernelGGL(guide_pack_kernel, dim3((unsigned)pf_cdiv((int64_t)h * w, 256), (unsigned)V), dim3(256), 0,
                     (hipStream_t)stream, depth, guide, h, w, s, reinterpret_cast<uint2*>(records));
  return pf_launch_status();
}

int pf_depth_upsample_f32(const void* records, const unsigned char* guide, const float* ws, const float* wc, int V, int h,
                          int w, int s, int radius, int anchor_radius, float rel_jump, float depth_min, float depth_max,
                          float* out, int* count, void* stream) {
  PF_REQUIRE(V >= 1 && V <= 65535 && h >= 0 && w >= 0 && s >= 1 && s <= 8 && radius >= 0 && radius <= 8);
  PF_REQUIRE(anchor_radius >= 0 && anchor_radius <= radius && anchor_radius <= 2);
  PF_REQUIRE(rel_jump >= 0.0f && rel_jump <= 0.5f);
  PF_REQUIRE((int64_t)h * s * w * s <= INT32_MAX / 4 && pf_cdiv((int64_t)h * s, kPfTile) <= 65535);
  if (h == 0 || w == 0) return PF_OK;
  PF_REQUIRE(records && guide && ws && wc && out);
  const int F = refine_footprint(s, radius), P = refine_pitch(s, F);
  const size_t bytes = (size_t)F * P * 8 + (size_t)(kWcFloats + s * (2 * radius + 1)) * sizeof(float);
  const dim3 grid((unsigned)pf_cdiv((int64_t)w * s, kPfTile), (unsigned)pf_cdiv((int64_t)h * s, kPfTile), (unsigned)V);
  const uint2* rec = reinterpret_cast<const uint2*>(records);
  if (count)
    hipLaunchKernelGGL(depth_upsample_kernel<true>, grid, dim3(kPfTile * kPfTile), bytes, (hipStream_t)stream, rec, guide,
                       ws, wc, h, w, s, radius, anchor_radius, F, P, rel_jump, depth_min, depth_max, out, count);
  else
    hipLaunchKernelGGL(depth_upsample_kernel<false>, grid, dim3(kPfTile * kPfTile), bytes, (hipStream_t)stream, rec, guide,
                       ws, wc, h, w, s, radius, anchor_radius, F, P, rel_jump, depth_min, depth_max, out, count);
  return pf_launch_status();
}

}  // extern "C"
