// Normal maps of depth maps, and the normals of the disparity fuser's points (specification: pointmvsnet_amd/normals.py,
// include/pointflow_hip.h).  Pixel centres at (x + 0.5, y + 0.5) as in fusion.hip.
//
//   depth_normals  one thread per pixel of every view, 16 x 16 pixel tiles like Stage A of fusion.hip.  P(q) = (A (xq + .5,
//                  yq + .5, 1)) d(q), the world-axis vector from the camera centre to the surface point: the centre is NOT
//                  added, so the differences below cancel at the size of the depth.  A tangent per axis from the linked
//                  neighbours `step` pixels away (central, else one-sided), n = cross(tx, ty) / |cross|, turned to face the
//                  camera.  The view index is blockIdx.z, so the 9 floats of A are wave-uniform and are read by scalar loads
//                  into SGPRs; the vector loads are the pixel's own depth and its four neighbours.  No LDS: the four
//                  neighbour taps of a tile are the centre taps of the same or an adjacent tile, so they come from the
//                  caches, and the bytes that reach HBM are one 4-byte read and one 12-byte write per pixel either way
//                  (DESIGN.md section 9 has the count).  Vectors are kept as scalars: no scratch.
//   fuse_normals   one thread per pixel of every view, blockIdx.y the view: an EMITTING pixel of Stage B sums its own normal
//                  and those of its matches in ascending slot order and normalises; V - 1 coalesced reads of `match`, a
//                  12-byte gather per match.  Rows of pixels that do not emit are not written.
// No atomics in either: two runs give identical bytes.
#include "pf_camera.h"

namespace {

// (m[0..8] (px, py, 1)) d of a view row m: pf_apply_map without the camera centre
__device__ __forceinline__ void ray_point(const float* __restrict__ m, float px, float py, float d, float& X, float& Y,
                                          float& Z) {
  X = (m[0] * px + m[1] * py + m[2]) * d;
  Y = (m[3] * px + m[4] * py + m[5]) * d;
  Z = (m[6] * px + m[7] * py + m[8]) * d;
}

// The tangent along one axis at a pixel with P = (X, Y, Z): `fwd` / `bwd` say whether the neighbour ahead / behind is linked,
// (Xf ..) and (Xb ..) are their points (anything when not linked).  False when neither is.
__device__ __forceinline__ bool tangent(bool fwd, bool bwd, float X, float Y, float Z, float Xf, float Yf, float Zf, float Xb,
                                        float Yb, float Zb, float& tx, float& ty, float& tz) {
  const float ax = fwd ? Xf : X, ay = fwd ? Yf : Y, az = fwd ? Zf : Z;
  const float bx = bwd ? Xb : X, by = bwd ? Yb : Y, bz = bwd ? Zb : Z;
  tx = ax - bx;
  ty = ay - by;
  tz = az - bz;
  return fwd || bwd;
}

__global__ __launch_bounds__(kPfTile * kPfTile) void depth_normals_kernel(
    const float* __restrict__ depth, const float* __restrict__ view_maps, int h, int w, int step, float rel_jump,
    float depth_min, float depth_max, float* __restrict__ normal) {
  int x, y, i;
  pf_tile_pixel(x, y, i);
  if (x >= w || y >= h) return;
  const int hw = h * w;
  const int p = y * w + x;
  const float* __restrict__ plane = depth + (int64_t)i * hw;
  const float* __restrict__ m = view_maps + i * PF_FUSE_VIEW_FLOATS;
  const float d = plane[p];
  const bool valid = d > depth_min && d < depth_max;
  // inside the map, written so that no sum of `step` can overflow; an outside tap reads the pixel itself
  const bool in_r = step < w - x, in_l = step <= x, in_d = step < h - y, in_u = step <= y;
  const float dr = plane[in_r ? p + step : p];
  const float dl = plane[in_l ? p - step : p];
  const float dd = plane[in_d ? p + step * w : p];
  const float du = plane[in_u ? p - step * w : p];
  const float jump = rel_jump * d;
  const bool lr = valid && in_r && dr > depth_min && dr < depth_max && fabsf(dr - d) <= jump;
  const bool ll = valid && in_l && dl > depth_min && dl < depth_max && fabsf(dl - d) <= jump;
  const bool ld = valid && in_d && dd > depth_min && dd < depth_max && fabsf(dd - d) <= jump;
  const bool lu = valid && in_u && du > depth_min && du < depth_max && fabsf(du - d) <= jump;
  const float px = (float)x + 0.5f, py = (float)y + 0.5f, fs = (float)step;
  float X, Y, Z, Xr, Yr, Zr, Xl, Yl, Zl, Xd, Yd, Zd, Xu, Yu, Zu;
  ray_point(m, px, py, d, X, Y, Z);
  ray_point(m, px + fs, py, dr, Xr, Yr, Zr);
  ray_point(m, px - fs, py, dl, Xl, Yl, Zl);
  ray_point(m, px, py + fs, dd, Xd, Yd, Zd);
  ray_point(m, px, py - fs, du, Xu, Yu, Zu);
  float ax, ay, az, bx, by, bz;
  bool ok = tangent(lr, ll, X, Y, Z, Xr, Yr, Zr, Xl, Yl, Zl, ax, ay, az);
  ok = tangent(ld, lu, X, Y, Z, Xd, Yd, Zd, Xu, Yu, Zu, bx, by, bz) && ok;
  const float cx = ay * bz - az * by;
  const float cy = az * bx - ax * bz;
  const float cz = ax * by - ay * bx;
  const float len = sqrtf(cx * cx + cy * cy + cz * cz);
  float nx = cx / len, ny = cy / len, nz = cz / len;
  const float facing = nx * X + ny * Y + nz * Z;
  // 0 < len < inf is false for NaN; a facing of exactly 0 (or NaN) leaves the side undecided
  ok = ok && len > 0.0f && len < INFINITY && (facing > 0.0f || facing < 0.0f);
  if (facing > 0.0f) {
    nx = -nx;
    ny = -ny;
    nz = -nz;
  }
  const int64_t o = ((int64_t)i * hw + p) * 3;
  normal[o + 0] = ok ? nx : 0.0f;
  normal[o + 1] = ok ? ny : 0.0f;
  normal[o + 2] = ok ? nz : 0.0f;
}

__global__ __launch_bounds__(256) void fuse_normals_kernel(const float* __restrict__ normal, const int* __restrict__ match,
                                                           const unsigned char* __restrict__ emit, int V, int hw,
                                                           float* __restrict__ out) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  const int view = blockIdx.y;
  if (p >= hw) return;
  const int64_t ip = (int64_t)view * hw + p;
  if (emit[ip] == 0) return;
  float sx = normal[ip * 3 + 0], sy = normal[ip * 3 + 1], sz = normal[ip * 3 + 2];
  for (int slot = 0; slot < V - 1; ++slot) {
    const int q = match[((int64_t)view * (V - 1) + slot) * hw + p];
    const int j = slot < view ? slot : slot + 1;         // the slot -> view map of fuse_mark_kernel
    if (q >= 0 && q < hw) {
      const int64_t jq = ((int64_t)j * hw + q) * 3;
      sx += normal[jq + 0];
      sy += normal[jq + 1];
      sz += normal[jq + 2];
    }
  }
  const float len = sqrtf(sx * sx + sy * sy + sz * sz);
  const bool ok = len > 0.0f && len < INFINITY;
  out[ip * 3 + 0] = ok ? sx / len : 0.0f;
  out[ip * 3 + 1] = ok ? sy / len : 0.0f;
  out[ip * 3 + 2] = ok ? sz / len : 0.0f;
}

}  // namespace

extern "C" {

int pf_depth_normals_f32(const float* depth, const float* view_maps, int V, int h, int w, int step, float rel_jump,
                         float depth_min, float depth_max, float* normal, void* stream) {
  PF_REQUIRE(V >= 1 && h >= 0 && w >= 0 && step >= 1 && (int64_t)h * w <= INT32_MAX / 4);
  PF_REQUIRE((pf_cdiv(h, kPfTile) <= 65535) && V <= 65535);
  if (h == 0 || w == 0) return PF_OK;
  PF_REQUIRE(depth && view_maps && normal);
  hipLaunchKernelGGL(depth_normals_kernel, dim3((unsigned)pf_cdiv(w, kPfTile), (unsigned)pf_cdiv(h, kPfTile), (unsigned)V),
                     dim3(kPfTile * kPfTile), 0, (hipStream_t)stream, depth, view_maps, h, w, step, rel_jump, depth_min,
                     depth_max, normal);
  return pf_launch_status();
}

int pf_fuse_normals_f32(const float* normal_maps, const int* match, const unsigned char* emit, int V, int h, int w,
                        float* out, void* stream) {
  PF_REQUIRE(V >= 1 && V <= 65535 && h >= 0 && w >= 0 && (int64_t)h * w <= INT32_MAX / 4);
  if (h == 0 || w == 0) return PF_OK;
  PF_REQUIRE(normal_maps && emit && out && (match || V == 1));
  hipLaunchKernelGGL(fuse_normals_kernel, dim3((unsigned)pf_cdiv((int64_t)h * w, 256), (unsigned)V), dim3(256), 0,
                     (hipStream_t)stream, normal_maps, match, emit, V, h * w, out);
  return pf_launch_status();
}

}  // extern "C"
