// Rasterising a triangle mesh into the depth maps of V views: the z-buffer of cloud_render.hip with a face for a point
// (specification: pointmvsnet_amd/render.py "Mesh rasterisation", include/pointflow_hip.h).  Pixel
// centres at (x + 0.5, y + 0.5); screen positions are snapped to 1/256 pixel, after which coverage is exact int64.
//
//   mr_vertex       THE projection of a vertex into a view: (xi, yi, z, valid).  Every kernel below calls it, so the table
//                   that mesh_screen writes, the rasteriser and the barycentric pass agree to the bit.
//   mesh_screen     one thread per vertex, the views are its loop (scalar loads of proj): writes the table.  For tests and
//                   inspection only -- the rasteriser re-projects: at 49 views and 1.5 M vertices the table would be 0.9 GB
//                   written and then gathered three times per face, where re-projecting costs a few GFLOP.
//   mesh_raster     one thread per face, 256 per block.  The thread loads its three indices and nine floats once and walks
//                   ALL V views; the view is the loop counter, so a view's 12 floats are wave-uniform scalar loads (the
//                   reasoning at the head of cloud_render.hip).  Per view: project the three vertices, orient, set up the
//                   three edge functions at the first pixel centre of the bounding box clamped to the map, and step them
//                   by int64 additions.  A covered pixel takes the 64-bit unsigned minimum of (float_bits(z) << 32 | face),
//                   after a plain peek of the cell as in the splat (the cell only ever decreases).
//                   A list-walking kernel lasts as long as its longest list (README, round 6), and a two-triangle plane
//                   covers the whole map.  So a face whose clamped bounding box holds at most S = lane_pixels pixels is
//                   walked by its own lane; the others are collected per view with __ballot and walked by the whole wave,
//                   64 pixels per step (the lanes side by side along the box's longer side, stepping along the shorter), the
//                   owner's set-up broadcast with __shfl -- the hub-row scheme of the EdgeConv backward (edgeconv.hip).
//                   Lanes past Nf and lanes whose face is skipped stay in the view loop with a flag: they take part in the
//                   ballots.  The minimum is order-free, so the result cannot depend on S.
//   mesh_bary       one thread per pixel: recomputes its winner's set-up through mr_vertex / mr_setup and writes the
//                   perspective-correct weights in the face's stored vertex order.
//
// S = PF_MESH_LANE_PIXELS = 64.  MEASURED on an MI355X (tools/microbench_mesh_render.py, profiles/mesh_render_microbench.jsonl;
// 49 views of 640 x 480, medians of 5): the raster kernel at S = 16 / 32 / 64 / 128 took 0.941 / 0.931 / 0.914 / 0.912 ms on
// the TSDF mesh at voxel 1.0 (717 080 faces), 1.572 / 1.533 / 1.531 / 1.535 ms at voxel 0.5 (2 976 664 faces) and 97.9 / 97.2 /
// 97.8 / 97.8 ms on a two-triangle plane that fills every view.  16 is the slowest on both meshes by 3 %; 32, 64 and 128 lie
// within 2 % of each other, which is the spread between two runs of one value, so nothing separates them and 64, the
// width of a wave, stays.  (Faces of a TSDF mesh cover a pixel or two; only the plane takes the shared path.)
// The shared path is one wave per face and view, and each of its steps waits for its peek: 98 ms for 98 face-views of
// 307 200 pixels is 0.2 us per step of 64 pixels.  Spreading such a face over more waves than its own is not built.
// No LDS, no scratch (no array is indexed at run time); every cell address lies in the clamped bounding box, every face
// row is < Nf and every vertex row is checked against Nv before it is read, whatever the matrices and indices hold.
#include "pf_camera.h"

#include <math.h>

// (see cloud_render.hip: the host re-compilation of tests/hipemu has no 64-bit atomicMin)
#if defined(__HIP__)
#define PF_MR_PEEK(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define PF_MR_MIN(p, key) atomicMin((p), (key))
#else
#define PF_MR_PEEK(p) __atomic_load_n((p), __ATOMIC_RELAXED)
#define PF_MR_MIN(p, key) __atomic_fetch_min((p), (key), __ATOMIC_RELAXED)
#endif

namespace {

typedef long long mr_i64;

struct MrVertex {
  int x, y;      // 24.8 fixed point, 0 unless ok
  float z;
  bool ok;
};

// qx, qy, z as step 1 of the splat; valid iff depth_min < z < depth_max and -G <= u < w + G, -G <= v < h + G, compared as
// floats before any conversion (false for NaN, and then |u * 256| <= 2^23: the conversion is in range)
__device__ __forceinline__ MrVertex mr_vertex(const float* __restrict__ p, float X, float Y, float Z, float ulim, float vlim,
                                              float depth_min, float depth_max) {
  const float G = (float)PF_MESH_GUARD_BAND;
  const float qx = ((p[0] * X + p[1] * Y) + p[2] * Z) + p[3];
  const float qy = ((p[4] * X + p[5] * Y) + p[6] * Z) + p[7];
  const float z = ((p[8] * X + p[9] * Y) + p[10] * Z) + p[11];
  const float u = qx / z, v = qy / z;
  MrVertex r;
  r.z = z;
  r.ok = z > depth_min && z < depth_max && u >= -G && u < ulim && v >= -G && v < vlim;
  r.x = r.ok ? (int)rintf(u * 256.0f) : 0;
  r.y = r.ok ? (int)rintf(v * 256.0f) : 0;
  return r;
}

// A face in a view, oriented so that area2 > 0.  e* are the edge functions opposite a, b, c (of the ORIENTED triangle) at
// the centre of pixel (x0, y0); a step of one pixel in x adds -256 dy*, in y +256 dx*.  b* is 0 where the edge owns its
// boundary and 1 where it does not: the pixel is covered iff e - b >= 0 for all three.
struct MrFace {
  mr_i64 ea, eb, ec;
  int dxa, dya, dxb, dyb, dxc, dyc;
  int ba, bb, bc;
  int x0, y0, bw, npix;
  float ra, rb, rc, area2f;
  bool swapped;
};

__device__ __forceinline__ int mr_min3(int a, int b, int c) { return min(a, min(b, c)); }
__device__ __forceinline__ int mr_max3(int a, int b, int c) { return max(a, max(b, c)); }
__device__ __forceinline__ int mr_bias(int dx, int dy) { return (dy > 0 || (dy == 0 && dx < 0)) ? 0 : 1; }

// false: the face writes nothing in this view (a vertex not valid, zero area, culled, or no pixel centre in its box)
__device__ __forceinline__ bool mr_setup(MrVertex a, MrVertex b, MrVertex c, int cull, int h, int w, MrFace& F) {
  if (!(a.ok && b.ok && c.ok)) return false;
  mr_i64 area2 = (mr_i64)(b.x - a.x) * (c.y - a.y) - (mr_i64)(b.y - a.y) * (c.x - a.x);
  if (area2 == 0) return false;
  const bool front = area2 < 0;
  if ((cull == PF_MESH_CULL_BACK && !front) || (cull == PF_MESH_CULL_FRONT && front)) return false;
  if (front) {
    const MrVertex t = b;
    b = c;
    c = t;
    area2 = -area2;
  }
  // pixel x is a candidate iff its centre 256 x + 128 lies in [min, max]: x >= ceil((min - 128) / 256), x <= floor(..)
  const int x0 = max((mr_min3(a.x, b.x, c.x) + 127) >> 8, 0), x1 = min((mr_max3(a.x, b.x, c.x) - 128) >> 8, w - 1);
  const int y0 = max((mr_min3(a.y, b.y, c.y) + 127) >> 8, 0), y1 = min((mr_max3(a.y, b.y, c.y) - 128) >> 8, h - 1);
  if (x0 > x1 || y0 > y1) return false;
  const int sx = 256 * x0 + 128, sy = 256 * y0 + 128;
  F.dxa = c.x - b.x, F.dya = c.y - b.y;                                    // opposite a: the edge b -> c
  F.dxb = a.x - c.x, F.dyb = a.y - c.y;                                    // opposite b: c -> a
  F.dxc = b.x - a.x, F.dyc = b.y - a.y;                                    // opposite c: a -> b
  F.ea = (mr_i64)F.dxa * (sy - b.y) - (mr_i64)F.dya * (sx - b.x);
  F.eb = (mr_i64)F.dxb * (sy - c.y) - (mr_i64)F.dyb * (sx - c.x);
  F.ec = (mr_i64)F.dxc * (sy - a.y) - (mr_i64)F.dyc * (sx - a.x);
  F.ba = mr_bias(F.dxa, F.dya), F.bb = mr_bias(F.dxb, F.dyb), F.bc = mr_bias(F.dxc, F.dyc);
  F.x0 = x0, F.y0 = y0, F.bw = x1 - x0 + 1, F.npix = F.bw * (y1 - y0 + 1);   // <= 2^28
  F.ra = 1.0f / a.z, F.rb = 1.0f / b.z, F.rc = 1.0f / c.z;
  F.area2f = (float)area2;
  F.swapped = front;
  return true;
}

__device__ __forceinline__ bool mr_covered(mr_i64 ea, mr_i64 eb, mr_i64 ec, int ba, int bb, int bc) {
  return ((ea - ba) | (eb - bb) | (ec - bc)) >= 0;
}

__device__ __forceinline__ float mr_inv(mr_i64 ea, mr_i64 eb, mr_i64 ec, float ra, float rb, float rc) {
  return ((float)ea * ra + (float)eb * rb) + (float)ec * rc;
}

__device__ __forceinline__ void mr_shade(mr_i64 ea, mr_i64 eb, mr_i64 ec, float ra, float rb, float rc, float area2f,
                                         unsigned face, unsigned long long* cell) {
  const float z = area2f / mr_inv(ea, eb, ec, ra, rb, rc);
  const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | (unsigned long long)face;
  if (key < PF_MR_PEEK(cell)) PF_MR_MIN(cell, key);
}

__global__ __launch_bounds__(256) void mesh_screen_kernel(const float* __restrict__ vertices, int64_t Nv,
                                                          const float* __restrict__ proj, int V, int h, int w,
                                                          float depth_min, float depth_max, int* __restrict__ xy,
                                                          float* __restrict__ zs, unsigned char* __restrict__ valid) {
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (n >= Nv) return;
  const float X = vertices[n * 3 + 0], Y = vertices[n * 3 + 1], Z = vertices[n * 3 + 2];
  const float ulim = (float)(w + PF_MESH_GUARD_BAND), vlim = (float)(h + PF_MESH_GUARD_BAND);
  for (int view = 0; view < V; ++view) {
    const MrVertex r = mr_vertex(proj + (int64_t)view * PF_RENDER_PROJ_FLOATS, X, Y, Z, ulim, vlim, depth_min, depth_max);
    const int64_t o = (int64_t)view * Nv + n;
    xy[o * 2 + 0] = r.x;
    xy[o * 2 + 1] = r.y;
    zs[o] = r.z;
    valid[o] = r.ok ? 1 : 0;
  }
}

__global__ __launch_bounds__(256) void mesh_raster_kernel(const float* __restrict__ vertices, int64_t Nv,
                                                          const int* __restrict__ faces, int64_t Nf,
                                                          const float* __restrict__ proj, int V, int h, int w,
                                                          float depth_min, float depth_max, int cull, int lane_pixels,
                                                          unsigned long long* zbuf) {
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  // no early return: every lane of the wave takes part in the ballots of the view loop
  bool alive = f < Nf;
  float ax = 0.f, ay = 0.f, az = 0.f, bx = 0.f, by = 0.f, bz = 0.f, cx = 0.f, cy = 0.f, cz = 0.f;
  if (alive) {
    const int ia = faces[f * 3 + 0], ib = faces[f * 3 + 1], ic = faces[f * 3 + 2];
    alive = ia >= 0 && ia < Nv && ib >= 0 && ib < Nv && ic >= 0 && ic < Nv;     // another index is never read through
    if (alive) {
      ax = vertices[(int64_t)ia * 3 + 0], ay = vertices[(int64_t)ia * 3 + 1], az = vertices[(int64_t)ia * 3 + 2];
      bx = vertices[(int64_t)ib * 3 + 0], by = vertices[(int64_t)ib * 3 + 1], bz = vertices[(int64_t)ib * 3 + 2];
      cx = vertices[(int64_t)ic * 3 + 0], cy = vertices[(int64_t)ic * 3 + 1], cz = vertices[(int64_t)ic * 3 + 2];
    }
  }
  const float ulim = (float)(w + PF_MESH_GUARD_BAND), vlim = (float)(h + PF_MESH_GUARD_BAND);
  const int64_t hw = (int64_t)h * w;
  const unsigned face = (unsigned)f;
  for (int view = 0; view < V; ++view) {
    const float* __restrict__ p = proj + (int64_t)view * PF_RENDER_PROJ_FLOATS;      // wave-uniform: scalar loads
    unsigned long long* plane = zbuf + (int64_t)view * hw;
    MrFace F = {};
    bool live = false;
    if (alive)
      live = mr_setup(mr_vertex(p, ax, ay, az, ulim, vlim, depth_min, depth_max),
                      mr_vertex(p, bx, by, bz, ulim, vlim, depth_min, depth_max),
                      mr_vertex(p, cx, cy, cz, ulim, vlim, depth_min, depth_max), cull, h, w, F);
    const bool shared = live && F.npix > lane_pixels;
    if (live && !shared) {                                                           // the lane's own walk: <= S pixels
      const mr_i64 stxa = -256 * (mr_i64)F.dya, stxb = -256 * (mr_i64)F.dyb, stxc = -256 * (mr_i64)F.dyc;
      const mr_i64 stya = 256 * (mr_i64)F.dxa, styb = 256 * (mr_i64)F.dxb, styc = 256 * (mr_i64)F.dxc;
      const int rows = F.npix / F.bw;
      mr_i64 rowa = F.ea, rowb = F.eb, rowc = F.ec;
      for (int y = 0; y < rows; ++y) {
        mr_i64 ea = rowa, eb = rowb, ec = rowc;
        unsigned long long* cell = plane + ((int64_t)(F.y0 + y) * w + F.x0);
        for (int x = 0; x < F.bw; ++x) {
          if (mr_covered(ea, eb, ec, F.ba, F.bb, F.bc)) mr_shade(ea, eb, ec, F.ra, F.rb, F.rc, F.area2f, face, cell + x);
          ea += stxa, eb += stxb, ec += stxc;
        }
        rowa += stya, rowb += styb, rowc += styc;
      }
    }
    unsigned long long todo = __ballot(shared);
    while (todo != 0ull) {                                                           // wave-uniform: the ballot's value
      const int o = __ffsll((long long)todo) - 1;
      todo &= todo - 1ull;
      const mr_i64 ea0 = __shfl(F.ea, o), eb0 = __shfl(F.eb, o), ec0 = __shfl(F.ec, o);
      const mr_i64 stxa = -256 * (mr_i64)__shfl(F.dya, o), stxb = -256 * (mr_i64)__shfl(F.dyb, o),
                   stxc = -256 * (mr_i64)__shfl(F.dyc, o);
      const mr_i64 stya = 256 * (mr_i64)__shfl(F.dxa, o), styb = 256 * (mr_i64)__shfl(F.dxb, o),
                   styc = 256 * (mr_i64)__shfl(F.dxc, o);
      const int bias = __shfl(F.ba | (F.bb << 1) | (F.bc << 2), o);
      const int ba = bias & 1, bb = (bias >> 1) & 1, bc = (bias >> 2) & 1;
      const int ox0 = __shfl(F.x0, o), oy0 = __shfl(F.y0, o), obw = __shfl(F.bw, o), onpix = __shfl(F.npix, o);
      const float ra = __shfl(F.ra, o), rb = __shfl(F.rb, o), rc = __shfl(F.rc, o), area2f = __shfl(F.area2f, o);
      const unsigned oface = (unsigned)__shfl((int)face, o);
      // Lanes lie along the box's longer side (along x they touch neighbouring cells) and step along the shorter one by
      // int64 additions: no division and no 64-bit product per pixel (measured on the two-triangle plane: 137 ms with
      // pixel = lane + 64 step and a division per pixel, 98 ms this way).
      const int obh = onpix / obw;
      const bool along_x = obw >= obh;
      const int n_major = along_x ? obw : obh, n_minor = along_x ? obh : obw;
      const mr_i64 mja = along_x ? stxa : stya, mjb = along_x ? stxb : styb, mjc = along_x ? stxc : styc;
      const mr_i64 mna = along_x ? stya : stxa, mnb = along_x ? styb : stxb, mnc = along_x ? styc : stxc;
      const int64_t cell_major = along_x ? 1 : w, cell_minor = along_x ? w : 1;
      unsigned long long* first = plane + ((int64_t)oy0 * w + ox0);
      for (int m = lane; m < n_major; m += 64) {
        mr_i64 ea = ea0 + m * mja, eb = eb0 + m * mjb, ec = ec0 + m * mjc;
        unsigned long long* cell = first + m * cell_major;
        for (int j = 0; j < n_minor; ++j) {
          if (mr_covered(ea, eb, ec, ba, bb, bc)) mr_shade(ea, eb, ec, ra, rb, rc, area2f, oface, cell);
          ea += mna, eb += mnb, ec += mnc;
          cell += cell_minor;
        }
      }
    }
  }
}

__global__ __launch_bounds__(256) void mesh_bary_kernel(const float* __restrict__ vertices, int64_t Nv,
                                                        const int* __restrict__ faces, int64_t Nf,
                                                        const float* __restrict__ proj, int h, int w, int64_t cells,
                                                        float depth_min, float depth_max, const int* __restrict__ index,
                                                        float* __restrict__ bary) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= cells) return;
  float wa = 0.f, wb = 0.f, wc = 0.f;
  const int raw = index[i];
  const int64_t f = (int64_t)(unsigned)raw;                                          // rows past 2^31 - 1 are bit patterns
  if (raw != -1 && f < Nf) {
    const int ia = faces[f * 3 + 0], ib = faces[f * 3 + 1], ic = faces[f * 3 + 2];
    if (ia >= 0 && ia < Nv && ib >= 0 && ib < Nv && ic >= 0 && ic < Nv) {
      const int64_t hw = (int64_t)h * w;
      const int view = (int)(i / hw);
      const int rem = (int)(i - view * hw), y = rem / w, x = rem - y * w;
      const float* __restrict__ p = proj + (int64_t)view * PF_RENDER_PROJ_FLOATS;
      const float ulim = (float)(w + PF_MESH_GUARD_BAND), vlim = (float)(h + PF_MESH_GUARD_BAND);
      const float* va = vertices + (int64_t)ia * 3;
      const float* vb = vertices + (int64_t)ib * 3;
      const float* vc = vertices + (int64_t)ic * 3;
      MrFace F = {};
      if (mr_setup(mr_vertex(p, va[0], va[1], va[2], ulim, vlim, depth_min, depth_max),
                   mr_vertex(p, vb[0], vb[1], vb[2], ulim, vlim, depth_min, depth_max),
                   mr_vertex(p, vc[0], vc[1], vc[2], ulim, vlim, depth_min, depth_max), PF_MESH_CULL_NONE, h, w, F)) {
        const int px = x - F.x0, py = y - F.y0;
        const mr_i64 ea = F.ea - 256 * (mr_i64)F.dya * px + 256 * (mr_i64)F.dxa * py;
        const mr_i64 eb = F.eb - 256 * (mr_i64)F.dyb * px + 256 * (mr_i64)F.dxb * py;
        const mr_i64 ec = F.ec - 256 * (mr_i64)F.dyc * px + 256 * (mr_i64)F.dxc * py;
        if (mr_covered(ea, eb, ec, F.ba, F.bb, F.bc)) {                              // a winner always is
          const float inv = mr_inv(ea, eb, ec, F.ra, F.rb, F.rc);
          const float t0 = (float)ea * F.ra / inv, t1 = (float)eb * F.rb / inv, t2 = (float)ec * F.rc / inv;
          wa = t0, wb = F.swapped ? t2 : t1, wc = F.swapped ? t1 : t2;              // back to the stored order
        }
      }
    }
  }
  bary[i * 3 + 0] = wa;
  bary[i * 3 + 1] = wb;
  bary[i * 3 + 2] = wc;
}

inline bool mr_maps_ok(int V, int h, int w) {
  return V >= 0 && V <= 65535 && h >= 0 && w >= 0 && h <= PF_MESH_MAX_SIDE && w <= PF_MESH_MAX_SIDE &&
         (int64_t)h * w <= INT32_MAX / 4;
}

}  // namespace

extern "C" {

int pf_mesh_screen_f32(const float* vertices, int64_t Nv, const float* proj, int V, int h, int w, float depth_min,
                       float depth_max, int* xy, float* z, unsigned char* valid, void* stream) {
  PF_REQUIRE(Nv >= 0 && Nv <= INT32_MAX && mr_maps_ok(V, h, w));
  if (Nv == 0 || V == 0) return PF_OK;
  PF_REQUIRE(vertices && proj && xy && z && valid);
  hipLaunchKernelGGL(mesh_screen_kernel, dim3((unsigned)pf_cdiv(Nv, 256)), dim3(256), 0, (hipStream_t)stream, vertices, Nv,
                     proj, V, h, w, depth_min, depth_max, xy, z, valid);
  return pf_launch_status();
}

int pf_mesh_raster_tuned_f32(const float* vertices, int64_t Nv, const int* faces, int64_t Nf, const float* proj, int V, int h,
                             int w, float depth_min, float depth_max, int cull, int lane_pixels, uint64_t* zbuf,
                             void* stream) {
  PF_REQUIRE(Nv >= 0 && Nv <= INT32_MAX && Nf >= 0 && Nf <= PF_MESH_MAX_FACES && mr_maps_ok(V, h, w) && lane_pixels >= 0 &&
             (cull == PF_MESH_CULL_NONE || cull == PF_MESH_CULL_BACK || cull == PF_MESH_CULL_FRONT));
  if (Nv == 0 || Nf == 0 || V == 0 || h == 0 || w == 0) return PF_OK;
  PF_REQUIRE(vertices && faces && proj && zbuf);
  hipLaunchKernelGGL(mesh_raster_kernel, dim3((unsigned)pf_cdiv(Nf, 256)), dim3(256), 0, (hipStream_t)stream, vertices, Nv,
                     faces, Nf, proj, V, h, w, depth_min, depth_max, cull, lane_pixels,
                     reinterpret_cast<unsigned long long*>(zbuf));
  return pf_launch_status();
}

int pf_mesh_raster_f32(const float* vertices, int64_t Nv, const int* faces, int64_t Nf, const float* proj, int V, int h,
                       int w, float depth_min, float depth_max, int cull, uint64_t* zbuf, void* stream) {
  return pf_mesh_raster_tuned_f32(vertices, Nv, faces, Nf, proj, V, h, w, depth_min, depth_max, cull, PF_MESH_LANE_PIXELS,
                                  zbuf, stream);
}

int pf_mesh_bary_f32(const float* vertices, int64_t Nv, const int* faces, int64_t Nf, const float* proj, int V, int h, int w,
                     float depth_min, float depth_max, const int* index, float* bary, void* stream) {
  PF_REQUIRE(Nv >= 0 && Nv <= INT32_MAX && Nf >= 0 && Nf <= PF_MESH_MAX_FACES && mr_maps_ok(V, h, w));
  const int64_t cells = (int64_t)V * h * w;
  if (cells == 0) return PF_OK;
  PF_REQUIRE(index && bary && pf_cdiv(cells, 256) <= INT32_MAX && (Nf == 0 || (vertices && faces && proj)));
  hipLaunchKernelGGL(mesh_bary_kernel, dim3((unsigned)pf_cdiv(cells, 256)), dim3(256), 0, (hipStream_t)stream, vertices, Nv,
                     faces, Nf, proj, h, w, cells, depth_min, depth_max, index, bary);
  return pf_launch_status();
}

}  // extern "C"
