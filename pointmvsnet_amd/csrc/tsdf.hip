// Meshing a scan: volumetric fusion of depth maps into a truncated signed distance field and the extraction of its zero
// surface by marching tetrahedra (specification: pointmvsnet_amd/tsdf.py, include/pointflow_hip.h).  Samples are indexed
// [k][j][i], x fastest; sample (i, j, k) sits at o + float(i) * voxel per coordinate.  Pixel centres at (x + 0.5, y + 0.5)
// as in pf_camera.h, so the pixel that contains a projection (u, v) is (floor(u), floor(v)).
//
//   tsdf_integrate  one thread per sample, 256 per block, x fastest: the 64 samples of a wave are a run along x (a run may
//                   wrap into the next row), which projects to a short segment of every view, so a wave's depth gathers of
//                   one view fall into few cache lines.  The thread keeps its sample's sums in registers and walks ALL V
//                   views in ascending order: the view is the loop counter, so the 12 floats of K [R | t] are wave-uniform
//                   and arrive by scalar loads.  A sample is owned by one thread: no atomics, the float32 sum has one
//                   order, and a call that continues earlier sums adds exactly what one call over all views would have.
//                   Every comparison that guards an address is made on floats BEFORE the conversion to int (false for
//                   NaN), so every conversion is in range and every gather inside its map, whatever the matrices hold.
//   tsdf_count      one thread per cell: 0 unless all 8 corners carry min_weight; else the triangles of its six tetrahedra
//                   (1 for a 1-3 split, 2 for a 2-2 split).
//   tsdf_emit       one thread per cell, the same walk: three 64-bit edge keys per triangle, written at the cell's offset
//                   (the inclusive prefix sum of the counts, made by the caller).  The winding is decided per triangle in
//                   integer arithmetic from the corners alone (twice the edge midpoints in index space), so it is a
//                   function of (tetrahedron, case) and nothing else.
//   tsdf_vertices   one thread per unique key: the vertex from the key alone, so every cell that refers to it sees one value.
//
// The update of a sample by a view, the tetrahedron ring, the triangles of a cell, the edge keys and the vertex arithmetic are
// those of pf_tsdf.h, shared with the sparse volume (sparse_tsdf.hip).  No table in memory, no per-thread array, no scratch, no
// LDS.
#include "pf_common.h"
#include "pf_tsdf.h"

#include <math.h>

namespace {

__global__ __launch_bounds__(256) void tsdf_integrate_kernel(const float* __restrict__ depths,
                                                             const unsigned char* __restrict__ images,
                                                             const float* __restrict__ proj, int V, int h, int w, float ox,
                                                             float oy, float oz, float voxel, int nx, int ny, int total,
                                                             float trunc, float depth_min, float depth_max,
                                                             float* __restrict__ S, int* __restrict__ W,
                                                             int* __restrict__ CS, int* __restrict__ CW) {
  const int64_t n64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (n64 >= total) return;
  const int n = (int)n64;
  const int i = n % nx, jk = n / nx;
  const int j = jk % ny, k = jk / ny;
  const float X = ox + (float)i * voxel, Y = oy + (float)j * voxel, Z = oz + (float)k * voxel;
  const float wf = (float)w, hf = (float)h;
  const int64_t hw = (int64_t)h * w;
  TsdfSums a = {S[n], W[n], 0, 0, 0, 0};
  if (images != nullptr) {
    a.cr = CS[(int64_t)n * 3 + 0];
    a.cg = CS[(int64_t)n * 3 + 1];
    a.cb = CS[(int64_t)n * 3 + 2];
    a.cw = CW[n];
  }
  for (int view = 0; view < V; ++view) {
    const float* __restrict__ p = proj + (int64_t)view * PF_RENDER_PROJ_FLOATS;      // wave-uniform: scalar loads
    tsdf_integrate_view(p, depths, images, view, hw, w, wf, hf, X, Y, Z, trunc, depth_min, depth_max, a);
  }
  S[n] = a.s;
  W[n] = a.cnt;
  if (images != nullptr) {
    CS[(int64_t)n * 3 + 0] = a.cr;
    CS[(int64_t)n * 3 + 1] = a.cg;
    CS[(int64_t)n * 3 + 2] = a.cb;
    CW[n] = a.cw;
  }
}

// ---- marching tetrahedra ------------------------------------------------------------------------------------------
// bit c of the result: corner c = dx + 2 dy + 4 dz of the cell is inside (tsdf < 0; false for NaN); -1 if the cell is not
// active (a corner with weight < min_weight).  `base` is the linear index of corner 0.
__device__ __forceinline__ int tsdf_cell_mask(const float* __restrict__ tsdf, const int* __restrict__ weight, int base, int nx,
                                              int nxy, int min_weight) {
  int mask = 0;
  bool active = true;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int at = base + (c & 1) + ((c >> 1) & 1) * nx + (c >> 2) * nxy;
    active = active && weight[at] >= min_weight;
    mask |= (tsdf[at] < 0.0f ? 1 : 0) << c;
  }
  return active ? mask : -1;
}

// the linear sample index of corner 0 of cell (k (ny - 1) + j) (nx - 1) + i
__device__ __forceinline__ int tsdf_cell_base(int cell, int nx, int ny) {
  const int cx = nx - 1, cy = ny - 1;
  const int i = cell % cx, jk = cell / cx;
  const int j = jk % cy, k = jk / cy;
  return (k * ny + j) * nx + i;
}

__global__ __launch_bounds__(256) void tsdf_count_kernel(const float* __restrict__ tsdf, const int* __restrict__ weight, int nx,
                                                         int ny, int cells, int min_weight, int* __restrict__ count) {
  const int64_t c64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c64 >= cells) return;
  const int base = tsdf_cell_base((int)c64, nx, ny);
  const int mask = tsdf_cell_mask(tsdf, weight, base, nx, nx * ny, min_weight);
  count[c64] = tsdf_cell_triangles(mask);
}

__global__ __launch_bounds__(256) void tsdf_emit_kernel(const float* __restrict__ tsdf, const int* __restrict__ weight, int nx,
                                                        int ny, int cells, int min_weight, const int64_t* __restrict__ incl,
                                                        int64_t faces, int64_t* __restrict__ keys) {
  const int64_t c64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c64 >= cells) return;
  const int nxy = nx * ny;
  const int base = tsdf_cell_base((int)c64, nx, ny);
  const int mask = tsdf_cell_mask(tsdf, weight, base, nx, nxy, min_weight);
  if (!(mask > 0 && mask < 255)) return;
  tsdf_emit_cell<int>(mask, base, nx, nxy, c64 ? incl[c64 - 1] : 0, faces, keys);
}

__global__ __launch_bounds__(256) void tsdf_vertices_kernel(const int64_t* __restrict__ keys, int64_t count,
                                                            const float* __restrict__ tsdf,
                                                            const unsigned char* __restrict__ colour, float ox, float oy,
                                                            float oz, float voxel, int nx, int ny, int nz,
                                                            float* __restrict__ vertices, unsigned char* __restrict__ colours) {
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (n >= count) return;
  const int64_t key = keys[n];
  const int dir = (int)(key & 7);
  const int64_t a64 = key >> 3;
  const int64_t total = (int64_t)nx * ny * nz;
  bool edge = false;
  int r = 0, g = 0, b = 0;
  if (a64 >= 0 && a64 < total) {
    const int a = (int)a64;
    const int i = a % nx, jk = a / nx;
    const int j = jk % ny, k = jk / ny;
    const int dx = dir & 1, dy = (dir >> 1) & 1, dz = dir >> 2;
    if (dir != 0 && i + dx < nx && j + dy < ny && k + dz < nz) {       // a key that is not this volume's reads nothing
      edge = true;
      const int bb = a + dx + dy * nx + dz * nx * ny;
      const float t = tsdf_vertex(tsdf[a], tsdf[bb], i, j, k, dx, dy, dz, ox, oy, oz, voxel, vertices + n * 3);
      if (colour != nullptr) {
        const unsigned char* ca = colour + (int64_t)a * 3;
        const unsigned char* cb = colour + (int64_t)bb * 3;
        r = tsdf_vertex_colour(ca[0], cb[0], t);
        g = tsdf_vertex_colour(ca[1], cb[1], t);
        b = tsdf_vertex_colour(ca[2], cb[2], t);
      }
    }
  }
  if (!edge) vertices[n * 3 + 0] = vertices[n * 3 + 1] = vertices[n * 3 + 2] = 0.0f;
  if (colours != nullptr) {
    colours[n * 3 + 0] = (unsigned char)r;
    colours[n * 3 + 1] = (unsigned char)g;
    colours[n * 3 + 2] = (unsigned char)b;
  }
}

inline bool tsdf_dims_ok(int nx, int ny, int nz) {
  return nx >= 1 && ny >= 1 && nz >= 1 && (int64_t)nx * ny * nz <= PF_TSDF_MAX_SAMPLES;
}

inline int tsdf_cells(int nx, int ny, int nz) { return (nx - 1) * (ny - 1) * (nz - 1); }

}  // namespace

extern "C" {

int pf_tsdf_integrate_f32(const float* depths, const unsigned char* images, const float* proj, int V, int h, int w, float ox,
                          float oy, float oz, float voxel, int nx, int ny, int nz, float trunc, float depth_min,
                          float depth_max, float* S, int* W, int* CS, int* CW, void* stream) {
  PF_REQUIRE(tsdf_dims_ok(nx, ny, nz) && V >= 0 && h >= 0 && w >= 0 && (int64_t)h * w <= INT32_MAX / 4);
  PF_REQUIRE(voxel > 0.0f && trunc > 0.0f);
  if (V == 0 || h == 0 || w == 0) return PF_OK;
  PF_REQUIRE(depths && proj && S && W && (images == nullptr || (CS && CW)));
  const int total = nx * ny * nz;
  hipLaunchKernelGGL(tsdf_integrate_kernel, dim3((unsigned)pf_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, depths,
                     images, proj, V, h, w, ox, oy, oz, voxel, nx, ny, total, trunc, depth_min, depth_max, S, W, CS, CW);
  return pf_launch_status();
}

int pf_tsdf_count_triangles(const float* tsdf, const int* weight, int nx, int ny, int nz, int min_weight, int* count,
                            void* stream) {
  PF_REQUIRE(tsdf_dims_ok(nx, ny, nz));
  const int cells = tsdf_cells(nx, ny, nz);
  if (cells == 0) return PF_OK;
  PF_REQUIRE(tsdf && weight && count);
  hipLaunchKernelGGL(tsdf_count_kernel, dim3((unsigned)pf_cdiv(cells, 256)), dim3(256), 0, (hipStream_t)stream, tsdf, weight,
                     nx, ny, cells, min_weight, count);
  return pf_launch_status();
}

int pf_tsdf_emit_triangles(const float* tsdf, const int* weight, int nx, int ny, int nz, int min_weight,
                           const int64_t* inclusive, int64_t faces, int64_t* keys, void* stream) {
  PF_REQUIRE(tsdf_dims_ok(nx, ny, nz) && faces >= 0);
  const int cells = tsdf_cells(nx, ny, nz);
  if (cells == 0 || faces == 0) return PF_OK;
  PF_REQUIRE(tsdf && weight && inclusive && keys);
  hipLaunchKernelGGL(tsdf_emit_kernel, dim3((unsigned)pf_cdiv(cells, 256)), dim3(256), 0, (hipStream_t)stream, tsdf, weight, nx,
                     ny, cells, min_weight, inclusive, faces, keys);
  return pf_launch_status();
}

int pf_tsdf_vertices_f32(const int64_t* keys, int64_t count, const float* tsdf, const unsigned char* colour, float ox, float oy,
                         float oz, float voxel, int nx, int ny, int nz, float* vertices, unsigned char* colours, void* stream) {
  PF_REQUIRE(tsdf_dims_ok(nx, ny, nz) && count >= 0 && pf_cdiv(count, 256) <= INT32_MAX);
  if (count == 0) return PF_OK;
  PF_REQUIRE(keys && tsdf && vertices && (colour == nullptr) == (colours == nullptr));
  hipLaunchKernelGGL(tsdf_vertices_kernel, dim3((unsigned)pf_cdiv(count, 256)), dim3(256), 0, (hipStream_t)stream, keys, count,
                     tsdf, colour, ox, oy, oz, voxel, nx, ny, nz, vertices, colours);
  return pf_launch_status();
}

}  // extern "C"
