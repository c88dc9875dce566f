// The sparse TSDF volume: the dense volume of tsdf.hip stored only near the surface, in bricks of 8 x 8 x 8 samples
// (specification: pointmvsnet_amd/sparse_tsdf.py, include/pointflow_hip.h).  The virtual grid is the dense one; brick
// (bi, bj, bk) = (i >> 3, j >> 3, k >> 3) has the key (bk NBy + bj) NBx + bi; the allocated bricks are ONE SORTED ARRAY of
// unique keys and a brick is found by binary search (the idiom of pf_cloud_grid.h; no hash table).  Brick b of that array
// owns rows b of S, W, CS, CW, 512 samples each, local index (lk * 8 + lj) * 8 + li, x fastest.  The per-view update, the
// tetrahedra, the edge keys and the vertex arithmetic are pf_tsdf.h's, the dense kernels' own.
//
//   sparse_tsdf_touch       one WAVE per virtual brick, four per block.  The view is the wave-uniform outer loop (its 12 floats
//                           arrive by scalar loads); the brick's box grown by one sample is projected by its 8 corners with the
//                           dense expression, the 64 lanes stride over the pixel box of the projections, and the wave leaves
//                           the brick at the first pixel whose depth falls into the box's z-interval widened by trunc (__any).
//                           One byte per virtual brick, only ever set: calls accumulate.  Every float comparison that guards
//                           an address is made before the conversion to int.
//   sparse_tsdf_neighbours  one thread per allocated brick: the rows of its +x, +y, +xy, +z, +xz, +yz, +xyz bricks, -1 where
//                           such a brick is not allocated or lies outside the grid.
//   sparse_tsdf_integrate   one block of 512 per brick, a thread per sample, x fastest, the sums in registers, all views in
//                           ascending order by tsdf_integrate_view.  A sample outside dims is left alone: it stays zero.
//   sparse_tsdf_count/emit  one block of 512 per brick, a thread per cell (owned by the brick of its corner 0).  The block
//                           first stages one BYTE per sample of the 9 x 9 x 9 corners of its cells -- bit 0: weight >=
//                           min_weight, bit 1: tsdf < 0; 0 for a sample of a brick that is not there -- from its own brick and
//                           the seven neighbours, then every thread reads its 8 corners from LDS.  729 bytes.  A wave's 64
//                           cells are an 8 x 8 slab: their reads of one corner are the bytes lj * 9 + li, 71 consecutive bytes
//                           in 18 consecutive dwords, so no two lanes of a 32-lane group meet on a bank at different
//                           addresses and the 9-stride needs no padding.  min_weight >= 1, so a sample outside dims
//                           (W = 0) and an absent one read alike and no cell reaches past the grid.
//   sparse_tsdf_vertices    one thread per unique key: key -> (i, j, k) and direction -> the bricks of both ends by binary
//                           search -> tsdf_vertex.  A key that names no edge between allocated samples gives (0, 0, 0).
//
// No scratch, no atomics, no table in memory.
#include "pf_common.h"
#include "pf_tsdf.h"

#include <math.h>

// hipcc spells LDS `__shared__`.  The host re-compilation of tests/hipemu rewrites that spelling in the sources of its fixed
// list only; it reaches this file through eval_out.hip, so the emulator's spelling is chosen here (as in depth_segments.hip).
#if defined(__HIP__)
#define PF_SPARSE_LDS_DYNAMIC(name) extern __shared__ __attribute__((aligned(16))) unsigned char name[]
#else
#define PF_SPARSE_LDS_DYNAMIC(name) unsigned char* name = reinterpret_cast<unsigned char*>(::hipemu_shared_memory())
#endif

namespace {

constexpr int kBrick = 8, kBrickSamples = 512, kTile = 9, kTileSamples = 729, kTileBytes = 736;

struct SparseGrid {
  int nx, ny, nz, nbx, nby, nbz;
};

// first j in [0, n] with keys[j] >= k (pf_cloud_grid.h's search)
__device__ __forceinline__ int sparse_lower_bound(const int64_t* __restrict__ keys, int n, int64_t k) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < k) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// the row of brick (bi, bj, bk) in the sorted keys, -1 if it is outside the grid or not allocated
__device__ __forceinline__ int sparse_find(const int64_t* __restrict__ keys, int n, const SparseGrid& g, int bi, int bj, int bk) {
  if (bi < 0 || bj < 0 || bk < 0 || bi >= g.nbx || bj >= g.nby || bk >= g.nbz) return -1;
  const int64_t key = ((int64_t)bk * g.nby + bj) * g.nbx + bi;
  const int at = sparse_lower_bound(keys, n, key);
  return at < n && keys[at] == key ? at : -1;
}

__device__ __forceinline__ void sparse_brick_of_key(int64_t key, const SparseGrid& g, int& bi, int& bj, int& bk) {
  bi = (int)(key % g.nbx);
  const int64_t jk = key / g.nbx;
  bj = (int)(jk % g.nby);
  bk = (int)(jk / g.nby);
}

// ---- allocation ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sparse_tsdf_touch_kernel(const float* __restrict__ depths, const float* __restrict__ proj,
                                                                int V, int h, int w, float ox, float oy, float oz, float voxel,
                                                                SparseGrid g, int bricks, float trunc, float depth_min,
                                                                float depth_max, unsigned char* __restrict__ touched) {
  const int lane = threadIdx.x & 63;
  const int64_t b64 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  // no early return: every lane of the wave takes part in the votes; a wave without a brick walks no view
  const bool alive = b64 < bricks && touched[b64 < bricks ? b64 : 0] == 0;
  const int brick = alive ? (int)b64 : 0;
  const int bi = brick % g.nbx, bjk = brick / g.nbx;
  const int bj = bjk % g.nby, bk = bjk / g.nby;
  // the brick's box grown by one sample per side (the index may be -1 or n: the position is the same expression)
  const float X0 = ox + (float)(bi * kBrick - 1) * voxel, X1 = ox + (float)(bi * kBrick + kBrick) * voxel;
  const float Y0 = oy + (float)(bj * kBrick - 1) * voxel, Y1 = oy + (float)(bj * kBrick + kBrick) * voxel;
  const float Z0 = oz + (float)(bk * kBrick - 1) * voxel, Z1 = oz + (float)(bk * kBrick + kBrick) * voxel;
  const float wf = (float)w, hf = (float)h;
  const int64_t hw = (int64_t)h * w;
  const float kRound = 9.5367431640625e-07f;                                      // 2^-20 = 16 eps
  bool hit = false;
  for (int view = 0; view < (alive ? V : 0) && !hit; ++view) {
    const float* __restrict__ p = proj + (int64_t)view * PF_RENDER_PROJ_FLOATS;      // wave-uniform: scalar loads
    float zlo = INFINITY, zhi = -INFINITY, ulo = INFINITY, uhi = -INFINITY, vlo = INFINITY, vhi = -INFINITY;
    float amag = 0.0f, zmag = 0.0f;                                                // the largest sums of magnitudes
    bool bad = false;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const float X = (c & 1) ? X1 : X0, Y = (c & 2) ? Y1 : Y0, Z = (c & 4) ? Z1 : Z0;
      const float qx = ((p[0] * X + p[1] * Y) + p[2] * Z) + p[3];
      const float qy = ((p[4] * X + p[5] * Y) + p[6] * Z) + p[7];
      const float z = ((p[8] * X + p[9] * Y) + p[10] * Z) + p[11];
      const float ax = ((fabsf(p[0] * X) + fabsf(p[1] * Y)) + fabsf(p[2] * Z)) + fabsf(p[3]);
      const float ay = ((fabsf(p[4] * X) + fabsf(p[5] * Y)) + fabsf(p[6] * Z)) + fabsf(p[7]);
      const float az = ((fabsf(p[8] * X) + fabsf(p[9] * Y)) + fabsf(p[10] * Z)) + fabsf(p[11]);
      amag = fmaxf(amag, fmaxf(ax, ay));
      zmag = fmaxf(zmag, az);
      bad = bad || !(z == z) || !(qx == qx) || !(qy == qy);
      zlo = fminf(zlo, z), zhi = fmaxf(zhi, z);
      const float u = qx / z, v = qy / z;                                          // used only if every corner is in front
      ulo = fminf(ulo, u), uhi = fmaxf(uhi, u), vlo = fminf(vlo, v), vhi = fmaxf(vhi, v);
    }
    const float m = kRound * (zmag + trunc);                                       // the rounding margin of the z-interval
    // A NaN anywhere (matrices that are not finite): the conservative answer is the whole image and every depth.
    float dlo = depth_min, dhi = depth_max;
    bool whole = bad;
    if (!bad) {
      if (zhi + m <= depth_min || zlo - m >= depth_max) continue;                  // no sample of the box passes step 1
      dlo = (zlo - trunc) - m, dhi = (zhi + trunc) + m;
      // behind or at the camera plane, or so close to it that a rounding of the projection could reach a quarter pixel
      whole = !(zlo - m > depth_min) || !(kRound * (amag + fmaxf(wf, hf) * zmag) < 0.25f * zlo);
    }
    float fx0 = 0.0f, fx1 = wf - 1.0f, fy0 = 0.0f, fy1 = hf - 1.0f;
    if (!whole) {
      fx0 = fmaxf(floorf(ulo) - 1.0f, 0.0f), fx1 = fminf(floorf(uhi) + 1.0f, wf - 1.0f);
      fy0 = fmaxf(floorf(vlo) - 1.0f, 0.0f), fy1 = fminf(floorf(vhi) + 1.0f, hf - 1.0f);
    }
    if (!(fx0 <= fx1 && fy0 <= fy1)) continue;                                     // as floats: the conversions are in range
    const int x0 = (int)fx0, y0 = (int)fy0;
    const int bw = (int)fx1 - x0 + 1, bh = (int)fy1 - y0 + 1;
    const int npix = bw * bh;                                                      // at most h * w <= INT32_MAX / 4
    const float* __restrict__ map = depths + (int64_t)view * hw;
    for (int first = 0; first < npix && !hit; first += PF_WAVE) {                  // wave-uniform bounds: every lane votes
      const int at = first + lane;
      bool mine = false;
      if (at < npix) {
        const int dy = at / bw, dx = at - dy * bw;
        const float d = map[(int64_t)(y0 + dy) * w + (x0 + dx)];
        mine = d > depth_min && d < depth_max && d >= dlo && d <= dhi;
      }
      hit = __any(mine) != 0;
    }
  }
  if (alive && hit && lane == 0) touched[brick] = 1;
}

__global__ __launch_bounds__(256) void sparse_tsdf_neighbours_kernel(const int64_t* __restrict__ keys, int count, SparseGrid g,
                                                                     int* __restrict__ rows) {
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (n >= count) return;
  int bi, bj, bk;
  sparse_brick_of_key(keys[n], g, bi, bj, bk);
#pragma unroll
  for (int c = 1; c < 8; ++c)
    rows[n * 7 + (c - 1)] = sparse_find(keys, count, g, bi + (c & 1), bj + ((c >> 1) & 1), bk + (c >> 2));
}

// ---- integration --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(512) void sparse_tsdf_integrate_kernel(const int64_t* __restrict__ keys,
                                                                    const float* __restrict__ depths,
                                                                    const unsigned char* __restrict__ images,
                                                                    const float* __restrict__ proj, int V, int h, int w, float ox,
                                                                    float oy, float oz, float voxel, SparseGrid g, float trunc,
                                                                    float depth_min, float depth_max, float* __restrict__ S,
                                                                    int* __restrict__ W, int* __restrict__ CS,
                                                                    int* __restrict__ CW) {
  int bi, bj, bk;
  sparse_brick_of_key(keys[blockIdx.x], g, bi, bj, bk);
  const int t = threadIdx.x;
  const int i = bi * kBrick + (t & 7), j = bj * kBrick + ((t >> 3) & 7), k = bk * kBrick + (t >> 6);
  if (i >= g.nx || j >= g.ny || k >= g.nz) return;                                 // outside dims: never integrated
  const int n = (int)blockIdx.x * kBrickSamples + t;                               // Nb * 512 <= INT32_MAX
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
// Stages the block's 9 x 9 x 9 corner bytes and returns the mask of the thread's cell (bit c: corner c is inside; -1: a
// corner with weight < min_weight, absent or outside dims).  Ends with the block's threads past a barrier.
__device__ __forceinline__ int sparse_cell_mask(const float* __restrict__ tsdf, const int* __restrict__ weight,
                                                const int* __restrict__ rows, int min_weight, unsigned char* tile) {
  const int brick = (int)blockIdx.x, t = threadIdx.x;
  for (int s = t; s < kTileSamples; s += kBrickSamples) {
    const int x = s % kTile, yz = s / kTile;
    const int y = yz % kTile, z = yz / kTile;
    const int c = (x >> 3) | ((y >> 3) << 1) | ((z >> 3) << 2);                    // which of the eight bricks
    const int row = c == 0 ? brick : rows[(int64_t)brick * 7 + (c - 1)];
    unsigned char code = 0;
    if (row >= 0) {
      const int at = row * kBrickSamples + (((z & 7) * kBrick + (y & 7)) * kBrick + (x & 7));
      code = (unsigned char)((weight[at] >= min_weight ? 1 : 0) | (tsdf[at] < 0.0f ? 2 : 0));
    }
    tile[s] = code;
  }
  __syncthreads();
  const int base = ((t >> 6) * kTile + ((t >> 3) & 7)) * kTile + (t & 7);
  int mask = 0, seen = 1;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int code = tile[base + (c & 1) + ((c >> 1) & 1) * kTile + (c >> 2) * kTile * kTile];
    seen &= code;
    mask |= (code >> 1) << c;
  }
  return seen ? mask : -1;
}

__global__ __launch_bounds__(512) void sparse_tsdf_count_kernel(const float* __restrict__ tsdf, const int* __restrict__ weight,
                                                                const int* __restrict__ rows, int min_weight,
                                                                int* __restrict__ count) {
  PF_SPARSE_LDS_DYNAMIC(tile);
  const int mask = sparse_cell_mask(tsdf, weight, rows, min_weight, tile);
  count[(int64_t)blockIdx.x * kBrickSamples + threadIdx.x] = tsdf_cell_triangles(mask);
}

__global__ __launch_bounds__(512) void sparse_tsdf_emit_kernel(const int64_t* __restrict__ keys, const float* __restrict__ tsdf,
                                                               const int* __restrict__ weight, const int* __restrict__ rows,
                                                               SparseGrid g, int min_weight, const int64_t* __restrict__ incl,
                                                               int64_t faces, int64_t* __restrict__ tri_keys) {
  PF_SPARSE_LDS_DYNAMIC(tile);
  const int mask = sparse_cell_mask(tsdf, weight, rows, min_weight, tile);
  if (!(mask > 0 && mask < 255)) return;
  int bi, bj, bk;
  sparse_brick_of_key(keys[blockIdx.x], g, bi, bj, bk);
  const int t = threadIdx.x;
  const int64_t i = bi * kBrick + (t & 7), j = bj * kBrick + ((t >> 3) & 7), k = bk * kBrick + (t >> 6);
  const int64_t nx = g.nx, nxy = (int64_t)g.nx * g.ny;
  const int64_t cell = (int64_t)blockIdx.x * kBrickSamples + t;
  tsdf_emit_cell<int64_t>(mask, (k * g.ny + j) * nx + i, nx, nxy, cell ? incl[cell - 1] : 0, faces, tri_keys);
}

// the row of sample (i, j, k) in the brick arrays, -1 if its brick is not allocated
__device__ __forceinline__ int sparse_sample_row(const int64_t* __restrict__ keys, int bricks, const SparseGrid& g, int i, int j,
                                                 int k) {
  const int row = sparse_find(keys, bricks, g, i >> 3, j >> 3, k >> 3);
  return row < 0 ? -1 : row * kBrickSamples + (((k & 7) * kBrick + (j & 7)) * kBrick + (i & 7));
}

__global__ __launch_bounds__(256) void sparse_tsdf_vertices_kernel(const int64_t* __restrict__ edge_keys, int64_t count,
                                                                   const int64_t* __restrict__ keys, int bricks,
                                                                   const float* __restrict__ tsdf,
                                                                   const unsigned char* __restrict__ colour, float ox, float oy,
                                                                   float oz, float voxel, SparseGrid g,
                                                                   float* __restrict__ vertices,
                                                                   unsigned char* __restrict__ colours) {
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (n >= count) return;
  const int64_t key = edge_keys[n];
  const int dir = (int)(key & 7);
  const int64_t a64 = key >> 3;
  const int64_t total = (int64_t)g.nx * g.ny * g.nz;
  bool edge = false;
  int r = 0, gr = 0, b = 0;
  if (a64 >= 0 && a64 < total && dir != 0) {
    const int i = (int)(a64 % g.nx);
    const int64_t jk = a64 / g.nx;
    const int j = (int)(jk % g.ny), k = (int)(jk / g.ny);
    const int dx = dir & 1, dy = (dir >> 1) & 1, dz = dir >> 2;
    if (i + dx < g.nx && j + dy < g.ny && k + dz < g.nz) {                         // a key that is not this volume's reads nothing
      const int a = sparse_sample_row(keys, bricks, g, i, j, k);
      const int bb = sparse_sample_row(keys, bricks, g, i + dx, j + dy, k + dz);
      if (a >= 0 && bb >= 0) {
        edge = true;
        const float t = tsdf_vertex(tsdf[a], tsdf[bb], i, j, k, dx, dy, dz, ox, oy, oz, voxel, vertices + n * 3);
        if (colour != nullptr) {
          const unsigned char* ca = colour + (int64_t)a * 3;
          const unsigned char* cb = colour + (int64_t)bb * 3;
          r = tsdf_vertex_colour(ca[0], cb[0], t);
          gr = tsdf_vertex_colour(ca[1], cb[1], t);
          b = tsdf_vertex_colour(ca[2], cb[2], t);
        }
      }
    }
  }
  if (!edge) vertices[n * 3 + 0] = vertices[n * 3 + 1] = vertices[n * 3 + 2] = 0.0f;
  if (colours != nullptr) {
    colours[n * 3 + 0] = (unsigned char)r;
    colours[n * 3 + 1] = (unsigned char)gr;
    colours[n * 3 + 2] = (unsigned char)b;
  }
}

// dims of the virtual grid: at most 2^20 samples per axis, fewer than 2^60 in all (implied), fewer than 2^31 bricks
inline bool sparse_grid_ok(int nx, int ny, int nz, SparseGrid* g) {
  if (nx < 1 || ny < 1 || nz < 1 || nx > PF_SPARSE_TSDF_MAX_AXIS || ny > PF_SPARSE_TSDF_MAX_AXIS || nz > PF_SPARSE_TSDF_MAX_AXIS)
    return false;
  *g = SparseGrid{nx, ny, nz, (nx + 7) / 8, (ny + 7) / 8, (nz + 7) / 8};
  return (int64_t)g->nbx * g->nby * g->nbz <= INT32_MAX;
}

inline bool sparse_bricks_ok(int64_t bricks) { return bricks >= 0 && bricks <= INT32_MAX / kBrickSamples; }

}  // namespace

extern "C" {

int pf_sparse_tsdf_touch(const float* depths, const float* proj, int V, int h, int w, float ox, float oy, float oz, float voxel,
                         int nx, int ny, int nz, float trunc, float depth_min, float depth_max, unsigned char* touched,
                         void* stream) {
  SparseGrid g;
  PF_REQUIRE(sparse_grid_ok(nx, ny, nz, &g) && V >= 0 && h >= 0 && w >= 0 && (int64_t)h * w <= INT32_MAX / 4);
  PF_REQUIRE(voxel > 0.0f && trunc > 0.0f);
  if (V == 0 || h == 0 || w == 0) return PF_OK;
  PF_REQUIRE(depths && proj && touched);
  const int bricks = g.nbx * g.nby * g.nbz;
  hipLaunchKernelGGL(sparse_tsdf_touch_kernel, dim3((unsigned)pf_cdiv(bricks, 4)), dim3(256), 0, (hipStream_t)stream, depths,
                     proj, V, h, w, ox, oy, oz, voxel, g, bricks, trunc, depth_min, depth_max, touched);
  return pf_launch_status();
}

int pf_sparse_tsdf_neighbours(const int64_t* keys, int64_t bricks, int nx, int ny, int nz, int* rows, void* stream) {
  SparseGrid g;
  PF_REQUIRE(sparse_grid_ok(nx, ny, nz, &g) && sparse_bricks_ok(bricks));
  if (bricks == 0) return PF_OK;
  PF_REQUIRE(keys && rows);
  hipLaunchKernelGGL(sparse_tsdf_neighbours_kernel, dim3((unsigned)pf_cdiv(bricks, 256)), dim3(256), 0, (hipStream_t)stream,
                     keys, (int)bricks, g, rows);
  return pf_launch_status();
}

int pf_sparse_tsdf_integrate_f32(const int64_t* keys, int64_t bricks, const float* depths, const unsigned char* images,
                                 const float* proj, int V, int h, int w, float ox, float oy, float oz, float voxel, int nx, int ny,
                                 int nz, float trunc, float depth_min, float depth_max, float* S, int* W, int* CS, int* CW,
                                 void* stream) {
  SparseGrid g;
  PF_REQUIRE(sparse_grid_ok(nx, ny, nz, &g) && sparse_bricks_ok(bricks));
  PF_REQUIRE(V >= 0 && h >= 0 && w >= 0 && (int64_t)h * w <= INT32_MAX / 4 && voxel > 0.0f && trunc > 0.0f);
  if (bricks == 0 || V == 0 || h == 0 || w == 0) return PF_OK;
  PF_REQUIRE(keys && depths && proj && S && W && (images == nullptr || (CS && CW)));
  hipLaunchKernelGGL(sparse_tsdf_integrate_kernel, dim3((unsigned)bricks), dim3(kBrickSamples), 0, (hipStream_t)stream, keys,
                     depths, images, proj, V, h, w, ox, oy, oz, voxel, g, trunc, depth_min, depth_max, S, W, CS, CW);
  return pf_launch_status();
}

int pf_sparse_tsdf_count_triangles(const float* tsdf, const int* weight, const int* rows, int64_t bricks, int min_weight,
                                   int* count, void* stream) {
  PF_REQUIRE(sparse_bricks_ok(bricks) && min_weight >= 1);
  if (bricks == 0) return PF_OK;
  PF_REQUIRE(tsdf && weight && rows && count);
  hipLaunchKernelGGL(sparse_tsdf_count_kernel, dim3((unsigned)bricks), dim3(kBrickSamples), kTileBytes, (hipStream_t)stream, tsdf,
                     weight, rows, min_weight, count);
  return pf_launch_status();
}

int pf_sparse_tsdf_emit_triangles(const int64_t* keys, int64_t bricks, const float* tsdf, const int* weight, const int* rows,
                                  int nx, int ny, int nz, int min_weight, const int64_t* inclusive, int64_t faces,
                                  int64_t* tri_keys, void* stream) {
  SparseGrid g;
  PF_REQUIRE(sparse_grid_ok(nx, ny, nz, &g) && sparse_bricks_ok(bricks) && min_weight >= 1 && faces >= 0);
  if (bricks == 0 || faces == 0) return PF_OK;
  PF_REQUIRE(keys && tsdf && weight && rows && inclusive && tri_keys);
  hipLaunchKernelGGL(sparse_tsdf_emit_kernel, dim3((unsigned)bricks), dim3(kBrickSamples), kTileBytes, (hipStream_t)stream, keys,
                     tsdf, weight, rows, g, min_weight, inclusive, faces, tri_keys);
  return pf_launch_status();
}

int pf_sparse_tsdf_vertices_f32(const int64_t* edge_keys, int64_t count, const int64_t* keys, int64_t bricks, const float* tsdf,
                                const unsigned char* colour, float ox, float oy, float oz, float voxel, int nx, int ny, int nz,
                                float* vertices, unsigned char* colours, void* stream) {
  SparseGrid g;
  PF_REQUIRE(sparse_grid_ok(nx, ny, nz, &g) && sparse_bricks_ok(bricks) && count >= 0 && pf_cdiv(count, 256) <= INT32_MAX);
  if (count == 0) return PF_OK;
  PF_REQUIRE(edge_keys && vertices && (bricks == 0 || (keys && tsdf)) && (colour == nullptr) == (colours == nullptr));
  hipLaunchKernelGGL(sparse_tsdf_vertices_kernel, dim3((unsigned)pf_cdiv(count, 256)), dim3(256), 0, (hipStream_t)stream, edge_keys,
                     count, keys, (int)bricks, tsdf, colour, ox, oy, oz, voxel, g, vertices, colours);
  return pf_launch_status();
}

}  // extern "C"
