// Exact point-to-triangle-mesh distances (pointmvsnet_amd/mesh_distance.py, which holds the specification): per query the
// lexicographic minimum of (d2, face index) over all faces, d2 in float64 from the float32 coordinates.
//
// The search structure is cloud_eval.hip's sorted sparse grid (pf_cloud_grid.h) with a (cell, face) PAIR for a point: a face
// is listed in every cell of the box lo .. hi, lo = cell(min over its vertices - margin), hi = cell(max + margin) per axis,
// margin = kBoxMargin * edge in float32.  The search is pf_cloud_grid.h's, whose margin comment argues for points; why it
// may trust a list of boxes: let c be the point of a face nearest to the query q and T(x) = (x - origin) / edge the true
// quotient per axis.  A computed cell coordinate is floor(T + e) with |e| < 0.016 (at most 2^17 cells per axis,
// pf_cloud_grid.h), so lo <= floor(T(min) - 0.02 + 0.016) <= floor(T(c)) <= hi:
// the face is listed in the cell floor(T(c)).  If |c - q| <= (r - 0.05) edge, then T(c) < T~(q) + 0.016 + r - 0.05 < T~(q) + r
// with T~ the computed quotient of q, so floor(T(c)) lies within r of q's computed cell, on both sides: a search that has
// walked the cube of radius r cells around q's cell has met every face nearer than (r - 0.05) edge.  (The float64 d2 is
// within 2^-50 L^2 of the true squared distance; the slack above is 0.018 cells >= 0.018 * extent / 2^17.)  A face listed in
// several visited cells is met several times, which the lexicographic minimum does not notice.
//
//   mesh_dist_count   one thread per face: the number of cells in its box, 0 for a face that is skipped (an index outside
//                     [0, Nv) or a non-finite vertex), clamped to `limit` so that the host's sum cannot overflow.
//   mesh_dist_emit    one thread per pair: its face by binary search in the inclusive sums (mesh_ops.hip's sample emit), its
//                     cell by its rank in the face's box: the cell key and the face index.  The host sorts the keys.
//   mesh_dist_pack    one thread per sorted slot: the 48-byte record (a, face index; b; c), so that the inner loops below
//                     have no dependent index load.
//   mesh_dist_cells / mesh_dist_wave   pf_cloud_grid.h's two passes over the face records (MeshNearest): a thread per query on
//                     the fine grid, a WAVE per unfinished query on the coarse grid (edge >= 1.05 * max_dist: 27 cells list
//                     every face within max_dist), minima by (d2, face index).
// No atomics, no LDS, no scratch (no per-thread stack: that is why this is a grid and not a tree); every load is guarded by
// its array's length.  Two runs give identical bytes.
#include "pf_cloud_grid.h"

namespace {

constexpr float kBoxMargin = 0.02f;        // PF_MESH_DIST_BOX_MARGIN of the header, in cells

struct __attribute__((aligned(16))) FaceRecord {
  float ax, ay, az;
  int face;
  float bx, by, bz;
  int pad0;
  float cx, cy, cz;
  int pad1;
};
static_assert(sizeof(FaceRecord) == 48, "the face record is three 16-byte rows");

struct FaceBox {
  int lx, ly, lz, hx, hy, hz;
  bool ok;
};

// the cells a face is listed in; !ok for a face without a surface
__device__ __forceinline__ FaceBox face_box(const float* __restrict__ vertices, int64_t Nv, const int* __restrict__ faces,
                                            int64_t f, const CloudGrid& g) {
  FaceBox box = {0, 0, 0, -1, -1, -1, false};
  const int a = faces[f * 3 + 0], b = faces[f * 3 + 1], c = faces[f * 3 + 2];
  if (a < 0 || b < 0 || c < 0 || a >= Nv || b >= Nv || c >= Nv) return box;
  const float ax = vertices[(int64_t)a * 3 + 0], ay = vertices[(int64_t)a * 3 + 1], az = vertices[(int64_t)a * 3 + 2];
  const float bx = vertices[(int64_t)b * 3 + 0], by = vertices[(int64_t)b * 3 + 1], bz = vertices[(int64_t)b * 3 + 2];
  const float cx = vertices[(int64_t)c * 3 + 0], cy = vertices[(int64_t)c * 3 + 1], cz = vertices[(int64_t)c * 3 + 2];
  if (!(isfinite(ax) && isfinite(ay) && isfinite(az) && isfinite(bx) && isfinite(by) && isfinite(bz) && isfinite(cx) &&
        isfinite(cy) && isfinite(cz)))
    return box;
  const float m = kBoxMargin * g.edge;
  box.lx = cell_coord(fminf(fminf(ax, bx), cx) - m, g.ox, g.edge, 0, g.nx - 1);
  box.ly = cell_coord(fminf(fminf(ay, by), cy) - m, g.oy, g.edge, 0, g.ny - 1);
  box.lz = cell_coord(fminf(fminf(az, bz), cz) - m, g.oz, g.edge, 0, g.nz - 1);
  box.hx = cell_coord(fmaxf(fmaxf(ax, bx), cx) + m, g.ox, g.edge, 0, g.nx - 1);
  box.hy = cell_coord(fmaxf(fmaxf(ay, by), cy) + m, g.oy, g.edge, 0, g.ny - 1);
  box.hz = cell_coord(fmaxf(fmaxf(az, bz), cz) + m, g.oz, g.edge, 0, g.nz - 1);
  box.ok = box.lx <= box.hx && box.ly <= box.hy && box.lz <= box.hz;
  return box;
}

__global__ __launch_bounds__(256) void mesh_dist_count_kernel(const float* __restrict__ vertices, int64_t Nv,
                                                              const int* __restrict__ faces, int64_t Nf, CloudGrid g,
                                                              int64_t limit, int64_t* __restrict__ count) {
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= Nf) return;
  const FaceBox box = face_box(vertices, Nv, faces, f, g);
  int64_t n = 0;
  if (box.ok) {
    n = (int64_t)(box.hx - box.lx + 1) * (int64_t)(box.hy - box.ly + 1) * (int64_t)(box.hz - box.lz + 1);   // <= 2^51
    n = n > limit ? limit : n;
  }
  count[f] = n;
}

__global__ __launch_bounds__(256) void mesh_dist_emit_kernel(const float* __restrict__ vertices, int64_t Nv,
                                                             const int* __restrict__ faces, int64_t Nf, CloudGrid g,
                                                             const int64_t* __restrict__ incl, int64_t total,
                                                             int64_t* __restrict__ keys, int* __restrict__ pair_face) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= total) return;
  int64_t lo = 0, hi = Nf;                                // the first face whose inclusive sum exceeds s
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (incl[mid] > s) {
      hi = mid;
    } else {
      lo = mid + 1;
    }
  }
  int64_t key = INT64_MAX;                                // (sums that are not this mesh's: a pair no search reaches)
  int face = -1;
  if (lo < Nf) {
    const int64_t f = lo;
    const int64_t j = s - (f ? incl[f - 1] : 0);
    const FaceBox box = face_box(vertices, Nv, faces, f, g);
    if (box.ok && j >= 0) {
      const int64_t ny = box.hy - box.ly + 1, nz = box.hz - box.lz + 1;
      const int64_t dx = j / (ny * nz), rest = j - dx * (ny * nz);
      const int64_t dy = rest / nz, dz = rest - dy * nz;
      if (dx <= box.hx - box.lx) {
        key = cell_key(box.lx + (int)dx, box.ly + (int)dy, box.lz + (int)dz);
        face = (int)f;
      }
    }
  }
  keys[s] = key;
  pair_face[s] = face;
}

__global__ __launch_bounds__(256) void mesh_dist_pack_kernel(const float* __restrict__ vertices, int64_t Nv,
                                                             const int* __restrict__ faces, int64_t Nf,
                                                             const int* __restrict__ pair_face,
                                                             const int64_t* __restrict__ order, int64_t total,
                                                             FaceRecord* __restrict__ records) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const float nan = __builtin_nanf("");
  FaceRecord r = {nan, nan, nan, -1, nan, nan, nan, 0, nan, nan, nan, 0};      // a NaN record loses every comparison
  const int64_t src = order[i];
  if (src >= 0 && src < total) {
    const int f = pair_face[src];
    if (f >= 0 && f < Nf) {
      const int a = faces[(int64_t)f * 3 + 0], b = faces[(int64_t)f * 3 + 1], c = faces[(int64_t)f * 3 + 2];
      if (a >= 0 && b >= 0 && c >= 0 && a < Nv && b < Nv && c < Nv) {
        r.ax = vertices[(int64_t)a * 3 + 0], r.ay = vertices[(int64_t)a * 3 + 1], r.az = vertices[(int64_t)a * 3 + 2];
        r.bx = vertices[(int64_t)b * 3 + 0], r.by = vertices[(int64_t)b * 3 + 1], r.bz = vertices[(int64_t)b * 3 + 2];
        r.cx = vertices[(int64_t)c * 3 + 0], r.cy = vertices[(int64_t)c * 3 + 1], r.cz = vertices[(int64_t)c * 3 + 2];
        r.face = f;
      }
    }
  }
  records[i] = r;
}

// ---- the distance of the specification, float64 throughout --------------------------------------------------------------
struct Vec3 {
  double x, y, z;
};

__device__ __forceinline__ Vec3 sub(const Vec3& u, const Vec3& v) { return {u.x - v.x, u.y - v.y, u.z - v.z}; }

__device__ __forceinline__ double dot(const Vec3& u, const Vec3& v) { return (u.x * v.x + u.y * v.y) + u.z * v.z; }

__device__ __forceinline__ Vec3 cross(const Vec3& u, const Vec3& v) {
  return {u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x};
}

__device__ __forceinline__ double seg_d2(const Vec3& p, const Vec3& u, const Vec3& v) {
  const Vec3 e = sub(v, u), w = sub(p, u);
  const double ee = dot(e, e);
  double t = 0.0;
  if (ee > 0.0) t = fmin(fmax(dot(w, e) / ee, 0.0), 1.0);
  const Vec3 r = {w.x - t * e.x, w.y - t * e.y, w.z - t * e.z};
  return dot(r, r);
}

__device__ __forceinline__ double face_d2(const Vec3& p, const FaceRecord& r) {
  const Vec3 a = {(double)r.ax, (double)r.ay, (double)r.az};
  const Vec3 b = {(double)r.bx, (double)r.by, (double)r.bz};
  const Vec3 c = {(double)r.cx, (double)r.cy, (double)r.cz};
  double d2 = fmin(fmin(seg_d2(p, a, b), seg_d2(p, b, c)), seg_d2(p, c, a));
  const Vec3 ab = sub(b, a), pa = sub(p, a);
  const Vec3 n = cross(ab, sub(c, a));
  const double nn = dot(n, n);
  const bool inside = nn > 0.0 && dot(cross(ab, pa), n) >= 0.0 && dot(cross(sub(c, b), sub(p, b)), n) >= 0.0 &&
                      dot(cross(sub(a, c), sub(p, c)), n) >= 0.0;
  if (inside) {
    const double h = dot(pa, n);
    d2 = fmin((h * h) / nn, d2);
  }
  return d2;
}

// point_mesh_distances' policy for pf_cloud_grid.h's two passes: float64 d2, the lexicographic minimum of (d2, face index)
struct MeshNearest {
  const FaceRecord* __restrict__ records;
  float* __restrict__ dist;
  int* __restrict__ face;
  Vec3 p;
  double best;
  int best_face;

  __device__ __forceinline__ void start(float x, float y, float z) {
    p = {(double)x, (double)y, (double)z};
    best = INFINITY;
    best_face = -1;
  }
  // (d2, f) replaces the best where it is better: never for a NaN d2
  __device__ __forceinline__ void take(double d2, int f) {
    if (d2 < best || (d2 == best && (unsigned)f < (unsigned)best_face)) {
      best = d2;
      best_face = f;
    }
  }
  __device__ __forceinline__ void offer(int j) {
    const FaceRecord rec = records[j];
    take(face_d2(p, rec), rec.face);
  }
  __device__ __forceinline__ bool within(float reach) const { return best <= (double)reach * (double)reach; }
  __device__ __forceinline__ void merge(int off) {
    const double ob = __shfl_xor(best, off);
    const int of = __shfl_xor(best_face, off);
    take(ob, of);
  }
  __device__ __forceinline__ void write(int64_t i, float max_dist) const {
    const float d = (float)sqrt(best);
    const bool capped = !(d < max_dist) || best_face < 0;
    dist[i] = capped ? max_dist : d;
    face[i] = capped ? -1 : best_face;
  }
};

__global__ __launch_bounds__(256) void mesh_dist_cells_kernel(const float* __restrict__ query, int64_t nq,
                                                              const FaceRecord* __restrict__ records,
                                                              const int64_t* __restrict__ keys, int np, CloudGrid g, int rings,
                                                              float max_dist, float* __restrict__ dist, int* __restrict__ face,
                                                              unsigned char* __restrict__ done) {
  nearest_cells_pass(MeshNearest{records, dist, face}, query, nq, keys, np, g, rings, max_dist, done);
}

__global__ __launch_bounds__(256) void mesh_dist_wave_kernel(const float* __restrict__ query, const int64_t* __restrict__ todo,
                                                             int64_t ntodo, int64_t nq, const FaceRecord* __restrict__ records,
                                                             const int64_t* __restrict__ keys, int np, CloudGrid g,
                                                             float max_dist, float* __restrict__ dist,
                                                             int* __restrict__ face) {
  nearest_wave_pass(MeshNearest{records, dist, face}, query, todo, ntodo, nq, keys, np, g, max_dist);
}

inline bool dist_sizes_ok(int64_t Nv, int64_t Nf) {
  return Nv >= 0 && Nv <= PF_MESH_OPS_MAX && Nf >= 0 && Nf <= PF_MESH_DIST_MAX_FACES;
}

inline bool pairs_ok(int64_t total) { return total >= 0 && total <= PF_MESH_DIST_MAX_PAIRS; }

}  // namespace

extern "C" {

int pf_mesh_dist_count_f32(const float* vertices, int64_t Nv, const int* faces, int64_t Nf, float ox, float oy, float oz,
                           float edge, int nx, int ny, int nz, int64_t limit, int64_t* count, void* stream) {
  PF_REQUIRE(dist_sizes_ok(Nv, Nf) && grid_ok(nx, ny, nz, edge) && limit >= 1 && limit <= (1ll << 32));
  if (Nf == 0) return PF_OK;
  PF_REQUIRE(faces && count && (vertices || Nv == 0));
  const CloudGrid g = {ox, oy, oz, edge, nx, ny, nz};
  hipLaunchKernelGGL(mesh_dist_count_kernel, dim3(blocks_of(Nf)), dim3(256), 0, (hipStream_t)stream, vertices, Nv, faces, Nf,
                     g, limit, count);
  return pf_launch_status();
}

int pf_mesh_dist_emit_f32(const float* vertices, int64_t Nv, const int* faces, int64_t Nf, float ox, float oy, float oz,
                          float edge, int nx, int ny, int nz, const int64_t* inclusive, int64_t total, int64_t* keys,
                          int* pair_face, void* stream) {
  PF_REQUIRE(dist_sizes_ok(Nv, Nf) && grid_ok(nx, ny, nz, edge) && pairs_ok(total));
  if (total == 0) return PF_OK;
  PF_REQUIRE(Nf > 0 && vertices && faces && inclusive && keys && pair_face);
  const CloudGrid g = {ox, oy, oz, edge, nx, ny, nz};
  hipLaunchKernelGGL(mesh_dist_emit_kernel, dim3(blocks_of(total)), dim3(256), 0, (hipStream_t)stream, vertices, Nv, faces,
                     Nf, g, inclusive, total, keys, pair_face);
  return pf_launch_status();
}

int pf_mesh_dist_pack_f32(const float* vertices, int64_t Nv, const int* faces, int64_t Nf, const int* pair_face,
                          const int64_t* order, int64_t total, void* records, void* stream) {
  PF_REQUIRE(dist_sizes_ok(Nv, Nf) && pairs_ok(total));
  if (total == 0) return PF_OK;
  PF_REQUIRE(Nf > 0 && vertices && faces && pair_face && order && records && ((uintptr_t)records & 15) == 0);
  hipLaunchKernelGGL(mesh_dist_pack_kernel, dim3(blocks_of(total)), dim3(256), 0, (hipStream_t)stream, vertices, Nv, faces,
                     Nf, pair_face, order, total, reinterpret_cast<FaceRecord*>(records));
  return pf_launch_status();
}

int pf_mesh_dist_cells_f64(const float* query, int64_t nq, const void* records, const int64_t* keys, int64_t total, float ox,
                           float oy, float oz, float edge, int nx, int ny, int nz, int rings, float max_dist, float* dist,
                           int* face, unsigned char* done, void* stream) {
  PF_REQUIRE(count_ok(nq) && pairs_ok(total) && total >= 1 && grid_ok(nx, ny, nz, edge) && rings >= 1 && rings <= 15 &&
             max_dist > 0.0f);
  if (nq == 0) return PF_OK;
  PF_REQUIRE(query && records && keys && dist && face && done && ((uintptr_t)records & 15) == 0);
  const CloudGrid g = {ox, oy, oz, edge, nx, ny, nz};
  hipLaunchKernelGGL(mesh_dist_cells_kernel, dim3(blocks_of(nq)), dim3(256), 0, (hipStream_t)stream, query, nq,
                     reinterpret_cast<const FaceRecord*>(records), keys, (int)total, g, rings, max_dist, dist, face, done);
  return pf_launch_status();
}

int pf_mesh_dist_wave_f64(const float* query, const int64_t* todo, int64_t ntodo, int64_t nq, const void* records,
                          const int64_t* keys, int64_t total, float ox, float oy, float oz, float edge, int nx, int ny, int nz,
                          float max_dist, float* dist, int* face, void* stream) {
  PF_REQUIRE(count_ok(nq) && pairs_ok(total) && total >= 1 && ntodo >= 0 && ntodo <= nq && grid_ok(nx, ny, nz, edge) &&
             max_dist > 0.0f);
  PF_REQUIRE(edge >= max_dist);                     // the 27 cells must list every face within max_dist
  if (ntodo == 0) return PF_OK;
  PF_REQUIRE(query && todo && records && keys && dist && face && ((uintptr_t)records & 15) == 0);
  PF_REQUIRE(ntodo <= (int64_t)UINT32_MAX * 4);     // one wave per query, four waves per block
  const CloudGrid g = {ox, oy, oz, edge, nx, ny, nz};
  hipLaunchKernelGGL(mesh_dist_wave_kernel, dim3(blocks_of(ntodo * PF_WAVE)), dim3(256), 0, (hipStream_t)stream, query, todo,
                     ntodo, nq, reinterpret_cast<const FaceRecord*>(records), keys, (int)total, g, max_dist, dist, face);
  return pf_launch_status();
}

}  // extern "C"
