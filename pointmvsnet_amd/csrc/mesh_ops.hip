// Mesh clean-up and scoring: connected components, area-weighted vertex normals and surface sampling of a triangle mesh
// (specification: pointmvsnet_amd/mesh_ops.py, include/pointflow_hip.h).  vertices (Nv, 3) float32, faces (Nf, 3) int32.
// Every kernel skips a face with an index outside [0, Nv) before it forms an address from it, and every table that comes
// from the caller (label, offsets, corners, the inclusive sums) is range-checked where it is read: no input faults.  No LDS,
// no per-thread array, no scratch, no float atomics.
//
//   mesh_cc_hook      one thread per face: unite(a, b) and unite(a, c) on the array `label` (two edges connect all three).
//   mesh_cc_compress  one thread per vertex: walk to the root, then atomicMin(label[v], root).
//   mesh_face_labels  one thread per face: the label of its first vertex (-1 for a face that is skipped).
//   mesh_vertex_normals  one thread per vertex walks its corner list (ascending corner 3 f + j) and adds the faces' float32
//                     cross products to a float64 sum in that order.  A vertex is owned by one thread: no atomics, one order.
//   mesh_sample_count one thread per face: floorf(area / pitch^2 + u_f), u_f from the face's hash (stochastic rounding).
//   mesh_sample_emit  one thread per SAMPLE: its face by binary search in the inclusive sums of the counts, its two random
//                     numbers from (face, j) alone.  A face that takes 10^6 samples is 10^6 threads, not one long loop.
//
// Connected components: the hook-and-compress scheme (cc_find, cc_unite) and the argument why it is correct on a chip whose
// caches are not coherent are stated in pf_union_find.h, which depth_segments.hip shares.
#include "pf_hash.h"
#include "pf_union_find.h"

#include <math.h>

namespace {

__device__ __forceinline__ bool mesh_face_ok(int a, int b, int c, int64_t Nv) {
  return a >= 0 && a < Nv && b >= 0 && b < Nv && c >= 0 && c < Nv;
}

__global__ __launch_bounds__(256) void mesh_cc_hook_kernel(const int* __restrict__ faces, int64_t Nf, int64_t Nv,
                                                           int* __restrict__ label, int* __restrict__ changed) {
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= Nf) return;
  const int a = faces[f * 3 + 0], b = faces[f * 3 + 1], c = faces[f * 3 + 2];
  if (!mesh_face_ok(a, b, c, Nv)) return;
  const bool ab = cc_unite(label, a, b);
  const bool ac = cc_unite(label, a, c);
  if (ab || ac) *changed = 1;                             // every writer writes the same value
}

__global__ __launch_bounds__(256) void mesh_cc_compress_kernel(int* __restrict__ label, int64_t Nv) {
  const int64_t v64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v64 >= Nv) return;
  const int v = (int)v64;
  const int r = cc_find(label, v);
  if (r != v) cc_min(label + v, r);
}

__global__ __launch_bounds__(256) void mesh_face_labels_kernel(const int* __restrict__ faces, int64_t Nf, int64_t Nv,
                                                               const int* __restrict__ label, int* __restrict__ face_label) {
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= Nf) return;
  const int a = faces[f * 3 + 0], b = faces[f * 3 + 1], c = faces[f * 3 + 2];
  face_label[f] = mesh_face_ok(a, b, c, Nv) ? label[a] : -1;
}

// ---- the float32 cross product of a face, shared by the normals and the sampler ---------------------------------------
struct MeshFace {
  float ax, ay, az;        // p_a
  float e1x, e1y, e1z;     // p_b - p_a
  float e2x, e2y, e2z;     // p_c - p_a
  float nx, ny, nz;        // e1 x e2: each component a product, a product and a difference
};

__device__ __forceinline__ MeshFace mesh_face(const float* __restrict__ vertices, int a, int b, int c) {
  const float* pa = vertices + (int64_t)a * 3;
  const float* pb = vertices + (int64_t)b * 3;
  const float* pc = vertices + (int64_t)c * 3;
  MeshFace m;
  m.ax = pa[0];
  m.ay = pa[1];
  m.az = pa[2];
  m.e1x = pb[0] - m.ax;
  m.e1y = pb[1] - m.ay;
  m.e1z = pb[2] - m.az;
  m.e2x = pc[0] - m.ax;
  m.e2y = pc[1] - m.ay;
  m.e2z = pc[2] - m.az;
  m.nx = m.e1y * m.e2z - m.e1z * m.e2y;
  m.ny = m.e1z * m.e2x - m.e1x * m.e2z;
  m.nz = m.e1x * m.e2y - m.e1y * m.e2x;
  return m;
}

__global__ __launch_bounds__(256) void mesh_vertex_normals_kernel(const float* __restrict__ vertices, int64_t Nv,
                                                                  const int* __restrict__ faces, int64_t Nf,
                                                                  const int64_t* __restrict__ offsets,
                                                                  const int64_t* __restrict__ corners,
                                                                  float* __restrict__ normals) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= Nv) return;
  const int64_t total = Nf * 3;
  int64_t at = offsets[v], end = offsets[v + 1];
  at = at < 0 ? 0 : at;
  end = end > total ? total : end;                        // a table that is not this mesh's reads nothing outside it
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (; at < end; ++at) {
    const int64_t corner = corners[at];
    if (corner < 0 || corner >= total) continue;
    const int64_t f = corner / 3;
    const int a = faces[f * 3 + 0], b = faces[f * 3 + 1], c = faces[f * 3 + 2];
    if (!mesh_face_ok(a, b, c, Nv)) continue;
    const MeshFace m = mesh_face(vertices, a, b, c);
    if (!(isfinite(m.nx) && isfinite(m.ny) && isfinite(m.nz))) continue;
    sx += (double)m.nx;
    sy += (double)m.ny;
    sz += (double)m.nz;
  }
  const double len = sqrt((sx * sx + sy * sy) + sz * sz);
  const bool ok = isfinite(len) && len > 0.0;
  normals[v * 3 + 0] = ok ? (float)(sx / len) : 0.0f;
  normals[v * 3 + 1] = ok ? (float)(sy / len) : 0.0f;
  normals[v * 3 + 2] = ok ? (float)(sz / len) : 0.0f;
}

// ---- surface sampling -------------------------------------------------------------------------------------------------
constexpr float kTwoPowMinus24 = 5.9604644775390625e-8f;
constexpr unsigned kTwoPow24 = 1u << 24;

__global__ __launch_bounds__(256) void mesh_sample_count_kernel(const float* __restrict__ vertices, int64_t Nv,
                                                                const int* __restrict__ faces, int64_t Nf, float inv,
                                                                unsigned seed, int* __restrict__ count) {
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= Nf) return;
  const int a = faces[f * 3 + 0], b = faces[f * 3 + 1], c = faces[f * 3 + 2];
  int n = 0;
  if (mesh_face_ok(a, b, c, Nv)) {
    const MeshFace m = mesh_face(vertices, a, b, c);
    const float q = (m.nx * m.nx + m.ny * m.ny) + m.nz * m.nz;
    const float area = 0.5f * sqrtf(q);
    const float x = area * inv;
    if (isfinite(x)) {
      const float u = (float)(prio_hash(prio_hash((unsigned)f ^ seed)) >> 8) * kTwoPowMinus24;
      const float t = floorf(x + u);
      n = t >= 2147483648.0f ? INT32_MAX : (t > 0.0f ? (int)t : 0);
    }
  }
  count[f] = n;
}

__global__ __launch_bounds__(256) void mesh_sample_emit_kernel(const float* __restrict__ vertices, int64_t Nv,
                                                               const int* __restrict__ faces, int64_t Nf,
                                                               const int64_t* __restrict__ incl, int64_t N, unsigned seed,
                                                               float* __restrict__ points, int* __restrict__ face_index,
                                                               float* __restrict__ bary) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= N) return;
  int64_t lo = 0, hi = Nf;                                // the first face whose inclusive sum exceeds s
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (incl[mid] > s) {
      hi = mid;
    } else {
      lo = mid + 1;
    }
  }
  float px = 0.0f, py = 0.0f, pz = 0.0f, b0 = 0.0f, b1 = 0.0f, b2 = 0.0f;
  int index = -1;
  if (lo < Nf) {                                          // (sums that are not this mesh's: the sample stays empty)
    const int64_t f = lo;
    const int64_t j = s - (f ? incl[f - 1] : 0);
    const int a = faces[f * 3 + 0], b = faces[f * 3 + 1], c = faces[f * 3 + 2];
    if (j >= 0 && mesh_face_ok(a, b, c, Nv)) {
      const unsigned h0 = prio_hash((unsigned)f ^ seed), j2 = 2u * (unsigned)j;
      unsigned i1 = prio_hash(h0 + j2 + 1u) >> 8, i2 = prio_hash(h0 + j2 + 2u) >> 8;
      if (i1 + i2 > kTwoPow24) {                          // r1 + r2 > 1, decided on the integers: both become 1 - r
        i1 = kTwoPow24 - i1;
        i2 = kTwoPow24 - i2;
      }
      const float r1 = (float)i1 * kTwoPowMinus24, r2 = (float)i2 * kTwoPowMinus24;
      const MeshFace m = mesh_face(vertices, a, b, c);
      px = m.ax + (r1 * m.e1x + r2 * m.e2x);
      py = m.ay + (r1 * m.e1y + r2 * m.e2y);
      pz = m.az + (r1 * m.e1z + r2 * m.e2z);
      b0 = (float)(kTwoPow24 - i1 - i2) * kTwoPowMinus24;
      b1 = r1;
      b2 = r2;
      index = (int)f;
    }
  }
  points[s * 3 + 0] = px;
  points[s * 3 + 1] = py;
  points[s * 3 + 2] = pz;
  face_index[s] = index;
  bary[s * 3 + 0] = b0;
  bary[s * 3 + 1] = b1;
  bary[s * 3 + 2] = b2;
}

inline bool mesh_sizes_ok(int64_t Nv, int64_t Nf) { return Nv >= 0 && Nv <= PF_MESH_OPS_MAX && Nf >= 0 && Nf <= PF_MESH_OPS_MAX; }

inline dim3 mesh_grid(int64_t n) { return dim3((unsigned)pf_cdiv(n, 256)); }

}  // namespace

extern "C" {

int pf_mesh_cc_hook(const int* faces, int64_t Nf, int64_t Nv, int* label, int* changed, void* stream) {
  PF_REQUIRE(mesh_sizes_ok(Nv, Nf));
  if (Nf == 0 || Nv == 0) return PF_OK;
  PF_REQUIRE(faces && label && changed);
  hipLaunchKernelGGL(mesh_cc_hook_kernel, mesh_grid(Nf), dim3(256), 0, (hipStream_t)stream, faces, Nf, Nv, label, changed);
  return pf_launch_status();
}

int pf_mesh_cc_compress(int* label, int64_t Nv, void* stream) {
  PF_REQUIRE(mesh_sizes_ok(Nv, 0));
  if (Nv == 0) return PF_OK;
  PF_REQUIRE(label);
  hipLaunchKernelGGL(mesh_cc_compress_kernel, mesh_grid(Nv), dim3(256), 0, (hipStream_t)stream, label, Nv);
  return pf_launch_status();
}

int pf_mesh_face_labels(const int* faces, int64_t Nf, int64_t Nv, const int* label, int* face_label, void* stream) {
  PF_REQUIRE(mesh_sizes_ok(Nv, Nf));
  if (Nf == 0) return PF_OK;
  PF_REQUIRE(faces && face_label && (label || Nv == 0));
  hipLaunchKernelGGL(mesh_face_labels_kernel, mesh_grid(Nf), dim3(256), 0, (hipStream_t)stream, faces, Nf, Nv, label,
                     face_label);
  return pf_launch_status();
}

int pf_mesh_vertex_normals_f32(const float* vertices, int64_t Nv, const int* faces, int64_t Nf, const int64_t* offsets,
                               const int64_t* corners, float* normals, void* stream) {
  PF_REQUIRE(mesh_sizes_ok(Nv, Nf));
  if (Nv == 0) return PF_OK;
  PF_REQUIRE(vertices && offsets && normals && (Nf == 0 || (faces && corners)));
  hipLaunchKernelGGL(mesh_vertex_normals_kernel, mesh_grid(Nv), dim3(256), 0, (hipStream_t)stream, vertices, Nv, faces, Nf,
                     offsets, corners, normals);
  return pf_launch_status();
}

int pf_mesh_sample_count_f32(const float* vertices, int64_t Nv, const int* faces, int64_t Nf, float inv, unsigned seed,
                             int* count, void* stream) {
  PF_REQUIRE(mesh_sizes_ok(Nv, Nf));
  if (Nf == 0) return PF_OK;
  PF_REQUIRE(faces && count && (vertices || Nv == 0));
  hipLaunchKernelGGL(mesh_sample_count_kernel, mesh_grid(Nf), dim3(256), 0, (hipStream_t)stream, vertices, Nv, faces, Nf, inv,
                     seed, count);
  return pf_launch_status();
}

int pf_mesh_sample_emit_f32(const float* vertices, int64_t Nv, const int* faces, int64_t Nf, const int64_t* inclusive,
                            int64_t N, unsigned seed, float* points, int* face_index, float* bary, void* stream) {
  PF_REQUIRE(mesh_sizes_ok(Nv, Nf) && N >= 0 && N <= PF_MESH_OPS_MAX);
  if (N == 0) return PF_OK;
  PF_REQUIRE(Nf > 0 && vertices && faces && inclusive && points && face_index && bary);
  hipLaunchKernelGGL(mesh_sample_emit_kernel, mesh_grid(N), dim3(256), 0, (hipStream_t)stream, vertices, Nv, faces, Nf,
                     inclusive, N, seed, points, face_index, bary);
  return pf_launch_status();
}

}  // extern "C"
