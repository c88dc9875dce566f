// Mesh simplification by vertex clustering with quadric placement (specification: pointmvsnet_amd/mesh_simplify.py,
// include/pointflow_hip.h).  vertices (Nv, 3) float32, faces (Nf, 3) int32, cluster (Nv) int64 = the cluster of each vertex
// (voxel_downsample's inverse map), M clusters.  Every kernel checks an index that comes from the caller (a face's vertex, a
// vertex's cluster, a list entry, a corner, a todo row) before it forms an address from it: no input faults.  No LDS, no
// per-thread array, no scratch, no atomics: every output element has one writer and every sum one order.
//
//   mesh_simplify_faces       one thread per face: the cluster triple in the face's own rotation, the collapsed flag (two of
//                             the three clusters equal, or a face that is skipped) and the ascending triple for the
//                             duplicate test.
//   mesh_simplify_keep_first  one thread per slot of the surviving faces sorted (stably) by their ascending triple: a face is
//                             kept iff its triple differs from the slot before it, i.e. it has the lowest face index of its run.
//   mesh_quadric_thread       one thread per cluster whose corner list is shorter than `threshold`: the nine sums in
//                             ascending list order, then the solve.
//   mesh_quadric_wave         one wave per listed cluster (the long lists): lane l adds the list entries l, l + 64, .. in that
//                             order, the 64 partial sums are combined by the xor butterfly 32, 16, .. 1 (every lane ends with
//                             the same bits: IEEE addition commutes), then lane 0 solves.
//
// Which kernel a cluster gets is a function of its list length alone, and each has one order of summation, so the positions
// are a pure function of the input.
#include "pf_common.h"

#include <math.h>

namespace {

__device__ __forceinline__ bool simplify_face_ok(int a, int b, int c, int64_t Nv) {
  return a >= 0 && a < Nv && b >= 0 && b < Nv && c >= 0 && c < Nv;
}

__global__ __launch_bounds__(256) void mesh_simplify_faces_kernel(const int* __restrict__ faces, int64_t Nf, int64_t Nv,
                                                                  const int64_t* __restrict__ cluster, int64_t M,
                                                                  int* __restrict__ triple, int* __restrict__ ascending,
                                                                  unsigned char* __restrict__ collapsed) {
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= Nf) return;
  const int a = faces[f * 3 + 0], b = faces[f * 3 + 1], c = faces[f * 3 + 2];
  int ca = -1, cb = -1, cc = -1;
  bool ok = simplify_face_ok(a, b, c, Nv);
  if (ok) {
    const int64_t ka = cluster[a], kb = cluster[b], kc = cluster[c];
    ok = ka >= 0 && ka < M && kb >= 0 && kb < M && kc >= 0 && kc < M;
    if (ok) {
      ca = (int)ka;
      cb = (int)kb;
      cc = (int)kc;
    }
  }
  triple[f * 3 + 0] = ca;
  triple[f * 3 + 1] = cb;
  triple[f * 3 + 2] = cc;
  const int lo = min(ca, min(cb, cc)), hi = max(ca, max(cb, cc));
  const int mid = max(min(ca, cb), min(max(ca, cb), cc));                // the median of three
  ascending[f * 3 + 0] = lo;
  ascending[f * 3 + 1] = mid;
  ascending[f * 3 + 2] = hi;
  collapsed[f] = (!ok || ca == cb || cb == cc || ca == cc) ? 1 : 0;
}

__global__ __launch_bounds__(256) void mesh_simplify_keep_first_kernel(const int* __restrict__ ascending, int64_t Nf,
                                                                       const int64_t* __restrict__ sorted_faces, int64_t K,
                                                                       unsigned char* __restrict__ keep) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= K) return;
  const int64_t f = sorted_faces[t];
  if (f < 0 || f >= Nf) return;
  bool first = true;
  if (t > 0) {
    const int64_t g = sorted_faces[t - 1];
    if (g >= 0 && g < Nf) {
      first = ascending[f * 3 + 0] != ascending[g * 3 + 0] || ascending[f * 3 + 1] != ascending[g * 3 + 1] ||
              ascending[f * 3 + 2] != ascending[g * 3 + 2];
    }
  }
  keep[f] = first ? 1 : 0;
}

// ---- the quadric of a cluster: A (symmetric, six entries) and b, nine float64 sums in named scalars -----------------------
struct Quadric {
  double a00, a01, a02, a11, a12, a22;
  double b0, b1, b2;
};

__device__ __forceinline__ Quadric quadric_zero() { return Quadric{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}; }

// The term of list entry `at`: the face of that corner, in coordinates relative to the cluster's mean (mx, my, mz).
__device__ __forceinline__ void quadric_add(Quadric& q, const float* __restrict__ vertices, int64_t Nv,
                                            const int* __restrict__ faces, int64_t total,
                                            const int64_t* __restrict__ corners, int64_t at, double mx, double my, double mz) {
  const int64_t corner = corners[at];
  if (corner < 0 || corner >= total) return;
  const int64_t f = corner / 3;
  const int a = faces[f * 3 + 0], b = faces[f * 3 + 1], c = faces[f * 3 + 2];
  if (!simplify_face_ok(a, b, c, Nv)) return;
  const float* pa = vertices + (int64_t)a * 3;
  const float* pb = vertices + (int64_t)b * 3;
  const float* pc = vertices + (int64_t)c * 3;
  const double ax = (double)pa[0] - mx, ay = (double)pa[1] - my, az = (double)pa[2] - mz;
  const double bx = (double)pb[0] - mx, by = (double)pb[1] - my, bz = (double)pb[2] - mz;
  const double cx = (double)pc[0] - mx, cy = (double)pc[1] - my, cz = (double)pc[2] - mz;
  const double e1x = bx - ax, e1y = by - ay, e1z = bz - az;
  const double e2x = cx - ax, e2y = cy - ay, e2z = cz - az;
  const double nx = e1y * e2z - e1z * e2y;
  const double ny = e1z * e2x - e1x * e2z;
  const double nz = e1x * e2y - e1y * e2x;
  if (!(isfinite(nx) && isfinite(ny) && isfinite(nz))) return;
  const double d = -((nx * ax + ny * ay) + nz * az);
  q.a00 += nx * nx;
  q.a01 += nx * ny;
  q.a02 += nx * nz;
  q.a11 += ny * ny;
  q.a12 += ny * nz;
  q.a22 += nz * nz;
  q.b0 += d * nx;
  q.b1 += d * ny;
  q.b2 += d * nz;
}

// (A + reg * t / 3 * I) x = -b by the root-free Cholesky factorisation M = L D L^T, in the order of mesh_simplify.py.
__device__ __forceinline__ void quadric_place(const Quadric& q, double mx, double my, double mz, float cell, double reg,
                                              float* __restrict__ position, unsigned char* __restrict__ fallback) {
  const double t = (q.a00 + q.a11) + q.a22;
  double x0 = 0.0, x1 = 0.0, x2 = 0.0;
  bool fell = false;
  if (isfinite(t) && t > 0.0) {
    const double lam = (reg * t) / 3.0;
    const double m00 = q.a00 + lam, m11 = q.a11 + lam, m22 = q.a22 + lam;
    const double l10 = q.a01 / m00, l20 = q.a02 / m00;
    const double d1 = m11 - l10 * q.a01;
    const double u21 = q.a12 - l20 * q.a01;
    const double l21 = u21 / d1;
    const double d2 = m22 - (l20 * q.a02 + l21 * u21);
    const double r0 = -q.b0, r1 = -q.b1, r2 = -q.b2;
    const double y0 = r0;                                   // L y = r
    const double y1 = r1 - l10 * y0;
    const double y2 = r2 - (l20 * y0 + l21 * y1);
    x2 = y2 / d2;                                           // D L^T x = y
    x1 = y1 / d1 - l21 * x2;
    x0 = y0 / m00 - (l10 * x1 + l20 * x2);
    const double limit = (double)cell;
    fell = !(fabs(x0) <= limit && fabs(x1) <= limit && fabs(x2) <= limit);     // a NaN falls back as well
    if (fell) {
      x0 = 0.0;
      x1 = 0.0;
      x2 = 0.0;
    }
  }
  position[0] = (float)(mx + x0);
  position[1] = (float)(my + x1);
  position[2] = (float)(mz + x2);
  *fallback = fell ? 1 : 0;
}

__global__ __launch_bounds__(256) void mesh_quadric_thread_kernel(const float* __restrict__ vertices, int64_t Nv,
                                                                  const int* __restrict__ faces, int64_t Nf,
                                                                  const int64_t* __restrict__ offsets,
                                                                  const int64_t* __restrict__ corners,
                                                                  const float* __restrict__ means, int64_t M, float cell,
                                                                  double reg, int64_t threshold,
                                                                  float* __restrict__ positions,
                                                                  unsigned char* __restrict__ fallback) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= M) return;
  const int64_t total = Nf * 3;
  const int64_t at0 = min(max(offsets[s], (int64_t)0), total), at1 = min(max(offsets[s + 1], at0), total);
  if (at1 - at0 >= threshold) return;                      // a long list: the wave kernel's
  const double mx = (double)means[s * 3 + 0], my = (double)means[s * 3 + 1], mz = (double)means[s * 3 + 2];
  Quadric q = quadric_zero();
  for (int64_t at = at0; at < at1; ++at) quadric_add(q, vertices, Nv, faces, total, corners, at, mx, my, mz);
  quadric_place(q, mx, my, mz, cell, reg, positions + s * 3, fallback + s);
}

__global__ __launch_bounds__(256) void mesh_quadric_wave_kernel(const float* __restrict__ vertices, int64_t Nv,
                                                                const int* __restrict__ faces, int64_t Nf,
                                                                const int64_t* __restrict__ offsets,
                                                                const int64_t* __restrict__ corners,
                                                                const float* __restrict__ means, int64_t M, float cell,
                                                                double reg, const int64_t* __restrict__ todo, int64_t ntodo,
                                                                float* __restrict__ positions,
                                                                unsigned char* __restrict__ fallback) {
  const int64_t w = ((int64_t)blockIdx.x * 256 + threadIdx.x) / PF_WAVE;     // uniform over the wave
  const int lane = threadIdx.x & (PF_WAVE - 1);
  if (w >= ntodo) return;
  const int64_t s = todo[w];
  if (s < 0 || s >= M) return;
  const int64_t total = Nf * 3;
  const int64_t at0 = min(max(offsets[s], (int64_t)0), total), at1 = min(max(offsets[s + 1], at0), total);
  const double mx = (double)means[s * 3 + 0], my = (double)means[s * 3 + 1], mz = (double)means[s * 3 + 2];
  Quadric q = quadric_zero();
  for (int64_t at = at0 + lane; at < at1; at += PF_WAVE) quadric_add(q, vertices, Nv, faces, total, corners, at, mx, my, mz);
#pragma unroll
  for (int off = PF_WAVE / 2; off >= 1; off >>= 1) {
    q.a00 += __shfl_xor(q.a00, off);
    q.a01 += __shfl_xor(q.a01, off);
    q.a02 += __shfl_xor(q.a02, off);
    q.a11 += __shfl_xor(q.a11, off);
    q.a12 += __shfl_xor(q.a12, off);
    q.a22 += __shfl_xor(q.a22, off);
    q.b0 += __shfl_xor(q.b0, off);
    q.b1 += __shfl_xor(q.b1, off);
    q.b2 += __shfl_xor(q.b2, off);
  }
  if (lane == 0) quadric_place(q, mx, my, mz, cell, reg, positions + s * 3, fallback + s);
}

inline bool simplify_sizes_ok(int64_t Nv, int64_t Nf, int64_t M) {
  return Nv >= 0 && Nv <= PF_MESH_OPS_MAX && Nf >= 0 && Nf <= PF_MESH_OPS_MAX && M >= 0 && M <= Nv;
}

inline bool quadric_args_ok(float cell, double reg) {
  return cell > 0.0f && isfinite(cell) && reg >= PF_MESH_SIMPLIFY_MIN_REG && reg <= 1.0;
}

inline dim3 simplify_grid(int64_t n) { return dim3((unsigned)pf_cdiv(n, 256)); }

}  // namespace

extern "C" {

int pf_mesh_simplify_faces(const int* faces, int64_t Nf, int64_t Nv, const int64_t* cluster, int64_t M, int* triple,
                           int* ascending, unsigned char* collapsed, void* stream) {
  PF_REQUIRE(simplify_sizes_ok(Nv, Nf, M));
  if (Nf == 0) return PF_OK;
  PF_REQUIRE(faces && triple && ascending && collapsed && (cluster || Nv == 0));
  hipLaunchKernelGGL(mesh_simplify_faces_kernel, simplify_grid(Nf), dim3(256), 0, (hipStream_t)stream, faces, Nf, Nv, cluster,
                     M, triple, ascending, collapsed);
  return pf_launch_status();
}

int pf_mesh_simplify_keep_first(const int* ascending, int64_t Nf, const int64_t* sorted_faces, int64_t K,
                                unsigned char* keep, void* stream) {
  PF_REQUIRE(Nf >= 0 && Nf <= PF_MESH_OPS_MAX && K >= 0 && K <= Nf);
  if (K == 0) return PF_OK;
  PF_REQUIRE(ascending && sorted_faces && keep);
  hipLaunchKernelGGL(mesh_simplify_keep_first_kernel, simplify_grid(K), dim3(256), 0, (hipStream_t)stream, ascending, Nf,
                     sorted_faces, K, keep);
  return pf_launch_status();
}

int pf_mesh_quadric_thread_f64(const float* vertices, int64_t Nv, const int* faces, int64_t Nf, const int64_t* offsets,
                               const int64_t* corners, const float* means, int64_t M, float cell, double regularisation,
                               int64_t threshold, float* positions, unsigned char* fallback, void* stream) {
  PF_REQUIRE(simplify_sizes_ok(Nv, Nf, M) && quadric_args_ok(cell, regularisation) && threshold >= 0);
  if (M == 0) return PF_OK;
  PF_REQUIRE(vertices && offsets && means && positions && fallback && (Nf == 0 || (faces && corners)));
  hipLaunchKernelGGL(mesh_quadric_thread_kernel, simplify_grid(M), dim3(256), 0, (hipStream_t)stream, vertices, Nv, faces, Nf,
                     offsets, corners, means, M, cell, regularisation, threshold, positions, fallback);
  return pf_launch_status();
}

int pf_mesh_quadric_wave_f64(const float* vertices, int64_t Nv, const int* faces, int64_t Nf, const int64_t* offsets,
                             const int64_t* corners, const float* means, int64_t M, float cell, double regularisation,
                             const int64_t* todo, int64_t ntodo, float* positions, unsigned char* fallback, void* stream) {
  PF_REQUIRE(simplify_sizes_ok(Nv, Nf, M) && quadric_args_ok(cell, regularisation) && ntodo >= 0 && ntodo <= M);
  if (ntodo == 0) return PF_OK;
  PF_REQUIRE(vertices && offsets && means && positions && fallback && todo && (Nf == 0 || (faces && corners)));
  hipLaunchKernelGGL(mesh_quadric_wave_kernel, simplify_grid(ntodo * PF_WAVE), dim3(256), 0, (hipStream_t)stream, vertices, Nv,
                     faces, Nf, offsets, corners, means, M, cell, regularisation, todo, ntodo, positions, fallback);
  return pf_launch_status();
}

}  // extern "C"
