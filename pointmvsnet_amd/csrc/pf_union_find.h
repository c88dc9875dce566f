// Hook-and-compress connected components on one int32 array, stated once: mesh_ops.hip runs it on a mesh's vertices,
// depth_segments.hip on a depth map's pixels (inside a tile on LDS, across tile borders on the global array).
// Everything sits in an anonymous namespace: each translation unit gets its own copy and the kernels keep their names.
//
// Connected components: why this is correct on a chip whose caches are not coherent
// ---------------------------------------------------------------------------------
// `label` is a forest: label[v] = v at first (the caller's arange), v is a root while label[v] == v.  The 8 XCDs' L2s are
// not coherent with each other and a CU's L1 is never refreshed inside a launch, so a load of `label` may return a value
// that another workgroup has since replaced.  The design does not need it to be fresh:
//
//  1. EVERY store to `label` after the initialisation is a device-scope atomicMin(label[x], y) with y < x a vertex of x's
//     own connected component (a value read from `label` along a walk from x, or the other end of a face edge's walk).  So
//     label[x] <= x holds at all times, labels only fall, and every value label[x] ever held is a vertex of x's component.
//     A stale load returns such an earlier value: still a vertex of the component, still <= x.
//  2. A walk x -> label[x] -> ... therefore strictly descends and ends after at most x steps whatever it reads (the guard
//     `(unsigned)p > (unsigned)x` ends it at once on an array that is not a forest, so a foreign `label` cannot hang or
//     fault it).  Where two walks meet, their starts are in one component.
//  3. unite(u, v): walk both to ru, rv; while they differ, old = atomicMin(label[hi], lo) with hi the larger.  The atomic
//     is executed at the device's point of coherence, so `old` is the truth whatever the walks saw.  old == hi: hi was a
//     root and now hangs below lo: done.  Otherwise hi had been hooked meanwhile (or the walk's last load was stale): its
//     parent was old < hi, it is now min(old, lo), and the thread goes on with unite(old, lo).  The larger of the pair
//     strictly falls, so the loop ends after at most hi turns; it never waits for another workgroup's store -- no spinning,
//     no lock, no cooperative launch.  Launch boundaries are the only hand-off.
//  4. Let H be the graph of all pairs {x, y} with label[x] == y at any time.  By induction over x (a value that replaces
//     label[x] is either handed on to a unite of the old and the new value, or was read two H-steps below x), every H-edge
//     lies inside one tree of the forest the launch leaves.  Walks follow H-edges, a successful hook adds one between the
//     two walks' ends, so when the hook launch ends both ends of every face edge are in one tree: trees == components.
//  5. The compress launch changes no root (a root's walk ends at once), so each thread's walk ends at the true root of its
//     tree, read across the launch boundary, and label[v] becomes that root: the smallest vertex of the tree, because every
//     step of every walk descends.
//  6. A hook launch in which no face edge found two different roots executed no atomic at all: `label` was constant during
//     the launch, all its loads saw the state the previous launch left, and both ends of every edge walked to one root.
//     That round, read by the host across a launch boundary, proves completion.  With step 3 the first round does all the
//     linking and the second confirms it; the host's loop nevertheless runs until a round is clean.
//
// The same scheme inside one workgroup (CcTile): `label` is an array in LDS, which is coherent for the workgroup, so no
// load is stale and the argument above is its simple case: steps 1 to 4 with every load fresh, a barrier for the launch
// boundary.  The atomics are workgroup-scope atomics on an LDS address (ds_min_rtn_i32), not flat ones.
#pragma once

#include "pf_common.h"

namespace {

// where the forest lives: the load and the atomic minimum of each
struct CcGlobal {
  // a load that is served by the L2 at least (not by a stale L1 line); correctness does not depend on it (see above)
#if defined(__HIP__)
  static __device__ __forceinline__ int load(const int* label, int x) {
    return __hip_atomic_load(label + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  static __device__ __forceinline__ int fetch_min(int* p, int v) { return atomicMin(p, v); }
#else  // the host re-compilation of tests/hipemu (reached through eval_out.hip), whose HIP subset has neither
  static inline int load(const int* label, int x) { return __atomic_load_n(label + x, __ATOMIC_RELAXED); }
  static inline int fetch_min(int* p, int v) { return __atomic_fetch_min(p, v, __ATOMIC_RELAXED); }
#endif
};

struct CcTile {
#if defined(__HIP__)
  static __device__ __forceinline__ int load(const int* label, int x) {
    return __hip_atomic_load(label + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  static __device__ __forceinline__ int fetch_min(int* p, int v) {
    return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
#else
  static inline int load(const int* label, int x) { return __atomic_load_n(label + x, __ATOMIC_RELAXED); }
  static inline int fetch_min(int* p, int v) { return __atomic_fetch_min(p, v, __ATOMIC_RELAXED); }
#endif
};

// the end of the walk from x, with path halving: label[x] = min(label[x], label[label[x]]) on the way
template <class M>
__device__ __forceinline__ int cc_find_in(int* __restrict__ label, int x) {
  int p = M::load(label, x);
  while (p != x) {
    if ((unsigned)p > (unsigned)x) break;                 // not a forest (a foreign array): x counts as a root
    const int g = M::load(label, p);
    if (g != p && (unsigned)g < (unsigned)p) M::fetch_min(label + x, g);
    x = p;
    p = g;
  }
  return x;
}

// true iff the two walks ended at different roots (the round's changed-flag)
template <class M>
__device__ __forceinline__ bool cc_unite_in(int* __restrict__ label, int u, int v) {
  int ru = cc_find_in<M>(label, u), rv = cc_find_in<M>(label, v);
  if (ru == rv) return false;
  while (ru != rv) {
    const int hi = ru > rv ? ru : rv, lo = ru > rv ? rv : ru;
    const int old = M::fetch_min(label + hi, lo);
    if (old == hi || (unsigned)old > (unsigned)hi) break; // hi was a root and hangs below lo now (or: not a forest)
    ru = cc_find_in<M>(label, old);                       // hi's parent was old: go on with (old, lo), both below hi
    rv = cc_find_in<M>(label, lo);
  }
  return true;
}

__device__ __forceinline__ int cc_load(const int* label, int x) { return CcGlobal::load(label, x); }
__device__ __forceinline__ int cc_min(int* p, int v) { return CcGlobal::fetch_min(p, v); }
__device__ __forceinline__ int cc_find(int* __restrict__ label, int x) { return cc_find_in<CcGlobal>(label, x); }
__device__ __forceinline__ bool cc_unite(int* __restrict__ label, int u, int v) { return cc_unite_in<CcGlobal>(label, u, v); }

}  // namespace
