// The 32-bit integer hash shared by the cloud thinning's priorities (cloud_eval.hip) and the surface sampler's random
// numbers (mesh_ops.hip): a bijection of the 32-bit integers (two xor-shift-multiply rounds), so distinct inputs never
// collide.  All arithmetic is mod 2^32.
#pragma once

#include "pf_common.h"

__device__ __forceinline__ unsigned prio_hash(unsigned x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}
