// What fusion.hip and geo_filter.hip share: the pixel tiling and the camera maps of pointmvsnet_amd/camera_maps.py.
//   view_maps (V, PF_FUSE_VIEW_FLOATS): A = R^-1 K^-1 (row-major 3x3), then C = -R^-1 t:  X = (A (x+.5, y+.5, 1)) d + C
//   a pair row i -> j (PF_FUSE_PAIR_FLOATS): M = K_j R_j R_i^-1 K_i^-1 (3x3), T = K_j (t_j - R_j R_i^-1 t_i), then
//     fb = K_j[0][0] |C_i - C_j| (fusion.hip alone reads it) and padding:  q = (M (x+.5, y+.5, 1)) d + T
#pragma once                       // a build without __HIP__ meets both files in one unit, through eval_out.hip
#include "pf_common.h"

constexpr int kPfTile = 16;        // kPfTile x kPfTile pixels per block, one thread each; blockIdx.z is the view
__device__ __forceinline__ void pf_tile_pixel(int& x, int& y, int& view) {
  x = blockIdx.x * kPfTile + (threadIdx.x & (kPfTile - 1));
  y = blockIdx.y * kPfTile + (threadIdx.x / kPfTile);
  view = blockIdx.z;
}

// (m[0..8] (px, py, 1)) d + m[9..11] of a view or pair row m
__device__ __forceinline__ void pf_apply_map(const float* __restrict__ m, float px, float py, float d, float& X, float& Y,
                                             float& Z) {
  X = (m[0] * px + m[1] * py + m[2]) * d + m[9];
  Y = (m[3] * px + m[4] * py + m[5]) * d + m[10];
  Z = (m[6] * px + m[7] * py + m[8]) * d + m[11];
}
