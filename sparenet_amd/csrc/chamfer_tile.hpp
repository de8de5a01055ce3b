// chamfer_tile.hpp -- what the brute-force Chamfer kernels share: the training kernel with its arg-min (chamfer.hip)
// and the set-level kernel that keeps only the minimum (set_chamfer.hip).  The distance expression, the min3 tree's
// element and the chunk-SoA layout of a target tile in LDS; the loops stay in their files.
//
// d = (dx*dx + dy*dy) + dz*dz with dx = t.x - q.x: three separately rounded products and two rounded sums (no FMA).
// Both kernels must give the same fp32 value for a pair, bit for bit, so there is one statement of it.
//
// Tile.  kTile targets per LDS tile, laid out in chunks of kChunk: x[8] y[8] z[8] per chunk = 6 float4, read with
// wave-uniform ds_read_b128 (broadcast, conflict free).  tile_slot(k, comp) is the float index of component comp of
// the tile's target k.
#pragma once
#include <hip/hip_runtime.h>

namespace sn {
namespace ct {

typedef float f2 __attribute__((ext_vector_type(2)));

constexpr int kThreads = 256;
constexpr int kChunk = 8;                    // targets per chunk
constexpr int kTile = 1024;                  // targets per LDS tile
constexpr int kTileF4 = kTile / kChunk * 6;  // float4 slots per tile

__device__ __forceinline__ int tile_slot(int k, int comp) { return (k >> 3) * 24 + comp * 8 + (k & 7); }

__device__ __forceinline__ float min3(float a, float b, float c) {
  return __builtin_fminf(__builtin_fminf(a, b), c);
}

// d = (dx*dx + dy*dy) + dz*dz, two queries at once, no contraction
__device__ __forceinline__ f2 dist2(float tx, float ty, float tz, f2 qx, f2 qy, f2 qz) {
#pragma clang fp contract(off)
  const f2 dx = tx - qx;
  const f2 dy = ty - qy;
  const f2 dz = tz - qz;
  const f2 xx = dx * dx;
  const f2 yy = dy * dy;
  const f2 zz = dz * dz;
  const f2 s = xx + yy;
  return s + zz;
}

__device__ __forceinline__ float dist1(float tx, float ty, float tz, float qx, float qy, float qz) {
#pragma clang fp contract(off)
  const float dx = tx - qx;
  const float dy = ty - qy;
  const float dz = tz - qz;
  const float xx = dx * dx;
  const float yy = dy * dy;
  const float zz = dz * dz;
  const float s = xx + yy;
  return s + zz;
}

}  // namespace ct
}  // namespace sn
