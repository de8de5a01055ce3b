// pointnet_pool.hip -- PointNet's per-point MLP (3 -> 64 -> 128 -> 1024) and its max over the points as ONE pass
// on the fp32 matrix cores (gfx950).  The hot path of the Frechet Point-cloud Distance (sparenet_amd/Frechet).
//
// Reference: STN3d.forward and PointNetfeat.forward of Frechet/pointnet.py: three 1x1 convolutions with batch norm,
// then torch.max over the points.  The stock layers write a [B, 1024, N] fp32 activation (2 GB at B = 30,
// N = 16384) and read it back to take 1024 maxima per cloud.  Here nothing wider than the input leaves the chip:
//
//   workgroup = one cloud x kTile = 128 points, 4 waves;  points are the ROWS of every product, channels the
//   columns, so in the 32x32 result layout a lane holds ONE channel and 16 points per accumulator;
//   layer 1 (K = 3) is computed where it is consumed: the A operand of layer 2's step s in lane l is
//   h1[point l & 31][channel 2 s + (l >> 5)], three fmaf and a max in that lane -- h1 never exists in memory;
//   layer 2 (K = 64): wave w owns channels 32 w .. 32 w + 31 for all 128 points = 4 accumulators of
//   v_mfma_f32_32x32x2_f32, started at the bias; ReLU, then the tile goes to LDS as h2[channel][point] (64.5 KB,
//   rows padded by 4 floats), which is exactly the A operand layout of layer 3 (unit stride along the points);
//   layer 3 (K = 128): wave w owns output channels 256 w .. 256 w + 255, in 8 passes of 32 channels x 128 points
//   (4 accumulators); the B operand is read straight from the TRANSPOSED weights (workspace, written by a small
//   kernel in front: lane l reads W3t[2 s + (l >> 5)][channel], unit stride), so a workgroup reads W3 once;
//   the maximum over the tile's points is 63 v_max in the lane's registers and one exchange between lane halves;
//   the per-tile maxima go to the workspace and a second small kernel takes the maximum over the tiles, adds the
//   bias and applies the ReLU (both monotone: bit-identical to applying them per point).
// A short last tile repeats the cloud's last point.  No workgroup waits for another; plain stream-ordered launches.
// Numeric contract: every product is a k-ordered fp32 fmaf chain (layer 1 and 2 start at the bias, layer 3 at 0
// with the bias added once after the maximum); x . trans is fmaf(x2, t2j, fmaf(x1, t1j, x0 * t0j)).
#include "common.hpp"

namespace {

typedef float f16v __attribute__((ext_vector_type(16)));
typedef float f4v __attribute__((ext_vector_type(4)));

constexpr int kTile = 128;        // points per workgroup
constexpr int kLd = kTile + 4;    // h2 row length in LDS (floats): 16-byte aligned rows, staggered banks
constexpr int kC1 = 64, kC2 = 128, kC3 = 1024;
constexpr size_t kLdsBytes = (size_t)(kC2 * kLd + kC1 * 4) * 4;

// W2 [128,64] -> w2t [64][128], W3 [1024,128] -> w3t [128][1024]
__global__ __launch_bounds__(256) void pn_transpose_kernel(const float *__restrict__ w2, const float *__restrict__ w3,
                                                           float *__restrict__ w2t, float *__restrict__ w3t) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;  // index into the OUTPUT (coalesced stores)
  if (e < kC2 * kC3) {
    const int k = e / kC3, c = e - k * kC3;
    w3t[e] = w3[c * kC2 + k];
  }
  if (e < kC1 * kC2) {
    const int k = e / kC2, c = e - k * kC2;
    w2t[e] = w2[c * kC1 + k];
  }
}

__global__ __launch_bounds__(256, 2) void pn_pool_kernel(const float *__restrict__ xyz, const float *__restrict__ trans,
                                                         const float *__restrict__ w1, const float *__restrict__ b1,
                                                         const float *__restrict__ w2t, const float *__restrict__ b2,
                                                         const float *__restrict__ w3t, int n, int ntiles,
                                                         float *__restrict__ partial) {
  extern __shared__ float smem[];
  float *h2s = smem;                  // [kC2][kLd]
  float *w1s = smem + kC2 * kLd;      // [kC1][4] = {w1[k][0..2], b1[k]}
  const int cloud = blockIdx.x / ntiles, tile = blockIdx.x - cloud * ntiles;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int h = lane >> 5, c31 = lane & 31;

  if (tid < kC1) {
    f4v v = {w1[tid * 3 + 0], w1[tid * 3 + 1], w1[tid * 3 + 2], b1[tid]};
    *reinterpret_cast<f4v *>(w1s + tid * 4) = v;
  }

  // the lane's four points (rows c31 of the four 32-point blocks), transformed
  float px[4], py[4], pz[4];
  {
    float t[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
    if (trans) {
#pragma unroll
      for (int i = 0; i < 9; ++i) t[i] = trans[(size_t)cloud * 9 + i];
    }
    const float *xb = xyz + (size_t)cloud * n * 3;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int p = tile * kTile + 32 * i + c31;
      p = p < n ? p : n - 1;  // a short last tile repeats the last point: a maximum cannot change
      const float x0 = xb[(size_t)p * 3 + 0], x1 = xb[(size_t)p * 3 + 1], x2 = xb[(size_t)p * 3 + 2];
      if (trans) {
        px[i] = fmaf(x2, t[6], fmaf(x1, t[3], x0 * t[0]));
        py[i] = fmaf(x2, t[7], fmaf(x1, t[4], x0 * t[1]));
        pz[i] = fmaf(x2, t[8], fmaf(x1, t[5], x0 * t[2]));
      } else {
        px[i] = x0;
        py[i] = x1;
        pz[i] = x2;
      }
    }
  }
  __syncthreads();

  // ---- layer 2: h2[32 wave + c31][point] = relu(b2 + sum_k h1[point][k] W2[ch][k]), h1 made in the lane
  {
    const int ch = 32 * wave + c31;
    const float bias = b2[ch];
    f16v acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][r] = bias;
    const float *bp = w2t + ch;
#pragma unroll 4
    for (int s = 0; s < kC1 / 2; ++s) {
      const int k = 2 * s + h;
      const f4v w = *reinterpret_cast<const f4v *>(w1s + k * 4);
      const float bv = bp[k * kC2];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float a = fmaxf(fmaf(w.z, pz[i], fmaf(w.y, py[i], fmaf(w.x, px[i], w.w))), 0.f);
        acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv, acc[i], 0, 0, 0);
      }
    }
    // result register 4 a + q of block i = point 32 i + 8 a + 4 h + q, channel ch
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        f4v v = {fmaxf(acc[i][4 * a + 0], 0.f), fmaxf(acc[i][4 * a + 1], 0.f), fmaxf(acc[i][4 * a + 2], 0.f),
                 fmaxf(acc[i][4 * a + 3], 0.f)};
        *reinterpret_cast<f4v *>(h2s + ch * kLd + 32 * i + 8 * a + 4 * h) = v;
      }
  }
  __syncthreads();

  // ---- layer 3: 8 passes of 32 output channels x 128 points, maximum over the points
  float *dst = partial + ((size_t)cloud * ntiles + tile) * kC3;
  const float *ap = h2s + h * kLd + c31;
  for (int pass = 0; pass < 8; ++pass) {
    const int ch = 256 * wave + 32 * pass + c31;
    const float *bp = w3t + (size_t)h * kC3 + ch;
    f16v acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
#pragma unroll 8
    for (int s = 0; s < kC2 / 2; ++s) {
      const float bv = bp[(size_t)2 * s * kC3];
      const float *as = ap + 2 * s * kLd;
      const float a0 = as[0], a1 = as[32], a2 = as[64], a3 = as[96];
      acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bv, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, bv, acc[1], 0, 0, 0);
      acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a2, bv, acc[2], 0, 0, 0);
      acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(a3, bv, acc[3], 0, 0, 0);
    }
    float m = acc[0][0];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) m = fmaxf(m, acc[i][r]);
    m = fmaxf(m, __shfl_xor(m, 32));
    if (h == 0) dst[ch] = m;
  }
}

// out[cloud][j] = act(b3[j] + max over the tiles of partial[cloud][tile][j]); block = 64 channels x 4 tile strides
__global__ __launch_bounds__(256) void pn_reduce_kernel(const float *__restrict__ partial, const float *__restrict__ b3,
                                                        int ntiles, int relu_last, float *__restrict__ out) {
  __shared__ float red[4][64];
  const int cloud = blockIdx.x >> 4, j = (blockIdx.x & 15) * 64 + (threadIdx.x & 63), q = threadIdx.x >> 6;
  const float *src = partial + (size_t)cloud * ntiles * kC3 + j;
  float m = src[0];
  for (int t = q; t < ntiles; t += 4) m = fmaxf(m, src[(size_t)t * kC3]);
  red[q][threadIdx.x & 63] = m;
  __syncthreads();
  if (q == 0) {
    m = fmaxf(fmaxf(red[0][threadIdx.x], red[1][threadIdx.x]), fmaxf(red[2][threadIdx.x], red[3][threadIdx.x]));
    m = m + b3[j];
    out[(size_t)cloud * kC3 + j] = relu_last ? fmaxf(m, 0.f) : m;
  }
}

inline int pn_tiles(int n) { return (n + kTile - 1) / kTile; }

struct PoolWs {  // the workspace
  float *w3t, *w2t;  // the transposed weights of layers 3 and 2
  float *partial;    // [b, tiles, kC3] per-tile maxima
};
PoolWs pool_layout(sn::Carver &c, int b, int n) {
  return {c.take<float>((size_t)kC2 * kC3 * 4), c.take<float>((size_t)kC1 * kC2 * 4),
          c.take256<float>((size_t)b * pn_tiles(n) * kC3 * 4)};
}

}  // namespace

extern "C" size_t sn_pointnet_pool_workspace_bytes(int b, int n) {
  if (b < 1 || n < 1 || n > (1 << 20)) return 0;
  return sn::layout_bytes(pool_layout, b, n);
}

extern "C" int sn_pointnet_pool_forward(const float *xyz, const float *trans, const float *w1, const float *b1,
                                        const float *w2, const float *b2, const float *w3, const float *b3,
                                        int relu_last, int b, int n, float *out, void *workspace,
                                        size_t workspace_bytes, void *stream) {
  SN_REQUIRE(xyz && w1 && b1 && w2 && b2 && w3 && b3 && out && workspace, "sn_pointnet_pool_forward: null pointer");
  SN_REQUIRE(b >= 1, "sn_pointnet_pool_forward: need b >= 1 (got %d)", b);
  SN_REQUIRE(n >= 1 && n <= (1 << 20), "sn_pointnet_pool_forward: need 1 <= n <= 2^20 (got %d)", n);
  const int ntiles = pn_tiles(n);
  SN_REQUIRE((long long)b * ntiles <= 0x7fffffffLL && b <= (1 << 26),
             "sn_pointnet_pool_forward: batch too large (b = %d, %d tiles per cloud)", b, ntiles);
  sn::Carver carver(workspace);
  const PoolWs w = pool_layout(carver, b, n);
  SN_REQUIRE(workspace_bytes >= carver.bytes(), "sn_pointnet_pool_forward: workspace too small (%zu bytes, need %zu)",
             workspace_bytes, carver.bytes());
  hipStream_t s = sn::as_stream(stream);
  pn_transpose_kernel<<<kC2 * kC3 / 256, 256, 0, s>>>(w2, w3, w.w2t, w.w3t);
  SN_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(pn_pool_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)kLdsBytes));  // per call: the attribute belongs to the current device
  SN_TIMED("pointnet_pool", s,
           (pn_pool_kernel<<<(unsigned)(b * ntiles), 256, kLdsBytes, s>>>(xyz, trans, w1, b1, w.w2t, b2, w.w3t, n,
                                                                         ntiles, w.partial)));
  pn_reduce_kernel<<<(unsigned)b * (kC3 / 64), 256, 0, s>>>(w.partial, b3, ntiles, relu_last, out);
  return sn::launch_status("sn_pointnet_pool_forward");
}
