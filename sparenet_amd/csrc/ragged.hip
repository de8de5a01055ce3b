// ragged.hip -- from the reference's padding convention to a ragged batch and back (sn_pad_compact /
// sn_pad_scatter_rows; the ragged-batch contract is in include/sparenet_hip.h).
//
// The reference marks padding by value: a row whose coordinates sum to zero (cuda/chamfer_dist/__init__.py:27-31,
// cuda/gridding/__init__.py:41-47).  The ragged ops take padding by position: the first lengths[b] rows of a cloud are
// its points.  sn_pad_compact moves the rows that are points to the front, in their order, and says where each came
// from; sn_pad_scatter_rows takes per-row values (gradients) back to the original places.
#include "block_scan.hpp"
#include "common.hpp"

namespace {

constexpr int kScanThreads = 1024;

// One workgroup per cloud, chunks of 1024 rows in ascending order with the running count carried in LDS: a stable
// partition by one prefix scan, for any n, and no workgroup waits for another.  The chunk protocol is the one of
// sn::BlockScan, written out: on sn::BlockScan this kernel measured 2 - 4 % slower (21.7 / 22.0 us against 21.3 / 20.9
// at 32 x 16384 rows, same registers and LDS), and the cause was not found.
__global__ __launch_bounds__(kScanThreads) void pad_compact_kernel(const float *__restrict__ xyz, int n,
                                                                   float *__restrict__ packed,
                                                                   int *__restrict__ lengths, int *__restrict__ src) {
  __shared__ int s_wave[kScanThreads / 64];
  __shared__ int s_carry;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t o = (size_t)blockIdx.x * n;
  if (tid == 0) s_carry = 0;
  __syncthreads();
  for (int base = 0; base < n; base += kScanThreads) {
    const int i = base + tid;
    float x = 0.f, y = 0.f, z = 0.f;
    if (i < n) {
      const float *p = xyz + (o + i) * 3;
      x = p[0];
      y = p[1];
      z = p[2];
    }
    // the rule of sn_gridding_forward_padded, in its order; a NaN sum is not zero: the row is a point
    const int keep = i < n && !((x + y) + z == 0.f);
    const int incl = sn::wave_inclusive_scan(keep);
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int before = s_carry;
    for (int w = 0; w < wave; ++w) before += s_wave[w];
    if (keep) {
      const size_t pos = o + before + incl - 1;
      packed[pos * 3 + 0] = x;
      packed[pos * 3 + 1] = y;
      packed[pos * 3 + 2] = z;
      src[pos] = i;
    }
    __syncthreads();
    if (tid == kScanThreads - 1) s_carry = before + incl;
    __syncthreads();
  }
  const int len = s_carry;
  if (tid == 0) lengths[blockIdx.x] = len;
  for (int i = len + tid; i < n; i += kScanThreads) {  // the tail: defined values, never read as points
    packed[(o + i) * 3 + 0] = 0.f;
    packed[(o + i) * 3 + 1] = 0.f;
    packed[(o + i) * 3 + 2] = 0.f;
    src[o + i] = -1;
  }
}

// out is zero on entry; packed row p of cloud b goes to row src[b, p]
__global__ __launch_bounds__(256) void pad_scatter_rows_kernel(const float *__restrict__ rows,
                                                               const int *__restrict__ src, long total, int n, int c,
                                                               float *__restrict__ out) {
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const long r = e / c;  // row b * n + p
    const int ch = (int)(e - r * c);
    const int s = src[r];
    if (s < 0 || s >= n) continue;
    out[((r / n) * n + s) * c + ch] = rows[e];
  }
}

}  // namespace

extern "C" int sn_pad_compact(const float *xyz, int b, int n, float *packed, int *lengths, int *src, void *stream) {
  SN_REQUIRE(xyz && packed && lengths && src, "sn_pad_compact: null pointer");
  SN_REQUIRE(xyz != packed, "sn_pad_compact: packed must not alias xyz");
  SN_REQUIRE(b >= 1 && b <= 65535 && n >= 1 && (long)b * n < (1L << 29),
             "sn_pad_compact: need 1 <= b <= 65535, n >= 1, b * n < 2^29 (got b=%d, n=%d)", b, n);
  pad_compact_kernel<<<b, kScanThreads, 0, sn::as_stream(stream)>>>(xyz, n, packed, lengths, src);
  return sn::launch_status("sn_pad_compact");
}

extern "C" int sn_pad_scatter_rows(const float *rows, const int *src, int b, int n, int c, float *out, void *stream) {
  SN_REQUIRE(rows && src && out, "sn_pad_scatter_rows: null pointer");
  SN_REQUIRE(rows != out, "sn_pad_scatter_rows: out must not alias rows");
  SN_REQUIRE(b >= 1 && n >= 1 && c >= 1 && (long)b * n * c < (1L << 31),
             "sn_pad_scatter_rows: need b, n, c >= 1 and b * n * c < 2^31 (got %d, %d, %d)", b, n, c);
  hipStream_t s = sn::as_stream(stream);
  const long total = (long)b * n * c;
  SN_HIP(hipMemsetAsync(out, 0, (size_t)total * 4, s));
  long blocks = (total + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  pad_scatter_rows_kernel<<<(int)blocks, 256, 0, s>>>(rows, src, total, n, c, out);
  return sn::launch_status("sn_pad_scatter_rows");
}
