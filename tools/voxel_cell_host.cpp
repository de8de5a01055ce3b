// voxel_cell_host.cpp -- the host routines of sparenet_amd/csrc/voxel_cell.hpp (what sn_voxel_grid_host and
// sn_voxel_pool_host run per cloud) in a plain C++ program with its own main, for a sanitizer build:
//
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all
//       tools/voxel_cell_host.cpp -o /tmp/voxel_cell_host && /tmp/voxel_cell_host
//
// Every buffer is a heap array of exactly the size the header gives it, so a write one element out is the sanitizer's
// finding.  The clouds are those of the tests: sizes around the chunk and tile edges, points on cell faces, -0.0 and
// +-1e-30, NaN and infinities, cells at and beyond +-32768, one voxel, all distinct, every cap in {1, count - 1, count, n}
// and every ragged length.  The outputs are checked against the invariants that need no second implementation.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

#include "../sparenet_amd/csrc/voxel_cell.hpp"

namespace {

int failures = 0;
#define CHECK(cond)                                                       \
  do {                                                                    \
    if (!(cond)) {                                                        \
      std::printf("%s:%d: %s failed\n", __FILE__, __LINE__, #cond);       \
      ++failures;                                                         \
    }                                                                     \
  } while (0)

struct Grid {
  int count;
  std::vector<float> centroid;
  std::vector<int> members, first, inverse, order, start;
};

Grid run(const std::vector<float> &xyz, int len, float size, const float *origin, int cap, bool all_outputs = true) {
  const int n = (int)xyz.size() / 3;
  Grid g;
  g.count = -7;
  g.centroid.assign((size_t)cap * 3, std::numeric_limits<float>::quiet_NaN());
  g.members.assign(cap, -7), g.first.assign(cap, -7), g.inverse.assign(n, -7), g.order.assign(n, -7);
  g.start.assign(cap + 1, -7);
  voxel_cell::CloudOut out{&g.count, g.centroid.data(), g.members.data(), g.first.data(), g.inverse.data(),
                           g.order.data(), g.start.data()};
  if (!all_outputs) out = voxel_cell::CloudOut{&g.count, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  voxel_cell::grid_cloud_host(xyz.data(), len, n, size, origin, cap, out);
  return g;
}

void check(const Grid &g, const std::vector<float> &xyz, int len, int cap) {
  const int n = (int)xyz.size() / 3, kept = g.count < cap ? g.count : cap;
  CHECK(g.count >= 0 && g.count <= len);
  int placed = 0;
  for (int k = 0; k < cap; ++k) {
    if (k < kept) {
      CHECK(g.members[k] == g.start[k + 1] - g.start[k] && g.members[k] >= 1);
      CHECK(g.first[k] == g.order[g.start[k]]);
      for (int r = g.start[k]; r < g.start[k + 1]; ++r) {
        CHECK(g.order[r] >= 0 && g.order[r] < len && g.inverse[g.order[r]] == k);
        CHECK(r == g.start[k] || g.order[r - 1] < g.order[r]);      // members by ascending index
      }
      placed += g.members[k];
    } else {
      CHECK(g.members[k] == 0 && g.first[k] == -1 && g.centroid[3 * k] == 0.f && g.start[k + 1] == g.start[kept]);
    }
  }
  CHECK(g.start[0] == 0);
  int with_voxel = 0;
  for (int i = 0; i < n; ++i) {
    CHECK(g.inverse[i] >= -1 && g.inverse[i] < kept);
    CHECK(i < len || g.inverse[i] == -1);
    with_voxel += g.order[i] >= 0;
    CHECK(i == 0 || g.order[i - 1] >= 0 || g.order[i] == -1);      // the -1 entries come last
  }
  CHECK(placed <= with_voxel && (g.count > cap || placed == with_voxel));
}

std::vector<float> cube(int n, unsigned seed, float scale) {
  std::mt19937 rng(seed);
  std::uniform_real_distribution<float> u(-scale, scale);
  std::vector<float> x((size_t)n * 3);
  for (float &v : x) v = u(rng);
  return x;
}

}  // namespace

int main() {
  const float zero[3] = {0.f, 0.f, 0.f}, far_origin[3] = {1e6f, -1e6f, 999936.f};
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  for (int n : {1, 2, 63, 64, 65, 1023, 1024, 1025, 2049, 16384}) {
    const std::vector<float> x = cube(n, 100 + n, 1.f);
    for (float size : {0.2f, 0.125f, 0.01f}) {
      const Grid full = run(x, n, size, zero, n);
      check(full, x, n, n);
      for (int cap : {1, full.count - 1, full.count, n}) {
        if (cap < 1 || cap > n) continue;
        const Grid g = run(x, n, size, zero, cap);
        check(g, x, n, cap);
        CHECK(g.count == full.count);
      }
      for (int len : {0, 1, n - 1, n}) {
        if (len < 0) continue;
        check(run(x, len, size, zero, n), x, len, n);
      }
      CHECK(run(x, n, size, zero, n, false).count == full.count);      // every output but count null
    }
    check(run(x, n, 64.f, far_origin, n), x, n, n);
  }
  // special values: faces, zeros of both signs, tiny values, non-finite coordinates, the rim of the 16-bit cells
  std::vector<float> s;
  for (float a : {-0.f, 0.f, 1e-30f, -1e-30f, -0.125f, 0.125f, -1.f, 3.375f, nan, inf, -inf, -32768.f, 32767.5f, -32768.5f,
                  32768.f, 3e38f, -3e38f})
    for (int axis = 0; axis < 3; ++axis) {
      float p[3] = {0.5f, 1.5f, 2.5f};
      p[axis] = a;
      s.insert(s.end(), p, p + 3);
    }
  for (float size : {1.f, 0.125f}) {
    const int n = (int)s.size() / 3;
    const Grid g = run(s, n, size, zero, n);
    check(g, s, n, n);
    for (int i = 0; i < n; ++i) {
      const bool finite = std::isfinite(s[3 * i]) && std::isfinite(s[3 * i + 1]) && std::isfinite(s[3 * i + 2]);
      CHECK(finite || g.inverse[i] == -1);
    }
  }
  {      // one voxel, and every point its own voxel
    std::vector<float> one = cube(4096, 7, 0.04f);
    for (float &v : one) v += 0.05f;
    const Grid g = run(one, 4096, 1.f, zero, 4096);
    CHECK(g.count == 1 && g.members[0] == 4096 && g.first[0] == 0);
    std::vector<float> line(3 * 1023);
    for (int i = 0; i < 1023; ++i) line[3 * i] = (float)((i * 7) % 1023), line[3 * i + 1] = 0.5f, line[3 * i + 2] = -(float)i;
    const Grid d = run(line, 1023, 1.f, zero, 1023);
    check(d, line, 1023, 1023);
    CHECK(d.count == 1023);
  }
  // pooling: a grid's own arrays, then arrays with foreign entries and offsets
  for (int c : {1, 5, 64}) {
    const int n = 257;
    std::vector<float> x = cube(n, 21, 0.3f), f = cube(n * c / 3 + 1, 22 + c, 2.f);
    x[15] = nan;
    f.resize((size_t)c * n);
    const Grid g = run(x, n, 0.25f, zero, n);
    for (int mode = 0; mode < 3; ++mode) {
      std::vector<float> out((size_t)c * n, nan);
      std::vector<int> arg((size_t)c * n, -7);
      voxel_cell::pool_cloud_host(f.data(), c, n, g.order.data(), g.start.data(), g.count, n, mode, out.data(), arg.data());
      for (int ch = 0; ch < c; ++ch)
        for (int v = 0; v < n; ++v) {
          const int a = arg[(size_t)ch * n + v];
          if (v >= g.count) CHECK(out[(size_t)ch * n + v] == 0.f && a == -1);
          else if (mode == voxel_cell::kMax) CHECK(a >= 0 && a < n && g.inverse[a] == v && out[(size_t)ch * n + v] == f[(size_t)ch * n + a]);
          else CHECK(a == -1);
        }
      voxel_cell::pool_cloud_host(f.data(), c, n, g.order.data(), g.start.data(), g.count, n, mode, out.data(), nullptr);
    }
  }
  {
    const int n = 8, cap = 4;
    const std::vector<float> f = cube(3 * n / 3, 5, 1.f);      // 3 channels of 8
    const int order[n] = {3, -1, 1, 99, 0, 2, -1, -1}, start[cap + 1] = {-2, 4, 3, 6, 9};
    for (int mode = 0; mode < 3; ++mode)
      for (int count : {-1, 0, 3, 4, 9}) {
        std::vector<float> out(3 * cap, nan);
        std::vector<int> arg(3 * cap, -7);
        voxel_cell::pool_cloud_host(f.data(), 3, n, order, start, count, cap, mode, out.data(), arg.data());
        for (float v : out) CHECK(v == v);
      }
  }
  std::printf(failures ? "voxel_cell_host: %d checks failed\n" : "voxel_cell_host: all checks passed\n", failures);
  return failures ? 1 : 0;
}
