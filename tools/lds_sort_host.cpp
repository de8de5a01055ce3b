// lds_sort_host.cpp -- the workgroup sorts of sparenet_amd/csrc/lds_sort.hpp (the record sort of swd.hip and
// voxel_grid.hip, the key sort of sorted_lists.hpp and emd_general.hip) in a plain C++ program with its own main, for a
// sanitizer build:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       tools/lds_sort_host.cpp -o /tmp/lds_sort_host && /tmp/lds_sort_host
//
// It runs the header's own drivers, sort_pass and index arithmetic: a workgroup is every lane 0 .. n - 1 one after
// another inside each pass, which is exact because within a pass no two lanes touch the same element.  The array of a
// width is a heap array of exactly slot(width) doubles (of exactly p2 keys), so one index out of range is the
// sanitizer's finding.  Every power-of-two width from 2 to 16384, which is every mix of 1- to 4-step passes and the
// multi-trip lane loop; records random, ascending, descending and two-valued, all unique by their index field.  The
// result must be ascending and a permutation of the input, and the gap behind every 16 records untouched.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../sparenet_amd/csrc/lds_sort.hpp"

namespace {

int failures = 0;
#define CHECK(cond)                                                       \
  do {                                                                    \
    if (!(cond)) {                                                        \
      std::printf("%s:%d: %s failed\n", __FILE__, __LINE__, #cond);       \
      ++failures;                                                         \
    }                                                                     \
  } while (0)

// the n lanes of a workgroup, one after another; nothing to wait for between two passes
template <int N>
struct Serial {
  static constexpr int first = 0, kCount = N;
  void barrier() const {}
};

using u64 = unsigned long long;
enum Kind { kRandom, kAscending, kDescending, kTwoValued, kKinds };

// a positive normal double: 1.0's exponent, mantissa (key << 14) | index -- the record of swd.hip
double record(unsigned key, int index) {
  const u64 bits = 0x3ff0000000000000ull | ((u64)key << 14) | (unsigned)index;
  double d;
  std::memcpy(&d, &bits, sizeof d);
  return d;
}

unsigned key_of(Kind kind, int i, int n, std::mt19937 &rng) {
  switch (kind) {
    case kAscending: return (unsigned)i;
    case kDescending: return (unsigned)(n - 1 - i);
    case kTwoValued: return rng() & 1u ? 0xffffffffu : 0u;
    default: return (unsigned)rng();
  }
}

void check_records(int width, Kind kind, std::mt19937 &rng) {
  const int slots = lds_sort::slot(width);
  CHECK(lds_sort::lds_bytes(width) == (size_t)slots * sizeof(double));
  const double gap = -7.0;      // no record: a pass that touched a gap would move or overwrite it
  double *rec = new double[slots];
  std::fill(rec, rec + slots, gap);
  std::vector<double> want(width);
  for (int i = 0; i < width; ++i) want[i] = rec[lds_sort::slot(i)] = record(key_of(kind, i, width, rng), i);
  lds_sort::sort_records(rec, width, Serial<lds_sort::kThreads>{});
  std::sort(want.begin(), want.end());      // unique records: ascending and a permutation = equal to the sorted input
  int records = 0;
  for (int i = 0; i < width; ++i) records += rec[lds_sort::slot(i)] == want[i];
  CHECK(records == width);
  CHECK(std::count(rec, rec + slots, gap) == slots - width);
  delete[] rec;
}

template <int kLanes, class T>
void check_keys(int p2, Kind kind, std::mt19937 &rng) {
  T *keys = new T[p2];
  for (int i = 0; i < p2; ++i) {
    const unsigned k = key_of(kind, i, p2, rng);
    keys[i] = (T)(kind == kRandom || kind == kTwoValued ? k : k - (unsigned)(p2 / 2));      // both signs of int
  }
  std::vector<T> want(keys, keys + p2);
  lds_sort::sort_keys<kLanes>(keys, p2, Serial<kLanes>{});
  std::sort(want.begin(), want.end());
  CHECK(std::equal(want.begin(), want.end(), keys));
  delete[] keys;
}

}  // namespace

int main() {
  std::mt19937 rng(20261021);
  for (int len : {0, 1, 2, 3, 16, 17, 1024, 1025, 16383, 16384}) {
    const int w = lds_sort::pow2_width(len);
    CHECK(w >= 2 && w >= len && (w & (w - 1)) == 0 && (w == 2 || w / 2 < len));
  }
  for (int width = 2; width <= 16384; width <<= 1)
    for (int kind = 0; kind < kKinds; ++kind) check_records(width, (Kind)kind, rng);
  for (int p2 : {1, 2, 64, 1024, 2048, 16384})
    for (int kind = 0; kind < kKinds; ++kind) {
      check_keys<256, int>(p2, (Kind)kind, rng);
      check_keys<256, unsigned>(p2, (Kind)kind, rng);
      check_keys<1024, int>(p2, (Kind)kind, rng);
      check_keys<1024, unsigned>(p2, (Kind)kind, rng);
    }
  std::printf(failures ? "lds_sort_host: %d checks failed\n" : "lds_sort_host: all checks passed\n", failures);
  return failures ? 1 : 0;
}
