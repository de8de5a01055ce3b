// split_launch.hpp -- the host side the split searches share (sinkhorn.hip, neighbors.hip): how many segments S the
// targets of a query are cut into, and the launch shape that follows from S.  A search serves its queries with one
// lane each and S waves per 64 queries, every wave walking targets / S of the targets; S == 1 is the wide workgroup
// of 256 queries.  Each file keeps its constants (cap, waves per compute unit, shortest segment, tiles), its LDS sizes
// and the read of its knob -- SN_KNOB("SN_..._SPLIT") at the call, where a search for the name finds it.  Host code.
#pragma once
#include "common.hpp"

#include <cstdlib>

namespace sn {

// S: the knob's value when it is set (held to [1, cap]); otherwise doubled while the launch stays within waves_per_cu
// waves per compute unit and a segment keeps min_segment targets.  A wave's time is its serial walk over targets / S
// targets, so until the device is that full a wider split is faster (DESIGN.md has each operator's sweep).
inline int pick_split(const char *knob, int b, int queries, int targets, int cap, int waves_per_cu, int min_segment,
                      int *out) {
  if (knob && *knob) {
    const int v = atoi(knob);
    *out = v < 1 ? 1 : (v > cap ? cap : v);
    return 0;
  }
  int dev = 0, cus = 0;
  SN_HIP(hipGetDevice(&dev));
  SN_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  const long waves = (long)b * ceil_div(queries, 64);
  int s = 1;
  while (s * 2 <= cap && waves * s * 2 <= (long)waves_per_cu * cus && targets / (s * 2) >= min_segment) s *= 2;
  *out = s;
  return 0;
}

struct SplitLaunch {      // the launch shape of a search with split S
  int split, qblocks;     // S; workgroups per cloud
  unsigned grid, threads;
};

constexpr int kWideLanes = 256;      // queries per workgroup, S == 1

inline int split_launch(const char *what, int b, int queries, int split, SplitLaunch *l) {
  const int lanes = split == 1 ? kWideLanes : 64;
  l->split = split;
  l->qblocks = ceil_div(queries, lanes);
  SN_REQUIRE((long)b * l->qblocks < (1L << 31), "%s: too many queries", what);
  l->grid = (unsigned)((long)b * l->qblocks);
  l->threads = (unsigned)(lanes * split);
  return 0;
}

}  // namespace sn
