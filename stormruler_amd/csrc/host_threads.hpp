// What the host-side build units (op_pack.hip, spmv_build.hip, mesh_host.hip, ordering.hip) share: how many threads a
// build takes, and the stage timer of the operator build.  Each unit keeps its own parallel-for with its own chunking rule.
#pragma once

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <thread>

namespace storm {

// STORM_HIP_BUILD_THREADS; unset, 0 or less: min(16, cores) (a one-GPU share of a host is about 16 cores)
inline int host_threads() {
  const char *e = getenv("STORM_HIP_BUILD_THREADS");
  int t = e ? atoi(e) : 0;
  if (t <= 0) t = (int)std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
  return t;
}

struct BuildTimer {  // STORM_HIP_BUILD_TIMING=1: stage times of the operator build on stderr
  bool on = getenv("STORM_HIP_BUILD_TIMING") != nullptr;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  void lap(const char *what) {
    if (!on) return;
    const auto t1 = std::chrono::steady_clock::now();
    fprintf(stderr, "[storm_hip build] %-28s %8.1f ms\n", what, std::chrono::duration<double, std::milli>(t1 - t0).count());
    t0 = t1;
  }
};

}  // namespace storm
