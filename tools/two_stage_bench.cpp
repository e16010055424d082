// Microseconds per CG iteration of the playground's Cahn-Hilliard solve (Playground.cpp:151-167) in three forms, written
// against include/storm_hip/Storm.hpp only (driven by tools/two_stage_bench.py):
//
//   two_stage_bench callback|engine|latency box:<n>|mesh:<tetgen prefix> <iterations> <solves>
//
//   callback  the operator exactly as tests/cpp/timestep_driver.cpp builds it: `make_operator` over the lambda with its two
//             stormDivGrad calls.  Uses nothing of the two-stage operator, so this mode also compiles against a header
//             without it (STORM_HIP_HAS_TWO_STAGE undefined): the baseline is taken on a build of the parent commit.
//             The lambda is affine (f + sigma (c_in - c) has a constant part) and goes to plain CG as in the playground:
//             with the tolerances off its iterates need not stay bounded -- the launches that are timed are the same;
//   engine    HipTwoStageOperator with option latency_path = 0: the engine's CG loop, both stages as library launches;
//   latency   HipTwoStageOperator on the one-kernel path (latency_path = 2).
//
// Playground constants, tolerances off, <iterations> iterations per solve, one warm-up solve and then <solves> timed
// ones between Context::sync() calls; one JSON line with every solve's us per iteration and their median.
#include <storm_hip/Storm.hpp>

#include <time.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace Storm;

namespace {

const double tau = 1.0e-3, Gamma = 1.0e-4, sigma = 2.0;  // Playground.cpp:113

// n^3 unit cube, faces cell-major +x, +y, +z, Dirichlet wall faces (the box of stormruler_amd.mesh.structured_box)
StencilMatrix box_matrix(const Context& ctx, int n, std::size_t& n_cells) {
  std::vector<int64_t> inner, outer, b_cell;
  std::vector<real_t> area, center, volume, b_area, b_center;
  const real_t h = 1.0 / n, a = h * h;
  n_cells = (std::size_t)n * n * n;
  volume.assign(n_cells, h * h * h);
  center.resize(3 * n_cells);
  for (int k = 0; k < n; ++k)
    for (int j = 0; j < n; ++j)
      for (int i = 0; i < n; ++i) {
        const int64_t c = ((int64_t)k * n + j) * n + i;
        const int idx[3] = {i, j, k};
        const int64_t stride[3] = {1, n, (int64_t)n * n};
        for (int ax = 0; ax < 3; ++ax) center[3 * (std::size_t)c + ax] = (idx[ax] + 0.5) * h;
        for (int ax = 0; ax < 3; ++ax)
          if (idx[ax] < n - 1) inner.push_back(c), outer.push_back(c + stride[ax]), area.push_back(a);
        for (int ax = 0; ax < 3; ++ax)
          for (int side = 0; side < 2; ++side)
            if (idx[ax] == (side ? n - 1 : 0)) {
              b_cell.push_back(c), b_area.push_back(a);
              for (int e = 0; e < 3; ++e) b_center.push_back(e == ax ? (side ? 1.0 : 0.0) : center[3 * (std::size_t)c + e]);
            }
      }
  return StencilMatrix::from_mesh(ctx, n_cells, 0, 3, inner, outer, area, center, b_cell, b_area, b_center, volume);
}

int run(const std::string& mode, const std::string& problem, int iterations, int solves) {
  Context ctx(0);
  std::size_t n = 0;
  StencilMatrix mesh;
  if (problem.rfind("box:", 0) == 0) {
    mesh = box_matrix(ctx, std::atoi(problem.c_str() + 4), n);
  } else if (problem.rfind("mesh:", 0) == 0) {
    const HostMesh host_mesh = HostMesh::read_tetgen(problem.substr(5), 2);
    mesh = host_mesh.matrix(ctx, /*neumann=*/true);
    n = host_mesh.num_cells();
  } else {
    throw std::runtime_error("problem: box:<n> or mesh:<prefix>");
  }
  DeviceVector c(ctx, n), c_hat(ctx, n), w_hat(ctx, n), f(ctx, n);
  std::vector<real_t> c0(n);
  unsigned long long lcg = 2024;
  for (auto& v : c0) lcg = lcg * 6364136223846793005ULL + 1442695040888963407ULL, v = (double)(lcg >> 11) / 9007199254740992.0;
  c.upload(c0.data(), n);
  f <<= map([](auto c) noexcept { return 2.0 * c * (c - 1.0) * (2.0 * c - 1.0); }, c);

  const auto lambda = make_operator<DeviceVector>([&](DeviceVector& c_hat, const DeviceVector& c_in) {
    w_hat <<= f + sigma * (c_in - c);
    stormDivGrad(mesh, w_hat, -Gamma, c_in);

    c_hat <<= c_in;
    stormDivGrad(mesh, c_hat, -tau, w_hat);
  });
  const Operator<DeviceVector>* op = lambda.get();
#ifdef STORM_HIP_HAS_TWO_STAGE
  const HipTwoStageOperator two_stage(mesh, -Gamma, sigma, -tau, 1.0);
  if (mode == "engine" || mode == "latency") {
    ctx.set_option("latency_path", mode == "latency" ? 2 : 0);
    op = &two_stage;
  } else
#endif
  if (mode != "callback") throw std::runtime_error("mode: callback (or, with the two-stage operator, engine / latency)");

  CgSolver<DeviceVector> solver;
  solver.num_iterations = (std::size_t)iterations;
  solver.absolute_error_tolerance = solver.relative_error_tolerance = 0.0;
  std::vector<double> us;
  for (int k = -1; k < solves; ++k) {  // (k = -1: warm-up)
    c_hat <<= c;
    ctx.sync();
    struct timespec start, finish;
    clock_gettime(CLOCK_MONOTONIC, &start);
    solver.solve(c_hat, c, *op);
    ctx.sync();
    clock_gettime(CLOCK_MONOTONIC, &finish);
    if (solver.iteration != (std::size_t)iterations) throw std::runtime_error("the solve stopped early");
    const double s = (double)(finish.tv_sec - start.tv_sec) + (double)(finish.tv_nsec - start.tv_nsec) / 1e9;
    if (k >= 0) us.push_back(s / iterations * 1e6);
  }
  std::vector<double> sorted = us;
  std::sort(sorted.begin(), sorted.end());
  std::printf("{\"mode\": \"%s\", \"problem\": \"%s\", \"rows\": %zu, \"iterations\": %d, \"us_per_iteration\": %.3f, \"solves_us_per_iteration\": [",
              mode.c_str(), problem.c_str(), n, iterations, sorted[sorted.size() / 2]);
  for (std::size_t i = 0; i < us.size(); ++i) std::printf("%s%.3f", i ? ", " : "", us[i]);
  std::printf("], \"latency_solves\": %lld, \"engine_solves\": %lld}\n", ctx.counter("latency_solves"), ctx.counter("engine_solves"));
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  try {
    if (argc == 5) return run(argv[1], argv[2], std::atoi(argv[3]), std::atoi(argv[4]));
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  std::fprintf(stderr, "usage: %s callback|engine|latency box:<n>|mesh:<prefix> <iterations> <solves>\n", argv[0]);
  return 2;
}
