// The smoothed-aggregation multigrid preconditioner through the reference's pre_op / pre_side hook (Solver.hpp:74-75),
// written the way cheb_driver.cpp writes a solve: compiled against include/storm_hip/Storm.hpp only.
//
//   amg_driver <n> <cg|bicgstab|gmres> <smoother degree> <reduced 0|1> <left|right> [coarse_rows]
//
// solves -L x = 1 on the n^3 box (fp64 records: option spmv_dict = 0) with AmgPreconditioner and prints one JSON line.
#include <storm_hip/Storm.hpp>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

using namespace Storm;

struct BoxMesh {
  std::vector<int64_t> inner, outer, b_cell;
  std::vector<real_t> coef, b_coef, volume;
  size_t n_cells = 0;
};

// n^3 unit cube, cell id (k*n + j)*n + i, faces cell-major +x,+y,+z, wall faces -x,+x,-y,+y,-z,+z
// (poisson_driver.cpp's mesh = stormruler_amd.mesh.structured_box).
static BoxMesh make_box(int n) {
  BoxMesh m;
  const real_t h = 1.0 / n;
  m.n_cells = (size_t)n * n * n;
  m.volume.assign(m.n_cells, h * h * h);
  auto center = [&](int i) { return (i + 0.5) * h; };
  auto dist = [&](real_t a, real_t b) {  // length(a - b) of Bittern: sqrt(0 + d*d)
    const real_t d = a - b;
    real_t s = 0.0;
    s = s + d * d;
    return std::sqrt(s);
  };
  const real_t area = h * h;
  for (int k = 0; k < n; ++k)
    for (int j = 0; j < n; ++j)
      for (int i = 0; i < n; ++i) {
        const int64_t c = ((int64_t)k * n + j) * n + i;
        if (i < n - 1) m.inner.push_back(c), m.outer.push_back(c + 1), m.coef.push_back(area / dist(center(i + 1), center(i)));
        if (j < n - 1) m.inner.push_back(c), m.outer.push_back(c + n), m.coef.push_back(area / dist(center(j + 1), center(j)));
        if (k < n - 1) m.inner.push_back(c), m.outer.push_back(c + (int64_t)n * n), m.coef.push_back(area / dist(center(k + 1), center(k)));
        const int idx[3] = {i, j, k};
        for (int ax = 0; ax < 3; ++ax) {
          if (idx[ax] == 0) m.b_cell.push_back(c), m.b_coef.push_back(area / dist(center(0) - 0.5 * h, center(0)));
          if (idx[ax] == n - 1) m.b_cell.push_back(c), m.b_coef.push_back(area / dist(center(n - 1) + 0.5 * h, center(n - 1)));
        }
      }
  return m;
}

template<template<class> class SolverT>
static int run(int n, int degree, bool reduced, PreconditionerSide side, int coarse_rows) {
  Context ctx(0);
  ctx.set_option("spmv_dict", 0);  // fp64 records: what the multigrid object reads
  const BoxMesh mesh = make_box(n);
  const StencilMatrix matrix = StencilMatrix::from_faces(ctx, mesh.n_cells, 0, mesh.inner, mesh.outer, mesh.coef,
                                                         mesh.b_cell, mesh.b_coef, mesh.volume);
  DeviceVector b(ctx, mesh.n_cells), x(ctx, mesh.n_cells);
  fill_with(b, 1.0);
  SolverT<DeviceVector> solver;
  if constexpr (std::is_base_of_v<InnerOuterIterativeSolver<DeviceVector>, SolverT<DeviceVector>>)
    solver.num_inner_iterations = 20;
  auto pre = std::make_unique<AmgPreconditioner>(degree, reduced);
  if (coarse_rows > 0) pre->params.coarse_rows = coarse_rows;
  const AmgPreconditioner* amg = pre.get();
  solver.pre_op = std::move(pre);
  solver.pre_side = side;
  const HipStencilOperator op(matrix, -1.0, 0.0);  // A = -L
  const bool converged = solver.solve(x, b, op);
  ctx.sync();
  std::string rows;
  for (int64_t r : amg->level_rows()) rows += (rows.empty() ? "" : ", ") + std::to_string((long long)r);
  std::printf("{\"n\": %d, \"converged\": %s, \"iterations\": %zu, \"absolute_error\": %.17g, \"x_norm2\": %.17g, "
              "\"pre_applies\": %zu, \"level_rows\": [%s], \"operator_complexity\": %.17g, \"amg_applies\": %lld, "
              "\"amg_fused_residuals\": %lld, \"amg_statement_residuals\": %lld, \"cheb_reduced_applies\": %lld}\n",
              n, converged ? "true" : "false", solver.iteration, solver.absolute_error, norm_2(x), solver.num_pre_applies,
              rows.c_str(), amg->get("operator_complexity"), ctx.counter("amg_applies"), ctx.counter("amg_fused_residuals"),
              ctx.counter("amg_statement_residuals"), ctx.counter("cheb_reduced_applies"));
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 6) {
    std::fprintf(stderr, "usage: %s <n> <cg|bicgstab|gmres> <smoother degree> <reduced 0|1> <left|right> [coarse_rows]\n", argv[0]);
    return 2;
  }
  const int n = std::atoi(argv[1]);
  const std::string kind = argv[2];
  const int degree = std::atoi(argv[3]);
  const bool reduced = std::atoi(argv[4]) != 0;
  const PreconditionerSide side = std::string(argv[5]) == "left" ? PreconditionerSide::Left : PreconditionerSide::Right;
  const int coarse_rows = argc > 6 ? std::atoi(argv[6]) : 0;
  try {
    if (kind == "cg") return run<CgSolver>(n, degree, reduced, side, coarse_rows);
    if (kind == "bicgstab") return run<BiCgStabSolver>(n, degree, reduced, side, coarse_rows);
    if (kind == "gmres") return run<GmresSolver>(n, degree, reduced, side, coarse_rows);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "amg_driver: %s\n", e.what());
    return 1;
  }
  std::fprintf(stderr, "amg_driver: unknown solver '%s'\n", kind.c_str());
  return 2;
}
