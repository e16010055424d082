// The multigrid preconditioner with the Jacobi smoother on a non-symmetric operator, through the reference's pre_op /
// pre_side hook (Solver.hpp:74-75), written the way amg_driver.cpp writes a solve: compiled against
// include/storm_hip/Storm.hpp only.
//
//   amg_jacobi_driver <n> <gmres|fgmres|bicgstab> <sweeps> <left|right> [coarse_rows]
//
// solves A x = 1, A = -nu L + C(v) (first-order upwind, nu = 1e-2, v = (1, 0.5, 0.25), Dirichlet 0: BASELINE config 4) on
// the n^3 box (fp64 records: option spmv_dict = 0) with AmgPreconditioner::use_jacobi and prints one JSON line.
#include <storm_hip/Storm.hpp>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

using namespace Storm;

struct Weights {
  std::vector<int64_t> inner, outer;
  std::vector<real_t> w_inner, w_outer, diag;
  size_t n_cells = 0;
};

// n^3 unit cube, cell id (k*n + j)*n + i, faces cell-major +x,+y,+z (stormruler_amd.mesh.structured_box); the weights of
// stormruler_amd.mesh.convection_diffusion_weights on it: (A x)_i = sum_f w_if (x_other - x_i) + diag_i x_i.
static Weights make_weights(int n, real_t nu, const real_t (&vel)[3]) {
  Weights m;
  const real_t h = 1.0 / n;
  m.n_cells = (size_t)n * n * n;
  m.diag.assign(m.n_cells, 0.0);
  const int64_t stride[3] = {1, n, (int64_t)n * n};
  for (int k = 0; k < n; ++k)
    for (int j = 0; j < n; ++j)
      for (int i = 0; i < n; ++i) {
        const int64_t c = ((int64_t)k * n + j) * n + i;
        const int idx[3] = {i, j, k};
        for (int ax = 0; ax < 3; ++ax) {
          const real_t vn = vel[ax];  // the unit vector inner -> outer is +e_ax
          if (idx[ax] < n - 1) {
            const int64_t o = c + stride[ax];
            m.inner.push_back(c), m.outer.push_back(o);
            m.w_inner.push_back(-nu / (h * h) + std::fmin(vn, 0.0) / h);
            m.w_outer.push_back(-nu / (h * h) - std::fmax(vn, 0.0) / h);
            m.diag[(size_t)c] += vn / h, m.diag[(size_t)o] -= vn / h;
          }
          // walls: the half-cell distance, a zero ghost state on inflow
          if (idx[ax] == 0) m.diag[(size_t)c] += 2.0 * nu / (h * h) + std::fmax(-vn, 0.0) / h;
          if (idx[ax] == n - 1) m.diag[(size_t)c] += 2.0 * nu / (h * h) + std::fmax(vn, 0.0) / h;
        }
      }
  return m;
}

template<template<class> class SolverT>
static int run(int n, int sweeps, PreconditionerSide side, int coarse_rows) {
  Context ctx(0);
  ctx.set_option("spmv_dict", 0);  // fp64 records: what the multigrid object reads
  const real_t vel[3] = {1.0, 0.5, 0.25};
  const Weights w = make_weights(n, 1e-2, vel);
  const StencilMatrix matrix = StencilMatrix::from_face_weights(ctx, w.n_cells, 0, w.inner, w.outer, w.w_inner, w.w_outer, w.diag.data());
  DeviceVector b(ctx, w.n_cells), x(ctx, w.n_cells);
  fill_with(b, 1.0);
  const HipStencilOperator op(matrix, 1.0, 0.0);
  SolverT<DeviceVector> plain;
  if constexpr (std::is_base_of_v<InnerOuterIterativeSolver<DeviceVector>, SolverT<DeviceVector>>) plain.num_inner_iterations = 30;
  const bool plain_converged = plain.solve(x, b, op);
  fill_with(x, 0.0);
  SolverT<DeviceVector> solver;
  if constexpr (std::is_base_of_v<InnerOuterIterativeSolver<DeviceVector>, SolverT<DeviceVector>>) solver.num_inner_iterations = 30;
  auto pre = std::make_unique<AmgPreconditioner>();
  pre->use_jacobi(sweeps);
  if (coarse_rows > 0) pre->params.coarse_rows = coarse_rows;
  const AmgPreconditioner* amg = pre.get();
  solver.pre_op = std::move(pre);
  solver.pre_side = side;
  const bool converged = solver.solve(x, b, op);
  ctx.sync();
  std::string rows;
  for (int64_t r : amg->level_rows()) rows += (rows.empty() ? "" : ", ") + std::to_string((long long)r);
  std::printf("{\"n\": %d, \"converged\": %s, \"iterations\": %zu, \"absolute_error\": %.17g, \"x_norm2\": %.17g, "
              "\"plain_converged\": %s, \"plain_iterations\": %zu, \"pre_applies\": %zu, \"level_rows\": [%s], "
              "\"smoother_kind\": %g, \"jacobi_sweeps\": %g, \"jacobi_omega\": %.17g, \"jacobi_sigma_0\": %.17g, "
              "\"amg_applies\": %lld, \"amg_fused_sweeps\": %lld, \"amg_statement_sweeps\": %lld}\n",
              n, converged ? "true" : "false", solver.iteration, solver.absolute_error, norm_2(x),
              plain_converged ? "true" : "false", plain.iteration, solver.num_pre_applies, rows.c_str(),
              amg->get("smoother_kind"), amg->get("jacobi_sweeps"), amg->get("jacobi_omega"), amg->get("jacobi_sigma_0"),
              ctx.counter("amg_applies"), ctx.counter("amg_fused_sweeps"), ctx.counter("amg_statement_sweeps"));
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 5) {
    std::fprintf(stderr, "usage: %s <n> <gmres|fgmres|bicgstab> <sweeps> <left|right> [coarse_rows]\n", argv[0]);
    return 2;
  }
  const int n = std::atoi(argv[1]);
  const std::string kind = argv[2];
  const int sweeps = std::atoi(argv[3]);
  const PreconditionerSide side = std::string(argv[4]) == "left" ? PreconditionerSide::Left : PreconditionerSide::Right;
  const int coarse_rows = argc > 5 ? std::atoi(argv[5]) : 0;
  try {
    if (kind == "gmres") return run<GmresSolver>(n, sweeps, side, coarse_rows);
    if (kind == "fgmres") return run<FgmresSolver>(n, sweeps, side, coarse_rows);
    if (kind == "bicgstab") return run<BiCgStabSolver>(n, sweeps, side, coarse_rows);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "amg_jacobi_driver: %s\n", e.what());
    return 1;
  }
  std::fprintf(stderr, "amg_jacobi_driver: unknown solver '%s'\n", kind.c_str());
  return 2;
}
