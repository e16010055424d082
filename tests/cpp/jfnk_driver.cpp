// The cubic problem A(x) = x - kappa L x + c x^3 = b on an n^3 box, solved through include/storm_hip/Storm.hpp the way
// a user of the reference writes it: the operator is a lambda through make_operator (Playground.cpp:151-167), the solver
// an object with the reference's knobs.
//
//   jfnk_driver <n> <native|host-loop|both>
//
// native:    HipJfnkSolver -- the Newton loop and every Jacobian-vector product inside the library (STORM_HIP_JFNK)
// host-loop: JfnkSolver    -- SolverNewton.hpp:101-173 as a user-level host loop, |y| on the host at every product
// prints one JSON line (with x at five sampled rows); both: a line per arm and a third with |x_native - x_host_loop|_2.
#include <storm_hip/Storm.hpp>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

using namespace Storm;

struct BoxMesh {
  std::vector<int64_t> inner, outer, b_cell;
  std::vector<real_t> coef, b_coef, volume, x_centre;
  size_t n_cells = 0;
};

// n^3 unit cube, cell id (k*n + j)*n + i, faces cell-major +x,+y,+z, wall faces -x,+x,-y,+y,-z,+z
// (the synthetic mesh of stormruler_amd.mesh.structured_box).
static BoxMesh make_box(int n) {
  BoxMesh m;
  const real_t h = 1.0 / n;
  m.n_cells = (size_t)n * n * n;
  m.volume.assign(m.n_cells, h * h * h);
  auto center = [&](int i) { return (i + 0.5) * h; };
  auto dist = [&](real_t a, real_t b) {
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
        m.x_centre.push_back(center(i));
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
static int run(int n, std::vector<real_t>& x_out) {
  constexpr real_t kappa = 1.0e-2, c3 = 0.5;
  Context ctx(0);
  const BoxMesh mesh = make_box(n);
  const StencilMatrix matrix = StencilMatrix::from_faces(ctx, mesh.n_cells, 0, mesh.inner, mesh.outer, mesh.coef,
                                                         mesh.b_cell, mesh.b_coef, mesh.volume);
  std::vector<real_t> b_host(mesh.n_cells);
  for (size_t i = 0; i < mesh.n_cells; ++i) b_host[i] = 1.0 + 0.5 * std::sin(5.0 * mesh.x_centre[i]);
  DeviceVector b(ctx, mesh.n_cells), x(ctx, mesh.n_cells), sq(ctx, mesh.n_cells), res(ctx, mesh.n_cells);
  b.upload(b_host.data(), b_host.size());
  const auto op = make_operator<DeviceVector>([&](DeviceVector& y_vec, const DeviceVector& x_vec) {
    matrix.apply(-kappa, 1.0, x_vec, y_vec);
    vmul(sq, x_vec, x_vec);
    if (storm_hip_vmul_add(y_vec.handle(), c3, sq.handle(), x_vec.handle()) != STORM_HIP_OK)  // y += c x^2 .* x
      throw std::runtime_error(storm_hip_last_error());
  });
  SolverT<DeviceVector> solver;
  ctx.sync();
  const long long reductions0 = ctx.counter("host_reductions");
  const auto t0 = std::chrono::steady_clock::now();
  const bool converged = solver.solve(x, b, *op);
  ctx.sync();
  const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  const long long reductions = ctx.counter("host_reductions") - reductions0;
  op->mul(res, x);
  res <<= b - res;
  x_out = x.to_host();
  const size_t last = mesh.n_cells - 1;
  const size_t rows[5] = {0, last / 4, last / 2, (3 * last) / 4, last};
  std::printf("{\"x_rows\": [%zu, %zu, %zu, %zu, %zu], \"x_samples\": [%.17g, %.17g, %.17g, %.17g, %.17g]}\n", rows[0], rows[1],
              rows[2], rows[3], rows[4], x_out[rows[0]], x_out[rows[1]], x_out[rows[2]], x_out[rows[3]], x_out[rows[4]]);
  std::printf("{\"n\": %d, \"converged\": %s, \"iterations\": %zu, \"inner_iterations\": %zu, \"absolute_error\": %.17g, "
              "\"relative_error\": %.17g, \"x_norm2\": %.17g, \"residual_norm2\": %.17g, \"host_reductions\": %lld, "
              "\"jfnk_inner_solves\": %lld, \"solve_seconds\": %.6f}\n",
              n, converged ? "true" : "false", solver.iteration, solver.inner_iterations, solver.absolute_error,
              solver.relative_error, norm_2(x), norm_2(res), reductions, ctx.counter("jfnk_inner_solves"), seconds);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: %s <n> <native|host-loop|both>\n", argv[0]);
    return 2;
  }
  const int n = std::atoi(argv[1]);
  const std::string mode = argv[2];
  try {
    std::vector<real_t> xa, xb;
    if (mode == "native") return run<HipJfnkSolver>(n, xa);
    if (mode == "host-loop") return run<JfnkSolver>(n, xa);
    if (mode == "both") {
      if (const int st = run<HipJfnkSolver>(n, xa)) return st;
      if (const int st = run<JfnkSolver>(n, xb)) return st;
      real_t diff = 0.0, norm = 0.0;
      for (size_t i = 0; i < xa.size(); ++i) diff += (xa[i] - xb[i]) * (xa[i] - xb[i]), norm += xb[i] * xb[i];
      std::printf("{\"x_diff_norm2\": %.17g, \"x_host_loop_norm2\": %.17g}\n", std::sqrt(diff), std::sqrt(norm));
      return 0;
    }
    std::fprintf(stderr, "unknown mode %s\n", mode.c_str());
    return 2;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
