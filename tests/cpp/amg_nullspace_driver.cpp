// The multigrid preconditioner on a singular operator whose kernel is the constants (AmgPreconditioner::nullspace_constant,
// storm_hip_amg_create_nullspace), compiled against include/storm_hip/Storm.hpp only:
//
//   amg_nullspace_driver <nx> <ny> <nz> <smoother degree> [coarse_rows]
//
// solves -L_N x = b on the nx x ny x nz box WITHOUT wall faces (pure Neumann; fp64 records: option spmv_dict = 0) for a
// mean-free right-hand side by CG with the preconditioner, and prints one JSON line: iterations, the true relative
// residual |b - A x| / |b| and the mean of x.
#include <storm_hip/Storm.hpp>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

using namespace Storm;

int main(int argc, char** argv) {
  if (argc < 5) {
    std::fprintf(stderr, "usage: %s <nx> <ny> <nz> <smoother degree> [coarse_rows]\n", argv[0]);
    return 2;
  }
  const int nx = std::atoi(argv[1]), ny = std::atoi(argv[2]), nz = std::atoi(argv[3]), degree = std::atoi(argv[4]);
  const int coarse_rows = argc > 5 ? std::atoi(argv[5]) : 0;
  if (nx < 1 || ny < 1 || nz < 1 || (int64_t)nx * ny * nz < 2) {
    std::fprintf(stderr, "amg_nullspace_driver: a box of at least two cells\n");
    return 2;
  }
  try {
    Context ctx(0);
    ctx.set_option("spmv_dict", 0);  // fp64 records: what the multigrid object reads
    // unit spacing, cell id (k ny + j) nx + i, faces cell-major +x, +y, +z, no wall faces
    const size_t n = (size_t)nx * ny * nz;
    std::vector<int64_t> inner, outer, none;
    std::vector<real_t> coef, no_coef, volume(n, 1.0);
    for (int k = 0; k < nz; ++k)
      for (int j = 0; j < ny; ++j)
        for (int i = 0; i < nx; ++i) {
          const int64_t c = ((int64_t)k * ny + j) * nx + i;
          if (i < nx - 1) inner.push_back(c), outer.push_back(c + 1), coef.push_back(1.0);
          if (j < ny - 1) inner.push_back(c), outer.push_back(c + nx), coef.push_back(1.0);
          if (k < nz - 1) inner.push_back(c), outer.push_back(c + (int64_t)nx * ny), coef.push_back(1.0);
        }
    const StencilMatrix matrix = StencilMatrix::from_faces(ctx, n, 0, inner, outer, coef, none, no_coef, volume);
    // b_i = sin(0.37 i) less its mean, the mean taken on the host in long double
    std::vector<real_t> b_host(n);
    long double sum = 0.0L;
    for (size_t i = 0; i < n; ++i) b_host[i] = std::sin(0.37 * (double)i), sum += b_host[i];
    for (size_t i = 0; i < n; ++i) b_host[i] -= (double)(sum / (long double)n);
    DeviceVector b(ctx, n), x(ctx, n), ax(ctx, n);
    b.upload(b_host.data(), n);
    CgSolver<DeviceVector> solver;
    auto pre = std::make_unique<AmgPreconditioner>(degree);
    pre->nullspace_constant = true;
    if (coarse_rows > 0) pre->params.coarse_rows = coarse_rows;
    const AmgPreconditioner* amg = pre.get();
    solver.pre_op = std::move(pre);
    const HipStencilOperator op(matrix, -1.0, 0.0);  // A = -L_N
    const bool converged = solver.solve(x, b, op);
    op.mul(ax, x);
    ctx.sync();
    const std::vector<real_t> x_host = x.to_host(), ax_host = ax.to_host();
    long double r2 = 0.0L, b2 = 0.0L, xs = 0.0L, x_max = 0.0L;
    for (size_t i = 0; i < n; ++i) {
      const long double r = (long double)b_host[i] - ax_host[i];
      r2 += r * r, b2 += (long double)b_host[i] * b_host[i], xs += x_host[i];
      x_max = std::fmax(x_max, std::fabs((long double)x_host[i]));
    }
    // project() on a copy of x: what it removes is the mean printed above
    DeviceVector xp(ctx, n);
    xp.upload(x_host.data(), n);
    amg->project(xp);
    ctx.sync();
    long double xps = 0.0L;
    for (real_t v : xp.to_host()) xps += v;
    std::string rows;
    for (int64_t r : amg->level_rows()) rows += (rows.empty() ? "" : ", ") + std::to_string((long long)r);
    std::printf("{\"n\": %zu, \"converged\": %s, \"iterations\": %zu, \"true_relative_residual\": %.17g, \"mean_x\": %.17g, "
                "\"max_abs_x\": %.17g, \"mean_projected_x\": %.17g, \"level_rows\": [%s], \"nullspace\": %d, \"coarse_shift\": %.17g, "
                "\"amg_applies\": %lld, \"amg_projections\": %lld, \"amg_fused_projections\": %lld}\n",
                n, converged ? "true" : "false", solver.iteration, (double)std::sqrt(r2 / b2), (double)(xs / (long double)n),
                (double)x_max, (double)(xps / (long double)n), rows.c_str(), (int)amg->get("nullspace"), amg->get("coarse_shift"),
                ctx.counter("amg_applies"), ctx.counter("amg_projections"), ctx.counter("amg_fused_projections"));
    return converged ? 0 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "amg_nullspace_driver: %s\n", e.what());
    return 1;
  }
}
