// MixedCgSolver (fp32 inner iterations on the fp32-weight companion records under fp64 refinement) on a box, compiled
// against include/storm_hip/Storm.hpp only.
//
//   mixed_cg_driver <n> <tolerance> <keep_direction 0|1>
//
// The 7-point operator on n^3 cells with Dirichlet walls as a face-weight operator (weight 1 per face, 2 per wall face on the
// diagonal), A = -M, b = 1.  Prints one JSON line: the outer steps, the inner iterations and the final TRUE residual,
// recomputed here with the fp64 operator.
#include <storm_hip/Storm.hpp>

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace Storm;

int main(int argc, char** argv) {
  if (argc < 4) {
    std::fprintf(stderr, "usage: %s <n> <tolerance> <keep_direction 0|1>\n", argv[0]);
    return 2;
  }
  const int64_t nx = std::atoll(argv[1]);
  const double tol = std::atof(argv[2]);
  if (nx < 2 || nx > 256 || !(tol > 0.0)) return 2;
  const size_t n = (size_t)(nx * nx * nx);
  std::vector<int64_t> inner, outer;
  std::vector<real_t> diag(n, -12.0);  // -2 per wall face; every interior face found below gives 2 back
  for (int64_t k = 0; k < nx; ++k)
    for (int64_t j = 0; j < nx; ++j)
      for (int64_t i = 0; i < nx; ++i) {
        const int64_t c = i + nx * (j + nx * k);
        const int64_t nb[3] = {i + 1 < nx ? c + 1 : -1, j + 1 < nx ? c + nx : -1, k + 1 < nx ? c + nx * nx : -1};
        for (const int64_t o : nb)
          if (o >= 0) inner.push_back(c), outer.push_back(o), diag[(size_t)c] += 2.0, diag[(size_t)o] += 2.0;
      }
  const std::vector<real_t> w(inner.size(), 1.0);
  try {
    Context ctx(0);
    ctx.set_option("spmv_dict", 0);  // fp64 records: what the companion records are a companion of
    const StencilMatrix matrix = StencilMatrix::from_face_weights(ctx, n, 0, inner, outer, w, w, diag.data());
    ctx.set_option("spmv_dict", 4);
    const HipStencilOperator op(matrix, -1.0, 0.0);  // A = -M
    op.build_reduced();
    DeviceVector b(ctx, n), x(ctx, n), t(ctx, n);
    fill_with(b, 1.0);
    MixedCgSolver solver;
    solver.absolute_error_tolerance = solver.relative_error_tolerance = tol;
    solver.keep_direction = std::atoi(argv[3]) != 0;
    const bool converged = solver.solve(x, b, op);
    op.mul(t, x);
    t <<= b - t;
    const real_t residual = norm_2(t);
    ctx.sync();
    std::printf("{\"converged\": %s, \"outer_steps\": %zu, \"inner_iterations\": %zu, \"fp64_iterations\": %zu, "
                "\"finished_fp64\": %d, \"iterations\": %zu, \"initial_error\": %.17g, \"absolute_error\": %.17g, "
                "\"true_residual\": %.17g, \"mixed_solves\": %lld}\n",
                converged ? "true" : "false", solver.outer_steps, solver.inner_iterations, solver.fp64_iterations,
                solver.finished_fp64, solver.iteration, solver.initial_error, solver.absolute_error, residual,
                ctx.counter("mixed_solves"));
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
