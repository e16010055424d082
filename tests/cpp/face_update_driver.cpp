// A time loop whose operator changes every step and never leaves the device, compiled against include/storm_hip/Storm.hpp
// only: variable-mobility diffusion (I - dt L_{M(c^n)}) c^{n+1} = c^n on a 6 x 5 x 4 box with M(c) = 0.1 + c^2 and the
// arithmetic face mean, no-flux walls.  Per step: cells_to_faces(c), two map statements form the face weights,
// set_face_weights refreshes the operator's records, CG solves.  The operator is created once, outside the loop.
//
//   face_update_driver [steps = 5]
//
// prints one JSON line per step (iterations, |w|_2 of the face weights, |c^{n+1}|_2): tests/test_gpu_face_update.py holds
// them against the same loop written with stormruler_amd.api.
#include <storm_hip/Storm.hpp>

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace Storm;

int main(int argc, char** argv) {
  const int steps = argc > 1 ? std::atoi(argv[1]) : 5;
  const int nx = 6, ny = 5, nz = 4;
  const real_t dt = 0.025;
  try {
    Context ctx(0);
    const size_t n = (size_t)nx * ny * nz;
    // faces cell by cell (+x, +y, +z of each); g_f = A_f / (d_f V) = 1 / h^2 of the face's direction
    std::vector<int64_t> inner, outer;
    std::vector<real_t> g;
    for (int k = 0; k < nz; ++k)
      for (int j = 0; j < ny; ++j)
        for (int i = 0; i < nx; ++i) {
          const int64_t c = i + nx * (j + (int64_t)ny * k);
          if (i + 1 < nx) inner.push_back(c), outer.push_back(c + 1), g.push_back(36.0);
          if (j + 1 < ny) inner.push_back(c), outer.push_back(c + nx), g.push_back(25.0);
          if (k + 1 < nz) inner.push_back(c), outer.push_back(c + (int64_t)nx * ny), g.push_back(16.0);
        }
    const size_t n_faces = inner.size();
    std::vector<real_t> c0(n), zeros(n_faces, 0.0);
    for (size_t i = 0; i < n; ++i) c0[i] = (real_t)((i * 37) % 101) / 101.0;
    StencilMatrix L = StencilMatrix::from_face_weights_updatable(ctx, n, 0, inner, outer, zeros, zeros);
    if (L.face_count() != n_faces) return 1;
    DeviceVector c(ctx, n), c_in(ctx, n_faces), c_out(ctx, n_faces), m(ctx, n_faces), w(ctx, n_faces), gf(ctx, n_faces);
    c.upload(c0.data(), n);
    gf.upload(g.data(), n_faces);
    const HipStencilOperator op(L, -dt, 1.0);  // A = I - dt L
    for (int step = 0; step < steps; ++step) {
      L.cells_to_faces(c, &c_in, &c_out);
      m <<= map([](auto a, auto b) { return 0.5 * ((0.1 + a * a) + (0.1 + b * b)); }, c_in, c_out);
      w <<= map([](auto mf, auto gg) { return mf * gg; }, m, gf);
      L.set_face_weights(w, w);
      DeviceVector x(ctx, n);
      CgSolver<DeviceVector> solver;
      solver.absolute_error_tolerance = 0.0;
      solver.relative_error_tolerance = 1.0e-12;
      const bool converged = solver.solve(x, c, op);
      c <<= 1.0 * x;
      std::printf("{\"step\": %d, \"converged\": %s, \"iterations\": %zu, \"w_norm2\": %.17g, \"c_norm2\": %.17g}\n", step,
                  converged ? "true" : "false", (size_t)solver.iteration, norm_2(w), norm_2(c));
    }
    std::printf("{\"op_face_updates\": %lld}\n", ctx.counter("op_face_updates"));
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
