// A time loop whose operator AND multigrid preconditioner are refreshed on the device every step, compiled against
// include/storm_hip/Storm.hpp only: -L_w x = 1 on the n^3 box with Dirichlet walls (wall weight 2), the face weights
// replaced before every solve.  The operator and the hierarchy are created once, outside the loop; per step:
// new weights into a face vector, set_face_weights, AmgPreconditioner::refresh, a CG solve.
//
//   amg_refresh_driver [n = 16] [steps = 3]
//
// Step s = 1, 2, ... puts 1 + ((7 f + 3 s) mod 16) / 16 on face f (exact in binary).  Prints one JSON line: the iteration
// counts, "amg_refreshes" and the level sizes; tests/test_gpu_amg_refresh.py holds them against the same loop written with
// stormruler_amd.api.
#include <storm_hip/Storm.hpp>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

using namespace Storm;

int main(int argc, char** argv) {
  const int n = argc > 1 ? std::atoi(argv[1]) : 16;
  const int steps = argc > 2 ? std::atoi(argv[2]) : 3;
  try {
    Context ctx(0);
    const size_t n_cells = (size_t)n * n * n;
    // cell id (k n + j) n + i, faces cell-major +x, +y, +z (stormruler_amd.mesh.structured_box); a wall face adds -2 to
    // the diagonal term of its cell
    std::vector<int64_t> inner, outer;
    std::vector<real_t> diag_extra(n_cells, 0.0);
    for (int k = 0; k < n; ++k)
      for (int j = 0; j < n; ++j)
        for (int i = 0; i < n; ++i) {
          const int64_t c = ((int64_t)k * n + j) * n + i;
          if (i < n - 1) inner.push_back(c), outer.push_back(c + 1);
          if (j < n - 1) inner.push_back(c), outer.push_back(c + n);
          if (k < n - 1) inner.push_back(c), outer.push_back(c + (int64_t)n * n);
          const int idx[3] = {i, j, k};
          for (int ax = 0; ax < 3; ++ax) diag_extra[(size_t)c] -= 2.0 * ((idx[ax] == 0) + (idx[ax] == n - 1));
        }
    const size_t n_faces = inner.size();
    std::vector<real_t> w_host(n_faces, 1.0);
    StencilMatrix L = StencilMatrix::from_face_weights_updatable(ctx, n_cells, 0, inner, outer, w_host, w_host, diag_extra.data());
    DeviceVector b(ctx, n_cells), w(ctx, n_faces), de(ctx, n_cells);
    fill_with(b, 1.0);
    de.upload(diag_extra.data(), n_cells);
    const HipStencilOperator op(L, -1.0, 0.0);  // A = -L
    CgSolver<DeviceVector> solver;
    auto pre = std::make_unique<AmgPreconditioner>();
    pre->refreshable = true;
    AmgPreconditioner* amg = pre.get();
    solver.pre_op = std::move(pre);
    solver.pre_side = PreconditionerSide::Right;
    DeviceVector x0(ctx, n_cells);
    amg->build(x0, b, op);  // the setup, once
    std::string its, conv;
    for (int s = 1; s <= steps; ++s) {
      for (size_t f = 0; f < n_faces; ++f) w_host[f] = 1.0 + std::fmod(7.0 * (real_t)f + 3.0 * s, 16.0) / 16.0;
      w.upload(w_host.data(), n_faces);
      L.set_face_weights(w, w, &de);
      amg->refresh();
      DeviceVector x(ctx, n_cells);
      const bool converged = solver.solve(x, b, op);
      its += (its.empty() ? "" : ", ") + std::to_string((long long)solver.iteration);
      conv += (conv.empty() ? "" : ", ") + std::string(converged ? "1" : "0");
    }
    ctx.sync();
    std::string rows;
    for (int64_t r : amg->level_rows()) rows += (rows.empty() ? "" : ", ") + std::to_string((long long)r);
    std::printf("{\"n\": %d, \"converged\": [%s], \"iterations\": [%s], \"amg_refreshes\": %lld, \"level_rows\": [%s], "
                "\"refresh_bytes\": %.17g}\n", n, conv.c_str(), its.c_str(), ctx.counter("amg_refreshes"), rows.c_str(),
                amg->get("refresh_bytes"));
  } catch (const std::exception& e) {
    std::fprintf(stderr, "amg_refresh_driver: %s\n", e.what());
    return 1;
  }
  return 0;
}
