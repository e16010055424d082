// The playground's Cahn-Hilliard time loop (source_apps/playground/Playground.cpp:133-210) with ONE operator object in
// place of the lambda: compiled against include/storm_hip/Storm.hpp only.
//
//   two_stage_driver <mesh prefix> <c0.f64> <steps> <out prefix>
//
// The playground's lambda (:153-167) is affine in c_in,
//     w_hat = f + sigma (c_in - c) - Gamma M c_in,    c_hat = c_in - tau M w_hat,
// and its linear part is the two-stage operator A x = x - tau M (sigma x - Gamma M x): `HipTwoStageOperator(mesh, -Gamma,
// sigma, -tau, 1)`.  What `solve_non_uniform` (Solver.hpp:271-292) does around the lambda is written out per step:
//     f <<= map(dF_dc, c);                        // :148
//     z = A(0) = -tau M (f - sigma c);            // the lambda at c_in = 0, with the existing statements
//     b = c - z;
//     c_hat <<= c;                                // the warm start, :150
//     solve<CgSolver>(c_hat, b, two_stage);       // :151, no callback: one cooperative kernel per solve on this mesh size
//     std::swap(c, c_hat);                        // :202
// Output as timestep_driver's: one JSON line per step on stdout ({"step", "iterations", "absolute_error",
// "relative_error", "converged", "seconds", "solves_logged"}), the field after every step in <out prefix>.step<k>.c.f64
// (raw doubles), and a last line with the context's counter "latency_solves" beside the totals.
#include <storm_hip/Storm.hpp>

#include <time.h>

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

using namespace Storm;

namespace {

const double tau = 1.0e-3, Gamma = 1.0e-4, sigma = 2.0;  // Playground.cpp:113

std::vector<real_t> read_f64(const std::string& path, std::size_t n) {
  std::vector<real_t> v(n);
  FILE* fh = std::fopen(path.c_str(), "rb");
  if (!fh || std::fread(v.data(), sizeof(real_t), n, fh) != n) throw std::runtime_error("cannot read " + path);
  std::fclose(fh);
  return v;
}
void write_f64(const std::string& path, const DeviceVector& v) {
  const std::vector<real_t> h = v.to_host();
  FILE* fh = std::fopen(path.c_str(), "wb");
  if (!fh || std::fwrite(h.data(), sizeof(real_t), h.size(), fh) != h.size()) throw std::runtime_error("cannot write " + path);
  std::fclose(fh);
}

// (the step's iteration count and errors are read from the reference's log line, as timestep_driver does)
struct SolveLog {
  std::size_t iterations = 0;
  real_t absolute_error = 0.0, relative_error = 0.0;
  std::size_t solves = 0;
} last_solve;

void cahn_hilliard_step(const StencilMatrix& mesh, const HipTwoStageOperator& two_stage, const DeviceVector& c, DeviceVector& c_hat,
                        DeviceVector& f, DeviceVector& w, DeviceVector& z, DeviceVector& b, bool& converged) {
  constexpr auto dF_dc = [](auto c) noexcept { return 2.0 * c * (c - 1.0) * (2.0 * c - 1.0); };
  f <<= map(dF_dc, c);

  w <<= f - sigma * c;
  fill_with(z, 0.0);
  stormDivGrad(mesh, z, -tau, w);
  b <<= c - z;

  c_hat <<= c;
  converged = solve<CgSolver>(c_hat, b, two_stage);
}

int run(const std::string& prefix, const std::string& c0_path, int steps, const std::string& out) {
  Context ctx(0);
  const HostMesh host_mesh = HostMesh::read_tetgen(prefix, 2);        // read_mesh_from_tetgen, Playground.cpp:252
  const StencilMatrix mesh = host_mesh.matrix(ctx, /*neumann=*/true);  // `interior_faces()` only, :119; built ONCE
  const HipTwoStageOperator two_stage(mesh, -Gamma, sigma, -tau, 1.0);
  const std::size_t n = host_mesh.num_cells();
  DeviceVector c(ctx, n), c_hat(ctx, n), f(ctx, n), w(ctx, n), z(ctx, n), b(ctx, n);
  const std::vector<real_t> c0 = read_f64(c0_path, n);
  c.upload(c0.data(), n);

  double total_time = 0.0;
  for (int time = 1; time <= steps; ++time) {
    struct timespec start, finish;
    ctx.sync();
    clock_gettime(CLOCK_MONOTONIC, &start);

    bool converged = false;
    cahn_hilliard_step(mesh, two_stage, c, c_hat, f, w, z, b, converged);

    ctx.sync();
    clock_gettime(CLOCK_MONOTONIC, &finish);
    double elapsed = (double)(finish.tv_sec - start.tv_sec);
    elapsed += (double)(finish.tv_nsec - start.tv_nsec) / 1000000000.0;
    total_time += elapsed;

    std::swap(c, c_hat);

    std::printf("{\"step\": %d, \"iterations\": %zu, \"absolute_error\": %.17g, \"relative_error\": %.17g, \"converged\": %s, "
                "\"seconds\": %.6f, \"solves_logged\": %zu}\n",
                time, last_solve.iterations, last_solve.absolute_error, last_solve.relative_error, converged ? "true" : "false",
                elapsed, last_solve.solves);
    write_f64(out + ".step" + std::to_string(time) + ".c.f64", c);
  }
  std::printf("{\"total_time\": %.6f, \"cells\": %zu, \"operator_builds\": 1, \"latency_solves\": %lld}\n", total_time, n,
              ctx.counter("latency_solves"));
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  try {
    set_log_sink([](const std::string& line) {
      unsigned long it = 0;
      double abs_err = 0.0, rel_err = 0.0;
      if (std::sscanf(line.c_str(), "n_iter: %lu, abs_err: %le, rel_err: %le", &it, &abs_err, &rel_err) == 3)
        last_solve.iterations = it, last_solve.absolute_error = abs_err, last_solve.relative_error = rel_err, ++last_solve.solves;
    });
    if (argc == 5) return run(argv[1], argv[2], std::atoi(argv[3]), argv[4]);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  std::fprintf(stderr, "usage: %s <mesh prefix> <c0.f64> <steps> <out prefix>\n", argv[0]);
  return 2;
}
