// k right-hand sides on one box through the block interface of include/storm_hip/Storm.hpp: a DeviceBlockVector per
// side (the reference's Field<Mesh, Index, Value, NumVars> layout, Feathers/Field.hpp:56-79), one solve_block_cg.
//
//   block_driver <n> <k>
//
// Column j of b holds b_j[i] = ((i * (j + 3)) % 17) - 8 (integers: any host reproduces them exactly).  Prints one JSON
// line with the per-column iteration counts and residual norms.
#include <storm_hip/Storm.hpp>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace Storm;

struct BoxMesh {
  std::vector<int64_t> inner, outer, b_cell;
  std::vector<real_t> coef, b_coef, volume;
  size_t n_cells = 0;
};

// n^3 unit cube, cell id (k*n + j)*n + i, faces cell-major +x,+y,+z, wall faces -x,+x,-y,+y,-z,+z
// (same synthetic mesh as stormruler_amd.mesh.structured_box / SURVEY.md 8d).
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

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: %s <n> <k>\n", argv[0]);
    return 2;
  }
  const int n = std::atoi(argv[1]);
  const size_t k = (size_t)std::atoi(argv[2]);
  try {
    Context ctx(0);
    ctx.set_option("spmv_dict", 0);  // fp64 records: what the block apply streams
    const BoxMesh mesh = make_box(n);
    const StencilMatrix matrix = StencilMatrix::from_faces(ctx, mesh.n_cells, 0, mesh.inner, mesh.outer, mesh.coef,
                                                           mesh.b_cell, mesh.b_coef, mesh.volume);
    const HipStencilOperator op(matrix, -1.0, 0.0);  // A = -L
    DeviceBlockVector b(ctx, mesh.n_cells, k), x(ctx, mesh.n_cells, k);
    std::vector<real_t> host(mesh.n_cells * k);
    for (size_t i = 0; i < mesh.n_cells; ++i)
      for (size_t j = 0; j < k; ++j) host[i * k + j] = (real_t)((i * (j + 3)) % 17) - 8.0;
    b.upload(host.data(), host.size());
    if (b.shape()[0] != mesh.n_cells || b.shape()[1] != k || b(1, k - 1) != host[k + k - 1]) return 3;
    const std::vector<BlockColumnResult> res = solve_block_cg(x, b, op);
    // every column's reported residual is the true one: |b_j - A x_j| from a block apply and a column dot
    DeviceBlockVector r(ctx, mesh.n_cells, k);
    op.mul_block(r, x);
    r -= b;
    const std::vector<real_t> rr = block_dot(r, r);
    std::printf("{\"n\": %d, \"k\": %zu, \"block_solves\": %lld, \"iterations\": [", n, k, ctx.counter("block_solves"));
    for (size_t j = 0; j < k; ++j) std::printf("%s%zu", j ? ", " : "", res[j].iteration);
    std::printf("], \"converged\": [");
    for (size_t j = 0; j < k; ++j) std::printf("%s%s", j ? ", " : "", res[j].converged ? "true" : "false");
    std::printf("], \"absolute_error\": [");
    for (size_t j = 0; j < k; ++j) std::printf("%s%.17g", j ? ", " : "", res[j].absolute_error);
    std::printf("], \"true_residual\": [");
    for (size_t j = 0; j < k; ++j) std::printf("%s%.17g", j ? ", " : "", std::sqrt(rr[j]));
    std::printf("]}\n");
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
