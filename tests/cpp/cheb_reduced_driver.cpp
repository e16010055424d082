// ChebyshevPreconditioner with reduced_records = true (the operator products read the matrix's fp32-weight companion
// records) through the reference's pre_op / pre_side hook, compiled against include/storm_hip/Storm.hpp only.
//
//   cheb_reduced_driver <fixture> <degree> <left|right> <reduced 0|1>
//
// <fixture>: a face-weight operator as raw little-endian data -- int64 n_cells, int64 n_faces, int64 inner[n_faces],
// int64 outer[n_faces], double w[n_faces] (both sides of a face), double diag_extra[n_cells] -- written by
// tests/test_gpu_reduced.py.  Solves -M x = 1 by CG on fp64 records and prints one JSON line.
#include <storm_hip/Storm.hpp>

#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

using namespace Storm;

template<class T>
static bool read_array(std::FILE* f, std::vector<T>& out, size_t count) {
  out.resize(count);
  return count == 0 || std::fread(out.data(), sizeof(T), count, f) == count;
}

int main(int argc, char** argv) {
  if (argc < 5) {
    std::fprintf(stderr, "usage: %s <fixture> <degree> <left|right> <reduced 0|1>\n", argv[0]);
    return 2;
  }
  const int degree = std::atoi(argv[2]);
  const std::string side_name = argv[3];
  if (side_name != "left" && side_name != "right") return 2;
  const bool reduced = std::atoi(argv[4]) != 0;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (f == nullptr) {
    std::fprintf(stderr, "error: cannot open %s\n", argv[1]);
    return 1;
  }
  int64_t head[2] = {0, 0};
  std::vector<int64_t> inner, outer;
  std::vector<real_t> w, diag;
  const bool ok = std::fread(head, sizeof(int64_t), 2, f) == 2 && head[0] > 0 && head[1] >= 0 &&
                  read_array(f, inner, (size_t)head[1]) && read_array(f, outer, (size_t)head[1]) &&
                  read_array(f, w, (size_t)head[1]) && read_array(f, diag, (size_t)head[0]);
  std::fclose(f);
  if (!ok) {
    std::fprintf(stderr, "error: short fixture %s\n", argv[1]);
    return 1;
  }
  try {
    Context ctx(0);
    const size_t n = (size_t)head[0];
    ctx.set_option("spmv_dict", 0);  // fp64 records: what reduced records are a companion of
    const StencilMatrix matrix = StencilMatrix::from_face_weights(ctx, n, 0, inner, outer, w, w, diag.data());
    ctx.set_option("spmv_dict", 4);
    DeviceVector b(ctx, n), x(ctx, n);
    fill_with(b, 1.0);
    CgSolver<DeviceVector> solver;
    auto pre = std::make_unique<ChebyshevPreconditioner>(degree);
    pre->reduced_records = reduced;
    const ChebyshevPreconditioner* cheb = pre.get();
    solver.pre_op = std::move(pre);
    solver.pre_side = side_name == "left" ? PreconditionerSide::Left : PreconditionerSide::Right;
    const HipStencilOperator op(matrix, -1.0, 0.0);  // A = -M
    const bool converged = solver.solve(x, b, op);
    ctx.sync();
    int64_t bytes = 0;
    detail::check(storm_hip_op_reduced_bytes(matrix.handle(), &bytes));
    std::printf("{\"converged\": %s, \"iterations\": %zu, \"x_norm2\": %.17g, \"pre_applies\": %zu, \"reduced\": %d, "
                "\"reduced_bytes\": %lld, \"cheb_reduced_applies\": %lld, \"op_reduced_builds\": %lld}\n",
                converged ? "true" : "false", solver.iteration, norm_2(x), solver.num_pre_applies, (int)cheb->get("reduced"),
                (long long)bytes, ctx.counter("cheb_reduced_applies"), ctx.counter("op_reduced_builds"));
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
