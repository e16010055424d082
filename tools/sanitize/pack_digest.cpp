// The host half of the operator build (csrc/op_pack.hip) on a fixed corpus, no GPU: one line per case with a 64-bit
// FNV-1a over a canonical serialisation of the OpImage -- every scalar, then (name, length, bytes) of every array, in
// a fixed order.  tests/test_op_pack.py holds the lines against tests/golden/op_pack_digests.json for several thread
// counts; tools/sanitize/run.sh runs the same corpus under the sanitizers.
//   pack_digest              the corpus, one line per case on stdout
//   pack_digest -v           ... and what each case came out as on stderr
//   pack_digest --time N R   R builds of the N^3 box, milliseconds per build on stdout
// Build: g++ -std=c++17 -O1 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude -Istormruler_amd/csrc
//        tools/sanitize/pack_digest.cpp -x c++ stormruler_amd/csrc/op_pack.hip -lpthread
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "common.hpp"

namespace storm {
static char g_err[512];
void set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
}
}  // namespace storm
using namespace storm;

namespace {

struct Fnv {
  uint64_t h = 0xcbf29ce484222325ull;
  void bytes(const void *p, size_t n) {
    for (size_t i = 0; i < n; ++i) h = (h ^ ((const unsigned char *)p)[i]) * 0x100000001b3ull;
  }
  void scalar(const char *name, int64_t v) {
    bytes(name, strlen(name) + 1);
    bytes(&v, 8);
  }
  template <class T>
  void array(const char *name, const std::vector<T> &a) {
    scalar(name, (int64_t)a.size());
    bytes(a.data(), sizeof(T) * a.size());
  }
};

uint64_t digest(const OpImage &m) {
  Fnv f;
  f.scalar("n_rows", m.n_rows), f.scalar("n_halo", m.n_halo), f.scalar("nnz", m.nnz), f.scalar("n_slices", m.n_slices);
  f.scalar("max_row_len", m.max_row_len), f.scalar("ell_slots", m.ell_slots), f.scalar("uniform_width", m.uniform_width);
  f.scalar("pair", m.pair), f.scalar("bnd_width", m.bnd_width), f.scalar("canon_k", m.canon_k), f.scalar("canon_m1", m.canon_m1);
  for (int k = 0; k < 7; ++k) f.scalar("canon_off", m.canon_off[k]);
  f.scalar("dict_size", m.dict_size), f.scalar("offs_size", m.offs_size), f.scalar("spw", m.spw);
  f.scalar("tail_rows", m.tail_rows), f.scalar("tail_nnz", m.tail_nnz), f.scalar("pack_bytes", m.pack_bytes);
  f.array("slice_off", m.slice_off), f.array("pack", m.pack), f.array("dict", m.dict), f.array("offs", m.offs);
  f.array("rec_idx", m.rec_idx), f.array("rec_words", m.rec_words), f.array("bnd_pack", m.bnd_pack);
  f.array("tail_row", m.tail_row), f.array("tail_ptr", m.tail_ptr), f.array("tail_col", m.tail_col), f.array("tail_val", m.tail_val);
  f.array("interior", m.interior), f.array("boundary", m.boundary), f.array("lat_off", m.lat_off), f.array("lat_pack", m.lat_pack);
  return f.h;
}

bool g_verbose = false;
void report(const std::string &name, const PackOptions &o, int st, const OpImage &m) {
  if (st != STORM_HIP_OK) {
    printf("%s dict=%d mixed=%d status=%d %s\n", name.c_str(), (int)o.spmv_dict, (int)o.spmv_mixed, st, g_err);
    return;
  }
  printf("%s dict=%d mixed=%d %016llx\n", name.c_str(), (int)o.spmv_dict, (int)o.spmv_mixed, (unsigned long long)digest(m));
  if (g_verbose)
    fprintf(stderr, "%s dict=%d mixed=%d: pair %d width %d values %d offsets %d words %zu index %zu boundary records %zu tail %lld/%lld "
            "slices %zu+%zu latency %zu\n", name.c_str(), (int)o.spmv_dict, (int)o.spmv_mixed, m.pair, m.uniform_width, m.dict_size,
            m.offs_size, m.rec_words.size(), m.rec_idx.size(), m.bnd_pack.size(), (long long)m.tail_rows, (long long)m.tail_nnz,
            m.interior.size(), m.boundary.size(), m.lat_pack.size());
}

struct Rng {  // splitmix64
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  double unit() { return (double)(next() >> 11) / 9007199254740992.0; }
};

// The faces of an nx x ny x nz box, cell by cell (+x, +y, +z of each): a row then lists its neighbours in the order
// -nx ny, -nx, -1, +1, +nx, +nx ny.  Planes [0, owned_planes) are owned; the plane behind them is the halo, numbered
// behind the owned rows.  `id`: a renumbering of the cells, or null.
struct Faces {
  int64_t n_owned = 0, n_halo = 0;
  std::vector<int64_t> inner, outer;
  std::vector<double> w_inner, w_outer, diag;
};
enum Weights { BY_DIRECTION, BY_POSITION, DISTINCT };
Faces box_faces(int nx, int ny, int nz, int owned_planes, Weights kind, const int64_t *id = nullptr) {
  Faces F;
  const int64_t plane = (int64_t)nx * ny;
  F.n_owned = plane * owned_planes, F.n_halo = owned_planes < nz ? plane : 0;
  F.diag.assign((size_t)F.n_owned, 0.0);
  Rng rng{12345};
  const double by_dir[3] = {1.0, 2.0, 0.5};
  for (int k = 0; k < owned_planes; ++k)
    for (int j = 0; j < ny; ++j)
      for (int i = 0; i < nx; ++i) {
        const int64_t c = i + nx * (j + (int64_t)ny * k);
        const int at[3] = {i, j, k}, lim[3] = {nx, ny, nz};
        const int64_t stride[3] = {1, nx, plane};
        for (int d = 0; d < 3; ++d) {
          if (at[d] == 0 || at[d] + 1 == lim[d]) F.diag[(size_t)(id ? id[c] : c)] -= by_dir[d];  // a wall
          if (at[d] + 1 == lim[d]) continue;
          const int64_t nb = c + stride[d];
          F.inner.push_back(id ? id[c] : c), F.outer.push_back(id ? id[nb] : nb);
          double wi = by_dir[d], wo = by_dir[d];
          if (kind == BY_POSITION) wi = 0.25 * (double)(1 + (c * 7 + d) % 13), wo = 0.25 * (double)(1 + (nb * 5 + d) % 11);
          if (kind == DISTINCT) wi = rng.unit(), wo = rng.unit();
          F.w_inner.push_back(wi), F.w_outer.push_back(wo);
        }
      }
  return F;
}

void run_faces(const std::string &name, const Faces &F, PackOptions o, bool with_diag = true) {
  for (int d = 0; d <= 4; ++d) {
    o.spmv_dict = d;
    OpImage m;
    const int st = op_pack_from_face_weights(o, F.n_owned, F.n_halo, (int64_t)F.inner.size(), F.inner.data(), F.outer.data(),
                                             F.w_inner.data(), F.w_outer.data(), with_diag ? F.diag.data() : nullptr, &m);
    report(name, o, st, m);
  }
}

void run_csr(const std::string &name, int64_t n, const std::vector<int64_t> &rp, const std::vector<int64_t> &col,
             const std::vector<double> &val, PackOptions o) {
  for (int d = 0; d <= 4; ++d) {
    o.spmv_dict = d;
    OpImage m;
    report(name, o, op_pack_csr(o, n, 0, rp.data(), col.data(), val.data(), &m), m);
  }
}

void csr_cases() {
  const int64_t n = 200;
  {  // row lengths 1 .. 5 and the diagonal
    std::vector<int64_t> rp(1, 0), col;
    std::vector<double> val;
    for (int64_t i = 0; i < n; ++i) {
      col.push_back(i), val.push_back(-4.0);
      for (int k = 0; k <= i % 5; ++k) col.push_back((i + 1 + 3 * k) % n), val.push_back(0.5 * (double)(1 + k));
      rp.push_back((int64_t)col.size());
    }
    run_csr("csr_200_lengths_1_to_5", n, rp, col, val, PackOptions());
  }
  {  // five entries per row, the offsets of even and odd rows disjoint: a pair would merge to 10, format 2 is the end
    std::vector<int64_t> rp(1, 0), col;
    std::vector<double> val;
    for (int64_t i = 0; i < n; ++i) {
      for (int k = 0; k < 5; ++k) col.push_back((i + 1 + i % 2 + 3 * k) % n), val.push_back(0.5 * (double)(1 + k));
      rp.push_back((int64_t)col.size());
    }
    run_csr("csr_200_pairs_disjoint", n, rp, col, val, PackOptions());
  }
  {  // three entries per row but for a 40-entry and a 70-entry row, ELL cap 8: the CSR tail, no latency copy
    std::vector<int64_t> rp(1, 0), col;
    std::vector<double> val;
    for (int64_t i = 0; i < n; ++i) {
      const int len = i == 17 ? 40 : i == 150 ? 70 : 3;
      for (int k = 0; k < len; ++k) col.push_back((i + 1 + 2 * k) % n), val.push_back(1.0 + 0.125 * (double)((i + k) % 9));
      rp.push_back((int64_t)col.size());
    }
    PackOptions o;
    o.ell_cap = 8;
    run_csr("csr_200_rows_of_40_and_70_cap_8", n, rp, col, val, o);
  }
}

// One cell with `n_star` faces, `between` chain faces of other cells after each of them.
void star_case(const std::string &name, int n_star, int between) {
  Faces F;
  F.n_owned = n_star + 1;
  for (int f = 0; f < n_star; ++f) {
    F.inner.push_back(0), F.outer.push_back(1 + f), F.w_inner.push_back(1.0 + (double)(f % 3)), F.w_outer.push_back(2.0);
    for (int q = 0; q < between; ++q) {
      const int64_t a = 1 + (f + q) % n_star, b = 1 + (f + q + 1) % n_star;
      F.inner.push_back(a), F.outer.push_back(b), F.w_inner.push_back(0.5), F.w_outer.push_back(0.25);
    }
  }
  run_faces(name, F, PackOptions(), false);
}

void mesh_case() {  // a 12 x 9 grid of 0.25 x 0.5 cells through the geometric entry point
  const int nx = 12, ny = 9;
  const double hx = 0.25, hy = 0.5;
  std::vector<int64_t> inner, outer, b_cell;
  std::vector<double> area, center, b_area, b_center, volume((size_t)nx * ny, hx * hy);
  for (int j = 0; j < ny; ++j)
    for (int i = 0; i < nx; ++i) center.push_back((i + 0.5) * hx), center.push_back((j + 0.5) * hy);
  for (int j = 0; j < ny; ++j)
    for (int i = 0; i < nx; ++i) {
      const int64_t c = i + (int64_t)nx * j;
      if (i + 1 < nx) inner.push_back(c), outer.push_back(c + 1), area.push_back(hy);
      if (j + 1 < ny) inner.push_back(c), outer.push_back(c + nx), area.push_back(hx);
      auto wall = [&](double a, double x, double y) { b_cell.push_back(c), b_area.push_back(a), b_center.push_back(x), b_center.push_back(y); };
      if (i == 0) wall(hy, 0.0, (j + 0.5) * hy);
      if (i + 1 == nx) wall(hy, nx * hx, (j + 0.5) * hy);
      if (j == 0) wall(hx, (i + 0.5) * hx, 0.0);
      if (j + 1 == ny) wall(hx, (i + 0.5) * hx, ny * hy);
    }
  PackOptions o;
  for (int d = 0; d <= 4; ++d) {
    o.spmv_dict = d;
    OpImage m;
    report("mesh_12x9", o, op_pack_from_mesh(o, nx * ny, 0, 2, (int64_t)inner.size(), inner.data(), outer.data(), area.data(), center.data(),
                                              (int64_t)b_cell.size(), b_cell.data(), b_area.data(), b_center.data(), volume.data(), &m), m);
  }
}

int time_box(int n, int reps) {
  const Faces F = box_faces(n, n, n, n, BY_DIRECTION);
  for (int r = 0; r < reps; ++r) {
    OpImage m;
    const auto t0 = std::chrono::steady_clock::now();
    const int st = op_pack_from_face_weights(PackOptions(), F.n_owned, 0, (int64_t)F.inner.size(), F.inner.data(), F.outer.data(),
                                             F.w_inner.data(), F.w_outer.data(), F.diag.data(), &m);
    printf("%.1f\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    if (st != STORM_HIP_OK || m.pair != 2) return 1;
  }
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc > 3 && !strcmp(argv[1], "--time")) return time_box(atoi(argv[2]), atoi(argv[3]));
  g_verbose = argc > 1 && !strcmp(argv[1], "-v");
  run_faces("box_3x1x1", box_faces(3, 1, 1, 1, BY_DIRECTION), PackOptions());
  run_faces("box_7x5x3", box_faces(7, 5, 3, 3, BY_DIRECTION), PackOptions());
  run_faces("box_16x10x6", box_faces(16, 10, 6, 6, BY_DIRECTION), PackOptions());
  run_faces("box_130x3x2_weights_by_position", box_faces(130, 3, 2, 2, BY_POSITION), PackOptions());
  for (int mixed : {1, 0}) {  // the lower planes of a box, the plane above them as halo columns
    PackOptions o;
    o.spmv_mixed = mixed;
    run_faces("slab_20x12x5_of_9", box_faces(20, 12, 9, 5, BY_DIRECTION), o);
  }
  {
    std::vector<int64_t> id(16 * 10 * 6);
    for (size_t i = 0; i < id.size(); ++i) id[i] = (int64_t)i;
    Rng rng{2024};
    for (size_t i = id.size() - 1; i > 0; --i) std::swap(id[i], id[(size_t)(rng.next() % (i + 1))]);
    run_faces("box_16x10x6_renumbered", box_faces(16, 10, 6, 6, BY_DIRECTION, id.data()), PackOptions());
  }
  run_faces("box_7x5x3_distinct_weights", box_faces(7, 5, 3, 3, DISTINCT), PackOptions());
  csr_cases();
  run_faces("grid_12x9", box_faces(12, 9, 1, 1, BY_DIRECTION), PackOptions(), false);
  star_case("star_300", 300, 0);
  star_case("star_300_spread", 300, 1);
  mesh_case();
  run_faces("empty", Faces(), PackOptions());
  return 0;
}
