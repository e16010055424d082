// The source map of an updatable operator (csrc/op_pack.hip, PackOptions::updatable) checked on the host, no GPU: for the
// shapes of tests/test_gpu_face_update.py and 1, 3 and 7 build threads (chunks of 5 faces / rows, so that small inputs
// thread too)
//   - every non-padding slot and every CSR-tail entry decodes to a face f and a side such that the slot's row and column
//     are that face's two cells in the right order and its value is w_side[f], and a row meets its faces in face order;
//   - every face side whose row is owned appears exactly once, every other never;
//   - padding slots hold -1, weight +0.0 and the row's own index as column;
//   - the records, offsets, lists and tail are those of a plain pack under spmv_dict = 0 byte for byte, no latency copy is
//     formed, and a pack without the flag carries no map at all.
// tests/test_op_srcmap.py builds it plain and under the sanitizers and runs both.
//   pack_srcmap [repository root]     one line per case, "srcmap: ok" at the end; exit status 1 on the first failure
// Build: g++ -std=c++17 -O1 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude -Istormruler_amd/csrc
//        tools/sanitize/pack_srcmap.cpp -x c++ stormruler_amd/csrc/op_pack.hip -lpthread
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "common.hpp"
#include "op_layout.hpp"

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

struct Rng {  // splitmix64
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  double sym() { return 2.0 * ((double)(next() >> 11) / 9007199254740992.0) - 1.0; }  // uniform(-1, 1)
};

struct Faces {
  int64_t n_owned = 0, n_halo = 0;
  std::vector<int64_t> inner, outer;
  std::vector<double> w_inner, w_outer, diag;
};

void random_weights(Faces &F, uint64_t seed) {
  Rng rng{seed};
  F.w_inner.resize(F.inner.size()), F.w_outer.resize(F.inner.size()), F.diag.resize((size_t)F.n_owned);
  for (size_t f = 0; f < F.inner.size(); ++f) F.w_inner[f] = rng.sym(), F.w_outer[f] = rng.sym();
  for (double &d : F.diag) d = rng.sym();
}

// the faces of an nx x ny x nz box, cell by cell (+x, +y, +z of each); planes [0, owned_planes) owned, the next one halo
Faces box(int nx, int ny, int nz, int owned_planes) {
  Faces F;
  const int64_t plane = (int64_t)nx * ny;
  F.n_owned = plane * owned_planes, F.n_halo = owned_planes < nz ? plane : 0;
  for (int k = 0; k < owned_planes; ++k)
    for (int j = 0; j < ny; ++j)
      for (int i = 0; i < nx; ++i) {
        const int64_t c = i + nx * (j + (int64_t)ny * k);
        if (i + 1 < nx) F.inner.push_back(c), F.outer.push_back(c + 1);
        if (j + 1 < ny) F.inner.push_back(c), F.outer.push_back(c + nx);
        if (k + 1 < nz) F.inner.push_back(c), F.outer.push_back(c + plane);
      }
  return F;
}

// ... its faces randomly permuted and randomly flipped
void shuffle_faces(Faces &F, uint64_t seed) {
  Rng rng{seed};
  for (size_t f = F.inner.size(); f > 1; --f) {
    const size_t g = (size_t)(rng.next() % f);
    std::swap(F.inner[f - 1], F.inner[g]), std::swap(F.outer[f - 1], F.outer[g]);
  }
  for (size_t f = 0; f < F.inner.size(); ++f)
    if (rng.next() & 1) std::swap(F.inner[f], F.outer[f]);
}

// the triangles of a Triangle .ele file, a face between two that share an edge (rows of at most 3 neighbours)
bool triangle_faces(const std::string &ele, Faces &F) {
  std::ifstream in(ele);
  int64_t n = 0, per = 0, attrs = 0;
  if (!(in >> n >> per >> attrs) || per != 3) return false;
  std::map<std::pair<int64_t, int64_t>, int64_t> first;  // edge -> the first triangle that has it
  for (int64_t t = 0; t < n; ++t) {
    int64_t id, v[3], skip;
    if (!(in >> id >> v[0] >> v[1] >> v[2])) return false;
    for (int64_t a = 0; a < attrs; ++a) in >> skip;
    for (int e = 0; e < 3; ++e) {
      const std::pair<int64_t, int64_t> key(std::min(v[e], v[(e + 1) % 3]), std::max(v[e], v[(e + 1) % 3]));
      auto it = first.find(key);
      if (it == first.end()) first[key] = t;
      else F.inner.push_back(it->second), F.outer.push_back(t);
    }
  }
  F.n_owned = n;
  return true;
}

Faces ring_and_hub(int n_ring) {
  Faces F;
  F.n_owned = n_ring + 1;
  for (int i = 0; i < n_ring; ++i) {
    F.inner.push_back(i), F.outer.push_back((i + 1) % n_ring);
    F.inner.push_back(n_ring), F.outer.push_back(i);  // the hub
  }
  return F;
}

uint64_t bits(double v) {
  uint64_t b;
  memcpy(&b, &v, 8);
  return b;
}

int g_failures = 0;
#define CHECK(cond, ...)                       \
  do {                                         \
    if (!(cond)) {                             \
      fprintf(stderr, "%s: ", name.c_str());   \
      fprintf(stderr, __VA_ARGS__);            \
      fprintf(stderr, "\n");                   \
      ++g_failures;                            \
      return;                                  \
    }                                          \
  } while (0)

void check_case(const std::string &name, const Faces &F, int64_t ell_cap, bool with_diag) {
  const int64_t n = F.n_owned, n_faces = (int64_t)F.inner.size();
  PackOptions o;
  o.ell_cap = ell_cap;
  OpImage off_img;  // without the flag: no map
  int st = op_pack_from_face_weights(o, n, F.n_halo, n_faces, F.inner.data(), F.outer.data(), F.w_inner.data(), F.w_outer.data(),
                                     with_diag ? F.diag.data() : nullptr, &off_img);
  CHECK(st == STORM_HIP_OK, "plain pack failed: %s", g_err);
  CHECK(off_img.updatable == 0 && off_img.n_faces == 0 && off_img.src.empty() && off_img.tail_src.empty() &&
            off_img.face_inner.empty() && off_img.face_outer.empty(), "a pack without the flag carries a source map");
  PackOptions o0 = o;
  o0.spmv_dict = 0, o0.latency_path = 0;
  OpImage ref;  // what the records of an updatable operator must equal
  st = op_pack_from_face_weights(o0, n, F.n_halo, n_faces, F.inner.data(), F.outer.data(), F.w_inner.data(), F.w_outer.data(),
                                 with_diag ? F.diag.data() : nullptr, &ref);
  CHECK(st == STORM_HIP_OK, "format-0 pack failed: %s", g_err);
  PackOptions ou = o;
  ou.updatable = 1;
  OpImage m;
  st = op_pack_from_face_weights(ou, n, F.n_halo, n_faces, F.inner.data(), F.outer.data(), F.w_inner.data(), F.w_outer.data(),
                                 with_diag ? F.diag.data() : nullptr, &m);
  CHECK(st == STORM_HIP_OK, "updatable pack failed: %s", g_err);
  CHECK(m.updatable == 1 && m.n_faces == n_faces, "flag / face count not carried");
  CHECK(m.dict_size == 0 && m.offs_size == 0 && m.pair == 0 && m.dict.empty() && m.offs.empty() && m.rec_idx.empty() &&
            m.rec_words.empty() && m.bnd_pack.empty(), "an updatable operator took a compact format");
  CHECK(m.lat_off.empty() && m.lat_pack.empty(), "an updatable operator formed a latency copy");
  CHECK(m.pack == ref.pack && m.slice_off == ref.slice_off && m.tail_row == ref.tail_row && m.tail_ptr == ref.tail_ptr &&
            m.tail_col == ref.tail_col && m.tail_val == ref.tail_val && m.interior == ref.interior && m.boundary == ref.boundary &&
            m.n_slices == ref.n_slices && m.ell_slots == ref.ell_slots && m.uniform_width == ref.uniform_width && m.spw == ref.spw &&
            m.nnz == ref.nnz && m.max_row_len == ref.max_row_len && m.tail_rows == ref.tail_rows && m.tail_nnz == ref.tail_nnz &&
            m.pack_bytes == ref.pack_bytes, "the records differ from those of a plain pack under spmv_dict = 0");
  CHECK((int64_t)m.face_inner.size() == n_faces && (int64_t)m.face_outer.size() == n_faces, "face arrays");
  for (int64_t f = 0; f < n_faces; ++f)
    CHECK(m.face_inner[(size_t)f] == F.inner[(size_t)f] && m.face_outer[(size_t)f] == F.outer[(size_t)f], "face %lld's cells", (long long)f);
  CHECK(m.tail_src.size() == m.tail_val.size(), "tail_src has %zu entries, tail_val %zu", m.tail_src.size(), m.tail_val.size());
  CHECK((int64_t)m.src.size() == m.ell_slots, "src has %zu entries for %lld slots", m.src.size(), (long long)m.ell_slots);

  std::vector<int> seen((size_t)(2 * n_faces), 0);
  std::vector<int64_t> last_face((size_t)n, -1);  // face order inside a row
  bool ok = true;
  auto entry = [&](int64_t r, int id, int col, double val, const char *where) {
    if (id < 0 || id >= 2 * n_faces || r >= n) {
      fprintf(stderr, "%s: %s of row %lld has source id %d\n", name.c_str(), where, (long long)r, id);
      return ok = false;
    }
    const int64_t f = id >> 1;
    const bool side = id & 1;
    const int64_t row = side ? F.outer[(size_t)f] : F.inner[(size_t)f], other = side ? F.inner[(size_t)f] : F.outer[(size_t)f];
    const double w = side ? F.w_outer[(size_t)f] : F.w_inner[(size_t)f];
    if (row != r || other != col || bits(w) != bits(val) || f <= last_face[(size_t)r]) {
      fprintf(stderr, "%s: %s of row %lld, column %d: id %d = face %lld side %d joins (%lld -> %lld), after face %lld\n", name.c_str(),
              where, (long long)r, col, id, (long long)f, (int)side, (long long)row, (long long)other, (long long)last_face[(size_t)r]);
      return ok = false;
    }
    last_face[(size_t)r] = f;
    ++seen[(size_t)id];
    return true;
  };
  for (int64_t s = 0; s < m.n_slices && ok; ++s) {
    const int64_t base = m.slice_off[(size_t)s];
    const int W = (int)((m.slice_off[(size_t)s + 1] - base - kExtBytes) / kSlotBytes);
    const char *rec = m.pack.data() + base;
    const int *c_ = reinterpret_cast<const int *>(rec + kExtBytes);
    const double *v_ = reinterpret_cast<const double *>(rec + kExtBytes + (int64_t)W * (kWave * 4));
    const int *s_ = m.src.data() + (base - s * kExtBytes) / (kSlotBytes / kWave);
    const int np2 = W >> 1;
    for (int k = 0; k < W && ok; ++k)  // slot by slot, so that a row meets its entries in their order
      for (int l = 0; l < kWave && ok; ++l) {
        const int64_t r = s * kWave + l;
        const int at = (k < 2 * np2) ? ((k >> 1) * kWave + l) * 2 + (k & 1) : np2 * 2 * kWave + l;
        if (s_[at] == -1) {
          const int64_t pad_col = r < n ? r : n - 1;
          if (bits(v_[at]) != 0 || c_[at] != (int)pad_col) {
            fprintf(stderr, "%s: padding slot %d of row %lld holds weight %g, column %d\n", name.c_str(), k, (long long)r, v_[at], c_[at]);
            ok = false;
          }
        } else {
          entry(r, s_[at], c_[at], v_[at], "a slot");
        }
      }
  }
  for (size_t t = 0; t < m.tail_row.size() && ok; ++t)
    for (int64_t k = m.tail_ptr[t]; k < m.tail_ptr[t + 1] && ok; ++k)
      entry(m.tail_row[t], m.tail_src[(size_t)k], m.tail_col[(size_t)k], m.tail_val[(size_t)k], "a tail entry");
  if (!ok) {
    ++g_failures;
    return;
  }
  for (int64_t f = 0; f < n_faces; ++f)
    for (int side = 0; side < 2; ++side) {
      const int64_t row = side ? F.outer[(size_t)f] : F.inner[(size_t)f];
      CHECK(seen[(size_t)(2 * f + side)] == (row < n ? 1 : 0), "face %lld side %d (row %lld of %lld owned) appears %d times", (long long)f, side,
            (long long)row, (long long)n, seen[(size_t)(2 * f + side)]);
    }
  printf("%s threads=%s: %lld rows, %lld faces, %lld slots, %lld tail entries ok\n", name.c_str(), getenv("STORM_HIP_BUILD_THREADS"),
         (long long)n, (long long)n_faces, (long long)m.ell_slots, (long long)m.tail_nnz);
}

}  // namespace

int main(int argc, char **argv) {
  const std::string root = argc > 1 ? argv[1] : ".";
  setenv("STORM_HIP_BUILD_MIN_CHUNK", "5", 1);  // (read once, at the first pack)
  for (const char *threads : {"1", "3", "7"}) {
    setenv("STORM_HIP_BUILD_THREADS", threads, 1);
    Faces a = box(5, 4, 3, 3);
    random_weights(a, 1);
    check_case("a_box_5x4x3", a, 0, true);
    Faces b = box(13, 13, 13, 13);
    shuffle_faces(b, 2);
    random_weights(b, 3);
    check_case("b_box_13_shuffled_flipped", b, 0, true);
    Faces c;
    if (!triangle_faces(root + "/tests/golden/mesh/square_nb.1.ele", c)) {
      fprintf(stderr, "cannot read %s/tests/golden/mesh/square_nb.1.ele\n", root.c_str());
      return 1;
    }
    random_weights(c, 4);
    check_case("c_triangles_square_nb", c, 0, false);
    Faces d = ring_and_hub(200);
    random_weights(d, 5);
    check_case("d_ring_200_and_hub", d, 0, true);
    check_case("d2_box_13_ell_cap_2", b, 2, false);
    Faces e = box(5, 4, 3, 2);
    random_weights(e, 6);
    check_case("e_box_5x4x3_last_plane_halo", e, 0, true);
    Faces f;
    f.n_owned = 3;
    random_weights(f, 7);
    check_case("f_three_cells_no_faces", f, 0, true);
    if (g_failures) return 1;
  }
  {  // 2^30 faces and more are refused before anything is read
    PackOptions o;
    o.updatable = 1;
    OpImage m;
    const int64_t cell = 0;
    const double w = 0.0;
    if (op_pack_from_face_weights(o, 2, 0, (int64_t)1 << 30, &cell, &cell, &w, &w, nullptr, &m) != STORM_HIP_E_INVALID || !strstr(g_err, "2^30")) {
      fprintf(stderr, "2^30 faces were not refused\n");
      return 1;
    }
  }
  printf("srcmap: ok\n");
  return 0;
}
