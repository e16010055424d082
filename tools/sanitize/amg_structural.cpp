// The host half of a refreshable multigrid object (csrc/amg_setup.hip) alone, no GPU: the structural setup
// (storm_hip_amg_setup_csr_structural) and the maps a refresh needs (amg_refresh_maps: the transpose map, the slot -> entry
// maps of the transfer records, the pattern of A P) on a 7-point box and on a random symmetric matrix with stored zeros.
// Every map is checked against the hierarchy it indexes.  One line per case on stdout; tools/sanitize/run.sh runs it under
// the sanitizers.
// Build: g++ -std=c++17 -O1 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude -Istormruler_amd/csrc
//        tools/sanitize/amg_structural.cpp -x c++ stormruler_amd/csrc/amg_setup.hip -lpthread
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#include "amg.hpp"

namespace storm {
static char g_err[512];
void set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
}
}  // namespace storm

namespace {

struct Csr {
  std::vector<int64_t> ptr, col;
  std::vector<double> val;
  int64_t n = 0;
};

Csr box(int e) {
  Csr a;
  a.n = (int64_t)e * e * e;
  a.ptr.push_back(0);
  for (int k = 0; k < e; ++k)
    for (int j = 0; j < e; ++j)
      for (int i = 0; i < e; ++i) {
        const int64_t c = ((int64_t)k * e + j) * e + i;
        if (k > 0) a.col.push_back(c - (int64_t)e * e), a.val.push_back(-1.0);
        if (j > 0) a.col.push_back(c - e), a.val.push_back(-1.0);
        if (i > 0) a.col.push_back(c - 1), a.val.push_back(-1.0);
        a.col.push_back(c), a.val.push_back(6.0);
        if (i < e - 1) a.col.push_back(c + 1), a.val.push_back(-1.0);
        if (j < e - 1) a.col.push_back(c + e), a.val.push_back(-1.0);
        if (k < e - 1) a.col.push_back(c + (int64_t)e * e), a.val.push_back(-1.0);
        a.ptr.push_back((int64_t)a.col.size());
      }
  return a;
}

// symmetric, diagonally dominant, a few random couplings per row; every seventh coupling is a stored zero
Csr random_symmetric(int64_t n, uint64_t seed) {
  std::vector<std::map<int64_t, double>> rows((size_t)n);
  uint64_t s = seed;
  auto next = [&s]() { return s = s * 6364136223846793005ull + 1442695040888963407ull, s >> 33; };
  int64_t count = 0;
  for (int64_t i = 0; i < n; ++i)
    for (int q = 0; q < 3; ++q) {
      const int64_t j = (int64_t)(next() % (uint64_t)n);
      if (j == i) continue;
      const double v = (++count % 7 == 0) ? 0.0 : -1.0 - (double)(next() % 1000) / 1000.0;
      rows[(size_t)i][j] = v, rows[(size_t)j][i] = v;
    }
  Csr a;
  a.n = n;
  a.ptr.push_back(0);
  for (int64_t i = 0; i < n; ++i) {
    double d = 1.0;
    for (const auto &e : rows[(size_t)i]) d += e.second < 0 ? -e.second : e.second;
    rows[(size_t)i][i] = 1.5 * d;
    for (const auto &e : rows[(size_t)i]) a.col.push_back(e.first), a.val.push_back(e.second);
    a.ptr.push_back((int64_t)a.col.size());
  }
  return a;
}

int check_maps(const storm_hip_amg_hierarchy &h, std::string *out) {
  double checksum = 0.0;
  for (size_t l = 0; l + 1 < h.levels.size(); ++l) {
    const storm::AmgHostLevel &L = h.levels[l];
    storm::AmgRefreshMaps m;
    if (storm::amg_refresh_maps(h, l, &m) != 0) return *out = std::string("maps refused: ") + storm::g_err, 1;
    if (L.strong.size() != L.A.col.size()) return *out = "a strong mask of the wrong length", 1;
    for (size_t k = 0; k < m.r_of.size(); ++k)
      if (m.r_of[k] < 0 || m.r_of[k] >= L.P.nnz() || L.P.val[(size_t)m.r_of[k]] != L.R.val[k]) return *out = "the transpose map is wrong", 1;
    // the slot maps against the records amg_pack_transfer writes: a slot's weight is its entry's value, padding has none
    const storm::AmgCsr *T[2] = {&L.P, &L.R};
    const std::vector<int> *slot[2] = {&m.p_slot, &m.r_slot};
    for (int t = 0; t < 2; ++t) {
      storm::AmgTransferImage img;
      if (storm::amg_pack_transfer(*T[t], &img) != 0) return *out = "transfer records refused", 1;
      if ((int64_t)slot[t]->size() != img.slots) return *out = "a slot map of the wrong length", 1;
      int64_t real = 0;
      for (int64_t s = 0; s < img.n_slices; ++s) {
        const int64_t w = (img.off[(size_t)s + 1] - img.off[(size_t)s]) / (storm::kWave * 12);
        const double *vp = reinterpret_cast<const double *>(img.pack.data() + img.off[(size_t)s] + w * storm::kWave * 4);
        for (int64_t q = 0; q < w * storm::kWave; ++q) {
          const int id = (*slot[t])[(size_t)(img.off[(size_t)s] / 12 + q)];
          if (id >= L.P.nnz()) return *out = "a slot map entry outside P", 1;
          if (id < 0 ? vp[q] != 0.0 : vp[q] != L.P.val[(size_t)id]) return *out = "a slot map entry names the wrong weight", 1;
          real += id >= 0;
        }
      }
      if (real != T[t]->nnz()) return *out = "a slot map misses entries", 1;
    }
    if (m.AP.n_rows != L.A.n_rows || m.AP.n_cols != L.P.n_cols) return *out = "A P of the wrong shape", 1;
    checksum += (double)m.AP.nnz() + (double)m.p_slot.size() + (double)m.r_slot.size();
    for (uint8_t b : L.strong) checksum += b;
  }
  char buf[96];
  snprintf(buf, sizeof buf, "%d levels, checksum %.12e", (int)h.levels.size(), checksum);
  *out = buf;
  return 0;
}

int run(const char *name, const Csr &a, const storm_hip_amg_params *p) {
  storm_hip_amg_hierarchy *h = nullptr;
  const int st = storm_hip_amg_setup_csr_structural(a.n, a.ptr.data(), a.col.data(), a.val.data(), p, &h);
  if (st != 0) {
    printf("%s: status %d (%s)\n", name, st, storm::g_err);
    return 1;
  }
  double structural = 0.0;
  storm_hip_amg_hierarchy_get(h, "structural", &structural);
  int64_t n = 0, nnz = 0, n_agg = 0, nnz_p = 0;
  storm_hip_amg_hierarchy_level_sizes(h, 0, &n, &nnz, &n_agg, &nnz_p);
  std::vector<uint8_t> mask((size_t)nnz);
  const int st_mask = storm_hip_amg_hierarchy_get_strong(h, 0, mask.data());
  std::string what;
  int bad = check_maps(*h, &what);
  if (structural != 1.0 || st_mask != 0 || nnz != (int64_t)a.col.size()) bad = 1, what += " (level 0 lost a stored entry, or no mask)";
  printf("%s: %s\n", name, what.c_str());
  storm_hip_amg_hierarchy_destroy(h);
  return bad;
}

}  // namespace

int main() {
  int bad = 0;
  storm_hip_amg_params p;
  storm_hip_amg_params_default(&p);
  p.coarse_rows = 32;
  bad += run("box 13", box(13), &p);
  bad += run("box 21 (threaded rows)", box(21), &p);
  bad += run("random symmetric with stored zeros", random_symmetric(3000, 7), &p);
  p.prolongator_omega = 0.0;
  bad += run("box 13, unsmoothed", box(13), &p);
  printf("%s\n", bad ? "amg_structural: FAILED" : "amg_structural: ok");
  return bad ? 1 : 0;
}
