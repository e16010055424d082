// The host setup of the multigrid preconditioner (csrc/amg_setup.hip) alone, no GPU: hierarchies of a 7-point box (large
// enough for the threaded row loops), of a scrambled copy with every entry split in two, and the refusals.  One line per
// case on stdout; tools/sanitize/run.sh runs it under the sanitizers.
// Build: g++ -std=c++17 -O1 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude -Istormruler_amd/csrc
//        tools/sanitize/amg_setup.cpp -x c++ stormruler_amd/csrc/amg_setup.hip -lpthread
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
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

Csr box(int e, bool split) {
  Csr a;
  a.n = (int64_t)e * e * e;
  a.ptr.push_back(0);
  for (int k = 0; k < e; ++k)
    for (int j = 0; j < e; ++j)
      for (int i = 0; i < e; ++i) {
        const int64_t c = ((int64_t)k * e + j) * e + i;
        std::vector<std::pair<int64_t, double>> row = {{c, 6.0}};
        if (i > 0) row.push_back({c - 1, -1.0});
        if (i < e - 1) row.push_back({c + 1, -1.0});
        if (j > 0) row.push_back({c - e, -1.0});
        if (j < e - 1) row.push_back({c + e, -1.0});
        if (k > 0) row.push_back({c - (int64_t)e * e, -1.0});
        if (k < e - 1) row.push_back({c + (int64_t)e * e, -1.0});
        if (split) {  // descending columns, every entry as two halves
          for (size_t q = row.size(); q-- > 0;) a.col.push_back(row[q].first), a.val.push_back(0.5 * row[q].second);
          for (size_t q = row.size(); q-- > 0;) a.col.push_back(row[q].first), a.val.push_back(0.5 * row[q].second);
        } else {
          for (const auto &p : row) a.col.push_back(p.first), a.val.push_back(p.second);
        }
        a.ptr.push_back((int64_t)a.col.size());
      }
  return a;
}

std::string describe(const storm_hip_amg_hierarchy *h) {
  int levels = 0;
  storm_hip_amg_hierarchy_levels(h, &levels);
  std::string s;
  double checksum = 0.0;
  for (int l = 0; l < levels; ++l) {
    int64_t n = 0, nnz = 0, n_agg = 0, nnz_p = 0;
    storm_hip_amg_hierarchy_level_sizes(h, l, &n, &nnz, &n_agg, &nnz_p);
    std::vector<int64_t> ptr((size_t)n + 1), col((size_t)nnz);
    std::vector<double> val((size_t)nnz);
    storm_hip_amg_hierarchy_get_operator(h, l, ptr.data(), col.data(), val.data());
    for (double v : val) checksum += v;
    if (l + 1 < levels) {
      std::vector<int64_t> agg((size_t)n), pp((size_t)n + 1), pc((size_t)nnz_p);
      std::vector<double> pv((size_t)nnz_p);
      storm_hip_amg_hierarchy_get_aggregates(h, l, agg.data());
      storm_hip_amg_hierarchy_get_prolongator(h, l, pp.data(), pc.data(), pv.data());
      for (double v : pv) checksum += v;
      storm::AmgCsr P;  // ... and its transfer records
      P.n_rows = n, P.n_cols = n_agg, P.ptr = pp, P.col.assign(pc.begin(), pc.end()), P.val = pv;
      storm::AmgTransferImage img;
      if (storm::amg_pack_transfer(P, &img) != 0) return "transfer records refused";
      checksum += (double)img.slots;
    }
    s += (l ? " / " : "") + std::to_string((long long)n);
  }
  int64_t n = 0, nnz = 0, a = 0, b = 0;
  storm_hip_amg_hierarchy_level_sizes(h, levels - 1, &n, &nnz, &a, &b);
  std::vector<double> inv((size_t)(n * n));
  storm_hip_amg_hierarchy_get_coarse_inverse(h, inv.data());
  for (double v : inv) checksum += v;
  char buf[64];
  snprintf(buf, sizeof buf, "  checksum %.12e", checksum);
  return s + buf;
}

int run(const char *name, const Csr &a, const storm_hip_amg_params *p, int expect) {
  storm_hip_amg_hierarchy *h = nullptr;
  const int st = storm_hip_amg_setup_csr(a.n, a.ptr.data(), a.col.data(), a.val.data(), p, &h);
  if (st != expect) {
    printf("%s: status %d, expected %d (%s)\n", name, st, expect, storm::g_err);
    return 1;
  }
  if (st == 0) printf("%s: %s\n", name, describe(h).c_str());
  else printf("%s: refused (%d): %s\n", name, st, storm::g_err);
  storm_hip_amg_hierarchy_destroy(h);
  return 0;
}

}  // namespace

int main() {
  int bad = 0;
  storm_hip_amg_params p;
  storm_hip_amg_params_default(&p);
  p.coarse_rows = 32;
  bad += run("box 13", box(13, false), &p, 0);
  bad += run("box 21 (threaded rows)", box(21, false), &p, 0);
  bad += run("box 21, scrambled and split", box(21, true), &p, 0);
  p.prolongator_omega = 0.0;
  bad += run("box 13, unsmoothed", box(13, false), &p, 0);
  storm_hip_amg_params_default(&p);
  bad += run("box 5, one level", box(5, false), &p, 0);
  p.max_levels = 2, p.coarse_rows = 32;
  bad += run("box 21, max_levels 2", box(21, false), &p, STORM_HIP_E_UNSUPPORTED);
  Csr neumann;
  neumann.n = 2, neumann.ptr = {0, 2, 4}, neumann.col = {0, 1, 0, 1}, neumann.val = {1.0, -1.0, -1.0, 1.0};
  bad += run("pure Neumann", neumann, nullptr, STORM_HIP_E_INVALID);
  Csr diag;
  diag.n = 2000;
  for (int64_t i = 0; i <= diag.n; ++i) diag.ptr.push_back(i);
  for (int64_t i = 0; i < diag.n; ++i) diag.col.push_back(i), diag.val.push_back(1.0 + (double)i);
  bad += run("diagonal (stagnation)", diag, nullptr, STORM_HIP_E_UNSUPPORTED);
  Csr out_of_range = neumann;
  out_of_range.col[1] = 7;
  bad += run("column out of range", out_of_range, nullptr, STORM_HIP_E_INVALID);
  printf("%s\n", bad ? "amg_setup: FAILED" : "amg_setup: ok");
  return bad ? 1 : 0;
}
