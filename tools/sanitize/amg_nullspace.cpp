// The null-space host setup of the multigrid preconditioner (storm_hip_amg_setup_csr_nullspace, csrc/amg_setup.hip) alone,
// no GPU: N1 (row sums), N2 (connectivity) and N3 (the coarsest level's pseudo-inverse) on a chain, a Neumann box (plain and
// structural), a two-component operator, a Dirichlet box, and a one-row coarsest level.  One line per case on stdout;
// tools/sanitize/run.sh runs it under the sanitizers.
// Build: g++ -std=c++17 -O1 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude -Istormruler_amd/csrc
//        tools/sanitize/amg_nullspace.cpp -x c++ stormruler_amd/csrc/amg_setup.hip -lpthread
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
  std::vector<int64_t> ptr{0}, col;
  std::vector<double> val;
  int64_t n = 0;
};

// the graph Laplacian of an nx x ny x nz box behind `first` rows that are already there; wall > 0: Dirichlet walls
void add_box(Csr *a, int nx, int ny, int nz, double wall) {
  const int64_t first = a->n;
  const int dims[3] = {nx, ny, nz};
  for (int k = 0; k < nz; ++k)
    for (int j = 0; j < ny; ++j)
      for (int i = 0; i < nx; ++i) {
        const int idx[3] = {i, j, k};
        const int64_t stride[3] = {1, nx, (int64_t)nx * ny};
        const int64_t c = first + ((int64_t)k * ny + j) * nx + i;
        double diag = 0.0;
        std::vector<std::pair<int64_t, double>> row;
        for (int ax = 0; ax < 3; ++ax) {
          const double w = 1.0 + 0.25 * ax;
          if (idx[ax] > 0) row.push_back({c - stride[ax], -w}), diag += w;
          else diag += wall;
          if (idx[ax] < dims[ax] - 1) row.push_back({c + stride[ax], -w}), diag += w;
          else diag += wall;
        }
        row.push_back({c, diag});
        for (const auto &p : row) a->col.push_back(p.first), a->val.push_back(p.second);
        a->ptr.push_back((int64_t)a->col.size());
      }
  a->n += (int64_t)nx * ny * nz;
}

// |A Ainv A - A|, the largest column / row sum of Ainv, and the largest |Ainv|, of the coarsest level
bool coarse_checks(const storm_hip_amg_hierarchy *h, std::string *out) {
  int levels = 0;
  storm_hip_amg_hierarchy_levels(h, &levels);
  std::string sizes;
  int64_t n = 0, nnz = 0, a = 0, b = 0;
  for (int l = 0; l < levels; ++l) {
    storm_hip_amg_hierarchy_level_sizes(h, l, &n, &nnz, &a, &b);
    sizes += (l ? " / " : "") + std::to_string((long long)n);
    if (l + 1 < levels) {  // the exports of a level with a transfer
      std::vector<int64_t> agg((size_t)n), pp((size_t)n + 1), pc((size_t)b);
      std::vector<double> pv((size_t)b);
      std::vector<uint8_t> mask((size_t)nnz);
      storm_hip_amg_hierarchy_get_aggregates(h, l, agg.data());
      storm_hip_amg_hierarchy_get_prolongator(h, l, pp.data(), pc.data(), pv.data());
      storm_hip_amg_hierarchy_get_strong(h, l, mask.data());
    }
  }
  std::vector<int64_t> ptr((size_t)n + 1), col((size_t)nnz);
  std::vector<double> val((size_t)nnz), inv((size_t)(n * n)), dense((size_t)(n * n), 0.0), t((size_t)(n * n), 0.0);
  storm_hip_amg_hierarchy_get_operator(h, levels - 1, ptr.data(), col.data(), val.data());
  storm_hip_amg_hierarchy_get_coarse_inverse(h, inv.data());
  for (int64_t i = 0; i < n; ++i)
    for (int64_t k = ptr[(size_t)i]; k < ptr[(size_t)i + 1]; ++k) dense[(size_t)(i * n + col[(size_t)k])] = val[(size_t)k];
  double scale = 0.0, big = 0.0, sums = 0.0, res = 0.0;
  for (int64_t i = 0; i < n; ++i)  // t = A Ainv
    for (int64_t j = 0; j < n; ++j) {
      double s = 0.0;
      for (int64_t k = 0; k < n; ++k) s += dense[(size_t)(i * n + k)] * inv[(size_t)(k * n + j)];
      t[(size_t)(i * n + j)] = s;
    }
  for (int64_t i = 0; i < n; ++i) {
    double row = 0.0, column = 0.0;
    for (int64_t j = 0; j < n; ++j) {
      double s = 0.0;
      for (int64_t k = 0; k < n; ++k) s += t[(size_t)(i * n + k)] * dense[(size_t)(k * n + j)];
      res = std::fmax(res, std::fabs(s - dense[(size_t)(i * n + j)]));
      scale = std::fmax(scale, std::fabs(dense[(size_t)(i * n + j)]));
      big = std::fmax(big, std::fabs(inv[(size_t)(i * n + j)]));
      row += inv[(size_t)(i * n + j)], column += inv[(size_t)(j * n + i)];
    }
    sums = std::fmax(sums, std::fmax(std::fabs(row), std::fabs(column)));
  }
  double ns = 0.0, shift = 0.0;
  storm_hip_amg_hierarchy_get(h, "nullspace", &ns);
  storm_hip_amg_hierarchy_get(h, "coarse_shift", &shift);
  char buf[256];
  snprintf(buf, sizeof buf, "%s  shift %.6e  |A Ainv A - A| %.2e  sums of Ainv %.2e  max|Ainv| %.3e", sizes.c_str(), shift, res, sums, big);
  *out = buf;
  const double eps = 2.220446049250313e-16;
  if (ns != 1.0) return false;
  if (n == 1) return inv[0] == 0.0 && shift == 0.0;
  return shift > 0.0 && res <= 1024.0 * (double)n * eps * scale && sums <= 64.0 * eps * big;
}

int run(const char *name, const Csr &a, const storm_hip_amg_params *p, int structural, int expect, const char *needle) {
  storm_hip_amg_hierarchy *h = nullptr;
  const int st = storm_hip_amg_setup_csr_nullspace(a.n, a.ptr.data(), a.col.data(), a.val.data(), p, structural, &h);
  int bad = 0;
  if (st != expect) {
    printf("%s: status %d, expected %d (%s)\n", name, st, expect, storm::g_err);
    bad = 1;
  } else if (st == 0) {
    std::string line;
    if (!coarse_checks(h, &line)) bad = 1;
    printf("%s: %s%s\n", name, line.c_str(), bad ? "  <-- FAILED" : "");
  } else {
    if (needle && !strstr(storm::g_err, needle)) bad = 1;
    printf("%s: refused (%d): %s%s\n", name, st, storm::g_err, bad ? "  <-- the message lacks its key word" : "");
  }
  storm_hip_amg_hierarchy_destroy(h);
  return bad;
}

}  // namespace

int main() {
  int bad = 0;
  storm_hip_amg_params p;
  storm_hip_amg_params_default(&p);
  p.coarse_rows = 16;
  Csr chain;
  add_box(&chain, 40, 1, 1, 0.0);
  bad += run("chain of 40", chain, &p, 0, 0, nullptr);
  p.coarse_rows = 1, p.prolongator_omega = 0.0;
  bad += run("chain of 40, unsmoothed, down to one row", chain, &p, 0, 0, nullptr);
  storm_hip_amg_params_default(&p);
  p.coarse_rows = 16;
  Csr box;
  add_box(&box, 12, 10, 9, 0.0);
  bad += run("Neumann box 12 x 10 x 9", box, &p, 0, 0, nullptr);
  bad += run("Neumann box 12 x 10 x 9, structural", box, &p, 1, 0, nullptr);
  Csr big;
  add_box(&big, 24, 21, 20, 0.0);
  bad += run("Neumann box 24 x 21 x 20 (threaded rows)", big, &p, 1, 0, nullptr);
  storm_hip_amg_params_default(&p);
  bad += run("Neumann box, default parameters (a coarsest level of 140 rows)", box, &p, 0, 0, nullptr);
  Csr one;
  add_box(&one, 1, 1, 1, 0.0);
  bad += run("one cell", one, nullptr, 0, 0, nullptr);
  Csr two = box;
  add_box(&two, 4, 4, 4, 0.0);
  bad += run("two boxes (N2)", two, &p, 0, STORM_HIP_E_INVALID, "2 connected components");
  bad += run("two boxes, structural (N2)", two, &p, 1, STORM_HIP_E_INVALID, "component");
  Csr walls;
  add_box(&walls, 6, 6, 6, 2.0);
  bad += run("Dirichlet box (N1)", walls, &p, 0, STORM_HIP_E_INVALID, "row 0 ");
  Csr isolated = chain;
  isolated.col.push_back(isolated.n), isolated.val.push_back(0.0), isolated.ptr.push_back((int64_t)isolated.col.size()), ++isolated.n;
  bad += run("chain and an isolated zero row (N2)", isolated, &p, 1, STORM_HIP_E_INVALID, "2 connected components");
  Csr negative = chain;
  for (double &v : negative.val) v = -v;
  p.coarse_rows = 64;
  bad += run("negated chain (N3: no positive diagonal)", negative, &p, 0, STORM_HIP_E_INVALID, "positive diagonal");
  p.smoother_degree = 17;
  bad += run("smoother_degree 17", chain, &p, 0, STORM_HIP_E_INVALID, "smoother_degree");
  printf("%s\n", bad ? "amg_nullspace: FAILED" : "amg_nullspace: ok");
  return bad ? 1 : 0;
}
