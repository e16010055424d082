// The host half of the smoothed-aggregation multigrid preconditioner: the hierarchy from assembled CSR.  Host code only: no
// context, no device (tests/test_amg_host.py runs it on a machine without one).  The recipe -- strength, aggregation,
// filtered matrix, prolongator, coarse operator, stopping rule, dense inverse -- is stated in include/storm_hip.h
// ("Smoothed-aggregation multigrid preconditioner") and restated in tests/amg_ref.py; the numbers below are its steps.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <thread>

#include "amg.hpp"
#include "host_threads.hpp"

namespace storm {

// Rows are independent: contiguous chunks of rows, one per thread (fewer threads for few rows).
template <class F>
static void amg_parallel_rows(int64_t n, F &&body) {
  int nt = (int)std::min<int64_t>(host_threads(), std::max<int64_t>(1, n / 4096));
  if (nt <= 1) {
    body((int64_t)0, n);
    return;
  }
  std::vector<std::thread> th;
  for (int t = 0; t < nt; ++t) th.emplace_back([&, t] { body(n * t / nt, n * (t + 1) / nt); });
  for (auto &x : th) x.join();
}

static AmgCsr amg_transpose(const AmgCsr &A) {
  AmgCsr T;
  T.n_rows = A.n_cols, T.n_cols = A.n_rows;
  T.ptr.assign((size_t)T.n_rows + 1, 0);
  for (int c : A.col) ++T.ptr[(size_t)c + 1];
  for (int64_t i = 0; i < T.n_rows; ++i) T.ptr[(size_t)i + 1] += T.ptr[(size_t)i];
  T.col.resize(A.col.size()), T.val.resize(A.val.size());
  std::vector<int64_t> at(T.ptr.begin(), T.ptr.end() - 1);
  for (int64_t i = 0; i < A.n_rows; ++i)  // rows in ascending order: every row of T comes out sorted
    for (int64_t k = A.ptr[(size_t)i]; k < A.ptr[(size_t)i + 1]; ++k) {
      const int64_t p = at[(size_t)A.col[(size_t)k]]++;
      T.col[(size_t)p] = (int)i, T.val[(size_t)p] = A.val[(size_t)k];
    }
  return T;
}

// The caller's CSR as a level operator: columns sorted, duplicates summed in their order, exact zeros dropped (structural:
// kept -- every stored entry stays), the diagonal kept even where it is zero.
static int amg_normalise(int64_t n, const int64_t *row_ptr, const int64_t *col, const double *val, bool structural, AmgCsr *out) {
  STORM_REQUIRE(n >= 1 && n < (int64_t)INT32_MAX, "amg_setup: %lld rows (1 .. 2^31 - 2)", (long long)n);
  STORM_REQUIRE(row_ptr[0] == 0, "amg_setup: row_ptr[0] != 0");
  AmgCsr A;
  A.n_rows = A.n_cols = n;
  A.ptr.assign((size_t)n + 1, 0);
  std::vector<std::pair<int, double>> row;
  for (int64_t i = 0; i < n; ++i) {
    STORM_REQUIRE(row_ptr[i + 1] >= row_ptr[i], "amg_setup: row_ptr not monotone at row %lld", (long long)i);
    row.clear();
    for (int64_t k = row_ptr[i]; k < row_ptr[i + 1]; ++k) {
      STORM_REQUIRE(col[k] >= 0 && col[k] < n, "amg_setup: column %lld of row %lld outside [0, %lld)", (long long)col[k],
                    (long long)i, (long long)n);
      STORM_REQUIRE(std::isfinite(val[k]), "amg_setup: a non-finite entry in row %lld", (long long)i);
      row.emplace_back((int)col[k], val[k]);
    }
    std::stable_sort(row.begin(), row.end(), [](const auto &a, const auto &b) { return a.first < b.first; });
    bool diag = false;
    for (size_t k = 0; k < row.size();) {
      double s = row[k].second;
      size_t e = k + 1;
      for (; e < row.size() && row[e].first == row[k].first; ++e) s += row[e].second;
      if (row[k].first == i) diag = true;
      if (!diag && row[k].first > i) A.col.push_back((int)i), A.val.push_back(0.0), diag = true;
      if (structural || s != 0.0 || row[k].first == i) A.col.push_back(row[k].first), A.val.push_back(s);
      k = e;
    }
    if (!diag) A.col.push_back((int)i), A.val.push_back(0.0);
    A.ptr[(size_t)i + 1] = (int64_t)A.col.size();
  }
  *out = std::move(A);
  return STORM_HIP_OK;
}

// Steps 1 and 2.  The strong graph lives on the union of the patterns of A and its transpose.
struct AmgStrong {
  std::vector<int64_t> ptr;
  std::vector<int> col;
  std::vector<double> weight;
};

static AmgStrong amg_strength(const AmgCsr &A, const AmgCsr &At, double theta) {
  const int64_t n = A.n_rows;
  std::vector<double> m((size_t)n, 0.0);
  for (int64_t i = 0; i < n; ++i)
    for (int64_t k = A.ptr[(size_t)i]; k < A.ptr[(size_t)i + 1]; ++k)
      if (A.col[(size_t)k] != i) m[(size_t)i] = std::max(m[(size_t)i], std::fabs(A.val[(size_t)k]));
  AmgStrong S;
  S.ptr.assign((size_t)n + 1, 0);
  for (int64_t i = 0; i < n; ++i) {
    int64_t a = A.ptr[(size_t)i], b = At.ptr[(size_t)i];
    const int64_t ae = A.ptr[(size_t)i + 1], be = At.ptr[(size_t)i + 1];
    while (a < ae || b < be) {
      const int ja = a < ae ? A.col[(size_t)a] : INT32_MAX, jb = b < be ? At.col[(size_t)b] : INT32_MAX;
      const int j = std::min(ja, jb);
      const double aij = ja == j ? A.val[(size_t)a] : 0.0, aji = jb == j ? At.val[(size_t)b] : 0.0;
      if (ja == j) ++a;
      if (jb == j) ++b;
      if (j == i) continue;
      const bool strong = (aij != 0.0 && std::fabs(aij) >= theta * m[(size_t)i]) ||
                          (aji != 0.0 && std::fabs(aji) >= theta * m[(size_t)j]);
      if (strong) S.col.push_back(j), S.weight.push_back(std::max(std::fabs(aij), std::fabs(aji)));
    }
    S.ptr[(size_t)i + 1] = (int64_t)S.col.size();
  }
  return S;
}

static int64_t amg_aggregate(const AmgStrong &S, int64_t n, std::vector<int> *agg_out) {
  std::vector<int> agg((size_t)n, -1);
  int n_agg = 0;
  for (int64_t i = 0; i < n; ++i) {  // pass 1
    const int64_t k0 = S.ptr[(size_t)i], k1 = S.ptr[(size_t)i + 1];
    if (k0 == k1 || agg[(size_t)i] >= 0) continue;
    bool free_all = true;
    for (int64_t k = k0; k < k1 && free_all; ++k) free_all = agg[(size_t)S.col[(size_t)k]] < 0;
    if (!free_all) continue;
    agg[(size_t)i] = n_agg;
    for (int64_t k = k0; k < k1; ++k) agg[(size_t)S.col[(size_t)k]] = n_agg;
    ++n_agg;
  }
  const std::vector<int> after1 = agg;
  for (int64_t i = 0; i < n; ++i) {  // pass 2
    if (after1[(size_t)i] >= 0) continue;
    int best = -1;
    double wbest = -1.0;
    for (int64_t k = S.ptr[(size_t)i]; k < S.ptr[(size_t)i + 1]; ++k) {
      const int j = S.col[(size_t)k];
      if (after1[(size_t)j] >= 0 && S.weight[(size_t)k] > wbest) best = j, wbest = S.weight[(size_t)k];
    }
    if (best >= 0) agg[(size_t)i] = after1[(size_t)best];
  }
  for (int64_t i = 0; i < n; ++i) {  // pass 3
    if (agg[(size_t)i] >= 0) continue;
    agg[(size_t)i] = n_agg;
    for (int64_t k = S.ptr[(size_t)i]; k < S.ptr[(size_t)i + 1]; ++k)
      if (agg[(size_t)S.col[(size_t)k]] < 0) agg[(size_t)S.col[(size_t)k]] = n_agg;
    ++n_agg;
  }
  *agg_out = std::move(agg);
  return n_agg;
}

// Steps 3 and 4: P = T - (omega / lambda_F) D_F^-1 A^F T, row by row.  structural: an entry that comes out zero stays, so
// that P lives on the pattern of T u A^F T whatever the values.  strong_out: the strong mask, one byte per entry of A.col.
static int amg_prolongator(const AmgCsr &A, const AmgStrong &S, const std::vector<int> &agg, int64_t n_agg, double omega,
                           bool structural, AmgCsr *P_out, std::vector<uint8_t> *strong_out) {
  const int64_t n = A.n_rows;
  // a^F: the row's strong entries and the diagonal plus its weak ones, on A's own pattern (weak slots marked)
  std::vector<double> dF((size_t)n, 0.0);
  std::vector<uint8_t> &keep = *strong_out;
  keep.assign(A.col.size(), 0);
  std::vector<double> ratio((size_t)n, 0.0);
  int64_t bad_row = -1;
  for (int64_t i = 0; i < n; ++i) {
    double d = 0.0, weak = 0.0, sum_abs = 0.0;
    int64_t s = S.ptr[(size_t)i];
    const int64_t se = S.ptr[(size_t)i + 1];
    for (int64_t k = A.ptr[(size_t)i]; k < A.ptr[(size_t)i + 1]; ++k) {
      const int j = A.col[(size_t)k];
      if (j == i) {
        d = A.val[(size_t)k];
        continue;
      }
      while (s < se && S.col[(size_t)s] < j) ++s;
      if (s < se && S.col[(size_t)s] == j) keep[(size_t)k] = 1, sum_abs += std::fabs(A.val[(size_t)k]);
      else weak += A.val[(size_t)k];
    }
    dF[(size_t)i] = d + weak;
    if (dF[(size_t)i] == 0.0 && bad_row < 0) bad_row = i;
    ratio[(size_t)i] = (sum_abs + std::fabs(dF[(size_t)i])) / std::fabs(dF[(size_t)i]);
  }
  if (bad_row >= 0)
    STORM_FAIL(STORM_HIP_E_INVALID, "amg_setup: row %lld of the filtered matrix has a zero diagonal", (long long)bad_row);
  double lambda = 0.0;
  for (int64_t i = 0; i < n; ++i) lambda = std::max(lambda, ratio[(size_t)i]);
  const double c = omega / lambda;
  AmgCsr P;
  P.n_rows = n, P.n_cols = n_agg;
  P.ptr.assign((size_t)n + 1, 0);
  if (omega == 0.0) {
    P.col.resize((size_t)n), P.val.assign((size_t)n, 1.0);
    for (int64_t i = 0; i < n; ++i) P.col[(size_t)i] = agg[(size_t)i], P.ptr[(size_t)i + 1] = i + 1;
    *P_out = std::move(P);
    return STORM_HIP_OK;
  }
  std::vector<std::vector<std::pair<int, double>>> rows((size_t)n);
  amg_parallel_rows(n, [&](int64_t r0, int64_t r1) {
    std::vector<std::pair<int, double>> acc;  // (aggregate, sum of a^F_ij over its columns, in column order)
    for (int64_t i = r0; i < r1; ++i) {
      acc.clear();
      for (int64_t k = A.ptr[(size_t)i]; k < A.ptr[(size_t)i + 1]; ++k) {
        const int j = A.col[(size_t)k];
        double v;
        if (j == i) v = dF[(size_t)i];
        else if (keep[(size_t)k]) v = A.val[(size_t)k];
        else continue;
        const int J = agg[(size_t)j];
        size_t q = 0;
        for (; q < acc.size() && acc[q].first != J; ++q) {}
        if (q == acc.size()) acc.emplace_back(J, v);
        else acc[q].second += v;
      }
      const double f = c / dF[(size_t)i];
      auto &row = rows[(size_t)i];
      for (const auto &a : acc) {
        const double p = (a.first == agg[(size_t)i] ? 1.0 : 0.0) - f * a.second;
        if (structural || p != 0.0) row.emplace_back(a.first, p);
      }
      std::sort(row.begin(), row.end(), [](const auto &a, const auto &b) { return a.first < b.first; });
    }
  });
  for (int64_t i = 0; i < n; ++i) {
    for (const auto &a : rows[(size_t)i]) P.col.push_back(a.first), P.val.push_back(a.second);
    P.ptr[(size_t)i + 1] = (int64_t)P.col.size();
  }
  *P_out = std::move(P);
  return STORM_HIP_OK;
}

// C = X Y by rows (Gustavson): every row accumulates in the order of X's entries; columns sorted; exact zeros dropped;
// with keep_diag the diagonal stays even where it is zero; structural: every entry a product reaches stays.
static AmgCsr amg_spgemm(const AmgCsr &X, const AmgCsr &Y, bool keep_diag, bool structural) {
  const int64_t n = X.n_rows, m = Y.n_cols;
  std::vector<std::vector<std::pair<int, double>>> rows((size_t)n);
  amg_parallel_rows(n, [&](int64_t r0, int64_t r1) {
    std::vector<double> acc((size_t)m, 0.0);
    std::vector<int64_t> mark((size_t)m, -1);
    std::vector<int> cols;
    for (int64_t i = r0; i < r1; ++i) {
      cols.clear();
      for (int64_t k = X.ptr[(size_t)i]; k < X.ptr[(size_t)i + 1]; ++k) {
        const int j = X.col[(size_t)k];
        const double x = X.val[(size_t)k];
        for (int64_t q = Y.ptr[(size_t)j]; q < Y.ptr[(size_t)j + 1]; ++q) {
          const int cidx = Y.col[(size_t)q];
          if (mark[(size_t)cidx] != i) mark[(size_t)cidx] = i, acc[(size_t)cidx] = 0.0, cols.push_back(cidx);
          acc[(size_t)cidx] += x * Y.val[(size_t)q];
        }
      }
      if (keep_diag && i < m && mark[(size_t)i] != i) mark[(size_t)i] = i, acc[(size_t)i] = 0.0, cols.push_back((int)i);
      std::sort(cols.begin(), cols.end());
      auto &row = rows[(size_t)i];
      for (int cidx : cols)
        if (structural || acc[(size_t)cidx] != 0.0 || (keep_diag && cidx == i)) row.emplace_back(cidx, acc[(size_t)cidx]);
    }
  });
  AmgCsr Cm;
  Cm.n_rows = n, Cm.n_cols = m;
  Cm.ptr.assign((size_t)n + 1, 0);
  for (int64_t i = 0; i < n; ++i) {
    for (const auto &a : rows[(size_t)i]) Cm.col.push_back(a.first), Cm.val.push_back(a.second);
    Cm.ptr[(size_t)i + 1] = (int64_t)Cm.col.size();
  }
  return Cm;
}

// Step 7: Gauss-Jordan with partial pivoting on [A | I].  shift is added to every entry of A and a pivot below floor is
// refused (N3 of a null-space hierarchy).  The plain step 7 passes 0 and 0: a zero pivot is refused, and so is one below
// 2^-40 max_i |a_ii| -- what the elimination of a SINGULAR matrix leaves in floating point (a few n eps of the scale: 1e-15 ..
// 7e-15 on the pure-Neumann boxes of tests/test_amg_nullspace_host.py, whose "inverse" then has entries of 1e11 .. 1e13),
// eleven orders of magnitude below the smallest pivot of the definite test operators (0.07).
static int amg_gauss_jordan(const AmgCsr &A, double shift, double floor, std::vector<double> *inv_out) {
  const int64_t n = A.n_rows;
  const bool ns = floor > 0.0;
  double scale = 0.0;
  for (int64_t i = 0; i < n; ++i)
    for (int64_t k = A.ptr[(size_t)i]; k < A.ptr[(size_t)i + 1]; ++k)
      if (A.col[(size_t)k] == i && std::isfinite(A.val[(size_t)k])) scale = std::max(scale, std::fabs(A.val[(size_t)k]));
  const double plain_floor = std::ldexp(scale, -40);
  std::vector<double> a((size_t)(n * n), shift), b((size_t)(n * n), 0.0);
  for (int64_t i = 0; i < n; ++i) {
    b[(size_t)(i * n + i)] = 1.0;
    for (int64_t k = A.ptr[(size_t)i]; k < A.ptr[(size_t)i + 1]; ++k) a[(size_t)(i * n + A.col[(size_t)k])] = ns ? A.val[(size_t)k] + shift : A.val[(size_t)k];
  }
  for (int64_t c = 0; c < n; ++c) {
    int64_t p = c;
    for (int64_t i = c + 1; i < n; ++i)
      if (std::fabs(a[(size_t)(i * n + c)]) > std::fabs(a[(size_t)(p * n + c)])) p = i;
    const double piv = a[(size_t)(p * n + c)];
    if (ns && (!std::isfinite(piv) || std::fabs(piv) < floor))
      STORM_FAIL(STORM_HIP_E_INVALID, "amg_setup: the coarsest level (%lld rows) is singular beyond the constants: pivot %g in "
                                      "column %lld is below 2^-30 of the largest diagonal entry", (long long)n, piv, (long long)c);
    if (piv == 0.0 || !std::isfinite(piv))
      STORM_FAIL(STORM_HIP_E_INVALID, "amg_setup: the coarsest level (%lld rows) is singular: zero pivot in column %lld (a "
                                      "pure-Neumann operator, for instance, has no inverse; storm_hip_amg_setup_csr_nullspace "
                                      "/ storm_hip_amg_create_nullspace take one)", (long long)n, (long long)c);
    if (!ns && std::fabs(piv) < plain_floor)
      STORM_FAIL(STORM_HIP_E_INVALID, "amg_setup: the coarsest level (%lld rows) is singular to working precision: pivot %g in "
                                      "column %lld is below 2^-40 of the largest diagonal entry (a pure-Neumann operator, for "
                                      "instance, has no inverse; storm_hip_amg_setup_csr_nullspace / "
                                      "storm_hip_amg_create_nullspace take one)", (long long)n, piv, (long long)c);
    if (p != c)
      for (int64_t j = 0; j < n; ++j) std::swap(a[(size_t)(p * n + j)], a[(size_t)(c * n + j)]), std::swap(b[(size_t)(p * n + j)], b[(size_t)(c * n + j)]);
    for (int64_t j = 0; j < n; ++j) a[(size_t)(c * n + j)] /= piv, b[(size_t)(c * n + j)] /= piv;
    for (int64_t i = 0; i < n; ++i) {
      if (i == c) continue;
      const double f = a[(size_t)(i * n + c)];
      if (f == 0.0) continue;
      for (int64_t j = 0; j < n; ++j) a[(size_t)(i * n + j)] -= f * a[(size_t)(c * n + j)], b[(size_t)(i * n + j)] -= f * b[(size_t)(c * n + j)];
    }
  }
  for (double v : b)
    if (!std::isfinite(v)) {
      if (ns)
        STORM_FAIL(STORM_HIP_E_INVALID, "amg_setup: the coarsest level (%lld rows) is singular beyond the constants: the "
                                        "inverse of the shifted matrix has a non-finite entry", (long long)n);
      STORM_FAIL(STORM_HIP_E_INVALID, "amg_setup: the coarsest level (%lld rows) is singular: its inverse has a non-finite "
                                      "entry (a pure-Neumann operator, for instance, has no inverse)", (long long)n);
    }
  *inv_out = std::move(b);
  return STORM_HIP_OK;
}

int amg_dense_inverse(const AmgCsr &A, std::vector<double> *inv_out) { return amg_gauss_jordan(A, 0.0, 0.0, inv_out); }

// N3: the coarsest level of a null-space hierarchy.  One row: Ainv = (0).  Otherwise s = max a_ii, G = A + (s / n) 1 1^T,
// Ainv = Pi G^-1 Pi with Pi = I - 1 1^T / n: every column less its mean (rows summed in ascending order), then every row.
int amg_coarse_nullspace(const AmgCsr &A, std::vector<double> *inv_out, double *shift_out) {
  const int64_t n = A.n_rows;
  *shift_out = 0.0;
  if (n == 1) {
    inv_out->assign(1, 0.0);
    return STORM_HIP_OK;
  }
  double s = -HUGE_VAL;
  for (int64_t i = 0; i < n; ++i)
    for (int64_t k = A.ptr[(size_t)i]; k < A.ptr[(size_t)i + 1]; ++k) {
      if (!std::isfinite(A.val[(size_t)k]))
        STORM_FAIL(STORM_HIP_E_INVALID, "amg_setup: the coarsest level (%lld rows) has a non-finite entry", (long long)n);
      if (A.col[(size_t)k] == i) s = std::max(s, A.val[(size_t)k]);
    }
  if (!(s > 0.0))
    STORM_FAIL(STORM_HIP_E_INVALID, "amg_setup: the coarsest level (%lld rows) has no positive diagonal entry (max a_ii = %g)",
               (long long)n, s);
  std::vector<double> g;
  STORM_TRY(amg_gauss_jordan(A, s / (double)n, std::ldexp(s, -30), &g));
  for (int64_t j = 0; j < n; ++j) {
    double sum = 0.0;
    for (int64_t i = 0; i < n; ++i) sum += g[(size_t)(i * n + j)];
    const double mean = sum / (double)n;
    for (int64_t i = 0; i < n; ++i) g[(size_t)(i * n + j)] -= mean;
  }
  for (int64_t i = 0; i < n; ++i) {
    double sum = 0.0;
    for (int64_t j = 0; j < n; ++j) sum += g[(size_t)(i * n + j)];
    const double mean = sum / (double)n;
    for (int64_t j = 0; j < n; ++j) g[(size_t)(i * n + j)] -= mean;
  }
  *shift_out = s;
  *inv_out = std::move(g);
  return STORM_HIP_OK;
}

// N1: the constants are in the kernel of level 0 -- every row sum is zero to 2^-40 of the row's absolute sum.
static int amg_check_row_sums(const AmgCsr &A) {
  for (int64_t i = 0; i < A.n_rows; ++i) {
    double sum = 0.0, sum_abs = 0.0;
    for (int64_t k = A.ptr[(size_t)i]; k < A.ptr[(size_t)i + 1]; ++k) sum += A.val[(size_t)k], sum_abs += std::fabs(A.val[(size_t)k]);
    if (!(std::fabs(sum) <= std::ldexp(sum_abs, -40)))
      STORM_FAIL(STORM_HIP_E_INVALID, "amg_setup: row %lld sums to %g (its absolute sum is %g): the operator does not have the "
                                      "constants in its kernel (a Dirichlet face or beta != 0: use storm_hip_amg_setup_csr / "
                                      "storm_hip_amg_create)", (long long)i, sum, sum_abs);
  }
  return STORM_HIP_OK;
}

// N2: the graph of the non-zero off-diagonal entries of level 0, both directions joined, is connected.
static int amg_check_connected(const AmgCsr &A) {
  const int64_t n = A.n_rows;
  std::vector<int> parent((size_t)n);
  for (int64_t i = 0; i < n; ++i) parent[(size_t)i] = (int)i;
  auto find = [&](int x) {
    while (parent[(size_t)x] != x) x = parent[(size_t)x] = parent[(size_t)parent[(size_t)x]];
    return x;
  };
  int64_t components = n;
  for (int64_t i = 0; i < n; ++i)
    for (int64_t k = A.ptr[(size_t)i]; k < A.ptr[(size_t)i + 1]; ++k) {
      if (A.col[(size_t)k] == i || A.val[(size_t)k] == 0.0) continue;
      const int a = find((int)i), b = find(A.col[(size_t)k]);
      if (a != b) parent[(size_t)std::max(a, b)] = std::min(a, b), --components;
    }
  if (components != 1)
    STORM_FAIL(STORM_HIP_E_INVALID, "amg_setup: the operator's graph has %lld connected components; the null-space setup "
                                    "takes one (every component adds a kernel vector the constants do not span)",
               (long long)components);
  return STORM_HIP_OK;
}

static std::string amg_sizes(const storm_hip_amg_hierarchy &h) {
  std::string s;
  for (const auto &l : h.levels) s += (s.empty() ? "" : " / ") + std::to_string((long long)l.A.n_rows);
  return s;
}

static int amg_check_params(const storm_hip_amg_params *p, const char *who) {
  STORM_REQUIRE(std::isfinite(p->strength_theta) && p->strength_theta >= 0.0 && p->strength_theta <= 1.0,
                "%s: strength_theta %g (0 .. 1)", who, p->strength_theta);
  STORM_REQUIRE(std::isfinite(p->prolongator_omega) && p->prolongator_omega >= 0.0 && p->prolongator_omega < 2.0,
                "%s: prolongator_omega %g (0 .. 2)", who, p->prolongator_omega);
  STORM_REQUIRE(p->smoother_degree >= 1 && p->smoother_degree <= kChebMaxDegree, "%s: smoother_degree %d (1 .. %d)", who,
                p->smoother_degree, kChebMaxDegree);
  STORM_REQUIRE(std::isfinite(p->smoother_ratio) && p->smoother_ratio > 1.0, "%s: smoother_ratio %g (> 1)", who, p->smoother_ratio);
  STORM_REQUIRE(p->max_levels >= 1, "%s: max_levels %d (>= 1)", who, p->max_levels);
  STORM_REQUIRE(p->coarse_rows >= 1 && p->coarse_rows <= kAmgMaxCoarse, "%s: coarse_rows %d (1 .. %d)", who, p->coarse_rows,
                kAmgMaxCoarse);
  STORM_REQUIRE(p->reduced_records == 0 || p->reduced_records == 1, "%s: reduced_records %d (0 or 1)", who, p->reduced_records);
  return STORM_HIP_OK;
}

static int amg_build(storm_hip_amg_hierarchy *h) {
  const storm_hip_amg_params &p = h->params;
  for (;;) {
    AmgHostLevel &L = h->levels.back();
    const int64_t n = L.A.n_rows;
    if (n <= p.coarse_rows) break;
    if ((int)h->levels.size() >= p.max_levels) {
      if (n <= kAmgMaxCoarse) break;
      STORM_FAIL(STORM_HIP_E_UNSUPPORTED, "amg_setup: max_levels = %d reached with %lld rows left, more than a dense coarsest "
                                          "level holds (%d); level sizes %s", p.max_levels, (long long)n, kAmgMaxCoarse,
                 amg_sizes(*h).c_str());
    }
    const AmgCsr At = amg_transpose(L.A);
    const AmgStrong S = amg_strength(L.A, At, p.strength_theta);
    std::vector<int> agg;
    const int64_t n_agg = amg_aggregate(S, n, &agg);
    if (10 * n_agg > 9 * n) {  // the next level would keep more than 90 % of the rows
      if (n <= kAmgMaxCoarse) break;
      STORM_FAIL(STORM_HIP_E_UNSUPPORTED, "amg_setup: coarsening stagnates (%lld aggregates of %lld rows), and %lld rows are more "
                                          "than a dense coarsest level holds (%d); level sizes %s", (long long)n_agg, (long long)n,
                 (long long)n, kAmgMaxCoarse, amg_sizes(*h).c_str());
    }
    L.agg = std::move(agg), L.n_agg = n_agg;
    STORM_TRY(amg_prolongator(L.A, S, L.agg, n_agg, p.prolongator_omega, h->structural, &L.P, &L.strong));
    L.R = amg_transpose(L.P);
    AmgHostLevel next;
    next.A = amg_spgemm(L.R, amg_spgemm(L.A, L.P, false, h->structural), true, h->structural);
    h->levels.push_back(std::move(next));  // (invalidates L)
  }
  if (h->nullspace) return amg_coarse_nullspace(h->levels.back().A, &h->ainv, &h->coarse_shift);  // N3
  return amg_dense_inverse(h->levels.back().A, &h->ainv);
}

int amg_pack_transfer(const AmgCsr &T, AmgTransferImage *img) {
  img->n_rows = T.n_rows, img->n_cols = T.n_cols, img->nnz = T.nnz();
  img->n_slices = (T.n_rows + kWave - 1) / kWave;
  img->off.assign((size_t)img->n_slices + 1, 0);
  img->slots = 0;
  for (int64_t s = 0; s < img->n_slices; ++s) {
    int64_t w = 0;
    for (int64_t i = s * kWave; i < std::min<int64_t>(T.n_rows, (s + 1) * kWave); ++i) w = std::max(w, T.ptr[(size_t)i + 1] - T.ptr[(size_t)i]);
    img->off[(size_t)s + 1] = img->off[(size_t)s] + w * kWave * 12;
    img->slots += w * kWave;
  }
  img->pack.assign((size_t)img->off.back(), 0);  // padding: column 0, weight 0
  for (int64_t s = 0; s < img->n_slices; ++s) {
    const int64_t w = (img->off[(size_t)s + 1] - img->off[(size_t)s]) / (kWave * 12);
    int *cp = reinterpret_cast<int *>(img->pack.data() + img->off[(size_t)s]);
    double *vp = reinterpret_cast<double *>(img->pack.data() + img->off[(size_t)s] + w * kWave * 4);
    for (int64_t i = s * kWave; i < std::min<int64_t>(T.n_rows, (s + 1) * kWave); ++i) {
      const int lane = (int)(i - s * kWave);
      int64_t q = 0;
      for (int64_t k = T.ptr[(size_t)i]; k < T.ptr[(size_t)i + 1]; ++k, ++q) {
        STORM_REQUIRE(T.col[(size_t)k] >= 0 && T.col[(size_t)k] < T.n_cols, "amg: a transfer column outside its level");
        cp[q * kWave + lane] = T.col[(size_t)k], vp[q * kWave + lane] = T.val[(size_t)k];
      }
    }
  }
  return STORM_HIP_OK;
}

static int amg_export_csr(const AmgCsr &M, int64_t *row_ptr, int64_t *col, double *val) {
  for (size_t i = 0; i < M.ptr.size(); ++i) row_ptr[i] = M.ptr[i];
  for (size_t k = 0; k < M.col.size(); ++k) col[k] = M.col[k], val[k] = M.val[k];
  return STORM_HIP_OK;
}

// The host half of storm_hip_amg_create_refreshable: what a refresh needs beside the hierarchy (amg.hpp).  Host code only.
int amg_refresh_maps(const storm_hip_amg_hierarchy &h, size_t l, AmgRefreshMaps *m) {
  STORM_REQUIRE(l + 1 < h.levels.size(), "amg_refresh_maps: level %d has no transfer", (int)l);
  const AmgHostLevel &L = h.levels[l];
  const AmgCsr &A = L.A, &P = L.P, &R = L.R;
  STORM_REQUIRE(L.strong.size() == A.col.size() && (int64_t)L.agg.size() == A.n_rows, "amg_refresh_maps: level %d is incomplete", (int)l);
  STORM_REQUIRE(A.nnz() < (int64_t)INT32_MAX && P.nnz() < (int64_t)INT32_MAX, "amg_refresh_maps: more than 2^31 - 2 entries on level %d", (int)l);
  // R_l = P_l^T: entry k of R (coarse row I, fine row i) is entry r_of[k] of P -- the walk of amg_transpose
  m->r_of.assign(R.col.size(), 0);
  std::vector<int64_t> at(R.ptr.begin(), R.ptr.end() - 1);
  for (int64_t i = 0; i < P.n_rows; ++i)
    for (int64_t k = P.ptr[(size_t)i]; k < P.ptr[(size_t)i + 1]; ++k) m->r_of[(size_t)at[(size_t)P.col[(size_t)k]]++] = (int)k;
  for (int64_t I = 0; I < R.n_rows; ++I)
    for (int64_t k = R.ptr[(size_t)I]; k < R.ptr[(size_t)I + 1]; ++k)
      STORM_REQUIRE(P.col[(size_t)m->r_of[(size_t)k]] == I && R.col[(size_t)k] >= 0 && R.col[(size_t)k] < P.n_rows,
                    "amg_refresh_maps: R_%d is not the transpose of P_%d", (int)l, (int)l);
  // the slot -> entry maps of the transfer records (amg_pack_transfer's slot k x 64 + lane behind the slices before)
  const AmgCsr *T[2] = {&P, &R};
  std::vector<int> *slot[2] = {&m->p_slot, &m->r_slot};
  for (int t = 0; t < 2; ++t) {
    const AmgCsr &M = *T[t];
    const int64_t ns = (M.n_rows + kWave - 1) / kWave;
    int64_t total = 0;
    std::vector<int64_t> first((size_t)ns + 1, 0);
    for (int64_t s = 0; s < ns; ++s) {
      int64_t w = 0;
      for (int64_t i = s * kWave; i < std::min<int64_t>(M.n_rows, (s + 1) * kWave); ++i) w = std::max(w, M.ptr[(size_t)i + 1] - M.ptr[(size_t)i]);
      total += w * kWave, first[(size_t)s + 1] = total;
    }
    slot[t]->assign((size_t)total, -1);
    for (int64_t i = 0; i < M.n_rows; ++i) {
      const int64_t s = i / kWave, lane = i % kWave;
      for (int64_t k = M.ptr[(size_t)i], q = 0; k < M.ptr[(size_t)i + 1]; ++k, ++q)
        (*slot[t])[(size_t)(first[(size_t)s] + q * kWave + lane)] = t == 0 ? (int)k : m->r_of[(size_t)k];
    }
  }
  // A_l P_l on its structural pattern (values are the device's to fill)
  m->AP = amg_spgemm(A, P, false, true);
  STORM_REQUIRE(m->AP.nnz() < (int64_t)INT32_MAX, "amg_refresh_maps: more than 2^31 - 2 entries in A_%d P_%d", (int)l, (int)l);
  // every contribution of R (A P) must find its column in the frozen A_{l+1}
  const AmgCsr &N = h.levels[l + 1].A;
  for (int64_t I = 0; I < R.n_rows; ++I)
    for (int64_t k = R.ptr[(size_t)I]; k < R.ptr[(size_t)I + 1]; ++k) {
      const int64_t i = R.col[(size_t)k];
      for (int64_t q = m->AP.ptr[(size_t)i]; q < m->AP.ptr[(size_t)i + 1]; ++q)
        STORM_REQUIRE(std::binary_search(N.col.begin() + N.ptr[(size_t)I], N.col.begin() + N.ptr[(size_t)I + 1], m->AP.col[(size_t)q]),
                      "amg_refresh_maps: A_%d is not on the structural pattern of R (A P)", (int)l + 1);
    }
  return STORM_HIP_OK;
}

}  // namespace storm

using namespace storm;

extern "C" {

void storm_hip_amg_params_default(storm_hip_amg_params *p) {
  if (!p) return;
  p->strength_theta = 0.25, p->prolongator_omega = 4.0 / 3.0, p->smoother_degree = 2, p->smoother_ratio = 30.0;
  p->max_levels = 10, p->coarse_rows = 512, p->reduced_records = 0;
}

static int amg_setup(int64_t n_rows, const int64_t *row_ptr, const int64_t *col, const double *val,
                     const storm_hip_amg_params *params, bool structural, bool nullspace, storm_hip_amg_hierarchy **out) {
  STORM_REQUIRE(row_ptr && out && (n_rows < 1 || row_ptr[n_rows] == 0 || (col && val)), "amg_setup: null argument");
  *out = nullptr;
  storm_hip_amg_params p;
  storm_hip_amg_params_default(&p);
  if (params) p = *params;
  STORM_TRY(amg_check_params(&p, "amg_setup"));
  const auto t0 = std::chrono::steady_clock::now();
  auto *h = new storm_hip_amg_hierarchy();
  h->params = p, h->structural = structural, h->nullspace = nullspace;
  h->levels.emplace_back();
  int st = amg_normalise(n_rows, row_ptr, col, val, structural, &h->levels[0].A);
  if (st == STORM_HIP_OK && nullspace) st = amg_check_row_sums(h->levels[0].A);
  if (st == STORM_HIP_OK && nullspace) st = amg_check_connected(h->levels[0].A);
  if (st == STORM_HIP_OK) st = amg_build(h);
  if (st != STORM_HIP_OK) {
    delete h;
    return st;
  }
  h->setup_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  *out = h;
  return STORM_HIP_OK;
}

int storm_hip_amg_setup_csr(int64_t n_rows, const int64_t *row_ptr, const int64_t *col, const double *val,
                            const storm_hip_amg_params *params, storm_hip_amg_hierarchy **out) {
  return amg_setup(n_rows, row_ptr, col, val, params, false, false, out);
}

int storm_hip_amg_setup_csr_structural(int64_t n_rows, const int64_t *row_ptr, const int64_t *col, const double *val,
                                       const storm_hip_amg_params *params, storm_hip_amg_hierarchy **out) {
  return amg_setup(n_rows, row_ptr, col, val, params, true, false, out);
}

int storm_hip_amg_setup_csr_nullspace(int64_t n_rows, const int64_t *row_ptr, const int64_t *col, const double *val,
                                      const storm_hip_amg_params *params, int structural, storm_hip_amg_hierarchy **out) {
  return amg_setup(n_rows, row_ptr, col, val, params, structural != 0, true, out);
}

int storm_hip_amg_hierarchy_get_strong(const storm_hip_amg_hierarchy *h, int level, uint8_t *mask) {
  STORM_REQUIRE(h && mask, "amg_hierarchy_get_strong: null argument");
  STORM_REQUIRE(level >= 0 && level + 1 < (int)h->levels.size(), "amg_hierarchy_get_strong: level %d has no strong mask (%d levels)",
                level, (int)h->levels.size());
  const auto &m = h->levels[(size_t)level].strong;
  if (!m.empty()) std::memcpy(mask, m.data(), m.size());
  return STORM_HIP_OK;
}

int storm_hip_amg_hierarchy_destroy(storm_hip_amg_hierarchy *h) {
  delete h;
  return STORM_HIP_OK;
}

int storm_hip_amg_hierarchy_levels(const storm_hip_amg_hierarchy *h, int *levels) {
  STORM_REQUIRE(h && levels, "amg_hierarchy_levels: null argument");
  *levels = (int)h->levels.size();
  return STORM_HIP_OK;
}

int storm_hip_amg_hierarchy_level_sizes(const storm_hip_amg_hierarchy *h, int level, int64_t *n_rows, int64_t *nnz_a,
                                        int64_t *n_aggregates, int64_t *nnz_p) {
  STORM_REQUIRE(h && n_rows && nnz_a && n_aggregates && nnz_p, "amg_hierarchy_level_sizes: null argument");
  STORM_REQUIRE(level >= 0 && level < (int)h->levels.size(), "amg_hierarchy_level_sizes: level %d of %d", level, (int)h->levels.size());
  const AmgHostLevel &L = h->levels[(size_t)level];
  *n_rows = L.A.n_rows, *nnz_a = L.A.nnz(), *n_aggregates = L.n_agg, *nnz_p = L.P.nnz();
  return STORM_HIP_OK;
}

int storm_hip_amg_hierarchy_get_operator(const storm_hip_amg_hierarchy *h, int level, int64_t *row_ptr, int64_t *col, double *val) {
  STORM_REQUIRE(h && row_ptr && col && val, "amg_hierarchy_get_operator: null argument");
  STORM_REQUIRE(level >= 0 && level < (int)h->levels.size(), "amg_hierarchy_get_operator: level %d of %d", level, (int)h->levels.size());
  return amg_export_csr(h->levels[(size_t)level].A, row_ptr, col, val);
}

int storm_hip_amg_hierarchy_get_aggregates(const storm_hip_amg_hierarchy *h, int level, int64_t *aggregate) {
  STORM_REQUIRE(h && aggregate, "amg_hierarchy_get_aggregates: null argument");
  STORM_REQUIRE(level >= 0 && level + 1 < (int)h->levels.size(), "amg_hierarchy_get_aggregates: level %d has no aggregates (%d levels)",
                level, (int)h->levels.size());
  const auto &a = h->levels[(size_t)level].agg;
  for (size_t i = 0; i < a.size(); ++i) aggregate[i] = a[i];
  return STORM_HIP_OK;
}

int storm_hip_amg_hierarchy_get_prolongator(const storm_hip_amg_hierarchy *h, int level, int64_t *row_ptr, int64_t *col, double *val) {
  STORM_REQUIRE(h && row_ptr && col && val, "amg_hierarchy_get_prolongator: null argument");
  STORM_REQUIRE(level >= 0 && level + 1 < (int)h->levels.size(), "amg_hierarchy_get_prolongator: level %d has no prolongator (%d levels)",
                level, (int)h->levels.size());
  return amg_export_csr(h->levels[(size_t)level].P, row_ptr, col, val);
}

int storm_hip_amg_hierarchy_get_coarse_inverse(const storm_hip_amg_hierarchy *h, double *inverse) {
  STORM_REQUIRE(h && inverse, "amg_hierarchy_get_coarse_inverse: null argument");
  std::memcpy(inverse, h->ainv.data(), sizeof(double) * h->ainv.size());
  return STORM_HIP_OK;
}

int storm_hip_amg_hierarchy_get(const storm_hip_amg_hierarchy *h, const char *key, double *value) {
  STORM_REQUIRE(h && key && value, "amg_hierarchy_get: null argument");
  double nnz = 0.0, rows = 0.0;
  for (const auto &l : h->levels) nnz += (double)l.A.nnz(), rows += (double)l.A.n_rows;
  if (!strcmp(key, "levels")) *value = (double)h->levels.size();
  else if (!strcmp(key, "operator_complexity")) *value = nnz / (double)h->levels[0].A.nnz();
  else if (!strcmp(key, "grid_complexity")) *value = rows / (double)h->levels[0].A.n_rows;
  else if (!strcmp(key, "setup_seconds")) *value = h->setup_seconds;
  else if (!strcmp(key, "structural")) *value = h->structural ? 1.0 : 0.0;
  else if (!strcmp(key, "nullspace")) *value = h->nullspace ? 1.0 : 0.0;
  else if (!strcmp(key, "coarse_shift")) *value = h->coarse_shift;
  else STORM_FAIL(STORM_HIP_E_INVALID, "amg_hierarchy_get: unknown key '%s'", key);
  return STORM_HIP_OK;
}

}  // extern "C"
