// The host-only half of the operator build (host code only; no device is touched): which of the five record formats an
// operator takes, and every byte the apply kernels read -- records, dictionaries, slice lists, the CSR tail, the latency
// path's compact copy -- as an OpImage.  spmv_build.hip uploads the image.  Record layouts: the header of spmv.hip;
// their sizes: op_layout.hpp.
//
// Threaded over rows / entries (STORM_HIP_BUILD_THREADS); what a thread count could change -- dictionaries in order of
// first occurrence, the order inside a row -- is merged in chunk order, so the image does not depend on it.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <thread>

#include "common.hpp"
#include "host_threads.hpp"
#include "op_layout.hpp"

namespace storm {
namespace {

int64_t forced_min_chunk() {  // STORM_HIP_BUILD_MIN_CHUNK (tests: thread small inputs too); 0: each pass's own
  static const int64_t forced = getenv("STORM_HIP_BUILD_MIN_CHUNK") ? atoll(getenv("STORM_HIP_BUILD_MIN_CHUNK")) : 0;
  return forced;
}
// fn(t, begin, end) over [0, n) in contiguous chunks, chunk t on thread t (in index order: results that depend on
// "first occurrence" are merged in chunk order and come out as a serial pass would leave them).
template <class F>
int parallel_chunks(int64_t n, int64_t min_chunk, F &&fn) {
  if (forced_min_chunk() > 0) min_chunk = forced_min_chunk();
  const int T = (int)std::max<int64_t>(1, std::min<int64_t>(host_threads(), n / std::max<int64_t>(1, min_chunk)));
  const int64_t per = (n + T - 1) / T;
  if (T == 1) {
    fn(0, (int64_t)0, n);
    return 1;
  }
  std::vector<std::thread> th;
  for (int t = 1; t < T; ++t) th.emplace_back([&, t] { fn(t, std::min(n, t * per), std::min(n, (t + 1) * per)); });
  fn(0, (int64_t)0, std::min(n, per));
  for (auto &x : th) x.join();
  return T;
}

// The distinct fp64 bit patterns of an operator, while there are at most 256 of them.
struct ValueDict {
  std::vector<uint64_t> values;               // index -> bit pattern
  std::vector<std::pair<uint64_t, int>> tab;  // open-addressing hash, 1024 buckets
  uint64_t last_bits = ~0ull;
  int last_idx = -1;
  ValueDict() : tab(1024, {0, -1}) {}
  static uint64_t bits(double v) {
    uint64_t b;
    memcpy(&b, &v, 8);
    return b;
  }
  int find(uint64_t b, bool insert) {
    if (last_idx >= 0 && b == last_bits) return last_idx;  // (an empty cache matches nothing: offset -1 is all ones too)
    size_t h = (size_t)((b * 0x9E3779B97F4A7C15ull) >> 54);
    for (;; h = (h + 1) & 1023) {
      if (tab[h].second < 0) {
        if (!insert || values.size() >= (size_t)kDictSize) return -1;
        tab[h] = {b, (int)values.size()};
        values.push_back(b);
      }
      if (tab[h].first == b && tab[h].second >= 0) {
        last_bits = b, last_idx = tab[h].second;
        return last_idx;
      }
    }
  }
  bool add(double v) { return find(bits(v), true) >= 0; }
  int index(double v) { return find(bits(v), false); }
  // the same look-up without the one-entry cache: safe from several threads once the dictionary is complete
  int lookup(uint64_t b) const {
    size_t h = (size_t)((b * 0x9E3779B97F4A7C15ull) >> 54);
    for (;; h = (h + 1) & 1023) {
      if (tab[h].second < 0) return -1;
      if (tab[h].first == b) return tab[h].second;
    }
  }
  int lookup(double v) const { return lookup(bits(v)); }
  // Distinct values of keys(i), i in [0, n), in order of first occurrence (what a serial pass of add() would give),
  // gathered by the build threads; false when there are more than the dictionary holds.
  template <class K>
  bool add_all(int64_t n, K &&key) {
    std::vector<ValueDict> part((size_t)host_threads());
    std::vector<char> ok(part.size(), 1);
    const int T = parallel_chunks(n, 1 << 16, [&](int t, int64_t b, int64_t e) {
      ValueDict &d = part[(size_t)t];
      for (int64_t i = b; i < e; ++i)
        if (d.find(key(i), true) < 0) {
          ok[(size_t)t] = 0;
          return;
        }
    });
    for (int t = 0; t < T; ++t) {
      if (!ok[(size_t)t]) return false;
      for (uint64_t v : part[(size_t)t].values)
        if (find(v, true) < 0) return false;
    }
    return true;
  }
};

// Shortest common supersequence of two short offset lists (format 3: the merged neighbour list of a row pair).
// Returns its length (<= na + nb), the sequence in out[], and where each input element landed in pa[] / pb[].
int merge_offsets(const int64_t *a, int na, const int64_t *b, int nb, int64_t *out, int *pa, int *pb) {
  int L[9][9];  // LCS of the suffixes a[i..], b[j..]
  for (int i = na; i >= 0; --i)
    for (int j = nb; j >= 0; --j)
      L[i][j] = (i == na || j == nb) ? 0 : (a[i] == b[j] ? 1 + L[i + 1][j + 1] : std::max(L[i + 1][j], L[i][j + 1]));
  int i = 0, j = 0, m = 0;
  while (i < na || j < nb) {
    if (i < na && j < nb && a[i] == b[j]) pa[i] = pb[j] = m, out[m++] = a[i], ++i, ++j;
    else if (j == nb || (i < na && L[i + 1][j] >= L[i][j + 1])) pa[i] = m, out[m++] = a[i], ++i;
    else pb[j] = m, out[m++] = b[j], ++j;
  }
  return m;
}

// ---- the stages of op_pack ------------------------------------------------------------------------------------------
struct Rows {  // what op_pack receives
  int64_t n, n_halo;
  const std::vector<int64_t> &row_ptr;
  const std::vector<int> &col;
  const std::vector<double> &val, &ext;
  const std::vector<int> *src;  // updatable operators: the source id 2 f + side of every entry, parallel to val (else null)
  int64_t len(int64_t r) const { return row_ptr[r + 1] - row_ptr[r]; }
  int64_t groups() const { return (n + 2 * kWave - 1) / (2 * kWave); }  // 128-row groups of paired rows (formats 3, 4)
};

int64_t longest_row(const Rows &A) {
  std::vector<int64_t> ml((size_t)host_threads(), 0);
  parallel_chunks(A.n, 1 << 16, [&](int t, int64_t b, int64_t e) {
    int64_t m = 0;
    for (int64_t i = b; i < e; ++i) m = std::max(m, A.len(i));
    ml[(size_t)t] = m;
  });
  return *std::max_element(ml.begin(), ml.end());
}

// Compact fp64 copy of an operator for the latency path (latency.hip: [ext 64 f64][col W x 64 i32][val W x 64 f64] per
// slice, slot-major); absent when the operator is too large, partitioned, or has rows longer than 64 entries.
void latency_image(const PackOptions &o, const Rows &A, std::vector<int64_t> &off, std::vector<char> &pack) {
  const int64_t n = A.n;
  if (o.latency_path == 0 || A.n_halo != 0 || n <= 0 || n > o.latency_rows) return;
  const int64_t n_slices = (n + kWave - 1) / kWave;
  off.assign((size_t)n_slices + 1, 0);
  for (int64_t s = 0; s < n_slices; ++s) {
    int64_t w = 0;
    for (int64_t r = s * kWave; r < std::min(n, (s + 1) * kWave); ++r) w = std::max(w, A.len(r));
    if (w > 64) {  // a very long row: the throughput path's CSR tail handles those
      off.clear();
      return;
    }
    off[(size_t)s + 1] = off[(size_t)s] + kWave * 8 + w * (kWave * 12);
  }
  pack.assign((size_t)off[(size_t)n_slices], 0);
  for (int64_t s = 0; s < n_slices; ++s) {
    const int width = (int)((off[(size_t)s + 1] - off[(size_t)s] - kWave * 8) / (kWave * 12));
    char *rec = pack.data() + off[(size_t)s];
    double *e_ = reinterpret_cast<double *>(rec);
    int *c_ = reinterpret_cast<int *>(rec + kWave * 8);
    double *v_ = reinterpret_cast<double *>(rec + kWave * 8 + (int64_t)width * (kWave * 4));
    for (int l = 0; l < kWave; ++l) {
      const int64_t r = s * kWave + l;
      e_[l] = r < n ? A.ext[(size_t)r] : 0.0;
      const int64_t b0 = r < n ? A.row_ptr[r] : 0, e0 = r < n ? A.row_ptr[r + 1] : 0;
      for (int k = 0; k < width; ++k) {
        const bool real = b0 + k < e0;
        c_[k * kWave + l] = real ? A.col[(size_t)(b0 + k)] : (int)(r < n ? r : n - 1);
        v_[k * kWave + l] = real ? A.val[(size_t)(b0 + k)] : 0.0;
      }
    }
  }
}

// Value dictionary (see the header comment of spmv.hip): lossless, so taken whenever the operator qualifies.
bool value_dictionary(const Rows &A, ValueDict &vd) {
  return vd.add(0.0) &&  // padding slots
         vd.add_all(A.n, [&](int64_t i) { return ValueDict::bits(A.ext[(size_t)i]); }) &&
         vd.add_all((int64_t)A.val.size(), [&](int64_t k) { return ValueDict::bits(A.val[(size_t)k]); });
}

// ... and the column offsets of the ELL part, the first w_op entries of every row (format 2)
bool offset_dictionary(const Rows &A, int64_t w_op, ValueDict &od) {
  bool co = od.find(0, true) >= 0;  // padding slots point at their own row
  std::vector<ValueDict> part((size_t)host_threads());
  std::vector<char> ok(part.size(), 1);
  const int T = parallel_chunks(A.n, 1 << 14, [&](int t, int64_t rb, int64_t re) {
    ValueDict &d = part[(size_t)t];
    for (int64_t r = rb; r < re; ++r) {
      const int64_t e = std::min(A.row_ptr[r + 1], A.row_ptr[r] + w_op);
      for (int64_t k = A.row_ptr[r]; k < e; ++k)
        if (d.find((uint64_t)((int64_t)A.col[(size_t)k] - r), true) < 0) {
          ok[(size_t)t] = 0;
          return;
        }
    }
  });
  for (int t = 0; co && t < T; ++t) {
    co = ok[(size_t)t] != 0;
    for (size_t q = 0; co && q < part[(size_t)t].values.size(); ++q) co = od.find(part[(size_t)t].values[q], true) >= 0;
  }
  return co;
}

// Format 3: consecutive rows share their gathers (see the header comment of spmv.hip).  The records of all groups into
// `pack`; returns the widest merged neighbour list, or 0 when some pair merges to more than 7 offsets or a gather
// would leave [guard, padding].
int paired_records(const Rows &A, ValueDict &vd, ValueDict &od, std::vector<char> &pack) {
  const int64_t n = A.n, n_total = A.n + A.n_halo;
  pack.assign((size_t)A.groups() * kPairRecBytes, 0);
  const uint64_t zero_v = (uint64_t)vd.index(0.0) << 3, zero_o = (uint64_t)od.find(0, false) << 2;
  std::atomic<int> pr_ok{1};
  std::vector<int> widths((size_t)host_threads(), 0);
  parallel_chunks(A.groups() * kWave, 1 << 13, [&](int t_, int64_t p_begin, int64_t p_end) {
    int pair_width = 0;  // (this thread's; folded below)
    for (int64_t p = p_begin; p < p_end && pr_ok.load(std::memory_order_relaxed); ++p) {
      const int64_t ra = 2 * p, rb = 2 * p + 1;
      int64_t oa[8], ob[8], merged[16];
      int pa[8], pb[8], na = 0, nb2 = 0;
      if (ra < n) for (int64_t k = A.row_ptr[ra]; k < A.row_ptr[ra + 1]; ++k) oa[na++] = (int64_t)A.col[(size_t)k] - ra;
      if (rb < n) for (int64_t k = A.row_ptr[rb]; k < A.row_ptr[rb + 1]; ++k) ob[nb2++] = (int64_t)A.col[(size_t)k] - rb;
      const int m = merge_offsets(oa, na, ob, nb2, merged, pa, pb);
      if (m > 7) { pr_ok = 0; break; }
      pair_width = std::max(pair_width, m);
      for (int k = 0; k < m; ++k)  // every 16-byte gather must stay inside [guard, padding]
        if (ra + merged[k] < -(int64_t)kVecGuard || rb + merged[k] > n_total + 3) pr_ok = 0;
      uint64_t wa = ra < n ? ((uint64_t)vd.lookup(A.ext[(size_t)ra]) << 3) : zero_v;
      uint64_t wb = rb < n ? ((uint64_t)vd.lookup(A.ext[(size_t)rb]) << 3) : zero_v;
      uint64_t jw = 0;
      for (int k = 0; k < 7; ++k) {
        wa |= zero_v << (8 * (k + 1)), wb |= zero_v << (8 * (k + 1));
        jw |= (k < m ? ((uint64_t)od.lookup((uint64_t)merged[k]) << 2) : zero_o) << (8 * k);
      }
      for (int k = 0; k < na; ++k) {
        wa &= ~(0xffull << (8 * (pa[k] + 1)));
        wa |= ((uint64_t)vd.lookup(A.val[(size_t)(A.row_ptr[ra] + k)]) << 3) << (8 * (pa[k] + 1));
      }
      for (int k = 0; k < nb2; ++k) {
        wb &= ~(0xffull << (8 * (pb[k] + 1)));
        wb |= ((uint64_t)vd.lookup(A.val[(size_t)(A.row_ptr[rb] + k)]) << 3) << (8 * (pb[k] + 1));
      }
      char *rec = pack.data() + (p / kWave) * kPairRecBytes;
      const int l = (int)(p % kWave);
      reinterpret_cast<uint64_t *>(rec)[2 * l] = wa;
      reinterpret_cast<uint64_t *>(rec)[2 * l + 1] = wb;
      reinterpret_cast<uint64_t *>(rec + 2 * kWave * 8)[l] = jw;
    }
    widths[(size_t)t_] = pair_width;
  });
  return pr_ok.load() != 0 ? *std::max_element(widths.begin(), widths.end()) : 0;
}

// The groups with a row that reads a halo column (they run behind the halo exchange); returns how many.
int64_t boundary_groups(const Rows &A, std::vector<char> &grp_bnd) {
  grp_bnd.assign((size_t)A.groups(), 0);
  if (A.n_halo == 0) return 0;
  std::vector<int64_t> cnt((size_t)host_threads(), 0);
  parallel_chunks(A.groups(), 1 << 10, [&](int t, int64_t gb, int64_t ge) {
    for (int64_t g = gb; g < ge; ++g) {
      const int64_t r1 = std::min<int64_t>(A.n, (g + 1) * 2 * kWave);
      for (int64_t k = A.row_ptr[g * 2 * kWave]; k < A.row_ptr[r1] && !grp_bnd[(size_t)g]; ++k) grp_bnd[(size_t)g] = A.col[(size_t)k] >= A.n;
      cnt[(size_t)t] += grp_bnd[(size_t)g];
    }
  });
  return std::accumulate(cnt.begin(), cnt.end(), (int64_t)0);
}

// Format 4 (see spmv_canon_kernel) asks that all rows list their neighbours in one common order of offsets.  A
// partitioned operator is MIXED: the common order is asked of the groups that read no halo column (a rank's slab of a
// structured box but for its outer planes), the others keep their format-3 records.
struct OffsetRelation {  // the distinct offsets and who precedes whom in some row
  int64_t dist[8];
  int nd = 0;
  bool before[8][8] = {};
  bool ok = true;  // at most 7 offsets, none twice in a row
};
OffsetRelation offset_relation(const Rows &A, const std::vector<char> &grp_bnd) {
  std::vector<OffsetRelation> loc((size_t)host_threads());
  const int T = parallel_chunks(A.n, 1 << 14, [&](int t, int64_t rb_, int64_t re_) {
    OffsetRelation &L = loc[(size_t)t];
    for (int64_t r = rb_; L.ok && r < re_; ++r) {
      if (grp_bnd[(size_t)(r / (2 * kWave))]) continue;
      int idx[8], no = 0;
      for (int64_t k = A.row_ptr[r]; L.ok && k < A.row_ptr[r + 1]; ++k) {
        const int64_t o = (int64_t)A.col[(size_t)k] - r;
        int q = 0;
        while (q < L.nd && L.dist[q] != o) ++q;
        if (q == L.nd) {
          if (L.nd == 7) { L.ok = false; break; }
          L.dist[L.nd++] = o;
        }
        idx[no++] = q;
      }
      for (int i = 0; L.ok && i < no; ++i)
        for (int j = i + 1; j < no; ++j) {
          if (idx[i] == idx[j]) L.ok = false;  // the same offset twice in one row
          L.before[idx[i]][idx[j]] = true;
        }
    }
  });
  OffsetRelation R;
  for (int t = 0; R.ok && t < T; ++t) {  // union of the threads' offsets and of their "precedes" relations
    const OffsetRelation &L = loc[(size_t)t];
    R.ok = L.ok;
    int map_[8];
    for (int q = 0; R.ok && q < L.nd; ++q) {
      int g = 0;
      while (g < R.nd && R.dist[g] != L.dist[q]) ++g;
      if (g == R.nd) {
        if (R.nd == 7) { R.ok = false; break; }
        R.dist[R.nd++] = L.dist[q];
      }
      map_[q] = g;
    }
    for (int i = 0; R.ok && i < L.nd; ++i)
      for (int j = 0; j < L.nd; ++j)
        if (L.before[i][j]) R.before[map_[i]][map_[j]] = true;
  }
  return R;
}
// A common order = a linear extension of the relation, and one the kernels have a variant for: 2, 4 or 6 offsets with
// -1, +1 in the middle.  Returns the number of offsets (0: none) and the slot of offset -1.
int common_offset_order(const OffsetRelation &R, int64_t *canon, int *canon_m1) {
  int len = 0, m1 = -1;
  bool placed[8] = {};
  while (R.ok && len < R.nd) {  // Kahn's algorithm; ties go to the smaller offset
    int pick = -1;
    for (int q = 0; q < R.nd; ++q) {
      if (placed[q]) continue;
      bool free_ = true;
      for (int q2 = 0; q2 < R.nd; ++q2) free_ = free_ && !(R.before[q2][q] && !placed[q2]);
      if (free_ && (pick < 0 || R.dist[q] < R.dist[pick])) pick = q;
    }
    if (pick < 0) return 0;  // a cycle: rows disagree about the order
    placed[pick] = true;
    canon[len++] = R.dist[pick];
  }
  for (int q = 0; q + 1 < len; ++q)
    if (canon[q] == -1 && canon[q + 1] == 1) m1 = q;
  bool cn = R.ok && ((len == 6 && m1 == 2) || (len == 4 && m1 == 1) || (len == 2 && m1 == 0));
  for (int q = 0; cn && q < len; ++q) cn = canon[q] > -(int64_t)INT32_MAX / 2 && canon[q] < (int64_t)INT32_MAX / 2;
  *canon_m1 = m1;
  return cn ? len : 0;
}

// The format-4 records of all groups: a row's weights in the slots of the common order.
void canonical_records(const Rows &A, const ValueDict &vd, uint64_t zero_v, const std::vector<char> &grp_bnd, const int64_t *canon,
                       std::vector<char> &pack) {
  const int64_t n = A.n;
  pack.assign((size_t)A.groups() * kCanonRecBytes, 0);
  parallel_chunks(A.groups() * kWave, 1 << 13, [&](int, int64_t p_begin, int64_t p_end) {
    for (int64_t p = p_begin; p < p_end; ++p) {
      uint64_t w2[2];
      for (int half = 0; half < 2; ++half) {
        const int64_t r = 2 * p + half;
        uint64_t w = r < n ? ((uint64_t)vd.lookup(A.ext[(size_t)r]) << 3) : zero_v;
        for (int k = 0; k < 7; ++k) w |= zero_v << (8 * (k + 1));
        if (r < n) {
          int q = 0;
          const bool by_entry = grp_bnd[(size_t)(r / (2 * kWave))] != 0;    // never applied from here: the weights
          for (int64_t k = A.row_ptr[r]; k < A.row_ptr[r + 1]; ++k) {       // only serve diag_sell_kernel
            if (by_entry) q = (int)(k - A.row_ptr[r]);
            else while (canon[q] != (int64_t)A.col[(size_t)k] - r) ++q;  // a subsequence of the common order
            w &= ~(0xffull << (8 * (q + 1)));
            w |= ((uint64_t)vd.lookup(A.val[(size_t)k]) << 3) << (8 * (q + 1));
          }
        }
        w2[half] = w;
      }
      uint64_t *rec = reinterpret_cast<uint64_t *>(pack.data() + (p / kWave) * kCanonRecBytes);
      rec[2 * (p % kWave)] = w2[0], rec[2 * (p % kWave) + 1] = w2[1];
    }
  });
}

// The row-record index: a lattice has a few dozen distinct row words (the interior class, walls, edges, corners); one
// byte per row naming the word in a table of them is what the tiled and marching kernels read (option
// spmv_record_index).  The 8-byte records stay: every other reader of the operator takes them.  Both stay empty when
// there are more than 256 distinct words.
void row_record_index(const std::vector<char> &pack, std::vector<uint8_t> &rec_idx, std::vector<uint64_t> &rec_words) {
  const int64_t n_words = (int64_t)pack.size() / 8;
  auto word_at = [&](int64_t i) {
    uint64_t w;
    memcpy(&w, pack.data() + (size_t)i * 8, 8);
    return w;
  };
  ValueDict wd;
  if (!wd.add_all(n_words, word_at)) return;
  rec_idx.resize((size_t)n_words);
  parallel_chunks(n_words, 1 << 16, [&](int, int64_t b, int64_t e) {
    for (int64_t i = b; i < e; ++i) rec_idx[(size_t)i] = (uint8_t)wd.lookup(word_at(i));
  });
  rec_words = std::move(wd.values);
}

// Formats 0 to 2: the width of every 64-row slice (its longest row up to the cap; w_op > 0, the 16-byte words of
// format 2: every slice padded to the operator's width) and the byte offsets of the slice records.
std::vector<int> slice_widths(const Rows &A, int64_t cap, int64_t slot_bytes, int64_t w_op, OpImage *img) {
  const int64_t n_slices = img->n_slices;
  std::vector<int> width((size_t)n_slices, 0);
  img->slice_off.assign((size_t)n_slices + 1, 0);
  bool uniform = true;
  for (int64_t s = 0; s < n_slices; ++s) {
    int64_t w = 0;
    const int64_t r1 = std::min<int64_t>(A.n, (s + 1) * kWave);
    for (int64_t r = s * kWave; r < r1; ++r) w = std::max(w, A.len(r));
    w = std::min(w, cap);
    if (w_op > 0) w = w_op;
    width[(size_t)s] = (int)w;
    img->slice_off[(size_t)s + 1] = img->slice_off[(size_t)s] + (w_op > 0 ? (int64_t)kWave * 16 : kExtBytes + w * slot_bytes);
    if (s > 0 && width[(size_t)s] != width[0]) uniform = false;
    img->ell_slots += w * kWave;
  }
  img->uniform_width = (uniform && n_slices > 0 && width[0] > 0) ? width[0] : 0;
  return width;
}
// ... and the records: fp64 (vd null), value-dictionary (format 1) or value + offset dictionary ones (format 2, od
// non-null), with the entries past a slice's width in the CSR tail and the slice lists.
void sell_records(const Rows &A, const std::vector<int> &width, ValueDict *vd, ValueDict *od, OpImage *img) {
  const int64_t n = A.n;
  const bool cv = vd != nullptr, co = od != nullptr;
  img->pack.assign((size_t)img->slice_off[(size_t)img->n_slices], 0);
  // the source map of an updatable operator (fp64 records only): one id per slot of every slice's val region, at the
  // slot's own index `at` behind the slots of the slices before it; padding slots -1
  if (A.src) img->src.assign((size_t)((img->slice_off[(size_t)img->n_slices] - img->n_slices * kExtBytes) / (kSlotBytes / kWave)), -1);
  for (int64_t s = 0; s < img->n_slices; ++s) {
    const int W = width[(size_t)s];
    char *rec = img->pack.data() + img->slice_off[(size_t)s];
    int *s_ = A.src ? img->src.data() + (img->slice_off[(size_t)s] - s * kExtBytes) / (kSlotBytes / kWave) : nullptr;
    double *e_ = reinterpret_cast<double *>(rec);
    uint64_t *i_ = reinterpret_cast<uint64_t *>(rec);  // cv: the index words take the place of ext
    int *c_ = reinterpret_cast<int *>(rec + kExtBytes);
    double *v_ = reinterpret_cast<double *>(rec + kExtBytes + (int64_t)W * (kWave * 4));
    bool touches_halo = false;
    for (int l = 0; l < kWave; ++l) {
      const int64_t r = s * kWave + l;
      const int64_t pad_col = r < n ? r : (n > 0 ? n - 1 : 0);
      const int64_t b = r < n ? A.row_ptr[r] : 0, e = r < n ? A.row_ptr[r + 1] : 0;
      uint64_t iw = 0, jw = 0;
      if (cv) iw = (uint64_t)vd->index(r < n ? A.ext[(size_t)r] : 0.0);
      else e_[l] = r < n ? A.ext[(size_t)r] : 0.0;
      if (co) {
        for (int k = 0; k < W; ++k) {
          const bool real = b + k < e;
          iw |= (uint64_t)vd->index(real ? A.val[(size_t)(b + k)] : 0.0) << (8 * (k + 1));
          jw |= (uint64_t)od->find(real ? (uint64_t)((int64_t)A.col[(size_t)(b + k)] - r) : 0, false) << (8 * k);
          touches_halo |= real && A.col[(size_t)(b + k)] >= n;
        }
        i_[2 * l] = iw, i_[2 * l + 1] = jw;
      }
      const int np2 = W >> 1;
      for (int k = 0; k < (co ? 0 : W); ++k) {
        // slots are stored in pairs: lane l reads (slot 2p, slot 2p+1) as one 8-byte column pair and
        // one 16-byte weight pair; an odd last slot is stored column-major behind the pairs
        const int at = (k < 2 * np2) ? ((k >> 1) * kWave + l) * 2 + (k & 1) : np2 * 2 * kWave + l;
        const bool real = b + k < e;
        c_[at] = real ? A.col[(size_t)(b + k)] : (int)pad_col;
        const double w_k = real ? A.val[(size_t)(b + k)] : 0.0;
        if (cv) iw |= (uint64_t)vd->index(w_k) << (8 * (k + 1));
        else v_[at] = w_k;
        if (s_ && real) s_[at] = (*A.src)[(size_t)(b + k)];
        touches_halo |= real && c_[at] >= n;
      }
      if (cv && !co) i_[l] = iw;
      if (e - b > W) {
        img->tail_row.push_back((int)r);
        for (int64_t k = b + W; k < e; ++k) {
          img->tail_col.push_back(A.col[(size_t)k]);
          img->tail_val.push_back(A.val[(size_t)k]);
          if (A.src) img->tail_src.push_back((*A.src)[(size_t)k]);
          touches_halo |= A.col[(size_t)k] >= n;
        }
        img->tail_ptr.push_back((int64_t)img->tail_col.size());
      }
    }
    (touches_halo ? img->boundary : img->interior).push_back((int)s);
  }
}

// The kDictSize-entry tables the kernels index, from the dictionaries.
void dictionary_tables(const ValueDict *vd, const ValueDict *od, OpImage *img) {
  if (vd) {
    img->dict.assign((size_t)kDictSize, 0.0);
    for (size_t k = 0; k < vd->values.size(); ++k) memcpy(&img->dict[k], &vd->values[k], 8);
    img->dict_size = (int)vd->values.size();
  }
  if (od) {
    img->offs.assign((size_t)kDictSize, 0);
    for (size_t k = 0; k < od->values.size(); ++k) img->offs[k] = (int)(int64_t)od->values[k];
    img->offs_size = (int)od->values.size();
  }
}

}  // namespace

// The most compact lossless format the operator qualifies for, capped by option spmv_dict: 4 (common offset order),
// 3 (paired rows), 2 (value + offset dictionary), 1 (value dictionary), 0 (fp64 sliced ELL).
// `src` (updatable operators, PackOptions::updatable): the source id of every entry; the operator then keeps its fp64
// records whatever it would qualify for, carries the source map (OpImage::src, tail_src) and forms no latency copy.
int op_pack(const PackOptions &options, int64_t n, int64_t n_halo, const std::vector<int64_t> &row_ptr, const std::vector<int> &col,
            const std::vector<double> &val, const std::vector<double> &ext, OpImage *img, const std::vector<int> *src) {
  PackOptions o = options;
  if (src) o.spmv_dict = 0, o.latency_path = 0;
  const Rows A{n, n_halo, row_ptr, col, val, ext, src};
  *img = OpImage();
  img->n_rows = n, img->n_halo = n_halo, img->nnz = row_ptr[n];
  BuildTimer timer;
  const int64_t max_len = img->max_row_len = longest_row(A);
  latency_image(o, A, img->lat_off, img->lat_pack);
  int64_t cap = o.ell_cap;
  if (cap <= 0) {
    const double mean = n > 0 ? (double)img->nnz / (double)n : 0.0;
    cap = std::max<int64_t>(8, (int64_t)std::ceil(2.0 * mean));
  }
  const int64_t w_op = std::min(max_len, cap);  // the width of the ELL part
  timer.lap("latency copy, max row");
  ValueDict vd, od;
  const bool cv = o.spmv_dict != 0 && w_op <= 7 && value_dictionary(A, vd);
  timer.lap("value dictionary");
  const bool co = cv && o.spmv_dict >= 2 && w_op > 0 && n + n_halo < (int64_t)INT32_MAX && offset_dictionary(A, w_op, od);
  timer.lap("offset dictionary");
  const int64_t n_groups = A.groups();
  const int pair_width = co && o.spmv_dict >= 3 && max_len <= std::min<int64_t>(7, cap) && vd.values.size() <= 32 &&
                                 od.values.size() <= 64 && n + n_halo < ((int64_t)1 << 28)
                             ? paired_records(A, vd, od, img->pack)
                             : 0;
  timer.lap("paired records");
  const bool pr = pair_width > 0;
  img->tail_ptr.assign(1, 0);
  std::vector<char> grp_bnd;
  const int64_t n_bnd_groups = pr ? boundary_groups(A, grp_bnd) : 0;
  int64_t canon[8];
  int canon_len = 0, canon_m1 = -1;
  if (pr && o.spmv_dict >= 4 && 2 * n_bnd_groups <= n_groups && (n_bnd_groups == 0 || o.spmv_mixed != 0))
    canon_len = common_offset_order(offset_relation(A, grp_bnd), canon, &canon_m1);
  if (canon_len > 0) {
    for (int64_t g = 0; g < n_groups; ++g)  // the format-3 records of the boundary groups, in list order
      if (grp_bnd[(size_t)g])
        img->bnd_pack.insert(img->bnd_pack.end(), img->pack.begin() + (size_t)g * kPairRecBytes, img->pack.begin() + (size_t)(g + 1) * kPairRecBytes);
    canonical_records(A, vd, (uint64_t)vd.index(0.0) << 3, grp_bnd, canon, img->pack);
    timer.lap("canonical order + records");
    row_record_index(img->pack, img->rec_idx, img->rec_words);
    timer.lap("row-record index");
    img->canon_k = canon_len, img->canon_m1 = canon_m1;
    for (int k = 0; k < canon_len; ++k) img->canon_off[k] = (int)canon[k];
  }
  if (pr) {  // format 3 (or 4) it is: a "slice" of this operator is a 128-row group
    const int rec_bytes = canon_len > 0 ? kCanonRecBytes : kPairRecBytes;
    img->pair = canon_len > 0 ? 2 : 1;
    img->bnd_width = pair_width;
    img->uniform_width = canon_len > 0 ? canon_len : pair_width;
    img->n_slices = n_groups;
    img->ell_slots = n_groups * 2 * kWave * img->uniform_width;
    img->slice_off.resize((size_t)n_groups + 1);
    for (int64_t s = 0; s <= n_groups; ++s) img->slice_off[(size_t)s] = s * rec_bytes;
    for (int64_t s = 0; s < n_groups; ++s) (grp_bnd[(size_t)s] ? img->boundary : img->interior).push_back((int)s);
    img->spw = 1;
  } else {
    img->n_slices = (n + kWave - 1) / kWave;
    sell_records(A, slice_widths(A, cap, cv ? kColSlotBytes : kSlotBytes, co ? w_op : 0, img), cv ? &vd : nullptr, co ? &od : nullptr, img);
    img->spw = (o.spmv_spw == 1 || o.spmv_spw == 2 || o.spmv_spw == 4) ? o.spmv_spw : 2;
  }
  dictionary_tables(cv ? &vd : nullptr, co ? &od : nullptr, img);
  img->tail_rows = (int64_t)img->tail_row.size();
  img->tail_nnz = (int64_t)img->tail_col.size();
  img->pack_bytes = (int64_t)img->pack.size() + (int64_t)img->bnd_pack.size();
  return STORM_HIP_OK;
}

namespace {

// Rows of the operator from its faces, entries in FACE ORDER (== the order in which the reference's face loop
// accumulates into u[i]): entry (a -> b) of face f carries weight(f, false), entry (b -> a) weight(f, true).
// Threaded over CHUNKS OF FACES: a chunk counts its entries per row (one byte per row and chunk), a prefix over the
// chunks turns the counts into each chunk's first position inside every row, and the chunks then fill their entries
// -- two passes over the faces whatever the thread count, and the order inside a row does not depend on it.
// (A row that takes > 255 entries from one chunk: every thread scans all faces for its own range of rows instead.)
template <class W>
void rows_from_faces(int64_t n_owned, int64_t n_faces, const int64_t *inner, const int64_t *outer, W &&weight,
                     std::vector<int64_t> &row_ptr, std::vector<int> &col, std::vector<double> &val, std::vector<int> *src = nullptr) {
  row_ptr.assign((size_t)n_owned + 1, 0);
  // one entry: its column, its weight and -- where asked for -- its source id 2 f + side (side 1: the entry of row outer[f])
  auto put = [&](size_t at, int64_t c, int64_t f, bool outer_side) {
    col[at] = (int)c, val[at] = weight(f, outer_side);
    if (src) (*src)[at] = (int)(2 * f + (outer_side ? 1 : 0));
  };
  const int64_t face_chunk = forced_min_chunk() > 0 ? forced_min_chunk() : (1 << 16);
  const int T = (int)std::max<int64_t>(1, std::min<int64_t>(host_threads(), n_faces / face_chunk));
  const int64_t per = (n_faces + T - 1) / T;
  std::vector<std::vector<unsigned char>> cnt((size_t)T);
  std::atomic<int> overflow{0};
  parallel_chunks(T, 1, [&](int, int64_t tb, int64_t te) {
    for (int64_t t = tb; t < te; ++t) {
      std::vector<unsigned char> &c_ = cnt[(size_t)t];
      c_.assign((size_t)n_owned, 0);
      for (int64_t f = t * per; f < std::min(n_faces, (t + 1) * per); ++f) {
        const int64_t a = inner[f], b = outer[f];
        if (a < n_owned && ++c_[(size_t)a] == 0) overflow = 1;
        if (b < n_owned && ++c_[(size_t)b] == 0) overflow = 1;
      }
    }
  });
  if (overflow.load()) {
    parallel_chunks(n_owned, 1 << 15, [&](int, int64_t r0, int64_t r1) {
      for (int64_t f = 0; f < n_faces; ++f) {
        const int64_t a = inner[f], b = outer[f];
        if (a >= r0 && a < r1) row_ptr[(size_t)a + 1]++;
        if (b >= r0 && b < r1) row_ptr[(size_t)b + 1]++;
      }
    });
    for (int64_t i = 0; i < n_owned; ++i) row_ptr[(size_t)i + 1] += row_ptr[(size_t)i];
    col.resize((size_t)row_ptr[(size_t)n_owned]), val.resize(col.size());
    if (src) src->resize(col.size());
    std::vector<int64_t> fill(row_ptr.begin(), row_ptr.end() - 1);
    parallel_chunks(n_owned, 1 << 15, [&](int, int64_t r0, int64_t r1) {
      for (int64_t f = 0; f < n_faces; ++f) {
        const int64_t a = inner[f], b = outer[f];
        if (a >= r0 && a < r1) {
          const size_t at = (size_t)fill[(size_t)a]++;
          put(at, b, f, false);
        }
        if (b >= r0 && b < r1) {
          const size_t at = (size_t)fill[(size_t)b]++;
          put(at, a, f, true);
        }
      }
    });
    return;
  }
  // counts -> each chunk's offset inside the row (in place), row lengths -> row_ptr
  parallel_chunks(n_owned, 1 << 16, [&](int, int64_t r0, int64_t r1) {
    for (int64_t r = r0; r < r1; ++r) {
      int64_t run = 0;
      for (int t = 0; t < T; ++t) {
        const int64_t here = cnt[(size_t)t][(size_t)r];
        cnt[(size_t)t][(size_t)r] = (unsigned char)run;  // (a row of > 255 entries in all: the serial prefix below still holds
        run += here;                                     //  the truth; positions are taken modulo 256 only when run < 256)
      }
      row_ptr[(size_t)r + 1] = run;
    }
  });
  bool long_rows = false;
  for (int64_t i = 0; i < n_owned; ++i) {
    long_rows |= row_ptr[(size_t)i + 1] > 255;
    row_ptr[(size_t)i + 1] += row_ptr[(size_t)i];
  }
  col.resize((size_t)row_ptr[(size_t)n_owned]), val.resize(col.size());
  if (src) src->resize(col.size());
  if (long_rows) {  // (offsets no longer fit a byte: one thread, plain fill)
    std::vector<int64_t> fill(row_ptr.begin(), row_ptr.end() - 1);
    for (int64_t f = 0; f < n_faces; ++f) {
      const int64_t a = inner[f], b = outer[f];
      if (a < n_owned) {
        const size_t at = (size_t)fill[(size_t)a]++;
        put(at, b, f, false);
      }
      if (b < n_owned) {
        const size_t at = (size_t)fill[(size_t)b]++;
        put(at, a, f, true);
      }
    }
    return;
  }
  parallel_chunks(T, 1, [&](int, int64_t tb, int64_t te) {
    for (int64_t t = tb; t < te; ++t) {
      std::vector<unsigned char> &o_ = cnt[(size_t)t];
      for (int64_t f = t * per; f < std::min(n_faces, (t + 1) * per); ++f) {
        const int64_t a = inner[f], b = outer[f];
        if (a < n_owned) {
          const size_t at = (size_t)(row_ptr[(size_t)a] + o_[(size_t)a]++);
          put(at, b, f, false);
        }
        if (b < n_owned) {
          const size_t at = (size_t)(row_ptr[(size_t)b] + o_[(size_t)b]++);
          put(at, a, f, true);
        }
      }
    }
  });
}

// inner / outer of every face inside [0, nt) and distinct; returns the first offending face or -1
int64_t first_bad_face(int64_t n_faces, const int64_t *inner, const int64_t *outer, int64_t nt) {
  std::atomic<int64_t> bad{-1};
  parallel_chunks(n_faces, 1 << 16, [&](int, int64_t fb, int64_t fe) {
    for (int64_t f = fb; f < fe; ++f) {
      const int64_t a = inner[f], b = outer[f];
      if (!(a >= 0 && a < nt && b >= 0 && b < nt) || a == b) {
        int64_t cur = bad.load();
        while ((cur < 0 || f < cur) && !bad.compare_exchange_weak(cur, f)) {
        }
        return;
      }
    }
  });
  return bad.load();
}
// Validate on the host once, instead of the reference's per-access STORM_ASSERT bounds checks
// (Utils/Table.hpp:150-154, Feathers/Field.hpp:93-101): a bad index must never reach a kernel.
int require_valid_faces(const char *who, int64_t n_faces, const int64_t *inner, const int64_t *outer, int64_t nt) {
  const int64_t f = first_bad_face(n_faces, inner, outer, nt);
  if (f < 0) return STORM_HIP_OK;
  const int64_t a = inner[f], b = outer[f];
  STORM_REQUIRE(a >= 0 && a < nt && b >= 0 && b < nt, "%s: face %lld joins cells (%lld, %lld) outside [0, %lld)", who,
                (long long)f, (long long)a, (long long)b, (long long)nt);
  STORM_REQUIRE(a != b, "%s: face %lld joins cell %lld to itself", who, (long long)f, (long long)a);
  return STORM_HIP_OK;
}

// from_faces / from_mesh share everything but where a face's transmissibility A_f / d_f comes from
template <class Coef, class BCoef>
int pack_from_faces_impl(const PackOptions &o, int64_t n_owned, int64_t n_halo, int64_t n_faces, const int64_t *inner,
                         const int64_t *outer, Coef &&coef, int64_t n_bfaces, const int64_t *b_cell, BCoef &&b_coef,
                         const double *volume, OpImage *img, const char *who) {
  const int64_t nt = n_owned + n_halo;
  STORM_REQUIRE(nt < (int64_t)INT32_MAX, "%s: %lld cells exceed int32 indexing", who, (long long)nt);
  BuildTimer timer;
  for (int64_t i = 0; i < nt; ++i)
    STORM_REQUIRE(volume[i] > 0.0, "%s: cell %lld has volume %g", who, (long long)i, volume[i]);
  STORM_TRY(require_valid_faces(who, n_faces, inner, outer, nt));
  std::vector<int64_t> row_ptr;
  std::vector<int> col;
  std::vector<double> val;
  // w_in = (A_f / d_f) / V_in, w_out = (A_f / d_f) / V_out      Playground.cpp:126-129
  rows_from_faces(n_owned, n_faces, inner, outer,
                  [&](int64_t f, bool outer_side) { return coef(f) / volume[outer_side ? outer[f] : inner[f]]; }, row_ptr, col, val);
  timer.lap("rows from faces");
  std::vector<double> ext((size_t)n_owned, 0.0);
  for (int64_t k = 0; k < n_bfaces; ++k) {  // flux to a zero ghost state at the wall
    const int64_t i = b_cell[k];
    STORM_REQUIRE(i >= 0 && i < n_owned, "%s: boundary face %lld on cell %lld outside [0, %lld)", who, (long long)k,
                  (long long)i, (long long)n_owned);
    ext[(size_t)i] -= b_coef(k) / volume[i];
  }
  return op_pack(o, n_owned, n_halo, row_ptr, col, val, ext, img);
}

// length(a - b) as the reference forms it (MatrixAlgorithms.hpp:303-305 -> norm_2 :262-270): squares added left to
// right, one rounding per operation (no contraction: the coefficients must be the bits the host's numpy / the
// reference's scalar loop give).
inline double center_distance(const double *a, const double *b, int dim) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  double s = 0.0;
  for (int k = 0; k < dim; ++k) {
    const double d = a[k] - b[k];
    s = s + d * d;
  }
  return sqrt(s);
}

}  // namespace

int op_pack_from_face_weights(const PackOptions &o, int64_t n_owned, int64_t n_halo, int64_t n_faces, const int64_t *inner,
                              const int64_t *outer, const double *w_inner, const double *w_outer, const double *diag_extra,
                              OpImage *img) {
  STORM_REQUIRE(n_owned >= 0 && n_halo >= 0 && n_faces >= 0, "op_create: negative size");
  STORM_REQUIRE(n_faces == 0 || (inner && outer && w_inner && w_outer), "op_create: null face array");
  const int64_t nt = n_owned + n_halo;
  STORM_REQUIRE(nt < (int64_t)INT32_MAX, "op_create: %lld cells exceed int32 indexing", (long long)nt);
  STORM_REQUIRE(o.updatable == 0 || n_faces < ((int64_t)1 << 30), "op_create: %lld faces exceed the 2^30 an updatable operator's int32 source ids hold",
                (long long)n_faces);
  BuildTimer timer;
  STORM_TRY(require_valid_faces("op_create", n_faces, inner, outer, nt));
  std::vector<int64_t> row_ptr;
  std::vector<int> col, src;
  std::vector<double> val;
  rows_from_faces(n_owned, n_faces, inner, outer, [&](int64_t f, bool outer_side) { return outer_side ? w_outer[f] : w_inner[f]; },
                  row_ptr, col, val, o.updatable != 0 ? &src : nullptr);
  timer.lap("rows from faces");
  std::vector<double> ext((size_t)n_owned, 0.0);
  if (diag_extra) std::copy(diag_extra, diag_extra + n_owned, ext.begin());
  STORM_TRY(op_pack(o, n_owned, n_halo, row_ptr, col, val, ext, img, o.updatable != 0 ? &src : nullptr));
  if (o.updatable != 0) {  // the faces' cells, for cells_to_faces (int32: nt < 2^31 was checked above)
    img->updatable = 1, img->n_faces = n_faces;
    img->face_inner.assign(inner, inner + n_faces), img->face_outer.assign(outer, outer + n_faces);
  }
  return STORM_HIP_OK;
}

int op_pack_from_faces(const PackOptions &o, int64_t n_owned, int64_t n_halo, int64_t n_faces, const int64_t *inner,
                       const int64_t *outer, const double *coef, int64_t n_bfaces, const int64_t *b_cell, const double *b_coef,
                       const double *volume, OpImage *img) {
  STORM_REQUIRE(n_owned >= 0 && n_halo >= 0 && n_faces >= 0 && n_bfaces >= 0, "op_create_from_faces: negative size");
  STORM_REQUIRE(volume && (n_faces == 0 || (inner && outer && coef)) && (n_bfaces == 0 || (b_cell && b_coef)),
                "op_create_from_faces: null array");
  return pack_from_faces_impl(o, n_owned, n_halo, n_faces, inner, outer, [&](int64_t f) { return coef[f]; }, n_bfaces, b_cell,
                              [&](int64_t k) { return b_coef[k]; }, volume, img, "op_create_from_faces");
}

int op_pack_from_mesh(const PackOptions &o, int64_t n_owned, int64_t n_halo, int32_t dim, int64_t n_faces, const int64_t *inner,
                      const int64_t *outer, const double *area, const double *center, int64_t n_bfaces, const int64_t *b_cell,
                      const double *b_area, const double *b_center, const double *volume, OpImage *img) {
  STORM_REQUIRE(n_owned >= 0 && n_halo >= 0 && n_faces >= 0 && n_bfaces >= 0 && dim >= 1 && dim <= 3,
                "op_create_from_mesh: bad size (dim = %d)", (int)dim);
  STORM_REQUIRE(volume && center && (n_faces == 0 || (inner && outer && area)) && (n_bfaces == 0 || (b_cell && b_area && b_center)),
                "op_create_from_mesh: null array");
  return pack_from_faces_impl(
      o, n_owned, n_halo, n_faces, inner, outer,
      [&](int64_t f) { return area[f] / center_distance(center + outer[f] * dim, center + inner[f] * dim, dim); }, n_bfaces, b_cell,
      [&](int64_t k) { return b_area[k] / center_distance(b_center + k * dim, center + b_cell[k] * dim, dim); }, volume, img,
      "op_create_from_mesh");
}

int op_pack_csr(const PackOptions &o, int64_t n_rows, int64_t n_halo, const int64_t *row_ptr, const int64_t *col,
                const double *val, OpImage *img) {
  STORM_REQUIRE(n_rows >= 0 && n_halo >= 0, "op_create_csr: negative size");
  const int64_t nt = n_rows + n_halo;
  STORM_REQUIRE(nt < (int64_t)INT32_MAX, "op_create_csr: %lld columns exceed int32 indexing", (long long)nt);
  STORM_REQUIRE(row_ptr[0] == 0, "op_create_csr: row_ptr[0] != 0");
  std::vector<int64_t> rp((size_t)n_rows + 1, 0);
  std::vector<int> oc;
  std::vector<double> ov;
  std::vector<double> ext((size_t)n_rows, 0.0);
  oc.reserve((size_t)row_ptr[n_rows]);
  ov.reserve((size_t)row_ptr[n_rows]);
  for (int64_t i = 0; i < n_rows; ++i) {
    STORM_REQUIRE(row_ptr[i + 1] >= row_ptr[i], "op_create_csr: row_ptr not monotone at row %lld", (long long)i);
    double rowsum = 0.0;  // M x = sum_j a_ij (x_j - x_i) + (sum_j a_ij) x_i
    for (int64_t k = row_ptr[i]; k < row_ptr[i + 1]; ++k) {
      STORM_REQUIRE(col[k] >= 0 && col[k] < nt, "op_create_csr: column %lld of row %lld outside [0, %lld)",
                    (long long)col[k], (long long)i, (long long)nt);
      rowsum += val[k];
      if (col[k] != i) {
        oc.push_back((int)col[k]);
        ov.push_back(val[k]);
      }
    }
    ext[(size_t)i] = rowsum;
    rp[(size_t)i + 1] = (int64_t)oc.size();
  }
  return op_pack(o, n_rows, n_halo, rp, oc, ov, ext, img);
}

}  // namespace storm
