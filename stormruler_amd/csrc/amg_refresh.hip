// Refreshable multigrid objects (storm_hip_amg_create_refreshable, _refresh, _download): every number of a hierarchy
// recomputed on the device from the operator's current records, on the structure the host setup froze once (the number of
// levels, the aggregates, the strong masks and the patterns of A_l, P_l, R_l and A_l P_l).  The frozen-structure recipe:
// include/storm_hip.h; restated in tests/amg_refresh_ref.py.
//
// What the object keeps beside a plain one (all counted in "refresh_bytes"): per level A_l as CSR with a value array, its
// strong mask and aggregates, P_l as CSR with a value array, the pattern of R_l with the entry of P_l behind each entry,
// A_l P_l as CSR with a value array, and the slot -> entry maps of the transfer records; for level 0 the slot -> entry map of
// the operator's records.  LEVEL 0 KEEPS A CSR COPY (pattern, values, mask): the products read it, not the records.
//
// Kernels (build-time launches like op_refresh_*: no api_done word).  One wavefront per slice of 64 rows and one row per
// lane; every output row is written by its own lane only, so there is no atomic on a floating-point value and the bits do
// not depend on the launch.  Order of summation inside a row: the entries of A_l in column order (steps 2 to 4 and A P), the
// entries of R_l in column order, i.e. fine rows ascending (R (A P)); level 0 sums the slots in slot order, then the tail.
//   amg_rf_decode_kernel    level 0: the records (and CSR tail) into A_0's values through the slot -> entry map
//   amg_rf_filter_kernel    a^F_ii and the row's ratio sum_j |a^F_ij| / |a^F_ii|; the wavefront's maximum; a zero or
//                           non-finite a^F_ii leaves its row in a flag word (integer atomicMin), read at the next wait
//   amg_rf_max_kernel       one block folds the wavefronts' maxima
//   amg_rf_prolong_kernel   the prolongator rows into P's values
//   amg_rf_ap_kernel        A_l P_l into its frozen pattern (a contribution finds its slot by bisection of the sorted row)
//   amg_rf_rap_kernel       R_l (A_l P_l) into A_{l+1}'s frozen pattern, R's values read through P's
//   amg_rf_transfer_kernel  the transfer records' weights from P's values through the slot maps
//   amg_rf_op_kernel / amg_rf_tail_kernel  a coarse operator's records (ext = the row sum in column order, the slots through
//                           the source map) and CSR tail from A_{l+1}'s values
// A product is rounded before it is added (__dmul_rn): the sums are the host setup's, term by term.
#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstring>

#include "amg.hpp"
#include "op_layout.hpp"

namespace storm {

__device__ __forceinline__ int rf_slot_at(int k, int np2, int lane) {  // sell_records' slot addressing
  return (k < 2 * np2) ? ((k >> 1) * kWave + lane) * 2 + (k & 1) : np2 * 2 * kWave + lane;
}

// the first position in [lo, hi) of the sorted cols whose column is >= key
__device__ __forceinline__ int64_t rf_lower_bound(const int *__restrict__ cols, int64_t lo, int64_t hi, int key) {
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (cols[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kBlock) void amg_rf_decode_kernel(const char *__restrict__ pack, const int64_t *__restrict__ slice_off,
                                                               const int *__restrict__ slot_ent, int64_t n_rows, int64_t n_slices,
                                                               double alpha, double beta, const int64_t *__restrict__ a_ptr,
                                                               const int *__restrict__ a_diag, double *a_val,
                                                               const int *__restrict__ tail_of, const int64_t *__restrict__ tail_ptr,
                                                               const double *__restrict__ tail_val, const int *__restrict__ tail_ent) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t s = (int64_t)blockIdx.x * (kBlock / kWave) + wave;
  if (s >= n_slices) return;
  const int64_t row = s * kWave + lane;
  const bool valid = row < n_rows;
  const int64_t base = slice_off[s];
  const int width = (int)((slice_off[s + 1] - base - kExtBytes) / kSlotBytes);
  const char *rec = pack + base;
  const double ext = __builtin_nontemporal_load(reinterpret_cast<const double *>(rec) + lane);
  const double *val = reinterpret_cast<const double *>(rec + kExtBytes + (int64_t)width * (kWave * 4));
  const int *ent = slot_ent + (base - s * kExtBytes) / (kSlotBytes / kWave);
  const int np2 = width >> 1;
  const int64_t e0 = valid ? a_ptr[row] : 0, e1 = valid ? a_ptr[row + 1] : 0;
  for (int64_t e = e0; e < e1; ++e) a_val[e] = 0.0;
  double sum = 0.0;
  for (int k = 0; k < width; ++k) {
    const int at = rf_slot_at(k, np2, lane);
    const int id = __builtin_nontemporal_load(ent + at);
    const double v = __builtin_nontemporal_load(val + at);
    if (!valid || id == -1) continue;  // padding
    sum += v;
    if (id >= 0) a_val[id] += v;
  }
  if (valid && tail_of != nullptr) {
    const int t = tail_of[row];
    if (t >= 0)
      for (int64_t k = tail_ptr[t]; k < tail_ptr[t + 1]; ++k) {
        const double v = tail_val[k];
        const int id = tail_ent[k];
        sum += v;
        if (id >= 0) a_val[id] += v;
      }
  }
  if (!valid) return;
  const int64_t dg = e0 + a_diag[row];
  for (int64_t e = e0; e < e1; ++e)
    if (e != dg) a_val[e] = __dmul_rn(alpha, a_val[e]);
  a_val[dg] = __dadd_rn(beta, __dmul_rn(alpha, ext - sum));
}

__global__ __launch_bounds__(kBlock) void amg_rf_filter_kernel(int64_t n_rows, int64_t n_slices, const int64_t *__restrict__ a_ptr,
                                                               const double *__restrict__ a_val, const uint8_t *__restrict__ strong,
                                                               const int *__restrict__ a_diag, double *__restrict__ df,
                                                               double *__restrict__ wave_max, int *bad) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t s = (int64_t)blockIdx.x * (kBlock / kWave) + wave;
  if (s >= n_slices) return;
  const int64_t row = s * kWave + lane;
  double ratio = 0.0;
  if (row < n_rows) {
    const int64_t e0 = a_ptr[row], e1 = a_ptr[row + 1], dg = e0 + a_diag[row];
    double weak = 0.0, sum_abs = 0.0;
    for (int64_t e = e0; e < e1; ++e) {
      if (e == dg) continue;
      const double v = a_val[e];
      if (strong[e]) sum_abs += fabs(v);
      else weak += v;
    }
    const double d = a_val[dg] + weak;
    df[row] = d;
    if (d != 0.0 && isfinite(d)) ratio = (sum_abs + fabs(d)) / fabs(d);
    else atomicMin(bad, (int)row);
  }
  for (int off = kWave / 2; off > 0; off >>= 1) ratio = fmax(ratio, __shfl_xor(ratio, off));
  if (lane == 0) wave_max[s] = ratio;
}

__global__ __launch_bounds__(kBlock) void amg_rf_max_kernel(const double *__restrict__ wave_max, int64_t m, double *__restrict__ out) {
  __shared__ double part[kBlock];
  double v = 0.0;
  for (int64_t i = threadIdx.x; i < m; i += kBlock) v = fmax(v, wave_max[i]);
  part[threadIdx.x] = v;
  __syncthreads();
  for (int off = kBlock / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) part[threadIdx.x] = fmax(part[threadIdx.x], part[threadIdx.x + off]);
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = part[0];
}

// P_iJ = [J = agg(i)] - (c / a^F_ii) sum_{j in J} a^F_ij, the sum over the row's entries in column order
__global__ __launch_bounds__(kBlock) void amg_rf_prolong_kernel(int64_t n_rows, int64_t n_slices, const int64_t *__restrict__ a_ptr,
                                                                const int *__restrict__ a_col, const double *__restrict__ a_val,
                                                                const uint8_t *__restrict__ strong, const int *__restrict__ a_diag,
                                                                const int *__restrict__ agg, const double *__restrict__ df, double c,
                                                                const int64_t *__restrict__ p_ptr, const int *__restrict__ p_col,
                                                                double *__restrict__ p_val) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t s = (int64_t)blockIdx.x * (kBlock / kWave) + wave;
  if (s >= n_slices) return;
  const int64_t row = s * kWave + lane;
  if (row >= n_rows) return;
  const int64_t e0 = a_ptr[row], e1 = a_ptr[row + 1], dg = e0 + a_diag[row];
  const double d = df[row], f = c / d;
  const int mine = agg[row];
  for (int64_t q = p_ptr[row]; q < p_ptr[row + 1]; ++q) {
    const int J = p_col[q];
    double sum = 0.0;
    for (int64_t e = e0; e < e1; ++e) {
      if (e != dg && !strong[e]) continue;
      if (agg[a_col[e]] != J) continue;
      sum += e == dg ? d : a_val[e];
    }
    p_val[q] = __dsub_rn(J == mine ? 1.0 : 0.0, __dmul_rn(f, sum));
  }
}

__global__ __launch_bounds__(kBlock) void amg_rf_ap_kernel(int64_t n_rows, int64_t n_slices, const int64_t *__restrict__ a_ptr,
                                                           const int *__restrict__ a_col, const double *__restrict__ a_val,
                                                           const int64_t *__restrict__ p_ptr, const int *__restrict__ p_col,
                                                           const double *__restrict__ p_val, const int64_t *__restrict__ ap_ptr,
                                                           const int *__restrict__ ap_col, double *ap_val) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t s = (int64_t)blockIdx.x * (kBlock / kWave) + wave;
  if (s >= n_slices) return;
  const int64_t row = s * kWave + lane;
  if (row >= n_rows) return;
  const int64_t o0 = ap_ptr[row], o1 = ap_ptr[row + 1];
  for (int64_t o = o0; o < o1; ++o) ap_val[o] = 0.0;
  for (int64_t e = a_ptr[row]; e < a_ptr[row + 1]; ++e) {
    const int j = a_col[e];
    const double x = a_val[e];
    for (int64_t q = p_ptr[j]; q < p_ptr[j + 1]; ++q) {
      const int J = p_col[q];
      const int64_t o = rf_lower_bound(ap_col, o0, o1, J);
      if (o < o1 && ap_col[o] == J) ap_val[o] += __dmul_rn(x, p_val[q]);
    }
  }
}

__global__ __launch_bounds__(kBlock) void amg_rf_rap_kernel(int64_t n_rows, int64_t n_slices, const int64_t *__restrict__ r_ptr,
                                                            const int *__restrict__ r_col, const int *__restrict__ r_of,
                                                            const double *__restrict__ p_val, const int64_t *__restrict__ ap_ptr,
                                                            const int *__restrict__ ap_col, const double *__restrict__ ap_val,
                                                            const int64_t *__restrict__ n_ptr, const int *__restrict__ n_col,
                                                            double *n_val) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t s = (int64_t)blockIdx.x * (kBlock / kWave) + wave;
  if (s >= n_slices) return;
  const int64_t row = s * kWave + lane;
  if (row >= n_rows) return;
  const int64_t o0 = n_ptr[row], o1 = n_ptr[row + 1];
  for (int64_t o = o0; o < o1; ++o) n_val[o] = 0.0;
  for (int64_t k = r_ptr[row]; k < r_ptr[row + 1]; ++k) {
    const int i = r_col[k];
    const double x = p_val[r_of[k]];
    for (int64_t q = ap_ptr[i]; q < ap_ptr[i + 1]; ++q) {
      const int J = ap_col[q];
      const int64_t o = rf_lower_bound(n_col, o0, o1, J);
      if (o < o1 && n_col[o] == J) n_val[o] += __dmul_rn(x, ap_val[q]);
    }
  }
}

// The weights of transfer records ([col W x 64 int32][val W x 64 fp64] per slice) from P's values; padding gets 0.
__global__ __launch_bounds__(kBlock) void amg_rf_transfer_kernel(char *__restrict__ pack, const int64_t *__restrict__ off,
                                                                 int64_t n_slices, const int *__restrict__ slot_map,
                                                                 const double *__restrict__ p_val) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t s = (int64_t)blockIdx.x * (kBlock / kWave) + wave;
  if (s >= n_slices) return;
  const int64_t base = off[s];
  const int width = (int)((off[s + 1] - base) / (kWave * 12));
  const int *mp = slot_map + base / 12 + lane;
  double *vp = reinterpret_cast<double *>(pack + base + (int64_t)width * (kWave * 4)) + lane;
  for (int k = 0; k < width; ++k) {
    const int id = __builtin_nontemporal_load(mp + k * kWave);
    vp[k * kWave] = id < 0 ? 0.0 : p_val[id];
  }
}

// A coarse operator's fp64 records from its level's values: ext = the row sum in column order, the slots through the
// source map (the id is the entry's index; padding gets 0).
__global__ __launch_bounds__(kBlock) void amg_rf_op_kernel(char *__restrict__ pack, const int64_t *__restrict__ slice_off,
                                                           const int *__restrict__ src, int64_t n_rows, int64_t n_slices,
                                                           const int64_t *__restrict__ a_ptr, const double *__restrict__ a_val) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t s = (int64_t)blockIdx.x * (kBlock / kWave) + wave;
  if (s >= n_slices) return;
  const int64_t row = s * kWave + lane;
  const int64_t base = slice_off[s];
  const int width = (int)((slice_off[s + 1] - base - kExtBytes) / kSlotBytes);
  char *rec = pack + base;
  double ext = 0.0;
  if (row < n_rows)
    for (int64_t e = a_ptr[row]; e < a_ptr[row + 1]; ++e) ext += a_val[e];
  reinterpret_cast<double *>(rec)[lane] = ext;
  double *val = reinterpret_cast<double *>(rec + kExtBytes + (int64_t)width * (kWave * 4));
  const int *sp = src + (base - s * kExtBytes) / (kSlotBytes / kWave);
  const int np2 = width >> 1;
  for (int k = 0; k < width; ++k) {
    const int at = rf_slot_at(k, np2, lane);
    const int id = __builtin_nontemporal_load(sp + at);
    val[at] = id < 0 ? 0.0 : a_val[id];
  }
}

__global__ __launch_bounds__(kBlock) void amg_rf_tail_kernel(int64_t tail_nnz, const int *__restrict__ tail_src,
                                                             const double *__restrict__ a_val, double *__restrict__ tail_val) {
  const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (k < tail_nnz) tail_val[k] = a_val[tail_src[k]];
}

template <class T>
static int rf_upload(storm_hip_amg *h, T **dst, const T *src, size_t count) {
  const size_t nbytes = sizeof(T) * (count ? count : 1);
  hipError_t e = hipMalloc((void **)dst, nbytes);
  if (e != hipSuccess) STORM_FAIL(STORM_HIP_E_ALLOC, "amg_create_refreshable: hipMalloc(%zu) failed: %s", nbytes, hipGetErrorString(e));
  if (count && src) HIP_TRY(hipMemcpy(*dst, src, sizeof(T) * count, hipMemcpyHostToDevice));
  h->refresh_bytes += (int64_t)nbytes, h->device_bytes += (int64_t)nbytes;
  return STORM_HIP_OK;
}

template <class T>
static int rf_download(std::vector<T> *dst, const T *d_src, size_t count) {
  dst->resize(count);
  if (count) HIP_TRY(hipMemcpy(dst->data(), d_src, sizeof(T) * count, hipMemcpyDeviceToHost));
  return STORM_HIP_OK;
}

static unsigned rf_blocks(int64_t n_rows) { return (unsigned)(((n_rows + kWave - 1) / kWave + 3) / 4); }

// A_l's pattern, values, mask and diagonal positions (the position inside the row: rows are shorter than 2^31)
static int rf_upload_operator(storm_hip_amg *h, const AmgHostLevel &H, storm_hip_amg::RefreshLevel *F) {
  const AmgCsr &A = H.A;
  F->n = A.n_rows, F->nnz_a = A.nnz();
  std::vector<int> diag((size_t)A.n_rows, -1);
  for (int64_t i = 0; i < A.n_rows; ++i) {
    const auto b = A.col.begin() + A.ptr[(size_t)i], e = A.col.begin() + A.ptr[(size_t)i + 1];
    const auto it = std::lower_bound(b, e, (int)i);
    STORM_REQUIRE(it != e && *it == i, "amg_create_refreshable: row %lld of a level operator has no diagonal entry", (long long)i);
    diag[(size_t)i] = (int)(it - b);
  }
  STORM_TRY(rf_upload(h, &F->d_a_ptr, A.ptr.data(), A.ptr.size()));
  STORM_TRY(rf_upload(h, &F->d_a_col, A.col.data(), A.col.size()));
  STORM_TRY(rf_upload(h, &F->d_a_val, A.val.data(), A.val.size()));
  STORM_TRY(rf_upload(h, &F->d_a_diag, diag.data(), diag.size()));
  return STORM_HIP_OK;
}

// Level 0: for every slot of the operator's records and every entry of its CSR tail the entry of A_0 it adds to.
static int rf_level0_maps(storm_hip_amg *h, storm_hip_amg::RefreshLevel *F) {
  const storm_hip_op *op = h->op;
  const AmgCsr &A = h->hier->levels[0].A;
  const int64_t n = op->n_rows, ns = op->n_slices;
  std::vector<int64_t> off, tptr;
  std::vector<char> pack;
  std::vector<int> src, trow, tcol;
  STORM_TRY(rf_download(&off, op->d_slice_off, (size_t)ns + 1));
  STORM_TRY(rf_download(&pack, op->d_pack, (size_t)off[(size_t)ns]));
  STORM_TRY(rf_download(&src, op->d_src, (size_t)((off[(size_t)ns] - ns * kExtBytes) / (kSlotBytes / kWave))));
  STORM_TRY(rf_download(&trow, op->d_tail_row, (size_t)op->tail_rows));
  STORM_TRY(rf_download(&tptr, op->d_tail_ptr, (size_t)op->tail_rows + 1));
  STORM_TRY(rf_download(&tcol, op->d_tail_col, (size_t)op->tail_nnz));
  auto entry_of = [&](int64_t i, int c, int *out) -> bool {
    if (c == i) return *out = -2, true;  // multiplies x_i - x_i: in the diagonal's sum only
    const auto b = A.col.begin() + A.ptr[(size_t)i], e = A.col.begin() + A.ptr[(size_t)i + 1];
    const auto it = std::lower_bound(b, e, c);
    if (it == e || *it != c) return false;
    return *out = (int)(it - A.col.begin()), true;
  };
  std::vector<int> ent(src.size(), -1);
  for (int64_t s = 0; s < ns; ++s) {
    const int W = (int)((off[(size_t)s + 1] - off[(size_t)s] - kExtBytes) / kSlotBytes), np2 = W >> 1;
    const int64_t first = (off[(size_t)s] - s * kExtBytes) / (kSlotBytes / kWave);
    const int *c_ = reinterpret_cast<const int *>(pack.data() + off[(size_t)s] + kExtBytes);
    for (int l = 0; l < kWave; ++l) {
      const int64_t i = s * kWave + l;
      for (int k = 0; k < W; ++k) {
        const int at = (k < 2 * np2) ? ((k >> 1) * kWave + l) * 2 + (k & 1) : np2 * 2 * kWave + l;
        if (src[(size_t)(first + at)] < 0) continue;
        STORM_REQUIRE(i < n && entry_of(i, c_[at], &ent[(size_t)(first + at)]),
                      "amg_create_refreshable: a slot of row %lld is not in the level operator's pattern", (long long)i);
      }
    }
  }
  STORM_TRY(rf_upload(h, &F->d_slot_ent, ent.data(), ent.size()));
  if (op->tail_rows > 0) {
    std::vector<int> tail_of((size_t)n, -1), tent((size_t)op->tail_nnz, -1);
    for (int64_t t = 0; t < op->tail_rows; ++t) {
      const int64_t i = trow[(size_t)t];
      STORM_REQUIRE(i >= 0 && i < n && tptr[(size_t)t] <= tptr[(size_t)t + 1] && tptr[(size_t)t + 1] <= op->tail_nnz,
                    "amg_create_refreshable: a tail row outside the operator");
      tail_of[(size_t)i] = (int)t;
      for (int64_t k = tptr[(size_t)t]; k < tptr[(size_t)t + 1]; ++k)
        STORM_REQUIRE(entry_of(i, tcol[(size_t)k], &tent[(size_t)k]),
                      "amg_create_refreshable: a tail entry of row %lld is not in the level operator's pattern", (long long)i);
    }
    STORM_TRY(rf_upload(h, &F->d_tail_of, tail_of.data(), tail_of.size()));
    STORM_TRY(rf_upload(h, &F->d_tail_ent, tent.data(), tent.size()));
  }
  return STORM_HIP_OK;
}

static int rf_build(storm_hip_amg *h) {
  const size_t nl = h->hier->levels.size();
  h->refresh.resize(nl);
  STORM_TRY(rf_upload(h, &h->d_scalars, (const double *)nullptr, 2));
  STORM_TRY(rf_upload(h, &h->d_bad, (const int *)nullptr, 1));
  for (size_t l = 0; l < nl; ++l) {
    const AmgHostLevel &H = h->hier->levels[l];
    storm_hip_amg::RefreshLevel &F = h->refresh[l];
    STORM_TRY(rf_upload_operator(h, H, &F));
    if (l == 0) STORM_TRY(rf_level0_maps(h, &F));
    if (l + 1 == nl) break;
    AmgRefreshMaps m;
    STORM_TRY(amg_refresh_maps(*h->hier, l, &m));
    F.nnz_p = H.P.nnz(), F.nnz_ap = m.AP.nnz(), F.p_slots = (int64_t)m.p_slot.size(), F.r_slots = (int64_t)m.r_slot.size();
    STORM_TRY(rf_upload(h, &F.d_strong, H.strong.data(), H.strong.size()));
    STORM_TRY(rf_upload(h, &F.d_agg, H.agg.data(), H.agg.size()));
    STORM_TRY(rf_upload(h, &F.d_df, (const double *)nullptr, (size_t)F.n));
    STORM_TRY(rf_upload(h, &F.d_wave_max, (const double *)nullptr, (size_t)((F.n + kWave - 1) / kWave)));
    STORM_TRY(rf_upload(h, &F.d_p_ptr, H.P.ptr.data(), H.P.ptr.size()));
    STORM_TRY(rf_upload(h, &F.d_p_col, H.P.col.data(), H.P.col.size()));
    STORM_TRY(rf_upload(h, &F.d_p_val, H.P.val.data(), H.P.val.size()));
    STORM_TRY(rf_upload(h, &F.d_r_ptr, H.R.ptr.data(), H.R.ptr.size()));
    STORM_TRY(rf_upload(h, &F.d_r_col, H.R.col.data(), H.R.col.size()));
    STORM_TRY(rf_upload(h, &F.d_r_of, m.r_of.data(), m.r_of.size()));
    STORM_TRY(rf_upload(h, &F.d_ap_ptr, m.AP.ptr.data(), m.AP.ptr.size()));
    STORM_TRY(rf_upload(h, &F.d_ap_col, m.AP.col.data(), m.AP.col.size()));
    STORM_TRY(rf_upload(h, &F.d_ap_val, (const double *)nullptr, m.AP.col.size()));
    STORM_TRY(rf_upload(h, &F.d_p_slot, m.p_slot.data(), m.p_slot.size()));
    STORM_TRY(rf_upload(h, &F.d_r_slot, m.r_slot.data(), m.r_slot.size()));
    // the maps address the transfer records as amg_pack_transfer laid them out
    const storm_hip_amg::Level &L = h->levels[l];
    STORM_REQUIRE(L.P.n_slices == (F.n + kWave - 1) / kWave && L.R.n_slices == (h->hier->levels[l + 1].A.n_rows + kWave - 1) / kWave,
                  "amg_create_refreshable: the transfer records of level %d do not match their maps", (int)l);
  }
  return STORM_HIP_OK;
}

void amg_refresh_free(storm_hip_amg *h) {
  for (auto &F : h->refresh) {
    void *ps[] = {F.d_a_ptr, F.d_a_col, F.d_a_val, F.d_strong, F.d_a_diag, F.d_agg, F.d_df, F.d_wave_max, F.d_p_ptr, F.d_p_col,
                  F.d_p_val, F.d_r_ptr, F.d_r_col, F.d_r_of, F.d_ap_ptr, F.d_ap_col, F.d_ap_val, F.d_p_slot, F.d_r_slot,
                  F.d_slot_ent, F.d_tail_ent, F.d_tail_of};
    for (void *p : ps) (void)hipFree(p);
  }
  h->refresh.clear();
  (void)hipFree(h->d_scalars), (void)hipFree(h->d_bad);
  h->d_scalars = nullptr, h->d_bad = nullptr;
}

// Step 7 of the frozen-structure recipe for one level: the scale, the bound and the polynomial, in place.
static int rf_smoother(storm_hip_amg *h, size_t l) {
  storm_hip_amg::Level &L = h->levels[l];
  const storm_hip_amg_params &p = h->hier->params;
  STORM_TRY(storm_hip_op_get_diagonal(L.op, L.alpha, L.beta, 1, L.dinv));
  double lmax = 0.0;
  if (p.reduced_records) STORM_TRY(storm_hip_op_gershgorin_reduced(L.op, L.alpha, L.beta, L.dinv, &lmax));
  else STORM_TRY(storm_hip_op_gershgorin(L.op, L.alpha, L.beta, L.dinv, &lmax));
  const double lmin = lmax / p.smoother_ratio;
  storm_hip_cheb *ch = L.cheb;
  STORM_TRY(storm_hip_cheb_coefficients(lmin, lmax, ch->degree, &ch->theta, ch->c1, ch->c2));
  ch->lmin = lmin, ch->lmax = lmax, ch->inv_theta = 1.0 / ch->theta;
  return STORM_HIP_OK;
}

static int rf_run(storm_hip_amg *h) {
  storm_hip_ctx *c = h->ctx;
  const size_t nl = h->levels.size();
  const storm_hip_amg_params &p = h->hier->params;
  const dim3 block(kBlock);
  const int none = INT_MAX;
  HIP_TRY(hipMemcpyAsync(h->d_bad, &none, sizeof(int), hipMemcpyHostToDevice, c->stream));
  {  // step 1: level 0 from the operator's records
    const storm_hip_op *op = h->op;
    const storm_hip_amg::RefreshLevel &F = h->refresh[0];
    hipLaunchKernelGGL(amg_rf_decode_kernel, dim3(rf_blocks(op->n_rows)), block, 0, c->stream, op->d_pack, op->d_slice_off, F.d_slot_ent,
                       op->n_rows, op->n_slices, h->alpha, h->beta, F.d_a_ptr, F.d_a_diag, F.d_a_val, F.d_tail_of, op->d_tail_ptr,
                       op->d_tail_val, F.d_tail_ent);
    HIP_TRY(hipGetLastError());
  }
  for (size_t l = 0; l + 1 < nl; ++l) {
    const storm_hip_amg::RefreshLevel &F = h->refresh[l], &N = h->refresh[l + 1];
    const storm_hip_amg::Level &L = h->levels[l];
    const int64_t ns = (F.n + kWave - 1) / kWave;
    const dim3 grid(rf_blocks(F.n));
    // steps 2 and 3, and the first wait of the level
    hipLaunchKernelGGL(amg_rf_filter_kernel, grid, block, 0, c->stream, F.n, ns, F.d_a_ptr, F.d_a_val, F.d_strong, F.d_a_diag, F.d_df,
                       F.d_wave_max, h->d_bad);
    hipLaunchKernelGGL(amg_rf_max_kernel, dim3(1), block, 0, c->stream, F.d_wave_max, ns, h->d_scalars);
    HIP_TRY(hipGetLastError());
    double lambda = 0.0;
    int bad = none;
    HIP_TRY(hipMemcpyAsync(&lambda, h->d_scalars, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(&bad, h->d_bad, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (bad != none)
      STORM_FAIL(STORM_HIP_E_INVALID, "amg_refresh: level %d, row %d: the diagonal of the filtered matrix is zero or not finite", (int)l, bad);
    STORM_REQUIRE(std::isfinite(lambda) && lambda > 0.0, "amg_refresh: level %d: lambda_F = %g", (int)l, lambda);
    if (p.prolongator_omega != 0.0) {  // step 4 (omega = 0: P = T is not touched)
      hipLaunchKernelGGL(amg_rf_prolong_kernel, grid, block, 0, c->stream, F.n, ns, F.d_a_ptr, F.d_a_col, F.d_a_val, F.d_strong,
                         F.d_a_diag, F.d_agg, F.d_df, p.prolongator_omega / lambda, F.d_p_ptr, F.d_p_col, F.d_p_val);
      hipLaunchKernelGGL(amg_rf_transfer_kernel, dim3((unsigned)((L.P.n_slices + 3) / 4)), block, 0, c->stream, L.P.d_pack, L.P.d_off,
                         L.P.n_slices, F.d_p_slot, F.d_p_val);
      hipLaunchKernelGGL(amg_rf_transfer_kernel, dim3((unsigned)((L.R.n_slices + 3) / 4)), block, 0, c->stream, L.R.d_pack, L.R.d_off,
                         L.R.n_slices, F.d_r_slot, F.d_p_val);
    }
    // step 5
    hipLaunchKernelGGL(amg_rf_ap_kernel, grid, block, 0, c->stream, F.n, ns, F.d_a_ptr, F.d_a_col, F.d_a_val, F.d_p_ptr, F.d_p_col,
                       F.d_p_val, F.d_ap_ptr, F.d_ap_col, F.d_ap_val);
    hipLaunchKernelGGL(amg_rf_rap_kernel, dim3(rf_blocks(N.n)), block, 0, c->stream, N.n, (N.n + kWave - 1) / kWave, F.d_r_ptr, F.d_r_col,
                       F.d_r_of, F.d_p_val, F.d_ap_ptr, F.d_ap_col, F.d_ap_val, N.d_a_ptr, N.d_a_col, N.d_a_val);
    HIP_TRY(hipGetLastError());
    if (l + 2 < nl) {  // the next level's operator records
      storm_hip_op *op = h->levels[l + 1].own_op;
      hipLaunchKernelGGL(amg_rf_op_kernel, dim3(rf_blocks(op->n_rows)), block, 0, c->stream, op->d_pack, op->d_slice_off, op->d_src,
                         op->n_rows, op->n_slices, N.d_a_ptr, N.d_a_val);
      if (op->tail_nnz > 0)
        hipLaunchKernelGGL(amg_rf_tail_kernel, dim3((unsigned)((op->tail_nnz + kBlock - 1) / kBlock)), block, 0, c->stream, op->tail_nnz,
                           op->d_tail_src, N.d_a_val, op->d_tail_val);
      HIP_TRY(hipGetLastError());
      if (op->d_pack32 != nullptr) STORM_TRY(op_reduced_convert(op, nullptr));
    }
  }
  {  // step 6: the coarsest level's round trip
    AmgCsr Ac = h->hier->levels[nl - 1].A;
    HIP_TRY(hipMemcpyAsync(Ac.val.data(), h->refresh[nl - 1].d_a_val, sizeof(double) * Ac.val.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (double v : Ac.val)
      if (!std::isfinite(v)) STORM_FAIL(STORM_HIP_E_INVALID, "amg_refresh: level %d (the coarsest) has a non-finite entry", (int)nl - 1);
    std::vector<double> inv;
    if (h->hier->nullspace) STORM_TRY(amg_coarse_nullspace(Ac, &inv, &h->hier->coarse_shift));  // N3 (N1 and N2 are the build's)
    else STORM_TRY(amg_dense_inverse(Ac, &inv));
    HIP_TRY(hipMemcpyAsync(h->d_ainv, inv.data(), sizeof(double) * inv.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));  // (inv leaves scope)
  }
  for (size_t l = 0; l + 1 < nl; ++l) STORM_TRY(rf_smoother(h, l));  // step 7
  return STORM_HIP_OK;
}

// The weights of transfer records back into the CSR they were packed from.
static int rf_download_transfer(const storm_hip_amg::Transfer &T, AmgCsr *M) {
  std::vector<int64_t> off;
  std::vector<char> pack;
  STORM_TRY(rf_download(&off, T.d_off, (size_t)T.n_slices + 1));
  STORM_TRY(rf_download(&pack, T.d_pack, (size_t)off[(size_t)T.n_slices]));
  STORM_REQUIRE(T.n_rows == M->n_rows, "amg_download: transfer records of %lld rows for %lld", (long long)T.n_rows, (long long)M->n_rows);
  for (int64_t i = 0; i < M->n_rows; ++i) {
    const int64_t s = i / kWave, lane = i % kWave;
    const int64_t w = (off[(size_t)s + 1] - off[(size_t)s]) / (kWave * 12);
    const int *cp = reinterpret_cast<const int *>(pack.data() + off[(size_t)s]);
    const double *vp = reinterpret_cast<const double *>(pack.data() + off[(size_t)s] + w * kWave * 4);
    STORM_REQUIRE(M->ptr[(size_t)i + 1] - M->ptr[(size_t)i] <= w, "amg_download: row %lld is wider than its slice", (long long)i);
    for (int64_t k = M->ptr[(size_t)i], q = 0; k < M->ptr[(size_t)i + 1]; ++k, ++q) {
      STORM_REQUIRE(cp[q * kWave + lane] == M->col[(size_t)k], "amg_download: the transfer records of row %lld left their pattern", (long long)i);
      M->val[(size_t)k] = vp[q * kWave + lane];
    }
  }
  return STORM_HIP_OK;
}

}  // namespace storm

using namespace storm;

extern "C" {

int storm_hip_amg_create_refreshable(storm_hip_op *op, double alpha, double beta, const storm_hip_amg_params *params, storm_hip_amg **out) {
  STORM_REQUIRE(op && out, "amg_create_refreshable: null argument");
  *out = nullptr;
  if (!op->updatable)
    STORM_FAIL(STORM_HIP_E_UNSUPPORTED, "amg_create_refreshable: the operator (%lld rows) was not created by "
                                        "storm_hip_op_create_from_face_weights_updatable (its source map says which slots are real)",
               (long long)op->n_rows);
  STORM_TRY(amg_create_checks(op, alpha, beta, "amg_create_refreshable"));
  STORM_REQUIRE(op->pack_bytes < ((int64_t)1 << 33), "amg_create_refreshable: %lld bytes of records exceed the int32 slot maps", (long long)op->pack_bytes);
  storm_hip_ctx *c = op->ctx;
  HIP_TRY(hipSetDevice(c->device));
  STORM_TRY(lazy_sync(c));
  std::vector<int64_t> ptr, col;
  std::vector<double> val;
  STORM_TRY(amg_decode(op, alpha, beta, true, &ptr, &col, &val));
  storm_hip_amg_hierarchy *hier = nullptr;
  STORM_TRY(storm_hip_amg_setup_csr_structural(op->n_rows, ptr.data(), col.data(), val.data(), params, &hier));
  storm_hip_amg *h = new storm_hip_amg();
  h->ctx = c, h->op = op, h->alpha = alpha, h->beta = beta, h->hier = hier;
  const auto t0 = std::chrono::steady_clock::now();
  int st = amg_build_device(h, op);
  if (st == STORM_HIP_OK) st = rf_build(h);
  if (st != STORM_HIP_OK) {
    (void)storm_hip_amg_destroy(h);
    return st;
  }
  h->upload_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  *out = h;
  return STORM_HIP_OK;
}

int storm_hip_amg_create_nullspace(storm_hip_op *op, double alpha, double beta, const storm_hip_amg_params *params, int refreshable,
                                   storm_hip_amg **out) {
  STORM_REQUIRE(op && out, "amg_create_nullspace: null argument");
  *out = nullptr;
  const bool rf = refreshable != 0;
  if (rf && !op->updatable)
    STORM_FAIL(STORM_HIP_E_UNSUPPORTED, "amg_create_nullspace: refreshable, but the operator (%lld rows) was not created by "
                                        "storm_hip_op_create_from_face_weights_updatable (its source map says which slots are real)",
               (long long)op->n_rows);
  STORM_TRY(amg_create_checks(op, alpha, beta, "amg_create_nullspace"));
  if (rf)
    STORM_REQUIRE(op->pack_bytes < ((int64_t)1 << 33), "amg_create_nullspace: %lld bytes of records exceed the int32 slot maps", (long long)op->pack_bytes);
  storm_hip_ctx *c = op->ctx;
  HIP_TRY(hipSetDevice(c->device));
  STORM_TRY(lazy_sync(c));
  std::vector<int64_t> ptr, col;
  std::vector<double> val;
  STORM_TRY(amg_decode(op, alpha, beta, rf, &ptr, &col, &val));
  storm_hip_amg_hierarchy *hier = nullptr;
  STORM_TRY(storm_hip_amg_setup_csr_nullspace(op->n_rows, ptr.data(), col.data(), val.data(), params, rf ? 1 : 0, &hier));
  storm_hip_amg *h = new storm_hip_amg();
  h->ctx = c, h->op = op, h->alpha = alpha, h->beta = beta, h->hier = hier;
  const auto t0 = std::chrono::steady_clock::now();
  int st = amg_build_device(h, op);
  if (st == STORM_HIP_OK && rf) st = rf_build(h);
  if (st != STORM_HIP_OK) {
    (void)storm_hip_amg_destroy(h);
    return st;
  }
  h->upload_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  *out = h;
  return STORM_HIP_OK;
}

int storm_hip_amg_refresh(storm_hip_amg *h) {
  STORM_REQUIRE(h, "amg_refresh: null argument");
  if (h->refresh.empty())
    STORM_FAIL(STORM_HIP_E_UNSUPPORTED, "amg_refresh: the object was not created by storm_hip_amg_create_refreshable (its hierarchy "
                                        "has no frozen structure on the device)");
  storm_hip_ctx *c = h->ctx;
  HIP_TRY(hipSetDevice(c->device));
  STORM_TRY(lazy_sync(c));
  h->invalid = 1;  // until every step is through
  amg_tail_invalidate(h);  // (the smoothers' coefficients move: the tail kernel's tables are built again)
  STORM_TRY(rf_run(h));
  h->invalid = 0;
  ++c->n_amg_refreshes;
  return STORM_HIP_OK;
}

int storm_hip_amg_download(storm_hip_amg *h) {
  STORM_REQUIRE(h, "amg_download: null argument");
  if (h->refresh.empty()) return STORM_HIP_OK;  // a plain object's host hierarchy is what was uploaded
  storm_hip_ctx *c = h->ctx;
  HIP_TRY(hipSetDevice(c->device));
  STORM_TRY(lazy_sync(c));
  HIP_TRY(hipStreamSynchronize(c->stream));
  const size_t nl = h->levels.size();
  for (size_t l = 0; l + 1 < nl; ++l) {  // what the cycle reads: the level operators' records, the transfer records
    AmgHostLevel &H = h->hier->levels[l];
    const storm_hip_amg::Level &L = h->levels[l];
    std::vector<int64_t> ptr, col;
    std::vector<double> val;
    STORM_TRY(amg_decode(L.op, L.alpha, L.beta, true, &ptr, &col, &val));
    STORM_REQUIRE(ptr == H.A.ptr && col.size() == H.A.col.size() && std::equal(col.begin(), col.end(), H.A.col.begin()),
                  "amg_download: the records of level %d left the frozen pattern", (int)l);
    H.A.val = std::move(val);
    STORM_TRY(rf_download_transfer(L.P, &H.P));
    STORM_TRY(rf_download_transfer(L.R, &H.R));
  }
  // the coarsest level has no records: its values as the last refresh left them, and the inverse the cycle multiplies by
  STORM_TRY(rf_download(&h->hier->levels[nl - 1].A.val, h->refresh[nl - 1].d_a_val, h->hier->levels[nl - 1].A.val.size()));
  STORM_TRY(rf_download(&h->hier->ainv, h->d_ainv, h->hier->ainv.size()));
  return STORM_HIP_OK;
}

}  // extern "C"
