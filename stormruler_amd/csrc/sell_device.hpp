// The row arithmetic of the sliced-ELL records, shared by spmv_sell.hip (one column), spmv_block.hip (a block of
// K interleaved columns, element (i, j) at x[i K + j]), precond_cheb.hip and op_reduced.hip (the fp32-weight companion
// records, through the record policy below): ONE definition of every statement that rounds, so that the two
// kernels contract the same products into the same additions and a block apply gives, column by column, the bits of
// the single apply (tests/test_gpu_block.py).  Record layout: the header of spmv.hip.
#pragma once
#include "spmv_device.hpp"

namespace storm {

// The K values of cell `col`.  K even: 16-byte loads (a block vector starts on a 16-byte boundary and a cell is K * 8 bytes).
// CO (one column only): x is written by other blocks of the SAME launch (amg_tail.hip) -- co_load's access (coop_device.hpp),
// a relaxed agent-scope atomic load; the value, hence everything summed from it, is the plain load's.
// X: the gathered vector's element type -- double, or float (mixed_cg.hip: one column, plain gathers), widened exactly
// where it is loaded.
template <int K, bool CO = false, class X = double>
__device__ __forceinline__ void ld_cols(const X *__restrict__ x, int col, double (&out)[K]) {
  static_assert(!CO || K == 1, "ld_cols: coherent gathers take one column");
  static_assert(std::is_same<X, double>::value || (K == 1 && !CO), "ld_cols: an fp32 vector is one column, gathered plainly");
  if constexpr (!std::is_same<X, double>::value) {
    out[0] = (double)x[col];
  } else if constexpr (CO) {
    out[0] = __hip_atomic_load(x + col, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  } else if constexpr (K == 1) {
    out[0] = x[col];
  } else if constexpr (K % 2 == 0) {
    const double2v *p = reinterpret_cast<const double2v *>(x + (int64_t)col * K);
#pragma unroll
    for (int q = 0; q < K / 2; ++q) {
      const double2v v = p[q];
      out[2 * q] = v.x, out[2 * q + 1] = v.y;
    }
  } else {
    const double *p = x + (int64_t)col * K;
#pragma unroll
    for (int j = 0; j < K; ++j) out[j] = p[j];
  }
}

// How the (col, w) of a row's slots are loaded -- the record policy of row_sum_block and everything above it.  The
// accumulation below the loads is the same statement for every policy.
//   Rec64  the fp64 records (header of spmv.hip): pairs read as int2 / double2, an odd last slot unpaired.
//   Rec32  the fp32-weight companion (op_reduced.hip): [ext 64 x f32][pairs (W/2) x 64 x {int col0, col1, float w0, w1}]
//          [odd last slot 64 x {int col, float w}] -- one 16-byte load per lane and slot pair; a weight is widened to double
//          (exactly) where it is loaded.
struct Rec64 {
  static constexpr int kExt = kExtBytes, kSlot = kSlotBytes;
  template <bool NT>
  static __device__ __forceinline__ double ext(const char *rec, int lane) {
    return ld_d<NT>(reinterpret_cast<const double *>(rec) + lane);
  }
  template <bool NT, int W>
  static __device__ __forceinline__ void load(const char *rec, int width, int lane, int s0, int (&col)[W > 0 ? W : 1],
                                              double (&w)[W > 0 ? W : 1]) {
    constexpr int NP = W / 2;
    const int npair_total = width >> 1;
    const int2v *cp2 = reinterpret_cast<const int2v *>(rec + kExtBytes) + lane + (s0 >> 1) * kWave;
    const char *vbase = rec + kExtBytes + (int64_t)width * (kWave * 4);
    const double2v *vp2 = reinterpret_cast<const double2v *>(vbase) + lane + (s0 >> 1) * kWave;
    int2v c[NP > 0 ? NP : 1];
    double2v v[NP > 0 ? NP : 1];
    int ct = 0;
    double vt = 0.0;
#pragma unroll
    for (int q = 0; q < NP; ++q) {
      c[q] = NT ? __builtin_nontemporal_load(cp2 + q * kWave) : cp2[q * kWave];
      v[q] = NT ? __builtin_nontemporal_load(vp2 + q * kWave) : vp2[q * kWave];
    }
    if (W & 1) {  // the slice's unpaired last slot
      ct = ld_i<NT>(reinterpret_cast<const int *>(rec + kExtBytes + (int64_t)npair_total * (kWave * 8)) + lane);
      vt = ld_d<NT>(reinterpret_cast<const double *>(vbase + (int64_t)npair_total * (kWave * 16)) + lane);
    }
#pragma unroll
    for (int q = 0; q < NP; ++q) {
      col[2 * q] = c[q].x, col[2 * q + 1] = c[q].y;
      w[2 * q] = v[q].x, w[2 * q + 1] = v[q].y;
    }
    if (W & 1) col[W - 1] = ct, w[W - 1] = vt;
  }
};

typedef int int4v __attribute__((ext_vector_type(4)));
struct Rec32 {
  static constexpr int kExt = kExt32Bytes, kSlot = kSlot32Bytes;
  template <bool NT>
  static __device__ __forceinline__ double ext(const char *rec, int lane) {
    const float *p = reinterpret_cast<const float *>(rec) + lane;
    return (double)(NT ? __builtin_nontemporal_load(p) : *p);
  }
  template <bool NT, int W>
  static __device__ __forceinline__ void load(const char *rec, int width, int lane, int s0, int (&col)[W > 0 ? W : 1],
                                              double (&w)[W > 0 ? W : 1]) {
    constexpr int NP = W / 2;
    const int npair_total = width >> 1;
    const int4v *pp = reinterpret_cast<const int4v *>(rec + kExt32Bytes) + lane + (s0 >> 1) * kWave;
    int4v c[NP > 0 ? NP : 1];
    int2v ct = {0, 0};
#pragma unroll
    for (int q = 0; q < NP; ++q) c[q] = NT ? __builtin_nontemporal_load(pp + q * kWave) : pp[q * kWave];
    if (W & 1) {  // the slice's unpaired last slot
      const int2v *tp = reinterpret_cast<const int2v *>(rec + kExt32Bytes + (int64_t)npair_total * (kWave * 16)) + lane;
      ct = NT ? __builtin_nontemporal_load(tp) : *tp;
    }
#pragma unroll
    for (int q = 0; q < NP; ++q) {
      col[2 * q] = c[q].x, col[2 * q + 1] = c[q].y;
      w[2 * q] = (double)__int_as_float(c[q].z), w[2 * q + 1] = (double)__int_as_float(c[q].w);
    }
    if (W & 1) col[W - 1] = ct.x, w[W - 1] = (double)__int_as_float(ct.y);
  }
};

// acc[j] = sum_k w_k (x_j[col_k] - xi[j]) over slots [S0, S0 + W) of a record whose slice has `width` slots
// (W compile-time, S0 even).  The (col, val) record is loaded once for all columns (by the record policy R); the
// neighbours' values are gathered kGather slots at a time (every slot at once up to
// K = 4: at most 32 doubles in flight per lane), the sums run over the slots in order whatever the chunking.
template <bool NT, int W, int K, class R = Rec64, bool CO = false, class X = double>
__device__ __forceinline__ void row_sum_block(const char *rec, int width, int lane, const X *__restrict__ x,
                                              const double (&xi)[K], double (&acc)[K], int s0 = 0) {
  constexpr int W1 = W > 0 ? W : 1;
  constexpr int kGather = K <= 4 ? W1 : 4;
  int col[W1];
  double w[W1];
  R::template load<NT, W>(rec, width, lane, s0, col, w);
#pragma unroll
  for (int j = 0; j < K; ++j) acc[j] = 0.0;
#pragma unroll
  for (int g0 = 0; g0 < W; g0 += kGather) {
    double xg[kGather][K];
#pragma unroll
    for (int s = 0; s < kGather; ++s)
      if (g0 + s < W) ld_cols<K, CO, X>(x, col[g0 + s], xg[s]);
#pragma unroll
    for (int s = 0; s < kGather; ++s) {
      if (g0 + s < W) {
#pragma unroll
        for (int j = 0; j < K; ++j) acc[j] += w[g0 + s] * (xg[s][j] - xi[j]);
      }
    }
  }
}

// Rows wider than 8 slots: chunk sums of 8, then the remainder.
template <bool NT, int K, class R = Rec64, bool CO = false, class X = double>
__device__ __forceinline__ void row_sum_wide_block(const char *rec, int width, int lane, const X *__restrict__ x,
                                                   const double (&xi)[K], double (&acc)[K]) {
  double part[K];
#pragma unroll
  for (int j = 0; j < K; ++j) acc[j] = 0.0, part[j] = 0.0;
  int s0 = 0;
  for (; s0 + 8 <= width; s0 += 8) {
    row_sum_block<NT, 8, K, R, CO, X>(rec, width, lane, x, xi, part, s0);
#pragma unroll
    for (int j = 0; j < K; ++j) acc[j] += part[j];
  }
  switch (width - s0) {
    case 1: row_sum_block<NT, 1, K, R, CO, X>(rec, width, lane, x, xi, part, s0); break;
    case 2: row_sum_block<NT, 2, K, R, CO, X>(rec, width, lane, x, xi, part, s0); break;
    case 3: row_sum_block<NT, 3, K, R, CO, X>(rec, width, lane, x, xi, part, s0); break;
    case 4: row_sum_block<NT, 4, K, R, CO, X>(rec, width, lane, x, xi, part, s0); break;
    case 5: row_sum_block<NT, 5, K, R, CO, X>(rec, width, lane, x, xi, part, s0); break;
    case 6: row_sum_block<NT, 6, K, R, CO, X>(rec, width, lane, x, xi, part, s0); break;
    case 7: row_sum_block<NT, 7, K, R, CO, X>(rec, width, lane, x, xi, part, s0); break;
    default: return;
  }
#pragma unroll
  for (int j = 0; j < K; ++j) acc[j] += part[j];
}

// The row's sum for a slice of `width` slots.  The width is wave-uniform: dispatch to a body with the width as a
// compile-time constant, so all (col, val) loads of the row are issued back to back, then the gathers, then the FMAs --
// no branch (and no s_waitcnt) between the gathers of one row.
template <bool NT, int K, class R = Rec64, bool CO = false, class X = double>
__device__ __forceinline__ void row_sum_any(const char *rec, int width, int lane, const X *__restrict__ x,
                                            const double (&xi)[K], double (&acc)[K]) {
  switch (width) {
    case 0:
#pragma unroll
      for (int j = 0; j < K; ++j) acc[j] = 0.0;
      break;
    case 1: row_sum_block<NT, 1, K, R, CO, X>(rec, 1, lane, x, xi, acc); break;
    case 2: row_sum_block<NT, 2, K, R, CO, X>(rec, 2, lane, x, xi, acc); break;
    case 3: row_sum_block<NT, 3, K, R, CO, X>(rec, 3, lane, x, xi, acc); break;
    case 4: row_sum_block<NT, 4, K, R, CO, X>(rec, 4, lane, x, xi, acc); break;
    case 5: row_sum_block<NT, 5, K, R, CO, X>(rec, 5, lane, x, xi, acc); break;
    case 6: row_sum_block<NT, 6, K, R, CO, X>(rec, 6, lane, x, xi, acc); break;
    case 7: row_sum_block<NT, 7, K, R, CO, X>(rec, 7, lane, x, xi, acc); break;
    case 8: row_sum_block<NT, 8, K, R, CO, X>(rec, 8, lane, x, xi, acc); break;
    default: row_sum_wide_block<NT, K, R, CO, X>(rec, width, lane, x, xi, acc); break;
  }
}

// y_i = beta x_i + alpha (acc + ext_i x_i) -- or, accumulating (stormDivGrad's own form), y_i + alpha (...): beta x_i is
// rounded on its own, then the two FMAs this expression contracts to.
__device__ __forceinline__ double sell_row_result(bool accumulate, double y_old, double beta, double xi, double alpha,
                                                  double acc, double ext) {
  return (accumulate ? y_old : beta * xi) + alpha * (acc + ext * xi);
}

// CSR tail, one wavefront per overflowing row t (row r): the lanes' partial products are folded with the __shfl_down
// tree and lane 0 adds the row's remainder to y.  `stride`, j: column j of a block of `stride` columns (1, 0: a vector).
template <class V>  // the tail's value type: double, or float of the fp32-weight companion (widened exactly)
__device__ __forceinline__ void tail_row_add(int64_t t, int r, int lane, const int64_t *__restrict__ tail_ptr,
                                             const int *__restrict__ tail_col, const V *__restrict__ tail_val,
                                             double alpha, const double *__restrict__ x, double *__restrict__ y,
                                             int64_t stride, int j) {
  const double xi = x[r * stride + j];
  double acc = 0.0;
  for (int64_t k = tail_ptr[t] + lane; k < tail_ptr[t + 1]; k += kWave)
    acc += (double)tail_val[k] * (x[tail_col[k] * stride + j] - xi);
  acc = wave_sum_down(acc);
  if (lane == 0) y[r * stride + j] += alpha * acc;
}

}  // namespace storm
