// Operator apply on a block vector: K interleaved columns over the operator's rows, element (i, j) at x[i K + j] -- the
// layout of the reference's Field<Mesh, Index, Value, NumVars> (Feathers/Field.hpp:56-79: every cell stores a
// Vec<Value, NumVars>).  fp64 sliced-ELL records (format 0, with or without a CSR tail); record layout: the header of
// spmv.hip.  The records -- 96 of the 112 B/row a single apply moves -- are streamed ONCE for the K columns, and one
// 16-byte gather fetches a neighbour's value for two columns from one cache line.
//
// spmv_block_kernel keeps spmv_sell_kernel's shape: one wavefront per slice, one row per lane, the same XCD remap,
// records (and, for K = 1, y) non-temporal under option nontemporal.  The arithmetic per column is sell_device.hpp's, the functions
// spmv_sell_kernel itself calls: Y_j is, bit for bit, what storm_hip_op_apply gives for column j.
#include "sell_device.hpp"

namespace storm {

struct BlockDotArgs {
  double *partials;  // [K][n_waves]: per-wave partials of <X_j, Y_j>
  int n_waves;
};

template <int K, bool NT>
__device__ __forceinline__ void st_cols(double *__restrict__ y, int64_t row, const double (&v)[K]) {
  if constexpr (K % 2 == 0) {
    double2v *p = reinterpret_cast<double2v *>(y + row * K);
#pragma unroll
    for (int q = 0; q < K / 2; ++q) {
      const double2v t = {v[2 * q], v[2 * q + 1]};
      if (NT) __builtin_nontemporal_store(t, p + q);
      else p[q] = t;
    }
  } else {
#pragma unroll
    for (int j = 0; j < K; ++j) {
      if (NT) __builtin_nontemporal_store(v[j], y + row * K + j);
      else y[row * K + j] = v[j];
    }
  }
}

//   NT  : record traffic (K = 1: and y) marked non-temporal so it does not evict x from L2.
//   DOT : epilogue writes per-wave partials of <X_j, Y_j> for every column (64-lane DPP tree, lane 63 stores: no LDS).
template <bool NT, bool DOT, int K>
__global__ __launch_bounds__(kBlock) void spmv_block_kernel(SellArgs A, double alpha, double beta,
                                                            const double *__restrict__ x, double *__restrict__ y,
                                                            int64_t n_launch_slices, BlockDotArgs dot, const int *done) {
  const int done_flag = done ? *done : 0;
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int bidx = (int)blockIdx.x;
  const int lb = A.xcd_group != 0 ? (A.xcd_group > 1 ? xcd_remap_grouped(bidx, gridDim.x, A.xcd_group) : xcd_remap(bidx, gridDim.x))
                                  : bidx;
  const int64_t slice = (int64_t)lb * (kBlock / kWave) + wave;
  double xi[K], yi[K];
#pragma unroll
  for (int j = 0; j < K; ++j) xi[j] = 0.0, yi[j] = 0.0;
  if (slice < n_launch_slices) {
    const int64_t row = slice * kWave + lane;
    const bool valid = row < A.n_rows;
    if (valid) ld_cols<K>(x, (int)row, xi);
    int64_t base;
    int width;
    if (A.uniform_width > 0) {
      width = A.uniform_width;
      base = slice * (int64_t)(kExtBytes + kSlotBytes * width);
    } else {
      base = A.slice_off[slice];
      width = (int)((A.slice_off[slice + 1] - base - kExtBytes) / kSlotBytes);
    }
    const char *rec = A.pack + base;
    const double ext = ld_d<NT>(reinterpret_cast<const double *>(rec) + lane);
    double acc[K];
    row_sum_any<NT, K>(rec, width, lane, x, xi, acc);
#pragma unroll
    for (int j = 0; j < K; ++j) yi[j] = sell_row_result(false, 0.0, beta, xi[j], alpha, acc[j], ext);
    // (y non-temporal only where a wave's store is contiguous, K = 1: with K > 1 a lane owns a whole cell and one store
    //  instruction writes 16 B out of every 8 K -- non-temporal, such partial lines cost 1.3x (K = 4) to 1.8x (K = 8) of
    //  the kernel, profiles/r16_block_nt_ab.json; plain, the L2 merges them before they leave)
    if (valid && !done_flag) st_cols<K, NT && K == 1>(y, row, yi);
    if (!valid) {
#pragma unroll
      for (int j = 0; j < K; ++j) yi[j] = 0.0;
    }
  }
  if (done_flag) return;  // block-uniform
  if (DOT) {
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const double a = wave_sum_to_lane63(xi[j] * yi[j]);
      if (lane == kWave - 1) dot.partials[(int64_t)j * dot.n_waves + (int)blockIdx.x * (kBlock / kWave) + wave] = a;
    }
  }
}

// CSR tail: one wavefront per overflowing row, the columns in turn (tail_row_add: spmv_tail_kernel's own statements).
__global__ __launch_bounds__(kBlock) void spmv_block_tail_kernel(int64_t n_tail, const int *__restrict__ tail_row,
                                                                 const int64_t *__restrict__ tail_ptr,
                                                                 const int *__restrict__ tail_col,
                                                                 const double *__restrict__ tail_val, double alpha, int k,
                                                                 const double *__restrict__ x, double *__restrict__ y,
                                                                 const int *done) {
  if (done && *done) return;
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t t = (int64_t)blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6);
  if (t >= n_tail) return;
  const int r = tail_row[t];
  for (int j = 0; j < k; ++j) tail_row_add(t, r, lane, tail_ptr, tail_col, tail_val, alpha, x, y, k, j);
}

template <bool NT, bool DOT>
static void launch_block(const storm_hip_op *op, int nb, int k, double alpha, double beta, const double *x, double *y,
                         BlockDotArgs dot, const int *done) {
  SellArgs A{op->d_pack, op->d_slice_off, op->n_rows, op->uniform_width, op->xcd_group_sell, nullptr, 0, nullptr, 0, 0};
  hipStream_t st = op->ctx->stream;
#define BLOCK_GO(K_) \
  hipLaunchKernelGGL((spmv_block_kernel<NT, DOT, K_>), dim3(nb), dim3(kBlock), 0, st, A, alpha, beta, x, y, op->n_slices, dot, done)
  STORM_K_SWITCH(k, BLOCK_GO)
#undef BLOCK_GO
}

int spmv_block_check(const storm_hip_op *op, int k, const storm_hip_vec *X, const storm_hip_vec *Y, const char *what) {
  STORM_REQUIRE(op && X && Y, "%s: null argument", what);
  STORM_REQUIRE(X->ctx == op->ctx && Y->ctx == op->ctx, "%s: context mismatch", what);
  STORM_REQUIRE(k >= 1 && k <= 8, "%s: k = %d outside [1, 8]", what, k);
  STORM_REQUIRE(X != Y && X->d != Y->d, "%s: X and Y must not alias", what);
  STORM_REQUIRE(X->n_owned == op->n_rows * k && Y->n_owned == op->n_rows * k,
                "%s: operator has %lld rows: a block of %d columns holds %lld elements, X has %lld, Y %lld", what,
                (long long)op->n_rows, k, (long long)(op->n_rows * k), (long long)X->n_owned, (long long)Y->n_owned);
  if (op->halo.n_nbrs > 0 || op->n_halo > 0 || op->ctx->comm != nullptr)
    STORM_FAIL(STORM_HIP_E_UNSUPPORTED, "%s: block vectors are single-rank (the operator has a halo plan or halo columns, "
                                        "or the context a communicator)", what);
  if (op->dict_size > 0 || op->offs_size > 0 || op->pair != 0)
    STORM_FAIL(STORM_HIP_E_UNSUPPORTED, "%s: block vectors need fp64 records; this operator was built in a compact record "
                                        "format -- build it with option spmv_dict = 0", what);
  return STORM_HIP_OK;
}

int spmv_block_launch(const storm_hip_op *op, double alpha, double beta, int k, const double *X, double *Y,
                      double *pz_partials, int *n_partials, const int *done) {
  storm_hip_ctx *c = op->ctx;
  if (n_partials) *n_partials = 0;
  if (op->n_rows == 0) return STORM_HIP_OK;
  const int nb = (int)((op->n_slices + (kBlock / kWave) - 1) / (kBlock / kWave));
  const bool want_dot = pz_partials != nullptr && op->tail_rows == 0;
  const BlockDotArgs dot{want_dot ? pz_partials : nullptr, (kBlock / kWave) * nb};
  if (want_dot && n_partials) *n_partials = dot.n_waves;
  const bool nt = c->opt_nt != 0;
  if (nt) {
    if (want_dot) launch_block<true, true>(op, nb, k, alpha, beta, X, Y, dot, done);
    else launch_block<true, false>(op, nb, k, alpha, beta, X, Y, dot, done);
  } else {
    if (want_dot) launch_block<false, true>(op, nb, k, alpha, beta, X, Y, dot, done);
    else launch_block<false, false>(op, nb, k, alpha, beta, X, Y, dot, done);
  }
  HIP_TRY(hipGetLastError());
  if (op->tail_rows > 0) {
    const int nbt = (int)((op->tail_rows + 3) / 4);
    hipLaunchKernelGGL(spmv_block_tail_kernel, dim3(nbt), dim3(kBlock), 0, c->stream, op->tail_rows, op->d_tail_row,
                       op->d_tail_ptr, op->d_tail_col, op->d_tail_val, alpha, k, X, Y, done);
    HIP_TRY(hipGetLastError());
  }
  return STORM_HIP_OK;
}

}  // namespace storm
