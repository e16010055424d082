// The fp32-weight companion of an operator on fp64 records (storm_hip_op_build_reduced and the *_reduced entry points):
// a second copy of the ELL records and of the CSR tail's values whose weights and ext are rounded to fp32 (IEEE round to
// nearest even) and widened back, exactly, where a kernel loads them.  Everything else -- vectors, sums, the order and
// the contraction of every operation -- is the fp64 kernels': the row arithmetic is the one definition of sell_device.hpp,
// instantiated with the record policy Rec32.  So an apply here has the bits of storm_hip_op_apply on an fp64-record
// operator built from double(float(w)), double(float(ext)) (tests/test_gpu_reduced.py).
//
// Record of a slice of width W (the fp64 record's width), 256 + 512 W bytes:
//     [ ext : 64 x f32 ][ pairs : (W / 2) x 64 x { i32 col0, i32 col1, f32 w0, f32 w1 } ][ odd last slot : 64 x { i32 col, f32 w } ]
// lane-major inside a pair block: a lane's two slots are ONE 16-byte load (1 KiB per wave instruction), so a row costs
// W / 2 + 1 record loads where the fp64 layout needs W + 1.  The companion has its own slice offsets (none with a uniform
// width); the tail shares tail_row / tail_ptr / tail_col and has float tail_val32[tail_nnz].
// Only the entry points of this file, the Chebyshev preconditioner's reduced object (precond_cheb.hip) and the refresh
// (op_update.hip) read it: no dispatch of spmv.hip knows it.
#include <cfloat>

#include "sell_device.hpp"

namespace storm {

// fp32's normal range: a nonzero weight outside it (or not finite) has no faithful fp32 image.
__device__ __forceinline__ int reduce_weight(double w, int &bad) {
  const double a = fabs(w);
  if (a != 0.0 && !(a >= (double)FLT_MIN && a <= (double)FLT_MAX)) bad = 1;  // (a NaN compares unequal to 0: flagged)
  return __float_as_int((float)w);
}

// Byte offsets of the companion's records from those of the fp64 records: the same widths, other sizes.
__global__ __launch_bounds__(kBlock) void op_reduce_offsets_kernel(int64_t n_slices, const int64_t *__restrict__ slice_off,
                                                                   int64_t *__restrict__ slice_off32) {
  const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (s > n_slices) return;
  const int64_t slots = (slice_off[s] - s * kExtBytes) / kSlotBytes;  // of the slices before this one
  slice_off32[s] = s * kExt32Bytes + slots * kSlot32Bytes;
}

// One wavefront per slice, four per block (op_refresh_sell_kernel's grid): a lane converts its own row -- ext, then per
// slot pair one int2 of columns and one double2 of weights in, one 16-byte word out.
__global__ __launch_bounds__(kBlock) void op_reduce_sell_kernel(const char *__restrict__ pack, const int64_t *__restrict__ slice_off,
                                                                char *__restrict__ pack32, const int64_t *__restrict__ slice_off32,
                                                                int uniform_width, int64_t n_slices, int *flag) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t s = (int64_t)blockIdx.x * (kBlock / kWave) + wave;
  if (s >= n_slices) return;
  const int64_t base = slice_off[s];
  const int width = (int)((slice_off[s + 1] - base - kExtBytes) / kSlotBytes);
  const char *rec = pack + base;
  char *out = pack32 + (uniform_width > 0 ? s * (int64_t)(kExt32Bytes + kSlot32Bytes * uniform_width) : slice_off32[s]);
  int bad = 0;
  reinterpret_cast<int *>(out)[lane] = reduce_weight(reinterpret_cast<const double *>(rec)[lane], bad);
  const int np2 = width >> 1;
  const int2v *cp = reinterpret_cast<const int2v *>(rec + kExtBytes) + lane;
  const char *vbase = rec + kExtBytes + (int64_t)width * (kWave * 4);
  const double2v *vp = reinterpret_cast<const double2v *>(vbase) + lane;
  int4v *op4 = reinterpret_cast<int4v *>(out + kExt32Bytes) + lane;
#pragma unroll 4
  for (int p = 0; p < np2; ++p) {
    const int2v c = cp[p * kWave];
    const double2v v = vp[p * kWave];
    int4v o;
    o.x = c.x, o.y = c.y, o.z = reduce_weight(v.x, bad), o.w = reduce_weight(v.y, bad);
    op4[p * kWave] = o;
  }
  if (width & 1) {  // the odd last slot, column-major behind the pairs
    int2v o;
    o.x = reinterpret_cast<const int *>(rec + kExtBytes + (int64_t)np2 * (kWave * 8))[lane];
    o.y = reduce_weight(reinterpret_cast<const double *>(vbase + (int64_t)np2 * (kWave * 16))[lane], bad);
    reinterpret_cast<int2v *>(out + kExt32Bytes + (int64_t)np2 * (kWave * 16))[lane] = o;
  }
  if (flag != nullptr && bad) atomicOr(flag, 1);
}

// One thread per entry of the CSR tail.
__global__ __launch_bounds__(kBlock) void op_reduce_tail_kernel(int64_t tail_nnz, const double *__restrict__ tail_val,
                                                                float *__restrict__ tail_val32, int *flag) {
  const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (k >= tail_nnz) return;
  int bad = 0;
  tail_val32[k] = __int_as_float(reduce_weight(tail_val[k], bad));
  if (flag != nullptr && bad) atomicOr(flag, 1);
}

// spmv_sell_kernel's shape on the companion records (one wavefront per slice, one row per lane, the same XCD runs, records
// and y non-temporal, x read plainly); no fused dot, no accumulate form, no slice list.
template <bool NT, bool XCD>
__global__ __launch_bounds__(kBlock) void spmv_sell32_kernel(SellArgs A, double alpha, double beta, const double *__restrict__ x,
                                                             double *__restrict__ y, int64_t n_slices, const int *done) {
  const int done_flag = done ? *done : 0;  // (as in spmv_sell_kernel: loaded first, tested before the store)
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int bidx = (int)blockIdx.x;
  const int lb = XCD ? (A.xcd_group > 1 ? xcd_remap_grouped(bidx, gridDim.x, A.xcd_group) : xcd_remap(bidx, gridDim.x))
                     : bidx;
  const int64_t slice = (int64_t)lb * (kBlock / kWave) + wave;
  if (slice >= n_slices) return;  // wave-uniform; the kernel has no barrier
  const int64_t row = slice * kWave + lane;
  const bool valid = row < A.n_rows;
  const double xi = valid ? x[row] : 0.0;
  int64_t base;
  int width;
  if (A.uniform_width > 0) {
    width = A.uniform_width;
    base = slice * (int64_t)(kExt32Bytes + kSlot32Bytes * width);
  } else {
    base = A.slice_off[slice];
    width = (int)((A.slice_off[slice + 1] - base - kExt32Bytes) / kSlot32Bytes);
  }
  const char *rec = A.pack + base;
  const double ext = Rec32::ext<NT>(rec, lane);
  const double xi1[1] = {xi};
  double acc1[1];
  row_sum_any<NT, 1, Rec32>(rec, width, lane, x, xi1, acc1);
  const double yi = sell_row_result(false, 0.0, beta, xi, alpha, acc1[0], ext);
  if (valid && !done_flag) {
    if (NT) __builtin_nontemporal_store(yi, y + row);
    else y[row] = yi;
  }
}

__global__ __launch_bounds__(kBlock) void spmv_tail32_kernel(int64_t n_tail, const int *__restrict__ tail_row,
                                                             const int64_t *__restrict__ tail_ptr,
                                                             const int *__restrict__ tail_col,
                                                             const float *__restrict__ tail_val32, double alpha,
                                                             const double *__restrict__ x, double *__restrict__ y, const int *done) {
  if (done && *done) return;
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t t = (int64_t)blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6);
  if (t >= n_tail) return;
  tail_row_add(t, tail_row[t], lane, tail_ptr, tail_col, tail_val32, alpha, x, y, 1, 0);
}

int op_reduced_check(const storm_hip_op *op, const char *who) {
  if (op->pair != 0 || op->dict_size > 0 || op->offs_size > 0 || op->d_bnd_pack != nullptr)
    STORM_FAIL(STORM_HIP_E_UNSUPPORTED, "%s: reduced records are a companion of fp64 records (an operator built with option "
                                        "spmv_dict = 0); this operator is on a compact format", who);
  if (op->halo.n_nbrs > 0 || op->n_halo > 0 || op->ctx->comm != nullptr)
    STORM_FAIL(STORM_HIP_E_UNSUPPORTED, "%s: reduced records are single-rank (the operator has a halo plan or halo columns, or "
                                        "the context a communicator)", who);
  return STORM_HIP_OK;
}

int op_reduced_require(const storm_hip_op *op, const char *who) {
  STORM_TRY(op_reduced_check(op, who));
  if (op->d_pack32 == nullptr)
    STORM_FAIL(STORM_HIP_E_UNSUPPORTED, "%s: the operator (%lld rows) has no reduced records (call storm_hip_op_build_reduced first)",
               who, (long long)op->n_rows);
  return STORM_HIP_OK;
}

int op_reduced_convert(storm_hip_op *op, int *d_flag) {
  hipStream_t st = op->ctx->stream;
  if (op->n_slices > 0) {
    if (op->d_slice_off32 != nullptr)
      hipLaunchKernelGGL(op_reduce_offsets_kernel, dim3((int)((op->n_slices + 1 + kBlock - 1) / kBlock)), dim3(kBlock), 0, st,
                         op->n_slices, op->d_slice_off, op->d_slice_off32);
    const int nb = (int)((op->n_slices + (kBlock / kWave) - 1) / (kBlock / kWave));
    hipLaunchKernelGGL(op_reduce_sell_kernel, dim3(nb), dim3(kBlock), 0, st, op->d_pack, op->d_slice_off, op->d_pack32,
                       op->d_slice_off32, op->uniform_width, op->n_slices, d_flag);
  }
  if (op->tail_nnz > 0)
    hipLaunchKernelGGL(op_reduce_tail_kernel, dim3((int)((op->tail_nnz + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, op->tail_nnz,
                       op->d_tail_val, op->d_tail_val32, d_flag);
  HIP_TRY(hipGetLastError());
  return STORM_HIP_OK;
}

bool op_reduced_nt(const storm_hip_op *op) { return op->ctx->opt_nt != 0; }

int op_reduced_apply(const storm_hip_op *op, double alpha, double beta, const double *x, double *y, const int *done) {
  if (op->n_slices == 0) return STORM_HIP_OK;
  const SellArgs A{op->d_pack32, op->d_slice_off32, op->n_rows, op->uniform_width, op->xcd_group_sell, nullptr, 0, nullptr, 0, 0};
  const dim3 grid(blocks_for(op, op->n_slices)), block(kBlock);
  hipStream_t st = op->ctx->stream;
  const bool nt = op->ctx->opt_nt != 0, xcd = op->xcd_group_sell != 0;
#define SELL32_GO(NT_, XCD_) \
  hipLaunchKernelGGL((spmv_sell32_kernel<NT_, XCD_>), grid, block, 0, st, A, alpha, beta, x, y, op->n_slices, done)
  if (nt && xcd) SELL32_GO(true, true);
  else if (nt) SELL32_GO(true, false);
  else if (xcd) SELL32_GO(false, true);
  else SELL32_GO(false, false);
#undef SELL32_GO
  if (op->tail_rows > 0)
    hipLaunchKernelGGL(spmv_tail32_kernel, dim3((int)((op->tail_rows + 3) / 4)), dim3(kBlock), 0, st, op->tail_rows, op->d_tail_row,
                       op->d_tail_ptr, op->d_tail_col, op->d_tail_val32, alpha, x, y, done);
  HIP_TRY(hipGetLastError());
  return STORM_HIP_OK;
}

static int64_t reduced_alloc_bytes(const storm_hip_op *op) {
  return (op->pack32_bytes > 0 ? op->pack32_bytes : 1) + (op->d_slice_off32 ? (int64_t)sizeof(int64_t) * (op->n_slices + 1) : 0) +
         (int64_t)sizeof(float) * (op->tail_nnz > 0 ? op->tail_nnz : 1);
}

static void reduced_free(storm_hip_op *op) {
  (void)hipFree(op->d_pack32);
  (void)hipFree(op->d_slice_off32);
  (void)hipFree(op->d_tail_val32);
  op->d_pack32 = nullptr, op->d_slice_off32 = nullptr, op->d_tail_val32 = nullptr, op->pack32_bytes = 0;
}

}  // namespace storm

using namespace storm;

extern "C" {

int storm_hip_op_build_reduced(storm_hip_op *op) {
  STORM_REQUIRE(op, "op_build_reduced: null argument");
  STORM_TRY(op_reduced_check(op, "op_build_reduced"));
  if (op->d_pack32 != nullptr) return STORM_HIP_OK;
  storm_hip_ctx *c = op->ctx;
  HIP_TRY(hipSetDevice(c->device));
  STORM_TRY(lazy_sync(c));
  const int64_t slots = (op->pack_bytes - op->n_slices * kExtBytes) / kSlotBytes;  // of 64 entries, over all slices
  op->pack32_bytes = op->n_slices * kExt32Bytes + slots * kSlot32Bytes;
  int *d_flag = nullptr;
  hipError_t e = hipMalloc((void **)&op->d_pack32, (size_t)(op->pack32_bytes > 0 ? op->pack32_bytes : 1));
  if (e == hipSuccess && op->uniform_width == 0)
    e = hipMalloc((void **)&op->d_slice_off32, sizeof(int64_t) * (size_t)(op->n_slices + 1));
  if (e == hipSuccess) e = hipMalloc((void **)&op->d_tail_val32, sizeof(float) * (size_t)(op->tail_nnz > 0 ? op->tail_nnz : 1));
  if (e == hipSuccess) e = hipMalloc((void **)&d_flag, sizeof(int));
  if (e != hipSuccess) {
    reduced_free(op);
    (void)hipFree(d_flag);
    STORM_FAIL(STORM_HIP_E_ALLOC, "op_build_reduced: hipMalloc failed: %s", hipGetErrorString(e));
  }
  // one host wait, as storm_hip_op_gershgorin makes: the range flag
  int flag = 0, st = STORM_HIP_OK;
  e = hipMemsetAsync(d_flag, 0, sizeof(int), c->stream);
  if (e == hipSuccess) st = op_reduced_convert(op, d_flag);
  if (e == hipSuccess && st == STORM_HIP_OK) e = hipMemcpyAsync(&flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess && st == STORM_HIP_OK) e = hipStreamSynchronize(c->stream);
  (void)hipFree(d_flag);
  if (e != hipSuccess || st != STORM_HIP_OK || flag != 0) {
    reduced_free(op);
    if (st != STORM_HIP_OK) return st;
    HIP_TRY(e);
    STORM_FAIL(STORM_HIP_E_UNSUPPORTED, "op_build_reduced: a nonzero weight or diagonal term of the operator (%lld rows) is not finite "
                                        "or lies outside fp32's normal range [2^-126, FLT_MAX]", (long long)op->n_rows);
  }
  op->device_bytes += reduced_alloc_bytes(op);
  c->n_op_reduced_builds++;
  return STORM_HIP_OK;
}

int storm_hip_op_drop_reduced(storm_hip_op *op) {
  STORM_REQUIRE(op, "op_drop_reduced: null argument");
  if (op->d_pack32 == nullptr) return STORM_HIP_OK;
  (void)storm_hip_ctx_sync(op->ctx);  // kernels in flight may still read the records
  op->device_bytes -= reduced_alloc_bytes(op);
  reduced_free(op);
  return STORM_HIP_OK;
}

int storm_hip_op_reduced_bytes(const storm_hip_op *op, int64_t *record_bytes) {
  STORM_REQUIRE(op && record_bytes, "op_reduced_bytes: null argument");
  *record_bytes = op->d_pack32 != nullptr ? op->pack32_bytes : 0;
  return STORM_HIP_OK;
}

int storm_hip_op_apply_reduced(const storm_hip_op *op, double alpha, double beta, const storm_hip_vec *x, storm_hip_vec *y) {
  STORM_REQUIRE(op && x && y, "op_apply_reduced: null argument");
  STORM_REQUIRE(x->ctx == op->ctx && y->ctx == op->ctx, "op_apply_reduced: context mismatch");
  STORM_REQUIRE(x != y && x->d != y->d, "op_apply_reduced: x and y must not alias");
  STORM_REQUIRE(x->n_owned == op->n_rows && y->n_owned == op->n_rows, "op_apply_reduced: operator has %lld rows, x %lld, y %lld",
                (long long)op->n_rows, (long long)x->n_owned, (long long)y->n_owned);
  STORM_TRY(op_reduced_require(op, "op_apply_reduced"));
  HIP_TRY(hipSetDevice(op->ctx->device));
  STORM_TRY(lazy_sync(op->ctx));
  return op_reduced_apply(op, alpha, beta, x->d, y->d, op->ctx->api_done);
}

int storm_hip_op_gershgorin_reduced(const storm_hip_op *op, double alpha, double beta, const storm_hip_vec *scale, double *lambda_max) {
  STORM_REQUIRE(op && lambda_max, "op_gershgorin_reduced: null argument");
  STORM_REQUIRE(scale == nullptr || (scale->ctx == op->ctx && scale->n_owned == op->n_rows),
                "op_gershgorin_reduced: the scale must be a vector of the operator's context and size");
  STORM_TRY(op_reduced_require(op, "op_gershgorin_reduced"));
  return gershgorin_run(op, true, alpha, beta, scale, lambda_max);
}

}  // extern "C"
