// The Chebyshev polynomial preconditioner (storm_hip_cheb_*): z = p_m(diag(s) A) diag(s) r for A = beta I + alpha M.
// Recurrence and the statement sequence that fixes the rounding: include/storm_hip.h ("Chebyshev polynomial preconditioner").
//
// Two paths, the same bits:
//   statements  the sequence of the header in library calls (every record format, with or without a CSR tail);
//   fused       fp64 records (format 0) without a CSR tail: cheb_d0_kernel, then one cheb_step_kernel per product.  The step
//               kernel has spmv_sell_kernel's shape (one wavefront per slice, one row per lane, the same XCD runs, records
//               non-temporal, the gathered direction read plainly so that it stays in L2); the row's product comes from
//               row_sum_any / sell_row_result (sell_device.hpp) and a x0 + b x1 from axpbz_value (blas1_device.hpp): nothing
//               that rounds is restated.  Multiplications by +-1 of the statements are exact, so `res - t` and `z + d` stand
//               for axpbz(1, res, -1, t) and axpbz(1, d, 1, z).  The new direction goes to the OTHER buffer: neighbours still
//               gather the old one.  Per row and step: records + 8 (res in) + 8 (res out) + 8 (direction out) + 8 + 8 (z) bytes,
//               + 8 with the scale; FIRST reads the caller's r for res and does not read z, LAST stores z only.
// A REDUCED object (storm_hip_cheb_create_reduced) takes its operator products from the operator's fp32-weight companion
// records (op_reduced.hip): the fused step is the same kernel with the record policy Rec32 (sell_device.hpp), the statement
// path calls storm_hip_op_apply_reduced in place of storm_hip_op_apply.
#include <cmath>
#include <cstring>
#include <utility>

#include "amg_device.hpp"

namespace storm {

struct ChebStepArgs {
  double c1, c2;
  const double *d;       // d_k: this row's value and the gathered neighbours
  double *d_out;         // d_{k+1} (not LAST)
  const double *res_in;  // FIRST: the caller's r (never written); else the object's residual
  double *res_out;       // (not LAST)
  const double *s;       // JACOBI: the scale
  double *z;
};

// d_0 = it (s .* r)  (JACOBI)  /  it r: vmul's product, then the one-term statement's.
template <bool JACOBI>
__global__ __launch_bounds__(kBlock) void cheb_d0_kernel(int64_t n, double inv_theta, const double *__restrict__ r,
                                                         const double *__restrict__ s, double *__restrict__ d, const int *done,
                                                         int nt) {
  if (done && *done) return;
  const int64_t n2 = n >> 1;
  const double2v *__restrict__ r2 = reinterpret_cast<const double2v *>(r);
  const double2v *__restrict__ s2 = reinterpret_cast<const double2v *>(s);
  double2v *__restrict__ d2 = reinterpret_cast<double2v *>(d);
  nt_dispatch(nt, [&](auto nt_) {
    for (int64_t base = (int64_t)blockIdx.x * (kBlock * kUnroll) + threadIdx.x; base < n2;
         base += (int64_t)gridDim.x * (kBlock * kUnroll)) {
      double2v vr[kUnroll], vs[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int64_t i = base + u * kBlock;
        if (i < n2) {
          vr[u] = ld2(r2 + i, nt_);
          if (JACOBI) vs[u] = ld2(s2 + i, nt_);
        }
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int64_t i = base + u * kBlock;
        if (i < n2) {
          double2v o;
          o.x = cheb_d0_value<JACOBI>(inv_theta, vr[u].x, JACOBI ? vs[u].x : 1.0);
          o.y = cheb_d0_value<JACOBI>(inv_theta, vr[u].y, JACOBI ? vs[u].y : 1.0);
          st2(d2 + i, o, nt_);
        }
      }
    }
  });
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    d[n - 1] = cheb_d0_value<JACOBI>(inv_theta, r[n - 1], JACOBI ? s[n - 1] : 1.0);
  }
}

// One Chebyshev step on a slice per wavefront:
//   t = A d;  res' = res - t;  d' = c1 d + c2 (s .* res');  z' = z + d'   (FIRST: z' = d + d').
template <bool NT, bool XCD, bool JACOBI, bool FIRST, bool LAST, class R>
__global__ __launch_bounds__(kBlock) void cheb_step_kernel(SellArgs A, double alpha, double beta, ChebStepArgs C,
                                                           int64_t n_slices, const int *done) {
  // (as in spmv_sell_kernel: the predicate is loaded first and tested before the first store)
  const int done_flag = done ? *done : 0;
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int bidx = (int)blockIdx.x;
  const int lb = XCD ? (A.xcd_group > 1 ? xcd_remap_grouped(bidx, gridDim.x, A.xcd_group) : xcd_remap(bidx, gridDim.x))
                     : bidx;
  const int64_t slice = (int64_t)lb * (kBlock / kWave) + wave;
  if (slice >= n_slices) return;  // wave-uniform; the kernel has no barrier
  const int64_t row = slice * kWave + lane;
  const bool valid = row < A.n_rows;
  const double *__restrict__ dv = C.d;
  const double xi = valid ? dv[row] : 0.0;
  // the row's own streams, early: off the tail of the dependency chain
  const double ri = valid ? ld_d<NT>(C.res_in + row) : 0.0;
  double si = 1.0, zi = 0.0;
  if (JACOBI) si = valid ? ld_d<NT>(C.s + row) : 0.0;
  if (!FIRST) zi = valid ? ld_d<NT>(C.z + row) : 0.0;
  const double t = sell_row_apply<NT, R>(A, slice, lane, dv, xi, alpha, beta);
  const ChebRow o = cheb_step_row<JACOBI, FIRST>(t, ri, si, xi, zi, C.c1, C.c2);
  if (valid && !done_flag) {
    if (!LAST) {
      if (NT) __builtin_nontemporal_store(o.rn, C.res_out + row), __builtin_nontemporal_store(o.dn, C.d_out + row);
      else C.res_out[row] = o.rn, C.d_out[row] = o.dn;
    }
    if (NT) __builtin_nontemporal_store(o.zn, C.z + row);
    else C.z[row] = o.zn;
  }
}

int cheb_scaled_start(storm_hip_ctx *c, int64_t n, double inv_theta, const double *r, const double *s, double *d) {
  if (n <= 0) return STORM_HIP_OK;
  hipLaunchKernelGGL(cheb_d0_kernel<true>, dim3(stream_blocks(n)), dim3(kBlock), 0, c->stream, n, inv_theta, r, s, d, c->api_done,
                     stream_nt(c, n));
  HIP_TRY(hipGetLastError());
  return STORM_HIP_OK;
}

static bool cheb_fused_applies(const storm_hip_cheb *h) {
  const storm_hip_op *op = h->op;
  return h->ctx->opt_cheb_fused != 0 && op->pair == 0 && op->dict_size == 0 && op->offs_size == 0 && op->tail_rows == 0 &&
         op->d_bnd_pack == nullptr && op->n_rows > 0;
}

template <bool NT, bool XCD, bool JACOBI>
static void launch_step(const storm_hip_cheb *h, const SellArgs &A, const ChebStepArgs &C, bool first, bool last, const int *done) {
  const storm_hip_op *op = h->op;
  const dim3 grid(blocks_for(op, op->n_slices)), block(kBlock);
  hipStream_t st = h->ctx->stream;
#define CHEB_GO(F_, L_) \
  do {                                                                                                                             \
    if (h->reduced)                                                                                                                \
      hipLaunchKernelGGL((cheb_step_kernel<NT, XCD, JACOBI, F_, L_, Rec32>), grid, block, 0, st, A, h->alpha, h->beta, C, op->n_slices, done); \
    else                                                                                                                           \
      hipLaunchKernelGGL((cheb_step_kernel<NT, XCD, JACOBI, F_, L_, Rec64>), grid, block, 0, st, A, h->alpha, h->beta, C, op->n_slices, done); \
  } while (0)
  if (first && last) CHEB_GO(true, true);
  else if (first) CHEB_GO(true, false);
  else if (last) CHEB_GO(false, true);
  else CHEB_GO(false, false);
#undef CHEB_GO
}

static int cheb_apply_fused(const storm_hip_cheb *h, const storm_hip_vec *r, storm_hip_vec *z) {
  storm_hip_ctx *c = h->ctx;
  const storm_hip_op *op = h->op;
  const int *done = c->api_done;
  const int64_t n = op->n_rows;
  const bool jacobi = h->dinv != nullptr;
  if (jacobi)
    hipLaunchKernelGGL(cheb_d0_kernel<true>, dim3(stream_blocks(n)), dim3(kBlock), 0, c->stream, n, h->inv_theta, r->d,
                       h->dinv->d, h->d[0]->d, done, stream_nt(c, n));
  else
    hipLaunchKernelGGL(cheb_d0_kernel<false>, dim3(stream_blocks(n)), dim3(kBlock), 0, c->stream, n, h->inv_theta, r->d,
                       (const double *)nullptr, h->d[0]->d, done, stream_nt(c, n));
  SellArgs A{op->d_pack, op->d_slice_off, op->n_rows, op->uniform_width, op->xcd_group_sell, op->d_dict, op->dict_size,
             op->d_offs, op->offs_size, 0};
  if (h->reduced) A.pack = op->d_pack32, A.slice_off = op->d_slice_off32;
  const bool nt = c->opt_nt != 0, xcd = op->xcd_group_sell != 0;
  for (int k = 0; k < h->degree; ++k) {
    const bool first = k == 0, last = k == h->degree - 1;
    const ChebStepArgs C{h->c1[k], h->c2[k], h->d[k & 1]->d, h->d[(k + 1) & 1]->d, first ? r->d : h->res->d, h->res->d,
                         jacobi ? h->dinv->d : nullptr, z->d};
#define CHEB_J(NT_, XCD_)                                                 \
  do {                                                                    \
    if (jacobi) launch_step<NT_, XCD_, true>(h, A, C, first, last, done); \
    else launch_step<NT_, XCD_, false>(h, A, C, first, last, done);       \
  } while (0)
    if (nt && xcd) CHEB_J(true, true);
    else if (nt) CHEB_J(true, false);
    else if (xcd) CHEB_J(false, true);
    else CHEB_J(false, false);
#undef CHEB_J
  }
  HIP_TRY(hipGetLastError());
  return STORM_HIP_OK;
}

// The sequence of the header, in library calls.  They go out as they are issued (no lazy_statements hold-back: the
// calls see callback_depth > 0), predicated on the context's api_done like any call a solver callback makes.
static int cheb_apply_statements(const storm_hip_cheb *h, const storm_hip_vec *r, storm_hip_vec *z) {
  struct Depth {
    storm_hip_ctx *c;
    explicit Depth(storm_hip_ctx *c_) : c(c_) { ++c->callback_depth; }
    ~Depth() { --c->callback_depth; }
  } depth(h->ctx);
  const storm_hip_vec *s = h->dinv;
  storm_hip_vec *d = h->d[0], *e = h->d[1], *res = h->res;
  if (s != nullptr) {
    STORM_TRY(storm_hip_vmul(d, s, r));
    STORM_TRY(storm_hip_axpbz(d, h->inv_theta, d, 0.0, d));
  } else {
    STORM_TRY(storm_hip_axpbz(d, h->inv_theta, r, 0.0, r));
  }
  for (int k = 0; k < h->degree; ++k) {
    if (h->reduced) STORM_TRY(storm_hip_op_apply_reduced(h->op, h->alpha, h->beta, d, e));
    else STORM_TRY(storm_hip_op_apply(h->op, h->alpha, h->beta, d, e));
    STORM_TRY(storm_hip_axpbz(res, 1.0, k == 0 ? r : res, -1.0, e));
    if (s != nullptr) {
      STORM_TRY(storm_hip_vmul(e, s, res));
      STORM_TRY(storm_hip_axpbz(e, h->c1[k], d, h->c2[k], e));
    } else {
      STORM_TRY(storm_hip_axpbz(e, h->c1[k], d, h->c2[k], res));
    }
    if (k == 0) STORM_TRY(storm_hip_axpbz(z, 1.0, d, 1.0, e));
    else STORM_TRY(storm_hip_axpy(z, 1.0, e));
    std::swap(d, e);
  }
  return STORM_HIP_OK;
}

static int cheb_single_rank(const storm_hip_op *op, const char *what) {
  if (op->halo.n_nbrs > 0 || op->n_halo > 0 || op->ctx->comm != nullptr)
    STORM_FAIL(STORM_HIP_E_UNSUPPORTED, "%s: the Chebyshev preconditioner is single-rank (the operator has a halo plan or halo "
                                        "columns, or the context a communicator)", what);
  return STORM_HIP_OK;
}

static int cheb_create(const storm_hip_op *op, double alpha, double beta, const storm_hip_vec *dinv, int degree, double lmin,
                       double lmax, bool reduced, storm_hip_cheb **out) {
  const char *who = reduced ? "cheb_create_reduced" : "cheb_create";
  STORM_REQUIRE(op && out, "%s: null argument", who);
  *out = nullptr;
  STORM_REQUIRE(degree >= 1 && degree <= kChebMaxDegree, "%s: degree %d (1 .. %d)", who, degree, kChebMaxDegree);
  STORM_REQUIRE(dinv == nullptr || dinv->ctx == op->ctx, "%s: the scale belongs to another context", who);
  STORM_REQUIRE(dinv == nullptr || dinv->n_owned == op->n_rows, "%s: operator has %lld rows, the scale %lld", who,
                (long long)op->n_rows, (long long)(dinv ? dinv->n_owned : 0));
  STORM_REQUIRE(std::isfinite(lmin) && std::isfinite(lmax), "%s: the bounds must be finite", who);
  STORM_TRY(cheb_single_rank(op, who));
  if (reduced) STORM_TRY(op_reduced_require(op, who));
  HIP_TRY(hipSetDevice(op->ctx->device));
  if (lmax <= 0.0) {
    if (reduced) STORM_TRY(storm_hip_op_gershgorin_reduced(op, alpha, beta, dinv, &lmax));
    else STORM_TRY(storm_hip_op_gershgorin(op, alpha, beta, dinv, &lmax));
  }
  if (lmin <= 0.0) lmin = lmax / 30.0;
  storm_hip_cheb *h = new storm_hip_cheb();
  h->ctx = op->ctx, h->op = op, h->alpha = alpha, h->beta = beta, h->dinv = dinv, h->degree = degree;
  h->lmin = lmin, h->lmax = lmax, h->reduced = reduced ? 1 : 0;
  int st = storm_hip_cheb_coefficients(lmin, lmax, degree, &h->theta, h->c1, h->c2);
  h->inv_theta = 1.0 / h->theta;
  storm_hip_vec **vs[3] = {&h->d[0], &h->d[1], &h->res};
  for (int i = 0; i < 3 && st == STORM_HIP_OK; ++i) st = storm_hip_vec_create(op->ctx, op->n_rows, 0, vs[i]);
  if (st != STORM_HIP_OK) {
    (void)storm_hip_cheb_destroy(h);
    return st;
  }
  *out = h;
  return STORM_HIP_OK;
}

}  // namespace storm

using namespace storm;

extern "C" {

int storm_hip_cheb_coefficients(double lmin, double lmax, int degree, double *theta, double *c1, double *c2) {
  STORM_REQUIRE(theta && c1 && c2, "cheb_coefficients: null argument");
  STORM_REQUIRE(std::isfinite(lmin) && std::isfinite(lmax) && 0.0 < lmin && lmin < lmax,
                "cheb_coefficients: the interval [%g, %g] must be finite with 0 < lmin < lmax", lmin, lmax);
  STORM_REQUIRE(degree >= 1 && degree <= kChebMaxDegree, "cheb_coefficients: degree %d (1 .. %d)", degree, kChebMaxDegree);
  const double th = (lmax + lmin) / 2.0, de = (lmax - lmin) / 2.0, sigma = th / de;
  double rho = 1.0 / sigma;
  for (int k = 0; k < degree; ++k) {
    const double rn = 1.0 / (2.0 * sigma - rho);
    c1[k] = rn * rho, c2[k] = 2.0 * rn / de;
    rho = rn;
  }
  *theta = th;
  return STORM_HIP_OK;
}

int storm_hip_cheb_create(const storm_hip_op *op, double alpha, double beta, const storm_hip_vec *dinv, int degree, double lmin,
                          double lmax, storm_hip_cheb **out) {
  return cheb_create(op, alpha, beta, dinv, degree, lmin, lmax, false, out);
}

int storm_hip_cheb_create_reduced(const storm_hip_op *op, double alpha, double beta, const storm_hip_vec *dinv, int degree,
                                  double lmin, double lmax, storm_hip_cheb **out) {
  return cheb_create(op, alpha, beta, dinv, degree, lmin, lmax, true, out);
}

int storm_hip_cheb_destroy(storm_hip_cheb *h) {
  if (!h) return STORM_HIP_OK;
  (void)storm_hip_vec_destroy(h->d[0]);
  (void)storm_hip_vec_destroy(h->d[1]);
  (void)storm_hip_vec_destroy(h->res);
  delete h;
  return STORM_HIP_OK;
}

int storm_hip_cheb_get(const storm_hip_cheb *h, const char *key, double *value) {
  STORM_REQUIRE(h && key && value, "cheb_get: null argument");
  if (!strcmp(key, "lambda_min")) *value = h->lmin;
  else if (!strcmp(key, "lambda_max")) *value = h->lmax;
  else if (!strcmp(key, "degree")) *value = (double)h->degree;
  else if (!strcmp(key, "reduced")) *value = (double)h->reduced;
  else STORM_FAIL(STORM_HIP_E_INVALID, "cheb_get: unknown key '%s'", key);
  return STORM_HIP_OK;
}

int storm_hip_cheb_apply(const storm_hip_cheb *h, const storm_hip_vec *r, storm_hip_vec *z) {
  STORM_REQUIRE(h && r && z, "cheb_apply: null argument");
  STORM_REQUIRE(r->ctx == h->ctx && z->ctx == h->ctx, "cheb_apply: context mismatch");
  STORM_REQUIRE(z != r && z->d != r->d, "cheb_apply: z must not alias r");
  STORM_REQUIRE(r->n_owned == h->op->n_rows && z->n_owned == h->op->n_rows, "cheb_apply: operator has %lld rows, r %lld, z %lld",
                (long long)h->op->n_rows, (long long)r->n_owned, (long long)z->n_owned);
  storm_hip_ctx *c = h->ctx;
  HIP_TRY(hipSetDevice(c->device));
  STORM_TRY(lazy_sync(c));
  if (h->op->n_rows == 0) return STORM_HIP_OK;
  if (h->reduced) {  // (the companion may have been dropped since the object was created)
    STORM_TRY(op_reduced_require(h->op, "cheb_apply"));
    ++c->n_cheb_reduced_applies;
  }
  if (cheb_fused_applies(h)) {
    ++c->n_cheb_fused_applies;
    return cheb_apply_fused(h, r, z);
  }
  ++c->n_cheb_statement_applies;
  return cheb_apply_statements(h, r, z);
}

}  // extern "C"
