// The device half of the smoothed-aggregation multigrid preconditioner (storm_hip_amg_*): z = B r, one symmetric V-cycle
// for A = beta I + alpha M.  Recipe and cycle: include/storm_hip.h; the hierarchy comes from amg_setup.hip (host).
//
// Per level: a Jacobi-scaled Chebyshev smoother (precond_cheb.hip, the existing object), the level's operator (level 0: the
// caller's; below: fp64 records from the CSR packer), the transfer records P and R = P^T, four work vectors.  The cycle
// enqueues and never waits: no reduction, no host wait, no atomics, no cooperative launch.  Kernels of this unit:
//   amg_residual_kernel     t = r - A z on fp64 records without a CSR tail: spmv_sell_kernel's / cheb_step_kernel's shape (one
//                           wavefront per slice, one row per lane, the same XCD runs, records non-temporal, z gathered
//                           plainly), the product from row_sum_any / sell_row_result, then fl(r_i - t_i): the bits of
//                           storm_hip_op_apply(op, alpha, beta, z, t); storm_hip_axpbz(t, 1, r, -1, t), which any other
//                           level (or option amg_fused = 0) takes.
//   amg_transfer_kernel     y = T x (restriction) or y += T x (prolongation) on the transfer records: one wavefront per slice
//                           of 64 rows, one row per lane, acc = fma(w_k, x[c_k], acc) in slot order.
//   amg_coarse_kernel       z = Ainv r, dense: one wavefront per row, lane j takes columns j, j + 64, ... by fma, then the
//                           wavefront's sum (wave_device.hpp).
// A null-space object (storm_hip_amg_create_nullspace) is B = Pi V Pi, Pi = I - 1 1^T / n on level 0; streaming kernels of
// blas1.hip's shape, the one reduction finished by tickets inside the kernel that formed its partial sums:
//   amg_mean_kernel         S = sum v, then mu = S / n into the object's slot by the block that drew the last ticket
//   amg_shift_kernel        out_i = v_i - mu
//   amg_axpy_mean_kernel    level 0's closing z = z + e with S of the stored z in the same launch (option amg_fused)
// An object of storm_hip_amg_create_smoother with kind 1 smooths by damped Jacobi sweeps instead (no storm_hip_cheb):
//   amg_jacobi_sweep_kernel z' = z + sigma (s .* (r - A z)) into the other buffer: amg_residual_kernel's shape and product on the
//                           record policy R (Rec64; Rec32 on the fp32-weight companion with reduced_records), then the scale's
//                           product and axpbz_value: the bits of storm_hip_op_apply; storm_hip_axpbz(t, 1, r, -1, t);
//                           storm_hip_vmul(t, s, t); storm_hip_axpbz(z', sigma, t, 1, z), which any other level takes.
// Every kernel loads the context's api_done word first and tests it before its first store.
// A row's arithmetic lives in amg_device.hpp, shared with amg_tail.hip: with option amg_tail the cycle hands a level, everything
// below it and the way back up to ONE cooperative kernel (amg_cycle asks amg_tail_run first; refused: the launches below).
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "amg.hpp"
#include "amg_device.hpp"
#include "ticket_device.hpp"
#include "wave_device.hpp"

namespace storm {

template <bool NT, bool XCD>
__global__ __launch_bounds__(kBlock) void amg_residual_kernel(SellArgs A, double alpha, double beta, const double *__restrict__ r,
                                                              const double *__restrict__ z, double *__restrict__ t,
                                                              int64_t n_slices, const int *done) {
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
  const double zi = valid ? z[row] : 0.0;
  const double ri = valid ? ld_d<NT>(r + row) : 0.0;  // the row's own stream, early
  const double az = sell_row_apply<NT, Rec64>(A, slice, lane, z, zi, alpha, beta);
  const double tn = amg_residual_value(ri, az);
  if (valid && !done_flag) {
    if (NT) __builtin_nontemporal_store(tn, t + row);
    else t[row] = tn;
  }
}

// One damped-Jacobi sweep z' = z + sigma (s .* (r - A z)) on a slice per wavefront: amg_residual_kernel with the record policy
// R, then vmul's product and the axpy statement's a x + 1 y.  z' goes to the OTHER buffer: neighbours still gather the old z.
template <bool NT, bool XCD, class R>
__global__ __launch_bounds__(kBlock) void amg_jacobi_sweep_kernel(SellArgs A, double alpha, double beta, double sigma,
                                                                  const double *__restrict__ r, const double *__restrict__ s,
                                                                  const double *__restrict__ z, double *__restrict__ z_out,
                                                                  int64_t n_slices, const int *done) {
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
  const double zi = valid ? z[row] : 0.0;
  const double ri = valid ? ld_d<NT>(r + row) : 0.0;  // the row's own streams, early
  const double si = valid ? ld_d<NT>(s + row) : 0.0;
  const double az = sell_row_apply<NT, R>(A, slice, lane, z, zi, alpha, beta);
  const double zn = amg_jacobi_value(ri, az, si, sigma, zi);
  if (valid && !done_flag) {
    if (NT) __builtin_nontemporal_store(zn, z_out + row);
    else z_out[row] = zn;
  }
}

// y_i = [y_i +] sum_k w_k x[c_k] over the slots of the row's slice, in slot order.
template <bool ADD>
__global__ __launch_bounds__(kBlock) void amg_transfer_kernel(const char *__restrict__ pack, const int64_t *__restrict__ off,
                                                              int64_t n_rows, int64_t n_slices, const double *__restrict__ x,
                                                              double *__restrict__ y, const int *done) {
  const int done_flag = done ? *done : 0;
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t slice = (int64_t)blockIdx.x * (kBlock / kWave) + wave;
  if (slice >= n_slices) return;  // wave-uniform
  const int64_t row = slice * kWave + lane;
  const bool valid = row < n_rows;
  double yi = 0.0;
  if (ADD) yi = valid ? y[row] : 0.0;
  const double yn = amg_transfer_row<ADD>(pack, off, slice, lane, x, yi);
  if (valid && !done_flag) y[row] = yn;
}

__global__ __launch_bounds__(kBlock) void amg_coarse_kernel(const double *__restrict__ ainv, int64_t n, const double *__restrict__ r,
                                                            double *__restrict__ z, const int *done) {
  const int done_flag = done ? *done : 0;
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t row = (int64_t)blockIdx.x * (kBlock / kWave) + wave;
  if (row >= n) return;  // wave-uniform: all 64 lanes take part in the sum
  const double acc = amg_coarse_row(ainv, n, row, lane, r);  // the total in lane 0
  if (lane == 0 && !done_flag) z[row] = acc;
}

// ---- the projection Pi = I - 1 1^T / n of a null-space object ---------------------------------------------------------------
// This thread's share of S = sum_i v_i on the stream_blocks(n) grid (blas1.hip's shape: a block owns 2048 consecutive
// entries per trip, a thread four 16-byte words of them; the odd last entry goes to thread 0 of block 0 behind its words).
// AXPY: v_i = z_i + e_i is formed and STORED first and the stored value is what is summed -- ONE loop for amg_mean_kernel and
// amg_axpy_mean_kernel, so the partition and the order, hence the bits of S, do not depend on which of them ran.
template <bool AXPY>
__device__ __forceinline__ double amg_sum_accumulate(int64_t n, double *z, const double *__restrict__ e, int nt) {
  const int64_t n2 = n >> 1;
  double2v *z2 = reinterpret_cast<double2v *>(z);
  const double2v *__restrict__ e2 = reinterpret_cast<const double2v *>(e);
  double acc = 0.0;
  nt_dispatch(nt, [&](auto nt) {
    for (int64_t base = (int64_t)blockIdx.x * (kBlock * kUnroll) + threadIdx.x; base < n2;
         base += (int64_t)gridDim.x * (kBlock * kUnroll)) {
      double2v v[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int64_t i = base + u * kBlock;
        if (i < n2) {
          v[u] = ld2(z2 + i, nt);
          if (AXPY) v[u] = v[u] + ld2(e2 + i, nt);
        }
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int64_t i = base + u * kBlock;
        if (i < n2) {
          if (AXPY) st2(z2 + i, v[u], nt);
          acc += v[u].x;
          acc += v[u].y;
        }
      }
    }
  });
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    double last = z[n - 1];
    if (AXPY) last = last + e[n - 1], z[n - 1] = last;
    acc += last;
  }
  return acc;
}

// The block sum, the two-level ticket fold (ticket_device.hpp), and mu = S / n by the block that drew the last ticket.
__device__ __forceinline__ void amg_mean_finish(double acc, int64_t n, const TicketArgs &t, double *mu) {
  __shared__ double lds[1][4];
  const double a1[1] = {acc};
  double mine[1], total[1];
  block_sum_multi<1>(a1, lds, mine);
  if (threadIdx.x >= kWave) return;
  if (ticket_reduce_wave0<1>(t, mine, 1, blockIdx.x, gridDim.x, total) && threadIdx.x == 0) *mu = __ddiv_rn(total[0], (double)n);
}

// (the done flag is the same for every block of a launch -- it is written by kernels earlier on the stream only -- so either
//  all blocks draw their tickets or none does)
__global__ __launch_bounds__(kBlock) void amg_mean_kernel(int64_t n, const double *v, TicketArgs t, double *mu, const int *done, int nt) {
  const int done_flag = done ? *done : 0;
  if (done_flag) return;
  amg_mean_finish(amg_sum_accumulate<false>(n, const_cast<double *>(v), nullptr, nt), n, t, mu);
}

__global__ __launch_bounds__(kBlock) void amg_axpy_mean_kernel(int64_t n, double *z, const double *e, TicketArgs t, double *mu,
                                                               const int *done, int nt) {
  const int done_flag = done ? *done : 0;
  if (done_flag) return;
  amg_mean_finish(amg_sum_accumulate<true>(n, z, e, nt), n, t, mu);
}

// out_i = v_i - mu (out == v: in place)
__global__ __launch_bounds__(kBlock) void amg_shift_kernel(int64_t n, const double *v, const double *mu, double *out, const int *done,
                                                           int nt) {
  const int done_flag = done ? *done : 0;
  if (done_flag) return;
  const double m = *mu;
  const int64_t n2 = n >> 1;
  const double2v *v2 = reinterpret_cast<const double2v *>(v);
  double2v *o2 = reinterpret_cast<double2v *>(out);
  nt_dispatch(nt, [&](auto nt) {
    for (int64_t base = (int64_t)blockIdx.x * (kBlock * kUnroll) + threadIdx.x; base < n2;
         base += (int64_t)gridDim.x * (kBlock * kUnroll)) {
      double2v w[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int64_t i = base + u * kBlock;
        if (i < n2) w[u] = ld2(v2 + i, nt);
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int64_t i = base + u * kBlock;
        if (i < n2) st2(o2 + i, w[u] - m, nt);
      }
    }
  });
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) out[n - 1] = v[n - 1] - m;
}

static TicketArgs amg_tickets(const storm_hip_amg *h) { return TicketArgs{h->d_mean_cnt, h->d_mean_part1, h->d_mean_part2}; }

// mu[slot] = fl(sum(v) / n); with e: v = v + e first (the closing statement of level 0)
static int amg_mean(const storm_hip_amg *h, storm_hip_vec *v, const storm_hip_vec *e, int slot) {
  storm_hip_ctx *c = h->ctx;
  const int64_t n = v->n_owned;
  const dim3 grid(stream_blocks(n)), block(kBlock);
  if (e)
    hipLaunchKernelGGL(amg_axpy_mean_kernel, grid, block, 0, c->stream, n, v->d, e->d, amg_tickets(h), h->d_mu + slot, c->api_done,
                       stream_nt(c, n));
  else
    hipLaunchKernelGGL(amg_mean_kernel, grid, block, 0, c->stream, n, v->d, amg_tickets(h), h->d_mu + slot, c->api_done, stream_nt(c, n));
  HIP_TRY(hipGetLastError());
  return STORM_HIP_OK;
}

static int amg_shift(const storm_hip_amg *h, const storm_hip_vec *v, int slot, storm_hip_vec *out) {
  storm_hip_ctx *c = h->ctx;
  const int64_t n = v->n_owned;
  hipLaunchKernelGGL(amg_shift_kernel, dim3(stream_blocks(n)), dim3(kBlock), 0, c->stream, n, v->d, h->d_mu + slot, out->d, c->api_done,
                     stream_nt(c, n));
  HIP_TRY(hipGetLastError());
  return STORM_HIP_OK;
}

int op_create_csr_fp64(storm_hip_ctx *c, int64_t n_rows, const int64_t *row_ptr, const int64_t *col, const double *val,
                       bool source_map, storm_hip_op **out);  // spmv_build.hip

bool amg_residual_fused(const storm_hip_amg *h, const storm_hip_op *op) {
  return h->ctx->opt_amg_fused != 0 && op->pair == 0 && op->dict_size == 0 && op->offs_size == 0 && op->tail_rows == 0 &&
         op->d_bnd_pack == nullptr && op->n_rows > 0;
}

// t = r - A_l z
static int amg_residual(const storm_hip_amg *h, const storm_hip_amg::Level &L, const storm_hip_vec *r, const storm_hip_vec *z,
                        storm_hip_vec *t) {
  storm_hip_ctx *c = h->ctx;
  const storm_hip_op *op = L.op;
  if (!amg_residual_fused(h, op)) {
    ++c->n_amg_statement_residuals;
    STORM_TRY(storm_hip_op_apply(op, L.alpha, L.beta, z, t));
    return storm_hip_axpbz(t, 1.0, r, -1.0, t);
  }
  ++c->n_amg_fused_residuals;
  const SellArgs A{op->d_pack, op->d_slice_off, op->n_rows, op->uniform_width, op->xcd_group_sell, op->d_dict, op->dict_size,
                   op->d_offs, op->offs_size, 0};
  const dim3 grid(blocks_for(op, op->n_slices)), block(kBlock);
  const bool nt = c->opt_nt != 0, xcd = op->xcd_group_sell != 0;
#define AMG_RES_GO(NT_, XCD_)                                                                                               \
  hipLaunchKernelGGL((amg_residual_kernel<NT_, XCD_>), grid, block, 0, c->stream, A, L.alpha, L.beta, r->d, z->d, t->d, \
                     op->n_slices, c->api_done)
  if (nt && xcd) AMG_RES_GO(true, true);
  else if (nt) AMG_RES_GO(true, false);
  else if (xcd) AMG_RES_GO(false, true);
  else AMG_RES_GO(false, false);
#undef AMG_RES_GO
  HIP_TRY(hipGetLastError());
  return STORM_HIP_OK;
}

static int amg_transfer(const storm_hip_amg *h, const storm_hip_amg::Transfer &T, bool add, const storm_hip_vec *x, storm_hip_vec *y) {
  storm_hip_ctx *c = h->ctx;
  const dim3 grid((unsigned)((T.n_slices + 3) / 4)), block(kBlock);
  if (add)
    hipLaunchKernelGGL(amg_transfer_kernel<true>, grid, block, 0, c->stream, T.d_pack, T.d_off, T.n_rows, T.n_slices, x->d, y->d,
                       c->api_done);
  else
    hipLaunchKernelGGL(amg_transfer_kernel<false>, grid, block, 0, c->stream, T.d_pack, T.d_off, T.n_rows, T.n_slices, x->d, y->d,
                       c->api_done);
  HIP_TRY(hipGetLastError());
  return STORM_HIP_OK;
}

// ---- the Jacobi smoother (storm_hip_amg_create_smoother, kind 1) ------------------------------------------------------------
static bool amg_reduced(const storm_hip_amg *h) { return h->hier->params.reduced_records != 0; }

// z = sigma (s .* r): a sweep from the zero guess.  Fused: cheb_d0_kernel<JACOBI>; otherwise its two statements.
static int amg_jacobi_start(const storm_hip_amg *h, const storm_hip_amg::Level &L, const storm_hip_vec *r, storm_hip_vec *z) {
  if (amg_residual_fused(h, L.op)) return cheb_scaled_start(h->ctx, L.n, L.sigma, r->d, L.dinv->d, z->d);
  STORM_TRY(storm_hip_vmul(z, L.dinv, r));
  return storm_hip_axpbz(z, L.sigma, z, 0.0, z);
}

// z_out = z_in + sigma (s .* (r - A_l z_in)); z_out is not z_in, L.t is the statements' work vector
static int amg_jacobi_sweep(const storm_hip_amg *h, const storm_hip_amg::Level &L, const storm_hip_vec *r, const storm_hip_vec *z_in,
                            storm_hip_vec *z_out) {
  storm_hip_ctx *c = h->ctx;
  const storm_hip_op *op = L.op;
  const bool reduced = amg_reduced(h);
  if (reduced) STORM_TRY(op_reduced_require(op, "amg: the Jacobi smoother"));  // (the companion may have been dropped)
  if (!amg_residual_fused(h, op)) {
    ++c->n_amg_statement_sweeps;
    if (reduced) STORM_TRY(storm_hip_op_apply_reduced(op, L.alpha, L.beta, z_in, L.t));
    else STORM_TRY(storm_hip_op_apply(op, L.alpha, L.beta, z_in, L.t));
    STORM_TRY(storm_hip_axpbz(L.t, 1.0, r, -1.0, L.t));
    STORM_TRY(storm_hip_vmul(L.t, L.dinv, L.t));
    return storm_hip_axpbz(z_out, L.sigma, L.t, 1.0, z_in);
  }
  ++c->n_amg_fused_sweeps;
  SellArgs A{op->d_pack, op->d_slice_off, op->n_rows, op->uniform_width, op->xcd_group_sell, op->d_dict, op->dict_size,
             op->d_offs, op->offs_size, 0};
  if (reduced) A.pack = op->d_pack32, A.slice_off = op->d_slice_off32;
  const dim3 grid(blocks_for(op, op->n_slices)), block(kBlock);
  const bool nt = c->opt_nt != 0, xcd = op->xcd_group_sell != 0;
#define AMG_SWEEP_GO(NT_, XCD_)                                                                                                 \
  do {                                                                                                                          \
    if (reduced)                                                                                                                \
      hipLaunchKernelGGL((amg_jacobi_sweep_kernel<NT_, XCD_, Rec32>), grid, block, 0, c->stream, A, L.alpha, L.beta, L.sigma,  \
                         r->d, L.dinv->d, z_in->d, z_out->d, op->n_slices, c->api_done);                                        \
    else                                                                                                                        \
      hipLaunchKernelGGL((amg_jacobi_sweep_kernel<NT_, XCD_, Rec64>), grid, block, 0, c->stream, A, L.alpha, L.beta, L.sigma,  \
                         r->d, L.dinv->d, z_in->d, z_out->d, op->n_slices, c->api_done);                                        \
  } while (0)
  if (nt && xcd) AMG_SWEEP_GO(true, true);
  else if (nt) AMG_SWEEP_GO(true, false);
  else if (xcd) AMG_SWEEP_GO(false, true);
  else AMG_SWEEP_GO(false, false);
#undef AMG_SWEEP_GO
  HIP_TRY(hipGetLastError());
  return STORM_HIP_OK;
}

static int amg_cycle(const storm_hip_amg *h, size_t l, const storm_hip_vec *r, storm_hip_vec *z);

// THE CYCLE with the Jacobi smoother.  The iterate alternates between the caller's z and the level's e; a sweep from the zero
// guess into e puts the last of the nu - 1 pre-sweeps where the nu post-sweeps must start to end in z, for every nu.
static int amg_cycle_jacobi(const storm_hip_amg *h, size_t l, const storm_hip_vec *r, storm_hip_vec *z) {
  const storm_hip_amg::Level &L = h->levels[l];
  const storm_hip_amg::Level &N = h->levels[l + 1];
  const int nu = h->jacobi_sweeps;
  storm_hip_vec *buf[2] = {z, L.e};
  int at = 1;
  STORM_TRY(amg_jacobi_start(h, L, r, buf[at]));
  for (int k = 1; k < nu; ++k, at ^= 1) STORM_TRY(amg_jacobi_sweep(h, L, r, buf[at], buf[at ^ 1]));
  STORM_TRY(amg_residual(h, L, r, buf[at], L.t));
  STORM_TRY(amg_transfer(h, L.R, false, L.t, N.r));
  STORM_TRY(amg_cycle(h, l + 1, N.r, N.z));
  STORM_TRY(amg_transfer(h, L.P, true, N.z, buf[at]));
  for (int k = 0; k < nu; ++k, at ^= 1) STORM_TRY(amg_jacobi_sweep(h, L, r, buf[at], buf[at ^ 1]));
  return STORM_HIP_OK;  // (at == 0: the last sweep stored into z)
}

static int amg_cycle(const storm_hip_amg *h, size_t l, const storm_hip_vec *r, storm_hip_vec *z) {
  storm_hip_ctx *c = h->ctx;
  if ((int)l == h->tail.at) {  // option amg_tail: this level, everything below it and the way back up in one cooperative kernel
    bool taken = false;
    STORM_TRY(amg_tail_run(h, l, r, z, &taken));
    if (taken) return STORM_HIP_OK;  // (refused: this apply goes on with the launches)
  }
  if (l + 1 == h->levels.size()) {
    hipLaunchKernelGGL(amg_coarse_kernel, dim3((unsigned)((h->n_coarse + 3) / 4)), dim3(kBlock), 0, c->stream, h->d_ainv,
                       h->n_coarse, r->d, z->d, c->api_done);
    HIP_TRY(hipGetLastError());
    return STORM_HIP_OK;
  }
  if (h->smoother_kind == 1) return amg_cycle_jacobi(h, l, r, z);
  const storm_hip_amg::Level &L = h->levels[l];
  const storm_hip_amg::Level &N = h->levels[l + 1];
  STORM_TRY(storm_hip_cheb_apply(L.cheb, r, z));
  STORM_TRY(amg_residual(h, L, r, z, L.t));
  STORM_TRY(amg_transfer(h, L.R, false, L.t, N.r));
  STORM_TRY(amg_cycle(h, l + 1, N.r, N.z));
  STORM_TRY(amg_transfer(h, L.P, true, N.z, z));
  STORM_TRY(amg_residual(h, L, r, z, L.t));
  STORM_TRY(storm_hip_cheb_apply(L.cheb, L.t, L.e));
  if (l == 0 && h->nullspace) {  // z = z + e and the mean of z: one launch, or the statement and amg_mean_kernel
    if (c->opt_amg_fused != 0) {
      ++c->n_amg_fused_projections;
      return amg_mean(h, z, L.e, 1);
    }
    STORM_TRY(storm_hip_axpy(z, 1.0, L.e));
    return amg_mean(h, z, nullptr, 1);
  }
  return storm_hip_axpy(z, 1.0, L.e);
}

// The operator's fp64 records (and CSR tail) as CSR of A = beta I + alpha M: a_ii = beta + alpha (ext_i - sum w_ik) over the
// row's slots and tail entries in their order, a_ij = alpha sum w over the slots of column j; padding (weight 0) dropped.
// structural (an operator with a source map): a slot is real where its source id is >= 0, whatever its value.
int amg_decode(const storm_hip_op *op, double alpha, double beta, bool structural, std::vector<int64_t> *ptr, std::vector<int64_t> *col,
               std::vector<double> *val) {
  const int64_t n = op->n_rows, ns = op->n_slices;
  std::vector<int64_t> off((size_t)ns + 1, 0);
  HIP_TRY(hipStreamSynchronize(op->ctx->stream));
  HIP_TRY(hipMemcpy(off.data(), op->d_slice_off, sizeof(int64_t) * (size_t)(ns + 1), hipMemcpyDeviceToHost));
  std::vector<char> pack((size_t)std::max<int64_t>(off[(size_t)ns], 1));  // (the records end where the last offset says)
  if (off[(size_t)ns] > 0) HIP_TRY(hipMemcpy(pack.data(), op->d_pack, (size_t)off[(size_t)ns], hipMemcpyDeviceToHost));
  std::vector<int> trow((size_t)op->tail_rows), tcol((size_t)op->tail_nnz);
  std::vector<int64_t> tptr((size_t)op->tail_rows + 1, 0);
  std::vector<double> tval((size_t)op->tail_nnz);
  if (op->tail_rows > 0) {
    HIP_TRY(hipMemcpy(trow.data(), op->d_tail_row, sizeof(int) * trow.size(), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(tptr.data(), op->d_tail_ptr, sizeof(int64_t) * tptr.size(), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(tcol.data(), op->d_tail_col, sizeof(int) * tcol.size(), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(tval.data(), op->d_tail_val, sizeof(double) * tval.size(), hipMemcpyDeviceToHost));
  }
  std::vector<int> src;
  if (structural) {
    STORM_REQUIRE(op->d_src != nullptr, "amg: the operator (%lld rows) has no source map", (long long)n);
    src.resize((size_t)((off[(size_t)ns] - ns * kExtBytes) / (kSlotBytes / kWave)));
    if (!src.empty()) HIP_TRY(hipMemcpy(src.data(), op->d_src, sizeof(int) * src.size(), hipMemcpyDeviceToHost));
  }
  std::vector<int64_t> tail_of((size_t)n, -1);
  for (int64_t t = 0; t < op->tail_rows; ++t) {
    STORM_REQUIRE(trow[(size_t)t] >= 0 && trow[(size_t)t] < n, "amg_create: a tail row outside the operator");
    tail_of[(size_t)trow[(size_t)t]] = t;
  }
  ptr->assign((size_t)n + 1, 0);
  col->clear(), val->clear();
  std::vector<std::pair<int, double>> row;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t s = i / kWave;
    const int l = (int)(i % kWave);
    const char *rec = pack.data() + off[(size_t)s];
    const int W = (int)((off[(size_t)s + 1] - off[(size_t)s] - kExtBytes) / kSlotBytes);
    const int np2 = W >> 1;
    const double ext = reinterpret_cast<const double *>(rec)[l];
    const int *c_ = reinterpret_cast<const int *>(rec + kExtBytes);
    const double *v_ = reinterpret_cast<const double *>(rec + kExtBytes + (int64_t)W * (kWave * 4));
    const int *s_ = structural ? src.data() + (off[(size_t)s] - s * kExtBytes) / (kSlotBytes / kWave) : nullptr;
    row.clear();
    double sum = 0.0;
    for (int k = 0; k < W; ++k) {
      const int at = (k < 2 * np2) ? ((k >> 1) * kWave + l) * 2 + (k & 1) : np2 * 2 * kWave + l;
      if (structural ? s_[at] < 0 : v_[at] == 0.0) continue;
      STORM_REQUIRE(c_[at] >= 0 && c_[at] < n, "amg_create: column %d of row %lld outside the operator", c_[at], (long long)i);
      sum += v_[at];
      row.emplace_back(c_[at], v_[at]);
    }
    if (tail_of[(size_t)i] >= 0)
      for (int64_t k = tptr[(size_t)tail_of[(size_t)i]]; k < tptr[(size_t)tail_of[(size_t)i] + 1]; ++k) {
        if (!structural && tval[(size_t)k] == 0.0) continue;
        STORM_REQUIRE(tcol[(size_t)k] >= 0 && tcol[(size_t)k] < n, "amg_create: column %d of row %lld outside the operator",
                      tcol[(size_t)k], (long long)i);
        sum += tval[(size_t)k];
        row.emplace_back(tcol[(size_t)k], tval[(size_t)k]);
      }
    std::stable_sort(row.begin(), row.end(), [](const auto &a, const auto &b) { return a.first < b.first; });
    double diag = beta + alpha * (ext - sum);
    bool placed = false;
    for (size_t k = 0; k < row.size();) {
      double w = row[k].second;
      size_t e = k + 1;
      for (; e < row.size() && row[e].first == row[k].first; ++e) w += row[e].second;
      if (row[k].first == i) {  // (a slot on the row's own column multiplies x_i - x_i: it adds nothing)
        k = e;
        continue;
      }
      if (!placed && row[k].first > i) col->push_back(i), val->push_back(diag), placed = true;
      col->push_back(row[k].first), val->push_back(alpha * w);
      k = e;
    }
    if (!placed) col->push_back(i), val->push_back(diag);
    (*ptr)[(size_t)i + 1] = (int64_t)col->size();
  }
  return STORM_HIP_OK;
}

template <class T>
static int amg_upload(T **dst, const T *src, size_t count, int64_t *bytes) {
  const size_t nbytes = sizeof(T) * (count ? count : 1);
  hipError_t e = hipMalloc((void **)dst, nbytes);
  if (e != hipSuccess) STORM_FAIL(STORM_HIP_E_ALLOC, "amg_create: hipMalloc(%zu) failed: %s", nbytes, hipGetErrorString(e));
  if (count) HIP_TRY(hipMemcpy(*dst, src, sizeof(T) * count, hipMemcpyHostToDevice));
  *bytes += (int64_t)nbytes;
  return STORM_HIP_OK;
}

static int amg_upload_transfer(storm_hip_amg *h, const AmgCsr &M, storm_hip_amg::Transfer *T) {
  AmgTransferImage img;
  STORM_TRY(amg_pack_transfer(M, &img));
  T->n_rows = img.n_rows, T->n_slices = img.n_slices;
  STORM_TRY(amg_upload(&T->d_off, img.off.data(), img.off.size(), &h->device_bytes));
  STORM_TRY(amg_upload(&T->d_pack, img.pack.data(), img.pack.size(), &h->device_bytes));
  h->transfer_slots += img.slots, h->transfer_nnz += img.nnz;
  return STORM_HIP_OK;
}

int amg_build_device(storm_hip_amg *h, storm_hip_op *op0) {
  storm_hip_ctx *c = h->ctx;
  const storm_hip_amg_params &p = h->hier->params;
  const size_t nl = h->hier->levels.size();
  h->levels.resize(nl);
  for (size_t l = 0; l < nl; ++l) {
    const AmgHostLevel &H = h->hier->levels[l];
    storm_hip_amg::Level &L = h->levels[l];
    L.n = H.A.n_rows;
    if (l > 0) {
      STORM_TRY(storm_hip_vec_create(c, L.n, 0, &L.r));
      STORM_TRY(storm_hip_vec_create(c, L.n, 0, &L.z));
      h->device_bytes += 2 * (int64_t)L.r->bytes;
    }
    if (l + 1 == nl) break;  // the coarsest level is its dense inverse
    if (l == 0) {
      L.op = op0, L.alpha = h->alpha, L.beta = h->beta;
    } else {
      std::vector<int64_t> col(H.A.col.begin(), H.A.col.end());
      STORM_TRY(op_create_csr_fp64(c, L.n, H.A.ptr.data(), col.data(), H.A.val.data(), h->hier->structural, &L.own_op));
      L.op = L.own_op, L.alpha = 1.0, L.beta = 0.0;
      h->device_bytes += L.own_op->device_bytes;
    }
    storm_hip_op *mine = l == 0 ? op0 : L.own_op;
    STORM_TRY(storm_hip_vec_create(c, L.n, 0, &L.dinv));
    STORM_TRY(storm_hip_vec_create(c, L.n, 0, &L.t));
    STORM_TRY(storm_hip_vec_create(c, L.n, 0, &L.e));
    const bool jacobi = h->smoother_kind == 1;
    h->device_bytes += (jacobi ? 3 : 6) * (int64_t)L.t->bytes;  // ... and the Chebyshev smoother's three
    STORM_TRY(storm_hip_op_get_diagonal(L.op, L.alpha, L.beta, 1, L.dinv));
    double lmax = 0.0;
    if (p.reduced_records) {
      const int64_t before = mine->device_bytes;
      STORM_TRY(storm_hip_op_build_reduced(mine));
      if (l > 0) h->device_bytes += mine->device_bytes - before;
      STORM_TRY(storm_hip_op_gershgorin_reduced(L.op, L.alpha, L.beta, L.dinv, &lmax));
      if (!jacobi)
        STORM_TRY(storm_hip_cheb_create_reduced(L.op, L.alpha, L.beta, L.dinv, p.smoother_degree, lmax / p.smoother_ratio, lmax, &L.cheb));
    } else {
      STORM_TRY(storm_hip_op_gershgorin(L.op, L.alpha, L.beta, L.dinv, &lmax));
      if (!jacobi)
        STORM_TRY(storm_hip_cheb_create(L.op, L.alpha, L.beta, L.dinv, p.smoother_degree, lmax / p.smoother_ratio, lmax, &L.cheb));
    }
    L.lmax = lmax;
    if (jacobi) {
      STORM_REQUIRE(std::isfinite(lmax) && lmax > 0.0, "amg_create_smoother: Gershgorin's bound of level %d is %g", (int)l, lmax);
      L.sigma = 2.0 * h->jacobi_omega / lmax;
    }
    STORM_TRY(amg_upload_transfer(h, H.P, &L.P));
    STORM_TRY(amg_upload_transfer(h, H.R, &L.R));
  }
  h->n_coarse = h->hier->levels.back().A.n_rows;
  STORM_TRY(amg_upload(&h->d_ainv, h->hier->ainv.data(), h->hier->ainv.size(), &h->device_bytes));
  if (h->hier->nullspace) {  // the projected residual, the two means, the mean's own ticket buffers (counters start at 0)
    const int64_t n = h->levels[0].n;
    const size_t nb = (size_t)stream_blocks(n), ng = (nb + kTicketGroup - 1) / kTicketGroup;
    h->nullspace = 1;
    STORM_TRY(storm_hip_vec_create(c, n, 0, &h->rp));
    h->device_bytes += (int64_t)h->rp->bytes;
    const std::vector<double> zeros(std::max(nb, (size_t)2), 0.0);
    const std::vector<int> zero_cnt((1 + ng) * kTicketStride, 0);
    STORM_TRY(amg_upload(&h->d_mu, zeros.data(), 2, &h->device_bytes));
    STORM_TRY(amg_upload(&h->d_mean_part1, zeros.data(), nb, &h->device_bytes));
    STORM_TRY(amg_upload(&h->d_mean_part2, zeros.data(), ng, &h->device_bytes));
    STORM_TRY(amg_upload(&h->d_mean_cnt, zero_cnt.data(), zero_cnt.size(), &h->device_bytes));
  }
  return STORM_HIP_OK;
}

int amg_create_checks(const storm_hip_op *op, double alpha, double beta, const char *who) {
  STORM_REQUIRE(std::isfinite(alpha) && std::isfinite(beta), "%s: alpha and beta must be finite", who);
  if (op->pair != 0 || op->dict_size > 0 || op->offs_size > 0 || op->d_bnd_pack != nullptr)
    STORM_FAIL(STORM_HIP_E_UNSUPPORTED, "%s: the operator is on compact records (a value / offset dictionary, paired rows "
                                        "or a mixed operator); the multigrid preconditioner reads fp64 records (what any mesh "
                                        "gets; a box built with option spmv_dict = 0)", who);
  if (op->halo.n_nbrs > 0 || op->n_halo > 0 || op->ctx->comm != nullptr)
    STORM_FAIL(STORM_HIP_E_UNSUPPORTED, "%s: the multigrid preconditioner is single-rank (the operator has a halo plan or "
                                        "halo columns, or the context a communicator)", who);
  STORM_REQUIRE(op->n_rows >= 1, "%s: the operator has no rows", who);
  return STORM_HIP_OK;
}

}  // namespace storm

using namespace storm;

extern "C" {

// The Jacobi scale s_i = 1 / a_ii must exist: the first zero or non-finite diagonal of a CSR level operator is refused.
static int amg_jacobi_diagonal_check(int level, int64_t n, const int64_t *ptr, const int64_t *col64, const int *col32,
                                     const double *val) {
  for (int64_t i = 0; i < n; ++i) {
    double d = 0.0;  // (a row without a stored diagonal has a zero one)
    for (int64_t k = ptr[i]; k < ptr[i + 1]; ++k)
      if ((col64 ? col64[k] : (int64_t)col32[k]) == i) d += val[k];
    STORM_REQUIRE(d != 0.0 && std::isfinite(d), "amg_create_smoother: the diagonal of level %d is %g in row %lld; the Jacobi "
                  "smoother divides by it", level, d, (long long)i);
  }
  return STORM_HIP_OK;
}

// storm_hip_amg_create, and with `smoother` of kind 1 storm_hip_amg_create_smoother's Jacobi object
static int amg_create_plain(storm_hip_op *op, double alpha, double beta, const storm_hip_amg_params *params,
                            const storm_hip_amg_smoother *smoother, const char *who, storm_hip_amg **out) {
  STORM_TRY(amg_create_checks(op, alpha, beta, who));
  storm_hip_ctx *c = op->ctx;
  HIP_TRY(hipSetDevice(c->device));
  STORM_TRY(lazy_sync(c));
  std::vector<int64_t> ptr, col;
  std::vector<double> val;
  STORM_TRY(amg_decode(op, alpha, beta, false, &ptr, &col, &val));
  const bool jacobi = smoother != nullptr && smoother->kind == 1;
  if (jacobi) STORM_TRY(amg_jacobi_diagonal_check(0, op->n_rows, ptr.data(), col.data(), nullptr, val.data()));
  storm_hip_amg_hierarchy *hier = nullptr;
  STORM_TRY(storm_hip_amg_setup_csr(op->n_rows, ptr.data(), col.data(), val.data(), params, &hier));
  for (size_t l = 1; jacobi && l + 1 < hier->levels.size(); ++l) {
    const AmgCsr &A = hier->levels[l].A;
    const int st = amg_jacobi_diagonal_check((int)l, A.n_rows, A.ptr.data(), nullptr, A.col.data(), A.val.data());
    if (st != STORM_HIP_OK) {
      (void)storm_hip_amg_hierarchy_destroy(hier);
      return st;
    }
  }
  storm_hip_amg *h = new storm_hip_amg();
  h->ctx = c, h->op = op, h->alpha = alpha, h->beta = beta, h->hier = hier;
  if (jacobi) h->smoother_kind = 1, h->jacobi_sweeps = smoother->sweeps, h->jacobi_omega = smoother->omega;
  const auto t0 = std::chrono::steady_clock::now();
  const int st = amg_build_device(h, op);
  if (st != STORM_HIP_OK) {
    (void)storm_hip_amg_destroy(h);
    return st;
  }
  h->upload_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  *out = h;
  return STORM_HIP_OK;
}

int storm_hip_amg_create(storm_hip_op *op, double alpha, double beta, const storm_hip_amg_params *params, storm_hip_amg **out) {
  STORM_REQUIRE(op && out, "amg_create: null argument");
  *out = nullptr;
  return amg_create_plain(op, alpha, beta, params, nullptr, "amg_create", out);
}

void storm_hip_amg_smoother_default(storm_hip_amg_smoother *s) {
  if (!s) return;
  s->kind = 1, s->sweeps = 2, s->omega = 2.0 / 3.0;
}

int storm_hip_amg_create_smoother(storm_hip_op *op, double alpha, double beta, const storm_hip_amg_params *params,
                                  const storm_hip_amg_smoother *smoother, storm_hip_amg **out) {
  STORM_REQUIRE(smoother && out, "amg_create_smoother: null argument");
  *out = nullptr;
  // (the smoother is judged before the operator is looked at)
  STORM_REQUIRE(smoother->kind == 0 || smoother->kind == 1, "amg_create_smoother: kind %d (0: Chebyshev, 1: Jacobi)", smoother->kind);
  if (smoother->kind == 1) {
    STORM_REQUIRE(smoother->sweeps >= 1 && smoother->sweeps <= 16, "amg_create_smoother: sweeps %d (1 .. 16)", smoother->sweeps);
    STORM_REQUIRE(smoother->omega > 0.0 && smoother->omega <= 1.0, "amg_create_smoother: omega %g outside (0, 1]", smoother->omega);
  }
  STORM_REQUIRE(op, "amg_create_smoother: null argument");
  return amg_create_plain(op, alpha, beta, params, smoother, "amg_create_smoother", out);
}

int storm_hip_amg_smooth(const storm_hip_amg *h, int level, const storm_hip_vec *r, const storm_hip_vec *z_in, storm_hip_vec *z_out) {
  STORM_REQUIRE(h && r && z_in && z_out, "amg_smooth: null argument");
  if (h->smoother_kind != 1)
    STORM_FAIL(STORM_HIP_E_UNSUPPORTED, "amg_smooth: the object has the Chebyshev smoother (a sweep belongs to an object made by "
                                        "storm_hip_amg_create_smoother with kind 1)");
  STORM_REQUIRE(level >= 0 && level + 1 < (int)h->levels.size(), "amg_smooth: level %d has no smoother (%d levels)", level,
                (int)h->levels.size());
  const storm_hip_amg::Level &L = h->levels[(size_t)level];
  STORM_REQUIRE(r->ctx == h->ctx && z_in->ctx == h->ctx && z_out->ctx == h->ctx, "amg_smooth: context mismatch");
  STORM_REQUIRE(z_out != z_in && z_out->d != z_in->d && z_out != r && z_out->d != r->d, "amg_smooth: z_out must not alias z_in or r");
  STORM_REQUIRE(r->n_owned == L.n && z_in->n_owned == L.n && z_out->n_owned == L.n,
                "amg_smooth: level %d has %lld rows; the vectors have %lld, %lld and %lld", level, (long long)L.n,
                (long long)r->n_owned, (long long)z_in->n_owned, (long long)z_out->n_owned);
  storm_hip_ctx *c = h->ctx;
  HIP_TRY(hipSetDevice(c->device));
  STORM_TRY(lazy_sync(c));
  struct Depth {  // (the statements go out as they are issued, as in storm_hip_amg_apply)
    storm_hip_ctx *c;
    explicit Depth(storm_hip_ctx *c_) : c(c_) { ++c->callback_depth; }
    ~Depth() { --c->callback_depth; }
  } depth(c);
  return amg_jacobi_sweep(h, L, r, z_in, z_out);
}

int storm_hip_amg_destroy(storm_hip_amg *h) {
  if (!h) return STORM_HIP_OK;
  for (auto &L : h->levels) {
    (void)storm_hip_cheb_destroy(L.cheb);
    storm_hip_vec *vs[5] = {L.dinv, L.r, L.z, L.t, L.e};
    for (storm_hip_vec *v : vs) (void)storm_hip_vec_destroy(v);
    (void)hipFree(L.P.d_off), (void)hipFree(L.P.d_pack), (void)hipFree(L.R.d_off), (void)hipFree(L.R.d_pack);
    (void)storm_hip_op_destroy(L.own_op);
  }
  (void)hipFree(h->d_ainv);
  (void)storm_hip_vec_destroy(h->rp);
  (void)hipFree(h->d_mu), (void)hipFree(h->d_mean_part1), (void)hipFree(h->d_mean_part2), (void)hipFree(h->d_mean_cnt);
  amg_refresh_free(h);
  amg_tail_free(h);
  (void)storm_hip_amg_hierarchy_destroy(h->hier);
  delete h;
  return STORM_HIP_OK;
}

int storm_hip_amg_apply(const storm_hip_amg *h, const storm_hip_vec *r, storm_hip_vec *z) {
  STORM_REQUIRE(h && r && z, "amg_apply: null argument");
  STORM_REQUIRE(r->ctx == h->ctx && z->ctx == h->ctx, "amg_apply: context mismatch");
  STORM_REQUIRE(z != r && z->d != r->d, "amg_apply: z must not alias r");
  STORM_REQUIRE(r->n_owned == h->op->n_rows && z->n_owned == h->op->n_rows, "amg_apply: operator has %lld rows, r %lld, z %lld",
                (long long)h->op->n_rows, (long long)r->n_owned, (long long)z->n_owned);
  STORM_REQUIRE(!h->invalid, "amg_apply: the last storm_hip_amg_refresh of this object failed; it is invalid until one succeeds");
  storm_hip_ctx *c = h->ctx;
  HIP_TRY(hipSetDevice(c->device));
  STORM_TRY(lazy_sync(c));
  // the library calls of the cycle go out as they are issued (no lazy_statements hold-back), predicated on api_done
  struct Depth {
    storm_hip_ctx *c;
    explicit Depth(storm_hip_ctx *c_) : c(c_) { ++c->callback_depth; }
    ~Depth() { --c->callback_depth; }
  } depth(c);
  ++c->n_amg_applies;
  h->tail.at = amg_tail_choose(h);
  if (!h->nullspace) return amg_cycle(h, 0, r, z);
  // B = Pi V Pi: rp = r - mean(r); z = V(rp), whose closing statement leaves mean(z) in the second slot; z = z - mean(z)
  c->n_amg_projections += 2;
  STORM_TRY(amg_mean(h, const_cast<storm_hip_vec *>(r), nullptr, 0));  // (reads r only)
  STORM_TRY(amg_shift(h, r, 0, h->rp));
  STORM_TRY(amg_cycle(h, 0, h->rp, z));
  if (h->levels.size() == 1) STORM_TRY(amg_mean(h, z, nullptr, 1));  // one level: z = Ainv rp has no closing statement
  return amg_shift(h, z, 1, z);
}

int storm_hip_amg_project(const storm_hip_amg *h, storm_hip_vec *v) {
  STORM_REQUIRE(h && v, "amg_project: null argument");
  if (!h->nullspace)
    STORM_FAIL(STORM_HIP_E_UNSUPPORTED, "amg_project: the object was not created by storm_hip_amg_create_nullspace (it has no "
                                        "null space to project out)");
  STORM_REQUIRE(v->ctx == h->ctx, "amg_project: context mismatch");
  STORM_REQUIRE(v->n_owned == h->op->n_rows, "amg_project: operator has %lld rows, v %lld", (long long)h->op->n_rows, (long long)v->n_owned);
  storm_hip_ctx *c = h->ctx;
  HIP_TRY(hipSetDevice(c->device));
  STORM_TRY(lazy_sync(c));
  ++c->n_amg_projections;
  STORM_TRY(amg_mean(h, v, nullptr, 0));
  return amg_shift(h, v, 0, v);
}

static int amg_level_check(const storm_hip_amg *h, int level, const storm_hip_vec *fine, const storm_hip_vec *coarse, const char *who) {
  STORM_REQUIRE(level >= 0 && level + 1 < (int)h->levels.size(), "%s: level %d has no transfer (%d levels)", who, level,
                (int)h->levels.size());
  STORM_REQUIRE(fine->ctx == h->ctx && coarse->ctx == h->ctx, "%s: context mismatch", who);
  STORM_REQUIRE(fine != coarse && fine->d != coarse->d, "%s: the vectors must not alias", who);
  STORM_REQUIRE(fine->n_owned == h->levels[(size_t)level].n && coarse->n_owned == h->levels[(size_t)level + 1].n,
                "%s: level %d has %lld rows and the next %lld; the vectors have %lld and %lld", who, level,
                (long long)h->levels[(size_t)level].n, (long long)h->levels[(size_t)level + 1].n, (long long)fine->n_owned,
                (long long)coarse->n_owned);
  HIP_TRY(hipSetDevice(h->ctx->device));
  return lazy_sync(h->ctx);
}

int storm_hip_amg_restrict(const storm_hip_amg *h, int level, const storm_hip_vec *fine, storm_hip_vec *coarse) {
  STORM_REQUIRE(h && fine && coarse, "amg_restrict: null argument");
  STORM_TRY(amg_level_check(h, level, fine, coarse, "amg_restrict"));
  return amg_transfer(h, h->levels[(size_t)level].R, false, fine, coarse);
}

int storm_hip_amg_prolong_add(const storm_hip_amg *h, int level, const storm_hip_vec *coarse, storm_hip_vec *fine) {
  STORM_REQUIRE(h && fine && coarse, "amg_prolong_add: null argument");
  STORM_TRY(amg_level_check(h, level, fine, coarse, "amg_prolong_add"));
  return amg_transfer(h, h->levels[(size_t)level].P, true, coarse, fine);
}

int storm_hip_amg_coarse_solve(const storm_hip_amg *h, const storm_hip_vec *r, storm_hip_vec *z) {
  STORM_REQUIRE(h && r && z, "amg_coarse_solve: null argument");
  STORM_REQUIRE(r->ctx == h->ctx && z->ctx == h->ctx, "amg_coarse_solve: context mismatch");
  STORM_REQUIRE(z != r && z->d != r->d, "amg_coarse_solve: z must not alias r");
  STORM_REQUIRE(r->n_owned == h->n_coarse && z->n_owned == h->n_coarse, "amg_coarse_solve: the coarsest level has %lld rows, r %lld, z %lld",
                (long long)h->n_coarse, (long long)r->n_owned, (long long)z->n_owned);
  HIP_TRY(hipSetDevice(h->ctx->device));
  STORM_TRY(lazy_sync(h->ctx));
  h->tail.at = -1;
  return amg_cycle(h, h->levels.size() - 1, r, z);
}

int storm_hip_amg_get(const storm_hip_amg *h, const char *key, double *value) {
  STORM_REQUIRE(h && key && value, "amg_get: null argument");
  if (!strcmp(key, "device_bytes")) *value = (double)h->device_bytes;
  else if (!strcmp(key, "transfer_padding"))
    *value = h->transfer_slots > 0 ? 1.0 - (double)h->transfer_nnz / (double)h->transfer_slots : 0.0;
  else if (!strcmp(key, "upload_seconds")) *value = h->upload_seconds;
  else if (!strcmp(key, "refresh_bytes")) *value = (double)h->refresh_bytes;
  else if (!strcmp(key, "refreshable")) *value = h->refresh.empty() ? 0.0 : 1.0;
  else if (!strcmp(key, "nullspace")) *value = h->nullspace ? 1.0 : 0.0;
  else if (!strcmp(key, "smoother_degree")) *value = (double)h->hier->params.smoother_degree;
  else if (!strcmp(key, "reduced")) *value = (double)h->hier->params.reduced_records;
  else if (!strcmp(key, "smoother_kind")) *value = (double)h->smoother_kind;
  else if (!strcmp(key, "jacobi_sweeps")) *value = (double)h->jacobi_sweeps;
  else if (!strcmp(key, "jacobi_omega")) *value = h->jacobi_omega;
  else if (!strncmp(key, "jacobi_sigma_", 13)) {
    char *end = nullptr;
    const long level = strtol(key + 13, &end, 10);
    STORM_REQUIRE(h->smoother_kind == 1 && end != key + 13 && *end == '\0' && level >= 0 && level + 1 < (long)h->levels.size(),
                  "amg_get: '%s': no Jacobi smoother on that level (%d levels)", key, (int)h->levels.size());
    *value = h->levels[(size_t)level].sigma;
  }
  else {
    bool known = false;  // tail_level, tail_blocks, tail_barriers (amg_tail.hip)
    STORM_TRY(amg_tail_get(h, key, value, &known));
    if (!known) return storm_hip_amg_hierarchy_get(h->hier, key, value);
  }
  return STORM_HIP_OK;
}

int storm_hip_amg_get_hierarchy(const storm_hip_amg *h, const storm_hip_amg_hierarchy **out) {
  STORM_REQUIRE(h && out, "amg_get_hierarchy: null argument");
  *out = h->hier;
  return STORM_HIP_OK;
}

}  // extern "C"
