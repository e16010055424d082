// Block vectors: k interleaved columns over n cells in one storm_hip_vec (element (i, j) at i k + j, the layout of the
// reference's Field<Mesh, Index, Value, NumVars>, Feathers/Field.hpp:56-79), 1 <= k <= 8.  Column copies, the per-column
// dot and axpy, and k independent CG solves A x_j = b_j (SolverCg.hpp:54-126 per column, the convergence rule of
// Solver.hpp:116-147 per column) whose operator apply streams the records once for all columns (spmv_block.hip).
//
// The batched CG is a throughput loop only.  Every column has its own gamma, <p,z>, alpha, beta, residual norms,
// iteration count and done / converged flags in the context's scalar slab (kColStride doubles per column); the
// SolverState's own iteration counter counts the block's iterations and its `done` means "every column done" -- that
// is the word the host polls in the pinned ring, `check_lag` iterations behind, as in the other loops.  Per iteration:
//   the block apply with per-wave partials of <p_j, z_j>, folded by reduce_finish_kernel, whose epilogue forms alpha_j;
//   block_cg_r_kernel:  r_j -= alpha_j z_j, <r_j, r_j> finished in the kernel by tickets (ticket_device.hpp), whose last
//                       block runs every column's scalar step and convergence rule;
//   block_cg_xp_kernel: x_j += alpha_j p_j; p_j = r_j + beta_j p_j.
// A column that is done is frozen: its x, r and p keep their values (no statement is applied to them any more) and its
// iteration count stays.
// A thread owns whole cells, so column j's sums run over the cells in an order that depends neither on j nor on what
// the other columns hold: a column's solve is the same bits wherever in the block it sits.
#include <algorithm>
#include <cstddef>
#include <vector>

#include "common.hpp"
#include "blas1_device.hpp"
#include "solver_device.hpp"
#include "ticket_device.hpp"

namespace storm {

constexpr int kMaxCols = 8;
constexpr int kColStride = 16;  // slab doubles per column
enum ColSlot { C_GAMMA = 0, C_PZ, C_BETA, C_ALPHA, C_INITIAL, C_ABS, C_REL, C_ITER, C_DONE, C_CONV };
static_assert(kMaxCols * kColStride <= kSlab, "the columns' scalars live in the slab");

// Streaming shape: a block owns kCellsPerThread * 256 = 2048 consecutive cells (the rows of a BLAS-1 block), a thread
// every 256th of them, U cells' loads in flight at a time.  The longest addition chain of a column's sum is 8 (thread)
// + 6 + 2 (block) + 6 + ceil(groups / 64) + 6 (tickets): below the 64 + ceil(blocks / 256) of the one-column kernels.
constexpr int kCellsPerThread = 8;
constexpr int kBlockCells = kBlock * kCellsPerThread;
template <int K>
constexpr int cells_in_flight() { return K <= 2 ? 4 : (K <= 4 ? 2 : 1); }
// Non-temporal accesses only for one column: with k > 1 a wave's instruction touches 16 B out of every 8 k (a lane owns a
// whole cell), and with non-temporal partial lines the batched CG at k = 4 took 759 instead of 455 us per
// column-iteration at 256^3 (profiles/r16_block_nt_ab.json, r16_block_bench_nt.json).
static inline int block_nt(const storm_hip_ctx *c, int64_t n, int k) { return k == 1 ? stream_nt(c, n) : 0; }
static inline int block_blocks(int64_t n) {
  int64_t b = (n + kBlockCells - 1) / kBlockCells;
  return (int)std::max<int64_t>(1, std::min<int64_t>(b, kMaxStreamBlocks));
}

template <int K, class NT>
__device__ __forceinline__ void ldk(const double *__restrict__ p, double (&v)[K], NT nt) {
  if constexpr (K % 2 == 0) {
#pragma unroll
    for (int q = 0; q < K / 2; ++q) {
      const double2v t = ld2(reinterpret_cast<const double2v *>(p) + q, nt);
      v[2 * q] = t.x, v[2 * q + 1] = t.y;
    }
  } else {
#pragma unroll
    for (int j = 0; j < K; ++j) v[j] = NT::value ? __builtin_nontemporal_load(p + j) : p[j];
  }
}
template <int K, class NT>
__device__ __forceinline__ void stk(double *__restrict__ p, const double (&v)[K], NT nt) {
  if constexpr (K % 2 == 0) {
#pragma unroll
    for (int q = 0; q < K / 2; ++q) st2(reinterpret_cast<double2v *>(p) + q, double2v{v[2 * q], v[2 * q + 1]}, nt);
  } else {
#pragma unroll
    for (int j = 0; j < K; ++j) {
      if (NT::value) __builtin_nontemporal_store(v[j], p + j);
      else p[j] = v[j];
    }
  }
}

// f(i, u) for the cells of block bx, U at a time: `load` first for all U, then `use`.
#define STORM_CELL_LOOP(n, bx, U, i, u, LOAD, USE)                                                         \
  for (int64_t c0_ = (int64_t)(bx) * kBlockCells; c0_ < (n); c0_ += (int64_t)gridDim.x * kBlockCells) {    \
    _Pragma("unroll") for (int u0_ = 0; u0_ < kCellsPerThread; u0_ += (U)) {                               \
      _Pragma("unroll") for (int u = 0; u < (U); ++u) {                                                    \
        const int64_t i = c0_ + (int64_t)(u0_ + u) * kBlock + threadIdx.x;                                 \
        if (i < (n)) { LOAD }                                                                              \
      }                                                                                                    \
      _Pragma("unroll") for (int u = 0; u < (U); ++u) {                                                    \
        const int64_t i = c0_ + (int64_t)(u0_ + u) * kBlock + threadIdx.x;                                 \
        if (i < (n)) { USE }                                                                               \
      }                                                                                                    \
    }                                                                                                      \
  }

// ---- column copies ------------------------------------------------------------------------------------------------
template <bool GET>
__global__ __launch_bounds__(kBlock) void block_column_kernel(int64_t n, int k, int j, double *__restrict__ X,
                                                              double *__restrict__ v, const int *done) {
  if (done && *done) return;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    if (GET) v[i] = X[i * k + j];
    else X[i * k + j] = v[i];
  }
}

// ---- per-column dot and axpy --------------------------------------------------------------------------------------
// partials[j * gridDim.x + block] = the block's share of <A_j, B_j>
template <int K>
__global__ __launch_bounds__(kBlock) void block_dot_kernel(int64_t n, const double *__restrict__ A,
                                                           const double *__restrict__ B, double *__restrict__ partials,
                                                           const int *done, int nt) {
  if (done && *done) return;
  __shared__ double lds[K][4];
  constexpr int U = cells_in_flight<K>();
  double acc[K];
#pragma unroll
  for (int j = 0; j < K; ++j) acc[j] = 0.0;
  nt_dispatch(nt, [&](auto nt) {
    double a[U][K], b[U][K];
    STORM_CELL_LOOP(n, blockIdx.x, U, i, u, ldk<K>(A + i * K, a[u], nt); ldk<K>(B + i * K, b[u], nt);, {
      _Pragma("unroll") for (int j = 0; j < K; ++j) acc[j] += a[u][j] * b[u][j];
    })
  });
  double sums[K];
  block_sum_multi<K>(acc, lds, sums);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int j = 0; j < K; ++j) partials[(int64_t)j * gridDim.x + blockIdx.x] = sums[j];
  }
}

struct ColCoefs {
  double a[kMaxCols];
};
// Y_j = fma(a[j], X_j, Y_j)
template <int K>
__global__ __launch_bounds__(kBlock) void block_axpy_kernel(int64_t n, double *__restrict__ Y, ColCoefs cf,
                                                            const double *__restrict__ X, const int *done, int nt) {
  if (done && *done) return;
  constexpr int U = cells_in_flight<K>();
  nt_dispatch(nt, [&](auto nt) {
    double x[U][K], y[U][K];
    STORM_CELL_LOOP(n, blockIdx.x, U, i, u, ldk<K>(X + i * K, x[u], nt); ldk<K>(Y + i * K, y[u], nt);, {
      _Pragma("unroll") for (int j = 0; j < K; ++j) y[u][j] += cf.a[j] * x[u][j];
      stk<K>(Y + i * K, y[u], nt);
    })
  });
}

// ---- the batched CG ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double *col_slots(SolverState *st, int j) { return st->s + j * kColStride; }

// Tell the host about block iteration st->iteration (advance() / begin() of solver_device.hpp, for the whole block).
__device__ inline void block_post(SolverState *st, bool all_done, bool at_begin) {
  if (all_done) st->done = 1;
  if (!st->done_ring) return;
  if (at_begin) {
    if (all_done)  // no iteration will run: every poll must see it
      for (int i = 0; i < kStateRing; ++i)
        __hip_atomic_store(st->done_ring + i, ring_word(st->ring_gen, kRingIterMask, true), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    return;
  }
  __hip_atomic_store(st->done_ring + (st->iteration - 1) % kStateRing,
                     ring_word(st->ring_gen, (unsigned long long)st->iteration, st->done != 0), __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_SYSTEM);
}
// After init(), per column: Solver.hpp:122-128; gamma = <r, r>, SolverCg.hpp:82, 85.
__device__ inline void block_begin(SolverState *st, int k, const double *rr) {
  bool all = true;
  for (int j = 0; j < k; ++j) {
    double *s = col_slots(st, j);
    s[C_GAMMA] = rr[j];
    const double err = sqrt(rr[j]);
    s[C_INITIAL] = err, s[C_ABS] = err, s[C_REL] = 0.0, s[C_ITER] = 0.0, s[C_DONE] = 0.0, s[C_CONV] = 0.0;
    if (st->history) st->history[(long long)j * (st->num_iterations + 1)] = err;
    if (st->abs_tol > 0.0 && err < st->abs_tol) s[C_CONV] = 1.0, s[C_DONE] = 1.0;
    if (st->num_iterations <= 0) s[C_DONE] = 1.0;
    all &= s[C_DONE] != 0.0;
  }
  st->iteration = 0, st->converged = 0, st->done = 0;
  block_post(st, all, true);
}
// The scalar step of SolverCg.hpp:110-125 and the loop body of Solver.hpp:132-140, for every column still running.
__device__ inline void block_advance(SolverState *st, int k, const double *rr) {
  bool all = true;
  for (int j = 0; j < k; ++j) {
    double *s = col_slots(st, j);
    if (s[C_DONE] == 0.0) {
      const double gamma_bar = s[C_GAMMA];
      s[C_GAMMA] = rr[j];
      s[C_BETA] = safe_divide(s[C_GAMMA], gamma_bar);
      const double err = sqrt(s[C_GAMMA]);
      s[C_ABS] = err;
      s[C_REL] = err / s[C_INITIAL];
      bool conv = false;
      conv |= (st->abs_tol > 0.0) && (s[C_ABS] < st->abs_tol);
      conv |= (st->rel_tol > 0.0) && (s[C_REL] < st->rel_tol);
      s[C_ITER] += 1.0;
      const long long it = (long long)s[C_ITER];
      if (st->history) st->history[(long long)j * (st->num_iterations + 1) + it] = err;
      if (conv) s[C_CONV] = 1.0;
      if (conv || it >= st->num_iterations) s[C_DONE] = 1.0;
    }
    all &= s[C_DONE] != 0.0;
  }
  st->iteration += 1;
  block_post(st, all, false);
}

// The epilogue of reduce_finish_kernel behind the fold of <p_j, z_j>: alpha_j = safe_divide(gamma_j, <p_j, z_j>)
// (SolverCg.hpp:97) for the columns still running.
struct BlockAlphaEpi {
  SolverState *st;
  int k;
  __device__ void operator()() const {
    for (int j = 0; j < k; ++j) {
      double *s = col_slots(st, j);
      if (s[C_DONE] == 0.0) s[C_ALPHA] = safe_divide(s[C_GAMMA], s[C_PZ]);
    }
  }
};

// INIT: r <<= b - r (Operator.hpp:98), p <<= r (SolverCg.hpp:81), <r_j, r_j>, block_begin.
// else: r_j -= alpha_j z_j for the running columns (SolverCg.hpp:99: fma(-alpha, z, r)), <r_j, r_j>, block_advance.
template <int K, bool INIT>
__global__ __launch_bounds__(kBlock) void block_cg_r_kernel(int64_t n, SolverState *st, double *__restrict__ R,
                                                            const double *__restrict__ ZB, double *__restrict__ P,
                                                            TicketArgs tickets, int nt) {
  if (!INIT && st->done) return;
  __shared__ double lds[K][4];
  constexpr int U = cells_in_flight<K>();
  double alpha[K], acc[K];
  bool run[K];
#pragma unroll
  for (int j = 0; j < K; ++j) {
    acc[j] = 0.0;
    run[j] = INIT || col_slots(st, j)[C_DONE] == 0.0;
    alpha[j] = INIT ? 0.0 : col_slots(st, j)[C_ALPHA];
  }
  nt_dispatch(nt, [&](auto nt) {
    double r[U][K], z[U][K];
    STORM_CELL_LOOP(n, blockIdx.x, U, i, u, ldk<K>(R + i * K, r[u], nt); ldk<K>(ZB + i * K, z[u], nt);, {
      _Pragma("unroll") for (int j = 0; j < K; ++j) {
        if (INIT) {
          r[u][j] = z[u][j] - r[u][j];
          acc[j] += r[u][j] * r[u][j];
        } else if (run[j]) {
          r[u][j] -= alpha[j] * z[u][j];
          acc[j] += r[u][j] * r[u][j];
        }
      }
      stk<K>(R + i * K, r[u], nt);
      if (INIT) stk<K>(P + i * K, r[u], nt);
    })
  });
  double mine[K], total[K];
  block_sum_multi<K>(acc, lds, mine);
  if (threadIdx.x >= kWave) return;
  if (ticket_reduce_wave0<K>(tickets, mine, K, blockIdx.x, gridDim.x, total)) {
    if (threadIdx.x == 0) {
      if (INIT) block_begin(st, K, total);
      else block_advance(st, K, total);
    }
  }
}

// x_j += alpha_j p_j (SolverCg.hpp:98: fma(alpha, p, x)) for the columns that ran block iteration my_iteration;
// p_j = r_j + beta_j p_j (:123: fma(beta, p, r)) for those of them that go on.
template <int K>
__global__ __launch_bounds__(kBlock) void block_cg_xp_kernel(int64_t n, const SolverState *st, long long my_iteration,
                                                             double *__restrict__ X, double *__restrict__ P,
                                                             const double *__restrict__ R, int nt) {
  if (st->iteration < my_iteration) return;  // enqueued past the last column's end: this iteration never ran
  constexpr int U = cells_in_flight<K>();
  double alpha[K], beta[K];
  bool ran[K], go_on[K];
  bool any_p = false;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const double *s = st->s + j * kColStride;
    ran[j] = s[C_ITER] >= (double)my_iteration;
    go_on[j] = ran[j] && s[C_DONE] == 0.0;
    any_p |= go_on[j];
    alpha[j] = s[C_ALPHA], beta[j] = s[C_BETA];
  }
  nt_dispatch(nt, [&](auto nt) {
    double x[U][K], p[U][K], r[U][K];
    STORM_CELL_LOOP(n, blockIdx.x, U, i, u, ldk<K>(X + i * K, x[u], nt); ldk<K>(P + i * K, p[u], nt);
                    if (any_p) ldk<K>(R + i * K, r[u], nt);, {
      _Pragma("unroll") for (int j = 0; j < K; ++j) {
        if (ran[j]) x[u][j] += alpha[j] * p[u][j];
        if (go_on[j]) p[u][j] = r[u][j] + beta[j] * p[u][j];
      }
      stk<K>(X + i * K, x[u], nt);
      if (any_p) stk<K>(P + i * K, p[u], nt);
    })
  });
}

// per-block partials of <A_j, B_j> into c->d_partials[j * nb + block]
static int block_dot_partials(storm_hip_ctx *c, int64_t n, int k, const double *A, const double *B, int *nb_out,
                              const int *done) {
  const int nb = block_blocks(n);
  STORM_TRY(partials_reserve(c, (int64_t)k * nb));
  const int nt = block_nt(c, n, k);
#define GO(K_) hipLaunchKernelGGL(block_dot_kernel<K_>, dim3(nb), dim3(kBlock), 0, c->stream, n, A, B, c->d_partials, done, nt)
  STORM_K_SWITCH(k, GO)
#undef GO
  HIP_TRY(hipGetLastError());
  *nb_out = nb;
  return STORM_HIP_OK;
}

static int check_block(const storm_hip_vec *X, int k, const char *what) {
  STORM_REQUIRE(X, "%s: null vector", what);
  STORM_REQUIRE(k >= 1 && k <= kMaxCols, "%s: k = %d outside [1, %d]", what, k, kMaxCols);
  STORM_REQUIRE(X->n_owned % k == 0, "%s: a vector of %lld elements is not a block of %d columns", what,
                (long long)X->n_owned, k);
  if (X->n_halo > 0 || X->ctx->comm != nullptr)
    STORM_FAIL(STORM_HIP_E_UNSUPPORTED, "%s: block vectors are single-rank (the vector has halo rows or the context a communicator)", what);
  return STORM_HIP_OK;
}

static int column_copy(const storm_hip_vec *X, int k, int j, const storm_hip_vec *v, bool get, const char *what) {
  STORM_REQUIRE(X && v, "%s: null vector", what);
  STORM_TRY(check_block(X, k, what));
  STORM_REQUIRE(j >= 0 && j < k, "%s: column %d outside [0, %d)", what, j, k);
  STORM_REQUIRE(v->ctx == X->ctx, "%s: vectors belong to different contexts", what);
  STORM_REQUIRE(v->n_owned * k == X->n_owned, "%s: the block has %lld cells, the vector %lld", what,
                (long long)(X->n_owned / k), (long long)v->n_owned);
  STORM_REQUIRE(v->d != X->d, "%s: the column vector is the block itself", what);
  storm_hip_ctx *c = X->ctx;
  HIP_TRY(hipSetDevice(c->device));
  STORM_TRY(lazy_sync(c));
  const int64_t n = v->n_owned;
  if (n == 0) return STORM_HIP_OK;
  const int nb = (int)std::min<int64_t>((n + kBlock - 1) / kBlock, 65536);
  if (get) hipLaunchKernelGGL(block_column_kernel<true>, dim3(nb), dim3(kBlock), 0, c->stream, n, k, j, X->d, v->d, c->api_done);
  else hipLaunchKernelGGL(block_column_kernel<false>, dim3(nb), dim3(kBlock), 0, c->stream, n, k, j, X->d, v->d, c->api_done);
  HIP_TRY(hipGetLastError());
  return STORM_HIP_OK;
}

}  // namespace storm

using namespace storm;

extern "C" {

int storm_hip_block_get_column(const storm_hip_vec *X, int k, int j, storm_hip_vec *v) {
  return column_copy(X, k, j, v, true, "block_get_column");
}

int storm_hip_block_set_column(storm_hip_vec *X, int k, int j, const storm_hip_vec *v) {
  return column_copy(X, k, j, v, false, "block_set_column");
}

int storm_hip_block_dot(const storm_hip_vec *A, const storm_hip_vec *B, int k, double *out) {
  STORM_REQUIRE(A && B && out, "block_dot: null argument");
  STORM_TRY(check_block(A, k, "block_dot"));
  STORM_REQUIRE(A->ctx == B->ctx, "block_dot: vectors belong to different contexts");
  STORM_REQUIRE(A->n_owned == B->n_owned, "block_dot: size mismatch (%lld vs %lld elements)", (long long)A->n_owned,
                (long long)B->n_owned);
  storm_hip_ctx *c = A->ctx;
  HIP_TRY(hipSetDevice(c->device));
  STORM_TRY(lazy_sync(c));
  ++c->n_host_reductions;
  const int64_t n = A->n_owned / k;
  if (n == 0) {
    for (int j = 0; j < k; ++j) out[j] = 0.0;
    return STORM_HIP_OK;
  }
  int nb = 0;
  STORM_TRY(block_dot_partials(c, n, k, A->d, B->d, &nb, nullptr));
  STORM_TRY(k_reduce_final(c, c->d_partials, nb, k, c->d_scalars, nullptr));
  HIP_TRY(hipMemcpyAsync(c->h_scalars, c->d_scalars, sizeof(double) * (size_t)k, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (int j = 0; j < k; ++j) out[j] = c->h_scalars[j];
  return STORM_HIP_OK;
}

int storm_hip_block_axpy(storm_hip_vec *Y, const double *a, const storm_hip_vec *X, int k) {
  STORM_REQUIRE(Y && X && a, "block_axpy: null argument");
  STORM_TRY(check_block(Y, k, "block_axpy"));
  STORM_REQUIRE(Y->ctx == X->ctx, "block_axpy: vectors belong to different contexts");
  STORM_REQUIRE(Y->n_owned == X->n_owned, "block_axpy: size mismatch (%lld vs %lld elements)", (long long)Y->n_owned,
                (long long)X->n_owned);
  STORM_REQUIRE(Y->d != X->d, "block_axpy: X and Y must not alias");
  storm_hip_ctx *c = Y->ctx;
  HIP_TRY(hipSetDevice(c->device));
  STORM_TRY(lazy_sync(c));
  const int64_t n = Y->n_owned / k;
  if (n == 0) return STORM_HIP_OK;
  ColCoefs cf{};
  for (int j = 0; j < k; ++j) cf.a[j] = a[j];
  const int nb = block_blocks(n), nt = block_nt(c, n, k);
#define GO(K_) hipLaunchKernelGGL(block_axpy_kernel<K_>, dim3(nb), dim3(kBlock), 0, c->stream, n, Y->d, cf, X->d, c->api_done, nt)
  STORM_K_SWITCH(k, GO)
#undef GO
  HIP_TRY(hipGetLastError());
  return STORM_HIP_OK;
}

int storm_hip_solve_cg_block(const storm_hip_op *op, double alpha, double beta, int k, const storm_hip_vec *B,
                             storm_hip_vec *X, const storm_hip_solver_params *params, storm_hip_solver_result *results,
                             double *histories) {
  STORM_REQUIRE(op && B && X && params && results, "solve_cg_block: null argument");
  STORM_TRY(spmv_block_check(op, k, B, X, "solve_cg_block"));
  STORM_REQUIRE(params->num_iterations >= 0, "solve_cg_block: num_iterations < 0");
  storm_hip_ctx *c = op->ctx;
  HIP_TRY(hipSetDevice(c->device));
  STORM_TRY(lazy_sync(c));
  const int64_t n = op->n_rows, N = params->num_iterations;
  SolverState *st = c->d_state;
  const int *done = &st->done;

  for (int i = 0; i < kStateRing; ++i) c->h_done_ring[i] = 0;  // (the previous solve ended with a stream wait: nothing posts any more)
  // (work vectors and the device history come from -- and go back to -- the context's pool: no allocation from the
  //  second solve on; the history is a zero-filled vector of k (N + 1) doubles)
  struct Cleanup {
    std::vector<storm_hip_vec *> v;
    ~Cleanup() {
      for (size_t i = v.size(); i-- > 0;) storm_hip_vec_destroy(v[i]);
    }
  } keep;
  double *d_history = nullptr;
  if (histories) {
    storm_hip_vec *h = nullptr;
    STORM_TRY(storm_hip_vec_create(c, (int64_t)k * (N + 1), 0, &h));
    keep.v.push_back(h);
    d_history = h->d;
  }
  STORM_TRY(state_init(c, st, params->absolute_error_tolerance, params->relative_error_tolerance, N, d_history, c->d_done_ring));
  int lag = params->check_lag > 0 ? params->check_lag : 4;
  lag = std::min(lag, kStateRing - 1);

  storm_hip_vec *work[3] = {nullptr, nullptr, nullptr};
  STORM_TRY(vec_create_work_batch(X, 3, work));
  keep.v.insert(keep.v.end(), work, work + 3);
  double *P = work[0]->d, *R = work[1]->d, *Z = work[2]->d;
  const int nbv = block_blocks(n);
  const int nb_spmv = (int)((op->n_slices + 3) / 4);
  STORM_TRY(partials_reserve(c, (int64_t)k * std::max(nbv, 4 * nb_spmv)));
  const TicketArgs tickets{c->d_tickets, c->d_partials, c->d_ticket_sums};
  const int nt = block_nt(c, n, k);

  // init: r = b - A x; p = r; gamma_j = <r_j, r_j>          SolverCg.hpp:75-85
  STORM_TRY(spmv_block_launch(op, alpha, beta, k, X->d, R, nullptr, nullptr, nullptr));
#define GO(K_) hipLaunchKernelGGL((block_cg_r_kernel<K_, true>), dim3(nbv), dim3(kBlock), 0, c->stream, n, st, R, B->d, P, tickets, nt)
  STORM_K_SWITCH(k, GO)
#undef GO
  HIP_TRY(hipGetLastError());

  OutPtrs<kMaxCols> pz{};
  for (int j = 0; j < kMaxCols; ++j) pz.p[j] = &st->s[(j < k ? j : 0) * kColStride + C_PZ];
  for (int64_t it = 0; it < N; ++it) {
    // z_j = A p_j, <p_j, z_j>, alpha_j                      SolverCg.hpp:96-97
    int np = 0;
    STORM_TRY(spmv_block_launch(op, alpha, beta, k, P, Z, c->d_partials, &np, done));
    if (np == 0) STORM_TRY(block_dot_partials(c, n, k, P, Z, &np, done));  // (a CSR tail: the sums by a kernel of their own)
    STORM_TRY(k_reduce_finish(c, c->d_partials, np, k, pz, done, BlockAlphaEpi{st, k}, pz, []() -> int { return STORM_HIP_OK; }));
    // r_j -= alpha_j z_j; gamma_j = <r_j, r_j>; beta_j; the convergence rule      SolverCg.hpp:99, 110-125
#define GO(K_) hipLaunchKernelGGL((block_cg_r_kernel<K_, false>), dim3(nbv), dim3(kBlock), 0, c->stream, n, st, R, Z, P, tickets, nt)
    STORM_K_SWITCH(k, GO)
#undef GO
    HIP_TRY(hipGetLastError());
    // x_j += alpha_j p_j; p_j = r_j + beta_j p_j            SolverCg.hpp:98, 123
#define GO(K_) hipLaunchKernelGGL(block_cg_xp_kernel<K_>, dim3(nbv), dim3(kBlock), 0, c->stream, n, st, (long long)(it + 1), X->d, P, R, nt)
    STORM_K_SWITCH(k, GO)
#undef GO
    HIP_TRY(hipGetLastError());
    bool stop = false;
    if (it >= lag) STORM_TRY(ring_wait(c, c->h_done_ring, it - lag, &stop, c->ring_gen));
    if (stop) break;
  }

  HIP_TRY(hipStreamSynchronize(c->stream));
  double cols[kMaxCols * kColStride];
  HIP_TRY(hipMemcpy(cols, reinterpret_cast<const char *>(st) + offsetof(SolverState, s), sizeof(double) * (size_t)k * kColStride,
                    hipMemcpyDeviceToHost));
  for (int j = 0; j < k; ++j) {
    const double *s = cols + j * kColStride;
    storm_hip_solver_result &r = results[j];
    r.iterations = (int64_t)s[C_ITER];
    r.absolute_error = s[C_ABS], r.relative_error = s[C_REL], r.initial_error = s[C_INITIAL];
    r.converged = s[C_CONV] != 0.0;
    r.path_fallback = 0;
    r.num_applies = 1 + r.iterations;
  }
  // (one copy for all columns; entries behind a column's iterations + 1 are zero)
  if (histories) HIP_TRY(hipMemcpy(histories, d_history, sizeof(double) * (size_t)k * (size_t)(N + 1), hipMemcpyDeviceToHost));
  ++c->n_block_solves;
  return STORM_HIP_OK;
}

}  // extern "C"
