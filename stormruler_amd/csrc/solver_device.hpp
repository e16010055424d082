// Device-side pieces shared by the solver translation units (solver_fused.hip and the unit of each loop: the fused CG /
// BiCGStab / GMRES loops of a stencil operator; krylov_engine.hip: the general Krylov engine): the reference's scalar helpers and the
// body of IterativeSolver::solve's loop, evaluated on the device against a SolverState -- and the fold and final
// pass every reduction of the library ends with (blas1.hip's too).
#pragma once

#include "common.hpp"
#include "ipc_device.hpp"
#include "wave_device.hpp"

namespace storm {

// Crow/MathUtils.hpp:49-52
__device__ __forceinline__ double safe_divide(double x, double y) { return (y == 0.0) ? 0.0 : (x / y); }

// The body of the for loop in IterativeSolver::solve, Solver.hpp:132-140.
// In two halves: the decision as a pure function of what the state holds (any thread may evaluate it, from values it
// loaded itself), and the stores (one thread).
struct AdvanceIn {
  double initial_error, abs_tol, rel_tol;
  long long iteration, num_iterations;
};
struct AdvanceOut {
  double absolute_error, relative_error;
  long long iteration;
  int converged, done;  // 1: set the flag (never cleared here)
};
__device__ __forceinline__ AdvanceIn advance_in(const SolverState *st) {
  return AdvanceIn{st->initial_error, st->abs_tol, st->rel_tol, st->iteration, st->num_iterations};
}
__device__ __forceinline__ AdvanceOut advance_eval(const AdvanceIn &in, double abs_err) {
  AdvanceOut o;
  o.absolute_error = abs_err;
  o.relative_error = abs_err / in.initial_error;
  bool conv = false;
  conv |= (in.abs_tol > 0.0) && (o.absolute_error < in.abs_tol);
  conv |= (in.rel_tol > 0.0) && (o.relative_error < in.rel_tol);
  o.iteration = in.iteration + 1;
  o.converged = conv ? 1 : 0;
  o.done = (conv || o.iteration >= in.num_iterations) ? 1 : 0;
  return o;
}
__device__ inline void advance_store(SolverState *st, const AdvanceOut &o) {
  st->absolute_error = o.absolute_error;
  st->relative_error = o.relative_error;
  st->iteration = o.iteration;
  if (st->history) st->history[o.iteration] = o.absolute_error;
  if (o.converged) st->converged = 1;
  if (o.done) st->done = 1;
  // Tell the host (it polls this pinned ring `check_lag` iterations behind): one system-scope store of a word that
  // names its iteration -- the host needs no event behind the kernel to trust it (common.hpp ring_wait).
  if (st->done_ring)
    __hip_atomic_store(st->done_ring + (o.iteration - 1) % kStateRing,
                       ring_word(st->ring_gen, (unsigned long long)o.iteration, st->done != 0), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ inline void advance(SolverState *st, double abs_err) { advance_store(st, advance_eval(advance_in(st), abs_err)); }

// After init(): Solver.hpp:122-128.
__device__ inline void begin(SolverState *st, double initial_error) {
  st->initial_error = initial_error;
  st->absolute_error = initial_error;
  st->relative_error = 0.0;
  st->iteration = 0;
  st->converged = 0;
  st->done = 0;
  if (st->history) st->history[0] = initial_error;
  if (st->abs_tol > 0.0 && initial_error < st->abs_tol) st->converged = 1, st->done = 1;
  if (st->num_iterations <= 0) st->done = 1;
  if (st->done && st->done_ring)  // no iterate() will run: every poll must see it
    for (int i = 0; i < kStateRing; ++i)
      __hip_atomic_store(st->done_ring + i, ring_word(st->ring_gen, kRingIterMask, true), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// The device-side state of a GMRES cycle and the Givens update of Hessenberg column k with the beta recurrence
// (SolverGmres.hpp:176-191; sym_ortho: Crow/MathUtils.hpp:164-179), followed by the convergence rule.  One thread.
struct GmresDev {
  double *H, *beta, *cs, *sn;  // device arrays: (m+1) x m row-major, m+1, m, m
  int m;
};
__device__ inline void gmres_givens_update(SolverState *st, GmresDev g, int k, double hn) {
  const int m = g.m;
#define H_(i, j) g.H[(i) * m + (j)]
  H_(k + 1, k) = hn;
  for (int i = 0; i < k; ++i) {
    const double chi = g.cs[i] * H_(i, k) + g.sn[i] * H_(i + 1, k);
    H_(i + 1, k) = -g.sn[i] * H_(i, k) + g.cs[i] * H_(i + 1, k);
    H_(i, k) = chi;
  }
  const double a = H_(k, k), b = H_(k + 1, k);
  const double rr = hypot(a, b);
  double cs, sn;
  if (rr > 0.0) cs = a / rr, sn = b / rr;
  else cs = 1.0, sn = 0.0;
  g.cs[k] = cs, g.sn[k] = sn;
  H_(k, k) = cs * H_(k, k) + sn * H_(k + 1, k);
  H_(k + 1, k) = 0.0;
  g.beta[k + 1] = -sn * g.beta[k];
  g.beta[k] *= cs;
  advance(st, fabs(g.beta[k + 1]));
#undef H_
}

// (the second half on its own: a kernel that forms several block sums before it meets a barrier -- solver_cg.hip
//  cg_r_planes_kernel -- keeps lane 0's wave_sum_down values of each and folds them here afterwards: the same bits)
__device__ __forceinline__ double block_sum256_of_waves(const double *lds4) { return (lds4[0] + lds4[1]) + (lds4[2] + lds4[3]); }
__device__ __forceinline__ double block_sum256(double v, double *lds4) {
  v = wave_sum_down(v);  // (the __shfl_down tree's order and bits, without the LDS crossbar: wave_device.hpp)
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) lds4[wave] = v;
  __syncthreads();
  return block_sum256_of_waves(lds4);
}

// The block's sum of p[i0 .. i1): lane t adds p[i0 + t], p[i0 + t + 256], ... in ascending order into ONE accumulator,
// then block_sum256.  Every final pass and every in-kernel fold of partials sums through here: the variants of a solver
// are compared to the bit, and this order is what they share.
// The order is written once, in fold_add: B values of a thread -- p[i], p[i + 256], ... below i1 -- are loaded by
// fold_issue, all before the first is used, and added by fold_add in ascending order.
template <int B>
struct FoldFlight {
  double v[B];
};
template <int B>
__device__ __forceinline__ void fold_issue(const double *__restrict__ p, int i, int i1, FoldFlight<B> &f) {
#pragma unroll
  for (int j = 0; j < B; ++j) {
    f.v[j] = 0.0;
    if (i + kBlock * j < i1) f.v[j] = p[i + kBlock * j];
  }
}
template <int B>
__device__ __forceinline__ void fold_add(const FoldFlight<B> &f, int i, int i1, double &v) {
#pragma unroll
  for (int j = 0; j < B; ++j)
    if (i + kBlock * j < i1) v += f.v[j];
}
__device__ __forceinline__ double block_fold(const double *__restrict__ p, int i0, int i1, double *lds4) {
  double v = 0.0;
  for (int i = i0 + threadIdx.x; i < i1; i += kBlock * 8) {
    FoldFlight<8> f;
    fold_issue(p, i, i1, f);
    fold_add(f, i, i1, v);
  }
  return block_sum256(v, lds4);
}
__device__ __forceinline__ double block_fold(const double *__restrict__ p, int n, double *lds4) {
  return block_fold(p, 0, n, lds4);
}
// block_fold(p, n, lds4) of at most kSinglePassPartials values in two halves, for a kernel that has loads of its own to
// put the fold's behind (solver_cg.hip cg_r_planes_kernel): block_fold_issue requests ALL of the thread's values (32 at
// most), block_fold_sum adds them -- fold_add's order, one accumulator from 0.0 -- and ends with block_sum256.
constexpr int kFoldWhole = kSinglePassPartials / kBlock;
static_assert(kFoldWhole * kBlock == kSinglePassPartials, "a whole fold holds kSinglePassPartials / kBlock values per thread");
using FoldWhole = FoldFlight<kFoldWhole>;
__device__ __forceinline__ void block_fold_issue(const double *__restrict__ p, int n, FoldWhole &f) {
  fold_issue(p, (int)threadIdx.x, n, f);
}
__device__ __forceinline__ double block_fold_sum(const FoldWhole &f, int n, double *lds4) {
  double v = 0.0;
  fold_add(f, (int)threadIdx.x, n, v);
  return block_sum256(v, lds4);
}

// Where the k sums of a final pass go; K: the most it takes (a kernel argument -- the solvers' final pass runs every
// iteration, and carries 4)
template <int K>
struct OutPtrs {
  double *p[K];
};

// Final pass of k simultaneous reductions + the scalar epilogue behind them: one block folds partials[j * nblocks ..],
// on the peer-window transport (use_ipc) exchanges its sums with the other ranks itself (ipc_device.hpp), stores sum j
// into *out.p[j] and runs epi() -- a scalar step (solver_fused.hpp) or a scalar program (krylov_engine.hip) -- in thread 0.
template <class Epi, int K>
__global__ __launch_bounds__(kBlock) void reduce_finish_kernel(const double *__restrict__ partials, int nblocks, int k,
                                                               OutPtrs<K> out, const int *done, IpcDev w, int use_ipc, Epi epi) {
  // (`done` is the same decision on every rank and the transport's all-reduce epoch is advanced by the device, by the
  //  all-reduces that run: skipping keeps the ranks in step)
  if (done && *done) return;
  __shared__ double lds4[4];
  __shared__ double vals[K];
  for (int j = 0; j < k; ++j) {
    const double sum = block_fold(partials + (int64_t)j * nblocks, nblocks, lds4);
    if (threadIdx.x == 0) vals[j] = sum;
  }
  if (use_ipc) ipc_allreduce_block(w, vals, k);
  else __syncthreads();
  if ((int)threadIdx.x < k) *out.p[threadIdx.x] = vals[threadIdx.x];
  __syncthreads();
  if (threadIdx.x == 0) epi();
}

// partials (k arrays of nblocks) -> *out.p[j] -> epi, the same way for every solver: the first pass if there are more
// than kSinglePassPartials; then, on one rank and on the peer-window transport, ONE launch.  Over RCCL the launch stores
// this rank's sums through `local` and runs no epilogue; rccl_tail() enqueues the all-reduce and the epilogue.
template <class Epi, int K, class Tail>
int k_reduce_finish(storm_hip_ctx *c, const double *partials, int nblocks, int k, const OutPtrs<K> &out, const int *done,
                    const Epi &epi, const OutPtrs<K> &local, Tail rccl_tail) {
  STORM_TRY(k_reduce_stage1(c, &partials, &nblocks, k, done));
  IpcDev w{};
  const bool one = c->comm == nullptr || comm_ipc_next(c, &w);
  hipLaunchKernelGGL((reduce_finish_kernel<Epi, K>), dim3(1), dim3(kBlock), 0, c->stream, partials, nblocks, k, one ? out : local,
                     done, w, (int)(c->comm != nullptr && one), one ? epi : Epi{});
  HIP_TRY(hipGetLastError());
  return one ? STORM_HIP_OK : rccl_tail();
}

}  // namespace storm
