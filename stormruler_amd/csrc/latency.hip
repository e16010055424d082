// The latency path: CG and BiCGStab for SMALL operators as ONE cooperative, persistent kernel per solve.
//
// The reference's own meshes have 6 000 .. 80 000 cells (tests/_data/mesh), BASELINE config 1 has 64^3 = 262 144:
// vectors of 50 KB .. 2 MB.  The throughput path (solver_cg.hip and its siblings) spends such an iteration on launch latency -- 7 kernels
// of a few microseconds each.  Here a solve is one launch (SolverCg.hpp:54-126 inside Solver.hpp:116-147):
//
//   * every wavefront owns a fixed set of 64-row slices for the whole solve and keeps x, r, p, z of its rows in
//     REGISTERS; what other wavefronts need for their gathers is published once per iteration -- the rows of the
//     new r and of the CURRENT p -- and a gathering wave forms the neighbour's next direction itself,
//     p'[c] = r[c] + beta p[c], with the same expression (hence the same bits) as the owner does in registers.
//     That removes the third synchronisation point of a CG iteration ("p complete"): TWO grid barriers per
//     iteration remain, one behind each reduction;
//   * the operator is read from a compact fp64 sliced-ELL copy made when the operator was built (op_pack.hip)
//     ([ext 64 f64][col W x 64 i32][val W x 64 f64] per slice, slot-major; small: it stays in L2 / Infinity Cache);
//   * a reduction IS the barrier: every block publishes its partial in its own slot as two self-validating 8-byte
//     words { half of the value, sequence number } (fire and forget: no ordering to rely on), and every block polls
//     all slots with single 16-byte coherent loads until both words of each carry the current sequence number, then
//     folds the values in slot order.  All
//     blocks hold bit-identical alpha, beta and the same convergence verdict (the exit condition is uniform), and
//     a synchronisation point costs about 2.5 memory round trips instead of the 6 of "partials, counter barrier,
//     read partials" (an iteration is a chain of ~0.8 us round trips; nothing else matters at this size);
//   * the records of a wave's slices are loaded into registers once (<= 8 slots per row, <= 2 slices per wave).
//   * rows are summed slot by slot exactly as the throughput kernels do (same expression, same contraction): the
//     SpMV values are bit-identical; dot products group their terms differently (rounding-level differences).
//
// Taken by storm_hip_solve_cg / storm_hip_solve_bicgstab / storm_hip_solve_cg2 (the two-stage operator: cg2_latency_kernel) when the operator has a latency copy (n_rows <= option `latency_rows`, no halo, no
// CSR tail), the context has no communicator, and option `latency_path` != 0.  With option `latency_pre` != 0,
// storm_hip_krylov_solve takes it for CG with a diagonal or a Chebyshev preconditioner too (pcg_latency_kernel, below; the
// rule: krylov_abi.hip pcg_latency_wanted).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "coop_device.hpp"
#include "spmv_device.hpp"
#include "solver_device.hpp"
#include "amg_device.hpp"

namespace storm {

struct LatArgs {
  const char *pack;          // compact records
  const int64_t *rec_off;    // [n_slices + 1] byte offsets
  int64_t n_rows, n_slices;
  double alpha, beta;        // A = beta I + alpha M (the two-stage kernel: the FIRST stage, beta1 I + alpha1 M)
  double alpha2, beta2;      // cg2_latency_kernel: A = beta2 I + alpha2 M (beta I + alpha M)
  const double *b;
  double *x;
  double *p, *r;             // published rows of the current direction and the new residual (see the header)
  double *v0, *v1;           // BiCGStab: published rows of v = A p of even / odd iterations
  double *t;                 // cg2_latency_kernel: published rows of the first stage's result
  char *slots;               // all-reduce slots, kLatSlotStride bytes per block, zeroed before the launch
  SolverState *st;
  int publish_xchg;          // rows are published with atomic exchanges whose return is awaited (option latency_publish)
};

// Neighbour value of the vector an SpMV is applied to: plain x (init), or the direction p' = r + beta p formed
// from the published rows.
struct LatPlain {
  const double *v;
  __device__ __forceinline__ double operator()(int c) const { return v[c]; }
};
struct LatPublished {  // a vector other blocks have published in this launch (coherent loads)
  const double *v;
  __device__ __forceinline__ double operator()(int c) const { return co_load(v + c); }
};
struct LatDirection {
  const double *r, *p;
  double beta;
  __device__ __forceinline__ double operator()(int c) const { return co_load(r + c) + beta * co_load(p + c); }
};

constexpr int kLatCacheWidth = 8;  // slots per row held in registers, at most
template <int S, int W>
struct LatRecords {  // the records of a wave's slices: W slots per row in registers, or (W == 0) re-read every time
  int col[W ? S : 1][W ? W : 1];
  double val[W ? S : 1][W ? W : 1];
  double ext[W ? S : 1];
};

// (M t)_row for one row of slice s: sum_k w_k (t[col_k] - t_i) + ext t_i, slots in order; the row of
// beta v + alpha M t is beta * v_i + alpha * that.  One stage (every kernel but cg2_latency_kernel) has t = v.
template <class Get>
__device__ __forceinline__ double lat_row2(const LatArgs &a, int64_t s, int lane, const Get &get, double ti, double vi, double alpha,
                                           double beta) {
  const int64_t o0 = a.rec_off[s];
  const int width = (int)((a.rec_off[s + 1] - o0 - kWave * 8) / (kWave * 12));
  const char *rec = a.pack + o0;
  const double ext = reinterpret_cast<const double *>(rec)[lane];
  const int *col = reinterpret_cast<const int *>(rec + kWave * 8) + lane;
  const double *val = reinterpret_cast<const double *>(rec + kWave * 8 + (int64_t)width * (kWave * 4)) + lane;
  double acc = 0.0;
  int k = 0;
  for (; k + 4 <= width; k += 4) {  // four neighbours in flight
    const int c0 = col[k * kWave], c1 = col[(k + 1) * kWave], c2 = col[(k + 2) * kWave], c3 = col[(k + 3) * kWave];
    const double w0 = val[k * kWave], w1 = val[(k + 1) * kWave], w2 = val[(k + 2) * kWave], w3 = val[(k + 3) * kWave];
    const double g0 = get(c0), g1 = get(c1), g2 = get(c2), g3 = get(c3);
    acc += w0 * (g0 - ti);
    acc += w1 * (g1 - ti);
    acc += w2 * (g2 - ti);
    acc += w3 * (g3 - ti);
  }
  for (; k < width; ++k) acc += val[k * kWave] * (get(col[k * kWave]) - ti);
  return beta * vi + alpha * (acc + ext * ti);
}
template <class Get>
__device__ __forceinline__ double lat_row(const LatArgs &a, int64_t s, int lane, const Get &get, double vi) {
  return lat_row2(a, s, lane, get, vi, vi, a.alpha, a.beta);
}
// The same from registers: W slots (4: triangle / quadrilateral meshes; 8), the ones past the row's width carry weight 0 and the row's own
// column (a term 0 * (t_i - t_i) leaves the sum as it is).
// (CHUNK neighbours in flight at a time: a neighbour costs one load with LatPlain, up to three with BiCGStab's.)
template <int S, int W, int CHUNK = W, class Get>
__device__ __forceinline__ double lat_row_cached2(const LatRecords<S, W> &rec, int q, const Get &get, double ti, double vi,
                                                  double alpha, double beta) {
  double acc = 0.0;
#pragma unroll
  for (int k0 = 0; k0 < W; k0 += CHUNK) {
    double g[CHUNK];
#pragma unroll
    for (int k = 0; k < CHUNK; ++k) g[k] = get(rec.col[q][k0 + k]);
#pragma unroll
    for (int k = 0; k < CHUNK; ++k) acc += rec.val[q][k0 + k] * (g[k] - ti);
  }
  return beta * vi + alpha * (acc + rec.ext[q] * ti);
}
template <int S, int W, int CHUNK = W, class Get>
__device__ __forceinline__ double lat_row_cached(const LatArgs &a, const LatRecords<S, W> &rec, int q, const Get &get,
                                                 double vi) {
  return lat_row_cached2<S, W, CHUNK>(rec, q, get, vi, vi, a.alpha, a.beta);
}

// The records of a wave's slices into registers (W > 0 variants).
template <int S, int W>
__device__ __forceinline__ void lat_load_records(const LatArgs &a, int64_t wave_id, int64_t n_waves, int lane,
                                                 LatRecords<S, W> &rec) {
  if (W > 0) {
#pragma unroll
    for (int q = 0; q < S; ++q) {
      const int64_t s = wave_id + q * n_waves, row = s * kWave + lane;
      const bool live = s < a.n_slices;
      const int64_t o0 = live ? a.rec_off[s] : 0;
      const int width = live ? (int)((a.rec_off[s + 1] - o0 - kWave * 8) / (kWave * 12)) : 0;
      const char *base = a.pack + o0;
      rec.ext[q] = live ? reinterpret_cast<const double *>(base)[lane] : 0.0;
#pragma unroll
      for (int k = 0; k < W; ++k) {
        const bool has = k < width;
        rec.col[q][k] = has ? (reinterpret_cast<const int *>(base + kWave * 8) + lane)[k * kWave]
                            : (int)(row < a.n_rows ? row : a.n_rows - 1);
        rec.val[q][k] = has ? (reinterpret_cast<const double *>(base + kWave * 8 + (int64_t)width * (kWave * 4)) + lane)[k * kWave]
                            : 0.0;
      }
    }
  }
}

// ---- what the three solvers share: the stopping rule, the end of a solve --------------------------------------------
// Tolerances, counters and errors of a solve (Solver.hpp:116-147); every block holds the same values.
struct LatProgress {
  double initial_error, abs_tol, rel_tol, abs_err, rel_err;
  long long num_iterations, it;
  double *history;
  bool converged;
};
// ... from the state and rr = <r, r> of the start residual                           Solver.hpp:124-128
__device__ __forceinline__ LatProgress lat_progress_begin(const SolverState *st, double rr) {
  LatProgress g;
  g.initial_error = sqrt(rr);
  g.abs_tol = st->abs_tol, g.rel_tol = st->rel_tol;
  g.num_iterations = st->num_iterations;
  g.history = st->history;
  g.converged = g.abs_tol > 0.0 && g.initial_error < g.abs_tol;
  g.abs_err = g.initial_error, g.rel_err = 0.0;
  g.it = 0;
  if (blockIdx.x == 0 && threadIdx.x == 0 && g.history) g.history[0] = g.initial_error;
  return g;
}
// ... into the state: the end of a solve
// (The rule after an iteration, the store of x and CG's update phase stay written out in each kernel: as functions over
//  the kernels' register arrays they cost the variants of 4 and 8 slices per wavefront 2 to 14 more SGPR spills.)
__device__ __forceinline__ void lat_finish(SolverState *st, const LatProgress &g) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    st->initial_error = g.initial_error;
    st->absolute_error = g.abs_err;
    st->relative_error = g.rel_err;
    st->iteration = g.it;
    st->converged = g.converged ? 1 : 0;
    st->done = 1;
  }
}

template <int S, int W>
__global__ __launch_bounds__(kLatBlock) void cg_latency_kernel(LatArgs a) {
  __shared__ double lds[kLatWaves];
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave_id = (int64_t)blockIdx.x * kLatWaves + (threadIdx.x >> 6);
  const int64_t n_waves = (int64_t)gridDim.x * kLatWaves;
  unsigned long long seq = 0, seen = 0;  // seen: what the publishing exchanges returned (consumed at the all-reduces)
  double x[S], r[S], p[S], z[S];
  LatRecords<S, W> rec;
  lat_load_records<S, W>(a, wave_id, n_waves, lane, rec);
  auto apply_row = [&](int q, int64_t s, const auto &get, double vi) -> double {
    if constexpr (W > 0) return lat_row_cached<S, W>(a, rec, q, get, vi);
    else return lat_row(a, s, lane, get, vi);
  };

  // ---- init: r = b - A x; p = r; gamma = <r, r>                                   SolverCg.hpp:54-84
  // (a.p arrives zero-filled -- a fresh work vector -- so the first direction r + 0 * p is r)
  double acc = 0.0;
#pragma unroll
  for (int q = 0; q < S; ++q) {
    const int64_t s = wave_id + q * n_waves, row = s * kWave + lane;
    const bool valid = s < a.n_slices && row < a.n_rows;
    x[q] = valid ? a.x[row] : 0.0;
    r[q] = p[q] = z[q] = 0.0;
    if (s < a.n_slices) {
      const double ax = apply_row(q, s, LatPlain{a.x}, x[q]);  // x is not written before the kernel's end
      r[q] = valid ? a.b[row] - ax : 0.0;
      p[q] = r[q];
      if (valid) co_publish(a.r + row, r[q], a.publish_xchg, seen);
      acc += r[q] * r[q];
    }
  }
  double gamma = lat_allreduce(acc, a.slots, ++seq, lds, true, seen);
  LatProgress g = lat_progress_begin(a.st, gamma);
  double beta = 0.0;

  // ---- iterations                                                                 SolverCg.hpp:86-126
  // entering: registers hold x, r and the direction p of the own rows; memory holds r and the PREVIOUS direction,
  // from which a neighbour's current direction is r[c] + beta p_prev[c]
  while (!g.converged && g.it < g.num_iterations) {
    acc = 0.0;
    const LatDirection dir{a.r, a.p, beta};
#pragma unroll
    for (int q = 0; q < S; ++q) {
      const int64_t s = wave_id + q * n_waves;
      if (s < a.n_slices) {
        z[q] = apply_row(q, s, dir, p[q]);
        z[q] = (s * kWave + lane < a.n_rows) ? z[q] : 0.0;
        acc += p[q] * z[q];
      }
    }
    // every gather of this iteration is done once all blocks have published their <p, z> partial
    const double alpha = safe_divide(gamma, lat_allreduce(acc, a.slots, ++seq, lds));
    // the last synchronisation point: x, r, the rule, the next direction (the same text in both CG kernels)
    acc = 0.0;
#pragma unroll
    for (int q = 0; q < S; ++q) {
      const int64_t s = wave_id + q * n_waves, row = s * kWave + lane;
      x[q] += alpha * p[q];
      r[q] -= alpha * z[q];
      acc += r[q] * r[q];
      if (s < a.n_slices && row < a.n_rows)
        co_publish(a.r + row, r[q], a.publish_xchg, seen), co_publish(a.p + row, p[q], a.publish_xchg, seen);
    }
    const double gamma_bar = gamma;
    gamma = lat_allreduce(acc, a.slots, ++seq, lds, true, seen);
    beta = safe_divide(gamma, gamma_bar);
    g.abs_err = sqrt(gamma);
    g.rel_err = g.abs_err / g.initial_error;
    g.converged = (g.abs_tol > 0.0 && g.abs_err < g.abs_tol) || (g.rel_tol > 0.0 && g.rel_err < g.rel_tol);
    ++g.it;
    if (blockIdx.x == 0 && threadIdx.x == 0 && g.history) g.history[g.it] = g.abs_err;
#pragma unroll
    for (int q = 0; q < S; ++q) p[q] = r[q] + beta * p[q];
  }
#pragma unroll
  for (int q = 0; q < S; ++q) {
    const int64_t s = wave_id + q * n_waves, row = s * kWave + lane;
    if (s < a.n_slices && row < a.n_rows) a.x[row] = x[q];
  }
  lat_finish(a.st, g);
}

// ---- CG for the TWO-STAGE operator on the latency path --------------------------------------------------------------
// A = beta2 I + alpha2 M (beta1 I + alpha1 M): the linear part of the playground's Cahn-Hilliard lambda, which applies
// stormDivGrad twice (Playground.cpp:153-167).  cg_latency_kernel with the apply in two halves and THREE synchronisation
// points per iteration:
//   1. t_i = beta1 p_i + alpha1 (M p')_i, neighbours formed as r[c] + beta p_prev[c] from the published rows as above;
//      the wave keeps t_i and publishes its row; a synchronisation point that carries no sum of the recurrence;
//   2. z_i = beta2 p_i + alpha2 (M t)_i, the neighbours' t from the published rows, the own one from the register;
//      the <p, z> all-reduce;
//   3. x += alpha p, r -= alpha z, r and p published, the <r, r> all-reduce: cg_latency_kernel's, unchanged.
// The init has the same extra point (t of x before r = b - A x).  Rounding per stage as lat_row's:
// beta * v_i + alpha * (acc + ext * t_i).
//   ONE buffer t is enough.  A block publishes the next t (point 1 of iteration k + 1, or of iteration 0 behind the
// init) only after it has passed the <p, z> and the <r, r> all-reduce that follow the current one, and every block
// enters the <p, z> all-reduce (the init: the <r, r> one) only after its gathers of the current t: when the first
// block is past it, nobody reads the current t any more.  The same argument covers r and p as in cg_latency_kernel:
// they are gathered in stage 1, in front of points 1 and 2, and overwritten behind point 2.
template <int S, int W>
__global__ __launch_bounds__(kLatBlock) void cg2_latency_kernel(LatArgs a) {
  __shared__ double lds[kLatWaves];
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave_id = (int64_t)blockIdx.x * kLatWaves + (threadIdx.x >> 6);
  const int64_t n_waves = (int64_t)gridDim.x * kLatWaves;
  unsigned long long seq = 0, seen = 0;  // seen: what the publishing exchanges returned (consumed at the all-reduces)
  double x[S], r[S], p[S], z[S], t[S];
  LatRecords<S, W> rec;
  lat_load_records<S, W>(a, wave_id, n_waves, lane, rec);
  // row of beta v + alpha M t, the neighbours' t through `get`, the own one ti
  auto stage_row = [&](int q, int64_t s, const auto &get, double ti, double vi, double alpha, double beta) -> double {
    if constexpr (W > 0) return lat_row_cached2<S, W>(rec, q, get, ti, vi, alpha, beta);
    else return lat_row2(a, s, lane, get, ti, vi, alpha, beta);
  };
  const LatPublished of_t{a.t};

  // ---- init: r = b - A x; p = r; gamma = <r, r>                                   SolverCg.hpp:54-84
  // (a.p arrives zero-filled, so the first direction r + 0 * p is r; a.t too: a padded slot reads a finite value)
#pragma unroll
  for (int q = 0; q < S; ++q) {
    const int64_t s = wave_id + q * n_waves, row = s * kWave + lane;
    const bool valid = s < a.n_slices && row < a.n_rows;
    x[q] = valid ? a.x[row] : 0.0;
    r[q] = p[q] = z[q] = t[q] = 0.0;
    if (s < a.n_slices) {
      t[q] = stage_row(q, s, LatPlain{a.x}, x[q], x[q], a.alpha, a.beta);  // x is not written before the kernel's end
      t[q] = valid ? t[q] : 0.0;
      if (valid) co_publish(a.t + row, t[q], a.publish_xchg, seen);
    }
  }
  (void)lat_allreduce(0.0, a.slots, ++seq, lds, true, seen);  // t of x is out
  double acc = 0.0;
#pragma unroll
  for (int q = 0; q < S; ++q) {
    const int64_t s = wave_id + q * n_waves, row = s * kWave + lane;
    const bool valid = s < a.n_slices && row < a.n_rows;
    if (s < a.n_slices) {
      const double ax = stage_row(q, s, of_t, t[q], x[q], a.alpha2, a.beta2);
      r[q] = valid ? a.b[row] - ax : 0.0;
      p[q] = r[q];
      if (valid) co_publish(a.r + row, r[q], a.publish_xchg, seen);
      acc += r[q] * r[q];
    }
  }
  double gamma = lat_allreduce(acc, a.slots, ++seq, lds, true, seen);
  LatProgress g = lat_progress_begin(a.st, gamma);
  double beta = 0.0;

  // ---- iterations                                                                 SolverCg.hpp:86-126
  // entering: registers hold x, r and the direction p of the own rows; memory holds r and the PREVIOUS direction,
  // from which a neighbour's current direction is r[c] + beta p_prev[c]
  while (!g.converged && g.it < g.num_iterations) {
    const LatDirection dir{a.r, a.p, beta};
#pragma unroll
    for (int q = 0; q < S; ++q) {
      const int64_t s = wave_id + q * n_waves, row = s * kWave + lane;
      if (s < a.n_slices) {
        t[q] = stage_row(q, s, dir, p[q], p[q], a.alpha, a.beta);
        t[q] = (row < a.n_rows) ? t[q] : 0.0;
        if (row < a.n_rows) co_publish(a.t + row, t[q], a.publish_xchg, seen);
      }
    }
    (void)lat_allreduce(0.0, a.slots, ++seq, lds, true, seen);  // t of the direction is out
    acc = 0.0;
#pragma unroll
    for (int q = 0; q < S; ++q) {
      const int64_t s = wave_id + q * n_waves;
      if (s < a.n_slices) {
        z[q] = stage_row(q, s, of_t, t[q], p[q], a.alpha2, a.beta2);
        z[q] = (s * kWave + lane < a.n_rows) ? z[q] : 0.0;
        acc += p[q] * z[q];
      }
    }
    // every gather of this iteration's t is done once all blocks have published their <p, z> partial
    const double alpha = safe_divide(gamma, lat_allreduce(acc, a.slots, ++seq, lds, false));
    // the last synchronisation point: x, r, the rule, the next direction (the same text in both CG kernels)
    acc = 0.0;
#pragma unroll
    for (int q = 0; q < S; ++q) {
      const int64_t s = wave_id + q * n_waves, row = s * kWave + lane;
      x[q] += alpha * p[q];
      r[q] -= alpha * z[q];
      acc += r[q] * r[q];
      if (s < a.n_slices && row < a.n_rows)
        co_publish(a.r + row, r[q], a.publish_xchg, seen), co_publish(a.p + row, p[q], a.publish_xchg, seen);
    }
    const double gamma_bar = gamma;
    gamma = lat_allreduce(acc, a.slots, ++seq, lds, true, seen);
    beta = safe_divide(gamma, gamma_bar);
    g.abs_err = sqrt(gamma);
    g.rel_err = g.abs_err / g.initial_error;
    g.converged = (g.abs_tol > 0.0 && g.abs_err < g.abs_tol) || (g.rel_tol > 0.0 && g.rel_err < g.rel_tol);
    ++g.it;
    if (blockIdx.x == 0 && threadIdx.x == 0 && g.history) g.history[g.it] = g.abs_err;
#pragma unroll
    for (int q = 0; q < S; ++q) p[q] = r[q] + beta * p[q];
  }
#pragma unroll
  for (int q = 0; q < S; ++q) {
    const int64_t s = wave_id + q * n_waves, row = s * kWave + lane;
    if (s < a.n_slices && row < a.n_rows) a.x[row] = x[q];
  }
  lat_finish(a.st, g);
}

// ---- BiCGStab on the latency path ---------------------------------------------------------------------------------
// SolverBiCgStab.hpp:60-167 inside Solver.hpp:116-147, THREE synchronisation points per iteration (the throughput path
// spends 13 launches on it).  Registers hold x, r, p, v, rt of the own rows.  What a neighbour needs is published as
// rows of r (the residual at the iteration's end), p, and v (two buffers, alternating by iteration); a gathering wave
// forms the vector the operator is applied to itself, by the expression the owner uses:
//   A p':  p'[c] = r[c] + beta (p[c] - omega v[c])            from r, p, v as of the END of the previous iteration
//   A s :  s[c]  = r[c] - alpha v'[c]                         from the same r and THIS iteration's v (other buffer)
// so neither "p complete" nor "s complete" is a barrier of its own: the all-reduces of <rt, v>, (<t, s>, <t, t>) and
// (<r, r>, <rt, r>) are the only ones.  A buffer is overwritten only after an all-reduce that every block enters
// after its last gather from it (r, p: behind the omega all-reduce; v of parity k: written in iteration k + 2, read
// last in iteration k + 1 before its first all-reduce).
__device__ __forceinline__ double bicg_direction(double r, double p, double v, double beta, double omega) {
  return __builtin_fma(beta, __builtin_fma(-omega, v, p), r);  // r + beta (p - omega v)      SolverBiCgStab.hpp:119
}
__device__ __forceinline__ double bicg_half_residual(double r, double v, double alpha) {
  return __builtin_fma(-alpha, v, r);  // r - alpha v                                         SolverBiCgStab.hpp:141
}
struct LatBicgDirection {
  const double *r, *p, *v;
  double beta, omega;
  __device__ __forceinline__ double operator()(int c) const {
    return bicg_direction(co_load(r + c), co_load(p + c), co_load(v + c), beta, omega);
  }
};
struct LatBicgHalf {
  const double *r, *v;
  double alpha;
  __device__ __forceinline__ double operator()(int c) const { return bicg_half_residual(co_load(r + c), co_load(v + c), alpha); }
};

template <int S, int W>
__global__ __launch_bounds__(kLatBlock) void bicgstab_latency_kernel(LatArgs a) {
  __shared__ double lds[2 * kLatWaves];
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave_id = (int64_t)blockIdx.x * kLatWaves + (threadIdx.x >> 6);
  const int64_t n_waves = (int64_t)gridDim.x * kLatWaves;
  unsigned long long seq = 0, seen = 0;  // seen: what the publishing exchanges returned (consumed at the all-reduces)
  double x[S], r[S], p[S], v[S], rt[S];
  LatRecords<S, W> rec;
  lat_load_records<S, W>(a, wave_id, n_waves, lane, rec);
  auto apply_row = [&](int q, int64_t s, const auto &get, double vi) -> double {
    if constexpr (W > 0) return lat_row_cached<S, W, 4>(a, rec, q, get, vi);
    else return lat_row(a, s, lane, get, vi);
  };

  // ---- init: r = b - A x; rt = r; rho = <rt, r>                                   SolverBiCgStab.hpp:82-90
  // (a.p, a.v0, a.v1 arrive zero-filled: the first direction r + 0 * (p - 0 * v) is r, :114)
  double acc = 0.0;
#pragma unroll
  for (int q = 0; q < S; ++q) {
    const int64_t s = wave_id + q * n_waves, row = s * kWave + lane;
    const bool valid = s < a.n_slices && row < a.n_rows;
    x[q] = valid ? a.x[row] : 0.0;
    r[q] = p[q] = v[q] = rt[q] = 0.0;
    if (s < a.n_slices) {
      const double ax = apply_row(q, s, LatPlain{a.x}, x[q]);
      r[q] = valid ? a.b[row] - ax : 0.0;
      rt[q] = r[q];
      if (valid) co_publish(a.r + row, r[q], a.publish_xchg, seen);
      acc += rt[q] * r[q];
    }
  }
  double rho = lat_allreduce(acc, a.slots, ++seq, lds, true, seen);
  LatProgress g = lat_progress_begin(a.st, rho);
  double alpha = 0.0, beta = 0.0, omega = 0.0;

  while (!g.converged && g.it < g.num_iterations) {
    double *v_prev = (g.it & 1) ? a.v0 : a.v1, *v_cur = (g.it & 1) ? a.v1 : a.v0;
    // p = r + beta (p - omega v) (own rows, registers); v = A p; <rt, v>              :114-119, :137-139
    acc = 0.0;
    const LatBicgDirection dir{a.r, a.p, v_prev, beta, omega};
#pragma unroll
    for (int q = 0; q < S; ++q) {
      const int64_t s = wave_id + q * n_waves, row = s * kWave + lane;
      p[q] = bicg_direction(r[q], p[q], v[q], beta, omega);
      if (s < a.n_slices) {
        v[q] = apply_row(q, s, dir, p[q]);
        v[q] = (row < a.n_rows) ? v[q] : 0.0;
        if (row < a.n_rows) co_publish(v_cur + row, v[q], a.publish_xchg, seen);
        acc += rt[q] * v[q];
      }
    }
    alpha = safe_divide(rho, lat_allreduce(acc, a.slots, ++seq, lds, true, seen));
    // s = r - alpha v (kept in r); t = A s; omega = <t, s> / <t, t>                   :140-141, :158-160
    double t[S];
    double acc_ts = 0.0, acc_tt = 0.0;
    const LatBicgHalf half{a.r, v_cur, alpha};
#pragma unroll
    for (int q = 0; q < S; ++q) {
      const int64_t s = wave_id + q * n_waves, row = s * kWave + lane;
      r[q] = bicg_half_residual(r[q], v[q], alpha);
      t[q] = 0.0;
      if (s < a.n_slices) {
        t[q] = apply_row(q, s, half, r[q]);
        t[q] = (row < a.n_rows) ? t[q] : 0.0;
        acc_ts += t[q] * r[q];
        acc_tt += t[q] * t[q];
      }
    }
    lat_allreduce2(acc_ts, acc_tt, a.slots, ++seq, lds, false);  // nothing published since the last one
    omega = safe_divide(acc_ts, acc_tt);
    // x += alpha p + omega s; r = s - omega t; |r|, <rt, r>                           :140, :161-164, :116
    double acc_rr = 0.0, acc_rho = 0.0;
#pragma unroll
    for (int q = 0; q < S; ++q) {
      const int64_t s = wave_id + q * n_waves, row = s * kWave + lane;
      x[q] += alpha * p[q];
      x[q] += omega * r[q];
      r[q] -= omega * t[q];
      acc_rr += r[q] * r[q];
      acc_rho += rt[q] * r[q];
      if (s < a.n_slices && row < a.n_rows)
        co_publish(a.r + row, r[q], a.publish_xchg, seen), co_publish(a.p + row, p[q], a.publish_xchg, seen);
    }
    lat_allreduce2(acc_rr, acc_rho, a.slots, ++seq, lds, true, seen);
    const double rho_bar = rho;
    rho = acc_rho;
    beta = safe_divide(alpha * rho, omega * rho_bar);  // :116-118, for the next iteration
    g.abs_err = sqrt(acc_rr);
    g.rel_err = g.abs_err / g.initial_error;
    g.converged = (g.abs_tol > 0.0 && g.abs_err < g.abs_tol) || (g.rel_tol > 0.0 && g.rel_err < g.rel_tol);
    ++g.it;
    if (blockIdx.x == 0 && threadIdx.x == 0 && g.history) g.history[g.it] = g.abs_err;
  }
#pragma unroll
  for (int q = 0; q < S; ++q) {
    const int64_t s = wave_id + q * n_waves, row = s * kWave + lane;
    if (s < a.n_slices && row < a.n_rows) a.x[row] = x[q];
  }
  lat_finish(a.st, g);
}

// ---- preconditioned CG on the latency path ------------------------------------------------------------------------
// SolverCg.hpp:54-126 with pre_op != nullptr inside Solver.hpp:116-147: z = P r, p = z + beta p, gamma = <r, z>, the
// reported error is norm_2(r).  cg_latency_kernel with the preconditioned residual u = P r in r's place: the rows of u
// and of the CURRENT p are published, a gathering wave forms the neighbour's next direction as u[c] + beta p_prev[c]
// (LatDirection pointed at u: the owner's expression, the same bits).  Three kinds of P, both of the library:
//   DIAG         u_i = d_i r_i (storm_hip_krylov_set_preconditioner_diag; d_i in a register).  Row-local: TWO
//                synchronisation points per iteration -- <p, A p>, then one lat_allreduce2 of (<r, u>, <r, r>).
//   CHEB         u = p_m(A) r, and
//   CHEB_JACOBI  u = p_m(diag(s) A) diag(s) r: a storm_hip_cheb object on the solve's own operator, degree m (a run-time
//                loop, coefficients in the argument struct).  Every row goes through cheb_d0_value / cheb_step_row
//                (amg_device.hpp) and lat_row / lat_row_cached: nothing that rounds is restated, u has the bits of
//                storm_hip_cheb_apply.  The recurrence has no reduction, only neighbour rows of its direction d_k between
//                the products: m + 2 points per iteration --
//                  A. <p, A p>;
//                  B. behind the published rows of d_0 (and of p); it carries <r, r>: every block has the verdict BEFORE
//                     the polynomial, and a solve that ends here does not run it (the count of preconditioner applies the
//                     host reports is the engine's, which does);
//                  C_1 .. C_{m-1}. behind the published d_k, between the products; no sum (cg2_latency_kernel's form);
//                  D. behind the published u; it carries <r, u>.
// The init has the same shape without A (r = b - A x from the caller's x in its place).
//   Overwrite safety: a buffer is rewritten only behind a point that every block enters after its last gather from it.
//     p, u   gathered (as the direction u + beta p_prev) by the product in front of A only.  p is rewritten behind A, u behind
//            the last product of the polynomial (DIAG: behind A), which is behind A too.
//     d[0]   d_0 is written behind A of iteration k.  Its last readers are the even products of iteration k - 1's polynomial,
//            each in front of a point C or D of that iteration, all of which every block has entered before it enters A.
//            d_2, d_4, ... are written by product j - 1 (j even) behind C_{j-1}; the last readers of the previous content
//            d_{j-2} are product j - 2, in front of C_{j-1}.
//     d[1]   d_1 is written by product 0, behind B; the last readers of d[1] belong to the previous polynomial (in front of
//            its D, hence of this A and B).  d_3, d_5, ...: as for d[0], product j - 1 (j odd) writes behind C_{j-1}, the
//            readers of d_{j-2} finished in front of it.
// Registers: x, r, p, u (+ d) and, CHEB*, the polynomial's residual and direction (+ s); z = A p lives from A to the
// residual update only.  Instantiated where that fits 128 VGPRs without scratch (NOTES.md has the table).
enum LatPre { LAT_PRE_DIAG = 0, LAT_PRE_CHEB = 1, LAT_PRE_CHEB_JACOBI = 2 };
struct LatPcgArgs {
  LatArgs a;          // (a.r, a.v0, a.v1, a.t stay null)
  const double *s;    // DIAG: the diagonal d; CHEB_JACOBI: the scale s
  double *u;          // published rows of u = P r
  double *d0, *d1;    // CHEB*: published rows of the polynomial's direction, even / odd products
  int degree;
  double inv_theta;
  double c1[kChebMaxDegree], c2[kChebMaxDegree];
};

template <int S, int W, int PRE>
__global__ __launch_bounds__(kLatBlock) void pcg_latency_kernel(LatPcgArgs A) {
  constexpr bool CHEB = PRE != LAT_PRE_DIAG, JACOBI = PRE == LAT_PRE_CHEB_JACOBI, SCALED = PRE != LAT_PRE_CHEB;
  __shared__ double lds[2 * kLatWaves];
  const LatArgs &a = A.a;
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave_id = (int64_t)blockIdx.x * kLatWaves + (threadIdx.x >> 6);
  const int64_t n_waves = (int64_t)gridDim.x * kLatWaves;
  unsigned long long seq = 0, seen = 0;  // seen: what the publishing exchanges returned (consumed at the all-reduces)
  double x[S], r[S], p[S], u[S], sc[SCALED ? S : 1], res[CHEB ? S : 1], dk[CHEB ? S : 1];
  LatRecords<S, W> rec;
  lat_load_records<S, W>(a, wave_id, n_waves, lane, rec);
  auto apply_row = [&](int q, int64_t s, const auto &get, double vi) -> double {
    if constexpr (W > 0) return lat_row_cached<S, W>(a, rec, q, get, vi);
    else return lat_row(a, s, lane, get, vi);
  };
#pragma unroll
  for (int q = 0; q < S; ++q) {
    const int64_t s = wave_id + q * n_waves, row = s * kWave + lane;
    const bool valid = s < a.n_slices && row < a.n_rows;
    x[q] = valid ? a.x[row] : 0.0;
    r[q] = p[q] = u[q] = 0.0;
    if (SCALED) sc[q] = valid ? A.s[row] : 0.0;
    if (CHEB) res[q] = dk[q] = 0.0;
  }

  // One trip = the residual of the step (the first: r = b - A x, SolverCg.hpp:54-84; then :86-126), u = P r, the rule.
  // (a.p arrives zero-filled -- a fresh work vector -- and the registers' p is 0: the first direction u + 0 * p is u)
  LatProgress g{};
  double gamma = 0.0, beta = 0.0;
  for (bool first = true;; first = false) {
    double acc_rr = 0.0, acc_ru = 0.0;
    if (first) {
#pragma unroll
      for (int q = 0; q < S; ++q) {
        const int64_t s = wave_id + q * n_waves, row = s * kWave + lane;
        if (s < a.n_slices) {
          const double ax = apply_row(q, s, LatPlain{a.x}, x[q]);  // x is not written before the kernel's end
          r[q] = (row < a.n_rows) ? a.b[row] - ax : 0.0;
        }
      }
    } else {
      // entering: registers hold x, r and the direction p of the own rows; memory holds u and the PREVIOUS direction,
      // from which a neighbour's current direction is u[c] + beta p_prev[c]
      double z[S], acc = 0.0;
      const LatDirection dir{A.u, a.p, beta};
#pragma unroll
      for (int q = 0; q < S; ++q) {
        const int64_t s = wave_id + q * n_waves;
        z[q] = 0.0;
        if (s < a.n_slices) {
          z[q] = apply_row(q, s, dir, p[q]);
          z[q] = (s * kWave + lane < a.n_rows) ? z[q] : 0.0;
          acc += p[q] * z[q];
        }
      }
      // A: every gather of u and p is done once all blocks have published their <p, z> partial
      const double alpha = safe_divide(gamma, lat_allreduce(acc, a.slots, ++seq, lds, false));
#pragma unroll
      for (int q = 0; q < S; ++q) {
        const int64_t s = wave_id + q * n_waves, row = s * kWave + lane;
        x[q] += alpha * p[q];
        r[q] -= alpha * z[q];
        if (s < a.n_slices && row < a.n_rows) co_publish(a.p + row, p[q], a.publish_xchg, seen);
      }
    }
    // the new residual's first part of u = P r, and <r, r>
#pragma unroll
    for (int q = 0; q < S; ++q) {
      const int64_t s = wave_id + q * n_waves, row = s * kWave + lane;
      const bool valid = s < a.n_slices && row < a.n_rows;
      acc_rr += r[q] * r[q];
      if constexpr (CHEB) {
        res[q] = r[q];
        dk[q] = cheb_d0_value<JACOBI>(A.inv_theta, r[q], JACOBI ? sc[q] : 1.0);
        if (valid) co_publish(A.d0 + row, dk[q], a.publish_xchg, seen);
      } else {
        u[q] = sc[q] * r[q];
        acc_ru += r[q] * u[q];
        if (valid) co_publish(A.u + row, u[q], a.publish_xchg, seen);
      }
    }
    if constexpr (CHEB) acc_rr = lat_allreduce(acc_rr, a.slots, ++seq, lds, true, seen);  // B
    else lat_allreduce2(acc_ru, acc_rr, a.slots, ++seq, lds, true, seen);
    // the rule                                                                    Solver.hpp:124-128, :130-147
    if (first) {
      g = lat_progress_begin(a.st, acc_rr);
    } else {
      g.abs_err = sqrt(acc_rr);
      g.rel_err = g.abs_err / g.initial_error;
      g.converged = (g.abs_tol > 0.0 && g.abs_err < g.abs_tol) || (g.rel_tol > 0.0 && g.rel_err < g.rel_tol);
      ++g.it;
      if (blockIdx.x == 0 && threadIdx.x == 0 && g.history) g.history[g.it] = g.abs_err;
    }
    if (g.converged || g.it >= g.num_iterations) break;  // (uniform: every block holds the same sums)
    if constexpr (CHEB) {
      // u = d_0 + d_1 + ... + d_m;  t = A d_k;  res' = res - t;  d' = c1 d + c2 (s .* res')
      for (int k = 0; k < A.degree; ++k) {
        const LatPublished of_d{(k & 1) ? A.d1 : A.d0};
        double *d_next = (k & 1) ? A.d0 : A.d1;
        const double c1 = A.c1[k], c2 = A.c2[k];
        const bool last = k + 1 == A.degree;
#pragma unroll
        for (int q = 0; q < S; ++q) {
          const int64_t s = wave_id + q * n_waves, row = s * kWave + lane;
          if (s < a.n_slices) {
            double t = apply_row(q, s, of_d, dk[q]);
            t = (row < a.n_rows) ? t : 0.0;
            const double si = JACOBI ? sc[q] : 1.0;
            const ChebRow o = k == 0 ? cheb_step_row<JACOBI, true>(t, res[q], si, dk[q], u[q], c1, c2)
                                     : cheb_step_row<JACOBI, false>(t, res[q], si, dk[q], u[q], c1, c2);
            res[q] = o.rn, dk[q] = o.dn, u[q] = o.zn;
            if (row < a.n_rows) co_publish((last ? A.u : d_next) + row, last ? u[q] : dk[q], a.publish_xchg, seen);
            if (last) acc_ru += r[q] * u[q];
          }
        }
        if (!last) (void)lat_allreduce(0.0, a.slots, ++seq, lds, true, seen);  // C: d_{k+1} is out
      }
      acc_ru = lat_allreduce(acc_ru, a.slots, ++seq, lds, true, seen);  // D
    }
    const double gamma_bar = gamma;
    gamma = acc_ru;
    beta = first ? 0.0 : safe_divide(gamma, gamma_bar);
#pragma unroll
    for (int q = 0; q < S; ++q) p[q] = u[q] + beta * p[q];
  }
#pragma unroll
  for (int q = 0; q < S; ++q) {
    const int64_t s = wave_id + q * n_waves, row = s * kWave + lane;
    if (s < a.n_slices && row < a.n_rows) a.x[row] = x[q];
  }
  lat_finish(a.st, g);
}

bool cg_latency_eligible(const storm_hip_op *op) {
  const storm_hip_ctx *c = op->ctx;
  return c->opt_latency_path != 0 && c->coop_disabled == 0 && c->comm == nullptr && op->d_lat_pack != nullptr &&
         c->opt_profile_spmv == 0;
}

// The whole solve; fills the SolverState on the device (the caller reads it back).  `family`: which of the four
// kernels; work vectors p, r (CG), p, r, v0, v1 (BiCGStab), p, r, t (two-stage CG) and p, u, d0, d1 (preconditioned CG)
// arrive zero-filled.  LAT_PCG: `pcg` is the kernel's argument (its LatArgs are filled from `a` here), `pre` its LatPre.
enum LatFamily { LAT_CG, LAT_BICGSTAB, LAT_CG2, LAT_PCG };
static int latency_solve(LatFamily family, const storm_hip_op *op, LatArgs a, bool *taken, LatPcgArgs *pcg = nullptr,
                         int pre = LAT_PRE_DIAG) {
  storm_hip_ctx *c = op->ctx;
  *taken = false;
  const int64_t n_slices = (op->n_rows + kWave - 1) / kWave;
  // A co-resident grid (cooperative launch): one 1024-thread block per CU at most (<= 256 blocks: one polling
  // thread per block), at least one slice per wavefront; the smallest register variant that covers all slices.
  // registers can hold the records of a wave's slices when rows have <= kLatCacheWidth slots and S <= 2
  const int w = c->opt_latency_cache == 0 ? 0 : op->max_row_len <= 4 ? 4 : op->max_row_len <= kLatCacheWidth ? 8 : 0;
  auto pick = [w](const void *w0, const void *w4, const void *w8) { return w == 4 ? w4 : w == 8 ? w8 : w0; };
  const void *cg[4] = {
      pick((const void *)cg_latency_kernel<1, 0>, (const void *)cg_latency_kernel<1, 4>, (const void *)cg_latency_kernel<1, 8>),
      pick((const void *)cg_latency_kernel<2, 0>, (const void *)cg_latency_kernel<2, 4>, (const void *)cg_latency_kernel<2, 8>),
      (const void *)cg_latency_kernel<4, 0>, (const void *)cg_latency_kernel<8, 0>};
  const void *bi[4] = {  // (two slices of records AND five vectors do not fit the registers)
      pick((const void *)bicgstab_latency_kernel<1, 0>, (const void *)bicgstab_latency_kernel<1, 4>,
           (const void *)bicgstab_latency_kernel<1, 8>),
      (const void *)bicgstab_latency_kernel<2, 0>, (const void *)bicgstab_latency_kernel<4, 0>, (const void *)bicgstab_latency_kernel<8, 0>};
  const void *cg2[4] = {
      pick((const void *)cg2_latency_kernel<1, 0>, (const void *)cg2_latency_kernel<1, 4>, (const void *)cg2_latency_kernel<1, 8>),
      pick((const void *)cg2_latency_kernel<2, 0>, (const void *)cg2_latency_kernel<2, 4>, (const void *)cg2_latency_kernel<2, 8>),
      (const void *)cg2_latency_kernel<4, 0>, (const void *)cg2_latency_kernel<8, 0>};
  // (preconditioned CG: only the instances that need no scratch at 128 VGPRs exist, NOTES.md -- where the cached form of a
  //  width is not among them the re-reading one stands in; none holds more than two slices per wavefront)
#define STORM_PCG_KERNEL(S_, W_, PRE_) (const void *)pcg_latency_kernel<S_, W_, PRE_>
#define STORM_PCG_VARIANTS(PRE_, W8_)                                                                     \
  {pick(STORM_PCG_KERNEL(1, 0, PRE_), STORM_PCG_KERNEL(1, 4, PRE_), STORM_PCG_KERNEL(1, W8_, PRE_)), \
   STORM_PCG_KERNEL(2, 0, PRE_), (const void *)nullptr, (const void *)nullptr}
  // (eight slots of records beside the polynomial's vectors: 92 bytes of scratch, with four neighbours in flight too)
  const void *pcg_v[3][4] = {STORM_PCG_VARIANTS(LAT_PRE_DIAG, 8), STORM_PCG_VARIANTS(LAT_PRE_CHEB, 0),
                             STORM_PCG_VARIANTS(LAT_PRE_CHEB_JACOBI, 0)};
#undef STORM_PCG_KERNEL
#undef STORM_PCG_VARIANTS
  const void *const *variants = family == LAT_BICGSTAB ? bi : family == LAT_CG2 ? cg2 : family == LAT_PCG ? pcg_v[pre] : cg;
  const int capacity[4] = {1, 2, 4, 8};
  const void *fn = nullptr;
  int64_t blocks = 0;
  for (int v = 0; v < 4 && fn == nullptr; ++v) {
    if (variants[v] == nullptr || occupancy_cached(c, variants[v], kLatBlock, 0) < 1) continue;
    blocks = std::max<int64_t>(1, std::min<int64_t>(std::min(c->num_cus, 256), (n_slices + kLatWaves - 1) / kLatWaves));
    const int64_t waves = blocks * kLatWaves;
    if ((n_slices + waves - 1) / waves <= capacity[v]) fn = variants[v];
  }
  if (fn == nullptr) {  // no register variant holds this many rows per wavefront (latency_rows raised, few CUs): the
    c->coop_fallback = 1;  // throughput path takes the solve
    return STORM_HIP_OK;
  }
  HIP_TRY(hipMemsetAsync(c->d_lat_slots, 0, (size_t)2 * 256 * kLatSlotStride + 256, c->stream));  // tags restart at 1; flag down
  a.pack = op->d_lat_pack, a.rec_off = op->d_lat_off, a.n_rows = op->n_rows, a.n_slices = n_slices, a.slots = c->d_lat_slots;
  a.publish_xchg = (int)(c->opt_latency_publish != 0);
  if (pcg != nullptr) pcg->a = a;
  void *args[] = {pcg != nullptr ? (void *)pcg : (void *)&a};
  *taken = coop_launch(c, fn, (unsigned)blocks, args);
  return STORM_HIP_OK;
}

int cg_latency_solve(const storm_hip_op *op, double alpha, double beta, const double *b, double *x, double *p,
                     double *r, SolverState *d_state, bool *taken) {
  LatArgs a{};
  a.alpha = alpha, a.beta = beta, a.b = b, a.x = x, a.p = p, a.r = r, a.st = d_state;
  return latency_solve(LAT_CG, op, a, taken);
}

int bicgstab_latency_solve(const storm_hip_op *op, double alpha, double beta, const double *b, double *x,
                           double *const work[4], SolverState *d_state, bool *taken) {
  LatArgs a{};
  a.alpha = alpha, a.beta = beta, a.b = b, a.x = x, a.p = work[0], a.r = work[1], a.v0 = work[2], a.v1 = work[3], a.st = d_state;
  return latency_solve(LAT_BICGSTAB, op, a, taken);
}

int cg2_latency_solve(const storm_hip_op *op, double alpha1, double beta1, double alpha2, double beta2, const double *b,
                      double *x, double *const work[3], SolverState *d_state, bool *taken) {
  LatArgs a{};
  a.alpha = alpha1, a.beta = beta1, a.alpha2 = alpha2, a.beta2 = beta2, a.b = b, a.x = x;
  a.p = work[0], a.r = work[1], a.t = work[2], a.st = d_state;
  return latency_solve(LAT_CG2, op, a, taken);
}

// CG with a diagonal (cheb == nullptr: z = scale .* r) or a Chebyshev polynomial preconditioner (cheb: an object on `op` with
// the solve's alpha and beta, not reduced; its scale, if any, is the kernel's).  work: p, u, d0, d1 (zero-filled; the
// last two with cheb only).
int pcg_latency_solve(const storm_hip_op *op, double alpha, double beta, const double *b, double *x, const double *scale,
                      const storm_hip_cheb *cheb, double *const work[4], SolverState *d_state, bool *taken) {
  LatArgs a{};
  a.alpha = alpha, a.beta = beta, a.b = b, a.x = x, a.p = work[0], a.st = d_state;
  LatPcgArgs g{};
  g.s = scale, g.u = work[1];
  int pre = LAT_PRE_DIAG;
  if (cheb != nullptr) {
    pre = cheb->dinv != nullptr ? LAT_PRE_CHEB_JACOBI : LAT_PRE_CHEB;
    g.s = cheb->dinv != nullptr ? cheb->dinv->d : nullptr;
    g.d0 = work[2], g.d1 = work[3], g.degree = cheb->degree, g.inv_theta = cheb->inv_theta;
    std::memcpy(g.c1, cheb->c1, sizeof g.c1);
    std::memcpy(g.c2, cheb->c2, sizeof g.c2);
  }
  return latency_solve(LAT_PCG, op, a, taken, &g, pre);
}

}  // namespace storm
