// Device-resident Krylov loops: CG, BiCGStab, GMRES(m).
//
// Restates Solvers/Solver.hpp:116-147 (IterativeSolver::solve), :236-257
// (InnerOuterIterativeSolver), SolverCg.hpp:54-126, SolverBiCgStab.hpp:59-165 and
// SolverGmres.hpp:51-249 for the operator A = beta*I + alpha*M on the device.
//
// Design: every scalar of the recurrences (gamma, alpha, beta, rho, omega, the Hessenberg
// column, Givens rotations, the residual norm, the iteration counter and the convergence
// verdict) lives in a SolverState in HBM.  Kernels read them from there, the last pass of
// each reduction is followed by a one-thread "step" that evaluates the reference's scalar
// statements (safe_divide, sqrt, sym_ortho, the convergence rule) on the device.  The host
// never waits for a scalar: it enqueues iterations ahead and looks at a pinned copy of the
// state `check_lag` iterations behind; once the device has set `done`, every later kernel
// returns at its first instruction, so the result is exactly the reference's: same
// iteration count, x frozen at the iteration that met the tolerance.
// This unit: what the three loops share (solver_cg.hip, solver_bicgstab.hip, solver_gmres.hip; interface: solver_fused.hpp).
#include <algorithm>
#include "solver_fused.hpp"
#include "blas1_device.hpp"
#include "spmv_device.hpp"

namespace storm {

// The first pass of NV sums (partials[j * nblocks + i]), finished in the kernel (ticket_device.hpp): the block that draws
// the last ticket folds the kStage2 block sums and leaves the totals in out[0 .. NV) -- the consumer (cg_r_kernel) reads
// one scalar instead of folding kStage2 partials in every one of its 8 192 blocks before its first load.
// use_ipc (peer-window transport): the finishing wave also exchanges the sums with the other ranks (ipc_allreduce_wave).
template <int NV>
__global__ __launch_bounds__(kBlock) void reduce_stage1_ticket_kernel(const double *__restrict__ partials, int nblocks,
                                                                      double *__restrict__ out, const SolverState *st,
                                                                      TicketArgs tickets, IpcDev w, int use_ipc) {
  if (st->done) return;
  __shared__ double lds4[4];
  const int g = blockIdx.x;
  const int chunk = (nblocks + gridDim.x - 1) / gridDim.x;
  const int i0 = g * chunk, i1 = min(i0 + chunk, nblocks);
  double mine[NV], total[NV];
  for (int j = 0; j < NV; ++j) mine[j] = block_fold(partials + (int64_t)j * nblocks, i0, i1, lds4);
  if (threadIdx.x >= kWave) return;
  if (ticket_reduce_wave0<NV>(tickets, mine, NV, (unsigned)g, gridDim.x, total)) {
    if (use_ipc) ipc_allreduce_wave<NV>(w, total, NV);
    if (threadIdx.x == 0)
      for (int j = 0; j < NV; ++j) out[j] = total[j];
  }
}

// Option ticket_verify: sums[j] (a reduction recomputed by the two-launch path) against the slab slots the in-kernel
// reduction filled -- they differ by rounding only (another folding order); anything else raises the sticky flag.
// `before`: the sums were taken of the vectors as they are NOW while the step has already run (iteration count).
struct VerifySlots {
  const double *sum[2];
  const double *slot[2];
  int k;
};
__global__ void verify_kernel(VerifySlots v, SolverState *st, long long iteration_of_slots) {
  // (past convergence the ticketed kernel returned early: nothing to compare)
  if (st->iteration != iteration_of_slots) return;
  for (int j = 0; j < v.k; ++j) {
    const double a = *v.sum[j], b = *v.slot[j];
    double scale = fabs(a) > fabs(b) ? fabs(a) : fabs(b);
    // (the second sum of a pair -- <rt, r> beside <r, r> -- has terms of both signs: its rounding error scales with the
    //  first, not with its own value; a lost block's partial is ~1/blocks of the sum, far above either bound)
    if (j == 1 && fabs(*v.sum[0]) > scale) scale = fabs(*v.sum[0]);
    if (!(fabs(a - b) <= (j == 0 ? 1e-10 : 1e-7) * scale)) st->verify_failed = 1;  // (also catches NaN)
  }
}

__global__ void step_kernel(int step, SolverState *st, GmresDev g, bool force) {
  if (!force && st->done) return;
  do_step(step, st, g);
}

// r <<= b - r (Operator.hpp:98); p <<= r (SolverCg.hpp:81 / SolverBiCgStab.hpp:87 for rt);
// partial <r, r>.
__global__ __launch_bounds__(kBlock) void init_residual_kernel(int64_t n, double *__restrict__ r,
                                                               const double *__restrict__ b,
                                                               double *__restrict__ copy_to,
                                                               double *__restrict__ partials, int nt) {
  __shared__ double lds4[4];
  double acc = 0.0;
  const int64_t n2 = n >> 1;
  double2v *r2 = reinterpret_cast<double2v *>(r), *c2 = reinterpret_cast<double2v *>(copy_to);
  const double2v *b2 = reinterpret_cast<const double2v *>(b);
  nt_dispatch(nt, [&](auto nt) {
  STORM_STREAM_FOR(base, n2) {
    double2v vb[kUnroll], vr[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int64_t i = base + u * kBlock;
      if (i < n2) vb[u] = ldv(b2 + i, nt), vr[u] = ldv(r2 + i, nt);
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int64_t i = base + u * kBlock;
      if (i < n2) {
        const double2v v = vb[u] - vr[u];
        stv(r2 + i, v, nt);
        if (copy_to) stv(c2 + i, v, nt);
        acc += v.x * v.x;
        acc += v.y * v.y;
      }
    }
  }
  });
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    const double v = b[n - 1] - r[n - 1];
    r[n - 1] = v;
    if (copy_to) copy_to[n - 1] = v;
    acc += v * v;
  }
  const double s = block_sum256(acc, lds4);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// ---- host-side driver helpers -------------------------------------------------------------------------
int Driver::step(int kind, bool force) {
  hipLaunchKernelGGL(step_kernel, dim3(1), dim3(1), 0, c->stream, kind, st, g, force);
  HIP_TRY(hipGetLastError());
  return STORM_HIP_OK;
}

int Driver::init_residual(double *r, const double *b, double *copy_to) {
  hipLaunchKernelGGL(init_residual_kernel, dim3(stream_blocks(n)), dim3(kBlock), 0, c->stream, n, r, b, copy_to, c->d_partials,
                     stream_nt(c, n));
  HIP_TRY(hipGetLastError());
  return STORM_HIP_OK;
}

int Driver::finish(int nblocks, int k, int slot0, int step, bool force) {
  OutPtrs<4> out{};
  for (int j = 0; j < k; ++j) out.p[j] = slot(slot0 + j);
  return k_reduce_finish(c, c->d_partials, nblocks, k, out, force ? nullptr : done, StepEpi{step, st, g}, out, [&]() -> int {
    STORM_TRY(comm_allreduce_sum(c, out.p[0], k));  // (RCCL: the k adjacent slots all-reduced by one call)
    return step != STEP_NONE ? this->step(step, force) : STORM_HIP_OK;
  });
}

int Driver::finish_dots(int ticketed, int nb, int k, int slot0, const double *a, const double *const *bs, Road allow,
                        int plain_step, Road *ran, const double **consumer_partials) {
  *ran = ticketed ? ROAD_IN_SPMV : ROAD_PLAIN;
  if (ticketed) return STORM_HIP_OK;
  if (nb == 0) {  // operator has a CSR tail: separate dot
    STORM_TRY(k_multi_dot(c, a, bs, k, n, slot(slot0), done));
    if (c->comm != nullptr) STORM_TRY(comm_allreduce_sum(c, slot(slot0), k));
    return plain_step != STEP_NONE ? step(plain_step) : STORM_HIP_OK;
  }
  if (allow != ROAD_PLAIN && (int64_t)k * nb + k * kStage2 <= c->partials_capacity) {
    // many partials: ONE small launch folds them and finishes the sums itself (tickets); the consumer reads them from
    // the slab and starts streaming at once.  (The block sums go behind the SpMV's partials.)
    const TicketArgs t{c->d_tickets, c->d_partials + (size_t)k * nb, c->d_ticket_sums};
    const auto kernel = k == 1 ? reduce_stage1_ticket_kernel<1> : reduce_stage1_ticket_kernel<2>;
    hipLaunchKernelGGL(kernel, dim3(kStage2), dim3(kBlock), 0, c->stream, c->d_partials, nb, slot(slot0), st, t, ipc_w,
                       (int)(allow == ROAD_TICKETS_IPC));
    HIP_TRY(hipGetLastError());
    *ran = allow;
    return allow == ROAD_TICKETS_RCCL ? comm_allreduce_sum(c, slot(slot0), k) : STORM_HIP_OK;
  }
  if (allow == ROAD_TICKETS_RCCL) return *ran = allow, finish(nb, k, slot0, STEP_NONE);
  if (consumer_partials != nullptr && c->comm == nullptr && nb > kSinglePassPartials) {
    // ... without tickets: the first pass here, the fold of its kStage2 results inside the consumer
    *ran = ROAD_CONSUMER, *consumer_partials = c->d_partials;
    return k_reduce_stage1(c, consumer_partials, &nb, k, done);
  }
  return finish(nb, k, slot0, plain_step);
}

int Driver::verify(const double *a, const double *b0, const double *b1, int slot0, int slot1, long long iteration_of_slots) {
  if (c->comm != nullptr) return STORM_HIP_OK;
  const double *bs[2] = {b0, b1};
  const int k = b1 ? 2 : 1;
  int nbp = 0;
  STORM_TRY(k_multi_dot_partials(c, a, bs, k, n, &nbp, nullptr));
  // (test hook ticket_verify_inject: the recomputation "loses" one block's partial, as a stale read would)
  STORM_TRY(k_reduce_final(c, c->d_partials, c->opt_ticket_verify_inject != 0 && nbp > 1 ? nbp - 1 : nbp, k, slot(S_SCRATCH + 8), nullptr));
  VerifySlots v{{slot(S_SCRATCH + 8), slot(S_SCRATCH + 9)}, {slot(slot0), slot(slot1 >= 0 ? slot1 : slot0)}, k};
  hipLaunchKernelGGL(verify_kernel, dim3(1), dim3(1), 0, c->stream, v, st, iteration_of_slots);
  HIP_TRY(hipGetLastError());
  return STORM_HIP_OK;
}

int Driver::apply(const double *x, double *y, int *nblocks, const ApplyDots &dots, bool predicated, const CgStep *cg) {
  SpmvDot sd;
  if (cg != nullptr) {
    sd.cg.iteration = &st->iteration, sd.cg.my_iteration = cg->my_iteration;
    sd.cg.ca = slot(S_ALPHA), sd.cg.cb = slot(S_BETA);
    sd.cg.x = cg->x, sd.cg.r = cg->r, sd.cg.p_out = cg->p_out;
    sd.cg.st = st, sd.cg.rr_sums = cg->rr_sums, sd.cg.rr_ng = cg->rr_ng;
  }
  sd.w = dots.w;
  sd.yy = dots.yy;
  sd.partials = c->d_partials;
  sd.nblocks_out = nblocks;
  if (dots.out0 >= 0) sd.out[0] = slot(dots.out0);
  if (dots.out1 >= 0) sd.out[1] = slot(dots.out1);
  sd.ticketed_out = dots.ticketed;
  if (dots.ticketed) *dots.ticketed = 0;
  const bool want = dots.w != nullptr || dots.yy;
  if (!want && nblocks) *nblocks = 0;
  return spmv_launch(op, host_scal(alpha), host_scal(beta), x, y, want ? &sd : nullptr, predicated ? done : nullptr);
}

int VecPool::make(const storm_hip_vec *like, int count, bool zero) {
  if (!zero) {
    std::vector<storm_hip_vec *> made((size_t)count, nullptr);
    STORM_TRY(vec_create_work_batch(like, count, made.data()));
    v.insert(v.end(), made.begin(), made.end());
    return STORM_HIP_OK;
  }
  for (int i = 0; i < count; ++i) {
    storm_hip_vec *p = nullptr;
    STORM_TRY(storm_hip_vec_create_like(like, &p));
    v.push_back(p);
  }
  return STORM_HIP_OK;
}

static int check_solve_args(const storm_hip_op *op, const storm_hip_vec *b, storm_hip_vec *x,
                            const storm_hip_solver_params *p, storm_hip_solver_result *r) {
  STORM_REQUIRE(op && b && x && p && r, "solve: null argument");
  STORM_REQUIRE(b->ctx == op->ctx && x->ctx == op->ctx, "solve: context mismatch");
  STORM_REQUIRE(b->n_owned == op->n_rows && x->n_owned == op->n_rows, "solve: operator has %lld rows, b %lld, x %lld",
                (long long)op->n_rows, (long long)b->n_owned, (long long)x->n_owned);
  STORM_REQUIRE(x->n_halo >= op->n_halo, "solve: x has %lld halo rows, operator needs %lld", (long long)x->n_halo,
                (long long)op->n_halo);
  STORM_REQUIRE(b != x, "solve: b and x must not alias");
  return STORM_HIP_OK;
}

int prepare_state(const FusedSolveArgs &args, Driver *dp) {
  storm_hip_ctx *c = args.op->ctx;
  HIP_TRY(hipSetDevice(c->device));
  *dp = Driver{c, args.op, args.alpha, args.beta, args.op->n_rows, c->d_state, &c->d_state->done};
  Driver &d = *dp;
  const storm_hip_solver_params *p = args.params;
  comm_forget_prebegun(c);
  STORM_REQUIRE(p->num_iterations >= 0, "solve: num_iterations < 0");
  for (int i = 0; i < kStateRing; ++i) c->h_done_ring[i] = 0;  // (the previous solve ended with a stream wait: nothing posts any more)
  if (args.history) {
    HIP_TRY(hipMalloc(&d.d_history, sizeof(double) * (size_t)(p->num_iterations + 1)));
    HIP_TRY(hipMemsetAsync(d.d_history, 0, sizeof(double) * (size_t)(p->num_iterations + 1), c->stream));
  }
  STORM_TRY(state_init(c, c->d_state, p->absolute_error_tolerance, p->relative_error_tolerance, p->num_iterations, d.d_history,
                       c->d_done_ring));
  d.lag = p->check_lag > 0 ? p->check_lag : 4;
  if (d.lag > kStateRing - 1) d.lag = kStateRing - 1;
  return STORM_HIP_OK;
}

int post_and_poll(Driver &d, int64_t it, bool *stop) {
  *stop = false;
  if (it >= d.lag) STORM_TRY(ring_wait(d.c, d.c->h_done_ring, it - d.lag, stop, d.c->ring_gen));
  return STORM_HIP_OK;
}

int collect(Driver &d, const FusedSolveArgs &args, int per_it, int64_t m) {
  storm_hip_ctx *c = d.c;
  storm_hip_solver_result *res = args.result;
  double *history = args.history;
  STORM_TRY(state_read(c, c->d_state, &c->h_state[0]));
  {  // (a cooperative kernel of this solve -- CG's, a Gram-Schmidt chain -- timed out: the caller re-runs the solve)
    const int st_coop = lat_check_gave_up(c);
    if (st_coop != STORM_HIP_OK) {
      if (d.d_history) (void)hipFree(d.d_history), d.d_history = nullptr;
      return st_coop;
    }
  }
  res->path_fallback = c->coop_fallback;
  if (c->h_state[0].verify_failed) {
    if (d.d_history) (void)hipFree(d.d_history), d.d_history = nullptr;
    STORM_FAIL(STORM_HIP_E_HIP, "ticket_verify: an in-kernel reduction disagreed with its two-launch recomputation "
                                "(a partial sum was not visible to the block that folded it)");
  }
  const SolverState &h = c->h_state[0];
  res->iterations = h.iteration;
  res->absolute_error = h.absolute_error;
  res->relative_error = h.relative_error;
  res->initial_error = h.initial_error;
  res->converged = h.converged;
  res->num_applies = 1 + per_it * h.iteration + (m > 0 ? (h.iteration + m - 1) / m : 0);
  if (history && d.d_history) {
    HIP_TRY(hipMemcpy(history, d.d_history, sizeof(double) * (size_t)(h.iteration + 1), hipMemcpyDeviceToHost));
  }
  if (d.d_history) (void)hipFree(d.d_history), d.d_history = nullptr;
  return STORM_HIP_OK;
}

static int run_fused_body(void *p) {
  const FusedSolveArgs &a = *static_cast<const FusedSolveArgs *>(p);
  return a.body(a);
}
int fused_solve(FusedSolveArgs a) {
  STORM_TRY(check_solve_args(a.op, a.b, a.x, a.params, a.result));
  storm_hip_ctx *c = a.op->ctx;
  HIP_TRY(hipSetDevice(c->device));
  int fb = 0;
  int st = coop_solve_with_fallback(c, a.x, run_fused_body, &a, &fb);
  if (st == STORM_HIP_OK) a.result->path_fallback = fb;
  // a bounded wait of a transport gave up during this solve (a hand-off flag, a peer window): its result is not one
  if (st == STORM_HIP_OK) st = comm_check_error(c);
  return st;
}

}  // namespace storm

extern "C" void storm_hip_solver_params_default(storm_hip_solver_params *p) {
  if (!p) return;
  p->num_iterations = 2000;            // Solver.hpp:67
  p->absolute_error_tolerance = 1e-6;  // Solver.hpp:71
  p->relative_error_tolerance = 1e-6;  // Solver.hpp:72
  p->num_inner_iterations = 50;        // Solver.hpp:159
  p->check_lag = 0;
  p->gram_schmidt = 0;
}
