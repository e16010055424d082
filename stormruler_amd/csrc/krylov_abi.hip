// The general Krylov engine, its host driving and its C ABI (storm_hip_krylov_*, storm_hip_op_apply2, storm_hip_solve_cg2):
// argument checks, the start and the end of a solve, the enqueue-ahead loop, the choice between the engine and a fused
// kernel, JFNK's inner solve.  The statements are in krylov_engine.hip, the methods in krylov_methods.hip.
#include "krylov_engine.hpp"
#include "amg.hpp"

using namespace storm;
using namespace storm::kry;

namespace {

int check_ready(K *k, const storm_hip_vec *b, storm_hip_vec *x, const storm_hip_solver_params *p) {
  STORM_REQUIRE(k && b && x && p, "krylov: null argument");
  const Operator &op = k->op;
  STORM_REQUIRE(op.is_set(), "krylov: no operator set");
  STORM_REQUIRE(b->ctx == k->c && x->ctx == k->c, "krylov: context mismatch");
  STORM_REQUIRE(b != x && b->d != x->d, "krylov: b and x must not alias");
  STORM_REQUIRE(b->n_owned == x->n_owned, "krylov: b has %lld rows, x %lld", (long long)b->n_owned,
                (long long)x->n_owned);
  if (op.is(Operator::NATIVE) || op.is(Operator::TWO_STAGE)) {
    STORM_REQUIRE(op.stencil->ctx == k->c, "krylov: operator belongs to another context");
    STORM_REQUIRE(x->n_owned == op.stencil->n_rows, "krylov: operator has %lld rows, x %lld", (long long)op.stencil->n_rows,
                  (long long)x->n_owned);
    STORM_REQUIRE(x->n_halo >= op.stencil->n_halo, "krylov: x has %lld halo rows, operator needs %lld",
                  (long long)x->n_halo, (long long)op.stencil->n_halo);
  }
  if (k->pre_diag) STORM_REQUIRE(k->pre_diag->n_owned == x->n_owned, "krylov: diagonal preconditioner size mismatch");
  if (k->pre_cheb) {
    STORM_REQUIRE(k->pre_cheb->ctx == k->c, "krylov: the Chebyshev preconditioner belongs to another context");
    STORM_REQUIRE(k->pre_cheb->op->n_rows == x->n_owned, "krylov: the Chebyshev preconditioner has %lld rows, x %lld",
                  (long long)k->pre_cheb->op->n_rows, (long long)x->n_owned);
  }
  if (k->pre_amg) {
    const int64_t rows = k->pre_amg->op->n_rows;
    STORM_REQUIRE(k->pre_amg->ctx == k->c, "krylov: the multigrid preconditioner belongs to another context");
    STORM_REQUIRE(rows == x->n_owned, "krylov: the multigrid preconditioner has %lld rows, x %lld", (long long)rows,
                  (long long)x->n_owned);
    STORM_REQUIRE(!k->pre_amg->invalid, "krylov: the last storm_hip_amg_refresh of the multigrid preconditioner failed; it is "
                                        "invalid until one succeeds");
  }
  if (op.is(Operator::FD)) {
    STORM_REQUIRE(op.x->ctx == k->c, "krylov: the finite-difference operator's vectors belong to another context");
    STORM_REQUIRE(op.x->n_owned == x->n_owned, "krylov: the finite-difference operator has %lld rows, x %lld",
                  (long long)op.x->n_owned, (long long)x->n_owned);
    STORM_REQUIRE(x != op.x && x != op.w && x->d != op.x->d && x->d != op.w->d,
                  "krylov: x must not alias the finite-difference operator's linearisation point or w");
    if (k->method == STORM_HIP_JFNK)
      STORM_FAIL(STORM_HIP_E_UNSUPPORTED, "krylov: JFNK differentiates the operator itself; it takes no finite-difference operator");
  }
  STORM_REQUIRE(p->num_iterations >= 0, "krylov: num_iterations < 0");
  return STORM_HIP_OK;
}

// The register file for S_top registers: grown where it is short, zeroed, the constant 1.0, and mu of a finite-difference
// operator in its register (stream-ordered: a device word is read when the copy runs).
int prepare_registers(K *k) {
  hipStream_t s = k->c->stream;
  if (k->S_top > k->S_cap) {
    if (k->S) (void)hipFree(k->S);
    k->S = nullptr, k->S_cap = 0;
    HIP_TRY(hipMalloc((void **)&k->S, sizeof(double) * (size_t)k->S_top));
    k->S_cap = k->S_top;
  }
  HIP_TRY(hipMemsetAsync(k->S, 0, sizeof(double) * (size_t)k->S_top, s));
  static const double one = 1.0;
  HIP_TRY(hipMemcpyAsync(k->S + R_ONE, &one, sizeof(double), hipMemcpyHostToDevice, s));
  if (!k->op.is(Operator::FD)) return STORM_HIP_OK;
  if (k->op.mu_dev != nullptr)
    HIP_TRY(hipMemcpyAsync(k->S + k->r_fd + 3, k->op.mu_dev, sizeof(double), hipMemcpyDeviceToDevice, s));
  else
    HIP_TRY(hipMemcpyAsync(k->S + k->r_fd + 3, &k->op.mu, sizeof(double), hipMemcpyHostToDevice, s));
  return STORM_HIP_OK;
}

void release_work(K *k) {
  for (auto *w : k->work) storm_hip_vec_destroy(w);
  k->work.clear();
  k->op_work = nullptr, k->fd_held = false;
  k->qs.clear(), k->zs.clear(), k->rs.clear(), k->us.clear(), k->ps.clear(), k->gs.clear();
  if (k->d_history) (void)hipFree(k->d_history), k->d_history = nullptr;
  k->active = false;
}

// Common start of solve() and init(): state, registers, work vectors, init() enqueued.
int begin_solve(K *k, const storm_hip_vec *b, storm_hip_vec *x, const storm_hip_solver_params *p, bool stepping,
                double *history) {
  storm_hip_ctx *c = k->c;
  STORM_TRY(check_ready(k, b, x, p));
  HIP_TRY(hipSetDevice(c->device));
  release_work(k);
  k->b = b, k->x = x, k->n = x->n_owned, k->status = STORM_HIP_OK, k->stepping = stepping;
  k->gram_schmidt = p->gram_schmidt;
  k->lag = p->check_lag > 0 ? p->check_lag : 4;
  if (k->lag > kStateRing - 1) k->lag = kStateRing - 1;
  switch (k->method) {
    case STORM_HIP_GMRES:
    case STORM_HIP_FGMRES: k->inner = (int)(p->num_inner_iterations > 0 ? p->num_inner_iterations : 50); break;
    case STORM_HIP_BICGSTAB_L: k->inner = (int)(p->num_inner_iterations > 0 ? p->num_inner_iterations : 2); break;
    case STORM_HIP_IDRS: k->inner = (int)(p->num_inner_iterations > 0 ? p->num_inner_iterations : 4); break;
    default: k->inner = 0;
  }
  if (k->method == STORM_HIP_BICGSTAB_L || k->method == STORM_HIP_IDRS)
    STORM_REQUIRE(k->inner <= 48, "krylov: num_inner_iterations = %d too large for this method (<= 48)", k->inner);
  if (k->method == STORM_HIP_IDRS)
    STORM_REQUIRE(c->n_ranks == 1, "krylov: IDR(s) draws its shadow space with fill_randomly, single rank only");
  k->clear_pending();
  k->dp = nullptr;
  k->applies = k->pre_applies = 0;
  k->it_enqueued = 0;
  k->active = true;
  k->setup();
  if (k->op.needs_work_vector()) k->op_work = k->vec();
  k->jf_inner_iterations = 0;
  if (!k->ok()) return k->status;
  STORM_TRY(prepare_registers(k));
  // solver state
  for (int i = 0; i < kStateRing; ++i) k->h_ring[i] = 0;
  if (history && !stepping) {
    HIP_TRY(hipMalloc((void **)&k->d_history, sizeof(double) * (size_t)(p->num_iterations + 1)));
    HIP_TRY(hipMemsetAsync(k->d_history, 0, sizeof(double) * (size_t)(p->num_iterations + 1), c->stream));
  }
  // (stepping: the caller owns the convergence decision)
  STORM_TRY(state_init(c, k->d_st, stepping ? 0.0 : p->absolute_error_tolerance, stepping ? 0.0 : p->relative_error_tolerance,
                       stepping ? (1LL << 62) : p->num_iterations, (history && !stepping) ? k->d_history : nullptr, k->d_ring));
  k->my_ring_gen = c->ring_gen;
  k->init();
  k->applies_after.assign(1, k->applies);
  k->pre_after.assign(1, k->pre_applies);
  k->dp = &k->d_st->done;
  return k->status;
}

typedef int (*fused_entry)(const storm_hip_op *, double, double, const storm_hip_vec *, storm_hip_vec *,
                           const storm_hip_solver_params *, storm_hip_solver_result *, double *);
// The fused kernel that takes this solve, if any: a stencil operator without preconditioner has one for CG, BiCGStab and
// GMRES (solver_cg.hip, solver_bicgstab.hip, solver_gmres.hip).  Such a solve has its own fallback.
fused_entry fused_for(const K *k, const storm_hip_solver_params *params) {
  if (!k->op.is(Operator::NATIVE) || k->has_pre() || k->c->opt_generic_solvers != 0) return nullptr;
  return k->method == STORM_HIP_CG         ? &storm_hip_solve_cg
         : k->method == STORM_HIP_BICGSTAB ? &storm_hip_solve_bicgstab
         : k->method == STORM_HIP_GMRES && params->num_inner_iterations < kMaxMulti
             ? &storm_hip_solve_gmres  // (its state slab holds restarts below kMaxMulti)
             : nullptr;
}

// The solve: a fused kernel where one takes it, else the engine's enqueue-ahead loop.
int krylov_solve_engine(storm_hip_krylov *k, const storm_hip_vec *b, storm_hip_vec *x,
                        const storm_hip_solver_params *params, storm_hip_solver_result *result, double *history,
                        int64_t *pre_applies) {
  storm_hip_ctx *c = k->c;
  if (const fused_entry fused = fused_for(k, params)) {
    if (pre_applies) *pre_applies = 0;
    return fused(k->op.stencil, k->op.alpha, k->op.beta, b, x, params, result, history);
  }
  int st = begin_solve(k, b, x, params, false, history);
  for (int64_t it = 0; st == STORM_HIP_OK && it < params->num_iterations; ++it) {
    k->iterate(it);
    st = k->status;
    if (st != STORM_HIP_OK) break;
    k->it_enqueued = it + 1;
    k->applies_after.push_back(k->applies);
    k->pre_after.push_back(k->pre_applies);
    // look at the verdict of iteration it - lag (JFNK: of this one -- a Newton step past convergence would run a
    // whole inner solve for nothing, and the inner solve has waited for the device anyway)
    const int64_t lag = k->method == STORM_HIP_JFNK ? 0 : k->lag;
    if (it >= lag) {
      bool stop = false;
      st = ring_wait(c, k->h_ring, it - lag, &stop, k->my_ring_gen);  // (a nested solve drew a generation of its own since)
      if (stop) break;
    }
  }
  if (st == STORM_HIP_OK) st = state_read(k->c, k->d_st, k->h_st);
  if (st == STORM_HIP_OK) st = lat_check_gave_up(c);
  if (st == STORM_HIP_OK) {
    const int64_t iters = k->h_st->iteration;
    const int64_t a0 = k->applies, p0 = k->pre_applies;
    k->finalize(iters, true);
    st = k->status;
    const size_t at = (size_t)std::min<int64_t>(iters, (int64_t)k->applies_after.size() - 1);
    result->iterations = iters;
    result->absolute_error = k->h_st->absolute_error;
    result->relative_error = k->h_st->relative_error;
    result->initial_error = k->h_st->initial_error;
    result->converged = k->h_st->converged;
    result->num_applies = k->applies_after[at] + (k->applies - a0);
    if (pre_applies) *pre_applies = k->pre_after[at] + (k->pre_applies - p0);
    if (st == STORM_HIP_OK && history && k->d_history)
      HIP_TRY(hipMemcpy(history, k->d_history, sizeof(double) * (size_t)(iters + 1), hipMemcpyDeviceToHost));
    if (st == STORM_HIP_OK) HIP_TRY(hipStreamSynchronize(c->stream));
  }
  (void)hipStreamSynchronize(c->stream);
  release_work(k);
  if (st == STORM_HIP_OK) st = comm_check_error(c);  // (a transport's bounded wait gave up during this solve)
  return st;
}

int stages2_supported(const storm_hip_op *op, const char *what) {
  if (op->halo.n_nbrs > 0 || op->n_halo > 0 || op->ctx->comm != nullptr)
    STORM_FAIL(STORM_HIP_E_UNSUPPORTED, "%s: the two-stage operator is single-rank (the operator has a halo plan or halo "
                                        "columns, or the context a communicator)", what);
  return STORM_HIP_OK;
}

// A solve under coop_solve_with_fallback (coop_host.hip: should a cooperative kernel give up -- the engine's GMRES runs its
// Gram-Schmidt chains as such where they fit -- x is restored and `attempt` repeated without them).
template <class F>
int solve_with_fallback(storm_hip_ctx *c, storm_hip_vec *x, storm_hip_solver_result *result, F attempt) {
  int fb = 0;
  const int st = coop_solve_with_fallback(c, x, [](void *p) -> int { return (*static_cast<F *>(p))(); }, &attempt, &fb);
  if (st == STORM_HIP_OK) result->path_fallback = fb;
  return st;
}
// CG on a two-stage operator.  One attempt: the one-kernel path (latency.hip, cg2_latency_kernel) where the operator is
// eligible and a register variant holds its rows, else -- and after a refused launch -- the engine's CG loop with the two
// stages as library launches.
int solve_cg2_on(storm_hip_krylov *k, const storm_hip_vec *b, storm_hip_vec *x, const storm_hip_solver_params *params,
                 storm_hip_solver_result *result, double *history) {
  storm_hip_ctx *c = k->c;
  HIP_TRY(hipSetDevice(c->device));
  int st = solve_with_fallback(c, x, result, [&]() -> int {
    const Operator &op = k->op;
    bool taken = false;
    STORM_TRY(cg2_latency_try(op.stencil, op.alpha, op.beta, op.alpha2, op.beta2, b, x, params, result, history, &taken));
    if (taken) return STORM_HIP_OK;
    // (not eligible, no register variant holds the rows, or the launch was refused -- noted in result->path_fallback)
    ++c->n_engine_solves;
    return krylov_solve_engine(k, b, x, params, result, history, nullptr);
  });
  if (st == STORM_HIP_OK) st = comm_check_error(c);
  return st;
}

// CG with a preconditioner the one-kernel path holds (latency.hip, pcg_latency_kernel; option latency_pre): a diagonal, or a
// Chebyshev object on the solve's own operator with its alpha and beta, reading the fp64 records.  CG has no preconditioner
// side.  (An operator the resident path takes without a preconditioner stays on the engine with one.)
bool pcg_latency_wanted(const K *k) {
  const storm_hip_ctx *c = k->c;
  if (c->opt_latency_pre == 0 || c->opt_generic_solvers != 0 || k->method != STORM_HIP_CG || !k->op.is(Operator::NATIVE)) return false;
  const storm_hip_op *op = k->op.stencil;
  if (!cg_latency_eligible(op) || res_eligible(op, false)) return false;
  if (k->pre_diag != nullptr) return true;
  const storm_hip_cheb *h = k->pre_cheb;
  return h != nullptr && h->reduced == 0 && h->op == op && h->alpha == k->op.alpha && h->beta == k->op.beta;
}
// One attempt: the kernel where a register variant holds the rows, else -- and after a refused launch -- the engine's loop.
int solve_pcg_on(storm_hip_krylov *k, const storm_hip_vec *b, storm_hip_vec *x, const storm_hip_solver_params *params,
                 storm_hip_solver_result *result, double *history, int64_t *pre_applies) {
  storm_hip_ctx *c = k->c;
  int st = solve_with_fallback(c, x, result, [&]() -> int {
    const Operator &op = k->op;
    bool taken = false;
    STORM_TRY(pcg_latency_try(op.stencil, op.alpha, op.beta, k->pre_diag, k->pre_cheb, b, x, params, result, history, pre_applies,
                              &taken));
    if (taken) return STORM_HIP_OK;
    // (no register variant holds the rows, the launch was refused, or the kernel gave up -- noted in result->path_fallback)
    ++c->n_engine_solves;
    return krylov_solve_engine(k, b, x, params, result, history, pre_applies);
  });
  if (st == STORM_HIP_OK) st = comm_check_error(c);
  return st;
}

// A(s) for the inner engine of a JFNK object: the outer object's operator, whatever its kind, as library launches
// (predicated on the inner solve's flag like any callback's).
int jfnk_outer_apply(void *user, storm_hip_vec *y, const storm_hip_vec *x) {
  const K *o = static_cast<const K *>(user);
  return o->op.apply_now(y, x, o->op_work);
}
}  // namespace

// J(x) t = r: the reference's inner BiCGStab (tolerances 1e-8, 2000 iterations, no preconditioner, SolverNewton.hpp:133-135)
// on the finite-difference operator at (x, w, mu), mu a register of the outer engine.
int storm::kry::jfnk_inner_solve(K *o) {
  storm_hip_krylov *in = o->jf_inner;
  in->op = Operator::fd(&jfnk_outer_apply, o, o->x, o->v, 0.0, o->S + o->r_a0);
  in->pre_fn = nullptr, in->pre_user = nullptr, in->pre_diag = nullptr, in->pre_cheb = nullptr, in->pre_amg = nullptr;
  storm_hip_solver_params ip;
  storm_hip_solver_params_default(&ip);
  ip.num_iterations = 2000, ip.absolute_error_tolerance = ip.relative_error_tolerance = 1.0e-8;
  storm_hip_solver_result ir{};
  ++o->c->n_jfnk_inner_solves;
  STORM_TRY(krylov_solve_engine(in, o->r, o->t, &ip, &ir, nullptr, nullptr));
  o->jf_inner_iterations += ir.iterations;
  o->applies += ir.num_applies;
  return STORM_HIP_OK;
}

extern "C" {

int storm_hip_krylov_create(storm_hip_ctx *ctx, int method, storm_hip_krylov **out) {
  STORM_REQUIRE(ctx && out, "krylov_create: null argument");
  STORM_REQUIRE(method >= STORM_HIP_CG && method <= STORM_HIP_JFNK, "krylov_create: unknown method %d", method);
  *out = nullptr;
  HIP_TRY(hipSetDevice(ctx->device));
  auto *k = new storm_hip_krylov();
  k->c = ctx, k->method = method;
  if (!ctx->krylov_free.empty()) {  // what a destroyed engine of this context left (begin_solve writes all of it anew)
    const KrylovRes r = ctx->krylov_free.back();
    ctx->krylov_free.pop_back();
    k->d_st = r.d_st, k->h_st = r.h_st, k->h_ring = r.h_ring, k->d_ring = r.d_ring, k->S = r.S, k->S_cap = r.S_cap;
  } else {
    hipError_t e = hipMalloc((void **)&k->d_st, sizeof(SolverState));
    if (e == hipSuccess) e = hipMemset(k->d_st, 0, sizeof(SolverState));
    if (e == hipSuccess) e = hipHostMalloc((void **)&k->h_st, sizeof(SolverState), hipHostMallocMapped);
    if (e == hipSuccess) e = hipHostMalloc((void **)&k->h_ring, sizeof(unsigned long long) * kStateRing, hipHostMallocMapped);
    if (e == hipSuccess) e = hipHostGetDevicePointer((void **)&k->d_ring, k->h_ring, 0);
    if (e != hipSuccess) {
      if (k->d_st) (void)hipFree(k->d_st);
      if (k->h_st) (void)hipHostFree(k->h_st);
      if (k->h_ring) (void)hipHostFree(k->h_ring);
      delete k;
      HIP_TRY(e);
    }
  }
  if (method == STORM_HIP_JFNK) {  // the inner solver of SolverNewton.hpp:133: one object for every Newton step
    const int st = storm_hip_krylov_create(ctx, STORM_HIP_BICGSTAB, &k->jf_inner);
    if (st != STORM_HIP_OK) {
      (void)storm_hip_krylov_destroy(k);
      return st;
    }
  }
  *out = k;
  return STORM_HIP_OK;
}

int storm_hip_krylov_destroy(storm_hip_krylov *k) {
  if (!k) return STORM_HIP_OK;
  if (k->jf_inner) (void)storm_hip_krylov_destroy(k->jf_inner), k->jf_inner = nullptr;
  (void)hipSetDevice(k->c->device);
  (void)hipStreamSynchronize(k->c->stream);
  release_work(k);
  if (k->c->krylov_free.size() < 8) {  // (the stream is idle: nothing reads these any more)
    k->c->krylov_free.push_back(KrylovRes{k->d_st, k->h_st, k->h_ring, k->d_ring, k->S, k->S_cap});
  } else {
    if (k->S) (void)hipFree(k->S);
    (void)hipFree(k->d_st);
    (void)hipHostFree(k->h_st);
    (void)hipHostFree(k->h_ring);
  }
  delete k;
  return STORM_HIP_OK;
}

int storm_hip_krylov_set_operator(storm_hip_krylov *k, const storm_hip_op *op, double alpha, double beta) {
  STORM_REQUIRE(k && op, "krylov_set_operator: null argument");
  k->op = Operator::native(op, alpha, beta);
  return STORM_HIP_OK;
}


int storm_hip_krylov_set_operator2(storm_hip_krylov *k, const storm_hip_op *op, double alpha1, double beta1, double alpha2,
                                   double beta2) {
  STORM_REQUIRE(k && op, "krylov_set_operator2: null argument");
  STORM_TRY(stages2_supported(op, "krylov_set_operator2"));
  k->op = Operator::stages2(op, alpha1, beta1, alpha2, beta2);
  return STORM_HIP_OK;
}

int storm_hip_krylov_set_operator_fn(storm_hip_krylov *k, storm_hip_apply_fn apply, void *user) {
  STORM_REQUIRE(k && apply, "krylov_set_operator_fn: null argument");
  k->op = Operator::callback(apply, user);
  return STORM_HIP_OK;
}

int storm_hip_krylov_set_operator_fd(storm_hip_krylov *k, storm_hip_apply_fn apply, void *user, const storm_hip_vec *x,
                                     const storm_hip_vec *w, double mu) {
  STORM_REQUIRE(std::isfinite(mu) && mu > 0.0, "krylov_set_operator_fd: mu = %g must be finite and > 0", mu);
  STORM_REQUIRE(k && apply && x && w, "krylov_set_operator_fd: null argument");
  STORM_REQUIRE(x->ctx == k->c && w->ctx == k->c, "krylov_set_operator_fd: x / w belong to another context");
  STORM_REQUIRE(x->n_owned == w->n_owned, "krylov_set_operator_fd: x has %lld rows, w %lld", (long long)x->n_owned,
                (long long)w->n_owned);
  k->op = Operator::fd(apply, user, x, w, mu, nullptr);
  return STORM_HIP_OK;
}

int storm_hip_krylov_get_int(const storm_hip_krylov *k, const char *key, int64_t *value) {
  STORM_REQUIRE(k && key && value, "krylov_get_int: null argument");
  if (!strcmp(key, "inner_iterations")) *value = k->jf_inner_iterations;
  else STORM_FAIL(STORM_HIP_E_INVALID, "krylov_get_int: unknown key '%s'", key);
  return STORM_HIP_OK;
}

// z = A(y) with the object's operator, outside a solve: enqueued on the context's stream, predicated like any library
// call when a callback makes it.
int storm_hip_krylov_apply(storm_hip_krylov *k, const storm_hip_vec *y, storm_hip_vec *z) {
  STORM_REQUIRE(k && y && z, "krylov_apply: null argument");
  STORM_REQUIRE(k->op.is_set(), "krylov_apply: no operator set");
  STORM_REQUIRE(z != y && z->d != y->d, "krylov_apply: z must not alias y");
  STORM_REQUIRE(y->ctx == k->c && z->ctx == k->c, "krylov_apply: context mismatch");
  STORM_REQUIRE(y->n_owned == z->n_owned, "krylov_apply: y has %lld rows, z %lld", (long long)y->n_owned, (long long)z->n_owned);
  STORM_REQUIRE(!k->active, "krylov_apply: a solve is in progress on this object");
  storm_hip_ctx *c = k->c;
  const Operator &op = k->op;
  if (op.is(Operator::FD)) {
    STORM_REQUIRE(op.x->n_owned == y->n_owned, "krylov_apply: the finite-difference operator has %lld rows, y %lld",
                  (long long)op.x->n_owned, (long long)y->n_owned);
    STORM_REQUIRE(z->d != op.x->d && z->d != op.w->d, "krylov_apply: z must not alias the operator's x or w");
  }
  HIP_TRY(hipSetDevice(c->device));
  STORM_TRY(lazy_sync(c));
  if (!op.is(Operator::FD)) {
    const int st = op.apply_now(z, y, nullptr);
    return op.calls_back() ? callback_status(st, "krylov_apply: the operator callback") : st;
  }
  // the engine's statements on a register file of the common registers and the operator's four
  k->status = STORM_HIP_OK, k->n = y->n_owned, k->dp = c->api_done;
  k->clear_pending();
  k->S_top = R_USER;
  k->r_fd = k->alloc(4);
  STORM_TRY(prepare_registers(k));
  storm_hip_vec *s = nullptr;  // a pooled work vector (stream-ordered: released below, reused by the next call)
  STORM_TRY(vec_create_work_batch(y, 1, &s));
  k->op_work = s;
  k->apply(z, y);
  k->flush();
  k->op_work = nullptr, k->dp = nullptr;
  (void)storm_hip_vec_destroy(s);
  return k->status;
}

int storm_hip_krylov_set_preconditioner_fn(storm_hip_krylov *k, storm_hip_apply_fn apply, void *user, int side) {
  STORM_REQUIRE(k, "krylov_set_preconditioner_fn: null solver");
  STORM_REQUIRE(side >= STORM_HIP_LEFT && side <= STORM_HIP_SYMMETRIC, "krylov: unknown preconditioner side %d", side);
  k->pre_fn = apply, k->pre_user = user, k->pre_diag = nullptr, k->pre_cheb = nullptr, k->pre_amg = nullptr, k->side = side;
  return STORM_HIP_OK;
}

int storm_hip_krylov_set_preconditioner_diag(storm_hip_krylov *k, const storm_hip_vec *d, int side) {
  STORM_REQUIRE(k, "krylov_set_preconditioner_diag: null solver");
  STORM_REQUIRE(side >= STORM_HIP_LEFT && side <= STORM_HIP_SYMMETRIC, "krylov: unknown preconditioner side %d", side);
  STORM_REQUIRE(d == nullptr || d->ctx == k->c, "krylov: preconditioner diagonal belongs to another context");
  k->pre_fn = nullptr, k->pre_user = nullptr, k->pre_diag = d, k->pre_cheb = nullptr, k->pre_amg = nullptr, k->side = side;
  return STORM_HIP_OK;
}

int storm_hip_krylov_set_preconditioner_cheb(storm_hip_krylov *k, const storm_hip_cheb *h, int side) {
  STORM_REQUIRE(k, "krylov_set_preconditioner_cheb: null solver");
  STORM_REQUIRE(side >= STORM_HIP_LEFT && side <= STORM_HIP_SYMMETRIC, "krylov: unknown preconditioner side %d", side);
  STORM_REQUIRE(h == nullptr || h->ctx == k->c, "krylov: the Chebyshev preconditioner belongs to another context");
  k->pre_fn = nullptr, k->pre_user = nullptr, k->pre_diag = nullptr, k->pre_cheb = h, k->pre_amg = nullptr, k->side = side;
  return STORM_HIP_OK;
}

int storm_hip_krylov_set_preconditioner_amg(storm_hip_krylov *k, const storm_hip_amg *h, int side) {
  STORM_REQUIRE(k, "krylov_set_preconditioner_amg: null solver");
  STORM_REQUIRE(side >= STORM_HIP_LEFT && side <= STORM_HIP_SYMMETRIC, "krylov: unknown preconditioner side %d", side);
  STORM_REQUIRE(h == nullptr || h->ctx == k->c, "krylov: the multigrid preconditioner belongs to another context");
  k->pre_fn = nullptr, k->pre_user = nullptr, k->pre_diag = nullptr, k->pre_cheb = nullptr, k->pre_amg = h, k->side = side;
  return STORM_HIP_OK;
}

int storm_hip_krylov_set_real(storm_hip_krylov *k, const char *key, double value) {
  STORM_REQUIRE(k && key, "krylov_set_real: null argument");
  if (!strcmp(key, "relaxation_factor")) k->relaxation = value;
  else STORM_FAIL(STORM_HIP_E_INVALID, "krylov_set_real: unknown key '%s'", key);
  return STORM_HIP_OK;
}

int storm_hip_krylov_solve(storm_hip_krylov *k, const storm_hip_vec *b, storm_hip_vec *x,
                           const storm_hip_solver_params *params, storm_hip_solver_result *result, double *history,
                           int64_t *pre_applies) {
  STORM_REQUIRE(k && result, "krylov_solve: null argument");
  STORM_TRY(lazy_sync(k->c));
  STORM_TRY(check_ready(k, b, x, params));
  storm_hip_ctx *c = k->c;
  HIP_TRY(hipSetDevice(c->device));
  // CG on a two-stage operator: the one-kernel path where it fits (storm_hip_solve_cg2), as single-stage CG below
  if (k->op.is(Operator::TWO_STAGE) && k->method == STORM_HIP_CG && !k->has_pre() && c->opt_generic_solvers == 0) {
    if (pre_applies) *pre_applies = 0;
    return solve_cg2_on(k, b, x, params, result, history);
  }
  if (fused_for(k, params) != nullptr) return krylov_solve_engine(k, b, x, params, result, history, pre_applies);
  if (pcg_latency_wanted(k)) return solve_pcg_on(k, b, x, params, result, history, pre_applies);
  ++c->n_engine_solves;
  return solve_with_fallback(c, x, result, [&] { return krylov_solve_engine(k, b, x, params, result, history, pre_applies); });
}

int storm_hip_krylov_init(storm_hip_krylov *k, const storm_hip_vec *b, storm_hip_vec *x,
                          const storm_hip_solver_params *params, double *initial_error) {
  STORM_REQUIRE(k && initial_error, "krylov_init: null argument");
  STORM_TRY(lazy_sync(k->c));
  int st = begin_solve(k, b, x, params, true, nullptr);
  if (st == STORM_HIP_OK) st = state_read(k->c, k->d_st, k->h_st);
  if (st != STORM_HIP_OK) {
    release_work(k);
    return st;
  }
  *initial_error = k->h_st->initial_error;
  return STORM_HIP_OK;
}

int storm_hip_krylov_iterate(storm_hip_krylov *k, double *error) {
  STORM_REQUIRE(k && error, "krylov_iterate: null argument");
  STORM_REQUIRE(k->active && k->stepping, "krylov_iterate: no storm_hip_krylov_init before");
  HIP_TRY(hipSetDevice(k->c->device));
  STORM_TRY(lazy_sync(k->c));
  k->iterate(k->it_enqueued);
  if (!k->ok()) return k->status;
  k->it_enqueued += 1;
  STORM_TRY(state_read(k->c, k->d_st, k->h_st));
  *error = k->h_st->absolute_error;
  return STORM_HIP_OK;
}

int storm_hip_krylov_finalize(storm_hip_krylov *k) {
  STORM_REQUIRE(k, "krylov_finalize: null solver");
  STORM_REQUIRE(k->active && k->stepping, "krylov_finalize: no storm_hip_krylov_init before");
  HIP_TRY(hipSetDevice(k->c->device));
  STORM_TRY(lazy_sync(k->c));
  k->finalize(k->it_enqueued, false);
  const int st = k->status;
  (void)hipStreamSynchronize(k->c->stream);
  release_work(k);
  return st;
}

// ---- the two-stage operator A = beta2 I + alpha2 M (beta1 I + alpha1 M) ------------------------------------------------
// The linear part of the playground's Cahn-Hilliard lambda (Playground.cpp:153-167: two stormDivGrad calls per apply).
int storm_hip_op_apply2(const storm_hip_op *op, double alpha1, double beta1, double alpha2, double beta2, const storm_hip_vec *x,
                        storm_hip_vec *t, storm_hip_vec *y) {
  STORM_REQUIRE(op && x && y, "op_apply2: null argument");
  STORM_REQUIRE(x->ctx == op->ctx && y->ctx == op->ctx && (t == nullptr || t->ctx == op->ctx), "op_apply2: context mismatch");
  STORM_REQUIRE(x != y && x->d != y->d && x != t && y != t && (t == nullptr || (t->d != x->d && t->d != y->d)),
                "op_apply2: x, t and y must be pairwise distinct");
  STORM_REQUIRE(x->n_owned == op->n_rows && y->n_owned == op->n_rows && (t == nullptr || t->n_owned == op->n_rows),
                "op_apply2: operator has %lld rows, x %lld, t %lld, y %lld", (long long)op->n_rows, (long long)x->n_owned,
                (long long)(t ? t->n_owned : op->n_rows), (long long)y->n_owned);
  STORM_TRY(stages2_supported(op, "op_apply2"));
  storm_hip_vec *work = nullptr;
  if (t == nullptr) {  // a pooled work vector (stream-ordered: released below, reused by the next call)
    STORM_TRY(vec_create_work_batch(x, 1, &work));
    t = work;
  }
  // t = beta1 x + alpha1 M x;  y = beta2 x;  y += alpha2 M t  (the lambda's statements, Playground.cpp:153-167)
  int st = storm_hip_op_apply(op, alpha1, beta1, x, t);
  if (st == STORM_HIP_OK) st = storm_hip_copy(y, x);
  if (st == STORM_HIP_OK) st = storm_hip_scale(y, beta2);
  if (st == STORM_HIP_OK) st = storm_hip_op_apply_add(op, alpha2, t, y);
  if (work != nullptr) {
    if (st == STORM_HIP_OK) st = lazy_sync(op->ctx);  // (nothing that reads the work vector may still be waiting)
    (void)storm_hip_vec_destroy(work);
  }
  return st;
}

int storm_hip_solve_cg2(const storm_hip_op *op, double alpha1, double beta1, double alpha2, double beta2, const storm_hip_vec *b,
                        storm_hip_vec *x, const storm_hip_solver_params *params, storm_hip_solver_result *result, double *history) {
  STORM_REQUIRE(op && b && x && params && result, "solve_cg2: null argument");
  STORM_TRY(stages2_supported(op, "solve_cg2"));
  STORM_TRY(lazy_sync(op->ctx));
  storm_hip_krylov *k = nullptr;  // (its state comes from the context's free list after the first solve)
  STORM_TRY(storm_hip_krylov_create(op->ctx, STORM_HIP_CG, &k));
  int st = storm_hip_krylov_set_operator2(k, op, alpha1, beta1, alpha2, beta2);
  if (st == STORM_HIP_OK) st = check_ready(k, b, x, params);
  if (st == STORM_HIP_OK) st = solve_cg2_on(k, b, x, params, result, history);
  (void)storm_hip_krylov_destroy(k);
  return st;
}

}  // extern "C"
