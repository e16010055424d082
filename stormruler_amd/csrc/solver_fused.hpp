// The interface of the fused loops' units -- solver_fused.hip (what the three loops share), solver_cg.hip,
// solver_bicgstab.hip and solver_gmres.hip (one loop each, with its kernels) -- as spmv_device.hpp is of the SpMV units.
// A unit reaches another unit's kernels through the host functions declared here (Driver's members), never by launching
// them: the library is built without relocatable device code.
#pragma once

#include "common.hpp"
#include "solver_device.hpp"
#include "ticket_device.hpp"

namespace storm {

// named slots of SolverState::s
enum Slot {
  S_GAMMA = 0, S_PZ, S_GAMMA_NEW, S_BETA, S_ALPHA,
  S_RHO, S_RTV, S_TR, S_TT, S_OMEGA, S_RR, S_RHO_NEW,  // (TR,TT) and (RR,RHO_NEW) stay adjacent: one all-reduce each
  S_TMP, S_HN,
  S_SCRATCH = 32,
  S_ALPHA_SEEN = 48,  // (+ 1: armed) option ticket_verify, RCCL BiCGStab: the alpha the early halo of s was formed with
  // option cg_rr_fold: what the residual kernel that ends at its group sums leaves for the kernel that folds them -- the
  // <r,r> its step began with, and (as a double) the iteration counter its sums will produce.  The folding launch reads
  // them and never writes them: its late blocks find what its first ones found.
  S_RR_GAMMA = 50, S_RR_GATE,
};

enum StepKind {
  STEP_NONE = 0,
  STEP_CG_INIT,    // gamma = <r,r>; begin(sqrt(gamma))
  STEP_CG_RR,      // gamma_new -> beta, gamma; advance(sqrt(gamma))
  STEP_BICG_INIT,  // rho = <rt,r>; begin(sqrt(rho))
  STEP_BICG_ALPHA, // alpha = rho / <rt,v>
  STEP_BICG_OMEGA, // omega = <t,r> / <t,t>
  STEP_BICG_END,   // err = sqrt(<r,r>); beta from rho_new; advance
  STEP_GMRES_BETA0_OUTER, // beta[0] = sqrt(tmp); begin(beta[0])
  STEP_GMRES_BETA0,       // beta[0] = sqrt(tmp)
  STEP_GMRES_HN,          // hn = sqrt(tmp)
};

// STEP_CG_RR in two halves (SolverCg.hpp:110-125): the outcome as a pure function of <r,r> and of what the state holds --
// every block of a kernel may evaluate it for itself --, and the stores, by one thread.
struct CgRrOutcome {
  double gamma, beta;  // the new <r,r>; beta = <r,r> / the previous <r,r>
  AdvanceOut a;
};
__device__ __forceinline__ CgRrOutcome cg_rr_eval(double gamma_new, double gamma_bar, const AdvanceIn &in) {
  CgRrOutcome o;
  o.gamma = gamma_new;
  o.beta = safe_divide(gamma_new, gamma_bar);
  o.a = advance_eval(in, sqrt(gamma_new));
  return o;
}
__device__ inline void cg_rr_store(SolverState *st, const CgRrOutcome &o) {
  st->s[S_GAMMA_NEW] = o.gamma;
  st->s[S_GAMMA] = o.gamma;
  st->s[S_BETA] = o.beta;
  advance_store(st, o.a);
}

__device__ inline void do_step(int kind, SolverState *st, GmresDev g) {
  double *s = st->s;
  switch (kind) {
    case STEP_CG_INIT:  // SolverCg.hpp:82,85
      begin(st, sqrt(s[S_GAMMA]));
      break;
    case STEP_CG_RR:  // SolverCg.hpp:110-125
      cg_rr_store(st, cg_rr_eval(s[S_GAMMA_NEW], s[S_GAMMA], advance_in(st)));
      break;
    case STEP_BICG_INIT:  // SolverBiCgStab.hpp:88-90
      begin(st, sqrt(s[S_RHO]));
      break;
    case STEP_BICG_ALPHA:  // SolverBiCgStab.hpp:139
      s[S_ALPHA] = safe_divide(s[S_RHO], s[S_RTV]);
      break;
    case STEP_BICG_OMEGA:  // SolverBiCgStab.hpp:159-160
      s[S_OMEGA] = safe_divide(s[S_TR], s[S_TT]);
      break;
    case STEP_BICG_END: {  // :164 then, for the next iteration, :116-118
      const double rho_bar = s[S_RHO];
      s[S_RHO] = s[S_RHO_NEW];
      s[S_BETA] = safe_divide(s[S_ALPHA] * s[S_RHO], s[S_OMEGA] * rho_bar);
      advance(st, sqrt(s[S_RR]));
    } break;
    case STEP_GMRES_BETA0_OUTER:  // SolverGmres.hpp:87,90
      g.beta[0] = sqrt(s[S_TMP]);
      s[S_HN] = g.beta[0];
      begin(st, g.beta[0]);
      break;
    case STEP_GMRES_BETA0:  // SolverGmres.hpp:115
      g.beta[0] = sqrt(s[S_TMP]);
      s[S_HN] = g.beta[0];
      break;
    case STEP_GMRES_HN:  // SolverGmres.hpp:161
      s[S_HN] = sqrt(s[S_TMP]);
      break;
    default: break;
  }
}

// The epilogue of reduce_finish_kernel (solver_device.hpp) for the fused solvers: a scalar step (STEP_NONE: none).
struct StepEpi {
  int step;
  SolverState *st;
  GmresDev g;
  __device__ void operator()() const {
    if (step != STEP_NONE) do_step(step, st, g);
  }
};

// The streaming shape of blas1.hip: one trip per thread, kUnroll x 16 bytes per stream in flight.
#define STORM_STREAM_FOR(base, n2) \
  for (int64_t base = (int64_t)blockIdx.x * (kBlock * kUnroll) + threadIdx.x; base < (n2); \
       base += (int64_t)gridDim.x * (kBlock * kUnroll))

// ---- host side -------------------------------------------------------------------------------------
struct FusedSolveArgs {
  const storm_hip_op *op;
  double alpha, beta;
  const storm_hip_vec *b;
  storm_hip_vec *x;
  const storm_hip_solver_params *params;
  storm_hip_solver_result *result;
  double *history;
  int (*body)(const FusedSolveArgs &);
};

// Driver::apply: y = A x, optionally with fused <w, y> / <y, y> partials; *nblocks: how many per sum (0 = not fused).
struct ApplyDots {
  const double *w = nullptr;  // <w, y>
  bool yy = false;            // <y, y>
  int out0 = -1, out1 = -1;   // slab slots (-1: none) where an in-kernel (ticketed) reduction may leave <w,y> / <y,y>
  int *ticketed = nullptr;    // whether it did -- then there are no partials to finish (*nblocks is still their count)
};
struct CgStep {  // the fused CG step of spmv.hip (CgFuseArgs): end iteration my_iteration - 1, then apply to the new p
  long long my_iteration;
  double *x;
  const double *r;
  double *p_out;
  // option cg_rr_fold: that iteration's residual kernel ended at its rr_ng group sums of <r,r> (rr_sums; null: the state
  // is complete) -- the step kernel folds them and runs STEP_CG_RR itself
  const double *rr_sums = nullptr;
  int rr_ng = 0;
};

struct Driver {
  storm_hip_ctx *c;
  const storm_hip_op *op;
  double alpha, beta;
  int64_t n;
  SolverState *st;
  const int *done;
  GmresDev g{nullptr, nullptr, nullptr, nullptr, 0};
  int lag;
  double *d_history = nullptr;
  IpcDev ipc_w{};  // the peer-window view (comm_ipc_next) for the kernels that exchange their sums themselves

  double *slot(int i) const { return &st->s[i]; }
  TicketArgs tickets() const { return TicketArgs{c->d_tickets, c->d_partials, c->d_ticket_sums}; }

  // the one-thread scalar step (step_kernel); force: also past convergence
  int step(int kind, bool force = false);
  // r <<= b - r, copy_to <<= r (nullable), stream_blocks(n) per-block partials of <r, r> (init_residual_kernel)
  int init_residual(double *r, const double *b, double *copy_to);
  // partials -> the k adjacent slots from slot0 (+ all-reduce over ranks) -> scalar step
  int finish(int nblocks, int k, int slot0, int step, bool force = false);

  // The dot(s) an apply left as nb per-wave partials (k = 1, 2 arrays of nb) -> the k adjacent slots from slot0.
  // `allow`: the road the caller's configuration permits; *ran: the one taken --
  //   ROAD_IN_SPMV      (ticketed != 0) the SpMV kernel finished them itself: nothing to do
  //   ROAD_PLAIN        Driver::finish with `plain_step`; nb == 0 (a CSR tail: no fused partials): k_multi_dot of
  //                     <a, bs[j]>, the all-reduce and `plain_step` as a launch of its own
  //   ROAD_TICKETS      ONE reduce_stage1_ticket_kernel<k> launch folds them and finishes the sums by tickets (its block
  //                     sums go behind the k nb partials: k nb + k kStage2 <= partials_capacity, else ROAD_PLAIN)
  //   ROAD_TICKETS_IPC  ... and its finishing wave exchanges them with the other ranks (peer windows)
  //   ROAD_TICKETS_RCCL ... comm_allreduce_sum behind the launch, no scalar step: the consumers form the quotient
  //                     (a short workspace: Driver::finish without a step, still ROAD_TICKETS_RCCL)
  //   ROAD_CONSUMER     (consumer_partials != null, one rank, nb > kSinglePassPartials, no ticket road) k_reduce_stage1
  //                     only: the consumer kernel folds the kStage2 block sums left at *consumer_partials itself
  enum Road { ROAD_PLAIN = 0, ROAD_TICKETS, ROAD_TICKETS_IPC, ROAD_TICKETS_RCCL, ROAD_IN_SPMV, ROAD_CONSUMER };
  int finish_dots(int ticketed, int nb, int k, int slot0, const double *a, const double *const *bs, Road allow, int plain_step,
                  Road *ran, const double **consumer_partials = nullptr);

  // Option ticket_verify: <a, b0> (and <a, b1>) once more by the two-launch path (per-block partials, then one block
  // folds them) into scratch slots, compared on the device with the slab slots an in-kernel reduction filled.
  // Single rank only (the slots then hold local sums).  `iteration_of_slots`: the value of the iteration counter for
  // which the slots are current (the ticketed kernel may have run the scalar step already).
  int verify(const double *a, const double *b0, const double *b1, int slot0, int slot1, long long iteration_of_slots);

  int apply(const double *x, double *y, int *nblocks, const ApplyDots &dots = ApplyDots(), bool predicated = true, const CgStep *cg = nullptr);
};

struct VecPool {  // work vectors: re-assigned (zeroed) on every solve like SolverCg.hpp:57-59
  std::vector<storm_hip_vec *> v;
  ~VecPool() {  // (in reverse: the context's pool is a stack -- the next solve finds every vector in its old role)
    for (size_t i = v.size(); i-- > 0;) storm_hip_vec_destroy(v[i]);
  }
  // zero = false: the solver writes every owned row of these vectors before it reads it (context.hip, vec_create_work)
  int make(const storm_hip_vec *like, int count, bool zero = true);
};

// The state of a solve about to start: the device, the Driver of args.op, the slab, the history buffer, the poll lag.
int prepare_state(const FusedSolveArgs &args, Driver *d);
// Iteration `it` is enqueued; *stop = the word the device posted for iteration it - lag says it is done.
int post_and_poll(Driver &d, int64_t it, bool *stop);
// The end of a solve: the slab into args.result and args.history; num_applies = 1 + per_it * iterations (+ with m > 0 one
// per restart cycle of m iterations).
int collect(Driver &d, const FusedSolveArgs &args, int per_it, int64_t m = 0);
// A fused solve that may take a cooperative kernel, re-run without them should one give up (coop_host.hip)
int fused_solve(FusedSolveArgs a);

}  // namespace storm
