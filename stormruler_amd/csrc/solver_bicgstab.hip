// The fused BiCGStab loop of a stencil operator (SolverBiCgStab.hpp:59-165) and its kernel; see solver_fused.hip.
#include "solver_fused.hpp"
#include "blas1_device.hpp"
#include "spmv_device.hpp"

namespace storm {

// The two half-steps of a BiCGStab iteration (SolverBiCgStab.hpp:140-141 and :161-164).
//   FIRST : r -= alpha v.  The reference's  x += alpha p  is deferred: nothing reads x before the
//           second half-step, and doing it there saves one read + write of x per iteration.
//   SECOND: x = (x + alpha p) + omega r  (the same two roundings, in the reference's order),
//           r -= omega t, partials of <r,r> and <rt,r>.
template <bool SECOND>
__global__ __launch_bounds__(kBlock) void bicg_update_kernel(int64_t n, SolverState *st, double *__restrict__ x,
                                                             double *__restrict__ r, const double *__restrict__ p,
                                                             const double *__restrict__ w,
                                                             const double *__restrict__ rt,
                                                             double *__restrict__ partials, int nt, int reverse,
                                                             TicketArgs tickets, const double *r_in = nullptr,
                                                             IpcDev ipc_w = IpcDev{}, int use_ipc = 0) {
  // r_in (second half-step): the vector r is READ from (s = r - alpha v, where the apply formed it into a vector of its
  // own); null: r itself
  if (st->done) return;
  const unsigned bx = reverse ? gridDim.x - 1 - blockIdx.x : blockIdx.x;  // the same rows and slots, dealt out from the far end
  __shared__ double lds4[4];
  // With tickets the SpMV before this kernel left the finished sums in the slab and no step kernel ran: every
  // block forms alpha (first half-step, :139) / omega (second, :159-160) itself, block 0 keeps it for later readers.
  double alpha = st->s[S_ALPHA], omega = st->s[S_OMEGA];
  if (tickets.cnt != nullptr) {
    if (!SECOND) {
      alpha = safe_divide(st->s[S_RHO], st->s[S_RTV]);
      if (blockIdx.x == 0 && threadIdx.x == 0) {
        st->s[S_ALPHA] = alpha;
        // Option ticket_verify over RCCL: the halo of s left BEFORE this kernel, its rows formed by halo_pack_bicg_kernel
        // with an alpha of its own division -- the bits of what the neighbours received depend on it being THIS alpha.
        if (st->s[S_ALPHA_SEEN + 1] != 0.0) {
          if (__double_as_longlong(st->s[S_ALPHA_SEEN]) != __double_as_longlong(alpha)) st->verify_failed = 1;
          st->s[S_ALPHA_SEEN + 1] = 0.0;
        }
      }
    } else {
      omega = safe_divide(st->s[S_TR], st->s[S_TT]);
      if (blockIdx.x == 0 && threadIdx.x == 0) st->s[S_OMEGA] = omega;
    }
  }
  double acc_rr = 0.0, acc_rho = 0.0;
  const int64_t n2 = n >> 1;
  double2v *x2 = reinterpret_cast<double2v *>(x), *r2 = reinterpret_cast<double2v *>(r);
  const double2v *ri2 = r_in ? reinterpret_cast<const double2v *>(r_in) : r2;
  const double2v *p2 = reinterpret_cast<const double2v *>(p), *w2 = reinterpret_cast<const double2v *>(w);
  const double2v *rt2 = reinterpret_cast<const double2v *>(rt);
  constexpr int U = SECOND ? 1 : kUnroll;  // 7 streams: one access per stream in flight (see cg_xp_kernel)
  nt_dispatch(nt, [&](auto nt) {
  for (int64_t base = (int64_t)bx * (kBlock * U) + threadIdx.x; base < n2;
       base += (int64_t)gridDim.x * (kBlock * U)) {
    double2v vx[U], vr[U], vw[U], vp[U], vt[U];
#pragma unroll
    for (int q = 0; q < U; ++q) {
      const int64_t i = base + q * kBlock;
      if (i < n2) {
        vr[q] = ldv(ri2 + i, nt), vw[q] = ldv(w2 + i, nt);
        if (SECOND) vx[q] = ldv(x2 + i, nt), vp[q] = ldv(p2 + i, nt), vt[q] = ldv(rt2 + i, nt);
      }
    }
#pragma unroll
    for (int q = 0; q < U; ++q) {
      const int64_t i = base + q * kBlock;
      if (i < n2) {
        if (!SECOND) {
          vr[q] -= alpha * vw[q];
          stv(r2 + i, vr[q], nt);
        } else {
          vx[q] += alpha * vp[q];
          vx[q] += omega * vr[q];
          vr[q] -= omega * vw[q];
          stv(x2 + i, vx[q], nt);
          stv(r2 + i, vr[q], nt);
          acc_rr += vr[q].x * vr[q].x;
          acc_rr += vr[q].y * vr[q].y;
          acc_rho += vt[q].x * vr[q].x;
          acc_rho += vt[q].y * vr[q].y;
        }
      }
    }
  }
  });
  if ((n & 1) && bx == 0 && threadIdx.x == 0) {
    const int64_t i = n - 1;
    if (!SECOND) {
      r[i] -= alpha * w[i];
    } else {
      const double ri = r_in ? r_in[i] : r[i];
      double vx = x[i] + alpha * p[i];
      vx += omega * ri;
      const double vr = ri - omega * w[i];
      x[i] = vx, r[i] = vr;
      acc_rr += vr * vr;
      acc_rho += rt[i] * vr;
    }
  }
  if (SECOND) {
    const double s0 = block_sum256(acc_rr, lds4);
    const double s1 = block_sum256(acc_rho, lds4);
    if (tickets.cnt == nullptr) {
      if (threadIdx.x == 0) partials[bx] = s0, partials[gridDim.x + bx] = s1;
      return;
    }
    if (threadIdx.x >= kWave) return;
    const double mine[2] = {s0, s1};
    double total[2];
    if (ticket_reduce_wave0<2>(tickets, mine, 2, bx, gridDim.x, total)) {
      if (use_ipc == 1) ipc_allreduce_wave<2>(ipc_w, total, 2);  // (peer windows: the global sums, the same bits on every rank)
      if (threadIdx.x == 0) {
        st->s[S_RR] = total[0], st->s[S_RHO_NEW] = total[1];
        st->s[S_OMEGA] = omega;  // (block 0's store of the same value need not be visible to this block yet)
        // (use_ipc == 2, RCCL: this rank's sums only -- the host enqueues the all-reduce and the step behind this kernel)
        if (use_ipc != 2) do_step(STEP_BICG_END, st, GmresDev{});  // :164, :116-118 and the convergence rule
      }
    }
  }
}


static int solve_bicgstab_body(const FusedSolveArgs &args) {
  const storm_hip_op *op = args.op;
  const double *b = args.b->d;
  double *x = args.x->d;
  Driver d;
  STORM_TRY(prepare_state(args, &d));
  storm_hip_ctx *c = d.c;
  const int64_t n = d.n;
  VecPool pool;
  if (res_eligible(op, true)) {  // (resident.hip)
    bool taken = false;
    STORM_TRY(pool.make(args.x, 1, false));  // the shadow residual
    STORM_TRY(res_solve(true, op, d.alpha, d.beta, b, x, pool.v[0]->d, c->d_state, &taken));
    if (taken) return ++c->n_resident_solves, collect(d, args, 2);
  }
  if (cg_latency_eligible(op)) {  // a small operator: the whole solve as one cooperative kernel (latency.hip)
    STORM_TRY(pool.make(args.x, 4));  // zero-filled: the kernel relies on that for the first direction
    double *const work[4] = {pool.v[0]->d, pool.v[1]->d, pool.v[2]->d, pool.v[3]->d};
    bool taken = false;
    STORM_TRY(bicgstab_latency_solve(op, d.alpha, d.beta, b, x, work, c->d_state, &taken));
    if (taken) return ++c->n_latency_solves, collect(d, args, 2);
  }
  ++c->n_throughput_solves;
  const size_t v0 = pool.v.size();
  // (s = r - alpha v formed inside the second apply -- the marching kernel without its x update -- was measured and dropped:
  //  452 against 445 us per iteration at 256^3; profiles/experiments/r08_pruned_experiments.patch)
  STORM_TRY(pool.make(args.x, 5, false));  // (r, rt: init; p: the copy of iteration 0; v, t: the SpMVs -- all before any read)
  double *p = pool.v[v0]->d, *r = pool.v[v0 + 1]->d, *rt = pool.v[v0 + 2]->d, *t = pool.v[v0 + 3]->d, *v = pool.v[v0 + 4]->d;
  const int nbv = stream_blocks(n);
  const int nbv2 = nbv;  // second half-step: one access per stream in flight, four trips per thread
  int nb = 0;

  // init: r = b - A x; rt = r; rho = <rt,r>           SolverBiCgStab.hpp:82-90
  STORM_TRY(d.apply(x, r, &nb, {}, false));
  STORM_TRY(d.init_residual(r, b, rt));
  STORM_TRY(d.finish(nbv, 1, S_RHO, STEP_BICG_INIT, true));
  // Sweep directions as in storm_hip_solve_cg: every streaming kernel starts at the end of the rows where its
  // predecessor stopped (what the Infinity Cache still holds); blocks keep their rows and partial slots.
  int dir = 1;
  auto flip = [&]() -> int { return dir ^= 1; };
  // ... and reductions finished in-kernel (see storm_hip_solve_cg): five launches per iteration instead of eleven.
  const bool tick = c->opt_ticket_reduce != 0 && c->comm == nullptr && nbv <= kTicketGroup * kTicketMaxGroups;
  // Peer windows: the applies leave per-wave partials; ONE small launch folds them, finishes the sum by tickets and exchanges
  // it with the other ranks (ipc_device.hpp); the update kernels form alpha / omega themselves and the second half-step's
  // last block all-reduces |r|^2, <rt, r> and runs the scalar step -- as on one rank, plus two small launches per iteration.
  const bool ipc_tick = c->opt_ticket_reduce != 0 && c->comm != nullptr && comm_ipc_next(c, &d.ipc_w) &&
                        nbv <= kTicketGroup * kTicketMaxGroups;
  // RCCL: the halo of the vector an update kernel is about to form leaves BEFORE that kernel (comm.hip)
  const bool early_halo = c->comm != nullptr && comm_is_rccl(c) && c->opt_rccl_early_halo != 0 && op->halo.n_nbrs > 0;
  // RCCL (option rccl_ticket): no scalar-step launch behind the all-reduces of <rt, v> and (<t, r>, <t, t>) -- the update
  // kernels (and the kernel that forms the halo of s) form alpha / omega themselves, as on one rank; the second half-step
  // finishes this rank's |r|^2 and <rt, r> by tickets, the all-reduce and the step follow it: four launches less per iteration
  // (ONE launch folds an apply's per-wave partials by tickets, the all-reduce follows)
  const bool rccl_tick = c->opt_ticket_reduce != 0 && c->opt_rccl_ticket != 0 && c->comm != nullptr && comm_is_rccl(c) &&
                         nbv <= kTicketGroup * kTicketMaxGroups;
  const Driver::Road allow = rccl_tick ? Driver::ROAD_TICKETS_RCCL : ipc_tick ? Driver::ROAD_TICKETS_IPC : Driver::ROAD_PLAIN;
  int ticketed = 0;
  auto apply_dir = [&](const double *xin, double *yout, const double *w, bool yy, int out0, int out1) -> int {
    c->spmv_reverse = flip();
    const int st_apply = d.apply(xin, yout, &nb, {.w = w, .yy = yy, .out0 = tick ? out0 : -1, .out1 = tick ? out1 : -1, .ticketed = &ticketed});
    c->spmv_reverse = 0;
    return st_apply;
  };
  // Everything of an iteration after the p update (iteration-invariant arguments).
  int64_t bi_it = 0;  // the iteration being enqueued (option ticket_verify)
  auto enqueue_rest = [&]() -> int {
    // v = A p; alpha = rho / <rt,v>                   :137-139
    STORM_TRY(apply_dir(p, v, rt, false, (int)S_RTV, -1));
    Driver::Road ran;
    const double *const rtv_with[1] = {v}, *const t_with[2] = {r, t};
    STORM_TRY(d.finish_dots(ticketed, nb, 1, S_RTV, rt, rtv_with, allow, STEP_BICG_ALPHA, &ran));
    const bool alpha_in_kernel = ran != Driver::ROAD_PLAIN;  // <rt,v> is in the slab; bicg_update forms alpha itself
    // (RCCL: the halo of s leaves now, under this update and the interior rows of the apply)
    //  (alpha not formed yet: the kernel that forms the rows to send divides rho by <rt, v> itself)
    if (early_halo)
      STORM_TRY(comm_halo_exchange_begin_formed(op, 0, r, nullptr, v, alpha_in_kernel ? d.slot(S_RHO) : d.slot(S_ALPHA),
                                                alpha_in_kernel ? d.slot(S_RTV) : nullptr, r,
                                                (alpha_in_kernel && c->opt_ticket_verify > 0) ? d.slot(S_ALPHA_SEEN) : nullptr));
    // r -= alpha v   (x += alpha p is applied in the second half-step)      :140-141
    hipLaunchKernelGGL(bicg_update_kernel<false>, dim3(nbv), dim3(kBlock), 0, c->stream, n, d.st, x, r, p, v, rt, c->d_partials,
                       stream_nt(c, n), flip(), alpha_in_kernel ? d.tickets() : TicketArgs{});
    HIP_TRY(hipGetLastError());
    // t = A r; omega = <t,r> / <t,t>                  :158-160
    STORM_TRY(apply_dir(r, t, r, true, (int)S_TR, (int)S_TT));
    STORM_TRY(d.finish_dots(ticketed, nb, 2, S_TR, t, t_with, allow, STEP_BICG_OMEGA, &ran));
    const bool omega_in_kernel = ran != Driver::ROAD_PLAIN, rccl_end = ran == Driver::ROAD_TICKETS_RCCL;
    // x = (x + alpha p) + omega r; r -= omega t; |r|, <rt,r>    :140, :161-164 (+ :116 of the next iteration)
    hipLaunchKernelGGL(bicg_update_kernel<true>, dim3(nbv2), dim3(kBlock), 0, c->stream, n, d.st, x, r, p, t, rt, c->d_partials,
                       stream_nt(c, n), flip(), omega_in_kernel ? d.tickets() : TicketArgs{}, (const double *)nullptr, d.ipc_w,
                       rccl_end ? 2 : (int)(ipc_tick && omega_in_kernel));
    HIP_TRY(hipGetLastError());
    if (!omega_in_kernel) {
      STORM_TRY(d.finish(nbv2, 2, S_RR, STEP_BICG_END));
    } else if (rccl_end) {
      STORM_TRY(comm_allreduce_sum(c, d.slot(S_RR), 2));
      STORM_TRY(d.step(STEP_BICG_END));
    } else if (c->opt_ticket_verify > 0 && bi_it % c->opt_ticket_verify == 0) {
      // |r|^2 and the next iteration's rho = <rt, r> as the second half-step's last block left them (it has run
      // STEP_BICG_END: rho_new sits in S_RHO, the counter is advanced)
      STORM_TRY(d.verify(r, r, rt, S_RR, S_RHO, (long long)(bi_it + 1)));
    }
    return STORM_HIP_OK;
  };
  auto enqueue_iteration = [&]() -> int {  // iterations >= 1
    // rho, beta were formed by STEP_BICG_END of the previous iteration (same r): :116-119
    if (early_halo) STORM_TRY(comm_halo_exchange_begin_formed(op, 1, r, p, v, d.slot(S_BETA), d.slot(S_OMEGA), p));
    c->stream_reverse = flip();
    const int st_p = k_bicg_p(c, p, r, dev_scal(d.slot(S_BETA)), dev_scal(d.slot(S_OMEGA)), v, n, d.done);
    c->stream_reverse = 0;
    STORM_TRY(st_p);
    return enqueue_rest();
  };
  for (int64_t it = 0; it < args.params->num_iterations; ++it) {
    bi_it = it;
    if (it == 0) {
      STORM_TRY(k_copy(c, p, r, n, d.done));  // :114
      STORM_TRY(enqueue_rest());
    } else {
      STORM_TRY(enqueue_iteration());
    }
    bool stop = false;
    STORM_TRY(post_and_poll(d, it, &stop));
    if (stop) break;
  }
  comm_forget_prebegun(c);
  return collect(d, args, 2);
}

}  // namespace storm

extern "C" int storm_hip_solve_bicgstab(const storm_hip_op *op, double alpha, double beta, const storm_hip_vec *b, storm_hip_vec *x,
                                        const storm_hip_solver_params *params, storm_hip_solver_result *result, double *history) {
  if (op) STORM_TRY(storm::lazy_sync(op->ctx));
  return storm::fused_solve(storm::FusedSolveArgs{op, alpha, beta, b, x, params, result, history, &storm::solve_bicgstab_body});
}
