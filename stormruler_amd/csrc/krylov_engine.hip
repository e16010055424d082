// The general Krylov engine, its statements: every member of KrylovEngine that enqueues work, and with them every launch of
// the engine's kernels (krylov_device.hpp is included here and nowhere else).  The methods written in these statements are
// in krylov_methods.hip, the host driving in krylov_abi.hip.
#include "krylov_device.hpp"

using namespace storm;
using namespace storm::kry;

// ---- picking a kernel instance from run-time values ----------------------------------------------------------------
// f(std::integral_constant<int, i>) for i in 1 .. N (anything above N counts as N), f(std::bool_constant<b>).
template <int N, class F>
static inline void with_int(int i, F &&f) {
  if constexpr (N == 1) f(std::integral_constant<int, 1>{});
  else if (i >= N) f(std::integral_constant<int, N>{});
  else with_int<N - 1>(i, f);
}
template <class F>
static inline void with_bool(bool b, F &&f) {
  if (b) f(std::true_type{});
  else f(std::false_type{});
}

// blocks for `items` at `per_block` each: at least one, at most `cap`
static inline int blocks_for(int64_t items, int64_t per_block, int64_t cap) {
  return (int)std::min<int64_t>(cap, std::max<int64_t>(1, (items + per_block - 1) / per_block));
}
// ... of a streaming statement over `streams` vectors (the kernels' U = lin_unroll(streams))
int K::lin_blocks(int streams, int64_t cap) const { return blocks_for(n, (int64_t)kBlock * lin_unroll(streams) * 2, cap); }

int storm::kry::callback_status(int st, const char *who) {
  if (st == 0) return STORM_HIP_OK;
  if (st > 0 || storm_hip_last_error()[0] == 0) set_error("%s returned %d", who, st);
  return st < 0 ? st : STORM_HIP_E_INVALID;
}

namespace {
struct ApiDone {  // library calls a callback makes are predicated on this solve's flag
  storm_hip_ctx *c;
  const int *saved;
  ApiDone(storm_hip_ctx *c_, const int *dp_) : c(c_), saved(c_->api_done) { c->api_done = dp_, ++c->callback_depth; }
  ~ApiDone() { c->api_done = saved, --c->callback_depth; }
};
}  // namespace

// -- scalar statements
void K::sc(uint16_t opc, int dd, int aa, int bb) {
  if (prog.n == kProgOps) flush();
  prog.ops[prog.n++] = SOp{opc, (uint16_t)dd, (uint16_t)aa, (uint16_t)bb};
}
int K::imm(double value) {
  if (n_imm == kProgImm || prog.n + 4 > kProgOps) flush();
  prog.imm[n_imm] = value;
  return kImm0 + n_imm++;
}

// May the held-back statement stay behind the scalar program about to go out?  0: no; 1: yes; 2: yes, and the
// program holds this iteration's convergence rule (the statement is then gated on the iteration counter).
int K::prog_lets_queued_wait() const {
  int verdict = 1;
  // (registers the pending REDUCTION writes directly count as written by the program that rides behind it)
  if (pend.kind != Pending::NONE)
    for (int j = 0; j < pend.k; ++j)
      for (int t = 0; t < 4; ++t)
        if (q_regs[t] == (int)pend.out.idx[j]) return 0;
  for (int i = 0; i < prog.n; ++i) {
    const SOp &o = prog.ops[i];
    if (o.op == SC_GIVENS || o.op == SC_BACKSOLVE || o.op == SC_BEGIN) return 0;  // (macros over register ranges; init)
    if (o.op == SC_ADVANCE) {
      verdict = 2;
      continue;
    }
    const int span = o.op == SC_SYMORTHO ? 3 : 1;
    for (int t = 0; t < 4; ++t)
      if (q_regs[t] >= (int)o.d && q_regs[t] < (int)o.d + span) return 0;
  }
  return verdict;
}
void K::settle() {  // the held-back statement goes out alone
  if (!q_has) return;
  q_has = false;
  if (!ok()) return;
  with_int<3>(q_nt, [&](auto nt) { launch_lin<decltype(nt)::value, false>(q_lin, q_gate); });
  q_gate = -1;
}
bool K::queued_touches(const double *ptr, bool written) const {  // would a statement on `ptr` conflict with it?
  if (!q_has || ptr == nullptr) return false;
  if (ptr == q_lin.y) return true;
  if (written)
    for (int t = 0; t < q_nt; ++t)
      if (ptr == q_lin.v[t]) return true;
  return false;
}
void K::settle_fd() {  // the held-back difference statement of the finite-difference product goes out alone
  if (!fd_held) return;
  fd_held = false;
  if (!ok() || n <= 0) return;
  hipLaunchKernelGGL(fd_diff_kernel, dim3(lin_blocks(2, 65536)), dim3(kBlock), 0, c->stream, n, fd_z, op.w->d, S + r_fd + 2, dp, stream_flags());
}

// The one place a reduction is filed: its kind, its grid, and the registers wanted of it (< 0: not wanted) in the
// kernel's order.  The caller has set the kernel's arguments in `pend`; flush() launches and clears it.
void K::file(Pending::Kind kind, int nb, const int *regs, int count) {
  pend.kind = kind, pend.nb = nb, pend.k = 0;
  for (int j = 0; j < count; ++j)
    if (regs[j] >= 0) pend.out.idx[pend.k++] = regs[j];
  if (pend.k == 0) pend.kind = Pending::NONE;
}

void K::flush(bool keep_queued) {
  settle_fd();  // (older than everything else that waits: apply() flushed before it ran the callback)
  if (q_has) {
    const int wait = (keep_queued && ok()) ? prog_lets_queued_wait() : 0;
    if (wait == 0) settle();
    else if (wait == 2) q_gate = (long long)cur_it + 1;
  }
  if (!ok()) return clear_pending();
  if (pend.kind == Pending::PARTIALS) {
    OutPtrs<kMaxMulti> out{}, scr{};  // (RCCL: the rank's sums go to the all-reduce slots; sprog_kernel moves them to their registers)
    for (int j = 0; j < pend.k; ++j) out.p[j] = S + pend.out.idx[j], scr.p[j] = S + R_SCR + j;
    const int st = k_reduce_finish(c, c->d_partials, pend.nb, pend.k, out, dp, ProgEpi{prog, S, d_st}, scr, [&]() -> int {
      STORM_TRY(comm_allreduce_sum(c, S + R_SCR, pend.k));
      hipLaunchKernelGGL(sprog_kernel, dim3(1), dim3(1), 0, c->stream, S, d_st, prog, pend.k, pend.out, (int)R_SCR, dp);
      return STORM_HIP_OK;
    });
    if (st != STORM_HIP_OK) fail(st);
  } else if (pend.kind != Pending::NONE) {
    const FinalPass f{c->d_tickets, c->d_ticket_sums, pend.k, pend.out, S, d_st, prog};
    const Pending &P = pend;
    const dim3 g(P.nb), b(kBlock);
    hipStream_t s = c->stream;
    double *parts = c->d_partials;
    switch (P.kind) {
      case Pending::DOTS:
        with_int<8>(P.k, [&](auto kb) { hipLaunchKernelGGL(dots_prog_kernel<decltype(kb)::value>, g, b, 0, s, n, P.a, P.bs, parts, dp, P.flags, f); });
        break;
      case Pending::VMUL_DOTS:
        hipLaunchKernelGGL(vmul_dots_prog_kernel, g, b, 0, s, n, P.z, P.d, P.r, parts, dp, P.flags, f);
        break;
      case Pending::FD_DIFF:
        with_bool(P.w != nullptr, [&](auto hasw) {
          hipLaunchKernelGGL(fd_diff_dots_prog_kernel<decltype(hasw)::value>, g, b, 0, s, n, P.z, P.r, P.w, S + r_fd + 2, P.yy, parts, dp, P.flags, f);
        });
        break;
      case Pending::LIN_DOT:
        with_int<3>(P.nt, [&](auto nt) {
          with_bool(P.w != nullptr, [&](auto hasw) {
            hipLaunchKernelGGL((lin_dot_prog_kernel<decltype(nt)::value, decltype(hasw)::value>), g, b, 0, s, n, P.lin, P.w, P.yy, parts, dp, P.flags, f);
          });
        });
        break;
      default:  // LIN2_DOT
        with_int<3>(P.nt0, [&](auto nt0) {
          with_int<3>(P.nt, [&](auto nt) {
            with_bool(P.w != nullptr, [&](auto hasw) {
              hipLaunchKernelGGL((lin2_dot_prog_kernel<decltype(nt0)::value, decltype(nt)::value, decltype(hasw)::value>), g, b, 0, s, n, P.lin0, P.lin, P.w, P.yy, parts, dp, P.flags, f);
            });
          });
        });
    }
  } else if (prog.n > 0) {
    hipLaunchKernelGGL(sprog_kernel, dim3(1), dim3(1), 0, c->stream, S, d_st, prog, 0, RedOut{}, 0, dp);
  }
  pend.kind = Pending::NONE;
  reset_prog();
  if (hipGetLastError() != hipSuccess) {
    set_error("krylov: kernel launch failed");
    fail(STORM_HIP_E_HIP);
  }
}

// -- reductions: reg_j = <a, b_j>
// The reductions of z behind a finite-difference product -- <z, z> and / or <z, u> for ONE other vector u -- ride in
// the pass of its held-back difference statement (fd_diff_dots_prog_kernel).  Same rule as a held-back lin: option
// lin_fuse, the one-launch reductions, and a request of exactly that shape; otherwise the statement leaves alone.
bool K::fd_dots(const storm_hip_vec *a, const DotOuts &outs) {
  if (!fd_held || !ok() || a->d != fd_z || c->opt_lin_fuse == 0 || !one_launch(2) || n <= 0) return false;
  if (prog.n > 0 || pend.kind != Pending::NONE || q_has) return false;  // (scalar statements issued since the product come first)
  int reg_zz = -1, reg_zu = -1;
  const double *u = nullptr;
  for (const auto &o : outs) {
    if (o.second->d == fd_z) {
      if (reg_zz >= 0) return false;
      reg_zz = o.first;
    } else {
      if (reg_zu >= 0) return false;
      reg_zu = o.first, u = o.second->d;
    }
  }
  if (outs.empty() || outs.size() > 2) return false;
  fd_held = false;  // (nothing else waits: apply() flushed before the callback, and nothing was issued since)
  ++c->n_fd_fused_dots;
  const int nb = lin_blocks(2 + (u != nullptr ? 1 : 0), std::min<int64_t>(32768, c->partials_capacity / 2));
  pend.z = fd_z, pend.r = op.w->d, pend.w = u, pend.yy = (int)(reg_zz >= 0), pend.flags = stream_flags();
  file(Pending::FD_DIFF, nb, {reg_zz, u != nullptr ? reg_zu : -1});
  return true;
}
void K::dots_v(const storm_hip_vec *a, const DotOuts &outs) {
  if (fd_dots(a, outs)) return;
  bool overtake = !queued_touches(a->d, false);  // a pure read: conflicts only with the held-back statement's target
  for (const auto &o : outs) overtake = overtake && !queued_touches(o.second->d, false);
  flush(overtake);
  if (!ok()) return;
  const int k = (int)outs.size();
  if (k < 1 || k > kMaxMulti) {
    set_error("krylov: %d simultaneous reductions (limit %d)", k, kMaxMulti);
    return fail(STORM_HIP_E_UNSUPPORTED);
  }
  const double *bs[kMaxMulti];
  int regs[kMaxMulti];
  // (every register here is >= 0 -- a literal one, or through wanted(): file() would drop one < 0 and pend.k fall short of k)
  for (int j = 0; j < k; ++j) bs[j] = outs[j].second->d, regs[j] = outs[j].first;
  if (one_launch(k)) {  // small: the partials kernel goes out at flush(), with the final pass in its last block
    int nb = stream_blocks(n);
    if ((int64_t)nb * k > c->partials_capacity) nb = (int)(c->partials_capacity / k);
    if ((int64_t)k * ((nb + kTicketGroup - 1) / kTicketGroup) <= (int64_t)8 * kTicketMaxGroups) {
      pend.a = a->d, pend.flags = stream_flags();
      for (int j = 0; j < kDotChunk; ++j) pend.bs.b[j] = bs[j < k ? j : 0];
      return file(Pending::DOTS, nb, regs, k);
    }
  }
  int nb = 1;
  if (n == 0) {  // an empty rank still takes part in the all-reduce
    const int st = (int)hipMemsetAsync(c->d_partials, 0, sizeof(double) * (size_t)k, c->stream);
    if (st != 0) return fail(STORM_HIP_E_HIP);
  } else {
    c->stream_reverse = flip();
    const int st = k_multi_dot_partials(c, a->d, bs, k, n, &nb, dp);
    c->stream_reverse = 0;
    if (st != STORM_HIP_OK) return fail(st);
  }
  file(Pending::PARTIALS, nb, regs, k);
}

// -- vector statements
template <int NT, bool NESTED>
void K::launch_lin(const LinArgs &a, long long gate) {
  if (n <= 0) return;
  hipLaunchKernelGGL((lin_kernel<NT, NESTED>), dim3(lin_blocks(NT, 65536)), dim3(kBlock), 0, c->stream, n, a, dp, stream_flags(),
                     gate >= 0 ? &d_st->iteration : nullptr, gate);
}
void K::launch_lin2(const LinArgs &a1, int nt1, const LinArgs &a2, int nt2) {
  const dim3 g(blocks_for(n >> 1, kBlock, 131072));
  const int fl = stream_flags();
  const long long *gp = q_gate >= 0 ? &d_st->iteration : nullptr;
  const long long gv = q_gate;
  with_int<3>(nt1, [&](auto n1) {
    with_int<3>(nt2, [&](auto n2) { hipLaunchKernelGGL((lin2_kernel<decltype(n1)::value, decltype(n2)::value>), g, dim3(kBlock), 0, c->stream, n, a1, a2, dp, fl, gp, gv); });
  });
  q_gate = -1;
}
void K::lin_v(V yv, const std::vector<Term> &terms, int cond) {
  if (c->opt_lin_fuse != 0 && terms.size() >= 1 && terms.size() <= 3 && n > 1) {
    flush(true);
    if (!ok()) return;
    LinArgs a{};
    a.y = yv->d;
    a.cond = cond >= 0 ? S + cond : nullptr;
    const int nt = (int)terms.size();
    int regs[4] = {-1, -1, -1, cond};
    for (int t = 0; t < nt; ++t) a.v[t] = terms[(size_t)t].v->d, a.c[t] = scal(terms[(size_t)t].c), regs[t] = terms[(size_t)t].c.reg;
    if (q_has) {  // the held-back statement and this one: one pass
      q_has = false;
      launch_lin2(q_lin, q_nt, a, nt);
    } else {
      q_has = true, q_lin = a, q_nt = nt;
      for (int t = 0; t < 4; ++t) q_regs[t] = regs[t];
    }
    return;
  }
  flush();
  if (!ok()) return;
  size_t at = 0;
  bool first = true;
  while (at < terms.size()) {
    LinArgs a{};
    a.y = yv->d;
    a.cond = cond >= 0 ? S + cond : nullptr;
    int nt = 0;
    if (!first) a.v[nt] = yv->d, a.c[nt] = Scal{nullptr, 1.0, 1.0}, ++nt;
    while (at < terms.size() && nt < 4) a.v[nt] = terms[at].v->d, a.c[nt] = scal(terms[at].c), ++nt, ++at;
    with_int<4>(nt, [&](auto k) { launch_lin<decltype(k)::value, false>(a); });
    first = false;
  }
}
// y = v0 + c1 * (v1 + c2 * v2)
void K::lin_nested(V yv, const storm_hip_vec *v0, Coef c1, const storm_hip_vec *v1, Coef c2, const storm_hip_vec *v2) {
  flush();
  if (!ok()) return;
  LinArgs a{};
  a.y = yv->d;
  a.v[0] = v0->d, a.v[1] = v1->d, a.v[2] = v2->d;
  a.c[0] = Scal{nullptr, 1.0, 1.0}, a.c[1] = scal(c1), a.c[2] = scal(c2);
  launch_lin<3, true>(a);
}
void K::divide(V yv, int reg) {
  flush();
  if (!ok()) return;
  c->stream_reverse = flip();
  const int st = k_scale(c, yv->d, n, dev_scal(S + reg), true, dp);
  c->stream_reverse = 0;
  if (st != STORM_HIP_OK) fail(st);
}

void K::lin_dots(V yv, std::initializer_list<Term> terms_il, int reg_yy, int reg_yw, const storm_hip_vec *wv) {
  std::vector<Term> terms(terms_il);
  if (terms.size() > 3 || n <= 0 || (wv != nullptr && wv == yv)) {  // not this kernel's shape: two statements
    lin_v(yv, terms);
    return dots_v(yv, wanted({{reg_yy, yv}, {reg_yw, wv}}));
  }
  bool overtake = !queued_touches(yv->d, true) && !(wv != nullptr && queued_touches(wv->d, false));
  for (const Term &t : terms) overtake = overtake && !queued_touches(t.v->d, false);
  // the held-back statement goes into THIS pass (it conflicts, so it cannot wait)
  bool with_held = q_has && !overtake && q_gate < 0 && q_lin.cond == nullptr && c->opt_lin_fuse != 0 && one_launch(2) && n > 1 &&
                   (reg_yy >= 0 || (reg_yw >= 0 && wv != nullptr));
  if (with_held) {
    flush(true);                         // (may still settle it: a scalar program in the way)
    with_held = q_has && q_gate < 0;
    if (q_has && !with_held) settle();
  } else {
    flush(overtake);
  }
  if (!ok()) return;
  LinArgs a{};
  a.y = yv->d;
  const int nt = (int)terms.size();
  for (int t = 0; t < nt; ++t) a.v[t] = terms[(size_t)t].v->d, a.c[t] = scal(terms[(size_t)t].c);
  const double *wd = (reg_yw >= 0 && wv != nullptr) ? wv->d : nullptr;
  // (the kernels' U counts w as a stream; with a held-back statement the grid is that of the statement alone: same rows
  //  per block, same partial sums)
  const int nb = lin_blocks(nt + (wd != nullptr ? 1 : 0), std::min<int64_t>(32768, c->partials_capacity / 2));
  const int yy = (int)(reg_yy >= 0);
  pend.lin = a, pend.nt = nt, pend.w = wd, pend.yy = yy, pend.flags = stream_flags();
  if (with_held) pend.lin0 = q_lin, pend.nt0 = q_nt, q_has = false;
  if (with_held || (one_launch(2) && (yy || wd != nullptr)))
    return file(with_held ? Pending::LIN2_DOT : Pending::LIN_DOT, nb, {reg_yy, wd != nullptr ? reg_yw : -1});
  with_int<3>(nt, [&](auto k) {
    with_bool(wd != nullptr, [&](auto hasw) {
      hipLaunchKernelGGL((lin_dot_kernel<decltype(k)::value, decltype(hasw)::value>), dim3(nb), dim3(kBlock), 0, c->stream, n, a, wd, yy, c->d_partials, dp, pend.flags);
    });
  });
  file(Pending::PARTIALS, nb, {reg_yy, wd != nullptr ? reg_yw : -1});
}

// -- operator and preconditioner
void K::apply_dots(V yv, const storm_hip_vec *xv, int reg_wy, const storm_hip_vec *wv, int reg_yy) {
  if (!(op.fuses_dots() && n > 0 && reg_wy >= 0)) {
    apply(yv, xv);
    return dots_v(yv, wanted({{reg_wy, wv}, {reg_yy, yv}}));
  }
  flush();
  if (!ok()) return;
  ++applies;
  int nblocks = 0;
  SpmvDot sd;
  sd.w = wv->d, sd.yy = reg_yy >= 0, sd.partials = c->d_partials, sd.nblocks_out = &nblocks;
  c->spmv_reverse = flip();
  const int st = spmv_launch(op.stencil, host_scal(op.alpha), host_scal(op.beta), xv->d, yv->d, &sd, dp);
  c->spmv_reverse = 0;
  if (st != STORM_HIP_OK) return fail(st);
  if (nblocks <= 0) return dots_v(yv, wanted({{reg_wy, wv}, {reg_yy, yv}}));  // the launch did not fuse after all
  file(Pending::PARTIALS, nblocks, {reg_wy, reg_yy});
}

void K::apply(V yv, const storm_hip_vec *xv) {
  if (op.is(Operator::FD)) return apply_fd(yv, xv);
  flush();
  if (!ok()) return;
  ++applies;
  int st;
  if (op.is(Operator::NATIVE)) {  // the SpMV itself: predicated, and dealt out from the end the last statement stopped at
    c->spmv_reverse = flip();
    st = spmv_launch(op.stencil, host_scal(op.alpha), host_scal(op.beta), xv->d, yv->d, nullptr, dp);
    c->spmv_reverse = 0;
  } else {  // the callback, or both stages as library launches, predicated like a callback's
    ApiDone guard(c, dp);
    st = op.apply_now(yv, xv, op_work);
    if (op.calls_back()) st = callback_status(st, "krylov: the operator callback");
  }
  if (st != STORM_HIP_OK) fail(st);
}
// z = J(y): four launches -- <y, y> with the scalar program that leaves delta and delta_inverse in their registers, the
// shift, the callback, the difference (held back: see fd_held) -- and no scalar on the host.
void K::apply_fd(V zv, const storm_hip_vec *yv) {
  dot(r_fd, yv, yv);
  sc(SC_SQRT, r_fd, r_fd);
  sc(SC_SDIV, r_fd + 1, r_fd + 3, r_fd);   // delta = safe_divide(mu, |y|)                  SolverNewton.hpp:144
  sc(SC_SDIV, r_fd + 2, R_ONE, r_fd + 1);  // delta_inverse = safe_divide(1, delta)         :147
  flush();
  if (!ok()) return;
  if (n > 0) {
    const int fl = stream_flags();
    with_bool(fl & 1, [&](auto nt) {
      hipLaunchKernelGGL(fd_shift_kernel<decltype(nt)::value>, dim3(stream_blocks(n)), dim3(kBlock), 0, c->stream, n, op_work->d, op.x->d, yv->d, S + r_fd + 1, dp, fl);
    });
  }
  ++applies;
  int st;
  {
    ApiDone guard(c, dp);
    st = op.apply_now(zv, op_work, nullptr);
  }
  st = callback_status(st, "krylov: the operator callback");
  if (st != STORM_HIP_OK) return fail(st);
  fd_held = true, fd_z = zv->d;
}
void K::pre(V yv, const storm_hip_vec *xv) {
  flush();
  if (!ok()) return;
  ++pre_applies;
  int st;
  ApiDone guard(c, dp);
  if (pre_fn != nullptr) {
    st = callback_status(pre_fn(pre_user, yv, xv), "krylov: the preconditioner callback");
  } else if (pre_cheb != nullptr) {  // (its launches are predicated on api_done like a callback's)
    st = storm_hip_cheb_apply(pre_cheb, xv, yv);
  } else if (pre_amg != nullptr) {
    st = storm_hip_amg_apply(pre_amg, xv, yv);
  } else {
    c->stream_reverse = flip();
    st = storm_hip_vmul(yv, pre_diag, xv);
    c->stream_reverse = 0;
  }
  if (st != STORM_HIP_OK) fail(st);
}
void K::pre_dots(V zv, const storm_hip_vec *rv, int reg_rz, int reg_rr) {
  if (pre_diag == nullptr || c->opt_lin_fuse == 0 || !one_launch(2) || zv == rv) {
    pre(zv, rv);
    return dots(rv, {{reg_rz, zv}, {reg_rr, rv}});
  }
  flush();
  if (!ok()) return;
  ++pre_applies;
  int nb = stream_blocks(n);
  if ((int64_t)nb * 2 > c->partials_capacity) nb = (int)(c->partials_capacity / 2);
  pend.z = zv->d, pend.d = pre_diag->d, pend.r = rv->d, pend.flags = stream_flags();
  file(Pending::VMUL_DOTS, nb, {reg_rz, reg_rr});
}
V K::vec() {
  storm_hip_vec *w = nullptr;
  if (ok()) {
    const int st = storm_hip_vec_create_like(x, &w);
    if (st != STORM_HIP_OK) fail(st);
  }
  work.push_back(w);
  return w;
}
