// The general Krylov engine: every solver of the reference's Solvers/ directory, for any operator
// (stencil operator or callback) and any preconditioner side, as a device-resident loop.
//
// What it stands in for (paths relative to the reference root): the bodies of
//   Solvers/SolverCg.hpp:54-126, SolverBiCgStab.hpp:59-165 and :195-367, SolverGmres.hpp:51-249,
//   SolverCgs.hpp:54-172, SolverTfqmr.hpp:41-204, SolverIdrs.hpp:60-281, SolverRichardson.hpp:48-96,
// driven by IterativeSolver::solve / InnerOuterIterativeSolver (Solver.hpp:116-147, :236-257).
//
// How it is built (nothing like the reference's host loops):
//   * A solver is written against a small ENGINE with three kinds of statements --
//       vector statements   y = sum_t c_t v_t   (one streaming kernel; c_t = host number or scalar REGISTER),
//                           y = A(x), y = P(x)  (stencil SpMV, or the caller's callback, which only enqueues),
//       reductions          reg_j = <a, b_j>    (batched partials kernel + one final pass),
//       scalar programs     short lists of micro-ops on the register file (safe_divide, sqrt, fma, compare,
//                           Givens / back-substitution macros, and the convergence rule of Solver.hpp:132-140)
//     The register file lives in HBM.  Scalar micro-ops are collected and ride in the kernel arguments of the final
//     pass of the reduction that precedes them (one launch for "finish the dot, divide, take the root, test for
//     convergence"), so a recurrence never costs the host a round trip.
//   * The host enqueues iterations ahead of the device and polls a pinned `done` ring `check_lag` iterations
//     behind; once the device's rule fires, every later kernel -- including those a callback enqueues, via
//     ctx->api_done -- returns at its first instruction, so x is frozen at exactly the reference's iteration.
//   * Multi-rank: a reduction's partial results are all-reduced (one call per batch) between the final pass and
//     the scalar program.
//
// This file: what the host fills in for the device, the operator value, the engine's data and its statement interface --
// no launch.  The other units (each says at its top what it holds): krylov_device.hpp, krylov_engine.hip, krylov_methods.hip, krylov_abi.hip.
#pragma once
#include <cmath>
#include <cstring>
#include <initializer_list>
#include <utility>
#include <vector>

#include "common.hpp"
#include "solver_device.hpp"
#include "blas1_device.hpp"

namespace storm {
namespace kry {

// ---- the scalar machine ---------------------------------------------------------------------------------
enum : uint16_t {
  SC_MOV,       // d = a
  SC_ADD,       // d = a + b
  SC_SUB,       // d = a - b
  SC_MUL,       // d = a * b
  SC_SDIV,      // d = safe_divide(a, b)          Crow/MathUtils.hpp:49-52
  SC_DIV,       // d = a / b
  SC_NEG,       // d = -a
  SC_SQRT,      // d = sqrt(a)
  SC_FMADD,     // d = d + a * b
  SC_FMSUB,     // d = d - a * b
  SC_LT,        // d = a < b ? 1 : 0
  SC_CMOV,      // d = (b != 0) ? a : d
  SC_SYMORTHO,  // (d, d+1, d+2) = (cs, sn, rr) of (a, b)   Crow/MathUtils.hpp:164-179
  SC_BEGIN,     // Solver.hpp:122-128 with initial error a
  SC_ADVANCE,   // Solver.hpp:132-140 with residual norm a
  SC_GIVENS,    // GMRES column a (an integer, not a register): H(a+1, a) = reg b; rotations; d = |beta_{a+1}|
  SC_BACKSOLVE  // GMRES: solve the a x a ... (a + 1) triangular system for beta (a an integer)
};
struct SOp {
  uint16_t op, d, a, b;
};
constexpr int kProgOps = 100;
constexpr int kProgImm = 8;
constexpr uint16_t kImm0 = 0xFFF0;  // operand codes kImm0 + i read imm[i]
struct SProg {
  int n;
  int aux[5];  // GMRES layout: H0, beta0, cs0, sn0, m (register indices)
  double imm[kProgImm];
  SOp ops[kProgOps];
};
struct RedOut {
  int idx[kMaxMulti];
};

// a vector statement as its kernel takes it
struct LinArgs {
  double *y;
  const double *v[4];
  Scal c[4];
  const double *cond;  // nullable: run only when *cond != 0
};


// ---- the engine ---------------------------------------------------------------------------------------------
struct Coef {  // a coefficient of a vector statement: a host number, or +-register
  int reg;
  double v, sign;
};
inline Coef R(int reg) { return Coef{reg, 0.0, 1.0}; }
inline Coef mR(int reg) { return Coef{reg, 0.0, -1.0}; }
inline Coef num(double v) { return Coef{-1, v, 1.0}; }
typedef storm_hip_vec *V;
struct Term {
  Coef c;
  const storm_hip_vec *v;
};
typedef std::vector<std::pair<int, const storm_hip_vec *>> DotOuts;  // reg_j = <a, b_j>: (register, b_j)

// registers every method has
enum { R_ZERO = 0, R_ONE, R_ERR, R_T0, R_T1, R_T2, R_T3, R_SCR /* kMaxMulti all-reduce slots */, R_USER = R_SCR + kMaxMulti };

// A callback's return value as a status, with a message where the callback left none: `who` = "krylov: the operator callback", ...
int callback_status(int st, const char *who);

// The operator of an engine, ONE value: a setter (storm_hip_krylov_set_operator*, jfnk_inner_solve) assigns a whole new one.
struct Operator {
  enum Kind { NONE, NATIVE, TWO_STAGE, CALLBACK, FD } kind = NONE;
  // NATIVE: A = beta I + alpha M;  TWO_STAGE: A = beta2 I + alpha2 M (beta I + alpha M)   (storm_hip_krylov_set_operator2)
  const storm_hip_op *stencil = nullptr;
  double alpha = 0.0, beta = 0.0, alpha2 = 0.0, beta2 = 0.0;
  // CALLBACK: A = fn;  FD: A = the finite-difference Jacobian of fn at x, with w = fn(x) (storm_hip_krylov_set_operator_fd):
  // z = (fn(x + delta y) - w) / delta, delta = safe_divide(mu, |y|).  mu: the host number, or the device word mu_dev.
  storm_hip_apply_fn fn = nullptr;
  void *user = nullptr;
  const storm_hip_vec *x = nullptr, *w = nullptr;
  double mu = 0.0;
  const double *mu_dev = nullptr;

  static Operator native(const storm_hip_op *op, double alpha, double beta) { return Operator{NATIVE, op, alpha, beta}; }
  static Operator stages2(const storm_hip_op *op, double alpha1, double beta1, double alpha2, double beta2) {
    return Operator{TWO_STAGE, op, alpha1, beta1, alpha2, beta2};
  }
  static Operator callback(storm_hip_apply_fn fn, void *user) { return Operator{CALLBACK, nullptr, 0.0, 0.0, 0.0, 0.0, fn, user}; }
  static Operator fd(storm_hip_apply_fn fn, void *user, const storm_hip_vec *x, const storm_hip_vec *w, double mu, const double *mu_dev) {
    return Operator{FD, nullptr, 0.0, 0.0, 0.0, 0.0, fn, user, x, w, mu, mu_dev};
  }
  bool is_set() const { return kind != NONE; }
  bool is(Kind k) const { return kind == k; }
  bool calls_back() const { return kind == CALLBACK || kind == FD; }
  bool fuses_dots() const { return kind == NATIVE && stencil->tail_rows == 0; }    // the SpMV's reduction epilogue
  bool needs_work_vector() const { return kind == TWO_STAGE || kind == FD; }       // per solve: the first stage's result / the shifted point
  // y = A(x) as the library call of the kind (FD: the callback it differentiates); t: the two-stage work vector, or null.
  int apply_now(storm_hip_vec *y, const storm_hip_vec *xv, storm_hip_vec *t) const {
    if (calls_back()) return fn(user, y, xv);
    if (kind == TWO_STAGE) return storm_hip_op_apply2(stencil, alpha, beta, alpha2, beta2, xv, t, y);
    return storm_hip_op_apply(stencil, alpha, beta, xv, y);
  }
};

// A reduction waiting for the scalar program behind it.  PARTIALS: the per-block partials are in c->d_partials already and
// flush() runs the final pass; every other kind: the partials kernel itself is launched at flush(), with the final pass
// and the scalar program inside.
struct Pending {
  enum Kind { NONE, PARTIALS, DOTS, LIN_DOT, LIN2_DOT, VMUL_DOTS, FD_DIFF } kind = NONE;
  int nb = 0, k = 0;  // grid (PARTIALS: blocks that wrote partials); sums
  RedOut out{};       // their registers
  // the kernel's arguments
  int flags = 0, yy = 0;
  double *z = nullptr;
  const double *d = nullptr, *r = nullptr, *a = nullptr, *w = nullptr;
  DotPtrs bs{};
  LinArgs lin{}, lin0{};  // (lin0: the held-back statement of LIN2_DOT)
  int nt = 0, nt0 = 0;
};

struct KrylovEngine {
  storm_hip_ctx *c = nullptr;
  int method = 0;
  // operator / preconditioner
  Operator op;
  storm_hip_apply_fn pre_fn = nullptr;
  void *pre_user = nullptr;
  const storm_hip_vec *pre_diag = nullptr;
  const storm_hip_cheb *pre_cheb = nullptr;  // the library's Chebyshev preconditioner (precond_cheb.hip): storm_hip_cheb_apply, no callback
  const storm_hip_amg *pre_amg = nullptr;    // the library's multigrid preconditioner (amg.hip): storm_hip_amg_apply, no callback
  int side = STORM_HIP_RIGHT;
  double relaxation = 1.0e-4;  // SolverRichardson.hpp:45
  // JFNK (STORM_HIP_JFNK): the inner BiCGStab engine, created with the object and reused by every Newton step
  storm_hip_krylov *jf_inner = nullptr;
  int64_t jf_inner_iterations = 0;
  unsigned long long my_ring_gen = 0;  // the generation state_init drew for THIS solve (a nested solve draws its own)
  // device state (own: solves may nest, e.g. a solver used as another solver's preconditioner)
  SolverState *d_st = nullptr, *h_st = nullptr;
  unsigned long long *h_ring = nullptr, *d_ring = nullptr;
  double *S = nullptr;
  int S_cap = 0, S_top = 0;
  double *d_history = nullptr;
  // the solve in progress
  const storm_hip_vec *b = nullptr;
  storm_hip_vec *x = nullptr;
  int64_t n = 0;
  int inner = 0, gram_schmidt = 0, lag = 4;
  std::vector<V> work;
  storm_hip_vec *op_work = nullptr;  // the operator's work vector (begin_solve): two-stage: the first stage's result; FD: the shifted point
  int r_fd = 0;                      // FD: registers <y, y> -> |y|, delta, delta_inverse, mu
  const int *dp = nullptr;           // predicate of the statements being enqueued (null: unconditional)
  int status = STORM_HIP_OK;
  int64_t it_enqueued = 0, applies = 0, pre_applies = 0;
  std::vector<int64_t> applies_after, pre_after;  // totals after init ([0]) and after each enqueued iteration
  bool stepping = false, active = false;
  // pending scalar program / reduction
  SProg prog{};
  int n_imm = 0;
  Pending pend;
  // The difference statement z = delta_inverse (z - w) of the last finite-difference product, held back: when the next thing the
  // method asks for is a reduction of z it rides in the statement's pass (dots_v), anything else makes it leave alone (flush).
  bool fd_held = false;
  double *fd_z = nullptr;
  // A vector statement held back (at most one): if the next statement is one too, both go out as ONE pass
  // (lin2_kernel); it may also be overtaken by a reduction that shares no vector with it.  It is older than any
  // pending reduction / scalar program, so launching it first is always right; holding it back past a program is
  // right when the program writes none of the registers its coefficients read.
  bool q_has = false;
  LinArgs q_lin{};
  int q_nt = 0;
  int q_regs[4] = {-1, -1, -1, -1};  // registers its coefficients (and its condition) read
  long long q_gate = -1;  // >= 0: held back past the convergence rule of iteration q_gate - 1 (see lin_kernel)
  int64_t cur_it = 0;     // the iteration iterate() is enqueuing
  // Sweep directions (see storm_hip_solve_cg): every streaming statement deals its blocks out from the end of the
  // rows where the previous one stopped -- what the Infinity Cache still holds.  Same rows and slots per block.
  int sweep_dir = 1;
  int flip() { return sweep_dir ^= 1; }
  int stream_flags() { return stream_nt(c, n) | (flip() << 1); }
  // per-method vectors and registers (krylov_methods.hip: each method's setup names the ones it uses)
  V p = nullptr, q = nullptr, r = nullptr, rt = nullptr, t = nullptr, u = nullptr, v = nullptr, y = nullptr, z = nullptr,
    d = nullptr, s_ = nullptr;
  std::vector<V> qs, zs, rs, us, ps, gs;
  int r_alpha = 0, r_beta = 0, r_rho = 0, r_omega = 0, r_gamma = 0, r_tau = 0, r_a0 = 0, r_a1 = 0, r_a2 = 0, r_a3 = 0,
      r_a4 = 0;
  int H0 = 0, B0 = 0, CS0 = 0, SN0 = 0, r_hn = 0;

  bool has_pre() const { return pre_fn != nullptr || pre_diag != nullptr || pre_cheb != nullptr || pre_amg != nullptr; }
  bool left() const { return has_pre() && side == STORM_HIP_LEFT; }
  bool right() const { return has_pre() && side == STORM_HIP_RIGHT; }
  bool ok() const { return status == STORM_HIP_OK; }
  void fail(int st) {
    if (status == STORM_HIP_OK) status = st;
  }
  int alloc(int count) {
    const int at = S_top;
    S_top += count;
    return at;
  }

  // ---- the statement interface (krylov_engine.hip) ----------------------------------------------------------------
  // -- scalar statements
  void sc(uint16_t opc, int dd, int aa = 0, int bb = 0);
  int imm(double value);
  void reset_prog() { prog.n = 0, n_imm = 0; }
  // everything that waits goes out (keep_queued: the held-back vector statement may stay where the program lets it)
  void flush(bool keep_queued = false);
  void clear_pending() { reset_prog(), pend.kind = Pending::NONE, q_has = false, fd_held = false; }
  // -- reductions: reg_j = <a, b_j>
  void dots(const storm_hip_vec *a, std::initializer_list<std::pair<int, const storm_hip_vec *>> outs) { dots_v(a, DotOuts(outs)); }
  void dots_v(const storm_hip_vec *a, const DotOuts &outs);
  void dot(int out, const storm_hip_vec *a, const storm_hip_vec *b2) { dots(a, {{out, b2}}); }
  static DotOuts wanted(std::initializer_list<DotOuts::value_type> all) {  // ... those of `all` with a register >= 0
    DotOuts outs;
    for (const auto &o : all)
      if (o.first >= 0) outs.push_back(o);
    return outs;
  }
  // -- vector statements: y = sum_t c_t v_t (cond >= 0: only when that register is not 0)
  void lin_v(V yv, const std::vector<Term> &terms, int cond = -1);
  void lin(V yv, std::initializer_list<Term> terms, int cond = -1) { lin_v(yv, std::vector<Term>(terms), cond); }
  void lin_nested(V yv, const storm_hip_vec *v0, Coef c1, const storm_hip_vec *v1, Coef c2, const storm_hip_vec *v2);
  void copy(V yv, const storm_hip_vec *xv, int cond = -1) { lin(yv, {{num(1.0), xv}}, cond); }
  void axpy(V yv, Coef a, const storm_hip_vec *xv) { lin(yv, {{num(1.0), yv}, {a, xv}}); }
  void scale(V yv, Coef a) { lin(yv, {{a, yv}}); }
  void divide(V yv, int reg);  // y /= reg (a true division per element, SolverGmres.hpp:88)
  // y = sum_t c_t v_t  AND  reg_yy = <y, y>, reg_yw = <y, w> of the new y (register < 0: not wanted), one pass.
  void lin_dots(V yv, std::initializer_list<Term> terms_il, int reg_yy, int reg_yw = -1, const storm_hip_vec *wv = nullptr);
  // -- operator and preconditioner
  void apply(V yv, const storm_hip_vec *xv);  // y = A(x)          Operator::mul, Operator.hpp:74
  // y = A(x)  AND  reg_wy = <w, y>, reg_yy = <y, y> (register < 0: not wanted): the stencil SpMV's fused epilogue
  // when the operator is native and has no CSR tail, separate reductions otherwise.
  void apply_dots(V yv, const storm_hip_vec *xv, int reg_wy, const storm_hip_vec *wv, int reg_yy = -1);
  void pre(V yv, const storm_hip_vec *xv);  // y = P(x)          Preconditioner::mul
  // z = P(r) AND reg_rz = <r, z>, reg_rr = <r, r>: one pass when the preconditioner is the library's diagonal one (any other
  // kind, the Chebyshev one included: pre, then dots).
  void pre_dots(V zv, const storm_hip_vec *rv, int reg_rz, int reg_rr);
  // The dispatch every preconditioned body repeats (chained mul, Operator.hpp:82-88):
  //   left: z = P(y = A x);  right: z = A(y = P x);  none: z = A x.
  void mul_side(V zv, V yv, const storm_hip_vec *xv) {
    if (left()) apply(yv, xv), pre(zv, yv);
    else if (right()) pre(yv, xv), apply(zv, yv);
    else apply(zv, xv);
  }
  void residual(V rv, const storm_hip_vec *bv, const storm_hip_vec *xv) {  // Operator::Residual, Operator.hpp:95-99
    apply(rv, xv);
    lin(rv, {{num(1.0), bv}, {num(-1.0), rv}});
  }
  V vec();  // a work vector like x, for this solve
  void norm_to_err_and(uint16_t what, const storm_hip_vec *a) {  // ERR = |a|; begin / advance
    dot(R_T0, a, a);
    sc(SC_SQRT, R_ERR, R_T0);
    sc(what, 0, R_ERR);
  }

  // ---- the solvers (krylov_methods.hip): one table row per method ---------------------------------------------------
  void setup();
  void init();
  void iterate(int64_t it);
  void finalize(int64_t iterations, bool forced);
  void cg_setup(), cg_init(), cg_iterate(int64_t it);
  void bicgstab_setup(), bicgstab_init(), bicgstab_iterate(int64_t it);
  void cgs_setup(), cgs_init(), cgs_iterate(int64_t it);
  void tfqmr_setup(), tfqmr_init(), tfqmr_iterate(int64_t it);
  void richardson_setup(), richardson_init(), richardson_iterate(int64_t it);
  void bicgstab_l_setup(), bicgstab_l_init(), bicgstab_l_iterate(int64_t it);
  void idrs_setup(), idrs_init(), idrs_iterate(int64_t it);
  void gmres_setup(), gmres_init(), gmres_iterate(int64_t it), gmres_finalize(int64_t iterations, bool forced);
  void gmres_start(bool outer), gmres_update_x(int k);
  void jfnk_setup(), jfnk_init(), jfnk_iterate(int64_t it);

 private:  // (krylov_engine.hip)
  int prog_lets_queued_wait() const;
  void settle();
  bool queued_touches(const double *ptr, bool written) const;
  void settle_fd();
  bool one_launch(int k) const { return c->comm == nullptr && c->opt_fused_reduce != 0 && n > 0 && k <= kDotChunk; }
  void file(Pending::Kind kind, int nb, const int *regs, int count);
  void file(Pending::Kind kind, int nb, std::initializer_list<int> regs) { file(kind, nb, regs.begin(), (int)regs.size()); }
  int lin_blocks(int streams, int64_t cap) const;
  bool fd_dots(const storm_hip_vec *a, const DotOuts &outs);
  Scal scal(const Coef &co) const { return co.reg >= 0 ? Scal{S + co.reg, 0.0, co.sign} : Scal{nullptr, co.v, 1.0}; }
  template <int NT, bool NESTED>
  void launch_lin(const LinArgs &a, long long gate = -1);
  void launch_lin2(const LinArgs &a1, int nt1, const LinArgs &a2, int nt2);
  void apply_fd(V zv, const storm_hip_vec *yv);
};

typedef KrylovEngine K;
int jfnk_inner_solve(K *outer);  // (krylov_abi.hip: the Newton step's inner solve, called by JFNK's iterate)

}  // namespace kry
}  // namespace storm

struct storm_hip_krylov : storm::kry::KrylovEngine {};  // the opaque handle of the C ABI
