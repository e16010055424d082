// The general Krylov engine, its methods: the ten solvers of the reference's Solvers/ directory, each restated in the
// engine's statements (krylov_engine.hpp) under the lines of the reference it stands for -- setup (the vectors and
// registers it names, allocated where the reference's init() allocates, e.g. SolverCg.hpp:57-59), init, iterate and,
// where it has one, finalize.  Host code only; kMethods at the end is the one way in.
#include "krylov_engine.hpp"

using namespace storm;
using namespace storm::kry;

// ---- CG: SolverCg.hpp:54-126 (takes no notice of pre_side) ----------------------------------------------------------
void K::cg_setup() {
  p = vec(), r = vec(), z = vec();
  r_gamma = alloc(1), r_alpha = alloc(1), r_beta = alloc(1), r_a0 = alloc(1), r_a1 = alloc(1);
}
void K::cg_init() {  // :54-84
  residual(r, b, x);
  if (has_pre()) {
    pre(z, r);
    copy(p, z);
    dots(r, {{r_gamma, z}, {R_T0, r}});
    sc(SC_SQRT, R_ERR, R_T0);
  } else {
    copy(p, r);
    dot(r_gamma, r, r);
    sc(SC_SQRT, R_ERR, r_gamma);
  }
  sc(SC_BEGIN, 0, R_ERR);
}
void K::cg_iterate(int64_t) {  // :86-126
  const bool P = has_pre();
  apply_dots(z, p, R_T0, p);
  sc(SC_SDIV, r_alpha, r_gamma, R_T0);
  sc(SC_MOV, r_a0, r_gamma);  // gamma_bar
  axpy(x, R(r_alpha), p);
  if (P) {
    axpy(r, mR(r_alpha), z);
    pre_dots(z, r, r_gamma, R_T1);
    sc(SC_SQRT, R_ERR, R_T1);
  } else {
    lin_dots(r, {{num(1.0), r}, {mR(r_alpha), z}}, r_gamma);
    sc(SC_SQRT, R_ERR, r_gamma);
  }
  sc(SC_SDIV, r_beta, r_gamma, r_a0);
  sc(SC_ADVANCE, 0, R_ERR);
  lin(p, {{num(1.0), P ? z : r}, {R(r_beta), p}});
}

// ---- BiCGStab: SolverBiCgStab.hpp:59-165 -----------------------------------------------------------------------------
void K::bicgstab_setup() {
  p = vec(), r = vec(), rt = vec(), t = vec(), v = vec();
  if (has_pre()) z = vec();
  r_alpha = alloc(1), r_beta = alloc(1), r_rho = alloc(1), r_omega = alloc(1), r_a0 = alloc(1), r_a1 = alloc(1),
  r_a2 = alloc(1);
}
void K::bicgstab_init() {  // :59-91
  residual(r, b, x);
  if (left()) std::swap(z, r), pre(r, z);
  copy(rt, r);
  dot(r_rho, rt, r);
  sc(SC_SQRT, R_ERR, r_rho);
  sc(SC_BEGIN, 0, R_ERR);
}
void K::bicgstab_iterate(int64_t it) {  // :93-165
  const bool P = has_pre();
  if (it == 0) {
    copy(p, r);
  } else {
    lin_nested(p, r, R(r_beta), p, mR(r_omega), v);  // (rho, beta: formed at the end of the previous iteration)
  }
  if (left()) {
    mul_side(v, z, p);
    dot(R_T0, rt, v);
  } else {  // the operator is applied last: its reduction rides in the SpMV
    if (right()) pre(z, p);
    apply_dots(v, right() ? z : p, R_T0, rt);
  }
  sc(SC_SDIV, r_alpha, r_rho, R_T0);
  // (:140, :161: without a preconditioner p and s = r are still there when omega is known, and
  //  x = (x + alpha p) + omega s goes out as ONE statement below -- the same two roundings per element)
  if (P) axpy(x, R(r_alpha), right() ? z : p);
  axpy(r, mR(r_alpha), v);
  if (left()) {
    mul_side(t, z, r);
    dots(t, {{R_T0, r}, {R_T1, t}});
  } else {
    if (right()) pre(z, r);
    apply_dots(t, right() ? z : r, R_T0, r, R_T1);
  }
  sc(SC_SDIV, r_omega, R_T0, R_T1);
  if (P) axpy(x, R(r_omega), right() ? z : r);
  else lin(x, {{num(1.0), x}, {R(r_alpha), p}, {R(r_omega), r}});
  lin_dots(r, {{num(1.0), r}, {mR(r_omega), t}}, R_T0, r_a1, rt);  // |r|^2 and the next iteration's <rt, r>
  sc(SC_SQRT, R_ERR, R_T0);
  sc(SC_ADVANCE, 0, R_ERR);
  // :116-118 of the NEXT iteration (the same r): rho_bar = rho; rho = <rt, r>; beta = (alpha rho) / (omega rho_bar)
  // -- in this pass's scalar program instead of a launch of their own at the start of the next iteration
  sc(SC_MOV, r_a0, r_rho);
  sc(SC_MOV, r_rho, r_a1);
  sc(SC_MUL, R_T0, r_alpha, r_rho);
  sc(SC_MUL, R_T1, r_omega, r_a0);
  sc(SC_SDIV, r_beta, R_T0, R_T1);
}

// ---- CGS: SolverCgs.hpp:54-172 ---------------------------------------------------------------------------------------
void K::cgs_setup() {
  p = vec(), q = vec(), r = vec(), rt = vec(), u = vec(), v = vec();
  r_alpha = alloc(1), r_beta = alloc(1), r_rho = alloc(1), r_a0 = alloc(1), r_a1 = alloc(1);
}
void K::cgs_init() {  // :54-88
  residual(r, b, x);
  if (left()) std::swap(u, r), pre(r, u);
  copy(rt, r);
  dot(r_rho, rt, r);
  sc(SC_SQRT, R_ERR, r_rho);
  sc(SC_BEGIN, 0, R_ERR);
}
void K::cgs_iterate(int64_t it) {  // :90-172
  if (it == 0) {
    copy(u, r);
    copy(p, u);
  } else {
    lin(u, {{num(1.0), r}, {R(r_beta), q}});  // (rho, beta: formed at the end of the previous iteration)
    lin_nested(p, u, R(r_beta), q, R(r_beta), p);
  }
  mul_side(v, q, p);
  dot(R_T0, rt, v);
  sc(SC_SDIV, r_alpha, r_rho, R_T0);
  lin(q, {{num(1.0), u}, {mR(r_alpha), v}});
  lin(v, {{num(1.0), u}, {num(1.0), q}});
  const storm_hip_vec *step = v;  // what r loses alpha times of
  if (left()) {
    axpy(x, R(r_alpha), v);
    apply(u, v), pre(v, u);
  } else if (right()) {
    pre(u, v), apply(v, u);
    axpy(x, R(r_alpha), u);
  } else {
    apply(u, v);
    axpy(x, R(r_alpha), v);
    step = u;
  }
  lin_dots(r, {{num(1.0), r}, {mR(r_alpha), step}}, R_T0, r_a1, rt);  // |r|^2 and the next iteration's <rt, r>
  sc(SC_SQRT, R_ERR, R_T0);
  sc(SC_ADVANCE, 0, R_ERR);
  sc(SC_MOV, r_a0, r_rho);  // SolverCgs.hpp:116-118 of the next iteration, in this pass's scalar program
  sc(SC_MOV, r_rho, r_a1);
  sc(SC_SDIV, r_beta, r_rho, r_a0);
}

// ---- TFQMR and TFQMR1: SolverTfqmr.hpp:41-204 ------------------------------------------------------------------------
void K::tfqmr_setup() {
  d = vec(), rt = vec(), u = vec(), v = vec(), y = vec(), s_ = vec();
  if (has_pre()) z = vec();
  r_alpha = alloc(1), r_beta = alloc(1), r_rho = alloc(1), r_tau = alloc(1), r_omega = alloc(1), r_a0 = alloc(1),
  r_a1 = alloc(3), r_a2 = alloc(1), r_a3 = alloc(1), r_a4 = alloc(1);
}
void K::tfqmr_init() {  // :41-87
  if (method == STORM_HIP_TFQMR1) copy(d, x);
  residual(y, b, x);
  if (left()) std::swap(z, y), pre(y, z);
  copy(u, y);
  copy(rt, u);
  dot(r_rho, rt, u);
  sc(SC_SQRT, r_tau, r_rho);
  sc(SC_BEGIN, 0, r_tau);
}
void K::tfqmr_iterate(int64_t it) {  // :89-204
  const bool l1 = method == STORM_HIP_TFQMR1;
  if (it == 0) {
    mul_side(s_, z, y);
    copy(v, s_);
  } else {
    sc(SC_MOV, r_a0, r_rho);
    sc(SC_MOV, r_rho, r_a4);  // <rt, u>: formed in the pass that produced this u (second half-step below)
    sc(SC_SDIV, r_beta, r_rho, r_a0);
    lin(v, {{num(1.0), s_}, {R(r_beta), v}});
    lin(y, {{num(1.0), u}, {R(r_beta), y}});
    mul_side(s_, z, y);
    lin(v, {{num(1.0), s_}, {R(r_beta), v}});
  }
  dot(R_T0, rt, v);
  sc(SC_SDIV, r_alpha, r_rho, R_T0);
  for (int half = 0; half <= 1; ++half) {
    axpy(d, R(r_alpha), right() ? z : y);
    if (half == 1) lin_dots(u, {{num(1.0), u}, {mR(r_alpha), s_}}, R_T0, r_a4, rt);  // + the next <rt, u>
    else lin_dots(u, {{num(1.0), u}, {mR(r_alpha), s_}}, R_T0);
    sc(SC_SQRT, r_omega, R_T0);
    if (l1) {
      sc(SC_LT, r_a2, r_omega, r_tau);
      sc(SC_CMOV, r_tau, r_omega, r_a2);
      copy(x, d, r_a2);
    } else {
      sc(SC_SYMORTHO, r_a1, r_tau, r_omega);  // (cs, sn, rr) in r_a1 .. r_a1 + 2
      sc(SC_MUL, r_tau, r_omega, r_a1);
      sc(SC_MUL, r_a2, r_a1, r_a1);            // cs^2
      sc(SC_MUL, r_a3, r_a1 + 1, r_a1 + 1);    // sn^2
      axpy(x, R(r_a2), d);
      scale(d, R(r_a3));
    }
    if (half == 0) {
      axpy(y, mR(r_alpha), v);
      mul_side(s_, z, y);
    }
  }
  if (l1) {
    sc(SC_ADVANCE, 0, r_tau);
  } else {
    sc(SC_MUL, R_ERR, r_tau, imm(std::sqrt(2.0 * (double)it + 3.0)));
    sc(SC_ADVANCE, 0, R_ERR);
  }
}

// ---- Richardson: SolverRichardson.hpp:48-96 (no notice of pre_side either) -------------------------------------------
void K::richardson_setup() {
  r = vec();
  if (has_pre()) z = vec();
}
void K::richardson_init() {  // :48-71
  residual(r, b, x);
  if (has_pre()) std::swap(z, r), pre(r, z);
  norm_to_err_and(SC_BEGIN, r);
}
void K::richardson_iterate(int64_t) {  // :73-96
  axpy(x, num(relaxation), r);
  residual(r, b, x);
  if (has_pre()) std::swap(z, r), pre(r, z);
  norm_to_err_and(SC_ADVANCE, r);
}

// ---- BiCGStab(l): SolverBiCgStab.hpp:195-367 (always left) ------------------------------------------------------------
void K::bicgstab_l_setup() {
  const int l = inner;
  rt = vec();
  if (has_pre()) z = vec();
  rs.clear(), us.clear();
  for (int i = 0; i <= l; ++i) rs.push_back(vec()), us.push_back(vec());
  r_alpha = alloc(1), r_beta = alloc(1), r_rho = alloc(1), r_omega = alloc(1), r_a0 = alloc(1);
  r_gamma = alloc(l + 1);           // gamma
  r_a1 = alloc(l + 1);              // gamma_bar
  r_a2 = alloc(l + 1);              // gamma_bbar
  r_a3 = alloc(l + 1);              // sigma
  r_a4 = alloc((l + 1) * (l + 1));  // tau
}
void K::bicgstab_l_init() {  // :195-233
  residual(rs[0], b, x);
  if (has_pre()) std::swap(z, rs[0]), pre(rs[0], z);
  copy(rt, rs[0]);
  dot(r_rho, rt, rs[0]);
  sc(SC_SQRT, R_ERR, r_rho);
  sc(SC_BEGIN, 0, R_ERR);
}
void K::bicgstab_l_iterate(int64_t it) {  // :235-367
  const bool P = has_pre();
  const int l = inner, j = (int)(it % l);
  const int G = r_gamma, GB = r_a1, GBB = r_a2, SG = r_a3;
  auto TAU = [&](int i, int jj) { return r_a4 + i * (l + 1) + jj; };
  if (it == 0) {
    copy(us[0], rs[0]);
  } else {
    sc(SC_MOV, r_a0, r_rho);
    dot(r_rho, rt, rs[j]);
    sc(SC_MUL, R_T0, r_alpha, r_rho);
    sc(SC_SDIV, r_beta, R_T0, r_a0);
    for (int i = 0; i <= j; ++i) lin(us[i], {{num(1.0), rs[i]}, {mR(r_beta), us[i]}});
  }
  if (P) apply(z, us[j]), pre(us[j + 1], z);
  else apply(us[j + 1], us[j]);
  dot(R_T0, rt, us[j + 1]);
  sc(SC_SDIV, r_alpha, r_rho, R_T0);
  for (int i = 0; i <= j; ++i) axpy(rs[i], mR(r_alpha), us[i + 1]);
  axpy(x, R(r_alpha), us[0]);
  if (P) apply(z, rs[j]), pre(rs[j + 1], z);
  else apply(rs[j + 1], rs[j]);
  if (j == l - 1) {
    for (int jj = 1; jj <= l; ++jj) {
      for (int i = 1; i < jj; ++i) {
        dot(R_T0, rs[i], rs[jj]);
        sc(SC_SDIV, TAU(i, jj), R_T0, SG + i);
        axpy(rs[jj], mR(TAU(i, jj)), rs[i]);
      }
      dots(rs[jj], {{SG + jj, rs[jj]}, {R_T0, rs[0]}});
      sc(SC_SDIV, GB + jj, R_T0, SG + jj);
    }
    sc(SC_MOV, G + l, GB + l);
    sc(SC_MOV, r_omega, G + l);
    sc(SC_NEG, R_T0, r_omega);
    sc(SC_MUL, r_rho, r_rho, R_T0);
    for (int jj = l - 1; jj != 0; --jj) {
      sc(SC_MOV, G + jj, GB + jj);
      for (int i = jj + 1; i <= l; ++i) sc(SC_FMSUB, G + jj, TAU(jj, i), G + i);
    }
    for (int jj = 1; jj < l; ++jj) {
      sc(SC_MOV, GBB + jj, G + jj + 1);
      for (int i = jj + 1; i < l; ++i) sc(SC_FMADD, GBB + jj, TAU(jj, i), G + i + 1);
    }
    axpy(x, R(G + 1), rs[0]);
    axpy(rs[0], mR(GB + l), rs[l]);
    axpy(us[0], mR(G + l), us[l]);
    for (int jj = 1; jj < l; ++jj) {
      axpy(x, R(GBB + jj), rs[jj]);
      axpy(rs[0], mR(GB + jj), rs[jj]);
      axpy(us[0], mR(G + jj), us[jj]);
    }
  }
  norm_to_err_and(SC_ADVANCE, rs[0]);
}

// ---- IDR(s): SolverIdrs.hpp:60-281 ------------------------------------------------------------------------------------
void K::idrs_setup() {
  const int s = inner;
  r = vec(), v = vec();
  if (has_pre()) z = vec();
  ps.clear(), us.clear(), gs.clear();
  for (int i = 0; i < s; ++i) ps.push_back(vec()), us.push_back(vec()), gs.push_back(vec());
  r_omega = alloc(1), r_alpha = alloc(1), r_beta = alloc(1);
  r_a0 = alloc(s);      // phi
  r_gamma = alloc(s);   // gamma
  r_a1 = alloc(s * s);  // mu
}
void K::idrs_init() {  // :60-106
  residual(r, b, x);
  if (left()) std::swap(z, r), pre(r, z);
  dot(R_T0, r, r);
  sc(SC_SQRT, r_a0, R_T0);
  sc(SC_BEGIN, 0, r_a0);
}
void K::idrs_iterate(int64_t it) {  // :109-281
  const int s = inner, k = (int)(it % s);
  const int PHI = r_a0, GAM = r_gamma;
  auto MU = [&](int i, int jj) { return r_a1 + i * s + jj; };
  if (k == 0) {  // inner_init :109-156
    if (it == 0) {
      sc(SC_MOV, r_omega, R_ONE);
      sc(SC_MOV, MU(0, 0), R_ONE);
      copy(ps[0], r);
      divide(ps[0], PHI);
      for (int i = 1; i < s; ++i) {
        sc(SC_MOV, MU(i, i), R_ONE);
        sc(SC_MOV, PHI + i, R_ZERO);
        flush();
        if (ok()) {
          const int st = storm_hip_fill_randomly(ps[i]);
          if (st != STORM_HIP_OK) fail(st);
        }
        for (int jj = 0; jj < i; ++jj) {
          sc(SC_MOV, MU(i, jj), R_ZERO);
          dot(R_T0, ps[i], ps[jj]);
          axpy(ps[i], mR(R_T0), ps[jj]);
        }
        dot(R_T0, ps[i], ps[i]);
        sc(SC_SQRT, R_T1, R_T0);
        divide(ps[i], R_T1);
      }
    } else {
      std::vector<std::pair<int, const storm_hip_vec *>> outs;
      for (int i = 0; i < s; ++i) outs.push_back({PHI + i, ps[i]});
      dots_v(r, outs);
    }
  }
  for (int i = k; i < s; ++i) {  // :182-188
    sc(SC_MOV, GAM + i, PHI + i);
    for (int jj = k; jj < i; ++jj) sc(SC_FMSUB, GAM + i, MU(i, jj), GAM + jj);
    sc(SC_DIV, GAM + i, GAM + i, MU(i, i));
  }
  {
    std::vector<Term> tv{{num(1.0), r}};
    for (int i = k; i < s; ++i) tv.push_back({mR(GAM + i), gs[i]});
    lin_v(v, tv);  // :200-203
  }
  if (right()) std::swap(z, v), pre(v, z);
  {
    std::vector<Term> tu{{R(r_omega), v}, {R(GAM + k), us[k]}};
    for (int i = k + 1; i < s; ++i) tu.push_back({R(GAM + i), us[i]});
    lin_v(us[k], tu);  // :208-211
  }
  if (left()) apply(z, us[k]), pre(gs[k], z);
  else apply(gs[k], us[k]);
  for (int i = 0; i < k; ++i) {  // :230-235
    dot(R_T0, ps[i], gs[k]);
    sc(SC_SDIV, r_alpha, R_T0, MU(i, i));
    axpy(us[k], mR(r_alpha), us[i]);
    axpy(gs[k], mR(r_alpha), gs[i]);
  }
  {
    std::vector<std::pair<int, const storm_hip_vec *>> outs;
    for (int i = k; i < s; ++i) outs.push_back({MU(i, k), ps[i]});
    dots_v(gs[k], outs);  // :236-238
  }
  sc(SC_SDIV, r_beta, PHI + k, MU(k, k));
  for (int i = k + 1; i < s; ++i) sc(SC_FMSUB, PHI + i, r_beta, MU(i, k));
  axpy(x, R(r_beta), us[k]);
  axpy(r, mR(r_beta), gs[k]);
  if (k == s - 1) {  // :256-279
    mul_side(v, z, r);
    dots(v, {{R_T0, r}, {R_T1, v}});
    sc(SC_SDIV, r_omega, R_T0, R_T1);
    axpy(x, R(r_omega), right() ? z : r);
    axpy(r, mR(r_omega), v);
  }
  norm_to_err_and(SC_ADVANCE, r);
}

// ---- GMRES and FGMRES: SolverGmres.hpp:51-249 inside Solver.hpp:236-257 ---------------------------------------------------
void K::gmres_setup() {
  const bool P = has_pre();
  const int m = inner;
  qs.clear(), zs.clear();
  for (int i = 0; i <= m; ++i) qs.push_back(vec());
  if (P) {
    const int nz = method == STORM_HIP_FGMRES ? m : 1;
    for (int i = 0; i < nz; ++i) zs.push_back(vec());
  }
  r_hn = alloc(1);
  B0 = alloc(m + 1), CS0 = alloc(m), SN0 = alloc(m);
  r_a0 = alloc(2 * kMaxMulti);  // classical Gram-Schmidt x2: the two passes' coefficients
  H0 = alloc((m + 1) * m);
}
// q0 = b - A x [left: q0 = P(b - A x)]; beta0 = |q0|; q0 /= beta0      (outer_init :82-90 and inner_init :110-116)
void K::gmres_start(bool outer) {
  const bool lp = has_pre() && method == STORM_HIP_GMRES && side == STORM_HIP_LEFT;
  residual(qs[0], b, x);
  if (lp) {
    std::swap(zs[0], qs[0]);
    pre(qs[0], zs[0]);
  }
  dot(R_T0, qs[0], qs[0]);
  sc(SC_SQRT, B0, R_T0);
  if (outer) sc(SC_BEGIN, 0, B0);
  divide(qs[0], B0);
}

// x += sum_i beta_i q_i after the back substitution (inner_finalize :194-249)
void K::gmres_update_x(int k) {
  const bool rp = has_pre() && (method == STORM_HIP_FGMRES || side == STORM_HIP_RIGHT);
  prog.aux[0] = H0, prog.aux[1] = B0, prog.aux[2] = CS0, prog.aux[3] = SN0, prog.aux[4] = inner;
  sc(SC_BACKSOLVE, 0, k);
  std::vector<Term> terms;
  if (!rp) {
    for (int i = 0; i <= k; ++i) terms.push_back({R(B0 + i), qs[i]});
    terms.insert(terms.begin(), Term{num(1.0), x});
    lin_v(x, terms);
  } else if (method == STORM_HIP_FGMRES) {
    terms.push_back({num(1.0), x});
    for (int i = 0; i <= k; ++i) terms.push_back({R(B0 + i), zs[i]});
    lin_v(x, terms);
  } else {  // q0 = sum beta_i q_i; z0 = P q0; x += z0          :242-247
    for (int i = 0; i <= k; ++i) terms.push_back({R(B0 + i), qs[i]});
    lin_v(qs[0], terms);
    pre(zs[0], qs[0]);
    axpy(x, num(1.0), zs[0]);
  }
}
void K::gmres_init() { gmres_start(true); }  // :51-91
void K::gmres_iterate(int64_t it) {  // Solver.hpp:236-248 around SolverGmres.hpp:119-192
  const bool P = has_pre();
  const int m = inner, k = (int)(it % m);
  const bool flexible = method == STORM_HIP_FGMRES;
  const bool lp = P && !flexible && side == STORM_HIP_LEFT, rp = P && (flexible || side == STORM_HIP_RIGHT);
  if (k == 0) gmres_start(false);
  V qn = qs[k + 1];
  if (lp) apply(zs[0], qs[k]), pre(qn, zs[0]);
  else if (rp) pre(zs[flexible ? k : 0], qs[k]), apply(qn, zs[flexible ? k : 0]);
  else apply(qn, qs[k]);
  flush();
  bool normalised = false;
  if (ok()) {
    std::vector<const double *> qd(m + 1);
    for (int i = 0; i <= m; ++i) qd[i] = qs[i]->d;
    const int st = gmres_orthogonalize(c, n, d_st, dp, qn->d, qd.data(), k, m, S + H0, S + R_T0, S + r_a0,
                                       gram_schmidt, &normalised);
    if (st != STORM_HIP_OK) fail(st);
  }
  sc(SC_SQRT, r_hn, R_T0);
  if (!normalised) divide(qn, r_hn);
  prog.aux[0] = H0, prog.aux[1] = B0, prog.aux[2] = CS0, prog.aux[3] = SN0, prog.aux[4] = m;
  sc(SC_GIVENS, R_ERR, k, r_hn);
  sc(SC_ADVANCE, 0, R_ERR);
  if (k == m - 1) {
    flush();
    gmres_update_x(k);
  }
}
// InnerOuterIterativeSolver::finalize, Solver.hpp:250-257 (none of the plain solvers has a finalize).
void K::gmres_finalize(int64_t iterations, bool forced) {
  // The in-loop update of the last iteration was skipped by the `done` predicate (or, when stepping, must not be
  // repeated: it already ran if that iteration closed a restart cycle).  With no iterate() at all the reference
  // divides by H(0,0) = 0 here; not reproduced.
  if (iterations <= 0) return;
  const int k = (int)((iterations - 1) % inner);
  if (!forced && k == inner - 1) return;
  const int *saved = dp;
  dp = nullptr;
  gmres_update_x(k);
  flush();
  dp = saved;
}

// ---- JFNK: SolverNewton.hpp:106-161 ------------------------------------------------------------------------------------
void K::jfnk_setup() {  // :108-111 (s lives in the inner engine: the work vector of its operator)
  t = vec(), r = vec(), v = vec();  // v: w = A(x)
  r_a0 = alloc(1);                  // mu
}
void K::jfnk_init() {  // :106-122: w = A(x); r = b - w (pre_op is taken and never read, :107-109)
  apply(v, x);
  lin(r, {{num(1.0), b}, {num(-1.0), v}});
  norm_to_err_and(SC_BEGIN, r);
}
void K::jfnk_iterate(int64_t) {  // :124-161
  dot(R_T0, x, x);  // mu = sqrt(eps) sqrt(1 + |x|), :128-130, into a register: the inner operator reads it there
  sc(SC_SQRT, R_T1, R_T0);
  sc(SC_ADD, R_T1, R_ONE, R_T1);
  sc(SC_SQRT, R_T1, R_T1);
  sc(SC_MUL, r_a0, imm(std::sqrt(2.220446049250313e-16)), R_T1);
  copy(t, r);  // the warm start, :131
  flush();
  if (ok()) {
    const int st = jfnk_inner_solve(this);  // J(x) t = r, :133-155 (the step's only host involvement: its polling)
    if (st != STORM_HIP_OK) fail(st);
  }
  axpy(x, num(1.0), t);  // :156
  apply(v, x);           // :157
  lin(r, {{num(1.0), b}, {num(-1.0), v}});
  norm_to_err_and(SC_ADVANCE, r);
}

// ---- the table: a row per method constant of storm_hip.h -----------------------------------------------------------------
namespace {
struct Method {
  void (K::*setup)();
  void (K::*init)();
  void (K::*iterate)(int64_t);
  void (K::*finalize)(int64_t, bool);  // nullable
};
const Method kTfqmr{&K::tfqmr_setup, &K::tfqmr_init, &K::tfqmr_iterate, nullptr};
const Method kGmres{&K::gmres_setup, &K::gmres_init, &K::gmres_iterate, &K::gmres_finalize};
const Method kMethods[STORM_HIP_JFNK + 1] = {
    /* STORM_HIP_CG */ {&K::cg_setup, &K::cg_init, &K::cg_iterate, nullptr},
    /* STORM_HIP_BICGSTAB */ {&K::bicgstab_setup, &K::bicgstab_init, &K::bicgstab_iterate, nullptr},
    /* STORM_HIP_GMRES, _FGMRES */ kGmres, kGmres,
    /* STORM_HIP_CGS */ {&K::cgs_setup, &K::cgs_init, &K::cgs_iterate, nullptr},
    /* STORM_HIP_TFQMR, _TFQMR1 */ kTfqmr, kTfqmr,
    /* STORM_HIP_BICGSTAB_L */ {&K::bicgstab_l_setup, &K::bicgstab_l_init, &K::bicgstab_l_iterate, nullptr},
    /* STORM_HIP_IDRS */ {&K::idrs_setup, &K::idrs_init, &K::idrs_iterate, nullptr},
    /* STORM_HIP_RICHARDSON */ {&K::richardson_setup, &K::richardson_init, &K::richardson_iterate, nullptr},
    /* STORM_HIP_JFNK */ {&K::jfnk_setup, &K::jfnk_init, &K::jfnk_iterate, nullptr}};
static_assert(STORM_HIP_CG == 0 && STORM_HIP_BICGSTAB == 1 && STORM_HIP_GMRES == 2 && STORM_HIP_FGMRES == 3 && STORM_HIP_CGS == 4 &&
                  STORM_HIP_TFQMR == 5 && STORM_HIP_TFQMR1 == 6 && STORM_HIP_BICGSTAB_L == 7 && STORM_HIP_IDRS == 8 &&
                  STORM_HIP_RICHARDSON == 9 && STORM_HIP_JFNK == 10, "kMethods is indexed by the method constant");
}  // namespace

void K::setup() {  // (method: one of the constants, storm_hip_krylov_create saw to it)
  S_top = R_USER;
  (this->*kMethods[method].setup)();
  if (op.is(Operator::FD)) r_fd = alloc(4);
}
void K::init() {
  (this->*kMethods[method].init)();
  flush();
}
void K::iterate(int64_t it) {
  cur_it = it;
  (this->*kMethods[method].iterate)(it);
  flush();
}
void K::finalize(int64_t iterations, bool forced) {
  if (kMethods[method].finalize != nullptr) (this->*kMethods[method].finalize)(iterations, forced);
}
