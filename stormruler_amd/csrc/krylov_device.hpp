// The device side of the general Krylov engine: the scalar machine's interpreter and every kernel of the engine.
// Included by krylov_engine.hip ALONE: the library is built without relocatable device code, so a kernel template
// instantiated in two units would be two kernels.  What the host fills in (SProg, RedOut, LinArgs) is in krylov_engine.hpp.
#pragma once
#include <type_traits>

#include "krylov_engine.hpp"
#include "ipc_device.hpp"
#include "ticket_device.hpp"

namespace storm {
namespace kry {

__device__ inline void exec_prog(const SProg &p, double *S, SolverState *st) {
  for (int i = 0; i < p.n; ++i) {
    const SOp o = p.ops[i];
#define RD(r) ((r) >= kImm0 ? p.imm[(r) - kImm0] : S[(r)])
    switch (o.op) {
      case SC_MOV: S[o.d] = RD(o.a); break;
      case SC_ADD: S[o.d] = RD(o.a) + RD(o.b); break;
      case SC_SUB: S[o.d] = RD(o.a) - RD(o.b); break;
      case SC_MUL: S[o.d] = RD(o.a) * RD(o.b); break;
      case SC_SDIV: S[o.d] = safe_divide(RD(o.a), RD(o.b)); break;
      case SC_DIV: S[o.d] = RD(o.a) / RD(o.b); break;
      case SC_NEG: S[o.d] = -RD(o.a); break;
      case SC_SQRT: S[o.d] = sqrt(RD(o.a)); break;
      case SC_FMADD: S[o.d] = S[o.d] + RD(o.a) * RD(o.b); break;
      case SC_FMSUB: S[o.d] = S[o.d] - RD(o.a) * RD(o.b); break;
      case SC_LT: S[o.d] = RD(o.a) < RD(o.b) ? 1.0 : 0.0; break;
      case SC_CMOV:
        if (RD(o.b) != 0.0) S[o.d] = RD(o.a);
        break;
      case SC_SYMORTHO: {
        const double a = RD(o.a), b = RD(o.b), rr = hypot(a, b);
        S[o.d] = rr > 0.0 ? a / rr : 1.0;
        S[o.d + 1] = rr > 0.0 ? b / rr : 0.0;
        S[o.d + 2] = rr;
      } break;
      case SC_BEGIN: begin(st, RD(o.a)); break;
      case SC_ADVANCE: advance(st, RD(o.a)); break;
      case SC_GIVENS: {  // SolverGmres.hpp:176-191
        double *H = S + p.aux[0], *beta = S + p.aux[1], *cs = S + p.aux[2], *sn = S + p.aux[3];
        const int m = p.aux[4], k = o.a;
#define H_(i, j) H[(i) * m + (j)]
        H_(k + 1, k) = S[o.b];
        for (int q = 0; q < k; ++q) {
          const double chi = cs[q] * H_(q, k) + sn[q] * H_(q + 1, k);
          H_(q + 1, k) = -sn[q] * H_(q, k) + cs[q] * H_(q + 1, k);
          H_(q, k) = chi;
        }
        const double a = H_(k, k), b = H_(k + 1, k), rr = hypot(a, b);
        const double c1 = rr > 0.0 ? a / rr : 1.0, s1 = rr > 0.0 ? b / rr : 0.0;
        cs[k] = c1, sn[k] = s1;
        H_(k, k) = c1 * H_(k, k) + s1 * H_(k + 1, k);
        H_(k + 1, k) = 0.0;
        beta[k + 1] = -s1 * beta[k];
        beta[k] *= c1;
        S[o.d] = fabs(beta[k + 1]);
      } break;
      case SC_BACKSOLVE: {  // SolverGmres.hpp:207-212
        double *H = S + p.aux[0], *beta = S + p.aux[1];
        const int m = p.aux[4], k = o.a;
        for (int q = k; q >= 0; --q) {
          for (int j = q + 1; j <= k; ++j) beta[q] -= H_(q, j) * beta[j];
          beta[q] /= H_(q, q);
        }
#undef H_
      } break;
      default: break;
    }
#undef RD
  }
}

// The epilogue of reduce_finish_kernel (solver_device.hpp) for the engine: the scalar program behind the sums.
struct ProgEpi {
  SProg prog;
  double *S;
  SolverState *st;
  __device__ void operator()() const {
    if (prog.n > 0) {
      __threadfence();
      exec_prog(prog, S, st);
    }
  }
};

// A scalar program alone; with nscatter > 0 first S[out.idx[j]] = S[scr + j] (results of an all-reduce).
__global__ void sprog_kernel(double *S, SolverState *st, SProg prog, int nscatter, RedOut out, int scr,
                             const int *done) {
  if (done && *done) return;
  for (int j = 0; j < nscatter; ++j) S[out.idx[j]] = S[scr + j];
  exec_prog(prog, S, st);
}

// o + c * v with ONE rounding per component, spelled out: the same statement must give the same bits whichever
// kernel evaluates it (alone, paired with its successor, with a reduction folded in).
__device__ __forceinline__ double2v fma2(double c, double2v v, double2v o) {
  double2v r;
  r.x = __builtin_fma(c, v.x, o.x), r.y = __builtin_fma(c, v.y, o.y);
  return r;
}
// The `nt` argument of the streaming kernels carries two flags: bit 0 = non-temporal accesses, bit 1 = deal the
// blocks out from the far end of the rows (the engine's sweep-direction scheme; a block keeps its rows and slots).
__device__ __forceinline__ unsigned sweep_block(int flags) { return (flags & 2) ? gridDim.x - 1 - blockIdx.x : blockIdx.x; }

// ---- reductions in ONE launch -----------------------------------------------------------------------------------
// A reduction is "partials kernel, then a one-block final pass that also runs the scalar program": two launches, and
// on the reference's own mesh sizes an iteration is nothing but launches (~4 us each, dependent).  Here the partials
// kernel finishes the job itself (ticket_device.hpp: two levels of tickets, partials published by awaited atomic
// exchange, fixed folding order): the block that draws the last ticket holds the sums, writes the registers and
// runs the scalar program.  The engine holds the partials kernel back until the program behind it is complete.
struct FinalPass {
  int *tickets;   // ticket_device.hpp counters (self re-arming)
  double *part2;  // [k][groups] group sums
  int k;
  RedOut out;
  double *S;
  SolverState *st;
  SProg prog;
};

// `mine[j]`: this block's partial of sum j (the same value in every thread).
template <int KMAX>
__device__ __forceinline__ void publish_and_finish(double *partials, const double (&mine)[KMAX], const FinalPass &f,
                                                   unsigned slot) {
  if (threadIdx.x >= kWave) return;
  double total[KMAX];
  const TicketArgs t{f.tickets, partials, f.part2};
  if (ticket_reduce_wave0<KMAX>(t, mine, f.k, slot, gridDim.x, total) && threadIdx.x == 0) {
#pragma unroll
    for (int j = 0; j < KMAX; ++j)
      if (j < f.k) f.S[f.out.idx[j]] = total[j];
    if (f.prog.n > 0) exec_prog(f.prog, f.S, f.st);
  }
}

template <int KB>
__global__ __launch_bounds__(kBlock) void dots_prog_kernel(int64_t n, const double *__restrict__ a, DotPtrs bs,
                                                           double *partials, const int *done, int nt, FinalPass f) {
  if (done && *done) return;
  __shared__ double lds4[4];
  double acc[KB];
#pragma unroll
  for (int j = 0; j < KB; ++j) acc[j] = 0.0;
  multi_dot_accumulate<KB>(n, a, bs, nt, acc);
  double mine[KB];
#pragma unroll
  for (int j = 0; j < KB; ++j) mine[j] = block_sum256(acc[j], lds4);
  publish_and_finish<KB>(partials, mine, f, sweep_block(nt));
}

// ---- vector statements ------------------------------------------------------------------------------------
__device__ __forceinline__ double ld_coef(const Scal &s) { return s.p ? (*s.p) * s.sign : s.v; }


// 16-byte accesses per stream and thread in flight: 4 for up to three streams, fewer beyond (measured,
// tools/cg_kernels_bench.hip: a 5-stream kernel runs 5 % faster with 1 than with 4, and collapses with 8).
__host__ __device__ constexpr int lin_unroll(int nt) { return nt <= 2 ? 4 : (nt == 3 ? 2 : 1); }

// y = c0 v0 + c1 v1 + ... (left to right), or NESTED (NT = 3):  y = v0 + c1 * (v1 + c2 * v2).
// Operands may alias y (every element is read before it is written by the same lane).
// `gate` (nullable): the statement was issued BEFORE the convergence rule of iteration gate_val - 1 but runs behind
// it (the engine held it back): it must execute iff that rule was evaluated at all -- the iteration counter has reached
// gate_val -- even when the rule then declared the solve done (the x update of the converging iteration).
template <int NT, bool NESTED>
__global__ __launch_bounds__(kBlock) void lin_kernel(int64_t n, LinArgs a, const int *done, int nt,
                                                     const long long *gate, long long gate_val) {
  if (gate ? (*gate < gate_val) : (done && *done)) return;
  if (a.cond && *a.cond == 0.0) return;
  const unsigned bx = sweep_block(nt);
  nt &= 1;
  double c[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) c[t] = ld_coef(a.c[t]);
  const int64_t n2 = n >> 1;
  double2v *y2 = reinterpret_cast<double2v *>(a.y);
  constexpr int U = lin_unroll(NT);
  nt_dispatch(nt, [&](auto nt) {
  for (int64_t base = (int64_t)bx * (kBlock * U) + threadIdx.x; base < n2;
       base += (int64_t)gridDim.x * (kBlock * U)) {
    double2v v[U][NT];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = base + u * kBlock;
      if (i < n2) {
#pragma unroll
        for (int t = 0; t < NT; ++t) v[u][t] = ldv(reinterpret_cast<const double2v *>(a.v[t]) + i, nt);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = base + u * kBlock;
      if (i < n2) {
        double2v o;
        if constexpr (NESTED) {
          o = v[u][0] + c[1] * (v[u][1] + c[2] * v[u][NT - 1]);
        } else {
          o = c[0] * v[u][0];
#pragma unroll
          for (int t = 1; t < NT; ++t) o = fma2(c[t], v[u][t], o);
        }
        stv(y2 + i, o, nt);
      }
    }
  }
  });
  if ((n & 1) && bx == 0 && threadIdx.x == 0) {
    const int64_t i = n - 1;
    double o;
    if constexpr (NESTED) {
      o = a.v[0][i] + c[1] * (a.v[1][i] + c[2] * a.v[NT - 1][i]);
    } else {
      o = c[0] * a.v[0][i];
      for (int t = 1; t < NT; ++t) o = __builtin_fma(c[t], a.v[t][i], o);
    }
    a.y[i] = o;
  }
}


// TWO consecutive vector statements in one pass, executed per element in program order (both are elementwise, so
// that is exactly their sequential meaning): y1 = sum c1_t v1_t;  y2 = sum c2_t v2_t, where an operand of the second
// that IS y1 takes the new value.  Every operand is loaded before anything is stored, so the second statement may
// overwrite an operand of the first ("x += alpha p;  p = r + beta p" -- p is read once: 40 instead of 48 bytes per
// row, one launch instead of two).
template <int NT1, int NT2>
__global__ __launch_bounds__(kBlock) void lin2_kernel(int64_t n, LinArgs a1, LinArgs a2, const int *done, int nt,
                                                      const long long *gate, long long gate_val) {
  bool run2 = !(done && *done);
  bool run1 = gate ? (*gate >= gate_val) : run2;  // (see lin_kernel; run2 implies run1)
  if (a1.cond && *a1.cond == 0.0) run1 = false;   // a conditional statement (TFQMR1's `if (omega < tau) x = d`)
  if (a2.cond && *a2.cond == 0.0) run2 = false;
  if (!run1 && !run2) return;
  const unsigned bx = sweep_block(nt);
  nt &= 1;
  double c1[NT1], c2[NT2];
  bool from1[NT2];
#pragma unroll
  for (int t = 0; t < NT1; ++t) c1[t] = ld_coef(a1.c[t]);
#pragma unroll
  for (int t = 0; t < NT2; ++t) c2[t] = ld_coef(a2.c[t]), from1[t] = run1 && a2.v[t] == a1.y;
  const int64_t n2 = n >> 1;
  double2v *y1 = reinterpret_cast<double2v *>(a1.y), *y2 = reinterpret_cast<double2v *>(a2.y);
  nt_dispatch(nt, [&](auto nt) {
  for (int64_t i = (int64_t)bx * kBlock + threadIdx.x; i < n2; i += (int64_t)gridDim.x * kBlock) {
    double2v v1[NT1], v2[NT2];
#pragma unroll
    for (int t = 0; t < NT1; ++t) v1[t] = ldv(reinterpret_cast<const double2v *>(a1.v[t]) + i, nt);
#pragma unroll
    for (int t = 0; t < NT2; ++t) v2[t] = ldv(reinterpret_cast<const double2v *>(a2.v[t]) + i, nt);
    double2v o1 = c1[0] * v1[0];
#pragma unroll
    for (int t = 1; t < NT1; ++t) o1 = fma2(c1[t], v1[t], o1);
    double2v o2 = c2[0] * (from1[0] ? o1 : v2[0]);
#pragma unroll
    for (int t = 1; t < NT2; ++t) o2 = fma2(c2[t], from1[t] ? o1 : v2[t], o2);
    if (run1) stv(y1 + i, o1, nt);
    if (run2) stv(y2 + i, o2, nt);
  }
  });
  if ((n & 1) && bx == 0 && threadIdx.x == 0) {
    const int64_t i = n - 1;
    double w1[NT1], w2[NT2];
    for (int t = 0; t < NT1; ++t) w1[t] = a1.v[t][i];
    for (int t = 0; t < NT2; ++t) w2[t] = a2.v[t][i];
    double o1 = c1[0] * w1[0];
    for (int t = 1; t < NT1; ++t) o1 = __builtin_fma(c1[t], w1[t], o1);
    double o2 = c2[0] * (from1[0] ? o1 : w2[0]);
    for (int t = 1; t < NT2; ++t) o2 = __builtin_fma(c2[t], from1[t] ? o1 : w2[t], o2);
    if (run1) a1.y[i] = o1;
    if (run2) a2.y[i] = o2;
  }
}

// The same statement with reductions of its RESULT folded in: per-block partials of <y, y> (dot_yy) and / or
// <y, w> into partials[j * gridDim.x + block] -- "r -= alpha z; gamma = <r, r>" is one pass over r, not two.
// HASW: a second operand w is streamed for <y, w> (it counts as a stream when the accesses in flight are chosen: "r -= alpha z;
// <r, r>" is a three-stream kernel like cg_r and runs with four, 79 -> 6x us at 256^3).
template <int NT, bool HASW>
__device__ __forceinline__ void lin_dot_body(int64_t n, const LinArgs &a, const double *w, int nt, double &acc_yy,
                                             double &acc_yw) {
  const unsigned bx = sweep_block(nt);
  nt &= 1;
  double c[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) c[t] = ld_coef(a.c[t]);
  const int64_t n2 = n >> 1;
  double2v *y2 = reinterpret_cast<double2v *>(a.y);
  const double2v *w2 = reinterpret_cast<const double2v *>(w);
  constexpr int U = lin_unroll(NT + (HASW ? 1 : 0));
  nt_dispatch(nt, [&](auto nt) {
  for (int64_t base = (int64_t)bx * (kBlock * U) + threadIdx.x; base < n2;
       base += (int64_t)gridDim.x * (kBlock * U)) {
    double2v v[U][NT], vw[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = base + u * kBlock;
      if (i < n2) {
#pragma unroll
        for (int t = 0; t < NT; ++t) v[u][t] = ldv(reinterpret_cast<const double2v *>(a.v[t]) + i, nt);
        if (w) vw[u] = ldv(w2 + i, nt);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = base + u * kBlock;
      if (i < n2) {
        double2v o = c[0] * v[u][0];
#pragma unroll
        for (int t = 1; t < NT; ++t) o = fma2(c[t], v[u][t], o);
        stv(y2 + i, o, nt);
        acc_yy += o.x * o.x;
        acc_yy += o.y * o.y;
        if (w) acc_yw += o.x * vw[u].x, acc_yw += o.y * vw[u].y;
      }
    }
  }
  });
  if ((n & 1) && bx == 0 && threadIdx.x == 0) {
    const int64_t i = n - 1;
    double o = c[0] * a.v[0][i];
    for (int t = 1; t < NT; ++t) o = __builtin_fma(c[t], a.v[t][i], o);
    a.y[i] = o;
    acc_yy += o * o;
    if (w) acc_yw += o * w[i];
  }
}

template <int NT, bool HASW>
__global__ __launch_bounds__(kBlock) void lin_dot_kernel(int64_t n, LinArgs a, const double *w, int dot_yy,
                                                         double *__restrict__ partials, const int *done, int nt) {
  if (done && *done) return;
  __shared__ double lds4[4];
  double acc_yy = 0.0, acc_yw = 0.0;
  lin_dot_body<NT, HASW>(n, a, w, nt, acc_yy, acc_yw);
  int j = 0;
  if (dot_yy) {
    const double sum = block_sum256(acc_yy, lds4);
    if (threadIdx.x == 0) partials[(int64_t)j * gridDim.x + sweep_block(nt)] = sum;
    ++j;
  }
  if (w) {
    const double sum = block_sum256(acc_yw, lds4);
    if (threadIdx.x == 0) partials[(int64_t)j * gridDim.x + sweep_block(nt)] = sum;
  }
}

// ... and with the final pass in the last block (see publish_and_finish).
template <int NT, bool HASW>
__global__ __launch_bounds__(kBlock) void lin_dot_prog_kernel(int64_t n, LinArgs a, const double *w, int dot_yy,
                                                              double *partials, const int *done, int nt, FinalPass f) {
  if (done && *done) return;
  __shared__ double lds4[4];
  double acc_yy = 0.0, acc_yw = 0.0;
  lin_dot_body<NT, HASW>(n, a, w, nt, acc_yy, acc_yw);
  double mine[2] = {0.0, 0.0};
  int j = 0;
  if (dot_yy) mine[j++] = block_sum256(acc_yy, lds4);
  if (w) mine[j] = block_sum256(acc_yw, lds4);
  publish_and_finish<2>(partials, mine, f, sweep_block(nt));
}

// A diagonal preconditioner and the reductions behind it in one pass: z = d .* r, <r, z>, <r, r> (preconditioned CG,
// SolverCg.hpp:100-115).  Rows per block and order of a thread's terms are those of multi_dot_accumulate<2>
// (blas1_device.hpp), so the sums carry the bits of the separate vmul + multi-dot.
__global__ __launch_bounds__(kBlock) void vmul_dots_prog_kernel(int64_t n, double *__restrict__ z,
                                                                const double *__restrict__ d,
                                                                const double *__restrict__ r, double *partials,
                                                                const int *done, int nt, FinalPass f) {
  if (done && *done) return;
  __shared__ double lds4[4];
  const unsigned bx = sweep_block(nt);
  const int64_t n2 = n >> 1;
  double2v *z2 = reinterpret_cast<double2v *>(z);
  const double2v *d2 = reinterpret_cast<const double2v *>(d), *r2 = reinterpret_cast<const double2v *>(r);
  double acc_rz = 0.0, acc_rr = 0.0;
  nt_dispatch(nt, [&](auto nt) {
  for (int64_t base = (int64_t)bx * (kBlock * kUnroll) + threadIdx.x; base < n2; base += (int64_t)gridDim.x * (kBlock * kUnroll)) {
    double2v vd[kUnroll], vr[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int64_t i = base + u * kBlock;
      if (i < n2) vd[u] = ldv(d2 + i, nt), vr[u] = ldv(r2 + i, nt);
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int64_t i = base + u * kBlock;
      if (i < n2) {
        const double2v vz = vd[u] * vr[u];
        stv(z2 + i, vz, nt);
        acc_rz += vr[u].x * vz.x;
        acc_rz += vr[u].y * vz.y;
        acc_rr += vr[u].x * vr[u].x;
        acc_rr += vr[u].y * vr[u].y;
      }
    }
  }
  });
  if ((n & 1) && bx == 0 && threadIdx.x == 0) {
    const double vz = d[n - 1] * r[n - 1];
    z[n - 1] = vz;
    acc_rz += r[n - 1] * vz;
    acc_rr += r[n - 1] * r[n - 1];
  }
  const double mine[2] = {block_sum256(acc_rz, lds4), block_sum256(acc_rr, lds4)};
  publish_and_finish<2>(partials, mine, f, bx);
}

// A held-back vector statement, the statement that follows it, and the reductions of THAT statement's result, in
// one pass (lin2_kernel + lin_dot_prog_kernel): BiCGStab's "x += alpha p + omega s;  r = s - omega t;  |r|^2, <rt, r>"
// reads x, p, r, t, rt and writes x, r once -- the hand-fused loop's second half-step.
template <int NT1, int NT2, bool HASW>
__global__ __launch_bounds__(kBlock) void lin2_dot_prog_kernel(int64_t n, LinArgs a1, LinArgs a2, const double *w,
                                                               int dot_yy, double *partials, const int *done, int nt,
                                                               FinalPass f) {
  if (done && *done) return;
  __shared__ double lds4[4];
  const unsigned bx = sweep_block(nt);
  double c1[NT1], c2[NT2];
  bool from1[NT2];
#pragma unroll
  for (int t = 0; t < NT1; ++t) c1[t] = ld_coef(a1.c[t]);
#pragma unroll
  for (int t = 0; t < NT2; ++t) c2[t] = ld_coef(a2.c[t]), from1[t] = a2.v[t] == a1.y;
  const bool w_from1 = w == a1.y;
  const int64_t n2 = n >> 1;
  double2v *y1 = reinterpret_cast<double2v *>(a1.y), *y2 = reinterpret_cast<double2v *>(a2.y);
  const double2v *w2 = reinterpret_cast<const double2v *>(w);
  double acc_yy = 0.0, acc_yw = 0.0;
  // (the rows of a block and the order of a thread's terms are those of lin_dot_body for the second statement: the
  //  partial sums -- and the reduction's bits -- do not depend on whether a held-back statement rode along)
  constexpr int U = lin_unroll(NT2 + (HASW ? 1 : 0));
  nt_dispatch(nt, [&](auto nt) {
  for (int64_t base = (int64_t)bx * (kBlock * U) + threadIdx.x; base < n2; base += (int64_t)gridDim.x * (kBlock * U)) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = base + u * kBlock;
      if (i < n2) {
        double2v v1[NT1], v2[NT2], vw = {0.0, 0.0};
#pragma unroll
        for (int t = 0; t < NT1; ++t) v1[t] = ldv(reinterpret_cast<const double2v *>(a1.v[t]) + i, nt);
#pragma unroll
        for (int t = 0; t < NT2; ++t) v2[t] = ldv(reinterpret_cast<const double2v *>(a2.v[t]) + i, nt);
        if (w) vw = ldv(w2 + i, nt);
        double2v o1 = c1[0] * v1[0];
#pragma unroll
        for (int t = 1; t < NT1; ++t) o1 = fma2(c1[t], v1[t], o1);
        double2v o2 = c2[0] * (from1[0] ? o1 : v2[0]);
#pragma unroll
        for (int t = 1; t < NT2; ++t) o2 = fma2(c2[t], from1[t] ? o1 : v2[t], o2);
        stv(y1 + i, o1, nt);
        stv(y2 + i, o2, nt);
        if (w_from1) vw = o1;
        acc_yy += o2.x * o2.x;
        acc_yy += o2.y * o2.y;
        if (w) acc_yw += o2.x * vw.x, acc_yw += o2.y * vw.y;
      }
    }
  }
  });
  if ((n & 1) && bx == 0 && threadIdx.x == 0) {
    const int64_t i = n - 1;
    double w1[NT1], w2v[NT2];
    for (int t = 0; t < NT1; ++t) w1[t] = a1.v[t][i];
    for (int t = 0; t < NT2; ++t) w2v[t] = a2.v[t][i];
    const double wl = w ? w[i] : 0.0;
    double o1 = c1[0] * w1[0];
    for (int t = 1; t < NT1; ++t) o1 = __builtin_fma(c1[t], w1[t], o1);
    double o2 = c2[0] * (from1[0] ? o1 : w2v[0]);
    for (int t = 1; t < NT2; ++t) o2 = __builtin_fma(c2[t], from1[t] ? o1 : w2v[t], o2);
    a1.y[i] = o1;
    a2.y[i] = o2;
    acc_yy += o2 * o2;
    if (w) acc_yw += o2 * (w_from1 ? o1 : wl);
  }
  double mine[2] = {0.0, 0.0};
  int j = 0;
  if (dot_yy) mine[j++] = block_sum256(acc_yy, lds4);
  if (w) mine[j] = block_sum256(acc_yw, lds4);
  publish_and_finish<2>(partials, mine, f, bx);
}

// ---- the finite-difference Jacobian: J(y) = (A(x + delta y) - A(x)) / delta, SolverNewton.hpp:143-156 ---------------
// Two vector statements around the callback, with the REFERENCE's roundings (two per element each), which none of
// lin_kernel's forms gives: it would contract x + delta y into one fma, and its NESTED form has no c (v1 - v2) without a
// leading operand.  delta and delta_inverse are registers: the scalar program behind <y, y> leaves them there.
//
// s = fl(x + fl(delta y)): the axpbz form fma(1, x, fl(b z)) of the header's table.  The product is a statement of its
// own, so -ffp-contract=on (contraction within ONE expression) cannot fuse it into the sum.  lin_kernel's streaming shape:
// one trip per thread, kUnroll independent 16-byte accesses per stream in flight; NT: non-temporal accesses.
template <bool NT>
__global__ __launch_bounds__(kBlock) void fd_shift_kernel(int64_t n, double *s, const double *x, const double *y,
                                                          const double *delta_reg, const int *done, int flags) {
  if (done && *done) return;
  const unsigned bx = sweep_block(flags);
  const double delta = *delta_reg;
  const std::integral_constant<bool, NT> nt{};
  const int64_t n2 = n >> 1;
  double2v *s2 = reinterpret_cast<double2v *>(s);
  const double2v *x2 = reinterpret_cast<const double2v *>(x), *y2 = reinterpret_cast<const double2v *>(y);
  for (int64_t base = (int64_t)bx * (kBlock * kUnroll) + threadIdx.x; base < n2;
       base += (int64_t)gridDim.x * (kBlock * kUnroll)) {
    double2v vx[kUnroll], vy[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int64_t i = base + u * kBlock;
      if (i < n2) vx[u] = ldv(x2 + i, nt), vy[u] = ldv(y2 + i, nt);
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int64_t i = base + u * kBlock;
      if (i < n2) {
        const double2v prod = delta * vy[u];  // (rounded here ...)
        const double2v sum = vx[u] + prod;    // (... and here)
        stv(s2 + i, sum, nt);
      }
    }
  }
  if ((n & 1) && bx == 0 && threadIdx.x == 0) {
    const double prod = delta * y[n - 1];
    const double sum = x[n - 1] + prod;
    s[n - 1] = sum;
  }
}

// z = fl(delta_inverse * fl(z - w)) in place, and per-thread terms of <z, z> / <z, u> of the new z: lin_dot_body's shape
// and unroll rule with w and u counted as streams.
template <bool HASW>
__device__ __forceinline__ void fd_diff_body(int64_t n, double *z, const double *w, const double *u, double dinv, int nt,
                                             double &acc_zz, double &acc_zu) {
  const unsigned bx = sweep_block(nt);
  nt &= 1;
  const int64_t n2 = n >> 1;
  double2v *z2 = reinterpret_cast<double2v *>(z);
  const double2v *w2 = reinterpret_cast<const double2v *>(w), *u2 = reinterpret_cast<const double2v *>(u);
  constexpr int U = lin_unroll(2 + (HASW ? 1 : 0));
  nt_dispatch(nt, [&](auto nt) {
  for (int64_t base = (int64_t)bx * (kBlock * U) + threadIdx.x; base < n2; base += (int64_t)gridDim.x * (kBlock * U)) {
    double2v vz[U], vw[U], vu[U];
#pragma unroll
    for (int q = 0; q < U; ++q) {
      const int64_t i = base + q * kBlock;
      if (i < n2) {
        vz[q] = ldv(z2 + i, nt), vw[q] = ldv(w2 + i, nt);
        if (HASW) vu[q] = ldv(u2 + i, nt);
      }
    }
#pragma unroll
    for (int q = 0; q < U; ++q) {
      const int64_t i = base + q * kBlock;
      if (i < n2) {
        const double2v diff = vz[q] - vw[q];
        const double2v o = dinv * diff;
        stv(z2 + i, o, nt);
        acc_zz += o.x * o.x;
        acc_zz += o.y * o.y;
        if (HASW) acc_zu += o.x * vu[q].x, acc_zu += o.y * vu[q].y;
      }
    }
  }
  });
  if ((n & 1) && bx == 0 && threadIdx.x == 0) {
    const int64_t i = n - 1;
    const double diff = z[i] - w[i];
    const double o = dinv * diff;
    z[i] = o;
    acc_zz += o * o;
    if (HASW) acc_zu += o * u[i];
  }
}

// The statement alone: what follows the product is no reduction of z (GMRES's Gram-Schmidt chain, a plain apply).
__global__ __launch_bounds__(kBlock) void fd_diff_kernel(int64_t n, double *z, const double *w, const double *dinv_reg,
                                                         const int *done, int nt) {
  if (done && *done) return;
  double acc_zz = 0.0, acc_zu = 0.0;
  fd_diff_body<false>(n, z, w, nullptr, *dinv_reg, nt, acc_zz, acc_zu);
}

// ... and with the reductions the solver takes of z next in the same pass, finished in the last block with the scalar
// program behind them (lin_dot_prog_kernel's dot_yy / w pair): BiCGStab's <rt, v> behind its first product, <t, s> and
// <t, t> behind its second (SolverBiCgStab.hpp:93-165).
template <bool HASW>
__global__ __launch_bounds__(kBlock) void fd_diff_dots_prog_kernel(int64_t n, double *z, const double *w, const double *u,
                                                                   const double *dinv_reg, int dot_zz, double *partials,
                                                                   const int *done, int nt, FinalPass f) {
  if (done && *done) return;
  __shared__ double lds4[4];
  double acc_zz = 0.0, acc_zu = 0.0;
  fd_diff_body<HASW>(n, z, w, u, *dinv_reg, nt, acc_zz, acc_zu);
  double mine[2] = {0.0, 0.0};
  int j = 0;
  if (dot_zz) mine[j++] = block_sum256(acc_zz, lds4);
  if (HASW) mine[j] = block_sum256(acc_zu, lds4);
  publish_and_finish<2>(partials, mine, f, sweep_block(nt));
}

}  // namespace kry
}  // namespace storm
