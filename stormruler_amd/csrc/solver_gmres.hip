// The fused GMRES(m) loop of a stencil operator (SolverGmres.hpp:51-249), its kernels, and the Gram-Schmidt ladder it
// shares with the general engine (krylov_methods.hip); see solver_fused.hip.
#include <algorithm>
#include "solver_fused.hpp"
#include "blas1_device.hpp"
#include "spmv_device.hpp"

namespace storm {

// One modified-Gram-Schmidt step fused with the next reduction (SolverGmres.hpp:157-161):
//   w -= h * qa;  partial <w, qb>   (qb == nullptr: partial <w, w>, the norm of :161)
// Same values as the reference's dot -> axpy -> dot chain, one pass over w instead of two.
// h comes either from memory (*h) or, on a single rank with few blocks, from the previous kernel's
// per-block partials: every block folds them itself in the same fixed order (so all blocks hold the
// same h) and block 0 stores it into the Hessenberg -- the separate final-reduction launch between two
// steps disappears, which is what a 128^3 problem (launch-bound MGS chain) is made of.
__global__ __launch_bounds__(kBlock) void mgs_step_kernel(int64_t n, const int *done, double *__restrict__ w,
                                                          const double *h, const double *__restrict__ in_partials,
                                                          int n_in, double *h_store,
                                                          const double *__restrict__ qa,
                                                          const double *qb, double *__restrict__ partials, int nt) {
  if (done && *done) return;
  __shared__ double lds4[4];
  double hv;
  if (in_partials) {
    hv = block_fold(in_partials, n_in, lds4);
    if (blockIdx.x == 0 && threadIdx.x == 0) *h_store = hv;
  } else {
    hv = *h;
  }
  double acc = 0.0;
  const int64_t n2 = n >> 1;
  double2v *w2 = reinterpret_cast<double2v *>(w);
  const double2v *a2 = reinterpret_cast<const double2v *>(qa), *b2 = reinterpret_cast<const double2v *>(qb);
  nt_dispatch(nt, [&](auto nt) {
  STORM_STREAM_FOR(base, n2) {
    double2v vw[kUnroll], va[kUnroll], vb[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int64_t i = base + u * kBlock;
      if (i < n2) {
        vw[u] = ldv(w2 + i, nt), va[u] = ldv(a2 + i, nt);
        if (qb) vb[u] = ldv(b2 + i, nt);
      }
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int64_t i = base + u * kBlock;
      if (i < n2) {
        vw[u] -= hv * va[u];
        stv(w2 + i, vw[u], nt);
        const double2v o = qb ? vb[u] : vw[u];
        acc += vw[u].x * o.x;
        acc += vw[u].y * o.y;
      }
    }
  }
  });
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    const double v = w[n - 1] - hv * qa[n - 1];
    w[n - 1] = v;
    acc += v * (qb ? qb[n - 1] : v);
  }
  const double s = block_sum256(acc, lds4);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// GMRES: Givens update of column k and the beta recurrence, SolverGmres.hpp:176-191.
// One wavefront copies column k and the rotations into LDS, lane 0 runs the reference's loop there (the arithmetic of
// gmres_givens_update, solver_device.hpp, in its order: the same bits) -- the k dependent steps cost an LDS access each
// instead of three trips to memory (9.7 -> ~3 us per inner iteration at k ~ 15).
__global__ __launch_bounds__(kWave) void gmres_givens_kernel(SolverState *st, GmresDev g, int k) {
  if (st->done) return;
  __shared__ double hcol[kMaxMulti + 2], cs_sh[kMaxMulti], sn_sh[kMaxMulti];
  const int lane = (int)threadIdx.x, m = g.m;
  for (int i = lane; i <= k; i += kWave) hcol[i] = g.H[(int64_t)i * m + k];
  for (int i = lane; i < k; i += kWave) cs_sh[i] = g.cs[i], sn_sh[i] = g.sn[i];
  __syncthreads();
  if (lane != 0) return;
  hcol[k + 1] = st->s[S_HN];
  for (int i = 0; i < k; ++i) {
    const double chi = cs_sh[i] * hcol[i] + sn_sh[i] * hcol[i + 1];
    hcol[i + 1] = -sn_sh[i] * hcol[i] + cs_sh[i] * hcol[i + 1];
    hcol[i] = chi;
  }
  const double ha = hcol[k], hb = hcol[k + 1];
  const double rr = hypot(ha, hb);
  double cs, sn;
  if (rr > 0.0) cs = ha / rr, sn = hb / rr;
  else cs = 1.0, sn = 0.0;
  g.cs[k] = cs, g.sn[k] = sn;
  hcol[k] = cs * ha + sn * hb;
  hcol[k + 1] = 0.0;
  for (int i = 0; i <= k + 1; ++i) g.H[(int64_t)i * m + k] = hcol[i];
  const double bk = g.beta[k];
  g.beta[k + 1] = -sn * bk;
  g.beta[k] = bk * cs;
  advance(st, fabs(-sn * bk));
}

// TWO modified-Gram-Schmidt steps per pass, the reductions finished in the kernel (ticket_device.hpp):
//   w -= ha qa;  w -= hb qb;                       (ha, hb from the Hessenberg; qa == nullptr: nothing to subtract,
//                                                   qb == nullptr: one vector)
//   then, of the updated w:  a = <w, qc>, b = <w, qd>, c = <qc, qd>   ->   *out_c = a,  *out_d = b - a c
//   (the reference's h = <w - a qc, qd>, by bilinearity -- see mgs_chain_kernel, mgs_chain.hip);
//   qd == nullptr: *out_c = <w, qc>;  qc == nullptr: *out_c = <w, w> (SolverGmres.hpp:161).
// 24 B/row/step and half a launch per step instead of 32 B/row/step and two launches (mgs_step_kernel + final pass).
__global__ __launch_bounds__(kBlock) void mgs_pair_kernel(int64_t n, const int *done, double *__restrict__ w,
                                                          const double *ha, const double *hb,
                                                          const double *__restrict__ qa, const double *__restrict__ qb,
                                                          const double *__restrict__ qc, const double *__restrict__ qd,
                                                          double *out_c, double *out_d, TicketArgs tickets, int nt) {
  if (done && *done) return;
  __shared__ double lds4[4];
  const double va = qa ? *ha : 0.0, vb = qb ? *hb : 0.0;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  const int64_t n2 = n >> 1;
  double2v *w2 = reinterpret_cast<double2v *>(w);
  const double2v *a2 = reinterpret_cast<const double2v *>(qa), *b2 = reinterpret_cast<const double2v *>(qb);
  const double2v *c2 = reinterpret_cast<const double2v *>(qc), *d2 = reinterpret_cast<const double2v *>(qd);
  nt_dispatch(nt, [&](auto nt) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n2; i += (int64_t)gridDim.x * kBlock) {
    double2v vw = ldv(w2 + i, nt), xa = {0.0, 0.0}, xb = {0.0, 0.0}, xc = {0.0, 0.0}, xd = {0.0, 0.0};
    if (qa) xa = ldv(a2 + i, nt);
    if (qb) xb = ldv(b2 + i, nt);
    if (qc) xc = ldv(c2 + i, nt);
    if (qd) xd = ldv(d2 + i, nt);
    if (qa) {
      vw -= va * xa;
      if (qb) vw -= vb * xb;
      stv(w2 + i, vw, nt);
    }
    if (qc) {
      s0 += vw.x * xc.x, s0 += vw.y * xc.y;
      if (qd) s1 += vw.x * xd.x, s1 += vw.y * xd.y, s2 += xc.x * xd.x, s2 += xc.y * xd.y;
    } else {
      s0 += vw.x * vw.x, s0 += vw.y * vw.y;
    }
  }
  });
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    const int64_t i = n - 1;
    double vw = w[i];
    if (qa) {
      vw -= va * qa[i];
      if (qb) vw -= vb * qb[i];
      w[i] = vw;
    }
    if (qc) {
      s0 += vw * qc[i];
      if (qd) s1 += vw * qd[i], s2 += qc[i] * qd[i];
    } else {
      s0 += vw * vw;
    }
  }
  const double mine[3] = {block_sum256(s0, lds4), block_sum256(s1, lds4), block_sum256(s2, lds4)};
  if (threadIdx.x >= kWave) return;
  double total[3];
  if (ticket_reduce_wave0<3>(tickets, mine, qd ? 3 : 1, blockIdx.x, gridDim.x, total) && threadIdx.x == 0) {
    *out_c = total[0];
    if (qd) *out_d = total[1] - total[0] * total[2];
  }
}

// T modified-Gram-Schmidt steps per pass (T = 3, 4): the pair kernel's scheme with more vectors per trip over w.
//   w -= h[0] qa[0]; ... ; w -= h[na-1] qa[na-1]       (the previous pass's coefficients, in the reference's order)
//   then, of the updated w:  c_j = <w, qc_j>,  g_ij = <qc_i, qc_j> (i < j < nc)
//   ->  out[j] = c_j - sum_{i<j} out[i] g_ij           (= <w - sum_{i<j} h_i qc_i, qc_j>, by bilinearity, j ascending)
//   nc == 0: out[0] = <w, w> (SolverGmres.hpp:161).
// 8 (2 + na + nc) B/row per pass: 20 B/row/step at T = 4 against the pair kernel's 24.  Shape: the streaming kernels'
// (stream_blocks(n) blocks, kUnroll trips per thread), one access per stream and trip in flight -- with up to ten streams
// that is as many as the pair kernel's five with two; the block's partials (up to T + T (T - 1) / 2) are folded once, after
// the last trip, through LDS with one barrier, and finished by tickets.
template <int T>
struct MgsMultiArgs {
  const double *h[T];   // coefficients of the vectors to subtract (device, finished by the previous pass)
  const double *qa[T];  // the vectors to subtract
  const double *qc[T];  // the vectors to project on next
  double *out[T];       // where their coefficients go (nc == 0: out[0] = the norm's square)
  int na, nc;
};
template <int T, int TRIPS>
__global__ __launch_bounds__(kBlock) void mgs_multi_kernel(int64_t n, const int *done, double *__restrict__ w, MgsMultiArgs<T> a,
                                                           TicketArgs tickets, int nt) {
  if (done && *done) return;
  constexpr int NG = T * (T - 1) / 2, NV = T + NG;
  __shared__ double lds[4][NV];
  double hv[T];
#pragma unroll
  for (int j = 0; j < T; ++j) hv[j] = j < a.na ? *a.h[j] : 0.0;
  double acc[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) acc[v] = 0.0;
  const int64_t n2 = n >> 1;
  double2v *w2 = reinterpret_cast<double2v *>(w);
  auto fold = [&](double wx, double wy, const double2v (&xc)[T]) {
    if (a.nc == 0) {
      acc[0] += wx * wx, acc[0] += wy * wy;
      return;
    }
    int g = T;
#pragma unroll
    for (int j = 0; j < T; ++j) {
      acc[j] += wx * xc[j].x, acc[j] += wy * xc[j].y;
#pragma unroll
      for (int i = 0; i < j; ++i, ++g) acc[g] += xc[i].x * xc[j].x, acc[g] += xc[i].y * xc[j].y;
    }
  };
  nt_dispatch(nt, [&](auto nt) {
  for (int64_t base = (int64_t)blockIdx.x * (kBlock * TRIPS) + threadIdx.x; base < n2;
       base += (int64_t)gridDim.x * (kBlock * TRIPS)) {
#pragma unroll
    for (int u = 0; u < TRIPS; ++u) {
      const int64_t i = base + u * kBlock;
      if (i >= n2) break;
      double2v vw = ldv(w2 + i, nt), xa[T], xc[T];
#pragma unroll
      for (int j = 0; j < T; ++j) {
        xa[j] = double2v{0.0, 0.0}, xc[j] = double2v{0.0, 0.0};
        if (j < a.na) xa[j] = ldv(reinterpret_cast<const double2v *>(a.qa[j]) + i, nt);
        if (j < a.nc) xc[j] = ldv(reinterpret_cast<const double2v *>(a.qc[j]) + i, nt);
      }
      if (a.na > 0) {
#pragma unroll
        for (int j = 0; j < T; ++j)
          if (j < a.na) vw -= hv[j] * xa[j];
        stv(w2 + i, vw, nt);
      }
      fold(vw.x, vw.y, xc);
    }
  }
  });
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    const int64_t i = n - 1;
    double vw = w[i];
    double2v xc[T];
#pragma unroll
    for (int j = 0; j < T; ++j) {
      if (j < a.na) vw -= hv[j] * a.qa[j][i];
      xc[j] = double2v{j < a.nc ? a.qc[j][i] : 0.0, 0.0};
    }
    if (a.na > 0) w[i] = vw;
    fold(vw, 0.0, xc);
  }
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const double s = wave_sum_to_lane63(acc[v]);  // (DPP: ten shuffle trees through the LDS crossbar cost ~1 us per wave)
    if (lane == kWave - 1) lds[wave][v] = s;
  }
  __syncthreads();
  if (threadIdx.x >= kWave) return;
  double mine[NV], total[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) mine[v] = (lds[0][v] + lds[1][v]) + (lds[2][v] + lds[3][v]);
  const int nv = a.nc == 0 ? 1 : NV;
  if (ticket_reduce_wave0<NV>(tickets, mine, nv, blockIdx.x, gridDim.x, total) && threadIdx.x == 0) {
    if (a.nc == 0) {
      *a.out[0] = total[0];
      return;
    }
    double hn[T];
    int g = T;
#pragma unroll
    for (int j = 0; j < T; ++j) {
      double v = total[j];
#pragma unroll
      for (int i = 0; i < j; ++i, ++g) v -= hn[i] * total[g];
      hn[j] = v;
      if (j < a.nc) *a.out[j] = v;
    }
  }
}

// Classical Gram-Schmidt x2: H(j0 : j0 + kk, k) = h_pass0 + h_pass1.
__global__ void gmres_cgs2_combine_kernel(const int *done, double *H, int m, int k, int j0, int kk,
                                          const double *scratch) {
  if (done && *done) return;
  for (int i = 0; i < kk; ++i) H[(j0 + i) * m + k] = scratch[i] + scratch[kMaxMulti + i];
}

// GMRES: back substitution, SolverGmres.hpp:207-212.  One wavefront copies the triangle and beta into LDS, lane 0 runs
// the reference's loops there (the same operations in the same order: one accumulator per row, j ascending) and the
// wavefront stores beta back: the ~k^2 / 2 dependent steps cost an LDS access each instead of two trips to memory
// (147 -> 2x us per restart of GMRES(50) at any size: 3 us of every inner iteration).
__global__ __launch_bounds__(kWave) void gmres_backsolve_kernel(SolverState *st, GmresDev g, int k, bool force) {
  if (!force && st->done) return;
  __shared__ double Hs[kMaxMulti * kMaxMulti], bs[kMaxMulti];
  const int m = g.m, n = k + 1, lane = threadIdx.x;
  // (every load of the lane issued before the first is stored: one after the other they cost a trip to memory each --
  //  fifteen of the kernel's 21 us at k = 29; the upper triangle is all the substitution reads)
  for (int r0 = 0; r0 < n; r0 += 8) {
    double hv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) hv[u] = (r0 + u < n && lane < n && lane >= r0 + u) ? g.H[(r0 + u) * m + lane] : 0.0;
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (r0 + u < n && lane < n) Hs[(r0 + u) * kMaxMulti + lane] = hv[u];
  }
  if (lane < n) bs[lane] = g.beta[lane];
  __syncthreads();
  if (lane == 0) {
    for (int i = k; i >= 0; --i) {
      double acc = bs[i];
      for (int j = i + 1; j <= k; ++j) acc -= Hs[i * kMaxMulti + j] * bs[j];
      bs[i] = acc / Hs[i * kMaxMulti + i];
    }
  }
  __syncthreads();
  if (lane < n) g.beta[lane] = bs[lane];
}

// Orthogonalise w = q_{k+1} against q_0 .. q_k (SolverGmres.hpp:157-161): H(0..k, k) and <w, w> (into *norm2_out;
// the caller takes the root and normalises).  H is the (m+1) x m row-major device Hessenberg.
//   gram_schmidt == 0: modified Gram-Schmidt with exactly the reference's values -- H(0,k) = <w,q_0>, then every
//     step applies  w -= H(i,k) q_i  and already accumulates the next reduction (<w,q_{i+1}>, or <w,w>);
//   gram_schmidt == 1: classical Gram-Schmidt applied twice (2 multi-dots + 2 multi-axpys, batched reductions);
//     `scratch` = 2 * kMaxMulti doubles for the two passes' coefficients.
// Shared by storm_hip_solve_gmres below and by the general engine (krylov_methods.hip).
// *normalised (nullable) = true when qn has already been divided by its norm (the cooperative chain does that).
int gmres_orthogonalize(storm_hip_ctx *c, int64_t n, const SolverState *st, const int *done, double *qn,
                        const double *const *q, int k, int m, double *H, double *norm2_out, double *scratch,
                        int gram_schmidt, bool *normalised, const MgsGivens *givens, bool *givens_done,
                        const ChainApply *apply) {
  // apply (nullable): qn = beta q[k] + alpha M(q[k]) has NOT been formed yet -- the cooperative chain does it itself where
  // it can (mgs_chain.hip: mgs_chain_quad_kernel<S, T, true>), otherwise it is formed here, before anything reads qn
  if (normalised) *normalised = false;
  if (givens_done) *givens_done = false;
  bool applied = false;
  if (gram_schmidt == 0 && n > 0) {  // small enough for registers: the whole chain as one cooperative kernel
    bool taken = false;
    STORM_TRY(gmres_mgs_chain_coop(c, n, done, qn, q, k, m, H, norm2_out, normalised != nullptr, &taken, givens, apply, &applied));
    if (taken && givens != nullptr && givens_done && c->opt_coop_mgs != 2) *givens_done = true;
    if (taken) {
      if (normalised) *normalised = true;
      return STORM_HIP_OK;
    }
  }
  if (apply != nullptr && !applied)
    STORM_TRY(spmv_launch(apply->op, host_scal(apply->alpha), host_scal(apply->beta), apply->x, qn, nullptr, done));
  const int nbv = stream_blocks(n);
  if (n <= 0) {  // an empty rank: zeros (and its share of the all-reduces)
    for (int i = 0; i <= k; ++i) {
      HIP_TRY(hipMemsetAsync(&H[i * m + k], 0, sizeof(double), c->stream));
      if (c->comm != nullptr) STORM_TRY(comm_allreduce_sum(c, &H[i * m + k], 1));
    }
    HIP_TRY(hipMemsetAsync(norm2_out, 0, sizeof(double), c->stream));
    if (c->comm != nullptr) STORM_TRY(comm_allreduce_sum(c, norm2_out, 1));
    return STORM_HIP_OK;
  }
  if (gram_schmidt == 0 && c->comm == nullptr && c->opt_ticket_reduce != 0) {
    // two steps per pass (mgs_pair_kernel): ceil((k + 1) / 2) + 1 launches for the k + 1 basis vectors
    const int nbp = (int)std::min<int64_t>(std::max<int64_t>(1, ((n >> 1) + kBlock - 1) / kBlock),
                                           std::min<int64_t>(32768, c->partials_capacity / 3));
    const TicketArgs t{c->d_tickets, c->d_partials, c->d_ticket_sums};
    const int nti = stream_nt(c, n);
    auto h_of = [&](int i) { return &H[(int64_t)i * m + k]; };
    auto launch = [&](int sub, int nsub, int nxt) {  // subtract q[sub .. sub + nsub), then the dots of q[nxt], q[nxt + 1]
      const int nnext = std::min(2, k + 1 - nxt);    // 2: a pair; 1: one vector; 0: the norm
      hipLaunchKernelGGL(mgs_pair_kernel, dim3(nbp), dim3(kBlock), 0, c->stream, n, done, qn,
                         nsub >= 1 ? h_of(sub) : nullptr, nsub >= 2 ? h_of(sub + 1) : nullptr,
                         nsub >= 1 ? q[sub] : nullptr, nsub >= 2 ? q[sub + 1] : nullptr,
                         nnext >= 1 ? q[nxt] : nullptr, nnext >= 2 ? q[nxt + 1] : nullptr,
                         nnext >= 1 ? h_of(nxt) : norm2_out, nnext >= 2 ? h_of(nxt + 1) : (double *)nullptr, t, nti);
    };
    const int64_t steps = c->opt_mgs_steps;
    // (two trips per thread: tools/multi_stream_bench.hip -- 5.47 TB/s against 5.35 with four and 5.45 with one)
    constexpr int kMgsTrips = 2;
    const int nbm = (int)std::min<int64_t>(std::max<int64_t>(1, ((n >> 1) + kBlock * kMgsTrips - 1) / (kBlock * kMgsTrips)), kMaxStreamBlocks);
    if ((steps == 3 || steps == 4) && k >= 2 && 10 * (int64_t)nbm <= c->partials_capacity &&
        10 * (int64_t)((nbm + kTicketGroup - 1) / kTicketGroup) <= 8 * 2048) {
      // three or four steps per pass (mgs_multi_kernel): ceil((k + 1) / T) + 1 launches
      auto go = [&](auto tag, int sub, int nsub, int nxt) {
        constexpr int T = decltype(tag)::value;
        MgsMultiArgs<T> a{};
        a.na = nsub, a.nc = std::max(0, std::min(T, k + 1 - nxt));
        for (int j = 0; j < T; ++j) {
          a.h[j] = h_of(sub + std::min(j, std::max(nsub - 1, 0))), a.qa[j] = q[std::min(sub + j, k)];
          a.qc[j] = q[std::min(nxt + j, k)], a.out[j] = j < a.nc ? h_of(nxt + j) : norm2_out;
        }
        hipLaunchKernelGGL((mgs_multi_kernel<T, kMgsTrips>), dim3(nbm), dim3(kBlock), 0, c->stream, n, done, qn, a, t, nti);
      };
      if (steps == 4) {
        go(std::integral_constant<int, 4>{}, 0, 0, 0);
        for (int i = 0; i <= k; i += 4) go(std::integral_constant<int, 4>{}, i, std::min(4, k + 1 - i), i + 4);
      } else {
        go(std::integral_constant<int, 3>{}, 0, 0, 0);
        for (int i = 0; i <= k; i += 3) go(std::integral_constant<int, 3>{}, i, std::min(3, k + 1 - i), i + 3);
      }
      HIP_TRY(hipGetLastError());
      return STORM_HIP_OK;
    }
    launch(0, 0, 0);
    for (int i = 0; i <= k; i += 2) launch(i, std::min(2, k + 1 - i), i + 2);
    HIP_TRY(hipGetLastError());
    return STORM_HIP_OK;
  }
  if (gram_schmidt == 0) {
    const bool fold_in_consumer = c->comm == nullptr && nbv <= 2048 && 2 * (int64_t)nbv <= c->partials_capacity;
    if (fold_in_consumer) {
      // partials ping-pong between two halves of the workspace: step i folds what step i-1 wrote
      double *cur = c->d_partials, *nxt = c->d_partials + nbv;
      STORM_TRY(k_dot_partials(c, qn, q[0], n, cur, nbv, done));
      for (int i = 0; i <= k; ++i) {
        const double *qb = i < k ? q[i + 1] : nullptr;
        hipLaunchKernelGGL(mgs_step_kernel, dim3(nbv), dim3(kBlock), 0, c->stream, n, done, qn,
                           (const double *)nullptr, cur, nbv, &H[i * m + k], q[i], qb, nxt,
                           stream_nt(c, n));
        HIP_TRY(hipGetLastError());
        std::swap(cur, nxt);
      }
      return k_reduce_final(c, cur, nbv, 1, norm2_out, done);  // <w, w>
    }
    {
      const double *bs[1] = {q[0]};
      STORM_TRY(k_multi_dot(c, qn, bs, 1, n, &H[0 * m + k], done));
      if (c->comm != nullptr) STORM_TRY(comm_allreduce_sum(c, &H[0 * m + k], 1));
    }
    for (int i = 0; i <= k; ++i) {
      double *h = &H[i * m + k];
      const double *qb = i < k ? q[i + 1] : nullptr;
      double *out = i < k ? &H[(i + 1) * m + k] : norm2_out;
      hipLaunchKernelGGL(mgs_step_kernel, dim3(nbv), dim3(kBlock), 0, c->stream, n, done, qn, h,
                         (const double *)nullptr, 0, (double *)nullptr, q[i], qb, c->d_partials,
                         stream_nt(c, n));
      HIP_TRY(hipGetLastError());
      STORM_TRY(k_reduce_final(c, c->d_partials, nbv, 1, out, done));
      if (c->comm != nullptr) STORM_TRY(comm_allreduce_sum(c, out, 1));
    }
    return STORM_HIP_OK;
  }
  // classical Gram-Schmidt applied twice; the second pass's coefficients are added to the first's (same span)
  for (int j0 = 0; j0 <= k; j0 += kMaxMulti) {  // restarts longer than one launch is wide: in chunks
    const int kk = std::min(k + 1 - j0, kMaxMulti);
    for (int pass = 0; pass < 2; ++pass) {
      STORM_TRY(k_multi_dot(c, qn, q + j0, kk, n, scratch + pass * kMaxMulti, done));
      if (c->comm != nullptr) STORM_TRY(comm_allreduce_sum(c, scratch + pass * kMaxMulti, kk));
      STORM_TRY(k_multi_axpy(c, qn, scratch + pass * kMaxMulti, -1.0, q + j0, kk, n, done));
    }
    hipLaunchKernelGGL(gmres_cgs2_combine_kernel, dim3(1), dim3(1), 0, c->stream, done, H, m, k, j0, kk, scratch);
    HIP_TRY(hipGetLastError());
  }
  {
    const double *bs[1] = {qn};
    STORM_TRY(k_multi_dot(c, qn, bs, 1, n, norm2_out, done));  // :161
    if (c->comm != nullptr) STORM_TRY(comm_allreduce_sum(c, norm2_out, 1));
  }
  return STORM_HIP_OK;
}


static int solve_gmres_body(const FusedSolveArgs &args) {
  const storm_hip_op *op = args.op;
  const double *b = args.b->d;
  double *x = args.x->d;
  const int m = (int)args.params->num_inner_iterations;
  STORM_REQUIRE(m >= 1 && m < kMaxMulti, "solve_gmres: num_inner_iterations = %d outside [1, %d)", m, kMaxMulti);
  Driver d;
  STORM_TRY(prepare_state(args, &d));
  storm_hip_ctx *c = d.c;
  const int64_t n = d.n;
  VecPool pool;
  STORM_TRY(pool.make(args.x, m + 1, false));  // q_0 .. q_m (SolverGmres.hpp:60-61): q_0 written by start(), q_k+1 by the apply of iteration k
  std::vector<const double *> q(m + 1);
  for (int i = 0; i <= m; ++i) q[i] = pool.v[i]->d;
  // H, beta, cs, sn                                                  SolverGmres.hpp:56-58
  const size_t gm_doubles = (size_t)(m + 1) * m + (m + 1) + m + m;
  if (gm_doubles > c->gmres_capacity) {  // (kept by the context: no allocation, no hipFree -- a device-wide wait -- per solve)
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->d_gmres) (void)hipFree(c->d_gmres);
    c->d_gmres = nullptr, c->gmres_capacity = 0;
    HIP_TRY(hipMalloc(&c->d_gmres, sizeof(double) * gm_doubles));
    c->gmres_capacity = gm_doubles;
  }
  double *d_gm = c->d_gmres;
  HIP_TRY(hipMemsetAsync(d_gm, 0, sizeof(double) * gm_doubles, c->stream));
  d.g = GmresDev{d_gm, d_gm + (size_t)(m + 1) * m, d_gm + (size_t)(m + 1) * m + (m + 1),
                 d_gm + (size_t)(m + 1) * m + (m + 1) + m, m};
  const int nbv = stream_blocks(n);
  int nb = 0;

  // q0 = b - A x; beta0 = |q0|; q0 /= beta0        (outer_init :82-88 and inner_init :110-116)
  auto start = [&](bool outer) -> int {
    double *q0 = const_cast<double *>(q[0]);
    STORM_TRY(d.apply(x, q0, &nb, {}, !outer));
    if (outer) {
      STORM_TRY(d.init_residual(q0, b, nullptr));
      STORM_TRY(d.finish(nbv, 1, S_TMP, STEP_GMRES_BETA0_OUTER, true));
      STORM_TRY(k_scale(c, q0, n, dev_scal(d.slot(S_HN)), true, nullptr));
    } else {
      STORM_TRY(k_axpbz(c, q0, host_scal(1.0), b, host_scal(-1.0), q0, n, d.done));
      const double *bs[1] = {q0};
      STORM_TRY(k_multi_dot(c, q0, bs, 1, n, d.slot(S_TMP), d.done));
      if (c->comm != nullptr) STORM_TRY(comm_allreduce_sum(c, d.slot(S_TMP), 1));
      STORM_TRY(d.step(STEP_GMRES_BETA0));
      STORM_TRY(k_scale(c, q0, n, dev_scal(d.slot(S_HN)), true, d.done));
    }
    return STORM_HIP_OK;
  };
  // x += sum_i beta_i q_i after the back substitution        inner_finalize :207-236
  auto finalize = [&](int k, bool force) -> int {
    hipLaunchKernelGGL(gmres_backsolve_kernel, dim3(1), dim3(kWave), 0, c->stream, d.st, d.g, k, force);
    HIP_TRY(hipGetLastError());
    return k_multi_axpy(c, x, d.g.beta, 1.0, q.data(), k + 1, n, force ? nullptr : d.done);
  };

  STORM_TRY(start(true));
  for (int64_t it = 0; it < args.params->num_iterations; ++it) {
    const int k = (int)(it % m);                         // Solver.hpp:239
    if (k == 0) STORM_TRY(start(false));                 // Solver.hpp:240-242
    double *qn = const_cast<double *>(q[k + 1]);
    // SolverGmres.hpp:155 -- by the chain kernel itself where the operator is a format-4 lattice one (one launch per inner
    // iteration, and qn = A q_k never travels through memory); gmres_orthogonalize applies it otherwise
    const ChainApply chain_apply{op, d.alpha, d.beta, q[k]};
    const bool defer_apply = args.params->gram_schmidt == 0 && c->comm == nullptr && c->opt_coop_mgs != 0 && c->opt_coop_mgs_apply != 0 &&
                             op->halo.n_nbrs == 0;
    if (!defer_apply) STORM_TRY(d.apply(q[k], qn, &nb));
    bool normalised = false, givens_done = false;
    // (the cooperative Gram-Schmidt chain, when it runs, also takes the root, normalises, applies the Givens
    //  rotations and the convergence rule in its last instructions: an inner iteration is then two launches)
    const MgsGivens givens{d.st, d.g.H, d.g.beta, d.g.cs, d.g.sn, d.slot(S_HN)};
    STORM_TRY(gmres_orthogonalize(c, n, d.st, d.done, qn, q.data(), k, m, d.g.H, d.slot(S_TMP), d.slot(S_SCRATCH),
                                  args.params->gram_schmidt, &normalised, &givens, &givens_done, defer_apply ? &chain_apply : nullptr));
    if (!givens_done) {
      STORM_TRY(d.step(STEP_GMRES_HN));
      if (!normalised) STORM_TRY(k_scale(c, qn, n, dev_scal(d.slot(S_HN)), true, d.done));      // :162
      hipLaunchKernelGGL(gmres_givens_kernel, dim3(1), dim3(kWave), 0, c->stream, d.st, d.g, k);    // :176-191
      HIP_TRY(hipGetLastError());
    }
    if (k == m - 1) STORM_TRY(finalize(k, false));       // Solver.hpp:244-246
    bool stop = false;
    STORM_TRY(post_and_poll(d, it, &stop));
    if (stop) break;
  }
  // InnerOuterIterativeSolver::finalize, Solver.hpp:250-257.  The in-loop finalize of the very
  // last iteration was skipped by the `done` predicate, so it always runs here.  (When no
  // iterate() ran the reference's finalize divides by H(0,0) = 0; that is not reproduced.)
  STORM_TRY(state_read(c, c->d_state, &c->h_state[0]));
  const int64_t iters = c->h_state[0].iteration;
  if (iters > 0) STORM_TRY(finalize((int)((iters - 1) % m), true));
  return collect(d, args, 1, m);
}

}  // namespace storm

extern "C" int storm_hip_solve_gmres(const storm_hip_op *op, double alpha, double beta, const storm_hip_vec *b, storm_hip_vec *x,
                                     const storm_hip_solver_params *params, storm_hip_solver_result *result, double *history) {
  if (op) STORM_TRY(storm::lazy_sync(op->ctx));
  return storm::fused_solve(storm::FusedSolveArgs{op, alpha, beta, b, x, params, result, history, &storm::solve_gmres_body});
}
