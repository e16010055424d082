// Mixed-precision CG (storm_hip_mixed_cg_*): fp32 inner iterations on the fp32-weight companion records under an fp64
// refinement loop that holds the answer to the reference's rule on the TRUE residual.  Algorithm and contract:
// include/storm_hip.h; DESIGN.md section 4.
//
// The contract extends op_reduced.hip's to vectors: an fp32 element is widened (exactly) where a kernel loads it, every
// operation is the fp64 kernel's in the same order with the same contraction, ONE round-to-nearest-even conversion at each
// fp32 store, sums in fp64.  So every vector statement below gives float(...) of the library's fp64 statement on the widened
// operands: storm_hip_op_apply_reduced (sell_row_apply<NT, Rec32> with the gathered element type float), storm_hip_axpy and
// storm_hip_xpay (axpbz_value, blas1_device.hpp -- the direction is xpay's r + fl(bt p), not one fma).
//
// Kernels (every one loads the context's api_done word -- and the inner loop's done word -- first and tests them before
// its first store; launches enqueued past the inner loop's exit store nothing):
//   mixed_begin_kernel      r32 = fl32(r_i (1 / rho)), d32 = 0, p32 = r32 (or the kept direction rescaled), g = <r32, r32>
//                           finished by tickets; the last block arms the inner loop's state.  Streaming, one pass.
//   mixed_apply_kernel      q32 = fl32(A~ p32) with <p32, q32>: spmv_sell32_kernel's / amg_residual_kernel's shape (one
//                           wavefront per slice, one row per lane, the operator's XCD runs, records non-temporal, p gathered
//                           plainly); the sum finished by tickets, the last block forms a = g / pq (pq <= 0 or not finite:
//                           BROKEN, the loop is done).
//   mixed_update_kernel     d32 = fl32(a p + d), r32 = fl32(-a q + r) with <r32, r32> finished by tickets; the last block
//                           forms bt = g' / g, g = g', counts the iteration, decides "leave" and posts the done word.
//   mixed_direction_kernel  p32 = fl32(r + bt p); gated on the iteration counter, so the leaving iteration's direction lands.
//   mixed_x_kernel          x = fma(rho, (double)d32, x) in fp64 (skipped when BROKEN).
//   mixed_widen_kernel      an fp32 vector into an fp64 one (storm_hip_mixed_cg_get_vector).
// Three launches per inner iteration, no host wait in it: the host polls the done word check_lag iterations behind
// (ring_wait, as post_and_poll does for the fused loops); one host wait per outer step (the true residual's norm).
//
// Access modes.  The apply has the two instances of op_reduced.hip's kernel (option nontemporal, asked through
// op_reduced_nt), the streaming kernels the two of blas1.hip's (option blas1_nt, asked through stream_nt_of): the choices
// are made by the owners of the two options.  Both instances of every kernel here run against the same bitwise pins in
// tests/test_gpu_mixed_cg.py::test_statements_bit_for_bit (blas1_nt 0 / 2 x nontemporal 0 / 1) and ::test_sums_are_exact_on_integers.
#include <cmath>
#include <cstring>

#include "amg_device.hpp"
#include "blas1_device.hpp"
#include "sell_device.hpp"
#include "solver_device.hpp"
#include "ticket_device.hpp"

namespace storm {

// The inner loop's device state (one per object).
struct MixedState {
  double rho, g, pq, alpha, beta, eta;
  long long it;                 // inner iterations of this outer step (an iteration counts once its <p, q> is formed)
  int done, broken;
  unsigned long long gen;       // generation of the ring words of this outer step
  unsigned long long *ring;     // device alias of the object's pinned ring (common.hpp ring_word)
};

typedef float float4v __attribute__((ext_vector_type(4)));

template <class NT>
__device__ __forceinline__ float4v ld4f(const float *p, NT) {
  const float4v *q = reinterpret_cast<const float4v *>(p);
  if constexpr (NT::value) return __builtin_nontemporal_load(q);
  else return *q;
}
template <class NT>
__device__ __forceinline__ void st4f(float *p, float4v v, NT) {
  float4v *q = reinterpret_cast<float4v *>(p);
  if constexpr (NT::value) __builtin_nontemporal_store(v, q);
  else *q = v;
}

constexpr int kMixedQuad = 4;                              // elements per thread and access (16 bytes of fp32)
constexpr int kMixedTrip = kBlock * kMixedQuad * 2;        // elements per block and trip: stream_blocks()' 2 048

// Every streaming kernel below: quads [4 i, 4 i + 4) by thread, two per trip, grid-stride; the thread that owns the ragged
// last quad takes its elements one by one.  body(i, m): elements i .. i + m - 1 (m = 4: the vector path).
template <class Body>
__device__ __forceinline__ void mixed_stream(int64_t n, Body &&body) {
  for (int64_t base = (int64_t)blockIdx.x * kMixedTrip + (int64_t)threadIdx.x * kMixedQuad; base < n;
       base += (int64_t)gridDim.x * kMixedTrip) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int64_t i = base + (int64_t)u * (kBlock * kMixedQuad);
      if (i + kMixedQuad <= n) body(i, kMixedQuad);
      else if (i < n) body(i, (int)(n - i));
    }
  }
}

// The block's sum into the ticket scheme; true in wave 0 of the block that drew the last ticket, total valid in all its lanes.
__device__ __forceinline__ bool mixed_finish_sum(double acc, const TicketArgs &t, double *total) {
  __shared__ double lds4[4];
  const double s = block_sum256(acc, lds4);
  if (threadIdx.x >= kWave) return false;
  const double mine[1] = {s};
  double tot[1];
  if (!ticket_reduce_wave0<1>(t, mine, 1, blockIdx.x, gridDim.x, tot)) return false;
  *total = tot[0];
  return true;
}

__device__ __forceinline__ void mixed_post(MixedState *st) {
  if (st->ring)
    __hip_atomic_store(st->ring + (st->it - 1) % kStateRing, ring_word(st->gen, (unsigned long long)st->it, st->done != 0),
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// r32 = fl32(r_i s), s = 1 / rho;  d32 = 0;  p32 = r32, or (ratio != 0) the kept direction fl32(p32_i ratio);  g = <r32, r32>.
__global__ __launch_bounds__(kBlock) void mixed_begin_kernel(int64_t n, const double *__restrict__ r, double rho, double rho_prev,
                                                             int keep, float *__restrict__ r32, float *__restrict__ p32,
                                                             float *__restrict__ d32, MixedState *st, TicketArgs t, double eta,
                                                             unsigned long long gen, unsigned long long *ring, const int *api_done,
                                                             int nt) {
  const int done_flag = api_done ? *api_done : 0;
  if (done_flag) return;  // (grid-uniform: set by a kernel in front of this one)
  const double s = 1.0 / rho;
  const double ratio = rho_prev / rho;
  double acc = 0.0;
  nt_dispatch(nt, [&](auto ntc) {
    mixed_stream(n, [&](int64_t i, int m) {
      if (m == kMixedQuad) {
        const double2v a = ld2(reinterpret_cast<const double2v *>(r + i), ntc), b = ld2(reinterpret_cast<const double2v *>(r + i) + 1, ntc);
        float4v pv = {0.f, 0.f, 0.f, 0.f};
        if (keep) pv = ld4f(p32 + i, ntc);
        float4v rv;
        rv.x = (float)(a.x * s), rv.y = (float)(a.y * s), rv.z = (float)(b.x * s), rv.w = (float)(b.y * s);
        if (keep) {
          pv.x = (float)((double)pv.x * ratio), pv.y = (float)((double)pv.y * ratio);
          pv.z = (float)((double)pv.z * ratio), pv.w = (float)((double)pv.w * ratio);
        } else {
          pv = rv;
        }
        acc += (double)rv.x * (double)rv.x;
        acc += (double)rv.y * (double)rv.y;
        acc += (double)rv.z * (double)rv.z;
        acc += (double)rv.w * (double)rv.w;
        st4f(r32 + i, rv, ntc);
        st4f(p32 + i, pv, ntc);
        st4f(d32 + i, float4v{0.f, 0.f, 0.f, 0.f}, ntc);
      } else {
        for (int e = 0; e < m; ++e) {
          const float rv = (float)(r[i + e] * s);
          const float pv = keep ? (float)((double)p32[i + e] * ratio) : rv;
          acc += (double)rv * (double)rv;
          r32[i + e] = rv, p32[i + e] = pv, d32[i + e] = 0.f;
        }
      }
    });
  });
  double total;
  if (!mixed_finish_sum(acc, t, &total)) return;
  if ((threadIdx.x & (kWave - 1)) == 0) {
    st->rho = rho, st->g = total, st->pq = 0.0, st->alpha = 0.0, st->beta = 0.0, st->eta = eta;
    st->it = 0, st->done = 0, st->broken = 0, st->gen = gen, st->ring = ring;
  }
}

// q32 = fl32(A~ p32), pq = <p32, q32>, a = g / pq.
template <bool NT, bool XCD>
__global__ __launch_bounds__(kBlock) void mixed_apply_kernel(SellArgs A, double alpha, double beta, const float *__restrict__ p32,
                                                             float *__restrict__ q32, int64_t n_slices, MixedState *st,
                                                             TicketArgs t, const int *api_done) {
  const int done_flag = (api_done ? *api_done : 0) | st->done;
  if (done_flag) return;  // (grid-uniform)
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int bidx = (int)blockIdx.x;
  const int lb = XCD ? (A.xcd_group > 1 ? xcd_remap_grouped(bidx, gridDim.x, A.xcd_group) : xcd_remap(bidx, gridDim.x))
                     : bidx;
  const int64_t slice = (int64_t)lb * (kBlock / kWave) + wave;
  double prod = 0.0;
  if (slice < n_slices) {  // wave-uniform (every wave meets the block sum's barriers below)
    const int64_t row = slice * kWave + lane;
    const bool valid = row < A.n_rows;
    const double pi = valid ? (double)p32[row] : 0.0;
    const double qd = sell_row_apply<NT, Rec32, false, float>(A, slice, lane, p32, pi, alpha, beta);
    const float qf = (float)qd;
    if (valid) {
      if (NT) __builtin_nontemporal_store(qf, q32 + row);
      else q32[row] = qf;
      prod = pi * (double)qf;
    }
  }
  double pq;
  if (!mixed_finish_sum(prod, t, &pq)) return;
  if (lane == 0) {
    st->pq = pq;
    st->alpha = st->g / pq;
    if (!(pq > 0.0) || !isfinite(pq)) {  // BROKEN: the iteration counts (its product ran), nothing of it is stored
      st->it = st->it + 1;
      st->broken = 1, st->done = 1;
      mixed_post(st);
    }
  }
}

// d32 = fl32(a p + d);  r32 = fl32(-a q + r);  g' = <r32, r32>;  bt = g' / g;  g = g'.
__global__ __launch_bounds__(kBlock) void mixed_update_kernel(int64_t n, const float *__restrict__ p32, const float *__restrict__ q32,
                                                              float *__restrict__ d32, float *__restrict__ r32, MixedState *st,
                                                              TicketArgs t, int check_exit, const int *api_done, int nt) {
  const int done_flag = (api_done ? *api_done : 0) | st->done;
  if (done_flag) return;  // (grid-uniform)
  const double a = st->alpha, na = -a;
  double acc = 0.0;
  nt_dispatch(nt, [&](auto ntc) {
    mixed_stream(n, [&](int64_t i, int m) {
      if (m == kMixedQuad) {
        const float4v pv = ld4f(p32 + i, ntc), qv = ld4f(q32 + i, ntc), dv = ld4f(d32 + i, ntc), rv = ld4f(r32 + i, ntc);
        float4v dn, rn;
        dn.x = (float)axpbz_value(a, (double)pv.x, 1.0, (double)dv.x), dn.y = (float)axpbz_value(a, (double)pv.y, 1.0, (double)dv.y);
        dn.z = (float)axpbz_value(a, (double)pv.z, 1.0, (double)dv.z), dn.w = (float)axpbz_value(a, (double)pv.w, 1.0, (double)dv.w);
        rn.x = (float)axpbz_value(na, (double)qv.x, 1.0, (double)rv.x), rn.y = (float)axpbz_value(na, (double)qv.y, 1.0, (double)rv.y);
        rn.z = (float)axpbz_value(na, (double)qv.z, 1.0, (double)rv.z), rn.w = (float)axpbz_value(na, (double)qv.w, 1.0, (double)rv.w);
        acc += (double)rn.x * (double)rn.x;
        acc += (double)rn.y * (double)rn.y;
        acc += (double)rn.z * (double)rn.z;
        acc += (double)rn.w * (double)rn.w;
        st4f(d32 + i, dn, ntc);
        st4f(r32 + i, rn, ntc);
      } else {
        for (int e = 0; e < m; ++e) {
          const float dn = (float)axpbz_value(a, (double)p32[i + e], 1.0, (double)d32[i + e]);
          const float rn = (float)axpbz_value(na, (double)q32[i + e], 1.0, (double)r32[i + e]);
          acc += (double)rn * (double)rn;
          d32[i + e] = dn, r32[i + e] = rn;
        }
      }
    });
  });
  double gn;
  if (!mixed_finish_sum(acc, t, &gn)) return;
  if ((threadIdx.x & (kWave - 1)) == 0) {
    st->beta = gn / st->g;
    st->g = gn;
    st->it = st->it + 1;
    if (!isfinite(gn)) st->broken = 1, st->done = 1;
    else if (check_exit && sqrt(gn) <= st->eta) st->done = 1;
    mixed_post(st);
  }
}

// p32 = fl32(r + bt p) of inner iteration my_it: it ran iff the counter reached it and the loop is not BROKEN.
__global__ __launch_bounds__(kBlock) void mixed_direction_kernel(int64_t n, float *__restrict__ p32, const float *__restrict__ r32,
                                                                 const MixedState *st, long long my_it, const int *api_done, int nt) {
  const int done_flag = (api_done ? *api_done : 0) | st->broken | (st->it < my_it ? 1 : 0);
  if (done_flag) return;
  const double bt = st->beta;
  nt_dispatch(nt, [&](auto ntc) {
    mixed_stream(n, [&](int64_t i, int m) {
      if (m == kMixedQuad) {
        const float4v pv = ld4f(p32 + i, ntc), rv = ld4f(r32 + i, ntc);
        float4v pn;
        pn.x = (float)axpbz_value(1.0, (double)rv.x, bt, (double)pv.x), pn.y = (float)axpbz_value(1.0, (double)rv.y, bt, (double)pv.y);
        pn.z = (float)axpbz_value(1.0, (double)rv.z, bt, (double)pv.z), pn.w = (float)axpbz_value(1.0, (double)rv.w, bt, (double)pv.w);
        st4f(p32 + i, pn, ntc);
      } else {
        for (int e = 0; e < m; ++e) p32[i + e] = (float)axpbz_value(1.0, (double)r32[i + e], bt, (double)p32[i + e]);
      }
    });
  });
}

// x = fma(rho, (double)d32_i, x_i); skipped when the inner loop is BROKEN.
__global__ __launch_bounds__(kBlock) void mixed_x_kernel(int64_t n, double *__restrict__ x, const float *__restrict__ d32, double rho,
                                                         const MixedState *st, const int *api_done, int nt) {
  const int done_flag = (api_done ? *api_done : 0) | st->broken;
  if (done_flag) return;
  nt_dispatch(nt, [&](auto ntc) {
    mixed_stream(n, [&](int64_t i, int m) {
      if (m == kMixedQuad) {
        double2v *xp = reinterpret_cast<double2v *>(x + i);
        const float4v dv = ld4f(d32 + i, ntc);
        double2v a = ld2(xp, ntc), b = ld2(xp + 1, ntc);
        a.x = __builtin_fma(rho, (double)dv.x, a.x), a.y = __builtin_fma(rho, (double)dv.y, a.y);
        b.x = __builtin_fma(rho, (double)dv.z, b.x), b.y = __builtin_fma(rho, (double)dv.w, b.y);
        st2(xp, a, ntc);
        st2(xp + 1, b, ntc);
      } else {
        for (int e = 0; e < m; ++e) x[i + e] = __builtin_fma(rho, (double)d32[i + e], x[i + e]);
      }
    });
  });
}

__global__ __launch_bounds__(kBlock) void mixed_widen_kernel(int64_t n, const float *__restrict__ v32, double *__restrict__ out,
                                                             const int *api_done) {
  const int done_flag = api_done ? *api_done : 0;
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < n && !done_flag) out[i] = (double)v32[i];
}

}  // namespace storm

using namespace storm;

struct storm_hip_mixed_cg {
  storm_hip_ctx *ctx = nullptr;
  const storm_hip_op *op = nullptr;  // not owned
  double alpha = 0.0, beta = 0.0;
  storm_hip_mixed_params mp{};
  int64_t n = 0;
  float *v32[4] = {nullptr, nullptr, nullptr, nullptr};  // r32, p32, q32, d32 (padded to whole slices + one, zeroed once)
  storm_hip_vec *r = nullptr;                             // the fp64 residual
  const storm_hip_vec *b = nullptr;                       // of the solve in progress
  MixedState *d_st = nullptr, *h_st = nullptr;            // device state, pinned copy
  unsigned long long *h_ring = nullptr, *d_ring = nullptr;
  unsigned long long gen = 0;
  int *d_cnt = nullptr;                                   // the object's own ticket counters and partial sums
  double *d_part1 = nullptr, *d_part2 = nullptr;
  int nb_apply = 0, nb_stream = 0;
  double rho = 0.0;                                       // the true residual's norm the running outer step started from
  int64_t enqueued = 0;                                   // inner iterations enqueued in the running outer step
  bool begun = false;
};

namespace storm {

enum { V_R32 = 0, V_P32 = 1, V_Q32 = 2, V_D32 = 3 };

static TicketArgs mixed_tickets(const storm_hip_mixed_cg *m) { return TicketArgs{m->d_cnt, m->d_part1, m->d_part2}; }

// What may run: fp64 records with a companion, no CSR tail, one rank.  Decided on the host before any launch.
static int mixed_require(const storm_hip_op *op, const char *who) {
  STORM_TRY(op_reduced_check(op, who));
  if (op->tail_rows > 0)
    STORM_FAIL(STORM_HIP_E_UNSUPPORTED, "%s: the operator has a CSR tail (%lld rows longer than the slices' width); the mixed-precision "
                                        "loop takes operators without one", who, (long long)op->tail_rows);
  STORM_TRY(op_reduced_require(op, who));
  if (blocks_for(op, op->n_slices) > kTicketGroup * kTicketMaxGroups)
    STORM_FAIL(STORM_HIP_E_UNSUPPORTED, "%s: %lld rows are more than the in-kernel reductions take", who, (long long)op->n_rows);
  return STORM_HIP_OK;
}

// r = b - A x on the fp64 records and its norm: the library's own entry points (one host wait).
static int mixed_true_residual(storm_hip_mixed_cg *m, const storm_hip_vec *x, double *rho) {
  STORM_TRY(storm_hip_op_apply(m->op, m->alpha, m->beta, x, m->r));
  STORM_TRY(storm_hip_axpbz(m->r, 1.0, m->b, -1.0, m->r));
  return storm_hip_norm2(m->r, rho);
}

// The conversion in front of an outer step: r -> r32, d32 = 0, the direction reset or (keep) rescaled, g; arms the state.
static int mixed_convert(storm_hip_mixed_cg *m, double rho, double rho_prev, bool keep, double eta) {
  storm_hip_ctx *c = m->ctx;
  for (int i = 0; i < kStateRing; ++i) m->h_ring[i] = 0;  // (the step before ended with a host wait: nothing posts any more)
  m->gen = (m->gen + 1) & 0xfffffull;
  if (m->gen == 0) m->gen = 1;
  hipLaunchKernelGGL(mixed_begin_kernel, dim3(m->nb_stream), dim3(kBlock), 0, c->stream, m->n, m->r->d, rho, rho_prev, keep ? 1 : 0,
                     m->v32[V_R32], m->v32[V_P32], m->v32[V_D32], m->d_st, mixed_tickets(m), eta, m->gen, m->d_ring, c->api_done,
                     stream_nt_of(c, m->n));
  HIP_TRY(hipGetLastError());
  m->rho = rho, m->enqueued = 0, m->begun = true;
  return STORM_HIP_OK;
}

// One inner iteration: three launches, nothing waits.
static int mixed_enqueue_iteration(storm_hip_mixed_cg *m, bool check_exit) {
  storm_hip_ctx *c = m->ctx;
  const storm_hip_op *op = m->op;
  const SellArgs A{op->d_pack32, op->d_slice_off32, op->n_rows, op->uniform_width, op->xcd_group_sell, nullptr, 0, nullptr, 0, 0};
  const dim3 grid(m->nb_apply), block(kBlock);
  const bool nt = op_reduced_nt(op), xcd = op->xcd_group_sell != 0;
  const TicketArgs t = mixed_tickets(m);
#define MIXED_APPLY_GO(NT_, XCD_)                                                                                            \
  hipLaunchKernelGGL((mixed_apply_kernel<NT_, XCD_>), grid, block, 0, c->stream, A, m->alpha, m->beta, m->v32[V_P32], m->v32[V_Q32], \
                     op->n_slices, m->d_st, t, c->api_done)
  if (nt && xcd) MIXED_APPLY_GO(true, true);
  else if (nt) MIXED_APPLY_GO(true, false);
  else if (xcd) MIXED_APPLY_GO(false, true);
  else MIXED_APPLY_GO(false, false);
#undef MIXED_APPLY_GO
  const int snt = stream_nt_of(c, m->n);
  hipLaunchKernelGGL(mixed_update_kernel, dim3(m->nb_stream), block, 0, c->stream, m->n, m->v32[V_P32], m->v32[V_Q32], m->v32[V_D32],
                     m->v32[V_R32], m->d_st, t, check_exit ? 1 : 0, c->api_done, snt);
  ++m->enqueued;
  hipLaunchKernelGGL(mixed_direction_kernel, dim3(m->nb_stream), block, 0, c->stream, m->n, m->v32[V_P32], m->v32[V_R32], m->d_st,
                     (long long)m->enqueued, c->api_done, snt);
  HIP_TRY(hipGetLastError());
  return STORM_HIP_OK;
}

// The end of an outer step: x += rho d (unless BROKEN), the true residual and its norm, the inner loop's state on the host.
static int mixed_end_outer(storm_hip_mixed_cg *m, storm_hip_vec *x, double *rho) {
  storm_hip_ctx *c = m->ctx;
  hipLaunchKernelGGL(mixed_x_kernel, dim3(m->nb_stream), dim3(kBlock), 0, c->stream, m->n, x->d, m->v32[V_D32], m->rho, m->d_st,
                     c->api_done, stream_nt_of(c, m->n));
  HIP_TRY(hipGetLastError());
  STORM_TRY(mixed_true_residual(m, x, rho));
  HIP_TRY(hipMemcpyAsync(m->h_st, m->d_st, sizeof(MixedState), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return STORM_HIP_OK;
}

static int mixed_check_vectors(const storm_hip_mixed_cg *m, const storm_hip_vec *b, const storm_hip_vec *x, const char *who) {
  STORM_REQUIRE(b->ctx == m->ctx && x->ctx == m->ctx, "%s: context mismatch", who);
  STORM_REQUIRE(b->n_owned == m->n && x->n_owned == m->n, "%s: the operator has %lld rows, b %lld, x %lld", who, (long long)m->n,
                (long long)b->n_owned, (long long)x->n_owned);
  STORM_REQUIRE(b != x && b->d != x->d, "%s: b and x must not alias", who);
  return STORM_HIP_OK;
}

static bool rule_converged(const storm_hip_solver_params *p, double abs_err, double rho0) {
  return (p->absolute_error_tolerance > 0.0 && abs_err < p->absolute_error_tolerance) ||
         (p->relative_error_tolerance > 0.0 && abs_err / rho0 < p->relative_error_tolerance);
}

static void mixed_free(storm_hip_mixed_cg *m) {
  for (float *&v : m->v32) (void)hipFree(v), v = nullptr;
  if (m->r) (void)storm_hip_vec_destroy(m->r), m->r = nullptr;
  (void)hipFree(m->d_st), (void)hipFree(m->d_cnt), (void)hipFree(m->d_part1), (void)hipFree(m->d_part2);
  if (m->h_st) (void)hipHostFree(m->h_st);
  if (m->h_ring) (void)hipHostFree(m->h_ring);
  delete m;
}

}  // namespace storm

extern "C" {

void storm_hip_mixed_params_default(storm_hip_mixed_params *p) {
  if (!p) return;
  p->inner_tolerance = 1e-3;
  p->inner_max = 0;
  p->max_outer = 16;
  p->keep_direction = 0;
}

int storm_hip_mixed_cg_create(const storm_hip_op *op, double alpha, double beta, const storm_hip_mixed_params *params,
                              storm_hip_mixed_cg **out) {
  STORM_REQUIRE(out && params, "mixed_cg_create: null argument");
  *out = nullptr;
  STORM_REQUIRE(params->inner_tolerance > 0.0 && params->inner_tolerance < 1.0, "mixed_cg_create: inner_tolerance %g is not in (0, 1)",
                params->inner_tolerance);
  STORM_REQUIRE(params->inner_max >= 0, "mixed_cg_create: inner_max %lld < 0", (long long)params->inner_max);
  STORM_REQUIRE(params->max_outer >= 1, "mixed_cg_create: max_outer %d < 1", (int)params->max_outer);
  STORM_REQUIRE(params->keep_direction == 0 || params->keep_direction == 1, "mixed_cg_create: keep_direction %d is neither 0 nor 1",
                (int)params->keep_direction);
  STORM_REQUIRE(op, "mixed_cg_create: null argument");
  STORM_TRY(mixed_require(op, "mixed_cg_create"));
  storm_hip_ctx *c = op->ctx;
  HIP_TRY(hipSetDevice(c->device));
  STORM_TRY(lazy_sync(c));
  storm_hip_mixed_cg *m = new storm_hip_mixed_cg;
  m->ctx = c, m->op = op, m->alpha = alpha, m->beta = beta, m->mp = *params, m->n = op->n_rows;
  m->nb_apply = blocks_for(op, op->n_slices), m->nb_stream = stream_blocks(m->n);
  if (m->nb_apply < 1) m->nb_apply = 1;
  const size_t n32 = (size_t)(op->n_slices + 1) * kWave;  // whole slices (a padding slot gathers its own row) and one beyond
  const int nb = m->nb_apply > m->nb_stream ? m->nb_apply : m->nb_stream;
  const size_t cnt_bytes = sizeof(int) * (size_t)(1 + kTicketMaxGroups) * kTicketStride;
  hipError_t e = hipSuccess;
  for (int k = 0; k < 4 && e == hipSuccess; ++k) {
    e = hipMalloc((void **)&m->v32[k], sizeof(float) * n32);
    if (e == hipSuccess) e = hipMemsetAsync(m->v32[k], 0, sizeof(float) * n32, c->stream);
  }
  if (e == hipSuccess) e = hipMalloc((void **)&m->d_st, sizeof(MixedState));
  if (e == hipSuccess) e = hipMemsetAsync(m->d_st, 0, sizeof(MixedState), c->stream);
  if (e == hipSuccess) e = hipMalloc((void **)&m->d_cnt, cnt_bytes);
  if (e == hipSuccess) e = hipMemsetAsync(m->d_cnt, 0, cnt_bytes, c->stream);
  if (e == hipSuccess) e = hipMalloc((void **)&m->d_part1, sizeof(double) * (size_t)nb);
  if (e == hipSuccess) e = hipMalloc((void **)&m->d_part2, sizeof(double) * (size_t)kTicketMaxGroups);
  if (e == hipSuccess) e = hipHostMalloc((void **)&m->h_st, sizeof(MixedState), hipHostMallocDefault);
  if (e == hipSuccess) e = hipHostMalloc((void **)&m->h_ring, sizeof(unsigned long long) * kStateRing, hipHostMallocDefault);
  if (e == hipSuccess) e = hipHostGetDevicePointer((void **)&m->d_ring, m->h_ring, 0);
  int st = STORM_HIP_OK;
  if (e == hipSuccess) {
    memset(m->h_st, 0, sizeof(MixedState));
    for (int i = 0; i < kStateRing; ++i) m->h_ring[i] = 0;
    st = storm_hip_vec_create(c, m->n, 0, &m->r);
  }
  if (e == hipSuccess && st == STORM_HIP_OK) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess || st != STORM_HIP_OK) {
    mixed_free(m);
    if (st != STORM_HIP_OK) return st;
    STORM_FAIL(STORM_HIP_E_ALLOC, "mixed_cg_create: allocation failed: %s", hipGetErrorString(e));
  }
  *out = m;
  return STORM_HIP_OK;
}

int storm_hip_mixed_cg_destroy(storm_hip_mixed_cg *m) {
  if (!m) return STORM_HIP_OK;
  (void)hipSetDevice(m->ctx->device);
  (void)hipStreamSynchronize(m->ctx->stream);  // kernels in flight may still use the buffers
  mixed_free(m);
  return STORM_HIP_OK;
}

int storm_hip_mixed_cg_begin(storm_hip_mixed_cg *m, const storm_hip_vec *b, const storm_hip_vec *x) {
  STORM_REQUIRE(m && b && x, "mixed_cg_begin: null argument");
  STORM_TRY(mixed_check_vectors(m, b, x, "mixed_cg_begin"));
  STORM_TRY(mixed_require(m->op, "mixed_cg_begin"));
  HIP_TRY(hipSetDevice(m->ctx->device));
  m->b = b;
  double rho = 0.0;
  STORM_TRY(mixed_true_residual(m, x, &rho));
  STORM_REQUIRE(rho > 0.0 && std::isfinite(rho), "mixed_cg_begin: the residual's norm %g leaves nothing to scale", rho);
  return mixed_convert(m, rho, rho, false, m->mp.inner_tolerance);
}

int storm_hip_mixed_cg_inner(storm_hip_mixed_cg *m, int64_t n_iterations) {
  STORM_REQUIRE(m, "mixed_cg_inner: null argument");
  STORM_REQUIRE(m->begun, "mixed_cg_inner: call storm_hip_mixed_cg_begin first");
  STORM_REQUIRE(n_iterations >= 0, "mixed_cg_inner: a negative count");
  STORM_TRY(mixed_require(m->op, "mixed_cg_inner"));
  HIP_TRY(hipSetDevice(m->ctx->device));
  for (int64_t j = 0; j < n_iterations; ++j) STORM_TRY(mixed_enqueue_iteration(m, false));
  return STORM_HIP_OK;
}

int storm_hip_mixed_cg_end_outer(storm_hip_mixed_cg *m, storm_hip_vec *x, double *rho) {
  STORM_REQUIRE(m && x && rho, "mixed_cg_end_outer: null argument");
  STORM_REQUIRE(m->begun, "mixed_cg_end_outer: call storm_hip_mixed_cg_begin first");
  STORM_TRY(mixed_check_vectors(m, m->b, x, "mixed_cg_end_outer"));
  HIP_TRY(hipSetDevice(m->ctx->device));
  STORM_TRY(mixed_end_outer(m, x, rho));
  m->begun = false;
  return STORM_HIP_OK;
}

int storm_hip_mixed_cg_get_vector(storm_hip_mixed_cg *m, const char *name, storm_hip_vec *out) {
  STORM_REQUIRE(m && name && out, "mixed_cg_get_vector: null argument");
  STORM_REQUIRE(out->ctx == m->ctx && out->n_owned == m->n, "mixed_cg_get_vector: the vector must be of the operator's context and size");
  int k = -1;
  if (!strcmp(name, "r32")) k = V_R32;
  else if (!strcmp(name, "p32")) k = V_P32;
  else if (!strcmp(name, "q32")) k = V_Q32;
  else if (!strcmp(name, "d32")) k = V_D32;
  STORM_REQUIRE(k >= 0, "mixed_cg_get_vector: unknown vector '%s' (r32, p32, q32, d32)", name);
  storm_hip_ctx *c = m->ctx;
  HIP_TRY(hipSetDevice(c->device));
  STORM_TRY(lazy_sync(c));
  if (m->n > 0)
    hipLaunchKernelGGL(mixed_widen_kernel, dim3((unsigned)((m->n + kBlock - 1) / kBlock)), dim3(kBlock), 0, c->stream, m->n, m->v32[k],
                       out->d, c->api_done);
  HIP_TRY(hipGetLastError());
  return STORM_HIP_OK;
}

int storm_hip_mixed_cg_get_scalar(storm_hip_mixed_cg *m, const char *name, double *value) {
  STORM_REQUIRE(m && name && value, "mixed_cg_get_scalar: null argument");
  storm_hip_ctx *c = m->ctx;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpyAsync(m->h_st, m->d_st, sizeof(MixedState), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  const MixedState &h = *m->h_st;
  if (!strcmp(name, "rho")) *value = h.rho;
  else if (!strcmp(name, "g")) *value = h.g;
  else if (!strcmp(name, "pq")) *value = h.pq;
  else if (!strcmp(name, "alpha")) *value = h.alpha;
  else if (!strcmp(name, "beta")) *value = h.beta;
  else STORM_FAIL(STORM_HIP_E_INVALID, "mixed_cg_get_scalar: unknown scalar '%s' (rho, g, pq, alpha, beta)", name);
  return STORM_HIP_OK;
}

int storm_hip_mixed_cg_solve(storm_hip_mixed_cg *m, const storm_hip_vec *b, storm_hip_vec *x, const storm_hip_solver_params *params,
                             storm_hip_solver_result *result, double *history, storm_hip_mixed_result *mixed_result) {
  STORM_REQUIRE(m && b && x && params && result, "mixed_cg_solve: null argument");
  STORM_TRY(mixed_check_vectors(m, b, x, "mixed_cg_solve"));
  STORM_REQUIRE(params->num_iterations >= 0, "mixed_cg_solve: num_iterations < 0");
  STORM_TRY(mixed_require(m->op, "mixed_cg_solve"));
  storm_hip_ctx *c = m->ctx;
  HIP_TRY(hipSetDevice(c->device));
  STORM_TRY(lazy_sync(c));
  m->b = b;
  storm_hip_mixed_result mr{0, 0, 0, 0};
  *result = storm_hip_solver_result{};
  int lag = params->check_lag > 0 ? params->check_lag : 4;
  if (lag > kStateRing - 1) lag = kStateRing - 1;

  double rho0 = 0.0;
  STORM_TRY(mixed_true_residual(m, x, &rho0));
  if (history) history[0] = rho0;
  result->initial_error = result->absolute_error = rho0, result->num_applies = 1;
  const double abs_tol = params->absolute_error_tolerance, rel_tol = params->relative_error_tolerance;
  const bool early = abs_tol > 0.0 && rho0 < abs_tol;  // Solver.hpp:122-128
  double target = 0.0;
  if (abs_tol > 0.0) target = abs_tol;
  if (rel_tol > 0.0 && rel_tol * rho0 > target) target = rel_tol * rho0;

  double rho = rho0, rho_prev = rho0;
  bool converged = early;
  int finish = 0;
  if (!early && !(rho0 > 0.0 && std::isfinite(rho0))) finish = 3;  // nothing to scale by: not converged, nothing runs
  while (!converged && finish == 0 && params->num_iterations > 0) {
    const int64_t left = params->num_iterations - mr.inner_iterations;
    int64_t inner_max = m->mp.inner_max > 0 ? m->mp.inner_max : params->num_iterations;
    if (inner_max > left) inner_max = left;
    double eta = 0.5 * target / rho;  // never deeper than the outer rule needs
    if (!(eta > m->mp.inner_tolerance)) eta = m->mp.inner_tolerance;
    STORM_TRY(mixed_convert(m, rho, rho_prev, m->mp.keep_direction != 0 && mr.outer_steps > 0, eta));
    for (int64_t j = 0; j < inner_max; ++j) {
      STORM_TRY(mixed_enqueue_iteration(m, true));
      bool stop = false;
      if (j >= lag) STORM_TRY(ring_wait(c, m->h_ring, j - lag, &stop, m->gen));
      if (stop) break;
    }
    double rho_new = 0.0;
    STORM_TRY(mixed_end_outer(m, x, &rho_new));
    m->begun = false;
    ++mr.outer_steps;
    mr.inner_iterations += m->h_st->it;
    result->num_applies += m->h_st->it + 1;
    if (history) history[mr.outer_steps] = rho_new;
    const bool broken = m->h_st->broken != 0;
    rho_prev = rho;
    converged = rule_converged(params, rho_new, rho0);
    if (!converged) {
      if (broken) finish = 2;
      else if (!(rho_new < rho)) finish = 1;
      else if (mr.outer_steps >= m->mp.max_outer || mr.inner_iterations >= params->num_iterations) finish = 3;
    }
    rho = rho_new;
  }
  if (!converged && finish == 0) finish = 3;  // (num_iterations = 0)
  result->absolute_error = rho;

  if (!converged && finish != 0 && rho > 0.0 && std::isfinite(rho) && mr.inner_iterations < params->num_iterations) {
    // the existing fp64 loop from this x with the iterations that are left, stopping at the SAME residual norm: its relative
    // rule is taken against its own first residual, so the tolerance is rescaled by rho_0 / |r| (unchanged where they agree)
    storm_hip_solver_params p2 = *params;
    p2.num_iterations = params->num_iterations - mr.inner_iterations;
    if (rel_tol > 0.0 && rho != rho0) p2.relative_error_tolerance = rel_tol * rho0 / rho;
    storm_hip_solver_result r2{};
    std::vector<double> h2(history ? (size_t)p2.num_iterations + 1 : 0);
    STORM_TRY(storm_hip_solve_cg(m->op, m->alpha, m->beta, b, x, &p2, &r2, history ? h2.data() : nullptr));
    for (int64_t k = 1; history && k <= r2.iterations; ++k) history[mr.outer_steps + k] = h2[(size_t)k];
    mr.fp64_iterations = r2.iterations;
    result->num_applies += r2.num_applies;
    result->path_fallback = r2.path_fallback;
    result->absolute_error = r2.absolute_error;
    converged = r2.converged != 0;
  }
  mr.finished_fp64 = finish;
  result->iterations = mr.inner_iterations + mr.fp64_iterations;
  result->relative_error = early ? 0.0 : result->absolute_error / rho0;
  result->converged = converged ? 1 : 0;
  ++c->n_mixed_solves;
  c->n_mixed_inner_iterations += mr.inner_iterations;
  c->n_mixed_outer_steps += mr.outer_steps;
  if (mr.finished_fp64 != 0) ++c->n_mixed_fp64_finishes;
  if (mixed_result) *mixed_result = mr;
  return STORM_HIP_OK;
}

}  // extern "C"
