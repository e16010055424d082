// The cooperative tail of the multigrid cycle (option amg_tail): from a level t down to the coarsest level and back up to t,
// ONE kernel whose blocks are all resident runs what amg_cycle / amg_cycle_jacobi (amg.hip) enqueue as about 11 launches per
// level.  The cycle has no reduction and every output row is a function of that row's record and of gathered inputs, so the
// kernel is the cycle's statements ("THE CYCLE", include/storm_hip.h) as PHASES between grid barriers, and the bits are those
// of the launches: every row goes through the functions of amg_device.hpp that the launched kernels call.
//
//   grid      blocks of kLatBlock threads; at most 256 (the slot all-reduce's limit), at most one per CU, no more than the
//             largest tail level has slices for; launched through coop_launch (coop_plain, coop_force_fail, coop_disabled hold).
//   phases    a table on the device, built on the host by walking the cycle (amg_tail_build): each entry names the statement,
//             the level whose records / scale it reads, its coefficients and its vectors.  Between two phases every block passes
//             co_allreduce_slots with one dummy value -- the barrier of every cooperative kernel here (coop_device.hpp).  Merged
//             where no row reads another row's output of the same phase: the smoother's start d_0 = it (s .* r) into the phase
//             that forms r (the restriction; the post-smoother's residual), the closing z = z + e into the last smoother step.
//             Inside a phase the waves take slices in a grid-stride loop; a block without a slice still arrives at the barrier.
//   coherence every vector element written here crosses blocks (and XCDs) before the next phase reads it: stores are
//             co_publish (the awaited exchange; option latency_publish), every load of a vector the kernel writes is co_load --
//             the gathers through the CO instance of row_sum_any / ld_cols -- and the barrier is the SEEN form, as in
//             latency.hip.  No whole-cache fence.  Records, scales, transfer records and the dense inverse are read-only:
//             plain loads (the one access mode of this unit).
//   safety    every wait is co_bounded_wait on the shared give-up flag (lat_gave_up); the context's api_done word is loaded
//             first and every block leaves before its first barrier when it is set; sequence numbers as the Gram-Schmidt
//             chains draw them (bit 31 set, c->lat_seq advanced by the launch's barrier count, taken back on a refusal).
#include <algorithm>
#include <cstring>
#include <vector>

#include "amg.hpp"
#include "amg_device.hpp"
#include "coop_device.hpp"

namespace storm {

enum : int { kTailD0 = 0, kTailStep, kTailResidual, kTailSweep, kTailTransfer, kTailCoarse };
enum : int { kTailFirst = 1, kTailLast = 2, kTailAxpy = 4, kTailWithD0 = 8, kTailAdd = 16 };

struct AmgTailLevel {
  SellArgs A;                 // the level operator's fp64 records: the residual's
  const char *pack_s;         // the smoother's records: the same, or the fp32-weight companion of a reduced object
  const int64_t *off_s;
  double alpha, beta;
  const double *dinv;         // the Jacobi scale s
  int64_t n_slices;
};

// Vector ids: 0 the caller's r, 1 the caller's z (they change from apply to apply: kernel arguments), >= 2 the table's.
struct AmgTailPhase {
  int kind, level, flags, pad;
  double a, b;                // D0: a = 1 / theta (Jacobi: sigma); STEP: c1, c2; SWEEP: a = sigma
  int v[6];
  const char *tpack;          // TRANSFER: the transfer records; COARSE: the dense inverse
  const int64_t *toff;
  int64_t n_rows, n_slices;   // of what the phase writes
};

struct AmgTailArgs {
  const AmgTailLevel *levels;
  const AmgTailPhase *phases;
  double *const *vecs;
  int n_phases, publish_xchg;
  const double *r;
  double *z;
  char *slots;
  unsigned long long seq_base;  // tags of this launch: seq_base + 1 .. seq_base + n_phases - 1
  const int *done;
};

// R: the record policy of the SMOOTHER's products (Rec32 for a reduced object); the residual reads the fp64 records always.
template <class R>
__global__ __launch_bounds__(kLatBlock) void amg_tail_kernel(AmgTailArgs a) {
  const int done_flag = a.done ? *a.done : 0;
  if (done_flag) return;  // (the same word in every block: it is written by kernels earlier on the stream only)
  __shared__ double lds[kLatWaves];
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave_id = (int64_t)blockIdx.x * kLatWaves + (threadIdx.x >> 6);
  const int64_t n_waves = (int64_t)gridDim.x * kLatWaves;
  unsigned long long seq = a.seq_base, seen = 0;  // seen: what the publishing exchanges returned (consumed at the barriers)
  const int xchg = a.publish_xchg;
  auto vec = [&](int id) -> double * { return id == 0 ? const_cast<double *>(a.r) : id == 1 ? a.z : a.vecs[id]; };
  for (int p = 0; p < a.n_phases; ++p) {
    const AmgTailPhase &P = a.phases[p];
    const AmgTailLevel &L = a.levels[P.level];
    const int flags = P.flags;
    switch (P.kind) {
      case kTailD0: {  // out = a (s .* in)
        const double *in = vec(P.v[0]);
        double *out = vec(P.v[1]);
        for (int64_t s = wave_id; s < P.n_slices; s += n_waves) {
          const int64_t row = s * kWave + lane;
          if (row < P.n_rows) co_publish(out + row, cheb_d0_value<true>(P.a, co_load(in + row), L.dinv[row]), xchg, seen);
        }
      } break;
      case kTailStep: {  // cheb_step_kernel's row; kTailAxpy: z = z + e in place of the store of e
        const double *d = vec(P.v[0]), *res_in = vec(P.v[1]);
        double *zv = vec(P.v[2]), *d_out = vec(P.v[3]), *res_out = vec(P.v[4]), *zz = vec(P.v[5]);
        SellArgs A = L.A;
        A.pack = L.pack_s, A.slice_off = L.off_s;
        const bool first = (flags & kTailFirst) != 0, last = (flags & kTailLast) != 0;
        for (int64_t s = wave_id; s < P.n_slices; s += n_waves) {
          const int64_t row = s * kWave + lane;
          const bool valid = row < P.n_rows;
          const double xi = valid ? co_load(d + row) : 0.0;
          const double ri = valid ? co_load(res_in + row) : 0.0;
          const double si = valid ? L.dinv[row] : 0.0;
          const double zi = (valid && !first) ? co_load(zv + row) : 0.0;
          const double t = sell_row_apply<false, R, true>(A, s, lane, d, xi, L.alpha, L.beta);
          const ChebRow o = first ? cheb_step_row<true, true>(t, ri, si, xi, zi, P.a, P.b)
                                  : cheb_step_row<true, false>(t, ri, si, xi, zi, P.a, P.b);
          if (valid) {
            if (!last) co_publish(res_out + row, o.rn, xchg, seen), co_publish(d_out + row, o.dn, xchg, seen);
            if (flags & kTailAxpy) co_publish(zz + row, amg_axpy_value(o.zn, co_load(zz + row)), xchg, seen);
            else co_publish(zv + row, o.zn, xchg, seen);
          }
        }
      } break;
      case kTailResidual: {  // t = r - A z; kTailWithD0: and the post-smoother's d_0 = a (s .* t)
        const double *r = vec(P.v[0]), *z = vec(P.v[1]);
        double *t = vec(P.v[2]), *d0 = vec(P.v[3]);
        for (int64_t s = wave_id; s < P.n_slices; s += n_waves) {
          const int64_t row = s * kWave + lane;
          const bool valid = row < P.n_rows;
          const double zi = valid ? co_load(z + row) : 0.0;
          const double ri = valid ? co_load(r + row) : 0.0;
          const double az = sell_row_apply<false, Rec64, true>(L.A, s, lane, z, zi, L.alpha, L.beta);
          const double tn = amg_residual_value(ri, az);
          if (valid) {
            co_publish(t + row, tn, xchg, seen);
            if (flags & kTailWithD0) co_publish(d0 + row, cheb_d0_value<true>(P.a, tn, L.dinv[row]), xchg, seen);
          }
        }
      } break;
      case kTailSweep: {  // amg_jacobi_sweep_kernel's row, into the other buffer
        const double *r = vec(P.v[0]), *z = vec(P.v[1]);
        double *z_out = vec(P.v[2]);
        SellArgs A = L.A;
        A.pack = L.pack_s, A.slice_off = L.off_s;
        for (int64_t s = wave_id; s < P.n_slices; s += n_waves) {
          const int64_t row = s * kWave + lane;
          const bool valid = row < P.n_rows;
          const double zi = valid ? co_load(z + row) : 0.0;
          const double ri = valid ? co_load(r + row) : 0.0;
          const double si = valid ? L.dinv[row] : 0.0;
          const double az = sell_row_apply<false, R, true>(A, s, lane, z, zi, L.alpha, L.beta);
          if (valid) co_publish(z_out + row, amg_jacobi_value(ri, az, si, P.a, zi), xchg, seen);
        }
      } break;
      case kTailTransfer: {  // y = T x / y += T x; kTailWithD0: and the next level's d_0 = a (s .* y), s of level P.level
        const double *x = vec(P.v[0]);
        double *y = vec(P.v[1]), *d0 = vec(P.v[2]);
        const bool add = (flags & kTailAdd) != 0;
        for (int64_t s = wave_id; s < P.n_slices; s += n_waves) {
          const int64_t row = s * kWave + lane;
          const bool valid = row < P.n_rows;
          const double yi = (add && valid) ? co_load(y + row) : 0.0;
          const double yn = add ? amg_transfer_row<true, true>(P.tpack, P.toff, s, lane, x, yi)
                                : amg_transfer_row<false, true>(P.tpack, P.toff, s, lane, x, yi);
          if (valid) {
            co_publish(y + row, yn, xchg, seen);
            if (flags & kTailWithD0) co_publish(d0 + row, cheb_d0_value<true>(P.a, yn, L.dinv[row]), xchg, seen);
          }
        }
      } break;
      default: {  // kTailCoarse: z = Ainv r, one wavefront per row
        const double *r = vec(P.v[0]);
        double *z = vec(P.v[1]);
        const double *ainv = reinterpret_cast<const double *>(P.tpack);
        for (int64_t row = wave_id; row < P.n_rows; row += n_waves) {
          const double acc = amg_coarse_row<true>(ainv, P.n_rows, row, lane, r);
          if (lane == 0) co_publish(z + row, acc, xchg, seen);
        }
      } break;
    }
    // what this phase stored is visible to every block behind the barrier (the last phase ends the kernel)
    if (p + 1 < a.n_phases) (void)lat_allreduce(0.0, a.slots, ++seq, lds, true, seen);
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
static bool tail_level_eligible(const storm_hip_amg *h, size_t l) {
  if (l + 1 == h->levels.size()) return true;  // the dense inverse
  if (l == 0 && h->nullspace) return false;    // its projections and the closing amg_axpy_mean stay launches
  const storm_hip_op *op = h->levels[l].op;
  if (!amg_residual_fused(h, op)) return false;
  if (h->hier->params.reduced_records != 0 && (op->d_pack32 == nullptr || op->d_slice_off32 == nullptr)) return false;
  return true;
}

int amg_tail_level(const storm_hip_amg *h) {
  const size_t nl = h->levels.size();
  size_t first_ok = nl;  // the first level from which every level is eligible
  for (size_t l = nl; l-- > 0;) {
    if (!tail_level_eligible(h, l)) break;
    first_ok = l;
  }
  for (size_t l = first_ok; l < nl; ++l)
    if (h->levels[l].n <= h->ctx->opt_amg_tail_rows) return (int)l;
  return -1;
}

int amg_tail_choose(const storm_hip_amg *h) {
  const storm_hip_ctx *c = h->ctx;
  if (c->opt_amg_tail == 0 || c->coop_disabled != 0 || c->comm != nullptr) return -1;
  const int t = amg_tail_level(h);
  return (t >= 0 && (size_t)t + 1 < h->levels.size()) ? t : -1;  // (the coarsest level alone is one launch already)
}

void amg_tail_invalidate(const storm_hip_amg *h) { h->tail.built_level = -1, h->tail.blocks = 0, h->tail.barriers = 0, h->tail.n_phases = 0; }

void amg_tail_free(storm_hip_amg *h) {
  if (h->tail.d_table) (void)hipFree(h->tail.d_table);
  h->tail.d_table = nullptr, h->tail.table_bytes = 0;
  amg_tail_invalidate(h);
}

constexpr int kTailVecsPerLevel = 7;  // r, z, t, e, the Chebyshev smoother's d[0], d[1], res
enum : int { kVr = 0, kVz, kVt, kVe, kVd0, kVd1, kVres };
static int tail_vec(size_t l, int which) { return 2 + (int)l * kTailVecsPerLevel + which; }

// The cycle from level l down and back as phases, in amg_cycle's / amg_cycle_jacobi's order.  r_id, z_id: the level's right-hand
// side and result; started: the smoother's start was merged into the phase that formed r.
static void tail_emit(const storm_hip_amg *h, size_t l, int r_id, int z_id, bool started, std::vector<AmgTailPhase> *out) {
  const size_t nl = h->levels.size();
  const storm_hip_amg::Level &L = h->levels[l];
  auto phase = [&](int kind, size_t level, int flags, double a, double b) {
    AmgTailPhase P;
    memset(&P, 0, sizeof P);
    P.kind = kind, P.level = (int)level, P.flags = flags, P.a = a, P.b = b;
    P.n_rows = h->levels[level].n, P.n_slices = (P.n_rows + kWave - 1) / kWave;
    for (int i = 0; i < 6; ++i) P.v[i] = 1;  // (an id the kernel can resolve; the phase's kind says which are read)
    return P;
  };
  if (l + 1 == nl) {
    AmgTailPhase P = phase(kTailCoarse, l, 0, 0.0, 0.0);
    P.v[0] = r_id, P.v[1] = z_id, P.tpack = reinterpret_cast<const char *>(h->d_ainv), P.n_rows = h->n_coarse;
    out->push_back(P);
    return;
  }
  const storm_hip_amg::Level &N = h->levels[l + 1];
  const bool jacobi = h->smoother_kind == 1;
  const bool next_smooths = l + 2 < nl;
  // the restriction, with the next level's start merged; the recursion; the prolongation into `into`
  auto down_and_up = [&](int into) {
    AmgTailPhase T = phase(kTailTransfer, l + 1, next_smooths ? kTailWithD0 : 0, 0.0, 0.0);
    T.v[0] = tail_vec(l, kVt), T.v[1] = tail_vec(l + 1, kVr), T.tpack = L.R.d_pack, T.toff = L.R.d_off;
    T.n_rows = L.R.n_rows, T.n_slices = L.R.n_slices;
    if (next_smooths) T.a = jacobi ? N.sigma : N.cheb->inv_theta, T.v[2] = tail_vec(l + 1, jacobi ? kVe : kVd0);
    out->push_back(T);
    tail_emit(h, l + 1, tail_vec(l + 1, kVr), tail_vec(l + 1, kVz), next_smooths, out);
    AmgTailPhase U = phase(kTailTransfer, l, kTailAdd, 0.0, 0.0);
    U.v[0] = tail_vec(l + 1, kVz), U.v[1] = into, U.tpack = L.P.d_pack, U.toff = L.P.d_off;
    U.n_rows = L.P.n_rows, U.n_slices = L.P.n_slices;
    out->push_back(U);
  };
  auto residual = [&](int zin, int flags, double a, int d0) {
    AmgTailPhase P = phase(kTailResidual, l, flags, a, 0.0);
    P.v[0] = r_id, P.v[1] = zin, P.v[2] = tail_vec(l, kVt), P.v[3] = d0;
    out->push_back(P);
  };
  if (jacobi) {  // (amg_cycle_jacobi: the iterate alternates between z and e)
    const int nu = h->jacobi_sweeps;
    const int buf[2] = {z_id, tail_vec(l, kVe)};
    int at = 1;
    if (!started) {
      AmgTailPhase P = phase(kTailD0, l, 0, L.sigma, 0.0);
      P.v[0] = r_id, P.v[1] = buf[at];
      out->push_back(P);
    }
    auto sweep = [&]() {
      AmgTailPhase P = phase(kTailSweep, l, 0, L.sigma, 0.0);
      P.v[0] = r_id, P.v[1] = buf[at], P.v[2] = buf[at ^ 1];
      out->push_back(P);
      at ^= 1;
    };
    for (int k = 1; k < nu; ++k) sweep();
    residual(buf[at], 0, 0.0, 1);
    down_and_up(buf[at]);
    for (int k = 0; k < nu; ++k) sweep();
    return;  // (at == 0: the last sweep stored into z)
  }
  const storm_hip_cheb *ch = L.cheb;
  const int d[2] = {tail_vec(l, kVd0), tail_vec(l, kVd1)}, res = tail_vec(l, kVres);
  // storm_hip_cheb_apply(rhs, zout) behind its start; axpy_into >= 0: the closing z = z + e merged into the last step
  auto smooth = [&](int rhs, int zout, int axpy_into) {
    for (int k = 0; k < ch->degree; ++k) {
      const bool first = k == 0, last = k == ch->degree - 1;
      AmgTailPhase P = phase(kTailStep, l, (first ? kTailFirst : 0) | (last ? kTailLast : 0) | ((last && axpy_into >= 0) ? kTailAxpy : 0),
                             ch->c1[k], ch->c2[k]);
      P.v[0] = d[k & 1], P.v[1] = first ? rhs : res, P.v[2] = zout, P.v[3] = d[(k + 1) & 1], P.v[4] = res;
      P.v[5] = axpy_into >= 0 ? axpy_into : zout;
      out->push_back(P);
    }
  };
  if (!started) {
    AmgTailPhase P = phase(kTailD0, l, 0, ch->inv_theta, 0.0);
    P.v[0] = r_id, P.v[1] = d[0];
    out->push_back(P);
  }
  smooth(r_id, z_id, -1);
  residual(z_id, 0, 0.0, 1);
  down_and_up(z_id);
  residual(z_id, kTailWithD0, ch->inv_theta, d[0]);
  smooth(tail_vec(l, kVt), tail_vec(l, kVe), z_id);
}

// The tables of a tail that starts at level t, on the device (the stream is drained first: an earlier launch may read them).
static int amg_tail_build(const storm_hip_amg *h, int t) {
  storm_hip_ctx *c = h->ctx;
  storm_hip_amg::Tail &T = h->tail;
  const size_t nl = h->levels.size();
  const bool reduced = h->hier->params.reduced_records != 0;
  std::vector<AmgTailLevel> levels(nl);
  std::vector<double *> vecs(2 + nl * kTailVecsPerLevel, nullptr);
  int64_t max_slices = 1;
  for (size_t l = 0; l < nl; ++l) {
    const storm_hip_amg::Level &L = h->levels[l];
    AmgTailLevel &D = levels[l];
    memset(&D, 0, sizeof D);
    auto put = [&](int which, const storm_hip_vec *v) { vecs[(size_t)tail_vec(l, which)] = v ? v->d : nullptr; };
    put(kVr, L.r), put(kVz, L.z), put(kVt, L.t), put(kVe, L.e);
    if (L.cheb) put(kVd0, L.cheb->d[0]), put(kVd1, L.cheb->d[1]), put(kVres, L.cheb->res);
    if (l + 1 == nl || (int)l < t) continue;
    const storm_hip_op *op = L.op;
    D.A = SellArgs{op->d_pack, op->d_slice_off, op->n_rows, op->uniform_width, 0, nullptr, 0, nullptr, 0, 0};
    D.pack_s = reduced ? op->d_pack32 : op->d_pack, D.off_s = reduced ? op->d_slice_off32 : op->d_slice_off;
    D.alpha = L.alpha, D.beta = L.beta, D.dinv = L.dinv->d, D.n_slices = op->n_slices;
    max_slices = std::max(max_slices, (int64_t)op->n_slices);
  }
  std::vector<AmgTailPhase> phases;
  tail_emit(h, (size_t)t, 0, 1, false, &phases);
  const size_t lb = sizeof(AmgTailLevel) * nl, pb = sizeof(AmgTailPhase) * phases.size(), vb = sizeof(double *) * vecs.size();
  std::vector<char> image(lb + pb + vb);
  memcpy(image.data(), levels.data(), lb);
  memcpy(image.data() + lb, phases.data(), pb);
  memcpy(image.data() + lb + pb, vecs.data(), vb);
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (image.size() > T.table_bytes) {
    if (T.d_table) (void)hipFree(T.d_table);
    T.d_table = nullptr, T.table_bytes = 0;
    HIP_TRY(hipMalloc((void **)&T.d_table, image.size()));
    T.table_bytes = image.size();
  }
  HIP_TRY(hipMemcpy(T.d_table, image.data(), image.size(), hipMemcpyHostToDevice));
  T.n_phases = (int)phases.size(), T.barriers = T.n_phases - 1;
  const int64_t want = (max_slices + kLatWaves - 1) / kLatWaves;
  T.blocks = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(256, c->num_cus), want));
  T.built_level = t, T.top_pack32 = h->levels[(size_t)t].op->d_pack32;
  return STORM_HIP_OK;
}

int amg_tail_run(const storm_hip_amg *h, size_t l, const storm_hip_vec *r, storm_hip_vec *z, bool *taken) {
  *taken = false;
  storm_hip_ctx *c = h->ctx;
  storm_hip_amg::Tail &T = h->tail;
  if (T.built_level != (int)l || T.top_pack32 != h->levels[l].op->d_pack32) STORM_TRY(amg_tail_build(h, (int)l));
  const bool reduced = h->hier->params.reduced_records != 0;
  const void *fn = reduced ? (const void *)amg_tail_kernel<Rec32> : (const void *)amg_tail_kernel<Rec64>;
  if (occupancy_cached(c, fn, kLatBlock, 0) < 1) {
    ++c->n_amg_tail_refusals;
    return STORM_HIP_OK;
  }
  const size_t nl = h->levels.size();
  AmgTailArgs a;
  a.levels = reinterpret_cast<const AmgTailLevel *>(T.d_table);
  a.phases = reinterpret_cast<const AmgTailPhase *>(T.d_table + sizeof(AmgTailLevel) * nl);
  a.vecs = reinterpret_cast<double *const *>(T.d_table + sizeof(AmgTailLevel) * nl + sizeof(AmgTailPhase) * (size_t)T.n_phases);
  a.n_phases = T.n_phases, a.publish_xchg = (int)(c->opt_latency_publish != 0);
  a.r = r->d, a.z = z->d, a.slots = c->d_lat_slots, a.done = c->api_done;
  a.seq_base = (1ull << 31) | (c->lat_seq & 0x7fffffffull);  // bit 31: never the tag of a CG solve (those count from 1)
  c->lat_seq += (unsigned long long)T.barriers;
  void *args[] = {&a};
  *taken = coop_launch(c, fn, (unsigned)T.blocks, args, 0, kLatBlock);
  if (!*taken) {
    c->lat_seq -= (unsigned long long)T.barriers;
    ++c->n_amg_tail_refusals;
    return STORM_HIP_OK;
  }
  ++c->n_amg_tail_applies;
  if (c->api_done == nullptr) c->amg_tail_unchecked = 1;  // outside a solve: storm_hip_ctx_sync reports a give-up
  return STORM_HIP_OK;
}

int amg_tail_get(const storm_hip_amg *h, const char *key, double *value, bool *known) {
  *known = true;
  const int t = amg_tail_level(h);
  const bool runs = t >= 0 && (size_t)t + 1 < h->levels.size();
  if (!strcmp(key, "tail_level")) *value = (double)t;
  else if (!strcmp(key, "tail_blocks") || !strcmp(key, "tail_barriers")) {
    if (runs && h->tail.built_level != t) STORM_TRY(amg_tail_build(h, t));
    *value = !runs ? 0.0 : key[5] == 'b' && key[6] == 'l' ? (double)h->tail.blocks : (double)h->tail.barriers;
  } else *known = false;
  return STORM_HIP_OK;
}

}  // namespace storm
