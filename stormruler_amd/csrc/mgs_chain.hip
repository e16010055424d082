// GMRES's modified Gram-Schmidt chain as ONE cooperative kernel per Arnoldi step: the register chain, the LDS-ring
// chain and the chain of four steps per synchronisation point (the default), each ending with the step's Givens
// rotations; gmres_mgs_chain_coop picks one and launches it.  The all-reduces are coop_device.hpp's; the launch and the
// give-up machinery coop_host.hip's.
#include <algorithm>
#include <cmath>

#include "common.hpp"
#include "coop_device.hpp"
#include "spmv_device.hpp"
#include "solver_device.hpp"

namespace storm {

// ---- modified Gram-Schmidt as ONE cooperative kernel -------------------------------------------------------------
// GMRES's Arnoldi step orthogonalises w = A q_k against q_0 .. q_k one after the other (SolverGmres.hpp:157-161); each
// step needs a global reduction before the next may start.  The throughput path runs a kernel per step that reads w,
// q_i and q_{i+1} and writes w (32 B/row/step, 13 us at 128^3: launch + HBM).  Here every wavefront keeps ITS rows of w
// in registers for the whole chain, streams the rows of q_i through once (prefetching q_{i+1} while the all-reduce of
// step i is in flight), and the k + 2 reductions are the tagged-slot all-reduces of the latency path: 8 B/row/step and
// ~3 us per step.  Same values in the same order (h_i = <w, q_i> with the updated w; w -= h_i q_i), the reduction
// trees differ in rounding only.  Finishes with h_{k+1,k}^2 = <w, w> and (optionally) q_{k+1} = w / sqrt of it.
constexpr int kMgsMaxVectors = 64;
struct MgsArgs {
  const double *q[kMgsMaxVectors];
  double *w;          // in: A q_k; out: q_{k+1} (normalised when `normalise`)
  double *H;          // column k of the (m + 1) x m row-major Hessenberg: H[i * m + k]
  double *norm2_out;  // <w, w> after the chain
  int64_t n_rows, n_slices;
  int k, m, normalise;
  int pairs;          // two Gram-Schmidt steps per synchronisation point (see the kernel)
  unsigned long long seq_base;  // tags of this launch: seq_base + 1 .. seq_base + k + 2 (bit 31 set: never a CG tag)
  char *slots;
  const int *done;
  MgsGivens givens;  // st == nullptr: the caller applies the rotations
  long long *prof;   // option resident_profile: [gridDim.x][8] ticks per phase of this launch (diagnostic)
  char *quad_slots;  // mgs_chain_quad_kernel: all-reduce slots of kQuadSlotStride bytes (two-level form) / dense granules
  int dense;         // ... the flat all-reduce with dense value-major slots instead of the two-level one: always 1 (the A/B is decided;
                     // the argument stays because without it mgs_chain_quad_kernel<4, 3> is allocated 238 / 222 VGPRs instead of 211 / 196)
  int prefetch;      // ... with the next group's vectors requested between its halves (S <= 4)
  int xcd_runs;      // ... and the blocks' chunks of rows dealt out in ONE contiguous run per XCD (see the kernel)
  int descend;       // ... the basis vectors taken in the order k, k - 1, ..., 0 (odd k: see the kernel)
  int rotate_early;  // ... the k earlier rotations of the column under the norm's all-reduce (block 0)
  // mgs_chain_quad_kernel<S, T, true>: w is not read but FORMED -- w = beta x + alpha M(x), x = ap_x (the newest basis
  // vector), from the operator's format-4 records with spmv_canon_kernel's arithmetic (the same bits): the apply's
  // launch and the round trip of w through memory disappear (SolverGmres.hpp:155 inside the kernel that consumes it)
  const char *ap_pack;
  const double *ap_dict, *ap_x;
  int ap_off[6], ap_max_gather;
  double ap_alpha, ap_beta;
};
// The end of an Arnoldi step, SolverGmres.hpp:161, :176-191 and Solver.hpp:132-140, by the thread of block 0 that holds
// column k of the Hessenberg: the arithmetic of gmres_givens_update (solver_device.hpp) on the LDS copies -- a chain of k
// dependent steps, ~1.5 us from LDS, ~9 us through memory (cs_sh / sn_sh are filled before the block's first barrier).
// The k earlier rotations on the column ...
__device__ __forceinline__ void mgs_rotate_earlier(double *hcol, const double *cs_sh, const double *sn_sh, int k) {
  for (int i = 0; i < k; ++i) {
    const double chi = cs_sh[i] * hcol[i] + sn_sh[i] * hcol[i + 1];
    hcol[i + 1] = -sn_sh[i] * hcol[i] + cs_sh[i] * hcol[i + 1];
    hcol[i] = chi;
  }
}
// ... and the tail: hn = h_{k+1,k} joins the column, the earlier rotations unless `rotated` already, the new rotation,
// column k of H, cs, sn and beta written back, the solver's state advanced.
__device__ __forceinline__ void mgs_rotation_tail(const MgsGivens gv, const int k, const int m, double hn, double *hcol, const double *cs_sh, const double *sn_sh,
                                                  bool rotated) {
  *gv.hn_slot = hn;
  hcol[k + 1] = hn;
  if (!rotated) mgs_rotate_earlier(hcol, cs_sh, sn_sh, k);
  const double ha = hcol[k], hb = hcol[k + 1];
  const double rr = hypot(ha, hb);
  double cs, sn;
  if (rr > 0.0) cs = ha / rr, sn = hb / rr;
  else cs = 1.0, sn = 0.0;
  gv.cs[k] = cs, gv.sn[k] = sn;
  hcol[k] = cs * ha + sn * hb;
  hcol[k + 1] = 0.0;
  for (int i = 0; i <= k + 1; ++i) gv.H[(int64_t)i * m + k] = hcol[i];
  const double bk = gv.beta[k];
  gv.beta[k + 1] = -sn * bk;
  gv.beta[k] = bk * cs;
  advance(gv.st, fabs(-sn * bk));
}
template <int S>
__global__ __launch_bounds__(kLatBlock) void mgs_chain_kernel(MgsArgs a) {
  if (a.done && *a.done) return;  // (uniform: every block reads the same flag before any of them synchronises)
  __shared__ double lds[3 * kLatWaves];
  // block 0 keeps column k of the Hessenberg and the earlier rotations in LDS (mgs_rotation_tail)
  __shared__ double hcol[kMgsMaxVectors + 1], cs_sh[kMgsMaxVectors], sn_sh[kMgsMaxVectors];
  const bool rotate = a.givens.st != nullptr && blockIdx.x == 0;
  if (rotate && (int)threadIdx.x < a.k) cs_sh[threadIdx.x] = a.givens.cs[threadIdx.x], sn_sh[threadIdx.x] = a.givens.sn[threadIdx.x];
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave_id = (int64_t)blockIdx.x * kLatWaves + (threadIdx.x >> 6);
  const int64_t n_waves = (int64_t)gridDim.x * kLatWaves;
  unsigned long long seq = a.seq_base;
  double w[S], qc[S], qn[S];
  int row[S];  // (-1: no such row; the chain takes at most 2^22 rows)
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int64_t sl = wave_id + s * n_waves;
    row[s] = (sl < a.n_slices && sl * kWave + lane < a.n_rows) ? (int)(sl * kWave + lane) : -1;
    w[s] = row[s] >= 0 ? a.w[row[s]] : 0.0;
    qc[s] = row[s] >= 0 ? a.q[0][row[s]] : 0.0;
    qn[s] = 0.0;
  }
  int i0 = 0;
  if constexpr (S <= 8) if (a.pairs) {  // (16 slices per wavefront leave no registers for the pair's vectors)
    // Two steps per synchronisation point.  The reference's h_{i+1} = <w - h_i q_i, q_{i+1}> is, by bilinearity,
    // <w, q_{i+1}> - h_i <q_i, q_{i+1}>: the three dot products of the right-hand side need only the w BEFORE step i,
    // so they share one all-reduce (the same algorithm; the roundings of the dot products group differently, as
    // with any other summation order).  q_{i+2} travels while the reduction is in flight.
    // (both vectors of the NEXT pair travel while this pair's reduction is in flight: round 3 loaded the second one at
    //  the top of the next pass, 16.8 MB at 128^3 with nothing to hide behind -- 3.4 us per pair)
    double qd[S], qe[S];
    bool have_n = false;  // qn holds q_{i0+1} already
    for (; i0 + 1 <= a.k; i0 += 2) {
      if (!have_n) {
#pragma unroll
        for (int s = 0; s < S; ++s) qn[s] = row[s] >= 0 ? a.q[i0 + 1][row[s]] : 0.0;
      }
      double s0 = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll
      for (int s = 0; s < S; ++s) s0 += w[s] * qc[s], s1 += w[s] * qn[s], s2 += qc[s] * qn[s];
      if (i0 + 2 <= a.k) {
#pragma unroll
        for (int s = 0; s < S; ++s) qd[s] = row[s] >= 0 ? a.q[i0 + 2][row[s]] : 0.0;
      }
      const bool have_next = i0 + 3 <= a.k;
      if (have_next) {
#pragma unroll
        for (int s = 0; s < S; ++s) qe[s] = row[s] >= 0 ? a.q[i0 + 3][row[s]] : 0.0;
      }
      lat_allreduce3(s0, s1, s2, a.slots, ++seq, lds);
      const double h0 = s0, h1 = s1 - h0 * s2;
      if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (rotate) hcol[i0] = h0, hcol[i0 + 1] = h1;
        else a.H[(int64_t)i0 * a.m + a.k] = h0, a.H[(int64_t)(i0 + 1) * a.m + a.k] = h1;
      }
#pragma unroll
      for (int s = 0; s < S; ++s) {
        w[s] -= h0 * qc[s];
        w[s] -= h1 * qn[s];
        qc[s] = qd[s];
        if (have_next) qn[s] = qe[s];
      }
      have_n = have_next;
    }
  }
  for (int i = i0; i <= a.k; ++i) {
    double acc = 0.0;
#pragma unroll
    for (int s = 0; s < S; ++s) acc += w[s] * qc[s];
    if (i < a.k) {  // the next basis vector travels while the reduction is in flight
#pragma unroll
      for (int s = 0; s < S; ++s) qn[s] = row[s] >= 0 ? a.q[i + 1][row[s]] : 0.0;
    }
    const double h = lat_allreduce(acc, a.slots, ++seq, lds, false);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      if (rotate) hcol[i] = h;  // (written back rotated, below)
      else a.H[(int64_t)i * a.m + a.k] = h;
    }
#pragma unroll
    for (int s = 0; s < S; ++s) w[s] -= h * qc[s], qc[s] = qn[s];
  }
  double acc = 0.0;
#pragma unroll
  for (int s = 0; s < S; ++s) acc += w[s] * w[s];
  const double norm2 = lat_allreduce(acc, a.slots, ++seq, lds, false);
  if (blockIdx.x == 0 && threadIdx.x == 0) *a.norm2_out = norm2;
  const double hn = sqrt(norm2);
#pragma unroll
  for (int s = 0; s < S; ++s)
    if (row[s] >= 0) a.w[row[s]] = a.normalise ? w[s] / hn : w[s];
  if (rotate && threadIdx.x == 0) mgs_rotation_tail(a.givens, a.k, a.m, hn, hcol, cs_sh, sn_sh, false);
}

// ---- ... with the basis vectors landing in LDS (round 4) ----------------------------------------------------------
// The chain above is bound by what it can keep in flight: w and the current pair of basis vectors fill the registers, so
// the next vectors' rows are requested only when a register array is free again and the HBM stream stops at every
// all-reduce (GMRES(30) at 128^3: 2.8 TB/s over the chain).  Here the NEXT pair of basis vectors is fetched by LDS-DMA
// (`global_load_lds_dwordx4`: no register destination) into a two-slot ring of the block's rows, 2 x SUB x 16 KiB,
// issued the moment the current pair has been read out of the ring: the stream runs through the reduction and the
// update of w.  A thread reads back exactly the 16 bytes its own DMA wrote (the ring is a per-thread landing zone, no
// barrier), behind `s_waitcnt vmcnt(0)`.  Rows of a block: [blockIdx * SUB * 2048, ...), pair 2 t + j * 2048 of thread t.
// Same steps, same values in the same order as the paired chain above; the block partials group the rows differently.
constexpr int kMgsSub = 2 * kLatBlock;  // rows per sub-chunk: one pair per thread
typedef double double2m __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void glds16(const void *gsrc, unsigned lds_dst /* wave-uniform byte address */) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(gsrc), "s"(lds_dst)
               : "memory");
}
template <int SUB>
__global__ __launch_bounds__(kLatBlock) void mgs_chain_lds_kernel(MgsArgs a) {
  if (a.done && *a.done) return;  // (uniform: every block reads the same flag before any of them synchronises)
  extern __shared__ __attribute__((aligned(16))) double ring[];  // [2][SUB * kMgsSub]
  __shared__ double lds[3 * kLatWaves];
  __shared__ double hcol[kMgsMaxVectors + 1], cs_sh[kMgsMaxVectors], sn_sh[kMgsMaxVectors];
  const bool rotate = a.givens.st != nullptr && blockIdx.x == 0;
  if (rotate && (int)threadIdx.x < a.k) cs_sh[threadIdx.x] = a.givens.cs[threadIdx.x], sn_sh[threadIdx.x] = a.givens.sn[threadIdx.x];
  const int tid = threadIdx.x, wave = tid >> 6;
  unsigned long long seq = a.seq_base;
  const int64_t chunk0 = (int64_t)blockIdx.x * SUB * kMgsSub;
  int64_t row[SUB];
  bool va[SUB], vb[SUB];
  double2m w[SUB];
#pragma unroll
  for (int j = 0; j < SUB; ++j) {
    row[j] = chunk0 + (int64_t)j * kMgsSub + 2 * tid;
    va[j] = row[j] < a.n_rows, vb[j] = row[j] + 1 < a.n_rows;
    w[j] = double2m{0.0, 0.0};
    if (vb[j]) w[j] = *reinterpret_cast<const double2m *>(a.w + row[j]);
    else if (va[j]) w[j].x = a.w[row[j]];
  }
  const unsigned ring_base = (unsigned)(size_t)(__attribute__((address_space(3))) void *)ring;  // the ring's LDS byte address
  // this block's rows of basis vector q into a slot of the ring (rows past the end: any valid address, masked below)
  auto issue = [&](int slot, const double *q) {
#pragma unroll
    for (int j = 0; j < SUB; ++j) {
      const unsigned dst = __builtin_amdgcn_readfirstlane(ring_base + (unsigned)(((slot * SUB + j) * kMgsSub + wave * 2 * kWave) * 8));
      glds16(q + (va[j] ? row[j] : 0), dst);
    }
  };
  auto take = [&](int slot, double2m (&v)[SUB]) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this thread's DMAs have landed
#pragma unroll
    for (int j = 0; j < SUB; ++j) {
      const double2m t = *reinterpret_cast<const double2m *>(&ring[(slot * SUB + j) * kMgsSub + 2 * tid]);
      v[j].x = va[j] ? t.x : 0.0, v[j].y = vb[j] ? t.y : 0.0;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // ... and are in registers: the slot may be refilled
  };
  long long tick[8] = {0, 0, 0, 0, 0, 0, 0, 0}, t_mark = a.prof ? wall_clock64() : 0;
  auto lap = [&](int p) {
    if (a.prof) {
      const long long now = wall_clock64();
      tick[p] += now - t_mark, t_mark = now;
    }
  };
  issue(0, a.q[0]);
  if (a.k >= 1) issue(1, a.q[1]);
  double2m qa[SUB], qb[SUB];
  int i = 0;
  for (; i + 1 <= a.k; i += 2) {
    lap(0);  // (the update of w, loop overhead)
    take(0, qa), take(1, qb);
    lap(1);  // waiting for the pair's rows
    // the next pair travels under the reduction and the update -- but for the waves that poll the other blocks' slots
    // (vector loads return in order: a poll behind a DMA would wait for it), which ask for theirs once they are through
    const bool polls = wave < 4;
    if (!polls) {
      if (i + 2 <= a.k) issue(0, a.q[i + 2]);
      if (i + 3 <= a.k) issue(1, a.q[i + 3]);
    }
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int j = 0; j < SUB; ++j) {
      s0 += w[j].x * qa[j].x, s1 += w[j].x * qb[j].x, s2 += qa[j].x * qb[j].x;
      s0 += w[j].y * qa[j].y, s1 += w[j].y * qb[j].y, s2 += qa[j].y * qb[j].y;
    }
    lap(2);  // DMA issue + dot products
    lat_allreduce3<true>(s0, s1, s2, a.slots, ++seq, lds);
    lap(3);  // the all-reduce
    if (polls) {
      if (i + 2 <= a.k) issue(0, a.q[i + 2]);
      if (i + 3 <= a.k) issue(1, a.q[i + 3]);
    }
    const double h0 = s0, h1 = s1 - h0 * s2;  // (mgs_chain_kernel: the reference's h_{i+1} by bilinearity)
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      if (rotate) hcol[i] = h0, hcol[i + 1] = h1;
      else a.H[(int64_t)i * a.m + a.k] = h0, a.H[(int64_t)(i + 1) * a.m + a.k] = h1;
    }
#pragma unroll
    for (int j = 0; j < SUB; ++j) {
      w[j].x -= h0 * qa[j].x, w[j].y -= h0 * qa[j].y;
      w[j].x -= h1 * qb[j].x, w[j].y -= h1 * qb[j].y;
    }
  }
  if (i <= a.k) {  // an odd vector is left: it sits in slot 0
    take(0, qa);
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < SUB; ++j) acc += w[j].x * qa[j].x, acc += w[j].y * qa[j].y;
    const double h = lat_allreduce(acc, a.slots, ++seq, lds, false);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      if (rotate) hcol[i] = h;
      else a.H[(int64_t)i * a.m + a.k] = h;
    }
#pragma unroll
    for (int j = 0; j < SUB; ++j) w[j].x -= h * qa[j].x, w[j].y -= h * qa[j].y;
  }
  double acc = 0.0;
#pragma unroll
  for (int j = 0; j < SUB; ++j) acc += w[j].x * w[j].x, acc += w[j].y * w[j].y;
  const double norm2 = lat_allreduce(acc, a.slots, ++seq, lds, false);
  if (blockIdx.x == 0 && threadIdx.x == 0) *a.norm2_out = norm2;
  const double hn = sqrt(norm2);
#pragma unroll
  for (int j = 0; j < SUB; ++j) {
    const double2m o = a.normalise ? double2m{w[j].x / hn, w[j].y / hn} : w[j];
    if (vb[j]) *reinterpret_cast<double2m *>(a.w + row[j]) = o;
    else if (va[j]) a.w[row[j]] = o.x;
  }
  lap(4);  // the tail: odd vector, norm, store
  if (a.prof && threadIdx.x == 0)
    for (int p = 0; p < 8; ++p) a.prof[blockIdx.x * 8 + p] = tick[p];
  if (rotate && threadIdx.x == 0) mgs_rotation_tail(a.givens, a.k, a.m, hn, hcol, cs_sh, sn_sh, false);
}

// ---- ... FOUR steps per synchronisation point (round 4) -----------------------------------------------------------
// Measured (option resident_profile, GMRES(30) at 128^3, the 30-vector chain): 134 of 167 us are the 15 all-reduces,
// 8.9 us each -- three times what the same all-reduce costs the resident CG kernel, because a poll queues behind the
// 33 MB of basis-vector rows the chain has just asked for (the ring above does not change that: the requests are FIFO).
// A chain is therefore (its bytes at the HBM rate) + (its synchronisation points x ~4.7 us), and what is left to take
// are the synchronisation points: FOUR Gram-Schmidt steps share one.  By bilinearity (as for the pairs above)
//   h_0 = <w, q_0>,   h_j = <w, q_j> - sum_{i < j} h_i <q_i, q_j>            (j = 1, 2, 3)
// are the reference's h_j = <w - h_0 q_0 - ... - h_{j-1} q_{j-1}, q_j> (SolverGmres.hpp:157-160); the ten dot products on
// the right need only the w before the group, and travel in one all-reduce.  Blocks of 512 threads (two wavefronts per
// SIMD: 256 registers per lane hold w and the group's four vectors of 2 S rows); the update w -= h_0 q_0; ... -= h_3 q_3
// runs in the reference's order.
constexpr int kQuadThreads = 512, kQuadWaves = kQuadThreads / kWave, kQuadSub = 2 * kQuadThreads;
constexpr int kQuadSlotStride = 256;  // ten values of 16 bytes
// LDSPF (S = 8, where no second set of vectors fits the registers): of the NEXT group's T vectors the first lands in
// registers and the others in LDS (LDS-DMA, 64 KiB per vector: `global_load_lds_dwordx4` has no register destination),
// all requested between the halves of the all-reduce; a thread reads back exactly the 16 bytes its own DMA wrote.
template <int S, int T, bool APPLY = false, bool LDSPF = false>  // T = 3 or 4 steps per synchronisation point
__global__ __launch_bounds__(kQuadThreads) void mgs_chain_quad_kernel(MgsArgs a) {
  if (a.done && *a.done) return;  // (uniform: every block reads the same flag before any of them synchronises)
  __shared__ double lds[10 * 256 + 16];  // co_allreduce_dense: NV x 256 polled values + the NV results
  __shared__ double dict_sh[32];
  extern __shared__ __attribute__((aligned(16))) double pf_ring[];  // LDSPF: [T - 1][S][kQuadSub] doubles
  __shared__ double hcol[kMgsMaxVectors + 1], cs_sh[kMgsMaxVectors], sn_sh[kMgsMaxVectors];
  const bool rotate = a.givens.st != nullptr && blockIdx.x == 0;
  if (rotate && (int)threadIdx.x < a.k) cs_sh[threadIdx.x] = a.givens.cs[threadIdx.x], sn_sh[threadIdx.x] = a.givens.sn[threadIdx.x];
  const int tid = threadIdx.x;
  unsigned long long seq = a.seq_base;
  int *gave_up = reinterpret_cast<int *>(a.slots + (size_t)2 * 256 * kLatSlotStride);  // (the latency path's flag)
  char *slots = a.quad_slots;
  // Which chunk of rows a block owns.  Blocks are dealt round-robin to the 8 XCDs (block b runs on XCD b % 8); with the
  // apply in the kernel a chunk's +-b neighbours (the planes below and above: two chunks away at 128^3) are gathered from
  // rows that OTHER blocks load as their own -- given to blocks of the same XCD (one contiguous run of chunks per XCD)
  // those gathers meet the owner's load in that XCD's L2 instead of fetching the line a second and third time.  The
  // all-reduce slots stay indexed by blockIdx.x: the same sums in another, equally fixed order.
  const int64_t chunk0 = (int64_t)(a.xcd_runs ? xcd_remap((int)blockIdx.x, (int)gridDim.x) : (int)blockIdx.x) * S * kQuadSub;
  unsigned off8[S];  // byte offset of the thread's pair j (rows < 2^22)
  bool va[S], vb[S];
  double2m w[S];
#pragma unroll
  for (int j = 0; j < S; ++j) {
    const int64_t row = chunk0 + (int64_t)j * kQuadSub + 2 * tid;
    va[j] = row < a.n_rows, vb[j] = row + 1 < a.n_rows;
    off8[j] = va[j] ? (unsigned)row << 3 : 0u;
    w[j] = double2m{0.0, 0.0};
    if (!APPLY && va[j]) w[j] = *reinterpret_cast<const double2m *>(reinterpret_cast<const char *>(a.w) + off8[j]);  // (>= 4 zero doubles behind the last row)
    w[j].y = vb[j] ? w[j].y : 0.0;
  }
  if constexpr (APPLY) {
    // w = beta x + alpha M(x) of the thread's row pairs: spmv_canon_kernel<false, 6, 2, false, G> (spmv_pair.hip) -- the
    // record word, the own pair, the four 16-byte gathers of offsets 0, 1, 4, 5, the +-1 neighbours from the adjacent
    // lanes (lanes 0 and 63 load theirs); two pairs' loads in flight at a time (registers)
    typedef unsigned long long u64x2m __attribute__((ext_vector_type(2)));
    const int lane = tid & (kWave - 1);
    if (lane < 32) dict_sh[lane] = a.ap_dict[lane];  // every wave stores the same words: no barrier (same-wave LDS order)
    __builtin_amdgcn_wave_barrier();
    const char *xb = reinterpret_cast<const char *>(a.ap_x);
    const char *xg_base = xb - (size_t)kVecGuard * 8;
    const double alpha = a.ap_alpha, beta = a.ap_beta;
    constexpr int JB = S >= 2 ? 2 : 1;  // (four pairs in flight at S = 8: 89.0 against 88.0 us per inner iteration at 128^3)
#pragma unroll
    for (int j0 = 0; j0 < S; j0 += JB) {
      u64x2m vw[JB];
      double2m xi[JB], xg[JB][6];
      double e[JB];
#pragma unroll
      for (int jj = 0; jj < JB; ++jj) {
        const unsigned rc = off8[j0 + jj] >> 3;  // (an absent pair re-reads pair 0: masked below)
        vw[jj] = __builtin_nontemporal_load(reinterpret_cast<const u64x2m *>(a.ap_pack + off8[j0 + jj]));
        xi[jj] = *reinterpret_cast<const double2m *>(xb + off8[j0 + jj]);
#pragma unroll
        for (int k = 0; k < 6; ++k) {
          if (k == 2 || k == 3) continue;
          int t = (int)rc + a.ap_off[k] + kVecGuard;  // guard-relative, clamped: an absent neighbour may point anywhere
          t = t < 0 ? 0 : t;
          t = t > a.ap_max_gather ? a.ap_max_gather : t;
          xg[jj][k] = *reinterpret_cast<const double2m *>(xg_base + (size_t)((unsigned)t << 3));
        }
        e[jj] = 0.0;
        if (lane == 0 || lane == kWave - 1)  // x[rc - 1] of lane 0, x[rc + 2] of lane 63
          e[jj] = *reinterpret_cast<const double *>(xg_base + (size_t)((rc + (unsigned)(kVecGuard + (lane == 0 ? -1 : 2))) << 3));
      }
#pragma unroll
      for (int jj = 0; jj < JB; ++jj) {
        const double left = dpp_shift<0x138>(xi[jj].y);   // wave_shr:1 -- lane i receives lane i - 1
        const double right = dpp_shift<0x130>(xi[jj].x);  // wave_shl:1 -- lane i receives lane i + 1
        xg[jj][2].x = lane == 0 ? e[jj] : left;
        xg[jj][2].y = xi[jj].x;
        xg[jj][3].x = xi[jj].y;
        xg[jj][3].y = lane == kWave - 1 ? e[jj] : right;
        double acc_a = 0.0, acc_b = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
          const unsigned ba = (unsigned)(vw[jj].x >> (8 * (k + 1))) & 0xffu, bb = (unsigned)(vw[jj].y >> (8 * (k + 1))) & 0xffu;
          acc_a += *reinterpret_cast<const double *>(reinterpret_cast<const char *>(dict_sh) + ba) * (xg[jj][k].x - xi[jj].x);
          acc_b += *reinterpret_cast<const double *>(reinterpret_cast<const char *>(dict_sh) + bb) * (xg[jj][k].y - xi[jj].y);
        }
        const double ext_a = *reinterpret_cast<const double *>(reinterpret_cast<const char *>(dict_sh) + ((unsigned)vw[jj].x & 0xffu));
        const double ext_b = *reinterpret_cast<const double *>(reinterpret_cast<const char *>(dict_sh) + ((unsigned)vw[jj].y & 0xffu));
        double2m yi;
        yi.x = __builtin_fma(alpha, __builtin_fma(ext_a, xi[jj].x, acc_a), beta * xi[jj].x);  // (spmv_canon_tile_kernel's form)
        yi.y = __builtin_fma(alpha, __builtin_fma(ext_b, xi[jj].y, acc_b), beta * xi[jj].y);
        w[j0 + jj].x = va[j0 + jj] ? yi.x : 0.0;
        w[j0 + jj].y = vb[j0 + jj] ? yi.y : 0.0;
        asm volatile("" : "+v"(w[j0 + jj].x), "+v"(w[j0 + jj].y));  // (the pair is finished HERE: nothing of it stays live)
      }
      // (group after group: with all S pairs' loads hoisted to the front the S = 8 kernel spilled 207 registers)
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  constexpr int ND = T == 4 ? 10 : 6;
  long long tick[8] = {0, 0, 0, 0, 0, 0, 0, 0}, t_mark = a.prof ? wall_clock64() : 0;
  auto lap = [&](int p) {
    if (a.prof) {
      const long long now = wall_clock64();
      tick[p] += now - t_mark, t_mark = now;
    }
  };
  // Where the registers allow it (S <= 4) the NEXT group's vectors are requested between the block's arrival at the
  // all-reduce and its wait for the others (co_allreduce_dense_arrive / _wait): their latency hides in the wait.
  constexpr bool kPrefetch = S <= 4;
  double2m qn[kPrefetch ? T : 1][(kPrefetch || LDSPF) ? S : 1];
  bool prefetched = false;
  const unsigned pf_base = LDSPF ? (unsigned)(size_t)(__attribute__((address_space(3))) void *)pf_ring : 0u;
  const int pf_wave = tid >> 6;
  // The ORDER in which w is orthogonalised against q_0 .. q_k alternates with k (round 6): ascending for even k, descending
  // for odd k.  A cycle's basis outgrows the 256 MB Infinity Cache from k = 15 on at 128^3 (16.8 MB per vector); read in the
  // same order every time, each vector has been evicted by the time it comes round again -- every read an HBM read.  Read
  // back and forth, an iteration starts with the vectors the previous one ended with: ~14 of them are still there.  The
  // reference's loop runs i = 0 .. k (SolverGmres.hpp:157-160); against an orthonormal basis the h_i of modified Gram-Schmidt
  // do not depend on the order but for their roundings (the fixed-K tests hold either order to 1e-10 / 1e-9), and the order
  // is a function of k alone: every run, every variant of this kernel takes the same one.
  const auto vidx = [&](int p) { return a.descend ? a.k - p : p; };  // position in the chain -> basis vector
  for (int i = 0; i <= a.k; i += T) {
    lap(0);  // the update of w
    double2m q[T][S];
    if (LDSPF && prefetched) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this thread's DMAs (and register loads) have landed
#pragma unroll
      for (int j = 0; j < S; ++j) q[0][j] = qn[0][LDSPF ? j : 0];
#pragma unroll
      for (int v = 1; v < T; ++v) {
        const bool have = i + v <= a.k;
#pragma unroll
        for (int j = 0; j < S; ++j) {
          const double2m t = *reinterpret_cast<const double2m *>(&pf_ring[((v - 1) * S + j) * kQuadSub + 2 * tid]);
          q[v][j].x = (have && va[j]) ? t.x : 0.0, q[v][j].y = (have && vb[j]) ? t.y : 0.0;
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // ... and are in registers: the landing zone may be refilled
    } else if (kPrefetch && prefetched) {
#pragma unroll
      for (int v = 0; v < T; ++v)
#pragma unroll
        for (int j = 0; j < S; ++j) q[v][j] = qn[kPrefetch ? v : 0][kPrefetch ? j : 0];
    } else {
#pragma unroll
      for (int v = 0; v < T; ++v) {
        const bool have = i + v <= a.k;  // (uniform; a vector past the end reads as zeros: its h comes out 0)
        const char *src = reinterpret_cast<const char *>(a.q[vidx(have ? i + v : i)]);
#pragma unroll
        for (int j = 0; j < S; ++j) {
          q[v][j] = double2m{0.0, 0.0};
          if (have && va[j]) q[v][j] = *reinterpret_cast<const double2m *>(src + off8[j]);
          q[v][j].y = vb[j] ? q[v][j].y : 0.0;
        }
      }
    }
    prefetched = false;
    // T = 4: <w,q0..3>, <q0,q1>, <q0,q2>, <q0,q3>, <q1,q2>, <q1,q3>, <q2,q3>;  T = 3: <w,q0..2>, <q0,q1>, <q0,q2>, <q1,q2>
    double d[ND];
#pragma unroll
    for (int e = 0; e < ND; ++e) d[e] = 0.0;
#pragma unroll
    for (int j = 0; j < S; ++j) {
#pragma unroll
      for (int v = 0; v < T; ++v) d[v] += w[j].x * q[v][j].x, d[v] += w[j].y * q[v][j].y;
      int e = T;
#pragma unroll
      for (int u = 0; u < T; ++u)
#pragma unroll
        for (int v = u + 1; v < T; ++v, ++e) d[e] += q[u][j].x * q[v][j].x, d[e] += q[u][j].y * q[v][j].y;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (a.prof) __syncthreads();  // (diagnostic: the whole block's rows have landed)
    lap(1);  // the group's rows (issue -> landed) and the dot products
    if (a.dense && (kPrefetch || LDSPF) && a.prefetch != 0) {
      ++seq;
      co_allreduce_dense_arrive<ND, kQuadWaves>(d, slots, seq, lds);
      if (i + T <= a.k) {
        if constexpr (LDSPF) {
          {  // the group's first vector: registers
            const char *src = reinterpret_cast<const char *>(a.q[vidx(i + T)]);
#pragma unroll
            for (int j = 0; j < S; ++j) {
              qn[0][j] = double2m{0.0, 0.0};
              if (va[j]) qn[0][j] = *reinterpret_cast<const double2m *>(src + off8[j]);
              qn[0][j].y = vb[j] ? qn[0][j].y : 0.0;
            }
          }
#pragma unroll
          for (int v = 1; v < T; ++v) {  // the others: LDS-DMA (rows past the end: any valid address, masked when read back)
            if (i + T + v <= a.k) {
              const char *src = reinterpret_cast<const char *>(a.q[vidx(i + T + v)]);
#pragma unroll
              for (int j = 0; j < S; ++j) {
                const unsigned dst = __builtin_amdgcn_readfirstlane(pf_base + (unsigned)((((v - 1) * S + j) * kQuadSub + pf_wave * 2 * kWave) * 8));
                glds16(src + off8[j], dst);
              }
            }
          }
        }
        if constexpr (kPrefetch) {
#pragma unroll
          for (int v = 0; v < T; ++v) {
            const bool have = i + T + v <= a.k;
            const char *src = reinterpret_cast<const char *>(a.q[vidx(have ? i + T + v : i + T)]);
#pragma unroll
            for (int j = 0; j < S; ++j) {
              qn[v][j] = double2m{0.0, 0.0};
              if (have && va[j]) qn[v][j] = *reinterpret_cast<const double2m *>(src + off8[j]);
              qn[v][j].y = vb[j] ? qn[v][j].y : 0.0;
            }
          }
        }
        prefetched = true;
      }
      co_allreduce_dense_wait<ND, kQuadWaves>(d, slots, gave_up, seq, lds);
    } else if (a.dense) {
      co_allreduce_dense<ND, kQuadWaves>(d, slots, gave_up, ++seq, lds);
    } else {
      co_allreduce2_n<ND, kQuadWaves>(d, slots, kQuadSlotStride, gave_up, ++seq, lds);
    }
    lap(2);  // the all-reduce
    double h[T];
    {
      int e = T;  // h_v = <w, q_v> - sum_{u < v} h_u <q_u, q_v>, the pairs (u, v) in the order they were summed
      double g[T][T];
#pragma unroll
      for (int u = 0; u < T; ++u)
#pragma unroll
        for (int v = u + 1; v < T; ++v, ++e) g[u][v] = d[e];
#pragma unroll
      for (int v = 0; v < T; ++v) {
        h[v] = d[v];
#pragma unroll
        for (int u = 0; u < v; ++u) h[v] -= h[u] * g[u][v];
      }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      for (int v = 0; v < T && i + v <= a.k; ++v) {
        if (rotate) hcol[vidx(i + v)] = h[v];
        else a.H[(int64_t)vidx(i + v) * a.m + a.k] = h[v];
      }
    }
#pragma unroll
    for (int j = 0; j < S; ++j) {
#pragma unroll
      for (int v = 0; v < T; ++v) w[j].x -= h[v] * q[v][j].x, w[j].y -= h[v] * q[v][j].y;
    }
  }
  double acc[1] = {0.0};
#pragma unroll
  for (int j = 0; j < S; ++j) acc[0] += w[j].x * w[j].x, acc[0] += w[j].y * w[j].y;
  bool rotated = false;
  if (a.dense && a.rotate_early != 0) {
    // The k earlier rotations of column k (SolverGmres.hpp:176-180) need every h of the chain and not the norm: block 0's
    // first thread applies them between the block's arrival at the norm's all-reduce and its wait for the others -- ~1.5 us
    // of a dependent chain through LDS that used to run after everything else, with the whole chip waiting for the kernel
    // to end.
    ++seq;
    co_allreduce_dense_arrive<1, kQuadWaves>(acc, slots, seq, lds);
    if (rotate && threadIdx.x == 0) {
      mgs_rotate_earlier(hcol, cs_sh, sn_sh, a.k);
      rotated = true;
    }
    co_allreduce_dense_wait<1, kQuadWaves>(acc, slots, gave_up, seq, lds);
  } else if (a.dense) {
    co_allreduce_dense<1, kQuadWaves>(acc, slots, gave_up, ++seq, lds);
  } else {
    co_allreduce2_n<1, kQuadWaves>(acc, slots, kQuadSlotStride, gave_up, ++seq, lds);
  }
  const double norm2 = acc[0];
  if (blockIdx.x == 0 && threadIdx.x == 0) *a.norm2_out = norm2;
  const double hn = sqrt(norm2);
#pragma unroll
  for (int j = 0; j < S; ++j) {
    const double2m o = a.normalise ? double2m{w[j].x / hn, w[j].y / hn} : w[j];
    if (vb[j]) *reinterpret_cast<double2m *>(reinterpret_cast<char *>(a.w) + off8[j]) = o;
    else if (va[j]) *reinterpret_cast<double *>(reinterpret_cast<char *>(a.w) + off8[j]) = o.x;
  }
  lap(3);  // the tail
  if (a.prof && threadIdx.x == 0)
    for (int p = 0; p < 8; ++p) a.prof[blockIdx.x * 8 + p] = tick[p];
  if (rotate && threadIdx.x == 0) mgs_rotation_tail(a.givens, a.k, a.m, hn, hcol, cs_sh, sn_sh, rotated);
}

// Which chain kernel takes a step of n rows, and how it is launched (fn == nullptr: none).
// (a step of the chain costs half an all-reduce, ~2.5 us, whatever the size; the kernel-per-step path costs a launch,
//  ~3.5 us, or 32 B/row of HBM traffic, whichever is more -- measured, us per inner iteration, per-step vs chained:
//  step.1 83..106 vs 74.5, 32^3 84..109 vs 72, 64^3 91..106 vs 93, 128^3 248 vs 147;
//  GMRES(30) us per inner iteration, register pairs / LDS ring / triples with the two-level all-reduce:
//  32^3 43.0 / 43.5 / 48.3, 64^3 60.5 / 51.1 / 55.2, 128^3 104.5 / 106.3 / 100.0 -- profiles/r04p_gmres_chain_ab.jsonl; with the
//  dense flat all-reduce the triples / quadruples take 38.9 / 52.6 / 97.2 and are the default wherever they fit;
//  options coop_mgs_quad: 0 off, else on; coop_mgs_lds: 0 never, 1 where the quadruples are off, 2 always)
struct MgsChoice {
  const void *fn = nullptr;
  unsigned threads = kLatBlock;
  int64_t blocks = 0;
  size_t dyn_lds = 0;
  bool quad = false;        // mgs_chain_quad_kernel: its slots, its step counter
  bool lds = false;         // mgs_chain_lds_kernel: its step counter
  bool with_apply = false;  // ... which forms w = beta x + alpha M(x) itself
  bool laps = false;        // the kernel records its phases (option resident_profile): every one but the register chain
  int pairs = 0;            // the register chain: two steps per synchronisation point
};
static MgsChoice mgs_choose(storm_hip_ctx *c, int64_t n, const double *qk, const ChainApply *apply, bool may_apply) {
  MgsChoice ch;
  const int cus = std::min(c->num_cus, 256);
  const int64_t n_slices = (n + kWave - 1) / kWave;
  const int64_t reg_blocks = std::max<int64_t>(1, std::min<int64_t>(cus, (n_slices + kLatWaves - 1) / kLatWaves));
  const int64_t need = (n_slices + reg_blocks * kLatWaves - 1) / (reg_blocks * kLatWaves);  // slices per wavefront
  ch.pairs = need <= 8 ? 1 : 0;  // (16 slices per wave + a third basis vector: spills)
  // four steps per synchronisation point (blocks of 512 threads, <= 8 pairs of rows per thread): the default
  const int64_t qsubs_total = (n + kQuadSub - 1) / kQuadSub;
  const int qsub = (int)((qsubs_total + cus - 1) / cus);
  if (c->opt_coop_mgs_quad != 0 && qsub >= 1 && qsub <= 8) {
    const int sv = qsub <= 1 ? 1 : qsub <= 2 ? 2 : qsub <= 4 ? 4 : 8;
    // (eight or sixteen rows per thread and FOUR vectors of them do not fit 256 registers beside the all-reduce: three there)
    // the operator applied inside the kernel: format-4 records with the six common offsets of a 3-D lattice numbering,
    // the dictionary within 32 values, no halo, no tail -- and the caller wanting the newest basis vector applied to
    const storm_hip_op *aop = apply ? apply->op : nullptr;
    const bool with_apply = aop != nullptr && may_apply && c->opt_coop_mgs_apply != 0 && aop->pair == 2 && aop->canon_k == 6 &&
                            aop->canon_m1 == 2 && aop->n_halo == 0 && aop->tail_rows == 0 && aop->d_bnd_pack == nullptr &&
                            aop->dict_size <= 32 && aop->n_rows == n && apply->x == qk;
    const void *qf = sv == 1 ? (const void *)mgs_chain_quad_kernel<1, 4> : sv == 2 ? (const void *)mgs_chain_quad_kernel<2, 4>
                   : sv == 4 ? (const void *)mgs_chain_quad_kernel<4, 3> : (const void *)mgs_chain_quad_kernel<8, 3>;
    if (with_apply)
      qf = sv == 1 ? (const void *)mgs_chain_quad_kernel<1, 4, true> : sv == 2 ? (const void *)mgs_chain_quad_kernel<2, 4, true>
         : sv == 4 ? (const void *)mgs_chain_quad_kernel<4, 3, true> : (const void *)mgs_chain_quad_kernel<8, 3, true>;
    // eight row pairs per thread: the next group's vectors through LDS (mgs_chain_quad_kernel<8, 3, APPLY, true>)
    size_t quad_lds = 0;
    // (with the apply only: the kernel that reads w instead has no registers left for the first vector -- 65 spills)
    if (sv == 8 && with_apply && c->opt_coop_mgs_prefetch != 0 && c->opt_coop_mgs_lds_prefetch != 0) {
      qf = (const void *)mgs_chain_quad_kernel<8, 3, true, true>;
      quad_lds = sizeof(double) * 2 * 8 * (size_t)kQuadSub;
    }
    if (occupancy_cached(c, qf, kQuadThreads, quad_lds) >= 1) {
      ch.fn = qf, ch.threads = kQuadThreads, ch.blocks = (qsubs_total + sv - 1) / sv, ch.dyn_lds = quad_lds;
      ch.quad = ch.laps = true, ch.with_apply = with_apply;
      return ch;
    }
  }
  // the LDS-ring chain: two steps per synchronisation point, <= 4 sub-chunks of 2048 rows per block (2 x 64 KiB of ring)
  const int64_t subs_total = (n + kMgsSub - 1) / kMgsSub;
  const int sub = (int)((subs_total + cus - 1) / cus);
  if ((c->opt_coop_mgs_lds == 2 || (c->opt_coop_mgs_lds == 1 && c->opt_coop_mgs_quad == 0 && n >= ((int64_t)1 << 17))) && sub >= 1 &&
      sub <= 4) {
    const int sv = sub <= 1 ? 1 : sub <= 2 ? 2 : 4;
    const void *lf = sv == 1 ? (const void *)mgs_chain_lds_kernel<1> : sv == 2 ? (const void *)mgs_chain_lds_kernel<2> : (const void *)mgs_chain_lds_kernel<4>;
    const size_t ring = sizeof(double) * 2 * (size_t)sv * kMgsSub;
    if (occupancy_cached(c, lf, kLatBlock, ring) >= 1) {
      ch.fn = lf, ch.blocks = (subs_total + sv - 1) / sv, ch.dyn_lds = ring, ch.laps = ch.lds = true;
      return ch;
    }
  }
  // the register chain (more than 16 slices per wavefront: registers cannot hold w)
  const void *rf = need <= 1    ? (const void *)mgs_chain_kernel<1>
                   : need <= 2  ? (const void *)mgs_chain_kernel<2>
                   : need <= 4  ? (const void *)mgs_chain_kernel<4>
                   : need <= 8  ? (const void *)mgs_chain_kernel<8>
                   : need <= 16 ? (const void *)mgs_chain_kernel<16>
                                : nullptr;
  if (rf != nullptr && occupancy_cached(c, rf, kLatBlock, 0) >= 1) ch.fn = rf, ch.blocks = reg_blocks;
  return ch;
}

// Returns STORM_HIP_OK with *taken = false when the chain does not qualify (too many rows / vectors, a communicator).
// apply (nullable): w has not been formed yet, w = beta x + alpha M(x) with x = q[k] (ChainApply, common.hpp): the quad
// kernels do it themselves, in front of any other variant it is launched here; *applied tells whether w exists when this
// returns -- if not (the chain did not qualify or could not be launched) the caller applies the operator itself.
int gmres_mgs_chain_coop(storm_hip_ctx *c, int64_t n, const int *done, double *w, const double *const *q, int k, int m,
                         double *H, double *norm2_out, bool normalise, bool *taken, const MgsGivens *givens,
                         const ChainApply *apply, bool *applied) {
  *taken = false;
  if (applied) *applied = false;
  if (c->opt_coop_mgs == 0 || c->coop_disabled != 0 || c->comm != nullptr || k + 1 > kMgsMaxVectors || c->opt_profile_spmv != 0)
    return STORM_HIP_OK;
  const MgsChoice ch = mgs_choose(c, n, q[k], apply, applied != nullptr);
  if (ch.fn == nullptr) return STORM_HIP_OK;
  if (ch.quad && c->d_quad_slots == nullptr) {
    const size_t bytes = std::max((size_t)2 * (256 + 8) * kQuadSlotStride, (size_t)2 * kDenseMaxValues * 256 * 16);  // either form
    HIP_TRY(hipMalloc((void **)&c->d_quad_slots, bytes));
    HIP_TRY(hipMemsetAsync(c->d_quad_slots, 0, bytes, c->stream));
  }
  MgsArgs a;
  for (int i = 0; i <= k; ++i) a.q[i] = q[i];
  for (int i = k + 1; i < kMgsMaxVectors; ++i) a.q[i] = q[0];
  a.w = w, a.H = H, a.norm2_out = norm2_out, a.n_rows = n, a.n_slices = (n + kWave - 1) / kWave, a.k = k, a.m = m;
  a.normalise = normalise ? 1 : 0;
  a.pairs = ch.pairs;
  a.seq_base = (1ull << 31) | (c->lat_seq & 0x7fffffffull);  // bit 31: never the tag of a CG solve (those count from 1)
  c->lat_seq += (unsigned long long)k + 2;
  a.slots = c->d_lat_slots, a.done = done;
  a.givens = (givens != nullptr && normalise && c->opt_coop_mgs != 2) ? *givens  // (coop_mgs = 2: A/B, rotations by the caller)
                                                                        : MgsGivens{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  a.quad_slots = c->d_quad_slots;
  a.dense = 1;  // (see MgsArgs)
  a.prefetch = (int)(c->opt_coop_mgs_prefetch != 0);
  a.xcd_runs = (int)(c->opt_coop_mgs_xcd_runs != 0);
  a.descend = (int)(c->opt_coop_mgs_alternate != 0 && (k & 1) != 0);
  a.rotate_early = (int)(c->opt_coop_mgs_rotate_early != 0);
  a.ap_pack = nullptr, a.ap_dict = nullptr, a.ap_x = nullptr, a.ap_max_gather = 0, a.ap_alpha = 0.0, a.ap_beta = 0.0;
  for (int i = 0; i < 6; ++i) a.ap_off[i] = 0;
  if (ch.with_apply) {
    const storm_hip_op *aop = apply->op;
    a.ap_pack = aop->d_pack, a.ap_dict = aop->d_dict, a.ap_x = apply->x;
    for (int i = 0; i < 6; ++i) a.ap_off[i] = aop->canon_off[i];
    a.ap_max_gather = (int)(aop->n_rows + aop->n_halo) + kVecGuard + 2;
    a.ap_alpha = apply->alpha, a.ap_beta = apply->beta;
  }
  a.prof = nullptr;
  if (c->opt_resident_profile != 0 && ch.laps && k == m - 1) {  // (diagnostic: the longest chain of a cycle)
    if (c->d_res_prof == nullptr) HIP_TRY(hipMalloc((void **)&c->d_res_prof, sizeof(long long) * 256 * 8));
    a.prof = c->d_res_prof, c->res_prof_blocks = (int)ch.blocks;
  }
  bool formed = false;
  if (apply != nullptr && applied != nullptr && !ch.with_apply) {  // a chain variant that READS w: the apply goes first
    STORM_TRY(spmv_launch(apply->op, host_scal(apply->alpha), host_scal(apply->beta), apply->x, w, nullptr, done));
    formed = true;
  }
  void *args[] = {&a};
  *taken = coop_launch(c, ch.fn, (unsigned)ch.blocks, args, ch.dyn_lds, ch.threads);
  if (!*taken) c->lat_seq -= (unsigned long long)k + 2;
  else ++c->n_mgs_chain_steps, c->n_mgs_quad_steps += ch.quad, c->n_mgs_lds_steps += ch.lds;
  if (applied) *applied = formed || (*taken && ch.with_apply);
  return STORM_HIP_OK;
}

}  // namespace storm
