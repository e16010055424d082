// A reduction that finishes inside the kernel that produced its partial sums, for ANY grid size: two levels of
// tickets.  Blocks form groups of kTicketGroup; the last block of a group to arrive folds the group's partials, the
// last group-folder to arrive folds the groups' sums and owns the result -- it can run the scalar step of the
// solver right there, and the launch of a separate final-pass kernel (~4-5 us, dependent) disappears.
//
// Protocol (no cache-wide fence anywhere -- an agent-scope release writes back the whole L2 on this chip):
//   * a partial sum is published by lane 0 with an atomic EXCHANGE whose returned value it waits for: a returning
//     read-modify-write has been performed at the point of coherence (a plain write-through store is acknowledged
//     by the XCD's L2 before the data has left it -- under load a reader on another XCD could still miss it: seen
//     as a rare wrong sum at 256^3); only then it draws its ticket with a relaxed agent-scope atomic add; whoever
//     draws the last ticket therefore finds every partial at the coherence point and reads it with coherent loads;
//   * counters re-arm themselves (the drawer of the last ticket stores 0), so a buffer zeroed once serves forever;
//   * only wave 0 of a block takes part (the other waves retire as soon as the block's partial is formed);
//   * fixed folding order (lane i takes entry i, i + 64, ...; xor-shuffle tree): run-to-run reproducible.
#pragma once
#include "common.hpp"
#include "wave_device.hpp"

namespace storm {

constexpr int kTicketGroup = 64;
constexpr int kTicketStride = 16;          // ints between counters (one 64-byte line each)
constexpr int kTicketMaxGroups = 2048;     // 131 072 blocks
// every streaming kernel that finishes its reduction with tickets (blas1.hip, krylov_engine.hip, the fused loops' units) sizes its grid
// with stream_blocks(): whatever the row count, its blocks fit the counters and the group-sum buffer
static_assert(kMaxStreamBlocks <= kTicketGroup * kTicketMaxGroups, "stream_blocks() may exceed the ticket counters");

struct TicketArgs {
  int *cnt;       // [1 + kTicketMaxGroups] counters, kTicketStride apart; null = tickets off
  double *part1;  // [K][n_blocks] block partials
  double *part2;  // [K][n_groups] group partials
};

// Store v[0 .. k) to p[j * stride] so that they are at the point of coherence when the function returns: atomic
// EXCHANGES, all issued back to back, whose returned values are then consumed -- a returning read-modify-write has
// been performed at the point of coherence; the empty statement that consumes them is also a compiler barrier for
// memory, so nothing later is issued before they are back.
template <int KMAX>
__device__ __forceinline__ void ticket_publish(double *p, size_t stride, const double (&v)[KMAX], int k) {
  unsigned long long seen = 0ull;
#pragma unroll
  for (int j = 0; j < KMAX; ++j) {
    if (j < k) {
#ifdef STORM_TICKET_STORE_EXPERIMENT  // (what the first version did; kept to reproduce the failure)
      __hip_atomic_store(p + (size_t)j * stride, v[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
      seen ^= __hip_atomic_exchange(reinterpret_cast<unsigned long long *>(p + (size_t)j * stride),
                                    (unsigned long long)__double_as_longlong(v[j]), __ATOMIC_RELAXED,
                                    __HIP_MEMORY_SCOPE_AGENT);
#endif
    }
  }
#ifdef STORM_TICKET_STORE_EXPERIMENT
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
#endif
  asm volatile("" : : "v"(seen) : "memory");
}
__device__ __forceinline__ double ticket_wave_sum(double v) {
  return wave_sum_all(v);  // (= the xor butterfly's value in every lane, bit for bit: wave_device.hpp)
}

// The top fold in two halves, so that a kernel with loads of its own can put the fold's behind them: lane i takes groups
// i, i + 64, ... in ascending order (the order of the sums is fixed); ticket_groups_issue requests one batch of them --
// kTicketAhead groups per lane and value, all before the first is added --, ticket_groups_add adds the batch to the lane's
// sums.  Every top fold of the library adds through ticket_groups_add and ends with ticket_wave_sum: the order is written once.
//   COHERENT: loads at the point of coherence, for the wave that drew the last top-level ticket of a running kernel;
//   false: plain loads, for a kernel launched behind the one that stored the group sums (the kernel boundary releases them).
template <int KMAX>
struct TicketGroupFlight {
  static constexpr int kAhead = KMAX <= 4 ? 4 : 2;
  double v[KMAX][kAhead];
};
constexpr unsigned kTicketFoldBatch1 = kWave * 4;  // the groups one batch of one value holds (TicketGroupFlight<1>)
template <int KMAX, bool COHERENT>
__device__ __forceinline__ void ticket_groups_issue(const double *part2, int k, unsigned ng, unsigned i0, TicketGroupFlight<KMAX> &f) {
#pragma unroll
  for (int j = 0; j < KMAX; ++j)
#pragma unroll
    for (int u = 0; u < TicketGroupFlight<KMAX>::kAhead; ++u) {
      const unsigned i = i0 + u * kWave;
      f.v[j][u] = 0.0;
      if (j < k && i < ng) {
        if constexpr (COHERENT) f.v[j][u] = __hip_atomic_load(part2 + (size_t)j * ng + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else f.v[j][u] = part2[(size_t)j * ng + i];
      }
    }
}
template <int KMAX>
__device__ __forceinline__ void ticket_groups_add(const TicketGroupFlight<KMAX> &f, unsigned ng, unsigned i0, double (&total)[KMAX]) {
#pragma unroll
  for (int j = 0; j < KMAX; ++j)
#pragma unroll
    for (int u = 0; u < TicketGroupFlight<KMAX>::kAhead; ++u)
      if (i0 + u * kWave < ng) total[j] += f.v[j][u];
}
// The top fold, by the wave that drew the last top-level ticket: total[j] = the sum of the ng group sums of value j, in
// all lanes.
template <int KMAX>
__device__ __forceinline__ void ticket_fold_groups(const TicketArgs &t, int k, unsigned ng, double (&total)[KMAX]) {
  const unsigned lane = threadIdx.x & (kWave - 1);
#pragma unroll
  for (int j = 0; j < KMAX; ++j) total[j] = 0.0;
  for (unsigned i0 = lane; i0 < ng; i0 += kWave * TicketGroupFlight<KMAX>::kAhead) {
    TicketGroupFlight<KMAX> f;
    ticket_groups_issue<KMAX, true>(t.part2, k, ng, i0, f);
    ticket_groups_add<KMAX>(f, ng, i0, total);
  }
#pragma unroll
  for (int j = 0; j < KMAX; ++j) total[j] = ticket_wave_sum(total[j]);
}
// ... of ONE value whose ng <= kTicketFoldBatch1 group sums a kernel behind the producer requested with
// ticket_groups_issue<1, false>(part2, 1, ng, lane, f): ticket_fold_groups<1>'s adds in its order, hence its bits.
__device__ __forceinline__ double ticket_fold_groups_flight(const TicketGroupFlight<1> &f, unsigned ng) {
  const unsigned lane = threadIdx.x & (kWave - 1);
  double total[1] = {0.0};
  ticket_groups_add<1>(f, ng, lane, total);
  return ticket_wave_sum(total[0]);
}

// Wave 0 of every block calls this (all 64 lanes) with the block's partials `mine[0 .. k)` (k <= KMAX).
// Returns true in wave 0 of exactly one block, the last to arrive, with total[j] valid in all lanes.
template <int KMAX>
__device__ __forceinline__ bool ticket_reduce_wave0(const TicketArgs &t, const double (&mine)[KMAX], int k, unsigned bx,
                                                    unsigned nb, double (&total)[KMAX]) {
  const unsigned lane = threadIdx.x & (kWave - 1);
  const unsigned g = bx / kTicketGroup, ng = (nb + kTicketGroup - 1) / kTicketGroup;
  const unsigned gsize = (nb - g * kTicketGroup) < (unsigned)kTicketGroup ? (nb - g * kTicketGroup) : (unsigned)kTicketGroup;
  int go = 0;
  if (lane == 0) {
    ticket_publish<KMAX>(t.part1 + bx, nb, mine, k);
    int *c = t.cnt + (size_t)(1 + g) * kTicketStride;
    if (__hip_atomic_fetch_add(c, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (int)gsize - 1) {
      __hip_atomic_store(c, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      go = 1;
    }
  }
  go = __shfl(go, 0, kWave);
  if (!go) return false;
  double gp[KMAX];
  // (all loads first, then the sums: a load per value waited for in turn costs a trip to memory each -- with ten values
  //  that was 12 us per group, and 24 - 57 us of serial tail in the last fold below)
#pragma unroll
  for (int j = 0; j < KMAX; ++j) {
    gp[j] = 0.0;
    if (j < k && lane < gsize)
      gp[j] = __hip_atomic_load(t.part1 + (size_t)j * nb + (size_t)g * kTicketGroup + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
#pragma unroll
  for (int j = 0; j < KMAX; ++j) gp[j] = ticket_wave_sum(gp[j]);
  go = 0;
  if (lane == 0) {
    ticket_publish<KMAX>(t.part2 + g, ng, gp, k);
    if (__hip_atomic_fetch_add(t.cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (int)ng - 1) {
      __hip_atomic_store(t.cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      go = 1;
    }
  }
  go = __shfl(go, 0, kWave);
  if (!go) return false;
  ticket_fold_groups<KMAX>(t, k, ng, total);
  return true;
}

// ticket_reduce_wave0 for a block that stands for SEVERAL virtual blocks of a grid of nb (a marching kernel that forms,
// plane by plane, the partials a one-trip streaming kernel's blocks would have formed): every lane of wave 0 that is `on`
// holds the partial `mine` of virtual block bxv (one value per block; the lanes' bxv all differ).  The partials are published by all
// lanes at once, then every group takes ONE ticket draw for all the slots this block owns in it ("old + count == group
// size" is the last), and the group sums and the top fold are ticket_reduce_wave0's: the same values in the same
// order, whichever hardware block formed them.  Round trips to memory do not grow with the number of slots: every
// step is issued for all its lanes (or, the group loads, four groups) at a time.
// Level 1 of it: returns the lanes that drew the last ticket of a group (0: none), each with its group's sum in `gsum`;
// `g`, `ng`: the lane's group and the number of groups.
__device__ __forceinline__ unsigned long long ticket_slots_level1(const TicketArgs &t, double mine, bool on, unsigned bxv, unsigned nb,
                                                                  unsigned &g, unsigned &ng, double &gsum) {
  const unsigned lane = threadIdx.x & (kWave - 1);
  g = bxv / kTicketGroup, ng = (nb + kTicketGroup - 1) / kTicketGroup;
  const unsigned gsize = (nb - g * kTicketGroup) < (unsigned)kTicketGroup ? (nb - g * kTicketGroup) : (unsigned)kTicketGroup;
  if (on) {
    const double v[1] = {mine};
    ticket_publish<1>(t.part1 + bxv, nb, v, 1);
  }
  // the lowest lane of every group draws for all of the block's slots in it
  int count = 0;
  bool leader = false;
  for (unsigned long long rest = __ballot(on); rest != 0ull;) {
    const int first = __ffsll((long long)rest) - 1;
    const unsigned long long same = __ballot(on && g == (unsigned)__shfl((int)g, first, kWave));
    if ((int)lane == first) leader = true, count = __popcll(same);
    rest &= ~same;
  }
  int go = 0;
  if (leader) {
    int *c = t.cnt + (size_t)(1 + g) * kTicketStride;
    if (__hip_atomic_fetch_add(c, count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + count == (int)gsize) {
      __hip_atomic_store(c, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      go = 1;
    }
  }
  // the groups this block completed: their sums (ticket_reduce_wave0's loads and wave sum) into the drawing lanes
  const unsigned long long done = __ballot(go != 0);
  gsum = 0.0;
  for (unsigned long long fin = done; fin != 0ull;) {
    int at[4];
    double gp[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      at[j] = fin != 0ull ? __ffsll((long long)fin) - 1 : -1;
      if (at[j] >= 0) fin &= fin - 1ull;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      gp[j] = 0.0;
      if (at[j] >= 0) {
        const unsigned gj = (unsigned)__shfl((int)g, at[j], kWave), nj = (unsigned)__shfl((int)gsize, at[j], kWave);
        if (lane < nj)
          gp[j] = __hip_atomic_load(t.part1 + (size_t)gj * kTicketGroup + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double sj = ticket_wave_sum(gp[j]);
      if ((int)lane == at[j]) gsum = sj;
    }
  }
  return done;
}
__device__ __forceinline__ bool ticket_reduce_wave0_slots(const TicketArgs &t, double mine, bool on, unsigned bxv, unsigned nb,
                                                          double *total) {
  const unsigned lane = threadIdx.x & (kWave - 1);
  unsigned g, ng;
  double gsum;
  const unsigned long long fin = ticket_slots_level1(t, mine, on, bxv, nb, g, ng, gsum);
  if (fin == 0ull) return false;
  const int n_fin = __popcll(fin);
  if ((fin >> lane) & 1ull) {
    const double v[1] = {gsum};
    ticket_publish<1>(t.part2 + g, ng, v, 1);
  }
  int go = 0;
  if (lane == 0) {
    if (__hip_atomic_fetch_add(t.cnt, n_fin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + n_fin == (int)ng) {
      __hip_atomic_store(t.cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      go = 1;
    }
  }
  go = __shfl(go, 0, kWave);
  if (!go) return false;
  double tot[1];
  ticket_fold_groups<1>(t, 1, ng, tot);
  *total = tot[0];
  return true;
}
// ... that ENDS at the group sums: the last block of a group stores its sum to part2[g] with a plain store and nobody
// draws a top-level ticket -- the kernel boundary releases the sums, and a kernel launched behind this one folds them
// (ticket_groups_issue<1, false>, ticket_fold_groups_flight): the chain of round trips behind the group sums -- the awaited
// exchange, the top ticket, the fold's loads -- is gone from the producer's tail.  The group counters re-arm as ever.
__device__ __forceinline__ void ticket_reduce_wave0_slots_to_groups(const TicketArgs &t, double mine, bool on, unsigned bxv, unsigned nb) {
  const unsigned lane = threadIdx.x & (kWave - 1);
  unsigned g, ng;
  double gsum;
  const unsigned long long fin = ticket_slots_level1(t, mine, on, bxv, nb, g, ng, gsum);
  if ((fin >> lane) & 1ull) t.part2[g] = gsum;
}

}  // namespace storm
