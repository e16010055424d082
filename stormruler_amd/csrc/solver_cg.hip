// The fused CG loop of a stencil operator (SolverCg.hpp:54-126) and its kernels; see solver_fused.hip.
#include <algorithm>
#include "solver_fused.hpp"
#include "blas1_device.hpp"
#include "spmv_device.hpp"

namespace storm {

// The reduction code of cg_r_kernel and cg_r_recompute_kernel: a residual kernel must form alpha and sum <r,r> exactly
// as the other does.  Prologue: alpha = safe_divide(gamma, <p,z>), with <p,z> folded from pz_partials by every block
// (the same n_pz values in the same order, hence the same alpha) or read from the slab; block 0 stores both.
// (Fold: block_fold of the partials, or -- cg_r_planes_kernel, whose fold's loads are in flight since block_fold_issue --
//  block_fold_sum of them: the same sum.  Gamma: the slab's <r,r>, read here or, by that kernel, with its first loads:
//  nothing writes it before the grid's last block has drawn its ticket)
template <class Fold, class Gamma>
__device__ __forceinline__ double cg_r_alpha_of(SolverState *st, bool folds, Fold fold, Gamma gamma) {
  double pz;
  if (folds) {
    pz = fold();
    if (blockIdx.x == 0 && threadIdx.x == 0) st->s[S_PZ] = pz;
  } else {
    pz = st->s[S_PZ];
  }
  const double alpha = safe_divide(gamma(), pz);
  if (blockIdx.x == 0 && threadIdx.x == 0) st->s[S_ALPHA] = alpha;  // for cg_xp_kernel / the next step kernel
  return alpha;
}
__device__ __forceinline__ double cg_r_alpha(SolverState *st, const double *__restrict__ pz_partials, int n_pz, double *lds4) {
  return cg_r_alpha_of(st, pz_partials != nullptr, [&] { return block_fold(pz_partials, n_pz, lds4); }, [&] { return st->s[S_GAMMA]; });
}
__device__ __forceinline__ double cg_r_alpha(SolverState *st, bool folds, const FoldWhole &pz_flight, int n_pz, double gamma,
                                             double *lds4) {
  return cg_r_alpha_of(st, folds, [&] { return block_fold_sum(pz_flight, n_pz, lds4); }, [&] { return gamma; });
}
// Epilogue: block bx's partial of <r,r> into partials[bx] (no tickets), or <r,r> finished here (ticket_device.hpp) and
// the scalar step of SolverCg.hpp:110-125 with the convergence rule in the last block: no final-pass launch.
__device__ __forceinline__ void cg_r_finish(SolverState *st, double acc, unsigned bx, double *__restrict__ partials,
                                            const TicketArgs &tickets, const IpcDev &w, int use_ipc, double *lds4) {
  const double s = block_sum256(acc, lds4);
  if (tickets.cnt == nullptr) {
    if (threadIdx.x == 0) partials[bx] = s;
    return;
  }
  if (threadIdx.x >= kWave) return;
  const double mine[1] = {s};
  double total[1];
  if (ticket_reduce_wave0<1>(tickets, mine, 1, bx, gridDim.x, total)) {
    if (use_ipc == 1) ipc_allreduce_wave<1>(w, total, 1);  // the global <r,r>: the same bits on every rank
    if (threadIdx.x == 0) {
      st->s[S_GAMMA_NEW] = total[0];
      // (use_ipc == 2: this rank's sum only -- the host enqueues the all-reduce and the step behind this kernel)
      if (use_ipc != 2) do_step(STEP_CG_RR, st, GmresDev{});
    }
  }
}

// CG iteration, vector part, in two kernels around the <r,r> reduction (SolverCg.hpp:97-123):
//   cg_r_kernel : alpha = safe_divide(gamma, <p,z>);  r -= alpha z;  partial <r,r>
//   cg_xp_kernel: x += alpha p;  p = r + beta p
// The reference's `x += alpha p` (:98) is moved behind the reduction next to the p update, where p
// is read anyway: same values, 64N instead of 72N bytes per iteration.  cg_xp must apply the x
// update of the iteration in which the solver converged (p no longer matters then), so it is
// keyed on the iteration counter, not on `done`.
// With pz_partials != null the kernel folds the (first-pass) partials of <p,z> itself -- every block the same
// n_pz values in the same order, hence the same alpha -- and the separate final-pass launch disappears.
__global__ __launch_bounds__(kBlock) void cg_r_kernel(int64_t n, SolverState *st, double *__restrict__ r,
                                                      const double *__restrict__ z,
                                                      double *__restrict__ partials, int nt,
                                                      const double *__restrict__ pz_partials, int n_pz, int reverse,
                                                      TicketArgs tickets, IpcDev w, int use_ipc) {
  if (st->done) return;
  __shared__ double lds4[4];
  // `reverse`: the blocks sweep the rows from the far end (see the sweep-direction note in storm_hip_solve_cg);
  // block bx still owns the same rows and the same partial, whichever way the grid is dealt out
  const unsigned bx = reverse ? gridDim.x - 1 - blockIdx.x : blockIdx.x;
  const double alpha = cg_r_alpha(st, pz_partials, n_pz, lds4);
  double acc = 0.0;
  const int64_t n2 = n >> 1;
  double2v *r2 = reinterpret_cast<double2v *>(r);
  const double2v *z2 = reinterpret_cast<const double2v *>(z);
  nt_dispatch(nt, [&](auto nt) {
  for (int64_t base = (int64_t)bx * (kBlock * kUnroll) + threadIdx.x; base < n2;
       base += (int64_t)gridDim.x * (kBlock * kUnroll)) {
    double2v vr[kUnroll], vz[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int64_t i = base + u * kBlock;
      if (i < n2) vr[u] = ldv(r2 + i, nt), vz[u] = ldv(z2 + i, nt);
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int64_t i = base + u * kBlock;
      if (i < n2) {
        vr[u] -= alpha * vz[u];
        stv(r2 + i, vr[u], nt);
        acc += vr[u].x * vr[u].x;
        acc += vr[u].y * vr[u].y;
      }
    }
  }
  });
  if ((n & 1) && bx == 0 && threadIdx.x == 0) {
    const double vr = r[n - 1] - alpha * z[n - 1];
    r[n - 1] = vr;
    acc += vr * vr;
  }
  cg_r_finish(st, acc, bx, partials, tickets, w, use_ipc, lds4);
}

// The residual recompute (option cg_residual_march): cg_r_kernel for the fused CG step on one rank, with z = A p'
// RECOMPUTED instead of read back, so that the step kernel (cg_step_march_kernel) stores no z.  Per row it streams p'
// (8 B), the record index (1 B) and r (read and written, 16 B): 25 B where z cost 8 B stored + 8 B read back.
// Everything cg_r_kernel decides is kept: its grid, its rows per thread and their order, its statements -- so r AND
// <r,r> are the same bits, and the solve is the one the z-storing loop computes.  A wave holds 64 consecutive row pairs
// per unrolled step, so the +-1 neighbours come from the next lanes (lanes 0 and 63 load their outer one) and the
// +-a / +-b lines are 16-byte gathers of p' (the tiled kernel's clamping: an absent neighbour has weight 0).  z is
// lattice_pair_apply of the operands the step kernel had in its registers: p' from memory is what that kernel stored.
template <bool IDX>
__global__ __launch_bounds__(kBlock) void cg_r_recompute_kernel(int64_t n, SolverState *st, double *__restrict__ r,
                                                                const double *__restrict__ p, SellArgs A, CanonTileArgs T,
                                                                Scal alpha_s, Scal beta_s, const double *__restrict__ pz_partials,
                                                                int n_pz, int reverse, TicketArgs tickets) {
  if (st->done) return;
  __shared__ double lds4[4];
  __shared__ double dict_sh[32];
  extern __shared__ __attribute__((aligned(16))) unsigned long long words_sh[];  // (IDX: the word table)
  const int lane = threadIdx.x & (kWave - 1);
  if (threadIdx.x < 32) dict_sh[threadIdx.x] = A.dict[threadIdx.x];
  if (IDX) rec_table_fill(A, words_sh);
  __syncthreads();
  const unsigned bx = reverse ? gridDim.x - 1 - blockIdx.x : blockIdx.x;  // (as cg_r_kernel)
  const double alpha = cg_r_alpha(st, pz_partials, n_pz, lds4);
  const double op_alpha = ld_scal2(alpha_s), op_beta = ld_scal2(beta_s);
  const int64_t a = T.a, b = T.b, mg = T.max_gather;
  const char *pg = reinterpret_cast<const char *>(p) - (size_t)kVecGuard * 8;
  auto pair_at = [&](int64_t row) {  // p'[row], p'[row + 1], row even; guard-relative and clamped like every gather
    int64_t gi = row + kVecGuard;
    gi = gi < 0 ? 0 : (gi > mg ? mg : gi);
    return *reinterpret_cast<const double2v *>(pg + (size_t)gi * 8);
  };
  auto one_at = [&](int64_t row) {
    int64_t gi = row + kVecGuard;
    gi = gi < 0 ? 0 : (gi > mg + 1 ? mg + 1 : gi);
    return *reinterpret_cast<const double *>(pg + (size_t)gi * 8);
  };
  double acc = 0.0;
  const int64_t n2 = n >> 1;
  double2v *r2 = reinterpret_cast<double2v *>(r);
  // (the loop runs while the wave's FIRST pair is in range, every lane inside it: the lane moves need the whole wave;
  //  a lane past the end works on the last pair and neither stores nor sums -- as cg_r_kernel's thread skips it)
  for (int64_t base = (int64_t)bx * (kBlock * kUnroll) + threadIdx.x; base - lane < n2;
       base += (int64_t)gridDim.x * (kBlock * kUnroll)) {
    double2v vr[kUnroll], c[kUnroll], nb[kUnroll][4];
    double el[kUnroll];
    RecRaw<IDX> w[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int64_t i = base + u * kBlock;
      const int64_t row = 2 * (i < n2 ? i : n2 - 1);
      vr[u] = r2[row >> 1];
      c[u] = pair_at(row);
      w[u] = rec_load<IDX>(A, (uint32_t)row);
      nb[u][0] = pair_at(row - b), nb[u][1] = pair_at(row - a), nb[u][2] = pair_at(row + a), nb[u][3] = pair_at(row + b);
      el[u] = 0.0;
      if (lane == 0) el[u] = one_at(row - 1);
      if (lane == kWave - 1) el[u] = one_at(row + 2);
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int64_t i = base + u * kBlock;
      double2v xg[6];
      xg[0] = nb[u][0], xg[1] = nb[u][1], xg[4] = nb[u][2], xg[5] = nb[u][3];
      const double left = dpp_shift<0x138>(c[u].y);   // wave_shr:1 -- lane i receives lane i - 1
      const double right = dpp_shift<0x130>(c[u].x);  // wave_shl:1 -- lane i receives lane i + 1
      xg[2].x = lane == 0 ? el[u] : left;
      xg[2].y = c[u].x;
      xg[3].x = c[u].y;
      xg[3].y = lane == kWave - 1 ? el[u] : right;
      const double2v vz = lattice_pair_apply(dict_sh, rec_word<IDX>(w[u], words_sh), xg, c[u], op_alpha, op_beta);
      if (i < n2) {  // cg_r_kernel's statements, verbatim
        vr[u] -= alpha * vz;
        r2[i] = vr[u];
        acc += vr[u].x * vr[u].x;
        acc += vr[u].y * vr[u].y;
      }
    }
  }
  // (an odd last row: cg_r_kernel's tail -- never here, the recompute takes operators with an even row count)
  // (<r, r> finishes here as in cg_r_kernel: the recompute always runs with tickets)
  cg_r_finish(st, acc, bx, nullptr, tickets, IpcDev{}, 0, lds4);
}

// Whether the residual recompute takes iteration k > 0 of the fused CG loop: one rank, an unsplit operator with an even
// row count whose fused step is the marching kernel, reductions finished by tickets, no ticket_verify (it reads z).
static bool cg_r_recompute_applies(const storm_hip_op *op, bool tick) {
  storm_hip_ctx *c = op->ctx;
  MarchArgs M;
  int nb = 0;
  return c->opt_cg_residual_march != 0 && tick && c->comm == nullptr && c->opt_ticket_verify == 0 && op->n_rows % 2 == 0 &&
         spmv_can_march(op) && cg_march_geometry(op, &M, &nb);
}
static int cg_r_recompute_run(const storm_hip_op *op, int nbv, Scal alpha, Scal beta, const double *p, SolverState *st, double *r,
                              const double *pz_partials, int n_pz, int reverse) {
  storm_hip_ctx *c = op->ctx;
  CanonTileArgs T;
  int nbt = 0;
  STORM_REQUIRE(canon_tile_geometry(op, &T, &nbt), "cg: the residual recompute needs a lattice operator");
  const SellArgs A = lattice_args(op);
  const size_t lds = sizeof(uint64_t) * (size_t)A.rec_words_n;
  const TicketArgs tk{c->d_tickets, c->d_partials, c->d_ticket_sums};
  if (A.rec_idx != nullptr)
    hipLaunchKernelGGL(cg_r_recompute_kernel<true>, dim3(nbv), dim3(kBlock), lds, c->stream, op->n_rows, st, r, p, A, T, alpha,
                       beta, pz_partials, n_pz, reverse, tk);
  else
    hipLaunchKernelGGL(cg_r_recompute_kernel<false>, dim3(nbv), dim3(kBlock), lds, c->stream, op->n_rows, st, r, p, A, T, alpha,
                       beta, pz_partials, n_pz, reverse, tk);
  HIP_TRY(hipGetLastError());
  return STORM_HIP_OK;
}

// The residual recompute MARCHING over planes (option cg_residual_planes): the same r and the same <r,r> bits as the two
// kernels above, without the gathers.  At these sizes cg_r_kernel's grid is one trip per block, so its block bx owns rows
// [2048 bx, 2048 bx + 2048): with b % 2048 == 0 a run of ONE plane.  A block here owns run yt of the plane and a chunk of
// planes, and forms, plane by plane, what cg_r_kernel's block bx' = plane * (b / 2048) + yt forms: thread t holds pairs
// t + 256 u (u = 0 .. 3) of p' and r, sums them into one accumulator in cg_r_kernel's order, and the block's sum of the
// plane is partial bx'.  p' of the planes behind and ahead stays in registers while the march advances, the +-a lines and
// the +-1 rows at the wave ends come from an LDS copy of the plane (the run and a rows on either side; two buffers in
// rotation, one barrier per plane), so every row of p' is loaded once -- plus the halo lines (2 a / 2048 of a plane,
// adjacent runs of one XCD march in step) and the two planes that bound the chunk.  Loads run one plane ahead of the
// plane whose neighbours they are, two ahead of the plane being applied.
//   The per-plane sums stay in the block (each wave's wave_sum_down value in LDS: block_sum256 without its barriers) and
// are published when the chunk ends, all at once, through ticket_reduce_wave0_slots with cg_r_kernel's block count: one
// atomic round trip per plane inside the march would serialise it.  With rr_gate != 0 (option cg_rr_fold) the kernel ends at
// the group sums -- ticket_reduce_wave0_slots_to_groups -- and the launch behind it folds them and runs the scalar step.
//   168 VGPRs and 41 KB of LDS at a = 256 (49 KB at a = 512): three blocks per CU.  At 256^3 the 512 blocks of 16 planes
// are ONE round of two blocks per CU (32 planes, one block per CU: the same time; 8 planes, two rounds: 1.2 % slower), so
// every block pays the start's round trips: the first planes are requested before anything is waited for.
struct ResidualPlanesArgs {
  int a, b;
  int runs_per_plane;  // b / 2048
  int per_xcd;         // runs_per_plane / 8 when that divides (adjacent runs on one XCD, as the step kernel's tiles), else 0
  int planes;          // n / b
  int nz;              // planes per block
  int max_gather;      // largest guard-relative index a 16-byte load may start at
};
constexpr int kResidualMaxChunk = 32;  // planes per block at most (the per-plane sums: one lane of wave 0 each)
template <int HLP, bool IDX>  // HLP: halo pairs per thread and plane: ceil(a / 256); IDX: the row-record index
__global__ __launch_bounds__(kBlock) void cg_r_planes_kernel(SolverState *st, double *__restrict__ r, const double *__restrict__ p,
                                                             SellArgs A, ResidualPlanesArgs G, Scal alpha_s, Scal beta_s,
                                                             const double *__restrict__ pz_partials, int n_pz, int reverse,
                                                             TicketArgs tickets, long long rr_gate) {
  const int done = st->done;  // (tested behind the first loads: in a grid of one round every block pays the start's round trips)
  const double gamma = st->s[S_GAMMA];  // (with it: a load behind the fold would be one more round trip in front of the march)
  __shared__ double lds4[4];
  __shared__ double dict_sh[32];
  __shared__ double wave_part[kResidualMaxChunk * (kBlock / kWave)];
  extern __shared__ __attribute__((aligned(16))) double plane_sh[];  // [2][a + 2048 + a], then (IDX) the word table
  const int a = G.a, b = G.b;
  const int ldw = kStreamBlockElems + 2 * a;
  unsigned long long *words_sh = reinterpret_cast<unsigned long long *>(plane_sh + 2 * ldw);
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int bidx = reverse ? (int)(gridDim.x - 1 - blockIdx.x) : (int)blockIdx.x;
  int zc, yt;
  if (G.per_xcd > 0) {
    const int xcd = bidx & (kNumXcd - 1), j = bidx >> 3;
    zc = j / G.per_xcd;
    yt = xcd * G.per_xcd + (j - zc * G.per_xcd);
  } else {
    zc = bidx / G.runs_per_plane;
    yt = bidx - zc * G.runs_per_plane;
  }
  const int z_begin = zc * G.nz, z_end = min(z_begin + G.nz, G.planes), nz = z_end - z_begin;
  // (the blocks are dealt out from the far end under `reverse`, where the step kernel stopped; each still marches
  //  upwards: a downward march measured 0.2 % slower at 256^3)
  auto plane = [&](int s) { return z_begin + s; };  // s = -1 and s = nz: the planes next to the chunk
  const int p0 = yt * kStreamBlockElems;
  const char *pg = reinterpret_cast<const char *>(p) - (size_t)kVecGuard * 8;
  double2v *r2 = reinterpret_cast<double2v *>(r);

  // p' of one plane in flight: the own four pairs and this thread's share of the halo lines
  struct Flight {
    double2v p[kUnroll], hp[HLP];
  };
  int hat[HLP], hjj[HLP];  // where the thread's halo pairs sit in the LDS copy (-1: none), and in the plane
#pragma unroll
  for (int i = 0; i < HLP; ++i) {
    const int h = (int)threadIdx.x + kBlock * i;  // pair h of the plane's a halo pairs
    hjj[i] = 2 * h < a ? 2 * h - a : kStreamBlockElems + 2 * h - a;
    hat[i] = h < a ? a + hjj[i] : -1;
  }
  auto load_p = [&](int64_t row) {  // guard-relative and clamped: a plane below the first / above the last has weight 0
    int64_t gi = row + kVecGuard;
    gi = gi < 0 ? 0 : (gi > (int64_t)G.max_gather ? (int64_t)G.max_gather : gi);
    return *reinterpret_cast<const double2v *>(pg + (size_t)gi * 8);
  };
  auto issue_p = [&](int zp, bool own, Flight &f) {
    const int64_t row0 = (int64_t)zp * b + p0;
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) f.p[u] = load_p(row0 + 2 * ((int)threadIdx.x + kBlock * u));
#pragma unroll
    for (int i = 0; i < HLP; ++i) {
      f.hp[i] = double2v{0.0, 0.0};
      if (own && hat[i] >= 0) f.hp[i] = load_p(row0 + hjj[i]);
    }
  };
  auto issue_rw = [&](int zp, double2v (&vr)[kUnroll], RecRaw<IDX> (&w)[kUnroll]) {  // (an own plane: every row exists)
    const int64_t row0 = (int64_t)zp * b + p0;
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int64_t row = row0 + 2 * ((int)threadIdx.x + kBlock * u);
      vr[u] = r2[row >> 1];
      w[u] = rec_load<IDX>(A, (uint32_t)row);
    }
  };

  Flight cur, nxt, fl;
  double2v pm[kUnroll], vr[kUnroll];
  RecRaw<IDX> w[kUnroll];
  issue_p(plane(-1), false, fl);
#pragma unroll
  for (int u = 0; u < kUnroll; ++u) pm[u] = fl.p[u];
  issue_p(plane(0), true, cur);
  issue_rw(plane(0), vr, w);
  issue_p(plane(1), 1 < nz, nxt);
  // (<p,z> folded here, option cg_pz_fold: the n_pz <= kSinglePassPartials per-wave partials of the step kernel, requested
  //  behind the planes so that they arrive under them -- no launch of one block that folds them while HBM idles)
  const bool folds = pz_partials != nullptr;  // (block-uniform)
  FoldWhole pz_flight;
  if (folds) block_fold_issue(pz_partials, n_pz, pz_flight);
  if (threadIdx.x < 32) dict_sh[threadIdx.x] = A.dict[threadIdx.x];
  if (IDX) rec_table_fill(A, words_sh);
  if (done) return;
  const double alpha = cg_r_alpha(st, folds, pz_flight, n_pz, gamma, lds4);
  // (option cg_rr_fold, rr_gate != 0: the kernel ends at its group sums and the launch behind it folds them and runs the
  //  scalar step -- for that launch, which rotates S_GAMMA itself, the <r,r> this step began with and the counter the
  //  sums will produce: the proof that this kernel ran)
  if (rr_gate != 0 && blockIdx.x == 0 && threadIdx.x == 0) st->s[S_RR_GAMMA] = gamma, st->s[S_RR_GATE] = (double)rr_gate;
  const double op_alpha = ld_scal2(alpha_s), op_beta = ld_scal2(beta_s);
  // (the first barrier of the march covers dict_sh and the word table)
  for (int s = 0; s < nz; ++s) {
    const int zp = plane(s);
    double *buf = plane_sh + (s & 1) * ldw;
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) *reinterpret_cast<double2v *>(&buf[a + 2 * ((int)threadIdx.x + kBlock * u)]) = cur.p[u];
#pragma unroll
    for (int i = 0; i < HLP; ++i)
      if (hat[i] >= 0) *reinterpret_cast<double2v *>(&buf[hat[i]]) = cur.hp[i];
    double2v vrn[kUnroll];
    RecRaw<IDX> wn[kUnroll];
    if (s + 2 <= nz) issue_p(plane(s + 2), s + 2 < nz, fl);
    if (s + 1 < nz) issue_rw(plane(s + 1), vrn, wn);
    __syncthreads();  // the LDS copy of plane zp is complete; the other buffer is free once every wave is past this point
    const int64_t i0 = (((int64_t)zp * b + p0) >> 1) + threadIdx.x;  // cg_r_kernel's `base` of block zp * runs_per_plane + yt
    double acc = 0.0;
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int at = a + 2 * ((int)threadIdx.x + kBlock * u);
      double2v xg[6];
      march_neighbours(buf, at, a, lane, pm[u], nxt.p[u], cur.p[u], xg);
      const double2v vz = lattice_pair_apply(dict_sh, rec_word<IDX>(w[u], words_sh), xg, cur.p[u], op_alpha, op_beta);
      // cg_r_kernel's statements, verbatim
      vr[u] -= alpha * vz;
      r2[i0 + u * kBlock] = vr[u];
      acc += vr[u].x * vr[u].x;
      acc += vr[u].y * vr[u].y;
    }
    acc = wave_sum_down(acc);
    if (lane == 0) wave_part[s * (kBlock / kWave) + wave] = acc;
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) pm[u] = cur.p[u], vr[u] = vrn[u], w[u] = wn[u];
    cur = nxt, nxt = fl;
  }
  __syncthreads();
  if (threadIdx.x >= kWave) return;
  // lane s: cg_r_kernel's block of plane(s) -- its block_sum256 value, its partial slot, its ticket
  const bool on = lane < nz;
  const double mine = on ? block_sum256_of_waves(wave_part + lane * (kBlock / kWave)) : 0.0;
  const unsigned bxv = on ? (unsigned)(plane(lane) * G.runs_per_plane + yt) : 0u;
  if (rr_gate != 0) {  // (block-uniform)
    ticket_reduce_wave0_slots_to_groups(tickets, mine, on, bxv, (unsigned)(G.planes * G.runs_per_plane));
    return;
  }
  double total;
  if (ticket_reduce_wave0_slots(tickets, mine, on, bxv, (unsigned)(G.planes * G.runs_per_plane), &total) && threadIdx.x == 0) {
    st->s[S_GAMMA_NEW] = total;
    do_step(STEP_CG_RR, st, GmresDev{});
  }
}

// Whether the plane march takes the residual recompute: whole planes of whole 2 048-row runs (cg_r_kernel's blocks do not
// straddle planes), one trip per cg_r_kernel block, and two LDS copies of a plane's run within a block's 64 KiB.
static bool cg_r_planes_geometry(const storm_hip_op *op, ResidualPlanesArgs *G, int *n_blocks) {
  storm_hip_ctx *c = op->ctx;
  CanonTileArgs T;
  int nbt = 0;
  if (c->opt_cg_residual_planes == 0 || !canon_tile_geometry(op, &T, &nbt)) return false;
  const int64_t n = op->n_rows;
  if (T.b % kStreamBlockElems != 0 || n % T.b != 0 || n / kStreamBlockElems > kMaxStreamBlocks) return false;
  if ((int64_t)sizeof(double) * 2 * (kStreamBlockElems + 2 * T.a) + (int64_t)sizeof(uint64_t) * op->rec_words > 60 * 1024) return false;
  G->a = T.a, G->b = T.b, G->max_gather = T.max_gather;
  G->runs_per_plane = T.b / kStreamBlockElems;
  G->per_xcd = (G->runs_per_plane % kNumXcd == 0 && c->opt_spmv_xcd_remap != 0) ? G->runs_per_plane / kNumXcd : 0;
  G->planes = (int)(n / T.b);
  // (option cg_residual_chunk is the chunk of a large lattice; a smaller one marches fewer planes per block so that the
  //  grid still holds about cg_residual_fill blocks, as cg_march_geometry does for the step kernel)
  const int64_t zc = std::min<int64_t>(std::max<int64_t>(c->opt_cg_residual_chunk, 2), kResidualMaxChunk);
  const int64_t want = c->opt_cg_residual_fill;
  const int64_t fill = want > 0 ? (int64_t)G->planes * G->runs_per_plane / want : zc;
  G->nz = (int)std::min<int64_t>(std::min<int64_t>(zc, std::max<int64_t>(2, fill)), G->planes);
  *n_blocks = ((G->planes + G->nz - 1) / G->nz) * G->runs_per_plane;
  return true;
}
// (rr_partials: where the kernel's <r,r> slots go -- the workspace's start, or behind pz_partials where the kernel folds the
//  step kernel's partials itself: a block that starts late must still find them)
// (rr_gate != 0: the kernel ends at the group sums of <r,r> in the context's group-sum buffer; see cg_rr_finish_kernel)
static int cg_r_planes_run(const storm_hip_op *op, const ResidualPlanesArgs &G, int n_blocks, Scal alpha, Scal beta, const double *p,
                           SolverState *st, double *r, const double *pz_partials, int n_pz, int reverse, double *rr_partials,
                           long long rr_gate = 0) {
  storm_hip_ctx *c = op->ctx;
  STORM_REQUIRE(pz_partials == nullptr || n_pz <= kSinglePassPartials, "cg: the plane march folds at most %d partials of <p,z>, not %d",
                kSinglePassPartials, n_pz);
  const SellArgs A = lattice_args(op);
  const size_t lds = sizeof(double) * 2 * (size_t)(kStreamBlockElems + 2 * G.a) + sizeof(uint64_t) * (size_t)A.rec_words_n;
  const TicketArgs tk{c->d_tickets, rr_partials, c->d_ticket_sums};
#define PLANES_GO(HLP_, IX_)                                                                                                   \
  hipLaunchKernelGGL((cg_r_planes_kernel<HLP_, IX_>), dim3(n_blocks), dim3(kBlock), lds, c->stream, st, r, p, A, G, alpha, beta, \
                     pz_partials, n_pz, reverse, tk, rr_gate)
  if (G.a <= kBlock) {
    if (A.rec_idx != nullptr) PLANES_GO(1, true);
    else PLANES_GO(1, false);
  } else {
    if (A.rec_idx != nullptr) PLANES_GO(2, true);
    else PLANES_GO(2, false);
  }
#undef PLANES_GO
  HIP_TRY(hipGetLastError());
  return STORM_HIP_OK;
}

// Option cg_rr_fold: the scalar step behind a residual kernel that ended at its group sums.  Inside the loop the NEXT
// iteration's step kernel runs it (spmv_lattice.hip cg_step_march_kernel<.., RR>); behind the solve's last enqueued
// iteration there is none, and this one wave does: the same fold, the same cg_rr_eval, the same stores.  (cg_xp_kernel,
// which follows, could: but each of its blocks -- 32 768 at 256^3 -- would fold the sums for one load of alpha, and it
// serves every other road of the loop.)  The gate: a residual kernel that found the solve done left no sums.
__global__ __launch_bounds__(kWave) void cg_rr_finish_kernel(SolverState *st, const double *__restrict__ rr_sums, int rr_ng,
                                                             long long my_iteration) {
  const double gate = st->s[S_RR_GATE], gamma_bar = st->s[S_RR_GAMMA];
  const AdvanceIn in{st->initial_error, st->abs_tol, st->rel_tol, my_iteration - 1, st->num_iterations};
  TicketGroupFlight<1> f;
  ticket_groups_issue<1, false>(rr_sums, 1, (unsigned)rr_ng, threadIdx.x, f);
  if (gate != (double)my_iteration) return;
  const CgRrOutcome o = cg_rr_eval(ticket_fold_groups_flight(f, (unsigned)rr_ng), gamma_bar, in);
  if (threadIdx.x == 0) cg_rr_store(st, o);
}

// Five streams (3 loads, 2 stores): measured best with ONE 16-byte access per stream and thread in flight
// (tools/cg_kernels_bench.hip at 256^3: U = 1 105.6 us, U = 2 108.2, U = 4 111.4 -- and U = 8 615 us: a wave that
// holds too many loads in flight stalls the memory pipeline), unlike the 2- and 3-stream kernels (U = 4).
constexpr int kUnrollXp = 1;
__global__ __launch_bounds__(kBlock) void cg_xp_kernel(int64_t n, const SolverState *st, long long my_iteration,
                                                       double *__restrict__ x, double *__restrict__ p,
                                                       const double *__restrict__ r, int nt, int reverse) {
  if (st->iteration < my_iteration) return;  // enqueued past convergence: this iteration never ran
  const unsigned bx = reverse ? gridDim.x - 1 - blockIdx.x : blockIdx.x;
  const bool update_p = !st->done && r != nullptr;  // (r == null: the tail of the fused loop -- only x is left to update)
  const double alpha = st->s[S_ALPHA], beta = st->s[S_BETA];
  const int64_t n2 = n >> 1;
  double2v *x2 = reinterpret_cast<double2v *>(x), *p2 = reinterpret_cast<double2v *>(p);
  const double2v *r2 = reinterpret_cast<const double2v *>(r);
  nt_dispatch(nt, [&](auto nt) {
  for (int64_t base = (int64_t)bx * (kBlock * kUnrollXp) + threadIdx.x; base < n2;
       base += (int64_t)gridDim.x * (kBlock * kUnrollXp)) {
    double2v vx[kUnrollXp], vp[kUnrollXp], vr[kUnrollXp];
#pragma unroll
    for (int u = 0; u < kUnrollXp; ++u) {
      const int64_t i = base + u * kBlock;
      if (i < n2) {
        vx[u] = ldv(x2 + i, nt), vp[u] = ldv(p2 + i, nt);
        if (update_p) vr[u] = ldv(r2 + i, nt);
      }
    }
#pragma unroll
    for (int u = 0; u < kUnrollXp; ++u) {
      const int64_t i = base + u * kBlock;
      if (i < n2) {
        vx[u] += alpha * vp[u];
        stv(x2 + i, vx[u], nt);
        if (update_p) stv(p2 + i, vr[u] + beta * vp[u], nt);
      }
    }
  }
  });
  if ((n & 1) && bx == 0 && threadIdx.x == 0) {
    const int64_t i = n - 1;
    x[i] += alpha * p[i];
    if (update_p) p[i] = r[i] + beta * p[i];
  }
}
static inline int xp_blocks(int64_t n) {
  int64_t b = ((n >> 1) + kBlock * kUnrollXp - 1) / (kBlock * kUnrollXp);
  return (int)(b < 1 ? 1 : (b > 131072 ? 131072 : b));
}


// Which road the loop takes, decided once per solve.
struct CgRoads {
  // (r: the init apply; p: init_residual's copy; z: the first SpMV -- all before any read; the fused step's second p)
  bool may_fuse_step;
  // Reductions that finish inside the kernels producing their partials (ticket_device.hpp), one rank: an iteration
  // is then three launches -- SpMV (+ <p,z>), cg_r (+ <r,r>, beta, the convergence rule), cg_xp.
  // (on the peer-window transport too: the block that finishes a reduction exchanges its sum with the other ranks itself)
  bool ipc, tick;
  // (<p,z> inside the SpMV only where it replaces a whole final-pass launch: with more per-wave partials than one
  // pass folds, the first pass + the fold inside cg_r cost what the ticket tail would add to the SpMV)
  bool tick_spmv;
  // The fused step (one rank, tiled format-4 operator): iteration k's SpMV kernel first ENDS iteration k - 1 --
  // x += alpha p, p' = r + beta p -- on the rows it loads anyway and applies the operator to p': x and p are no longer
  // streamed by a kernel of their own (cg_xp).  p ping-pongs between two vectors (a tile's old p is another tile's
  // halo).  Two launches + the small first pass per iteration (two where the plane march folds <p,z> itself, option
  // cg_pz_fold -- where, option cg_rr_fold, the plane march also ends at the group sums of <r,r> and the NEXT step kernel
  // runs the scalar step; behind the loop cg_rr_finish_kernel does); the last iteration's x update runs behind the loop.
  // (on the peer-window transport too: the marching launch also sends p' of the boundary rows, spmv.hip)
  // (on RCCL too, round 4: there the reductions keep their all-reduce between partials and step -- no tickets --, the
  //  step kernel reads alpha, beta and the iteration counter from the slab exactly as cg_xp_kernel does)
  bool rccl, fuse_step;
  // RCCL: the local sums still finish inside the kernels that produce them (tickets) -- the library all-reduce and the
  // scalar step follow as launches of their own; two small launches per iteration fewer than partials + final pass
  bool rtick;
  // (the residual recompute: from iteration 1 on, the step kernel stores no z and r -= alpha z recomputes it; iteration
  //  0's plain apply writes z for cg_r_kernel)
  bool r_march;
  // (... marching over planes where the lattice allows, cg_r_planes_kernel; else cg_r_kernel's grid with gathers)
  bool r_planes;
  ResidualPlanesArgs planes_args;
  int planes_blocks = 0;
};
static CgRoads cg_roads(Driver &d, int nbv) {
  storm_hip_ctx *c = d.c;
  CgRoads w;
  w.may_fuse_step = c->opt_cg_fuse != 0 && spmv_can_fuse_cg(d.op);
  w.ipc = c->comm != nullptr && comm_ipc_next(c, &d.ipc_w);
  w.tick = c->opt_ticket_reduce != 0 && (c->comm == nullptr || w.ipc) && nbv <= kTicketGroup * kTicketMaxGroups;
  w.tick_spmv = w.tick && !w.ipc && 4 * (int64_t)spmv_grid_blocks(d.op) <= kSinglePassPartials;
  w.rccl = c->comm != nullptr && comm_is_rccl(c);
  w.fuse_step = w.may_fuse_step && (w.rccl ? true : ((c->comm == nullptr || w.ipc) && w.tick && !w.tick_spmv));
  w.rtick = w.rccl && w.fuse_step && c->opt_ticket_reduce != 0 && c->opt_rccl_ticket != 0 && nbv <= kTicketGroup * kTicketMaxGroups;
  w.r_march = w.fuse_step && !w.rccl && cg_r_recompute_applies(d.op, w.tick);
  w.r_planes = w.r_march && cg_r_planes_geometry(d.op, &w.planes_args, &w.planes_blocks);
  if (w.fuse_step) ++c->n_cg_fused_steps;
  if (w.r_march) ++c->n_cg_residual_marches;
  if (w.r_planes) ++c->n_cg_residual_plane_marches;
  return w;
}

static int solve_cg_body(const FusedSolveArgs &args) {
  const storm_hip_op *op = args.op;
  const double *b = args.b->d;
  double *x = args.x->d;
  Driver d;
  STORM_TRY(prepare_state(args, &d));
  storm_hip_ctx *c = d.c;
  const int64_t n = d.n;
  VecPool pool;
  if (res_eligible(op, false)) {  // a lattice operator that fits the chip's registers: one persistent kernel, a box per block (resident.hip)
    bool taken = false;
    STORM_TRY(res_solve(false, op, d.alpha, d.beta, b, x, nullptr, c->d_state, &taken));
    if (taken) return ++c->n_resident_solves, collect(d, args, 1);
  }
  if (cg_latency_eligible(op)) {  // a small operator: the whole solve as one cooperative kernel (latency.hip)
    STORM_TRY(pool.make(args.x, 2));  // zero-filled: the kernel relies on that for the first direction
    bool taken = false;
    STORM_TRY(cg_latency_solve(op, d.alpha, d.beta, b, x, pool.v[0]->d, pool.v[1]->d, c->d_state, &taken));
    if (taken) return ++c->n_latency_solves, collect(d, args, 1);
    // (the cooperative kernel could not be launched: the throughput path below, noted in result->path_fallback)
  }
  ++c->n_throughput_solves;
  const size_t v0 = pool.v.size();
  const int nbv = stream_blocks(n);
  const CgRoads road = cg_roads(d, nbv);
  STORM_TRY(pool.make(args.x, road.may_fuse_step ? 4 : 3, false));
  // (which of the four work vectors -- consecutive slots of the context's arena -- plays p, r, z and the second direction
  //  vector is a matter of placement: the 24 assignments at 256^3 gave 4 505 - 4 570 it/s, profiles/r05z_roles.txt)
  static const int kRolesFused[4] = {1, 2, 0, 3}, kRolesPlain[3] = {0, 1, 2};
  const int *role = road.may_fuse_step ? kRolesFused : kRolesPlain;
  double *p = pool.v[v0 + role[0]]->d, *r = pool.v[v0 + role[1]]->d, *z = pool.v[v0 + role[2]]->d;
  double *p_alt = road.fuse_step ? pool.v[v0 + role[3]]->d : nullptr;

  // init: r = b - A x; p = r; gamma = <r,r>          SolverCg.hpp:75-85
  int nb = 0;
  STORM_TRY(d.apply(x, r, &nb, {}, false));
  STORM_TRY(d.init_residual(r, b, p));
  STORM_TRY(d.finish(nbv, 1, S_GAMMA, STEP_CG_INIT, true));
  // One iteration's launches (the scalars live in the slab; only the iteration index varies).
  int64_t cur_it = 0;
  // Sweep directions.  The 256 MB Infinity Cache still holds the END of what the previous kernel streamed (a read
  // served from it runs ~18 % faster than from HBM, tools/mall_probe.hip), so every kernel starts where its
  // predecessor stopped: iteration k even -- SpMV forward, cg_r backward, cg_xp forward; k odd -- the mirror image.
  // Blocks keep their rows and their partial slots: the same bits either way.  (Per rank: with a communicator too.)
  const int nt_stream = stream_nt(c, n);
  int64_t last_enqueued = -1;
  bool pz_fold_counted = false, rr_fold_counted = false;
  // (option cg_rr_fold: the last enqueued residual kernel ended at its group sums -- the state is one STEP_CG_RR behind)
  bool rr_pending = false;
  const int rr_ng = road.r_planes ? (int)(((int64_t)road.planes_args.planes * road.planes_args.runs_per_plane + kTicketGroup - 1) / kTicketGroup) : 0;
  auto enqueue_iteration = [&]() -> int {
    const int q = road.fuse_step ? 0 : (int)(cur_it & 1);  // (fused: the step kernel forward, cg_r backward, always)
    // z = A p, <p,z>                                  SolverCg.hpp:96-97
    c->spmv_reverse = q;
    int pz_done = 0;  // <p,z> finished inside the SpMV kernel (tickets): cg_r reads it from the slab
    int st_apply;
    const bool r_march_now = road.r_march && cur_it > 0;
    if (road.fuse_step && cur_it > 0) {
      // ends iteration cur_it - 1 (SolverCg.hpp:98, :123) -- and, where its residual kernel left the group sums, its scalar step
      const CgStep step{(long long)cur_it, x, r, p_alt, rr_pending ? c->d_ticket_sums : nullptr, rr_ng};
      rr_pending = false;
      // (<p,z>: per-wave partials for the plane march's fold or the final pass below -- finishing it inside the marching
      //  kernel by tickets was measured for this loop and dropped; the host loop's fused step, lazy.hip, does finish it there: one launch less
      //  in front of a host wait)
      st_apply = d.apply(p, r_march_now ? nullptr : z, &nb, {.w = p, .ticketed = &pz_done}, true, &step);
      std::swap(p, p_alt);
    } else {
      st_apply = d.apply(p, z, &nb, {.w = p, .out0 = road.tick_spmv ? (int)S_PZ : -1, .ticketed = &pz_done});
    }
    last_enqueued = cur_it;
    c->spmv_reverse = 0;
    STORM_TRY(st_apply);
    // (tickets on one rank only where one pass does not fold the partials; without them the fold inside cg_r_kernel)
    const bool tickets_now = road.tick && (nb > kSinglePassPartials || road.ipc);
    const Driver::Road allow = road.rtick ? Driver::ROAD_TICKETS_RCCL
                                          : !tickets_now ? Driver::ROAD_PLAIN : road.ipc ? Driver::ROAD_TICKETS_IPC : Driver::ROAD_TICKETS;
    Driver::Road ran;
    const double *pz_partials = nullptr, *const pz_with[1] = {z};
    // (option cg_pz_fold: the plane march folds the step kernel's nb partials itself, under its first loads -- no launch in
    //  between; its own <r,r> slots then go behind them.  One rank without tickets for <p,z>: r_march implies the first)
    const int64_t rr_slots = road.r_planes ? (int64_t)road.planes_args.planes * road.planes_args.runs_per_plane : 0;
    const bool pz_fold_now = c->opt_cg_pz_fold != 0 && r_march_now && road.r_planes && c->comm == nullptr && !tickets_now &&
                             !pz_done && nb > 0 && nb <= kSinglePassPartials && nb + rr_slots <= c->partials_capacity;
    if (pz_fold_now && !pz_fold_counted) ++c->n_cg_pz_consumer_folds, pz_fold_counted = true;
    if (!pz_fold_now) STORM_TRY(d.finish_dots(pz_done, nb, 1, S_PZ, p, pz_with, allow, STEP_NONE, &ran, &pz_partials));
    // r -= alpha z; gamma = <r,r>                     SolverCg.hpp:97,99,115
    // (option cg_rr_fold, on the same road: the kernel ends at its group sums where one batch holds them; the next
    //  iteration's step kernel -- the marching one: r_march -- or the launch behind the loop takes it from there)
    const bool rr_fold_now = pz_fold_now && c->opt_cg_rr_fold != 0 && rr_ng >= 1 && rr_ng <= (int)kTicketFoldBatch1;
    if (rr_fold_now && !rr_fold_counted) ++c->n_cg_rr_consumer_folds, rr_fold_counted = true;
    if (pz_fold_now) {
      STORM_TRY(cg_r_planes_run(op, road.planes_args, road.planes_blocks, host_scal(d.alpha), host_scal(d.beta), p, d.st, r, c->d_partials,
                                nb, 1 - q, c->d_partials + nb, rr_fold_now ? (long long)(cur_it + 1) : 0));
      rr_pending = rr_fold_now;
    } else if (r_march_now && road.r_planes) {
      STORM_TRY(cg_r_planes_run(op, road.planes_args, road.planes_blocks, host_scal(d.alpha), host_scal(d.beta), p, d.st, r, pz_partials,
                                (int)kStage2, 1 - q, c->d_partials));
    } else if (r_march_now) {
      STORM_TRY(cg_r_recompute_run(op, nbv, host_scal(d.alpha), host_scal(d.beta), p, d.st, r, pz_partials, (int)kStage2, 1 - q));
    } else {
      hipLaunchKernelGGL(cg_r_kernel, dim3(nbv), dim3(kBlock), 0, c->stream, n, d.st, r, z, c->d_partials, nt_stream, pz_partials,
                         (int)kStage2, 1 - q, (road.tick || road.rtick) ? d.tickets() : TicketArgs{}, d.ipc_w,
                         road.rtick ? 2 : (int)(road.ipc && road.tick));
      HIP_TRY(hipGetLastError());
    }
    if (road.rtick) {
      STORM_TRY(comm_allreduce_sum(c, d.slot(S_GAMMA_NEW), 1));
      STORM_TRY(d.step(STEP_CG_RR));
    } else if (!road.tick) {
      STORM_TRY(d.finish(nbv, 1, S_GAMMA_NEW, STEP_CG_RR));
    }
    if (road.tick && c->opt_ticket_verify > 0 && cur_it % c->opt_ticket_verify == 0) {
      // <p, z> as the SpMV / first pass left it, <r, r> as cg_r's last block did (it has advanced the counter already)
      STORM_TRY(d.verify(p, z, nullptr, S_PZ, -1, (long long)(cur_it + 1)));
      STORM_TRY(d.verify(r, r, nullptr, S_GAMMA, -1, (long long)(cur_it + 1)));
    }
    if (road.fuse_step) return STORM_HIP_OK;  // (the next iteration's step kernel, or the tail below, ends this one)
    // (RCCL, no fused step: the halo of the new direction leaves before cg_xp forms it, comm.hip)
    if (road.rccl && c->opt_rccl_early_halo != 0 && op->halo.n_nbrs > 0)
      STORM_TRY(comm_halo_exchange_begin_formed(op, 2, r, p, nullptr, d.slot(S_BETA), nullptr, p));
    // x += alpha p; p = r + beta p                    SolverCg.hpp:98,123
    hipLaunchKernelGGL(cg_xp_kernel, dim3(xp_blocks(n)), dim3(kBlock), 0, c->stream, n, d.st, (long long)(cur_it + 1), x, p, r,
                       nt_stream, q);
    HIP_TRY(hipGetLastError());
    return STORM_HIP_OK;
  };
  for (int64_t it = 0; it < args.params->num_iterations; ++it) {
    cur_it = it;
    STORM_TRY(enqueue_iteration());
    bool stop = false;
    STORM_TRY(post_and_poll(d, it, &stop));
    if (stop) break;
  }
  if (rr_pending) {  // the scalar step of the last enqueued iteration: no step kernel behind it
    hipLaunchKernelGGL(cg_rr_finish_kernel, dim3(1), dim3(kWave), 0, c->stream, d.st, c->d_ticket_sums, rr_ng, (long long)(last_enqueued + 1));
    HIP_TRY(hipGetLastError());
  }
  if (road.fuse_step && last_enqueued >= 0) {
    // the x update of the last enqueued iteration (a no-op when that iteration never ran: the step kernel of the
    // iteration behind the converging one has applied it already)
    hipLaunchKernelGGL(cg_xp_kernel, dim3(xp_blocks(n)), dim3(kBlock), 0, c->stream, n, d.st, (long long)(last_enqueued + 1), x, p,
                       (const double *)nullptr, nt_stream, 0);
    HIP_TRY(hipGetLastError());
  }
  comm_forget_prebegun(c);
  return collect(d, args, 1);
}

// CG for the two-stage operator A = beta2 I + alpha2 M (beta1 I + alpha1 M) as one cooperative kernel (latency.hip,
// cg2_latency_kernel), under the rules of the single-stage solve above.  *taken = false: the caller runs its own loop.
int cg2_latency_try(const storm_hip_op *op, double alpha1, double beta1, double alpha2, double beta2, const storm_hip_vec *b,
                    storm_hip_vec *x, const storm_hip_solver_params *params, storm_hip_solver_result *result, double *history,
                    bool *taken) {
  *taken = false;
  if (!cg_latency_eligible(op)) return STORM_HIP_OK;
  storm_hip_ctx *c = op->ctx;
  const FusedSolveArgs args{op, alpha1, beta1, b, x, params, result, history, nullptr};
  Driver d;
  STORM_TRY(prepare_state(args, &d));
  VecPool pool;
  int st = pool.make(x, 3);  // p, r, t; zero-filled: the kernel relies on that for the first direction
  if (st == STORM_HIP_OK) {
    double *const work[3] = {pool.v[0]->d, pool.v[1]->d, pool.v[2]->d};
    st = cg2_latency_solve(op, alpha1, beta1, alpha2, beta2, b->d, x->d, work, c->d_state, taken);
  }
  if (st == STORM_HIP_OK && *taken) return ++c->n_latency_solves, collect(d, args, 1);  // (one apply is both stages)
  if (d.d_history) (void)hipFree(d.d_history), d.d_history = nullptr;
  return st;
}

// CG with a diagonal or a Chebyshev preconditioner as one cooperative kernel (latency.hip, pcg_latency_kernel), under the same
// rules.  The counts are the engine's for the same solve: one operator and one preconditioner apply for the init and per iteration.
int pcg_latency_try(const storm_hip_op *op, double alpha, double beta, const storm_hip_vec *diag, const storm_hip_cheb *cheb,
                    const storm_hip_vec *b, storm_hip_vec *x, const storm_hip_solver_params *params, storm_hip_solver_result *result,
                    double *history, int64_t *pre_applies, bool *taken) {
  *taken = false;
  if (!cg_latency_eligible(op)) return STORM_HIP_OK;
  storm_hip_ctx *c = op->ctx;
  const FusedSolveArgs args{op, alpha, beta, b, x, params, result, history, nullptr};
  Driver d;
  STORM_TRY(prepare_state(args, &d));
  VecPool pool;
  int st = pool.make(x, cheb != nullptr ? 4 : 2);  // p, u, d0, d1; zero-filled: the kernel relies on that for the first direction
  if (st == STORM_HIP_OK) {
    double *const work[4] = {pool.v[0]->d, pool.v[1]->d, cheb != nullptr ? pool.v[2]->d : nullptr, cheb != nullptr ? pool.v[3]->d : nullptr};
    st = pcg_latency_solve(op, alpha, beta, b->d, x->d, diag != nullptr ? diag->d : nullptr, cheb, work, c->d_state, taken);
  }
  if (st == STORM_HIP_OK && *taken) {
    ++c->n_latency_solves, ++c->n_latency_pre_solves;
    st = collect(d, args, 1);
    if (st == STORM_HIP_OK && pre_applies) *pre_applies = 1 + result->iterations;
    return st;
  }
  if (d.d_history) (void)hipFree(d.d_history), d.d_history = nullptr;
  return st;
}

}  // namespace storm

extern "C" int storm_hip_solve_cg(const storm_hip_op *op, double alpha, double beta, const storm_hip_vec *b, storm_hip_vec *x,
                                  const storm_hip_solver_params *params, storm_hip_solver_result *result, double *history) {
  if (op) STORM_TRY(storm::lazy_sync(op->ctx));
  return storm::fused_solve(storm::FusedSolveArgs{op, alpha, beta, b, x, params, result, history, &storm::solve_cg_body});
}
