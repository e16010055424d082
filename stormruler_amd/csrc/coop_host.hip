// The host side of every cooperative path -- kernels whose blocks are all resident and synchronise through memory: the
// latency solvers (latency.hip), the Gram-Schmidt chains (mgs_chain.hip), the resident lattice solves (resident.hip), the
// multigrid cycle's tail (amg_tail.hip):
// the occupancy question, the launch that may be refused, the look at the give-up flag of the bounded waits
// (coop_device.hpp co_bounded_wait) and the re-run of a solve whose kernel gave up.
#include <algorithm>

#include "common.hpp"
#include "coop_device.hpp"

namespace storm {

// Blocks of `fn` that fit a CU (0: the kernel cannot run with this much dynamic LDS), asked once PER CONTEXT: the answer --
// and the hipFuncAttributeMaxDynamicSharedMemorySize it needs -- belong to the device, a context is one device and one
// host thread (a process-wide static cache served a second device with the first one's answer and raced between threads).
int occupancy_cached(storm_hip_ctx *c, const void *fn, int threads, size_t dyn_lds) {
  const auto it = c->occupancy.find(fn);
  if (it != c->occupancy.end()) return it->second;
  int res = 0;
  if (dyn_lds == 0 || hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn_lds) == hipSuccess)
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&res, fn, threads, dyn_lds);
  (void)hipGetLastError();
  c->occupancy[fn] = res;
  return res;
}


// A cooperative launch that may be refused (too many blocks for what is resident, a device that does not take them):
// false = not launched, nothing ran, the error is cleared.
bool coop_launch(storm_hip_ctx *c, const void *fn, unsigned blocks, void **args, size_t dyn_lds, unsigned threads) {
  if (c->opt_coop_force_fail == 1) {
    c->coop_fallback = 1;
    return false;
  }
  // coop_plain: an ordinary launch of the same kernel.  These kernels synchronise through memory (no grid.sync()); what
  // they need is every block resident, which the callers size the grid for (<= one block per CU, a variant that fits) and
  // which holds on a device this process has to itself once the kernel in front has drained -- the runtime's cooperative
  // launch adds no more than that check, but runs on a queue of its own: 12-13 us of idle device in front of the kernel
  // AND in front of the next ordinary one (kernel trace, GMRES(30) at 128^3: two such gaps per inner iteration of 160 us).
  const hipError_t e = c->opt_coop_plain != 0 ? hipLaunchKernel(fn, dim3(blocks), dim3(threads), args, dyn_lds, c->stream)
                                              : hipLaunchCooperativeKernel(fn, dim3(blocks), dim3(threads), args, (unsigned)dyn_lds, c->stream);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    c->coop_fallback = 1;
    return false;
  }
  c->coop_ran = 1;
  return true;
}

// After a cooperative kernel has completed: did one of its waits give up?
int lat_check_gave_up(storm_hip_ctx *c) {
  if (!c->coop_ran) return STORM_HIP_OK;  // (no cooperative kernel since the last look: nothing to read back)
  int flag = 0;
  HIP_TRY(hipMemcpyAsync(&flag, c->d_lat_slots + (size_t)2 * 256 * kLatSlotStride, sizeof flag, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (c->opt_coop_force_fail == 2 && c->coop_ran && !c->coop_disabled) flag = 1;  // (test hook)
  c->coop_ran = 0;
  if (flag != 0) {
    (void)hipMemsetAsync(c->d_lat_slots + (size_t)2 * 256 * kLatSlotStride, 0, sizeof flag, c->stream);
    // The resident kernels carry their all-reduce / exchange sequence numbers from solve to solve in d_res_slots and
    // trust every block to leave with the same pair.  After a give-up that no longer holds (blocks left at different
    // checks, some never started): a later solve could find a slot or granule of the aborted one already at "its" number.
    // The stream is idle here: drop both buffers, the next resident solve allocates them zero-filled and restarts at 0.
    if (c->d_res_slots) (void)hipFree(c->d_res_slots);
    if (c->d_res_exch) (void)hipFree(c->d_res_exch);
    c->d_res_slots = nullptr, c->d_res_exch = nullptr, c->res_exch_rows = 0;
    set_error("cooperative kernel: a block waited 10 s for the others (is the device shared with another process's "
              "cooperative kernel?)");
    return kStatusCoopGaveUp;  // coop_solve_with_fallback re-runs the solve on the kernel-per-statement path
  }
  return STORM_HIP_OK;
}

// Run a solve that may use cooperative kernels; when one of them gave up, restore x and run it again without them.
int coop_solve_with_fallback(storm_hip_ctx *c, storm_hip_vec *x, int (*run)(void *), void *arg, int *fallback_out) {
  c->coop_fallback = 0, c->coop_ran = 0;
  // A cooperative kernel of an earlier solve gave up for real (a grid that did not become resident: a device shared
  // with another tenant, a CU mask): the next solves run without them instead of paying the bounded wait again --
  // 16 solves after the first give-up, twice as many after every further one.
  const bool backing_off = c->coop_skip > 0;
  if (backing_off) --c->coop_skip, c->coop_disabled = 1;
  const int64_t n_total = x->n_owned + x->n_halo;
  storm_hip_vec *x0 = nullptr;  // the start vector, kept for the re-run (pooled storage: no allocation, no stream wait per solve)
  const bool keep = c->comm == nullptr && c->coop_disabled == 0 &&
                    (c->opt_latency_path != 0 || c->opt_coop_mgs != 0 || c->opt_resident_path != 0 || c->opt_amg_tail != 0) &&
                    n_total > 0 && n_total <= ((int64_t)1 << 23);  // (no cooperative kernel takes more rows than that)
  if (keep) {
    STORM_TRY(vec_create_work_batch(x, 1, &x0));
    const hipError_t e = hipMemcpyAsync(x0->d, x->d, sizeof(double) * (size_t)n_total, hipMemcpyDeviceToDevice, c->stream);
    if (e != hipSuccess) {
      (void)storm_hip_vec_destroy(x0);
      HIP_TRY(e);
    }
  }
  int st = run(arg);
  if (st == kStatusCoopGaveUp && keep) {
    (void)hipMemcpyAsync(x->d, x0->d, sizeof(double) * (size_t)n_total, hipMemcpyDeviceToDevice, c->stream);
    c->coop_disabled = 1;
    st = run(arg);
    c->coop_disabled = 0;
    c->coop_fallback = 2;
    if (c->opt_coop_force_fail != 2) {  // (the test hook gives up once per solve: no back-off)
      c->coop_backoff = c->coop_backoff == 0 ? 16 : std::min<int64_t>(2 * c->coop_backoff, (int64_t)1 << 30);
      c->coop_skip = c->coop_backoff;
    }
  }
  if (backing_off) c->coop_disabled = 0;
  if (st == kStatusCoopGaveUp) st = STORM_HIP_E_HIP;  // (the message of lat_check_gave_up stands)
  if (x0) (void)storm_hip_vec_destroy(x0);
  if (fallback_out) *fallback_out = c->coop_fallback;
  return st;
}

}  // namespace storm
