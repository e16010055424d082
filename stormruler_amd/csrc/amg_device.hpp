// The per-row arithmetic of the Chebyshev smoother (precond_cheb.hip) and of the multigrid cycle (amg.hip), shared with the
// cooperative tail of the cycle (amg_tail.hip): ONE definition of every statement that rounds, so that a level run by the tail
// kernel gives the bits of the launches it replaces.  The kernels differ in how a row's operands are loaded and stored (plain,
// non-temporal, or coherently across the blocks of one launch: CO) and in which wavefront takes which slice -- never in a sum.
#pragma once
#include "blas1_device.hpp"
#include "sell_device.hpp"
#include "wave_device.hpp"

namespace storm {

// (beta x + alpha M x)_row on the records of the row's slice: row_sum_any, then sell_row_result.  xi: the row's own x.
// X: the gathered vector's element type (double; float for the fp32 vectors of mixed_cg.hip, widened where they are loaded).
template <bool NT, class R, bool CO = false, class X = double>
__device__ __forceinline__ double sell_row_apply(const SellArgs &A, int64_t slice, int lane, const X *__restrict__ x, double xi,
                                                 double alpha, double beta) {
  int64_t base;
  int width;
  if (A.uniform_width > 0) {
    width = A.uniform_width;
    base = slice * (int64_t)(R::kExt + R::kSlot * width);
  } else {
    base = A.slice_off[slice];
    width = (int)((A.slice_off[slice + 1] - base - R::kExt) / R::kSlot);
  }
  const char *rec = A.pack + base;
  const double ext = R::template ext<NT>(rec, lane);
  const double xi1[1] = {xi};
  double acc1[1];
  row_sum_any<NT, 1, R, CO, X>(rec, width, lane, x, xi1, acc1);
  return sell_row_result(false, 0.0, beta, xi, alpha, acc1[0], ext);
}

// d_0 = it (s .* r)  (JACOBI)  /  it r: vmul's product, then the one-term statement's.
template <bool JACOBI>
__device__ __forceinline__ double cheb_d0_value(double inv_theta, double r, double s) {
  double t = r;
  if (JACOBI) t = s * t;
  return inv_theta * t;
}

// One Chebyshev step of a row, t = (A d)_row:  res' = res - t;  d' = c1 d + c2 (s .* res');  z' = z + d'  (FIRST: z' = d + d').
struct ChebRow {
  double rn, dn, zn;
};
template <bool JACOBI, bool FIRST>
__device__ __forceinline__ ChebRow cheb_step_row(double t, double ri, double si, double xi, double zi, double c1, double c2) {
  ChebRow o;
  o.rn = ri - t;
  double w = o.rn;
  if (JACOBI) w = si * o.rn;
  o.dn = axpbz_value(c1, xi, c2, w);
  o.zn = FIRST ? xi + o.dn : o.dn + zi;
  return o;
}

// t = r - A z of a row, az = (A z)_row: axpbz(t, 1, r, -1, t), whose multiplications by +-1 are exact.
__device__ __forceinline__ double amg_residual_value(double ri, double az) { return ri - az; }

// One damped-Jacobi sweep of a row: the residual, vmul(t, s, t), then axpbz(z', sigma, t, 1, z) -- the axpy statement's kernel.
__device__ __forceinline__ double amg_jacobi_value(double ri, double az, double si, double sigma, double zi) {
  const double tn = amg_residual_value(ri, az);
  const double w = si * tn;
  return axpbz_value(sigma, w, 1.0, zi);
}

// z = z + e of a row: storm_hip_axpy(z, 1, e), which is axpbz(z, 1, e, 1, z).
__device__ __forceinline__ double amg_axpy_value(double ei, double zi) { return axpbz_value(1.0, ei, 1.0, zi); }

// (T x)_row on the transfer records [col W x 64 int32][val W x 64 fp64] of the row's slice, acc = fma(w_k, x[c_k], acc) in slot
// order; ADD: y_row + that.  (padding: column 0, weight 0 -- inside x for every lane of the slice)
template <bool ADD, bool CO = false>
__device__ __forceinline__ double amg_transfer_row(const char *__restrict__ pack, const int64_t *__restrict__ off, int64_t slice,
                                                   int lane, const double *__restrict__ x, double yi) {
  const int64_t base = off[slice];
  const int width = (int)((off[slice + 1] - base) / (kWave * 12));
  const int *__restrict__ cp = reinterpret_cast<const int *>(pack + base) + lane;
  const double *__restrict__ vp = reinterpret_cast<const double *>(pack + base + (int64_t)width * (kWave * 4)) + lane;
  double acc = 0.0;
#pragma unroll 4  // (the loads of four slots in flight; the sum stays in slot order)
  for (int k = 0; k < width; ++k) {
    const int c = __builtin_nontemporal_load(cp + k * kWave);
    const double w = __builtin_nontemporal_load(vp + k * kWave);
    double xc[1];
    ld_cols<1, CO>(x, c, xc);
    acc = fma(w, xc[0], acc);
  }
  return ADD ? yi + acc : acc;
}

// (Ainv r)_row, dense: lane j takes columns j, j + 64, ... by fma, then the wavefront's sum -- the total in lane 0.
template <bool CO = false>
__device__ __forceinline__ double amg_coarse_row(const double *__restrict__ ainv, int64_t n, int64_t row, int lane,
                                                 const double *__restrict__ r) {
  const double *__restrict__ a = ainv + row * n;
  double acc = 0.0;
  for (int64_t j = lane; j < n; j += kWave) {
    double rj[1];
    ld_cols<1, CO>(r, (int)j, rj);
    acc = fma(a[j], rj[0], acc);
  }
  return wave_sum_down(acc);
}

}  // namespace storm
