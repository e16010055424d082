// The smoothed-aggregation multigrid preconditioner (storm_hip_amg_*): what the host setup (amg_setup.hip), the device
// object (amg.hip) and the engine's preconditioner slot (krylov_*.hip) share.  Recipe: include/storm_hip.h.
#pragma once

#include <vector>

#include "common.hpp"

namespace storm {

struct AmgCsr {  // rows sorted by column, no duplicates
  int64_t n_rows = 0, n_cols = 0;
  std::vector<int64_t> ptr;
  std::vector<int> col;
  std::vector<double> val;
  int64_t nnz() const { return (int64_t)col.size(); }
};

struct AmgHostLevel {
  AmgCsr A;              // explicit diagonal, exact zeros dropped
  std::vector<int> agg;  // aggregate of every row (empty on the coarsest level)
  int64_t n_agg = 0;
  AmgCsr P, R;           // prolongator to this level from the next, and its explicit transpose
  std::vector<uint8_t> strong;  // one byte per entry of A.col: 1 where the pair is strong (empty on the coarsest level)
};

constexpr int kAmgMaxCoarse = 1024;  // rows of a dense coarsest level

// One slice of 64 rows of a transfer operator: [col W x 64 int32][val W x 64 fp64], W the slice's widest row; padding has
// weight 0 and column 0.  off[s] is the slice's byte offset.
struct AmgTransferImage {
  int64_t n_rows = 0, n_cols = 0, n_slices = 0, slots = 0, nnz = 0;
  std::vector<int64_t> off;
  std::vector<char> pack;
};
int amg_pack_transfer(const AmgCsr &T, AmgTransferImage *img);
int amg_dense_inverse(const AmgCsr &A, std::vector<double> *inv_out);  // step 7 (amg_setup.hip)
// N3 of a null-space hierarchy instead of step 7: Ainv = Pi (A + (s / n) 1 1^T)^-1 Pi, s = max a_ii (0 for one row)
int amg_coarse_nullspace(const AmgCsr &A, std::vector<double> *inv_out, double *shift_out);

// What a refresh of level l needs beside the structural hierarchy, built once on the host (amg_setup.hip, no device):
// r_of[k]: the entry of P_l that entry k of R_l = P_l^T carries; p_slot / r_slot: for every slot of the transfer records of
// P_l / R_l (slot k x 64 + lane behind the slots of the slices before) the entry of P_l it carries, -1 for padding; AP: the
// structural pattern of A_l P_l.
struct AmgRefreshMaps {
  std::vector<int> r_of, p_slot, r_slot;
  AmgCsr AP;
};
int amg_refresh_maps(const storm_hip_amg_hierarchy &h, size_t l, AmgRefreshMaps *m);

}  // namespace storm

struct storm_hip_amg_hierarchy {
  storm_hip_amg_params params;
  std::vector<storm::AmgHostLevel> levels;
  std::vector<double> ainv;  // the coarsest level's inverse, row-major
  double setup_seconds = 0.0;
  bool structural = false;  // storm_hip_amg_setup_csr_structural: no pattern depends on a value
  bool nullspace = false;   // storm_hip_amg_setup_csr_nullspace: the constants are A's kernel (N1 - N3)
  double coarse_shift = 0.0;  // N3's s (0 on a plain hierarchy and on a one-row coarsest level)
};

struct storm_hip_amg {
  storm_hip_ctx *ctx = nullptr;
  const storm_hip_op *op = nullptr;  // level 0's operator (not owned)
  double alpha = 0.0, beta = 0.0;
  storm_hip_amg_hierarchy *hier = nullptr;
  struct Transfer {
    int64_t n_rows = 0, n_slices = 0;
    int64_t *d_off = nullptr;
    char *d_pack = nullptr;
  };
  struct Level {
    const storm_hip_op *op = nullptr;
    storm_hip_op *own_op = nullptr;  // levels >= 1
    double alpha = 1.0, beta = 0.0;
    int64_t n = 0;
    storm_hip_vec *dinv = nullptr;
    storm_hip_cheb *cheb = nullptr;  // null with the Jacobi smoother
    double lmax = 0.0, sigma = 0.0;  // Gershgorin's bound of diag(s) A_l; the Jacobi smoother's 2 omega / lmax
    Transfer P, R;
    storm_hip_vec *r = nullptr, *z = nullptr;  // levels >= 1: the restricted residual and the correction
    storm_hip_vec *t = nullptr, *e = nullptr;
  };
  std::vector<Level> levels;
  // storm_hip_amg_create_smoother: 0 Chebyshev, 1 damped Jacobi sweeps (the object then holds no storm_hip_cheb)
  int smoother_kind = 0, jacobi_sweeps = 2;
  double jacobi_omega = 2.0 / 3.0;
  double *d_ainv = nullptr;
  int64_t n_coarse = 0;
  int64_t device_bytes = 0, transfer_slots = 0, transfer_nnz = 0;
  double upload_seconds = 0.0;
  // storm_hip_amg_create_refreshable (amg_refresh.hip): per level the frozen structure and the value arrays of a refresh.
  // All of it is counted in refresh_bytes (and in device_bytes).
  struct RefreshLevel {
    int64_t n = 0, nnz_a = 0, nnz_p = 0, nnz_ap = 0, p_slots = 0, r_slots = 0;
    int64_t *d_a_ptr = nullptr;   // A_l as CSR: [n + 1], [nnz_a], [nnz_a]; the strong mask [nnz_a]; the diagonal's entry [n]
    int *d_a_col = nullptr;
    double *d_a_val = nullptr;
    uint8_t *d_strong = nullptr;
    int *d_a_diag = nullptr;
    int *d_agg = nullptr;         // [n]
    double *d_df = nullptr;       // [n] the filtered diagonal
    double *d_wave_max = nullptr; // [slices of n] the wavefronts' maxima of the ratio
    int64_t *d_p_ptr = nullptr;   // P_l as CSR
    int *d_p_col = nullptr;
    double *d_p_val = nullptr;
    int64_t *d_r_ptr = nullptr;   // R_l's pattern and the entry of P_l behind each of its entries
    int *d_r_col = nullptr, *d_r_of = nullptr;
    int64_t *d_ap_ptr = nullptr;  // A_l P_l
    int *d_ap_col = nullptr;
    double *d_ap_val = nullptr;
    int *d_p_slot = nullptr, *d_r_slot = nullptr;  // the transfer records' slot -> entry of P_l maps
    // level 0: the records' slot -> entry of A_0 maps (-1: padding, -2: a real slot on the row's own column) and the row ->
    // tail row map (null without a CSR tail)
    int *d_slot_ent = nullptr, *d_tail_ent = nullptr, *d_tail_of = nullptr;
  };
  std::vector<RefreshLevel> refresh;  // empty: a plain object
  int64_t refresh_bytes = 0;
  double *d_scalars = nullptr;  // [0]: the folded maximum of a level's ratio
  int *d_bad = nullptr;         // the lowest row whose filtered diagonal is zero or non-finite (INT32_MAX: none)
  int invalid = 0;              // a refresh failed: apply and solves return STORM_HIP_E_INVALID until one succeeds
  // storm_hip_amg_create_nullspace: B = Pi V Pi.  The projected residual, the two means (d_mu[0]: of r, or of a projected
  // vector; d_mu[1]: of z) and the object's own ticket buffers (the context's may hold a solver's partials across an apply).
  int nullspace = 0;
  storm_hip_vec *rp = nullptr;
  double *d_mu = nullptr;
  int *d_mean_cnt = nullptr;
  double *d_mean_part1 = nullptr, *d_mean_part2 = nullptr;
  // The cooperative tail (amg_tail.hip, option amg_tail): the level and phase tables of the kernel that runs the cycle from
  // `built_level` down and back, on the device; rebuilt when the start level changes, dropped by a refresh (the coefficients
  // move).  `at`: the level at which the CURRENT apply hands over to the kernel (-1: none), set by storm_hip_amg_apply.
  struct Tail {
    int at = -1;
    int built_level = -1, blocks = 0, barriers = 0, n_phases = 0;
    char *d_table = nullptr;
    size_t table_bytes = 0;
    const char *top_pack32 = nullptr;  // the start level's companion records as built (level 0's may be dropped and built again)
  };
  mutable Tail tail;
};

namespace storm {
// amg.hip, shared with amg_refresh.hip
int amg_decode(const storm_hip_op *op, double alpha, double beta, bool structural, std::vector<int64_t> *ptr, std::vector<int64_t> *col,
               std::vector<double> *val);
int amg_build_device(storm_hip_amg *h, storm_hip_op *op0);
int amg_create_checks(const storm_hip_op *op, double alpha, double beta, const char *who);
void amg_refresh_free(storm_hip_amg *h);  // amg_refresh.hip
// d = it (s .* r): cheb_d0_kernel<JACOBI> (precond_cheb.hip), the start of a Jacobi sweep from the zero guess
int cheb_scaled_start(storm_hip_ctx *c, int64_t n, double inv_theta, const double *r, const double *s, double *d);
// a level whose residual (and smoother) runs on fp64 records without a CSR tail or a compact format: option amg_fused on
bool amg_residual_fused(const storm_hip_amg *h, const storm_hip_op *op);
// amg_tail.hip.  amg_tail_level: the first level with at most amg_tail_rows rows from which every level is eligible (it may be
// the coarsest, which alone is no tail), -1: none.  amg_tail_choose: the level at which an apply hands over to the kernel
// under the context's options now (-1: none).  amg_tail_run: levels l .. coarsest .. l in one launch; *taken = false: refused
// or not launchable, nothing ran, the caller goes on with the launches.
int amg_tail_level(const storm_hip_amg *h);
int amg_tail_choose(const storm_hip_amg *h);
int amg_tail_run(const storm_hip_amg *h, size_t l, const storm_hip_vec *r, storm_hip_vec *z, bool *taken);
int amg_tail_get(const storm_hip_amg *h, const char *key, double *value, bool *known);
void amg_tail_invalidate(const storm_hip_amg *h);  // the tables are built again by the next apply
void amg_tail_free(storm_hip_amg *h);
}  // namespace storm
