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

}  // namespace storm

struct storm_hip_amg_hierarchy {
  storm_hip_amg_params params;
  std::vector<storm::AmgHostLevel> levels;
  std::vector<double> ainv;  // the coarsest level's inverse, row-major
  double setup_seconds = 0.0;
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
    storm_hip_cheb *cheb = nullptr;
    Transfer P, R;
    storm_hip_vec *r = nullptr, *z = nullptr;  // levels >= 1: the restricted residual and the correction
    storm_hip_vec *t = nullptr, *e = nullptr;
  };
  std::vector<Level> levels;
  double *d_ainv = nullptr;
  int64_t n_coarse = 0;
  int64_t device_bytes = 0, transfer_slots = 0, transfer_nnz = 0;
  double upload_seconds = 0.0;
};
