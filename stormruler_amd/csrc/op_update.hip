// Updatable face-weight operators: the weights of an operator created by storm_hip_op_create_from_face_weights_updatable
// rewritten on the device from vectors of per-face values, no host rebuild.  The host packer (op_pack.hip) left a source
// map beside the fp64 records: for every slot of every slice's val region and for every entry of the CSR tail the id
// 2 f + side of the face weight it carries (side 0: w_inner[f] in row inner[f]; side 1: w_outer[f] in row outer[f]; -1: a
// padding slot).  A refresh rewrites every byte of the ext and val regions and of tail_val from that map; columns, slice
// offsets and slice lists are not touched, so the operator is then the one a fresh create with those weights gives.
// Record layout: the header of spmv.hip.
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "op_layout.hpp"
#include "spmv_device.hpp"

namespace storm {

__device__ __forceinline__ double face_weight(int id, const double *__restrict__ w_inner, const double *__restrict__ w_outer) {
  return id < 0 ? 0.0 : ((id & 1) ? w_outer[id >> 1] : w_inner[id >> 1]);
}

template <bool NT>
__device__ __forceinline__ void st_pair(double2v *p, double2v v) {
  if (NT) __builtin_nontemporal_store(v, p);
  else *p = v;
}

// One wavefront per slice, four per block (the grid and the slot addressing of diag_sell_kernel).  Per slot pair a lane
// reads one int2 of source ids (512 B per wave instruction), gathers the two weights and stores one double2 (1 KiB per
// wave instruction); the 64 values of ext and of an odd last slot leave as double2 from the lower half of the wave.
// Streams 4 W + 8 W + 8 W + 16 bytes per row (ids, gathered weights, stored weights, diag_extra + ext).
template <bool NT>
__global__ __launch_bounds__(kBlock) void op_refresh_sell_kernel(char *__restrict__ pack, const int64_t *__restrict__ slice_off,
                                                                 const int *__restrict__ src, int64_t n_rows, int64_t n_slices,
                                                                 const double *__restrict__ w_inner,
                                                                 const double *__restrict__ w_outer,
                                                                 const double *__restrict__ diag_extra) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t s = (int64_t)blockIdx.x * (kBlock / kWave) + wave;
  if (s >= n_slices) return;
  const int64_t base = slice_off[s];
  const int width = (int)((slice_off[s + 1] - base - kExtBytes) / kSlotBytes);
  char *rec = pack + base;
  if (lane < kWave / 2) {  // ext: rows 64 s + 2 lane, + 1; rows past n_rows get 0
    const int64_t r = s * kWave + 2 * lane;
    double2v e;
    e.x = (diag_extra != nullptr && r < n_rows) ? diag_extra[r] : 0.0;
    e.y = (diag_extra != nullptr && r + 1 < n_rows) ? diag_extra[r + 1] : 0.0;
    st_pair<NT>(reinterpret_cast<double2v *>(rec) + lane, e);
  }
  const int *sp = src + (base - s * kExtBytes) / (kSlotBytes / kWave);  // the slots of the slices before this one
  double *val = reinterpret_cast<double *>(rec + kExtBytes + (int64_t)width * (kWave * 4));
  const int np2 = width >> 1;
  const int2v *ip = reinterpret_cast<const int2v *>(sp) + lane;
  double2v *vp = reinterpret_cast<double2v *>(val) + lane;
#pragma unroll 4
  for (int p = 0; p < np2; ++p) {  // (unrolled: the ids of four pairs, then their eight gathers, are in flight together)
    const int2v id = NT ? __builtin_nontemporal_load(ip + p * kWave) : ip[p * kWave];
    double2v v;
    v.x = face_weight(id.x, w_inner, w_outer);
    v.y = face_weight(id.y, w_inner, w_outer);
    st_pair<NT>(vp + p * kWave, v);
  }
  if ((width & 1) && lane < kWave / 2) {  // the odd last slot, column-major behind the pairs: rows 2 lane, + 1
    const int2v id = reinterpret_cast<const int2v *>(sp + np2 * 2 * kWave)[lane];
    double2v v;
    v.x = face_weight(id.x, w_inner, w_outer);
    v.y = face_weight(id.y, w_inner, w_outer);
    st_pair<NT>(reinterpret_cast<double2v *>(val + np2 * 2 * kWave) + lane, v);
  }
}

// One thread per entry of the CSR tail (no padding there: every id names a face).
__global__ __launch_bounds__(kBlock) void op_refresh_tail_kernel(int64_t tail_nnz, const int *__restrict__ tail_src,
                                                                 const double *__restrict__ w_inner,
                                                                 const double *__restrict__ w_outer,
                                                                 double *__restrict__ tail_val) {
  const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (k < tail_nnz) tail_val[k] = face_weight(tail_src[k], w_inner, w_outer);
}

// One thread per face: the cell field at the face's two cells (owned rows and the halo tail as it stands).
__global__ __launch_bounds__(kBlock) void cells_to_faces_kernel(int64_t n_faces, const int *__restrict__ inner,
                                                                const int *__restrict__ outer, const double *__restrict__ cell,
                                                                double *__restrict__ at_inner, double *__restrict__ at_outer) {
  const int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (f >= n_faces) return;
  if (at_inner) at_inner[f] = cell[inner[f]];
  if (at_outer) at_outer[f] = cell[outer[f]];
}

static int require_updatable(const storm_hip_op *op, const char *who) {
  if (!op->updatable)
    STORM_FAIL(STORM_HIP_E_UNSUPPORTED, "%s: the operator (%lld rows) was not created by storm_hip_op_create_from_face_weights_updatable",
               who, (long long)op->n_rows);
  return STORM_HIP_OK;
}

static int require_face_vector(const storm_hip_op *op, const storm_hip_vec *v, const char *who, const char *name) {
  STORM_REQUIRE(v->ctx == op->ctx, "%s: %s belongs to another context", who, name);
  STORM_REQUIRE(v->n_owned == op->n_faces && v->n_halo == 0, "%s: the operator has %lld faces, %s has %lld rows and %lld halo rows", who,
                (long long)op->n_faces, name, (long long)v->n_owned, (long long)v->n_halo);
  return STORM_HIP_OK;
}

}  // namespace storm

using namespace storm;

extern "C" {

int storm_hip_op_face_count(const storm_hip_op *op, int64_t *n_faces) {
  STORM_REQUIRE(op && n_faces, "op_face_count: null argument");
  *n_faces = op->updatable ? op->n_faces : 0;
  return STORM_HIP_OK;
}

int storm_hip_op_set_face_weights(storm_hip_op *op, const storm_hip_vec *w_inner, const storm_hip_vec *w_outer,
                                  const storm_hip_vec *diag_extra) {
  STORM_REQUIRE(op && w_inner && w_outer, "op_set_face_weights: null argument");
  STORM_TRY(require_updatable(op, "op_set_face_weights"));
  STORM_TRY(require_face_vector(op, w_inner, "op_set_face_weights", "w_inner"));
  STORM_TRY(require_face_vector(op, w_outer, "op_set_face_weights", "w_outer"));
  if (diag_extra) {
    STORM_REQUIRE(diag_extra->ctx == op->ctx, "op_set_face_weights: diag_extra belongs to another context");
    STORM_REQUIRE(diag_extra->n_owned == op->n_rows, "op_set_face_weights: the operator has %lld rows, diag_extra %lld",
                  (long long)op->n_rows, (long long)diag_extra->n_owned);
  }
  storm_hip_ctx *c = op->ctx;
  HIP_TRY(hipSetDevice(c->device));
  STORM_TRY(lazy_sync(c));
  const double *de = diag_extra ? diag_extra->d : nullptr;
  if (op->n_slices > 0) {
    const int nb = (int)((op->n_slices + (kBlock / kWave) - 1) / (kBlock / kWave));
    if (stream_nt(c, op->n_rows))
      hipLaunchKernelGGL(op_refresh_sell_kernel<true>, dim3(nb), dim3(kBlock), 0, c->stream, op->d_pack, op->d_slice_off, op->d_src,
                         op->n_rows, op->n_slices, w_inner->d, w_outer->d, de);
    else
      hipLaunchKernelGGL(op_refresh_sell_kernel<false>, dim3(nb), dim3(kBlock), 0, c->stream, op->d_pack, op->d_slice_off, op->d_src,
                         op->n_rows, op->n_slices, w_inner->d, w_outer->d, de);
  }
  if (op->tail_nnz > 0)
    hipLaunchKernelGGL(op_refresh_tail_kernel, dim3((int)((op->tail_nnz + kBlock - 1) / kBlock)), dim3(kBlock), 0, c->stream,
                       op->tail_nnz, op->d_tail_src, w_inner->d, w_outer->d, op->d_tail_val);
  HIP_TRY(hipGetLastError());
  if (op->d_pack32 != nullptr) {  // the fp32-weight companion (op_reduced.hip) stays the rounding of the records: no wait, no range check
    STORM_TRY(op_reduced_convert(op, nullptr));
    c->n_op_reduced_refreshes++;
  }
  c->n_op_face_updates++;
  return STORM_HIP_OK;
}

int storm_hip_op_cells_to_faces(const storm_hip_op *op, const storm_hip_vec *cell, storm_hip_vec *at_inner, storm_hip_vec *at_outer) {
  STORM_REQUIRE(op && cell, "op_cells_to_faces: null argument");
  STORM_TRY(require_updatable(op, "op_cells_to_faces"));
  STORM_REQUIRE(cell->ctx == op->ctx, "op_cells_to_faces: cell belongs to another context");
  STORM_REQUIRE(cell->n_owned == op->n_rows && cell->n_halo >= op->n_halo,
                "op_cells_to_faces: the operator has %lld rows and %lld halo rows, cell %lld and %lld", (long long)op->n_rows,
                (long long)op->n_halo, (long long)cell->n_owned, (long long)cell->n_halo);
  if (at_inner) STORM_TRY(require_face_vector(op, at_inner, "op_cells_to_faces", "at_inner"));
  if (at_outer) STORM_TRY(require_face_vector(op, at_outer, "op_cells_to_faces", "at_outer"));
  STORM_REQUIRE(at_inner != cell && at_outer != cell, "op_cells_to_faces: an output aliases cell");
  if (op->n_faces == 0 || (!at_inner && !at_outer)) return STORM_HIP_OK;
  storm_hip_ctx *c = op->ctx;
  HIP_TRY(hipSetDevice(c->device));
  STORM_TRY(lazy_sync(c));
  hipLaunchKernelGGL(cells_to_faces_kernel, dim3((int)((op->n_faces + kBlock - 1) / kBlock)), dim3(kBlock), 0, c->stream, op->n_faces,
                     op->d_face_inner, op->d_face_outer, cell->d, at_inner ? at_inner->d : nullptr, at_outer ? at_outer->d : nullptr);
  HIP_TRY(hipGetLastError());
  return STORM_HIP_OK;
}

}  // extern "C"
