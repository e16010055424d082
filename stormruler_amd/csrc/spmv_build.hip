// The device half of the operator build: the storm_hip_op_create_* entry points, which pack the operator on the host
// (op_pack.hip: formats, records, dictionaries, slice lists -- an OpImage) and upload the image.
// Record layouts: the header of spmv.hip.
#include <algorithm>
#include <utility>

#include <hip/hip_runtime.h>

#include "common.hpp"
#include "host_threads.hpp"

namespace storm {

template <class T>
static int upload(T **dst, const std::vector<T> &src, int64_t *bytes) {
  const size_t nbytes = sizeof(T) * (src.size() ? src.size() : 1);
  hipError_t e = hipMalloc((void **)dst, nbytes);
  if (e != hipSuccess) STORM_FAIL(STORM_HIP_E_ALLOC, "hipMalloc(%zu) failed: %s", nbytes, hipGetErrorString(e));
  if (!src.empty()) HIP_TRY(hipMemcpy(*dst, src.data(), sizeof(T) * src.size(), hipMemcpyHostToDevice));
  *bytes += (int64_t)nbytes;
  return STORM_HIP_OK;
}

// Called from op_set_halo (comm.hip): upload the interior / boundary slice lists.
int op_upload_slice_lists(storm_hip_op *op) {
  if (op->d_interior || op->d_boundary) return STORM_HIP_OK;
  int64_t bytes = 0;
  STORM_TRY(upload(&op->d_interior, op->h_interior, &bytes));
  STORM_TRY(upload(&op->d_boundary, op->h_boundary, &bytes));
  op->n_interior = (int64_t)op->h_interior.size();
  op->n_boundary = (int64_t)op->h_boundary.size();
  // a mixed operator whose interior groups are whole planes of its lattice (a slab of a box but for its outer planes)
  // runs them on the tiled kernel: planes [int_plane0, int_plane1)
  op->int_plane0 = op->int_plane1 = 0;
  if (op->pair == 2 && op->canon_k == 6 && op->n_interior > 0) {
    const int64_t b = op->canon_off[5], g0 = op->h_interior.front(), g1 = (int64_t)op->h_interior.back() + 1;
    const int64_t r0 = g0 * 2 * kWave, r1 = std::min<int64_t>(op->n_rows, g1 * 2 * kWave);
    if (b > 0 && g1 - g0 == op->n_interior && r0 % b == 0 && (r1 % b == 0 || r1 == op->n_rows))
      op->int_plane0 = r0 / b, op->int_plane1 = (r1 + b - 1) / b;
  }
  op->device_bytes += bytes;
  return STORM_HIP_OK;
}

// Every allocation of an operator, in a fixed order (the latency copy, the dictionaries, the records, the CSR tail, the
// row-record index, a mixed operator's boundary records and slice lists), and the reduction workspace it needs.
// (the records in a slot of their vectors' arena -- option pack_arena -- gave no gain: profiles/r05v_pack_arena.jsonl,
//  profiles/experiments/r08_pruned_experiments.patch)
static int op_upload_arrays(storm_hip_ctx *c, const OpImage &img, storm_hip_op *op) {
  HIP_TRY(hipSetDevice(c->device));
  BuildTimer timer;
  int64_t bytes = 0;
  if (!img.lat_off.empty()) {  // (not counted in device_bytes)
    HIP_TRY(hipMalloc((void **)&op->d_lat_pack, img.lat_pack.size() ? img.lat_pack.size() : 1));
    HIP_TRY(hipMalloc((void **)&op->d_lat_off, sizeof(int64_t) * img.lat_off.size()));
    HIP_TRY(hipMemcpy(op->d_lat_pack, img.lat_pack.data(), img.lat_pack.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(op->d_lat_off, img.lat_off.data(), sizeof(int64_t) * img.lat_off.size(), hipMemcpyHostToDevice));
    op->lat_bytes = (int64_t)img.lat_pack.size();
  }
  if (!img.dict.empty()) STORM_TRY(upload(&op->d_dict, img.dict, &bytes));
  if (!img.offs.empty()) STORM_TRY(upload(&op->d_offs, img.offs, &bytes));
  STORM_TRY(upload(&op->d_slice_off, img.slice_off, &bytes));
  STORM_TRY(upload(&op->d_pack, img.pack, &bytes));
  STORM_TRY(upload(&op->d_tail_row, img.tail_row, &bytes));
  STORM_TRY(upload(&op->d_tail_ptr, img.tail_ptr, &bytes));
  STORM_TRY(upload(&op->d_tail_col, img.tail_col, &bytes));
  STORM_TRY(upload(&op->d_tail_val, img.tail_val, &bytes));
  if (!img.rec_words.empty()) {
    STORM_TRY(upload(&op->d_rec_idx, img.rec_idx, &bytes));
    STORM_TRY(upload(&op->d_rec_words, img.rec_words, &bytes));
  }
  if (!img.bnd_pack.empty()) {
    STORM_TRY(upload(&op->d_bnd_pack, img.bnd_pack, &bytes));
    STORM_TRY(op_upload_slice_lists(op));
  }
  if (img.updatable) {  // the source map (4 B per ELL slot and tail entry) and the faces' cells (8 B per face)
    STORM_TRY(upload(&op->d_src, img.src, &bytes));
    STORM_TRY(upload(&op->d_tail_src, img.tail_src, &bytes));
    STORM_TRY(upload(&op->d_face_inner, img.face_inner, &bytes));
    STORM_TRY(upload(&op->d_face_outer, img.face_outer, &bytes));
  }
  timer.lap("upload");
  op->device_bytes += bytes;
  // fused-dot partials: two per SpMV block
  return partials_reserve(c, 8 * (((op->n_rows + kWave - 1) / kWave + 3) / 4) + 16 + 2 * kMaxMulti);
}

static int op_upload(storm_hip_ctx *c, OpImage &&img, storm_hip_op **out) {
  auto *op = new storm_hip_op();
  op->ctx = c;
  op->n_rows = img.n_rows, op->n_halo = img.n_halo, op->nnz = img.nnz;
  op->n_slices = img.n_slices, op->max_row_len = img.max_row_len, op->ell_slots = img.ell_slots;
  op->uniform_width = img.uniform_width, op->pair = img.pair, op->bnd_width = img.bnd_width;
  op->canon_k = img.canon_k, op->canon_m1 = img.canon_m1;
  std::copy(img.canon_off, img.canon_off + 7, op->canon_off);
  op->dict_size = img.dict_size, op->offs_size = img.offs_size, op->rec_words = (int)img.rec_words.size();
  op->spw = img.spw, op->tail_rows = img.tail_rows, op->tail_nnz = img.tail_nnz, op->pack_bytes = img.pack_bytes;
  op->xcd_group_sell = (int)c->opt_spmv_xcd_remap_sell;
  op->updatable = img.updatable, op->n_faces = img.n_faces;
  op->h_interior = std::move(img.interior), op->h_boundary = std::move(img.boundary);
  op->n_interior_slices = (int64_t)op->h_interior.size();
  const int st = op_upload_arrays(c, img, op);
  if (st != STORM_HIP_OK) {
    storm_hip_op_destroy(op);
    return st;
  }
  *out = op;
  return STORM_HIP_OK;
}

static PackOptions pack_options(const storm_hip_ctx *c) {
  PackOptions o;
  o.ell_cap = c->opt_ell_cap, o.spmv_dict = c->opt_spmv_dict, o.spmv_mixed = c->opt_spmv_mixed, o.spmv_spw = c->opt_spmv_spw;
  o.latency_path = c->opt_latency_path, o.latency_rows = c->opt_latency_rows;
  return o;
}

// amg.hip: a coarse-level operator from assembled CSR, forced to fp64 records (the context's ell_cap holds; no latency copy)
// source_map (amg_refresh.hip): the records carry a source map whose id is the CSR entry's index (off-diagonal entries; the
// diagonal is in ext), so that they can be rewritten from a value array; the packing is op_pack_csr's.
int op_create_csr_fp64(storm_hip_ctx *c, int64_t n_rows, const int64_t *row_ptr, const int64_t *col, const double *val,
                       bool source_map, storm_hip_op **out) {
  *out = nullptr;
  PackOptions o = pack_options(c);
  o.spmv_dict = 0, o.latency_path = 0;
  OpImage img;
  if (!source_map) {
    STORM_TRY(op_pack_csr(o, n_rows, 0, row_ptr, col, val, &img));
    return op_upload(c, std::move(img), out);
  }
  STORM_REQUIRE(n_rows >= 0 && row_ptr[n_rows] < (int64_t)INT32_MAX, "amg: a level operator of %lld entries exceeds int32 source ids",
                (long long)row_ptr[n_rows]);
  std::vector<int64_t> rp((size_t)n_rows + 1, 0);
  std::vector<int> oc, src;
  std::vector<double> ov, ext((size_t)n_rows, 0.0);
  for (int64_t i = 0; i < n_rows; ++i) {
    double rowsum = 0.0;
    for (int64_t k = row_ptr[i]; k < row_ptr[i + 1]; ++k) {
      STORM_REQUIRE(col[k] >= 0 && col[k] < n_rows, "amg: column %lld of row %lld outside [0, %lld)", (long long)col[k], (long long)i,
                    (long long)n_rows);
      rowsum += val[k];
      if (col[k] != i) oc.push_back((int)col[k]), ov.push_back(val[k]), src.push_back((int)k);
    }
    ext[(size_t)i] = rowsum;
    rp[(size_t)i + 1] = (int64_t)oc.size();
  }
  STORM_TRY(op_pack(o, n_rows, 0, rp, oc, ov, ext, &img, &src));
  img.updatable = 1, img.n_faces = 0;  // (uploads the source map; no face lists)
  STORM_TRY(op_upload(c, std::move(img), out));
  (*out)->updatable = 0;  // not a face-weight operator: storm_hip_op_set_face_weights must refuse it
  return STORM_HIP_OK;
}

}  // namespace storm

using namespace storm;

extern "C" {

int storm_hip_op_create_from_face_weights(storm_hip_ctx *c, int64_t n_owned, int64_t n_halo,
                                          int64_t n_faces, const int64_t *inner, const int64_t *outer,
                                          const double *w_inner, const double *w_outer,
                                          const double *diag_extra, storm_hip_op **out) {
  STORM_REQUIRE(c && out, "op_create: null argument");
  *out = nullptr;
  OpImage img;
  STORM_TRY(op_pack_from_face_weights(pack_options(c), n_owned, n_halo, n_faces, inner, outer, w_inner, w_outer, diag_extra, &img));
  return op_upload(c, std::move(img), out);
}

int storm_hip_op_create_from_face_weights_updatable(storm_hip_ctx *c, int64_t n_owned, int64_t n_halo, int64_t n_faces,
                                                    const int64_t *inner, const int64_t *outer, const double *w_inner,
                                                    const double *w_outer, const double *diag_extra, storm_hip_op **out) {
  STORM_REQUIRE(c && out, "op_create: null argument");
  *out = nullptr;
  OpImage img;
  PackOptions o = pack_options(c);
  o.updatable = 1;
  STORM_TRY(op_pack_from_face_weights(o, n_owned, n_halo, n_faces, inner, outer, w_inner, w_outer, diag_extra, &img));
  return op_upload(c, std::move(img), out);
}

int storm_hip_op_create_from_faces(storm_hip_ctx *c, int64_t n_owned, int64_t n_halo, int64_t n_faces,
                                   const int64_t *inner, const int64_t *outer, const double *coef,
                                   int64_t n_bfaces, const int64_t *b_cell, const double *b_coef,
                                   const double *volume, storm_hip_op **out) {
  STORM_REQUIRE(c && out, "op_create_from_faces: null argument");
  *out = nullptr;
  OpImage img;
  STORM_TRY(op_pack_from_faces(pack_options(c), n_owned, n_halo, n_faces, inner, outer, coef, n_bfaces, b_cell, b_coef, volume, &img));
  return op_upload(c, std::move(img), out);
}

int storm_hip_op_create_from_mesh(storm_hip_ctx *c, int64_t n_owned, int64_t n_halo, int32_t dim, int64_t n_faces,
                                  const int64_t *inner, const int64_t *outer, const double *area, const double *center,
                                  int64_t n_bfaces, const int64_t *b_cell, const double *b_area, const double *b_center,
                                  const double *volume, storm_hip_op **out) {
  STORM_REQUIRE(c && out, "op_create_from_mesh: null argument");
  *out = nullptr;
  OpImage img;
  STORM_TRY(op_pack_from_mesh(pack_options(c), n_owned, n_halo, dim, n_faces, inner, outer, area, center, n_bfaces, b_cell, b_area,
                              b_center, volume, &img));
  return op_upload(c, std::move(img), out);
}

int storm_hip_op_create_csr(storm_hip_ctx *c, int64_t n_rows, int64_t n_halo, const int64_t *row_ptr,
                            const int64_t *col, const double *val, storm_hip_op **out) {
  STORM_REQUIRE(c && out && row_ptr, "op_create_csr: null argument");
  *out = nullptr;
  OpImage img;
  STORM_TRY(op_pack_csr(pack_options(c), n_rows, n_halo, row_ptr, col, val, &img));
  return op_upload(c, std::move(img), out);
}

}  // extern "C"
