/*
 * storm_hip.h -- C ABI of the MI355X-native Krylov backend for StormRuler.
 *
 * This is the drop-in boundary: plain pointers and sizes, opaque
 * handles, `int` status returns, no exceptions, no torch / C++ types.  Every
 * entry point names the reference interface it stands in for (paths relative
 * to the reference root).  The C++ header `storm_hip/Storm.hpp` maps the
 * reference's `Storm::Operator / Vector / Solver` template interface onto
 * these calls; INTEGRATION.md shows the binding a StormRuler maintainer adds.
 *
 * Conventions
 *  - Status: 0 = ok; negative = error (STORM_HIP_E_*); text of the last error
 *    of the calling thread via storm_hip_last_error().
 *  - Ownership: the caller owns every handle it creates and destroys it; the
 *    library copies host arrays passed to *_create_* (the caller may free them
 *    on return) and never frees caller memory.
 *  - Threading: as the reference (single-threaded, stateful solver objects,
 *    Solvers/Solver.hpp:66-76) -- one host thread per context; a context owns
 *    its HIP streams; calls on one context are not re-entrant.
 *  - Multi-GPU: one process (context) per GPU.  Vectors hold `n_owned` rows
 *    followed by `n_halo` ghost rows; reductions are summed over all ranks.
 *  - All arithmetic is fp64 (`real_t = double`, Crow/Base/Types.hpp:38);
 *    indices cross the ABI as int64 (the reference's Index wraps size_t,
 *    Utils/Index.hpp:41) and are narrowed to int32 on the device after a
 *    range check.
 */
#ifndef STORM_HIP_H_
#define STORM_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* every declaration below is an exported symbol of libstorm_hip.so */
#pragma GCC visibility push(default)

#define STORM_HIP_ABI_VERSION 6
/* Feature-test macro, here to stay: defined (to 1) by every header that declares the two-stage operator
 * (storm_hip_op_apply2, storm_hip_solve_cg2, storm_hip_krylov_set_operator2; HipTwoStageOperator in storm_hip/Storm.hpp),
 * which was added within ABI 6.  A caller that must also build against an older header tests it with #ifdef. */
#define STORM_HIP_HAS_TWO_STAGE 1
/* ... and by every header that declares the updatable face-weight operator (storm_hip_op_create_from_face_weights_updatable,
 * storm_hip_op_set_face_weights, storm_hip_op_cells_to_faces, storm_hip_op_face_count), added within ABI 6 as well. */
#define STORM_HIP_HAS_FACE_UPDATE 1
/* ... and by every header that declares the fp32-weight companion records (storm_hip_op_build_reduced and the *_reduced
 * entry points, storm_hip_cheb_create_reduced), added within ABI 6 as well. */
#define STORM_HIP_HAS_REDUCED_RECORDS 1

enum {
  STORM_HIP_OK = 0,
  STORM_HIP_E_INVALID = -1,   /* bad argument (null handle, size mismatch, index out of range) */
  STORM_HIP_E_HIP = -2,       /* a HIP runtime call failed */
  STORM_HIP_E_NO_DEVICE = -3, /* no usable gfx950 device */
  STORM_HIP_E_COMM = -4,      /* RCCL failure / communicator misuse */
  STORM_HIP_E_ALLOC = -5,
  STORM_HIP_E_UNSUPPORTED = -6
};

typedef struct storm_hip_ctx storm_hip_ctx;
typedef struct storm_hip_vec storm_hip_vec;
typedef struct storm_hip_op storm_hip_op;

int storm_hip_abi_version(void);
const char *storm_hip_last_error(void);

/* ---- context -------------------------------------------------------------
 * Nothing in the reference (it has no device, SURVEY.md headline fact 1). */
int storm_hip_ctx_create(int device_id, storm_hip_ctx **out);
int storm_hip_ctx_destroy(storm_hip_ctx *ctx);
int storm_hip_ctx_sync(storm_hip_ctx *ctx);
/* name: >= 64 bytes. */
int storm_hip_ctx_info(storm_hip_ctx *ctx, char *name, int name_len, int *num_cus,
                       int64_t *total_mem_bytes);

/* HIP-event stopwatch on the context's compute stream (the stream every
 * kernel of this library is launched on). */
int storm_hip_timer_start(storm_hip_ctx *ctx);
int storm_hip_timer_stop(storm_hip_ctx *ctx, float *elapsed_ms);

/* With option "profile_spmv" = 1 every launch of the dominant kernel (the sliced-ELL SpMV)
 * is bracketed by a HIP-event pair on the compute stream; this returns and resets the
 * accumulated launch count and durations (synchronises the stream). */
int storm_hip_ctx_get_spmv_profile(storm_hip_ctx *ctx, int64_t *launches, double *total_ms,
                                   double *min_ms);
/* ... the same launches one by one (milliseconds each, in launch order; at most `capacity` are written, *count is
 * how many there were); resets the profile like the call above. */
int storm_hip_ctx_get_spmv_profile_samples(storm_hip_ctx *ctx, double *ms_out, int64_t capacity, int64_t *count);

/* ---- communicator (RCCL over xGMI) -------------------------
 * rank 0 fills a 128-byte id, the host distributes it (torch.distributed /
 * MPI / a file), every rank calls comm_init.  n_ranks == 1 needs neither. */
int storm_hip_comm_unique_id(void *id128);
int storm_hip_ctx_comm_init(storm_hip_ctx *ctx, const void *id128, int n_ranks, int rank);
int storm_hip_ctx_comm_size(storm_hip_ctx *ctx, int *n_ranks, int *rank);
/* What RCCL ITSELF says about this context's communicators (not what the host passed to comm_init): ncclCommCount /
 * ncclCommUserRank / ncclCommCuDevice of the halo communicator, ncclCommCount of the reduction communicator, the HIP
 * device of the context and its PCI bus id (>= 16 bytes).  All counts are 0 on a context without an RCCL communicator
 * (one rank, or the host-staged / peer-window transports).  Fails with STORM_HIP_E_COMM when RCCL reports an asynchronous
 * error.  For a run's record: a reader can check that RCCL saw N ranks on N distinct devices.  Nothing in the reference
 * corresponds to it (single process). */
int storm_hip_ctx_comm_rccl_view(storm_hip_ctx *ctx, int *halo_count, int *halo_user_rank, int *halo_device, int *red_count,
                                 int *hip_device, char *pci_bus_id, int pci_bus_id_len);
/* Host-staged transport: the same multi-rank protocol (halo planes before the boundary rows of an SpMV,
 * global sums behind every reduction) with the bytes moved by the host program's own messaging layer
 * instead of RCCL -- for hosts that already run MPI / gloo, and for putting several ranks on ONE device.
 *   allreduce(user, buf, count): in-place sum of `count` doubles over all ranks (host memory);
 *   exchange(user, n_nbrs, nbr_rank, send_ptr, send, recv_ptr, recv): deliver send[send_ptr[q]..send_ptr[q+1])
 *     to rank nbr_rank[q] and fill recv[recv_ptr[q]..recv_ptr[q+1]) with what that rank sent here.
 * Both return 0 on success.  Synchronous (no overlap with the interior rows).  Nothing in the reference
 * corresponds to it (single process); SURVEY.md 8e. */
typedef int (*storm_hip_allreduce_fn)(void *user, double *buf, int count);
typedef int (*storm_hip_exchange_fn)(void *user, int n_nbrs, const int32_t *nbr_rank, const int64_t *send_ptr,
                                     const double *send, const int64_t *recv_ptr, double *recv);
int storm_hip_ctx_comm_init_host(storm_hip_ctx *ctx, int n_ranks, int rank, storm_hip_allreduce_fn allreduce,
                                 storm_hip_exchange_fn exchange, void *user);

/* Peer-window transport: every rank owns a window of device memory that all ranks map through HIP IPC; halo planes
 * and reduction scalars are written straight into the RECEIVER's window by the sender's kernels (over xGMI between
 * GPUs) and picked up by polling -- a one-shot all-reduce of up to 64 doubles summed in rank order (the same bits
 * on every rank; SURVEY.md 8e "Determinism") and direct halo writes with flag + acknowledgement, in place of
 * RCCL's latency-bound small collectives.  Also works between processes that share ONE device.
 *   1. every rank: storm_hip_ctx_comm_ipc_export(ctx, n_ranks, rank, window_bytes (0 = 16 MiB), handle64)
 *   2. the host program all-gathers the 64-byte handles (rank order)
 *   3. every rank: storm_hip_ctx_comm_init_ipc(ctx, handles)
 * A (sender, receiver) pair may move up to (window_bytes / (2 n_ranks)) bytes per exchange.  Waits are bounded (5 s);
 * a timeout surfaces as STORM_HIP_E_COMM from the next call.  Needs HSA_ENABLE_IPC_MODE_LEGACY=0 on hosts whose
 * driver only supports dmabuf IPC.  Nothing in the reference corresponds to it (single process). */
int storm_hip_ctx_comm_ipc_export(storm_hip_ctx *ctx, int n_ranks, int rank, int64_t window_bytes, void *handle64);
int storm_hip_ctx_comm_init_ipc(storm_hip_ctx *ctx, const void *handles);

/* ---- vectors -------------------------------------------------------------
 * `Feathers::Field` as the solver `Vector` (Feathers/Field.hpp:60-114):
 * contiguous doubles, one per cell.  create == `assign(other, false)`, which
 * value-initialises (zero-fills) a new field (Field.hpp:82-84). */
int storm_hip_vec_create(storm_hip_ctx *ctx, int64_t n_owned, int64_t n_halo, storm_hip_vec **out);
int storm_hip_vec_create_like(const storm_hip_vec *other, storm_hip_vec **out);
int storm_hip_vec_destroy(storm_hip_vec *v);
int storm_hip_vec_size(const storm_hip_vec *v, int64_t *n_owned, int64_t *n_halo);
int storm_hip_vec_upload(storm_hip_vec *v, const double *host, int64_t n);
int storm_hip_vec_download(const storm_hip_vec *v, double *host, int64_t n);
/* Raw device pointer (n_owned + n_halo doubles), for zero-copy interop.  The address stays valid until the vector is
 * destroyed (a vector that has given its address out is never one whose storage option lazy_statements = 2 exchanges). */
int storm_hip_vec_device_ptr(storm_hip_vec *v, void **dev_ptr);
/* The context a vector lives on. */
int storm_hip_vec_context(const storm_hip_vec *v, storm_hip_ctx **ctx);
/* One element (waits for the stream; a debugging / concept-check accessor, never used by the solvers):
 * `Field::operator()(row, col)`, Feathers/Field.hpp:104-111. */
int storm_hip_vec_get(const storm_hip_vec *v, int64_t row, double *value);

/* ---- block vectors ---------------------------------------------------------
 * `Field<Mesh, Index, Value, NumVars>` with NumVars > 1 (Feathers/Field.hpp:56-79: shape [num_entities, NumVars], every
 * cell stores a Vec<Value, NumVars>; the playground's CellField<Mesh, real_t, 5>, Playground.cpp:217-218).  No handle
 * type of its own: a block of k columns over n cells IS a storm_hip_vec with n_owned = n * k and n_halo = 0, element
 * (i, j) at i * k + j -- the reference's layout.  1 <= k <= 8.  Upload, download, fill, copy, scale and every other
 * elementwise entry point work on it as on any vector, and storm_hip_dot over two blocks is the reference's
 * dot_product over all NumVars components (MatrixAlgorithms.hpp:310-317).  Single rank only: a vector with halo rows or
 * a context with a communicator is refused with STORM_HIP_E_UNSUPPORTED. */
/* Strided copy between column j of a block and a plain n-vector: `Field::operator()(row, j)` for every row,
 * Feathers/Field.hpp:104-111. */
int storm_hip_block_get_column(const storm_hip_vec *X, int k, int j, storm_hip_vec *v);
int storm_hip_block_set_column(storm_hip_vec *X, int k, int j, const storm_hip_vec *v);
/* out[j] = <A_j, B_j>, j < k: dot_product (MatrixAlgorithms.hpp:310-317) column by column. */
int storm_hip_block_dot(const storm_hip_vec *A, const storm_hip_vec *B, int k, double *out);
/* Y_j = fma(a[j], X_j, Y_j), j < k: `y += a * x` (SolverCg.hpp:98) with one coefficient per column.  X and Y must not alias. */
int storm_hip_block_axpy(storm_hip_vec *Y, const double *a, const storm_hip_vec *X, int k);

/* ---- BLAS-1 --------------------------------------------------------------
 * One call per Bittern expression statement the solver bodies execute
 * (overload census); each is one kernel over the owned rows.
 * Reference loops: Bittern/MatrixAlgorithms.hpp:58-81 (matrix_for_each),
 * :162-205 (reduce).  Reductions return the sum over all ranks.
 *
 * Rounding.  The library is built with -ffp-contract=on: a product may be fused into the addition that consumes it,
 * within one expression.  WHICH evaluation of the reference's expression an entry point gives is part of its contract,
 * the same on every row (the odd last row included), for every size, under every blas1_nt setting and with
 * lazy_statements 0 or 1 (tests/test_gpu_exact_statements.py; fl = one rounding, fma(a, b, c) = fl(a b + c) with the
 * product exact).  ONE EXCEPTION, lazy_statements = 2 (which the host loops of Storm.hpp / api.py switch on): where
 * `x += a p; p <<= r + b p; z = A p; <p, z>` leaves as the fused CG step of a lattice operator (see that option below),
 * storm_hip_xpay IS fma(b, y, x) -- one rounding, as the library's device loop computes it -- not the form of this table
 * (storm_hip_axpy is fma(a, x, y) either way):
 *     fill, copy, scale, div_scalar, vmul                    one operation, correctly rounded
 *     vdiv                                                   fl(fl(s a) / b);  a == NULL: fl(s / b)
 *     axpbz(y, a, x, b, z)                                   fma(a, x, fl(b z)): the FIRST product is the fused one
 *       with b == 0 and z the same vector as x               fl(a x) -- `y <<= a * x`: -0, +-inf as a * x gives them
 *     axpy(y, a, x)   = axpbz(y, a, x, 1, y)                 fma(a, x, y)
 *     xpay(y, x, b)   = axpbz(y, 1, x, b, y)                 fl(x + fl(b y)): NOT fma(b, y, x)
 *     lin3(y, r, s, a, x, b, z)                              fma(s, fma(a, x, fl(b z)), r)
 *     bicgstab_p(p, r, beta, omega, v)                       fma(beta, fma(-omega, v, p), r)
 *     vmul_add(y, s, a, b)                                   fma(s, fl(a b), y)
 *     multi_axpy(y, coefs, xs, k)                            y = fma(coefs[j], xs[j], y) for j = 0 .. k - 1 in turn
 *     map                                                    every operation rounded on its own (see below)
 *   and the two statements around the callback of a finite-difference operator (storm_hip_krylov_set_operator_fd):
 *     s = x + delta y                                        fl(x + fl(delta y)) = fma(1, x, fl(delta y)): NOT fma(delta, y, x)
 *     z = delta_inverse (z - w)                              fl(delta_inverse fl(z - w))
 * So BiCGStab's p through storm_hip_lin3(p, r, beta, 1, p, -omega, v) -- fma(beta, fl(p + fl(-omega v)), r) -- and through
 * storm_hip_bicgstab_p differ in the last place on about one row in eleven: a caller who wants the bits of one must
 * call that one. */
int storm_hip_fill(storm_hip_vec *y, double value);                        /* fill_with(y, v)   Solver.hpp:281 */
int storm_hip_copy(storm_hip_vec *y, const storm_hip_vec *x);              /* y <<= x           MatrixAlgorithms.hpp:120-124 */
int storm_hip_scale(storm_hip_vec *y, double s);                           /* y *= s            MatrixTarget.hpp:96-99 */
int storm_hip_div_scalar(storm_hip_vec *y, double s);                      /* y /= s            MatrixTarget.hpp:101-105, SolverGmres.hpp:88 */
int storm_hip_axpy(storm_hip_vec *y, double a, const storm_hip_vec *x);    /* y += a*x (a<0: y -= |a|*x)  SolverCg.hpp:98-99 */
int storm_hip_xpay(storm_hip_vec *y, const storm_hip_vec *x, double b);    /* y <<= x + b*y     SolverCg.hpp:123 */
/* y <<= a*x + b*z  (covers r <<= b - r, Operator.hpp:98; y may alias x or z).  b == 0 with z the same vector as x is
 * the one-term statement `y <<= a * x`: x is streamed once. */
int storm_hip_axpbz(storm_hip_vec *y, double a, const storm_hip_vec *x, double b, const storm_hip_vec *z);
/* p <<= r + beta*(p - omega*v)   SolverBiCgStab.hpp:119 */
int storm_hip_bicgstab_p(storm_hip_vec *p, const storm_hip_vec *r, double beta, double omega,
                         const storm_hip_vec *v);
/* y <<= r + s*(a*x + b*z): the nested three-term updates -- BiCGStab's p (above) and CGS's
 * `p <<= u + beta*(q + beta*p)`, SolverCgs.hpp:122.  y may alias any operand. */
int storm_hip_lin3(storm_hip_vec *y, const storm_hip_vec *r, double s, double a, const storm_hip_vec *x,
                   double b, const storm_hip_vec *z);
/* y += s * (a .* b), elementwise.  Not in the solver census: the nonlinear term a time-step
 * driver forms between solves (cf. `f <<= map(dF_dc, c)`, Playground.cpp:148). */
int storm_hip_vmul_add(storm_hip_vec *y, double s, const storm_hip_vec *a, const storm_hip_vec *b);
/* `out <<= map(func, mats...)`  Bittern/MatrixMath.hpp:44-105 (MapMatrixView, map) evaluated by the element loop of
 * MatrixAlgorithms.hpp:75-79, 120-124 -- the playground's `f <<= map(dF_dc, c)`, Playground.cpp:142-148.  `func` arrives as
 * a program in reverse Polish notation over the elements x0[i], x1[i], y[i] (the old value of the target) and up to 16
 * constants: program[k] = opcode | (constant index << 8), at most 48 operations, at most 8 operands at once; it must leave
 * exactly one value.  Only exactly-rounded operations (+ - * / sqrt abs neg min max), each rounded on its own, no
 * contraction: y[i] is what the host's scalar evaluation of the same expression in the same order gives, BIT FOR BIT.
 * x0 / x1 may be NULL when the program does not read them and may alias y.  include/storm_hip/Storm.hpp builds the
 * program by tracing a generic lambda: `f <<= map([](auto c) { return 2.0 * c * (c - 1.0) * (2.0 * c - 1.0); }, c)`. */
enum {
  STORM_HIP_MAP_X0 = 0, STORM_HIP_MAP_X1 = 1, STORM_HIP_MAP_Y = 2, STORM_HIP_MAP_CONST = 3, /* push an operand */
  STORM_HIP_MAP_NEG = 8, STORM_HIP_MAP_ABS = 9, STORM_HIP_MAP_SQRT = 10,                    /* top = op(top) */
  STORM_HIP_MAP_ADD = 16, STORM_HIP_MAP_SUB = 17, STORM_HIP_MAP_MUL = 18, STORM_HIP_MAP_DIV = 19, /* second OP top */
  STORM_HIP_MAP_MIN = 20, STORM_HIP_MAP_MAX = 21
};
int storm_hip_map(storm_hip_vec *y, const storm_hip_vec *x0, const storm_hip_vec *x1, const int32_t *program, int n_ops,
                  const double *constants, int n_constants);
/* y = a .* b, elementwise: `Preconditioner::mul` of a diagonal (Jacobi) preconditioner behind the
 * pre_op hook of Solvers/Solver.hpp:74-75 (the reference ships only IdentityPreconditioner,
 * Preconditioner.hpp:84-97).  y may alias a or b. */
int storm_hip_vmul(storm_hip_vec *y, const storm_hip_vec *a, const storm_hip_vec *b);
/* y = (s * a) ./ b, elementwise; a == NULL: y = s ./ b.  The quotient nodes of the reference's expression
 * templates, `scalar / mat` and `mat1 / mat2` (Bittern/MatrixMath.hpp:261-265, :298-302; known answers
 * tests/unit/BitternMath.cpp:160-171).  Not in the solver census.  y may alias a or b. */
int storm_hip_vdiv(storm_hip_vec *y, double s, const storm_hip_vec *a, const storm_hip_vec *b);
/* fill_randomly(y)  Bittern/MatrixAlgorithms.hpp:140-153: uniform [0, 1) numbers from a
 * function-static std::mt19937_64{} (default seed, state persists across calls), drawn
 * sequentially on the host in row order and uploaded -- the same engine, distribution and
 * standard library the reference uses, hence the same numbers.  Single rank only.
 * storm_hip_rng_reset() restarts the engine (what a fresh process is to the reference). */
int storm_hip_fill_randomly(storm_hip_vec *y);
void storm_hip_rng_reset(void);
/* dot_product(a, b)  MatrixAlgorithms.hpp:310-317;  norm_2(a)  :262-270 */
int storm_hip_dot(const storm_hip_vec *a, const storm_hip_vec *b, double *result);
int storm_hip_norm2(const storm_hip_vec *a, double *result);
/* out[i] = <a, bs[i]>, i < k: the Arnoldi multi-dot (SolverGmres.hpp:157-160 batched). */
int storm_hip_multi_dot(const storm_hip_vec *a, const storm_hip_vec *const *bs, int k, double *out);
/* The same reduction in two halves: _begin enqueues it and returns a request, _end waits for the
 * sums (in pinned host memory, written by the kernel's last block) -- up to 8 requests in flight,
 * ended in any order; the caller's host work, or further launches, overlap the ~9 us a synchronous
 * dot spends between the end of its kernel and the start of the next one.  storm_hip_multi_dot is
 * _begin + _end.  (With a communicator, or k > 8, _begin computes the sums and _end returns them.) */
int storm_hip_multi_dot_begin(const storm_hip_vec *a, const storm_hip_vec *const *bs, int k, int *request);
int storm_hip_multi_dot_end(storm_hip_ctx *ctx, int request, double *out);
/* y += sum_i coefs[i] * xs[i]  (SolverGmres.hpp:233-236 batched).  No xs[i] may be y (refused); they may repeat. */
int storm_hip_multi_axpy(storm_hip_vec *y, const double *coefs, const storm_hip_vec *const *xs, int k);

/* ---- operators -----------------------------------------------------------
 * The matrix-free FVM stencil `stormDivGrad` (source_apps/playground/
 * Playground.cpp:115-131) precomputed into gather form.  Applying an operator
 * computes   y = beta * x + alpha * M(x)   on the owned rows, where for the
 * face-graph constructors
 *     M(x)_i = sum_{faces f of i} w_if * (x_other(f) - x_i) + diag_extra_i * x_i .
 * `alpha = -1, beta = 0` is the Poisson operator -L; `alpha = -kappa, beta = 1`
 * the Helmholtz operator of the playground lambda (Playground.cpp:153-167).
 *
 * Row i's entries are summed in face order, the order in which the
 * reference's face loop accumulates into u[i].
 */

/* Diffusion operator from the mesh quantities the reference reads:
 *   inner/outer[F]   face -> cells (FaceView::inner_cell/outer_cell, Mallard/Mesh.hpp:269-280),
 *                    local ids in [0, n_owned + n_halo);
 *   coef[F]          A_f / |x_outer - x_inner|   (Playground.cpp:126-128);
 *   b_cell/b_coef[B] Dirichlet boundary faces: owning cell and A_b / |x_face - x_cell|
 *                    (ghost value 0 at the face; loop shape of Feathers/ConvectionScheme.hpp:95-106);
 *   volume[n_owned + n_halo]  cell volumes (CellView::volume, Mallard/Mesh.hpp:304).
 * w_if = coef_f / volume_i;  diag_extra_i = -sum_b b_coef_b / volume_i. */
int storm_hip_op_create_from_faces(storm_hip_ctx *ctx, int64_t n_owned, int64_t n_halo,
                                   int64_t n_faces, const int64_t *inner, const int64_t *outer,
                                   const double *coef, int64_t n_bfaces, const int64_t *b_cell,
                                   const double *b_coef, const double *volume, storm_hip_op **out);

/* The same operator straight from the mesh arrays the reference's face loop reads (Playground.cpp:119-129): the
 * library forms A_f / |x_outer - x_inner| itself -- squares summed left to right like `length`
 * (MatrixAlgorithms.hpp:262-270, 303-305), threaded -- instead of taking it as `coef`.
 *   area[F], center[(n_owned + n_halo) * dim] (row-major), b_area[B], b_center[B * dim]; dim in 1..3.
 * Bit-identical to storm_hip_op_create_from_faces with coefficients computed that way on the host. */
int storm_hip_op_create_from_mesh(storm_hip_ctx *ctx, int64_t n_owned, int64_t n_halo, int32_t dim, int64_t n_faces,
                                  const int64_t *inner, const int64_t *outer, const double *area, const double *center,
                                  int64_t n_bfaces, const int64_t *b_cell, const double *b_area, const double *b_center,
                                  const double *volume, storm_hip_op **out);

/* General (non-symmetric) face-graph operator: row inner[f] gets weight
 * w_inner[f] on (x_outer - x_inner), row outer[f] gets w_outer[f] on
 * (x_inner - x_outer); diag_extra[n_owned] may be NULL (zeros).  This is the
 * form the upwind convection face loop (Feathers/ConvectionScheme.hpp:80-107)
 * lowers to. */
int storm_hip_op_create_from_face_weights(storm_hip_ctx *ctx, int64_t n_owned, int64_t n_halo,
                                          int64_t n_faces, const int64_t *inner,
                                          const int64_t *outer, const double *w_inner,
                                          const double *w_outer, const double *diag_extra,
                                          storm_hip_op **out);

/* The same operator, UPDATABLE: its face weights can be rewritten on the device (storm_hip_op_set_face_weights) from
 * vectors of per-face values, with no host rebuild -- for coefficients that change every step and are known only on
 * the device: an upwind convection term whose velocity moves (Feathers/ConvectionScheme.hpp:80-107; the playground's
 * commented-out CONV, Playground.cpp:155-166), a mobility M(c), a variable density.  Same arguments, same rows, same
 * face-order summation.  The operator keeps the fp64 records (as under option spmv_dict = 0) whatever it would qualify
 * for, keeps no compact copy for the one-kernel paths, and carries a source map: 4 bytes per record slot and CSR-tail
 * entry plus 8 bytes per face of device memory.  n_faces >= 2^30: STORM_HIP_E_INVALID.
 *
 * A FACE VECTOR is an ordinary storm_hip_vec of the operator's context with n_owned == n_faces and n_halo == 0, element f
 * belonging to face f of the arrays the operator was created from; every vector statement (storm_hip_map, _vmul, ...)
 * works on it.
 *
 * storm_hip_op_face_count: n_faces of an updatable operator, 0 for any other.
 * storm_hip_op_set_face_weights: the weights become w_inner / w_outer and the diagonal term diag_extra (n_owned rows of
 *   the operator; NULL: zeros).  Enqueued on the context's stream; never waits for the device.  Contract: afterwards the
 *   operator is in every respect -- apply, block apply, diagonal, Gershgorin bound, every solver -- the one a fresh create
 *   with those weights gives, bit for bit.  Objects that cached something derived from the OLD values are the caller's to
 *   rebuild: a storm_hip_cheb (its eigenvalue bounds), a storm_hip_amg (its whole hierarchy: coarse operators, transfers,
 *   smoothers' scales and bounds are those of the old weights -- unless it was created refreshable: then
 *   storm_hip_amg_refresh recomputes all of them on the device) and a diagonal obtained earlier.  An update between
 *   storm_hip_krylov_init and storm_hip_krylov_finalize of a solve on this operator is the caller's error.
 *   Counted by "op_face_updates" (storm_hip_ctx_get_counter).
 * storm_hip_op_cells_to_faces: at_inner[f] = cell[inner[f]], at_outer[f] = cell[outer[f]] for a cell vector of the
 *   operator's size (its halo tail is read as it stands: no exchange); either output may be NULL.
 * Refusals, all before a device is touched, with a message that names the sizes: an operator that was not created
 * updatable STORM_HIP_E_UNSUPPORTED; a null argument, a vector of the wrong length or of another context
 * STORM_HIP_E_INVALID. */
int storm_hip_op_create_from_face_weights_updatable(storm_hip_ctx *ctx, int64_t n_owned, int64_t n_halo,
                                                    int64_t n_faces, const int64_t *inner,
                                                    const int64_t *outer, const double *w_inner,
                                                    const double *w_outer, const double *diag_extra,
                                                    storm_hip_op **out);
int storm_hip_op_face_count(const storm_hip_op *op, int64_t *n_faces);
int storm_hip_op_set_face_weights(storm_hip_op *op, const storm_hip_vec *w_inner, const storm_hip_vec *w_outer,
                                  const storm_hip_vec *diag_extra);
int storm_hip_op_cells_to_faces(const storm_hip_op *op, const storm_hip_vec *cell, storm_hip_vec *at_inner,
                                storm_hip_vec *at_outer);

/* Assembled CSR rows (n_rows owned rows, columns in [0, n_rows + n_halo)). */
int storm_hip_op_create_csr(storm_hip_ctx *ctx, int64_t n_rows, int64_t n_halo,
                            const int64_t *row_ptr, const int64_t *col, const double *val,
                            storm_hip_op **out);

/* Options: 40 keys (csrc/context.hip), all with measured defaults.  Refinements that were measured and dropped are not
 * switches any more: their patch is profiles/experiments/r08_pruned_experiments.patch.
 *
 * Build knobs, read when an operator / vector is created:
 *   ell_cap (0 = none): rows longer than this spill their remaining entries to the CSR tail;
 *   spmv_dict (4): the most compact LOSSLESS record format an operator may take -- 0 fp64 weights + int32 columns (what any
 *              mesh gets); 1 byte-indexed weights (<= 256 distinct fp64 bit patterns, <= 7 neighbours per row); 2 + byte-indexed
 *              column offsets; 3 + two consecutive rows share one merged neighbour list and their 16-byte gathers; 4 + one
 *              common offset order for the whole operator (a structured box in natural ordering), +-1 neighbours from the
 *              adjacent lanes.  Every format gives the same bits (tests/test_gpu_formats.py);
 *   spmv_mixed (1): a partitioned operator keeps format 4 for the row groups that read no halo column, format 3 elsewhere;
 *   spmv_spw (0 = automatic): slices per wavefront of the byte-indexed kernel (1, 2, 4);
 *   spmv_canon_tile (2), spmv_canon_tile_min_rows (2^20): format 4 on a lattice -- tiles of 1024 rows x 2 (4) planes with the
 *              in-plane neighbours from LDS and the out-of-plane ones from registers, from this many rows on (0 = plain kernel);
 *   latency_rows (2^19): operators up to this size keep a compact fp64 copy for the one-kernel CG / BiCGStab;
 *   pool_bytes (16 GiB): vector storage released by vec_destroy is kept for the next vec_create of the same size;
 *   vec_arena (1): the vectors of one size are slots of ONE physically contiguous allocation a fixed distance apart.
 * Paths (which loop a solve takes; every path gives the reference's iteration to rounding):
 *   latency_path (1), latency_cache (1): CG / BiCGStab of a small halo-free operator as ONE cooperative kernel per solve
 *              (0: neither this nor the resident path; 2: this path only); operator records held in registers where they fit;
 *   latency_pre (0): 1 = storm_hip_krylov_solve with method CG and a preconditioner takes that path too (csrc/latency.hip,
 *              pcg_latency_kernel: z = P r, p = z + beta p, gamma = <r, z>, the error norm_2(r); two synchronisation points per
 *              iteration with a diagonal, degree + 2 with a Chebyshev polynomial) when ALL of these hold: the operator is the
 *              unpreconditioned path's (a native single-stage operator with a compact copy -- latency_rows, no halo, no CSR
 *              tail --, no communicator, latency_path != 0) and not one the resident path takes; generic_solvers == 0; the
 *              preconditioner is a diagonal (storm_hip_krylov_set_preconditioner_diag) or a storm_hip_cheb that is not reduced
 *              and was created on the solve's own operator with the solve's alpha and beta.  Any side (CG has none).  Everything
 *              else -- a Chebyshev object on another operator, a callback or multigrid preconditioner, a two-stage operator,
 *              BiCGStab, more than two slices of rows per wavefront -- runs the engine as before; a refused launch or a kernel
 *              that gave up re-runs on the engine (path_fallback 1 / 2).  iterations, converged, the errors, history,
 *              num_applies and *pre_applies are what the engine reports for the same solve;
 *   resident_path (1), resident_max_rows (2^22), resident_planes (0 = automatic), resident_early (1): CG / BiCGStab of a
 *              halo-free LATTICE operator as one persistent kernel in which every block owns a box of the lattice
 *              (csrc/resident.hip); surfaces travelling under the all-reduces;
 *   coop_mgs (1), coop_mgs_lds (1), coop_mgs_quad (1): GMRES's Gram-Schmidt chain as one cooperative kernel per Arnoldi step;
 *              its LDS-ring and four-steps-per-synchronisation forms (2 = forced, for tests; 0 = off);
 *   mgs_steps (4): modified-Gram-Schmidt steps per pass over w on the kernel-per-statement path (2, 3, 4);
 *   generic_solvers (0): 1 sends storm_hip_krylov_solve through the engine even where a fused loop exists;
 *   cheb_fused (1): storm_hip_cheb_apply runs its fused step kernel where it applies (fp64 records, no CSR tail); 0: the
 *              statement path everywhere (the same bits);
 *   recycle_fused (1): storm_hip_recycle_guess / _update run their fused kernels; 0: the same recipe out of library launchers
 *              (the same bits; counters "recycle_fused_launches" / "recycle_statement_launches");
 *   cg_fuse (1), cg_march (8), cg_march_fill (2048): the SpMV launch of a tiled format-4 operator ends the previous CG
 *              iteration (x += alpha p, p = r + beta p) itself, as blocks marching through this many planes (0: tiles), fewer
 *              planes per block on small lattices so that the grid holds about cg_march_fill blocks (0: as given);
 *   cg_residual_march (1), cg_residual_planes (1), cg_residual_chunk (16), cg_residual_fill (512): on one rank that loop's
 *              r -= alpha z recomputes z = A p from p instead of reading a stored z back (the same bits); by blocks that
 *              own a 2 048-row run of a plane and march through cg_residual_chunk planes where every plane is whole such
 *              runs (fewer planes on small lattices: about cg_residual_fill blocks; 0: as given), else -- and with
 *              cg_residual_planes 0 -- by gathers in the streaming kernel's grid;
 *   cg_pz_fold (1): the plane march also folds the step kernel's per-wave partials of <p,z> itself, under its first loads,
 *              where one pass folds them (at most 8 192): two launches an iteration instead of three (0: a one-block launch
 *              folds them in between).  The same bits;
 *   cg_rr_fold (1): on that road the plane march ends at the group sums of <r,r> (at most 256 groups of 64 slots) and the
 *              NEXT iteration's step kernel folds them under its first loads and forms beta, the convergence outcome and the
 *              iteration counter in every block (its first block stores them); a one-wave launch does it behind the last
 *              iteration of a solve (0: the plane march's last block draws a top-level ticket, folds and runs the scalar
 *              step).  The same bits;
 *   fused_reduce (1), lin_fuse (1), ticket_reduce (1): engine reductions finished by the partials kernel's last block; two
 *              consecutive vector statements as one pass; fused-loop reductions finished inside the producing kernels;
 *   nontemporal (1), blas1_nt (1): non-temporal record / y traffic of the SpMV; of the BLAS-1 and solver kernels (0 never,
 *              2 always, 1 for vectors of at least 6 * 2^20 rows: shorter ones survive in the Infinity Cache between kernels);
 *   lazy_statements (0): HOST loops -- storm_hip_copy / _scale / _axpy / _xpay / _axpbz and storm_hip_op_apply are not
 *              launched when called but wait, in program order, for the call that needs their result; two consecutive linear
 *              statements leave as ONE pass, and a storm_hip_dot / _norm2 over a vector the last waiting statement writes
 *              rides in that statement's kernel (`x += alpha p; r -= alpha z; <r, r>`: one kernel; `z = A p; <p, z>`: the
 *              apply with its fused-dot epilogue).  Every other entry point launches what waits first, so nothing is
 *              observed out of order; nothing waits inside a solver's operator / preconditioner callback.  The
 *              linear statements and their reductions give the eager kernels' values bit for bit; the apply's fused dot
 *              sums in the SpMV kernel's order (equal to rounding) (csrc/lazy.hip).  A statement neither the last one
 *              nor the sum depends on keeps waiting (the x-update above, when `<r, r>` is asked for).  Value 2 adds the
 *              library's fused CG step for a host loop: `x += alpha p; ...; p <<= r + beta p; z = A p; <p, z>` on a lattice
 *              operator is ONE launch (x, the new p, z and the sum: 56 B/row, the device loop's kernel, its FMA roundings);
 *              the new p is written to a spare vector whose storage p's handle then takes over -- never for a vector whose
 *              address storm_hip_vec_device_ptr has handed out.  The host loops of Storm.hpp / api.py switch level 2 on
 *              for their duration (IterativeSolver::lazy_statements).
 * RCCL transport:
 *   rccl_fused (1), rccl_ticket (1): the fused CG step on a partitioned lattice operator (the boundary planes of the new
 *              direction packed by a small kernel and sent under the marching launch); local sums finished in the kernels
 *              (CG's <r, r>; BiCGStab's |r|^2 and <rt, r>, whose alpha and omega the update kernels form themselves from
 *              the all-reduced sums -- no scalar-step launch behind those all-reduces);
 *   rccl_early_halo (1): BiCGStab -- the boundary planes of s and of the new direction are formed by a small kernel and sent
 *              before the update kernel that forms the vector runs.  The same bits;
 *   rccl_flag_wait (1): the boundary rows of an apply are released by a flag in device memory (set by a one-thread kernel
 *              behind the send / recv group on the comm stream, polled by a one-thread kernel in front of the boundary
 *              launch; bounded: 10 s, then STORM_HIP_E_COMM from the next call) instead of a cross-stream event, which costs
 *              ~15 us between "exchange done" and "boundary rows start" on this platform (5 us with the flag).  The same bits.
 * Instrumentation: profile_spmv (HIP-event pair around every SpMV launch), profile_comm (RCCL path: device timestamps
 *   around every step of an exchange and every all-reduce), resident_profile (the resident kernels time their phases),
 *   ticket_verify (k > 0: every k-th iteration the fused loops recompute their in-kernel reductions by the two-launch path
 *   and compare on the device).
 * Test hooks (not options: they exist so that tests can force a path or compare a kernel with its plainer form):
 *   coop_force_fail (1: cooperative launches "fail"; 2: cooperative kernels "gave up"), ticket_verify_inject,
 *   test_disable (a bit mask; every bit switches ONE refinement off, the plain form must give the same bits: 1 the chain
 *   kernel's own operator apply, 2 its prefetch under the all-reduce, 4 the resident path's coefficient cache, 8 its halo
 *   interleave, 16 awaited publishing exchanges of the latency path, 32 ordinary launch of the one-kernel paths, 64 downward
 *   marching of odd z-chunks). */
int storm_hip_ctx_set_option(storm_hip_ctx *ctx, const char *key, int64_t value);

/* Which path the solves of this context took so far (no reference counterpart: a diagnostic of this library; the
 * reference logs one line per solve, Solver.hpp:144-145).  Keys: "resident_solves" (csrc/resident.hip),
 * "latency_solves" (csrc/latency.hip: one cooperative kernel per solve), "latency_pre_solves" (those of them that were CG with
 * a preconditioner, option latency_pre: such a solve moves both and neither "engine_solves" nor the cheb_*_applies), "throughput_solves" (a kernel per statement,
 * fused loops of csrc/solver_cg.hip, solver_bicgstab.hip, solver_gmres.hip), "engine_solves" (csrc/krylov_abi.hip), "jfnk_inner_solves" (inner BiCGStab solves of
 * STORM_HIP_JFNK), "fd_fused_dots" (products of a finite-difference operator whose difference statement took the method's
 * reductions of z along in its pass), "host_reductions" (calls of storm_hip_dot / _norm2 / _multi_dot / _multi_dot_end / _block_dot: the reduction
 * entry points that make the host wait for their sums -- a device-resident loop leaves it where it was), "block_solves" (storm_hip_solve_cg_block, csrc/block.hip), "op_face_updates" (storm_hip_op_set_face_weights, csrc/op_update.hip), "nt_stream_launches" (launch sites of the streaming kernels at which the host chose the non-temporal instance, option "blas1_nt": what the host chose, not what instructions that instance holds), "cheb_fused_applies" / "cheb_statement_applies" (storm_hip_cheb_apply by path), "cheb_reduced_applies" (... of reduced objects, counted in addition), "op_reduced_builds" / "op_reduced_refreshes" (csrc/op_reduced.hip: companions built; converted again behind storm_hip_op_set_face_weights), "cg_fused_steps" (solves whose CG step rode in
 * the SpMV launch), "lazy_fused_dots" / "lazy_fused_pairs" / "lazy_apply_dots" / "lazy_cg_steps" / "lazy_waiting" (option
 * lazy_statements: reductions that rode in a statement's kernel, pairs of statements that left as one pass, applies that
 * left with a fused dot, fused CG steps, statements waiting now).  On the peer-window transport, where the time of the exchanges went (ticks of 10 ns of the device's
 * real-time counter, and counts): "ipc_allreduce_wait_ticks" / "ipc_allreduces" (from a rank's own contribution being
 * stored to every rank's being read), "ipc_ack_wait_ticks" / "ipc_ack_waits" (a send waiting for the receivers to have
 * consumed the plane two exchanges back), "ipc_halo_slow_poll_ticks" / "ipc_halo_slow_polls" (halo values that had not
 * arrived when the boundary rows asked for them; thread-ticks).  On the RCCL transport with option "profile_comm" = 1
 * (one-thread stamp kernels around every step, both streams; setting the option restarts the sums): "rccl_prof_exchanges",
 * "rccl_prof_event_to_comm_ticks" (the compute stream has the vector ready -> the comm stream starts),
 * "rccl_prof_pack_ticks", "rccl_prof_sendrecv_ticks", "rccl_prof_unhidden_wait_ticks" (the exchange still running when the
 * interior rows had ended), "rccl_prof_resume_ticks" (exchange and interior rows done -> the boundary rows start),
 * "rccl_prof_allreduces", "rccl_prof_allreduce_ticks".  With option "resident_profile" = 1:
 * "resident_phase_mean_<k>" / "resident_phase_max_<k>" (csrc/resident.hip).  "option_spmv_dict": no counter but the
 * current value of option "spmv_dict", for a caller that builds one operator on fp64 records and restores the option. */
int storm_hip_ctx_get_counter(storm_hip_ctx *ctx, const char *key, int64_t *value);

/* A cell ordering from geometry: host preprocessing in the role METIS plays in the north star; the reference's hook
 * is UnstructuredMesh::permute (Mallard/MeshUnstructured.hpp:443-459, 557-612: entities renumbered, adjacency rows keep
 * their order).  centers: [n_cells][dim] cell centres (CellView::center, Mallard/Mesh.hpp:304-311).  order_out[i] = the
 * cell that becomes cell i.  mode 0: the lexicographic order of a LATTICE where the centres form a tensor-product
 * grid (a renumbered structured mesh gets its natural order -- and the lattice record formats -- back), else the
 * Z-order (Morton) curve of the centres; 1: Morton always; 2: lattice or an error.  *kind_out (nullable): 1 lattice,
 * 2 Morton.  No device is touched. */
int storm_hip_order_cells(int32_t dim, int64_t n_cells, const double *centers, int32_t mode, int64_t *order_out,
                          int32_t *kind_out);

/* ---- host-side meshes: the data either side of the path (SURVEY.md 8f row 4, 8e "Partitioning") -----------------
 * A storm_hip_mesh is a face graph in host memory -- exactly the arrays stormDivGrad's face loop reads
 * (Playground.cpp:119-129: face -> inner / outer cell, face area, cell centre, cell volume) plus the boundary faces,
 * and, for a rank's part of a partitioned mesh, its halo cells and halo plan.  No device is touched by any of these
 * calls; all are threaded (STORM_HIP_BUILD_THREADS).  stormruler_amd/io_tetgen.py and partition.py are the numpy
 * restatements they are checked against array for array. */
typedef struct storm_hip_mesh storm_hip_mesh;
typedef struct storm_hip_mesh_view {
  int32_t dim, n_nbrs;
  int64_t n_cells, n_halo, n_faces, n_bfaces;
  const int64_t *inner, *outer;   /* [n_faces] local cell ids in [0, n_cells + n_halo)             Mesh.hpp:269-280 */
  const double *area;             /* [n_faces]                                                      Mesh.hpp:254 */
  const double *center, *volume;  /* [(n_cells + n_halo) * dim], [n_cells + n_halo]                 Mesh.hpp:304-311 */
  const int64_t *b_cell;          /* [n_bfaces] owning cell of a labelled (boundary) face */
  const double *b_area, *b_center;/* [n_bfaces], [n_bfaces * dim] */
  const int64_t *global_id;       /* [n_cells + n_halo] or NULL (an unpermuted single-rank mesh: the identity) */
  const int32_t *halo_owner;      /* [n_halo] or NULL */
  const int32_t *nbr_rank;        /* halo plan, as storm_hip_op_set_halo takes it */
  const int64_t *send_ptr, *send_idx, *recv_ptr;
} storm_hip_mesh_view;

/* `read_mesh_from_tetgen(mesh, path)`  Mallard/IoTetgen.hpp:44-235, both branches: <prefix>.node / .edge / [.face] /
 * .ele (prefix ends with ".1." or ".1"; '#' comments; zero-based ids used as written), then the face graph the
 * reference's insert() calls build (MeshUnstructured.hpp:350-425, 509-554: listed sides keep file order and their
 * marker as label, unlisted ones are created by the first cell that owns them in the order of Triangle::edges() /
 * Tetrahedron::faces() with label 0; inner = first owner, outer = second, which must see the side reversed;
 * interior = label 0).  dim = mesh_dim_v<Mesh> the caller expects (2, 3; 0 = what the node file says): a mismatch is the
 * reference's I/O error.  Errors (missing file, short file, bad header, bad topology) return STORM_HIP_E_INVALID with
 * the reference's message (STORM_THROW_IO -> std::runtime_error, Crow/Base/Exception.hpp:35-44).  Geometry:
 * Shape.hpp:155-167, 242-247, 309-321, 598-607; the tetrahedron's volume |det| / 6 is this build's own (the reference
 * has no volume(Tetrahedron): SURVEY.md headline fact 4). */
int storm_hip_mesh_read_tetgen(const char *prefix, int32_t dim, storm_hip_mesh **out);
/* The same face graph from arrays in memory: pos[n_nodes * dim], listed[n_listed * dim] (+ listed_label[n_listed] or
 * NULL = all 0), cells[n_cells * (dim + 1)]. */
int storm_hip_mesh_from_simplices(int32_t dim, int64_t n_nodes, const double *pos, int64_t n_listed, const int64_t *listed,
                                  const int64_t *listed_label, int64_t n_cells, const int64_t *cells, storm_hip_mesh **out);
/* Writes the four files in the format above (doubles in the shortest form that round-trips; 3-D: an .edge file
 * with no entries).  Test / bench infrastructure: the reference only reads. */
int storm_hip_mesh_write_tetgen(const char *prefix, int32_t dim, int64_t n_nodes, const double *pos, int64_t n_listed,
                                const int64_t *listed, const int64_t *listed_label, int64_t n_cells, const int64_t *cells);
/* A mesh from face-graph arrays the caller already has (copied); global_id / halo_owner may be NULL when n_halo == 0. */
int storm_hip_mesh_create(int32_t dim, int64_t n_cells, int64_t n_halo, int64_t n_faces, const int64_t *inner,
                          const int64_t *outer, const double *area, const double *center, const double *volume,
                          int64_t n_bfaces, const int64_t *b_cell, const double *b_area, const double *b_center,
                          const int64_t *global_id, const int32_t *halo_owner, storm_hip_mesh **out);
/* Pointers into the mesh's own arrays: valid until the mesh is permuted or destroyed. */
int storm_hip_mesh_get_view(const storm_hip_mesh *mesh, storm_hip_mesh_view *view);
/* `UnstructuredMesh::permute`  MeshUnstructured.hpp:443-459 for cells: new cell i is old cell order[i]; faces keep
 * their order and their inner / outer roles; halo cells keep their slot; global_id follows (and is created for a
 * single-rank mesh, so a later partition still knows the original ids). */
int storm_hip_mesh_permute_cells(storm_hip_mesh *mesh, const int64_t *order);
/* Cell -> rank maps (the reference has no partitioner, METIS is not in the image): recursive coordinate
 * bisection -- the longest axis of a part's bounding box cut at the k-th smallest (coordinate, cell id), k
 * proportional to the ranks on either side, any n_parts -- and slabs along one axis (contiguous ranges of the cells
 * ordered by (coordinate, cell id): k whole planes per rank for a structured box of k * n_parts planes). */
int storm_hip_partition_rcb(int32_t dim, int64_t n_cells, const double *centers, int32_t n_parts, int32_t *part_out);
int storm_hip_partition_slabs(int32_t dim, int64_t n_cells, const double *centers, int32_t axis, int32_t n_parts,
                              int32_t *part_out);
/* A rank's part of a single-rank mesh: its owned cells in ascending id, then the halo cells grouped by owner rank,
 * each group in ascending global id; every face that touches an owned cell, in mesh order; the boundary faces of the
 * owned cells; and the halo plan -- towards neighbour q the owned cells that share a face with one of q's cells, in
 * ascending global id (= q's halo group for this rank: no index lists are ever exchanged). */
int storm_hip_mesh_partition(const storm_hip_mesh *global_mesh, const int32_t *part, int32_t n_parts, int32_t rank,
                             storm_hip_mesh **out);
/* (Re)computes the halo plan of a local mesh built with storm_hip_mesh_create from its global ids and halo owners. */
int storm_hip_mesh_halo_plan(storm_hip_mesh *mesh, int32_t rank);
/* storm_hip_op_create_from_mesh on the mesh's arrays + storm_hip_op_set_halo with its halo plan. */
int storm_hip_op_create_from_mesh_object(storm_hip_ctx *ctx, const storm_hip_mesh *mesh, storm_hip_op **out);
int storm_hip_mesh_destroy(storm_hip_mesh *mesh);

/* Halo plan of a row-partitioned operator.  For neighbour q
 * (rank nbr_rank[q]) the owned rows send_idx[send_ptr[q] .. send_ptr[q+1]) are
 * sent, and the halo rows n_owned + [recv_ptr[q] .. recv_ptr[q+1]) received;
 * both sides order a segment by global cell id. */
int storm_hip_op_set_halo(storm_hip_op *op, int n_nbrs, const int32_t *nbr_rank,
                          const int64_t *send_ptr, const int64_t *send_idx,
                          const int64_t *recv_ptr);

/* `Operator::mul(y, x)`  Solvers/Operator.hpp:74:  y = beta*x + alpha*M(x).
 * Exchanges x's halo first when a halo plan is set.  x and y must not alias.
 * PRECONDITION: x is finite.  An Inf / NaN in x reaches the rows the reference's face loop lets it reach, and --
 * in the paired record format (spmv_dict = 3: two rows share their gathers; a row without a neighbour in a
 * shared slot multiplies the gathered value by weight 0) -- additionally rows whose index is one stencil
 * offset away from it without being its neighbour; rows stored in the CSR tail form a_ii x_i as
 * rowsum x_i - sum_j a_ij x_i, which is NaN instead of Inf for x_i = Inf.  Nothing else differs
 * (tests/test_gpu_edge_cases.py pins this). */
int storm_hip_op_apply(const storm_hip_op *op, double alpha, double beta, const storm_hip_vec *x,
                       storm_hip_vec *y);

/* `Operator::mul(y, x)` (Solvers/Operator.hpp:74) on a block of k columns (see "block vectors"): Y_j = beta X_j +
 * alpha M(X_j) for every column, the operator's records streamed ONCE -- by bytes 96 + 16 k per row instead of 112 k.
 * Column j of Y is, bit for bit, what storm_hip_op_apply gives for column j of X.  X and Y must not alias.  Needs
 * fp64 records (an operator built with option spmv_dict = 0; with or without a CSR tail): an operator in a compact
 * record format, one with a halo plan, or a context with a communicator returns STORM_HIP_E_UNSUPPORTED.  Sizes that
 * are not n_rows * k, k outside 1..8 and aliasing return STORM_HIP_E_INVALID. */
int storm_hip_op_apply_block(const storm_hip_op *op, double alpha, double beta, int k, const storm_hip_vec *X,
                             storm_hip_vec *Y);

/* d_i = diagonal entry i of beta*I + alpha*M; with invert != 0 its safe inverse (0 -> 0,
 * Crow/MathUtils.hpp:54-58).  What `Preconditioner::build(x, b, op)` (Preconditioner.hpp:70-72) of a
 * Jacobi preconditioner needs from the operator. */
int storm_hip_op_get_diagonal(const storm_hip_op *op, double alpha, double beta, int invert, storm_hip_vec *d);

/* `stormDivGrad(mesh, u, dt, c)`  source_apps/playground/Playground.cpp:115-131 in its own form:
 * u += dt * M(c)  (y += alpha*M(x)); what the playground's operator lambda calls twice per apply
 * (:153-167).  Exchanges x's halo first when a halo plan is set.  x and y must not alias. */
int storm_hip_op_apply_add(const storm_hip_op *op, double alpha, const storm_hip_vec *x, storm_hip_vec *y);

/* The playground's operator lambda (Playground.cpp:153-167) -- two stormDivGrad calls per apply -- as ONE operator: its
 * linear part is the two-stage operator
 *     A x = beta2 x + alpha2 M (beta1 x + alpha1 M x),      beta1 = sigma, alpha1 = -Gamma, beta2 = 1, alpha2 = -tau.
 * Computes t = beta1 x + alpha1 M x (the lambda's w_hat minus its constant part) and y = beta2 x + alpha2 M t.  t may be
 * NULL (a pooled work vector is used).  y and t are, bit for bit and in every record format, what
 *     storm_hip_op_apply(op, alpha1, beta1, x, t);  storm_hip_copy(y, x);  storm_hip_scale(y, beta2);
 *     storm_hip_op_apply_add(op, alpha2, t, y)
 * give.  x, t and y must be pairwise distinct (STORM_HIP_E_INVALID, as sizes that differ from the operator's).  An
 * operator with a halo plan or a context with a communicator returns STORM_HIP_E_UNSUPPORTED. */
int storm_hip_op_apply2(const storm_hip_op *op, double alpha1, double beta1, double alpha2, double beta2,
                        const storm_hip_vec *x, storm_hip_vec *t, storm_hip_vec *y);

typedef struct storm_hip_op_stats {
  int64_t n_rows, n_cols, nnz_offdiag;  /* off-diagonal entries (2F for a face graph) */
  int64_t ell_slots;                    /* stored ELL slots incl. padding */
  int64_t tail_nnz, tail_rows;          /* CSR tail */
  int64_t n_slices, max_row_len;
  int64_t n_interior_slices;            /* slices whose rows reference no halo column */
  int64_t device_bytes;
  int64_t record_bytes;                 /* bytes of the slice records as stored (format 4: 8 per row, kept whether or not the row-record index is used) */
  int64_t value_dictionary_size;        /* > 0: weights stored as byte indices into this many distinct values */
  int64_t offset_dictionary_size;       /* > 0: columns stored as byte indices into this many distinct col - row */
  int64_t paired_rows;                  /* 1: two consecutive rows per lane share their 16-byte gathers; n_slices then counts 128-row groups; 2: the same with one common offset order (format 4); 3: format 5 (one byte per row) */
  int64_t tiled_planes;                 /* > 0: an unsplit apply runs the tiled format-4 kernel (lattice offsets -b,-a,-1,+1,+a,+b): tiles of 1024 rows x this many planes */
  int64_t spmv_blocks;                  /* workgroups of an unsplit apply */
  int64_t xcd_run_blocks;               /* (ABI 6) fp64-record kernel: runs of this many workgroups (256 rows each) go to one XCD */
  int64_t streamed_record_bytes;        /* (ABI 6) record bytes one apply actually reads: record_bytes, or with the row-record index (format 4 on a lattice, <= 256 distinct row words, option spmv_record_index) one byte per row + the table of words */
} storm_hip_op_stats;
int storm_hip_op_get_stats(const storm_hip_op *op, storm_hip_op_stats *stats);
int storm_hip_op_destroy(storm_hip_op *op);

/* ---- whole-solver entry points --------------------------------------------
 * `solve<XSolver>(x, b, op)`  Solvers/Solver.hpp:261-265 for the operator
 * A = beta*I + alpha*M, with the reference's public knobs (Solver.hpp:66-72,
 * 158-159) and exactly its convergence rule (Solver.hpp:116-147): early exit
 * iff abs_tol > 0 && |r0| < abs_tol; then per iteration converged iff
 * (abs_tol > 0 && abs < abs_tol) || (rel_tol > 0 && abs/|r0| < rel_tol);
 * `iterations` = number of iterate() calls.  The loops run device-resident:
 * scalars (alpha, beta, rho, omega, Givens) never visit the host, and the
 * host polls the device's `done` flag `check_lag` iterations behind. */
typedef struct storm_hip_solver_params {
  int64_t num_iterations;           /* default 2000  (Solver.hpp:67) */
  double absolute_error_tolerance;  /* default 1e-6  (Solver.hpp:71) */
  double relative_error_tolerance;  /* default 1e-6  (Solver.hpp:72) */
  int64_t num_inner_iterations;     /* GMRES restart m, default 50 (Solver.hpp:159) */
  int32_t check_lag;                /* 0 = default (4) */
  int32_t gram_schmidt;             /* GMRES: 0 = modified (reference, SolverGmres.hpp:157-160), 1 = classical x2 */
} storm_hip_solver_params;

typedef struct storm_hip_solver_result {
  int64_t iterations;
  double absolute_error, relative_error, initial_error;
  int32_t converged;
  int32_t path_fallback;  /* 0: the path the library chose ran; 1: a cooperative (one-kernel) path could not be launched and
                             the solve ran on the kernel-per-statement path instead; 2: a cooperative kernel's bounded wait
                             gave up (the device shared with another cooperative kernel) -- x was restored and the solve
                             re-run on the kernel-per-statement path.  Same results either way (to rounding). */
  int64_t num_applies;
} storm_hip_solver_result;

void storm_hip_solver_params_default(storm_hip_solver_params *p);

/* history: NULL or room for num_iterations + 1 residual norms (entry 0 = initial). */
int storm_hip_solve_cg(const storm_hip_op *op, double alpha, double beta, const storm_hip_vec *b,
                       storm_hip_vec *x, const storm_hip_solver_params *params,
                       storm_hip_solver_result *result, double *history);       /* SolverCg.hpp:47-128 */
int storm_hip_solve_bicgstab(const storm_hip_op *op, double alpha, double beta, const storm_hip_vec *b,
                             storm_hip_vec *x, const storm_hip_solver_params *params,
                             storm_hip_solver_result *result, double *history); /* SolverBiCgStab.hpp:52-167 */
int storm_hip_solve_gmres(const storm_hip_op *op, double alpha, double beta, const storm_hip_vec *b,
                          storm_hip_vec *x, const storm_hip_solver_params *params,
                          storm_hip_solver_result *result, double *history);    /* SolverGmres.hpp:41-255 */

/* `solve<CgSolver>(c_hat, c, lambda)`  Playground.cpp:151-167 for the linear part of the lambda, the two-stage operator
 * A = beta2 I + alpha2 M (beta1 I + alpha1 M) of storm_hip_op_apply2: SolverCg.hpp:54-126 under the rule of
 * Solver.hpp:116-147.  num_applies = iterations + 1 (one apply is both stages).  A small halo-free operator runs as ONE
 * cooperative kernel per solve (csrc/latency.hip, three synchronisation points per iteration; counted by
 * "latency_solves"), under the rules of storm_hip_solve_cg's one-kernel path (options latency_path, latency_rows;
 * path_fallback); everything else runs the engine's CG loop with the two stages as library launches ("engine_solves").
 * Halo plan / communicator: STORM_HIP_E_UNSUPPORTED. */
int storm_hip_solve_cg2(const storm_hip_op *op, double alpha1, double beta1, double alpha2, double beta2,
                        const storm_hip_vec *b, storm_hip_vec *x, const storm_hip_solver_params *params,
                        storm_hip_solver_result *result, double *history);

/* k independent CG solves A x_j = b_j on the columns of a block (see "block vectors"): SolverCg.hpp:54-126 per column,
 * the convergence rule of Solver.hpp:116-147 per column, the operator's records streamed once per iteration for all
 * columns (storm_hip_op_apply_block; the same operators are refused).  Every column has its own gamma, alpha, beta,
 * residual norms and done flag on the device; the statements are rounded as storm_hip_solve_cg's kernel-per-statement
 * loop rounds them (fma(alpha, p, x), fma(-alpha, z, r), fma(beta, p, r)).  A column that has converged -- or left at
 * once by abs_tol > 0 && |r0| < abs_tol -- is frozen: its x keeps the value of the iteration where it stopped, its
 * `iterations` stays there, and nothing it holds reaches another column.  results[k]; histories: NULL or
 * k * (num_iterations + 1) doubles, column j's residual norms at histories[j * (num_iterations + 1) ...] (entry 0 =
 * initial; iterations + 1 norms, zeros behind them).  Counted by "block_solves" (storm_hip_ctx_get_counter). */
int storm_hip_solve_cg_block(const storm_hip_op *op, double alpha, double beta, int k, const storm_hip_vec *B,
                             storm_hip_vec *X, const storm_hip_solver_params *params,
                             storm_hip_solver_result *results, double *histories);

/* ---- the general Krylov engine ---------------------------------------------
 * Every solver of Solvers/  for ANY operator, device-resident:
 *   storm_hip_krylov_* objects stand in for the reference's solver objects (`CgSolver<Vector> s;`,
 *   Solvers/Solver.hpp:66-76): they hold the operator, the optional preconditioner (`pre_op`, `pre_side`,
 *   Solver.hpp:74-75) and the work vectors.
 * Operator and preconditioner are either native (a storm_hip_op / a diagonal held in a vector) or a
 * CALLBACK -- the reference's only call site passes a lambda through make_operator
 * (Playground.cpp:151-167, Operator.hpp:125-200).  A callback computes y = A(x) by calling this
 * library (storm_hip_op_apply, storm_hip_op_apply_add, BLAS-1 ...): those calls only ENQUEUE work on the
 * context's stream, so the solver loop around them never waits for the device -- every scalar of the
 * recurrences (alpha, beta, rho, omega, the IDR/BiCGStab(l) small systems, Hessenberg + Givens) stays in
 * HBM, the convergence rule of Solver.hpp:132-140 is evaluated there, and the host polls a pinned flag
 * `check_lag` iterations behind.  A callback that itself waits (storm_hip_dot ...) is still correct.
 * While a callback runs, the library calls it makes are predicated on the solve's `done` flag, so work
 * enqueued past convergence costs nothing.  Return 0 from a callback; anything else aborts the solve with
 * STORM_HIP_E_INVALID. */
typedef struct storm_hip_krylov storm_hip_krylov;
typedef int (*storm_hip_apply_fn)(void *user, storm_hip_vec *y, const storm_hip_vec *x);

enum storm_hip_method {
  STORM_HIP_CG = 0,          /* SolverCg.hpp:47-128 */
  STORM_HIP_BICGSTAB = 1,    /* SolverBiCgStab.hpp:52-167 */
  STORM_HIP_GMRES = 2,       /* SolverGmres.hpp:281-283 */
  STORM_HIP_FGMRES = 3,      /* SolverGmres.hpp:306-308 */
  STORM_HIP_CGS = 4,         /* SolverCgs.hpp:50-176 */
  STORM_HIP_TFQMR = 5,       /* SolverTfqmr.hpp:227-240 */
  STORM_HIP_TFQMR1 = 6,      /* SolverTfqmr.hpp:252-265 */
  STORM_HIP_BICGSTAB_L = 7,  /* SolverBiCgStab.hpp:184-383; num_inner_iterations = l (default 2) */
  STORM_HIP_IDRS = 8,        /* SolverIdrs.hpp:52-291;      num_inner_iterations = s (default 4) */
  STORM_HIP_RICHARDSON = 9,  /* SolverRichardson.hpp:41-98 */
  /* JfnkSolver, SolverNewton.hpp:101-173: Newton steps on A(x) = b for a NONLINEAR callback A (any operator kind is taken; a
   * native one is linear and one step lands on the answer).  init: w = A(x), r = b - w, |r| (:106-122).  iterate (:124-161):
   * mu = sqrt(eps) sqrt(1 + |x|) formed on the device; t = r; J(x) t = r by a nested BiCGStab object (tolerances 1e-8, 2000
   * iterations, no preconditioner, :133-135) on the finite-difference operator of storm_hip_krylov_set_operator_fd at (x, w,
   * mu); x += t; w = A(x); r = b - w; |r|.  No scalar visits the host: the inner solve's own polling is the only host
   * involvement inside a step.  iterations counts Newton steps, num_applies every application of A (outer and inner);
   * storm_hip_krylov_get_int "inner_iterations" the inner iterations.  A preconditioner that is set is IGNORED, as in the
   * reference (:107-109, :126-128 take pre_op and never read it).  A finite-difference operator as A is refused
   * (STORM_HIP_E_UNSUPPORTED). */
  STORM_HIP_JFNK = 10
};
enum storm_hip_side { STORM_HIP_LEFT = 0, STORM_HIP_RIGHT = 1, STORM_HIP_SYMMETRIC = 2 }; /* Preconditioner.hpp:39-60 */

int storm_hip_krylov_create(storm_hip_ctx *ctx, int method, storm_hip_krylov **out);
int storm_hip_krylov_destroy(storm_hip_krylov *k);
/* A = beta*I + alpha*M of a stencil operator (CG / BiCGStab / GMRES without preconditioner then run the fused
 * kernels of storm_hip_solve_*), or a callback. */
int storm_hip_krylov_set_operator(storm_hip_krylov *k, const storm_hip_op *op, double alpha, double beta);
int storm_hip_krylov_set_operator_fn(storm_hip_krylov *k, storm_hip_apply_fn apply, void *user);
/* z = (A(x + delta y) - w) / delta, delta = safe_divide(mu, |y|) (MathUtils.hpp:49-52: 0 when |y| == 0, and then z = 0):
 * the Jacobian-vector product of SolverNewton.hpp:143-156 as an operator any method can take (GMRES on a Jacobian, say).
 * Per product: <y, y> with delta and 1 / delta formed behind it on the device, s = x + delta y, the callback, and
 * z = (z - w) / delta with the reductions the method takes of z next in the same pass -- four launches, no host wait.
 * x and w = A(x) must stay alive and unchanged during a solve.  mu not finite or <= 0, x / w of different sizes or
 * contexts: STORM_HIP_E_INVALID. */
int storm_hip_krylov_set_operator_fd(storm_hip_krylov *k, storm_hip_apply_fn apply, void *user,
                                     const storm_hip_vec *x, const storm_hip_vec *w, double mu);
/* z = A(y) with the object's operator (any kind; Operator::mul, Operator.hpp:74), enqueued; no host wait.  z must not alias
 * y; not while a stepping solve is open on the object. */
int storm_hip_krylov_apply(storm_hip_krylov *k, const storm_hip_vec *y, storm_hip_vec *z);
/* "inner_iterations" (JFNK: total inner BiCGStab iterations of the last solve, SolverNewton.hpp:133-155). */
int storm_hip_krylov_get_int(const storm_hip_krylov *k, const char *key, int64_t *value);
/* The two-stage operator A = beta2 I + alpha2 M (beta1 I + alpha1 M) of storm_hip_op_apply2 (the playground's lambda,
 * Playground.cpp:153-167, without a callback): an apply is both stages as library launches, so every method and every
 * preconditioner side works on it; CG without preconditioner runs storm_hip_solve_cg2.  Halo plan / communicator:
 * STORM_HIP_E_UNSUPPORTED. */
int storm_hip_krylov_set_operator2(storm_hip_krylov *k, const storm_hip_op *op, double alpha1, double beta1, double alpha2,
                                   double beta2);
/* pre_op / pre_side.  fn == NULL removes it.  The diagonal form is y = d .* x (e.g. d from
 * storm_hip_op_get_diagonal(..., invert = 1): Jacobi); the vector must outlive the solves. */
int storm_hip_krylov_set_preconditioner_fn(storm_hip_krylov *k, storm_hip_apply_fn apply, void *user, int side);
int storm_hip_krylov_set_preconditioner_diag(storm_hip_krylov *k, const storm_hip_vec *d, int side);
/* Extra knobs: "relaxation_factor" (Richardson, default 1e-4, SolverRichardson.hpp:45). */
int storm_hip_krylov_set_real(storm_hip_krylov *k, const char *key, double value);
/* `Solver::solve(x, b, op)`: the whole solve, no host wait inside the loop.  num_applies counts operator
 * applications; *pre_applies (nullable) preconditioner applications. */
int storm_hip_krylov_solve(storm_hip_krylov *k, const storm_hip_vec *b, storm_hip_vec *x,
                           const storm_hip_solver_params *params, storm_hip_solver_result *result,
                           double *history, int64_t *pre_applies);
/* The reference's protected stepping interface (Solver.hpp:78-111): init returns |b - A x|, each iterate the
 * new residual norm (ONE host wait per call -- not per reduction); the caller owns the convergence decision,
 * as IterativeSolver::solve does; finalize after the last iterate.  `params` supplies num_inner_iterations /
 * gram_schmidt only. */
int storm_hip_krylov_init(storm_hip_krylov *k, const storm_hip_vec *b, storm_hip_vec *x,
                          const storm_hip_solver_params *params, double *initial_error);
int storm_hip_krylov_iterate(storm_hip_krylov *k, double *error);
int storm_hip_krylov_finalize(storm_hip_krylov *k);

/* ---- Chebyshev polynomial preconditioner -------------------------------------------------------------------------
 * z = p_m(diag(s) A) diag(s) r for A = beta I + alpha M and an optional scale s (e.g. the inverse diagonal; s = 1
 * without): Saad, Iterative Methods for Sparse Linear Systems, Alg. 12.1 started from zero, for an eigenvalue interval
 * [lmin, lmax] of diag(s) A.  With theta = (lmax + lmin) / 2, delta = (lmax - lmin) / 2, sigma = theta / delta,
 * rho_0 = 1 / sigma:
 *     d_0 = (s .* r) / theta,  z = d_0,  res = r;
 *     for k = 0 .. m-1:  res -= A d_k;  rho_{k+1} = 1 / (2 sigma - rho_k);
 *                        d_{k+1} = (rho_{k+1} rho_k) d_k + (2 rho_{k+1} / delta) (s .* res);  z += d_{k+1}
 * The residual polynomial is T_{m+1}((theta - lambda) / delta) / T_{m+1}(sigma).  Only operator applies and streaming
 * statements: no reduction, no host wait; a fixed linear operator (SPD where diag(s) A is and the interval holds its
 * spectrum), so every method and side may use it.  degree = m = operator products per apply, 1 .. 16.
 *
 * Two paths give the same bits (tests/test_gpu_cheb.py).  The STATEMENT path, for every record format, is this sequence
 * of library calls (d, e: the object's two direction buffers, swapped after every step; it = 1 / theta, a host double):
 *     d_0:      s given:  storm_hip_vmul(d, s, r);  storm_hip_axpbz(d, it, d, 0, d)      else  storm_hip_axpbz(d, it, r, 0, r)
 *     step k:   storm_hip_op_apply(op, alpha, beta, d, e)
 *               storm_hip_axpbz(res, 1, k == 0 ? r : res, -1, e)
 *               s given:  storm_hip_vmul(e, s, res);  storm_hip_axpbz(e, c1_k, d, c2_k, e)   else  storm_hip_axpbz(e, c1_k, d, c2_k, res)
 *               k == 0:   storm_hip_axpbz(z, 1, d, 1, e)                                       else  storm_hip_axpy(z, 1, e)
 * The FUSED path (option cheb_fused, default 1; operators on fp64 records -- built with option spmv_dict = 0 -- without
 * a CSR tail) is one streaming kernel for d_0 and one kernel per step that forms the row's product and updates res, the
 * direction and z on the row it holds: m + 1 launches instead of about 4 m + 1.  Counters "cheb_fused_applies" and
 * "cheb_statement_applies" (storm_hip_ctx_get_counter) say which path an apply took. */
typedef struct storm_hip_cheb storm_hip_cheb;
/* theta and the m pairs c1[k] = rho_{k+1} rho_k, c2[k] = 2 rho_{k+1} / delta.  Host code, needs no device.
 * STORM_HIP_E_INVALID unless 0 < lmin < lmax, both finite, 1 <= degree <= 16. */
int storm_hip_cheb_coefficients(double lmin, double lmax, int degree, double *theta, double *c1, double *c2);
/* Gershgorin's bound of diag(s) A, A = beta I + alpha M:  max_i |s_i| (|a_ii| + sum_k |alpha w_ik|); scale may be NULL
 * (s = 1).  Every record format, ELL records and CSR tail.  One host wait (build time).  Halo plan / communicator:
 * STORM_HIP_E_UNSUPPORTED. */
int storm_hip_op_gershgorin(const storm_hip_op *op, double alpha, double beta, const storm_hip_vec *scale,
                            double *lambda_max);
/* lmax <= 0: Gershgorin's bound is taken; lmin <= 0: lmax / 30 (the ratio hypre and Ifpack2 default to -- a default, not
 * a claim).  The object owns three work vectors; `op` and `dinv` (nullable) must outlive it -- applying an object
 * whose operator was destroyed is the caller's error.  Halo plan / communicator: STORM_HIP_E_UNSUPPORTED. */
int storm_hip_cheb_create(const storm_hip_op *op, double alpha, double beta, const storm_hip_vec *dinv, int degree,
                          double lmin, double lmax, storm_hip_cheb **out);
/* z = P(r); z must not alias r, r is not written.  Enqueues and never waits; inside a solver callback the kernels are
 * predicated on the solve's `done` flag like those of storm_hip_vmul and storm_hip_op_apply. */
int storm_hip_cheb_apply(const storm_hip_cheb *h, const storm_hip_vec *r, storm_hip_vec *z);
/* "lambda_min", "lambda_max" (the bounds in use, defaults resolved), "degree", "reduced" (1 for an object made by
 * storm_hip_cheb_create_reduced, 0 otherwise). */
int storm_hip_cheb_get(const storm_hip_cheb *h, const char *key, double *value);
int storm_hip_cheb_destroy(storm_hip_cheb *h);
/* pre_op as the library's Chebyshev preconditioner (h == NULL removes it): bound natively, no callback.  Its operator
 * need not be the solve's.  A size that differs from the solve's vectors: STORM_HIP_E_INVALID from the solve. */
int storm_hip_krylov_set_preconditioner_cheb(storm_hip_krylov *k, const storm_hip_cheb *h, int side);

/* ---- fp32-weight companion records ("reduced records") --------------------------------------------------------------
 * An operator on fp64 records (format 0: what any mesh gets; a box built with option spmv_dict = 0) can carry a second copy
 * of its ELL records and CSR tail values whose weights and diagonal terms are rounded to fp32: 256 + 512 W bytes per slice
 * of width W instead of 512 + 768 W.  It is a companion, not a format: only the entry points below read it, and every
 * other call on the operator -- apply, solves, block and fused paths -- keeps reading the fp64 records.  Its purpose is the
 * Chebyshev preconditioner, whose every step is an operator product: a preconditioner only has to be a fixed linear operator
 * close to the inverse, and the polynomial of the rounded operator is as good a one as the polynomial of A.
 *
 * THE CONTRACT.  w32 = (float)w is IEEE round-to-nearest-even; a weight is widened back to double, exactly, where a kernel
 * loads it.  Vectors, sums and every other operand stay fp64, every operation is the fp64 kernel's in the same order with the
 * same contraction.  So storm_hip_op_apply_reduced, storm_hip_op_gershgorin_reduced, storm_hip_cheb_apply of a reduced
 * object (either path) and a solve preconditioned by it give, BIT FOR BIT, what storm_hip_op_apply, storm_hip_op_gershgorin
 * and an ordinary Chebyshev object give on a fresh fp64-record operator built from double(float(w)), double(float(ext))
 * (tests/test_gpu_reduced.py).
 *
 * RANGE.  storm_hip_op_build_reduced converts on the device and makes one host wait: if a nonzero weight or diagonal term is
 * not finite or has a magnitude outside fp32's normal range [2^-126, FLT_MAX], it frees the companion and returns
 * STORM_HIP_E_UNSUPPORTED (the operator itself is untouched).  storm_hip_op_set_face_weights on an updatable operator that
 * has a companion enqueues the same conversion behind its refresh, so the companion is always the rounding of the current
 * fp64 records -- but it makes no host wait and reports no range check: there the range is the CALLER'S PRECONDITION.
 * A storm_hip_cheb made before a refresh keeps its bounds; rebuilding it is the caller's, as for an ordinary object.
 *
 * Refused with STORM_HIP_E_UNSUPPORTED: an operator that is not on fp64 records (a value / offset dictionary, paired rows,
 * a mixed operator); a halo plan, halo columns or a communicator; apply / gershgorin / cheb_create_reduced on an operator
 * without a companion (nothing is built behind the caller's back).  Counters (storm_hip_ctx_get_counter):
 * "op_reduced_builds", "op_reduced_refreshes", "cheb_reduced_applies" (beside "cheb_fused_applies" / "cheb_statement_applies").
 * storm_hip_op_destroy frees the companion; device_bytes of storm_hip_op_get_stats includes it. */
int storm_hip_op_build_reduced(storm_hip_op *op); /* idempotent */
int storm_hip_op_drop_reduced(storm_hip_op *op);  /* waits for the context's stream; no companion: a no-op */
/* bytes of the companion's records; 0: no companion */
int storm_hip_op_reduced_bytes(const storm_hip_op *op, int64_t *record_bytes);
/* y = beta x + alpha M~ x.  Enqueue-only (held-back lazy statements are launched first); inside a solver callback predicated
 * on the solve's `done` flag like storm_hip_op_apply.  y must not alias x and is not read. */
int storm_hip_op_apply_reduced(const storm_hip_op *op, double alpha, double beta, const storm_hip_vec *x, storm_hip_vec *y);
/* storm_hip_op_gershgorin from the companion records.  One host wait. */
int storm_hip_op_gershgorin_reduced(const storm_hip_op *op, double alpha, double beta, const storm_hip_vec *scale,
                                    double *lambda_max);
/* storm_hip_cheb_create whose object takes its operator products (and, with lmax <= 0, its Gershgorin default) from the
 * companion records.  storm_hip_cheb_apply runs the fused step on them where the fp64 fused step would run (option
 * cheb_fused on, no CSR tail), otherwise the statement sequence with storm_hip_op_apply_reduced in place of
 * storm_hip_op_apply: the same bits.  The solvers bind the object like any other.  Applying it after
 * storm_hip_op_drop_reduced: STORM_HIP_E_UNSUPPORTED. */
int storm_hip_cheb_create_reduced(const storm_hip_op *op, double alpha, double beta, const storm_hip_vec *dinv, int degree,
                                  double lmin, double lmax, storm_hip_cheb **out);

/* ---- Smoothed-aggregation multigrid preconditioner ------------------------------------------------------------------
 * z = B r: one symmetric V-cycle of smoothed-aggregation multigrid (Vanek, Mandel, Brezina 1996) for A = beta I + alpha M,
 * the one preconditioner of this library that removes operator products instead of making them cheaper.  Usable as pre_op
 * of every method and side like storm_hip_cheb: it enqueues and never waits, has no reduction and no host wait inside an
 * apply.  Single rank.  For symmetric (or diagonally symmetrisable) operators: for a strongly non-symmetric operator, upwind
 * convection-diffusion for instance, use the Jacobi smoother (storm_hip_amg_create_smoother below).  Added within ABI 6
 * (STORM_HIP_HAS_AMG).
 *
 * THE RECIPE (normative; tests/amg_ref.py restates it).  A level operator A_l is CSR with sorted columns, duplicates
 * merged, exact zeros dropped and an explicit diagonal.
 *   1. Strength.  m_i = max_{j != i} |a_ij|.  The pair (i, j), j != i, is strong if a_ij != 0 and |a_ij| >= theta m_i, or the
 *      same holds for (j, i): the union of both directions.  Its weight is max(|a_ij|, |a_ji|), a missing entry counting 0.
 *   2. Aggregation, three sequential passes in row order.  Pass 1: a row that has a strong neighbour and is unaggregated
 *      together with all of them founds an aggregate with them.  Pass 2: every row still free joins the aggregate -- as it
 *      stood after pass 1 -- of its strong neighbour of largest weight that pass 1 aggregated; ties go to the lowest
 *      column.  Pass 3: every row still free founds an aggregate with its still-free strong neighbours.  Aggregates are
 *      numbered in order of creation.
 *   3. Filtered matrix A^F: strong off-diagonal entries are kept, weak ones are added to the diagonal,
 *      a^F_ii = a_ii + sum_weak a_ij.  A zero a^F_ii: STORM_HIP_E_INVALID.
 *   4. Prolongator P = T - (omega / lambda_F) D_F^-1 A^F T with T_iI = 1 for row i in aggregate I and
 *      lambda_F = max_i sum_j |a^F_ij| / |a^F_ii|; rows sorted by column, exact zeros dropped.  omega = 0: P = T.  R = P^T is
 *      stored explicitly.  (Smoothing with the FILTERED matrix keeps the coarse operators sparse on anisotropic weights.)
 *   5. Coarse operator A_{l+1} = P^T A_l P.
 *   6. Stop when n_l <= coarse_rows; also when the next level would keep more than 90 % of the rows, or when max_levels
 *      is reached -- in these two cases a level of at most 1024 rows becomes the coarsest, otherwise the result is
 *      STORM_HIP_E_UNSUPPORTED with the level sizes in the message.
 *   7. The coarsest level's dense inverse is formed on the host by Gauss-Jordan with partial pivoting.  A zero pivot, a
 *      pivot below 2^-40 max_i |a_ii| in magnitude (singular to working precision: what rounding leaves of a zero pivot) or
 *      a non-finite entry -- a pure-Neumann operator, for instance --: STORM_HIP_E_INVALID, and the message says so.  (For
 *      operators whose kernel is the constants there is storm_hip_amg_setup_csr_nullspace below.)
 *
 * THE CYCLE for level l with right-hand side r and output z (S_l: the level's Chebyshev smoother with the Jacobi scale,
 * degree smoother_degree, on [lmax / smoother_ratio, lmax] with Gershgorin's lmax; t, e: the level's work vectors):
 *     z  = S_l(r)                 storm_hip_cheb_apply
 *     t  = r - A_l z              storm_hip_op_apply(op_l, alpha_l, beta_l, z, t); storm_hip_axpbz(t, 1, r, -1, t)
 *     rc = R_l t                  acc = 0; acc = fma(w_k, t[c_k], acc) over the row's entries in column order
 *     zc = cycle(l + 1, rc)       coarsest level: zc = Ainv rc, row i: lane j of a wavefront sums columns j, j + 64, ... by fma,
 *                                 then the wavefront's tree sum
 *     z  = z + P_l zc             the same sum, then z_i + acc
 *     t  = r - A_l z
 *     e  = S_l(t);  z = z + e     storm_hip_cheb_apply; storm_hip_axpy(z, 1, e)
 * With option amg_fused (default 1) the residual on a level with fp64 records and no CSR tail is ONE kernel that gives the
 * bits of the two statements; amg_fused = 0 takes the statements everywhere, and with cheb_fused = 0 as well the cycle holds
 * no fused kernel but the transfers.  All settings give the same bits (tests/test_gpu_amg.py).  Counters
 * (storm_hip_ctx_get_counter): "amg_applies", "amg_fused_residuals", "amg_statement_residuals".  About 11 launches per level:
 * small meshes are launch-bound.
 *
 * THE TAIL (option amg_tail, default 0; csrc/amg_tail.hip).  With amg_tail = 1 the cycle from a level t down to the coarsest
 * level and back up to t is ONE cooperative kernel: the statements above, in their order, as phases between grid barriers, each
 * row through the device functions the launched kernels call -- the same bits (tests/test_gpu_amg_tail.py).  t is the first
 * level with at most amg_tail_rows rows (option; default 0 = no level, see below) from which every level is eligible: fp64 records, no CSR tail,
 * no compact format, option amg_fused on; level 0 of a null-space object is never eligible (its projections stay launches); a
 * tail of the coarsest level alone is not taken.  Levels above t stay launches; when the whole hierarchy is small t = 0 and
 * an apply is one launch.  Both smoothers, fp64 and reduced records, plain, refreshable (a refresh drops the kernel's tables)
 * and null-space objects, inside a solve and stand-alone.  A launch that is refused takes the launches for that apply.  Should
 * a wait inside the kernel give up (10 s; a device shared with another cooperative kernel), a solve is re-run without the tail
 * (storm_hip_solver_result::path_fallback 2); after a stand-alone storm_hip_amg_apply the next storm_hip_ctx_sync returns
 * STORM_HIP_E_HIP, and z of that apply is UNDEFINED.  Counters "amg_tail_applies" (applies whose tail ran as the kernel;
 * the per-path counters above do not move for its levels) and "amg_tail_refusals"; storm_hip_amg_get keys "tail_level" (t
 * under the current amg_tail_rows, -1: none; the coarsest level's index: no tail is taken), "tail_blocks", "tail_barriers".
 * MEASURED (profiles/INDEX_r34.md): the kernel is SLOWER than the launches at every level size tried, 1.3x to 3x -- a phase
 * costs three dependent trips through the fabric (coherent gathers, the publishing exchange, the barrier) where a launch on a
 * warm stream costs about 2 us.  Hence amg_tail_rows = 0 by default: amg_tail = 1 changes nothing until a size is named. */
#define STORM_HIP_HAS_AMG 1
typedef struct storm_hip_amg_params {
  double strength_theta;    /* 0.25 */
  double prolongator_omega; /* 4/3; 0: the unsmoothed, piecewise-constant prolongator */
  int32_t smoother_degree;  /* 2 (1 .. 16) */
  double smoother_ratio;    /* 30: lmin = lmax / ratio, the Chebyshev object's default */
  int32_t max_levels;       /* 10 */
  int32_t coarse_rows;      /* 512 (1 .. 1024) */
  int32_t reduced_records;  /* 0; 1: every level's smoother reads fp32-weight companion records of its operator */
} storm_hip_amg_params;
typedef struct storm_hip_amg_hierarchy storm_hip_amg_hierarchy;
typedef struct storm_hip_amg storm_hip_amg;
void storm_hip_amg_params_default(storm_hip_amg_params *params);
/* The hierarchy of assembled CSR (any column order, duplicates are summed).  HOST CODE: needs no context and no device.
 * params == NULL: the defaults. */
int storm_hip_amg_setup_csr(int64_t n_rows, const int64_t *row_ptr, const int64_t *col, const double *val,
                            const storm_hip_amg_params *params, storm_hip_amg_hierarchy **out);
int storm_hip_amg_hierarchy_destroy(storm_hip_amg_hierarchy *h);
int storm_hip_amg_hierarchy_levels(const storm_hip_amg_hierarchy *h, int *levels);
/* rows and entries of A_l; aggregates and entries of P_l (both 0 on the coarsest level) */
int storm_hip_amg_hierarchy_level_sizes(const storm_hip_amg_hierarchy *h, int level, int64_t *n_rows, int64_t *nnz_a,
                                        int64_t *n_aggregates, int64_t *nnz_p);
/* A_l as CSR into the caller's arrays ([n_rows + 1], [nnz_a], [nnz_a]) */
int storm_hip_amg_hierarchy_get_operator(const storm_hip_amg_hierarchy *h, int level, int64_t *row_ptr, int64_t *col,
                                         double *val);
/* the aggregate of every row of level l ([n_rows]); not on the coarsest level */
int storm_hip_amg_hierarchy_get_aggregates(const storm_hip_amg_hierarchy *h, int level, int64_t *aggregate);
/* P_l (n_rows x n_aggregates) as CSR ([n_rows + 1], [nnz_p], [nnz_p]); not on the coarsest level */
int storm_hip_amg_hierarchy_get_prolongator(const storm_hip_amg_hierarchy *h, int level, int64_t *row_ptr, int64_t *col,
                                            double *val);
/* the coarsest level's inverse, row-major [n x n] */
int storm_hip_amg_hierarchy_get_coarse_inverse(const storm_hip_amg_hierarchy *h, double *inverse);
/* "levels", "operator_complexity" (sum of nnz(A_l) / nnz(A_0)), "grid_complexity" (sum of n_l / n_0), "setup_seconds",
 * "structural" */
int storm_hip_amg_hierarchy_get(const storm_hip_amg_hierarchy *h, const char *key, double *value);
/* ---- Refreshable hierarchies (STORM_HIP_HAS_AMG_REFRESH, added within ABI 6) ------------------------------------------------
 * The split between symbolic and numeric setup: the graph work (strength, aggregation, pattern discovery) runs once on the
 * host, the numbers are recomputed on the device whenever the operator's weights changed.
 *
 * STRUCTURAL SETUP.  storm_hip_amg_setup_csr_structural is THE RECIPE with one difference: no pattern depends on a value.
 * Level 0 keeps every stored entry of the caller's CSR (duplicates merged, a zero stays); P_l lives on the pattern of
 * T u A^F T; A_l P_l and R_l (A_l P_l) live on their structural patterns.  A zero entry is never strong, as in the recipe.
 * Where the plain setup drops no zero the two hierarchies are equal bit for bit.  storm_hip_amg_hierarchy_get key
 * "structural" is 1 for such a hierarchy.  storm_hip_amg_hierarchy_get_strong: the strong mask of level l, one byte per entry
 * of A_l in the order of _get_operator (1: the pair is strong); available on plain hierarchies too, not on the coarsest level.
 *
 * THE FROZEN-STRUCTURE RECIPE (normative; tests/amg_refresh_ref.py restates it).  Frozen: the number of levels, the
 * aggregates, the strong mask of every level, the patterns of A_l, P_l, R_l and of the intermediate A_l P_l.  For level l:
 *   1. Level 0: a_ii = beta + alpha (ext_i - sum_k w_ik) and a_ij = alpha times the sum of w over the slots of column j: the
 *      decode of storm_hip_amg_create, except that every REAL slot counts whatever its value.  A slot is real when its
 *      source-map id is >= 0; padding (id -1) is left out.  (Hence the updatable operator: its source map says which.)
 *   2. a^F_ii = a_ii + the sum of the entries the mask calls weak; the strong entries are kept.
 *   3. lambda_F = max_i sum_j |a^F_ij| / |a^F_ii|.  A zero or non-finite a^F_ii: the refresh fails.
 *   4. P_iJ = [J = agg(i)] - (omega / lambda_F) / a^F_ii sum_{j in J} a^F_ij on P's frozen pattern; omega = 0: P is not
 *      touched.  R gets the same values, transposed.
 *   5. A_{l+1} = R_l (A_l P_l) on the frozen patterns.  The coarse operator's records get ext_i = the row sum in column order
 *      (as the CSR packer forms it), slots and CSR-tail entries the off-diagonal values.
 *   6. The coarsest level's values go to the host, are inverted as in step 7 of THE RECIPE, and the inverse is uploaded.  A
 *      singular level: the refresh fails.
 *   7. Every level's smoother is rebuilt from the refreshed level operator: the Jacobi scale (storm_hip_op_get_diagonal),
 *      Gershgorin's bound, the polynomial on [lmax / smoother_ratio, lmax].  With reduced_records the coarse operators'
 *      companions are converted again first.
 * Order of summation: inside a row of steps 2 to 4 and of A_l P_l the entries of A_l in column order; inside a row of
 * R_l (A_l P_l) the entries of R_l in column order (fine rows ascending), each contribution A P's entries in column order;
 * level 0 sums a column's slots in slot order, then its tail entries.  Every product is rounded before it is added.  A
 * refresh is deterministic (the same records give the same bits) and uses no floating-point atomics.
 *
 * storm_hip_amg_create_refreshable: storm_hip_amg_create with the structural setup, for an operator from
 *   storm_hip_op_create_from_face_weights_updatable (anything else: STORM_HIP_E_UNSUPPORTED).  The coarse operators carry a
 *   source map (the id of a slot is its entry's index in A_l).  Uploaded once beside the plain object: per level A_l as CSR
 *   (LEVEL 0 INCLUDED: the products read this copy, not the records), strong mask, aggregates, P_l as CSR, R_l's pattern,
 *   A_l P_l as CSR, the slot -> entry maps of the transfer records and of level 0's records.  storm_hip_amg_get key
 *   "refresh_bytes" reports this memory (it is part of "device_bytes"); "refreshable" is 1.
 * storm_hip_amg_refresh: the recipe above on the operator's records as they stand on the context's stream.  Waits on the
 *   host like a create: two max reductions per level (lambda_F, Gershgorin) and the coarsest level's round trip.  Not to be
 *   called between storm_hip_krylov_init and _finalize.  A zero or non-finite filtered diagonal (found by a device-side check
 *   that sets a flag word read at the level's wait) or a singular coarsest level: STORM_HIP_E_INVALID with level and row in
 *   the message; the object is then INVALID -- storm_hip_amg_apply and a solve bound to it return STORM_HIP_E_INVALID -- until
 *   a refresh succeeds.  On an object from storm_hip_amg_create: STORM_HIP_E_UNSUPPORTED.  Counter "amg_refreshes".
 * storm_hip_amg_download: brings the object's host hierarchy (storm_hip_amg_get_hierarchy, the export calls) up to date with
 *   what the cycle's kernels read: the level operators' records decoded as in step 1, the transfer records, the dense
 *   inverse; the coarsest level, which has no records, from its value array.  Waits on the host.  On a plain object it changes
 *   nothing. */
#define STORM_HIP_HAS_AMG_REFRESH 1
int storm_hip_amg_setup_csr_structural(int64_t n_rows, const int64_t *row_ptr, const int64_t *col, const double *val,
                                       const storm_hip_amg_params *params, storm_hip_amg_hierarchy **out);
int storm_hip_amg_hierarchy_get_strong(const storm_hip_amg_hierarchy *h, int level, uint8_t *mask);
int storm_hip_amg_create_refreshable(storm_hip_op *op, double alpha, double beta, const storm_hip_amg_params *params,
                                     storm_hip_amg **out);
int storm_hip_amg_refresh(storm_hip_amg *h);
int storm_hip_amg_download(storm_hip_amg *h);
/* The device object for an operator on fp64 records (format 0: what any mesh gets; a box built with option spmv_dict = 0;
 * a CSR tail is allowed).  The records are downloaded once and decoded to CSR: a_ii = beta + alpha (ext_i - sum_k w_ik),
 * a_ij = alpha sum w over the slots of column j, padding dropped; the setup above runs on the host; the coarse operators go
 * through the CSR packer, forced to fp64 records; level 0 uses `op` itself.  With reduced_records every level's operator
 * gets a companion (storm_hip_op_build_reduced: `op` too, if it has none).  Host waits (build time).
 * STORM_HIP_E_UNSUPPORTED: compact record formats; a halo plan, halo columns or a communicator.
 * `op` must outlive the object.  An object built before storm_hip_op_set_face_weights is STALE (its hierarchy and bounds are
 * those of the old weights); rebuilding it is the caller's, as for a storm_hip_cheb -- or the object is created by
 * storm_hip_amg_create_refreshable below and brought up to date by storm_hip_amg_refresh. */
int storm_hip_amg_create(storm_hip_op *op, double alpha, double beta, const storm_hip_amg_params *params, storm_hip_amg **out);
/* z = B r; z must not alias r, r is not written.  Enqueues and never waits; inside a solver callback predicated on the
 * solve's `done` flag. */
int storm_hip_amg_apply(const storm_hip_amg *h, const storm_hip_vec *r, storm_hip_vec *z);
/* The cycle's grid transfers and coarsest-level solve on their own (enqueued like an apply): coarse = R_l fine;
 * fine += P_l coarse; z = Ainv r on the coarsest level.  Vectors of the levels' sizes; the two must not alias. */
int storm_hip_amg_restrict(const storm_hip_amg *h, int level, const storm_hip_vec *fine, storm_hip_vec *coarse);
int storm_hip_amg_prolong_add(const storm_hip_amg *h, int level, const storm_hip_vec *coarse, storm_hip_vec *fine);
int storm_hip_amg_coarse_solve(const storm_hip_amg *h, const storm_hip_vec *r, storm_hip_vec *z);
/* the keys of storm_hip_amg_hierarchy_get, and "device_bytes" (what the object allocated), "transfer_padding" (the share of
 * the transfer records' slots that is padding), "upload_seconds", "smoother_degree", "reduced", "refresh_bytes",
 * "refreshable" */
int storm_hip_amg_get(const storm_hip_amg *h, const char *key, double *value);
/* the object's host hierarchy, for the export calls above (borrowed: it lives as long as the object) */
int storm_hip_amg_get_hierarchy(const storm_hip_amg *h, const storm_hip_amg_hierarchy **out);
int storm_hip_amg_destroy(storm_hip_amg *h);
/* pre_op as the library's multigrid preconditioner (h == NULL removes it): bound natively, no callback.  A size that differs
 * from the solve's vectors: STORM_HIP_E_INVALID from the solve. */
int storm_hip_krylov_set_preconditioner_amg(storm_hip_krylov *k, const storm_hip_amg *h, int side);
/* ---- Singular operators with the constants as their kernel (STORM_HIP_HAS_AMG_NULLSPACE, added within ABI 6) ----------------
 * The pressure equation of a projection method, -L_N p = rhs with Neumann walls, is symmetric positive SEMI-definite: A 1 = 0.
 * The entry points above refuse it at step 7 (they still do); the ones below build B = Pi V Pi, the V-cycle between two
 * projections onto the mean-free vectors, Pi = I - 1 1^T / n.  Strictly opt-in: nothing above changes its behaviour.
 *
 * storm_hip_amg_setup_csr_nullspace is THE RECIPE (structural != 0: its structural variant) with three differences
 * (normative; tests/amg_nullspace_ref.py restates them):
 *   N1. Row sums.  After normalisation every level-0 row must satisfy |sum_j a_ij| <= 2^-40 sum_j |a_ij| (both sums in column
 *       order).  Otherwise STORM_HIP_E_INVALID; the message names the first such row.  2^-40 classifies, it is no tolerance: a
 *       decoded Neumann row sits at a few eps, one Dirichlet face or beta != 0 gives O(0.1).
 *   N2. Connectivity.  The graph of the non-zero off-diagonal entries of level 0, both directions joined, must have ONE
 *       connected component (a row without an off-diagonal entry is a component of its own).  Otherwise STORM_HIP_E_INVALID
 *       with "component" and the count in the message.  (A disconnected operator coarsens to a numerically zero coarsest
 *       matrix, which no pivot test sees.)
 *   N3. Coarsest level, instead of step 7.  n_c = 1: Ainv = (0).  Otherwise s = max_i a_ii (s <= 0: STORM_HIP_E_INVALID),
 *       G = A_c + (s / n_c) 1 1^T entrywise, G^-1 by the Gauss-Jordan of step 7 -- a pivot below 2^-30 s in magnitude or a
 *       non-finite entry: STORM_HIP_E_INVALID, "singular beyond the constants" -- and Ainv = Pi G^-1 Pi, formed as: from every
 *       column its mean is subtracted (the sum over the rows in ascending order, divided by n_c), then from every row its
 *       mean (the sum over the columns in ascending order, divided by n_c).  Ainv is the pseudo-inverse of A_c up to rounding.
 * storm_hip_amg_hierarchy_get keys "nullspace" (0 / 1) and "coarse_shift" (s; 0 on a plain hierarchy and on a one-row
 * coarsest level); storm_hip_amg_hierarchy_get_coarse_inverse exports Ainv.
 *
 * storm_hip_amg_create_nullspace: storm_hip_amg_create on the setup above; refreshable != 0: storm_hip_amg_create_refreshable
 * on it (structural = 1).  The refusals of those two apply (compact records, halo, communicator, a non-updatable operator).
 * storm_hip_amg_refresh on such an object runs N3 in step 6 of the frozen-structure recipe; N1 AND N2 ARE NOT REPEATED AT A
 * REFRESH (the weights the caller sets must keep the operator a connected Neumann operator); a pivot failure leaves the
 * object invalid as on a plain one.  _download, _get_hierarchy and the grid-transfer entry points work as on a plain object;
 * storm_hip_amg_get key "nullspace".
 *
 * THE CYCLE of a null-space object (V: THE CYCLE above with Ainv from N3; Pi acts on level 0 only):
 *     rp = r - mu_r,  mu_r = fl(S_r / n)     r is not written; rp is one more level-0 work vector
 *     z  = V(rp)                             exactly the launches of a plain object, ending in z = z + e
 *     z  = z - mu_z,  mu_z = fl(S_z / n)
 * S is the sum of the vector's n entries by the library's streaming reduction: the stream_blocks(n) grid (a block owns 2048
 * consecutive entries, a thread its four 16-byte words in ascending order), the block sum, then the two-level ticket fold.
 * It depends on n only.  The block that draws the last ticket stores mu = S / n (an IEEE division) into a slot the object
 * owns; the next kernel on the stream reads it.  No host wait, no floating-point atomic.  Kernels (all predicated on the
 * solve's done flag): amg_mean_kernel (S, mu), amg_shift_kernel (out_i = v_i - mu), amg_axpy_mean_kernel (level 0's closing
 * z_i = z_i + e_i accumulating the stored values into amg_mean_kernel's partition: with option amg_fused = 1 it replaces
 * storm_hip_axpy + amg_mean_kernel; amg_fused = 0 runs the two; the same bits either way).  A one-level object is
 * Pi Ainv Pi from the same kernels.  Counters "amg_projections" (+2 per apply, +1 per storm_hip_amg_project) and
 * "amg_fused_projections" (+1 per apply that closed with the fused kernel).
 * storm_hip_amg_project: v <- v - mean(v) in place, v of level 0's size (anything else: STORM_HIP_E_INVALID); on a plain
 * object STORM_HIP_E_UNSUPPORTED.  Enqueued like an apply. */
#define STORM_HIP_HAS_AMG_NULLSPACE 1
int storm_hip_amg_setup_csr_nullspace(int64_t n_rows, const int64_t *row_ptr, const int64_t *col, const double *val,
                                      const storm_hip_amg_params *params, int structural, storm_hip_amg_hierarchy **out);
int storm_hip_amg_create_nullspace(storm_hip_op *op, double alpha, double beta, const storm_hip_amg_params *params,
                                   int refreshable, storm_hip_amg **out);
int storm_hip_amg_project(const storm_hip_amg *h, storm_hip_vec *v);
/* ---- Non-symmetric operators: the damped-Jacobi smoother (STORM_HIP_HAS_AMG_JACOBI, added within ABI 6) ---------------------
 * The setup above needs no symmetry (strength on the union of A and A^T, A_{l+1} = P^T A_l P, a pivoting inverse); the
 * Chebyshev smoother does: a polynomial on [lmax / ratio, lmax] assumes a real positive spectrum, and on first-order upwind
 * convection-diffusion its cycle is not a convergent preconditioner.  storm_hip_amg_create_smoother with kind 1 builds the
 * same hierarchy with damped Jacobi sweeps as the smoother.  Strictly opt-in: nothing above changes its behaviour or its bits.
 *
 * THE SMOOTHER (normative; tests/amg_jacobi_ref.py restates it).  Per level l: s_i = 1 / a_ii, the Jacobi scale as the
 * Chebyshev smoother obtains it (storm_hip_op_get_diagonal); lmax = Gershgorin's bound of diag(s) A_l, the one the Chebyshev
 * object uses (from the companion records with reduced_records); sigma_l = 2 omega / lmax, computed on the host in double.
 * One sweep is z' = z + sigma (s .* (r - A_l z)); a sweep from the zero guess is z = sigma (s .* r).
 *
 * THE CYCLE with nu = sweeps (t, e: the level's work vectors):
 *     z  = sigma (s .* r);  nu - 1 sweeps on z        pre-smoothing (nu = 1: no operator product)
 *     t  = r - A_l z                                   the residual of THE CYCLE above
 *     rc = R_l t;  zc = cycle(l + 1, rc);  z = z + P_l zc     unchanged
 *     nu sweeps on z                                   post-smoothing
 * 2 nu + 3 launches per level.  For a symmetric A this B is symmetric.  A sweep gathers its neighbours' old z, so it stores
 * into the other of two buffers, the caller's z and e: the sweep from the zero guess stores into e, which for every nu makes
 * the last sweep store into the caller's z.  No copy kernel; r is never written.
 *
 * THE ROUNDING of a sweep is that of the statement sequence
 *     storm_hip_op_apply(op_l, alpha_l, beta_l, z, t)          (storm_hip_op_apply_reduced with reduced_records)
 *     storm_hip_axpbz(t, 1, r, -1, t)
 *     storm_hip_vmul(t, s, t)
 *     storm_hip_axpbz(z', sigma, t, 1, z)                      the kernel of storm_hip_axpy: fma(sigma, t_i, z_i)
 * and of storm_hip_vmul(z, s, r); storm_hip_axpbz(z, sigma, z, 0, z) for the sweep from the zero guess.  A level on fp64
 * records without a CSR tail runs ONE kernel per sweep instead (amg_jacobi_sweep_kernel: records + 32 bytes per row where
 * the statements move 88) with the same bits; a level with a CSR tail, or option amg_fused = 0, runs the statements
 * (tests/test_gpu_amg_jacobi.py).  With reduced_records the sweep reads the level's fp32-weight companion records; the
 * residual keeps the fp64 records, as in a Chebyshev object.  Counters "amg_fused_sweeps" and "amg_statement_sweeps".
 *
 * storm_hip_amg_create_smoother: storm_hip_amg_create with the smoother chosen.  kind 0: exactly storm_hip_amg_create's
 *   object.  kind 1: smoother_degree and smoother_ratio of `params` are ignored; the object holds no Chebyshev object (three
 *   work vectors fewer per level).  STORM_HIP_E_INVALID: kind other than 0 / 1, sweeps outside 1 .. 16, omega outside (0, 1],
 *   a zero or non-finite diagonal on any level (the message names level and row).  The refusals of storm_hip_amg_create apply.
 *   There is no refreshable and no null-space object with this smoother: storm_hip_amg_refresh and storm_hip_amg_project on
 *   it return STORM_HIP_E_UNSUPPORTED, as on any plain object.  Single rank, fp64 records on level 0.
 * storm_hip_amg_smooth: one sweep on its own, z_out = z_in + sigma_l (s .* (r - A_l z_in)) on level l (not the coarsest),
 *   enqueued like an apply; z_out must alias neither z_in nor r.  On a Chebyshev object: STORM_HIP_E_UNSUPPORTED.
 * storm_hip_amg_get keys: "smoother_kind", "jacobi_sweeps", "jacobi_omega", "jacobi_sigma_<level>". */
#define STORM_HIP_HAS_AMG_JACOBI 1
typedef struct storm_hip_amg_smoother {
  int32_t kind;   /* 1; 0: the Chebyshev smoother, 1: damped Jacobi sweeps */
  int32_t sweeps; /* 2 (1 .. 16) */
  double omega;   /* 2/3, in (0, 1] */
} storm_hip_amg_smoother;
void storm_hip_amg_smoother_default(storm_hip_amg_smoother *smoother);
int storm_hip_amg_create_smoother(storm_hip_op *op, double alpha, double beta, const storm_hip_amg_params *params,
                                  const storm_hip_amg_smoother *smoother, storm_hip_amg **out);
int storm_hip_amg_smooth(const storm_hip_amg *h, int level, const storm_hip_vec *r, const storm_hip_vec *z_in,
                         storm_hip_vec *z_out);

/* ---- successive right-hand sides: the initial guess projected onto past solves ----------------------------------------
 * A time loop solves with one operator and a slowly changing right-hand side.  storm_hip_recycle keeps up to m pairs
 * (u_j, v_j = A u_j) of earlier solutions, made orthogonal as they arrive, and one device scalar g_j per pair; guess() is
 * the best initial guess in their span (Fischer, Projection techniques for iterative solution of Ax = b with successive
 * right-hand sides, CMAME 163 (1998)).  The object never applies A: the caller hands it A x.  No scalar of it visits the
 * host during guess or update (counter "host_reductions" does not move).  Added within ABI 6 (additive).
 *
 * THE RECIPE (restated in tests/recycle_ref.py).
 *   kind 0 is the energy projection, for SPD operators: the test vector is t_j = u_j, the norm is N(a, b) = <a, b> on
 *     (u, v), and g_j = 1 / <u_j, v_j>.
 *   kind 1 is residual-minimising, for any operator: t_j = v_j, the norm is <v, v>, and g_j = 1 / <v_j, v_j>.
 *   count is known to the host.  Slots j >= count are empty.  A slot with g_j = 0 contributes nothing.
 *
 *   guess(b, x):
 *     e_j = <t_j, b> for j < count.
 *     c_j = g_j * e_j.  The c values are kept on the device for the next update.
 *     x = ((0 + c_0 u_0) + c_1 u_1) + ...: one fma per term, ascending j, starting from +0.0.
 *     Owned rows only.  Halo rows are left as they are.
 *     count == 0 gives x = 0.
 *
 *   update(x, ax), count < m, s = count:
 *     d = x - sum_{j<s} c_j u_j and ad = ax - sum_{j<s} c_j v_j.  Each is a chain fma(-c_j, ., acc) in ascending j,
 *       starting from x or ax.
 *     e_j = <t_j, ad>.  nu0 = <d, ad> for kind 0, <ad, ad> for kind 1.
 *     beta_j = g_j e_j.  u_s = d - sum beta_j u_j and v_s = ad - sum beta_j v_j, the same chains.
 *     nu = <u_s, v_s> for kind 0, <v_s, v_s> for kind 1.
 *     g_s = 1 / nu if nu is finite, nu > 0 and nu > 2^-40 nu0.  Otherwise g_s = 0.  (The 2^-40 guard is the multigrid coarse
 *       level's pivot rule.)  g_s is decided by the block that finishes the reduction.
 *     count += 1.
 *     An update with no guess since the last update uses c = 0, so d = x (the first chain is not run).
 *
 *   update at count == m: restart.
 *     u_0 = x, v_0 = ax, nu = N(x, ax), g_0 by the same guard with nu0 = nu.
 *     g_j = 0 for j > 0.
 *     count = 1.  The restarts counter goes up by one.
 *
 *   reset() sets count = 0 and clears every g_j.
 *
 * Capacity is 1 .. 16.  Above 8 the chains continue across launches of 8, as the multi-axpy chunks them.
 *
 * LAUNCHES.  Option recycle_fused = 1 (the default): guess is the multi-dot and recycle_guess_kernel; update is
 * recycle_defect_kernel (d and ad formed in registers from one read of the 2 s + 2 vectors, written into slot s, with the
 * s + 1 sums finished by tickets) and recycle_orth_kernel (slot s updated in place, nu finished by tickets, its last block
 * writes g_s); the restart -- and the first pair of an empty object -- is one launch.  More than 8 slots: one more launch
 * per kernel and one multi-dot.  recycle_fused = 0 runs the same recipe out of the library's multi-dot, multi-axpy, copy
 * and fill launchers and a one-block scalar kernel: the reference the fused kernels are held to, bit for bit (with option
 * ticket_reduce at its default).  Counters: "recycle_guesses", "recycle_updates", "recycle_restarts",
 * "recycle_fused_launches", "recycle_statement_launches".
 *
 * storm_hip_recycle_get keys: "capacity", "count", "kind", "updates", "restarts", "device_bytes" (no wait);
 *   "weight_<j>" (g_j) and "coef_<j>" (c_j of the last guess; 0 when an update has followed it): wait for the stream.
 * storm_hip_recycle_get_slot / _set_slot: for checkpointing a time loop and for tests.  get_slot copies pair j < count into
 *   u and v (either may be null) and g_j into *g (may be null; waits when it is not).  set_slot needs j <= count; j == count
 *   appends (j < capacity).  The caller answers for the pairs being orthogonal in the kind's sense.
 * STORM_HIP_E_INVALID: a null argument, a capacity outside 1 .. 16, a kind other than 0 / 1, vectors of another context or
 *   size, x aliasing b in guess, x aliasing ax in update.  STORM_HIP_E_UNSUPPORTED: a context with a communicator (the sums
 *   here are local: single rank for now).  An operator that changes between solves leaves the pairs stale: reset() is the
 *   caller's job. */
typedef struct storm_hip_recycle storm_hip_recycle;
enum storm_hip_recycle_kind { STORM_HIP_RECYCLE_ENERGY = 0, STORM_HIP_RECYCLE_RESIDUAL = 1 };
int storm_hip_recycle_create(storm_hip_ctx *ctx, int64_t n_owned, int64_t n_halo, int capacity, int kind, storm_hip_recycle **out);
int storm_hip_recycle_destroy(storm_hip_recycle *h);
int storm_hip_recycle_guess(storm_hip_recycle *h, const storm_hip_vec *b, storm_hip_vec *x);
int storm_hip_recycle_update(storm_hip_recycle *h, const storm_hip_vec *x, const storm_hip_vec *ax);
int storm_hip_recycle_reset(storm_hip_recycle *h);
int storm_hip_recycle_get(const storm_hip_recycle *h, const char *key, double *value);
int storm_hip_recycle_get_slot(const storm_hip_recycle *h, int j, storm_hip_vec *u, storm_hip_vec *v, double *g);
int storm_hip_recycle_set_slot(storm_hip_recycle *h, int j, const storm_hip_vec *u, const storm_hip_vec *v, double g);

/* ---- Mixed-precision CG: fp32 inner iterations under fp64 refinement (STORM_HIP_HAS_MIXED_CG, added within ABI 6) -----------
 * CG for A = beta I + alpha M whose inner iterations live on fp32 vectors and on the operator's fp32-weight companion records
 * (A~, storm_hip_op_build_reduced: 51.9 instead of 79.8 B/row of records, 56 instead of 112 B/row of vectors), inside an fp64
 * outer loop that holds the answer to the reference's rule (Solver.hpp:116-147) on the TRUE fp64 residual: iterative
 * refinement.  Strictly opt-in: no other entry point changes its path or its bits.  Single rank.
 *
 * THE ALGORITHM (normative; tests/mixed_cg_ref.py restates it in numpy).
 *   r = b - A x on the fp64 records;  rho_0 = |r|;  the early exit of the rule (abs_tol > 0 and rho_0 < abs_tol)
 *   target = the norm at which the rule stops: the larger of abs_tol and rel_tol rho_0 over the criteria that are enabled
 *   outer step k = 1, 2, ...:
 *     rho = |r|;  s = 1.0 / rho                                          (fp64, on the device)
 *     r32 = fl32(r_i s);  d32 = 0;  p32 = r32        (keep_direction = 1 and k > 1: p32 = fl32(p32_i (rho_prev / rho)))
 *     g = <r32, r32>;  eta = max(inner_tolerance, 0.5 target / rho)       (never deeper than the outer rule needs)
 *     inner iteration j = 1 .. inner_max:
 *       q32 = fl32(A~ p32);  pq = <p32, q32>;  a = g / pq;   BROKEN when pq <= 0 or pq is not finite (nothing more is stored)
 *       d32 = fl32(a p + d);  r32 = fl32(-a q + r);  g' = <r32, r32>;  bt = g' / g
 *       p32 = fl32(r + fl(bt p));  g = g';   leave when sqrt(g') <= eta;  BROKEN when g' is not finite
 *     x = fma(rho, (double)d32_i, x_i)                                    (fp64; skipped when BROKEN)
 *     r = b - A x on the fp64 records;  the rule on |r|: converged -> done
 *     BROKEN (2), or |r| not smaller than rho (1), or k == max_outer or the inner iterations have reached
 *       params.num_iterations (3): finish with storm_hip_solve_cg from this x with the iterations that are left, held to the
 *       same residual norm (its relative tolerance rescaled by rho_0 / |r|); the number is storm_hip_mixed_result::finished_fp64.
 *
 * THE CONTRACT extends the reduced records' to vectors: an fp32 vector element is widened, exactly, where a kernel loads it;
 * every operation is the fp64 kernel's in the same order with the same contraction; ONE IEEE round-to-nearest-even conversion
 * at each fp32 store; sums accumulate in fp64.  So every vector statement of the inner loop gives, BIT FOR BIT, (float) of what
 * storm_hip_op_apply_reduced, storm_hip_axpy (d, r) and storm_hip_xpay (p) give on the widened operands; a and bt are single
 * fp64 divisions of the device's own sums (tests/test_gpu_mixed_cg.py).
 *
 * Three launches per inner iteration and no host wait in it: the host polls the inner loop's done word check_lag iterations
 * behind; one host wait per outer step (the true residual's norm).  result->iterations counts the inner iterations plus those
 * of an fp64 finish; num_applies every operator product, A~ and A alike; history (NULL or room for num_iterations + 1) gets the
 * TRUE residual norms, one per outer step behind the initial one, then the finishing loop's; absolute_error, relative_error
 * and converged are those of the last true residual.  Counters: "mixed_solves", "mixed_inner_iterations",
 * "mixed_outer_steps", "mixed_fp64_finishes".
 *
 * STORM_HIP_E_UNSUPPORTED, decided on the host before any launch: an operator that is not on fp64 records; one with a CSR
 * tail; one without a companion (nothing is built behind the caller's back: call storm_hip_op_build_reduced first), also in a
 * solve after storm_hip_op_drop_reduced; a halo plan, halo columns or a communicator.  STORM_HIP_E_INVALID: inner_tolerance
 * not in (0, 1), inner_max < 0, max_outer < 1, keep_direction other than 0 / 1, a null argument, vectors of another context
 * or size.  storm_hip_op_set_face_weights refreshes the companion: an updatable operator needs nothing new.  The operator
 * must outlive the object.
 *
 * The stepping entry points (tests, benchmarks): _begin forms r, rho and the conversion of the first outer step (one host
 * wait); _inner enqueues exactly n inner iterations with no exit test (enqueue-only); _end_outer updates x, forms the true
 * residual and returns its norm (one host wait); _get_vector widens "r32" | "p32" | "q32" | "d32" into an fp64 vector
 * (enqueue-only); _get_scalar reads "rho" | "g" | "pq" | "alpha" | "beta" (waits for the stream). */
#define STORM_HIP_HAS_MIXED_CG 1
typedef struct storm_hip_mixed_params {
  double inner_tolerance;   /* default 1e-3 */
  int64_t inner_max;        /* inner iterations per outer step; 0 (default) = params.num_iterations */
  int32_t max_outer;        /* default 16 */
  int32_t keep_direction;   /* default 0: the direction restarts at every outer step; 1: kept, rescaled */
} storm_hip_mixed_params;
typedef struct storm_hip_mixed_result {
  int64_t outer_steps, inner_iterations, fp64_iterations;
  int32_t finished_fp64;    /* 0 no; 1 the true residual did not fall; 2 BROKEN; 3 max_outer or the iteration budget */
} storm_hip_mixed_result;
typedef struct storm_hip_mixed_cg storm_hip_mixed_cg;
void storm_hip_mixed_params_default(storm_hip_mixed_params *p);
int storm_hip_mixed_cg_create(const storm_hip_op *op, double alpha, double beta, const storm_hip_mixed_params *mixed_params,
                              storm_hip_mixed_cg **out);
int storm_hip_mixed_cg_destroy(storm_hip_mixed_cg *m);
int storm_hip_mixed_cg_solve(storm_hip_mixed_cg *m, const storm_hip_vec *b, storm_hip_vec *x, const storm_hip_solver_params *params,
                             storm_hip_solver_result *result, double *history, storm_hip_mixed_result *mixed_result);
int storm_hip_mixed_cg_begin(storm_hip_mixed_cg *m, const storm_hip_vec *b, const storm_hip_vec *x);
int storm_hip_mixed_cg_inner(storm_hip_mixed_cg *m, int64_t n_iterations);
int storm_hip_mixed_cg_end_outer(storm_hip_mixed_cg *m, storm_hip_vec *x, double *rho);
int storm_hip_mixed_cg_get_vector(storm_hip_mixed_cg *m, const char *name, storm_hip_vec *out);
int storm_hip_mixed_cg_get_scalar(storm_hip_mixed_cg *m, const char *name, double *value);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* STORM_HIP_H_ */
