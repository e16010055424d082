// Storm.hpp -- the reference's Operator / Vector / Solver interface on top of the storm_hip C ABI.
//
// Driver code written against StormRuler's solver layer compiles against this header unchanged:
// the class templates below keep the reference's names, public members, defaults and virtual
// signatures (reference paths relative to its root):
//     Operator, FunctionalOperator, make_operator, make_symmetric_operator   Solvers/Operator.hpp:66-200
//     Preconditioner, IdentityPreconditioner, PreconditionerSide              Solvers/Preconditioner.hpp:39-97
//     Solver, IterativeSolver, InnerOuterIterativeSolver, solve<>, solve_non_uniform
//                                                                             Solvers/Solver.hpp:43-292
//     CgSolver / BiCgStabSolver / GmresSolver                                 Solvers/SolverCg.hpp, SolverBiCgStab.hpp, SolverGmres.hpp
// (three of those reference headers do not compile as shipped -- SURVEY.md headline fact 5 -- so
// they are restated here rather than included).
//
// `DeviceVector` plays the role of `Feathers::Field` (Feathers/Field.hpp:60-114).  Every vector
// statement a solver body executes is intercepted by an overload in this header and lowered to
// exactly ONE C-ABI call (one HIP kernel).  DeviceVector also models the reference's `legacy_vector_like`
// concept (Solvers/Operator.hpp:39-45: `shape()`, `operator()(row, col)`, `assign`), so the reference's own
// solver templates can be instantiated on it (tools/check_reference_binding.sh); its element
// access is a slow host proxy that exists for the concept only -- every statement of the overload census
//  has a non-template overload here for const and non-const operands alike, which overload
// resolution prefers to Bittern's generic element-loop templates.
//
// The solver classes of this header are knob holders: `solve` hands the whole solve to the library's
// device-resident loops (storm_hip_krylov_*, csrc/krylov.hip) for ANY operator -- a `HipStencilOperator`
// binds natively, a lambda through make_operator (as Playground.cpp:151-167 does) as a callback that only
// enqueues its kernels -- and no scalar of a recurrence ever visits the host.
//
// C++17, header-only, needs only <storm_hip.h> and libstorm_hip.so.
#pragma once

#include <storm_hip.h>

#include <array>
#include <cmath>
#include <cstdio>
#include <cstddef>
#include <cstring>
#include <exception>
#include <functional>
#include <initializer_list>
#include <limits>
#include <memory>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

namespace Storm {

using real_t = double;  // Crow/Base/Types.hpp:38

namespace detail {
// Error convention of SURVEY 8b: a nonzero C-ABI status becomes std::runtime_error, like the
// reference's STORM_THROW_IO (Crow/Base/Exception.hpp:35-44); non-convergence is not an error.
inline void check(int status) {
  if (status != 0) throw std::runtime_error(std::string("storm_hip: ") + storm_hip_last_error());
}
}  // namespace detail

#ifndef STORM_HIP_NO_SOLVERS  // (defined: the reference's own Crow / Solvers headers supply what this block restates)
/// y == 0 ? 0 : x / y                                         (Crow/MathUtils.hpp:49-52)
inline real_t safe_divide(real_t x, real_t y) noexcept { return (y == 0.0) ? 0.0 : (x / y); }

/// Givens rotation (cs, sn, rr) with rr = hypot(a, b)         (Crow/MathUtils.hpp:164-179)
inline std::array<real_t, 3> sym_ortho(real_t a, real_t b) noexcept {
  const real_t rr = std::hypot(a, b);
  if (rr > 0.0) return {a / rr, b / rr, rr};
  return {1.0, 0.0, rr};
}

#endif  // STORM_HIP_NO_SOLVERS
// ---------------------------------------------------------------------------------------------
/// One GPU and its streams / workspaces.  One per process (rank).
class Context {
public:
  explicit Context(int device = 0) { detail::check(storm_hip_ctx_create(device, &_h)); }
  ~Context() { storm_hip_ctx_destroy(_h); }
  Context(const Context&) = delete;
  Context& operator=(const Context&) = delete;
  storm_hip_ctx* handle() const noexcept { return _h; }
  void sync() const { detail::check(storm_hip_ctx_sync(_h)); }
  void set_option(const char* key, long long value) { detail::check(storm_hip_ctx_set_option(_h, key, value)); }
  /// Which path the context's solves took, what its host loops fused ... (`storm_hip_ctx_get_counter`).
  long long counter(const char* key) const {
    int64_t value = 0;
    detail::check(storm_hip_ctx_get_counter(_h, key, &value));
    return (long long)value;
  }
  void comm_init(const void* id128, int n_ranks, int rank) {
    detail::check(storm_hip_ctx_comm_init(_h, id128, n_ranks, rank));
  }

private:
  storm_hip_ctx* _h = nullptr;
};

// ---------------------------------------------------------------------------------------------
class DeviceVector;

namespace expr {
// The few expression shapes the solver bodies build (cf. the op census of SURVEY 8b).
struct Scaled { real_t a; const DeviceVector* v; };                          // a * v
struct Lin2 { real_t a; const DeviceVector* x; real_t b; const DeviceVector* z; };  // a x + b z
struct ScaledLin2 { real_t s; Lin2 e; };                                      // s (a x + b z)
struct Lin3 { const DeviceVector* r; real_t s; Lin2 e; };                     // r + s (a x + b z)
struct Quot { const DeviceVector* v; real_t s; };                             // v / s (true division)
}  // namespace expr

/// N doubles in HBM (+ halo rows in multi-GPU runs): the solver `Vector`.
class DeviceVector {
public:
  DeviceVector() = default;
  DeviceVector(const Context& ctx, std::size_t n_owned, std::size_t n_halo = 0) {
    detail::check(storm_hip_vec_create(ctx.handle(), (int64_t)n_owned, (int64_t)n_halo, &_h));
  }
  DeviceVector(DeviceVector&& o) noexcept : _h(std::exchange(o._h, nullptr)), _view(std::exchange(o._view, false)) {}
  DeviceVector& operator=(DeviceVector&& o) noexcept {
    if (this != &o) {
      release();
      _h = std::exchange(o._h, nullptr);
      _view = std::exchange(o._view, false);
    }
    return *this;
  }
  DeviceVector(const DeviceVector&) = delete;
  DeviceVector& operator=(const DeviceVector&) = delete;
  ~DeviceVector() { release(); }

  /// A non-owning view of a vector the library hands to an operator / preconditioner callback.
  static DeviceVector view_of(storm_hip_vec* handle) noexcept {
    DeviceVector v;
    v._h = handle, v._view = true;
    return v;
  }

  /// Field::assign(other, copy): a new zero-initialised vector shaped like `other`; the reference
  /// ignores `copy` (Feathers/Field.hpp:82-84) and so does this.
  void assign(const DeviceVector& other, bool /*copy*/ = true) {
    storm_hip_vec* fresh = nullptr;
    detail::check(storm_hip_vec_create_like(other._h, &fresh));
    release();
    _h = fresh;
  }

  /// Field::shape() = {N, NumVars}  (Field.hpp:77-79)
  std::array<std::size_t, 2> shape() const {
    int64_t n = 0;
    if (_h) detail::check(storm_hip_vec_size(_h, &n, nullptr));
    return {(std::size_t)n, 1};
  }
  std::size_t size() const { return shape()[0]; }

  /// Field::operator()(row, col) (Field.hpp:104-111; `col` ignored, NumVars == 1).  A HOST PROXY: one blocking
  /// 8-byte copy per call.  It exists so that DeviceVector models the reference's `matrix` concept
  /// (Bittern/Matrix.hpp:40-45: `std::apply(mat, mat.shape())`); no solver statement goes through it.
  real_t operator()(std::size_t row, std::size_t /*col*/ = 0) const {
    real_t value = 0.0;
    detail::check(storm_hip_vec_get(_h, (int64_t)row, &value));
    return value;
  }

  void upload(const real_t* host, std::size_t n) { detail::check(storm_hip_vec_upload(_h, host, (int64_t)n)); }
  void download(real_t* host, std::size_t n) const { detail::check(storm_hip_vec_download(_h, host, (int64_t)n)); }
  std::vector<real_t> to_host() const {
    std::vector<real_t> out(size());
    download(out.data(), out.size());
    return out;
  }
  storm_hip_vec* handle() const noexcept { return _h; }

  // TargetMatrixInterface (Bittern/MatrixTarget.hpp:96-119): one kernel each.
  DeviceVector& operator+=(const expr::Scaled& e) { detail::check(storm_hip_axpy(_h, e.a, e.v->_h)); return *this; }
  DeviceVector& operator-=(const expr::Scaled& e) { detail::check(storm_hip_axpy(_h, -e.a, e.v->_h)); return *this; }
  DeviceVector& operator+=(const DeviceVector& v) { detail::check(storm_hip_axpy(_h, 1.0, v._h)); return *this; }
  DeviceVector& operator-=(const DeviceVector& v) { detail::check(storm_hip_axpy(_h, -1.0, v._h)); return *this; }
  DeviceVector& operator*=(real_t s) { detail::check(storm_hip_scale(_h, s)); return *this; }
  DeviceVector& operator/=(real_t s) { detail::check(storm_hip_div_scalar(_h, s)); return *this; }

private:
  void release() noexcept {
    if (!_view) storm_hip_vec_destroy(_h);
    _h = nullptr, _view = false;
  }
  storm_hip_vec* _h = nullptr;
  bool _view = false;
};

// Expression builders (Bittern/MatrixMath.hpp:247-285 for this vector type).
//
// Bittern's own operators are templates on forwarding references (`operator*(scalar auto, matrix auto&&)` ...):
// for a NON-const DeviceVector lvalue they deduce `DeviceVector&`, an identity binding that would beat an
// overload taking `const DeviceVector&`.  So every first-level operator that has a raw DeviceVector operand is
// spelled out for both `DeviceVector&` and `const DeviceVector&` -- equal conversions, and then the
// non-template wins (tests/cpp/concept_check.cpp plays Bittern's side with templates of the same shape).
#define STORM_HIP_CV1(MACRO) MACRO(const DeviceVector&) MACRO(DeviceVector&)
#define STORM_HIP_CV2(MACRO)                                             \
  MACRO(const DeviceVector&, const DeviceVector&) MACRO(DeviceVector&, const DeviceVector&) \
  MACRO(const DeviceVector&, DeviceVector&) MACRO(DeviceVector&, DeviceVector&)

#define STORM_HIP_SCALED(V) \
  inline expr::Scaled operator*(real_t a, V v) { return {a, &v}; }
STORM_HIP_CV1(STORM_HIP_SCALED)
#define STORM_HIP_QUOT(V) \
  inline expr::Quot operator/(V v, real_t s) { return {&v, s}; }
STORM_HIP_CV1(STORM_HIP_QUOT)
#define STORM_HIP_PLUS_SCALED(V)                                                                    \
  inline expr::Lin2 operator+(V x, const expr::Scaled& s) { return {1.0, &x, s.a, s.v}; }           \
  inline expr::Lin2 operator-(V x, const expr::Scaled& s) { return {1.0, &x, -s.a, s.v}; }          \
  inline expr::Lin3 operator+(V r, const expr::ScaledLin2& e) { return {&r, e.s, e.e}; }
STORM_HIP_CV1(STORM_HIP_PLUS_SCALED)
#define STORM_HIP_SUM(X, Z)                                                      \
  inline expr::Lin2 operator+(X x, Z z) { return {1.0, &x, 1.0, &z}; }           \
  inline expr::Lin2 operator-(X x, Z z) { return {1.0, &x, -1.0, &z}; }
STORM_HIP_CV2(STORM_HIP_SUM)
namespace expr {  // (operands of namespace expr only: declared there, where argument-dependent lookup looks)
inline Lin2 operator+(const Scaled& a, const Scaled& b) { return {a.a, a.v, b.a, b.v}; }
inline ScaledLin2 operator*(real_t s, const Lin2& e) { return {s, e}; }
}  // namespace expr

// out <<= expr   (Bittern/MatrixAlgorithms.hpp:120-124)
#define STORM_HIP_COPY(V)                                              \
  inline DeviceVector& operator<<=(DeviceVector& out, V v) {           \
    detail::check(storm_hip_copy(out.handle(), v.handle()));           \
    return out;                                                        \
  }
STORM_HIP_CV1(STORM_HIP_COPY)
inline DeviceVector& operator<<=(DeviceVector& out, const expr::Scaled& e) {
  detail::check(storm_hip_axpbz(out.handle(), e.a, e.v->handle(), 0.0, e.v->handle()));
  return out;
}
inline DeviceVector& operator<<=(DeviceVector& out, const expr::Lin2& e) {
  detail::check(storm_hip_axpbz(out.handle(), e.a, e.x->handle(), e.b, e.z->handle()));
  return out;
}
inline DeviceVector& operator<<=(DeviceVector& out, const expr::Lin3& e) {
  // p <<= r + beta * (p - omega * v)  (SolverBiCgStab.hpp:119) and  p <<= u + beta * (q + beta * p)
  // (SolverCgs.hpp:122): one kernel that evaluates r + s * (a x + b z) in this nesting
  detail::check(storm_hip_lin3(out.handle(), e.r->handle(), e.s, e.e.a, e.e.x->handle(), e.e.b, e.e.z->handle()));
  return out;
}
inline DeviceVector& operator<<=(DeviceVector& out, const expr::ScaledLin2& e) {
  // z <<= delta_inverse * (z - w)  (SolverNewton.hpp:148): the inner sum is rounded before the
  // scaling, as the reference's expression tree evaluates it
  detail::check(storm_hip_axpbz(out.handle(), e.e.a, e.e.x->handle(), e.e.b, e.e.z->handle()));
  detail::check(storm_hip_scale(out.handle(), e.s));
  return out;
}
inline DeviceVector& operator<<=(DeviceVector& out, const expr::Quot& e) {  // p <<= r / phi, SolverIdrs.hpp:131
  if (e.v != &out) detail::check(storm_hip_copy(out.handle(), e.v->handle()));
  detail::check(storm_hip_div_scalar(out.handle(), e.s));
  return out;
}

// out <<= map(func, mats...)   (Bittern/MatrixMath.hpp:44-105, evaluated by MatrixAlgorithms.hpp:75-79, 120-124)
//
// `func` runs on the device, so it cannot be handed over as a host callable: it is TRACED.  Called once with operands of
// type expr::Sym, a generic lambda records the operations it performs, in the order it performs them, as a short program
// for storm_hip_map -- each operation rounded on its own, so the device's result equals the host's evaluation of the same
// expression bit for bit.  The playground's (Playground.cpp:142-148)
//     constexpr auto dF_dc = [](real_t c) noexcept { return 2.0 * c * (c - 1.0) * (2.0 * c - 1.0); };
//     f <<= map(dF_dc, c);
// needs ONE token changed: `real_t c` -> `auto c`.  Supported: + - * /, unary -, abs, sqrt, min, max, mixed with
// real_t constants; one or two vector operands, or three when one of them is the target itself (`y <<= map(f, y, a, b)`);
// no data-dependent branches (a traced value has no truth value).
namespace expr {
class Sym {
public:
  Sym(real_t constant) { _consts.push_back(constant), _code.push_back(STORM_HIP_MAP_CONST); }  // NOLINT: `2.0 * c`
  static Sym input(int slot) {  // (slot k is recorded as opcode k; `<<=` assigns the slots to x0 / x1 / y)
    Sym s;
    s._code.push_back(slot);
    return s;
  }
  static Sym unary(int op, const Sym& a) {
    Sym s = a;
    s._code.push_back(op);
    return s;
  }
  static Sym binary(int op, const Sym& a, const Sym& b) {
    Sym s = a;
    for (int32_t word : b._code) {
      if ((word & 0xff) == STORM_HIP_MAP_CONST) word = STORM_HIP_MAP_CONST | (s.constant(b._consts[(std::size_t)(word >> 8)]) << 8);
      s._code.push_back(word);
    }
    s._code.push_back(op);
    return s;
  }
  const std::vector<int32_t>& code() const noexcept { return _code; }
  const std::vector<real_t>& constants() const noexcept { return _consts; }

private:
  Sym() = default;
  int32_t constant(real_t value) {  // one slot per distinct bit pattern
    for (std::size_t k = 0; k < _consts.size(); ++k)
      if (std::memcmp(&_consts[k], &value, sizeof value) == 0) return (int32_t)k;
    _consts.push_back(value);
    return (int32_t)_consts.size() - 1;
  }
  std::vector<int32_t> _code;  // a lone constant's word carries index 0: Sym(real_t) pushes it first
  std::vector<real_t> _consts;
};
inline Sym operator+(const Sym& a, const Sym& b) { return Sym::binary(STORM_HIP_MAP_ADD, a, b); }
inline Sym operator-(const Sym& a, const Sym& b) { return Sym::binary(STORM_HIP_MAP_SUB, a, b); }
inline Sym operator*(const Sym& a, const Sym& b) { return Sym::binary(STORM_HIP_MAP_MUL, a, b); }
inline Sym operator/(const Sym& a, const Sym& b) { return Sym::binary(STORM_HIP_MAP_DIV, a, b); }
inline Sym operator-(const Sym& a) { return Sym::unary(STORM_HIP_MAP_NEG, a); }
inline Sym operator+(const Sym& a) { return a; }
inline Sym abs(const Sym& a) { return Sym::unary(STORM_HIP_MAP_ABS, a); }
inline Sym sqrt(const Sym& a) { return Sym::unary(STORM_HIP_MAP_SQRT, a); }
inline Sym min(const Sym& a, const Sym& b) { return Sym::binary(STORM_HIP_MAP_MIN, a, b); }
inline Sym max(const Sym& a, const Sym& b) { return Sym::binary(STORM_HIP_MAP_MAX, a, b); }

struct Mapped {  // map(func, mats...): the traced program and its operands (slot k of the program reads x[k])
  Sym program;
  const DeviceVector* x[3];
};
}  // namespace expr

#define STORM_HIP_MAP1(V)                                        \
  template<class Func>                                           \
  inline expr::Mapped map(Func func, V x0) {                     \
    return {func(expr::Sym::input(0)), {&x0, nullptr, nullptr}}; \
  }
STORM_HIP_CV1(STORM_HIP_MAP1)
#define STORM_HIP_MAP2(X, Z)                                                            \
  template<class Func>                                                                  \
  inline expr::Mapped map(Func func, X x0, Z x1) {                                      \
    return {func(expr::Sym::input(0), expr::Sym::input(1)), {&x0, &x1, nullptr}};       \
  }
STORM_HIP_CV2(STORM_HIP_MAP2)
/// Three operands (one of which must be the target of the `<<=` that consumes the node: the device kernel streams the
/// target and two more vectors).
#define STORM_HIP_MAP3(X, Y, Z)                                                                                \
  template<class Func>                                                                                         \
  inline expr::Mapped map(Func func, X x0, Y x1, Z x2) {                                                       \
    return {func(expr::Sym::input(0), expr::Sym::input(1), expr::Sym::input(2)), {&x0, &x1, &x2}};             \
  }
#define STORM_HIP_MAP3_Z(X, Y) STORM_HIP_MAP3(X, Y, const DeviceVector&) STORM_HIP_MAP3(X, Y, DeviceVector&)
STORM_HIP_CV2(STORM_HIP_MAP3_Z)
#undef STORM_HIP_MAP1
#undef STORM_HIP_MAP2
#undef STORM_HIP_MAP3
#undef STORM_HIP_MAP3_Z
inline DeviceVector& operator<<=(DeviceVector& out, const expr::Mapped& e) {
  // the program's slots -> the kernel's operands: the target itself is `y`, the others x0, x1 in their order
  int opcode_of[3] = {-1, -1, -1};
  const DeviceVector* xs[2] = {nullptr, nullptr};
  int used = 0;
  for (int k = 0; k < 3; ++k) {
    if (e.x[k] == nullptr) continue;
    if (e.x[k] == &out) {
      opcode_of[k] = STORM_HIP_MAP_Y;
    } else {
      if (used == 2) throw std::invalid_argument("map: three operands, none of which is the target of `<<=`");
      xs[used] = e.x[k];
      opcode_of[k] = used == 0 ? STORM_HIP_MAP_X0 : STORM_HIP_MAP_X1;
      ++used;
    }
  }
  std::vector<int32_t> code = e.program.code();
  for (int32_t& word : code)
    if ((word & 0xff) < STORM_HIP_MAP_CONST) word = opcode_of[word & 0xff];
  const auto& consts = e.program.constants();
  detail::check(storm_hip_map(out.handle(), xs[0] ? xs[0]->handle() : nullptr, xs[1] ? xs[1]->handle() : nullptr, code.data(),
                              (int)code.size(), consts.data(), (int)consts.size()));
  return out;
}

/// Bittern/MatrixAlgorithms.hpp:140-153: the reference's engine, distribution and sequence.
inline void fill_randomly(DeviceVector& a) { detail::check(storm_hip_fill_randomly(a.handle())); }

/// y = a .* b elementwise (a diagonal preconditioner's `mul`).
inline void vmul(DeviceVector& y, const DeviceVector& a, const DeviceVector& b) {
  detail::check(storm_hip_vmul(y.handle(), a.handle(), b.handle()));
}

/// Bittern/MatrixAlgorithms.hpp:310-317 (global sum over all ranks).
#define STORM_HIP_DOT(A, B)                                              \
  inline real_t dot_product(A a, B b) {                                  \
    real_t r = 0.0;                                                      \
    detail::check(storm_hip_dot(a.handle(), b.handle(), &r));            \
    return r;                                                            \
  }
STORM_HIP_CV2(STORM_HIP_DOT)
/// Bittern/MatrixAlgorithms.hpp:262-270.
#define STORM_HIP_NORM(A)                                   \
  inline real_t norm_2(A a) {                               \
    real_t r = 0.0;                                         \
    detail::check(storm_hip_norm2(a.handle(), &r));         \
    return r;                                               \
  }
STORM_HIP_CV1(STORM_HIP_NORM)
#undef STORM_HIP_SCALED
#undef STORM_HIP_QUOT
#undef STORM_HIP_PLUS_SCALED
#undef STORM_HIP_SUM
#undef STORM_HIP_COPY
#undef STORM_HIP_DOT
#undef STORM_HIP_NORM
#undef STORM_HIP_CV1
#undef STORM_HIP_CV2
/// ADL hook used at Solvers/Solver.hpp:281 and SolverBiCgStab.hpp:224.
inline void fill_with(DeviceVector& a, real_t value) { detail::check(storm_hip_fill(a.handle(), value)); }

// ---------------------------------------------------------------------------------------------
#ifndef STORM_HIP_NO_SOLVERS
/// Abstract operator y <- A(x).
template<class InVector, class OutVector = InVector>
class Operator {
public:
  virtual ~Operator() = default;

  virtual void mul(OutVector& y_vec, const InVector& x_vec) const = 0;

  /// z <- A(y <- B(x))
  template<class InOutVector = InVector>
  void mul(OutVector& z_vec, InOutVector& y_vec, const Operator<InVector, InOutVector>& other_op,
           const InVector& x_vec) const {
    other_op.mul(y_vec, x_vec);
    mul(z_vec, y_vec);
  }

  /// r <- b - A(x)
  void Residual(OutVector& r_vec, const OutVector& b_vec, const InVector& x_vec) const {
    mul(r_vec, x_vec);
    r_vec <<= b_vec - r_vec;
  }

  real_t ResidualNorm(const OutVector& b_vec, const InVector& x_vec) const {
    OutVector r_vec;
    r_vec.assign(b_vec, false);
    Residual(r_vec, b_vec, x_vec);
    return norm_2(r_vec);
  }

  virtual void conj_mul(InVector& /*x_vec*/, const OutVector& /*y_vec*/) const {
    throw std::runtime_error("`Operator::conj_mul` was not overriden");
  }
};

/// Operator given by callables.
template<class InVector, class OutVector = InVector>
class FunctionalOperator final : public Operator<InVector, OutVector> {
public:
  template<class MatVec>
  explicit FunctionalOperator(MatVec&& mat_vec) : _mat_vec{std::forward<MatVec>(mat_vec)} {}
  template<class MatVec, class ConjMatVec>
  FunctionalOperator(MatVec&& mat_vec, ConjMatVec&& conj_mat_vec)
      : _mat_vec{std::forward<MatVec>(mat_vec)}, _conj_mat_vec{std::forward<ConjMatVec>(conj_mat_vec)} {}

  void mul(OutVector& y_vec, const InVector& x_vec) const override { _mat_vec(y_vec, x_vec); }
  void conj_mul(InVector& x_vec, const OutVector& y_vec) const override {
    if (!_conj_mat_vec)
      throw std::runtime_error("`FunctionalOperator::conj_mul` conjugate product function was not set.");
    _conj_mat_vec(x_vec, y_vec);
  }

private:
  std::function<void(OutVector&, const InVector&)> _mat_vec;
  std::function<void(InVector&, const OutVector&)> _conj_mat_vec;
};

template<class InVector, class OutVector = InVector, class MatVec>
auto make_operator(MatVec&& mat_vec) {
  return std::make_unique<FunctionalOperator<InVector, OutVector>>(std::forward<MatVec>(mat_vec));
}
template<class InVector, class OutVector = InVector, class MatVec, class ConjMatVec>
auto make_operator(MatVec&& mat_vec, ConjMatVec&& conj_mat_vec) {
  return std::make_unique<FunctionalOperator<InVector, OutVector>>(std::forward<MatVec>(mat_vec),
                                                                    std::forward<ConjMatVec>(conj_mat_vec));
}
template<class Vector, class MatVec>
auto make_symmetric_operator(MatVec&& mat_vec) {
  return std::make_unique<FunctionalOperator<Vector>>(mat_vec, std::forward<MatVec>(mat_vec));
}

#endif  // STORM_HIP_NO_SOLVERS

// ---------------------------------------------------------------------------------------------
/// The face-graph operator M in HBM (sliced-ELL records + CSR tail); owns the handle.
class StencilMatrix {
public:
  StencilMatrix() = default;
  /// Diffusion stencil of stormDivGrad (Playground.cpp:115-131) from mesh quantities; see storm_hip.h.
  static StencilMatrix from_faces(const Context& ctx, std::size_t n_owned, std::size_t n_halo,
                                  const std::vector<int64_t>& inner, const std::vector<int64_t>& outer,
                                  const std::vector<real_t>& coef, const std::vector<int64_t>& b_cell,
                                  const std::vector<real_t>& b_coef, const std::vector<real_t>& volume) {
    StencilMatrix m;
    detail::check(storm_hip_op_create_from_faces(ctx.handle(), (int64_t)n_owned, (int64_t)n_halo,
                                                 (int64_t)inner.size(), inner.data(), outer.data(), coef.data(),
                                                 (int64_t)b_cell.size(), b_cell.data(), b_coef.data(),
                                                 volume.data(), &m._h));
    return m;
  }
  /// The same straight from the arrays the face loop reads (Playground.cpp:119-129): the library forms
  /// area / length(center(out) - center(in)) itself (storm_hip_op_create_from_mesh).  `center` = cells x dim, row-major.
  static StencilMatrix from_mesh(const Context& ctx, std::size_t n_owned, std::size_t n_halo, int dim,
                                 const std::vector<int64_t>& inner, const std::vector<int64_t>& outer,
                                 const std::vector<real_t>& area, const std::vector<real_t>& center,
                                 const std::vector<int64_t>& b_cell, const std::vector<real_t>& b_area,
                                 const std::vector<real_t>& b_center, const std::vector<real_t>& volume) {
    StencilMatrix m;
    detail::check(storm_hip_op_create_from_mesh(ctx.handle(), (int64_t)n_owned, (int64_t)n_halo, (int32_t)dim,
                                                (int64_t)inner.size(), inner.data(), outer.data(), area.data(), center.data(),
                                                (int64_t)b_cell.size(), b_cell.data(), b_area.data(), b_center.data(),
                                                volume.data(), &m._h));
    return m;
  }
  static StencilMatrix from_face_weights(const Context& ctx, std::size_t n_owned, std::size_t n_halo,
                                         const std::vector<int64_t>& inner, const std::vector<int64_t>& outer,
                                         const std::vector<real_t>& w_inner, const std::vector<real_t>& w_outer,
                                         const real_t* diag_extra = nullptr) {
    StencilMatrix m;
    detail::check(storm_hip_op_create_from_face_weights(ctx.handle(), (int64_t)n_owned, (int64_t)n_halo,
                                                        (int64_t)inner.size(), inner.data(), outer.data(),
                                                        w_inner.data(), w_outer.data(), diag_extra, &m._h));
    return m;
  }
  /// The same operator with weights that set_face_weights rewrites on the device (storm_hip.h: "UPDATABLE").
  static StencilMatrix from_face_weights_updatable(const Context& ctx, std::size_t n_owned, std::size_t n_halo,
                                                   const std::vector<int64_t>& inner, const std::vector<int64_t>& outer,
                                                   const std::vector<real_t>& w_inner, const std::vector<real_t>& w_outer,
                                                   const real_t* diag_extra = nullptr) {
    StencilMatrix m;
    detail::check(storm_hip_op_create_from_face_weights_updatable(ctx.handle(), (int64_t)n_owned, (int64_t)n_halo,
                                                                  (int64_t)inner.size(), inner.data(), outer.data(),
                                                                  w_inner.data(), w_outer.data(), diag_extra, &m._h));
    return m;
  }
  /// Takes ownership of an operator handle made through the C ABI.
  static StencilMatrix adopt(storm_hip_op* handle) noexcept {
    StencilMatrix m;
    m._h = handle;
    return m;
  }
  StencilMatrix(StencilMatrix&& o) noexcept : _h(std::exchange(o._h, nullptr)) {}
  StencilMatrix& operator=(StencilMatrix&& o) noexcept {
    if (this != &o) {
      storm_hip_op_destroy(_h);
      _h = std::exchange(o._h, nullptr);
    }
    return *this;
  }
  StencilMatrix(const StencilMatrix&) = delete;
  StencilMatrix& operator=(const StencilMatrix&) = delete;
  ~StencilMatrix() { storm_hip_op_destroy(_h); }

  /// y = beta x + alpha M(x)
  void apply(real_t alpha, real_t beta, const DeviceVector& x, DeviceVector& y) const {
    detail::check(storm_hip_op_apply(_h, alpha, beta, x.handle(), y.handle()));
  }
  /// y += alpha M(x)
  void apply_add(real_t alpha, const DeviceVector& x, DeviceVector& y) const {
    detail::check(storm_hip_op_apply_add(_h, alpha, x.handle(), y.handle()));
  }
  /// Faces of an updatable operator (the length of its face vectors); 0 for any other.
  std::size_t face_count() const {
    int64_t n = 0;
    detail::check(storm_hip_op_face_count(_h, &n));
    return (std::size_t)n;
  }
  /// The weights of an updatable operator from face vectors (face_count() elements), the diagonal term from a cell vector
  /// (null: zeros), on the device; the operator is then the one a fresh from_face_weights with those values gives.
  void set_face_weights(const DeviceVector& w_inner, const DeviceVector& w_outer, const DeviceVector* diag_extra = nullptr) {
    detail::check(storm_hip_op_set_face_weights(_h, w_inner.handle(), w_outer.handle(), diag_extra ? diag_extra->handle() : nullptr));
  }
  /// at_inner[f] = cell[inner[f]], at_outer[f] = cell[outer[f]] over the faces of an updatable operator (either may be null).
  void cells_to_faces(const DeviceVector& cell, DeviceVector* at_inner, DeviceVector* at_outer) const {
    detail::check(storm_hip_op_cells_to_faces(_h, cell.handle(), at_inner ? at_inner->handle() : nullptr,
                                              at_outer ? at_outer->handle() : nullptr));
  }
  storm_hip_op* handle() const noexcept { return _h; }

private:
  storm_hip_op* _h = nullptr;
};

/// `stormDivGrad(mesh, u, dt, c)` (source_apps/playground/Playground.cpp:115-131): u += dt * div grad c,
/// with `matrix` holding what the face loop reads from `mesh`.  The playground's operator lambda
/// (:153-167) is then, statement for statement,
///     w_hat <<= f + sigma * (c_in - c);  stormDivGrad(L, w_hat, -Gamma, c_in);
///     c_hat <<= c_in;                    stormDivGrad(L, c_hat, -tau, w_hat);
inline void stormDivGrad(const StencilMatrix& matrix, DeviceVector& u, real_t dt, const DeviceVector& c) {
  matrix.apply_add(dt, c, u);
}

/// A mesh in host memory: exactly what stormDivGrad's face loop reads (`storm_hip_mesh`).  `read_mesh_from_tetgen`
/// (Mallard/IoTetgen.hpp:44-235) is `HostMesh::read_tetgen`; the operator over it `matrix()`.  As Playground.cpp:248-255:
///     auto mesh = HostMesh::read_tetgen("mesh/step.1.");   StencilMatrix L = mesh.matrix(ctx);
class HostMesh {
public:
  /// dim: mesh_dim_v<Mesh> the caller expects (2, 3; 0: what the node file says).  I/O errors throw std::runtime_error with
  /// the reference's message (STORM_THROW_IO, Crow/Base/Exception.hpp:35-44).
  static HostMesh read_tetgen(const std::string& prefix, int dim = 0) {
    HostMesh m;
    detail::check(storm_hip_mesh_read_tetgen(prefix.c_str(), (int32_t)dim, &m._h));
    return m;
  }
  HostMesh(HostMesh&& o) noexcept : _h(std::exchange(o._h, nullptr)) {}
  HostMesh& operator=(HostMesh&& o) noexcept {
    if (this != &o) {
      storm_hip_mesh_destroy(_h);
      _h = std::exchange(o._h, nullptr);
    }
    return *this;
  }
  HostMesh(const HostMesh&) = delete;
  HostMesh& operator=(const HostMesh&) = delete;
  ~HostMesh() { storm_hip_mesh_destroy(_h); }

  storm_hip_mesh_view view() const {
    storm_hip_mesh_view v;
    detail::check(storm_hip_mesh_get_view(_h, &v));
    return v;
  }
  std::size_t num_cells() const { return (std::size_t)view().n_cells; }
  std::size_t num_halo_cells() const { return (std::size_t)view().n_halo; }
  /// The gather-form operator of the face loop over this mesh (boundary faces skipped like `interior_faces()`,
  /// Playground.cpp:119, when `neumann`; otherwise they carry a homogeneous Dirichlet ghost value).
  StencilMatrix matrix(const Context& ctx, bool neumann = false) const {
    if (!neumann) return StencilMatrix::adopt(create(ctx, _h));
    const storm_hip_mesh_view v = view();
    storm_hip_mesh* interior = nullptr;  // the same mesh without its labelled faces
    detail::check(storm_hip_mesh_create(v.dim, v.n_cells, v.n_halo, v.n_faces, v.inner, v.outer, v.area, v.center, v.volume, 0,
                                        nullptr, nullptr, nullptr, v.global_id, v.halo_owner, &interior));
    storm_hip_op* op = nullptr;
    const int st = storm_hip_op_create_from_mesh_object(ctx.handle(), interior, &op);
    storm_hip_mesh_destroy(interior);
    detail::check(st);
    return StencilMatrix::adopt(op);
  }
  storm_hip_mesh* handle() const noexcept { return _h; }

private:
  HostMesh() = default;
  static storm_hip_op* create(const Context& ctx, const storm_hip_mesh* mesh) {
    storm_hip_op* op = nullptr;
    detail::check(storm_hip_op_create_from_mesh_object(ctx.handle(), mesh, &op));
    return op;
  }
  storm_hip_mesh* _h = nullptr;
};

/// `Field<Mesh, Index, Value, NumVars>` with NumVars = k > 1 (Feathers/Field.hpp:56-79): k interleaved columns over n
/// cells, element (i, j) at i k + j, 1 <= k <= 8.  It IS a DeviceVector of n k elements: every vector statement,
/// dot_product and norm_2 work on it (over all columns, as Bittern's do on such a field).
class DeviceBlockVector : public DeviceVector {
public:
  DeviceBlockVector() = default;
  DeviceBlockVector(const Context& ctx, std::size_t n, std::size_t k) : DeviceVector(ctx, n * k, 0), _k{k} {
    if (k < 1 || k > 8) throw std::invalid_argument("DeviceBlockVector: k outside [1, 8]");
  }
  DeviceBlockVector(DeviceBlockVector&& o) noexcept : DeviceVector(std::move(o)), _k{o._k} {}
  DeviceBlockVector& operator=(DeviceBlockVector&& o) noexcept {
    DeviceVector::operator=(std::move(o));
    _k = o._k;
    return *this;
  }

  /// Field::assign(other, copy): a new zero-initialised block shaped like `other`.
  void assign(const DeviceBlockVector& other, bool copy = true) {
    DeviceVector::assign(other, copy);
    _k = other._k;
  }
  /// Field::shape() = {N, NumVars}  (Field.hpp:77-79)
  std::array<std::size_t, 2> shape() const { return {DeviceVector::size() / _k, _k}; }
  std::size_t num_cells() const { return shape()[0]; }
  std::size_t num_vars() const noexcept { return _k; }
  /// Field::operator()(row, col) (Field.hpp:104-111): a host proxy, one blocking 8-byte copy per call.
  real_t operator()(std::size_t row, std::size_t col) const { return DeviceVector::operator()(row * _k + col); }

  /// Column j as / from a plain n-vector (strided copies on the device).
  void get_column(std::size_t j, DeviceVector& v) const {
    detail::check(storm_hip_block_get_column(handle(), (int)_k, (int)j, v.handle()));
  }
  void set_column(std::size_t j, const DeviceVector& v) {
    detail::check(storm_hip_block_set_column(handle(), (int)_k, (int)j, v.handle()));
  }

private:
  std::size_t _k = 1;
};

/// out[j] = <A_j, B_j>: dot_product (MatrixAlgorithms.hpp:310-317) column by column.
inline std::vector<real_t> block_dot(const DeviceBlockVector& a, const DeviceBlockVector& b) {
  std::vector<real_t> out(a.num_vars());
  detail::check(storm_hip_block_dot(a.handle(), b.handle(), (int)a.num_vars(), out.data()));
  return out;
}
/// Y_j = fma(coefs[j], X_j, Y_j): `y += a * x` with one coefficient per column.
inline void block_axpy(DeviceBlockVector& y, const std::vector<real_t>& coefs, const DeviceBlockVector& x) {
  if (coefs.size() != y.num_vars()) throw std::invalid_argument("block_axpy: one coefficient per column");
  detail::check(storm_hip_block_axpy(y.handle(), coefs.data(), x.handle(), (int)y.num_vars()));
}

/// A = beta I + alpha M as an Operator<DeviceVector> (the caller keeps `matrix` alive, as the
/// reference's operator lambdas capture the mesh by reference, Playground.cpp:152-167).
class HipStencilOperator final : public Operator<DeviceVector> {
public:
  HipStencilOperator(const StencilMatrix& matrix, real_t alpha, real_t beta)
      : _matrix{&matrix}, _alpha{alpha}, _beta{beta} {}
  void mul(DeviceVector& y_vec, const DeviceVector& x_vec) const override {
    _matrix->apply(_alpha, _beta, x_vec, y_vec);
  }
  /// `mul` on a block: Y_j = A X_j for every column, the operator's records streamed once; column by column the
  /// bits of `mul`.  Needs fp64 records (a matrix built with option spmv_dict = 0).
  void mul_block(DeviceBlockVector& y_block, const DeviceBlockVector& x_block) const {
    detail::check(storm_hip_op_apply_block(_matrix->handle(), _alpha, _beta, (int)x_block.num_vars(), x_block.handle(),
                                           y_block.handle()));
  }
  /// Give the matrix (fp64 records: option spmv_dict = 0) its fp32-weight companion records (storm_hip_op_build_reduced;
  /// idempotent): what a ChebyshevPreconditioner with `reduced_records` reads.  A weight outside fp32's normal range throws.
  void build_reduced() const { detail::check(storm_hip_op_build_reduced(_matrix->handle())); }
  const StencilMatrix& matrix() const noexcept { return *_matrix; }
  real_t alpha() const noexcept { return _alpha; }
  real_t beta() const noexcept { return _beta; }

private:
  const StencilMatrix* _matrix;
  real_t _alpha, _beta;
};

/// A = beta2 I + alpha2 M (beta1 I + alpha1 M) over one StencilMatrix as an Operator<DeviceVector>: the linear part of
/// the playground's Cahn-Hilliard lambda (Playground.cpp:153-167, two stormDivGrad calls per apply; beta1 = sigma,
/// alpha1 = -Gamma, beta2 = 1, alpha2 = -tau).  The solvers bind it natively -- no callback; CG on a small mesh is one
/// cooperative kernel per solve (storm_hip_solve_cg2).  `intermediate` (optional; the caller keeps it alive) receives
/// t = beta1 x + alpha1 M x of every `mul`: the lambda's w_hat minus its constant part.
class HipTwoStageOperator final : public Operator<DeviceVector> {
public:
  HipTwoStageOperator(const StencilMatrix& matrix, real_t alpha1, real_t beta1, real_t alpha2, real_t beta2,
                      DeviceVector* intermediate = nullptr)
      : _matrix{&matrix}, _alpha1{alpha1}, _beta1{beta1}, _alpha2{alpha2}, _beta2{beta2}, _intermediate{intermediate} {}
  void mul(DeviceVector& y_vec, const DeviceVector& x_vec) const override {
    detail::check(storm_hip_op_apply2(_matrix->handle(), _alpha1, _beta1, _alpha2, _beta2, x_vec.handle(),
                                      _intermediate != nullptr ? _intermediate->handle() : nullptr, y_vec.handle()));
  }
  const StencilMatrix& matrix() const noexcept { return *_matrix; }
  real_t alpha1() const noexcept { return _alpha1; }
  real_t beta1() const noexcept { return _beta1; }
  real_t alpha2() const noexcept { return _alpha2; }
  real_t beta2() const noexcept { return _beta2; }

private:
  const StencilMatrix* _matrix;
  real_t _alpha1, _beta1, _alpha2, _beta2;
  DeviceVector* _intermediate;
};

/// The finite-difference Jacobian of `any_op` at `x_vec` (SolverNewton.hpp:143-156) as an Operator<DeviceVector>:
/// z = (A(x + delta y) - w) / delta with w_vec = A(x_vec) (the caller forms it) and delta = safe_divide(mu, |y|).  The
/// solvers bind it natively (storm_hip_krylov_set_operator_fd): |y|, delta and 1 / delta stay on the device, the two
/// statements around `any_op.mul` are one kernel each and the reductions the method takes of z ride in the second, so
/// `solve<GmresSolver>(t, r, HipFdJacobianOperator{op, x, w, mu})` solves J(x) t = r without a host wait per product.
/// The three objects must outlive the operator; x_vec and w_vec stay unchanged during a solve.
class HipFdJacobianOperator final : public Operator<DeviceVector> {
public:
  HipFdJacobianOperator(const Operator<DeviceVector>& any_op, const DeviceVector& x_vec, const DeviceVector& w_vec, real_t mu)
      : _op{&any_op}, _x{&x_vec}, _w{&w_vec}, _mu{mu} {}
  HipFdJacobianOperator(const HipFdJacobianOperator&) = delete;
  HipFdJacobianOperator& operator=(const HipFdJacobianOperator&) = delete;
  ~HipFdJacobianOperator() override { storm_hip_krylov_destroy(_k); }  // (waits for the stream, once)
  /// z = J(y) outside a solve: storm_hip_krylov_apply on an object of its own, created by the first call and kept --
  /// every later call only enqueues (the callback runs on the host inside the call, so `bound` may live on its stack).
  void mul(DeviceVector& z_vec, const DeviceVector& y_vec) const override {
    storm_hip_ctx* ctx = nullptr;
    detail::check(storm_hip_vec_context(z_vec.handle(), &ctx));
    if (_k == nullptr || ctx != _ctx) {
      storm_hip_krylov_destroy(_k);
      _k = nullptr;
      detail::check(storm_hip_krylov_create(ctx, STORM_HIP_BICGSTAB, &_k));
      _ctx = ctx;
    }
    Bound bound{_op, nullptr};
    int st = storm_hip_krylov_set_operator_fd(_k, &HipFdJacobianOperator::trampoline, &bound, _x->handle(), _w->handle(), _mu);
    if (st == STORM_HIP_OK) st = storm_hip_krylov_apply(_k, y_vec.handle(), z_vec.handle());
    if (bound.thrown) std::rethrow_exception(bound.thrown);
    detail::check(st);
  }
  const Operator<DeviceVector>& op() const noexcept { return *_op; }
  const DeviceVector& x() const noexcept { return *_x; }
  const DeviceVector& w() const noexcept { return *_w; }
  real_t mu() const noexcept { return _mu; }

private:
  struct Bound {
    const Operator<DeviceVector>* op;
    std::exception_ptr thrown;
  };
  static int trampoline(void* user, storm_hip_vec* y, const storm_hip_vec* x) noexcept {
    auto* bound = static_cast<Bound*>(user);
    try {
      DeviceVector y_view = DeviceVector::view_of(y);
      const DeviceVector x_view = DeviceVector::view_of(const_cast<storm_hip_vec*>(x));
      bound->op->mul(y_view, x_view);
      return 0;
    } catch (...) {
      bound->thrown = std::current_exception();
      return 1;
    }
  }
  const Operator<DeviceVector>* _op;
  const DeviceVector *_x, *_w;
  real_t _mu;
  mutable storm_hip_krylov* _k = nullptr;
  mutable storm_hip_ctx* _ctx = nullptr;
};

/// What one column of a block solve reports: the fields of IterativeSolver (Solver.hpp:66-72) after `solve`.
struct BlockColumnResult {
  std::size_t iteration = 0;
  real_t absolute_error = 0.0, relative_error = 0.0, initial_error = 0.0;
  bool converged = false;
  std::vector<real_t> history;  // with record_history: iteration + 1 residual norms
};
/// k independent CG solves A x_j = b_j on the columns of a block (storm_hip_solve_cg_block): SolverCg.hpp:54-126 and the
/// convergence rule of Solver.hpp:116-147 per column, with the reference's knob names and defaults.
inline std::vector<BlockColumnResult> solve_block_cg(DeviceBlockVector& x_block, const DeviceBlockVector& b_block,
                                                     const HipStencilOperator& op, std::size_t num_iterations = 2000,
                                                     real_t absolute_error_tolerance = 1.0e-6,
                                                     real_t relative_error_tolerance = 1.0e-6, bool record_history = false) {
  const std::size_t k = b_block.num_vars();
  storm_hip_solver_params p;
  storm_hip_solver_params_default(&p);
  p.num_iterations = (int64_t)num_iterations;
  p.absolute_error_tolerance = absolute_error_tolerance;
  p.relative_error_tolerance = relative_error_tolerance;
  std::vector<storm_hip_solver_result> res(k);
  std::vector<real_t> hist(record_history ? k * (num_iterations + 1) : 0);
  detail::check(storm_hip_solve_cg_block(op.matrix().handle(), op.alpha(), op.beta(), (int)k, b_block.handle(), x_block.handle(),
                                         &p, res.data(), record_history ? hist.data() : nullptr));
  std::vector<BlockColumnResult> out(k);
  for (std::size_t j = 0; j < k; ++j) {
    out[j].iteration = (std::size_t)res[j].iterations;
    out[j].absolute_error = res[j].absolute_error, out[j].relative_error = res[j].relative_error;
    out[j].initial_error = res[j].initial_error, out[j].converged = res[j].converged != 0;
    if (record_history)
      out[j].history.assign(hist.begin() + (std::ptrdiff_t)(j * (num_iterations + 1)),
                            hist.begin() + (std::ptrdiff_t)(j * (num_iterations + 1) + out[j].iteration + 1));
  }
  return out;
}

// ---------------------------------------------------------------------------------------------
#ifndef STORM_HIP_NO_SOLVERS
enum class PreconditionerSide { Left, Right, Symmetric };

template<class Vector>
class Preconditioner : public Operator<Vector> {
public:
  virtual void build(const Vector& /*x_vec*/, const Vector& /*b_vec*/, const Operator<Vector>& /*any_op*/) {}
  virtual void add_secant(const Vector& /*y_vec*/, const Vector& /*s_vec*/) {}
};

template<class Vector>
class IdentityPreconditioner final : public Preconditioner<Vector> {
  void mul(Vector& y_vec, const Vector& x_vec) const override { y_vec <<= x_vec; }
  void conj_mul(Vector& x_vec, const Vector& y_vec) const override { x_vec <<= y_vec; }
};

#endif  // STORM_HIP_NO_SOLVERS

/// Diagonal preconditioner P = diag(A)^-1 of a HipStencilOperator, entirely on the device: the
/// build's own addition behind the reference's pre_op hook (Solver.hpp:74-75).  `build`
/// (Preconditioner.hpp:70-72) reads the diagonal of the operator it is given.
class JacobiPreconditioner final : public Preconditioner<DeviceVector> {
public:
  void build(const DeviceVector& x_vec, const DeviceVector& /*b_vec*/,
             const Operator<DeviceVector>& any_op) override {
    if (dynamic_cast<const HipTwoStageOperator*>(&any_op) != nullptr)
      throw std::runtime_error("JacobiPreconditioner cannot read the diagonal of a HipTwoStageOperator");
    const auto* hip_op = dynamic_cast<const HipStencilOperator*>(&any_op);
    if (hip_op == nullptr) throw std::runtime_error("JacobiPreconditioner needs a HipStencilOperator");
    _dinv.assign(x_vec, false);
    detail::check(storm_hip_op_get_diagonal(hip_op->matrix().handle(), hip_op->alpha(), hip_op->beta(), 1,
                                            _dinv.handle()));
  }
  void mul(DeviceVector& y_vec, const DeviceVector& x_vec) const override { vmul(y_vec, _dinv, x_vec); }
  void conj_mul(DeviceVector& x_vec, const DeviceVector& y_vec) const override { vmul(x_vec, _dinv, y_vec); }
  const DeviceVector& inverse_diagonal() const noexcept { return _dinv; }

private:
  DeviceVector _dinv;
};

/// Chebyshev polynomial preconditioner z = p_m(diag(s) A) diag(s) r of a HipStencilOperator (storm_hip_cheb_*,
/// storm_hip.h): `degree` operator products per apply, no reduction, no host wait.  lambda_max <= 0 takes Gershgorin's
/// bound, lambda_min <= 0 a thirtieth of lambda_max; `jacobi` scales with the inverse diagonal.  The knob-holder solvers
/// bind it natively; `mul` is storm_hip_cheb_apply.  The operator it was built from must outlive it.  `reduced_records`:
/// the operator products read the matrix's fp32-weight companion records (built here if missing) -- the polynomial of the
/// operator with weights rounded to fp32; every vector and sum stays fp64 (storm_hip.h, "fp32-weight companion records").
class ChebyshevPreconditioner final : public Preconditioner<DeviceVector> {
public:
  int degree = 4;
  real_t lambda_min = 0.0, lambda_max = 0.0;
  bool jacobi = false;
  bool reduced_records = false;

  ChebyshevPreconditioner() = default;
  explicit ChebyshevPreconditioner(int degree_, real_t lambda_min_ = 0.0, real_t lambda_max_ = 0.0, bool jacobi_ = false)
      : degree(degree_), lambda_min(lambda_min_), lambda_max(lambda_max_), jacobi(jacobi_) {}
  ChebyshevPreconditioner(const ChebyshevPreconditioner&) = delete;
  ChebyshevPreconditioner& operator=(const ChebyshevPreconditioner&) = delete;
  ~ChebyshevPreconditioner() override { storm_hip_cheb_destroy(_h); }

  void build(const DeviceVector& x_vec, const DeviceVector& /*b_vec*/, const Operator<DeviceVector>& any_op) override {
    if (dynamic_cast<const HipTwoStageOperator*>(&any_op) != nullptr)
      throw std::runtime_error("ChebyshevPreconditioner cannot take a HipTwoStageOperator");
    const auto* hip_op = dynamic_cast<const HipStencilOperator*>(&any_op);
    if (hip_op == nullptr) throw std::runtime_error("ChebyshevPreconditioner needs a HipStencilOperator");
    storm_hip_cheb_destroy(_h);
    _h = nullptr;
    if (jacobi) {
      _dinv.assign(x_vec, false);
      detail::check(storm_hip_op_get_diagonal(hip_op->matrix().handle(), hip_op->alpha(), hip_op->beta(), 1, _dinv.handle()));
    }
    if (reduced_records) {
      hip_op->build_reduced();
      detail::check(storm_hip_cheb_create_reduced(hip_op->matrix().handle(), hip_op->alpha(), hip_op->beta(),
                                                  jacobi ? _dinv.handle() : nullptr, degree, lambda_min, lambda_max, &_h));
    } else {
      detail::check(storm_hip_cheb_create(hip_op->matrix().handle(), hip_op->alpha(), hip_op->beta(),
                                          jacobi ? _dinv.handle() : nullptr, degree, lambda_min, lambda_max, &_h));
    }
  }
  void mul(DeviceVector& y_vec, const DeviceVector& x_vec) const override {
    detail::check(storm_hip_cheb_apply(_h, x_vec.handle(), y_vec.handle()));
  }
  void conj_mul(DeviceVector& x_vec, const DeviceVector& y_vec) const override {
    detail::check(storm_hip_cheb_apply(_h, y_vec.handle(), x_vec.handle()));
  }
  /// "lambda_min" / "lambda_max" (the bounds in use), "degree" or "reduced".
  real_t get(const char* key) const {
    double v = 0.0;
    detail::check(storm_hip_cheb_get(_h, key, &v));
    return v;
  }
  const storm_hip_cheb* handle() const noexcept { return _h; }

private:
  DeviceVector _dinv;
  storm_hip_cheb* _h = nullptr;
};

/// Smoothed-aggregation multigrid preconditioner for a HipStencilOperator on fp64 records (storm_hip_amg_*, storm_hip.h,
/// "Smoothed-aggregation multigrid preconditioner"): one symmetric V-cycle per apply with Jacobi-scaled Chebyshev smoothers,
/// no reduction and no host wait inside an apply.  For symmetric operators, single rank.  `build` runs the setup on the host
/// and uploads the hierarchy -- once: a solver calls it before every solve, and it returns at once while matrix, alpha, beta
/// and `params` are those of the last build; the solvers bind the object natively; `mul` is storm_hip_amg_apply.  The
/// operator it was built from must outlive it; after StencilMatrix::set_face_weights the object is stale: `reset()` it --
/// or, if `refreshable` (set before the build; the matrix must come from from_face_weights_updatable), `refresh()` it: every
/// number of the hierarchy is recomputed on the device on the structure the setup froze (storm_hip_amg_refresh).
/// `params.reduced_records`: every level's smoother reads fp32-weight companion records (the matrix gets one if missing).
/// `nullspace_constant` (set before the build): for a singular operator whose kernel is the constants -- a pure-Neumann
/// pressure equation -- the object is storm_hip_amg_create_nullspace's: the cycle between two projections onto the mean-free
/// vectors, and `project(v)` is v <- v - mean(v).
/// `smoother.kind = 1` (set before the build; `use_jacobi(sweeps, omega)`): damped Jacobi sweeps instead of the Chebyshev
/// polynomial (storm_hip_amg_create_smoother) -- the smoother for a non-symmetric operator such as upwind
/// convection-diffusion; `smooth` is one sweep on its own.  Not with `refreshable` or `nullspace_constant`: build() throws.
class AmgPreconditioner final : public Preconditioner<DeviceVector> {
public:
  storm_hip_amg_params params;
  bool refreshable = false;  ///< read by build(): storm_hip_amg_create_refreshable instead of storm_hip_amg_create
  bool nullspace_constant = false;  ///< read by build(): storm_hip_amg_create_nullspace (with `refreshable` as its flag)
  storm_hip_amg_smoother smoother;  ///< read by build(): kind 0 (the default here) Chebyshev, 1 Jacobi with `sweeps`, `omega`

  AmgPreconditioner() {
    storm_hip_amg_params_default(&params);
    storm_hip_amg_smoother_default(&smoother);
    smoother.kind = 0;  // (every default keeps its behaviour: the Jacobi smoother is opt-in)
  }
  /// Smooth by `sweeps` damped Jacobi sweeps with `omega` before and after the coarse correction.
  AmgPreconditioner& use_jacobi(int sweeps = 2, real_t omega = 2.0 / 3.0) {
    smoother.kind = 1, smoother.sweeps = sweeps, smoother.omega = omega;
    return *this;
  }
  explicit AmgPreconditioner(int smoother_degree, bool reduced_records = false) : AmgPreconditioner() {
    params.smoother_degree = smoother_degree;
    params.reduced_records = reduced_records ? 1 : 0;
  }
  AmgPreconditioner(const AmgPreconditioner&) = delete;
  AmgPreconditioner& operator=(const AmgPreconditioner&) = delete;
  ~AmgPreconditioner() override { storm_hip_amg_destroy(_h); }

  void build(const DeviceVector& /*x_vec*/, const DeviceVector& /*b_vec*/, const Operator<DeviceVector>& any_op) override {
    if (dynamic_cast<const HipTwoStageOperator*>(&any_op) != nullptr)
      throw std::runtime_error("AmgPreconditioner cannot take a HipTwoStageOperator");
    const auto* hip_op = dynamic_cast<const HipStencilOperator*>(&any_op);
    if (hip_op == nullptr) throw std::runtime_error("AmgPreconditioner needs a HipStencilOperator");
    // a solver calls build() before every solve: the hierarchy is kept while operator and parameters are the same
    // (a matrix whose weights were refreshed is the same handle: reset() first -- staleness is the caller's)
    if (_h != nullptr && _op == hip_op->matrix().handle() && _alpha == hip_op->alpha() && _beta == hip_op->beta() &&
        _built.strength_theta == params.strength_theta && _built.prolongator_omega == params.prolongator_omega &&
        _built.smoother_degree == params.smoother_degree && _built.smoother_ratio == params.smoother_ratio &&
        _built.max_levels == params.max_levels && _built.coarse_rows == params.coarse_rows &&
        _built.reduced_records == params.reduced_records && _built_refreshable == refreshable &&
        _built_nullspace == nullspace_constant && _built_smoother.kind == smoother.kind &&
        (smoother.kind == 0 || (_built_smoother.sweeps == smoother.sweeps && _built_smoother.omega == smoother.omega)))
      return;
    reset();
    if (smoother.kind != 0) {
      if (refreshable || nullspace_constant)
        throw std::runtime_error("AmgPreconditioner: the Jacobi smoother cannot be combined with refreshable or nullspace_constant");
      detail::check(storm_hip_amg_create_smoother(hip_op->matrix().handle(), hip_op->alpha(), hip_op->beta(), &params, &smoother, &_h));
    } else if (nullspace_constant)
      detail::check(storm_hip_amg_create_nullspace(hip_op->matrix().handle(), hip_op->alpha(), hip_op->beta(), &params,
                                                   refreshable ? 1 : 0, &_h));
    else if (refreshable)
      detail::check(storm_hip_amg_create_refreshable(hip_op->matrix().handle(), hip_op->alpha(), hip_op->beta(), &params, &_h));
    else
      detail::check(storm_hip_amg_create(hip_op->matrix().handle(), hip_op->alpha(), hip_op->beta(), &params, &_h));
    _op = hip_op->matrix().handle(), _alpha = hip_op->alpha(), _beta = hip_op->beta(), _built = params;
    _built_refreshable = refreshable, _built_nullspace = nullspace_constant, _built_smoother = smoother;
  }
  /// One Jacobi sweep z_out = z_in + sigma_l (s .* (r - A_l z_in)) on level l (a Jacobi object; storm_hip_amg_smooth).
  void smooth(int level, const DeviceVector& r, const DeviceVector& z_in, DeviceVector& z_out) const {
    detail::check(storm_hip_amg_smooth(_h, level, r.handle(), z_in.handle(), z_out.handle()));
  }
  /// v <- v - mean(v) in place (a `nullspace_constant` object; storm_hip_amg_project).
  void project(DeviceVector& v) const { detail::check(storm_hip_amg_project(_h, v.handle())); }
  /// Recompute every number of the hierarchy from the matrix's current records (a refreshable object; waits on the host).
  void refresh() { detail::check(storm_hip_amg_refresh(_h)); }
  /// Bring the host hierarchy (storm_hip_amg_get_hierarchy) up to date with what the cycle reads on the device.
  void download() { detail::check(storm_hip_amg_download(_h)); }
  /// Drop the hierarchy: the next build() runs the setup again (after set_face_weights, for instance).
  void reset() noexcept {
    storm_hip_amg_destroy(_h);
    _h = nullptr;
  }
  void mul(DeviceVector& y_vec, const DeviceVector& x_vec) const override {
    detail::check(storm_hip_amg_apply(_h, x_vec.handle(), y_vec.handle()));
  }
  void conj_mul(DeviceVector& x_vec, const DeviceVector& y_vec) const override {
    detail::check(storm_hip_amg_apply(_h, y_vec.handle(), x_vec.handle()));
  }
  /// "levels", "operator_complexity", "grid_complexity", "setup_seconds", "upload_seconds", "device_bytes",
  /// "transfer_padding", "smoother_degree", "reduced", "nullspace", "coarse_shift", "smoother_kind", "jacobi_sweeps",
  /// "jacobi_omega" or "jacobi_sigma_<level>".
  real_t get(const char* key) const {
    double v = 0.0;
    detail::check(storm_hip_amg_get(_h, key, &v));
    return v;
  }
  /// Rows of every level, finest first.
  std::vector<int64_t> level_rows() const {
    const storm_hip_amg_hierarchy* hier = nullptr;
    detail::check(storm_hip_amg_get_hierarchy(_h, &hier));
    int levels = 0;
    detail::check(storm_hip_amg_hierarchy_levels(hier, &levels));
    std::vector<int64_t> rows((size_t)levels);
    for (int l = 0; l < levels; ++l) {
      int64_t nnz_a = 0, n_agg = 0, nnz_p = 0;
      detail::check(storm_hip_amg_hierarchy_level_sizes(hier, l, &rows[(size_t)l], &nnz_a, &n_agg, &nnz_p));
    }
    return rows;
  }
  const storm_hip_amg* handle() const noexcept { return _h; }

private:
  storm_hip_amg* _h = nullptr;
  const storm_hip_op* _op = nullptr;
  real_t _alpha = 0.0, _beta = 0.0;
  storm_hip_amg_params _built{};
  bool _built_refreshable = false, _built_nullspace = false;
  storm_hip_amg_smoother _built_smoother{};
};

/// The initial guess of a solve projected onto the solutions of earlier solves with the same operator (storm_hip_recycle_*;
/// the recipe: storm_hip.h): up to `capacity` (1 .. 16) pairs (u_j, A u_j) on the device, made orthogonal as they arrive; a
/// full object restarts from the newest pair.  Energy kind for SPD operators, residual kind for any.  Point
/// IterativeSolver::recycler at one, or call guess() before and update() after a solve yourself.  No scalar visits the
/// host in either.  Single rank.  An operator that changes between solves leaves the pairs stale: reset() is the caller's job.
class SolutionRecycler {
public:
  SolutionRecycler(const Context& ctx, std::size_t n_owned, std::size_t n_halo = 0, int capacity = 8,
                   int kind = STORM_HIP_RECYCLE_ENERGY)
      : _ctx(&ctx), _n_owned(n_owned), _n_halo(n_halo) {
    detail::check(storm_hip_recycle_create(ctx.handle(), (int64_t)n_owned, (int64_t)n_halo, capacity, kind, &_h));
  }
  SolutionRecycler(const SolutionRecycler&) = delete;
  SolutionRecycler& operator=(const SolutionRecycler&) = delete;
  ~SolutionRecycler() { (void)storm_hip_recycle_destroy(_h); }

  /// x = the projection of the solution of A x = b onto the stored pairs (zeros while there is none)
  void guess(const DeviceVector& b_vec, DeviceVector& x_vec) {
    detail::check(storm_hip_recycle_guess(_h, b_vec.handle(), x_vec.handle()));
  }
  /// take a solve's x in, with ax = A x
  void update(const DeviceVector& x_vec, const DeviceVector& ax_vec) {
    detail::check(storm_hip_recycle_update(_h, x_vec.handle(), ax_vec.handle()));
  }
  /// ... with A x formed by `any_op` in a scratch vector of the object's
  void update(const DeviceVector& x_vec, const Operator<DeviceVector>& any_op) {
    if (_ax == nullptr) _ax = std::make_unique<DeviceVector>(*_ctx, _n_owned, _n_halo);
    any_op.mul(*_ax, x_vec);
    update(x_vec, *_ax);
  }
  void reset() { detail::check(storm_hip_recycle_reset(_h)); }
  /// "capacity", "count", "kind", "updates", "restarts", "device_bytes"; "weight_<j>", "coef_<j>" (these two wait for the stream)
  real_t get(const char* key) const {
    double v = 0.0;
    detail::check(storm_hip_recycle_get(_h, key, &v));
    return v;
  }
  /// copies of pair j into u and v; returns its weight g_j (for a checkpoint, for tests)
  real_t slot(int j, DeviceVector& u, DeviceVector& v) const {
    double g = 0.0;
    detail::check(storm_hip_recycle_get_slot(_h, j, u.handle(), v.handle(), &g));
    return g;
  }
  /// load pair j <= count (j == count appends); the caller answers for the pairs being orthogonal
  void set_slot(int j, const DeviceVector& u, const DeviceVector& v, real_t g) {
    detail::check(storm_hip_recycle_set_slot(_h, j, u.handle(), v.handle(), g));
  }
  storm_hip_recycle* handle() const noexcept { return _h; }

private:
  storm_hip_recycle* _h = nullptr;
  const Context* _ctx;
  std::size_t _n_owned, _n_halo;
  std::unique_ptr<DeviceVector> _ax;
};

#ifndef STORM_HIP_NO_SOLVERS
// ---------------------------------------------------------------------------------------------
template<class InVector, class OutVector = InVector>
class Solver {
public:
  virtual ~Solver() = default;
  virtual bool solve(InVector& x_vec, const OutVector& b_vec, const Operator<InVector, OutVector>& any_op) = 0;
};

namespace detail {
inline std::function<void(const std::string&)>& log_sink() {
  static std::function<void(const std::string&)> sink;  // empty: silent
  return sink;
}
inline void log_solve(std::size_t iteration, real_t absolute_error, real_t relative_error) {
  if (!log_sink()) return;
  char line[128];
  std::snprintf(line, sizeof line, "n_iter: %4zu, abs_err: %-12e, rel_err: %-12e", iteration, absolute_error,
                relative_error);
  log_sink()(line);
}

/// One `storm_hip_krylov` object -- the library's device-resident solver loops (csrc/krylov.hip) -- with the
/// caller's Operator / Preconditioner objects bound to it.  A HipStencilOperator, HipTwoStageOperator or HipFdJacobianOperator
/// (its inner operator as the callback) binds natively; any other
/// operator (a lambda through make_operator, Playground.cpp:151-167) and any preconditioner but the Jacobi
/// and the Chebyshev one bind as callbacks, which only enqueue kernels.  An exception thrown inside a callback aborts the solve
/// and is rethrown from the call that ran it.
class Engine {
public:
  Engine() = default;
  Engine(const Engine&) = delete;
  Engine& operator=(const Engine&) = delete;
  ~Engine() { storm_hip_krylov_destroy(_h); }

  void bind(int method, const DeviceVector& like, const Operator<DeviceVector>& any_op,
            const Preconditioner<DeviceVector>* pre_op, PreconditionerSide side) {
    storm_hip_ctx* ctx = nullptr;
    check(storm_hip_vec_context(like.handle(), &ctx));
    if (_h == nullptr || ctx != _ctx || method != _method) {
      storm_hip_krylov_destroy(_h);
      _h = nullptr;
      check(storm_hip_krylov_create(ctx, method, &_h));
      _ctx = ctx, _method = method;
    }
    _op = Bound{&any_op, &_thrown};
    if (const auto* hip_op = dynamic_cast<const HipStencilOperator*>(&any_op))
      check(storm_hip_krylov_set_operator(_h, hip_op->matrix().handle(), hip_op->alpha(), hip_op->beta()));
    else if (const auto* two = dynamic_cast<const HipTwoStageOperator*>(&any_op))
      check(storm_hip_krylov_set_operator2(_h, two->matrix().handle(), two->alpha1(), two->beta1(), two->alpha2(), two->beta2()));
    else if (const auto* fd = dynamic_cast<const HipFdJacobianOperator*>(&any_op)) {
      _op = Bound{&fd->op(), &_thrown};
      check(storm_hip_krylov_set_operator_fd(_h, &Engine::trampoline, &_op, fd->x().handle(), fd->w().handle(), fd->mu()));
    } else
      check(storm_hip_krylov_set_operator_fn(_h, &Engine::trampoline, &_op));
    const int c_side = side == PreconditionerSide::Left    ? STORM_HIP_LEFT
                       : side == PreconditionerSide::Right ? STORM_HIP_RIGHT
                                                           : STORM_HIP_SYMMETRIC;
    _pre = Bound{pre_op, &_thrown};
    if (pre_op == nullptr)
      check(storm_hip_krylov_set_preconditioner_diag(_h, nullptr, c_side));
    else if (const auto* jacobi = dynamic_cast<const JacobiPreconditioner*>(pre_op))
      check(storm_hip_krylov_set_preconditioner_diag(_h, jacobi->inverse_diagonal().handle(), c_side));
    else if (const auto* cheb = dynamic_cast<const ChebyshevPreconditioner*>(pre_op))
      check(storm_hip_krylov_set_preconditioner_cheb(_h, cheb->handle(), c_side));
    else if (const auto* amg = dynamic_cast<const AmgPreconditioner*>(pre_op))
      check(storm_hip_krylov_set_preconditioner_amg(_h, amg->handle(), c_side));
    else
      check(storm_hip_krylov_set_preconditioner_fn(_h, &Engine::trampoline, &_pre, c_side));
  }
  storm_hip_krylov* handle() const noexcept { return _h; }
  /// Status of a library call that may have run callbacks.
  void finish(int status) {
    if (_thrown) std::rethrow_exception(std::exchange(_thrown, nullptr));
    check(status);
  }

private:
  struct Bound {
    const Operator<DeviceVector>* op;
    std::exception_ptr* thrown;
  };
  static int trampoline(void* user, storm_hip_vec* y, const storm_hip_vec* x) noexcept {
    auto* bound = static_cast<Bound*>(user);
    try {
      DeviceVector y_view = DeviceVector::view_of(y);
      const DeviceVector x_view = DeviceVector::view_of(const_cast<storm_hip_vec*>(x));
      bound->op->mul(y_view, x_view);
      return 0;
    } catch (...) {
      *bound->thrown = std::current_exception();
      return 1;
    }
  }
  storm_hip_krylov* _h = nullptr;
  storm_hip_ctx* _ctx = nullptr;
  int _method = -1;
  Bound _op{nullptr, nullptr}, _pre{nullptr, nullptr};
  std::exception_ptr _thrown;
};
}  // namespace detail

/// The reference logs one line per solve through spdlog (`STORM_INFO("n_iter: ..., abs_err: ..., rel_err: ...")`,
/// Solvers/Solver.hpp:144-145).  This header has no logging dependency: install a sink to receive the same
/// line (e.g. `Storm::set_log_sink([](const std::string& s) { spdlog::info(s); })`); none installed = silent.
inline void set_log_sink(std::function<void(const std::string&)> sink) { detail::log_sink() = std::move(sink); }

namespace detail {
/// Option `lazy_statements` on the vector's context for the lifetime of the scope (leaving it launches what still waits).
struct LazyScope {
  storm_hip_ctx* ctx = nullptr;
  template<class V>
  LazyScope(const V& v, bool on) {
    if constexpr (std::is_same_v<V, DeviceVector>) {
      if (on && v.handle() != nullptr && storm_hip_vec_context(v.handle(), &ctx) == STORM_HIP_OK && ctx != nullptr)
        (void)storm_hip_ctx_set_option(ctx, "lazy_statements", 2);
    }
  }
  ~LazyScope() {
    if (ctx != nullptr) (void)storm_hip_ctx_set_option(ctx, "lazy_statements", 0);
  }
  LazyScope(const LazyScope&) = delete;
  LazyScope& operator=(const LazyScope&) = delete;
};
}  // namespace detail

/// Solvers/Solver.hpp:62-149: the public knobs (names, defaults), the protected stepping hooks and `solve`.
///
/// The solvers this header ships name a library method (`device_method()`); their `solve` is ONE call,
/// `storm_hip_krylov_solve`: the loop of Solver.hpp:132-140 and every scalar of the recurrence stay on the
/// device.  Their init / iterate / finalize hooks go through `storm_hip_krylov_init / _iterate / _finalize`,
/// and `device_loop = false` runs the host loop below over them instead (one host wait per iteration).  A
/// user-defined subclass that names no method gets that host loop over its own hooks.
template<class InVector, class OutVector = InVector>
class IterativeSolver : public Solver<InVector, OutVector> {
public:
  std::size_t iteration{0};
  std::size_t num_iterations{2000};
  real_t absolute_error{0.0};
  real_t relative_error{0.0};

  real_t absolute_error_tolerance{1.0e-6};
  real_t relative_error_tolerance{1.0e-6};

  PreconditionerSide pre_side{PreconditionerSide::Right};
  std::unique_ptr<Preconditioner<InVector>> pre_op{nullptr};
  std::string name;

  // extras of this build
  bool device_loop{true};
  /// The HOST loop (a user-defined solver, or `device_loop = false`) runs with the library's option `lazy_statements`:
  /// the linear vector statements and operator applies of an `iterate()` body wait for the call that needs their result,
  /// consecutive statements leave as one pass and a `dot_product` / `norm_2` over a vector the last waiting statement
  /// writes rides in that statement's kernel (`x += alpha * p; r -= alpha * z; dot_product(r, r)`: ONE kernel).  The
  /// linear statements and their reductions give the eager kernels' bits; two things do not: a dot product riding in an
  /// operator apply sums in the SpMV kernel's order, and (level 2, what this switch selects) `x += alpha p; p <<= r +
  /// beta p; z = A p; <p, z>` on a lattice operator is ONE launch of the device loop's fused step, whose updates round
  /// as fused multiply-adds -- equal to the eager statements to rounding, not to the bit (tests/test_gpu_lazy.py).
  /// Caveat: statements wait until a library call needs their result.  A kernel of YOUR OWN that reads a vector through a
  /// pointer from `storm_hip_vec_device_ptr` must be preceded by `storm_hip_ctx_sync` (or any reduction), which flushes
  /// what waits; level 2 never exchanges the storage of a vector whose address has been handed out.
  /// `false`: every statement is a launch of its own when it is called.
  bool lazy_statements{true};
  std::size_t num_applies{0}, num_pre_applies{0};  ///< of the last device-loop solve
  real_t initial_error{0.0};  ///< |r0| of the last solve
  /// Not owned.  When set (DeviceVector solves), solve() takes its guess for x before init and hands it x and A x -- one more
  /// apply -- after the loop; null: solve() is the plain one.
  SolutionRecycler* recycler{nullptr};
  int path_fallback{0};  ///< storm_hip_solver_result::path_fallback of the last device-loop solve (0: the chosen path ran)

protected:
  virtual real_t init(const InVector& x_vec, const OutVector& b_vec, const Operator<InVector, OutVector>& any_op,
                      const Preconditioner<InVector>* pre_op) = 0;
  virtual real_t iterate(InVector& x_vec, const OutVector& b_vec, const Operator<InVector, OutVector>& any_op,
                         const Preconditioner<InVector>* pre_op) = 0;
  virtual void finalize(InVector& /*x_vec*/, const OutVector& /*b_vec*/,
                        const Operator<InVector, OutVector>& /*any_op*/, const Preconditioner<InVector>* /*pre_op*/) {}

  /// storm_hip_method of a shipped solver; -1: none (the host loop runs the hooks above).
  virtual int device_method() const noexcept { return -1; }
  virtual void fill_params(storm_hip_solver_params& /*p*/) const {}
  virtual void configure(storm_hip_krylov* /*k*/) const {}
  /// After a device-loop solve or a stepping iterate: what a shipped solver reads back from its object.
  virtual void collect(storm_hip_krylov* /*k*/) {}

  storm_hip_solver_params params() const {
    storm_hip_solver_params p;
    storm_hip_solver_params_default(&p);
    p.num_iterations = (int64_t)num_iterations;
    p.absolute_error_tolerance = absolute_error_tolerance;
    p.relative_error_tolerance = relative_error_tolerance;
    p.num_inner_iterations = 0;  // "the method's default"; InnerOuterIterativeSolver fills its knob in
    fill_params(p);
    return p;
  }
  detail::Engine _engine;

public:
  bool solve(InVector& x_vec, const OutVector& b_vec, const Operator<InVector, OutVector>& any_op) final {
    if constexpr (std::is_same_v<InVector, DeviceVector> && std::is_same_v<OutVector, DeviceVector>) {
      if (recycler != nullptr) {
        recycler->guess(b_vec, x_vec);
        const bool converged = solve_plain(x_vec, b_vec, any_op);
        recycler->update(x_vec, any_op);
        return converged;
      }
    }
    return solve_plain(x_vec, b_vec, any_op);
  }

private:
  bool solve_plain(InVector& x_vec, const OutVector& b_vec, const Operator<InVector, OutVector>& any_op) {
    if (pre_op != nullptr) pre_op->build(x_vec, b_vec, any_op);
    if constexpr (std::is_same_v<InVector, DeviceVector> && std::is_same_v<OutVector, DeviceVector>) {
      if (device_method() >= 0 && device_loop) {
        _engine.bind(device_method(), x_vec, any_op, pre_op.get(), pre_side);
        configure(_engine.handle());
        const storm_hip_solver_params p = params();
        storm_hip_solver_result r{};
        int64_t n_pre = 0;
        _engine.finish(storm_hip_krylov_solve(_engine.handle(), b_vec.handle(), x_vec.handle(), &p, &r, nullptr, &n_pre));
        iteration = (std::size_t)r.iterations;
        absolute_error = r.absolute_error, relative_error = r.relative_error, initial_error = r.initial_error;
        num_applies = (std::size_t)r.num_applies, num_pre_applies = (std::size_t)n_pre;
        path_fallback = r.path_fallback;
        collect(_engine.handle());
        detail::log_solve(iteration, absolute_error, relative_error);
        return r.converged != 0;
      }
    }
    // Host loop with the reference's rule: stop on abs_tol > 0 && abs < abs_tol, or rel_tol > 0 && abs / initial < rel_tol.
    detail::LazyScope lazy(x_vec, lazy_statements);
    initial_error = init(x_vec, b_vec, any_op, pre_op.get());
    absolute_error = initial_error;
    const auto met = [this](real_t value, real_t tolerance) { return tolerance > 0.0 && value < tolerance; };
    bool converged = met(absolute_error, absolute_error_tolerance);
    const bool silent = converged;  // the early return of Solver.hpp:124-128 logs nothing
    iteration = 0;
    while (!converged && iteration < num_iterations) {
      absolute_error = iterate(x_vec, b_vec, any_op, pre_op.get());
      relative_error = absolute_error / initial_error;
      converged = met(absolute_error, absolute_error_tolerance) || met(relative_error, relative_error_tolerance);
      ++iteration;
    }
    finalize(x_vec, b_vec, any_op, pre_op.get());
    if (!silent) detail::log_solve(iteration, absolute_error, relative_error);
    return converged;
  }
};

/// Solvers/Solver.hpp:154-259: `num_inner_iterations` and the restart bookkeeping over five hooks.  (For the shipped
/// solvers that bookkeeping lives in the library; they implement only outer_init / inner_iterate / outer_finalize.)
template<class InVector, class OutVector = InVector>
class InnerOuterIterativeSolver : public IterativeSolver<InVector, OutVector> {
public:
  std::size_t inner_iteration{0};
  std::size_t num_inner_iterations{50};

protected:
  virtual real_t outer_init(const InVector& x_vec, const OutVector& b_vec,
                            const Operator<InVector, OutVector>& any_op, const Preconditioner<InVector>* pre_op) = 0;
  virtual void inner_init(const InVector&, const OutVector&, const Operator<InVector, OutVector>&,
                          const Preconditioner<InVector>*) {}
  virtual real_t inner_iterate(InVector& x_vec, const OutVector& b_vec,
                               const Operator<InVector, OutVector>& any_op, const Preconditioner<InVector>* pre_op) = 0;
  virtual void inner_finalize(InVector&, const OutVector&, const Operator<InVector, OutVector>&,
                              const Preconditioner<InVector>*) {}
  virtual void outer_finalize(InVector&, const OutVector&, const Operator<InVector, OutVector>&,
                              const Preconditioner<InVector>*) {}

  void fill_params(storm_hip_solver_params& p) const override { p.num_inner_iterations = (int64_t)num_inner_iterations; }

private:
  bool closes_a_cycle() const noexcept { return inner_iteration + 1 == num_inner_iterations; }

  real_t init(const InVector& x_vec, const OutVector& b_vec, const Operator<InVector, OutVector>& any_op,
              const Preconditioner<InVector>* pre_op) final {
    return outer_init(x_vec, b_vec, any_op, pre_op);
  }
  real_t iterate(InVector& x_vec, const OutVector& b_vec, const Operator<InVector, OutVector>& any_op,
                 const Preconditioner<InVector>* pre_op) final {
    inner_iteration = this->iteration % num_inner_iterations;
    if (inner_iteration == 0) inner_init(x_vec, b_vec, any_op, pre_op);
    const real_t residual_norm = inner_iterate(x_vec, b_vec, any_op, pre_op);
    if (closes_a_cycle()) inner_finalize(x_vec, b_vec, any_op, pre_op);
    return residual_norm;
  }
  void finalize(InVector& x_vec, const OutVector& b_vec, const Operator<InVector, OutVector>& any_op,
                const Preconditioner<InVector>* pre_op) final {
    if (!closes_a_cycle()) inner_finalize(x_vec, b_vec, any_op, pre_op);
    outer_finalize(x_vec, b_vec, any_op, pre_op);
  }
};

template<template<class> class SolverT, class Vector>
bool solve(Vector& x_vec, const Vector& b_vec, const Operator<Vector>& any_op) {
  SolverT<Vector> solver{};
  return solver.solve(x_vec, b_vec, any_op);
}

/// A(x) = b for a non-uniform operator (A(0) != 0): solve A(x) - A(0) = b - A(0).  Solver.hpp:271-292.
template<class Vector>
bool solve_non_uniform(Solver<Vector>& solver, Vector& x_vec, const Vector& b_vec, const Operator<Vector>& any_op) {
  Vector at_zero, rhs;
  at_zero.assign(x_vec, false);
  rhs.assign(b_vec, false);
  fill_with(rhs, 0.0);
  any_op.mul(at_zero, rhs);
  rhs <<= b_vec - at_zero;
  const auto shifted = make_operator<Vector>([&](Vector& y_vec, const Vector& in_vec) {
    any_op.mul(y_vec, in_vec);
    y_vec -= at_zero;
  });
  return solver.solve(x_vec, rhs, *shifted);
}

// ---------------------------------------------------------------------------------------------
// The shipped solvers.  Each names its library method; the loop bodies are csrc/krylov.hip (and, for a stencil
// operator without preconditioner, the fused kernels of csrc/solver_cg.hip, solver_bicgstab.hip, solver_gmres.hip).  They exist for DeviceVector only.
namespace detail {

/// Stepping hooks of a shipped plain solver over the library's stepping calls.
template<class Vector, int Method>
class DeviceIterativeSolver : public IterativeSolver<Vector> {
  static_assert(std::is_same_v<Vector, DeviceVector>, "the shipped solvers run on Storm::DeviceVector");

protected:
  int device_method() const noexcept final { return Method; }
  real_t init(const Vector& x_vec, const Vector& b_vec, const Operator<Vector>& any_op,
              const Preconditioner<Vector>* pre_op) final {
    this->_engine.bind(Method, x_vec, any_op, pre_op, this->pre_side);
    this->configure(this->_engine.handle());
    const storm_hip_solver_params p = this->params();
    real_t initial_error = 0.0;
    this->_engine.finish(storm_hip_krylov_init(this->_engine.handle(), b_vec.handle(), x_vec.handle(), &p, &initial_error));
    return initial_error;
  }
  real_t iterate(Vector&, const Vector&, const Operator<Vector>&, const Preconditioner<Vector>*) final {
    real_t residual_norm = 0.0;
    this->_engine.finish(storm_hip_krylov_iterate(this->_engine.handle(), &residual_norm));
    this->collect(this->_engine.handle());
    return residual_norm;
  }
  void finalize(Vector&, const Vector&, const Operator<Vector>&, const Preconditioner<Vector>*) final {
    this->_engine.finish(storm_hip_krylov_finalize(this->_engine.handle()));
  }
};

/// The same for a restarted solver: the library restarts / updates x inside its iterate and finalize.
template<class Vector, int Method, std::size_t DefaultInner>
class DeviceInnerOuterSolver : public InnerOuterIterativeSolver<Vector> {
  static_assert(std::is_same_v<Vector, DeviceVector>, "the shipped solvers run on Storm::DeviceVector");

public:
  DeviceInnerOuterSolver() { this->num_inner_iterations = DefaultInner; }

protected:
  int device_method() const noexcept final { return Method; }
  real_t outer_init(const Vector& x_vec, const Vector& b_vec, const Operator<Vector>& any_op,
                    const Preconditioner<Vector>* pre_op) final {
    this->_engine.bind(Method, x_vec, any_op, pre_op, this->pre_side);
    this->configure(this->_engine.handle());
    const storm_hip_solver_params p = this->params();
    real_t initial_error = 0.0;
    this->_engine.finish(storm_hip_krylov_init(this->_engine.handle(), b_vec.handle(), x_vec.handle(), &p, &initial_error));
    return initial_error;
  }
  real_t inner_iterate(Vector&, const Vector&, const Operator<Vector>&, const Preconditioner<Vector>*) final {
    real_t residual_norm = 0.0;
    this->_engine.finish(storm_hip_krylov_iterate(this->_engine.handle(), &residual_norm));
    return residual_norm;
  }
  void outer_finalize(Vector&, const Vector&, const Operator<Vector>&, const Preconditioner<Vector>*) final {
    this->_engine.finish(storm_hip_krylov_finalize(this->_engine.handle()));
  }
};

}  // namespace detail

/// SolverCg.hpp:47-128.
template<class Vector>
class CgSolver final : public detail::DeviceIterativeSolver<Vector, STORM_HIP_CG> {};
/// CG whose inner iterations run on fp32 vectors and the matrix's fp32-weight companion records under an fp64 refinement
/// loop held to the reference's rule on the TRUE residual (storm_hip_mixed_cg_*; algorithm and contract:
/// include/storm_hip.h).  Opt-in, a knob holder like the solvers above: the reference's knobs and the mixed ones, the
/// results of the last solve.  Takes a HipStencilOperator on fp64 records (option spmv_dict = 0) without a CSR tail whose
/// matrix has a companion (HipStencilOperator::build_reduced); anything else throws.
class MixedCgSolver final {
public:
  std::size_t num_iterations{2000};
  real_t absolute_error_tolerance{1.0e-6}, relative_error_tolerance{1.0e-6};
  real_t inner_tolerance{1.0e-3};   ///< the inner loop leaves at this relative residual (or where the outer rule needs less)
  std::size_t inner_max{0};         ///< inner iterations per outer step; 0: num_iterations
  int max_outer{16};
  bool keep_direction{false};       ///< the direction survives the outer step (rescaled) instead of restarting
  int check_lag{0};

  // the last solve
  std::size_t iteration{0}, num_applies{0};  ///< inner iterations plus those of an fp64 finish; operator products, A~ and A alike
  real_t absolute_error{0.0}, relative_error{0.0}, initial_error{0.0};  ///< of the last TRUE residual
  std::size_t outer_steps{0}, inner_iterations{0}, fp64_iterations{0};
  int finished_fp64{0};  ///< 0 no; 1 the true residual did not fall; 2 broken; 3 max_outer or the iteration budget

  bool solve(DeviceVector& x_vec, const DeviceVector& b_vec, const HipStencilOperator& op) {
    storm_hip_mixed_params mp;
    storm_hip_mixed_params_default(&mp);
    mp.inner_tolerance = inner_tolerance, mp.inner_max = (int64_t)inner_max, mp.max_outer = max_outer;
    mp.keep_direction = keep_direction ? 1 : 0;
    storm_hip_mixed_cg* h = nullptr;
    detail::check(storm_hip_mixed_cg_create(op.matrix().handle(), op.alpha(), op.beta(), &mp, &h));
    storm_hip_solver_params p;
    storm_hip_solver_params_default(&p);
    p.num_iterations = (int64_t)num_iterations;
    p.absolute_error_tolerance = absolute_error_tolerance, p.relative_error_tolerance = relative_error_tolerance;
    p.check_lag = check_lag;
    storm_hip_solver_result r{};
    storm_hip_mixed_result mr{};
    const int status = storm_hip_mixed_cg_solve(h, b_vec.handle(), x_vec.handle(), &p, &r, nullptr, &mr);
    (void)storm_hip_mixed_cg_destroy(h);
    detail::check(status);
    iteration = (std::size_t)r.iterations, num_applies = (std::size_t)r.num_applies;
    absolute_error = r.absolute_error, relative_error = r.relative_error, initial_error = r.initial_error;
    outer_steps = (std::size_t)mr.outer_steps, inner_iterations = (std::size_t)mr.inner_iterations;
    fp64_iterations = (std::size_t)mr.fp64_iterations, finished_fp64 = mr.finished_fp64;
    return r.converged != 0;
  }
};
/// SolverBiCgStab.hpp:52-167.
template<class Vector>
class BiCgStabSolver final : public detail::DeviceIterativeSolver<Vector, STORM_HIP_BICGSTAB> {};
/// SolverCgs.hpp:50-176.
template<class Vector>
class CgsSolver final : public detail::DeviceIterativeSolver<Vector, STORM_HIP_CGS> {};
/// SolverTfqmr.hpp:227-240 / :252-265.
template<class Vector>
class TfqmrSolver final : public detail::DeviceIterativeSolver<Vector, STORM_HIP_TFQMR> {};
template<class Vector>
class Tfqmr1Solver final : public detail::DeviceIterativeSolver<Vector, STORM_HIP_TFQMR1> {};
/// SolverRichardson.hpp:41-98.
template<class Vector>
class RichardsonSolver final : public detail::DeviceIterativeSolver<Vector, STORM_HIP_RICHARDSON> {
public:
  real_t relaxation_factor{1.0e-4};

private:
  void configure(storm_hip_krylov* k) const override {
    detail::check(storm_hip_krylov_set_real(k, "relaxation_factor", relaxation_factor));
  }
};
/// SolverGmres.hpp:281-283 (default restart 50, Solver.hpp:159).  `gram_schmidt = 1`: classical Gram-Schmidt x2.
template<class Vector>
class GmresSolver final : public detail::DeviceInnerOuterSolver<Vector, STORM_HIP_GMRES, 50> {
public:
  int gram_schmidt{0};

private:
  void fill_params(storm_hip_solver_params& p) const override {
    p.num_inner_iterations = (int64_t)this->num_inner_iterations;
    p.gram_schmidt = gram_schmidt;
  }
};
/// SolverGmres.hpp:306-308: one preconditioned vector per inner iteration, so the preconditioner may vary.
template<class Vector>
class FgmresSolver final : public detail::DeviceInnerOuterSolver<Vector, STORM_HIP_FGMRES, 50> {};
/// SolverBiCgStab.hpp:184-383; `num_inner_iterations` is l (default 2, :379-381).
template<class Vector>
class BiCgStabLSolver final : public detail::DeviceInnerOuterSolver<Vector, STORM_HIP_BICGSTAB_L, 2> {};
/// SolverIdrs.hpp:52-291; `num_inner_iterations` is s (default 4, :287-289).
template<class Vector>
class IdrsSolver final : public detail::DeviceInnerOuterSolver<Vector, STORM_HIP_IDRS, 4> {};

/// SolverNewton.hpp:55-72: declared but unimplemented in the reference (STORM_ABORT); here the same
/// message arrives as an exception instead of std::abort().
template<class Vector>
class NewtonSolver : public IterativeSolver<Vector> {
  [[noreturn]] static void unimplemented() { throw std::runtime_error("Newton solver is not implemented yet!"); }
  real_t init(const Vector&, const Vector&, const Operator<Vector>&, const Preconditioner<Vector>*) override {
    unimplemented();
  }
  real_t iterate(Vector&, const Vector&, const Operator<Vector>&, const Preconditioner<Vector>*) override {
    unimplemented();
  }
};

/// SolverNewton.hpp:101-173: first-order Jacobian-free Newton-Krylov; `any_op` may be nonlinear.  A user-level
/// solver on the host loop: every Newton step solves J(x) t = r with a BiCgStabSolver at 1e-8 (:133-135) whose
/// operator is the finite-difference product (A(x + delta y) - A(x)) / delta, delta = mu / |y| (:136-148).
template<class Vector>
class JfnkSolver final : public IterativeSolver<Vector> {
public:
  std::size_t inner_iterations{0};

private:
  Vector _shifted, _step, _residual, _at_x;

  real_t residual_of(const Vector& x_vec, const Vector& b_vec, const Operator<Vector>& any_op) {
    any_op.mul(_at_x, x_vec);
    _residual <<= b_vec - _at_x;
    return norm_2(_residual);
  }
  real_t init(const Vector& x_vec, const Vector& b_vec, const Operator<Vector>& any_op,
              const Preconditioner<Vector>*) override {
    for (Vector* work : {&_shifted, &_step, &_residual, &_at_x}) work->assign(x_vec, false);
    inner_iterations = 0;
    return residual_of(x_vec, b_vec, any_op);
  }
  real_t iterate(Vector& x_vec, const Vector& b_vec, const Operator<Vector>& any_op,
                 const Preconditioner<Vector>*) override {
    const real_t mu = std::sqrt(std::numeric_limits<real_t>::epsilon()) * std::sqrt(1.0 + norm_2(x_vec));
    const auto jacobian = make_operator<Vector>([&](Vector& z_vec, const Vector& y_vec) {
      const real_t delta = safe_divide(mu, norm_2(y_vec));
      _shifted <<= x_vec + delta * y_vec;
      any_op.mul(z_vec, _shifted);
      z_vec <<= safe_divide(1.0, delta) * (z_vec - _at_x);
    });
    BiCgStabSolver<Vector> inner;
    inner.absolute_error_tolerance = inner.relative_error_tolerance = 1.0e-8;
    _step <<= _residual;
    inner.solve(_step, _residual, *jacobian);
    inner_iterations += inner.iteration;
    x_vec += _step;
    return residual_of(x_vec, b_vec, any_op);
  }
};

/// SolverNewton.hpp:101-173 inside the library (STORM_HIP_JFNK): the Newton loop is an engine method and every
/// Jacobian-vector product of the inner BiCGStab (1e-8, :133-135) the native finite-difference operator of
/// HipFdJacobianOperator -- no scalar visits the host inside a Newton step, where JfnkSolver waits for |y| at every
/// product.  `any_op` may be nonlinear (a lambda) or native; `pre_op` is ignored, as the reference ignores it (:107-109).
template<class Vector>
class HipJfnkSolver final : public detail::DeviceIterativeSolver<Vector, STORM_HIP_JFNK> {
public:
  std::size_t inner_iterations{0};  ///< inner BiCGStab iterations of the last solve

private:
  void collect(storm_hip_krylov* k) override {
    int64_t value = 0;
    detail::check(storm_hip_krylov_get_int(k, "inner_iterations", &value));
    inner_iterations = (std::size_t)value;
  }
};

#endif  // STORM_HIP_NO_SOLVERS

}  // namespace Storm
