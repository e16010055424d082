"""Preconditioned CG on the latency path (csrc/latency.hip, pcg_latency_kernel; option ``latency_pre``, counter
``latency_pre_solves``): CG with api.JacobiPreconditioner or api.ChebyshevPreconditioner as ONE cooperative kernel per
solve -- z = P r, p = z + beta p, gamma = <r, z>, the reported error norm_2(r) (SolverCg.hpp:54-126 with pre_op).

The plain latency kernel is forced with ``latency_path = 2`` (1 would hand lattice operators to the resident path,
which takes no preconditioner), ``latency_pre = 1`` switches the new kernel on; the fixture restores every option.

  1. Jacobi against the exact reference (tests/exact_ref.py, the pins of the engine's Jacobi CG: no new tolerance);
  2. the first direction is the library's own polynomial: x_1 = fl(alpha u_0), u_0 from storm_hip_cheb_apply;
  3. against the engine beyond the first steps, with the bounds tests/test_gpu_latency_path.py holds the unpreconditioned
     kernel to, and the engine's counts of applies;
  4. the edges of the stopping rule (Solver.hpp:116-147);
  5. reproducible bits;
  6. refusals run the engine; a refused launch and a give-up fall back (tests/test_gpu_fallbacks.py's hook)."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import exact_ref as er
from test_gpu_exact_engine_steps import _check
from test_gpu_exact_first_step import _matrix

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATHS = ("resident_solves", "latency_solves", "latency_pre_solves", "throughput_solves", "engine_solves", "cheb_fused_applies",
         "cheb_statement_applies")
RESTORE = (("latency_pre", 0), ("latency_path", 1), ("latency_rows", 1 << 19), ("latency_cache", 1), ("generic_solvers", 0),
           ("coop_force_fail", 0), ("spmv_dict", 4), ("ell_cap", 0), ("spmv_record_index", 1))


@pytest.fixture(scope="module")
def env():
    from oracle import oracle
    from stormruler_amd import api, mesh

    ctx = api.Context(0)
    yield api, mesh, oracle, ctx
    for k, v in RESTORE:
        ctx.set_option(k, v)
    _problems.clear()
    ctx.close()


@pytest.fixture(autouse=True)
def _restore(env):
    yield
    for k, v in RESTORE:
        env[3].set_option(k, v)


PRE = {
    "diag": lambda api: api.JacobiPreconditioner(),
    "cheb2": lambda api: api.ChebyshevPreconditioner(degree=2),
    "chebj4": lambda api: api.ChebyshevPreconditioner(degree=4, jacobi=True),
}


def _solve(api, ctx, op, b_host, pre, latency_pre, cls=None, x0=None, **knobs):
    """One solve with a fresh solver and the preconditioner ``pre`` (an object, or a key of PRE); which paths it moved."""
    ctx.set_option("latency_path", 2)
    ctx.set_option("latency_pre", latency_pre)
    s = (cls or api.CgSolver)()
    s.record_history = True
    s.pre_op = PRE[pre](api) if isinstance(pre, str) else pre
    for k, v in knobs.items():
        setattr(s, k, v)
    b_host = np.asarray(b_host, dtype=np.float64)
    b = api.DeviceVector.from_numpy(ctx, b_host)
    x = api.DeviceVector.from_numpy(ctx, np.zeros(b_host.size) if x0 is None else np.asarray(x0, dtype=np.float64))
    before = {k: ctx.counter(k) for k in PATHS}
    ok = s.solve(x, b, op)
    moved = {k: ctx.counter(k) - before[k] for k in PATHS}
    return ok, s, x.to_numpy(), moved


def _took_the_kernel(s, moved):
    assert s.path_fallback == 0
    assert moved == dict({k: 0 for k in PATHS}, latency_solves=1, latency_pre_solves=1), moved


def _took_the_engine(s, moved):
    assert s.path_fallback == 0
    assert moved["engine_solves"] == 1 and moved["latency_pre_solves"] == 0 and moved["latency_solves"] == 0, moved


def test_the_option_and_the_counter(env):
    api, mesh, oracle, ctx = env
    ctx.set_option("latency_pre", 1)
    assert ctx.counter("latency_pre_solves") == 0
    # 0 is the default: a fresh context sends a preconditioned solve to the engine
    other = api.Context(0)
    g = mesh.structured_box(6, 5, 4)
    mat = api.StencilMatrix.from_face_graph(other, g)
    s = api.CgSolver()
    s.pre_op = api.JacobiPreconditioner()
    b, x = api.DeviceVector.from_numpy(other, np.ones(g.n_cells)), api.DeviceVector(other, g.n_cells)
    assert s.solve(x, b, api.HipStencilOperator(mat, -1.0, 0.0))
    assert other.counter("latency_pre_solves") == 0 and other.counter("engine_solves") == 1
    mat.close()
    other.close()


# ---- 1. Jacobi against the exact reference ------------------------------------------------------------------------------

_problems = {}


def _step_problem(env, shape):
    if shape not in _problems:
        _problems[shape] = er.StepProblem(env[2], env[1], shape, "poisson")
    return _problems[shape]


@pytest.mark.parametrize("side", ["left", "right"])
@pytest.mark.parametrize("shape", [b[0] for b in er.ENGINE_STEP_BOXES], ids=lambda s: "x".join(map(str, s)))
def test_jacobi_steps_against_the_exact_reference(env, shape, side):
    """Three iterations, tolerances off, fp64 records: history, ||b - A x_3|| and (the small box) x_3 under the pins and caps
    of the engine's Jacobi CG -- CG takes no notice of the side."""
    api, mesh, oracle, ctx = env
    p = _step_problem(env, shape)
    pins = p.engine_pins("cg", None, side, er.ENGINE_JACOBI_K)
    mat = _matrix(api, ctx, p.g, "fp64")
    d = api.DeviceVector(ctx, p.b.size)
    mat.diagonal(-1.0, 0.0, d, invert=True)
    assert np.array_equal(d.to_numpy(), pins.dinv)  # the dinv the reference is restated with
    ok, s, x, moved = _solve(api, ctx, api.HipStencilOperator(mat, -1.0, 0.0), p.b, "diag", 1, num_iterations=er.ENGINE_JACOBI_K,
                             absolute_error_tolerance=0.0, relative_error_tolerance=0.0,
                             pre_side=api.PreconditionerSide.Left if side == "left" else api.PreconditionerSide.Right)
    _took_the_kernel(s, moved)
    assert not ok and s.num_applies == 4 and s.num_pre_applies == 4
    _check(pins, f"latency cg jacobi-{side} {'x'.join(map(str, shape))}", s, x)
    mat.close()


# ---- 2. the first direction is the library's own polynomial -------------------------------------------------------------

def _ulp(v):
    return np.spacing(np.abs(v))


@pytest.mark.parametrize("jacobi", [False, True], ids=["plain", "jacobi"])
@pytest.mark.parametrize("degree", [1, 2, 3, 8])
@pytest.mark.parametrize("shape", [(24, 24, 24), (37, 21, 19)], ids=lambda s: "x".join(map(str, s)))
def test_the_first_direction_is_the_polynomial_of_cheb_apply(env, shape, degree, jacobi):
    """x_0 = 0 and one iteration: x_1 = fl(alpha u_0), u_0 = P b by storm_hip_cheb_apply's launches on the solver's own
    object (24^3: 216 slices, gathers cross blocks; 37 x 21 x 19: ragged slices).  alpha from the row of largest |u_0|,
    in long double: the quotient is within 2^-53 of alpha (the rounding of x_1 there), so alpha_est u_0 lies within
    half an ulp + one ulp of x_1 wherever the kernel's u_0 has the launches' bits -- a missed publication, a wrong buffer or
    a restated rounding is an error of order one."""
    api, mesh, oracle, ctx = env
    g = mesh.structured_box(*shape)
    mat = _matrix(api, ctx, g, "fp64")
    b_host = 1.0 + 0.25 * np.sin(0.01 * np.arange(g.n_cells))
    pre = api.ChebyshevPreconditioner(degree=degree, jacobi=jacobi)
    ok, s, x1, moved = _solve(api, ctx, api.HipStencilOperator(mat, -1.0, 0.0), b_host, pre, 1, num_iterations=1,
                              absolute_error_tolerance=0.0, relative_error_tolerance=0.0)
    _took_the_kernel(s, moved)
    assert s.iteration == 1 and s.num_pre_applies == 2
    b, u = api.DeviceVector.from_numpy(ctx, b_host), api.DeviceVector(ctx, g.n_cells)
    fused = ctx.counter("cheb_fused_applies")
    pre.mul(u, b)
    assert ctx.counter("cheb_fused_applies") == fused + 1
    u0 = u.to_numpy()
    i = int(np.argmax(np.abs(u0)))
    alpha = np.longdouble(x1[i]) / np.longdouble(u0[i])
    far = np.abs(x1.astype(np.longdouble) - alpha * u0.astype(np.longdouble)) / _ulp(x1)
    print(f"first direction {shape} degree {degree} jacobi {jacobi}: alpha {float(alpha):.6e}, worst {float(far.max()):.2f} ulp")
    assert np.all(np.isfinite(x1)) and x1.any() and float(far.max()) <= 2.0, float(far.max())
    pre.close()
    mat.close()


# ---- 3. against the engine, beyond the first steps ------------------------------------------------------------------------

def _csr_operator(api, ctx):
    """Rows longer than the eight slots of the register cache and a ragged last slice (4099 rows, ~40 per row), built as
    test_rows_longer_than_the_register_cache_and_ragged_sizes builds it."""
    rng = np.random.default_rng(5)
    n, per_row = 4099, 20
    rows = np.repeat(np.arange(n), per_row)
    a = sp.coo_matrix((rng.random(rows.size) * 0.1, (rows, rng.integers(0, n, rows.size))), shape=(n, n)).tocsr()
    a = a + a.T
    a.setdiag(0.0)
    a.eliminate_zeros()
    a = (sp.diags(np.asarray(abs(a).sum(axis=1)).ravel() + 1.0) - a).tocsr()  # SPD, diagonally dominant
    mat = api.StencilMatrix.from_csr(ctx, a)
    assert mat.stats()["tail_rows"] == 0
    return mat, 1.0, 0.0, rng.random(n) + 0.5


def _step1_operator(api, mesh, ctx):
    from stormruler_amd import io_tetgen

    g = io_tetgen.read_triangle(os.path.join(ROOT, "tests", "golden", "mesh", "step.1."))
    g = mesh.FaceGraph(g.n_cells, 2, g.inner, g.outer, g.area, g.center, g.volume, b_center=np.zeros((0, 2)))
    return api.StencilMatrix.from_face_graph(ctx, g), -1.0e-2, 1.0, np.sin(3 * g.center[:, 0]) * np.cos(7 * g.center[:, 1])


def _box_operator(api, mesh, ctx, shape):
    g = mesh.structured_box(*shape)
    return api.StencilMatrix.from_face_graph(ctx, g), -1.0, 0.0, 1.0 + 0.25 * np.sin(0.01 * np.arange(g.n_cells))


# 64^3: one slice per wavefront of 256 blocks; 80^3: two (the largest variant the kernel is built in: csrc/latency.hip)
ENGINE_CASES = [(5, 3, 2), (9, 7, 1), (24, 24, 24), (64, 64, 64), (80, 80, 80), "csr", "step.1"]
# Cases whose run to the tolerance is a fixed count instead (NOTES.md has the figures): the two roads part there by the
# roundings of their sums alone, and the bounds are not widened for it.
#   80^3 with the diagonal: 160 iterations to 1e-6; the histories are 7e-12 apart at iteration 40, 1.3e-10 at 50, 1.7e-9 at
#   75 and 1.0e-8 at the end, while the two x agree to 9e-16 -- late iterations of an ill-conditioned case.
#   step.1 with the scale (the diagonal, Chebyshev-Jacobi): the mesh operator is not symmetric in the Euclidean product once
#   its rows are scaled, preconditioned CG DIVERGES on it on the engine and in the kernel alike (|r| 8.7e6 after 3 iterations
#   with the diagonal, 1.7e4 with Chebyshev-Jacobi, 2000 iterations without meeting 1e-6) and amplifies every rounding on
#   the way: 8.7e-14 apart at iteration 3 and 8e-8 at 10 with the diagonal; 3e-11 at 40 and 7e-9 at 75 with Chebyshev-Jacobi.
FIXED_COUNT = {((80, 80, 80), "diag"): 40, ("step.1", "diag"): 3, ("step.1", "chebj4"): 40}


@pytest.mark.parametrize("pre", list(PRE))
@pytest.mark.parametrize("case", ENGINE_CASES, ids=lambda c: c if isinstance(c, str) else "x".join(map(str, c)))
def test_against_the_engine(env, case, pre):
    """The same solve with latency_pre 1 and 0: to the default tolerances (1e-6; FIXED_COUNT: for that many iterations)
    and for three iterations."""
    api, mesh, oracle, ctx = env
    mat, alpha, beta, b_host = (_csr_operator(api, ctx) if case == "csr" else _step1_operator(api, mesh, ctx) if case == "step.1"
                                else _box_operator(api, mesh, ctx, case))
    op = api.HipStencilOperator(mat, alpha, beta)
    long_run = ("tolerance", {}) if (case, pre) not in FIXED_COUNT else \
        ("fixed", dict(num_iterations=FIXED_COUNT[case, pre], absolute_error_tolerance=0.0, relative_error_tolerance=0.0))
    for label, knobs in (long_run, ("count", dict(num_iterations=3, absolute_error_tolerance=0.0, relative_error_tolerance=0.0))):
        ok_l, s_l, x_l, moved_l = _solve(api, ctx, op, b_host, pre, 1, **knobs)
        ok_e, s_e, x_e, moved_e = _solve(api, ctx, op, b_host, pre, 0, **knobs)
        _took_the_kernel(s_l, moved_l)
        _took_the_engine(s_e, moved_e)
        m = min(len(s_l.history), len(s_e.history))
        far_h = float(np.max(np.abs(s_l.history[:m] / s_e.history[:m] - 1.0)))
        far_x = float(np.linalg.norm(x_l - x_e) / np.linalg.norm(x_e))
        print(f"engine {case} {pre} {label}: iterations {s_l.iteration} / {s_e.iteration}, history {far_h:.2e}, x {far_x:.2e}")
        assert ok_l == ok_e == (label == "tolerance")
        assert abs(s_l.iteration - s_e.iteration) <= 1
        assert np.allclose(s_l.history[:m], s_e.history[:m], rtol=1e-9)
        assert far_x <= 1e-9
        if s_l.iteration == s_e.iteration:
            assert s_l.num_applies == s_e.num_applies and s_l.num_pre_applies == s_e.num_pre_applies
        assert s_l.num_applies == s_l.iteration + 1 and s_l.num_pre_applies == s_l.iteration + 1
        assert s_e.num_applies == s_e.iteration + 1 and s_e.num_pre_applies == s_e.iteration + 1
        for a, b in (("initial_error", 1e-12), ("absolute_error", 1e-6), ("relative_error", 1e-6)):
            if s_l.iteration == s_e.iteration:
                assert np.isclose(getattr(s_l, a), getattr(s_e, a), rtol=b, atol=0.0), a
    mat.close()


# ---- 4. the edges of the rule ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pre", list(PRE))
def test_convergence_rule_edges(env, pre):
    """The cases of test_convergence_rule_edges_on_the_latency_path, preconditioned."""
    api, mesh, oracle, ctx = env
    g = mesh.structured_box(10)
    mat = api.StencilMatrix.from_face_graph(ctx, g)
    op = api.HipStencilOperator(mat, -1.0, 0.0)
    b_host = np.ones(g.n_cells)
    x0 = 0.01 * np.cos(0.3 * np.arange(g.n_cells))
    # tolerances off: exactly num_iterations iterations, converged == False
    ok, s, _, moved = _solve(api, ctx, op, b_host, pre, 1, num_iterations=17, relative_error_tolerance=0.0,
                             absolute_error_tolerance=0.0)
    _took_the_kernel(s, moved)
    assert not ok and s.iteration == 17 and len(s.history) == 18 and s.num_applies == 18 and s.num_pre_applies == 18
    # the initial residual already meets the absolute tolerance: no iteration, converged, x untouched (Solver.hpp:124-128)
    ok, s, x, moved = _solve(api, ctx, op, b_host, pre, 1, x0=x0, absolute_error_tolerance=1e9)
    _, s_e, _, _ = _solve(api, ctx, op, b_host, pre, 0, x0=x0, absolute_error_tolerance=1e9)
    _took_the_kernel(s, moved)
    assert ok and s.iteration == 0 and np.array_equal(x, x0) and len(s.history) == 1
    assert (s.num_applies, s.num_pre_applies, s.relative_error) == (s_e.num_applies, s_e.num_pre_applies, s_e.relative_error)
    assert np.isclose(s.initial_error, s_e.initial_error, rtol=1e-12) and s.absolute_error == s.initial_error
    # num_iterations = 0
    ok, s, x, moved = _solve(api, ctx, op, b_host, pre, 1, x0=x0, num_iterations=0)
    _, s_e, _, _ = _solve(api, ctx, op, b_host, pre, 0, x0=x0, num_iterations=0)
    _took_the_kernel(s, moved)
    assert not ok and s.iteration == 0 and np.array_equal(x, x0)
    assert (s.num_applies, s.num_pre_applies) == (s_e.num_applies, s_e.num_pre_applies)
    # a stop by the relative tolerance alone
    ok, s, x, moved = _solve(api, ctx, op, b_host, pre, 1, relative_error_tolerance=1e-3, absolute_error_tolerance=0.0)
    ok_e, s_e, x_e, _ = _solve(api, ctx, op, b_host, pre, 0, relative_error_tolerance=1e-3, absolute_error_tolerance=0.0)
    _took_the_kernel(s, moved)
    assert ok and ok_e and s.iteration == s_e.iteration and s.relative_error < 1e-3 <= s.history[-2] / s.history[0]
    assert s.history[-1] / s.history[0] == s.relative_error and s.absolute_error == s.history[-1]
    assert np.linalg.norm(x - x_e) <= 1e-9 * np.linalg.norm(x_e)
    # zero right-hand side: safe_divide keeps everything finite (Crow/MathUtils.hpp:49-52)
    ok, s, x, moved = _solve(api, ctx, op, np.zeros(g.n_cells), pre, 1)
    _took_the_kernel(s, moved)
    assert np.all(np.isfinite(x)) and not x.any() and np.all(np.isfinite(s.history))
    ok, s, x, moved = _solve(api, ctx, op, np.zeros(g.n_cells), pre, 1, num_iterations=3, relative_error_tolerance=0.0,
                             absolute_error_tolerance=0.0)
    _took_the_kernel(s, moved)
    assert s.iteration == 3 and np.all(np.isfinite(x)) and not x.any() and np.all(np.isfinite(s.history))
    # a warm start is honoured
    ref = oracle.solve("cg", oracle.StencilOperator(g, -1.0, 0.0), b_host)
    ok, s, x, moved = _solve(api, ctx, op, b_host, pre, 1, x0=ref.x)
    _took_the_kernel(s, moved)
    assert s.initial_error <= 2e-6 * np.linalg.norm(b_host)  # started from the solution, not from zero
    mat.close()


def test_a_one_row_operator(env):
    api, mesh, oracle, ctx = env
    mat = api.StencilMatrix.from_csr(ctx, sp.csr_matrix(np.array([[2.0]])))
    for pre in PRE:
        ok, s, x, moved = _solve(api, ctx, api.HipStencilOperator(mat, 1.0, 0.0), np.array([3.0]), pre, 1)
        _took_the_kernel(s, moved)
        assert ok and abs(x[0] - 1.5) <= 1e-12
    mat.close()


# ---- 5. reproducible bits ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pre", list(PRE))
@pytest.mark.parametrize("shape", [(64, 64, 64), (80, 80, 80)], ids=lambda s: "x".join(map(str, s)))
def test_the_bits_are_reproducible(env, shape, pre):
    """Rows published by one block are gathered by others behind a synchronisation point only: a row that a gathering wave
    saw too early, or a buffer rewritten too soon, would show as a run-to-run difference.  200 iterations (400 .. 1 200
    points), tolerances off, twice."""
    api, mesh, oracle, ctx = env
    mat, alpha, beta, b_host = _box_operator(api, mesh, ctx, shape)
    runs = []
    for _ in range(2):
        ok, s, x, moved = _solve(api, ctx, api.HipStencilOperator(mat, alpha, beta), b_host, pre, 1, num_iterations=200,
                                 relative_error_tolerance=0.0, absolute_error_tolerance=0.0)
        _took_the_kernel(s, moved)
        runs.append((np.array(s.history), x))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    mat.close()


# ---- 6. refusals fall through, failures fall back ---------------------------------------------------------------------------------

def _refusals(api, mesh, ctx, mat, twin):
    class OnAnotherOperator(api.ChebyshevPreconditioner):
        def __init__(self, other, **kw):
            super().__init__(**kw)
            self._other = other

        def build(self, x_vec, b_vec, any_op):
            super().build(x_vec, b_vec, self._other)

    class CallbackJacobi(api.Preconditioner):
        """A preconditioner the library knows only as a callback."""

        def __init__(self):
            self._inner = api.JacobiPreconditioner()

        def build(self, x_vec, b_vec, any_op):
            self._inner.build(x_vec, b_vec, any_op)

        def mul(self, y_vec, x_vec):
            self._inner.mul(y_vec, x_vec)

        def conj_mul(self, x_vec, y_vec):
            self._inner.conj_mul(x_vec, y_vec)

    return {
        "cheb on another matrix": (api.CgSolver, {}, lambda: OnAnotherOperator(api.HipStencilOperator(twin, -1.0, 0.0), degree=2)),
        "cheb with another alpha": (api.CgSolver, {}, lambda: OnAnotherOperator(api.HipStencilOperator(mat, -2.0, 0.0), degree=2)),
        "cheb with another beta": (api.CgSolver, {}, lambda: OnAnotherOperator(api.HipStencilOperator(mat, -1.0, 0.5), degree=2)),
        "reduced cheb": (api.CgSolver, {}, lambda: api.ChebyshevPreconditioner(degree=2, reduced_records=True)),
        "amg": (api.CgSolver, {}, lambda: api.AmgPreconditioner()),
        "callback": (api.CgSolver, {}, lambda: CallbackJacobi()),
        "generic_solvers": (api.CgSolver, {"generic_solvers": 1}, lambda: api.JacobiPreconditioner()),
        "bicgstab": (api.BiCgStabSolver, {}, lambda: api.JacobiPreconditioner()),
    }


REFUSALS = ["cheb on another matrix", "cheb with another alpha", "cheb with another beta", "reduced cheb", "amg", "callback",
            "generic_solvers", "bicgstab"]


@pytest.mark.parametrize("name", REFUSALS)
def test_refusals_run_the_engine(env, name):
    """latency_pre 1 and a solve outside the rule: the engine takes it and gives what it gives with latency_pre 0, to the bit."""
    api, mesh, oracle, ctx = env
    g = mesh.structured_box(20, 18, 16)
    mat, twin = _matrix(api, ctx, g, "fp64"), _matrix(api, ctx, g, "fp64")  # (fp64 records: a reduced object needs them)
    cls, opts, make = _refusals(api, mesh, ctx, mat, twin)[name]
    b_host = 1.0 + 0.25 * np.sin(0.01 * np.arange(g.n_cells))
    runs = []
    for latency_pre in (1, 0):
        for k, v in opts.items():
            ctx.set_option(k, v)
        pre = make()
        ok, s, x, moved = _solve(api, ctx, api.HipStencilOperator(mat, -1.0, 0.0), b_host, pre, latency_pre, cls=cls)
        _took_the_engine(s, moved)
        assert ok
        runs.append((s.iteration, np.array(s.history), x, s.num_applies, s.num_pre_applies))
        if hasattr(pre, "close"):
            pre.close()
    assert runs[0][0] == runs[1][0] and runs[0][3:] == runs[1][3:]
    assert np.array_equal(runs[0][1], runs[1][1]) and np.array_equal(runs[0][2], runs[1][2])
    mat.close()
    twin.close()


def test_a_two_stage_operator_and_the_resident_path_stay_where_they_are(env):
    """No preconditioner: the two-stage CG and (latency_path 1) the resident path are not the new kernel's business."""
    api, mesh, oracle, ctx = env
    g = mesh.structured_box(64, 48, 40)
    mat = api.StencilMatrix.from_face_graph(ctx, g)
    b_host = np.ones(g.n_cells)
    ctx.set_option("latency_pre", 1)
    b, x = api.DeviceVector.from_numpy(ctx, b_host), api.DeviceVector(ctx, g.n_cells)
    before = ctx.counter("resident_solves")
    assert api.CgSolver().solve(x, b, api.HipStencilOperator(mat, -1.0, 0.0)) and ctx.counter("resident_solves") == before + 1
    before = {k: ctx.counter(k) for k in PATHS}
    s = api.CgSolver()
    x = api.DeviceVector(ctx, g.n_cells)
    assert s.solve(x, b, api.HipTwoStageOperator(mat, -1.0e-2, 1.0, -1.0e-2, 1.0))
    s = api.CgSolver()
    s.pre_op = api.JacobiPreconditioner()  # latency_path 1: the operator is the resident path's, the solve the engine's
    x = api.DeviceVector(ctx, g.n_cells)
    assert s.solve(x, b, api.HipStencilOperator(mat, -1.0, 0.0))
    moved = {k: ctx.counter(k) - before[k] for k in PATHS}
    assert moved["latency_pre_solves"] == 0 and moved["latency_solves"] == 1 and moved["engine_solves"] == 1, moved
    mat.close()


@pytest.mark.parametrize("pre", list(PRE))
@pytest.mark.parametrize("how", [1, 2])
def test_a_failed_launch_or_a_give_up_falls_back_and_says_so(env, how, pre):
    """Option coop_force_fail (tests/test_gpu_fallbacks.py): 1 the launch is refused, 2 the kernel "gave up" -- x is restored
    and the engine runs the solve; path_fallback says which."""
    api, mesh, oracle, ctx = env
    g = mesh.structured_box(24, 20, 16)
    mat = api.StencilMatrix.from_face_graph(ctx, g)
    op = api.HipStencilOperator(mat, -1.0, 0.0)
    b_host = np.ones(g.n_cells)
    x0 = 0.01 * np.cos(0.3 * np.arange(g.n_cells))  # a start that a botched restore of x would show
    ok0, s0, xa, moved0 = _solve(api, ctx, op, b_host, pre, 1, x0=x0)
    _took_the_kernel(s0, moved0)
    ok_e, s_e, x_e, _ = _solve(api, ctx, op, b_host, pre, 0, x0=x0)
    ctx.set_option("coop_force_fail", how)
    ok1, s1, xb, moved1 = _solve(api, ctx, op, b_host, pre, 1, x0=x0)
    ctx.set_option("coop_force_fail", 0)
    assert ok0 and ok1 and s1.path_fallback == how, (s1.path_fallback, how)
    assert moved1["engine_solves"] == 1 and moved1["latency_pre_solves"] == (1 if how == 2 else 0), moved1
    # the engine's own result, to the bit
    assert s1.iteration == s_e.iteration and np.array_equal(xb, x_e) and np.array_equal(s1.history, s_e.history)
    assert (s1.num_applies, s1.num_pre_applies) == (s_e.num_applies, s_e.num_pre_applies)
    assert abs(s1.iteration - s0.iteration) <= 1 and np.linalg.norm(xa - xb) <= 1e-9 * np.linalg.norm(xa)
    mat.close()


def test_no_register_variant_runs_the_engine(env):
    """latency_rows raised: 100^3 needs four slices per wavefront, the kernel is built for two at most -- the engine takes
    the solve and path_fallback says 1, as the unpreconditioned kernel does beyond its eight."""
    api, mesh, oracle, ctx = env
    g = mesh.structured_box(100, 100, 100)
    ctx.set_option("latency_rows", 1 << 21)
    mat = api.StencilMatrix.from_face_graph(ctx, g)
    ctx.set_option("latency_rows", 1 << 19)
    ok, s, x, moved = _solve(api, ctx, api.HipStencilOperator(mat, -1.0, 0.0), np.ones(g.n_cells), "diag", 1, num_iterations=5)
    assert s.iteration == 5 and s.path_fallback == 1 and moved["engine_solves"] == 1 and moved["latency_pre_solves"] == 0
    mat.close()
