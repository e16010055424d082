"""The two-stage operator A = beta2 I + alpha2 M (beta1 I + alpha1 M) -- the linear part of the playground's Cahn-Hilliard
lambda (Playground.cpp:153-167: two stormDivGrad calls per apply) -- as a native operator at every layer:

  * `storm_hip_op_apply2`: bit for bit the three-call composition of today's entry points, in every record format;
  * `storm_hip_solve_cg2`: CG as ONE cooperative kernel per solve (csrc/latency.hip, cg2_latency_kernel: three
    synchronisation points per iteration) against the engine's loop and the oracle, for every register variant, ragged
    and long rows, degenerate constants, the edges of the convergence rule, run-to-run bits and the forced fallbacks;
  * `storm_hip_krylov_set_operator2`: the other methods on the same operator without a callback;
  * tests/cpp/two_stage_driver: the playground's time loop with the one operator object.

The reference is always the oracle's solver over a Python callback that applies the oracle's one-stage operator twice."""
import json
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAYGROUND = (-1.0e-4, 2.0, -1.0e-3, 1.0)  # alpha1 = -Gamma, beta1 = sigma, alpha2 = -tau, beta2 = 1   (Playground.cpp:113)
OTHER = (-0.05, 1.0, -0.5, 0.75)
FORMATS = [(0, 1), (1, 1), (1, 2), (2, 1), (2, 2), (2, 4), (3, 0), (4, 0), (5, 0)]  # (spmv_dict, spmv_spw), as test_gpu_formats.py
INVALID, UNSUPPORTED = -1, -6


@pytest.fixture(scope="module")
def env():
    from oracle import oracle
    from stormruler_amd import api, mesh

    ctx = api.Context(0)
    yield api, mesh, oracle, ctx
    for key, value in (("latency_path", 1), ("latency_rows", 1 << 19), ("coop_force_fail", 0), ("spmv_dict", 4), ("spmv_spw", 0)):
        ctx.set_option(key, value)
    ctx.close()


def _triangle_mesh(name):
    from stormruler_amd import io_tetgen, mesh

    g = io_tetgen.read_triangle(os.path.join(ROOT, "tests", "golden", "mesh", name + "."))
    return mesh.FaceGraph(g.n_cells, 2, g.inner, g.outer, g.area, g.center, g.volume, b_center=np.zeros((0, 2)))  # `interior_faces()` only


def _two_stage_fn(apply_m, consts):
    a1, b1, a2, b2 = consts
    return lambda x: b2 * x + a2 * apply_m(b1 * x + a1 * apply_m(x))


def _oracle_op(oracle, g, consts):
    m = oracle.StencilOperator(g, 1.0, 0.0)
    return oracle.CallbackOperator(g.n_cells, _two_stage_fn(m.apply, consts))


def _status(api, fn):
    with pytest.raises(api._lib.StormHipError) as e:
        fn()
    return e.value.status, str(e.value)


def _cg2(api, ctx, op, b_host, latency, x0=None, **knobs):
    """`solve<CgSolver>(x, b, two_stage)`: the solver binds the operator natively and CG forwards to storm_hip_solve_cg2."""
    ctx.set_option("latency_path", 2 if latency else 0)
    s = api.CgSolver()
    s.record_history = True
    for k, v in knobs.items():
        setattr(s, k, v)
    b = api.DeviceVector.from_numpy(ctx, b_host)
    x = api.DeviceVector(ctx, b_host.size) if x0 is None else api.DeviceVector.from_numpy(ctx, x0)
    before = (ctx.counter("latency_solves"), ctx.counter("engine_solves"))
    ok = s.solve(x, b, op)
    s.took = (ctx.counter("latency_solves") - before[0], ctx.counter("engine_solves") - before[1])
    ctx.set_option("latency_path", 1)
    return ok, s, x.to_numpy()


# ---- apply ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("problem", [(5, 3, 2), (9, 7, 1), (24, 24, 24), "square_nb.1"])
def test_apply2_is_the_three_call_composition_bit_for_bit_in_every_format(env, problem):
    api, mesh, oracle, ctx = env
    g = _triangle_mesh(problem) if isinstance(problem, str) else mesh.structured_box(*problem)
    n = g.n_cells
    x_host = np.sin(0.37 * np.arange(n)) + 0.1
    ref_m = oracle.StencilOperator(g, 1.0, 0.0)
    ys = {}
    for fmt in FORMATS:
        ctx.set_option("spmv_dict", fmt[0])
        ctx.set_option("spmv_spw", fmt[1])
        mat = api.StencilMatrix.from_face_graph(ctx, g)
        ctx.set_option("spmv_dict", 4)
        ctx.set_option("spmv_spw", 0)
        x = api.DeviceVector.from_numpy(ctx, x_host)
        for consts in (PLAYGROUND, OTHER):
            a1, b1, a2, b2 = consts
            # today's calls
            t_ref, y_ref = api.DeviceVector(ctx, n), api.DeviceVector(ctx, n)
            mat.apply(a1, b1, x, t_ref)
            y_ref <<= x
            y_ref *= b2
            mat.apply_add(a2, t_ref, y_ref)
            # the new entry point, with the caller's t and with the pooled one
            t, y, y_null = api.DeviceVector(ctx, n), api.DeviceVector(ctx, n), api.DeviceVector(ctx, n)
            api.HipTwoStageOperator(mat, a1, b1, a2, b2, intermediate=t).mul(y, x)
            api.HipTwoStageOperator(mat, a1, b1, a2, b2).mul(y_null, x)
            assert np.array_equal(y.to_numpy(), y_ref.to_numpy()), (fmt, consts)
            assert np.array_equal(t.to_numpy(), t_ref.to_numpy()), (fmt, consts)
            assert np.array_equal(y_null.to_numpy(), y_ref.to_numpy()), (fmt, consts)
            want = _two_stage_fn(ref_m.apply, consts)(x_host)
            assert np.abs(y.to_numpy() - want).max() <= 1e-13 * np.abs(want).max(), (fmt, consts)
            ys[(fmt, consts)] = y.to_numpy()
        mat.close()
    for fmt in FORMATS[1:]:
        for consts in (PLAYGROUND, OTHER):
            assert np.array_equal(ys[(fmt, consts)], ys[(FORMATS[0], consts)]), (fmt, consts)


def test_apply2_and_its_solvers_refuse_what_they_do_not_support(env):
    api, mesh, oracle, ctx = env
    lib, C = api._lib.lib, api.C
    g = mesh.structured_box(8)
    n = g.n_cells
    mat = api.StencilMatrix.from_face_graph(ctx, g)
    x, t, y = (api.DeviceVector(ctx, n) for _ in range(3))
    short = api.DeviceVector(ctx, n - 1)

    def apply2(xv, tv, yv, m=mat):
        return lambda: api._lib.check(lib.storm_hip_op_apply2(m._h, *PLAYGROUND, xv._h, None if tv is None else tv._h, yv._h))

    for call in (apply2(x, t, x), apply2(x, x, y), apply2(x, y, y), apply2(x, None, x),     # aliasing
                 apply2(short, t, y), apply2(x, short, y), apply2(x, t, short)):              # sizes
        assert _status(api, call)[0] == INVALID
    apply2(x, t, y)()  # ... and the well-formed call goes through
    # an operator with a halo plan
    loc, send_idx = mesh.periodic_z_local_graph(8, 8, 8)
    halo = api.StencilMatrix.from_face_graph(ctx, loc)
    halo.set_halo([0], [0, loc.n_halo], send_idx, [0, loc.n_halo])
    xh, yh = api.DeviceVector(ctx, loc.n_cells, loc.n_halo), api.DeviceVector(ctx, loc.n_cells, loc.n_halo)
    status, what = _status(api, apply2(xh, None, yh, halo))
    assert status == UNSUPPORTED and "halo" in what, what
    p, r = api._lib.SolverParams(), api._lib.SolverResult()
    lib.storm_hip_solver_params_default(C.byref(p))
    assert lib.storm_hip_solve_cg2(halo._h, *PLAYGROUND, xh._h, yh._h, C.byref(p), C.byref(r), None) == UNSUPPORTED
    status, what = _status(api, lambda: api.CgSolver().solve(yh, xh, api.HipTwoStageOperator(halo, *PLAYGROUND)))
    assert status == UNSUPPORTED and "halo" in what, what
    halo.close()
    # a context with a communicator
    c2 = api.Context(0)
    c2.comm_init(api.Context.comm_unique_id(), 1, 0)
    m2 = api.StencilMatrix.from_face_graph(c2, g)
    x2, y2 = api.DeviceVector(c2, n), api.DeviceVector(c2, n)
    assert _status(api, apply2(x2, None, y2, m2))[0] == UNSUPPORTED
    assert lib.storm_hip_solve_cg2(m2._h, *PLAYGROUND, x2._h, y2._h, C.byref(p), C.byref(r), None) == UNSUPPORTED
    assert _status(api, lambda: api.BiCgStabSolver().solve(y2, x2, api.HipTwoStageOperator(m2, *PLAYGROUND)))[0] == UNSUPPORTED
    m2.close()
    c2.close()
    # the diagonal of a two-stage operator is not available: a clear error, not a wrong preconditioner
    with pytest.raises(TypeError, match="HipTwoStageOperator"):
        api.JacobiPreconditioner().build(x, x, api.HipTwoStageOperator(mat, *PLAYGROUND))
    with pytest.raises(RuntimeError, match="conj_mul"):
        api.HipTwoStageOperator(mat, *PLAYGROUND).conj_mul(x, y)
    mat.close()


# ---- the latency kernel against the engine path and the oracle ------------------------------------------------------------
# rows: 64^3 fills 256 blocks x 16 waves with one slice each; the larger boxes need 2 / 4 / 8 slices per wavefront
@pytest.mark.parametrize("shape", [(5, 3, 2), (9, 7, 1), (24, 24, 24), (64, 64, 64), (80, 80, 80), (100, 100, 100),
                                   (128, 128, 100)])
def test_box_matches_engine_path_and_oracle(env, shape):
    api, mesh, oracle, ctx = env
    g = mesh.structured_box(*shape)
    ctx.set_option("latency_rows", 1 << 21)
    mat = api.StencilMatrix.from_face_graph(ctx, g)
    ctx.set_option("latency_rows", 1 << 19)
    op = api.HipTwoStageOperator(mat, *PLAYGROUND)
    b_host = 1.0 + 0.25 * np.sin(0.01 * np.arange(g.n_cells))
    ok_l, s_l, x_l = _cg2(api, ctx, op, b_host, True)
    ok_e, s_e, x_e = _cg2(api, ctx, op, b_host, False)
    print(f"{shape}: latency {s_l.iteration} iterations, engine {s_e.iteration}")
    assert ok_l and ok_e
    assert s_l.path_fallback == 0 and s_l.took == (1, 0) and s_e.took == (0, 1)
    assert abs(s_l.iteration - s_e.iteration) <= 1 and s_l.num_applies == s_l.iteration + 1
    m = min(len(s_l.history), len(s_e.history))
    assert np.allclose(s_l.history[:m], s_e.history[:m], rtol=1e-9)
    assert np.linalg.norm(x_l - x_e) <= 1e-9 * np.linalg.norm(x_e)
    if g.n_cells <= 64 ** 3:
        ref = oracle.solve("cg", _oracle_op(oracle, g, PLAYGROUND), b_host)
        assert abs(s_l.iteration - ref.iterations) <= max(2, int(0.02 * ref.iterations)), (s_l.iteration, ref.iterations)
        assert np.linalg.norm(x_l - ref.x) <= 1e-8 * np.linalg.norm(ref.x)
    mat.close()


@pytest.mark.parametrize("shape", [(5, 3, 2), (9, 7, 1)])
def test_box_with_the_second_constant_set(env, shape):
    """(-0.05, 1, -0.5, 1) on the two smallest boxes (17 and 45 iterations on the oracle): a second stage that dominates."""
    api, mesh, oracle, ctx = env
    consts = (-0.05, 1.0, -0.5, 1.0)
    g = mesh.structured_box(*shape)
    mat = api.StencilMatrix.from_face_graph(ctx, g)
    b_host = 1.0 + 0.25 * np.sin(0.01 * np.arange(g.n_cells))
    ok_l, s_l, x_l = _cg2(api, ctx, api.HipTwoStageOperator(mat, *consts), b_host, True)
    ref = oracle.solve("cg", _oracle_op(oracle, g, consts), b_host)
    assert ok_l and ref.converged and s_l.took == (1, 0)
    assert abs(s_l.iteration - ref.iterations) <= max(2, int(0.02 * ref.iterations)), (s_l.iteration, ref.iterations)
    assert np.linalg.norm(x_l - ref.x) <= 1e-8 * np.linalg.norm(ref.x)
    mat.close()


@pytest.mark.parametrize("name", ["square_nb.1", "rectangle.1"])
def test_triangle_meshes_against_the_oracle_and_the_true_residual(env, name):
    """The reference's own meshes: three neighbours per row (records in registers, four slots)."""
    api, mesh, oracle, ctx = env
    g = _triangle_mesh(name)
    mat = api.StencilMatrix.from_face_graph(ctx, g)
    b_host = np.sin(3 * g.center[:, 0]) * np.cos(7 * g.center[:, 1])
    ok, s, x = _cg2(api, ctx, api.HipTwoStageOperator(mat, *PLAYGROUND), b_host, True)
    assert ok and s.took == (1, 0) and s.path_fallback == 0
    ref = oracle.solve("cg", _oracle_op(oracle, g, PLAYGROUND), b_host)
    print(f"{name}: {s.iteration} iterations (oracle {ref.iterations})")
    assert abs(s.iteration - ref.iterations) <= max(2, int(0.02 * ref.iterations)), (s.iteration, ref.iterations)
    assert np.linalg.norm(x - ref.x) <= 1e-8 * np.linalg.norm(ref.x)
    a1, b1, a2, b2 = PLAYGROUND
    m = mesh.assemble_csr(g, 1.0, 0.0)
    eye = sp.identity(g.n_cells, format="csr")
    a = b2 * eye + a2 * (m @ (b1 * eye + a1 * m))
    assert np.linalg.norm(b_host - a @ x) <= 2e-6 * np.linalg.norm(b_host)
    mat.close()


def _random_spd_csr(rng, n, per_row):
    if not per_row:
        return sp.csr_matrix(np.array([[2.0]]))
    rows = np.repeat(np.arange(n), per_row)
    cols = rng.integers(0, n, rows.size)
    a = sp.coo_matrix((rng.random(rows.size) * 0.1, (rows, cols)), shape=(n, n)).tocsr()
    a = a + a.T
    a.setdiag(0.0)
    a.eliminate_zeros()
    return (sp.diags(np.asarray(abs(a).sum(axis=1)).ravel() + 1.0) - a).tocsr()  # SPD, diagonally dominant


def test_rows_longer_than_the_register_cache_and_ragged_sizes(env):
    api, mesh, oracle, ctx = env
    rng = np.random.default_rng(5)
    consts = (-0.01, 1.0, -0.01, 1.0)  # A = I - 0.01 M (I - 0.01 M): SPD because M is symmetric
    for n, per_row in ((1, 0), (63, 2), (65, 3), (1000, 12), (4099, 20)):
        m = _random_spd_csr(rng, n, per_row)
        mat = api.StencilMatrix.from_csr(ctx, m)
        assert mat.stats()["tail_rows"] == 0
        b_host = rng.random(n) + 0.5
        op = api.HipTwoStageOperator(mat, *consts)
        knobs = dict(relative_error_tolerance=1e-10, absolute_error_tolerance=0.0)
        ok_l, s_l, x_l = _cg2(api, ctx, op, b_host, True, **knobs)
        ok_e, s_e, x_e = _cg2(api, ctx, op, b_host, False, **knobs)
        assert ok_l and ok_e and s_l.took == (1, 0) and s_e.took == (0, 1)
        assert abs(s_l.iteration - s_e.iteration) <= 1
        assert np.linalg.norm(x_l - x_e) <= 1e-9 * np.linalg.norm(x_e)
        eye = sp.identity(n, format="csr")
        a = eye - 0.01 * (m @ (eye - 0.01 * m))
        assert np.linalg.norm(a @ x_l - b_host) <= 1e-8 * np.linalg.norm(b_host)
        mat.close()


def test_degenerate_constants(env):
    api, mesh, oracle, ctx = env
    lib, C = api._lib.lib, api.C
    # alpha1 = 0: A = beta2 I + alpha2 beta1 M, the single-stage operator of storm_hip_solve_cg
    g = mesh.structured_box(24)
    mat = api.StencilMatrix.from_face_graph(ctx, g)
    b_host = 1.0 + 0.25 * np.sin(0.01 * np.arange(g.n_cells))
    a1, b1, a2, b2 = 0.0, 2.0, -1.0e-3, 1.0
    ctx.set_option("latency_path", 2)
    p = api._lib.SolverParams()
    lib.storm_hip_solver_params_default(C.byref(p))
    b = api.DeviceVector.from_numpy(ctx, b_host)
    results = []
    for two in (True, False):
        x, r = api.DeviceVector(ctx, g.n_cells), api._lib.SolverResult()
        before = ctx.counter("latency_solves")
        if two:  # (the C entry point itself, not through a solver object)
            api._lib.check(lib.storm_hip_solve_cg2(mat._h, a1, b1, a2, b2, b._h, x._h, C.byref(p), C.byref(r), None))
        else:
            api._lib.check(lib.storm_hip_solve_cg(mat._h, a2 * b1, b2, b._h, x._h, C.byref(p), C.byref(r), None))
        assert r.converged and r.path_fallback == 0 and ctx.counter("latency_solves") == before + 1
        assert r.num_applies == r.iterations + 1
        results.append((r.iterations, x.to_numpy()))
    ctx.set_option("latency_path", 1)
    assert abs(results[0][0] - results[1][0]) <= 1, (results[0][0], results[1][0])
    assert np.linalg.norm(results[0][1] - results[1][1]) <= 1e-9 * np.linalg.norm(results[1][1])
    mat.close()
    # beta1 = beta2 = 0: A = alpha1 alpha2 M^2 on the diagonally dominant CSR operator
    rng = np.random.default_rng(7)
    n = 1000
    m = _random_spd_csr(rng, n, 12)
    mat = api.StencilMatrix.from_csr(ctx, m)
    consts = (-0.5, 0.0, -0.5, 0.0)
    b_host = rng.random(n) + 0.5
    ok, s, x = _cg2(api, ctx, api.HipTwoStageOperator(mat, *consts), b_host, True)
    ref = oracle.solve("cg", oracle.CallbackOperator(n, _two_stage_fn(oracle.CsrOperator(m).apply, consts)), b_host)
    assert ok and ref.converged and s.took == (1, 0)
    assert abs(s.iteration - ref.iterations) <= max(2, int(0.02 * ref.iterations)), (s.iteration, ref.iterations)
    assert np.linalg.norm(x - ref.x) <= 1e-8 * np.linalg.norm(ref.x)
    mat.close()


def test_convergence_rule_edges_on_the_latency_path(env):
    api, mesh, oracle, ctx = env
    g = mesh.structured_box(10)
    mat = api.StencilMatrix.from_face_graph(ctx, g)
    op = api.HipTwoStageOperator(mat, *OTHER)
    b_host = np.ones(g.n_cells)
    # tolerances off: exactly num_iterations iterate() calls, converged == False
    ok, s, _ = _cg2(api, ctx, op, b_host, True, num_iterations=17, relative_error_tolerance=0.0, absolute_error_tolerance=0.0)
    assert not ok and s.iteration == 17 and len(s.history) == 18 and s.took == (1, 0)
    # the initial residual already meets the absolute tolerance: no iteration, converged (Solver.hpp:124-128)
    ok, s, x = _cg2(api, ctx, op, b_host, True, absolute_error_tolerance=1e9)
    assert ok and s.iteration == 0 and not x.any()
    # num_iterations = 0
    ok, s, x = _cg2(api, ctx, op, b_host, True, num_iterations=0)
    assert not ok and s.iteration == 0 and not x.any()
    # zero right-hand side: safe_divide keeps everything finite (Crow/MathUtils.hpp:49-52)
    ok, s, x = _cg2(api, ctx, op, np.zeros(g.n_cells), True)
    assert np.all(np.isfinite(x)) and not x.any()
    # a warm start is honoured
    ref = oracle.solve("cg", _oracle_op(oracle, g, OTHER), b_host)
    ok, s, x = _cg2(api, ctx, op, b_host, True, x0=ref.x)
    assert s.took == (1, 0) and s.initial_error <= 2e-6 * np.linalg.norm(b_host)  # started from the solution, not from zero
    mat.close()


@pytest.mark.parametrize("shape", [(64, 64, 64), (80, 80, 80)])
def test_two_stage_latency_path_is_bitwise_reproducible(env, shape):
    """The rows of t published by one block are gathered by others behind a synchronisation point only: a row gathered too
    early would show as a run-to-run difference.  600 iterations (1 800 synchronisation points) with the tolerances off,
    three times: bitwise equal histories and solutions."""
    api, mesh, oracle, ctx = env
    g = mesh.structured_box(*shape)
    ctx.set_option("latency_rows", 1 << 21)
    mat = api.StencilMatrix.from_face_graph(ctx, g)
    ctx.set_option("latency_rows", 1 << 19)
    op = api.HipTwoStageOperator(mat, *PLAYGROUND)
    b_host = 1.0 + 0.25 * np.sin(0.01 * np.arange(g.n_cells))
    runs = []
    for _ in range(3):
        ok, s, x = _cg2(api, ctx, op, b_host, True, num_iterations=600, relative_error_tolerance=0.0, absolute_error_tolerance=0.0)
        assert s.took == (1, 0) and s.iteration == 600
        runs.append((np.array(s.history), x))
    for h, x in runs[1:]:
        assert np.array_equal(h, runs[0][0]) and np.array_equal(x, runs[0][1])
    mat.close()


@pytest.mark.parametrize("how", [1, 2])
def test_forced_fallbacks_give_the_engine_result(env, how):
    api, mesh, oracle, ctx = env
    g = mesh.structured_box(24, 20, 16)
    mat = api.StencilMatrix.from_face_graph(ctx, g)
    op = api.HipTwoStageOperator(mat, *PLAYGROUND)
    b_host = 1.0 + 0.25 * np.sin(0.01 * np.arange(g.n_cells))
    x0 = 0.01 * np.cos(0.3 * np.arange(g.n_cells))  # a start that a botched restore of x would show
    ok0, s0, xa = _cg2(api, ctx, op, b_host, True, x0=x0)
    assert ok0 and s0.path_fallback == 0 and s0.took == (1, 0)
    ctx.set_option("coop_force_fail", how)
    ok1, s1, xb = _cg2(api, ctx, op, b_host, True, x0=x0)
    ctx.set_option("coop_force_fail", 0)
    assert ok1 and s1.path_fallback == how, (s1.path_fallback, how)
    assert s1.took[1] == 1  # the engine's loop ran (how == 2: after the cooperative kernel "gave up")
    assert abs(s1.iteration - s0.iteration) <= 1
    assert np.linalg.norm(xa - xb) <= 1e-9 * np.linalg.norm(xa)
    mat.close()


# ---- the other methods ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["bicgstab", "gmres"])
def test_other_engine_methods_on_the_two_stage_operator(env, kind):
    """BiCGStab and GMRES(20) through storm_hip_krylov_set_operator2 (no callback), bounds of tests/test_gpu_cross_product.py."""
    api, mesh, oracle, ctx = env
    g = mesh.structured_box(24)
    mat = api.StencilMatrix.from_face_graph(ctx, g)
    b_host = 1.0 + 0.25 * np.sin(0.01 * np.arange(g.n_cells))
    s = api.BiCgStabSolver() if kind == "bicgstab" else api.GmresSolver()
    if kind == "gmres":
        s.num_inner_iterations = 20
    b, x = api.DeviceVector.from_numpy(ctx, b_host), api.DeviceVector(ctx, g.n_cells)
    before = ctx.counter("engine_solves")
    ok = s.solve(x, b, api.HipTwoStageOperator(mat, *PLAYGROUND))
    assert ok and ctx.counter("engine_solves") == before + 1
    ref = oracle.solve(kind, _oracle_op(oracle, g, PLAYGROUND), b_host, num_inner_iterations=20)
    assert ref.converged
    band = max(4, int(0.1 * ref.iterations)) if kind == "bicgstab" else max(2, int(0.05 * ref.iterations))
    assert abs(s.iteration - ref.iterations) <= band, (s.iteration, ref.iterations)
    assert np.linalg.norm(x.to_numpy() - ref.x) <= 5e-6 * np.linalg.norm(ref.x)
    mat.close()


# ---- the time loop --------------------------------------------------------------------------------------------------------
def test_cahn_hilliard_time_loop_with_the_two_stage_operator(tmp_path):
    """tests/cpp/two_stage_driver.cpp on `square_nb.1`, six steps, against oracle.cahn_hilliard_step_non_uniform with the
    bounds of the `ch-nonuniform` test of tests/test_gpu_timestep_driver.py; every solve is one cooperative kernel."""
    from oracle import oracle

    g = _triangle_mesh("square_nb.1")
    prefix = os.path.join(ROOT, "tests", "golden", "mesh", "square_nb.1.")
    steps = 6
    c = np.random.default_rng(2024).random(g.n_cells)
    c0_path = tmp_path / "c0.f64"
    c.tofile(c0_path)
    p = subprocess.run([os.path.join(ROOT, "tests", "cpp", "two_stage_driver"), prefix, str(c0_path), str(steps), str(tmp_path / "ts")],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + "\n" + p.stderr[-2000:]
    lines = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
    rows, last = lines[:-1], lines[-1]
    assert len(rows) == steps and last["operator_builds"] == 1 and last["cells"] == g.n_cells
    assert last["latency_solves"] == steps
    m = oracle.Mesh(g)
    for k, row in enumerate(rows, 1):
        c, res = oracle.cahn_hilliard_step_non_uniform(m, c)
        assert res.converged and row["converged"] and row["solves_logged"] == k
        assert abs(row["iterations"] - res.iterations) <= 1, (k, row["iterations"], res.iterations)
        dev = np.fromfile(tmp_path / f"ts.step{k}.c.f64")
        assert np.abs(dev - c).max() <= 1e-8 * np.abs(c).max(), (k, np.abs(dev - c).max())
        c = dev  # (the next step starts from the DEVICE's field on both sides: the comparison is per step, not accumulated)
