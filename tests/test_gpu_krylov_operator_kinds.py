"""An operator set on an engine replaces the previous one completely: whatever kind a ``storm_hip_krylov`` object held
before (native stencil, two-stage, callback, finite-difference Jacobian), after ``set_operator`` it applies and solves
bit for bit like a fresh object that only ever held the new one."""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BOXES = {"5x4x3": (5, 4, 3), "9x8x7": (9, 8, 7)}  # 60 rows: under a wavefront, one padded slice; 504: slices, the last partial
KINDS = ("native", "two_stage", "callback", "fd")
STENCIL = (-0.05, 1.0)           # alpha, beta of A = beta I + alpha M
TWO = (-0.05, 1.0, -0.5, 0.75)   # alpha1, beta1, alpha2, beta2
MU = 1.0e-8


@pytest.fixture(scope="module")
def env():
    from stormruler_amd import api, mesh

    ctx = api.Context(0)
    yield api, mesh, ctx
    _BUILT.clear()
    ctx.close()


_BUILT = {}


def _build(env, name):
    """The four operators over one box, and for every kind the result of a fresh engine that only ever held it (built once)."""
    if name in _BUILT:
        return _BUILT[name]
    api, mesh, ctx = env
    g = mesh.structured_box(*BOXES[name])
    n = g.n_cells
    mat = api.StencilMatrix.from_face_graph(ctx, g)
    y = api.DeviceVector.from_numpy(ctx, np.sin(0.37 * np.arange(n)))
    point = api.DeviceVector.from_numpy(ctx, np.sin(0.37 * np.arange(n) + 1.0))  # the linearisation point of the fd kind
    native = api.HipStencilOperator(mat, *STENCIL)
    callback = api.make_operator(lambda out, x: native.mul(out, x))
    w = api.DeviceVector(ctx, n)
    native.mul(w, point)
    ops = {"native": native, "two_stage": api.HipTwoStageOperator(mat, *TWO), "callback": callback,
           "fd": api.FdJacobianOperator(callback, point, w, MU)}
    fresh = {}
    for kind in KINDS:
        eng, z = api.Krylov(ctx), api.DeviceVector(ctx, n)
        eng.set_operator(ops[kind])
        eng.apply(z, y)
        fresh[kind] = z.to_numpy()
        assert np.isfinite(fresh[kind]).all() and fresh[kind].any()
    _BUILT[name] = (n, ops, y, fresh)
    return _BUILT[name]


@pytest.fixture(scope="module", params=sorted(BOXES))
def problem(env, request):
    return _build(env, request.param)


@pytest.mark.parametrize("first,second", list(itertools.permutations(KINDS, 2)))
def test_apply_after_another_kind_is_the_fresh_engines(env, problem, first, second):
    api, mesh, ctx = env
    n, ops, y, fresh = problem
    eng, z = api.Krylov(ctx), api.DeviceVector(ctx, n)
    eng.set_operator(ops[first])
    eng.apply(z, y)
    assert np.array_equal(z.to_numpy(), fresh[first])
    eng.set_operator(ops[second])
    eng.apply(z, y)
    assert np.array_equal(z.to_numpy(), fresh[second])


def _solver(api, cls):
    s = cls()
    s.num_iterations, s.absolute_error_tolerance, s.relative_error_tolerance = 6, 0.0, 0.0
    s.record_history = True
    s.pre_op = api.JacobiPreconditioner()  # (keeps the solve on the engine rather than a fused kernel)
    return s


@pytest.mark.parametrize("solver", ["CgsSolver", "BiCgStabLSolver"])
def test_solve_after_the_fd_kind_is_the_fresh_engines(env, solver):
    api, mesh, ctx = env
    n, ops, y, fresh = _build(env, "9x8x7")
    b_host = np.sin(0.37 * np.arange(n))

    def run(held_fd):
        s = _solver(api, getattr(api, solver))
        if held_fd:  # the solver's engine has held, and applied, the finite-difference operator
            s._engine = api.Krylov(ctx, s._method)
            s._engine.set_operator(ops["fd"])
            z = api.DeviceVector(ctx, n)
            s._engine.apply(z, y)
            assert np.array_equal(z.to_numpy(), fresh["fd"])
        b, x = api.DeviceVector.from_numpy(ctx, b_host), api.DeviceVector(ctx, n)
        before = ctx.counter("engine_solves")
        s.solve(x, b, ops["native"])
        assert ctx.counter("engine_solves") == before + 1 and s.iteration == 6
        return s, x.to_numpy()

    ref, x_ref = run(False)
    s, x = run(True)
    assert np.isfinite(x_ref).all() and x_ref.any() and ref.history.size == 7
    assert np.array_equal(x, x_ref)
    assert np.array_equal(s.history, ref.history)
    assert s._engine.get_int("inner_iterations") == 0


def test_apply_during_a_stepped_solve_is_refused(env, problem):
    api, mesh, ctx = env
    n, ops, y, fresh = problem
    s = api.CgsSolver()
    s._engine = api.Krylov(ctx, s._method)
    b, x, z = api.DeviceVector.from_numpy(ctx, np.sin(0.37 * np.arange(n))), api.DeviceVector(ctx, n), api.DeviceVector(ctx, n)
    s.init(x, b, ops["native"], None)
    with pytest.raises(api._lib.StormHipError) as e:
        s._engine.apply(z, y)
    s.finalize(x, b, ops["native"], None)
    assert "krylov_apply: a solve is in progress on this object" in str(e.value)
    s._engine.apply(z, y)  # ... and taken again once the sequence is over
    assert np.array_equal(z.to_numpy(), fresh["native"])
