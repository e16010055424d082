"""The engine's other methods -- CGS, TFQMR, TFQMR1, BiCGStab(l), IDR(s), FGMRES, Richardson and every
Jacobi-preconditioned solve (krylov_methods.hip) -- past their second step, and the x they leave, pinned to exact
references on integer data (tests/exact_ref.py: ``EnginePins``, the table ``ENGINE_STEP_CASES``).

tests/test_gpu_exact_first_step.py holds these methods' histories for K = 2 (1 ... 5 for BiCGStab(l) and IDR(s)) and
drops x.  Their histories come from recurrence residuals that never read x, so nothing there sees an x update dropped,
applied twice or fed the wrong vector -- the axpy of CGS, TFQMR's d, x and the predicated copy of TFQMR1, the gamma
updates of BiCGStab(l), IDR(s)'s two, the three branches of gmres_update_x -- all of which pass through the engine's
held-back and fused statements.  Nor does K = 2 reach BiCGStab(l)'s beta with rho *= -omega, the first beta of a second
cycle, or TFQMR1's copy with its predicate false.

Every case: tolerances off, exactly K iterations; engine_solves moved alone, no fallback; history[0] bitwise where r0
is b, history[k] within tol_k = max(floor_k, 16 e_k) <= 1e-10 of the exact value; ||b - A x|| in long double against the
exact ||b - A x_K|| (formed from the exact x_K, not from the history) under the same rule; below 20 000 rows x itself
against the exact x_K.  The early exits stop by an absolute tolerance halfway between two exact history entries and
check the x of the iteration that met it; GMRES and FGMRES stop at a cycle's last step and inside a cycle
(gmres_finalize's branches).  Each case prints a "ratio" line: the largest |h - exact| / exact, the x distances, the
tolerances."""
import numpy as np
import pytest

import exact_ref as er
import test_gpu_exact_gmres as tg
from test_gpu_exact_first_step import (CLASSES, DEFAULTS, PATHS, SMALL, _check_access_mode, _knobs, _matrix, _method_id, _only,
                                       _problem, _solve)

pytestmark = pytest.mark.gpu

CONFIGS = [("lattice", {}), ("fp64", {}), ("tail", {}), ("lattice", {"lin_fuse": 0}), ("lattice", {"blas1_nt": 2})]
POISSON = [c for c in er.ENGINE_STEP_CASES if c[4] == "poisson" and c[2] is None]
JACOBI = [(m, p, side, shape, K) for shape, _ in er.ENGINE_STEP_BOXES for m, p in er.ENGINE_JACOBI for side in ("left", "right")
          for K in (er.ENGINE_JACOBI_K,)]
CONVDIFF = [c for c in er.ENGINE_STEP_CASES if c[4] == "convdiff"]
GMRES_DEFAULTS = tg.DEFAULTS + (("lin_fuse", 1),)


@pytest.fixture(scope="module")
def env():
    from oracle import oracle
    from stormruler_amd import api, mesh

    ctx = api.Context(0)
    yield api, mesh, ctx, oracle
    _problems.clear(), _gmres.clear()
    ctx.close()


@pytest.fixture(autouse=True)
def _defaults(env):
    yield
    ctx = env[2]
    for k, v in DEFAULTS + GMRES_DEFAULTS:
        ctx.set_option(k, v)


_problems, _gmres = {}, {}


def _step_problem(env, shape, kind):
    """The box with its chains and pins, kept per shape as the sibling files keep theirs."""
    _, mesh, _, oracle = env
    if (shape, kind) not in _problems:
        _problems[shape, kind] = er.StepProblem(oracle, mesh, shape, kind)
        if kind == "poisson":  # the data of tests/test_gpu_exact_first_step.py, whose _problem and _matrix serve here
            assert np.array_equal(_problems[shape, kind].b, _problem(mesh, shape)[1])
    return _problems[shape, kind]


def _shape_id(s):
    return "x".join(map(str, s))


def _config_id(c):
    return c[0] + "".join(f"-{k}{v}" for k, v in c[1].items())


def _report(label, pins, far, xr, k):
    e_res, tol_res, rule, e_x, tol_x = pins.x_tolerances(k)
    print(f"ratio {label}: far {max(far):.1e} at {int(np.argmax(far))}   x " + " ".join(f"{v:.1e}" for v in xr) + "   tol " +
          " ".join("bitwise" if t is None else f"{t:.1e}/{r}" for t, r in zip(pins.tol[:k + 1], pins.rule)) +
          f"   tol_res {tol_res:.1e}/{rule}" + ("" if tol_x is None else f" tol_x {tol_x:.1e}"))


def _check(pins, label, s, x, k=None):
    k = pins.K if k is None else k
    assert s.iteration == k and s.history.size == k + 1, (label, s.iteration, s.history.size)
    far = pins.check(list(s.history), label, k)
    _report(label, pins, far, pins.check_x(x, k, label), k)


def _run(api, ctx, cls, op, b_h, iters, stop=0.0, **knobs):
    """``_solve`` of the first-step file for any operator and with an absolute tolerance: the solve may stop early."""
    s = cls()
    s.num_iterations, s.absolute_error_tolerance, s.relative_error_tolerance = iters, stop, 0.0
    s.record_history = True
    for k, v in knobs.items():
        setattr(s, k, v)
    b = api.DeviceVector.from_numpy(ctx, b_h.astype(np.float64))
    x = api.DeviceVector.from_numpy(ctx, np.zeros(b_h.size))
    before = {k: ctx.counter(k) for k in PATHS + ("nt_stream_launches",)}
    s.solve(x, b, op)
    moved = {k: ctx.counter(k) - before[k] for k in before}
    s.nt_stream_launches = moved.pop("nt_stream_launches")
    assert s.path_fallback == 0
    return s, x.to_numpy(), moved


# ---- K iterations ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("config", CONFIGS, ids=_config_id)
@pytest.mark.parametrize("case", POISSON, ids=lambda c: f"{_method_id(c[:2])}-{_shape_id(c[3])}-K{c[5]}")
def test_engine_steps(env, case, config):
    api, mesh, ctx, _ = env
    kind, param, _, shape, _, K = case
    fmt, opts = config
    p = _step_problem(env, shape, "poisson")
    pins = p.engine_pins(kind, param, None, K)
    mat = _matrix(api, ctx, p.g, fmt)
    for k, v in opts.items():
        ctx.set_option(k, v)
    api.rng_reset()
    s, x, path = _solve(api, ctx, getattr(api, CLASSES[kind]), mat, p.b, iters=K, **_knobs(kind, param))
    _only(path, "engine_solves")
    _check_access_mode(s, opts, p.b.size)
    _check(pins, f"{_method_id(case[:2])} {_config_id(config)} {_shape_id(shape)}", s, x)
    mat.close()


@pytest.mark.parametrize("config", CONFIGS, ids=_config_id)
@pytest.mark.parametrize("case", JACOBI, ids=lambda c: f"{_method_id(c[:2])}-{c[2]}-{_shape_id(c[3])}")
def test_engine_steps_with_jacobi(env, case, config):
    """api.JacobiPreconditioner on either side (Richardson and BiCGStab(l) apply it on the left, FGMRES on the right,
    whatever pre_side says): three iterations, x_3 against the reference restated with P = diag(fl(1 / d))."""
    api, mesh, ctx, _ = env
    kind, param, side, shape, K = case
    fmt, opts = config
    p = _step_problem(env, shape, "poisson")
    pins = p.engine_pins(kind, param, er.ENGINE_FIXED_SIDE.get(kind, side), K)
    mat = _matrix(api, ctx, p.g, fmt)
    d = api.DeviceVector(ctx, p.b.size)
    mat.diagonal(-1.0, 0.0, d, invert=True)
    assert np.array_equal(d.to_numpy(), pins.dinv)  # the dinv the reference is restated with
    if kind == "cg":
        ctx.set_option("generic_solvers", 1)
    for k, v in opts.items():
        ctx.set_option(k, v)
    knobs = dict(_knobs(kind, param), pre_op=api.JacobiPreconditioner(),
                 pre_side=api.PreconditionerSide.Left if side == "left" else api.PreconditionerSide.Right)
    api.rng_reset()
    s, x, path = _solve(api, ctx, getattr(api, CLASSES[kind]), mat, p.b, iters=K, **knobs)
    _only(path, "engine_solves")
    _check_access_mode(s, opts, p.b.size)
    _check(pins, f"{_method_id(case[:2])} jacobi-{side} {_config_id(config)} {_shape_id(shape)}", s, x)
    mat.close()


@pytest.mark.parametrize("lin_fuse", [1, 0])
@pytest.mark.parametrize("case", CONVDIFF, ids=lambda c: f"{_method_id(c[:2])}-{_shape_id(c[3])}-K{c[5]}")
def test_engine_steps_on_the_non_symmetric_box(env, case, lin_fuse):
    """Convection-diffusion, A != A^T: r~ and r swapped in a shadow dot shows.  On 7 x 5 x 3 TFQMR1's omega < tau comes
    out true eight times and then false four times in its six iterations: the predicated copy(x, d) runs both ways."""
    api, mesh, ctx, _ = env
    kind, param, _, shape, _, K = case
    p = _step_problem(env, shape, "convdiff")
    pins = p.engine_pins(kind, param, None, K)
    if kind == "tfqmr1":
        assert pins.preds == [True] * 8 + [False] * 4
    g = p.g
    mat = api.StencilMatrix.from_face_weights(ctx, g.n_cells, g.n_halo, g.inner, g.outer, *p.weights)
    ctx.set_option("lin_fuse", lin_fuse)
    s, x, path = _run(api, ctx, getattr(api, CLASSES[kind]), api.HipStencilOperator(mat, 1.0, 0.0), p.b, K, **_knobs(kind, param))
    _only(path, "engine_solves")
    _check_access_mode(s, {}, p.b.size)
    _check(pins, f"{_method_id(case[:2])} convdiff lin_fuse{lin_fuse} {_shape_id(shape)}", s, x)
    mat.close()


# ---- the early exit ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lin_fuse", [1, 0])
@pytest.mark.parametrize("method", list(er.ENGINE_STOPS), ids=_method_id)
def test_engine_stops_with_the_x_of_that_iteration(env, method, lin_fuse):
    """64 x 48 x 40, num_iterations K, an absolute tolerance that iteration k is the first to meet (er.ENGINE_STOPS:
    k = 3 except for IDR(2) and IDR(4), whose history[3] is above history[1]): the solve stops there with k + 1 history
    entries and x_k.  For BiCGStab(2) iteration 3 is inside a cycle, for BiCGStab(3) a cycle's end."""
    api, mesh, ctx, _ = env
    kind, param = method
    K, k = er.ENGINE_STOPS[method]
    p = _step_problem(env, SMALL, "poisson")
    pins = p.engine_pins(kind, param, None, K)
    mat = _matrix(api, ctx, p.g, "lattice")
    ctx.set_option("lin_fuse", lin_fuse)
    api.rng_reset()
    s, x, path = _run(api, ctx, getattr(api, CLASSES[kind]), api.HipStencilOperator(mat, -1.0, 0.0), p.b, K,
                      pins.stop_between(k), **_knobs(kind, param))
    _only(path, "engine_solves")
    _check(pins, f"{_method_id(method)} stop{k} of {K} lin_fuse{lin_fuse}", s, x, k)
    mat.close()


# ---- GMRES and FGMRES: the tolerance stop ---------------------------------------------------------------------------------------------

GMRES_SHAPES = ((7, 5, 3), (37, 21, 19))
GMRES_K, GMRES_M = 12, 5
# the variants of tests/test_gpu_exact_gmres.py, and FGMRES on the engine: without a preconditioner the same iteration
# (z_k = q_k), x by gmres_update_x's flexible branch
GMRES_VARIANTS = ("default", "engine", "steps4", "cgs2", "fgmres")


def _gmres_problem(env, shape):
    _, mesh, _, oracle = env
    if shape not in _gmres:
        _gmres[shape] = er.GmresProblem(oracle, mesh, shape)
    return _gmres[shape]


@pytest.mark.parametrize("k", er.ENGINE_GMRES_STOPS)
@pytest.mark.parametrize("name", GMRES_VARIANTS)
@pytest.mark.parametrize("shape", GMRES_SHAPES, ids=_shape_id)
def test_gmres_stops_by_tolerance(env, shape, name, k):
    """GMRES(5) with num_iterations 12 and an absolute tolerance halfway between the exact history[k - 1] and
    history[k]: k = 5 is a cycle's last step (gmres_finalize returns early: the cycle's own update already ran), k = 7
    is inside a cycle (the update the `done` predicate skipped is repeated).  history[0..k] and x against ``GmresPins``
    built with K = k, whose restatement finalizes at exit."""
    api, mesh, ctx, _ = env
    p = _gmres_problem(env, shape)
    pins = p.pins(k, GMRES_M)
    assert pins.x is not None
    stop = 0.5 * (pins.exact[k] + pins.exact[k - 1])
    assert pins.exact[k] * 1.05 < stop < min(pins.exact[:k]) / 1.05
    g = p.g
    mat = api.StencilMatrix.from_face_weights(ctx, g.n_cells, g.n_halo, g.inner, g.outer, *p.weights)
    opts, family = tg.VARIANTS["engine" if name == "fgmres" else name]
    opts = dict(opts)
    gram_schmidt = opts.pop("gram_schmidt", 0)
    for key, v in opts.items():
        ctx.set_option(key, v)
    before = {c: ctx.counter(c) for c in tg.COUNTERS}
    s, x, path = _run(api, ctx, api.FgmresSolver if name == "fgmres" else api.GmresSolver, api.HipStencilOperator(mat, 1.0, 0.0),
                      p.b, GMRES_K, stop, num_inner_iterations=GMRES_M, gram_schmidt=gram_schmidt)
    moved = {c: ctx.counter(c) - before[c] for c in tg.COUNTERS}
    label = f"gmres({GMRES_M}) {_shape_id(shape)} {name} stop{k} of {GMRES_K}"
    assert s.iteration == k and s.history.size == k + 1, (label, s.iteration, s.history.size)
    # the chain counters count the steps the host ENQUEUED: it runs `check_lag` iterations ahead of the device's `done`
    # flag (krylov_engine.hpp), so k ... K of them -- the same for every family the variant runs, zero for the others
    want = tg._expected(shape, family, 1)
    steps = set(v for c, v in moved.items() if want[c])
    assert all(v == 0 for c, v in moved.items() if not want[c]) and len(steps) <= 1, (label, moved)
    assert all(k <= v <= GMRES_K for v in steps), (label, moved)
    ratios = pins.check(list(s.history), label)
    tg._report(label, pins, ratios, pins.check_x(x, label))
    mat.close()


@pytest.mark.parametrize("k,K", er.ENGINE_FGMRES_STOPS)
@pytest.mark.parametrize("side", ["left", "right"])
@pytest.mark.parametrize("shape", [b[0] for b in er.ENGINE_STEP_BOXES], ids=_shape_id)
def test_fgmres_with_jacobi_stops_by_tolerance(env, shape, side, k, K):
    """FGMRES(2) with the Jacobi preconditioner on the engine, stopped at iteration 2 of 3 (a cycle's last step) and at 3
    of 4 (inside the second cycle): x from the z_k = P q_k the cycle kept."""
    api, mesh, ctx, _ = env
    p = _step_problem(env, shape, "poisson")
    pins = p.engine_pins("fgmres", er.ENGINE_FGMRES_M, "right", K)
    mat = _matrix(api, ctx, p.g, "lattice")
    knobs = dict(num_inner_iterations=er.ENGINE_FGMRES_M, pre_op=api.JacobiPreconditioner(),
                 pre_side=api.PreconditionerSide.Left if side == "left" else api.PreconditionerSide.Right)
    s, x, path = _run(api, ctx, api.FgmresSolver, api.HipStencilOperator(mat, -1.0, 0.0), p.b, K, pins.stop_between(k), **knobs)
    _only(path, "engine_solves")
    _check(pins, f"fgmres(2) jacobi-{side} {_shape_id(shape)} stop{k} of {K}", s, x, k)
    mat.close()
