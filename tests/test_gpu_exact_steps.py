"""CG and BiCGStab past their first step, pinned to exact references on integer data (tests/exact_ref.py: ``cg``,
``bicgstab``, ``StepPins``): history[0..K] and the x the solver leaves, K = 8 for CG, 5 for BiCGStab, 4 for CG on the
two-stage operator (I + A)^2.

tests/test_gpu_exact_first_step.py holds every path to closed forms after ONE iteration from x0 = 0.  One iteration
never runs what solve_cg_body (solver_cg.hip) does from the second on: the step kernel ending iteration k - 1 inside
iteration k's SpMV with p and p_alt swapped, cg_r_recompute_kernel / cg_r_planes_kernel in place of cg_r_kernel, the <p,z>
fold inside the plane march, the sweep direction alternating with the iteration, the tail cg_xp_kernel; nor BiCGStab's
beta = (rho / rho_bar)(alpha / omega), p = r + beta (p - omega v), and the latency kernel's v0 / v1 by parity.  The
bitwise tests between forms compare device loops that share their scalars and their host loop; here the ground truth is
Python Fractions over the integer Krylov chain.

Every case: tolerances off, exactly K iterations, record_history; path_fallback == 0; the path and kernel counters the
case is there for; history[0] bitwise, history[k] within tol_k = max(floor_k, 16 e_k) <= 1e-10 of the exact value (e_k:
the oracle's own distance from it; history[1] by the first step's closed form where that is tighter); ||b - A x|| in long
double within the same rule of the exact history[K]; below 20 000 rows x itself against the exact x_K.  The early-exit
cases stop at iteration 3 of K by an absolute tolerance halfway between the exact history[2] and history[3] and check
x_3: the x update is keyed to the iteration that ran, not to the last one enqueued.  Each case prints the largest
|h - exact| / exact and the x distances ("steps" lines)."""
import numpy as np
import pytest

import exact_ref as er
from test_gpu_exact_first_step import BICG, CG_SMALL, DEFAULTS as FIRST_DEFAULTS, ODD, PATHS, SMALL, _matrix, _only

pytestmark = pytest.mark.gpu

PLANES = (256, 128, 130)  # 4.26 M rows, 16 runs of 2 048 rows per plane: the plane march (tests/test_gpu_residual_planes.py)
NO_PLANES = (200, 100, 211)  # 4.22 M rows, planes of 20 000 rows: cg_r_recompute_kernel, the gathering form
CONVDIFF = (40, 30, 17)  # the GMRES pins' non-symmetric box: A != A^T, so a swapped r~ and r shows
FUSED_COUNTERS = ("cg_fused_steps", "cg_residual_marches", "cg_residual_plane_marches", "cg_pz_consumer_folds")
DEFAULTS = FIRST_DEFAULTS + (("resident_planes", 0), ("coop_force_fail", 0))
FUSED_DEFAULTS = (("spmv_record_index", 1), ("cg_residual_march", 1), ("cg_residual_planes", 1), ("cg_residual_chunk", 16),
                  ("cg_march", 8), ("cg_pz_fold", 1), ("cg_fuse", 1), ("ticket_reduce", 1))


@pytest.fixture(scope="module")
def env():
    from oracle import oracle
    from stormruler_amd import api, mesh

    ctx = api.Context(0)
    yield api, mesh, oracle, ctx
    _problems.clear()
    ctx.close()


@pytest.fixture(scope="module")
def fused_env(env):
    """A context of its own for the fused step: no latency kernel, the tiled kernel at every size, the chunk sizes asked
    for however small the lattice (as tests/test_gpu_residual_planes.py sets them)."""
    api, mesh, oracle, _ = env
    ctx = api.Context(0)
    for k in ("latency_path", "spmv_canon_tile_min_rows", "cg_march_fill", "cg_residual_fill"):
        ctx.set_option(k, 0)
    yield api, mesh, oracle, ctx
    for mat in _fused_matrices.values():
        mat.close()
    _fused_matrices.clear()
    ctx.close()


@pytest.fixture(autouse=True)
def _defaults(env):
    yield
    ctx = env[3]
    for k, v in DEFAULTS:
        ctx.set_option(k, v)


_problems, _fused_matrices = {}, {}


def _problem(env, shape, method, kind="poisson"):
    """The problem of a shape and its pins for ``method``, built once and kept; of the 4 M-row shapes one at a time (a
    chain of 300 MB and an operator of 30 M entries)."""
    _, mesh, oracle, _ = env
    assert (shape, kind) in er.STEP_CASES[method]  # (its caps hold on the reference alone: tests/test_exact_reference.py)
    key = (shape, kind)
    if key not in _problems:
        if shape in (PLANES, NO_PLANES):
            for other in (PLANES, NO_PLANES):
                _problems.pop((other, kind), None)
        _problems[key] = er.StepProblem(oracle, mesh, shape, kind)
    return _problems[key], _problems[key].pins(method)


def _solve(api, ctx, cls, op, p, iters, stop=0.0):
    s = cls()
    s.num_iterations, s.absolute_error_tolerance, s.relative_error_tolerance = iters, stop, 0.0
    s.record_history = True
    b = api.DeviceVector.from_numpy(ctx, p.b.astype(np.float64))
    x = api.DeviceVector.from_numpy(ctx, np.zeros(p.b.size))
    before = {k: ctx.counter(k) for k in PATHS + FUSED_COUNTERS[1:] + ("nt_stream_launches",)}
    s.solve(x, b, op)
    moved = {k: ctx.counter(k) - before[k] for k in before}
    assert s.path_fallback == 0
    return s, x.to_numpy(), moved


def _check(pins, label, s, x, k=None):
    k = pins.K if k is None else k
    assert s.iteration == k and s.history.size == k + 1, (label, s.iteration, s.history.size)
    far = pins.check(list(s.history), label, k)
    xr = pins.check_x(x, k, label)
    tol_res = pins.x_tolerances(k)
    print(f"steps {label}: far {max(far):.1e} at {int(np.argmax(far))}   x " + " ".join(f"{v:.1e}" for v in xr) +
          "   tol " + " ".join("bitwise" if t is None else f"{t:.1e}/{r}" for t, r in zip(pins.tol[:k + 1], pins.rule)) +
          f"   tol_res {tol_res[1]:.1e}/{tol_res[2]}" + ("" if tol_res[4] is None else f" tol_x {tol_res[4]:.1e}"))


def _case_id(c):
    return f"{c[0]}-{c[2]}" + "".join(f"-{k}{v}" for k, v in c[1].items())


def _shape_id(s):
    return "x".join(map(str, s))


def _small_case(env, shape, case, cls, method, k=None, fused=None):
    """One row of CG_SMALL / BICG on a Poisson box: K iterations (or the early exit at k) on the path the row names."""
    api, mesh, oracle, ctx = env
    fmt, opts, key = case[:3]
    if shape == ODD and key == "resident_solves":
        key = "latency_solves"  # (an odd line length: no resident kernel; the latency path takes it)
    p, pins = _problem(env, shape, method)
    mat = _matrix(api, ctx, p.g, fmt)
    for name, v in opts.items():
        ctx.set_option(name, v)
    stop = 0.0 if k is None else pins.stop_between(k)
    s, x, moved = _solve(api, ctx, cls, api.HipStencilOperator(mat, -1.0, 0.0), p, pins.K, stop)
    _only({name: moved[name] for name in PATHS}, key, fused)
    # (the host's choice of instance at the streaming launch sites; both shapes are far below the default's size switch)
    assert (moved["nt_stream_launches"] > 0) == (opts.get("blas1_nt", 1) == 2), (opts, moved)
    _check(pins, f"{method} {_shape_id(shape)} {_case_id(case)}" + ("" if k is None else f" stop{k}"), s, x, k)
    mat.close()


# ---- CG: the small shapes ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [SMALL, ODD], ids=_shape_id)
@pytest.mark.parametrize("case", CG_SMALL, ids=_case_id)
def test_cg_steps(env, shape, case):
    """Every row of the first step's CG_SMALL for 8 iterations: the resident and the latency kernel, the throughput loop
    with and without tickets (cg_xp_kernel and the alternating sweeps), the CSR tail, the engine."""
    _small_case(env, shape, case, env[0].CgSolver, "cg", fused=case[3])


@pytest.mark.parametrize("shape,planes", [((36, 30, 8), 3), ((64, 64, 12), 6)], ids=lambda v: str(v).replace(" ", ""))
def test_cg_steps_resident_with_forced_planes(env, shape, planes):
    """The resident kernel with boxes of exactly 3 planes (chunks of 3, 3, 2; a last run of 56 rows) and of 6."""
    api, mesh, oracle, ctx = env
    p, pins = _problem(env, shape, "cg")
    mat = _matrix(api, ctx, p.g, "lattice")
    ctx.set_option("resident_planes", planes)
    s, x, moved = _solve(api, ctx, api.CgSolver, api.HipStencilOperator(mat, -1.0, 0.0), p, pins.K)
    _only({name: moved[name] for name in PATHS}, "resident_solves", 0)
    _check(pins, f"cg {_shape_id(shape)} resident planes {planes}", s, x)
    mat.close()


def _non_temporal(rows):
    """The throughput and engine rows of a first-step table with every streaming launch on its non-temporal instance
    (blas1_nt 2: cg_r_kernel, cg_xp_kernel, the BiCGStab statements, the engine's): the same path, the same pins."""
    return [(c[0], dict(c[1], blas1_nt=2)) + tuple(c[2:]) for c in rows if c[2] in ("throughput_solves", "engine_solves")]


CG_NT, BICG_NT = _non_temporal(CG_SMALL), _non_temporal(BICG)
assert len(CG_NT) == 9 and len(BICG_NT) == 5


@pytest.mark.parametrize("shape", [SMALL, ODD], ids=_shape_id)
@pytest.mark.parametrize("case", CG_NT, ids=_case_id)
def test_cg_steps_non_temporal(env, shape, case):
    _small_case(env, shape, case, env[0].CgSolver, "cg", fused=case[3])


@pytest.mark.parametrize("shape", [SMALL, ODD], ids=_shape_id)
@pytest.mark.parametrize("case", BICG_NT, ids=_case_id)
def test_bicgstab_steps_non_temporal(env, shape, case):
    _small_case(env, shape, case, env[0].BiCgStabSolver, "bicgstab")


# ---- CG: the fused step -------------------------------------------------------------------------------------------------------

# name: (options, (cg_fused_steps, cg_residual_marches, cg_residual_plane_marches, cg_pz_consumer_folds) on PLANES)
FUSED = {
    "planes": ({}, (1, 1, 1, 1)),  # cg_r_planes_kernel with the <p,z> fold inside it
    "gather": ({"cg_residual_planes": 0}, (1, 1, 0, 0)),  # cg_r_recompute_kernel
    "z": ({"cg_residual_march": 0}, (1, 0, 0, 0)),  # z stored by the step kernel, cg_r_kernel reads it back
    "launch": ({"cg_pz_fold": 0}, (1, 1, 1, 0)),  # the one-block launch between step kernel and plane march
    "records8": ({"spmv_record_index": 0}, (1, 1, 1, 1)),  # 8-byte records
    "march5": ({"cg_march": 5}, (1, 1, 1, 1)),  # 26 chunks of 5 planes, 3 328 partials
    "chunk3": ({"cg_residual_chunk": 3}, (1, 1, 1, 1)),  # a last residual chunk of ONE plane
    "unfused": ({"cg_fuse": 0}, (0, 0, 0, 0)),  # cg_xp_kernel every iteration, the sweeps alternating
    "no-tickets": ({"ticket_reduce": 0}, (0, 0, 0, 0)),  # ... and every sum through reduce_finish_kernel
}
assert PLANES[2] % 3 == 1 and (PLANES[0] * PLANES[1]) % er.STREAM_BLOCK == 0 and (NO_PLANES[0] * NO_PLANES[1]) % er.STREAM_BLOCK


def _fused_matrix(fenv, p, idx):
    api, mesh, oracle, ctx = fenv
    key = (p.shape, idx)
    if key not in _fused_matrices:
        for other in [k for k in _fused_matrices if k[0] != p.shape]:
            _fused_matrices.pop(other).close()
        ctx.set_option("spmv_record_index", idx)
        _fused_matrices[key] = api.StencilMatrix.from_face_graph(ctx, p.g)
        assert _fused_matrices[key].stats()["paired_rows"] == 2
    return _fused_matrices[key]


def _fused_case(fenv, shape, name, want, k=None):
    api, mesh, oracle, ctx = fenv
    opts = FUSED[name][0]
    p, pins = _problem(fenv, shape, "cg")
    mat = _fused_matrix(fenv, p, opts.get("spmv_record_index", 1))
    try:
        for key, v in opts.items():
            ctx.set_option(key, v)
        stop = 0.0 if k is None else pins.stop_between(k)
        s, x, moved = _solve(api, ctx, api.CgSolver, api.HipStencilOperator(mat, -1.0, 0.0), p, pins.K, stop)
    finally:
        for key, v in FUSED_DEFAULTS:
            ctx.set_option(key, v)
    _only({key: moved[key] for key in PATHS}, "throughput_solves", want[0])
    assert tuple(moved[key] for key in FUSED_COUNTERS[1:]) == want[1:], (name, moved)
    _check(pins, f"cg {_shape_id(shape)} fused-{name}" + ("" if k is None else f" stop{k}"), s, x, k)


@pytest.mark.parametrize("name", list(FUSED))
def test_cg_steps_fused_with_plane_marches(env, fused_env, name):
    _fused_case(fused_env, PLANES, name, FUSED[name][1])


@pytest.mark.parametrize("name", ["planes", "z"])
def test_cg_steps_fused_where_planes_are_not_whole_runs(env, fused_env, name):
    """200 x 100 x 211: no plane march whatever `cg_residual_planes` says; "planes" runs the gathering
    cg_r_recompute_kernel, "z" cg_r_kernel."""
    _fused_case(fused_env, NO_PLANES, name, {"planes": (1, 1, 0, 0), "z": (1, 0, 0, 0)}[name])


# ---- the early exit -------------------------------------------------------------------------------------------------------------

STOP_AT = er.STEP_STOP
CG_STOP = [CG_SMALL[0], CG_SMALL[2], ("lattice", {"latency_path": 0, "ticket_reduce": 0}, "throughput_solves", 0),
           ("lattice", {"generic_solvers": 1}, "engine_solves", 0)]
BICG_STOP = BICG[:3]
assert [c[2] for c in CG_STOP] == ["resident_solves", "latency_solves", "throughput_solves", "engine_solves"]
assert [c[2] for c in BICG_STOP] == ["resident_solves", "latency_solves", "throughput_solves"]


@pytest.mark.parametrize("case", CG_STOP, ids=_case_id)
def test_cg_stops_at_iteration_3_with_x_3(env, case):
    _small_case(env, SMALL, case, env[0].CgSolver, "cg", k=STOP_AT, fused=case[3])


def test_cg_fused_stops_at_iteration_3_with_x_3(env, fused_env):
    """The fused step with plane march and fold: iteration 4 is enqueued behind the converging one and must not reach x
    (the tail cg_xp_kernel is keyed to the iteration that ran)."""
    _fused_case(fused_env, PLANES, "planes", FUSED["planes"][1], k=STOP_AT)


@pytest.mark.parametrize("case", BICG_STOP, ids=_case_id)
def test_bicgstab_stops_at_iteration_3_with_x_3(env, case):
    _small_case(env, SMALL, case, env[0].BiCgStabSolver, "bicgstab", k=STOP_AT)


# ---- BiCGStab ---------------------------------------------------------------------------------------------------------------------

BICG_CASES = [(SMALL, c) for c in BICG] + [(ODD, c) for c in BICG if c[2] in ("latency_solves", "throughput_solves")]


@pytest.mark.parametrize("shape,case", BICG_CASES, ids=[f"{_shape_id(s)}-{_case_id(c)}" for s, c in BICG_CASES])
def test_bicgstab_steps(env, shape, case):
    """5 iterations: beta and p = r + beta (p - omega v) four times, each parity buffer of the latency kernel twice."""
    _small_case(env, shape, case, env[0].BiCgStabSolver, "bicgstab")


def test_bicgstab_steps_on_the_non_symmetric_box(env):
    """The throughput loop on convection-diffusion (40 x 30 x 17, v = (2, 1, -1)): <r~, v> and <r~, r> are not <r, v>
    and <r, r> of a symmetric operator with the vectors swapped."""
    api, mesh, oracle, ctx = env
    p, pins = _problem(env, CONVDIFF, "bicgstab", "convdiff")
    g = p.g
    mat = api.StencilMatrix.from_face_weights(ctx, g.n_cells, g.n_halo, g.inner, g.outer, *p.weights)
    ctx.set_option("latency_path", 0)
    s, x, moved = _solve(api, ctx, api.BiCgStabSolver, api.HipStencilOperator(mat, 1.0, 0.0), p, pins.K)
    _only({name: moved[name] for name in PATHS}, "throughput_solves")
    _check(pins, f"bicgstab convdiff {_shape_id(CONVDIFF)} throughput", s, x)
    mat.close()


# ---- CG on the two-stage operator ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("how", ["latency", "engine", "forced"])
@pytest.mark.parametrize("shape", [(24, 24, 24), (9, 7, 1)], ids=_shape_id)
def test_two_stage_cg_steps(env, shape, how):
    """HipTwoStageOperator with (alpha1, beta1, alpha2, beta2) = (-1, 2, -1, 1): (I + A)^2, an integer SPD polynomial of
    A = -L.  "latency": cg2_latency_kernel; "engine": the engine's loop with `latency_path` 0; "forced": the cooperative
    launch "fails" (`coop_force_fail` 1) and the engine's loop takes the solve -- path_fallback says so."""
    api, mesh, oracle, ctx = env
    p, pins = _problem(env, shape, "cg2")
    mat = api.StencilMatrix.from_face_graph(ctx, p.g)
    op = api.HipTwoStageOperator(mat, *er.TWO_STAGE)
    ctx.set_option("latency_path", 0 if how == "engine" else 2)
    ctx.set_option("coop_force_fail", 1 if how == "forced" else 0)
    s = api.CgSolver()
    s.num_iterations, s.absolute_error_tolerance, s.relative_error_tolerance, s.record_history = pins.K, 0.0, 0.0, True
    b = api.DeviceVector.from_numpy(ctx, p.b.astype(np.float64))
    x = api.DeviceVector.from_numpy(ctx, np.zeros(p.b.size))
    before = {k: ctx.counter(k) for k in PATHS}
    s.solve(x, b, op)
    moved = {k: ctx.counter(k) - before[k] for k in PATHS}
    assert s.path_fallback == (1 if how == "forced" else 0)
    _only(moved, "latency_solves" if how == "latency" else "engine_solves")
    _check(pins, f"cg2 {_shape_id(shape)} {how}", s, x.to_numpy())
    mat.close()
