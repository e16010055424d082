"""The first iteration of every solver path pinned to closed forms on integer data (tests/exact_ref.py).

With x0 = 0, r0 = b and b integer on a unit-spacing box, <r,r> and <p,z> of iteration 0 are exact integers on every
correct path, so:
    history[0]           == sqrt(rr), bitwise, every solver
    CG x1                == fl(fl(rr / pz) * b_i), bitwise, every element: the whole <p,z> and <r,r> reduction of
                            iteration 0, whatever grid, fold or format produced it
    CG / GMRES / BiCGStab history[1]  within a tolerance derived from the data and the fold depth (<= 1e-12)
    the engine's CGS, TFQMR(1), Richardson, BiCGStab(l), IDR(s) and Jacobi-preconditioned solves: history[0..K]
                            against the exact coefficient-form reference (exact_ref.Pins)
Each case asserts the path it is meant to reach from the context's path counters and the operator's stats; the
comment names the <p,z> branch of the fused CG loop (solver_cg.hip, storm_hip_solve_cg; the branches themselves:
Driver::finish_dots, solver_fused.hip) it takes.

What one iteration cannot reach -- the step kernel that ends iteration k - 1 inside iteration k's SpMV, the residual
recompute and its plane march, the <p,z> fold inside it, the tail x update, BiCGStab's beta and parity buffers -- is
pinned by tests/test_gpu_exact_steps.py: the rows of CG_SMALL and BICG below for 8 (CG) and 5 (BiCGStab) iterations, the
fused step on 4 M rows, CG on the two-stage operator for 4, against exact_ref.StepPins (history[0..K] and x_K)."""
import math

import numpy as np
import pytest

import exact_ref as er

pytestmark = pytest.mark.gpu

PATHS = ("resident_solves", "latency_solves", "throughput_solves", "engine_solves", "cg_fused_steps")
SMALL = (64, 48, 40)  # 122 880 rows: nx even, a plane of 64 x 48 -- the resident and latency kernels take it
ODD = (37, 21, 19)  # odd everything: ragged lines, planes and blocks
# 256 x 256 x 258: the SpMV of iteration 0 leaves more per-wave partials than one pass folds (256^3 sits at exactly
# kSinglePassPartials = 8192), so the fused CG reaches its branches for nb > kSinglePassPartials
BIG = (256, 256, 258)
NT_ROWS = 6 << 20  # kBlas1NtRows (common.hpp): from here on the default blas1_nt = 1 streams non-temporally


@pytest.fixture(scope="module")
def env():
    from stormruler_amd import api, mesh

    ctx = api.Context(0)
    yield api, mesh, ctx
    ctx.close()


DEFAULTS = (("resident_path", 1), ("latency_path", 1), ("generic_solvers", 0), ("ticket_reduce", 1), ("coop_mgs", 1),
            ("spmv_record_index", 1), ("spmv_dict", 4), ("ell_cap", 0), ("lazy_statements", 0), ("test_disable", 0),
            ("fused_reduce", 1), ("lin_fuse", 1), ("blas1_nt", 1))


@pytest.fixture(autouse=True)
def _defaults(env):
    yield
    _, _, ctx = env
    for k, v in DEFAULTS:
        ctx.set_option(k, v)


_cache = {}


def _problem(mesh, shape):
    if shape not in _cache:
        _cache.clear()
        g = er.unit_box(mesh, *shape)
        b = er.int_vector(g.n_cells, 31)
        _cache[shape] = (g, b, er.FirstStep(er.Sums(shape, b)))
    return _cache[shape]


def _matrix(api, ctx, g, fmt):
    """fmt: "lattice" (format 4, the one-byte row index on), "lattice8" (format 4, 8-byte records), "fp64" (fp64
    weights and int32 columns) or "tail" (fp64 records, ell_cap 3: half of every row in a CSR tail)."""
    ctx.set_option("spmv_dict", 0 if fmt in ("fp64", "tail") else 4)
    ctx.set_option("ell_cap", 3 if fmt == "tail" else 0)
    mat = api.StencilMatrix.from_face_graph(ctx, g)
    ctx.set_option("spmv_dict", 4)
    ctx.set_option("ell_cap", 0)
    ctx.set_option("spmv_record_index", 0 if fmt == "lattice8" else 1)
    st = mat.stats()
    if fmt.startswith("lattice"):
        assert st["paired_rows"] == 2 and st["tail_rows"] == 0
    elif fmt == "fp64":
        assert st["value_dictionary_size"] == 0 and st["tail_rows"] == 0
    else:
        assert st["tail_rows"] > 0
    return mat


def _solve(api, ctx, cls, mat, b_h, x0=None, iters=1, **knobs):
    s = cls()
    s.num_iterations, s.absolute_error_tolerance, s.relative_error_tolerance = iters, 0.0, 0.0
    s.record_history = True
    for k, v in knobs.items():
        setattr(s, k, v)
    b = api.DeviceVector.from_numpy(ctx, b_h.astype(np.float64))
    x = api.DeviceVector.from_numpy(ctx, np.zeros(b_h.size) if x0 is None else x0.astype(np.float64))
    before = {k: ctx.counter(k) for k in PATHS}
    nt_before = ctx.counter("nt_stream_launches")
    s.solve(x, b, api.HipStencilOperator(mat, -1.0, 0.0))
    path = {k: ctx.counter(k) - before[k] for k in PATHS}
    s.nt_stream_launches = ctx.counter("nt_stream_launches") - nt_before
    assert s.path_fallback == 0 and s.iteration == iters and s.history.size == iters + 1
    return s, x.to_numpy(), path


def _check_access_mode(s, opts, n_rows):
    """Option blas1_nt 2: the solve's launch sites chose the non-temporal instances (counter nt_stream_launches: the
    host's choice); 0, or the default below the size switch: none did."""
    assert n_rows < NT_ROWS
    if opts.get("blas1_nt", 1) == 2:
        assert s.nt_stream_launches > 0, s.nt_stream_launches
    else:
        assert s.nt_stream_launches == 0, s.nt_stream_launches


def _only(path, key, fused=None):
    want = {k: 0 for k in PATHS}
    want[key] = 1
    if fused is not None:
        want["cg_fused_steps"] = fused
    else:
        want.pop("cg_fused_steps")
        path = {k: v for k, v in path.items() if k != "cg_fused_steps"}
    assert path == want, path


def _check_cg(api, s, x, fs, b_h):
    assert s.history[0] == fs.h0
    assert np.array_equal(x, fs.cg_x1(b_h)), f"x1: {np.count_nonzero(x != fs.cg_x1(b_h))} elements differ"
    assert er.close(s.history[1], fs.cg_h1, fs.cg_tol), (s.history[1], fs.cg_h1)


# ---- CG ----------------------------------------------------------------------------------------------------------------

# (options, expected path, cg_fused_steps or None)
CG_SMALL = [
    # resident.hip: the persistent kernel, a box per block, its own in-kernel folds
    ("lattice", {}, "resident_solves", 0),
    ("lattice8", {}, "resident_solves", 0),
    # latency.hip: the whole solve as one cooperative kernel
    ("lattice", {"resident_path": 0}, "latency_solves", 0),
    ("fp64", {}, "latency_solves", 0),
    ("tail", {}, "latency_solves", 0),
    # the throughput loop: <p,z> finished by tickets inside the SpMV kernel (tick_spmv: few partials) and <r,r> inside
    # cg_r_kernel; on fp64 records and the lattice format alike
    ("lattice", {"latency_path": 0}, "throughput_solves", None),
    ("fp64", {"latency_path": 0}, "throughput_solves", None),
    # ... without tickets: <p,z> and <r,r> through reduce_finish_kernel (Driver::finish)
    ("lattice", {"latency_path": 0, "ticket_reduce": 0}, "throughput_solves", 0),
    ("fp64", {"latency_path": 0, "ticket_reduce": 0}, "throughput_solves", 0),
    # CSR tail: no fused dot in the SpMV (nb == 0), <p,z> by a separate k_multi_dot
    ("tail", {"latency_path": 0}, "throughput_solves", 0),
    ("tail", {"latency_path": 0, "ticket_reduce": 0}, "throughput_solves", 0),
    # the engine (krylov_*.hip): the reference's statements as kernels, scalar programs behind reduce_finish_kernel
    ("lattice", {"generic_solvers": 1}, "engine_solves", 0),
    ("tail", {"generic_solvers": 1}, "engine_solves", 0),
    ("lattice", {"generic_solvers": 1, "ticket_reduce": 0}, "engine_solves", 0),
]


@pytest.mark.parametrize("shape", [SMALL, ODD])
@pytest.mark.parametrize("case", CG_SMALL, ids=lambda c: f"{c[0]}-{c[2]}-" + "-".join(f"{k}{v}" for k, v in c[1].items()))
def test_cg_first_step(env, shape, case):
    api, mesh, ctx = env
    fmt, opts, key, fused = case
    if shape == ODD and key == "resident_solves":
        key = "latency_solves"  # (an odd line length: no resident kernel; the latency path takes it)
    g, b_h, fs = _problem(mesh, shape)
    mat = _matrix(api, ctx, g, fmt)
    for k, v in opts.items():
        ctx.set_option(k, v)
    s, x, path = _solve(api, ctx, api.CgSolver, mat, b_h)
    _only(path, key, fused)
    _check_cg(api, s, x, fs, b_h)
    mat.close()


@pytest.mark.parametrize("ticket", [1, 0])
@pytest.mark.parametrize("fmt", ["lattice", "lattice8"])
def test_cg_first_step_many_partials(env, fmt, ticket):
    """256 x 256 x 258, nb > kSinglePassPartials in the SpMV of iteration 0:
    ticket_reduce 1 -- the fused step loop (cg_fused_steps), <p,z> by reduce_stage1_ticket_kernel<1> (one launch folds
                       the partials and finishes the sum), <r,r> by tickets inside cg_r_kernel;
    ticket_reduce 0 -- no fused step; <p,z> by reduce_stage1_kernel with the fold of its kStage2 results inside
                       cg_r_kernel (pz_partials), <r,r> by reduce_finish_kernel."""
    api, mesh, ctx = env
    g, b_h, fs = _problem(mesh, BIG)
    mat = _matrix(api, ctx, g, fmt)
    ctx.set_option("ticket_reduce", ticket)
    s, x, path = _solve(api, ctx, api.CgSolver, mat, b_h)
    _only(path, "throughput_solves", ticket)
    _check_cg(api, s, x, fs, b_h)
    mat.close()


def test_cg_first_step_from_an_integer_x0(env):
    """history[0] with x0 != 0: the residual r0 = b - A x0 formed by the init kernels is an exact integer vector."""
    api, mesh, ctx = env
    shape = SMALL
    g, b_h, _ = _problem(mesh, shape)
    x0 = er.int_vector(g.n_cells, 41, -50, 50)
    r0 = b_h - er.int_apply(shape, x0)
    h0 = math.sqrt(float(er.exact_dot(r0, r0)))
    mat = _matrix(api, ctx, g, "lattice")
    for opts, key in (({}, "resident_solves"), ({"resident_path": 0}, "latency_solves"),
                      ({"latency_path": 0}, "throughput_solves"), ({"generic_solvers": 1}, "engine_solves")):
        for k, v in DEFAULTS:
            ctx.set_option(k, v)
        for k, v in opts.items():
            ctx.set_option(k, v)
        s, _, path = _solve(api, ctx, api.CgSolver, mat, b_h, x0=x0)
        _only(path, key)
        assert s.history[0] == h0, key
    mat.close()


@pytest.mark.parametrize("lazy", [0, 1, 2])
def test_python_cg_step_under_lazy_statements(env, lazy):
    """The reference's CG body written against the vector interface (SolverCg.hpp:96-123), run at lazy_statements
    0 (every statement a kernel), 1 and 2 (statements wait; the apply's dot rides in the SpMV, x += alpha p; r -=
    alpha z; <r,r> leave as one lazy_lin_kernel pass; at 2 the second iteration's p' = r + beta p; z = A p'; <p',z>
    is the library's fused step)."""
    api, mesh, ctx = env
    g, b_h, fs = _problem(mesh, SMALL)
    mat = _matrix(api, ctx, g, "lattice")
    op = api.HipStencilOperator(mat, -1.0, 0.0)
    n = g.n_cells
    b = api.DeviceVector.from_numpy(ctx, b_h.astype(np.float64))
    x, r, p, z = (api.DeviceVector(ctx, n) for _ in range(4))
    ctx.set_option("lazy_statements", lazy)
    before = ctx.counter("lazy_apply_dots")
    api.fill_with(x, 0.0)
    r <<= b
    p <<= b
    gamma = api.dot_product(r, r)
    op.mul(z, p)
    alpha = api.safe_divide(gamma, api.dot_product(p, z))
    x += alpha * p
    r -= alpha * z
    gamma1 = api.dot_product(r, r)
    rode = ctx.counter("lazy_apply_dots") - before
    ctx.set_option("lazy_statements", 0)
    assert rode == (1 if lazy else 0)
    assert math.sqrt(gamma) == fs.h0 and alpha == fs.cg_alpha
    assert np.array_equal(x.to_numpy(), fs.cg_x1(b_h))
    assert er.close(math.sqrt(gamma1), fs.cg_h1, fs.cg_tol)
    mat.close()


# ---- BiCGStab and GMRES -------------------------------------------------------------------------------------------------

BICG = [
    ("lattice", {}, "resident_solves"),
    ("lattice", {"resident_path": 0}, "latency_solves"),
    ("lattice", {"latency_path": 0}, "throughput_solves"),
    ("lattice", {"latency_path": 0, "ticket_reduce": 0}, "throughput_solves"),
    ("fp64", {"latency_path": 0}, "throughput_solves"),
    ("tail", {"latency_path": 0}, "throughput_solves"),
    ("lattice", {"generic_solvers": 1}, "engine_solves"),
]


@pytest.mark.parametrize("case", BICG, ids=lambda c: f"{c[0]}-{c[2]}-" + "-".join(f"{k}{v}" for k, v in c[1].items()))
def test_bicgstab_first_step(env, case):
    api, mesh, ctx = env
    fmt, opts, key = case
    g, b_h, fs = _problem(mesh, SMALL)
    mat = _matrix(api, ctx, g, fmt)
    for k, v in opts.items():
        ctx.set_option(k, v)
    s, _, path = _solve(api, ctx, api.BiCgStabSolver, mat, b_h)
    _only(path, key)
    assert s.history[0] == fs.h0
    assert er.close(s.history[1], fs.bicgstab_h1, fs.bicgstab_tol), (s.history[1], fs.bicgstab_h1)
    mat.close()


@pytest.mark.parametrize("chain", [(1, 0), (1, 128), (0, 0)], ids=lambda c: f"coop{c[0]}-td{c[1]}")
@pytest.mark.parametrize("m", [1, 30])
@pytest.mark.parametrize("fmt", ["lattice", "fp64"])
def test_gmres_first_step(env, fmt, m, chain):
    """GMRES(m), any m: history[1] = sqrt(rr - pz^2 / zz).  coop_mgs 1: the Gram-Schmidt step runs as a chain kernel
    (counter mgs_chain_steps; test_disable 128 deals its row chunks out by block index instead of by XCD runs);
    0: one kernel per statement.  (Bits 256 and 512 act only from the second basis vector on -- the order of the
    vectors, the earlier rotations -- so the first step cannot see them: tests/test_gpu_gmres_chain_hooks.py.)"""
    coop_mgs, test_disable = chain
    api, mesh, ctx = env
    g, b_h, fs = _problem(mesh, SMALL)
    mat = _matrix(api, ctx, g, fmt)
    ctx.set_option("coop_mgs", coop_mgs)
    ctx.set_option("test_disable", test_disable)
    chain_before = ctx.counter("mgs_chain_steps")
    s, _, path = _solve(api, ctx, api.GmresSolver, mat, b_h, num_inner_iterations=m)
    # the fused GMRES loop (solver_gmres.hip) counts no solve path; its chain steps tell the two Gram-Schmidt forms apart
    assert path == {k: 0 for k in PATHS}, path
    assert ctx.counter("mgs_chain_steps") - chain_before == coop_mgs
    assert s.history[0] == fs.h0
    assert er.close(s.history[1], fs.gmres_h1, fs.gmres_tol), (s.history[1], fs.gmres_h1)
    ctx.set_option("generic_solvers", 1)
    s, _, path = _solve(api, ctx, api.GmresSolver, mat, b_h, num_inner_iterations=m)
    _only(path, "engine_solves")
    assert s.history[0] == fs.h0
    assert er.close(s.history[1], fs.gmres_h1, fs.gmres_tol), (s.history[1], fs.gmres_h1)
    mat.close()


# ---- the engine's other methods -------------------------------------------------------------------------------------------
#
# CGS, TFQMR, TFQMR1, Richardson, BiCGStab(l), IDR(s) (krylov_methods.hip) and the preconditioned engine solves against the
# coefficient-form restatement of the reference's headers (tests/exact_ref.py, ``Pins``): history[0] bitwise wherever
# r0 is b, Richardson (omega = 2^-5) bitwise in x_k and history[1], history[1] of the rest by the floor rule or the
# closed forms, every later or preconditioned entry within max(floor, 16 e_k) of the exact value, e_k the oracle's own
# distance from it.  Each case prints |h - exact| / (exact e_k) per entry ("ratio" lines).

CLASSES = {"cgs": "CgsSolver", "tfqmr": "TfqmrSolver", "tfqmr1": "Tfqmr1Solver", "richardson": "RichardsonSolver",
           "bicgstabl": "BiCgStabLSolver", "idrs": "IdrsSolver", "cg": "CgSolver", "fgmres": "FgmresSolver"}
ENGINE_METHODS = [("cgs", None), ("tfqmr", None), ("tfqmr1", None), ("richardson", None), ("bicgstabl", 1),
                  ("bicgstabl", 2), ("bicgstabl", 3), ("idrs", 1), ("idrs", 2), ("idrs", 4)]
# each format once with the defaults, each engine option once against the lattice format; the non-temporal instances of
# the engine's statement kernels (blas1_nt 2: krylov_device.hpp lin_kernel, lin2_kernel, the lin_dot / pre_dots bodies), fused
# and statement by statement
ENGINE_CONFIGS = [("lattice", {}), ("lattice8", {}), ("fp64", {}), ("tail", {}), ("lattice", {"fused_reduce": 0}),
                  ("lattice", {"lin_fuse": 0}), ("lattice", {"ticket_reduce": 0}), ("lattice", {"blas1_nt": 2}),
                  ("fp64", {"blas1_nt": 2, "lin_fuse": 0})]

_bases, _pins_cache = {}, {}


def _method_id(m):
    return m[0] + ("" if m[1] is None else str(m[1]))


def _pins(mesh, shape, kind, param, side=None):
    from oracle import oracle

    key = (shape, kind, param, side)
    if key not in _pins_cache:
        g, b_h, fs = _problem(mesh, shape)
        bkey = (shape, side is not None)
        if bkey not in _bases:
            _bases[bkey] = er.Basis(shape, b_h, 1.0 / er.int_diagonal(shape) if side is not None else None)
        _pins_cache[key] = er.Pins(oracle, g, shape, b_h, kind, param, side, fs=fs, basis=_bases[bkey])
    return _pins_cache[key]


def _knobs(kind, param):
    if kind in ("bicgstabl", "idrs", "fgmres"):
        return {"num_inner_iterations": param}
    if kind == "richardson":
        return {"relaxation_factor": float(er.OMEGA)}
    return {}


def _report(label, pins, ratios):
    print(f"ratio {label}: " + " ".join(f"{r:.2f}" for r in ratios) + "   tol " +
          " ".join("bitwise" if t is None else f"{t:.1e}" for t in pins.tol))


@pytest.mark.parametrize("shape", [SMALL, ODD], ids=["small", "odd"])
@pytest.mark.parametrize("case", ENGINE_CONFIGS, ids=lambda c: c[0] + "".join(f"-{k}{v}" for k, v in c[1].items()))
@pytest.mark.parametrize("method", ENGINE_METHODS, ids=_method_id)
def test_engine_methods_against_the_exact_reference(env, method, case, shape):
    """history[0..K] of every engine method pinned (K from er.iterations), plus: Richardson's x_k bitwise for
    k = 1 ... 4 and its history[1] bitwise; BiCGStab(l >= 2)'s x after one iteration is CG's x1, bitwise."""
    api, mesh, ctx = env
    kind, param = method
    fmt, opts = case
    g, b_h, fs = _problem(mesh, shape)
    pins = _pins(mesh, shape, kind, param)
    mat = _matrix(api, ctx, g, fmt)
    for k, v in opts.items():
        ctx.set_option(k, v)
    cls = getattr(api, CLASSES[kind])
    label = f"{_method_id(method)} {fmt} {opts} {shape}"
    api.rng_reset()
    s, x, path = _solve(api, ctx, cls, mat, b_h, iters=pins.K, **_knobs(kind, param))
    _only(path, "engine_solves")
    _check_access_mode(s, opts, g.n_cells)
    assert s.history[0] == fs.h0
    _report(label, pins, pins.check(s.history, label))
    if kind == "bicgstabl" and param >= 2:
        s, x, _ = _solve(api, ctx, cls, mat, b_h, iters=1, **_knobs(kind, param))
        assert np.array_equal(x, fs.cg_x1(b_h)), f"x1: {np.count_nonzero(x != fs.cg_x1(b_h))} elements differ"
    if kind == "richardson":
        for k in range(1, 5):
            X, _ = er.richardson_integers(shape, b_h, k)
            s, x, path = _solve(api, ctx, cls, mat, b_h, iters=k, **_knobs(kind, param))
            _only(path, "engine_solves")
            want = X / 32.0 ** k  # exact: |X| < 2^53
            assert np.array_equal(x, want), f"x_{k}: {np.count_nonzero(x != want)} elements differ"
            if k == 1:
                assert s.history[1] == er.richardson_h1(shape, b_h), (s.history[1], er.richardson_h1(shape, b_h))
    mat.close()


@pytest.mark.parametrize("method", [("cgs", None), ("bicgstabl", 2)], ids=_method_id)
def test_engine_methods_many_partials(env, method):
    """256 x 256 x 258: more partials than one pass folds, in every engine reduction.  (The reference's chain of
    this box is not kept beyond the test: about 1 GB.)"""
    from oracle import oracle

    api, mesh, ctx = env
    kind, param = method
    g, b_h, fs = _problem(mesh, BIG)
    pins = er.Pins(oracle, g, BIG, b_h, kind, param, fs=fs)
    mat = _matrix(api, ctx, g, "lattice")
    s, x, path = _solve(api, ctx, getattr(api, CLASSES[kind]), mat, b_h, iters=pins.K, **_knobs(kind, param))
    _only(path, "engine_solves")
    label = f"{_method_id(method)} lattice BIG"
    _report(label, pins, pins.check(s.history, label))
    mat.close()


JACOBI_METHODS = [("cg", None), ("cgs", None), ("tfqmr", None), ("idrs", 2), ("fgmres", 1), ("fgmres", 30),
                  ("richardson", None), ("bicgstabl", 2)]
# the side the reference applies the preconditioner on whatever pre_side says: Richardson (SolverRichardson.hpp:66-69,
# :90-93) and BiCGStab(l) (SolverBiCgStab.hpp:226-229) always on the left, FGMRES (SolverGmres.hpp:125-130) always on
# the right; CG (SolverCg.hpp:74-77) has no side
FIXED_SIDE = {"richardson": "left", "bicgstabl": "left", "fgmres": "right"}


def _jacobi_case(env, shape, method, side, lin_fuse, blas1_nt=1):
    api, mesh, ctx = env
    kind, param = method
    g, b_h, fs = _problem(mesh, shape)
    mat = _matrix(api, ctx, g, "lattice")
    d = api.DeviceVector(ctx, g.n_cells)
    mat.diagonal(-1.0, 0.0, d, invert=True)
    assert np.array_equal(d.to_numpy(), 1.0 / er.int_diagonal(shape))  # the dinv the reference is restated with
    pins = _pins(mesh, shape, kind, param, FIXED_SIDE.get(kind, side))
    if kind == "cg":
        ctx.set_option("generic_solvers", 1)
    ctx.set_option("lin_fuse", lin_fuse)
    ctx.set_option("blas1_nt", blas1_nt)
    knobs = dict(_knobs(kind, param), pre_op=api.JacobiPreconditioner(),
                 pre_side=api.PreconditionerSide.Left if side == "left" else api.PreconditionerSide.Right)
    api.rng_reset()
    s, _, path = _solve(api, ctx, getattr(api, CLASSES[kind]), mat, b_h, iters=pins.K, **knobs)
    _only(path, "engine_solves")
    _check_access_mode(s, {"blas1_nt": blas1_nt}, g.n_cells)
    label = f"{_method_id(method)} jacobi-{side} lin_fuse{lin_fuse} blas1_nt{blas1_nt} {shape}"
    _report(label, pins, pins.check(s.history, label))
    mat.close()


@pytest.mark.parametrize("lin_fuse", [1, 0])
@pytest.mark.parametrize("side", ["left", "right"])
@pytest.mark.parametrize("method", JACOBI_METHODS, ids=_method_id)
@pytest.mark.parametrize("shape", [SMALL, ODD], ids=["small", "odd"])
def test_engine_methods_with_jacobi(env, shape, method, side, lin_fuse):
    """api.JacobiPreconditioner on either side, lin_fuse on and off (for CG it switches the fused pre_dots pass,
    z = P r with <r,z> and <r,r>): history[0..2] against the reference restated with P = diag(fl(1/d))."""
    _jacobi_case(env, shape, method, side, lin_fuse)


@pytest.mark.parametrize("lin_fuse", [1, 0])
@pytest.mark.parametrize("method", JACOBI_METHODS, ids=_method_id)
@pytest.mark.parametrize("shape", [SMALL, ODD], ids=["small", "odd"])
def test_engine_methods_with_jacobi_non_temporal(env, shape, method, lin_fuse):
    """The same pins with every streaming launch of the solve on its non-temporal instance (blas1_nt 2), side left."""
    _jacobi_case(env, shape, method, "left", lin_fuse, blas1_nt=2)


@pytest.mark.parametrize("cls", ["CgsSolver", "TfqmrSolver", "Tfqmr1Solver", "IdrsSolver", "BiCgStabLSolver"])
def test_engine_methods_initial_residual(env, cls):
    api, mesh, ctx = env
    g, b_h, fs = _problem(mesh, SMALL)
    mat = _matrix(api, ctx, g, "lattice")
    api.rng_reset()
    s, _, path = _solve(api, ctx, getattr(api, cls), mat, b_h)
    _only(path, "engine_solves")
    assert s.history[0] == fs.h0
    mat.close()


# ---- a size-1 RCCL communicator ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fused", [1, 2])
def test_cg_first_step_over_rccl(fused):
    """The same pins through the RCCL transport: every sum goes through the library all-reduce, whose order is
    irrelevant on exact integers.  rccl_fused 1 + rccl_ticket 1: the rtick branch -- <p,z> by
    reduce_stage1_ticket_kernel<1> and the all-reduce, <r,r> by tickets in cg_r_kernel, then step_kernel; 2: the
    fused step with partials and the RCCL form of k_reduce_finish (launch, all-reduce, step).  (rccl_fused = 0 only
    acts on an operator with a halo, spmv.hip: on this one it is the same loop as 2.)"""
    from stormruler_amd import api, mesh

    g, b_h, fs = _problem(mesh, SMALL)
    ctx = api.Context(0)
    try:
        ctx.set_option("spmv_canon_tile_min_rows", 0)
        ctx.set_option("rccl_fused", min(fused, 1))
        ctx.set_option("rccl_ticket", int(fused == 1))
        ctx.comm_init(api.Context.comm_unique_id(), 1, 0)
        mat = _matrix(api, ctx, g, "lattice")
        s, x, path = _solve(api, ctx, api.CgSolver, mat, b_h)
        _only(path, "throughput_solves", 1)
        _check_cg(api, s, x, fs, b_h)
        s, _, path = _solve(api, ctx, api.BiCgStabSolver, mat, b_h)
        assert s.history[0] == fs.h0
        assert er.close(s.history[1], fs.bicgstab_h1, fs.bicgstab_tol), (s.history[1], fs.bicgstab_h1)
        s, _, path = _solve(api, ctx, api.GmresSolver, mat, b_h, num_inner_iterations=30)
        assert s.history[0] == fs.h0
        assert er.close(s.history[1], fs.gmres_h1, fs.gmres_tol), (s.history[1], fs.gmres_h1)
        for kind, param in (("cgs", None), ("idrs", 2)):  # the engine's methods, every sum through the all-reduce
            pins = _pins(mesh, SMALL, kind, param)
            api.rng_reset()
            s, _, path = _solve(api, ctx, getattr(api, CLASSES[kind]), mat, b_h, iters=pins.K, **_knobs(kind, param))
            _only(path, "engine_solves")
            pins.check(s.history, f"{kind} rccl_fused {fused}")
        mat.close()
    finally:
        ctx.close()
