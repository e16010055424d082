"""The RCCL transport while it carries a halo, pinned to exact references on integer data (tests/exact_ref.py:
``periodic_box``, ``StepPins``, ``GmresPins``).

One process, an RCCL communicator of size 1 and a box that is periodic in z, the rank its own neighbour
(tests/test_gpu_comm.py): the pack kernels, grouped send / recv on the comm stream, the interior / boundary split of the
apply, the hand-off flag and the all-reduce of every sum all run.  At unit spacing every coefficient is an integer --
-L with diagonal 6 ... 8 and off-diagonals -1, and first-order upwind convection-diffusion with nu = 1, v = (2, 1, -1) --
so the apply and the sums are held to the bit, and CG (K = 8), BiCGStab (K = 5) and GMRES(m) ((K, m) = (12, 5), (9, 9))
to the exact history[0..K] and x_K of Fractions / 80-digit decimals over the integer Krylov chain.

What only shows from the second iteration on, because at step 0 p = r: halo_pack_direction_kernel (p' = r + beta p with
the beta of the slab), halo_pack_bicg_kernel<0> (s = r - alpha v, alpha formed in the kernel) and <1>, <2> (p' from beta
and omega), a boundary launch that did not wait for the exchange, a halo packed one statement early.  Each would change
two planes of one operand; tests/test_exact_reference.py shows that such a defect leaves the pins by a factor of 1e8 or
more (``test_halo_defects_fall_outside_the_periodic_pins``), where a comparison of two variants that share it, or of a
converged solution with the oracle's, sees nothing.

Boxes: G = 20 x 12 x 9 gets general records; on L = 32 x 32 x 24 and L2 = 64 x 16 x 40 the interior planes get lattice
records (option spmv_mixed) and CG its fused step.  Every solve: tolerances 0, exactly K iterations, record_history; no
fallback; the kernel-per-launch loop and no other path; history[0] bitwise, history[k] within tol_k = max(floor_k, 16 e_k) <= 1e-10, ||b - A x|| in
long double by the same rule, on G also x against the exact x_k.  Each case prints its largest |h - exact| / exact
("rccl" lines)."""
import math
import os
import sys

import numpy as np
import pytest

import exact_ref as er

pytestmark = pytest.mark.gpu

G, L, L2 = er.PERIODIC_G, er.PERIODIC_L, er.PERIODIC_L2
LATTICE = (L, L2)
DEFAULTS = (("rccl_fused", 1), ("rccl_ticket", 1), ("rccl_early_halo", 1), ("rccl_flag_wait", 1), ("ticket_verify", 0),
            ("mgs_steps", 4), ("spmv_dict", 4), ("spmv_mixed", 1))
PATHS = ("resident_solves", "latency_solves", "throughput_solves", "engine_solves")
MGS_COUNTERS = ("mgs_chain_steps", "mgs_quad_steps", "mgs_lds_steps")


def _plain_options():
    """bench.RCCL_PLAIN_OPTIONS: the switches the benchmark's rccl-plain fallback turns off together (read, not copied)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    import bench

    return {key: 0 for key in bench.RCCL_PLAIN_OPTIONS}


@pytest.fixture(scope="module")
def env():
    from oracle import oracle
    from stormruler_amd import api, mesh

    ctx = api.Context(0)
    ctx.comm_init(api.Context.comm_unique_id(), 1, 0)
    ctx.set_option("spmv_canon_tile_min_rows", 0)  # (the lattice kernels on slabs this small)
    yield api, mesh, oracle, ctx
    for mat in _matrices.values():
        mat.close()
    _matrices.clear(), _steps.clear(), _gmres.clear()
    ctx.close()


_steps, _gmres, _matrices = {}, {}, {}


def _step_problem(env, shape, kind):
    """The box, its chain and its pins: built once per (shape, kind) and kept for the module."""
    _, mesh, oracle, _ = env
    if (shape, kind) not in _steps:
        _steps[shape, kind] = er.StepProblem(oracle, mesh, shape, kind)
    return _steps[shape, kind]


def _gmres_problem(env, shape):
    _, mesh, oracle, _ = env
    assert shape in er.PERIODIC_GMRES_CASES
    if shape not in _gmres:
        _gmres[shape] = er.GmresProblem(oracle, mesh, shape, "periodic_convdiff")
    return _gmres[shape]


def _matrix(env, p, dict_=4, mixed=1):
    """The device operator of a problem with its halo plan: -L from the mesh quantities (apply with alpha = -1), the
    convection-diffusion operator from its face weights (alpha = 1).  spmv_dict and spmv_mixed are read when the
    operator is built."""
    api, _, _, ctx = env
    key = (p.shape, p.kind, dict_, mixed)
    if key not in _matrices:
        g = p.g
        try:
            ctx.set_option("spmv_dict", dict_)
            ctx.set_option("spmv_mixed", mixed)
            if p.kind == "periodic":
                mat = api.StencilMatrix.from_face_graph(ctx, g)
            else:
                mat = api.StencilMatrix.from_face_weights(ctx, g.n_cells, g.n_halo, g.inner, g.outer, *p.weights)
        finally:
            ctx.set_option("spmv_dict", 4)
            ctx.set_option("spmv_mixed", 1)
        mat.set_halo([0], [0, g.n_halo], p.send_idx, [0, g.n_halo])
        st = mat.stats()
        assert st["tail_rows"] == 0 and 0 < st["n_interior_slices"] < st["n_slices"]  # an interior / boundary split
        _matrices[key] = mat
    return _matrices[key]


def _alpha(p):
    return -1.0 if p.kind == "periodic" else 1.0


def _sid(shape):
    return "x".join(map(str, shape))


class _Options:
    """Options for the length of a ``with`` block; the defaults come back whatever happens inside."""

    def __init__(self, ctx, opts):
        self.ctx, self.opts = ctx, opts

    def __enter__(self):
        try:
            for k, v in self.opts.items():
                self.ctx.set_option(k, v)
        except BaseException:
            self.__exit__()
            raise

    def __exit__(self, *exc):
        for k, v in DEFAULTS:
            self.ctx.set_option(k, v)


def _solve(env, cls, mat, p, iters, stop=0.0, **knobs):
    """One solve from x0 = 0: exactly what the options ask, counted."""
    api, _, _, ctx = env
    g = p.g
    s = cls()
    s.num_iterations, s.absolute_error_tolerance, s.relative_error_tolerance, s.record_history = iters, stop, 0.0, True
    for k, v in knobs.items():
        setattr(s, k, v)
    b = api.DeviceVector.from_numpy(ctx, p.b.astype(np.float64), n_halo=g.n_halo)
    x = api.DeviceVector.from_numpy(ctx, np.zeros(g.n_cells), n_halo=g.n_halo)
    names = PATHS + ("cg_fused_steps",) + MGS_COUNTERS
    before = {k: ctx.counter(k) for k in names}
    s.solve(x, b, api.HipStencilOperator(mat, _alpha(p), 0.0))
    moved = {k: ctx.counter(k) - before[k] for k in names}
    assert s.path_fallback == 0
    # CG and BiCGStab count their kernel-per-launch loop; GMRES's own loop (solver_gmres.hip) has no counter: for it
    # the assertion is that no other path took the solve
    want = dict.fromkeys(PATHS, 0)
    want["throughput_solves"] = 0 if cls is api.GmresSolver else 1
    assert {k: moved[k] for k in PATHS} == want, moved
    return s, x.to_numpy(), moved


def _check_steps(pins, label, s, x, k=None):
    k = pins.K if k is None else k
    assert s.iteration == k and s.history.size == k + 1, (label, s.iteration, s.history.size)
    far = pins.check(list(s.history), label, k)
    xr = pins.check_x(x, k, label)
    t = pins.x_tolerances(k)
    print(f"rccl {label}: far {max(far):.1e} at {int(np.argmax(far))}   x " + " ".join(f"{v:.1e}" for v in xr) +
          f"   largest tol_k {max(pins.tol[1:k + 1]):.1e}   tol_res {t[1]:.1e}/{t[2]}" + ("" if t[4] is None else f" tol_x {t[4]:.1e}"))


# ---- the apply and the sums ------------------------------------------------------------------------------------------------

APPLY = [(shape, kind, d, m) for shape in (G, L) for kind in er.PERIODIC_KINDS for d in (4, 0) for m in (1, 0)]


@pytest.mark.parametrize("case", APPLY, ids=lambda c: f"{_sid(c[0])}-{c[1]}-dict{c[2]}-mixed{c[3]}")
def test_apply_and_sums_over_the_halo_are_exact(env, case):
    """The split apply with its exchange, three times in a row (the events, the flag and the streams must hold across
    applies), with the hand-off flag and with the cross-stream event: A b to the bit; an accumulate form with integer
    constants, 3 b + 2 M b; the halo tail of b holds the rows it was sent; <b, b>, <b, A b> and |b| through the size-1
    all-reduce are the exact integers and the correctly rounded root."""
    api, _, _, ctx = env
    shape, kind, dict_, mixed = case
    p = _step_problem(env, shape, kind)
    g, n = p.g, p.g.n_cells
    mat = _matrix(env, p, dict_, mixed)
    st = mat.stats()
    if dict_ == 0:
        assert st["value_dictionary_size"] == 0
    zi = p.A.apply(p.b)
    a = int(_alpha(p))
    acc = 3 * p.b + 2 * a * zi  # 3 b + 2 M b, M = a A
    assert int(np.abs(acc).max()) < er.EXACT
    rr, pz = er.exact_dot(p.b, p.b), er.exact_dot(p.b, zi)
    for flag in (1, 0):
        with _Options(ctx, {"rccl_flag_wait": flag}):
            b = api.DeviceVector.from_numpy(ctx, p.b.astype(np.float64), n_halo=g.n_halo)
            z = api.DeviceVector(ctx, n, g.n_halo)
            y = api.DeviceVector(ctx, n, g.n_halo)
            for _ in range(3):
                mat.apply(float(a), 0.0, b, z)
            mat.apply(2.0, 3.0, b, y)
            label = f"{case} flag {flag}"
            assert np.array_equal(z.to_numpy(), zi.astype(np.float64)), f"{label}: {np.count_nonzero(z.to_numpy() != zi)} rows of A b differ"
            assert np.array_equal(y.to_numpy(), acc.astype(np.float64)), f"{label}: {np.count_nonzero(y.to_numpy() != acc)} rows of 3 b + 2 M b differ"
            assert np.array_equal(b.to_numpy(with_halo=True)[n:], p.b[p.send_idx].astype(np.float64)), label
            assert api.dot_product(b, b) == float(rr) and api.dot_product(b, z) == float(pz), label
            assert api.norm_2(b) == math.sqrt(float(rr)), label


# ---- CG -----------------------------------------------------------------------------------------------------------------------

# name: (options, does a lattice box run the fused step)
CG_ROADS = {
    "fused-tickets": ({"rccl_fused": 1, "rccl_ticket": 1}, True),  # halo_pack_direction_kernel; the local sums by tickets
    "fused-partials": ({"rccl_fused": 1, "rccl_ticket": 0}, True),  # ... by partials and a final pass
    "statements-early": ({"rccl_fused": 0, "rccl_ticket": 1, "rccl_early_halo": 1}, False),  # halo_pack_bicg_kernel<2>
    "statements-late": ({"rccl_fused": 0, "rccl_early_halo": 0}, False),  # the apply begins the exchange itself
    "plain": (None, False),  # bench.RCCL_PLAIN_OPTIONS, all at once
    "fused-verify": ({"ticket_verify": 1}, True),  # every iteration's ticketed sums recomputed on the device
}
CG_CASES = [(shape, road, 1) for shape in (G, L, L2) for road in CG_ROADS] + [(L, road, 0) for road in CG_ROADS if road != "plain"]


def _road_options(opts, flag):
    """The options of a road (None: the plain combination) with the hand-off flag or the event."""
    opts = dict(_plain_options() if opts is None else opts)
    opts.setdefault("rccl_flag_wait", flag)
    return opts


@pytest.mark.parametrize("case", CG_CASES, ids=lambda c: f"{_sid(c[0])}-{c[1]}-flag{c[2]}")
def test_cg_steps_over_the_halo(env, case):
    """8 iterations on periodic Poisson: history[0..8] and x_8; a solve stopped at iteration 3 by an absolute tolerance
    between the exact history[2] and history[3], with x_3 (the x update behind the loop's last iteration belongs to the
    iteration that ran); and a second solve on the same solver, operator and context with the same bits."""
    api, _, _, ctx = env
    shape, road, flag = case
    p = _step_problem(env, shape, "periodic")
    pins = p.pins("cg")
    mat = _matrix(env, p)
    fused = CG_ROADS[road][1] and shape in LATTICE
    label = f"cg {_sid(shape)} {road} flag{flag}"
    with _Options(ctx, _road_options(CG_ROADS[road][0], flag)):
        s, x, moved = _solve(env, api.CgSolver, mat, p, pins.K)
        assert (moved["cg_fused_steps"] >= 1) == fused and (fused or moved["cg_fused_steps"] == 0), (label, moved)
        _check_steps(pins, label, s, x)
        s3, x3, moved3 = _solve(env, api.CgSolver, mat, p, pins.K, stop=pins.stop_between(er.STEP_STOP))
        assert (moved3["cg_fused_steps"] >= 1) == fused, (label, moved3)
        _check_steps(pins, label + f" stop{er.STEP_STOP}", s3, x3, er.STEP_STOP)
        again, x_again, _ = _solve(env, api.CgSolver, mat, p, pins.K)
        assert np.array_equal(again.history, s.history) and np.array_equal(x_again, x), label


# ---- BiCGStab ---------------------------------------------------------------------------------------------------------------

BICG_ROADS = {
    "early-tickets": {"rccl_early_halo": 1, "rccl_ticket": 1},  # halo_pack_bicg_kernel<0> for s, <1> for p'
    "early-partials": {"rccl_early_halo": 1, "rccl_ticket": 0},
    "late-tickets": {"rccl_early_halo": 0, "rccl_ticket": 1},
    "late-partials": {"rccl_early_halo": 0, "rccl_ticket": 0},
    "verify": {"ticket_verify": 1},  # ... and the alpha the early halo of s was formed with must be the update kernel's
    "plain": None,
}
BICG_CASES = [(shape, kind, road) for kind in er.PERIODIC_KINDS for shape in (G, L) for road in BICG_ROADS]
assert all((c[0], c[1]) in er.PERIODIC_STEP_CASES["bicgstab"] for c in BICG_CASES)
assert all((c[0], "periodic") in er.PERIODIC_STEP_CASES["cg"] for c in CG_CASES)


@pytest.mark.parametrize("case", BICG_CASES, ids=lambda c: f"{_sid(c[0])}-{c[1]}-{c[2]}")
def test_bicgstab_steps_over_the_halo(env, case):
    """5 iterations on periodic Poisson and on periodic convection-diffusion (A != A^T: a swapped r~ and r shows):
    history[0..5], x_5, and the solve stopped at iteration 3 with x_3."""
    api, _, _, ctx = env
    shape, kind, road = case
    p = _step_problem(env, shape, kind)
    pins = p.pins("bicgstab")
    mat = _matrix(env, p)
    label = f"bicgstab {_sid(shape)} {kind} {road}"
    with _Options(ctx, _road_options(BICG_ROADS[road], 1)):
        s, x, _ = _solve(env, api.BiCgStabSolver, mat, p, pins.K)
        _check_steps(pins, label, s, x)
        s3, x3, _ = _solve(env, api.BiCgStabSolver, mat, p, pins.K, stop=pins.stop_between(er.STEP_STOP))
        _check_steps(pins, label + f" stop{er.STEP_STOP}", s3, x3, er.STEP_STOP)


# ---- GMRES ----------------------------------------------------------------------------------------------------------------------

GMRES_CASES = [(shape, K, m, gs, steps) for shape, runs in er.PERIODIC_GMRES_CASES.items() for K, m in runs
               for gs in (0, 1) for steps in (2, 4)]


@pytest.mark.parametrize("case", GMRES_CASES, ids=lambda c: f"{_sid(c[0])}-K{c[1]}m{c[2]}-gs{c[3]}-steps{c[4]}")
def test_gmres_over_the_halo(env, case):
    """GMRES(m) on periodic convection-diffusion, with the hand-off flag and with the event: modified Gram-Schmidt
    (gram_schmidt 0) and classical Gram-Schmidt applied twice (1: two multi-dots and multi-axpys per step and
    gmres_cgs2_combine_kernel) -- in exact arithmetic the same iteration, so the same pins.  With a communicator every
    projection is a sum that goes through the all-reduce: neither the cooperative chains nor the ticketed pair /
    multi-step kernels run (the counters say so, whatever mgs_steps asks for)."""
    api, _, _, ctx = env
    shape, K, m, gs, steps = case
    p = _gmres_problem(env, shape)
    pins = p.pins(K, m)
    assert (pins.x is not None) == (shape == G)
    mat = _matrix(env, p)
    for flag in (1, 0):
        label = f"gmres({m}) K{K} {_sid(shape)} gs{gs} steps{steps} flag{flag}"
        with _Options(ctx, {"mgs_steps": steps, "rccl_flag_wait": flag}):
            s, x, moved = _solve(env, api.GmresSolver, mat, p, K, num_inner_iterations=m, gram_schmidt=gs)
        assert s.iteration == K and s.history.size == K + 1, (label, s.iteration)
        assert {k: moved[k] for k in MGS_COUNTERS} == {k: 0 for k in MGS_COUNTERS}, (label, moved)
        ratios = pins.check(list(s.history), label)
        xr = pins.check_x(x, label)
        far = max(abs(h - e) / e for h, e in zip(s.history, pins.exact))
        print(f"rccl {label}: far {far:.1e}   |h - exact| / (exact e_k) " + " ".join(f"{r:.1e}" for r in ratios) + "   x " +
              " ".join(f"{r:.1e}" for r in xr) + f"   largest tol_k {max(pins.tol[1:]):.1e}   tol_res {pins.tol_res:.1e}/{pins.rule_res}   " +
              "chain counters " + " ".join(f"{k} {moved[k]}" for k in MGS_COUNTERS))
