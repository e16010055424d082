"""The cooperative tail of the multigrid cycle (option amg_tail, csrc/amg_tail.hip): from a level t down to the coarsest level
and back, one kernel runs what the cycle otherwise enqueues as launches.  Every comparison here is BITWISE (np.array_equal on
the uint64 view): the tail kernel sends each row through the device functions the launched kernels call (csrc/amg_device.hpp).

1. tail against launches for every start level (amg_tail_rows swept over the level sizes of the 13^3 box, 2197 / 280 / 16);
2. full slices (12^3 = 27 x 64 rows, lognormal weights), irregular rows (the random symmetric CSR), a Triangle mesh;
3. Chebyshev degree 1, 2, 3 and Jacobi with 1, 2, 3 sweeps, each on fp64 and on reduced records;
4. a null-space object (level 0 stays launches) and a refreshable object after a refresh;
5. CG + multigrid and GMRES(30) + Jacobi-multigrid: iterations, history and x;
6. a refused launch (coop_force_fail = 1) and a give-up (coop_force_fail = 2, the test hook: nothing is made to hang);
7. applies back to back, and an apply after a GMRES solve that ran the cooperative Gram-Schmidt chains (sequence numbers);
8. applies enqueued past convergence (the engine runs ahead of the device's verdict): predicated off by the api_done word.

Test 5's count: the issue asks for amg_tail_applies == num_pre_applies.  The counter moves when an apply is ENQUEUED, and the
engine enqueues up to check_lag iterations past convergence (their kernels see api_done set), while num_pre_applies counts up
to the converged iteration.  So the equality is asserted on solves whose num_iterations is the converged count (nothing is
enqueued past it); on the open-ended solves the assertion is amg_tail_applies == amg_applies >= num_pre_applies."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import amg_cases  # noqa: E402
import amg_jacobi_ref  # noqa: E402
import amg_nullspace_ref  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 1 << 40  # an amg_tail_rows above every level


@pytest.fixture(scope="module")
def env():
    from stormruler_amd import api, mesh

    ctx = api.Context(0)
    yield api, mesh, ctx
    ctx.set_option("amg_tail", 0)
    ctx.close()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def rhs(n):
    """An unstructured right-hand side."""
    return np.sin(0.37 * np.arange(n)) + np.random.default_rng(5).standard_normal(n)


def fp64_matrix(ctx, build, *args, ell_cap=0):
    """A StencilMatrix on fp64 records (spmv_dict = 0), options restored afterwards."""
    ctx.set_option("spmv_dict", 0)
    ctx.set_option("ell_cap", ell_cap)
    try:
        return build(ctx, *args)
    finally:
        ctx.set_option("spmv_dict", 4)
        ctx.set_option("ell_cap", 0)


def build(env, mat, alpha, beta, **params):
    api, mesh, ctx = env
    pre = api.AmgPreconditioner(**params)
    x = api.DeviceVector(ctx, mat.stats()["n_rows"])
    pre.build(x, x, api.HipStencilOperator(mat, alpha, beta))
    return pre


def apply(env, pre, r_host, tail, rows=BIG):
    """z = B r with the tail on or off; (z, tail applies, tail refusals)."""
    api, mesh, ctx = env
    ctx.set_option("amg_tail", tail)
    ctx.set_option("amg_tail_rows", rows)
    try:
        r, z = api.DeviceVector.from_numpy(ctx, r_host), api.DeviceVector(ctx, r_host.size)
        z.upload(np.full(r_host.size, np.nan))  # (the cycle must not read z)
        before = ctx.counter("amg_tail_applies"), ctx.counter("amg_tail_refusals")
        pre.mul(z, r)
        ctx.sync()
        assert np.array_equal(r.to_numpy(), r_host)  # r is not written
        return z.to_numpy(), ctx.counter("amg_tail_applies") - before[0], ctx.counter("amg_tail_refusals") - before[1]
    finally:
        ctx.set_option("amg_tail", 0)


def check_tail_equals_launches(env, pre, n, want_level=None):
    """The whole eligible hierarchy as one kernel against the launches; returns the start level."""
    api, mesh, ctx = env
    r_host = rhs(n)
    want, took, _ = apply(env, pre, r_host, 0)
    assert took == 0 and np.isfinite(want).all()
    ctx.set_option("amg_tail_rows", BIG)
    level = int(pre.get("tail_level"))
    if want_level is not None:
        assert level == want_level
    got, took, refused = apply(env, pre, r_host, 1)
    assert (took, refused) == (1, 0)
    assert pre.get("tail_blocks") >= 1 and pre.get("tail_barriers") >= 3
    assert same_bits(got, want)
    return level


# ---- 1. every start level ---------------------------------------------------------------------------------------------------
def test_tail_equals_launches_from_every_start_level(env):
    api, mesh, ctx = env
    a = amg_cases.poisson_box(13)
    mat = fp64_matrix(ctx, api.StencilMatrix.from_csr, a)
    pre = build(env, mat, 1.0, 0.0, coarse_rows=32)
    assert pre.hierarchy.level_rows() == [2197, 280, 16]  # a partial last slice; fewer slices than waves below
    r_host = rhs(2197)
    want, took, _ = apply(env, pre, r_host, 0)
    assert took == 0
    for rows, level, runs in ((16, 2, False), (280, 1, True), (2197, 0, True), (15, -1, False)):
        got, took, refused = apply(env, pre, r_host, 1, rows)
        ctx.set_option("amg_tail_rows", rows)
        assert pre.get("tail_level") == level, rows
        assert (took, refused) == (int(runs), 0), rows  # (the coarsest level alone is not a tail)
        assert (pre.get("tail_blocks") >= 1) == runs and (pre.get("tail_barriers") >= 3) == runs
        assert same_bits(got, want), rows
    # level 0 in the tail: 35 slices on 16 waves per block -- three blocks; level 1 alone: one
    ctx.set_option("amg_tail_rows", 2197)
    assert pre.get("tail_blocks") == 3
    ctx.set_option("amg_tail_rows", 280)
    assert pre.get("tail_blocks") == 1
    pre.close()
    mat.close()


# ---- 2. full slices, irregular rows, a Triangle mesh --------------------------------------------------------------------------
def test_full_slices_with_lognormal_weights(env):
    api, mesh, ctx = env
    g, w, de, a = amg_cases.face_weight_case(mesh, 12, "lognormal")
    assert g.n_cells == 27 * 64
    mat = fp64_matrix(ctx, api.StencilMatrix.from_face_weights, g.n_cells, 0, g.inner, g.outer, w, w, de)
    pre = build(env, mat, -1.0, 0.0, coarse_rows=32)
    assert pre.get("levels") >= 3
    check_tail_equals_launches(env, pre, g.n_cells, want_level=0)
    pre.close()
    mat.close()


@pytest.mark.parametrize("ell_cap", [0, 4])
def test_irregular_rows_and_a_level_with_a_csr_tail(env, ell_cap):
    """The random symmetric operator (918 rows, non-uniform widths).  With ell_cap = 4 level 0 keeps a CSR tail, which the
    fused kernels do not take: the tail starts at level 1."""
    api, mesh, ctx = env
    a = amg_cases.random_symmetric(3)
    assert a.shape[0] == 918
    mat = fp64_matrix(ctx, api.StencilMatrix.from_csr, a, ell_cap=ell_cap)
    st = mat.stats()
    assert st["tail_rows"] > 0 or ell_cap == 0
    pre = build(env, mat, 1.0, 0.0, coarse_rows=32)
    assert pre.get("levels") >= 3
    level = check_tail_equals_launches(env, pre, 918)
    assert level == (1 if st["tail_rows"] > 0 else 0)
    pre.close()
    mat.close()


def test_triangle_mesh(env):
    api, mesh, ctx = env
    from stormruler_amd import io_tetgen

    tri = io_tetgen.read_triangle(os.path.join(ROOT, "tests", "golden", "mesh", "square_nb.1."))
    mat = fp64_matrix(ctx, api.StencilMatrix.from_face_graph, tri)
    pre = build(env, mat, -1.0, 1.0, coarse_rows=32)  # (I - L: definite whatever the mesh's boundary)
    print("square_nb.1 levels", pre.hierarchy.level_rows())
    assert pre.get("levels") >= 3
    check_tail_equals_launches(env, pre, tri.n_cells, want_level=0)
    pre.close()
    mat.close()


# ---- 3. smoothers and records -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def convdiff(env):
    """The upwind convection-diffusion box of the Jacobi smoother's tests: 13^3, non-symmetric, levels 2197 / 280 / 24."""
    api, mesh, ctx = env
    g, (wi, wo, de), a = amg_jacobi_ref.convdiff_box(mesh, 13)
    mat = fp64_matrix(ctx, api.StencilMatrix.from_face_weights, g.n_cells, 0, g.inner, g.outer, wi, wo, de)
    yield mat, g.n_cells
    mat.close()


@pytest.fixture(scope="module")
def box13(env):
    api, mesh, ctx = env
    mat = fp64_matrix(ctx, api.StencilMatrix.from_csr, amg_cases.poisson_box(13))
    yield mat
    mat.close()


@pytest.mark.parametrize("reduced", [0, 1])
@pytest.mark.parametrize("degree", [1, 2, 3])
def test_chebyshev_smoother(env, box13, degree, reduced):
    pre = build(env, box13, 1.0, 0.0, coarse_rows=32, smoother_degree=degree, reduced_records=reduced)
    assert pre.get("smoother_degree") == degree and pre.get("reduced") == reduced
    check_tail_equals_launches(env, pre, 2197, want_level=0)
    # per smoothed level: degree steps, the residual and a transfer on the way down, the same on the way up; one phase for
    # the top level's start, one for the dense inverse; a barrier between two phases
    assert pre.get("tail_barriers") == 2 * 2 * (degree + 2) + 1
    pre.close()


@pytest.mark.parametrize("reduced", [0, 1])
@pytest.mark.parametrize("sweeps", [1, 2, 3])
def test_jacobi_smoother(env, convdiff, sweeps, reduced):
    """Both parities of the buffer alternation (the iterate moves between z and e)."""
    mat, n = convdiff
    pre = build(env, mat, 1.0, 0.0, coarse_rows=32, smoother="jacobi", jacobi_sweeps=sweeps, reduced_records=reduced)
    assert pre.get("smoother_kind") == 1 and pre.get("jacobi_sweeps") == sweeps
    assert pre.hierarchy.level_rows() == [2197, 280, 24]
    check_tail_equals_launches(env, pre, n, want_level=0)
    assert pre.get("tail_barriers") == 2 * (2 * sweeps + 2) + 1  # (2 nu - 1 sweeps, residual, two transfers per level)
    pre.close()


# ---- 4. objects ---------------------------------------------------------------------------------------------------------------
def test_null_space_object_keeps_level_0_in_launches(env):
    api, mesh, ctx = env
    g, a = amg_nullspace_ref.neumann_box(mesh, 12, 10, 9)
    mat = fp64_matrix(ctx, api.StencilMatrix.from_face_graph, g)
    pre = build(env, mat, -1.0, 0.0, nullspace="constant", coarse_rows=16)
    assert pre.get("nullspace") == 1 and pre.get("levels") >= 3
    r_host = rhs(g.n_cells)
    keys = ("amg_projections", "amg_fused_projections")
    before = [ctx.counter(k) for k in keys]
    want, _, _ = apply(env, pre, r_host, 0)
    moved_off = [ctx.counter(k) - b for k, b in zip(keys, before)]
    before = [ctx.counter(k) for k in keys]
    got, took, refused = apply(env, pre, r_host, 1)
    moved_on = [ctx.counter(k) - b for k, b in zip(keys, before)]
    ctx.set_option("amg_tail_rows", BIG)
    assert pre.get("tail_level") == 1  # (never level 0: its projections and the closing sum stay launches)
    assert (took, refused) == (1, 0) and moved_on == moved_off == [2, 1]
    assert same_bits(got, want)
    pre.close()
    mat.close()


def test_refreshed_object(env):
    """The tail reads the refreshed numbers: records, scales, transfer weights, smoother coefficients, the dense inverse."""
    api, mesh, ctx = env
    g = mesh.structured_box(13)
    de = np.zeros(g.n_cells)
    np.add.at(de, g.b_cell, -2.0)
    w0 = np.ones(g.inner.size)
    mat = api.StencilMatrix.from_face_weights_updatable(ctx, g.n_cells, 0, g.inner, g.outer, w0, w0, de)
    pre = build(env, mat, -1.0, 0.0, refreshable=True, coarse_rows=32)
    r_host = rhs(g.n_cells)
    check_tail_equals_launches(env, pre, g.n_cells, want_level=0)  # (the tables are built: the refresh must drop them)
    first, _, _ = apply(env, pre, r_host, 1)
    w1 = np.exp(np.random.default_rng(12).standard_normal(g.inner.size))
    dv = api.DeviceVector.from_numpy
    mat.set_face_weights(dv(ctx, w1), dv(ctx, w1), dv(ctx, de))
    pre.refresh()
    want, _, _ = apply(env, pre, r_host, 0)
    got, took, refused = apply(env, pre, r_host, 1)
    assert (took, refused) == (1, 0)
    assert same_bits(got, want) and not same_bits(got, first)
    pre.close()
    mat.close()


# ---- 5. - 8. in a solve -------------------------------------------------------------------------------------------------------
def solve(env, solver, mat, alpha, beta, b_host, pre, tail, num_iterations=None):
    api, mesh, ctx = env
    ctx.set_option("amg_tail", tail)
    ctx.set_option("amg_tail_rows", BIG)
    try:
        b, x = api.DeviceVector.from_numpy(ctx, b_host), api.DeviceVector(ctx, b_host.size)
        solver.pre_op = pre
        solver.pre_side = api.PreconditionerSide.Right
        solver.record_history = True
        if num_iterations is not None:
            solver.num_iterations = num_iterations
        keys = ("amg_applies", "amg_tail_applies", "amg_tail_refusals")
        before = [ctx.counter(k) for k in keys]
        ok = solver.solve(x, b, api.HipStencilOperator(mat, alpha, beta))
        moved = dict(zip(keys, (ctx.counter(k) - v for k, v in zip(keys, before))))
        return dict(ok=ok, it=solver.iteration, x=x.to_numpy(), history=np.array(solver.history), pre_applies=solver.num_pre_applies,
                    fallback=solver.path_fallback, **moved)
    finally:
        ctx.set_option("amg_tail", 0)


def same_solve(got, want):
    return got["ok"] and want["ok"] and got["it"] == want["it"] and same_bits(got["history"], want["history"]) and \
        same_bits(got["x"], want["x"])


def solver_cases(env, box13, convdiff):
    api, mesh, ctx = env
    cd_mat, cd_n = convdiff

    def gmres():
        s = api.GmresSolver()
        s.num_inner_iterations = 30
        return s

    return {"cg": (api.CgSolver, box13, 2197, dict(coarse_rows=32)),
            "gmres": (gmres, cd_mat, cd_n, dict(coarse_rows=32, smoother="jacobi"))}


@pytest.mark.parametrize("name", ["cg", "gmres"])
def test_solves_are_bit_identical(env, box13, convdiff, name):
    api, mesh, ctx = env
    make, mat, n, params = solver_cases(env, box13, convdiff)[name]
    b_host = np.random.default_rng(8).standard_normal(n)
    pre = api.AmgPreconditioner(**params)
    off = solve(env, make(), mat, 1.0, 0.0, b_host, pre, 0)
    on = solve(env, make(), mat, 1.0, 0.0, b_host, pre, 1)
    print(name, {k: (off[k], on[k]) for k in ("it", "pre_applies", "amg_applies", "amg_tail_applies", "fallback")})
    assert off["amg_tail_applies"] == 0 and off["it"] > 0
    assert same_solve(on, off)
    assert on["fallback"] == off["fallback"] and on["amg_tail_refusals"] == 0
    # every apply took the tail.  8: the engine enqueues applies past the converged iteration; their kernels find api_done set
    # and store nothing -- x and the history above are those of the launches
    assert on["amg_tail_applies"] == on["amg_applies"] >= on["pre_applies"] > 0
    assert on["amg_applies"] > on["pre_applies"], "no apply was enqueued past convergence: the predicate was not exercised"
    # nothing enqueued past the last iteration: the count the issue asks for
    capped_off = solve(env, make(), mat, 1.0, 0.0, b_host, pre, 0, num_iterations=off["it"])
    capped = solve(env, make(), mat, 1.0, 0.0, b_host, pre, 1, num_iterations=off["it"])
    print(name, "capped", capped["it"], capped["pre_applies"], capped["amg_tail_applies"])
    assert same_solve(capped, capped_off) and same_bits(capped["x"], off["x"])
    assert capped["amg_tail_applies"] == capped["pre_applies"]
    pre.close()


def test_refused_launch_takes_the_launches(env, box13):
    api, mesh, ctx = env
    pre = build(env, box13, 1.0, 0.0, coarse_rows=32)
    r_host = rhs(2197)
    want, _, _ = apply(env, pre, r_host, 0)
    b_host = np.random.default_rng(8).standard_normal(2197)
    off = solve(env, api.CgSolver(), box13, 1.0, 0.0, b_host, pre, 0)
    ctx.set_option("coop_force_fail", 1)
    try:
        got, took, refused = apply(env, pre, r_host, 1)
        assert (took, refused) == (0, 1) and same_bits(got, want)
        on = solve(env, api.CgSolver(), box13, 1.0, 0.0, b_host, pre, 1)
    finally:
        ctx.set_option("coop_force_fail", 0)
    assert on["amg_tail_applies"] == 0 and on["amg_tail_refusals"] == on["amg_applies"] > 0
    assert on["fallback"] == 1 and same_solve(on, off)
    pre.close()


def test_give_up_reruns_the_solve_without_the_tail(env, box13):
    """The test hook reports a give-up after the solve's kernels have completed normally: nothing waits, nothing hangs."""
    api, mesh, ctx = env
    pre = build(env, box13, 1.0, 0.0, coarse_rows=32)
    b_host = np.random.default_rng(8).standard_normal(2197)
    off = solve(env, api.CgSolver(), box13, 1.0, 0.0, b_host, pre, 0)
    ctx.set_option("coop_force_fail", 2)
    try:
        on = solve(env, api.CgSolver(), box13, 1.0, 0.0, b_host, pre, 1)
    finally:
        ctx.set_option("coop_force_fail", 0)
    assert on["fallback"] == 2 and on["amg_tail_applies"] > 0
    assert on["amg_applies"] > on["amg_tail_applies"]  # (the re-run's applies are launches)
    assert same_solve(on, off)
    pre.close()


def test_a_stand_alone_give_up_is_reported_by_sync(env, box13):
    api, mesh, ctx = env
    pre = build(env, box13, 1.0, 0.0, coarse_rows=32)
    r, z = api.DeviceVector.from_numpy(ctx, rhs(2197)), api.DeviceVector(ctx, 2197)
    ctx.set_option("amg_tail", 1)
    ctx.set_option("amg_tail_rows", BIG)
    ctx.set_option("coop_force_fail", 2)
    try:
        pre.mul(z, r)
        with pytest.raises(Exception, match="cooperative kernel"):
            ctx.sync()
        ctx.sync()  # reported once
    finally:
        ctx.set_option("coop_force_fail", 0)
        ctx.set_option("amg_tail", 0)
    want, _, _ = apply(env, pre, r.to_numpy(), 0)
    got, took, _ = apply(env, pre, r.to_numpy(), 1)  # the path is whole afterwards
    assert took == 1 and same_bits(got, want)
    pre.close()


# ---- 8. api_done set: z untouched ---------------------------------------------------------------------------------------------
def test_an_apply_past_convergence_leaves_z_untouched(env, box13):
    """The engine enqueues iterations ahead of the device's verdict; once the solve's done word is set, the kernels of every
    later call find it.  A callback preconditioner applies the object twice: into the solver's vector and into a side vector
    of its own, NaN-filled before the solve.  A side vector is then either written whole or not at all."""
    api, mesh, ctx = env
    amg = build(env, box13, 1.0, 0.0, coarse_rows=32)
    side = [api.DeviceVector.from_numpy(ctx, np.full(2197, np.nan)) for _ in range(24)]

    class Probe(api.Preconditioner):
        calls = 0

        def mul(self, y_vec, x_vec):
            amg.mul(y_vec, x_vec)
            if self.calls < len(side):
                amg.mul(side[self.calls], x_vec)
            self.calls += 1

    probe = Probe()
    b_host = np.random.default_rng(8).standard_normal(2197)
    on = solve(env, api.CgSolver(), box13, 1.0, 0.0, b_host, probe, 1)
    assert on["ok"] and probe.calls <= len(side)
    assert on["amg_tail_applies"] == 2 * probe.calls and on["amg_tail_refusals"] == 0
    got = [v.to_numpy() for v in side[:probe.calls]]
    written = [bool(np.isfinite(g).all()) for g in got]
    untouched = [bool(np.isnan(g).all()) for g in got]
    print("calls", probe.calls, "pre_applies", on["pre_applies"], "written", written)
    assert all(w != u for w, u in zip(written, untouched))  # whole or not at all
    live = written.index(False)
    assert not any(written[live:])  # once the word is set it stays set
    assert live == on["pre_applies"] and probe.calls > live
    amg.close()


# ---- 7. sequence numbers --------------------------------------------------------------------------------------------------------
def test_applies_back_to_back_and_after_a_chain_solve(env, box13, convdiff):
    api, mesh, ctx = env
    pre = build(env, box13, 1.0, 0.0, coarse_rows=32)
    r_host = rhs(2197)
    want, _, _ = apply(env, pre, r_host, 0)
    ctx.set_option("amg_tail", 1)
    ctx.set_option("amg_tail_rows", BIG)
    try:
        r = api.DeviceVector.from_numpy(ctx, r_host)
        zs = [api.DeviceVector(ctx, 2197) for _ in range(3)]
        before = ctx.counter("amg_tail_applies")
        for z in zs:  # no wait in between
            pre.mul(z, r)
        ctx.sync()
        assert ctx.counter("amg_tail_applies") - before == 3
        for z in zs:
            assert same_bits(z.to_numpy(), want)
    finally:
        ctx.set_option("amg_tail", 0)
    # an unpreconditioned GMRES solve that runs the cooperative Gram-Schmidt chains, then an apply
    cd_mat, cd_n = convdiff
    s = api.GmresSolver()
    s.num_inner_iterations = 30
    chains = ctx.counter("mgs_chain_steps")
    b, x = api.DeviceVector.from_numpy(ctx, np.random.default_rng(8).standard_normal(cd_n)), api.DeviceVector(ctx, cd_n)
    assert s.solve(x, b, api.HipStencilOperator(cd_mat, 1.0, 0.0))
    assert ctx.counter("mgs_chain_steps") > chains
    got, took, _ = apply(env, pre, r_host, 1)
    assert took == 1 and same_bits(got, want)
    pre.close()
