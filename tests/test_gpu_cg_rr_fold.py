"""The top level of <r,r> folded inside the step kernel (option `cg_rr_fold`): on the road that folds <p,z> in the plane
march (`cg_pz_fold`; one rank, from iteration 1 on), cg_r_planes_kernel ends at its group sums -- no top-level ticket, no
scalar step in its last block -- and the NEXT iteration's cg_step_march_kernel folds them in ticket_fold_groups' order,
forms beta, `done` and the iteration counter in every block and stores them from its first; behind the last enqueued
iteration cg_rr_finish_kernel does.  Everything is the SAME BITS as with the option off: every comparison here is
`np.array_equal` of x, the residual history, the final residual and the iteration count.  Counter `cg_rr_consumer_folds`:
the solves that took the road.

Slot counts.  The loop takes the fused step only where the tiled kernel's 4 n / 2 048 per-wave partials exceed one pass
(8 192), so on this road the <r,r> slot count n / 2 048 is at least 2 049: the group shapes are met THERE -- 2 080 slots (a
ragged last group of 32), 2 112 (33 full groups), 2 049 (a last group of ONE slot).  Lattices of 40, 64, 65 and 300 slots
never reach the fused step: the option must be inert on them (same bits, the counter still)."""
import numpy as np
import pytest

import exact_ref as er

pytestmark = pytest.mark.gpu

OPTIONS = (("spmv_record_index", 1), ("cg_residual_march", 1), ("cg_residual_planes", 1), ("cg_residual_chunk", 16),
           ("cg_march", 8), ("ticket_verify", 0), ("cg_pz_fold", 1), ("cg_rr_fold", 1))
RAGGED, FULL, ONE = (256, 128, 130), (256, 128, 132), (64, 32, 2049)  # 2 080, 2 112, 2 049 slots
assert [s[0] * s[1] * s[2] // er.STREAM_BLOCK % 64 for s in (RAGGED, FULL, ONE)] == [32, 0, 1]


@pytest.fixture(scope="module")
def env():
    from stormruler_amd import api, mesh

    ctx = api.Context(0)
    ctx.set_option("latency_path", 0)
    ctx.set_option("spmv_canon_tile_min_rows", 0)
    ctx.set_option("cg_march_fill", 0)  # (the chunk sizes asked for, however small the lattice)
    ctx.set_option("cg_residual_fill", 0)
    yield api, mesh, ctx
    for mat in _matrices.values():
        mat.close()
    _matrices.clear()
    ctx.close()


@pytest.fixture(autouse=True)
def _defaults(env):
    yield
    _, _, ctx = env
    for k, v in OPTIONS:
        ctx.set_option(k, v)


_matrices = {}


def _matrix(env, shape):
    """The operator of a box with spacing 1/128 (exact in binary: few distinct row words), built once; one 4 M-row box at a time."""
    api, mesh, ctx = env
    if shape not in _matrices:
        for other in list(_matrices):
            _matrices.pop(other).close()
        g = mesh.structured_box(*shape, lengths=tuple(s / 128.0 for s in shape))
        _matrices[shape] = api.StencilMatrix.from_face_graph(ctx, g)
    return _matrices[shape]


def _rhs(n, k=0.05):
    return 1.0 + 0.5 * np.sin(k * np.arange(n))


def _solve(env, mat, b, iters=None, abs_tol=None):
    api, _, ctx = env
    s = api.CgSolver()
    s.record_history = True
    if iters is not None:
        s.num_iterations = iters
    if abs_tol is not None:
        s.absolute_error_tolerance, s.relative_error_tolerance = abs_tol, 0.0
    x = api.DeviceVector(ctx, b.size)
    ok = s.solve(x, api.DeviceVector.from_numpy(ctx, b), api.HipStencilOperator(mat, -1.0, 0.0))
    return bool(ok), int(s.iteration), np.array(s.history), x.to_numpy(), float(s.absolute_error)


def _same(got, ref, what):
    assert got[0] == ref[0] and got[1] == ref[1], (what, got[0], got[1], ref[0], ref[1])
    assert np.array_equal(got[2], ref[2]), (what, "history")
    assert np.array_equal(got[3], ref[3]), (what, "x", int(np.count_nonzero(got[3] != ref[3])))
    assert got[4] == ref[4], (what, "final residual", got[4], ref[4])


def _on_off(env, mat, b, solves, folds=1, options=()):
    """Each of `solves` (keyword sets of _solve) with the option on and off: the same bits; the counter rises by `folds`
    per solve with the option on and stands with it off.  Returns the runs with the option on."""
    _, _, ctx = env
    runs = {}
    for fold in (1, 0):
        for k, v in options:
            ctx.set_option(k, v)
        ctx.set_option("cg_rr_fold", fold)
        before = ctx.counter("cg_rr_consumer_folds")
        runs[fold] = [_solve(env, mat, b, **kw) for kw in solves]
        assert ctx.counter("cg_rr_consumer_folds") - before == (len(solves) * folds if fold else 0), fold
    for kw, got, ref in zip(solves, runs[1], runs[0]):
        _same(got, ref, kw)
    return runs[1]


@pytest.mark.parametrize("shape", [FULL, ONE, RAGGED], ids=["full-groups", "group-of-one", "ragged-group"])
def test_on_and_off_are_bitwise_and_the_counter_moves(env, shape):
    """To tolerance (the converging iteration's scalar step runs in the step kernel enqueued behind it, x complete), 7 and
    2 iterations (ended by `num_iterations`: the scalar step of the last one runs in cg_rr_finish_kernel)."""
    mat = _matrix(env, shape)
    n = shape[0] * shape[1] * shape[2]
    runs = _on_off(env, mat, _rhs(n), ({}, {"iters": 7}, {"iters": 2}))
    assert runs[0][0] and 7 < runs[0][1] < 2000
    assert not runs[1][0] and runs[1][1] == 7 and runs[1][2].size == 8
    assert not runs[2][0] and runs[2][1] == 2 and runs[2][2].size == 3


def test_a_solve_of_one_iteration_has_nothing_to_fold(env):
    mat = _matrix(env, RAGGED)
    runs = _on_off(env, mat, _rhs(RAGGED[0] * RAGGED[1] * RAGGED[2]), ({"iters": 1},), folds=0)
    assert runs[0][1] == 1


@pytest.mark.parametrize("nz", [40, 64, 65, 300])
def test_lattices_below_the_fused_step_are_left_alone(env, nz):
    """a = 64, b = 2 048: nz slots of <r,r> -- one ragged group, exactly one, a second of one slot, five with a ragged last.
    The SpMV finishes <p,z> by tickets at these sizes and the loop has no fused step: the option changes nothing."""
    api, mesh, ctx = env
    shape = (64, 32, nz)
    g = mesh.structured_box(*shape, lengths=tuple(s / 128.0 for s in shape))
    mat = api.StencilMatrix.from_face_graph(ctx, g)
    before = ctx.counter("cg_fused_steps")
    _on_off(env, mat, _rhs(g.n_cells), ({"iters": 7}, {"iters": 2}), folds=0)
    assert ctx.counter("cg_fused_steps") == before
    mat.close()


def test_a_second_round_of_residual_blocks(env):
    """Residual chunks of 2 planes: 65 x 16 = 1 040 blocks, more than are resident at once -- late blocks draw from group
    counters that earlier blocks of the same launch and the launches before it left re-armed."""
    mat = _matrix(env, RAGGED)
    runs = _on_off(env, mat, _rhs(RAGGED[0] * RAGGED[1] * RAGGED[2]), ({"iters": 9},), options=(("cg_residual_chunk", 2),))
    assert runs[0][1] == 9


def test_convergence_mid_way_by_an_absolute_tolerance(env):
    """The solve stops at the first iteration k >= 3 whose residual is below all before it (the history of a solve to the
    default tolerances says which), by an absolute tolerance halfway down to it, with k + 4 iterations allowed: x is
    complete (the step kernel behind iteration k applies its update and no more), `iteration` = k, converged."""
    mat = _matrix(env, RAGGED)
    b = _rhs(RAGGED[0] * RAGGED[1] * RAGGED[2])
    h = _solve(env, mat, b)[2]
    k = next(i for i in range(3, h.size) if h[i] < h[:i].min())
    tol = 0.5 * (h[k] + h[:k].min())
    runs = _on_off(env, mat, b, ({"iters": k + 4, "abs_tol": tol},))
    assert runs[0][0] and runs[0][1] == k and runs[0][2].size == k + 1
    # (x of the stopped solve is x_k: the same as k iterations by count)
    assert np.array_equal(runs[0][3], _solve(env, mat, b, iters=k, abs_tol=0.0)[3])


def test_two_solves_back_to_back_on_one_context(env):
    """Counters and the group-sum buffer are reused: a second right-hand side behind the first, and the first again."""
    _, _, ctx = env
    mat = _matrix(env, RAGGED)
    n = RAGGED[0] * RAGGED[1] * RAGGED[2]
    runs = {}
    for fold in (1, 0):
        ctx.set_option("cg_rr_fold", fold)
        before = ctx.counter("cg_rr_consumer_folds")
        runs[fold] = [_solve(env, mat, _rhs(n), iters=5), _solve(env, mat, _rhs(n, 0.031), iters=6), _solve(env, mat, _rhs(n), iters=5)]
        assert ctx.counter("cg_rr_consumer_folds") - before == (3 if fold else 0)
    for i in range(3):
        _same(runs[1][i], runs[0][i], i)
    _same(runs[1][2], runs[1][0], "again")


@pytest.mark.parametrize("option", ["ticket_verify", "cg_pz_fold", "cg_residual_planes"])
def test_the_other_roads_keep_their_code(env, option):
    """`ticket_verify`, the one-block <p,z> launch and the gathering recompute: the residual kernel finishes <r,r> itself."""
    mat = _matrix(env, RAGGED)
    b = _rhs(RAGGED[0] * RAGGED[1] * RAGGED[2])
    ref = _on_off(env, mat, b, ({"iters": 7},))[0]
    value = 1 if option == "ticket_verify" else 0
    got = _on_off(env, mat, b, ({"iters": 7},), folds=0, options=((option, value),))[0]
    _same(got, ref, option)


def test_a_512_with_a_last_chunk_of_one_plane(env):
    """(512,64,130), a = 512 (two halo pairs per thread), residual chunks of 3 planes whose last chunk is ONE plane."""
    shape = (512, 64, 130)
    assert shape[2] % 3 == 1
    mat = _matrix(env, shape)
    _on_off(env, mat, _rhs(shape[0] * shape[1] * shape[2]), ({}, {"iters": 7}, {"iters": 2}), options=(("cg_residual_chunk", 3),))


def test_the_first_two_steps_against_the_exact_reference(env):
    """Integer data on the unit box, as tests/test_gpu_exact_steps.py forms it (exact_ref.StepProblem, pins of CG with
    K = 2): history[0] bitwise, history[1..2] and x_2 within the pins' tolerances -- iteration 1 is the first whose residual
    kernel ends at its group sums, and with two iterations cg_rr_finish_kernel runs its scalar step."""
    from oracle import oracle

    import test_gpu_exact_steps as steps  # (its cache of step problems: the 4 M-row chain is built once for both modules)

    api, mesh, ctx = env
    assert RAGGED == steps.PLANES
    key = (RAGGED, "poisson")
    if key not in steps._problems:
        steps._problems[key] = er.StepProblem(oracle, mesh, RAGGED)
    p = steps._problems[key]
    pins = p.pins("cg", K=2)
    mat = api.StencilMatrix.from_face_graph(ctx, p.g)
    b = p.b.astype(np.float64)
    runs = _on_off(env, mat, b, ({"iters": 2, "abs_tol": 0.0},))
    ok, it, h, x, _ = runs[0]
    assert it == 2 and h.size == 3
    pins.check(list(h), "cg_rr_fold", 2)
    pins.check_x(x, 2, "cg_rr_fold")
    mat.close()
