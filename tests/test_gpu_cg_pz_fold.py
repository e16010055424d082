"""<p,z> folded inside the residual kernel (option `cg_pz_fold`, solver_cg.hip cg_r_planes_kernel): where the plane march
runs and one pass folds the step kernel's per-wave partials (at most 8 192), every block of the march folds them itself
-- block_fold's order, through block_fold_issue / block_fold_sum -- and the one-block launch between the two kernels is
gone.  The sum, alpha and everything behind them are the SAME BITS as with the launch (`cg_pz_fold` 0), with the
gathering recompute (`cg_residual_planes` 0) and with z stored and read back (`cg_residual_march` 0): every comparison
here is `np.array_equal`.  Counter `cg_pz_consumer_folds`: the solves that took the road."""
import numpy as np
import pytest

import exact_ref as er

pytestmark = pytest.mark.gpu

OPTIONS = (("spmv_record_index", 1), ("cg_residual_march", 1), ("cg_residual_planes", 1), ("cg_residual_chunk", 16),
           ("cg_march", 8), ("ticket_verify", 0), ("cg_pz_fold", 1))


@pytest.fixture(scope="module")
def env():
    from stormruler_amd import api, mesh

    ctx = api.Context(0)
    ctx.set_option("latency_path", 0)
    ctx.set_option("spmv_canon_tile_min_rows", 0)
    ctx.set_option("cg_march_fill", 0)  # (the chunk sizes asked for, however small the lattice)
    ctx.set_option("cg_residual_fill", 0)
    yield api, mesh, ctx
    ctx.close()


@pytest.fixture(autouse=True)
def _defaults(env):
    yield
    _, _, ctx = env
    for k, v in OPTIONS:
        ctx.set_option(k, v)


def _box(mesh, shape):
    # (spacing 1/128 in every direction: exact in binary, so the box has few distinct weights -- and row words)
    return mesh.structured_box(*shape, lengths=tuple(s / 128.0 for s in shape))


def _rhs(n):
    return 1.0 + 0.5 * np.sin(0.05 * np.arange(n))


def _solve(api, ctx, mat, b, iters=None):
    s = api.CgSolver()
    s.record_history = True
    if iters is not None:
        s.num_iterations = iters
    x = api.DeviceVector(ctx, b.size)
    ok = s.solve(x, api.DeviceVector.from_numpy(ctx, b), api.HipStencilOperator(mat, -1.0, 0.0))
    return ok, s.iteration, np.array(s.history), x.to_numpy()


def _same(got, ref, what):
    assert got[0] == ref[0] and got[1] == ref[1], (what, got[0], got[1], ref[0], ref[1])
    assert np.array_equal(got[2], ref[2]), (what, "history")
    assert np.array_equal(got[3], ref[3]), (what, "x", int(np.count_nonzero(got[3] != ref[3])))


# (cg_pz_fold, cg_residual_march, cg_residual_planes) -> whether a solve of two iterations or more folds in the consumer
FORMS = {"fold": (1, 1, 1), "launch": (0, 1, 1), "gather": (1, 1, 0), "z": (1, 0, 1)}


def _run_forms(api, ctx, mat, b, iters_list, forms=("fold", "launch", "gather", "z"), folds=1):
    """Every form's solves; the counter rises by `folds` per solve in form "fold" and by none in the others."""
    runs = {}
    for name in forms:
        fold, rm, planes = FORMS[name]
        ctx.set_option("cg_pz_fold", fold)
        ctx.set_option("cg_residual_march", rm)
        ctx.set_option("cg_residual_planes", planes)
        before = ctx.counter("cg_pz_consumer_folds")
        runs[name] = {iters: _solve(api, ctx, mat, b, iters) for iters in iters_list}
        want = len(iters_list) * folds if name == "fold" else 0
        assert ctx.counter("cg_pz_consumer_folds") - before == want, name
    return runs


def _all_same(runs, iters_list):
    for iters in iters_list:
        for name in runs:
            if name != "fold":
                _same(runs["fold"][iters], runs[name][iters], (name, iters))


@pytest.mark.parametrize("idx", [1, 0])
@pytest.mark.parametrize("march", [8, 5])
def test_fold_on_and_off_are_bitwise_and_the_counter_moves(env, march, idx):
    """(256,128,130): 32 tiles per plane, four waves per block; chunks of 8 planes: 17 x 32 x 4 = 2 176 partials (8.5 per
    thread), of 5: 26 x 32 x 4 = 3 328 (13 per thread).  To tolerance, 7 and 2 iterations."""
    api, mesh, ctx = env
    shape = (256, 128, 130)
    assert -(-shape[2] // march) * 32 * 4 == {8: 2176, 5: 3328}[march] <= 8192
    g = _box(mesh, shape)
    ctx.set_option("cg_march", march)
    ctx.set_option("spmv_record_index", idx)
    mat = api.StencilMatrix.from_face_graph(ctx, g)
    runs = _run_forms(api, ctx, mat, _rhs(g.n_cells), (None, 7, 2))
    assert runs["fold"][None][0] and runs["fold"][7][1] == 7 and runs["fold"][2][1] == 2
    _all_same(runs, (None, 7, 2))
    mat.close()


def test_ragged_count_and_a_last_chunk_of_one_plane(env):
    """(512,64,130), a = 512: 2 176 partials -- eight for every thread and a ninth for half of them --, residual chunks
    of 3 planes whose last chunk is ONE plane."""
    api, mesh, ctx = env
    shape = (512, 64, 130)
    assert shape[2] % 3 == 1 and (-(-shape[2] // 8) * 32 * 4) % 256 != 0
    g = _box(mesh, shape)
    ctx.set_option("cg_residual_chunk", 3)
    mat = api.StencilMatrix.from_face_graph(ctx, g)
    runs = _run_forms(api, ctx, mat, _rhs(g.n_cells), (None, 7, 2))
    assert runs["fold"][None][0]
    _all_same(runs, (None, 7, 2))
    mat.close()


def test_above_the_single_pass_limit_the_launch_stays(env):
    """(256,256,80) in chunks of 2 planes: 40 x 64 x 4 = 10 240 partials, more than one pass folds: the ticketed first pass
    keeps its launch, the counter does not move."""
    api, mesh, ctx = env
    shape = (256, 256, 80)
    assert (shape[2] // 2) * 64 * 4 == 10240 > 8192
    g = _box(mesh, shape)
    ctx.set_option("cg_march", 2)
    mat = api.StencilMatrix.from_face_graph(ctx, g)
    runs = _run_forms(api, ctx, mat, _rhs(g.n_cells), (None, 7), forms=("fold", "launch"), folds=0)
    _all_same(runs, (None, 7))
    mat.close()


def test_a_late_block_does_not_see_clobbered_partials(env):
    """Residual chunks of 2 planes: 65 x 16 = 1 040 blocks, more than are resident at once -- the first to finish publish
    their <r,r> partials while the last have not started: those slots must not be the <p,z> partials'."""
    api, mesh, ctx = env
    g = _box(mesh, (256, 128, 130))
    ctx.set_option("cg_residual_chunk", 2)
    mat = api.StencilMatrix.from_face_graph(ctx, g)
    runs = _run_forms(api, ctx, mat, _rhs(g.n_cells), (7,), forms=("fold", "launch"))
    assert runs["fold"][7][1] == 7
    _all_same(runs, (7,))
    mat.close()


@pytest.mark.parametrize("idx", [1, 0])
def test_first_step_pins_with_the_fold(env, idx):
    """Integer data on the unit box (exact_ref.py): sqrt(<b,b>), x1 = fl(alpha b) and |r1| pinned with the fold on;
    iteration 1 -- the first whose <p,z> the residual kernel folds -- the same bits as with the launch."""
    api, mesh, ctx = env
    shape = (256, 256, 66)  # 4.3 M rows; 9 chunks of 8 planes x 64 tiles x 4 waves = 2 304 partials
    g = er.unit_box(mesh, *shape)
    b_i = er.int_vector(g.n_cells, 31)
    fs = er.FirstStep(er.Sums(shape, b_i))
    b = b_i.astype(np.float64)
    ctx.set_option("spmv_record_index", idx)
    mat = api.StencilMatrix.from_face_graph(ctx, g)
    before = ctx.counter("cg_pz_consumer_folds")
    runs = {"fold": {iters: _solve(api, ctx, mat, b, iters) for iters in (1, 2)}}
    assert ctx.counter("cg_pz_consumer_folds") - before == 1  # (a solve of ONE iteration has no fused step)
    for iters in (1, 2):
        ok, it, h, x = runs["fold"][iters]
        assert it == iters and h.size == iters + 1
        assert h[0] == fs.h0
        assert er.close(h[1], fs.cg_h1, fs.cg_tol), (h[1], fs.cg_h1)
    assert np.array_equal(runs["fold"][1][3], fs.cg_x1(b_i))
    ctx.set_option("cg_pz_fold", 0)
    runs["launch"] = {iters: _solve(api, ctx, mat, b, iters) for iters in (1, 2)}
    assert ctx.counter("cg_pz_consumer_folds") - before == 1
    _all_same(runs, (1, 2))
    mat.close()


def test_ticket_verify_takes_neither_the_plane_march_nor_the_fold(env):
    api, mesh, ctx = env
    g = _box(mesh, (256, 128, 130))
    mat = api.StencilMatrix.from_face_graph(ctx, g)
    b = _rhs(g.n_cells)
    before = ctx.counter("cg_pz_consumer_folds")
    ref = _solve(api, ctx, mat, b)
    assert ctx.counter("cg_pz_consumer_folds") - before == 1
    ctx.set_option("ticket_verify", 1)
    before = ctx.counter("cg_residual_plane_marches"), ctx.counter("cg_pz_consumer_folds")
    got = _solve(api, ctx, mat, b)
    assert (ctx.counter("cg_residual_plane_marches"), ctx.counter("cg_pz_consumer_folds")) == before
    _same(got, ref, "ticket_verify")
    mat.close()
