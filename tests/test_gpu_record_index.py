"""The row-record index of format-4 lattice operators (option `spmv_record_index`: one byte per row naming the row's
8-byte record word in a table of the distinct words) and the residual march of the fused CG loop (option
`cg_residual_march`: r -= alpha z with z = A p' recomputed from p' instead of stored by the step kernel and read
back).  The index carries the same word to the same arithmetic, and the recompute forms z with the step kernel's
arithmetic and r and <r,r> with cg_r_kernel's rows, order and statements: applies and whole solves are BIT-identical
with and without either."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (nx, ny, nz): lines shorter / longer than a wave's rows, planes smaller than a tile, ragged last tiles and chunks
SHAPES = [(20, 6, 9), (256, 8, 8), (128, 16, 11), (64, 40, 9), (34, 34, 17), (64, 32, 24), (512, 4, 8)]
# The fused CG step runs where the SpMV's per-wave partials outnumber one reduction pass (more than 2048 tiles): ~4 M
# rows.  A plane of 32 tiles; one of 19.5 tiles with an odd plane count; a = 512 (two halo pairs per thread and plane)
FUSED_SHAPES = [(256, 128, 130), (200, 100, 211), (512, 64, 130)]


@pytest.fixture(scope="module")
def env():
    from stormruler_amd import api, mesh

    ctx = api.Context(0)
    ctx.set_option("latency_path", 0)
    ctx.set_option("spmv_canon_tile_min_rows", 0)
    ctx.set_option("cg_march_fill", 0)  # (the chunk sizes asked for, however small the lattice)
    yield api, mesh, ctx
    ctx.close()


@pytest.fixture(autouse=True)
def _defaults(env):
    yield
    _, _, ctx = env
    for k, v in (("spmv_record_index", 1), ("cg_residual_march", 1), ("spmv_canon_tile", 2), ("cg_march", 8),
                 ("ticket_verify", 0)):
        ctx.set_option(k, v)


def _box(mesh, shape):
    # (spacing 1/128 in every direction: exact in binary, so the box has few distinct weights -- and row words)
    return mesh.structured_box(*shape, lengths=tuple(s / 128.0 for s in shape))


def _apply(api, ctx, mat, x, alpha=-0.7, beta=0.3):
    xv, yv = api.DeviceVector.from_numpy(ctx, x), api.DeviceVector(ctx, x.size)
    mat.apply(alpha, beta, xv, yv)
    return yv.to_numpy()


def _solve(api, ctx, mat, b, iters=None):
    s = api.CgSolver()
    s.record_history = True
    if iters is not None:
        s.num_iterations = iters
    x = api.DeviceVector(ctx, b.size)
    ok = s.solve(x, api.DeviceVector.from_numpy(ctx, b), api.HipStencilOperator(mat, -1.0, 0.0))
    return ok, s.iteration, np.array(s.history), x.to_numpy()


@pytest.mark.parametrize("tz", [2, 4])
@pytest.mark.parametrize("shape", SHAPES)
def test_tiled_apply_is_bitwise_with_and_without_the_index(env, shape, tz):
    api, mesh, ctx = env
    g = _box(mesh, shape)
    ctx.set_option("spmv_canon_tile", tz)
    mat = api.StencilMatrix.from_face_graph(ctx, g)
    st = mat.stats()
    if st["tiled_planes"] == 0:  # (a = 512 with four planes: the tile's LDS copy would not fit)
        mat.close()
        return
    assert st["paired_rows"] == 2 and st["record_bytes"] == 1024 * st["n_slices"]
    # one byte per row and a table of at most 256 words
    assert 128 * st["n_slices"] < st["streamed_record_bytes"] <= 128 * st["n_slices"] + 8 * 256
    x = np.sin(0.37 * np.arange(g.n_cells)) + 1e-3 * np.cos(1.7 * np.arange(g.n_cells))
    y1 = _apply(api, ctx, mat, x)
    ctx.set_option("spmv_record_index", 0)
    assert mat.stats()["streamed_record_bytes"] == st["record_bytes"]
    y0 = _apply(api, ctx, mat, x)
    ctx.set_option("spmv_canon_tile", 0)
    y_plain = _apply(api, ctx, mat, x)
    assert np.array_equal(y1, y0) and np.array_equal(y0, y_plain)
    mat.close()


@pytest.mark.parametrize("march", [8, 5, 2])
@pytest.mark.parametrize("shape", FUSED_SHAPES)
def test_march_step_is_bitwise_with_and_without_the_index(env, shape, march):
    """The marching step kernel (x += alpha p, p' = r + beta p, z = A p', <p', z>) with the index against the 8-byte
    records, the residual march off: every scalar of the solve and x are the same bits."""
    api, mesh, ctx = env
    g = _box(mesh, shape)
    ctx.set_option("cg_march", march)
    ctx.set_option("cg_residual_march", 0)
    mat = api.StencilMatrix.from_face_graph(ctx, g)
    b = 1.0 + 0.5 * np.sin(0.05 * np.arange(g.n_cells))
    runs = {}
    for idx in (1, 0):
        ctx.set_option("spmv_record_index", idx)
        before = ctx.counter("cg_fused_steps")
        runs[idx] = [_solve(api, ctx, mat, b, iters) for iters in (None, 7)]
        assert ctx.counter("cg_fused_steps") - before == 2
    for r1, r0 in zip(runs[1], runs[0]):
        assert r1[0] == r0[0] and r1[1] == r0[1]
        assert np.array_equal(r1[2], r0[2]) and np.array_equal(r1[3], r0[3])
    mat.close()


@pytest.mark.parametrize("idx", [1, 0])
@pytest.mark.parametrize("march", [8, 5, 2])
@pytest.mark.parametrize("shape", FUSED_SHAPES)
def test_residual_recompute_is_bitwise(env, shape, march, idx):
    api, mesh, ctx = env
    g = _box(mesh, shape)
    ctx.set_option("cg_march", march)
    ctx.set_option("spmv_record_index", idx)
    mat = api.StencilMatrix.from_face_graph(ctx, g)
    b = 1.0 + 0.5 * np.sin(0.05 * np.arange(g.n_cells))
    runs = {}
    for rm in (1, 0):
        ctx.set_option("cg_residual_march", rm)
        before = ctx.counter("cg_residual_marches")
        runs[rm] = {iters: _solve(api, ctx, mat, b, iters) for iters in (None, 7, 2)}
        assert ctx.counter("cg_residual_marches") - before == 3 * rm
    for iters in (None, 7, 2):
        ok1, it1, h1, x1 = runs[1][iters]
        ok0, it0, h0, x0 = runs[0][iters]
        assert ok1 == ok0 and it1 == it0, (iters, it1, it0)
        assert ok0 == (iters is None)
        assert np.array_equal(h1, h0) and np.array_equal(x1, x0), iters
    mat.close()


def test_residual_recompute_steps_aside_for_ticket_verify(env):
    """Option ticket_verify recomputes <p, z> from z: the loop then keeps z and cg_r_kernel -- the same bits as with the
    residual march switched off."""
    api, mesh, ctx = env
    g = _box(mesh, FUSED_SHAPES[0])
    mat = api.StencilMatrix.from_face_graph(ctx, g)
    b = 1.0 + 0.5 * np.sin(0.05 * np.arange(g.n_cells))
    ctx.set_option("ticket_verify", 1)
    runs = {}
    for rm in (1, 0):
        ctx.set_option("cg_residual_march", rm)
        before = ctx.counter("cg_residual_marches")
        runs[rm] = _solve(api, ctx, mat, b)
        assert ctx.counter("cg_residual_marches") == before
    assert runs[1][0] and runs[1][1] == runs[0][1]
    assert np.array_equal(runs[1][2], runs[0][2]) and np.array_equal(runs[1][3], runs[0][3])
    ctx.set_option("ticket_verify", 0)
    ctx.set_option("cg_residual_march", 1)
    s_rm = _solve(api, ctx, mat, b)
    assert s_rm[1] == runs[0][1] and np.array_equal(s_rm[2], runs[0][2]) and np.array_equal(s_rm[3], runs[0][3])
    mat.close()


def test_more_than_256_row_words_keep_the_8_byte_records(env):
    """Weights drawn at random from four values: thousands of distinct row words, no index -- the kernels read the
    records as before, and the option changes nothing."""
    api, mesh, ctx = env
    g = _box(mesh, FUSED_SHAPES[0])
    rng = np.random.default_rng(7)
    w = rng.choice(np.array([0.5, 1.0, 1.5, 2.0]), g.n_faces)
    mat = api.StencilMatrix.from_face_weights(ctx, g.n_cells, g.n_halo, g.inner, g.outer, w, w, None)
    st = mat.stats()
    assert st["paired_rows"] == 2 and st["tiled_planes"] == 2
    assert st["streamed_record_bytes"] == st["record_bytes"]
    before = ctx.counter("cg_residual_marches")
    x = np.sin(0.37 * np.arange(g.n_cells))
    b = 1.0 + 0.5 * np.sin(0.05 * np.arange(g.n_cells))
    out = {}
    for idx in (1, 0):
        ctx.set_option("spmv_record_index", idx)
        out[idx] = (_apply(api, ctx, mat, x), _solve(api, ctx, mat, b, 6))
    assert ctx.counter("cg_residual_marches") - before == 2  # (the residual march reads the 8-byte records then)
    assert np.array_equal(out[1][0], out[0][0])
    assert np.array_equal(out[1][1][2], out[0][1][2]) and np.array_equal(out[1][1][3], out[0][1][3])
    mat.close()
