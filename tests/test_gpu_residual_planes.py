"""The plane march of the residual recompute (option `cg_residual_planes`, solver_cg.hip cg_r_planes_kernel): blocks that
own a 2 048-row run of a plane and march over planes form, plane by plane, the accumulators, the block sums and the
partial slots of cg_r_kernel's blocks and hand them to the same ticket fold.  r, <r,r> and with them every scalar of
the solve and x are therefore the SAME BITS as with the gathering form (`cg_residual_planes` 0) and as with z stored
and read back (`cg_residual_march` 0): every comparison here is `np.array_equal`."""
import numpy as np
import pytest

import exact_ref as er

pytestmark = pytest.mark.gpu

# Above the ~4 M rows at which the fused step engages (FUSED_SHAPES of test_gpu_record_index.py), planes of whole
# 2 048-row runs: 16 runs per plane; a = 512 (two halo pairs per thread and plane), 16 runs; 32 runs per plane
PLANE_SHAPES = [(256, 128, 130), (512, 64, 130), (256, 256, 80)]
NO_PLANE_SHAPES = [(200, 100, 211), (192, 120, 190)]  # planes of 20 000 and of 23 040 rows: b % 2048 != 0
# 130 planes leave a last chunk of 2 planes with chunks of 16 (the default), 8 and 32, and of ONE plane with chunks of 3
CHUNKS = [16, 8, 32, 3]
OPTIONS = (("spmv_record_index", 1), ("cg_residual_march", 1), ("cg_residual_planes", 1), ("cg_residual_chunk", 16),
           ("cg_march", 8), ("ticket_verify", 0))


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


# the three forms of r -= alpha z: (cg_residual_march, cg_residual_planes) -> (residual marches, plane marches) counted
FORMS = {"planes": (1, 1), "gather": (1, 0), "z": (0, 1)}


def _run_forms(api, ctx, mat, b, iters_list, plane_marches=1):
    runs = {}
    for name, (rm, planes) in FORMS.items():
        ctx.set_option("cg_residual_march", rm)
        ctx.set_option("cg_residual_planes", planes)
        before = ctx.counter("cg_residual_marches"), ctx.counter("cg_residual_plane_marches")
        runs[name] = {iters: _solve(api, ctx, mat, b, iters) for iters in iters_list}
        assert ctx.counter("cg_residual_marches") - before[0] == len(iters_list) * rm, name
        want = len(iters_list) * plane_marches if name == "planes" else 0
        assert ctx.counter("cg_residual_plane_marches") - before[1] == want, name
    return runs


@pytest.mark.parametrize("idx", [1, 0])
@pytest.mark.parametrize("march", [8, 5, 2])
@pytest.mark.parametrize("shape", PLANE_SHAPES)
def test_plane_march_is_bitwise(env, shape, march, idx):
    api, mesh, ctx = env
    g = _box(mesh, shape)
    ctx.set_option("cg_march", march)
    ctx.set_option("spmv_record_index", idx)
    mat = api.StencilMatrix.from_face_graph(ctx, g)
    runs = _run_forms(api, ctx, mat, _rhs(g.n_cells), (None, 7, 2))
    for iters in (None, 7, 2):
        assert runs["z"][iters][0] == (iters is None)
        _same(runs["planes"][iters], runs["gather"][iters], ("gather", iters))
        _same(runs["planes"][iters], runs["z"][iters], ("z", iters))
    mat.close()


@pytest.mark.parametrize("idx", [1, 0])
@pytest.mark.parametrize("chunk", CHUNKS)
def test_short_last_chunk_is_bitwise(env, chunk, idx):
    api, mesh, ctx = env
    shape = PLANE_SHAPES[0]
    assert shape[2] % chunk != 0
    g = _box(mesh, shape)
    ctx.set_option("cg_residual_chunk", chunk)
    ctx.set_option("spmv_record_index", idx)
    mat = api.StencilMatrix.from_face_graph(ctx, g)
    runs = _run_forms(api, ctx, mat, _rhs(g.n_cells), (None, 7, 2))
    for iters in (None, 7, 2):
        _same(runs["planes"][iters], runs["gather"][iters], ("gather", iters))
        _same(runs["planes"][iters], runs["z"][iters], ("z", iters))
    mat.close()


def test_default_fill_shortens_the_chunk_and_stays_bitwise(env):
    """With the default `cg_residual_fill` a lattice of 130 x 16 runs marches chunks shorter than `cg_residual_chunk`."""
    api, mesh, ctx = env
    g = _box(mesh, PLANE_SHAPES[0])
    mat = api.StencilMatrix.from_face_graph(ctx, g)
    ctx.set_option("cg_residual_fill", 512)
    try:
        runs = _run_forms(api, ctx, mat, _rhs(g.n_cells), (None, 7))
    finally:
        ctx.set_option("cg_residual_fill", 0)
    for iters in (None, 7):
        _same(runs["planes"][iters], runs["gather"][iters], ("gather", iters))
        _same(runs["planes"][iters], runs["z"][iters], ("z", iters))
    mat.close()


@pytest.mark.parametrize("shape", NO_PLANE_SHAPES)
def test_planes_that_are_not_whole_runs_keep_the_gathering_kernel(env, shape):
    api, mesh, ctx = env
    assert (shape[0] * shape[1]) % er.STREAM_BLOCK != 0
    g = _box(mesh, shape)
    mat = api.StencilMatrix.from_face_graph(ctx, g)
    runs = _run_forms(api, ctx, mat, _rhs(g.n_cells), (None, 7), plane_marches=0)
    for iters in (None, 7):
        _same(runs["planes"][iters], runs["gather"][iters], ("gather", iters))
        _same(runs["planes"][iters], runs["z"][iters], ("z", iters))
    mat.close()


def test_plane_march_steps_aside_for_ticket_verify(env):
    api, mesh, ctx = env
    g = _box(mesh, PLANE_SHAPES[0])
    mat = api.StencilMatrix.from_face_graph(ctx, g)
    b = _rhs(g.n_cells)
    ref = _solve(api, ctx, mat, b)
    ctx.set_option("ticket_verify", 1)
    before = ctx.counter("cg_residual_marches"), ctx.counter("cg_residual_plane_marches")
    got = _solve(api, ctx, mat, b)
    assert (ctx.counter("cg_residual_marches"), ctx.counter("cg_residual_plane_marches")) == before
    _same(got, ref, "ticket_verify")
    mat.close()


def test_256_cubed_200_iterations_are_bitwise():
    """The benchmark's lattice with the library's defaults (32 runs per plane, 256 planes), 200 fixed iterations: a
    plane march that summed <r,r> in an order of its own drifts away from the other forms here."""
    from stormruler_amd import api, mesh

    ctx = api.Context(0)
    g = mesh.structured_box(256)
    mat = api.StencilMatrix.from_face_graph(ctx, g)
    runs = _run_forms(api, ctx, mat, np.ones(g.n_cells), (200,))
    assert runs["planes"][200][1] == 200
    _same(runs["planes"][200], runs["gather"][200], "gather")
    _same(runs["planes"][200], runs["z"][200], "z")
    mat.close()
    ctx.close()


@pytest.mark.parametrize("idx", [1, 0])
def test_first_step_pins_where_the_plane_march_runs(env, idx):
    """Integer data on the unit box (exact_ref.py): sqrt(<b,b>), x1 = fl(alpha b) and |r1| pinned on a lattice that
    takes the plane march; iteration 1 -- the first whose residual the plane march forms -- the same bits in all forms."""
    api, mesh, ctx = env
    shape = (256, 256, 66)  # 4.3 M rows, 32 runs per plane; 66 planes: chunks of 16 leave a last chunk of 2
    g = er.unit_box(mesh, *shape)
    b_i = er.int_vector(g.n_cells, 31)
    fs = er.FirstStep(er.Sums(shape, b_i))
    b = b_i.astype(np.float64)
    ctx.set_option("spmv_record_index", idx)
    mat = api.StencilMatrix.from_face_graph(ctx, g)
    before = ctx.counter("cg_fused_steps")
    runs = _run_forms(api, ctx, mat, b, (1, 2))
    assert ctx.counter("cg_fused_steps") - before == 6
    for name in FORMS:
        for iters in (1, 2):
            ok, it, h, x = runs[name][iters]
            assert it == iters and h.size == iters + 1
            assert h[0] == fs.h0, name
            assert er.close(h[1], fs.cg_h1, fs.cg_tol), (name, h[1], fs.cg_h1)
        assert np.array_equal(runs[name][1][3], fs.cg_x1(b_i)), name
    for iters in (1, 2):
        _same(runs["planes"][iters], runs["gather"][iters], ("gather", iters))
        _same(runs["planes"][iters], runs["z"][iters], ("z", iters))
    mat.close()
