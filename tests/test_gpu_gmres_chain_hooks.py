"""The test hooks of the GMRES Gram-Schmidt chain kernel (option test_disable, context.hip) on a case that runs
mgs_chain_quad_kernel: BASELINE config 4's operator, convection-diffusion on the 128^3 box, fixed-K GMRES(30) over two
restart cycles.  Every step's chain must be the quad kernel (counter mgs_quad_steps).
    512  the column's earlier Givens rotations under the norm's all-reduce, off: after everything else -- the same
         arithmetic moved in time: the same bits
    128  one contiguous run of row chunks per XCD, off: chunk = block index -- the all-reduce slots stay indexed by
         block, so a block's partial covers other rows: the same sums in another fixed order (mgs_chain_quad_kernel's
         own comment), not the same bits
    256  the order of the basis vectors alternating with k, off: ascending -- the projections are summed in another
         order
    128 and 256: history and x within 1e-12 (x is H's back-substitution: the API exposes no H)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ITERS = 60


@pytest.fixture(scope="module")
def env():
    from stormruler_amd import api, mesh

    ctx = api.Context(0)
    g = mesh.structured_box(128)
    wi, wo, de = mesh.convection_diffusion_weights(g, 1e-2, (1.0, 0.5, 0.25))
    mat = api.StencilMatrix.from_face_weights(ctx, g.n_cells, g.n_halo, g.inner, g.outer, wi, wo, de)
    yield api, ctx, g, mat
    ctx.set_option("test_disable", 0)
    mat.close()
    ctx.close()


def _run(api, ctx, g, mat, bits):
    ctx.set_option("test_disable", bits)
    s = api.GmresSolver()
    s.num_inner_iterations, s.num_iterations = 30, ITERS
    s.absolute_error_tolerance = s.relative_error_tolerance = 0.0
    s.record_history = True
    b = api.DeviceVector.from_numpy(ctx, 1.0 + 0.5 * np.sin(0.01 * np.arange(g.n_cells)))
    x = api.DeviceVector(ctx, g.n_cells)
    before = ctx.counter("mgs_chain_steps"), ctx.counter("mgs_quad_steps")
    s.solve(x, b, api.HipStencilOperator(mat, 1.0, 0.0))
    chain, quad = ctx.counter("mgs_chain_steps") - before[0], ctx.counter("mgs_quad_steps") - before[1]
    ctx.set_option("test_disable", 0)
    assert s.path_fallback == 0 and s.iteration == ITERS
    assert quad == chain == ITERS, (chain, quad)
    return np.array(s.history), x.to_numpy()


def test_chain_hooks_ab(env):
    api, ctx, g, mat = env
    h0, x0 = _run(api, ctx, g, mat, 0)
    assert h0[-1] < h0[0]
    h, x = _run(api, ctx, g, mat, 512)
    assert np.array_equal(h, h0) and np.array_equal(x, x0)
    for bits in (128, 256):
        h, x = _run(api, ctx, g, mat, bits)
        assert np.allclose(h, h0, rtol=1e-12, atol=0.0), bits
        assert np.linalg.norm(x - x0) <= 1e-12 * np.linalg.norm(x0), bits
