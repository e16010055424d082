"""The operators of the multigrid preconditioner's tests, as host data: the assembled matrix A (scipy CSR) of every case and
what a device test needs to build the same operator."""
import numpy as np
import scipy.sparse as sp


def poisson_box(n):
    """The 7-point Laplacian on n^3 points with Dirichlet walls (diagonal 6, off-diagonals -1): the "box" of the level
    sizes the tests pin (2197 / 280 / 16 ...)."""
    t = sp.diags([-np.ones(n - 1), 2.0 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1])
    i = sp.identity(n)
    a = (sp.kron(sp.kron(t, i), i) + sp.kron(sp.kron(i, t), i) + sp.kron(sp.kron(i, i), t)).tocsr()
    a.sort_indices()
    return a


def mesh_box(mesh, n):
    """-Laplacian of the library's own n^3 box mesh (alpha = -1, beta = 0; the wall cells' diagonals are larger): (graph, A)."""
    g = mesh.structured_box(n)
    return g, mesh.assemble_csr(g, -1.0, 0.0).tocsr()[:, :g.n_cells]


def _direction(delta):
    return np.abs(delta).argmax(axis=1)


def face_weight_case(mesh, n, kind):
    """Diffusion with face weights on the n^3 box and Dirichlet walls, A = -M: `kind` "lognormal" (weights exp(N(0, 1)) per
    interior face) or "aniso" (1 : 1 : 100 by direction).  Returns (graph, w, diag_extra, A) for
    StencilMatrix.from_face_weights(ctx, n_cells, 0, g.inner, g.outer, w, w, diag_extra) applied with alpha = -1, beta = 0."""
    g = mesh.structured_box(n)
    nc = g.n_cells
    by_dir = np.array([1.0, 1.0, 100.0])
    if kind == "aniso":
        w = by_dir[_direction(g.center[g.outer] - g.center[g.inner])]
        wb = 2.0 * by_dir[_direction(g.b_center - g.center[g.b_cell])]
    else:
        w = np.exp(np.random.default_rng(11).standard_normal(g.inner.size))
        wb = np.full(g.b_cell.size, 2.0)
    diag_extra = np.zeros(nc)
    np.add.at(diag_extra, g.b_cell, -wb)
    rows = np.concatenate([g.inner, g.outer, g.inner, g.outer, np.arange(nc)])
    cols = np.concatenate([g.outer, g.inner, g.inner, g.outer, np.arange(nc)])
    vals = np.concatenate([-w, -w, w, w, -diag_extra])
    a = sp.coo_matrix((vals, (rows, cols)), shape=(nc, nc)).tocsr()
    a.sum_duplicates()
    return g, w, diag_extra, a


def random_symmetric(seed=3):
    """The random symmetric, diagonally dominant CSR operator of tests/test_gpu_cheb.py (918 rows at seed 3)."""
    rng = np.random.default_rng(100 + seed)
    n = int(rng.integers(200, 1500))
    nnz_row = int(rng.integers(2, 9))
    rows = np.repeat(np.arange(n), nnz_row)
    cols = (rows + rng.integers(1, n, size=rows.size)) % n
    off = sp.coo_matrix((rng.uniform(-1.0, 1.0, rows.size), (rows, cols)), shape=(n, n)).tocsr()
    off.sum_duplicates()
    sym_off = (off + off.T) * 0.5
    return (sym_off + sp.diags(np.abs(sym_off).sum(axis=1).A1 * 1.5 + 1.0)).tocsr()
