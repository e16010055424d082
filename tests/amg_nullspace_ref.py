"""What the null-space multigrid setup and cycle add to tests/amg_ref.py, restated in numpy / scipy: N1 (row sums), N2
(connectivity) and N3 (the coarsest level's pseudo-inverse) of include/storm_hip.h ("Singular operators with the constants as
their kernel"), the cycle B = Pi V Pi, and the operators of the tests.  Steps 1 - 6 of the recipe, the smoother and the V-cycle
are amg_ref's.  Nothing here calls the library."""
import os
import sys

import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import amg_cases  # noqa: E402
import amg_ref  # noqa: E402

ROW_SUM_THRESHOLD = 2.0 ** -40
PIVOT_THRESHOLD = 2.0 ** -30


def first_bad_row(a):
    """N1: the first row of the normalised matrix with |sum_j a_ij| > 2^-40 sum_j |a_ij|, or None."""
    a = amg_ref.normalise(a)
    s = np.asarray(a.sum(axis=1)).ravel()
    sa = np.asarray(abs(a).sum(axis=1)).ravel()
    bad = np.flatnonzero(np.abs(s) > ROW_SUM_THRESHOLD * sa)
    return int(bad[0]) if bad.size else None


def components(a):
    """N2: connected components of the graph of the non-zero off-diagonal entries, both directions joined."""
    a = amg_ref.normalise(a)
    off = (a - sp.diags(a.diagonal())).tocsr()
    off.eliminate_zeros()
    return int(connected_components(off, directed=False)[0])


def coarse_inverse(ac):
    """N3: (Ainv, s) of the dense coarsest matrix."""
    ac = np.asarray(ac, dtype=np.float64)
    n = ac.shape[0]
    if n == 1:
        return np.zeros((1, 1)), 0.0
    s = float(ac.diagonal().max())
    if not s > 0.0:
        raise ValueError("no positive diagonal entry")
    g = np.linalg.inv(ac + s / n)
    g = g - g.sum(axis=0, keepdims=True) / n  # every column less its mean
    g = g - g.sum(axis=1, keepdims=True) / n  # ... then every row
    return g, s


def hierarchy(a, **params):
    """amg_ref.hierarchy with N1 - N3: (levels, Ainv, s).  Raises ValueError where the library returns E_INVALID."""
    q = dict(amg_ref.DEFAULTS, **params)
    row = first_bad_row(a)
    if row is not None:
        raise ValueError(f"row {row}: the constants are not in the kernel")
    if components(a) != 1:
        raise ValueError(f"{components(a)} components")
    levels = [dict(A=amg_ref.normalise(a))]
    while True:  # steps 1 - 6, unchanged
        cur = levels[-1]["A"]
        n = cur.shape[0]
        if n <= q["coarse_rows"]:
            break
        if len(levels) >= q["max_levels"]:
            if n <= amg_ref.MAX_COARSE:
                break
            raise RuntimeError("max_levels reached")
        s = amg_ref.strength(cur, q["strength_theta"])
        agg, count = amg_ref.aggregate(s)
        if 10 * count > 9 * n:
            if n <= amg_ref.MAX_COARSE:
                break
            raise RuntimeError("stagnation")
        p = amg_ref.prolongator(cur, s, agg, count, q["prolongator_omega"])
        levels[-1].update(agg=agg, P=p)
        levels.append(dict(A=amg_ref.coarse_operator(cur, p)))
    ainv, shift = coarse_inverse(levels[-1]["A"].toarray())
    return levels, ainv, shift


class Cycle(amg_ref.Cycle):
    """z = Pi V Pi r: amg_ref's V-cycle (with Ainv from N3) between two projections on level 0."""

    def __call__(self, r):
        r = np.asarray(r, dtype=self.dtype)
        n = self.dtype(r.size)
        z = self._cycle(0, r - r.sum() / n)
        return z - z.sum() / n


# ---- the operators of the tests ---------------------------------------------------------------------------------------------
def neumann_box_graph(mesh, nx, ny, nz):
    return mesh.structured_box(nx, ny, nz, dirichlet=False)


def neumann_box(mesh, nx, ny, nz):
    """-Laplacian of the nx x ny x nz box without wall faces (alpha = -1, beta = 0): (graph, A)."""
    g = neumann_box_graph(mesh, nx, ny, nz)
    return g, mesh.assemble_csr(g, -1.0, 0.0).tocsr()[:, :g.n_cells]


def face_weight_matrix(g, w):
    """A = -M of StencilMatrix.from_face_weights(ctx, n, 0, g.inner, g.outer, w, w, None): a_ij = -w_f, a_ii = sum w_f."""
    nc = g.n_cells
    rows = np.concatenate([g.inner, g.outer, g.inner, g.outer])
    cols = np.concatenate([g.outer, g.inner, g.inner, g.outer])
    a = sp.coo_matrix((np.concatenate([-w, -w, w, w]), (rows, cols)), shape=(nc, nc)).tocsr()
    a.sum_duplicates()
    a.sort_indices()
    return a


def lognormal_weights(g, seed=11):
    return np.exp(np.random.default_rng(seed).standard_normal(g.inner.size))


def lognormal_box(mesh, nx=12, ny=10, nz=9):
    """(graph, face weights, A) of the Neumann box with weights exp(N(0, 1)) per face."""
    g = neumann_box_graph(mesh, nx, ny, nz)
    w = lognormal_weights(g)
    return g, w, face_weight_matrix(g, w)


def renumbered(a, seed=5):
    """Q A Q^T for a random permutation of the rows."""
    perm = np.random.default_rng(seed).permutation(a.shape[0])
    out = a.tocsr()[perm][:, perm].tocsr()
    out.sort_indices()
    return out


def graph_laplacian(seed=3):
    """The graph Laplacian D - W on the pattern of amg_cases.random_symmetric(seed), w_ij = |a_ij|."""
    a = amg_cases.random_symmetric(seed)
    w = abs(a - sp.diags(a.diagonal())).tocsr()
    w.eliminate_zeros()
    out = (sp.diags(np.asarray(w.sum(axis=1)).ravel()) - w).tocsr()
    out.sort_indices()
    return out


def mean_free(n, seed=8):
    b = np.random.default_rng(seed).standard_normal(n)
    return b - b.mean()


def plain_cg_count(a, b, rel_tol=1e-6, max_it=5000):
    """Iterations of unpreconditioned CG from x = 0 to ||r|| <= rel_tol ||b||."""
    return amg_ref.pcg(a, b, lambda r: r.copy(), rel_tol=rel_tol, abs_tol=0.0, max_it=max_it)[1]
