"""Reference arithmetic of the multigrid preconditioner's Jacobi smoother (include/storm_hip.h, "Non-symmetric operators:
the damped-Jacobi smoother"): the cycle restated in numpy / scipy on the hierarchy of tests/amg_ref.py, the non-symmetric
cases (first-order upwind convection-diffusion from mesh.convection_diffusion_weights, a random row-dominant CSR operator)
beside those of tests/amg_cases.py, and a right-preconditioned restarted GMRES.  Nothing here calls the library."""
import os
import sys

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import amg_ref  # noqa: E402
import cheb_ref  # noqa: E402

NU, VEL = 1e-2, (1.0, 0.5, 0.25)  # BASELINE config 4
OMEGA = 2.0 / 3.0


def convdiff_box(mesh, nx, ny=None, nz=None, nu=NU, vel=VEL):
    """A = -nu L + C(v) on the library's own box mesh: (graph, (w_inner, w_outer, diag_extra), assembled A).  The weights go
    to StencilMatrix.from_face_weights and are applied with alpha = 1, beta = 0:
    (A x)_i = sum_f w_if (x_other - x_i) + diag_extra_i x_i."""
    g = mesh.structured_box(nx, ny, nz)
    wi, wo, de = mesh.convection_diffusion_weights(g, nu, vel)
    n = g.n_cells
    rows = np.concatenate([g.inner, g.outer, g.inner, g.outer, np.arange(n)])
    cols = np.concatenate([g.outer, g.inner, g.inner, g.outer, np.arange(n)])
    vals = np.concatenate([wi, wo, -wi, -wo, de])
    a = sp.coo_matrix((vals, (rows, cols)), shape=(n, n)).tocsr()
    a.sum_duplicates()
    a.sort_indices()
    return g, (wi, wo, de), a


def random_nonsymmetric(seed=3):
    """tests/amg_cases.random_symmetric without the symmetrisation: a random non-symmetric, row-dominant CSR operator (918
    rows at seed 3)."""
    rng = np.random.default_rng(100 + seed)
    n = int(rng.integers(200, 1500))
    nnz_row = int(rng.integers(2, 9))
    rows = np.repeat(np.arange(n), nnz_row)
    cols = (rows + rng.integers(1, n, size=rows.size)) % n
    off = sp.coo_matrix((rng.uniform(-1.0, 1.0, rows.size), (rows, cols)), shape=(n, n)).tocsr()
    off.sum_duplicates()
    return (off + sp.diags(np.abs(off).sum(axis=1).A1 * 1.5 + 1.0)).tocsr()


class JacobiCycle(amg_ref.Cycle):
    """z = B r with `sweeps` damped Jacobi sweeps before and after the coarse correction, sigma_l = 2 omega / lmax with
    Gershgorin's lmax of diag(s) A_l (a float64 number, as the library's), in `dtype` arithmetic."""

    def __init__(self, ops, prolongators, inverse, sweeps=2, omega=OMEGA, dtype=np.float64):
        self.dtype = dtype
        self.ops = [sp.csr_matrix(a) for a in ops]
        self.ps = [sp.csr_matrix(p) for p in prolongators]
        self.inverse = np.asarray(inverse, dtype=dtype)
        self.sweeps = sweeps
        self.scale, self.sigma = [], []
        for a in self.ops[:-1]:
            s = 1.0 / a.diagonal()
            self.scale.append(s.astype(dtype))
            self.sigma.append(2.0 * omega / cheb_ref.gershgorin(a, s))

    def sweep(self, lv, r, z):
        return z + self.dtype(self.sigma[lv]) * (self.scale[lv] * (r - self._mul(self.ops[lv], z)))

    def _cycle(self, lv, r):
        if lv == len(self.ops) - 1:
            return self.inverse @ r
        a, p = self.ops[lv], self.ps[lv]
        z = self.dtype(self.sigma[lv]) * (self.scale[lv] * r)
        for _ in range(self.sweeps - 1):
            z = self.sweep(lv, r, z)
        t = r - self._mul(a, z)
        z = z + self._mul(p, self._cycle(lv + 1, self._mul(p.T.tocsr(), t)))
        for _ in range(self.sweeps):
            z = self.sweep(lv, r, z)
        return z


def cycles(a, sweeps=2, omega=OMEGA, degree=2, **params):
    """(levels, the Jacobi cycle, the Chebyshev cycle) on amg_ref.hierarchy(a, **params)."""
    levels, inverse = amg_ref.hierarchy(a, **params)
    ops, ps = [lv["A"] for lv in levels], [lv["P"] for lv in levels[:-1]]
    return levels, JacobiCycle(ops, ps, inverse, sweeps, omega), amg_ref.Cycle(ops, ps, inverse, degree=degree)


def gmres_right(a, b, precond=None, restart=30, rel_tol=1e-6, abs_tol=1e-6, max_it=300):
    """Restarted GMRES on A B u = b, x = B u, from x = 0 (modified Gram-Schmidt, Givens rotations); stops when the residual
    estimate is <= abs_tol or <= rel_tol ||b||.  Returns (x, inner iterations, converged)."""
    precond = precond if precond is not None else (lambda v: v)
    n = b.size
    x = np.zeros(n)
    r0 = np.linalg.norm(b)
    it = 0
    while True:
        r = b - a @ x
        beta = np.linalg.norm(r)
        if beta <= abs_tol or beta <= rel_tol * r0:
            return x, it, True
        if it >= max_it:
            return x, it, False
        q = np.zeros((restart + 1, n))
        h = np.zeros((restart + 1, restart))
        cs, sn, g = np.zeros(restart), np.zeros(restart), np.zeros(restart + 1)
        q[0], g[0] = r / beta, beta
        k = 0
        while k < restart and it < max_it:
            w = a @ precond(q[k])
            for j in range(k + 1):
                h[j, k] = q[j] @ w
                w = w - h[j, k] * q[j]
            h[k + 1, k] = np.linalg.norm(w)
            if h[k + 1, k] > 0:
                q[k + 1] = w / h[k + 1, k]
            for j in range(k):
                h[j, k], h[j + 1, k] = cs[j] * h[j, k] + sn[j] * h[j + 1, k], -sn[j] * h[j, k] + cs[j] * h[j + 1, k]
            rho = np.hypot(h[k, k], h[k + 1, k])
            cs[k], sn[k] = h[k, k] / rho, h[k + 1, k] / rho
            h[k, k], h[k + 1, k] = rho, 0.0
            g[k + 1], g[k] = -sn[k] * g[k], cs[k] * g[k]
            k += 1
            it += 1
            if abs(g[k]) <= abs_tol or abs(g[k]) <= rel_tol * r0:
                break
        y = np.linalg.solve(np.triu(h[:k, :k]), g[:k])
        x = x + precond(q[:k].T @ y)
