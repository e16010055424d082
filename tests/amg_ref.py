"""Reference arithmetic of the multigrid preconditioner's tests: the recipe of include/storm_hip.h ("Smoothed-aggregation
multigrid preconditioner") and its V-cycle restated in numpy / scipy, the smoother from tests/cheb_ref.py.  Nothing here
calls the library.  The aggregation is the three sequential passes of the recipe as plain loops: it is meant to be read
beside the header, not to be fast."""
import os
import sys

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cheb_ref  # noqa: E402

DEFAULTS = dict(strength_theta=0.25, prolongator_omega=4.0 / 3.0, smoother_degree=2, smoother_ratio=30.0, max_levels=10,
                coarse_rows=512, reduced_records=0)
MAX_COARSE = 1024


def normalise(a):
    """CSR with sorted columns, duplicates merged, exact zeros dropped and an explicit diagonal."""
    a = sp.csr_matrix(a, dtype=np.float64)
    a.sum_duplicates()
    a.eliminate_zeros()
    n = a.shape[0]
    c = a.tocoo()
    have = np.zeros(n, bool)
    have[c.row[c.row == c.col]] = True
    miss = np.flatnonzero(~have)
    # an explicit zero survives the COO -> CSR conversion (only sum_duplicates / eliminate_zeros would touch it)
    out = sp.coo_matrix((np.concatenate([c.data, np.zeros(miss.size)]), (np.concatenate([c.row, miss]),
                                                                          np.concatenate([c.col, miss]))), shape=a.shape).tocsr()
    out.sort_indices()
    return out


def strength(a, theta):
    """The strong graph as CSR of weights on the union of the patterns of A and A^T (step 1)."""
    n = a.shape[0]
    off = (a - sp.diags(a.diagonal())).tocsr()
    off.eliminate_zeros()
    ab = abs(off).tocsr()
    m = np.zeros(n)
    rows = np.repeat(np.arange(n), np.diff(ab.indptr))
    np.maximum.at(m, rows, ab.data)
    own = sp.csr_matrix(((ab.data >= theta * m[rows]).astype(np.float64), ab.indices.copy(), ab.indptr.copy()), shape=a.shape)
    own.eliminate_zeros()
    strong = ((own + own.T) > 0).astype(np.float64)
    weight = ab.maximum(ab.T).multiply(strong).tocsr()
    weight.sort_indices()
    return weight


def aggregate(s):
    """Step 2: (aggregate of every row, number of aggregates)."""
    n = s.shape[0]
    ptr, col, w = s.indptr, s.indices, s.data
    agg = np.full(n, -1, np.int64)
    count = 0
    for i in range(n):  # pass 1
        nb = col[ptr[i]:ptr[i + 1]]
        if nb.size and agg[i] < 0 and (agg[nb] < 0).all():
            agg[i] = count
            agg[nb] = count
            count += 1
    after1 = agg.copy()
    for i in range(n):  # pass 2
        if after1[i] >= 0:
            continue
        best, wbest = -1, -1.0
        for k in range(ptr[i], ptr[i + 1]):
            if after1[col[k]] >= 0 and w[k] > wbest:  # (columns ascend: a tie keeps the lowest)
                best, wbest = col[k], w[k]
        if best >= 0:
            agg[i] = after1[best]
    for i in range(n):  # pass 3
        if agg[i] >= 0:
            continue
        agg[i] = count
        nb = col[ptr[i]:ptr[i + 1]]
        agg[nb[agg[nb] < 0]] = count
        count += 1
    return agg, count


def filtered(a, s):
    """Step 3."""
    pattern = (s > 0).astype(np.float64)
    off = (a - sp.diags(a.diagonal())).tocsr()
    strong = off.multiply(pattern).tocsr()
    weak = (off - strong).tocsr()
    d = a.diagonal() + np.asarray(weak.sum(axis=1)).ravel()
    return (strong + sp.diags(d)).tocsr(), d


def prolongator(a, s, agg, count, omega):
    """Step 4."""
    n = a.shape[0]
    t = sp.csr_matrix((np.ones(n), (np.arange(n), agg)), shape=(n, count))
    if omega == 0.0:
        return t
    af, d = filtered(a, s)
    if (d == 0.0).any():
        raise ZeroDivisionError("a zero diagonal of the filtered matrix")
    lam = (np.asarray(abs(af).sum(axis=1)).ravel() / np.abs(d)).max()
    p = (t - sp.diags((omega / lam) / d) @ (af @ t)).tocsr()
    p.eliminate_zeros()
    p.sort_indices()
    return p


def coarse_operator(a, p):
    """Step 5."""
    return normalise(p.T @ a @ p)


def one_level(a, theta=0.25, omega=4.0 / 3.0):
    """(aggregates, their number, P, the next operator) of one level operator."""
    s = strength(a, theta)
    agg, count = aggregate(s)
    p = prolongator(a, s, agg, count, omega)
    return agg, count, p, coarse_operator(a, p)


def hierarchy(a, **params):
    """The whole setup: a list of levels dict(A=, agg=, P=) (the coarsest has A only) and the dense inverse."""
    q = dict(DEFAULTS, **params)
    levels = [dict(A=normalise(a))]
    while True:
        cur = levels[-1]["A"]
        n = cur.shape[0]
        if n <= q["coarse_rows"]:
            break
        if len(levels) >= q["max_levels"]:
            if n <= MAX_COARSE:
                break
            raise RuntimeError("max_levels reached")
        s = strength(cur, q["strength_theta"])
        agg, count = aggregate(s)
        if 10 * count > 9 * n:
            if n <= MAX_COARSE:
                break
            raise RuntimeError("stagnation")
        p = prolongator(cur, s, agg, count, q["prolongator_omega"])
        levels[-1].update(agg=agg, P=p)
        levels.append(dict(A=coarse_operator(cur, p)))
    return levels, np.linalg.inv(levels[-1]["A"].toarray())


def complexity(levels):
    return sum(lv["A"].nnz for lv in levels) / levels[0]["A"].nnz


class Cycle:
    """z = B r on given level operators A_l, prolongators P_l and coarse inverse (the library's exported ones, or
    `hierarchy`'s), in `dtype` arithmetic (np.float64, or np.longdouble as the measure of the float64 cycle's rounding)."""

    def __init__(self, ops, prolongators, inverse, degree=2, ratio=30.0, dtype=np.float64):
        self.dtype = dtype
        self.ops = [sp.csr_matrix(a) for a in ops]
        self.ps = [sp.csr_matrix(p) for p in prolongators]
        self.inverse = np.asarray(inverse, dtype=dtype)
        self.smooth = []
        for a in self.ops[:-1]:
            s = 1.0 / a.diagonal()
            lmax = cheb_ref.gershgorin(a, s)  # bounds and coefficients stay float64 numbers: the library's are
            self.smooth.append((s.astype(dtype), cheb_ref.coefficients(lmax / ratio, lmax, degree)))

    def _mul(self, m, x):
        if self.dtype == np.float64:
            return m @ x
        out = np.zeros(m.shape[0], self.dtype)  # scipy has no long double kernels
        rows = np.repeat(np.arange(m.shape[0]), np.diff(m.indptr))
        np.add.at(out, rows, m.data.astype(self.dtype) * x[m.indices])
        return out

    def _smoother(self, lv, r):
        s, (theta, c1, c2) = self.smooth[lv]
        a = self.ops[lv]
        d = (s * r) / self.dtype(theta)
        z, res = d.copy(), r.copy()
        for k in range(len(c1)):
            res = res - self._mul(a, d)
            d = self.dtype(c1[k]) * d + self.dtype(c2[k]) * (s * res)
            z = z + d
        return z

    def _cycle(self, lv, r):
        if lv == len(self.ops) - 1:
            return self.inverse @ r
        a, p = self.ops[lv], self.ps[lv]
        z = self._smoother(lv, r)
        t = r - self._mul(a, z)
        zc = self._cycle(lv + 1, self._mul(p.T.tocsr(), t))
        z = z + self._mul(p, zc)
        t = r - self._mul(a, z)
        return z + self._smoother(lv, t)

    def __call__(self, r):
        return self._cycle(0, np.asarray(r, dtype=self.dtype))


def pcg(a, b, precond, rel_tol=1e-6, abs_tol=1e-6, max_it=2000):
    """Preconditioned CG from x = 0; stops when ||r|| <= abs_tol or ||r|| <= rel_tol ||r_0|| (the library's test, on the
    true-residual recurrence).  Returns (x, iterations)."""
    x = np.zeros_like(b)
    r = b.copy()
    z = precond(r)
    p = z.copy()
    rz = r @ z
    r0 = np.linalg.norm(r)
    for it in range(1, max_it + 1):
        ap = a @ p
        alpha = rz / (p @ ap)
        x = x + alpha * p
        r = r - alpha * ap
        rn = np.linalg.norm(r)
        if rn <= abs_tol or rn <= rel_tol * r0:
            return x, it
        z = precond(r)
        rz_new = r @ z
        p = z + (rz_new / rz) * p
        rz = rz_new
    return x, max_it
