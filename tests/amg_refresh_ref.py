"""The frozen-structure recipe of include/storm_hip.h ("Refreshable hierarchies") restated in numpy / scipy, on top of
tests/amg_ref.py: one level's numbers from its current operator on a structure that is given -- the strong mask and the
aggregates -- instead of recomputed, and on patterns that depend on no value.  Nothing here calls the library."""
import os
import sys

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import amg_ref  # noqa: E402

EPS = np.finfo(np.float64).eps


def ones(m):
    """The stored pattern of m (stored zeros included) with every value 1."""
    m = sp.csr_matrix(m)
    if not m.has_sorted_indices:
        m = m.sorted_indices()
    return sp.csr_matrix((np.ones(m.indices.size), m.indices.copy(), m.indptr.copy()), shape=m.shape)


def on_pattern(m, pattern):
    """The values of m on the stored entries of `pattern` (0 where m stores nothing), columns sorted."""
    pattern = sp.csr_matrix(pattern)
    pattern.sort_indices()
    rows = np.repeat(np.arange(pattern.shape[0]), np.diff(pattern.indptr))
    vals = np.asarray(sp.csr_matrix(m)[rows, pattern.indices]).ravel() if pattern.indices.size else np.zeros(0)
    return sp.csr_matrix((vals.astype(np.float64), pattern.indices.copy(), pattern.indptr.copy()), shape=pattern.shape)


def mask_matrix(a, strong_mask):
    """The strong mask (one byte per stored entry of a) as a CSR matrix of ones on the strong entries."""
    a = sp.csr_matrix(a)
    keep = np.asarray(strong_mask, bool)
    rows = np.repeat(np.arange(a.shape[0]), np.diff(a.indptr))
    return sp.csr_matrix((np.ones(int(keep.sum())), (rows[keep], a.indices[keep])), shape=a.shape)


def strong_mask_of(a, s):
    """The mask of a's stored entries that the strength graph s (amg_ref.strength) calls strong."""
    a = sp.csr_matrix(a)
    rows = np.repeat(np.arange(a.shape[0]), np.diff(a.indptr))
    hit = np.asarray((s > 0).astype(np.float64).tocsr()[rows, a.indices]).ravel() > 0
    return (hit & (rows != a.indices)).astype(np.uint8)


def structural_patterns(a, strong_mask, agg, count, omega):
    """(pattern of P, pattern of A P, pattern of R (A P) with the diagonal), as matrices of ones."""
    n = a.shape[0]
    t = sp.csr_matrix((np.ones(n), (np.arange(n), agg)), shape=(n, count))
    if omega == 0.0:
        p = t
    else:
        p = ones(t + (mask_matrix(a, strong_mask) + sp.identity(n)) @ t)
    ap = ones(ones(a) @ p)
    nxt = ones(p.T @ ap + sp.identity(count))
    return p, ap, nxt


def frozen_level(a, strong_mask, agg, count, omega):
    """(P, A_next) of steps 2 to 5 of the frozen-structure recipe, on the structural patterns.  `a` is the level operator
    with its stored entries (zeros included), `strong_mask` one byte per stored entry."""
    a = sp.csr_matrix(a, dtype=np.float64)
    s = mask_matrix(a, strong_mask)
    p_pat, _, n_pat = structural_patterns(a, strong_mask, agg, count, omega)
    p = on_pattern(amg_ref.prolongator(a, s, agg, count, omega), p_pat)
    return p, on_pattern(p.T @ a @ p, n_pat)


def within(lib, ref, terms, magnitude, what):
    """|lib - ref| <= 8 eps terms magnitude entrywise, on the union of the patterns: the bound of a reordered sum."""
    bound = (8.0 * EPS) * sp.csr_matrix(terms).multiply(magnitude)
    excess = (abs(sp.csr_matrix(lib) - sp.csr_matrix(ref)) - bound).tocsr()
    worst = excess.max() if excess.nnz else 0.0
    assert worst <= 0.0, f"{what}: an entry is {worst:.3e} beyond the reordered-sum bound"


def prolongator_bound(a, strong_mask, agg, count, omega):
    """(terms, sum of |products|) of P = T - (omega / lambda_F) D_F^-1 A^F T: every sum behind an entry of row i -- the weak
    entries into the diagonal, the aggregate's columns -- has at most nnz(row i) + 1 terms."""
    a = sp.csr_matrix(a)
    n = a.shape[0]
    s = mask_matrix(a, strong_mask)
    t = sp.csr_matrix((np.ones(n), (np.arange(n), agg)), shape=(n, count))
    af, d = amg_ref.filtered(a, s)
    off = (a - sp.diags(a.diagonal())).tocsr()
    strong = off.multiply(s)
    weak_abs = np.asarray(abs(off - strong).sum(axis=1)).ravel()
    af_abs = abs(strong) + sp.diags(np.abs(a.diagonal()) + weak_abs)
    lam = (np.asarray(abs(af).sum(axis=1)).ravel() / np.abs(d)).max()
    magnitude = (t + sp.diags(np.abs((omega / lam) / d)) @ (af_abs @ t)).tocsr()
    terms = sp.diags(np.diff(a.indptr) + 1.0) @ ones(magnitude)
    return terms.tocsr(), magnitude


def coarse_bound(a, p):
    """(terms, sum of |products|) of P^T A P."""
    return (ones(p).T @ ones(a) @ ones(p)).tocsr(), (abs(p).T @ abs(a) @ abs(p)).tocsr()


def same_pattern(x, y):
    x, y = sp.csr_matrix(x), sp.csr_matrix(y)
    return x.shape == y.shape and np.array_equal(x.indptr, y.indptr) and np.array_equal(x.indices, y.indices)
