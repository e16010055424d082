"""The host setup of the multigrid preconditioner (storm_hip_amg_setup_csr, csrc/amg_setup.hip) against the numpy / scipy
restatement of the recipe (tests/amg_ref.py), without a device.

Level by level, with the LIBRARY'S exported A_l as each level's input (a last-place difference in a coarse operator then
cannot flip a threshold comparison of the next level):
  * aggregate ids equal exactly;
  * P_l and A_{l+1} entrywise within 8 eps (terms in the sum) (sum of |products|), the bound of a reordered sum;
  * the level sizes of the 7-point boxes are the pinned ones;
  * the coarsest level's inverse inverts, the export format holds (sorted columns, explicit diagonal, no stored zeros);
  * refusals: a singular coarsest level, stagnation, max_levels, a zero filtered diagonal, parameters out of range."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import amg_cases  # noqa: E402
import amg_ref  # noqa: E402

EPS = np.finfo(np.float64).eps
E_INVALID, E_UNSUPPORTED = -1, -6


@pytest.fixture(scope="module")
def api():
    from stormruler_amd import api

    return api


def _case(name):
    from stormruler_amd import mesh

    if name.startswith("box"):
        return amg_cases.poisson_box(int(name[3:])), dict(coarse_rows=32 if name in ("box13", "box20") else 512)
    if name == "meshbox13":
        return amg_cases.mesh_box(mesh, 13)[1], dict(coarse_rows=32)
    if name in ("aniso", "lognormal"):
        return amg_cases.face_weight_case(mesh, 16, name)[3], {}
    assert name == "random"
    return amg_cases.random_symmetric(), dict(coarse_rows=32)


_cache = {}


def _hierarchy(api, name):
    if name not in _cache:
        a, params = _case(name)
        _cache[name] = (a, params, api.AmgHierarchy.from_csr(a, **params))
    return _cache[name]


def _ones(m):
    return sp.csr_matrix((np.ones(m.nnz), m.indices, m.indptr), shape=m.shape)


def _within(lib, ref, terms, magnitude, what):
    """|lib - ref| <= 8 eps terms magnitude entrywise, on the union of the patterns."""
    bound = (8.0 * EPS) * terms.multiply(magnitude)
    excess = (abs(lib - ref) - bound).tocsr()
    worst = excess.max() if excess.nnz else 0.0
    assert worst <= 0.0, f"{what}: an entry is {worst:.3e} beyond the reordered-sum bound"


def _prolongator_bound(a, s, agg, count, omega):
    """(terms, sum of |products|) of P = T - (omega / lambda_F) D_F^-1 A^F T: every sum behind an entry of row i -- the weak
    entries into the diagonal, the aggregate's columns -- has at most nnz(row i) + 1 terms."""
    n = a.shape[0]
    t = sp.csr_matrix((np.ones(n), (np.arange(n), agg)), shape=(n, count))
    af, d = amg_ref.filtered(a, s)
    off = (a - sp.diags(a.diagonal())).tocsr()
    strong = off.multiply((s > 0).astype(np.float64))
    weak_abs = np.asarray(abs(off - strong).sum(axis=1)).ravel()
    af_abs = abs(strong) + sp.diags(np.abs(a.diagonal()) + weak_abs)
    lam = (np.asarray(abs(af).sum(axis=1)).ravel() / np.abs(d)).max()
    magnitude = (t + sp.diags(np.abs((omega / lam) / d)) @ (af_abs @ t)).tocsr()
    terms = sp.diags(np.diff(a.indptr) + 1.0) @ _ones(magnitude)
    return terms.tocsr(), magnitude


CASES = ["box13", "box20", "box24", "meshbox13", "aniso", "lognormal", "random"]


@pytest.mark.parametrize("name", CASES)
def test_every_level_against_the_restatement(api, name):
    a, params, h = _hierarchy(api, name)
    q = dict(amg_ref.DEFAULTS, **params)
    assert h.levels >= 2
    a0 = h.operator(0)
    assert abs(a0 - amg_ref.normalise(a)).max() == 0.0  # level 0 is the caller's matrix
    for lv in range(h.levels):
        al = h.operator(lv)
        n = al.shape[0]
        assert al.has_sorted_indices and (np.diff(al.indptr) > 0).all()
        rows = np.repeat(np.arange(n), np.diff(al.indptr))
        assert (al.data[rows != al.indices] != 0.0).all(), "a stored off-diagonal zero"
        assert np.array_equal(np.sort(al.indices[rows == al.indices]), np.arange(n)), "the diagonal is not explicit"
        # duplicates would show as a repeated column in a row
        assert (np.diff(al.indices)[np.diff(rows) == 0] > 0).all()
        if lv == h.levels - 1:
            break
        s = amg_ref.strength(al, q["strength_theta"])
        agg, count = amg_ref.aggregate(s)
        assert np.array_equal(h.aggregates(lv), agg), f"level {lv}: aggregates differ"
        assert h.sizes(lv)[2] == count == h.sizes(lv + 1)[0]
        p_lib, p_ref = h.prolongator(lv), amg_ref.prolongator(al, s, agg, count, q["prolongator_omega"])
        assert p_lib.has_sorted_indices and (p_lib.data != 0.0).all()
        terms, magnitude = _prolongator_bound(al, s, agg, count, q["prolongator_omega"])
        _within(p_lib, p_ref, terms, magnitude, f"{name} P_{lv}")
        # the coarse operator of the library's own P (held to the restatement's above)
        c_ref = amg_ref.coarse_operator(al, p_lib)
        c_terms = (_ones(p_lib).T @ _ones(al) @ _ones(p_lib)).tocsr()
        c_mag = (abs(p_lib).T @ abs(al) @ abs(p_lib)).tocsr()
        _within(h.operator(lv + 1), c_ref, c_terms, c_mag, f"{name} A_{lv + 1}")
    # the coarsest level: n <= coarse_rows, and its inverse
    ac = h.operator(h.levels - 1).toarray()
    assert ac.shape[0] <= q["coarse_rows"]
    inv = h.coarse_inverse()
    m = ac.shape[0]
    # Gauss-Jordan with partial pivoting: a residual of order m eps cond(A) (Higham, Accuracy and Stability, section 14.4)
    assert np.abs(inv @ ac - np.eye(m)).max() <= 64 * m * EPS * np.linalg.cond(ac)
    assert h.get("levels") == h.levels
    assert abs(h.get("operator_complexity") - sum(h.sizes(lv)[1] for lv in range(h.levels)) / a0.nnz) < 1e-12
    assert abs(h.get("grid_complexity") - sum(h.level_rows()) / a0.shape[0]) < 1e-12
    assert h.get("setup_seconds") > 0.0


@pytest.mark.parametrize("name,sizes", [("box13", [2197, 280, 16]), ("box20", [8000, 1040, 50, 7]),
                                        ("box24", [13824, 1685, 72])])
def test_level_sizes_of_the_boxes(api, name, sizes):
    a, params, h = _hierarchy(api, name)
    assert h.level_rows() == sizes
    levels, _ = amg_ref.hierarchy(a, **params)  # the restatement on its own coarse operators agrees
    assert [lv["A"].shape[0] for lv in levels] == sizes


def test_filtered_smoothing_keeps_the_anisotropic_hierarchy_sparse(api):
    a, params, h = _hierarchy(api, "aniso")
    levels, _ = amg_ref.hierarchy(a, **params)
    ref = amg_ref.complexity(levels)
    print(f"1 : 1 : 100 weights: levels {h.level_rows()}, operator complexity {h.get('operator_complexity'):.4f} "
          f"(restatement {ref:.4f})")
    assert h.get("operator_complexity") <= 1.01 * ref
    assert ref < 2.5  # (smoothing with the full matrix reaches 8.6 here)


def test_one_row_coarsest_level(api):
    a, params, h = _hierarchy(api, "random")
    assert h.level_rows() == [918, 69, 1]
    assert h.coarse_inverse().shape == (1, 1)
    assert h.coarse_inverse()[0, 0] == 1.0 / h.operator(2)[0, 0]


def test_unsmoothed_prolongator_is_the_aggregates_indicator(api):
    a = amg_cases.poisson_box(13)
    h = api.AmgHierarchy.from_csr(a, coarse_rows=32, prolongator_omega=0.0)
    for lv in range(h.levels - 1):
        p, agg = h.prolongator(lv), h.aggregates(lv)
        assert (p.data == 1.0).all() and np.array_equal(p.indices, agg) and np.array_equal(np.diff(p.indptr), np.ones(agg.size))


def test_unsorted_input_with_duplicates_is_merged(api):
    a = amg_cases.poisson_box(7).tocoo()
    rng = np.random.default_rng(5)
    perm = rng.permutation(a.nnz)
    half = a.data[perm] * 0.5  # every entry twice, in a scrambled order: halves sum exactly
    rows, cols = np.concatenate([a.row[perm], a.row[perm]]), np.concatenate([a.col[perm], a.col[perm]])
    order = np.argsort(rows, kind="stable")
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=a.shape[0]))]).astype(np.int64)
    raw = sp.csr_matrix((np.concatenate([half, half])[order], cols[order], rp), shape=a.shape)
    h1, h2 = api.AmgHierarchy.from_csr(raw, coarse_rows=32), api.AmgHierarchy.from_csr(a.tocsr(), coarse_rows=32)
    assert h1.level_rows() == h2.level_rows()
    for lv in range(h1.levels):
        assert abs(h1.operator(lv) - h2.operator(lv)).max() == 0.0


def _setup_status(a, **params):
    from stormruler_amd import _lib, api

    a = sp.csr_matrix(a)
    rp, col, val = a.indptr.astype(np.int64), a.indices.astype(np.int64), a.data.astype(np.float64)
    h = C.c_void_p()
    p = api._amg_params(**params)
    st = _lib.lib.storm_hip_amg_setup_csr(a.shape[0], rp.ctypes.data_as(_lib.i64p), col.ctypes.data_as(_lib.i64p),
                                          val.ctypes.data_as(_lib.f64p), C.byref(p), C.byref(h))
    msg = _lib.lib.storm_hip_last_error().decode()
    if st == 0:
        _lib.lib.storm_hip_amg_hierarchy_destroy(h)
    else:
        assert not h.value
    return st, msg


def test_refusals():
    # a singular coarsest level: the pure-Neumann Laplacian of two cells
    st, msg = _setup_status(np.array([[1.0, -1.0], [-1.0, 1.0]]))
    assert st == E_INVALID and "singular" in msg and "Neumann" in msg
    # ... and below a hierarchy: Neumann on a 1-d chain, exactly representable weights
    n = 40
    chain = sp.diags([-np.ones(n - 1), np.r_[1.0, 2.0 * np.ones(n - 2), 1.0], -np.ones(n - 1)], [-1, 0, 1]).tocsr()
    st, msg = _setup_status(chain, coarse_rows=1, prolongator_omega=0.0)
    assert st == E_INVALID and "singular" in msg
    # stagnation: nothing is strongly connected, every row is its own aggregate
    st, msg = _setup_status(sp.identity(2000).tocsr())
    assert st == E_UNSUPPORTED and "stagnates" in msg and "2000" in msg
    # ... with few enough rows the stagnant level is the (dense) coarsest one
    st, msg = _setup_status(sp.identity(600).tocsr())
    assert st == 0
    # max_levels reached above what a dense level holds
    st, msg = _setup_status(amg_cases.poisson_box(20), coarse_rows=32, max_levels=2)
    assert st == E_UNSUPPORTED and "max_levels" in msg and "8000 / 1040" in msg
    st, msg = _setup_status(amg_cases.poisson_box(13), coarse_rows=32, max_levels=2)
    assert st == 0
    # a zero diagonal of the filtered matrix
    st, msg = _setup_status(np.array([[0.0, 1.0], [1.0, 0.0]]), coarse_rows=1)
    assert st == E_INVALID and "zero diagonal" in msg
    # parameters out of range
    small = amg_cases.poisson_box(4)
    for bad in (dict(smoother_degree=0), dict(smoother_degree=17), dict(coarse_rows=0), dict(coarse_rows=1025),
                dict(max_levels=0), dict(strength_theta=-0.5), dict(prolongator_omega=float("nan")), dict(smoother_ratio=1.0),
                dict(reduced_records=2)):
        st, msg = _setup_status(small, **bad)
        assert st == E_INVALID and list(bad)[0] in msg, (bad, st, msg)
    # malformed CSR
    from stormruler_amd import _lib

    h = C.c_void_p()
    rp = np.array([0, 1], np.int64)
    col = np.array([3], np.int64)
    val = np.array([1.0])
    assert _lib.lib.storm_hip_amg_setup_csr(1, rp.ctypes.data_as(_lib.i64p), col.ctypes.data_as(_lib.i64p),
                                            val.ctypes.data_as(_lib.f64p), None, C.byref(h)) == E_INVALID
    assert b"column" in _lib.lib.storm_hip_last_error()


def test_defaults():
    from stormruler_amd import _lib

    p = _lib.AmgParams()
    _lib.lib.storm_hip_amg_params_default(C.byref(p))
    assert (p.strength_theta, p.prolongator_omega, p.smoother_degree, p.smoother_ratio, p.max_levels, p.coarse_rows,
            p.reduced_records) == (0.25, 4.0 / 3.0, 2, 30.0, 10, 512, 0)
