"""The structural host setup of the multigrid preconditioner (storm_hip_amg_setup_csr_structural, csrc/amg_setup.hip) -- the
setup whose patterns depend on no value, which a refreshable object freezes -- against the restatement of the
frozen-structure recipe (tests/amg_refresh_ref.py), without a device.

Level by level, with the library's exported A_l as each level's input:
  * aggregates equal exactly, the strong mask equal to the pattern of amg_ref.strength;
  * P_l and A_{l+1} within 8 eps (terms) (sum of |products|) of frozen_level, the bound of a reordered sum;
  * the patterns of P_l and A_{l+1} are the structural products of the patterns;
  * where the plain setup drops no zero (lognormal, aniso) the two hierarchies are equal bit for bit; on the 13^3 box the
    structural one is the plain one plus stored zeros;
  * a stored zero of the caller's CSR stays at level 0;
  * refusals and null arguments of the new entry points."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import amg_cases  # noqa: E402
import amg_ref  # noqa: E402
import amg_refresh_ref as rr  # noqa: E402

E_INVALID, E_UNSUPPORTED = -1, -6


@pytest.fixture(scope="module")
def api():
    from stormruler_amd import api

    return api


def _case(name):
    from stormruler_amd import mesh

    if name.startswith("box"):
        return amg_cases.poisson_box(int(name[3:])), dict(coarse_rows=32)
    if name in ("aniso", "lognormal"):
        return amg_cases.face_weight_case(mesh, 16, name)[3], {}
    assert name == "random"
    return amg_cases.random_symmetric(), dict(coarse_rows=32)


_cache = {}


def _hierarchies(api, name):
    """(A, parameters, structural hierarchy, plain hierarchy) of a case, computed once."""
    if name not in _cache:
        a, params = _case(name)
        _cache[name] = (a, params, api.AmgHierarchy.from_csr(a, structural=True, **params), api.AmgHierarchy.from_csr(a, **params))
    return _cache[name]


CASES = ["box13", "box20", "lognormal", "aniso", "random"]


@pytest.mark.parametrize("name", CASES)
def test_every_level_against_the_frozen_restatement(api, name):
    a, params, h, plain = _hierarchies(api, name)
    q = dict(amg_ref.DEFAULTS, **params)
    omega = q["prolongator_omega"]
    assert h.get("structural") == 1.0 and plain.get("structural") == 0.0
    assert h.levels >= 2 and h.level_rows() == plain.level_rows()
    a0 = h.operator(0)
    assert abs(a0 - amg_ref.normalise(a)).max() == 0.0
    for lv in range(h.levels - 1):
        al = h.operator(lv)
        assert al.has_sorted_indices
        s = amg_ref.strength(al, q["strength_theta"])
        agg, count = amg_ref.aggregate(s)
        assert np.array_equal(h.aggregates(lv), agg), f"level {lv}: aggregates differ"
        mask = h.strong(lv)
        assert mask.dtype == np.uint8 and mask.size == al.nnz
        assert np.array_equal(mask, rr.strong_mask_of(al, s)), f"level {lv}: the strong mask differs from the strength graph"
        p_ref, c_ref = rr.frozen_level(al, mask, agg, count, omega)
        p_pat, _, n_pat = rr.structural_patterns(al, mask, agg, count, omega)
        p_lib, c_lib = h.prolongator(lv), h.operator(lv + 1)
        assert rr.same_pattern(p_lib, p_pat), f"level {lv}: P is not on the pattern of T u A^F T"
        assert rr.same_pattern(c_lib, n_pat), f"level {lv + 1}: A is not on the structural pattern of R (A P)"
        rr.within(p_lib, p_ref, *rr.prolongator_bound(al, mask, agg, count, omega), f"{name} P_{lv}")
        # the coarse operator of the library's own P (held to the restatement's above)
        rr.within(c_lib, rr.on_pattern(p_lib.T @ al @ p_lib, n_pat), *rr.coarse_bound(al, p_lib), f"{name} A_{lv + 1}")
        assert rr.same_pattern(c_ref, c_lib) and rr.same_pattern(p_ref, p_lib)
        # the plain hierarchy's mask is the same function of its own operator
        assert np.array_equal(plain.strong(lv), rr.strong_mask_of(plain.operator(lv), amg_ref.strength(plain.operator(lv), q["strength_theta"])))
    ac = h.operator(h.levels - 1).toarray()
    m = ac.shape[0]
    assert np.abs(h.coarse_inverse() @ ac - np.eye(m)).max() <= 64 * m * rr.EPS * np.linalg.cond(ac)


@pytest.mark.parametrize("name", ["lognormal", "aniso"])
def test_equal_to_the_plain_hierarchy_where_no_zero_is_dropped(api, name):
    a, params, h, plain = _hierarchies(api, name)
    for lv in range(h.levels):
        x, y = h.operator(lv), plain.operator(lv)
        assert rr.same_pattern(x, y) and np.array_equal(x.data, y.data), f"A_{lv}"
        if lv + 1 < h.levels:
            x, y = h.prolongator(lv), plain.prolongator(lv)
            assert rr.same_pattern(x, y) and np.array_equal(x.data, y.data), f"P_{lv}"
            assert np.array_equal(h.strong(lv), plain.strong(lv)) and np.array_equal(h.aggregates(lv), plain.aggregates(lv))
    assert np.array_equal(h.coarse_inverse(), plain.coarse_inverse())


def test_the_box_keeps_the_entries_that_cancel(api):
    a, params, h, plain = _hierarchies(api, "box13")
    assert h.level_rows() == plain.level_rows() == [2197, 280, 16]
    grew = 0
    for lv in range(h.levels):
        pairs = [(h.operator(lv), plain.operator(lv))]
        if lv + 1 < h.levels:
            pairs.append((h.prolongator(lv), plain.prolongator(lv)))
            assert np.array_equal(h.aggregates(lv), plain.aggregates(lv))
        for x, y in pairs:
            assert x.nnz >= y.nnz
            grew += x.nnz - y.nnz
            on_plain = rr.on_pattern(x, y)
            assert np.array_equal(on_plain.data, y.data), f"level {lv}: a value differs on the plain pattern"
            assert (rr.ones(x) - rr.ones(y)).min() >= 0.0, f"level {lv}: the plain pattern is not inside the structural one"
            assert np.count_nonzero(x.data) == np.count_nonzero(y.data), f"level {lv}: an extra entry is not a stored zero"
    assert h.sizes(1)[1] == 6410 and plain.sizes(1)[1] == 6408  # A_1: two entries cancel exactly
    assert grew >= 2
    assert np.array_equal(h.coarse_inverse(), plain.coarse_inverse())


def test_a_stored_zero_stays_at_level_0(api):
    a = amg_cases.poisson_box(7).tolil()
    a[0, 300] = 1.0
    a[300, 0] = 1.0
    a[5, 320] = 1.0  # (no transpose entry)
    a = a.tocsr()
    a.sort_indices()
    at = np.repeat(np.arange(a.shape[0]), np.diff(a.indptr))
    a.data[((at == 0) & (a.indices == 300)) | ((at == 5) & (a.indices == 320))] = 0.0  # stored, zero
    assert a.nnz == amg_cases.poisson_box(7).nnz + 3
    # duplicates still merge: every entry twice, as halves
    rows = np.repeat(np.arange(a.shape[0]), np.diff(a.indptr))
    order = np.argsort(np.concatenate([rows, rows]), kind="stable")
    rp = np.concatenate([[0], np.cumsum(2 * np.diff(a.indptr))]).astype(np.int64)
    twice = sp.csr_matrix((np.concatenate([a.data, a.data])[order] * 0.5, np.concatenate([a.indices, a.indices])[order], rp), shape=a.shape)
    for m in (a, twice):
        hs = api.AmgHierarchy.from_csr(m, structural=True, coarse_rows=32)
        hp = api.AmgHierarchy.from_csr(m, coarse_rows=32)
        a0 = hs.operator(0)
        assert a0.nnz == a.nnz and rr.same_pattern(a0, a) and np.array_equal(a0.data, a.data)
        assert hp.operator(0).nnz == a.nnz - 2

        def entry(i, j):
            return int(np.flatnonzero((at == i) & (a0.indices == j))[0])

        mask = hs.strong(0)
        assert a0.data[entry(5, 320)] == 0.0 and mask[entry(5, 320)] == 0  # a zero entry is never strong by itself ...
        # ... but the mask is that of the PAIR: the transpose's value makes (0, 300) strong in both rows
        assert a0.data[entry(0, 300)] == 0.0 and mask[entry(0, 300)] == 1 and mask[entry(300, 0)] == 1
        assert np.array_equal(mask, rr.strong_mask_of(a0, amg_ref.strength(a0, 0.25)))


def test_refusals_and_null_arguments():
    from stormruler_amd import _lib

    lib = _lib.lib
    for name in ("storm_hip_amg_setup_csr_structural", "storm_hip_amg_hierarchy_get_strong", "storm_hip_amg_create_refreshable",
                 "storm_hip_amg_refresh", "storm_hip_amg_download"):
        assert name in _lib.SIGNATURES
    h = C.c_void_p()
    assert lib.storm_hip_amg_setup_csr_structural(4, None, None, None, None, C.byref(h)) == E_INVALID and not h.value
    assert b"amg_setup: null" in lib.storm_hip_last_error()
    rp = (C.c_int64 * 2)(0, 1)
    assert lib.storm_hip_amg_setup_csr_structural(1, rp, None, None, None, C.byref(h)) == E_INVALID and not h.value
    assert lib.storm_hip_amg_setup_csr_structural(1, rp, None, None, None, None) == E_INVALID
    assert lib.storm_hip_amg_hierarchy_get_strong(None, 0, None) == E_INVALID
    assert b"amg_hierarchy_get_strong: null" in lib.storm_hip_last_error()
    d = C.c_double(-5.0)
    assert lib.storm_hip_amg_hierarchy_get(None, b"structural", C.byref(d)) == E_INVALID and d.value == -5.0
    # the device entry points, before a device is touched
    assert lib.storm_hip_amg_create_refreshable(None, 1.0, 0.0, None, C.byref(h)) == E_INVALID and not h.value
    assert b"amg_create_refreshable: null" in lib.storm_hip_last_error()
    assert lib.storm_hip_amg_create_refreshable(None, 1.0, 0.0, None, None) == E_INVALID
    assert lib.storm_hip_amg_refresh(None) == E_INVALID
    assert b"amg_refresh: null" in lib.storm_hip_last_error()
    assert lib.storm_hip_amg_download(None) == E_INVALID
    assert b"amg_download: null" in lib.storm_hip_last_error()
    # the same refusals as the plain setup: a singular coarsest level, parameters out of range, malformed CSR
    from stormruler_amd import api

    def status(a, **params):
        a = sp.csr_matrix(a)
        r, c, v = a.indptr.astype(np.int64), a.indices.astype(np.int64), a.data.astype(np.float64)
        p = api._amg_params(**params)
        out = C.c_void_p()
        st = lib.storm_hip_amg_setup_csr_structural(a.shape[0], r.ctypes.data_as(_lib.i64p), c.ctypes.data_as(_lib.i64p),
                                                    v.ctypes.data_as(_lib.f64p), C.byref(p), C.byref(out))
        msg = lib.storm_hip_last_error().decode()
        if st == 0:
            lib.storm_hip_amg_hierarchy_destroy(out)
        return st, msg

    st, msg = status(np.array([[1.0, -1.0], [-1.0, 1.0]]))
    assert st == E_INVALID and "singular" in msg
    st, msg = status(sp.identity(2000).tocsr())
    assert st == E_UNSUPPORTED and "stagnates" in msg
    st, msg = status(np.array([[0.0, 1.0], [1.0, 0.0]]), coarse_rows=1)
    assert st == E_INVALID and "zero diagonal" in msg
    st, msg = status(amg_cases.poisson_box(4), smoother_degree=0)
    assert st == E_INVALID and "smoother_degree" in msg
    # the strong mask is not available on the coarsest level
    hs = api.AmgHierarchy.from_csr(sp.identity(3).tocsr(), structural=True)
    mask = np.zeros(3, np.uint8)
    assert lib.storm_hip_amg_hierarchy_get_strong(hs._h, 0, mask.ctypes.data_as(C.POINTER(C.c_uint8))) == E_INVALID
    assert b"no strong mask" in lib.storm_hip_last_error()
    assert hs.get("structural") == 1.0


def test_binding_classes_have_the_refresh_knobs():
    from stormruler_amd import api

    assert api.AmgPreconditioner().refreshable is False and api.AmgPreconditioner(refreshable=True).refreshable is True
    for name in ("refresh", "download"):
        assert hasattr(api.AmgPreconditioner, name)
    assert hasattr(api.AmgHierarchy, "strong")
