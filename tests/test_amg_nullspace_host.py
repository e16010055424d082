"""The host setup for singular operators with the constants as their kernel (storm_hip_amg_setup_csr_nullspace,
csrc/amg_setup.hip) against the restatement (tests/amg_nullspace_ref.py on top of tests/amg_ref.py), without a device.

  * every level against the restatement by the comparison of tests/test_amg_host.py (aggregates exactly; P_l and A_{l+1}
    within the reordered-sum bound, each level fed the LIBRARY'S exported operator);
  * the coarsest level's Ainv against N3 restated: |A_c Ainv A_c - A_c| within 10 x the same figure of numpy's pinv (the
    reference; both are printed), column and row sums of Ainv below 64 eps max|Ainv|, and Ainv entrywise beside the
    restatement's;
  * the structural variant equals the plain one where the plain setup drops no zero;
  * refusals N1 (a Dirichlet box; the message names the row), N2 (two boxes side by side: "component", 2), parameters;
  * a one-row coarsest level: Ainv = (0), coarse_shift = 0;
  * storm_hip_amg_setup_csr on the same operators still answers E_INVALID with "singular".

Measured with the build this file arrived with (|A Ainv A - A|: library / pinv):
  box 12x10x9, coarse_rows 16 (1080 / 140 / 10)  6.8e-13 / 2.7e-12;  coarse_rows 512 (1080 / 140)  1.6e-12 / 1.1e-12
  lognormal (1080 / 193 / 15)  8.9e-15 / 2.1e-14;  renumbered (1080 / 166 / 12)  7.1e-15 / 4.5e-14
  relative row sums at level 0 at most 1.8e-16; column and row sums of Ainv at most 0.11 of their bound.

test_the_plain_setup_still_refuses: step 7 of the plain recipe refuses a coarsest level that is singular to working
precision (a pivot below 2^-40 of the largest diagonal entry).  Rounding leaves the last pivot of these four singular
coarsest matrices at 1.6e-15, 6.6e-15, 3.2e-15 and 9.2e-16 of that scale, not at zero; the smallest pivot of the definite
operators of tests/test_amg_host.py is 0.066 of it."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import amg_cases  # noqa: E402
import amg_nullspace_ref as nr  # noqa: E402
import amg_ref  # noqa: E402
import test_amg_host as base  # noqa: E402  (the comparison: _within, _prolongator_bound, _ones)

EPS = np.finfo(np.float64).eps
E_INVALID = -1


@pytest.fixture(scope="module")
def api():
    from stormruler_amd import api

    return api


def _case(name):
    from stormruler_amd import mesh

    if name in ("box16", "box512"):
        return nr.neumann_box(mesh, 12, 10, 9)[1], dict(coarse_rows=int(name[3:]))
    a = nr.lognormal_box(mesh)[2]
    if name == "lognormal":
        return a, dict(coarse_rows=16)
    assert name == "renumbered"
    return nr.renumbered(a), dict(coarse_rows=16)


CASES = ["box16", "box512", "lognormal", "renumbered"]
_cache = {}


def _hierarchy(api, name):
    if name not in _cache:
        a, params = _case(name)
        _cache[name] = (a, params, api.AmgHierarchy.from_csr(a, nullspace="constant", **params))
    return _cache[name]


@pytest.mark.parametrize("name", CASES)
def test_every_level_against_the_restatement(api, name):
    a, params, h = _hierarchy(api, name)
    q = dict(amg_ref.DEFAULTS, **params)
    assert h.get("nullspace") == 1 and h.get("structural") == 0 and h.levels >= 2
    assert nr.first_bad_row(a) is None and nr.components(a) == 1
    rel = np.abs(np.asarray(a.sum(axis=1)).ravel()) / np.asarray(abs(a).sum(axis=1)).ravel()
    print(f"{name}: levels {h.level_rows()}, largest relative row sum {rel.max():.2e} (threshold {nr.ROW_SUM_THRESHOLD:.2e})")
    assert abs(h.operator(0) - amg_ref.normalise(a)).max() == 0.0
    for lv in range(h.levels - 1):
        al = h.operator(lv)
        s = amg_ref.strength(al, q["strength_theta"])
        agg, count = amg_ref.aggregate(s)
        assert np.array_equal(h.aggregates(lv), agg), f"level {lv}: aggregates differ"
        assert h.sizes(lv)[2] == count == h.sizes(lv + 1)[0]
        p_lib, p_ref = h.prolongator(lv), amg_ref.prolongator(al, s, agg, count, q["prolongator_omega"])
        base._within(p_lib, p_ref, *base._prolongator_bound(al, s, agg, count, q["prolongator_omega"]), f"{name} P_{lv}")
        c_ref = amg_ref.coarse_operator(al, p_lib)
        c_terms = (base._ones(p_lib).T @ base._ones(al) @ base._ones(p_lib)).tocsr()
        c_mag = (abs(p_lib).T @ abs(al) @ abs(p_lib)).tocsr()
        base._within(h.operator(lv + 1), c_ref, c_terms, c_mag, f"{name} A_{lv + 1}")
    # the restatement run on its own coarse operators reaches the same level sizes
    levels, _, _ = nr.hierarchy(a, **params)
    assert [lv["A"].shape[0] for lv in levels] == h.level_rows()


@pytest.mark.parametrize("name", CASES)
def test_coarse_pseudo_inverse(api, name):
    a, params, h = _hierarchy(api, name)
    ac = h.operator(h.levels - 1).toarray()
    m = ac.shape[0]
    assert 1 < m <= params["coarse_rows"]
    ainv = h.coarse_inverse()
    ref, s = nr.coarse_inverse(ac)
    assert h.get("coarse_shift") == s == ac.diagonal().max() > 0
    pinv = np.linalg.pinv(ac)
    res, res_pinv = np.abs(ac @ ainv @ ac - ac).max(), np.abs(ac @ pinv @ ac - ac).max()
    sums = max(np.abs(ainv.sum(axis=0)).max(), np.abs(ainv.sum(axis=1)).max())
    print(f"{name} ({m} rows): |A Ainv A - A| = {res:.3e} (pinv {res_pinv:.3e}); sums of Ainv {sums:.3e} "
          f"(64 eps max|Ainv| = {64 * EPS * np.abs(ainv).max():.3e}); |Ainv - pinv| = {np.abs(ainv - pinv).max():.3e}")
    assert res <= 10.0 * res_pinv
    assert sums <= 64 * EPS * np.abs(ainv).max()
    # beside the restatement of N3 (numpy's LU in place of the Gauss-Jordan): two inverses of G = A_c + (s / m) 1 1^T, each
    # with an entrywise residual of at most 64 m eps cond(G) (tests/test_amg_host.py), differ by at most that times
    # m |G^-1|; the projections are contractions
    g = ac + s / m
    bound = 2 * 64 * m * EPS * np.linalg.cond(g) * m * np.abs(np.linalg.inv(g)).max()
    assert np.abs(ainv - ref).max() <= bound
    # the smallest pivot the Gauss-Jordan can meet is far above the refusal threshold
    assert np.linalg.eigvalsh(g).min() > 2.0 ** -20 * s


@pytest.mark.parametrize("name", CASES)
def test_structural_and_plain_agree_where_no_zero_is_dropped(api, name):
    a, params, h = _hierarchy(api, name)
    hs = api.AmgHierarchy.from_csr(a, structural=True, nullspace="constant", **params)
    assert hs.get("structural") == 1 and hs.get("nullspace") == 1 and hs.level_rows() == h.level_rows()
    # none of these operators has a stored zero, and no entry of a P_l or an A_{l+1} cancels exactly: the plain setup drops
    # nothing, so the two hierarchies are equal bit for bit
    for lv in range(h.levels):
        assert hs.sizes(lv) == h.sizes(lv)
        assert abs(hs.operator(lv) - h.operator(lv)).max() == 0.0
        if lv + 1 < h.levels:
            assert abs(hs.prolongator(lv) - h.prolongator(lv)).max() == 0.0 and np.array_equal(hs.strong(lv), h.strong(lv))
    assert np.array_equal(hs.coarse_inverse(), h.coarse_inverse()) and hs.get("coarse_shift") == h.get("coarse_shift")


def _status(a, plain=False, structural=0, **params):
    from stormruler_amd import _lib, api

    a = sp.csr_matrix(a)
    rp, col, val = a.indptr.astype(np.int64), a.indices.astype(np.int64), a.data.astype(np.float64)
    h = C.c_void_p()
    p = api._amg_params(**params)
    args = (a.shape[0], rp.ctypes.data_as(_lib.i64p), col.ctypes.data_as(_lib.i64p), val.ctypes.data_as(_lib.f64p), C.byref(p))
    if plain:
        st = _lib.lib.storm_hip_amg_setup_csr(*args, C.byref(h))
    else:
        st = _lib.lib.storm_hip_amg_setup_csr_nullspace(*args, structural, C.byref(h))
    msg = _lib.lib.storm_hip_last_error().decode()
    if st == 0:
        _lib.lib.storm_hip_amg_hierarchy_destroy(h)
    else:
        assert not h.value
    return st, msg


def test_refusals():
    from stormruler_amd import mesh

    # N1: Dirichlet walls -- the first wall cell is row 0
    g = mesh.structured_box(6)
    dirichlet = mesh.assemble_csr(g, -1.0, 0.0).tocsr()[:, :g.n_cells]
    row = nr.first_bad_row(dirichlet)
    assert row == 0
    for structural in (0, 1):
        st, msg = _status(dirichlet, structural=structural)
        assert st == E_INVALID and f"row {row} " in msg and "constants" in msg and "storm_hip_amg_setup_csr" in msg
    # ... and a Neumann box with beta != 0; a single Dirichlet face in the middle of the numbering
    _, neumann = nr.neumann_box(mesh, 5, 4, 3)
    st, msg = _status(neumann + 0.5 * sp.identity(60))
    assert st == E_INVALID and "row 0 " in msg
    one_face = neumann.tolil()
    one_face[37, 37] += 2.0
    assert nr.first_bad_row(one_face.tocsr()) == 37
    st, msg = _status(one_face.tocsr())
    assert st == E_INVALID and "row 37 " in msg
    # N2: two boxes side by side
    two = sp.block_diag([nr.neumann_box(mesh, 4, 4, 4)[1], neumann]).tocsr()
    assert nr.first_bad_row(two) is None and nr.components(two) == 2
    for structural in (0, 1):
        st, msg = _status(two, structural=structural, coarse_rows=16)
        assert st == E_INVALID and "component" in msg and "2 " in msg
    # ... a row without an off-diagonal entry is a component of its own (its row sum is zero: N1 passes)
    st, msg = _status(sp.block_diag([neumann, sp.csr_matrix((1, 1))]).tocsr())
    assert st == E_INVALID and "component" in msg and "2 " in msg
    # ... and an entry stored as zero joins nothing
    chain = sp.diags([-np.ones(5), np.r_[1.0, 2.0 * np.ones(4), 1.0], -np.ones(5)], [-1, 0, 1]).tolil()
    chain[2, 3] = chain[3, 2] = 0.0
    chain[2, 2] = chain[3, 3] = 1.0
    cut = chain.tocsr()
    assert nr.components(cut) == 2
    st, msg = _status(cut, structural=1)
    assert st == E_INVALID and "component" in msg
    # parameters
    st, msg = _status(neumann, smoother_degree=17)
    assert st == E_INVALID and "smoother_degree" in msg
    # the connected Neumann operators themselves are accepted
    assert _status(neumann)[0] == 0 and _status(neumann, structural=1, coarse_rows=16)[0] == 0


def test_one_row_coarsest_level(api):
    a = nr.graph_laplacian(4)
    levels, ainv, s = nr.hierarchy(a, coarse_rows=16)
    assert levels[-1]["A"].shape[0] == 1 and ainv.shape == (1, 1) and ainv[0, 0] == 0.0 and s == 0.0
    h = api.AmgHierarchy.from_csr(a, nullspace="constant", coarse_rows=16)
    assert h.level_rows() == [lv["A"].shape[0] for lv in levels] and h.level_rows()[-1] == 1
    assert np.array_equal(h.coarse_inverse(), np.zeros((1, 1))) and h.get("coarse_shift") == 0.0
    print(f"graph Laplacian (seed 4): levels {h.level_rows()}, the coarsest entry {h.operator(h.levels - 1)[0, 0]:.3e}")


@pytest.mark.parametrize("name", CASES)
def test_the_plain_setup_still_refuses(api, name):
    a, params, h = _hierarchy(api, name)
    st, msg = _status(a, plain=True, **params)
    print(f"{name}: storm_hip_amg_setup_csr -> {st} ({msg})")
    assert st == E_INVALID and "singular" in msg and "nullspace" in msg
    plain = api.AmgHierarchy.from_csr(amg_cases.poisson_box(5))
    assert plain.get("nullspace") == 0 and plain.get("coarse_shift") == 0.0
