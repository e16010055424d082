"""Refreshable multigrid objects on the device (storm_hip_amg_create_refreshable, _refresh, _download; csrc/amg_refresh.hip):
after StencilMatrix.set_face_weights a refresh recomputes every number of the hierarchy on the frozen structure.

1. a refresh at the setup's own weights reproduces the setup's export (patterns identical, values within the
   reordered-sum bound);
2. new weights against the restatement of the frozen-structure recipe (tests/amg_refresh_ref.py), level by level, also
   with CSR tails (ell_cap = 4);
3. exact whatever the order of summation: doubled weights, and integer weights with the unsmoothed prolongator;
4. determinism and no leakage from one state to the next;
5. the cycle reads what was refreshed (against amg_ref.Cycle on the downloaded hierarchy; reduced records; unfused options);
6. solves: iteration counts against the restatement's PCG, a fresh build and the stale object;
7. refusals;  8. the C++ driver.

Operators: amg_cases.face_weight_case through StencilMatrix.from_face_weights_updatable on fp64 records, alpha = -1,
beta = 0 (one case alpha = -1, beta = 0.5).  Bounds: 8 eps (terms) (sum of |products|) for reordered sums
(tests/test_amg_host.py); the cycle's margin is 10 x the difference between the restatement in float64 and in long double
(tests/test_gpu_amg.py)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import amg_cases  # noqa: E402
import amg_ref  # noqa: E402
import amg_refresh_ref as rr  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_UNSUPPORTED = -1, -6
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def env():
    from oracle import oracle
    from stormruler_amd import api, mesh

    ctx = api.Context(0)
    yield api, mesh, oracle, ctx
    ctx.close()


def _assemble(g, w, diag_extra, alpha=-1.0, beta=0.0):
    """A = beta I + alpha M of the face weights w (both sides) and the diagonal term diag_extra."""
    nc = g.n_cells
    rows = np.concatenate([g.inner, g.outer, g.inner, g.outer, np.arange(nc)])
    cols = np.concatenate([g.outer, g.inner, g.inner, g.outer, np.arange(nc)])
    vals = np.concatenate([alpha * w, alpha * w, -alpha * w, -alpha * w, beta + alpha * diag_extra])
    a = sp.coo_matrix((vals, (rows, cols)), shape=(nc, nc)).tocsr()
    a.sum_duplicates()
    return a


def _case(mesh, name):
    """(graph, weights, diag_extra, multigrid parameters)."""
    if name == "box13":
        g = mesh.structured_box(13)
        de = np.zeros(g.n_cells)
        np.add.at(de, g.b_cell, -2.0)
        return g, np.ones(g.inner.size), de, dict(coarse_rows=32)
    g, w, de, _ = amg_cases.face_weight_case(mesh, 16, name)
    return g, w, de, {}


def _seed12(g):
    return np.exp(np.random.default_rng(12).standard_normal(g.inner.size))


def _matrix(env, g, w, de, ell_cap=0):
    api, mesh, oracle, ctx = env
    ctx.set_option("ell_cap", ell_cap)
    try:
        return api.StencilMatrix.from_face_weights_updatable(ctx, g.n_cells, 0, g.inner, g.outer, w, w, de)
    finally:
        ctx.set_option("ell_cap", 0)


def _set(env, mat, w, de):
    api, mesh, oracle, ctx = env
    mat.set_face_weights(api.DeviceVector.from_numpy(ctx, w), api.DeviceVector.from_numpy(ctx, w), api.DeviceVector.from_numpy(ctx, de))


def _build(env, mat, alpha=-1.0, beta=0.0, ell_cap=0, refreshable=True, **params):
    api, mesh, oracle, ctx = env
    pre = api.AmgPreconditioner(refreshable=refreshable, **params)
    x = api.DeviceVector(ctx, mat.stats()["n_rows"])
    ctx.set_option("ell_cap", ell_cap)  # (the coarse operators go through the packer under the context's cap)
    try:
        pre.build(x, x, api.HipStencilOperator(mat, alpha, beta))
    finally:
        ctx.set_option("ell_cap", 0)
    return pre


def _export(pre):
    h = pre.hierarchy
    return dict(ops=[h.operator(lv) for lv in range(h.levels)], ps=[h.prolongator(lv) for lv in range(h.levels - 1)],
                aggs=[h.aggregates(lv) for lv in range(h.levels - 1)], masks=[h.strong(lv) for lv in range(h.levels - 1)],
                inv=h.coarse_inverse())


def _same_bits(x, y):
    return all(rr.same_pattern(p, q) and np.array_equal(p.data, q.data) for p, q in zip(x["ops"] + x["ps"], y["ops"] + y["ps"])) and \
        np.array_equal(x["inv"], y["inv"])


def _level0_slack(a):
    return (np.diff(a.indptr).max() + 2) * EPS * np.asarray(abs(a).sum(axis=1)).ravel().max()


def _inverse_holds(ops, inv):
    ac = ops[-1].toarray()
    m = ac.shape[0]
    res = np.abs(inv @ ac - np.eye(m)).max()
    bound = 64 * m * EPS * np.linalg.cond(ac)
    print(f"coarsest level ({m} rows): |inv A - I| = {res:.3e}, bound {bound:.3e}")
    assert res <= bound


def _apply(env, pre, r_host):
    api, mesh, oracle, ctx = env
    r, z = api.DeviceVector.from_numpy(ctx, r_host), api.DeviceVector(ctx, r_host.size)
    z.upload(np.full(r_host.size, np.nan))
    pre.mul(z, r)
    return z.to_numpy()


# ---- 1. a refresh at the setup's own weights --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lognormal", "aniso", "box13"])
def test_refresh_at_the_setups_own_weights(env, name):
    api, mesh, oracle, ctx = env
    g, w, de, params = _case(mesh, name)
    mat = _matrix(env, g, w, de)
    pre = _build(env, mat, **params)
    assert pre.get("refreshable") == 1 and pre.get("structural") == 1
    assert 0 < pre.get("refresh_bytes") < pre.get("device_bytes")
    before = _export(pre)
    omega = amg_ref.DEFAULTS["prolongator_omega"]
    moved = ctx.counter("amg_refreshes")
    pre.refresh()
    assert ctx.counter("amg_refreshes") == moved + 1
    pre.download()
    after = _export(pre)
    assert len(after["ops"]) == len(before["ops"]) >= 3
    for x, y in zip(after["ops"] + after["ps"], before["ops"] + before["ps"]):
        assert rr.same_pattern(x, y)
    for x, y in zip(after["aggs"] + after["masks"], before["aggs"] + before["masks"]):
        assert np.array_equal(x, y)
    a0 = before["ops"][0]
    d0 = abs(after["ops"][0] - a0).max()
    print(f"{name}: level 0 differs by {d0:.3e} (slack {_level0_slack(a0):.3e})")
    assert d0 <= _level0_slack(a0)
    for lv in range(len(before["ps"])):
        al, p0 = before["ops"][lv], before["ps"][lv]
        rr.within(after["ps"][lv], p0, *rr.prolongator_bound(al, before["masks"][lv], before["aggs"][lv], p0.shape[1], omega), f"{name} P_{lv}")
        rr.within(after["ops"][lv + 1], before["ops"][lv + 1], *rr.coarse_bound(al, p0), f"{name} A_{lv + 1}")
        print(f"{name}: P_{lv} differs by {abs(after['ps'][lv] - p0).max():.3e}, A_{lv + 1} by "
              f"{abs(after['ops'][lv + 1] - before['ops'][lv + 1]).max():.3e}")
    _inverse_holds(after["ops"], after["inv"])
    # X1 - X0 = (I - X0 A1) X1 + X0 (A1 X1 - I) and I - X0 A1 = (I - X0 A0) + X0 (A0 - A1): both inverses leave a residual of at
    # most r = 64 m eps cond in every entry (m r in the infinity norm), and the two exports of the coarsest level differ by
    # at most the reordered-sum bound B
    ac = after["ops"][-1].toarray()
    m = ac.shape[0]
    r = 64 * m * EPS * np.linalg.cond(ac)
    inf = lambda x: float(np.abs(x).sum(axis=1).max())  # noqa: E731
    terms, magnitude = rr.coarse_bound(before["ops"][-2], before["ps"][-1])
    b_inf = inf(((8.0 * EPS) * terms.multiply(magnitude)).toarray())
    x0, x1 = inf(before["inv"]), inf(after["inv"])
    gap = float(np.abs(after["inv"] - before["inv"]).max())
    bound = m * r * (x0 + x1) + x0 * b_inf * x1
    print(f"{name}: the inverses differ by {gap:.3e} (bound {bound:.3e})")
    assert gap <= bound
    pre.close()
    mat.close()


# ---- 2. new weights against the frozen restatement --------------------------------------------------------------------------
def _check_against_frozen(name, got, a_new, omega):
    a0 = got["ops"][0]
    d0 = abs(a0 - a_new).max()
    print(f"{name}: level 0 against the assembled matrix {d0:.3e} (slack {_level0_slack(a_new):.3e})")
    assert d0 <= _level0_slack(a_new)
    for lv in range(len(got["ps"])):
        al, mask, agg = got["ops"][lv], got["masks"][lv], got["aggs"][lv]
        count = got["ps"][lv].shape[1]
        p_ref, c_ref = rr.frozen_level(al, mask, agg, count, omega)
        p_lib, c_lib = got["ps"][lv], got["ops"][lv + 1]
        assert rr.same_pattern(p_lib, p_ref) and rr.same_pattern(c_lib, c_ref)
        rr.within(p_lib, p_ref, *rr.prolongator_bound(al, mask, agg, count, omega), f"{name} P_{lv}")
        # the coarse operator of the library's own P (held to the restatement's above)
        rr.within(c_lib, rr.on_pattern(p_lib.T @ al @ p_lib, rr.ones(c_ref)), *rr.coarse_bound(al, p_lib), f"{name} A_{lv + 1}")
    _inverse_holds(got["ops"], got["inv"])


@pytest.mark.parametrize("name", ["lognormal_to_seed12", "aniso_to_lognormal", "lognormal_to_seed12_tails", "lognormal_beta"])
def test_new_weights_against_the_frozen_restatement(env, name):
    api, mesh, oracle, ctx = env
    tails = name.endswith("tails")
    beta = 0.5 if name == "lognormal_beta" else 0.0
    g, w, de, params = _case(mesh, "aniso" if name.startswith("aniso") else "lognormal")
    if name.startswith("aniso"):
        _, w_new, de_new, _ = _case(mesh, "lognormal")
    else:
        w_new, de_new = _seed12(g), de
    cap = 4 if tails else 0
    mat = _matrix(env, g, w, de, ell_cap=cap)
    if tails:
        assert mat.stats()["tail_rows"] > 0
    pre = _build(env, mat, beta=beta, ell_cap=cap, **params)
    levels = pre.hierarchy.level_rows()
    frozen = _export(pre)
    _set(env, mat, w_new, de_new)
    pre.refresh()
    pre.download()
    got = _export(pre)
    assert pre.hierarchy.level_rows() == levels and len(levels) >= 3
    for x, y in zip(got["aggs"] + got["masks"], frozen["aggs"] + frozen["masks"]):
        assert np.array_equal(x, y)  # frozen
    for x, y in zip(got["ops"] + got["ps"], frozen["ops"] + frozen["ps"]):
        assert rr.same_pattern(x, y)
    assert abs(got["ops"][1] - frozen["ops"][1]).max() > 0  # ... and the numbers did move
    _check_against_frozen(name, got, _assemble(g, w_new, de_new, -1.0, beta), amg_ref.DEFAULTS["prolongator_omega"])
    pre.close()
    mat.close()


# ---- 3. exact, whatever the summation order ---------------------------------------------------------------------------------
def test_doubled_weights_double_every_operator_exactly(env):
    api, mesh, oracle, ctx = env
    g, w, de, params = _case(mesh, "lognormal")
    mat = _matrix(env, g, w, de)
    pre = _build(env, mat, **params)
    pre.refresh()
    pre.download()
    one = _export(pre)
    _set(env, mat, 2.0 * w, 2.0 * de)
    pre.refresh()
    pre.download()
    two = _export(pre)
    for lv, (p, q) in enumerate(zip(two["ps"], one["ps"])):
        assert np.array_equal(p.data, q.data), f"P_{lv} changed"
    for lv, (x, y) in enumerate(zip(two["ops"], one["ops"])):
        assert np.array_equal(x.data, 2.0 * y.data), f"A_{lv} is not doubled"
    assert np.array_equal(two["inv"], 0.5 * one["inv"])
    pre.close()
    mat.close()


def test_integer_weights_with_the_unsmoothed_prolongator_are_exact(env):
    api, mesh, oracle, ctx = env
    g, w, de, params = _case(mesh, "lognormal")
    mat = _matrix(env, g, w, de)
    pre = _build(env, mat, prolongator_omega=0.0, coarse_rows=32)
    w_int = np.random.default_rng(5).integers(1, 5, g.inner.size).astype(np.float64)
    _set(env, mat, w_int, de)  # (diag_extra is -2 per wall face: integers)
    pre.refresh()
    pre.download()
    got = _export(pre)
    assert len(got["ops"]) >= 3
    assert np.array_equal(got["ops"][0].toarray(), _assemble(g, w_int, de).toarray())
    for lv, (al, agg) in enumerate(zip(got["ops"], got["aggs"])):
        n, count = al.shape[0], got["ops"][lv + 1].shape[0]
        t = sp.csr_matrix((np.ones(n), (np.arange(n), agg)), shape=(n, count))
        assert (got["ps"][lv] != t).nnz == 0
        assert np.array_equal(got["ops"][lv + 1].toarray(), (t.T @ al @ t).toarray()), f"A_{lv + 1}"
    pre.close()
    mat.close()


# ---- 4. determinism and no leakage ------------------------------------------------------------------------------------------
def test_refresh_is_deterministic_and_keeps_nothing_of_the_state_before(env):
    api, mesh, oracle, ctx = env
    g, w0, de, params = _case(mesh, "lognormal")
    w1 = _seed12(g)
    mat = _matrix(env, g, w0, de)
    pre = _build(env, mat, **params)
    r_host = np.random.default_rng(4).standard_normal(g.n_cells)

    def state():
        pre.refresh()
        pre.download()
        return _export(pre), _apply(env, pre, r_host)

    h_a, z_a = state()
    h_b, z_b = state()
    assert _same_bits(h_a, h_b) and np.array_equal(z_a, z_b)
    _set(env, mat, w1, de)
    h_1, z_1 = state()
    assert not np.array_equal(z_1, z_a)
    _set(env, mat, w0, de)
    h_c, z_c = state()
    assert _same_bits(h_a, h_c) and np.array_equal(z_a, z_c)
    pre.close()
    mat.close()


# ---- 5. the cycle reads what was refreshed ------------------------------------------------------------------------------------
def _restatement(pre, dtype=np.float64):
    h = pre.hierarchy
    ops = [h.operator(lv) for lv in range(h.levels)]
    ps = [h.prolongator(lv) for lv in range(h.levels - 1)]
    return amg_ref.Cycle(ops, ps, h.coarse_inverse(), degree=int(pre.get("smoother_degree")), dtype=dtype)


@pytest.mark.parametrize("degree", [1, 2])
def test_cycle_against_the_restatement_on_the_downloaded_hierarchy(env, degree):
    api, mesh, oracle, ctx = env
    g, w, de, params = _case(mesh, "lognormal")
    mat = _matrix(env, g, w, de)
    pre = _build(env, mat, smoother_degree=degree, **params)
    _set(env, mat, _seed12(g), de)
    pre.refresh()
    pre.download()
    r_host = np.random.default_rng(4).standard_normal(g.n_cells)
    z_dev = _apply(env, pre, r_host)
    z64, zld = _restatement(pre)(r_host), _restatement(pre, np.longdouble)(r_host)
    margin = 10.0 * float(np.abs(z64 - zld.astype(np.float64)).max())
    diff = float(np.abs(z_dev - z64).max())
    print(f"degree {degree}: |device - restatement| = {diff:.3e}, margin {margin:.3e}, |z| = {np.abs(z64).max():.3e}")
    assert margin > 0 and diff <= margin
    # the unfused paths read the same refreshed objects: the same bits
    try:
        ctx.set_option("amg_fused", 0)
        ctx.set_option("cheb_fused", 0)
        assert np.array_equal(_apply(env, pre, r_host), z_dev)
    finally:
        ctx.set_option("amg_fused", 1)
        ctx.set_option("cheb_fused", 1)
    pre.close()
    mat.close()


def _solve(api, ctx, solver, mat, alpha, beta, b_host, pre_op, side="right"):
    b, x = api.DeviceVector.from_numpy(ctx, b_host), api.DeviceVector(ctx, b_host.size)
    solver.pre_op = pre_op
    solver.pre_side = api.PreconditionerSide.Left if side == "left" else api.PreconditionerSide.Right
    ok = solver.solve(x, b, api.HipStencilOperator(mat, alpha, beta))
    return ok, solver.iteration, x.to_numpy()


def test_reduced_records_smoothers_after_a_refresh(env):
    api, mesh, oracle, ctx = env
    g, w, de, params = _case(mesh, "lognormal")
    w1 = _seed12(g)
    a1 = _assemble(g, w1, de)
    b_host = np.random.default_rng(8).standard_normal(g.n_cells)
    counts = {}
    for reduced in (False, True):
        mat = _matrix(env, g, w, de)
        pre = _build(env, mat, reduced_records=reduced, **params)
        _set(env, mat, w1, de)
        pre.refresh()
        before = ctx.counter("cheb_reduced_applies")
        ok, it, x = _solve(api, ctx, api.CgSolver(), mat, -1.0, 0.0, b_host, pre)
        moved = ctx.counter("cheb_reduced_applies") - before
        assert ok and np.linalg.norm(b_host - a1 @ x) <= 1e-5 * np.linalg.norm(b_host)
        if reduced:
            assert pre.get("reduced") == 1 and moved >= 2 * (int(pre.get("levels")) - 1) * it > 0 and mat.reduced_bytes > 0
        else:
            assert moved == 0
        counts[reduced] = it
        pre.close()
        mat.close()
    print(f"fp64 smoothers {counts[False]} iterations, fp32-weight smoothers {counts[True]}")
    assert abs(counts[True] - counts[False]) <= 1


# ---- 6. solves ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def refreshed_counts():
    return {}


@pytest.mark.parametrize("degree", [1, 2])
def test_cg_counts_refreshed_fresh_and_stale(env, refreshed_counts, degree):
    api, mesh, oracle, ctx = env
    g, w0, de, params = _case(mesh, "lognormal")
    w1 = _seed12(g)
    a1 = _assemble(g, w1, de)
    n = g.n_cells
    b_host = np.random.default_rng(8).standard_normal(n)
    mat = _matrix(env, g, w0, de)
    pre = _build(env, mat, smoother_degree=degree, **params)
    _set(env, mat, w1, de)
    ok_stale, it_stale, _ = _solve(api, ctx, api.CgSolver(), mat, -1.0, 0.0, b_host, pre)
    handle, moved = pre._h.value, ctx.counter("amg_refreshes")
    pre.refresh()
    assert ctx.counter("amg_refreshes") == moved + 1
    ok, it, x = _solve(api, ctx, api.CgSolver(), mat, -1.0, 0.0, b_host, pre)
    assert pre._h.value == handle  # the same object: build() kept it
    pre.download()
    cycle = _restatement(pre)
    ref = oracle.solve("cg", oracle.CsrOperator(a1), b_host, pre=oracle.CallbackOperator(n, cycle), side="right")
    fresh_mat = _matrix(env, g, w1, de)
    fresh = api.AmgPreconditioner(smoother_degree=degree, **params)
    ok_fresh, it_fresh, _ = _solve(api, ctx, api.CgSolver(), fresh_mat, -1.0, 0.0, b_host, fresh)
    print(f"degree {degree}: refreshed {it} iterations (restatement's PCG {ref.iterations}), fresh {it_fresh}, stale {it_stale} "
          f"(converged: {ok_stale})")
    assert ok and ok_fresh and ref.converged
    assert abs(it - ref.iterations) <= 1
    assert it <= it_fresh + 2
    assert 2 * it <= it_stale
    assert np.linalg.norm(b_host - a1 @ x) <= 1e-5 * np.linalg.norm(b_host)
    refreshed_counts[degree] = it
    for o in (pre, fresh, mat, fresh_mat):
        o.close()


@pytest.mark.parametrize("side", ["left", "right"])
@pytest.mark.parametrize("kind", ["bicgstab", "fgmres"])
def test_other_methods_converge_with_the_refreshed_object(env, kind, side):
    api, mesh, oracle, ctx = env
    g, w0, de, params = _case(mesh, "lognormal")
    w1 = _seed12(g)
    a1 = _assemble(g, w1, de)
    b_host = np.random.default_rng(8).standard_normal(g.n_cells)
    mat = _matrix(env, g, w0, de)
    pre = _build(env, mat, **params)
    _set(env, mat, w1, de)
    pre.refresh()
    solver = api.BiCgStabSolver() if kind == "bicgstab" else api.FgmresSolver()
    ok, it, x = _solve(api, ctx, solver, mat, -1.0, 0.0, b_host, pre, side)
    print(f"{kind} {side}: {it} iterations")
    assert ok and 0 < it <= 20
    assert np.linalg.norm(b_host - a1 @ x) <= 1e-4 * np.linalg.norm(b_host)
    pre.close()
    mat.close()


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals(env, refreshed_counts):
    api, mesh, oracle, ctx = env
    from stormruler_amd import _lib
    from stormruler_amd._lib import lib

    def create(mat, alpha=-1.0, beta=0.0):
        h = C.c_void_p()
        st = lib.storm_hip_amg_create_refreshable(mat._h, alpha, beta, None, C.byref(h))
        msg = lib.storm_hip_last_error().decode()
        assert st != 0 and not h.value
        return st, msg

    g, w, de, params = _case(mesh, "lognormal")
    ctx.set_option("spmv_dict", 0)
    try:
        plain_mat = api.StencilMatrix.from_face_weights(ctx, g.n_cells, 0, g.inner, g.outer, w, w, de)
        csr_mat = api.StencilMatrix.from_csr(ctx, amg_cases.poisson_box(6))
    finally:
        ctx.set_option("spmv_dict", 4)
    compact = api.StencilMatrix.from_face_graph(ctx, mesh.structured_box(6))
    assert compact.stats()["value_dictionary_size"] > 0
    for m in (plain_mat, csr_mat, compact):
        st, msg = create(m)
        assert st == E_UNSUPPORTED and "updatable" in msg
    # refresh on a plain object
    plain = _build(env, plain_mat, refreshable=False, **params)
    assert lib.storm_hip_amg_refresh(plain._h) == E_UNSUPPORTED
    assert b"create_refreshable" in lib.storm_hip_last_error()
    with pytest.raises(_lib.StormHipError):
        plain.refresh()
    before = _export(plain)
    plain.download()  # allowed, and changes nothing
    assert _same_bits(before, _export(plain)) and plain.get("refreshable") == 0 and plain.get("refresh_bytes") == 0
    plain.close()
    # a row whose weights and diagonal term are all zero: its filtered diagonal is zero
    mat = _matrix(env, g, w, de)
    pre = _build(env, mat, **params)
    row = 17
    w_bad, de_bad = w.copy(), de.copy()
    w_bad[(g.inner == row) | (g.outer == row)] = 0.0
    de_bad[row] = 0.0
    _set(env, mat, w_bad, de_bad)
    moved = ctx.counter("amg_refreshes")
    assert lib.storm_hip_amg_refresh(pre._h) == E_INVALID
    msg = lib.storm_hip_last_error().decode()
    assert "level 0" in msg and f"row {row}" in msg and ctx.counter("amg_refreshes") == moved
    n = g.n_cells
    r, z = api.DeviceVector.from_numpy(ctx, np.ones(n)), api.DeviceVector(ctx, n)
    assert lib.storm_hip_amg_apply(pre._h, r._h, z._h) == E_INVALID and b"refresh" in lib.storm_hip_last_error()
    eng = api.Krylov(ctx, 0)
    eng.set_operator(api.HipStencilOperator(mat, -1.0, 0.0))
    assert lib.storm_hip_krylov_set_preconditioner_amg(eng._h, pre._h, 1) == 0
    x = api.DeviceVector(ctx, n)
    p, res = _lib.SolverParams(), _lib.SolverResult()
    lib.storm_hip_solver_params_default(C.byref(p))
    assert lib.storm_hip_krylov_solve(eng._h, r._h, x._h, C.byref(p), C.byref(res), None, None) == E_INVALID
    assert b"refresh" in lib.storm_hip_last_error()
    assert lib.storm_hip_krylov_set_preconditioner_amg(eng._h, None, 1) == 0
    # restored weights: the object solves again, with the count of the solves above
    w1 = _seed12(g)
    _set(env, mat, w1, de)
    pre.refresh()
    b_host = np.random.default_rng(8).standard_normal(n)
    ok, it, xs = _solve(api, ctx, api.CgSolver(), mat, -1.0, 0.0, b_host, pre)
    assert ok and np.linalg.norm(b_host - _assemble(g, w1, de) @ xs) <= 1e-5 * np.linalg.norm(b_host)
    if 2 in refreshed_counts:
        assert it == refreshed_counts[2]
    for o in (pre, mat, plain_mat, csr_mat, compact):
        o.close()


# ---- 8. the C++ driver -------------------------------------------------------------------------------------------------------
def test_cpp_driver(env):
    api, mesh, oracle, ctx = env
    exe = os.path.join(ROOT, "tests", "cpp", "amg_refresh_driver")
    if not os.path.exists(exe):  # (git-ignored: a checkout that arrived without it)
        import __graft_entry__ as ge

        ge.build()
    out = subprocess.run([exe, "16", "3"], check=True, capture_output=True, text=True, timeout=300).stdout
    got = json.loads(out.strip().splitlines()[-1])
    # the driver's weights: step s puts 1 + ((7 f + 3 s) mod 16) / 16 on face f (exact in binary), the walls keep weight 2
    g = mesh.structured_box(16)
    de = np.zeros(g.n_cells)
    np.add.at(de, g.b_cell, -2.0)
    f = np.arange(g.inner.size, dtype=np.float64)
    mat = _matrix(env, g, np.ones(g.inner.size), de)
    pre = _build(env, mat)
    its = []
    for s in range(1, 4):
        w = 1.0 + np.mod(7.0 * f + 3.0 * s, 16.0) / 16.0
        _set(env, mat, w, de)
        pre.refresh()
        ok, it, x = _solve(api, ctx, api.CgSolver(), mat, -1.0, 0.0, np.ones(g.n_cells), pre)
        assert ok
        its.append(it)
    print(got, "python:", its)
    assert got["converged"] == [1, 1, 1] and got["iterations"] == its
    assert got["amg_refreshes"] == 3 and got["level_rows"] == pre.hierarchy.level_rows()
    pre.close()
    mat.close()
