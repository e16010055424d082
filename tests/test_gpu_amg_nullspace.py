"""The multigrid preconditioner for singular operators with the constants as their kernel (storm_hip_amg_create_nullspace,
storm_hip_amg_project; csrc/amg.hip, csrc/amg_refresh.hip) on the device: B = Pi V Pi.

1. the projection is exact on integer-valued vectors, at every size where the streaming reduction changes shape;
2. the cycle against the restatement (tests/amg_nullspace_ref.py), B 1 = 0, symmetry, positivity on mean-free vectors;
3. the same bits with amg_fused / cheb_fused on and off, with fp64 and with reduced-record smoothers; the counters;
4. solves: CG counts against the restatement's PCG and below plain CG, the true residual, the mean of x; other methods;
5. refresh: against a fresh structural build, against the frozen restatement, CG counts; a cut box;
6. refusals and plumbing: the entry points, AmgPreconditioner(matrix=...), the cavity driver, the C++ driver.

_nb(nx, ny, nz) is the Neumann box: mesh.structured_box(..., dirichlet=False) built with spmv_dict = 0, applied with
alpha = -1, beta = 0.  Margins of 2 are those of tests/test_gpu_amg.py: 10 x the difference between the restatement in
float64 and in np.longdouble; the tests print what they measure.

What refuses the cut box of test_refresh_refuses_a_cut_box.  N1 and N2 are not repeated at a refresh, and N3's pivot test
does NOT see a cut: on the frozen structure the aggregates straddle it, the component indicators are not in the range of the
smoothed prolongators, and the coarsest matrix keeps a one-dimensional kernel (the frozen-structure restatement in numpy,
12 x 10 x 9 box with the structure of unit weights, lognormal weights with one plane of faces set to 0, each of the 28
planes in turn: the smallest eigenvalue of G = A_c + (s / n_c) 1 1^T stays between 0.21 s and 0.26 s with coarse_rows = 16
and between 0.023 s and 0.048 s with coarse_rows = 512, against the threshold of 2^-30 s).  The refusal the test sees is
step 3's: on the structure frozen from the lognormal weights a cell of the cut plane has its only strong links across the
cut, its filtered diagonal a_ii + (weak entries) = -(strong entries) becomes exactly 0, and the device-side check reports
the row (426 here).  A cut that leaves every row a strong link is not refused by a refresh; a build refuses it by N2.

First run on an MI355X: cycle |device - restatement| at most 0.17 of its margin, |B 1| = 0 exactly; symmetry at most 0.01 of
its margin; CG counts equal to the restatement's PCG on all ten solves (10 / 7, 11 / 8, 11 / 8, 11 / 8, 10 / 7 at degree
1 / 2 against 59, 92, 148, 146, 25 without a preconditioner); |mean(x)| at most 1.5e-17."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import amg_nullspace_ref as nr  # noqa: E402
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


def _matrix(api, ctx, build, *args):
    """A StencilMatrix on fp64 records (spmv_dict = 0), the option restored afterwards."""
    ctx.set_option("spmv_dict", 0)
    try:
        return build(ctx, *args)
    finally:
        ctx.set_option("spmv_dict", 4)


def _nb(env, nx, ny, nz):
    """(matrix, assembled A) of the Neumann box."""
    api, mesh, oracle, ctx = env
    g, a = nr.neumann_box(mesh, nx, ny, nz)
    return _matrix(api, ctx, api.StencilMatrix.from_face_graph, g), a


def _operator(env, name):
    """(matrix, alpha, assembled A) of a named case; beta = 0."""
    api, mesh, oracle, ctx = env
    if name in ("box", "box20"):
        mat, a = _nb(env, 12, 10, 9) if name == "box" else _nb(env, 20, 18, 16)
        return mat, -1.0, a
    g, w, a = nr.lognormal_box(mesh)
    if name == "lognormal":
        return _matrix(api, ctx, api.StencilMatrix.from_face_weights, g.n_cells, 0, g.inner, g.outer, w, w, None), -1.0, a
    if name == "renumbered":
        a = nr.renumbered(a)
    else:
        assert name == "graph"
        a = nr.graph_laplacian(3)
    return _matrix(api, ctx, api.StencilMatrix.from_csr, a), 1.0, a


CASES = ["box", "box20", "lognormal", "renumbered", "graph"]
PARAMS = dict(coarse_rows=16)


def _build(env, mat, alpha, **kw):
    api, mesh, oracle, ctx = env
    pre = api.AmgPreconditioner(nullspace="constant", **kw)
    x = api.DeviceVector(ctx, mat.stats()["n_rows"])
    pre.build(x, x, api.HipStencilOperator(mat, alpha, 0.0))
    assert pre.get("nullspace") == 1
    return pre


def _restatement(pre, dtype=np.float64):
    h = pre.hierarchy
    ops = [h.operator(lv) for lv in range(h.levels)]
    ps = [h.prolongator(lv) for lv in range(h.levels - 1)]
    return nr.Cycle(ops, ps, h.coarse_inverse(), degree=int(pre.get("smoother_degree")), dtype=dtype)


def _apply(env, pre, r_host):
    api, mesh, oracle, ctx = env
    r, z = api.DeviceVector.from_numpy(ctx, r_host), api.DeviceVector(ctx, r_host.size)
    z.upload(np.full(r_host.size, np.nan))  # (the cycle must not read z)
    pre.mul(z, r)
    assert np.array_equal(r.to_numpy(), r_host)  # r is not written
    return z.to_numpy()


# ---- 1. the projection, exact -------------------------------------------------------------------------------------------------
def _chain(n):
    return sp.diags([-np.ones(n - 1), np.r_[1.0, 2.0 * np.ones(n - 2), 1.0], -np.ones(n - 1)], [-1, 0, 1]).tocsr()


@pytest.mark.parametrize("n", [2, 63, 64, 65, 2047, 2048, 2049, 133123])
def test_projection_is_exact_on_integers(env, n):
    """One lane pair, a wavefront -+ 1, a block of 2048 doubles -+ 1, and 66 blocks: more than one ticket group of 64."""
    api, mesh, oracle, ctx = env
    mat = _matrix(api, ctx, api.StencilMatrix.from_csr, _chain(n))
    pre = _build(env, mat, 1.0)
    rng = np.random.default_rng(n)
    ints = rng.integers(-2 ** 20, 2 ** 20 + 1, n)
    divisible = ints.copy()  # ... the same with a sum that n divides: the mean is an integer
    divisible[0] -= int(divisible.sum()) % n
    if abs(int(divisible[0])) > 2 ** 20:
        divisible[0] += n
    assert int(divisible.sum()) % n == 0 and np.abs(divisible).max() <= 2 ** 20
    before, expected = ctx.counter("amg_projections"), 0
    for vals in (ints, divisible, np.full(n, int(ints[0]) or 7)):
        s = int(vals.sum())  # Python integers: exact; every partial sum of the device is an integer below 2^53 too
        v = api.DeviceVector.from_numpy(ctx, vals.astype(np.float64))
        pre.project(v)
        expected += 1
        got = v.to_numpy()
        assert np.array_equal(got, vals.astype(np.float64) - s / n), (n, np.abs(got - (vals - s / n)).max())
        if s % n == 0:
            pre.project(v)
            expected += 1
            assert np.array_equal(v.to_numpy(), got)
        if (vals == vals[0]).all():
            assert not got.any()
    assert ctx.counter("amg_projections") - before == expected >= 3 + 2  # (the divisible and the constant vector: twice)
    pre.close()
    mat.close()


# ---- 2. the cycle ---------------------------------------------------------------------------------------------------------------
DEGREE = dict(box=2, box20=1, lognormal=2, renumbered=2, graph=2)


@pytest.fixture(scope="module")
def cycles(env):
    """Per case: the device object, the restatement in float64 and in long double, the operator."""
    out = {}
    for name in CASES:
        mat, alpha, a = _operator(env, name)
        pre = _build(env, mat, alpha, smoother_degree=DEGREE[name], **PARAMS)
        out[name] = (mat, pre, _restatement(pre), _restatement(pre, np.longdouble), a)
    yield out
    for mat, pre, *_ in out.values():
        pre.close()
        mat.close()


@pytest.mark.parametrize("name", CASES)
def test_cycle_against_the_restatement(env, cycles, name):
    mat, pre, c64, cld, a = cycles[name]
    n = a.shape[0]
    a0 = pre.hierarchy.operator(0)
    slack = (np.diff(a.indptr).max() + 2) * EPS * np.asarray(abs(a).sum(axis=1)).ravel().max()
    assert abs(a0 - a).max() <= slack
    r_host = np.random.default_rng(4).standard_normal(n)
    z_dev, z64, zld = _apply(env, pre, r_host), c64(r_host), cld(r_host)
    margin = 10.0 * float(np.abs(z64 - zld.astype(np.float64)).max())
    diff = float(np.abs(z_dev - z64).max())
    b1 = float(np.abs(_apply(env, pre, np.ones(n))).max())
    print(f"{name}: levels {pre.hierarchy.level_rows()}, |device - restatement| = {diff:.3e}, margin {margin:.3e}, "
          f"|z| = {np.abs(z64).max():.3e}, |B 1| = {b1:.3e}, mean(z) = {z_dev.mean():.3e}")
    assert margin > 0 and diff <= margin
    assert b1 < margin


@pytest.mark.parametrize("name", CASES)
def test_cycle_is_symmetric_and_positive_on_mean_free_vectors(env, cycles, name):
    mat, pre, c64, cld, a = cycles[name]
    n = a.shape[0]
    rng = np.random.default_rng(6)
    u_host, v_host = rng.standard_normal(n), rng.standard_normal(n)
    u_host, v_host = u_host - u_host.mean(), v_host - v_host.mean()
    bu, bv = _apply(env, pre, u_host), _apply(env, pre, v_host)
    ld = np.longdouble
    asym = abs(float(u_host.astype(ld) @ bv.astype(ld) - v_host.astype(ld) @ bu.astype(ld)))
    margin = 10.0 * float(np.abs(u_host) @ np.abs(c64(v_host) - cld(v_host).astype(float)) +
                          np.abs(v_host) @ np.abs(c64(u_host) - cld(u_host).astype(float)))
    print(f"{name}: |<u,Bv> - <v,Bu>| = {asym:.3e}, margin {margin:.3e}, <u,Bu> = {u_host @ bu:.3e}")
    assert asym <= margin
    assert u_host @ bu > 0 and v_host @ bv > 0


# ---- 3. the same bits on every path -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reduced", [0, 1])
@pytest.mark.parametrize("name", ["box", "graph", "chain100"])
def test_options_give_the_same_bits(env, name, reduced):
    api, mesh, oracle, ctx = env
    if name == "chain100":  # one level: Pi Ainv Pi, no closing statement to fuse
        mat, alpha, a = _matrix(api, ctx, api.StencilMatrix.from_csr, _chain(100)), 1.0, _chain(100)
        pre = _build(env, mat, alpha, reduced_records=bool(reduced))
    else:
        mat, alpha, a = _operator(env, name)
        pre = _build(env, mat, alpha, reduced_records=bool(reduced), **PARAMS)
    levels = int(pre.get("levels"))
    assert (levels == 1) == (name == "chain100") and pre.get("reduced") == reduced
    n = a.shape[0]
    r_host = np.random.default_rng(9).standard_normal(n) + 0.25
    keys = ("amg_applies", "amg_projections", "amg_fused_projections", "amg_fused_residuals", "amg_statement_residuals")
    out, counts = [], []
    try:
        for amg_fused, cheb_fused in ((1, 1), (0, 1), (1, 0), (0, 0)):
            ctx.set_option("amg_fused", amg_fused)
            ctx.set_option("cheb_fused", cheb_fused)
            before = [ctx.counter(k) for k in keys]
            out.append(_apply(env, pre, r_host))
            counts.append(tuple(ctx.counter(k) - b for k, b in zip(keys, before)))
    finally:
        ctx.set_option("amg_fused", 1)
        ctx.set_option("cheb_fused", 1)
    print(name, "reduced", reduced, "levels", pre.hierarchy.level_rows(), "counters", counts)
    fused = 1 if levels > 1 else 0
    assert [c[:3] for c in counts] == [(1, 2, fused), (1, 2, 0), (1, 2, fused), (1, 2, 0)]
    assert np.isfinite(out[0]).all() and np.abs(out[0]).max() > 0
    for other in out[1:]:
        assert np.array_equal(out[0], other)
    pre.close()
    mat.close()


# ---- 4. solves --------------------------------------------------------------------------------------------------------------------
def _solve(api, ctx, solver, mat, alpha, b_host, pre_op, side="right"):
    b, x = api.DeviceVector.from_numpy(ctx, b_host), api.DeviceVector(ctx, b_host.size)
    solver.pre_op = pre_op
    solver.pre_side = api.PreconditionerSide.Left if side == "left" else api.PreconditionerSide.Right
    ok = solver.solve(x, b, api.HipStencilOperator(mat, alpha, 0.0))
    return ok, solver.iteration, x.to_numpy()


@pytest.fixture(scope="module")
def plain_counts(env):
    """CG iterations without a preconditioner, per case (computed once on the device)."""
    api, mesh, oracle, ctx = env
    cache = {}

    def count(name, mat, alpha, b_host):
        if name not in cache:
            ok, it, _ = _solve(api, ctx, api.CgSolver(), mat, alpha, b_host, None)
            assert ok
            cache[name] = it
        return cache[name]

    return count


@pytest.mark.parametrize("degree", [1, 2])
@pytest.mark.parametrize("name", CASES)
def test_cg_counts_match_the_restatement_and_beat_plain_cg(env, plain_counts, name, degree):
    api, mesh, oracle, ctx = env
    mat, alpha, a = _operator(env, name)
    n = a.shape[0]
    b_host = nr.mean_free(n)
    pre = api.AmgPreconditioner(nullspace="constant", smoother_degree=degree, **PARAMS)
    before = ctx.counter("amg_applies")
    ok, it, x = _solve(api, ctx, api.CgSolver(), mat, alpha, b_host, pre)
    assert ok and ctx.counter("amg_applies") - before >= it > 0
    ref = oracle.solve("cg", oracle.CsrOperator(a), b_host, pre=oracle.CallbackOperator(n, _restatement(pre)), side="right")
    plain = plain_counts(name, mat, alpha, b_host)
    res = np.linalg.norm(b_host - a @ x) / np.linalg.norm(b_host)
    print(f"{name} degree {degree}: {it} iterations (restatement's PCG {ref.iterations}, plain CG {plain}), levels "
          f"{pre.hierarchy.level_rows()}, true residual {res:.3e}, mean(x) = {x.mean():.3e}, max|x| = {np.abs(x).max():.3e}")
    assert ref.converged and abs(it - ref.iterations) <= 1
    assert it < plain
    assert res <= 1e-5
    assert abs(x.mean()) <= 64 * EPS * np.abs(x).max()
    pre.close()
    mat.close()


@pytest.mark.parametrize("kind,side", [("bicgstab", "left"), ("fgmres", "right")])
def test_other_methods_converge(env, kind, side):
    api, mesh, oracle, ctx = env
    mat, alpha, a = _operator(env, "box")
    b_host = nr.mean_free(a.shape[0])
    pre = api.AmgPreconditioner(nullspace="constant", **PARAMS)
    solver = api.BiCgStabSolver() if kind == "bicgstab" else api.FgmresSolver()
    ok, it, x = _solve(api, ctx, solver, mat, alpha, b_host, pre, side)
    res = np.linalg.norm(b_host - a @ x) / np.linalg.norm(b_host)
    print(f"{kind} {side}: {it} iterations, true residual {res:.3e}")
    assert ok and res <= 1e-4
    pre.close()
    mat.close()


# ---- 5. refresh -------------------------------------------------------------------------------------------------------------------
def _updatable(env, g, w):
    api, mesh, oracle, ctx = env
    return api.StencilMatrix.from_face_weights_updatable(ctx, g.n_cells, 0, g.inner, g.outer, w, w, np.zeros(g.n_cells))


def _set(env, mat, g, w):
    api, mesh, oracle, ctx = env
    mat.set_face_weights(api.DeviceVector.from_numpy(ctx, w), api.DeviceVector.from_numpy(ctx, w),
                         api.DeviceVector.from_numpy(ctx, np.zeros(g.n_cells)))


def _export(h):
    return dict(ops=[h.operator(lv) for lv in range(h.levels)], ps=[h.prolongator(lv) for lv in range(h.levels - 1)],
                aggs=[h.aggregates(lv) for lv in range(h.levels - 1)], masks=[h.strong(lv) for lv in range(h.levels - 1)],
                inv=h.coarse_inverse(), shift=h.get("coarse_shift"))


def _pseudo_inverses_agree(ac, x0, x1, b_inf, what):
    """Two pseudo-inverses by N3 of coarsest matrices that differ by at most b_inf (infinity norm): the bound of
    tests/test_gpu_amg_refresh.py for two inverses, on G = A_c + (s / m) 1 1^T, times 4 for the two projections (the
    infinity norm of Pi is below 2)."""
    m = ac.shape[0]
    s = ac.diagonal().max()
    g = ac + s / m
    r = 64 * m * EPS * np.linalg.cond(g)
    inf = lambda x: float(np.abs(x).sum(axis=1).max())  # noqa: E731
    gi = inf(np.linalg.inv(g))
    bound = 4.0 * (m * r * 2 * gi + gi * b_inf * gi)
    gap = float(np.abs(x1 - x0).max())
    res, res_pinv = np.abs(ac @ x1 @ ac - ac).max(), np.abs(ac @ np.linalg.pinv(ac) @ ac - ac).max()
    print(f"{what}: the pseudo-inverses differ by {gap:.3e} (bound {bound:.3e}); |A Ainv A - A| = {res:.3e} (pinv {res_pinv:.3e})")
    assert gap <= bound and res <= 10.0 * res_pinv


def test_refresh_against_a_fresh_structural_build(env):
    """The object is built on twice the lognormal weights -- the same structure, every number of A doubled exactly -- and
    refreshed to the lognormal set: download() must give what storm_hip_amg_setup_csr_nullspace(structural = 1) builds from
    the new matrix, by the rule of tests/test_gpu_amg_refresh.py for a refresh against a build (patterns, aggregates and
    masks identical; values within the reordered-sum bound); and the refreshed CG count is a fresh build's."""
    api, mesh, oracle, ctx = env
    g, w, a_new = nr.lognormal_box(mesh)
    mat = _updatable(env, g, 2.0 * w)
    pre = _build(env, mat, -1.0, refreshable=True, **PARAMS)
    assert pre.get("refreshable") == 1 and pre.get("structural") == 1 and pre.get("nullspace") == 1
    old = _export(pre.hierarchy)
    _set(env, mat, g, w)
    moved = ctx.counter("amg_refreshes")
    pre.refresh()
    assert ctx.counter("amg_refreshes") == moved + 1
    pre.download()
    got = _export(pre.hierarchy)
    assert abs(got["ops"][1] - old["ops"][1]).max() > 0  # the numbers did move
    fresh = _export(api.AmgHierarchy.from_csr(got["ops"][0], structural=True, nullspace="constant", **PARAMS))
    omega = amg_ref.DEFAULTS["prolongator_omega"]
    a0 = got["ops"][0]
    slack = (np.diff(a_new.indptr).max() + 2) * EPS * np.asarray(abs(a_new).sum(axis=1)).ravel().max()
    assert abs(a0 - a_new).max() <= slack
    assert len(got["ops"]) == len(fresh["ops"]) >= 3
    for x, y in zip(got["ops"] + got["ps"], fresh["ops"] + fresh["ps"]):
        assert rr.same_pattern(x, y)
    for x, y in zip(got["aggs"] + got["masks"], fresh["aggs"] + fresh["masks"]):
        assert np.array_equal(x, y)
    for lv in range(len(fresh["ps"])):
        al, p0 = fresh["ops"][lv], fresh["ps"][lv]
        rr.within(got["ps"][lv], p0, *rr.prolongator_bound(al, fresh["masks"][lv], fresh["aggs"][lv], p0.shape[1], omega), f"P_{lv}")
        rr.within(got["ops"][lv + 1], fresh["ops"][lv + 1], *rr.coarse_bound(al, p0), f"A_{lv + 1}")
        print(f"P_{lv} differs by {abs(got['ps'][lv] - p0).max():.3e}, A_{lv + 1} by {abs(got['ops'][lv + 1] - fresh['ops'][lv + 1]).max():.3e}")
    terms, magnitude = rr.coarse_bound(fresh["ops"][-2], fresh["ps"][-1])
    b_inf = float(np.abs(((8.0 * EPS) * terms.multiply(magnitude)).toarray()).sum(axis=1).max())
    _pseudo_inverses_agree(got["ops"][-1].toarray(), fresh["inv"], got["inv"], b_inf, "refreshed against fresh")
    assert got["shift"] == got["ops"][-1].diagonal().max()
    # CG with the refreshed object against a fresh refreshable build on the new weights
    b_host = nr.mean_free(g.n_cells)
    ok, it, x = _solve(api, ctx, api.CgSolver(), mat, -1.0, b_host, pre)
    mat2 = _updatable(env, g, w)
    pre2 = api.AmgPreconditioner(nullspace="constant", refreshable=True, **PARAMS)
    ok2, it2, _ = _solve(api, ctx, api.CgSolver(), mat2, -1.0, b_host, pre2)
    print(f"CG: refreshed {it}, fresh build {it2}")
    assert ok and ok2 and it == it2
    assert np.linalg.norm(b_host - a_new @ x) <= 1e-5 * np.linalg.norm(b_host)
    for o in (pre, pre2, mat, mat2):
        o.close()


def test_refresh_to_new_weights_against_the_frozen_restatement(env):
    """From unit weights to the lognormal set: the structure stays that of the unit weights, every level is the frozen
    recipe's (tests/amg_refresh_ref.py) and the coarsest level's Ainv is N3's."""
    api, mesh, oracle, ctx = env
    g, w, a_new = nr.lognormal_box(mesh)
    mat = _updatable(env, g, np.ones(g.inner.size))
    pre = _build(env, mat, -1.0, refreshable=True, **PARAMS)
    frozen = _export(pre.hierarchy)
    _set(env, mat, g, w)
    pre.refresh()
    pre.download()
    got = _export(pre.hierarchy)
    omega = amg_ref.DEFAULTS["prolongator_omega"]
    for x, y in zip(got["aggs"] + got["masks"], frozen["aggs"] + frozen["masks"]):
        assert np.array_equal(x, y)
    for x, y in zip(got["ops"] + got["ps"], frozen["ops"] + frozen["ps"]):
        assert rr.same_pattern(x, y)
    slack = (np.diff(a_new.indptr).max() + 2) * EPS * np.asarray(abs(a_new).sum(axis=1)).ravel().max()
    assert abs(got["ops"][0] - a_new).max() <= slack
    for lv in range(len(got["ps"])):
        al, mask, agg = got["ops"][lv], got["masks"][lv], got["aggs"][lv]
        count = got["ps"][lv].shape[1]
        p_ref, c_ref = rr.frozen_level(al, mask, agg, count, omega)
        p_lib, c_lib = got["ps"][lv], got["ops"][lv + 1]
        assert rr.same_pattern(p_lib, p_ref) and rr.same_pattern(c_lib, c_ref)
        rr.within(p_lib, p_ref, *rr.prolongator_bound(al, mask, agg, count, omega), f"P_{lv}")
        rr.within(c_lib, rr.on_pattern(p_lib.T @ al @ p_lib, rr.ones(c_ref)), *rr.coarse_bound(al, p_lib), f"A_{lv + 1}")
    ac = got["ops"][-1].toarray()
    ref, s = nr.coarse_inverse(ac)
    assert got["shift"] == s
    _pseudo_inverses_agree(ac, ref, got["inv"], 0.0, "refreshed against N3 restated")
    # ... and the cycle reads what was refreshed
    r_host = np.random.default_rng(4).standard_normal(g.n_cells)
    z64, zld = _restatement(pre)(r_host), _restatement(pre, np.longdouble)(r_host)
    margin = 10.0 * float(np.abs(z64 - zld.astype(np.float64)).max())
    diff = float(np.abs(_apply(env, pre, r_host) - z64).max())
    print(f"cycle after the refresh: |device - restatement| = {diff:.3e}, margin {margin:.3e}")
    assert diff <= margin
    pre.close()
    mat.close()


def test_refresh_refuses_a_cut_box(env):
    """The weights of the plane of faces between x-layers 5 and 6 are 0, which cuts the box in two: the refresh returns
    E_INVALID (by which check: the module's docstring) and the object refuses apply until a good refresh."""
    api, mesh, oracle, ctx = env
    from stormruler_amd._lib import lib

    g, w, _ = nr.lognormal_box(mesh)
    mat = _updatable(env, g, w)
    pre = _build(env, mat, -1.0, refreshable=True, **PARAMS)
    d = g.center[g.outer] - g.center[g.inner]
    mid = 0.5 * (g.center[g.outer] + g.center[g.inner])
    cut = (np.abs(d).argmax(axis=1) == 0) & np.isclose(mid[:, 0], 0.5)
    assert cut.sum() == 10 * 9
    w_cut = np.where(cut, 0.0, w)
    assert nr.components(nr.face_weight_matrix(g, w_cut)) == 2
    _set(env, mat, g, w_cut)
    st = lib.storm_hip_amg_refresh(pre._h)
    msg = lib.storm_hip_last_error().decode()
    print(f"refresh on the cut box: status {st}" + (f" ({msg})" if st else ""))
    if st == 0:
        pre.download()
        ac = pre.hierarchy.operator(int(pre.get("levels")) - 1).toarray()
        s = pre.get("coarse_shift")
        print(f"  smallest eigenvalue of G / s = {np.linalg.eigvalsh(ac + s / ac.shape[0]).min() / s:.3e}")
    assert st == E_INVALID
    n = g.n_cells
    r, z = api.DeviceVector.from_numpy(ctx, np.ones(n)), api.DeviceVector(ctx, n)
    assert lib.storm_hip_amg_apply(pre._h, r._h, z._h) == E_INVALID
    _set(env, mat, g, w)
    pre.refresh()
    pre.mul(z, r)
    pre.close()
    mat.close()


# ---- 6. refusals and plumbing ---------------------------------------------------------------------------------------------------
def test_refusals(env):
    api, mesh, oracle, ctx = env
    from stormruler_amd._lib import lib

    def create(mat, alpha=-1.0, beta=0.0, refreshable=0, **kw):
        h = C.c_void_p()
        p = api._amg_params(**kw)
        st = lib.storm_hip_amg_create_nullspace(mat._h, alpha, beta, C.byref(p), refreshable, C.byref(h))
        msg = lib.storm_hip_last_error().decode()
        if st == 0:
            lib.storm_hip_amg_destroy(h)
        else:
            assert not h.value
        return st, msg

    g = mesh.structured_box(6)
    dirichlet = _matrix(api, ctx, api.StencilMatrix.from_face_graph, g)
    st, msg = create(dirichlet)  # N1
    assert st == E_INVALID and "row 0 " in msg and "constants" in msg
    gn = nr.neumann_box_graph(mesh, 6, 6, 6)
    neumann = _matrix(api, ctx, api.StencilMatrix.from_face_graph, gn)
    st, msg = create(neumann, beta=0.5)  # N1 again: beta != 0
    assert st == E_INVALID and "constants" in msg
    st, msg = create(neumann, smoother_degree=17)
    assert st == E_INVALID and "smoother_degree" in msg
    st, msg = create(neumann, refreshable=1)
    assert st == E_UNSUPPORTED and "updatable" in msg
    assert create(neumann)[0] == 0
    compact = api.StencilMatrix.from_face_graph(ctx, gn)  # the default compact records
    assert compact.stats()["value_dictionary_size"] > 0
    st, msg = create(compact)
    assert st == E_UNSUPPORTED and "compact" in msg
    loc, send_idx = mesh.periodic_z_local_graph(8, 8, 8)
    halo = _matrix(api, ctx, api.StencilMatrix.from_face_graph, loc)
    st, msg = create(halo)
    assert st == E_UNSUPPORTED and "single-rank" in msg
    # storm_hip_amg_create on the two-cell Neumann operator still refuses, and its message names the way out
    two = _matrix(api, ctx, api.StencilMatrix.from_face_weights, 2, 0, np.array([0]), np.array([1]), np.array([1.0]), np.array([1.0]), None)
    h = C.c_void_p()
    assert lib.storm_hip_amg_create(two._h, -1.0, 0.0, None, C.byref(h)) == E_INVALID and not h.value
    msg = lib.storm_hip_last_error().decode()
    assert "singular" in msg and "nullspace" in msg
    assert create(two)[0] == 0
    # project: a vector of another size; a plain object
    pre = _build(env, neumann, -1.0)
    n = gn.n_cells
    short, full = api.DeviceVector(ctx, n - 1), api.DeviceVector.from_numpy(ctx, np.arange(n, dtype=np.float64))
    assert lib.storm_hip_amg_project(pre._h, short._h) == E_INVALID and b"rows" in lib.storm_hip_last_error()
    pre.project(full)
    assert np.array_equal(full.to_numpy(), np.arange(n) - (n - 1) / 2)
    plain = api.AmgPreconditioner()
    x = api.DeviceVector(ctx, g.n_cells)
    plain.build(x, x, api.HipStencilOperator(dirichlet, -1.0, 0.0))
    assert plain.get("nullspace") == 0
    assert lib.storm_hip_amg_project(plain._h, x._h) == E_UNSUPPORTED and b"amg_create_nullspace" in lib.storm_hip_last_error()
    for o in (pre, plain, dirichlet, neumann, compact, halo, two):
        o.close()


def test_hierarchy_from_a_second_matrix(env):
    """AmgPreconditioner(matrix=...): the outer operator keeps its compact records, the hierarchy comes from an fp64 copy."""
    api, mesh, oracle, ctx = env
    g, a = nr.neumann_box(mesh, 12, 10, 9)
    compact = api.StencilMatrix.from_face_graph(ctx, g)
    fp64 = _matrix(api, ctx, api.StencilMatrix.from_face_graph, g)
    assert compact.stats()["value_dictionary_size"] > 0 and fp64.stats()["value_dictionary_size"] == 0
    b_host = nr.mean_free(g.n_cells)
    pre = api.AmgPreconditioner(nullspace="constant", matrix=fp64, **PARAMS)
    ok, it, x = _solve(api, ctx, api.CgSolver(), compact, -1.0, b_host, pre)
    handle = pre._h.value
    ok_again, it_again, _ = _solve(api, ctx, api.CgSolver(), compact, -1.0, b_host, pre)
    assert pre._h.value == handle and it_again == it  # the cache key holds: no second setup
    pre64 = api.AmgPreconditioner(nullspace="constant", **PARAMS)
    ok64, it64, _ = _solve(api, ctx, api.CgSolver(), fp64, -1.0, b_host, pre64)
    print(f"compact outer records with matrix=: {it} iterations; fp64 outer records: {it64}")
    assert ok and ok_again and ok64 and abs(it - it64) <= 1
    assert np.linalg.norm(b_host - a @ x) <= 1e-5 * np.linalg.norm(b_host)
    with pytest.raises(RuntimeError):  # without matrix= the compact records are refused, as by a plain object
        api.AmgPreconditioner(nullspace="constant").build(api.DeviceVector(ctx, g.n_cells), None, api.HipStencilOperator(compact, -1.0, 0.0))
    for o in (pre, pre64, compact, fp64):
        o.close()


def test_cavity_driver_with_the_multigrid_pressure_solve(env):
    api, mesh, oracle, ctx = env
    from stormruler_amd.cavity import CavityProjection

    before = ctx.counter("option_spmv_dict")
    plain, amg = CavityProjection(ctx, 16), CavityProjection(ctx, 16, pressure_preconditioner="amg")
    assert ctx.counter("option_spmv_dict") == before  # the option is restored
    assert plain.solver.pre_op is None and amg.solver.pre_op.get("nullspace") == 1
    assert amg.L_N.stats()["value_dictionary_size"] > 0 and amg.L_N64.stats()["value_dictionary_size"] == 0
    for step in range(3):
        it_p, _, ok_p = plain.step()
        it_a, _, ok_a = amg.step()
        print(f"step {step}: pressure iterations plain {it_p}, multigrid {it_a}")
        assert ok_p and ok_a and 0 < it_a < it_p
    d_p, d_a = plain.divergence_norm(), amg.divergence_norm()
    print(f"divergence norm after three steps: plain {d_p:.3e}, multigrid {d_a:.3e}")
    assert d_a <= 10.0 * d_p
    with pytest.raises(ValueError):
        CavityProjection(ctx, 16, pressure_preconditioner="jacobi")
    with pytest.raises(ValueError):
        CavityProjection(ctx, 16, graph=mesh.structured_box(16), pressure_preconditioner="amg")


def test_cpp_driver(env):
    api, mesh, oracle, ctx = env
    exe = os.path.join(ROOT, "tests", "cpp", "amg_nullspace_driver")
    if not os.path.exists(exe):  # (git-ignored: a checkout that arrived without it)
        import __graft_entry__ as ge

        ge.build()
    out = subprocess.run([exe, "12", "10", "9", "2", "16"], check=True, capture_output=True, text=True, timeout=300).stdout
    got = json.loads(out.strip().splitlines()[-1])
    print(got)
    assert got["converged"] and got["nullspace"] == 1 and got["coarse_shift"] > 0
    g = nr.neumann_box_graph(mesh, 12, 10, 9)  # the driver's box has unit spacing: all weights 1
    host = api.AmgHierarchy.from_csr(nr.face_weight_matrix(g, np.ones(g.inner.size)), nullspace="constant", **PARAMS)
    assert got["level_rows"] == host.level_rows() and len(got["level_rows"]) == 3
    assert 0 < got["iterations"] <= 9  # (the restatement's PCG takes 7 on the 12 x 10 x 9 boxes at degree 2)
    assert got["true_relative_residual"] <= 1e-5
    assert abs(got["mean_x"]) <= 64 * EPS * got["max_abs_x"] and abs(got["mean_projected_x"]) <= 64 * EPS * got["max_abs_x"]
    assert got["amg_projections"] == 2 * got["amg_applies"] + 1 and got["amg_fused_projections"] == got["amg_applies"]
