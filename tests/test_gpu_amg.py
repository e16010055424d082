"""The smoothed-aggregation multigrid preconditioner (storm_hip_amg_*, csrc/amg.hip) on the device:

1. the fused residual kernel gives the two statements' bits, and so does the cycle with the Chebyshev smoothers' fused step
   off as well (counters say which path ran): 13^3 box (ragged last slice, three levels), 20^3 box (a coarsest level of 7
   rows: smaller than a wavefront), the random CSR with ell_cap set so that a level has a CSR tail and falls to the
   statements by itself, 52^3 box (more than 8 x 64 blocks: the XCD runs are active);
2. with prolongator_omega = 0 (P is 0 / 1) restriction and prolongation of integer-valued vectors equal numpy bit for bit;
3. with the smoothed P every row of a transfer, and of the coarse GEMV, is within (k_i + 1) 2^-53 sum |w x| of math.fsum;
4. the cycle against the numpy restatement (tests/amg_ref.py) on the exported hierarchy;
5. symmetry and positivity of B;
6. solves: iteration counts against the restatement's PCG, and below the Jacobi-scaled Chebyshev degree-2 count;
7. refusals and the C++ driver.

The boxes are the 7-point Laplacian (diagonal 6, tests/amg_cases.py) built from CSR on fp64 records; the face-weight cases
go through StencilMatrix.from_face_weights.

Calibration of 4 and 5 (margin = 10 x the difference between the restatement in float64 and in np.longdouble on the same
input; the tests print the figures they measure beside it).  First run on an MI355X:
  cycle, max |device - restatement| / margin:  13^3 4.4e-16 / 4.4e-15;  20^3 (degree 1) 6.7e-16 / 5.6e-15;
                                               random CSR 3.3e-16 / 2.2e-15;  1 : 1 : 100 weights 8.3e-17 / 6.9e-16
  symmetry, |<u,Bv> - <v,Bu>| / margin:        13^3 4.3e-15 / 2.0e-12;  random CSR 2.2e-15 / 5.1e-13;  1 : 1 : 100 1.1e-15 / 5.9e-13
  transfers use at most 0.56 of the row bound of 3, the coarse solve 0.08; CG counts 10 (degree 1) and 7 (degree 2) on every
  shape, equal to the restatement's, against 16 - 26 with the Chebyshev polynomial."""
import ctypes as C
import json
import math
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import amg_cases  # noqa: E402
import amg_ref  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_UNSUPPORTED = -1, -6


@pytest.fixture(scope="module")
def env():
    from oracle import oracle
    from stormruler_amd import api, mesh

    ctx = api.Context(0)
    yield api, mesh, oracle, ctx
    ctx.close()


def _matrix(api, ctx, build, *args, ell_cap=0):
    """A StencilMatrix on fp64 records (spmv_dict = 0), options restored afterwards."""
    ctx.set_option("spmv_dict", 0)
    ctx.set_option("ell_cap", ell_cap)
    try:
        return build(ctx, *args)
    finally:
        ctx.set_option("spmv_dict", 4)
        ctx.set_option("ell_cap", 0)


def _operator(env, name):
    """(matrix, alpha, beta, assembled A, multigrid parameters) of a named case."""
    api, mesh, oracle, ctx = env
    if name.startswith("box"):
        n = int(name[3:])
        a = amg_cases.poisson_box(n)
        return _matrix(api, ctx, api.StencilMatrix.from_csr, a), 1.0, 0.0, a, dict(coarse_rows=32 if n in (13, 20) else 512)
    if name in ("aniso", "lognormal"):
        g, w, diag_extra, a = amg_cases.face_weight_case(mesh, 16, name)
        mat = _matrix(api, ctx, api.StencilMatrix.from_face_weights, g.n_cells, 0, g.inner, g.outer, w, w, diag_extra)
        return mat, -1.0, 0.0, a, {}
    assert name == "random"
    a = amg_cases.random_symmetric()
    return _matrix(api, ctx, api.StencilMatrix.from_csr, a), 1.0, 0.0, a, dict(coarse_rows=32)


def _build(env, mat, alpha, beta, ell_cap=0, **params):
    api, mesh, oracle, ctx = env
    pre = api.AmgPreconditioner(**params)
    x = api.DeviceVector(ctx, mat.stats()["n_rows"])
    ctx.set_option("ell_cap", ell_cap)  # (the coarse operators go through the packer under the context's cap)
    try:
        pre.build(x, x, api.HipStencilOperator(mat, alpha, beta))
    finally:
        ctx.set_option("ell_cap", 0)
    return pre


def _restatement(pre, dtype=np.float64):
    h = pre.hierarchy
    ops = [h.operator(lv) for lv in range(h.levels)]
    ps = [h.prolongator(lv) for lv in range(h.levels - 1)]
    return amg_ref.Cycle(ops, ps, h.coarse_inverse(), degree=int(pre.get("smoother_degree")), dtype=dtype)


# ---- 1. the same bits on every path ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,degree", [("box13", 2), ("box13", 1), ("box20", 2), ("random_tail", 2), ("box52", 2)])
def test_fused_residual_gives_the_statements_bits(env, name, degree):
    api, mesh, oracle, ctx = env
    tail = name == "random_tail"
    mat, alpha, beta, a, params = _operator(env, "random" if tail else name)
    pre = _build(env, mat, alpha, beta, ell_cap=8 if tail else 0, smoother_degree=degree, **params)
    levels = int(pre.get("levels"))
    rows = pre.hierarchy.level_rows()
    st = mat.stats()
    assert st["value_dictionary_size"] == 0 and st["paired_rows"] == 0 and st["tail_rows"] == 0
    if name == "box13":
        assert rows == [2197, 280, 16] and rows[0] % 64 != 0
    if name == "box20":
        assert rows == [8000, 1040, 50, 7]
    if name == "box52":
        assert st["spmv_blocks"] > 8 * 64 and st["xcd_run_blocks"] == 64
    n = rows[0]
    r_host = np.sin(0.37 * np.arange(n)) + 0.25
    r, z = api.DeviceVector.from_numpy(ctx, r_host), api.DeviceVector(ctx, n)
    out, counts = [], []
    keys = ("amg_applies", "amg_fused_residuals", "amg_statement_residuals", "cheb_fused_applies", "cheb_statement_applies")
    try:
        for amg_fused, cheb_fused in ((1, 1), (0, 1), (0, 0)):
            ctx.set_option("amg_fused", amg_fused)
            ctx.set_option("cheb_fused", cheb_fused)
            z.upload(np.full(n, np.nan))  # (the cycle must not read z)
            before = [ctx.counter(k) for k in keys]
            pre.mul(z, r)
            out.append(z.to_numpy())
            counts.append(tuple(ctx.counter(k) - b for k, b in zip(keys, before)))
            assert np.array_equal(r.to_numpy(), r_host)  # r is not written
    finally:
        ctx.set_option("amg_fused", 1)
        ctx.set_option("cheb_fused", 1)
    per = 2 * (levels - 1)  # residuals, and smoother applies, of a cycle
    print(name, "levels", rows, "counters", counts)
    if tail:  # level 1 (69 rows, rows wider than the cap) has a CSR tail: statements by itself, on both objects
        assert rows == [918, 69, 1]
        assert counts[0] == (1, 2, 2, 2, 2)
    else:
        assert counts[0] == (1, per, 0, per, 0)
    assert counts[1][:3] == (1, 0, per) and counts[2] == (1, 0, per, 0, per)
    assert np.isfinite(out[0]).all() and np.abs(out[0]).max() > 0
    assert np.array_equal(out[0], out[1]) and np.array_equal(out[0], out[2])
    pre.close()
    mat.close()


# ---- 2. / 3. the transfers and the coarse solve -----------------------------------------------------------------------------
def test_unsmoothed_transfers_are_exact_on_integers(env):
    api, mesh, oracle, ctx = env
    mat, alpha, beta, a, params = _operator(env, "box13")
    pre = _build(env, mat, alpha, beta, prolongator_omega=0.0, **params)
    h = pre.hierarchy
    rng = np.random.default_rng(1)
    for lv in range(h.levels - 1):
        p = h.prolongator(lv)
        assert (p.data == 1.0).all()
        nf, nc = p.shape
        fine_host = rng.integers(-1000, 1000, nf).astype(np.float64)
        coarse_host = rng.integers(-1000, 1000, nc).astype(np.float64)
        fine, coarse = api.DeviceVector.from_numpy(ctx, fine_host), api.DeviceVector(ctx, nc)
        coarse.upload(np.full(nc, np.nan))
        pre.restrict(lv, fine, coarse)
        assert np.array_equal(coarse.to_numpy(), p.T @ fine_host)  # integer sums: exact in any order
        coarse.upload(coarse_host)
        pre.prolong_add(lv, coarse, fine)
        assert np.array_equal(fine.to_numpy(), fine_host + p @ coarse_host)
        assert np.array_equal(coarse.to_numpy(), coarse_host)
    pre.close()
    mat.close()


def _rows_within_fsum(m, x, got, base=None):
    """Every row of got = [base +] m x within (k_i + 1) 2^-53 sum |w x| of math.fsum over the row's EXACT products (each
    product as its rounded value plus its rounding error, which is a double: the kernels' fma does not round a product).
    Returns the largest share of the bound a row uses."""
    worst = 0.0
    for i in range(m.shape[0]):
        terms, magnitude, k = [], 0.0, 0
        for wk, c in zip(m.data[m.indptr[i]:m.indptr[i + 1]], m.indices[m.indptr[i]:m.indptr[i + 1]]):
            u, v = float(wk), float(x[c])
            p = u * v
            terms += [p, float(Fraction(u) * Fraction(v) - Fraction(p))]
            magnitude += abs(p)
            k += 1
        if base is not None:
            terms.append(float(base[i]))
            magnitude += abs(float(base[i]))
            k += 1
        err = abs(float(got[i]) - math.fsum(terms))
        bound = (k + 1) * 2.0 ** -53 * magnitude
        assert err <= bound, (i, err, bound)
        if bound > 0:
            worst = max(worst, err / bound)
    return worst


def test_smoothed_transfers_and_the_coarse_solve_row_by_row(env):
    api, mesh, oracle, ctx = env
    mat, alpha, beta, a, params = _operator(env, "box13")
    pre = _build(env, mat, alpha, beta, **params)
    h = pre.hierarchy
    rng = np.random.default_rng(2)
    for lv in range(h.levels - 1):
        p = h.prolongator(lv).tocsr()
        r_mat = p.T.tocsr()
        r_mat.sort_indices()
        nf, nc = p.shape
        fine_host, coarse_host = rng.standard_normal(nf), rng.standard_normal(nc)
        fine, coarse = api.DeviceVector.from_numpy(ctx, fine_host), api.DeviceVector(ctx, nc)
        pre.restrict(lv, fine, coarse)
        w1 = _rows_within_fsum(r_mat, fine_host, coarse.to_numpy())
        coarse.upload(coarse_host)
        pre.prolong_add(lv, coarse, fine)
        w2 = _rows_within_fsum(p, coarse_host, fine.to_numpy(), base=fine_host)
        print(f"level {lv}: restriction uses {w1:.3f} of its bound, prolongation {w2:.3f}; padding {pre.get('transfer_padding'):.3f}")
    import scipy.sparse as sp

    inv = h.coarse_inverse()
    nc = inv.shape[0]
    rc_host = rng.standard_normal(nc)
    rc, zc = api.DeviceVector.from_numpy(ctx, rc_host), api.DeviceVector(ctx, nc)
    pre.coarse_solve(rc, zc)
    w3 = _rows_within_fsum(sp.csr_matrix(inv), rc_host, zc.to_numpy())
    print(f"coarse solve ({nc} rows) uses {w3:.3f} of its bound")
    assert 0.0 <= pre.get("transfer_padding") < 1.0
    pre.close()
    mat.close()


# ---- 4. / 5. the cycle ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cycles(env):
    """Per case: the device object, the restatement in float64 and in long double, the operator."""
    api, mesh, oracle, ctx = env
    out = {}
    for name, degree in (("box13", 2), ("box20", 1), ("random", 2), ("aniso", 2)):
        mat, alpha, beta, a, params = _operator(env, name)
        pre = _build(env, mat, alpha, beta, smoother_degree=degree, **params)
        out[name] = (mat, pre, _restatement(pre), _restatement(pre, np.longdouble), a)
    yield out
    for mat, pre, *_ in out.values():
        pre.close()
        mat.close()


@pytest.mark.parametrize("name", ["box13", "box20", "random", "aniso"])
def test_cycle_against_the_restatement(env, cycles, name):
    api, mesh, oracle, ctx = env
    mat, pre, c64, cld, a = cycles[name]
    n = a.shape[0]
    # the decoded level-0 operator is the assembled matrix (a_ii = beta + alpha (ext_i - sum w): one rounding per term)
    a0 = pre.hierarchy.operator(0)
    slack = (np.diff(a.indptr).max() + 2) * np.finfo(float).eps * np.asarray(abs(a).sum(axis=1)).ravel().max()
    assert abs(a0 - a).max() <= slack
    r_host = np.random.default_rng(4).standard_normal(n)
    r, z = api.DeviceVector.from_numpy(ctx, r_host), api.DeviceVector(ctx, n)
    pre.mul(z, r)
    z_dev, z64, zld = z.to_numpy(), c64(r_host), cld(r_host)
    margin = 10.0 * float(np.abs(z64 - zld.astype(np.float64)).max())
    diff = float(np.abs(z_dev - z64).max())
    print(f"{name}: |device - restatement| = {diff:.3e}, margin {margin:.3e}, |z| = {np.abs(z64).max():.3e}")
    assert margin > 0 and diff <= margin


@pytest.mark.parametrize("name", ["box13", "random", "aniso"])
def test_cycle_is_symmetric_and_positive(env, cycles, name):
    api, mesh, oracle, ctx = env
    mat, pre, c64, cld, a = cycles[name]
    n = a.shape[0]
    rng = np.random.default_rng(6)
    u_host, v_host = rng.standard_normal(n), rng.standard_normal(n)
    u, v, z = api.DeviceVector.from_numpy(ctx, u_host), api.DeviceVector.from_numpy(ctx, v_host), api.DeviceVector(ctx, n)
    pre.mul(z, u)
    bu = z.to_numpy()
    pre.mul(z, v)
    bv = z.to_numpy()
    ld = np.longdouble
    asym = abs(float(u_host.astype(ld) @ bv.astype(ld) - v_host.astype(ld) @ bu.astype(ld)))
    margin = 10.0 * float(np.abs(u_host) @ np.abs(c64(v_host) - cld(v_host).astype(float)) +
                          np.abs(v_host) @ np.abs(c64(u_host) - cld(u_host).astype(float)))
    print(f"{name}: |<u,Bv> - <v,Bu>| = {asym:.3e}, margin {margin:.3e}, <u,Bu> = {u_host @ bu:.3e}")
    assert asym <= margin
    assert u_host @ bu > 0 and v_host @ bv > 0


# ---- 6. solves --------------------------------------------------------------------------------------------------------------
def _solve(api, ctx, solver, mat, alpha, beta, b_host, pre_op, side="right"):
    b, x = api.DeviceVector.from_numpy(ctx, b_host), api.DeviceVector(ctx, b_host.size)
    solver.pre_op = pre_op
    solver.pre_side = api.PreconditionerSide.Left if side == "left" else api.PreconditionerSide.Right
    ok = solver.solve(x, b, api.HipStencilOperator(mat, alpha, beta))
    return ok, solver.iteration, x.to_numpy()


@pytest.fixture(scope="module")
def chebyshev_counts(env):
    """CG iterations with the Jacobi-scaled Chebyshev polynomial of degree 2, per case (computed once)."""
    api, mesh, oracle, ctx = env
    cache = {}

    def count(name, mat, alpha, beta, b_host):
        if name not in cache:
            ok, it, _ = _solve(api, ctx, api.CgSolver(), mat, alpha, beta, b_host, api.ChebyshevPreconditioner(degree=2, jacobi=True))
            assert ok
            cache[name] = it
        return cache[name]

    return count


@pytest.mark.parametrize("degree", [1, 2])
@pytest.mark.parametrize("name", ["box13", "box20", "box24", "lognormal", "aniso"])
def test_cg_counts_match_the_restatement_and_beat_chebyshev(env, chebyshev_counts, name, degree):
    api, mesh, oracle, ctx = env
    mat, alpha, beta, a, params = _operator(env, name)
    n = a.shape[0]
    b_host = np.random.default_rng(8).standard_normal(n)
    pre = api.AmgPreconditioner(smoother_degree=degree, **params)
    before = ctx.counter("amg_applies")
    ok, it, x = _solve(api, ctx, api.CgSolver(), mat, alpha, beta, b_host, pre)
    assert ok and ctx.counter("amg_applies") - before >= it > 0
    cycle = _restatement(pre)
    ref = oracle.solve("cg", oracle.CsrOperator(a), b_host, pre=oracle.CallbackOperator(n, cycle), side="right")
    cheb = chebyshev_counts(name, mat, alpha, beta, b_host)
    print(f"{name} degree {degree}: {it} iterations (restatement's PCG {ref.iterations}, Chebyshev degree 2 {cheb}), "
          f"levels {pre.hierarchy.level_rows()}, operator complexity {pre.get('operator_complexity'):.3f}")
    assert ref.converged and abs(it - ref.iterations) <= 1
    assert it < cheb
    assert np.linalg.norm(b_host - a @ x) <= 1e-5 * np.linalg.norm(b_host)
    pre.close()
    mat.close()


@pytest.mark.parametrize("side", ["left", "right"])
@pytest.mark.parametrize("kind", ["bicgstab", "fgmres"])
def test_other_methods_and_sides(env, kind, side):
    api, mesh, oracle, ctx = env
    mat, alpha, beta, a, params = _operator(env, "box13")
    n = a.shape[0]
    b_host = np.random.default_rng(8).standard_normal(n)
    pre = api.AmgPreconditioner(**params)
    solver = api.BiCgStabSolver() if kind == "bicgstab" else api.FgmresSolver()
    ok, it, x = _solve(api, ctx, solver, mat, alpha, beta, b_host, pre, side)
    cycle = _restatement(pre)
    pre_ref = oracle.CallbackOperator(n, cycle)
    if kind == "fgmres":
        ref, _ = oracle.solve_gmres_pre(oracle.CsrOperator(a), pre_ref, b_host, side=side, flexible=True)
    else:
        ref = oracle.solve(kind, oracle.CsrOperator(a), b_host, pre=pre_ref, side=side)
    print(f"{kind} {side}: {it} iterations (oracle {ref.iterations})")
    assert ok and ref.converged and abs(it - ref.iterations) <= 1
    assert np.linalg.norm(b_host - a @ x) <= 1e-4 * np.linalg.norm(b_host)
    pre.close()
    mat.close()


def test_reduced_records_smoothers(env):
    api, mesh, oracle, ctx = env
    mat, alpha, beta, a, params = _operator(env, "box20")
    b_host = np.random.default_rng(8).standard_normal(a.shape[0])
    pre64 = api.AmgPreconditioner(**params)
    ok64, it64, _ = _solve(api, ctx, api.CgSolver(), mat, alpha, beta, b_host, pre64)
    pre64.close()
    pre32 = api.AmgPreconditioner(reduced_records=True, **params)
    before = ctx.counter("cheb_reduced_applies")
    ok32, it32, x = _solve(api, ctx, api.CgSolver(), mat, alpha, beta, b_host, pre32)
    moved = ctx.counter("cheb_reduced_applies") - before
    print(f"fp64 smoothers {it64} iterations, fp32-weight smoothers {it32}; cheb_reduced_applies + {moved}")
    assert ok64 and ok32 and abs(it32 - it64) <= 1
    assert pre32.get("reduced") == 1 and moved >= 2 * (int(pre32.get("levels")) - 1) * it32 > 0
    assert mat.reduced_bytes > 0
    assert np.linalg.norm(b_host - a @ x) <= 1e-5 * np.linalg.norm(b_host)
    pre32.close()
    mat.close()


def test_one_level_hierarchy_is_the_dense_solve(env):
    api, mesh, oracle, ctx = env
    a = amg_cases.poisson_box(5)  # 125 rows <= coarse_rows: the object is the dense inverse
    mat = _matrix(api, ctx, api.StencilMatrix.from_csr, a)
    pre = _build(env, mat, 1.0, 0.0)
    assert pre.get("levels") == 1
    r_host = np.random.default_rng(3).standard_normal(125)
    r, z = api.DeviceVector.from_numpy(ctx, r_host), api.DeviceVector(ctx, 125)
    pre.mul(z, r)
    assert np.linalg.norm(a @ z.to_numpy() - r_host) <= 1e-12 * np.linalg.norm(r_host)
    pre.close()
    mat.close()


def test_hierarchy_is_kept_across_solves(env):
    """A solver calls build() before every solve: the setup must run once per operator, and again after close()."""
    api, mesh, oracle, ctx = env
    mat, alpha, beta, a, params = _operator(env, "box13")
    pre = api.AmgPreconditioner(**params)
    b_host = np.ones(a.shape[0])
    ok, it1, _ = _solve(api, ctx, api.CgSolver(), mat, alpha, beta, b_host, pre)
    handle, stamp = pre._h.value, pre.get("setup_seconds")
    ok2, it2, _ = _solve(api, ctx, api.CgSolver(), mat, alpha, beta, b_host, pre)
    assert ok and ok2 and it1 == it2
    assert pre._h.value == handle and pre.get("setup_seconds") == stamp  # the same object: no second setup
    pre.params["smoother_degree"] = 1  # other parameters: another hierarchy object
    ok3, it3, _ = _solve(api, ctx, api.CgSolver(), mat, alpha, beta, b_host, pre)
    assert ok3 and it3 > it2 and pre.get("smoother_degree") == 1
    pre.close()
    assert pre._h is None
    ok4, it4, _ = _solve(api, ctx, api.CgSolver(), mat, alpha, beta, b_host, pre)
    assert ok4 and it4 == it3 and pre._h is not None
    pre.close()
    mat.close()


# ---- 7. refusals and the C++ driver -----------------------------------------------------------------------------------------
def test_refusals(env):
    api, mesh, oracle, ctx = env
    from stormruler_amd import _lib
    from stormruler_amd._lib import lib

    def create(mat, alpha=-1.0, beta=0.0, **kw):
        h = C.c_void_p()
        p = api._amg_params(**kw)
        st = lib.storm_hip_amg_create(mat._h, alpha, beta, C.byref(p), C.byref(h))
        msg = lib.storm_hip_last_error().decode()
        if st == 0:
            lib.storm_hip_amg_destroy(h)
        else:
            assert not h.value
        return st, msg

    g = mesh.structured_box(6)
    compact = api.StencilMatrix.from_face_graph(ctx, g)  # the default compact records
    assert compact.stats()["value_dictionary_size"] > 0
    st, msg = create(compact)
    assert st == E_UNSUPPORTED and "compact" in msg
    loc, send_idx = mesh.periodic_z_local_graph(8, 8, 8)
    halo = _matrix(api, ctx, api.StencilMatrix.from_face_graph, loc)
    st, msg = create(halo)
    assert st == E_UNSUPPORTED and "single-rank" in msg
    plain = _matrix(api, ctx, api.StencilMatrix.from_face_graph, g)
    st, msg = create(plain, smoother_degree=17)
    assert st == E_INVALID and "smoother_degree" in msg
    # a pure-Neumann operator of two cells: a singular coarsest level
    neumann = _matrix(api, ctx, api.StencilMatrix.from_face_weights, 2, 0, np.array([0]), np.array([1]), np.array([1.0]),
                      np.array([1.0]), None)
    st, msg = create(neumann)
    assert st == E_INVALID and "singular" in msg
    # a two-stage operator has no single matrix to coarsen
    with pytest.raises(TypeError):
        api.AmgPreconditioner().build(api.DeviceVector(ctx, g.n_cells), None, api.HipTwoStageOperator(plain, -1.0, 1.0, -1.0, 1.0))
    pre = _build(env, plain, -1.0, 0.0)
    n = g.n_cells
    r, z, short = api.DeviceVector(ctx, n), api.DeviceVector(ctx, n), api.DeviceVector(ctx, n - 1)
    assert lib.storm_hip_amg_apply(pre._h, r._h, r._h) == E_INVALID and b"alias" in lib.storm_hip_last_error()
    assert lib.storm_hip_amg_apply(pre._h, short._h, z._h) == E_INVALID
    assert lib.storm_hip_amg_apply(pre._h, r._h, short._h) == E_INVALID
    assert lib.storm_hip_amg_restrict(pre._h, 0, r._h, z._h) == E_INVALID  # one level: no transfer
    v = C.c_double()
    assert lib.storm_hip_amg_get(pre._h, b"nonsense", C.byref(v)) == E_INVALID
    for key in ("levels", "operator_complexity", "grid_complexity", "setup_seconds", "device_bytes", "transfer_padding"):
        assert pre.get(key) >= 0
    # bound to an engine whose vectors have another size: refused by the solve
    g2 = mesh.structured_box(5)
    mat2 = api.StencilMatrix.from_face_graph(ctx, g2)
    eng = api.Krylov(ctx, 0)
    eng.set_operator(api.HipStencilOperator(mat2, -1.0, 0.0))
    assert lib.storm_hip_krylov_set_preconditioner_amg(eng._h, pre._h, 1) == 0
    b2, x2 = api.DeviceVector.from_numpy(ctx, np.ones(g2.n_cells)), api.DeviceVector(ctx, g2.n_cells)
    p, res = _lib.SolverParams(), _lib.SolverResult()
    lib.storm_hip_solver_params_default(C.byref(p))
    assert lib.storm_hip_krylov_solve(eng._h, b2._h, x2._h, C.byref(p), C.byref(res), None, None) == E_INVALID
    assert b"multigrid" in lib.storm_hip_last_error()
    assert lib.storm_hip_krylov_set_preconditioner_amg(eng._h, pre._h, 7) == E_INVALID  # no such side
    assert lib.storm_hip_krylov_set_preconditioner_amg(eng._h, None, 1) == 0
    pre.close()
    for m in (compact, halo, plain, neumann, mat2):
        m.close()


def test_cpp_driver(env):
    api, mesh, oracle, ctx = env
    exe = os.path.join(ROOT, "tests", "cpp", "amg_driver")
    if not os.path.exists(exe):  # (git-ignored: a checkout that arrived without it)
        import __graft_entry__ as ge

        ge.build()
    n = 13
    out = subprocess.run([exe, str(n), "cg", "2", "0", "right", "32"], check=True, capture_output=True, text=True, timeout=300).stdout
    got = json.loads(out.strip().splitlines()[-1])
    g = mesh.structured_box(n)
    mat = _matrix(api, ctx, api.StencilMatrix.from_face_graph, g)
    pre = api.AmgPreconditioner(coarse_rows=32)
    ok, it, x = _solve(api, ctx, api.CgSolver(), mat, -1.0, 0.0, np.ones(g.n_cells), pre)
    print(got, "python:", it, pre.hierarchy.level_rows())
    assert got["converged"] and ok and got["iterations"] == it
    assert got["level_rows"] == pre.hierarchy.level_rows()
    # (the host enqueues ahead of the device's verdict: applies issued past convergence are predicated off, and counted)
    assert got["amg_applies"] >= got["pre_applies"] > 0
    assert got["amg_fused_residuals"] == 2 * (len(got["level_rows"]) - 1) * got["amg_applies"]
    assert got["amg_statement_residuals"] == 0
    assert abs(got["x_norm2"] - np.linalg.norm(x)) <= 1e-9 * np.linalg.norm(x)
    pre.close()
    mat.close()
