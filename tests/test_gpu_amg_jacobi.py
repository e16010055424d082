"""The multigrid preconditioner's damped-Jacobi smoother (storm_hip_amg_create_smoother, csrc/amg.hip) on the device:

1. the fused sweep kernel gives the statements' bits: the whole cycle with amg_fused 1 against 0 for 1, 2 and 3 sweeps (both
   buffer parities), counters saying which path ran: 13^3 convection-diffusion box (ragged last slice, three levels),
   20x18x16 box (a coarsest level of 6 rows), the random non-symmetric CSR with ell_cap set so that level 1 has a CSR tail
   and falls to the statements by itself, 52^3 box (the XCD runs are active; bits only);
2. storm_hip_amg_smooth on level 0 is exact on integer-valued data (sigma = 1, s = 1 / 8);
3. the cycle against the numpy restatement (tests/amg_jacobi_ref.py) on the exported hierarchy;
4. symmetry of B on a symmetric operator;
5. solves on the convection-diffusion boxes: GMRES(30) right and left, FGMRES, BiCGStab;
6. reduced records: a sweep of a reduced object is the statement sequence on the operator rebuilt from the rounded weights;
7. refusals and the C++ driver.

Calibration of 3 and 4 (margin = 10 x the difference between the restatement in float64 and in np.longdouble on the same
input; the tests print the figures they measure beside it).  First run on an MI355X:
  cycle, max |device - restatement| / margin, 1 and 2 sweeps:  13^3 5.6e-17 / 4.2e-16 and 5.6e-17 / 2.8e-16;
                                   20x18x16 4.2e-17 / 2.8e-16 and 4.2e-17 / 1.4e-16;  random CSR 2.2e-16 / 1.1e-15 and 2.2e-16 / 2.2e-15
  symmetry, |<u,Bv> - <v,Bu>| / margin:  13^3 Poisson box 1.3e-15 / 7.7e-13
  two sweeps, iterations (plain): GMRES(30) right 10 (48) and 12 (66), equal to the restatement's; left 9 and 10; FGMRES 10 and
  12; BiCGStab 6 (27) and 6 (36); the solver's residual within 7e-15 of the recomputed one."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import amg_cases  # noqa: E402
import amg_jacobi_ref  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_UNSUPPORTED = -1, -6
SWEEP_KEYS = ("amg_applies", "amg_fused_sweeps", "amg_statement_sweeps", "amg_fused_residuals", "amg_statement_residuals")


@pytest.fixture(scope="module")
def env():
    from oracle import oracle
    from stormruler_amd import api, mesh

    ctx = api.Context(0)
    yield api, mesh, oracle, ctx
    ctx.close()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def _matrix(api, ctx, build, *args, ell_cap=0):
    """A StencilMatrix on fp64 records (spmv_dict = 0), options restored afterwards."""
    ctx.set_option("spmv_dict", 0)
    ctx.set_option("ell_cap", ell_cap)
    try:
        return build(ctx, *args)
    finally:
        ctx.set_option("spmv_dict", 4)
        ctx.set_option("ell_cap", 0)


CD_SHAPES = {"cd13": (13,), "cd20": (20, 18, 16), "cd52": (52,)}


def _operator(env, name):
    """(matrix, alpha, beta, assembled A, multigrid parameters) of a named case."""
    api, mesh, oracle, ctx = env
    if name in CD_SHAPES:
        g, (wi, wo, de), a = amg_jacobi_ref.convdiff_box(mesh, *CD_SHAPES[name])
        mat = _matrix(api, ctx, api.StencilMatrix.from_face_weights, g.n_cells, 0, g.inner, g.outer, wi, wo, de)
        return mat, 1.0, 0.0, a, dict(coarse_rows=512 if name == "cd52" else 32)
    if name == "box13":
        a = amg_cases.poisson_box(13)
        return _matrix(api, ctx, api.StencilMatrix.from_csr, a), 1.0, 0.0, a, dict(coarse_rows=32)
    assert name == "random"
    a = amg_jacobi_ref.random_nonsymmetric()
    return _matrix(api, ctx, api.StencilMatrix.from_csr, a), 1.0, 0.0, a, dict(coarse_rows=32)


def _build(env, mat, alpha, beta, ell_cap=0, **params):
    api, mesh, oracle, ctx = env
    params.setdefault("smoother", "jacobi")
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
    return amg_jacobi_ref.JacobiCycle(ops, ps, h.coarse_inverse(), sweeps=int(pre.get("jacobi_sweeps")),
                                      omega=pre.get("jacobi_omega"), dtype=dtype)


# ---- 1. the same bits on both paths -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("sweeps", [1, 2, 3])
@pytest.mark.parametrize("name", ["cd13", "cd20", "random_tail", "cd52"])
def test_fused_sweep_gives_the_statements_bits(env, name, sweeps):
    api, mesh, oracle, ctx = env
    tail = name == "random_tail"
    mat, alpha, beta, a, params = _operator(env, "random" if tail else name)
    pre = _build(env, mat, alpha, beta, ell_cap=8 if tail else 0, jacobi_sweeps=sweeps, **params)
    assert pre.get("smoother_kind") == 1 and pre.get("jacobi_sweeps") == sweeps and pre.get("jacobi_omega") == 2.0 / 3.0
    levels = int(pre.get("levels"))
    rows = pre.hierarchy.level_rows()
    st = mat.stats()
    assert st["value_dictionary_size"] == 0 and st["paired_rows"] == 0 and st["tail_rows"] == 0
    if name == "cd13":
        assert rows == [2197, 280, 24] and rows[0] % 64 != 0
    if name == "cd20":
        assert rows == [5760, 752, 52, 6]
    if name == "cd52":
        assert st["spmv_blocks"] > 8 * 64 and st["xcd_run_blocks"] == 64
    n = rows[0]
    r_host = np.sin(0.37 * np.arange(n)) + 0.25
    r, z = api.DeviceVector.from_numpy(ctx, r_host), api.DeviceVector(ctx, n)
    out, counts = [], []
    try:
        for amg_fused in (1, 0):
            ctx.set_option("amg_fused", amg_fused)
            z.upload(np.full(n, np.nan))  # (the cycle must not read z)
            before = [ctx.counter(k) for k in SWEEP_KEYS]
            pre.mul(z, r)
            out.append(z.to_numpy())
            counts.append(tuple(ctx.counter(k) - b for k, b in zip(SWEEP_KEYS, before)))
            assert np.array_equal(r.to_numpy(), r_host)  # r is not written
    finally:
        ctx.set_option("amg_fused", 1)
    smoothing = levels - 1
    per = 2 * sweeps - 1  # sweeps of a level past the one from the zero guess
    print(name, "sweeps", sweeps, "levels", rows, "counters", counts)
    if tail:  # level 1 (68 rows, rows wider than the cap) has a CSR tail: statements by itself
        assert rows == [918, 68, 1]
        assert counts[0] == (1, per, per, 1, 1)
    else:
        assert counts[0] == (1, per * smoothing, 0, smoothing, 0)
    assert counts[1] == (1, 0, per * smoothing, 0, smoothing)
    assert np.isfinite(out[0]).all() and np.abs(out[0]).max() > 0
    assert same_bits(out[0], out[1]), int(np.sum(bits(out[0]) != bits(out[1])))
    pre.close()
    mat.close()


# ---- 2. a sweep on integers -------------------------------------------------------------------------------------------------
def test_a_sweep_is_exact_on_integers(env):
    api, mesh, oracle, ctx = env
    import scipy.sparse as sp

    a = amg_cases.poisson_box(13)
    mat = _matrix(api, ctx, api.StencilMatrix.from_csr, a)
    pre = _build(env, mat, 1.0, 2.0, jacobi_omega=0.875, coarse_rows=32)  # diagonal 8: s = 1 / 8, lmax = 14 / 8
    assert pre.get("jacobi_sigma_0") == 1.0
    n = a.shape[0]
    full = (a + 2.0 * sp.identity(n)).tocsr()
    assert (full.diagonal() == 8.0).all()
    rng = np.random.default_rng(5)
    r_host = 8.0 * rng.integers(-1000, 1000, n)
    z_host = 8.0 * rng.integers(-1000, 1000, n)
    want = z_host + (r_host - full @ z_host) / 8.0  # every intermediate an integer far below 2^53
    assert np.array_equal(want, np.round(want)) and np.abs(full @ z_host).max() < 2.0 ** 40
    r, z_in, z_out = (api.DeviceVector.from_numpy(ctx, r_host), api.DeviceVector.from_numpy(ctx, z_host), api.DeviceVector(ctx, n))
    try:
        for amg_fused, key in ((1, "amg_fused_sweeps"), (0, "amg_statement_sweeps")):
            ctx.set_option("amg_fused", amg_fused)
            z_out.upload(np.full(n, np.nan))
            before = ctx.counter(key)
            pre.smooth(0, r, z_in, z_out)
            assert ctx.counter(key) == before + 1
            assert same_bits(z_out.to_numpy(), want)
            assert np.array_equal(r.to_numpy(), r_host) and np.array_equal(z_in.to_numpy(), z_host)
    finally:
        ctx.set_option("amg_fused", 1)
    pre.close()
    mat.close()


# ---- 3. / 4. the cycle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sweeps", [1, 2])
@pytest.mark.parametrize("name", ["cd13", "cd20", "random"])
def test_cycle_against_the_restatement(env, name, sweeps):
    api, mesh, oracle, ctx = env
    mat, alpha, beta, a, params = _operator(env, name)
    pre = _build(env, mat, alpha, beta, jacobi_sweeps=sweeps, **params)
    c64, cld = _restatement(pre), _restatement(pre, np.longdouble)
    n = a.shape[0]
    a0 = pre.hierarchy.operator(0)
    slack = (np.diff(a.indptr).max() + 2) * np.finfo(float).eps * np.asarray(abs(a).sum(axis=1)).ravel().max()
    assert abs(a0 - a).max() <= slack
    for lv in range(pre.hierarchy.levels - 1):  # sigma_l: 2 omega / lmax, lmax to a few ulps of the restatement's
        assert abs(pre.get(f"jacobi_sigma_{lv}") - c64.sigma[lv]) <= 8 * np.finfo(float).eps * c64.sigma[lv]
    r_host = np.random.default_rng(4).standard_normal(n)
    r, z = api.DeviceVector.from_numpy(ctx, r_host), api.DeviceVector(ctx, n)
    pre.mul(z, r)
    z_dev, z64, zld = z.to_numpy(), c64(r_host), cld(r_host)
    margin = 10.0 * float(np.abs(z64 - zld.astype(np.float64)).max())
    diff = float(np.abs(z_dev - z64).max())
    print(f"{name} sweeps {sweeps}: |device - restatement| = {diff:.3e}, margin {margin:.3e}, |z| = {np.abs(z64).max():.3e}")
    assert margin > 0 and diff <= margin
    pre.close()
    mat.close()


def test_cycle_is_symmetric_on_a_symmetric_operator(env):
    api, mesh, oracle, ctx = env
    mat, alpha, beta, a, params = _operator(env, "box13")
    pre = _build(env, mat, alpha, beta, **params)
    c64, cld = _restatement(pre), _restatement(pre, np.longdouble)
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
    print(f"box13: |<u,Bv> - <v,Bu>| = {asym:.3e}, margin {margin:.3e}, <u,Bu> = {u_host @ bu:.3e}")
    assert asym <= margin
    assert u_host @ bu > 0 and v_host @ bv > 0
    pre.close()
    mat.close()


# ---- 5. solves --------------------------------------------------------------------------------------------------------------
def _solver(api, kind):
    s = {"gmres": api.GmresSolver, "fgmres": api.FgmresSolver, "bicgstab": api.BiCgStabSolver}[kind]()
    if kind != "bicgstab":
        s.num_inner_iterations = 30
    return s


@pytest.fixture(scope="module")
def solve_cases(env):
    """Per box: matrix, operator, b, the plain counts per method, ONE Jacobi object (two sweeps) and its restatement's
    right-preconditioned GMRES(30) count."""
    api, mesh, oracle, ctx = env
    out = {}
    for name in ("cd13", "cd20"):
        mat, alpha, beta, a, params = _operator(env, name)
        n = a.shape[0]
        op = api.HipStencilOperator(mat, alpha, beta)
        b = api.DeviceVector.from_numpy(ctx, np.ones(n))
        plain = {}
        for kind in ("gmres", "fgmres", "bicgstab"):
            s, x = _solver(api, kind), api.DeviceVector(ctx, n)
            assert s.solve(x, b, op)
            plain[kind] = s.iteration
        pre = _build(env, mat, alpha, beta, jacobi_sweeps=2, **params)
        ref, _ = oracle.solve_gmres_pre(oracle.CsrOperator(a), oracle.CallbackOperator(n, _restatement(pre)), np.ones(n),
                                        side="right", num_inner_iterations=30)
        assert ref.converged
        out[name] = (mat, op, b, a, plain, pre, ref.iterations)
    yield out
    for mat, op, b, a, plain, pre, _ in out.values():
        pre.close()
        mat.close()


@pytest.mark.parametrize("kind,side", [("gmres", "right"), ("gmres", "left"), ("fgmres", "right"), ("bicgstab", "right")])
@pytest.mark.parametrize("name", ["cd13", "cd20"])
def test_solves_converge_below_the_plain_count(env, solve_cases, name, kind, side):
    api, mesh, oracle, ctx = env
    mat, op, b, a, plain, pre, ref_it = solve_cases[name]
    n = a.shape[0]
    s, x = _solver(api, kind), api.DeviceVector(ctx, n)
    s.pre_op = pre
    s.pre_side = api.PreconditionerSide.Left if side == "left" else api.PreconditionerSide.Right
    before = ctx.counter("amg_applies")
    ok = s.solve(x, b, op)
    assert ok and s.relative_error < 1e-6 and ctx.counter("amg_applies") - before >= s.iteration > 0
    # the true residual of the returned x in the norm the solver reports: ||b - A x||, left: ||B (b - A x)||
    res = api.DeviceVector.from_numpy(ctx, np.ones(n) - a @ x.to_numpy())
    if side == "left":
        pres = api.DeviceVector(ctx, n)
        pre.mul(pres, res)
        true_res = np.linalg.norm(pres.to_numpy())
    else:
        true_res = op.ResidualNorm(b, x)
    print(f"{name} {kind} {side}: {s.iteration} iterations (plain {plain[kind]}, restatement's right GMRES {ref_it}); "
          f"|true residual - solver's| = {abs(true_res - s.absolute_error):.3e}, initial {s.initial_error:.3e}")
    assert abs(true_res - s.absolute_error) <= 1e-6 * s.initial_error
    assert s.iteration < plain[kind]
    if (kind, side) == ("gmres", "right"):
        assert abs(s.iteration - ref_it) <= max(2, int(0.05 * ref_it))
        assert ref_it <= 30


# ---- 6. reduced records -----------------------------------------------------------------------------------------------------
def f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def _dyadic_nonsymmetric():
    """The random non-symmetric CSR with entries on a grid fine enough that (almost) none is its own fp32 rounding and coarse
    enough that every sum the packer forms is exact: off-diagonals k / 2^30 in +-[1/4, 1), the diagonal a multiple of 2^-30
    in [16, 32).  Returns (A, A~): A~ is A rebuilt from double(float(w)) and double(float(ext)), ext the row sum."""
    import scipy.sparse as sp

    rng = np.random.default_rng(103)
    n, nnz_row = 918, 5
    rows = np.repeat(np.arange(n), nnz_row)
    cols = (rows + 1 + np.tile(np.arange(nnz_row), n) * 37 + rng.integers(0, 30, size=rows.size)) % n  # (no duplicates in a row)
    vals = rng.choice([-1.0, 1.0], rows.size) * rng.integers(2 ** 28, 2 ** 30, rows.size) / 2.0 ** 30
    off = sp.coo_matrix((vals, (rows, cols)), shape=(n, n)).tocsr()
    assert off.nnz == rows.size and (off.diagonal() == 0).all()
    diag = rng.integers(2 ** 34, 2 ** 35, n) / 2.0 ** 30
    a = (off + sp.diags(diag)).tocsr()
    ext = diag + np.asarray(off.sum(axis=1)).ravel()  # exact: multiples of 2^-30 below 2^6
    off32 = sp.csr_matrix((f32(off.data), off.indices.copy(), off.indptr.copy()), shape=off.shape)
    diag32 = f32(ext) - np.asarray(off32.sum(axis=1)).ravel()  # exact again: multiples of 2^-26 below 2^6
    return a, (off32 + sp.diags(diag32)).tocsr()


def test_reduced_sweep_is_the_statement_sequence_on_the_rounded_operator(env):
    """tests/test_gpu_reduced.py's notion of exact, with ONE scale and ONE sigma for both sides as there: a sweep of the
    reduced object (fused kernel on Rec32, and the statements with storm_hip_op_apply_reduced) gives the bits of
    storm_hip_op_apply on a fresh fp64-record operator built from the rounded weights followed by the three vector
    statements.  (An ordinary Jacobi object on the rebuilt operator would divide by ITS diagonal: another scale, another
    hierarchy.)  The whole cycle of the reduced object, every level on its companion, is compared fused against statements."""
    api, mesh, oracle, ctx = env
    from stormruler_amd._lib import lib

    a, a32 = _dyadic_nonsymmetric()
    assert np.mean(a.data != f32(a.data)) >= 0.95
    mat, ref = _matrix(api, ctx, api.StencilMatrix.from_csr, a), _matrix(api, ctx, api.StencilMatrix.from_csr, a32)
    assert mat.stats()["tail_rows"] == 0 and mat.stats()["value_dictionary_size"] == 0
    pre = _build(env, mat, 1.0, 0.0, reduced_records=True, coarse_rows=32)
    assert pre.get("reduced") == 1 and mat.reduced_bytes > 0 and int(pre.get("levels")) >= 2
    n = a.shape[0]
    sigma = pre.get("jacobi_sigma_0")
    s = api.DeviceVector(ctx, n)
    mat.diagonal(1.0, 0.0, s, invert=True)
    r_host, z_host = np.cos(0.11 * np.arange(n)) + 0.5, np.sin(0.37 * np.arange(n))
    r, z_in = api.DeviceVector.from_numpy(ctx, r_host), api.DeviceVector.from_numpy(ctx, z_host)
    t, want, got = api.DeviceVector(ctx, n), api.DeviceVector(ctx, n), api.DeviceVector(ctx, n)
    ref.apply(1.0, 0.0, z_in, t)
    assert lib.storm_hip_axpbz(t._h, 1.0, r._h, -1.0, t._h) == 0
    assert lib.storm_hip_vmul(t._h, s._h, t._h) == 0
    assert lib.storm_hip_axpbz(want._h, sigma, t._h, 1.0, z_in._h) == 0
    want_host = want.to_numpy()
    mat.apply(1.0, 0.0, z_in, t)  # (the fp64 records of A itself give something else)
    own = z_host + sigma * (s.to_numpy() * (r_host - t.to_numpy()))
    assert np.mean(bits(own) != bits(want_host)) >= 0.5
    cycle = []
    rr, zz = api.DeviceVector.from_numpy(ctx, r_host), api.DeviceVector(ctx, n)
    try:
        for amg_fused, key in ((1, "amg_fused_sweeps"), (0, "amg_statement_sweeps")):
            ctx.set_option("amg_fused", amg_fused)
            got.upload(np.full(n, np.nan))
            before = ctx.counter(key)
            pre.smooth(0, r, z_in, got)
            assert ctx.counter(key) == before + 1
            assert same_bits(got.to_numpy(), want_host), (amg_fused, int(np.sum(bits(got.to_numpy()) != bits(want_host))))
            zz.upload(np.full(n, np.nan))
            pre.mul(zz, rr)
            cycle.append(zz.to_numpy())
    finally:
        ctx.set_option("amg_fused", 1)
    assert np.isfinite(cycle[0]).all() and same_bits(cycle[0], cycle[1])
    pre.close()
    mat.close(), ref.close()


# ---- 7. refusals and the C++ driver -----------------------------------------------------------------------------------------
def test_refusals(env):
    api, mesh, oracle, ctx = env
    from stormruler_amd import _lib
    from stormruler_amd._lib import lib

    mat, alpha, beta, a, params = _operator(env, "cd13")
    n = a.shape[0]
    pre = _build(env, mat, alpha, beta, **params)
    cheb = _build(env, mat, alpha, beta, smoother="chebyshev", **params)
    r, z, z2, short = (api.DeviceVector(ctx, n), api.DeviceVector(ctx, n), api.DeviceVector(ctx, n), api.DeviceVector(ctx, n - 1))
    # a Jacobi object is a plain object: no refresh, no projection
    assert lib.storm_hip_amg_refresh(pre._h) == E_UNSUPPORTED
    assert lib.storm_hip_amg_project(pre._h, z._h) == E_UNSUPPORTED
    with pytest.raises(ValueError):
        api.AmgPreconditioner(smoother="jacobi", refreshable=True)
    with pytest.raises(ValueError):
        api.AmgPreconditioner(smoother="jacobi", nullspace="constant")
    late = api.AmgPreconditioner(smoother="jacobi", **params)
    late.refreshable = True
    with pytest.raises(ValueError):
        late.build(r, r, api.HipStencilOperator(mat, alpha, beta))
    # one sweep on its own
    assert lib.storm_hip_amg_smooth(cheb._h, 0, r._h, z._h, z2._h) == E_UNSUPPORTED
    assert b"Chebyshev" in lib.storm_hip_last_error()
    assert lib.storm_hip_amg_smooth(pre._h, 0, r._h, z._h, z._h) == E_INVALID and b"alias" in lib.storm_hip_last_error()
    assert lib.storm_hip_amg_smooth(pre._h, 0, r._h, z._h, r._h) == E_INVALID and b"alias" in lib.storm_hip_last_error()
    assert lib.storm_hip_amg_smooth(pre._h, 0, r._h, short._h, z._h) == E_INVALID
    levels = int(pre.get("levels"))
    assert lib.storm_hip_amg_smooth(pre._h, levels - 1, r._h, z._h, z2._h) == E_INVALID  # the coarsest level has no smoother
    assert lib.storm_hip_amg_smooth(pre._h, -1, r._h, z._h, z2._h) == E_INVALID
    v = C.c_double()
    assert lib.storm_hip_amg_get(pre._h, f"jacobi_sigma_{levels - 1}".encode(), C.byref(v)) == E_INVALID
    assert lib.storm_hip_amg_get(pre._h, b"jacobi_sigma_x", C.byref(v)) == E_INVALID
    assert lib.storm_hip_amg_get(cheb._h, b"jacobi_sigma_0", C.byref(v)) == E_INVALID
    assert cheb.get("smoother_kind") == 0 and pre.get("smoother_kind") == 1
    assert pre.get("device_bytes") < cheb.get("device_bytes")  # no Chebyshev object: three vectors fewer per level
    # kind 0 is storm_hip_amg_create's object: the same bits
    h0 = C.c_void_p()
    p = api._amg_params(**params)
    sm = _lib.AmgSmoother(0, 99, -1.0)  # (sweeps and omega are not looked at)
    assert lib.storm_hip_amg_create_smoother(mat._h, alpha, beta, C.byref(p), C.byref(sm), C.byref(h0)) == 0
    r.upload(np.sin(0.37 * np.arange(n)) + 0.25)
    cheb.mul(z, r)
    assert lib.storm_hip_amg_apply(h0, r._h, z2._h) == 0
    assert same_bits(z.to_numpy(), z2.to_numpy())
    lib.storm_hip_amg_destroy(h0)
    # a zero diagonal: beta = -alpha a_00 on the Poisson box puts 0 on every diagonal
    box = _matrix(api, ctx, api.StencilMatrix.from_csr, amg_cases.poisson_box(5))
    sm = _lib.AmgSmoother(1, 2, 2.0 / 3.0)
    assert lib.storm_hip_amg_create_smoother(box._h, 1.0, -6.0, None, C.byref(sm), C.byref(h0)) == E_INVALID and not h0.value
    msg = lib.storm_hip_last_error().decode()
    assert "level 0" in msg and "row 0" in msg and "diagonal" in msg
    # the refusals of storm_hip_amg_create apply
    compact = api.StencilMatrix.from_face_graph(ctx, mesh.structured_box(6))
    assert lib.storm_hip_amg_create_smoother(compact._h, -1.0, 0.0, None, C.byref(sm), C.byref(h0)) == E_UNSUPPORTED
    for obj in (pre, cheb, late):
        obj.close()
    for m in (mat, box, compact):
        m.close()


def test_hierarchy_is_kept_across_solves_and_rebuilt_for_other_knobs(env):
    api, mesh, oracle, ctx = env
    mat, alpha, beta, a, params = _operator(env, "cd13")
    n = a.shape[0]
    op = api.HipStencilOperator(mat, alpha, beta)
    b = api.DeviceVector.from_numpy(ctx, np.ones(n))
    pre = api.AmgPreconditioner(smoother="jacobi", **params)
    its = []
    for sweeps in (2, 2, 1):
        pre.jacobi_sweeps = sweeps
        s, x = _solver(api, "gmres"), api.DeviceVector(ctx, n)
        s.pre_op = pre
        assert s.solve(x, b, op)
        its.append((s.iteration, pre._h.value, pre.get("jacobi_sweeps")))
    assert its[0][:2] == its[1][:2] and its[2][2] == 1 and its[2][0] > its[1][0]
    pre.close()
    mat.close()


def test_cpp_driver(env):
    api, mesh, oracle, ctx = env
    exe = os.path.join(ROOT, "tests", "cpp", "amg_jacobi_driver")
    if not os.path.exists(exe):  # (git-ignored: a checkout that arrived without it)
        import __graft_entry__ as ge

        ge.build()
    out = subprocess.run([exe, "13", "gmres", "2", "right", "32"], check=True, capture_output=True, text=True, timeout=300).stdout
    got = json.loads(out.strip().splitlines()[-1])
    mat, alpha, beta, a, params = _operator(env, "cd13")
    n = a.shape[0]
    pre = api.AmgPreconditioner(smoother="jacobi", **params)
    s, x = _solver(api, "gmres"), api.DeviceVector(ctx, n)
    s.pre_op = pre
    ok = s.solve(x, api.DeviceVector.from_numpy(ctx, np.ones(n)), api.HipStencilOperator(mat, alpha, beta))
    print(got, "python:", s.iteration, pre.hierarchy.level_rows())
    assert got["converged"] and got["plain_converged"] and ok
    assert abs(got["iterations"] - s.iteration) <= 1 and got["iterations"] < got["plain_iterations"]
    # (the driver forms its weights in C++: the last level's size may differ from numpy's weights' by a tie in the aggregation)
    assert got["level_rows"][:2] == pre.hierarchy.level_rows()[:2] and len(got["level_rows"]) == int(pre.get("levels"))
    assert (got["smoother_kind"], got["jacobi_sweeps"], got["jacobi_omega"]) == (1, 2, 2.0 / 3.0)
    assert abs(got["jacobi_sigma_0"] - pre.get("jacobi_sigma_0")) <= 1e-12 * pre.get("jacobi_sigma_0")
    assert got["amg_applies"] >= got["pre_applies"] > 0
    assert got["amg_fused_sweeps"] == 3 * (len(got["level_rows"]) - 1) * got["amg_applies"] and got["amg_statement_sweeps"] == 0
    assert abs(got["x_norm2"] - np.linalg.norm(x.to_numpy())) <= 1e-6 * np.linalg.norm(x.to_numpy())
    pre.close()
    mat.close()
