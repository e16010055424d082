"""The Chebyshev polynomial preconditioner (storm_hip_cheb_*, csrc/precond_cheb.hip) on the device:

1. the fused step kernel gives the statement path's bits (13^3 box: ragged last slice, slice count not a multiple of 4; a
   random symmetric CSR operator: slices of mixed width, rows wider than 8; 52^3 box: more than 8 x 64 blocks, so the XCD
   runs are active with a ragged tail), and operators it does not take fall to the statements by themselves;
2. the device z against the closed form of the residual polynomial from an eigendecomposition (tests/cheb_ref.py);
3. Gershgorin's bound against the assembled matrix, and above the largest eigenvalue;
4. preconditioned solves against the oracle with the numpy recurrence as its preconditioner callback;
5. refusals;  6. the C++ driver.
A preconditioner object whose operator was destroyed is the caller's error (storm_hip.h) and is not tested."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cheb_ref  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NU, VEL = 1e-2, (1.0, 0.5, 0.25)
E_INVALID, E_UNSUPPORTED = -1, -6


@pytest.fixture(scope="module")
def env():
    from oracle import oracle
    from stormruler_amd import api, mesh

    ctx = api.Context(0)
    yield api, mesh, oracle, ctx
    ctx.close()


def _graded_box(mesh, n):  # test_gpu_precond.py's: cell volumes vary, so the diagonal does
    g = mesh.structured_box(n)
    rng = np.random.default_rng(7)
    g.volume = g.volume * (0.25 + 1.5 * rng.random(g.n_total))
    return g


def _matrix(api, ctx, build, *args, spmv_dict=None, ell_cap=None):
    """A StencilMatrix built under the given options (restored afterwards: spmv_dict 4, ell_cap 0 are the defaults)."""
    if spmv_dict is not None:
        ctx.set_option("spmv_dict", spmv_dict)
    if ell_cap is not None:
        ctx.set_option("ell_cap", ell_cap)
    try:
        return build(ctx, *args)
    finally:
        ctx.set_option("spmv_dict", 4)
        ctx.set_option("ell_cap", 0)


def _random_symmetric(seed=3):
    import scipy.sparse as sp

    rng = np.random.default_rng(100 + seed)
    n = int(rng.integers(200, 1500))
    nnz_row = int(rng.integers(2, 9))
    rows = np.repeat(np.arange(n), nnz_row)
    cols = (rows + rng.integers(1, n, size=rows.size)) % n
    off = sp.coo_matrix((rng.uniform(-1.0, 1.0, rows.size), (rows, cols)), shape=(n, n)).tocsr()
    off.sum_duplicates()
    sym_off = (off + off.T) * 0.5
    return (sym_off + sp.diags(np.abs(sym_off).sum(axis=1).A1 * 1.5 + 1.0)).tocsr()


class _Cheb:
    """storm_hip_cheb_* through ctypes, for the cases the Python class does not reach (explicit scale, bounds, refusals)."""

    def __init__(self, lib, mat, alpha, beta, dinv, degree, lmin=0.0, lmax=0.0):
        self.lib, self.h = lib, C.c_void_p()
        self.status = lib.storm_hip_cheb_create(mat._h, alpha, beta, None if dinv is None else dinv._h, degree, lmin, lmax,
                                                C.byref(self.h))

    def apply(self, r, z):
        return self.lib.storm_hip_cheb_apply(self.h, r._h, z._h)

    def get(self, key):
        v = C.c_double()
        assert self.lib.storm_hip_cheb_get(self.h, key.encode(), C.byref(v)) == 0
        return v.value

    def close(self):
        if self.h:
            self.lib.storm_hip_cheb_destroy(self.h)
            self.h = C.c_void_p()


def _both_paths(api, ctx, mat, alpha, beta, jacobi, degree, r_host):
    """z by option cheb_fused = 1 and = 0, and the counters' increments (fused, statements) of the first apply."""
    from stormruler_amd._lib import lib

    n = r_host.size
    dinv = None
    if jacobi:
        dinv = api.DeviceVector(ctx, n)
        mat.diagonal(alpha, beta, dinv, invert=True)
    ch = _Cheb(lib, mat, alpha, beta, dinv, degree)
    assert ch.status == 0, lib.storm_hip_last_error()
    r, z = api.DeviceVector.from_numpy(ctx, r_host), api.DeviceVector(ctx, n)
    out, counts = [], []
    try:
        for fused in (1, 0):
            ctx.set_option("cheb_fused", fused)
            z.upload(np.full(n, np.nan))  # (the FIRST step must not read z)
            before = (ctx.counter("cheb_fused_applies"), ctx.counter("cheb_statement_applies"))
            assert ch.apply(r, z) == 0, lib.storm_hip_last_error()
            out.append(z.to_numpy())
            counts.append((ctx.counter("cheb_fused_applies") - before[0], ctx.counter("cheb_statement_applies") - before[1]))
            assert np.array_equal(r.to_numpy(), r_host)  # r is not written
    finally:
        ctx.set_option("cheb_fused", 1)
        ch.close()
    return out, counts


@pytest.fixture(scope="module")
def fused_operators(env):
    """fp64 records without a CSR tail (spmv_dict = 0): what the fused step takes."""
    api, mesh, oracle, ctx = env
    ops = {}
    for name, n in (("box13", 13), ("box52", 52)):
        g = mesh.structured_box(n)
        ops[name] = (_matrix(api, ctx, api.StencilMatrix.from_face_graph, g, spmv_dict=0), -1.0, 0.0, g.n_cells)
    a = _random_symmetric()
    ops["random_csr"] = (_matrix(api, ctx, api.StencilMatrix.from_csr, a, spmv_dict=0), 1.0, 0.0, a.shape[0])
    yield ops
    for mat, *_ in ops.values():
        mat.close()


@pytest.mark.parametrize("jacobi", [False, True])
@pytest.mark.parametrize("degree", [1, 2, 3, 8])
@pytest.mark.parametrize("name", ["box13", "random_csr", "box52"])
def test_fused_step_gives_the_statement_path_s_bits(env, fused_operators, name, degree, jacobi):
    api, mesh, oracle, ctx = env
    mat, alpha, beta, n = fused_operators[name]
    st = mat.stats()
    assert st["value_dictionary_size"] == 0 and st["paired_rows"] == 0 and st["tail_rows"] == 0
    if name == "box13":
        assert n % 64 != 0 and st["n_slices"] % 4 != 0
    if name == "random_csr":
        assert st["max_row_len"] > 8
    if name == "box52":
        assert st["spmv_blocks"] > 8 * 64 and st["xcd_run_blocks"] == 64 and st["spmv_blocks"] % (8 * 64) != 0
    r_host = np.sin(0.37 * np.arange(n)) + 0.25
    (z_fused, z_stmt), counts = _both_paths(api, ctx, mat, alpha, beta, jacobi, degree, r_host)
    assert counts == [(1, 0), (0, 1)]
    assert np.isfinite(z_stmt).all() and np.abs(z_stmt).max() > 0
    assert np.array_equal(z_fused, z_stmt)


@pytest.mark.parametrize("build", ["compact", "tail"])
def test_operators_the_fused_step_does_not_take_fall_to_the_statements(env, build):
    api, mesh, oracle, ctx = env
    g = mesh.structured_box(13)
    ref_mat = _matrix(api, ctx, api.StencilMatrix.from_face_graph, g, spmv_dict=0)
    if build == "tail":
        mat = _matrix(api, ctx, api.StencilMatrix.from_face_graph, g, spmv_dict=0, ell_cap=3)
        assert mat.stats()["tail_rows"] > 0
    else:
        mat = api.StencilMatrix.from_face_graph(ctx, g)  # the default compact format
        assert mat.stats()["value_dictionary_size"] > 0
    r_host = np.sin(0.37 * np.arange(g.n_cells)) + 0.25
    for jacobi in (False, True):
        (z1, z0), counts = _both_paths(api, ctx, mat, -1.0, 0.0, jacobi, 3, r_host)
        assert counts == [(0, 1), (0, 1)]  # cheb_fused = 1 took the statement path by itself
        assert np.array_equal(z1, z0)
        if build == "compact":  # every record format gives the fp64 records' bits
            (zf, _), _ = _both_paths(api, ctx, ref_mat, -1.0, 0.0, jacobi, 3, r_host)
            assert np.array_equal(z1, zf)
    mat.close()
    ref_mat.close()


# ---- 2. the closed form -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha,beta", [(-1.0, 0.0), (-1e-2, 1.0)])
@pytest.mark.parametrize("jacobi", [False, True])
def test_device_z_matches_the_closed_form(env, alpha, beta, jacobi):
    """Rounding grows at most like degree x condition number x 2^-53 (below 1e-12 on the 8^3 box); 1e-10 covers the SpMV's
    difference form.  Both paths (they are the same bits; the fused one needs fp64 records)."""
    api, mesh, oracle, ctx = env
    from stormruler_amd._lib import lib

    g = mesh.structured_box(8)
    a = mesh.assemble_csr(g, alpha, beta).tocsr()
    n = g.n_cells
    s = 1 / a.diagonal() if jacobi else np.ones(n)
    lmax = cheb_ref.gershgorin(a, s)
    lmin = lmax / 30
    r_host = np.sin(0.37 * np.arange(n))
    mat = _matrix(api, ctx, api.StencilMatrix.from_face_graph, g, spmv_dict=0)
    dinv = api.DeviceVector.from_numpy(ctx, s) if jacobi else None
    r, z = api.DeviceVector.from_numpy(ctx, r_host), api.DeviceVector(ctx, n)
    for degree in (1, 3, 6):
        ref = cheb_ref.closed_form(a, s, r_host, lmin, lmax, degree)
        ch = _Cheb(lib, mat, alpha, beta, dinv, degree, lmin, lmax)
        assert ch.status == 0
        try:
            for fused in (1, 0):
                ctx.set_option("cheb_fused", fused)
                assert ch.apply(r, z) == 0
                rel = np.linalg.norm(z.to_numpy() - ref) / np.linalg.norm(ref)
                print(f"alpha {alpha} beta {beta} jacobi {jacobi} degree {degree} fused {fused}: rel {rel:.3e}")
                assert rel <= 1e-10
        finally:
            ctx.set_option("cheb_fused", 1)
            ch.close()
    mat.close()


# ---- 3. Gershgorin ------------------------------------------------------------------------------------------------------
def _gershgorin_cases(api, mesh, ctx):
    from stormruler_amd import io_tetgen

    box = mesh.structured_box(13)
    graded = _graded_box(mesh, 13)
    tri = io_tetgen.read_triangle(os.path.join(ROOT, "tests", "golden", "mesh", "square_nb.1."))
    fg = api.StencilMatrix.from_face_graph
    return [("box13_fp64", box, _matrix(api, ctx, fg, box, spmv_dict=0), True),
            ("graded13", graded, _matrix(api, ctx, fg, graded), False),
            ("square_nb", tri, _matrix(api, ctx, fg, tri), False),
            ("box13_compact", box, fg(ctx, box), True),
            ("box13_tail", box, _matrix(api, ctx, fg, box, spmv_dict=0, ell_cap=3), True)]


def test_gershgorin_bound(env):
    import scipy.sparse.linalg as spla

    api, mesh, oracle, ctx = env
    seen_formats = set()
    for name, g, mat, symmetric in _gershgorin_cases(api, mesh, ctx):
        st = mat.stats()
        seen_formats.add((st["value_dictionary_size"] > 0, st["paired_rows"], st["tail_rows"] > 0))
        for alpha, beta in ((-1.0, 0.0), (-0.7, 0.3)):
            a = mesh.assemble_csr(g, alpha, beta).tocsr()
            d = api.DeviceVector(ctx, g.n_cells)
            mat.diagonal(alpha, beta, d, invert=True)
            for scale, s in ((None, np.ones(g.n_cells)), (d, d.to_numpy())):
                want = cheb_ref.gershgorin(a, s)
                got = mat.gershgorin(alpha, beta, scale)
                print(f"{name} alpha {alpha} beta {beta} scaled {scale is not None}: {got!r} vs {want!r}")
                assert abs(got - want) <= 1e-13 * want
            if symmetric:
                # On the uniform box the bound is ATTAINED: the vector (-1)^(i+j+k) is an eigenvector with the eigenvalue
                # beta + 12 |alpha| / h^2 = the row sum of every row.  So `>=` is held up to the eigensolver's own
                # error: eigsh to machine precision (tol = 0) returns the eigenvalue to a few ulps of rounding in its
                # n-term products, 1e-12 relative at most (measured: bound 2028.0000000000014, eigsh 2028.0000000000036).
                top = spla.eigsh(a, k=1, which="LA", return_eigenvectors=False, tol=0)[0]
                got = mat.gershgorin(alpha, beta)
                print(f"{name} alpha {alpha} beta {beta}: bound {got!r}, largest eigenvalue {top!r}")
                assert got >= top * (1 - 1e-12)
        mat.close()
    assert (False, 0, True) in seen_formats and (False, 0, False) in seen_formats  # fp64 records with and without a tail
    assert any(f[0] for f in seen_formats)  # and a compact format


def test_cheb_get_reports_the_bounds_in_use(env):
    api, mesh, oracle, ctx = env
    from stormruler_amd._lib import lib

    g = mesh.structured_box(13)
    mat = api.StencilMatrix.from_face_graph(ctx, g)
    gersh = mat.gershgorin(-1.0, 0.0)
    for lmin, lmax, want in ((0.0, 0.0, (gersh / 30.0, gersh)), (0.0, 90.0, (3.0, 90.0)), (2.5, 0.0, (2.5, gersh)),
                             (-1.0, -1.0, (gersh / 30.0, gersh)), (1.25, 77.0, (1.25, 77.0))):
        ch = _Cheb(lib, mat, -1.0, 0.0, None, 5, lmin, lmax)
        assert ch.status == 0
        assert (ch.get("lambda_min"), ch.get("lambda_max"), ch.get("degree")) == (want[0], want[1], 5.0)
        ch.close()
    pre = api.ChebyshevPreconditioner(degree=2, jacobi=True)
    x = api.DeviceVector(ctx, g.n_cells)
    pre.build(x, x, api.HipStencilOperator(mat, -1.0, 0.0))
    d = api.DeviceVector(ctx, g.n_cells)
    mat.diagonal(-1.0, 0.0, d, invert=True)
    assert pre.get("lambda_max") == mat.gershgorin(-1.0, 0.0, d) and pre.get("lambda_min") == pre.get("lambda_max") / 30.0
    pre.close()
    mat.close()


# ---- 4. solves against the oracle ---------------------------------------------------------------------------------------
def _accept(api, s, x, ref, n_pre_ref, op, b, b_host, side, count_at=None):
    """The bars of test_every_solver_with_jacobi_matches_oracle, the preconditioner count, and the true residual.

    The preconditioner count must EQUAL the oracle's.  The iteration bar allows the device a few iterations more or fewer
    than the oracle (short recurrences amplify rounding: on the graded problem the oracle itself moves between 21 and 22
    BiCGStab iterations when the interval's upper end moves by one ulp), and a count is a function of the iterations
    run; so where the two stopped at different iterations the device's count is held to the oracle's count AT THE
    DEVICE'S NUMBER OF ITERATIONS (`count_at`: the same oracle solve with the tolerances off and that many iterations)."""
    assert ref.converged
    tol_it = max(2, int(0.1 * ref.iterations))
    assert abs(s.iteration - ref.iterations) <= tol_it, (s.iteration, ref.iterations)
    assert np.linalg.norm(x.to_numpy() - ref.x) <= 2e-5 * np.linalg.norm(ref.x)
    m = min(len(s.history), len(ref.history), 6)
    assert np.allclose(s.history[:m], ref.history[:m], rtol=1e-6)
    if s.iteration != ref.iterations and count_at is not None:
        n_pre_ref = count_at(s.iteration)
    print(f"iterations {s.iteration} (oracle {ref.iterations}), preconditioner applies {s.num_pre_applies} (oracle {n_pre_ref})")
    assert s.num_pre_applies == n_pre_ref, (s.num_pre_applies, n_pre_ref, s.iteration, ref.iterations)
    if side == "right":  # (right-preconditioned: the reported norm is the true residual's)
        r = api.DeviceVector(x.ctx, b_host.size)
        op.Residual(r, b, x)
        assert abs(api.norm_2(r) - s.absolute_error) <= 1e-6 * np.linalg.norm(b_host)


@pytest.fixture(scope="module")
def box16(env):
    api, mesh, oracle, ctx = env
    g = mesh.structured_box(16)
    a = mesh.assemble_csr(g, -1.0, 0.0).tocsr()
    ref_op = oracle.StencilOperator(g, -1.0, 0.0)
    plain = oracle.solve("cg", ref_op, np.ones(g.n_cells))
    return g, a, ref_op, plain


@pytest.mark.parametrize("side", ["left", "right"])
@pytest.mark.parametrize("jacobi", [False, True])
@pytest.mark.parametrize("degree", [2, 4])
def test_cg_with_chebyshev_matches_oracle(env, box16, degree, jacobi, side):
    api, mesh, oracle, ctx = env
    g, a, ref_op, plain = box16
    n = g.n_cells
    s_host = 1 / a.diagonal() if jacobi else np.ones(n)
    lmax = cheb_ref.gershgorin(a, s_host)
    b_host = np.ones(n)
    pre_ref = oracle.CallbackOperator(n, lambda v: cheb_ref.apply(a, s_host, v, lmax / 30, lmax, degree))
    ref = oracle.solve("cg", ref_op, b_host, pre=pre_ref, side=side)
    n_pre_ref = oracle.last_pre_applies()
    assert plain.converged and ref.converged and ref.iterations < plain.iterations, (ref.iterations, plain.iterations)

    def count_at(iterations):
        oracle.solve("cg", ref_op, b_host, pre=pre_ref, side=side, num_iterations=iterations, abs_tol=0.0, rel_tol=0.0)
        return oracle.last_pre_applies()

    mat = _matrix(api, ctx, api.StencilMatrix.from_face_graph, g, spmv_dict=0)  # fp64 records: the fused step runs
    op = api.HipStencilOperator(mat, -1.0, 0.0)
    b, x = api.DeviceVector.from_numpy(ctx, b_host), api.DeviceVector(ctx, n)
    s = api.CgSolver()
    s.pre_op = api.ChebyshevPreconditioner(degree=degree, jacobi=jacobi)
    s.pre_side = api.PreconditionerSide.Left if side == "left" else api.PreconditionerSide.Right
    s.record_history = True
    fused_before = ctx.counter("cheb_fused_applies")
    assert s.solve(x, b, op)
    assert ctx.counter("cheb_fused_applies") - fused_before >= s.num_pre_applies > 0
    assert abs(s.pre_op.get("lambda_max") - lmax) <= 1e-13 * lmax
    _accept(api, s, x, ref, n_pre_ref, op, b, b_host, side, count_at)
    s.pre_op.close()
    mat.close()


@pytest.mark.parametrize("side", ["left", "right"])
@pytest.mark.parametrize("kind", ["bicgstab", "gmres"])
def test_nonsymmetric_solvers_with_chebyshev_match_oracle(env, kind, side):
    """test_gpu_precond.py's graded convection-diffusion problem at n = 14, Jacobi scale, degree 3.  The oracle's callback
    takes the interval the device object reports (Gershgorin's bound is pinned in test_gershgorin_bound)."""
    api, mesh, oracle, ctx = env
    g = _graded_box(mesh, 14)
    n, degree = g.n_cells, 3
    wi, wo, de = mesh.convection_diffusion_weights(g, NU, VEL)
    mat = api.StencilMatrix.from_face_weights(ctx, n, g.n_halo, g.inner, g.outer, wi, wo, de)
    op = api.HipStencilOperator(mat, 1.0, 0.0)
    ref_op = oracle.StencilOperator(g, -NU, 0.0, conv=1.0, vel=VEL)
    b_host = np.ones(n)
    b, x = api.DeviceVector.from_numpy(ctx, b_host), api.DeviceVector(ctx, n)
    s = api.BiCgStabSolver() if kind == "bicgstab" else api.GmresSolver()
    if kind == "gmres":
        s.num_inner_iterations = 20
    s.pre_op = api.ChebyshevPreconditioner(degree=degree, jacobi=True)
    s.pre_side = api.PreconditionerSide.Left if side == "left" else api.PreconditionerSide.Right
    s.record_history = True
    assert s.solve(x, b, op)
    lmin, lmax = s.pre_op.get("lambda_min"), s.pre_op.get("lambda_max")
    assert lmin == lmax / 30.0
    d = api.DeviceVector(ctx, n)
    mat.diagonal(1.0, 0.0, d, invert=True)
    dinv = d.to_numpy()

    class _A:  # the oracle's operator as the numpy recurrence's matrix
        def __matmul__(self, v):
            return ref_op.apply(v)

    pre_ref = oracle.CallbackOperator(n, lambda v: cheb_ref.apply(_A(), dinv, v, lmin, lmax, degree))
    if kind == "gmres":
        ref, n_pre_ref = oracle.solve_gmres_pre(ref_op, pre_ref, b_host, side=side, num_inner_iterations=20)
        plain = oracle.solve("gmres", ref_op, b_host, num_inner_iterations=20)
    else:
        ref = oracle.solve(kind, ref_op, b_host, pre=pre_ref, side=side)
        n_pre_ref = oracle.last_pre_applies()
        plain = oracle.solve(kind, ref_op, b_host)
    assert ref.iterations < plain.iterations, (ref.iterations, plain.iterations)

    def count_at(iterations):
        if kind == "gmres":
            return oracle.solve_gmres_pre(ref_op, pre_ref, b_host, side=side, num_inner_iterations=20,
                                          num_iterations=iterations, abs_tol=0.0, rel_tol=0.0)[1]
        oracle.solve(kind, ref_op, b_host, pre=pre_ref, side=side, num_iterations=iterations, abs_tol=0.0, rel_tol=0.0)
        return oracle.last_pre_applies()

    _accept(api, s, x, ref, n_pre_ref, op, b, b_host, side, count_at)
    s.pre_op.close()
    mat.close()


# ---- 5. refusals --------------------------------------------------------------------------------------------------------
def test_refusals(env):
    api, mesh, oracle, ctx = env
    from stormruler_amd import _lib
    from stormruler_amd._lib import lib

    g = mesh.structured_box(6)
    mat = api.StencilMatrix.from_face_graph(ctx, g)
    n = g.n_cells
    r, z = api.DeviceVector(ctx, n), api.DeviceVector(ctx, n)
    ch = _Cheb(lib, mat, -1.0, 0.0, None, 2)
    assert ch.status == 0
    assert ch.apply(r, r) == E_INVALID and b"alias" in lib.storm_hip_last_error()
    short = api.DeviceVector(ctx, n - 1)
    assert ch.apply(short, z) == E_INVALID and ch.apply(r, short) == E_INVALID
    for degree in (0, 17):
        bad = _Cheb(lib, mat, -1.0, 0.0, None, degree)
        assert bad.status == E_INVALID and not bad.h
    bad = _Cheb(lib, mat, -1.0, 0.0, None, 2, 5.0, 4.0)  # lmin >= lmax
    assert bad.status == E_INVALID
    bad = _Cheb(lib, mat, -1.0, 0.0, short, 2)  # a scale of another size
    assert bad.status == E_INVALID
    v = C.c_double()
    assert lib.storm_hip_cheb_get(ch.h, b"no_such_key", C.byref(v)) == E_INVALID
    # a size mismatch is caught where the diagonal's is: at the solve
    g2 = mesh.structured_box(5)
    mat2 = api.StencilMatrix.from_face_graph(ctx, g2)
    eng = api.Krylov(ctx, 0)
    eng.set_operator(api.HipStencilOperator(mat2, -1.0, 0.0))
    assert lib.storm_hip_krylov_set_preconditioner_cheb(eng._h, ch.h, 1) == 0
    b2, x2 = api.DeviceVector.from_numpy(ctx, np.ones(g2.n_cells)), api.DeviceVector(ctx, g2.n_cells)
    p, res = _lib.SolverParams(), _lib.SolverResult()
    lib.storm_hip_solver_params_default(C.byref(p))
    assert lib.storm_hip_krylov_solve(eng._h, b2._h, x2._h, C.byref(p), C.byref(res), None, None) == E_INVALID
    assert b"Chebyshev" in lib.storm_hip_last_error()
    assert lib.storm_hip_krylov_set_preconditioner_cheb(eng._h, ch.h, 7) == E_INVALID  # no such side
    assert lib.storm_hip_krylov_set_preconditioner_cheb(eng._h, None, 1) == 0
    # a halo plan: single-rank only
    loc, send_idx = mesh.periodic_z_local_graph(8, 8, 8)
    halo = api.StencilMatrix.from_face_graph(ctx, loc)
    halo.set_halo([0], [0, loc.n_halo], send_idx, [0, loc.n_halo])
    assert _Cheb(lib, halo, -1.0, 0.0, None, 2).status == E_UNSUPPORTED
    assert lib.storm_hip_op_gershgorin(halo._h, -1.0, 0.0, None, C.byref(v)) == E_UNSUPPORTED
    # the Python class refuses what JacobiPreconditioner refuses
    pre = api.ChebyshevPreconditioner()
    with pytest.raises(TypeError):
        pre.build(r, r, api.HipTwoStageOperator(mat, -1.0, 1.0, -1.0, 1.0))
    with pytest.raises(TypeError):
        pre.build(r, r, api.make_operator(lambda y, x: None))
    ch.close()
    eng._free()
    for m in (mat, mat2, halo):
        m.close()


def test_chebyshev_preconditioner_is_an_operator_on_its_own(env):
    api, mesh, oracle, ctx = env
    g = mesh.structured_box(8)
    a = mesh.assemble_csr(g, -1.0, 0.0).tocsr()
    mat = api.StencilMatrix.from_face_graph(ctx, g)
    pre = api.ChebyshevPreconditioner(degree=3)
    r_host = np.cos(0.2 * np.arange(g.n_cells))
    r, z = api.DeviceVector.from_numpy(ctx, r_host), api.DeviceVector(ctx, g.n_cells)
    pre.build(z, r, api.HipStencilOperator(mat, -1.0, 0.0))
    pre.mul(z, r)
    lmax = cheb_ref.gershgorin(a, np.ones(g.n_cells))
    ref = cheb_ref.apply(a, np.ones(g.n_cells), r_host, lmax / 30, lmax, 3)
    assert np.linalg.norm(z.to_numpy() - ref) <= 1e-10 * np.linalg.norm(ref)
    pre.close()
    mat.close()


# ---- 6. the C++ driver --------------------------------------------------------------------------------------------------
def _driver(*args):
    exe = os.path.join(ROOT, "tests", "cpp", "cheb_driver")
    if not os.path.exists(exe):  # (git-ignored: a checkout that arrived without it)
        import __graft_entry__ as ge

        ge.build()
    out = subprocess.run([exe, *map(str, args)], check=True, capture_output=True, text=True, timeout=300).stdout
    return json.loads(out.strip().splitlines()[-1])


@pytest.mark.parametrize("kind,degree,jacobi,side", [("cg", 4, 0, "right"), ("bicgstab", 3, 1, "left")])
def test_cpp_driver_matches_oracle(kind, degree, jacobi, side):
    from oracle import oracle
    from stormruler_amd import mesh

    n = 16
    got = _driver(n, kind, degree, jacobi, side)
    g = mesh.structured_box(n)
    a = mesh.assemble_csr(g, -1.0, 0.0).tocsr()
    s_host = 1 / a.diagonal() if jacobi else np.ones(g.n_cells)
    lmax = cheb_ref.gershgorin(a, s_host)
    assert abs(got["lambda_max"] - lmax) <= 1e-13 * lmax and got["lambda_min"] == got["lambda_max"] / 30.0
    pre_ref = oracle.CallbackOperator(g.n_cells, lambda v: cheb_ref.apply(a, s_host, v, lmax / 30, lmax, degree))
    ref = oracle.solve(kind, oracle.StencilOperator(g, -1.0, 0.0), np.ones(g.n_cells), pre=pre_ref, side=side)
    assert got["converged"] and ref.converged
    assert abs(got["iterations"] - ref.iterations) <= max(2, int(0.1 * ref.iterations)), (got["iterations"], ref.iterations)
    assert abs(got["x_norm2"] - np.linalg.norm(ref.x)) <= 1e-5 * np.linalg.norm(ref.x)
    assert got["pre_applies"] == oracle.last_pre_applies()
    assert got["cheb_fused_applies"] + got["cheb_statement_applies"] >= got["pre_applies"] > 0
