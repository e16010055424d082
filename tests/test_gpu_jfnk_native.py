"""Device-resident JFNK: the finite-difference Jacobian as an operator of the engine (storm_hip_krylov_set_operator_fd),
the Newton loop as an engine method (STORM_HIP_JFNK) and their bindings, against numpy restatements of
SolverNewton.hpp:101-173 and the oracle's ``solve_jfnk``."""
import ctypes as C
import json
import math
import os
import subprocess

import numpy as np
import pytest

import exact_ref as er

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = float(np.finfo(np.float64).eps)
KAPPA, C3 = 1e-2, 0.5
BOXES = {"12": (12, 12, 12), "11x9x7": (11, 9, 7), "16": (16, 16, 16)}
NT_ROWS = 6 * (1 << 20) + 1  # the non-temporal instantiation, a partial block and the odd tail row


# ---- the numpy model of the product (SolverNewton.hpp:143-156, every operation rounded on its own) ----------------------
def safe_divide(a, b):
    return 0.0 if b == 0.0 else a / b


def dot_exact(a, b):
    """<a, b> of small dyadic vectors.  Every product is a multiple of q = the lowest set bit among them, and the sum of
    their magnitudes stays below 2^53 q (asserted): every product and every partial sum in any order is exact in fp64, so
    a device reduction has one admissible value -- this one."""
    prod = np.asarray(a, np.float64) * np.asarray(b, np.float64)
    nz = np.abs(prod[prod != 0.0])
    if nz.size == 0:
        return 0.0
    m, e = np.frexp(nz)
    k = np.ldexp(m, 53).astype(np.int64)
    q = float(np.ldexp((k & -k).astype(np.float64), e - 53).min())
    assert float((nz / q).sum()) < 2.0 ** 53 and np.array_equal(nz / q, np.rint(nz / q))
    return float((prod / q).sum()) * q  # (a sum of integers below 2^53, scaled by a power of two: exact)


def newton_mu(x):
    """:128-130 with <x, x> taken exactly (the fixtures keep it exact in any summation order)."""
    return math.sqrt(EPS) * math.sqrt(1.0 + math.sqrt(dot_exact(x, x)))


def fd_model(apply, x, w, y, mu, yy=None):
    """(z, s, delta, delta_inverse): z = fl(dinv * fl(A(s) - w)), s = fl(x + fl(delta y))."""
    yy = dot_exact(y, y) if yy is None else yy
    delta = safe_divide(mu, math.sqrt(yy))
    dinv = safe_divide(1.0, delta)
    prod = delta * y
    s = x + prod
    diff = apply(s) - w
    return dinv * diff, s, delta, dinv


def product_fixture(n):
    """x: stmt_vector scaled by 2^-40 (dyadic doubles of the size of delta y, so that the roundings of s show); w = 2 x;
    y integer-valued: <x, x> and <y, y> are exact whatever the order of the sum."""
    x = er.stmt_vector(n, 5).astype(np.float64) * 2.0 ** -40  # (seeds: the 2049-row fixture shows both roundings on its last row)
    y = er.int_vector(n, 5).astype(np.float64)
    if not y.any():
        y[0] = 7.0
    return x, 2.0 * x, y


@pytest.fixture(scope="module")
def env():
    from oracle import oracle
    from stormruler_amd import api, mesh

    ctx = api.Context(0)
    yield api, mesh, oracle, ctx
    ctx.close()


def _two_x(api, seen=None):
    """A(x) = 2 x as one axpbz with b = 0: exact.  ``seen``: a vector that keeps the last argument (the shifted point)."""
    lib = api.lib

    def mul(y_vec, x_vec):
        if seen is not None:
            api.check(lib.storm_hip_copy(seen._h, x_vec._h))
        api.check(lib.storm_hip_axpbz(y_vec._h, 2.0, x_vec._h, 0.0, x_vec._h))

    return api.make_operator(mul)


# ---- 1. the product, bit for bit -----------------------------------------------------------------------------------------
def test_the_roundings_of_the_fixture_show():
    """On the CPU: the one-rounding forms differ from the contract's on at least 1 % of the 2049-row fixture's rows and
    on its last row -- otherwise the bitwise case below proves nothing about the rounding."""
    n = 2049
    x, w, y = product_fixture(n)
    mu = newton_mu(x)
    z, s, delta, dinv = fd_model(lambda v: 2.0 * v, x, w, y, mu)
    s_fused = er.vfma(delta, y, x)
    z_fused = er.vfma(dinv, 2.0 * s, -(dinv * w))
    ds, dz = er.bits(s) != er.bits(s_fused), er.bits(z) != er.bits(z_fused)
    print(f"rows where fma(delta, y, x) differs: {ds.mean():.3f}; fma(dinv, z, -dinv w): {dz.mean():.3f}")
    assert ds.mean() >= 0.01 and ds[-1]
    assert dz.mean() >= 0.01 and dz[-1]


@pytest.mark.parametrize("n", [1, 2, 3, 693, 2049, NT_ROWS])
def test_product_bit_for_bit(env, n):
    api, mesh, oracle, ctx = env
    x, w, y = product_fixture(n)
    mu = newton_mu(x)
    xv, wv, yv = (api.DeviceVector.from_numpy(ctx, a) for a in (x, w, y))
    zv, seen = api.DeviceVector(ctx, n), api.DeviceVector(ctx, n)
    api.fill_with(zv, er.SENTINEL)
    op = api.FdJacobianOperator(_two_x(api, seen), xv, wv, mu)
    op.mul(zv, yv)
    z, s, _, _ = fd_model(lambda v: 2.0 * v, x, w, y, mu)
    assert er.same_bits(seen.to_numpy(), s)
    assert er.same_bits(zv.to_numpy(), z)
    assert er.same_bits(xv.to_numpy(), x) and er.same_bits(wv.to_numpy(), w) and er.same_bits(yv.to_numpy(), y)


# ---- 2. y = 0 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 2049])
def test_zero_direction(env, n):
    api, mesh, oracle, ctx = env
    x, w, _ = product_fixture(n)
    xv, wv = api.DeviceVector.from_numpy(ctx, x), api.DeviceVector.from_numpy(ctx, w)
    yv, zv, seen = api.DeviceVector(ctx, n), api.DeviceVector(ctx, n), api.DeviceVector(ctx, n)
    api.fill_with(zv, er.SENTINEL)
    api.FdJacobianOperator(_two_x(api, seen), xv, wv, newton_mu(x)).mul(zv, yv)
    z = zv.to_numpy()
    assert not np.isnan(z).any() and not z.any()
    assert er.same_bits(seen.to_numpy(), x)


# ---- 3. the fused reductions -----------------------------------------------------------------------------------------------
def _four_squares(t):
    """Integers (a, b, c, d) with a^2 + b^2 + c^2 + d^2 = t (Lagrange), by search from the largest a down."""
    for a in range(math.isqrt(t), -1, -1):
        ra = t - a * a
        for b in range(min(a, math.isqrt(ra)), -1, -1):
            rb = ra - b * b
            for c in range(min(b, math.isqrt(rb)), -1, -1):
                d = math.isqrt(rb - c * c)
                if d * d == rb - c * c:
                    return a, b, c, d
    raise AssertionError(t)


def split_fixture(n, seed):
    """(d, b, |b|): d = 1 on even rows and 3 on odd ones, b integer-valued and row dependent with <b, b> = 4^k, half of
    it on either class of rows (the last four rows of a class complete its sum of squares).  With A = diag(d), mu a power
    of two and x = 0, BiCGStab's first iteration is EXACT up to omega and none of its sums is trivial:
      delta = mu / 2^k, so v = J b = d b exactly; <rt, v> = 4^k / 2 + 3 4^k / 2 = 2 4^k; alpha = 1 / 2;
      s = b - d b / 2 = +- b / 2 with <s, s> = 4^(k - 1): delta is a power of two AGAIN and t = J s = d s exactly;
      <t, s> = 4^k / 2 and <t, t> = 5 4^k / 4 are exact in any order; omega = fl(2 / 5) is one division of exact values.
    So x = fma(omega, s, b / 2) has one admissible value per row, and it depends on both sums of the second product."""
    d = np.where(np.arange(n) % 2 == 0, 1.0, 3.0)
    b = er.int_vector(n, seed, -300, 300).astype(np.int64)
    rows = [np.flatnonzero(d == c) for c in (1.0, 3.0)]
    for r in rows:
        b[r[-4:]] = 0
    have = [int((b[r] * b[r]).sum()) for r in rows]
    k = 1
    while 2 ** (2 * k - 1) <= max(have):
        k += 1
    for r, h in zip(rows, have):
        b[r[-4:]] = _four_squares(2 ** (2 * k - 1) - h)
    assert all(int((b[r] * b[r]).sum()) == 2 ** (2 * k - 1) for r in rows) and np.abs(b).max() < 1 << 20
    return d, b.astype(np.float64), 2.0 ** k


def bicgstab_model(product, b, iterations, fma=None):
    """SolverBiCgStab.hpp:93-165 without preconditioner from x = 0, as the engine states it: every dot exact
    (``dot_exact`` where the data allow it), the vector statements with the engine's roundings (``fma``: exact_ref.vfma)."""
    fma = fma or er.vfma
    x = np.zeros_like(b)
    r = b - product(x)
    rt = r.copy()
    rho = dot_exact(rt, r)
    hist = [math.sqrt(rho)]
    p, v = r.copy(), np.zeros_like(b)
    alpha = omega = beta = 0.0
    for it in range(iterations):
        p = r.copy() if it == 0 else fma(beta, fma(-omega, v, p), r)
        v = product(p)
        alpha = safe_divide(rho, dot_exact(rt, v))
        r = fma(-alpha, v, r)
        t = product(r)
        omega = safe_divide(dot_exact(t, r), dot_exact(t, t))
        x = fma(omega, r, fma(alpha, p, x))
        r = fma(-omega, t, r)
        hist.append(math.sqrt(float(np.dot(r, r))))  # (r is no longer dyadic: this entry is held to n eps, not to the bit)
        rho_bar, rho = rho, float(np.dot(rt, r))
        beta = safe_divide(alpha * rho, omega * rho_bar)
    return x, np.array(hist), (alpha, omega)


@pytest.mark.parametrize("n", [693, 4099, NT_ROWS])
def test_fused_reductions_on_exact_data(env, n):
    """One BiCGStab iteration on A = diag(d) through the finite-difference operator (``split_fixture``): x equals the numpy
    restatement of SolverBiCgStab.hpp:93-165 around the product model bit for bit -- so <rt, v> behind the first product
    and <t, s>, <t, t> behind the second arrived exactly -- with the reductions riding in the difference statement's pass
    (``fd_fused_dots`` rises by two) and with ``lin_fuse = 0``, where it leaves alone (the counter does not move).  At
    6 2^20 + 1 rows (non-temporal accesses, a partial block, the odd tail) the model's fused multiply-adds are numpy's
    a x + t, a double rounding of the same exact value: x is held to one last place there.  history[1] = |r| is a sum of
    n squares of rounded values, order dependent: held to n eps."""
    api, mesh, oracle, ctx = env
    d, b, norm_b = split_fixture(n, 11)
    x_lin = er.stmt_vector(n, 2).astype(np.float64)
    w, mu = d * x_lin, 2.0 ** -20
    big = n > 100000
    fma = (lambda a, x, t: a * x + t) if big else None
    ref_x, ref_hist, (alpha, omega) = bicgstab_model(lambda y: fd_model(lambda v: d * v, x_lin, w, y, mu)[0], b, 1, fma)
    assert ref_hist[0] == norm_b and alpha == 0.5 and omega == 2.0 / 5.0
    xl, wv, bv, dv = (api.DeviceVector.from_numpy(ctx, a) for a in (x_lin, w, b, d))
    op = api.FdJacobianOperator(api.make_operator(lambda y_vec, x_vec: api.vmul(y_vec, dv, x_vec)), xl, wv, mu)
    got = {}
    for fuse in (1, 0):  # held back with the reductions in its pass / leaving alone
        ctx.set_option("lin_fuse", fuse)
        rode = ctx.counter("fd_fused_dots")
        try:
            s = api.BiCgStabSolver()
            s.num_iterations, s.absolute_error_tolerance, s.relative_error_tolerance = 1, 0.0, 0.0
            s.record_history = True
            xv = api.DeviceVector(ctx, n)
            s.solve(xv, bv, op)
        finally:
            ctx.set_option("lin_fuse", 1)
        assert s.iteration == 1
        assert ctx.counter("fd_fused_dots") - rode == (2 if fuse else 0)
        got[fuse] = (xv.to_numpy(), s.history.copy())
        assert got[fuse][1][0] == ref_hist[0]
        assert abs(got[fuse][1][1] - ref_hist[1]) <= n * EPS * ref_hist[1], (fuse, got[fuse][1], ref_hist)
        if big:
            assert (np.abs(got[fuse][0] - ref_x) <= np.spacing(np.abs(ref_x))).all(), fuse
        else:
            assert er.same_bits(got[fuse][0], ref_x), fuse
    assert er.same_bits(got[0][0], got[1][0])  # (x depends on exact sums only: the same bits either way)


# ---- the cubic problem of tests/test_gpu_precond.py::test_jfnk_on_a_nonlinear_operator -----------------------------------
class Cubic:
    """A(x) = x - kappa L x + c x^3 on a box: the device callback, the oracle's operator and the right-hand side."""

    def __init__(self, api, mesh, oracle, ctx, shape):
        self.g = g = mesh.structured_box(*shape) if len(set(shape)) > 1 else mesh.structured_box(shape[0])
        self.n = g.n_cells
        self.mat = api.StencilMatrix.from_face_graph(ctx, g)
        self.sq = api.DeviceVector(ctx, g.n_cells)
        self.lin = {v: oracle.StencilOperator(g, -KAPPA, 1.0, variant=v) for v in ("strict", "fma")}
        self.ref_op = oracle.CallbackOperator(g.n_cells, self.host)
        self.b = 1.0 + 0.5 * np.sin(5.0 * g.center[: g.n_cells, 0])
        self.api = api

    def host(self, v, variant="strict"):
        return self.lin[variant].apply(v) + C3 * ((v * v) * v)

    def device(self, y, x):
        self.mat.apply(-KAPPA, 1.0, x, y)
        self.api.vmul(self.sq, x, x)
        self.api.vmul_add(y, C3, self.sq, x)

    def close(self):
        self.mat.close()


@pytest.fixture(scope="module")
def cubics(env):
    api, mesh, oracle, ctx = env
    made = {}

    def get(name):
        if name not in made:
            pb = Cubic(api, mesh, oracle, ctx, BOXES[name])
            pb.ref, pb.ref_inner = oracle.solve_jfnk(pb.ref_op, pb.b)  # computed once, shared, left unchanged
            fma_op = oracle.CallbackOperator(pb.n, lambda v, pb=pb: pb.host(v, "fma"))
            pb.ref_fma, _ = oracle.solve_jfnk(fma_op, pb.b, variant="fma")  # the oracle's other build: its own spread
            made[name] = pb
        return made[name]

    yield get
    for pb in made.values():
        pb.close()


# ---- 4. the product on a real operator --------------------------------------------------------------------------------------
def test_product_on_the_cubic_operator(env, cubics):
    """|z_dev - z_ref|_i <= max(10 |z_strict - z_fma|_inf, 64 eps (|A(s)|_i + |w_i|) delta_inverse).

    The floor: z_i = delta_inverse (A(s)_i - w_i).  A(s)_i and w_i are each a 7-point row plus a cubic, about a dozen
    rounded operations whose order and contraction differ between the device and numpy, so each carries an absolute error
    of a few eps times its magnitude (64 eps bounds a dozen operations with room for the row's cancellation); the
    difference of the two keeps those absolute errors and the quotient multiplies them by delta_inverse -- the
    cancellation a difference quotient amplifies."""
    api, mesh, oracle, ctx = env
    pb = cubics("11x9x7")
    assert pb.n == 693
    x = pb.b.copy()
    y = np.sin(0.37 * np.arange(pb.n) + 0.1)
    mu = math.sqrt(EPS) * math.sqrt(1.0 + float(np.linalg.norm(x)))
    yy = float(np.dot(y, y))
    model = {v: fd_model(lambda s, v=v: pb.host(s, v), x, pb.host(x, v), y, mu, yy) for v in ("strict", "fma")}
    z_ref, s_ref, _, dinv = model["strict"]
    spread = float(np.abs(z_ref - model["fma"][0]).max())
    xv, yv = api.DeviceVector.from_numpy(ctx, x), api.DeviceVector.from_numpy(ctx, y)
    wv, zv = api.DeviceVector(ctx, pb.n), api.DeviceVector(ctx, pb.n)
    op = api.make_operator(pb.device)
    op.mul(wv, xv)
    api.FdJacobianOperator(op, xv, wv, mu).mul(zv, yv)
    err = np.abs(zv.to_numpy() - z_ref)
    floor = 64.0 * EPS * (np.abs(pb.host(s_ref)) + np.abs(pb.host(x))) * dinv
    tol = np.maximum(10.0 * spread, floor)
    print(f"fd product on the cubic operator, 693 rows: max |z_dev - z_ref| = {err.max():.3e}, oracle builds' spread "
          f"{spread:.3e}, floor min {floor.min():.3e} max {floor.max():.3e}, max err / tol = {(err / tol).max():.3f}")
    assert (err <= tol).all()


# ---- 5. whole solves against the oracle ------------------------------------------------------------------------------------
def _device_solve(api, ctx, pb, solver=None):
    s = solver or api.DeviceJfnkSolver()
    s.record_history = True
    b, x = api.DeviceVector.from_numpy(ctx, pb.b), api.DeviceVector(ctx, pb.n)
    ok = s.solve(x, b, api.make_operator(pb.device))
    return s, ok, x.to_numpy()


@pytest.mark.parametrize("name", list(BOXES))
def test_whole_solve_against_the_oracle(env, cubics, name):
    api, mesh, oracle, ctx = env
    pb = cubics(name)
    ref, inner = pb.ref, pb.ref_inner
    assert ref.converged and 1 < ref.iterations < 20
    s, ok, x = _device_solve(api, ctx, pb)
    # The per-step history, entry by entry: within 1e-6 relative of the oracle's, and where the oracle's own two builds
    # differ by more than a tenth of that (the last step: its residual is what the inner solves' 1e-8 stopping left, and
    # strict and FMA differ by 7.5e-6 / 2.1e-5 / 1.2e-5 of it on the three boxes) never tighter than ten times their
    # spread at that step -- the project's rule (test_gpu_fixed_k.py).
    assert ref.history.shape == pb.ref_fma.history.shape
    spread = np.abs(ref.history - pb.ref_fma.history) / ref.history
    tol = np.maximum(1e-6, 10.0 * spread)
    rel_hist = np.abs(s.history - ref.history) / ref.history if s.history.shape == ref.history.shape else np.full(1, np.inf)
    print(f"box {name}: Newton steps {s.iteration} (oracle {ref.iterations}), inner {s.inner_iterations} (oracle {inner}), "
          f"|x - x_ref| / |x_ref| = {np.linalg.norm(x - ref.x) / np.linalg.norm(ref.x):.3e}, history relative "
          f"differences entry by entry {np.array2string(rel_hist, precision=2)}, bounds {np.array2string(tol, precision=2)}, "
          f"applies {s.num_applies}")
    assert ok
    assert s.iteration == ref.iterations
    assert abs(s.inner_iterations - inner) <= max(2, int(0.1 * inner))
    assert np.linalg.norm(x - ref.x) <= 1e-7 * np.linalg.norm(ref.x)
    res = pb.host(x) - pb.b
    assert np.linalg.norm(res) < 1.01 * max(1e-6, 1e-6 * ref.initial_error)
    assert s.history.shape == ref.history.shape and (rel_hist <= tol).all()
    # every application of A: one per residual (init and each step), and per inner solve one for its initial residual
    # and two per inner iteration
    assert s.num_applies == 1 + s.iteration * 2 + 2 * s.inner_iterations


def test_linear_kat_native_operator(env):
    """A native operator is linear: the first step lands on the answer, as the oracle's does."""
    api, mesh, oracle, ctx = env
    g = mesh.structured_box(16)
    mat = api.StencilMatrix.from_face_graph(ctx, g)
    ref, inner = oracle.solve_jfnk(oracle.StencilOperator(g, -1.0, 0.0), np.ones(g.n_cells))
    s = api.DeviceJfnkSolver()
    b, x = api.DeviceVector.from_numpy(ctx, np.ones(g.n_cells)), api.DeviceVector(ctx, g.n_cells)
    assert s.solve(x, b, api.HipStencilOperator(mat, -1.0, 0.0)) and ref.converged
    assert s.iteration == ref.iterations
    assert abs(s.inner_iterations - inner) <= max(2, int(0.1 * inner))
    assert np.linalg.norm(x.to_numpy() - ref.x) <= 1e-7 * np.linalg.norm(ref.x)
    mat.close()


# ---- 6. residency --------------------------------------------------------------------------------------------------------
def test_no_reduction_visits_the_host(env, cubics):
    api, mesh, oracle, ctx = env
    pb = cubics("12")
    h0, j0 = ctx.counter("host_reductions"), ctx.counter("jfnk_inner_solves")
    s, ok, _ = _device_solve(api, ctx, pb)
    assert ok
    assert ctx.counter("host_reductions") == h0
    assert ctx.counter("jfnk_inner_solves") - j0 == s.iteration > 0
    h1 = ctx.counter("host_reductions")
    host, ok, _ = _device_solve(api, ctx, pb, api.JfnkSolver())  # the unchanged host loop: |y| at every product
    assert ok
    assert ctx.counter("host_reductions") - h1 >= 2 * host.inner_iterations > 0
    assert ctx.counter("jfnk_inner_solves") - j0 == s.iteration


# ---- 7. stepping -----------------------------------------------------------------------------------------------------------
def test_stepping_and_a_second_solve_reproduce_the_first(env, cubics):
    api, mesh, oracle, ctx = env
    pb = cubics("11x9x7")
    s = api.DeviceJfnkSolver()
    first, ok, x1 = _device_solve(api, ctx, pb, s)
    hist1, inner1 = first.history.copy(), first.inner_iterations
    assert ok
    _, ok, x2 = _device_solve(api, ctx, pb, s)  # the same object: the nested engine's state is reset
    assert ok and er.same_bits(s.history, hist1) and er.same_bits(x2, x1) and s.inner_iterations == inner1
    step = api.DeviceJfnkSolver()
    step.device_loop = False  # the reference's loop over init / iterate / finalize
    _, ok, x3 = _device_solve(api, ctx, pb, step)
    assert ok and er.same_bits(step.history, hist1) and er.same_bits(x3, x1) and step.inner_iterations == inner1


# ---- 8. the operator under GMRES(20) ---------------------------------------------------------------------------------------
def test_fd_operator_under_gmres(env, cubics):
    """J t = r at the second Newton iterate against a dense solve with the analytic Jacobian I - kappa L + 3 c diag(x^2).
    Truncation and cancellation of the difference quotient are both ~ mu |x| ~ 1e-8 relative: two decades of margin."""
    api, mesh, oracle, ctx = env
    pb = cubics("11x9x7")
    two, _ = oracle.solve_jfnk(pb.ref_op, pb.b, num_iterations=2)
    assert two.iterations == 2
    x = two.x
    r = pb.b - pb.host(x)
    jac = mesh.assemble_csr(pb.g, -KAPPA, 1.0)[:, : pb.n].toarray() + np.diag(3.0 * C3 * x * x)
    t_ref = np.linalg.solve(jac, r)
    mu = math.sqrt(EPS) * math.sqrt(1.0 + float(np.linalg.norm(x)))
    xv, rv = api.DeviceVector.from_numpy(ctx, x), api.DeviceVector.from_numpy(ctx, r)
    wv, tv = api.DeviceVector(ctx, pb.n), api.DeviceVector(ctx, pb.n)
    op = api.make_operator(pb.device)
    op.mul(wv, xv)
    s = api.GmresSolver()
    s.num_inner_iterations = 20
    s.absolute_error_tolerance, s.relative_error_tolerance = 0.0, 1e-10
    assert s.solve(tv, rv, api.FdJacobianOperator(op, xv, wv, mu))
    rel = np.linalg.norm(tv.to_numpy() - t_ref) / np.linalg.norm(t_ref)
    print(f"GMRES(20) on the fd operator, 693 rows: {s.iteration} iterations, |t - t_ref| / |t_ref| = {rel:.3e}")
    assert rel <= 1e-6


# ---- 9. errors -------------------------------------------------------------------------------------------------------------
def test_a_failing_callback_aborts_and_the_context_stays_usable(env, cubics):
    api, mesh, oracle, ctx = env
    lib, _lib = api.lib, api._lib
    pb = cubics("11x9x7")

    def cg():
        s = api.CgSolver()
        b, x = api.DeviceVector.from_numpy(ctx, pb.b), api.DeviceVector(ctx, pb.n)
        assert s.solve(x, b, api.HipStencilOperator(pb.mat, -KAPPA, 1.0))
        return x.to_numpy(), s.iteration

    before = cg()
    calls = []

    def failing(_user, y_handle, x_handle):
        try:
            calls.append(1)
            if len(calls) == 3:
                return 7
            pb.device(api.DeviceVector._borrow(ctx, y_handle), api.DeviceVector._borrow(ctx, x_handle))
            return 0
        except BaseException:  # never unwind through the C frames, and never leave the solve waiting
            return 1

    cb = _lib.APPLY_FN(failing)
    h = C.c_void_p()
    api.check(lib.storm_hip_krylov_create(ctx._h, 10, C.byref(h)))
    try:
        api.check(lib.storm_hip_krylov_set_operator_fn(h, cb, None))
        p, r = _lib.SolverParams(), _lib.SolverResult()
        lib.storm_hip_solver_params_default(C.byref(p))
        b, x = api.DeviceVector.from_numpy(ctx, pb.b), api.DeviceVector(ctx, pb.n)
        assert lib.storm_hip_krylov_solve(h, b._h, x._h, C.byref(p), C.byref(r), None, None) == -1  # STORM_HIP_E_INVALID
        assert b"returned 7" in lib.storm_hip_last_error() and len(calls) == 3
    finally:
        lib.storm_hip_krylov_destroy(h)
    after = cg()
    assert after[1] == before[1] and er.same_bits(after[0], before[0])


def test_refusals(env):
    api, mesh, oracle, ctx = env
    lib, _lib = api.lib, api._lib
    cb = _lib.APPLY_FN(lambda _u, _y, _x: 0)
    a, b3, c = api.DeviceVector(ctx, 4), api.DeviceVector(ctx, 3), api.DeviceVector(ctx, 4)
    other = api.Context(0)
    foreign = api.DeviceVector(other, 4)
    h = C.c_void_p()
    api.check(lib.storm_hip_krylov_create(ctx._h, 1, C.byref(h)))
    try:
        def refused(status, word):
            assert status == -1 and word in lib.storm_hip_last_error(), (status, lib.storm_hip_last_error())

        refused(lib.storm_hip_krylov_set_operator_fd(None, cb, None, a._h, c._h, 1e-8), b"null")
        refused(lib.storm_hip_krylov_set_operator_fd(h, C.cast(None, _lib.APPLY_FN), None, a._h, c._h, 1e-8), b"null")
        refused(lib.storm_hip_krylov_set_operator_fd(h, cb, None, None, c._h, 1e-8), b"null")
        refused(lib.storm_hip_krylov_set_operator_fd(h, cb, None, a._h, None, 1e-8), b"null")
        for mu in (0.0, -1e-8, math.inf, math.nan):
            refused(lib.storm_hip_krylov_set_operator_fd(h, cb, None, a._h, c._h, mu), b"mu")
        refused(lib.storm_hip_krylov_set_operator_fd(h, cb, None, a._h, b3._h, 1e-8), b"rows")
        refused(lib.storm_hip_krylov_set_operator_fd(h, cb, None, a._h, foreign._h, 1e-8), b"context")
        api.check(lib.storm_hip_krylov_set_operator_fd(h, cb, None, a._h, c._h, 1e-8))
        y, z = api.DeviceVector(ctx, 4), api.DeviceVector(ctx, 4)
        refused(lib.storm_hip_krylov_apply(None, y._h, z._h), b"null")
        refused(lib.storm_hip_krylov_apply(h, None, z._h), b"null")
        refused(lib.storm_hip_krylov_apply(h, y._h, None), b"null")
        refused(lib.storm_hip_krylov_apply(h, y._h, y._h), b"alias")
        v = C.c_int64(-5)
        refused(lib.storm_hip_krylov_get_int(None, b"inner_iterations", C.byref(v)), b"null")
        refused(lib.storm_hip_krylov_get_int(h, None, C.byref(v)), b"null")
        refused(lib.storm_hip_krylov_get_int(h, b"inner_iterations", None), b"null")
        refused(lib.storm_hip_krylov_get_int(h, b"no_such_key", C.byref(v)), b"unknown key")
        api.check(lib.storm_hip_krylov_get_int(h, b"inner_iterations", C.byref(v)))
        assert v.value == 0
        # JFNK differentiates its operator itself: a finite-difference operator as A is refused, before any device work
        j = C.c_void_p()
        api.check(lib.storm_hip_krylov_create(ctx._h, 10, C.byref(j)))
        try:
            api.check(lib.storm_hip_krylov_set_operator_fd(j, cb, None, a._h, c._h, 1e-8))
            p, r = _lib.SolverParams(), _lib.SolverResult()
            lib.storm_hip_solver_params_default(C.byref(p))
            assert lib.storm_hip_krylov_solve(j, y._h, z._h, C.byref(p), C.byref(r), None, None) == -6  # STORM_HIP_E_UNSUPPORTED
            assert b"JFNK" in lib.storm_hip_last_error()
        finally:
            lib.storm_hip_krylov_destroy(j)
    finally:
        lib.storm_hip_krylov_destroy(h)
        other.close()


# ---- 10. C++ ---------------------------------------------------------------------------------------------------------------
def _driver(*args):
    exe = os.path.join(ROOT, "tests", "cpp", "jfnk_driver")
    if not os.path.exists(exe):  # (git-ignored: a checkout that arrived without it)
        import __graft_entry__ as ge

        ge.build()
    out = subprocess.run([exe, *map(str, args)], check=True, capture_output=True, text=True, timeout=300).stdout
    return [json.loads(line) for line in out.strip().splitlines()]


def test_cpp_driver_native_against_the_oracle_and_the_host_loop(cubics):
    pb = cubics("12")
    ref, inner = pb.ref, pb.ref_inner
    samples, native, _, host, both = _driver(12, "both")  # per arm: x at five rows, the result line; then the arms' distance
    assert native["converged"] and host["converged"]
    assert native["iterations"] == ref.iterations
    assert abs(native["inner_iterations"] - inner) <= max(2, int(0.1 * inner))
    assert abs(native["x_norm2"] - np.linalg.norm(ref.x)) <= 1e-7 * np.linalg.norm(ref.x)
    # (one JSON line cannot carry x: five rows of it against the oracle's, to the bound ||x - x_ref|| has in case 5)
    rows = samples["x_rows"]
    assert rows[0] == 0 and rows[-1] == pb.n - 1
    assert np.abs(np.array(samples["x_samples"]) - ref.x[rows]).max() <= 1e-7 * np.linalg.norm(ref.x)
    assert native["residual_norm2"] < 1.01 * max(1e-6, 1e-6 * ref.initial_error)
    assert both["x_diff_norm2"] <= 1e-7 * both["x_host_loop_norm2"]  # ||x_native - x_host_loop||, not a difference of norms
    assert native["host_reductions"] == 0 < host["host_reductions"]
