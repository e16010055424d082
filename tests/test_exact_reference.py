"""The exact references of tests/exact_ref.py, checked where no GPU is needed: the integer operator against the CPU
oracle's stencil, the closed forms of the first Krylov iteration against a Fraction brute force and against
``oracle.solve(..., num_iterations=1)`` in both of its arithmetic variants; the coefficient-form restatement of every
engine method against an elementwise brute force, its tolerances against their caps and the oracle on the GPU tests'
own data, and the size of the defects those tolerances must see."""
import math
from fractions import Fraction

import numpy as np
import pytest

import exact_ref as er

BOXES = [(13, 9, 7), (4, 4, 4), (16, 8, 6), (31, 3, 5)]


@pytest.fixture(scope="module")
def env():
    from oracle import oracle
    from stormruler_amd import mesh

    return oracle, mesh


def _case(mesh, shape, seed):
    g = er.unit_box(mesh, *shape)
    b = er.int_vector(g.n_cells, seed)
    return g, b


@pytest.mark.parametrize("shape", BOXES)
def test_integer_operator_is_the_oracle_stencil(env, shape):
    oracle, mesh = env
    g, b = _case(mesh, shape, 1)
    z = er.int_apply(shape, b)
    assert np.array_equal(oracle.StencilOperator(g, -1.0, 0.0).apply(b.astype(np.float64)), z.astype(np.float64))
    # the slab rows of a partition are the same rows of the whole box
    nx, ny, nz = shape
    assert np.array_equal(er.int_apply(shape, b, 2, nz - 1), z[2 * nx * ny:(nz - 1) * nx * ny])


def test_exact_sums_refuse_what_fp64_cannot_add_exactly():
    a = np.full(10, 1 << 26, dtype=np.int64)
    with pytest.raises(AssertionError):
        er.exact_dot(a, a)  # 10 * 2^52 >= 2^53
    assert er.exact_dot(a[:1], a[:1]) == 1 << 52
    first = np.arange(1, 1001, dtype=np.int64)
    assert er.exact_dot(np.ones(1000, np.int64), first) == 1000 * 1001 // 2


def test_tolerance_is_tight_enough_to_see_one_row():
    assert er.fold_depth(1) == 65 and er.fold_depth(2048 * 256) == 65 and er.fold_depth(2048 * 256 + 1) == 66
    with pytest.raises(AssertionError):
        er.tolerance(1 << 20, 10**12, 1)  # cancellation this deep cannot separate a dropped row from rounding


def test_closed_forms_against_a_fraction_brute_force(env):
    """The first iteration of CG, GMRES and BiCGStab, done in exact rational arithmetic on a tiny box."""
    oracle, mesh = env
    shape = (3, 4, 2)
    _, b = _case(mesh, shape, 7)
    s = er.Sums(shape, b)
    fs = er.FirstStep(s)
    bq = [Fraction(int(v)) for v in b]

    def apply(v):
        # the operator on Fractions: columns of the integer operator
        out = [Fraction(0)] * len(v)
        for j, vj in enumerate(v):
            if vj == 0:
                continue
            e = np.zeros(len(v), np.int64)
            e[j] = 1
            col = er.int_apply(shape, e)
            for i in np.nonzero(col)[0]:
                out[i] += int(col[i]) * vj
        return out

    def dot(u, v):
        return sum((ui * vi for ui, vi in zip(u, v)), Fraction(0))

    z = apply(bq)
    assert dot(bq, bq) == s.rr and dot(bq, z) == s.pz and dot(z, z) == s.zz
    y = apply(z)
    assert dot(y, z) == s.yz and dot(y, y) == s.yy and dot(y, bq) == s.yb == s.zz
    a = dot(bq, bq) / dot(bq, z)
    # CG
    r1 = [bi - a * zi for bi, zi in zip(bq, z)]
    assert dot(r1, r1) == a * a * s.zz - s.rr
    assert er.close(math.sqrt(float(dot(r1, r1))), fs.cg_h1, 1e-15)
    # GMRES: the first step minimises |b - c A b| over c
    c = dot(bq, z) / dot(z, z)
    g1 = [bi - c * zi for bi, zi in zip(bq, z)]
    assert dot(g1, g1) == s.rr - Fraction(s.pz * s.pz, s.zz)
    assert er.close(math.sqrt(float(dot(g1, g1))), fs.gmres_h1, 1e-15)
    # BiCGStab
    sv = r1
    t = apply(sv)
    om = dot(t, sv) / dot(t, t)
    b1 = [si - om * ti for si, ti in zip(sv, t)]
    assert er.close(math.sqrt(float(dot(b1, b1))), fs.bicgstab_h1, 1e-15)
    assert fs.h0 == math.sqrt(float(dot(bq, bq)))


@pytest.mark.parametrize("variant", ["strict", "fma"])
@pytest.mark.parametrize("shape", BOXES)
def test_closed_forms_against_the_oracle_solvers(env, shape, variant):
    oracle, mesh = env
    g, b = _case(mesh, shape, 3)
    fs = er.FirstStep(er.Sums(shape, b))
    op = oracle.StencilOperator(g, -1.0, 0.0)
    bf = b.astype(np.float64)

    def one(kind, **kw):
        r = oracle.solve(kind, op, bf, num_iterations=1, abs_tol=0.0, rel_tol=0.0, variant=variant, **kw)
        assert r.iterations == 1 and r.history.size == 2
        assert r.history[0] == fs.h0  # bitwise: sqrt of an exact integer sum
        return r

    r = one("cg")
    assert np.array_equal(r.x, fs.cg_x1(b))  # bitwise, every element
    assert er.close(r.history[1], fs.cg_h1, fs.cg_tol)
    for m in (1, 30):
        r = one("gmres", num_inner_iterations=m)
        assert er.close(r.history[1], fs.gmres_h1, fs.gmres_tol)
    r = one("bicgstab")
    assert er.close(r.history[1], fs.bicgstab_h1, fs.bicgstab_tol)
    basis = er.Basis(shape, b)
    for kind in ("cgs", "tfqmr"):
        pins = er.Pins(oracle, g, shape, b, kind, fs=fs, K=1, basis=basis)
        pins.check(one(kind).history, f"{kind} {variant}")
    # IDR(s > 1) at k = 0 and BiCGStab(l >= 2) at j = 0 (here s = l = 50, the oracle's default) end their first
    # iteration on CG's r1: beta = phi_0 / <p_0, A r> = rr / pz (SolverIdrs.hpp:132, :244-246), and r_0 - alpha u_1
    # with u_1 = A b, alpha = rr / pz (SolverBiCgStab.hpp:275-283).  IDR's floor (c = 7, er.C1) on CG's terms
    oracle.rng_reset(variant)
    r = one("idrs")
    a = Fraction(fs.s.rr, fs.s.pz)
    assert er.close(r.history[1], fs.cg_h1, er.tolerance(fs.s.n, fs.s.rr + a * a * fs.s.zz, a * a * fs.s.zz - fs.s.rr,
                                                         c=er.C1["idrs"]))
    r = one("bicgstabl")
    assert er.close(r.history[1], fs.cg_h1, fs.cg_tol)


def test_a_dropped_row_is_far_outside_the_tolerance(env):
    """What the pins are for: one row fewer in <r,r> or <p,z> moves every closed form by far more than its tolerance."""
    oracle, mesh = env
    shape = (16, 8, 6)
    _, b = _case(mesh, shape, 5)
    s = er.Sums(shape, b)
    fs = er.FirstStep(s)
    z = er.int_apply(shape, b)
    short = float(s.pz - int(b[-1]) * int(z[-1]))
    assert s.rr / short != fs.cg_alpha
    a = Fraction(s.rr) / Fraction(short)
    assert not er.close(math.sqrt(float(a * a * s.zz - s.rr)), fs.cg_h1, fs.cg_tol)


# ---- the Krylov methods in coefficient form (exact_ref.Space) ----------------------------------------------------------

SMALL = (64, 48, 40)  # the shapes and data of tests/test_gpu_exact_first_step.py
ODD = (37, 21, 19)
ENGINE = [("cgs", None), ("tfqmr", None), ("tfqmr1", None), ("richardson", None), ("bicgstabl", 1),
          ("bicgstabl", 2), ("bicgstabl", 3), ("idrs", 1), ("idrs", 2), ("idrs", 4)]
JACOBI = [("cg", None), ("cgs", None), ("tfqmr", None), ("idrs", 2), ("fgmres", 1), ("fgmres", 30),
          ("richardson", None), ("bicgstabl", 2)]
FIXED_SIDE = {"richardson": "left", "bicgstabl": "left", "fgmres": "right"}  # what these methods do whatever pre_side
BRUTE = [(m, p, None) for m, p in ENGINE + [("cg", None)]] + \
        [(m, p, side) for m, p in JACOBI for side in ("left", "right") if FIXED_SIDE.get(m, side) == side]


def _mid(m, p):
    return m + ("" if p is None else str(p))


_gpu_data = {}


def _gpu_case(env, shape):
    """The GPU tests' problem: the unit box, b = int_vector(n, 31), one Basis per preconditioning."""
    oracle, mesh = env
    if shape not in _gpu_data:
        g = er.unit_box(mesh, *shape)
        b = er.int_vector(g.n_cells, 31)
        _gpu_data[shape] = (g, b, er.FirstStep(er.Sums(shape, b)),
                            {False: er.Basis(shape, b), True: er.Basis(shape, b, 1.0 / er.int_diagonal(shape))})
    return _gpu_data[shape]


@pytest.mark.parametrize("shape", BOXES + [(5, 1, 3)])
def test_integer_diagonal_is_the_operator_diagonal(shape):
    n = shape[0] * shape[1] * shape[2]
    d = er.int_diagonal(shape)
    assert all(int(er.int_apply(shape, np.eye(n, dtype=np.int64)[i])[i]) == d[i] for i in range(n))


@pytest.mark.parametrize("method,param,side", BRUTE, ids=[f"{_mid(m, p)}-{s}" for m, p, s in BRUTE])
def test_coefficient_form_against_a_brute_force(method, param, side):
    """Every method's statements run once on coefficient columns over the integer chain (Gram matrix, shifts, the
    2^-56 scale of D') and once elementwise in Fractions / PREC-digit decimals on a tiny box: the same history and
    x_K (exactly where rational; to 1e-60 where decimal).  IDR(s) takes fixed dyadic shadow vectors; the Jacobi cases
    run the preconditioner on both sides of the comparison."""
    shape = (4, 3, 3)
    n = 36
    b = er.int_vector(n, 7)
    dinv = 1.0 / er.int_diagonal(shape) if side else None
    rng = np.random.default_rng(11)
    shadow = [rng.integers(1, 1 << 20, n) / float(1 << 21) for _ in range(3)]  # dyadic, as fill_randomly's are
    K = er.iterations(method, param, side is not None) + 1
    dec = method in er.DECIMAL_METHODS
    sp = er.Space(er.Basis(shape, b, dinv), decimal=dec)
    el = er.ElemSpace(shape, b, dinv, decimal=dec)

    coef = er.exact_run(sp, method, param, K, side, shadow)
    brute = er.exact_run(el, method, param, K, side, shadow)
    assert len(coef.hist_sq) == len(brute.hist_sq) == K + 1
    if not dec:
        assert coef.hist_sq == brute.hist_sq
        assert np.array_equal(sp.materialize(coef.x), np.array([float(v) for v in brute.x]))
        return
    from decimal import localcontext

    with localcontext() as ctx:
        ctx.prec = er.PREC
        for c, e in zip(coef.hist_sq, brute.hist_sq):
            assert abs(c - e) <= abs(e) * er._dec(Fraction(1, 10 ** 60))
        xc = sum((er._dec(c) * sp.basis.W[k].astype(object) for k, c in coef.x.c.items()), np.zeros(n, dtype=object))
        scale = max(abs(v) for v in brute.x)
        assert max(abs(a - e) for a, e in zip(xc, brute.x)) <= scale * er._dec(Fraction(1, 10 ** 60))


@pytest.mark.parametrize("shape", [SMALL, ODD], ids=["small", "odd"])
def test_richardson_is_exact_in_integers(env, shape):
    """omega = 2^-5: the coefficient form's x_k, materialised, is 32^-k times the integer iteration, k = 1 ... 4, and
    history[1] is the root of an exact sum (every bound asserted inside richardson_integers)."""
    g, b, _, bases = _gpu_case(env, shape)
    sp = er.Space(bases[False])
    run = er.richardson(sp, 4, er.OMEGA)
    for k in range(1, 5):
        X, R = er.richardson_integers(shape, b, k)
        assert np.array_equal(sp.materialize(er.richardson(sp, k, er.OMEGA).x), X / 32.0 ** k)
        assert run.hist_sq[k] == Fraction(er.big_dot(R, R), 4 ** (5 * k))
    assert run.history[1] == er.richardson_h1(shape, b)


GPU_CASES = [(m, p, None) for m, p in ENGINE] + \
            [(m, p, side) for m, p in JACOBI for side in ("left", "right") if FIXED_SIDE.get(m, side) == side]


@pytest.mark.parametrize("shape", [SMALL, ODD], ids=["small", "odd"])
@pytest.mark.parametrize("method,param,side", GPU_CASES, ids=[f"{_mid(m, p)}-{s}" for m, p, s in GPU_CASES])
def test_the_oracle_lies_within_the_pins(env, shape, method, param, side):
    """Every case of the GPU tests: its tolerances at or below their caps (1e-12 for the floor rule at history[1],
    TOL_CAP for the measured ones -- asserted as Pins is built), and both oracle variants inside them."""
    oracle, _ = env
    g, b, fs, bases = _gpu_case(env, shape)
    pins = er.Pins(oracle, g, shape, b, method, param, side, fs=fs, basis=bases[side is not None])
    for variant, hist in pins.oracle.items():
        pins.check(list(hist), f"{_mid(method, param)} {side} {variant}")


@pytest.mark.parametrize("shape", [SMALL, ODD], ids=["small", "odd"])
def test_tfqmr1_meets_cgs_on_these_data(env, shape):
    """On these data TFQMR1's minimum takes the omega after the second half-step -- CGS's residual -- in both
    iterations pinned: a cross-pin that holds for this b (shown here), not in general."""
    _, _, _, bases = _gpu_case(env, shape)
    sp = er.Space(bases[False])
    assert er.tfqmr(sp, 2, l1=True).hist_sq == er.cgs(sp, 2).hist_sq


@pytest.mark.parametrize("method,param", [("cgs", None), ("tfqmr", None), ("bicgstabl", 2)],
                         ids=["cgs", "tfqmr", "bicgstabl2"])
def test_a_defect_at_iteration_2_is_far_outside_the_tolerance(env, method, param):
    """What the later pins are for: at history[2] on SMALL, each of one dropped row in one dot of the second
    iteration, a beta formed from the previous pass's rho alone (the register read before this pass writes it), and
    r~ replaced by r moves the exact value by more than 100 times its tolerance."""
    oracle, _ = env
    g, b, fs, bases = _gpu_case(env, SMALL)
    pins = er.Pins(oracle, g, SMALL, b, method, param, fs=fs, basis=bases[False])
    tol, exact = pins.tol[2], pins.exact[2]

    def run(K, defect=None, drop_at=None):
        sp = er.Space(bases[False])
        sp.drop_at = drop_at
        if method == "bicgstabl":
            return er.bicgstab_l(sp, K, param, defect=defect), sp
        return {"cgs": er.cgs, "tfqmr": er.tfqmr}[method](sp, K, defect=defect), sp

    assert run(2)[0].history[2] == exact
    _, first = run(1)  # (first.ndots: the dots of the first iteration)
    # the two dots that form the second iteration's coefficients: rho = <r~, r> and <r~, v> (<r~, u_2> for BiCGStab(l)).
    # (The dots of BiCGStab(l)'s MR part are not held here: the MR coefficients minimise |r_0|, so a small error in
    # them moves the norm only to second order.)
    for at in (first.ndots + 1, first.ndots + 2):
        h = run(2, drop_at=at)[0].history[2]
        assert abs(h - exact) > 100 * tol * exact, ("dropped row", at, h, exact, tol)
    for defect in ("stale_beta", "shadow_r"):
        h = run(2, defect=defect)[0].history[2]
        assert abs(h - exact) > 100 * tol * exact, (defect, h, exact, tol)


# ---- the vector statements -------------------------------------------------------------------------------------------

F = Fraction


def _brute_multi(coefs):
    return lambda v: [v[0][i] + sum(F(c) * x[i] for c, x in zip(coefs, v[1:])) for i in range(len(v[0]))]


def _each(f):
    return lambda v: [f(*row) for row in zip(*v)]


# every statement of the integer model restated on Fractions, element by element, from the header's formula
BRUTE = {
    "fill": _each(lambda y: F(er.I_FILL)),
    "copy": _each(lambda y, x: x),
    "scale": _each(lambda y: y * F(er.I_SCALE)),
    "div_scalar": _each(lambda y: y / F(er.I_DIV)),
    "scaled_copy": _each(lambda y, x: F(er.I_A1) * x),
    "axpy": _each(lambda y, x: y + F(er.I_AXPY) * x),
    "xpay": _each(lambda y, x: x + F(er.I_XPAY) * y),
    "axpbz": _each(lambda y, x, z: F(er.I_A) * x + F(er.I_B) * z),
    "lin3": _each(lambda y, r, x, z: r + F(er.I_S) * (F(er.I_A) * x + F(er.I_B) * z)),
    "bicgstab_p": _each(lambda p, r, v: r + F(er.I_BETA) * (p - F(er.I_OMEGA) * v)),
    "vmul_add": _each(lambda y, a, b: y + F(er.I_VS) * (a * b)),
    "vmul": _each(lambda y, a, b: a * b),
    "vdiv": _each(lambda y, a, b: F(er.I_VD) * a / b),
    "vdiv_scalar": _each(lambda y, b: F(er.I_VD) / b),
    "map": _each(lambda y, x0, x1: F(er.MAP_CONSTS[0]) * x0 + x1 * y),
}
for _k in er.MULTI_KS:
    BRUTE[f"multi_axpy{_k}"] = _brute_multi(er.multi_coefs_int(_k))


def _fractions(vecs):
    return [[F(int(e)) for e in v] for v in vecs]


def test_every_statement_has_both_models_and_a_brute_force():
    assert set(BRUTE) == set(er.INT_STATEMENTS) == set(er.REAL_STATEMENTS)


@pytest.mark.parametrize("name", sorted(er.INT_STATEMENTS))
def test_integer_statement_model_matches_fractions(name):
    for n in (1, 2, 7, 64):
        maps = [tuple(range(er.INT_STATEMENTS[name][0]))] + er.ALIASINGS.get(name, [])
        for amap in maps:
            vecs = er.aliased_operands(name, n, amap, seed=n)
            got = er.int_result(name, vecs)
            exact = BRUTE[name](_fractions(vecs))
            assert got.dtype == np.float64 and [F(float(g)) for g in got] == exact, (name, n, amap)
            assert not np.any(got == er.SENTINEL)


def test_integer_model_refuses_data_that_could_round():
    big = np.full(4, 1 << 40, np.int64)
    with pytest.raises(AssertionError):
        er.int_result("vmul", [big, big, big])  # 2^80
    with pytest.raises(AssertionError):
        er.int_axpbz(0.3, np.array([3]), 1, np.array([1]))  # fl(0.3) is k / 2^54: its multiples need more than 53 bits
    with pytest.raises(AssertionError):
        er.Dyadic(np.array([3])).over_pow2(np.array([6]))
    top = np.full(4, (1 << 52) + 1, np.int64)
    with pytest.raises(AssertionError):
        er.int_axpbz(1, top, 1, top)  # the sum reaches 2^53


def test_integer_model_signs_its_zeros_as_ieee_does():
    """(-0.25) * 0 is -0, (-0) + (+0) is +0, (-0) + (-0) is -0: whatever a kernel fuses, the products are exact and the
    zero's sign is the same -- the model must give it, bit for bit."""
    x = np.array([0, 0, 5, -5, 0, 3], np.int64)
    z = np.array([0, 7, 0, 0, -2, 3], np.int64)
    xf, zf = x.astype(np.float64), z.astype(np.float64)
    for a, b in ((-0.25, 3.0), (-0.25, -0.5), (0.5, -3.0), (2.0, 0.5)):
        assert er.same_bits(er.int_axpbz(a, x, b, z).value(), a * xf + b * zf), (a, b)
        assert er.same_bits((er.Dyadic.of(a) * er.Dyadic(x)).value(), a * xf)
        assert er.same_bits((er.Dyadic(x) * er.Dyadic(z)).value(), xf * zf)
        assert er.same_bits(er.int_lin3(z, a, b, x, a, z).value(), zf + a * (b * xf + a * zf))
        assert er.same_bits((er.Dyadic.of(a) * er.Dyadic(x)).over_pow2(np.array([1, 2, 4, 8, 1, 2])).value(),
                            a * xf / np.array([1.0, 2.0, 4.0, 8.0, 1.0, 2.0]))
    assert np.signbit(er.int_result("scale", [x])).tolist() == [True, True, True, False, True, True]


def test_statement_vectors_depend_on_the_row():
    v = er.stmt_vector(12345, 3)
    for shift in (1, 2, 256, 2048):
        assert not np.array_equal(v[shift:], v[:-shift])
    assert not np.array_equal(v[:2048], v[2048:4096])


def test_fma_is_the_exactly_rounded_sum():
    rng = np.random.default_rng(5)
    for _ in range(3000):
        a, x, t = (rng.standard_normal(3) * 10.0 ** rng.integers(-4, 5, 3)).tolist()
        assert er.fma(a, x, t) == float(F(a) * F(x) + F(t))
    big, tiny, inf = 1.7976931348623157e308, 5e-324, math.inf
    assert er.fma(big, 2.0, -big) == big  # no overflow where fl(a x) overflows
    assert er.fma(big, 2.0, 0.0) == inf and er.fma(-big, 2.0, 0.0) == -inf
    assert er.fma(big, 2.0, -inf) == -inf and math.isnan(er.fma(inf, 0.0, 1.0)) and math.isnan(er.fma(inf, 1.0, -inf))
    assert er.fma(tiny, 0.5, 0.0) == 0.0 and er.fma(tiny, 0.75, 0.0) == tiny  # ties to even; subnormal results
    assert math.copysign(1.0, er.fma(-1.0, 0.0, 0.0)) == 1.0 and math.copysign(1.0, er.fma(-1.0, 0.0, -0.0)) == -1.0


def test_unfused_forms_are_one_rounding_per_operation():
    """numpy's a * x + b * z against Fractions rounded after every operation, and the single-form statements."""
    rnd = lambda q: float(q)  # noqa: E731
    (y, x, z), forms = er.real_operands("axpbz", 2049)
    want = [rnd(F(rnd(F(er.R_A) * F(xi))) + F(rnd(F(er.R_B) * F(zi)))) for xi, zi in zip(x[:300].tolist(), z[:300].tolist())]
    assert forms["none"][:300].tolist() == want
    (y,), forms = er.real_operands("div_scalar", 2049)
    assert forms["exact"][:300].tolist() == [rnd(F(yi) / F(er.R_DIV)) for yi in y[:300].tolist()]
    (y, a, b), forms = er.real_operands("vdiv", 2049)
    assert forms["exact"][:300].tolist() == [rnd(F(rnd(F(er.R_VD) * F(ai))) / F(bi)) for ai, bi in zip(a[:300].tolist(), b[:300].tolist())]


@pytest.mark.parametrize("name", sorted(er.REAL_STATEMENTS))
def test_rounding_forms_are_told_apart_by_the_fixtures(name):
    """The condition that makes `classify` mean something on the GPU tests' own data: every two admissible forms of a
    statement differ on at least 1 % of the rows, and on the LAST row of every odd-length fixture (the kernels' scalar
    tail).  Without it a result could "identify" a form by accident."""
    for n in er.real_rows(name):
        vecs, forms = er.real_operands(name, n)
        assert all(v.shape == (n,) for v in forms.values())
        for (p, q), share in er.differing_share(forms).items():
            assert share >= 0.01, (name, n, p, q, share)
            if n & 1:
                assert er.bits(forms[p])[-1] != er.bits(forms[q])[-1], (name, n, p, q)
        for p in forms:
            assert er.classify(forms[p], forms) == [p]


def test_form_lists_are_the_admissible_evaluations():
    assert list(er.real_operands("axpbz", 3)[1]) == ["none", "fuse_x", "fuse_z"]
    assert list(er.real_operands("axpy", 3)[1]) == ["none", "fuse_x"]  # (b = 1: fuse_z is `none` by construction)
    assert list(er.real_operands("xpay", 3)[1]) == ["none", "fuse_z"]
    assert sorted(er.real_operands("lin3", 3)[1]) == sorted(f"{i}/{o}" for i in ("none", "fuse_x", "fuse_z") for o in ("none", "fused"))
    assert sorted(er.real_operands("bicgstab_p", 3)[1]) == sorted(f"{i}/{o}" for i in ("none", "fuse_z") for o in ("none", "fused"))
    assert list(er.real_operands("vmul_add", 3)[1]) == ["prod/none", "prod/fused"]
    assert list(er.real_operands("multi_axpy9", 3)[1]) == ["none", "fused"]


def _mutations(good, other, n):
    """Wrong results a kernel with a wrong bound, stride or tail would leave (n odd, more than two blocks)."""
    blk = er.STREAM_BLOCK
    m = {}
    m["dropped last row"] = good.copy()
    m["dropped last row"][-1] = er.SENTINEL
    m["shifted by one double2"] = np.concatenate([good[2:], good[:2]])
    m["block written twice"] = good.copy()
    m["block written twice"][blk:2 * blk] = good[:blk]
    m["tail from another form"] = good.copy()
    m["tail from another form"][-1] = other[-1]
    m["one ulp off"] = good.copy()
    m["one ulp off"][n // 2] = np.nextafter(good[n // 2], np.inf)
    return m


def test_mutations_are_caught():
    n = 2 * er.STREAM_BLOCK + 1
    (y, x, z), forms = er.real_operands("axpbz", 2049)
    rng = np.random.default_rng(9)
    vecs = [np.concatenate([rng.standard_normal(n - 2049), v]) for v in (y, x, z)]  # (the tuned last row stays last)
    forms = er.REAL_STATEMENTS["axpbz"][1](vecs)
    for what, bad in _mutations(forms["fuse_x"], forms["fuse_z"], n).items():
        assert er.classify(bad, forms) == [], what
    ivecs = er.int_operands("axpbz", n)
    good = er.int_result("axpbz", ivecs)
    other = er.int_result("axpbz", [ivecs[0], ivecs[2], ivecs[1]])
    assert er.same_bits(good, good.copy())
    for what, bad in _mutations(good, other, n).items():
        assert not er.same_bits(bad, good), what


def test_loop_edits_are_caught_at_the_row_counts_the_gpu_tests_use():
    """The four one-line kernel edits a test of the streaming kernels must catch, on the model of their loop
    (er.loop_model) and on the GPU tests' own row counts and comparisons -- which comparison catches which:
      n2 = (n >> 1) - 1         the bitwise integer comparison, at EVERY size of two rows or more (the last pair keeps the
                                sentinel, or the old value of a target the statement reads);
      tail guard bx == 1        the integer comparison at the odd sizes whose grid is ONE block (1, 3, 2047): with two
                                blocks or more block 1 exists and writes the tail, so 2049, 4097, 12345 and the odd
                                2^26-class sizes cannot see it -- which is why the small odd sizes are in the list;
      grid-stride for -> if     the integer comparison at 2^26 + 2, 2^26 + 2049 (and 2^27 + 2051, not modelled here for
                                its memory): rows of the second trip keep the sentinel.  NOT at 2^26 + 1: its one row
                                beyond the first trip is the odd tail, which block 0 writes outside the loop -- the
                                first row of the second trip is row 2^26 of a vector of 2^26 + 2, the size this model
                                added to the list;
      AxpbzF's operands swapped the form test: classify gives [fuse_z] where the table says fuse_x, for axpbz, and
                                [none] instead of [fuse_x] for axpy (y += a x); xpay's two forms swap likewise; the
                                integer comparison cannot see it, by construction."""
    caught = {m: [] for m in er.LOOP_MUTATIONS}
    for n in er.STMT_SMALL_ROWS + er.STMT_BIG_ROWS[:5]:
        # `fill` on a sentinel target (a statement that does not read its target) and `scale` (one that does)
        for result, before in ((np.full(n, er.I_FILL), np.full(n, er.SENTINEL)),) + \
                (((lambda y: (er.I_SCALE * y, y))(er.stmt_vector(n, 3).astype(np.float64)),) if n <= 12345 else ()):
            assert np.array_equal(er.loop_model(result, before), result), n
            for m in er.LOOP_MUTATIONS:
                same = np.array_equal(er.loop_model(result, before, m), result)
                if not same and n not in caught[m]:
                    caught[m].append(n)
                if n <= 12345:  # both statements agree on where the edit shows
                    assert same == (n not in caught[m]), (m, n)
    big = list(er.STMT_BIG_ROWS[:5])
    assert caught["dropped_pair"] == [n for n in er.STMT_SMALL_ROWS if n >= 2] + big
    assert caught["tail_guard_block_1"] == [1, 3, 2047]
    assert caught["one_trip"] == [(1 << 26) + 2, (1 << 26) + 2049]
    # the swapped functor: a * x0 + b * x1 fuses its FIRST product, so b * x1 + a * x0 is the form fuse_z
    for name, swapped in (("axpbz", "fuse_z"), ("axpy", "none"), ("xpay", "fuse_z")):
        for n in er.real_rows(name):
            vecs, forms = er.real_operands(name, n)
            if name == "axpbz":
                got = er.forms_axpbz(er.R_B, vecs[2], er.R_A, vecs[1])["fuse_x"]
            elif name == "axpy":
                got = er.forms_axpbz(1.0, vecs[0], er.R_AXPY, vecs[1])["none"]  # fma(1, y, fl(a x))
            else:
                got = er.forms_axpbz(er.R_XPAY, vecs[0], 1.0, vecs[1])["fuse_x"]  # fma(b, y, fl(1 x))
            assert er.classify(got, forms) == [swapped], (name, n)


# ---- GMRES(m) on the non-symmetric integer operator (exact_ref.gmres, GmresPins) ----------------------------------------

GMRES_ODD = (37, 21, 19)
DEFECTS = ["skip_q0", "skip_in_group", "drop_row", "rotation_order"]
_gmres_problems = {}


def _gmres_problem(env, shape):
    oracle, mesh = env
    if shape not in _gmres_problems:
        _gmres_problems[shape] = er.GmresProblem(oracle, mesh, shape)
    return _gmres_problems[shape]


def _rel(h, pins):
    return [abs(a - x) / x for a, x in zip(h, pins.exact)]


@pytest.mark.parametrize("shape", [(5, 4, 3), GMRES_ODD])
def test_convection_diffusion_box_is_an_integer_operator(env, shape):
    """The operator of the GMRES pins: integer face weights, row sums of |A| <= 20, |A - A^T| = 2 -- and the oracle's
    face loops, the operator the device gets and ``IntOperator`` are the same matrix, bit for bit on integers."""
    oracle, mesh = env
    p = _gmres_problem(env, shape)
    for w in p.weights:
        assert np.array_equal(w, np.rint(w))
    assert p.A.rowsum <= 20 and abs(p.A.csr - p.A.csr.T).max() == 2
    z = p.A.apply(p.b)
    assert np.array_equal(p.oracle_op("strict").apply(p.b.astype(np.float64)), z.astype(np.float64))
    assert np.array_equal(p.A.apply(p.b.astype(object)).astype(np.int64), z)
    # nu = 1, v = 0 is -L of the unit box: the Poisson chain of ``Basis`` is the same chain
    lap = er.IntOperator.from_face_weights(p.g, *mesh.convection_diffusion_weights(p.g, 1.0, (0.0, 0.0, 0.0)))
    assert np.array_equal(lap.apply(p.b), er.int_apply(shape, p.b))
    r = er.true_residual(p.A, p.b, np.zeros(p.b.size))
    assert r == math.sqrt(float(er.exact_dot(p.b, p.b)))


def test_chain_of_a_general_operator_leaves_int64_when_it_must(env):
    p = _gmres_problem(env, (5, 4, 3))
    basis = er.OpBasis(p.A, p.b)
    basis.grow(16)
    kinds = [w.dtype == object for w in basis.W]
    assert not any(kinds[:13]) and kinds[-1] and kinds == sorted(kinds)
    w = basis.W[0].astype(object)
    for t in range(1, 17):
        w = p.A.apply(w)
        assert [int(v) for v in basis.W[t]] == list(w), t


@pytest.mark.parametrize("m", [3, 7])
def test_gmres_coefficient_form_against_a_brute_force(env, m):
    """``gmres`` on coefficient columns over the chain of the non-symmetric operator against ``gmres`` with every
    element a PREC-digit decimal: history and x_K to 1e-60, through restarts (m = 3: two inner_finalize and the exit
    inside the third cycle) and without (m = 7)."""
    from decimal import localcontext

    p = _gmres_problem(env, (5, 4, 3))
    sp = er.Space(er.OpBasis(p.A, p.b), decimal=True)
    el = er.ElemSpace(None, p.b, decimal=True, op=p.A)
    coef, brute = er.gmres(sp, 7, m), er.gmres(el, 7, m)
    assert len(coef.hist_sq) == len(brute.hist_sq) == 8
    with localcontext() as ctx:
        ctx.prec = er.PREC
        tiny = er._dec(Fraction(1, 10 ** 60))
        for c, e in zip(coef.hist_sq, brute.hist_sq):
            assert abs(c - e) <= abs(e) * tiny
        xc = sum((er._dec(c) * sp.basis.W[k].astype(object) for k, c in coef.x.c.items()), np.zeros(p.b.size, dtype=object))
        assert max(abs(a - e) for a, e in zip(xc, brute.x)) <= max(abs(v) for v in brute.x) * tiny
        # x is the solver's: the true residual of the exact x is the last history entry
        r = p.b.astype(object) - p.A.apply(brute.x)
        assert abs(sum(v * v for v in r) - brute.hist_sq[7]) <= brute.hist_sq[7] * tiny


@pytest.mark.parametrize("shape", list(er.GMRES_CASES), ids=lambda s: "x".join(map(str, s)))
def test_gmres_pins_of_every_gpu_case(env, shape):
    """Every case of tests/test_gpu_exact_gmres.py: the precision guard (PREC against 2 PREC digits) and the cap
    (tol_k, tol_res, tol_x <= TOL_CAP) are asserted as ``GmresPins`` is built; both oracle builds lie inside."""
    p = _gmres_problem(env, shape)
    for K, m in er.GMRES_CASES[shape]:
        pins = p.pins(K, m)
        assert pins.tol[0] is None and max(pins.tol[1:]) <= er.TOL_CAP and pins.tol_res <= er.TOL_CAP
        assert (pins.x is not None) == (p.b.size <= er.GMRES_X_ROWS)
        for variant, hist in pins.oracle.items():
            pins.check(list(hist), f"gmres({m}) {shape} {variant}")
            pins.check_x(pins.oracle_x[variant], f"gmres({m}) {shape} {variant}")
    if p.b.size > er.GMRES_X_ROWS:
        del _gmres_problems[shape]  # (hundreds of MB of chain that no other test here needs)


def test_gmres_pins_refuse_more_steps_than_the_power_basis_carries(env):
    p = _gmres_problem(env, (5, 4, 3))
    with pytest.raises(AssertionError):
        er.GmresPins(p.oracle, p.oracle_op, p.basis, p.A, p.b, 13, 13)
    from decimal import InvalidOperation, localcontext

    # ... and what the guard is for: with too few digits the K = 12 history is not the 80-digit one to 1e-40 (or a
    # squared norm comes out negative)
    sp = er.Space(er.OpBasis(p.A, p.b), decimal=True)
    fine = er.gmres(sp, 12, 12)
    for digits in (12, 30):
        try:
            coarse = er.gmres(sp, 12, 12, prec=digits)
            with localcontext() as ctx:
                ctx.prec = er.PREC
                lost = abs(coarse.hist_sq[12] - fine.hist_sq[12]) > abs(fine.hist_sq[12]) * er._dec(Fraction(1, 10 ** 40))
        except InvalidOperation:
            lost = True
        assert lost, digits


@pytest.mark.parametrize("defect", DEFECTS)
def test_gmres_defects_fall_outside_the_pins(env, defect):
    """What the pins are for, on 37 x 21 x 19 with K = m = 9: a float64 restatement of the Gram-Schmidt step with one
    defect -- the projection on q_0 dropped from the third step on; one projection of a group of four dropped; one
    dot without its last row; the earlier rotations in the wrong order -- leaves the pins at some k by a factor of
    1000 or more.  The same restatement without a defect lies inside (the grouped test below, T = 1)."""
    p = _gmres_problem(env, GMRES_ODD)
    pins = p.pins(9, 9)
    h = er.mgs_float64(p.A.float64(), p.b, 9, 9, defect=defect)
    out = [d / t for d, t in zip(_rel(h, pins)[1:], pins.tol[1:])]
    assert max(out) >= 1e3, (defect, out)
    with pytest.raises(AssertionError):
        pins.check(list(h), defect)


def test_poisson_cannot_see_a_dropped_old_projection(env):
    """Why the operator had to change.  On the symmetric Poisson box H is tridiagonal: the projections on
    q_0 ... q_{k-2} are rounding noise, and GMRES with the projection on q_0 dropped for k >= 2 stays inside Poisson's
    own pins -- the same defect that leaves the convection-diffusion pins by a factor of 1e3 (above)."""
    oracle, mesh = env
    g = er.unit_box(mesh, *GMRES_ODD)
    b = er.int_vector(g.n_cells, er.GMRES_SEED, *er.GMRES_RANGE)
    lap = er.IntOperator.from_face_weights(g, *mesh.convection_diffusion_weights(g, 1.0, (0.0, 0.0, 0.0)))
    assert np.array_equal(lap.apply(b), er.int_apply(GMRES_ODD, b))
    pins = er.GmresPins(oracle, lambda v: oracle.StencilOperator(g, -1.0, 0.0, variant=v), er.Basis(GMRES_ODD, b), lap, b,
                        9, 9)
    good = er.mgs_float64(lap.float64(), b, 9, 9)
    bad = er.mgs_float64(lap.float64(), b, 9, 9, defect="skip_q0")
    pins.check(list(good), "poisson")
    pins.check(list(bad), "poisson, q_0 skipped")  # invisible
    assert max(_rel(bad, pins)) < 1e-13


@pytest.mark.parametrize("T", [1, 2, 3, 4])
def test_grouped_gram_schmidt_is_no_defect(env, T):
    """The chain kernels take T projections per synchronisation point: the T dots of a group against the w from
    before the group, regrouped by bilinearity (``mgs_float64``).  In fp64 that form stays within 1e-14 of the exact
    history on 37 x 21 x 19 -- inside the pins, and no further from the exact value than the plain form (T = 1)."""
    p = _gmres_problem(env, GMRES_ODD)
    for K, m in er.GMRES_CASES[GMRES_ODD]:
        pins = p.pins(K, m)
        h = er.mgs_float64(p.A.float64(), p.b, K, m, group=T)
        pins.check(list(h), f"grouped T={T}")
        assert max(_rel(h, pins)) <= 1e-14, _rel(h, pins)


# ---- CG and BiCGStab past their first step (exact_ref.cg, bicgstab, StepPins) ---------------------------------------------

_step_problems = {}
STEP_METHODS = {"cg": er.cg, "bicgstab": er.bicgstab, "cg2": er.cg}
STEP_DEFECTS = [("cg", d) for d in er.CG_DEFECTS] + [("bicgstab", d) for d in er.BICGSTAB_DEFECTS]


def _step_problem(env, shape, kind="poisson", seed=er.STEP_SEED):
    oracle, mesh = env
    key = (shape, kind, seed)
    if key not in _step_problems:
        _step_problems[key] = er.StepProblem(oracle, mesh, shape, kind, seed)
    return _step_problems[key]


@pytest.mark.parametrize("defect", [None, "all"])
@pytest.mark.parametrize("method", ["cg", "bicgstab", "cg2"])
def test_step_coefficient_form_against_a_brute_force(env, method, defect):
    """``cg``, ``bicgstab`` and CG on the two-stage space on coefficient columns over the chain against the same
    statements with every element a Fraction, on 4 x 3 x 3: the same history, the same x_k for every k and the same
    own-term ratios, exactly -- without a defect and with each of the defects the separation tests inject."""
    oracle, mesh = env
    shape, K = (4, 3, 3), {"cg": 5, "bicgstab": 4, "cg2": 3}[method]
    b = er.int_vector(36, 7)
    A = er.poisson_operator(mesh, er.unit_box(mesh, *shape))
    assert np.array_equal(A.apply(b), er.int_apply(shape, b))
    if method == "cg2":
        A2 = er.two_stage_operator(A)
        z = er.int_apply(shape, b)
        assert np.array_equal(A2.apply(b), b + 2 * z + er.int_apply(shape, z))  # (I + A)^2
        assert abs(A2.csr - A2.csr.T).max() == 0
    names = [None] if defect is None else list(er.BICGSTAB_DEFECTS if method == "bicgstab" else er.CG_DEFECTS)
    for name in names:
        sp = (er.TwoStageSpace if method == "cg2" else er.Space)(er.Basis(shape, b))
        el = er.ElemSpace(None, b, op=A2) if method == "cg2" else er.ElemSpace(shape, b)
        coef, brute = (STEP_METHODS[method](s, K, defect=name) for s in (sp, el))
        assert coef.hist_sq == brute.hist_sq and len(coef.hist_sq) == K + 1, name
        assert coef.ratio_sq == brute.ratio_sq, name
        for k in range(K + 1):
            want = np.array([float(v) for v in brute.xs[k]]) if k else np.zeros(36)
            assert np.array_equal(sp.materialize(coef.xs[k]) if k else np.zeros(36), want), (name, k)
        if name is None:  # x_k is the solver's: its true residual is history[k]
            for k in range(1, K + 1):
                r = b.astype(object) - el.A(brute.xs[k])
                assert sum(v * v for v in r) == brute.hist_sq[k], k


def _step_cases():
    out = [(m, shape, kind, er.STEP_SEED, er.STEP_K[m]) for m, cases in er.STEP_CASES.items() for shape, kind in cases]
    out += [(m, shape, "poisson", er.STEP_SEED, er.STEP_RANK_K) for m in ("cg", "bicgstab") for shape in er.STEP_RANK_SHAPES]
    out += [("cg", SMALL, "poisson", seed, er.STEP_K["cg"]) for seed in er.STEP_BLOCK_SEEDS[1:]]
    return out


@pytest.mark.parametrize("case", _step_cases(), ids=lambda c: f"{c[0]}-{'x'.join(map(str, c[1]))}-{c[2]}-seed{c[3]}-K{c[4]}")
def test_step_pins_of_every_gpu_case(env, case):
    """Every (method, shape) the GPU tests pin -- tests/test_gpu_exact_steps.py, the K = 4 runs of the rank test, the
    K = 8 columns of the block CG: every cap (tol_k, tol_res and tol_x at K and at the early exit's iteration <=
    TOL_CAP) is asserted as the pins are built; history[0] is bitwise; both oracle builds lie inside, history and x.
    Prints the host time of the reference per shape (NOTES.md)."""
    import time

    method, shape, kind, seed, K = case
    t0 = time.perf_counter()
    p = _step_problem(env, shape, kind, seed)
    pins = p.pins(method, K)
    t1 = time.perf_counter()
    assert pins.K == K and pins.tol[0] is None and max(pins.tol[1:]) <= er.TOL_CAP
    for k in sorted({K, min(K, er.STEP_STOP)}):
        e_res, tol_res, rule, e_x, tol_x = pins.x_tolerances(k)
        assert tol_res <= er.TOL_CAP and (tol_x is None) == (p.b.size > er.GMRES_X_ROWS)
        assert tol_x is None or tol_x <= er.TOL_CAP
        for variant in pins.oracle:
            pins.check_x(pins.oracle_x(variant, k), k, f"{method} {shape} {variant}")
        if k < K:
            assert pins.stop_between(k) > 0
    for variant, hist in pins.oracle.items():
        # (history[1] under the closed form's tolerance is a pin for a fold of depth ~65: the oracle adds n terms in a
        #  chain and on 4 M rows lies 1.6e-14 from the exact value, outside it; it is held to the other entries)
        assert hist[0] == pins.exact[0]
        for j in range(1, K + 1):
            if pins.rule[j] != "closed form":
                assert er.close(hist[j], pins.exact[j], pins.tol[j]), (method, shape, variant, j, hist[j], pins.exact[j])
        assert [j for j in range(K + 1) if pins.rule[j] == "closed form"] in ([], [1])
    print(f"step pins {method} {shape} {kind} K={K}: reference {t1 - t0:.1f} s, x checks {time.perf_counter() - t1:.1f} s; "
          f"largest tol_k {max(pins.tol[1:]):.1e} ({pins.rule[1 + int(np.argmax(pins.tol[1:]))]}), largest floor "
          f"{max(pins.floor):.1e}, tol_res {pins.x_tolerances(K)[1]:.1e} ({pins.x_tolerances(K)[2]})")
    if p.b.size > (1 << 20):
        _step_problems.clear()  # (gigabytes of chain and operator that no other test here needs)


def _defect_runs(env, method):
    p = _step_problem(env, ODD)
    pins = p.pins(method)
    f64 = er.cg_float64 if method == "cg" else er.bicgstab_float64
    return p, pins, f64, f64(p.A.float64(), p.b, pins.K)


@pytest.mark.parametrize("method", ["cg", "bicgstab"])
def test_clean_float64_restatement_lies_within_the_step_pins(env, method):
    p, pins, f64, (h, xs) = _defect_runs(env, method)
    pins.check(list(h), method)
    for k in (er.STEP_STOP, pins.K):
        pins.check_x(xs[k], k, method)
    if method == "bicgstab":  # ... and on the non-symmetric box
        q = _step_problem(env, (40, 30, 17), "convdiff")
        h, xs = er.bicgstab_float64(q.A.float64(), q.b, 5)
        q.pins("bicgstab").check(list(h), "convdiff")
        q.pins("bicgstab").check_x(xs[5], 5, "convdiff")


@pytest.mark.parametrize("method,defect", STEP_DEFECTS, ids=[f"{m}-{d}" for m, d in STEP_DEFECTS])
def test_step_defects_fall_outside_the_pins_and_are_invisible_to_the_first_step(env, method, defect):
    """What the pins are for, on 37 x 21 x 19: the float64 restatement with one defect leaves history[0], history[1]
    and x_1 BITWISE what the clean restatement gives -- the quantities of tests/test_gpu_exact_first_step.py cannot see
    it -- and falls outside the pins of history[2..K] or of x_K.  Prints error / tolerance, the larger of the history's
    and the residual's (NOTES.md records them); every one must be 100 or more."""
    p, pins, f64, (h0, xs0) = _defect_runs(env, method)
    K = pins.K
    h, xs = f64(p.A.float64(), p.b, K, defect=defect)
    assert np.array_equal(h[:2], h0[:2]) and np.array_equal(xs[1], xs0[1]), defect
    by_history = max(abs(h[k] - pins.exact[k]) / (pins.exact[k] * pins.tol[k]) for k in range(2, K + 1))
    res = er.true_residual(p.A, p.b, xs[K])
    by_x = abs(res - pins.exact[K]) / (pins.exact[K] * pins.x_tolerances(K)[1])
    print(f"step defect {method} {defect}: error / tolerance {by_history:.1e} (history) {by_x:.1e} (x_K)")
    assert max(by_history, by_x) >= 100, (defect, by_history, by_x)
    rejected = 0
    for check in (lambda: pins.check(list(h), defect), lambda: pins.check_x(xs[K], K, defect)):
        try:
            check()
        except AssertionError:
            rejected += 1
    assert rejected >= 1, defect
    if defect in ("skip_x", "double_x", "skip_x_omega"):
        assert by_history < 1 and by_x >= 100  # the history cannot see x: only check_x holds these


def test_a_dropped_row_in_the_exact_form(env):
    """``Space.drop_at`` through ``cg``: the last row left out of <r, r> at the second iteration moves the exact
    history[2] by about r_n^2 / (2 <r, r>) -- many orders above tol_2 -- and leaves history[0..1] alone."""
    p = _step_problem(env, ODD)
    pins = p.pins("cg")
    run = er.cg(er.Space(p.basis), 3, defect="drop_row")
    assert run.hist_sq[:2] == pins.run.hist_sq[:2] and run.history[2] != pins.exact[2]
    assert abs(run.history[2] - pins.exact[2]) > 100 * pins.tol[2] * pins.exact[2]


# ---- the z-periodic boxes: integer operators with a halo (exact_ref.periodic_box, tests/test_gpu_exact_rccl.py) ------------

PERIODIC_TINY = (5, 4, 3)
# (method, defect, box): CG on the symmetric operator, BiCGStab on both
HALO_DEFECTS = [("cg", d, "periodic") for d in er.CG_HALO_DEFECTS] + \
    [("bicgstab", d, kind) for d in er.BICGSTAB_HALO_DEFECTS for kind in er.PERIODIC_KINDS]


def test_periodic_local_graph_without_lengths_is_what_it_was():
    """``mesh.periodic_z_local_graph(8, 8, 8)`` returns, array for array and bit for bit, what it returned before it took
    ``lengths`` (tests/golden/periodic_z_local_graph_8x8x8.npz: the arrays of that version)."""
    import os

    from stormruler_amd import mesh

    want = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "periodic_z_local_graph_8x8x8.npz"))
    loc, send_idx = mesh.periodic_z_local_graph(8, 8, 8)
    assert [loc.n_cells, loc.dim, loc.n_halo] == list(want["counts"])
    for name in ("inner", "outer", "area", "center", "volume", "b_cell", "b_area", "b_center", "global_id", "halo_owner"):
        got = getattr(loc, name)
        assert got.dtype == want[name].dtype and got.shape == want[name].shape and got.tobytes() == want[name].tobytes(), name
    assert send_idx.dtype == want["send_idx"].dtype and np.array_equal(send_idx, want["send_idx"])


def test_periodic_local_graph_with_lengths():
    """With ``lengths`` the graph is ``structured_box(..., lengths=...)`` without its z walls, the images of planes nz - 1
    and 0 shifted by -Lz and +Lz and the seam faces with the area of a z face."""
    from stormruler_amd import mesh

    nx, ny, nz = 6, 4, 5
    lengths = (3.0, 8.0, 10.0)
    loc, send_idx = mesh.periodic_z_local_graph(nx, ny, nz, lengths=lengths)
    g = mesh.structured_box(nx, ny, nz, lengths=lengths)
    P, N = nx * ny, nx * ny * nz
    assert loc.n_cells == N and loc.n_halo == 2 * P and loc.n_faces == g.n_faces + 2 * P
    assert loc.n_bfaces == g.n_bfaces - 2 * P and not np.any(np.isin(loc.b_center[:, 2], (0.0, lengths[2])))
    assert np.array_equal(np.sort(loc.b_cell), np.sort(g.b_cell[(g.b_center[:, 2] != 0.0) & (g.b_center[:, 2] != lengths[2])]))
    assert np.array_equal(loc.center[:N], g.center) and np.array_equal(loc.global_id[N:], send_idx)
    assert np.array_equal(loc.center[N:N + P], g.center[N - P:] - [0.0, 0.0, lengths[2]])
    assert np.array_equal(loc.center[N + P:], g.center[:P] + [0.0, 0.0, lengths[2]])
    assert np.all(loc.area[g.n_faces:] == (lengths[0] / nx) * (lengths[1] / ny))
    d = loc.center[loc.outer[g.n_faces:]] - loc.center[loc.inner[g.n_faces:]]
    assert np.allclose(d, [0.0, 0.0, lengths[2] / nz], rtol=0, atol=1e-14)


@pytest.mark.parametrize("kind", er.PERIODIC_KINDS)
@pytest.mark.parametrize("shape", [PERIODIC_TINY, er.PERIODIC_G], ids=lambda s: "x".join(map(str, s)))
def test_periodic_box_is_the_oracle_operator_on_the_local_graph(env, shape, kind):
    """``IntOperator.from_local_graph`` -- the halo columns folded onto the owned cells they are images of -- equals the
    oracle's face loops over the local graph with the halo filled, strict and fma, bit for bit on an integer vector.
    Every weight is an integer; -L is symmetric with diagonal 6 ... 8 and off-diagonals -1; the convection-diffusion
    operator has max|A - A^T| = 2 and row sums of |A| of at most 20."""
    oracle, mesh = env
    vel = er.GMRES_VEL if kind == "periodic_convdiff" else None
    loc, send_idx, w, A = er.periodic_box(mesh, *shape, vel=vel)
    n = loc.n_cells
    assert n == shape[0] * shape[1] * shape[2] and loc.n_halo == 2 * shape[0] * shape[1] and A.n == n
    for v in w:
        assert np.array_equal(v, np.rint(v))
    b = er.int_vector(n, er.GMRES_SEED, *er.GMRES_RANGE)
    z = A.apply(b)
    assert np.array_equal(A.apply(b.astype(object)).astype(np.int64), z)
    for variant in ("strict", "fma"):
        kw = {} if vel is None else dict(conv=1.0, vel=vel)
        full = oracle.StencilOperator(loc, -1.0, 0.0, variant=variant, **kw).apply(np.concatenate([b, b[send_idx]]).astype(np.float64))
        assert np.array_equal(full[:n], z.astype(np.float64)), variant
    asym = abs(A.csr - A.csr.T).max()
    if vel is None:
        off = A.csr - __import__("scipy.sparse").sparse.diags(A.csr.diagonal())
        assert asym == 0 and A.rowsum <= 12 and set(A.csr.diagonal()) <= {6, 7, 8} and set(off.data) == {-1}
        # (no wall in z: a cell away from the x and y walls has all six neighbours, the two across the seam included)
        assert set(np.diff(A.csr.indptr)) == {5, 6, 7} and np.array_equal(np.diff(A.csr.indptr) - 1, 12 - A.csr.diagonal())
    else:
        assert asym == 2 and A.rowsum <= 20
    with pytest.raises(AssertionError):
        er.IntOperator.from_face_weights(loc, *w)  # (a graph with a halo is not its business)
    # the split along the seam: two planes of rows, one entry each, and nothing lost
    a_in, a_h = A.seam_split(shape)
    assert abs(a_in + a_h - A.float64()).max() == 0 and a_h.nnz == loc.n_halo
    assert set(np.flatnonzero(np.diff(a_h.indptr))) == set(send_idx)


@pytest.mark.parametrize("method,kind", [("cg", "periodic"), ("bicgstab", "periodic"), ("bicgstab", "periodic_convdiff")])
def test_step_coefficient_form_on_the_periodic_boxes_against_a_brute_force(env, method, kind):
    """``cg`` and ``bicgstab`` on coefficient columns over ``OpBasis`` of the periodic operators against the same
    statements with every element a Fraction (``ElemSpace(op=...)``) on 5 x 4 x 3: the same history, x_k and own-term
    ratios, exactly."""
    oracle, mesh = env
    p = _step_problem(env, PERIODIC_TINY, kind)
    K = {"cg": 5, "bicgstab": 4}[method]
    sp, el = er.Space(er.OpBasis(p.A, p.b)), er.ElemSpace(None, p.b, op=p.A)
    coef, brute = (STEP_METHODS[method](s, K) for s in (sp, el))
    assert coef.hist_sq == brute.hist_sq and len(coef.hist_sq) == K + 1
    assert coef.ratio_sq == brute.ratio_sq
    for k in range(1, K + 1):
        assert np.array_equal(sp.materialize(coef.xs[k]), np.array([float(v) for v in brute.xs[k]])), k
        r = p.b.astype(object) - el.A(brute.xs[k])
        assert sum(v * v for v in r) == brute.hist_sq[k], k


@pytest.mark.parametrize("m", [3, 7])
def test_gmres_coefficient_form_on_the_periodic_box_against_a_brute_force(env, m):
    """``gmres`` over ``OpBasis`` of the periodic convection-diffusion operator against PREC-digit decimals per element
    on 5 x 4 x 3: history and x_K to 1e-60, with restarts (m = 3) and without (m = 7)."""
    from decimal import localcontext

    oracle, mesh = env
    p = er.GmresProblem(oracle, mesh, PERIODIC_TINY, "periodic_convdiff")
    sp = er.Space(er.OpBasis(p.A, p.b), decimal=True)
    el = er.ElemSpace(None, p.b, decimal=True, op=p.A)
    coef, brute = er.gmres(sp, 7, m), er.gmres(el, 7, m)
    assert len(coef.hist_sq) == len(brute.hist_sq) == 8
    with localcontext() as ctx:
        ctx.prec = er.PREC
        tiny = er._dec(Fraction(1, 10 ** 60))
        for c, e in zip(coef.hist_sq, brute.hist_sq):
            assert abs(c - e) <= abs(e) * tiny
        xc = sum((er._dec(c) * sp.basis.W[k].astype(object) for k, c in coef.x.c.items()), np.zeros(p.b.size, dtype=object))
        assert max(abs(a - e) for a, e in zip(xc, brute.x)) <= max(abs(v) for v in brute.x) * tiny
        r = p.b.astype(object) - p.A.apply(brute.x)
        assert abs(sum(v * v for v in r) - brute.hist_sq[7]) <= brute.hist_sq[7] * tiny


def _periodic_cases():
    return [(m, shape, kind) for m, cases in er.PERIODIC_STEP_CASES.items() for shape, kind in cases]


@pytest.mark.parametrize("case", _periodic_cases(), ids=lambda c: f"{c[0]}-{'x'.join(map(str, c[1]))}-{c[2]}")
def test_step_pins_of_every_periodic_case(env, case):
    """Every (method, box) of tests/test_gpu_exact_rccl.py: every cap (tol_k, and tol_res and tol_x at K and at the early
    exit's iteration, <= TOL_CAP) is asserted as the pins are built, on the reference alone; history[0] is bitwise; both
    oracle builds lie inside, history and x.  x itself is compared on 20 x 12 x 9 only."""
    method, shape, kind = case
    p = _step_problem(env, shape, kind)
    pins = p.pins(method)
    K = er.STEP_K[method]
    assert pins.K == K and pins.tol[0] is None and max(pins.tol[1:]) <= er.TOL_CAP and "closed form" not in pins.rule
    for k in (er.STEP_STOP, K):
        e_res, tol_res, rule, e_x, tol_x = pins.x_tolerances(k)
        assert tol_res <= er.TOL_CAP and (tol_x is None) == (shape != er.PERIODIC_G)
        assert tol_x is None or tol_x <= er.TOL_CAP
        for variant in pins.oracle:
            pins.check_x(pins.oracle_x(variant, k), k, f"{method} {shape} {variant}")
    assert pins.stop_between(er.STEP_STOP) > 0
    for variant, hist in pins.oracle.items():
        pins.check(list(hist), f"{method} {shape} {kind} {variant}")
    print(f"periodic pins {method} {shape} {kind}: largest tol_k {max(pins.tol[1:]):.1e}, tol_res "
          f"{max(pins.x_tolerances(k)[1] for k in (er.STEP_STOP, K)):.1e}")


@pytest.mark.parametrize("shape", list(er.PERIODIC_GMRES_CASES), ids=lambda s: "x".join(map(str, s)))
def test_gmres_pins_of_every_periodic_case(env, shape):
    """The GMRES cases of tests/test_gpu_exact_rccl.py on the periodic convection-diffusion box: the precision guard and
    every cap are asserted as ``GmresPins`` is built; both oracle builds lie inside."""
    oracle, mesh = env
    p = er.GmresProblem(oracle, mesh, shape, "periodic_convdiff")
    for K, m in er.PERIODIC_GMRES_CASES[shape]:
        pins = p.pins(K, m)
        assert pins.tol[0] is None and max(pins.tol[1:]) <= er.TOL_CAP and pins.tol_res <= er.TOL_CAP
        assert (pins.x is not None) == (shape == er.PERIODIC_G)
        assert pins.x is None or pins.tol_x <= er.TOL_CAP
        for variant, hist in pins.oracle.items():
            pins.check(list(hist), f"gmres({m}) {shape} {variant}")
            pins.check_x(pins.oracle_x[variant], f"gmres({m}) {shape} {variant}")
        print(f"periodic pins gmres({m}) K={K} {shape}: largest tol_k {max(pins.tol[1:]):.1e}, tol_res {pins.tol_res:.1e}")


def _halo_runs(env, method, kind):
    p = _step_problem(env, er.PERIODIC_G, kind)
    a_in, a_h = p.A.seam_split(er.PERIODIC_G)
    f64 = er.cg_float64 if method == "cg" else er.bicgstab_float64
    return p, p.pins(method), lambda **kw: f64(a_in, p.b, er.STEP_K[method], a_halo=a_h, **kw)


@pytest.mark.parametrize("method,kind", [("cg", "periodic"), ("bicgstab", "periodic"), ("bicgstab", "periodic_convdiff")])
def test_clean_float64_restatement_with_the_split_lies_within_the_periodic_pins(env, method, kind):
    p, pins, run = _halo_runs(env, method, kind)
    h, xs = run()
    pins.check(list(h), method)
    for k in (er.STEP_STOP, pins.K):
        pins.check_x(xs[k], k, method)


@pytest.mark.parametrize("method,defect,kind", HALO_DEFECTS, ids=[f"{m}-{d}-{k}" for m, d, k in HALO_DEFECTS])
def test_halo_defects_fall_outside_the_periodic_pins(env, method, defect, kind):
    """What the pins of tests/test_gpu_exact_rccl.py are for, on 20 x 12 x 9: the float64 restatement whose HALO alone
    is wrong -- the exchange missed once (the previous direction still there), the halo rows of p' formed with the
    previous beta, those of s with the previous alpha, those of BiCGStab's p' with the omega before the last: two planes
    of one operand -- leaves history[0..1] and x_1 bitwise what the clean restatement gives and lies outside the pin of
    some history[k], k <= K, by a factor of 1000 or more (printed: |h_k - exact| / (exact tol_k), the largest over k)."""
    p, pins, run = _halo_runs(env, method, kind)
    (h0, xs0), (h, xs) = run(), run(defect=defect, at=2)
    K = pins.K
    assert np.array_equal(h[:2], h0[:2]) and np.array_equal(xs[1], xs0[1]), defect
    factor = [abs(h[k] - pins.exact[k]) / (pins.exact[k] * pins.tol[k]) for k in range(1, K + 1)]
    print(f"halo defect {method} {kind} {defect}: |h_k - exact| / (exact tol_k) = {max(factor):.1e} at k = {1 + int(np.argmax(factor))}, "
          f"first outside at k = {1 + next(i for i, f in enumerate(factor) if f > 1)}")
    assert max(factor) >= 1e3, (defect, factor)
    with pytest.raises(AssertionError):
        pins.check(list(h), defect)
    with pytest.raises(AssertionError):  # (a space without the split cannot state them)
        (er.cg_float64 if method == "cg" else er.bicgstab_float64)(p.A.float64(), p.b, K, defect=defect)


# ---- the engine's other methods past their second step (exact_ref.EnginePins, tests/test_gpu_exact_engine_steps.py) ----------

# (method, param, side, K) at the K of the table, on 4 x 3 x 3; TFQMR1 also on the tiny convection-diffusion box
ENGINE_BRUTE = sorted({(m, p, side, K) for m, p, side, _, _, K in er.ENGINE_STEP_CASES}, key=str) + \
    [("fgmres", er.ENGINE_FGMRES_M, "right", K) for _, K in er.ENGINE_FGMRES_STOPS]


def _dec_close(a, b, scale=None):
    from decimal import localcontext

    with localcontext() as ctx:
        ctx.prec = er.PREC
        return abs(er._dec(a) - er._dec(b)) <= abs(er._dec(b) if scale is None else scale) * er._dec(Fraction(1, 10 ** 60))


@pytest.mark.parametrize("method,param,side,K", ENGINE_BRUTE, ids=[f"{_mid(m, p)}-{s}-K{K}" for m, p, s, K in ENGINE_BRUTE])
def test_engine_step_coefficient_form_against_a_brute_force(env, method, param, side, K):
    """Every restatement at the K the GPU tests pin, on coefficient columns and with every element exact (Fractions; for
    IDR(s) and FGMRES PREC-digit decimals, to 1e-60): the same history, the same ``ratio_sq``, the same x_k for EVERY k,
    and the same ||b - A x_k||^2 formed from it; TFQMR1's predicates alike.  K = 6 of TFQMR1 runs on the
    convection-diffusion box 4 x 3 x 3."""
    oracle, mesh = env
    shape, n = (4, 3, 3), 36
    dec = method in er.DECIMAL_METHODS
    rng = np.random.default_rng(11)
    shadow = [rng.integers(1, 1 << 20, n) / float(1 << 21) for _ in range(3)]
    if method == "tfqmr1" and K == 6:
        g, w, A = er.convdiff_box(mesh, *shape)
        b = er.int_vector(n, er.GMRES_SEED, *er.GMRES_RANGE)
        sp, el = er.Space(er.OpBasis(A, b)), er.ElemSpace(None, b, op=A)
    else:
        b = er.int_vector(n, 7)
        dinv = 1.0 / er.int_diagonal(shape) if side else None
        sp, el = er.Space(er.Basis(shape, b, dinv), decimal=dec), er.ElemSpace(shape, b, dinv, decimal=dec)
    coef, brute = (er.exact_run(s, method, param, K, side, shadow) for s in (sp, el))
    assert len(coef.hist_sq) == len(brute.hist_sq) == len(coef.xs) == len(brute.xs) == len(coef.ratio_sq) == K + 1
    assert getattr(coef, "preds", None) == getattr(brute, "preds", None)
    from decimal import localcontext

    with localcontext() as ctx:
        ctx.prec = er.PREC
        for k in range(K + 1):
            rc, rb = sp.b() - sp.A(coef.xs[k]), el.b() - el.A(brute.xs[k])
            res_c, res_b = sp.dot(rc, rc), el.dot(rb, rb)
            if not dec:
                assert coef.hist_sq[k] == brute.hist_sq[k] and coef.ratio_sq[k] == brute.ratio_sq[k] and res_c == res_b, k
                if k:
                    assert np.array_equal(sp.materialize(coef.xs[k]), np.array([float(v) for v in brute.xs[k]])), k
                continue
            assert _dec_close(coef.hist_sq[k], brute.hist_sq[k]) and _dec_close(res_c, res_b), k
            assert _dec_close(coef.ratio_sq[k], brute.ratio_sq[k]), k
            if k:
                xc = sum((er._dec(c) * sp.basis.W[t].astype(object) for t, c in coef.xs[k].c.items()), np.zeros(n, dtype=object))
                scale = max(abs(v) for v in brute.xs[k])
                assert all(_dec_close(a, e, scale) for a, e in zip(xc, brute.xs[k])), k
    # the x a method leaves is consistent with its history wherever the history is the true residual's norm: not TFQMR's
    # bound, not the norm of P r under a left preconditioner
    if method not in ("tfqmr", "tfqmr1") and (side is None or method == "cg" or er.ENGINE_FIXED_SIDE.get(method, side) == "right"):
        with localcontext() as ctx:
            ctx.prec = er.PREC
            rb = el.b() - el.A(brute.xs[K])
            assert _dec_close(el.dot(rb, rb), brute.hist_sq[K]) if dec else el.dot(rb, rb) == brute.hist_sq[K]


_engine_problems = {}


def _engine_problem(env, shape, kind):
    oracle, mesh = env
    if (shape, kind) not in _engine_problems:
        _engine_problems[shape, kind] = er.StepProblem(oracle, mesh, shape, kind)
    return _engine_problems[shape, kind]


def _engine_cases():
    out = [c + ((c[5],),) for c in er.ENGINE_STEP_CASES]
    out += [(m, p, None, SMALL, "poisson", K, (k,)) for (m, p), (K, k) in er.ENGINE_STOPS.items()]
    out += [("fgmres", er.ENGINE_FGMRES_M, "right", shape, kind, K, (k,)) for shape, kind in er.ENGINE_STEP_BOXES
            for k, K in er.ENGINE_FGMRES_STOPS]
    return out


@pytest.mark.parametrize("case", _engine_cases(),
                         ids=lambda c: f"{_mid(c[0], c[1])}-{c[2]}-{'x'.join(map(str, c[3]))}-{c[4]}-K{c[5]}-x{c[6][0]}")
def test_engine_step_pins_of_every_gpu_case(env, case):
    """Every case of tests/test_gpu_exact_engine_steps.py on the reference alone: every cap (tol_k, and tol_res and tol_x
    at the iterations whose x is checked, <= TOL_CAP) and the decimal methods' precision guard are asserted as the pins
    are built; both oracle builds lie inside, history and x; the early exits' tolerances exist (``stop_between``)."""
    method, param, side, shape, kind, K, ks = case
    p = _engine_problem(env, shape, kind)
    pins = p.engine_pins(method, param, side, K)
    assert pins.K == K and max(t for t in pins.tol if t is not None) <= er.TOL_CAP
    assert (pins.tol[0] is None) == (side != "left" or method == "cg")  # (bitwise where r0 is b: CG's preconditioner has no side)
    for k in ks:
        e_res, tol_res, rule, e_x, tol_x = pins.x_tolerances(k)
        assert tol_res <= er.TOL_CAP and (tol_x is None) == (p.b.size > er.GMRES_X_ROWS)
        assert tol_x is None or tol_x <= er.TOL_CAP
        for variant in pins.oracle:
            pins.check_x(pins.oracle_x(variant, k), k, f"{method} {shape} {variant}")
        if k < K:
            assert pins.stop_between(k) > 0
    for variant, hist in pins.oracle.items():
        pins.check(list(hist), f"{_mid(method, param)} {side} {shape} {variant}")
    if method == "tfqmr1" and kind == "convdiff":
        assert pins.preds == [True] * 8 + [False] * 4  # both outcomes of omega < tau
    print(f"engine pins {_mid(method, param)} {side} {shape} {kind} K={K}: largest tol_k "
          f"{max(t for t in pins.tol if t is not None):.1e}, e_k {max(pins.e):.1e}, floor {max(pins.floor):.1e}, " +
          " ".join(f"e_res({k}) {pins.x_tolerances(k)[0]:.1e} tol_res({k}) {pins.x_tolerances(k)[1]:.1e}" for k in ks))


def test_tfqmr_history_is_not_the_residual_of_x(env):
    """Why ``check_x`` forms ||b - A x_k|| from ``xs[k]``: TFQMR's history is the bound tau sqrt(2 k + 1), and on
    37 x 21 x 19 at K = 4 the exact residual of x_4 is 0.5687 of it."""
    pins = _engine_problem(env, ODD, "poisson").engine_pins("tfqmr", None, None, 4)
    assert abs(pins.res_exact(4) / pins.exact[4] - 0.5687) < 1e-4


def test_idrs_history_is_not_monotone_on_the_small_box(env):
    """Why IDR(2) and IDR(4) stop elsewhere than at iteration 3 (er.ENGINE_STOPS): history[3] is above history[1]."""
    p = _engine_problem(env, SMALL, "poisson")
    for s in (2, 4):
        K, k = er.ENGINE_STOPS["idrs", s]
        pins = p.engine_pins("idrs", s, None, K)
        assert pins.exact[3] > pins.exact[1]
        with pytest.raises(AssertionError):
            pins.stop_between(3)
        assert k == next(j for j in range(2, K + 1) if pins.exact[j] * 1.05 < min(pins.exact[:j]))


# (method, param, side, shape, box, K, defect, at)
X_DEFECTS = [
    ("cgs", None, None, ODD, "poisson", 4, "skip_x", 2), ("cgs", None, None, ODD, "poisson", 4, "double_x", None),
    ("cgs", None, "right", ODD, "poisson", 3, "x_wrong_side", None),
    ("tfqmr", None, "right", ODD, "poisson", 3, "d_wrong_vector", None),
    ("tfqmr", None, None, ODD, "poisson", 4, "x_sn_for_cs", None), ("tfqmr", None, None, ODD, "poisson", 4, "d_not_scaled", None),
    ("tfqmr1", None, None, (7, 5, 3), "convdiff", 6, "copy_always", None),
    ("tfqmr1", None, None, (7, 5, 3), "convdiff", 6, "copy_never", None),
    ("bicgstabl", 2, None, ODD, "poisson", 5, "skip_x_mr", None), ("bicgstabl", 2, None, ODD, "poisson", 5, "gbb_shift", None),
    ("bicgstabl", 3, None, ODD, "poisson", 7, "gbb_shift", None),
    ("idrs", 2, None, ODD, "poisson", 6, "skip_x_omega", 3), ("idrs", 2, "right", ODD, "poisson", 3, "x_omega_wrong_side", 1),
]
HISTORY_DEFECTS = [
    ("bicgstabl", 1, None, ODD, "poisson", 3, "rho_without_omega", None),
    ("bicgstabl", 2, None, ODD, "poisson", 5, "rho_without_omega", None),
    ("bicgstabl", 1, None, ODD, "poisson", 3, "beta_without_alpha", 2),
    ("bicgstabl", 2, None, ODD, "poisson", 5, "beta_without_alpha", 2),
    ("bicgstabl", 3, None, ODD, "poisson", 7, "beta_without_alpha", 3),
    ("cgs", None, None, ODD, "poisson", 4, "stale_beta", 3), ("tfqmr", None, None, ODD, "poisson", 4, "stale_beta", 3),
]


def _defect_id(c):
    return f"{_mid(c[0], c[1])}-{c[2]}-{c[6]}" + ("" if c[7] is None else f"-at{c[7]}")


def _engine_defect(env, case):
    method, param, side, shape, kind, K, defect, at = case
    assert any(c[:6] == case[:6] for c in er.ENGINE_STEP_CASES)  # (a case the GPU tests pin)
    p = _engine_problem(env, shape, kind)
    pins = p.engine_pins(method, param, side, K)
    kw = dict(side=side, dinv=pins.dinv, shadow=pins.shadow)
    clean = er.engine_float64(p.A, p.b, method, param, K, **kw)
    bad = er.engine_float64(p.A, p.b, method, param, K, defect=defect, at=at, **kw)
    pins.check(list(clean[0]), "clean fp64"), pins.check_x(clean[1][K], K, "clean fp64")
    first = 1 if pins.tol[0] is None else 0
    by_history = max(abs(bad[0][k] - pins.exact[k]) / (pins.exact[k] * pins.tol[k]) for k in range(first, K + 1))
    res = er.true_residual(p.A, p.b, bad[1][K])
    by_x = abs(res - pins.res_exact(K)) / (pins.res_exact(K) * pins.x_tolerances(K)[1])
    return pins, clean, bad, by_history, by_x


@pytest.mark.parametrize("case", X_DEFECTS, ids=_defect_id)
def test_engine_x_defects_are_invisible_to_the_history_and_far_outside_check_x(env, case):
    """What ``check_x`` is for: the float64 restatement with one statement of x wrong -- an update left out or applied
    twice, the vector of the other side of the preconditioner, the rotation's other factor, a predicate ignored --
    leaves the history BITWISE what the clean restatement gives (below 1 x tol_k of the exact one) and moves
    ||b - A x_K|| by 100 x tol_res or more.  Prints error / tolerance (NOTES.md records them)."""
    pins, clean, bad, by_history, by_x = _engine_defect(env, case)
    K = pins.K
    assert np.array_equal(bad[0], clean[0]) and by_history < 1, (case, by_history)
    print(f"engine x defect {_defect_id(case)}: error / tolerance {by_history:.1e} (history) {by_x:.1e} (x_K)")
    assert by_x >= 100, (case, by_x)
    pins.check(list(bad[0]), "defect")
    with pytest.raises(AssertionError):
        pins.check_x(bad[1][K], K, "defect")


@pytest.mark.parametrize("case", HISTORY_DEFECTS, ids=_defect_id)
def test_engine_history_defects_of_the_newly_reached_iterations(env, case):
    """What the larger K is for: BiCGStab(l)'s rho *= -omega left out, or its beta without alpha in a second cycle, and a
    stale beta at iteration 3 of CGS and TFQMR, leave every entry the K of ``er.iterations`` pins bitwise alone and move a
    later one by 100 x tol_k or more."""
    method, param, side, shape, kind, K, defect, at = case
    pins, clean, bad, by_history, by_x = _engine_defect(env, case)
    old = er.iterations(method, param, False)
    if (method, param) == ("bicgstabl", 2):
        old = 2  # (its K = 3 already forms the second cycle's first beta; K = 5 forms the third's)
    assert np.array_equal(bad[0][:old + 1], clean[0][:old + 1]), case
    print(f"engine history defect {_defect_id(case)}: error / tolerance {by_history:.1e} (history) {by_x:.1e} (x_K)")
    assert by_history >= 100, (case, by_history)
    with pytest.raises(AssertionError):
        pins.check(list(bad[0]), "defect")
