"""Mixed-precision CG (csrc/mixed_cg.hip; include/storm_hip.h "Mixed-precision CG").

1. every vector statement of the inner loop, bit for bit, against (float) of the library's own fp64 statements on the
   widened operands, in both access modes of both options; alpha and beta as single divisions of the device's sums
2. the sums: exact on dyadic data, within the order-independent bound of storm_hip_dot elsewhere
3. solves to 1e-6 and 1e-9 held to the reference's rule on the recomputed true residual, to the fp64 solve, to the numpy
   restatement's outer-step count (tests/mixed_cg_ref.py) and to an iteration cap
4. the fp64 finish, 5. no host wait inside the inner loop and the counters, 6. every refusal, 7. a refreshed operator,
8. the C++ driver.

Statement shapes (all built with spmv_dict = 0): chains of 2, 64, 65, 127 and 4 097 rows, the 12 x 10 x 9 box (1 080 rows, a
ragged last slice), amg_cases.random_symmetric(seed 3) -- the smallest at which a slice edge, the ticket fold (more than one
block of either grid) and the rounding can go wrong."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import amg_cases
import mixed_cg_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_UNSUPPORTED = -1, -6
MODES = [(0, 0), (2, 1), (0, 1), (2, 0)]  # (blas1_nt, nontemporal)


@pytest.fixture(scope="module")
def env():
    from stormruler_amd import _lib, api

    ctx = api.Context(0)
    yield api, _lib, ctx
    ctx.set_option("blas1_nt", 1)
    ctx.set_option("nontemporal", 1)
    ctx.close()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def f32w(a):
    """double(float(a)), numpy's round-to-nearest-even conversion."""
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def face_matrix(api, ctx, case, updatable=False, ell_cap=0, spmv_dict=0, n_halo=0):
    n, inner, outer, w, de = case
    ctx.set_option("spmv_dict", spmv_dict)
    ctx.set_option("ell_cap", ell_cap)
    try:
        make = api.StencilMatrix.from_face_weights_updatable if updatable else api.StencilMatrix.from_face_weights
        return make(ctx, n - n_halo, n_halo, inner, outer, w, w, de[: n - n_halo])
    finally:
        ctx.set_option("spmv_dict", 4)
        ctx.set_option("ell_cap", 0)


def statement_cases():
    """{name: ("face", (n, inner, outer, w, diag_extra)) | ("csr", A)}; alpha, beta follow from the kind."""
    out = {}
    for n in (2, 64, 65, 127, 4097):
        i, o = ref.chain_faces(n)
        out[f"chain{n}"] = ("face", (n, i, o) + ref.jittered_case(n, i, o, seed=20 + n))
    i, o = ref.box_faces(12, 10, 9)
    out["box12x10x9"] = ("face", (1080, i, o) + ref.jittered_case(1080, i, o, seed=31))
    out["random_symmetric3"] = ("csr", amg_cases.random_symmetric(3))
    return out


STATEMENT_NAMES = ["chain2", "chain64", "chain65", "chain127", "chain4097", "box12x10x9", "random_symmetric3"]


def build_statement_case(api, ctx, name):
    kind, data = statement_cases()[name]
    if kind == "face":
        mat, coef, n = face_matrix(api, ctx, data), (-1.0, 0.0), data[0]
    else:
        ctx.set_option("spmv_dict", 0)
        try:
            mat = api.StencilMatrix.from_csr(ctx, data)
        finally:
            ctx.set_option("spmv_dict", 4)
        coef, n = (1.0, 0.0), data.shape[0]
    mat.build_reduced()
    return mat, api.HipStencilOperator(mat, *coef), n


def true_residual(api, lib, ctx, op, b, x):
    """(r, |r|) by the library's own statements: storm_hip_op_apply, storm_hip_axpbz(t, 1, b, -1, t), storm_hip_norm2."""
    t = api.DeviceVector(ctx, b.n_owned)
    op.mul(t, x)
    api._lib.check(lib.storm_hip_axpbz(t._h, 1.0, b._h, -1.0, t._h))
    return t, api.norm_2(t)


def widened(api, ctx, s, name, n):
    v = api.DeviceVector(ctx, n)
    s.get_vector(name, v)
    return v


def dot_bound(a, b):
    """n 2^-53 sum |a_i b_i|: whatever the order of an fp64 sum of the exact products (exact here: fp32 x fp32)."""
    return a.size * 2.0 ** -53 * float(np.abs(a * b).sum())


# ---- 1. statements, bit for bit; 2. the sums on unstructured data -------------------------------------------------------
@pytest.mark.parametrize("name", STATEMENT_NAMES)
def test_statements_bit_for_bit(env, name):
    api, _lib, ctx = env
    lib = _lib.lib
    mat, op, n = build_statement_case(api, ctx, name)
    rng = np.random.default_rng(3)
    b = api.DeviceVector.from_numpy(ctx, rng.standard_normal(n))
    x = api.DeviceVector.from_numpy(ctx, 0.1 * rng.standard_normal(n))
    alpha_op, beta_op = op.alpha, op.beta
    try:
        for blas1_nt, nontemporal in MODES:
            ctx.set_option("blas1_nt", blas1_nt)
            ctx.set_option("nontemporal", nontemporal)
            launches = ctx.counter("nt_stream_launches")
            s = api.MixedCgSolver()
            s.begin(x, b, op)
            r, rho = true_residual(api, lib, ctx, op, b, x)
            assert s.get_scalar("rho") == rho
            want_r = f32w(r.to_numpy() * (1.0 / rho))
            r_w, p_w, d_w = (widened(api, ctx, s, k, n) for k in ("r32", "p32", "d32"))
            assert same_bits(r_w.to_numpy(), want_r), (name, blas1_nt, nontemporal, "r32")
            assert same_bits(p_w.to_numpy(), want_r) and not d_w.to_numpy().any()
            g = s.get_scalar("g")
            assert abs(g - api.dot_product(r_w, r_w)) <= dot_bound(want_r, want_r)
            for step in range(3):
                s.inner(1)
                where = (name, blas1_nt, nontemporal, step)
                q_w = widened(api, ctx, s, "q32", n)
                t = api.DeviceVector.from_numpy(ctx, np.full(n, np.nan))
                mat.apply_reduced(alpha_op, beta_op, p_w, t)
                assert same_bits(q_w.to_numpy(), f32w(t.to_numpy())), where + ("q32",)
                pq, al, bt, g_new = (s.get_scalar(k) for k in ("pq", "alpha", "beta", "g"))
                assert abs(pq - api.dot_product(p_w, q_w)) <= dot_bound(p_w.to_numpy(), q_w.to_numpy()), where
                assert bits(al) == bits(g / pq) and bits(bt) == bits(g_new / g), where
                api._lib.check(lib.storm_hip_axpy(d_w._h, al, p_w._h))    # d = fma(a, p, d)
                api._lib.check(lib.storm_hip_axpy(r_w._h, -al, q_w._h))   # r = fma(-a, q, r)
                want_d, want_r = f32w(d_w.to_numpy()), f32w(r_w.to_numpy())
                d_w, r_w = widened(api, ctx, s, "d32", n), widened(api, ctx, s, "r32", n)
                assert same_bits(d_w.to_numpy(), want_d), where + ("d32",)
                assert same_bits(r_w.to_numpy(), want_r), where + ("r32",)
                assert abs(g_new - api.dot_product(r_w, r_w)) <= dot_bound(want_r, want_r), where
                api._lib.check(lib.storm_hip_xpay(p_w._h, r_w._h, bt))    # p = r + bt p
                want_p = f32w(p_w.to_numpy())
                p_w = widened(api, ctx, s, "p32", n)
                assert same_bits(p_w.to_numpy(), want_p), where + ("p32",)
                g = g_new
            if blas1_nt == 2:  # the comparison of the two streaming instances cannot be vacuous
                assert ctx.counter("nt_stream_launches") > launches
            s.close()
    finally:
        ctx.set_option("blas1_nt", 1)
        ctx.set_option("nontemporal", 1)
        mat.close()


@pytest.mark.parametrize("n", [2, 64, 65, 127, 4097, 1080])
def test_sums_are_exact_on_integers(env, n):
    """Small-integer weights and a right-hand side of 4^k entries +-1: |b| = 2^k, so r32 = p32 = +-2^-k and every product and
    every partial sum of g and of <p32, A~ p32> is a dyadic number far inside fp32 and fp64 -- whatever the order, g = 1
    and 4^k pq is the integer the assembled operator gives (the method of tests/exact_ref.py)."""
    api, _lib, ctx = env
    rng = np.random.default_rng(40 + n)
    i, o = ref.box_faces(12, 10, 9) if n == 1080 else ref.chain_faces(n)
    w = rng.integers(1, 8, i.size).astype(np.float64)
    de = -rng.integers(1, 5, n).astype(np.float64)
    m = 1
    while 4 * m <= n:
        m *= 4
    b_host = np.zeros(n)
    b_host[rng.choice(n, m, replace=False)] = rng.choice([-1.0, 1.0], m)
    a = ref.face_operator(n, i, o, w, de)
    want_pq = float(b_host @ (a @ b_host)) / m  # an integer over 4^k: exact
    mat = face_matrix(api, ctx, (n, i, o, w, de))
    mat.build_reduced()
    op = api.HipStencilOperator(mat, -1.0, 0.0)
    b, x = api.DeviceVector.from_numpy(ctx, b_host), api.DeviceVector.from_numpy(ctx, np.zeros(n))
    try:
        for blas1_nt, nontemporal in MODES[:2]:
            ctx.set_option("blas1_nt", blas1_nt)
            ctx.set_option("nontemporal", nontemporal)
            s = api.MixedCgSolver()
            s.begin(x, b, op)
            assert s.get_scalar("rho") == np.sqrt(m) and s.get_scalar("g") == 1.0
            s.inner(1)
            assert s.get_scalar("pq") == want_pq, (n, blas1_nt, nontemporal)
            assert bits(s.get_scalar("alpha")) == bits(1.0 / want_pq)
            s.close()
    finally:
        ctx.set_option("blas1_nt", 1)
        ctx.set_option("nontemporal", 1)
        mat.close()


# ---- 3. solves -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solve_inputs(env):
    """Per input: the matrix with its companion, the operator, the host operators (A, A~) -- built once."""
    api, _lib, ctx = env
    out = {}
    for name, case in ref.solve_cases().items():
        mat = face_matrix(api, ctx, case)
        mat.build_reduced()
        out[name] = (case, mat, api.HipStencilOperator(mat, -1.0, 0.0), ref.face_operator_pair(*case))
    yield out
    for _case, mat, _op, _pair in out.values():
        mat.close()


def meets_rule(abs_err, rho0, tol):
    return ref.rule(abs_err, rho0, tol, tol)


@pytest.mark.parametrize("name", ["box24", "jitter37x21x19", "square_nb"])
@pytest.mark.parametrize("kind", ["ones", "random"])
@pytest.mark.parametrize("tol", [1e-6, 1e-9])
def test_solves_meet_the_rule_without_fallback(env, solve_inputs, name, kind, tol):
    api, _lib, ctx = env
    lib = _lib.lib
    case, mat, op, (a, a32) = solve_inputs[name]
    n = case[0]
    b_host = ref.rhs(n, kind)
    b = api.DeviceVector.from_numpy(ctx, b_host)
    # the fp64 solve converges on this input (asserted first), and is the yardstick of the two bounds below
    x64 = api.DeviceVector.from_numpy(ctx, np.zeros(n))
    cg = api.CgSolver()
    cg.absolute_error_tolerance = cg.relative_error_tolerance = tol
    assert cg.solve(x64, b, op)
    _, rho0 = true_residual(api, lib, ctx, op, b, api.DeviceVector.from_numpy(ctx, np.zeros(n)))
    bound = 2.0 * max(tol, tol * rho0)
    for keep in (0, 1):
        for itol in (1e-2, 1e-3):
            x = api.DeviceVector.from_numpy(ctx, np.zeros(n))
            s = api.MixedCgSolver()
            s.absolute_error_tolerance = s.relative_error_tolerance = tol
            s.inner_tolerance, s.keep_direction, s.record_history = itol, keep, True
            converged = s.solve(x, b, op)
            m = ref.mixed_cg(a, a32, b_host, abs_tol=tol, rel_tol=tol, inner_tolerance=itol, keep_direction=keep)
            print(f"{name} {kind} tol {tol:g} inner_tol {itol:g} keep {keep}: fp64 CG {cg.iteration} iterations; mixed "
                  f"{s.inner_iterations} inner / {s.outer_steps} outer / {s.fp64_iterations} fp64 (finished_fp64 "
                  f"{s.finished_fp64}); restatement {m['inner_iterations']} inner / {m['outer_steps']} outer")
            where = (name, kind, tol, itol, keep)
            # correctness
            assert converged, where
            r, rho = true_residual(api, lib, ctx, op, b, x)
            assert meets_rule(rho, rho0, tol), where + (rho, rho0)
            api._lib.check(lib.storm_hip_axpbz(r._h, 1.0, x._h, -1.0, x64._h))  # r = x_mixed - x_fp64
            t = api.DeviceVector(ctx, n)
            op.mul(t, r)
            assert api.norm_2(t) <= bound, where
            assert s.history.size == s.outer_steps + 1 and s.history[0] == rho0 and s.history[-1] == rho, where
            assert s.absolute_error == rho and s.initial_error == rho0 and s.iteration == s.inner_iterations
            assert s.num_applies == 1 + s.inner_iterations + s.outer_steps
            assert np.all(np.diff(s.history) < 0), where
            # no fallback, here and in the restatement
            assert s.finished_fp64 == 0 and s.fp64_iterations == 0 and m["finished_fp64"] == 0, where
            assert abs(s.outer_steps - m["outer_steps"]) <= 1, where
            assert s.inner_iterations <= 2 * cg.iteration, where  # a condition, not a measurement: a stall must not pass
            s.close()


def test_history_holds_the_true_residual_of_every_outer_step(env, solve_inputs):
    """The norms between the first and the last: a solve cut after k outer steps by its iteration budget (the inner iterations
    a solve with max_outer = k reports) returns the x of that step, whose recomputed residual norm is entry k, bit for bit."""
    api, _lib, ctx = env
    lib = _lib.lib
    case, mat, op, _pair = solve_inputs["square_nb"]
    n = case[0]
    b = api.DeviceVector.from_numpy(ctx, ref.rhs(n, "random"))

    def solver(**kw):
        s = api.MixedCgSolver()
        s.absolute_error_tolerance = s.relative_error_tolerance = 1e-9
        s.inner_tolerance, s.record_history = 1e-2, True
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    full = solver()
    x = api.DeviceVector.from_numpy(ctx, np.zeros(n))
    assert full.solve(x, b, op) and full.outer_steps >= 3
    for k in range(1, full.outer_steps):
        probe = solver(max_outer=k)
        probe.solve(api.DeviceVector.from_numpy(ctx, np.zeros(n)), b, op)
        assert probe.finished_fp64 == 3 and probe.outer_steps == k
        cut = solver(num_iterations=probe.inner_iterations)
        xk = api.DeviceVector.from_numpy(ctx, np.zeros(n))
        assert not cut.solve(xk, b, op)
        assert cut.outer_steps == k and cut.fp64_iterations == 0 and cut.finished_fp64 == 3
        _, rho_k = true_residual(api, lib, ctx, op, b, xk)
        assert full.history[k] == rho_k == cut.history[k] == cut.absolute_error, k
        for s in (probe, cut):
            s.close()
    full.close()


# ---- 4. the fp64 finish ---------------------------------------------------------------------------------------------------
def test_one_outer_step_is_finished_in_fp64(env, solve_inputs):
    api, _lib, ctx = env
    lib = _lib.lib
    case, mat, op, _pair = solve_inputs["square_nb"]
    n = case[0]
    b = api.DeviceVector.from_numpy(ctx, ref.rhs(n, "ones"))
    x = api.DeviceVector.from_numpy(ctx, np.zeros(n))
    s = api.MixedCgSolver()
    s.absolute_error_tolerance = s.relative_error_tolerance = 1e-9  # one outer step at inner_tolerance 1e-3 cannot reach it
    s.max_outer, s.record_history = 1, True
    finishes = ctx.counter("mixed_fp64_finishes")
    assert s.solve(x, b, op)
    assert s.finished_fp64 == 3 and s.outer_steps == 1 and s.fp64_iterations > 0
    assert s.iteration == s.inner_iterations + s.fp64_iterations
    assert s.history.size == 1 + s.outer_steps + s.fp64_iterations
    assert ctx.counter("mixed_fp64_finishes") == finishes + 1
    _, rho = true_residual(api, lib, ctx, op, b, x)
    assert meets_rule(rho * (1 - 1e-6), s.initial_error, 1e-9)  # (the finishing loop's recurrence residual met it)
    s.close()


def test_a_broken_inner_loop_leaves_x_to_the_fp64_loop(env, solve_inputs):
    """alpha = +1 on the box: A = M is negative definite, <p, A~ p> < 0 in the first inner iteration.  The step stores
    nothing, x is the starting x, and the result is what storm_hip_solve_cg gives from it."""
    api, _lib, ctx = env
    case, mat, _op, _pair = solve_inputs["box24"]
    n = case[0]
    op = api.HipStencilOperator(mat, 1.0, 0.0)
    b = api.DeviceVector.from_numpy(ctx, ref.rhs(n, "random"))
    x0 = 0.01 * np.random.default_rng(8).standard_normal(n)
    x, x64 = api.DeviceVector.from_numpy(ctx, x0), api.DeviceVector.from_numpy(ctx, x0)
    cg = api.CgSolver()
    ok64 = cg.solve(x64, b, op)
    s = api.MixedCgSolver()
    ok = s.solve(x, b, op)
    assert s.finished_fp64 == 2 and s.outer_steps == 1 and s.inner_iterations == 1
    assert ok == ok64 and s.fp64_iterations == cg.iteration
    assert same_bits(x.to_numpy(), x64.to_numpy())
    s.close()


# ---- 5. no host wait inside the inner loop; the counters ----------------------------------------------------------------
def test_no_host_wait_in_the_inner_loop_and_the_counters_add_up(env, solve_inputs):
    api, _lib, ctx = env
    case, mat, op, _pair = solve_inputs["jitter37x21x19"]
    n = case[0]
    b = api.DeviceVector.from_numpy(ctx, ref.rhs(n, "random"))
    x = api.DeviceVector.from_numpy(ctx, np.zeros(n))
    s = api.MixedCgSolver()
    s.begin(x, b, op)
    waits = ctx.counter("host_reductions")
    s.inner(50)
    assert ctx.counter("host_reductions") == waits
    rho = s.end_outer(x)
    assert ctx.counter("host_reductions") == waits + 1  # the true residual's norm: one per outer step
    assert np.isfinite(rho) and rho < np.linalg.norm(ref.rhs(n, "random"))
    keys = ("mixed_solves", "mixed_inner_iterations", "mixed_outer_steps", "mixed_fp64_finishes")
    before = [ctx.counter(k) for k in keys]
    total = [0, 0, 0, 0]
    for max_outer in (16, 1):
        s.max_outer = max_outer
        s.absolute_error_tolerance = s.relative_error_tolerance = 1e-9
        waits = ctx.counter("host_reductions")
        assert s.solve(api.DeviceVector.from_numpy(ctx, np.zeros(n)), b, op)
        if s.finished_fp64 == 0:  # one wait for |r_0| and one per outer step, none per inner iteration
            assert ctx.counter("host_reductions") == waits + 1 + s.outer_steps
        total = [total[0] + 1, total[1] + s.inner_iterations, total[2] + s.outer_steps, total[3] + int(s.finished_fp64 != 0)]
    assert [ctx.counter(k) for k in keys] == [u + v for u, v in zip(before, total)]
    assert total[3] == 1
    s.close()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------
def test_every_refusal_by_code(env):
    api, _lib, ctx = env
    lib = _lib.lib
    i, o = ref.box_faces(12, 10, 9)
    case = (1080, i, o) + ref.jittered_case(1080, i, o, seed=31)
    good = _lib.MixedParams()
    lib.storm_hip_mixed_params_default(C.byref(good))
    h = C.c_void_p()

    def create(mat, params=good, alpha=-1.0):
        return lib.storm_hip_mixed_cg_create(mat._h, alpha, 0.0, C.byref(params), C.byref(h))

    def still_applies(mat, n):
        xv = api.DeviceVector.from_numpy(ctx, np.ones(n))
        y = api.DeviceVector(ctx, n)
        mat.apply(-1.0, 0.0, xv, y)
        assert np.isfinite(y.to_numpy()).all()

    # not on fp64 records (a few distinct weights: the default build takes a compact format)
    mat = face_matrix(api, ctx, (1080, i, o, np.ones(i.size), np.full(1080, -0.5)), spmv_dict=4)
    assert mat.stats()["value_dictionary_size"] > 0 or mat.stats()["paired_rows"] > 0
    assert create(mat) == E_UNSUPPORTED and not h.value
    still_applies(mat, 1080)
    mat.close()
    # a CSR tail
    mat = face_matrix(api, ctx, case, ell_cap=2)
    mat.build_reduced()
    assert mat.stats()["tail_rows"] > 0
    assert create(mat) == E_UNSUPPORTED and b"tail" in lib.storm_hip_last_error() and not h.value
    still_applies(mat, 1080)
    mat.close()
    # halo columns: the last plane of the box as halo
    keep = i < 960
    mat = face_matrix(api, ctx, (1080, i[keep], o[keep], case[3][keep], case[4]), n_halo=120)
    assert create(mat) == E_UNSUPPORTED and not h.value
    mat.close()
    # no companion; then the knobs; then a solve after the companion was dropped
    mat = face_matrix(api, ctx, case)
    assert create(mat) == E_UNSUPPORTED and b"storm_hip_op_build_reduced" in lib.storm_hip_last_error() and not h.value
    mat.build_reduced()
    for field, value in (("inner_tolerance", 0.0), ("inner_tolerance", 1.0), ("inner_tolerance", -0.5), ("inner_max", -1),
                         ("max_outer", 0), ("keep_direction", 2)):
        p = _lib.MixedParams()
        lib.storm_hip_mixed_params_default(C.byref(p))
        setattr(p, field, value)
        assert create(mat, p) == E_INVALID and not h.value, (field, value)
    assert create(mat) == 0 and h.value
    n = 1080
    b, x = api.DeviceVector.from_numpy(ctx, np.ones(n)), api.DeviceVector.from_numpy(ctx, np.zeros(n))
    short = api.DeviceVector.from_numpy(ctx, np.zeros(n - 1))
    p, r, mr = _lib.SolverParams(), _lib.SolverResult(), _lib.MixedResult()
    lib.storm_hip_solver_params_default(C.byref(p))
    solve = lambda bv, xv: lib.storm_hip_mixed_cg_solve(h, bv._h, xv._h, C.byref(p), C.byref(r), None, C.byref(mr))  # noqa: E731
    assert solve(b, short) == E_INVALID and solve(b, b) == E_INVALID
    assert lib.storm_hip_mixed_cg_inner(h, 1) == E_INVALID  # no begin yet
    assert lib.storm_hip_mixed_cg_get_vector(h, b"z32", x._h) == E_INVALID
    assert lib.storm_hip_mixed_cg_get_scalar(h, b"omega", C.byref(C.c_double())) == E_INVALID
    assert solve(b, x) == 0 and r.converged == 1
    mat.drop_reduced()
    x0 = x.to_numpy()
    assert solve(b, x) == E_UNSUPPORTED and lib.storm_hip_mixed_cg_begin(h, b._h, x._h) == E_UNSUPPORTED
    assert same_bits(x.to_numpy(), x0)  # decided before any launch
    still_applies(mat, n)
    assert lib.storm_hip_mixed_cg_destroy(h) == 0
    mat.close()


# ---- 7. a refreshed operator ---------------------------------------------------------------------------------------------
def test_a_solve_after_a_refresh_meets_the_rule_on_the_new_operator(env):
    api, _lib, ctx = env
    lib = _lib.lib
    i, o = ref.box_faces(12, 10, 9)
    n = 1080
    w0, de0 = ref.jittered_case(n, i, o, seed=51)
    w1, de1 = ref.jittered_case(n, i, o, seed=52, shift=0.2)
    mat = face_matrix(api, ctx, (n, i, o, w0, de0), updatable=True)
    mat.build_reduced()
    op = api.HipStencilOperator(mat, -1.0, 0.0)
    b = api.DeviceVector.from_numpy(ctx, ref.rhs(n, "random"))
    s = api.MixedCgSolver()
    x = api.DeviceVector.from_numpy(ctx, np.zeros(n))
    assert s.solve(x, b, op) and s.finished_fp64 == 0
    x_old = x.to_numpy()
    wv, dv = api.DeviceVector.from_numpy(ctx, w1), api.DeviceVector.from_numpy(ctx, de1)
    mat.set_face_weights(wv, wv, dv)
    fresh = face_matrix(api, ctx, (n, i, o, w1, de1))
    x = api.DeviceVector.from_numpy(ctx, np.zeros(n))
    assert s.solve(x, b, op) and s.finished_fp64 == 0
    _, rho = true_residual(api, lib, ctx, api.HipStencilOperator(fresh, -1.0, 0.0), b, x)  # on the NEW operator, built afresh
    assert meets_rule(rho, s.initial_error, 1e-6)
    assert np.linalg.norm(x.to_numpy() - x_old) > 1e-3 * np.linalg.norm(x_old)
    s.close()
    fresh.close()
    mat.close()


# ---- 8. the C++ driver ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keep", [0, 1])
def test_cpp_driver(keep):
    exe = os.path.join(ROOT, "tests", "cpp", "mixed_cg_driver")
    if not os.path.exists(exe):
        import __graft_entry__ as ge

        ge.build()
    out = subprocess.run([exe, "24", "1e-8", str(keep)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    d = json.loads(out.stdout.strip().splitlines()[-1])
    print(d)
    assert d["converged"] and d["finished_fp64"] == 0 and d["mixed_solves"] == 1
    assert d["outer_steps"] >= 2 and d["iterations"] == d["inner_iterations"]
    # the same residual by two fp64 statements that may round differently: ulps of |b| per entry, far below this
    assert abs(d["true_residual"] - d["absolute_error"]) <= 1e-12 * d["initial_error"]
    assert meets_rule(d["true_residual"], d["initial_error"], 1e-8)
