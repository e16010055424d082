"""Mixed-precision CG without a device: the numpy restatement (tests/mixed_cg_ref.py) against plain float64 CG on the shapes
of tests/test_gpu_mixed_cg.py, the defaults of storm_hip_mixed_params_default, and the refusals that need no device."""
import ctypes as C

import numpy as np
import pytest

import mixed_cg_ref as ref

E_INVALID = -1


@pytest.mark.parametrize("name", ["box24", "jitter37x21x19", "square_nb"])
@pytest.mark.parametrize("kind", ["ones", "random"])
@pytest.mark.parametrize("tol", [1e-6, 1e-9])
def test_the_restatement_and_float64_cg_both_reach_the_rule(name, kind, tol):
    n, inner, outer, w, de = ref.solve_cases()[name]
    a, a32 = ref.face_operator_pair(n, inner, outer, w, de)
    b = ref.rhs(n, kind)
    x64, it64, ok64, _ = ref.cg64(a, b, abs_tol=tol, rel_tol=tol)
    assert ok64
    rho0 = np.linalg.norm(b)
    assert ref.rule(np.linalg.norm(b - a @ x64) * (1 - 1e-9), rho0, tol, tol)
    for keep in (0, 1):
        for itol in (1e-2, 1e-3):
            m = ref.mixed_cg(a, a32, b, abs_tol=tol, rel_tol=tol, inner_tolerance=itol, keep_direction=keep)
            print(f"{name} {kind} tol {tol:g} inner_tol {itol:g} keep {keep}: fp64 {it64}, inner {m['inner_iterations']}, "
                  f"outer {m['outer_steps']}, finished_fp64 {m['finished_fp64']}")
            assert m["converged"] and m["finished_fp64"] == 0 and m["fp64_iterations"] == 0
            assert ref.rule(np.linalg.norm(b - a @ m["x"]), rho0, tol, tol)
            assert m["inner_iterations"] <= 2 * it64  # the cap the GPU test holds the library to
            # the true residual fell at every outer step
            assert np.all(np.diff(m["history"]) < 0)


def test_the_restatement_finishes_in_float64_when_it_must():
    n, inner, outer, w, de = ref.solve_cases()["square_nb"]
    a, a32 = ref.face_operator_pair(n, inner, outer, w, de)
    b = ref.rhs(n, "ones")
    m = ref.mixed_cg(a, a32, b, abs_tol=1e-9, rel_tol=1e-9, max_outer=1)
    assert m["finished_fp64"] == 3 and m["converged"] and m["fp64_iterations"] > 0
    m = ref.mixed_cg(-a, -a32, b, abs_tol=1e-9, rel_tol=1e-9, num_iterations=50)  # negative definite: <p, q> < 0 at once
    assert m["finished_fp64"] == ref.BROKEN and m["inner_iterations"] == 1 and m["outer_steps"] == 1


def test_defaults_of_the_mixed_params():
    from stormruler_amd import _lib, api

    p = _lib.MixedParams(-1.0, -1, -1, -1)
    _lib.lib.storm_hip_mixed_params_default(C.byref(p))
    assert (p.inner_tolerance, p.inner_max, p.max_outer, p.keep_direction) == (1e-3, 0, 16, 0)
    _lib.lib.storm_hip_mixed_params_default(None)  # a null pointer is ignored
    s = api.MixedCgSolver()
    assert (s.inner_tolerance, s.inner_max, s.max_outer, s.keep_direction) == (1e-3, 0, 16, 0)
    assert (s.num_iterations, s.absolute_error_tolerance, s.relative_error_tolerance) == (2000, 1e-6, 1e-6)


def test_refusals_that_need_no_device():
    from stormruler_amd import _lib, api

    lib = _lib.lib
    h = C.c_void_p()
    good = _lib.MixedParams()
    lib.storm_hip_mixed_params_default(C.byref(good))
    # the knobs are checked before the operator is looked at
    for field, value, word in (("inner_tolerance", 0.0, b"inner_tolerance"), ("inner_tolerance", 1.0, b"inner_tolerance"),
                               ("inner_tolerance", float("nan"), b"inner_tolerance"), ("inner_max", -1, b"inner_max"),
                               ("max_outer", 0, b"max_outer"), ("keep_direction", 2, b"keep_direction"),
                               ("keep_direction", -1, b"keep_direction")):
        p = _lib.MixedParams()
        lib.storm_hip_mixed_params_default(C.byref(p))
        setattr(p, field, value)
        assert lib.storm_hip_mixed_cg_create(None, -1.0, 0.0, C.byref(p), C.byref(h)) == E_INVALID
        assert word in lib.storm_hip_last_error(), (field, value, lib.storm_hip_last_error())
        assert not h.value
    assert lib.storm_hip_mixed_cg_create(None, -1.0, 0.0, C.byref(good), C.byref(h)) == E_INVALID
    assert b"null" in lib.storm_hip_last_error()
    assert lib.storm_hip_mixed_cg_create(None, -1.0, 0.0, None, C.byref(h)) == E_INVALID
    assert lib.storm_hip_mixed_cg_solve(None, None, None, None, None, None, None) == E_INVALID
    assert lib.storm_hip_mixed_cg_begin(None, None, None) == E_INVALID
    assert lib.storm_hip_mixed_cg_inner(None, 1) == E_INVALID
    assert lib.storm_hip_mixed_cg_end_outer(None, None, None) == E_INVALID
    assert lib.storm_hip_mixed_cg_get_vector(None, b"r32", None) == E_INVALID
    assert lib.storm_hip_mixed_cg_get_scalar(None, b"g", None) == E_INVALID
    assert lib.storm_hip_mixed_cg_destroy(None) == 0
    # the Python class takes a HipStencilOperator and nothing else
    s = api.MixedCgSolver()
    with pytest.raises(TypeError):
        s.solve(None, None, api.make_symmetric_operator(lambda y, x: None))
    with pytest.raises(TypeError):
        s.begin(None, None, object())
