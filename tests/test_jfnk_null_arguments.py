"""The entry points of the finite-difference operator (include/storm_hip.h: storm_hip_krylov_set_operator_fd,
storm_hip_krylov_apply, storm_hip_krylov_get_int) reject NULL arguments and a bad mu with STORM_HIP_E_INVALID before they
touch a device; the binding classes exist with the reference's knobs."""
import ctypes as C
import math


def test_fd_entry_points_reject_null_arguments_and_bad_mu_without_a_device():
    from stormruler_amd import _lib

    lib = _lib.lib
    cb = _lib.APPLY_FN(lambda _user, _y, _x: 0)
    assert lib.storm_hip_krylov_set_operator_fd(None, cb, None, None, None, 1.0e-8) == -1
    assert b"krylov_set_operator_fd: null" in lib.storm_hip_last_error()
    assert lib.storm_hip_krylov_set_operator_fd(None, C.cast(None, _lib.APPLY_FN), None, None, None, 1.0e-8) == -1
    assert b"krylov_set_operator_fd: null" in lib.storm_hip_last_error()
    for mu in (0.0, -1.0e-8, math.inf, -math.inf, math.nan):  # (checked first: no object is needed to refuse it)
        assert lib.storm_hip_krylov_set_operator_fd(None, cb, None, None, None, mu) == -1
        assert b"krylov_set_operator_fd: mu" in lib.storm_hip_last_error()
    assert lib.storm_hip_krylov_apply(None, None, None) == -1
    assert b"krylov_apply: null" in lib.storm_hip_last_error()
    v = C.c_int64(-5)
    assert lib.storm_hip_krylov_get_int(None, b"inner_iterations", C.byref(v)) == -1
    assert b"krylov_get_int: null" in lib.storm_hip_last_error()
    assert lib.storm_hip_krylov_get_int(None, None, None) == -1 and v.value == -5
    h = C.c_void_p()
    assert lib.storm_hip_krylov_create(None, 10, C.byref(h)) == -1 and not h.value  # STORM_HIP_JFNK: no context, no object


def test_device_jfnk_solver_has_the_references_knobs():
    from stormruler_amd import api

    s = api.DeviceJfnkSolver()
    assert s._method == 10 and s.inner_iterations == 0
    assert s.num_iterations == 2000 and s.absolute_error_tolerance == 1.0e-6 and s.relative_error_tolerance == 1.0e-6
    assert s.pre_side == api.PreconditionerSide.Right and s.pre_op is None and s.iteration == 0
    assert api.JfnkSolver._method is None  # the host loop stays what it is
    op = api.FdJacobianOperator(api.make_operator(lambda y, x: None), None, None, 1.0e-8)
    assert op.mu == 1.0e-8 and isinstance(op, api.Operator)
