"""The three entry points of the two-stage operator (include/storm_hip.h: storm_hip_op_apply2, storm_hip_solve_cg2,
storm_hip_krylov_set_operator2) reject NULL arguments with STORM_HIP_E_INVALID before they touch a device."""
import ctypes as C


def test_two_stage_entry_points_reject_null_arguments_without_a_device():
    from stormruler_amd import _lib

    lib = _lib.lib
    consts = (-1.0e-4, 2.0, -1.0e-3, 1.0)
    p, r = _lib.SolverParams(), _lib.SolverResult()
    lib.storm_hip_solver_params_default(C.byref(p))
    assert lib.storm_hip_op_apply2(None, *consts, None, None, None) == -1
    assert b"op_apply2" in lib.storm_hip_last_error()
    assert lib.storm_hip_solve_cg2(None, *consts, None, None, C.byref(p), C.byref(r), None) == -1
    assert b"solve_cg2" in lib.storm_hip_last_error()
    assert lib.storm_hip_krylov_set_operator2(None, None, *consts) == -1
    assert b"krylov_set_operator2" in lib.storm_hip_last_error()
