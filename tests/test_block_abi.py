"""Block vectors (k interleaved columns, include/storm_hip.h "block vectors"): the new entry points are declared, bound
and exported, keep the ABI version, and validate their arguments before they touch a device."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("storm_hip_block_get_column", "storm_hip_block_set_column", "storm_hip_block_dot", "storm_hip_block_axpy",
       "storm_hip_op_apply_block", "storm_hip_solve_cg_block")


@pytest.fixture(scope="module")
def lib():
    from stormruler_amd import _lib

    return _lib


def test_block_entry_points_are_declared_bound_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "storm_hip.h")).read()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in lib.SIGNATURES and lib.SIGNATURES[name][0] is C.c_int, name
        assert getattr(lib.lib, name) is not None
    assert lib.lib.storm_hip_abi_version() == 6  # additive only


def test_header_cites_the_reference_for_every_block_entry_point():
    header = open(os.path.join(ROOT, "include", "storm_hip.h")).read()
    for name, cite in (("storm_hip_block_get_column", "Field.hpp"), ("storm_hip_block_dot", "MatrixAlgorithms.hpp"),
                       ("storm_hip_block_axpy", "SolverCg.hpp"), ("storm_hip_op_apply_block", "Operator.hpp"),
                       ("storm_hip_solve_cg_block", "SolverCg.hpp")):
        at = header.index("int " + name)
        assert cite in header[max(0, at - 1500):at], (name, cite)


def test_null_handles_are_refused_without_a_device(lib):
    L = lib.lib
    one = (C.c_double * 8)()
    res = (lib.SolverResult * 8)()
    p = lib.SolverParams()
    L.storm_hip_solver_params_default(C.byref(p))
    calls = {
        "storm_hip_block_get_column": lambda: L.storm_hip_block_get_column(None, 2, 0, None),
        "storm_hip_block_set_column": lambda: L.storm_hip_block_set_column(None, 2, 0, None),
        "storm_hip_block_dot": lambda: L.storm_hip_block_dot(None, None, 2, one),
        "storm_hip_block_axpy": lambda: L.storm_hip_block_axpy(None, one, None, 2),
        "storm_hip_op_apply_block": lambda: L.storm_hip_op_apply_block(None, -1.0, 0.0, 2, None, None),
        "storm_hip_solve_cg_block": lambda: L.storm_hip_solve_cg_block(None, -1.0, 0.0, 2, None, None, C.byref(p), res, None),
    }
    assert set(calls) == set(NEW)
    for name, call in calls.items():
        assert call() == -1, name  # STORM_HIP_E_INVALID
        assert b"null" in L.storm_hip_last_error(), (name, L.storm_hip_last_error())
    # k outside 1..8 is no better with null handles, and a null output array is an argument error too
    assert L.storm_hip_op_apply_block(None, -1.0, 0.0, 9, None, None) == -1
    assert L.storm_hip_block_dot(None, None, 0, None) == -1
    assert L.storm_hip_solve_cg_block(None, -1.0, 0.0, 4, None, None, None, None, None) == -1


def test_python_block_api_is_exported():
    from stormruler_amd import api

    for name in ("BlockVector", "block_dot", "block_axpy", "BlockCgSolver"):
        assert hasattr(api, name), name
    assert hasattr(api.HipStencilOperator, "mul_block")
    s = api.BlockCgSolver()  # the reference's knob names and defaults (Solver.hpp:66-72)
    assert (s.num_iterations, s.absolute_error_tolerance, s.relative_error_tolerance) == (2000, 1.0e-6, 1.0e-6)
    assert issubclass(api.BlockVector, api.DeviceVector)
    with pytest.raises(ValueError):
        api.BlockVector(object(), 4, 9)  # k outside 1..8 is refused before anything is allocated
