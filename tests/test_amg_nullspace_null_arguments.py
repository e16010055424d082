"""The null-space entry points of the multigrid preconditioner (include/storm_hip.h: storm_hip_amg_setup_csr_nullspace,
storm_hip_amg_create_nullspace, storm_hip_amg_project) reject NULL handles and out-of-range arguments with
STORM_HIP_E_INVALID before they touch a device; the binding classes carry the knobs."""
import ctypes as C

import pytest


def test_nullspace_entry_points_reject_null_arguments_without_a_device():
    from stormruler_amd import _lib

    lib = _lib.lib
    for name in ("storm_hip_amg_setup_csr_nullspace", "storm_hip_amg_create_nullspace", "storm_hip_amg_project"):
        assert name in _lib.SIGNATURES
    h = C.c_void_p()
    for structural in (0, 1):
        assert lib.storm_hip_amg_setup_csr_nullspace(4, None, None, None, None, structural, C.byref(h)) == -1 and not h.value
        assert b"amg_setup: null" in lib.storm_hip_last_error()
    rp = (C.c_int64 * 2)(0, 1)
    assert lib.storm_hip_amg_setup_csr_nullspace(1, rp, None, None, None, 0, C.byref(h)) == -1 and not h.value
    assert b"amg_setup: null" in lib.storm_hip_last_error()
    assert lib.storm_hip_amg_setup_csr_nullspace(1, rp, None, None, None, 0, None) == -1
    for refreshable in (0, 1):
        assert lib.storm_hip_amg_create_nullspace(None, -1.0, 0.0, None, refreshable, C.byref(h)) == -1 and not h.value
        assert b"amg_create_nullspace: null" in lib.storm_hip_last_error()
    assert lib.storm_hip_amg_create_nullspace(None, -1.0, 0.0, None, 0, None) == -1
    assert lib.storm_hip_amg_project(None, None) == -1
    assert b"amg_project: null" in lib.storm_hip_last_error()


def test_out_of_range_arguments_of_the_setup():
    from stormruler_amd import _lib, api

    lib = _lib.lib
    h = C.c_void_p()
    col, val = (C.c_int64 * 4)(0, 1, 0, 1), (C.c_double * 4)(1.0, -1.0, -1.0, 1.0)
    rp = (C.c_int64 * 3)(0, 2, 4)
    # no rows, a first offset that is not 0, offsets that decrease, a column outside the matrix, a non-finite entry
    assert lib.storm_hip_amg_setup_csr_nullspace(0, rp, col, val, None, 0, C.byref(h)) == -1 and not h.value
    assert b"rows" in lib.storm_hip_last_error()
    assert lib.storm_hip_amg_setup_csr_nullspace(2, (C.c_int64 * 3)(1, 2, 4), col, val, None, 0, C.byref(h)) == -1
    assert b"row_ptr[0]" in lib.storm_hip_last_error()
    assert lib.storm_hip_amg_setup_csr_nullspace(2, (C.c_int64 * 3)(0, 3, 2), col, val, None, 0, C.byref(h)) == -1
    assert b"monotone" in lib.storm_hip_last_error()
    assert lib.storm_hip_amg_setup_csr_nullspace(2, rp, (C.c_int64 * 4)(0, 2, 0, 1), val, None, 0, C.byref(h)) == -1
    assert b"column" in lib.storm_hip_last_error()
    assert lib.storm_hip_amg_setup_csr_nullspace(2, rp, col, (C.c_double * 4)(1.0, float("nan"), -1.0, 1.0), None, 0, C.byref(h)) == -1
    assert b"non-finite" in lib.storm_hip_last_error() and not h.value
    for bad in (dict(smoother_degree=0), dict(smoother_degree=17), dict(coarse_rows=0), dict(coarse_rows=1025), dict(max_levels=0),
                dict(strength_theta=1.5), dict(prolongator_omega=2.0), dict(smoother_ratio=1.0), dict(reduced_records=2)):
        p = api._amg_params(**bad)
        assert lib.storm_hip_amg_setup_csr_nullspace(2, rp, col, val, C.byref(p), 0, C.byref(h)) == -1 and not h.value
        assert list(bad)[0].encode() in lib.storm_hip_last_error()
    # the two-cell Neumann operator itself is accepted, with either value of `structural` (any non-zero value counts as 1)
    for structural in (0, 1, 7):
        assert lib.storm_hip_amg_setup_csr_nullspace(2, rp, col, val, None, structural, C.byref(h)) == 0 and h.value
        d = C.c_double()
        assert lib.storm_hip_amg_hierarchy_get(h, b"structural", C.byref(d)) == 0 and d.value == (1.0 if structural else 0.0)
        assert lib.storm_hip_amg_hierarchy_get(h, b"nullspace", C.byref(d)) == 0 and d.value == 1.0
        assert lib.storm_hip_amg_hierarchy_destroy(h) == 0


def test_binding_classes_have_the_nullspace_knobs():
    from stormruler_amd import api

    p = api.AmgPreconditioner()
    assert p.nullspace is None and p.matrix is None
    assert api.AmgPreconditioner(nullspace="constant").nullspace == "constant"
    with pytest.raises(ValueError):
        api.AmgPreconditioner(nullspace="rigid")
    with pytest.raises(ValueError):
        api.AmgHierarchy.from_csr(None, nullspace="rigid")
    with pytest.raises(RuntimeError):
        p.project(None)
    assert hasattr(api.AmgPreconditioner, "project")
