"""The entry points of the fp32-weight companion records (include/storm_hip.h: storm_hip_op_build_reduced, _drop_reduced,
_reduced_bytes, _apply_reduced, _gershgorin_reduced, storm_hip_cheb_create_reduced) reject NULL handles with
STORM_HIP_E_INVALID before they touch a device; the binding classes carry the new knobs."""
import ctypes as C


def test_reduced_entry_points_reject_null_arguments_without_a_device():
    from stormruler_amd import _lib

    lib = _lib.lib
    for name in ("storm_hip_op_build_reduced", "storm_hip_op_drop_reduced", "storm_hip_op_reduced_bytes",
                 "storm_hip_op_apply_reduced", "storm_hip_op_gershgorin_reduced", "storm_hip_cheb_create_reduced"):
        assert name in _lib.SIGNATURES
    assert lib.storm_hip_op_build_reduced(None) == -1
    assert b"op_build_reduced: null" in lib.storm_hip_last_error()
    assert lib.storm_hip_op_drop_reduced(None) == -1
    assert b"op_drop_reduced: null" in lib.storm_hip_last_error()
    n = C.c_int64(-5)
    assert lib.storm_hip_op_reduced_bytes(None, C.byref(n)) == -1 and n.value == -5
    assert b"op_reduced_bytes: null" in lib.storm_hip_last_error()
    assert lib.storm_hip_op_apply_reduced(None, 1.0, 0.0, None, None) == -1
    assert b"op_apply_reduced: null" in lib.storm_hip_last_error()
    v = C.c_double(-5.0)
    assert lib.storm_hip_op_gershgorin_reduced(None, 1.0, 0.0, None, C.byref(v)) == -1 and v.value == -5.0
    assert b"op_gershgorin_reduced: null" in lib.storm_hip_last_error()
    h = C.c_void_p()
    assert lib.storm_hip_cheb_create_reduced(None, 1.0, 0.0, None, 2, 0.0, 0.0, C.byref(h)) == -1 and not h.value
    assert b"cheb_create_reduced: null" in lib.storm_hip_last_error()
    assert lib.storm_hip_cheb_create_reduced(None, 1.0, 0.0, None, 2, 0.0, 0.0, None) == -1
    assert b"cheb_create_reduced: null" in lib.storm_hip_last_error()
    assert lib.storm_hip_cheb_create(None, 1.0, 0.0, None, 2, 0.0, 0.0, C.byref(h)) == -1  # the ordinary one keeps its name
    assert b"cheb_create: null" in lib.storm_hip_last_error()


def test_binding_classes_have_the_reduced_knobs():
    from stormruler_amd import api

    assert api.ChebyshevPreconditioner().reduced_records is False
    assert api.ChebyshevPreconditioner(degree=2, reduced_records=True).reduced_records is True
    for name in ("build_reduced", "drop_reduced", "reduced_bytes", "apply_reduced", "gershgorin_reduced"):
        assert hasattr(api.StencilMatrix, name)
