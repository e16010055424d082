"""The entry points of the multigrid preconditioner (include/storm_hip.h: storm_hip_amg_*,
storm_hip_krylov_set_preconditioner_amg) reject NULL handles with STORM_HIP_E_INVALID before they touch a device; the
binding classes carry the knobs."""
import ctypes as C


def test_amg_entry_points_reject_null_arguments_without_a_device():
    from stormruler_amd import _lib

    lib = _lib.lib
    for name in ("storm_hip_amg_params_default", "storm_hip_amg_setup_csr", "storm_hip_amg_hierarchy_destroy",
                 "storm_hip_amg_hierarchy_levels", "storm_hip_amg_hierarchy_level_sizes", "storm_hip_amg_hierarchy_get_operator",
                 "storm_hip_amg_hierarchy_get_aggregates", "storm_hip_amg_hierarchy_get_prolongator",
                 "storm_hip_amg_hierarchy_get_coarse_inverse", "storm_hip_amg_hierarchy_get", "storm_hip_amg_create",
                 "storm_hip_amg_apply", "storm_hip_amg_restrict", "storm_hip_amg_prolong_add", "storm_hip_amg_coarse_solve",
                 "storm_hip_amg_get", "storm_hip_amg_get_hierarchy", "storm_hip_amg_destroy",
                 "storm_hip_krylov_set_preconditioner_amg"):
        assert name in _lib.SIGNATURES
    lib.storm_hip_amg_params_default(None)  # (a no-op)
    h = C.c_void_p()
    assert lib.storm_hip_amg_setup_csr(4, None, None, None, None, C.byref(h)) == -1 and not h.value
    assert b"amg_setup: null" in lib.storm_hip_last_error()
    rp = (C.c_int64 * 2)(0, 1)
    assert lib.storm_hip_amg_setup_csr(1, rp, None, None, None, C.byref(h)) == -1 and not h.value
    assert b"amg_setup: null" in lib.storm_hip_last_error()
    assert lib.storm_hip_amg_setup_csr(1, rp, None, None, None, None) == -1
    assert lib.storm_hip_amg_hierarchy_destroy(None) == 0 and lib.storm_hip_amg_destroy(None) == 0
    n = C.c_int(-5)
    assert lib.storm_hip_amg_hierarchy_levels(None, C.byref(n)) == -1 and n.value == -5
    assert b"amg_hierarchy_levels: null" in lib.storm_hip_last_error()
    v = [C.c_int64(-5) for _ in range(4)]
    assert lib.storm_hip_amg_hierarchy_level_sizes(None, 0, *[C.byref(x) for x in v]) == -1 and v[0].value == -5
    assert b"amg_hierarchy_level_sizes: null" in lib.storm_hip_last_error()
    assert lib.storm_hip_amg_hierarchy_get_operator(None, 0, None, None, None) == -1
    assert b"amg_hierarchy_get_operator: null" in lib.storm_hip_last_error()
    assert lib.storm_hip_amg_hierarchy_get_aggregates(None, 0, None) == -1
    assert b"amg_hierarchy_get_aggregates: null" in lib.storm_hip_last_error()
    assert lib.storm_hip_amg_hierarchy_get_prolongator(None, 0, None, None, None) == -1
    assert b"amg_hierarchy_get_prolongator: null" in lib.storm_hip_last_error()
    assert lib.storm_hip_amg_hierarchy_get_coarse_inverse(None, None) == -1
    assert b"amg_hierarchy_get_coarse_inverse: null" in lib.storm_hip_last_error()
    d = C.c_double(-5.0)
    assert lib.storm_hip_amg_hierarchy_get(None, b"levels", C.byref(d)) == -1 and d.value == -5.0
    assert b"amg_hierarchy_get: null" in lib.storm_hip_last_error()
    assert lib.storm_hip_amg_create(None, 1.0, 0.0, None, C.byref(h)) == -1 and not h.value
    assert b"amg_create: null" in lib.storm_hip_last_error()
    assert lib.storm_hip_amg_create(None, 1.0, 0.0, None, None) == -1
    assert lib.storm_hip_amg_apply(None, None, None) == -1
    assert b"amg_apply: null" in lib.storm_hip_last_error()
    assert lib.storm_hip_amg_restrict(None, 0, None, None) == -1
    assert b"amg_restrict: null" in lib.storm_hip_last_error()
    assert lib.storm_hip_amg_prolong_add(None, 0, None, None) == -1
    assert b"amg_prolong_add: null" in lib.storm_hip_last_error()
    assert lib.storm_hip_amg_coarse_solve(None, None, None) == -1
    assert b"amg_coarse_solve: null" in lib.storm_hip_last_error()
    assert lib.storm_hip_amg_get(None, b"levels", C.byref(d)) == -1 and d.value == -5.0
    assert b"amg_get: null" in lib.storm_hip_last_error()
    assert lib.storm_hip_amg_get_hierarchy(None, C.byref(h)) == -1
    assert b"amg_get_hierarchy: null" in lib.storm_hip_last_error()
    assert lib.storm_hip_krylov_set_preconditioner_amg(None, None, 1) == -1
    assert b"krylov_set_preconditioner_amg: null" in lib.storm_hip_last_error()


def test_hierarchy_level_arguments_are_checked():
    import numpy as np
    import scipy.sparse as sp

    from stormruler_amd import _lib, api

    h = api.AmgHierarchy.from_csr(sp.identity(3).tocsr())
    assert h.levels == 1
    agg = np.zeros(3, np.int64)
    assert _lib.lib.storm_hip_amg_hierarchy_get_aggregates(h._h, 0, agg.ctypes.data_as(_lib.i64p)) == -1
    assert b"no aggregates" in _lib.lib.storm_hip_last_error()
    v = [C.c_int64() for _ in range(4)]
    assert _lib.lib.storm_hip_amg_hierarchy_level_sizes(h._h, 1, *[C.byref(x) for x in v]) == -1
    d = C.c_double()
    assert _lib.lib.storm_hip_amg_hierarchy_get(h._h, b"nonsense", C.byref(d)) == -1


def test_binding_classes_have_the_amg_knobs():
    from stormruler_amd import api

    p = api.AmgPreconditioner()
    assert p.reduced_records is False and p.params["smoother_degree"] is None
    assert api.AmgPreconditioner(smoother_degree=1, reduced_records=True).reduced_records is True
    for name in ("build", "mul", "conj_mul", "get", "close", "hierarchy"):
        assert hasattr(api.AmgPreconditioner, name)
    assert issubclass(api.AmgPreconditioner, api.Preconditioner)
