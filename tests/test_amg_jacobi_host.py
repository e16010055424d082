"""The multigrid preconditioner's Jacobi smoother without a device: the new entry points exist, carry the documented
defaults and refuse NULL handles and out-of-range smoothers before they touch a device; and the numpy restatement
(tests/amg_jacobi_ref.py) shows what the smoother is for -- on upwind convection-diffusion the cycle with two Jacobi sweeps
makes right-preconditioned GMRES(30) converge within 30 iterations where the Chebyshev cycle does not converge in 300.

Restatement counts (inner iterations to 1e-6, b = 1, coarse_rows = 32), plain / 1, 2, 3 sweeps:
  13^3 (2197 / 280 / 24): 48 / 16, 10, 7;  20x18x16 (5760 / 752 / 52 / 6): 66 / 19, 12, 8;  Chebyshev degree 2: relative
  residual 0.94 and 0.96 after 300."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import amg_jacobi_ref  # noqa: E402

E_INVALID = -1


def test_entry_points_exist_with_their_defaults():
    from stormruler_amd import _lib

    for name in ("storm_hip_amg_smoother_default", "storm_hip_amg_create_smoother", "storm_hip_amg_smooth"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "storm_hip.h")).read()
    assert "#define STORM_HIP_HAS_AMG_JACOBI 1" in header
    s = _lib.AmgSmoother(-7, -7, -7.0)
    _lib.lib.storm_hip_amg_smoother_default(C.byref(s))
    assert (s.kind, s.sweeps, s.omega) == (1, 2, 2.0 / 3.0)
    _lib.lib.storm_hip_amg_smoother_default(None)  # (a no-op)
    assert _lib.lib.storm_hip_abi_version() == 6


def test_null_arguments_are_refused_without_a_device():
    from stormruler_amd import _lib

    lib = _lib.lib
    s = _lib.AmgSmoother()
    lib.storm_hip_amg_smoother_default(C.byref(s))
    h = C.c_void_p()
    assert lib.storm_hip_amg_create_smoother(None, 1.0, 0.0, None, C.byref(s), C.byref(h)) == E_INVALID and not h.value
    assert b"amg_create_smoother: null" in lib.storm_hip_last_error()
    assert lib.storm_hip_amg_create_smoother(None, 1.0, 0.0, None, None, C.byref(h)) == E_INVALID and not h.value
    assert b"amg_create_smoother: null" in lib.storm_hip_last_error()
    assert lib.storm_hip_amg_create_smoother(None, 1.0, 0.0, None, C.byref(s), None) == E_INVALID
    assert b"amg_create_smoother: null" in lib.storm_hip_last_error()
    assert lib.storm_hip_amg_smooth(None, 0, None, None, None) == E_INVALID
    assert b"amg_smooth: null" in lib.storm_hip_last_error()


@pytest.mark.parametrize("kind,sweeps,omega,word", [(1, 0, 0.5, "sweeps"), (1, 17, 0.5, "sweeps"), (1, -1, 0.5, "sweeps"),
                                                     (1, 2, 0.0, "omega"), (1, 2, -0.5, "omega"), (1, 2, 1.0000001, "omega"),
                                                     (1, 2, float("nan"), "omega"), (1, 2, float("inf"), "omega"),
                                                     (2, 2, 0.5, "kind"), (-1, 2, 0.5, "kind")])
def test_smoother_ranges_are_refused_without_a_device(kind, sweeps, omega, word):
    """The smoother is judged before the operator is looked at, so the refusal needs no operator."""
    from stormruler_amd import _lib

    s = _lib.AmgSmoother(kind, sweeps, omega)
    h = C.c_void_p()
    assert _lib.lib.storm_hip_amg_create_smoother(None, 1.0, 0.0, None, C.byref(s), C.byref(h)) == E_INVALID and not h.value
    msg = _lib.lib.storm_hip_last_error().decode()
    assert "amg_create_smoother" in msg and word in msg and "null" not in msg


def test_binding_class_has_the_knobs_and_refuses_the_combinations():
    from stormruler_amd import api

    p = api.AmgPreconditioner(smoother="jacobi")
    assert (p.smoother, p.jacobi_sweeps, p.jacobi_omega) == ("jacobi", 2, 2.0 / 3.0)
    assert api.AmgPreconditioner().smoother == "chebyshev"
    assert hasattr(api.AmgPreconditioner, "smooth")
    with pytest.raises(ValueError):
        api.AmgPreconditioner(smoother="gauss-seidel")
    with pytest.raises(ValueError):
        api.AmgPreconditioner(smoother="jacobi", refreshable=True)
    with pytest.raises(ValueError):
        api.AmgPreconditioner(smoother="jacobi", nullspace="constant")


@pytest.fixture(scope="module")
def boxes():
    from stormruler_amd import mesh

    out = {}
    for name, shape in (("13^3", (13,)), ("20x18x16", (20, 18, 16))):
        g, w, a = amg_jacobi_ref.convdiff_box(mesh, *shape)
        out[name] = (a, np.ones(a.shape[0])) + amg_jacobi_ref.cycles(a, sweeps=2, coarse_rows=32)
    return out


@pytest.mark.parametrize("name,rows", [("13^3", [2197, 280, 24]), ("20x18x16", [5760, 752, 52, 6])])
def test_two_jacobi_sweeps_converge_within_30_where_chebyshev_does_not_in_300(boxes, name, rows):
    a, b, levels, jacobi, chebyshev = boxes[name]
    assert [lv["A"].shape[0] for lv in levels] == rows
    assert abs(a - a.T).max() > 0.1 * abs(a).max()  # strongly non-symmetric
    _, plain, ok_plain = amg_jacobi_ref.gmres_right(a, b)
    x, it, ok = amg_jacobi_ref.gmres_right(a, b, jacobi)
    xc, it_c, ok_c = amg_jacobi_ref.gmres_right(a, b, chebyshev, max_it=300)
    rel_c = np.linalg.norm(b - a @ xc) / np.linalg.norm(b)
    print(f"{name}: plain {plain}, two Jacobi sweeps {it}, Chebyshev degree 2 {it_c} (relative residual {rel_c:.2e})")
    assert ok_plain and ok and it <= 30 and it < plain
    assert np.linalg.norm(b - a @ x) <= 1e-6 * np.linalg.norm(b) * (1 + 1e-8)
    assert not ok_c and it_c == 300 and rel_c > 1e-6


def test_restatement_is_symmetric_on_a_symmetric_operator():
    """For symmetric A the Jacobi cycle is a symmetric B (nu sweeps before, nu after, R = P^T)."""
    import amg_cases

    a = amg_cases.poisson_box(7)
    _, jacobi, _ = amg_jacobi_ref.cycles(a, sweeps=2, coarse_rows=32)
    rng = np.random.default_rng(6)
    u, v = rng.standard_normal(a.shape[0]), rng.standard_normal(a.shape[0])
    bu, bv = jacobi(u), jacobi(v)
    assert abs(u @ bv - v @ bu) <= 1e-12 * (np.linalg.norm(u) * np.linalg.norm(bv))
    assert u @ bu > 0 and v @ bv > 0
