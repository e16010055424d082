"""Host side of the Chebyshev preconditioner (no device): storm_hip_cheb_coefficients against the closed form of the
residual polynomial, and the argument checks."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cheb_ref  # noqa: E402

from stormruler_amd import _lib, mesh  # noqa: E402
from stormruler_amd._lib import lib  # noqa: E402

E_INVALID = -1


def _coefficients(lmin, lmax, degree):
    theta = C.c_double()
    c1, c2 = np.zeros(16), np.zeros(16)
    st = lib.storm_hip_cheb_coefficients(lmin, lmax, degree, C.byref(theta), c1.ctypes.data_as(_lib.f64p),
                                         c2.ctypes.data_as(_lib.f64p))
    return st, theta.value, c1[:max(degree, 0)], c2[:max(degree, 0)]


@pytest.fixture(scope="module")
def box8():
    g = mesh.structured_box(8)
    out = {}
    for alpha, beta in ((-1.0, 0.0), (-1e-2, 1.0)):
        a = mesh.assemble_csr(g, alpha, beta).tocsr()
        out[(alpha, beta)] = a
    return out


@pytest.mark.parametrize("alpha,beta", [(-1.0, 0.0), (-1e-2, 1.0)])
@pytest.mark.parametrize("jacobi", [False, True])
@pytest.mark.parametrize("degree", [1, 3, 6, 16])
def test_library_coefficients_reproduce_the_closed_form(box8, alpha, beta, jacobi, degree):
    a = box8[(alpha, beta)]
    n = a.shape[0]
    s = 1 / a.diagonal() if jacobi else np.ones(n)
    lmax = cheb_ref.gershgorin(a, s)
    lmin = lmax / 30
    st, theta, c1, c2 = _coefficients(lmin, lmax, degree)
    assert st == 0 and len(c1) == degree
    r = np.sin(0.37 * np.arange(n))
    z = cheb_ref.recurrence(a, s, r, theta, c1, c2)
    ref = cheb_ref.closed_form(a, s, r, lmin, lmax, degree)
    rel = np.linalg.norm(z - ref) / np.linalg.norm(ref)
    print(f"alpha {alpha} beta {beta} jacobi {jacobi} degree {degree}: rel {rel:.3e}")
    assert rel <= 1e-12


def test_api_coefficients_are_the_library_s():
    from stormruler_amd import api

    theta, c1, c2 = api.cheb_coefficients(0.25, 7.5, 5)
    st, theta_l, c1_l, c2_l = _coefficients(0.25, 7.5, 5)
    assert st == 0 and theta == theta_l and np.array_equal(c1, c1_l) and np.array_equal(c2, c2_l)
    t_ref, c1_ref, c2_ref = cheb_ref.coefficients(0.25, 7.5, 5)
    assert theta == t_ref
    np.testing.assert_allclose(c1, c1_ref, rtol=4e-16 * 8)
    np.testing.assert_allclose(c2, c2_ref, rtol=4e-16 * 8)


@pytest.mark.parametrize("lmin,lmax,degree", [(0.0, 1.0, 2), (-1.0, 1.0, 2), (1.0, 1.0, 2), (2.0, 1.0, 2),
                                              (float("nan"), 1.0, 2), (0.1, float("inf"), 2), (0.1, float("nan"), 2),
                                              (0.1, 1.0, 0), (0.1, 1.0, 17), (0.1, 1.0, -3)])
def test_invalid_coefficient_arguments(lmin, lmax, degree):
    st, *_ = _coefficients(lmin, lmax, degree)
    assert st == E_INVALID
    assert lib.storm_hip_last_error()


def test_null_arguments_need_no_device():
    theta = C.c_double()
    buf = np.zeros(16)
    p = buf.ctypes.data_as(_lib.f64p)
    assert lib.storm_hip_cheb_coefficients(0.1, 1.0, 2, None, p, p) == E_INVALID
    assert lib.storm_hip_cheb_coefficients(0.1, 1.0, 2, C.byref(theta), None, p) == E_INVALID
    assert b"null" in lib.storm_hip_last_error()
    h = C.c_void_p()
    v = C.c_double()
    assert lib.storm_hip_cheb_create(None, -1.0, 0.0, None, 2, 0.0, 0.0, C.byref(h)) == E_INVALID
    assert b"null" in lib.storm_hip_last_error()
    assert lib.storm_hip_cheb_apply(None, None, None) == E_INVALID
    assert lib.storm_hip_cheb_get(None, b"degree", C.byref(v)) == E_INVALID
    assert lib.storm_hip_op_gershgorin(None, -1.0, 0.0, None, C.byref(v)) == E_INVALID
    assert lib.storm_hip_krylov_set_preconditioner_cheb(None, None, 1) == E_INVALID
    assert lib.storm_hip_cheb_destroy(None) == 0
