"""Reference arithmetic of the Chebyshev preconditioner's tests: the recurrence in numpy (Saad, Iterative Methods, Alg. 12.1
started from zero) and the closed form it must reproduce, from an eigendecomposition -- neither calls the library."""
import numpy as np
import scipy.sparse as sp


def coefficients(lmin, lmax, degree):
    theta, delta = (lmax + lmin) / 2, (lmax - lmin) / 2
    sigma = theta / delta
    rho = 1 / sigma
    c1, c2 = [], []
    for _ in range(degree):
        rn = 1 / (2 * sigma - rho)
        c1.append(rn * rho)
        c2.append(2 * rn / delta)
        rho = rn
    return theta, np.array(c1), np.array(c2)


def recurrence(a, s, r, theta, c1, c2):
    """z after len(c1) steps, with the given coefficients (the library's, or `coefficients`')."""
    d = (s * r) / theta
    z, res = d.copy(), r.copy()
    for k in range(len(c1)):
        res = res - a @ d
        d = c1[k] * d + c2[k] * (s * res)
        z = z + d
    return z


def apply(a, s, r, lmin, lmax, degree):
    return recurrence(a, s, r, *coefficients(lmin, lmax, degree))


def chebyshev_t(k, x):
    x = np.asarray(x, dtype=float)
    out = np.empty_like(x)
    inside = np.abs(x) <= 1
    out[inside] = np.cos(k * np.arccos(x[inside]))
    out[~inside] = np.sign(x[~inside]) ** k * np.cosh(k * np.arccosh(np.abs(x[~inside])))
    return out


def eigenpairs(a, s):
    """(w, V) of diag(sqrt s) A diag(sqrt s): `closed_form`'s decomposition, for a caller that evaluates several degrees."""
    sh = np.sqrt(s)
    return np.linalg.eigh((sp.diags(sh) @ a @ sp.diags(sh)).toarray())


def closed_form(a, s, r, lmin, lmax, degree, eig=None):
    """z = diag(sqrt s) V ((1 - R(w)) / w) V^T diag(sqrt s) r with (w, V) the eigenpairs of diag(sqrt s) A diag(sqrt s) and
    R(w) = T_{m+1}((theta - w) / delta) / T_{m+1}(theta / delta).  `a` symmetric, s > 0.  `eig`: eigenpairs(a, s), if kept."""
    sh = np.sqrt(s)
    w, v = eigenpairs(a, s) if eig is None else eig
    theta, delta = (lmax + lmin) / 2, (lmax - lmin) / 2
    res_poly = chebyshev_t(degree + 1, (theta - w) / delta) / chebyshev_t(degree + 1, np.array([theta / delta]))[0]
    return sh * (v @ (((1 - res_poly) / w) * (v.T @ (sh * r))))


def gershgorin(a, s):
    return float(np.asarray(np.abs(sp.diags(s) @ a).sum(axis=1)).ravel().max())
