"""Exact references for reductions and for the first Krylov iteration on integer data.

On a unit-spacing box every coefficient of the 7-point operator ``-L`` is a small integer (diagonal 6 + number of
walls, off-diagonals -1), so ``A`` maps integer vectors to integer vectors exactly.  When every partial sum of a dot
product is an integer below 2^53, a correct fp64 reduction returns the exact sum in ANY summation order: every grid
shape, fold, transport and rank count can be held to the bit against Python integers.

With x0 = 0 and r0 = b, the first iteration of CG, GMRES(m) and BiCGStab has closed forms in a few integer sums
(``first_step``); the residual norms after it are held to a tolerance derived from the data and the fold depth
(``tolerance``), never tuned to an observed error.

Plain module, not a conftest: the tests import it by name.
"""
import math
from fractions import Fraction

import numpy as np

EXACT = 1 << 53  # every partial sum strictly below: fp64 adds integers exactly
STREAM_BLOCK = 2048  # kStreamBlockElems: rows per block of the streaming kernels


def unit_box(mesh, nx, ny, nz):
    """The nx*ny*nz Dirichlet box with unit spacing: integer stencil coefficients."""
    return mesh.structured_box(nx, ny, nz, lengths=(float(nx), float(ny), float(nz)))


def int_apply(shape, x, k0=0, k1=None):
    """``(-L) x`` of the unit box exactly, in int64.  ``x`` holds the whole box (x fastest, then y, then z); with
    ``k0 / k1`` only the rows of planes k0 <= k < k1 are returned (a slab's owned rows)."""
    nx, ny, nz = shape
    k1 = nz if k1 is None else k1
    v = np.asarray(x, dtype=np.int64).reshape(nz, ny, nx)
    assert int(np.abs(v).max(initial=0)) * 12 < (1 << 62)
    out = np.zeros_like(v)
    for ax in range(3):
        n = v.shape[ax]
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[ax], hi[ax] = slice(0, n - 1), slice(1, n)
        lo, hi = tuple(lo), tuple(hi)
        d = v[lo] - v[hi]  # interior faces: (x_i - x_j) to both cells
        out[lo] += d
        out[hi] -= d
        first = [slice(None)] * 3
        last = [slice(None)] * 3
        first[ax], last[ax] = 0, n - 1
        out[tuple(first)] += 2 * v[tuple(first)]  # a wall: ghost value 0 at half the distance, weight 2
        out[tuple(last)] += 2 * v[tuple(last)]
    return out[k0:k1].reshape(-1)


def int_vector(n, seed, lo=-1000, hi=1000):
    """Integers uniform in [lo, hi] as int64."""
    return np.random.default_rng(seed).integers(lo, hi + 1, size=n, dtype=np.int64)


def exact_dot(a, b):
    """<a, b> of int64 vectors as a Python int, with the check that no partial sum in any order can reach 2^53 (so
    that an fp64 reduction must return it exactly) -- and that the int64 sum itself cannot wrap."""
    a = np.asarray(a, dtype=np.int64)
    b = np.asarray(b, dtype=np.int64)
    if a.size == 0:
        return 0
    ma, mb = int(np.abs(a).max()), int(np.abs(b).max())
    assert ma * mb * a.size < (1 << 62), "int64 sum could overflow"
    bound = int(np.dot(np.abs(a), np.abs(b)))
    assert bound < EXACT, f"partial sums may reach 2^53 ({bound})"
    return int(np.dot(a, b))


def wide_dot(a, b):
    """<a, b> as a Python int without the 2^53 condition (quantities only used through closed forms)."""
    a = np.asarray(a, dtype=np.int64)
    b = np.asarray(b, dtype=np.int64)
    assert int(np.abs(a).max(initial=0)) * int(np.abs(b).max(initial=0)) * max(a.size, 1) < (1 << 62)
    return int(np.dot(a, b))


class Sums:
    """The integer sums of b, z = A b and y = A z that the first iteration depends on."""

    def __init__(self, shape, b):
        b = np.asarray(b, dtype=np.int64)
        z = int_apply(shape, b)
        y = int_apply(shape, z)
        self.n = b.size
        self.rr = exact_dot(b, b)
        self.pz = exact_dot(b, z)
        self.zz = wide_dot(z, z)
        self.yz = wide_dot(y, z)
        self.yy = wide_dot(y, y)
        self.yb = wide_dot(y, b)  # == zz for a symmetric A


def fold_depth(n):
    """The longest addition chain through the fold: D = 64 + ceil(nblocks / 256), nblocks the streaming blocks."""
    nblocks = max(1, -(-n // STREAM_BLOCK))
    return 64 + -(-nblocks // 256)


def tolerance(n, magnitude, h1_sq):
    """Relative tolerance of a residual norm h1 after one iteration, from the data and the fold depth:

        tol = 2^-53 * (D + 16 * sqrt(M) / h1)

    h1^2 is the fold of the squares of the residual's computed elements: the fold adds at most D roundings of
    relative size 2^-53 to h1^2 (half that to h1).  Each element r_i is a combination of terms -- b and a z for CG
    (r1 = b - a z), b and c z for GMRES, b, a z, omega z and omega a y for BiCGStab -- and carries an error of a few
    roundings of its terms: a vector e with |e| <= 16 * 2^-53 * sqrt(M), M the sum of the squared norms of the terms,
    which moves h1 by at most |e|.  GMRES forms no r1: its history[1] is beta |s_1| from the Givens rotation of
    h11 = <w, v1> and h21 = |w - h11 v1|, w = A v1 = z / beta.  The one explicitly formed vector is u = z - (pz/rr) b,
    and h1 = sqrt(rr / zz) |u| up to the rotation's few roundings, so the argument holds for u: its terms give
    M_u = zz + pz^2/rr, and M_u / |u|^2 = (rr zz + pz^2) / (rr zz - pz^2) = M / h1^2 with GMRES's M = rr + pz^2/zz.
    At or below 1e-12 on every case the tests use (asserted): a dropped or doubled
    row moves these values by ~1/n, orders of magnitude more."""
    q = Fraction(magnitude) / Fraction(h1_sq)
    tol = (fold_depth(n) + 16.0 * math.sqrt(float(q))) * 2.0 ** -53
    assert tol <= 1e-12, f"tolerance {tol:.3e} above 1e-12: the case cannot separate a dropped row from rounding"
    return tol


def _sqrt(q):
    return math.sqrt(float(q))


class FirstStep:
    """Closed forms of the first iteration with x0 = 0, r0 = b.  ``h0``: sqrt(rr), the correctly rounded root of an
    integer below 2^53 (what every solver's history[0] must be, bitwise).  ``cg_alpha``: fl(rr / pz), one IEEE
    division of two exact sums; ``cg_x1(b)``: fl(alpha * b_i), elementwise (with x0 = 0, fma(a, p, 0) == a * p).  The
    ``*_h1`` are the exact residual norms after one iteration, ``*_tol`` their relative tolerances."""

    def __init__(self, s: Sums):
        self.s = s
        rr, pz, zz = s.rr, s.pz, s.zz
        assert pz > 0
        self.h0 = math.sqrt(float(rr))
        self.cg_alpha = float(rr) / float(pz)
        a = Fraction(rr, pz)
        # CG: r1 = b - a z, |r1|^2 = rr - 2 a pz + a^2 zz = a^2 zz - rr
        cg_sq = a * a * zz - rr
        self.cg_h1 = _sqrt(cg_sq)
        self.cg_tol = tolerance(s.n, rr + a * a * zz, cg_sq)
        # GMRES(m), any m: the first column minimises |b - c z|: |r1|^2 = rr - pz^2 / zz
        gm_sq = rr - Fraction(pz * pz, zz)
        self.gmres_h1 = _sqrt(gm_sq)
        self.gmres_tol = tolerance(s.n, rr + Fraction(pz * pz, zz), gm_sq)
        # BiCGStab: s = b - a z, t = A s = z - a y, omega = <t,s> / <t,t>, |r1|^2 = <s,s> - <t,s>^2 / <t,t>
        ss = rr - 2 * a * pz + a * a * zz
        ts = pz - a * zz - a * s.yb + a * a * s.yz
        tt = zz - 2 * a * s.yz + a * a * s.yy
        bi_sq = ss - ts * ts / tt
        self.bicgstab_h1 = _sqrt(bi_sq)
        om = ts / tt
        self.bicgstab_tol = tolerance(s.n, rr + a * a * zz + om * om * (zz + a * a * s.yy), bi_sq)

    def cg_x1(self, b):
        return self.cg_alpha * np.asarray(b, dtype=np.float64)


def close(value, exact, tol):
    return abs(value - exact) <= tol * exact
