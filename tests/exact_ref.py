"""Exact references for reductions and for the first Krylov iteration on integer data.

On a unit-spacing box every coefficient of the 7-point operator ``-L`` is a small integer (diagonal 6 + number of
walls, off-diagonals -1), so ``A`` maps integer vectors to integer vectors exactly.  When every partial sum of a dot
product is an integer below 2^53, a correct fp64 reduction returns the exact sum in ANY summation order: every grid
shape, fold, transport and rank count can be held to the bit against Python integers.

With x0 = 0 and r0 = b, the first iteration of CG, GMRES(m) and BiCGStab has closed forms in a few integer sums
(``first_step``); the residual norms after it are held to a tolerance derived from the data and the fold depth
(``tolerance``), never tuned to an observed error.

The engine's other methods -- CGS, TFQMR(1), BiCGStab(l), IDR(s), Richardson, and the Jacobi-preconditioned solves --
are restated from the reference's headers on coefficient columns over the integer Krylov chain, in Fractions or
high-precision decimals (``Space`` and the method functions); ``Pins`` turns their exact histories into the values and
tolerances the tests assert.

GMRES(m) beyond its first step is pinned on a NON-symmetric integer operator -- convection-diffusion on the unit box
(``convdiff_box``, ``IntOperator``): on the symmetric Poisson box H is tridiagonal, the projections on q_0 ... q_{k-2}
are rounding noise, and a Gram-Schmidt kernel that skipped them could not be told from a correct one.  ``OpBasis`` is
the chain of a general integer operator (no Hankel shortcut in its Gram matrix), ``gmres`` the restatement of
SolverGmres.hpp with its inner_finalize, ``GmresPins`` the pins of history[0..K] and of x_K (``true_residual``), with a
precision guard: the power basis loses digits with K, so every pinned case is run at PREC and at 2 PREC digits and must
agree to 1e-40, and K stays at 12 or below.  ``mgs_float64`` is the same step in fp64 numpy, with the grouped evaluation
of the device's chain kernels and with the defects the pins must reject.

CG and BiCGStab past their first step: ``cg`` and ``bicgstab`` (SolverCg.hpp, SolverBiCgStab.hpp in Fractions; CG on
the two-stage operator (I + A)^2 through ``TwoStageSpace``) keep every iterate x_k and the ratio sqrt(M) / h of each
step's own terms; ``StepPins`` holds history[0..K], x_k and their tolerances by ``Pins``' rule, ``StepProblem`` one box
with its chain and operator.  The same bodies run on ``Float64Space`` (``cg_float64``, ``bicgstab_float64``) with the
defects the pins must reject.

Operators with a halo: ``periodic_box`` is the unit-spacing box that is periodic in z as one rank's local graph, the
rank its own neighbour -- -L (diagonal 6 ... 8) and the same convection-diffusion -- with ``IntOperator.from_local_graph``
folding the halo columns onto the owned cells they copy; ``StepProblem`` and ``GmresProblem`` take them as kinds
"periodic" and "periodic_convdiff" (tests/test_gpu_exact_rccl.py).  ``Float64Space`` takes the split A = A_in + A_h
along the periodic seam, and ``cg`` / ``bicgstab`` the defects of the halo alone (``CG_HALO_DEFECTS``,
``BICGSTAB_HALO_DEFECTS``): a missed exchange, halo rows formed with the previous beta, alpha or omega.

Plain module, not a conftest: the tests import it by name.
"""
import math
from decimal import Decimal, localcontext
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
    return _stencil(v)[k0:k1].reshape(-1)


def exact_apply(shape, x):
    """``(-L) x`` of the whole unit box for an object array (Python ints, Fractions, Decimals): no range limit."""
    nx, ny, nz = shape
    return _stencil(np.asarray(x, dtype=object).reshape(nz, ny, nx)).reshape(-1)


def int_diagonal(shape):
    """The diagonal of ``-L`` on the unit box: per axis 2, plus 1 for every wall the cell touches (6 ... 9, or more
    on a box one cell thick)."""
    nx, ny, nz = shape
    d = np.zeros((nz, ny, nx), np.int64)
    for ax, n in ((2, nx), (1, ny), (0, nz)):
        i = np.arange(n)
        w = 2 + (i == 0) + (i == n - 1)
        d += w.reshape([n if a == ax else 1 for a in range(3)])
    return d.reshape(-1)


def _stencil(v):
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
    return out


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


def tolerance(n, magnitude, h1_sq, c=16):
    """Relative tolerance of a residual norm h1 after one iteration, from the data and the fold depth:

        tol = 2^-53 * (D + c * sqrt(M) / h1),   c = 16 for the three closed forms below

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
    tol = (fold_depth(n) + c * math.sqrt(float(q))) * 2.0 ** -53
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


# ---- the Krylov methods in coefficient form -------------------------------------------------------------------------
#
# With x0 = 0 every vector CGS, TFQMR, BiCGStab(l), IDR(s), Richardson, CG and GMRES form lies in the span of a chain
# of integer vectors: W_0 = b, W_{t+1} = A W_t without a preconditioner; with the Jacobi preconditioner P = diag(dinv)
# the chain alternates W_{t+1} = D' W_t (t even) and A W_t (t odd), D' = 2^56 dinv an integer diagonal (fl(1/d) is a
# dyadic rational for d in {6, 7, 8, 9}), so that P W_t = 2^-56 W_{t+1}.  A vector is its coefficient column over the
# chain (plus, for IDR(s), over its fixed dyadic shadow vectors); applying A or P shifts the column by one place, and
# <u, v> = c_u^T G c_v with the Gram matrix G of the chain formed exactly in Python integers.  The method bodies below
# restate the reference's init / iterate on such columns (the header lines are cited on every statement); the scalars
# are Fractions where the method is rational and decimals of PREC digits where it takes a square root.  They are
# written against a small vector interface (``b``, ``zero``, ``A``, ``P``, ``dot``, ``fixed``), so the same bodies run
# on ``Space`` (coefficient columns) and ``ElemSpace`` (every element a Fraction / decimal, the brute force).

PRE_SHIFT = 56  # 2^56 * fl(1/d) is an integer for d in {6, 7, 8, 9} (1/9 has the finest last place, 2^-56)
PREC = 80  # decimal digits wherever a method takes a square root


def _dec(q):
    """A Fraction (or int) as a decimal of the current context: one rounding at 10^-PREC relative."""
    if isinstance(q, Decimal):
        return q
    q = Fraction(q)
    return Decimal(q.numerator) / Decimal(q.denominator)


def _mul(a, b):
    if isinstance(a, Decimal) != isinstance(b, Decimal):
        return _dec(a) * _dec(b)
    return a * b


def _add(a, b):
    if isinstance(a, Decimal) != isinstance(b, Decimal):
        return _dec(a) + _dec(b)
    return a + b


def _sdiv(x, y):
    """safe_divide (MathUtils.hpp:50-52)."""
    return 0 * x if y == 0 else x / y


class Vec:
    """A vector as its coefficient column {chain index (>= 0) or fixed vector (< 0): coefficient}."""
    __slots__ = ("c",)

    def __init__(self, c):
        self.c = c

    def _comb(self, o, sign):
        c = dict(self.c)
        for k, v in o.c.items():
            c[k] = _add(c[k], sign * v) if k in c else sign * v
        return Vec(c)

    def __add__(self, o):
        return self._comb(o, 1)

    def __sub__(self, o):
        return self._comb(o, -1)

    def __rmul__(self, a):
        return Vec({k: _mul(a, v) for k, v in self.c.items()})

    def __truediv__(self, a):
        return Vec({k: _dec(v) / a if isinstance(a, Decimal) else v / a for k, v in self.c.items()})


def _limbs(a, bits):
    """Signed limbs of an int64 vector: a = sum_k 2^(bits k) limb_k, |limb_k| < 2^bits."""
    s, m = np.sign(a), np.abs(a)
    out = []
    while True:
        out.append(s * (m & ((1 << bits) - 1)))
        m = m >> bits
        if not m.any():
            return out


def big_dot(u, v):
    """<u, v> as a Python int for integer vectors of any size: object arrays directly, int64 by limbs small enough that
    no int64 partial sum can wrap."""
    if u.dtype == object or v.dtype == object:
        return int(np.dot(u.astype(object), v.astype(object)))
    bits = (62 - max(1, u.size).bit_length()) // 2
    lu, lv = _limbs(u, bits), _limbs(v, bits)
    return sum(int(np.dot(a, b)) << (bits * (i + j)) for i, a in enumerate(lu) for j, b in enumerate(lv))


class Basis:
    """The integer chain of one problem (shape, b, optional Jacobi dinv), grown on demand, and its Gram entries,
    cached: one per problem serves every method, side and number type."""

    def __init__(self, shape, b, dinv=None):
        self.shape, self.n = tuple(shape), int(np.asarray(b).size)
        self.pre = dinv is not None
        if self.pre:
            dinv = np.asarray(dinv, np.float64)
            assert np.array_equal(dinv, 1.0 / int_diagonal(shape)), "dinv is not fl(1 / diag(A))"
            dp = dinv * 2.0 ** PRE_SHIFT  # exact: a power-of-two scaling
            assert np.all(dp == np.floor(dp)) and dp.max() < 2.0 ** 62
            self.dp = dp.astype(np.int64).astype(object)
            self.W = [np.asarray(b, np.int64).astype(object)]
        else:
            self.W = [np.asarray(b, np.int64)]
        self.R = []  # fixed dyadic vectors: (integer numerators as objects, common power-of-two denominator)
        self._fixed, self._g = {}, {}

    def grow(self, t):
        while len(self.W) <= t:
            w = self.W[-1]
            if self.pre and len(self.W) % 2 == 1:
                self.W.append(self.dp * w)
            elif w.dtype == object:
                self.W.append(exact_apply(self.shape, w))
            else:
                self.W.append(int_apply(self.shape, w))  # (asserts that int64 holds it)

    def fixed(self, values):
        """Register a fixed fp64 vector (a dyadic rational per element); returns its key (the same for the same bits)."""
        values = np.ascontiguousarray(values, np.float64)
        if values.tobytes() not in self._fixed:
            ratios = [float(v).as_integer_ratio() for v in values]
            den = max(d for _, d in ratios)
            self.R.append((np.array([p * (den // d) for p, d in ratios], dtype=object), den))
            self._fixed[values.tobytes()] = -len(self.R)
        return self._fixed[values.tobytes()]

    def _vec(self, k):
        if k >= 0:
            self.grow(k)
            return self.W[k], 1
        return self.R[-1 - k]

    def gram(self, i, j):
        key = (min(i, j), max(i, j))
        if key not in self._g:
            (u, du), (v, dv) = self._vec(i), self._vec(j)
            self._g[key] = Fraction(big_dot(u, v), du * dv)
        return self._g[key]

    def last_row(self, k):
        u, d = self._vec(k)
        return Fraction(int(u[-1]), d)


class IntOperator:
    """A square integer matrix held as CSR, applied exactly: int64 vectors while no partial sum can wrap (asserted
    from the largest row sum of |A|, as ``int_apply`` does), object vectors (Python ints, Fractions, decimals)
    without a limit.  ``from_face_weights`` assembles the device operator's difference form
    ``(A x)_i = sum_f w_if (x_other - x_i) + diag_extra_i x_i`` of a face graph -- what
    ``StencilMatrix.from_face_weights`` applies with alpha = 1, beta = 0 -- and asserts that every weight is an
    integer (true of ``mesh.convection_diffusion_weights`` on unit spacing with integer nu and velocity)."""

    def __init__(self, n, rows, cols, vals):
        import scipy.sparse as sps

        vals = np.asarray(vals)
        assert np.array_equal(vals, np.rint(vals)), "the operator is not integer"
        a = sps.coo_matrix((vals.astype(np.int64), (rows, cols)), shape=(n, n)).tocsr()
        a.sum_duplicates()
        a.eliminate_zeros()
        a.sort_indices()
        self.n, self.csr = n, a
        self.rowsum = int(abs(a).sum(axis=1).max())
        assert int(np.diff(a.indptr).min()) > 0  # (no empty row: ``true_residual`` reduces row by row)
        self._rows = self._obj = None  # (the object form: built when first applied to an object vector)

    @classmethod
    def from_face_weights(cls, g, w_inner, w_outer, diag_extra):
        n = g.n_cells
        assert g.n_halo == 0
        i, o = np.asarray(g.inner), np.asarray(g.outer)
        cells = np.arange(n)
        return cls(n, np.concatenate([i, i, o, o, cells]), np.concatenate([o, i, i, o, cells]),
                   np.concatenate([w_inner, -w_inner, w_outer, -w_outer, diag_extra]))

    @classmethod
    def from_local_graph(cls, g, w_inner, w_outer, diag_extra):
        """``from_face_weights`` for a local graph with a halo whose halo cells are copies of owned cells (a periodic
        box, the rank its own neighbour): the rows are the owned cells only, a halo column is folded onto the owned
        cell it is the image of, ``g.global_id[col]``."""
        n = g.n_cells
        gid = np.asarray(g.global_id, np.int64)
        assert g.n_halo > 0 and gid.shape == (g.n_total,) and np.array_equal(gid[:n], np.arange(n))
        assert int(gid[n:].min()) >= 0 and int(gid[n:].max()) < n, "a halo cell is no copy of an owned cell"
        i, o = np.asarray(g.inner), np.asarray(g.outer)
        cells = np.arange(n)
        rows = np.concatenate([i, i, o, o, cells])
        cols = np.concatenate([o, i, i, o, cells])
        vals = np.concatenate([w_inner, -w_inner, w_outer, -w_outer, diag_extra])
        own = rows < n
        return cls(n, rows[own], gid[cols[own]], vals[own])

    def seam_split(self, shape):
        """A = A_in + A_h as fp64 CSR for a box periodic in z: A_h holds the entries that cross the periodic seam --
        rows of plane 0 with columns in plane nz - 1 and the reverse, what a rank reads from its halo --, A_in the
        rest.  Three planes or more, so that no neighbour inside the box is also the one across the seam."""
        nx, ny, nz = shape
        assert nx * ny * nz == self.n and nz >= 3
        a = self.csr.tocoo()
        plane = a.row // (nx * ny), a.col // (nx * ny)
        seam = ((plane[0] == 0) & (plane[1] == nz - 1)) | ((plane[0] == nz - 1) & (plane[1] == 0))
        import scipy.sparse as sps

        part = lambda m: sps.coo_matrix((a.data[m].astype(np.float64), (a.row[m], a.col[m])), shape=a.shape).tocsr()  # noqa: E731
        assert int(seam.sum()) > 0
        return part(~seam), part(seam)

    def apply(self, w):
        w = np.asarray(w)
        if w.dtype == object:
            if self._obj is None:
                self._rows = np.repeat(np.arange(self.n), np.diff(self.csr.indptr))
                self._obj = self.csr.data.astype(object)
            out = np.zeros(self.n, dtype=object)
            np.add.at(out, self._rows, self._obj * w[self.csr.indices])
            return out
        assert w.dtype == np.int64 and int(np.abs(w).max(initial=0)) * self.rowsum < (1 << 62)
        return self.csr @ w

    def float64(self):
        """The same matrix with fp64 entries (the float64 restatements)."""
        return self.csr.astype(np.float64)


def true_residual(A, b, x):
    """||b - A x||_2 in ``np.longdouble`` for an fp64 x and an ``IntOperator`` A: every product is exact there (an
    integer of a few bits times 53 bits), the sums carry the long double's rounding."""
    a = A.csr
    ld = np.longdouble
    prod = a.data.astype(ld) * np.asarray(x, np.float64).astype(ld)[a.indices]
    r = np.asarray(b).astype(ld) - np.add.reduceat(prod, a.indptr[:-1])
    return float(np.sqrt(np.dot(r, r)))


class OpBasis(Basis):
    """``Basis`` over a general integer operator: W_0 = b, W_{t+1} = A W_t with A an ``IntOperator``.  int64 while
    max|W_t| * rowsum < 2^62 (3 * 20^t fits for t <= 13 with row sums of 20), Python integers beyond.  No
    preconditioner.  ``gram`` is the parent's: ``big_dot(W_i, W_j)`` for every pair -- A need not be symmetric, so
    <W_i, W_j> is no function of i + j."""

    def __init__(self, op, b):
        self.op, self.shape, self.n, self.pre = op, None, int(np.asarray(b).size), False
        assert op.n == self.n
        self.W = [np.asarray(b, np.int64)]
        self.R = []
        self._fixed, self._g, self._limb = {}, {}, {}

    def grow(self, t):
        while len(self.W) <= t:
            w = self.W[-1]
            if w.dtype != object and int(np.abs(w).max(initial=0)) * self.op.rowsum >= (1 << 62):
                w = w.astype(object)
            self.W.append(self.op.apply(w))

    def gram(self, i, j):
        """``big_dot(W_i, W_j)`` with the limbs of every int64 chain vector split once (all pairs are asked for)."""
        key = (min(i, j), max(i, j))
        if key not in self._g:
            self.grow(max(key[1], 0))
            bits = (62 - max(1, self.n).bit_length()) // 2
            if key[0] < 0 or self.W[key[1]].dtype == object or bits > 31:
                return Basis.gram(self, i, j)
            for t in key:
                if t not in self._limb:
                    self._limb[t] = [a.astype(np.int32) for a in _limbs(self.W[t], bits)]  # (|limb| < 2^bits)
            self._g[key] = Fraction(sum(int(np.dot(a.astype(np.int64), b.astype(np.int64))) << (bits * (s + t))
                                        for s, a in enumerate(self._limb[i]) for t, b in enumerate(self._limb[j])))
        return self._g[key]


class Space:
    """The coefficient-form vectors of a Basis.  ``drop_at``: the ordinal of one dot product (counted from 1 in call
    order) that leaves the last row out -- the defect a lost partial sum would make."""

    def __init__(self, basis, decimal=False):
        self.basis, self.decimal = basis, decimal
        self.one = Decimal(1) if decimal else Fraction(1)
        self.ndots, self.drop_at = 0, None

    def b(self):
        return Vec({0: self.one})

    def zero(self):
        return Vec({})

    def A(self, v):
        for k in v.c:
            assert k >= 0 and (not self.basis.pre or k % 2 == 1), "A applies to chain vectors of the other kind"
        return Vec({k + 1: c for k, c in v.c.items()})

    def P(self, v):
        assert self.basis.pre
        for k in v.c:
            assert k >= 0 and k % 2 == 0, "P applies to chain vectors of the other kind"
        s = Fraction(1, 1 << PRE_SHIFT)
        return Vec({k + 1: _mul(c, s) for k, c in v.c.items()})

    def fixed(self, values):
        return Vec({self.basis.fixed(values): self.one})

    def dot(self, u, v):
        self.ndots += 1
        drop = self.ndots == self.drop_at
        s = 0
        for i, ci in u.c.items():
            for j, cj in v.c.items():
                g = self.basis.gram(i, j)
                if drop:
                    g -= self.basis.last_row(i) * self.basis.last_row(j)
                s += _mul(_mul(ci, cj), g)
        return _dec(s) if self.decimal else Fraction(s)

    def magnitude(self, v):
        """M: the sum of the squared norms of the terms c_t W_t that form v."""
        return sum((_mul(_mul(c, c), self.basis.gram(k, k)) for k, c in v.c.items()), 0)

    def materialize(self, v):
        """The exact elements of a vector with Fraction coefficients, each rounded once to fp64."""
        den = 1
        for k, c in v.c.items():
            den = math.lcm(den, Fraction(c).denominator * self.basis._vec(k)[1])
        acc = np.zeros(self.basis.n, dtype=object)
        for k, c in v.c.items():
            u, d = self.basis._vec(k)
            acc = acc + int(Fraction(c) * den / d) * u.astype(object)
        return np.array([int(a) / den for a in acc])


class ElemSpace:
    """The same interface with every element held exactly (Fraction) or in PREC-digit decimals: the brute force.
    ``op``: an ``IntOperator`` in place of the unit box's ``-L`` (then ``shape`` is None)."""

    def __init__(self, shape, b, dinv=None, decimal=False, op=None):
        self.shape, self.decimal, self.op = (None if shape is None else tuple(shape)), decimal, op
        conv = _dec if decimal else Fraction
        with localcontext() as ctx:
            ctx.prec = PREC
            self._b = np.array([conv(int(v)) for v in b], dtype=object)
            self._dinv = None if dinv is None else np.array([conv(Fraction(float(v))) for v in dinv], dtype=object)
        self.ndots, self.drop_at = 0, None

    def b(self):
        return self._b.copy()

    def zero(self):
        return np.zeros(self._b.size, dtype=object)

    def A(self, v):
        return exact_apply(self.shape, v) if self.op is None else self.op.apply(v)

    def P(self, v):
        return self._dinv * v

    def fixed(self, values):
        conv = _dec if self.decimal else Fraction
        return np.array([conv(Fraction(float(x))) for x in values], dtype=object)

    def dot(self, u, v):
        self.ndots += 1
        n = u.size - (1 if self.ndots == self.drop_at else 0)
        s = sum((u[i] * v[i] for i in range(n)), 0)
        return _dec(s) if self.decimal else Fraction(s)


class Run:
    """What a method restated on a space gives: the exact squares of history[0..K] (``hist_sq``), x_K, and per
    history entry the vectors whose norms formed it (``feeds``: the floor of the tolerance reads their terms)."""

    def __init__(self, hist_sq, x, feeds, xs=None, ratio_sq=None):
        self.hist_sq, self.x, self.feeds = hist_sq, x, feeds
        if xs is not None:  # x_0 ... x_K and, per history entry, M / h^2 of the statements that formed it (``EnginePins``)
            self.xs, self.ratio_sq = xs, ratio_sq

    @property
    def history(self):
        with localcontext() as ctx:
            ctx.prec = PREC
            return [float(_dec(h).sqrt()) for h in self.hist_sq]


def _ops(sp, side):
    """``s <- op(y)`` with its intermediate z, as every method writes it: left P(z <- A y), right A(z <- P y)."""
    def op(y):
        if side == "left":
            z = sp.A(y)
            return sp.P(z), z
        if side == "right":
            z = sp.P(y)
            return sp.A(z), z
        return sp.A(y), None
    return op


CGS_X_DEFECTS = ("skip_x", "double_x", "x_wrong_side")
TFQMR_X_DEFECTS = ("d_wrong_vector", "x_sn_for_cs", "d_not_scaled")
TFQMR1_X_DEFECTS = ("copy_always", "copy_never")
BICGSTABL_X_DEFECTS = ("skip_x_mr", "gbb_shift")
BICGSTABL_DEFECTS = ("rho_without_omega", "beta_without_alpha")
IDRS_X_DEFECTS = ("skip_x_omega", "x_omega_wrong_side")


def cgs(sp, K, side=None, defect=None, at=None):
    """SolverCgs.hpp:57-174.  Besides ``Run``'s fields the result carries ``xs`` (x_0 ... x_K) and ``ratio_sq[k]``, M / h^2
    of history[k] from the step's own terms: r_k = r_{k-1} - alpha w, M = |r_{k-1}|^2 + alpha^2 |w|^2.

    ``defect`` (the separation tests only; ``at``: the 0-based iteration of the one-shot ones, None: every iteration):
      "stale_beta"   beta from the rho of the previous pass alone
      "shadow_r"     r for r~ in the shadow dots
      "skip_x"       x += alpha (u + q) left out at iteration ``at``
      "double_x"     ... applied twice at the last iteration
      "x_wrong_side" side right: x += alpha v, the vector after the apply, for alpha u, the one P gave"""
    assert defect != "x_wrong_side" or side == "right"
    b = sp.b()
    r = b  # :80 (x0 = 0)
    if side == "left":
        r = sp.P(r)  # :81-84
    rt = r  # :85
    shadow = (lambda: r) if defect == "shadow_r" else (lambda: rt)
    rho = sp.dot(rt, r)  # :86
    x, hist, feeds = sp.zero(), [rho], [[r]]
    xs, ratio = [x], [1]
    for it in range(K):
        if it == 0:
            u = r  # :113-115
            p = u
        else:
            rho_bar, rho = rho, sp.dot(shadow(), r)  # :117-118
            stale = defect == "stale_beta" and at in (None, it)
            beta = _sdiv(rho_bar if stale else rho, rho_bar)  # :119
            u = r + beta * q  # :120
            p = u + beta * (q + beta * p)  # :121
        if side == "left":
            q = sp.A(p)  # :136
            v = sp.P(q)
        elif side == "right":
            q = sp.P(p)  # :137
            v = sp.A(q)
        else:
            v = sp.A(p)  # :138
        alpha = _sdiv(rho, sp.dot(shadow(), v))  # :139
        q = u - alpha * v  # :140
        v = u + q  # :141
        r_old = r
        if side == "left":
            dx = alpha * v  # :160-162
            u = sp.A(v)
            v = sp.P(u)
            dr = alpha * v
        elif side == "right":
            u = sp.P(v)  # :164-166
            v = sp.A(u)
            dx = alpha * (v if defect == "x_wrong_side" else u)
            dr = alpha * v
        else:
            u = sp.A(v)  # :168-170
            dx = alpha * v
            dr = alpha * u
        if not (defect == "skip_x" and it == at):
            x = x + dx
        if defect == "double_x" and it == K - 1:
            x = x + dx
        r = r - dr
        hist.append(sp.dot(r, r))  # :173
        feeds.append([r])
        xs.append(x)
        ratio.append(_own_ratio(sp, [r_old, dr], hist[-1]))
    return Run(hist, x, feeds, xs, ratio)


def tfqmr(sp, K, side=None, l1=False, defect=None, at=None):
    """SolverTfqmr.hpp:44-209 (``l1``: TFQMR1).  Rational throughout in the squares: tau^2, omega^2 and the rotation's
    cs^2 = tau^2 / (tau^2 + omega^2), sn^2 = omega^2 / (tau^2 + omega^2) (sym_ortho, MathUtils.hpp:165-179); only the
    history takes a root.  ``xs``, and ``ratio_sq[k]`` from the two u -= alpha s of the iteration (the larger M / h^2);
    for TFQMR1 ``preds``, the outcome of omega < tau at every half-step.

    ``defect``: "stale_beta", "shadow_r" as for ``cgs``; of x alone
      "d_wrong_vector" side right: d += alpha y for alpha z
      "x_sn_for_cs"    x += sn^2 d for cs^2 d
      "d_not_scaled"   d *= sn^2 left out
      "copy_always", "copy_never"  TFQMR1: x <- d whatever omega < tau says, or never"""
    assert defect != "d_wrong_vector" or side == "right"
    op = _ops(sp, side)
    d = x = sp.zero()  # :74-78 (x0 = 0: d = x = 0 for both variants)
    y = sp.b()  # :79
    if side == "left":
        y = sp.P(y)  # :80-83
    u = y  # :84
    rt = u  # :85
    shadow = (lambda: u) if defect == "shadow_r" else (lambda: rt)
    rho = sp.dot(rt, u)  # :86
    tau2 = rho
    hist, feeds = [tau2], [[u]]
    xs, ratio, preds = [x], [1], []
    for it in range(K):
        if it == 0:
            s, z = op(y)  # :128-130
            v = s  # :131
        else:
            rho_bar, rho = rho, sp.dot(shadow(), u)  # :133-134
            stale = defect == "stale_beta" and at in (None, it)
            beta = _sdiv(rho_bar if stale else rho, rho_bar)  # :135
            v = s + beta * v  # :136
            y = u + beta * y  # :137
            s, z = op(y)  # :138-140
            v = s + beta * v  # :141
        alpha = _sdiv(rho, sp.dot(shadow(), v))  # :173
        fed, own = [], []
        for m in (0, 1):
            u_old, du = u, alpha * s
            u = u - du  # :175
            d = d + alpha * (z if side == "right" and defect != "d_wrong_vector" else y)  # :176
            om2 = sp.dot(u, u)  # :177
            fed.append(u)
            own.append(_own_ratio(sp, [u_old, du], om2))
            if l1:
                preds.append(bool(om2 < tau2))
                if preds[-1]:  # :178-179
                    tau2 = om2
                if defect == "copy_always" or (preds[-1] and defect != "copy_never"):
                    x = d
            else:
                h2 = tau2 + om2  # :181-184
                cs2, sn2 = (tau2 / h2, om2 / h2) if h2 > 0 else (sp.one, 0 * sp.one)
                tau2 = om2 * cs2
                x = x + (sn2 if defect == "x_sn_for_cs" else cs2) * d
                if defect != "d_not_scaled":
                    d = sn2 * d
            if m == 0:
                y = y - alpha * v  # :187
                s, z = op(y)  # :188-190
        hist.append(tau2 if l1 else tau2 * (2 * it + 3))  # :202-206
        feeds.append(fed)
        xs.append(x)
        ratio.append(max(own))
    run = Run(hist, x, feeds, xs, ratio)
    run.preds = preds
    return run


def bicgstab_l(sp, K, l, pre=False, defect=None, at=None):
    """SolverBiCgStab.hpp:194-375, BiCGStab(l); a preconditioner is always applied on the left (:226-229, :275-279,
    :295-299).  ``xs``, and ``ratio_sq[k]`` from the terms that form r_0 in the iteration: r_0, alpha u_1 and, at the end
    of a cycle, the gamma-bar_j r_j of the MR part.

    ``defect``: "stale_beta" (at iteration ``at``, None: every one), "shadow_r" as for ``cgs``;
      "rho_without_omega"  rho *= -omega at the end of a cycle left out
      "beta_without_alpha" beta = rho / rho-bar at iteration ``at``
    and of x alone, at the end of every cycle:
      "skip_x_mr"  x += gamma_1 r_0 left out
      "gbb_shift"  gamma-bar-bar_j formed from gamma_j ... for gamma_{j+1} ... (l >= 2)"""
    b = sp.b()
    r, u = [b] + [sp.zero()] * l, [sp.zero()] * (l + 1)  # :208-211, :224-225 (x0 = 0)
    if pre:
        r[0] = sp.P(r[0])  # :226-229
    rt = r[0]  # :230
    shadow = (lambda: r[0]) if defect == "shadow_r" else (lambda: rt)
    rho = sp.dot(rt, r[0])  # :231
    x, hist, feeds = sp.zero(), [rho], [[r[0]]]
    xs, ratio = [x], [1]
    alpha = None

    def apply(v):
        return sp.P(sp.A(v)) if pre else sp.A(v)

    tau, sigma, gbar, gam, gbb = {}, {}, {}, {}, {}
    for it in range(K):
        j = it % l  # Solver.hpp:239
        if it == 0:
            u[0] = r[0]  # :265-266
        else:
            rho_bar, rho = rho, sp.dot(shadow(), r[j])  # :268-269
            stale = defect == "stale_beta" and at in (None, it)
            a = 1 if defect == "beta_without_alpha" and it == at else alpha
            beta = _sdiv(a * (rho_bar if stale else rho), rho_bar)  # :270
            for i in range(j + 1):
                u[i] = r[i] - beta * u[i]  # :271-273
        u[j + 1] = apply(u[j])  # :275-279
        alpha = _sdiv(rho, sp.dot(shadow(), u[j + 1]))  # :280
        terms = [r[0], alpha * u[1]]
        for i in range(j + 1):
            r[i] = r[i] - alpha * u[i + 1]  # :281-283
        x = x + alpha * u[0]  # :294
        r[j + 1] = apply(r[j])  # :295-299
        if j == l - 1:
            for jj in range(1, l + 1):  # :313-322
                for i in range(1, jj):
                    tau[i, jj] = _sdiv(sp.dot(r[i], r[jj]), sigma[i])
                    r[jj] = r[jj] - tau[i, jj] * r[i]
                sigma[jj] = sp.dot(r[jj], r[jj])
                gbar[jj] = _sdiv(sp.dot(r[0], r[jj]), sigma[jj])
            omega = gam[l] = gbar[l]  # :339
            if defect != "rho_without_omega":
                rho = rho * -omega
            for jj in range(l - 1, 0, -1):  # :340-345
                gam[jj] = gbar[jj]
                for i in range(jj + 1, l + 1):
                    gam[jj] = gam[jj] - tau[jj, i] * gam[i]
            sh = 0 if defect == "gbb_shift" else 1
            for jj in range(1, l):  # :346-351
                gbb[jj] = gam[jj + sh]
                for i in range(jj + 1, l):
                    gbb[jj] = gbb[jj] + tau[jj, i] * gam[i + sh]
            terms += [gbar[jj] * r[jj] for jj in range(1, l + 1)]
            if defect != "skip_x_mr":
                x = x + gam[1] * r[0]  # :364-366
            r[0] = r[0] - gbar[l] * r[l]
            u[0] = u[0] - gam[l] * u[l]
            for jj in range(1, l):  # :367-371
                x = x + gbb[jj] * r[jj]
                r[0] = r[0] - gbar[jj] * r[jj]
                u[0] = u[0] - gam[jj] * u[jj]
        hist.append(sp.dot(r[0], r[0]))  # :374
        feeds.append([r[0]])
        xs.append(x)
        ratio.append(_own_ratio(sp, terms, hist[-1]))
    return Run(hist, x, feeds, xs, ratio)


def richardson(sp, K, omega, pre=False):
    """SolverRichardson.hpp:51-96: the preconditioner, if any, acts on the residual (left) whatever the side.  ``xs``, and
    ``ratio_sq[k]`` from r = b - A x (both under P with a preconditioner)."""
    b = sp.b()
    x, r = sp.zero(), b  # :65 (x0 = 0)
    pb = b
    if pre:
        r = pb = sp.P(r)  # :66-69
    hist, feeds = [sp.dot(r, r)], [[r]]  # :71
    xs, ratio = [x], [1]
    for _ in range(K):
        x = x + omega * r  # :88
        ax = sp.A(x)
        r = b - ax  # :89
        if pre:
            r = sp.P(r)  # :90-93
        hist.append(sp.dot(r, r))  # :95
        feeds.append([r])
        xs.append(x)
        ratio.append(_own_ratio(sp, [pb, sp.P(ax) if pre else ax], hist[-1]))
    return Run(hist, x, feeds, xs, ratio)


def _own_ratio(sp, terms, h_sq):
    """M / h^2 of one step: M the sum of the squared norms of the step's own terms, h^2 the squared norm of the vector
    they form.  The dots are not counted (``ndots``, ``drop_at`` are the method's)."""
    n, drop, sp.drop_at = sp.ndots, sp.drop_at, None
    m = sum((sp.dot(t, t) for t in terms), 0)
    sp.ndots, sp.drop_at = n, drop
    return m / h_sq if h_sq else 0 * m


def _dot_without_last_row(sp, u, v):
    sp.drop_at = sp.ndots + 1
    d = sp.dot(u, v)
    sp.drop_at = None
    return d


CG_DEFECTS = ("stale_gamma", "old_r", "skip_x", "double_x", "stale_pz", "old_p", "drop_row")
BICGSTAB_DEFECTS = ("beta_no_ratio", "stale_omega", "skip_x_omega", "old_v", "rho_early")
# defects of the halo alone: a space whose ``A(v, halo_of=u)`` reads the rows across the periodic seam from u
# (``Float64Space`` with its split); they change two planes of one operand of one apply
CG_HALO_DEFECTS = ("halo_stale_p", "halo_old_beta")
BICGSTAB_HALO_DEFECTS = ("halo_s_old_alpha", "halo_p_old_omega")


def cg(sp, K, pre=False, defect=None, at=2):
    """SolverCg.hpp:54-126; the preconditioner has no side (z = P r).  Besides ``Run``'s fields the result carries
    ``xs`` (x_0 ... x_K) and ``ratio_sq[k]``, M / h^2 of history[k] from the step's OWN terms: r_k = r_{k-1} - alpha z,
    M = |r_{k-1}|^2 + alpha^2 |z|^2, h = |r_k| -- what ``floor_tol`` takes after a root (``StepPins``).

    ``defect`` (the separation tests only; none acts before the second iteration, so history[0..1] and x_1 keep their
    values -- ``at`` is the 0-based iteration of the one-shot ones):
      "stale_gamma"  beta = gamma_k / gamma_0: the gamma-bar register never refreshed
      "old_r"        p' = r + beta p with the r of before r -= alpha z
      "skip_x"       x += alpha p left out at iteration ``at``
      "double_x"     x += alpha p applied twice at the last iteration (the tail kernel after a fused step)
      "stale_pz"     alpha from the previous iteration's <p, z>
      "old_p"        p' = r + beta p_{k-2} at iteration ``at`` (the wrong buffer of the ping-pong)
      "drop_row"     <r, r> of iteration ``at`` - 1 without its last row (history[``at``])
    and in the halo (``CG_HALO_DEFECTS``):
      "halo_stale_p"  z = A_in p + A_h p_prev at iteration ``at``: the exchange did not happen, or was not waited for
      "halo_old_beta" from iteration 1 on the halo rows of p' are r + beta_prev p, the previous iteration's beta"""
    assert defect is None or (defect in CG_DEFECTS + CG_HALO_DEFECTS and at >= 1 and not pre)
    b = sp.b()
    x, r = sp.zero(), b  # :73 (x0 = 0)
    if pre:
        z = sp.P(r)  # :74-77
        p = z
        gamma = sp.dot(r, z)
    else:
        p = r  # :79-80
        gamma = sp.dot(r, r)
    hist, feeds = [sp.dot(r, r) if pre else gamma], [[r]]  # :83
    xs, ratio = [x], [1]
    gamma_0, pz_prev, p_prev = gamma, None, None
    p_halo = beta_prev = None  # (what the halo holds where it is not p: the halo defects)
    for it in range(K):
        if defect == "halo_stale_p" and it == at:
            z = sp.A(p, halo_of=p_prev)
        elif p_halo is not None:
            z = sp.A(p, halo_of=p_halo)
        else:
            z = sp.A(p)  # :96
        pz = sp.dot(p, z)
        alpha = _sdiv(gamma, pz_prev if defect == "stale_pz" and it >= 1 else pz)  # :97
        pz_prev = pz
        if not (defect == "skip_x" and it == at):
            x = x + alpha * p  # :98
        if defect == "double_x" and it == K - 1 and it >= 1:
            x = x + alpha * p
        r_old, az = r, alpha * z
        r = r - az  # :99
        gamma_bar = gamma  # :110
        if pre:
            z = sp.P(r)  # :111-113
            gamma = sp.dot(r, z)
        elif defect == "drop_row" and it == at - 1:
            gamma = _dot_without_last_row(sp, r, r)
        else:
            gamma = sp.dot(r, r)  # :115
        beta = _sdiv(gamma, gamma_0 if defect == "stale_gamma" else gamma_bar)  # :122
        lead = z if pre else (r_old if defect == "old_r" and it >= 1 else r)
        p_halo = lead + beta_prev * p if defect == "halo_old_beta" and it >= 1 else None
        beta_prev = beta
        p_prev, p = p, lead + beta * (p_prev if defect == "old_p" and it == at else p)  # :123
        hist.append(sp.dot(r, r) if pre else gamma)  # :125
        feeds.append([r])
        xs.append(x)
        ratio.append(_own_ratio(sp, [r_old, az], hist[-1]))
    run = Run(hist, x, feeds)
    run.xs, run.ratio_sq = xs, ratio
    return run


def bicgstab(sp, K, defect=None, at=2):
    """SolverBiCgStab.hpp:53-167, plain BiCGStab from x0 = 0 without a preconditioner -- what api.BiCgStabSolver and
    oracle.solve("bicgstab", ...) implement.  Rational throughout; only the history takes a root.  ``xs`` and
    ``ratio_sq`` as ``cg`` records them: r_k = r_{k-1} - alpha v - omega t, M = |r_{k-1}|^2 + alpha^2 |v|^2 +
    omega^2 |t|^2.

    ``defect`` (none acts before the second iteration; ``at``: the 0-based iteration of the one-shot ones):
      "beta_no_ratio" beta = rho / rho-bar, the factor alpha / omega left out
      "stale_omega"   p = r + beta (p - omega v) with the omega of the iteration before the last (from iteration 2 on)
      "skip_x_omega"  x += omega r left out at iteration ``at``
      "old_v"         v_{k-2} read for v_{k-1} in p at iteration ``at`` (the wrong parity buffer)
      "rho_early"     rho = <r~, r> with the r of before r -= omega t
    and in the halo (``BICGSTAB_HALO_DEFECTS``):
      "halo_s_old_alpha" from iteration 1 on t = A_in s + A_h (r - alpha_prev v): the halo rows of s with the alpha of
                         the iteration before
      "halo_p_old_omega" from iteration 2 on the halo rows of p' are r + beta (p - omega_prev v), the omega before the last"""
    assert defect is None or (defect in BICGSTAB_DEFECTS + BICGSTAB_HALO_DEFECTS and at >= 2)
    r = sp.b()  # :82 (x0 = 0)
    rt = r  # :87
    rho = sp.dot(rt, r)  # :88
    x, hist, feeds = sp.zero(), [rho], [[r]]
    xs, ratio = [x], [1]
    alpha = omega = omega_prev = v = v_prev = s = None
    for it in range(K):
        if it == 0:
            p = r  # :114
        else:
            rho_bar, rho = rho, sp.dot(rt, s if defect == "rho_early" else r)  # :116-117
            beta = _sdiv(rho, rho_bar) if defect == "beta_no_ratio" else _sdiv(alpha * rho, omega * rho_bar)  # :118
            om = omega_prev if defect == "stale_omega" and it >= 2 else omega
            p_halo = r + beta * (p - omega_prev * v) if defect == "halo_p_old_omega" and it >= 2 else None
            p = r + beta * (p - om * (v_prev if defect == "old_v" and it == at else v))  # :119
        v_prev, v = v, (sp.A(p) if it == 0 or p_halo is None else sp.A(p, halo_of=p_halo))  # :137
        alpha_prev, alpha = alpha, _sdiv(rho, sp.dot(rt, v))  # :139
        x = x + alpha * p  # :140
        r_old, av = r, alpha * v
        r = s = r - av  # :141
        if defect == "halo_s_old_alpha" and it >= 1:
            t = sp.A(r, halo_of=r_old - alpha_prev * v)
        else:
            t = sp.A(r)  # :158
        omega_prev, omega = omega, _sdiv(sp.dot(t, r), sp.dot(t, t))  # :159-160
        if not (defect == "skip_x_omega" and it == at):
            x = x + omega * r  # :161
        ot = omega * t
        r = r - ot  # :162
        hist.append(sp.dot(r, r))  # :164
        feeds.append([r])
        xs.append(x)
        ratio.append(_own_ratio(sp, [r_old, av, ot], hist[-1]))
    run = Run(hist, x, feeds)
    run.xs, run.ratio_sq = xs, ratio
    return run


class Float64Space:
    """The vector interface in plain fp64 numpy over a scipy CSR matrix: the method bodies above become float64
    restatements, with their defects.  ``a_halo``: the optional split A = a + a_halo (``IntOperator.seam_split``), a
    the entries inside the box and a_halo those across the periodic seam; ``A(v, halo_of=u)`` then multiplies a_halo by u
    in place of v -- a halo that holds something else than the vector it belongs to."""

    one, scalar, root = 1.0, float, staticmethod(math.sqrt)  # (the scalars of ``tfqmr`` and ``idrs`` in fp64)

    def __init__(self, a, b, a_halo=None, dinv=None):
        self.a, self.a_halo, self._b = a, a_halo, np.asarray(b, np.float64)
        self._dinv = None if dinv is None else np.asarray(dinv, np.float64)
        self.ndots, self.drop_at = 0, None

    def P(self, v):
        return self._dinv * v

    def fixed(self, values):
        return np.asarray(values, np.float64).copy()

    def b(self):
        return self._b.copy()

    def zero(self):
        return np.zeros(self._b.size)

    def A(self, v, halo_of=None):
        if self.a_halo is None:
            assert halo_of is None, "a halo defect needs the split A = A_in + A_h"
            return self.a @ v
        return self.a @ v + self.a_halo @ (v if halo_of is None else halo_of)

    def dot(self, u, v):
        self.ndots += 1
        if self.ndots == self.drop_at:
            return float(np.dot(u[:-1], v[:-1]))
        return float(np.dot(u, v))


def _float64_run(method, a, b, K, defect, at, a_halo=None):
    run = method(Float64Space(a, b, a_halo), K, defect=defect, at=at)
    return np.sqrt(np.array(run.hist_sq, np.float64)), run.xs


def cg_float64(a, b, K, defect=None, at=2, a_halo=None):
    """CG's history[0..K] and x_0 ... x_K in plain fp64 numpy (``a``: scipy CSR, fp64): ``cg``'s statements, and the
    defects the pins must reject (``CG_DEFECTS``; with the split ``a`` + ``a_halo`` also ``CG_HALO_DEFECTS``)."""
    return _float64_run(cg, a, b, K, defect, at, a_halo)


def bicgstab_float64(a, b, K, defect=None, at=2, a_halo=None):
    """BiCGStab's history[0..K] and x_0 ... x_K in plain fp64 numpy, with ``BICGSTAB_DEFECTS`` (and, with the split,
    ``BICGSTAB_HALO_DEFECTS``)."""
    return _float64_run(bicgstab, a, b, K, defect, at, a_halo)


def _root(v):
    return _dec(v).sqrt()


def idrs(sp, K, s, shadow=(), side=None, prec=None, defect=None, at=None):
    """SolverIdrs.hpp:62-283, IDR(s), in decimals of ``prec`` digits (PREC; p_0 = r / |r| and the normalisations take
    roots); every dot is exact before its one conversion.  ``shadow``: the s - 1 fp64 vectors fill_randomly draws for
    p_1 ... p_{s-1}.  ``xs``, and ``ratio_sq[k]`` from r -= beta g_k and, at the end of a cycle, r -= omega v.  A space
    may bring its own scalars (``scalar``, ``root``: ``Float64Space``).

    ``defect`` (of x alone, at the end of the cycle that iteration ``at`` closes):
      "skip_x_omega"        x += omega r left out
      "x_omega_wrong_side"  side right: x += omega r for omega z, z = P r"""
    assert defect != "x_omega_wrong_side" or side == "right"
    op = _ops(sp, side)
    dec, root = getattr(sp, "scalar", _dec), getattr(sp, "root", _root)
    with localcontext() as ctx:
        ctx.prec = prec or PREC
        r = sp.b()  # :94 (x0 = 0)
        if side == "left":
            r = sp.P(r)  # :95-98
        phi, gamma, mu = [dec(0)] * s, [dec(0)] * s, {}
        phi[0] = root(sp.dot(r, r))  # :99
        x, hist, feeds = sp.zero(), [phi[0] * phi[0]], [[r]]
        xs, ratio = [x], [1]
        g, u, p = [sp.zero()] * s, [sp.zero()] * s, [None] * s
        omega = None
        for it in range(K):
            k = it % s  # Solver.hpp:239
            if k == 0:
                if it == 0:
                    omega = mu[0, 0] = dec(1)  # :131
                    p[0] = r / phi[0]  # :132
                    for i in range(1, s):  # :133-141
                        mu[i, i], phi[i] = dec(1), dec(0)
                        p[i] = sp.fixed(shadow[i - 1])
                        for j in range(i):
                            mu[i, j] = dec(0)
                            p[i] = p[i] - dec(sp.dot(p[i], p[j])) * p[j]
                        p[i] = p[i] / root(sp.dot(p[i], p[i]))
                else:
                    for i in range(s):  # :143-145
                        phi[i] = dec(sp.dot(p[i], r))
            for i in range(k, s):  # :167-173
                gamma[i] = phi[i]
                for j in range(k, i):
                    gamma[i] -= mu[i, j] * gamma[j]
                gamma[i] /= mu[i, i]
            v = r - gamma[k] * g[k]  # :195
            for i in range(k + 1, s):
                v = v - gamma[i] * g[i]  # :196-198
            if side == "right":
                v = sp.P(v)  # :199-202
            u[k] = omega * v + gamma[k] * u[k]  # :203
            for i in range(k + 1, s):
                u[k] = u[k] + gamma[i] * u[i]  # :204-206
            g[k] = sp.P(sp.A(u[k])) if side == "left" else sp.A(u[k])  # :207-211
            for i in range(k):  # :221-226
                a = _sdiv(dec(sp.dot(p[i], g[k])), mu[i, i])
                u[k] = u[k] - a * u[i]
                g[k] = g[k] - a * g[i]
            for i in range(k, s):
                mu[i, k] = dec(sp.dot(p[i], g[k]))  # :234-236
            beta = _sdiv(phi[k], mu[k, k])  # :244
            x = x + beta * u[k]  # :245
            terms = [r, beta * g[k]]
            r = r - beta * g[k]  # :246
            for i in range(k + 1, s):
                phi[i] -= beta * mu[i, k]  # :254-256
            if k == s - 1:
                v, z = op(r)  # :272-274
                omega = _sdiv(dec(sp.dot(v, r)), dec(sp.dot(v, v)))  # :276-277
                if not (defect == "skip_x_omega" and it == at):
                    wrong = defect == "x_omega_wrong_side" and it == at
                    x = x + omega * (z if side == "right" and not wrong else r)  # :278
                terms.append(omega * v)
                r = r - omega * v  # :279
            hist.append(dec(sp.dot(r, r)))  # :282
            feeds.append([r])
            xs.append(x)
            ratio.append(_own_ratio(sp, terms, hist[-1]))
    return Run(hist, x, feeds, xs, ratio)


def fgmres(sp, K, m, prec=None):
    """SolverGmres.hpp:51-249 with Flexible = true: a preconditioner is applied on the right whatever the side
    (:69-70, :125-130), z_k = P q_k kept per k (:152-153), x += sum beta_i z_i at the end of a cycle (:237-240) and at
    exit inside one (Solver.hpp:253-255).  ``xs[k]``: the x the solver leaves after k iterations -- inner_finalize on
    the Hessenberg columns formed so far; ``ratio_sq[k]`` as ``gmres`` records its ratio: w = A z_k - sum_i H_ik q_i,
    M = |A z_k|^2 + sum_i H_ik^2, h = H_{k+1,k}, the largest over the steps of the cycle so far.  Without a
    preconditioner (``sp.P`` absent from the chain) z_k = q_k."""
    pre = sp.basis.pre if hasattr(sp, "basis") else sp._dinv is not None
    with localcontext() as ctx:
        ctx.prec = prec or PREC
        b = sp.b()
        x = sp.zero()
        q, z, H, cs, sn, beta = [None] * (m + 1), [None] * m, {}, [None] * m, [None] * m, [Decimal(0)] * (m + 1)
        hist, feeds = [], []
        xs, ratio = [x], [1]

        def finalized(k):  # inner_finalize, :207-240, on a copy of beta
            y = list(beta)
            for i in range(k, -1, -1):
                for j in range(i + 1, k + 1):
                    y[i] -= H[i, j] * y[j]
                y[i] /= H[i, i]
            out = x
            for i in range(k + 1):
                out = out + y[i] * z[i]
            return out

        for it in range(K + 1):
            if it == 0 or it % m == 0:  # outer_init (:82-88) and inner_init (:110-116) alike
                q[0] = b - sp.A(x) if it else b
                beta[0] = _root(sp.dot(q[0], q[0]))
                if it == 0:
                    hist.append(beta[0] * beta[0])
                    feeds.append([q[0]])
                q[0] = q[0] / beta[0]
                worst = Decimal(0)
            if it == K:
                break
            k = it % m
            z[k] = sp.P(q[k]) if pre else q[k]  # :152-153
            w = sp.A(z[k])
            mag = _dec(sp.dot(w, w))
            for i in range(k + 1):  # :157-160
                H[i, k] = _dec(sp.dot(w, q[i]))
                w = w - H[i, k] * q[i]
                mag += H[i, k] * H[i, k]
            H[k + 1, k] = _root(sp.dot(w, w))  # :161
            q[k + 1] = w / H[k + 1, k]  # :162
            worst = max(worst, mag / (H[k + 1, k] * H[k + 1, k]))
            for i in range(k):  # :176-180
                chi = cs[i] * H[i, k] + sn[i] * H[i + 1, k]
                H[i + 1, k] = -sn[i] * H[i, k] + cs[i] * H[i + 1, k]
                H[i, k] = chi
            rr = (H[k, k] ** 2 + H[k + 1, k] ** 2).sqrt()  # :181, MathUtils.hpp:165-179
            cs[k], sn[k] = (H[k, k] / rr, H[k + 1, k] / rr) if rr > 0 else (Decimal(1), Decimal(0))
            H[k, k] = cs[k] * H[k, k] + sn[k] * H[k + 1, k]  # :182-183
            H[k + 1, k] = Decimal(0)
            beta[k + 1], beta[k] = -sn[k] * beta[k], cs[k] * beta[k]  # :189
            hist.append(beta[k + 1] * beta[k + 1])  # :191
            feeds.append([w])
            xs.append(finalized(k))
            ratio.append(worst)
            if k == m - 1:
                x = xs[-1]
    return Run(hist, xs[-1], feeds, xs, ratio)


def gmres(sp, K, m, prec=None):
    """SolverGmres.hpp:51-249 with Flexible = false and no preconditioner: ``fgmres`` with z_k = q_k, and with
    inner_finalize where the solver calls it -- at the end of every cycle (Solver.hpp:244-246) and at exit after K
    steps when the last cycle is unfinished (Solver.hpp:253-255) -- so x is what the solver leaves.  ``prec``: the
    decimal digits (PREC).  Besides ``Run``'s fields the result carries ``ratio[k]``, sqrt(M) / h for history[k] as
    ``floor_tol`` takes it: the vector a step forms is w = A q_k - sum_i H_ik q_i, its terms have the squared norms
    |A q_k|^2 and H_ik^2 (|q_i| = 1), and h is |w| = H_{k+1,k}; the largest over the steps of the cycle so far, since
    history[k + 1] is a product of all their rotations."""
    with localcontext() as ctx:
        ctx.prec = prec or PREC
        b = sp.b()
        x = sp.zero()
        q, H, cs, sn, beta = [None] * (m + 1), {}, [None] * m, [None] * m, [Decimal(0)] * (m + 1)
        hist, feeds, ratio = [], [], [Decimal(1)]

        def finalize(k):  # inner_finalize, :207-236
            nonlocal x
            for i in range(k, -1, -1):
                for j in range(i + 1, k + 1):
                    beta[i] -= H[i, j] * beta[j]  # :209
                beta[i] /= H[i, i]  # :211
            for i in range(k + 1):
                x = x + beta[i] * q[i]  # :234-236

        for it in range(K):
            k = it % m  # Solver.hpp:239
            if k == 0:  # outer_init (:82-88) at it = 0, inner_init (:110-116) at the head of every cycle
                q[0] = b - sp.A(x) if it else b  # :82, :110
                beta[0] = _root(sp.dot(q[0], q[0]))  # :87, :115
                if it == 0:
                    hist.append(beta[0] * beta[0])  # :90
                    feeds.append([q[0]])
                q[0] = q[0] / beta[0]  # :88, :116
                worst = Decimal(0)
            w = sp.A(q[k])  # :155
            mag = _dec(sp.dot(w, w))
            for i in range(k + 1):  # :157-160
                H[i, k] = _dec(sp.dot(w, q[i]))  # :158
                w = w - H[i, k] * q[i]  # :159
                mag += H[i, k] * H[i, k]
            H[k + 1, k] = _root(sp.dot(w, w))  # :161
            q[k + 1] = w / H[k + 1, k]  # :162
            worst = max(worst, mag.sqrt() / H[k + 1, k])
            for i in range(k):  # :176-180
                chi = cs[i] * H[i, k] + sn[i] * H[i + 1, k]  # :177
                H[i + 1, k] = -sn[i] * H[i, k] + cs[i] * H[i + 1, k]  # :178
                H[i, k] = chi  # :179
            rr = (H[k, k] ** 2 + H[k + 1, k] ** 2).sqrt()  # :181, MathUtils.hpp:165-179
            cs[k], sn[k] = (H[k, k] / rr, H[k + 1, k] / rr) if rr > 0 else (Decimal(1), Decimal(0))
            H[k, k] = cs[k] * H[k, k] + sn[k] * H[k + 1, k]  # :182
            H[k + 1, k] = Decimal(0)  # :183
            beta[k + 1], beta[k] = -sn[k] * beta[k], cs[k] * beta[k]  # :189
            hist.append(beta[k + 1] * beta[k + 1])  # :191
            feeds.append([w])
            ratio.append(worst)
            if k == m - 1:
                finalize(k)  # Solver.hpp:244-246
        if K and (K - 1) % m != m - 1:
            finalize((K - 1) % m)  # Solver.hpp:253-255
    run = Run(hist, x, feeds)
    run.ratio = [float(r) for r in ratio]
    return run


def mgs_float64(a, b, K, m, defect=None, group=None, drop=(3, 1)):
    """GMRES(m)'s history[0..K] in plain fp64 numpy (``a``: scipy CSR, fp64), the same statements as ``gmres``.

    ``group`` = T: the projections of a step taken T at a time the way the device's chain kernels take them -- the T
    dots of a group against the SAME w, the one from before the group, then regrouped by bilinearity,
    h_{i+v} = <w, q_{i+v}> - sum_{u<v} h_{i+u} <q_{i+u}, q_{i+v}>, then w -= sum_v h_{i+v} q_{i+v}.  Not a defect.

    ``defect`` (what the pins must reject):
      "skip_q0"     the projection on q_0 dropped for k >= 2
      "skip_in_group" the projection on q_2 dropped for k >= 4 (one of a group of four)
      "drop_row"    the dot <w, q_i> of step k, (k, i) = ``drop``, without its last row
      "rotation_order" the earlier rotations of a column applied last first"""
    b = np.asarray(b, np.float64)
    n = b.size
    x = np.zeros(n)
    q, H = [None] * (m + 1), np.zeros((m + 1, m))
    cs, sn, beta = np.zeros(m), np.zeros(m), np.zeros(m + 1)
    hist = []
    for it in range(K):
        k = it % m
        if k == 0:
            q[0] = b - a @ x if it else b.copy()
            beta[0] = math.sqrt(np.dot(q[0], q[0]))
            if it == 0:
                hist.append(beta[0])
            q[0] = q[0] / beta[0]
        w = a @ q[k]
        i = 0
        while i <= k:
            T = min(group or 1, k + 1 - i)
            w0 = w
            for v in range(T):
                j = i + v
                if defect == "drop_row" and (k, j) == tuple(drop):
                    h = np.dot(w0[:-1], q[j][:-1])
                else:
                    h = np.dot(w0, q[j])
                for u in range(v):
                    h -= H[i + u, k] * np.dot(q[i + u], q[j])
                if (defect == "skip_q0" and j == 0 and k >= 2) or (defect == "skip_in_group" and j == 2 and k >= 4):
                    h = 0.0
                H[j, k] = h
            for v in range(T):
                w = w - H[i + v, k] * q[i + v]
            i += T
        H[k + 1, k] = math.sqrt(np.dot(w, w))
        q[k + 1] = w / H[k + 1, k]
        order = range(k - 1, -1, -1) if defect == "rotation_order" else range(k)
        for i in order:
            chi = cs[i] * H[i, k] + sn[i] * H[i + 1, k]
            H[i + 1, k] = -sn[i] * H[i, k] + cs[i] * H[i + 1, k]
            H[i, k] = chi
        rr = math.hypot(H[k, k], H[k + 1, k])
        cs[k], sn[k] = (H[k, k] / rr, H[k + 1, k] / rr) if rr > 0 else (1.0, 0.0)
        H[k, k] = cs[k] * H[k, k] + sn[k] * H[k + 1, k]
        H[k + 1, k] = 0.0
        beta[k + 1], beta[k] = -sn[k] * beta[k], cs[k] * beta[k]
        hist.append(abs(beta[k + 1]))
        if k == m - 1 and it + 1 < K:
            y = np.linalg.solve(np.triu(H[:m, :m]), beta[:m])
            for i in range(m):
                x = x + y[i] * q[i]
    return np.array(hist)


# ---- what the tests pin, and how tightly -----------------------------------------------------------------------------

DECIMAL_METHODS = ("idrs", "fgmres")
OMEGA = Fraction(1, 32)  # Richardson's relaxation_factor in the pins: 2^-5 keeps every x_k and r_k dyadic
TOL_CAP = 1e-10  # a measured tolerance above this could not tell a dropped row (~1/n) from rounding


def iterations(method, param, pre):
    """K, the iterations pinned: two for CGS, TFQMR(1), Richardson and every preconditioned case; the whole first
    cycle of BiCGStab(l) with its MR part (one more for l = 2); s + 1 for IDR(s), which reaches the next cycle's dots."""
    if pre or method in ("cgs", "tfqmr", "tfqmr1", "richardson", "cg", "fgmres"):
        return 2
    return param + 1 if method == "idrs" or param == 2 else param


def shadow_vectors(oracle, n, s):
    """p_1 ... p_{s-1} of IDR(s): fill_randomly's sequence from a fresh generator, n values each in turn."""
    oracle.rng_reset()
    return [oracle.fill_randomly(n) for _ in range(s - 1)]


def exact_run(sp, method, param, K, side=None, shadow=(), prec=None, defect=None, at=None):
    """The method restated on a space (``Space`` or ``ElemSpace``, decimal for DECIMAL_METHODS; ``Float64Space`` for the
    defects); ``side`` None: no preconditioner, else the space's dinv on that side (or the method's own).  ``prec``: the
    digits of the decimal methods (PREC)."""
    pre = side is not None
    kw = {} if defect is None else dict(defect=defect, at=at)
    if method == "cgs":
        return cgs(sp, K, side, **kw)
    if method in ("tfqmr", "tfqmr1"):
        return tfqmr(sp, K, side, l1=method == "tfqmr1", **kw)
    if method == "bicgstabl":
        return bicgstab_l(sp, K, param, pre=pre, **kw)
    if method == "idrs":
        return idrs(sp, K, param, shadow, side, prec=prec, **kw)
    assert defect is None
    if method == "richardson":
        return richardson(sp, K, OMEGA, pre=pre)
    if method == "cg":
        return cg(sp, K, pre=pre)
    if method == "fgmres":
        return fgmres(sp, K, param, prec=prec)
    raise ValueError(method)


# c of the floor rule at history[1], no preconditioner, from the statements that touch the vector since r0 (fp64, no
# fma contraction): a statement a u + b v rounds an element at most twice, an apply of a non-integer vector at most 13
# times (7 products, 6 sums), a scalar once per division or root; an error that then passes through an apply grows by
# at most ||A|| <= 12 (row sums of |A| on the unit box).
#   CGS     v = A p exact (p = b); alpha 1; q = u - alpha v 2; v = u + q 1; u = A v 13 + 12 (2 + 1 + 1);
#           r = r - alpha u 2 + 1                                                                        -> 64
#   TFQMR1  s = A y exact; alpha 1; u -= alpha s 2 + 1; y -= alpha v 2 + 1, s = A y 13 + 12 * 3;
#           u -= alpha s 2 + 1 on top of the first 3                                                       -> 54
#   TFQMR   the same and the rotation's hypot, divisions and product, 5                                   -> 59
#   IDR(s)  phi_0 = |r| 1; p_0 = r / phi_0 1; mu_00 = <p_0, g_0>, beta = phi_0 / mu_00 2 (g_0 = A r exact);
#   s > 1   r -= beta g_0 2 + 1                                                                            -> 7
#   IDR(1)  then v = A r 13 + 12 * 7; omega 1; r -= omega v 2 + 7                                          -> 107
#   Richardson: every vector exact (``richardson_integers``)                                               -> 0
#   GMRES   q_0 = b / beta 1 + 1; w = A q_k 13; per projection h 1, w -= h q_i 2 (the terms of M count every one);
#   FGMRES  |w| 1, q_{k+1} = w / |w| 1; the rotation's hypot, divisions and products ~8                   -> 32
#           (``gmres`` takes sqrt(M) / h from the step's own terms -- A q_k and the H_ik q_i -- not from the chain)
#   BiCGStab v = A p exact (p = b); alpha 1; s = r - alpha v 2; t = A s 13 + 12 (1 + 2); omega 1;
#           r = s - omega t 2 on top of s's 3                                                             -> 55
#           (``cg`` and ``bicgstab`` record sqrt(M) / h from the step's own terms as well: ``StepPins``)
# Later iterations and the preconditioned cases repeat these statements: c_k = k c_1 (+ 4k + 1 with the elementwise
# products of a preconditioner) is their floor; there the measured error of the oracle decides (``Pins``).
C1 = {"cgs": 64, "tfqmr": 59, "tfqmr1": 54, "idrs": 7, "idrs1": 107, "richardson": 0, "bicgstabl": 64, "cg": 16,
      "fgmres": 32, "gmres": 32, "bicgstab": 55}


def _c(method, param, k, pre):
    c1 = C1["idrs1" if method == "idrs" and param == 1 else method]
    return k * c1 + (4 * k + 1 if pre else 0)


def floor_tol(n, ratio, c):
    """2^-53 (D + c sqrt(M) / h): ``tolerance`` with the ratio sqrt(M) / h given."""
    return (fold_depth(n) + c * ratio) * 2.0 ** -53


def oracle_histories(oracle, g, b, method, param, K, side=None, dinv=None):
    """history[0..K] of the CPU oracle on the same data, in both of its arithmetic variants."""
    out = {}
    bf = np.asarray(b, np.float64)
    for variant in ("strict", "fma"):
        op = oracle.StencilOperator(g, -1.0, 0.0, variant=variant)
        pre = None if dinv is None else oracle.DiagOperator(dinv, variant=variant)
        common = dict(num_iterations=K, abs_tol=0.0, rel_tol=0.0, variant=variant)
        if method == "fgmres":
            r, _ = oracle.solve_gmres_pre(op, pre, bf, side=side, flexible=True, num_inner_iterations=param, **common)
        else:
            kw = {}
            if method in ("bicgstabl", "idrs"):
                kw["num_inner_iterations"] = param
            if method == "richardson":
                kw["relaxation_factor"] = float(OMEGA)
            if method == "idrs":
                oracle.rng_reset(variant)
            if pre is not None:
                kw.update(pre=pre, side=side)
            r = oracle.solve(method, op, bf, **common, **kw)
        assert r.history.size == K + 1, (method, r.history)
        out[variant] = r.history
    return out


class Pins:
    """history[0..K] of one case with the tolerance of every entry (None: bitwise).

    - history[0] where r0 is b itself: sqrt of an exact integer sum, bitwise.
    - history[1] without a preconditioner: CGS, TFQMR(1), IDR(s) by the floor rule (c from ``C1``), at most 1e-12;
      Richardson bitwise (``richardson_integers``); BiCGStab(l) by the closed forms of ``FirstStep`` (CG's |r1| for
      l >= 2, BiCGStab's for l = 1).
    - everything else: tol_k = max(floor_k, 16 e_k), e_k the larger relative distance of the oracle's two variants
      from the exact value.  The device folds its dots in a tree of depth D ~ 65 where the oracle adds in a chain of
      n terms, so its reduction error is not the larger; what differs is the rounding pattern of the vector statements
      and where an fma contracts, and 16 times one sample of that error covers another pattern.  Every tol_k is at
      most TOL_CAP (asserted: a condition on the case, not a measurement)."""

    def __init__(self, oracle, g, shape, b, method, param=None, side=None, fs=None, K=None, basis=None):
        b = np.asarray(b, np.int64)
        pre = side is not None
        self.n, self.method, self.param, self.side = b.size, method, param, side
        self.K = K = iterations(method, param, pre) if K is None else K
        dinv = 1.0 / int_diagonal(shape) if pre else None
        basis = basis or Basis(shape, b, dinv)
        assert basis.pre == pre
        shadow = shadow_vectors(oracle, b.size, param) if method == "idrs" else ()
        sp = Space(basis, decimal=method in DECIMAL_METHODS)
        run = exact_run(sp, method, param, K, side, shadow)
        self.run = run
        self.exact = exact = run.history
        hist = oracle_histories(oracle, g, b, method, param, K, side, dinv)
        self.oracle = hist
        self.e = [max(abs(h[k] - exact[k]) / exact[k] for h in hist.values()) for k in range(K + 1)]
        fs = fs or FirstStep(Sums(shape, b))
        self.tol, self.rule = [], []
        for k in range(K + 1):
            ratio = max(math.sqrt(float(_dec(sp.magnitude(v)) / _dec(sp.dot(v, v)))) for v in run.feeds[k])
            floor = floor_tol(self.n, ratio, _c(method, param, k, pre))
            if k == 0 and run.feeds[0][0].c == {0: 1}:
                assert exact[0] == fs.h0
                self.tol.append(None), self.rule.append("exact")
            elif k == 1 and not pre and method == "richardson":
                h1 = richardson_h1(shape, b)
                assert close(h1, exact[1], 1e-15)
                exact[1] = h1
                self.tol.append(None), self.rule.append("exact")
            elif k == 1 and not pre and method == "bicgstabl":
                h1, tol = (fs.cg_h1, fs.cg_tol) if param >= 2 else (fs.bicgstab_h1, fs.bicgstab_tol)
                assert close(exact[1], h1, 1e-15)
                self.tol.append(tol), self.rule.append("closed form")
            elif k == 1 and not pre and method in ("cgs", "tfqmr", "tfqmr1", "idrs"):
                assert floor <= 1e-12, f"{method}: floor {floor:.3e} above 1e-12"
                self.tol.append(floor), self.rule.append(f"floor c={_c(method, param, k, pre)}")
            else:
                tol = max(floor, 16 * self.e[k])
                assert tol <= TOL_CAP, f"{method}({param}) {side}: tol_{k} = {tol:.3e} above the cap {TOL_CAP}"
                self.tol.append(tol), self.rule.append("16 e_k" if tol > floor else "floor")

    def check(self, history, label=""):
        """Assert a history against the pins; returns the ratios |h - exact| / (exact e_k)."""
        assert len(history) == self.K + 1, (label, history)
        ratios = []
        for k, (h, x, tol) in enumerate(zip(history, self.exact, self.tol)):
            if tol is None:
                assert h == x, f"{label} history[{k}] = {h!r}, exact {x!r} (bitwise)"
            else:
                assert close(h, x, tol), f"{label} history[{k}] = {h!r}, exact {x!r}: rel {abs(h - x) / x:.3e} > tol " \
                                         f"{tol:.3e} ({self.rule[k]})"
            ratios.append(abs(h - x) / (x * self.e[k]) if self.e[k] > 0 else (0.0 if h == x else math.inf))
        return ratios


def convdiff_box(mesh, nx, ny, nz, vel=(2.0, 1.0, -1.0)):
    """The non-symmetric integer operator of the GMRES pins: A = -L + C(v) on the unit box, nu = 1, v = (2, 1, -1),
    first-order upwind.  Every face weight is an integer; row sums of |A| <= 20, |A - A^T| = 2.  Returns the face
    graph, the weights for ``StencilMatrix.from_face_weights`` (apply with alpha = 1, beta = 0) and the
    ``IntOperator``; the oracle's operator of it is ``oracle.StencilOperator(g, -1.0, 0.0, conv=1.0, vel=vel)``."""
    g = unit_box(mesh, nx, ny, nz)
    w = mesh.convection_diffusion_weights(g, 1.0, vel)
    op = IntOperator.from_face_weights(g, *w)
    assert op.rowsum <= 20
    return g, w, op


def periodic_box(mesh, nx, ny, nz, vel=None):
    """The integer operators WITH A HALO: the box at unit spacing, walls in x and y, periodic in z, as one rank's local
    graph whose halo planes are the images of its own planes nz - 1 and 0 (``mesh.periodic_z_local_graph``).  ``vel``
    None: -L, diagonal 6 ... 8, off-diagonals -1, symmetric; else first-order upwind convection-diffusion with nu = 1,
    row sums of |A| <= 20, |A - A^T| = 2.  Returns the local graph, the rows the rank sends (itself), the face weights
    for ``StencilMatrix.from_face_weights`` (apply with alpha = 1, beta = 0; -L is also ``from_face_graph`` with
    alpha = -1) and the ``IntOperator`` of the owned cells, the halo folded (``from_local_graph``)."""
    loc, send_idx = mesh.periodic_z_local_graph(nx, ny, nz, lengths=(float(nx), float(ny), float(nz)))
    w = mesh.convection_diffusion_weights(loc, 1.0, (0.0, 0.0, 0.0) if vel is None else vel)
    op = IntOperator.from_local_graph(loc, *w)
    assert op.rowsum <= (12 if vel is None else 20)
    return loc, send_idx, w, op


def periodic_oracle_op(oracle, loc, send_idx, vel=None, variant="strict"):
    """The oracle's operator of ``periodic_box``: its face loops over the local graph, the halo filled with the rows
    the rank would receive."""
    kw = {} if vel is None else dict(conv=1.0, vel=vel)
    op = oracle.StencilOperator(loc, -1.0, 0.0, variant=variant, **kw)
    n = loc.n_cells
    return oracle.CallbackOperator(n, lambda x: op.apply(np.concatenate([x, x[send_idx]]))[:n])


PERIODIC_KINDS = ("periodic", "periodic_convdiff")
GMRES_VEL = (2.0, 1.0, -1.0)
GMRES_SEED, GMRES_RANGE = 31, (-3, 3)  # b = int_vector(n, 31, -3, 3): W_t stays in int64 through t = 13
# shape -> the (K, m) pinned on it (tests/test_gpu_exact_gmres.py names the kernel width each shape is there for).
# K = 9 = m: 1 ... 9 basis vectors per step, every remainder of groups of 2, 3 and 4; K = 12, m = 5: inner_finalize
# twice and the exit in the middle of a cycle
GMRES_CASES = {(7, 5, 3): [(12, 5)], (37, 21, 19): [(12, 5), (9, 9)], (64, 64, 65): [(9, 9)], (64, 64, 129): [(9, 9)],
               (128, 128, 65): [(9, 9)], (128, 128, 129): [(9, 9)]}
GMRES_X_ROWS = 20000  # at or below: x itself is compared with the exact x (``Space.materialize`` is elementwise Python)


class GmresProblem:
    """One shape of the GMRES pins: the convection-diffusion box, b, the chain, and the pins of its (K, m), built on
    demand and kept."""

    def __init__(self, oracle, mesh, shape, kind="convdiff"):
        self.oracle, self.shape, self.kind = oracle, shape, kind
        if kind in PERIODIC_KINDS:  # the same operators on the z-periodic box: ``g`` is the local graph with its halo
            self.vel = GMRES_VEL if kind == "periodic_convdiff" else None
            self.g, self.send_idx, self.weights, self.A = periodic_box(mesh, *shape, vel=self.vel)
        else:
            assert kind == "convdiff"
            self.g, self.weights, self.A = convdiff_box(mesh, *shape, vel=GMRES_VEL)
        self.b = int_vector(self.g.n_cells, GMRES_SEED, *GMRES_RANGE)
        self.basis = OpBasis(self.A, self.b)
        self._pins = {}

    def oracle_op(self, variant):
        if self.kind in PERIODIC_KINDS:
            return periodic_oracle_op(self.oracle, self.g, self.send_idx, self.vel, variant)
        return self.oracle.StencilOperator(self.g, -1.0, 0.0, conv=1.0, vel=GMRES_VEL, variant=variant)

    def pins(self, K, m):
        if (K, m) not in self._pins:
            self._pins[K, m] = GmresPins(self.oracle, self.oracle_op, self.basis, self.A, self.b, K, m,
                                         with_x=self.b.size <= GMRES_X_ROWS)
        return self._pins[K, m]


class GmresPins:
    """history[0..K] and x_K of unpreconditioned GMRES(m) from x0 = 0 on an integer operator, with ``Pins``' rule
    unchanged: history[0] bitwise (the root of an exact integer below 2^53); for k >= 1 tol_k = max(floor_k, 16 e_k),
    e_k the larger relative distance of the oracle's strict and fma builds from the exact value, floor_k =
    ``floor_tol`` with c = k C1["gmres"] and the ratio ``gmres`` records; every tol_k at most TOL_CAP (asserted).

    The coefficient form over the power basis loses digits with K (at PREC = 80 it is wrong in the second digit by
    K = 64 on the convection-diffusion box): the restatement is run at PREC and at 2 PREC digits and the two histories
    must agree to 1e-40 (asserted), and K is held at 12 or below.

    x: ``tol_res`` for ``true_residual(A, b, x)`` against the exact history[K] -- max(floor_K, 16 e_x), e_x the same
    quantity of the oracle's two x; with ``with_x`` also ``x`` (the exact x_K, each element rounded once) and
    ``tol_x`` for the relative 2-norm distance from it, by the same rule on the oracle's two x."""

    MAX_K = 12

    def __init__(self, oracle, make_op, basis, A, b, K, m, with_x=False):
        b = np.asarray(b, np.int64)
        assert 1 <= K <= self.MAX_K, "the power basis does not carry more steps at PREC digits"
        self.n, self.K, self.m, self.A, self.b = b.size, K, m, A, b
        self.run = run = gmres(Space(basis, decimal=True), K, m)
        fine = gmres(Space(basis, decimal=True), K, m, prec=2 * PREC)
        with localcontext() as ctx:
            ctx.prec = 2 * PREC
            for k, (c, f) in enumerate(zip(run.hist_sq, fine.hist_sq)):
                assert abs(c - f) <= abs(f) * Decimal(10) ** -40, f"history[{k}]^2 depends on the precision: {c} {f}"
        self.exact = exact = run.history
        rr = exact_dot(b, b)
        assert exact[0] == math.sqrt(float(rr))
        self.oracle, self.oracle_x = {}, {}
        bf = b.astype(np.float64)
        for variant in ("strict", "fma"):
            r = oracle.solve("gmres", make_op(variant), bf, num_iterations=K, abs_tol=0.0, rel_tol=0.0,
                             num_inner_iterations=m, variant=variant)
            assert r.history.size == K + 1, r.history
            self.oracle[variant], self.oracle_x[variant] = r.history, r.x
        self.e = [max(abs(h[k] - exact[k]) / exact[k] for h in self.oracle.values()) for k in range(K + 1)]
        self.tol, self.rule = [None], ["exact"]
        for k in range(1, K + 1):
            floor = floor_tol(self.n, run.ratio[k], _c("gmres", m, k, False))
            self.tol.append(self._cap(max(floor, 16 * self.e[k]), f"tol_{k}"))
            self.rule.append("16 e_k" if self.tol[k] > floor else "floor")
        floor = floor_tol(self.n, run.ratio[K], _c("gmres", m, K, False))
        self.e_res = max(abs(true_residual(A, b, x) - exact[K]) / exact[K] for x in self.oracle_x.values())
        self.tol_res = self._cap(max(floor, 16 * self.e_res), "tol_res")
        self.rule_res = "16 e_x" if self.tol_res > floor else "floor"
        self.x = None
        if with_x:
            self.x = Space(basis).materialize(run.x)
            nx = float(np.linalg.norm(self.x))
            self.e_x = max(float(np.linalg.norm(x - self.x)) / nx for x in self.oracle_x.values())
            self.tol_x = self._cap(max(floor, 16 * self.e_x), "tol_x")

    def _cap(self, tol, what):
        assert tol <= TOL_CAP, f"gmres({self.m}) K={self.K} n={self.n}: {what} = {tol:.3e} above the cap {TOL_CAP}"
        return tol

    check = Pins.check

    def check_x(self, x, label=""):
        """Assert a solution against the pins; returns |res - exact| / (exact e_x) (and the same for x itself)."""
        res, want = true_residual(self.A, self.b, x), self.exact[self.K]
        assert close(res, want, self.tol_res), f"{label} |b - A x| = {res!r}, exact history[{self.K}] {want!r}: rel " \
                                               f"{abs(res - want) / want:.3e} > tol {self.tol_res:.3e} ({self.rule_res})"
        out = [abs(res - want) / (want * self.e_res) if self.e_res > 0 else 0.0]
        if self.x is not None:
            d = float(np.linalg.norm(x - self.x)) / float(np.linalg.norm(self.x))
            assert d <= self.tol_x, f"{label} |x - exact| / |exact| = {d:.3e} > tol {self.tol_x:.3e}"
            out.append(d / self.e_x if self.e_x > 0 else 0.0)
        return out


# ---- CG and BiCGStab past their first step ---------------------------------------------------------------------------

STEP_K = {"cg": 8, "bicgstab": 5, "cg2": 4}  # the iterations pinned; BiCGStab at 5 reaches each parity buffer at least twice
TWO_STAGE = (-1.0, 2.0, -1.0, 1.0)  # (alpha1, beta1, alpha2, beta2) over M = L: y = x - L (2 x - L x) = (I + A)^2 x, A = -L


class TwoStageSpace(Space):
    """``Space`` whose operator is (I + A)^2 = I + 2 A + A^2 -- the two-stage operator with the integer constants
    ``TWO_STAGE``: a polynomial in A, so its Krylov vectors are columns over the same chain."""

    def A(self, v):
        a = Space.A(self, v)
        return v + 2 * a + Space.A(self, a)


def two_stage_operator(A):
    """(I + A)^2 of an ``IntOperator`` as an ``IntOperator``."""
    import scipy.sparse as sps

    m = sps.identity(A.n, dtype=np.int64, format="csr") + A.csr
    c = (m @ m).tocoo()
    return IntOperator(A.n, c.row, c.col, c.data)


def two_stage_oracle_op(oracle, g, variant="strict"):
    """The oracle's two-stage operator: a callback that applies its one-stage operator M = L twice."""
    m = oracle.StencilOperator(g, 1.0, 0.0, variant=variant)
    a1, b1, a2, b2 = TWO_STAGE
    return oracle.CallbackOperator(g.n_cells, lambda x: b2 * x + a2 * m.apply(b1 * x + a1 * m.apply(x)))


def poisson_operator(mesh, g):
    """``-L`` of the unit box as an ``IntOperator`` (convection-diffusion with nu = 1, v = 0)."""
    return IntOperator.from_face_weights(g, *mesh.convection_diffusion_weights(g, 1.0, (0.0, 0.0, 0.0)))


class StepPins:
    """history[0..K] and x_0 ... x_K of unpreconditioned CG ("cg"; "cg2": CG on the two-stage operator) or BiCGStab from
    x0 = 0, with ``Pins``' rule unchanged: history[0] bitwise; tol_k = max(floor_k, 16 e_k), e_k the larger relative
    distance of the oracle's strict and fma builds from the exact value, floor_k = ``floor_tol`` with c = k C1[method]
    and the ratio sqrt(M) / h of the step's own terms (``cg``, ``bicgstab``); every tol_k at most TOL_CAP (asserted).
    With ``fs`` (the Poisson box's ``FirstStep``) history[1] keeps the closed form's tolerance where that is tighter.

    ``check_x(x, k)``: ||b - A x|| (``true_residual``) against the exact history[k] within max(floor_k, 16 e_x), e_x
    the same quantity of the oracle's two x after k iterations; at or below GMRES_X_ROWS rows also x against the exact
    x_k (``Space.materialize``) by relative 2-norm under the same rule.  The oracle's x_k and the exact x_k are formed
    when first asked for and kept."""

    def __init__(self, oracle, make_op, space, A, b, method, K=None, fs=None):
        b = np.asarray(b, np.int64)
        self.method, self.K = method, STEP_K[method] if K is None else K
        self.n, self.A, self.b, self.space = b.size, A, b, space
        self._oracle, self._make_op = oracle, make_op
        self.kind = "bicgstab" if method == "bicgstab" else "cg"
        K = self.K
        self.run = run = (bicgstab if self.kind == "bicgstab" else cg)(space, K)
        self.exact = exact = run.history
        assert exact[0] == math.sqrt(float(exact_dot(b, b)))
        self.oracle, self._ox, self._x, self._res, self._xt = {}, {}, {}, {}, {}
        for variant in ("strict", "fma"):
            r = self._solve(variant, K)
            self.oracle[variant], self._ox[K, variant] = r.history, r.x
        self.e = [max(abs(h[k] - exact[k]) / exact[k] for h in self.oracle.values()) for k in range(K + 1)]
        self.floor = [0.0] + [floor_tol(self.n, math.sqrt(float(run.ratio_sq[k])), k * C1[self.kind])
                              for k in range(1, K + 1)]
        self.tol, self.rule = [None], ["exact"]
        for k in range(1, K + 1):
            tol = self._cap(max(self.floor[k], 16 * self.e[k]), f"tol_{k}")
            rule = "16 e_k" if tol > self.floor[k] else "floor"
            if k == 1 and fs is not None:
                h1, t1 = (fs.cg_h1, fs.cg_tol) if self.kind == "cg" else (fs.bicgstab_h1, fs.bicgstab_tol)
                assert close(exact[1], h1, 1e-15)
                if t1 < tol:
                    tol, rule = t1, "closed form"
            self.tol.append(tol), self.rule.append(rule)

    def _solve(self, variant, k):
        r = self._oracle.solve(self.kind, self._make_op(variant), self.b.astype(np.float64), num_iterations=k,
                               abs_tol=0.0, rel_tol=0.0, variant=variant)
        assert r.history.size == k + 1, (self.method, r.history)
        return r

    def _cap(self, tol, what):
        assert tol <= TOL_CAP, f"{self.method} K={self.K} n={self.n}: {what} = {tol:.3e} above the cap {TOL_CAP}"
        return tol

    def check(self, history, label="", k=None):
        """Assert history[0..k] (K by default; a solve that stopped at iteration k leaves k + 1 entries) against the
        pins; returns |h - exact| / exact per entry."""
        k = self.K if k is None else k
        assert len(history) == k + 1, (label, history)
        far = []
        for j, (h, x, tol) in enumerate(zip(history, self.exact, self.tol)):
            if tol is None:
                assert h == x, f"{label} history[{j}] = {h!r}, exact {x!r} (bitwise)"
            else:
                assert close(h, x, tol), f"{label} history[{j}] = {h!r}, exact {x!r}: rel {abs(h - x) / x:.3e} > tol " \
                                         f"{tol:.3e} ({self.rule[j]})"
            far.append(abs(h - x) / x)
        return far

    def stop_between(self, k):
        """An absolute tolerance that iteration k is the first to meet: the midpoint of the exact history[k] and
        history[k - 1] (they differ by orders of magnitude more than any tol)."""
        mid = 0.5 * (self.exact[k] + self.exact[k - 1])
        assert self.exact[k] * 1.05 < mid < min(self.exact[:k]) / 1.05
        return mid

    def res_exact(self, k):
        """The exact ||b - A x_k||: for CG and BiCGStab without a preconditioner it is history[k]."""
        return self.exact[k]

    def oracle_x(self, variant, k):
        if (k, variant) not in self._ox:
            self._ox[k, variant] = self._solve(variant, k).x
        return self._ox[k, variant]

    def x(self, k):
        """The exact x_k, each element rounded once (None above GMRES_X_ROWS rows)."""
        if self.n > GMRES_X_ROWS:
            return None
        if k not in self._x:
            self._x[k] = self.space.materialize(self.run.xs[k])
        return self._x[k]

    def x_tolerances(self, k):
        """(e_res, tol_res, rule, e_x, tol_x) of x_k; the last two None where the exact x is not formed."""
        if k not in self._xt:
            assert 1 <= k <= self.K
            want = self.res_exact(k)
            xs = [self.oracle_x(v, k) for v in ("strict", "fma")]
            e_res = max(abs(true_residual(self.A, self.b, x) - want) / want for x in xs)
            tol_res = self._cap(max(self.floor[k], 16 * e_res), f"tol_res({k})")
            e_x = tol_x = None
            if self.x(k) is not None:
                nx = float(np.linalg.norm(self.x(k)))
                e_x = max(float(np.linalg.norm(x - self.x(k))) / nx for x in xs)
                tol_x = self._cap(max(self.floor[k], 16 * e_x), f"tol_x({k})")
            self._xt[k] = (e_res, tol_res, "16 e_x" if tol_res > self.floor[k] else "floor", e_x, tol_x)
        return self._xt[k]

    def check_x(self, x, k=None, label=""):
        """Assert a solution after k iterations (K by default); returns |res - exact| / exact (and |x - exact| / |exact|)."""
        k = self.K if k is None else k
        e_res, tol_res, rule, e_x, tol_x = self.x_tolerances(k)
        res, want = true_residual(self.A, self.b, x), self.res_exact(k)
        assert close(res, want, tol_res), f"{label} |b - A x_{k}| = {res!r}, exact {want!r}: rel " \
                                          f"{abs(res - want) / want:.3e} > tol {tol_res:.3e} ({rule})"
        out = [abs(res - want) / want]
        if tol_x is not None:
            d = float(np.linalg.norm(x - self.x(k))) / float(np.linalg.norm(self.x(k)))
            assert d <= tol_x, f"{label} |x_{k} - exact| / |exact| = {d:.3e} > tol {tol_x:.3e}"
            out.append(d)
        return out


STEP_SEED = 31  # b = int_vector(n, 31) on the Poisson boxes: the data of the first-step pins
# method -> the (shape, box) the GPU tests pin it on, and the iterations k whose x_k they check (K and the early exit);
# tests/test_exact_reference.py asserts every cap of every one on the reference alone
STEP_CASES = {
    "cg": [((64, 48, 40), "poisson"), ((37, 21, 19), "poisson"), ((36, 30, 8), "poisson"), ((64, 64, 12), "poisson"),
           ((256, 128, 130), "poisson"), ((200, 100, 211), "poisson")],
    "bicgstab": [((64, 48, 40), "poisson"), ((37, 21, 19), "poisson"), ((40, 30, 17), "convdiff")],
    "cg2": [((24, 24, 24), "poisson"), ((9, 7, 1), "poisson")],
}
STEP_STOP = 3  # the early-exit tests stop at this iteration
STEP_RANK_SHAPES, STEP_RANK_K = [(64, 16, 24), (32, 16, 18)], 4  # tests/test_gpu_exact_ranks.py: the whole boxes (2 and 3 slabs)
STEP_BLOCK_SEEDS = (31, 32, 33, 34)  # tests/test_gpu_block.py: the columns of the block CG on 64 x 48 x 40, K = 8
# tests/test_gpu_exact_rccl.py, the z-periodic boxes over a size-1 communicator: G gets general records; on L and L2 the
# interior planes get lattice records and CG its fused step.  Only G is below GMRES_X_ROWS (x against the exact x_k)
PERIODIC_G, PERIODIC_L, PERIODIC_L2 = (20, 12, 9), (32, 32, 24), (64, 16, 40)
PERIODIC_STEP_CASES = {
    "cg": [(PERIODIC_G, "periodic"), (PERIODIC_L, "periodic"), (PERIODIC_L2, "periodic")],
    "bicgstab": [(PERIODIC_G, "periodic"), (PERIODIC_L, "periodic"), (PERIODIC_G, "periodic_convdiff"),
                 (PERIODIC_L, "periodic_convdiff")],
}
PERIODIC_GMRES_CASES = {PERIODIC_G: [(12, 5), (9, 9)], PERIODIC_L: [(12, 5), (9, 9)]}  # on "periodic_convdiff"


class StepProblem:
    """One box of the step pins -- "poisson": -L on the unit box, b = int_vector(n, 31); "convdiff": the GMRES pins'
    non-symmetric box and b -- with its chain, its ``IntOperator`` (built once) and the pins per method, kept."""

    def __init__(self, oracle, mesh, shape, kind="poisson", seed=STEP_SEED):
        self.oracle, self.shape, self.kind = oracle, tuple(shape), kind
        if kind in PERIODIC_KINDS:
            self.vel = GMRES_VEL if kind == "periodic_convdiff" else None
            self.g, self.send_idx, self.weights, self.A = periodic_box(mesh, *shape, vel=self.vel)
            self.b = int_vector(self.g.n_cells, GMRES_SEED, *GMRES_RANGE)
            self.basis, self.fs = OpBasis(self.A, self.b), None
        elif kind == "convdiff":
            self.g, self.weights, self.A = convdiff_box(mesh, *shape, vel=GMRES_VEL)
            self.b = int_vector(self.g.n_cells, GMRES_SEED, *GMRES_RANGE)
            self.basis, self.fs = OpBasis(self.A, self.b), None
        else:
            self.g = unit_box(mesh, *shape)
            self.A = poisson_operator(mesh, self.g)
            self.b = int_vector(self.g.n_cells, seed)
            self.basis, self.fs = Basis(shape, self.b), FirstStep(Sums(shape, self.b))
        self._pins, self._A2, self._pre_basis = {}, None, None

    def oracle_op(self, variant):
        if self.kind in PERIODIC_KINDS:
            return periodic_oracle_op(self.oracle, self.g, self.send_idx, self.vel, variant)
        if self.kind == "convdiff":
            return self.oracle.StencilOperator(self.g, -1.0, 0.0, conv=1.0, vel=GMRES_VEL, variant=variant)
        return self.oracle.StencilOperator(self.g, -1.0, 0.0, variant=variant)

    def pins(self, method, K=None):
        key = (method, STEP_K[method] if K is None else K)
        if key not in self._pins:
            if method == "cg2":
                assert self.kind == "poisson"
                self._A2 = self._A2 or two_stage_operator(self.A)
                self._pins[key] = StepPins(self.oracle, lambda v: two_stage_oracle_op(self.oracle, self.g, v),
                                           TwoStageSpace(self.basis), self._A2, self.b, method, key[1])
            else:
                self._pins[key] = StepPins(self.oracle, self.oracle_op, Space(self.basis), self.A, self.b, method,
                                           key[1], fs=self.fs)
        return self._pins[key]

    def engine_pins(self, method, param=None, side=None, K=None):
        """``EnginePins`` of an engine method on this box (``side``: the Jacobi preconditioner on it; Poisson boxes)."""
        key = ("engine", method, param, side, K)
        if key not in self._pins:
            dinv = None
            basis = self.basis
            if side is not None:
                assert self.kind == "poisson"
                dinv = 1.0 / int_diagonal(self.shape)
                if self._pre_basis is None:
                    self._pre_basis = Basis(self.shape, self.b, dinv)
                basis = self._pre_basis
            self._pins[key] = EnginePins(self.oracle, self.oracle_op, basis, self.A, self.b, method, param, K, side, dinv)
        return self._pins[key]


# ---- the engine's other methods past their second step ----------------------------------------------------------------

ENGINE_STEP_BOXES = [((64, 48, 40), "poisson"), ((37, 21, 19), "poisson")]
ENGINE_STEP_K = [("cgs", None, 4), ("tfqmr", None, 4), ("tfqmr1", None, 4), ("bicgstabl", 1, 3), ("bicgstabl", 2, 5),
                 ("bicgstabl", 3, 7), ("idrs", 1, 4), ("idrs", 2, 6), ("idrs", 4, 6)]
# (BiCGStab(l): 2 l + 1, a second cycle's beta.  IDR(4): 6, not 7 -- on 37 x 21 x 19 the oracle's own x_7 lies 9.6e-12 from
# the exact one, and 16 times that is above TOL_CAP: NOTES.md)
# The early exit on 64 x 48 x 40: (K, the iteration an absolute tolerance stops at).  Iteration 3 of K wherever
# history[3] lies below every earlier entry.  IDR(2) and IDR(4) are not monotone there -- history[3] is above history[1]
# -- so no tolerance makes iteration 3 the first to meet it: IDR(2) stops at 6 of 7 (the end of its third cycle), IDR(4)
# at 5 of 6 (inside its second), the first iterations after 1 that lie below all before them
ENGINE_STOPS = {(m, p): (K, STEP_STOP) for m, p, K in ENGINE_STEP_K}
ENGINE_STOPS.update({("idrs", 2): (7, 6), ("idrs", 4): (6, 5)})
ENGINE_GMRES_STOPS = (5, 7)  # GMRES(5) of 12 iterations on the convection-diffusion boxes: a cycle's last step, inside one
ENGINE_FGMRES_M, ENGINE_FGMRES_STOPS = 2, [(2, 3), (3, 4)]  # FGMRES(2) with Jacobi on the Poisson boxes: (stop at, of K)
ENGINE_STEP_CONVDIFF = [("cgs", None, 4, (40, 30, 17)), ("tfqmr", None, 4, (40, 30, 17)), ("bicgstabl", 2, 5, (40, 30, 17)),
                        ("tfqmr1", None, 6, (7, 5, 3))]  # on 7 x 5 x 3 TFQMR1's omega < tau comes out both ways
ENGINE_JACOBI = [("cg", None), ("cgs", None), ("tfqmr", None), ("idrs", 2), ("bicgstabl", 2), ("fgmres", 1), ("fgmres", 30),
                 ("richardson", None)]
ENGINE_JACOBI_K = 3
# the side the reference applies the preconditioner on whatever pre_side says (tests/test_gpu_exact_first_step.py)
ENGINE_FIXED_SIDE = {"richardson": "left", "bicgstabl": "left", "fgmres": "right"}
# (method, param, side, shape, box, K): every case tests/test_gpu_exact_engine_steps.py pins; tests/test_exact_reference.py
# asserts every cap of every one on the reference alone
ENGINE_STEP_CASES = [(m, p, None, shape, kind, K) for shape, kind in ENGINE_STEP_BOXES for m, p, K in ENGINE_STEP_K] + \
    [(m, p, None, shape, "convdiff", K) for m, p, K, shape in ENGINE_STEP_CONVDIFF] + \
    [(m, p, side, shape, kind, ENGINE_JACOBI_K) for shape, kind in ENGINE_STEP_BOXES for m, p in ENGINE_JACOBI
     for side in ("left", "right") if ENGINE_FIXED_SIDE.get(m, side) == side]


def oracle_solutions(oracle, make_op, b, method, param, k, side=None, dinv=None):
    """``oracle_histories`` with the operator given (``make_op(variant)``) and the whole result kept: history[0..k] and
    the x the oracle leaves after k iterations, in both of its arithmetic variants."""
    out = {}
    bf = np.asarray(b, np.float64)
    for variant in ("strict", "fma"):
        op = make_op(variant)
        pre = None if dinv is None else oracle.DiagOperator(dinv, variant=variant)
        common = dict(num_iterations=k, abs_tol=0.0, rel_tol=0.0, variant=variant)
        if method == "fgmres":
            r, _ = oracle.solve_gmres_pre(op, pre, bf, side=side or "right", flexible=True, num_inner_iterations=param, **common)
        else:
            kw = {}
            if method in ("bicgstabl", "idrs"):
                kw["num_inner_iterations"] = param
            if method == "richardson":
                kw["relaxation_factor"] = float(OMEGA)
            if method == "idrs":
                oracle.rng_reset(variant)
            if pre is not None:
                kw.update(pre=pre, side=side)
            r = oracle.solve(method, op, bf, **common, **kw)
        assert r.history.size == k + 1, (method, r.history)
        out[variant] = r
    return out


def engine_float64(A, b, method, param, K, side=None, dinv=None, shadow=(), defect=None, at=None):
    """An engine method's history[0..K] and x_0 ... x_K in plain fp64 numpy (``A``: an ``IntOperator``): the statements of
    the restatement on ``Float64Space``, with the defects the pins must reject."""
    sp = Float64Space(A.float64(), b, dinv=dinv)
    run = exact_run(sp, method, param, K, side, shadow, defect=defect, at=at)
    return np.sqrt(np.array(run.hist_sq, np.float64)), run.xs


class EnginePins(StepPins):
    """history[0..K] and x_0 ... x_K of an engine method (CGS, TFQMR, TFQMR1, BiCGStab(l), IDR(s), FGMRES, Richardson, CG
    with a preconditioner) from x0 = 0, with ``StepPins``' rule and its ``check``, ``check_x`` and ``stop_between``:

    - history[0] bitwise where r0 is b; otherwise tol_k = max(floor_k, 16 e_k) <= TOL_CAP (asserted), e_k the larger
      relative distance of the oracle's strict and fma builds from the exact value, floor_k = ``floor_tol`` with the
      ratio sqrt(M) / h of the statements that form the entry (``ratio_sq`` of the restatements -- not the power-basis
      terms, which cancel) and c = k C1[method], plus 4 k + 1 under a preconditioner.
    - x: ``true_residual(A, b, x)`` against the exact ||b - A x_k||, formed from ``xs[k]`` in the space -- NOT history[k]:
      TFQMR's history is the bound tau sqrt(2 k + 1), a left-preconditioned method's the norm of P r -- within
      max(floor_k, 16 e_res), e_res the same quantity of the oracle's two x; at or below GMRES_X_ROWS rows also x against
      the exact x_k by relative 2-norm under the same rule.
    - the decimal methods run at PREC and at 2 PREC digits and must agree to 1e-40 (asserted), history and residuals.

    ``preds``: for TFQMR1 the outcome of omega < tau at every half-step."""

    def __init__(self, oracle, make_op, basis, A, b, method, param=None, K=None, side=None, dinv=None):
        b = np.asarray(b, np.int64)
        pre = side is not None
        assert basis.pre == pre and (dinv is not None) == pre
        self.method, self.param, self.side, self.dinv = method, param, side, dinv
        self.K = K = iterations(method, param, pre) if K is None else K
        self.n, self.A, self.b = b.size, A, b
        self._oracle, self._make_op = oracle, make_op
        self.decimal = method in DECIMAL_METHODS
        self.shadow = shadow_vectors(oracle, b.size, param) if method == "idrs" else ()
        self.space = Space(basis, decimal=self.decimal)
        self.run = run = exact_run(self.space, method, param, K, side, self.shadow)
        self._fine = exact_run(Space(basis, decimal=True), method, param, K, side, self.shadow, prec=2 * PREC) if self.decimal else None
        if self.decimal:
            self._agree(run.hist_sq, self._fine.hist_sq, "history")
        self.preds = getattr(run, "preds", None)
        self.exact = exact = run.history
        self.oracle, self._ox, self._x, self._res, self._xt = {}, {}, {}, {}, {}
        for variant, r in self._solve(K).items():
            self.oracle[variant], self._ox[K, variant] = r.history, r.x
        self.e = [max(abs(h[k] - exact[k]) / exact[k] for h in self.oracle.values()) for k in range(K + 1)]
        self.floor = [floor_tol(self.n, math.sqrt(float(run.ratio_sq[k])), _c(method, param, k, pre)) for k in range(K + 1)]
        self.tol, self.rule = [], []
        for k in range(K + 1):
            if k == 0 and run.feeds[0][0].c == self.space.b().c:
                assert exact[0] == math.sqrt(float(exact_dot(b, b)))
                self.tol.append(None), self.rule.append("exact")
            else:
                self.tol.append(self._cap(max(self.floor[k], 16 * self.e[k]), f"tol_{k}"))
                self.rule.append("16 e_k" if self.tol[k] > self.floor[k] else "floor")

    @staticmethod
    def _agree(coarse, fine, what):
        with localcontext() as ctx:
            ctx.prec = 2 * PREC
            for k, (c, f) in enumerate(zip(coarse, fine)):
                assert abs(c - f) <= abs(f) * Decimal(10) ** -40, f"{what}[{k}]^2 depends on the precision: {c} {f}"

    def _cap(self, tol, what):
        assert tol <= TOL_CAP, f"{self.method}({self.param}) {self.side} K={self.K} n={self.n}: {what} = {tol:.3e} above the cap {TOL_CAP}"
        return tol

    def stop_between(self, k):
        """``StepPins.stop_between`` for a history that need not fall: the midpoint of the exact history[k] and the
        smallest earlier entry (history[k - 1] where the history is monotone)."""
        mid = 0.5 * (self.exact[k] + min(self.exact[:k]))
        assert self.exact[k] * 1.05 < mid < min(self.exact[:k]) / 1.05
        return mid

    def _solve(self, k):
        return oracle_solutions(self._oracle, self._make_op, self.b, self.method, self.param, k, self.side, self.dinv)

    def oracle_x(self, variant, k):
        if (k, variant) not in self._ox:
            for v, r in self._solve(k).items():
                self._ox[k, v] = r.x
        return self._ox[k, variant]

    def _res_sq(self, run, k, prec):
        sp = self.space
        with localcontext() as ctx:
            ctx.prec = prec
            r = sp.b() - sp.A(run.xs[k])
            n = sp.ndots
            sq = sp.dot(r, r)
            sp.ndots = n
        return sq

    def res_exact(self, k):
        """The exact ||b - A x_k||, from ``xs[k]`` in the space."""
        if k not in self._res:
            sq = self._res_sq(self.run, k, PREC)
            if self.decimal:
                self._agree([sq], [self._res_sq(self._fine, k, 2 * PREC)], f"|b - A x_{k}|")
            with localcontext() as ctx:
                ctx.prec = PREC
                self._res[k] = float(_dec(sq).sqrt())
        return self._res[k]


def richardson_integers(shape, b, k):
    """Richardson with omega = 2^-5 in integers: X = 32^k x_k and R = 32^k r_k.  With |X| and every partial sum of A X
    below 2^53 (asserted, from row sums of |A| <= 12), every statement x += omega r, r = b - A x is exact in any order
    and with any fma: x_k = X / 32^k to the bit."""
    b = np.asarray(b, np.int64)
    X, R = np.zeros_like(b), b.copy()
    for j in range(k):
        X = 32 * X + R  # 32^(j+1) x_{j+1} = 32 (32^j x_j) + 32^j r_j
        assert int(np.abs(X).max()) * 12 < EXACT
        R = (32 ** (j + 1)) * b - int_apply(shape, X)  # 32^(j+1) (b - A x_{j+1})
        assert int(np.abs(R).max()) < EXACT
    return X, R


def richardson_h1(shape, b):
    """history[1] of Richardson with omega = 2^-5: sum (32 r_1)^2 below 2^53 (exact_dot), so <r_1, r_1> is exact at
    its scale 2^-10 and its root correctly rounded -- bitwise."""
    _, R = richardson_integers(shape, b, 1)
    return math.sqrt(exact_dot(R, R) / 1024.0)


# ---- the vector statements --------------------------------------------------------------------------------------------
#
# The elementwise half of BLAS-1 (fill, copy, *=, /=, +=, x + b y, a x + b z, r + s (a x + b z), BiCGStab's p, vmul,
# vmul_add, vdiv, multi_axpy) in two models.
#
# Integer model (``INT_STATEMENTS``): integer vectors, coefficients integers or dyadic fractions, divisors powers of
# two.  Every value is k / 2^s with |k| < 2^53 (``Dyadic``, asserted on every product and every sum), so every product
# and every sum is exact in fp64, every contraction choice gives the same bits, and a kernel is compared BITWISE
# whatever the compiler did.  The vectors depend on the row index (``stmt_vector``), so a shifted, swapped or repeated
# block cannot reproduce the expected vector.
#
# Rounding forms (``REAL_STATEMENTS``): on real-valued data a statement has a finite list of admissible evaluations of
# the reference's expression under "a product may be fused into the addition that consumes it".  Each form is a named
# vector of correctly rounded fp64 values: unfused steps are numpy's (one IEEE operation per ufunc, nothing contracts),
# fused ones come from exact integer ratios (``fma``: int / int is correctly rounded in CPython).  ``classify`` names the
# forms a result equals on EVERY element.

SENTINEL = -1.0e300  # pre-fill of a target: no statement below produces it


def stmt_vector(n, seed):
    """int_vector plus (row mod 1999): integers in [-1000, 2998] that depend on the row index."""
    return int_vector(n, seed) + (np.arange(n, dtype=np.int64) % 1999)


def pow2_vector(n, seed):
    """Divisors for vdiv: 1, 2, 4 or 8, by row and seed."""
    return np.int64(1) << ((np.arange(n, dtype=np.int64) + seed) % 4)


class Dyadic:
    """k / 2^s elementwise (k int64, |k| < 2^53): an fp64 value exactly.  Products and sums assert the bound on their
    result at the finer of the two scales, which covers every operand of every evaluation order.  A zero carries the
    sign IEEE arithmetic gives it (``neg0``: the rows that are -0; None: none) -- the same for every contraction choice,
    since the products are exact: (-0.25) * 0 is -0, and a sum is -0 only where both terms are."""

    def __init__(self, k, s=0, neg0=None):
        self.k = np.asarray(k, dtype=np.int64)
        self.s = int(s)
        self.neg0 = neg0
        assert self.mag() < EXACT, f"|k| reaches 2^53 ({self.mag()})"

    @classmethod
    def of(cls, c):
        """A scalar coefficient: an integer or a dyadic fraction."""
        q = Fraction(c)
        s = q.denominator.bit_length() - 1
        assert q.denominator == 1 << s, f"{c!r} is not dyadic"
        return cls(q.numerator, s)

    def mag(self):
        return int(np.abs(self.k).max(initial=0))

    def _negative(self):
        return (self.k < 0) if self.neg0 is None else ((self.k < 0) | self.neg0)

    def __mul__(self, o):
        assert self.mag() * o.mag() < EXACT, "a product reaches 2^53"
        k = self.k * o.k
        neg0 = (k == 0) & (self._negative() ^ o._negative())
        return Dyadic(k, self.s + o.s, neg0 if neg0.any() else None)

    def __add__(self, o):
        s = max(self.s, o.s)
        assert (self.mag() << (s - self.s)) + (o.mag() << (s - o.s)) < EXACT, "a sum reaches 2^53"
        neg0 = None if self.neg0 is None or o.neg0 is None else self.neg0 & o.neg0
        return Dyadic((self.k << (s - self.s)) + (o.k << (s - o.s)), s, neg0)

    def over_pow2(self, b):
        """Elementwise quotient by powers of two (positive int64)."""
        b = np.asarray(b, dtype=np.int64)
        assert b.size == 0 or (int(b.min()) > 0 and not int(np.bitwise_and(b, b - 1).max()))
        top = int(b.max(initial=1))
        return self * Dyadic(top // b, top.bit_length() - 1)

    def value(self):
        v = np.ldexp(self.k.astype(np.float64), -self.s)
        if self.neg0 is not None:
            v[np.broadcast_to(self.neg0, v.shape)] = -0.0
        return v


def _d(v):
    return v if isinstance(v, Dyadic) else (Dyadic(v) if isinstance(v, np.ndarray) else Dyadic.of(v))


def int_axpbz(a, x, b, z):
    return _d(a) * _d(x) + _d(b) * _d(z)


def int_lin3(r, s, a, x, b, z):
    return _d(r) + _d(s) * int_axpbz(a, x, b, z)


def int_multi_axpy(y, coefs, xs):
    acc = _d(y)
    for c, x in zip(coefs, xs):  # ascending j: the kernel's order, every partial sum asserted
        acc = acc + _d(c) * _d(x)
    return acc


# coefficients of the integer model: integers and dyadic fractions of both signs
I_FILL, I_SCALE, I_DIV, I_A1, I_AXPY, I_XPAY = 7.0, -0.25, 4.0, -0.25, 0.5, 3.0
I_A, I_B, I_S, I_BETA, I_OMEGA, I_VS, I_VD = 3.0, -0.25, 0.5, -0.25, 3.0, 0.5, 3.0
MAP_CONSTS = (3.0,)  # the fixed storm_hip_map program: y <<= 3 x0 + x1 * y  (RPN: x0 c0 * x1 y * +)


def multi_coefs_int(k):
    return [(0.5, -0.25, 3.0, -1.0, 2.0)[j % 5] for j in range(k)]


# name -> (number of vectors, the target's old value first; f(vectors) -> Dyadic).  The divisors of vdiv are the LAST vector.
INT_STATEMENTS = {
    "fill": (1, lambda v: Dyadic.of(I_FILL) * Dyadic(np.ones_like(v[0]))),
    "copy": (2, lambda v: _d(v[1])),
    "scale": (1, lambda v: _d(I_SCALE) * _d(v[0])),
    "div_scalar": (1, lambda v: _d(v[0]) * Dyadic.of(1 / Fraction(I_DIV))),
    "scaled_copy": (2, lambda v: _d(I_A1) * _d(v[1])),
    "axpy": (2, lambda v: int_axpbz(I_AXPY, v[1], 1, v[0])),
    "xpay": (2, lambda v: int_axpbz(1, v[1], I_XPAY, v[0])),
    "axpbz": (3, lambda v: int_axpbz(I_A, v[1], I_B, v[2])),
    "lin3": (4, lambda v: int_lin3(v[1], I_S, I_A, v[2], I_B, v[3])),
    "bicgstab_p": (3, lambda v: int_lin3(v[1], I_BETA, 1, v[0], -I_OMEGA, v[2])),
    "vmul_add": (3, lambda v: _d(v[0]) + _d(I_VS) * (_d(v[1]) * _d(v[2]))),
    "vmul": (3, lambda v: _d(v[1]) * _d(v[2])),
    "vdiv": (3, lambda v: (_d(I_VD) * _d(v[1])).over_pow2(v[2])),
    "vdiv_scalar": (2, lambda v: (_d(I_VD) * Dyadic(np.ones_like(v[1]))).over_pow2(v[1])),
    "map": (3, lambda v: _d(MAP_CONSTS[0]) * _d(v[1]) + _d(v[2]) * _d(v[0])),
}
MULTI_KS = (1, 2, 3, 4, 5, 8, 9, 19, 64)  # every multi_axpy_kernel<KB> unroll class (1-2, 3-4, 5-8) and the chunk boundary
for _k in MULTI_KS:
    INT_STATEMENTS[f"multi_axpy{_k}"] = (_k + 1, lambda v, _k=_k: int_multi_axpy(v[0], multi_coefs_int(_k), v[1:]))
DIVISOR_LAST = ("vdiv", "vdiv_scalar")


def int_operands(name, n, seed=0, distinct=None, make=stmt_vector):
    """The int64 vectors of a statement of the integer model (target first), each from its own seed.  ``distinct``:
    at most so many different INPUT vectors, repeated in turn (a long multi_axpy on long vectors; 4 is coprime to the
    period of its coefficients).  ``make(n, seed)`` builds a vector (a caller may cache)."""
    count = INT_STATEMENTS[name][0]
    vecs = [make(n, 101 + 7 * seed + (j if distinct is None or j == 0 else 1 + (j - 1) % distinct)) for j in range(count)]
    if name in DIVISOR_LAST:
        vecs[-1] = pow2_vector(n, seed)
    return vecs


def int_result(name, vecs):
    """The exact result as fp64; ``vecs`` may repeat an array (aliasing)."""
    return INT_STATEMENTS[name][1](vecs).value()


# ---- rounding forms -----------------------------------------------------------------------------------------------------


def fma(a, x, t):
    """One element of fma(a, x, t): the exact a x + t rounded once (IEEE, overflow and special values included)."""
    a, x, t = float(a), float(x), float(t)
    if not (math.isfinite(a) and math.isfinite(x)):
        with np.errstate(all="ignore"):
            return float(np.float64(a) * np.float64(x) + np.float64(t))  # (the product is +-inf or NaN exactly)
    if not math.isfinite(t):
        return t  # a finite product, however large, plus +-inf or NaN
    (an, ad), (xn, xd), (tn, td) = a.as_integer_ratio(), x.as_integer_ratio(), t.as_integer_ratio()
    num, den = an * xn * td + tn * ad * xd, ad * xd * td  # the exact a x + t (the denominators are powers of two)
    if num == 0:
        return a * x + t  # a x = -t exactly: the float expression is exact and carries the IEEE sign of the zero
    try:
        return num / den  # int / int is correctly rounded in CPython, subnormal results included
    except OverflowError:
        return math.inf if num > 0 else -math.inf


def vfma(a, x, t):
    """fma elementwise; scalars broadcast."""
    a, x, t = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(x, np.float64), np.asarray(t, np.float64))
    out = np.empty(a.shape, np.float64)
    flat = out.reshape(-1)
    for i, (ai, xi, ti) in enumerate(zip(a.reshape(-1).tolist(), x.reshape(-1).tolist(), t.reshape(-1).tolist())):
        flat[i] = fma(ai, xi, ti)
    return out


def _unit(c):
    return c == 1.0 or c == -1.0  # fma(+-1, x, t) == fl(+-x + t): the fused form is the unfused one by construction


def forms_axpbz(a, x, b, z):
    """a x + b z: ``none`` fl(fl(a x) + fl(b z)); ``fuse_x`` fma(a, x, fl(b z)); ``fuse_z`` fma(b, z, fl(a x)).  A form
    that is another one by construction (a coefficient +-1) is left out."""
    a, b = np.float64(a), np.float64(b)
    with np.errstate(all="ignore"):
        ax, bz = a * x, b * z
        forms = {"none": ax + bz}
    if not _unit(a):
        forms["fuse_x"] = vfma(a, x, bz)
    if not _unit(b):
        forms["fuse_z"] = vfma(b, z, ax)
    return forms


def forms_outer(r, s, inner):
    """r + s t for every form t of the inner sum: ``<inner>/none`` fl(r + fl(s t)), ``<inner>/fused`` fma(s, t, r)."""
    s = np.float64(s)
    forms = {}
    for name, t in inner.items():
        with np.errstate(all="ignore"):
            forms[f"{name}/none"] = r + s * t
        if not _unit(s):
            forms[f"{name}/fused"] = vfma(s, t, r)
    return forms


def forms_lin3(r, s, a, x, b, z):
    return forms_outer(r, s, forms_axpbz(a, x, b, z))


def forms_vmul_add(y, s, a, b):
    with np.errstate(all="ignore"):
        return forms_outer(y, s, {"prod": a * b})  # (the inner product feeds a product: never fused)


def forms_multi_axpy(y, coefs, xs):
    """All k steps fused, or none, in ascending j -- straight through the chunk boundary at k = 9."""
    none, fused = np.array(y, np.float64), np.array(y, np.float64)
    for c, x in zip(coefs, xs):
        with np.errstate(all="ignore"):
            none = none + np.float64(c) * x
        fused = vfma(c, x, fused)
    return {"none": none, "fused": fused}


def _one(value):
    return {"exact": value}


# the non-dyadic coefficients of the rounding-form fixtures
R_FILL, R_SCALE, R_DIV, R_A1, R_AXPY, R_XPAY = 0.3, 0.3, 0.7, -0.3, 0.3, 0.7
R_A, R_B, R_S, R_BETA, R_OMEGA, R_VS, R_VD = 0.75, -1.25, 0.3, 0.3, 0.7, 0.3, 0.3


def multi_coefs_real(k):
    return [0.3 + 0.07 * j for j in range(k)]


def _np(f):
    def g(v):
        with np.errstate(all="ignore"):
            return _one(f(v))
    return g


# name -> (number of vectors, target first; f(vectors) -> {form: fp64 vector})
REAL_STATEMENTS = {
    "fill": (1, _np(lambda v: np.full_like(v[0], R_FILL))),
    "copy": (2, _np(lambda v: v[1].copy())),
    "scale": (1, _np(lambda v: v[0] * np.float64(R_SCALE))),
    "div_scalar": (1, _np(lambda v: v[0] / np.float64(R_DIV))),
    "scaled_copy": (2, _np(lambda v: np.float64(R_A1) * v[1])),
    "axpy": (2, lambda v: forms_axpbz(R_AXPY, v[1], 1.0, v[0])),
    "xpay": (2, lambda v: forms_axpbz(1.0, v[1], R_XPAY, v[0])),
    "axpbz": (3, lambda v: forms_axpbz(R_A, v[1], R_B, v[2])),
    "lin3": (4, lambda v: forms_lin3(v[1], R_S, R_A, v[2], R_B, v[3])),
    "bicgstab_p": (3, lambda v: forms_lin3(v[1], R_BETA, 1.0, v[0], -R_OMEGA, v[2])),
    "vmul_add": (3, lambda v: forms_vmul_add(v[0], R_VS, v[1], v[2])),
    "vmul": (3, _np(lambda v: v[1] * v[2])),
    "vdiv": (3, _np(lambda v: (np.float64(R_VD) * v[1]) / v[2])),
    "vdiv_scalar": (2, _np(lambda v: np.float64(R_VD) / v[1])),
    "map": (3, _np(lambda v: np.float64(MAP_CONSTS[0]) * v[1] + v[2] * v[0])),  # (every operation a statement: no fusing)
}
for _k in MULTI_KS:
    REAL_STATEMENTS[f"multi_axpy{_k}"] = (_k + 1, lambda v, _k=_k: forms_multi_axpy(v[0], multi_coefs_real(_k), v[1:]))

REAL_ROWS = (1, 3, 2049, 4096, 100003)
# multi_axpy at 100 003 rows costs k exact fmas per row: one width per unroll class there (1, 3) and the chunk
# boundary (9); the other widths stay at the sizes up to 4096
REAL_LONG_NAMES = tuple(n for n in REAL_STATEMENTS if not n.startswith("multi_axpy") or int(n[10:]) in (1, 3, 9))


def real_rows(name):
    return REAL_ROWS if name in REAL_LONG_NAMES else REAL_ROWS[:-1]


def forms_differ(forms):
    """All forms pairwise different on every element of (short) vectors."""
    vals = list(forms.values())
    return all(bool(np.all(bits(vals[i]) != bits(vals[j]))) for i in range(len(vals)) for j in range(i))


_REAL_CACHE = {}


def real_operands(name, n):
    """Standard-normal vectors of a statement (target first), seeded by the statement and the size, and their forms.
    The LAST row is redrawn from the same stream until every two forms differ on it: the odd tail of a kernel (and the
    only row of a one-row vector) then always tells the forms apart -- the seed chosen so that the condition of
    tests/test_exact_reference.py holds."""
    key = (name, n)
    if key not in _REAL_CACHE:
        count, fn = REAL_STATEMENTS[name]
        rng = np.random.default_rng([sorted(REAL_STATEMENTS).index(name), n])
        vecs = [rng.standard_normal(n) for _ in range(count)]
        for _ in range(100000):
            tail = [v[-1:] for v in vecs]
            if forms_differ(fn(tail)):
                break
            for v in vecs:
                v[-1] = rng.standard_normal()
        else:
            raise AssertionError(f"{name}: no last row separates the forms")
        _REAL_CACHE[key] = (vecs, fn(vecs))
    return _REAL_CACHE[key]


def bits(a):
    """fp64 values as their bit patterns, every NaN as one pattern."""
    a = np.ascontiguousarray(a, np.float64)
    b = a.view(np.uint64).copy()
    b[np.isnan(a)] = np.uint64(0x7ff8000000000000)
    return b


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.array_equal(bits(a), bits(b)))


def classify(got, forms):
    """The names of the forms that ``got`` equals, bit for bit, on EVERY element."""
    return [name for name, value in forms.items() if same_bits(got, value)]


def differing_share(forms):
    """{(form, form): share of the elements on which the two differ} for every pair of forms."""
    names = list(forms)
    return {(p, q): float(np.mean(bits(forms[p]) != bits(forms[q]))) if forms[p].size else 0.0
            for i, p in enumerate(names) for q in names[:i]}


# Operand aliasings the header allows ("y may alias x or z", "y may alias any operand", "may alias a or b"): operand i
# of the statement (target first, INT_STATEMENTS' order) is vector ALIASINGS[name][..][i].
_THREE = [(0, 0, 2), (0, 1, 0), (0, 1, 1), (0, 0, 0)]  # y is x; y is z; x is z; all three
ALIASINGS = {
    "copy": [(0, 0)],
    "axpbz": _THREE,
    "bicgstab_p": _THREE,
    "vmul": _THREE,
    "vmul_add": _THREE,
    "vdiv": _THREE,
    "lin3": [(0, 0, 2, 3), (0, 1, 0, 3), (0, 1, 2, 0), (0, 1, 2, 2), (0, 0, 2, 2), (0, 0, 0, 0)],
}


def aliased_operands(name, n, amap, seed=0, make=stmt_vector):
    """int_operands with operand i taken from vector amap[i] (a divisor vector stays a vector of powers of two)."""
    base = int_operands(name, n, seed, make=make)
    if name in DIVISOR_LAST:
        base[-1] = make(n, 99 + seed)
        base[amap[-1]] = pow2_vector(n, seed)
    return [base[i] for i in amap]


# ---- the loop shape of the streaming kernels, as a model ------------------------------------------------------------------
#
# Which rows ew_kernel (and lin3_kernel, multi_axpy_kernel, map_kernel, lazy_lin_kernel: the same shape) writes: pairs of
# rows i < n >> 1 in a grid-stride loop over min(ceil(n / 2048), 32768) blocks of 1024 pairs, and the odd last row by
# thread 0 of block 0.  With ``mutation`` one line of it is edited -- the edits a test of these kernels must catch;
# tests/test_exact_reference.py shows at which of the GPU tests' row counts each one changes the result.
STMT_SMALL_ROWS = (1, 2, 3, 2047, 2048, 2049, 4097, 12345)
STMT_BIG_ROWS = ((1 << 26) - 3, 1 << 26, (1 << 26) + 1, (1 << 26) + 2, (1 << 26) + 2049, (1 << 27) + 2051)
MAX_STREAM_BLOCKS = 32768  # kMaxStreamBlocks (common.hpp)
LOOP_MUTATIONS = ("dropped_pair", "tail_guard_block_1", "one_trip")


def loop_model(result, before, mutation=None):
    """What the target holds after the kernel: ``result`` on the rows the loop writes, ``before`` elsewhere.
    dropped_pair: `n2 = (n >> 1) - 1`; tail_guard_block_1: the tail guard `bx == 0` changed to `bx == 1`; one_trip: the
    grid-stride `for` turned into an `if`."""
    assert mutation is None or mutation in LOOP_MUTATIONS
    n = result.size
    out = before.copy()
    if n == 0:
        return out
    grid = min(max(1, -(-n // STREAM_BLOCK)), MAX_STREAM_BLOCKS)
    n2 = (n >> 1) - (1 if mutation == "dropped_pair" else 0)
    pairs = max(0, min(n2, grid * (STREAM_BLOCK // 2)) if mutation == "one_trip" else n2)
    out[:2 * pairs] = result[:2 * pairs]
    tail_block = 1 if mutation == "tail_guard_block_1" else 0
    if (n & 1) and tail_block < grid:
        out[n - 1] = result[n - 1]
    return out
