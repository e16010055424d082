"""The recipe of storm_hip_recycle (include/storm_hip.h) restated once, over a number space.

THE RECIPE.
  kind 0 is the energy projection, for SPD operators: the test vector is t_j = u_j, the norm is N(a, b) = <a, b> on
    (u, v), and g_j = 1 / <u_j, v_j>.
  kind 1 is residual-minimising, for any operator: t_j = v_j, the norm is <v, v>, and g_j = 1 / <v_j, v_j>.
  count is known to the host.  Slots j >= count are empty.  A slot with g_j = 0 contributes nothing.

  guess(b, x):
    e_j = <t_j, b> for j < count.
    c_j = g_j * e_j.  The c values are kept on the device for the next update.
    x = ((0 + c_0 u_0) + c_1 u_1) + ...: one fma per term, ascending j, starting from +0.0.
    Owned rows only.  Halo rows are left as they are.
    count == 0 gives x = 0.

  update(x, ax), count < m, s = count:
    d = x - sum_{j<s} c_j u_j and ad = ax - sum_{j<s} c_j v_j.  Each is a chain fma(-c_j, ., acc) in ascending j,
      starting from x or ax.
    e_j = <t_j, ad>.  nu0 = <d, ad> for kind 0, <ad, ad> for kind 1.
    beta_j = g_j e_j.  u_s = d - sum beta_j u_j and v_s = ad - sum beta_j v_j, the same chains.
    nu = <u_s, v_s> for kind 0, <v_s, v_s> for kind 1.
    g_s = 1 / nu if nu is finite, nu > 0 and nu > 2^-40 nu0.  Otherwise g_s = 0.  (The 2^-40 guard is the multigrid coarse
      level's pivot rule.)  g_s is decided by the block that finishes the reduction.
    count += 1.
    An update with no guess since the last update uses c = 0, so d = x (the first chain is not run).

  update at count == m: restart.
    u_0 = x, v_0 = ax, nu = N(x, ax), g_0 by the same guard with nu0 = nu.
    g_j = 0 for j > 0.
    count = 1.  The restarts counter goes up by one.

  reset() sets count = 0 and clears every g_j.

Two number spaces run it: ``Exact`` (Fractions: nothing rounds) and ``F64`` (fp64 numpy: every product c_j = g_j e_j, every
1 / nu and every fma of a chain rounds once, the chains in the stated order; a dot is numpy's).  ``fma`` is
float(Fraction(a) * Fraction(b) + Fraction(c)).  Also here: a small CG for the CPU checks, the designed integer data of
the exactness test and the right-hand sides of the box sequence.  Plain module, not a conftest.
"""
import math
from fractions import Fraction

import numpy as np

GUARD = Fraction(1, 1 << 40)


def fma(a, b, c):
    """float(Fraction(a) * Fraction(b) + Fraction(c)): the exact a b + c, rounded once.  (Fraction(float) is the float's
    integer ratio, and int / int rounds correctly; a zero sum takes the sign IEEE gives it; non-finite operands: a b + c.)"""
    a, b, c = float(a), float(b), float(c)
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        with np.errstate(all="ignore"):
            return float(np.float64(a) * np.float64(b) + np.float64(c))
    (an, ad), (bn, bd), (cn, cd) = a.as_integer_ratio(), b.as_integer_ratio(), c.as_integer_ratio()
    num, den = an * bn * cd + cn * ad * bd, ad * bd * cd
    if num == 0:
        return a * b + c
    try:
        return num / den
    except OverflowError:
        return math.inf if num > 0 else -math.inf


class Exact:
    """Vectors are object arrays of Fractions; nothing rounds."""

    name = "exact"

    @staticmethod
    def vec(a):
        return np.array([Fraction(v) for v in np.asarray(a).tolist()], dtype=object)

    @staticmethod
    def zeros(n):
        return np.array([Fraction(0)] * n, dtype=object)

    @staticmethod
    def scalar(v):
        return Fraction(v)

    @staticmethod
    def dot(a, b):
        return sum((x * y for x, y in zip(a.tolist(), b.tolist())), Fraction(0))

    @staticmethod
    def mul(g, e):
        return g * e

    @staticmethod
    def axpy(c, u, acc):  # acc + c u, elementwise
        return acc + c * u

    @staticmethod
    def weight(nu, nu0):
        return 1 / nu if (nu > 0 and nu > GUARD * nu0) else Fraction(0)


class F64:
    """Vectors are float64 arrays; a chain term is one fma, c = g e one product, 1 / nu one division."""

    name = "fp64"

    @staticmethod
    def vec(a):
        return np.array(a, dtype=np.float64)

    @staticmethod
    def zeros(n):
        return np.zeros(n, np.float64)

    @staticmethod
    def scalar(v):
        return float(v)

    @staticmethod
    def dot(a, b):
        with np.errstate(all="ignore"):
            return float(np.dot(a, b))

    @staticmethod
    def mul(g, e):
        with np.errstate(all="ignore"):
            return float(np.float64(g) * np.float64(e))

    @staticmethod
    def axpy(c, u, acc):
        out = np.array(acc, dtype=np.float64)
        if not math.isfinite(c):
            touched = np.arange(out.size)
        elif c == 0.0 and np.all(np.isfinite(u)):
            touched = np.nonzero(acc == 0.0)[0]  # (acc + (+-0) = acc except for the sign of a zero)
        else:
            touched = np.nonzero((u != 0.0) | (acc == 0.0) | ~np.isfinite(u))[0]
        ul, al = u[touched].tolist(), acc[touched].tolist()
        out[touched] = [fma(c, x, t) for x, t in zip(ul, al)]
        return out

    @staticmethod
    def weight(nu, nu0):
        with np.errstate(all="ignore"):
            ok = math.isfinite(nu) and nu > 0.0 and nu > float(np.float64(2.0 ** -40) * np.float64(nu0))
        return 1.0 / nu if ok else 0.0


class Recycler:
    """The recipe.  ``u``, ``v``: the slots (lists of vectors of the space), ``g``, ``c``: the scalars."""

    def __init__(self, space, n, capacity, kind):
        assert 1 <= capacity <= 16 and kind in (0, 1)
        self.sp, self.n, self.m, self.kind = space, n, capacity, kind
        self.u, self.v = [None] * capacity, [None] * capacity
        self.g = [space.scalar(0)] * capacity
        self.c = None  # the coefficients of the last guess, until an update takes them
        self.count = self.updates = self.restarts = 0
        self.last = {}  # e, nu0, beta, nu of the last update

    def t(self, j):
        return self.v[j] if self.kind else self.u[j]

    def norm(self, a, b):
        return self.sp.dot(b, b) if self.kind else self.sp.dot(a, b)

    def set_slot(self, j, u, v, g):
        assert j <= self.count and j < self.m
        self.u[j], self.v[j], self.g[j] = self.sp.vec(u), self.sp.vec(v), self.sp.scalar(g)
        self.count = max(self.count, j + 1)
        self.c = None

    def guess(self, b):
        sp = self.sp
        b = sp.vec(b)
        x = sp.zeros(self.n)
        e = [sp.dot(self.t(j), b) for j in range(self.count)]
        c = [sp.mul(self.g[j], e[j]) for j in range(self.count)]
        for j in range(self.count):
            x = sp.axpy(c[j], self.u[j], x)
        self.c = c if self.count else None
        return x

    def update(self, x, ax):
        sp = self.sp
        x, ax = sp.vec(x), sp.vec(ax)
        self.updates += 1
        if self.count == self.m:  # restart
            nu = self.norm(x, ax)
            self.u[0], self.v[0] = x, ax
            self.g = [sp.weight(nu, nu)] + [sp.scalar(0)] * (self.m - 1)
            self.count, self.c = 1, None
            self.restarts += 1
            self.last = {"e": [], "nu0": nu, "beta": [], "nu": nu}
            return
        s = self.count
        d, ad = x, ax
        if self.c is not None:
            for j in range(s):
                d, ad = sp.axpy(-self.c[j], self.u[j], d), sp.axpy(-self.c[j], self.v[j], ad)
        e = [sp.dot(self.t(j), ad) for j in range(s)]
        nu0 = self.norm(d, ad)
        beta = [sp.mul(self.g[j], e[j]) for j in range(s)]
        us, vs = d, ad
        for j in range(s):
            us, vs = sp.axpy(-beta[j], self.u[j], us), sp.axpy(-beta[j], self.v[j], vs)
        nu = self.norm(us, vs)
        self.u[s], self.v[s], self.g[s] = us, vs, sp.weight(nu, nu0)
        self.count, self.c = s + 1, None
        self.last = {"e": e, "nu0": nu0, "beta": beta, "nu": nu, "d": d, "ad": ad}

    def reset(self):
        self.count, self.c = 0, None
        self.g = [self.sp.scalar(0)] * self.m


# ---- a small CG and the box sequence ------------------------------------------------------------------------------------


def box_apply(shape):
    """x -> (-L) x of the unit box (exact_ref.unit_box) in fp64."""
    import exact_ref

    nx, ny, nz = shape

    def apply(x):
        return exact_ref._stencil(np.asarray(x, np.float64).reshape(nz, ny, nx)).reshape(-1)

    return apply


def cg(apply, b, x0, abs_tol, max_iter=2000):
    """CG as the library's loop runs it: stop when the recursive |r| < abs_tol (checked before the first iteration too).
    Returns (x, iterations, |r0|, converged)."""
    x = np.array(x0, np.float64)
    r = b - apply(x)
    rr = float(r @ r)
    r0 = math.sqrt(rr)
    if r0 < abs_tol:
        return x, 0, r0, True
    p = r.copy()
    for k in range(1, max_iter + 1):
        z = apply(p)
        alpha = rr / float(p @ z)
        x += alpha * p
        r -= alpha * z
        rr_new = float(r @ r)
        if math.sqrt(rr_new) < abs_tol:
            return x, k, r0, True
        p = r + (rr_new / rr) * p
        rr = rr_new
    return x, max_iter, r0, False


BOX_SHAPE = (12, 10, 9)
BOX_SOLVES = 14
BOX_TOL = 1e-8  # absolute tolerance BOX_TOL |b_t|, relative 0
# what the GPU test asserts, and the CPU test holds the restatement alone to
BOX_RATIO = 0.5            # recycled total of iterations <= BOX_RATIO x the warm total
BOX_CAPPED = range(3, 9)   # solves 4 .. 9 counted from 1 (t = 3 .. 8: the object holds 3 .. 8 pairs) ...
BOX_CAP = 8                # ... need at most this many iterations each
BOX_FREE = 9               # solve 10 (t = 9) follows the restart at capacity 8: it is free, no cap of its own


def box_fields():
    n = BOX_SHAPE[0] * BOX_SHAPE[1] * BOX_SHAPE[2]
    i = np.arange(n, dtype=np.float64)
    return np.sin(0.37 * i), np.cos(np.mod(0.11 * i * i, 7.0)), np.mod(7919.0 * i, 13.0) - 6.0


def box_rhs(t):
    """b_t = f0 + sin(0.3 t) f1 + cos(0.2 t) f2."""
    f0, f1, f2 = box_fields()
    return f0 + math.sin(0.3 * t) * f1 + math.cos(0.2 * t) * f2


def box_sequence(capacity, kind, space=F64):
    """The box sequence on the CPU: capacity 0 is the warm-start arm.  Per solve (iterations, |r0|, converged, true residual)."""
    apply = box_apply(BOX_SHAPE)
    n = BOX_SHAPE[0] * BOX_SHAPE[1] * BOX_SHAPE[2]
    rec = Recycler(space, n, capacity, kind) if capacity else None
    x = np.zeros(n)
    out = []
    for t in range(BOX_SOLVES):
        b = box_rhs(t)
        tol = BOX_TOL * float(np.linalg.norm(b))
        if rec is not None:
            x = np.asarray(rec.guess(b), np.float64)
        x, it, r0, ok = cg(apply, b, x, tol)
        if rec is not None:
            rec.update(x, apply(x))
        out.append((it, r0, ok, float(np.linalg.norm(b - apply(x)))))
    return out


# ---- the designed integer data ---------------------------------------------------------------------------------------------


def hadamard(q):
    h = np.array([[1]], dtype=np.int64)
    for _ in range(q):
        h = np.block([[h, h], [h, -h]])
    return h


def designed_q(n):
    """The sign patterns live on the last 2^q rows: as many as fit behind row 0 (which stays zero), at most 16."""
    return min(4, int(math.floor(math.log2(n - 1)))) if n >= 2 else 0


def designed_slots(n, loaded, kind):
    """``loaded`` pairs (u_j, v_j = 2 u_j, g_j): u_j = column j of the 2^q Hadamard matrix on the last 2^q rows (+-1; the
    odd last row carries data, row 0 is zero), so <u_i, v_j> = 0 for i != j and nu = 2 * 2^q (kind 1: 4 * 2^q), a power of
    two: g_j = 1 / nu is exact.  Beyond the 2^q columns there are no more orthogonal patterns: those pairs are zero vectors
    with g_j = 0, the slot that contributes nothing."""
    q = designed_q(n)
    w = 1 << q
    h = hadamard(q)
    slots = []
    for j in range(loaded):
        u = np.zeros(n, np.int64)
        if j < w:
            u[n - w:] = h[:, j]
            nu = (4 if kind else 2) * w
            slots.append((u, 2 * u, Fraction(1, nu)))
        else:
            slots.append((u, 2 * u, Fraction(0)))
    return slots


def designed_vectors(n, seed):
    """Dense integer b, x (|.| <= 100, no zero) and ax = 2 x: the test owns the operator, A = 2 I."""
    rng = np.random.default_rng(seed)

    def dense():
        a = rng.integers(1, 101, size=n, dtype=np.int64)
        return a * rng.choice(np.array([-1, 1], dtype=np.int64), size=n)

    b, x, b2 = dense(), dense(), dense()
    return b, x, 2 * x, b2


def designed_is_exact(n, loaded, kind, seed=0):
    """The exactness conditions of the designed data, checked on the Exact run of guess(b) / update(x, 2 x): every g, c
    and beta is a dyadic rational fp64 holds exactly, and every vector element, every term of every chain and of every
    sum, and the sum of the absolute values of a sum's terms -- a bound on every partial sum in ANY order -- is an integer
    multiple of ONE power of two, 2^-unit, below 2^53 of them."""
    def dyadic(v, unit=12):
        f = Fraction(v) * (1 << unit)
        return f.denominator == 1 and abs(f.numerator) < (1 << 53)

    r = Recycler(Exact, n, max(loaded + 1, 1), kind)
    for j, (u, v, g) in enumerate(designed_slots(n, loaded, kind)):
        r.set_slot(j, u, v, g)
    b, x, ax, _ = designed_vectors(n, seed)
    xg = r.guess(b)
    c = list(r.c or [])
    ok = all(dyadic(v) for v in xg.tolist()) and all(dyadic(v) for v in c) and all(dyadic(v) for v in r.g)
    for j in range(r.count):
        ok = ok and dyadic(sum(abs(a * bb) for a, bb in zip(r.t(j).tolist(), Exact.vec(b).tolist())))
        ok = ok and all(dyadic(c[j] * a) for a in r.u[j].tolist())
    r.update(x, ax)
    last, s = r.last, r.count - 1
    d, ad = last.get("d", Exact.vec(x)), last.get("ad", Exact.vec(ax))
    for j in range(s):
        ok = ok and dyadic(last["beta"][j]) and dyadic(sum(abs(a * bb) for a, bb in zip(r.t(j).tolist(), ad.tolist())))
        ok = ok and all(dyadic(last["beta"][j] * a) and dyadic(last["beta"][j] * 2 * a) for a in r.u[j].tolist())
    w0, ws = (ad if kind else d), (r.v[s] if kind else r.u[s])
    ok = ok and dyadic(sum(abs(a * bb) for a, bb in zip(w0.tolist(), ad.tolist())))
    ok = ok and dyadic(sum(abs(a * bb) for a, bb in zip(ws.tolist(), r.v[s].tolist())))
    ok = ok and all(dyadic(v) for v in r.u[s].tolist()) and all(dyadic(v) for v in r.v[s].tolist())
    return bool(ok)


def designed_run(n, capacity, loaded, kind, seed=0):
    """The F64 restatement on the designed data: guess(b) -> x0, update(x, 2 x) -> slot s, g_s, then guess(b2) -> x1 (one
    rounded g_s in it).  Returns the recycler and a dict of what the device is held to, bit for bit."""
    r = Recycler(F64, n, capacity, kind)
    for j, (u, v, g) in enumerate(designed_slots(n, loaded, kind)):
        r.set_slot(j, u, v, float(g))
    b, x, ax, b2 = designed_vectors(n, seed)
    x0 = r.guess(b)
    c0 = list(r.c or [])
    r.update(x, ax)
    s = r.count - 1
    x1 = r.guess(b2)
    return r, {"b": b, "x": x, "ax": ax, "b2": b2, "x0": x0, "c0": c0, "s": s, "u_s": r.u[s].copy(), "v_s": r.v[s].copy(),
               "g_s": r.g[s], "x1": x1, "c1": list(r.c or [])}
