"""The mixed-precision CG of include/storm_hip.h ("Mixed-precision CG"), restated in numpy: float32 storage of the inner
vectors, float64 arithmetic and sums, one conversion at each float32 store, the fp64 outer loop on the true residual.

It is a restatement of the ALGORITHM -- the iteration and outer-step counts the tests compare come from here -- not of the
kernels' bits: numpy has no fused multiply-add and sums in another order (the bitwise pins of tests/test_gpu_mixed_cg.py use
the library's own fp64 statements).  `a` is the fp64 operator, `a32` the same operator assembled from the weights rounded to
float32 (scipy CSR, float64 values), the model of the companion records."""
import os

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BROKEN = 2


def f32(v):
    return np.asarray(v, np.float64).astype(np.float32)


def wide(v):
    return np.asarray(v, np.float32).astype(np.float64)


def rule(abs_err, rho0, abs_tol, rel_tol):
    """Solver.hpp:116-147 on a residual norm."""
    return bool((abs_tol > 0.0 and abs_err < abs_tol) or (rel_tol > 0.0 and abs_err / rho0 < rel_tol))


def rule_target(rho0, abs_tol, rel_tol):
    t = 0.0
    if abs_tol > 0.0:
        t = abs_tol
    if rel_tol > 0.0:
        t = max(t, rel_tol * rho0)
    return t


def cg64(a, b, x0=None, abs_tol=1e-6, rel_tol=1e-6, num_iterations=2000):
    """Plain float64 CG (SolverCg.hpp:47-128) under the rule: (x, iterations, converged, history)."""
    x = np.zeros_like(b) if x0 is None else np.array(x0, np.float64)
    r = b - a @ x
    rho0 = float(np.linalg.norm(r))
    hist = [rho0]
    if abs_tol > 0.0 and rho0 < abs_tol:
        return x, 0, True, np.array(hist)
    p, g = r.copy(), float(r @ r)
    for it in range(1, num_iterations + 1):
        z = a @ p
        al = g / float(p @ z)
        x += al * p
        r -= al * z
        gn = float(r @ r)
        p = r + (gn / g) * p
        g = gn
        hist.append(float(np.sqrt(g)))
        if rule(hist[-1], rho0, abs_tol, rel_tol):
            return x, it, True, np.array(hist)
    return x, num_iterations, False, np.array(hist)


def inner_loop(a32, r32, p32, eta, inner_max):
    """The fp32 inner iterations from (r32, p32), d32 = 0: (d32, r32, p32, iterations, broken)."""
    d32 = np.zeros_like(r32)
    g = float(wide(r32) @ wide(r32))
    broken, it = False, 0
    for it in range(1, inner_max + 1):
        p = wide(p32)
        q32 = f32(a32 @ p)
        pq = float(p @ wide(q32))
        if not (pq > 0.0) or not np.isfinite(pq):
            broken = True
            break
        al = g / pq
        d32 = f32(al * p + wide(d32))
        r32 = f32(-al * wide(q32) + wide(r32))
        gn = float(wide(r32) @ wide(r32))
        if not np.isfinite(gn):
            broken = True
            break
        bt = gn / g
        p32 = f32(wide(r32) + bt * p)
        g = gn
        if np.sqrt(gn) <= eta:
            break
    return d32, r32, p32, it, broken


def mixed_cg(a, a32, b, x0=None, abs_tol=1e-6, rel_tol=1e-6, num_iterations=2000, inner_tolerance=1e-3, inner_max=0,
             max_outer=16, keep_direction=0):
    """dict(x, converged, outer_steps, inner_iterations, fp64_iterations, finished_fp64, history)."""
    x = np.zeros_like(b) if x0 is None else np.array(x0, np.float64)
    r = b - a @ x
    rho0 = float(np.linalg.norm(r))
    out = dict(x=x, converged=False, outer_steps=0, inner_iterations=0, fp64_iterations=0, finished_fp64=0, history=[rho0])
    if abs_tol > 0.0 and rho0 < abs_tol:
        out["converged"] = True
        return out
    target = rule_target(rho0, abs_tol, rel_tol)
    rho, rho_prev, p32, finish = rho0, rho0, None, 0
    while not out["converged"] and finish == 0 and num_iterations > 0:
        left = num_iterations - out["inner_iterations"]
        cap = min(inner_max if inner_max > 0 else num_iterations, left)
        r32 = f32(r * (1.0 / rho))
        p32 = f32(wide(p32) * (rho_prev / rho)) if (keep_direction and out["outer_steps"] > 0) else r32.copy()
        eta = max(inner_tolerance, 0.5 * target / rho)
        d32, _, p32, its, broken = inner_loop(a32, r32, p32, eta, cap)
        if not broken:
            x = x + rho * wide(d32)
        r = b - a @ x
        rho_new = float(np.linalg.norm(r))
        out["outer_steps"] += 1
        out["inner_iterations"] += its
        out["history"].append(rho_new)
        rho_prev = rho
        out["converged"] = rule(rho_new, rho0, abs_tol, rel_tol)
        if not out["converged"]:
            if broken:
                finish = BROKEN
            elif not rho_new < rho:
                finish = 1
            elif out["outer_steps"] >= max_outer or out["inner_iterations"] >= num_iterations:
                finish = 3
        rho = rho_new
    if not out["converged"] and finish == 0:
        finish = 3
    if not out["converged"] and out["inner_iterations"] < num_iterations:
        x, its, conv, hist = cg64(a, b, x, abs_tol, rel_tol * rho0 / rho if rel_tol > 0.0 else 0.0,
                                  num_iterations - out["inner_iterations"])
        out["fp64_iterations"], out["converged"] = its, conv
        out["history"] += list(hist[1:])
    out["x"], out["finished_fp64"], out["history"] = x, finish, np.array(out["history"])
    return out


# ---- the operators of the tests, as host data ---------------------------------------------------------------------------
def face_operator(n, inner, outer, w, diag_extra):
    """A = -M for the face-weight operator M (symmetric weights w, diagonal term diag_extra) as scipy CSR:
    (A x)_i = sum_faces w (x_i - x_j) - diag_extra_i x_i -- StencilMatrix.from_face_weights applied with alpha = -1, beta = 0."""
    inner, outer = np.asarray(inner, np.int64), np.asarray(outer, np.int64)
    w, diag_extra = np.asarray(w, np.float64), np.asarray(diag_extra, np.float64)
    rows = np.concatenate([inner, outer, inner, outer, np.arange(n)])
    cols = np.concatenate([outer, inner, inner, outer, np.arange(n)])
    vals = np.concatenate([-w, -w, w, w, -diag_extra])
    a = sp.coo_matrix((vals, (rows, cols)), shape=(n, n)).tocsr()
    a.sum_duplicates()
    return a


def face_operator_pair(n, inner, outer, w, diag_extra):
    """(A, A~): the operator and the one assembled from the weights and the diagonal term rounded to float32."""
    return face_operator(n, inner, outer, w, diag_extra), face_operator(n, inner, outer, wide(f32(w)), wide(f32(diag_extra)))


def box_faces(nx, ny, nz):
    inner, outer = [], []
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                c = i + nx * (j + ny * k)
                if i + 1 < nx:
                    inner.append(c), outer.append(c + 1)
                if j + 1 < ny:
                    inner.append(c), outer.append(c + nx)
                if k + 1 < nz:
                    inner.append(c), outer.append(c + nx * ny)
    return np.array(inner, np.int64), np.array(outer, np.int64)


def chain_faces(n):
    i = np.arange(n - 1, dtype=np.int64)
    return i, i + 1


def jittered_case(n, inner, outer, seed, shift=0.05):
    """Random (not power-of-two) symmetric face weights in [0.5, 1.5) and a diagonal term -shift (1 + u), u in [0, 1):
    A is symmetric positive definite.  Returns (w, diag_extra)."""
    rng = np.random.default_rng(seed)
    return rng.uniform(0.5, 1.5, np.asarray(inner).size), -shift * (1.0 + rng.uniform(0.0, 1.0, n))


def solve_cases():
    """{name: (n, inner, outer, w, diag_extra)} of the solve tests: the 24^3 box with Dirichlet walls, a jittered
    37 x 21 x 19 box, the reference's triangles (square_nb.1) with jittered weights."""
    from stormruler_amd import io_tetgen

    out = {}
    i, o = box_faces(24, 24, 24)
    n = 24 ** 3
    walls = np.full(n, 6.0)
    np.subtract.at(walls, i, 1.0)
    np.subtract.at(walls, o, 1.0)
    out["box24"] = (n, i, o, np.ones(i.size), -2.0 * walls)
    i, o = box_faces(37, 21, 19)
    out["jitter37x21x19"] = (37 * 21 * 19, i, o) + jittered_case(37 * 21 * 19, i, o, seed=7)
    tri = io_tetgen.read_triangle(os.path.join(ROOT, "tests", "golden", "mesh", "square_nb.1."))
    i, o = np.asarray(tri.inner, np.int64), np.asarray(tri.outer, np.int64)
    out["square_nb"] = (tri.n_cells, i, o) + jittered_case(tri.n_cells, i, o, seed=9)
    return out


def rhs(n, kind):
    return np.ones(n) if kind == "ones" else np.random.default_rng(5).standard_normal(n)
