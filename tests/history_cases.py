"""A catalogue of small solves, one per solver path, and of disturbances that leave state behind in a context -- the data of
tests/test_gpu_history_independence.py (a solve's result bits are those the same solve gives in a context that has done
nothing else) and of tests/test_history_cases_host.py (the checks on this catalogue that need no device).

A CASE builds its operators once per context (``build``), runs its solve(s) under the options it names (``run``; every
option goes back to the library's default in a ``finally``) and returns a RECORD: per solve ok, iteration, num_applies,
num_pre_applies, path_fallback, absolute_error and initial_error as bits, the residual history and x as uint64 views and the
solver's extra integers; and the deltas of the counters the case watches.  ``counters`` says how the path counters must move
(an int, or "positive"), ``anchor`` is the truth check the case's own feature test applies (with that test's bound; the
pointer stands at every anchor).  The shapes are the smallest at which each path is taken, from the feature tests.

A DISTURBANCE leaves state behind and is not compared.  ``schedule(seed)`` is the pure generator of the seeded orders."""
import ctypes as C
import random

import numpy as np

BIG = 1 << 40  # an amg_tail_rows above every level (tests/test_gpu_amg_tail.py)
BOX = (20, 18, 16)  # tests/test_gpu_cross_product.py: not a cube, the lattice offsets differ per axis

# the library's defaults (csrc/common.hpp) of every option a case or a disturbance sets: what ``finally`` restores
DEFAULTS = {
    "resident_path": 1, "resident_planes": 0, "latency_path": 1, "latency_pre": 0, "generic_solvers": 0, "fused_reduce": 1,
    "amg_tail": 0, "amg_tail_rows": 0, "coop_force_fail": 0, "ticket_verify": 0, "ticket_verify_inject": 0,
    "lazy_statements": 0, "spmv_dict": 4, "ell_cap": 0, "spmv_canon_tile_min_rows": 1 << 20, "cg_march_fill": 2048,
    "cg_residual_fill": 512, "cg_rr_fold": 1, "pool_bytes": 16 << 30,
}
PATH_COUNTERS = ("resident_solves", "latency_solves", "latency_pre_solves", "throughput_solves", "engine_solves", "block_solves",
                 "mixed_solves", "jfnk_inner_solves")
FIELDS = ("ok", "iteration", "num_applies", "num_pre_applies", "path_fallback", "absolute_error", "initial_error", "history", "x",
          "extra")


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


class Options:
    """The options of a dict set on entry and put back to the defaults on exit, in reverse."""

    def __init__(self, ctx, options):
        self.ctx, self.options = ctx, dict(options)

    def __enter__(self):
        for k, v in self.options.items():
            self.ctx.set_option(k, v)

    def __exit__(self, *exc):
        for k in reversed(list(self.options)):
            self.ctx.set_option(k, DEFAULTS[k])
        return False


def other_rhs(b, which):
    """0: the case's right-hand side; 1: another one of its size; "zero"."""
    b = np.asarray(b, np.float64)
    if which == 0:
        return b
    if which == "zero":
        return np.zeros_like(b)
    return 0.5 * b + (0.3 * np.cos(0.11 * np.arange(b.size))).reshape(b.shape)


def _part(ok, s, x, extra=()):
    hist = s.history if isinstance(s.history, list) else [s.history]
    return {"ok": np.asarray(ok), "iteration": np.asarray(s.iterations if hasattr(s, "iterations") else s.iteration, np.int64),
            "num_applies": np.asarray(s.num_applies, np.int64), "num_pre_applies": np.asarray(getattr(s, "num_pre_applies", 0), np.int64),
            "path_fallback": np.asarray(s.path_fallback, np.int64), "absolute_error": bits(s.absolute_error),
            "initial_error": bits(s.initial_error), "history": bits(np.concatenate([np.asarray(h, np.float64) for h in hist])),
            "x": bits(x).ravel(), "extra": np.asarray(extra, np.int64)}


def floats(view):
    return np.asarray(view).view(np.float64)


def differences(got, ref):
    """The fields in which two records differ, as text (empty: the same bits and counts)."""
    out = []
    if len(got["parts"]) != len(ref["parts"]):
        return [f"{len(got['parts'])} solves, not {len(ref['parts'])}"]
    for i, (g, r) in enumerate(zip(got["parts"], ref["parts"])):
        for f in FIELDS:
            if not np.array_equal(g[f], r[f]):
                n = int(np.count_nonzero(g[f] != r[f])) if g[f].shape == r[f].shape else -1
                small = f not in ("history", "x")
                out.append(f"solve {i} {f}: {g[f].tolist() if small else n} != {r[f].tolist() if small else 'fresh (entries)'}")
    if got["counters"] != ref["counters"]:
        out.append(f"counters: {got['counters']} != {ref['counters']}")
    return out


class Case:
    """id, path, the options of build and run, how the counters must move, build / solve / anchor, and (``companion``) the
    options of a second solve in the fresh context that the anchor compares with (the other path of the feature test)."""

    def __init__(self, id, path, options, counters, build, solve, anchor, companion=None, heavy=False):
        self.id, self.path, self.options, self.counters = id, path, options, counters
        self._build, self._solve, self.anchor, self.companion, self.heavy = build, solve, anchor, companion, heavy

    def build(self, ctx):
        from stormruler_amd import api

        with Options(ctx, self.options):
            return self._build(api, ctx)

    def run(self, ctx, built, options=None, **knobs):
        from stormruler_amd import api

        watched = tuple(dict.fromkeys(tuple(self.counters) + PATH_COUNTERS))
        before = {k: ctx.counter(k) for k in watched}
        with Options(ctx, self.options if options is None else options):
            parts = self._solve(api, ctx, built, **knobs)
        return {"parts": parts, "counters": {k: ctx.counter(k) - before[k] for k in watched}}

    def counters_moved(self, record):
        """The catalogue's statement about the path counters, on a record: no comparison can be vacuous."""
        for k, want in self.counters.items():
            got = record["counters"][k]
            assert (got > 0) if want == "positive" else (got == want), (self.id, k, got, want)

    def close(self, built):
        for p in built:
            for obj in p.get("closers", ()):
                obj.close()


# ---- the solve every vector case shares ---------------------------------------------------------------------------------------
def _solve(api, ctx, built, rhs=0, x0=None, num_iterations=None):
    parts = []
    for i, p in enumerate(built):
        with Options(ctx, p.get("options", {})):
            s = p["solver"]()
            s.record_history = True
            if num_iterations is not None:
                s.num_iterations = num_iterations
            pre = p["make_pre"]() if "make_pre" in p else p.get("pre")
            if pre is not None:
                s.pre_op = pre
            b_host = other_rhs(p["b"], rhs)
            b = api.DeviceVector.from_numpy(ctx, b_host)
            x = api.DeviceVector(ctx, b_host.size) if x0 is None else api.DeviceVector.from_numpy(ctx, floats(x0[i]))
            if "before" in p:
                p["before"]()
            try:
                ok = s.solve(x, b, p["op"])
                parts.append(_part(ok, s, x.to_numpy(), tuple(int(getattr(s, k)) for k in p.get("extra", ()))))
            finally:
                for obj in ((pre,) if "make_pre" in p else ()) + (s,):
                    if hasattr(obj, "close"):
                        obj.close()
                if getattr(s, "_engine", None) is not None:
                    s._engine._free()
    return parts


def _solve_block(api, ctx, built, rhs=0, x0=None, num_iterations=None):
    p = built[0]
    s = api.BlockCgSolver()
    s.record_history = True
    s.num_iterations = p["iterations"] if num_iterations is None else num_iterations
    s.absolute_error_tolerance = s.relative_error_tolerance = 0.0  # tests/test_gpu_block.py::_block_solve
    b_host = other_rhs(p["b"], rhs)
    B = api.BlockVector.from_numpy(ctx, b_host)
    X = api.BlockVector(ctx, B.n, B.k) if x0 is None else api.BlockVector.from_numpy(ctx, floats(x0[0]).reshape(b_host.shape))
    ok = s.solve(X, B, p["op"])
    return [_part(ok, s, X.to_numpy())]


# ---- builders -------------------------------------------------------------------------------------------------------------------
def _cross_rhs(g):
    """The right-hand side of tests/test_gpu_cross_product.py::problem."""
    return np.sin(3 * g.center[:, 0]) * np.cos(7 * g.center[:, 1]) * np.cos(2 * g.center[:, 2])


def _resident_rhs(n):
    return 1.0 + 0.25 * np.sin(0.01 * np.arange(n))  # tests/test_gpu_resident.py


def _triangles(name="square_nb.1"):
    from test_gpu_two_stage import _triangle_mesh

    return _triangle_mesh(name)


def _box(kind, **more):
    """CG / BiCGStab / GMRES(10) / IDR(4) of the Poisson operator on the 20 x 18 x 16 box (tests/test_gpu_cross_product.py)."""
    def build(api, ctx):
        from stormruler_amd import mesh

        g = mesh.structured_box(*BOX)
        mat = api.StencilMatrix.from_face_graph(ctx, g)

        def solver():
            s = {"cg": api.CgSolver, "bicgstab": api.BiCgStabSolver, "gmres": api.GmresSolver, "idrs": api.IdrsSolver}[kind]()
            if kind == "gmres":
                s.num_inner_iterations = 10
            return s

        p = dict(solver=solver, op=api.HipStencilOperator(mat, -1.0, 0.0), b=_cross_rhs(g), g=g, kind=kind, closers=[mat])
        if kind == "idrs":  # (the shadow space is fill_randomly's: a solve is a function of the sequence's position)
            p["before"] = api.rng_reset
        return [dict(p, **more)]

    return build


def _build_lat_cg(api, ctx):
    g = _triangles()
    mat = api.StencilMatrix.from_face_graph(ctx, g)
    tri = dict(solver=api.CgSolver, op=api.HipStencilOperator(mat, -1.0e-2, 1.0), b=np.sin(3 * g.center[:, 0]) * np.cos(7 * g.center[:, 1]),
               g=g, kind="cg", coef=(-1.0e-2, 1.0), closers=[mat])  # tests/test_gpu_latency_pcg.py::_step1_operator's operator
    return _box("cg")(api, ctx) + [tri]


def _build_resident(kind):
    def build(api, ctx):
        from stormruler_amd import mesh

        out = []
        for shape, planes in (((12, 86, 5), 0), ((36, 30, 8), 3)):  # tests/test_gpu_resident.py::CASES
            if kind == "cg":
                g = mesh.structured_box(*shape)
                mat, alpha = api.StencilMatrix.from_face_graph(ctx, g), -1.0
            else:  # (cubic cells: at most 32 distinct upwind weights)
                g = mesh.structured_box(*shape, lengths=tuple(n / 64.0 for n in shape))
                wi, wo, de = mesh.convection_diffusion_weights(g, 1e-2, (1.0, 0.5, 0.25))
                mat, alpha = api.StencilMatrix.from_face_weights(ctx, g.n_cells, g.n_halo, g.inner, g.outer, wi, wo, de), 1.0
            out.append(dict(solver=api.CgSolver if kind == "cg" else api.BiCgStabSolver, op=api.HipStencilOperator(mat, alpha, 0.0),
                            b=_resident_rhs(g.n_cells), g=g, kind=kind, options={"resident_planes": planes}, closers=[mat]))
        return out

    return build


def _build_cg_step(api, ctx):
    from stormruler_amd import mesh
    from test_gpu_cg_rr_fold import ONE, _rhs

    g = mesh.structured_box(*ONE, lengths=tuple(s / 128.0 for s in ONE))
    mat = api.StencilMatrix.from_face_graph(ctx, g)

    def solver():
        s = api.CgSolver()
        s.num_iterations = 7
        return s

    return [dict(solver=solver, op=api.HipStencilOperator(mat, -1.0, 0.0), b=_rhs(g.n_cells), closers=[mat])]


def _build_preconditioned(make_pre_name):
    def build(api, ctx):
        import amg_cases
        from test_gpu_amg_tail import fp64_matrix

        a = amg_cases.random_symmetric(3)  # 918 rows: the smallest case whose level 0 the tail takes
        mat = fp64_matrix(ctx, api.StencilMatrix.from_csr, a)
        b = np.random.default_rng(8).standard_normal(a.shape[0])  # tests/test_gpu_amg.py, test_gpu_amg_tail.py
        p = dict(solver=api.CgSolver, op=api.HipStencilOperator(mat, 1.0, 0.0), b=b, a=a, closers=[mat])
        if make_pre_name == "cheb":
            p["make_pre"] = lambda: api.ChebyshevPreconditioner(degree=2, jacobi=True)
        else:  # (the hierarchy is kept from solve to solve: tests/test_gpu_amg.py::test_hierarchy_is_kept_across_solves)
            p["pre"] = api.AmgPreconditioner(coarse_rows=32)
            p["closers"].insert(0, p["pre"])
        return [p]

    return build


def _build_lat_pcg(pre):
    def build(api, ctx):
        from test_gpu_latency_pcg import PRE

        p = _box("cg")(api, ctx)[0]
        p["b"] = _resident_rhs(p["g"].n_cells)  # tests/test_gpu_latency_pcg.py::_box_operator
        p["make_pre"] = lambda: PRE[pre](api)
        return [p]

    return build


def _build_two_stage(api, ctx):
    from stormruler_amd import mesh
    from test_gpu_two_stage import PLAYGROUND

    out = []
    for shape in ((9, 7, 1), (24, 24, 24)):
        g = mesh.structured_box(*shape)
        mat = api.StencilMatrix.from_face_graph(ctx, g)
        out.append(dict(solver=api.CgSolver, op=api.HipTwoStageOperator(mat, *PLAYGROUND), b=_resident_rhs(g.n_cells), g=g, closers=[mat]))
    return out


def _build_mixed(api, ctx):
    import mixed_cg_ref as ref
    from test_gpu_mixed_cg import face_matrix

    case = ref.solve_cases()["square_nb"]  # 6 252 rows: the smallest of tests/test_gpu_mixed_cg.py's converging inputs
    mat = face_matrix(api, ctx, case)
    mat.build_reduced()
    return [dict(solver=api.MixedCgSolver, op=api.HipStencilOperator(mat, -1.0, 0.0), b=ref.rhs(case[0], "ones"), closers=[mat],
                 extra=("outer_steps", "inner_iterations", "fp64_iterations", "finished_fp64"))]


def _build_block(api, ctx):
    import exact_ref as er
    from stormruler_amd import mesh
    from test_gpu_block import SMALL, _fp64

    g = er.unit_box(mesh, *SMALL)
    mat = _fp64(ctx, lambda: api.StencilMatrix.from_face_graph(ctx, g))
    cols = [er.int_vector(g.n_cells, 31 + j) for j in range(3)]
    return [dict(op=api.HipStencilOperator(mat, -1.0, 0.0), b=np.stack([np.asarray(c, np.float64) for c in cols], axis=1), cols=cols,
                 g=g, iterations=2, closers=[mat])]


def _build_jfnk(api, ctx):
    from oracle import oracle
    from stormruler_amd import mesh
    from test_gpu_jfnk_native import BOXES, Cubic

    pb = Cubic(api, mesh, oracle, ctx, BOXES["11x9x7"])
    return [dict(solver=api.DeviceJfnkSolver, op=api.make_operator(pb.device), b=pb.b, pb=pb, closers=[pb], extra=("inner_iterations",))]


def face_update_shape_b():
    """Shape b of tests/test_gpu_face_update.py (13^3, convection-diffusion weights, faces permuted and flipped) and the
    symmetric parts of its two weight sets."""
    from stormruler_amd import mesh
    from test_gpu_face_update import NU, VEL_A, VEL_B, _shuffled

    g = mesh.structured_box(13)
    wa, wb = mesh.convection_diffusion_weights(g, NU, VEL_A), mesh.convection_diffusion_weights(g, NU, VEL_B)
    i, o, (fa, fb) = _shuffled(g.inner, g.outer, [(wa[0], wa[1]), (wb[0], wb[1])])
    s = dict(n=g.n_cells, n_halo=0, inner=i, outer=o, ell_cap=0)
    sym = [(0.5 * (f[0] + f[1]), 0.5 * (f[0] + f[1]), w[2]) for f, w in ((fa, wa), (fb, wb))]
    return s, sym[0], sym[1]


def _build_upd(api, ctx):
    from test_gpu_face_update import _create, _set

    s, sym_a, sym_b = face_update_shape_b()
    mat = _create(api, ctx, s, sym_a, True, True)
    b = np.random.default_rng(40).uniform(0.5, 1.5, s["n"])
    return [dict(solver=api.CgSolver, op=api.HipStencilOperator(mat, 1.0, 0.0), b=b, shape=s, weights=sym_b,
                 before=lambda: _set(api, ctx, mat, sym_b, True), closers=[mat])]


# ---- anchors: the check, with the bound, of the case's own feature test -----------------------------------------------------------
_refs = {}


def _oracle(key, make):
    if key not in _refs:
        _refs[key] = make()
    return _refs[key]


class _Solved:
    """A record's solve as the feature tests' helpers see a solver."""

    def __init__(self, part):
        self.iteration, self.num_applies = int(part["iteration"]), int(part["num_applies"])
        self.num_pre_applies = int(part["num_pre_applies"])
        self.history, self.x, self.ok = floats(part["history"]), floats(part["x"]), bool(part["ok"])
        self.absolute_error, self.initial_error = float(floats(part["absolute_error"])), float(floats(part["initial_error"]))


def _box_ref(kind):
    from oracle import oracle
    from stormruler_amd import mesh

    def make():
        g = mesh.structured_box(*BOX)
        return oracle.solve(kind, oracle.StencilOperator(g, -1.0, 0.0), _cross_rhs(g), num_inner_iterations=10)

    return _oracle(("box", kind), make)


def anchor_cross_product(kind):
    """tests/test_gpu_cross_product.py::_check, against the oracle's solve of the same box."""
    def anchor(record, built, companion=None):
        from test_gpu_cross_product import _check

        s = _Solved(record["parts"][0])
        _check(kind, s.ok, s, s.x, _box_ref(kind), kind)

    anchor.__doc__ = anchor_cross_product.__doc__
    return anchor


def anchor_lat_cg(record, built, companion=None):
    """The box: tests/test_gpu_cross_product.py::_check.  The triangles: the same check (two solves that each stop at
    relative 1e-6) against the oracle's solve of that operator, and num_applies of test_gpu_latency_path.py:52."""
    from oracle import oracle
    from test_gpu_cross_product import _check

    anchor_cross_product("cg")(record, built)
    p, s = built[1], _Solved(record["parts"][1])
    ref = _oracle("triangles", lambda: oracle.solve("cg", oracle.StencilOperator(p["g"], *p["coef"]), p["b"]))
    assert ref.converged and s.num_applies == s.iteration + 1
    _check("cg", s.ok, s, s.x, ref, "square_nb.1")


def anchor_resident(kind):
    """tests/test_gpu_resident.py::test_cg_box_matches_throughput_path_and_oracle (lines 65-74) and
    ::test_bicgstab_box_matches_throughput_path_and_oracle (lines 91-100): the throughput path's solve is the companion."""
    def anchor(record, built, companion):
        from oracle import oracle

        for p, part, other in zip(built, record["parts"], companion["parts"]):
            r, t = _Solved(part), _Solved(other)
            assert r.ok and t.ok
            m = min(len(r.history), len(t.history))
            if kind == "cg":
                ref = oracle.solve("cg", oracle.StencilOperator(p["g"], -1.0, 0.0), p["b"])
                assert abs(r.iteration - t.iteration) <= 1 and r.num_applies == r.iteration + 1
                assert np.allclose(r.history[:m], t.history[:m], rtol=1e-9)
                assert np.linalg.norm(r.x - t.x) <= 1e-9 * np.linalg.norm(t.x)
                assert abs(r.iteration - ref.iterations) <= max(2, int(0.02 * ref.iterations))
                assert np.linalg.norm(r.x - ref.x) <= 1e-8 * np.linalg.norm(ref.x)
            else:
                ref = oracle.solve("bicgstab", oracle.StencilOperator(p["g"], -1e-2, 0.0, conv=1.0, vel=(1.0, 0.5, 0.25)), p["b"])
                assert r.num_applies == 2 * r.iteration + 1
                assert abs(r.iteration - t.iteration) <= max(1, int(0.05 * t.iteration)), (r.iteration, t.iteration)
                m = min(m, 6)
                assert np.allclose(r.history[:m], t.history[:m], rtol=1e-8)
                assert np.linalg.norm(r.x - t.x) <= 1e-6 * np.linalg.norm(t.x)
                assert abs(r.iteration - ref.iterations) <= max(2, int(0.05 * ref.iterations))
                assert np.linalg.norm(r.x - ref.x) <= 1e-6 * np.linalg.norm(ref.x)

    anchor.__doc__ = anchor_resident.__doc__
    return anchor


def anchor_lat_pcg(record, built, companion):
    """tests/test_gpu_latency_pcg.py::test_against_the_engine (lines 240-247): the engine's solve is the companion."""
    l, e = _Solved(record["parts"][0]), _Solved(companion["parts"][0])
    assert companion["counters"]["engine_solves"] == 1 and companion["counters"]["latency_pre_solves"] == 0
    assert l.ok and e.ok and abs(l.iteration - e.iteration) <= 1
    m = min(len(l.history), len(e.history))
    assert np.allclose(l.history[:m], e.history[:m], rtol=1e-9)
    assert np.linalg.norm(l.x - e.x) <= 1e-9 * np.linalg.norm(e.x)
    assert l.num_applies == l.iteration + 1 and l.num_pre_applies == l.iteration + 1


def anchor_cg_step(record, built, companion):
    """tests/test_gpu_cg_rr_fold.py::test_on_and_off_are_bitwise_and_the_counter_moves on its group-of-one lattice: the solve
    with cg_rr_fold = 0 (the companion) has the same bits (::_same), 7 iterations by count (line 113)."""
    assert companion["counters"]["cg_rr_consumer_folds"] == 0
    assert [f for f in FIELDS if not np.array_equal(record["parts"][0][f], companion["parts"][0][f])] == []
    s = _Solved(record["parts"][0])
    assert not s.ok and s.iteration == 7 and s.history.size == 8


def anchor_true_residual(record, built, companion=None):
    """tests/test_gpu_amg.py:332: ||b - A x|| <= 1e-5 ||b|| on the assembled matrix (right-preconditioned CG to 1e-6); with a
    companion (amg_tail = 0) tests/test_gpu_amg_tail.py::same_solve: the launches' bits."""
    p, s = built[0], _Solved(record["parts"][0])
    assert s.ok and s.iteration > 0 and s.num_pre_applies > 0
    assert np.linalg.norm(p["b"] - p["a"] @ s.x) <= 1e-5 * np.linalg.norm(p["b"])
    if companion is not None:
        assert companion["counters"]["amg_tail_applies"] == 0
        for f in ("ok", "iteration", "history", "x"):
            assert np.array_equal(record["parts"][0][f], companion["parts"][0][f]), f


def anchor_two_stage(record, built, companion=None):
    """tests/test_gpu_two_stage.py::test_box_matches_engine_path_and_oracle (lines 184, 189-191)."""
    from oracle import oracle
    from test_gpu_two_stage import PLAYGROUND, _oracle_op

    for p, part in zip(built, record["parts"]):
        s = _Solved(part)
        ref = oracle.solve("cg", _oracle_op(oracle, p["g"], PLAYGROUND), p["b"])
        assert s.ok and s.num_applies == s.iteration + 1
        assert abs(s.iteration - ref.iterations) <= max(2, int(0.02 * ref.iterations)), (s.iteration, ref.iterations)
        assert np.linalg.norm(s.x - ref.x) <= 1e-8 * np.linalg.norm(ref.x)


def anchor_mixed(record, built, companion=None):
    """tests/test_gpu_mixed_cg.py::test_solves_meet_the_rule_without_fallback (lines 260-272) on the solver's own true
    residual norms (history holds the recomputed ||b - A x|| of every outer step, line 267)."""
    import mixed_cg_ref as ref

    part = record["parts"][0]
    s = _Solved(part)
    outer, inner, fp64, finished = (int(v) for v in part["extra"])
    assert s.ok and ref.rule(s.absolute_error, s.initial_error, 1e-6, 1e-6)
    assert s.history.size == outer + 1 and s.history[0] == s.initial_error and s.history[-1] == s.absolute_error
    assert s.iteration == inner and s.num_applies == 1 + inner + outer and np.all(np.diff(s.history) < 0)
    assert finished == 0 and fp64 == 0


def anchor_block(record, built, companion=None):
    """tests/test_gpu_block.py::test_block_cg_two_iterations_against_the_exact_pins (lines 292-296): two iterations per column
    against exact_ref.Pins."""
    import exact_ref as er
    from oracle import oracle
    from test_gpu_block import SMALL

    part, p = record["parts"][0], built[0]
    assert part["iteration"].tolist() == [2, 2, 2]
    hist = floats(part["history"]).reshape(3, 3)
    for j in range(3):
        er.Pins(oracle, p["g"], SMALL, p["cols"][j], "cg").check(list(hist[j]), label=f"column {j}")


def anchor_jfnk(record, built, companion=None):
    """tests/test_gpu_jfnk_native.py::test_whole_solve_against_the_oracle (lines 349-352, 358)."""
    from oracle import oracle

    pb, part = built[0]["pb"], record["parts"][0]
    s, inner_dev = _Solved(part), int(part["extra"][0])
    ref, inner = _oracle("jfnk", lambda: oracle.solve_jfnk(pb.ref_op, pb.b))
    assert s.ok and ref.converged and s.iteration == ref.iterations
    assert abs(inner_dev - inner) <= max(2, int(0.1 * inner))
    assert np.linalg.norm(s.x - ref.x) <= 1e-7 * np.linalg.norm(ref.x)
    assert s.num_applies == 1 + s.iteration * 2 + 2 * inner_dev
    assert record["counters"]["jfnk_inner_solves"] == s.iteration


def anchor_idrs(record, built, companion=None):
    """tests/test_more_solvers.py::test_hip_bicgstabl_idrs_match_oracle (lines 155-159), both generators reset."""
    from oracle import oracle
    from stormruler_amd import mesh

    def make():
        g = mesh.structured_box(*BOX)
        oracle.rng_reset()
        return oracle.solve("idrs", oracle.StencilOperator(g, -1.0, 0.0), _cross_rhs(g), num_inner_iterations=4)

    s, ref = _Solved(record["parts"][0]), _oracle("idrs", make)
    assert s.ok and ref.converged
    assert abs(s.iteration - ref.iterations) <= max(2, int(0.1 * ref.iterations))
    assert np.linalg.norm(s.x - ref.x) <= 1e-5 * np.linalg.norm(ref.x)
    k = min(len(s.history), len(ref.history), 6)
    assert np.allclose(s.history[:k], ref.history[:k], rtol=1e-7)


def companion_upd(api, ctx, built):
    """The same CG on an operator created afresh with the refreshed weights."""
    from test_gpu_face_update import _create

    p = built[0]
    fresh = _create(api, ctx, p["shape"], p["weights"], True, True)
    try:
        return {"parts": _solve(api, ctx, [dict(solver=api.CgSolver, op=api.HipStencilOperator(fresh, 1.0, 0.0), b=p["b"])]), "counters": {}}
    finally:
        fresh.close()


def anchor_upd(record, built, companion):
    """tests/test_gpu_face_update.py::test_solves_on_a_refreshed_operator_are_those_on_a_fresh_one (lines 295-297)."""
    s = _Solved(record["parts"][0])
    assert s.ok
    for f in ("iteration", "x"):
        assert np.array_equal(record["parts"][0][f], companion["parts"][0][f]), f


# ---- the catalogue -----------------------------------------------------------------------------------------------------------------
THROUGHPUT = {"resident_path": 0, "latency_path": 0}
ENGINE = {"generic_solvers": 1}
LATENCY_PRE = {"latency_path": 2, "latency_pre": 1}  # tests/test_gpu_latency_pcg.py::_solve (2: the latency kernel, not the resident one)
CG_STEP = {"latency_path": 0, "spmv_canon_tile_min_rows": 0, "cg_march_fill": 0, "cg_residual_fill": 0}  # tests/test_gpu_cg_rr_fold.py::env
TAIL = dict(ENGINE, amg_tail=1, amg_tail_rows=BIG)

CASES = [
    Case("res_cg", "resident", {}, {"resident_solves": 2}, _build_resident("cg"), _solve, anchor_resident("cg"), companion=THROUGHPUT),
    Case("res_bicg", "resident", {}, {"resident_solves": 2}, _build_resident("bicgstab"), _solve, anchor_resident("bicgstab"),
         companion=THROUGHPUT),
    Case("lat_cg", "latency", {"resident_path": 0}, {"latency_solves": 2}, _build_lat_cg, _solve, anchor_lat_cg),
    Case("lat_pcg_j", "latency_pre", LATENCY_PRE, {"latency_pre_solves": 1, "latency_solves": 1},
         _build_lat_pcg("diag"), _solve, anchor_lat_pcg, companion=dict(LATENCY_PRE, latency_pre=0)),
    Case("lat_pcg_c2", "latency_pre", LATENCY_PRE, {"latency_pre_solves": 1, "latency_solves": 1},
         _build_lat_pcg("cheb2"), _solve, anchor_lat_pcg, companion=dict(LATENCY_PRE, latency_pre=0)),
    Case("thr_cg", "throughput", THROUGHPUT, {"throughput_solves": 1}, _box("cg"), _solve, anchor_cross_product("cg")),
    Case("thr_bicg", "throughput", THROUGHPUT, {"throughput_solves": 1}, _box("bicgstab"), _solve, anchor_cross_product("bicgstab")),
    # (GMRES's own loop, solver_gmres.hip, has no counter -- tests/test_gpu_exact_rccl.py:153 --: its Gram-Schmidt chains move,
    #  and no other path took the solve)
    Case("thr_gmres", "throughput", THROUGHPUT,
         {"mgs_chain_steps": "positive", "resident_solves": 0, "latency_solves": 0, "throughput_solves": 0, "engine_solves": 0},
         _box("gmres"), _solve, anchor_cross_product("gmres")),
    Case("thr_cg_step", "throughput", CG_STEP,
         {"throughput_solves": 1, "cg_fused_steps": "positive", "cg_residual_plane_marches": "positive",
          "cg_pz_consumer_folds": "positive", "cg_rr_consumer_folds": 1},
         _build_cg_step, _solve, anchor_cg_step, companion=dict(CG_STEP, cg_rr_fold=0), heavy=True),
    Case("eng_cg", "engine", ENGINE, {"engine_solves": 1}, _box("cg"), _solve, anchor_cross_product("cg")),
    Case("eng_bicg", "engine", ENGINE, {"engine_solves": 1}, _box("bicgstab"), _solve, anchor_cross_product("bicgstab")),
    Case("eng_gmres", "engine", ENGINE, {"engine_solves": 1}, _box("gmres"), _solve, anchor_cross_product("gmres")),
    Case("eng_idrs", "engine", ENGINE, {"engine_solves": 1}, _box("idrs"), _solve, anchor_idrs),
    Case("eng_gmres_2l", "engine", dict(ENGINE, fused_reduce=0), {"engine_solves": 1}, _box("gmres"), _solve, anchor_cross_product("gmres")),
    Case("eng_cheb", "engine", ENGINE, {"engine_solves": 1, "cheb_fused_applies": "positive"}, _build_preconditioned("cheb"), _solve,
         anchor_true_residual),
    Case("eng_amg", "engine", ENGINE, {"engine_solves": 1, "amg_applies": "positive", "amg_tail_applies": 0},
         _build_preconditioned("amg"), _solve, anchor_true_residual),
    Case("eng_amg_tail", "engine", TAIL, {"engine_solves": 1, "amg_tail_applies": "positive", "amg_tail_refusals": 0},
         _build_preconditioned("amg"), _solve, anchor_true_residual, companion=dict(TAIL, amg_tail=0)),
    Case("two_stage", "latency", {}, {"latency_solves": 2, "engine_solves": 0}, _build_two_stage, _solve, anchor_two_stage),
    Case("mixed", "mixed", {}, {"mixed_solves": 1}, _build_mixed, _solve, anchor_mixed),
    Case("block3", "block", {}, {"block_solves": 1}, _build_block, _solve_block, anchor_block),
    Case("jfnk", "jfnk", {}, {"jfnk_inner_solves": "positive"}, _build_jfnk, _solve, anchor_jfnk),
    Case("upd", "updatable", {}, {"op_face_updates": 1}, _build_upd, _solve, anchor_upd, companion=companion_upd),
]
BY_ID = {c.id: c for c in CASES}
LIGHT = [c.id for c in CASES if not c.heavy]
STEP_BEFORE = ("thr_cg", "res_cg", "eng_gmres_2l")  # thr_cg_step precedes these only (4 M rows: time)


class Session:
    """One context and what was built on it: every case's objects once, closed with the session."""

    def __init__(self, ctx=None):
        from stormruler_amd import api

        self.api, self.ctx, self.built = api, ctx if ctx is not None else api.Context(0), {}

    def objects(self, case_id):
        if case_id not in self.built:
            self.built[case_id] = BY_ID[case_id].build(self.ctx)
        return self.built[case_id]

    def run(self, case_id, **knobs):
        return BY_ID[case_id].run(self.ctx, self.objects(case_id), **knobs)

    def close(self):
        for case_id, built in self.built.items():
            BY_ID[case_id].close(built)
        self.built.clear()
        self.ctx.close()


# ---- disturbances ------------------------------------------------------------------------------------------------------------------
VERIFY_BOX = BOX  # the smallest box with more than one block of partials on which the injected loss is caught


def _cut(k):
    return lambda ses, case_id: ses.run(case_id, rhs=1, num_iterations=k)


def _from_solution(ses, case_id):
    first = ses.run(case_id)
    ses.run(case_id, x0=[p["x"] for p in first["parts"]])


def _forced(how):
    def run(ses, case_id):
        built = ses.objects(case_id)
        with Options(ses.ctx, {"coop_force_fail": how}):  # (the hook: no back-off is set, nothing waits)
            BY_ID[case_id].run(ses.ctx, built)

    return run


def _abort_callback(ses, case_id=None):
    """tests/test_gpu_jfnk_native.py::test_a_failing_callback_aborts_and_the_context_stays_usable: the third call returns 7.  The
    Newton method as there, and GMRES with its sums on the two-launch road (a reduction is pending when the call fails)."""
    from stormruler_amd import mesh

    api, ctx = ses.api, ses.ctx
    lib, _lib = api.lib, api._lib
    g = mesh.structured_box(11, 9, 7)
    mat = api.StencilMatrix.from_face_graph(ctx, g)
    try:
        for method, options in ((10, {}), (2, {"fused_reduce": 0})):
            calls = []

            def failing(_user, y_handle, x_handle):
                try:
                    calls.append(1)
                    if len(calls) == 3:
                        return 7
                    mat.apply(-1.0e-2, 1.0, api.DeviceVector._borrow(ctx, x_handle), api.DeviceVector._borrow(ctx, y_handle))
                    return 0
                except BaseException:  # never unwind through the C frames
                    return 1

            cb = _lib.APPLY_FN(failing)
            h = C.c_void_p()
            api.check(lib.storm_hip_krylov_create(ctx._h, method, C.byref(h)))
            try:
                with Options(ctx, options):
                    api.check(lib.storm_hip_krylov_set_operator_fn(h, cb, None))
                    p, r = _lib.SolverParams(), _lib.SolverResult()
                    lib.storm_hip_solver_params_default(C.byref(p))
                    b, x = api.DeviceVector.from_numpy(ctx, np.ones(g.n_cells)), api.DeviceVector(ctx, g.n_cells)
                    status = lib.storm_hip_krylov_solve(h, b._h, x._h, C.byref(p), C.byref(r), None, None)
                    assert status == -1 and b"returned 7" in lib.storm_hip_last_error() and len(calls) == 3, (method, status, len(calls))
            finally:
                lib.storm_hip_krylov_destroy(h)
    finally:
        mat.close()


def _verify_trip(ses, case_id=None):
    """tests/test_gpu_under_load.py::test_ticket_verify_passes_and_catches_a_lost_partial on a small box: a fused CG and a fused
    BiCGStab solve whose recomputed sums lose a partial both return the error; SolverState::verify_failed was set."""
    from stormruler_amd import mesh

    api, ctx = ses.api, ses.ctx
    g = mesh.structured_box(*VERIFY_BOX)
    mat = api.StencilMatrix.from_face_graph(ctx, g)
    try:
        with Options(ctx, dict(THROUGHPUT, ticket_verify=1, ticket_verify_inject=1)):
            for cls in (api.CgSolver, api.BiCgStabSolver):
                b, x = api.DeviceVector.from_numpy(ctx, np.ones(g.n_cells)), api.DeviceVector(ctx, g.n_cells)
                s = cls()
                try:
                    s.solve(x, b, api.HipStencilOperator(mat, -1.0, 0.0))
                except api._lib.StormHipError as e:
                    assert "ticket_verify" in str(e), str(e)
                else:
                    raise AssertionError(f"{cls.__name__}: the injected loss was not caught")
                finally:
                    if s._engine is not None:
                        s._engine._free()
    finally:
        mat.close()


def _other_sizes(ses, case_id=None):
    from stormruler_amd import mesh

    api, ctx = ses.api, ses.ctx
    for shape in ((5, 4, 3), (40, 30, 17)):  # arena and pool classes on either side of the cases', workspace growth
        g = mesh.structured_box(*shape)
        mat = api.StencilMatrix.from_face_graph(ctx, g)
        vs = [api.DeviceVector.from_numpy(ctx, np.full(g.n_cells, 1.0 + j)) for j in range(5)]
        x = api.DeviceVector(ctx, g.n_cells)
        s = api.CgSolver()
        assert s.solve(x, vs[0], api.HipStencilOperator(mat, -1.0, 0.0))
        s._engine._free()
        del vs, x
        mat.close()


def _pool_trim(ses, case_id=None):
    ses.ctx.set_option("pool_bytes", 0)
    ses.ctx.set_option("pool_bytes", DEFAULTS["pool_bytes"])


def _lazy_burst(ses, case_id=None):
    api, ctx = ses.api, ses.ctx
    n = BOX[0] * BOX[1] * BOX[2]
    x, p, r = (api.DeviceVector.from_numpy(ctx, np.sin(0.1 * (j + 1) * np.arange(n))) for j in range(3))
    fused = ctx.counter("lazy_fused_dots")
    with Options(ctx, {"lazy_statements": 1}):
        x += 0.3 * p
        r -= 0.3 * x
        rr = api.dot_product(r, r)  # rides with the pair above (tests/test_gpu_lazy.py::_lin_steps)
        p <<= r + 0.7 * p           # held back until the option goes to 0
    assert np.isfinite(rr) and ctx.counter("lazy_fused_dots") == fused + 1


def _many_short(ses, case_id=None):
    """40 one-iteration solves of alternating kinds and roads: ring generations, tag parities, engines destroyed and created."""
    api, ctx = ses.api, ses.ctx
    p = ses.objects("thr_cg")[0]
    b = api.DeviceVector.from_numpy(ctx, other_rhs(p["b"], 1))
    kinds = (api.CgSolver, api.BiCgStabSolver, api.GmresSolver)
    roads = ({}, ENGINE, THROUGHPUT, {"resident_path": 0})
    for i in range(40):
        s = kinds[i % 3]()
        s.num_iterations = 1
        x = api.DeviceVector(ctx, p["b"].size)
        with Options(ctx, roads[i % 4]):
            s.solve(x, b, p["op"])
        assert s.iteration == 1
        s._engine._free()


def _refresh_other(ses, case_id=None):
    """set_face_weights on an unrelated updatable operator that has a reduced companion (tests/test_gpu_mixed_cg.py section 7)."""
    import mixed_cg_ref as ref
    from test_gpu_mixed_cg import face_matrix

    api, ctx = ses.api, ses.ctx
    i, o = ref.box_faces(5, 4, 3)
    w0, de0 = ref.jittered_case(60, i, o, seed=51)
    w1, de1 = ref.jittered_case(60, i, o, seed=52, shift=0.2)
    mat = face_matrix(api, ctx, (60, i, o, w0, de0), updatable=True)
    try:
        mat.build_reduced()
        before = ctx.counter("op_face_updates")
        wv, dv = api.DeviceVector.from_numpy(ctx, w1), api.DeviceVector.from_numpy(ctx, de1)
        mat.set_face_weights(wv, wv, dv)
        assert ctx.counter("op_face_updates") == before + 1
    finally:
        mat.close()


# id -> (takes a case, function of (session, case id))
DISTURBANCES = {
    "cut1": (True, _cut(1)), "cut2": (True, _cut(2)), "cut3": (True, _cut(3)),
    "zero_rhs": (True, lambda ses, case_id: ses.run(case_id, rhs="zero")),
    "from_solution": (True, _from_solution), "coop_refused": (True, _forced(1)), "coop_gave_up": (True, _forced(2)),
    "abort_callback": (False, _abort_callback), "verify_trip": (False, _verify_trip), "other_sizes": (False, _other_sizes),
    "pool_trim": (False, _pool_trim), "lazy_burst": (False, _lazy_burst), "many_short": (False, _many_short),
    "refresh_other": (False, _refresh_other),
}


def disturb(ses, name, case_id=None):
    DISTURBANCES[name][1](ses, case_id)


# ---- orders: entries ("check", case) compared with the fresh record, ("use", case) run only, ("dist", name, case or None) --------
def others_of(b_id):
    """Every other case in front of B; thr_cg_step only in front of STEP_BEFORE."""
    return [c.id for c in CASES if c.id != b_id and (not c.heavy or b_id in STEP_BEFORE)]


def after_every_other_path(b_id):
    out = []
    for a in others_of(b_id):
        out += [("use", a), ("check", b_id)]
    return out


def disturbances_of(b_id):
    """Every disturbance that takes a case on B's own path and on two other paths (the next two light cases of the catalogue
    on another path), every other disturbance once."""
    i = LIGHT.index(b_id) if b_id in LIGHT else 0
    ring = LIGHT[i + 1:] + LIGHT[:i]
    two = []
    for c in ring:
        if BY_ID[c].path != BY_ID[b_id].path and BY_ID[c].path not in [BY_ID[t].path for t in two]:
            two.append(c)
        if len(two) == 2:
            break
    out = []
    for name, (takes_case, _) in DISTURBANCES.items():
        out += [(name, c) for c in [b_id] + two] if takes_case else [(name, None)]
    return out


def after_every_disturbance(b_id):
    out = []
    for name, c in disturbances_of(b_id):
        out += [("dist", name, c), ("check", b_id)]
    if b_id == "thr_gmres":  # a give-up on the resident path, then every path that shares its buffers, in turn
        out += [("dist", "coop_gave_up", "res_cg"), ("check", "res_bicg"), ("check", "lat_cg"), ("check", "thr_gmres")]
    return out


SEEDS = (0, 1, 2)
SCHEDULE_LENGTH = 60


def schedule(seed, length=SCHEDULE_LENGTH):
    """A pure function of the seed: every case once as a compared entry and every disturbance once, filled up to ``length`` with
    draws of two cases to one disturbance, shuffled.  A disturbance that takes a case draws a light one."""
    rng = random.Random(seed)
    entries = [("check", c.id) for c in CASES]
    entries += [("dist", name, rng.choice(LIGHT) if takes else None) for name, (takes, _) in DISTURBANCES.items()]
    names = list(DISTURBANCES)
    while len(entries) < length:
        if rng.randrange(3) < 2:
            entries.append(("check", rng.choice(LIGHT)))
        else:
            name = rng.choice(names)
            entries.append(("dist", name, rng.choice(LIGHT) if DISTURBANCES[name][0] else None))
    rng.shuffle(entries)
    return entries


# two live contexts take turns: four cases each
TWO_CONTEXTS = (("res_cg", "thr_gmres", "eng_amg_tail", "lat_pcg_j"), ("lat_cg", "res_bicg", "eng_gmres_2l", "two_stage"))
