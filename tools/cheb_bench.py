#!/usr/bin/env python3
"""What the Chebyshev preconditioner's fused step kernel buys, and what the preconditioner buys a solve (one MI355X).

    python tools/cheb_bench.py [--n 256] [--tet-edge 128] [--repeats 30] [--skip-solves] [--out profiles/NAME.json]
    python tools/cheb_bench.py --reduced [--n 256] [--repeats 30] [--skip-solves] [--out profiles/NAME.json]

(a) Microseconds per storm_hip_cheb_apply, fused step (option cheb_fused = 1) against the statement path (= 0: library
    statements only), degrees 2, 4 and 8, with and without the Jacobi scale, on the n^3 box with fp64 records (option
    spmv_dict = 0) and on the 6 * tet_edge^3-cell tetrahedral box of tools/block_bench.py.  One HIP-event pair per apply on
    the library's compute stream, the two arms ALTERNATING apply by apply, two (r, z) pairs in rotation, the median of
    `repeats` applies per arm after a warm-up of both.  The two arms' z are compared to the bit at the timed size.
    Bytes per row and step by the algorithm: fused records + 48 (+ 8 with the scale), statements records + 88 (+ 24).
(b) CG to the default tolerance (1e-6) on the same box (right-hand side 1): plain against Chebyshev of degrees 2 and 4,
    and CG on the Triangle mesh `step.1` with the Jacobi scale: iterations, operator products (applies + degree x
    preconditioner applies), wall time of a solve between two context synchronisations (the median of three, after one).
(c) --reduced: the third arm.  The n^3 box as a face-weight operator on fp64 records, the fused step of an ordinary object
    against that of a REDUCED object (the operator's fp32-weight companion records, csrc/op_reduced.hip), same method as
    (a); z of the reduced object is compared, at the timed size, with z of an ordinary object on the operator rebuilt from
    the weights rounded to fp32.  Bytes per row and step: reduced records + 48 (+ 8).  Then CG to 1e-6 as plain / degree 2 /
    degree 2 reduced, the preconditioner's build (for the reduced arm: the companion's as well) inside the timed solve.
    The fused arm of ANOTHER build of the library (the parent commit's) comes from running that build's own copy of this
    tool in the same session; this tool only measures the library it imports.
Prints and writes one JSON document.  Not a pass / fail: tests/test_gpu_cheb.py and tests/test_gpu_reduced.py hold the results."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def apply_times(api, ctx, mat, alpha, beta, repeats, warmup=4):
    st = mat.stats()
    n = st["n_rows"]
    rec = st["record_bytes"] / n
    out = {"rows": n, "record_bytes_per_row": rec, "tail_rows": st["tail_rows"], "cases": []}
    op = api.HipStencilOperator(mat, alpha, beta)
    rs = [api.DeviceVector.from_numpy(ctx, np.sin(0.37 * (j + 1) * np.arange(n)) + 0.25) for j in range(2)]
    zs = [api.DeviceVector(ctx, n) for _ in range(2)]
    for jacobi in (False, True):
        for degree in (2, 4, 8):
            pre = api.ChebyshevPreconditioner(degree=degree, jacobi=jacobi)
            pre.build(zs[0], rs[0], op)
            ms = {1: [], 0: []}
            before = (ctx.counter("cheb_fused_applies"), ctx.counter("cheb_statement_applies"))
            for i in range(warmup + repeats):
                for fused in ((1, 0) if i % 2 == 0 else (0, 1)):  # alternating, and alternating who goes first
                    ctx.set_option("cheb_fused", fused)
                    ctx.timer_start()
                    pre.mul(zs[i % 2], rs[i % 2])
                    t = ctx.timer_stop()
                    if i >= warmup:
                        ms[fused].append(t)
            counts = (ctx.counter("cheb_fused_applies") - before[0], ctx.counter("cheb_statement_applies") - before[1])
            assert counts == (warmup + repeats, warmup + repeats), counts
            ctx.set_option("cheb_fused", 1)
            pre.mul(zs[0], rs[0])
            ctx.set_option("cheb_fused", 0)
            pre.mul(zs[1], rs[0])
            ctx.set_option("cheb_fused", 1)
            same = bool(np.array_equal(zs[0].to_numpy(), zs[1].to_numpy()))
            f, s = np.array(ms[1]), np.array(ms[0])
            fused_b, stmt_b = rec + 48 + (8 if jacobi else 0), rec + 88 + (24 if jacobi else 0)
            out["cases"].append({
                "degree": degree, "jacobi": jacobi, "applies_per_arm": repeats,
                "fused_us_median": 1e3 * float(np.median(f)), "fused_us_min": 1e3 * float(f.min()), "fused_us_max": 1e3 * float(f.max()),
                "statements_us_median": 1e3 * float(np.median(s)), "statements_us_min": 1e3 * float(s.min()),
                "statements_us_max": 1e3 * float(s.max()),
                "speedup_fused_over_statements": float(np.median(s) / np.median(f)),
                "bytes_per_row_step_fused": fused_b, "bytes_per_row_step_statements": stmt_b,
                "model_speedup_by_bytes": stmt_b / fused_b,
                "fused_GBs": (degree * fused_b + 16 + (8 if jacobi else 0)) * n / (float(np.median(f)) * 1e-3) / 1e9,
                "bitwise_equal": same})
            print(json.dumps(out["cases"][-1]), flush=True)
            pre.close()
    return out


def reduced_times(api, ctx, mat, ref, alpha, beta, repeats, warmup=4):
    """Fused step: an ordinary object against a reduced one on `mat`; z against an ordinary object on `ref` (rounded weights)."""
    st = mat.stats()
    n = st["n_rows"]
    mat.build_reduced()
    rec, rec32 = st["record_bytes"] / n, mat.reduced_bytes / n
    out = {"rows": n, "record_bytes_per_row": rec, "reduced_record_bytes_per_row": rec32, "cases": []}
    op, ref_op = api.HipStencilOperator(mat, alpha, beta), api.HipStencilOperator(ref, alpha, beta)
    rs = [api.DeviceVector.from_numpy(ctx, np.sin(0.37 * (j + 1) * np.arange(n)) + 0.25) for j in range(2)]
    zs = [api.DeviceVector(ctx, n) for _ in range(2)]
    for jacobi in (False, True):
        for degree in (2, 4, 8):
            pres = {False: api.ChebyshevPreconditioner(degree=degree, jacobi=jacobi),
                    True: api.ChebyshevPreconditioner(degree=degree, jacobi=jacobi, reduced_records=True)}
            for pre in pres.values():
                pre.build(zs[0], rs[0], op)
            ms = {True: [], False: []}
            before = (ctx.counter("cheb_fused_applies"), ctx.counter("cheb_reduced_applies"))
            for i in range(warmup + repeats):
                for red in ((True, False) if i % 2 == 0 else (False, True)):  # alternating, and alternating who goes first
                    ctx.timer_start()
                    pres[red].mul(zs[i % 2], rs[i % 2])
                    t = ctx.timer_stop()
                    if i >= warmup:
                        ms[red].append(t)
            counts = (ctx.counter("cheb_fused_applies") - before[0], ctx.counter("cheb_reduced_applies") - before[1])
            assert counts == (2 * (warmup + repeats), warmup + repeats), counts
            # the contract at the timed size: the reduced z against an ordinary object on the rounded operator (the SAME
            # scale: the reduced object's own, taken from the fp64 diagonal of `mat`)
            if jacobi:
                on_ref = _cheb_with_scale(api, ref, alpha, beta, pres[True]._dinv, degree)
            else:
                on_ref = api.ChebyshevPreconditioner(degree=degree)
                on_ref.build(zs[0], rs[0], ref_op)
            pres[True].mul(zs[0], rs[0])
            on_ref.mul(zs[1], rs[0])
            same = bool(np.array_equal(zs[0].to_numpy().view(np.uint64), zs[1].to_numpy().view(np.uint64)))
            f, r = np.array(ms[False]), np.array(ms[True])
            f_b, r_b = rec + 48 + (8 if jacobi else 0), rec32 + 48 + (8 if jacobi else 0)
            out["cases"].append({
                "degree": degree, "jacobi": jacobi, "applies_per_arm": repeats,
                "fp64_us_median": 1e3 * float(np.median(f)), "fp64_us_min": 1e3 * float(f.min()), "fp64_us_max": 1e3 * float(f.max()),
                "reduced_us_median": 1e3 * float(np.median(r)), "reduced_us_min": 1e3 * float(r.min()),
                "reduced_us_max": 1e3 * float(r.max()),
                "speedup_reduced_over_fp64": float(np.median(f) / np.median(r)),
                "bytes_per_row_step_fp64": f_b, "bytes_per_row_step_reduced": r_b, "ceiling_by_bytes": f_b / r_b,
                "reduced_GBs": (degree * r_b + 16 + (8 if jacobi else 0)) * n / (float(np.median(r)) * 1e-3) / 1e9,
                "bitwise_equal_to_ordinary_on_rounded_operator": same})
            print(json.dumps(out["cases"][-1]), flush=True)
            for pre in list(pres.values()) + [on_ref]:
                pre.close()
    return out


class _cheb_with_scale:
    """storm_hip_cheb_create with an explicit scale (the Python class derives its own from the operator it is built on)."""

    def __init__(self, api, mat, alpha, beta, dinv, degree):
        import ctypes as C

        from stormruler_amd import _lib

        self._lib, self._h = _lib, C.c_void_p()
        _lib.check(_lib.lib.storm_hip_cheb_create(mat._h, alpha, beta, dinv._h, degree, 0.0, 0.0, C.byref(self._h)))

    def mul(self, y, x):
        self._lib.check(self._lib.lib.storm_hip_cheb_apply(self._h, x._h, y._h))

    def close(self):
        if self._h:
            self._lib.lib.storm_hip_cheb_destroy(self._h)
            self._h = None


def solve_times(api, ctx, mat, alpha, beta, arms, repeats=3):
    n = mat.stats()["n_rows"]
    op = api.HipStencilOperator(mat, alpha, beta)
    b, x = api.DeviceVector.from_numpy(ctx, np.ones(n)), api.DeviceVector(ctx, n)
    rows = []
    for name, pre in arms:
        s = api.CgSolver()
        s.pre_op = pre
        times = []
        for i in range(repeats + 1):
            api.fill_with(x, 0.0)
            if getattr(pre, "reduced_records", False):
                mat.drop_reduced()  # (the companion's build is part of the timed solve)
            ctx.sync()
            t0 = time.perf_counter()
            ok = s.solve(x, b, op)
            ctx.sync()
            if i > 0:
                times.append(time.perf_counter() - t0)
        degree = getattr(pre, "degree", 0)  # (operator products per preconditioner apply)
        rows.append({"arm": name, "converged": bool(ok), "iterations": int(s.iteration),
                     "operator_products": int(s.num_applies + degree * s.num_pre_applies), "pre_applies": int(s.num_pre_applies),
                     "wall_ms_median": 1e3 * float(np.median(times)), "wall_ms_min": 1e3 * float(min(times)),
                     "wall_ms_max": 1e3 * float(max(times)), "relative_error": float(s.relative_error)})
        print(json.dumps(rows[-1]), flush=True)
        if pre is not None:
            pre.close()
    return {"rows": n, "solves": rows}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--tet-edge", type=int, default=128, help="cubes per edge of the tetrahedral box (0: skip it)")
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--skip-solves", action="store_true")
    ap.add_argument("--reduced", action="store_true", help="the reduced-records arm (c) instead of (a), (b)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from stormruler_amd import api, host_mesh, io_tetgen, mesh

    ctx = api.Context(0)
    doc = {"device": ctx.info()["name"],
           "method": "apply: HIP-event pair per apply, arms alternating, median; solve: host clock between context syncs, median of 3"}

    def save():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(doc, f, indent=1)

    if args.reduced:
        g = mesh.structured_box(args.n)
        coef, b_coef = mesh.face_coefficients(g)
        ext = np.zeros(g.n_total)
        np.add.at(ext, g.b_cell, -b_coef / g.volume[g.b_cell])
        w = (coef / g.volume[g.inner], coef / g.volume[g.outer], ext[: g.n_cells])
        w32 = tuple(a.astype(np.float32).astype(np.float64) for a in w)
        ctx.set_option("spmv_dict", 0)
        mat = api.StencilMatrix.from_face_weights(ctx, g.n_cells, 0, g.inner, g.outer, *w)
        ref = api.StencilMatrix.from_face_weights(ctx, g.n_cells, 0, g.inner, g.outer, *w32)
        ctx.set_option("spmv_dict", 4)
        doc["box"] = {"n": args.n, "operator": "A = -M, M the box's diffusion stencil from face weights, fp64 records",
                      "weights_changed_by_fp32_rounding": float(np.mean(np.concatenate(w) != np.concatenate(w32))),
                      "apply": reduced_times(api, ctx, mat, ref, -1.0, 0.0, args.repeats)}
        ref.close()
        save()
        if not args.skip_solves:
            doc["box"]["cg"] = solve_times(api, ctx, mat, -1.0, 0.0,
                                           [("plain", None), ("chebyshev degree 2", api.ChebyshevPreconditioner(degree=2)),
                                            ("chebyshev degree 2, reduced records",
                                             api.ChebyshevPreconditioner(degree=2, reduced_records=True))])
            save()
        mat.close()
        print(json.dumps(doc), flush=True)
        ctx.close()
        return 0

    ctx.set_option("spmv_dict", 0)
    mat = api.StencilMatrix.from_face_graph(ctx, mesh.structured_box(args.n))
    ctx.set_option("spmv_dict", 4)
    doc["box"] = {"n": args.n, "apply": apply_times(api, ctx, mat, -1.0, 0.0, args.repeats)}
    save()
    if not args.skip_solves:
        doc["box"]["cg"] = solve_times(api, ctx, mat, -1.0, 0.0,
                                       [("plain", None), ("chebyshev degree 2", api.ChebyshevPreconditioner(degree=2)),
                                        ("chebyshev degree 4", api.ChebyshevPreconditioner(degree=4))])
        save()
    mat.close()

    if not args.skip_solves:
        g = io_tetgen.read_triangle(os.path.join(ROOT, "tests", "golden", "mesh", "step.1."))
        ctx.set_option("spmv_dict", 0)
        mat = api.StencilMatrix.from_face_graph(ctx, g)
        ctx.set_option("spmv_dict", 4)
        ctx.set_option("latency_path", 0)  # (the plain arm through the same kind of loop as the preconditioned ones)
        doc["step.1"] = {"operator": "A = I - 1e-2 L", "cg": solve_times(
            api, ctx, mat, -1e-2, 1.0,
            [("plain", None), ("jacobi", api.JacobiPreconditioner()),
             ("chebyshev degree 2, jacobi", api.ChebyshevPreconditioner(degree=2, jacobi=True)),
             ("chebyshev degree 4, jacobi", api.ChebyshevPreconditioner(degree=4, jacobi=True))])}
        ctx.set_option("latency_path", 1)
        mat.close()
        save()

    if args.tet_edge > 0:
        with tempfile.TemporaryDirectory() as d:
            pos, bf, cells = io_tetgen.tet_box(args.tet_edge)
            prefix = os.path.join(d, "tetbox.1")
            host_mesh.write_tetgen(prefix, pos, bf, np.ones(len(bf), np.int64), cells)
            del pos, bf, cells
            hm = host_mesh.HostMesh.read_tetgen(prefix + ".", 3)
        assert hm.order_cells("morton") == "morton"
        mat = hm.create_operator(ctx)
        assert mat.stats()["paired_rows"] == 0 and mat.stats()["value_dictionary_size"] == 0
        doc["tetrahedra"] = {"edge": args.tet_edge, "apply": apply_times(api, ctx, mat, -1.0, 0.0, args.repeats)}
        mat.close()
        save()
    print(json.dumps(doc), flush=True)
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
