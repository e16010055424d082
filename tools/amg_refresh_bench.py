#!/usr/bin/env python3
"""What refreshing a multigrid hierarchy on the device costs and buys, on one MI355X.

    python tools/amg_refresh_bench.py [--n 256] [--degree 1] [--fp64-smoothers] [--repeats 5] [--out profiles/NAME.json]
    python tools/amg_refresh_bench.py --rebuild-only [--package-root DIR] ...   # the road of a build without refresh()

The n^3 face-weight box of tools/amg_bench.py as an UPDATABLE operator (fp64 records), A = -M, right-hand side 1, CG to
1e-6.  Two weight sets alternate: A, the box's own weights, and B, the same times exp(0.5 N(0, 1)) per face (seed 12).
The refreshable object is set up once at A.  Measured, wall clock between two context synchronisations:
  * ms per refresh() after set_face_weights, weights alternating B, A, B, ...: the median of `repeats` after one warm-up;
  * "refresh_bytes" and "device_bytes";
  * CG on B with the refreshed object: iterations and ms (median of 3);
  * the same CG with a fresh AmgPreconditioner built on B (its setup and upload seconds are this build's rebuild);
  * the same CG with Chebyshev degree 2 on reduced records, the best arm that needs no setup;
  * the stale object (set up at A, solving B), iterations only.
--rebuild-only uses nothing a build without storm_hip_amg_refresh lacks: the object is set up at A, the weights become B,
and close() + build() is timed once, then the CG on B and the Chebyshev arm.  --package-root names the tree whose
stormruler_amd package (and library) is imported: a checkout of the parent commit, built.
The bar: refresh + refreshed solve below the Chebyshev arm's solve; refresh below a tenth of the rebuild.
Prints and writes one JSON document.  Not a pass / fail: tests/test_gpu_amg_refresh.py holds the results."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def timed(ctx, fn):
    ctx.sync()
    t0 = time.perf_counter()
    out = fn()
    ctx.sync()
    return time.perf_counter() - t0, out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--degree", type=int, default=1)
    ap.add_argument("--fp64-smoothers", action="store_true", help="smoothers on the fp64 records (default: reduced records)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rebuild-only", action="store_true")
    ap.add_argument("--package-root", default=ROOT)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))

    from stormruler_amd import api, mesh

    ctx = api.Context(0)
    g = mesh.structured_box(args.n)
    coef, b_coef = mesh.face_coefficients(g)
    ext = np.zeros(g.n_total)
    np.add.at(ext, g.b_cell, -b_coef / g.volume[g.b_cell])
    ext = ext[: g.n_cells]
    w_a = coef / g.volume[g.inner]  # (a box: every cell has the same volume, both sides carry the same weight)
    w_b = w_a * np.exp(0.5 * np.random.default_rng(12).standard_normal(w_a.size))
    n = g.n_cells
    mat = api.StencilMatrix.from_face_weights_updatable(ctx, n, 0, g.inner, g.outer, w_a, w_a, ext)
    del g, coef, b_coef
    sets = {"A": api.DeviceVector.from_numpy(ctx, w_a), "B": api.DeviceVector.from_numpy(ctx, w_b)}
    de = api.DeviceVector.from_numpy(ctx, ext)
    op = api.HipStencilOperator(mat, -1.0, 0.0)
    b, x = api.DeviceVector.from_numpy(ctx, np.ones(n)), api.DeviceVector(ctx, n)
    reduced = not args.fp64_smoothers
    doc = {"device": ctx.info()["name"], "n": args.n, "rows": n, "smoother_degree": args.degree, "reduced_records": reduced,
           "package_root": os.path.relpath(os.path.abspath(args.package_root), ROOT), "rebuild_only": bool(args.rebuild_only),
           "method": "host clock between context syncs; refresh: median after one warm-up, weights alternating; solves: median of 3"}

    def weights(name):
        mat.set_face_weights(sets[name], sets[name], de)

    def solve(pre):
        ts, s = [], None
        for _ in range(4):
            s = api.CgSolver()
            s.pre_op = pre
            api.fill_with(x, 0.0)
            dt, ok = timed(ctx, lambda: s.solve(x, b, op))
            ts.append(dt)
        return {"converged": bool(ok), "iterations": int(s.iteration), "ms_median": 1e3 * float(np.median(ts[1:])),
                "ms_min": 1e3 * float(min(ts[1:])), "ms_max": 1e3 * float(max(ts[1:]))}

    params = dict(smoother_degree=args.degree, reduced_records=reduced)
    if args.rebuild_only:
        pre = api.AmgPreconditioner(**params)
        dt, _ = timed(ctx, lambda: pre.build(x, b, op))
        doc["first_build_seconds"] = dt
        weights("B")

        def rebuild():
            pre.close()
            pre.build(x, b, op)

        dt, _ = timed(ctx, rebuild)
        doc["rebuild"] = {"close_and_build_seconds": dt, "host_setup_seconds": pre.get("setup_seconds"),
                          "upload_seconds": pre.get("upload_seconds"), "device_bytes": int(pre.get("device_bytes")),
                          "level_rows": pre.hierarchy.level_rows()}
        doc["cg_rebuilt"] = solve(pre)
        pre.close()
    else:
        pre = api.AmgPreconditioner(refreshable=True, **params)
        dt, _ = timed(ctx, lambda: pre.build(x, b, op))
        doc["refreshable_build"] = {"seconds": dt, "host_setup_seconds": pre.get("setup_seconds"), "upload_seconds": pre.get("upload_seconds"),
                                    "device_bytes": int(pre.get("device_bytes")), "refresh_bytes": int(pre.get("refresh_bytes")),
                                    "level_rows": pre.hierarchy.level_rows(), "operator_complexity": pre.get("operator_complexity")}
        print(json.dumps(doc["refreshable_build"]), flush=True)
        weights("B")
        s = api.CgSolver()
        s.num_iterations = 200
        s.pre_op = pre
        api.fill_with(x, 0.0)
        ok = s.solve(x, b, op)
        doc["cg_stale"] = {"converged": bool(ok), "iterations": int(s.iteration), "iteration_limit": 200}
        ts, ts_set = [], []
        before = ctx.counter("amg_refreshes")
        for i in range(args.repeats + 1):  # ... B, A, B, A, B: the last refresh leaves B
            name = "B" if (args.repeats - i) % 2 == 0 else "A"
            dt_set, _ = timed(ctx, lambda: weights(name))
            dt, _ = timed(ctx, pre.refresh)
            if i > 0:
                ts.append(dt), ts_set.append(dt_set)
        doc["refresh"] = {"ms_median": 1e3 * float(np.median(ts)), "ms_min": 1e3 * float(min(ts)), "ms_max": 1e3 * float(max(ts)),
                          "set_face_weights_ms_median": 1e3 * float(np.median(ts_set)), "count": ctx.counter("amg_refreshes") - before,
                          "left_on_weights": name}
        print(json.dumps(doc["refresh"]), flush=True)
        doc["cg_refreshed"] = solve(pre)
        pre.close()
        fresh = api.AmgPreconditioner(**params)
        dt, _ = timed(ctx, lambda: fresh.build(x, b, op))
        doc["fresh_build"] = {"seconds": dt, "host_setup_seconds": fresh.get("setup_seconds"), "upload_seconds": fresh.get("upload_seconds"),
                              "device_bytes": int(fresh.get("device_bytes")), "level_rows": fresh.hierarchy.level_rows()}
        doc["cg_fresh"] = solve(fresh)
        fresh.close()
    cheb = api.ChebyshevPreconditioner(degree=2, reduced_records=True)
    doc["cg_chebyshev_degree_2_reduced"] = solve(cheb)
    cheb.close()
    if not args.rebuild_only:
        total = doc["refresh"]["ms_median"] + doc["cg_refreshed"]["ms_median"]
        doc["refresh_plus_refreshed_solve_ms"] = total
        doc["bar_faster_than_chebyshev"] = bool(total < doc["cg_chebyshev_degree_2_reduced"]["ms_median"])
        doc["refresh_over_this_builds_rebuild"] = doc["refresh"]["ms_median"] / (1e3 * doc["fresh_build"]["seconds"])
    print(json.dumps(doc), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
    mat.close()
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
