#!/usr/bin/env python3
"""Preconditioned CG on the one-kernel path (option latency_pre, csrc/latency.hip pcg_latency_kernel) against the engine's
loop and against plain latency CG, on one MI355X.

    python tools/latency_pcg_bench.py --parent-root DIR [--rounds 5] [--iterations 200] [--out profiles/NAME.json]

Problems: the Triangle meshes square_nb.1, rectangle.1 and step.1 of tests/golden/mesh (A = I - 1e-2 M, the recorded run of
BASELINE.md 2) and the 64^3 box (A = -M, BASELINE config 1).  CG from x = 0 to 1e-6 (absolute and relative) on the
right-hand side of tools/two_stage_bench.cpp (its 64-bit congruential sequence in [0, 1)), at most 2000 iterations.
Arms:
  plain           CG without a preconditioner on the latency kernel (latency_path 2)
  jacobi_engine, cheb2_engine, chebj4_engine
                  JacobiPreconditioner, ChebyshevPreconditioner(2), ChebyshevPreconditioner(4, jacobi=True) on the engine's
                  statement loop (latency_pre 0: today's road)
  jacobi_latency, cheb2_latency, chebj4_latency
                  the same three with latency_pre 1 (this build only)
The REFERENCE of the plain and engine arms is the parent commit's build (--parent-root: a built checkout of it): every
round is one fresh child process per build and problem, which runs each of its arms once -- a warm-up solve, the timed
solve to tolerance, and a timed solve of `iterations` iterations with the tolerances off (microseconds per iteration) --
in an order that rotates with the round; the two builds' children alternate.  Time: the host clock between two context
synchronisations.  An arm's figure is the median over the rounds.  This build's own plain and engine arms are recorded
beside the parent's (no existing kernel changed: they must agree within the +-3 % box-to-box spread).
The bar for proposing latency_pre = 1 as a default: time to tolerance more than 6 % below the parent's engine arm with
the same preconditioner on both square_nb.1 and step.1, and no slower than it on the 64^3 box.  The document says which
way it fell; the option stays 0 either way.  Prints and writes one JSON document."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBLEMS = ["square_nb.1", "rectangle.1", "step.1", "box64"]
PRECONDITIONERS = ["jacobi", "cheb2", "chebj4"]
OLD_ARMS = ["plain"] + [p + "_engine" for p in PRECONDITIONERS]
NEW_ARMS = [p + "_latency" for p in PRECONDITIONERS]
MAX_ITERATIONS = 2000


def right_hand_side(n):
    """tools/two_stage_bench.cpp: lcg = lcg * 6364136223846793005 + 1442695040888963407, (lcg >> 11) / 2^53, from 2024."""
    out, lcg, mask = np.empty(n), 2024, (1 << 64) - 1
    for i in range(n):
        lcg = (lcg * 6364136223846793005 + 1442695040888963407) & mask
        out[i] = (lcg >> 11) / 9007199254740992.0
    return out


def child(args) -> int:
    sys.path.insert(0, os.path.abspath(args.package_root))
    from stormruler_amd import api, io_tetgen, mesh

    ctx = api.Context(0)
    if args.problem == "box64":
        g, alpha, beta = mesh.structured_box(64), -1.0, 0.0
    else:
        g = io_tetgen.read_triangle(os.path.join(ROOT, "tests", "golden", "mesh", args.problem + "."))
        g = mesh.FaceGraph(g.n_cells, 2, g.inner, g.outer, g.area, g.center, g.volume, b_center=np.zeros((0, 2)))
        alpha, beta = -1.0e-2, 1.0
    mat = api.StencilMatrix.from_face_graph(ctx, g)
    op = api.HipStencilOperator(mat, alpha, beta)
    b = api.DeviceVector.from_numpy(ctx, right_hand_side(g.n_cells))
    x = api.DeviceVector(ctx, g.n_cells)
    ctx.set_option("latency_path", 2)  # (the latency kernel itself: 1 hands the box to the resident path)
    arms = args.arms.split(",")
    arms = arms[args.round % len(arms):] + arms[:args.round % len(arms)]
    doc = {"problem": args.problem, "rows": int(g.n_cells), "device": ctx.info()["name"], "arms": {}}
    for arm in arms:
        kind, _, road = arm.partition("_")
        if road == "latency":
            ctx.set_option("latency_pre", 1)
        pre = {"plain": lambda: None, "jacobi": api.JacobiPreconditioner, "cheb2": lambda: api.ChebyshevPreconditioner(degree=2),
               "chebj4": lambda: api.ChebyshevPreconditioner(degree=4, jacobi=True)}[kind]()
        if pre is not None:  # (a solver builds its preconditioner on every solve: built once here, outside what is timed)
            pre.build(x, b, op)
            pre.build = lambda x_vec, b_vec, any_op: None
        keys = ("latency_solves", "engine_solves") + (("latency_pre_solves",) if road == "latency" else ())
        before = {k: ctx.counter(k) for k in keys}

        def solve(iterations, tol):
            s = api.CgSolver()
            s.pre_op, s.num_iterations = pre, iterations
            s.absolute_error_tolerance = s.relative_error_tolerance = tol
            api.fill_with(x, 0.0)
            ctx.sync()
            t = time.perf_counter()
            ok = s.solve(x, b, op)
            ctx.sync()
            return s, bool(ok), 1e6 * (time.perf_counter() - t)

        solve(MAX_ITERATIONS, 1e-6)
        s, ok, us = solve(MAX_ITERATIONS, 1e-6)
        sf, _, usf = solve(args.iterations, 0.0)
        moved = {k: ctx.counter(k) - before[k] for k in keys}
        doc["arms"][arm] = {"iterations": int(s.iteration), "converged": ok, "solve_us": us,
                            "us_per_iteration": usf / max(int(sf.iteration), 1), "fixed_iterations": int(sf.iteration),
                            "path_fallback": int(s.path_fallback), "moved": moved}
        if road == "latency":
            ctx.set_option("latency_pre", 0)
        if hasattr(pre, "close"):
            pre.close()
    print(json.dumps(doc), flush=True)
    mat.close()
    ctx.close()
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit (the reference of the plain and engine arms)")
    ap.add_argument("--rounds", type=int, default=5, help="solves per arm")
    ap.add_argument("--iterations", type=int, default=200, help="iterations of the solve with the tolerances off")
    ap.add_argument("--problems", default=",".join(PROBLEMS))
    ap.add_argument("--out", default=None)
    ap.add_argument("--problem", default=None, help="(internal) run one round of one problem in this process")
    ap.add_argument("--arms", default=None, help="(internal)")
    ap.add_argument("--round", type=int, default=0, help="(internal)")
    ap.add_argument("--package-root", default=ROOT, help="(internal) the tree the child imports")
    args = ap.parse_args()
    if args.problem is not None:
        return child(args)
    builds = ([("parent", args.parent_root, OLD_ARMS)] if args.parent_root else []) + [("this", ROOT, OLD_ARMS + NEW_ARMS)]
    raw = {p: {name: [] for name, _, _ in builds} for p in args.problems.split(",")}
    for problem in raw:
        for rnd in range(args.rounds):
            for name, root, arms in builds:
                cmd = [sys.executable, os.path.abspath(__file__), "--problem", problem, "--arms", ",".join(arms), "--round", str(rnd),
                       "--iterations", str(args.iterations), "--package-root", root]
                done = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
                if done.returncode != 0:
                    print(done.stdout[-2000:], done.stderr[-4000:], file=sys.stderr)
                    return 1
                raw[problem][name].append(json.loads(done.stdout.strip().splitlines()[-1]))
            print(f"{problem} round {rnd}: " + ", ".join(
                f"{a} {v['iterations']} it {v['solve_us']:.0f} us" for a, v in raw[problem]["this"][-1]["arms"].items()), flush=True)
    ref = "parent" if args.parent_root else "this"
    results = {}
    for problem, by_build in raw.items():
        row = {"rows": by_build["this"][0]["rows"], "arms": {}}
        for name, runs in by_build.items():
            for arm in runs[0]["arms"]:
                vals = [r["arms"][arm] for r in runs]
                row["arms"][(arm if name == "this" else arm + "@parent")] = {
                    "iterations": vals[0]["iterations"], "converged": all(v["converged"] for v in vals),
                    "solve_us_median": float(np.median([v["solve_us"] for v in vals])),
                    "solve_us": [v["solve_us"] for v in vals],
                    "us_per_iteration_median": float(np.median([v["us_per_iteration"] for v in vals])),
                    "path_fallback": max(v["path_fallback"] for v in vals), "moved": vals[0]["moved"]}
        suffix = "@parent" if ref == "parent" else ""
        plain = row["arms"]["plain" + suffix]
        row["new_over_parent_engine"], row["new_over_parent_plain"], row["this_over_parent"] = {}, {}, {}
        for p in PRECONDITIONERS:
            new, eng = row["arms"][p + "_latency"], row["arms"][p + "_engine" + suffix]
            row["new_over_parent_engine"][p] = {"time_to_tolerance": new["solve_us_median"] / eng["solve_us_median"],
                                                "us_per_iteration": new["us_per_iteration_median"] / eng["us_per_iteration_median"]}
            row["new_over_parent_plain"][p] = {"time_to_tolerance": new["solve_us_median"] / plain["solve_us_median"],
                                               "us_per_iteration": new["us_per_iteration_median"] / plain["us_per_iteration_median"]}
        if ref == "parent":
            row["this_over_parent"] = {a: row["arms"][a]["solve_us_median"] / row["arms"][a + "@parent"]["solve_us_median"] for a in OLD_ARMS}
        results[problem] = row
    bar = {}
    for p in PRECONDITIONERS:
        have = all(q in results for q in ("square_nb.1", "step.1", "box64"))
        bar[p] = (all(results[q]["new_over_parent_engine"][p]["time_to_tolerance"] < 0.94 for q in ("square_nb.1", "step.1")) and
                  results["box64"]["new_over_parent_engine"][p]["time_to_tolerance"] <= 1.0) if have else None
    doc = {"device": next(iter(raw.values()))["this"][0]["device"], "rounds": args.rounds, "fixed_iterations": args.iterations,
           "reference_build": ref,
           "parent_root": None if not args.parent_root else os.path.relpath(os.path.abspath(args.parent_root), ROOT),
           "method": "one fresh child process per build, problem and round, the builds alternating, the arms' order rotating with the "
                     "round; per arm a warm-up solve, the timed solve to 1e-6 and a timed solve with the tolerances off; host clock "
                     "between context syncs; medians over the rounds; the preconditioner is built outside the timed region",
           "results": results, "meets_the_bar_for_a_default": bar, "raw": raw}
    print(json.dumps({k: v for k, v in doc.items() if k != "raw"}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
