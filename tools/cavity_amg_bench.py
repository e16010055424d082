#!/usr/bin/env python3
"""The cavity driver's pressure solve with and without the multigrid preconditioner, on one MI355X.

    python tools/cavity_amg_bench.py [--small] [--steps 15] [--runs 3] [--package-root DIR] [--out profiles/NAME.json]

The 128^3 lid-driven cavity of stormruler_amd/cavity.py (64^3 with --small), `steps` time steps per run.  Two arms:
  plain  CavityProjection(ctx, n): warm-started CG on -L_N p = rhs, no preconditioner (the driver's default);
  amg    CavityProjection(ctx, n, pressure_preconditioner="amg"): the same CG with AmgPreconditioner(nullspace="constant")
         on a second, fp64 copy of L_N.  The preconditioner is built in the constructor, outside the timed steps.
Every run is a fresh child process; the arms alternate run by run (plain, amg, plain, amg, ...), so that a drift of the
machine touches both alike.  Per step the child records the pressure iterations and the pressure-solve time: the host clock
between two context synchronisations around solver.solve().  A run's figure is the median over the steps after the first
five (the flow, and with it the iteration count, is still starting up there); an arm's figure is the median of its runs.
--package-root names the tree whose stormruler_amd package (and library) the PLAIN arm imports: a checkout of the parent
commit, built -- the reference for the plain figures, measured in the same session.  Without it both arms import this tree.
No bar: the driver's default stays plain CG whatever comes out.  The document says whether the multigrid arm's pressure-solve
time is more than 6 % below the plain arm's (twice the box-to-box spread).  Prints and writes one JSON document."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKIP = 5  # steps left out of a run's median


def child(args) -> int:
    sys.path.insert(0, os.path.abspath(args.package_root))
    from stormruler_amd import api
    from stormruler_amd.cavity import CavityProjection

    ctx = api.Context(0)
    n = 64 if args.small else 128
    t0 = time.perf_counter()
    drv = CavityProjection(ctx, n) if args.arm == "plain" else CavityProjection(ctx, n, pressure_preconditioner="amg")
    ctx.sync()
    build_seconds = time.perf_counter() - t0
    solve, spent = drv.solver.solve, []

    def timed_solve(x, b, op):
        ctx.sync()
        t = time.perf_counter()
        ok = solve(x, b, op)
        ctx.sync()
        spent.append(time.perf_counter() - t)
        return ok

    drv.solver.solve = timed_solve
    steps = []
    for _ in range(args.steps):
        it, sec, ok = drv.step()
        steps.append({"pressure_iterations": int(it), "pressure_solve_ms": 1e3 * spent[-1], "step_ms": 1e3 * sec, "converged": bool(ok)})
    doc = {"arm": args.arm, "n": n, "device": ctx.info()["name"], "build_seconds": build_seconds, "steps": steps,
           "divergence_norm": drv.divergence_norm()}
    if args.arm == "amg":
        pre = drv.solver.pre_op
        doc["level_rows"] = pre.hierarchy.level_rows()
        doc["setup_seconds"], doc["upload_seconds"] = pre.get("setup_seconds"), pre.get("upload_seconds")
        doc["device_bytes"] = int(pre.get("device_bytes"))
    print(json.dumps(doc), flush=True)
    ctx.close()
    return 0


def summary(runs):
    """Medians over the steps after the first SKIP, per run; then the median of the runs."""
    per_run = []
    for r in runs:
        tail = r["steps"][SKIP:]
        per_run.append({"pressure_iterations_median": float(np.median([s["pressure_iterations"] for s in tail])),
                        "pressure_solve_ms_median": float(np.median([s["pressure_solve_ms"] for s in tail])),
                        "step_ms_median": float(np.median([s["step_ms"] for s in tail])),
                        "all_converged": all(s["converged"] for s in r["steps"])})
    ms = [p["pressure_solve_ms_median"] for p in per_run]
    return {"runs": per_run, "pressure_iterations_median": float(np.median([p["pressure_iterations_median"] for p in per_run])),
            "pressure_solve_ms_median": float(np.median(ms)), "pressure_solve_ms_min": float(min(ms)),
            "pressure_solve_ms_max": float(max(ms)), "step_ms_median": float(np.median([p["step_ms_median"] for p in per_run]))}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true", help="64^3 instead of 128^3")
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--runs", type=int, default=3, help="runs per arm")
    ap.add_argument("--package-root", default=ROOT, help="the tree the plain arm imports (a built checkout of the parent commit)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--arm", choices=["plain", "amg"], default=None, help="(internal) run one arm in this process")
    args = ap.parse_args()
    if args.arm is not None:
        return child(args)
    if args.steps <= SKIP:
        ap.error(f"--steps must exceed {SKIP}")
    runs = {"plain": [], "amg": []}
    for _ in range(args.runs):
        for arm in ("plain", "amg"):
            root = args.package_root if arm == "plain" else ROOT
            cmd = [sys.executable, os.path.abspath(__file__), "--arm", arm, "--steps", str(args.steps), "--package-root", root]
            done = subprocess.run(cmd + (["--small"] if args.small else []), capture_output=True, text=True)
            if done.returncode != 0:
                print(done.stdout[-2000:], done.stderr[-4000:], file=sys.stderr)
                return 1
            runs[arm].append(json.loads(done.stdout.strip().splitlines()[-1]))
            last = runs[arm][-1]
            print(f"{arm}: iterations {[s['pressure_iterations'] for s in last['steps']]}, pressure solve "
                  f"{np.median([s['pressure_solve_ms'] for s in last['steps'][SKIP:]]):.2f} ms", flush=True)
    plain, amg = summary(runs["plain"]), summary(runs["amg"])
    ratio = amg["pressure_solve_ms_median"] / plain["pressure_solve_ms_median"]
    doc = {"device": runs["amg"][0]["device"], "n": runs["amg"][0]["n"], "steps_per_run": args.steps, "steps_skipped": SKIP,
           "runs_per_arm": args.runs, "plain_package_root": os.path.relpath(os.path.abspath(args.package_root), ROOT),
           "method": "fresh child process per run, arms alternating; host clock between context syncs around solver.solve(); "
                     "per run the median over the steps after the first five, per arm the median of the runs",
           "plain": plain, "amg": amg, "amg_over_plain_pressure_solve": ratio, "amg_more_than_6_percent_faster": bool(ratio < 0.94),
           "amg_build": {k: runs["amg"][0][k] for k in ("level_rows", "setup_seconds", "upload_seconds", "device_bytes", "build_seconds")},
           "plain_build_seconds": runs["plain"][0]["build_seconds"],
           "divergence_norm": {"plain": runs["plain"][0]["divergence_norm"], "amg": runs["amg"][0]["divergence_norm"]},
           "raw": runs}
    print(json.dumps({k: v for k, v in doc.items() if k != "raw"}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
