#!/usr/bin/env python3
"""The cavity's pressure solve with the initial guess projected onto past solves (SolutionRecycler), on one MI355X.

    python tools/recycle_bench.py --parent-root DIR [--small] [--steps 30] [--runs 3] [--out profiles/NAME.json]

The 128^3 lid-driven cavity of stormruler_amd/cavity.py (64^3 with --small), `steps` time steps per run, the first five
left out.  Arms:
  parent     the PARENT commit's build (--parent-root: a built checkout of it), CavityProjection(ctx, n): the warm start.
             This is the reference;
  plain      this build, CavityProjection(ctx, n): must match the parent's within the +-3 % box-to-box spread (no existing
             kernel changed);
  recycle8, recycle16   this build, CavityProjection(ctx, n, pressure_recycle=8 / 16).
Every run is a fresh child process and the arms alternate run by run.  The measured quantity is the host clock between two
context synchronisations around the pressure solve -- guess + solve + the extra apply + update, all inside solver.solve();
a run's figure is the median over its steps, an arm's the median of its runs (tools/cavity_amg_bench.py's method).  Also
reported: the iterations per step, the recycler's device bytes, and (one more child) the microseconds per guess and per
update at the cavity's size, fused kernels against the statement path: HIP events, the two paths alternating, the median of 30.
The bar for making it the cavity's default: the recycled pressure-solve time more than 6 % below the parent's plain arm
(twice the box-to-box spread).  The document says which way it fell; the default stays 0 either way.
Prints and writes one JSON document."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKIP = 5  # steps left out of a run's median
ARMS = {"parent": 0, "plain": 0, "recycle8": 8, "recycle16": 16}
MICRO_SAMPLES = 30


def child(args) -> int:
    sys.path.insert(0, os.path.abspath(args.package_root))
    from stormruler_amd import api
    from stormruler_amd.cavity import CavityProjection

    ctx = api.Context(0)
    n = 64 if args.small else 128
    m = ARMS[args.arm]
    drv = CavityProjection(ctx, n, pressure_recycle=m) if m else CavityProjection(ctx, n)
    ctx.sync()
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
    doc = {"arm": args.arm, "n": n, "device": ctx.info()["name"], "steps": steps, "divergence_norm": drv.divergence_norm()}
    if m:
        rec = drv.solver.recycler
        doc["device_bytes"], doc["restarts"] = int(rec.get("device_bytes")), int(rec.get("restarts"))
    print(json.dumps(doc), flush=True)
    ctx.close()
    return 0


def micro(args) -> int:
    """Microseconds per guess (8 pairs) and per update (into slot 7) at the cavity's size, per path."""
    sys.path.insert(0, ROOT)
    from stormruler_amd import api

    ctx = api.Context(0)
    side = 64 if args.small else 128
    n = side ** 3
    i = np.arange(n, dtype=np.float64)
    vecs = [api.DeviceVector.from_numpy(ctx, np.sin(0.37 * i + k)) for k in range(4)]
    b, x, xs, ax = vecs
    rec = api.SolutionRecycler(ctx, n, capacity=8)

    pairs = [(api.DeviceVector.from_numpy(ctx, np.cos(0.011 * (j + 1) * i)),
              api.DeviceVector.from_numpy(ctx, 2.0 * np.cos(0.011 * (j + 1) * i) + np.sin(0.5 * j + 0.001 * i))) for j in range(7)]

    def fill(count):
        rec.reset()
        for u, v in pairs[:count]:
            rec.update(u, v)

    times = {"guess": {0: [], 1: []}, "update": {0: [], 1: []}}
    for sample in range(MICRO_SAMPLES + 2):
        for fused in (1, 0) if sample % 2 else (0, 1):
            ctx.set_option("recycle_fused", fused)
            fill(7)
            rec.guess(b, x)
            ctx.sync()
            ctx.timer_start()
            rec.update(xs, ax)
            t_update = 1e3 * ctx.timer_stop()
            ctx.timer_start()
            rec.guess(b, x)
            t_guess = 1e3 * ctx.timer_stop()
            if sample >= 2:  # (two warm-up rounds)
                times["update"][fused].append(t_update)
                times["guess"][fused].append(t_guess)
    ctx.set_option("recycle_fused", 1)
    doc = {"n": n, "pairs": 8, "samples": MICRO_SAMPLES,
           "guess_us": {"fused": float(np.median(times["guess"][1])), "statements": float(np.median(times["guess"][0]))},
           "update_us": {"fused": float(np.median(times["update"][1])), "statements": float(np.median(times["update"][0]))},
           "device_bytes": int(rec.get("device_bytes"))}
    print(json.dumps(doc), flush=True)
    rec.close()
    ctx.close()
    return 0


def summary(runs):
    per_run = []
    for r in runs:
        tail = r["steps"][SKIP:]
        per_run.append({"pressure_iterations_median": float(np.median([s["pressure_iterations"] for s in tail])),
                        "pressure_iterations": [s["pressure_iterations"] for s in r["steps"]],
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
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--runs", type=int, default=3, help="runs per arm")
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit (the reference arm)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--arm", choices=list(ARMS) + ["micro"], default=None, help="(internal) run one arm in this process")
    ap.add_argument("--package-root", default=ROOT, help="(internal) the tree the child imports")
    args = ap.parse_args()
    if args.arm == "micro":
        return micro(args)
    if args.arm is not None:
        return child(args)
    if args.steps <= SKIP:
        ap.error(f"--steps must exceed {SKIP}")
    arms = [a for a in ARMS if a != "parent" or args.parent_root]
    runs = {a: [] for a in arms}

    def spawn(arm, root):
        cmd = [sys.executable, os.path.abspath(__file__), "--arm", arm, "--steps", str(args.steps), "--package-root", root]
        done = subprocess.run(cmd + (["--small"] if args.small else []), capture_output=True, text=True)
        if done.returncode != 0:
            print(done.stdout[-2000:], done.stderr[-4000:], file=sys.stderr)
            return None
        return json.loads(done.stdout.strip().splitlines()[-1])

    for _ in range(args.runs):
        for arm in arms:
            last = spawn(arm, args.parent_root if arm == "parent" else ROOT)
            if last is None:
                return 1
            runs[arm].append(last)
            print(f"{arm}: iterations {[s['pressure_iterations'] for s in last['steps']]}, pressure solve "
                  f"{np.median([s['pressure_solve_ms'] for s in last['steps'][SKIP:]]):.2f} ms", flush=True)
    mic = spawn("micro", ROOT)
    if mic is None:
        return 1
    res = {a: summary(runs[a]) for a in arms}
    ref = "parent" if "parent" in res else "plain"
    base = res[ref]["pressure_solve_ms_median"]
    doc = {"device": runs["plain"][0]["device"], "n": runs["plain"][0]["n"], "steps_per_run": args.steps, "steps_skipped": SKIP,
           "runs_per_arm": args.runs, "reference_arm": ref,
           "parent_root": None if not args.parent_root else os.path.relpath(os.path.abspath(args.parent_root), ROOT),
           "method": "fresh child process per run, arms alternating; host clock between context syncs around solver.solve() "
                     "(guess + solve + the extra apply + update); per run the median over the steps after the first five, per arm "
                     "the median of the runs",
           "arms": res, "micro": mic,
           "over_reference": {a: res[a]["pressure_solve_ms_median"] / base for a in arms},
           "plain_matches_parent_within_3_percent": (abs(res["plain"]["pressure_solve_ms_median"] / base - 1.0) <= 0.03) if ref == "parent" else None,
           "more_than_6_percent_faster": {a: bool(res[a]["pressure_solve_ms_median"] / base < 0.94) for a in arms if a.startswith("recycle")},
           "device_bytes": {a: runs[a][0].get("device_bytes") for a in arms if a.startswith("recycle")},
           "divergence_norm": {a: runs[a][0]["divergence_norm"] for a in arms},
           "raw": runs}
    print(json.dumps({k: v for k, v in doc.items() if k != "raw"}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
