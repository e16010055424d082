#!/usr/bin/env python3
"""Wall time of a JFNK solve of the cubic problem A(x) = x - kappa L x + c x^3 = b (kappa = 1e-2, c = 0.5,
b = 1 + 0.5 sin(5 x_centre), zero start: tests/test_gpu_jfnk_native.py) in two forms:

  native    -- api.DeviceJfnkSolver: the Newton loop an engine method (STORM_HIP_JFNK), every Jacobian-vector product the
               finite-difference operator's four launches, no scalar on the host inside a step;
  host_loop -- api.JfnkSolver: SolverNewton.hpp:101-173 as a user-level host loop over the device-resident BiCGStab, its
               product a callback that waits for |y| (this change leaves its code untouched:
               `git diff <parent> -- stormruler_amd/api.py` shows only additions outside the class).

Problems: the reference's Triangle meshes square_nb.1 (6 252 cells) and step.1 (79 672), the 64^3 and 128^3 boxes.
Protocol: per problem one warm-up solve of each arm, then 5 timed solves of each arm ALTERNATING (native, host loop,
native, ...), each between Context.sync() calls; the medians, and from them microseconds per inner BiCGStab iteration
(wall / inner iterations: everything a Newton step costs is spread over its inner iterations) and wall time per Newton
step.  Both arms call the same Python callback for A.  Writes one JSON file (--out) and prints one line per problem."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KAPPA, C3 = 1e-2, 0.5
PROBLEMS = ["square_nb.1", "step.1", "box64", "box128"]


def face_graph(name):
    from stormruler_amd import io_tetgen, mesh

    if name.startswith("box"):
        return mesh.structured_box(int(name[3:]))
    g = io_tetgen.read_triangle(os.path.join(ROOT, "tests", "golden", "mesh", name + "."))
    return mesh.FaceGraph(g.n_cells, 2, g.inner, g.outer, g.area, g.center, g.volume, b_center=np.zeros((0, 2)))


def run(name, solves):
    from stormruler_amd import api

    g = face_graph(name)
    ctx = api.Context(0)
    mat = api.StencilMatrix.from_face_graph(ctx, g)
    sq = api.DeviceVector(ctx, g.n_cells)

    def nonlinear(y, x):
        mat.apply(-KAPPA, 1.0, x, y)
        api.vmul(sq, x, x)
        api.vmul_add(y, C3, sq, x)

    op = api.make_operator(nonlinear)
    b = api.DeviceVector.from_numpy(ctx, 1.0 + 0.5 * np.sin(5.0 * g.center[: g.n_cells, 0]))
    arms = {"native": api.DeviceJfnkSolver, "host_loop": api.JfnkSolver}
    times, info, xs = {a: [] for a in arms}, {}, {}
    for timed in [False] + [True] * solves:
        for arm, cls in arms.items():
            x = api.DeviceVector(ctx, g.n_cells)
            s = cls()
            ctx.sync()
            t0 = time.perf_counter()
            ok = s.solve(x, b, op)
            ctx.sync()
            dt = time.perf_counter() - t0
            if not ok:
                raise RuntimeError(f"{name} / {arm}: not converged")
            if timed:
                times[arm].append(dt)
            info[arm] = {"newton_steps": int(s.iteration), "inner_iterations": int(s.inner_iterations),
                         "absolute_error": float(s.absolute_error)}
            xs[arm] = x.to_numpy()
    out = {"problem": name, "rows": int(g.n_cells),
           "x_native_vs_host_loop": float(np.linalg.norm(xs["native"] - xs["host_loop"]) / np.linalg.norm(xs["host_loop"]))}
    for arm in arms:
        med = statistics.median(times[arm])
        out[arm] = dict(info[arm], solve_seconds=times[arm], median_seconds=med,
                        us_per_inner_iteration=1e6 * med / max(1, info[arm]["inner_iterations"]),
                        ms_per_newton_step=1e3 * med / max(1, info[arm]["newton_steps"]))
    out["speedup_native_over_host_loop"] = out["host_loop"]["median_seconds"] / out["native"]["median_seconds"]
    mat.close()
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--problems", nargs="*", default=PROBLEMS)
    ap.add_argument("--solves", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_jfnk_bench.json"))
    args = ap.parse_args()
    results = []
    for name in args.problems:
        r = run(name, args.solves)
        results.append(r)
        print(f"{name:12s} rows {r['rows']:8d}  native {r['native']['us_per_inner_iteration']:8.1f} us/inner it "
              f"({r['native']['ms_per_newton_step']:7.2f} ms/step, {r['native']['inner_iterations']} inner)   host loop "
              f"{r['host_loop']['us_per_inner_iteration']:8.1f} us/inner it ({r['host_loop']['ms_per_newton_step']:7.2f} ms/step, "
              f"{r['host_loop']['inner_iterations']} inner)   x{r['speedup_native_over_host_loop']:.2f}", flush=True)
    with open(args.out, "w") as f:
        json.dump({"protocol": "arms alternating, one warm-up solve each, median of %d" % args.solves, "results": results}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
