#!/usr/bin/env python3
"""Mixed-precision CG (storm_hip_mixed_cg_*) against the PARENT build's storm_hip_solve_cg on the fp64-record path.

    python tools/mixed_cg_bench.py --parent-root DIR --out profiles/r36_mixed_cg_bench.json [--n 256] [--rounds 5]

DIR is a built checkout of the parent commit (its stormruler_amd package with libstorm_hip.so).  The reference of every
comparison is that build, never this build's own fp64 arm (which is recorded beside it).  Operators: the n^3 box in natural
order on fp64 records (option spmv_dict = 0) and bench.py's jittered, scrambled, Morton-ordered box.

Every round starts a FRESH process per build and operator, the parent's first, then this build's (the arms alternate at the
process level: two builds of one library cannot share a process).  A process measures
  * per iteration: parent -- a 200-iteration storm_hip_solve_cg with the tolerances off; this build -- begin + inner(200);
    both between HIP events (storm_hip_timer_start / _stop), `--iter-samples` samples per process;
  * time to tolerance: wall clock between two context synchronisations, x = 0, to 1e-6 and 1e-9, b = 1 and a seeded normal b:
    parent -- storm_hip_solve_cg; this build -- its own storm_hip_solve_cg and the mixed solver at inner_tolerance
    1e-2 / 1e-3 / 1e-4 with keep_direction 0 / 1, the inner / outer / fp64-finish counts beside the times;
  * this build only: the companion's build (storm_hip_op_build_reduced), timed on its own and excluded from everything else.
The driver takes medians over the rounds and writes the table and the bar for a later default: time to 1e-6 more than 6 %
below the parent's on both operators (both right-hand sides, one and the same mixed setting)."""
import argparse
import json
import os
import subprocess
import sys
import time

CEILING = 191.7 / 108.0  # bytes per row and iteration, fp64 loop over fp32 inner loop (records 79.8 -> 51.9, vectors 112 -> 56)
TOLS = (1e-6, 1e-9)
KINDS = ("ones", "random")
MIXED_ARMS = [(itol, keep) for itol in (1e-2, 1e-3, 1e-4) for keep in (0, 1)]
INNER = 200


def worker(a):
    sys.path.insert(0, os.path.abspath(a.root))
    import numpy as np
    from stormruler_amd import api, host_mesh, mesh

    assert os.path.abspath(os.path.dirname(os.path.dirname(api.__file__))) == os.path.abspath(a.root), api.__file__
    new = a.worker == "new"
    ctx = api.Context(0)
    n = a.n
    t0 = time.time()
    g = mesh.structured_box(n)
    ctx.set_option("spmv_dict", 0)  # fp64 records: what every Triangle / TetGen mesh gets
    if a.case == "box":
        mat = api.StencilMatrix.from_face_graph(ctx, g)
    else:  # bench.py's unstructured stress variant
        hm = host_mesh.HostMesh.from_face_graph(mesh.jitter_geometry(g, 1.0 / n))
        hm.permute_cells(mesh.random_permutation(g.n_cells))
        assert hm.order_cells("morton") == "morton"
        mat = hm.create_operator(ctx)
        hm.close()
    ctx.set_option("spmv_dict", 4)
    ctx.sync()
    out = {"arm": a.worker, "case": a.case, "n_rows": g.n_cells, "operator_build_seconds": time.time() - t0}
    st = mat.stats()
    assert st["value_dictionary_size"] == 0 and st["paired_rows"] == 0, st
    N = g.n_cells
    del g
    op = api.HipStencilOperator(mat, alpha=-1.0, beta=0.0)
    rhs = {"ones": np.ones(N), "random": np.random.default_rng(5).standard_normal(N)}
    bs = {k: api.DeviceVector.from_numpy(ctx, v) for k, v in rhs.items()}
    x = api.DeviceVector(ctx, N)

    def fp64_solve(b, tol, iters=None):
        s = api.CgSolver()
        s.num_iterations = iters if iters is not None else 20000
        s.absolute_error_tolerance = s.relative_error_tolerance = tol
        api.fill_with(x, 0.0)
        ctx.sync()
        t = time.perf_counter()
        ok = s.solve(x, b, op)
        ctx.sync()
        return {"seconds": time.perf_counter() - t, "iterations": int(s.iteration), "converged": bool(ok)}

    if new:
        ctx.sync()
        t = time.perf_counter()
        mat.build_reduced()
        ctx.sync()
        out["companion_build_seconds"] = time.perf_counter() - t
        out["companion_bytes"] = int(mat.reduced_bytes)
        out["record_bytes"] = int(st["record_bytes"])

        def mixed_solve(b, tol, itol, keep):
            s = api.MixedCgSolver()
            s.num_iterations = 20000
            s.absolute_error_tolerance = s.relative_error_tolerance = tol
            s.inner_tolerance, s.keep_direction = itol, keep
            s._bound(op)  # the object's allocations are not the solve
            api.fill_with(x, 0.0)
            ctx.sync()
            t = time.perf_counter()
            ok = s.solve(x, b, op)
            ctx.sync()
            r = {"seconds": time.perf_counter() - t, "converged": bool(ok), "inner_iterations": int(s.inner_iterations),
                 "outer_steps": int(s.outer_steps), "fp64_iterations": int(s.fp64_iterations), "finished_fp64": int(s.finished_fp64)}
            s.close()
            return r

    # ---- per iteration, HIP events ----
    def fp64_per_iteration():
        s = api.CgSolver()
        s.num_iterations, s.absolute_error_tolerance, s.relative_error_tolerance = INNER, 0.0, 0.0
        api.fill_with(x, 0.0)
        ctx.timer_start()
        s.solve(x, bs["random"], op)
        ms = ctx.timer_stop()
        assert s.iteration == INNER
        return ms * 1e3 / INNER

    fp64_per_iteration()  # warm-up: code objects, work vectors
    out["fp64_us_per_iteration"] = [fp64_per_iteration() for _ in range(a.iter_samples)]
    if new:
        sm = api.MixedCgSolver()
        api.fill_with(x, 0.0)

        def mixed_per_iteration():
            ctx.timer_start()
            sm.begin(x, bs["random"], op)
            sm.inner(INNER)
            return ctx.timer_stop() * 1e3 / INNER

        mixed_per_iteration()
        # alternating with this build's own fp64 arm inside the process; the parent's comes from the parent's process
        out["mixed_us_per_inner_iteration"] = [mixed_per_iteration() for _ in range(a.iter_samples)]
        sm.close()

    # ---- time to tolerance ----
    fp64_solve(bs["ones"], 1e-2)  # warm-up of the solve path
    if new:
        mixed_solve(bs["ones"], 1e-2, 1e-2, 0)
    ttt = {}
    for tol in TOLS:
        for kind in KINDS:
            key = f"{tol:g}/{kind}"
            ttt[key] = {"fp64": fp64_solve(bs[kind], tol)}
            if new:
                for itol, keep in MIXED_ARMS:
                    ttt[key][f"mixed itol={itol:g} keep={keep}"] = mixed_solve(bs[kind], tol, itol, keep)
    out["time_to_tolerance"] = ttt
    print("RESULT " + json.dumps(out), flush=True)
    mat.close()
    ctx.close()


def median(v):
    v = sorted(v)
    return None if not v else (v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2]))


def driver(a):
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    roots = {"parent": os.path.abspath(a.parent_root), "new": here}
    runs = {(arm, case): [] for arm in roots for case in a.cases}
    for rnd in range(a.rounds):
        for case in a.cases:
            for arm in ("parent", "new"):  # alternating, a fresh process each
                cmd = [sys.executable, os.path.abspath(__file__), "--worker", arm, "--root", roots[arm], "--case", case, "--n", str(a.n),
                       "--iter-samples", str(a.iter_samples)]
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.worker_timeout, cwd=roots[arm])
                line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
                if p.returncode != 0 or not line:
                    raise RuntimeError(f"worker {arm}/{case} failed ({p.returncode}): {(p.stdout + p.stderr)[-2000:]}")
                runs[(arm, case)].append(json.loads(line[-1][7:]))
                print(f"round {rnd} {case} {arm}: done", flush=True)
    report = {"n": a.n, "rounds": a.rounds, "iter_samples_per_process": a.iter_samples, "ceiling_by_bytes": CEILING,
              "inner_iterations_per_sample": INNER, "cases": {}, "tetrahedra_12_6M": "NOT MEASURED", "raw": {f"{k[0]}/{k[1]}": v for k, v in runs.items()}}
    best_everywhere = None
    for case in a.cases:
        par, new = runs[("parent", case)], runs[("new", case)]
        us_parent = median([u for r in par for u in r["fp64_us_per_iteration"]])
        us_own = median([u for r in new for u in r["fp64_us_per_iteration"]])
        us_mixed = median([u for r in new for u in r["mixed_us_per_inner_iteration"]])
        c = {"n_rows": par[0]["n_rows"],
             "per_iteration": {"parent_fp64_us": us_parent, "this_build_fp64_us": us_own, "mixed_inner_us": us_mixed,
                               "ratio_parent_over_mixed": us_parent / us_mixed, "ceiling_by_bytes": CEILING,
                               "samples_per_arm": a.rounds * a.iter_samples},
             "companion_build_seconds": median([r["companion_build_seconds"] for r in new]),
             "companion_bytes": new[0]["companion_bytes"], "record_bytes": new[0]["record_bytes"], "time_to_tolerance": {}}
        for key in par[0]["time_to_tolerance"]:
            ref = median([r["time_to_tolerance"][key]["fp64"]["seconds"] for r in par])
            row = {"parent_fp64": {"seconds": ref, "iterations": par[0]["time_to_tolerance"][key]["fp64"]["iterations"]}}
            for arm in new[0]["time_to_tolerance"][key]:
                t = median([r["time_to_tolerance"][key][arm]["seconds"] for r in new])
                row["this_build_fp64" if arm == "fp64" else arm] = dict(new[0]["time_to_tolerance"][key][arm], seconds=t,
                                                                        relative_to_parent=t / ref)
            c["time_to_tolerance"][key] = row
        # the bar: one mixed setting more than 6 % below the parent at 1e-6 for both right-hand sides
        ok = {arm for arm in c["time_to_tolerance"]["1e-06/ones"] if arm.startswith("mixed") and
              all(c["time_to_tolerance"][f"1e-06/{k}"][arm]["relative_to_parent"] < 0.94 and
                  c["time_to_tolerance"][f"1e-06/{k}"][arm]["converged"] for k in KINDS)}
        c["settings_meeting_the_bar"] = sorted(ok)
        best_everywhere = ok if best_everywhere is None else best_everywhere & ok
        report["cases"][case] = c
    full = a.rounds >= 5 and set(a.cases) == {"box", "morton"} and a.n == 256
    report["bar"] = {"rule": "time to 1e-6 more than 6 % below the parent build's on both boxes (median of 5 fresh-process rounds)",
                     "settings_meeting_it_on_every_case_run": sorted(best_everywhere or []),
                     "verdict": ("MET" if best_everywhere else "NOT MET") if full else "NOT MEASURED (fewer rounds, cases or rows than the rule names)"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(report, f, indent=1)
    for case, c in report["cases"].items():
        pi = c["per_iteration"]
        print(f"{case}: parent fp64 {pi['parent_fp64_us']:.1f} us/it, mixed inner {pi['mixed_inner_us']:.1f} us/it, ratio "
              f"{pi['ratio_parent_over_mixed']:.3f} (ceiling {CEILING:.2f}); companion build {c['companion_build_seconds'] * 1e3:.1f} ms")
        for key, row in c["time_to_tolerance"].items():
            for arm, v in row.items():
                extra = "" if "inner_iterations" not in v else (f" inner {v['inner_iterations']} outer {v['outer_steps']} fp64 "
                                                                f"{v['fp64_iterations']} (finished_fp64 {v['finished_fp64']})")
                rel = "" if "relative_to_parent" not in v else f" x{v['relative_to_parent']:.3f}"
                print(f"  {key:>16} {arm:<28} {v['seconds'] * 1e3:9.2f} ms{rel} it {v.get('iterations', '')}{extra}")
    print("bar:", report["bar"]["verdict"], report["bar"]["settings_meeting_it_on_every_case_run"])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-root")
    ap.add_argument("--out", default="profiles/r36_mixed_cg_bench.json")
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iter-samples", type=int, default=6, help="per process: rounds x this = samples per arm (30 by default)")
    ap.add_argument("--cases", nargs="+", default=["box", "morton"], choices=["box", "morton"])
    ap.add_argument("--worker-timeout", type=int, default=900)
    ap.add_argument("--worker", choices=["parent", "new"])
    ap.add_argument("--root")
    ap.add_argument("--case", default="box")
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    if not a.parent_root:
        ap.error("--parent-root DIR (a built checkout of the parent commit) is required")
    driver(a)


if __name__ == "__main__":
    main()
