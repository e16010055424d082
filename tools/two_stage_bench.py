#!/usr/bin/env python3
"""Microseconds per CG iteration of the playground's Cahn-Hilliard solve (Playground.cpp:151-167) on the reference's
meshes and the 64^3 and 80^3 boxes, in three forms (tools/two_stage_bench.cpp, C++ against include/storm_hip/Storm.hpp as the
playground is):

  1. callback -- `make_operator` over the lambda with its two stormDivGrad calls, exactly as tests/cpp/timestep_driver.cpp
     builds it.  Uses nothing of the two-stage operator: the BASELINE is this mode on a build of the parent commit --
     the same source compiled against the parent's header and library (the two-stage modes compile out where the header
     lacks STORM_HIP_HAS_TWO_STAGE).  --parent-tree DIR names a checkout of the parent commit in which the library has
     been built (`make -C DIR/stormruler_amd/csrc`): the binary is compiled into DIR/two_stage_bench; --parent-binary
     names one that exists already.  This tree's own callback mode is recorded beside it.  (The lambda is affine, not
     linear, and plain CG with the tolerances off iterates on it for all 500 iterations as the playground's own call
     does: its iterates need not stay bounded, while the two other arms solve the well-posed linear part.  The
     launches per iteration, which is what is timed, are the same either way.)
  2. engine   -- HipTwoStageOperator, option latency_path = 0: the engine's CG loop, both stages as library launches;
  3. latency  -- HipTwoStageOperator on the one-kernel path (csrc/latency.hip, cg2_latency_kernel).

Playground constants, tolerances off, 500 iterations, one warm-up solve and the median of 5 solves between
Context::sync() calls.  One process at a time, each under its own time limit; a failing step ends the run.  The arms of
a problem run one after the other (parent callback, callback, engine, latency), not interleaved: a drift of the clocks
within a problem's ~10 s lands on the later arms.  Writes one JSON file (--out, default
profiles/r19_two_stage_bench.json) and prints one line per measurement."""
import argparse
import gzip
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINARY = os.path.join(ROOT, "tools", "two_stage_bench")
# (box80: 512 000 rows, two slices per wavefront -- the top of what option latency_rows admits by default)
PROBLEMS = [("square_nb.1", "mesh"), ("rectangle.1", "mesh"), ("step.1", "mesh"), ("box64", "box:64"), ("box80", "box:80")]


def build_binary(tree=ROOT, out=BINARY):
    """tools/two_stage_bench.cpp of THIS tree against the header and the library of `tree`."""
    lib_dir = os.path.join(tree, "stormruler_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(tree, "include"),
                           os.path.join(ROOT, "tools", "two_stage_bench.cpp"), "-L" + lib_dir, "-lstorm_hip",
                           "-Wl,-rpath," + os.path.abspath(lib_dir), "-Wl,-rpath-link,/opt/rocm/lib", "-o", out])


def stage_mesh(name, workdir):
    """The TetGen files of tests/golden/mesh under one prefix in workdir (some are stored gzipped)."""
    src = os.path.join(ROOT, "tests", "golden", "mesh")
    for ext in ("node", "edge", "ele"):
        plain, packed = os.path.join(src, f"{name}.{ext}"), os.path.join(src, f"{name}.{ext}.gz")
        dst = os.path.join(workdir, f"{name}.{ext}")
        if os.path.exists(plain):
            shutil.copy(plain, dst)
        else:
            with gzip.open(packed, "rb") as fi, open(dst, "wb") as fo:
                shutil.copyfileobj(fi, fo)
    return os.path.join(workdir, name + ".")


def measure(binary, mode, problem, iterations, solves):
    p = subprocess.run([binary, mode, problem, str(iterations), str(solves)], capture_output=True, text=True, timeout=300)
    if p.returncode != 0:
        raise SystemExit(f"{binary} {mode} {problem}: exit status {p.returncode}\n{p.stderr[-2000:]}")
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-binary", help="two_stage_bench compiled against a build of the parent commit (mode 1, the baseline)")
    ap.add_argument("--parent-tree", help="a checkout of the parent commit with its library built: the baseline binary is compiled there")
    ap.add_argument("--iterations", type=int, default=500)
    ap.add_argument("--solves", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_two_stage_bench.json"))
    args = ap.parse_args()
    if not os.path.exists(BINARY):
        build_binary()
    if args.parent_tree and not args.parent_binary:
        args.parent_binary = os.path.join(args.parent_tree, "two_stage_bench")
        if not os.path.exists(args.parent_binary):
            build_binary(args.parent_tree, args.parent_binary)
    arms = ([("callback_parent", args.parent_binary, "callback")] if args.parent_binary else []) + \
           [("callback", BINARY, "callback"), ("engine", BINARY, "engine"), ("latency", BINARY, "latency")]
    results = []
    with tempfile.TemporaryDirectory() as workdir:
        for name, kind in PROBLEMS:
            problem = kind if kind != "mesh" else "mesh:" + stage_mesh(name, workdir)
            row = {"problem": name}
            for arm, binary, mode in arms:
                r = measure(binary, mode, problem, args.iterations, args.solves)
                row["rows"] = r["rows"]
                row[arm + "_us_per_iteration"] = r["us_per_iteration"]
                row[arm + "_solves_us_per_iteration"] = r["solves_us_per_iteration"]
                if arm == "latency" and r["latency_solves"] != args.solves + 1:
                    raise SystemExit(f"{name}: the one-kernel path did not take every solve ({r['latency_solves']})")
                print(json.dumps({"problem": name, "rows": r["rows"], "arm": arm, "us_per_iteration": r["us_per_iteration"]}), flush=True)
            base = row.get("callback_parent_us_per_iteration", row["callback_us_per_iteration"])
            row["baseline"] = "callback_parent" if args.parent_binary else "callback"
            row["latency_speedup_over_baseline"] = base / row["latency_us_per_iteration"]
            row["engine_speedup_over_baseline"] = base / row["engine_us_per_iteration"]
            results.append(row)
    doc = {"what": "us per CG iteration, playground constants, tolerances off", "iterations": args.iterations,
           "solves": args.solves, "statistic": "median of the timed solves (one warm-up solve before them)", "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"written": os.path.relpath(args.out, ROOT)}))


if __name__ == "__main__":
    sys.exit(main())
