#!/usr/bin/env python3
"""What the cooperative tail of the multigrid cycle (option amg_tail, csrc/amg_tail.hip) costs and buys on one MI355X.

    python tools/amg_tail_bench.py [--cases square_nb,step,box64,box128,cavity128,box256] [--degrees 1,2]
                                   [--parent-root DIR] [--parent-rounds 3] [--solves] [--out profiles/NAME.json]

The cycle: microseconds per storm_hip_amg_apply between one HIP-event pair, on r = sin(0.37 i).  Arms: the launches
(amg_tail = 0) and, for every level size of the case, the tail that starts at that level (amg_tail = 1, amg_tail_rows = the
level's rows), the arms ALTERNATING apply by apply, the median of 30 after 3 warm-up rounds; every tail arm's z is compared
with the launches' bit for bit.  --parent-root DIR (a built checkout of the parent commit): the same apply on THAT build, a
fresh process per round (3 + 30 applies, its median), the median of the rounds -- the reference arm; without it the
reference is marked NOT MEASURED and this build's own launches stand in.

Cases: the Triangle meshes tests/golden/mesh/square_nb.1 and step.1 (A = I - L: definite whatever the boundary), the 64^3,
128^3 and 256^3 Poisson boxes (A = -L, Dirichlet walls), the 128^3 box without walls as a null-space object (the cavity's
pressure operator).  All on fp64 records, Chebyshev smoother of every --degrees.

--solves: CG to 1e-6 on step.1, plain against multigrid with the tail off and on (host clock between two context syncs, the
arms alternating, the median of 5).

The default of amg_tail_rows is the largest level size at which no measured case is more than 3 % (the box-to-box spread)
slower than its launches; the bar for turning amg_tail on by default is more than 6 % below the PARENT's cycle on both
Triangle meshes and at 128^3 and within 3 % of it at 256^3.  Prints and writes one JSON document; not a pass / fail."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM, TIMED = 3, 30


def make_case(api, mesh, ctx, name):
    """(matrix, alpha, beta, preconditioner keywords)."""
    ctx.set_option("spmv_dict", 0)
    try:
        if name in ("square_nb", "step"):
            from stormruler_amd import io_tetgen

            g = io_tetgen.read_triangle(os.path.join(ROOT, "tests", "golden", "mesh", name + ".1."))
            return api.StencilMatrix.from_face_graph(ctx, g), -1.0, 1.0, dict(coarse_rows=32)
        if name.startswith("box"):
            return api.StencilMatrix.from_face_graph(ctx, mesh.structured_box(int(name[3:]))), -1.0, 0.0, {}
        assert name.startswith("cavity"), name
        g = mesh.structured_box(int(name[6:]), dirichlet=False)
        return api.StencilMatrix.from_face_graph(ctx, g), -1.0, 0.0, dict(nullspace="constant")
    finally:
        ctx.set_option("spmv_dict", 4)


def build_pre(api, ctx, mat, alpha, beta, degree, kw):
    pre = api.AmgPreconditioner(smoother_degree=degree, **kw)
    n = mat.stats()["n_rows"]
    v = api.DeviceVector(ctx, n)
    pre.build(v, v, api.HipStencilOperator(mat, alpha, beta))
    return pre, n


def timed_apply(ctx, pre, z, r):
    ctx.timer_start()
    pre.mul(z, r)
    return 1e3 * ctx.timer_stop()  # microseconds


def child(args) -> int:
    """The reference arm: this process imports the package of --package-root and knows no amg_tail option."""
    from stormruler_amd import api, mesh

    ctx = api.Context(0)
    mat, alpha, beta, kw = make_case(api, mesh, ctx, args.case)
    pre, n = build_pre(api, ctx, mat, alpha, beta, args.degree, kw)
    r, z = api.DeviceVector.from_numpy(ctx, np.sin(0.37 * np.arange(n))), api.DeviceVector(ctx, n)
    us = [timed_apply(ctx, pre, z, r) for _ in range(WARM + TIMED)][WARM:]
    print(json.dumps({"us_median": float(np.median(us)), "z_norm2": float(np.linalg.norm(z.to_numpy())),
                      "level_rows": pre.hierarchy.level_rows()}), flush=True)
    pre.close(), mat.close(), ctx.close()
    return 0


def cycle_bench(api, mesh, ctx, name, degree, args):
    mat, alpha, beta, kw = make_case(api, mesh, ctx, name)
    pre, n = build_pre(api, ctx, mat, alpha, beta, degree, kw)
    rows = pre.hierarchy.level_rows()
    r, z = api.DeviceVector.from_numpy(ctx, np.sin(0.37 * np.arange(n))), api.DeviceVector(ctx, n)
    arms = [("launches", 0, 0)] + [(f"tail from {m} rows", 1, m) for m in rows[:-1]]
    us = {a[0]: [] for a in arms}
    out, meta = {}, {}
    try:
        for i in range(WARM + TIMED):
            for label, tail, m in arms:
                ctx.set_option("amg_tail", tail)
                ctx.set_option("amg_tail_rows", m)
                t = timed_apply(ctx, pre, z, r)
                if i >= WARM:
                    us[label].append(t)
                if i == 0:
                    out[label] = z.to_numpy()
                    meta[label] = {k: int(pre.get(k)) for k in ("tail_level", "tail_blocks", "tail_barriers")} if tail else {}
    finally:
        ctx.set_option("amg_tail", 0)
    base = float(np.median(us["launches"]))
    doc = {"case": name, "degree": degree, "level_rows": rows, "launches_us_median": base, "arms": []}
    for label, tail, m in arms[1:]:
        med = float(np.median(us[label]))
        doc["arms"].append(dict(arm=label, amg_tail_rows=m, us_median=med, over_launches=med / base, **meta[label],
                                same_bits_as_launches=bool(np.array_equal(out[label].view(np.uint64), out["launches"].view(np.uint64)))))
    if args.parent_root:
        rounds = []
        for _ in range(args.parent_rounds):
            o = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--package-root", args.parent_root, "--case", name,
                                "--degree", str(degree)], check=True, capture_output=True, text=True, timeout=900).stdout
            rounds.append(json.loads(o.strip().splitlines()[-1]))
        ref = float(np.median([p["us_median"] for p in rounds]))
        doc["parent"] = {"us_median": ref, "rounds": [p["us_median"] for p in rounds], "launches_over_parent": base / ref,
                         "same_z_norm2": bool(rounds[0]["z_norm2"] == float(np.linalg.norm(out["launches"])))}
        for a in doc["arms"]:
            a["over_parent"] = a["us_median"] / ref
    else:
        doc["parent"] = "NOT MEASURED"
    pre.close(), mat.close()
    return doc


def solve_bench(api, mesh, ctx, repeats=5):
    mat, alpha, beta, kw = make_case(api, mesh, ctx, "step")
    pre, n = build_pre(api, ctx, mat, alpha, beta, 2, kw)
    op = api.HipStencilOperator(mat, alpha, beta)
    b, x = api.DeviceVector.from_numpy(ctx, np.ones(n)), api.DeviceVector(ctx, n)

    class Built(type(pre)):  # (a solver builds its preconditioner before every solve: this one is built)
        def build(self, *a):
            pass

    pre.__class__ = Built
    arms = [("cg plain", None, 0), ("cg + multigrid, launches", pre, 0), ("cg + multigrid, tail", pre, 1)]
    ms, info = {a[0]: [] for a in arms}, {}
    try:
        for rnd in range(repeats + 1):
            for label, p, tail in arms:
                ctx.set_option("amg_tail", tail)
                ctx.set_option("amg_tail_rows", 1 << 40)
                s = api.CgSolver()
                s.pre_op, s.relative_error_tolerance = p, 1e-6
                api.fill_with(x, 0.0)
                ctx.sync()
                t0 = time.perf_counter()
                ok = s.solve(x, b, op)
                ctx.sync()
                if rnd > 0:
                    ms[label].append(1e3 * (time.perf_counter() - t0))
                info[label] = {"converged": bool(ok), "iterations": int(s.iteration), "x_norm2": float(np.linalg.norm(x.to_numpy()))}
    finally:
        ctx.set_option("amg_tail", 0)
    doc = {"case": "step.1, CG to 1e-6, b = 1", "rows": n, "level_rows": pre.hierarchy.level_rows(),
           "arms": [dict(arm=label, wall_ms_median=float(np.median(ms[label])), **info[label]) for label, _, _ in arms]}
    pre.close(), mat.close()
    return doc


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="square_nb,step,box64,box128,cavity128,box256")
    ap.add_argument("--degrees", default="1,2")
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--parent-rounds", type=int, default=3)
    ap.add_argument("--package-root", default=ROOT)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--case", default="box64")
    ap.add_argument("--degree", type=int, default=2)
    ap.add_argument("--solves", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))
    if args.child:
        return child(args)

    from stormruler_amd import api, mesh

    ctx = api.Context(0)
    doc = {"device": ctx.info()["name"],
           "method": f"cycle: one HIP-event pair per apply, arms alternating, median of {TIMED} after {WARM}; parent: a fresh process "
                     f"per round, median of {args.parent_rounds} rounds' medians",
           "cycles": [], "solves": "NOT MEASURED",
           "cavity pressure solve, 15 steps (tools/cavity_amg_bench.py)": "NOT MEASURED"}
    for name in [c for c in args.cases.split(",") if c]:
        for degree in [int(d) for d in args.degrees.split(",") if d]:
            row = cycle_bench(api, mesh, ctx, name, degree, args)
            print(json.dumps(row), flush=True)
            doc["cycles"].append(row)
    if args.solves:
        doc["solves"] = solve_bench(api, mesh, ctx)
        print(json.dumps(doc["solves"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
