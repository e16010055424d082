#!/usr/bin/env python3
"""What the multigrid preconditioner's Jacobi smoother buys BASELINE config 4 on one MI355X, and what its fused sweep costs.

    python tools/amg_jacobi_bench.py [--n 128] [--repeats 3] [--parent-root DIR] [--sweep-sizes 128,256] [--out profiles/NAME.json]

Solves: A = -nu L + C(v) (first-order upwind, nu = 1e-2, v = (1, 0.5, 0.25)) on the n^3 box as a face-weight operator on
fp64 records (option spmv_dict = 0), b = 1, to 1e-6.  Arms: GMRES(30) and BiCGStab, each plain -- on the default records, as
BASELINE config 4 builds the operator, and on fp64 records -- and right-preconditioned by the multigrid cycle with 1 and 2
Jacobi sweeps (fp64 records: what the hierarchy reads).  Every preconditioner is built ONCE, outside the timed solves; its setup is
reported on its own.  Wall clock of a solve between two context synchronisations, the arms ALTERNATING round by round, the
median of `repeats` rounds after one warm-up round.  --parent-root DIR (a built checkout of the parent commit): every round
also runs plain GMRES(30) on THAT build, in a fresh process (one warm-up solve, one timed solve, per record format); its
default-record solve is the reference arm, and a multigrid arm is called faster only if it is more than 6 % below it.

The sweep: microseconds per fused sweep (amg_jacobi_sweep_kernel, option amg_fused = 1) against the four statements
(amg_fused = 0) of storm_hip_amg_smooth on level 0 of the box of every --sweep-sizes edge, one HIP-event pair per sweep,
the two arms alternating sweep by sweep, the median of 30; beside it the ratio of the bytes per row each moves (records + 32
against records + 88).

--plain-only --package-root DIR: the child's run (imports stormruler_amd from DIR, plain GMRES(30) only).
Prints and writes one JSON document.  Not a pass / fail: tests/test_gpu_amg_jacobi.py holds the results."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NU, VEL = 1e-2, (1.0, 0.5, 0.25)


def prebuilt(cls, *args, **kw):
    """An instance of a preconditioner class whose build() runs once (a solver calls it before every solve)."""

    class Once(cls):
        built = False

        def build(self, x_vec, b_vec, any_op):
            if not self.built:
                super().build(x_vec, b_vec, any_op)
                self.built = True

    return Once(*args, **kw)


def box_operator(api, mesh, ctx, n, default_records=False):
    """(fp64-record matrix, rows), or with default_records (fp64-record matrix, default-record matrix, rows): the default
    records are what BASELINE config 4 and bench.py build."""
    g = mesh.structured_box(n)
    wi, wo, de = mesh.convection_diffusion_weights(g, NU, VEL)
    ctx.set_option("spmv_dict", 0)
    try:
        mat = api.StencilMatrix.from_face_weights(ctx, g.n_cells, 0, g.inner, g.outer, wi, wo, de)
    finally:
        ctx.set_option("spmv_dict", 4)
    if not default_records:
        return mat, g.n_cells
    return mat, api.StencilMatrix.from_face_weights(ctx, g.n_cells, 0, g.inner, g.outer, wi, wo, de), g.n_cells


def timed_solve(api, ctx, kind, pre, x, b, op):
    s = api.GmresSolver() if kind == "gmres" else api.BiCgStabSolver()
    if kind == "gmres":
        s.num_inner_iterations = 30
    s.pre_op = pre
    api.fill_with(x, 0.0)
    ctx.sync()
    t0 = time.perf_counter()
    ok = s.solve(x, b, op)
    ctx.sync()
    dt = time.perf_counter() - t0
    return dt, {"converged": bool(ok), "iterations": int(s.iteration), "pre_applies": int(s.num_pre_applies),
                "relative_error": float(s.relative_error)}


def plain_only(args) -> int:
    from stormruler_amd import api, mesh

    ctx = api.Context(0)
    mat, mat_default, n = box_operator(api, mesh, ctx, args.n, True)
    b, x = api.DeviceVector.from_numpy(ctx, np.ones(n)), api.DeviceVector(ctx, n)
    out = {}
    for name, m in (("default records", mat_default), ("fp64 records", mat)):
        op = api.HipStencilOperator(m, 1.0, 0.0)
        timed_solve(api, ctx, "gmres", None, x, b, op)  # warm-up
        dt, info = timed_solve(api, ctx, "gmres", None, x, b, op)
        out[name] = dict(info, wall_ms=1e3 * dt, x_norm2=float(np.linalg.norm(x.to_numpy())))
    print(json.dumps(out), flush=True)
    mat.close(), mat_default.close()
    ctx.close()
    return 0


def sweep_bench(api, mesh, ctx, n, pre=None, mat=None):
    own = pre is None
    if own:
        mat, rows = box_operator(api, mesh, ctx, n)
        pre = api.AmgPreconditioner(smoother="jacobi", jacobi_sweeps=1)
        v = api.DeviceVector(ctx, rows)
        pre.build(v, v, api.HipStencilOperator(mat, 1.0, 0.0))
    rows = mat.stats()["n_rows"]
    rec = mat.stats()["record_bytes"] / rows
    r = api.DeviceVector.from_numpy(ctx, np.sin(0.37 * np.arange(rows)) + 0.25)
    z_in = api.DeviceVector.from_numpy(ctx, np.cos(0.11 * np.arange(rows)))
    z_out = api.DeviceVector(ctx, rows)
    ms = {1: [], 0: []}
    out = {}
    try:
        for i in range(33):
            for fused in (1, 0):
                ctx.set_option("amg_fused", fused)
                ctx.timer_start()
                pre.smooth(0, r, z_in, z_out)
                t = ctx.timer_stop()
                if i >= 3:
                    ms[fused].append(t)
                if i == 0:
                    out[fused] = z_out.to_numpy()
    finally:
        ctx.set_option("amg_fused", 1)
    row = {"n": n, "rows": rows, "record_bytes_per_row": rec, "fused_us_median": 1e3 * float(np.median(ms[1])),
           "statements_us_median": 1e3 * float(np.median(ms[0])),
           "speedup": float(np.median(ms[0]) / np.median(ms[1])), "ratio_of_bytes": (rec + 88.0) / (rec + 32.0),
           "fused_tb_per_s": float((rec + 32.0) * rows / (1e-3 * np.median(ms[1])) / 1e12),
           "same_bits_at_this_size": bool(np.array_equal(out[1].view(np.uint64), out[0].view(np.uint64)))}
    if own:
        pre.close()
        mat.close()
    return row


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--package-root", default=ROOT)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--sweep-sizes", default="128,256")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))
    if args.plain_only:
        return plain_only(args)

    from stormruler_amd import api, mesh

    ctx = api.Context(0)
    mat, mat_default, n = box_operator(api, mesh, ctx, args.n, True)
    op, op_default = api.HipStencilOperator(mat, 1.0, 0.0), api.HipStencilOperator(mat_default, 1.0, 0.0)
    b, x = api.DeviceVector.from_numpy(ctx, np.ones(n)), api.DeviceVector(ctx, n)
    doc = {"device": ctx.info()["name"], "n": args.n, "rows": n, "record_bytes_per_row": mat.stats()["record_bytes"] / n,
           "default_record_bytes_per_row": mat_default.stats()["record_bytes"] / n,
           "method": "solve: host clock between context syncs, arms alternating, median; sweep: HIP-event pair per sweep, "
                     "arms alternating, median of 30"}
    pres = {1: prebuilt(api.AmgPreconditioner, smoother="jacobi", jacobi_sweeps=1),
            2: prebuilt(api.AmgPreconditioner, smoother="jacobi", jacobi_sweeps=2)}
    setup = {}
    for sweeps, pre in pres.items():
        ctx.sync()
        t0 = time.perf_counter()
        pre.build(x, b, op)
        ctx.sync()
        setup[sweeps] = time.perf_counter() - t0
        print(json.dumps({"built": f"{sweeps} sweeps", "seconds": setup[sweeps]}), flush=True)
    # (arm, method, preconditioner, sweeps, the solve's operator); "default records": what BASELINE config 4 builds
    arms = []
    for kind in ("gmres", "bicgstab"):
        arms.append((f"{kind} plain, default records", kind, None, 0, op_default))
        arms.append((f"{kind} plain, fp64 records", kind, None, 0, op))
        for sweeps in (1, 2):
            arms.append((f"{kind} + multigrid, {sweeps} Jacobi sweep{'s' if sweeps > 1 else ''}, right, fp64 records", kind,
                         pres[sweeps], sweeps, op))
    times = {name: [] for name, *_ in arms}
    info, parent = {}, []
    for rnd in range(args.repeats + 1):
        for name, kind, pre, _, the_op in arms:
            dt, info[name] = timed_solve(api, ctx, kind, pre, x, b, the_op)
            if rnd > 0:
                times[name].append(dt)
            if pre is None:
                info[name]["x_norm2"] = float(np.linalg.norm(x.to_numpy()))
        if args.parent_root and rnd > 0:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--plain-only", "--package-root", args.parent_root,
                                  "--n", str(args.n)], check=True, capture_output=True, text=True, timeout=600).stdout
            parent.append(json.loads(out.strip().splitlines()[-1]))
            print(json.dumps({"parent round": rnd, **parent[-1]}), flush=True)
    rows = []
    for name, kind, pre, sweeps, _ in arms:
        t = times[name]
        row = dict(arm=name, **info[name], wall_ms_median=1e3 * float(np.median(t)), wall_ms_min=1e3 * float(min(t)),
                   wall_ms_max=1e3 * float(max(t)))
        if pre is not None:
            row.update(build_seconds_total=setup[sweeps], host_setup_seconds=pre.get("setup_seconds"),
                       upload_seconds=pre.get("upload_seconds"), device_bytes=int(pre.get("device_bytes")),
                       level_rows=pre.hierarchy.level_rows(), operator_complexity=pre.get("operator_complexity"),
                       jacobi_sigma_0=pre.get("jacobi_sigma_0"))
        rows.append(row)
    own_plain = rows[0]["wall_ms_median"]
    if parent:
        ref = float(np.median([p["default records"]["wall_ms"] for p in parent]))
        ref64 = float(np.median([p["fp64 records"]["wall_ms"] for p in parent]))
        doc["reference"] = {"arm": "gmres plain, default records, on the parent commit's build (a fresh process per round)",
                            "wall_ms_median": ref, "fp64_records_wall_ms_median": ref64, "rounds": parent,
                            "this_build_plain_over_parent": own_plain / ref,
                            "this_build_plain_fp64_over_parent": rows[1]["wall_ms_median"] / ref64,
                            "same_iterations": [parent[0][k]["iterations"] == r["iterations"]
                                                for k, r in (("default records", rows[0]), ("fp64 records", rows[1]))],
                            "same_x_norm2": [parent[0][k]["x_norm2"] == r["x_norm2"]
                                             for k, r in (("default records", rows[0]), ("fp64 records", rows[1]))]}
    else:
        ref = own_plain
        doc["reference"] = {"arm": "NOT MEASURED on the parent commit's build; this build's own gmres plain, default records",
                            "wall_ms_median": ref}
    for row in rows:
        row["below_reference"] = 1.0 - row["wall_ms_median"] / ref
        row["faster_by_the_bar_of_6_percent"] = bool(row["below_reference"] > 0.06) if "multigrid" in row["arm"] else None
        print(json.dumps(row), flush=True)
    doc["solves"] = rows
    doc["sweep"] = []
    for edge in [int(s) for s in args.sweep_sizes.split(",") if s]:
        if edge == args.n:
            row = sweep_bench(api, mesh, ctx, edge, pres[1], mat)
        else:
            for pre in pres.values():  # (room for the larger box)
                pre.close()
            row = sweep_bench(api, mesh, ctx, edge)
        print(json.dumps(row), flush=True)
        doc["sweep"].append(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
    for pre in pres.values():
        pre.close()
    mat.close(), mat_default.close()
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
