#!/usr/bin/env python3
"""What the smoothed-aggregation multigrid preconditioner buys a CG solve on one MI355X.

    python tools/amg_bench.py [--n 256] [--repeats 3] [--cycles 20] [--out profiles/NAME.json]

The n^3 box as a face-weight operator on fp64 records (option spmv_dict = 0), A = -M, right-hand side 1, CG to 1e-6.
Arms: plain (the fused CG loop), Chebyshev degree 2 on reduced records, AMG with smoothers of degree 1 and 2, each with
fp64 and with fp32-weight (reduced) smoother records.  Every preconditioner is built ONCE, outside the timed solves;
its setup is reported on its own.  Wall clock of a solve between two context synchronisations, the arms ALTERNATING
round by round, the median of `repeats` rounds after one warm-up round.
Per arm: iterations, fine-level operator products (applies + per preconditioner apply: the polynomial's degree, or for a
V-cycle 2 x degree smoother products + 2 residuals) and ms.  For the AMG arms also: host setup and upload seconds, the
number of solves after which the setup is paid back against the best other arm, microseconds per V-cycle (one HIP-event
pair per apply, the median of `cycles`) against the bytes the algorithm moves on the FINE level times the operator
complexity (a floor: the transfers are not in it), device bytes, level sizes, operator complexity, transfer padding.
Prints and writes one JSON document.  Not a pass / fail: tests/test_gpu_amg.py holds the results."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def prebuilt(cls, *args, **kw):
    """An instance of a preconditioner class whose build() runs once (a solver calls it before every solve)."""

    class Once(cls):
        built = False

        def build(self, x_vec, b_vec, any_op):
            if not self.built:
                super().build(x_vec, b_vec, any_op)
                self.built = True

    return Once(*args, **kw)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cycles", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from stormruler_amd import api, mesh

    ctx = api.Context(0)
    g = mesh.structured_box(args.n)
    coef, b_coef = mesh.face_coefficients(g)
    ext = np.zeros(g.n_total)
    np.add.at(ext, g.b_cell, -b_coef / g.volume[g.b_cell])
    ctx.set_option("spmv_dict", 0)
    mat = api.StencilMatrix.from_face_weights(ctx, g.n_cells, 0, g.inner, g.outer, coef / g.volume[g.inner],
                                              coef / g.volume[g.outer], ext[: g.n_cells])
    ctx.set_option("spmv_dict", 4)
    n = g.n_cells
    del g, coef, b_coef, ext
    st = mat.stats()
    rec = st["record_bytes"] / n
    op = api.HipStencilOperator(mat, -1.0, 0.0)
    b, x = api.DeviceVector.from_numpy(ctx, np.ones(n)), api.DeviceVector(ctx, n)
    doc = {"device": ctx.info()["name"], "n": args.n, "rows": n, "record_bytes_per_row": rec,
           "method": "solve: host clock between context syncs, arms alternating, median; V-cycle: HIP-event pair per apply, median"}

    arms = [("plain", None, 0), ("chebyshev degree 2, reduced records",
                                 prebuilt(api.ChebyshevPreconditioner, degree=2, reduced_records=True), 2)]
    for degree in (1, 2):
        for reduced in (False, True):
            arms.append((f"amg degree {degree}" + (", reduced records" if reduced else ""),
                         prebuilt(api.AmgPreconditioner, smoother_degree=degree, reduced_records=reduced), 2 * degree + 2))
    setup = {}
    for name, pre, _ in arms:  # build, outside the timed solves
        if pre is None:
            continue
        ctx.sync()
        t0 = time.perf_counter()
        pre.build(x, b, op)
        ctx.sync()
        setup[name] = time.perf_counter() - t0
        print(json.dumps({"built": name, "seconds": setup[name]}), flush=True)

    times = {name: [] for name, _, _ in arms}
    info = {}
    for rnd in range(args.repeats + 1):
        for name, pre, products in arms:
            s = api.CgSolver()
            s.pre_op = pre
            api.fill_with(x, 0.0)
            ctx.sync()
            t0 = time.perf_counter()
            ok = s.solve(x, b, op)
            ctx.sync()
            dt = time.perf_counter() - t0
            if rnd > 0:
                times[name].append(dt)
            info[name] = {"converged": bool(ok), "iterations": int(s.iteration), "pre_applies": int(s.num_pre_applies),
                          "fine_level_products": int(s.num_applies + products * s.num_pre_applies),
                          "relative_error": float(s.relative_error)}
    rows = []
    for name, pre, _ in arms:
        t = times[name]
        row = dict(arm=name, **info[name], wall_ms_median=1e3 * float(np.median(t)), wall_ms_min=1e3 * float(min(t)),
                   wall_ms_max=1e3 * float(max(t)))
        if pre is not None:
            row["build_seconds_total"] = setup[name]
        rows.append(row)
    best_other = min(r["wall_ms_median"] for r in rows if not r["arm"].startswith("amg"))
    r_vec, z_vec = api.DeviceVector.from_numpy(ctx, np.sin(0.37 * np.arange(n)) + 0.25), api.DeviceVector(ctx, n)
    for row, (name, pre, _) in zip(rows, arms):
        if not name.startswith("amg"):
            continue
        degree = int(pre.get("smoother_degree"))
        ms = []
        for i in range(args.cycles + 3):
            ctx.timer_start()
            pre.mul(z_vec, r_vec)
            t = ctx.timer_stop()
            if i >= 3:
                ms.append(t)
        srec = rec if not pre.reduced_records else (256 + 512 * (rec * 64 - 512) / 768) / 64
        fine = 2 * (24 + degree * (srec + 56)) + 2 * (rec + 24)  # two smoother applies (d_0, then the steps), two residuals
        oc = pre.get("operator_complexity")
        gain = best_other - row["wall_ms_median"]
        row.update(host_setup_seconds=pre.get("setup_seconds"), upload_seconds=pre.get("upload_seconds"),
                   solves_to_pay_back_setup=(1e3 * (pre.get("setup_seconds") + pre.get("upload_seconds")) / gain) if gain > 0 else None,
                   vcycle_us_median=1e3 * float(np.median(ms)), vcycle_algorithmic_bytes_floor=float(fine * n * oc),
                   vcycle_floor_tb_per_s=float(fine * n * oc / (1e-3 * np.median(ms)) / 1e12),
                   device_bytes=int(pre.get("device_bytes")), level_rows=pre.hierarchy.level_rows(), operator_complexity=oc,
                   grid_complexity=pre.get("grid_complexity"), transfer_padding=pre.get("transfer_padding"),
                   faster_than_best_other_arm=1.0 - row["wall_ms_median"] / best_other)
    for row in rows:
        print(json.dumps(row), flush=True)
    doc["cg"] = rows
    doc["best_other_arm_ms"] = best_other
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
    for _, pre, _ in arms:
        if pre is not None:
            pre.close()
    mat.close()
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
