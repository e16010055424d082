#!/usr/bin/env python3
"""What reading the operator's records once for k columns buys: the block apply and the batched CG against their
one-column counterparts in the same process (storm_hip_op_apply and storm_hip_solve_cg, the baseline).

    python tools/block_bench.py [--n 256] [--tet-edge 128] [--launches 60] [--cg-iterations 40] [--out profiles/NAME.json]

On the n^3 box with fp64 records (option spmv_dict = 0: what any real mesh gets) and on the 6 * tet_edge^3-cell
tetrahedral box (Z-order numbering), after a warm-up:
  * mul_block for k = 2, 4, 8: one HIP-event pair per launch on the library's compute stream, the median of `launches`
    launches rotating over three (X, Y) pairs (every launch finds its vectors evicted from the Infinity Cache) -- against
    k back-to-back storm_hip_op_apply launches on three (x, y) pairs, one event pair around the k of them.  Priced by the
    bytes moved: records + 16 k per row (on the box 96 + 16 k), as a fraction of the 8 TB/s peak;
  * BlockCgSolver for k = 4 at a fixed number of iterations (both tolerances 0), per column-iteration -- against four
    CgSolver solves with latency_path = 0.
Prints and writes one JSON document.  Not a pass / fail: tests/test_gpu_block.py holds the results to the bit."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK_GBS = 8000.0


def timed(ctx, fn, launches, warmup=6):
    for i in range(warmup):
        fn(i)
    ms = []
    for i in range(launches):
        ctx.timer_start()
        fn(i)
        ms.append(ctx.timer_stop())
    ms = np.array(ms)
    return {"launches": launches, "median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max())}


def apply_rates(api, ctx, mat, launches):
    st = mat.stats()
    n = st["n_rows"]
    rec = st["record_bytes"] / n
    op = api.HipStencilOperator(mat, -1.0, 0.0)
    x = np.sin(0.37 * np.arange(n))
    out = {"rows": n, "record_bytes_per_row": rec, "tail_rows": st["tail_rows"]}
    xs = [api.DeviceVector.from_numpy(ctx, x) for _ in range(3)]
    ys = [api.DeviceVector(ctx, n) for _ in range(3)]
    single = timed(ctx, lambda i: op.mul(ys[i % 3], xs[i % 3]), launches)
    single["bytes_per_row"] = rec + 16
    single["frac_of_peak"] = (rec + 16) * n / (single["median_ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS
    out["single_apply"] = single
    for k in (2, 4, 8):
        host = np.stack([np.sin(0.37 * (j + 1) * np.arange(n)) for j in range(k)], axis=1)
        X = [api.BlockVector.from_numpy(ctx, host) for _ in range(3)]
        Y = [api.BlockVector(ctx, n, k) for _ in range(3)]
        blk = timed(ctx, lambda i: op.mul_block(Y[i % 3], X[i % 3]), launches)

        def k_singles(i):
            for j in range(k):
                op.mul(ys[(i + j) % 3], xs[(i + j) % 3])

        sing = timed(ctx, k_singles, launches)
        by = rec + 16 * k
        out[f"k{k}"] = {"mul_block": blk, "k_single_applies": sing, "bytes_per_row": by,
                        "bytes_per_row_k_singles": k * (rec + 16), "model_speedup_by_bytes": k * (rec + 16) / by,
                        "frac_of_peak": by * n / (blk["median_ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS,
                        "speedup_over_k_single_applies": sing["median_ms"] / blk["median_ms"]}
        del X, Y
    return out


def cg_rates(api, ctx, mat, iterations, repeats=3):
    n, k = mat.stats()["n_rows"], 4
    op = api.HipStencilOperator(mat, -1.0, 0.0)
    host = np.stack([np.sin(0.37 * (j + 1) * np.arange(n)) for j in range(k)], axis=1)
    B = api.BlockVector.from_numpy(ctx, host)
    bs = [api.DeviceVector.from_numpy(ctx, host[:, j]) for j in range(k)]
    x1 = api.DeviceVector(ctx, n)
    X = api.BlockVector(ctx, n, k)
    ctx.set_option("latency_path", 0)

    def block():
        s = api.BlockCgSolver()
        s.num_iterations, s.absolute_error_tolerance, s.relative_error_tolerance = iterations, 0.0, 0.0
        api.fill_with(X, 0.0)
        ctx.sync()
        t0 = time.perf_counter()
        s.solve(X, B, op)
        return time.perf_counter() - t0

    def singles():
        t = 0.0
        for j in range(k):
            s = api.CgSolver()
            s.num_iterations, s.absolute_error_tolerance, s.relative_error_tolerance = iterations, 0.0, 0.0
            api.fill_with(x1, 0.0)
            ctx.sync()
            t0 = time.perf_counter()
            s.solve(x1, bs[j], op)
            t += time.perf_counter() - t0
        return t

    block(), singles()  # warm-up (kernels loaded, work vectors pooled)
    tb = float(np.median([block() for _ in range(repeats)]))
    ts = float(np.median([singles() for _ in range(repeats)]))
    ctx.set_option("latency_path", 1)
    return {"k": k, "iterations": iterations, "repeats": repeats, "block_solve_s": tb, "four_single_solves_s": ts,
            "block_us_per_column_iteration": 1e6 * tb / (k * iterations),
            "single_us_per_column_iteration": 1e6 * ts / (k * iterations), "speedup_over_four_single_solves": ts / tb,
            "throughput_solves": ctx.counter("throughput_solves"), "block_solves": ctx.counter("block_solves")}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--tet-edge", type=int, default=128, help="cubes per edge of the tetrahedral box (0: skip it)")
    ap.add_argument("--launches", type=int, default=60)
    ap.add_argument("--cg-iterations", type=int, default=40)
    ap.add_argument("--out", default=None)
    ap.add_argument("--opt", action="append", default=[], metavar="KEY=VALUE", help="a context option for the whole run (A/B)")
    args = ap.parse_args()

    from stormruler_amd import api, host_mesh, io_tetgen, mesh

    ctx = api.Context(0)
    for kv in args.opt:
        key, value = kv.split("=")
        ctx.set_option(key, int(value))
    doc = {"options": args.opt, "device": ctx.info()["name"], "method": "HIP-event pair per launch, median; three (X, Y) pairs in rotation",
           "hbm_peak_GBs": HBM_PEAK_GBS}

    ctx.set_option("spmv_dict", 0)
    mat = api.StencilMatrix.from_face_graph(ctx, mesh.structured_box(args.n))
    ctx.set_option("spmv_dict", 4)
    doc["box"] = {"n": args.n, "apply": apply_rates(api, ctx, mat, args.launches),
                  "cg": cg_rates(api, ctx, mat, args.cg_iterations)}
    mat.close()
    print(json.dumps({"box": doc["box"]}), flush=True)

    if args.tet_edge > 0:
        with tempfile.TemporaryDirectory() as d:
            pos, bf, cells = io_tetgen.tet_box(args.tet_edge)
            prefix = os.path.join(d, "tetbox.1")
            host_mesh.write_tetgen(prefix, pos, bf, np.ones(len(bf), np.int64), cells)
            del pos, bf, cells
            hm = host_mesh.HostMesh.read_tetgen(prefix + ".", 3)
        assert hm.order_cells("morton") == "morton"
        mat = hm.create_operator(ctx)
        assert mat.stats()["paired_rows"] == 0 and mat.stats()["value_dictionary_size"] == 0
        doc["tetrahedra"] = {"edge": args.tet_edge, "apply": apply_rates(api, ctx, mat, args.launches),
                             "cg": cg_rates(api, ctx, mat, args.cg_iterations)}
        mat.close()
        print(json.dumps({"tetrahedra": doc["tetrahedra"]}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
