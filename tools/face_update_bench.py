#!/usr/bin/env python3
"""What a device-side refresh of an operator's face weights costs (one MI355X).

    python tools/face_update_bench.py [--n 256] [--tet-edge 128] [--repeats 30] [--out profiles/NAME.json]

On the n^3 box with convection-diffusion weights and on the 6 * tet_edge^3-cell tetrahedral box that bench.py generates
(Morton order), for an operator created by ``StencilMatrix.from_face_weights_updatable``:

  refresh         ``set_face_weights`` (op_refresh_sell_kernel + op_refresh_tail_kernel where there is a tail): one HIP-event
                  pair per call on the library's stream, two weight sets (two velocities) alternating, the median of
                  `repeats` calls after a warm-up;
  apply           ``apply`` of the same operator in the same run, timed the same way: the yardstick;
  cells_to_faces  both outputs, timed the same way;
  host rebuild    the only road without this feature: a fresh ``from_face_weights`` from host arrays, host clock, ending in
                  a context synchronisation, the median of 3;
  bitwise_equal   at the timed size: the apply after a refresh against the apply of a fresh operator.

The refresh is reported as a fraction of the 8 TB/s peak on the bytes the algorithm streams -- per ELL slot 4 (source id)
+ 8 (gathered weight) + 8 (stored weight), per row 16 (diag_extra read, ext stored), per tail entry 20 -- and as a
multiple of the apply's time.  Prints and writes one JSON document.  Not a pass / fail: tests/test_gpu_face_update.py
holds the results."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_BYTES_PER_S = 8.0e12
NU, VEL_A, VEL_B = 1e-2, (1.0, 0.5, 0.25), (-0.3, 0.8, 0.6)


def timed(ctx, call, repeats, warmup=4):
    ms = []
    for i in range(warmup + repeats):
        ctx.timer_start()
        call(i)
        t = ctx.timer_stop()
        if i >= warmup:
            ms.append(t)
    a = np.array(ms)
    return {"us_median": 1e3 * float(np.median(a)), "us_min": 1e3 * float(a.min()), "us_max": 1e3 * float(a.max()), "calls": repeats}


def measure(api, mesh, ctx, g, repeats):
    n, f = g.n_cells, g.n_faces
    sets = [mesh.convection_diffusion_weights(g, NU, v) for v in (VEL_A, VEL_B)]
    mat = api.StencilMatrix.from_face_weights_updatable(ctx, n, g.n_halo, g.inner, g.outer, *sets[0])
    st = mat.stats()
    dev = [tuple(api.DeviceVector.from_numpy(ctx, a) for a in s) for s in sets]
    out = {"rows": n, "faces": f, "ell_slots": st["ell_slots"], "mean_width": st["ell_slots"] / n, "tail_nnz": st["tail_nnz"],
           "record_bytes": st["record_bytes"], "device_bytes": st["device_bytes"]}
    streamed = 20 * st["ell_slots"] + 16 * n + 20 * st["tail_nnz"]
    out["refresh_streamed_bytes"] = streamed
    out["refresh"] = timed(ctx, lambda i: mat.set_face_weights(*dev[(i + 1) % 2]), repeats)
    x = api.DeviceVector.from_numpy(ctx, np.sin(0.37 * np.arange(n)) + 0.25)
    y = api.DeviceVector(ctx, n)
    out["apply"] = timed(ctx, lambda i: mat.apply(1.0, 0.0, x, y), repeats)
    ai, ao = api.DeviceVector(ctx, f), api.DeviceVector(ctx, f)
    out["cells_to_faces"] = timed(ctx, lambda i: mat.cells_to_faces(x, ai, ao), repeats)
    out["refresh_fraction_of_peak"] = streamed / (out["refresh"]["us_median"] * 1e-6) / PEAK_BYTES_PER_S
    out["refresh_GBs"] = streamed / (out["refresh"]["us_median"] * 1e-6) / 1e9
    out["refresh_over_apply"] = out["refresh"]["us_median"] / out["apply"]["us_median"]
    out["refresh_over_apply_by_bytes"] = streamed / (st["record_bytes"] + 16 * n)
    # the road without the feature: a fresh operator from host arrays (and the one to compare bits with)
    walls, fresh = [], None
    for _ in range(3):
        if fresh is not None:
            fresh.close()
        ctx.sync()
        t0 = time.perf_counter()
        fresh = api.StencilMatrix.from_face_weights(ctx, n, g.n_halo, g.inner, g.outer, *sets[1])
        ctx.sync()
        walls.append(time.perf_counter() - t0)
    out["host_rebuild_ms_median"] = 1e3 * float(np.median(walls))
    out["host_rebuild_over_refresh"] = out["host_rebuild_ms_median"] * 1e3 / out["refresh"]["us_median"]
    mat.set_face_weights(*dev[1])
    mat.apply(1.0, 0.0, x, y)
    y2 = api.DeviceVector(ctx, n)
    fresh.apply(1.0, 0.0, x, y2)
    out["bitwise_equal"] = bool(np.array_equal(y.to_numpy().view(np.uint64), y2.to_numpy().view(np.uint64)))
    mat.cells_to_faces(x, ai, ao)
    xh = x.to_numpy()
    out["cells_to_faces_equal"] = bool(np.array_equal(ai.to_numpy(), xh[g.inner]) and np.array_equal(ao.to_numpy(), xh[g.outer]))
    fresh.close()
    mat.close()
    print(json.dumps(out), flush=True)
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256, help="edge of the box (0: skip it)")
    ap.add_argument("--tet-edge", type=int, default=128, help="cubes per edge of the tetrahedral box (0: skip it)")
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from stormruler_amd import api, host_mesh, io_tetgen, mesh

    ctx = api.Context(0)
    doc = {"device": ctx.info()["name"], "peak_bytes_per_s": PEAK_BYTES_PER_S,
           "method": "HIP-event pair per call on the library's stream, median after 4 warm-up calls, weight sets alternating; "
                     "host rebuild: host clock between context syncs, median of 3"}

    def save():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(doc, f, indent=1)

    if args.n > 0:
        doc["box"] = dict(n=args.n, **measure(api, mesh, ctx, mesh.structured_box(args.n), args.repeats))
        save()
    if args.tet_edge > 0:
        with tempfile.TemporaryDirectory() as d:
            pos, bf, cells = io_tetgen.tet_box(args.tet_edge)
            prefix = os.path.join(d, "tetbox.1")
            host_mesh.write_tetgen(prefix, pos, bf, np.ones(len(bf), np.int64), cells)
            del pos, bf, cells
            hm = host_mesh.HostMesh.read_tetgen(prefix + ".", 3)
        assert hm.order_cells("morton") == "morton"
        g = hm.face_graph()
        hm.close()
        doc["tetrahedra"] = dict(edge=args.tet_edge, **measure(api, mesh, ctx, g, args.repeats))
        save()
    print(json.dumps(doc), flush=True)
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
