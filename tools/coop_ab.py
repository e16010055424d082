#!/usr/bin/env python3
"""A/B of two builds of the library on the cooperative paths (csrc/latency.hip, mgs_chain.hip, resident.hip): one fixed
list of solves, every x, residual history and counter into an .npz; two such files must hold equal arrays.

    STORM_HIP_LIB=/path/to/other/libstorm_hip.so python tools/coop_ab.py --out a.npz     (one fresh process per arm)
    python tools/coop_ab.py --out b.npz
    python tools/coop_ab.py --compare a.npz b.npz                                        (exit code 1 if anything differs)
    python tools/coop_ab.py --speed [runs]      us per iteration, one JSON line per run (alternate the arms by hand)

Every case: tolerances 0; 6 iterations of CG, BiCGStab and two-stage CG; GMRES(6) for 8 inner iterations (a restart, both
parities of k); `latency_path` 2 for the latency cases, `latency_rows` 2^21 while the operator is built.  The sizes are
the smallest that reach each register variant on 256 CUs."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stormruler_amd import api, mesh  # noqa: E402

PLAYGROUND = (-1.0e-4, 2.0, -1.0e-3, 1.0)
NU, VEL = 1e-2, (1.0, 0.5, 0.25)
COUNTERS = ("resident_solves", "latency_solves", "throughput_solves", "engine_solves", "mgs_chain_steps", "mgs_quad_steps")
# (the library's defaults, common.hpp: there is no entry point that reads an option back -- keep the two in step)
OPTIONS = {"latency_path": 1, "latency_cache": 1, "test_disable": 0, "coop_mgs_lds": 1, "coop_mgs_quad": 1, "resident_early": 1}


def box(shape, cubic=False):
    return mesh.structured_box(*shape, lengths=tuple(s / 64.0 for s in shape)) if cubic else mesh.structured_box(*shape)


def poisson(ctx, g):
    return api.StencilMatrix.from_face_graph(ctx, g)


def convdiff(ctx, g):
    wi, wo, de = mesh.convection_diffusion_weights(g, NU, VEL)
    return api.StencilMatrix.from_face_weights(ctx, g.n_cells, g.n_halo, g.inner, g.outer, wi, wo, de)


def triangle(name):
    from stormruler_amd import io_tetgen

    g = io_tetgen.read_triangle(os.path.join(ROOT, "tests", "golden", "mesh", name + "."))
    return mesh.FaceGraph(g.n_cells, 2, g.inner, g.outer, g.area, g.center, g.volume, b_center=np.zeros((0, 2)))


def csr_matrix(ctx, n=4099, per_row=20):
    import scipy.sparse as sp

    rng = np.random.default_rng(23)
    rows = np.repeat(np.arange(n), per_row // 2)
    cols = rng.integers(0, n, rows.size)
    a = sp.coo_matrix((rng.random(rows.size) * 0.1, (rows, cols)), shape=(n, n)).tocsr()
    a = a + a.T
    return api.StencilMatrix.from_csr(ctx, (sp.diags(np.asarray(abs(a).sum(axis=1)).ravel() + 1.0) - a).tocsr())


def solve(ctx, out, name, cls, op, n, iters, inner=None, **options):
    """One solve from x = 0 with the options set for its duration; x, history, iteration and the counters it moved."""
    for key, value in options.items():
        ctx.set_option(key, value)
    s = cls()
    s.num_iterations, s.absolute_error_tolerance, s.relative_error_tolerance, s.record_history = iters, 0.0, 0.0, True
    if inner:
        s.num_inner_iterations = inner
    b = api.DeviceVector.from_numpy(ctx, 1.0 + 0.25 * np.sin(0.01 * np.arange(n)))
    x = api.DeviceVector(ctx, n)
    before = [ctx.counter(k) for k in COUNTERS]
    s.solve(x, b, op)
    for key in options:
        ctx.set_option(key, OPTIONS[key])
    out[name + "/x"] = x.to_numpy()
    out[name + "/history"] = np.asarray(s.history, dtype=np.float64)
    out[name + "/counters"] = np.array([s.iteration, s.path_fallback] + [ctx.counter(k) - v for k, v in zip(COUNTERS, before)],
                                       dtype=np.int64)


def run_cases(ctx):
    out = {}

    def latency_matrix(make):
        ctx.set_option("latency_rows", 1 << 21)
        mat = make()
        ctx.set_option("latency_rows", 1 << 19)
        return mat

    # ---- latency CG, BiCGStab, two-stage CG
    def on(g):
        return lambda: (poisson(ctx, g), g.n_cells)

    lat = [("square_nb.1", on(triangle("square_nb.1")), {}),                      # 3 neighbours: W = 4
           ("box9x7x1", on(box((9, 7, 1))), {}),                                  # ragged last slice
           ("box24", on(box((24, 24, 24))), {}),                                  # W = 8, S = 1
           ("csr4099x20", lambda: (csr_matrix(ctx), 4099), {}),                   # W = 0
           ("box24_nocache", on(box((24, 24, 24))), {"latency_cache": 0}),        # W = 0 on a box
           ("box80", on(box((80, 80, 80))), {}),                                  # S = 2
           ("box100", on(box((100, 100, 100))), {}),                              # S = 4
           ("box128x128x100", on(box((128, 128, 100))), {})]                      # S = 8
    for name, make, options in lat:
        mat, n = latency_matrix(make)
        solve(ctx, out, f"lat/{name}/cg", api.CgSolver, api.HipStencilOperator(mat, -1.0, 0.0), n, 6, latency_path=2, **options)
        solve(ctx, out, f"lat/{name}/bicgstab", api.BiCgStabSolver, api.HipStencilOperator(mat, -1.0, 0.0), n, 6, latency_path=2, **options)
        solve(ctx, out, f"lat/{name}/cg2", api.CgSolver, api.HipTwoStageOperator(mat, *PLAYGROUND), n, 6, latency_path=2, **options)
        mat.close()
    g = box((24, 24, 24))
    mat = latency_matrix(lambda: convdiff(ctx, g))
    for publish, bits in ((1, 0), (0, 16)):  # latency_publish 1 / 0 (test_disable bit 16: write-through stores)
        solve(ctx, out, f"lat/convdiff24/bicgstab_publish{publish}", api.BiCgStabSolver, api.HipStencilOperator(mat, 1.0, 0.0), g.n_cells, 6,
              latency_path=2, test_disable=bits)
    mat.close()

    # ---- the Gram-Schmidt chains: GMRES(6), 8 inner iterations, the convection-diffusion box
    def gmres(name, mat, n, alpha=1.0, **options):
        solve(ctx, out, name, api.GmresSolver, api.HipStencilOperator(mat, alpha, 0.0), n, 8, inner=6, **options)

    for shape in ((7, 5, 3), (80, 80, 80), (100, 100, 100), (128, 128, 100), (128, 128, 130)):  # S = 1, 2, 4, 8, 16
        g = box(shape, cubic=True)
        mat = convdiff(ctx, g)
        gmres("mgs/reg/%dx%dx%d" % shape, mat, g.n_cells, coop_mgs_lds=0, coop_mgs_quad=0)
        mat.close()
    for shape in ((64, 64, 64), (100, 100, 100), (128, 128, 100)):  # SUB = 1, 2, 4
        g = box(shape, cubic=True)
        mat = convdiff(ctx, g)
        gmres("mgs/lds/%dx%dx%d" % shape, mat, g.n_cells, coop_mgs_lds=2, coop_mgs_quad=0)
        mat.close()
    for shape in ((48, 40, 36), (80, 80, 80), (100, 100, 100), (128, 128, 128)):  # S = 1, 2, 4, 8 (128^3 with the apply: LDS prefetch)
        g = box(shape, cubic=True)
        for kind, mat, alpha in (("convdiff", convdiff(ctx, g), 1.0), ("poisson", poisson(ctx, g), -1.0)):
            for bits in (0, 1, 2):  # test_disable: 1 the apply as a launch, 2 no prefetch under the all-reduce
                gmres("mgs/quad/%s/%dx%dx%d/disable%d" % ((kind,) + shape + (bits,)), mat, g.n_cells, alpha, test_disable=bits)
            mat.close()
    g = box((48, 40, 36), cubic=True)
    mat = convdiff(ctx, g)
    gmres("mgs/quad/convdiff/48x40x36/disable512", mat, g.n_cells, test_disable=512)  # the rotations NOT under the norm's all-reduce
    mat.close()

    # ---- the resident paths
    for e in (64, 128):
        g = box((e, e, e))
        mat = poisson(ctx, g)
        op = api.HipStencilOperator(mat, -1.0, 0.0)
        solve(ctx, out, f"res/{e}/cg", api.CgSolver, op, g.n_cells, 6)
        solve(ctx, out, f"res/{e}/bicgstab", api.BiCgStabSolver, op, g.n_cells, 6)
        solve(ctx, out, f"res/{e}/cg_early0", api.CgSolver, op, g.n_cells, 6, resident_early=0)
        solve(ctx, out, f"res/{e}/bicgstab_early0", api.BiCgStabSolver, op, g.n_cells, 6, resident_early=0)
        mat.close()
    return out


def compare(path_a, path_b):
    a, b = np.load(path_a), np.load(path_b)
    bad = sorted(set(a.files) ^ set(b.files))
    for key in sorted(set(a.files) & set(b.files)):
        if not np.array_equal(a[key], b[key]):
            bad.append(key)
    cases = sorted({k.rsplit("/", 1)[0] for k in a.files})
    print(f"{len(cases)} cases, {len(a.files)} arrays, {len(bad)} differ")
    for key in bad:
        print("  DIFFERS:", key)
    names = ("iteration", "path_fallback") + COUNTERS
    for case in cases:
        c = a[case + "/counters"]
        print(" ", case, {n: int(v) for n, v in zip(names, c) if v})
    return 1 if bad else 0


def rate(ctx, cls, op, n, iters, inner=None, **options):
    for key, value in options.items():
        ctx.set_option(key, value)
    b = api.DeviceVector(ctx, n)
    api.fill_with(b, 1.0)
    times = []
    for _ in range(4):  # (the first one warms up)
        s = cls()
        s.num_iterations, s.absolute_error_tolerance, s.relative_error_tolerance = iters, 0.0, 0.0
        if inner:
            s.num_inner_iterations = inner
        x = api.DeviceVector(ctx, n)
        ctx.sync()
        t = time.perf_counter()
        s.solve(x, b, op)
        ctx.sync()
        times.append((time.perf_counter() - t) / iters * 1e6)
    for key in options:
        ctx.set_option(key, OPTIONS[key])
    return round(min(times[1:]), 3)


def speed(ctx, runs):
    g64, g128 = box((64, 64, 64)), box((128, 128, 128))
    p64, p128 = poisson(ctx, g64), poisson(ctx, g128)
    c64, c128 = convdiff(ctx, g64), convdiff(ctx, g128)
    for _ in range(runs):
        line = {"lib": os.environ.get("STORM_HIP_LIB", "tree")}
        for name, cls in (("cg", api.CgSolver), ("bicgstab", api.BiCgStabSolver)):
            line[f"latency64_{name}"] = rate(ctx, cls, api.HipStencilOperator(p64, -1.0, 0.0), g64.n_cells, 400, latency_path=2)
            line[f"resident128_{name}"] = rate(ctx, cls, api.HipStencilOperator(p128, -1.0, 0.0), g128.n_cells, 400)
        line["gmres30_convdiff128"] = rate(ctx, api.GmresSolver, api.HipStencilOperator(c128, 1.0, 0.0), g128.n_cells, 300, inner=30)
        line["gmres30_convdiff64"] = rate(ctx, api.GmresSolver, api.HipStencilOperator(c64, 1.0, 0.0), g64.n_cells, 300, inner=30)
        print(json.dumps(line), flush=True)


def main():
    if len(sys.argv) >= 4 and sys.argv[1] == "--compare":
        return compare(sys.argv[2], sys.argv[3])
    ctx = api.Context(0)
    if len(sys.argv) >= 2 and sys.argv[1] == "--speed":
        speed(ctx, int(sys.argv[2]) if len(sys.argv) > 2 else 1)
    elif len(sys.argv) >= 3 and sys.argv[1] == "--out":
        out = run_cases(ctx)
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
        np.savez(sys.argv[2], **out)
        print(f"{len({k.rsplit('/', 1)[0] for k in out})} cases, {len(out)} arrays -> {sys.argv[2]}")
    else:
        print(__doc__)
        return 2
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
