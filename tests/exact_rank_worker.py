"""Worker of tests/test_gpu_exact_ranks.py: one rank of a W-rank run whose ranks all share device 0.

Launched by torch.distributed.run with the gloo backend.  Every rank builds its z-slab of a UNIT-SPACING nx*ny*(nzl*W)
box (integer stencil coefficients, tests/exact_ref.py) and connects the host-staged transport or, with
STORM_TRANSPORT=ipc, the peer-window transport.  On integer data every all-reduce is exact whatever its order, so each
rank must reproduce the closed forms of the whole box: the global <b,b>, <b,z> and z = A b bitwise, CG's x1 =
fl(fl(rr/pz) * b_local) bitwise, history[0] bitwise and history[1] of CG, BiCGStab and GMRES(30) within the derived
tolerance -- on fp64 records and on format 4 (mixed records on a slab).  CG and BiCGStab also run K = 4 iterations
against the step pins of the whole box (exact_ref.StepPins): history[0..4] on every rank, and on rank 0 the residual of
the x gathered from all ranks (and, on a box of at most 20 000 rows, that x against the exact x_4).  On the host-staged
transport the engine's CGS and TFQMR also run to K = 2 against exact_ref.Pins of the whole box."""
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch.distributed as td  # noqa: E402

import exact_ref as er  # noqa: E402
from stormruler_amd import api, dist, mesh, partition  # noqa: E402


def _solve(ctx, cls, mat, b, n, n_halo, counted=True, iters=1, **knobs):
    s = cls()
    s.num_iterations, s.absolute_error_tolerance, s.relative_error_tolerance = iters, 0.0, 0.0
    s.record_history = True
    for k, v in knobs.items():
        setattr(s, k, v)
    x = api.DeviceVector(ctx, n, n_halo)
    before = ctx.counter("throughput_solves"), ctx.counter("cg_fused_steps")
    s.solve(x, b, api.HipStencilOperator(mat, -1.0, 0.0))
    # (a partitioned operator: the throughput loops, with their all-reduces; the fused GMRES loop counts no path)
    assert ctx.counter("throughput_solves") == before[0] + int(counted) and s.iteration == iters and s.path_fallback == 0
    return s, x.to_numpy(), ctx.counter("cg_fused_steps") - before[1]


def _engine_solve(ctx, cls, mat, b, n, n_halo, iters):
    s = cls()
    s.num_iterations, s.absolute_error_tolerance, s.relative_error_tolerance = iters, 0.0, 0.0
    s.record_history = True
    x = api.DeviceVector(ctx, n, n_halo)
    before = ctx.counter("engine_solves")
    s.solve(x, b, api.HipStencilOperator(mat, -1.0, 0.0))
    assert ctx.counter("engine_solves") == before + 1 and s.iteration == iters and s.path_fallback == 0
    return s


def main():
    nx, ny, nzl = (int(v) for v in sys.argv[1:4])
    dist.init_process_group("gloo")
    rank, world = td.get_rank(), td.get_world_size()
    ctx = api.Context(0)
    transport = os.environ.get("STORM_TRANSPORT", "host")
    if transport == "ipc":
        dist.connect_ipc(ctx)
    else:
        dist.connect_host_staged(ctx)
    assert (ctx.n_ranks, ctx.rank) == (world, rank)

    nz = nzl * world
    k0, k1 = rank * nzl, (rank + 1) * nzl
    loc = mesh.structured_box_slab(nx, ny, nz, k0, k1, (float(nx), float(ny), float(nz)), rank_of_k=lambda k: k // nzl)
    plan = partition.halo_plan(loc, rank)
    n, n_halo = loc.n_cells, loc.n_halo
    shape = (nx, ny, nz)
    b_glob = er.int_vector(nx * ny * nz, 31)
    fs = er.FirstStep(er.Sums(shape, b_glob))
    b_loc = b_glob[loc.global_id[:n]]
    z_loc = er.int_apply(shape, b_glob, k0, k1)
    report = {"rank": rank, "world": world, "nbrs": [int(r) for r in plan.nbr_rank], "fused": {}, "history": {}}
    pins = {}
    from oracle import oracle

    # CG and BiCGStab to K = 4 against the step pins of the whole box (exact_ref.StepPins), on both transports
    steps = er.StepProblem(oracle, mesh, shape)
    assert np.array_equal(steps.b, b_glob)
    if transport == "host":  # the engine's CGS and TFQMR to K = 2 against the exact reference of the whole box
        g, basis = er.unit_box(mesh, *shape), er.Basis(shape, b_glob)
        pins = {kind: er.Pins(oracle, g, shape, b_glob, kind, fs=fs, basis=basis) for kind in ("cgs", "tfqmr")}

    ctx.set_option("spmv_canon_tile_min_rows", 0)  # (the lattice kernels on slabs this small)
    for fmt in (0, 4):
        ctx.set_option("spmv_dict", fmt)
        mat = api.StencilMatrix.from_face_graph(ctx, loc)
        ctx.set_option("spmv_dict", 4)
        mat.set_halo(plan.nbr_rank, plan.send_ptr, plan.send_idx, plan.recv_ptr)
        b = api.DeviceVector.from_numpy(ctx, b_loc.astype(np.float64), n_halo=n_halo)
        # the apply through the halo exchange and the global reductions
        zv = api.DeviceVector(ctx, n, n_halo)
        mat.apply(-1.0, 0.0, b, zv)
        assert np.array_equal(zv.to_numpy(), z_loc.astype(np.float64)), ("apply", fmt)
        assert api.dot_product(b, zv) == float(fs.s.pz), ("<b,z>", fmt)
        assert api.dot_product(b, b) == float(fs.s.rr), ("<b,b>", fmt)
        assert api.norm_2(b) == fs.h0, ("norm", fmt)
        # CG: x1 bitwise on the rank's rows
        s, x, fused = _solve(ctx, api.CgSolver, mat, b, n, n_halo)
        assert s.history[0] == fs.h0, ("cg h0", fmt, s.history[0], fs.h0)
        assert np.array_equal(x, fs.cg_x1(b_loc)), ("cg x1", fmt, int(np.count_nonzero(x != fs.cg_x1(b_loc))))
        assert er.close(s.history[1], fs.cg_h1, fs.cg_tol), ("cg h1", fmt, s.history[1], fs.cg_h1)
        report["fused"][f"cg{fmt}"] = int(fused)
        report["history"][f"cg{fmt}"] = [float(v) for v in s.history]
        s, _, _ = _solve(ctx, api.BiCgStabSolver, mat, b, n, n_halo)
        assert s.history[0] == fs.h0, ("bicgstab h0", fmt)
        assert er.close(s.history[1], fs.bicgstab_h1, fs.bicgstab_tol), ("bicgstab h1", fmt, s.history[1], fs.bicgstab_h1)
        report["history"][f"bicgstab{fmt}"] = [float(v) for v in s.history]
        s, _, _ = _solve(ctx, api.GmresSolver, mat, b, n, n_halo, counted=False, num_inner_iterations=30)
        assert s.history[0] == fs.h0, ("gmres h0", fmt)
        assert er.close(s.history[1], fs.gmres_h1, fs.gmres_tol), ("gmres h1", fmt, s.history[1], fs.gmres_h1)
        report["history"][f"gmres{fmt}"] = [float(v) for v in s.history]
        assert math.isfinite(s.history[1])
        for kind, cls in (("cg", api.CgSolver), ("bicgstab", api.BiCgStabSolver)):
            sp = steps.pins(kind, er.STEP_RANK_K)
            s, x, _ = _solve(ctx, cls, mat, b, n, n_halo, iters=sp.K)
            sp.check(list(s.history), f"{kind} K={sp.K} rank {rank} format {fmt}")
            report["history"][f"{kind}{fmt}K{sp.K}"] = [float(v) for v in s.history]
            parts = [None] * world
            td.all_gather_object(parts, (np.asarray(loc.global_id[:n]), x))
            if rank == 0:  # the residual of the gathered x against the exact history[K] (and x itself on a small box)
                x_glob = np.full(b_glob.size, np.nan)
                for ids, part in parts:
                    x_glob[ids] = part
                report.setdefault("x", {})[f"{kind}{fmt}"] = sp.check_x(x_glob, sp.K, f"{kind} K={sp.K} format {fmt}")
        for kind, cls in (("cgs", api.CgsSolver), ("tfqmr", api.TfqmrSolver)):
            if kind in pins:
                s = _engine_solve(ctx, cls, mat, b, n, n_halo, pins[kind].K)
                pins[kind].check(s.history, f"{kind} rank {rank} format {fmt}")
                report["history"][f"{kind}{fmt}"] = [float(v) for v in s.history]
        mat.close()
    ctx.sync()
    td.barrier()  # nobody unmaps / frees a peer window another rank's kernels may still write to
    ctx.close()
    td.barrier()
    with open(os.path.join(os.environ["STORM_REPORT_DIR"], f"rank{rank}.json"), "w") as f:
        json.dump(report, f)
    td.destroy_process_group()


if __name__ == "__main__":
    main()
