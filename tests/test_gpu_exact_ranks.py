"""The first-iteration pins of tests/test_gpu_exact_first_step.py across ranks (worker: tests/exact_rank_worker.py).

Exact integers make the order of every all-reduce irrelevant, so on the slab partition of a unit-spacing box each rank
must reproduce the whole box's closed forms: x1 bitwise on its own rows, history[0] bitwise and history[1] within the
derived tolerance, and the same history on every rank; CG and BiCGStab also run K = 4 iterations against the step pins
of the whole box (exact_ref.StepPins: history on every rank, the gathered x on rank 0).  World 2 on the host-staged
transport (with the engine's CGS and TFQMR to K = 2 against the exact reference of the whole box, exact_ref.Pins); world 3 on the
peer-window transport, where the fused CG finishes <p,z> with reduce_stage1_ticket_kernel<1> exchanging its sum itself
(the `ipc` branch of storm_hip_solve_cg) and cg_r_kernel finishes <r,r> through the window.  At most 4 processes with
the GPU open: the ranks and this one."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("world,dims,transport", [(2, (64, 16, 12), "host"), (3, (32, 16, 6), "ipc")])
def test_first_step_pins_on_every_rank(world, dims, transport, tmp_path):
    import exact_ref as er

    assert (dims[0], dims[1], dims[2] * world) in er.STEP_RANK_SHAPES  # (their caps: tests/test_exact_reference.py)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(ROOT, "tests", "exact_rank_worker.py"), *map(str, dims)]
    env = dict(os.environ, OMP_NUM_THREADS="1", STORM_REPORT_DIR=str(tmp_path), STORM_TRANSPORT=transport,
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-3000:] + "\n" + p.stderr[-3000:]
    reports = [json.load(open(tmp_path / f"rank{r}.json")) for r in range(world)]
    assert sorted(r["rank"] for r in reports) == list(range(world))
    for r in reports:
        assert len(r["nbrs"]) == (1 if r["rank"] in (0, world - 1) else 2)
        assert r["history"] == reports[0]["history"]  # every rank: the same bits
        assert all(len(r["history"][f"{kind}{fmt}K4"]) == 5 for kind in ("cg", "bicgstab") for fmt in (0, 4))
        if transport == "host":
            assert all(f"{kind}{fmt}" in r["history"] for kind in ("cgs", "tfqmr") for fmt in (0, 4))
    # rank 0 held the gathered x_4 of both methods and both formats to the exact residual and, on a box of at most
    # GMRES_X_ROWS rows (the three-rank one), to the exact x
    assert sorted(reports[0]["x"]) == ["bicgstab0", "bicgstab4", "cg0", "cg4"]
    rows = dims[0] * dims[1] * dims[2] * world
    assert all(len(v) == (2 if rows <= er.GMRES_X_ROWS else 1) for v in reports[0]["x"].values())
    if transport == "ipc":
        # the peer-window transport keeps the fused step on format 4 (the ticketed finishes, ipc branch)
        assert all(r["fused"]["cg4"] == 1 for r in reports), [r["fused"] for r in reports]
