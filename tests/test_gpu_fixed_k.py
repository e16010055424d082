"""Statement-level parity of BiCGStab and GMRES(30) at the BASELINE sizes: tolerances OFF, a fixed number K of iterations
(K = 5, 10, 20; GMRES also across a restart), the residual history and the iterate against the oracle.

The converged-solve comparisons of tests/test_gpu_parity.py state looser bounds (iterations +-5 %, x to 2e-6 / 5e-6):
two solves that each stop at rel 1e-6 agree no better than that, and BiCGStab's recurrence amplifies one-ulp
differences.  This file backs those bounds with a statement-by-statement check: every residual norm the device loop
reports and the iterate it leaves against the oracle's loop (SolverBiCgStab.hpp:93-165, SolverGmres.hpp:119-192, 194-249
restated in oracle/storm_oracle.c), on the 64^3 and 128^3 Poisson boxes and on BASELINE config 4's 128^3
convection-diffusion operator -- through whichever kernels the dispatch picks at that size (resident / latency / chain /
kernel-per-statement: tests/test_gpu_dispatch.py pins which).

The bound: 1e-10 while the recurrence has not amplified anything yet (BiCGStab K = 5, GMRES K <= 10), 1e-9 beyond -- and
never tighter than what the ORACLE ITSELF can be held to: the same C source built with and without FMA contraction
(liboracle.so / liboracle_fma.so: two legitimate roundings of the reference's statements) is run beside the device, and
10 x their disagreement replaces the bound where it is larger.  Measured (round 6): BiCGStab after 20 iterations --
oracle against oracle 4e-8 (64^3), 9e-8 (128^3), 2.8e-6 (convection-diffusion); device against oracle 3.9e-8, 1.8e-7,
6.1e-6: the device sits inside the oracle's own rounding sensitivity, which is the strongest statement a comparison of
two roundings of this recurrence admits.  GMRES: oracle against oracle ~1e-12, device against oracle 1e-10 ... 3e-10.
That distance is the ORACLE's, not the device's: both oracle builds add every dot product as one serial chain of n terms
and share that error, so they agree with each other far better than either agrees with the exact value.  Against the
exact Arnoldi reference (tests/test_gpu_exact_gmres.py, K = 9 on 0.27 ... 2.1 M rows of an integer convection-diffusion
operator) the oracle is 4e-13 ... 6e-12 away and every device variant -- the chains of csrc/mgs_chain.hip with their
steps grouped by bilinearity included -- at most 1.3e-15: a few ulps.  A float64 restatement of the grouped form on
the CPU is no further from the exact value than the ungrouped one either (tests/test_exact_reference.py).

This file has no CG case.  CG -- and BiCGStab once more -- are held to an EXACT value, not to the oracle, for their first
8 (BiCGStab: 5) iterations in tests/test_gpu_exact_steps.py (exact_ref.StepPins, integer boxes of 15 k ... 4.3 M rows):
there the oracle's two builds lie 1e-15 ... 3e-13 from the exact history (the serial chain again, growing with n) and
every device path at most 6e-16."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

def _base_tol(kind, K):
    return 1e-10 if (kind == "bicgstab" and K <= 5) or (kind == "gmres" and K <= 10) else 1e-9


@pytest.fixture(scope="module")
def env():
    from oracle import oracle
    from stormruler_amd import api, mesh

    ctx = api.Context(0)
    yield api, mesh, oracle, ctx
    ctx.close()


def _device(api, ctx, cls, operator, b_host, iterations, restart=None):
    s = cls()
    s.record_history, s.num_iterations = True, iterations
    s.absolute_error_tolerance = s.relative_error_tolerance = 0.0  # both tests off (Solver.hpp:136-139): exactly K steps
    if restart is not None:
        s.num_inner_iterations = restart
    b = api.DeviceVector.from_numpy(ctx, b_host)
    x = api.DeviceVector(ctx, b_host.size)
    s.solve(x, b, operator)
    return s, x.to_numpy()


def _oracle_pair(oracle, kind, make_op, b, K):
    """The oracle's solve (strict build: the checker) and how far the FMA build of the same source is from it."""
    ref, fma = (oracle.solve(kind, make_op(v), b, num_iterations=K, abs_tol=0.0, rel_tol=0.0, num_inner_iterations=30, variant=v)
                for v in ("strict", "fma"))
    spread_h = np.abs(fma.history - ref.history).max() / np.abs(ref.history).max()
    spread_x = np.linalg.norm(fma.x - ref.x) / np.linalg.norm(ref.x)
    return ref, spread_h, spread_x


def _check(s, x, ref, spread_h, spread_x, base, what):
    assert s.iteration == ref.iterations, what
    hist = np.array(s.history)
    assert hist.shape == ref.history.shape, what
    worst = np.abs(hist - ref.history).max() / np.abs(ref.history).max()
    tol_h, tol_x = max(base, 10.0 * spread_h), max(base, 10.0 * spread_x)
    assert worst <= tol_h, (what, "history", worst, "bound", tol_h, "oracle strict vs fma", spread_h)
    err = np.linalg.norm(x - ref.x) / np.linalg.norm(ref.x)
    assert err <= tol_x, (what, "x", err, "bound", tol_x, "oracle strict vs fma", spread_x)


@pytest.mark.parametrize("n", [64, 128])
@pytest.mark.parametrize("kind,K", [("bicgstab", 5), ("bicgstab", 10), ("bicgstab", 20), ("gmres", 10), ("gmres", 20)])
def test_poisson_box_fixed_k_against_the_oracle(env, n, kind, K):
    """BASELINE configs 1 / 3's operator (7-point Poisson, Dirichlet walls, b = 1 and the survey's trigonometric b)."""
    api, mesh, oracle, ctx = env
    g = mesh.structured_box(n)
    mat = api.StencilMatrix.from_face_graph(ctx, g)
    op = api.HipStencilOperator(mat, -1.0, 0.0)
    c = g.center
    for name, b in (("ones", np.ones(g.n_cells)), ("trig", np.sin(3 * c[:, 0]) * np.cos(7 * c[:, 1]) * np.cos(2 * c[:, 2]))):
        ref, sh, sx = _oracle_pair(oracle, kind, lambda v: oracle.StencilOperator(g, -1.0, 0.0, variant=v), b, K)
        cls = api.BiCgStabSolver if kind == "bicgstab" else api.GmresSolver
        s, x = _device(api, ctx, cls, op, b, K, 30 if kind == "gmres" else None)
        _check(s, x, ref, sh, sx, _base_tol(kind, K), (n, kind, K, name))
    mat.close()


@pytest.mark.parametrize("kind,K", [("gmres", 10), ("gmres", 20), ("gmres", 45), ("bicgstab", 5), ("bicgstab", 10), ("bicgstab", 20)])
def test_convection_diffusion_128_fixed_k_against_the_oracle(env, kind, K):
    """BASELINE config 4's operator (128^3, nu = 1e-2, v = (1, 0.5, 0.25), first-order upwind): GMRES(30) through the
    Arnoldi chain kernel -- K = 45 crosses a restart (inner_finalize + outer restart, Solver.hpp:236-248) -- and BiCGStab on
    the same non-symmetric operator."""
    api, mesh, oracle, ctx = env
    g = mesh.structured_box(128)
    nu, vel = 1e-2, (1.0, 0.5, 0.25)
    wi, wo, de = mesh.convection_diffusion_weights(g, nu, vel)
    mat = api.StencilMatrix.from_face_weights(ctx, g.n_cells, g.n_halo, g.inner, g.outer, wi, wo, de)
    op = api.HipStencilOperator(mat, 1.0, 0.0)
    b = np.ones(g.n_cells)
    ref, sh, sx = _oracle_pair(oracle, kind, lambda v: oracle.StencilOperator(g, -nu, 0.0, conv=1.0, vel=vel, variant=v), b, K)
    cls = api.BiCgStabSolver if kind == "bicgstab" else api.GmresSolver
    s, x = _device(api, ctx, cls, op, b, K, 30 if kind == "gmres" else None)
    _check(s, x, ref, sh, sx, _base_tol(kind, K), ("convdiff128", kind, K))
    mat.close()
