"""Full-size, full-solve parity at the BASELINE sizes against the oracle's committed fixtures
(tests/golden/full_size_*.json, written by tools/make_full_size_fixtures.py from oracle/liboracle.so):

    configs[1]  CG,        7-point Poisson 256^3            526 iterations
    configs[2]  BiCGStab,  the same 256^3 block per GPU     355 iterations (reference summation order)
    configs[3]  GMRES(30), convection-diffusion 128^3       376 iterations

Every case runs twice on the device: through the fused loops of csrc/solver_cg.hip, solver_bicgstab.hip, solver_gmres.hip (what a stencil operator gets)
and through the general engine of csrc/krylov_*.hip (`generic_solvers = 1`: what a callback operator gets).

CG and GMRES reproduce the fixtures: same iteration count and operator applications, every entry of the residual
history to 1e-7 relative (measured: 1.7e-8 / 2.1e-8 -- tree sums against sequential ones over 1.7e7 / 2.1e6 terms), the
solution samples and norm to 1e-8.

BiCGStab at 256^3 cannot, and the fixture says why: the SAME oracle source with ONLY the order in which its
dot products add their 16.7 M terms changed (pairwise tree / one long double) or with FMA contraction allowed gives
350 / 352 / 355 / 361 iterations, and every one of those variants leaves the reference-order history by 1e-8 at
iteration 10, by 1e-6 at 18, by 1e-3 at 28 and by 10 % before iteration 45 (`summation_order_study`): the recurrence
amplifies rounding by ~10^2 every 8 iterations, after ~40 iterations no two roundings share a digit and the stopping
iteration (the residual hovers around the tolerance for the last ~30 iterations) is a draw.  A GPU reduction is a
tree sum, i.e. one more such variant.  What is asserted for it is therefore what the CPU variants satisfy among
themselves:
  * the residual history equals the reference-order one to 1e-6 for the first 12 iterations and to 1e-3 for the
    first 20 (the variants: 18 and 28),
  * the solve converges, the TRUE residual |b - A x| / |b| of the returned x is below 1.5e-6,
  * the solution agrees with the reference-order one to 1e-6 relative at every sampled cell and in norm (two solves
    that stop at relative residual 1e-6; the CPU variants differ by 6e-8 in norm),
  * the iteration count lies within three sample standard deviations of the mean of `perturbation_study` -- runs of
    the reference's statements on the operator in the HIP kernels' arithmetic form with every apply perturbed by at
    most one unit in the last place (tools/bicgstab_draw_study.py; 48 runs: 337 .. 382, mean 358.2, sigma 10.5).
    Measured on the device: 332 .. 378 depending on how the fused dot products group their partial sums.

The last test is SURVEY 8d's unstructured stress variant at full size: the 256^3 cells renumbered by the seeded
permutation, then reverse Cuthill-McKee -- no lattice, ~49 000 rows of column distance -- checked through properties
that do not need an oracle run: the permuted operator is the natural one conjugated by the permutation.
"""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NU, VEL = 1e-2, (1.0, 0.5, 0.25)


def _fixture(case):
    with open(os.path.join(ROOT, "tests", "golden", f"full_size_{case}.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def env():
    from stormruler_amd import api, mesh

    ctx = api.Context(0)
    yield api, mesh, ctx
    ctx.close()


@pytest.fixture(scope="module")
def poisson256(env):
    api, mesh, ctx = env
    g = mesh.structured_box(256)
    mat = api.StencilMatrix.from_face_graph(ctx, g)
    yield g, mat
    mat.close()


def _solve(api, ctx, solver, op, n_cells, generic):
    b, x = api.DeviceVector(ctx, n_cells), api.DeviceVector(ctx, n_cells)
    api.fill_with(b, 1.0)
    solver.record_history = True
    ctx.set_option("generic_solvers", int(generic))
    try:
        ok = solver.solve(x, b, op)
    finally:
        ctx.set_option("generic_solvers", 0)
    r = api.DeviceVector(ctx, n_cells)
    op.Residual(r, b, x)
    true_rel = api.norm_2(r) / api.norm_2(b)
    return ok, x.to_numpy(), true_rel


def _compare_exactly(fx, solver, ok, x, true_rel, hist_tol, x_tol):
    assert ok and fx["converged"]
    assert solver.iteration == fx["iterations"], (solver.iteration, fx["iterations"])
    assert solver.num_applies == fx["num_applies"]
    ref_h = np.array(fx["history"])
    assert len(solver.history) == len(ref_h)
    assert np.max(np.abs(solver.history - ref_h) / ref_h) <= hist_tol
    idx, ref_x = np.array(fx["sample_cells"]), np.array(fx["x_samples"])
    assert np.max(np.abs(x[idx] - ref_x) / np.abs(ref_x)) <= x_tol
    assert abs(np.sqrt(np.sum(x * x)) - fx["x_norm2"]) <= x_tol * fx["x_norm2"]
    assert abs(solver.relative_error - fx["relative_error"]) <= 1e-6 * fx["relative_error"] + hist_tol
    assert true_rel <= 1.5e-6


@pytest.mark.parametrize("generic", [False, True], ids=["fused", "engine"])
def test_cg_256_matches_the_oracle_fixture(env, poisson256, generic):
    api, mesh, ctx = env
    g, mat = poisson256
    fx = _fixture("cg256")
    s = api.CgSolver()
    ok, x, true_rel = _solve(api, ctx, s, api.HipStencilOperator(mat, -1.0, 0.0), g.n_cells, generic)
    _compare_exactly(fx, s, ok, x, true_rel, hist_tol=1e-7, x_tol=1e-8)


@pytest.mark.parametrize("generic", [False, True], ids=["fused", "engine"])
def test_gmres30_convdiff_128_matches_the_oracle_fixture(env, generic):
    api, mesh, ctx = env
    fx = _fixture("gmres128cd")
    g = mesh.structured_box(128)
    wi, wo, de = mesh.convection_diffusion_weights(g, NU, VEL)
    mat = api.StencilMatrix.from_face_weights(ctx, g.n_cells, g.n_halo, g.inner, g.outer, wi, wo, de)
    s = api.GmresSolver()
    s.num_inner_iterations = 30
    ok, x, true_rel = _solve(api, ctx, s, api.HipStencilOperator(mat, 1.0, 0.0), g.n_cells, generic)
    _compare_exactly(fx, s, ok, x, true_rel, hist_tol=1e-7, x_tol=1e-8)
    mat.close()


def test_the_fixture_itself_shows_bicgstab_256_is_a_draw():
    """CPU-side facts the BiCGStab bound rests on (no GPU involved; kept with the test that uses them)."""
    fx = _fixture("bicgstab256")
    study = fx["summation_order_study"]
    counts = {v: o["iterations"] for v, o in study.items()}
    assert fx["iterations"] == 355 and counts == {"fma": 350, "pairwise": 361, "longdouble": 352}
    for o in study.values():
        first = o["first_iteration_where_history_leaves_strict_by"]
        assert first["1e-08"] <= 12 and first["1e-06"] <= 20 and first["0.001"] <= 30 and first["0.1"] <= 45
        assert abs(o["x_norm2"] - fx["x_norm2"]) <= 1e-7 * fx["x_norm2"]
    # ... and the 24 runs of tools/bicgstab_draw_study.py: the reference's statements on the operator in the HIP
    # kernels' arithmetic form, every apply perturbed by at most one unit in the last place
    ps = fx["perturbation_study"]
    counts = [r["iterations"] for r in ps["runs"]]
    assert len(counts) >= 48 and all(r["converged"] for r in ps["runs"])
    assert (min(counts), max(counts)) == (ps["min_iterations"], ps["max_iterations"])
    assert min(counts) <= 337 and max(counts) >= 378  # (the first 24 runs alone span that much)
    lo, hi = _bicgstab256_count_bounds(fx)
    assert lo <= min(counts) and max(counts) <= hi and hi - lo <= 80  # the band holds its own data, and is a band
    by_family = {f: [r["iterations"] for r in ps["runs"] if r["family"] == f] for f in ("devlike", "strict")}
    assert max(by_family["strict"]) - min(by_family["strict"]) >= 20  # the reference's own summation order spreads too
    for r in ps["runs"]:
        assert abs(r["x_norm2"] - fx["x_norm2"]) <= 1e-6 * fx["x_norm2"]


def _bicgstab256_count_bounds(fx):
    """mean +- 3 sample standard deviations of the iteration counts of the committed last-place perturbation study
    (tools/bicgstab_draw_study.py): the device's count is one more draw from that distribution and must lie inside."""
    counts = np.array([r["iterations"] for r in fx["perturbation_study"]["runs"]], dtype=float)
    mean, std = counts.mean(), counts.std(ddof=1)
    return int(np.floor(mean - 3.0 * std)), int(np.ceil(mean + 3.0 * std))


@pytest.mark.parametrize("generic", [False, True], ids=["fused", "engine"])
def test_bicgstab_256_within_the_bound_summation_order_allows(env, poisson256, generic):
    api, mesh, ctx = env
    g, mat = poisson256
    fx = _fixture("bicgstab256")
    s = api.BiCgStabSolver()
    ok, x, true_rel = _solve(api, ctx, s, api.HipStencilOperator(mat, -1.0, 0.0), g.n_cells, generic)
    assert ok and s.relative_error < 1e-6 and true_rel <= 1.5e-6
    ref_h = np.array(fx["history"])
    rel = np.abs(s.history[:21] - ref_h[:21]) / ref_h[:21]
    assert np.max(rel[:13]) <= 1e-6, rel[:13]
    assert np.max(rel) <= 1e-3, rel
    lo, hi = _bicgstab256_count_bounds(fx)  # mean +- 3 sigma of the committed study (48 runs: 326 .. 390), not a percentage
    assert lo <= s.iteration <= hi, (s.iteration, lo, hi)
    assert s.num_applies == 1 + 2 * s.iteration
    idx, ref_x = np.array(fx["sample_cells"]), np.array(fx["x_samples"])
    assert np.max(np.abs(x[idx] - ref_x) / np.abs(ref_x)) <= 1e-6
    assert abs(np.sqrt(np.sum(x * x)) - fx["x_norm2"]) <= 1e-6 * fx["x_norm2"]


@pytest.mark.parametrize("kind", ["cg", "bicgstab"])
def test_in_kernel_reductions_are_reproducible_at_full_size(env, poisson256, kind):
    """The fused loops finish their reductions inside the kernels that produce the partial sums (two levels of
    tickets over up to 16 384 blocks, csrc/ticket_device.hpp).  A partial that a block published but the folding
    block did not yet see would show as a rare wrong sum: 1 500 iterations with the tolerances off, twice -- the
    residual histories (4 500 .. 7 500 ticketed reductions each) must agree BITWISE, and with the two-launch path
    (`ticket_reduce = 0`: other folding order) to rounding."""
    api, mesh, ctx = env
    g, mat = poisson256
    op = api.HipStencilOperator(mat, -1.0, 0.0)
    b = api.DeviceVector(ctx, g.n_cells)
    api.fill_with(b, 1.0)
    runs = []
    for ticket in (1, 1, 0):
        ctx.set_option("ticket_reduce", ticket)
        s = api.CgSolver() if kind == "cg" else api.BiCgStabSolver()
        s.record_history, s.num_iterations = True, 1500 if kind == "cg" else 60
        s.absolute_error_tolerance = s.relative_error_tolerance = 0.0
        x = api.DeviceVector(ctx, g.n_cells)
        s.solve(x, b, op)
        runs.append(np.array(s.history))
    ctx.set_option("ticket_reduce", 1)
    assert np.array_equal(runs[0], runs[1])
    k = 400 if kind == "cg" else 12  # (beyond, rounding differences have grown: see the module docstring)
    assert np.allclose(runs[0][:k], runs[2][:k], rtol=1e-6 if kind == "cg" else 1e-5)


def test_library_ordering_at_256_restores_the_lattice_and_orders_a_jittered_mesh(env, poisson256):
    """Round 4: the library's ordering from the cell centres (storm_hip_order_cells) at full size.  (i) The scrambled
    256^3 box gets its natural order back: the operator built from the re-ordered mesh has the natural one's records
    (format 4, tiled) and applies BITWISE like it.  (ii) The jittered geometry (all weights distinct: fp64 records) on the
    Z-order curve: P A P^T of the natural order's operator to 1e-13, and the same CG residuals."""
    from stormruler_amd import host_mesh

    api, mesh, ctx = env
    g, mat = poisson256
    n = g.n_cells
    perm = mesh.random_permutation(n)
    # (the library's own host mesh: scramble, order and operator build without a numpy pass over the faces)
    hm = host_mesh.HostMesh.from_face_graph(g)
    hm.permute_cells(perm)
    assert hm.order_cells("auto") == "lattice"
    assert np.array_equal(np.ctypeslib.as_array(hm.view().global_id, shape=(n,)), np.arange(n))
    matr = hm.create_operator(ctx)
    hm.close()
    st, st0 = matr.stats(), mat.stats()
    assert st["paired_rows"] == 2 and st["tiled_planes"] == st0["tiled_planes"] and st["record_bytes"] == st0["record_bytes"]
    x = api.DeviceVector.from_numpy(ctx, np.sin(0.37 * np.arange(n)))
    y0, y1 = api.DeviceVector(ctx, n), api.DeviceVector(ctx, n)
    mat.apply(-1.0, 0.0, x, y0), matr.apply(-1.0, 0.0, x, y1)
    assert np.array_equal(y0.to_numpy(), y1.to_numpy())
    matr.close()
    # (ii)
    gj = mesh.jitter_geometry(g, 1.0 / 256)
    matj = api.StencilMatrix.from_face_graph(ctx, gj)
    assert matj.stats()["value_dictionary_size"] == 0 and matj.stats()["paired_rows"] == 0  # fp64 weights + int32 columns
    hmj = host_mesh.HostMesh.from_face_graph(gj)
    del gj
    hmj.permute_cells(perm)
    assert hmj.order_cells("morton") == "morton"
    new_to_old = np.ctypeslib.as_array(hmj.view().global_id, shape=(n,)).copy()
    assert np.array_equal(np.sort(new_to_old), np.arange(n))
    matm = hmj.create_operator(ctx)
    hmj.close()
    xh = np.sin(0.37 * np.arange(n))
    yj, ym = api.DeviceVector(ctx, n), api.DeviceVector(ctx, n)
    matj.apply(-1.0, 0.0, api.DeviceVector.from_numpy(ctx, xh), yj)
    matm.apply(-1.0, 0.0, api.DeviceVector.from_numpy(ctx, xh[new_to_old]), ym)
    y_nat, y_m = yj.to_numpy(), ym.to_numpy()
    assert np.abs(y_m - y_nat[new_to_old]).max() <= 1e-13 * np.abs(y_nat).max()
    hist = {}
    for name, m in (("natural", matj), ("morton", matm)):
        s = api.CgSolver()
        s.record_history, s.num_iterations = True, 40
        s.absolute_error_tolerance = s.relative_error_tolerance = 0.0
        b, xs = api.DeviceVector(ctx, n), api.DeviceVector(ctx, n)
        api.fill_with(b, 1.0)
        s.solve(xs, b, api.HipStencilOperator(m, -1.0, 0.0))
        hist[name] = np.array(s.history)
    assert np.allclose(hist["natural"], hist["morton"], rtol=1e-10)
    matj.close(), matm.close()


def test_permuted_256_is_the_natural_operator_conjugated(env, poisson256):
    """SURVEY.md 8d "unstructured stress variant", full size (scrambled, then re-ordered by the build's ordering -- here the
    library's Z-order curve; reverse Cuthill-McKee, numpy / scipy, is the bench line's `roofline_permuted_rcm` and
    test_partition.py's at small size): P A P^T from the renumbered mesh (byte-indexed weights + int32 columns) against A
    from the natural ordering -- y' = P y to 1e-13, the operator
    symmetric to rounding, and 40 CG iterations give the same residual norms (a permutation changes no sum's terms,
    only their order)."""
    from stormruler_amd import host_mesh

    api, mesh, ctx = env
    g, mat = poisson256
    n = g.n_cells
    perm = mesh.random_permutation(n)
    hm = host_mesh.HostMesh.from_face_graph(g)
    hm.permute_cells(perm)
    assert hm.order_cells("morton") == "morton"  # (the Z-order curve asked for by name: "auto" would find the lattice again)
    new_to_old = np.ctypeslib.as_array(hm.view().global_id, shape=(n,)).copy()  # cell i of the renumbered mesh is cell new_to_old[i] of the natural one
    assert np.array_equal(np.sort(new_to_old), np.arange(n))
    v_ = hm.view()
    nf = int(v_.n_faces)
    dist = np.abs(np.ctypeslib.as_array(v_.inner, shape=(nf,)) - np.ctypeslib.as_array(v_.outer, shape=(nf,)))
    assert np.median(dist) <= 64  # (the curve keeps neighbours close: the scramble alone has a median of ~n / 3)
    matp = hm.create_operator(ctx)
    hm.close()
    st = matp.stats()
    assert st["n_rows"] == n and st["paired_rows"] == 0 and st["tiled_planes"] == 0 and st["tail_rows"] == 0
    assert st["value_dictionary_size"] > 0  # (byte-indexed weights + int32 columns: the box's five coefficients, no lattice order)
    x = np.sin(0.37 * np.arange(n))
    y = api.DeviceVector(ctx, n)
    mat.apply(-1.0, 0.0, api.DeviceVector.from_numpy(ctx, x), y)
    yp = api.DeviceVector(ctx, n)
    matp.apply(-1.0, 0.0, api.DeviceVector.from_numpy(ctx, x[new_to_old]), yp)
    y_nat, y_perm = y.to_numpy(), yp.to_numpy()
    assert np.abs(y_perm - y_nat[new_to_old]).max() <= 1e-13 * np.abs(y_nat).max()
    # symmetry: <A u, v> == <u, A v>
    u, v = api.DeviceVector.from_numpy(ctx, np.cos(0.11 * np.arange(n))), api.DeviceVector.from_numpy(ctx, x)
    au, av = api.DeviceVector(ctx, n), api.DeviceVector(ctx, n)
    matp.apply(-1.0, 0.0, u, au), matp.apply(-1.0, 0.0, v, av)
    lhs, rhs = api.dot_product(au, v), api.dot_product(u, av)
    assert abs(lhs - rhs) <= 1e-11 * abs(lhs)
    hist = {}
    for name, m in (("natural", mat), ("renumbered", matp)):
        s = api.CgSolver()
        s.record_history, s.num_iterations = True, 40
        s.absolute_error_tolerance = s.relative_error_tolerance = 0.0
        b, xs = api.DeviceVector(ctx, n), api.DeviceVector(ctx, n)
        api.fill_with(b, 1.0)
        s.solve(xs, b, api.HipStencilOperator(m, -1.0, 0.0))
        hist[name] = np.array(s.history)
    assert np.allclose(hist["renumbered"], hist["natural"], rtol=1e-9)
    matp.close()


def test_tetrahedral_mesh_at_full_size_against_the_oracle_and_under_renumbering(env):
    """The unstructured 3-D workload of the bench line at its full size: 12 582 912 tetrahedra (io_tetgen.tet_box(128): six
    shapes of cells, all weights distinct, rows of 2 - 4 neighbours) built by the library's host mesh.  (i) the HIP SpMV
    against the ORACLE's face loop over the same 25 M faces, <= 1e-13; (ii) the cells renumbered along the Z-order curve:
    the operator is the file order's conjugated by the permutation -- y' == y[order] to the last bit (faces keep their
    order: every row sums the same terms in the same order)."""
    from oracle import oracle
    from stormruler_amd import host_mesh, io_tetgen

    api, mesh, ctx = env
    pos, bf, cells = io_tetgen.tet_box(128)
    hm = host_mesh.HostMesh.from_simplices(pos, bf, np.ones(len(bf), np.int64), cells)
    del pos, bf, cells
    g = hm.face_graph()
    n = g.n_cells
    assert n == 6 * 128 ** 3 and g.n_faces == 25_067_520
    x = np.sin(0.37 * np.arange(n))
    ref_op = oracle.StencilOperator(g, -1.0, 0.0)
    y_ref = ref_op.apply(x)
    ref = oracle.solve("cg", ref_op, np.ones(n), num_iterations=12, abs_tol=0.0, rel_tol=0.0)  # (the reference's loop, 12 iterations)
    ref_b = oracle.solve("bicgstab", ref_op, np.ones(n), num_iterations=3, abs_tol=0.0, rel_tol=0.0)
    ref_g = oracle.solve("gmres", ref_op, np.ones(n), num_iterations=5, abs_tol=0.0, rel_tol=0.0, num_inner_iterations=5)
    del g, ref_op
    mat = hm.create_operator(ctx)
    st = mat.stats()
    assert st["max_row_len"] == 4 and st["tail_nnz"] == 0 and st["value_dictionary_size"] == 0
    y = api.DeviceVector(ctx, n)
    mat.apply(-1.0, 0.0, api.DeviceVector.from_numpy(ctx, x), y)
    y_file = y.to_numpy()
    assert np.abs(y_file - y_ref).max() <= 1e-13 * np.abs(y_ref).max()
    # ... and CG's first 12 residual norms and iterate against the oracle's solve of the same 12.6 M unknowns
    s = api.CgSolver()
    s.record_history, s.num_iterations = True, 12
    s.absolute_error_tolerance = s.relative_error_tolerance = 0.0
    b, xs = api.DeviceVector(ctx, n), api.DeviceVector(ctx, n)
    api.fill_with(b, 1.0)
    s.solve(xs, b, api.HipStencilOperator(mat, -1.0, 0.0))
    assert s.iteration == ref.iterations == 12
    assert np.allclose(np.array(s.history), ref.history, rtol=1e-10, atol=0.0)
    assert np.linalg.norm(xs.to_numpy() - ref.x) <= 1e-10 * np.linalg.norm(ref.x)
    for cls, want in ((api.BiCgStabSolver, ref_b), (api.GmresSolver, ref_g)):  # ... and the other two loops of the path, briefly
        s = cls()
        s.record_history, s.num_iterations = True, want.iterations
        if cls is api.GmresSolver:
            s.num_inner_iterations = 5
        s.absolute_error_tolerance = s.relative_error_tolerance = 0.0
        xs = api.DeviceVector(ctx, n)
        s.solve(xs, b, api.HipStencilOperator(mat, -1.0, 0.0))
        assert s.iteration == want.iterations
        assert np.allclose(np.array(s.history), want.history, rtol=1e-9, atol=0.0), cls.__name__
        assert np.linalg.norm(xs.to_numpy() - want.x) <= 1e-9 * np.linalg.norm(want.x), cls.__name__
    del b, xs
    mat.close()
    assert hm.order_cells("morton") == "morton"
    order = np.ctypeslib.as_array(hm.view().global_id, shape=(n,)).copy()
    mat = hm.create_operator(ctx)
    hm.close()
    mat.apply(-1.0, 0.0, api.DeviceVector.from_numpy(ctx, x[order]), y)
    assert np.array_equal(y.to_numpy(), y_file[order])
    mat.close()
