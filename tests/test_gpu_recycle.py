"""storm_hip_recycle on the GPU (the recipe: include/storm_hip.h, restated in tests/recycle_ref.py).

1. Designed integer data: guess, update and the next guess equal the restatement bit for bit, in both access modes and on
   both paths (the fused kernels and the statement path).
2. Data with no structure: the fused kernels equal the statement path bit for bit over a whole sequence with a restart.
3. The guard, the restart, reset, and no host reduction.
4. The box sequence end to end through CgSolver.recycler, against a warm-started arm measured in the same test; the same
   sequence through tests/cpp/recycle_driver.
5. guess and update against the fp64 restatement on that box, tolerance by the rule of exact_ref.Pins.
6. The cavity with pressure_recycle.
7. Refusals.
"""
import math
import os
import subprocess

import numpy as np
import pytest

import exact_ref
import recycle_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPS = ((1, 0), (3, 2), (8, 7), (9, 8), (16, 15))
SIZES = (2, 127, 4097)  # 4 097: two stream blocks and an odd last row
E_INVALID, E_UNSUPPORTED = -1, -6


@pytest.fixture(scope="module")
def gpu():
    from stormruler_amd import api

    ctx = api.Context(0)
    yield api, ctx
    ctx.close()


@pytest.fixture(autouse=True)
def _defaults(gpu):
    yield
    _, ctx = gpu
    ctx.set_option("blas1_nt", 1)
    ctx.set_option("recycle_fused", 1)


def _vec(api, ctx, a):
    return api.DeviceVector.from_numpy(ctx, np.asarray(a, np.float64))


def _same(got, want, what):
    assert exact_ref.same_bits(got, want), f"{what}: {int(np.sum(exact_ref.bits(got) != exact_ref.bits(want)))} of {np.size(want)} " \
                                           f"elements differ, first at {int(np.argmax(exact_ref.bits(got) != exact_ref.bits(want)))}"


_DESIGNED = {}


def _designed(n, capacity, loaded, kind):
    """The restatement of one case, computed once and left unchanged."""
    key = (n, capacity, loaded, kind)
    if key not in _DESIGNED:
        _DESIGNED[key] = R.designed_run(n, capacity, loaded, kind)[1]
    return _DESIGNED[key]


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("capacity, loaded", CAPS)
@pytest.mark.parametrize("n", SIZES)
def test_designed_data_is_exact(gpu, n, capacity, loaded, kind):
    api, ctx = gpu
    want = _designed(n, capacity, loaded, kind)
    slots = R.designed_slots(n, loaded, kind)
    for nt in (0, 2):
        for fused in (0, 1):
            ctx.set_option("blas1_nt", nt)
            ctx.set_option("recycle_fused", fused)
            label = f"n={n} capacity={capacity} loaded={loaded} kind={kind} blas1_nt={nt} recycle_fused={fused}"
            keys = ("nt_stream_launches", "recycle_fused_launches", "recycle_statement_launches")
            before = [ctx.counter(k) for k in keys]
            rec = api.SolutionRecycler(ctx, n, capacity=capacity, kind=kind)
            try:
                for j, (u, v, g) in enumerate(slots):
                    rec.set_slot(j, _vec(api, ctx, u), _vec(api, ctx, v), float(g))
                assert rec.get("count") == loaded
                x = _vec(api, ctx, np.full(n, 7.0))  # (what a guess must overwrite)
                rec.guess(_vec(api, ctx, want["b"]), x)
                _same(x.to_numpy(), want["x0"], f"{label}: guess")
                assert [rec.get(f"coef_{j}") for j in range(loaded)] == want["c0"], label
                rec.update(_vec(api, ctx, want["x"]), _vec(api, ctx, want["ax"]))
                s = want["s"]
                assert rec.get("count") == s + 1 == loaded + 1
                u_s, v_s, g_s = rec.slot(s)
                _same(u_s.to_numpy(), want["u_s"], f"{label}: u_s")
                _same(v_s.to_numpy(), want["v_s"], f"{label}: v_s")
                assert g_s == want["g_s"] == rec.get(f"weight_{s}") and g_s > 0.0, (label, g_s, want["g_s"])
                assert rec.get("coef_0") == 0.0  # an update has followed the guess
                rec.guess(_vec(api, ctx, want["b2"]), x)
                _same(x.to_numpy(), want["x1"], f"{label}: the next guess")
                assert [rec.get(f"coef_{j}") for j in range(s + 1)] == want["c1"], label
            finally:
                rec.close()
            moved = [ctx.counter(k) - b for k, b in zip(keys, before)]
            assert (moved[0] > 0) == (nt == 2), (label, moved)  # the host chose the instance the option names
            assert (moved[1] > 0, moved[2] > 0) == (fused == 1, fused == 0), (label, moved)


def _unstructured(n, k):
    i = np.arange(n, dtype=np.float64)
    return np.sin(0.37 * i + 1.3 * k) + 0.25 * np.cos(0.011 * (k + 1) * i)


def _sequence(api, ctx, n, capacity, kind):
    """capacity + 2 guess / update rounds on vectors with no structure (ax = a smooth SPD-like map of x, the test's own);
    every x, every new pair and every scalar the object exposes."""
    rec = api.SolutionRecycler(ctx, n, capacity=capacity, kind=kind)
    out = []
    try:
        x = api.DeviceVector(ctx, n)
        for k in range(capacity + 2):
            b = _unstructured(n, 2 * k)
            xs = _unstructured(n, 2 * k + 1)
            ax = 3.0 * xs + 0.5 * np.roll(xs, 1) + 0.5 * np.roll(xs, -1)
            if k != 1:  # (round 1: an update with no guess since the last one)
                rec.guess(_vec(api, ctx, b), x)
                out.append(x.to_numpy())
                out.append(np.array([rec.get(f"coef_{j}") for j in range(capacity)]))
            rec.update(_vec(api, ctx, xs), _vec(api, ctx, ax))
            count = int(rec.get("count"))
            u, v, g = rec.slot(count - 1)
            out += [u.to_numpy(), v.to_numpy(), np.array([g]), np.array([rec.get(f"weight_{j}") for j in range(capacity)])]
        count = restarts = 0
        for _ in range(capacity + 2):  # the host's bookkeeping: a full object restarts
            restarts, count = (restarts + 1, 1) if count == capacity else (restarts, count + 1)
        assert restarts >= 1 and (rec.get("restarts"), rec.get("updates"), rec.get("count")) == (restarts, capacity + 2, count)
    finally:
        rec.close()
    return out


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("capacity", [c for c, _ in CAPS])
@pytest.mark.parametrize("n", SIZES)
def test_fused_kernels_equal_the_statement_path_bit_for_bit(gpu, n, capacity, kind):
    api, ctx = gpu
    for nt in (0, 2):
        ctx.set_option("blas1_nt", nt)
        runs = []
        for fused in (0, 1):
            ctx.set_option("recycle_fused", fused)
            runs.append(_sequence(api, ctx, n, capacity, kind))
        assert len(runs[0]) == len(runs[1])
        for k, (a, b) in enumerate(zip(*runs)):
            _same(b, a, f"n={n} capacity={capacity} kind={kind} blas1_nt={nt}: item {k} (fused against statements)")
        assert any(np.any(a != 0.0) for a in runs[0])


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("kind", [0, 1])
def test_the_guard_the_restart_and_reset(gpu, kind, fused):
    api, ctx = gpu
    ctx.set_option("recycle_fused", fused)
    n, m = 4097, 3
    rec = api.SolutionRecycler(ctx, n, n_halo=3, capacity=m, kind=kind)
    try:
        host_before = ctx.counter("host_reductions")
        launches = "recycle_fused_launches" if fused else "recycle_statement_launches"
        x0, b0 = _unstructured(n, 0), _unstructured(n, 1)
        x = api.DeviceVector(ctx, n, 3)
        l0 = ctx.counter(launches)
        rec.guess(_vec_h(api, ctx, b0), x)  # empty: zeros
        assert not np.any(x.to_numpy(with_halo=True))
        rec.update(_vec_h(api, ctx, x0), _vec_h(api, ctx, 2.0 * x0))
        if fused:
            assert ctx.counter(launches) - l0 == 2  # a fill; the first pair in one launch
        l0 = ctx.counter(launches)
        rec.guess(_vec_h(api, ctx, b0), x)
        g1 = x.to_numpy()
        if fused:
            assert ctx.counter(launches) - l0 == 2  # the multi-dot and recycle_guess_kernel
        # an x inside the span: nu <= 2^-40 nu0, the pair gets no weight and the next guess is unchanged
        l0 = ctx.counter(launches)
        rec.update(_vec_h(api, ctx, 3.0 * x0), _vec_h(api, ctx, 6.0 * x0))
        if fused:
            assert ctx.counter(launches) - l0 == 2  # recycle_defect_kernel and recycle_orth_kernel
        assert rec.get("count") == 2 and rec.get("weight_1") == 0.0 and rec.get("weight_0") > 0.0
        rec.guess(_vec_h(api, ctx, b0), x)
        _same(x.to_numpy(), g1, "the guess after a pair without weight")
        assert not np.any(x.to_numpy(with_halo=True)[n:])  # halo rows are left as they are
        # a non-finite ax
        bad = 2.0 * _unstructured(n, 5)
        bad[n // 2] = np.inf
        rec.update(_vec_h(api, ctx, _unstructured(n, 5)), _vec_h(api, ctx, bad))
        assert rec.get("count") == 3 and rec.get("weight_2") == 0.0 and rec.get("restarts") == 0
        # count == m: the restart
        xr = _unstructured(n, 7)
        axr = 2.0 * xr + 0.5 * np.roll(xr, 1) + 0.5 * np.roll(xr, -1)
        l0 = ctx.counter(launches)
        rec.update(_vec_h(api, ctx, xr), _vec_h(api, ctx, axr))
        if fused:
            assert ctx.counter(launches) - l0 == 1
        assert rec.get("count") == 1 and rec.get("restarts") == 1 and rec.get("updates") == 4
        u, v, g = rec.slot(0)
        _same(u.to_numpy(), xr, "u_0 after the restart")
        _same(v.to_numpy(), axr, "v_0 after the restart")
        nu = float(np.dot(axr, axr) if kind else np.dot(xr, axr))
        # g_0 = 1 / nu: the device's fold (depth D) and numpy's pairwise sum (shallower) each round relative to the sum of
        # the terms' absolute values; the division and this product round once each
        terms = float(np.dot(np.abs(axr), np.abs(axr if kind else xr)))
        assert g > 0.0 and abs(g * nu - 1.0) <= (2 * exact_ref.fold_depth(n) + 4) * 2.0 ** -53 * terms / nu
        assert [rec.get(f"weight_{j}") for j in (1, 2)] == [0.0, 0.0]
        # reset
        rec.reset()
        assert rec.get("count") == 0 and rec.get("weight_0") == 0.0
        x.upload(np.ones(n))
        rec.guess(_vec_h(api, ctx, b0), x)
        assert not np.any(x.to_numpy())
        assert ctx.counter("host_reductions") == host_before
    finally:
        rec.close()


def _vec_h(api, ctx, a):
    return api.DeviceVector.from_numpy(ctx, np.asarray(a, np.float64), n_halo=3)


def test_launch_counts_beyond_one_chunk(gpu):
    """16 pairs: the chains continue across launches of 8 -- a guess is 2 multi-dots + 2 launches, the update into slot 15 is
    2 + 1 multi-dot + 2."""
    api, ctx = gpu
    n = 127
    rec = api.SolutionRecycler(ctx, n, capacity=16, kind=0)
    try:
        for j, (u, v, g) in enumerate(R.designed_slots(n, 15, 0)):
            rec.set_slot(j, _vec(api, ctx, u), _vec(api, ctx, v), float(g))
        x = api.DeviceVector(ctx, n)
        l0 = ctx.counter("recycle_fused_launches")
        rec.guess(_vec(api, ctx, _unstructured(n, 0)), x)
        assert ctx.counter("recycle_fused_launches") - l0 == 4
        l0 = ctx.counter("recycle_fused_launches")
        xs = _unstructured(n, 1)
        rec.update(_vec(api, ctx, xs), _vec(api, ctx, 2.0 * xs))
        assert ctx.counter("recycle_fused_launches") - l0 == 5
        assert ctx.counter("recycle_guesses") >= 1 and ctx.counter("recycle_updates") >= 1
    finally:
        rec.close()


# ---- the box sequence ------------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def box(gpu):
    from stormruler_amd import mesh

    api, ctx = gpu
    g = exact_ref.unit_box(mesh, *R.BOX_SHAPE)
    mat = api.StencilMatrix.from_face_graph(ctx, g)
    op = api.HipStencilOperator(mat, alpha=-1.0, beta=0.0)  # A = -L
    yield g.n_cells, op
    mat.close()


def _box_arm(api, ctx, n, op, recycler):
    """The 14 solves; per solve (iterations, |r0|, converged, true |b - A x|).  recycler None: the warm start."""
    s = api.CgSolver()
    s.relative_error_tolerance = 0.0
    s.recycler = recycler
    x, ax = api.DeviceVector(ctx, n), api.DeviceVector(ctx, n)
    out = []
    for t in range(R.BOX_SOLVES):
        b = R.box_rhs(t)
        bv = _vec(api, ctx, b)
        s.absolute_error_tolerance = R.BOX_TOL * api.norm_2(bv)  # (the device's norm: the C++ driver forms the same value)
        ok = s.solve(x, bv, op)
        op.mul(ax, x)
        out.append((int(s.iteration), float(s.initial_error), bool(ok), float(np.linalg.norm(b - ax.to_numpy()))))
    return out


@pytest.fixture(scope="module")
def box_warm(gpu, box):
    api, ctx = gpu
    return _box_arm(api, ctx, box[0], box[1], None)


@pytest.mark.parametrize("kind", ["energy", "residual"])
def test_box_sequence_end_to_end(gpu, box, box_warm, kind, tmp_path):
    api, ctx = gpu
    n, op = box
    rec = api.SolutionRecycler(ctx, n, capacity=8, kind=kind)
    try:
        host_before = ctx.counter("host_reductions")
        got = _box_arm(api, ctx, n, op, rec)
        assert rec.get("restarts") == 1 and rec.get("updates") == R.BOX_SOLVES and rec.get("count") == R.BOX_SOLVES - 8
    finally:
        rec.close()
    warm_total, rec_total = sum(w[0] for w in box_warm), sum(w[0] for w in got)
    print(f"{kind}: warm {[w[0] for w in box_warm]} = {warm_total}; recycled {[w[0] for w in got]} = {rec_total}; "
          f"ratio {rec_total / warm_total:.3f}; |r0| {[f'{w[1]:.2e}' for w in got]}; "
          f"true residual warm {max(w[3] for w in box_warm):.3e} recycled {max(w[3] for w in got):.3e}; "
          f"host reductions moved by {ctx.counter('host_reductions') - host_before}")
    assert rec_total <= R.BOX_RATIO * warm_total
    for t in R.BOX_CAPPED:
        assert got[t][0] <= R.BOX_CAP, (t, got[t])
    assert all(w[2] for w in got), "every recycled solve converges"
    assert max(w[3] for w in got) <= 2.0 * max(w[3] for w in box_warm)
    # the same sequence through the C++ binding: the same library calls on the same right-hand sides
    rhs = tmp_path / "rhs.f64"
    np.stack([R.box_rhs(t) for t in range(R.BOX_SOLVES)]).astype(np.float64).tofile(rhs)
    driver = os.path.join(ROOT, "tests", "cpp", "recycle_driver")
    out = subprocess.run([driver, str(rhs), kind, "8"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = [ln.split() for ln in out.stdout.strip().split("\n") if ln.startswith("solve")]
    assert len(lines) == R.BOX_SOLVES, out.stdout
    for t, ln in enumerate(lines):
        assert int(ln[1]) == t and int(ln[2]) == got[t][0], (t, ln, got[t])
        assert float(ln[3]) == pytest.approx(got[t][1], rel=1e-12), (t, ln, got[t])
        assert ln[4] == "1"


def _guess_floor(ref, b):
    """An a-priori bound on |x_device - x_exact| of a guess, elementwise maximum: each e_j is a fold of depth D whose terms are
    |t_j b| (D + 1 roundings with the product c_j = g_j e_j), and the chain adds one rounding per term."""
    D = exact_ref.fold_depth(ref.n)
    k = ref.count
    bound = np.zeros(ref.n)
    for j in range(k):
        mag = abs(ref.g[j]) * float(np.dot(np.abs(ref.t(j)), np.abs(b)))
        bound += ((D + 1) * mag + k * abs(ref.c[j])) * np.abs(ref.u[j])
    return 2.0 ** -53 * float(bound.max())


@pytest.mark.parametrize("kind", [0, 1])
def test_guess_and_update_against_the_fp64_restatement_on_the_box(gpu, box, kind):
    """Five solves of the box sequence fill five pairs; then one guess and one update on the device against the restatement
    fed with the device's own pairs (get_slot).  Tolerance: max(floor, 16 x the fp64 restatement's distance from the
    Fraction value) -- derived from the data, as exact_ref.Pins derives its own."""
    api, ctx = gpu
    n, op = box
    rec = api.SolutionRecycler(ctx, n, capacity=8, kind=kind)
    try:
        s = api.CgSolver()
        s.relative_error_tolerance, s.recycler = 0.0, rec
        x, ax = api.DeviceVector(ctx, n), api.DeviceVector(ctx, n)
        for t in range(5):
            b = R.box_rhs(t)
            s.absolute_error_tolerance = R.BOX_TOL * float(np.linalg.norm(b))
            assert s.solve(x, _vec(api, ctx, b), op)
        count = int(rec.get("count"))
        assert count == 5
        refs = [R.Recycler(sp, n, 8, kind) for sp in (R.F64, R.Exact)]
        for j in range(count):
            u, v, g = rec.slot(j)
            assert g > 0.0
            for ref in refs:
                ref.set_slot(j, u.to_numpy(), v.to_numpy(), g)
        b = R.box_rhs(5)
        rec.guess(_vec(api, ctx, b), x)
        x_dev = x.to_numpy()
        x64, xex = refs[0].guess(b), refs[1].guess(b)
        xex_f = np.array([float(v) for v in xex.tolist()])
        own = max(abs(float(a - bb)) for a, bb in zip(R.Exact.vec(x64).tolist(), xex.tolist()))
        floor = _guess_floor(refs[0], b)
        dist = float(np.abs(x_dev - xex_f).max())
        print(f"kind {kind} guess: device-exact {dist:.3e}, fp64-exact {own:.3e}, floor {floor:.3e}, |x| {np.abs(xex_f).max():.3e}")
        assert floor <= 1e-10 * float(np.abs(xex_f).max())  # (a condition on the case: the bound separates rounding from a defect)
        assert dist <= max(floor, 16.0 * own)
        # the update: a solve's x and its A x, taken from the device
        s.recycler = None
        s.absolute_error_tolerance = R.BOX_TOL * float(np.linalg.norm(b))
        assert s.solve(x, _vec(api, ctx, b), op)
        op.mul(ax, x)
        xs, axs = x.to_numpy(), ax.to_numpy()
        rec.update(x, ax)
        u, v, g = rec.slot(count)
        for ref in refs:
            ref.update(xs, axs)
        D, k = exact_ref.fold_depth(n), count
        f64, ex = refs
        # floor of the new pair: the chains' terms and the coefficients' folds, as in _guess_floor, for both chains
        for name, dev, r64, rex, which in (("u_s", u.to_numpy(), f64.u[count], ex.u[count], f64.u), ("v_s", v.to_numpy(), f64.v[count], ex.v[count], f64.v)):
            start = np.abs(xs if name == "u_s" else axs)
            bound = 2 * k * start
            ad_abs = np.abs(axs) + sum(abs(cj) * np.abs(f64.v[j]) for j, cj in enumerate(_coefs(f64, b)))
            for j in range(k):
                cmag = abs(f64.g[j]) * float(np.dot(np.abs(f64.t(j)), np.abs(b)))
                bmag = abs(f64.g[j]) * float(np.dot(np.abs(f64.t(j)), ad_abs))
                bound = bound + ((D + 1) * (cmag + bmag) + 2 * k * (cmag + bmag)) * np.abs(which[j])
            floor = 2.0 ** -53 * float(bound.max())
            rex_f = np.array([float(q) for q in rex.tolist()])
            own = max(abs(float(a - bb)) for a, bb in zip(R.Exact.vec(r64).tolist(), rex.tolist()))
            dist = float(np.abs(dev - rex_f).max())
            print(f"kind {kind} {name}: device-exact {dist:.3e}, fp64-exact {own:.3e}, floor {floor:.3e}, |{name}| {np.abs(rex_f).max():.3e}")
            assert dist <= max(floor, 16.0 * own), name
        assert g > 0.0
    finally:
        rec.close()


def _coefs(ref, b):
    """c_j of the guess with b on the pairs before the update (the restatement forgets them with the update)."""
    return [ref.sp.mul(ref.g[j], ref.sp.dot(ref.t(j), ref.sp.vec(b))) for j in range(ref.count - 1)]


# ---- the cavity ------------------------------------------------------------------------------------------------------------


def test_cavity_with_pressure_recycle(gpu):
    from stormruler_amd.cavity import CavityProjection

    api, ctx = gpu
    plain, zero, rec = CavityProjection(ctx, 12), CavityProjection(ctx, 12, pressure_recycle=0), CavityProjection(ctx, 12, pressure_recycle=6)
    assert plain.solver.recycler is None and zero.solver.recycler is None and rec.solver.recycler is not None
    its = {"plain": [], "zero": [], "rec": []}
    for step in range(10):
        for name, cav in (("plain", plain), ("zero", zero), ("rec", rec)):
            it, _, ok = cav.step()
            assert ok, (name, step)
            its[name].append(it)
        assert rec.divergence_norm() <= 2.0 * plain.divergence_norm(), step
    print(f"cavity 12^3 pressure iterations: plain {its['plain']}, pressure_recycle=6 {its['rec']}")
    assert its["zero"] == its["plain"]
    assert rec.solver.recycler.get("updates") == 10 and rec.solver.recycler.get("restarts") == 1
    with pytest.raises(ValueError):
        CavityProjection(ctx, 12, pressure_recycle=17)


# ---- refusals --------------------------------------------------------------------------------------------------------------


def test_refusals(gpu):
    api, ctx = gpu
    StormHipError = api._lib.StormHipError

    def refused(fn, status=E_INVALID):
        with pytest.raises(StormHipError) as e:
            fn()
        assert e.value.status == status, e.value

    refused(lambda: api.SolutionRecycler(ctx, 16, capacity=0))
    refused(lambda: api.SolutionRecycler(ctx, 16, capacity=17))
    refused(lambda: api.SolutionRecycler(ctx, 16, kind=2))
    rec = api.SolutionRecycler(ctx, 16, capacity=2)
    try:
        a, b, short = api.DeviceVector(ctx, 16), api.DeviceVector(ctx, 16), api.DeviceVector(ctx, 15)
        refused(lambda: rec.guess(short, a))
        refused(lambda: rec.guess(a, short))
        refused(lambda: rec.update(a, short))
        refused(lambda: rec.guess(a, a))
        refused(lambda: rec.update(a, a))
        refused(lambda: rec.set_slot(1, a, b, 1.0))  # j <= count
        refused(lambda: rec.slot(0))                 # j < count
        refused(lambda: rec.get("weight_2"))
        other = api.Context(0)
        try:
            refused(lambda: rec.guess(api.DeviceVector(other, 16), a))
        finally:
            other.close()
        rec.set_slot(0, a, b, 0.0)  # j == count appends
        assert rec.get("count") == 1
    finally:
        rec.close()
    comm_ctx = api.Context(0)
    try:
        comm_ctx.comm_init(api.Context.comm_unique_id(), 1, 0)  # the size-1 RCCL communicator of test_gpu_comm.py
        refused(lambda: api.SolutionRecycler(comm_ctx, 16), E_UNSUPPORTED)
    finally:
        comm_ctx.close()
