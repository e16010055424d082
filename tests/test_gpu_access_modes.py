"""Both access-mode instances of every kernel family against the same pins.

Two options pick, at launch time, which compiled copy of a kernel runs:

* ``blas1_nt`` (common.hpp: stream_nt): 0 plain, 2 non-temporal loads and stores in the streaming kernels, 1 (the default)
  non-temporal from 6 * 2^20 rows on -- so below that size the suite runs the plain copy and a 256^3 user the other one;
* ``nontemporal`` (opt_nt): the NT template instance of the record-reading kernels (default 1, so the suite runs NT = true).

Here the kernels that no other file runs in their other instance -- the Chebyshev step and start kernels, the multigrid
residual, Jacobi sweep and null-space projection, the face-weight refresh, the reduced apply, the one-column block kernels,
the finite-difference product -- run in all four modes (nontemporal, blas1_nt) of MODES on the smallest shapes at which their
edges occur (the shapes, builders and references of the files that own them: imported, not copied).  Outputs are compared
BITWISE across the modes; what the owning file pins to an exact or closed-form reference is pinned again in mode (0, 2), the
one in which no default instance runs.  No tolerance of its own: every bound is the owning file's.

The comparison cannot be vacuous: counter ``nt_stream_launches`` counts the launch sites at which the host chose the
non-temporal instance.  Every call under blas1_nt 2 that has such a site must move it, no call under blas1_nt 0 may.
(``nontemporal`` has no size gate and is read directly at its six launch sites.)  The counter says what the host chose, not
what instructions the instance holds.  tests/test_access_mode_ledger.py keeps the list of files with such a site complete."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cheb_ref  # noqa: E402
import exact_ref as er  # noqa: E402
import test_gpu_amg as t_amg  # noqa: E402
import test_gpu_amg_jacobi as t_jac  # noqa: E402
import test_gpu_amg_nullspace as t_null  # noqa: E402
import test_gpu_block as t_block  # noqa: E402
import test_gpu_cheb as t_cheb  # noqa: E402
import test_gpu_face_update as t_face  # noqa: E402
import test_gpu_jfnk_native as t_jfnk  # noqa: E402
import test_gpu_reduced as t_red  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = ((1, 0), (1, 2), (0, 0), (0, 2))  # (nontemporal, blas1_nt); below 6 * 2^20 rows the first is what the defaults run
LAST = (0, 2)  # no default instance runs
CHEB_KEYS = ("cheb_fused_applies", "cheb_statement_applies", "cheb_reduced_applies")


@pytest.fixture(scope="module")
def env():
    from oracle import oracle
    from stormruler_amd import _lib, api, io_tetgen, mesh

    ctx = api.Context(0)
    # `four` / `five`: the tuples the owning files' helpers take as their `env`
    yield SimpleNamespace(api=api, mesh=mesh, oracle=oracle, lib=_lib, ctx=ctx, four=(api, mesh, oracle, ctx),
                          five=(api, mesh, io_tetgen, _lib, ctx))
    ctx.close()


@pytest.fixture(autouse=True)
def _defaults(env):
    yield
    for k, v in (("nontemporal", 1), ("blas1_nt", 1), ("cheb_fused", 1), ("amg_fused", 1), ("spmv_dict", 4), ("ell_cap", 0),
                 ("lazy_statements", 0)):
        env.ctx.set_option(k, v)


def _in_mode(ctx, mode, call, streams=True):
    """call() under a mode.  ``streams``: the call has a launch site that asks stream_nt (under blas1_nt 2 the counter must
    move); False: it has none (the counter must stay); None: its kernels are picked by `nontemporal`, whatever else it
    launches.  Under blas1_nt 0 the counter stays, always."""
    ctx.set_option("nontemporal", mode[0])
    ctx.set_option("blas1_nt", mode[1])
    before = ctx.counter("nt_stream_launches")
    out = call()
    moved = ctx.counter("nt_stream_launches") - before
    if mode[1] == 2 and streams:
        assert moved > 0, (mode, moved)
    elif mode[1] != 2 or streams is False:
        assert moved == 0, (mode, moved)
    return out


def _all_same(outs, what):
    for mode, out in zip(MODES[1:], outs[1:]):
        assert er.same_bits(out, outs[0]), (what, mode, int(np.sum(er.bits(out) != er.bits(outs[0]))))
    assert np.isfinite(outs[0]).all() and np.abs(outs[0]).max() > 0, what


# ---- a. Chebyshev ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cheb_ops(env):
    """test_gpu_cheb.py's fused_operators (fp64 records, no tail); the 13^3 box with its fp32-weight companion."""
    api, mesh, ctx = env.api, env.mesh, env.ctx
    ops = {}
    for name, n in (("box13", 13), ("box52", 52)):
        g = mesh.structured_box(n)
        mat = t_cheb._matrix(api, ctx, api.StencilMatrix.from_face_graph, g, spmv_dict=0)
        ops[name] = (mat, -1.0, 0.0, g.n_cells, mesh.assemble_csr(g, -1.0, 0.0).tocsr() if n == 13 else None)
    a = t_cheb._random_symmetric()
    ops["random_csr"] = (t_cheb._matrix(api, ctx, api.StencilMatrix.from_csr, a, spmv_dict=0), 1.0, 0.0, a.shape[0], a)
    ops["box13"][0].build_reduced()
    yield ops
    for mat, *_ in ops.values():
        mat.close()


def _cheb_paths(ctx, ch, r, z, n):
    """z by cheb_fused 1 and 0 of one object, and what the counters moved by."""
    out, counts = [], []
    try:
        for fused in (1, 0):
            ctx.set_option("cheb_fused", fused)
            z.upload(np.full(n, np.nan))  # (the FIRST step must not read z)
            before = [ctx.counter(k) for k in CHEB_KEYS]
            assert ch.apply(r, z) == 0
            out.append(z.to_numpy())
            counts.append(tuple(ctx.counter(k) - b for k, b in zip(CHEB_KEYS, before)))
    finally:
        ctx.set_option("cheb_fused", 1)
    return out, counts


# degrees 1, 2, 4: the FIRST & LAST instance; FIRST, LAST; and the middle one.  The reduced-record object (Rec32) on the 13^3 box.
CHEB_CASES = [(name, degree, jacobi, records) for name in ("box13", "random_csr", "box52") for degree in (1, 2, 4)
              for jacobi in (False, True) for records in (("fp64", "fp32") if name == "box13" else ("fp64",))]


@pytest.mark.parametrize("name,degree,jacobi,records", CHEB_CASES,
                         ids=[f"{c[0]}-degree{c[1]}-{'jacobi' if c[2] else 'unscaled'}-{c[3]}" for c in CHEB_CASES])
def test_chebyshev_apply_in_every_mode(env, cheb_ops, name, degree, jacobi, records):
    """cheb_d0_kernel (blas1_nt; 2 197 rows: its odd tail row) and cheb_step_kernel<NT, ...> (nontemporal) on Rec64 and Rec32,
    and the statement path under them."""
    api, ctx = env.api, env.ctx
    mat, alpha, beta, n, _ = cheb_ops[name]
    if name == "box13":
        assert n % 2 == 1 and n % 64 != 0
    dinv = None
    if jacobi:
        dinv = api.DeviceVector(ctx, n)
        mat.diagonal(alpha, beta, dinv, invert=True)
    reduced = records == "fp32"
    ch = t_red._Cheb(env.lib.lib, mat, alpha, beta, dinv, degree, reduced)
    assert ch.status == 0 and ch.get("reduced") == float(reduced)
    r_host = np.sin(0.37 * np.arange(n)) + 0.25
    r, z = api.DeviceVector.from_numpy(ctx, r_host), api.DeviceVector(ctx, n)
    outs = []
    for mode in MODES:
        (z_fused, z_stmt), counts = _in_mode(ctx, mode, lambda: _cheb_paths(ctx, ch, r, z, n))
        assert counts == [(1, 0, int(reduced)), (0, 1, int(reduced))], (mode, counts)  # as in the default mode
        assert er.same_bits(z_fused, z_stmt), mode
        outs.append(z_fused)
    _all_same(outs, (name, degree, jacobi, records))
    assert np.array_equal(r.to_numpy(), r_host)  # r is not written
    ch.close()


@pytest.fixture(scope="module")
def cheb_eigenpairs(cheb_ops):
    """The eigendecompositions of the closed form, once per (operator, scale)."""
    made = {}

    def get(name, jacobi):
        if (name, jacobi) not in made:
            a = cheb_ops[name][4]
            s = 1 / a.diagonal() if jacobi else np.ones(a.shape[0])
            made[name, jacobi] = (s, cheb_ref.eigenpairs(a, s))
        return made[name, jacobi]

    return get


@pytest.mark.parametrize("jacobi", [False, True], ids=["unscaled", "jacobi"])
@pytest.mark.parametrize("name", ["box13", "random_csr"])
def test_chebyshev_closed_form_in_the_last_mode(env, cheb_ops, cheb_eigenpairs, name, jacobi):
    """test_device_z_matches_the_closed_form's bound, 1e-10 (degree x condition number x 2^-53 stays below 1e-11 on these two:
    the 13^3 box has about three times the 8^3 box's condition number), with NT = false steps and a non-temporal start."""
    api, ctx = env.api, env.ctx
    mat, alpha, beta, n, a = cheb_ops[name]
    s, eig = cheb_eigenpairs(name, jacobi)
    lmax = cheb_ref.gershgorin(a, s)
    lmin = lmax / 30
    r_host = np.sin(0.37 * np.arange(n))
    dinv = api.DeviceVector.from_numpy(ctx, s) if jacobi else None
    r, z = api.DeviceVector.from_numpy(ctx, r_host), api.DeviceVector(ctx, n)
    for degree in (1, 2, 4):
        ref = cheb_ref.closed_form(a, s, r_host, lmin, lmax, degree, eig=eig)
        ch = t_cheb._Cheb(env.lib.lib, mat, alpha, beta, dinv, degree, lmin, lmax)
        assert ch.status == 0
        (z_fused, z_stmt), counts = _in_mode(ctx, LAST, lambda: _cheb_paths(ctx, ch, r, z, n))
        assert counts == [(1, 0, 0), (0, 1, 0)]
        for which, got in (("fused", z_fused), ("statements", z_stmt)):
            rel = np.linalg.norm(got - ref) / np.linalg.norm(ref)
            print(f"{name} jacobi {jacobi} degree {degree} {which}: rel {rel:.3e}")
            assert rel <= 1e-10
        ch.close()


# ---- b. multigrid ---------------------------------------------------------------------------------------------------------
AMG_KEYS = ("amg_applies", "amg_fused_residuals", "amg_statement_residuals", "cheb_fused_applies", "cheb_statement_applies")
AMG_CHEB_CASES = {"box13": 2, "box20": 2, "random_tail": 2, "box52": 2}  # name: smoother degree (test_gpu_amg.py's)


@pytest.fixture(scope="module")
def amg_hierarchies(env):
    """One hierarchy per operator, reused across the modes: only the options change between applies."""
    made = {}

    def get(name):
        if name not in made:
            tail = name == "random_tail"
            mat, alpha, beta, a, params = t_amg._operator(env.four, "random" if tail else name)
            pre = t_amg._build(env.four, mat, alpha, beta, ell_cap=8 if tail else 0, smoother_degree=AMG_CHEB_CASES[name], **params)
            made[name] = (mat, pre, a)
        return made[name]

    yield get
    for mat, pre, _ in made.values():
        pre.close()
        mat.close()


def _amg_paths(ctx, pre, r, z, n, keys, paths):
    """z of one apply per (amg_fused, cheb_fused) pair, and what the counters moved by."""
    out, counts = [], []
    try:
        for amg_fused, cheb_fused in paths:
            ctx.set_option("amg_fused", amg_fused)
            ctx.set_option("cheb_fused", cheb_fused)
            z.upload(np.full(n, np.nan))  # (the cycle must not read z)
            before = [ctx.counter(k) for k in keys]
            pre.mul(z, r)
            out.append(z.to_numpy())
            counts.append(tuple(ctx.counter(k) - b for k, b in zip(keys, before)))
    finally:
        ctx.set_option("amg_fused", 1)
        ctx.set_option("cheb_fused", 1)
    return out, counts


@pytest.mark.parametrize("name", list(AMG_CHEB_CASES))
def test_multigrid_cycle_with_the_chebyshev_smoother_in_every_mode(env, amg_hierarchies, name):
    """amg_residual_kernel<NT, XCD> and the smoothers' step kernels (nontemporal), their start kernels and the statements
    (blas1_nt): 13^3 (ragged last slice), 20^3 (a coarsest level of 7 rows), the random CSR with a level that falls to the
    statements by itself, 52^3 (the XCD instances)."""
    api, ctx = env.api, env.ctx
    mat, pre, a = amg_hierarchies(name)
    rows = pre.hierarchy.level_rows()
    levels, n = len(rows), rows[0]
    if name == "box20":
        assert rows[-1] == 7
    if name == "box52":
        assert mat.stats()["spmv_blocks"] > 8 * 64 and mat.stats()["xcd_run_blocks"] == 64
    r_host = np.sin(0.37 * np.arange(n)) + 0.25
    r, z = api.DeviceVector.from_numpy(ctx, r_host), api.DeviceVector(ctx, n)
    per = 2 * (levels - 1)
    outs = []
    for mode in MODES:
        out, counts = _in_mode(ctx, mode, lambda: _amg_paths(ctx, pre, r, z, n, AMG_KEYS, ((1, 1), (0, 1), (0, 0))))
        if name == "random_tail":  # (test_fused_residual_gives_the_statements_bits: level 1 has a CSR tail)
            assert rows == [918, 69, 1] and counts[0] == (1, 2, 2, 2, 2), (mode, counts)
        else:
            assert counts[0] == (1, per, 0, per, 0), (mode, counts)
        assert counts[1][:3] == (1, 0, per) and counts[2] == (1, 0, per, 0, per), (mode, counts)
        assert er.same_bits(out[0], out[1]) and er.same_bits(out[0], out[2]), mode
        outs.append(out[0])
    _all_same(outs, name)
    assert np.array_equal(r.to_numpy(), r_host)


def _against_the_restatement(label, z_dev, c64, cld, r_host):
    """The owning files' rule: |device - restatement| within 10 x the restatement's own float64-against-long-double distance."""
    z64, zld = c64(r_host), cld(r_host)
    margin = 10.0 * float(np.abs(z64 - zld.astype(np.float64)).max())
    diff = float(np.abs(z_dev - z64).max())
    print(f"{label}: |device - restatement| = {diff:.3e}, margin {margin:.3e}, |z| = {np.abs(z64).max():.3e}")
    assert margin > 0 and diff <= margin


@pytest.mark.parametrize("name", ["box13", "box20", "random_tail"])
def test_multigrid_cycle_against_the_restatement_in_the_last_mode(env, amg_hierarchies, name):
    api, ctx = env.api, env.ctx
    mat, pre, a = amg_hierarchies(name)
    n = a.shape[0]
    r_host = np.random.default_rng(4).standard_normal(n)
    r, z = api.DeviceVector.from_numpy(ctx, r_host), api.DeviceVector(ctx, n)
    out, _ = _in_mode(ctx, LAST, lambda: _amg_paths(ctx, pre, r, z, n, AMG_KEYS, ((1, 1),)))
    _against_the_restatement(name, out[0], t_amg._restatement(pre), t_amg._restatement(pre, np.longdouble), r_host)


@pytest.mark.parametrize("sweeps", [1, 2])
@pytest.mark.parametrize("name", ["cd13", "cd20", "random_tail", "cd52"])
def test_multigrid_cycle_with_the_jacobi_smoother_in_every_mode(env, name, sweeps):
    """amg_jacobi_sweep_kernel<NT, XCD, R> (nontemporal), the sweep from the zero guess (cheb_d0_kernel: blas1_nt) and the
    statements, on test_fused_sweep_gives_the_statements_bits's cases; .smooth() of level 0; and the cycle against the
    restatement in the last mode."""
    api, ctx = env.api, env.ctx
    tail = name == "random_tail"
    mat, alpha, beta, a, params = t_jac._operator(env.four, "random" if tail else name)
    pre = t_jac._build(env.four, mat, alpha, beta, ell_cap=8 if tail else 0, jacobi_sweeps=sweeps, **params)
    rows = pre.hierarchy.level_rows()
    n, smoothing, per = rows[0], len(rows) - 1, 2 * sweeps - 1
    r_host = np.sin(0.37 * np.arange(n)) + 0.25
    z_host = np.cos(0.11 * np.arange(n))
    r, z = api.DeviceVector.from_numpy(ctx, r_host), api.DeviceVector(ctx, n)
    z_in = api.DeviceVector.from_numpy(ctx, z_host)

    def smooth():
        out = []
        try:
            for amg_fused, key in ((1, "amg_fused_sweeps"), (0, "amg_statement_sweeps")):
                ctx.set_option("amg_fused", amg_fused)
                z.upload(np.full(n, np.nan))
                before = ctx.counter(key)
                pre.smooth(0, r, z_in, z)
                assert ctx.counter(key) == before + 1
                out.append(z.to_numpy())
        finally:
            ctx.set_option("amg_fused", 1)
        return out

    cycles, smoothed = [], []
    for mode in MODES:
        out, counts = _in_mode(ctx, mode, lambda: _amg_paths(ctx, pre, r, z, n, t_jac.SWEEP_KEYS, ((1, 1), (0, 1))))
        if tail:
            assert counts[0] == (1, per, per, 1, 1), (mode, counts)
        else:
            assert counts[0] == (1, per * smoothing, 0, smoothing, 0), (mode, counts)
        assert counts[1] == (1, 0, per * smoothing, 0, smoothing), (mode, counts)
        assert er.same_bits(out[0], out[1]), mode
        cycles.append(out[0])
        both = _in_mode(ctx, mode, smooth)  # (the statement form streams; the fused sweep reads `nontemporal` alone)
        assert er.same_bits(both[0], both[1]), mode
        smoothed.append(both[0])
    _all_same(cycles, (name, sweeps, "cycle"))
    _all_same(smoothed, (name, sweeps, "smooth"))
    assert np.array_equal(z_in.to_numpy(), z_host) and np.array_equal(r.to_numpy(), r_host)
    if name != "cd52":  # (the restatement in long double: on the sizes the owning file restates)
        rr_host = np.random.default_rng(4).standard_normal(n)
        r.upload(rr_host)
        out, _ = _in_mode(ctx, LAST, lambda: _amg_paths(ctx, pre, r, z, n, t_jac.SWEEP_KEYS, ((1, 1),)))
        _against_the_restatement(f"{name} sweeps {sweeps}", out[0], t_jac._restatement(pre), t_jac._restatement(pre, np.longdouble),
                                 rr_host)
    pre.close()
    mat.close()


def test_a_jacobi_sweep_is_exact_on_integers_in_the_last_mode(env):
    """test_a_sweep_is_exact_on_integers itself: the NT = false sweep and the non-temporal statements."""
    _in_mode(env.ctx, LAST, lambda: t_jac.test_a_sweep_is_exact_on_integers(env.four))


@pytest.mark.parametrize("n", [2, 63, 64, 65, 2047, 2048, 2049, 133123])  # (test_projection_is_exact_on_integers's: five odd)
def test_projection_is_exact_on_integers_in_the_last_mode(env, n):
    """amg_mean_kernel and amg_shift_kernel (in place) on their non-temporal instances: that test's data and sizes."""
    _in_mode(env.ctx, LAST, lambda: t_null.test_projection_is_exact_on_integers(env.four, n))


def test_null_space_object_in_every_mode(env):
    """Pi and Pi V Pi on the owning file's smallest singular case (the 12 x 10 x 9 Neumann box): amg_mean_kernel,
    amg_axpy_mean_kernel (the fused closing statement) and amg_shift_kernel by blas1_nt, the cycle inside by both options."""
    api, ctx = env.api, env.ctx
    mat, alpha, a = t_null._operator(env.four, "box")
    pre = t_null._build(env.four, mat, alpha, smoother_degree=t_null.DEGREE["box"], **t_null.PARAMS)
    n = a.shape[0]
    assert n == 1080 and int(pre.get("levels")) > 1
    v_host = np.random.default_rng(9).standard_normal(n) + 0.25
    keys = ("amg_applies", "amg_projections", "amg_fused_projections", "amg_fused_residuals", "amg_statement_residuals")

    def project():
        v = api.DeviceVector.from_numpy(ctx, v_host)
        before = ctx.counter("amg_projections")
        pre.project(v)
        assert ctx.counter("amg_projections") == before + 1
        return v.to_numpy()

    def cycle():
        out, counts = [], []
        try:
            for amg_fused in (1, 0):
                ctx.set_option("amg_fused", amg_fused)
                before = [ctx.counter(k) for k in keys]
                out.append(t_null._apply(env.four, pre, v_host))
                counts.append(tuple(ctx.counter(k) - b for k, b in zip(keys, before)))
        finally:
            ctx.set_option("amg_fused", 1)
        return out, counts

    projected, cycled = [], []
    for mode in MODES:
        projected.append(_in_mode(ctx, mode, project))
        out, counts = _in_mode(ctx, mode, cycle)
        assert [c[:3] for c in counts] == [(1, 2, 1), (1, 2, 0)], (mode, counts)  # (test_options_give_the_same_bits's)
        assert er.same_bits(out[0], out[1]), mode
        cycled.append(out[0])
    _all_same(projected, "project")
    _all_same(cycled, "cycle")
    r_host = np.random.default_rng(4).standard_normal(n)
    z_dev = _in_mode(ctx, LAST, lambda: t_null._apply(env.four, pre, r_host))
    _against_the_restatement("null-space box", z_dev, t_null._restatement(pre), t_null._restatement(pre, np.longdouble), r_host)
    pre.close()
    mat.close()


# ---- c. the face-weight refresh -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def face_shapes(env):
    return t_face.shapes.__wrapped__(env.five)


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "d2", "e", "f"])
@pytest.mark.parametrize("diag", [True, False], ids=["diag_random", "diag_null"])
def test_face_weight_refresh_in_both_streaming_modes(env, face_shapes, name, diag):
    """op_refresh_sell_kernel<true> (its non-temporal load of the ids, st_pair<true>) and <false>: the refreshed operator is
    the fresh one, bit for bit; on shape b the fp32 companion converted behind the refresh as well."""
    api, ctx, lib = env.api, env.ctx, env.lib
    s = face_shapes[name]
    n, nt = s["n"], s["n"] + s["n_halo"]
    w0, w1 = t_face._weights(s, 10), t_face._weights(s, 11)
    rng = np.random.default_rng(12)
    x_all, y0, xb = rng.uniform(-1, 1, nt), rng.uniform(-1, 1, n), rng.uniform(-1, 1, (n, 2))
    fresh = t_face._create(api, ctx, s, w1, diag, False, dict0=True)
    want = t_face._everything(api, lib, ctx, s, fresh, x_all, y0, xb)
    assert {"apply", "apply_add", "diagonal"} <= set(want)
    companion = name == "b"
    if companion:
        rounded = t_red._create(api, ctx, s, t_red._rounded(w1), diag)
        x = api.DeviceVector.from_numpy(ctx, x_all)
        want_reduced = t_red._apply(api, ctx, rounded, -0.7, 0.3, x, False)
        rounded.close()
    for blas1_nt in (2, 0):
        up = t_face._create(api, ctx, s, w0, diag, True)
        if companion:
            up.build_reduced()
        refreshes = ctx.counter("op_reduced_refreshes")
        _in_mode(ctx, (1, blas1_nt), lambda: t_face._set(api, ctx, up, w1, diag))
        ctx.set_option("blas1_nt", 1)
        got = t_face._everything(api, lib, ctx, s, up, x_all, y0, xb)
        assert sorted(got) == sorted(want)
        for key in got:
            assert er.same_bits(got[key], want[key]), (blas1_nt, key)
        if companion:
            assert ctx.counter("op_reduced_refreshes") == refreshes + 1
            assert er.same_bits(t_red._apply(api, ctx, up, -0.7, 0.3, x, True), want_reduced), blas1_nt
        up.close()
    fresh.close()


def _assembled_product(s, w, x_all):
    """M x of the face-weight operator in int64 (storm_hip.h: row inner[f] gets w_inner[f] (x_outer - x_inner), row outer[f]
    w_outer[f] (x_inner - x_outer), and diag_extra on the diagonal), with exact_dot's check: the magnitudes of a row's terms
    sum far below 2^53, so every order and every contraction gives this value."""
    n = s["n"]
    wi, wo, de = (np.asarray(a, np.int64) for a in w)
    x = np.asarray(x_all, np.int64)
    i, o = s["inner"], s["outer"]
    y, mag = de * x[:n], np.abs(de) * np.abs(x[:n])
    np.add.at(y, i, wi * (x[o] - x[i]))
    np.add.at(mag, i, np.abs(wi) * (np.abs(x[o]) + np.abs(x[i])))
    own = o < n  # (a halo cell has no row)
    np.add.at(y, o[own], (wo * (x[i] - x[o]))[own])
    np.add.at(mag, o[own], (np.abs(wo) * (np.abs(x[i]) + np.abs(x[o])))[own])
    assert int(mag.max()) < er.EXACT
    return y


@pytest.mark.parametrize("name", ["a", "e"])
def test_refreshed_integer_weights_apply_exactly(env, face_shapes, name):
    """Integer weights in [-8, 8] written by the refresh, an integer x in [-1000, 1000]: apply(1, 0) is the int64 product of
    the assembled matrix.  (Compared as values plus + 0.0: an exactly zero row sum has the sign its order of summation
    gives it, which the bitwise comparison with the fresh operator above holds; every other bit is compared.)"""
    api, ctx, lib = env.api, env.ctx, env.lib
    s = face_shapes[name]
    n, f = s["n"], s["inner"].size
    w0 = tuple(er.int_vector(k, 50 + j, -8, 8) for j, k in enumerate((f, f, n)))
    w1 = tuple(er.int_vector(k, 60 + j, -8, 8) for j, k in enumerate((f, f, n)))
    x_all = er.int_vector(n + s["n_halo"], 70)
    want = _assembled_product(s, w1, x_all).astype(np.float64)
    assert np.abs(want).max() > 0
    x = t_face._vector_with_halo(api, lib, ctx, x_all.astype(np.float64), n)
    for blas1_nt in (2, 0):
        up = t_face._create(api, ctx, s, tuple(a.astype(np.float64) for a in w0), True, True)
        _in_mode(ctx, (1, blas1_nt), lambda: t_face._set(api, ctx, up, tuple(a.astype(np.float64) for a in w1), True))
        y = api.DeviceVector.from_numpy(ctx, np.full(n, np.nan))
        up.apply(1.0, 0.0, x, y)
        assert er.same_bits(y.to_numpy() + 0.0, want), (blas1_nt, int(np.count_nonzero(y.to_numpy() != want)))
        up.close()


# ---- d. the reduced apply -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def reduced_shapes(env):
    return t_red.shapes.__wrapped__(env.five)


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "d2", "f", "box52"])
@pytest.mark.parametrize("diag", [True, False], ids=["diag_random", "diag_null"])
def test_reduced_apply_with_plain_loads(env, reduced_shapes, name, diag):
    """op_reduced.hip's apply with NT = false on test_reduced_apply_is_the_fp64_apply_of_the_rounded_operator's shapes: the
    fp64 apply of the rounded operator (default mode), bit for bit, and the NT = true reduced apply's bits."""
    api, ctx = env.api, env.ctx
    s = reduced_shapes[name]
    w = t_red._weights(s, 50)
    op, ref = t_red._create(api, ctx, s, w, diag), t_red._create(api, ctx, s, t_red._rounded(w), diag)
    op.build_reduced()
    x = api.DeviceVector.from_numpy(ctx, t_red._x(s["n"]))
    for alpha, beta in t_red.COEFS:
        want = t_red._apply(api, ctx, ref, alpha, beta, x, False)
        got = [_in_mode(ctx, (nt, 1), lambda: t_red._apply(api, ctx, op, alpha, beta, x, True), streams=False) for nt in (0, 1)]
        assert not np.isnan(got[0]).any()
        assert er.same_bits(got[0], want) and er.same_bits(got[1], want), (alpha, beta)
    op.close(), ref.close()


# ---- e. block vectors of one column ---------------------------------------------------------------------------------------
def test_one_column_block_kernels_in_both_streaming_modes(env):
    """block_nt is non-zero for k = 1 alone: block_dot on integers at 40 x 30 x 17 (exact), block_axpy (one fma per element),
    mul_block on integers (exact; `nontemporal` picks its instance), under blas1_nt 2 and 0."""
    api, mesh, ctx = env.api, env.mesh, env.ctx
    n = 40 * 30 * 17
    a, b = er.int_vector(n, 31), er.int_vector(n, 71)
    A = api.BlockVector.from_numpy(ctx, a.astype(np.float64)[:, None])
    B = api.BlockVector.from_numpy(ctx, b.astype(np.float64)[:, None])
    m = 4099
    rng = np.random.default_rng(3)
    x, y, coef = rng.standard_normal((m, 1)), rng.standard_normal((m, 1)), rng.standard_normal(1)
    want_axpy = er.vfma(coef[0], x[:, 0], y[:, 0])[:, None]

    def dots_and_axpy():
        got, sq = api.block_dot(A, B), api.block_dot(A, A)
        X, Y = api.BlockVector.from_numpy(ctx, x), api.BlockVector.from_numpy(ctx, y)
        api.block_axpy(Y, coef, X)
        return got[0], sq[0], Y.to_numpy()

    for mode in MODES:
        got, sq, axpy = _in_mode(ctx, mode, dots_and_axpy)
        assert got == float(er.exact_dot(a, b)) and sq == float(er.exact_dot(a, a)), mode
        assert er.same_bits(axpy, want_axpy), mode
        for shape in (t_block.SMALL, t_block.ODD):
            _in_mode(ctx, mode, lambda: t_block.test_mul_block_on_integers_is_exact(env.four, shape, 1), streams=None)


def test_one_column_block_cg_against_the_exact_pins(env):
    """test_block_cg_two_iterations_against_the_exact_pins with ONE column (seed 31, its first) on its shape: 2 iterations
    against exact_ref.Pins, 8 against exact_ref.StepPins, under blas1_nt 2; history and x bitwise those of blas1_nt 0."""
    api, mesh, oracle, ctx = env.api, env.mesh, env.oracle, env.ctx
    shape = t_block.SMALL
    g = er.unit_box(mesh, *shape)
    mat = t_block._fp64(ctx, lambda: api.StencilMatrix.from_face_graph(ctx, g))
    seed = er.STEP_BLOCK_SEEDS[0]
    b = er.int_vector(g.n_cells, seed)
    pins2 = er.Pins(oracle, g, shape, b, "cg")
    p = er.StepProblem(oracle, mesh, shape, seed=seed)
    assert np.array_equal(p.b, b)
    pins = p.pins("cg")
    runs = {}
    for blas1_nt in (2, 0):
        s2, _, _ = _in_mode(ctx, (1, blas1_nt), lambda: t_block._block_solve(api, ctx, mat, [b], 2))
        s8, x8, _ = _in_mode(ctx, (1, blas1_nt), lambda: t_block._block_solve(api, ctx, mat, [b], er.STEP_K["cg"]))
        runs[blas1_nt] = (np.array(s2.history[0]), np.array(s8.history[0]), x8)
        ratios = pins2.check(list(s2.history[0]), label=f"one column, blas1_nt {blas1_nt}")
        assert s8.iterations[0] == pins.K
        far = pins.check(list(s8.history[0]), f"one column, blas1_nt {blas1_nt}")
        xr = pins.check_x(x8[:, 0], pins.K, f"one column, blas1_nt {blas1_nt}")
        print(f"steps block-cg one column blas1_nt {blas1_nt}: ratios {ratios}   far {max(far):.1e}   x {xr[0]:.1e}")
    for got, want in zip(runs[2], runs[0]):
        assert er.same_bits(got, want)
    mat.close()


# ---- f. the finite-difference product and a Newton solve --------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 693, 2049])  # (test_product_bit_for_bit's; its 6 * 2^20 + 1 streams non-temporally there)
def test_finite_difference_product_streams_non_temporally(env, n):
    """fd_shift_kernel<true> and the non-temporal difference statement against the reference roundings that test asserts."""
    for mode in ((1, 2), (0, 2)):
        _in_mode(env.ctx, mode, lambda: t_jfnk.test_product_bit_for_bit(env.four, n))


def test_newton_solve_is_the_same_in_every_mode(env):
    """One whole solve of the smallest cubic (11 x 9 x 7): history and x bitwise in the four modes."""
    api, mesh, oracle, ctx = env.api, env.mesh, env.oracle, env.ctx
    pb = t_jfnk.Cubic(api, mesh, oracle, ctx, t_jfnk.BOXES["11x9x7"])
    assert pb.n == 693
    hist, xs = [], []
    for mode in MODES:
        s, ok, x = _in_mode(ctx, mode, lambda: t_jfnk._device_solve(api, ctx, pb))
        assert ok and s.iteration > 1
        hist.append(np.array(s.history))
        xs.append(x)
    _all_same(hist, "history")
    _all_same(xs, "x")
    pb.close()
