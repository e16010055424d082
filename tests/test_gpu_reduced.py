"""fp32-weight companion records (csrc/op_reduced.hip, include/storm_hip.h "fp32-weight companion records").

The one contract: with ``F(w)`` a fresh fp64-record operator built from ``double(float(w))``, ``double(float(ext))``, a
reduced apply, Gershgorin bound, Chebyshev apply (either path) or a solve preconditioned by it on ``op(w)`` is BIT FOR BIT
what the existing fp64 entry point gives on ``F(w)``.  Shapes (those of tests/test_gpu_face_update.py, spmv_dict = 0):

  a    5x4x3 box: 60 rows, one ragged slice
  b    13^3 box, faces randomly permuted and flipped: 2 197 rows, 35 slices, ragged last
  c    the reference's triangles (square_nb.1): width 3, the unpaired last slot
  d    a 200-cell ring and a hub joined to every cell: the wide-row path, most of the hub's row in the CSR tail
  d2   shape b under ell_cap = 2: a tail in every row
  e    shape a with its last plane as halo columns (refused)
  f    three cells, no faces: width 0
  box52  52^3 box, faces in natural order: more than 8 x 64 blocks, so the XCD runs are active with a ragged tail
"""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_UNSUPPORTED = -1, -6
NU, VEL_A = 1e-2, (1.0, 0.5, 0.25)
COEFS = ((-1.0, 0.0), (1e-2, 1.0), (0.37, -1.3))


@pytest.fixture(scope="module")
def env():
    from stormruler_amd import _lib, api, io_tetgen, mesh

    ctx = api.Context(0)
    yield api, mesh, io_tetgen, _lib, ctx
    ctx.close()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def f32(a):
    """double(float(a)): IEEE round to nearest even, numpy's conversion."""
    return None if a is None else np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def _box_faces(nx, ny, nz, owned_planes):
    inner, outer = [], []
    for k in range(owned_planes):
        for j in range(ny):
            for i in range(nx):
                c = i + nx * (j + ny * k)
                if i + 1 < nx:
                    inner.append(c), outer.append(c + 1)
                if j + 1 < ny:
                    inner.append(c), outer.append(c + nx)
                if k + 1 < nz:
                    inner.append(c), outer.append(c + nx * ny)
    return np.array(inner, np.int64), np.array(outer, np.int64)


def _shuffled(inner, outer, arrays, seed=2):
    rng = np.random.default_rng(seed)
    p = rng.permutation(inner.size)
    flip = rng.random(inner.size) < 0.5
    i2, o2 = np.where(flip, outer[p], inner[p]), np.where(flip, inner[p], outer[p])
    return i2, o2, [(np.where(flip, wo[p], wi[p]), np.where(flip, wi[p], wo[p])) for wi, wo in arrays]


@pytest.fixture(scope="module")
def shapes(env):
    api, mesh, io_tetgen, _lib, ctx = env
    out = {}
    i, o = _box_faces(5, 4, 3, 3)
    out["a"] = dict(n=60, n_halo=0, inner=i, outer=o, ell_cap=0)
    g = mesh.structured_box(13)
    wa = mesh.convection_diffusion_weights(g, NU, VEL_A)
    i, o, (fa,) = _shuffled(g.inner, g.outer, [(wa[0], wa[1])])
    out["b"] = dict(n=g.n_cells, n_halo=0, inner=i, outer=o, ell_cap=0, vel_a=(fa[0], fa[1], wa[2]))
    tri = io_tetgen.read_triangle(os.path.join(ROOT, "tests", "golden", "mesh", "square_nb.1."))
    out["c"] = dict(n=tri.n_cells, n_halo=0, inner=tri.inner, outer=tri.outer, ell_cap=0)
    ring = np.arange(200, dtype=np.int64)
    i = np.stack([ring, np.full(200, 200, np.int64)], 1).ravel()
    o = np.stack([(ring + 1) % 200, ring], 1).ravel()
    out["d"] = dict(n=201, n_halo=0, inner=i, outer=o, ell_cap=0)
    out["d2"] = dict(out["b"], ell_cap=2)
    i, o = _box_faces(5, 4, 3, 2)
    out["e"] = dict(n=40, n_halo=20, inner=i, outer=o, ell_cap=0)
    out["f"] = dict(n=3, n_halo=0, inner=np.zeros(0, np.int64), outer=np.zeros(0, np.int64), ell_cap=0)
    g = mesh.structured_box(52)
    out["box52"] = dict(n=g.n_cells, n_halo=0, inner=np.asarray(g.inner, np.int64), outer=np.asarray(g.outer, np.int64), ell_cap=0)
    return out


def _weights(s, seed):
    rng = np.random.default_rng(seed)
    f = s["inner"].size
    return rng.uniform(-1, 1, f), rng.uniform(-1, 1, f), rng.uniform(-1, 1, s["n"])


def _create(api, ctx, s, w, diag, updatable=False, spmv_dict=0):
    ctx.set_option("ell_cap", s["ell_cap"])
    ctx.set_option("spmv_dict", spmv_dict)
    try:
        make = api.StencilMatrix.from_face_weights_updatable if updatable else api.StencilMatrix.from_face_weights
        return make(ctx, s["n"], s["n_halo"], s["inner"], s["outer"], w[0], w[1], w[2] if diag else None)
    finally:
        ctx.set_option("ell_cap", 0)
        ctx.set_option("spmv_dict", 4)


def _rounded(w):
    return f32(w[0]), f32(w[1]), f32(w[2])


def _x(n):
    return np.sin(0.37 * np.arange(n))


def _apply(api, ctx, mat, alpha, beta, x, reduced):
    y = api.DeviceVector.from_numpy(ctx, np.full(mat.stats()["n_rows"], np.nan))  # y must not be read
    (mat.apply_reduced if reduced else mat.apply)(alpha, beta, x, y)
    return y.to_numpy()


# ---- 1. the contract ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "b", "c", "d", "d2", "f", "box52"])
@pytest.mark.parametrize("diag", [True, False], ids=["diag_random", "diag_null"])
def test_reduced_apply_is_the_fp64_apply_of_the_rounded_operator(env, shapes, name, diag):
    api, mesh, io_tetgen, _lib, ctx = env
    s = shapes[name]
    n = s["n"]
    w = _weights(s, 50)
    every = np.concatenate([w[0], w[1]] + ([w[2]] if diag else []))
    if every.size:  # the fixture can fail: (almost) no weight is its own fp32 rounding
        assert np.mean(every != f32(every)) >= 0.99
    op, ref = _create(api, ctx, s, w, diag), _create(api, ctx, s, _rounded(w), diag)
    st = op.stats()
    assert st["value_dictionary_size"] == 0 and st["paired_rows"] == 0
    if name in ("d", "d2"):
        assert st["tail_nnz"] > 0
    if name == "d":
        assert st["max_row_len"] == 200
    if name == "box52":
        assert st["spmv_blocks"] > 8 * 64 and st["spmv_blocks"] % (8 * 64) != 0
    builds = ctx.counter("op_reduced_builds")
    op.build_reduced()
    assert ctx.counter("op_reduced_builds") == builds + 1
    x = api.DeviceVector.from_numpy(ctx, _x(n))
    for alpha, beta in COEFS:
        got = _apply(api, ctx, op, alpha, beta, x, True)
        want = _apply(api, ctx, ref, alpha, beta, x, False)
        assert not np.isnan(got).any()
        assert same_bits(got, want), (alpha, beta, int(np.sum(bits(got) != bits(want))))
        if s["inner"].size:  # the companion is neither an alias of the fp64 records nor a truncation of them
            own = _apply(api, ctx, op, alpha, beta, x, False)
            has_nb = np.zeros(n, bool)
            has_nb[s["inner"]] = has_nb[s["outer"]] = True
            differs = bits(own) != bits(got)
            print(f"{name} ({alpha}, {beta}): {differs[has_nb].mean():.3f} of the rows with neighbours differ from the fp64 apply")
            assert differs[has_nb].mean() >= 0.9
    op.close(), ref.close()


def test_truncation_would_not_pass(env, shapes):
    """The reference of the contract is round-to-nearest: the operator of the weights chopped towards zero applies differently."""
    api, mesh, io_tetgen, _lib, ctx = env
    s = shapes["b"]
    w = _weights(s, 50)

    def chop(a):
        return (np.asarray(a, np.float64).view(np.uint64) & np.uint64(0xFFFFFFFFE0000000)).view(np.float64)

    op, trunc = _create(api, ctx, s, w, True), _create(api, ctx, s, tuple(chop(a) for a in w), True)
    op.build_reduced()
    x = api.DeviceVector.from_numpy(ctx, _x(s["n"]))
    got, other = _apply(api, ctx, op, -1.0, 0.0, x, True), _apply(api, ctx, trunc, -1.0, 0.0, x, False)
    assert np.mean(bits(got) != bits(other)) >= 0.9
    op.close(), trunc.close()


# ---- 2. idempotence on fp32-exact operators ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["b", "c", "d", "d2"])
def test_dyadic_face_weights_apply_the_same_either_way(env, shapes, name):
    api, mesh, io_tetgen, _lib, ctx = env
    s = shapes[name]
    rng = np.random.default_rng(60)
    f = s["inner"].size
    w = tuple(rng.integers(-256, 257, k) / 64.0 for k in (f, f, s["n"]))  # multiples of 2^-6 in [-4, 4]
    assert all(np.array_equal(a, f32(a)) for a in w)
    op = _create(api, ctx, s, w, True)
    op.build_reduced()
    x = api.DeviceVector.from_numpy(ctx, _x(s["n"]))
    for alpha, beta in COEFS:
        assert same_bits(_apply(api, ctx, op, alpha, beta, x, True), _apply(api, ctx, op, alpha, beta, x, False))
    op.close()


def _dyadic_symmetric(seed=3):
    """test_gpu_cheb.py's _random_symmetric with entries that are multiples of 1/8: every sum the packer forms is exact."""
    import scipy.sparse as sp

    rng = np.random.default_rng(200 + seed)
    n, nnz_row = 777, 6
    rows = np.repeat(np.arange(n), nnz_row)
    cols = (rows + rng.integers(1, n, size=rows.size)) % n
    off = sp.coo_matrix((rng.integers(-16, 17, rows.size) / 8.0, (rows, cols)), shape=(n, n)).tocsr()  # [-2, 2]; a duplicate sums to [-4, 4]
    off.sum_duplicates()
    sym_off = off + off.T  # (entries of [-4, 4] + [-4, 4]: still multiples of 1/8, far inside fp32's 24 bits)
    return (sym_off + sp.diags(np.abs(sym_off).sum(axis=1).A1 * 2.0 + 1.0)).tocsr()


@pytest.mark.parametrize("ell_cap", [0, 4], ids=["no_tail", "tail"])
def test_dyadic_csr_operator_applies_the_same_either_way(env, ell_cap):
    api, mesh, io_tetgen, _lib, ctx = env
    a = _dyadic_symmetric()
    assert np.array_equal(a.data, f32(a.data))
    ctx.set_option("spmv_dict", 0)
    ctx.set_option("ell_cap", ell_cap)
    try:
        op = api.StencilMatrix.from_csr(ctx, a)
    finally:
        ctx.set_option("spmv_dict", 4)
        ctx.set_option("ell_cap", 0)
    st = op.stats()
    assert st["max_row_len"] > 8 and st["value_dictionary_size"] == 0 and (st["tail_nnz"] > 0) == (ell_cap > 0)
    op.build_reduced()
    n = a.shape[0]
    x = api.DeviceVector.from_numpy(ctx, _x(n))
    for alpha, beta in COEFS:
        assert same_bits(_apply(api, ctx, op, alpha, beta, x, True), _apply(api, ctx, op, alpha, beta, x, False))
    assert op.gershgorin_reduced(1.0, 0.0) == op.gershgorin(1.0, 0.0)
    op.close()


# ---- 3. Gershgorin -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["b", "d", "d2"])
def test_reduced_gershgorin_is_that_of_the_rounded_operator(env, shapes, name):
    api, mesh, io_tetgen, _lib, ctx = env
    s = shapes[name]
    w = _weights(s, 70)
    op, ref = _create(api, ctx, s, w, True), _create(api, ctx, s, _rounded(w), True)
    op.build_reduced()
    scale = api.DeviceVector.from_numpy(ctx, np.random.default_rng(71).uniform(-1, 1, s["n"]))
    for alpha, beta in COEFS:
        for sc in (None, scale):
            got, want = op.gershgorin_reduced(alpha, beta, sc), ref.gershgorin(alpha, beta, sc)
            assert got > 0.0 and same_bits([got], [want]), (alpha, beta, sc is not None, got, want)
            assert not same_bits([got], [op.gershgorin(alpha, beta, sc)])  # (the fp64 records give another bound)
    op.close(), ref.close()


# ---- 4. Chebyshev ------------------------------------------------------------------------------------------------------
class _Cheb:
    """storm_hip_cheb_create / _create_reduced through ctypes (an explicit scale, shared by two objects)."""

    def __init__(self, lib, mat, alpha, beta, dinv, degree, reduced):
        self.lib, self.h = lib, C.c_void_p()
        create = lib.storm_hip_cheb_create_reduced if reduced else lib.storm_hip_cheb_create
        self.status = create(mat._h, alpha, beta, None if dinv is None else dinv._h, degree, 0.0, 0.0, C.byref(self.h))

    def apply(self, r, z):
        return self.lib.storm_hip_cheb_apply(self.h, r._h, z._h)

    def get(self, key):
        v = C.c_double()
        assert self.lib.storm_hip_cheb_get(self.h, key.encode(), C.byref(v)) == 0
        return v.value

    def close(self):
        if self.h:
            self.lib.storm_hip_cheb_destroy(self.h)
            self.h = C.c_void_p()


@pytest.mark.parametrize("name", ["b", "c", "d2", "box52"])
@pytest.mark.parametrize("jacobi", [False, True], ids=["unscaled", "jacobi"])
def test_reduced_chebyshev_is_the_ordinary_one_on_the_rounded_operator(env, shapes, name, jacobi):
    api, mesh, io_tetgen, _lib, ctx = env
    lib = _lib.lib
    s = shapes[name]
    n = s["n"]
    w = _weights(s, 80)
    alpha, beta = -0.7, 0.3
    op, ref = _create(api, ctx, s, w, True), _create(api, ctx, s, _rounded(w), True)
    op.build_reduced()
    dinv = None
    if jacobi:  # ONE scale for both objects
        dinv = api.DeviceVector(ctx, n)
        op.diagonal(alpha, beta, dinv, invert=True)
    r_host = np.cos(0.11 * np.arange(n)) + 0.5
    r, z = api.DeviceVector.from_numpy(ctx, r_host), api.DeviceVector(ctx, n)
    keys = ("cheb_fused_applies", "cheb_statement_applies", "cheb_reduced_applies")
    fused_runs = name != "d2"  # (a CSR tail: the statement path by itself)
    try:
        for degree in (1, 2, 3, 8):
            red, plain = _Cheb(lib, op, alpha, beta, dinv, degree, True), _Cheb(lib, ref, alpha, beta, dinv, degree, False)
            assert red.status == 0 and plain.status == 0, lib.storm_hip_last_error()
            assert red.get("reduced") == 1.0 and plain.get("reduced") == 0.0
            for key in ("lambda_min", "lambda_max"):  # both bounds default: the Gershgorin defaults agree
                assert same_bits([red.get(key)], [plain.get(key)]), key
            out = {}
            for fused in (1, 0):
                ctx.set_option("cheb_fused", fused)
                for which, obj in (("reduced", red), ("plain", plain)):
                    z.upload(np.full(n, np.nan))
                    before = [ctx.counter(k) for k in keys]
                    assert obj.apply(r, z) == 0, lib.storm_hip_last_error()
                    out[which, fused] = z.to_numpy()
                    moved = tuple(ctx.counter(k) - b for k, b in zip(keys, before))
                    took_fused = 1 if (fused == 1 and fused_runs) else 0
                    assert moved == (took_fused, 1 - took_fused, 1 if which == "reduced" else 0), (which, fused, moved)
            assert np.array_equal(r.to_numpy(), r_host)  # r is not written
            assert np.isfinite(out["plain", 1]).all() and np.abs(out["plain", 1]).max() > 0.0
            for key, zz in out.items():
                assert same_bits(zz, out["plain", 1]), (degree, key, int(np.sum(bits(zz) != bits(out["plain", 1]))))
            red.close(), plain.close()
    finally:
        ctx.set_option("cheb_fused", 1)
    op.close(), ref.close()


# ---- 5. whole solves ---------------------------------------------------------------------------------------------------
def _ChebOn(api, fixed_op, **kw):
    """A ChebyshevPreconditioner built on a FIXED operator, whatever operator the solve runs on."""

    class Fixed(api.ChebyshevPreconditioner):
        def build(self, x_vec, b_vec, any_op):
            super().build(x_vec, b_vec, fixed_op)

    return Fixed(**kw)


def _solve(api, ctx, solver_cls, op, b_host, pre=None, side=None):
    s = solver_cls()
    s.record_history = True
    if pre is not None:
        s.pre_op, s.pre_side = pre, side
    b, x = api.DeviceVector.from_numpy(ctx, b_host), api.DeviceVector(ctx, b_host.size)
    ok = s.solve(x, b, op)
    return dict(converged=ok, iterations=s.iteration, history=np.array(s.history), x=x.to_numpy())


def _spd16(mesh):
    g = mesh.structured_box(16)
    rng = np.random.default_rng(90)
    w = rng.uniform(0.5, 1.5, g.inner.size)
    return dict(n=g.n_cells, n_halo=0, inner=np.asarray(g.inner, np.int64), outer=np.asarray(g.outer, np.int64), ell_cap=0), \
        (w, w, -rng.uniform(0.1, 1.0, g.n_cells))


@pytest.fixture(scope="module")
def spd_solves(env):
    """CG on A = -M of the 16^3 fixture: plain, and per (degree, side) reduced-on-op(w) against ordinary-on-F(w)."""
    api, mesh, io_tetgen, _lib, ctx = env
    s, w = _spd16(mesh)
    mat, ref = _create(api, ctx, s, w, True), _create(api, ctx, s, _rounded(w), True)
    a_op, f_op = api.HipStencilOperator(mat, -1.0, 0.0), api.HipStencilOperator(ref, -1.0, 0.0)
    b_host = np.ones(s["n"])
    out = dict(fixture=(s, w), plain=_solve(api, ctx, api.CgSolver, a_op, b_host))
    for degree in (2, 4):
        for side_name, side in (("right", api.PreconditionerSide.Right), ("left", api.PreconditionerSide.Left)):
            red = _solve(api, ctx, api.CgSolver, a_op, b_host, api.ChebyshevPreconditioner(degree=degree, reduced_records=True), side)
            plain = _solve(api, ctx, api.CgSolver, a_op, b_host, _ChebOn(api, f_op, degree=degree), side)
            out[degree, side_name] = (red, plain)
    assert mat.reduced_bytes > 0 and ref.reduced_bytes == 0  # built by the preconditioner, on the solve's operator only
    mat.close(), ref.close()
    return out


@pytest.mark.parametrize("degree", [2, 4])
@pytest.mark.parametrize("side", ["right", "left"])
def test_cg_preconditioned_by_the_reduced_object_is_cg_preconditioned_by_the_rounded_operators(spd_solves, degree, side):
    red, plain = spd_solves[degree, side]
    base = spd_solves["plain"]
    print(f"degree {degree} {side}: {red['iterations']} iterations (reduced), {plain['iterations']} (ordinary on F(w)), "
          f"{base['iterations']} unpreconditioned")
    assert red["converged"] and plain["converged"] and base["converged"]
    assert red["iterations"] == plain["iterations"]
    assert same_bits(red["history"], plain["history"])
    assert same_bits(red["x"], plain["x"])
    assert red["iterations"] < base["iterations"]


def test_bicgstab_preconditioned_by_the_reduced_object(env, shapes):
    api, mesh, io_tetgen, _lib, ctx = env
    s = shapes["b"]
    w = s["vel_a"]
    mat, ref = _create(api, ctx, s, w, True), _create(api, ctx, s, _rounded(w), True)
    a_op, f_op = api.HipStencilOperator(mat, 1.0, 0.0), api.HipStencilOperator(ref, 1.0, 0.0)
    b_host = np.random.default_rng(91).uniform(0.5, 1.5, s["n"])
    base = _solve(api, ctx, api.BiCgStabSolver, a_op, b_host)
    for degree in (2, 4):
        for side_name, side in (("right", api.PreconditionerSide.Right), ("left", api.PreconditionerSide.Left)):
            red = _solve(api, ctx, api.BiCgStabSolver, a_op, b_host, api.ChebyshevPreconditioner(degree=degree, reduced_records=True), side)
            plain = _solve(api, ctx, api.BiCgStabSolver, a_op, b_host, _ChebOn(api, f_op, degree=degree), side)
            print(f"degree {degree} {side_name}: {red['iterations']} iterations (reduced), {plain['iterations']} (ordinary on F(w)), "
                  f"{base['iterations']} unpreconditioned")
            assert red["converged"] and plain["converged"] and base["converged"]
            assert red["iterations"] == plain["iterations"]
            assert same_bits(red["history"], plain["history"])
            assert same_bits(red["x"], plain["x"])
            assert red["iterations"] < base["iterations"]
    mat.close(), ref.close()


# ---- 6. refresh --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["b", "d2", "c"])
def test_a_refresh_converts_the_companion_again(env, shapes, name):
    api, mesh, io_tetgen, _lib, ctx = env
    s = shapes[name]
    w0, w1 = _weights(s, 100), _weights(s, 101)
    up = _create(api, ctx, s, w0, True, updatable=True)
    up.build_reduced()
    builds, refreshes = ctx.counter("op_reduced_builds"), ctx.counter("op_reduced_refreshes")
    up.build_reduced()  # a second build is a no-op
    assert ctx.counter("op_reduced_builds") == builds
    x = api.DeviceVector.from_numpy(ctx, _x(s["n"]))
    first = _apply(api, ctx, up, -0.7, 0.3, x, True)
    wi, wo, de = (api.DeviceVector.from_numpy(ctx, a) for a in w1)
    up.set_face_weights(wi, wo, de)
    assert ctx.counter("op_reduced_refreshes") == refreshes + 1 and ctx.counter("op_reduced_builds") == builds
    ref = _create(api, ctx, s, _rounded(w1), True)
    got = _apply(api, ctx, up, -0.7, 0.3, x, True)
    assert same_bits(got, _apply(api, ctx, ref, -0.7, 0.3, x, False))
    assert not same_bits(got, first)
    assert same_bits([up.gershgorin_reduced(-0.7, 0.3)], [ref.gershgorin(-0.7, 0.3)])
    no_companion = _create(api, ctx, s, w0, True, updatable=True)  # without a companion a refresh converts nothing
    no_companion.set_face_weights(wi, wo, de)
    assert ctx.counter("op_reduced_refreshes") == refreshes + 1
    for m in (up, ref, no_companion):
        m.close()


# ---- 7. refusals and lifetime ------------------------------------------------------------------------------------------
def test_refusals_and_lifetime(env, shapes):
    api, mesh, io_tetgen, _lib, ctx = env
    lib = _lib.lib

    def status(call, *args):
        st = call(*[a._h if hasattr(a, "_h") else a for a in args])
        return st, lib.storm_hip_last_error().decode()

    # a compact format (the default spmv_dict on a box), a halo operator
    g = mesh.structured_box(8)
    compact = api.StencilMatrix.from_face_graph(ctx, g)
    assert compact.stats()["value_dictionary_size"] > 0
    st, msg = status(lib.storm_hip_op_build_reduced, compact)
    assert st == E_UNSUPPORTED and "op_build_reduced" in msg and "fp64 records" in msg
    halo = _create(api, ctx, shapes["e"], _weights(shapes["e"], 110), True)
    st, msg = status(lib.storm_hip_op_build_reduced, halo)
    assert st == E_UNSUPPORTED and "single-rank" in msg
    assert compact.reduced_bytes == 0 and halo.reduced_bytes == 0

    s = shapes["b"]
    n = s["n"]
    w = _weights(s, 111)
    op = _create(api, ctx, s, w, True)
    x, y, short = api.DeviceVector.from_numpy(ctx, _x(n)), api.DeviceVector(ctx, n), api.DeviceVector(ctx, n - 1)
    lam, h = C.c_double(), C.c_void_p()

    def refused_without_a_companion():
        st, msg = status(lib.storm_hip_op_apply_reduced, op, 1.0, 0.0, x, y)
        assert st == E_UNSUPPORTED and "no reduced records" in msg, msg
        st, msg = status(lib.storm_hip_op_gershgorin_reduced, op, 1.0, 0.0, None, C.byref(lam))
        assert st == E_UNSUPPORTED and "no reduced records" in msg, msg
        st, msg = status(lib.storm_hip_cheb_create_reduced, op, 1.0, 0.0, None, 2, 0.0, 0.0, C.byref(h))
        assert st == E_UNSUPPORTED and "no reduced records" in msg and not h.value, msg
        assert op.reduced_bytes == 0

    refused_without_a_companion()  # nothing is built behind the caller's back
    before = op.stats()
    op.build_reduced()
    slice_off_sum = 0
    rows = np.zeros(n, np.int64)
    np.add.at(rows, s["inner"], 1), np.add.at(rows, s["outer"], 1)
    for s0 in range(0, n, 64):
        slice_off_sum += 256 + 512 * int(rows[s0:s0 + 64].max())
    assert op.reduced_bytes == slice_off_sum
    assert before["record_bytes"] == sum(512 + 768 * int(rows[s0:s0 + 64].max()) for s0 in range(0, n, 64))
    after = op.stats()
    assert after["device_bytes"] - before["device_bytes"] >= op.reduced_bytes
    assert after["record_bytes"] == before["record_bytes"]  # the stats of the fp64 records do not move
    # sizes, another context
    st, msg = status(lib.storm_hip_op_apply_reduced, op, 1.0, 0.0, short, y)
    assert st == E_INVALID and "2197 rows" in msg
    st, msg = status(lib.storm_hip_op_apply_reduced, op, 1.0, 0.0, x, x)
    assert st == E_INVALID and "alias" in msg
    other = api.Context(0)
    foreign = api.DeviceVector(other, n)
    st, msg = status(lib.storm_hip_op_apply_reduced, op, 1.0, 0.0, foreign, y)
    assert st == E_INVALID and "context" in msg
    st, msg = status(lib.storm_hip_op_gershgorin_reduced, op, 1.0, 0.0, foreign, C.byref(lam))
    assert st == E_INVALID and "scale" in msg
    st, msg = status(lib.storm_hip_cheb_create_reduced, op, 1.0, 0.0, foreign, 2, 0.0, 0.0, C.byref(h))
    assert st == E_INVALID and "another context" in msg
    st, msg = status(lib.storm_hip_cheb_create_reduced, op, 1.0, 0.0, None, 0, 0.0, 0.0, C.byref(h))
    assert st == E_INVALID and "degree" in msg
    other.close()
    # an object outlives a drop: its apply is refused, not a read of freed memory
    st, msg = status(lib.storm_hip_cheb_create_reduced, op, -1.0, 0.0, None, 2, 0.0, 0.0, C.byref(h))
    assert st == 0, msg
    op.drop_reduced()
    assert lib.storm_hip_cheb_apply(h, x._h, y._h) == E_UNSUPPORTED
    lib.storm_hip_cheb_destroy(h)
    h = C.c_void_p()
    assert op.stats()["device_bytes"] == before["device_bytes"]
    refused_without_a_companion()
    op.drop_reduced()  # (a no-op)

    # a weight outside fp32's normal range: refused, and the operator still applies in fp64 with unchanged bits
    for bad in (1e300, 1e-300):
        wb = tuple(a.copy() for a in w)
        wb[1][5] = bad
        big = _create(api, ctx, s, wb, True)
        want = _apply(api, ctx, big, -1.0, 0.0, x, False)
        st, msg = status(lib.storm_hip_op_build_reduced, big)
        assert st == E_UNSUPPORTED and "normal range" in msg, (bad, st, msg)
        assert big.reduced_bytes == 0
        assert same_bits(_apply(api, ctx, big, -1.0, 0.0, x, False), want)
        big.close()
    wb = tuple(a.copy() for a in w)
    wb[2][7] = 1e-300  # ... the diagonal term as well
    big = _create(api, ctx, s, wb, True)
    assert status(lib.storm_hip_op_build_reduced, big)[0] == E_UNSUPPORTED
    big.close()
    with pytest.raises(_lib.StormHipError):
        compact.build_reduced()
    for m in (compact, halo, op):
        m.close()


# ---- 8. C++ ------------------------------------------------------------------------------------------------------------
def test_cpp_driver_solves_with_reduced_records(env, spd_solves, tmp_path):
    exe = os.path.join(ROOT, "tests", "cpp", "cheb_reduced_driver")
    if not os.path.exists(exe):  # (git-ignored: a checkout that arrived without it)
        import __graft_entry__ as ge

        ge.build()
    s, w = spd_solves["fixture"]
    path = tmp_path / "spd16.bin"
    with open(path, "wb") as f:
        f.write(np.array([s["n"], s["inner"].size], np.int64).tobytes())
        for a, t in ((s["inner"], np.int64), (s["outer"], np.int64), (w[0], np.float64), (w[2], np.float64)):
            f.write(np.ascontiguousarray(a, t).tobytes())
    for degree, side in ((2, "right"), (4, "left")):
        red, _ = spd_solves[degree, side]
        out = subprocess.run([exe, str(path), str(degree), side, "1"], check=True, capture_output=True, text=True, timeout=300).stdout
        got = json.loads(out.strip().splitlines()[-1])
        print(got)
        assert got["converged"] and got["reduced"] == 1 and got["op_reduced_builds"] == 1 and got["reduced_bytes"] > 0
        assert got["cheb_reduced_applies"] >= got["pre_applies"] > 0
        assert got["iterations"] == red["iterations"]
        # the same solution: its norm by the device's tree sum against numpy's pairwise sum of the Python solve's x -- two
        # sums of 4 096 non-negative terms in different orders, each within 12 eps of the exact one (log2 n levels)
        ref = float(np.linalg.norm(red["x"]))
        assert abs(got["x_norm2"] - ref) <= 24 * np.finfo(np.float64).eps * ref, (got["x_norm2"], ref)
