"""Updatable face-weight operators (csrc/op_update.hip): an operator whose weights ``set_face_weights`` rewrote on the
device is, bit for bit, the operator a fresh create with those weights gives -- apply, apply_add, block apply, diagonal,
Gershgorin bound, GMRES / BiCGStab / CG -- on the smallest shapes at which the slot addressing can go wrong:

  a   5x4x3 box: 60 rows, one ragged slice, even width
  b   13^3 box, convection-diffusion weights, faces randomly permuted and flipped: 35 slices, ragged last, the order
      inside a row differs from the natural one
  c   the reference's triangles (square_nb.1): rows of <= 3 neighbours, the odd, column-major last slot
  d   a 200-cell ring and a hub joined to every cell: one row of 200 entries, most of them in the CSR tail
  d2  shape b under ell_cap = 2: a tail in every row
  e   shape a with its last plane as halo columns: n_owned = 40, n_halo = 20
  f   three cells, no faces: ext only

and a time loop whose coefficients never leave the device (variable-mobility diffusion), in Python and in C++."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_UNSUPPORTED = -1, -6
NU, VEL_A, VEL_B = 1e-2, (1.0, 0.5, 0.25), (-0.3, 0.8, 0.6)


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


def _box_faces(nx, ny, nz, owned_planes):
    """Faces cell by cell (+x, +y, +z of each) of the owned planes; the plane behind them is the halo."""
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
    """Faces randomly permuted and randomly flipped; ``arrays``: pairs (w_inner, w_outer) flipped with them."""
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
    wa, wb = mesh.convection_diffusion_weights(g, NU, VEL_A), mesh.convection_diffusion_weights(g, NU, VEL_B)
    i, o, (fa, fb) = _shuffled(g.inner, g.outer, [(wa[0], wa[1]), (wb[0], wb[1])])
    out["b"] = dict(n=g.n_cells, n_halo=0, inner=i, outer=o, ell_cap=0, vel_a=(fa[0], fa[1], wa[2]), vel_b=(fb[0], fb[1], wb[2]))
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
    return out


def _weights(s, seed):
    rng = np.random.default_rng(seed)
    f = s["inner"].size
    return rng.uniform(-1, 1, f), rng.uniform(-1, 1, f), rng.uniform(-1, 1, s["n"])


def _create(api, ctx, s, w, diag, updatable, dict0=False):
    ctx.set_option("ell_cap", s["ell_cap"])
    if dict0:
        ctx.set_option("spmv_dict", 0)
    try:
        make = api.StencilMatrix.from_face_weights_updatable if updatable else api.StencilMatrix.from_face_weights
        return make(ctx, s["n"], s["n_halo"], s["inner"], s["outer"], w[0], w[1], w[2] if diag else None)
    finally:
        ctx.set_option("ell_cap", 0)
        ctx.set_option("spmv_dict", 4)


def _hip_runtime():
    """The HIP runtime this process has loaded already (the one libstorm_hip.so runs on)."""
    with open("/proc/self/maps") as maps:
        path = next(line.split()[-1] for line in maps if "libamdhip64.so" in line)
    return C.CDLL(path)


def _vector_with_halo(api, _lib, ctx, values, n_owned):
    """A vector of n_owned rows whose halo tail holds values[n_owned:] (no exchange: written through the device pointer)."""
    v = api.DeviceVector.from_numpy(ctx, values[:n_owned], values.size - n_owned)
    if values.size > n_owned:
        hip = _hip_runtime()
        p = C.c_void_p()
        _lib.check(_lib.lib.storm_hip_vec_device_ptr(v._h, C.byref(p)))
        ctx.sync()
        tail = np.ascontiguousarray(values[n_owned:], np.float64)
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        assert hip.hipMemcpy(C.c_void_p(p.value + 8 * n_owned), tail.ctypes.data_as(C.c_void_p), tail.nbytes, 1) == 0
    return v


def _set(api, ctx, mat, w, diag):
    wi, wo = api.DeviceVector.from_numpy(ctx, w[0]), api.DeviceVector.from_numpy(ctx, w[1])
    mat.set_face_weights(wi, wo, api.DeviceVector.from_numpy(ctx, w[2]) if diag else None)


def _everything(api, _lib, ctx, s, mat, x_all, y0, xb):
    """Every value-reading entry point of an operator on fixed inputs, as arrays."""
    n = s["n"]
    x = _vector_with_halo(api, _lib, ctx, x_all, n)
    out = {}
    y = api.DeviceVector(ctx, n)
    mat.apply(-0.7, 0.3, x, y)
    out["apply"] = y.to_numpy()
    ya = api.DeviceVector.from_numpy(ctx, y0)
    mat.apply_add(-0.7, x, ya)
    out["apply_add"] = ya.to_numpy()
    d = api.DeviceVector(ctx, n)
    mat.diagonal(-0.7, 0.3, d)
    out["diagonal"] = d.to_numpy()
    if s["n_halo"] == 0:
        out["gershgorin"] = np.array([mat.gershgorin(-0.7, 0.3)])
        xbv, ybv = api.BlockVector.from_numpy(ctx, xb), api.BlockVector(ctx, n, 2)
        api.HipStencilOperator(mat, -0.7, 0.3).mul_block(ybv, xbv)
        out["apply_block"] = ybv.to_numpy()
    return out


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "d2", "e", "f"])
@pytest.mark.parametrize("diag", [True, False], ids=["diag_random", "diag_null"])
def test_refreshed_operator_is_the_fresh_one_bit_for_bit(env, shapes, name, diag):
    api, mesh, io_tetgen, _lib, ctx = env
    s = shapes[name]
    n, nt = s["n"], s["n"] + s["n_halo"]
    w0, w1 = _weights(s, 10), _weights(s, 11)
    rng = np.random.default_rng(12)
    x_all, y0, xb = rng.uniform(-1, 1, nt), rng.uniform(-1, 1, n), rng.uniform(-1, 1, (n, 2))
    updates0 = ctx.counter("op_face_updates")
    up = _create(api, ctx, s, w0, diag, True)
    assert up.face_count == s["inner"].size
    st = up.stats()
    assert st["value_dictionary_size"] == 0 and st["paired_rows"] == 0
    if name in ("d", "d2"):
        assert st["tail_nnz"] > 0
    before = _everything(api, _lib, ctx, s, up, x_all, y0, xb)
    _set(api, ctx, up, w1, diag)
    got = _everything(api, _lib, ctx, s, up, x_all, y0, xb)
    fresh_up = _create(api, ctx, s, w1, diag, True)
    fresh_def = _create(api, ctx, s, w1, diag, False, dict0=True)
    assert fresh_def.face_count == 0
    for ref in (_everything(api, _lib, ctx, s, fresh_up, x_all, y0, xb), _everything(api, _lib, ctx, s, fresh_def, x_all, y0, xb)):
        assert sorted(ref) == sorted(got)
        for key in got:
            assert same_bits(got[key], ref[key]), key
    if s["inner"].size:
        assert not same_bits(got["apply"], before["apply"])  # (the refresh did change something)
    _set(api, ctx, up, w0, diag)  # w0 -> w1 -> w0 restores the original bits
    back = _everything(api, _lib, ctx, s, up, x_all, y0, xb)
    for key in before:
        assert same_bits(back[key], before[key]), key
    assert ctx.counter("op_face_updates") == updates0 + 2
    for m in (up, fresh_up, fresh_def):
        m.close()


@pytest.mark.parametrize("name", ["b", "c", "e"])
def test_cells_to_faces_is_numpys_gather(env, shapes, name):
    api, mesh, io_tetgen, _lib, ctx = env
    s = shapes[name]
    n, f = s["n"], s["inner"].size
    cell = np.random.default_rng(20).uniform(-1, 1, n + s["n_halo"])
    mat = _create(api, ctx, s, _weights(s, 21), False, True)
    c = _vector_with_halo(api, _lib, ctx, cell, n)
    ai, ao = api.DeviceVector(ctx, f), api.DeviceVector(ctx, f)
    mat.cells_to_faces(c, ai, ao)
    assert same_bits(ai.to_numpy(), cell[s["inner"]]) and same_bits(ao.to_numpy(), cell[s["outer"]])
    only_i, only_o = api.DeviceVector(ctx, f), api.DeviceVector(ctx, f)
    mat.cells_to_faces(c, only_i, None)
    mat.cells_to_faces(c, None, only_o)
    assert same_bits(only_i.to_numpy(), cell[s["inner"]]) and same_bits(only_o.to_numpy(), cell[s["outer"]])
    mat.close()


def test_refusals(env, shapes):
    api, mesh, io_tetgen, _lib, ctx = env
    lib = _lib.lib
    s = shapes["a"]
    n, f = s["n"], s["inner"].size
    w = _weights(s, 30)
    up, plain = _create(api, ctx, s, w, False, True), _create(api, ctx, s, w, False, False)
    wf, wrong, cell, short = (api.DeviceVector(ctx, k) for k in (f, f + 1, n, n - 1))
    halo_face = api.DeviceVector(ctx, f - 1, 1)
    other = api.Context(0)
    foreign_f, foreign_c = api.DeviceVector(other, f), api.DeviceVector(other, n)

    def status(call, *args):
        st = call(*[a._h if hasattr(a, "_h") else a for a in args])
        return st, lib.storm_hip_last_error().decode()

    set_w, c2f = lib.storm_hip_op_set_face_weights, lib.storm_hip_op_cells_to_faces
    st, msg = status(set_w, plain, wf, wf, None)
    assert st == E_UNSUPPORTED and "60 rows" in msg
    st, msg = status(c2f, plain, cell, wf, wf)
    assert st == E_UNSUPPORTED and "60 rows" in msg
    for args in ((None, wf, wf, None), (up, None, wf, None), (up, wf, None, None)):
        st, msg = status(set_w, *args)
        assert st == E_INVALID and "null" in msg
    for args in ((None, cell, wf, wf), (up, None, wf, wf)):
        st, msg = status(c2f, *args)
        assert st == E_INVALID and "null" in msg
    n64 = C.c_int64()
    assert lib.storm_hip_op_face_count(None, C.byref(n64)) == E_INVALID and lib.storm_hip_op_face_count(up._h, None) == E_INVALID
    for args in ((up, wrong, wf, None), (up, wf, wrong, None), (up, halo_face, wf, None)):
        st, msg = status(set_w, *args)
        assert st == E_INVALID and f"{f} faces" in msg, msg
    st, msg = status(set_w, up, wf, wf, short)
    assert st == E_INVALID and "60 rows" in msg and "59" in msg
    for args in ((up, short, wf, wf), (up, cell, wrong, wf), (up, cell, wf, wrong)):
        st, msg = status(c2f, *args)
        assert st == E_INVALID and (f"{f} faces" in msg or "60 rows" in msg), msg
    for call, args in ((set_w, (up, foreign_f, wf, None)), (set_w, (up, wf, foreign_f, None)), (set_w, (up, wf, wf, foreign_c)),
                       (c2f, (up, foreign_c, wf, wf)), (c2f, (up, cell, foreign_f, wf)), (c2f, (up, cell, wf, foreign_f))):
        st, msg = status(call, *args)
        assert st == E_INVALID and "another context" in msg, msg
    with pytest.raises(_lib.StormHipError):
        plain.set_face_weights(wf, wf)
    other.close()
    up.close(), plain.close()


def _solve(api, ctx, kind, mat, b_host, alpha=1.0):
    s = {"gmres": api.GmresSolver, "bicgstab": api.BiCgStabSolver, "cg": api.CgSolver}[kind]()
    if kind == "gmres":
        s.num_inner_iterations = 30
    b, x = api.DeviceVector.from_numpy(ctx, b_host), api.DeviceVector(ctx, b_host.size)
    assert s.solve(x, b, api.HipStencilOperator(mat, alpha, 0.0))
    return s.iteration, x.to_numpy()


def test_solves_on_a_refreshed_operator_are_those_on_a_fresh_one(env, shapes):
    api, mesh, io_tetgen, _lib, ctx = env
    s = shapes["b"]
    b_host = np.random.default_rng(40).uniform(0.5, 1.5, s["n"])
    fresh = _create(api, ctx, s, s["vel_b"], True, True)
    # the project's standing property first: two solves on one operator agree bit for bit (order-fixed reductions)
    it1, x1 = _solve(api, ctx, "gmres", fresh, b_host)
    it2, x2 = _solve(api, ctx, "gmres", fresh, b_host)
    assert it1 == it2 and same_bits(x1, x2)
    up = _create(api, ctx, s, s["vel_a"], True, True)
    it_a, x_a = _solve(api, ctx, "gmres", up, b_host)
    _set(api, ctx, up, s["vel_b"], True)
    it_u, x_u = _solve(api, ctx, "gmres", up, b_host)
    assert it_u == it1 and same_bits(x_u, x1)
    assert not same_bits(x_a, x1)
    it_f, x_f = _solve(api, ctx, "bicgstab", fresh, b_host)
    it_u, x_u = _solve(api, ctx, "bicgstab", up, b_host)
    assert it_u == it_f and same_bits(x_u, x_f)
    # CG on the symmetric part alone: A_s = (w_inner + w_outer) / 2 on both sides (uniform volumes), diagonal kept
    sym = {k: (0.5 * (s[k][0] + s[k][1]), 0.5 * (s[k][0] + s[k][1]), s[k][2]) for k in ("vel_a", "vel_b")}
    fresh_s = _create(api, ctx, s, sym["vel_b"], True, True)
    up_s = _create(api, ctx, s, sym["vel_a"], True, True)
    _set(api, ctx, up_s, sym["vel_b"], True)
    it_f, x_f = _solve(api, ctx, "cg", fresh_s, b_host)
    it_u, x_u = _solve(api, ctx, "cg", up_s, b_host)
    assert it_u == it_f and same_bits(x_u, x_f)
    for m in (fresh, up, fresh_s, up_s):
        m.close()


# ---- a loop that never leaves the device ------------------------------------------------------------------------------
NX, NY, NZ, DT, STEPS = 6, 5, 4, 0.025, 5


def _mobility_problem():
    inner, outer = _box_faces(NX, NY, NZ, NZ)
    step = np.array([1, NX, NX * NY])
    g = np.array([36.0, 25.0, 16.0])[np.searchsorted(step, outer - inner)]  # 1 / h^2 of the face's direction
    n = NX * NY * NZ
    c0 = ((np.arange(n) * 37) % 101) / 101.0
    return n, inner, outer, g, c0


def _run_python_loop(api, ctx):
    """The loop with stormruler_amd.api; per step what the checks need (downloads are the checks', not the loop's)."""
    n, inner, outer, g, c0 = _mobility_problem()
    f = inner.size
    mat = api.StencilMatrix.from_face_weights_updatable(ctx, n, 0, inner, outer, np.zeros(f), np.zeros(f))
    c, gf = api.DeviceVector.from_numpy(ctx, c0), api.DeviceVector.from_numpy(ctx, g)
    ci, co, m, w = (api.DeviceVector(ctx, f) for _ in range(4))
    op = api.HipStencilOperator(mat, -DT, 1.0)
    steps = []
    updates0 = ctx.counter("op_face_updates")
    for _ in range(STEPS):
        c_n = c.to_numpy()
        mat.cells_to_faces(c, ci, co)
        m <<= api.map(lambda a, b: 0.5 * ((0.1 + a * a) + (0.1 + b * b)), ci, co)
        w <<= api.map(lambda mf, gg: mf * gg, m, gf)
        mat.set_face_weights(w, w)
        x = api.DeviceVector(ctx, n)
        s = api.CgSolver()
        s.absolute_error_tolerance, s.relative_error_tolerance = 0.0, 1e-12
        ok = s.solve(x, c, op)
        c <<= 1.0 * x
        steps.append(dict(c_n=c_n, w=w.to_numpy(), c_next=c.to_numpy(), converged=ok, iterations=s.iteration,
                          gershgorin=mat.gershgorin(1.0, 0.0), w_norm2=api.norm_2(w), c_norm2=api.norm_2(c)))
    updates = ctx.counter("op_face_updates") - updates0
    mat.close()
    return dict(steps=steps, updates=updates)


@pytest.fixture(scope="module")
def python_loop(env):
    api, mesh, io_tetgen, _lib, ctx = env
    return _run_python_loop(api, ctx)


def test_variable_mobility_loop_stays_on_the_device(env, python_loop):
    n, inner, outer, g, c0 = _mobility_problem()
    assert python_loop["updates"] == STEPS  # one refresh per step, and the operator was created once, before the loop
    for k, st in enumerate(python_loop["steps"]):
        c_n = st["c_n"]
        a, b = c_n[inner], c_n[outer]
        w_ref = (0.5 * ((0.1 + a * a) + (0.1 + b * b))) * g
        assert same_bits(st["w"], w_ref), k  # map is exactly rounded
        assert DT * st["gershgorin"] <= 9.0, (k, st["gershgorin"])  # condition number of I - dt L at most 10
        lap = np.zeros((n, n))
        np.add.at(lap, (inner, outer), st["w"]), np.add.at(lap, (inner, inner), -st["w"])
        np.add.at(lap, (outer, inner), st["w"]), np.add.at(lap, (outer, outer), -st["w"])
        ref = np.linalg.solve(np.eye(n) - DT * lap, c_n)  # from the DEVICE's c^n: steps do not compound
        err = np.abs(st["c_next"] - ref).max() / np.abs(ref).max()
        print(f"step {k}: {st['iterations']} iterations, dt * gershgorin = {DT * st['gershgorin']:.3f}, error {err:.3e}")
        assert st["converged"]
        assert err <= 1e-10, (k, err)  # 1e-12 of the solver x the condition bound 10 x a margin of 10 for rounding


def test_no_operator_is_created_inside_the_loop():
    """The loop's source holds one create call, in front of the ``for``."""
    import inspect

    src = inspect.getsource(_run_python_loop)
    head, body = src.split("for _ in range(STEPS):")
    assert head.count("from_face_weights_updatable(") == 1
    assert "from_face_weights" not in body and "from_csr" not in body and "from_face_graph" not in body


def test_cpp_driver_runs_the_same_loop(python_loop):
    exe = os.path.join(ROOT, "tests", "cpp", "face_update_driver")
    if not os.path.exists(exe):  # (git-ignored: a checkout that arrived without it)
        import __graft_entry__ as ge

        ge.build()
    out = subprocess.run([exe, str(STEPS)], check=True, capture_output=True, text=True, timeout=300).stdout
    lines = [json.loads(ln) for ln in out.strip().splitlines()]
    assert lines[-1] == {"op_face_updates": STEPS}
    assert len(lines) == STEPS + 1
    for k, (got, st) in enumerate(zip(lines[:-1], python_loop["steps"])):
        assert got["step"] == k and got["converged"] and got["iterations"] == st["iterations"]
        assert same_bits(np.array([got["w_norm2"], got["c_norm2"]]), np.array([st["w_norm2"], st["c_norm2"]])), (k, got, st)
