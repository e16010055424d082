"""Every vector-statement entry point held to exact elementwise references (tests/exact_ref.py), through the C ABI.

a. Coverage and placement: integer data, compared BITWISE with the integer model.  Rows in streaming blocks of 2048:
   1 .. 12345 (pairs split, the odd tail, a second block); kBlas1NtRows - 1, kBlas1NtRows, + 1 at the default
   blas1_nt = 1 (the size switch itself); and the 2^26 class -- 2^26 - 3, 2^26 (the last single trip of 32768 blocks),
   2^26 + 1 (one row more: the odd tail, which block 0 writes outside the loop), 2^26 + 2 (the first row of the second
   trip), 2^26 + 2049 (a second trip with a partial block and an odd tail), 2^27 + 2051 (a third trip).  Each under blas1_nt 0 and 2, the statements that can wait also under
   lazy_statements 1, alone and as the pair `x += a p; r -= a z` followed by <r, r> -- that sum held to the Python
   integer.  A target the statement does not read is pre-filled with a sentinel.
   At the 2^26 class a vector is 0.5 to 1 GiB on the device and twice that on the host, so NOT the whole cross product
   runs there: one call per kernel template (BIG_TEMPLATES; multi_axpy with k <= 9 only, its inputs four vectors
   repeated in turn) at 2^26 + 2049 rows, and at the other five sizes one call per grid-stride loop the templates are
   instantiated from (BIG_LOOPS: ew_kernel, lin3_kernel, multi_axpy_kernel, map_kernel, lazy_lin_kernel), with
   blas1_nt alternating 0 / 2 from call to call.  multi_axpy with k = 19 and 64 on more than 2^20 rows also repeats
   four input vectors in turn.
b. Aliasing: every combination the header allows, integer data, bitwise, at 2049 and 2^26 + 2049 rows.
c. What surrounds the owned rows stays as it was: the 32-double zero guard in front of element 0, the halo rows and the
   zero padding behind them, read back raw.
d. Rounding form on standard-normal data: every entry point gives exactly ONE admissible form, the same on every
   element (the odd tail included), in every mode, at every size, eager and lazy (lazy_statements 1) -- the one
   EXPECTED names; and the one exception: the fused CG step of lazy_statements 2.
e. Special values against the pinned form evaluated exactly.

Every comparison is bitwise or a set membership; there is no floating-point tolerance in this file."""
import ctypes as C

import numpy as np
import pytest

import exact_ref as er

pytestmark = pytest.mark.gpu

BLK = er.STREAM_BLOCK
NT_ROWS = 6 << 20  # kBlas1NtRows (common.hpp): from here on blas1_nt = 1 streams non-temporally
SMALL = list(er.STMT_SMALL_ROWS)  # (tests/test_exact_reference.py shows which one-line loop edit shows at which of these)
SWITCH = [NT_ROWS - 1, NT_ROWS, NT_ROWS + 1]
BIG_ALL = (1 << 26) + 2049
BIG = list(er.STMT_BIG_ROWS)
assert BIG_ALL in BIG
LONG = 1 << 20  # beyond: a multi_axpy wider than 9 repeats four input vectors in turn

NAMES = sorted(er.INT_STATEMENTS)
LAZY_NAMES = ("copy", "scale", "scaled_copy", "axpy", "xpay", "axpbz")  # lazy.hip: the statements that can wait
# statements that never read the target's old value (unless an operand aliases it): the target starts as the sentinel
BLIND = ("fill", "copy", "scaled_copy", "axpbz", "lin3", "vmul", "vdiv", "vdiv_scalar")
# one statement per kernel template: ew_kernel<FillF, CopyF, ScaleF (both branches), ScaleXF, AxpbzF, BicgPF,
# VmulAddF, VmulF, VdivF (both branches)>, lin3_kernel, map_kernel, multi_axpy_kernel<1 .. 5, 8> and <8> + <1>
BIG_TEMPLATES = ["fill", "copy", "scale", "div_scalar", "scaled_copy", "axpbz", "bicgstab_p", "vmul_add", "vmul", "vdiv",
                 "vdiv_scalar", "lin3", "map", "multi_axpy1", "multi_axpy2", "multi_axpy3", "multi_axpy4", "multi_axpy5",
                 "multi_axpy8", "multi_axpy9"]
BIG_LOOPS = ["axpbz", "lin3", "map", "multi_axpy9"]

# The form each entry point computes, read from the gfx950 assembly of blas1.hip / lazy.hip built with the Makefile's
# flags (-ffp-contract=on; `-S --cuda-device-only`), NOT from a GPU run: per element ew_kernel<AxpbzF> is one
# v_mul_f64 (b z) and one v_fmac_f64 (a x + that) -- the FIRST product of `av * x0 + bv * x1` is the fused one --;
# BicgPF is v_fma_f64 + v_fmac_f64 (both products fused); lin3_kernel v_mul_f64 + two v_fmac_f64 (a x fused into the
# inner sum, s (..) into the outer); VmulAddF v_mul_f64 + v_fmac_f64; multi_axpy_kernel one v_fmac_f64 per term;
# lazy_lin_kernel evaluates AxpbzF's expression.  So `y += a x` is fma(a, x, y), while `y <<= x + b y` rounds b y first
# and adds x to it: fma(1, x, fl(b y)), which is the unfused value.  (include/storm_hip.h has the same table.)
EXPECTED = {"fill": "exact", "copy": "exact", "scale": "exact", "div_scalar": "exact", "scaled_copy": "exact",
            "vmul": "exact", "vdiv": "exact", "vdiv_scalar": "exact", "map": "exact",
            "axpy": "fuse_x", "xpay": "none", "axpbz": "fuse_x", "lin3": "fuse_x/fused", "bicgstab_p": "fuse_z/fused",
            "vmul_add": "prod/fused"}
EXPECTED.update({f"multi_axpy{k}": "fused" for k in er.MULTI_KS})

MAP_PROGRAM = [0, 3 | (0 << 8), 18, 1, 2, 18, 16]  # x0 c0 * x1 y * +   (STORM_HIP_MAP_*: storm_hip.h)


@pytest.fixture(scope="module")
def env():
    from stormruler_amd import _lib, api

    ctx = api.Context(0)
    yield api, _lib, ctx
    ctx.set_option("lazy_statements", 0)
    ctx.set_option("blas1_nt", 1)
    ctx.close()
    _cache.drop()  # (up to a few GiB of host vectors of the 2^26 class)


def _call(_lib, name, h, kind):
    """The entry point of statement ``name`` on the handles ``h`` (target first, exact_ref's operand order) with the
    coefficients of the integer (``I``) or the rounding-form (``R``) model."""
    lib, check = _lib.lib, _lib.check
    c = lambda key: float(getattr(er, f"{kind}_{key}"))  # noqa: E731
    if name == "fill":
        check(lib.storm_hip_fill(h[0], c("FILL")))
    elif name == "copy":
        check(lib.storm_hip_copy(h[0], h[1]))
    elif name == "scale":
        check(lib.storm_hip_scale(h[0], c("SCALE")))
    elif name == "div_scalar":
        check(lib.storm_hip_div_scalar(h[0], c("DIV")))
    elif name == "scaled_copy":  # `y <<= a * x` as both adapters emit it
        check(lib.storm_hip_axpbz(h[0], c("A1"), h[1], 0.0, h[1]))
    elif name == "axpy":
        check(lib.storm_hip_axpy(h[0], c("AXPY"), h[1]))
    elif name == "xpay":
        check(lib.storm_hip_xpay(h[0], h[1], c("XPAY")))
    elif name == "axpbz":
        check(lib.storm_hip_axpbz(h[0], c("A"), h[1], c("B"), h[2]))
    elif name == "lin3":
        check(lib.storm_hip_lin3(h[0], h[1], c("S"), c("A"), h[2], c("B"), h[3]))
    elif name == "bicgstab_p":
        check(lib.storm_hip_bicgstab_p(h[0], h[1], c("BETA"), c("OMEGA"), h[2]))
    elif name == "vmul_add":
        check(lib.storm_hip_vmul_add(h[0], c("VS"), h[1], h[2]))
    elif name == "vmul":
        check(lib.storm_hip_vmul(h[0], h[1], h[2]))
    elif name == "vdiv":
        check(lib.storm_hip_vdiv(h[0], c("VD"), h[1], h[2]))
    elif name == "vdiv_scalar":
        check(lib.storm_hip_vdiv(h[0], c("VD"), None, h[1]))
    elif name == "map":
        prog = (C.c_int32 * len(MAP_PROGRAM))(*MAP_PROGRAM)
        consts = (C.c_double * len(er.MAP_CONSTS))(*er.MAP_CONSTS)
        check(lib.storm_hip_map(h[0], h[1], h[2], prog, len(MAP_PROGRAM), consts, len(er.MAP_CONSTS)))
    else:
        k = int(name[len("multi_axpy"):])
        coefs = er.multi_coefs_int(k) if kind == "I" else er.multi_coefs_real(k)
        check(lib.storm_hip_multi_axpy(h[0], (C.c_double * k)(*coefs), (C.c_void_p * k)(*[v.value for v in h[1:]]), k))


def _same(a, b):
    """Bit for bit.  Long vectors (integer-valued here: no NaN to canonicalise) without the copies er.bits makes."""
    if a.size > LONG:
        return a.shape == b.shape and bool(np.array_equal(a.view(np.uint64), b.view(np.uint64)))
    return er.same_bits(a, b)


def _identity(name):
    return tuple(range(er.INT_STATEMENTS[name][0]))


def _device(api, ctx, name, host, amap, n_halo=0):
    """One device vector per DISTINCT host vector of ``host`` (operand i is host[i]; amap says which are the same
    vector); the target of a statement that does not read it starts as the sentinel.  Returns (vectors, operands)."""
    vecs = {}
    for i, j in enumerate(amap):
        if j not in vecs:
            blind = j == amap[0] and name in BLIND and amap.count(j) == 1
            data = np.full(host[i].size, er.SENTINEL) if blind else host[i]
            vecs[j] = api.DeviceVector.from_numpy(ctx, data, n_halo)
    return vecs, [vecs[j] for j in amap]


def _run(env, name, host, kind, lazy, amap=None):
    """Statement ``name`` on fresh device copies of the fp64 vectors ``host``: the target's values afterwards.
    ``lazy``: the lazy_statements level _modes has set (the option has no getter)."""
    api, _lib, ctx = env
    amap = amap or _identity(name)
    vecs, ops = _device(api, ctx, name, host, amap)
    waits = ctx.counter("lazy_waiting")
    _call(_lib, name, [v._h for v in ops], kind)
    if name in LAZY_NAMES and len(set(amap)) == len(amap):
        assert ctx.counter("lazy_waiting") - waits == (1 if lazy else 0), name
    out = ops[0].to_numpy()
    for j, v in vecs.items():  # the inputs are left alone
        if j != amap[0]:
            assert _same(v.to_numpy(), host[amap.index(j)]), f"{name}: input vector {j} changed"
    return out


def _modes(ctx, name, nts=(0, 2)):
    for nt in nts:
        for lazy in ((0, 1) if name in LAZY_NAMES else (0,)):
            ctx.set_option("blas1_nt", nt)
            ctx.set_option("lazy_statements", lazy)
            yield nt, lazy
    ctx.set_option("lazy_statements", 0)
    ctx.set_option("blas1_nt", 1)


class _Cache:
    """stmt_vector(n, seed) and its fp64 copy, kept while the row count stays the same (a vector of the 2^26 class
    takes seconds to make)."""

    def __init__(self):
        self.n, self.ints, self.reals = None, {}, {}

    def make(self, n, seed):
        if n != self.n:
            self.n, self.ints, self.reals = n, {}, {}
        if seed not in self.ints:
            self.ints[seed] = er.stmt_vector(n, seed)
        return self.ints[seed]

    def drop(self):
        self.n, self.ints, self.reals = None, {}, {}

    def real(self, v):
        if not any(v is w for w in self.ints.values()):
            return v.astype(np.float64)
        key = id(v)
        if key not in self.reals:
            self.reals[key] = v.astype(np.float64)
        return self.reals[key]


_cache = _Cache()


def _int_case(name, n, amap=None):
    """(fp64 operand vectors, the exact result) of the integer model."""
    distinct = 4 if (n > LONG and er.INT_STATEMENTS[name][0] > 10) or n > (1 << 25) else None
    if amap is None:
        ints = er.int_operands(name, n, distinct=distinct, make=_cache.make)
    else:
        ints = er.aliased_operands(name, n, amap, make=_cache.make)
    return [_cache.real(v) for v in ints], er.int_result(name, ints)


def _check_int(env, name, n, nts=(0, 2), amap=None):
    ctx = env[2]
    host, exact = _int_case(name, n, amap)
    assert not np.any(exact == er.SENTINEL)
    for nt, lazy in _modes(ctx, name, nts):
        got = _run(env, name, host, "I", lazy, amap)
        if _same(got, exact):
            continue
        bad = np.flatnonzero(er.bits(got) != er.bits(exact))
        assert bad.size == 0, (f"{name} n={n} nt={nt} lazy={lazy} alias={amap}: {bad.size} rows differ, first {bad[0]} "
                               f"(block {bad[0] // BLK}, row {bad[0] % BLK} of it): got {got[bad[0]]!r}, exact {exact[bad[0]]!r}")


# ---- a. coverage and placement ----------------------------------------------------------------------------------------


@pytest.mark.parametrize("n", SMALL + SWITCH)
def test_every_statement_is_exact_on_integer_data(env, n):
    for name in NAMES:
        _check_int(env, name, n, nts=(0, 1, 2) if n in SWITCH else (0, 2))


def _pair(env, n, nt, lazy, both=True, chained=False):
    """x += 2 p; r -= 2 z; <r, r>  (both = False: the second statement and the sum alone).  With statements waiting the
    sum rides in the kernel of the statement that writes r, lazy_lin_kernel<1, true> (grid clamped to
    partials_capacity), and `x += 2 p`, which neither it nor the sum depends on, keeps waiting (lazy_try_dot) and leaves
    through <1, false>.  chained: x += 2 p; r -= x; <r, r> -- the second statement reads what the first writes, so both
    leave in ONE launch of lazy_lin_kernel<2, true>, the row of x handed over in registers."""
    api, _lib, ctx = env
    xs, ps, rs, zs = (_cache.make(n, 101 + j) for j in range(4))
    x1d = er.int_axpbz(2, ps, 1, xs)
    x1 = x1d.value()
    r1 = er.int_axpbz(-1, x1d.k, 1, rs) if chained else er.int_axpbz(-2, zs, 1, rs)
    rr = er.exact_dot(r1.k, r1.k)
    x, p, r, z = (api.DeviceVector.from_numpy(ctx, _cache.real(v)) for v in (xs, ps, rs, zs))
    ctx.set_option("blas1_nt", nt)
    ctx.set_option("lazy_statements", lazy)
    try:
        dots, pairs = ctx.counter("lazy_fused_dots"), ctx.counter("lazy_fused_pairs")
        if both:
            x += 2.0 * p
        if chained:
            r -= x
        else:
            r -= 2.0 * z
        got = api.dot_product(r, r)
        assert ctx.counter("lazy_fused_dots") - dots == (1 if lazy else 0)
        assert ctx.counter("lazy_fused_pairs") - pairs == (1 if lazy and chained else 0)
        assert ctx.counter("lazy_waiting") == (1 if lazy and both and not chained else 0)
    finally:
        ctx.set_option("lazy_statements", 0)
        ctx.set_option("blas1_nt", 1)
    tag = f"n={n} nt={nt} lazy={lazy} both={both} chained={chained}"
    assert got == float(rr), tag
    assert _same(r.to_numpy(), r1.value()), tag
    if both:
        assert _same(x.to_numpy(), x1), tag


@pytest.mark.parametrize("n", SMALL + SWITCH)
def test_the_cg_update_pair_and_its_sum_are_exact(env, n):
    for nt in (0, 2):
        for lazy in (0, 1):
            _pair(env, n, nt, lazy)
            _pair(env, n, nt, lazy, both=False)
            _pair(env, n, nt, lazy, chained=True)


@pytest.mark.parametrize("n", BIG)
def test_every_loop_is_exact_beyond_one_trip_of_the_grid(env, n):
    """The 2^26 class: see the module docstring for which calls run where."""
    api, _lib, ctx = env
    names = BIG_TEMPLATES if n == BIG_ALL else BIG_LOOPS
    for i, name in enumerate(names):
        _check_int(env, name, n, nts=(2 * (i & 1),))
    # the statements' own kernels: lazy_lin_kernel<2, true> (two chained statements with the sum riding) at every size;
    # <1, true> and <1, false> (the CG pair; one statement with the sum), <2, false> (two statements, no sum) once
    _pair(env, n, 0, 1, chained=True)
    if n == BIG_ALL:
        _pair(env, n, 0, 1)
        _pair(env, n, 2, 1, both=False)
        _pair(env, n, 2, 0)
        host, exact = _int_case("axpy", n)
        host2, exact2 = _int_case("scaled_copy", n)
        ctx.set_option("lazy_statements", 1)
        try:
            a = _device(api, ctx, "axpy", host, _identity("axpy"))[1]
            b = _device(api, ctx, "scaled_copy", host2, _identity("scaled_copy"))[1]
            pairs = ctx.counter("lazy_fused_pairs")
            _call(_lib, "axpy", [v._h for v in a], "I")
            _call(_lib, "scaled_copy", [v._h for v in b], "I")
            assert ctx.counter("lazy_waiting") == 2
            got = a[0].to_numpy()
            assert ctx.counter("lazy_fused_pairs") - pairs == 1
        finally:
            ctx.set_option("lazy_statements", 0)
        assert _same(got, exact) and _same(b[0].to_numpy(), exact2)


# ---- b. aliasing --------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", sorted(er.ALIASINGS))
@pytest.mark.parametrize("n", [2049, BIG_ALL])  # (n varies slowest: the 2^26-class vectors are made once for all seven statements)
def test_aliased_operands_are_exact(env, name, n):
    for i, amap in enumerate(er.ALIASINGS[name]):
        _check_int(env, name, n, nts=(0, 2) if n < LONG else (2 * (i & 1),), amap=amap)


def test_multi_axpy_refuses_an_input_that_is_the_target(env):
    """The kernel loads a chunk's x_j before it updates y (declared __restrict__) and a second chunk sees the first
    one's y: `xs[j] is y` is neither y += sum c_j x_j on the old y nor the sequential statements.  Refused."""
    api, _lib, ctx = env
    host = [v.astype(np.float64) for v in er.int_operands("multi_axpy9", 2049)]
    dev = [api.DeviceVector.from_numpy(ctx, v) for v in host]
    for j in (0, 3, 8):
        xs = dev[1:]
        xs[j] = dev[0]
        with pytest.raises(_lib.StormHipError, match=f"xs\\[{j}\\] aliases y"):
            api.multi_axpy(dev[0], er.multi_coefs_int(9), xs)
        assert er.same_bits(dev[0].to_numpy(), host[0])
    api.multi_axpy(dev[0], er.multi_coefs_int(9), [dev[1]] * 9)  # (inputs may repeat among themselves)


# ---- c. what surrounds the owned rows ---------------------------------------------------------------------------------

VEC_GUARD = 32  # kVecGuard (common.hpp): zero doubles in front of element 0
HALO_MARK = 4.0e300


def _padded(n_rows):
    """Doubles from element 0 to the end of the allocation: context.hip, vec_create_impl --
    `bytes = sizeof(double) * (kVecGuard + (n_owned + n_halo + 3) / 4 * 4 + 4)`."""
    return (n_rows + 3) // 4 * 4 + 4


def _hip_runtime():
    """The HIP runtime the library has already loaded into this process."""
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    assert len(paths) == 1, paths
    hip = C.CDLL(paths.pop())
    hip.hipMemcpy.restype = C.c_int
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return hip


def _device_ptr(_lib, v):
    p = C.c_void_p()
    _lib.check(_lib.lib.storm_hip_vec_device_ptr(v._h, C.byref(p)))
    return p.value


SURROUND = [(arena, n, halo) for arena, sizes in ((0, (2049, 4098, 270001, 270002)), (1, (270001, 270002)))
            for n in sizes for halo in (0, 1, 5, 240)]  # (an arena holds vectors of at least 1 MiB: context.hip arena_take)


def _arena_pitch(n_rows):
    """The distance between two vectors of an arena: context.hip, arena_take -- the allocation rounded up to a multiple
    of 4 MiB, then 2 MiB less if the vector still fits, 2 MiB more if not."""
    nbytes, mib = 8 * (VEC_GUARD + _padded(n_rows)), 1 << 20
    pitch = -(-nbytes // (4 * mib)) * (4 * mib)
    return pitch - 2 * mib if pitch - 2 * mib >= nbytes else pitch + 2 * mib


@pytest.mark.parametrize("arena", [0, 1])
def test_statements_leave_guard_halo_and_padding_alone(arena):
    """Every paired, lattice and marching SpMV kernel relies on the guard and the padding being ZERO: a weight-0 slot
    times a stray non-finite value there is a NaN in y.  In an arena the neighbour is another vector's guard."""
    from stormruler_amd import _lib, api

    ctx = api.Context(0)
    ctx.set_option("vec_arena", arena)
    hip = _hip_runtime()
    try:
        probes = []
        if arena:
            # The library has no counter for it, so an address test: the first two vectors of a size class are the
            # first two slots of a fresh arena, exactly one pitch apart (6 MiB for these 2.2 MB vectors: not a
            # distance two allocations of their own would be at).  So arena_take does not decline these sizes and the
            # arm below is not vec_arena = 0 again.  (The two stay alive to the end: slots 0 and 1 are taken.)
            n, halo = SURROUND[-1][1:]
            probes = [api.DeviceVector(ctx, n, halo) for _ in range(2)]
            d0, d1 = (_device_ptr(_lib, v) for v in probes)
            assert d1 - d0 == _arena_pitch(n + halo) == 6 << 20, (n, halo, d1 - d0)
        for _, n, halo in [c for c in SURROUND if c[0] == arena]:
            for name in NAMES:
                for lazy in ((0, 1) if name in LAZY_NAMES else (0,)):
                    ints = er.int_operands(name, n)
                    host = [v.astype(np.float64) for v in ints]
                    exact = er.int_result(name, ints)
                    amap = _identity(name)
                    vecs, ops = _device(api, ctx, name, host, amap, n_halo=halo)
                    ptrs = {j: _device_ptr(_lib, v) for j, v in vecs.items()}
                    mark = np.full(halo, HALO_MARK)
                    for p in ptrs.values():
                        if halo:
                            assert hip.hipMemcpy(p + 8 * n, mark.ctypes.data, 8 * halo, 1) == 0  # host to device
                    ctx.set_option("lazy_statements", lazy)
                    _call(_lib, name, [v._h for v in ops], "I")
                    ctx.set_option("lazy_statements", 0)
                    ctx.sync()
                    for j, p in ptrs.items():  # the raw reads last
                        raw = np.empty(VEC_GUARD + _padded(n + halo))
                        assert hip.hipMemcpy(raw.ctypes.data, p - 8 * VEC_GUARD, raw.nbytes, 2) == 0  # device to host
                        tag = f"{name} n={n} halo={halo} arena={arena} lazy={lazy} vector {j}"
                        own = raw[VEC_GUARD:VEC_GUARD + n]
                        assert er.same_bits(own, exact if j == amap[0] else host[amap.index(j)]), tag
                        assert not raw[:VEC_GUARD].view(np.uint64).any(), f"{tag}: the guard is not zero"
                        assert er.same_bits(raw[VEC_GUARD + n:VEC_GUARD + n + halo], mark), f"{tag}: halo rows changed"
                        assert not raw[VEC_GUARD + n + halo:].view(np.uint64).any(), f"{tag}: the padding is not zero"
        del probes
    finally:
        ctx.close()


# ---- d. rounding form ---------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", sorted(er.REAL_STATEMENTS))
def test_every_entry_point_computes_its_one_rounding_form(env, name):
    """If the GPU disagrees with EXPECTED, or body and tail disagree, that is a finding to explain, not a table to
    edit: the table is the contract include/storm_hip.h states."""
    ctx = env[2]
    for n in er.real_rows(name):
        host, forms = er.real_operands(name, n)
        assert EXPECTED[name] in forms
        for nt, lazy in _modes(ctx, name):
            got = _run(env, name, host, "R", lazy)
            which = er.classify(got, forms)
            if which != [EXPECTED[name]]:
                body, tail = er.classify(got[:n & ~1], {k: v[:n & ~1] for k, v in forms.items()}), \
                    er.classify(got[n - 1:], {k: v[n - 1:] for k, v in forms.items()})
                raise AssertionError(f"{name} n={n} nt={nt} lazy={lazy}: forms {which}, expected [{EXPECTED[name]}]; "
                                     f"paired rows alone {body}, last row alone {tail}")


def test_the_fused_cg_step_of_level_two_is_the_named_exception():
    """lazy_statements = 2 on a lattice operator: `x += a p; p <<= r + b p; z = A p; <p, z>` leaves as the library's
    fused CG step (lazy.hip try_cg_step -> cg_step_march_kernel, which computes `__builtin_fma(cg_b, p, r)` and
    `__builtin_fma(cg_a, p, x)`: spmv_lattice.hip).  There storm_hip_xpay is fma(b, y, x) -- the form `fuse_z`, NOT the
    table's `none` -- and storm_hip_axpy is fma(a, x, y) as everywhere: the one exception include/storm_hip.h names.
    At levels 0 and 1 the same four calls give the table's forms."""
    from stormruler_amd import _lib, api, mesh

    ctx = api.Context(0)
    try:
        ctx.set_option("spmv_canon_tile_min_rows", 0)  # (a 15 k-row lattice on the kernels of the large ones)
        g = mesh.structured_box(32, 24, 20)
        mat = api.StencilMatrix.from_face_graph(ctx, g)
        n = g.n_cells
        rng = np.random.default_rng(77)
        x0, p0, r0 = (rng.standard_normal(n) for _ in range(3))
        x_forms = er.forms_axpbz(er.R_AXPY, p0, 1.0, x0)
        p_forms = er.forms_axpbz(1.0, r0, er.R_XPAY, p0)
        for forms in (x_forms, p_forms):  # the fixture tells the forms apart
            assert min(er.differing_share(forms).values()) >= 0.01
        for level, p_form in ((0, "none"), (1, "none"), (2, "fuse_z")):
            x, p, r = (api.DeviceVector.from_numpy(ctx, v) for v in (x0, p0, r0))
            z = api.DeviceVector(ctx, n)
            steps = ctx.counter("lazy_cg_steps")
            ctx.set_option("lazy_statements", level)
            try:
                _lib.check(_lib.lib.storm_hip_axpy(x._h, er.R_AXPY, p._h))
                _lib.check(_lib.lib.storm_hip_xpay(p._h, r._h, er.R_XPAY))
                mat.apply(-1.0, 0.0, p, z)
                api.dot_product(p, z)
            finally:
                ctx.set_option("lazy_statements", 0)
            assert ctx.counter("lazy_cg_steps") - steps == (1 if level == 2 else 0), level
            assert er.classify(p.to_numpy(), p_forms) == [p_form], level
            assert er.classify(x.to_numpy(), x_forms) == ["fuse_x"], level
        mat.close()
    finally:
        ctx.close()


# ---- e. special values --------------------------------------------------------------------------------------------------

DBL_MAX, TRUE_MIN = 1.7976931348623157e308, 5e-324
SPECIAL = [0.0, -0.0, np.inf, -np.inf, np.nan, DBL_MAX, -DBL_MAX, TRUE_MIN, -TRUE_MIN, 1.0e-310, 1.5, -2.75, 3.0e150]


@pytest.mark.parametrize("name", sorted(er.REAL_STATEMENTS))
def test_special_values(env, name):
    """Operand j is SPECIAL rotated by 3 j places: pairs straddle the special values, and with 13 rows one of them sits
    in the odd tail of every operand (3e150, a subnormal, -DBL_MAX, -inf ...); 14 rows: no tail.  Expected: numpy's
    evaluation of the reference's expression (a * x, y + a * x, x / s ...) where the entry point's form has no fused
    step; where it has one, that form (EXPECTED) evaluated exactly -- an fma does not overflow where fl(a x) does, so
    `DBL_MAX * c - DBL_MAX` style rows legitimately differ from the unfused expression.  Bit patterns, all NaNs equal."""
    ctx = env[2]
    count, fn = er.REAL_STATEMENTS[name]
    for extra in ([], [1.0]):
        host = [np.array(list(np.roll(SPECIAL, 3 * j)) + extra) for j in range(count)]
        exact = fn(host)[EXPECTED[name]]
        for nt, lazy in _modes(ctx, name):
            got = _run(env, name, host, "R", lazy)
            bad = np.flatnonzero(er.bits(got) != er.bits(exact))
            assert bad.size == 0, (f"{name} nt={nt} lazy={lazy} rows={len(got)}: row {bad[0]} of operands "
                                   f"{[h[bad[0]] for h in host]}: got {got[bad[0]]!r}, expected {exact[bad[0]]!r}")
