"""Every BLAS-1 and lazy-statement reduction held to the bit against exact integer sums.

On integer data whose every partial sum stays below 2^53 (tests/exact_ref.py) a correct reduction returns the exact
sum whatever its order, so a fold that drops, doubles or shortens a range of partials cannot hide behind a tolerance
or behind a second path that shares the bug.  Row counts sit at every change of the fold's shape, in streaming blocks
of kStreamBlockElems = 2048 rows:
    1 .. 2049                    one block, a scalar tail, the first second block
    64 / 65 blocks (+1 row)      one ticket group full, a second group one block long
    8192 blocks, +1 row, 8193    the last single-pass fold of the partials; the first two-pass (reduce_stage1_kernel)
    2^26, 2^26 + 1               kMaxStreamBlocks = 32768 blocks; from the next row on, the grid-stride loop
and k at 1, 2, 7, 8 (multi_dot_ticket_kernel, one launch) and 9, 19, 64 (chunks of 8 through multi_dot_kernel and the
final pass).  At 8193 blocks and k = 64, and at 2^26 rows and k = 9, nb * k exceeds partials_capacity (262 144): the
grid is clamped and the grid-stride loop covers the rest (blas1.hip, k_multi_dot_partials).

Two fixtures: integers uniform in [-1000, 1000]; and the first moment, a = 1, b_i = i + 1 -- exact up to ~1.3e8
rows, and it needs more than 24 mantissa bits, so an fp32 intermediate anywhere fails it."""
import math

import numpy as np
import pytest

import exact_ref as er

pytestmark = pytest.mark.gpu

BLK = er.STREAM_BLOCK
ROWS = [1, 2, 3, 2047, 2048, 2049, 12345, 64 * BLK, 64 * BLK + 1, 65 * BLK + 7, 8192 * BLK, 8192 * BLK + 1,
        8193 * BLK, (1 << 26) - 3, 1 << 26, (1 << 26) + 1]
KS = [1, 2, 7, 8, 9, 19, 64]


@pytest.fixture(scope="module")
def env():
    from stormruler_amd import api

    ctx = api.Context(0)  # (no operator is ever built on it: partials_capacity keeps its default)
    yield api, ctx
    ctx.set_option("ticket_reduce", 1)
    ctx.set_option("blas1_nt", 1)
    ctx.close()


def _modes(ctx):
    """ticket_reduce 1 / 0 (one-launch ticket kernel, direct host words / partials + final pass) x blas1_nt 0 / 2
    (plain / non-temporal accesses, whatever the size)."""
    for ticket in (1, 0):
        for nt in (0, 2):
            ctx.set_option("ticket_reduce", ticket)
            ctx.set_option("blas1_nt", nt)
            yield ticket, nt
    ctx.set_option("ticket_reduce", 1)
    ctx.set_option("blas1_nt", 1)


@pytest.mark.parametrize("n", ROWS)
def test_blas1_reductions_are_exact(env, n):
    api, ctx = env
    a_h, b_h, c_h = (er.int_vector(n, s) for s in (11, 12, 13))
    vec = {k: api.DeviceVector.from_numpy(ctx, v.astype(np.float64)) for k, v in (("a", a_h), ("b", b_h), ("c", c_h))}
    exact = {k: er.exact_dot(a_h, v) for k, v in (("b", b_h), ("c", c_h), ("a", a_h))}
    one = api.DeviceVector.from_numpy(ctx, np.ones(n))
    first = api.DeviceVector.from_numpy(ctx, np.arange(1, n + 1, dtype=np.float64))
    moment = float(n * (n + 1) // 2)
    assert n * (n + 1) // 2 < er.EXACT
    order = ("b", "c", "a")
    for ticket, nt in _modes(ctx):
        tag = f"n={n} ticket={ticket} nt={nt}"
        assert api.dot_product(vec["a"], vec["b"]) == float(exact["b"]), tag
        assert api.dot_product(one, first) == moment, tag
        assert api.dot_product(first, one) == moment, tag
        assert api.norm_2(vec["a"]) == math.sqrt(float(exact["a"])), tag
        for k in KS:
            names = [order[j % 3] for j in range(k)]
            got = api.multi_dot(vec["a"], [vec[m] for m in names])
            assert np.array_equal(got, np.array([float(exact[m]) for m in names])), f"{tag} k={k}"
            got = api.multi_dot(one, [first if j % 2 == 0 else one for j in range(k)])
            assert np.array_equal(got, np.array([moment if j % 2 == 0 else float(n) for j in range(k)])), f"{tag} k={k}"
        # PendingDots: with ticket_reduce on and k <= 8 the kernel's last block leaves the sums in pinned host words
        # (the direct road of storm_hip_multi_dot_begin); k = 9 and ticket_reduce 0 take the final pass and a copy.
        # Several in flight, ended out of order.
        p2 = api.PendingDots(vec["a"], [vec["b"], vec["c"]])
        p9 = api.PendingDots(vec["a"], [vec[order[j % 3]] for j in range(9)])
        p1 = api.PendingDots(one, [first])
        assert p1.result()[0] == moment, tag
        assert np.array_equal(p9.result(), np.array([float(exact[order[j % 3]]) for j in range(9)])), tag
        assert np.array_equal(p2.result(), np.array([float(exact["b"]), float(exact["c"])])), tag


# ---- an apply with the reduction riding in it ------------------------------------------------------------------------

# (spmv_dict, spmv_record_index, ell_cap): fp64 records, byte-indexed weights and offsets, paired rows, the lattice
# format with and without its one-byte row index; fp64 records with a CSR tail (ell_cap 3: half of every row)
FORMATS = [(0, 1, 0), (2, 1, 0), (3, 1, 0), (4, 1, 0), (4, 0, 0), (0, 1, 3)]
# a small box (one single-pass fold of the per-wave partials) and one with more partials than a single pass folds
SHAPES = [(40, 30, 17), (256, 128, 130)]


@pytest.fixture(scope="module")
def spmv_env():
    from stormruler_amd import api, mesh

    ctx = api.Context(0)
    yield api, mesh, ctx
    ctx.set_option("lazy_statements", 0)
    ctx.set_option("spmv_dict", 4)
    ctx.set_option("spmv_record_index", 1)
    ctx.set_option("ell_cap", 0)
    ctx.close()


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("shape", SHAPES)
def test_apply_with_riding_dot_is_exact(spmv_env, shape, fmt):
    """z = A p; <p, z> at lazy_statements 0, 1 and 2.  At 0 the apply and the dot are two eager calls.  At 1 and 2 the
    apply waits and the dot rides in its kernel (lazy.hip lazy_try_dot: the apply's fused-dot epilogue, SpmvDot) --
    except on an operator with a CSR tail, which has no fused epilogue: the apply is launched and the ordinary dot
    follows.  (Level 2's fused CG step needs three waiting statements; one apply never reaches it.)"""
    api, mesh, ctx = spmv_env
    dict_level, idx, ell = fmt
    g = er.unit_box(mesh, *shape)
    n = g.n_cells
    ctx.set_option("spmv_dict", dict_level)
    ctx.set_option("ell_cap", ell)
    mat = api.StencilMatrix.from_face_graph(ctx, g)
    ctx.set_option("spmv_dict", 4)
    ctx.set_option("ell_cap", 0)
    ctx.set_option("spmv_record_index", idx)
    st = mat.stats()
    assert (st["tail_rows"] > 0) == (ell != 0)
    assert (st["value_dictionary_size"] > 0) == (dict_level >= 1)
    if dict_level == 4:
        assert st["paired_rows"] == 2
    p_h = er.int_vector(n, 21)
    z_h = er.int_apply(shape, p_h)
    pz, zz = er.exact_dot(p_h, z_h), er.exact_dot(z_h, z_h)
    p = api.DeviceVector.from_numpy(ctx, p_h.astype(np.float64))
    try:
        for lazy in (0, 1, 2):
            ctx.set_option("lazy_statements", lazy)
            for which in ("pz", "zp", "zz"):
                z = api.DeviceVector(ctx, n)
                before = ctx.counter("lazy_apply_dots")
                mat.apply(-1.0, 0.0, p, z)
                got = {"pz": lambda: api.dot_product(p, z), "zp": lambda: api.dot_product(z, p),
                       "zz": lambda: api.dot_product(z, z)}[which]()
                rode = ctx.counter("lazy_apply_dots") - before
                assert rode == (1 if lazy > 0 and ell == 0 else 0), (lazy, which)
                assert got == float(zz if which == "zz" else pz), (lazy, which)
                ctx.set_option("lazy_statements", 0)
                assert np.array_equal(z.to_numpy(), z_h.astype(np.float64))
                ctx.set_option("lazy_statements", lazy)
    finally:
        ctx.set_option("lazy_statements", 0)
        ctx.set_option("spmv_record_index", 1)
        mat.close()
