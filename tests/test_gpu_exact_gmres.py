"""GMRES(m)'s Gram-Schmidt kernels -- the cooperative chains of mgs_chain.hip (register, LDS ring, quad; every
template width) and the per-step kernels of solver_gmres.hip (mgs_pair_kernel, mgs_multi_kernel) -- pinned to the exact
Arnoldi reference of tests/exact_ref.py (``gmres``, ``GmresPins``) for K = 9 and 12 steps on a NON-symmetric integer
operator: convection-diffusion on the unit box, nu = 1, v = (2, 1, -1), b integer in [-3, 3].

On the symmetric Poisson box H is tridiagonal and the projections on q_0 ... q_{k-2} are rounding noise: a kernel that
skipped them would pass any test there.  Here a dropped projection, a dropped row of one dot or the earlier rotations
in the wrong order move the history by 1e5 ... 1e12 times the tolerances, which are 1e-13 ... 1e-10
(tests/test_exact_reference.py shows both halves of that on the CPU).

Every run asserts: no fallback; the chain counters (mgs_chain_steps, mgs_quad_steps, mgs_lds_steps) moved by K or by 0
as the variant demands; history[0] bitwise and history[1..K] within tol_k = max(floor_k, 16 e_k) <= 1e-10 of the exact
value (e_k: the oracle's own distance from it); ||b - A x|| of the x the solver leaves, in long double, within the same
rule of the exact history[K]; and at the two small shapes x itself against the exact x.  Each case prints
|h - exact| / (exact e_k) per entry and the rule that set each tolerance ("ratio" lines).

Shapes: each the smallest, or nearly, at which ``mgs_choose`` (mgs_chain.hip) selects a width with 256 CUs -- WIDTHS
below, checked against a restatement of its size rules.  With K = m = 9 the steps carry 1 ... 9 basis vectors: every
remainder of groups of 2, 3 and 4.  K = 12 with m = 5 crosses inner_finalize twice and exits inside a cycle."""
import numpy as np
import pytest

import exact_ref as er

pytestmark = pytest.mark.gpu

ODD = (37, 21, 19)
HOOKED = (ODD, (128, 128, 65))
# shape: (quad <S, T>, register <S>, LDS ring <S>) -- None: the family does not take the size
WIDTHS = {
    (7, 5, 3): ((1, 4), 1, 1),  # 105 rows: fewer than one sub-chunk, one block
    ODD: ((1, 4), 1, 1),  # 14 763 rows: ragged last slice, fewer blocks than CUs
    (64, 64, 65): ((2, 4), 2, 1),  # 266 240
    (64, 64, 129): ((4, 3), 4, 2),  # 528 384
    (128, 128, 65): ((8, 3), 8, 4),  # 1 064 960: the quad kernel's LDS-prefetch form with the fused apply
    (128, 128, 129): (None, 16, None),  # 2 113 536: past the quad and LDS limits; the register chain without pairs
}
CUS = 256


def chain_widths(n, cus=CUS):
    """The size rules of mgs_choose (mgs_chain.hip) restated: blocks of 1024 rows (quad) and 2048 rows (LDS ring)
    dealt to the CUs, 64-row slices to 16 wavefronts per block (register)."""
    up = lambda a, b: -(-a // b)  # noqa: E731
    qsub = up(up(n, 1024), cus)
    quad = None if qsub > 8 else ((1, 4) if qsub <= 1 else (2, 4) if qsub <= 2 else (4, 3) if qsub <= 4 else (8, 3))
    sub = up(up(n, 2048), cus)
    lds = None if sub > 4 else (1 if sub <= 1 else 2 if sub <= 2 else 4)
    slices = up(n, 64)
    need = up(slices, max(1, min(cus, up(slices, 16))) * 16)
    reg = next((s for s in (1, 2, 4, 8, 16) if need <= s), None)
    return quad, reg, lds


for _shape, _w in WIDTHS.items():
    assert chain_widths(_shape[0] * _shape[1] * _shape[2]) == _w, (_shape, chain_widths(_shape[0] * _shape[1] * _shape[2]))
assert set(WIDTHS) == set(er.GMRES_CASES)

QUAD = {"coop_mgs_quad": 2, "coop_mgs_lds": 0}
REG = {"coop_mgs_quad": 0, "coop_mgs_lds": 0}
LDS = {"coop_mgs_quad": 0, "coop_mgs_lds": 2}
# name: (options, the chain family it runs -- "default": the quad kernel where it takes the size, else the register chain)
VARIANTS = {
    "default": ({}, "default"),
    "engine": ({"generic_solvers": 1}, "default"),  # (krylov_methods.hip: the same gmres_orthogonalize)
    "quad": (QUAD, "quad"),
    "register": (REG, "register"),
    "lds": (LDS, "lds"),
    "caller-rotations": ({"coop_mgs": 2}, "default"),
    "steps2": ({"coop_mgs": 0, "mgs_steps": 2}, None),  # mgs_pair_kernel
    "steps3": ({"coop_mgs": 0, "mgs_steps": 3}, None),  # mgs_multi_kernel<3>
    "steps4": ({"coop_mgs": 0, "mgs_steps": 4}, None),  # mgs_multi_kernel<4>
}
# The quad kernel with one test hook at a time (option test_disable, context.hip): 1 the operator applied by a launch in
# front of the chain instead of inside it -- the same bits, as today; 2 no prefetch under the all-reduce; 128 row chunks
# dealt by block index; 256 the basis vectors in ascending order for every k; 512 the earlier rotations after
# everything else
# classical Gram-Schmidt applied twice (solver attribute gram_schmidt = 1: multi-dots and multi-axpys): in exact arithmetic
# the same iteration, so the same pins; and the per-step kernels and that form with every streaming launch on its
# non-temporal instance (blas1_nt 2) -- on the two small shapes, NT_SHAPES.  "step": without tickets one step per pass
# (mgs_step_kernel, each pass folding the partials of the one before)
VARIANTS["cgs2"] = ({"gram_schmidt": 1}, None)
VARIANTS["step"] = ({"coop_mgs": 0, "ticket_reduce": 0}, None)
VARIANTS.update({f"{name}-nt": (dict(VARIANTS[name][0], blas1_nt=2), None) for name in ("steps2", "steps3", "steps4", "cgs2", "step")})
NT_SHAPES = ((7, 5, 3), ODD)
HOOKS = (1, 2, 128, 256, 512)
VARIANTS.update({f"quad-test_disable{bit}": (dict(QUAD, test_disable=bit), "quad") for bit in HOOKS})
DEFAULTS = (("generic_solvers", 0), ("coop_mgs", 1), ("coop_mgs_quad", 1), ("coop_mgs_lds", 1), ("mgs_steps", 4),
            ("test_disable", 0), ("spmv_dict", 4), ("blas1_nt", 1), ("ticket_reduce", 1))
COUNTERS = ("mgs_chain_steps", "mgs_quad_steps", "mgs_lds_steps")


def _cases():
    out = []
    for shape, runs in er.GMRES_CASES.items():
        quad, _, lds = WIDTHS[shape]
        for fmt in ("default", "fp64") if shape[0] % 2 == 0 else ("default",):
            for K, m in runs:
                for name, (_, family) in VARIANTS.items():
                    if (family == "quad" and quad is None) or (family == "lds" and lds is None):
                        continue  # (a forced family that does not take the size is the register chain again)
                    if "test_disable" in name:
                        continue  # (the hooks: on HOOKED alone, below)
                    if (name.endswith("-nt") or name in ("cgs2", "step")) and shape not in NT_SHAPES:
                        continue
                    if fmt == "fp64" and family is None:
                        continue  # (the per-step kernels read w: the records' format does not reach them)
                    out.append((shape, fmt, K, m, name))
            if fmt == "default" and shape in HOOKED:
                out += [(shape, fmt, *runs[-1], f"quad-test_disable{bit}") for bit in HOOKS]
    return out


def _id(case):
    shape, fmt, K, m, name = case
    return f"{'x'.join(map(str, shape))}-{fmt}-K{K}m{m}-{name}"


@pytest.fixture(scope="module")
def env():
    from oracle import oracle
    from stormruler_amd import api, mesh

    ctx = api.Context(0)
    yield api, mesh, oracle, ctx
    _problems.clear(), _matrices.clear()
    ctx.close()


@pytest.fixture(autouse=True)
def _defaults(env):
    yield
    ctx = env[3]
    for k, v in DEFAULTS:
        ctx.set_option(k, v)


_problems, _matrices = {}, {}


def _problem(env, shape):
    """One shape at a time: the chain of the largest is 170 MB."""
    api, mesh, oracle, ctx = env
    if shape not in _problems:
        for mat in _matrices.values():
            mat.close()
        _problems.clear(), _matrices.clear()
        _problems[shape] = er.GmresProblem(oracle, mesh, shape)
    return _problems[shape]


def _matrix(env, p, fmt):
    """"default": the records the library picks (on an even line length: format 4 with paired rows, the one the quad
    kernel applies itself); "fp64": fp64 weights and int32 columns (no fused apply)."""
    api, mesh, oracle, ctx = env
    if fmt not in _matrices:
        ctx.set_option("spmv_dict", 0 if fmt == "fp64" else 4)
        g = p.g
        mat = api.StencilMatrix.from_face_weights(ctx, g.n_cells, g.n_halo, g.inner, g.outer, *p.weights)
        ctx.set_option("spmv_dict", 4)
        st = mat.stats()
        assert st["tail_rows"] == 0
        if fmt == "fp64":
            assert st["value_dictionary_size"] == 0
        elif p.shape[0] % 2 == 0:
            assert st["paired_rows"] == 2  # the fused apply is reached
        _matrices[fmt] = mat
    return _matrices[fmt]


def _expected(shape, family, K):
    """What the counters must move by."""
    quad = WIDTHS[shape][0]
    if family == "default":
        family = "quad" if quad is not None else "register"
    return {"mgs_chain_steps": 0 if family is None else K, "mgs_quad_steps": K if family == "quad" else 0,
            "mgs_lds_steps": K if family == "lds" else 0}


def _solve(env, mat, p, K, m, opts):
    api, mesh, oracle, ctx = env
    opts = dict(opts)
    gram_schmidt = opts.pop("gram_schmidt", 0)
    for k, v in opts.items():
        ctx.set_option(k, v)
    s = api.GmresSolver()
    s.gram_schmidt = gram_schmidt
    s.num_iterations, s.num_inner_iterations, s.record_history = K, m, True
    s.absolute_error_tolerance = s.relative_error_tolerance = 0.0
    b = api.DeviceVector.from_numpy(ctx, p.b.astype(np.float64))
    x = api.DeviceVector.from_numpy(ctx, np.zeros(p.b.size))
    before = {k: ctx.counter(k) for k in COUNTERS + ("nt_stream_launches",)}
    s.solve(x, b, api.HipStencilOperator(mat, 1.0, 0.0))
    moved = {k: ctx.counter(k) - before[k] for k in COUNTERS}
    nt_launches = ctx.counter("nt_stream_launches") - before["nt_stream_launches"]
    for k, v in DEFAULTS:
        ctx.set_option(k, v)
    assert s.path_fallback == 0 and s.iteration == K and s.history.size == K + 1
    # the host's choice of instance at the streaming launch sites (every shape is below the default's size switch)
    assert (nt_launches > 0) == (opts.get("blas1_nt", 1) == 2), (opts, nt_launches)
    return np.array(s.history), x.to_numpy(), moved


def _report(label, pins, ratios, xr):
    far = max(r * e for r, e in zip(ratios, pins.e))  # the largest |h - exact| / exact
    print(f"ratio {label}: " + " ".join(f"{r:.1e}" for r in ratios) + f"   far {far:.1e}   x " +
          " ".join(f"{r:.1e}" for r in xr) + "   tol " +
          " ".join("bitwise" if t is None else f"{t:.1e}/{r}" for t, r in zip(pins.tol, pins.rule)) +
          f"   tol_res {pins.tol_res:.1e}/{pins.rule_res}")


def _check(env, p, pins, label, hist, x, moved, family):
    assert moved == _expected(p.shape, family, pins.K), (label, moved)
    ratios = pins.check(list(hist), label)
    _report(label, pins, ratios, pins.check_x(x, label))


def _needs_the_cus(env, shape):
    cus = env[3].info()["num_cus"]
    if min(cus, 256) != CUS and shape not in ((7, 5, 3), ODD):
        pytest.skip(f"the kernel widths of {shape} are those of a device with {CUS} CUs or more; this one has {cus}")


@pytest.mark.parametrize("case", _cases(), ids=_id)
def test_gmres_against_the_exact_reference(env, case):
    shape, fmt, K, m, name = case
    _needs_the_cus(env, shape)
    p = _problem(env, shape)
    pins = p.pins(K, m)
    assert (pins.x is not None) == (shape in ((7, 5, 3), ODD))
    opts, family = VARIANTS[name]
    hist, x, moved = _solve(env, _matrix(env, p, fmt), p, K, m, opts)
    _check(env, p, pins, _id(case), hist, x, moved, family)
    if name == "quad-test_disable1":  # launch-then-chain: bitwise the fused form
        fused = _solve(env, _matrix(env, p, fmt), p, K, m, QUAD)
        assert np.array_equal(hist, fused[0]) and np.array_equal(x, fused[1])
