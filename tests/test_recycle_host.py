"""storm_hip_recycle without a GPU: the ABI surface, the null refusals, and the restatement of the recipe
(tests/recycle_ref.py) held to its own invariants, to the exactness conditions of the designed data, and to the bounds the
GPU test asserts on the box sequence."""
import ctypes as C
import os
import random
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import recycle_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "storm_hip.h")
LIB = os.path.join(ROOT, "stormruler_amd", "libstorm_hip.so")

ENTRY_POINTS = ("storm_hip_recycle_create", "storm_hip_recycle_destroy", "storm_hip_recycle_guess", "storm_hip_recycle_update",
                "storm_hip_recycle_reset", "storm_hip_recycle_get", "storm_hip_recycle_get_slot", "storm_hip_recycle_set_slot")


def test_header_declares_and_library_exports_the_entry_points():
    from stormruler_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    exported = subprocess.check_output(["nm", "-D", "--defined-only", LIB], text=True)
    for name in ENTRY_POINTS:
        assert re.search(rf"\bint {name}\s*\(", text), name
        assert re.search(rf" T {name}\b", exported), name
        assert name in _lib.SIGNATURES
    assert "STORM_HIP_RECYCLE_ENERGY = 0" in text and "STORM_HIP_RECYCLE_RESIDUAL = 1" in text
    assert re.search(r"#define\s+STORM_HIP_ABI_VERSION\s+6\b", text)
    assert _lib.lib.storm_hip_abi_version() == 6


def test_the_header_restates_the_recipe_of_the_reference_module():
    """The recipe, as the reference module states it, stands in the header word for word (whitespace and comment stars aside)."""
    def squeeze(s):
        return re.sub(r"[\s*]+", " ", s)

    header = squeeze(open(HEADER).read())
    doc = R.__doc__.split("THE RECIPE.")[1].split("Two number spaces")[0]
    assert len(doc.split()) > 250
    assert squeeze(doc).strip() in header


def test_every_entry_point_refuses_null_arguments_without_a_context():
    from stormruler_amd._lib import lib

    h, v = C.c_void_p(), C.c_double()
    calls = [lambda: lib.storm_hip_recycle_create(None, 8, 0, 4, 0, C.byref(h)),
             lambda: lib.storm_hip_recycle_guess(None, None, None),
             lambda: lib.storm_hip_recycle_update(None, None, None),
             lambda: lib.storm_hip_recycle_reset(None),
             lambda: lib.storm_hip_recycle_get(None, b"count", C.byref(v)),
             lambda: lib.storm_hip_recycle_get_slot(None, 0, None, None, None),
             lambda: lib.storm_hip_recycle_set_slot(None, 0, None, None, 1.0)]
    for call in calls:
        assert call() == -1  # STORM_HIP_E_INVALID
        assert b"null" in lib.storm_hip_last_error()
    assert lib.storm_hip_recycle_destroy(None) == 0  # (as every destroy of the library)


def test_fma_is_the_fraction_statement():
    rng = random.Random(5)
    for _ in range(2000):
        a, b, c = (rng.uniform(-1, 1) * 2.0 ** rng.randint(-30, 30) for _ in range(3))
        if rng.random() < 0.3:
            c = -a * b  # cancellation: the low half of the product is all that is left
        assert R.fma(a, b, c) == float(Fraction(a) * Fraction(b) + Fraction(c))
    assert R.fma(3.0, 0.0, -0.0) == 0.0 and str(R.fma(3.0, 0.0, -0.0)) == "0.0"
    assert str(R.fma(-3.0, 0.0, -0.0)) == "-0.0"


def _random_problem(n, seed):
    rng = np.random.default_rng(seed)
    m = rng.integers(-3, 4, size=(n, n))
    a = m @ m.T + n * np.eye(n, dtype=np.int64)  # SPD, integer
    return a, rng


@pytest.mark.parametrize("kind", [0, 1])
def test_the_exact_restatement_keeps_its_invariants(kind):
    """In Fractions, after EACH update: <t_i, v_j> = 0 for i != j and g_j N(u_j, v_j) = 1 -- through guesses, an update
    without a guess, and a restart."""
    n, m = 9, 4
    a, rng = _random_problem(n, 11 + kind)
    r = R.Recycler(R.Exact, n, m, kind)
    seen_restart = False
    for step in range(m + 3):
        b = rng.integers(-9, 10, size=n)
        if step != 2:  # (step 2: an update with no guess since the last one)
            r.guess(b)
        x = rng.integers(-9, 10, size=n)
        r.update(x, a @ x)
        seen_restart |= r.restarts > 0
        assert r.count == (step % m) + 1
        for i in range(r.count):
            for j in range(r.count):
                if i != j:
                    assert R.Exact.dot(r.t(i), r.v[j]) == 0, (step, i, j)
            assert r.g[i] * r.norm(r.u[i], r.v[i]) == 1, (step, i)
            assert all(vi == sum(int(a[k, l]) * ul for l, ul in enumerate(r.u[i].tolist())) for k, vi in enumerate(r.v[i].tolist()))
        for j in range(r.count, m):
            assert r.g[j] == 0
    assert seen_restart and r.restarts == 1 and r.updates == m + 3


@pytest.mark.parametrize("kind", [0, 1])
def test_the_exact_guess_is_the_best_in_the_span(kind):
    """The projection's defining property: the error (kind 0) / the residual (kind 1) of the guess is orthogonal to the span."""
    n, m = 9, 4
    a, rng = _random_problem(n, 3 + kind)
    r = R.Recycler(R.Exact, n, m, kind)
    for _ in range(3):
        x = rng.integers(-9, 10, size=n)
        r.update(x, a @ x)
    b = R.Exact.vec(rng.integers(-9, 10, size=n))
    x = r.guess(b)
    res = b - np.array([sum(int(a[k, l]) * xl for l, xl in enumerate(x.tolist())) for k in range(n)], dtype=object)
    for j in range(r.count):
        assert R.Exact.dot(r.t(j), res) == 0


def test_the_guard_drops_a_dependent_vector_and_a_non_finite_one():
    n = 6
    a, rng = _random_problem(n, 7)
    r = R.Recycler(R.F64, n, 4, 0)
    x0 = rng.integers(-9, 10, size=n).astype(np.float64)
    r.update(x0, a @ x0)
    r.guess(a @ (3.0 * x0))
    r.update(3.0 * x0, a @ (3.0 * x0))  # inside the span
    assert r.g[1] == 0.0 and r.count == 2
    bad = (a @ x0).astype(np.float64)
    bad[2] = np.inf
    r.update(x0 + 1.0, bad)
    assert r.g[2] == 0.0 and r.count == 3
    r.reset()
    assert r.count == 0 and not np.any(r.guess(np.ones(n)))


DESIGNED_CAPS = ((1, 0), (3, 2), (8, 7), (9, 8), (16, 15))


@pytest.mark.parametrize("n, caps", [(2, DESIGNED_CAPS), (127, DESIGNED_CAPS), (4097, ((1, 0), (16, 15)))])
@pytest.mark.parametrize("kind", [0, 1])
def test_the_designed_data_meets_its_exactness_conditions(n, caps, kind):
    """(4 097 rows: the smallest and the largest object -- the sums of absolute values grow with the pairs.)"""
    for capacity, loaded in caps:
        assert R.designed_is_exact(n, loaded, kind), (n, capacity, loaded, kind)
        if n <= 127:
            # ... so the fp64 restatement IS the exact one up to 1 / nu of the new pair, which rounds once
            ex = R.Recycler(R.Exact, n, capacity, kind)
            for j, (u, v, g) in enumerate(R.designed_slots(n, loaded, kind)):
                ex.set_slot(j, u, v, g)
            _, d = R.designed_run(n, capacity, loaded, kind)
            assert [Fraction(v) for v in d["x0"].tolist()] == ex.guess(d["b"]).tolist()
            assert [Fraction(v) for v in d["c0"]] == list(ex.c or [])
            ex.update(d["x"], d["ax"])
            s = d["s"]
            assert [Fraction(v) for v in d["u_s"].tolist()] == ex.u[s].tolist()
            assert [Fraction(v) for v in d["v_s"].tolist()] == ex.v[s].tolist()
            assert d["g_s"] == float(ex.g[s]) and d["g_s"] > 0.0


def test_the_designed_patterns_are_orthogonal_with_power_of_two_norms():
    for n in (2, 127, 4097):
        for kind in (0, 1):
            slots = R.designed_slots(n, 15, kind)
            for i, (ui, vi, gi) in enumerate(slots):
                assert ui[0] == 0 and np.array_equal(vi, 2 * ui)
                for j, (uj, vj, _) in enumerate(slots):
                    t = vi if kind else ui
                    dot = int(t @ vj)
                    if i != j:
                        assert dot == 0
                    elif gi:
                        assert dot & (dot - 1) == 0 and gi * dot == 1 and ui[-1] != 0
                    else:
                        assert dot == 0


@pytest.fixture(scope="module")
def box_warm():
    return R.box_sequence(0, 0)


@pytest.mark.parametrize("kind", [0, 1])
def test_the_restatement_alone_stays_inside_the_bounds_of_the_box_sequence(box_warm, kind):
    rec = R.box_sequence(8, kind)
    warm_total, rec_total = sum(w[0] for w in box_warm), sum(w[0] for w in rec)
    print(f"kind {kind}: warm {[w[0] for w in box_warm]} = {warm_total}, recycled {[w[0] for w in rec]} = {rec_total}")
    assert rec_total <= R.BOX_RATIO * warm_total
    for t in R.BOX_CAPPED:
        assert rec[t][0] <= R.BOX_CAP, (t, rec[t])
    assert all(w[2] for w in rec) and all(w[2] for w in box_warm)
    assert max(w[3] for w in rec) <= 2.0 * max(w[3] for w in box_warm)
    # the solve behind the restart starts from one pair: it is the free one, and the pairs rebuild from there
    assert rec[R.BOX_FREE][0] > R.BOX_CAP and rec[R.BOX_FREE + 2][0] <= R.BOX_CAP
