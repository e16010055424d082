"""The catalogue of tests/history_cases.py and its orders, checked without a device: what
tests/test_gpu_history_independence.py runs covers what it says it covers."""
import history_cases as hc


def test_ids_are_unique_and_every_case_is_complete():
    ids = [c.id for c in hc.CASES]
    assert len(ids) == len(set(ids)) == 22
    for c in hc.CASES:
        assert c.counters and all(k and (v == "positive" or isinstance(v, int)) for k, v in c.counters.items()), c.id
        assert any(v == "positive" or v > 0 for v in c.counters.values()), c.id  # something must MOVE
        assert callable(c.anchor) and c.anchor.__doc__ and "tests/test_" in c.anchor.__doc__, c.id  # the pointer to its feature test
        assert callable(c._build) and callable(c._solve)
        if c.companion is not None and not callable(c.companion):
            assert set(c.companion) <= set(hc.DEFAULTS), c.id
        assert set(c.options) <= set(hc.DEFAULTS), c.id  # every option a case sets has a default to go back to


def test_a_record_differs_in_every_field_it_holds():
    import numpy as np

    class S:
        iteration, num_applies, num_pre_applies, path_fallback, absolute_error, initial_error = 3, 4, 0, 0, 0.5, 2.0
        history = np.array([2.0, 1.0, 0.75, 0.5])

    ref = {"parts": [hc._part(True, S, np.arange(5.0), (1, 2))], "counters": {"engine_solves": 1}}
    assert hc.differences(ref, ref) == []
    for field in hc.FIELDS:
        other = {"parts": [dict(ref["parts"][0])], "counters": dict(ref["counters"])}
        v = other["parts"][0][field].copy()
        other["parts"][0][field] = (~v if v.dtype == bool else v + 1)  # one unit in the last place, or one count
        assert len(hc.differences(other, ref)) == 1 and field in hc.differences(other, ref)[0], field
    assert hc.differences({"parts": ref["parts"], "counters": {"engine_solves": 2}}, ref)
    # -0.0 and 0.0, and two NaNs of different payload, are different bits
    assert not np.array_equal(hc.bits(-0.0), hc.bits(0.0))


def test_options_go_back_to_the_defaults_even_when_the_body_raises():
    class Ctx:
        def __init__(self):
            self.log = []

        def set_option(self, k, v):
            self.log.append((k, v))

    ctx = Ctx()
    try:
        with hc.Options(ctx, hc.TAIL):
            raise RuntimeError
    except RuntimeError:
        pass
    n = len(hc.TAIL)
    assert ctx.log[:n] == list(hc.TAIL.items())
    assert ctx.log[n:] == [(k, hc.DEFAULTS[k]) for k in reversed(list(hc.TAIL))]


def test_the_generator_is_deterministic_and_covers_everything():
    seen_cases, seen_dist = {}, {}
    for seed in hc.SEEDS:
        a, b = hc.schedule(seed), hc.schedule(seed)
        assert a == b and len(a) == hc.SCHEDULE_LENGTH
        for e in a:
            if e[0] == "check":
                seen_cases[e[1]] = seen_cases.get(e[1], 0) + 1
            else:
                assert e[0] == "dist" and (e[2] is not None) == hc.DISTURBANCES[e[1]][0]
                assert e[2] is None or e[2] in hc.LIGHT
                seen_dist[e[1]] = seen_dist.get(e[1], 0) + 1
    assert hc.schedule(0) != hc.schedule(1) != hc.schedule(2)
    assert set(seen_cases) == set(hc.BY_ID) and min(seen_cases.values()) >= 2
    assert set(seen_dist) == set(hc.DISTURBANCES) and min(seen_dist.values()) >= 1


def test_every_ordered_pair_of_paths_is_run_but_the_stated_exclusions():
    pairs = set()
    for c in hc.CASES:
        entries = hc.after_every_other_path(c.id)
        assert [e[0] for e in entries] == ["use", "check"] * (len(entries) // 2)
        assert all(e[1] == c.id for e in entries[1::2])
        pairs |= {(e[1], c.id) for e in entries[0::2]}
    ids = [c.id for c in hc.CASES]
    want = {(a, b) for a in ids for b in ids if a != b}
    excluded = {("thr_cg_step", b) for b in ids if b != "thr_cg_step" and b not in hc.STEP_BEFORE}
    assert want - pairs == excluded and pairs <= want
    assert set(hc.STEP_BEFORE) == {"thr_cg", "res_cg", "eng_gmres_2l"}


def test_every_case_meets_every_disturbance_on_its_own_path_and_on_two_others():
    for c in hc.CASES:
        ds = hc.disturbances_of(c.id)
        for name, (takes, _) in hc.DISTURBANCES.items():
            on = [t for n, t in ds if n == name]
            if takes:
                assert on[0] == c.id and len(on) == 3 and len({hc.BY_ID[t].path for t in on}) == 3, (c.id, name)
                assert all(t in hc.LIGHT for t in on[1:])
            else:
                assert on == [None], (c.id, name)
        entries = hc.after_every_disturbance(c.id)
        assert all(entries[i + 1] == ("check", c.id) for i in range(0, 2 * len(ds), 2))

    def follows(b_id, first, then):
        e = hc.after_every_disturbance(b_id)
        return any(e[i] == first and e[i + 1: i + 1 + len(then)] == then for i in range(len(e)))

    assert follows("eng_gmres_2l", ("dist", "abort_callback", None), [("check", "eng_gmres_2l")])
    assert follows("thr_cg", ("dist", "verify_trip", None), [("check", "thr_cg")])
    assert follows("thr_bicg", ("dist", "verify_trip", None), [("check", "thr_bicg")])
    assert follows("thr_gmres", ("dist", "coop_gave_up", "res_cg"), [("check", "res_bicg"), ("check", "lat_cg"), ("check", "thr_gmres")])


def test_two_contexts_take_four_cases_each():
    a, b = hc.TWO_CONTEXTS
    assert len(a) == len(b) == 4 and len(set(a) | set(b)) == 8 and set(a) | set(b) <= set(hc.BY_ID)
