"""A solve's result bits are those the same solve gives in a context that has done nothing else, whatever ran before it.

A context carries state from solve to solve and shares it between the solver paths ("What a context carries between
solves"): the self-re-arming tickets, the all-reduce slots and their tag counter, the resident kernels' sequence numbers, the
done ring's generations, the resources of destroyed engines, the engine's pending reduction, the workspaces that grow, the
vector pool and arenas, the lazy queue's spare vector, the cooperative-launch flags, SolverState::verify_failed.  The feature
tests check each path against itself in a context that does nothing else; here every path of tests/history_cases.py runs
behind every other path, behind every disturbance, in seeded orders and in two contexts that take turns, and every record
must equal the record of a fresh context FIELD BY FIELD: np.array_equal on the uint64 views of x, the history and the errors,
== on the counts and on the deltas of the path counters.  The only toleranced checks are the anchors of the fresh records,
each the check of the case's own feature test.

Left out, because they depend on their history BY DESIGN:
  * SolutionRecycler objects (the guess is a function of the solves before it);
  * fill_randomly without rng_reset (the reference's function-static generator runs on; eng_idrs resets it);
  * the back-off after a REAL give-up of a cooperative kernel (coop_skip; the hook coop_force_fail sets none);
  * a multigrid object after a failed refresh;
  * options the caller leaves set (every case and disturbance here restores its own)."""
import pytest

import history_cases as hc

pytestmark = pytest.mark.gpu

IDS = [c.id for c in hc.CASES]


@pytest.fixture(scope="module")
def fresh():
    """case id -> the record of that case in a context of its own that has done nothing else; made on first use, kept.  On
    it: no fallback, the path counters moved as the catalogue says, and the anchor holds."""
    from stormruler_amd import api

    records = {}

    def get(case_id):
        if case_id not in records:
            case = hc.BY_ID[case_id]
            ctx = api.Context(0)
            try:
                built = case.build(ctx)
                record = case.run(ctx, built)
                for part in record["parts"]:
                    assert int(part["path_fallback"]) == 0, case_id
                case.counters_moved(record)
                companion = None
                if callable(case.companion):
                    companion = case.companion(api, ctx, built)
                elif case.companion is not None:
                    companion = case.run(ctx, built, options=case.companion)
                case.anchor(record, built, companion)
                case.close(built)
            finally:
                ctx.close()
            records[case_id] = record
        return records[case_id]

    yield get
    records.clear()


def run_entries(ses, entries, fresh):
    """The entries in order on one session; every ("check", case) must give the fresh record.  Returns how many were compared."""
    done, compared = [], 0
    for entry in entries:
        where = f"behind {done[-1] if done else 'nothing'}"
        try:
            if entry[0] == "dist":
                hc.disturb(ses, entry[1], entry[2])
                record = None
            else:
                record = ses.run(entry[1])
        except Exception as e:  # (an error status is a difference too: say behind what)
            raise AssertionError(f"{':'.join(map(str, entry))} {where} raised {e!r}; so far {done}") from e
        if entry[0] == "check":
            diff = hc.differences(record, fresh(entry[1]))
            assert not diff, f"{entry[1]} {where}: {diff}; so far {done}"
            compared += 1
        done.append(":".join(str(e) for e in entry[1:] if e is not None))
    return compared


def _session_for(b_id, fresh, entries):
    for entry in entries:  # (the fresh contexts are closed before this one opens: no two cooperative kernels in flight)
        if entry[0] == "check":
            fresh(entry[1])
    ses = hc.Session()
    ses.objects(b_id)  # B's operator is built once, at the start
    return ses


@pytest.mark.parametrize("b_id", IDS)
def test_after_every_other_path(fresh, b_id):
    """A1, B, A2, B, ... over every other case A in one context (the history accumulates): every run of B is the fresh B."""
    entries = hc.after_every_other_path(b_id)
    ses = _session_for(b_id, fresh, entries)
    try:
        assert run_entries(ses, entries, fresh) == len(hc.others_of(b_id))
    finally:
        ses.close()


@pytest.mark.parametrize("b_id", IDS)
def test_after_every_disturbance(fresh, b_id):
    """D1, B, D2, B, ...: every disturbance, those that take a case on B's own path and on two others.  Among the orders:
    abort_callback -> eng_gmres_2l (a failed solve, then the two-launch road), verify_trip -> thr_cg / thr_bicg (the sticky
    flag), coop_gave_up(res_cg) -> res_bicg -> lat_cg -> thr_gmres (the give-up flag shares the slots' buffer)."""
    entries = hc.after_every_disturbance(b_id)
    ses = _session_for(b_id, fresh, entries)
    try:
        assert run_entries(ses, entries, fresh) >= len(hc.disturbances_of(b_id))
    finally:
        ses.close()


@pytest.mark.parametrize("seed", hc.SEEDS)
def test_seeded_schedules(fresh, seed):
    entries = hc.schedule(seed)
    for entry in entries:
        if entry[0] == "check":
            fresh(entry[1])
    ses = hc.Session()
    try:
        assert run_entries(ses, entries, fresh) >= len(hc.CASES)
    finally:
        ses.close()


def test_two_contexts_alternate(fresh):
    """Two live contexts on the device take turns, four cases each, twice round.  Every solve completes and its context is
    synchronised before the other's next call, so no two cooperative kernels are ever in flight together."""
    for ids in hc.TWO_CONTEXTS:
        for case_id in ids:
            fresh(case_id)
    sessions = [hc.Session(), hc.Session()]
    try:
        for turn in range(2 * len(hc.TWO_CONTEXTS[0])):
            for ses, ids in zip(sessions, hc.TWO_CONTEXTS):
                case_id = ids[turn % len(ids)]
                record = ses.run(case_id)
                ses.ctx.sync()
                diff = hc.differences(record, fresh(case_id))
                assert not diff, f"{case_id} in turn {turn}: {diff}"
    finally:
        for ses in sessions:
            ses.close()
