"""externalTime sides of a stream-stream join on the CPU: the literal model
(tests/join_ext_model.py) on hand-worked answers, the closed form the device
code uses against the literal queue loop, the planner's lowering, validation
and refusals, and what the generated GPU workload reaches (DESIGN.md "Joins").
"""
import bisect
import random

import pytest

import join_cases as jc
import join_ext_cases as xc
import join_ext_model as jx
from siddhi_amd import planner as pl
from siddhi_amd import query_compiler as qc

AB = xc.STREAMS
C, E = jx.CURRENT, jx.EXPIRED


def plan_of(text):
    app = qc.parse(text)
    return pl.plan_query(app, app.queries[0], pl.StringDictionary())


# ---------------------------------------------------------------- the model on known answers
def _named():
    """Events are [name, k, tau]; a row is (left name, right name)."""
    side = lambda: jx.ext(2, 10)   # noqa: E731
    return jx.Model(jx.Spec(side(), side(), lambda l, r: [l and l[0], r and r[0]], lambda l, r: l[1] == r[1],
                            "inner", "all"))


def test_hand_worked_example():
    m = _named()
    assert m.send(0, [(1000, ["a0", 1, 100])]) is None
    assert m.send(1, [(1001, ["b0", 1, 103])]) == [(C, 1001, ["a0", "b0"])]
    assert m.send(0, [(1002, ["a1", 1, 105])]) == [(C, 1002, ["a1", "b0"])]
    # 100 - 110 + 10 = 0: a0 is due; a2 (k2) meets nothing
    assert m.send(0, [(1003, ["a2", 2, 110])]) == [(E, 110, ["a0", "b0"])]
    # a step back expires nothing
    assert m.send(0, [(1004, ["a3", 1, 90])]) == [(C, 1004, ["a3", "b0"])]
    # a1, a2 (no match) and a3 expire in FIFO order, stamped 200; b0 is still there: B's window
    # moves only with B's events
    assert m.send(0, [(1005, ["a4", 1, 200])]) == [(E, 200, ["a1", "b0"]), (E, 200, ["a3", "b0"]),
                                                   (C, 1005, ["a4", "b0"])]
    assert [d[0] for _, d in m.q[0]] == ["a4"] and [d[0] for _, d in m.q[1]] == ["b0"]


def test_fifo_blocking():
    """Queue [tau 100, tau 50], T = 10: tau 65 expires nothing, though 50 - 65 + 10 <= 0."""
    assert jx.literal_windows([100, 50, 65], 10) == [([], 0), ([], 0), ([], 0)]
    m = _named()
    m.count_blocked = True
    for i, tau in enumerate((100, 50, 65)):
        m.send(0, [(i, ["a%d" % i, 1, tau])])
    assert [d[2] for _, d in m.q[0]] == [100, 50, 65] and m.stats["blocked_due_items"] == 1
    # once the head goes, the blocked item goes with it
    assert jx.literal_windows([100, 50, 65, 110], 10)[-1] == ([0, 1, 2], 3)


def test_null_time_attribute_is_dropped_and_moves_no_clock():
    m = _named()
    m.send(0, [(1, ["a0", 1, 100])])
    assert m.send(0, [(2, ["a1", 1, None])]) is None
    assert [d[0] for _, d in m.q[0]] == ["a0"]


def test_each_side_has_its_own_clock():
    m = _named()
    m.send(0, [(1, ["a0", 1, 100])])
    assert m.send(1, [(2, ["b0", 1, 10_000])]) == [(C, 2, ["a0", "b0"])]
    assert len(m.q[0]) == 1


# ---------------------------------------------------------------- closed form == literal loop
def closed_form_push(carried, new, T):
    """What engine_join.hip computes for one push of a side: `carried` is the
    side's window (time values, oldest first), `new` the push's items.  M is
    the running maximum over carried + new; the window after new item j starts
    at lo_j, the first i with M_i - M_j + T > 0 (a binary search: M never
    decreases); item j expires [lo_{j-1}, lo_j), lo_{-1} = 0.  Returns (per new
    item the positions it expires, the position the next carry starts at)."""
    taus = list(carried) + list(new)
    M, run = [], None
    for t in taus:
        run = t if run is None or t > run else run
        M.append(run)
    out, prev = [], 0
    for j in range(len(carried), len(taus)):
        lo = bisect.bisect_right(M, M[j] - T, 0, j + 1)   # first i with M_i > M_j - T
        out.append(list(range(prev, lo)))
        prev = lo
    return out, prev


def random_taus(rng, n, T):
    tau, out = rng.randrange(-50, 50), []
    for _ in range(n):
        r = rng.random()
        if r < 0.05:
            tau += T + rng.randrange(0, 3 * T)      # a jump larger than T
        elif r < 0.25:
            tau -= rng.randrange(1, 2 * T)          # a step back
        elif r < 0.5:
            pass                                    # a repeat
        else:
            tau += rng.randrange(1, max(2, T // 2))
        out.append(tau)
    return out


def test_closed_form_matches_the_literal_loop():
    """3 000 random sequences, cut into pushes at random: the closed form over
    carried + new items gives the literal loop's expirations, item for item."""
    rng = random.Random(20)
    for _ in range(3000):
        T = rng.choice((1, 2, 3, 10, 100))
        taus = random_taus(rng, rng.randrange(1, 60), T)
        want = jx.literal_windows(taus, T)
        base, pos, carried = 0, 0, []        # base: the sequence index of the carry's first item
        while pos < len(taus):
            n = rng.randrange(1, 12)
            new = taus[pos:pos + n]
            gone, lo = closed_form_push(carried, new, T)
            for j, g in enumerate(gone):
                assert [base + i for i in g] == want[pos + j][0], (taus, T, pos + j)
            carried = (carried + new)[lo:]
            base += lo
            pos += len(new)
            assert base == want[pos - 1][1]


# ---------------------------------------------------------------- planner
J = "select a.k as ak, b.k as bk insert into O;"


def test_external_time_sides_lower_to_packed_words():
    p = plan_of(AB + "from A#window.externalTime(et, 1500) as a join B#window.externalTime(b.et, 2 sec) as b "
                "on a.k == b.k " + J).plan
    assert p.kind == pl.KIND_JOIN and pl.VERSION == 1
    assert [s[3] for s in p.join_sides] == [pl.W_EXTERNAL_TIME, pl.W_EXTERNAL_TIME]
    assert [pl.join_ext_unpack(s[4]) for s in p.join_sides] == [(2, 1500), (2, 2000)]
    assert p.join_sides[0][4] == (2 << 48) | 1500
    # a side's seven words: stream, trigger, outer, window, p_lo, p_hi, n_filters -- the layout is unchanged.
    # After the two sides: on_expr, the selector (6 words + 2 per output) and the null-string id (2 words)
    w = p.to_words()
    k = len(w) - (1 + 6 + 2 * 2 + 2) - 14
    assert w[k:k + 7] == [0, 1, 0, pl.W_EXTERNAL_TIME, 1500, 2 << 16, 0]
    assert w[k + 7:k + 14] == [1, 1, 0, pl.W_EXTERNAL_TIME, 2000, 2 << 16, 0]


MIXES = [
    ("A#window.externalTime(et, 7) as a", "B#window.length(3) as b", [(pl.W_EXTERNAL_TIME, (2 << 48) | 7),
                                                                       (pl.W_LENGTH, 3)]),
    ("A#window.length(1) as a", "B#window.externalTime(et, 7) as b", [(pl.W_LENGTH, 1),
                                                                       (pl.W_EXTERNAL_TIME, (2 << 48) | 7)]),
    ("A#window.externalTime(et, 7) as a", "B as b", [(pl.W_EXTERNAL_TIME, (2 << 48) | 7), (0, 0)]),
    ("A[price > 1.0]#window.externalTime(et, 7) as a unidirectional", "B#window.externalTime(et, 9L) as b",
     [(pl.W_EXTERNAL_TIME, (2 << 48) | 7), (pl.W_EXTERNAL_TIME, (2 << 48) | 9)]),
]


@pytest.mark.parametrize("left,right,want", MIXES, ids=[m[0] + " x " + m[1] for m in MIXES])
def test_window_mixes_plan(left, right, want):
    for words in ("join", "left outer join", "full outer join"):
        p = plan_of(AB + "from %s %s %s on a.k == b.k %s" % (left, words, right, J)).plan
        assert [(s[3], s[4]) for s in p.join_sides] == want


def test_time_attribute_index_is_the_sides_own():
    p = plan_of("define stream A (et long, k int); define stream B (k int, lim float, et long); "
                "from A#window.externalTime(et, 5) as a join B#window.externalTime(et, 6) as b " + J).plan
    assert [pl.join_ext_unpack(s[4]) for s in p.join_sides] == [(0, 5), (2, 6)]


def test_a_length_joins_words_are_unchanged():
    """The words tests/test_join.py pins, for the id-less streams used here."""
    qp = plan_of(AB + "from A#window.length(2) join B on A.k == B.k select A.et as aet insert into O;")
    w = qp.plan.to_words()
    assert w[:3] == [pl.MAGIC, 1, 3]
    join = [0, 0, 1, 0, pl.W_LENGTH, 2, 0, 0, 1, 1, 0, 0, 0, 0, 0, qp.plan.join_on]
    selector = [1, 0, 0, 0, -1, 1, pl.T_LONG, qp.plan.outputs[0][2], -1, -1]
    assert w[-len(join + selector):] == join + selector


X = "from A#window.externalTime(%s) as a join B as b on a.k == b.k " + J
VALIDATION = [
    ("one parameter", "et"),
    ("three parameters", "et, 10, 20"),
    ("timestamp is a constant", "5, 10"),
    ("timestamp is the other side's attribute", "b.et, 10"),
    ("timestamp is no attribute of the side", "lim, 10"),
    ("timestamp is an int attribute", "k, 10"),
    ("timestamp is a float attribute", "price, 10"),
    ("window time is an attribute", "et, et"),
    ("window time is a float", "et, 1.5"),
    ("window time is a string", "et, '10'"),
]


@pytest.mark.parametrize("name,params", VALIDATION, ids=[v[0] for v in VALIDATION])
def test_reference_validation_errors_stay_validation_errors(name, params):
    with pytest.raises(pl.SiddhiAppValidationException) as ei:
        plan_of(AB + X % params)
    assert not isinstance(ei.value, pl.UnsupportedPlanException)


REFUSALS = [
    ("T = 0", X % "et, 0", "window time of 0 or less on a join side"),
    ("T < 0", X % "et, -5", "window time of 0 or less on a join side"),
    ("T = 2^48", X % ("et, %dL" % (1 << 48)), r"window time of 2\^48 or more on a join side"),
    ("time side", "from A#window.time(1 sec) as a join B#window.externalTime(et, 5) as b " + J,
     "time windows on a join side"),
    ("timeLength side", "from A#window.timeLength(1 sec, 5) as a join B as b " + J,
     "window timelength on a join side"),
    ("timeBatch side", "from A as a join B#window.timeBatch(1 sec) as b " + J, "window timebatch on a join side"),
    ("lengthBatch side", "from A#window.lengthBatch(2) as a join B as b " + J, "window lengthbatch on a join side"),
    ("externalTimeBatch side", "from A#window.externalTimeBatch(et, 1 sec) as a join B as b " + J,
     "window externaltimebatch on a join side"),
]


@pytest.mark.parametrize("name,text,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refused_with_unsupported_plan(name, text, message):
    with pytest.raises(pl.UnsupportedPlanException, match=message):
        plan_of(AB + text)


def test_largest_window_time_is_accepted():
    p = plan_of(AB + X % ("et, %dL" % ((1 << 48) - 1))).plan
    assert pl.join_ext_unpack(p.join_sides[0][4]) == (2, (1 << 48) - 1)


def test_the_time_known_answers_are_still_not_run():
    assert len(jc.REFUSED_CASES) == 4
    for case in jc.REFUSED_CASES:
        with pytest.raises(pl.UnsupportedPlanException, match="time windows on a join side"):
            plan_of(case["app"])


# ---------------------------------------------------------------- what the generated workload reaches
def test_generated_workload_reaches_the_kernels_tile_numbers():
    """On the model alone: the workload tests/test_gpu_join_external_time.py
    runs goes past the 64-item tile, the 256-slot workgroup and the item
    store's first 1024 slots, and has a blocked step back."""
    s = xc.Shape("ext x ext", kind="full_outer")
    _, st = xc.model_run(s.spec, s.sends(), count_blocked=True)
    assert st["max_expired_by_one_event"] > jc.JOIN_TRIG
    assert st["max_window_met"] > jc.JOIN_TILE
    assert st["max_carried"] > 1024
    assert st["blocked_due_items"] >= 1


@pytest.mark.parametrize("events", ["current", "expired", "all"])
def test_every_output_mode_has_rows_of_expired_triggers(events):
    """EXPIRED triggers reach the output of `expired events` and `all events`;
    `insert into` drops their rows, but the model's run still produced them
    (the window is trimmed all the same)."""
    s = xc.Shape("mode", events=events)
    rows, st = xc.model_run(s.spec, s.sends())
    expired = sum(len(e) for _, e in rows)
    if events == "current":
        assert expired == 0 and sum(len(c) for c, _ in rows) > 0
        both, _ = xc.model_run(xc.Shape("mode", events="all").spec, s.sends())
        assert [c for c, _ in rows if c] == [c for c, _ in both if c]   # trimmed as in `all events`
    else:
        assert expired > 0 and st["expired_rows"] == expired
