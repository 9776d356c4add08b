"""min / max / minForever / maxForever: the Python model (tests/minmax_model.py)
that is their yardstick, the reference's own known answers, and the planner.

The CPU oracle does not know these aggregators, so the model is pinned to it in
two halves: its windows, partition, group-by and selector batching run the
generated workloads with sum / avg / count in place of min / max and must give
the oracle's callbacks exactly; its four executors are restated line by line
from C/query/selector/attribute/aggregator/{Max,Min,MaxForever,MinForever}
AttributeAggregatorExecutor.java and checked by hand here, quirks included.
"""
import numpy as np
import pytest

import minmax_cases as mc
import minmax_model as mm
from kat_runner import check_case
from oracle_engine import OracleQueryEngine
from siddhi_amd import planner as pl
from siddhi_amd import query_compiler as qc


def plan_of(text, query_index=0):
    app = qc.parse(text)
    item = app.execution_order[query_index]
    d = pl.StringDictionary()
    if isinstance(item, qc.Partition):
        return pl.plan_query(app, item.queries[0], d, item)
    return pl.plan_query(app, item, d, None)


# ---------------------------------------------------------------- the model's window and selector == the oracle
@pytest.mark.parametrize("case", mc.SHAPES, ids=[c.name for c in mc.SHAPES])
def test_model_window_and_selector_equal_the_oracle(case):
    """Rows, values, timestamps and callback boundaries of every generated
    shape, with aggregators the oracle knows."""
    c = case.with_aggs(mc.TO_ORACLE)
    d = mc.make_stream(**c.stream)
    want = mc.model_chunks(c.spec, d, c.pushes)
    got = mc.runtime_chunks(c.app, d, OracleQueryEngine, c.pushes)
    mc.assert_same(got, want)
    # (an ungrouped `all events` chunk ends in a CURRENT row, and only its last row shows)
    if c.spec.events == "expired" or (c.spec.events == "all" and c.spec.group is not None):
        assert any(rem for cur, rem in want), "the shape emits no EXPIRED row"


# ---------------------------------------------------------------- the executors, by hand
def fold(state, ops):
    return [state.add(v) if op == "+" else state.remove(v) for op, v in ops]


def test_max_is_the_reference_deque_not_a_sliding_maximum():
    """length(3) over 3, 5, 3, 1, 0: the first 3's expiry takes the third
    event's 3 out of the deque [5, 3]; when 5 expires the window still holds a
    3, and max says 1."""
    s = mm.MaxState(mm.T_INT, True)
    got = fold(s, [("+", 3), ("+", 5), ("+", 3), ("-", 3), ("+", 1), ("-", 5), ("+", 0)])
    assert got == [3, 5, 5, 5, 5, 1, 1]


def test_max_is_null_while_the_window_holds_events():
    """length(3) over 1, 2, 1, 0, 1, 0: the first 1's expiry takes the third
    event's 1 from [2, 1]; 2 expires, the fifth event's 1 pops the 0: [1]; then
    the third event's 1 expires and takes that one: null, with 0 and 1 in the window."""
    s = mm.MaxState(mm.T_INT, True)
    got = fold(s, [("+", 1), ("+", 2), ("+", 1), ("-", 1), ("+", 0), ("-", 2), ("+", 1), ("-", 1), ("+", 0)])
    assert got == [1, 2, 2, 2, 2, 0, 1, None, 0]
    # the same through the window model: the row of the expiry before the sixth event's add
    m = mm.Model(mm.Spec(("length", 3), [("max", 0, mm.T_INT)], [("agg", 0)], "expired"))
    out = m.run([[(t, [v])] for t, v in enumerate([1, 2, 1, 0, 1, 0])])
    assert [vals for c in out for t, ts, vals in c] == [[2], [0], [None]]


def test_min_mirrors_max():
    s = mm.MaxState(mm.T_LONG, True, is_max=False)
    assert fold(s, [("+", 3), ("+", 1), ("+", 3), ("-", 3), ("+", 5), ("-", 1), ("+", 9)]) == [3, 1, 1, 1, 1, 5, 5]


def test_nan_and_signed_zero():
    nan = float("nan")
    s = mm.MaxState(mm.T_DOUBLE, True)
    # NaN compares false both ways: it is never popped and pops nothing
    out = fold(s, [("+", 1.0), ("+", nan), ("+", 0.5)])
    assert out[0] == 1.0 and out[1] == 1.0 and out[2] == 1.0 and len(s.deque) == 3
    # removal is equals(): NaN equals NaN
    s.remove(1.0)
    assert s.value != s.value and len(s.deque) == 2
    s.remove(float("nan"))
    assert s.deque == [0.5] and s.value == 0.5
    # 0.0 does not equal -0.0: the remove finds nothing, the pops compare numerically
    s = mm.MaxState(mm.T_DOUBLE, True)
    fold(s, [("+", 0.0), ("+", -0.0)])
    assert len(s.deque) == 2                      # -0.0 < 0.0 is false: not popped
    s.remove(-0.0)
    assert [x.hex() for x in s.deque] == [(0.0).hex()]
    s.remove(-0.0)
    assert len(s.deque) == 1 and s.value.hex() == (0.0).hex()
    # float: compared as float, equal by floatToIntBits
    s = mm.MaxState(mm.T_FLOAT, True)
    fold(s, [("+", np.float32(0.1)), ("+", np.float32(0.1))])
    s.remove(np.float32(0.1))
    assert len(s.deque) == 1


def test_without_tracking_remove_nulls_an_equal_value():
    s = mm.MaxState(mm.T_INT, False)
    assert s.deque is None
    assert fold(s, [("+", 4), ("+", 2), ("-", 2), ("-", 4), ("+", 1)]) == [4, 4, 4, None, 1]


def test_reset_both_families():
    s = mm.MaxState(mm.T_INT, True)
    fold(s, [("+", 4), ("+", 2)])
    s.reset()
    assert s.value is None and s.deque == []
    assert s.add(1) == 1                          # an empty state behaves as a fresh one
    f = mm.MaxForeverState(mm.T_INT, True)
    assert fold(f, [("+", 4), ("-", 9), ("+", 2)]) == [4, 9, 9]   # a remove folds its value in too
    assert f.reset() == 9 and f.value == 9        # reset() returns the value and keeps it
    g = mm.MaxForeverState(mm.T_INT, True, is_max=False)
    assert fold(g, [("+", 4), ("-", 1), ("+", 2)]) == [4, 1, 1]


def test_null_arguments_leave_the_state_alone():
    for kind in ("max", "min", "maxForever", "minForever"):
        st = mm.new_state(kind, mm.T_DOUBLE, True)
        assert mm.step(kind, st, mm.CURRENT, None) is None
        assert mm.step(kind, st, mm.CURRENT, 2.0) == 2.0
        assert mm.step(kind, st, mm.EXPIRED, None) == 2.0
        assert mm.step(kind, st, mm.CURRENT, None) == 2.0


def test_lengthbatch_reset_clears_max_and_keeps_forever():
    spec = mm.Spec(("lengthBatch", 2), [("max", 0, mm.T_INT), ("maxForever", 0, mm.T_INT)], [("agg", 0), ("agg", 1)])
    m = mm.Model(spec)
    out = m.run([[(1, [9]), (2, [3])], [(3, [1]), (4, [2])]])
    assert [[vals for t, ts, vals in c] for c in out] == [[[9, 9]], [[2, 9]]]


# ---------------------------------------------------------------- the generated workload shows the quirk
def test_duplicate_valued_workload_differs_from_the_true_extremum():
    """A kernel computing the true window maximum must fail the generated
    tests: on the shipped length(5) workload over values 0..7 the reference's
    answer after an expiry differs from the true maximum of the four events
    left, and is null while they are there."""
    case = next(c for c in mc.SHAPES if c.name == "length5-expired-quirk")
    d = mc.make_stream(**case.stream)
    rows = [r for cur, rem in mc.model_chunks(case.spec, d, case.pushes) for r in rem]
    x = d["x"]
    differ = nulls = 0
    for ts, (i, mx, mn) in rows:
        left = x[i + 1:i + 5]
        assert len(left) == 4
        differ += (mx != int(left.max())) + (mn != int(left.min()))
        nulls += (mx is None) + (mn is None)
    assert differ >= 50 and nulls >= 3, (differ, nulls)


# ---------------------------------------------------------------- the reference's own tests
def test_every_known_answer_has_a_spec():
    assert sorted(mc.KAT_SPECS) == sorted(c["name"] for c in mc.RUN_KATS)
    assert len(mc.RUN_KATS) == 13 and len(mc.FAIL_KATS) == 4


@pytest.mark.parametrize("case", mc.RUN_KATS, ids=[mc.short(c) for c in mc.RUN_KATS])
def test_model_reproduces_reference_known_answer(case):
    assert check_case(case, mc.model_collector(case)) == []


@pytest.mark.parametrize("case", mc.RUN_KATS, ids=[mc.short(c) for c in mc.RUN_KATS])
def test_known_answer_plans(case):
    qp = plan_of(case["app"])
    assert [a[0] for a in qp.plan.aggs][0] in (pl.AGG_MAX, pl.AGG_MIN, pl.AGG_MAX_FOREVER, pl.AGG_MIN_FOREVER)


@pytest.mark.parametrize("case", mc.FAIL_KATS, ids=[mc.short(c) for c in mc.FAIL_KATS])
def test_reference_creation_failures(case):
    """max(weight, deviceId), maxForever(price1, price2, price3): the app's creation fails."""
    assert case["expected_exception"] == "SiddhiAppCreationException"
    with pytest.raises(pl.SiddhiAppCreationException) as ei:
        plan_of(case["app"])
    assert not isinstance(ei.value, pl.UnsupportedPlanException)


# ---------------------------------------------------------------- the planner
KINDS = [("max", pl.AGG_MAX), ("min", pl.AGG_MIN), ("maxForever", pl.AGG_MAX_FOREVER),
         ("minForever", pl.AGG_MIN_FOREVER)]


def test_kinds_follow_count_in_the_ir():
    assert (pl.AGG_SUM, pl.AGG_AVG, pl.AGG_COUNT) == (1, 2, 3)
    assert [k for _, k in KINDS] == [4, 5, 6, 7]
    with open(mc.ROOT + "/include/siddhi_ir.h") as fp:
        text = fp.read()
    for name, k in (("SHD_AGG_MAX", 4), ("SHD_AGG_MIN", 5), ("SHD_AGG_MAX_FOREVER", 6), ("SHD_AGG_MIN_FOREVER", 7)):
        assert "%s = %d" % (name, k) in text
    assert "#define SHD_IR_VERSION 1" in text


@pytest.mark.parametrize("fn,kind", KINDS)
@pytest.mark.parametrize("attr,t", [("x", pl.T_INT), ("y", pl.T_LONG), ("f", pl.T_FLOAT), ("d", pl.T_DOUBLE)])
def test_ir_words_and_return_type(fn, kind, attr, t):
    """The aggregator entry is (kind, argument expression, argument type); the
    result has the argument's type -- no widening as sum has."""
    qp = plan_of(mc.S + "from S#window.length(3) select %s(%s) as m, sum(%s) as s insert into O;" % (fn, attr, attr))
    (k0, e0, t0), (k1, e1, t1) = qp.plan.aggs
    assert (k0, t0) == (kind, t) and (k1, t1) == (pl.AGG_SUM, t)
    assert qp.output_types[0] == t
    assert qp.output_types[1] == (pl.T_LONG if t in (pl.T_INT, pl.T_LONG) else pl.T_DOUBLE)
    words = np.frombuffer(qp.ir, np.int32)
    assert words[1] == 1                                        # SHD_IR_VERSION
    assert any((words[n:n + 3] == [kind, e0, t]).all() for n in range(len(words) - 2))
    # the function name is matched without regard to case, like sum
    assert plan_of(mc.S + "from S select %s(%s) as m insert into O;" % (fn.upper(), attr)).plan.aggs[0][0] == kind


def test_accepted_wherever_sum_is():
    qp = plan_of(mc.S + "from S#window.length(5) select g, max(d) - min(d) as spread, minForever(x) as lo "
                 "group by g having max(x) > 3 and spread >= 0.0 insert all events into O;")
    assert sorted(a[0] for a in qp.plan.aggs) == [4, 4, 4, 5, 5, 7]   # having re-plans the outputs it names
    assert qp.output_types[1:] == [pl.T_DOUBLE, pl.T_INT]
    # int - long widens as arithmetic does, from the aggregators' own types
    assert plan_of(mc.S + "from S select max(x) - min(y) as r insert into O;").output_types == [pl.T_LONG]
    with pytest.raises(pl.SiddhiAppValidationException, match="not allowed here"):
        plan_of(mc.S + "from S[max(x) > 1] select x insert into O;")


@pytest.mark.parametrize("fn,kind", KINDS)
def test_validation_is_not_an_unsupported_plan(fn, kind):
    for text in ("%s(x, y)" % fn, "%s()" % fn, "%s(k)" % fn):
        with pytest.raises(pl.SiddhiAppCreationException) as ei:
            plan_of(mc.S + "from S#window.length(3) select %s as m insert into O;" % text)
        assert not isinstance(ei.value, pl.UnsupportedPlanException), text


def test_never_offered_to_a_shared_segmented_scan_pass():
    """Length-window group-by queries that differ in the window length share one
    segmented-scan pass (planner.share_groups); a min / max query stays out of
    it -- it runs on the keyed window engine, whatever its window and output."""
    app = qc.parse(mc.S + "from S#window.length(3) select g, sum(d) as s group by g insert into A; "
                   "from S#window.length(9) select g, sum(d) as s group by g insert into A; "
                   "from S#window.length(3) select g, max(d) as s group by g insert into B; "
                   "from S#window.length(9) select g, max(d) as s group by g insert into B; "
                   "from S#window.length(3) select g, sum(d) as s group by g having min(d) > 0.0 insert into C; "
                   "from S#window.length(9) select g, sum(d) as s group by g having min(d) > 0.0 insert into C;")
    qs = list(app.execution_order)
    assert pl.share_signature(qs[0]) is not None
    assert [pl.share_signature(q) for q in qs[2:]] == [None] * 4
    assert pl.share_groups(qs) == [[0, 1]]


def test_time_slices_with_a_halo_refuse_min_max():
    """Multi-GPU time slices rebuild a rank's state from the window's content
    (exchange.window_of); a min / max deque depends on values long expired."""
    from siddhi_amd import exchange
    assert exchange.window_of(plan_of(mc.S + "from S#window.length(9) select sum(d) as s insert into O;")) == ("length", 9)
    with pytest.raises(pl.UnsupportedPlanException, match="min / max"):
        exchange.window_of(plan_of(mc.S + "from S#window.length(9) select max(d) as s insert into O;"))


def test_pattern_output_takes_the_post_section():
    qp = plan_of("define stream A (k string, v double); define stream B (k string, v double); "
                 "from every e1=A -> e2=B[k == e1.k] select max(e2.v) as m, minForever(e1.v) as lo insert into O;")
    assert qp.plan.kind == pl.KIND_STATE and qp.plan.post is not None
