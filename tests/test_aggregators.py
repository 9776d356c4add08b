"""stdDev / distinctCount / and / or: the Python model (tests/agg_model.py) that
is their yardstick, the reference's own known answers, and the planner.

The CPU oracle does not know these aggregators (it gives null for a kind it
does not know), so nothing here compares them with it.  The model is pinned in
two halves, as tests/test_minmax.py does: its windows, partition, group-by and
selector batching are tests/minmax_model.py's and run the generated workloads
with sum / avg / count in place of the new kinds against the oracle; its four
executors are restated line by line from C/query/selector/attribute/aggregator/
{StdDev,DistinctCount,And,Or}AttributeAggregatorExecutor.java and checked by
hand here, branch by branch.
"""
import math

import numpy as np
import pytest

import agg_cases as ac
import agg_model as am
from kat_runner import run_case
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
ORACLE_SHAPES = [c for c in ac.SHAPES if c.oracle_ok]


@pytest.mark.parametrize("case", ORACLE_SHAPES, ids=[c.name for c in ORACLE_SHAPES])
def test_model_window_and_selector_equal_the_oracle(case):
    c = case.with_aggs(ac.TO_ORACLE)
    d = ac.make_stream(**c.stream)
    want = ac.model_chunks(c.spec, d, c.pushes)
    ac.assert_same(ac.runtime_chunks(c.app, d, OracleQueryEngine, c.pushes), want)
    if c.spec.events == "expired" or (c.spec.events == "all" and c.spec.group is not None):
        assert any(rem for cur, rem in want), "the shape emits no EXPIRED row"


def test_model_time_window_equals_the_oracle():
    case, spec = ac.time_case(["avg(d)", "count()", "sum(x)"])
    got = ac.collector_chunks(run_case(case, OracleQueryEngine))
    want = ac.collector_chunks(ac.model_collector(case, spec))
    assert got == want and len(want) > 200
    assert sum(len(rem) for cur, rem in want) > 100


# ---------------------------------------------------------------- the executors, by hand
def bits(x):
    return None if x is None else float(x).hex()


def test_stddev_counts_0_1_2_and_back():
    s = am.StdDevState()
    assert s.current() is None                    # count 0
    assert s.add(3.0) == 0.0 and (s.sum, s.mean, s.std, s.count) == (3.0, 3.0, 0.0, 1)
    # count 2: oldMean 3, sum 8, mean 4, stdDeviation += (5 - 3) * (5 - 4) = 2, sqrt(2 / 2) = 1
    assert s.add(5.0) == 1.0 and (s.sum, s.mean, s.std, s.count) == (8.0, 4.0, 2.0, 2)
    # back to 1: oldMean 4, sum 3, mean 3, stdDeviation -= (5 - 4) * (5 - 3) = 2 -> 0; the result is the literal 0.0
    assert s.remove(5.0) == 0.0 and (s.sum, s.mean, s.std, s.count) == (3.0, 3.0, 0.0, 1)
    # to 0: everything zeroed, null
    assert s.remove(3.0) is None and (s.sum, s.mean, s.std, s.count) == (0.0, 0.0, 0.0, 0)
    assert s.add(7.0) == 0.0 and s.mean == 7.0    # refilled: as a fresh state
    s.add(9.0)
    assert s.reset() is None and (s.sum, s.mean, s.std, s.count) == (0.0, 0.0, 0.0, 0)


def test_stddev_three_values_by_hand():
    # 1, 2, 4: means 1, 1.5, 7/3; M2 = 0 + (2-1)(2-1.5) = 0.5; + (4-1.5)(4-7/3)
    s = am.StdDevState()
    s.add(1.0)
    assert s.add(2.0) == math.sqrt(0.5 / 2)
    m3 = 7.0 / 3
    assert bits(s.add(4.0)) == bits(math.sqrt((0.5 + (4.0 - 1.5) * (4.0 - m3)) / 3))
    assert bits(s.mean) == bits(m3)


def test_stddev_null_argument_at_each_count():
    s = am.StdDevState()
    assert am.step("stdDev", s, am.CURRENT, None) is None and s.count == 0
    assert am.step("stdDev", s, am.EXPIRED, None) is None and s.count == 0
    am.step("stdDev", s, am.CURRENT, 2.0)
    assert am.step("stdDev", s, am.CURRENT, None) == 0.0 and s.count == 1
    am.step("stdDev", s, am.CURRENT, 4.0)
    assert am.step("stdDev", s, am.EXPIRED, None) == 1.0 and s.count == 2


def test_stddev_widens_int_long_float():
    for t, vals in ((am.T_INT, [3, 5]), (am.T_LONG, [3 * 10 ** 12, 5 * 10 ** 12]),
                    (am.T_FLOAT, [np.float32(0.1), np.float32(0.7)])):
        s = am.new_state("stdDev", t, True)
        s.add(vals[0])
        a, b = float(vals[0]), float(vals[1])
        mean = (a + b) / 2
        assert bits(s.add(vals[1])) == bits(math.sqrt(((b - a) * (b - mean)) / 2))
    assert float(np.float32(0.1)) != 0.1          # the float widens exactly, it is not re-read as a double literal


def test_stddev_negative_residue_is_nan():
    """Equal values leave a residue of rounding in stdDeviation; a negative one
    gives NaN from the square root (Math.sqrt), and that is the answer."""
    assert math.isnan(am._sqrt(-1e-30)) and bits(am._sqrt(-0.0)) == bits(-0.0)
    case = ac.shape("length4-stddev-all")
    d = ac.make_stream(**case.stream)
    rows = [r for cur, rem in ac.model_chunks(case.spec, d, case.pushes) for r in cur + rem]
    assert sum(1 for ts, vals in rows if vals[1] == "nan") >= 3
    assert not np.isnan(d["d"]).any()             # no NaN went in


def test_folded_stddev_differs_from_a_two_pass_recomputation():
    """Over a sliding length window the reference's incremental update keeps
    residue of values long expired: a kernel recomputing from the window's
    content (numpy.std, two-pass) gives other bits."""
    rng = np.random.default_rng(12)
    x = rng.uniform(0.0, 1000.0, 400)
    m = am.Model(am.Spec(("length", 8), [("stdDev", 0, am.T_DOUBLE)], [("agg", 0)]))
    out = m.run([[(j, [float(v)])] for j, v in enumerate(x)])
    got = [vals[0] for c in out for t, ts, vals in c]
    assert len(got) == 400
    two_pass = [float(np.std(x[max(0, j - 7):j + 1])) for j in range(400)]
    differ = sum(1 for a, b in zip(got, two_pass) if bits(a) != bits(b))
    assert differ >= 1, "the inputs do not tell a fold from a recomputation"
    assert all(abs(a - b) <= 1e-9 * max(1.0, abs(b)) for a, b in zip(got, two_pass))   # and yet it is a stdDev


def test_distinct_count_null_nan_and_signed_zero():
    s = am.DistinctCountState(am.T_DOUBLE)
    nan = float("nan")
    assert [am.step("distinctCount", s, am.CURRENT, v) for v in (None, None, nan, -nan, 0.0, -0.0, 0.0)] == \
        [1, 1, 2, 2, 3, 4, 4]                     # null is a key, every NaN one key, 0.0 and -0.0 two
    assert [am.step("distinctCount", s, am.EXPIRED, v) for v in (None, 0.0, None, -0.0, 0.0, nan, nan)] == \
        [4, 4, 3, 2, 1, 1, 0]
    f = am.DistinctCountState(am.T_FLOAT)
    assert [f.add(np.float32(v)) for v in (0.1, 0.1, np.float32("nan"), np.float32("nan"), -0.0, 0.0)] == [1, 1, 2, 2, 3, 4]


def test_distinct_count_key_goes_1_2_1_0():
    s = am.DistinctCountState(am.T_INT)
    assert s.add(7) == 1 and s.values == {7: 1}
    assert s.add(7) == 1 and s.values == {7: 2}
    assert s.add(8) == 2
    assert s.remove(7) == 2 and s.values == {7: 1, 8: 1}
    assert s.remove(7) == 1 and s.values == {8: 1}
    assert s.remove(7) == 1                       # absent: a no-op here (the reference throws)
    assert s.reset() == 0 and s.values == {}
    for t, a, b in ((am.T_STRING, "p", "q"), (am.T_BOOL, True, False), (am.T_LONG, 2 ** 40, 2 ** 40 + 1)):
        s = am.DistinctCountState(t)
        assert [s.add(a), s.add(b), s.add(a), s.remove(b)] == [1, 2, 2, 1]


def test_and_or_truth_tables():
    for kind, table in (("and", {(0, 0): False, (1, 0): True, (0, 1): False, (1, 1): False, (2, 0): True}),
                        ("or", {(0, 0): False, (1, 0): True, (0, 1): False, (1, 1): True, (0, 2): False})):
        for (nt, nf), want in table.items():
            s = am.new_state(kind, am.T_BOOL, True)
            assert s.current() is False           # both counters at 0: false, never null
            for _ in range(nt):
                s.add(True)
            for _ in range(nf):
                last = s.add(False)
            assert s.current() is want and (s.true, s.false) == (nt, nf)
        s = am.new_state(kind, am.T_BOOL, True)
        s.add(True)
        s.add(False)
        assert s.remove(False) is True and s.remove(True) is False and (s.true, s.false) == (0, 0)
        s.add(True)
        assert s.reset() is False and (s.true, s.false) == (0, 0)


def test_and_or_null_argument_leaves_the_state_alone():
    for kind in ("and", "or"):
        s = am.new_state(kind, am.T_BOOL, True)
        assert am.step(kind, s, am.CURRENT, None) is False
        am.step(kind, s, am.CURRENT, True)
        assert am.step(kind, s, am.CURRENT, None) is True and am.step(kind, s, am.EXPIRED, None) is True
        assert (s.true, s.false) == (1, 0)


def test_lengthbatch_reset_clears_all_four():
    spec = am.Spec(("lengthBatch", 2), [("stdDev", 0, am.T_INT), ("distinctCount", 0, am.T_INT), ("and", 1, am.T_BOOL),
                                        ("or", 1, am.T_BOOL)], [("agg", 0), ("agg", 1), ("agg", 2), ("agg", 3)])
    out = am.Model(spec).run([[(1, [1, False]), (2, [3, True])], [(3, [5, True]), (4, [5, True])]])
    assert [[vals for t, ts, vals in c] for c in out] == [[[1.0, 2, False, True]], [[0.0, 1, True, True]]]


def test_length_window_keys_expire_out_of_insertion_order():
    """length(3) over 5, 1, 5, 9, 2: the key 5 is inserted first and stays
    (re-added) after 1, inserted later, has gone."""
    spec = am.Spec(("length", 3), [("distinctCount", 0, am.T_INT)], [("agg", 0)], "all")
    m = am.Model(spec)
    out = m.run([[(j, [v])] for j, v in enumerate([5, 1, 5, 9, 2])])
    assert [vals[0] for c in out for t, ts, vals in c] == [1, 2, 2, 3, 3]
    assert list(m.states[None][None][0].values) == [5, 9, 2]


# ---------------------------------------------------------------- the reference's own tests
def test_every_known_answer_has_a_spec():
    assert sorted(ac.KAT_SPECS) == sorted(c["name"] for c in ac.RUN_KATS)
    assert len(ac.RUN_KATS) == 18 and len(ac.FAIL_KATS) == 4
    for c in ac.KATS:
        if "stdDev" in c["name"] and "expected_exception" not in c:
            assert c["epsilon"] == 0.00001


@pytest.mark.parametrize("case", ac.RUN_KATS, ids=[ac.short(c) for c in ac.RUN_KATS])
def test_model_reproduces_reference_known_answer(case):
    assert ac.check_kat(case, ac.model_collector(case)) == []


@pytest.mark.parametrize("case", ac.RUN_KATS, ids=[ac.short(c) for c in ac.RUN_KATS])
def test_known_answer_plans(case):
    qp = plan_of(case["app"])
    assert qp.plan.aggs[0][0] in (pl.AGG_STDDEV, pl.AGG_DISTINCT_COUNT, pl.AGG_AND, pl.AGG_OR)


@pytest.mark.parametrize("case", ac.FAIL_KATS, ids=[ac.short(c) for c in ac.FAIL_KATS])
def test_reference_creation_failures(case):
    assert case["expected_exception"] == "SiddhiAppCreationException"
    with pytest.raises(pl.SiddhiAppCreationException) as ei:
        plan_of(case["app"])
    assert not isinstance(ei.value, pl.UnsupportedPlanException)


# ---------------------------------------------------------------- the planner and the parser
KINDS = [("stdDev", pl.AGG_STDDEV, 8), ("distinctCount", pl.AGG_DISTINCT_COUNT, 9), ("and", pl.AGG_AND, 10),
         ("or", pl.AGG_OR, 11)]


def test_kinds_follow_min_forever_in_the_ir():
    assert [k for _, k, _ in KINDS] == [8, 9, 10, 11]
    with open(ac.ROOT + "/include/siddhi_ir.h") as fp:
        text = fp.read()
    for name, k in (("SHD_AGG_STDDEV", 8), ("SHD_AGG_DISTINCT_COUNT", 9), ("SHD_AGG_AND", 10), ("SHD_AGG_OR", 11)):
        assert "%s = %d" % (name, k) in text
    assert "#define SHD_IR_VERSION 1" in text


def test_and_or_in_primary_position_parse_as_function_calls():
    app = qc.parse("define stream S (b bool, c bool); from S select and(b) as a, or(c) as o, b and c as both, "
                   "not (b or c) as neither insert into O;")
    a, o, both, neither = [oa.expr for oa in app.execution_order[0].selector.attrs]
    assert isinstance(a, qc.Func) and a.name == "and" and a.namespace is None and len(a.args) == 1
    assert isinstance(o, qc.Func) and o.name == "or" and len(o.args) == 1
    assert isinstance(both, qc.BinOp) and isinstance(neither, qc.Not)


@pytest.mark.parametrize("attr,t", [("x", pl.T_INT), ("y", pl.T_LONG), ("f", pl.T_FLOAT), ("d", pl.T_DOUBLE),
                                    ("s", pl.T_STRING), ("b", pl.T_BOOL)])
def test_kind_and_return_type(attr, t):
    fns = [("distinctCount", pl.AGG_DISTINCT_COUNT, pl.T_LONG)]
    if t in (pl.T_INT, pl.T_LONG, pl.T_FLOAT, pl.T_DOUBLE):
        fns.append(("stdDev", pl.AGG_STDDEV, pl.T_DOUBLE))
    if t == pl.T_BOOL:
        fns += [("and", pl.AGG_AND, pl.T_BOOL), ("or", pl.AGG_OR, pl.T_BOOL)]
    for fn, kind, rt in fns:
        qp = plan_of(ac.S + "from S#window.length(3) select %s(%s) as m insert into O;" % (fn, attr))
        (k0, e0, t0), = qp.plan.aggs
        assert (k0, t0) == (kind, t) and qp.output_types == [rt]
        words = np.frombuffer(qp.ir, np.int32)
        assert words[1] == 1                                        # SHD_IR_VERSION
        assert any((words[n:n + 3] == [kind, e0, t]).all() for n in range(len(words) - 2))
        # the name is matched without regard to case, like sum
        assert plan_of(ac.S + "from S select %s(%s) as m insert into O;" % (fn.upper(), attr)).plan.aggs[0][0] == kind


def test_accepted_wherever_sum_is():
    qp = plan_of(ac.S + "from S#window.length(5) select g, d > avg(d) + 2.0 * stdDev(d) as outlier, "
                 "distinctCount(s) as pages, and(b) as every group by g having stdDev(x) > 0.5 and pages > 2 "
                 "insert all events into O;")
    assert {pl.AGG_STDDEV, pl.AGG_DISTINCT_COUNT, pl.AGG_AND, pl.AGG_AVG} <= {a[0] for a in qp.plan.aggs}
    assert qp.output_types[1:] == [pl.T_BOOL, pl.T_LONG, pl.T_BOOL]
    with pytest.raises(pl.SiddhiAppValidationException, match="not allowed here"):
        plan_of(ac.S + "from S[stdDev(x) > 1.0] select x insert into O;")
    with pytest.raises(pl.SiddhiAppValidationException, match="not allowed here"):
        plan_of(ac.S + "from S[and(b)] select x insert into O;")


def test_pattern_output_takes_the_post_section():
    qp = plan_of("define stream A (k string, v double); define stream B (k string, v double); "
                 "from every e1=A -> e2=B[k == e1.k] select stdDev(e2.v) as sd, distinctCount(e1.k) as n insert into O;")
    assert qp.plan.kind == pl.KIND_STATE and qp.plan.post is not None


@pytest.mark.parametrize("fn", ["stdDev", "distinctCount", "and", "or"])
def test_wrong_parameter_count_fails_creation(fn):
    for text in ("%s(x, y)" % fn, "%s()" % fn):
        with pytest.raises(pl.SiddhiAppCreationException) as ei:
            plan_of(ac.S + "from S#window.length(3) select %s as m insert into O;" % text)
        assert not isinstance(ei.value, pl.UnsupportedPlanException), text


def test_argument_types():
    def plan(text):
        return plan_of(ac.S + "from S#window.length(3) select %s as m insert into O;" % text)
    for text in ("stdDev(k)", "stdDev(b)"):       # non-numeric: creation fails, as for min / max
        with pytest.raises(pl.SiddhiAppCreationException) as ei:
            plan(text)
        assert not isinstance(ei.value, pl.UnsupportedPlanException), text
    for text in ("and(x)", "or(k)", "and(d)"):    # the reference creates the app and fails every event
        with pytest.raises(pl.UnsupportedPlanException):
            plan(text)
    # an OBJECT argument has no key on the device
    with pytest.raises(pl.UnsupportedPlanException):
        plan_of("define stream A (k string, v double); define stream B (k string, v double); "
                "from every e1=A -> e2=B[k == e1.k]<2:3> select distinctCount(e2.v) as n insert into O;")


def test_never_offered_to_a_shared_segmented_scan_pass():
    texts = ["select g, sum(d) as s group by g insert into A; ", "select g, stdDev(d) as s group by g insert into B; ",
             "select g, distinctCount(x) as s group by g insert into C; ",
             "select g, and(b) as s group by g insert into D; ", "select g, or(b) as s group by g insert into E; ",
             "select g, sum(d) as s group by g having stdDev(d) > 0.0 insert into F; "]
    app = qc.parse(ac.S + "".join("from S#window.length(%d) %s" % (n, t) for t in texts for n in (3, 9)))
    qs = list(app.execution_order)
    assert pl.share_signature(qs[0]) is not None
    assert [pl.share_signature(q) for q in qs[2:]] == [None] * 10
    assert pl.share_groups(qs) == [[0, 1]]


def test_time_slices_with_a_halo_refuse_the_new_kinds():
    from siddhi_amd import exchange
    for text in ("stdDev(d)", "distinctCount(x)", "and(b)", "or(b)"):
        with pytest.raises(pl.UnsupportedPlanException, match="min / max"):
            exchange.window_of(plan_of(ac.S + "from S#window.length(9) select %s as s insert into O;" % text))
