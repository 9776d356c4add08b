"""stdDev / distinctCount / and / or on the device (window-x engine:
k_xw_fold<true, true>, the list store of engine_window.hip, agg.h ext_step),
through the product path (SiddhiManager -> HipQueryEngine, multi-call
send_batch), row for row and bit for bit against the Python model of the
reference's executors (tests/agg_model.py, pinned in tests/test_aggregators.py):
values, nulls, types, timestamps, callback chunks.

Bit equality, not a tolerance: the fold is sequential in the reference's order
and every operation in it is correctly rounded on both sides.  The stdDev
workloads are ones on which a two-pass recomputation gives other bits and on
which the residue of stdDeviation turns negative (NaN), both asserted in
tests/test_aggregators.py.
"""
import numpy as np
import pytest

import agg_cases as ac
import agg_model as am
from kat_runner import run_case
from parity import assert_same_rows, compile_single_query, concat_rows
from siddhi_amd import planner as pl
from siddhi_amd import runtime as rt

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- generated streams against the model
@pytest.mark.parametrize("case", ac.SHAPES, ids=[c.name for c in ac.SHAPES])
def test_generated_shape_equals_model(hip_available, case):
    """About 3 000 events in three pushes of call sizes 1 / 37 / 1024."""
    d = ac.make_stream(**case.stream)
    want = ac.model_chunks(case.spec, d, case.pushes)
    ac.assert_same(ac.runtime_chunks(case.app, d, None, case.pushes), want)


def test_time_window_on_a_stepped_clock(hip_available):
    from siddhi_amd.hip_engine import HipQueryEngine
    case, spec = ac.time_case(["stdDev(d)", "distinctCount(x)", "and(b)", "or(b)"])
    want = ac.collector_chunks(ac.model_collector(case, spec))
    assert sum(len(rem) for cur, rem in want) > 100
    assert ac.collector_chunks(run_case(case, HipQueryEngine)) == want


# ---------------------------------------------------------------- snapshots, shd_reset
@pytest.mark.parametrize("name", ["length4-group700", "lengthBatch3-all", "partition-length4", "distinct-types",
                                  "length4-stddev-all", "bool-nulls"])
def test_snapshot_mid_stream_restores_to_identical_rows(hip_available, name):
    """Plans with distinctCount (their key lists travel in the snapshot) and
    without (stdDev / and / or live in the state tables alone)."""
    case = ac.shape(name)
    d = ac.make_stream(**case.stream)
    want = ac.model_chunks(case.spec, d, case.pushes)
    ac.assert_same(ac.runtime_chunks(case.app, d, None, case.pushes, snapshot_after=0), want)
    ac.assert_same(ac.runtime_chunks(case.app, d, None, case.pushes, snapshot_after=1), want)


def test_shd_reset_then_replay_gives_the_same_rows(hip_available):
    from siddhi_amd.hip_engine import DeviceQuery, SHD_MEM_HOST
    case = ac.Case("reset", "length(64)", ["i", "stdDev(d)", "distinctCount(s)", "distinctCount(x)", "and(b)", "or(b)"],
                   "expired")
    qp, dictionary = compile_single_query(case.app)
    d = ac.make_stream(seed=9)
    other = ac.make_stream(seed=10, domain=500)

    def push(dq, src, a, b, call):
        bt = ac.as_batch(src, a, b, call, dictionary)
        cols = [np.ascontiguousarray(c) for c in bt.cols]
        ts = np.ascontiguousarray(bt.ts, np.int64)
        dq.push_raw(0, bt.n, ts.ctypes.data, [c.ctypes.data for c in cols], [0] * len(cols), SHD_MEM_HOST,
                    bt.call_offsets, True)
        return dq.poll()

    fresh = DeviceQuery(qp.ir)
    want = concat_rows([push(fresh, d, 0, 700, 1), push(fresh, d, 700, 1400, 37)])
    fresh.close()
    dq = DeviceQuery(qp.ir)
    push(dq, other, 1400, 3000, 1024)
    dq.reset()
    got = concat_rows([push(dq, d, 0, 700, 1), push(dq, d, 700, 1400, 37)])
    dq.close()
    assert len(want[2]) > 500
    assert_same_rows(got, want)


# ---------------------------------------------------------------- the key store grows
GROWTH_PUSHES = [(0, 1800, 1024), (1800, 3400, 1024), (3400, 3560, 37)]


def test_key_store_grows_past_its_first_allocation(hip_available):
    """One state, length(5000): 3 200 distinct keys arrive in an order that is
    not their key order (every insert shifts part of the sorted list), so the
    store crosses its first allocation of 1024 words and doubles; then repeats.
    A snapshot taken while the list is long restores to the same rows."""
    n = GROWTH_PUSHES[-1][1]
    d = ac.make_stream(n=n, seed=5)
    v = np.concatenate([np.random.default_rng(6).permutation(3200), np.arange(n - 3200) * 7 % 3200]).astype(np.int64)
    d["x"] = (v - 1500).astype(np.int32)
    d["d"] = v / 7.0
    case = ac.Case("growth", "length(5000)", ["i", "distinctCount(x)", "distinctCount(d)", "stdDev(d)"], "all",
                   pushes=GROWTH_PUSHES)
    want = ac.model_chunks(case.spec, d, GROWTH_PUSHES)
    assert max(vals[1] for cur, rem in want for ts, vals in cur) == 3200
    ac.assert_same(ac.runtime_chunks(case.app, d, None, GROWTH_PUSHES), want)
    ac.assert_same(ac.runtime_chunks(case.app, d, None, GROWTH_PUSHES, snapshot_after=0), want)


def test_keys_expire_in_an_order_other_than_their_insertion(hip_available):
    """length(64) over keys that are re-added while older, other keys expire:
    a key inserted early outlives keys inserted after it, and the removes hit
    the list front, middle and back."""
    d = ac.make_stream(seed=21, domain=90)
    rng = np.random.default_rng(22)
    hot = rng.integers(0, ac.N, ac.N // 3)
    d["x"][hot] = 7                               # one key that never leaves for long
    case = ac.Case("expiry-order", "length(64)", ["i", "distinctCount(x)", "count()"], "expired")
    want = ac.model_chunks(case.spec, d, case.pushes)
    counts = {vals[1] for cur, rem in want for ts, vals in rem}
    assert len(counts) > 8
    ac.assert_same(ac.runtime_chunks(case.app, d, None, case.pushes), want)


# ---------------------------------------------------------------- over pattern output (POST selector)
def test_stddev_and_distinct_count_over_pattern_output(hip_available):
    """The selector of a pattern query runs on one match per chunk, without a
    window: running folds over the matches.  The match set comes from the
    oracle running the same pattern without aggregators, the folds from the model."""
    from oracle_engine import OracleQueryEngine
    from siddhi_amd.hip_engine import HipQueryEngine
    from test_gpu_post_selector import _events
    head = ("@app:playback define stream S (symbol string, price float, volume int); @info(name = 'q') "
            "from every e1=S[price > 60] -> e2=S[symbol == e1.symbol and price < e1.price] ")
    rng = np.random.default_rng(7)
    sends = [(1000 + i, ["S%d" % rng.integers(0, 4), float(np.float32(rng.uniform(20, 80))),
                         int(rng.integers(0, 100))]) for i in range(1500)]
    matches = _events(head + "select e1.price as p1, e2.price as p2, e2.volume as v insert into O;",
                      OracleQueryEngine, sends)
    dev = _events(head + "select e1.price as p1, stdDev(e2.price) as sd, distinctCount(e2.volume) as n, "
                  "stdDev(e2.volume) as sv insert into O;", HipQueryEngine, sends)
    assert sum(len(c) for c in matches) > 100
    sd, dc, sv = am.StdDevState(), am.DistinctCountState(am.T_INT), am.StdDevState()
    want = []
    for ts, (p1, p2, v) in [m for chunk in matches for m in chunk]:
        want.append((ts, [p1, am.norm(sd.add(np.float32(p2))), dc.add(v), am.norm(sv.add(v))]))
    got = [(ts, [am.norm(x) if isinstance(x, float) and n in (1, 3) else x for n, x in enumerate(vals)])
           for chunk in dev for ts, vals in chunk]
    assert got == want


# ---------------------------------------------------------------- refusals
def test_more_than_eight_aggregators_is_an_unsupported_plan(hip_available):
    """The reference's lengthWindowTest4 has 28 aggregators: the engine's
    refusal surfaces as UnsupportedPlanException, not as an error."""
    sel = ", ".join("stdDev(%s) as a%d, distinctCount(%s) as b%d" % (c, n, c, n) for n, c in enumerate("xyfdx"))
    with pytest.raises(pl.UnsupportedPlanException, match="too many aggregators"):
        rt.SiddhiManager().createSiddhiAppRuntime(ac.S + "@info(name = 'q') from S#window.length(4) select " + sel +
                                                  " insert into O;").start()


# ---------------------------------------------------------------- the reference's own tests
@pytest.mark.parametrize("case", ac.RUN_KATS, ids=[ac.short(c) for c in ac.RUN_KATS])
def test_reference_known_answer_on_device(hip_available, case):
    from siddhi_amd.hip_engine import HipQueryEngine
    assert ac.check_kat(case, run_case(case, HipQueryEngine)) == []


@pytest.mark.parametrize("case", ac.FAIL_KATS, ids=[ac.short(c) for c in ac.FAIL_KATS])
def test_reference_creation_failure_on_device(hip_available, case):
    with pytest.raises(pl.SiddhiAppCreationException) as ei:
        rt.SiddhiManager().createSiddhiAppRuntime(case["app"])
    assert not isinstance(ei.value, pl.UnsupportedPlanException)
