"""min / max / minForever / maxForever on the device (window-x engine:
k_xw_fold<true>, the deque store of engine_window.hip, agg.h mm_step), through
the product path (SiddhiManager -> HipQueryEngine, multi-call send_batch), row
for row and bit for bit against the Python model of the reference's executors
(tests/minmax_model.py, pinned to the oracle in tests/test_minmax.py): values,
nulls, types, timestamps, callback chunks.

The duplicate-valued streams make the reference's deque differ from the true
window extremum (test_minmax.py asserts it on the same workload), so a kernel
computing the true maximum fails here; the distinct-valued stream is checked
against numpy alone, without the model.
"""
import numpy as np
import pytest

import minmax_cases as mc
from kat_runner import check_case, run_case
from parity import assert_same_rows, compile_single_query, concat_rows
from siddhi_amd import planner as pl
from siddhi_amd import runtime as rt

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- generated streams against the model
@pytest.mark.parametrize("case", mc.SHAPES, ids=[c.name for c in mc.SHAPES])
def test_generated_shape_equals_model(hip_available, case):
    """About 3 000 events in three pushes of call sizes 1 / 37 / 1024."""
    d = mc.make_stream(**case.stream)
    want = mc.model_chunks(case.spec, d, case.pushes)
    mc.assert_same(mc.runtime_chunks(case.app, d, None, case.pushes), want)


@pytest.mark.parametrize("name", ["length5-all", "length5-group700", "externalTime-all", "partition-length5",
                                  "lengthBatch4-all-group"])
def test_distinct_values_equal_model(hip_available, name):
    case = next(c for c in mc.SHAPES if c.name == name)
    d = mc.make_stream(**dict(case.stream, domain=0, seed=3))
    mc.assert_same(mc.runtime_chunks(case.app, d, None, case.pushes), mc.model_chunks(case.spec, d, case.pushes))


@pytest.mark.parametrize("name", ["length5-expired-quirk", "length64-double-nulls", "length5-group700",
                                  "lengthBatch4-all-group", "partition-length5"])
def test_snapshot_mid_stream_restores_to_identical_rows(hip_available, name):
    case = next(c for c in mc.SHAPES if c.name == name)
    d = mc.make_stream(**case.stream)
    want = mc.model_chunks(case.spec, d, case.pushes)
    mc.assert_same(mc.runtime_chunks(case.app, d, None, case.pushes, snapshot_after=0), want)
    mc.assert_same(mc.runtime_chunks(case.app, d, None, case.pushes, snapshot_after=1), want)


# ---------------------------------------------------------------- an independent yardstick: numpy, no model
def test_distinct_values_equal_numpy_sliding_extremum(hip_available):
    """With pairwise distinct values the quirk cannot fire: max / min over
    length(64) are the true sliding extrema, maxForever the running maximum."""
    case = mc.Case("numpy", "length(64)", ["i", "max(x)", "min(d)", "maxForever(x)", "minForever(f)"])
    d = mc.make_stream(domain=0, seed=11)
    rows = [r for cur, rem in mc.runtime_chunks(case.app, d, None, mc.PUSHES) for r in cur]
    assert len(rows) > 1000
    x, dd, f = d["x"], d["d"], d["f"]
    run_max = np.maximum.accumulate(x)
    run_min = np.minimum.accumulate(f)
    for ts, (i, mx, mn, fmx, fmn) in rows:
        lo = max(0, i - 63)
        assert ts == mc.T0 + i
        assert mx == int(x[lo:i + 1].max()) and mn == float(dd[lo:i + 1].min()).hex()
        assert fmx == int(run_max[i]) and fmn == float(run_min[i]).hex()


# ---------------------------------------------------------------- the deque store grows
def growth_stream(values):
    n = len(values)
    d = mc.make_stream(n=n, seed=5)
    v = np.asarray(values, np.int64)
    d["x"] = v.astype(np.int32)
    d["d"] = v.astype(np.float64) / 8.0
    return d


GROWTH_PUSHES = [(0, 1800, 1024), (1800, 3400, 1024), (3400, 3560, 37)]


def test_deque_store_grows_and_collapses(hip_available):
    """One state, length(3000), 3 500 strictly descending values: the deque
    holds the whole window, past the store's first allocation (1024 values);
    one large value collapses it to one entry.  A snapshot taken while it is
    long restores to the same rows."""
    values = list(range(20000, 20000 - 3500, -1)) + [10 ** 6] + list(range(59, 0, -1))
    assert len(values) == GROWTH_PUSHES[-1][1]
    case = mc.Case("growth", "length(3000)", ["i", "max(x)", "min(x)", "max(d)"], "expired")
    d = growth_stream(values)
    want = mc.model_chunks(case.spec, d, GROWTH_PUSHES)
    assert any(rem for cur, rem in want)
    mc.assert_same(mc.runtime_chunks(case.app, d, None, GROWTH_PUSHES), want)
    mc.assert_same(mc.runtime_chunks(case.app, d, None, GROWTH_PUSHES, snapshot_after=1), want)


def test_expiries_that_find_nothing_in_a_long_deque(hip_available):
    """600 equal small values, one large value that pops them all, then a
    descending run of 2 900: every expiry of a small value searches a deque of
    thousands and finds nothing (the binary search of agg.h mm_find; a literal
    scan would walk the whole deque each time)."""
    values = [1] * 600 + [10 ** 6] + list(range(9000, 9000 - 2900, -1)) + list(range(59, 0, -1))
    assert len(values) == GROWTH_PUSHES[-1][1]
    case = mc.Case("nofind", "length(3000)", ["i", "max(x)"], "expired")
    d = growth_stream(values)
    want = mc.model_chunks(case.spec, d, GROWTH_PUSHES)
    mc.assert_same(mc.runtime_chunks(case.app, d, None, GROWTH_PUSHES), want)


# ---------------------------------------------------------------- RESET, shd_reset
def test_forever_kinds_keep_their_value_across_lengthbatch_resets(hip_available):
    """lengthBatch(4) RESETs between batches: max / min start over, the Forever
    kinds keep their value, as their reset() does (DESIGN.md 4.4.1 says how the
    reference's state holder treats the object that reset() is called on)."""
    case = mc.Case("forever-reset", "lengthBatch(4)", ["max(x)", "maxForever(x)", "min(x)", "minForever(x)"])
    d = growth_stream([9, 3, 5, 4, 1, 2, 2, 1, 7, 8, 0, 6])
    got = mc.runtime_chunks(case.app, d, None, [(0, 12, 5)])
    assert [vals for cur, rem in got for ts, vals in cur] == [[9, 9, 3, 3], [2, 9, 1, 1], [8, 9, 0, 0]]
    mc.assert_same(got, mc.model_chunks(case.spec, d, [(0, 12, 5)]))


def test_shd_reset_forgets_deques_and_forever_values(hip_available):
    """Distinct values far outside 0..7 first (deques hundreds of entries deep,
    Forever values no later event reaches), then shd_reset: the rows equal a
    fresh query's."""
    from siddhi_amd.hip_engine import DeviceQuery, SHD_MEM_HOST
    case = mc.Case("reset", "length(64)", ["i", "max(x)", "min(x)", "maxForever(x)", "minForever(d)"], "expired")
    qp, dictionary = compile_single_query(case.app)
    d = mc.make_stream(seed=9)
    other = mc.make_stream(seed=10, domain=0)
    assert other["x"].max() > 1000 and other["d"].min() < -100

    def push(dq, src, a, b, call):
        bt = mc.as_batch(src, a, b, call, dictionary)
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


# ---------------------------------------------------------------- over pattern output (POST selector)
def test_max_over_pattern_output(hip_available):
    """The selector of a pattern query runs on one match per chunk, without a
    window: max / minForever are running folds over the matches.  The match set
    comes from the oracle running the same pattern without aggregators."""
    from oracle_engine import OracleQueryEngine
    from siddhi_amd.hip_engine import HipQueryEngine
    from test_gpu_post_selector import _events
    head = ("@app:playback define stream S (symbol string, price float, volume int); @info(name = 'q') "
            "from every e1=S[price > 60] -> e2=S[symbol == e1.symbol and price < e1.price] ")
    rng = np.random.default_rng(7)
    sends = [(1000 + i, ["S%d" % rng.integers(0, 4), float(np.float32(rng.uniform(20, 80))),
                         int(rng.integers(0, 100))]) for i in range(3000)]
    matches = _events(head + "select e1.price as p1, e2.price as p2, e2.volume as v insert into O;",
                      OracleQueryEngine, sends)
    dev = _events(head + "select e1.price as p1, max(e2.price) as hi, min(e2.volume) as lo, "
                  "minForever(e1.price) as lowest insert into O;", HipQueryEngine, sends)
    assert sum(len(c) for c in matches) > 100
    want, hi, lo, lowest = [], None, None, None
    for ts, (p1, p2, v) in [m for chunk in matches for m in chunk]:
        hi = p2 if hi is None or hi < p2 else hi
        lo = v if lo is None or lo > v else lo
        lowest = p1 if lowest is None or lowest > p1 else lowest
        want.append((ts, [p1, hi, lo, lowest]))
    assert [row for chunk in dev for row in chunk] == want


# ---------------------------------------------------------------- the reference's own tests
@pytest.mark.parametrize("case", mc.RUN_KATS, ids=[mc.short(c) for c in mc.RUN_KATS])
def test_reference_known_answer_on_device(hip_available, case):
    from siddhi_amd.hip_engine import HipQueryEngine
    assert check_case(case, run_case(case, HipQueryEngine)) == []


@pytest.mark.parametrize("case", mc.FAIL_KATS, ids=[mc.short(c) for c in mc.FAIL_KATS])
def test_reference_creation_failure_on_device(hip_available, case):
    with pytest.raises(pl.SiddhiAppCreationException) as ei:
        rt.SiddhiManager().createSiddhiAppRuntime(case["app"])
    assert not isinstance(ei.value, pl.UnsupportedPlanException)
