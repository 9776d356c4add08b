"""externalTime sides of a stream-stream join on the device, through the product
path (SiddhiManager -> HipQueryEngine, multi-call send_batch), row for row
against the literal Python model (tests/join_ext_model.py): values, nulls,
event types, timestamps and callback boundaries.  No aggregates, so the
comparison is exact.

The workload (tests/join_ext_cases.py) is about 3 000 events in the three
rounds of join_cases.three_rounds(); tests/test_join_external_time.py asserts,
on the model alone, that it takes the kernels past one LDS tile, one workgroup
of trigger slots and the item store's first allocation.
"""
import numpy as np
import pytest

import join_ext_cases as xc
import join_ext_model as jx
from join_ext_cases import EXT, Shape
from siddhi_amd import hip_engine as he
from siddhi_amd import planner as pl
from siddhi_amd import query_compiler as qc
from siddhi_amd import runtime as rt

pytestmark = pytest.mark.gpu


def _or(l, r):
    return (l[0] is not None and l[0] == r[0]) or l[1] > 19.0


def _gt(l, r):
    return l[0] is not None and l[0] == r[0] and l[1] > r[1]


SHAPES = [Shape("ext x ext, " + k, kind=k) for k in xc.WORDS]
SHAPES += [
    Shape("ext x length(3)", EXT, ("length", 3), kind="full_outer"),
    Shape("length(1) x ext", ("length", 1), EXT, kind="full_outer"),
    Shape("ext x none", EXT, None, kind="left_outer"),
    Shape("ext x none, right outer", EXT, None, kind="right_outer"),
    Shape("none x ext", None, EXT),
    Shape("unidirectional left", kind="left_outer", uni=0),
    Shape("unidirectional right", kind="full_outer", uni=1),
    Shape("insert into", events="current"),
    Shape("insert into, outer", events="current", kind="full_outer"),
    Shape("expired events", events="expired"),
    Shape("expired events, outer", events="expired", kind="full_outer"),
    Shape("a filter on each side", fa=("price > 3.0", lambda d: d[1] > 3.0),
          fb=("lim < 15.0 and k >= 0", lambda d: d[1] < 15.0 and d[0] is not None and d[0] >= 0), nulls=True),
    Shape("null keys and null event times", kind="full_outer", nulls=True),
    Shape("interpreted condition", on="a.k == b.k or a.price > 19.0", on_fn=_or, nulls=True),
    Shape("non-equi condition", on="a.price > b.lim and a.k == b.k", on_fn=_gt),
    Shape("no condition, small", on=None, plan=[(1, [70]), (0, [40, 3, 1]), (1, [5])]),
    Shape("one event per push", kind="full_outer", plan=[(s, [1]) for s in (0, 1, 0, 0, 1, 1, 0, 1) * 6]),
]


def new_runtime(app, got):
    r = rt.SiddhiManager().createSiddhiAppRuntime(app)
    r.addCallback("q", rt._FnQueryCallback(
        lambda ts, cur, rem: got.append(([(e.timestamp, list(e.data)) for e in (cur or [])],
                                         [(e.timestamp, list(e.data)) for e in (rem or [])]))))
    r.start()
    return r


def send(r, side, calls):
    stream = "AB"[side]
    if len(calls) > 1:
        assert r._batch_push_ok(stream), "a multi-call send_batch must go down as one push"
    r.getInputHandler(stream).send_batch(xc.to_batch(side, calls))


def device_run(app, sends, snapshot_after=None, reset_after=None, engine="window-join"):
    """Callbacks of the app over the sends.  snapshot_after = p: the state is
    saved after send p and the rest runs in a fresh runtime restored from it;
    reset_after = p: the query is reset (shd_reset) after send p."""
    got = []
    r = new_runtime(app, got)
    if engine is not None:
        assert r.queries[0].engine.engine_name == engine
    for p, (side, calls) in enumerate(sends):
        send(r, side, calls)
        if snapshot_after == p:
            image = r.snapshot()
            r.shutdown()
            r = new_runtime(app, got)
            r.restore(image)
        if reset_after == p:
            r.queries[0].engine.dq.reset()
    r.shutdown()
    return got


def assert_same(got, want):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, "callback %d of %d" % (k, len(want))


@pytest.mark.parametrize("shape", SHAPES, ids=[s.name for s in SHAPES])
def test_generated_streams_match_the_model(shape):
    sends = shape.sends()
    want, _ = xc.model_run(shape.spec, sends)
    assert want
    assert_same(device_run(shape.app, sends), want)


def test_filtered_events_do_not_move_the_sides_clock():
    """A's filter drops the event whose `et` would have expired everything."""
    s = Shape("filter", fa=("price > 3.0", lambda d: d[1] > 3.0), kind="left_outer")
    sends = [(1, [[(1, [1, 9.0, 100])]]),
             (0, [[(2, [1, 5.0, 100]), (3, [1, 5.0, 101])]]),
             (0, [[(4, [1, 1.0, 100_000])], [(5, [1, 4.0, 102])]]),           # the jump is filtered out
             (0, [[(6, [1, 4.0, 101 + xc.T]), (7, [2, 4.0, 101 + xc.T])]])]   # expires et 100 and 101, not 102
    want, st = xc.model_run(s.spec, sends)
    assert st["max_expired_by_one_event"] == 2 and sum(len(e) for _, e in want) == 2
    assert_same(device_run(s.app, sends), want)


def test_snapshot_after_the_first_send_and_restore():
    s = Shape("snapshot", kind="full_outer")
    sends = s.sends()
    assert_same(device_run(s.app, sends, snapshot_after=0), xc.model_run(s.spec, sends)[0])


def test_snapshot_of_a_grown_window_and_restore():
    """More items than a fresh runtime's first allocation travel in the image."""
    s = Shape("snapshot, grown", kind="full_outer")
    sends = s.sends()
    p = len(sends) - 2          # after A's push of 1024 events
    want, _ = xc.model_run(s.spec, sends)
    head, st = xc.model_run(s.spec, sends[:p + 1])
    assert st["max_carried"] > 1024
    assert_same(device_run(s.app, sends, snapshot_after=p), want)


def test_reset_forgets_both_windows():
    s = Shape("reset", kind="left_outer", plan=[(1, [80]), (0, [30]), (0, [20]), (1, [5])])
    sends = s.sends()
    want = xc.model_run(s.spec, sends[:2])[0] + xc.model_run(s.spec, sends[2:])[0]
    assert_same(device_run(s.app, sends, reset_after=1), want)


def test_left_outer_join_with_an_empty_side_equals_the_single_stream_window():
    """The independent yardstick: B holds nothing, so every CURRENT and EXPIRED
    event of A's window comes out once -- the rows and chunks of the
    single-stream externalTime window (checked against the C++ oracle in
    tests/test_gpu_kat.py and tests/test_gpu_window_x.py)."""
    sends = [sd for sd in xc.gen_sends() if sd[0] == 0]
    t = 300     # A alone is sparser in `et` than both streams together: a shorter window, so that most items expire
    gone = sum(len(g) for g, _ in jx.literal_windows([e[1][xc.ET] for _, cs in sends for c in cs for e in c], t))
    assert gone > 256
    join = ("@app:playback " + xc.STREAMS + "@info(name = 'q') from A#window.externalTime(et, %d) as a "
            "left outer join B as b select a.k, a.et insert all events into O;" % t)
    single = ("@app:playback " + xc.STREAMS + "@info(name = 'q') from A#window.externalTime(et, %d) "
              "select k, et insert all events into O;" % t)
    got = device_run(join, sends)
    assert sum(len(e) for _, e in got) == gone
    assert sum(len(c) for c, _ in got) == sum(len(c) for _, cs in sends for c in cs)
    assert_same(got, device_run(single, sends, engine=None))


def test_in_seq_of_an_expired_trigger_is_the_expirers():
    """shd_out.in_seq of a row from an EXPIRED trigger: the arrival index of the
    event that pushed the item out; its chunk: that event's call."""
    app = qc.parse(xc.STREAMS + "from A#window.externalTime(et, 10) as a left outer join B as b "
                   "select a.k as ak, a.et as aet insert all events into O;")
    qp = pl.plan_query(app, app.queries[0], pl.StringDictionary())
    dq = he.DeviceQuery(qp.ir)
    assert dq.engine_kind == 5

    def push(ets, t0):
        n = len(ets)
        ts = np.arange(t0, t0 + n, dtype=np.int64)
        cols = [np.arange(n, dtype=np.int32), np.zeros(n, np.float32), np.array(ets, np.int64)]
        dq.set_time(int(ts[-1]))
        dq.push_raw(0, n, ts.ctypes.data, [c.ctypes.data for c in cols], [0, 0, 0])
        r = dq.poll(with_seq=True)
        return (r[1].tolist(), r[2].tolist(), r[5].tolist()) if r is not None else None

    # types, timestamps, in_seq
    assert push([100, 105], 1000) == ([0, 0], [1000, 1001], [0, 1])
    # 110 expires et 100 (stamped 110), 90 expires nothing, 200 expires 105, 110 and 90 (stamped 200)
    assert push([110, 90, 200], 2000) == ([1, 0, 0, 1, 1, 1, 0], [110, 2000, 2001, 200, 200, 200, 2002],
                                          [2, 2, 3, 4, 4, 4, 4])
    dq.close()


def test_a_million_items_behind_one_head():
    """More items than 1024 tiles of the running-maximum scan (a third level
    of its recursion), with `et` falling from the first item on: the maximum
    has to travel from item 0 through every tile, or a later item sees a lower
    one and expires items that are blocked behind the head.  Nothing expires
    until an event moves the clock past the head; then everything does, in one
    push of a million EXPIRED triggers, three of which find B's item."""
    n = (1 << 20) + 1024 + 5
    hits = [3, 1 << 10, n - 2]
    app = ("@app:playback " + xc.STREAMS + "@info(name = 'q') from A#window.externalTime(et, 10) as a "
           "join B#window.length(1) as b on a.k == b.k select a.price as price, a.et as aet, b.et as bet "
           "insert expired events into O;")
    got = []
    r = new_runtime(app, got)
    assert r.queries[0].engine.engine_name == "window-join"

    def batch(ts0, k, price, et):
        m = len(k)
        return rt.ColumnBatch(np.arange(ts0, ts0 + m, dtype=np.int64),
                              [np.asarray(k, np.int32), np.asarray(price, np.float32), np.asarray(et, np.int64)],
                              [None, None, None], np.array([0, m], np.int64))

    r.getInputHandler("B").send_batch(batch(1, [7], [0.0], [55]))
    k = np.zeros(n, np.int32)
    k[hits] = 7
    et = n - np.arange(n, dtype=np.int64)          # n, n - 1, ..., 1
    r.getInputHandler("A").send_batch(batch(10, k, np.arange(n) % 1000, et))
    assert got == []
    r.getInputHandler("A").send_batch(batch(10 + n, [0, 0], [0.0, 0.0], [n + 9, 5]))     # n - (n + 9) + 10 > 0
    assert got == []
    r.getInputHandler("A").send_batch(batch(20 + n, [0], [0.0], [n + 10]))
    r.shutdown()
    # everything before the last event goes, the two events of the third push (k = 0) included
    assert got == [([], [(n + 10, [float(i % 1000), n - i, 55]) for i in hits])]
