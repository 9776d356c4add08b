"""Stream-stream window joins on the device, through the product path
(SiddhiManager -> HipQueryEngine, multi-call send_batch), row for row against
the Python model of the reference's join (tests/join_model.py): values, nulls,
event types, timestamps and callback boundaries.  No aggregates, so the
comparison is exact.

The first group is the reference's own join tests (tests/golden/kat_join); the
second is generated two-stream workloads around the kernels' tile numbers
(engine_join.hip: kJoinTrig trigger slots per workgroup, kJoinTile items per LDS
tile).  `time` sides are refused by the planner, so the
reference's time cases and generated time shapes are not run here; the CPU
tests check the refusal and run those cases through the model.
"""
import numpy as np
import pytest

import join_cases as jc
import join_model as jm
from kat_runner import check_case, run_case
from siddhi_amd import hip_engine as he
from siddhi_amd import planner as pl
from siddhi_amd import query_compiler as qc
from siddhi_amd import runtime as rt

pytestmark = pytest.mark.gpu

TRIG, TILE = jc.JOIN_TRIG, jc.JOIN_TILE
EVENTS = {"current": "", "all": "all events ", "expired": "expired events "}
WORDS = {"inner": "join", "left_outer": "left outer join", "right_outer": "right outer join",
         "full_outer": "full outer join"}


# ---------------------------------------------------------------- the reference's cases
@pytest.mark.parametrize("case", jc.RUN_CASES, ids=[jc.short(c) for c in jc.RUN_CASES])
def test_reference_known_answer_on_device(case):
    col = run_case(case, None)
    errs = check_case(case, col) + jc.check_extras(case, col)
    assert not errs, "%s (%s): %s" % (case["name"], case["source"], errs)
    assert jc.collector_rows(col) == jc.collector_rows(jc.model_collector(case))


# ---------------------------------------------------------------- generated workloads
def side_text(stream, alias, window, flt, uni):
    return "%s%s%s as %s%s" % (stream, "[%s]" % flt if flt else "", "#window.length(%d)" % window if window else "",
                               alias, " unidirectional" if uni else "")


class Shape:
    """One generated case: the app's text and the model's spec from the same parameters."""

    def __init__(self, name, wa, wb, kind="inner", on="a.k == b.k", on_fn=None, events="current", fa=None, fb=None,
                 uni=None, plan=None, keys=16, nulls=False, rows_max=200_000):
        self.name, self.plan, self.keys, self.nulls, self.rows_max = name, plan, keys, nulls, rows_max
        self.app = ("@app:playback " + jc.GEN_STREAMS + "@info(name = 'q') from " +
                    side_text("A", "a", wa, fa and fa[0], uni == 0) + " " + WORDS[kind] + " " +
                    side_text("B", "b", wb, fb and fb[0], uni == 1) + (" on " + on if on else "") + " " +
                    jc.GEN_SELECT + "insert " + EVENTS[events] + "into O;")
        if on and on_fn is None:
            on_fn = lambda l, r: l[0] is not None and l[0] == r[0]   # noqa: E731  a.k == b.k (null -> false)
        self.spec = jm.Spec(jm.Side(("length", wa) if wa else None, fa and fa[1], uni == 0),
                            jm.Side(("length", wb) if wb else None, fb and fb[1], uni == 1),
                            jc.gen_select, on_fn if on else None, kind, events)

    def sends(self):
        return jc.gen_sends(self.plan or jc.three_rounds(), self.keys, nulls=self.nulls)


def _gt(l, r):
    return l[0] is not None and l[0] == r[0] and l[1] > r[1]


def _or(l, r):
    return (l[0] is not None and l[0] == r[0]) or l[1] > 18.0


SHAPES = [Shape("window=%d" % w, 5, w, keys=max(4, w // 4), events="all")
          for w in (TILE - 1, TILE, TILE + 1, 2 * TILE + 3)]
SHAPES += [
    Shape("length(1) both sides", 1, 1, keys=3, events="all"),
    Shape("calls of kJoinTrig and kJoinTrig+1 triggers", 9, 40, plan=[(1, [100]), (0, [TRIG]), (0, [TRIG + 1])]),
    Shape("filled in one push, read in the next", 9, 200, keys=40, plan=[(1, [200]), (0, [50]), (1, [7]), (0, [3])]),
    Shape("still-empty side, inner", 9, 40, plan=[(0, [40, 3, 1])]),
    Shape("still-empty side, left outer", 9, 40, kind="left_outer", events="all", plan=[(0, [40, 3, 1])]),
    Shape("nothing satisfies, inner", 5, TILE + 1, on="a.k == b.k and a.k < 0", on_fn=lambda l, r: False),
    Shape("nothing satisfies, full outer", 5, TILE + 1, kind="full_outer", on="a.k == b.k and a.k < 0",
          on_fn=lambda l, r: False, events="all"),
    Shape("everything satisfies, 300 x 300", 300, 300, on=None, plan=[(1, [300]), (0, [300])]),
    Shape("non-equi condition", 7, TILE + 1, on="a.price > b.lim and a.k == b.k", on_fn=_gt, keys=6),
    Shape("interpreted condition", 7, TILE + 1, on="a.k == b.k or a.price > 18.0", on_fn=_or, nulls=True),
    Shape("a filter on each side", 7, TILE + 1, fa=("price > 3.0", lambda d: d[1] > 3.0),
          fb=("lim < 15.0 and k >= 0", lambda d: d[1] < 15.0 and d[0] is not None and d[0] >= 0), nulls=True),
    Shape("null keys", 7, TILE + 1, kind="full_outer", events="all", nulls=True),
]
SHAPES += [Shape(k, 9, TILE + 1, kind=k, events="all") for k in WORDS]
SHAPES += [
    Shape("unidirectional left", 9, TILE + 1, kind="left_outer", uni=0, events="all"),
    Shape("unidirectional right", 9, TILE + 1, kind="full_outer", uni=1, events="all"),
    Shape("expired events", 7, TILE + 1, events="expired"),
    Shape("expired events, outer", 7, TILE + 1, kind="full_outer", events="expired", keys=40),
    Shape("windowless left side", 0, TILE + 1, events="all"),
    Shape("windowless right side, right outer", 9, 0, kind="right_outer", events="all"),
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
    r.getInputHandler(stream).send_batch(jc.to_batch(side, calls))


def device_run(app, sends, snapshot_after=None, reset_after=None):
    """Callbacks of the app over the sends.  snapshot_after = p: the state is
    saved after send p and the rest runs in a fresh runtime restored from it;
    reset_after = p: the query is reset (shd_reset) after send p."""
    got = []
    r = new_runtime(app, got)
    assert r.queries[0].engine.engine_name == "window-join"
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


@pytest.mark.parametrize("shape", SHAPES, ids=[s.name for s in SHAPES])
def test_generated_streams_match_the_model(shape):
    sends = shape.sends()
    want = jc.model_run(shape.spec, sends)
    assert sum(len(c) + len(e) for c, e in want) < shape.rows_max
    got = device_run(shape.app, sends)
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, "callback %d of %d" % (k, len(want))


def test_shapes_cover_what_they_claim():
    """The generated workloads do reach the cases they are named for."""
    by = {s.name: s for s in SHAPES}
    assert jc.model_run(by["nothing satisfies, inner"].spec, by["nothing satisfies, inner"].sends()) == []
    full = jc.model_run(by["nothing satisfies, full outer"].spec, by["nothing satisfies, full outer"].sends())
    assert full and all(row[1][0] is None or row[1][3] is None for c, e in full for row in c + e)
    assert sum(len(c) for c, _ in jc.model_run(by["everything satisfies, 300 x 300"].spec,
                                               by["everything satisfies, 300 x 300"].sends())) == 300 * 300
    # a small key alphabet: a trigger of A meets anything from no item to eight and more of B's window
    s = by["window=%d" % (2 * TILE + 3)]
    held, met = [], set()
    for side, calls in s.sends():
        for ts, (k, _, _) in (e for call in calls for e in call):
            if side == 1:
                held = (held + [k])[-(2 * TILE + 3):]
            else:
                met.add(held.count(k))
    assert 0 in met and max(met) >= 8


def test_snapshot_after_the_second_push_and_restore():
    s = Shape("snapshot", 9, TILE + 1, kind="full_outer", events="all")
    sends = s.sends()
    assert device_run(s.app, sends, snapshot_after=1) == jc.model_run(s.spec, sends)


def test_reset_forgets_both_windows():
    s = Shape("reset", 9, TILE + 1, kind="left_outer", events="all", plan=[(1, [80]), (0, [30]), (0, [20]), (1, [5])])
    sends = s.sends()
    want = jc.model_run(s.spec, sends[:2]) + jc.model_run(s.spec, sends[2:])
    assert device_run(s.app, sends, reset_after=1) == want


def test_in_seq_and_state_idx():
    """shd_out.in_seq: the arrival index, over both streams, of the event whose
    call produced the row; state_idx: the trigger side's stream index."""
    app = qc.parse(jc.GEN_STREAMS + "from A#window.length(2) as a full outer join B#window.length(3) as b "
                   "on a.k == b.k " + jc.GEN_SELECT + "insert all events into O;")
    qp = pl.plan_query(app, app.queries[0], pl.StringDictionary())
    dq = he.DeviceQuery(qp.ir)
    assert dq.engine_kind == 5

    def push(side, ks, t0):
        n = len(ks)
        ts = np.arange(t0, t0 + n, dtype=np.int64)
        cols = [np.array(ks, np.int32), np.zeros(n, np.float32), np.arange(n, dtype=np.int64)]
        dq.set_time(int(ts[-1]))
        dq.push_raw(side, n, ts.ctypes.data, [c.ctypes.data for c in cols], [0, 0, 0])
        r = dq.poll(with_seq=True)
        return (r[1].tolist(), r[5].tolist(), dq.last_state_idx.tolist()) if r is not None else None

    assert push(1, [1, 2, 1], 10) == ([0, 0, 0], [0, 1, 2], [1, 1, 1])             # outer rows of B
    assert push(0, [1, 3], 20) == ([0, 0, 0], [3, 3, 4], [0, 0, 0])                # A k=1 meets two, k=3 none
    # A's third event pushes out its first (EXPIRED, two matches), then joins itself (one match)
    assert push(0, [2], 30) == ([1, 1, 0], [5, 5, 5], [0, 0, 0])
    dq.close()
