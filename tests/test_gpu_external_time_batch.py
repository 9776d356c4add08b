"""externalTimeBatch on the device, through the product path (SiddhiManager ->
HipQueryEngine, multi-call send_batch), row for row against the Python model
of the reference's processor (tests/etb_model.py): values, event types,
timestamps and callback boundaries.

Comparison is exact.  The window-x engine folds each aggregator state
sequentially in the reference's order (k_xw_fold: sum += v, avg = sum / count
at emission), so sum / avg doubles equal the model's float64 fold in the same
order bit for bit.

Reference: C/query/processor/stream/window/ExternalTimeBatchWindowProcessor.java
:238-311, :313-334, :336-383, :440-456.
"""
import numpy as np
import pytest

import etb_model as em
from kat_runner import check_case, run_case
from siddhi_amd import runtime as rt
from test_external_time_batch import FAIL_CASES, RUN_CASES, check_extras, short

pytestmark = pytest.mark.gpu

ATTRS = ["i", "k", "g", "v", "et", "st"]
S = "@app:playback define stream S (i long, k string, g string, v double, et long, st long); "
SEL = {"i": ("attr", 0), "k": ("attr", 1), "g": ("attr", 2), "v": ("attr", 3), "et": ("attr", 4),
       "count() as c": ("count",), "sum(v) as s": ("sum", 3), "avg(v) as a": ("avg", 3), "sum(i) as si": ("sum", 0),
       "avg(i) as ai": ("avg", 0)}
T_EVENT0 = 1_000_000          # playback timestamps: T_EVENT0 + event index
PUSHES = [(0, 1500, 1), (1500, 3000, 37), (3000, 4500, 1024)]   # (first event, end, call size)


def make_stream(n=4500, seed=0, nkeys=1, ngroups=5, T=8, quiet=None, strict=False, late_key=None, st_ahead=False):
    """Events with late timestamps (below the running maximum), timestamps on
    a window boundary (small integer steps against a small T make them
    common), gaps of many windows; `quiet` = (a, b): et does not move over
    those events (no trigger); `strict`: et rises by one per event; `late_key`:
    index from which one more key appears."""
    rng = np.random.default_rng(seed)
    key = rng.integers(0, nkeys, n)
    if late_key is not None:
        key[late_key + rng.choice(n - late_key, 40, replace=False)] = nkeys
    grp = rng.integers(0, ngroups, n)
    v = rng.integers(1, 4000, n) / 8.0
    et = np.zeros(n, np.int64)
    cur = 5000
    steps = rng.choice([0, 0, 1, 1, 2, 3, 5 * T + 1, 40 * T, -1, -T - 2], n)
    for j in range(n):
        if strict:
            cur += 1
            et[j] = cur
        elif quiet and quiet[0] <= j < quiet[1]:
            et[j] = cur
        elif steps[j] < 0:
            et[j] = max(0, cur + steps[j])
        else:
            cur += int(steps[j])
            et[j] = cur
    st = et - rng.integers(0, 2 * T + 1, n)
    if st_ahead:                  # a startTime attribute ahead of the key's first events
        st = np.where(key % 2 == 0, et + 3 * T + rng.integers(0, T, n), st)
    return {"i": np.arange(n, dtype=np.int64), "k": key, "g": grp, "v": v, "et": et, "st": st}


def as_events(d):
    return [(T_EVENT0 + j, [j, "K%04d" % d["k"][j], "G%04d" % d["g"][j], float(d["v"][j]), int(d["et"][j]),
                            int(d["st"][j])]) for j in range(len(d["i"]))]


def as_batch(d, a, b, call, dictionary):
    kid = np.array([dictionary.id("K%04d" % x) for x in d["k"][a:b]], np.uint32)
    gid = np.array([dictionary.id("G%04d" % x) for x in d["g"][a:b]], np.uint32)
    offs = np.append(np.arange(0, b - a, call, dtype=np.int64), np.int64(b - a))
    ts = T_EVENT0 + np.arange(a, b, dtype=np.int64)
    return rt.ColumnBatch(ts, [d["i"][a:b].copy(), kid, gid, d["v"][a:b].copy(), d["et"][a:b].copy(),
                               d["st"][a:b].copy()], [None] * 6, offs), offs


def app_text(window, select, events="", group=False, part=False):
    q = "@info(name = 'q') from S#window.externalTimeBatch(%s) select %s %sinsert %sinto O;" % (
        window, ", ".join(select), "group by g " if group else "", events + " " if events else "")
    return S + ("partition with (k of S) begin %s end;" % q if part else q)


def spec_of(T, select, events="", group=False, part=False, start=("none", 0), replace=False):
    return em.Spec(4, T, start[0], start[1], replace, [SEL[s] for s in select], [2] if group else [],
                   {"": "current", "all events": "all", "expired events": "expired"}[events], 1 if part else None)


def new_runtime(app, got):
    r = rt.SiddhiManager().createSiddhiAppRuntime(app)
    r.addCallback("q", rt._FnQueryCallback(
        lambda ts, cur, rem: got.append(([(e.timestamp, list(e.data)) for e in (cur or [])],
                                         [(e.timestamp, list(e.data)) for e in (rem or [])]))))
    r.start()
    return r


def device_chunks(app, d, pushes=PUSHES, snapshot_after=None):
    """Callbacks of the app over the pushes; with snapshot_after = p the state
    is saved after push p and the rest runs in a fresh runtime restored from it."""
    got = []
    r = new_runtime(app, got)
    for p, (a, b, call) in enumerate(pushes):
        batch, _ = as_batch(d, a, b, call, r.dictionary)
        assert r._batch_push_ok("S"), "a multi-call send_batch must go down as one push"
        r.getInputHandler("S").send_batch(batch)
        if snapshot_after == p:
            image = r.snapshot()
            r.shutdown()
            r = new_runtime(app, got)
            r.restore(image)
    r.shutdown()
    return got


def model_chunks(spec, d, pushes=PUSHES, per_push=None):
    m = em.Model(spec)
    evs = as_events(d)
    out = []
    for a, b, call in pushes:
        calls = [evs[x:min(x + call, b)] for x in range(a, b, call)]
        chunks = m.run(calls)
        if per_push is not None:
            per_push.append(chunks)
        out.extend(chunks)
    return [([(ts, vals) for t, ts, vals in c if t == em.CURRENT], [(ts, vals) for t, ts, vals in c if t == em.EXPIRED])
            for c in out]


def assert_same(dev, want):
    assert len(want) > 0
    for n, (a, b) in enumerate(zip(dev, want)):
        assert a == b, "callback %d: device %r != model %r" % (n, a, b)
    assert len(dev) == len(want)


def check(window, T, select, events="", group=False, part=False, start=("none", 0), replace=False, **stream):
    d = make_stream(T=T, **stream)
    want = model_chunks(spec_of(T, select, events, group, part, start, replace), d)
    assert_same(device_chunks(app_text(window, select, events, group, part), d), want)
    return want


EVENTS = ["", "all events", "expired events"]


@pytest.mark.parametrize("events", EVENTS)
def test_projection(hip_available, events):
    """Call sizes 1, 37 and 1024 over three pushes; late, boundary-equal and
    far-ahead timestamps."""
    check("et, 8", 8, ["i", "k", "v", "et"], events, seed=1)


def test_batches_cross_the_push_boundary(hip_available):
    """The model's first callback of push 2 expires a batch and emits a batch
    that both arrived in push 1: one batch stayed open and one awaited its
    expiry across the push (and so on the device, row for row)."""
    d = make_stream(T=8, seed=1)
    per = []
    model_chunks(spec_of(8, ["i", "k", "v", "et"], "all events"), d, per_push=per)
    first = per[1][0]
    assert any(t == em.EXPIRED and vals[0] < 1500 for t, _, vals in first)
    assert any(t == em.CURRENT and vals[0] < 1500 for t, _, vals in first)


@pytest.mark.parametrize("events", EVENTS)
def test_count_without_group_by(hip_available, events):
    """The reference tests' shape: one row per flush."""
    check("et, 8", 8, ["et", "k", "count() as c"], events, seed=2)


@pytest.mark.parametrize("events", EVENTS)
def test_sum_avg_five_groups(hip_available, events):
    check("et, 50", 50, ["g", "sum(v) as s", "avg(v) as a", "count() as c", "avg(i) as ai"], events, group=True,
          seed=3, ngroups=5)


def test_sum_avg_700_groups(hip_available):
    check("et, 2 sec", 2000, ["g", "sum(v) as s", "avg(v) as a", "sum(i) as si"], "all events", group=True, seed=4,
          ngroups=700)


def test_push_without_a_trigger(hip_available):
    """et stands still over the whole second push: it emits nothing and the
    open batch grows across it."""
    select = ["i", "et", "count() as c"]
    check("et, 8", 8, select, "all events", seed=5, quiet=(1500, 3000))
    per = []
    model_chunks(spec_of(8, select, "all events"), make_stream(T=8, seed=5, quiet=(1500, 3000)), per_push=per)
    assert len(per[0]) > 0 and len(per[1]) == 0 and len(per[2]) > 0


def test_every_event_triggers(hip_available):
    """T = 1 and strictly rising timestamps: a flush per event."""
    want = check("et, 1", 1, ["i", "et"], "all events", seed=6, strict=True)
    assert len(want) == 4499


@pytest.mark.parametrize("name,window,start", [
    ("const-below", "et, 8, 1203", ("const", 1203)),
    ("const-above", "et, 8, 9001", ("const", 9001)),       # above the first timestamps: negative remainders
    ("const-far-above", "et, 50, 100000000", ("const", 100000000)),   # never reached
    ("attr", "et, 8, st", ("attr", 5)),
])
def test_start_time(hip_available, name, window, start):
    T = int(window.split(",")[1])
    check(window, T, ["i", "et", "count() as c"], "all events", start=start, seed=7)


def test_start_time_attribute_per_key(hip_available):
    """Each key reads startTime from its own first event; for half the keys it
    lies ahead of their first timestamps."""
    check("et, 8, st", 8, ["i", "k", "et"], "all events", part=True, start=("attr", 5), seed=8, nkeys=12,
          st_ahead=True)


@pytest.mark.parametrize("select,group", [(["i", "et", "k"], False), (["g", "et", "sum(v) as s"], True)])
def test_replace_timestamp_with_batch_end_time(hip_available, select, group):
    """The appended clone's timestamp attribute is the endTime in force: in the
    CURRENT rows and in the later EXPIRED copies."""
    check("et, 8, 1203, 0, true", 8, select, "all events", group=group, start=("const", 1203), replace=True, seed=9)


@pytest.mark.parametrize("events", EVENTS)
def test_partitioned_three_keys(hip_available, events):
    """Flushes of different keys interleave inside the calls of 37 and 1024
    events: callbacks come in the order of their trigger events."""
    check("et, 8", 8, ["i", "k", "sum(v) as s", "count() as c"], events, part=True, seed=10, nkeys=3)


def test_partitioned_600_keys_grouped(hip_available):
    """About 600 keys, one of them first seen in the last push."""
    want = check("et, 20", 20, ["k", "g", "avg(v) as a", "count() as c"], "all events", group=True, part=True,
                 seed=11, nkeys=600, ngroups=4, late_key=3100)
    assert any(vals[0] == "K0600" for cur, _ in want for _, vals in cur)


def test_two_keys_interleave_inside_one_call(hip_available):
    """One call: A opens, B opens, A's trigger, B's trigger, A's trigger --
    three callbacks in that order."""
    rows = [("A", 0), ("B", 3), ("A", 5), ("B", 4), ("A", 12), ("B", 20), ("A", 25), ("B", 21)]
    n = len(rows)
    d = {"i": np.arange(n, dtype=np.int64), "k": np.array([0 if k == "A" else 1 for k, _ in rows]),
         "g": np.zeros(n, np.int64), "v": np.ones(n), "et": np.array([t for _, t in rows], np.int64),
         "st": np.zeros(n, np.int64)}
    pushes = [(0, n, n)]
    select = ["i", "k", "count() as c"]
    want = model_chunks(spec_of(10, select, "all events", part=True), d, pushes)
    assert [cur[-1][1][1] for cur, _ in want] == ["K0000", "K0001", "K0000"]
    assert_same(device_chunks(app_text("et, 10", select, "all events", part=True), d, pushes), want)


@pytest.mark.parametrize("part", [False, True])
def test_snapshot_restore_mid_stream(hip_available, part):
    """snapshot() after push 2, restore() into a fresh runtime, push 3: the
    rows of the uninterrupted run (the open batch, the batch awaiting expiry,
    each key's startTime / endTime / lastCurrentEventTime, RESET epochs)."""
    select = ["i", "g", "sum(v) as s", "count() as c"]
    d = make_stream(T=8, seed=12, nkeys=7 if part else 1)
    app = app_text("et, 8, st", select, "all events", group=True, part=part)
    want = model_chunks(spec_of(8, select, "all events", True, part, ("attr", 5)), d)
    assert_same(device_chunks(app, d, snapshot_after=1), want)


@pytest.mark.parametrize("case", RUN_CASES, ids=[short(c) for c in RUN_CASES])
def test_reference_known_answers(hip_available, case):
    from siddhi_amd.hip_engine import HipQueryEngine
    col = run_case(case, HipQueryEngine)
    errs = check_case(case, col) + check_extras(case, col)
    assert not errs, "%s (%s): %s" % (case["name"], case["source"], errs)


@pytest.mark.parametrize("case", FAIL_CASES, ids=[short(c) for c in FAIL_CASES])
def test_reference_creation_failures(hip_available, case):
    from siddhi_amd.hip_engine import HipQueryEngine
    from siddhi_amd.planner import SiddhiAppCreationException
    with pytest.raises(SiddhiAppCreationException):
        run_case(case, HipQueryEngine)
