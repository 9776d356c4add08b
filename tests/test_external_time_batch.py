"""externalTimeBatch on the CPU: the Python model (tests/etb_model.py) against
the reference's own known answers, the closed-form trigger rule the device
uses against the model's sequential one, and the planner's lowering and
validation (ExternalTimeBatchWindowProcessor.java:153-227, 238-311, 440-444;
include/siddhi_ir.h shd_window EXTERNAL_TIME_BATCH).
"""
import json
import os

import numpy as np
import pytest

import etb_model as em
from kat_runner import Collector, _py, check_case
from parity import compile_single_query
from siddhi_amd import planner as pl
from siddhi_amd import runtime as rt

KAT_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kat_external_time_batch",
                        "ExternalTimeBatchWindowTestCase.json")
with open(KAT_FILE) as _fp:
    CASES = json.load(_fp)
RUN_CASES = [c for c in CASES if "expected_exception" not in c]
FAIL_CASES = [c for c in CASES if "expected_exception" in c]

# the model's spec of each transcribed app (attribute indices of its stream)
_LOGIN_OUT = [("attr", 0), ("attr", 1), ("count",)]
SPECS = {
    "test02NoMsg": em.Spec(1, 10000, outputs=[("avg", 0), ("count",)]),
    "test05EdgeCase": em.Spec(1, 10000, outputs=[("avg", 0), ("count",)]),
    "test01DownSampling": em.Spec(4, 10000, outputs=[("avg", 0), ("avg", 1), ("avg", 2), ("avg", 3), ("attr", 4),
                                                      ("count",)]),
    "test1": em.Spec(0, 5000, outputs=[("attr", 1)]),
    "test2": em.Spec(0, 5000, "const", 1200, outputs=[("attr", 1)]),
    "externalTimeBatchWindowTest2": em.Spec(0, 1000, outputs=_LOGIN_OUT, events="all"),
    "externalTimeBatchWindowTest3": em.Spec(0, 1000, outputs=_LOGIN_OUT, events="all"),
    "externalTimeBatchWindowTest11": em.Spec(0, 1000, "const", 0, outputs=_LOGIN_OUT),
    "externalTimeBatchWindowTest14": em.Spec(0, 1000, "attr", 0, outputs=_LOGIN_OUT, events="all"),
}


def short(case):
    return case["name"].split(".", 1)[1]


def model_collector(case):
    """The case's sends through the model, as the callbacks kat_runner collects."""
    spec = SPECS[short(case)]
    calls = [[(s["ts"], [_py(v)[1] for v in s["data"]])] for s in case["sends"]]
    col = Collector()
    for chunk in em.Model(spec).run(calls):
        cur = [rt.Event(ts, vals) for t, ts, vals in chunk if t == em.CURRENT]
        exp = [rt.Event(ts, vals) for t, ts, vals in chunk if t == em.EXPIRED]
        col.chunks.append((cur, exp))
        col.in_events.extend(cur)
        col.remove_events.extend(exp)
    return col


def check_extras(case, col):
    """The two fields this directory adds to kat_runner's format."""
    errs = []
    if case.get("expected_chunks") is not None and len(col.chunks) != case["expected_chunks"]:
        errs.append("%d callbacks, expected %d" % (len(col.chunks), case["expected_chunks"]))
    return errs


def test_every_transcribed_case_has_a_spec():
    assert sorted(SPECS) == sorted(short(c) for c in RUN_CASES)
    assert len(RUN_CASES) == 9 and len(FAIL_CASES) == 8


@pytest.mark.parametrize("case", RUN_CASES, ids=[short(c) for c in RUN_CASES])
def test_model_reproduces_reference_known_answer(case):
    """Validates the model, not the feature."""
    col = model_collector(case)
    errs = check_case(case, col) + check_extras(case, col)
    assert not errs, "%s (%s): %s" % (case["name"], case["source"], errs)


# ---------------------------------------------------------------- trigger rule
def closed_form_triggers(ts, T, mode, start_value):
    """The rule engine_window.hip uses, in NumPy.  M = inclusive prefix maximum
    of ts seeded with 0 (lastCurrentEventTime's initial value).  The key's
    first event fixes startTime / endTime and never emits.  While the maximum
    of the earlier events is below startTime the events are walked one by one
    (k_etb_lane); from the first event i with M[i-1] >= startTime on, event i
    triggers iff ts[i] >= findEndTime(M[i-1], startTime, T) (k_etb_trig).
    Returns the indices of the triggers that flush."""
    ts = np.asarray(ts, np.int64)
    n = len(ts)
    M = np.maximum.accumulate(np.maximum(ts, 0))
    if mode == "const":
        start = start_value
        E = em.find_end_time(int(ts[0]), start, T)
    else:
        start = int(start_value[0]) if mode == "attr" else int(ts[0])
        E = start + T
    if ts[0] >= E:
        E = em.find_end_time(int(M[0]), start, T)   # flushes an empty batch: no chunk
    trig = []
    i = 1
    while i < n and M[i - 1] < start:
        if ts[i] >= E:
            trig.append(i)
            E = em.find_end_time(int(M[i]), start, T)
        i += 1
    if i < n:
        prev = M[i - 1:n - 1]
        assert (prev >= start).all()
        bnd = prev + (T - (prev - start) % T)
        trig.extend((i + np.nonzero(ts[i:] >= bnd)[0]).tolist())
    return trig


def random_stream(seed, n=300):
    """Timestamps with late events, values exactly on a boundary, gaps of many
    windows; every fifth stream has T = 1, every third a constant startTime
    above its first timestamps, every seventh an attribute startTime."""
    rng = np.random.default_rng(1000 + seed)
    T = 1 if seed % 5 == 0 else int(rng.choice([3, 10, 1000]))
    t0 = int(rng.integers(0, 5000))
    if seed % 3 == 0:
        mode, start = "const", t0 + int(rng.integers(1, 40)) * T + int(rng.integers(0, T))
    elif seed % 7 == 0:
        mode, start = "attr", None
    else:
        mode, start = ("const", int(rng.integers(0, t0 + 1))) if seed % 2 else ("none", None)
    ts, cur, stats = [t0], t0, {"late": 0, "boundary": 0, "gap": 0}
    sattr = [t0 + int(rng.integers(-3, 4)) * T]
    grid0 = start if mode == "const" else (sattr[0] if mode == "attr" else t0)
    for _ in range(n - 1):
        r = rng.random()
        if r < 0.15:                                   # late: below the running maximum
            t = max(0, cur - int(rng.integers(1, 3 * T + 2)))
            stats["late"] += t < cur
        elif r < 0.35:                                 # exactly on a boundary of the grid
            k = (cur - grid0) // T + int(rng.integers(1, 3))
            t = max(0, grid0 + k * T)
            stats["boundary"] += 1
        elif r < 0.45:                                 # a gap of many windows
            t = cur + int(rng.integers(5, 50)) * T + int(rng.integers(0, T))
            stats["gap"] += 1
        else:
            t = cur + int(rng.integers(0, max(2, T // 2 + 1)))
        ts.append(t)
        sattr.append(int(rng.integers(0, 10000)))      # read from the first event only
        cur = max(cur, t)
    return T, mode, start, ts, sattr, stats


def test_closed_form_trigger_rule_equals_sequential_model():
    total = {"late": 0, "boundary": 0, "gap": 0}
    negative = t1 = ntrig = 0
    for seed in range(200):
        T, mode, start, ts, sattr, stats = random_stream(seed)
        for k in total:
            total[k] += stats[k]
        spec = em.Spec(0, T, mode, 1 if mode == "attr" else (start or 0), outputs=[("attr", 0)])
        m = em.Model(spec)
        m.run([[(0, [t, s]) for t, s in zip(ts, sattr)]])
        want = [i for i in m.triggers() if i > 0]      # a first event's trigger finds an empty batch
        got = closed_form_triggers(ts, T, mode, sattr if mode == "attr" else start)
        assert got == want, (seed, T, mode, start)
        negative += mode == "const" and start > ts[0]
        t1 += T == 1
        ntrig += len(want)
    assert min(total.values()) > 200 and negative >= 60 and t1 == 40 and ntrig > 5000


def test_find_end_time_truncating_remainder():
    """A startTime after the event gives a negative remainder and an endTime
    more than T ahead (findEndTime :440-444 with Java's %)."""
    assert em.find_end_time(10000, 1200, 5000) == 11200
    assert em.find_end_time(5, 100, 10) == 20
    assert em.find_end_time(11, 100, 10) == 30
    assert em.find_end_time(100, 100, 10) == 110


# ---------------------------------------------------------------- planner
S = "define stream S (k string, v double, et long, st long, n int); "


def window_of(app):
    qp, _ = compile_single_query(app)
    h = [x for x in qp.plan.handlers if x[0] == pl.H_WINDOW]
    assert len(h) == 1
    return qp.plan, h[0]


def q(window, tail="select k, v insert into O;"):
    return S + "@info(name = 'q') from S#window.externalTimeBatch(%s) %s" % (window, tail)


def test_lowering_two_parameters():
    _, h = window_of(q("et, 1 sec"))
    assert h == (pl.H_WINDOW, 8, 1000, 2)
    assert pl.W_EXTERNAL_TIME_BATCH == 8 and pl.VERSION == 1


def test_lowering_constant_start():
    plan, h = window_of(q("et, 500, 1200"))
    kind, wk, p, qw = h
    assert (wk, p) == (8, 500)
    assert qw & 0xFFFF == 2 and (qw >> 16) & 3 == 1 and (qw >> 18) & 1 == 0
    assert plan.consts[(qw >> 24) & 0xFFFF] == 1200
    assert qw >> 40 == 0


def test_lowering_attribute_start():
    _, h = window_of(q("et, 500, st"))
    assert h[3] == 2 | (2 << 16) | (3 << 24)


def test_lowering_five_parameters():
    plan, h = window_of(q("et, 2 sec, 0, 0, true", "select k, et insert all events into O;"))
    qw = h[3]
    assert h[2] == 2000
    assert qw & 0xFFFF == 2 and (qw >> 16) & 3 == 1 and (qw >> 18) & 1 == 1
    assert plan.consts[(qw >> 24) & 0xFFFF] == 0
    assert pl.etb_pack(2, pl.ETB_START_CONST, (qw >> 24) & 0xFFFF, True) == qw


def test_partitioned_use_is_planned():
    app = S + "partition with (k of S) begin @info(name = 'q') from S#window.externalTimeBatch(et, 10) " \
              "select k, sum(v) as s insert into O; end;"
    qp, _ = compile_single_query(app)
    assert qp.partitioned and any(h[0] == pl.H_WINDOW and h[1] == 8 for h in qp.plan.handlers)


@pytest.mark.parametrize("window", [
    "n, 1 sec",              # timestamp is an int attribute
    "v, 1 sec",              # ... a double
    "'et', 1 sec",           # ... not an attribute
    "et, '1 sec'",           # windowTime is a string
    "et, n",                 # ... an attribute
    "et, 1.5",               # ... a double
    "et, 1 sec, 1.0",        # startTime is a double constant
    "et, 1 sec, n",          # ... an int attribute
    "et, 1 sec, 1/2",        # ... an expression
    "et, 1 sec, 0, 10.5",    # timeout is a double
    "et, 1 sec, 0, st",      # ... an attribute
    "et, 1 sec, 0, 0, 100",  # the fifth parameter is not a bool
    "et, 1 sec, 0, 100, 100",
    "et",                    # one parameter
    "et, 1 sec, 0, 0, true, 1",   # six
])
def test_validation_errors(window):
    with pytest.raises(pl.SiddhiAppValidationException):
        compile_single_query(q(window))


@pytest.mark.parametrize("window", ["et, 1 sec, 0, 100", "et, 1 sec, st, 6 sec", "et, 1 sec, 0, 1, true"])
def test_positive_timeout_is_refused(window):
    with pytest.raises(pl.UnsupportedPlanException, match="timeout"):
        compile_single_query(q(window))


def test_timeout_zero_is_planned():
    _, h = window_of(q("et, 1 sec, st, 0"))
    assert h[1] == 8


def test_filter_after_the_window_is_refused():
    app = S + "@info(name = 'q') from S#window.externalTimeBatch(et, 1 sec)[v > 1.0] select k insert into O;"
    with pytest.raises(pl.UnsupportedPlanException, match="filter after a batch window"):
        compile_single_query(app)


@pytest.mark.parametrize("case", FAIL_CASES, ids=[short(c) for c in FAIL_CASES])
def test_reference_creation_failures(case):
    assert case["expected_exception"] == "SiddhiAppCreationException"
    with pytest.raises(pl.SiddhiAppCreationException):
        compile_single_query(case["app"])


# Plan bytes of two queries as the commit before this window produced them:
# the handler record's layout and SHD_IR_VERSION are unchanged.
PARENT_PLAN_BYTES = {
    S + "@info(name = 'q') from S[v > 2.0]#window.lengthBatch(4) select k, sum(v) as s group by k "
        "insert all events into O;":
        "534844500100000002000000010000000500000000000000040000000200000002000000010000000100000000000000"
        "0000004005000000030000000300000000000000ffffffff01000400010000000000000004000000000000000d000000"
        "040000000000000000000000010000000300000000000000ffffffff00000000010000000300000000000000ffffffff"
        "010004000100000015000000000000000000000000000000010000000300000000000000ffffffff0000000000000000"
        "000000000200000001000000000000000200000003000000040000000000000000000000000000000100000001000000"
        "010000000100000002000000040000000100000004000000ffffffff0200000000000000010000000400000003000000"
        "0000000000000000",
    S + "@info(name = 'q') from S#window.externalTime(et, 1 sec) select k, v, count() as c insert into O;":
        "534844500100000002000000010000000500000000000000040000000200000002000000010000000000000003000000"
        "010000000300000000000000ffffffff00000000010000000300000000000000ffffffff010004000100000015000000"
        "0000000000000000000000000000000000000000010000000200000006000000e8030000000000000200000000000000"
        "01000000000000000100000003000000ffffffffffffffff00000000ffffffff03000000000000000000000004000000"
        "010000000200000002000000ffffffffffffffff",
}


@pytest.mark.parametrize("app", list(PARENT_PLAN_BYTES), ids=["lengthBatch", "externalTime"])
def test_existing_plan_bytes_unchanged(app):
    qp, _ = compile_single_query(app)
    assert qp.ir.hex() == PARENT_PLAN_BYTES[app]
