"""Shared by tests/test_join.py (CPU) and tests/test_gpu_join.py: the reference's
join known answers with their model specs, and generated two-stream workloads
in both the model's and the runtime's form."""
import json
import os

import numpy as np

import join_model as jm
from kat_runner import TICK_MS, Collector, _py
from siddhi_amd import runtime as rt

HERE = os.path.dirname(os.path.abspath(__file__))
KAT_DIR = os.path.join(HERE, "golden", "kat_join")

# the join kernels' tile numbers (engine_join.hip; test_join.py checks the text)
JOIN_TRIG = 256
JOIN_TILE = 64


def load_cases():
    cases = []
    for f in ("JoinTestCase.json", "OuterJoinTestCase.json"):
        with open(os.path.join(KAT_DIR, f)) as fp:
            cases.extend(json.load(fp))
    return cases


CASES = load_cases()
FAIL_CASES = [c for c in CASES if "expected_exception" in c]
REFUSED_CASES = [c for c in CASES if "not_run" in c]
# every case that runs somewhere: the model runs all of them, the library the ones it does not refuse
MODEL_CASES = [c for c in CASES if "expected_exception" not in c]
RUN_CASES = [c for c in MODEL_CASES if "not_run" not in c]


def short(case):
    return case["name"]


# ---- model specs of the transcribed apps: cse = [symbol, price, volume], twitter = [user, tweet, company]
def _a(side, i):
    return None if side is None else side[i]


def _sel3(l, r):
    return [_a(l, 0), _a(r, 1), _a(l, 1)]


def _sel4(l, r):
    return [_a(l, 0), _a(r, 1), _a(l, 1), _a(r, 2)]


def _sel2(l, r):
    return [_a(l, 0), _a(r, 1)]


def _sym(l, r):
    return l[0] == r[2]


def _time(t):
    return jm.Side(("time", t))


def _len(n):
    return jm.Side(("length", n))


SPECS = {
    "JoinTestCase.joinTest1": jm.Spec(_time(1000), _time(1000), _sel3, _sym, events="all"),
    "JoinTestCase.joinTest2": jm.Spec(_time(1000), _time(1000), _sel3, _sym, events="all"),
    "JoinTestCase.joinTest4": jm.Spec(_time(2000), _time(2000), _sel3, _sym, events="all"),
    "JoinTestCase.joinTest5": jm.Spec(_len(1), _len(1), _sel3, events="all"),
    "JoinTestCase.joinTest8": jm.Spec(_len(1), _len(1), _sel3, events="all"),
    "JoinTestCase.joinTest12": jm.Spec(_time(1000), _time(1000), lambda l, r: list(l) + list(r), _sym),
    "OuterJoinTestCase.joinTest1": jm.Spec(_len(3), _len(1), _sel3, _sym, "full_outer", "all"),
    "OuterJoinTestCase.joinTest2": jm.Spec(_len(1), _len(2), _sel4, _sym, "right_outer", "all"),
    "OuterJoinTestCase.joinTest3": jm.Spec(_len(2), _len(1), _sel4, _sym, "left_outer", "all"),
    "OuterJoinTestCase.joinTest6": jm.Spec(_len(2), jm.Side(None), _sel2, _sym, "right_outer", "all"),
    "OuterJoinTestCase.joinTest7": jm.Spec(jm.Side(None), _len(2), _sel2, _sym, "left_outer", "all"),
    "OuterJoinTestCase.joinTest8": jm.Spec(_len(3), _len(1), _sel3, _sym, "inner", "all"),
    "OuterJoinTestCase.joinTest9": jm.Spec(_len(3), _len(1), _sel3, _sym, "inner", "all"),
}


def chunks_to_collector(chunks):
    """Model chunks as the callbacks kat_runner collects."""
    col = Collector()
    for chunk in chunks:
        cur = [rt.Event(ts, vals) for t, ts, vals in chunk if t == jm.CURRENT]
        exp = [rt.Event(ts, vals, True) for t, ts, vals in chunk if t == jm.EXPIRED]
        col.chunks.append((cur, exp))
        col.in_events.extend(cur)
        col.remove_events.extend(exp)
    return col


def model_collector(case):
    """The case's steps through the model, the clock moved the way kat_runner
    moves the runtime's: to each send's timestamp, and in TICK_MS steps through
    a pause."""
    m = jm.Model(SPECS[short(case)])
    clock = case["start_time"]
    steps = []
    for s in case["sends"]:
        if "time" in s:
            while clock < s["time"]:
                clock = min(s["time"], clock + TICK_MS)
                steps.append(("time", clock))
            continue
        clock = max(clock, s["ts"])
        steps.append(("time", s["ts"]))
        steps.append((0 if s["stream"] == "cseEventStream" else 1, [(s["ts"], [_py(v)[1] for v in s["data"]])]))
    return chunks_to_collector(m.run(steps))


def check_extras(case, col):
    """The fields kat_runner.check_case does not know."""
    errs = []
    if case.get("expected_chunks") is not None and len(col.chunks) != case["expected_chunks"]:
        errs.append("%d callbacks, expected %d" % (len(col.chunks), case["expected_chunks"]))
    if case.get("expected_arrived") is not None and bool(col.chunks) != case["expected_arrived"]:
        errs.append("eventArrived %s, expected %s" % (bool(col.chunks), case["expected_arrived"]))
    return errs


def collector_rows(col):
    """Callbacks as comparable data: per callback (current rows, expired rows), a row (timestamp, values)."""
    def rows(evs):
        return [(e.getTimestamp(), list(e.getData())) for e in evs]
    return [(rows(c[0]), rows(c[1])) for c in col.chunks]


# ---------------------------------------------------------------- generated workloads
# A (k int, price float, id long) and B (k int, lim float, id long); a send is
# (side, [call, ...]), a call a list of (timestamp, [k, price, id]) events.
GEN_STREAMS = "define stream A (k int, price float, id long); define stream B (k int, lim float, id long); "
GEN_SELECT = "select a.k as ak, a.price as price, a.id as aid, b.k as bk, b.lim as lim, b.id as bid "


def gen_select(l, r):
    return [_a(l, 0), _a(l, 1), _a(l, 2), _a(r, 0), _a(r, 1), _a(r, 2)]


def gen_sends(plan, keys, seed=7, nulls=False):
    """plan: [(side, [call sizes])].  Keys from range(keys); prices in halves
    (exact in float32); timestamps mostly rise, sometimes repeat, now and then
    step back; with `nulls` about one key in sixteen is null."""
    rng = np.random.default_rng(seed)
    t, ident, out = 1000, 0, []
    for side, sizes in plan:
        calls = []
        for n in sizes:
            call = []
            for _ in range(n):
                step = int(rng.integers(0, 4))
                t += -2 if step == 0 and rng.integers(0, 8) == 0 else step
                k = int(rng.integers(0, keys))
                if nulls and rng.integers(0, 16) == 0:
                    k = None
                call.append((t, [k, float(rng.integers(0, 40)) / 2.0, ident]))
                ident += 1
            calls.append(call)
        out.append((side, calls))
    return out


def three_rounds():
    """About 3 000 events, two streams interleaved, in three rounds of sends
    with call sizes 1, 37 and 1024."""
    return ([(s, [1] * 8) for s in (0, 1, 0, 1)] + [(s, [37] * 5) for s in (0, 1, 1, 0)] +
            [(0, [1024]), (1, [1024])])


def model_run(spec, sends):
    """Every call of every send through the model -> comparable callbacks."""
    m = jm.Model(spec)
    steps = []
    for side, calls in sends:
        for call in calls:
            steps.append((side, call))
    return collector_rows(chunks_to_collector(m.run(steps)))


def to_batch(side, calls):
    """One send as the ColumnBatch InputHandler.send_batch takes."""
    evs = [e for call in calls for e in call]
    n = len(evs)
    ts = np.array([e[0] for e in evs], np.int64)
    knull = np.array([e[1][0] is None for e in evs], np.uint8)
    k = np.array([0 if e[1][0] is None else e[1][0] for e in evs], np.int32)
    price = np.array([e[1][1] for e in evs], np.float32)
    ident = np.array([e[1][2] for e in evs], np.int64)
    offs = np.cumsum([0] + [len(c) for c in calls]).astype(np.int64)
    return rt.ColumnBatch(ts, [k, price, ident], [knull if knull.any() else None, None, None], offs)
