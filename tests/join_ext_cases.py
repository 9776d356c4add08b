"""Shared by tests/test_join_external_time.py (CPU) and
tests/test_gpu_join_external_time.py: generated two-stream workloads whose
sides carry an event-time attribute, in the model's and the runtime's form, and
the shapes (app text + model spec) both files use."""
import numpy as np

import join_cases as jc
import join_ext_model as jx
from siddhi_amd import runtime as rt

# A (k int, price float, et long) and B (k int, lim float, et long); a send is
# (side, [call, ...]), a call a list of (timestamp, [k, price, et]) events.
STREAMS = "define stream A (k int, price float, et long); define stream B (k int, lim float, et long); "
SELECT = "select a.k as ak, a.price as price, a.et as aet, b.k as bk, b.lim as lim, b.et as bet "
ET = 2          # the time attribute's index on both sides
T = 1500        # the window time of every generated shape
SEED = 1        # with T, chosen for what tests/test_join_external_time.py asserts of the model's run
KEYS = 64


def select(l, r):
    a = lambda side, i: None if side is None else side[i]   # noqa: E731
    return [a(l, 0), a(l, 1), a(l, 2), a(r, 0), a(r, 1), a(r, 2)]


def gen_sends(plan=None, keys=KEYS, seed=SEED, nulls=False, t=T):
    """plan: [(side, [call sizes])], join_cases.three_rounds() by default.  The
    timestamps mostly rise; `et` (one sequence over both streams) mostly rises
    by 1 or 2, repeats about one time in four, steps back by 1 to 3 about one
    time in sixteen and jumps by more than T about one time in a thousand.
    With `nulls` about one key in sixteen and one `et` in thirty-two is null."""
    rng = np.random.default_rng(seed)
    ts, et, out = 1000, 5000, []
    for side, sizes in (plan or jc.three_rounds()):
        calls = []
        for n in sizes:
            call = []
            for _ in range(n):
                ts += int(rng.integers(0, 3))
                r = int(rng.integers(0, 1000))
                if r < 1:
                    et += t + int(rng.integers(1, 50))
                elif r < 64:
                    et -= int(rng.integers(1, 4))
                elif r >= 300:
                    et += int(rng.integers(1, 3))
                k = int(rng.integers(0, keys))
                e = et
                if nulls and rng.integers(0, 16) == 0:
                    k = None
                if nulls and rng.integers(0, 32) == 0:
                    e = None
                call.append((ts, [k, float(rng.integers(0, 40)) / 2.0, e]))
            calls.append(call)
        out.append((side, calls))
    return out


def model_run(spec, sends, count_blocked=False):
    """Every call of every send through the model -> (comparable callbacks,
    the model's stats; max_carried: the most items a side held after a send)."""
    m = jx.Model(spec, count_blocked)
    chunks, carried = [], 0
    for side, calls in sends:
        for call in calls:
            rows = m.send(side, call)
            if rows:
                chunks.append(rows)
        carried = max(carried, len(m.q[side]))
    stats = dict(m.stats, max_carried=carried)
    return jc.collector_rows(jc.chunks_to_collector(chunks)), stats


def to_batch(side, calls):
    """One send as the ColumnBatch InputHandler.send_batch takes."""
    evs = [e for call in calls for e in call]
    ts = np.array([e[0] for e in evs], np.int64)
    knull = np.array([e[1][0] is None for e in evs], np.uint8)
    enull = np.array([e[1][2] is None for e in evs], np.uint8)
    k = np.array([0 if e[1][0] is None else e[1][0] for e in evs], np.int32)
    price = np.array([e[1][1] for e in evs], np.float32)
    et = np.array([0 if e[1][2] is None else e[1][2] for e in evs], np.int64)
    offs = np.cumsum([0] + [len(c) for c in calls]).astype(np.int64)
    return rt.ColumnBatch(ts, [k, price, et], [knull if knull.any() else None, None, enull if enull.any() else None],
                          offs)


EVENTS = {"current": "", "all": "all events ", "expired": "expired events "}
WORDS = {"inner": "join", "left_outer": "left outer join", "right_outer": "right outer join",
         "full_outer": "full outer join"}
EXT = ("ext", T)


def _window_text(w):
    if w is None:
        return ""
    return "#window.externalTime(et, %d)" % w[1] if w[0] == "ext" else "#window.length(%d)" % w[1]


def _model_side(w, flt, uni):
    window = None if w is None else ("externalTime", ET, w[1]) if w[0] == "ext" else ("length", w[1])
    return jx.Side(window, flt and flt[1], uni)


def _side_text(stream, alias, w, flt, uni):
    return "%s%s%s as %s%s" % (stream, "[%s]" % flt[0] if flt else "", _window_text(w), alias,
                               " unidirectional" if uni else "")


def _eq(l, r):
    return l[0] is not None and l[0] == r[0]   # a.k == b.k (null -> false)


class Shape:
    """One generated case: the app's text and the model's spec from the same
    parameters.  wa / wb: ("ext", T), ("length", L) or None."""

    def __init__(self, name, wa=EXT, wb=EXT, kind="inner", on="a.k == b.k", on_fn=_eq, events="all", fa=None, fb=None,
                 uni=None, plan=None, nulls=False):
        self.name, self.plan, self.nulls = name, plan, nulls
        self.app = ("@app:playback " + STREAMS + "@info(name = 'q') from " + _side_text("A", "a", wa, fa, uni == 0) +
                    " " + WORDS[kind] + " " + _side_text("B", "b", wb, fb, uni == 1) + (" on " + on if on else "") +
                    " " + SELECT + "insert " + EVENTS[events] + "into O;")
        self.spec = jx.Spec(_model_side(wa, fa, uni == 0), _model_side(wb, fb, uni == 1), select,
                            on_fn if on else None, kind, events)

    def sends(self):
        return gen_sends(self.plan, nulls=self.nulls)
