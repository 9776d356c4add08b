"""Per-event Python model of a single-stream aggregating query: the windows
none / length / lengthBatch / externalTime (and time, on a stepped clock), an
optional partition, `group by`, the selector's per-chunk batching, current /
expired / all output and the aggregator executors min, max, minForever,
maxForever (plus sum, avg and count, which tie the model to the CPU oracle).

Test infrastructure: the yardstick of tests/test_minmax.py (where its window
and selector are compared with the oracle, which does not know min / max) and
tests/test_gpu_minmax.py.  Nothing here imports the library; every part is
written from the reference (C = modules/siddhi-core/src/main/java/io/siddhi/core):

  C/query/selector/attribute/aggregator/MaxAttributeAggregatorExecutor.java:84-150,
    state classes :152-454; MinAttributeAggregatorExecutor.java (the same text, > for <)
  C/query/selector/attribute/aggregator/MaxForeverAttributeAggregatorExecutor.java:119-200,
    MinForeverAttributeAggregatorExecutor.java
  C/query/selector/attribute/aggregator/AttributeAggregatorExecutor.java:66-151
  C/query/selector/attribute/aggregator/{Sum,Avg,Count}AttributeAggregatorExecutor.java
  C/query/selector/QuerySelector.java:271-313 (processInBatchNoGroupBy), :315-373 (processInBatchGroupBy)
  C/query/processor/stream/window/LengthWindowProcessor.java:105-142
  C/query/processor/stream/window/LengthBatchWindowProcessor.java:206-243 (processFullBatchEvents)
  C/query/processor/stream/window/ExternalTimeWindowProcessor.java:124-158
  C/query/processor/stream/window/TimeWindowProcessor.java:132-169
  C/query/processor/stream/window/SlidingWindowProcessor.java:90, BatchingWindowProcessor.java:95
  C/partition/PartitionStreamReceiver.java:175-216 (same-key runs of a call are chunks)

Values: INT / LONG are Python ints, DOUBLE Python floats, FLOAT numpy float32
(compared as float, as Java compares the unboxed values); None is null.

RESET.  AttributeAggregatorExecutor.processReset (:145-151) takes the states
out of the holder and calls the executor's reset() on one of them.  The model
restates the executors' reset(): min / max clear value and deque (Max...State
.reset :196-202), the Forever kinds return their value and keep it
(MaxForever...State.reset :177-179), sum / avg / count start over.
"""
import struct

import numpy as np

CURRENT, EXPIRED = 0, 1
T_STRING, T_INT, T_LONG, T_FLOAT, T_DOUBLE = 0, 1, 2, 3, 4


# ---------------------------------------------------------------- executors
def _equals(t, a, b):
    """equals() of the boxed values: Integer / Long by value, Float / Double by
    floatToIntBits / doubleToLongBits -- NaN equals NaN, 0.0 does not equal -0.0."""
    if t in (T_INT, T_LONG):
        return a == b
    if a != a or b != b:
        return a != a and b != b
    fmt = "<f" if t == T_FLOAT else "<d"
    return struct.pack(fmt, a) == struct.pack(fmt, b)


class MaxState:
    """MaxAttributeAggregatorExecutor.MaxAttributeAggregatorState{Double,Float,Int,Long}
    (:152-454: four copies of one text); is_max False: MinAttributeAggregatorExecutor's."""

    def __init__(self, t, track, is_max=True):
        self.t = t
        self.deque = [] if track else None        # :157-161
        self.value = None
        self.below = (lambda a, b: a < b) if is_max else (lambda a, b: a > b)

    def add(self, v):                             # processAdd :164-180
        if self.deque is not None:
            while self.deque and self.below(self.deque[-1], v):   # descendingIterator, remove while < value
                self.deque.pop()
            self.deque.append(v)                  # addLast
        if self.value is None or self.below(self.value, v):
            self.value = v
        return self.value

    def remove(self, v):                          # processRemove :183-193
        if self.deque is not None:
            for i, x in enumerate(self.deque):    # removeFirstOccurrence
                if _equals(self.t, x, v):
                    del self.deque[i]
                    break
            self.value = self.deque[0] if self.deque else None   # peekFirst
        elif self.value is not None and _equals(self.t, self.value, v):
            self.value = None
        return self.value

    def reset(self):                              # :196-202
        if self.deque is not None:
            self.deque.clear()
        self.value = None

    def current(self):
        return self.value


class MaxForeverState:
    """MaxForeverAttributeAggregatorExecutor.MaxForeverAttributeAggregatorState* (:154-352)."""

    def __init__(self, t, track, is_max=True):
        self.value = None
        self.below = (lambda a, b: a < b) if is_max else (lambda a, b: a > b)

    def add(self, v):                             # :159-165
        if self.value is None or self.below(self.value, v):
            self.value = v
        return self.value

    remove = add                                  # :168-174: the same fold

    def reset(self):                              # :177-179: returns maxValue, keeps it
        return self.value

    def current(self):
        return self.value


class SumState:
    """SumAttributeAggregatorExecutor: double sums for FLOAT / DOUBLE, long for INT / LONG
    (values in these tests stay far inside the exact range of both)."""

    def __init__(self, t, track, is_max=True):
        self.int = t in (T_INT, T_LONG)
        self.sum = 0 if self.int else 0.0
        self.count = 0

    def add(self, v):
        self.count += 1
        self.sum += int(v) if self.int else float(v)
        return self.sum

    def remove(self, v):
        self.count -= 1
        self.sum -= int(v) if self.int else float(v)
        return self.current()

    def reset(self):
        self.sum = 0 if self.int else 0.0
        self.count = 0

    def current(self):
        return self.sum if self.count != 0 else None


class AvgState(SumState):
    """AvgAttributeAggregatorExecutor: a double sum over a count."""

    def __init__(self, t, track, is_max=True):
        self.int = False
        self.sum = 0.0
        self.count = 0

    def add(self, v):
        SumState.add(self, v)
        return self.current()

    def current(self):
        return self.sum / self.count if self.count != 0 else None


class CountState:
    def __init__(self, t, track, is_max=True):
        self.count = 0

    def add(self, v):
        self.count += 1
        return self.count

    def remove(self, v):
        self.count -= 1
        return self.count

    def reset(self):
        self.count = 0

    def current(self):
        return self.count


KINDS = {"max": (MaxState, True), "min": (MaxState, False), "maxForever": (MaxForeverState, True),
         "minForever": (MaxForeverState, False), "sum": (SumState, True), "avg": (AvgState, True),
         "count": (CountState, True)}


def new_state(kind, t, track):
    cls, is_max = KINDS[kind]
    return cls(t, track, is_max)


def agg_type(kind, t):
    """The aggregator's return type: min / max keep the argument's (getReturnType :115-117)."""
    if kind == "count":
        return T_LONG
    if kind == "avg":
        return T_DOUBLE
    if kind == "sum":
        return T_LONG if t in (T_INT, T_LONG) else T_DOUBLE
    return t


def step(kind, state, etype, v):
    """AttributeAggregatorExecutor.processAttribute (:85-95) with the executors'
    null rule ({Max,MaxForever}...processAdd / processRemove :120-139: a null
    argument returns the current value); count() counts every event."""
    if kind == "count":
        return state.add(v) if etype == CURRENT else state.remove(v)
    if v is None:
        return state.current()
    return state.add(v) if etype == CURRENT else state.remove(v)


# ---------------------------------------------------------------- the query
class Spec:
    """window: None, ("length", L), ("lengthBatch", L), ("externalTime", attr, T) or ("time", T);
    partition / group: an attribute index or None; aggs: [(kind, attr or None, type)];
    outputs: [("attr", i) | ("agg", k) | ("fn", f(data, aggs))]; having: f(data, aggs) or None;
    events: "current" | "expired" | "all"; where: f(data) or None (a filter before the window)."""

    def __init__(self, window, aggs, outputs, events="current", group=None, partition=None, having=None, where=None):
        self.window, self.aggs, self.outputs, self.events = window, aggs, outputs, events
        self.group, self.partition, self.having, self.where = group, partition, having, where
        # MaxAttributeAggregatorExecutor.init :93-96: SLIDE windows (SlidingWindowProcessor.java:90;
        # length, time, externalTime) or an output that expects EXPIRED events
        self.track = (window is not None and window[0] in ("length", "time", "externalTime")) or events != "current"


class _Window:
    """One window instance (one per partition key): process(events, now) -> chunks,
    each a list of (type, timestamp, data) with "RESET" entries."""

    def __init__(self, spec):
        self.w = spec.window
        self.expired_out = spec.events != "current"
        self.q = []          # the window's expired-event queue / the open batch
        self.prev = []       # lengthBatch: the batch awaiting its expiry

    def process(self, events, now):
        w = self.w
        if w is None:
            return [[(CURRENT, ts, d) for ts, d in events]]
        out = []
        if w[0] == "length":                      # LengthWindowProcessor.java:105-142
            for ts, d in events:
                if len(self.q) >= w[1]:
                    ots, od = self.q.pop(0)
                    out.append((EXPIRED, now, od))   # expired.setTimestamp(currentTime), before the current event
                self.q.append((ts, d))
                out.append((CURRENT, ts, d))
            return [out]
        if w[0] == "externalTime":                # ExternalTimeWindowProcessor.java:124-158
            for ts, d in events:
                t = d[w[1]]
                while self.q and self.q[0][1][w[1]] + w[2] <= t:
                    ots, od = self.q.pop(0)
                    out.append((EXPIRED, t, od))
                self.q.append((ts, d))
                out.append((CURRENT, ts, d))
            return [out]
        if w[0] == "time":                        # TimeWindowProcessor.java:132-169
            for ts, d in events:
                out.extend(self._time_expire(now))
                self.q.append((ts, d))
                out.append((CURRENT, ts, d))
            return [out]
        assert w[0] == "lengthBatch"              # LengthBatchWindowProcessor.java:206-243
        chunks = []
        for ts, d in events:
            self.q.append((ts, d))
            if len(self.q) == w[1]:
                c = []
                if self.expired_out:              # expiredEventQueue exists only when the output expects it
                    c.extend((EXPIRED, now, od) for ots, od in self.prev)
                    self.prev = self.q
                c.append("RESET")
                c.extend((CURRENT, ots, od) for ots, od in self.q)
                self.q = []
                chunks.append(c)
        return chunks

    def _time_expire(self, now):
        out = []
        while self.q and self.q[0][0] + self.w[1] <= now:
            ots, od = self.q.pop(0)
            out.append((EXPIRED, now, od))
        return out

    def timer(self, now):
        """A Scheduler TIMER at `now` (time windows): the due events expire in a chunk of their own."""
        c = self._time_expire(now)
        return [c] if c else []

    def next_due(self):
        return self.q[0][0] + self.w[1] if self.w and self.w[0] == "time" and self.q else None


class Model:
    def __init__(self, spec):
        self.spec = spec
        self.windows = {}     # partition key -> _Window
        self.states = {}      # partition key -> {group key -> [state per aggregator]}

    # -- selector: one chunk in, at most one callback chunk out
    def _select(self, pkey, chunk):
        s = self.spec
        groups = self.states.setdefault(pkey, {})
        picked = {}           # processInBatchGroupBy's LinkedHashMap: first put fixes the place, last the row
        last = None           # processInBatchNoGroupBy's lastEvent
        for ev in chunk:
            if ev == "RESET":
                for sts in groups.values():       # every group state of this partition key
                    for st in sts:
                        st.reset()
                continue
            etype, ts, d = ev
            gk = d[s.group] if s.group is not None else None
            sts = groups.get(gk)
            if sts is None:
                sts = groups[gk] = [new_state(k, t, s.track) for k, a, t in s.aggs]
            vals = [step(k, st, etype, None if a is None else d[a]) for (k, a, t), st in zip(s.aggs, sts)]
            if s.having is not None and not s.having(d, vals):
                continue
            on = (etype == CURRENT and s.events in ("current", "all")) or \
                 (etype == EXPIRED and s.events in ("expired", "all"))
            if not on:
                continue
            row = (etype, ts, [d[o[1]] if o[0] == "attr" else vals[o[1]] if o[0] == "agg" else o[1](d, vals)
                               for o in s.outputs])
            if s.group is not None:
                picked[gk] = row
            else:
                last = row
        if s.group is not None:
            return list(picked.values())
        return [last] if last is not None else []

    def _window(self, pkey):
        w = self.windows.get(pkey)
        if w is None:
            w = self.windows[pkey] = _Window(self.spec)
        return w

    def run(self, calls):
        """calls: the InputHandler calls, each a list of (timestamp, data); the
        playback clock of a call is its last event's timestamp.  Returns the
        callback chunks: lists of (type, timestamp, values)."""
        s = self.spec
        out = []
        for call in calls:
            if not call:
                continue
            now = call[-1][0]
            evs = [e for e in call if s.where is None or s.where(e[1])]
            runs = []
            if s.partition is None:
                runs = [(None, evs)] if evs else []
            else:
                for e in evs:                     # same-key runs of the call
                    k = e[1][s.partition]
                    if runs and runs[-1][0] == k:
                        runs[-1][1].append(e)
                    else:
                        runs.append((k, [e]))
            for k, run in runs:
                for chunk in self._window(k).process(run, now):
                    rows = self._select(k, chunk)
                    if rows:
                        out.append(rows)
        return out

    def advance(self, now):
        """Wall-clock time passes to `now` (time windows, unpartitioned): every
        due notify time fires one TIMER chunk (Scheduler.java:113-209)."""
        out = []
        w = self._window(None)
        while True:
            due = w.next_due()
            if due is None or due > now:
                break
            for chunk in w.timer(due):
                rows = self._select(None, chunk)
                if rows:
                    out.append(rows)
        return out


# ---------------------------------------------------------------- comparison form
def norm(v):
    """A value as something == compares bit for bit: floats by their hex form
    (0.0 and -0.0 differ, every NaN is 'nan')."""
    if isinstance(v, (float, np.floating)):
        return float(v).hex()
    if isinstance(v, (np.integer,)):
        return int(v)
    return v


def norm_chunks(chunks):
    """Model chunks as ([(ts, values)] current, [(ts, values)] expired) per callback."""
    return [([(ts, [norm(x) for x in vals]) for t, ts, vals in c if t == CURRENT],
             [(ts, [norm(x) for x in vals]) for t, ts, vals in c if t == EXPIRED]) for c in chunks]
