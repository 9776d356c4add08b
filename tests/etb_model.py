"""Plain-Python, per-event restatement of the reference's externalTimeBatch
window without a timeout, and of the batch selector behind it.

Window: C/query/processor/stream/window/ExternalTimeBatchWindowProcessor.java
  process :238-311, initTiming :313-334, flushToOutputChunk :336-383,
  findEndTime :440-444, cloneAppend :446-456, WindowState :495-517.
Selector: C/query/selector/QuerySelector.java :271-313 (processInBatchNoGroupBy),
  :315-373 (processInBatchGroupBy), restated the way oracle.cpp
  selector_process does: a chunk emits its last selected event (aggregators,
  no group by), one event per group in first-seen order with the group's last
  values (group by), or every selected event (no aggregators).
Partitions: C/partition/PartitionStreamReceiver.java :175-216 -- a call's
  consecutive events of one key are one chunk of that key's instance.

Selector subset: attribute references, count(), sum(a), avg(a), group-by
attributes, current / expired / all events.  No nulls.
"""
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

CURRENT, EXPIRED, RESET = "CURRENT", "EXPIRED", "RESET"


def java_rem(a: int, b: int) -> int:
    """Java's (and C's) truncating %: the sign of the dividend."""
    r = abs(a) % abs(b)
    return -r if a < 0 else r


def find_end_time(cur: int, start: int, t: int) -> int:
    """findEndTime :440-444."""
    return cur + (t - java_rem(cur - start, t))


@dataclass
class Spec:
    ts_attr: int                       # index of the LONG timestamp attribute
    T: int
    start_mode: str = "none"           # none | const | attr
    start_value: int = 0               # the constant, or the attribute's index
    replace: bool = False              # replaceTimestampWithBatchEndTime
    outputs: List[Tuple] = field(default_factory=list)   # ("attr", i) | ("count",) | ("sum", i) | ("avg", i)
    group_by: List[int] = field(default_factory=list)
    events: str = "current"            # current | expired | all
    partition_attr: Optional[int] = None


class _Ev:
    __slots__ = ("type", "ts", "data")

    def __init__(self, type_, ts, data):
        self.type, self.ts, self.data = type_, ts, list(data)

    def clone(self):
        return _Ev(self.type, self.ts, self.data)


class _Window:
    """WindowState + process for one partition key."""

    def __init__(self, spec: Spec):
        self.s = spec
        self.expects_expired = spec.events in ("expired", "all")
        self.start = spec.start_value if spec.start_mode == "const" else 0
        self.end = -1
        self.last = 0                  # lastCurrentEventTime
        self.cur: List[_Ev] = []
        self.exp: Optional[List[_Ev]] = [] if self.expects_expired else None
        self.reset: Optional[_Ev] = None
        self.trigger_log: List[int] = []   # ordinals (per key) of the events that found ts >= endTime
        self.seen = 0

    def _init_timing(self, first: _Ev):
        s = self.s
        if self.end < 0:
            ts = first.data[s.ts_attr]
            if s.start_mode == "const":
                self.end = find_end_time(ts, self.start, s.T)
            elif s.start_mode == "attr":
                self.start = first.data[s.start_value]
                self.end = self.start + s.T
            else:
                self.start = ts
                self.end = self.start + s.T

    def _clone_append(self, ev: _Ev):
        c = ev.clone()
        if self.s.replace:
            c.data[self.s.ts_attr] = self.end
        self.cur.append(c)
        if self.reset is None:
            self.reset = _Ev(RESET, ev.ts, ev.data)

    def _flush(self, chunks, current_time):
        out: List[_Ev] = []
        if self.expects_expired and self.exp:
            for e in self.exp:
                e.ts = current_time
            out.extend(self.exp)
        if self.exp is not None:
            self.exp = []
        if self.cur:
            self.reset.ts = current_time
            out.append(self.reset)
            self.reset = None
            if self.exp is not None:
                for e in self.cur:
                    x = e.clone()
                    x.type = EXPIRED
                    self.exp.append(x)
            out.extend(self.cur)
        self.cur = []
        if out:
            chunks.append(out)

    def process(self, chunk: List[_Ev]) -> List[List[_Ev]]:
        if not chunk:
            return []
        chunks: List[List[_Ev]] = []
        self._init_timing(chunk[0])
        for ev in chunk:
            ts = ev.data[self.s.ts_attr]
            if self.last < ts:
                self.last = ts
            if ts < self.end:
                self._clone_append(ev)
            else:
                self.trigger_log.append(self.seen)
                self._flush(chunks, self.last)
                self.end = find_end_time(self.last, self.start, self.s.T)
                self._clone_append(ev)
            self.seen += 1
        return chunks


class _Selector:
    """One partition instance's selector: aggregator states per group key."""

    def __init__(self, spec: Spec):
        self.s = spec
        self.groups = {}
        self.has_agg = any(o[0] != "attr" for o in spec.outputs)

    def _values(self, ev: _Ev):
        s = self.s
        gk = tuple(ev.data[g] for g in s.group_by)
        st = self.groups.setdefault(gk, [[0, 0] for _ in s.outputs])   # [sum, count] per output
        vals = []
        for o, a in zip(s.outputs, st):
            if o[0] == "attr":
                vals.append(ev.data[o[1]])
                continue
            add = ev.type == CURRENT
            if o[0] == "count":
                a[1] += 1 if add else -1
                vals.append(a[1])
                continue
            x = ev.data[o[1]]
            if o[0] == "avg":
                x = float(x)
            a[0] = a[0] + x if add else a[0] - x
            a[1] += 1 if add else -1
            if a[1] == 0:
                vals.append(None)
            else:
                vals.append(a[0] / a[1] if o[0] == "avg" else a[0])
        return gk, vals

    def process(self, chunk: List[_Ev]):
        s = self.s
        rows, order, by_group, last = [], [], {}, None
        for ev in chunk:
            if ev.type == RESET:
                self.groups.clear()
                continue
            gk, vals = self._values(ev)
            on = (ev.type == CURRENT and s.events in ("current", "all")) or \
                 (ev.type == EXPIRED and s.events in ("expired", "all"))
            if not on:
                continue
            row = (ev.type, ev.ts, vals)
            if s.group_by:
                if gk not in by_group:
                    order.append(gk)
                by_group[gk] = row
            elif self.has_agg:
                last = row
            else:
                rows.append(row)
        if s.group_by:
            return [by_group[g] for g in order]
        if self.has_agg:
            return [last] if last is not None else []
        return rows


class Model:
    """run(calls) -> chunks; a call is a list of (timestamp, data) events, a
    chunk a list of (type, timestamp, values).  State persists across run()s."""

    def __init__(self, spec: Spec):
        self.s = spec
        self.inst = {}

    def _instance(self, key):
        if key not in self.inst:
            self.inst[key] = (_Window(self.s), _Selector(self.s))
        return self.inst[key]

    def run(self, calls):
        out = []
        for call in calls:
            runs = []
            for ts, data in call:
                key = data[self.s.partition_attr] if self.s.partition_attr is not None else None
                if runs and runs[-1][0] == key:
                    runs[-1][1].append(_Ev(CURRENT, ts, data))
                else:
                    runs.append((key, [_Ev(CURRENT, ts, data)]))
            for key, evs in runs:
                w, sel = self._instance(key)
                for chunk in w.process(evs):
                    rows = sel.process(chunk)
                    if rows:
                        out.append(rows)
        return out

    def triggers(self, key=None):
        return list(self._instance(key)[0].trigger_log)
