"""Per-event Python model of the aggregator executors stdDev, distinctCount,
and, or, on the window / partition / selector model of tests/minmax_model.py
(imported, not copied: its windows and selector batching are the ones pinned to
the CPU oracle).  The yardstick of tests/test_aggregators.py and
tests/test_gpu_aggregators.py; the CPU oracle does not know these aggregators.

Written from the reference (C = modules/siddhi-core/src/main/java/io/siddhi/core):

  C/query/selector/attribute/aggregator/StdDevAttributeAggregatorExecutor.java:81-107 (init),
    :115-133 (null argument -> currentValue), :157-231 (AggregatorState)
  C/query/selector/attribute/aggregator/DistinctCountAttributeAggregatorExecutor.java:88-102 (init),
    :105-143 (processAdd / processRemove / reset), :146-170 (state)
  C/query/selector/attribute/aggregator/AndAttributeAggregatorExecutor.java:83-96, :98-151
  C/query/selector/attribute/aggregator/OrAttributeAggregatorExecutor.java (the same text, its
    computeLogicalOperation is trueEventsCount > 0)

Values as in minmax_model: FLOAT is numpy.float32 (widened with float()), None
is null.  Python floats are IEEE doubles and +, -, *, / and math.sqrt are
correctly rounded, as Java's double arithmetic and Math.sqrt are.

Differences from the reference, on purpose:
  * and / or unbox a null argument and fail the call (NullPointerException);
    here a null argument leaves the counters alone and returns the current result;
  * distinctCount's remove of a key that is not in the map throws
    (`preVal--` on null); no supported plan reaches it, here it is a no-op.
"""
import math
import struct

import numpy as np

import minmax_model as mm
from minmax_model import CURRENT, EXPIRED, T_DOUBLE, T_FLOAT, T_INT, T_LONG, T_STRING, Spec, norm, norm_chunks  # noqa: F401

T_BOOL = 5


class StdDevState:
    """StdDevAttributeAggregatorExecutor.AggregatorState (:148-232)."""

    def __init__(self, t=T_DOUBLE):
        self.mean = self.std = self.sum = 0.0     # :150
        self.count = 0                            # :151

    def add(self, v):                             # processAdd :157-173
        v = float(v)                              # (double) of the unboxed value :237-300
        self.count += 1
        if self.count == 0:
            return None
        if self.count == 1:
            self.sum = self.mean = v
            self.std = 0.0
            return 0.0
        old_mean = self.mean
        self.sum += v
        self.mean = self.sum / self.count
        self.std += (v - old_mean) * (v - self.mean)
        return _sqrt(self.std / self.count)

    def remove(self, v):                          # processRemove :175-192
        v = float(v)
        self.count -= 1
        if self.count == 0:
            self.sum = self.mean = 0.0
            self.std = 0.0
            return None
        old_mean = self.mean
        self.sum -= v
        self.mean = self.sum / self.count
        self.std -= (v - old_mean) * (v - self.mean)
        if self.count == 1:
            return 0.0
        return _sqrt(self.std / self.count)

    def reset(self):                              # :194-199
        self.sum = self.mean = 0.0
        self.std = 0.0
        self.count = 0
        return None

    def current(self):                            # currentValue :224-231
        if self.count == 0:
            return None
        if self.count == 1:
            return 0.0
        return _sqrt(self.std / self.count)


def _sqrt(x):
    """Math.sqrt: NaN for a negative argument (and for NaN), -0.0 for -0.0."""
    if x != x or x < 0.0:
        return float("nan")
    return math.sqrt(x)


def key_of(t, v):
    """What HashMap compares: equals() of the boxed value.  Integer / Long by
    value, Float / Double by floatToIntBits / doubleToLongBits (every NaN one
    key, 0.0 and -0.0 two), String and Boolean by value; null is a key."""
    if v is None:
        return None
    if t in (T_FLOAT, T_DOUBLE):
        if v != v:
            return "nan"
        return struct.pack("<f" if t == T_FLOAT else "<d", v)
    if t == T_BOOL:
        return bool(v)
    return v if t == T_STRING else int(v)


class DistinctCountState:
    """DistinctCountAttributeAggregatorExecutor (:105-170)."""

    def __init__(self, t):
        self.t = t
        self.values = {}                          # :148

    def add(self, v):                             # processAdd :105-113
        k = key_of(self.t, v)
        self.values[k] = self.values.get(k, 0) + 1
        return len(self.values)

    def remove(self, v):                          # processRemove :122-131
        k = key_of(self.t, v)
        pre = self.values.get(k)
        if pre is None:
            return len(self.values)               # the reference throws here (see the module text)
        if pre - 1 > 0:
            self.values[k] = pre - 1
        else:
            del self.values[k]
        return len(self.values)

    def reset(self):                              # :140-143
        self.values.clear()
        return 0

    def current(self):
        return len(self.values)


class BoolState:
    """{And,Or}AttributeAggregatorExecutor (:98-176)."""

    def __init__(self, is_and):
        self.is_and = is_and
        self.true = self.false = 0                # :155-156

    def add(self, v):                             # processAdd :99-106
        if v:
            self.true += 1
        else:
            self.false += 1
        return self.current()

    def remove(self, v):                          # processRemove :121-128
        if v:
            self.true -= 1
        else:
            self.false -= 1
        return self.current()

    def reset(self):                              # :147-151
        self.true = self.false = 0
        return False

    def current(self):                            # computeLogicalOperation :142-144
        return (self.true > 0 and self.false == 0) if self.is_and else self.true > 0


def new_state(kind, t, track):
    if kind == "stdDev":
        return StdDevState(t)
    if kind == "distinctCount":
        return DistinctCountState(t)
    if kind in ("and", "or"):
        return BoolState(kind == "and")
    return mm.new_state(kind, t, track)


def step(kind, state, etype, v):
    """AttributeAggregatorExecutor.processAttribute (:85-95) with each executor's
    null rule: stdDev returns currentValue() (:115-133); distinctCount passes null
    on as a key; and / or (see the module text) leave the state alone."""
    if kind == "distinctCount":
        return state.add(v) if etype == CURRENT else state.remove(v)
    if kind in ("stdDev", "and", "or"):
        if v is None:
            return state.current()
        return state.add(v) if etype == CURRENT else state.remove(v)
    return mm.step(kind, state, etype, v)


class Model(mm.Model):
    """minmax_model.Model with this module's state table and step: the windows,
    the partition's runs and the selector's per-chunk pick are its own."""

    def _select(self, pkey, chunk):
        s = self.spec
        groups = self.states.setdefault(pkey, {})
        picked = {}
        last = None
        for ev in chunk:
            if ev == "RESET":
                for sts in groups.values():
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
