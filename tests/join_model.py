"""Plain-Python, per-event restatement of the reference's stream-stream window
join, for the window kinds `length`, `time` and none.

Join: C/query/input/stream/join/JoinProcessor.java :79-190 (process, execute:
  TIMER skipped, find, outer rows, joinEventBuilder), C/util/parser/
  JoinInputStreamParser.java :200-225 (trigger flags), :334-352 (outer flags).
Windows: LengthWindowProcessor.java :105-158, TimeWindowProcessor.java :132-183,
  EmptyWindowProcessor.java :66-120 (a side without a window holds nothing).
Find: OperatorParser.constructOperator over an event queue -- the queue is
  walked from its oldest event, matches come out in that order.
Selector: QuerySelector.process(List<ComplexEventChunk>) -- drops the event
  types the output clause does not want; all rows of one window chunk (one
  send call or one timer firing) are one callback; no rows, no callback.

The rules as the library states them (DESIGN.md "Joins"):
* a side's window handles the whole call first, then every CURRENT and EXPIRED
  event of its chunk, in the window's order, looks the other side up -- unless
  the other side is `unidirectional`;
* the other side does not change during the call; its content is the last
  min(L, count) items (length), the items with ts + T > clock (time), nothing
  (no window);
* a row carries the trigger's type and timestamp and (left, right) order; a
  trigger without a match emits one row with the other side missing when its
  own side is the outer one;
* the clock of a call is the largest "last timestamp of a call" seen so far;
  EXPIRED events are stamped with it (length, none) or with the time they
  expired at (time, at a call or at a timer).

No library code is used.  Conditions and projections are Python callables over
(left, right), each a list of attribute values or None for a missing side.
"""
from dataclasses import dataclass
from typing import Callable, List, Optional, Tuple

CURRENT, EXPIRED = "CURRENT", "EXPIRED"


@dataclass
class Side:
    window: Optional[Tuple[str, int]] = None    # ("length", L) | ("time", T) | None
    filter: Optional[Callable] = None           # data -> bool
    unidirectional: bool = False


@dataclass
class Spec:
    left: Side
    right: Side
    select: Callable                            # (left, right) -> list of values
    on: Optional[Callable] = None               # (left, right) -> bool; None: constant true
    type: str = "inner"                         # inner | left_outer | right_outer | full_outer
    events: str = "current"                     # current | expired | all


class Model:
    """send(side, events) -> the call's callback chunk (or None); advance(now)
    -> the chunks of the timers that fire.  An event is (timestamp, data); a
    chunk is a list of (type, timestamp, values)."""

    def __init__(self, spec: Spec):
        self.s = spec
        self.sides = (spec.left, spec.right)
        self.q: List[List[Tuple[int, list]]] = [[], []]
        self.clock: Optional[int] = None
        self.outer = (spec.type in ("left_outer", "full_outer"), spec.type in ("right_outer", "full_outer"))

    # -- window content
    def _content(self, y: int):
        side = self.sides[y]
        if side.window is None:
            return []
        if side.window[0] == "time":
            # FIFO: the queue is popped from its head while the head has expired
            k = 0
            while k < len(self.q[y]) and self.q[y][k][0] + side.window[1] <= self.clock:
                k += 1
            return self.q[y][k:]
        return self.q[y]

    def _wanted(self, typ):
        return self.s.events == "all" or (self.s.events == "current") == (typ == CURRENT)

    def _join(self, x: int, chunk):
        """chunk: [(type, ts, data)] of side x, in the window's order."""
        if self.sides[1 - x].unidirectional:
            return []
        rows = []
        found_in = self._content(1 - x)
        for typ, ts, data in chunk:
            hits = 0
            for _, other in found_in:
                pair = (data, other) if x == 0 else (other, data)
                if self.s.on is None or self.s.on(*pair):
                    hits += 1
                    if self._wanted(typ):
                        rows.append((typ, ts, self.s.select(*pair)))
            if hits == 0 and self.outer[x] and self._wanted(typ):
                pair = (data, None) if x == 0 else (None, data)
                rows.append((typ, ts, self.s.select(*pair)))
        return rows

    def _expire_time(self, x: int):
        """The EXPIRED events a time side emits at the current clock."""
        T = self.sides[x].window[1]
        out = []
        while self.q[x] and self.q[x][0][0] + T <= self.clock:
            _, data = self.q[x].pop(0)
            out.append((EXPIRED, self.clock, data))
        return out

    # -- input
    def advance(self, now: int):
        """The app clock moves to `now`: the time sides' due timers fire in the
        order of their due times (the Scheduler's notifyAt of each item's
        ts + T), the left side's first on a tie, each with the clock at its due
        time; a firing is one chunk."""
        if self.clock is not None and now < self.clock:
            return []
        chunks = []
        while True:
            due = [(self.q[x][0][0] + self.sides[x].window[1], x) for x in (0, 1)
                   if self.sides[x].window is not None and self.sides[x].window[0] == "time" and self.q[x]]
            due = [d for d in due if d[0] <= now]
            if not due:
                break
            t, x = min(due)
            self.clock = t if self.clock is None else max(self.clock, t)
            rows = self._join(x, self._expire_time(x))
            if rows:
                chunks.append(rows)
        self.clock = now
        return chunks

    def send(self, x: int, events):
        """One InputHandler call on side x.  The runtime moves the clock (and
        fires the timers) before it routes the call: see advance()."""
        last = events[-1][0]
        if self.clock is None or last >= self.clock:
            self.clock = last
        side = self.sides[x]
        chunk = []
        for ts, data in events:
            if side.filter is not None and not side.filter(data):
                continue
            if side.window is None:
                chunk.append((CURRENT, ts, data))
                chunk.append((EXPIRED, self.clock, data))
            elif side.window[0] == "length":
                if len(self.q[x]) >= side.window[1]:
                    _, old = self.q[x].pop(0)
                    chunk.append((EXPIRED, self.clock, old))
                chunk.append((CURRENT, ts, data))
                self.q[x].append((ts, data))
            else:
                chunk.extend(self._expire_time(x))
                chunk.append((CURRENT, ts, data))
                self.q[x].append((ts, data))
        rows = self._join(x, chunk)
        return rows or None

    def run(self, steps):
        """steps: (side, [events]) sends and ("time", now) clock moves; returns
        every callback chunk in order."""
        out = []
        for a, b in steps:
            if a == "time":
                out.extend(self.advance(b))
            else:
                rows = self.send(a, b)
                if rows:
                    out.append(rows)
        return out
