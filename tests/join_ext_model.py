"""Plain-Python, per-event restatement of a stream-stream join whose sides may
hold an `externalTime` window, next to the kinds tests/join_model.py knows
(`length`, none).

Window: ExternalTimeWindowProcessor.java :125-161 (process), :174-186 (find).
For every event j that passes the side's filters, with tau the value of the
side's time attribute:

  1. while the queue's head i has tau_i - tau_j + T <= 0: pop it and emit it
     as an EXPIRED event stamped tau_j (the arriving event's attribute, not the
     app clock); stop at the first head that is not due -- an item with a small
     tau behind such a head stays (FIFO blocking);
  2. emit j as CURRENT with its own timestamp and append it to the queue.

The whole call is handled this way first; then every CURRENT and EXPIRED event
of the chunk, in that order, looks the other side up as join_model.Model._join
does.  Each side has its own clock: one side's events never expire the other
side's items.  An event whose time attribute is null does not enter the join
(the reference fails its whole call with a NullPointerException; the library
drops the event like a filter miss, DESIGN.md "Joins").

This file walks the queue literally; it does not use the closed form the device
code uses (running maximum + binary search).  No library code is used.

A side's window is ("externalTime", attribute index, T), ("length", L) or None.
"""
import join_model as jm
from join_model import CURRENT, EXPIRED, Side, Spec   # noqa: F401  (re-exported for the tests)


def ext(col, t, filter=None, unidirectional=False):
    return Side(("externalTime", col, t), filter, unidirectional)


class Model(jm.Model):
    """join_model.Model with externalTime sides.  stats: what a run reached
    (the tests assert that their workloads reach the kernels' tile numbers)."""

    def __init__(self, spec, count_blocked=False):
        super().__init__(spec)
        self.count_blocked = count_blocked   # a scan of the whole queue per event: only where a test asks
        self.stats = {"max_expired_by_one_event": 0, "max_window_met": 0, "blocked_due_items": 0,
                      "expired_rows": 0}

    def _join(self, x, chunk):
        if chunk and not self.sides[1 - x].unidirectional:
            self.stats["max_window_met"] = max(self.stats["max_window_met"], len(self._content(1 - x)))
        rows = super()._join(x, chunk)
        self.stats["expired_rows"] += sum(1 for r in rows if r[0] == EXPIRED)
        return rows

    def send(self, x, events):
        side = self.sides[x]
        if side.window is None or side.window[0] != "externalTime":
            return super().send(x, events)
        last = events[-1][0]
        if self.clock is None or last >= self.clock:
            self.clock = last
        _, col, T = side.window
        q = self.q[x]
        chunk = []
        for ts, data in events:
            if side.filter is not None and not side.filter(data):
                continue
            tau = data[col]
            if tau is None:
                continue
            popped = 0
            while q and q[0][1][col] - tau + T <= 0:
                _, old = q.pop(0)
                chunk.append((EXPIRED, tau, old))
                popped += 1
            if self.count_blocked and any(d[col] - tau + T <= 0 for _, d in q):
                self.stats["blocked_due_items"] += 1
            self.stats["max_expired_by_one_event"] = max(self.stats["max_expired_by_one_event"], popped)
            chunk.append((CURRENT, ts, data))
            q.append((ts, data))
        rows = self._join(x, chunk)
        return rows or None


def literal_windows(taus, T):
    """The literal loop over one side's time values alone: per item j, (the
    indices it expires, the index its window starts at afterwards)."""
    q, out = [], []
    for j, tau in enumerate(taus):
        gone = []
        while q and taus[q[0]] - tau + T <= 0:
            gone.append(q.pop(0))
        q.append(j)
        out.append((gone, q[0]))
    return out
