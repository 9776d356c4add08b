"""Keyed exact window engine (engine_window.hip): the storage paths that only
run when a table outgrows itself between pushes, each against the CPU oracle
row for row like tests/test_gpu_window_x.py.

* the item store grows while it carries items (WindowXEngine::ensure_items
  with C > 0: every column -- and every strided attribute / argument
  sub-column -- is copied into a slot of another capacity);
* the aggregator state tables, and a batch window's epoch table, grow while
  they hold sums that a later push reads (ensure_states);
* a snapshot taken after that growth restores into tables of exactly the saved
  size (load_state), and the stream continues as if uninterrupted.

Sizes follow the engine's constants (first capacity 1024, doubling; a carry of
k items leaves a slot of max(2k, 1024)): pushes of 600, 600 and 4500 events
through length(3000) reach the third push with 1200 carried items in a slot of
2400, which 5700 items outgrow."""
import numpy as np
import pytest

from parity import assert_same_rows, compile_single_query, concat_rows, run_device, run_oracle
from siddhi_amd.runtime import ColumnBatch
from test_gpu_window_x import SCHEMA

pytestmark = pytest.mark.gpu


def make_pushes(seed, keys_per_push, call=257):
    """One batch per entry of keys_per_push (its events' k column); the other
    attributes drawn, 5 % nulls, playback time increasing with repeats."""
    rng = np.random.default_rng(seed)
    out = []
    t = 10_000
    for k in keys_per_push:
        k = np.asarray(k, np.int32)
        m = len(k)
        i = rng.integers(0, 5, m).astype(np.int32)
        lv = rng.integers(-10 ** 6, 10 ** 6, m).astype(np.int64)
        f = rng.uniform(-50, 50, m).astype(np.float32)
        d = rng.uniform(0, 100, m)
        nl = [None, None] + [(rng.random(m) < 0.05).astype(np.uint8) for _ in range(3)]
        ts = t + np.cumsum(rng.choice([0, 0, 1, 1, 2], m)).astype(np.int64)
        t = int(ts.max()) + 3
        offs = np.arange(0, m + 1, call, dtype=np.int64)
        if offs[-1] != m:
            offs = np.append(offs, m)
        out.append((0, ColumnBatch(ts, [k, i, lv, f, d], nl, offs)))
    return out


ITEM_APPS = [
    ("plain", "from S#window.length(3000) select k, f, d insert all events into O;"),
    ("groupby", "from S#window.length(3000) select k, sum(d) as s, avg(f) as a, count() as c group by k "
                "insert all events into O;"),
]


@pytest.mark.parametrize("name,app", ITEM_APPS, ids=[a[0] for a in ITEM_APPS])
def test_item_store_grows_while_it_carries(hip_available, name, app):
    rng = np.random.default_rng(3)
    qp, _ = compile_single_query(SCHEMA + app)
    batches = make_pushes(11, [rng.integers(0, 40, m) for m in (600, 600, 4500)])
    ora = run_oracle(qp, batches)
    dev, counters, kind = run_device(qp, batches)
    assert kind == 2
    assert counters["carry"] == 3000
    assert (ora[1] == 1).sum() > 0   # EXPIRED rows: the window overflowed in the third push
    assert_same_rows(dev, ora)


STATE_APPS = [
    ("length", "from S#window.length(3000) select k, sum(d) as s, count() as c group by k "
               "insert all events into O;"),
    ("lengthBatch", "from S#window.lengthBatch(50) select k, sum(d) as s, count() as c group by k "
                    "insert all events into O;"),
]


def state_pushes():
    """700 distinct keys, then 1500 more (2200 states outgrow the first table
    of 1024), then the keys of the first push again."""
    rng = np.random.default_rng(5)
    p1 = rng.permutation(np.r_[np.arange(700), np.arange(700), np.arange(25)])
    p2 = rng.permutation(np.r_[np.arange(700, 2200), np.arange(700, 713)])
    p3 = rng.permutation(np.arange(715) % 700)
    return make_pushes(17, [p1, p2, p3])


@pytest.fixture(scope="module")
def state_runs():
    """Per app: the compiled query, the pushes and the oracle's rows."""
    runs = {}
    batches = state_pushes()
    for name, app in STATE_APPS:
        qp, _ = compile_single_query(SCHEMA + app)
        runs[name] = (qp, batches, run_oracle(qp, batches))
    return runs


@pytest.mark.parametrize("name", [a[0] for a in STATE_APPS])
def test_state_tables_grow_while_they_hold_sums(hip_available, state_runs, name):
    qp, batches, ora = state_runs[name]
    dev, _, kind = run_device(qp, batches)
    assert kind == 2
    assert len(ora[2]) > 0
    assert_same_rows(dev, ora)


@pytest.mark.parametrize("name", [a[0] for a in STATE_APPS])
def test_snapshot_after_growth(hip_available, state_runs, name):
    """shd_snapshot after the push that grew the tables, restore into a fresh
    query: the third push gives the rows of the uninterrupted run."""
    from siddhi_amd.hip_engine import DeviceQuery, SHD_MEM_HOST
    qp, batches, ora = state_runs[name]

    def push(dq, si, b):
        cols = [np.ascontiguousarray(c) for c in b.cols]
        nuls = [None if x is None else np.ascontiguousarray(x, np.uint8) for x in b.nulls]
        ts = np.ascontiguousarray(b.ts, np.int64)
        dq.push_raw(si, b.n, ts.ctypes.data, [c.ctypes.data for c in cols],
                    [0 if x is None else x.ctypes.data for x in nuls], SHD_MEM_HOST, b.call_offsets, True)
        return dq.poll()

    parts = []
    dq = DeviceQuery(qp.ir)
    try:
        for si, b in batches[:2]:
            r = push(dq, si, b)
            if r is not None:
                parts.append(r)
        image = dq.snapshot()
    finally:
        dq.close()
    dq2 = DeviceQuery(qp.ir)
    try:
        dq2.restore(image)
        for si, b in batches[2:]:
            r = push(dq2, si, b)
            if r is not None:
                parts.append(r)
    finally:
        dq2.close()
    assert_same_rows(concat_rows(parts), ora)
