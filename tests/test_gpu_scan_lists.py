"""The pattern engine's emitting forward scan (k_forward_scan_rec): on sparse
keys in the plain / OR forms the scan itself writes, per sub-tile (one wave's
quarter of a tile), the records of the positions that end open or deferred
and the list of deferred positions; the deferred walks run from those lists
and the carry is gathered from the records (k_gather_rec).  SHD_NO_SCAN_LISTS=1
keeps the list passes (k_open_list + k_gather_list).

Every case runs several pushes once by default and once with
SHD_NO_SCAN_LISTS=1 (SHD_FUSED_SORT=1 and SHD_RESUME_MODE=0, so test sizes
take P3's path) and asserts: rows equal the CPU oracle's; the walk counters
are equal between the two runs; the state image after every push is equal
between the two runs.  The image (shd_snapshot) also holds the per-push kernel
time and the carry columns the plan never reads again, which no gather
writes, so the test decodes it and compares the state: arrival seq, playback
time, chunk id, counters without the two times, C, horizon, last times, and of
the carry the columns the plan keeps with their null bytes, times, keys, seqs
and pend flags.

At test sizes a tile is 256 positions and a sub-tile one 64-position slice;
past 2^20 extended rows a tile is 512 and a sub-tile two slices, past 2^21 a
tile is 768 and a sub-tile three (one large case each).  The scripted case
puts the runs of its hot keys across position 64 (slice, and sub-tile at the
small size), 128 (sub-tile) and 512 (tile); the 2^21 case fills the scan's
per-wave record ring past its 128 slots with records left waiting across a
flush, as the flagship run does.

Reference: ST/StreamPreStateProcessor.java:118-129,326-403 (expiry, process,
new / pending list placement)."""
import ctypes

import numpy as np
import pytest

from parity import assert_same_rows, compile_single_query, concat_rows, run_oracle, stock_batch
from siddhi_amd import workloads as wl
from siddhi_amd.runtime import ColumnBatch

pytestmark = pytest.mark.gpu

COUNTERS = ("events", "matches", "partials", "partial_scans", "carry")
KEYS = 1 << 22
# a long `within` and an f2 that holds only for e1.price < 72.46 and e2.price > 96.6
LONG_APP = wl.P3_APP.replace("within 1 sec", "within 20 sec").replace("e1.price*1.05", "e1.price*1.38")
assert LONG_APP.count("within 20 sec") == 1 and LONG_APP.count("e1.price*1.38") == 1
P3_CARRIED = (0, 1)   # e1.symbol, e1.price
OR_CARRIED = (1,)     # e1.price


def decode(image, carried):
    """The state held by a snapshot image (layout: shd_snapshot + PatternEngine::save_state)."""
    from siddhi_amd.hip_engine import ShdCounters
    names = [f for f, _ in ShdCounters._fields_]
    kind = int(np.frombuffer(image, np.int32, 1, 8)[0])
    off = 12 + 8 + 8 + 8   # magic, version, kind, layout hint, start time, plan hash
    head = np.frombuffer(image, np.int64, 3, off).tolist()   # seq, now, chunk_seq
    off += 24
    cnt = np.frombuffer(image, np.int64, len(names), off).tolist()
    off += ctypes.sizeof(ShdCounters)
    st = {"kind": kind, "head": head,
          "counters": {k: v for k, v in zip(names, cnt) if not k.startswith("kernel_ns")}}
    if kind != 1:
        return st
    C = int(np.frombuffer(image, np.int64, 1, off)[0])
    st["C"] = C
    st["have_horizon"] = int(np.frombuffer(image, np.int32, 1, off + 8)[0])
    st["tail"] = np.frombuffer(image, np.int64, 3, off + 12).tolist()   # horizon, t_last, last_b_seq
    ncols = int(np.frombuffer(image, np.int32, 1, off + 36)[0])
    off += 40

    def blob():
        nonlocal off
        n = int(np.frombuffer(image, np.uint64, 1, off)[0])
        b = image[off + 8:off + 8 + n]
        off += 8 + n
        return b

    for c in range(ncols):
        col, nul = blob(), blob()
        assert len(nul) == C
        if c in carried:
            st["col%d" % c] = col
            st["nul%d" % c] = nul
    for k in ("ts", "key", "seq", "pend"):
        st[k] = blob()
    assert len(st["ts"]) == 8 * C and len(st["pend"]) == C
    assert off == len(image)
    return st


def run_device_snap(qp, batches, carried):
    """parity.run_device, with the decoded state image after every push."""
    from siddhi_amd.hip_engine import DeviceQuery, SHD_MEM_HOST
    dq = DeviceQuery(qp.ir)
    parts, snaps = [], []
    try:
        for si, b in batches:
            cols = [np.ascontiguousarray(c) for c in b.cols]
            nuls = [None if x is None else np.ascontiguousarray(x, np.uint8) for x in b.nulls]
            ts = np.ascontiguousarray(b.ts, np.int64)
            dq.push_raw(si, b.n, ts.ctypes.data, [c.ctypes.data for c in cols],
                        [0 if x is None else x.ctypes.data for x in nuls], SHD_MEM_HOST,
                        b.call_offsets if len(b.call_offsets) > 2 else None, True)
            r = dq.poll()
            if r is not None:
                parts.append(r)
            snaps.append(decode(dq.snapshot(), carried))
        counters = dq.counters()
        kind = dq.engine_kind
    finally:
        dq.close()
    return concat_rows(parts), counters, kind, snaps


def leaves_open_partial(batches):
    """From the input alone: some key's last event passes f1 (price > 70 in
    every app here) under a non-null key.  A partitioned plan expires or
    completes a partial only on a later event of its key, so that one is
    carried out of the last push."""
    sym = np.concatenate([b.cols[0] for _, b in batches]).astype(np.int64)
    price = np.concatenate([b.cols[1] for _, b in batches])
    nul = np.concatenate([np.zeros(b.n, np.uint8) if b.nulls[0] is None else b.nulls[0] for _, b in batches])
    sym, price = sym[nul == 0], price[nul == 0]
    _, first_rev = np.unique(sym[::-1], return_index=True)
    last = len(sym) - 1 - first_rev
    return bool((price[last] > 70.0).any())


def check(qp, batches, monkeypatch, carried=P3_CARRIED, kind_end=1, min_carry=1):
    ora = run_oracle(qp, batches)
    assert len(ora[2]) >= 1, "the shape yields no row"
    assert leaves_open_partial(batches), "the shape carries no partial"
    monkeypatch.setenv("SHD_FUSED_SORT", "1")
    monkeypatch.setenv("SHD_RESUME_MODE", "0")
    monkeypatch.delenv("SHD_NO_RESUME_LIST", raising=False)
    monkeypatch.delenv("SHD_NO_SCAN_LISTS", raising=False)
    dev, c_scan, kind, s_scan = run_device_snap(qp, batches, carried)
    assert kind == kind_end
    assert_same_rows(dev, ora)
    monkeypatch.setenv("SHD_NO_SCAN_LISTS", "1")
    dev2, c_list, kind2, s_list = run_device_snap(qp, batches, carried)
    assert kind2 == kind_end
    assert_same_rows(dev2, ora)
    for k in COUNTERS:
        assert c_scan[k] == c_list[k], k
    assert max(s.get("C", 0) for s in s_list) >= min_carry, "the shape carries no partial"
    for i, (a, b) in enumerate(zip(s_scan, s_list)):
        assert a.keys() == b.keys(), "push %d" % i
        for k in a:
            assert a[k] == b[k], "state after push %d: %s" % (i, k)
    return s_list


def batch(sym, price, ts, nul=None, call=256):
    sym = np.asarray(sym, np.uint32)
    price = np.asarray(price, np.float64)
    ts = np.asarray(ts, np.int64)
    vol = (np.arange(len(ts), dtype=np.int64) % 1000) + 1
    if nul is None:
        return (0, stock_batch(sym, price, vol, ts, call))
    offs = np.append(np.arange(0, len(ts), call, dtype=np.int64), np.int64(len(ts)))
    return (0, ColumnBatch(ts, [sym, price, vol], [nul, None, None], offs))


def random_push(rng, n, t0, hot, p_hot=0.15, dt=1.0):
    """n events, `p_hot` of them on the hot keys, the rest over KEYS key ids."""
    sym = rng.integers(0, KEYS, n)
    m = rng.random(n) < p_hot
    sym[m] = rng.choice(hot, int(m.sum()))
    price = 50.0 + 50.0 * rng.random(n)
    ts = wl.T0 + t0 + np.floor(np.arange(n) * dt).astype(np.int64)
    return sym, price, ts


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 257, 1025])
def test_scan_lists_first_push_sizes(hip_available, monkeypatch, n):
    """n_ext of the first push around the slice, sub-tile and tile sizes: the
    last sub-tile and its last slice partial, sub-tiles past the end empty."""
    qp, _ = compile_single_query(LONG_APP)
    rng = np.random.default_rng(100 + n)
    hot = np.array([7, KEYS // 2 + 1, KEYS - 3])
    s1, p1, t1 = random_push(rng, n, 0, hot)
    s1[0], p1[0] = hot[1], 71.0                     # an open partial at any n ...
    s2, p2, t2 = random_push(rng, 300, 2000, hot)
    s2[150], p2[150] = hot[1], 99.9                 # ... that the second push completes
    s3, p3, t3 = random_push(rng, 300, 4000, hot)
    check(qp, [batch(s1, p1, t1), batch(s2, p2, t2), batch(s3, p3, t3)], monkeypatch)


def scripted(fill, seed):
    """Three pushes over `fill` cold events of distinct even keys and four hot
    (odd) keys whose first-push runs start at sorted positions 60 (H), 126 (G),
    510 (M) and further on (X).  Times in ms from T0; `within` is 20 s.
      H  candidates 71, 71.5, 72, 71.2 with a low event between and 72.3 last:
         deferred walks that end open (PS_PEND) and a plain open one in one key;
         push 2 sends a low event, then 99.9: the carried ones defer and all
         five complete on that one e2 event (rows in creation order).
      G  candidates 75, 80, 85 no event can complete: carried through all three
         pushes; a low event in push 2 moves them to the pending list
         (pend_old 0 -> 1), cold partials keep pend 0.
      M  71, a low event, 99.9 inside one push: a deferred walk that ends in a
         match (and again in push 3).
      X  71, a low event 10 s later, another 25 s later: a deferred walk that
         ends expired."""
    rng = np.random.default_rng(seed)
    ck = np.sort(rng.choice(KEYS // 2, fill, replace=False)) * 2
    H = ck[60] - 1
    G = ck[126 - 7] - 1
    M = ck[510 - 7 - 3] - 1
    X = ck[700] - 1

    def hot(key, *tp):
        return [(t, key, p) for t, p in tp]

    def push(cold_ts, cold_key, cold_price, hots):
        ts, key, price = (np.array(v) for v in zip(*hots))
        ts = np.concatenate([cold_ts, ts])
        o = np.argsort(ts, kind="stable")
        return batch(np.concatenate([cold_key, key])[o], np.concatenate([cold_price, price])[o], wl.T0 + ts[o],
                     call=4096)

    def cold_price(n):   # one in four a candidate
        u = rng.random(n)
        return np.where(rng.random(n) < 0.25, 70.5 + 29.0 * u, 50.0 + 19.0 * u)

    p1 = push(rng.integers(0, 26000, fill), rng.permutation(ck), cold_price(fill),
              hot(H, *[(20000 + 100 * i, p) for i, p in enumerate((71.0, 71.5, 60.0, 72.0, 71.2, 55.0, 72.3))]) +
              hot(G, (22000, 75.0), (22100, 80.0), (22200, 85.0)) +
              hot(M, (9000, 71.0), (10000, 60.0), (11000, 99.9)) +
              hot(X, (0, 71.0), (10000, 60.0), (25500, 60.0)))
    p2 = push(27000 + 20 * np.arange(200), ck[:200] + 2 * KEYS, cold_price(200),
              hot(H, (28000, 60.0), (30000, 99.9)) + hot(G, (29000, 60.0)))
    p3 = push(36000 + 10 * np.arange(100), ck[200:300] + 2 * KEYS, cold_price(100),
              hot(M, (36100, 71.0), (36200, 60.0), (36300, 99.9)))
    return [p1, p2, p3]


@pytest.mark.parametrize("fill", [1500, (1 << 20) + 300], ids=["tile256", "tile512"])
def test_scan_lists_hot_runs_across_boundaries(hip_available, monkeypatch, fill):
    qp, _ = compile_single_query(LONG_APP)
    snaps = check(qp, scripted(fill, 7), monkeypatch)
    # both pend values are carried out of the last push
    pend = np.frombuffer(snaps[-1]["pend"], np.uint8)
    assert pend.min() == 0 and pend.max() == 1


def test_scan_lists_every_position_open(hip_available, monkeypatch):
    """Every position of the first push a candidate that stays open: a
    sub-tile's records fill it; the second push defers half of them."""
    qp, _ = compile_single_query(LONG_APP)
    rng = np.random.default_rng(5)
    n = 320
    keys = rng.choice(KEYS, n, replace=False)
    b1 = batch(keys, np.full(n, 71.0), wl.T0 + np.arange(n))
    k2 = np.concatenate([keys[::2], keys[:10]])
    p2 = np.concatenate([np.full(n // 2, 60.0), np.full(10, 99.0)])
    b2 = batch(k2, p2, wl.T0 + 1000 + np.arange(len(k2)))
    snaps = check(qp, [b1, b2], monkeypatch)
    assert snaps[0]["C"] == n


def test_scan_lists_push_without_open_and_without_deferral(hip_available, monkeypatch):
    """Push 1 has no candidate (no open partial, no record), push 2 distinct
    keys only (no deferral), push 3 completes and defers some of them."""
    qp, _ = compile_single_query(LONG_APP)
    rng = np.random.default_rng(6)
    k1 = rng.choice(KEYS, 200, replace=False)
    b1 = batch(k1, 50.0 + 19.0 * rng.random(200), wl.T0 + np.arange(200))
    k2 = rng.choice(KEYS, 300, replace=False)
    b2 = batch(k2, 70.5 + 1.5 * rng.random(300), wl.T0 + 1000 + np.arange(300))
    k3 = np.concatenate([k2[:40], k2[:20]])
    p3 = np.concatenate([np.full(40, 60.0), np.full(20, 99.5)])
    b3 = batch(k3, p3, wl.T0 + 2000 + np.arange(60))
    snaps = check(qp, [b1, b2, b3], monkeypatch)
    assert snaps[0]["C"] == 0 and snaps[1]["C"] == 300


def test_scan_lists_null_partition_keys(hip_available, monkeypatch):
    qp, _ = compile_single_query(LONG_APP)
    rng = np.random.default_rng(8)
    hot = np.array([11, KEYS // 3, KEYS - 5])
    batches = []
    for i in range(3):
        s, p, t = random_push(rng, 500, 1000 * i, hot, p_hot=0.3)
        batches.append(batch(s, p, t, nul=(rng.random(500) < 0.1).astype(np.uint8)))
    check(qp, batches, monkeypatch)


def test_scan_lists_time_regression_hands_over(hip_available, monkeypatch):
    """The third push goes back in time inside the hot keys: the generic NFA
    engine takes over from the carry of the second push (compared above by the
    state after push 2) and the rows stay the oracle's."""
    qp, _ = compile_single_query(LONG_APP)
    rng = np.random.default_rng(9)
    hot = np.array([5, KEYS // 2, KEYS - 9])
    pushes = [random_push(rng, 400, 1000 * i, hot, p_hot=0.3) for i in range(3)]
    s3, p3, t3 = pushes[2]
    pushes[2] = (s3, p3, t3 - 1700)   # starts before the second push's first event
    check(qp, [batch(*p) for p in pushes], monkeypatch, kind_end=4)


def test_scan_lists_or_form(hip_available, monkeypatch):
    """`e1 -> (e2 or e3)` partitioned takes the same path (logical OR)."""
    qp, _ = compile_single_query(wl.S4_PART_APPS["or"])
    sym, price, vol, ts = wl.stock_stream(60_000, 4_000_000, 0.01, seed_offset=29)
    cuts = [0, 20_480, 40_960, 60_000]
    batches = [(0, stock_batch(sym[a:b], price[a:b], vol[a:b], ts[a:b])) for a, b in zip(cuts[:-1], cuts[1:])]
    check(qp, batches, monkeypatch, carried=OR_CARRIED)


def test_scan_lists_record_ring_wraps_and_carries_over(hip_available, monkeypatch):
    """The scan's per-wave record ring (kRecRing = 128 slots, 64 records leave
    at a time) in the state the flagship run has it in: past 2^21 extended
    rows a tile is 768 positions and a sub-tile three slices.  Distinct keys,
    so every candidate stays open; in sorted order the lowest quarter of the
    keys are all candidates (a sub-tile yields 192 records: three flushes, the
    third slice's records wrap to slots 0..63) and the rest candidates at 70 %
    (about 45 records a slice: flushes that leave a remainder waiting, slots
    past 128 reused, a last partial flush).  The second push (tile 512 over
    the carried rows, every one an open record) defers some and completes
    some."""
    qp, _ = compile_single_query(LONG_APP)
    rng = np.random.default_rng(12)
    n = (1 << 21) + 600
    keys = rng.choice(1 << 23, n, replace=False)
    dense = keys < (1 << 21)                                  # about a quarter, the lowest keys
    price = np.where(dense | (rng.random(n) < 0.7), 71.0, 60.0)
    b1 = batch(keys, price, wl.T0 + np.arange(n) // 200, call=8192)
    low = keys[dense]
    k2 = np.concatenate([low[:1000], low[500:700]])
    p2 = np.concatenate([np.full(1000, 60.0), np.full(200, 99.0)])
    b2 = batch(k2, p2, wl.T0 + 12000 + np.arange(len(k2)))
    snaps = check(qp, [b1, b2], monkeypatch)
    assert snaps[0]["C"] == int((price == 71.0).sum())
    # 200 partials complete; the 200 completing events (99.0 > 70) open one each
    assert snaps[1]["C"] == snaps[0]["C"] - 200 + 200
