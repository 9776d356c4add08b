"""The lean forward scan that decides or defers (k_forward_scan_rec<true,
false>): a candidate is open (end of its key's run), dead by the slice bounds,
or deferred as it stands -- the scan reads no row and walks nothing.  The
deferred walk (k_resume_list, HOT) starts at p + 1 with the scan's own hot
walk and only then goes on with f2; a hot walk that ends open has met no B
event of its key, so the partial stays in the new list (pend flag unchanged).
SHD_SCAN_ROW_WALK=1 keeps the scan that reads its undecided candidates' rows
and walks them itself.

Every case runs the same pushes three ways under SHD_FUSED_SORT=1,
SHD_LEAN_SORT=1 and SHD_RESUME_MODE=0 -- the default, SHD_SCAN_ROW_WALK=1 and
SHD_NO_LEAN_SORT=1 -- and asserts: rows equal the CPU oracle's; the five walk
counters are equal across the three runs; the decoded state image after every
push (carry keys, times, seqs, pend flags and kept columns) is equal across
the three runs.

`within` is 1 s and pushes step 0.25 ms per row as in test_gpu_lean_sort.py.
At test sizes a tile is 256 positions and a sub-tile one 64-position slice.

Reference: ST/StreamPreStateProcessor.java:118-129,326-403 (expiry, process,
new / pending list placement)."""
import numpy as np
import pytest

from parity import assert_same_rows, compile_single_query, run_oracle, stock_batch
from siddhi_amd import workloads as wl
from siddhi_amd.runtime import ColumnBatch
from test_gpu_lean_sort import OR_APP, W, as_batch, cold, pair, put, three_pushes
from test_gpu_scan_lists import COUNTERS, OR_CARRIED, P3_CARRIED, batch, run_device_snap

pytestmark = pytest.mark.gpu

WAYS = (("default", ()), ("row_walk", (("SHD_SCAN_ROW_WALK", "1"),)), ("no_lean", (("SHD_NO_LEAN_SORT", "1"),)))


def check3(qp, batches, monkeypatch, carried=P3_CARRIED, kind_end=1, min_rows=1):
    ora = run_oracle(qp, batches)
    assert len(ora[2]) >= min_rows, "the shape yields no row"
    for k in ("SHD_NO_RESUME_LIST", "SHD_NO_SCAN_LISTS", "SHD_TS64", "SHD_LOCKSTEP", "SHD_SCAN_ROW_WALK",
              "SHD_NO_LEAN_SORT"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SHD_FUSED_SORT", "1")
    monkeypatch.setenv("SHD_LEAN_SORT", "1")
    monkeypatch.setenv("SHD_RESUME_MODE", "0")
    runs = []
    for name, env in WAYS:
        for k, v in env:
            monkeypatch.setenv(k, v)
        dev, counters, kind, snaps = run_device_snap(qp, batches, carried)
        for k, _ in env:
            monkeypatch.delenv(k)
        assert kind == kind_end, name
        assert_same_rows(dev, ora)
        runs.append((name, counters, snaps))
    _, c0, s0 = runs[0]
    for name, c, s in runs[1:]:
        for k in COUNTERS:
            assert c0[k] == c[k], "%s: %s" % (name, k)
        assert len(s0) == len(s)
        for i, (a, b) in enumerate(zip(s0, s)):
            assert a.keys() == b.keys(), "%s: push %d" % (name, i)
            for k in a:
                assert a[k] == b[k], "%s: state after push %d: %s" % (name, i, k)
    return s0


def pend_of(snap, key):
    """Pend flags of the carried partials of `key`, in carry order."""
    keys = np.frombuffer(snap["key"], np.uint64)
    return np.frombuffer(snap["pend"], np.uint8)[keys == key].tolist()


@pytest.mark.parametrize("gap", [W - 1, W, W + 1])
def test_defer_pairs_undecided_by_the_slice_bounds(hip_available, monkeypatch, gap):
    """Pairs `gap` ms apart inside one push: completing, failing and staying pending."""
    qp, _ = compile_single_query(wl.P3_APP)
    check3(qp, three_pushes(np.random.default_rng(140 + gap), gap), monkeypatch)


def test_defer_fresh_walk_ends_open_without_a_b_event(hip_available, monkeypatch):
    """Keys 101 (three partials: the first two met a later event of the key,
    pend 1; the last did not, pend 0) and 102 (two partials) are carried across
    push 2, which holds no event of either: their carried rows are neighbours
    in sorted order, every one but the key's last is deferred, and its hot walk
    passes carried rows only and ends open -- the pend flags stay what they
    were.  Key 101 returns in push 3 inside `within` (all three complete), key
    102 past it (both expire), key 103 never."""
    rng = np.random.default_rng(151)
    a = cold(rng, 3001, 0)                       # 0 .. 750 ms
    for i, p in enumerate((71.0, 71.5, 72.0)):
        put(a, 2800 + 4 * i, 101, p)             # 700 ms
    put(a, 400, 102, 71.0)                       # 100 ms
    put(a, 404, 102, 72.0)
    put(a, 1000, 103, 71.0)
    put(a, 1004, 103, 71.2)
    put(a, 2000, 104, 71.0)                      # a row for push 1
    put(a, 2012, 104, 99.9)
    b = cold(rng, 801, 755)                      # .. 955 ms
    c = cold(rng, 2001, 960)
    put(c, 0, 101, 99.9)                         # 260 ms after its partials
    put(c, 4 * 200, 102, 99.9)                   # 1160 ms: 1060 after
    qp, _ = compile_single_query(wl.P3_APP)
    snaps = check3(qp, [as_batch(a), as_batch(b), as_batch(c)], monkeypatch)
    for key, pend in ((101, [1, 1, 0]), (102, [1, 0]), (103, [1, 0])):
        assert pend_of(snaps[0], key) == pend, key
        assert pend_of(snaps[1], key) == pend, key
    assert pend_of(snaps[2], 101) == [0]         # the completing event's own partial
    assert pend_of(snaps[2], 102) == [0]
    assert pend_of(snaps[2], 103) == [1, 0]


def test_defer_fresh_walk_past_carried_rows_to_an_event_of_the_push(hip_available, monkeypatch):
    """The carried partials' key returns inside the same push: the hot walk
    passes the key's other carried rows, stops at the pushed event, and the f2
    walk matches (111), finds the partials expired (112) or fails f2 and
    leaves them pending (113: pend 1)."""
    rng = np.random.default_rng(152)
    a = cold(rng, 3001, 0)
    put(a, 2800, 111, 71.0)
    put(a, 2804, 111, 71.5)
    put(a, 400, 112, 71.0)
    put(a, 404, 112, 71.5)
    put(a, 2900, 113, 71.0)
    put(a, 2904, 113, 71.5)
    put(a, 2908, 113, 71.7)
    b = cold(rng, 2001, 755)                     # .. 1255 ms
    put(b, 40, 111, 99.9)
    put(b, 4 * 400, 112, 99.9)                   # 1155 ms: 1055 after
    put(b, 80, 113, 60.0)
    c = cold(rng, 1001, 1260)
    put(c, 8, 113, 99.9)
    qp, _ = compile_single_query(wl.P3_APP)
    snaps = check3(qp, [as_batch(a), as_batch(b), as_batch(c)], monkeypatch)
    assert pend_of(snaps[0], 113) == [1, 1, 0]
    assert pend_of(snaps[1], 113) == [1, 1, 1]
    assert pend_of(snaps[1], 111) == [0] and pend_of(snaps[1], 112) == [0]


def test_defer_null_keys_and_null_f2_operands_on_the_successor(hip_available, monkeypatch):
    """Key 2000's candidate is followed in sorted order by a dropped (null-key)
    row, which sorts by its row index; key 120's candidate by an event of its
    key whose price is null (f2 false: pending), then by one that completes."""
    rng = np.random.default_rng(153)
    n = 5001
    a = cold(rng, n, 0)
    knul = (rng.random(n) < 0.1).astype(np.uint8)
    knul[[500, 512, 600, 1500, 2400, 4000]] = 0
    knul[2000] = 1
    put(a, 1500, 2000, 71.0)
    put(a, 2400, 2000, 99.9)
    put(a, 4000, 2000, 60.0)
    pnul = (rng.random(n) < 0.05).astype(np.uint8)
    pnul[[500, 600, 1500, 2400, 4000]] = 0
    pnul[512] = 1
    put(a, 500, 120, 71.0)
    put(a, 512, 120, 99.9)                       # null price
    put(a, 600, 120, 99.9)
    b = cold(rng, 2001, int(a[2][-1]) + 5)
    put(b, 16, 120, 60.0)

    def nb(push, kn, pn):
        sym = np.asarray(push[0], np.uint32)
        ts = wl.T0 + np.asarray(push[2], np.int64)
        vol = (np.arange(len(ts), dtype=np.int64) % 1000) + 1
        offs = np.append(np.arange(0, len(ts), 4096, dtype=np.int64), np.int64(len(ts)))
        return (0, ColumnBatch(ts, [sym, np.asarray(push[1], np.float64), vol], [kn, pn, None], offs))

    qp, _ = compile_single_query(wl.P3_APP)
    check3(qp, [nb(a, knul, pnul), nb(b, np.zeros(2001, np.uint8), np.zeros(2001, np.uint8))], monkeypatch)


@pytest.mark.parametrize("n", [255, 256, 257, 300])
def test_defer_every_candidate_deferred(hip_available, monkeypatch, n):
    """Three hot keys, every event a candidate, everything inside `within`:
    every position but each key's last is deferred, so each sub-tile's deferred
    list is as long as the sub-tile.  n_ext just below, at and above one tile
    (256); 257 and 300 leave a last sub-tile of 1 and 44 positions."""
    rng = np.random.default_rng(160 + n)
    hot = np.array([7, 1 << 21, (1 << 22) - 3])
    k1 = rng.choice(hot, n)
    p1 = 70.5 + 29.0 * rng.random(n)
    k2 = rng.choice(hot, 200)
    p2 = 70.5 + 29.0 * rng.random(200)
    b1 = batch(k1, p1, wl.T0 + np.arange(n))
    b2 = batch(k2, p2, wl.T0 + n + 5 + np.arange(200))
    qp, _ = compile_single_query(wl.P3_APP)
    check3(qp, [b1, b2], monkeypatch)


def test_defer_time_regression_seen_by_a_deferred_walk_only(hip_available, monkeypatch):
    """Key 82's candidate (row 10 of push 2) carries a later time than the
    key's next event (row 100): the regression lies at the first step of the
    candidate's own walk, before any f2 -- the step the scan used to take
    itself.  The scan now defers the candidate unread, the deferred walk's hot
    stage reports the regression, and the generic NFA engine takes over from
    push 1's carry."""
    rng = np.random.default_rng(164)
    a = cold(rng, 3001, 0)
    pair(a, 400, 3, 81)
    b = cold(rng, 2001, int(a[2][-1]) + 5)
    put(b, 10, 82, 71.0)
    put(b, 100, 82, 60.0)
    b[2][10] += 100                              # key 82: the earlier row carries the later time
    put(b, 200, 81, 99.9)
    qp, _ = compile_single_query(wl.P3_APP)
    check3(qp, [as_batch(a), as_batch(b)], monkeypatch, kind_end=4)


def test_defer_or_form(hip_available, monkeypatch):
    qp, _ = compile_single_query(OR_APP)
    sym, price, vol, ts = wl.stock_stream(12_000, 4_000_000, 0.25, seed_offset=41)
    sym[3000], price[3000] = 7, 71.0
    sym[3012], price[3012] = 7, 60.0     # 3 ms later, below 0.9 * 71: the e3 branch
    sym[2000], price[2000] = 8, 71.0
    sym[2000 + 4 * (W + 1)], price[2000 + 4 * (W + 1)] = 8, 99.0   # expired
    sym[5900], price[5900] = 9, 71.0
    sym[5904], price[5904] = 9, 71.5     # two partials carried past push 2's carried rows
    sym[6100], price[6100] = 9, 99.0
    cuts = [0, 6001, 9004, 12_000]
    batches = [(0, stock_batch(sym[a:b], price[a:b], vol[a:b], ts[a:b])) for a, b in zip(cuts[:-1], cuts[1:])]
    check3(qp, batches, monkeypatch, carried=OR_CARRIED)
