"""The pattern engine's lean key sort: where the emitting forward scan runs
(fused key sort on a 32-bit plain key, plain / OR form, sparse keys, finite
`within`) the rows are sorted as (key, payload) pairs without the 32-bit time
word.  The first pass writes the pushed rows' earliest / latest time per slice
of 1024 extended rows instead; the scan (k_forward_scan_rec<true>) declares a
candidate dead when its successor's slice starts more than `within` after the
latest time the candidate can have, and reads exact times from the rows for
every other candidate; the deferred walks and the carry gather read times
from the rows too.  A push whose sort ran lean but which then takes another
path gets its sorted times rebuilt from the rows (k_sorted_ts32, or
k_sorted_ts64 when 32-bit offsets overflow).

Every case runs the same pushes with the lean sort forced (SHD_LEAN_SORT=1)
and with SHD_NO_LEAN_SORT=1, both under SHD_FUSED_SORT=1 (and
SHD_RESUME_MODE=0 where the case is about the lean scan, so test sizes take
the flagship's path), and asserts: rows equal the CPU oracle's; the walk
counters (partial_scans among them) are equal between the two runs; the
decoded state image after every push (carry times, keys, seqs, pend flags and
kept columns) is equal between the two runs.

`within` is 1 s.  Pushes step 0.25 ms per row, so a 1024-row slice spans
256 ms and a same-key pair about `within` apart is undecided by the slice
bounds; the jump cases put a pair exactly on a slice edge with the bounds
exactly `within` - 1, `within` and `within` + 1 apart.

Reference: ST/StreamPreStateProcessor.java:118-129,326-403 (expiry, process,
new / pending list placement)."""
import numpy as np
import pytest

from parity import assert_same_rows, compile_single_query, run_oracle, stock_batch
from siddhi_amd import workloads as wl
from test_gpu_scan_lists import COUNTERS, OR_CARRIED, P3_CARRIED, batch, leaves_open_partial, run_device_snap

pytestmark = pytest.mark.gpu

W = 1000                      # `within` of P3_APP, ms
COLD0 = 1 << 20               # cold keys are drawn at or above this id; scripted keys lie below
OR_APP = wl.S4_PART_APPS["or"].replace(") select", ") within 1 sec select")
assert OR_APP.count("within 1 sec") == 1


def check(qp, batches, monkeypatch, carried=P3_CARRIED, kind_end=1, min_carry=1, env=(("SHD_RESUME_MODE", "0"),)):
    ora = run_oracle(qp, batches)
    assert len(ora[2]) >= 1, "the shape yields no row"
    assert leaves_open_partial(batches), "the shape carries no partial"
    for k in ("SHD_RESUME_MODE", "SHD_NO_RESUME_LIST", "SHD_NO_SCAN_LISTS", "SHD_TS64", "SHD_LOCKSTEP"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SHD_FUSED_SORT", "1")
    for k, v in env:
        monkeypatch.setenv(k, v)
    monkeypatch.delenv("SHD_NO_LEAN_SORT", raising=False)
    monkeypatch.setenv("SHD_LEAN_SORT", "1")
    dev, c_lean, kind, s_lean = run_device_snap(qp, batches, carried)
    assert kind == kind_end
    assert_same_rows(dev, ora)
    monkeypatch.delenv("SHD_LEAN_SORT")
    monkeypatch.setenv("SHD_NO_LEAN_SORT", "1")
    dev2, c_full, kind2, s_full = run_device_snap(qp, batches, carried)
    assert kind2 == kind_end
    assert_same_rows(dev2, ora)
    for k in COUNTERS:
        assert c_lean[k] == c_full[k], k
    assert max(s.get("C", 0) for s in s_full) >= min_carry, "the shape carries no partial"
    for i, (a, b) in enumerate(zip(s_lean, s_full)):
        assert a.keys() == b.keys(), "push %d" % i
        for k in a:
            assert a[k] == b[k], "state after push %d: %s" % (i, k)
    return s_full


def cold(rng, n, t0, dt=0.25, p_cand=0.25):
    """n events of distinct keys, time-ordered from t0 (ms), one in four a candidate."""
    key = COLD0 + rng.choice(1 << 22, n, replace=False)
    u = rng.random(n)
    price = np.where(rng.random(n) < p_cand, 70.5 + 29.0 * u, 50.0 + 19.0 * u)
    ts = t0 + np.floor(np.arange(n) * dt).astype(np.int64)
    return key, price, ts


def put(push, row, key, price):
    push[0][row], push[1][row] = key, price


def pair(push, i, gap, key, p2=99.9):
    """Rows i and i + 4 * gap (0.25 ms a row, i a multiple of 4: exactly `gap` ms apart)
    become a candidate of `key` and a later event of it."""
    assert i % 4 == 0 and push[2][i + 4 * gap] - push[2][i] == gap
    put(push, i, key, 71.0)
    put(push, i + 4 * gap, key, p2)


def as_batch(push, nul=None):
    return batch(push[0], push[1], wl.T0 + push[2], nul=nul, call=4096)


def three_pushes(rng, gap):
    """9001 + 5003 + 3002 rows.  Push 1: pairs `gap` ms apart inside the push
    (undecided by the slice bounds) with a completing and a failing second
    event, starting inside a slice and on a slice's last rows; candidates in
    its last 100 ms whose key returns early in push 2 (inside and outside
    `within`), and cold candidates no later push touches.  Pushes 2 and 3 start
    on carried partials (not a multiple of 1024), so their slices are offset
    against their batch rows."""
    a = cold(rng, 9001, 0)
    pair(a, 400, gap, 11)
    pair(a, 1020, gap, 12, p2=60.0)        # candidate on a slice's last rows
    pair(a, 2048, gap, 13)                 # candidate on a slice's first row
    pair(a, 3000, gap - 1, 14)
    pair(a, 3100, gap + 1, 15, p2=60.0)
    pair(a, 4096, 3, 16)                   # close pair: a deferral that completes
    pair(a, 4200, 3, 17, p2=60.0)          # ... and one that stays open (pending list)
    t_end = int(a[2][-1])
    for n, key in enumerate((21, 22, 23, 24)):
        put(a, 9000 - 40 * n - 4, key, 71.0 + n)
    b = cold(rng, 5003, t_end + 700)
    put(b, 0, 21, 99.9)                    # 700 ms and a little after its candidate: completes
    put(b, 1, 22, 60.0)                    # inside `within`, f2 fails: pending
    put(b, 4 * 350, 23, 99.9)              # past `within` of its candidate: expires it
    put(b, 4 * 250, 24, 99.9)
    pair(b, 400, gap, 31)
    c = cold(rng, 3002, int(b[2][-1]) + 1)
    put(c, 7, 22, 99.9)                    # the pending partial expires or completes by its time
    put(c, 2000, 17, 99.9)
    return [as_batch(a), as_batch(b), as_batch(c)]


@pytest.mark.parametrize("gap", [W - 1, W, W + 1])
def test_lean_three_pushes_gaps_about_within(hip_available, monkeypatch, gap):
    qp, _ = compile_single_query(wl.P3_APP)
    snaps = check(qp, three_pushes(np.random.default_rng(40 + gap), gap), monkeypatch)
    assert snaps[0]["C"] % 1024 != 0 and snaps[1]["C"] % 1024 != 0


@pytest.mark.parametrize("gap", [W - 1, W, W + 1])
def test_lean_pair_across_a_slice_edge_at_the_bound(hip_available, monkeypatch, gap):
    """Rows 1023 and 1024 of the first push are one key's candidate and next
    event; the time jumps between them, so the candidate's slice ends and the
    successor's slice starts exactly `gap` ms apart: the slice bounds decide
    the pair at `within` + 1 and leave it to the exact times below."""
    rng = np.random.default_rng(50 + gap)
    a = cold(rng, 6001, 0)
    a[2][1024:] += gap - (a[2][1024] - a[2][1023])
    assert a[2][1024] - a[2][1023] == gap
    put(a, 1023, 41, 71.0)
    put(a, 1024, 41, 99.9)
    put(a, 2047, 42, 71.0)   # the same across the next edge, no jump: 0 ms apart
    put(a, 2048, 42, 99.9)
    b = cold(rng, 3001, int(a[2][-1]) + 5)
    qp, _ = compile_single_query(wl.P3_APP)
    check(qp, [as_batch(a), as_batch(b)], monkeypatch)


def test_lean_run_of_one_timestamp(hip_available, monkeypatch):
    """Rows 900 .. 3499 share one timestamp (two whole slices with tmin == tmax)."""
    rng = np.random.default_rng(61)
    a = cold(rng, 8001, 0)
    a[2][900:3500] = a[2][900]
    a[2][3500:] += 800 - (a[2][3500] - a[2][900])          # the run, then 800 ms later
    put(a, 1000, 51, 71.0)
    put(a, 3000, 51, 99.9)    # same time: completes
    put(a, 1100, 52, 71.0)
    put(a, 3600, 52, 99.9)    # 800 ms + a little: completes
    put(a, 1200, 53, 71.0)
    put(a, 3500 + 4 * 300, 53, 99.9)   # 1100 ms: expired
    b = cold(rng, 3001, int(a[2][-1]) + 5)
    qp, _ = compile_single_query(wl.P3_APP)
    check(qp, [as_batch(a), as_batch(b)], monkeypatch)


def test_lean_null_keys_and_a_dropped_row_as_successor(hip_available, monkeypatch):
    """A dropped (null-key) row sorts by its row index: row 2000 carries a null
    key, and key 2000 has a candidate before it and an event after it, so the
    candidate's successor in sorted order is the dropped row -- passed over,
    never taken for an event of the key."""
    rng = np.random.default_rng(62)
    a = cold(rng, 7001, 0)
    nul = (rng.random(7001) < 0.1).astype(np.uint8)
    nul[[1500, 2400, 6000]] = 0
    nul[2000] = 1
    put(a, 1500, 2000, 71.0)
    put(a, 2400, 2000, 99.9)          # 225 ms after the candidate: completes
    put(a, 6000, 2000, 60.0)
    b = cold(rng, 3001, int(a[2][-1]) + 5)
    nul_b = (rng.random(3001) < 0.1).astype(np.uint8)
    qp, _ = compile_single_query(wl.P3_APP)
    check(qp, [as_batch(a, nul), as_batch(b, nul_b)], monkeypatch)


def test_lean_or_form(hip_available, monkeypatch):
    qp, _ = compile_single_query(OR_APP)
    sym, price, vol, ts = wl.stock_stream(18_000, 4_000_000, 0.25, seed_offset=31)
    sym[8000], price[8000] = 7, 71.0
    sym[8012], price[8012] = 7, 60.0     # 3 ms later, below 0.9 * 71: the e3 branch
    sym[9000], price[9000] = 8, 71.0
    sym[9000 + 4 * (W + 1)], price[9000 + 4 * (W + 1)] = 8, 99.0   # expired
    cuts = [0, 9001, 14_004, 18_000]
    batches = [(0, stock_batch(sym[a:b], price[a:b], vol[a:b], ts[a:b])) for a, b in zip(cuts[:-1], cuts[1:])]
    check(qp, batches, monkeypatch, carried=OR_CARRIED)


def test_lean_push_ordered_per_key_only(hip_available, monkeypatch):
    """The cold rows' times are shuffled (every key once, so each key is in
    order); the scripted pairs keep theirs.  The slice tables assume no order."""
    rng = np.random.default_rng(63)
    a = cold(rng, 8001, 0)
    hot = [400, 400 + 4 * W, 1020, 1020 + 4 * (W + 1), 3000, 3012]
    keep = np.zeros(8001, bool)
    keep[hot] = True
    idx = np.flatnonzero(~keep)
    a[2][idx] = a[2][rng.permutation(idx)]
    for n, (i, j) in enumerate(zip(hot[::2], hot[1::2])):
        put(a, i, 71 + n, 71.0)
        put(a, j, 71 + n, 99.9)
    b = cold(rng, 3001, int(a[2].max()) + 5)
    qp, _ = compile_single_query(wl.P3_APP)
    check(qp, [as_batch(a), as_batch(b)], monkeypatch)


def test_lean_time_regression_hands_over(hip_available, monkeypatch):
    """Push 2 goes back in time inside a key: the generic NFA engine takes over
    from the carry of push 1, as after the three-word sort."""
    rng = np.random.default_rng(64)
    a = cold(rng, 5001, 0)
    pair(a, 400, 3, 81)
    put(a, 4000, 82, 71.0)
    b = cold(rng, 3001, int(a[2][-1]) + 5)
    put(b, 100, 82, 60.0)
    put(b, 10, 82, 60.0)
    b[2][10] += 100                      # key 82: the earlier row carries the later time
    put(b, 200, 81, 99.9)
    qp, _ = compile_single_query(wl.P3_APP)
    check(qp, [as_batch(a), as_batch(b)], monkeypatch, kind_end=4)


def dense_pushes(seed):
    """Three pushes over 300 keys, 0.25 ms a row: a partial expects a dozen events of its key inside `within`."""
    sym, price, vol, ts = wl.stock_stream(14_000, 300, 0.25, seed_offset=seed)
    cuts = [0, 6001, 10_004, 14_000]
    return [(0, stock_batch(sym[a:b], price[a:b], vol[a:b], ts[a:b])) for a, b in zip(cuts[:-1], cuts[1:])]


def test_lean_fallback_dense_keys(hip_available, monkeypatch):
    """Lean forced on dense keys: the push takes the capped lane walks, which
    read sorted times -- rebuilt from the rows (k_sorted_ts32)."""
    qp, _ = compile_single_query(wl.P3_APP)
    check(qp, dense_pushes(33), monkeypatch, env=())


def test_lean_fallback_ts64_knob(hip_available, monkeypatch):
    qp, _ = compile_single_query(wl.P3_APP)
    check(qp, three_pushes(np.random.default_rng(65), W), monkeypatch,
          env=(("SHD_RESUME_MODE", "0"), ("SHD_TS64", "1")))


def test_lean_fallback_offsets_past_int32(hip_available, monkeypatch):
    """Push 2 starts 2^31 + 5 ms after push 1 ended: the carried partials'
    offsets from its first event do not fit 32 bits (k_sorted_ts64)."""
    rng = np.random.default_rng(66)
    a = cold(rng, 5001, 0)
    pair(a, 400, 3, 91)
    put(a, 4000, 92, 71.0)
    b = cold(rng, 3001, int(a[2][-1]) + (1 << 31) + 5)
    put(b, 100, 92, 99.9)
    pair(b, 400, 3, 93)
    qp, _ = compile_single_query(wl.P3_APP)
    check(qp, [as_batch(a), as_batch(b)], monkeypatch)


def test_lean_by_the_device_estimate(hip_available, monkeypatch):
    """No forcing knob: k_ks_finish decides from each push's key density (a
    sparse push, then pushes on 300 hot keys), against SHD_NO_LEAN_SORT=1."""
    qp, _ = compile_single_query(wl.P3_APP)
    sparse = three_pushes(np.random.default_rng(67), W)[:1]
    batches = sparse + [(0, b) for _, b in dense_pushes(35)]
    t_shift = int(sparse[0][1].ts[-1]) + 5 - int(batches[1][1].ts[0])
    for _, b in batches[1:]:
        b.ts += t_shift
    ora = run_oracle(qp, batches)
    monkeypatch.setenv("SHD_FUSED_SORT", "1")
    for k in ("SHD_RESUME_MODE", "SHD_LEAN_SORT", "SHD_NO_LEAN_SORT"):
        monkeypatch.delenv(k, raising=False)
    dev, c_auto, kind, s_auto = run_device_snap(qp, batches, P3_CARRIED)
    assert_same_rows(dev, ora)
    monkeypatch.setenv("SHD_NO_LEAN_SORT", "1")
    dev2, c_full, kind2, s_full = run_device_snap(qp, batches, P3_CARRIED)
    assert_same_rows(dev2, ora)
    assert kind == kind2 == 1
    for k in COUNTERS:
        assert c_auto[k] == c_full[k], k
    assert s_auto == s_full
