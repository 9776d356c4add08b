"""Order of the pattern engine's push tail on the records path (the scan
emitted open / deferred records): the carry gather is queued right after the
totals' readback, before the host waits for them, with carry[nxt] reserved
for min(C + candidates, n_ext) rows; the match chain (k_emit_pairs, the pair
sort, k_project) follows the gather.  SHD_NO_SCAN_LISTS=1 takes the list
passes, whose tail keeps the earlier order (project, then gather, both after
the wait).

Every case compares the rows with the CPU oracle's and rows, walk counters
and the decoded state image after every push with the SHD_NO_SCAN_LISTS=1
run, under SHD_FUSED_SORT=1 and SHD_RESUME_MODE=0 (test sizes take the
flagship's path)."""
import numpy as np
import pytest

from parity import assert_same_rows, compile_single_query, concat_rows, run_oracle
from siddhi_amd import workloads as wl
from test_gpu_lean_sort import as_batch, cold, pair, put
from test_gpu_scan_lists import COUNTERS, P3_CARRIED, decode, run_device_snap

pytestmark = pytest.mark.gpu


def check2(qp, batches, monkeypatch, kind_end=1):
    ora = run_oracle(qp, batches)
    for k in ("SHD_NO_RESUME_LIST", "SHD_NO_SCAN_LISTS", "SHD_TS64", "SHD_LOCKSTEP", "SHD_SCAN_ROW_WALK",
              "SHD_NO_LEAN_SORT", "SHD_LEAN_SORT"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SHD_FUSED_SORT", "1")
    monkeypatch.setenv("SHD_RESUME_MODE", "0")
    dev, c_rec, kind, s_rec = run_device_snap(qp, batches, P3_CARRIED)
    assert kind == kind_end
    assert_same_rows(dev, ora)
    monkeypatch.setenv("SHD_NO_SCAN_LISTS", "1")
    dev2, c_list, kind2, s_list = run_device_snap(qp, batches, P3_CARRIED)
    monkeypatch.delenv("SHD_NO_SCAN_LISTS")
    assert kind2 == kind_end
    assert_same_rows(dev2, ora)
    for k in COUNTERS:
        assert c_rec[k] == c_list[k], k
    for i, (a, b) in enumerate(zip(s_rec, s_list)):
        assert a.keys() == b.keys(), "push %d" % i
        for k in a:
            assert a[k] == b[k], "state after push %d: %s" % (i, k)
    return ora, c_rec, s_rec


def no_candidates(rng, n, t0):
    a = cold(rng, n, t0)
    a[1][:] = 50.0 + 19.0 * rng.random(n)
    return a


def test_order_matches_and_no_open_partial(hip_available, monkeypatch):
    """Key 5: 71.0, then 99.9 (a match; the event opens a partial of its own),
    then a low event 2 s later that expires that partial.  No other candidate."""
    rng = np.random.default_rng(201)
    a = no_candidates(rng, 12_001, 0)            # 3 s
    put(a, 400, 5, 71.0)
    put(a, 440, 5, 99.9)
    put(a, 440 + 4 * 2000, 5, 60.0)
    b = no_candidates(rng, 2001, int(a[2][-1]) + 5)
    qp, _ = compile_single_query(wl.P3_APP)
    ora, c, snaps = check2(qp, [as_batch(a), as_batch(b)], monkeypatch)
    assert len(ora[2]) == 1 and c["matches"] == 1
    assert snaps[0]["C"] == 0 and snaps[1]["C"] == 0


def test_order_open_partials_and_no_match(hip_available, monkeypatch):
    rng = np.random.default_rng(202)
    a = cold(rng, 3001, 0)
    b = cold(rng, 2001, int(a[2][-1]) + 5)
    qp, _ = compile_single_query(wl.P3_APP)
    ora, c, snaps = check2(qp, [as_batch(a), as_batch(b)], monkeypatch)
    assert len(ora[2]) == 0 and c["matches"] == 0
    assert snaps[0]["C"] > 0 and snaps[1]["C"] > snaps[0]["C"]


def test_order_neither_match_nor_open_partial(hip_available, monkeypatch):
    rng = np.random.default_rng(203)
    a = no_candidates(rng, 3001, 0)
    b = no_candidates(rng, 2001, int(a[2][-1]) + 5)
    qp, _ = compile_single_query(wl.P3_APP)
    ora, c, snaps = check2(qp, [as_batch(a), as_batch(b)], monkeypatch)
    assert len(ora[2]) == 0 and c["partials"] == 0
    assert snaps[0]["C"] == 0 and snaps[1]["C"] == 0


@pytest.mark.parametrize("n", [700, 1025])
def test_order_every_candidate_stays_open(hip_available, monkeypatch, n):
    """Distinct keys, every event a candidate: after each push the carry holds
    every extended row -- n_open equals the bound the carry was reserved for."""
    rng = np.random.default_rng(204 + n)
    a = cold(rng, n, 0, p_cand=1.1)
    b = cold(rng, 333, int(a[2][-1]) + 5, p_cand=1.1)
    b[0][:] += 1 << 23                           # keys of push 1 do not return
    qp, _ = compile_single_query(wl.P3_APP)
    ora, c, snaps = check2(qp, [as_batch(a), as_batch(b)], monkeypatch)
    assert snaps[0]["C"] == n and snaps[1]["C"] == n + 333


def test_order_time_regression_after_a_carrying_push(hip_available, monkeypatch):
    """Push 2 goes back in time inside key 82 after push 1 carried partials:
    the gather of push 2 has run when the regression is read, and wrote the
    uncommitted table only -- the hand-over replays push 1's carry.  The
    snapshot taken before the failing push restores into a fresh query and
    replays the push to the same rows."""
    from siddhi_amd.hip_engine import DeviceQuery, SHD_MEM_HOST
    rng = np.random.default_rng(205)
    a = cold(rng, 3001, 0)
    pair(a, 400, 3, 81)
    put(a, 2800, 82, 71.0)
    put(a, 2900, 83, 71.0)
    b = cold(rng, 2001, int(a[2][-1]) + 5)
    put(b, 10, 82, 71.0)
    put(b, 100, 82, 60.0)
    b[2][10] += 100                              # key 82: the earlier row carries the later time
    put(b, 200, 83, 99.9)                        # completes a carried partial after the hand-over
    batches = [as_batch(a), as_batch(b)]
    qp, _ = compile_single_query(wl.P3_APP)
    ora, c, snaps = check2(qp, batches, monkeypatch, kind_end=4)
    assert snaps[0]["C"] > 0 and len(ora[2]) >= 2

    def push(dq, item):
        si, bt = item
        cols = [np.ascontiguousarray(x) for x in bt.cols]
        ts = np.ascontiguousarray(bt.ts, np.int64)
        dq.push_raw(si, bt.n, ts.ctypes.data, [x.ctypes.data for x in cols], [0] * len(cols), SHD_MEM_HOST,
                    bt.call_offsets if len(bt.call_offsets) > 2 else None, True)
        r = dq.poll()
        return [] if r is None else [r]

    dq, dq2 = DeviceQuery(qp.ir), DeviceQuery(qp.ir)
    try:
        parts = push(dq, batches[0])
        image = dq.snapshot()
        assert decode(image, P3_CARRIED)["C"] == snaps[0]["C"]
        first = concat_rows(parts + push(dq, batches[1]))
        assert dq.engine_kind == 4
        dq2.restore(image)
        again = concat_rows(parts + push(dq2, batches[1]))
        assert dq2.engine_kind == 4
    finally:
        dq.close()
        dq2.close()
    assert_same_rows(first, ora)
    assert_same_rows(again, ora)
