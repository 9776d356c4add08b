// engine_window.hip -- keyed exact window engine ("window-x").
//
// Single-stream queries the segmented-scan engine (engine_single.hip) does
// not take: windows whose selector emits EXPIRED events (`insert all events` /
// `insert expired events`), and window / aggregate queries inside a
// `partition with (...)` block.  Reference semantics
// (modules/siddhi-core/src/main/java/io/siddhi/core/):
//   query/processor/stream/window/LengthWindowProcessor.java:105-142
//   query/processor/stream/window/TimeWindowProcessor.java:132-169 (+ state :196-222)
//   util/Scheduler.java:71-104,113-209 (TIMER events in playback: onTimeChange)
//   query/selector/QuerySelector.java:76-99 (process), :161-205 (processNoGroupBy),
//     :271-313 (processInBatchNoGroupBy), :315-373 (processInBatchGroupBy)
//   query/selector/attribute/aggregator/{Sum,Avg,Count}AttributeAggregatorExecutor.java
//   query/selector/attribute/aggregator/{Max,Min,MaxForever,MinForever}AttributeAggregatorExecutor.java
//     (every plan with one of these runs here: k_xw_fold<true> and the list store)
//   query/selector/attribute/aggregator/{StdDev,DistinctCount,And,Or}AttributeAggregatorExecutor.java
//     (k_xw_fold<true, true>; distinctCount keeps its keys in the list store)
//   partition/PartitionStreamReceiver.java:175-216 (same-key runs = chunks)
//   util/snapshot/state/PartitionStateHolder.java:43-69 (state per (partition key,
//     group key); a window state is dropped when its queue empties)
//
// Formulation: every window item (a filtered, keyed event) lives in its
// partition key's FIFO.  Items of a push -- the carried FIFOs first, then the
// new items in arrival order -- are stable-sorted by partition key, so each key
// is one contiguous segment in FIFO order.  Each item gets its EXPIRY
// OPPORTUNITY: the add of a later item of its key (length: the L-th next item;
// time: the first later item whose call clock reaches ts + T) or a TIMER of its
// key at a time change; FIFO order makes the opportunities non-decreasing along
// a segment.  The reference's operation stream of one key -- at each
// opportunity its expirations (FIFO), then the add -- then has a closed-form
// position for every operation (counting by binary search inside the segment),
// so all operations of the push are written in key-major order in one pass.
// Aggregator states (dense ids of (partition key, group key), device group
// dictionary) are folded SEQUENTIALLY in that order (bit-exact add / remove,
// agg.h); output rows are the selector's per-chunk picks, ordered by (chunk,
// position) with a radix sort.
//
// Time windows with expired output need the Scheduler's TIMER events: a key's
// notify queue holds ts + T of every item that raised the key's last time
// (state.lastTimestamp); at a time change to `now` every key whose queue head
// is <= now gets one TIMER chunk that expires its FIFO prefix with ts + T <= now
// (emitted as its own callback chunk, before the call's events).  That part is
// inherently sequential per key: one lane per key segment walks its items and
// the push's clock moves (k_xw_time_lane); everything else is data-parallel.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <deque>
#include <cstdlib>

#include "engine.h"
#include "gdict.h"
#include "agg.h"
#include "stream_kernels.h"
#include "window_items.h"

namespace shd {

namespace {

constexpr uint64_t kNoOpp = ~0ull;        // item does not expire in this push
constexpr uint32_t kNoTimer = 0xFFFFFFFFu;

// ---------------------------------------------------------------- contexts
// A window item (attributes as 64-bit payloads) with the row's timestamp and
// aggregator values: selector outputs and `having`.
struct ItemCtx {
  const uint64_t* attr;   // [ncols][cap]
  const uint8_t* nul;
  int64_t cap;
  int64_t item;
  int ncols;
  int64_t tsv;            // the output event's timestamp (EXPIRED: the expiry time)
  const uint64_t* aggv;
  const uint8_t* aggn;
  __device__ __forceinline__ Val load(int, int, int a) const {
    if ((unsigned)a >= (unsigned)ncols) return Val{0, 1};
    return Val{attr[(int64_t)a * cap + item], (int)nul[(int64_t)a * cap + item]};
  }
  __device__ __forceinline__ bool evnull(int, int) const { return false; }
  __device__ __forceinline__ int64_t ts(int, int) const { return tsv; }
  __device__ __forceinline__ Val agg(int i) const { return Val{aggv[i], (int)aggn[i]}; }
};

// ---------------------------------------------------------------- searches
// First index of [lo, hi) at which pred is false (pred holds on a prefix).
template <class I, class P>
__device__ __forceinline__ I first_false(I lo, I hi, P pred) {
  while (lo < hi) {
    const I mid = (lo + hi) >> 1;
    if (pred(mid)) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}
// Ascending a[lo, hi): the first index with a[i] >= v (lower) / a[i] > v (upper).
template <class T, class I>
__device__ __forceinline__ I lower_bound(const T* a, I lo, I hi, T v) {
  return first_false(lo, hi, [=](I i) { return a[i] < v; });
}
template <class T, class I>
__device__ __forceinline__ I upper_bound(const T* a, I lo, I hi, T v) {
  return first_false(lo, hi, [=](I i) { return a[i] <= v; });
}


// ---------------------------------------------------------------- segments
// segS[k] = first sorted position of segment k; segid[j]
__global__ __launch_bounds__(kBlock) void k_xw_seg_list(const uint32_t* head, const uint32_t* hscan, int64_t total,
                                                        int64_t* segS, uint32_t* segid) {
  for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < total; j = total) {
    const uint32_t k = hscan[j] + head[j] - 1;
    segid[j] = k;
    if (head[j]) segS[k] = j;
    if (j == total - 1) segS[k + 1] = total;
  }
}

// inclusive partition-run id of every keyed event, in place over the starts
__global__ __launch_bounds__(kBlock) void k_xw_run_ids(int64_t n, const uint32_t* run_excl, uint32_t* start_to_id) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i = n)
    start_to_id[i] = run_excl[i] + start_to_id[i] - 1u;
}

__global__ __launch_bounds__(kBlock) void k_xw_widen(const uint8_t* f, int64_t n, uint32_t* out) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i = n) out[i] = f[i];
}

// Per segment: carried items at its front (ck), its pending notify entries
// [pA, pB) (pending keys sorted), the output room of its pending entries.
__global__ __launch_bounds__(kBlock) void k_xw_seg_info(int64_t nseg, const int64_t* segS, const uint32_t* sp,
                                                        int64_t C, const uint64_t* ipk, const uint64_t* ppk, int64_t np,
                                                        int64_t* segCk, int64_t* pA, int64_t* pB, uint32_t* proom) {
  for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < nseg; k = nseg) {
    const int64_t s = segS[k], e = segS[k + 1];
    const int64_t lo = lower_bound(sp, s, e, (uint32_t)C);   // first position holding a new item
    segCk[k] = lo - s;
    const uint64_t pk = ipk[sp[s]];
    const int64_t a = lower_bound(ppk, (int64_t)0, np, pk);
    const int64_t c = upper_bound(ppk, a, np, pk);
    pA[k] = a;
    pB[k] = c;
    proom[k] = (uint32_t)((c - a) + (e - s - (lo - s)));
  }
}

// ---------------------------------------------------------------- expiry
// length(L): item at segment rank r leaves at the add of rank r + L
// (LengthWindowProcessor :105-142; a carried FIFO holds at most L items).
__global__ __launch_bounds__(kBlock) void k_xw_len_expiry(int64_t total, int64_t L, const int64_t* segS,
                                                          const uint32_t* segid, const uint32_t* sp,
                                                          const int32_t* irow, uint64_t* eopp, uint32_t* etid) {
  for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < total; j = total) {
    const int64_t e = segS[segid[j] + 1];
    uint64_t o = kNoOpp;
    if (j + L < e) o = 2ull * (uint64_t)irow[sp[j + L]] + 1ull;
    eopp[j] = o;
    etid[j] = kNoTimer;
  }
}

struct LaneArgs {
  int64_t nseg;
  const int64_t* segS;
  const int64_t* segCk;
  const int64_t* pA;
  const int64_t* pB;
  const uint32_t* proom_off;   // exclusive scan of the per-segment pending room
  const uint32_t* sp;
  const uint64_t* ipk;
  const int64_t* its;
  const int32_t* icall;
  const int32_t* irow;
  const int64_t* ilast;
  const int64_t* call_now;
  const int64_t* offs;
  const int32_t* F;            // firing calls (clock moves), ascending
  const int64_t* fnow;
  int nf;
  int64_t T;
  int64_t L;                   // timeLength: the length bound (0: time window)
  int ext_col;                 // externalTime: the item attribute holding its time (-1: the clock)
  const uint64_t* iattr;       // [ncols][cap]
  int64_t cap;
  int partitioned;
  int64_t last_global;         // unpartitioned: the window's lastTimestamp
  const int64_t* pv;           // pending notify values (sorted by key, then value)
  // outputs
  uint64_t* eopp;
  uint32_t* etid;
  uint8_t* rec;
  unsigned int* ntimer;
  int32_t* tF;
  int64_t* tHead;
  uint32_t* tSeg;
  uint64_t* pout_pk;
  int64_t* pout_v;
  uint32_t* pcnt;
  int64_t* last_out;
};

// One lane per key segment: TimeWindowProcessor.process over the key's items
// in arrival order, interleaved with the push's clock moves (Scheduler
// onTimeChange -> sendTimerEvents for the key when its notify head <= now).
__global__ __launch_bounds__(kBlock) void k_xw_time_lane(const LaneArgs* __restrict__ ap) {
  const LaneArgs& a = *ap;
  for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < a.nseg; k = a.nseg) {
    const int64_t s = a.segS[k], e = a.segS[k + 1], ck = a.segCk[k];
    const int64_t pB = a.pB[k];
    int64_t pc = a.pA[k];
    const uint64_t pk = a.ipk[a.sp[s]];
    int64_t lastTs = a.partitioned ? (ck > 0 ? a.ilast[a.sp[s]] : INT64_MIN) : a.last_global;
    int64_t h = s;          // FIFO head
    int64_t rnext = -1;     // oldest unconsumed new notify entry (a record position)
    int fi = 0;
    for (int64_t j = s; j < s + ck; j++) a.rec[j] = 0;
    for (int64_t y = s + ck;; y++) {
      const int32_t cy = y < e ? a.icall[a.sp[y]] : 0x7FFFFFFF;
      // clock moves before item y (its call's setCurrentTimestamp comes first)
      while (fi < a.nf && a.F[fi] <= cy) {
        const int fe = upper_bound(a.F, fi, a.nf, cy);
        int64_t hv;
        if (pc < pB) hv = a.pv[pc];
        else if (rnext >= 0) hv = a.its[a.sp[rnext]] + a.T;
        else {
          fi = fe;
          break;
        }
        const int lo = lower_bound(a.fnow, fi, fe, hv);   // first clock move reaching the head
        if (lo == fe) {
          fi = fe;
          break;
        }
        const int32_t f = a.F[lo];
        const int64_t nowf = a.fnow[lo];
        // sendTimerEvents: the notify queue (a FIFO, Scheduler.SchedulerState
        // toNotifyQueue) is polled while its head is <= now
        while (pc < pB && a.pv[pc] <= nowf) pc++;
        while (pc == pB && rnext >= 0 && a.its[a.sp[rnext]] + a.T <= nowf) {
          a.rec[rnext] = 2;
          int64_t q = rnext + 1;
          while (q < y && a.rec[q] != 1) q++;
          rnext = q < y ? q : -1;
        }
        const uint32_t tid = atomicAdd(a.ntimer, 1u);
        a.tF[tid] = f;
        a.tHead[tid] = hv;
        a.tSeg[tid] = (uint32_t)k;
        // the TIMER chunk: FIFO prefix with ts - now + T <= 0 (:141-151)
        const uint64_t o = 2ull * (uint64_t)a.offs[f];
        while (h < y && a.its[a.sp[h]] + a.T <= nowf) {
          a.eopp[h] = o;
          a.etid[h] = tid;
          h++;
        }
        // PartitionStateHolder.returnState: an empty window state is dropped
        if (a.partitioned && h == y) lastTs = INT64_MIN;
        fi = lo + 1;
      }
      if (y >= e) break;
      // externalTime (ExternalTimeWindowProcessor.java:128-149): each event's
      // own time attribute is the clock, items expire by theirs
      const int64_t nowy = a.ext_col >= 0 ? (int64_t)a.iattr[(int64_t)a.ext_col * a.cap + a.sp[y]] : a.call_now[cy];
      const uint64_t oy = 2ull * (uint64_t)a.irow[a.sp[y]] + 1ull;
      while (h < y && (a.ext_col >= 0 ? (int64_t)a.iattr[(int64_t)a.ext_col * a.cap + a.sp[h]] : a.its[a.sp[h]]) + a.T <=
                          nowy) {
        a.eopp[h] = oy;
        a.etid[h] = kNoTimer;
        h++;
      }
      // timeLength (TimeLengthWindowProcessor.java:160-178): a full window
      // gives up its head to the add
      if (a.L > 0 && y - h >= a.L) {
        a.eopp[h] = oy;
        a.etid[h] = kNoTimer;
        h++;
      }
      const int64_t tsy = a.its[a.sp[y]];
      // scheduler.notifyAt(ts + T): the time window when its lastTimestamp
      // rises (TimeWindowProcessor :156-159), timeLength for every add (:177)
      if (a.ext_col < 0 && (a.L > 0 || lastTs < tsy)) {
        a.rec[y] = 1;
        lastTs = tsy;
        if (rnext < 0) rnext = y;
      } else {
        a.rec[y] = 0;
      }
    }
    for (int64_t j = h; j < e; j++) {
      a.eopp[j] = kNoOpp;
      a.etid[j] = kNoTimer;
    }
    // notify entries still queued for the next push
    const int64_t o0 = a.proom_off[k];
    int64_t c = 0;
    for (; pc < pB; pc++, c++) {
      a.pout_pk[o0 + c] = pk;
      a.pout_v[o0 + c] = a.pv[pc];
    }
    if (rnext >= 0)
      for (int64_t j = rnext; j < e; j++)
        if (a.rec[j] == 1) {
          a.pout_pk[o0 + c] = pk;
          a.pout_v[o0 + c] = a.its[a.sp[j]] + a.T;
          c++;
        }
    a.pcnt[k] = (uint32_t)c;
    a.last_out[k] = lastTs;
  }
}

// Pending entries of keys without items: a clock move of the push reaching
// them consumes them (their TIMER chunk finds an empty window: no rows).
__global__ __launch_bounds__(kBlock) void k_xw_orphans(int64_t np, const uint64_t* ppk, const int64_t* pv,
                                                       int64_t nseg, const uint64_t* seg_pk, int nf,
                                                       const int64_t* fnow, uint32_t* keep) {
  for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < np; p = np) {
    const int64_t lo = lower_bound(seg_pk, (int64_t)0, nseg, ppk[p]);
    const bool has_seg = lo < nseg && seg_pk[lo] == ppk[p];
    // the key's FIFO is polled while its head <= now: entry p is gone when it
    // and every earlier entry of its key are <= the push's last clock
    bool consumed = nf > 0 && fnow[nf - 1] >= pv[p];
    for (int64_t q = p - 1; consumed && q >= 0 && ppk[q] == ppk[p]; q--) consumed = fnow[nf - 1] >= pv[q];
    keep[p] = (!has_seg && !consumed) ? 1u : 0u;
  }
}

__global__ __launch_bounds__(kBlock) void k_xw_seg_pk(int64_t nseg, const int64_t* segS, const uint32_t* sp,
                                                      const uint64_t* ipk, uint64_t* seg_pk) {
  for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < nseg; k = nseg) seg_pk[k] = ipk[sp[segS[k]]];
}

// ---------------------------------------------------------------- operations
__global__ __launch_bounds__(kBlock) void k_xw_nops(int64_t total, int64_t C, const uint32_t* sp,
                                                    const uint64_t* eopp, uint32_t* nops) {
  for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < total; j = total)
    nops[j] = (sp[j] >= (uint32_t)C ? 1u : 0u) + (eopp[j] != kNoOpp ? 1u : 0u);
}

struct OpArgs {
  int64_t total, C;
  const uint32_t* sp;
  const uint32_t* segid;
  const int64_t* segS;
  const int64_t* segCk;
  const uint64_t* eopp;
  const uint32_t* etid;
  const uint32_t* opscan;     // exclusive scan of k_xw_nops
  const int32_t* irow;
  const int64_t* iseq;
  const int32_t* call_of;     // per batch row
  const int64_t* call_now;    // per call
  const uint32_t* run_of;     // per batch row: partition run id (partitioned)
  const int64_t* offs;
  const int64_t* fnow_of_call;   // per call: clock after its move (timers)
  const uint32_t* trank;      // timer id -> rank in (call, head, key) order
  const int32_t* sF;          // sorted timers' calls
  int64_t nt;
  const uint64_t* runs_before;   // per call: partition runs in earlier calls
  const int64_t* row_now;     // externalTime: per batch row its time attribute (null: the call's clock)
  int partitioned;
  int current_on, expired_on;
  int64_t seq0;
  // outputs [nops]
  uint32_t* op_item;
  uint8_t* op_add;
  uint8_t* op_on;
  uint32_t* op_chunk;         // chunk ordinal of the push
  int64_t* op_now;            // EXPIRED rows: the expiry time (currentTime)
  int64_t* op_seq;            // shd_out.in_seq of a row emitted at this op
};

// chunk ordinal of an item opportunity at batch row r: the event chunks (calls
// or partition runs) and timer chunks interleave per call, timers first
__device__ __forceinline__ uint32_t event_ordinal(const OpArgs& a, int64_t r) {
  const int32_t c = a.call_of[r];
  const int64_t ev = a.partitioned ? (int64_t)a.run_of[r] : (int64_t)c;
  return (uint32_t)(ev + upper_bound(a.sF, (int64_t)0, a.nt, c));
}

__global__ __launch_bounds__(kBlock) void k_xw_ops(const OpArgs* __restrict__ ap) {
  const OpArgs& a = *ap;
  for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < a.total; j = a.total) {
    const uint32_t k = a.segid[j];
    const int64_t s = a.segS[k], e = a.segS[k + 1], ck = a.segCk[k];
    const int64_t base = a.opscan[s];
    const uint32_t it = a.sp[j];
    if (it >= (uint32_t)a.C) {   // the add (CURRENT) of a new item
      const int64_t r = a.irow[it];
      const uint64_t oy = 2ull * (uint64_t)r + 1ull;
      const int64_t lo = upper_bound(a.eopp, s, j, oy);   // expirations of this key at or before the opportunity
      const int64_t q = base + (j - s - ck) + (lo - s);
      a.op_item[q] = it;
      a.op_add[q] = 1;
      a.op_on[q] = (uint8_t)a.current_on;
      a.op_chunk[q] = event_ordinal(a, r);
      a.op_now[q] = a.call_now[a.call_of[r]];
      a.op_seq[q] = a.iseq[it];
    }
    const uint64_t o = a.eopp[j];
    if (o != kNoOpp) {           // the EXPIRED event of item j
      // adds of this key before the opportunity
      const int64_t lo = first_false(s + ck, e, [&](int64_t i) { return 2ull * (uint64_t)a.irow[a.sp[i]] + 1ull < o; });
      const int64_t q = base + (j - s) + (lo - s - ck);
      a.op_item[q] = it;
      a.op_add[q] = 0;
      a.op_on[q] = (uint8_t)a.expired_on;
      const uint32_t tid = a.etid[j];
      if (tid == kNoTimer) {
        const int64_t r = (int64_t)((o - 1) >> 1);
        a.op_chunk[q] = event_ordinal(a, r);
        a.op_now[q] = a.row_now ? a.row_now[r] : a.call_now[a.call_of[r]];
        a.op_seq[q] = a.seq0 + r;
      } else {
        const uint32_t t = a.trank[tid];
        const int32_t f = a.sF[t];
        const int64_t ev = a.partitioned ? (int64_t)a.runs_before[f] : (int64_t)f;
        a.op_chunk[q] = (uint32_t)(t + ev);
        a.op_now[q] = a.fnow_of_call[f];
        a.op_seq[q] = a.seq0 + a.offs[f];
      }
    }
  }
}

// runs_before[c]: partition runs that start in calls before c
__global__ __launch_bounds__(kBlock) void k_xw_runs_before(int ncalls, const int64_t* offs, int64_t n,
                                                           const uint32_t* run_excl, uint64_t total_runs,
                                                           uint64_t* out) {
  for (int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x; c < ncalls; c = ncalls) {
    const int64_t r = offs[c];
    out[c] = r < n ? (uint64_t)run_excl[r] : total_runs;
  }
}

// ---------------------------------------------------------------- selector
struct FoldArgsX {
  int nagg;
  int kind[kMaxAggs];
  int type[kMaxAggs];
  int group;          // processInBatchGroupBy: row at the first pick, values of the last
  int64_t cap, nops, nstates;
  const uint64_t* argv;
  const uint8_t* argn;
  const uint32_t* op_item;
  const uint8_t* op_add;
  const uint8_t* op_on;
  const uint32_t* op_chunk;
  const int64_t* op_now;
  const int64_t* its;
  const uint64_t* attr;
  const uint8_t* nul;
  int ncols;
  DExprSet es;
  int has_having;
  DExpr having;
  double* dsum;
  int64_t* lsum;
  int64_t* cnt;
  // batch windows: the chunk of a state's last RESET-started add (RESET clears
  // every group state of the partition; applied when the state is next added to)
  int64_t* epoch;     // [nstates], null: no batch window
  const int64_t* op_epoch;   // per add: the RESET epoch it folds in
  uint64_t* resv;     // [nagg][nops]
  uint8_t* resn;
  uint8_t* rowflag;   // [nops]
  uint32_t* rowsrc;
  // min / max states keep their value in lsum and their flags in cnt (agg.h
  // mm_step).  Tracking deques: dq[g] = the deque row of aggregator g (-1:
  // none).  Carried deques: row d, state s holds dq_len[d * nstates + s]
  // values at dq_val + dq_off[...]; during the fold each lane owns the region
  // dq_work + dq_woff[lane * ndq + d] and leaves the length and the place of
  // what is left in dq_nlen / dq_nsrc (kDqWork: in the work area).
  int ndq;
  int dq[kMaxAggs];
  const uint32_t* dq_len;
  const uint32_t* dq_off;
  const uint64_t* dq_val;
  const uint32_t* dq_woff;
  uint64_t* dq_work;
  uint32_t* dq_nlen;
  uint32_t* dq_nsrc;
  // The same store holds distinctCount's keys, (key bits, count) pairs sorted
  // by key (agg.h dc_step): dq_esz[d] = words an add can append to row d (1 a
  // deque value, 2 a pair).  stdDev / and / or keep the three scalars only.
  int dq_esz[kMaxAggs];
};
constexpr uint32_t kDqWork = 0x80000000u;

// Aggregated value of one aggregator after a step (avg divided here).
__device__ __forceinline__ void agg_value(int kind, uint64_t ob, bool on, int64_t c, uint64_t& v, uint8_t& vn) {
  v = ob;
  vn = (uint8_t)on;
  if (kind == SHD_AGG_AVG && !on) v = p_f64(__ddiv_rn(v_f64(ob), (double)c));
}

// One lane per aggregator state (a (partition key, group key) pair): the
// state's operations in the reference's order.  The selector's pick per chunk
// is tracked on the fly: a run = the state's consecutive operations of one
// chunk; its first and last selected ("on") operations decide the row.
// MM: the plan has min / max aggregators (the plain instance is the kernel
// the sum / avg / count plans have always run).  XA: it has stdDev /
// distinctCount / and / or (k_xw_fold<true, true>: MM is set with it).
template <bool MM, bool XA = false>
__global__ __launch_bounds__(kBlock) void k_xw_fold(const FoldArgsX* __restrict__ ap, const uint32_t* heads,
                                                    int64_t nheads, const uint32_t* ssid, const uint32_t* sq) {
  const FoldArgsX& a = *ap;
  for (int64_t hh = (int64_t)blockIdx.x * kBlock + threadIdx.x; hh < nheads; hh = nheads) {
    const int64_t q0 = heads[hh];
    const int64_t q1 = hh + 1 < nheads ? (int64_t)heads[hh + 1] : a.nops;
    const uint32_t sid = ssid[q0];
    double d[kMaxAggs];
    int64_t l[kMaxAggs], c[kMaxAggs];
    for (int g = 0; g < a.nagg; g++) {
      d[g] = a.dsum[(int64_t)g * a.nstates + sid];
      l[g] = a.lsum[(int64_t)g * a.nstates + sid];
      c[g] = a.cnt[(int64_t)g * a.nstates + sid];
    }
    MmDeque dq[MM ? kMaxAggs : 1];
    if constexpr (MM) {
      // the carried deques move to the front of the lane's regions
      for (int k = 0; k < a.ndq; k++) {
        const int64_t cell = (int64_t)k * a.nstates + sid;
        const int64_t n0 = a.dq_len[cell];
        const uint64_t* src = a.dq_val + a.dq_off[cell];
        dq[k].w = a.dq_work + a.dq_woff[hh * a.ndq + k];
        dq[k].h = 0;
        dq[k].t = n0;
        dq[k].room = n0 + (q1 - q0) * (XA ? a.dq_esz[k] : 1);
        for (int64_t i = 0; i < n0; i++) dq[k].w[i] = src[i];
      }
    }
    int64_t ep = a.epoch ? a.epoch[sid] : 0;
    uint32_t cur = 0xFFFFFFFFu;
    int64_t first = -1, last = -1;
    for (int64_t p = q0; p < q1; p++) {
      const uint32_t q = sq[p];
      const uint32_t it = a.op_item[q];
      const bool add = a.op_add[q];
      if (a.epoch && add && ep != a.op_epoch[q]) {
        // a RESET came after this state's last operation
        ep = a.op_epoch[q];
        for (int g = 0; g < a.nagg; g++) {
          if constexpr (MM) {
            // reset(): min / max clear value and deque, the Forever kinds keep theirs;
            // stdDev / distinctCount / and / or clear everything, the key list too
            if (a.kind[g] == SHD_AGG_MAX_FOREVER || a.kind[g] == SHD_AGG_MIN_FOREVER) continue;
            if (a.dq[g] >= 0) dq[a.dq[g]].h = dq[a.dq[g]].t;
          }
          d[g] = 0.0;
          l[g] = 0;
          c[g] = 0;
        }
      }
      uint64_t vv[kMaxAggs];
      uint8_t vn[kMaxAggs];
      for (int g = 0; g < a.nagg; g++) {
        uint64_t ob;
        bool on;
        const uint64_t xb = a.argv[(int64_t)g * a.cap + it];
        const bool xn = a.argn[(int64_t)g * a.cap + it] != 0;
        if (XA && agg_is_ext(a.kind[g])) {
          ext_step(a.kind[g], a.type[g], add, xb, xn, d[g], l[g], c[g], a.dq[g] >= 0 ? &dq[a.dq[g]] : nullptr, ob, on);
        } else if (MM && agg_is_minmax(a.kind[g])) {
          uint64_t v = (uint64_t)l[g];
          mm_step(a.kind[g], a.type[g], add, xb, xn, v, c[g], a.dq[g] >= 0 ? &dq[a.dq[g]] : nullptr, ob, on);
          l[g] = (int64_t)v;
        } else {
          agg_step(a.kind[g], a.type[g], add, xb, xn, d[g], l[g], c[g], ob, on);
        }
        agg_value(a.kind[g], ob, on, c[g], vv[g], vn[g]);
      }
      bool sel = a.op_on[q] != 0;
      if (sel && a.has_having) {
        ItemCtx cx{a.attr, a.nul, a.cap, (int64_t)it, a.ncols, add ? a.its[it] : a.op_now[q], vv, vn};
        sel = eval_bool(a.es.ins + a.having.off, a.having.len, a.es.consts, cx);
      }
      if (!sel) continue;
      for (int g = 0; g < a.nagg; g++) {
        a.resv[(int64_t)g * a.nops + q] = vv[g];
        a.resn[(int64_t)g * a.nops + q] = vn[g];
      }
      const uint32_t ch = a.op_chunk[q];
      if (ch != cur) {
        if (first >= 0) {
          const int64_t at = a.group ? first : last;
          a.rowflag[at] = 1;
          a.rowsrc[at] = (uint32_t)last;
        }
        cur = ch;
        first = q;
      }
      last = q;
    }
    if (first >= 0) {
      const int64_t at = a.group ? first : last;
      a.rowflag[at] = 1;
      a.rowsrc[at] = (uint32_t)last;
    }
    for (int g = 0; g < a.nagg; g++) {
      a.dsum[(int64_t)g * a.nstates + sid] = d[g];
      a.lsum[(int64_t)g * a.nstates + sid] = l[g];
      a.cnt[(int64_t)g * a.nstates + sid] = c[g];
    }
    if (a.epoch) a.epoch[sid] = ep;
    if constexpr (MM) {
      for (int k = 0; k < a.ndq; k++) {
        const int64_t cell = (int64_t)k * a.nstates + sid;
        a.dq_nlen[cell] = (uint32_t)(dq[k].t - dq[k].h);
        a.dq_nsrc[cell] = (a.dq_woff[hh * a.ndq + k] + (uint32_t)dq[k].h) | kDqWork;
      }
    }
  }
}

// Room of each lane's list regions: the carried list plus, per operation of
// the state in this push, what an add can append (esz: one deque value, or one
// (key, count) pair).
struct DqEsz {
  int v[kMaxAggs];
};
__global__ __launch_bounds__(kBlock) void k_xw_dq_room(const uint32_t* heads, int64_t nheads, int64_t nops,
                                                       const uint32_t* ssid, int ndq, DqEsz esz, int64_t nstates,
                                                       const uint32_t* dq_len, uint32_t* room) {
  for (int64_t hh = (int64_t)blockIdx.x * kBlock + threadIdx.x; hh < nheads; hh = nheads) {
    const int64_t q0 = heads[hh];
    const int64_t q1 = hh + 1 < nheads ? (int64_t)heads[hh + 1] : nops;
    const uint32_t sid = ssid[q0];
    for (int k = 0; k < ndq; k++)
      room[hh * ndq + k] = dq_len[(int64_t)k * nstates + sid] + (uint32_t)(q1 - q0) * (uint32_t)esz.v[k];
  }
}

// The deques after the fold, packed into the other slot of the store: value e
// of the new store belongs to the last cell whose offset is <= e (empty cells
// share their successor's offset); its source is the work area for the states
// this push folded, the old store for the rest.
__global__ __launch_bounds__(kBlock) void k_xw_dq_pack(int64_t total, int64_t ncell, const uint32_t* noff,
                                                       const uint32_t* nsrc, const uint64_t* old_val,
                                                       const uint64_t* work, uint64_t* dst) {
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e = total) {
    const int64_t cell = upper_bound(noff, (int64_t)0, ncell, (uint32_t)e) - 1;
    const uint32_t src = nsrc[cell];
    const int64_t i = e - noff[cell];
    dst[e] = (src & kDqWork) ? work[(src & ~kDqWork) + i] : old_val[src + i];
  }
}

// processNoGroupBy: every selected operation is a row.
__global__ __launch_bounds__(kBlock) void k_xw_plain_rows(const FoldArgsX* __restrict__ ap) {
  const FoldArgsX& a = *ap;
  for (int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x; q < a.nops; q = a.nops) {
    bool sel = a.op_on[q] != 0;
    if (sel && a.has_having) {
      const uint32_t it = a.op_item[q];
      ItemCtx cx{a.attr, a.nul, a.cap, (int64_t)it, a.ncols, a.op_add[q] ? a.its[it] : a.op_now[q], nullptr, nullptr};
      sel = eval_bool(a.es.ins + a.having.off, a.having.len, a.es.consts, cx);
    }
    a.rowflag[q] = sel ? 1 : 0;
    a.rowsrc[q] = (uint32_t)q;
  }
}

__global__ __launch_bounds__(kBlock) void k_xw_row_keys(int64_t nops, const uint8_t* rowflag, const uint32_t* roff,
                                                        const uint32_t* op_chunk, uint64_t* rkey, uint32_t* rq) {
  for (int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x; q < nops; q = nops) {
    if (!rowflag[q]) continue;
    rkey[roff[q]] = ((uint64_t)op_chunk[q] << 32) | (uint64_t)q;
    rq[roff[q]] = (uint32_t)q;
  }
}

struct EmitArgsX {
  DExprSet es;
  DExpr outs[kMaxCols];
  int nout, nagg, ncols;
  int64_t cap, nops, row0, chunk0;
  const uint32_t* rowsrc;
  const uint32_t* op_item;
  const uint8_t* op_add;
  const uint32_t* op_chunk;
  const int64_t* op_now;
  const int64_t* op_seq;
  const int64_t* its;
  const uint64_t* attr;
  const uint8_t* nul;
  const uint64_t* resv;
  const uint8_t* resn;
};

__global__ __launch_bounds__(kBlock) void k_xw_emit(const EmitArgsX* __restrict__ ap, int64_t nrows, const uint32_t* rq,
                                                    int64_t* o_chunk, int32_t* o_type, int64_t* o_ts, uint64_t* o_vals,
                                                    uint8_t* o_nul, int64_t* o_seq, int32_t* o_sidx) {
  const EmitArgsX& a = *ap;
  for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < nrows; r = nrows) {
    const uint32_t q = rq[r];
    const uint32_t src = a.rowsrc[q];
    const uint32_t it = a.op_item[src];
    const bool add = a.op_add[src];
    uint64_t vv[kMaxAggs];
    uint8_t vn[kMaxAggs];
    for (int g = 0; g < a.nagg; g++) {
      vv[g] = a.resv[(int64_t)g * a.nops + src];
      vn[g] = a.resn[(int64_t)g * a.nops + src];
    }
    const int64_t ts = add ? a.its[it] : a.op_now[src];
    ItemCtx cx{a.attr, a.nul, a.cap, (int64_t)it, a.ncols, ts, vv, vn};
    const int64_t row = a.row0 + r;
    for (int c = 0; c < a.nout; c++) {
      Val v = eval_expr(a.es.ins + a.outs[c].off, a.outs[c].len, a.es.consts, cx);
      o_vals[row * a.nout + c] = v.b;
      o_nul[row * a.nout + c] = (uint8_t)v.null;
    }
    o_ts[row] = ts;
    o_type[row] = add ? 0 : 1;
    o_chunk[row] = a.chunk0 + (int64_t)a.op_chunk[q];
    o_seq[row] = a.op_seq[src];
    o_sidx[row] = 0;
  }
}

// ---------------------------------------------------------------- carry / misc
__global__ __launch_bounds__(kBlock) void k_xw_keep(int64_t total, const uint64_t* eopp, int window, uint32_t* keep) {
  for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < total; j = total)
    keep[j] = (window && eopp[j] == kNoOpp) ? 1u : 0u;
}

struct CarryArgs {
  int64_t total, cap_src, cap_dst;
  int ncols, nagg;
  const uint32_t* sp;
  const uint32_t* keep;
  const uint32_t* koff;
  const uint32_t* segid;
  const int64_t* last_out;   // per segment (time windows), may be null
  const int64_t* last_j;     // batch windows: per sorted position, its ilast in the carry
  ItemPtrs src, dst;
};

// The kept items, in sorted (key, FIFO) order, become the next push's carry.
__global__ __launch_bounds__(kBlock) void k_xw_carry(const CarryArgs* __restrict__ ap) {
  const CarryArgs& a = *ap;
  for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < a.total; j = a.total) {
    if (!a.keep[j]) continue;
    const int64_t t = a.koff[j];
    const uint32_t it = a.sp[j];
    a.dst.pk[t] = a.src.pk[it];
    a.dst.ts[t] = a.src.ts[it];
    a.dst.seq[t] = a.src.seq[it];
    a.dst.sid[t] = a.src.sid[it];
    a.dst.last[t] = a.last_j ? a.last_j[j] : (a.last_out ? a.last_out[a.segid[j]] : INT64_MIN);
    a.dst.call[t] = -1;
    a.dst.row[t] = -1;
    for (int c = 0; c < a.ncols; c++) {
      a.dst.attr[(int64_t)c * a.cap_dst + t] = a.src.attr[(int64_t)c * a.cap_src + it];
      a.dst.nul[(int64_t)c * a.cap_dst + t] = a.src.nul[(int64_t)c * a.cap_src + it];
    }
    for (int g = 0; g < a.nagg; g++) {
      a.dst.argv[(int64_t)g * a.cap_dst + t] = a.src.argv[(int64_t)g * a.cap_src + it];
      a.dst.argn[(int64_t)g * a.cap_dst + t] = a.src.argn[(int64_t)g * a.cap_src + it];
    }
  }
}

// new pending list = the segments' remaining entries + the kept orphans
__global__ __launch_bounds__(kBlock) void k_xw_pend_gather(int64_t nseg, const uint32_t* proom_off, const uint32_t* pcnt,
                                                           const uint32_t* pcnt_off, const uint64_t* spk,
                                                           const int64_t* sv, uint64_t* dpk, int64_t* dv) {
  for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < nseg; k = nseg) {
    const int64_t o = proom_off[k], d = pcnt_off[k];
    for (uint32_t i = 0; i < pcnt[k]; i++) {
      dpk[d + i] = spk[o + i];
      dv[d + i] = sv[o + i];
    }
  }
}

__global__ __launch_bounds__(kBlock) void k_xw_pend_orphan_copy(int64_t np, const uint32_t* keep, const uint32_t* koff,
                                                                int64_t base, const uint64_t* ppk, const int64_t* pv,
                                                                uint64_t* dpk, int64_t* dv) {
  for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < np; p = np) {
    if (!keep[p]) continue;
    dpk[base + koff[p]] = ppk[p];
    dv[base + koff[p]] = pv[p];
  }
}

// k_gather_u64 with the values' sign bit flipped (signed -> order-preserving unsigned)
__global__ __launch_bounds__(kBlock) void k_xw_gather_u64(const uint64_t* src, const uint32_t* perm, uint64_t* dst,
                                                          int64_t n, uint64_t flip) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i = n) dst[i] = src[perm[i]] ^ flip;
}
__global__ __launch_bounds__(kBlock) void k_xw_gather_u32(const uint32_t* src, const uint32_t* perm, uint32_t* dst,
                                                          int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i = n) dst[i] = src[perm[i]];
}
__global__ __launch_bounds__(kBlock) void k_xw_timer_rank(const uint32_t* perm, const int32_t* tF, int64_t nt,
                                                          uint32_t* rank, int32_t* sF) {
  for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < nt; t = nt) {
    rank[perm[t]] = (uint32_t)t;
    sF[t] = tF[perm[t]];
  }
}
__global__ __launch_bounds__(kBlock) void k_xw_op_sid(int64_t nops, const uint32_t* op_item, const uint64_t* isid,
                                                      uint32_t* out) {
  for (int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x; q < nops; q = nops) out[q] = (uint32_t)isid[op_item[q]];
}

// ---------------------------------------------------------------- batch windows
// lengthBatch / timeBatch in full-batch mode (LengthBatchWindowProcessor.java:
// 206-243, TimeBatchWindowProcessor.java:279-366).  A flush F of a key emits
// one chunk: the previous batch's items as EXPIRED (when the query outputs
// expired events), RESET, the batch's items as CURRENT.  Items of a key
// segment in FIFO order: [a carried items already added, awaiting expiry]
// [carried items of the open batch] [new items]; each item's add and expiry
// opportunities are flushes (2F + 1, expiry before add at one flush), both
// non-decreasing along the segment, so the operations of a key keep
// k_xw_ops' closed-form positions.  RESET (every group state of the partition
// cleared, PartitionStateHolder.cleanGroupByStates) is applied lazily by the
// fold: a state's first add of a flush starts it from zero (k_xw_fold epochs).

// added_j[j]: the item at sorted position j was added at an earlier flush
__global__ __launch_bounds__(kBlock) void k_xb_added(int64_t total, int64_t C, const uint32_t* sp, const int64_t* ilast,
                                                     uint8_t* added_j) {
  for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < total; j = total) {
    const uint32_t it = sp[j];
    added_j[j] = (it < (uint32_t)C && ilast[it] == 1) ? 1 : 0;
  }
}

// carried items of the segment [s, s + ck) already added: a prefix (FIFO)
__device__ __forceinline__ int64_t xb_added_count(const uint8_t* added_j, int64_t s, int64_t ck) {
  return first_false(s, s + ck, [=](int64_t i) { return added_j[i] != 0; }) - s;
}

struct XbArgs {
  int64_t total, C, L;
  int expired_on;
  const uint32_t* sp;
  const uint32_t* segid;
  const int64_t* segS;
  const int64_t* segCk;
  const uint8_t* added_j;
  const int32_t* irow;
  const int32_t* icall;
  const uint32_t* fr;        // lengthBatch: flush rank of each batch row (exclusive scan of the triggers)
  const int32_t* bflush;     // timeBatch: per call, the flush its events join (-1: none in this push)
  int64_t nf;                // timeBatch: flushes of this push
  // stream.current.event timeBatch: per call its chunk, the first flush at or
  // after it and its RESET epoch; the push's first flush (carried items)
  const int32_t* cchunk;
  const int32_t* cflush;
  const int64_t* cepoch;
  int64_t first_flush;
  const int64_t* ilast;      // carried items' ilast (lengthBatch stream mode: their batch epoch)
  int64_t chunk0;            // global id of the push's first chunk
  // externalTimeBatch: per sorted position its trigger flag and the triggers
  // before it (all keys), the triggers' sorted positions (nf of them)
  const uint32_t* trig_j;
  const uint32_t* tjx;
  const uint32_t* tpos;
  uint64_t* aopp;
  uint64_t* eopp;
  int64_t* epoch_j;          // per sorted position: the RESET epoch its add folds in
  uint8_t* keep_j;           // carried to the next push
  int64_t* last_j;           // its ilast there
};

// batch window modes (WindowXEngine::bmode)
enum : int { XB_FULL_LEN = 0, XB_FULL_TIME = 1, XB_STREAM_LEN = 2, XB_ZERO_LEN = 3, XB_STREAM_TIME = 4,
              XB_FULL_EXT = 5 };

// lengthBatch triggers: the new item whose open-batch ordinal completes a batch
__global__ __launch_bounds__(kBlock) void k_xb_len_trig(const XbArgs* __restrict__ ap, uint32_t* trig) {
  const XbArgs& a = *ap;
  for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < a.total; j = a.total) {
    const uint32_t k = a.segid[j];
    const int64_t s = a.segS[k], ck = a.segCk[k];
    const int64_t na = xb_added_count(a.added_j, s, ck);
    const int64_t o = j - s - na;
    const uint32_t it = a.sp[j];
    if (o >= 0 && (o + 1) % a.L == 0 && it >= (uint32_t)a.C) trig[a.irow[it]] = 1u;
  }
}

// per flush (lengthBatch): its clock and in_seq, from the trigger row
__global__ __launch_bounds__(kBlock) void k_xb_len_flushes(int64_t n, const uint32_t* trig, const uint32_t* fr,
                                                           const int32_t* call_of, const int64_t* call_now, int64_t seq0,
                                                           int64_t* fnow, int64_t* fseq) {
  for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < n; r = n) {
    if (!trig[r]) continue;
    fnow[fr[r]] = call_now[call_of[r]];
    fseq[fr[r]] = seq0 + r;
  }
}

// Each item's add / expiry opportunities (op positions: 2 * chunk + 1 when
// expirations come first in the chunk, 2 * chunk for an add before them),
// the epoch of its add and what is carried.
__global__ __launch_bounds__(kBlock) void k_xb_opp(const XbArgs* __restrict__ ap, int mode) {
  const XbArgs& a = *ap;
  for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < a.total; j = a.total) {
    const uint32_t k = a.segid[j];
    const int64_t s = a.segS[k], e = a.segS[k + 1], ck = a.segCk[k];
    const uint32_t it = a.sp[j];
    uint64_t ao = kNoOpp, eo = kNoOpp;
    int64_t ep = -1, last = 0;
    bool keep = false;
    if (mode == XB_FULL_LEN || mode == XB_FULL_TIME || mode == XB_FULL_EXT) {
      // full batches: [expired previous batch] RESET [batch] at each flush
      const int64_t na = xb_added_count(a.added_j, s, ck);
      if (mode == XB_FULL_LEN) {
        const int64_t tot = e - s - na;             // open batch + new items
        const int64_t nb = tot / a.L;               // batches completed in this push
        // flush of batch b: the trigger at ordinal (b + 1) L - 1
        auto flush_of = [&](int64_t b) -> uint64_t {
          return (uint64_t)a.fr[a.irow[a.sp[s + na + (b + 1) * a.L - 1]]];
        };
        if (j - s < na) {
          if (a.expired_on && nb >= 1) eo = 2 * flush_of(0) + 1;
        } else {
          const int64_t b = (j - s - na) / a.L;
          if (b < nb) ao = 2 * flush_of(b) + 1;
          if (a.expired_on && b + 1 < nb) eo = 2 * flush_of(b + 1) + 1;
        }
      } else if (mode == XB_FULL_EXT) {
        // externalTimeBatch: an item's flush is its key's first trigger after
        // it (the trigger event itself opens the next batch); the batch
        // awaiting expiry leaves at the key's first trigger of the push
        const int64_t r = (int64_t)a.tjx[j] + (int64_t)a.trig_j[j];   // triggers at or before j
        auto flush_at = [&](int64_t q) -> int64_t {   // the q-th trigger's flush, if it is this key's
          if (q >= a.nf || (int64_t)a.tpos[q] >= e) return -1;
          return (int64_t)a.fr[a.irow[a.sp[a.tpos[q]]]];
        };
        const int64_t f0 = flush_at(r);
        if (j - s < na) {
          if (a.expired_on && f0 >= 0) eo = 2 * (uint64_t)f0 + 1;
        } else if (f0 >= 0) {
          ao = 2 * (uint64_t)f0 + 1;
          const int64_t f1 = flush_at(r + 1);
          if (a.expired_on && f1 >= 0) eo = 2 * (uint64_t)f1 + 1;
        }
      } else {
        if (j - s < na) {
          if (a.expired_on && a.nf >= 1) eo = 1;
        } else {
          const int64_t f = it < (uint32_t)a.C ? (a.nf >= 1 ? 0 : -1) : (int64_t)a.bflush[a.icall[it]];
          if (f >= 0) {
            ao = 2 * (uint64_t)f + 1;
            if (a.expired_on && f + 1 < a.nf) eo = 2 * (uint64_t)(f + 1) + 1;
          }
        }
      }
      if (ao != kNoOpp) ep = a.chunk0 + (int64_t)(ao >> 1);   // the flush's RESET precedes its adds
      const bool added = a.added_j[j] || ao != kNoOpp;
      keep = !added || (a.expired_on && eo == kNoOpp);
      last = added ? 1 : 0;
    } else if (mode == XB_STREAM_LEN) {
      // processStreamCurrentEvents: every event its own chunk (a new item's
      // rank); batch b of the key = ordinals [bL, (b+1)L) with the carried open
      // batch first; the first item of batch b + 1 expires batch b and RESETs
      // before its own add
      const int64_t o = j - s, bl = (e - s - 1) / a.L, b = o / a.L;
      if (o >= ck) ao = 2 * (uint64_t)(it - (uint32_t)a.C) + 1;
      if (a.expired_on && b < bl) eo = 2 * (uint64_t)(a.sp[s + (b + 1) * a.L] - (uint32_t)a.C) + 1;
      const int64_t f = s + b * a.L;   // the batch's first item
      ep = f < s + ck ? a.ilast[a.sp[f]] : a.chunk0 + (int64_t)(a.sp[f] - (uint32_t)a.C);
      keep = b == bl;
      last = ep;
    } else if (mode == XB_ZERO_LEN) {
      // processLengthZeroBatch: the event, its EXPIRED copy, RESET -- one chunk
      const uint64_t c = (uint64_t)(it - (uint32_t)a.C);
      ao = 2 * c;
      if (a.expired_on) eo = 2 * c + 1;
      ep = a.chunk0 + (int64_t)c;
    } else {
      // stream.current.event timeBatch: a call's events in its chunk, then at a
      // flush (that chunk or a later TIMER) every event since the last flush
      // as EXPIRED, then RESET
      if (it < (uint32_t)a.C) {
        if (a.expired_on && a.first_flush >= 0) eo = 2 * (uint64_t)a.first_flush + 1;
      } else {
        const int32_t c = a.icall[it];
        ao = 2 * (uint64_t)a.cchunk[c];
        if (a.expired_on && a.cflush[c] >= 0) eo = 2 * (uint64_t)a.cflush[c] + 1;
        ep = a.cepoch[c];
      }
      keep = a.expired_on && eo == kNoOpp;
    }
    a.aopp[j] = ao;
    a.eopp[j] = eo;
    a.epoch_j[j] = ep;
    a.keep_j[j] = keep ? 1 : 0;
    a.last_j[j] = last;
  }
}

// per chunk of a new item (lengthBatch stream / zero modes): its clock and in_seq
__global__ __launch_bounds__(kBlock) void k_xb_item_chunks(int64_t C, int64_t m, const int32_t* icall,
                                                           const int32_t* irow, const int64_t* call_now, int64_t seq0,
                                                           int64_t* fnow, int64_t* fseq) {
  for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < m; j = m) {
    fnow[j] = call_now[icall[C + j]];
    fseq[j] = seq0 + irow[C + j];
  }
}

__global__ __launch_bounds__(kBlock) void k_xb_nops(int64_t total, const uint64_t* aopp, const uint64_t* eopp,
                                                    uint32_t* nops) {
  for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < total; j = total)
    nops[j] = (aopp[j] != kNoOpp ? 1u : 0u) + (eopp[j] != kNoOpp ? 1u : 0u);
}

struct XbOpArgs {
  int64_t total;
  const uint32_t* sp;
  const uint32_t* segid;
  const int64_t* segS;
  const int64_t* segCk;
  const uint8_t* added_j;
  const uint64_t* aopp;
  const uint64_t* eopp;
  const int64_t* epoch_j;
  int full;                   // full-batch modes: carried items awaiting expiry precede the adds
  const uint32_t* opscan;
  const int64_t* fnow;
  const int64_t* fseq;
  int current_on, expired_on;
  int64_t* op_epoch;
  uint32_t* op_item;
  uint8_t* op_add;
  uint8_t* op_on;
  uint32_t* op_chunk;
  int64_t* op_now;
  int64_t* op_seq;
};

// Operations of a key in the reference's order: per flush its expirations
// (FIFO), then its adds (FIFO).  Adds occupy the contiguous positions
// [s + a, ...), expirations a prefix [s, ...) of the segment.
__global__ __launch_bounds__(kBlock) void k_xb_ops(const XbOpArgs* __restrict__ ap) {
  const XbOpArgs& a = *ap;
  for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < a.total; j = a.total) {
    const uint32_t k = a.segid[j];
    const int64_t s = a.segS[k], e = a.segS[k + 1], ck = a.segCk[k];
    const int64_t base = a.opscan[s];
    // adds occupy [s + na, ...): after the carried items awaiting expiry (full
    // batches), after every carried item (stream modes: carried items were added)
    const int64_t na = a.full ? xb_added_count(a.added_j, s, ck) : ck;
    const uint32_t it = a.sp[j];
    const uint64_t ao = a.aopp[j], eo = a.eopp[j];
    if (ao != kNoOpp) {
      const int64_t lo = upper_bound(a.eopp, s, e, ao);   // expirations at or before this flush
      const int64_t q = base + (j - s - na) + (lo - s);
      const uint32_t f = (uint32_t)(ao >> 1);
      a.op_item[q] = it;
      a.op_add[q] = 1;
      a.op_on[q] = (uint8_t)a.current_on;
      a.op_chunk[q] = f;
      a.op_now[q] = a.fnow[f];
      a.op_seq[q] = a.fseq[f];
      a.op_epoch[q] = a.epoch_j[j];
    }
    if (eo != kNoOpp) {
      const int64_t lo = lower_bound(a.aopp, s + na, e, eo);   // adds at earlier flushes
      const int64_t q = base + (j - s) + (lo - s - na);
      const uint32_t f = (uint32_t)(eo >> 1);
      a.op_item[q] = it;
      a.op_add[q] = 0;
      a.op_on[q] = (uint8_t)a.expired_on;
      a.op_chunk[q] = f;
      a.op_now[q] = a.fnow[f];
      a.op_seq[q] = a.fseq[f];
    }
  }
}

// timeBatch: per call its passing items and the in_seq of its last one
__global__ __launch_bounds__(kBlock) void k_xb_call_items(int64_t C, int64_t m, const int32_t* icall,
                                                          const int32_t* irow, int64_t seq0, uint32_t* ccount,
                                                          int64_t* clast_seq) {
  for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < m; j = m) {
    const int32_t c = icall[C + j];
    atomicAdd(ccount + c, 1u);
    if (j + 1 == m || icall[C + j + 1] != c) clast_seq[c] = seq0 + irow[C + j];
  }
}

// ---------------------------------------------------------------- externalTimeBatch
// ExternalTimeBatchWindowProcessor.java without a timeout: process :238-311,
// initTiming :313-334, flushToOutputChunk :336-383, findEndTime :440-444,
// cloneAppend :446-456.  A tumbling batch per partition key clocked by the
// event's own LONG attribute ts.  Per key: startTime, endTime E and
// lastCurrentEventTime M (the running maximum of ts, 0 before the first
// event).  An event with ts >= E first flushes the open batch -- one chunk:
// [previous batch EXPIRED, stamped M] RESET [batch CURRENT] -- then sets
// E = findEndTime(M, startTime, T) and opens the next batch; any other event
// joins the open batch.  After a key's first event its open batch is never
// empty, so every trigger emits a chunk and the pending RESET
// (state.resetEvent, non-null iff the open batch holds an event) needs no
// flag of its own.  The flush of an item is its key's first trigger after it:
// the full-batch operation encoding of lengthBatch applies (k_xb_opp).
//
// Where the flushes fall.  Write B(x) = findEndTime(x, start, T) and M_i for
// the key's running maximum after event i.  Invariant: M_i < E_i (after the
// first event E > ts = M; a non-trigger has ts < E; a trigger sets
// E = B(M) > M).  So a trigger has ts_i >= E_{i-1} > M_{i-1}, i.e. M_i = ts_i.
//   Claim: if M_{i-1} >= start then E_{i-1} = B(M_{i-1}), so event i triggers
//   iff ts_i >= B(M_{i-1}) -- a test on the prefix maximum alone.
//   Proof: for x >= start the remainder (x - start) % T is non-negative and
//   B(x) is the first point of the grid start + kT strictly above x.  E_{i-1}
//   is on the grid: it is start + T (no / attribute startTime) or some B(y);
//   for y >= start that is a grid point with B(y) - T <= y, for y < start
//   Java's truncating % gives B(y) = (first grid point >= y) + T <= start + T.
//   In each case E_{i-1} - T <= max(y, start) <= M_{i-1} (y is an earlier
//   maximum), and M_{i-1} < E_{i-1} by the invariant: E_{i-1} is the first
//   grid point above M_{i-1}.  []
// While M_{i-1} < start (a startTime ahead of the data: negative remainders,
// batches up to 2T long) E depends on the maximum at the last trigger itself,
// not on its grid cell, and the rule above does not hold: that stretch of a
// key -- a prefix of its events, M never decreases -- and the key's first
// event are walked by one lane per key (k_etb_lane); everything after it is
// data-parallel over the segmented prefix maximum (k_etb_trig).  Timestamps
// are taken as non-negative, which the reference's endTime = -1 sentinel
// assumes too (a negative endTime would re-run initTiming at the next call).
__host__ __device__ __forceinline__ int64_t etb_find_end(int64_t cur, int64_t start, int64_t T) {
  // :440-444; C's % truncates like Java's
  return cur + (T - (int64_t)((uint64_t)cur - (uint64_t)start) % T);
}

struct EtbArgs {
  int64_t total, C, T, cap, nseg, seq0;
  int ts_col, start_mode, start_col, replace;
  int64_t start_const;
  const uint32_t* sp;
  const uint32_t* segid;
  const int64_t* segS;
  const int64_t* segCk;
  const int64_t* pA;          // per key segment: its carried (startTime, endTime, M) at pv[pA .. pA + 3)
  const int64_t* pB;
  const int64_t* pv;
  const int32_t* irow;
  uint64_t* iattr;            // [ncols][cap]
  uint8_t* inul;
  int64_t* M;                 // [total] ts of the new items -> the key's running maximum
  uint32_t* head;             // [total] segment heads
  int64_t* E;                 // [total] endTime in force once the item is appended
  uint32_t* trig_j;           // [total] the item triggers a flush
  uint32_t* trig_r;           // [n] the same per batch row
  int64_t* seg_start;         // [nseg] the key's startTime
  int64_t* seg_end;           // [nseg] its endTime after the lane's stretch
  int64_t* seg_j1;            // [nseg] first position the data-parallel rule decides
};

// scan input: the new items' ts; a key's first position also takes the carried M
__global__ __launch_bounds__(kBlock) void k_etb_seed(const EtbArgs* __restrict__ ap) {
  const EtbArgs& a = *ap;
  for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < a.total; j = a.total) {
    const uint32_t k = a.segid[j];
    const uint32_t it = a.sp[j];
    int64_t v = it >= (uint32_t)a.C ? (int64_t)a.iattr[(int64_t)a.ts_col * a.cap + it] : INT64_MIN;
    const bool hd = j == a.segS[k];
    if (hd) {
      const int64_t seed = a.pB[k] - a.pA[k] == 3 ? a.pv[a.pA[k] + 2] : 0;   // lastCurrentEventTime starts at 0
      v = v > seed ? v : seed;
    }
    a.M[j] = v;
    a.head[j] = hd ? 1u : 0u;
    a.trig_j[j] = 0u;
    a.E[j] = 0;
  }
}

// Segmented inclusive prefix maximum over (head flag, int64): per-tile
// aggregates, one block over the tiles, then each tile with its carry-in.
constexpr int kEtbTile = kBlock * 4;
struct SegMax {
  int64_t v;
  uint32_t f;
};
__device__ __forceinline__ SegMax segmax_op(SegMax x, SegMax y) {
  return SegMax{y.f ? y.v : (x.v > y.v ? x.v : y.v), x.f | y.f};
}
// inclusive scan of one value per thread, left in LDS: lv / lf [kBlock]
__device__ __forceinline__ void block_segmax_incl(SegMax x, int64_t* lv, uint32_t* lf) {
  const int t = threadIdx.x;
  lv[t] = x.v;
  lf[t] = x.f;
  __syncthreads();
  for (int o = 1; o < kBlock; o <<= 1) {
    SegMax p{INT64_MIN, 0u};
    if (t >= o) p = SegMax{lv[t - o], lf[t - o]};
    __syncthreads();
    if (t >= o) {
      x = segmax_op(p, x);
      lv[t] = x.v;
      lf[t] = x.f;
    }
    __syncthreads();
  }
}
// a thread's four items of its tile, folded
__device__ __forceinline__ SegMax etb_load4(const int64_t* v, const uint32_t* f, int64_t n, int64_t b0, SegMax* x) {
  SegMax acc{INT64_MIN, 0u};
#pragma unroll
  for (int i = 0; i < 4; i++) {
    x[i] = b0 + i < n ? SegMax{v[b0 + i], f[b0 + i]} : SegMax{INT64_MIN, 0u};
    acc = segmax_op(acc, x[i]);
  }
  return acc;
}
__global__ __launch_bounds__(kBlock) void k_etb_pmax_tiles(const int64_t* v, const uint32_t* f, int64_t n, int64_t* tv,
                                                           uint32_t* tf) {
  __shared__ int64_t lv[kBlock];
  __shared__ uint32_t lf[kBlock];
  SegMax x[4];
  const SegMax acc = etb_load4(v, f, n, (int64_t)blockIdx.x * kEtbTile + threadIdx.x * 4, x);
  block_segmax_incl(acc, lv, lf);
  if (threadIdx.x == 0) {
    tv[blockIdx.x] = lv[kBlock - 1];
    tf[blockIdx.x] = lf[kBlock - 1];
  }
}
// exclusive scan of the tile aggregates, in place (the carry-in's value is all a tile needs)
__global__ __launch_bounds__(kBlock) void k_etb_pmax_scan(int64_t* tv, const uint32_t* tf, int64_t nt) {
  __shared__ int64_t lv[kBlock];
  __shared__ uint32_t lf[kBlock];
  SegMax carry{INT64_MIN, 0u};
  for (int64_t base = 0; base < nt; base += kBlock) {
    const int64_t i = base + threadIdx.x;
    const SegMax x = i < nt ? SegMax{tv[i], tf[i]} : SegMax{INT64_MIN, 0u};
    block_segmax_incl(x, lv, lf);
    const SegMax ex = threadIdx.x > 0 ? SegMax{lv[threadIdx.x - 1], lf[threadIdx.x - 1]} : SegMax{INT64_MIN, 0u};
    if (i < nt) tv[i] = segmax_op(carry, ex).v;
    carry = segmax_op(carry, SegMax{lv[kBlock - 1], lf[kBlock - 1]});
    __syncthreads();
  }
}
__global__ __launch_bounds__(kBlock) void k_etb_pmax_apply(int64_t* v, const uint32_t* f, int64_t n, const int64_t* tpre) {
  __shared__ int64_t lv[kBlock];
  __shared__ uint32_t lf[kBlock];
  SegMax x[4];
  const int64_t b0 = (int64_t)blockIdx.x * kEtbTile + threadIdx.x * 4;
  const SegMax acc = etb_load4(v, f, n, b0, x);
  block_segmax_incl(acc, lv, lf);
  SegMax run{tpre[blockIdx.x], 0u};
  if (threadIdx.x > 0) run = segmax_op(run, SegMax{lv[threadIdx.x - 1], lf[threadIdx.x - 1]});
#pragma unroll
  for (int i = 0; i < 4; i++) {
    run = segmax_op(run, x[i]);
    if (b0 + i < n) v[b0 + i] = run.v;
  }
}

// One lane per key: a new key's first event (initTiming, and the event itself:
// with an attribute startTime it may reach endTime at once, which flushes an
// empty batch -- no chunk -- and moves endTime), then the events met while the
// running maximum is still below startTime.
__global__ __launch_bounds__(kBlock) void k_etb_lane(const EtbArgs* __restrict__ ap) {
  const EtbArgs& a = *ap;
  for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < a.nseg; k = a.nseg) {
    const int64_t s = a.segS[k], e = a.segS[k + 1];
    const uint64_t* tsv = a.iattr + (int64_t)a.ts_col * a.cap;
    int64_t j = s + a.segCk[k];
    int64_t start = 0, E = 0;
    if (a.pB[k] - a.pA[k] == 3) {
      start = a.pv[a.pA[k]];
      E = a.pv[a.pA[k] + 1];
    } else if (j < e) {
      const uint32_t it = a.sp[j];
      const int64_t ts0 = (int64_t)tsv[it];
      if (a.start_mode == SHD_ETB_START_CONST) {
        start = a.start_const;
        E = etb_find_end(ts0, start, a.T);
      } else {
        start = a.start_mode == SHD_ETB_START_ATTR ? (int64_t)a.iattr[(int64_t)a.start_col * a.cap + it] : ts0;
        E = start + a.T;
      }
      if (ts0 >= E) E = etb_find_end(a.M[j], start, a.T);
      a.E[j] = E;
      j++;
    }
    while (j < e && j > s && a.M[j - 1] < start) {
      const uint32_t it = a.sp[j];
      if ((int64_t)tsv[it] >= E) {
        a.trig_j[j] = 1u;
        a.trig_r[a.irow[it]] = 1u;
        E = etb_find_end(a.M[j], start, a.T);
      }
      a.E[j] = E;
      j++;
    }
    a.seg_start[k] = start;
    a.seg_end[k] = E;
    a.seg_j1[k] = j;
  }
}

// Every other new item: triggers iff ts >= B(M of the events before it)
// (the claim above); endTime once it is appended is B of the maximum then.
__global__ __launch_bounds__(kBlock) void k_etb_trig(const EtbArgs* __restrict__ ap) {
  const EtbArgs& a = *ap;
  for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < a.total; j = a.total) {
    const uint32_t it = a.sp[j];
    const uint32_t k = a.segid[j];
    if (it < (uint32_t)a.C || j < a.seg_j1[k] || j <= a.segS[k]) continue;
    const int64_t start = a.seg_start[k];
    const int64_t bnd = etb_find_end(a.M[j - 1], start, a.T);
    const bool tr = (int64_t)a.iattr[(int64_t)a.ts_col * a.cap + it] >= bnd;
    a.E[j] = tr ? etb_find_end(a.M[j], start, a.T) : bnd;
    if (tr) {
      a.trig_j[j] = 1u;
      a.trig_r[a.irow[it]] = 1u;
    }
  }
}

// per flush: lastCurrentEventTime at its trigger (the EXPIRED rows' timestamp) and in_seq
__global__ __launch_bounds__(kBlock) void k_etb_flushes(const EtbArgs* __restrict__ ap, const uint32_t* fr,
                                                        int64_t* fnow, int64_t* fseq) {
  const EtbArgs& a = *ap;
  for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < a.total; j = a.total) {
    if (!a.trig_j[j]) continue;
    const int64_t r = a.irow[a.sp[j]];
    fnow[fr[r]] = a.M[j];
    fseq[fr[r]] = a.seq0 + r;
  }
}

// The keys' state for the next push (three entries per key, key order), and
// replaceTimestampWithBatchEndTime: the appended clone's ts attribute becomes
// the endTime in force (:446-451).
__global__ __launch_bounds__(kBlock) void k_etb_state(const EtbArgs* __restrict__ ap, const uint64_t* ipk,
                                                      uint64_t* dpk, int64_t* dv) {
  const EtbArgs& a = *ap;
  for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < a.nseg; k = a.nseg) {
    const int64_t s = a.segS[k], e = a.segS[k + 1];
    const uint64_t pk = ipk[a.sp[s]];
    dpk[3 * k] = dpk[3 * k + 1] = dpk[3 * k + 2] = pk;
    dv[3 * k] = a.seg_start[k];
    dv[3 * k + 1] = e - 1 >= a.seg_j1[k] ? a.E[e - 1] : a.seg_end[k];
    dv[3 * k + 2] = a.M[e - 1];
  }
}
__global__ __launch_bounds__(kBlock) void k_etb_replace(const EtbArgs* __restrict__ ap) {
  const EtbArgs& a = *ap;
  for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < a.total; j = a.total) {
    const uint32_t it = a.sp[j];
    if (it < (uint32_t)a.C) continue;
    a.iattr[(int64_t)a.ts_col * a.cap + it] = (uint64_t)a.E[j];
    a.inul[(int64_t)a.ts_col * a.cap + it] = 0;
  }
}

int bits_for(uint64_t v) {
  int b = 0;
  while (b < 64 && (v >> b)) b++;
  return std::max(b, 1);
}

}  // namespace

// ====================================================================== host
// The keyed window engine's readback block (WindowXEngine::tot): every value
// is read back on its own, right after the call that writes it.
struct WindowTotals {
  uint32_t scan_total;   // scan_exclusive_u32 (WindowXEngine::scan)
  uint64_t kmax;         // reduce_max_u64: largest partition key of the items
};
static_assert(offsetof(WindowTotals, scan_total) == 0 && offsetof(WindowTotals, kmax) == 8 &&
                  sizeof(WindowTotals) <= 64,
              "WindowTotals device layout");
struct WindowTotalsHost : WindowTotals {
  uint32_t n_timer;   // copy of the time lane's timer count (ntimer)
  int64_t last_out;   // copy of the last output sequence (last_out)
};

struct WindowXEngine : Engine {
  std::vector<int> filters;
  int wkind = 0;
  int64_t wparam = 0;
  bool partitioned = false;
  int key_expr = -1, key_col = -1, key_type = 0;
  int ngk = 0;
  int gk_expr[kMaxGroupAttrs] = {}, gk_col[kMaxGroupAttrs] = {}, gk_type[kMaxGroupAttrs] = {};
  int nagg = 0, ncols = 0, nw = 0;
  bool group = false, plain = false;
  GroupDict gd;
  // window items: [0, C) of slot items.cur carried (key-sorted, FIFO inside a key)
  int64_t C = 0;
  ItemStore items;
  // pending notify entries (time windows with timers): grouped by key (sorted),
  // each key's entries in queue (FIFO) order
  int64_t np = 0;
  DevBuf ppk, pv, ppk2, pv2;
  int64_t last_global = INT64_MIN;   // unpartitioned time window: state.lastTimestamp
  // aggregator states [nagg][nstates]
  DevBuf g_dsum, g_lsum, g_cnt;
  int64_t nstates = 0;
  // min / max: `mm` the plan has such aggregators (k_xw_fold<true>), `track`
  // their tracking mode.  The deque store of the ndq tracking ones: lengths and
  // offsets [ndq][nstates], the values packed in slot dq_cur of dq_val
  // (double-buffered like the items: a push reads one slot and packs what is
  // left into the other, which grows by doubling).
  // `xa`: the plan has stdDev / distinctCount / and / or (k_xw_fold<true, true>); each
  // distinctCount owns a row of the store too, its (key, count) pairs
  // (dq_esz: the words an add can append to a row).
  bool mm = false, track = false, xa = false;
  int ndq = 0, dq_words = 0;
  int dq_of[kMaxAggs] = {};
  int dq_esz[kMaxAggs] = {};
  DevBuf dq_len, dq_off, dq_val[2];
  int dq_cur = 0;
  int64_t dq_total = 0;
  // batch windows: per state its RESET epoch (k_xw_fold); timeBatch's
  // processor-level nextEmitTime and the Scheduler's notify queue (FIFO)
  bool batch = false;
  int64_t wparam2 = 0;
  DevBuf g_epoch;
  int64_t tb_next = -1;
  std::deque<int64_t> tb_notify;
  int bmode = 0;   // XB_* (k_xb_opp)
  int64_t tb_epoch = -1;   // stream.current.event timeBatch: global chunk id of the last flush
  // externalTimeBatch: the packed parameters (siddhi_ir.h); each key's
  // (startTime, endTime, lastCurrentEventTime) is carried as three entries of
  // the pending list ppk / pv (a known key always holds its open batch, so it
  // has a segment in every push and the list is rewritten in segment order)
  int etb_ts_col = 0, etb_start_mode = 0, etb_start_col = 0, etb_replace = 0;
  int64_t etb_start_const = 0;

  // ---- per-push scratch, by the phase that first writes it
  // calls and clock
  DevBuf d_offs, d_call_of, d_last, d_call_now, d_F, d_fnow;
  // filter, partition key, runs
  DevBuf d_flags, d_cnt, d_off, d_pkey, d_start, d_run;
  // new items: their state key words
  DevBuf kw, kn, kh;
  // key segments
  DevBuf spk, spk2, sp, sp2, head, hscan, segS, segid, segCk, pA, pB, proom;
  // sliding windows: expiry, timer order
  DevBuf proom_off, etid, rec, tF, tHead, tSeg, ntimer, pout_pk, pout_v, pcnt, pcnt_off, last_out, tperm, tperm2, tk32,
      tk32b, tk64, tk64b, trank, sF, d_runs_before;
  // batch windows: flushes, opportunities
  DevBuf xb_added, xb_aopp, xb_trig, xb_fr, xb_fnow, xb_fseq, xb_bflush, xb_ccount, xb_clast, xb_epoch, xb_keep,
      xb_last, xb_cchunk, xb_cflush, xb_cepoch, op_epoch;
  DevBuf etb_M, etb_head, etb_E, etb_trigj, etb_tjx, etb_tpos, etb_tv, etb_tf, etb_seg_start, etb_seg_end, etb_seg_j1;
  // operations (either kind of window)
  DevBuf eopp, nops_b, opscan, op_item, op_add, op_on, op_chunk, op_now, op_seq;
  // fold and row selection
  DevBuf osid, osid2, oq, oq2, ohead, ohoff, ohl, resv, resn, rowflag, rowsrc, roff;
  // min / max deques: the lanes' regions, what the fold leaves
  DevBuf dq_room, dq_woff, dq_work, dq_nlen, dq_noff, dq_nsrc;
  // emit
  DevBuf rkey, rkey2, rq, rq2;
  // carry and pending
  DevBuf keep, koff, seg_pk, okeep, okoff, pend_tmp_pk, pend_tmp_v, pend_idx, pend_idx2, pend_key2;
  // scan and sort work space
  DevBuf d_scan, d_sort;
  PinnedBuf h_last, h_pin;
  ReadbackBlock<WindowTotals, WindowTotalsHost> tot;
  std::vector<int64_t> h_offs, h_now;
  std::vector<int32_t> h_F;
  std::vector<int64_t> h_fnow;

  int kind() const override { return ENG_WINDOW; }
  // sliding windows with timers: time, timeLength
  bool time_like() const { return timed() || wkind == SHD_W_EXTERNAL_TIME; }
  // with Scheduler TIMER chunks
  bool timed() const { return wkind == SHD_W_TIME || wkind == SHD_W_TIME_LENGTH; }

  // aggregates here always fold sequentially (bit-exact): the option is a no-op
  void set_option(const std::string& key, int64_t v) override {
    if (key == "exact_aggregates") return;
    Engine::set_option(key, v);
  }

  void reset() override {
    C = 0;
    np = 0;
    seq = 0;
    now = INT64_MIN;
    chunk_seq = 0;
    out.count = 0;
    counters = shd_counters{};
    last_global = INT64_MIN;
    tb_next = -1;
    tb_epoch = -1;
    tb_notify.clear();
    gd.reset(stream);
    if (nstates) {
      SHD_HIP(hipMemsetAsync(g_dsum.p, 0, g_dsum.cap, stream));
      SHD_HIP(hipMemsetAsync(g_lsum.p, 0, g_lsum.cap, stream));
      SHD_HIP(hipMemsetAsync(g_cnt.p, 0, g_cnt.cap, stream));
      if (g_epoch.p) SHD_HIP(hipMemsetAsync(g_epoch.p, 0xFF, g_epoch.cap, stream));
      if (dq_len.p) SHD_HIP(hipMemsetAsync(dq_len.p, 0, dq_len.cap, stream));
      if (dq_off.p) SHD_HIP(hipMemsetAsync(dq_off.p, 0, dq_off.cap, stream));
    }
    dq_total = 0;
  }

  // ---- storage
  // slot items.cur with room for `need` items, its [0, C) preserved
  void ensure_items(int64_t need) {
    const int from = items.cur, to = from ^ 1;
    if (items.cap[from] >= need) return;
    items.alloc(to, std::max<int64_t>(need, std::max<int64_t>(1024, items.cap[from] * 2)));
    if (C > 0)
      items.each([&](int c, int sub) {
        SHD_HIP(hipMemcpyAsync(items.at(to, c, sub), items.at(from, c, sub), C * kItemCol[c].size,
                               hipMemcpyDeviceToDevice, stream));
      });
    items.cur = to;
  }
  // A [rows][n] table of 8-byte cells (`cell` bytes) becomes [rows][n2]: new
  // cells are filled with `fill` bytes, the old rows copied.
  void grow_table(DevBuf& t, int rows, int64_t n, int64_t n2, int fill, size_t cell = 8) {
    DevBuf g;
    g.reserve((size_t)rows * n2 * cell);
    SHD_HIP(hipMemsetAsync(g.p, fill, (size_t)rows * n2 * cell, stream));
    for (int r = 0; r < rows && n; r++)
      SHD_HIP(hipMemcpyAsync(g.as<char>() + (size_t)r * n2 * cell, t.as<char>() + (size_t)r * n * cell, n * cell,
                             hipMemcpyDeviceToDevice, stream));
    SHD_HIP(hipStreamSynchronize(stream));
    t.swap(g);
  }
  // the aggregator state tables with exactly ns states per row
  void grow_states(int64_t ns) {
    grow_table(g_dsum, nagg, nstates, ns, 0);
    grow_table(g_lsum, nagg, nstates, ns, 0);
    grow_table(g_cnt, nagg, nstates, ns, 0);
    if (batch) grow_table(g_epoch, 1, nstates, ns, 0xFF);
    if (ndq > 0) {
      grow_table(dq_len, ndq, nstates, ns, 0, 4);
      grow_table(dq_off, ndq, nstates, ns, 0, 4);
    }
    nstates = ns;
  }
  void ensure_states(int64_t n) {
    if (nagg == 0) nstates = std::max(nstates, n);
    else if (n > nstates) grow_states(std::max<int64_t>(n, std::max<int64_t>(1024, nstates * 2)));
  }

  template <class T> void upload(DevBuf& d, const std::vector<T>& v) {
    d.reserve(std::max<size_t>(v.size(), 1) * sizeof(T));
    if (v.empty()) return;
    h_pin.reserve(v.size() * sizeof(T));
    SHD_HIP(hipStreamSynchronize(stream));   // the pinned staging area is free again
    std::memcpy(h_pin.p, v.data(), v.size() * sizeof(T));
    SHD_HIP(hipMemcpyAsync(d.p, h_pin.p, v.size() * sizeof(T), hipMemcpyHostToDevice, stream));
    SHD_HIP(hipStreamSynchronize(stream));
  }
  // exclusive scan; returns the total (every scan of this engine is read back on its own)
  uint32_t scan(const uint32_t* in, uint32_t* outp, int64_t n) {
    tot.reserve();
    return Engine::scan(in, outp, n, &tot.dev()->scan_total, &tot.host().scan_total, d_scan);
  }
  // stable sort of (key, value) pairs; returns the values' final array
  const uint32_t* sort_u32(DevBuf& k, DevBuf& v, DevBuf& k2, DevBuf& v2, int64_t n, int bits, const uint32_t** keys) {
    bool alt = false;
    radix_sort_pairs_u32(k.as<uint32_t>(), v.as<uint32_t>(), k2.as<uint32_t>(), v2.as<uint32_t>(), n, bits, d_sort,
                         stream, alt);
    if (keys) *keys = (alt ? k2 : k).as<uint32_t>();
    return (alt ? v2 : v).as<uint32_t>();
  }
  const uint32_t* sort_u64(DevBuf& k, DevBuf& v, DevBuf& k2, DevBuf& v2, int64_t n, int bits, const uint64_t** keys) {
    bool alt = false;
    radix_sort_pairs_u64(k.as<uint64_t>(), v.as<uint32_t>(), k2.as<uint64_t>(), v2.as<uint32_t>(), n, bits, d_sort,
                         stream, alt);
    if (keys) *keys = (alt ? k2 : k).as<uint64_t>();
    return (alt ? v2 : v).as<uint32_t>();
  }

  // ---- push
  // The scalars of one push, filled in phase by phase.
  struct Push {
    const Staged& b;
    bool extra_move;      // one clock move to `extra_t` with no events (shd_set_time)
    int64_t extra_t;
    int64_t n;            // events
    int ncalls = 0;       // InputHandler calls over them
    std::vector<char> moved;   // per call: the clock moved
    int64_t clk = 0;      // the clock after the push
    bool timers = false;  // the window runs TIMER chunks
    int nf = 0;           // clock moves they see
    XwArgs xa{};
    int64_t m = 0;        // new items
    uint32_t nruns = 0;   // partition runs
    int64_t total = 0;    // carried + new items
    int64_t cap = 0;      // capacity of the item slot in use
    ItemPtrs it{};        // its columns
    int64_t nseg = 0;     // key segments
    const uint32_t* SP = nullptr;   // the items in (key, FIFO) order
    int64_t nt = 0;       // TIMER chunks
    bool lane_ran = false;
    int64_t nflush = 0;   // batch windows: output chunks
    int64_t nops = 0, nrows = 0;
  };
  // output chunks of the push
  int64_t chunks(const Push& P) const {
    return batch ? P.nflush : P.nt + (partitioned ? (int64_t)P.nruns : (int64_t)P.ncalls);
  }

  void push(const Staged& b) override { run(b, false, 0); }

  void set_time(int64_t t) override {
    if (t < now) return;
    if ((timed() && plan.expired_on) ||
        ((wkind == SHD_W_TIME_BATCH || wkind == SHD_W_TIME_BATCH_STREAM) && !tb_notify.empty() &&
         tb_notify.front() <= t)) {
      Staged z;
      z.n = 0;
      z.call_offsets = {0, 0};
      z.advance_time = true;
      run(z, true, t);
    } else {
      now = t;
    }
  }

  void run(const Staged& b, bool extra_move, int64_t extra_t) {
    Push P{b, extra_move, extra_t, b.n};
    SHD_HIP(hipEventRecord(ev0, stream));
    stage_begin();
    push_calls(P);
    push_filter(P);
    mark("filter");
    push_items(P);
    mark("window_items");
    push_segments(P);
    mark("segments");
    if (batch) {
      batch_operations(P);
    } else {
      expiry(P);
      mark("expiry");
      timer_order(P);
      sliding_operations(P);
    }
    mark("operations");
    push_fold(P);   // marks "fold" when the push has operations
    push_emit(P);
    mark("emit");
    push_carry(P);
    mark("carry");
    push_counters(P);
  }

  // calls and clock moves (TimestampGeneratorImpl.setCurrentTimestamp per call, playback)
  void push_calls(Push& P) {
    const int64_t n = P.n;
    h_offs = P.b.call_offsets;
    if (h_offs.size() < 2) h_offs = {0, n};
    const int ncalls = P.ncalls = (int)h_offs.size() - 1;
    upload(d_offs, h_offs);
    d_call_of.reserve(std::max<int64_t>(n, 1) * 4);
    d_last.reserve((size_t)ncalls * 8);
    std::vector<int64_t> last(ncalls, INT64_MIN);
    if (n > 0) {
      launch_grid(k_call_of, (unsigned)ncalls, d_offs.as<int64_t>(), ncalls, P.b.cs.ts, d_call_of.as<int32_t>(),
                  d_last.as<int64_t>());
      h_last.reserve((size_t)ncalls * 8);
      SHD_HIP(hipMemcpyAsync(h_last.p, d_last.p, (size_t)ncalls * 8, hipMemcpyDeviceToHost, stream));
      SHD_HIP(hipStreamSynchronize(stream));
      std::memcpy(last.data(), h_last.p, (size_t)ncalls * 8);
    }
    h_now.assign(ncalls, now);
    h_F.clear();
    h_fnow.clear();
    P.clk = now;
    P.moved.assign(ncalls, 0);
    for (int c = 0; c < ncalls; c++) {
      int64_t t = INT64_MIN;
      bool move = false;
      if (P.extra_move && c == 0) {
        t = P.extra_t;
        move = true;
      } else if (P.b.advance_time && h_offs[c + 1] > h_offs[c]) {
        t = last[c];
        move = true;   // InputHandler.send(Event[]) with events
      }
      if (move && t >= P.clk) {
        P.clk = t;
        h_F.push_back(c);
        h_fnow.push_back(t);
        P.moved[c] = 1;
      }
      h_now[c] = P.clk;
    }
    P.timers = timed() && plan.expired_on;
    if (!P.timers) {   // clock moves only matter to the TIMER chunks
      h_F.clear();
      h_fnow.clear();
    }
    upload(d_call_now, h_now);
    upload(d_F, h_F);
    upload(d_fnow, h_fnow);
    P.nf = (int)h_F.size();
  }

  // filter, partition key, partition runs
  void push_filter(Push& P) {
    const int64_t n = P.n;
    d_flags.reserve(std::max<int64_t>(n, 1));
    d_cnt.reserve(std::max<int64_t>(n, 1) * 4);
    d_off.reserve(std::max<int64_t>(n, 1) * 4);
    d_pkey.reserve(std::max<int64_t>(n, 1) * 8);
    XwArgs& xa = P.xa;
    xa.cs = P.b.cs;
    xa.es = dset();
    xa.filters = dfilters(filters);
    xa.partitioned = partitioned;
    if (partitioned) {
      xa.key = dexpr(key_expr);
      xa.key_col = key_col;
      xa.key_type = key_type;
    }
    xa.ngk = ngk;
    for (int g = 0; g < ngk; g++) {
      xa.group[g] = dexpr(gk_expr[g]);
      xa.group_col[g] = gk_col[g];
      xa.group_type[g] = gk_type[g];
    }
    xa.null_str_id = plan.null_str_id;
    xa.nagg = nagg;
    for (int g = 0; g < nagg; g++) {
      xa.has_arg[g] = plan.aggs[g].expr >= 0;
      if (xa.has_arg[g]) xa.agg_arg[g] = dexpr(plan.aggs[g].expr);
    }
    xa.ncols = ncols;
    xa.nw = nw;
    xa.C = C;
    xa.seq0 = seq;
    if (n <= 0) return;
    launch(k_xw_filter, n, dev_args(xa), n, d_flags.as<uint8_t>(), d_cnt.as<uint32_t>(), d_pkey.as<uint64_t>());
    P.m = scan(d_cnt.as<uint32_t>(), d_off.as<uint32_t>(), n);
    if (partitioned) {
      d_start.reserve(n * 4);
      d_run.reserve(n * 4);
      launch(k_run_starts, n, d_flags.as<uint8_t>(), d_pkey.as<uint64_t>(), d_call_of.as<int32_t>(), n,
             d_start.as<uint32_t>());
      // d_run: the exclusive count of run starts; run_ids() makes the inclusive ids of it
      P.nruns = scan(d_start.as<uint32_t>(), d_run.as<uint32_t>(), n);
    }
  }

  // new items [C, C + m) and their state ids
  void push_items(Push& P) {
    const int64_t n = P.n, m = P.m;
    P.total = C + m;
    if (P.total >= (int64_t)INT32_MAX) throw Error(SHD_E_CAPACITY, "window items exceed 2^31");
    ensure_items(std::max<int64_t>(P.total, 1));
    P.cap = P.xa.cap = items.cap[items.cur];
    P.it = items.ptrs(items.cur);
    if (m > 0) {
      kw.reserve((size_t)std::max(nw, 1) * m * 8);
      kn.reserve(m);
      kh.reserve(m * 8);
      const ItemOut io{P.it, kw.as<uint64_t>(), kn.as<uint8_t>(), kh.as<uint64_t>()};
      const XwArgs* d_xa = dev_args(P.xa);
      launch(k_xw_items, n, d_xa, dev_args(io), n, d_cnt.as<uint32_t>(), d_off.as<uint32_t>(), d_pkey.as<uint64_t>(),
             d_call_of.as<int32_t>(), m);
      if (nw > 0) {
        gd.nk = nw;
        gd.assign(m, kh.as<uint64_t>(), kw.as<uint64_t>(), kn.as<uint8_t>(), m, P.it.sid, C, stream);
      } else {
        launch(k_fill_u64, m, P.it.sid + C, m, 0);
      }
    }
    ensure_states(nw > 0 ? std::max<int64_t>(gd.count, 1) : 1);
  }

  // key segments: stable sort by partition key (carried first, FIFO kept)
  void push_segments(Push& P) {
    hipStream_t s = stream;
    const int64_t total = P.total;
    sp.reserve(std::max<int64_t>(total, 1) * 4);
    if (total > 0) {
      fill_iota_u32(sp.as<uint32_t>(), total, 0, s);
      spk.reserve(total * 8);
      SHD_HIP(hipMemcpyAsync(spk.p, P.it.pk, total * 8, hipMemcpyDeviceToDevice, s));
      const uint32_t* spv = sp.as<uint32_t>();
      const uint64_t* spkv = spk.as<uint64_t>();
      if (partitioned) {
        tot.reserve();
        reduce_max_u64(P.it.pk, total, &tot.dev()->kmax, s);
        tot.fetch(&WindowTotals::kmax, s);
        SHD_HIP(hipStreamSynchronize(s));
        spk2.reserve(total * 8);
        sp2.reserve(total * 4);
        spv = sort_u64(spk, sp, spk2, sp2, total, bits_for(tot.host().kmax), &spkv);
      }
      head.reserve(total * 4);
      hscan.reserve(total * 4);
      launch(k_seg_heads_u64, total, spkv, total, head.as<uint32_t>());
      P.nseg = scan(head.as<uint32_t>(), hscan.as<uint32_t>(), total);
      segS.reserve((P.nseg + 1) * 8);
      segid.reserve(total * 4);
      launch(k_xw_seg_list, total, head.as<uint32_t>(), hscan.as<uint32_t>(), total, segS.as<int64_t>(),
             segid.as<uint32_t>());
      if (spv != sp.as<uint32_t>()) SHD_HIP(hipMemcpyAsync(sp.p, spv, total * 4, hipMemcpyDeviceToDevice, s));
    }
    P.SP = sp.as<uint32_t>();
    const int64_t nseg = P.nseg;
    segCk.reserve((nseg + 1) * 8);
    pA.reserve((nseg + 1) * 8);
    pB.reserve((nseg + 1) * 8);
    proom.reserve((nseg + 1) * 4);
    proom_off.reserve((nseg + 1) * 4);
    if (nseg > 0)
      launch(k_xw_seg_info, nseg, nseg, segS.as<int64_t>(), P.SP, C, P.it.pk, ppk.as<uint64_t>(), np,
             segCk.as<int64_t>(), pA.as<int64_t>(), pB.as<int64_t>(), proom.as<uint32_t>());
  }

  // sliding windows: each item's expiry opportunity
  void expiry(Push& P) {
    hipStream_t s = stream;
    const int64_t total = P.total, nseg = P.nseg;
    eopp.reserve(std::max<int64_t>(total, 1) * 8);
    etid.reserve(std::max<int64_t>(total, 1) * 4);
    if (total > 0 && wkind == SHD_W_LENGTH) {
      launch(k_xw_len_expiry, total, total, wparam, segS.as<int64_t>(), segid.as<uint32_t>(), P.SP, P.it.row,
             eopp.as<uint64_t>(), etid.as<uint32_t>());
    } else if (total > 0 && time_like()) {
      const uint32_t room = nseg > 0 ? scan(proom.as<uint32_t>(), proom_off.as<uint32_t>(), nseg) : 0;
      rec.reserve(total);
      tF.reserve((np + P.m + 1) * 4);
      tHead.reserve((np + P.m + 1) * 8);
      tSeg.reserve((np + P.m + 1) * 4);
      ntimer.reserve(64);
      pout_pk.reserve(std::max<uint32_t>(room, 1) * 8);
      pout_v.reserve(std::max<uint32_t>(room, 1) * 8);
      pcnt.reserve((nseg + 1) * 4);
      pcnt_off.reserve((nseg + 1) * 4);
      last_out.reserve((nseg + 1) * 8);
      SHD_HIP(hipMemsetAsync(ntimer.p, 0, 4, s));
      LaneArgs la{};
      la.nseg = nseg;
      la.segS = segS.as<int64_t>();
      la.segCk = segCk.as<int64_t>();
      la.pA = pA.as<int64_t>();
      la.pB = pB.as<int64_t>();
      la.proom_off = proom_off.as<uint32_t>();
      la.sp = P.SP;
      la.ipk = P.it.pk;
      la.its = P.it.ts;
      la.icall = P.it.call;
      la.irow = P.it.row;
      la.ilast = P.it.last;
      la.call_now = d_call_now.as<int64_t>();
      la.offs = d_offs.as<int64_t>();
      la.F = d_F.as<int32_t>();
      la.fnow = d_fnow.as<int64_t>();
      la.nf = P.nf;
      la.T = wparam;
      la.L = wkind == SHD_W_TIME_LENGTH ? wparam2 : 0;
      la.ext_col = wkind == SHD_W_EXTERNAL_TIME ? (int)wparam2 : -1;
      la.iattr = P.it.attr;
      la.cap = P.cap;
      la.partitioned = partitioned;
      la.last_global = last_global;
      la.pv = pv.as<int64_t>();
      la.eopp = eopp.as<uint64_t>();
      la.etid = etid.as<uint32_t>();
      la.rec = rec.as<uint8_t>();
      la.ntimer = ntimer.as<unsigned int>();
      la.tF = tF.as<int32_t>();
      la.tHead = tHead.as<int64_t>();
      la.tSeg = tSeg.as<uint32_t>();
      la.pout_pk = pout_pk.as<uint64_t>();
      la.pout_v = pout_v.as<int64_t>();
      la.pcnt = pcnt.as<uint32_t>();
      la.last_out = last_out.as<int64_t>();
      launch(k_xw_time_lane, nseg, dev_args(la));
      tot.reserve();
      P.nt = read_u32(ntimer.p, &tot.host().n_timer);
      P.lane_ran = true;
    } else if (total > 0) {   // no window: items never expire
      launch(k_fill_u64, total, eopp.as<uint64_t>(), total, kNoOpp);
      SHD_HIP(hipMemsetAsync(etid.p, 0xFF, total * 4, s));
    }
  }

  // timers in (call, notify head, key) order: the TIMER chunks' order
  // (Scheduler.onTimeChange: sortedExpires by time; ties by key order)
  void timer_order(Push& P) {
    hipStream_t s = stream;
    const int64_t nt = P.nt;
    trank.reserve(std::max<int64_t>(nt, 1) * 4);
    sF.reserve(std::max<int64_t>(nt, 1) * 4);
    if (nt <= 0) return;
    tperm.reserve(nt * 4);
    tperm2.reserve(nt * 4);
    tk32.reserve(nt * 4);
    tk32b.reserve(nt * 4);
    tk64.reserve(nt * 8);
    tk64b.reserve(nt * 8);
    fill_iota_u32(tperm.as<uint32_t>(), nt, 0, s);
    // a stable sort's permutation, left in tperm
    auto settle = [&](const uint32_t* perm) {
      if (perm != tperm.as<uint32_t>()) SHD_HIP(hipMemcpyAsync(tperm.p, perm, nt * 4, hipMemcpyDeviceToDevice, s));
    };
    // 1) by segment (key order)
    SHD_HIP(hipMemcpyAsync(tk32.p, tSeg.p, nt * 4, hipMemcpyDeviceToDevice, s));
    settle(sort_u32(tk32, tperm, tk32b, tperm2, nt, bits_for((uint64_t)P.nseg), nullptr));
    // 2) by notify head (signed -> order-preserving unsigned)
    launch(k_xw_gather_u64, nt, tHead.as<uint64_t>(), tperm.as<uint32_t>(), tk64.as<uint64_t>(), nt,
           0x8000000000000000ull);
    settle(sort_u64(tk64, tperm, tk64b, tperm2, nt, 64, nullptr));
    // 3) by call
    launch(k_xw_gather_u32, nt, tF.as<uint32_t>(), tperm.as<uint32_t>(), tk32.as<uint32_t>(), nt);
    settle(sort_u32(tk32, tperm, tk32b, tperm2, nt, bits_for((uint64_t)P.ncalls), nullptr));
    launch(k_xw_timer_rank, nt, tperm.as<uint32_t>(), tF.as<int32_t>(), nt, trank.as<uint32_t>(), sF.as<int32_t>());
  }

  // sliding windows: the operations in key-major order
  void sliding_operations(Push& P) {
    hipStream_t s = stream;
    const int64_t n = P.n, total = P.total;
    // partition runs before each call (chunk ordinals of timer chunks)
    d_runs_before.reserve((size_t)P.ncalls * 8);
    if (partitioned && n > 0) {
      launch(k_xw_runs_before, P.ncalls, P.ncalls, d_offs.as<int64_t>(), n, d_run.as<uint32_t>(), P.nruns,
             d_runs_before.as<uint64_t>());
    } else if (partitioned) {
      SHD_HIP(hipMemsetAsync(d_runs_before.p, 0, (size_t)P.ncalls * 8, s));
    }
    nops_b.reserve(std::max<int64_t>(total, 1) * 4);
    opscan.reserve(std::max<int64_t>(total, 1) * 4);
    if (total > 0) {
      launch(k_xw_nops, total, total, C, P.SP, eopp.as<uint64_t>(), nops_b.as<uint32_t>());
      P.nops = scan(nops_b.as<uint32_t>(), opscan.as<uint32_t>(), total);
    }
    if (partitioned && n > 0 && P.nruns > 0) run_ids(n);
    reserve_ops(P.nops);
    if (P.nops <= 0) return;
    OpArgs oa{};
    oa.total = total;
    oa.C = C;
    oa.sp = P.SP;
    oa.segid = segid.as<uint32_t>();
    oa.segS = segS.as<int64_t>();
    oa.segCk = segCk.as<int64_t>();
    oa.eopp = eopp.as<uint64_t>();
    oa.etid = etid.as<uint32_t>();
    oa.opscan = opscan.as<uint32_t>();
    oa.irow = P.it.row;
    oa.iseq = P.it.seq;
    oa.call_of = d_call_of.as<int32_t>();
    oa.call_now = d_call_now.as<int64_t>();
    oa.run_of = partitioned ? d_start.as<uint32_t>() : nullptr;
    oa.offs = d_offs.as<int64_t>();
    oa.fnow_of_call = d_call_now.as<int64_t>();
    oa.trank = trank.as<uint32_t>();
    oa.sF = sF.as<int32_t>();
    oa.nt = P.nt;
    oa.runs_before = d_runs_before.as<uint64_t>();
    oa.partitioned = partitioned;
    oa.row_now = wkind == SHD_W_EXTERNAL_TIME ? reinterpret_cast<const int64_t*>(P.b.cs.col[wparam2]) : nullptr;
    oa.current_on = plan.current_on;
    oa.expired_on = plan.expired_on;
    oa.seq0 = seq;
    oa.op_item = op_item.as<uint32_t>();
    oa.op_add = op_add.as<uint8_t>();
    oa.op_on = op_on.as<uint8_t>();
    oa.op_chunk = op_chunk.as<uint32_t>();
    oa.op_now = op_now.as<int64_t>();
    oa.op_seq = op_seq.as<int64_t>();
    launch(k_xw_ops, total, dev_args(oa));
  }

  void reserve_ops(int64_t nops) {
    const int64_t nop_alloc = std::max<int64_t>(nops, 1);
    op_item.reserve(nop_alloc * 4);
    op_add.reserve(nop_alloc);
    op_on.reserve(nop_alloc);
    op_chunk.reserve(nop_alloc * 4);
    op_now.reserve(nop_alloc * 8);
    op_seq.reserve(nop_alloc * 8);
  }

  // TimeBatchWindowProcessor.process (:279-366) for one chunk at clock t:
  // nextEmitTime set up by the first chunk; a flush when t reached it
  bool tb_process(int64_t t) {
    const int64_t T = wparam;
    if (tb_next == -1) {
      if (wparam2 != INT64_MIN) tb_next = t + (T - (t - wparam2) % T);   // getNextEmitTime (:368-373)
      else tb_next = t + T;
      tb_notify.push_back(tb_next);
    }
    if (t >= tb_next) {
      tb_next += T;
      tb_notify.push_back(tb_next);
      return true;
    }
    return false;
  }

  // Batch windows: the push's output chunks (ordinals 0..nflush-1 in output
  // order: flushes, or every event / call in the stream modes), each item's
  // add / expiry chunk and RESET epoch, the operations in key-major order
  // (k_xb_ops).
  void batch_operations(Push& P) {
    const int64_t total = P.total, ta = std::max<int64_t>(total, 1);
    xb_added.reserve(ta);
    xb_aopp.reserve(ta * 8);
    eopp.reserve(ta * 8);
    xb_epoch.reserve(ta * 8);
    xb_keep.reserve(ta);
    xb_last.reserve(ta * 8);
    if (total > 0) launch(k_xb_added, total, total, C, P.SP, P.it.last, xb_added.as<uint8_t>());
    XbArgs xb{};
    xb.total = total;
    xb.C = C;
    xb.L = std::max<int64_t>(wparam, 1);
    xb.expired_on = plan.expired_on;
    xb.sp = P.SP;
    xb.segid = segid.as<uint32_t>();
    xb.segS = segS.as<int64_t>();
    xb.segCk = segCk.as<int64_t>();
    xb.added_j = xb_added.as<uint8_t>();
    xb.irow = P.it.row;
    xb.icall = P.it.call;
    xb.ilast = P.it.last;
    xb.chunk0 = chunk_seq;
    xb.first_flush = -1;
    xb.aopp = xb_aopp.as<uint64_t>();
    xb.eopp = eopp.as<uint64_t>();
    xb.epoch_j = xb_epoch.as<int64_t>();
    xb.keep_j = xb_keep.as<uint8_t>();
    xb.last_j = xb_last.as<int64_t>();
    if (bmode == XB_FULL_LEN) P.nflush = len_flushes(P, xb);
    else if (bmode == XB_FULL_EXT) P.nflush = ext_flushes(P, xb);
    else if (bmode == XB_STREAM_LEN || bmode == XB_ZERO_LEN) P.nflush = item_chunks(P);
    else P.nflush = time_flushes(P, xb);
    if (total > 0) launch(k_xb_opp, total, dev_args(xb), bmode);
    nops_b.reserve(ta * 4);
    opscan.reserve(ta * 4);
    if (total > 0) {
      launch(k_xb_nops, total, total, xb_aopp.as<uint64_t>(), eopp.as<uint64_t>(), nops_b.as<uint32_t>());
      P.nops = scan(nops_b.as<uint32_t>(), opscan.as<uint32_t>(), total);
    }
    reserve_ops(P.nops);
    op_epoch.reserve(std::max<int64_t>(P.nops, 1) * 8);
    if (P.nops <= 0) return;
    XbOpArgs oa{};
    oa.total = total;
    oa.sp = P.SP;
    oa.segid = segid.as<uint32_t>();
    oa.segS = segS.as<int64_t>();
    oa.segCk = segCk.as<int64_t>();
    oa.added_j = xb_added.as<uint8_t>();
    oa.aopp = xb_aopp.as<uint64_t>();
    oa.eopp = eopp.as<uint64_t>();
    oa.epoch_j = xb_epoch.as<int64_t>();
    oa.full = bmode == XB_FULL_LEN || bmode == XB_FULL_TIME || bmode == XB_FULL_EXT;
    oa.opscan = opscan.as<uint32_t>();
    oa.fnow = xb_fnow.as<int64_t>();
    oa.fseq = xb_fseq.as<int64_t>();
    oa.current_on = plan.current_on;
    oa.expired_on = plan.expired_on;
    oa.op_epoch = op_epoch.as<int64_t>();
    oa.op_item = op_item.as<uint32_t>();
    oa.op_add = op_add.as<uint8_t>();
    oa.op_on = op_on.as<uint8_t>();
    oa.op_chunk = op_chunk.as<uint32_t>();
    oa.op_now = op_now.as<int64_t>();
    oa.op_seq = op_seq.as<int64_t>();
    launch(k_xb_ops, total, dev_args(oa));
  }

  // lengthBatch: a flush per completed batch, ranked by its trigger row.
  // Returns the flush count, as the next three do.
  int64_t len_flushes(Push& P, XbArgs& xb) {
    const int64_t n = P.n;
    xb_trig.reserve(std::max<int64_t>(n, 1) * 4);
    xb_fr.reserve(std::max<int64_t>(n, 1) * 4);
    if (n > 0) SHD_HIP(hipMemsetAsync(xb_trig.p, 0, n * 4, stream));
    if (P.total > 0) launch(k_xb_len_trig, P.total, dev_args(xb), xb_trig.as<uint32_t>());
    const int64_t nflush = n > 0 ? scan(xb_trig.as<uint32_t>(), xb_fr.as<uint32_t>(), n) : 0;
    xb_fnow.reserve(std::max<int64_t>(nflush, 1) * 8);
    xb_fseq.reserve(std::max<int64_t>(nflush, 1) * 8);
    if (nflush > 0)
      launch(k_xb_len_flushes, n, n, xb_trig.as<uint32_t>(), xb_fr.as<uint32_t>(), d_call_of.as<int32_t>(),
             d_call_now.as<int64_t>(), seq, xb_fnow.as<int64_t>(), xb_fseq.as<int64_t>());
    xb.fr = xb_fr.as<uint32_t>();
    return nflush;
  }

  // lengthBatch stream / zero modes: an output chunk per event (its rank among the push's new items)
  int64_t item_chunks(Push& P) {
    const int64_t m = P.m;
    xb_fnow.reserve(std::max<int64_t>(m, 1) * 8);
    xb_fseq.reserve(std::max<int64_t>(m, 1) * 8);
    if (m > 0)
      launch(k_xb_item_chunks, m, C, m, P.it.call, P.it.row, d_call_now.as<int64_t>(), seq, xb_fnow.as<int64_t>(),
             xb_fseq.as<int64_t>());
    return m;
  }

  // timeBatch: the flush schedule is sequential in the chunks (calls and
  // TIMER chunks), not in the events: run it on the host per call
  int64_t time_flushes(Push& P, XbArgs& xb) {
    hipStream_t s = stream;
    const int ncalls = P.ncalls;
    xb_ccount.reserve((size_t)ncalls * 4);
    xb_clast.reserve((size_t)ncalls * 8);
    SHD_HIP(hipMemsetAsync(xb_ccount.p, 0, (size_t)ncalls * 4, s));
    if (P.m > 0)
      launch(k_xb_call_items, P.m, C, P.m, P.it.call, P.it.row, seq, xb_ccount.as<uint32_t>(), xb_clast.as<int64_t>());
    std::vector<uint32_t> cc(ncalls);
    std::vector<int64_t> cl(ncalls);
    h_pin.reserve((size_t)ncalls * 12);
    SHD_HIP(hipMemcpyAsync(h_pin.p, xb_ccount.p, (size_t)ncalls * 4, hipMemcpyDeviceToHost, s));
    SHD_HIP(hipMemcpyAsync(h_pin.as<char>() + (size_t)ncalls * 4, xb_clast.p, (size_t)ncalls * 8,
                           hipMemcpyDeviceToHost, s));
    SHD_HIP(hipStreamSynchronize(s));
    std::memcpy(cc.data(), h_pin.p, (size_t)ncalls * 4);
    std::memcpy(cl.data(), h_pin.as<char>() + (size_t)ncalls * 4, (size_t)ncalls * 8);
    const bool stream_cur = bmode == XB_STREAM_TIME;
    // per call: full batches -- the flush its events join; stream mode -- its
    // chunk, the first flush at or after it, its RESET epoch
    std::vector<int32_t> bfl(ncalls, -1), cch(ncalls, -1), cfl(ncalls, -1);
    std::vector<int64_t> cep(ncalls, -1), fn, fs;
    std::vector<int> pending;
    auto flush_here = [&](int64_t t, int64_t sq) {   // a flush ends the current chunk list
      const int32_t f = (int32_t)fn.size();
      for (int pc : pending) (stream_cur ? cfl : bfl)[pc] = f;
      pending.clear();
      fn.push_back(t);
      fs.push_back(sq);
      if (stream_cur) tb_epoch = chunk_seq + f;   // RESET after this chunk's expirations
    };
    for (int c = 0; c < ncalls; c++) {
      if (P.moved[c]) {
        // Scheduler.sendTimerEvents (C/util/Scheduler.java:190-220): TIMER
        // chunks while the queue head is due, each through the window
        const int64_t t = h_now[c];
        while (!tb_notify.empty() && tb_notify.front() <= t) {
          tb_notify.pop_front();
          if (tb_process(t)) {
            if (xb.first_flush < 0) xb.first_flush = (int64_t)fn.size();
            flush_here(t, seq + h_offs[c]);
          }
        }
      }
      if (cc[c] > 0) {   // a chunk of events reaches the window
        pending.push_back(c);
        const bool send = tb_process(h_now[c]);
        if (stream_cur) {   // the call is a chunk of its own (its events stay in it)
          cch[c] = (int32_t)fn.size();
          cep[c] = tb_epoch;
          fn.push_back(h_now[c]);
          fs.push_back(cl[c]);
          if (send) {   // expirations appended to the same chunk
            for (int pc : pending) cfl[pc] = cch[c];
            pending.clear();
            if (xb.first_flush < 0) xb.first_flush = cch[c];
            tb_epoch = chunk_seq + cch[c];
          }
        } else if (send) {
          flush_here(h_now[c], cl[c]);
        }
      }
    }
    const int64_t nflush = (int64_t)fn.size();
    upload(xb_fnow, fn);
    upload(xb_fseq, fs);
    if (stream_cur) {
      upload(xb_cchunk, cch);
      upload(xb_cflush, cfl);
      upload(xb_cepoch, cep);
      xb.cchunk = xb_cchunk.as<int32_t>();
      xb.cflush = xb_cflush.as<int32_t>();
      xb.cepoch = xb_cepoch.as<int64_t>();
    } else {
      upload(xb_bflush, bfl);
      xb.bflush = xb_bflush.as<int32_t>();
      xb.nf = nflush;
    }
    return nflush;
  }

  // externalTimeBatch: where the flushes fall (k_etb_*), ranked by trigger row;
  // the keys' carried timing for the next push
  int64_t ext_flushes(Push& P, XbArgs& xb) {
    const int64_t n = P.n, total = P.total, nseg = P.nseg;
    xb_trig.reserve(std::max<int64_t>(n, 1) * 4);
    xb_fr.reserve(std::max<int64_t>(n, 1) * 4);
    xb_fnow.reserve(std::max<int64_t>(n, 1) * 8);
    xb_fseq.reserve(std::max<int64_t>(n, 1) * 8);
    if (total <= 0 || nseg <= 0) return 0;
    const int64_t nt = ceil_div(total, kEtbTile);
    etb_M.reserve(total * 8);
    etb_head.reserve(total * 4);
    etb_E.reserve(total * 8);
    etb_trigj.reserve(total * 4);
    etb_tjx.reserve(total * 4);
    etb_tpos.reserve(total * 4);
    etb_tv.reserve(nt * 8);
    etb_tf.reserve(nt * 4);
    etb_seg_start.reserve(nseg * 8);
    etb_seg_end.reserve(nseg * 8);
    etb_seg_j1.reserve(nseg * 8);
    if (n > 0) SHD_HIP(hipMemsetAsync(xb_trig.p, 0, n * 4, stream));
    EtbArgs ea{};
    ea.total = total;
    ea.C = C;
    ea.T = wparam;
    ea.cap = P.cap;
    ea.nseg = nseg;
    ea.seq0 = seq;
    ea.ts_col = etb_ts_col;
    ea.start_mode = etb_start_mode;
    ea.start_col = etb_start_col;
    ea.replace = etb_replace;
    ea.start_const = etb_start_const;
    ea.sp = P.SP;
    ea.segid = segid.as<uint32_t>();
    ea.segS = segS.as<int64_t>();
    ea.segCk = segCk.as<int64_t>();
    ea.pA = pA.as<int64_t>();
    ea.pB = pB.as<int64_t>();
    ea.pv = pv.as<int64_t>();
    ea.irow = P.it.row;
    ea.iattr = P.it.attr;
    ea.inul = P.it.nul;
    ea.M = etb_M.as<int64_t>();
    ea.head = etb_head.as<uint32_t>();
    ea.E = etb_E.as<int64_t>();
    ea.trig_j = etb_trigj.as<uint32_t>();
    ea.trig_r = xb_trig.as<uint32_t>();
    ea.seg_start = etb_seg_start.as<int64_t>();
    ea.seg_end = etb_seg_end.as<int64_t>();
    ea.seg_j1 = etb_seg_j1.as<int64_t>();
    const EtbArgs* d_ea = dev_args(ea);
    launch(k_etb_seed, total, d_ea);
    launch_grid(k_etb_pmax_tiles, (unsigned)nt, etb_M.as<int64_t>(), etb_head.as<uint32_t>(), total,
                etb_tv.as<int64_t>(), etb_tf.as<uint32_t>());
    launch_grid(k_etb_pmax_scan, 1, etb_tv.as<int64_t>(), etb_tf.as<uint32_t>(), nt);
    launch_grid(k_etb_pmax_apply, (unsigned)nt, etb_M.as<int64_t>(), etb_head.as<uint32_t>(), total,
                etb_tv.as<int64_t>());
    launch(k_etb_lane, nseg, d_ea);
    launch(k_etb_trig, total, d_ea);
    // flushes in trigger-row order; per key, the triggers' sorted positions
    const int64_t nflush = n > 0 ? scan(xb_trig.as<uint32_t>(), xb_fr.as<uint32_t>(), n) : 0;
    scan(etb_trigj.as<uint32_t>(), etb_tjx.as<uint32_t>(), total);   // the same count, in key order
    if (nflush > 0) {
      launch(k_head_list, total, etb_trigj.as<uint32_t>(), etb_tjx.as<uint32_t>(), total, etb_tpos.as<uint32_t>());
      launch(k_etb_flushes, total, d_ea, xb_fr.as<uint32_t>(), xb_fnow.as<int64_t>(), xb_fseq.as<int64_t>());
    }
    ppk2.reserve(nseg * 24);
    pv2.reserve(nseg * 24);
    launch(k_etb_state, nseg, d_ea, P.it.pk, ppk2.as<uint64_t>(), pv2.as<int64_t>());
    if (etb_replace) launch(k_etb_replace, total, d_ea);
    SHD_HIP(hipStreamSynchronize(stream));
    ppk.swap(ppk2);
    pv.swap(pv2);
    np = 3 * nseg;
    xb.fr = xb_fr.as<uint32_t>();
    xb.nf = nflush;
    xb.trig_j = etb_trigj.as<uint32_t>();
    xb.tjx = etb_tjx.as<uint32_t>();
    xb.tpos = etb_tpos.as<uint32_t>();
    return nflush;
  }

  // inclusive run id of each keyed event into d_start (k_xw_ops' run_of):
  // exclusive count + own start - 1
  void run_ids(int64_t n) { launch(k_xw_run_ids, n, n, d_run.as<uint32_t>(), d_start.as<uint32_t>()); }

  int64_t scan_u8_flags(const uint8_t* f, int64_t n) {
    nops_b.reserve(n * 4);
    launch(k_xw_widen, n, f, n, nops_b.as<uint32_t>());
    return scan(nops_b.as<uint32_t>(), roff.as<uint32_t>(), n);
  }

  // selector: aggregator folds and the rows each chunk emits
  void push_fold(Push& P) {
    const int64_t nops = P.nops, nop_alloc = std::max<int64_t>(nops, 1);
    const int na = std::max(nagg, 1);
    rowflag.reserve(nop_alloc);
    rowsrc.reserve(nop_alloc * 4);
    resv.reserve((size_t)na * nop_alloc * 8);
    resn.reserve((size_t)na * nop_alloc);
    if (nops <= 0) return;
    FoldArgsX fa{};
    fa.nagg = nagg;
    for (int g = 0; g < nagg; g++) {
      fa.kind[g] = plan.aggs[g].kind;
      fa.type[g] = plan.aggs[g].type;
    }
    fa.group = group;
    fa.cap = P.cap;
    fa.nops = nops;
    fa.nstates = nstates;
    fa.argv = P.it.argv;
    fa.argn = P.it.argn;
    fa.op_item = op_item.as<uint32_t>();
    fa.op_add = op_add.as<uint8_t>();
    fa.op_on = op_on.as<uint8_t>();
    fa.op_chunk = op_chunk.as<uint32_t>();
    fa.op_now = op_now.as<int64_t>();
    fa.its = P.it.ts;
    fa.attr = P.it.attr;
    fa.nul = P.it.nul;
    fa.ncols = ncols;
    fa.es = dset();
    fa.has_having = plan.having >= 0;
    if (fa.has_having) fa.having = dexpr(plan.having);
    fa.dsum = g_dsum.as<double>();
    fa.lsum = g_lsum.as<int64_t>();
    fa.cnt = g_cnt.as<int64_t>();
    fa.epoch = (batch && nagg > 0) ? g_epoch.as<int64_t>() : nullptr;
    fa.op_epoch = op_epoch.as<int64_t>();
    fa.resv = resv.as<uint64_t>();
    fa.resn = resn.as<uint8_t>();
    fa.rowflag = rowflag.as<uint8_t>();
    fa.rowsrc = rowsrc.as<uint32_t>();
    if (plain) {
      launch(k_xw_plain_rows, nops, dev_args(fa));
    } else {
      // one lane per state: the operations grouped by state id, in order
      SHD_HIP(hipMemsetAsync(rowflag.p, 0, nops, stream));
      osid.reserve(nops * 4);
      osid2.reserve(nops * 4);
      oq.reserve(nops * 4);
      oq2.reserve(nops * 4);
      launch(k_xw_op_sid, nops, nops, op_item.as<uint32_t>(), P.it.sid, osid.as<uint32_t>());
      fill_iota_u32(oq.as<uint32_t>(), nops, 0, stream);
      const uint32_t* ssid = nullptr;
      const uint32_t* sq =
          sort_u32(osid, oq, osid2, oq2, nops, bits_for((uint64_t)std::max<int64_t>(gd.count, 1)), &ssid);
      ohead.reserve(nops * 4);
      ohoff.reserve(nops * 4);
      launch(k_seg_heads, nops, ssid, nops, ohead.as<uint32_t>());
      const int64_t nheads = scan(ohead.as<uint32_t>(), ohoff.as<uint32_t>(), nops);
      ohl.reserve(std::max<int64_t>(nheads, 1) * 4);
      launch(k_head_list, nops, ohead.as<uint32_t>(), ohoff.as<uint32_t>(), nops, ohl.as<uint32_t>());
      if (!mm && !xa) {
        launch(k_xw_fold<false>, nheads, dev_args(fa), ohl.as<uint32_t>(), nheads, ssid, sq);
      } else {
        fold_minmax(fa, nheads, ssid, sq);
      }
    }
    mark("fold");
    roff.reserve(nops * 4);
    P.nrows = scan_u8_flags(rowflag.as<uint8_t>(), nops);
  }

  // The fold of a plan with min / max (or stdDev / distinctCount / and / or)
  // aggregators.  Tracking deques and distinctCount key lists: every
  // lane (a state with operations in this push) gets one region per list,
  // sized by its carried length plus its operations and placed by one
  // exclusive scan, so no lane allocates or waits; after the fold the deques of
  // all states -- folded ones from the work area, the rest from the old slot --
  // are packed into the other slot of the store (lengths, scan, copy).
  void fold_minmax(FoldArgsX& fa, int64_t nheads, const uint32_t* ssid, const uint32_t* sq) {
    const int64_t nops = fa.nops;
    const int64_t ncell = (int64_t)ndq * nstates;
    fa.ndq = ndq;
    for (int g = 0; g < nagg; g++) fa.dq[g] = dq_of[g];
    DqEsz esz{};
    for (int k = 0; k < ndq; k++) esz.v[k] = fa.dq_esz[k] = dq_esz[k];
    if (ndq > 0) {
      if ((int64_t)dq_words * nops + dq_total >= (int64_t)INT32_MAX)
        throw Error(SHD_E_CAPACITY, "aggregator lists (min / max deques, distinctCount keys) exceed 2^31 values");
      const int64_t nr = nheads * ndq;
      dq_room.reserve(nr * 4);
      dq_woff.reserve(nr * 4);
      launch(k_xw_dq_room, nheads, ohl.as<uint32_t>(), nheads, nops, ssid, ndq, esz, nstates, dq_len.as<uint32_t>(),
             dq_room.as<uint32_t>());
      const int64_t wtotal = scan(dq_room.as<uint32_t>(), dq_woff.as<uint32_t>(), nr);
      dq_work.reserve(std::max<int64_t>(wtotal, 1) * 8);
      dq_val[dq_cur].reserve(8);
      dq_nlen.reserve(ncell * 4);
      dq_noff.reserve(ncell * 4);
      dq_nsrc.reserve(ncell * 4);
      SHD_HIP(hipMemcpyAsync(dq_nlen.p, dq_len.p, ncell * 4, hipMemcpyDeviceToDevice, stream));
      SHD_HIP(hipMemcpyAsync(dq_nsrc.p, dq_off.p, ncell * 4, hipMemcpyDeviceToDevice, stream));
      fa.dq_len = dq_len.as<uint32_t>();
      fa.dq_off = dq_off.as<uint32_t>();
      fa.dq_val = dq_val[dq_cur].as<uint64_t>();
      fa.dq_woff = dq_woff.as<uint32_t>();
      fa.dq_work = dq_work.as<uint64_t>();
      fa.dq_nlen = dq_nlen.as<uint32_t>();
      fa.dq_nsrc = dq_nsrc.as<uint32_t>();
    }
    if (xa) launch(k_xw_fold<true, true>, nheads, dev_args(fa), ohl.as<uint32_t>(), nheads, ssid, sq);
    else launch(k_xw_fold<true>, nheads, dev_args(fa), ohl.as<uint32_t>(), nheads, ssid, sq);
    if (ndq == 0) return;
    const int64_t ntotal = scan(dq_nlen.as<uint32_t>(), dq_noff.as<uint32_t>(), ncell);
    const int oth = dq_cur ^ 1;
    if ((int64_t)(dq_val[oth].cap / 8) < ntotal)
      dq_val[oth].reserve((size_t)std::max<int64_t>(ntotal, std::max<int64_t>(1024, (int64_t)(dq_val[oth].cap / 8) * 2)) * 8);
    if (ntotal > 0)
      launch(k_xw_dq_pack, ntotal, ntotal, ncell, dq_noff.as<uint32_t>(), dq_nsrc.as<uint32_t>(),
             dq_val[dq_cur].as<uint64_t>(), dq_work.as<uint64_t>(), dq_val[oth].as<uint64_t>());
    dq_len.swap(dq_nlen);
    dq_off.swap(dq_noff);
    dq_cur = oth;
    dq_total = ntotal;
  }

  // rows in (chunk, position) order
  void push_emit(Push& P) {
    const int64_t nrows = P.nrows, nops = P.nops;
    if (nrows <= 0) return;
    rkey.reserve(nrows * 8);
    rkey2.reserve(nrows * 8);
    rq.reserve(nrows * 4);
    rq2.reserve(nrows * 4);
    launch(k_xw_row_keys, nops, nops, rowflag.as<uint8_t>(), roff.as<uint32_t>(), op_chunk.as<uint32_t>(),
           rkey.as<uint64_t>(), rq.as<uint32_t>());
    const uint32_t* RQ = sort_u64(rkey, rq, rkey2, rq2, nrows, 32 + bits_for((uint64_t)chunks(P)), nullptr);
    out.ensure(nrows, stream);
    EmitArgsX ea{};
    ea.es = dset();
    ea.nout = (int)plan.outputs.size();
    for (int c = 0; c < ea.nout; c++) ea.outs[c] = dexpr(plan.outputs[c].second);
    ea.nagg = nagg;
    ea.ncols = ncols;
    ea.cap = P.cap;
    ea.nops = nops;
    ea.row0 = out.count;
    ea.chunk0 = chunk_seq;
    ea.rowsrc = rowsrc.as<uint32_t>();
    ea.op_item = op_item.as<uint32_t>();
    ea.op_add = op_add.as<uint8_t>();
    ea.op_chunk = op_chunk.as<uint32_t>();
    ea.op_now = op_now.as<int64_t>();
    ea.op_seq = op_seq.as<int64_t>();
    ea.its = P.it.ts;
    ea.attr = P.it.attr;
    ea.nul = P.it.nul;
    ea.resv = resv.as<uint64_t>();
    ea.resn = resn.as<uint8_t>();
    launch(k_xw_emit, nrows, dev_args(ea), nrows, RQ, out.d_chunk(), out.d_type(), out.d_ts(), out.d_vals(),
           out.d_nulls(), out.d_seq(), out.d_sidx());
    out.count += nrows;
  }

  // carry: unexpired items (no window: nothing is kept; states persist); time
  // windows: the notify entries still queued and the window's last time
  void push_carry(Push& P) {
    const int64_t total = P.total;
    int64_t kept = 0;
    const int oth = items.cur ^ 1;
    if (total > 0) {
      keep.reserve(total * 4);
      koff.reserve(total * 4);
      if (batch) launch(k_xw_widen, total, xb_keep.as<uint8_t>(), total, keep.as<uint32_t>());
      else launch(k_xw_keep, total, total, eopp.as<uint64_t>(), wkind != 0 ? 1 : 0, keep.as<uint32_t>());
      kept = scan(keep.as<uint32_t>(), koff.as<uint32_t>(), total);
    }
    if (kept > 0) {
      if (items.cap[oth] < std::max<int64_t>(kept, 1024)) items.alloc(oth, std::max<int64_t>(kept * 2, 1024));
      CarryArgs ca{};
      ca.total = total;
      ca.cap_src = P.cap;
      ca.cap_dst = items.cap[oth];
      ca.ncols = ncols;
      ca.nagg = nagg;
      ca.sp = P.SP;
      ca.keep = keep.as<uint32_t>();
      ca.koff = koff.as<uint32_t>();
      ca.segid = segid.as<uint32_t>();
      ca.last_out = P.lane_ran ? last_out.as<int64_t>() : nullptr;
      ca.last_j = batch ? xb_last.as<int64_t>() : nullptr;
      ca.src = P.it;
      ca.dst = items.ptrs(oth);
      launch(k_xw_carry, total, dev_args(ca));
    }
    if (time_like() && P.timers) update_pending(P);
    if (time_like() && !partitioned && P.lane_ran && P.nseg > 0) {
      tot.reserve();
      SHD_HIP(hipMemcpyAsync(&tot.host().last_out, last_out.p, 8, hipMemcpyDeviceToHost, stream));
      SHD_HIP(hipStreamSynchronize(stream));
      last_global = tot.host().last_out;
    }
    items.cur = oth;
    C = kept;
  }

  void push_counters(Push& P) {
    SHD_HIP(hipEventRecord(ev1, stream));
    stage_end();
    SHD_HIP(hipEventSynchronize(ev1));
    float ms = 0.f;
    SHD_HIP(hipEventElapsedTime(&ms, ev0, ev1));
    counters.kernel_ns = (int64_t)(ms * 1e6);
    counters.kernel_ns_total += counters.kernel_ns;
    counters.events += P.n;
    counters.matches += P.nrows;
    counters.carry = C;
    counters.partial_scans += P.nops;
    chunk_seq += chunks(P);
    now = P.clk;
    seq += P.n;
  }

  // the notify entries still queued: the segments' remaining ones and the
  // orphans (queued entries of keys without items in this push)
  void update_pending(Push& P) {
    hipStream_t s = stream;
    const int64_t nseg = P.nseg;
    int64_t nseg_out = 0;
    if (P.lane_ran && nseg > 0) nseg_out = scan(pcnt.as<uint32_t>(), pcnt_off.as<uint32_t>(), nseg);
    okeep.reserve(std::max<int64_t>(np, 1) * 4);
    okoff.reserve(std::max<int64_t>(np, 1) * 4);
    seg_pk.reserve(std::max<int64_t>(nseg, 1) * 8);
    int64_t nork = 0;
    if (np > 0) {
      if (nseg > 0) launch(k_xw_seg_pk, nseg, nseg, segS.as<int64_t>(), P.SP, P.it.pk, seg_pk.as<uint64_t>());
      launch(k_xw_orphans, np, np, ppk.as<uint64_t>(), pv.as<int64_t>(), nseg, seg_pk.as<uint64_t>(), P.nf,
             d_fnow.as<int64_t>(), okeep.as<uint32_t>());
      nork = scan(okeep.as<uint32_t>(), okoff.as<uint32_t>(), np);
    }
    const int64_t nn = nseg_out + nork;
    ppk2.reserve(std::max<int64_t>(nn, 1) * 8);
    pv2.reserve(std::max<int64_t>(nn, 1) * 8);
    if (nseg_out > 0)
      launch(k_xw_pend_gather, nseg, nseg, proom_off.as<uint32_t>(), pcnt.as<uint32_t>(), pcnt_off.as<uint32_t>(),
             pout_pk.as<uint64_t>(), pout_v.as<int64_t>(), ppk2.as<uint64_t>(), pv2.as<int64_t>());
    if (nork > 0)
      launch(k_xw_pend_orphan_copy, np, np, okeep.as<uint32_t>(), okoff.as<uint32_t>(), nseg_out, ppk.as<uint64_t>(),
             pv.as<int64_t>(), ppk2.as<uint64_t>(), pv2.as<int64_t>());
    // both parts are key-sorted: one stable key sort merges them (values stay
    // in order inside a key: a key is in one part only)
    if (nseg_out > 0 && nork > 0) {
      pend_idx.reserve(nn * 4);
      pend_idx2.reserve(nn * 4);
      pend_key2.reserve(nn * 8);
      pend_tmp_pk.reserve(nn * 8);
      pend_tmp_v.reserve(nn * 8);
      fill_iota_u32(pend_idx.as<uint32_t>(), nn, 0, s);
      SHD_HIP(hipMemcpyAsync(pend_tmp_pk.p, ppk2.p, nn * 8, hipMemcpyDeviceToDevice, s));
      const uint32_t* perm = sort_u64(pend_tmp_pk, pend_idx, pend_key2, pend_idx2, nn, 64, nullptr);
      launch(k_gather_u64, nn, ppk2.as<uint64_t>(), perm, pend_tmp_pk.as<uint64_t>(), nn);
      launch(k_gather_u64, nn, pv2.as<uint64_t>(), perm, pend_tmp_v.as<uint64_t>(), nn);
      ppk2.swap(pend_tmp_pk);
      pv2.swap(pend_tmp_v);
    }
    SHD_HIP(hipStreamSynchronize(s));
    ppk.swap(ppk2);
    pv.swap(pv2);
    np = nn;
  }

  // ---- snapshot: window items, notify queue, aggregator states, dictionary
  void save_state(SnapW& w) override {
    w.put<int64_t>(C);
    w.put<int32_t>(ncols);
    w.put<int32_t>(nagg);
    w.put<int64_t>(np);
    w.put<int64_t>(last_global);
    w.put<int64_t>(nstates);
    if (C > 0)
      items.each([&](int c, int sub) {
        if (kItemCol[c].saved) w.dev(items.at(items.cur, c, sub), C * kItemCol[c].size);
      });
    if (np > 0) {
      w.dev(ppk.p, np * 8);
      w.dev(pv.p, np * 8);
    }
    if (nagg > 0 && nstates > 0) {
      w.dev(g_dsum.p, (size_t)nagg * nstates * 8);
      w.dev(g_lsum.p, (size_t)nagg * nstates * 8);
      w.dev(g_cnt.p, (size_t)nagg * nstates * 8);
    }
    gd.save(w);
    // batch windows: RESET epochs, timeBatch's nextEmitTime and notify queue
    w.put<int64_t>(tb_next);
    w.put<int64_t>(tb_epoch);
    w.put<int64_t>((int64_t)tb_notify.size());
    for (int64_t t : tb_notify) w.put<int64_t>(t);
    if (batch && nagg > 0 && nstates > 0) w.dev(g_epoch.p, (size_t)nstates * 8);
    // min / max deques (the values and flags travel in the state tables above)
    if (ndq > 0) {
      w.put<int32_t>(ndq);
      w.put<int64_t>(dq_total);
      if (nstates > 0) {
        w.dev(dq_len.p, (size_t)ndq * nstates * 4);
        w.dev(dq_off.p, (size_t)ndq * nstates * 4);
      }
      if (dq_total > 0) w.dev(dq_val[dq_cur].p, (size_t)dq_total * 8);
    }
  }
  void load_state(SnapR& r) override {
    const int64_t c0 = r.get<int64_t>();
    if (r.get<int32_t>() != ncols || r.get<int32_t>() != nagg || c0 < 0)
      throw Error(SHD_E_ARG, "snapshot of a different plan");
    const int64_t np0 = r.get<int64_t>();
    last_global = r.get<int64_t>();
    const int64_t ns = r.get<int64_t>();
    items.cur = 0;
    if (c0 > 0) {
      if (items.cap[0] < c0) items.alloc(0, std::max<int64_t>(c0, 1024));
      items.each([&](int c, int sub) {   // what is not saved means "carried": all ones
        if (kItemCol[c].saved) r.dev_into(items.at(0, c, sub), c0 * kItemCol[c].size);
        else SHD_HIP(hipMemsetAsync(items.at(0, c, sub), 0xFF, c0 * kItemCol[c].size, stream));
      });
    }
    C = c0;
    np = np0;
    if (np > 0) {
      ppk.reserve(np * 8);
      pv.reserve(np * 8);
      r.dev_into(ppk.p, np * 8);
      r.dev_into(pv.p, np * 8);
    }
    nstates = 0;
    if (nagg > 0 && ns > 0) {
      grow_states(ns);   // tables of exactly the saved size
      r.dev_into(g_dsum.p, (size_t)nagg * ns * 8);
      r.dev_into(g_lsum.p, (size_t)nagg * ns * 8);
      r.dev_into(g_cnt.p, (size_t)nagg * ns * 8);
    } else {
      nstates = ns;
    }
    gd.nk = std::max(nw, 1);
    gd.load(r, stream);
    tb_next = r.get<int64_t>();
    tb_epoch = r.get<int64_t>();
    tb_notify.clear();
    const int64_t nn = r.get<int64_t>();
    for (int64_t i = 0; i < nn; i++) tb_notify.push_back(r.get<int64_t>());
    if (batch && nagg > 0 && nstates > 0) r.dev_into(g_epoch.p, (size_t)nstates * 8);
    if (ndq > 0) {
      if (r.get<int32_t>() != ndq) throw Error(SHD_E_ARG, "snapshot of a different plan");
      dq_total = r.get<int64_t>();
      if (dq_total < 0 || dq_total >= (int64_t)INT32_MAX) throw Error(SHD_E_ARG, "snapshot of a different plan");
      if (nstates > 0) {
        r.dev_into(dq_len.p, (size_t)ndq * nstates * 4);
        r.dev_into(dq_off.p, (size_t)ndq * nstates * 4);
      }
      if (dq_total > 0) {
        dq_val[dq_cur].reserve((size_t)dq_total * 8);
        r.dev_into(dq_val[dq_cur].p, (size_t)dq_total * 8);
      }
    }
    counters.carry = C;
  }
};

std::unique_ptr<Engine> make_window_x_engine(const Plan& p, std::string& why) {
  if (p.kind != SHD_KIND_SINGLE) { why = "not a single-stream query"; return nullptr; }
  auto e = std::make_unique<WindowXEngine>();
  const auto& types = p.stream_types[p.single_stream];
  if (types.size() > (size_t)kMaxCols) { why = "too many attributes"; return nullptr; }
  e->ncols = (int)types.size();
  bool seen_window = false;
  for (auto& h : p.handlers) {
    if (h.kind == SHD_H_FILTER) {
      if (seen_window) { why = "filter after window"; return nullptr; }
      e->filters.push_back(h.expr);
    } else {
      seen_window = true;
      e->wkind = h.wkind;
      e->wparam = h.param;
      e->wparam2 = h.param2;
    }
  }
  if (e->filters.size() > 4) { why = "too many filters"; return nullptr; }
  if (e->wkind == SHD_W_LENGTH && e->wparam <= 0) { why = "length(0) window"; return nullptr; }
  e->batch = e->wkind == SHD_W_LENGTH_BATCH || e->wkind == SHD_W_TIME_BATCH ||
             e->wkind == SHD_W_TIME_BATCH_STREAM || e->wkind == SHD_W_EXTERNAL_TIME_BATCH;
  if (e->wkind == SHD_W_LENGTH_BATCH)
    e->bmode = e->wparam == 0 ? XB_ZERO_LEN : ((e->wparam2 & 1) ? XB_STREAM_LEN : XB_FULL_LEN);
  else if (e->wkind == SHD_W_TIME_BATCH)
    e->bmode = XB_FULL_TIME;
  else if (e->wkind == SHD_W_TIME_BATCH_STREAM)
    e->bmode = XB_STREAM_TIME;
  if (e->wkind == SHD_W_EXTERNAL_TIME_BATCH) {
    e->bmode = XB_FULL_EXT;
    const int64_t q = e->wparam2;
    e->etb_ts_col = SHD_ETB_TS_COL(q);
    e->etb_start_mode = SHD_ETB_START_MODE(q);
    e->etb_replace = SHD_ETB_REPLACE(q);
    const int ref = SHD_ETB_START_REF(q);
    auto long_col = [&](int c) { return c >= 0 && c < e->ncols && types[c] == SHD_T_LONG; };
    if (q < 0 || !long_col(e->etb_ts_col)) { why = "externalTimeBatch timestamp attribute"; return nullptr; }
    if (e->etb_start_mode == SHD_ETB_START_CONST) {
      if (ref >= (int)p.consts.size()) { why = "externalTimeBatch startTime constant"; return nullptr; }
      e->etb_start_const = (int64_t)p.consts[ref];
    } else if (e->etb_start_mode == SHD_ETB_START_ATTR) {
      if (!long_col(ref)) { why = "externalTimeBatch startTime attribute"; return nullptr; }
      e->etb_start_col = ref;
    } else if (e->etb_start_mode != SHD_ETB_START_NONE) {
      why = "externalTimeBatch startTime mode";
      return nullptr;
    }
  }
  if (e->wkind == SHD_W_EXTERNAL_TIME && (e->wparam2 < 0 || e->wparam2 >= e->ncols)) {
    why = "externalTime attribute";
    return nullptr;
  }
  if (e->wkind == SHD_W_TIME_LENGTH && (e->wparam2 <= 0 || e->wparam < 0)) {
    why = "timeLength window of length 0";
    return nullptr;
  }
  if (e->batch && e->wparam <= 0 && e->bmode != XB_ZERO_LEN) { why = "batch window of time 0"; return nullptr; }
  if (e->wkind == SHD_W_TIME && e->wparam < 0) { why = "negative time window"; return nullptr; }
  if (p.outputs.size() > (size_t)kMaxCols) { why = "too many outputs"; return nullptr; }
  e->nagg = (int)p.aggs.size();
  if (e->nagg > kMaxAggs) { why = "too many aggregators"; return nullptr; }
  // min / max track future states when the window slides or the query emits
  // EXPIRED events (MaxAttributeAggregatorExecutor.java:93-96; SLIDE is
  // SlidingWindowProcessor.java:90, every other window here is BATCH or RESET)
  e->track = e->wkind == SHD_W_LENGTH || e->wkind == SHD_W_TIME || e->wkind == SHD_W_TIME_LENGTH ||
             e->wkind == SHD_W_EXTERNAL_TIME || p.expired_on;
  for (int g = 0; g < e->nagg; g++) {
    const auto& a = p.aggs[g];
    e->dq_of[g] = -1;
    if (a.kind < SHD_AGG_SUM || a.kind > SHD_AGG_OR) { why = "unknown aggregator"; return nullptr; }
    if (a.kind < SHD_AGG_MAX) continue;
    if (a.kind >= SHD_AGG_STDDEV) {
      // stdDev of a number, and / or of a BOOL, distinctCount of anything a slot holds
      const bool num = a.type >= SHD_T_INT && a.type <= SHD_T_DOUBLE;
      const bool ok = a.kind == SHD_AGG_STDDEV ? num
                      : a.kind == SHD_AGG_DISTINCT_COUNT ? (num || a.type == SHD_T_STRING || a.type == SHD_T_BOOL)
                                                         : a.type == SHD_T_BOOL;
      if (a.expr < 0 || !ok) { why = "stdDev / distinctCount / and / or of an argument of this type"; return nullptr; }
      e->xa = true;
      if (a.kind == SHD_AGG_DISTINCT_COUNT) {
        e->dq_esz[e->ndq] = 2;
        e->dq_words += 2;
        e->dq_of[g] = e->ndq++;
      }
      continue;
    }
    if (a.expr < 0 || a.type < SHD_T_INT || a.type > SHD_T_DOUBLE) { why = "min / max of a non-numeric argument"; return nullptr; }
    e->mm = true;
    if (e->track && (a.kind == SHD_AGG_MAX || a.kind == SHD_AGG_MIN)) {
      e->dq_esz[e->ndq] = 1;
      e->dq_words += 1;
      e->dq_of[g] = e->ndq++;
    }
  }
  e->partitioned = !p.part_keys.empty();
  if (e->partitioned) {
    e->key_expr = p.part_keys[0].second;
    const auto& code = p.exprs[e->key_expr];
    e->key_col = (code.size() == 1 && code[0].op == SHD_OP_LOAD) ? (code[0].c & 0xFFFF) : -1;
    e->key_type = expr_result_type(p, e->key_expr, {});
  }
  if (p.group_by.size() > (size_t)kMaxGroupAttrs) { why = "more than 4 group-by attributes"; return nullptr; }
  e->ngk = (int)p.group_by.size();
  for (int g = 0; g < e->ngk; g++) {
    e->gk_expr[g] = p.group_by[g];
    const auto& code = p.exprs[e->gk_expr[g]];
    e->gk_col[g] = (code.size() == 1 && code[0].op == SHD_OP_LOAD) ? (code[0].c & 0xFFFF) : -1;
    e->gk_type[g] = expr_result_type(p, e->gk_expr[g], {});
  }
  e->group = e->ngk > 0;
  if (e->wkind == SHD_W_EXTERNAL_TIME_BATCH && e->etb_replace) {
    // aggregator arguments and group keys are taken from the arriving event;
    // the reference reads them from the clone whose timestamp was replaced
    auto reads_ts = [&](int x) {
      if (x < 0) return false;
      for (auto& in : p.exprs[x])
        if (in.op == SHD_OP_LOAD && (in.c & 0xFFFF) == e->etb_ts_col) return true;
      return false;
    };
    bool bad = false;
    for (auto& a : p.aggs) bad = bad || reads_ts(a.expr);
    for (int g : p.group_by) bad = bad || reads_ts(g);
    if (bad) { why = "externalTimeBatch: aggregating or grouping by the replaced timestamp"; return nullptr; }
  }
  e->plain = e->ngk == 0 && e->nagg == 0;
  // state key words: (partition key, group words); none for one global state
  e->nw = e->plain ? 0 : (e->partitioned ? 1 : 0) + e->ngk;
  e->gd.nk = std::max(e->nw, 1);
  e->items.nsub[SUB_ATTR] = e->ncols;
  e->items.nsub[SUB_AGG] = e->nagg;
  return e;
}

}  // namespace shd
