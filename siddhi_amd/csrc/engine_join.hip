// engine_join.hip -- stream-stream window joins (`from A#window... join B#window... on ...`).
//
// Reference semantics (modules/siddhi-core/src/main/java/io/siddhi/core/):
//   query/input/stream/join/JoinProcessor.java:79-190 (trigger, find, outer rows, TIMER skipped)
//   util/parser/JoinInputStreamParser.java:200-225,334-352,393-452 (sides, trigger / outer flags)
//   query/processor/stream/window/LengthWindowProcessor.java:105-158 (chunk order, find on the queue)
//   query/processor/stream/window/EmptyWindowProcessor.java:66-120 (a side without a window)
//   query/processor/stream/window/ExternalTimeWindowProcessor.java:125-161,174-186 (event-time side)
//   util/parser/OperatorParser.java (constructOperator over an event queue: matches oldest first)
//   query/selector/QuerySelector.java process(List<ComplexEventChunk>) (type filter, one output chunk)
//
// Formulation: each side keeps its filtered events in arrival order (an
// ItemStore, window_items.h).  The content of a side's window at any moment is
// a contiguous range of that sequence, so a trigger event of side X meets the
// items [lo, hi) of side Y, where the range depends only on the trigger's call.
// One push of X appends X's items, enumerates its trigger slots in chunk order
// (closed form for `length` and windowless sides; an externalTime side, whose
// events expire a variable number of items, builds a trigger list first: see
// "externalTime sides" below), counts each slot's matches (k_join_count), scans
// the counts into row offsets and writes the rows (k_join_emit, the same walk).  Both kernels are a nested-loop band join: a
// workgroup owns kJoinTrig consecutive slots, one per thread, and walks the
// union of their Y ranges in tiles of kJoinTile items staged in LDS; every
// lane reads the same staged item at the same time (LDS broadcast reads).
#include <algorithm>
#include <cstring>

#include "engine.h"
#include "stream_kernels.h"
#include "window_items.h"

namespace shd {

namespace {

// Trigger slots per workgroup (one per thread) and Y items per LDS tile.
// The choice is reasoned, not measured: see DESIGN.md "Joins".
constexpr int kJoinTrig = 256;
constexpr int kJoinTile = 64;
static_assert(kJoinTrig == kBlock, "one trigger slot per thread of a kBlock workgroup");

struct JoinArgs {
  DExprSet es;
  DExpr on;
  int32_t has_on;
  FPred fp;            // the `on` condition as a fast predicate (fp.ok), else the interpreter
  int32_t pre;         // bit 2i / 2i+1: left / right term of comparison i reads no Y attribute
  DExpr outs[kMaxCols];
  int32_t nout;
  // X: the side whose events trigger (slot = one CURRENT or EXPIRED event of its chunk)
  const uint64_t* xattr;   // [xncols][xcap]
  const uint8_t* xnul;
  const int64_t* xts;
  const int64_t* xseq;
  const int32_t* xcall;
  int64_t xcap;
  int32_t xncols;
  int32_t xside;       // 0: X is the left side
  int32_t per;         // slots per new item: the wanted event types (1 or 2)
  int32_t want_cur;
  int32_t self_exp;    // no window: an item's EXPIRED event follows its own CURRENT one
  int32_t outer;       // a slot without a match emits one row with Y null
  int64_t C, L, nslots;
  int32_t ext;               // X is an externalTime side: the slots are the records of its trigger list
  const int32_t* trig_item;  // [nslots] the X item the slot's event carries
  const int32_t* trig_by;    // [nslots] the new item whose arrival made the event (itself: CURRENT)
  const int64_t* xtau;       // X's time attribute, per item (stamp of its EXPIRED events)
  const int64_t* call_now;   // [ncalls] the clock of each call (stamp of EXPIRED events)
  // Y: the side that is looked up
  const uint64_t* yattr;   // [yncols][ycap]
  const uint8_t* ynul;
  int64_t ycap;
  int32_t yncols;
  const int64_t* ylo;  // [ncalls] first item of Y's window for the triggers of a call
  int64_t yhi;         // one past its last item
  // output
  int64_t row0, chunk0;
};

// One trigger slot: slot u of the push belongs to new item u / per.
struct Trig {
  bool valid;
  int type;        // SHD_EV_CURRENT / SHD_EV_EXPIRED
  int64_t item;    // X item the event carries
  int32_t call;
  int64_t ts, seq;
};

__device__ __forceinline__ Trig join_slot(const JoinArgs& a, int64_t u) {
  Trig t;
  if (a.ext) {
    const int64_t fresh = a.C + gld(a.trig_by, u);
    t.item = gld(a.trig_item, u);
    t.call = gld(a.xcall, fresh);
    t.seq = gld(a.xseq, fresh);
    t.valid = true;
    t.type = t.item == fresh ? SHD_EV_CURRENT : SHD_EV_EXPIRED;
    t.ts = t.type == SHD_EV_CURRENT ? gld(a.xts, fresh) : gld(a.xtau, fresh);
    return t;
  }
  const int64_t j = u / a.per;
  const int k = (int)(u - j * a.per);
  const int64_t fresh = a.C + j;
  t.call = gld(a.xcall, fresh);
  t.seq = gld(a.xseq, fresh);
  t.valid = true;
  if (a.self_exp) {   // CURRENT, then its own EXPIRED (EmptyWindowProcessor)
    t.type = a.per == 2 ? k : (a.want_cur ? SHD_EV_CURRENT : SHD_EV_EXPIRED);
    t.item = fresh;
  } else {            // the item the new one pushes out, then the new one (LengthWindowProcessor)
    t.type = a.per == 2 ? 1 - k : (a.want_cur ? SHD_EV_CURRENT : SHD_EV_EXPIRED);
    t.item = t.type == SHD_EV_EXPIRED ? fresh - a.L : fresh;
    t.valid = t.item >= 0;
  }
  const int64_t it = t.valid ? t.item : fresh;
  t.ts = t.type == SHD_EV_CURRENT ? gld(a.xts, it) : gld(a.call_now, (int64_t)t.call);
  return t;
}

// A (trigger, found item) pair: the trigger's attributes come from X's item
// columns, the found item's from the staged tile.  missing: the outer row.
struct JoinCtx {
  const JoinArgs* a;
  int64_t xitem;
  const uint64_t* tv;   // LDS tile [yncols][kJoinTile]
  const uint8_t* tn;
  int k;
  bool missing;
  int64_t tsv;
  __device__ __forceinline__ Val load(int st, int, int attr) const {
    if (st == a->xside) {
      if ((unsigned)attr >= (unsigned)a->xncols) return Val{0, 1};
      const int64_t o = (int64_t)attr * a->xcap + xitem;
      return Val{gld(a->xattr, o), (int)gld(a->xnul, o)};
    }
    if (missing || (unsigned)attr >= (unsigned)a->yncols) return Val{0, 1};
    return Val{tv[attr * kJoinTile + k], (int)tn[attr * kJoinTile + k]};
  }
  __device__ __forceinline__ bool evnull(int st, int) const { return st != a->xside && missing; }
  __device__ __forceinline__ int64_t ts(int, int) const { return tsv; }
  __device__ __forceinline__ Val agg(int) const { return Val{0, 1}; }
};

// The terms of the fast predicate that read only the trigger: evaluated once
// per slot and kept in registers for the whole walk.
struct PreTerms {
  Val l[4], r[4];
};

__device__ __forceinline__ void join_pre(const JoinArgs& a, const JoinCtx& cx, PreTerms& p) {
#pragma unroll
  for (int i = 0; i < 4; i++) {
    p.l[i] = Val{0, 1};
    p.r[i] = Val{0, 1};
    if (a.fp.ok && i < a.fp.n) {
      if ((a.pre >> (2 * i)) & 1) p.l[i] = fp_term(a.fp.c[i].l, cx);
      if ((a.pre >> (2 * i + 1)) & 1) p.r[i] = fp_term(a.fp.c[i].r, cx);
    }
  }
}

__device__ __forceinline__ bool join_on(const JoinArgs& a, const JoinCtx& cx, const PreTerms& p) {
  if (!a.has_on) return true;
  if (a.fp.ok) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      if (i < a.fp.n) {
        const FCmp& c = a.fp.c[i];
        const Val l = ((a.pre >> (2 * i)) & 1) ? p.l[i] : fp_term(c.l, cx);
        const Val r = ((a.pre >> (2 * i + 1)) & 1) ? p.r[i] : fp_term(c.r, cx);
        if (l.null || r.null || !d_compare(c.op, c.type, l.b, r.b)) return false;
      }
    }
    return true;
  }
  return eval_bool(a.es.ins + a.on.off, a.on.len, a.es.consts, cx);
}

// The walk both kernels share: stage Y's items [base, base + kJoinTile) and
// hand every (slot, item) pair of the slot's own range that satisfies `on` to
// f(k, ordinal).  Returns the slot's match count.
template <class F>
__device__ __forceinline__ uint32_t join_walk(const JoinArgs& a, const Trig& t, uint64_t* tv, uint8_t* tn,
                                              int64_t* blk_lo, F f) {
  const int tid = threadIdx.x;
  const int64_t my_lo = t.valid ? gld(a.ylo, (int64_t)t.call) : a.yhi;
  if (tid == 0) *blk_lo = a.yhi;
  __syncthreads();
  if (my_lo < a.yhi) atomicMin((unsigned long long*)blk_lo, (unsigned long long)my_lo);   // ranges are >= 0
  __syncthreads();
  const int64_t lo = *blk_lo;
  JoinCtx cx{&a, t.valid ? t.item : 0, tv, tn, 0, false, t.ts};
  PreTerms pt;
  join_pre(a, cx, pt);
  uint32_t cnt = 0;
  for (int64_t base = lo; base < a.yhi; base += kJoinTile) {
    const int len = (int)(a.yhi - base < kJoinTile ? a.yhi - base : kJoinTile);
    __syncthreads();   // the previous tile has been read
    for (int idx = tid; idx < a.yncols * kJoinTile; idx += kJoinTrig) {
      const int c = idx / kJoinTile, k = idx - c * kJoinTile;
      if (k < len) {
        const int64_t o = (int64_t)c * a.ycap + base + k;
        tv[idx] = gld(a.yattr, o);
        tn[idx] = gld(a.ynul, o);
      }
    }
    __syncthreads();
    if (t.valid) {
      for (int k = 0; k < len; k++) {
        if (base + k < my_lo) continue;
        cx.k = k;
        if (join_on(a, cx, pt)) {
          f(cx, cnt);
          cnt++;
        }
      }
    }
  }
  return cnt;
}

struct JoinTotals {
  uint32_t scan_total;   // scan_exclusive_u32 over the slots' row counts
  uint32_t pad;
  uint64_t rows;         // the same total in 64 bits (k_join_total): the capacity check
  int64_t lo_last;       // externalTime side: first item of its window after the push (k_jext_lo)
};
static_assert(offsetof(JoinTotals, scan_total) == 0 && offsetof(JoinTotals, rows) == 8 &&
                  offsetof(JoinTotals, lo_last) == 16 && sizeof(JoinTotals) <= 64,
              "JoinTotals device layout");

// ---------------------------------------------------------------- externalTime sides
// ExternalTimeWindowProcessor pops its queue's head while tau_head - tau_j + T
// <= 0 when item j arrives, and stops at the first head that is not due.  With
// M the running maximum of tau over the side's items (scan_inclusive_max_i64),
// the window after item j is [lo_j, j], lo_j the first i with M_i - M_j + T > 0
// (M never decreases: a binary search), and item j expires [lo_{j-1}, lo_j).
// The carried items are the window itself, so lo_{-1} = 0 and the maximum over
// carried + new items is the maximum over all history.  In chunk order the
// events before item j's group are lo_{j-1} EXPIRED and j CURRENT ones, which
// places every wanted event without a scan: expired item e lands at
// e + (CURRENT wanted ? j : 0) for its expirer j (the first j with lo_j > e),
// item j's CURRENT event at (EXPIRED wanted ? lo_j : 0) + j.
struct JoinExtArgs {
  const int64_t* M;      // [C + m] running maximum of the time attribute
  int64_t C, m, T;
  int64_t* lo;           // [m] first item of the window after new item j
  int64_t nexp;          // EXPIRED slots of the push (0 when the output does not want them)
  int32_t want_cur;
  int32_t* trig_item;    // [nexp + (want_cur ? m : 0)]
  int32_t* trig_by;
  JoinTotals* tot;
};

__global__ __launch_bounds__(kBlock) void k_jext_lo(const JoinExtArgs* __restrict__ ap) {
  const JoinExtArgs& a = *ap;
  for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < a.m; j = a.m) {
    const int64_t g = a.C + j;
    const int64_t mg = gld(a.M, g);
    int64_t l = 0, h = g;   // M_g - M_g + T > 0: the answer is in [0, g]
    while (l < h) {
      const int64_t mid = l + ((h - l) >> 1);
      if (gld(a.M, mid) - mg + a.T > 0) h = mid;
      else l = mid + 1;
    }
    a.lo[j] = l;
    if (j == a.m - 1) a.tot->lo_last = l;
  }
}

// One thread per wanted event of the push: the expired items [0, nexp), then
// the new items.
__global__ __launch_bounds__(kBlock) void k_jext_trig(const JoinExtArgs* __restrict__ ap) {
  const JoinExtArgs& a = *ap;
  const int64_t n = a.nexp + (a.want_cur ? a.m : 0);
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i = n) {
    int64_t slot, item, by;
    if (i < a.nexp) {   // its expirer: the first new item j with lo_j > i (lo_{m-1} >= nexp > i)
      int64_t l = 0, h = a.m - 1;
      while (l < h) {
        const int64_t mid = l + ((h - l) >> 1);
        if (gld(a.lo, mid) > i) h = mid;
        else l = mid + 1;
      }
      by = l;
      item = i;
      slot = i + (a.want_cur ? by : 0);
    } else {
      by = i - a.nexp;
      item = a.C + by;
      slot = (a.nexp > 0 ? gld(a.lo, by) : 0) + by;
    }
    a.trig_item[slot] = (int32_t)item;
    a.trig_by[slot] = (int32_t)by;
  }
}

// cnt[u] = rows of slot u: its matches, or 1 for an outer slot without one;
// blk[b] = rows of workgroup b's slots (folded by k_join_total: no atomics on
// one address from every workgroup).
__global__ __launch_bounds__(kJoinTrig) void k_join_count(const JoinArgs* __restrict__ ap, uint32_t* cnt,
                                                          uint64_t* blk) {
  __shared__ uint64_t tv[kMaxCols * kJoinTile];
  __shared__ uint8_t tn[kMaxCols * kJoinTile];
  __shared__ int64_t blk_lo;
  __shared__ unsigned long long blk_rows;
  const JoinArgs& a = *ap;
  const int64_t u = (int64_t)blockIdx.x * kJoinTrig + threadIdx.x;
  const bool live = u < a.nslots;
  Trig t{};
  if (live) t = join_slot(a, u);
  t.valid = live && t.valid;
  if (threadIdx.x == 0) blk_rows = 0;
  uint32_t c = join_walk(a, t, tv, tn, &blk_lo, [](const JoinCtx&, uint32_t) {});
  if (t.valid && c == 0 && a.outer) c = 1;
  if (live) cnt[u] = c;
  if (c) atomicAdd(&blk_rows, (unsigned long long)c);
  __syncthreads();
  if (threadIdx.x == 0) blk[blockIdx.x] = blk_rows;
}

// tot->rows = the sum of the nb workgroup totals (one workgroup).
__global__ __launch_bounds__(kBlock) void k_join_total(const uint64_t* blk, int64_t nb, JoinTotals* tot) {
  __shared__ unsigned long long sum;
  if (threadIdx.x == 0) sum = 0;
  __syncthreads();
  unsigned long long v = 0;
  for (int64_t i = threadIdx.x; i < nb; i += kBlock) v += blk[i];
  if (v) atomicAdd(&sum, v);
  __syncthreads();
  if (threadIdx.x == 0) tot->rows = sum;
}

__global__ __launch_bounds__(kJoinTrig) void k_join_emit(const JoinArgs* __restrict__ ap, const uint32_t* off,
                                                         int64_t* o_chunk, int32_t* o_type, int64_t* o_ts,
                                                         uint64_t* o_vals, uint8_t* o_nul, int64_t* o_seq,
                                                         int32_t* o_sidx) {
  __shared__ uint64_t tv[kMaxCols * kJoinTile];
  __shared__ uint8_t tn[kMaxCols * kJoinTile];
  __shared__ int64_t blk_lo;
  const JoinArgs& a = *ap;
  const int64_t u = (int64_t)blockIdx.x * kJoinTrig + threadIdx.x;
  const bool live = u < a.nslots;
  Trig t{};
  if (live) t = join_slot(a, u);
  t.valid = live && t.valid;
  const int64_t first = a.row0 + (live ? (int64_t)off[u] : 0);
  auto write = [&](const JoinCtx& cx, uint32_t ord) {
    const int64_t row = first + ord;
    for (int c = 0; c < a.nout; c++) {
      const Val v = eval_expr(a.es.ins + a.outs[c].off, a.outs[c].len, a.es.consts, cx);
      o_vals[row * a.nout + c] = v.b;
      o_nul[row * a.nout + c] = (uint8_t)v.null;
    }
    o_ts[row] = t.ts;
    o_type[row] = t.type;
    o_chunk[row] = a.chunk0 + t.call;
    o_seq[row] = t.seq;
    o_sidx[row] = a.xside;
  };
  const uint32_t c = join_walk(a, t, tv, tn, &blk_lo, write);
  if (t.valid && c == 0 && a.outer) {
    JoinCtx cx{&a, t.item, tv, tn, 0, true, t.ts};
    write(cx, 0);
  }
}

// The items [from, from + kept) of one slot become [0, kept) of the other.
struct JoinCarryArgs {
  ItemPtrs src, dst;
  int64_t from, kept, cap_src, cap_dst;
  int32_t ncols;
};

__global__ __launch_bounds__(kBlock) void k_join_carry(const JoinCarryArgs* __restrict__ ap) {
  const JoinCarryArgs& a = *ap;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < a.kept; i = a.kept) {
    const int64_t s = a.from + i;
    a.dst.ts[i] = a.src.ts[s];
    a.dst.seq[i] = a.src.seq[s];
    a.dst.call[i] = -1;
    a.dst.row[i] = -1;
    for (int c = 0; c < a.ncols; c++) {
      a.dst.attr[(int64_t)c * a.cap_dst + i] = a.src.attr[(int64_t)c * a.cap_src + s];
      a.dst.nul[(int64_t)c * a.cap_dst + i] = a.src.nul[(int64_t)c * a.cap_src + s];
    }
  }
}

}  // namespace

// ====================================================================== host
struct JoinEngine : Engine {
  struct Side {
    int stream = 0, wkind = 0, ncols = 0;
    bool trigger = true, outer = false;
    int64_t L = 0;   // length: L; externalTime: T
    int tcol = -1;   // externalTime: the attribute holding the event time
    bool ext() const { return wkind == SHD_W_EXTERNAL_TIME; }
    std::vector<int> filters;
    ItemStore items;
    int64_t C = 0;   // items held: [0, C) of slot items.cur, in arrival order
  };
  Side side[2];
  int on_expr = -1;

  DevBuf d_offs, d_call_of, d_last, d_call_now, d_ylo;
  DevBuf d_flags, d_cnt, d_off, d_pkey, d_rows, d_roff, d_blk, d_scan;
  DevBuf d_M, d_lo, d_trig_item, d_trig_by;   // externalTime sides
  PinnedBuf h_pin;
  ReadbackBlock<JoinTotals> tot;

  int kind() const override { return ENG_JOIN; }

  void reset() override {
    for (Side& s : side) s.C = 0;
    seq = 0;
    now = INT64_MIN;
    chunk_seq = 0;
    out.count = 0;
    counters = shd_counters{};
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

  // slot items.cur of a side with room for `need` items, its [0, C) preserved
  void ensure_items(Side& s, int64_t need) {
    ItemStore& it = s.items;
    const int from = it.cur, to = from ^ 1;
    if (it.cap[from] >= need) return;
    it.alloc(to, std::max<int64_t>(need, std::max<int64_t>(1024, it.cap[from] * 2)));
    if (s.C > 0)
      it.each([&](int c, int sub) {
        SHD_HIP(hipMemcpyAsync(it.at(to, c, sub), it.at(from, c, sub), s.C * kItemCol[c].size,
                               hipMemcpyDeviceToDevice, stream));
      });
    it.cur = to;
  }

  void push(const Staged& b) override {
    const int xs = b.stream == side[0].stream ? 0 : 1;
    Side& X = side[xs];
    Side& Y = side[xs ^ 1];
    if (b.stream != X.stream) throw Error(SHD_E_ARG, "stream is not a side of this join");
    const int64_t n = b.n;
    SHD_HIP(hipEventRecord(ev0, stream));
    stage_begin();

    // calls and their clocks (setCurrentTimestamp before each call's events)
    std::vector<int64_t> offs = b.call_offsets;
    if (offs.size() < 2) offs = {0, n};
    const int ncalls = (int)offs.size() - 1;
    upload(d_offs, offs);
    d_call_of.reserve(std::max<int64_t>(n, 1) * 4);
    d_last.reserve((size_t)ncalls * 8);
    launch_grid(k_call_of, (unsigned)ncalls, d_offs.as<int64_t>(), ncalls, b.cs.ts, d_call_of.as<int32_t>(),
                d_last.as<int64_t>());
    std::vector<int64_t> call_now(ncalls, now);
    int64_t clk = now;
    if (b.advance_time) {
      h_pin.reserve((size_t)ncalls * 8);
      SHD_HIP(hipMemcpyAsync(h_pin.p, d_last.p, (size_t)ncalls * 8, hipMemcpyDeviceToHost, stream));
      SHD_HIP(hipStreamSynchronize(stream));
      const int64_t* last = h_pin.as<int64_t>();
      for (int c = 0; c < ncalls; c++) {
        if (offs[c + 1] > offs[c] && last[c] >= clk) clk = last[c];
        call_now[c] = clk;
      }
    }

    // X's new items [C, C + m)
    d_flags.reserve(n);
    d_cnt.reserve(n * 4);
    d_off.reserve(n * 4);
    d_pkey.reserve(n * 8);
    XwArgs xa{};
    xa.cs = b.cs;
    xa.es = dset();
    xa.filters = dfilters(X.filters);
    xa.ncols = X.ncols;
    xa.C = X.C;
    xa.seq0 = seq;
    xa.notnull1 = X.ext() ? X.tcol + 1 : 0;   // a null event time: the event does not enter the join
    tot.reserve();
    launch(k_xw_filter, n, dev_args(xa), n, d_flags.as<uint8_t>(), d_cnt.as<uint32_t>(), d_pkey.as<uint64_t>());
    const int64_t m = scan(d_cnt.as<uint32_t>(), d_off.as<uint32_t>(), n, &tot.dev()->scan_total,
                           &tot.host().scan_total, d_scan);
    const int64_t total = X.C + m;
    if (total >= (int64_t)INT32_MAX) throw Error(SHD_E_CAPACITY, "window items exceed 2^31");
    ensure_items(X, std::max<int64_t>(total, 1));
    xa.cap = X.items.cap[X.items.cur];
    const ItemPtrs xp = X.items.ptrs(X.items.cur);
    if (m > 0) {
      const ItemOut io{xp, nullptr, nullptr, nullptr};
      launch(k_xw_items, n, dev_args(xa), dev_args(io), n, d_cnt.as<uint32_t>(), d_off.as<uint32_t>(),
             d_pkey.as<uint64_t>(), d_call_of.as<int32_t>(), m);
    }
    mark("items");

    // externalTime: the running maximum of X's time attribute, the window's
    // first item after each new item, and the item the push's window starts at
    int64_t lo_last = 0;
    JoinExtArgs ea{};
    if (X.ext() && m > 0) {
      d_M.reserve((size_t)total * 8);
      d_lo.reserve((size_t)m * 8);
      const int64_t* tau = reinterpret_cast<const int64_t*>(xp.attr) + (int64_t)X.tcol * xa.cap;
      scan_inclusive_max_i64(tau, d_M.as<int64_t>(), total, d_scan, stream);
      ea.M = d_M.as<int64_t>();
      ea.C = X.C;
      ea.m = m;
      ea.T = X.L;
      ea.lo = d_lo.as<int64_t>();
      ea.tot = tot.dev();
      launch(k_jext_lo, m, dev_args(ea));
      tot.fetch(&JoinTotals::lo_last, stream);
      SHD_HIP(hipStreamSynchronize(stream));
      lo_last = tot.host().lo_last;
      mark("window");
    }

    // trigger slots, their matches and rows
    const int per = (plan.current_on ? 1 : 0) + (plan.expired_on ? 1 : 0);
    int64_t nrows = 0, nslots = 0;
    if (X.trigger && m > 0)
      nslots = X.ext() ? (plan.expired_on ? lo_last : 0) + (plan.current_on ? m : 0) : m * per;
    if (nslots > 0) {
      if (nslots >= (int64_t)INT32_MAX) throw Error(SHD_E_CAPACITY, "join triggers exceed 2^31");
      if (X.ext()) {   // the trigger list, in chunk order
        d_trig_item.reserve((size_t)nslots * 4);
        d_trig_by.reserve((size_t)nslots * 4);
        ea.nexp = plan.expired_on ? lo_last : 0;
        ea.want_cur = plan.current_on;
        ea.trig_item = d_trig_item.as<int32_t>();
        ea.trig_by = d_trig_by.as<int32_t>();
        launch(k_jext_trig, nslots, dev_args(ea));
      }
      // Y's window at each call: the items it holds (length and windowless
      // sides keep exactly their window between pushes)
      upload(d_call_now, call_now);
      upload(d_ylo, std::vector<int64_t>(ncalls, 0));
      JoinArgs ja{};
      ja.es = dset();
      ja.has_on = on_expr >= 0;
      if (ja.has_on) {
        ja.on = dexpr(on_expr);
        ja.fp = dfilters({on_expr}).fp;
        for (int i = 0; ja.fp.ok && i < ja.fp.n; i++) {
          auto free_of_y = [&](const FTerm& t) {
            const bool a = t.a.kind != FA_LOAD || t.a.st == xs;
            const bool bb = t.aop == 0 || t.b.kind != FA_LOAD || t.b.st == xs;
            return a && bb;
          };
          if (free_of_y(ja.fp.c[i].l)) ja.pre |= 1 << (2 * i);
          if (free_of_y(ja.fp.c[i].r)) ja.pre |= 1 << (2 * i + 1);
        }
      }
      ja.nout = (int)plan.outputs.size();
      for (int c = 0; c < ja.nout; c++) ja.outs[c] = dexpr(plan.outputs[c].second);
      ja.xattr = xp.attr;
      ja.xnul = xp.nul;
      ja.xts = xp.ts;
      ja.xseq = xp.seq;
      ja.xcall = xp.call;
      ja.xcap = xa.cap;
      ja.xncols = X.ncols;
      ja.xside = xs;
      ja.per = per;
      ja.want_cur = plan.current_on;
      ja.self_exp = X.wkind == 0;
      ja.outer = X.outer;
      ja.C = X.C;
      ja.L = X.L;
      ja.nslots = nslots;
      ja.ext = X.ext();
      if (ja.ext) {
        ja.trig_item = d_trig_item.as<int32_t>();
        ja.trig_by = d_trig_by.as<int32_t>();
        ja.xtau = reinterpret_cast<const int64_t*>(xp.attr) + (int64_t)X.tcol * xa.cap;
      }
      ja.call_now = d_call_now.as<int64_t>();
      const ItemPtrs yp = Y.items.ptrs(Y.items.cur);
      ja.yattr = yp.attr;
      ja.ynul = yp.nul;
      ja.ycap = Y.items.cap[Y.items.cur];
      ja.yncols = Y.ncols;
      ja.ylo = d_ylo.as<int64_t>();
      ja.yhi = Y.C;
      ja.row0 = out.count;
      ja.chunk0 = chunk_seq;
      d_rows.reserve(nslots * 4);
      d_roff.reserve(nslots * 4);
      const JoinArgs* d_ja = dev_args(ja);
      const unsigned grid = (unsigned)ceil_div(nslots, kJoinTrig);
      d_blk.reserve((size_t)grid * 8);
      launch_grid(k_join_count, grid, d_ja, d_rows.as<uint32_t>(), d_blk.as<uint64_t>());
      launch_grid(k_join_total, 1, d_blk.as<uint64_t>(), (int64_t)grid, tot.dev());
      mark("join_count");
      tot.fetch(&JoinTotals::rows, stream);
      SHD_HIP(hipStreamSynchronize(stream));
      if (tot.host().rows > (uint64_t)INT32_MAX) throw Error(SHD_E_CAPACITY, "a join push of more than 2^31 - 1 rows");
      nrows = (int64_t)tot.host().rows;
      if (nrows > 0) {
        scan_exclusive_u32(d_rows.as<uint32_t>(), d_roff.as<uint32_t>(), nslots, &tot.dev()->scan_total, d_scan,
                           stream);
        out.ensure(nrows, stream);
        launch_grid(k_join_emit, grid, d_ja, d_roff.as<uint32_t>(), out.d_chunk(), out.d_type(), out.d_ts(),
                    out.d_vals(), out.d_nulls(), out.d_seq(), out.d_sidx());
        out.count += nrows;
      }
      mark("join_emit");
    }

    // carry: X keeps its window (length: the last L items; externalTime: the
    // items from lo_last on, however many; no window: nothing)
    const int64_t kept = X.ext() ? total - lo_last : X.wkind == SHD_W_LENGTH ? std::min<int64_t>(X.L, total) : 0;
    const int64_t from = total - kept;
    if (kept > 0 && from > 0) {
      ItemStore& it = X.items;
      const int oth = it.cur ^ 1;
      if (it.cap[oth] < kept) it.alloc(oth, std::max<int64_t>(kept * 2, 1024));
      JoinCarryArgs ca{xp, it.ptrs(oth), from, kept, xa.cap, it.cap[oth], X.ncols};
      launch(k_join_carry, kept, dev_args(ca));
      it.cur = oth;
    }
    X.C = kept;
    mark("carry");

    SHD_HIP(hipEventRecord(ev1, stream));
    stage_end();
    SHD_HIP(hipEventSynchronize(ev1));
    float ms = 0.f;
    SHD_HIP(hipEventElapsedTime(&ms, ev0, ev1));
    counters.kernel_ns = (int64_t)(ms * 1e6);
    counters.kernel_ns_total += counters.kernel_ns;
    counters.events += n;
    counters.matches += nrows;
    counters.carry = side[0].C + side[1].C;
    counters.partial_scans += nslots;
    chunk_seq += ncalls;
    now = clk;
    seq += n;
  }

  // ---- snapshot: both sides' items (timestamps, arrival indices, attributes)
  static constexpr int kSaved[4] = {I_TS, I_SEQ, I_ATTR, I_NUL};
  void save_state(SnapW& w) override {
    for (Side& s : side) {
      w.put<int64_t>(s.C);
      w.put<int32_t>(s.ncols);
      if (s.C <= 0) continue;
      for (int c : kSaved)
        for (int sub = 0; sub < s.items.nsub[kItemCol[c].sub]; sub++)
          w.dev(s.items.at(s.items.cur, c, sub), s.C * kItemCol[c].size);
    }
  }
  void load_state(SnapR& r) override {
    for (Side& s : side) {
      const int64_t c0 = r.get<int64_t>();
      // an externalTime window holds any number of items
      const int64_t most = s.ext() ? (int64_t)INT32_MAX - 1 : s.wkind == SHD_W_LENGTH ? s.L : 0;
      if (r.get<int32_t>() != s.ncols || c0 < 0 || c0 > most)
        throw Error(SHD_E_ARG, "snapshot of a different plan");
      s.items.cur = 0;
      if (c0 > 0) {
        if (s.items.cap[0] < c0) s.items.alloc(0, std::max<int64_t>(c0, 1024));
        for (int c : kSaved)
          for (int sub = 0; sub < s.items.nsub[kItemCol[c].sub]; sub++)
            r.dev_into(s.items.at(0, c, sub), c0 * kItemCol[c].size);
      }
      s.C = c0;
    }
    counters.carry = side[0].C + side[1].C;
  }
};

std::unique_ptr<Engine> make_join_engine(const Plan& p, std::string& why) {
  if (p.kind != SHD_KIND_JOIN) { why = "not a join query"; return nullptr; }
  auto e = std::make_unique<JoinEngine>();
  if (p.jside[0].stream == p.jside[1].stream) { why = "self-join"; return nullptr; }
  if (!p.aggs.empty() || !p.group_by.empty() || p.having >= 0) { why = "aggregating selector over a join"; return nullptr; }
  if (!p.part_keys.empty()) { why = "join inside a partition"; return nullptr; }
  if (p.outputs.size() > (size_t)kMaxCols) { why = "too many outputs"; return nullptr; }
  for (int sd = 0; sd < 2; sd++) {
    const Plan::JoinSide& j = p.jside[sd];
    JoinEngine::Side& s = e->side[sd];
    const auto& types = p.stream_types[j.stream];
    if (types.size() > (size_t)kMaxCols) { why = "too many attributes"; return nullptr; }
    if (j.filters.size() > 4) { why = "too many filters"; return nullptr; }
    if (j.wkind != 0 && j.wkind != SHD_W_LENGTH && j.wkind != SHD_W_EXTERNAL_TIME) {
      why = "join side window other than length or externalTime";
      return nullptr;
    }
    // externalTime: shd_api.cpp has split the packed word into T (param) and the time attribute (ts_col)
    if (j.wkind == SHD_W_EXTERNAL_TIME &&
        (j.param <= 0 || j.param >= (int64_t(1) << 48) || j.ts_col < 0 || j.ts_col >= (int)types.size() ||
         types[j.ts_col] != SHD_T_LONG)) {
      why = "externalTime join side: window time outside (0, 2^48) or no LONG time attribute";
      return nullptr;
    }
    if (j.wkind == SHD_W_LENGTH && (j.param <= 0 || j.param >= (int64_t)INT32_MAX)) {
      why = "length window of 0 or beyond 2^31 on a join side";
      return nullptr;
    }
    s.stream = j.stream;
    s.wkind = j.wkind;
    s.L = j.param;
    s.tcol = j.ts_col;
    s.trigger = j.trigger != 0;
    s.outer = j.outer != 0;
    s.filters = j.filters;
    s.ncols = (int)types.size();
    s.items.nsub[SUB_ATTR] = s.ncols;
  }
  e->on_expr = p.join_on;
  return e;
}

}  // namespace shd
