// window_items.h -- the window item store and the kernels that build items
// from a batch, shared by the engines that keep filtered events across pushes
// (engine_window.hip, engine_join.hip).  Like stream_kernels.h, everything
// sits in an unnamed namespace: each engine's code object carries its own
// copy under the name it has always had in profiles.
#pragma once
#include <algorithm>
#include <cstring>

#include "engine.h"
#include "gdict.h"
#include "agg.h"

namespace shd {

namespace {

// An event of the batch (filters, keys, aggregator arguments).
struct BatchCtx {
  const ColSet* cs;
  int64_t row;
  __device__ __forceinline__ Val load(int, int, int attr) const { return col_load(*cs, row, attr); }
  __device__ __forceinline__ bool evnull(int, int) const { return false; }
  __device__ __forceinline__ int64_t ts(int, int) const { return cs->ts[row]; }
  __device__ __forceinline__ Val agg(int) const { return Val{0, 1}; }
};

// ---------------------------------------------------------------- items
struct XwArgs {
  ColSet cs;
  DExprSet es;
  DFilters filters;
  int partitioned;
  DExpr key;
  int key_col, key_type;
  int ngk;                          // group-by attributes
  DExpr group[kMaxGroupAttrs];
  int group_col[kMaxGroupAttrs];
  int group_type[kMaxGroupAttrs];
  int64_t null_str_id;
  int nagg;
  DExpr agg_arg[kMaxAggs];
  int has_arg[kMaxAggs];
  int ncols;
  int nw;                           // state key words (partition key + group words), 0 = one state
  int64_t C, cap, seq0;
  int notnull1;                     // 1 + the attribute an item needs non-null (a join side's event time), 0 = none
};

// flags[i]: bit0 passes the filters, bit1 has a (non-null) partition key
__global__ __launch_bounds__(kBlock) void k_xw_filter(const XwArgs* __restrict__ ap, int64_t n, uint8_t* flags,
                                                      uint32_t* cnt, uint64_t* pkey) {
  const XwArgs& a = *ap;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i = n) {
    BatchCtx cx{&a.cs, i};
    uint8_t f = 0;
    uint64_t k = 0;
    bool keyed = true;
    if (a.partitioned) {
      Val kv = a.key_col >= 0 ? col_load(a.cs, i, a.key_col)
                              : eval_expr(a.es.ins + a.key.off, a.key.len, a.es.consts, cx);
      keyed = !kv.null;
      k = canon_key(kv, a.key_type);
    }
    if (keyed) {
      f |= 2;
      if (eval_filters(a.es, a.filters, cx) && !(a.notnull1 && col_load(a.cs, i, a.notnull1 - 1).null)) f |= 1;
    }
    flags[i] = f;
    pkey[i] = k;
    cnt[i] = f == 3 ? 1u : 0u;
  }
}

// The columns of a window item.  One table row each: element size, how many
// strided sub-columns it has ([sub][cap]: one, one per attribute, one per
// aggregator) and whether snapshots carry it (call / row only mean something
// inside the push that added the item).  ItemStore (host) allocates, grows,
// saves and loads by this table; ItemPtrs is one slot as the kernels see it.
enum ItemCol { I_PK, I_TS, I_SEQ, I_SID, I_LAST, I_CALL, I_ROW, I_ATTR, I_NUL, I_ARGV, I_ARGN, kItemCols };
enum ItemSub { SUB_ONE, SUB_ATTR, SUB_AGG, kItemSubs };
struct ItemColDesc {
  int size;
  ItemSub sub;
  bool saved;
};
constexpr ItemColDesc kItemCol[kItemCols] = {
    {8, SUB_ONE, true},    // I_PK    partition key
    {8, SUB_ONE, true},    // I_TS    event timestamp
    {8, SUB_ONE, true},    // I_SEQ   arrival index (shd_out.in_seq)
    {8, SUB_ONE, true},    // I_SID   aggregator state id
    {8, SUB_ONE, true},    // I_LAST  time windows: the key's lastTimestamp; batch windows: added flag / epoch
    {4, SUB_ONE, false},   // I_CALL  call of the push (-1: carried)
    {4, SUB_ONE, false},   // I_ROW   batch row of the push (-1: carried)
    {8, SUB_ATTR, true},   // I_ATTR  attributes as 64-bit payloads
    {1, SUB_ATTR, true},   // I_NUL   their null flags
    {8, SUB_AGG, true},    // I_ARGV  aggregator arguments
    {1, SUB_AGG, true},    // I_ARGN  their null flags
};
struct ItemPtrs {   // one pointer per column, in ItemCol order
  uint64_t* pk;
  int64_t* ts;
  int64_t* seq;
  uint64_t* sid;
  int64_t* last;
  int32_t* call;
  int32_t* row;
  uint64_t* attr;   // [ncols][cap]
  uint8_t* nul;
  uint64_t* argv;   // [nagg][cap]
  uint8_t* argn;
};
static_assert(sizeof(ItemPtrs) == kItemCols * sizeof(void*), "ItemPtrs: one pointer per ItemCol");

struct ItemOut {
  ItemPtrs it;
  uint64_t* kw;     // [nw][m] state key words of the new items
  uint8_t* kn;
  uint64_t* kh;
};

// New window items [C, C + m): one per passing event.
__global__ __launch_bounds__(kBlock) void k_xw_items(const XwArgs* __restrict__ ap, const ItemOut* __restrict__ op,
                                                     int64_t n, const uint32_t* cnt, const uint32_t* off,
                                                     const uint64_t* pkey, const int32_t* call_of, int64_t m) {
  const XwArgs& a = *ap;
  const ItemOut& o = *op;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i = n) {
    if (!cnt[i]) continue;
    const int64_t j = off[i];
    const int64_t t = a.C + j;
    BatchCtx cx{&a.cs, i};
    o.it.pk[t] = pkey[i];
    o.it.ts[t] = a.cs.ts[i];
    o.it.seq[t] = a.seq0 + i;
    o.it.call[t] = call_of[i];
    o.it.row[t] = (int32_t)i;
    for (int c = 0; c < a.ncols; c++) {
      Val v = col_load(a.cs, i, c);
      o.it.attr[(int64_t)c * a.cap + t] = v.b;
      o.it.nul[(int64_t)c * a.cap + t] = (uint8_t)v.null;
    }
    for (int g = 0; g < a.nagg; g++) {
      Val v{0, 1};
      if (a.has_arg[g]) v = eval_expr(a.es.ins + a.agg_arg[g].off, a.agg_arg[g].len, a.es.consts, cx);
      o.it.argv[(int64_t)g * a.cap + t] = v.b;
      o.it.argn[(int64_t)g * a.cap + t] = (uint8_t)v.null;
    }
    if (a.nw > 0) {
      // state key: (partition key, GroupByKeyGenerator words) -- gdict.h
      uint64_t h = kGdictSeed;
      uint8_t nm = 0;
      int w = 0;
      if (a.partitioned) {
        o.kw[j] = pkey[i];
        h = gdict_hash_step(h, pkey[i], w);
        w++;
      }
      for (int g = 0; g < a.ngk; g++, w++) {
        Val kv = a.group_col[g] >= 0 ? col_load(a.cs, i, a.group_col[g])
                                     : eval_expr(a.es.ins + a.group[g].off, a.group[g].len, a.es.consts, cx);
        bool isnull = false;
        const uint64_t gw = group_word(kv, a.group_type[g], a.null_str_id, isnull);
        o.kw[(int64_t)w * m + j] = gw;
        nm |= (uint8_t)((isnull ? 1u : 0u) << w);
        h = gdict_hash_step(h, gw, w);
      }
      h = gdict_hash_final(h, nm);
      o.kn[j] = nm;
      o.kh[j] = h;
    }
  }
}

// Both slots of the window items (double-buffered: a push reads slot `cur`
// and carries into the other).  Every column operation walks kItemCol.
struct ItemStore {
  int nsub[kItemSubs] = {1, 0, 0};   // sub-columns per ItemSub: 1, ncols, nagg
  int cur = 0;
  int64_t cap[2] = {0, 0};
  DevBuf buf[2][kItemCols];

  void alloc(int s, int64_t n) {
    for (int c = 0; c < kItemCols; c++)
      buf[s][c].reserve((size_t)std::max(nsub[kItemCol[c].sub], 1) * n * kItemCol[c].size);
    cap[s] = n;
  }
  ItemPtrs ptrs(int s) const {
    void* v[kItemCols];
    for (int c = 0; c < kItemCols; c++) v[c] = buf[s][c].p;
    ItemPtrs p;
    std::memcpy(&p, v, sizeof(p));
    return p;
  }
  char* at(int s, int c, int sub) const { return buf[s][c].as<char>() + (size_t)sub * cap[s] * kItemCol[c].size; }
  // f(column, sub-column) for every sub-column, in snapshot order: the
  // per-item columns, then each attribute's columns, then each aggregator's
  template <class F> void each(F f) const {
    for (int k = 0; k < kItemSubs; k++)
      for (int sub = 0; sub < nsub[k]; sub++)
        for (int c = 0; c < kItemCols; c++)
          if (kItemCol[c].sub == k) f(c, sub);
  }
};

}  // namespace

}  // namespace shd
