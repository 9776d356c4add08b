// agg.h -- the reference's incremental aggregator steps on the device.
//
// Sum / Avg / Count AttributeAggregatorExecutor (C/query/selector/attribute/
// aggregator/*.java: processAdd / processRemove): one CURRENT (add) or EXPIRED
// (remove) operand at a time, in the reference's order, so every double sum is
// the same IEEE result (built with -ffp-contract=off).  Below them the
// {Max,Min}[Forever]AttributeAggregatorExecutor steps (mm_step): a value and,
// in tracking mode, the reference's deque, restated with its quirk; and the
// {StdDev,DistinctCount,And,Or}AttributeAggregatorExecutor steps (ext_step).
#pragma once
#include "engine.h"

namespace shd {
namespace {

__device__ __forceinline__ int64_t java_d2l(double d) {
  if (d != d) return 0;
  if (d >= 9.2233720368547758e18) return INT64_MAX;
  if (d <= -9.2233720368547758e18) return INT64_MIN;
  return (int64_t)d;
}

// One aggregator step on a CURRENT (add) or EXPIRED (remove) event: the
// reference's incremental executors, Sum/Avg/CountAttributeAggregatorExecutor
// (.../selector/attribute/aggregator/*.java: processAdd / processRemove).
// ob/on: the aggregator's value after the step (on = null).  avg: ob is the
// running sum and the count is the state c; the division value / count happens
// at emission (k_emit) for the rows that are emitted, not in the sequential fold.
__device__ __forceinline__ void agg_step(int kind, int type, bool add, uint64_t xb, bool xn, double& d, int64_t& l,
                                         int64_t& c, uint64_t& ob, bool& on) {
  ob = 0;
  on = true;
  switch (kind) {
    case SHD_AGG_COUNT:
      c += add ? 1 : -1;
      ob = (uint64_t)c;
      on = false;
      break;
    case SHD_AGG_SUM:
      if (type == SHD_T_INT || type == SHD_T_LONG) {
        if (xn) {
          if (c != 0) { ob = (uint64_t)l; on = false; }
          break;
        }
        int64_t x = type == SHD_T_INT ? (int64_t)v_i32(xb) : (int64_t)xb;
        if (add) {
          l = (int64_t)((uint64_t)l + (uint64_t)x);
          c++;
          ob = (uint64_t)l;
          on = false;
        } else {
          l = java_d2l(__dsub_rn((double)l, (double)x));
          c--;
          if (c != 0) { ob = (uint64_t)l; on = false; }
        }
      } else {
        if (xn) {
          if (type == SHD_T_DOUBLE && c != 0) { ob = p_f64(d); on = false; }
          break;
        }
        double x = type == SHD_T_FLOAT ? (double)v_f32(xb) : v_f64(xb);
        if (add) {
          d = __dadd_rn(d, x);
          c++;
          ob = p_f64(d);
          on = false;
        } else {
          d = __dsub_rn(d, x);
          c--;
          if (c != 0) { ob = p_f64(d); on = false; }
        }
      }
      break;
    case SHD_AGG_AVG: {
      if (xn) {
        if (c != 0) { ob = p_f64(d); on = false; }
        break;
      }
      double x;
      switch (type) {
        case SHD_T_INT: x = (double)v_i32(xb); break;
        case SHD_T_LONG: x = (double)(int64_t)xb; break;
        case SHD_T_FLOAT: x = (double)v_f32(xb); break;
        default: x = v_f64(xb);
      }
      if (add) { c++; d = __dadd_rn(d, x); }
      else { c--; d = __dsub_rn(d, x); }
      if (c != 0) { ob = p_f64(d); on = false; }
      break;
    }
  }
}

// ---------------------------------------------------------------- min / max
// {Max,Min}AttributeAggregatorExecutor.java:84-150 with their state classes
// (:152-), {Max,Min}ForeverAttributeAggregatorExecutor.java:119-200.  A state is
// a value with its null flag and, in tracking mode (processing mode SLIDE or
// expired output, :93-96), a deque of values.  The executors are restated as
// they are, not as a sliding extremum: an add pops the back while it compares
// below (max) / above (min) the new value, a remove is removeFirstOccurrence
// by equals() and leaves peekFirst() as the value -- removing a value an
// earlier add already popped takes a later event's equal value with it.
__device__ __forceinline__ bool agg_is_minmax(int kind) { return kind >= SHD_AGG_MAX; }

// a < b on the unboxed values (Java's <: false against NaN); INT is the signed
// low word of the slot, FLOAT compares as float
__device__ __forceinline__ bool mm_lt(int type, uint64_t a, uint64_t b) {
  switch (type) {
    case SHD_T_INT: return v_i32(a) < v_i32(b);
    case SHD_T_LONG: return (int64_t)a < (int64_t)b;
    case SHD_T_FLOAT: return v_f32(a) < v_f32(b);
    default: return v_f64(a) < v_f64(b);
  }
}
// a gives way to b: a < b for max, a > b for min
__device__ __forceinline__ bool mm_below(bool is_max, int type, uint64_t a, uint64_t b) {
  return is_max ? mm_lt(type, a, b) : mm_lt(type, b, a);
}
__device__ __forceinline__ bool mm_isnan(int type, uint64_t a) {
  if (type == SHD_T_FLOAT) return v_f32(a) != v_f32(a);
  if (type == SHD_T_DOUBLE) return v_f64(a) != v_f64(a);
  return false;
}
// equals() of the boxed values compares these: Integer / Long by value, Float /
// Double by floatToIntBits / doubleToLongBits (every NaN equal, 0.0 != -0.0)
__device__ __forceinline__ uint64_t mm_bits(int type, uint64_t a) {
  switch (type) {
    case SHD_T_INT: return (uint64_t)(uint32_t)a;
    case SHD_T_LONG: return a;
    case SHD_T_FLOAT: return mm_isnan(type, a) ? 0x7fc00000ull : (uint64_t)(uint32_t)a;
    default: return mm_isnan(type, a) ? 0x7ff8000000000000ull : a;
  }
}

// One state's deque while a push folds it: the live elements are w[h, t) of
// the lane's own region of `room` slots (the carried deque copied to its
// front; every add appends at most one element).
struct MmDeque {
  uint64_t* w;
  int64_t h, t, room;
};

// The deque position of removeFirstOccurrence(x), -1 when absent.  While no
// NaN has entered the deque since it was last empty it is monotone (max:
// non-increasing), so the elements numerically equal to x are one run found by
// two binary searches, and equals() is decided inside that run alone (it
// separates 0.0 from -0.0).  After a NaN the order is lost: the literal scan.
__device__ __forceinline__ int64_t mm_find(bool is_max, int type, const MmDeque& q, bool had_nan, uint64_t x) {
  const uint64_t xb = mm_bits(type, x);
  int64_t lo = q.h, hi = q.t;
  if (!had_nan) {
    if (mm_isnan(type, x)) return -1;
    int64_t e = q.t;
    while (lo < e) {   // first element that does not beat x
      const int64_t mid = (lo + e) >> 1;
      if (mm_below(is_max, type, x, q.w[mid])) lo = mid + 1;
      else e = mid;
    }
    hi = lo;
    e = q.t;
    while (hi < e) {   // first element x beats
      const int64_t mid = (hi + e) >> 1;
      if (!mm_below(is_max, type, q.w[mid], x)) hi = mid + 1;
      else e = mid;
    }
  }
  for (int64_t i = lo; i < hi; i++)
    if (mm_bits(type, q.w[i]) == xb) return i;
  return -1;
}

// One step of a min / max / minForever / maxForever state.  val: the value's
// payload; flags: bit 0 the value is set (non-null), bit 1 the deque has taken
// a NaN since it was last empty; q: the tracking deque, null without tracking.
// ob / on: the aggregator's value after the step, in the argument's type.
__device__ __forceinline__ void mm_step(int kind, int type, bool add, uint64_t x, bool xn, uint64_t& val,
                                        int64_t& flags, MmDeque* q, uint64_t& ob, bool& on) {
  const bool is_max = kind == SHD_AGG_MAX || kind == SHD_AGG_MAX_FOREVER;
  bool has = (flags & 1) != 0;
  if (xn) {
    // a null argument leaves the state alone (processAdd / processRemove :120-139)
  } else if (kind == SHD_AGG_MAX_FOREVER || kind == SHD_AGG_MIN_FOREVER) {
    // add and remove alike (MaxForever...StateDouble :158-174)
    if (!has || mm_below(is_max, type, val, x)) val = x;
    has = true;
  } else if (add) {
    if (q) {
      while (q->t > q->h && mm_below(is_max, type, q->w[q->t - 1], x)) q->t--;   // descendingIterator (:167-173)
      if (q->t == q->h) flags &= ~(int64_t)2;
      if (q->t < q->room) q->w[q->t++] = x;                                      // addLast (:174)
      if (mm_isnan(type, x)) flags |= 2;
    }
    if (!has || mm_below(is_max, type, val, x)) val = x;   // :176-178
    has = true;
  } else if (q) {
    const int64_t i = mm_find(is_max, type, *q, (flags & 2) != 0, x);   // removeFirstOccurrence (:185)
    if (i >= 0) {
      // close the gap from the shorter side
      if (i - q->h <= q->t - 1 - i) {
        for (int64_t j = i; j > q->h; j--) q->w[j] = q->w[j - 1];
        q->h++;
      } else {
        for (int64_t j = i; j + 1 < q->t; j++) q->w[j] = q->w[j + 1];
        q->t--;
      }
    }
    has = q->t > q->h;   // peekFirst (:186)
    if (has) val = q->w[q->h];
    else flags &= ~(int64_t)2;
  } else if (has && mm_bits(type, val) == mm_bits(type, x)) {
    has = false;   // without tracking: maxValue.equals(data) (:188-190)
  }
  flags = (flags & ~(int64_t)1) | (has ? 1 : 0);
  ob = has ? val : 0;
  on = !has;
}

// ---------------------------------------------------------------- stdDev / distinctCount / and / or
// {StdDev,DistinctCount,And,Or}AttributeAggregatorExecutor.java.  They use the
// three state scalars as follows (d, l, c of the fold):
//   stdDev         d = sum, l = the bits of stdDeviation, c = count; the mean is
//                  not stored: whenever count >= 1 the reference's mean is the
//                  double sum / count of exactly these two values
//   and / or       l = trueEventsCount, c = falseEventsCount
//   distinctCount  l = the count of the null key, c = the number of other keys;
//                  the keys are a list of (key bits, count) pairs in the list
//                  store, sorted by key bits
__device__ __forceinline__ bool agg_is_ext(int kind) { return kind >= SHD_AGG_STDDEV; }

// StdDevAttributeAggregatorExecutor.java:157-231 (Welford's update, add and
// remove), :115-133 (a null argument returns currentValue()).  Every operation
// is one correctly rounded IEEE operation in the reference's order; a negative
// stdDeviation residue gives NaN from the square root, as Math.sqrt does.
__device__ __forceinline__ void sd_step(int type, bool add, uint64_t xb, bool xn, double& sum, int64_t& sdb,
                                        int64_t& c, uint64_t& ob, bool& on) {
  double sd = __longlong_as_double(sdb);
  if (!xn) {
    double v;
    switch (type) {   // (double) of the unboxed Integer / Long / Float (:237-300)
      case SHD_T_INT: v = (double)v_i32(xb); break;
      case SHD_T_LONG: v = (double)(int64_t)xb; break;
      case SHD_T_FLOAT: v = (double)v_f32(xb); break;
      default: v = v_f64(xb);
    }
    // the mean before this step: sum / count as the last step computed it
    // (0.0 at count 0, where every field is zeroed)
    const double old_mean = c == 0 ? 0.0 : __ddiv_rn(sum, (double)c);
    if (add) {
      c++;                               // :159
      if (c == 1) {                      // :162-165
        sum = v;
        sd = 0.0;
      } else if (c != 0) {               // :166-171
        sum = __dadd_rn(sum, v);
        const double mean = __ddiv_rn(sum, (double)c);
        sd = __dadd_rn(sd, __dmul_rn(__dsub_rn(v, old_mean), __dsub_rn(v, mean)));
      }
    } else {
      c--;                               // :176
      if (c == 0) {                      // :177-180
        sum = 0.0;
        sd = 0.0;
      } else {                           // :181-186
        sum = __dsub_rn(sum, v);
        const double mean = __ddiv_rn(sum, (double)c);
        sd = __dsub_rn(sd, __dmul_rn(__dsub_rn(v, old_mean), __dsub_rn(v, mean)));
      }
    }
  }
  sdb = __double_as_longlong(sd);
  // null at count 0, 0.0 at count 1, else Math.sqrt(stdDeviation / count) (:224-231)
  on = c == 0;
  ob = (on || c == 1) ? p_f64(0.0) : p_f64(__dsqrt_rn(__ddiv_rn(sd, (double)c)));
}

// {And,Or}AttributeAggregatorExecutor.java:98-144.  The reference unboxes a
// null argument and fails the call; here it leaves the counters alone.
__device__ __forceinline__ void bool_step(int kind, bool add, uint64_t xb, bool xn, int64_t& nt, int64_t& nf,
                                          uint64_t& ob, bool& on) {
  if (!xn) {
    if (xb & 1) nt += add ? 1 : -1;
    else nf += add ? 1 : -1;
  }
  ob = kind == SHD_AGG_AND ? (nt > 0 && nf == 0) : (nt > 0);   // computeLogicalOperation (:142-144)
  on = false;
}

// What equals() / hashCode() of the boxed key compare: mm_bits for the numeric
// types, the dictionary id of a String, the value of a Boolean.
__device__ __forceinline__ uint64_t dc_key(int type, uint64_t a) {
  switch (type) {
    case SHD_T_INT: case SHD_T_LONG: case SHD_T_FLOAT: case SHD_T_DOUBLE: return mm_bits(type, a);
    case SHD_T_BOOL: return a & 1;
    default: return (uint64_t)(uint32_t)a;
  }
}

// DistinctCountAttributeAggregatorExecutor.java:105-131: a HashMap<Object, Long>
// as a list of (key, count) pairs sorted by key bits in w[h, t) of the lane's
// region (two words a pair; an add creates at most one).  Find is a binary
// search; a new key opens its gap, and a key whose count reaches 0 closes it,
// from the shorter side -- linear in the list in the worst case.  Null is a key
// (HashMap allows it): its count is nnull.  Removing a key that is not there
// throws in the reference; no supported plan does it, here it is a no-op.
__device__ __forceinline__ void dc_step(int type, bool add, uint64_t xb, bool xn, int64_t& nnull, int64_t& nkeys,
                                        MmDeque* q, uint64_t& ob, bool& on) {
  if (xn) {
    if (add) nnull++;
    else if (nnull > 0) nnull--;
  } else if (q) {
    const uint64_t k = dc_key(type, xb);
    int64_t lo = 0, n = (q->t - q->h) >> 1;
    while (lo < n) {   // the first pair whose key is not below k
      const int64_t mid = (lo + n) >> 1;
      if (q->w[q->h + 2 * mid] < k) lo = mid + 1;
      else n = mid;
    }
    int64_t i = q->h + 2 * lo;
    const bool found = i < q->t && q->w[i] == k;
    if (add && found) {
      q->w[i + 1]++;                                     // put(data, ++preVal) (:107-108)
    } else if (add) {
      // put(data, 1L) (:110): the region holds the carried pairs plus one per
      // operation, so one side always has room
      const bool left = q->h >= 2 && (i - q->h <= q->t - i || q->t + 2 > q->room);
      if (left) {
        for (int64_t j = q->h; j < i; j++) q->w[j - 2] = q->w[j];
        q->h -= 2;
        i -= 2;
      } else if (q->t + 2 <= q->room) {
        for (int64_t j = q->t - 1; j >= i; j--) q->w[j + 2] = q->w[j];
        q->t += 2;
      } else {
        i = -1;
      }
      if (i >= 0) {
        q->w[i] = k;
        q->w[i + 1] = 1;
      }
    } else if (found && --q->w[i + 1] == 0) {            // remove(data) at 0 (:124-129)
      if (i - q->h <= q->t - 2 - i) {
        for (int64_t j = i + 1; j >= q->h + 2; j--) q->w[j] = q->w[j - 2];
        q->h += 2;
      } else {
        for (int64_t j = i; j + 2 < q->t; j++) q->w[j] = q->w[j + 2];
        q->t -= 2;
      }
    }
    nkeys = (q->t - q->h) >> 1;
  }
  ob = (uint64_t)(nkeys + (nnull > 0 ? 1 : 0));          // distinctValues.size() (:167-169)
  on = false;
}

// One step of a stdDev / distinctCount / and / or state.
__device__ __forceinline__ void ext_step(int kind, int type, bool add, uint64_t xb, bool xn, double& d, int64_t& l,
                                         int64_t& c, MmDeque* q, uint64_t& ob, bool& on) {
  if (kind == SHD_AGG_STDDEV) sd_step(type, add, xb, xn, d, l, c, ob, on);
  else if (kind == SHD_AGG_DISTINCT_COUNT) dc_step(type, add, xb, xn, l, c, q, ob, on);
  else bool_step(kind, add, xb, xn, l, c, ob, on);
}

}  // namespace
}  // namespace shd
