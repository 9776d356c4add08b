// knobs.h -- every SHD_* environment switch the library reads, and the only
// place that calls getenv.  Standard library only: a plain C++ program can
// include it (tests/test_knobs.py does).  The table in DESIGN.md
// ("Environment switches") mirrors this list.
//
// X(id, environment name, kind, when read, effect)
//   kind  FLAG      knob_on():    set, non-empty and not beginning with '0'
//         TRISTATE  knob_force(): -1 unset or empty, 0 begins with '0', 1 otherwise
//         INT       knob_int():   false when unset or empty, else v = atoi(value);
//                                 the caller checks the range
//   when  PROCESS   once per process (cached by the caller)
//         LOAD      at plan load / engine construction
//         PUSH      on every push
// `when` records where the read sits; no accessor caches, so a test can flip a
// variable between two engines of one process.
#pragma once
#include <cassert>
#include <cstdlib>

namespace shd {

#define SHD_KNOBS(X)                                                                                                  \
  /* shd_api.cpp */                                                                                                   \
  X(SYNC_CHECK, "SHD_SYNC_CHECK", FLAG, PROCESS, "synchronize after every kernel launch so a fault names its launch") \
  X(NO_FAST_PRED, "SHD_NO_FAST_PRED", FLAG, PUSH, "filters run on the expression interpreter, never pre-decoded")     \
  X(FORCE_NFA, "SHD_FORCE_NFA", FLAG, LOAD, "every state plan runs on the generic NFA engine")                        \
  X(NO_LOGICAL_SCAN, "SHD_NO_LOGICAL_SCAN", FLAG, LOAD, "`every e1 -> (e2 or/and e3)` runs on the generic NFA engine") \
  X(NO_ABSENT_SCAN, "SHD_NO_ABSENT_SCAN", FLAG, LOAD, "`every e1 -> not X for t` runs on the generic NFA engine")     \
  /* engine_pattern.hip */                                                                                            \
  X(NO_HASH, "SHD_NO_HASH", FLAG, PUSH, "pattern: never sort by hashed buckets")                                      \
  X(HASH_BITS, "SHD_HASH_BITS", INT, PUSH, "pattern: sort by this many hashed-bucket bits (outside 1..32: none)")     \
  X(FUSED_SORT, "SHD_FUSED_SORT", TRISTATE, PUSH, "pattern: fused prepare + first sort pass off / on at any push size") \
  X(TS64, "SHD_TS64", FLAG, PUSH, "pattern: 64-bit sorted timestamps even when 32-bit offsets fit")                   \
  X(RESUME_MODE, "SHD_RESUME_MODE", INT, PUSH, "pattern: deferred-walk mode 0..3 (ignored where the mode cannot run)") \
  X(LOCKSTEP, "SHD_LOCKSTEP", TRISTATE, PUSH, "pattern: lockstep walks off / on wherever they can run")               \
  X(NO_BPOS, "SHD_NO_BPOS", FLAG, PUSH, "pattern: never copy e2 attributes into position order (wins over SHD_BPOS)") \
  X(BPOS, "SHD_BPOS", FLAG, PUSH, "pattern: position-major e2 attributes whenever walks are dense")                   \
  X(NO_SPLIT, "SHD_NO_SPLIT", FLAG, PUSH, "pattern: f2 through eval_fpred per step, not split per comparison")        \
  X(NO_BLOCK_SKIP, "SHD_NO_BLOCK_SKIP", FLAG, PUSH, "pattern: walks never skip 64-position blocks (wins over SHD_BLOCK_SKIP)") \
  X(BLOCK_SKIP, "SHD_BLOCK_SKIP", FLAG, PUSH, "pattern: block skipping at any key density")                           \
  X(NO_RESUME_LIST, "SHD_NO_RESUME_LIST", FLAG, PUSH, "pattern: sparse deferred walks without the compacted list")    \
  X(NO_SCAN_LISTS, "SHD_NO_SCAN_LISTS", FLAG, PUSH, "pattern: open and deferred lists by the list passes, not from the scan") \
  X(NO_IMPLICIT_KEY, "SHD_NO_IMPLICIT_KEY", FLAG, LOAD, "pattern: a key equality in f2 does not partition the plan")  \
  X(NO_LEAN_SORT, "SHD_NO_LEAN_SORT", FLAG, PUSH, "pattern: never the lean (two-word) key sort (wins over SHD_LEAN_SORT)") \
  X(LEAN_SORT, "SHD_LEAN_SORT", FLAG, PUSH, "pattern: the lean key sort wherever it can run, at any key density")     \
  X(SCAN_ROW_WALK, "SHD_SCAN_ROW_WALK", FLAG, PUSH, "pattern: the lean scan walks its undecided candidates itself, from their rows") \
  /* keyed_sort.hip */                                                                                                \
  X(KS_GENERIC_F1, "SHD_KS_GENERIC_F1", FLAG, PUSH, "fused sort: f1 through eval_fpred per row, not pre-decoded")     \
  /* engine_nfa.hip */                                                                                                \
  X(NFA_DEBUG, "SHD_NFA_DEBUG", FLAG, LOAD, "NFA: print window-lane decisions (and phase clocks in the prof build)")  \
  X(NFA_CHUNK, "SHD_NFA_CHUNK", INT, PUSH, "NFA: window-lane chunk length in events (at least 1)")                    \
  X(NFA_HASH1_ZERO, "SHD_NFA_HASH1_ZERO", FLAG, PUSH, "NFA: zero the first window-lane state hash (forces the fallback)") \
  X(NFA_WINDOW, "SHD_NFA_WINDOW", TRISTATE, LOAD, "NFA: 0 turns window lanes off")                                    \
  X(NFA_LIST, "SHD_NFA_LIST", INT, LOAD, "NFA: pending-list capacity per key (> 0)")                                  \
  X(NFA_PARTIALS, "SHD_NFA_PARTIALS", INT, LOAD, "NFA: partial capacity per key (> 0)")                               \
  X(NFA_EVENTS, "SHD_NFA_EVENTS", INT, LOAD, "NFA: event capacity per key (> 0)")                                     \
  X(NFA_RECORDS, "SHD_NFA_RECORDS", INT, LOAD, "NFA: record capacity per key (> 0)")                                  \
  X(NFA_TIMERS, "SHD_NFA_TIMERS", INT, LOAD, "NFA: timer capacity per key (> 0)")                                     \
  /* engine_single.hip */                                                                                             \
  X(DEBUG_ARGS, "SHD_DEBUG_ARGS", FLAG, PUSH, "filter: print k_filter's arguments and stop before the launch")        \
  X(WCHUNK, "SHD_WCHUNK", FLAG, PUSH, "windows: the chunked walk (opt-in)")                                           \
  X(NO_WCHUNK, "SHD_NO_WCHUNK", FLAG, PUSH, "windows: never the chunked walk (wins over SHD_WCHUNK)")                 \
  X(NO_CALLWIN, "SHD_NO_CALLWIN", FLAG, PUSH, "windows: never the call-window path")                                  \
  X(FOLD_LANE, "SHD_FOLD_LANE", FLAG, PUSH, "group fold: one lane per group at any segment length")                   \
  X(FOLD_GENERIC, "SHD_FOLD_GENERIC", FLAG, PUSH, "group fold: the generic fold, not the sum + count one")            \
  X(EXACT_AGGREGATES, "SHD_EXACT_AGGREGATES", FLAG, LOAD, "aggregates: the in-order running fold, not segmented scans") \
  X(GROUP_DICT, "SHD_GROUP_DICT", FLAG, LOAD, "group by: the group dictionary for every key, dense ids for none")

enum class Knob : int {
#define X(id, name, kind, when, doc) id,
  SHD_KNOBS(X)
#undef X
};

enum class KnobKind { FLAG, TRISTATE, INT };
enum class KnobWhen { PROCESS, LOAD, PUSH };

struct KnobInfo {
  const char* name;
  KnobKind kind;
  KnobWhen when;
  const char* doc;
};

inline constexpr KnobInfo kKnobs[] = {
#define X(id, name, kind, when, doc) {name, KnobKind::kind, KnobWhen::when, doc},
    SHD_KNOBS(X)
#undef X
};
inline constexpr int kNumKnobs = (int)(sizeof(kKnobs) / sizeof(kKnobs[0]));

// the value of a knob of kind `kind`, nullptr when unset or empty
inline const char* knob_value(Knob k, KnobKind kind) {
  const KnobInfo& info = kKnobs[(int)k];
  assert(info.kind == kind);
  (void)kind;
  const char* v = std::getenv(info.name);
  return v && *v ? v : nullptr;
}

inline bool knob_on(Knob k) {
  const char* v = knob_value(k, KnobKind::FLAG);
  return v && *v != '0';
}

inline int knob_force(Knob k) {
  const char* v = knob_value(k, KnobKind::TRISTATE);
  return !v ? -1 : *v == '0' ? 0 : 1;
}

inline bool knob_int(Knob k, int& out) {
  const char* v = knob_value(k, KnobKind::INT);
  if (v) out = std::atoi(v);
  return v != nullptr;
}

}  // namespace shd
