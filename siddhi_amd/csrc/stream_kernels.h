// stream_kernels.h -- the small front-end kernels of the single-stream engines
// (engine_single.hip, engine_window.hip): calls, partition runs, key segments.
// All are grid-stride loops, correct under any grid.  They sit in an unnamed
// namespace: each engine's code object carries its own copy, under the name
// it has always had in profiles (shd::(anonymous namespace)::k_narrow, ...).
#pragma once
#include "common.h"

namespace shd {

namespace {

// call_of[i] for every event; call_last_ts[c]
__global__ void k_call_of(const int64_t* offs, int ncalls, const int64_t* ts, int32_t* call_of, int64_t* last_ts) {
  for (int c = blockIdx.x; c < ncalls; c += gridDim.x) {
    int64_t a = offs[c], b = offs[c + 1];
    for (int64_t i = a + threadIdx.x; i < b; i += blockDim.x) call_of[i] = c;
    if (threadIdx.x == 0) last_ts[c] = b > a ? ts[b - 1] : INT64_MIN;
  }
}

// Partition runs (PartitionStreamReceiver.receive(Event[]) :189-214): a run
// starts at the first keyed event of a call or where the key changes from the
// previous keyed event.  run_start[i] in {0,1}; computed over keyed events.
__global__ void k_run_starts(const uint8_t* flags, const uint64_t* pkey, const int32_t* call_of, int64_t n,
                             uint32_t* start) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    uint32_t s = 0;
    if (flags[i] & 2) {
      int64_t p = i - 1;
      while (p >= 0 && call_of[p] == call_of[i] && !(flags[p] & 2)) p--;
      s = (p < 0 || call_of[p] != call_of[i] || pkey[p] != pkey[i]) ? 1u : 0u;
    }
    start[i] = s;
  }
}

__global__ void k_narrow(const uint64_t* in, uint32_t* out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    out[i] = (uint32_t)in[i];
}

__global__ void k_gather_u64(const uint64_t* src, const uint32_t* perm, uint64_t* dst, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    dst[i] = src[perm[i]];
}

__global__ void k_seg_heads(const uint32_t* skey, int64_t n, uint32_t* head) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    head[i] = (i == 0 || skey[i] != skey[i - 1]) ? 1u : 0u;
}

__global__ void k_seg_heads_u64(const uint64_t* skey, int64_t n, uint32_t* head) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    head[i] = (i == 0 || skey[i] != skey[i - 1]) ? 1u : 0u;
}

__global__ void k_head_list(const uint32_t* head, const uint32_t* hoff, int64_t n, uint32_t* hl) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    if (head[i]) hl[hoff[i]] = (uint32_t)i;
}

__global__ void k_fill_u64(uint64_t* p, int64_t n, uint64_t v) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    p[i] = v;
}

}  // namespace

}  // namespace shd
