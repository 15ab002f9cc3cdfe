// lane_search.h — the shape every tree search on the device shares (k_solve, k_search,
// k_solve_deep, k_leaf_solve): one lane runs one search at a time, a lane whose search ended
// takes the next task index from a global counter, and the kernel loop is "every lane with
// work advances one node", so a wave diverges inside one node step at most, never across
// whole searches.  The frames below each lane's top frame live in LDS, laid out
// [frame][field][lane]: the 64 lanes of a wave touch 64 consecutive 8-byte or 4-byte words,
// conflict-free, and nothing is a runtime-indexed private array.
//
// Every loop is bounded: a search ends after node_limit nodes at the latest, the lane loop
// ends when the task counter passes the task count, and no lane waits for another.
//
// The search itself (Search, init, step) comes from the header of its namespace (solve.h,
// search.h, solve_deep.h) and its kRun / kDone states from negamax.h; step is found through
// its Search argument.
#pragma once
#include <algorithm>

#include "common.h"
#include "negamax.h"

namespace azl {

using azn::kDone;
using azn::kRun;
constexpr int kLdsBytes = 160 * 1024;

// A lane's column of the block's frame stack: WORDS 8-byte fields per frame, then (PACKED) one
// 4-byte word, in one LDS array of words(nf) 8-byte words: [nf][WORDS][BLOCK] u64, then
// [nf][BLOCK] u32.  put / get are the ones step() of the namespace calls.
template <int BLOCK, int WORDS, bool PACKED>
struct LdsStack {
  static constexpr int kFrameBytes = WORDS * 8 + (PACKED ? 4 : 0);
  static constexpr int lds_bytes(int nf) { return nf * BLOCK * kFrameBytes; }
  static constexpr int words(int nf) { return lds_bytes(nf) / 8; }
  static_assert(BLOCK % 64 == 0 && (WORDS == 2 || WORDS == 3), "whole waves, two or three fields");

  uint64_t* w;
  uint32_t* p;
  __device__ __forceinline__ LdsStack(uint64_t* lds, int nf)
      : w(lds + threadIdx.x),
        p(reinterpret_cast<uint32_t*>(lds + nf * WORDS * BLOCK) + threadIdx.x) {}

  __device__ __forceinline__ void put(int f, uint64_t a, uint64_t b, uint32_t pk) {
    static_assert(WORDS == 2 && PACKED, "frame of two fields and a packed word");
    w[(2 * f) * BLOCK] = a;
    w[(2 * f + 1) * BLOCK] = b;
    p[f * BLOCK] = pk;
  }
  __device__ __forceinline__ void get(int f, uint64_t& a, uint64_t& b, uint32_t& pk) const {
    static_assert(WORDS == 2 && PACKED, "frame of two fields and a packed word");
    a = w[(2 * f) * BLOCK];
    b = w[(2 * f + 1) * BLOCK];
    pk = p[f * BLOCK];
  }
  __device__ __forceinline__ void put(int f, uint64_t a, uint64_t b, uint64_t c) {
    static_assert(WORDS == 3 && !PACKED, "frame of three fields");
    w[(3 * f) * BLOCK] = a;
    w[(3 * f + 1) * BLOCK] = b;
    w[(3 * f + 2) * BLOCK] = c;
  }
  __device__ __forceinline__ void get(int f, uint64_t& a, uint64_t& b, uint64_t& c) const {
    static_assert(WORDS == 3 && !PACKED, "frame of three fields");
    a = w[(3 * f) * BLOCK];
    b = w[(3 * f + 1) * BLOCK];
    c = w[(3 * f + 2) * BLOCK];
  }
  __device__ __forceinline__ void put(int f, uint64_t a, uint64_t b, uint64_t c, uint32_t pk) {
    static_assert(WORDS == 3 && PACKED, "frame of three fields and a packed word");
    w[(3 * f) * BLOCK] = a;
    w[(3 * f + 1) * BLOCK] = b;
    w[(3 * f + 2) * BLOCK] = c;
    p[f * BLOCK] = pk;
  }
  __device__ __forceinline__ void get(int f, uint64_t& a, uint64_t& b, uint64_t& c,
                                      uint32_t& pk) const {
    static_assert(WORDS == 3 && PACKED, "frame of three fields and a packed word");
    a = w[(3 * f) * BLOCK];
    b = w[(3 * f + 1) * BLOCK];
    c = w[(3 * f + 2) * BLOCK];
    pk = p[f * BLOCK];
  }
};

// The lane loop.  start(s, t) begins task t < n (the namespace's init), ended(s) takes the
// results of a search that has just ended; a search that init already finished ends in the
// same turn.
template <class Search, class Stack, class Start, class Ended>
__device__ __forceinline__ void run_lanes(Stack& st, uint32_t n, uint32_t* __restrict__ queue,
                                          uint64_t node_limit, int frames, Start start,
                                          Ended ended) {
  Search s;
  s.state = kDone;
  for (;;) {
    if (s.state != kRun) {  // no work: take the next task, or leave
      const uint32_t t = atomicAdd(queue, 1u);
      if (t >= n) break;
      start(s, t);
    } else {
      step(s, st, node_limit, frames);
    }
    if (s.state != kRun) ended(s);
  }
}

// every array of a workspace starts on a 256-byte boundary
inline size_t align_up(size_t x) { return (x + 255) & ~size_t(255); }

// Grid of a launch that fills the device: per CU as many blocks as their LDS lets in, 16 at
// the most; with the task count known on the host (n_ptr null), no more lanes than tasks.
inline int fill_grid(unsigned* grid, int block, int lds_bytes, const uint32_t* n_ptr,
                     uint32_t n_host) {
  int dev = 0, cus = 0;
  AZ_HIP(hipGetDevice(&dev));
  AZ_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  const int per_cu = std::min(16, kLdsBytes / lds_bytes);
  unsigned g = (unsigned)(cus > 0 ? cus : 1) * (unsigned)per_cu;
  if (!n_ptr) {
    const unsigned need = (n_host + block - 1) / block;
    g = need < g ? (need < 1 ? 1 : need) : g;
  }
  *grid = g;
  return AZ_OK;
}

// The argument and workspace protocol of a *_gpu entry point `who` over n items (`what` names
// them), after the checks of its own: n and split_plies in range, a query (null workspace)
// answered with `need`, the workspace large enough and 8-byte aligned, nothing to do for
// n = 0, no null buffer.  *run tells whether there is work; a rejected call writes nothing.
inline int claim_workspace(const char* who, const char* what, int64_t n, int32_t split_plies,
                           size_t need, void* workspace, size_t* workspace_bytes, bool buffers,
                           bool* run) {
  *run = false;
  AZ_REQUIRE(n >= 0 && n < (int64_t(1) << 31), AZ_ERR_ARG, "%s: %s=%lld outside 0..2^31", who,
             what, (long long)n);
  AZ_REQUIRE(split_plies >= 0 && split_plies <= 2, AZ_ERR_ARG, "%s: split_plies=%d outside 0..2",
             who, (int)split_plies);
  AZ_REQUIRE(workspace_bytes, AZ_ERR_ARG, "%s: null workspace_bytes", who);
  if (!workspace) {
    *workspace_bytes = need;
    return AZ_OK;
  }
  AZ_REQUIRE(*workspace_bytes >= need, AZ_ERR_ARG, "%s: workspace %zu < %zu bytes", who,
             *workspace_bytes, need);
  AZ_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0, AZ_ERR_ARG,
             "%s: workspace must be 8-byte aligned", who);
  if (n == 0) return AZ_OK;
  AZ_REQUIRE(buffers, AZ_ERR_ARG, "%s: null buffer", who);
  *run = true;
  return AZ_OK;
}

}  // namespace azl
