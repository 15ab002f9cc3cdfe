// split_front.h — the split front end of the batched tree searches (oth_solve_gpu,
// oth_search_gpu, oth_solve_deep_gpu with split_plies = 1 or 2), once.
//
// Roots are expanded level by level into their children (k_split_expand; child slots by
// atomicAdd), every leaf of that small tree is a task of the search's lane kernel
// (lane_search.h), and the levels are combined bottom-up (k_split_combine) by atomicMax on the
// key (value + bias) << 8 | (255 - action): independent of the order of arrival, and the
// lowest action among the best.  k_split_finish writes the roots' results.  Roots go through
// the workspace in chunks.  With split_plies = 0 the roots themselves are the tasks.
//
// A search describes itself by a traits struct T:
//   Value                   element type of the value output (int8_t / int16_t)
//   kBias, kAborted         key bias (above every |value|) and the abort code
//   kChunk1, kChunk2        roots per chunk with one / two split plies
//   Params                  what the entry point was called with (a kernel argument)
//   children1/2(par)        children per node, at most, on level 1 / level 2
//   expand_root(par, o, p)  whether a root with disjoint boards is split at all
//   kExtras                 per-node extra bytes (0..2: nothing, a depth, a window), with
//   root_extra(par)         the bytes of a root,
//   child_extra(x, pass)    the bytes of a child of a node with bytes x; the lane kernel reads
//                           them through TaskList::extra when the task starts.
//
// A level that overruns: the caps are chunk * children1 and chunk * children1 * children2
// nodes.  A node whose children do not fit is marked aborted (so is its root), writes no
// child, and the one node that crosses the end fills the slots it was handed below it with
// inert nodes (an empty board: a task that ends at once), so a later level and the combine
// read no slot that was never written.  For the alpha-beta search an arbitrary board with
// more than 33 placements gets there.  For the two solvers it is unreachable: a split root has
// e <= max_empties empties and so at most e children; a pass child keeps e but is one node,
// and every placement child has e - 1 empties, so the caps are the worst case.
#pragma once
#include "bitboard.h"
#include "common.h"
#include "lane_search.h"

namespace azf {

constexpr int kAuxBlock = 256;

// counters of one chunk
enum { kCtrQueue = 0, kCtrTasks = 1, kCtrL1 = 2, kCtrL2 = 3, kCtrWords = 4 };

struct Extra {
  uint8_t b[2];
};

template <class T>
struct SplitWs {
  uint64_t *own, *opp, *nodes;
  int32_t *parent, *task;
  uint32_t *key, *abort, *ctr;
  typename T::Value* value;
  uint8_t *action, *best, *expanded;
  uint8_t* extra[2];  // T::kExtras of them
};

// What a lane kernel is launched over: task t < *n_ptr (or n_host) is position ids[t] (or t
// itself) of own / opp with the extra bytes extra[k][node]; results go to the same index.
template <class T>
struct TaskList {
  const uint64_t *own, *opp;
  const int32_t* ids;
  const uint8_t* extra[2];
  const uint32_t* n_ptr;
  uint32_t n_host;
  uint32_t* queue;
  typename T::Value* value;
  uint8_t* best;
  uint64_t* nodes;
};

// One level of the expansion: node i of the level (count from the host, or from the counter
// count_ctr) either becomes a task or gets its children in the next level.  Level 0 (src_own
// given) copies the roots in and expands those T::expand_root admits; deeper levels expand
// every non-terminal node.
template <class T>
__global__ __launch_bounds__(kAuxBlock) void k_split_expand(
    SplitWs<T> ws, const uint64_t* __restrict__ src_own, const uint64_t* __restrict__ src_opp,
    uint32_t base, uint32_t count_host, int count_ctr, uint32_t next_base, uint32_t next_cap,
    int next_ctr, int child_tasks, typename T::Params par) {
  const uint32_t count = count_ctr >= 0 ? min(ws.ctr[count_ctr], count_host) : count_host;
  const uint32_t stride = gridDim.x * kAuxBlock;
  for (uint32_t i = blockIdx.x * kAuxBlock + threadIdx.x; i < count; i += stride) {
    const uint32_t node = base + i;
    uint64_t o, p;
    Extra x{};
    bool expand = true;
    if (src_own) {
      o = src_own[i];
      p = src_opp[i];
      x = T::root_extra(par);
      ws.own[node] = o;
      ws.opp[node] = p;
      ws.parent[node] = -1;
      ws.action[node] = azb::kPass;
      for (int k = 0; k < T::kExtras; ++k) ws.extra[k][node] = x.b[k];
      expand = (o & p) == 0 && T::expand_root(par, o, p);
    } else {
      o = ws.own[node];
      p = ws.opp[node];
      for (int k = 0; k < T::kExtras; ++k) x.b[k] = ws.extra[k][node];
    }
    ws.key[node] = 0;
    ws.abort[node] = 0;
    ws.nodes[node] = 0;
    uint64_t m = 0;
    bool pass = false;
    if (expand) {
      m = azb::legal(o, p);
      if (!m) {
        pass = azb::legal(p, o) != 0;
        expand = pass;
      }
    }
    const Extra cx = T::child_extra(x, pass);
    uint32_t k = 0, slot = 0;
    if (expand) {
      k = pass ? 1u : (uint32_t)azb::popc(m);
      slot = atomicAdd(&ws.ctr[next_ctr], k);
      if (slot + k > next_cap) {  // the level overruns: see the head of this file
        ws.abort[node] = 1;
        for (uint32_t c = next_base + min(slot, next_cap); c < next_base + next_cap; ++c) {
          ws.own[c] = 0;
          ws.opp[c] = 0;
          ws.parent[c] = (int32_t)node;
          ws.action[c] = azb::kPass;
          ws.expanded[c] = 0;
          for (int e = 0; e < T::kExtras; ++e) ws.extra[e][c] = cx.b[e];
          ws.nodes[c] = 0;
          ws.value[c] = (typename T::Value)T::kAborted;
        }
        k = 0;
      }
    }
    ws.expanded[node] = expand ? 1 : 0;
    if (!expand) {
      ws.task[atomicAdd(&ws.ctr[kCtrTasks], 1u)] = (int32_t)node;
      continue;
    }
    ws.nodes[node] = 1;
    const uint32_t tb = (child_tasks && k) ? atomicAdd(&ws.ctr[kCtrTasks], k) : 0u;
    for (uint32_t j = 0; j < k; ++j) {
      int a = azb::kPass;
      uint64_t cap = 0;
      if (!pass) {
        a = __builtin_ctzll(m);
        m &= m - 1;
        cap = azb::flips(o, p, a);
      }
      const uint32_t c = next_base + slot + j;
      azb::play(o, p, a, cap, &ws.own[c], &ws.opp[c]);
      ws.parent[c] = (int32_t)node;
      ws.action[c] = (uint8_t)a;
      ws.expanded[c] = 0;
      for (int e = 0; e < T::kExtras; ++e) ws.extra[e][c] = cx.b[e];
      if (child_tasks) ws.task[tb + j] = (int32_t)c;
    }
  }
}

// One level of the combine: every node of the level hands its value (a task's value, or the
// key its own children left) to its parent.  Every child has the other side to move, so the
// parent's value of the move is the negated child value.
template <class T>
__global__ __launch_bounds__(kAuxBlock) void k_split_combine(SplitWs<T> ws, uint32_t base,
                                                             uint32_t cap, int count_ctr) {
  const uint32_t count = min(ws.ctr[count_ctr], cap);
  const uint32_t stride = gridDim.x * kAuxBlock;
  for (uint32_t i = blockIdx.x * kAuxBlock + threadIdx.x; i < count; i += stride) {
    const uint32_t c = base + i;
    bool ab;
    int v;
    if (ws.expanded[c]) {
      ab = ws.abort[c] != 0;
      v = (int)(ws.key[c] >> 8) - T::kBias;
    } else {
      v = ws.value[c];
      ab = v == T::kAborted;
    }
    const int32_t par = ws.parent[c];
    if (ab)
      atomicOr(&ws.abort[par], 1u);
    else
      atomicMax(&ws.key[par], ((uint32_t)(T::kBias - v) << 8) | (255u - ws.action[c]));
    atomicAdd(reinterpret_cast<unsigned long long*>(&ws.nodes[par]),
              (unsigned long long)ws.nodes[c]);
  }
}

template <class T>
__global__ __launch_bounds__(kAuxBlock) void k_split_finish(SplitWs<T> ws, uint32_t count,
                                                            typename T::Value* __restrict__ value_o,
                                                            uint8_t* __restrict__ best_o,
                                                            uint64_t* __restrict__ nodes_o) {
  const uint32_t stride = gridDim.x * kAuxBlock;
  for (uint32_t i = blockIdx.x * kAuxBlock + threadIdx.x; i < count; i += stride) {
    int v = ws.value[i];
    int b = ws.best[i];
    if (ws.expanded[i]) {
      const uint32_t key = ws.key[i];
      const bool ab = ws.abort[i] != 0;
      v = ab ? T::kAborted : (int)(key >> 8) - T::kBias;
      b = ab ? 255 : 255 - (int)(key & 0xFF);
    }
    value_o[i] = (typename T::Value)v;
    best_o[i] = (uint8_t)b;
    if (nodes_o) nodes_o[i] = ws.nodes[i];
  }
}

// Workspace layout for `cap` nodes, every array padded to 256 bytes on its own (the total does
// not depend on their order); returns the bytes used.
template <class T>
size_t carve(char* base, size_t cap, SplitWs<T>* ws) {
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* q = base ? base + off : nullptr;
    off += azl::align_up(bytes);
    return q;
  };
  SplitWs<T> w{};
  w.ctr = reinterpret_cast<uint32_t*>(take(kCtrWords * 4));
  w.own = reinterpret_cast<uint64_t*>(take(cap * 8));
  w.opp = reinterpret_cast<uint64_t*>(take(cap * 8));
  w.nodes = reinterpret_cast<uint64_t*>(take(cap * 8));
  w.parent = reinterpret_cast<int32_t*>(take(cap * 4));
  w.task = reinterpret_cast<int32_t*>(take(cap * 4));
  w.key = reinterpret_cast<uint32_t*>(take(cap * 4));
  w.abort = reinterpret_cast<uint32_t*>(take(cap * 4));
  w.value = reinterpret_cast<typename T::Value*>(take(cap * sizeof(typename T::Value)));
  w.action = reinterpret_cast<uint8_t*>(take(cap));
  w.best = reinterpret_cast<uint8_t*>(take(cap));
  w.expanded = reinterpret_cast<uint8_t*>(take(cap));
  for (int k = 0; k < T::kExtras; ++k) w.extra[k] = reinterpret_cast<uint8_t*>(take(cap));
  if (ws) *ws = w;
  return off;
}

struct Plan {
  int64_t chunk;      // roots per chunk
  size_t cap1, cap2;  // node capacity of levels 1 and 2
  size_t cap;         // all levels
};

template <class T>
Plan plan_for(int64_t n, int split, const typename T::Params& par) {
  Plan pl{};
  if (split == 0) return pl;
  const int64_t lim = split == 1 ? T::kChunk1 : T::kChunk2;
  pl.chunk = n < lim ? n : lim;
  pl.cap1 = (size_t)pl.chunk * T::children1(par);
  pl.cap2 = split == 2 ? pl.cap1 * T::children2(par) : 0;
  pl.cap = (size_t)pl.chunk + pl.cap1 + pl.cap2;
  return pl;
}

// bytes of workspace a call needs: the counters alone when the roots are the tasks
template <class T>
size_t workspace_need(int64_t n, int split, const typename T::Params& par) {
  return split == 0 ? azl::align_up(kCtrWords * 4)
                    : carve<T>(nullptr, plan_for<T>(n, split, par).cap, nullptr);
}

inline unsigned aux_grid(size_t n) {
  const size_t b = (n + kAuxBlock - 1) / kAuxBlock;
  return (unsigned)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

// The whole call on stream s, after its arguments were checked: launch(tasks) starts the
// search's lane kernel over a task list and returns AZ_OK or an error code.
template <class T, class Launch>
int run(const uint64_t* own, const uint64_t* opp, int64_t n, int split,
        const typename T::Params& par, typename T::Value* value_o, uint8_t* best_o,
        uint64_t* nodes_o, void* workspace, hipStream_t s, Launch launch) {
  if (split == 0) {
    uint32_t* ctr = static_cast<uint32_t*>(workspace);
    AZ_HIP(hipMemsetAsync(ctr, 0, kCtrWords * 4, s));
    return launch(TaskList<T>{own, opp, nullptr, {nullptr, nullptr}, nullptr, (uint32_t)n,
                              ctr + kCtrQueue, value_o, best_o, nodes_o});
  }
  const Plan pl = plan_for<T>(n, split, par);
  SplitWs<T> ws;
  carve<T>(static_cast<char*>(workspace), pl.cap, &ws);
  const uint32_t b1 = (uint32_t)pl.chunk, b2 = (uint32_t)(pl.chunk + pl.cap1);
  const uint32_t cap1 = (uint32_t)pl.cap1, cap2 = (uint32_t)pl.cap2;
  const uint64_t* none = nullptr;
  for (int64_t off = 0; off < n; off += pl.chunk) {
    const uint32_t r = (uint32_t)(n - off < pl.chunk ? n - off : pl.chunk);
    AZ_HIP(hipMemsetAsync(ws.ctr, 0, kCtrWords * 4, s));
    hipLaunchKernelGGL(k_split_expand<T>, dim3(aux_grid(r)), dim3(kAuxBlock), 0, s, ws, own + off,
                       opp + off, 0u, r, -1, b1, cap1, (int)kCtrL1, split == 1 ? 1 : 0, par);
    if (split == 2)
      hipLaunchKernelGGL(k_split_expand<T>, dim3(aux_grid(cap1)), dim3(kAuxBlock), 0, s, ws, none,
                         none, b1, cap1, (int)kCtrL1, b2, cap2, (int)kCtrL2, 1, par);
    AZ_HIP(hipGetLastError());
    const int rc = launch(TaskList<T>{ws.own, ws.opp, ws.task, {ws.extra[0], ws.extra[1]},
                                      ws.ctr + kCtrTasks, 0u, ws.ctr + kCtrQueue, ws.value,
                                      ws.best, ws.nodes});
    if (rc != AZ_OK) return rc;
    if (split == 2)
      hipLaunchKernelGGL(k_split_combine<T>, dim3(aux_grid(cap2)), dim3(kAuxBlock), 0, s, ws, b2,
                         cap2, (int)kCtrL2);
    hipLaunchKernelGGL(k_split_combine<T>, dim3(aux_grid(cap1)), dim3(kAuxBlock), 0, s, ws, b1,
                       cap1, (int)kCtrL1);
    hipLaunchKernelGGL(k_split_finish<T>, dim3(aux_grid(r)), dim3(kAuxBlock), 0, s, ws, r,
                       value_o + off, best_o + off, nodes_o ? nodes_o + off : nullptr);
    AZ_HIP(hipGetLastError());
  }
  return AZ_OK;
}

}  // namespace azf
