// search.hip — depth-limited alpha-beta entry points (oth_eval_* / oth_search_*).
//
// The search itself is search.h's step(), the same code on both sides.  The device side
// follows solve.hip: one lane runs one search at a time (k_search), a lane whose search
// ended takes the next task index from a global counter, and the kernel loop is "every lane
// with work advances one node".  The frames below each lane's top frame live in LDS, laid
// out [frame][field][lane]: the 64 lanes of a wave touch 64 consecutive 8-byte words,
// conflict-free, and nothing is a runtime-indexed private array.
//
// Every loop is bounded: a search ends after node_limit nodes at the latest, the lane loop
// ends when the task counter passes the task count, and no lane waits for another.
//
// Split front end (split_plies = 1 or 2, depth > split_plies): every non-terminal root is
// expanded level by level into its children (k_split_expand; child slots by atomicAdd), a
// placement child has one ply less than its parent and a pass child keeps its depth, every
// leaf of that small tree is a full-window task of the same k_search queue, and the levels
// are combined bottom-up (k_split_combine) by atomicMax on the key
// (value + 32768) << 8 | (255 - action): independent of the order of arrival, and the lowest
// action among the best.  Roots go through the workspace in chunks.
#include <stdexcept>

#include "bitboard.h"
#include "common.h"
#include "search.h"

static_assert(AZ_SEARCH_SKIPPED == azq::kSkipped && AZ_SEARCH_ABORTED == azq::kAborted &&
                  AZ_SEARCH_MAX_DEPTH == azq::kMaxDepth,
              "include/az_othello.h and csrc/search.h disagree");

namespace {

constexpr int kSearchBlock = 128;  // two waves, as k_solve
constexpr int kLdsBytes = 160 * 1024;
constexpr int kAuxBlock = 256;

// no reachable position has more than 33 placements; a node with more (an arbitrary board)
// that would overrun its level is not written and its root is reported aborted
constexpr int kMaxChildren = 33;
// roots per chunk of the split front end: bounds the workspace while one chunk still fills
// the chip with tasks
constexpr int kChunk1 = 16384, kChunk2 = 1024;

struct LdsStack {
  uint64_t* w;  // [frame][3][kSearchBlock], this lane's column
  __device__ __forceinline__ void put(int f, uint64_t flips, uint64_t moves, uint64_t pk) {
    w[(3 * f) * kSearchBlock] = flips;
    w[(3 * f + 1) * kSearchBlock] = moves;
    w[(3 * f + 2) * kSearchBlock] = pk;
  }
  __device__ __forceinline__ void get(int f, uint64_t& flips, uint64_t& moves,
                                      uint64_t& pk) const {
    flips = w[(3 * f) * kSearchBlock];
    moves = w[(3 * f + 1) * kSearchBlock];
    pk = w[(3 * f + 2) * kSearchBlock];
  }
};

constexpr int frame_bytes(int nf) { return nf * kSearchBlock * 24; }

// NF = frames of LDS stack per lane (depth - 1 at most are ever used).  Task t is position
// task_ids[t] (or t itself) of own / opp, searched to depth_of[node] (or depth) plies;
// results go to the same index.
template <int NF>
__global__ __launch_bounds__(kSearchBlock) void k_search(
    const uint64_t* __restrict__ own, const uint64_t* __restrict__ opp,
    const int32_t* __restrict__ task_ids, const uint8_t* __restrict__ depth_of,
    const uint32_t* __restrict__ n_ptr, uint32_t n_host, int depth, uint64_t node_limit,
    uint32_t* __restrict__ queue, int16_t* __restrict__ value_o, uint8_t* __restrict__ best_o,
    uint64_t* __restrict__ nodes_o) {
  __shared__ uint64_t w[NF * 3 * kSearchBlock];
  LdsStack st{w + threadIdx.x};
  const uint32_t n = n_ptr ? *n_ptr : n_host;
  azq::Search s;
  s.state = azq::kDone;
  uint32_t node = 0;
  for (;;) {
    if (s.state != azq::kRun) {  // no work: take the next task, or leave
      const uint32_t t = atomicAdd(queue, 1u);
      if (t >= n) break;
      node = task_ids ? (uint32_t)task_ids[t] : t;
      azq::init(s, own[node], opp[node], depth_of ? (int)depth_of[node] : depth);
    } else {
      azq::step(s, st, node_limit, NF);
    }
    if (s.state != azq::kRun) {
      value_o[node] = (int16_t)s.value;
      best_o[node] = (uint8_t)s.root_best;
      if (nodes_o) nodes_o[node] = s.nodes;
    }
  }
}

__global__ __launch_bounds__(kAuxBlock) void k_eval(const uint64_t* __restrict__ own,
                                                    const uint64_t* __restrict__ opp, int64_t n,
                                                    int16_t* __restrict__ value_o) {
  const int64_t stride = (int64_t)gridDim.x * kAuxBlock;
  for (int64_t i = (int64_t)blockIdx.x * kAuxBlock + threadIdx.x; i < n; i += stride)
    value_o[i] = (int16_t)azq::evaluate(own[i], opp[i]);
}

// ---- split front end -------------------------------------------------------------------

// counters of one chunk
enum { kCtrQueue = 0, kCtrTasks = 1, kCtrL1 = 2, kCtrL2 = 3, kCtrWords = 4 };

struct SplitWs {
  uint64_t *own, *opp, *nodes;
  int32_t *parent, *task;
  uint32_t *key, *abort, *ctr;
  int16_t* value;
  uint8_t *action, *best, *expanded, *depth;
};

// One level of the expansion: node i of the level (count from the host, or from the
// counter count_ctr) either becomes a task or gets its children in the next level.  Level
// 0 (src_own given) copies the roots in; every node that is neither terminal nor overlapping
// is expanded.
__global__ __launch_bounds__(kAuxBlock) void k_split_expand(
    SplitWs ws, const uint64_t* __restrict__ src_own, const uint64_t* __restrict__ src_opp,
    uint32_t base, uint32_t count_host, int count_ctr, uint32_t next_base, uint32_t next_cap,
    int next_ctr, int child_tasks, int root_depth) {
  const uint32_t count = count_ctr >= 0 ? min(ws.ctr[count_ctr], count_host) : count_host;
  const uint32_t stride = gridDim.x * kAuxBlock;
  for (uint32_t i = blockIdx.x * kAuxBlock + threadIdx.x; i < count; i += stride) {
    const uint32_t node = base + i;
    uint64_t o, p;
    bool expand = true;
    if (src_own) {
      o = src_own[i];
      p = src_opp[i];
      ws.own[node] = o;
      ws.opp[node] = p;
      ws.parent[node] = -1;
      ws.action[node] = azb::kPass;
      ws.depth[node] = (uint8_t)root_depth;
      expand = (o & p) == 0;
    } else {
      o = ws.own[node];
      p = ws.opp[node];
    }
    const int d = ws.depth[node];
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
    uint32_t k = 0, slot = 0;
    if (expand) {
      k = pass ? 1u : (uint32_t)azb::popc(m);
      slot = atomicAdd(&ws.ctr[next_ctr], k);
      if (slot + k > next_cap) {
        // more children than any reachable position has: the node is aborted and writes no
        // child; the one node that crosses the end fills the slots it was given below it
        // with inert nodes (an empty board: a terminal task), so the level holds no slot
        // that was never written
        ws.abort[node] = 1;
        for (uint32_t c = next_base + min(slot, next_cap); c < next_base + next_cap; ++c) {
          ws.own[c] = 0;
          ws.opp[c] = 0;
          ws.parent[c] = (int32_t)node;
          ws.action[c] = azb::kPass;
          ws.expanded[c] = 0;
          ws.depth[c] = 1;
          ws.nodes[c] = 0;
          ws.value[c] = (int16_t)azq::kAborted;
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
      ws.depth[c] = (uint8_t)(pass ? d : d - 1);
      if (child_tasks) ws.task[tb + j] = (int32_t)c;
    }
  }
}

// One level of the combine: every node of the level hands its value (a task's value, or
// the key its own children left) to its parent.  Every child has the other side to move,
// so the parent's value of the move is the negated child value.
__global__ __launch_bounds__(kAuxBlock) void k_split_combine(SplitWs ws, uint32_t base,
                                                             uint32_t cap, int count_ctr) {
  const uint32_t count = min(ws.ctr[count_ctr], cap);
  const uint32_t stride = gridDim.x * kAuxBlock;
  for (uint32_t i = blockIdx.x * kAuxBlock + threadIdx.x; i < count; i += stride) {
    const uint32_t c = base + i;
    bool ab;
    int v;
    if (ws.expanded[c]) {
      ab = ws.abort[c] != 0;
      v = (int)(ws.key[c] >> 8) - 32768;
    } else {
      v = ws.value[c];
      ab = v == azq::kAborted;
    }
    const int32_t par = ws.parent[c];
    if (ab)
      atomicOr(&ws.abort[par], 1u);
    else
      atomicMax(&ws.key[par], ((uint32_t)(32768 - v) << 8) | (255u - ws.action[c]));
    atomicAdd(reinterpret_cast<unsigned long long*>(&ws.nodes[par]),
              (unsigned long long)ws.nodes[c]);
  }
}

__global__ __launch_bounds__(kAuxBlock) void k_split_finish(SplitWs ws, uint32_t count,
                                                            int16_t* __restrict__ value_o,
                                                            uint8_t* __restrict__ best_o,
                                                            uint64_t* __restrict__ nodes_o) {
  const uint32_t stride = gridDim.x * kAuxBlock;
  for (uint32_t i = blockIdx.x * kAuxBlock + threadIdx.x; i < count; i += stride) {
    int v = ws.value[i];
    int b = ws.best[i];
    if (ws.expanded[i]) {
      const uint32_t key = ws.key[i];
      const bool ab = ws.abort[i] != 0;
      v = ab ? azq::kAborted : (int)(key >> 8) - 32768;
      b = ab ? 255 : 255 - (int)(key & 0xFF);
    }
    value_o[i] = (int16_t)v;
    best_o[i] = (uint8_t)b;
    if (nodes_o) nodes_o[i] = ws.nodes[i];
  }
}

size_t align_up(size_t x) { return (x + 255) & ~size_t(255); }

// workspace layout for `cap` nodes; returns the bytes used
size_t carve(char* base, size_t cap, SplitWs* ws) {
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* q = base ? base + off : nullptr;
    off += align_up(bytes);
    return q;
  };
  SplitWs w;
  w.ctr = reinterpret_cast<uint32_t*>(take(kCtrWords * 4));
  w.own = reinterpret_cast<uint64_t*>(take(cap * 8));
  w.opp = reinterpret_cast<uint64_t*>(take(cap * 8));
  w.nodes = reinterpret_cast<uint64_t*>(take(cap * 8));
  w.parent = reinterpret_cast<int32_t*>(take(cap * 4));
  w.task = reinterpret_cast<int32_t*>(take(cap * 4));
  w.key = reinterpret_cast<uint32_t*>(take(cap * 4));
  w.abort = reinterpret_cast<uint32_t*>(take(cap * 4));
  w.value = reinterpret_cast<int16_t*>(take(cap * 2));
  w.action = reinterpret_cast<uint8_t*>(take(cap));
  w.best = reinterpret_cast<uint8_t*>(take(cap));
  w.expanded = reinterpret_cast<uint8_t*>(take(cap));
  w.depth = reinterpret_cast<uint8_t*>(take(cap));
  if (ws) *ws = w;
  return off;
}

struct Plan {
  int64_t chunk;      // roots per chunk
  size_t cap1, cap2;  // node capacity of levels 1 and 2
  size_t cap;         // all levels
};

Plan plan_for(int64_t n, int split) {
  Plan pl{};
  if (split == 0) return pl;
  const int64_t lim = split == 1 ? kChunk1 : kChunk2;
  pl.chunk = n < lim ? n : lim;
  pl.cap1 = (size_t)pl.chunk * kMaxChildren;
  pl.cap2 = split == 2 ? pl.cap1 * kMaxChildren : 0;
  pl.cap = (size_t)pl.chunk + pl.cap1 + pl.cap2;
  return pl;
}

unsigned aux_grid(size_t n) {
  const size_t b = (n + kAuxBlock - 1) / kAuxBlock;
  return (unsigned)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

// max_depth = the deepest task of the launch (sizes the LDS stack)
int launch_search(const uint64_t* own, const uint64_t* opp, const int32_t* task_ids,
                  const uint8_t* depth_of, const uint32_t* n_ptr, uint32_t n_host, int max_depth,
                  uint64_t node_limit, uint32_t* queue, int16_t* value_o, uint8_t* best_o,
                  uint64_t* nodes_o, hipStream_t stream) {
  int dev = 0, cus = 0;
  AZ_HIP(hipGetDevice(&dev));
  AZ_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  const int nf = max_depth <= 4 ? 3 : (max_depth <= 7 ? 6 : 9);
  const int per_cu = std::min(16, kLdsBytes / frame_bytes(nf));
  unsigned grid = (unsigned)(cus > 0 ? cus : 1) * (unsigned)per_cu;
  if (!n_ptr) {  // task count known here: no more lanes than tasks
    const unsigned need = (n_host + kSearchBlock - 1) / kSearchBlock;
    grid = need < grid ? (need < 1 ? 1 : need) : grid;
  }
#define AZ_SEARCH_LAUNCH(NF)                                                                  \
  hipLaunchKernelGGL(k_search<NF>, dim3(grid), dim3(kSearchBlock), 0, stream, own, opp,       \
                     task_ids, depth_of, n_ptr, n_host, max_depth, node_limit, queue, value_o, \
                     best_o, nodes_o)
  if (nf == 3)
    AZ_SEARCH_LAUNCH(3);
  else if (nf == 6)
    AZ_SEARCH_LAUNCH(6);
  else
    AZ_SEARCH_LAUNCH(9);
#undef AZ_SEARCH_LAUNCH
  AZ_HIP(hipGetLastError());
  return AZ_OK;
}

}  // namespace

extern "C" {

int oth_eval_cpu(const uint64_t* own, const uint64_t* opp, int64_t n, int16_t* value_o) {
  AZ_REQUIRE(n >= 0, AZ_ERR_ARG, "oth_eval_cpu: n=%lld < 0", (long long)n);
  AZ_REQUIRE(n == 0 || (own && opp && value_o), AZ_ERR_ARG, "oth_eval_cpu: null buffer");
  for (int64_t i = 0; i < n; ++i) value_o[i] = (int16_t)azq::evaluate(own[i], opp[i]);
  return AZ_OK;
}

int oth_eval_gpu(const uint64_t* own, const uint64_t* opp, int64_t n, int16_t* value_o,
                 void* stream) {
  AZ_REQUIRE(n >= 0, AZ_ERR_ARG, "oth_eval_gpu: n=%lld < 0", (long long)n);
  if (n == 0) return AZ_OK;
  AZ_REQUIRE(own && opp && value_o, AZ_ERR_ARG, "oth_eval_gpu: null buffer");
  hipLaunchKernelGGL(k_eval, dim3(aux_grid((size_t)n)), dim3(kAuxBlock), 0,
                     azc::as_stream(stream), own, opp, n, value_o);
  AZ_HIP(hipGetLastError());
  return AZ_OK;
}

int oth_search_cpu(const uint64_t* own, const uint64_t* opp, int64_t n, int32_t depth,
                   uint64_t node_limit, int16_t* value_o, uint8_t* best_o, uint64_t* nodes_o) {
  AZ_REQUIRE(n >= 0, AZ_ERR_ARG, "oth_search_cpu: n=%lld < 0", (long long)n);
  AZ_REQUIRE(depth >= 1 && depth <= AZ_SEARCH_MAX_DEPTH, AZ_ERR_ARG,
             "oth_search_cpu: depth=%d outside 1..%d", (int)depth, AZ_SEARCH_MAX_DEPTH);
  AZ_REQUIRE(n == 0 || (own && opp && value_o && best_o), AZ_ERR_ARG,
             "oth_search_cpu: null buffer");
  for (int64_t i = 0; i < n; ++i)
    azq::search_one(own[i], opp[i], depth, node_limit, value_o + i, best_o + i,
                    nodes_o ? nodes_o + i : nullptr);
  return AZ_OK;
}

int oth_search_gpu(const uint64_t* own, const uint64_t* opp, int64_t n, int32_t depth,
                   uint64_t node_limit, int32_t split_plies, int16_t* value_o, uint8_t* best_o,
                   uint64_t* nodes_o, void* workspace, size_t* workspace_bytes, void* stream) {
  AZ_REQUIRE(n >= 0 && n < (int64_t(1) << 31), AZ_ERR_ARG,
             "oth_search_gpu: n=%lld outside 0..2^31", (long long)n);
  AZ_REQUIRE(depth >= 1 && depth <= AZ_SEARCH_MAX_DEPTH, AZ_ERR_ARG,
             "oth_search_gpu: depth=%d outside 1..%d", (int)depth, AZ_SEARCH_MAX_DEPTH);
  AZ_REQUIRE(split_plies >= 0 && split_plies <= 2, AZ_ERR_ARG,
             "oth_search_gpu: split_plies=%d outside 0..2", (int)split_plies);
  AZ_REQUIRE(workspace_bytes, AZ_ERR_ARG, "oth_search_gpu: null workspace_bytes");
  if (depth <= split_plies) split_plies = 0;  // nothing left below the split: one search
  const Plan pl = plan_for(n, split_plies);
  const size_t need = split_plies == 0 ? align_up(kCtrWords * 4) : carve(nullptr, pl.cap, nullptr);
  if (!workspace) {
    *workspace_bytes = need;
    return AZ_OK;
  }
  AZ_REQUIRE(*workspace_bytes >= need, AZ_ERR_ARG, "oth_search_gpu: workspace %zu < %zu bytes",
             *workspace_bytes, need);
  AZ_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0, AZ_ERR_ARG,
             "oth_search_gpu: workspace must be 8-byte aligned");
  if (n == 0) return AZ_OK;
  AZ_REQUIRE(own && opp && value_o && best_o, AZ_ERR_ARG, "oth_search_gpu: null buffer");
  hipStream_t s = azc::as_stream(stream);
  if (split_plies == 0) {
    uint32_t* ctr = static_cast<uint32_t*>(workspace);
    AZ_HIP(hipMemsetAsync(ctr, 0, kCtrWords * 4, s));
    return launch_search(own, opp, nullptr, nullptr, nullptr, (uint32_t)n, depth, node_limit,
                         ctr + kCtrQueue, value_o, best_o, nodes_o, s);
  }
  SplitWs ws;
  carve(static_cast<char*>(workspace), pl.cap, &ws);
  const uint32_t b1 = (uint32_t)pl.chunk, b2 = (uint32_t)(pl.chunk + pl.cap1);
  for (int64_t off = 0; off < n; off += pl.chunk) {
    const uint32_t r = (uint32_t)(n - off < pl.chunk ? n - off : pl.chunk);
    AZ_HIP(hipMemsetAsync(ws.ctr, 0, kCtrWords * 4, s));
    hipLaunchKernelGGL(k_split_expand, dim3(aux_grid(r)), dim3(kAuxBlock), 0, s, ws, own + off,
                       opp + off, 0u, r, -1, b1, (uint32_t)pl.cap1, (int)kCtrL1,
                       split_plies == 1 ? 1 : 0, (int)depth);
    if (split_plies == 2)
      hipLaunchKernelGGL(k_split_expand, dim3(aux_grid(pl.cap1)), dim3(kAuxBlock), 0, s, ws,
                         (const uint64_t*)nullptr, (const uint64_t*)nullptr, b1,
                         (uint32_t)pl.cap1, (int)kCtrL1, b2, (uint32_t)pl.cap2, (int)kCtrL2, 1,
                         (int)depth);
    AZ_HIP(hipGetLastError());
    // a task is a root (terminal or overlapping: finished by init) or a node at least one
    // ply down, a pass child keeping its parent's depth
    const int rc = launch_search(ws.own, ws.opp, ws.task, ws.depth, ws.ctr + kCtrTasks, 0u, depth,
                                 node_limit, ws.ctr + kCtrQueue, ws.value, ws.best, ws.nodes, s);
    if (rc != AZ_OK) return rc;
    if (split_plies == 2)
      hipLaunchKernelGGL(k_split_combine, dim3(aux_grid(pl.cap2)), dim3(kAuxBlock), 0, s, ws, b2,
                         (uint32_t)pl.cap2, (int)kCtrL2);
    hipLaunchKernelGGL(k_split_combine, dim3(aux_grid(pl.cap1)), dim3(kAuxBlock), 0, s, ws, b1,
                       (uint32_t)pl.cap1, (int)kCtrL1);
    hipLaunchKernelGGL(k_split_finish, dim3(aux_grid(r)), dim3(kAuxBlock), 0, s, ws, r,
                       value_o + off, best_o + off, nodes_o ? nodes_o + off : nullptr);
    AZ_HIP(hipGetLastError());
  }
  return AZ_OK;
}

}  // extern "C"
