// solve.hip — exact endgame solver entry points (oth_solve_cpu / oth_solve_gpu).
//
// The search itself is solve.h's step(), the same code on both sides.  On the device one
// lane runs one search at a time (k_solve): a lane whose search ended takes the next task
// index from a global counter, and the kernel loop is "every lane with work advances one
// node", so a wave diverges inside one node step at most, never across whole searches.
// The frames below each lane's top frame live in LDS, laid out [frame][field][lane]: the
// 64 lanes of a wave touch 64 consecutive 8-byte (capture set, untried moves) or 4-byte
// (packed window) words, conflict-free, and nothing is a runtime-indexed private array.
//
// Every loop is bounded: a search ends after node_limit nodes at the latest, the lane loop
// ends when the task counter passes the task count, and no lane waits for another.
//
// Split front end (split_plies = 1 or 2): roots with at least AZ_SOLVE_SPLIT_MIN empties are
// expanded level by level into their children (k_split_expand; child slots by atomicAdd),
// every leaf of that small tree is a full-window task of the same k_solve queue, and the
// levels are combined bottom-up (k_split_combine) by atomicMax on the key
// (value + 64) * 256 + (255 - action): independent of the order of arrival, and the lowest
// action among the best.  Roots go through the workspace in chunks.
#include <stdexcept>

#include "bitboard.h"
#include "common.h"
#include "solve.h"

static_assert(AZ_SOLVE_SKIPPED == azs::kSkipped && AZ_SOLVE_ABORTED == azs::kAborted &&
                  AZ_SOLVE_MAX_EMPTIES == azs::kMaxEmpties,
              "include/az_othello.h and csrc/solve.h disagree");

namespace {

constexpr int kSolveBlock = 128;  // two waves: the LDS granule that fits 4 / 5 / 9 per CU
constexpr int kLdsBytes = 160 * 1024;
constexpr int kAuxBlock = 256;

// roots per chunk of the split front end: bounds the workspace (a root has at most 14
// children and 14 * 13 grandchildren) while one chunk still fills the chip with tasks
constexpr int kChunk1 = 16384, kChunk2 = 2048;

struct LdsStack {
  uint64_t* w;  // [frame][2][kSolveBlock], this lane's column
  uint32_t* p;  // [frame][kSolveBlock]
  __device__ __forceinline__ void put(int f, uint64_t flips, uint64_t moves, uint32_t pk) {
    w[(2 * f) * kSolveBlock] = flips;
    w[(2 * f + 1) * kSolveBlock] = moves;
    p[f * kSolveBlock] = pk;
  }
  __device__ __forceinline__ void get(int f, uint64_t& flips, uint64_t& moves,
                                      uint32_t& pk) const {
    flips = w[(2 * f) * kSolveBlock];
    moves = w[(2 * f + 1) * kSolveBlock];
    pk = p[f * kSolveBlock];
  }
};

constexpr int frame_bytes(int nf) { return nf * kSolveBlock * 20; }

// NF = frames of LDS stack per lane (max_empties - 1 at most are ever used).  Task t is
// position task_ids[t] (or t itself) of own / opp; results go to the same index.
template <int NF>
__global__ __launch_bounds__(kSolveBlock) void k_solve(
    const uint64_t* __restrict__ own, const uint64_t* __restrict__ opp,
    const int32_t* __restrict__ task_ids, const uint32_t* __restrict__ n_ptr, uint32_t n_host,
    int max_empties, uint64_t node_limit, uint32_t* __restrict__ queue,
    int8_t* __restrict__ score_o, uint8_t* __restrict__ best_o, uint64_t* __restrict__ nodes_o) {
  __shared__ uint64_t w[NF * 2 * kSolveBlock];
  __shared__ uint32_t p[NF * kSolveBlock];
  LdsStack st{w + threadIdx.x, p + threadIdx.x};
  const uint32_t n = n_ptr ? *n_ptr : n_host;
  azs::Search s;
  s.state = azs::kDone;
  uint32_t node = 0;
  for (;;) {
    if (s.state != azs::kRun) {  // no work: take the next task, or leave
      const uint32_t t = atomicAdd(queue, 1u);
      if (t >= n) break;
      node = task_ids ? (uint32_t)task_ids[t] : t;
      azs::init(s, own[node], opp[node], max_empties);
    } else {
      azs::step(s, st, node_limit, NF);
    }
    if (s.state != azs::kRun) {
      score_o[node] = (int8_t)s.score;
      best_o[node] = (uint8_t)s.root_best;
      if (nodes_o) nodes_o[node] = s.nodes;
    }
  }
}

// ---- split front end -------------------------------------------------------------------

// counters of one chunk
enum { kCtrQueue = 0, kCtrTasks = 1, kCtrL1 = 2, kCtrL2 = 3, kCtrWords = 4 };

struct SplitWs {
  uint64_t *own, *opp, *nodes;
  int32_t *parent, *task;
  uint32_t *key, *abort, *ctr;
  uint8_t *action, *best, *expanded;
  int8_t* score;
};

// One level of the expansion: node i of the level (count from the host, or from the
// counter count_ctr) either becomes a task or gets its children in the next level.  Level
// 0 (src_own given) copies the roots in and expands only searchable roots with at least
// split_min empties; deeper levels expand every non-terminal node.
__global__ __launch_bounds__(kAuxBlock) void k_split_expand(
    SplitWs ws, const uint64_t* __restrict__ src_own, const uint64_t* __restrict__ src_opp,
    uint32_t base, uint32_t count_host, int count_ctr, uint32_t next_base, uint32_t next_cap,
    int next_ctr, int child_tasks, int max_empties, int split_min) {
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
      const int e = 64 - azb::popc(o | p);
      expand = (o & p) == 0 && e >= split_min && e <= max_empties;
    } else {
      o = ws.own[node];
      p = ws.opp[node];
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
    uint32_t k = 0, slot = 0;
    if (expand) {
      k = pass ? 1u : (uint32_t)azb::popc(m);
      slot = atomicAdd(&ws.ctr[next_ctr], k);
      if (slot + k > next_cap) {  // cannot happen (the caps are the worst case): no write
        ws.abort[node] = 1;
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
      if (child_tasks) ws.task[tb + j] = (int32_t)c;
    }
  }
}

// One level of the combine: every node of the level hands its value (a task's score, or
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
      v = (int)(ws.key[c] >> 8) - 64;
    } else {
      v = ws.score[c];
      ab = v == azs::kAborted;
    }
    const int32_t par = ws.parent[c];
    if (ab)
      atomicOr(&ws.abort[par], 1u);
    else
      atomicMax(&ws.key[par], ((uint32_t)(64 - v) << 8) | (255u - ws.action[c]));
    atomicAdd(reinterpret_cast<unsigned long long*>(&ws.nodes[par]),
              (unsigned long long)ws.nodes[c]);
  }
}

__global__ __launch_bounds__(kAuxBlock) void k_split_finish(SplitWs ws, uint32_t count,
                                                            int8_t* __restrict__ score_o,
                                                            uint8_t* __restrict__ best_o,
                                                            uint64_t* __restrict__ nodes_o) {
  const uint32_t stride = gridDim.x * kAuxBlock;
  for (uint32_t i = blockIdx.x * kAuxBlock + threadIdx.x; i < count; i += stride) {
    int sc = ws.score[i];
    int b = ws.best[i];
    if (ws.expanded[i]) {
      const uint32_t key = ws.key[i];
      const bool ab = ws.abort[i] != 0;
      sc = ab ? azs::kAborted : (int)(key >> 8) - 64;
      b = ab ? 255 : 255 - (int)(key & 0xFF);
    }
    score_o[i] = (int8_t)sc;
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
  w.action = reinterpret_cast<uint8_t*>(take(cap));
  w.best = reinterpret_cast<uint8_t*>(take(cap));
  w.expanded = reinterpret_cast<uint8_t*>(take(cap));
  w.score = reinterpret_cast<int8_t*>(take(cap));
  if (ws) *ws = w;
  return off;
}

struct Plan {
  int64_t chunk;        // roots per chunk
  size_t cap1, cap2;    // node capacity of levels 1 and 2
  size_t cap;           // all levels
};

Plan plan_for(int64_t n, int max_empties, int split) {
  Plan pl{};
  const size_t m = (size_t)(max_empties < 1 ? 1 : max_empties);
  if (split == 0) return pl;
  const int64_t lim = split == 1 ? kChunk1 : kChunk2;
  pl.chunk = n < lim ? n : lim;
  pl.cap1 = (size_t)pl.chunk * m;
  pl.cap2 = split == 2 ? pl.cap1 * (m > 1 ? m - 1 : 1) : 0;
  pl.cap = (size_t)pl.chunk + pl.cap1 + pl.cap2;
  return pl;
}

unsigned aux_grid(size_t n) {
  const size_t b = (n + kAuxBlock - 1) / kAuxBlock;
  return (unsigned)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

int launch_solve(const uint64_t* own, const uint64_t* opp, const int32_t* task_ids,
                 const uint32_t* n_ptr, uint32_t n_host, int max_empties, uint64_t node_limit,
                 uint32_t* queue, int8_t* score_o, uint8_t* best_o, uint64_t* nodes_o,
                 hipStream_t stream) {
  int dev = 0, cus = 0;
  AZ_HIP(hipGetDevice(&dev));
  AZ_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  const int nf = max_empties <= 8 ? 7 : (max_empties <= 12 ? 11 : 13);
  const int per_cu = std::min(16, kLdsBytes / frame_bytes(nf));
  unsigned grid = (unsigned)(cus > 0 ? cus : 1) * (unsigned)per_cu;
  if (!n_ptr) {  // task count known here: no more lanes than tasks
    const unsigned need = (n_host + kSolveBlock - 1) / kSolveBlock;
    grid = need < grid ? (need < 1 ? 1 : need) : grid;
  }
#define AZ_SOLVE_LAUNCH(NF)                                                                   \
  hipLaunchKernelGGL(k_solve<NF>, dim3(grid), dim3(kSolveBlock), 0, stream, own, opp,         \
                     task_ids, n_ptr, n_host, max_empties, node_limit, queue, score_o, best_o, \
                     nodes_o)
  if (nf == 7)
    AZ_SOLVE_LAUNCH(7);
  else if (nf == 11)
    AZ_SOLVE_LAUNCH(11);
  else
    AZ_SOLVE_LAUNCH(13);
#undef AZ_SOLVE_LAUNCH
  AZ_HIP(hipGetLastError());
  return AZ_OK;
}

}  // namespace

extern "C" {

int oth_solve_cpu(const uint64_t* own, const uint64_t* opp, int64_t n, int32_t max_empties,
                  uint64_t node_limit, int8_t* score_o, uint8_t* best_o, uint64_t* nodes_o) {
  AZ_REQUIRE(n >= 0, AZ_ERR_ARG, "oth_solve_cpu: n=%lld < 0", (long long)n);
  AZ_REQUIRE(max_empties >= 0 && max_empties <= AZ_SOLVE_MAX_EMPTIES, AZ_ERR_ARG,
             "oth_solve_cpu: max_empties=%d outside 0..%d", (int)max_empties,
             AZ_SOLVE_MAX_EMPTIES);
  AZ_REQUIRE(n == 0 || (own && opp && score_o && best_o), AZ_ERR_ARG,
             "oth_solve_cpu: null buffer");
  for (int64_t i = 0; i < n; ++i)
    azs::solve_one(own[i], opp[i], max_empties, node_limit, score_o + i, best_o + i,
                   nodes_o ? nodes_o + i : nullptr);
  return AZ_OK;
}

int oth_solve_gpu(const uint64_t* own, const uint64_t* opp, int64_t n, int32_t max_empties,
                  uint64_t node_limit, int32_t split_plies, int8_t* score_o, uint8_t* best_o,
                  uint64_t* nodes_o, void* workspace, size_t* workspace_bytes, void* stream) {
  AZ_REQUIRE(n >= 0 && n < (int64_t(1) << 31), AZ_ERR_ARG,
             "oth_solve_gpu: n=%lld outside 0..2^31", (long long)n);
  AZ_REQUIRE(max_empties >= 0 && max_empties <= AZ_SOLVE_MAX_EMPTIES, AZ_ERR_ARG,
             "oth_solve_gpu: max_empties=%d outside 0..%d", (int)max_empties,
             AZ_SOLVE_MAX_EMPTIES);
  AZ_REQUIRE(split_plies >= 0 && split_plies <= 2, AZ_ERR_ARG,
             "oth_solve_gpu: split_plies=%d outside 0..2", (int)split_plies);
  AZ_REQUIRE(workspace_bytes, AZ_ERR_ARG, "oth_solve_gpu: null workspace_bytes");
  const Plan pl = plan_for(n, max_empties, split_plies);
  const size_t need = split_plies == 0 ? align_up(kCtrWords * 4) : carve(nullptr, pl.cap, nullptr);
  if (!workspace) {
    *workspace_bytes = need;
    return AZ_OK;
  }
  AZ_REQUIRE(*workspace_bytes >= need, AZ_ERR_ARG, "oth_solve_gpu: workspace %zu < %zu bytes",
             *workspace_bytes, need);
  AZ_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0, AZ_ERR_ARG,
             "oth_solve_gpu: workspace must be 8-byte aligned");
  if (n == 0) return AZ_OK;
  AZ_REQUIRE(own && opp && score_o && best_o, AZ_ERR_ARG, "oth_solve_gpu: null buffer");
  hipStream_t s = azc::as_stream(stream);
  if (split_plies == 0) {
    uint32_t* ctr = static_cast<uint32_t*>(workspace);
    AZ_HIP(hipMemsetAsync(ctr, 0, kCtrWords * 4, s));
    return launch_solve(own, opp, nullptr, nullptr, (uint32_t)n, max_empties, node_limit,
                        ctr + kCtrQueue, score_o, best_o, nodes_o, s);
  }
  SplitWs ws;
  carve(static_cast<char*>(workspace), pl.cap, &ws);
  const uint32_t b1 = (uint32_t)pl.chunk, b2 = (uint32_t)(pl.chunk + pl.cap1);
  for (int64_t off = 0; off < n; off += pl.chunk) {
    const uint32_t r = (uint32_t)(n - off < pl.chunk ? n - off : pl.chunk);
    AZ_HIP(hipMemsetAsync(ws.ctr, 0, kCtrWords * 4, s));
    hipLaunchKernelGGL(k_split_expand, dim3(aux_grid(r)), dim3(kAuxBlock), 0, s, ws, own + off,
                       opp + off, 0u, r, -1, b1, (uint32_t)pl.cap1, (int)kCtrL1,
                       split_plies == 1 ? 1 : 0, (int)max_empties, (int)AZ_SOLVE_SPLIT_MIN);
    if (split_plies == 2)
      hipLaunchKernelGGL(k_split_expand, dim3(aux_grid(pl.cap1)), dim3(kAuxBlock), 0, s, ws,
                         (const uint64_t*)nullptr, (const uint64_t*)nullptr, b1,
                         (uint32_t)pl.cap1, (int)kCtrL1, b2, (uint32_t)pl.cap2, (int)kCtrL2, 1,
                         (int)max_empties, (int)AZ_SOLVE_SPLIT_MIN);
    AZ_HIP(hipGetLastError());
    const int rc = launch_solve(ws.own, ws.opp, ws.task, ws.ctr + kCtrTasks, 0u, max_empties,
                                node_limit, ws.ctr + kCtrQueue, ws.score, ws.best, ws.nodes, s);
    if (rc != AZ_OK) return rc;
    if (split_plies == 2)
      hipLaunchKernelGGL(k_split_combine, dim3(aux_grid(pl.cap2)), dim3(kAuxBlock), 0, s, ws, b2,
                         (uint32_t)pl.cap2, (int)kCtrL2);
    hipLaunchKernelGGL(k_split_combine, dim3(aux_grid(pl.cap1)), dim3(kAuxBlock), 0, s, ws, b1,
                       (uint32_t)pl.cap1, (int)kCtrL1);
    hipLaunchKernelGGL(k_split_finish, dim3(aux_grid(r)), dim3(kAuxBlock), 0, s, ws, r,
                       score_o + off, best_o + off, nodes_o ? nodes_o + off : nullptr);
    AZ_HIP(hipGetLastError());
  }
  return AZ_OK;
}

}  // extern "C"
