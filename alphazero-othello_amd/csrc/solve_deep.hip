// solve_deep.hip — windowed, move-ordered endgame solver entry points (oth_solve_deep_cpu /
// oth_solve_deep_gpu).  The search is solve_deep.h's step(), the same code on both sides.
//
// The kernel has k_solve's shape (solve.hip): one lane runs one search at a time, a lane
// whose search ended takes the next task index from a global counter, and the kernel loop is
// "every lane with work advances one step".  The frames below each lane's top frame live in
// LDS, laid out [frame][field][lane]: the 64 lanes of the wave touch 64 consecutive 8-byte
// (capture set, untried moves, order word) or 4-byte (packed window) words, conflict-free,
// and nothing is a runtime-indexed private array.  A workgroup is one wave: there is no
// barrier, and the smaller LDS granule (28 bytes * frames * 64) packs a CU better.
//
// Every loop is bounded: a search ends after node_limit nodes at the latest (at most 20
// probes precede each), the lane loop ends when the task counter passes the task count, and
// no lane waits for another.
//
// Split front end (split_plies = 1 or 2): solve.hip's, copied so that solve.hip stays as it
// is, with a window per node.  Roots with at least AZ_SOLVE_SPLIT_MIN empties are expanded
// level by level into their children; a child's window is its parent's negated and swapped
// (every child, the one after a pass included, has the other side to move), every leaf of
// that small tree is a task of the same k_solve_deep queue, and the levels are combined
// bottom-up by atomicMax on the key (value + 64) * 256 + (255 - action).  The maximum is
// sound for bounds: a child's v_c in its window (-b, -a) gives the move's value -v_c exactly
// inside (a, b), an upper bound <= a below it and a lower bound >= b above it, so the
// maximum over the moves obeys the parent's contract in (a, b), and its argmax is an optimal
// move (exact result) or a move worth >= b (fail high).  Siblings do not narrow each
// other's windows, so a split search visits more nodes than an unsplit one.
#include <stdexcept>

#include "bitboard.h"
#include "common.h"
#include "solve_deep.h"

static_assert(AZ_SOLVE_SKIPPED == azd::kSkipped && AZ_SOLVE_ABORTED == azd::kAborted &&
                  AZ_SOLVE_DEEP_MAX_EMPTIES == azd::kMaxEmpties,
              "include/az_othello.h and csrc/solve_deep.h disagree");

namespace {

constexpr int kDeepBlock = 64;  // one wave
constexpr int kLdsBytes = 160 * 1024;
constexpr int kAuxBlock = 256;
constexpr int kFrameBytes = 28;

// roots per chunk of the split front end (a root has at most max_empties children)
constexpr int kChunk1 = 16384, kChunk2 = 2048;

struct LdsStack {
  uint64_t* w;  // [frame][3][kDeepBlock], this lane's column
  uint32_t* p;  // [frame][kDeepBlock]
  __device__ __forceinline__ void put(int f, uint64_t flips, uint64_t moves, uint64_t order,
                                      uint32_t pk) {
    w[(3 * f) * kDeepBlock] = flips;
    w[(3 * f + 1) * kDeepBlock] = moves;
    w[(3 * f + 2) * kDeepBlock] = order;
    p[f * kDeepBlock] = pk;
  }
  __device__ __forceinline__ void get(int f, uint64_t& flips, uint64_t& moves, uint64_t& order,
                                      uint32_t& pk) const {
    flips = w[(3 * f) * kDeepBlock];
    moves = w[(3 * f + 1) * kDeepBlock];
    order = w[(3 * f + 2) * kDeepBlock];
    pk = p[f * kDeepBlock];
  }
};

constexpr int frame_bytes(int nf) { return nf * kDeepBlock * kFrameBytes; }

// NF = frames of LDS stack per lane (max_empties - 1 at most are ever used).  Task t is
// position task_ids[t] (or t itself) of own / opp; its window is (wa[node], wb[node]) when
// given, else (alpha, beta).  Results go to the same index.
template <int NF>
__global__ __launch_bounds__(kDeepBlock) void k_solve_deep(
    const uint64_t* __restrict__ own, const uint64_t* __restrict__ opp,
    const int32_t* __restrict__ task_ids, const uint32_t* __restrict__ n_ptr, uint32_t n_host,
    int max_empties, int alpha, int beta, const int8_t* __restrict__ wa,
    const int8_t* __restrict__ wb, uint64_t node_limit, uint32_t* __restrict__ queue,
    int8_t* __restrict__ score_o, uint8_t* __restrict__ best_o, uint64_t* __restrict__ nodes_o) {
  __shared__ uint64_t w[NF * 3 * kDeepBlock];
  __shared__ uint32_t p[NF * kDeepBlock];
  LdsStack st{w + threadIdx.x, p + threadIdx.x};
  const uint32_t n = n_ptr ? *n_ptr : n_host;
  azd::Search s;
  s.state = azd::kDone;
  uint32_t node = 0;
  for (;;) {
    if (s.state != azd::kRun) {  // no work: take the next task, or leave
      const uint32_t t = atomicAdd(queue, 1u);
      if (t >= n) break;
      node = task_ids ? (uint32_t)task_ids[t] : t;
      azd::init(s, own[node], opp[node], max_empties, wa ? (int)wa[node] : alpha,
                wb ? (int)wb[node] : beta);
    } else {
      azd::step(s, st, node_limit, NF);
    }
    if (s.state != azd::kRun) {
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
  int8_t *score, *wa, *wb;
};

// One level of the expansion: node i of the level (count from the host, or from the
// counter count_ctr) either becomes a task or gets its children in the next level.  Level
// 0 (src_own given) copies the roots in with the window (alpha, beta) and expands only
// searchable roots with at least split_min empties; deeper levels expand every non-terminal
// node.
__global__ __launch_bounds__(kAuxBlock) void k_deep_expand(
    SplitWs ws, const uint64_t* __restrict__ src_own, const uint64_t* __restrict__ src_opp,
    uint32_t base, uint32_t count_host, int count_ctr, uint32_t next_base, uint32_t next_cap,
    int next_ctr, int child_tasks, int max_empties, int split_min, int alpha, int beta) {
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
      ws.wa[node] = (int8_t)alpha;
      ws.wb[node] = (int8_t)beta;
      const int e = 64 - azb::popc(o | p);
      expand = (o & p) == 0 && e >= split_min && e <= max_empties;
    } else {
      o = ws.own[node];
      p = ws.opp[node];
    }
    const int8_t ca = (int8_t)-ws.wb[node], cb = (int8_t)-ws.wa[node];
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
      ws.wa[c] = ca;
      ws.wb[c] = cb;
      if (child_tasks) ws.task[tb + j] = (int32_t)c;
    }
  }
}

// One level of the combine: every node of the level hands its value (a task's score, or
// the key its own children left) to its parent.  Every child has the other side to move,
// so the parent's value of the move is the negated child value.
__global__ __launch_bounds__(kAuxBlock) void k_deep_combine(SplitWs ws, uint32_t base,
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
      ab = v == azd::kAborted;
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

__global__ __launch_bounds__(kAuxBlock) void k_deep_finish(SplitWs ws, uint32_t count,
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
      sc = ab ? azd::kAborted : (int)(key >> 8) - 64;
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
  w.wa = reinterpret_cast<int8_t*>(take(cap));
  w.wb = reinterpret_cast<int8_t*>(take(cap));
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

int launch_deep(const uint64_t* own, const uint64_t* opp, const int32_t* task_ids,
                const uint32_t* n_ptr, uint32_t n_host, int max_empties, int alpha, int beta,
                const int8_t* wa, const int8_t* wb, uint64_t node_limit, uint32_t* queue,
                int8_t* score_o, uint8_t* best_o, uint64_t* nodes_o, hipStream_t stream) {
  int dev = 0, cus = 0;
  AZ_HIP(hipGetDevice(&dev));
  AZ_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  const int nf = max_empties <= 12 ? 11 : (max_empties <= 16 ? 15 : 19);
  const int per_cu = std::min(16, kLdsBytes / frame_bytes(nf));
  unsigned grid = (unsigned)(cus > 0 ? cus : 1) * (unsigned)per_cu;
  if (!n_ptr) {  // task count known here: no more lanes than tasks
    const unsigned need = (n_host + kDeepBlock - 1) / kDeepBlock;
    grid = need < grid ? (need < 1 ? 1 : need) : grid;
  }
#define AZ_DEEP_LAUNCH(NF)                                                                    \
  hipLaunchKernelGGL(k_solve_deep<NF>, dim3(grid), dim3(kDeepBlock), 0, stream, own, opp,     \
                     task_ids, n_ptr, n_host, max_empties, alpha, beta, wa, wb, node_limit,   \
                     queue, score_o, best_o, nodes_o)
  if (nf == 11)
    AZ_DEEP_LAUNCH(11);
  else if (nf == 15)
    AZ_DEEP_LAUNCH(15);
  else
    AZ_DEEP_LAUNCH(19);
#undef AZ_DEEP_LAUNCH
  AZ_HIP(hipGetLastError());
  return AZ_OK;
}

bool window_ok(int alpha, int beta) {
  return alpha >= -azd::kInf && beta <= azd::kInf && alpha < beta;
}

}  // namespace

extern "C" {

int oth_solve_deep_cpu(const uint64_t* own, const uint64_t* opp, int64_t n, int32_t max_empties,
                       int32_t alpha, int32_t beta, uint64_t node_limit, int8_t* score_o,
                       uint8_t* best_o, uint64_t* nodes_o) {
  AZ_REQUIRE(n >= 0, AZ_ERR_ARG, "oth_solve_deep_cpu: n=%lld < 0", (long long)n);
  AZ_REQUIRE(max_empties >= 0 && max_empties <= AZ_SOLVE_DEEP_MAX_EMPTIES, AZ_ERR_ARG,
             "oth_solve_deep_cpu: max_empties=%d outside 0..%d", (int)max_empties,
             AZ_SOLVE_DEEP_MAX_EMPTIES);
  AZ_REQUIRE(window_ok(alpha, beta), AZ_ERR_ARG,
             "oth_solve_deep_cpu: window (%d, %d) is empty or outside -65..65", (int)alpha,
             (int)beta);
  AZ_REQUIRE(n == 0 || (own && opp && score_o && best_o), AZ_ERR_ARG,
             "oth_solve_deep_cpu: null buffer");
  for (int64_t i = 0; i < n; ++i)
    azd::solve_one(own[i], opp[i], max_empties, alpha, beta, node_limit, score_o + i, best_o + i,
                   nodes_o ? nodes_o + i : nullptr);
  return AZ_OK;
}

int oth_solve_deep_gpu(const uint64_t* own, const uint64_t* opp, int64_t n, int32_t max_empties,
                       int32_t alpha, int32_t beta, uint64_t node_limit, int32_t split_plies,
                       int8_t* score_o, uint8_t* best_o, uint64_t* nodes_o, void* workspace,
                       size_t* workspace_bytes, void* stream) {
  AZ_REQUIRE(n >= 0 && n < (int64_t(1) << 31), AZ_ERR_ARG,
             "oth_solve_deep_gpu: n=%lld outside 0..2^31", (long long)n);
  AZ_REQUIRE(max_empties >= 0 && max_empties <= AZ_SOLVE_DEEP_MAX_EMPTIES, AZ_ERR_ARG,
             "oth_solve_deep_gpu: max_empties=%d outside 0..%d", (int)max_empties,
             AZ_SOLVE_DEEP_MAX_EMPTIES);
  AZ_REQUIRE(window_ok(alpha, beta), AZ_ERR_ARG,
             "oth_solve_deep_gpu: window (%d, %d) is empty or outside -65..65", (int)alpha,
             (int)beta);
  AZ_REQUIRE(split_plies >= 0 && split_plies <= 2, AZ_ERR_ARG,
             "oth_solve_deep_gpu: split_plies=%d outside 0..2", (int)split_plies);
  AZ_REQUIRE(workspace_bytes, AZ_ERR_ARG, "oth_solve_deep_gpu: null workspace_bytes");
  const Plan pl = plan_for(n, max_empties, split_plies);
  const size_t need = split_plies == 0 ? align_up(kCtrWords * 4) : carve(nullptr, pl.cap, nullptr);
  if (!workspace) {
    *workspace_bytes = need;
    return AZ_OK;
  }
  AZ_REQUIRE(*workspace_bytes >= need, AZ_ERR_ARG,
             "oth_solve_deep_gpu: workspace %zu < %zu bytes", *workspace_bytes, need);
  AZ_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0, AZ_ERR_ARG,
             "oth_solve_deep_gpu: workspace must be 8-byte aligned");
  if (n == 0) return AZ_OK;
  AZ_REQUIRE(own && opp && score_o && best_o, AZ_ERR_ARG, "oth_solve_deep_gpu: null buffer");
  hipStream_t s = azc::as_stream(stream);
  if (split_plies == 0) {
    uint32_t* ctr = static_cast<uint32_t*>(workspace);
    AZ_HIP(hipMemsetAsync(ctr, 0, kCtrWords * 4, s));
    return launch_deep(own, opp, nullptr, nullptr, (uint32_t)n, max_empties, alpha, beta, nullptr,
                       nullptr, node_limit, ctr + kCtrQueue, score_o, best_o, nodes_o, s);
  }
  SplitWs ws;
  carve(static_cast<char*>(workspace), pl.cap, &ws);
  const uint32_t b1 = (uint32_t)pl.chunk, b2 = (uint32_t)(pl.chunk + pl.cap1);
  for (int64_t off = 0; off < n; off += pl.chunk) {
    const uint32_t r = (uint32_t)(n - off < pl.chunk ? n - off : pl.chunk);
    AZ_HIP(hipMemsetAsync(ws.ctr, 0, kCtrWords * 4, s));
    hipLaunchKernelGGL(k_deep_expand, dim3(aux_grid(r)), dim3(kAuxBlock), 0, s, ws, own + off,
                       opp + off, 0u, r, -1, b1, (uint32_t)pl.cap1, (int)kCtrL1,
                       split_plies == 1 ? 1 : 0, (int)max_empties, (int)AZ_SOLVE_SPLIT_MIN,
                       (int)alpha, (int)beta);
    if (split_plies == 2)
      hipLaunchKernelGGL(k_deep_expand, dim3(aux_grid(pl.cap1)), dim3(kAuxBlock), 0, s, ws,
                         (const uint64_t*)nullptr, (const uint64_t*)nullptr, b1,
                         (uint32_t)pl.cap1, (int)kCtrL1, b2, (uint32_t)pl.cap2, (int)kCtrL2, 1,
                         (int)max_empties, (int)AZ_SOLVE_SPLIT_MIN, (int)alpha, (int)beta);
    AZ_HIP(hipGetLastError());
    const int rc = launch_deep(ws.own, ws.opp, ws.task, ws.ctr + kCtrTasks, 0u, max_empties,
                               alpha, beta, ws.wa, ws.wb, node_limit, ws.ctr + kCtrQueue,
                               ws.score, ws.best, ws.nodes, s);
    if (rc != AZ_OK) return rc;
    if (split_plies == 2)
      hipLaunchKernelGGL(k_deep_combine, dim3(aux_grid(pl.cap2)), dim3(kAuxBlock), 0, s, ws, b2,
                         (uint32_t)pl.cap2, (int)kCtrL2);
    hipLaunchKernelGGL(k_deep_combine, dim3(aux_grid(pl.cap1)), dim3(kAuxBlock), 0, s, ws, b1,
                       (uint32_t)pl.cap1, (int)kCtrL1);
    hipLaunchKernelGGL(k_deep_finish, dim3(aux_grid(r)), dim3(kAuxBlock), 0, s, ws, r,
                       score_o + off, best_o + off, nodes_o ? nodes_o + off : nullptr);
    AZ_HIP(hipGetLastError());
  }
  return AZ_OK;
}

}  // extern "C"
