// solve_deep.hip — windowed, move-ordered endgame solver entry points (oth_solve_deep_cpu /
// oth_solve_deep_gpu).  The search is solve_deep.h's step(), the same code on both sides.
//
// On the device k_solve_deep is the lane kernel of lane_search.h, its frames (capture set,
// untried moves, order word, packed window) 28 bytes each; at most 20 probes precede each node
// of a search.  A workgroup is one wave: there is no barrier, and the smaller LDS granule
// (28 bytes * frames * 64) packs a CU better.
//
// With split_plies = 1 or 2 the front end of split_front.h expands roots with at least
// AZ_SOLVE_SPLIT_MIN empties, with a window per node (the two per-node bytes): a child's window
// is its parent's negated and swapped (every child, the one after a pass included, has the
// other side to move), and every leaf of that small tree is a task of the same k_solve_deep
// queue.  The maximum of the combine is sound for bounds: a child's v_c in its window (-b, -a)
// gives the move's value -v_c exactly inside (a, b), an upper bound <= a below it and a lower
// bound >= b above it, so the maximum over the moves obeys the parent's contract in (a, b),
// and its argmax is an optimal move (exact result) or a move worth >= b (fail high).
// Siblings do not narrow each other's windows, so a split search visits more nodes than an
// unsplit one.
#include "bitboard.h"
#include "common.h"
#include "lane_search.h"
#include "solve_deep.h"
#include "split_front.h"

static_assert(AZ_SOLVE_SKIPPED == azd::kSkipped && AZ_SOLVE_ABORTED == azd::kAborted &&
                  AZ_SOLVE_DEEP_MAX_EMPTIES == azd::kMaxEmpties,
              "include/az_othello.h and csrc/solve_deep.h disagree");

namespace {

constexpr int kDeepBlock = 64;  // one wave
using Stack = azl::LdsStack<kDeepBlock, 3, true>;

struct DeepSplit {
  using Value = int8_t;
  static constexpr int kBias = 64, kAborted = azd::kAborted;
  // roots per chunk (a root has at most max_empties children)
  static constexpr int kChunk1 = 16384, kChunk2 = 2048;
  struct Params {
    int max_empties, alpha, beta;
  };
  static size_t children1(const Params& q) { return q.max_empties < 1 ? 1 : q.max_empties; }
  static size_t children2(const Params& q) { return q.max_empties < 2 ? 1 : q.max_empties - 1; }
  static __device__ bool expand_root(const Params& q, uint64_t o, uint64_t p) {
    const int e = 64 - azb::popc(o | p);
    return e >= AZ_SOLVE_SPLIT_MIN && e <= q.max_empties;
  }
  static constexpr int kExtras = 2;  // the window (a, b) as two int8_t
  static __device__ azf::Extra root_extra(const Params& q) {
    return {{(uint8_t)q.alpha, (uint8_t)q.beta}};
  }
  static __device__ azf::Extra child_extra(azf::Extra x, bool) {
    const int a = (int8_t)x.b[0], b = (int8_t)x.b[1];
    return {{(uint8_t)-b, (uint8_t)-a}};
  }
};

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
  __shared__ uint64_t lds[Stack::words(NF)];
  Stack st(lds, NF);
  uint32_t node = 0;
  azl::run_lanes<azd::Search>(
      st, n_ptr ? *n_ptr : n_host, queue, node_limit, NF,
      [&](azd::Search& s, uint32_t t) {
        node = task_ids ? (uint32_t)task_ids[t] : t;
        azd::init(s, own[node], opp[node], max_empties, wa ? (int)wa[node] : alpha,
                  wb ? (int)wb[node] : beta);
      },
      [&](const azd::Search& s) {
        score_o[node] = (int8_t)s.score;
        best_o[node] = (uint8_t)s.root_best;
        if (nodes_o) nodes_o[node] = s.nodes;
      });
}

template <int NF>
int launch_nf(const azf::TaskList<DeepSplit>& t, const DeepSplit::Params& q, uint64_t node_limit,
              hipStream_t stream) {
  unsigned grid = 0;
  const int rc = azl::fill_grid(&grid, kDeepBlock, Stack::lds_bytes(NF), t.n_ptr, t.n_host);
  if (rc != AZ_OK) return rc;
  hipLaunchKernelGGL(k_solve_deep<NF>, dim3(grid), dim3(kDeepBlock), 0, stream, t.own, t.opp,
                     t.ids, t.n_ptr, t.n_host, q.max_empties, q.alpha, q.beta,
                     reinterpret_cast<const int8_t*>(t.extra[0]),
                     reinterpret_cast<const int8_t*>(t.extra[1]), node_limit, t.queue, t.value,
                     t.best, t.nodes);
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
  AZ_REQUIRE(max_empties >= 0 && max_empties <= AZ_SOLVE_DEEP_MAX_EMPTIES, AZ_ERR_ARG,
             "oth_solve_deep_gpu: max_empties=%d outside 0..%d", (int)max_empties,
             AZ_SOLVE_DEEP_MAX_EMPTIES);
  AZ_REQUIRE(window_ok(alpha, beta), AZ_ERR_ARG,
             "oth_solve_deep_gpu: window (%d, %d) is empty or outside -65..65", (int)alpha,
             (int)beta);
  const DeepSplit::Params par{max_empties, alpha, beta};
  bool run = false;
  const int rc = azl::claim_workspace(
      "oth_solve_deep_gpu", "n", n, split_plies,
      azf::workspace_need<DeepSplit>(n, split_plies, par), workspace, workspace_bytes,
      own && opp && score_o && best_o, &run);
  if (rc != AZ_OK || !run) return rc;
  hipStream_t s = azc::as_stream(stream);
  return azf::run<DeepSplit>(own, opp, n, split_plies, par, score_o, best_o, nodes_o, workspace, s,
                             [&](const azf::TaskList<DeepSplit>& t) {
                               return max_empties <= 12   ? launch_nf<11>(t, par, node_limit, s)
                                      : max_empties <= 16 ? launch_nf<15>(t, par, node_limit, s)
                                                          : launch_nf<19>(t, par, node_limit, s);
                             });
}

}  // extern "C"
