// solve.hip — exact endgame solver entry points (oth_solve_cpu / oth_solve_gpu).
//
// The search itself is solve.h's step(), the same code on both sides.  On the device k_solve
// is the lane kernel of lane_search.h, its frames (capture set, untried moves, packed window)
// 20 bytes each.  With split_plies = 1 or 2 the front end of split_front.h expands roots with
// at least AZ_SOLVE_SPLIT_MIN empties, and every leaf of that small tree is a full-window task
// of the same k_solve queue.
#include "bitboard.h"
#include "common.h"
#include "lane_search.h"
#include "solve.h"
#include "split_front.h"

static_assert(AZ_SOLVE_SKIPPED == azs::kSkipped && AZ_SOLVE_ABORTED == azs::kAborted &&
                  AZ_SOLVE_MAX_EMPTIES == azs::kMaxEmpties,
              "include/az_othello.h and csrc/solve.h disagree");

namespace {

constexpr int kSolveBlock = 128;  // two waves: the LDS granule that fits 4 / 5 / 9 per CU
using Stack = azl::LdsStack<kSolveBlock, 2, true>;

struct SolveSplit {
  using Value = int8_t;
  static constexpr int kBias = 64, kAborted = azs::kAborted;
  // roots per chunk: bounds the workspace (a root has at most 14 children and 14 * 13
  // grandchildren) while one chunk still fills the chip with tasks
  static constexpr int kChunk1 = 16384, kChunk2 = 2048;
  struct Params {
    int max_empties;
  };
  static size_t children1(const Params& q) { return q.max_empties < 1 ? 1 : q.max_empties; }
  static size_t children2(const Params& q) { return q.max_empties < 2 ? 1 : q.max_empties - 1; }
  static __device__ bool expand_root(const Params& q, uint64_t o, uint64_t p) {
    const int e = 64 - azb::popc(o | p);
    return e >= AZ_SOLVE_SPLIT_MIN && e <= q.max_empties;
  }
  static constexpr int kExtras = 0;
  static __device__ azf::Extra root_extra(const Params&) { return {}; }
  static __device__ azf::Extra child_extra(azf::Extra x, bool) { return x; }
};

// NF = frames of LDS stack per lane (max_empties - 1 at most are ever used).  Task t is
// position task_ids[t] (or t itself) of own / opp; results go to the same index.
template <int NF>
__global__ __launch_bounds__(kSolveBlock) void k_solve(
    const uint64_t* __restrict__ own, const uint64_t* __restrict__ opp,
    const int32_t* __restrict__ task_ids, const uint32_t* __restrict__ n_ptr, uint32_t n_host,
    int max_empties, uint64_t node_limit, uint32_t* __restrict__ queue,
    int8_t* __restrict__ score_o, uint8_t* __restrict__ best_o, uint64_t* __restrict__ nodes_o) {
  __shared__ uint64_t lds[Stack::words(NF)];
  Stack st(lds, NF);
  uint32_t node = 0;
  azl::run_lanes<azs::Search>(
      st, n_ptr ? *n_ptr : n_host, queue, node_limit, NF,
      [&](azs::Search& s, uint32_t t) {
        node = task_ids ? (uint32_t)task_ids[t] : t;
        azs::init(s, own[node], opp[node], max_empties);
      },
      [&](const azs::Search& s) {
        score_o[node] = (int8_t)s.score;
        best_o[node] = (uint8_t)s.root_best;
        if (nodes_o) nodes_o[node] = s.nodes;
      });
}

template <int NF>
int launch_nf(const azf::TaskList<SolveSplit>& t, int max_empties, uint64_t node_limit,
              hipStream_t stream) {
  unsigned grid = 0;
  const int rc = azl::fill_grid(&grid, kSolveBlock, Stack::lds_bytes(NF), t.n_ptr, t.n_host);
  if (rc != AZ_OK) return rc;
  hipLaunchKernelGGL(k_solve<NF>, dim3(grid), dim3(kSolveBlock), 0, stream, t.own, t.opp, t.ids,
                     t.n_ptr, t.n_host, max_empties, node_limit, t.queue, t.value, t.best,
                     t.nodes);
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
  AZ_REQUIRE(max_empties >= 0 && max_empties <= AZ_SOLVE_MAX_EMPTIES, AZ_ERR_ARG,
             "oth_solve_gpu: max_empties=%d outside 0..%d", (int)max_empties,
             AZ_SOLVE_MAX_EMPTIES);
  const SolveSplit::Params par{max_empties};
  bool run = false;
  const int rc = azl::claim_workspace(
      "oth_solve_gpu", "n", n, split_plies, azf::workspace_need<SolveSplit>(n, split_plies, par),
      workspace, workspace_bytes, own && opp && score_o && best_o, &run);
  if (rc != AZ_OK || !run) return rc;
  hipStream_t s = azc::as_stream(stream);
  return azf::run<SolveSplit>(
      own, opp, n, split_plies, par, score_o, best_o, nodes_o, workspace, s,
      [&](const azf::TaskList<SolveSplit>& t) {
        return max_empties <= 8    ? launch_nf<7>(t, max_empties, node_limit, s)
               : max_empties <= 12 ? launch_nf<11>(t, max_empties, node_limit, s)
                                   : launch_nf<13>(t, max_empties, node_limit, s);
      });
}

}  // extern "C"
