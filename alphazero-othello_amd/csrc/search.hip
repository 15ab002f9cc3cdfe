// search.hip — depth-limited alpha-beta entry points (oth_eval_* / oth_search_*).
//
// The search itself is search.h's step(), the same code on both sides.  On the device
// k_search is the lane kernel of lane_search.h, its frames three 8-byte words.  With
// split_plies = 1 or 2 and depth > split_plies the front end of split_front.h expands every
// non-terminal root; a placement child has one ply less than its parent and a pass child
// keeps its depth (the per-node byte), and every leaf of that small tree is a full-window
// task of the same k_search queue.
#include "bitboard.h"
#include "common.h"
#include "lane_search.h"
#include "search.h"
#include "split_front.h"

static_assert(AZ_SEARCH_SKIPPED == azq::kSkipped && AZ_SEARCH_ABORTED == azq::kAborted &&
                  AZ_SEARCH_MAX_DEPTH == azq::kMaxDepth,
              "include/az_othello.h and csrc/search.h disagree");

namespace {

constexpr int kSearchBlock = 128;  // two waves, as k_solve
using Stack = azl::LdsStack<kSearchBlock, 3, false>;

struct SearchSplit {
  using Value = int16_t;
  static constexpr int kBias = 32768, kAborted = azq::kAborted;
  // roots per chunk: bounds the workspace while one chunk still fills the chip with tasks
  static constexpr int kChunk1 = 16384, kChunk2 = 1024;
  struct Params {
    int depth;
  };
  // no reachable position has more than 33 placements; an arbitrary board with more may
  // overrun its level and is then reported aborted
  static size_t children1(const Params&) { return 33; }
  static size_t children2(const Params&) { return 33; }
  static __device__ bool expand_root(const Params&, uint64_t, uint64_t) { return true; }
  static constexpr int kExtras = 1;  // the plies left at the node
  static __device__ azf::Extra root_extra(const Params& q) { return {{(uint8_t)q.depth, 0}}; }
  static __device__ azf::Extra child_extra(azf::Extra x, bool pass) {
    return {{(uint8_t)(pass ? x.b[0] : x.b[0] - 1), 0}};
  }
};

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
  __shared__ uint64_t lds[Stack::words(NF)];
  Stack st(lds, NF);
  uint32_t node = 0;
  azl::run_lanes<azq::Search>(
      st, n_ptr ? *n_ptr : n_host, queue, node_limit, NF,
      [&](azq::Search& s, uint32_t t) {
        node = task_ids ? (uint32_t)task_ids[t] : t;
        azq::init(s, own[node], opp[node], depth_of ? (int)depth_of[node] : depth);
      },
      [&](const azq::Search& s) {
        value_o[node] = (int16_t)s.score;
        best_o[node] = (uint8_t)s.root_best;
        if (nodes_o) nodes_o[node] = s.nodes;
      });
}

__global__ __launch_bounds__(azf::kAuxBlock) void k_eval(const uint64_t* __restrict__ own,
                                                         const uint64_t* __restrict__ opp,
                                                         int64_t n, int16_t* __restrict__ value_o) {
  const int64_t stride = (int64_t)gridDim.x * azf::kAuxBlock;
  for (int64_t i = (int64_t)blockIdx.x * azf::kAuxBlock + threadIdx.x; i < n; i += stride)
    value_o[i] = (int16_t)azq::evaluate(own[i], opp[i]);
}

// max_depth = the deepest task of the launch (a root's depth; sizes the LDS stack)
template <int NF>
int launch_nf(const azf::TaskList<SearchSplit>& t, int max_depth, uint64_t node_limit,
              hipStream_t stream) {
  unsigned grid = 0;
  const int rc = azl::fill_grid(&grid, kSearchBlock, Stack::lds_bytes(NF), t.n_ptr, t.n_host);
  if (rc != AZ_OK) return rc;
  hipLaunchKernelGGL(k_search<NF>, dim3(grid), dim3(kSearchBlock), 0, stream, t.own, t.opp, t.ids,
                     t.extra[0], t.n_ptr, t.n_host, max_depth, node_limit, t.queue, t.value,
                     t.best, t.nodes);
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
  hipLaunchKernelGGL(k_eval, dim3(azf::aux_grid((size_t)n)), dim3(azf::kAuxBlock), 0,
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
  AZ_REQUIRE(depth >= 1 && depth <= AZ_SEARCH_MAX_DEPTH, AZ_ERR_ARG,
             "oth_search_gpu: depth=%d outside 1..%d", (int)depth, AZ_SEARCH_MAX_DEPTH);
  const SearchSplit::Params par{depth};
  const int split = depth <= split_plies ? 0 : split_plies;  // nothing below the split: one search
  bool run = false;
  const int rc = azl::claim_workspace(
      "oth_search_gpu", "n", n, split_plies, azf::workspace_need<SearchSplit>(n, split, par),
      workspace, workspace_bytes, own && opp && value_o && best_o, &run);
  if (rc != AZ_OK || !run) return rc;
  hipStream_t s = azc::as_stream(stream);
  // a task is a root (terminal or overlapping: finished by init) or a node at least one ply
  // down, a pass child keeping its parent's depth
  return azf::run<SearchSplit>(own, opp, n, split, par, value_o, best_o, nodes_o, workspace, s,
                               [&](const azf::TaskList<SearchSplit>& t) {
                                 return depth <= 4   ? launch_nf<3>(t, depth, node_limit, s)
                                        : depth <= 7 ? launch_nf<6>(t, depth, node_limit, s)
                                                     : launch_nf<9>(t, depth, node_limit, s);
                               });
}

}  // extern "C"
