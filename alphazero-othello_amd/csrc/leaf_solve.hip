// leaf_solve.hip — exact win / draw / loss values for late leaves of the search
// (az_leaf_solve_cpu / az_leaf_solve_gpu / az_leaf_solve_stats_gpu).
//
// The evaluators write values[row] for the canonical planes in nn_in[row]; the expansion
// reads values later on the same stream.  Between the two, this pass decodes every row's
// bitboards from its planes and, where the position has 1..max_empties empties, replaces the
// net's guess by sign(score) of solve_deep.h's search in the window (-1, 1).  Every other
// row (no leaf, a full board, more empties, a search that passed node_limit) keeps its value
// bit for bit.  The result depends on the position only up to the board's symmetries, so
// D4-augmented rows (the planes of a transformed board) need nothing extra.
//
// Two kernels behind a counter reset, a linear chain on the caller's stream with no host
// synchronisation, no allocation and no host read in it (it captures into a HIP graph):
//
//   k_leaf_decode  one wave per row: lane i loads nn_in[row][i] (one coalesced 256-byte read),
//                  two ballots give own / opp, and a row that qualifies appends itself to the
//                  task list in the workspace with one atomic add.
//   k_leaf_solve   the lane kernel of lane_search.h over azd::init / azd::step with
//                  k_solve_deep's frames, 11 of them (12 empties at most).  The task count is
//                  read from the workspace; the grid follows `rows` (a step has a few thousand
//                  rows and usually a few dozen tasks), not the device's size.
//
// Every loop is bounded: the lane loop by the task count, a search by node_limit nodes with at
// most 20 probes before each; no lane waits for another.  The order in which rows enter the
// task list varies from run to run; a row's result does not depend on it, and the counters are
// sums.
//
// Workspace (device memory, 8-byte aligned, zeroed once by its owner; one caller on one
// stream): a 256-byte head {u32 queue, u32 tasks, ..., u64 stats[3] at byte 64}, then the
// task list (int32 row, u64 own, u64 opp per row).  Each call re-arms queue and tasks; the
// stats accumulate until the owner zeroes the workspace again.
#include "bitboard.h"
#include "common.h"
#include "lane_search.h"
#include "solve_deep.h"

namespace {

constexpr int kWave = 64;
constexpr int kDecodeBlock = 256;  // four rows per block
constexpr int kLeafFrames = 11;    // AZ_LEAF_SOLVE_MAX_EMPTIES - 1
constexpr size_t kHeadBytes = 256;
constexpr size_t kStatsOffset = 64;  // bytes

static_assert(AZ_LEAF_SOLVE_MAX_EMPTIES == kLeafFrames + 1 &&
                  AZ_LEAF_SOLVE_MAX_EMPTIES <= azd::kMaxEmpties,
              "include/az_othello.h and csrc/leaf_solve.hip disagree");

using Stack = azl::LdsStack<kWave, 3, true>;  // k_solve_deep's

struct LeafWs {
  uint32_t* ctr;    // [0] queue, [1] tasks
  uint64_t* stats;  // [3] rows solved, rows left at the node limit, nodes
  int32_t* row;     // [rows]
  uint64_t *own, *opp;
};

size_t layout(char* base, size_t rows, LeafWs* ws) {
  size_t off = kHeadBytes;
  auto take = [&](size_t bytes) {
    char* q = base ? base + off : nullptr;
    off += azl::align_up(bytes);
    return q;
  };
  LeafWs w;
  w.ctr = reinterpret_cast<uint32_t*>(base);
  w.stats = reinterpret_cast<uint64_t*>(base ? base + kStatsOffset : nullptr);
  w.row = reinterpret_cast<int32_t*>(take(rows * 4));
  w.own = reinterpret_cast<uint64_t*>(take(rows * 8));
  w.opp = reinterpret_cast<uint64_t*>(take(rows * 8));
  if (ws) *ws = w;
  return off;
}

// planes -> bitboards: own = squares above 0.5, opp = squares below -0.5
inline void decode_row_host(const float* x, uint64_t* own, uint64_t* opp) {
  uint64_t o = 0, p = 0;
  for (int i = 0; i < 64; ++i) {
    o |= (uint64_t)(x[i] > 0.5f) << i;
    p |= (uint64_t)(x[i] < -0.5f) << i;
  }
  *own = o;
  *opp = p;
}

AZ_HD bool qualifies(uint64_t own, uint64_t opp, int max_empties) {
  const int e = 64 - azb::popc(own | opp);
  return e >= 1 && e <= max_empties;
}

AZ_HD float sign_value(int score) { return score > 0 ? 1.0f : (score < 0 ? -1.0f : 0.0f); }

__global__ __launch_bounds__(kDecodeBlock) void k_leaf_decode(const float* __restrict__ nn_in,
                                                              int64_t rows, int max_empties,
                                                              LeafWs ws) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t r = (int64_t)blockIdx.x * (kDecodeBlock / kWave) + (threadIdx.x >> 6);
  if (r >= rows) return;  // the whole wave
  const float x = nn_in[r * 64 + lane];
  const uint64_t own = __ballot(x > 0.5f), opp = __ballot(x < -0.5f);
  if (lane == 0 && qualifies(own, opp, max_empties)) {
    const uint32_t t = atomicAdd(&ws.ctr[1], 1u);  // t < rows: a row appends itself once
    ws.row[t] = (int32_t)r;
    ws.own[t] = own;
    ws.opp[t] = opp;
  }
}

__global__ __launch_bounds__(kWave) void k_leaf_solve(float* __restrict__ values, int max_empties,
                                                      uint64_t node_limit, LeafWs ws) {
  __shared__ uint64_t lds[Stack::words(kLeafFrames)];
  Stack st(lds, kLeafFrames);
  int32_t row = 0;
  unsigned long long solved = 0, limited = 0, nodes = 0;
  azl::run_lanes<azd::Search>(
      st, ws.ctr[1], &ws.ctr[0], node_limit, kLeafFrames,
      [&](azd::Search& s, uint32_t t) {
        row = ws.row[t];
        azd::init(s, ws.own[t], ws.opp[t], max_empties, -1, 1);
      },
      [&](const azd::Search& s) {
        nodes += s.nodes;
        if (s.score == azd::kAborted) {
          ++limited;  // the net's value stays
        } else {
          ++solved;
          values[row] = sign_value(s.score);
        }
      });
  auto* stats = reinterpret_cast<unsigned long long*>(ws.stats);
  if (solved) atomicAdd(&stats[0], solved);
  if (limited) atomicAdd(&stats[1], limited);
  if (nodes) atomicAdd(&stats[2], nodes);
}

int check_args(const char* who, int64_t rows, int32_t max_empties, uint64_t node_limit) {
  AZ_REQUIRE(rows >= 0 && rows < (int64_t(1) << 31), AZ_ERR_ARG, "%s: rows=%lld outside 0..2^31",
             who, (long long)rows);
  AZ_REQUIRE(max_empties >= 1 && max_empties <= AZ_LEAF_SOLVE_MAX_EMPTIES, AZ_ERR_ARG,
             "%s: max_empties=%d outside 1..%d", who, (int)max_empties,
             AZ_LEAF_SOLVE_MAX_EMPTIES);
  AZ_REQUIRE(node_limit > 0, AZ_ERR_ARG, "%s: node_limit=0", who);
  return AZ_OK;
}

}  // namespace

extern "C" {

int az_leaf_solve_cpu(const float* nn_in, float* values, int64_t rows, int32_t max_empties,
                      uint64_t node_limit, uint64_t* stats3) {
  const int rc = check_args("az_leaf_solve_cpu", rows, max_empties, node_limit);
  if (rc != AZ_OK) return rc;
  AZ_REQUIRE(rows == 0 || (nn_in && values), AZ_ERR_ARG, "az_leaf_solve_cpu: null buffer");
  uint64_t solved = 0, limited = 0, nodes = 0;
  for (int64_t r = 0; r < rows; ++r) {
    uint64_t own, opp;
    decode_row_host(nn_in + r * 64, &own, &opp);
    if (!qualifies(own, opp, max_empties)) continue;
    azd::Search s;
    azd::HostStack st;
    azd::init(s, own, opp, max_empties, -1, 1);
    while (s.state == azd::kRun) azd::step(s, st, node_limit, kLeafFrames);
    nodes += s.nodes;
    if (s.score == azd::kAborted) {
      ++limited;
    } else {
      ++solved;
      values[r] = sign_value(s.score);
    }
  }
  if (stats3) {
    stats3[0] = solved;
    stats3[1] = limited;
    stats3[2] = nodes;
  }
  return AZ_OK;
}

int az_leaf_solve_gpu(const float* nn_in, float* values, int64_t rows, int32_t max_empties,
                      uint64_t node_limit, void* workspace, size_t* workspace_bytes,
                      void* stream) {
  int rc = check_args("az_leaf_solve_gpu", rows, max_empties, node_limit);
  if (rc != AZ_OK) return rc;
  bool run = false;
  rc = azl::claim_workspace("az_leaf_solve_gpu", "rows", rows, 0,
                            layout(nullptr, (size_t)rows, nullptr), workspace, workspace_bytes,
                            nn_in && values, &run);
  if (rc != AZ_OK || !run) return rc;
  LeafWs ws;
  layout(static_cast<char*>(workspace), (size_t)rows, &ws);
  hipStream_t s = azc::as_stream(stream);
  AZ_HIP(hipMemsetAsync(ws.ctr, 0, 2 * sizeof(uint32_t), s));
  constexpr int kRowsPerBlock = kDecodeBlock / kWave;
  hipLaunchKernelGGL(k_leaf_decode, dim3((unsigned)((rows + kRowsPerBlock - 1) / kRowsPerBlock)),
                     dim3(kDecodeBlock), 0, s, nn_in, rows, (int)max_empties, ws);
  // a lane per row at most: every task finds a lane at once, in as few waves as hold them
  hipLaunchKernelGGL(k_leaf_solve, dim3((unsigned)((rows + kWave - 1) / kWave)), dim3(kWave), 0, s,
                     values, (int)max_empties, node_limit, ws);
  AZ_HIP(hipGetLastError());
  return AZ_OK;
}

int az_leaf_solve_stats_gpu(const void* workspace, uint64_t* stats3, void* stream) {
  AZ_REQUIRE(workspace && stats3, AZ_ERR_ARG, "az_leaf_solve_stats_gpu: null argument");
  hipStream_t s = azc::as_stream(stream);
  AZ_HIP(hipMemcpyAsync(stats3, static_cast<const char*>(workspace) + kStatsOffset,
                        3 * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  AZ_HIP(hipStreamSynchronize(s));
  return AZ_OK;
}

}  // extern "C"
