// line_step.hip — oth_line_step_gpu / oth_line_step_cpu: one ply of every root's optimal line
// (line_step.h has the body, include/az_othello.h the contract).  The device kernel is one lane
// per root; the roots still alive after the ply are counted into *live_o (one atomic per wave),
// the one word this step adds to what the ply loop of endgame.optimal_line reads back.
#include <stdexcept>

#include "common.h"
#include "line_step.h"

namespace {

constexpr int kBlock = 256;

__global__ __launch_bounds__(kBlock) void k_line_step(azl::Line L, int32_t* __restrict__ live_o,
                                                      int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int alive = i < n ? azl::line_step_one(L, i) : 0;
  const unsigned long long m = __ballot(alive);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(live_o, (int)__popcll(m));
}

int check_args(const char* who, const azl::Line& L, const int32_t* live_o, int64_t n) {
  AZ_REQUIRE(n >= 0, AZ_ERR_ARG, "%s: n=%lld < 0", who, (long long)n);
  AZ_REQUIRE(n < (int64_t(1) << 24), AZ_ERR_ARG, "%s: n=%lld exceeds 2^24 roots per call", who,
             (long long)n);
  AZ_REQUIRE(L.stride >= 1 && L.stride <= 2 * AZ_SOLVE_DEEP_MAX_EMPTIES, AZ_ERR_ARG,
             "%s: stride=%d outside 1..%d", who, (int)L.stride, 2 * AZ_SOLVE_DEEP_MAX_EMPTIES);
  AZ_REQUIRE(live_o, AZ_ERR_ARG, "%s: null live counter", who);
  AZ_REQUIRE(n == 0 || (L.own && L.opp && L.values && L.score && L.count && L.done &&
                        L.root_score && L.row_own && L.row_opp && L.row_pi && L.row_act &&
                        L.row_z),
             AZ_ERR_ARG, "%s: null buffer", who);
  return AZ_OK;
}

}  // namespace

extern "C" {

int oth_line_step_cpu(uint64_t* own, uint64_t* opp, const int8_t* values, const int8_t* score,
                      int64_t n, int32_t stride, int32_t first, int32_t* count, uint8_t* done,
                      int8_t* root_score, uint64_t* row_own, uint64_t* row_opp, float* row_pi,
                      uint8_t* row_act, float* row_z, int32_t* live_o) {
  const azl::Line L{own, opp, values, score, count, done, root_score, row_own, row_opp,
                    row_pi, row_act, row_z, stride, first ? 1 : 0};
  if (const int rc = check_args("oth_line_step_cpu", L, live_o, n)) return rc;
  int32_t live = 0;
  for (int64_t i = 0; i < n; ++i) live += azl::line_step_one(L, i);
  *live_o = live;
  return AZ_OK;
}

int oth_line_step_gpu(uint64_t* own, uint64_t* opp, const int8_t* values, const int8_t* score,
                      int64_t n, int32_t stride, int32_t first, int32_t* count, uint8_t* done,
                      int8_t* root_score, uint64_t* row_own, uint64_t* row_opp, float* row_pi,
                      uint8_t* row_act, float* row_z, int32_t* live_o, void* stream) {
  const azl::Line L{own, opp, values, score, count, done, root_score, row_own, row_opp,
                    row_pi, row_act, row_z, stride, first ? 1 : 0};
  if (const int rc = check_args("oth_line_step_gpu", L, live_o, n)) return rc;
  hipStream_t s = azc::as_stream(stream);
  AZ_HIP(hipMemsetAsync(live_o, 0, sizeof(int32_t), s));
  if (n == 0) return AZ_OK;
  hipLaunchKernelGGL(k_line_step, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                     s, L, live_o, n);
  AZ_HIP(hipGetLastError());
  return AZ_OK;
}

}  // extern "C"
