// records.hip — recorded games to training rows (oth_records_cpu / oth_records_gpu).
//
// The replay itself is records.h's entry(), the same code on both sides.  On the device one
// lane replays one game (k_records): its transcript line (at most 128 bytes) is fetched up
// front as 16-byte loads into registers, the loop over the entries runs until every game of
// the wavefront has stopped (so its bound is the wave's longest game) and picks the current
// 16-byte chunk, word and byte with wave-uniform selects -- no LDS, no atomics, no
// runtime-indexed private array.  Rows are stored ply-major (row r of game g at r*n + g):
// while the games of a wavefront are on the same row, which they are until a pass or a stop,
// its 64 lanes store 64 consecutive elements of each output array.
#include "bitboard.h"
#include "common.h"
#include "records.h"

static_assert(AZ_REC_TERMINAL == azr::kTerminal && AZ_REC_UNFINISHED == azr::kUnfinished &&
                  AZ_REC_ILLEGAL == azr::kIllegal && AZ_REC_OVERFLOW == azr::kOverflow &&
                  AZ_REC_PASS_ROWS == azr::kPassRows && AZ_REC_MAX_STRIDE == azr::kMaxStride &&
                  AZ_REC_MAX_ROWS == azr::kMaxRows,
              "include/az_othello.h and csrc/records.h disagree");

namespace {

constexpr int kBlock = 256;

// the ply-major row store of game `g` of `n`
struct RowSink {
  uint64_t* own_o;
  uint64_t* opp_o;
  uint8_t* act_o;
  uint8_t* ply_o;
  int64_t n, g;
  AZ_HD void row(int r, uint64_t own, uint64_t opp, int act, int ply) {
    const int64_t k = (int64_t)r * n + g;
    own_o[k] = own;
    opp_o[k] = opp;
    act_o[k] = (uint8_t)act;
    ply_o[k] = (uint8_t)ply;
  }
};

struct GameOut {
  int8_t* z_o;
  int32_t* n_rows;
  uint8_t* status;
  uint8_t* bad_ply;
  uint64_t* final_own;
  uint64_t* final_opp;
  int8_t* final_colour;
  int8_t* final_diff;
};

// the per-game outputs and the rows' z, once the game has stopped
AZ_HD void write_game(const azr::Game& gm, const int8_t* winner, int64_t n, int64_t g,
                      const GameOut& o) {
  const int w = azr::outcome(gm, winner, g);
  for (int r = 0; r < gm.rows; ++r) o.z_o[(int64_t)r * n + g] = (int8_t)azr::z_of(gm, r, w);
  o.n_rows[g] = gm.rows;
  o.status[g] = (uint8_t)gm.status;
  o.bad_ply[g] = (uint8_t)gm.bad;
  o.final_own[g] = gm.own;
  o.final_opp[g] = gm.opp;
  o.final_colour[g] = (int8_t)gm.colour;
  o.final_diff[g] = (int8_t)azr::final_diff(gm);
}

// One 16-byte chunk of a transcript line, or end marks past the line / for a lane without a
// game.
__device__ __forceinline__ uint4 load_chunk(const uint8_t* line, int c, bool have) {
  return have ? reinterpret_cast<const uint4*>(line)[c] : make_uint4(~0u, ~0u, ~0u, ~0u);
}

__device__ __forceinline__ uint4 sel4(bool p, const uint4& a, const uint4& b) {
  return make_uint4(p ? a.x : b.x, p ? a.y : b.y, p ? a.z : b.z, p ? a.w : b.w);
}

__global__ __launch_bounds__(kBlock) void k_records(
    const uint8_t* __restrict__ acts, int stride, const uint64_t* __restrict__ own0,
    const uint64_t* __restrict__ opp0, const int8_t* __restrict__ winner, int64_t n, int max_rows,
    int flags, RowSink sink, GameOut out) {
  const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool live = g < n;
  const int chunks = stride >> 4;
  // the whole line in registers: eight named chunks (an array indexed by the loop's chunk
  // number would live in scratch), the current one picked by a tree of wave-uniform selects
  const uint8_t* line = acts + (live ? g : 0) * stride;
  const uint4 t0 = load_chunk(line, 0, live), t1 = load_chunk(line, 1, live && chunks > 1),
              t2 = load_chunk(line, 2, live && chunks > 2),
              t3 = load_chunk(line, 3, live && chunks > 3),
              t4 = load_chunk(line, 4, live && chunks > 4),
              t5 = load_chunk(line, 5, live && chunks > 5),
              t6 = load_chunk(line, 6, live && chunks > 6),
              t7 = load_chunk(line, 7, live && chunks > 7);
  azr::Game gm;
  azr::init(gm, live && own0 ? own0[g] : azb::kInitOwn, live && opp0 ? opp0[g] : azb::kInitOpp);
  if (!live) gm.status = azr::kTerminal;
  sink.g = g;
  uint4 cur = t0;
  for (int i = 0; i < stride; ++i) {
    if (__ballot(gm.status == azr::kRunning) == 0) break;
    if ((i & 15) == 0) {
      const int c = i >> 4;
      cur = sel4(c & 4, sel4(c & 2, sel4(c & 1, t7, t6), sel4(c & 1, t5, t4)),
                 sel4(c & 2, sel4(c & 1, t3, t2), sel4(c & 1, t1, t0)));
    }
    const int w = (i >> 2) & 3;
    const uint32_t word = w == 0 ? cur.x : (w == 1 ? cur.y : (w == 2 ? cur.z : cur.w));
    const int a = (int)((word >> ((i & 3) * 8)) & 0xFFu);
    if (gm.status == azr::kRunning) azr::entry(gm, i, a, flags, max_rows, sink);
  }
  if (!live) return;
  azr::finish(gm);
  write_game(gm, winner, n, g, out);
}

int check_args(const char* who, const uint8_t* acts, int32_t stride, const uint64_t* own0,
               const uint64_t* opp0, int64_t n, int32_t max_rows, int32_t flags,
               const RowSink& s, const GameOut& o) {
  AZ_REQUIRE(n >= 0, AZ_ERR_ARG, "%s: n=%lld < 0", who, (long long)n);
  AZ_REQUIRE(stride > 0 && stride <= AZ_REC_MAX_STRIDE && stride % 16 == 0, AZ_ERR_ARG,
             "%s: stride=%d is not a multiple of 16 in 16..%d", who, (int)stride,
             AZ_REC_MAX_STRIDE);
  AZ_REQUIRE(max_rows >= 0 && max_rows <= AZ_REC_MAX_ROWS, AZ_ERR_ARG,
             "%s: max_rows=%d outside 0..%d", who, (int)max_rows, AZ_REC_MAX_ROWS);
  AZ_REQUIRE((flags & ~AZ_REC_PASS_ROWS) == 0, AZ_ERR_ARG, "%s: unknown flags 0x%x", who,
             (unsigned)flags);
  AZ_REQUIRE((own0 == nullptr) == (opp0 == nullptr), AZ_ERR_ARG,
             "%s: own0 and opp0 must both be given or both be NULL", who);
  if (n == 0) return AZ_OK;
  AZ_REQUIRE(acts && o.n_rows && o.status && o.bad_ply && o.final_own && o.final_opp &&
                 o.final_colour && o.final_diff,
             AZ_ERR_ARG, "%s: null buffer", who);
  AZ_REQUIRE(max_rows == 0 || (s.own_o && s.opp_o && s.act_o && s.ply_o && o.z_o), AZ_ERR_ARG,
             "%s: null row buffer", who);
  AZ_REQUIRE((reinterpret_cast<uintptr_t>(acts) & 15u) == 0, AZ_ERR_ARG,
             "%s: acts must be 16-byte aligned", who);
  return AZ_OK;
}

}  // namespace

extern "C" {

int oth_records_cpu(const uint8_t* acts, int32_t stride, const uint64_t* own0,
                    const uint64_t* opp0, const int8_t* winner, int64_t n, int32_t max_rows,
                    int32_t flags, uint64_t* own_o, uint64_t* opp_o, uint8_t* act_o, int8_t* z_o,
                    uint8_t* ply_o, int32_t* n_rows, uint8_t* status, uint8_t* bad_ply,
                    uint64_t* final_own, uint64_t* final_opp, int8_t* final_colour,
                    int8_t* final_diff) {
  RowSink sink{own_o, opp_o, act_o, ply_o, n, 0};
  const GameOut out{z_o, n_rows, status, bad_ply, final_own, final_opp, final_colour, final_diff};
  const int rc = check_args("oth_records_cpu", acts, stride, own0, opp0, n, max_rows, flags,
                            sink, out);
  if (rc != AZ_OK) return rc;
  for (int64_t g = 0; g < n; ++g) {
    const uint8_t* line = acts + g * stride;
    azr::Game gm;
    azr::init(gm, own0 ? own0[g] : azb::kInitOwn, opp0 ? opp0[g] : azb::kInitOpp);
    sink.g = g;
    for (int i = 0; i < stride && gm.status == azr::kRunning; ++i)
      azr::entry(gm, i, line[i], flags, max_rows, sink);
    azr::finish(gm);
    write_game(gm, winner, n, g, out);
  }
  return AZ_OK;
}

int oth_records_gpu(const uint8_t* acts, int32_t stride, const uint64_t* own0,
                    const uint64_t* opp0, const int8_t* winner, int64_t n, int32_t max_rows,
                    int32_t flags, uint64_t* own_o, uint64_t* opp_o, uint8_t* act_o, int8_t* z_o,
                    uint8_t* ply_o, int32_t* n_rows, uint8_t* status, uint8_t* bad_ply,
                    uint64_t* final_own, uint64_t* final_opp, int8_t* final_colour,
                    int8_t* final_diff, void* stream) {
  RowSink sink{own_o, opp_o, act_o, ply_o, n, 0};
  const GameOut out{z_o, n_rows, status, bad_ply, final_own, final_opp, final_colour, final_diff};
  const int rc = check_args("oth_records_gpu", acts, stride, own0, opp0, n, max_rows, flags,
                            sink, out);
  if (rc != AZ_OK) return rc;
  if (n == 0) return AZ_OK;
  AZ_REQUIRE(n * (int64_t)(max_rows > 0 ? max_rows : 1) < (int64_t(1) << 31), AZ_ERR_ARG,
             "oth_records_gpu: n * max_rows = %lld * %d is 2^31 or more", (long long)n,
             (int)max_rows);
  const unsigned grid = (unsigned)((n + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(k_records, dim3(grid), dim3(kBlock), 0, azc::as_stream(stream), acts,
                     (int)stride, own0, opp0, winner, n, (int)max_rows, (int)flags, sink, out);
  AZ_HIP(hipGetLastError());
  return AZ_OK;
}

}  // extern "C"
