// solve_moves.hip — the exact value of every move of a late position (oth_solve_moves_cpu):
// every root is expanded into its children, each child is one unsplit search of
// solve_deep.h in the window its mode asks for, and the root's 65-column table, score and
// node count are put together from them (include/az_othello.h has the contract).
//
// Host only.  On the device the same table is composed from the entry points that exist
// (endgame.solve_moves: oth_legal_gpu, oth_step_gpu and oth_solve_deep_gpu unsplit, which
// runs solve_deep.h's step() as this file does, so values, scores and node counts agree bit
// for bit).  A single-call kernel chain for it is not part of this file: see DESIGN.md,
// "Per-move endgame values", left out.
#include <stdexcept>

#include "bitboard.h"
#include "common.h"
#include "solve_deep.h"

static_assert(AZ_MOVES_NONE == azd::kSkipped, "AZ_MOVES_NONE is the skipped code's byte");

namespace {

constexpr int kNone = AZ_MOVES_NONE;

int sign_of(int v) { return (v > 0) - (v < 0); }

// One root: its searches in a fixed order (the root's own first in OPTIMAL mode, then the
// children by ascending action).
void moves_one(uint64_t o, uint64_t p, int max_empties, int mode, uint64_t node_limit,
               int8_t* row, int8_t* score_o, uint64_t* nodes_o) {
  for (int a = 0; a < 65; ++a) row[a] = (int8_t)kNone;
  if ((o & p) != 0 || 64 - azb::popc(o | p) > max_empties) {
    *score_o = (int8_t)azd::kSkipped;
    if (nodes_o) *nodes_o = 0;
    return;
  }
  uint64_t m = azb::legal(o, p);
  const bool pass = !m && azb::legal(p, o) != 0;
  if (!m && !pass) {
    *score_o = (int8_t)(azb::popc(o) - azb::popc(p));
    if (nodes_o) *nodes_o = 1;
    return;
  }
  uint64_t nodes = 1, nd = 0;
  bool ab = false;
  int8_t sc = 0;
  uint8_t best = 0;
  int wa = mode == AZ_MOVES_WLD ? -1 : -azd::kInf, wb = -wa, root = 0;
  if (mode == AZ_MOVES_OPTIMAL) {
    azd::solve_one(o, p, azd::kMaxEmpties, -azd::kInf, azd::kInf, node_limit, &sc, &best, &nd);
    nodes += nd;
    ab = sc == azd::kAborted;
    root = sc;
    wa = -root - 1;
    wb = -root + 1;
  }
  // an aborted child does not stop its siblings (a batched device run searches them all): the
  // node count covers every search, the row goes back to NONE
  int top = kNone;
  bool child_ab = false;
  for (int j = 0; !ab && j < (pass ? 1 : 64); ++j) {
    const int a = pass ? azb::kPass : j;
    if (!pass && !((m >> j) & 1ull)) continue;
    uint64_t co, cp;
    azb::play(o, p, a, pass ? 0ull : azb::flips(o, p, j), &co, &cp);
    azd::solve_one(co, cp, azd::kMaxEmpties, wa, wb, node_limit, &sc, &best, &nd);
    nodes += nd;
    if (sc == azd::kAborted) {
      child_ab = true;
      continue;
    }
    const int v = mode == AZ_MOVES_WLD ? -sign_of(sc) : -sc;
    row[a] = (int8_t)v;
    if (v > top) top = v;
  }
  if (ab || child_ab) {
    for (int a = 0; a < 65; ++a) row[a] = (int8_t)kNone;
    *score_o = (int8_t)azd::kAborted;
  } else {
    *score_o = (int8_t)(mode == AZ_MOVES_OPTIMAL ? root : top);
  }
  if (nodes_o) *nodes_o = nodes;
}

bool mode_ok(int mode) {
  return mode == AZ_MOVES_SCORES || mode == AZ_MOVES_WLD || mode == AZ_MOVES_OPTIMAL;
}

}  // namespace

extern "C" {

int oth_solve_moves_cpu(const uint64_t* own, const uint64_t* opp, int64_t n, int32_t max_empties,
                        int32_t mode, uint64_t node_limit, int8_t* values_o, int8_t* score_o,
                        uint64_t* nodes_o) {
  AZ_REQUIRE(n >= 0, AZ_ERR_ARG, "oth_solve_moves_cpu: n=%lld < 0", (long long)n);
  AZ_REQUIRE(max_empties >= 0 && max_empties <= AZ_SOLVE_DEEP_MAX_EMPTIES, AZ_ERR_ARG,
             "oth_solve_moves_cpu: max_empties=%d outside 0..%d", (int)max_empties,
             AZ_SOLVE_DEEP_MAX_EMPTIES);
  AZ_REQUIRE(mode_ok(mode), AZ_ERR_ARG, "oth_solve_moves_cpu: mode=%d is none of 0, 1, 2",
             (int)mode);
  AZ_REQUIRE(n == 0 || (own && opp && values_o && score_o), AZ_ERR_ARG,
             "oth_solve_moves_cpu: null buffer");
  for (int64_t i = 0; i < n; ++i)
    moves_one(own[i], opp[i], max_empties, mode, node_limit, values_o + i * 65, score_o + i,
              nodes_o ? nodes_o + i : nullptr);
  return AZ_OK;
}

}  // extern "C"
