// line_step.h — one ply of the optimal line of a solved root (endgame.optimal_line): from the
// root's solve_moves table (mode OPTIMAL) and score, write the ply's training row, play the
// lowest score-optimal action and say whether the game goes on.  One body for the device kernel
// and its host mirror (csrc/line_step.hip), so the two agree bit for bit.
#pragma once
#include "../../include/az_othello.h"
#include "bitboard.h"

namespace azl {

constexpr int kNone = AZ_MOVES_NONE;
constexpr int kSkipped = AZ_SOLVE_SKIPPED, kAborted = AZ_SOLVE_ABORTED;
// the boards of a retired root: own & opp != 0, which every solver skips without a node
constexpr uint64_t kRetired = ~0ull;

struct Line {          // SoA over the n roots of a call
  uint64_t* own;       // [n] current position, side to move first (in / out)
  uint64_t* opp;
  const int8_t* values;  // [n, 65] this ply's solve_moves table
  const int8_t* score;   // [n] this ply's score (or a skipped / aborted code)
  int32_t* count;      // [n] rows written so far (in / out)
  uint8_t* done;       // [n] 1 = the line is complete (in / out)
  int8_t* root_score;  // [n] written on the first ply; kAborted if a later ply aborts
  uint64_t* row_own;   // [n, stride]
  uint64_t* row_opp;
  float* row_pi;       // [n, stride, 65]
  uint8_t* row_act;    // [n, stride]
  float* row_z;        // [n, stride]
  int32_t stride;
  int32_t first;       // this is the roots' first ply
};

// Root i's ply.  Returns 1 when the root needs another ply.
AZ_HD int line_step_one(const Line& L, int64_t i) {
  if (L.done[i]) return 0;
  const int s = L.score[i];
  const int8_t* v = L.values + i * 65;
  if (L.first) L.root_score[i] = (int8_t)s;
  int top = kNone, hits = 0, act = -1;
  for (int a = 0; a < 65; ++a) {
    const int x = v[a];
    if (x == kNone) continue;
    if (x > top) {
      top = x;
      hits = 1;
      act = a;
    } else if (x == top) {
      ++hits;
    }
  }
  const int cnt = L.count[i];
  const bool room = (uint32_t)cnt < (uint32_t)L.stride;
  bool stop = s == kSkipped || s == kAborted || act < 0 || !room;
  if (s == kAborted || (act >= 0 && !room)) {
    // an aborted search at any ply (or a line longer than the caller's rows, which the stride
    // 2 * max_empties rules out) leaves no partial line behind
    L.root_score[i] = (int8_t)kAborted;
    L.count[i] = 0;
  }
  if (!stop) {
    const int64_t r = i * (int64_t)L.stride + cnt;
    const uint64_t o = L.own[i], p = L.opp[i];
    // exact_policy's float32(1 / hits): one correctly rounded float64 division, narrowed
    const float w = (float)(1.0 / (double)hits);
    float* pi = L.row_pi + r * 65;
    for (int a = 0; a < 65; ++a) pi[a] = (v[a] == top && v[a] != kNone) ? w : 0.0f;
    L.row_own[r] = o;
    L.row_opp[r] = p;
    L.row_act[r] = (uint8_t)act;
    L.row_z[r] = (float)((s > 0) - (s < 0));
    L.count[i] = cnt + 1;
    uint64_t no, np;
    azb::play(o, p, act, act == azb::kPass ? 0ull : azb::flips(o, p, act), &no, &np);
    stop = azb::legal(no, np) == 0 && azb::legal(np, no) == 0;
    L.own[i] = no;
    L.opp[i] = np;
  }
  if (stop) {
    L.done[i] = 1;
    L.own[i] = kRetired;
    L.opp[i] = kRetired;
  }
  return stop ? 0 : 1;
}

}  // namespace azl
