// records.h — replay of one recorded game into training rows, shared by oth_records_cpu and
// the k_records kernel (one source of truth, like solve.h): process_game of the reference
// (supervised_benchmark.py:179-223) on bitboards, with the side to move tracked by the rules
// instead of by alternation.
//
// A game is a small state machine: entry() consumes ONE transcript entry (a placement, a
// pass or the end mark), finish() settles the status of a line that ran out.  The caller owns
// the loop over the entries (host: a plain loop over the bytes; device: a loop bounded by the
// wavefront's longest game over bytes held in registers) and the Sink that stores a row.
//
// Legality costs one flips() per placement: a placement is legal iff its square is empty and
// it captures something.  The legal-move fill runs only when that fails (is this an omitted
// pass, or an illegal entry?), for a written pass, and once at the end of the line.
//
// The colour of every emitted row is kept in a 128-bit mask: z = winner x colour can only be
// written once the game is over (without a given winner it is the sign of the final disc
// difference), by z_of() for each row.
#pragma once
#include "bitboard.h"

namespace azr {

constexpr int kRunning = -1;
constexpr int kTerminal = 0, kUnfinished = 1, kIllegal = 2, kOverflow = 3;  // AZ_REC_*
constexpr int kPassRows = 1;                                                // AZ_REC_PASS_ROWS
constexpr int kEnd = 255;
constexpr int kMaxStride = 128, kMaxRows = 128;

struct Game {
  uint64_t own, opp;    // side to move, its opponent
  uint64_t neg0, neg1;  // bit r set: row r was emitted with colour -1
  int colour;           // side to move, +1 = the first mover
  int rows;             // rows emitted
  int extra;            // forced passes inserted so far (ply = entry index + extra)
  int status;           // kRunning, or the AZ_REC_* status
  int bad;              // entry index that stopped the game, 255 = none
};

AZ_HD void init(Game& g, uint64_t own, uint64_t opp) {
  g.own = own;
  g.opp = opp;
  g.neg0 = g.neg1 = 0;
  g.colour = 1;
  g.rows = 0;
  g.extra = 0;
  g.status = kRunning;
  g.bad = 255;
}

AZ_HD void stop(Game& g, int status, int i) {
  g.status = status;
  g.bad = i;
}

AZ_HD void swap_sides(Game& g) {
  const uint64_t t = g.own;
  g.own = g.opp;
  g.opp = t;
  g.colour = -g.colour;
}

// Emit the row (own, opp, act) of the side to move; false (and the game stopped) when it
// would be row max_rows.
template <class Sink>
AZ_HD bool emit(Game& g, int i, int act, int max_rows, Sink& out) {
  if (g.rows >= max_rows) {
    stop(g, kOverflow, i);
    return false;
  }
  const uint64_t bit = (g.colour < 0 ? 1ull : 0ull) << (g.rows & 63);
  if (g.rows < 64)
    g.neg0 |= bit;
  else
    g.neg1 |= bit;
  out.row(g.rows, g.own, g.opp, act, i + g.extra);
  ++g.rows;
  return true;
}

// The line is over (end mark, or stride entries consumed): terminal or unfinished.
AZ_HD void finish(Game& g) {
  if (g.status != kRunning) return;
  const bool full = (g.own | g.opp) == ~0ull;
  const bool any = !full && (azb::legal(g.own, g.opp) != 0 || azb::legal(g.opp, g.own) != 0);
  g.status = any ? kUnfinished : kTerminal;
}

// Entry i of the transcript (a in 0..255) for a running game.
template <class Sink>
AZ_HD void entry(Game& g, int i, int a, int flags, int max_rows, Sink& out) {
  if (a == kEnd) {
    finish(g);
    return;
  }
  if (a > azb::kPass) {
    stop(g, kIllegal, i);
    return;
  }
  if (a == azb::kPass) {  // a written pass: the mover has no placement, the opponent has one
    if (azb::legal(g.own, g.opp) != 0 || azb::legal(g.opp, g.own) == 0) {
      stop(g, kIllegal, i);
      return;
    }
    if ((flags & kPassRows) && !emit(g, i, azb::kPass, max_rows, out)) return;
    swap_sides(g);
    return;
  }
  const uint64_t bit = 1ull << a;
  if ((g.own | g.opp) & bit) {  // occupied for either side: no pass makes it legal
    stop(g, kIllegal, i);
    return;
  }
  uint64_t f = azb::flips(g.own, g.opp, a);
  if (f == 0) {
    // not a placement of the mover.  An omitted pass: the mover has none at all and a is one
    // of the opponent's (which then has one); anything else is illegal (a terminal position
    // included).
    const uint64_t fo = azb::flips(g.opp, g.own, a);
    if (fo == 0 || azb::legal(g.own, g.opp) != 0) {
      stop(g, kIllegal, i);
      return;
    }
    if ((flags & kPassRows) && !emit(g, i, azb::kPass, max_rows, out)) return;
    swap_sides(g);
    ++g.extra;
    f = fo;
  }
  if (!emit(g, i, a, max_rows, out)) return;
  const uint64_t nown = g.opp ^ f, nopp = (g.own | bit) ^ f;
  g.own = nown;
  g.opp = nopp;
  g.colour = -g.colour;
}

// disc difference of the final position from the first mover's view
AZ_HD int final_diff(const Game& g) {
  return g.colour * (azb::popc(g.own) - azb::popc(g.opp));
}

// the outcome the rows are labelled with, from the first mover's view
AZ_HD int outcome(const Game& g, const int8_t* winner_or_null, int64_t game) {
  if (winner_or_null) return winner_or_null[game];
  if (g.status != kTerminal) return 0;
  const int d = final_diff(g);
  return d > 0 ? 1 : (d < 0 ? -1 : 0);
}

AZ_HD int z_of(const Game& g, int r, int w) {
  const uint64_t m = r < 64 ? g.neg0 : g.neg1;
  return ((m >> (r & 63)) & 1ull) ? -w : w;
}

}  // namespace azr
