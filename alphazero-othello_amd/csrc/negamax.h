// negamax.h — the rules the three tree searches share (solve.h, search.h, solve_deep.h), each
// defined once: an iterative fail-soft negamax written as a per-position state machine, the
// top frame in registers and the frames below it in a stack the caller provides.  A search's
// step() in its own header names these pieces in order and adds what is its own (the horizon,
// the move order, how a value travels up).  Nothing here recurses and no rule loops; run_host
// is the one loop, bounded by the node limit.
//
// The game.  Value = the side to move's result with both sides maximising it; a side without a
// placement passes, the game ends when neither side has one.  A child without a placement is
// never a frame of its own: if the mover cannot place either, the game ended with the move
// (a leaf whose value goes straight to the parent), otherwise the child is the position after
// the pass: the mover's side again, `sign` = 1, its value reaches the parent without the
// negation and its window is the parent's.
//
// Nodes.  The root counts 1, or 2 when it has to pass; every move made counts 1, every pass
// below the root 1 more.  The limit is tested where a move is counted and nowhere else; a
// search over the limit, or one whose stack is full, ends with the caller's aborted code and
// best 255.  Roots that are not searched count no node and report best 255 as well.
#pragma once
#include "bitboard.h"

namespace azn {

constexpr int kRun = 0, kDone = 1;  // Frame::state
constexpr int kInf = 65;            // outside every disc difference (|d| <= 64)
constexpr uint64_t kCorners = 0x8100000000000081ull;

// The top frame and the search's totals: what every search keeps in registers.
struct Frame {
  uint64_t own, opp;  // top frame: side to move, its opponent
  uint64_t moves;     // top frame: placements not tried yet
  uint64_t flips;     // capture set of the move that led to the top frame
  uint64_t nodes;     // nodes visited so far
  int alpha, beta, best;  // top frame's window (alpha already raised to best) and value so far
  int sq, sign;       // square of the move that led here; 1 = reached through a pass as well
  int sp;             // frames on the stack below the top frame
  int state;          // kRun / kDone
  int root_pass;      // the root itself had to pass: the top-level frame is the opponent's
  int score, root_best;  // results once state == kDone (search.h: score = its value)
};

// A Frame whose children's values wait one step before they are taken (solve.h, search.h):
// a value on its way up costs a step of its own.
struct WaitingFrame : Frame {
  int ret, ret_sq, pending;  // a child's value (parent's view) waiting to be taken
};

// The position after a move of the top frame's side, from the view of the side to move there.
struct Child {
  uint64_t own, opp, moves, flips;
  int sq, sign;
};

AZ_HD void finish(Frame& s, int score, int best) {
  s.state = kDone;
  s.score = score;
  s.root_best = best;
}

// The top frame is the root's and has no move left: the search's result.
AZ_HD void finish_root(Frame& s) {
  finish(s, s.root_pass ? -s.best : s.best, s.root_pass ? azb::kPass : s.root_best);
}

// Start the search of one position in (alpha, beta), values bounded by inf.  Returns the
// root's placements, or 0 when the search finished here: `skip` ends it with the code
// `skipped`, no node and best 255; a terminal root ends it with `terminal`, its value.  A root
// that passes becomes the opponent's position in the negated window, negated back at the end.
AZ_HD uint64_t start(Frame& s, uint64_t own, uint64_t opp, int alpha, int beta, int inf,
                     bool skip, int skipped, int terminal) {
  s.own = own;
  s.opp = opp;
  s.moves = 0;
  s.flips = 0;
  s.nodes = 0;
  s.alpha = alpha;
  s.beta = beta;
  s.best = -inf;
  s.sq = 0;
  s.sign = 0;
  s.sp = 0;
  s.root_pass = 0;
  s.state = kRun;
  s.score = 0;
  s.root_best = azb::kPass;
  if (skip) {
    finish(s, skipped, 255);
    return 0;
  }
  s.nodes = 1;
  uint64_t m = azb::legal(own, opp);
  if (!m) {
    m = azb::legal(opp, own);
    if (!m) {
      finish(s, terminal, azb::kPass);
      return 0;
    }
    s.own = opp;
    s.opp = own;
    s.alpha = -beta;
    s.beta = -alpha;
    s.root_pass = 1;
    s.nodes = 2;
  }
  return m;
}

AZ_HD void start(WaitingFrame& s, uint64_t own, uint64_t opp, int inf, bool skip, int skipped,
                 int terminal) {
  s.ret = 0;
  s.ret_sq = 0;
  s.pending = 0;
  s.moves = start(static_cast<Frame&>(s), own, opp, -inf, inf, inf, skip, skipped, terminal);
}

// Take the value `ret` of the move `sq` just tried into the top frame: strict improvements
// only, the root remembers the move, a value at or above beta ends the frame.
AZ_HD void take(Frame& s, int ret, int sq) {
  if (ret > s.best) {
    s.best = ret;
    if (s.sp == 0) s.root_best = sq;
    if (s.best > s.alpha) s.alpha = s.best;
    if (s.best >= s.beta) s.moves = 0;
  }
}

// The same through the waiting slot: hand() leaves a value, the next step takes it.
AZ_HD void hand(WaitingFrame& s, int ret, int sq) {
  s.ret = ret;
  s.ret_sq = sq;
  s.pending = 1;
}

AZ_HD void take_handed(WaitingFrame& s) {
  if (s.pending) {
    s.pending = 0;
    take(s, s.ret, s.ret_sq);
  }
}

// The finished top frame's value from its parent's view, with the move that led to it undone:
// child boards are (opp ^ f, (own | bit) ^ f), swapped after a pass.  Pops the frame count; the
// caller reloads the parent's fields from its stack (s.sq is still the move's until then).
AZ_HD int undo(Frame& s) {
  const uint64_t bit = 1ull << s.sq;
  const uint64_t mover = s.sign ? s.own : s.opp;
  const uint64_t other = s.sign ? s.opp : s.own;
  s.own = (mover ^ s.flips) & ~bit;
  s.opp = other ^ s.flips;
  --s.sp;
  return s.sign ? s.best : -s.best;
}

// The next untried placement: corners first where `corners` says so, then ascending.
AZ_HD int pick(uint64_t moves, bool corners) {
  if (corners && (moves & kCorners)) moves &= kCorners;
  return __builtin_ctzll(moves);
}

// Count the move sq of the top frame as made.  False: the node limit is passed, the search has
// ended with `aborted`.
AZ_HD bool count_move(Frame& s, int sq, uint64_t node_limit, int aborted) {
  s.moves &= ~(1ull << sq);
  if (++s.nodes > node_limit) {
    finish(s, aborted, 255);
    return false;
  }
  return true;
}

// The child of the move sq and its placements.  full_is_end: a full board has no placement, so
// legal() is not asked (the solvers, most of whose leaves are full boards; search.h, which hardly
// meets one, goes without the test).
AZ_HD Child make_child(const Frame& s, int sq, bool full_is_end) {
  Child c;
  c.flips = azb::flips(s.own, s.opp, sq);
  c.own = s.opp ^ c.flips;
  c.opp = (s.own | (1ull << sq)) ^ c.flips;
  c.moves = full_is_end && (c.own | c.opp) == ~0ull ? 0ull : azb::legal(c.own, c.opp);
  c.sq = sq;
  c.sign = 0;
  return c;
}

// The mover's own placements in the child: with none on either side the game ended with the
// move, and final_diff is its result from the mover's view.
AZ_HD uint64_t mover_moves(const Child& c, bool full_is_end) {
  return full_is_end && (c.own | c.opp) == ~0ull ? 0ull : azb::legal(c.opp, c.own);
}
AZ_HD int final_diff(const Child& c) { return azb::popc(c.opp) - azb::popc(c.own); }

// The child's side has no placement but the mover has (c.moves holds the mover's by now): the
// opponent passes, the child is the mover's side again, and the pass is a node.
AZ_HD void pass(Frame& s, Child& c) {
  const uint64_t t = c.own;
  c.own = c.opp;
  c.opp = t;
  c.sign = 1;
  ++s.nodes;
}

// Room for one more frame below the top.  False: the stack is full (unreachable while the cap
// on empties or depth is at most max_frames + 1), the search has ended with `aborted`.
AZ_HD bool room(Frame& s, int max_frames, int aborted) {
  if (s.sp < max_frames) return true;
  finish(s, aborted, 255);
  return false;
}

// The child becomes the top frame (the caller has stored the old one at s.sp): the window
// negated and swapped, or kept after a pass.
AZ_HD void enter(Frame& s, const Child& c, int inf) {
  ++s.sp;
  const int a = s.alpha, b = s.beta;
  s.alpha = c.sign ? a : -b;
  s.beta = c.sign ? b : -a;
  s.best = -inf;
  s.own = c.own;
  s.opp = c.opp;
  s.moves = c.moves;
  s.flips = c.flips;
  s.sq = c.sq;
  s.sign = c.sign;
}

// The stored frame's small fields in one word, for values within kInf (solve.h, solve_deep.h).
AZ_HD uint32_t pack_frame(const Frame& s) {
  return (uint32_t)(s.alpha + kInf) | ((uint32_t)(s.beta + kInf) << 8) |
         ((uint32_t)(s.best + kInf) << 16) | ((uint32_t)(s.sq | (s.sign << 6)) << 24);
}

AZ_HD void unpack_frame(Frame& s, uint32_t w) {
  s.alpha = (int)(w & 0xFF) - kInf;
  s.beta = (int)((w >> 8) & 0xFF) - kInf;
  s.best = (int)((w >> 16) & 0xFF) - kInf;
  s.sq = (int)((w >> 24) & 63);
  s.sign = (int)((w >> 30) & 1);
}

// One whole search on the host, from a started Search to its results.  step is the one of the
// Search's namespace.
template <class Stack, class Search, class Value>
inline void run_host(Search& s, uint64_t node_limit, int frames, Value* value, uint8_t* best,
                     uint64_t* nodes) {
  Stack st;
  while (s.state == kRun) step(s, st, node_limit, frames);
  *value = (Value)s.score;
  *best = (uint8_t)s.root_best;
  if (nodes) *nodes = s.nodes;
}

}  // namespace azn
