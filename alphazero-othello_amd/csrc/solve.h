// solve.h — exact endgame search shared by oth_solve_cpu and the k_solve kernel (one source
// of truth, like bitboard.h): an iterative fail-soft negamax alpha-beta written as a
// per-position state machine.  step() advances ONE node of one search: it either makes the
// next move of the top frame (a new node: push a frame, or a terminal leaf whose value is
// handed back) or returns the finished top frame's value to its parent.  No recursion, and
// every loop around step() is bounded by the node limit.
//
// Value = final popcount(own) - popcount(opp) from the side to move's view with both sides
// maximising it; empties go to nobody, a side without a placement passes, the game ends
// when neither side has one (reference envs/othello.py:214-220, 435-457).
//
// Frames.  The top frame lives in registers (Search); the frames below it live in a Stack
// the caller provides (host: a plain array, device: LDS laid out [frame][field][lane]).
// A stored frame is 20 bytes: the capture set and square of the move that led to it (the
// parent's boards are rebuilt from the child's by undoing that move), its untried moves, and
// alpha / beta / best packed in one word.  A position with e empties stacks at most e - 1
// frames (every frame below the top has made a placement), 13 at the cap of 14 empties.
//
// A child without a placement is never a frame of its own: if the mover's opponent cannot
// place either it is a terminal leaf, otherwise the frame pushed is the position after the
// pass (the parent's side to move again, `sign` = 1: its value goes to the parent without
// the negation, its window is the parent's).
//
// Move order: the root tries its placements in ascending square order and keeps the first
// that strictly improves, so `best` is the lowest square that achieves the score.  Interior
// nodes only return values; they try corners first, then ascending.
#pragma once
#include "bitboard.h"

namespace azs {

constexpr int kSkipped = -128;   // AZ_SOLVE_SKIPPED
constexpr int kAborted = -127;   // AZ_SOLVE_ABORTED
constexpr int kMaxEmpties = 14;  // AZ_SOLVE_MAX_EMPTIES
constexpr int kMaxFrames = kMaxEmpties - 1;
constexpr int kInf = 65;  // outside every value (|value| <= 64)
constexpr uint64_t kCorners = 0x8100000000000081ull;

enum : int { kRun = 0, kDone = 1 };

struct Search {
  uint64_t own, opp;  // top frame: side to move, its opponent
  uint64_t moves;     // top frame: placements not tried yet
  uint64_t flips;     // capture set of the move that led to the top frame
  uint64_t nodes;     // nodes visited so far
  int alpha, beta, best;  // top frame's window (alpha already raised to best) and value so far
  int sq, sign;       // square of the move that led here; 1 = reached through a pass as well
  int sp;             // frames on the stack below the top frame
  int ret, ret_sq, pending;  // a child's value (parent's view) waiting to be taken
  int state;          // kRun / kDone
  int root_pass;      // the root itself had to pass: the top-level frame is the opponent's
  int score, root_best;  // results once state == kDone
};

AZ_HD uint32_t pack_frame(const Search& s) {
  return (uint32_t)(s.alpha + kInf) | ((uint32_t)(s.beta + kInf) << 8) |
         ((uint32_t)(s.best + kInf) << 16) | ((uint32_t)(s.sq | (s.sign << 6)) << 24);
}

AZ_HD void unpack_frame(Search& s, uint32_t w) {
  s.alpha = (int)(w & 0xFF) - kInf;
  s.beta = (int)((w >> 8) & 0xFF) - kInf;
  s.best = (int)((w >> 16) & 0xFF) - kInf;
  s.sq = (int)((w >> 24) & 63);
  s.sign = (int)((w >> 30) & 1);
}

// the host's frame stack (the device's is in solve.hip)
struct HostStack {
  uint64_t w[kMaxFrames][2];
  uint32_t p[kMaxFrames];
  AZ_HD void put(int f, uint64_t flips, uint64_t moves, uint32_t pk) {
    w[f][0] = flips;
    w[f][1] = moves;
    p[f] = pk;
  }
  AZ_HD void get(int f, uint64_t& flips, uint64_t& moves, uint32_t& pk) const {
    flips = w[f][0];
    moves = w[f][1];
    pk = p[f];
  }
};

AZ_HD void finish(Search& s, int score, int best) {
  s.state = kDone;
  s.score = score;
  s.root_best = best;
}

// Start the search of one position.  Positions that are not searched (more than
// max_empties empties, overlapping boards) and terminal roots finish here.
AZ_HD void init(Search& s, uint64_t own, uint64_t opp, int max_empties) {
  s.own = own;
  s.opp = opp;
  s.moves = 0;
  s.flips = 0;
  s.nodes = 0;
  s.alpha = -kInf;
  s.beta = kInf;
  s.best = -kInf;
  s.sq = 0;
  s.sign = 0;
  s.sp = 0;
  s.ret = 0;
  s.ret_sq = 0;
  s.pending = 0;
  s.root_pass = 0;
  s.state = kRun;
  s.score = 0;
  s.root_best = azb::kPass;
  if ((own & opp) != 0 || 64 - azb::popc(own | opp) > max_empties) {
    finish(s, kSkipped, 255);
    return;
  }
  s.nodes = 1;
  uint64_t m = azb::legal(own, opp);
  if (!m) {
    m = azb::legal(opp, own);
    if (!m) {
      finish(s, azb::popc(own) - azb::popc(opp), azb::kPass);
      return;
    }
    s.own = opp;  // the root passes: search the opponent's position, negate at the end
    s.opp = own;
    s.root_pass = 1;
    s.nodes = 2;
  }
  s.moves = m;
}

// Advance one node.  max_frames = the stack's capacity (a full stack aborts the search
// instead of writing past it; unreachable for max_empties <= max_frames + 1).
template <class Stack>
AZ_HD void step(Search& s, Stack& st, uint64_t node_limit, int max_frames) {
  if (s.pending) {  // the value of the move tried last
    s.pending = 0;
    if (s.ret > s.best) {
      s.best = s.ret;
      if (s.sp == 0) s.root_best = s.ret_sq;
      if (s.best > s.alpha) s.alpha = s.best;
      if (s.best >= s.beta) s.moves = 0;
    }
  }
  if (s.moves == 0) {  // this frame is finished: hand its value to the parent
    if (s.sp == 0) {
      finish(s, s.root_pass ? -s.best : s.best, s.root_pass ? azb::kPass : s.root_best);
      return;
    }
    // undo the move: child boards are (opp ^ f, (own | bit) ^ f), swapped after a pass
    const uint64_t bit = 1ull << s.sq;
    const uint64_t mover = s.sign ? s.own : s.opp;
    const uint64_t other = s.sign ? s.opp : s.own;
    s.ret = s.sign ? s.best : -s.best;
    s.ret_sq = s.sq;
    s.pending = 1;
    s.own = (mover ^ s.flips) & ~bit;
    s.opp = other ^ s.flips;
    --s.sp;
    uint32_t pk;
    st.get(s.sp, s.flips, s.moves, pk);
    unpack_frame(s, pk);
    return;
  }
  // the next move of this frame
  uint64_t m = s.moves;
  if (s.sp > 0 && (m & kCorners)) m &= kCorners;
  const int sq = __builtin_ctzll(m);
  const uint64_t bit = 1ull << sq;
  s.moves &= ~bit;
  if (++s.nodes > node_limit) {
    finish(s, kAborted, 255);
    return;
  }
  const uint64_t f = azb::flips(s.own, s.opp, sq);
  uint64_t cown = s.opp ^ f, copp = (s.own | bit) ^ f;
  const bool full = (cown | copp) == ~0ull;
  uint64_t cm = full ? 0ull : azb::legal(cown, copp);
  int sign = 0;
  if (!cm) {
    cm = full ? 0ull : azb::legal(copp, cown);
    if (!cm) {  // the game ended with this move
      s.ret = azb::popc(copp) - azb::popc(cown);
      s.ret_sq = sq;
      s.pending = 1;
      return;
    }
    const uint64_t t = cown;  // the opponent passes: the mover's side again
    cown = copp;
    copp = t;
    sign = 1;
    ++s.nodes;
  }
  if (s.sp >= max_frames) {
    finish(s, kAborted, 255);
    return;
  }
  st.put(s.sp, s.flips, s.moves, pack_frame(s));
  ++s.sp;
  const int a = s.alpha, b = s.beta;
  s.alpha = sign ? a : -b;
  s.beta = sign ? b : -a;
  s.best = -kInf;
  s.own = cown;
  s.opp = copp;
  s.moves = cm;
  s.flips = f;
  s.sq = sq;
  s.sign = sign;
}

// One whole search on the host.
inline void solve_one(uint64_t own, uint64_t opp, int max_empties, uint64_t node_limit,
                      int8_t* score, uint8_t* best, uint64_t* nodes) {
  Search s;
  HostStack st;
  init(s, own, opp, max_empties);
  while (s.state == kRun) step(s, st, node_limit, kMaxFrames);
  *score = (int8_t)s.score;
  *best = (uint8_t)s.root_best;
  if (nodes) *nodes = s.nodes;
}

}  // namespace azs
