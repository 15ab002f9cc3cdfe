// solve_deep.h — windowed, move-ordered endgame search shared by oth_solve_deep_cpu and the
// k_solve_deep kernel.  The same shape as solve.h (an iterative fail-soft negamax written as
// a per-position state machine, the top frame in registers, the frames below it in a stack
// the caller provides, no recursion, every loop around step() bounded by the node limit);
// new are a root window and an ordering of the moves.  solve.h's search is untouched: its
// lowest-square `best` and its node counts are pinned by tests.
//
// Window.  The root is searched in (alpha, beta), -65 <= alpha < beta <= 65.  With s the true
// score the result v is: v = s if alpha < s < beta; beta <= v <= s if s >= beta;
// s <= v <= alpha if s <= alpha (fail-soft).  (-65, 65) is the full window, (-1, 1) gives the
// exact win / draw / loss as sign(v).
//
// Order.  A node with at least kOrderMin empties and more than one placement first probes
// every placement: key = 2 * (placements the opponent has after it) + (0 for a corner, else
// 1).  The ten lowest keys are kept, in order (ties: the lower square first), as 6-bit
// squares in one 64-bit word with their count in bits 60..63; moves beyond ten follow from
// the untried mask, corners first, then ascending, which is also the whole order of the
// nodes below kOrderMin (solve.h's order).  One step() first returns the top frame's value to its
// parent if that frame is finished, then makes one probe or one move, so the lanes of a
// wave spend a step on the same flips + legal pair whether they probe or move, and a value
// on its way up costs no step of its own.  Probes are not nodes.
//
// kOrderMin = 5.  Total nodes over the 605 corpus positions with 12 empties, full window /
// (-1, 1), in millions (solve.h: 193.8), and the hardest root's in the full window:
//   kOrderMin 3: 24.3 / 2.46, 0.46   4: 25.2 / 2.55, 0.48   5: 27.0 / 2.81, 0.55
//             6: 30.7 / 3.31, 0.62   7: 35.2 / 3.94, 0.84   8: 43.4 / 5.13, 0.93
// One host thread needs 2.2..2.8 s for the full-window set at every threshold from 4 to 7
// (3.3 s at 3): the probes that a lower threshold adds cost what the nodes it saves did.
// Below 5 the node count hardly falls any more (10 % from 5 to 3) while every node near
// the leaves, where almost all nodes are, starts with its probes; above 5 the hardest root,
// which is the device's tail, grows.  So 5.
//
// Frames are solve.h's plus the order word: 28 bytes.  A position with e empties stacks at
// most e - 1 frames, 19 at the cap of 20 empties.  The probe state (squares still to probe,
// the keys of the kept squares) is never stacked: a node finishes probing before its first
// move is made.
//
// best: the move that last raised the root's value.  If alpha < v < beta it is an optimal
// action (not necessarily the lowest); if v >= beta its value is >= beta; if v <= alpha it
// is merely legal.  64 when the side to move has no placement.
#pragma once
#include "bitboard.h"

namespace azd {

constexpr int kSkipped = -128;   // AZ_SOLVE_SKIPPED
constexpr int kAborted = -127;   // AZ_SOLVE_ABORTED
constexpr int kMaxEmpties = 20;  // AZ_SOLVE_DEEP_MAX_EMPTIES
constexpr int kMaxFrames = kMaxEmpties - 1;
constexpr int kInf = 65;  // outside every value (|value| <= 64)
constexpr int kOrderMin = 5;
constexpr int kOrderSlots = 10;
constexpr uint64_t kCorners = 0x8100000000000081ull;
constexpr uint64_t kNoKeys = 0x0FFFFFFFFFFFFFFFull;  // ten empty slots: key 63 each

enum : int { kRun = 0, kDone = 1 };

struct Search {
  uint64_t own, opp;  // top frame: side to move, its opponent
  uint64_t moves;     // top frame: placements not tried yet
  uint64_t order;     // top frame: ordered squares not tried yet (6 bits each, count in 60..63)
  uint64_t flips;     // capture set of the move that led to the top frame
  uint64_t probe;     // top frame: placements still to probe for the order (not stacked)
  uint64_t keys;      // keys of the squares in `order` while probing (not stacked)
  uint64_t nodes;     // nodes visited so far
  int alpha, beta, best;  // top frame's window (alpha already raised to best) and value so far
  int sq, sign;       // square of the move that led here; 1 = reached through a pass as well
  int sp;             // frames on the stack below the top frame
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

// the host's frame stack (the device's is in solve_deep.hip)
struct HostStack {
  uint64_t w[kMaxFrames][3];
  uint32_t p[kMaxFrames];
  AZ_HD void put(int f, uint64_t flips, uint64_t moves, uint64_t order, uint32_t pk) {
    w[f][0] = flips;
    w[f][1] = moves;
    w[f][2] = order;
    p[f] = pk;
  }
  AZ_HD void get(int f, uint64_t& flips, uint64_t& moves, uint64_t& order, uint32_t& pk) const {
    flips = w[f][0];
    moves = w[f][1];
    order = w[f][2];
    pk = p[f];
  }
};

AZ_HD void finish(Search& s, int score, int best) {
  s.state = kDone;
  s.score = score;
  s.root_best = best;
}

// A frame with placements m starts: decide whether its moves are probed first.
AZ_HD void start_frame(Search& s, uint64_t m) {
  s.moves = m;
  s.order = 0;
  s.keys = kNoKeys;
  const bool ordered = 64 - azb::popc(s.own | s.opp) >= kOrderMin && (m & (m - 1)) != 0;
  s.probe = ordered ? m : 0ull;
}

// Insert square sq with key k (0..62) into the kept squares: behind every key <= k.
AZ_HD void order_insert(Search& s, int sq, int k) {
  int pos = 0;
#pragma unroll
  for (int i = 0; i < kOrderSlots; ++i) pos += (int)((s.keys >> (6 * i)) & 63) <= k;
  if (pos >= kOrderSlots) return;  // beyond the ten kept: stays in the untried mask only
  const uint64_t cnt = s.order >> 60;
  const uint64_t lo = (1ull << (6 * pos)) - 1, body = (1ull << 60) - 1;
  const uint64_t o = s.order & body;
  s.order = (((o & lo) | ((uint64_t)sq << (6 * pos)) | ((o & ~lo) << 6)) & body) |
            ((cnt < kOrderSlots ? cnt + 1 : cnt) << 60);
  s.keys = ((s.keys & lo) | ((uint64_t)k << (6 * pos)) | ((s.keys & ~lo) << 6)) & body;
}

// Start the search of one position in the window (alpha, beta).  Positions that are not
// searched (more than max_empties empties, overlapping boards) and terminal roots finish
// here.
AZ_HD void init(Search& s, uint64_t own, uint64_t opp, int max_empties, int alpha, int beta) {
  s.own = own;
  s.opp = opp;
  s.moves = 0;
  s.order = 0;
  s.flips = 0;
  s.probe = 0;
  s.keys = kNoKeys;
  s.nodes = 0;
  s.alpha = alpha;
  s.beta = beta;
  s.best = -kInf;
  s.sq = 0;
  s.sign = 0;
  s.sp = 0;
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
    s.alpha = -beta;
    s.beta = -alpha;
    s.root_pass = 1;
    s.nodes = 2;
  }
  start_frame(s, m);
}

// Take the value `ret` of the move `sq` just tried into the top frame.
AZ_HD void take(Search& s, int ret, int sq) {
  if (ret > s.best) {
    s.best = ret;
    if (s.sp == 0) s.root_best = sq;
    if (s.best > s.alpha) s.alpha = s.best;
    if (s.best >= s.beta) s.moves = 0;
  }
}

// Advance one step: a finished frame's value handed to its parent, then a probe or a move
// (a new node).  max_frames = the stack's capacity (a full stack aborts the search instead of
// writing past it; unreachable for max_empties <= max_frames + 1).
template <class Stack>
AZ_HD void step(Search& s, Stack& st, uint64_t node_limit, int max_frames) {
  if (s.moves == 0) {  // this frame is finished: hand its value to the parent
    if (s.sp == 0) {
      finish(s, s.root_pass ? -s.best : s.best, s.root_pass ? azb::kPass : s.root_best);
      return;
    }
    // undo the move: child boards are (opp ^ f, (own | bit) ^ f), swapped after a pass
    const int sq = s.sq;
    const uint64_t bit = 1ull << sq;
    const uint64_t mover = s.sign ? s.own : s.opp;
    const uint64_t other = s.sign ? s.opp : s.own;
    const int ret = s.sign ? s.best : -s.best;
    s.own = (mover ^ s.flips) & ~bit;
    s.opp = other ^ s.flips;
    --s.sp;
    uint32_t pk;
    st.get(s.sp, s.flips, s.moves, s.order, pk);
    unpack_frame(s, pk);
    take(s, ret, sq);
    if (s.moves == 0) return;  // the parent is finished as well: the next step's work
  }
  // the square of this step: the next probe, else the next move of this frame
  const bool probing = s.probe != 0;
  int sq;
  if (probing) {
    sq = __builtin_ctzll(s.probe);
  } else if (s.order >> 60) {
    sq = (int)(s.order & 63);
  } else {
    uint64_t m = s.moves;
    if (m & kCorners) m &= kCorners;
    sq = __builtin_ctzll(m);
  }
  const uint64_t bit = 1ull << sq;
  const uint64_t f = azb::flips(s.own, s.opp, sq);
  uint64_t cown = s.opp ^ f, copp = (s.own | bit) ^ f;
  const bool full = (cown | copp) == ~0ull;
  uint64_t cm = full ? 0ull : azb::legal(cown, copp);
  if (probing) {
    s.probe &= ~bit;
    order_insert(s, sq, 2 * azb::popc(cm) + ((bit & kCorners) ? 0 : 1));
    return;
  }
  if (s.order >> 60) s.order = ((s.order & ((1ull << 60) - 1)) >> 6) | (((s.order >> 60) - 1) << 60);
  s.moves &= ~bit;
  if (++s.nodes > node_limit) {
    finish(s, kAborted, 255);
    return;
  }
  int sign = 0;
  if (!cm) {
    cm = full ? 0ull : azb::legal(copp, cown);
    if (!cm) {  // the game ended with this move
      take(s, azb::popc(copp) - azb::popc(cown), sq);
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
  st.put(s.sp, s.flips, s.moves, s.order, pack_frame(s));
  ++s.sp;
  const int a = s.alpha, b = s.beta;
  s.alpha = sign ? a : -b;
  s.beta = sign ? b : -a;
  s.best = -kInf;
  s.own = cown;
  s.opp = copp;
  s.flips = f;
  s.sq = sq;
  s.sign = sign;
  start_frame(s, cm);
}

// One whole search on the host.
inline void solve_one(uint64_t own, uint64_t opp, int max_empties, int alpha, int beta,
                      uint64_t node_limit, int8_t* score, uint8_t* best, uint64_t* nodes) {
  Search s;
  HostStack st;
  init(s, own, opp, max_empties, alpha, beta);
  while (s.state == kRun) step(s, st, node_limit, kMaxFrames);
  *score = (int8_t)s.score;
  *best = (uint8_t)s.root_best;
  if (nodes) *nodes = s.nodes;
}

}  // namespace azd
