// solve.h — exact endgame search shared by oth_solve_cpu and the k_solve kernel (one source
// of truth, like bitboard.h): an iterative fail-soft negamax alpha-beta written as a
// per-position state machine out of negamax.h's pieces (the pass, end-of-game and node
// rules, the window, the frame word).  step() advances ONE node of one search: it either
// makes the next move of the top frame (a new node: push a frame, or a terminal leaf whose
// value is handed back) or returns the finished top frame's value to its parent.  No
// recursion, and every loop around step() is bounded by the node limit.
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
// Move order: the root tries its placements in ascending square order and keeps the first
// that strictly improves, so `best` is the lowest square that achieves the score.  Interior
// nodes only return values; they try corners first, then ascending.
#pragma once
#include "negamax.h"

namespace azs {

using azn::kDone;
using azn::kRun;
constexpr int kSkipped = -128;   // AZ_SOLVE_SKIPPED
constexpr int kAborted = -127;   // AZ_SOLVE_ABORTED
constexpr int kMaxEmpties = 14;  // AZ_SOLVE_MAX_EMPTIES
constexpr int kMaxFrames = kMaxEmpties - 1;
constexpr int kInf = azn::kInf;  // outside every value (|value| <= 64)

struct Search : azn::WaitingFrame {};

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

// Start the search of one position.  Positions that are not searched (more than
// max_empties empties, overlapping boards) and terminal roots finish here.
AZ_HD void init(Search& s, uint64_t own, uint64_t opp, int max_empties) {
  azn::start(s, own, opp, kInf, (own & opp) != 0 || 64 - azb::popc(own | opp) > max_empties,
             kSkipped, azb::popc(own) - azb::popc(opp));
}

// Advance one node.  max_frames = the stack's capacity (a full stack aborts the search
// instead of writing past it; unreachable for max_empties <= max_frames + 1).
template <class Stack>
AZ_HD void step(Search& s, Stack& st, uint64_t node_limit, int max_frames) {
  azn::take_handed(s);  // the value of the move tried last
  if (s.moves == 0) {   // this frame is finished: hand its value to the parent
    if (s.sp == 0) return azn::finish_root(s);
    azn::hand(s, azn::undo(s), s.sq);
    uint32_t pk;
    st.get(s.sp, s.flips, s.moves, pk);
    azn::unpack_frame(s, pk);
    return;
  }
  // the next move of this frame: the root in ascending order, so its best is the lowest
  const int sq = azn::pick(s.moves, s.sp > 0);
  if (!azn::count_move(s, sq, node_limit, kAborted)) return;
  azn::Child c = azn::make_child(s, sq, true);
  if (!c.moves) {
    c.moves = azn::mover_moves(c, true);
    if (!c.moves) return azn::hand(s, azn::final_diff(c), sq);  // the game ended with this move
    azn::pass(s, c);
  }
  if (!azn::room(s, max_frames, kAborted)) return;
  st.put(s.sp, s.flips, s.moves, azn::pack_frame(s));
  azn::enter(s, c, kInf);
}

// One whole search on the host.
inline void solve_one(uint64_t own, uint64_t opp, int max_empties, uint64_t node_limit,
                      int8_t* score, uint8_t* best, uint64_t* nodes) {
  Search s;
  init(s, own, opp, max_empties);
  azn::run_host<HostStack>(s, node_limit, kMaxFrames, score, best, nodes);
}

}  // namespace azs
