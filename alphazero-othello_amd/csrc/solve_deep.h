// solve_deep.h — windowed, move-ordered endgame search shared by oth_solve_deep_cpu and the
// k_solve_deep kernel.  The same shape as solve.h (an iterative fail-soft negamax written as
// a per-position state machine, the top frame in registers, the frames below it in a stack
// the caller provides, no recursion, every loop around step() bounded by the node limit) out
// of the same pieces (negamax.h: the pass, end-of-game and node rules, the window, the frame
// word); its own are a root window and an ordering of the moves.  solve.h keeps its order and
// its lowest-square `best`; every root's result and node count of both are pinned by
// tests/golden/search_goldens.npz.
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
#include "negamax.h"

namespace azd {

using azn::kDone;
using azn::kRun;
constexpr int kSkipped = -128;   // AZ_SOLVE_SKIPPED
constexpr int kAborted = -127;   // AZ_SOLVE_ABORTED
constexpr int kMaxEmpties = 20;  // AZ_SOLVE_DEEP_MAX_EMPTIES
constexpr int kMaxFrames = kMaxEmpties - 1;
constexpr int kInf = azn::kInf;  // outside every value (|value| <= 64)
constexpr int kOrderMin = 5;
constexpr int kOrderSlots = 10;
constexpr uint64_t kNoKeys = 0x0FFFFFFFFFFFFFFFull;  // ten empty slots: key 63 each

struct Search : azn::Frame {
  uint64_t order;  // top frame: ordered squares not tried yet (6 bits each, count in 60..63)
  uint64_t probe;  // top frame: placements still to probe for the order (not stacked)
  uint64_t keys;   // keys of the squares in `order` while probing (not stacked)
};

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

// The top frame starts with its placements s.moves: decide whether they are probed first.
AZ_HD void start_frame(Search& s) {
  const uint64_t m = s.moves;
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
  s.order = 0;
  s.probe = 0;
  s.keys = kNoKeys;
  s.moves = azn::start(s, own, opp, alpha, beta, kInf,
                       (own & opp) != 0 || 64 - azb::popc(own | opp) > max_empties, kSkipped,
                       azb::popc(own) - azb::popc(opp));
  if (s.moves) start_frame(s);
}

// The next ordered square leaves the order word.
AZ_HD void order_pop(Search& s) {
  s.order = ((s.order & ((1ull << 60) - 1)) >> 6) | (((s.order >> 60) - 1) << 60);
}

// Advance one step: a finished frame's value handed to its parent, then a probe or a move
// (a new node).  max_frames = the stack's capacity (a full stack aborts the search instead of
// writing past it; unreachable for max_empties <= max_frames + 1).
template <class Stack>
AZ_HD void step(Search& s, Stack& st, uint64_t node_limit, int max_frames) {
  if (s.moves == 0) {  // this frame is finished: its parent takes its value in this step
    if (s.sp == 0) return azn::finish_root(s);
    const int sq = s.sq, ret = azn::undo(s);
    uint32_t pk;
    st.get(s.sp, s.flips, s.moves, s.order, pk);
    azn::unpack_frame(s, pk);
    azn::take(s, ret, sq);
    if (s.moves == 0) return;  // the parent is finished as well: the next step's work
  }
  // the square of this step: the next probe, else the next move of this frame
  const bool probing = s.probe != 0, ordered = (s.order >> 60) != 0;
  const int sq = probing ? __builtin_ctzll(s.probe)
                         : (ordered ? (int)(s.order & 63) : azn::pick(s.moves, true));
  azn::Child c = azn::make_child(s, sq, true);
  if (probing) {
    const uint64_t bit = 1ull << sq;
    s.probe &= ~bit;
    order_insert(s, sq, 2 * azb::popc(c.moves) + ((bit & azn::kCorners) ? 0 : 1));
    return;
  }
  if (ordered) order_pop(s);
  if (!azn::count_move(s, sq, node_limit, kAborted)) return;
  if (!c.moves) {
    c.moves = azn::mover_moves(c, true);
    if (!c.moves) return azn::take(s, azn::final_diff(c), sq);  // the game ended with this move
    azn::pass(s, c);
  }
  if (!azn::room(s, max_frames, kAborted)) return;
  st.put(s.sp, s.flips, s.moves, s.order, azn::pack_frame(s));
  azn::enter(s, c, kInf);
  start_frame(s);
}

// One whole search on the host.
inline void solve_one(uint64_t own, uint64_t opp, int max_empties, int alpha, int beta,
                      uint64_t node_limit, int8_t* score, uint8_t* best, uint64_t* nodes) {
  Search s;
  init(s, own, opp, max_empties, alpha, beta);
  azn::run_host<HostStack>(s, node_limit, kMaxFrames, score, best, nodes);
}

}  // namespace azd
