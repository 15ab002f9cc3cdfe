// search.h — depth-limited alpha-beta with a heuristic leaf evaluation, shared by
// oth_search_cpu / oth_eval_cpu and the k_search / k_eval kernels (one source of truth, like
// solve.h, and like it a per-position state machine out of negamax.h's pieces): step()
// advances ONE node of one search, nothing recurses, and every loop around step() is bounded
// by the node limit.
//
// Value V(pos, depth) from the side to move's view, the first rule that matches:
//   1. neither side has a placement: T(d) = sign(d) * (10000 + 100 * |d|), 0 for d = 0, with
//      d = popcount(own) - popcount(opp) (empties to nobody, as in solve.h) -- at any depth;
//   2. depth = 0: the heuristic h below;
//   3. the side to move has no placement: -V(sides swapped, depth) (a pass costs no depth);
//   4. otherwise the maximum over placements a of -V(child_a, depth - 1).
// h(own, opp) = sum_sq W[sq] * ([sq in own] - [sq in opp])
//             + 12 * (popcount(legal(own, opp)) - popcount(legal(opp, own)))
// with W the classical D4-symmetric square table kW: seven weight classes, so fourteen mask
// popcounts and no table lookup.  |h| < 1400 < 10000: a decided game outranks any heuristic.
//
// Frames.  As in solve.h the top frame lives in registers (Search) and the frames below it
// in a Stack the caller provides (host: a plain array, device: LDS [frame][field][lane]).  A
// stored frame is 24 bytes: the capture set of the move that led to it, its untried moves,
// and one word packing alpha / beta / best (16 bits each, offset by 32768), the square, the
// pass flag and the remaining depth.  A child without a placement is never a frame of its
// own (solve.h), so every pushed frame has one ply less than its parent and a search of
// depth D stacks at most D - 1 frames, 9 at the cap of 10.
//
// Move order: the root tries its placements in ascending square order and keeps strict
// improvements only, so with fail-soft alpha-beta `best` is the lowest square that achieves
// the value; interior nodes try corners first, then ascending.  value and best are
// properties of the minimax tree, not of the order.
#pragma once
#include "negamax.h"

namespace azq {

using azn::kCorners;
using azn::kDone;
using azn::kRun;
constexpr int kSkipped = -32768;  // AZ_SEARCH_SKIPPED
constexpr int kAborted = -32767;  // AZ_SEARCH_ABORTED
constexpr int kMaxDepth = 10;     // AZ_SEARCH_MAX_DEPTH
constexpr int kMaxFrames = kMaxDepth - 1;
constexpr int kInf = 32000;  // outside every value (|value| <= 10000 + 100 * 64)

// rows 0..3 of W; rows 4..7 mirror them
constexpr int kW[4][8] = {{100, -20, 10, 5, 5, 10, -20, 100},
                          {-20, -50, -2, -2, -2, -2, -50, -20},
                          {10, -2, -1, -1, -1, -1, -2, 10},
                          {5, -2, -1, -1, -1, -1, -2, 5}};
constexpr int square_weight(int sq) { return kW[(sq >> 3) > 3 ? 7 - (sq >> 3) : (sq >> 3)][sq & 7]; }
constexpr uint64_t weight_mask(int v) {
  uint64_t m = 0;
  for (int i = 0; i < 64; ++i)
    if (square_weight(i) == v) m |= 1ull << i;
  return m;
}
constexpr uint64_t kM100 = weight_mask(100), kM20 = weight_mask(-20), kM10 = weight_mask(10),
                   kM5 = weight_mask(5), kM50 = weight_mask(-50), kM2 = weight_mask(-2),
                   kM1 = weight_mask(-1);
static_assert((kM100 | kM20 | kM10 | kM5 | kM50 | kM2 | kM1) == ~0ull && kM100 == kCorners,
              "the weight classes cover the board");

AZ_HD int disc_sum(uint64_t x) {
  return 100 * azb::popc(x & kM100) - 20 * azb::popc(x & kM20) + 10 * azb::popc(x & kM10) +
         5 * azb::popc(x & kM5) - 50 * azb::popc(x & kM50) - 2 * azb::popc(x & kM2) -
         azb::popc(x & kM1);
}

// h from the two legal masks (lo = legal(own, opp), lp = legal(opp, own))
AZ_HD int heuristic(uint64_t own, uint64_t opp, uint64_t lo, uint64_t lp) {
  return disc_sum(own) - disc_sum(opp) + 12 * (azb::popc(lo) - azb::popc(lp));
}

AZ_HD int terminal_value(int d) { return d == 0 ? 0 : (d > 0 ? 10000 + 100 * d : -10000 + 100 * d); }

// T(d) for a terminal position, else h (oth_eval_*)
AZ_HD int evaluate(uint64_t own, uint64_t opp) {
  const uint64_t lo = azb::legal(own, opp), lp = azb::legal(opp, own);
  if (!(lo | lp)) return terminal_value(azb::popc(own) - azb::popc(opp));
  return heuristic(own, opp, lo, lp);
}

struct Search : azn::WaitingFrame {
  int depth;  // plies left below the top frame's position (>= 1)
};

AZ_HD uint64_t pack_frame(const Search& s) {
  return (uint64_t)(uint32_t)(s.alpha + 32768) | ((uint64_t)(uint32_t)(s.beta + 32768) << 16) |
         ((uint64_t)(uint32_t)(s.best + 32768) << 32) |
         ((uint64_t)(uint32_t)(s.sq | (s.sign << 6) | (s.depth << 7)) << 48);
}

AZ_HD void unpack_frame(Search& s, uint64_t w) {
  s.alpha = (int)(w & 0xFFFF) - 32768;
  s.beta = (int)((w >> 16) & 0xFFFF) - 32768;
  s.best = (int)((w >> 32) & 0xFFFF) - 32768;
  s.sq = (int)((w >> 48) & 63);
  s.sign = (int)((w >> 54) & 1);
  s.depth = (int)((w >> 55) & 15);
}

// the host's frame stack (the device's is in search.hip)
struct HostStack {
  uint64_t w[kMaxFrames][3];
  AZ_HD void put(int f, uint64_t flips, uint64_t moves, uint64_t pk) {
    w[f][0] = flips;
    w[f][1] = moves;
    w[f][2] = pk;
  }
  AZ_HD void get(int f, uint64_t& flips, uint64_t& moves, uint64_t& pk) const {
    flips = w[f][0];
    moves = w[f][1];
    pk = w[f][2];
  }
};

// Start the search of one position to `depth` >= 1 plies.  Overlapping boards are not
// searched; terminal roots finish here.
AZ_HD void init(Search& s, uint64_t own, uint64_t opp, int depth) {
  s.depth = depth;
  azn::start(s, own, opp, kInf, (own & opp) != 0, kSkipped,
             terminal_value(azb::popc(own) - azb::popc(opp)));
}

// Advance one node.  max_frames = the stack's capacity (a full stack aborts the search
// instead of writing past it; unreachable for depth <= max_frames + 1).
template <class Stack>
AZ_HD void step(Search& s, Stack& st, uint64_t node_limit, int max_frames) {
  azn::take_handed(s);  // the value of the move tried last
  if (s.moves == 0) {   // this frame is finished: hand its value to the parent
    if (s.sp == 0) return azn::finish_root(s);
    azn::hand(s, azn::undo(s), s.sq);
    uint64_t pk;
    st.get(s.sp, s.flips, s.moves, pk);
    unpack_frame(s, pk);
    return;
  }
  // the next move of this frame: the root in ascending order, so its best is the lowest
  const int sq = azn::pick(s.moves, s.sp > 0);
  if (!azn::count_move(s, sq, node_limit, kAborted)) return;
  azn::Child c = azn::make_child(s, sq, false);
  // the mover's own placements decide a pass / the end of the game, and are half of h
  const uint64_t m2 = (s.depth == 1 || !c.moves) ? azn::mover_moves(c, false) : 0ull;
  if (!(c.moves | m2))  // the game ended with this move
    return azn::hand(s, terminal_value(azn::final_diff(c)), sq);
  if (s.depth == 1)  // the horizon
    return azn::hand(s, -heuristic(c.own, c.opp, c.moves, m2), sq);
  if (!c.moves) {  // the opponent passes, the same plies left
    c.moves = m2;
    azn::pass(s, c);
  }
  if (!azn::room(s, max_frames, kAborted)) return;
  st.put(s.sp, s.flips, s.moves, pack_frame(s));
  azn::enter(s, c, kInf);
  --s.depth;
}

// One whole search on the host.
inline void search_one(uint64_t own, uint64_t opp, int depth, uint64_t node_limit,
                       int16_t* value, uint8_t* best, uint64_t* nodes) {
  Search s;
  init(s, own, opp, depth);
  azn::run_host<HostStack>(s, node_limit, kMaxFrames, value, best, nodes);
}

}  // namespace azq
