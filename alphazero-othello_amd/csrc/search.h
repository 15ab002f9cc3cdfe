// search.h — depth-limited alpha-beta with a heuristic leaf evaluation, shared by
// oth_search_cpu / oth_eval_cpu and the k_search / k_eval kernels (one source of truth, like
// solve.h, whose per-position state machine this follows): step() advances ONE node of one
// search, nothing recurses, and every loop around step() is bounded by the node limit.
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
#include "bitboard.h"

namespace azq {

constexpr int kSkipped = -32768;  // AZ_SEARCH_SKIPPED
constexpr int kAborted = -32767;  // AZ_SEARCH_ABORTED
constexpr int kMaxDepth = 10;     // AZ_SEARCH_MAX_DEPTH
constexpr int kMaxFrames = kMaxDepth - 1;
constexpr int kInf = 32000;  // outside every value (|value| <= 10000 + 100 * 64)
constexpr uint64_t kCorners = 0x8100000000000081ull;

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

enum : int { kRun = 0, kDone = 1 };

struct Search {
  uint64_t own, opp;  // top frame: side to move, its opponent
  uint64_t moves;     // top frame: placements not tried yet
  uint64_t flips;     // capture set of the move that led to the top frame
  uint64_t nodes;     // nodes visited so far
  int alpha, beta, best;  // top frame's window (alpha already raised to best) and value so far
  int sq, sign;       // square of the move that led here; 1 = reached through a pass as well
  int depth;          // plies left below the top frame's position (>= 1)
  int sp;             // frames on the stack below the top frame
  int ret, ret_sq, pending;  // a child's value (parent's view) waiting to be taken
  int state;          // kRun / kDone
  int root_pass;      // the root itself had to pass: the top-level frame is the opponent's
  int value, root_best;  // results once state == kDone
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

AZ_HD void finish(Search& s, int value, int best) {
  s.state = kDone;
  s.value = value;
  s.root_best = best;
}

// Start the search of one position to `depth` >= 1 plies.  Overlapping boards are not
// searched; terminal roots finish here.
AZ_HD void init(Search& s, uint64_t own, uint64_t opp, int depth) {
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
  s.depth = depth;
  s.sp = 0;
  s.ret = 0;
  s.ret_sq = 0;
  s.pending = 0;
  s.root_pass = 0;
  s.state = kRun;
  s.value = 0;
  s.root_best = azb::kPass;
  if ((own & opp) != 0) {
    finish(s, kSkipped, 255);
    return;
  }
  s.nodes = 1;
  uint64_t m = azb::legal(own, opp);
  if (!m) {
    m = azb::legal(opp, own);
    if (!m) {
      finish(s, terminal_value(azb::popc(own) - azb::popc(opp)), azb::kPass);
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
// instead of writing past it; unreachable for depth <= max_frames + 1).
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
    uint64_t pk;
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
  const int cdepth = s.depth - 1;
  uint64_t cm = azb::legal(cown, copp);
  // the mover's own placements decide a pass / the end of the game, and are half of h
  const uint64_t cm2 = (cdepth == 0 || !cm) ? azb::legal(copp, cown) : 0ull;
  if (!(cm | cm2)) {  // the game ended with this move
    s.ret = terminal_value(azb::popc(copp) - azb::popc(cown));
    s.ret_sq = sq;
    s.pending = 1;
    return;
  }
  if (cdepth == 0) {  // the horizon
    s.ret = -heuristic(cown, copp, cm, cm2);
    s.ret_sq = sq;
    s.pending = 1;
    return;
  }
  int sign = 0;
  if (!cm) {  // the opponent passes: the mover's side again, the same plies left
    const uint64_t t = cown;
    cown = copp;
    copp = t;
    cm = cm2;
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
  s.depth = cdepth;
}

// One whole search on the host.
inline void search_one(uint64_t own, uint64_t opp, int depth, uint64_t node_limit,
                       int16_t* value, uint8_t* best, uint64_t* nodes) {
  Search s;
  HostStack st;
  init(s, own, opp, depth);
  while (s.state == kRun) step(s, st, node_limit, kMaxFrames);
  *value = (int16_t)s.value;
  *best = (uint8_t)s.root_best;
  if (nodes) *nodes = s.nodes;
}

}  // namespace azq
