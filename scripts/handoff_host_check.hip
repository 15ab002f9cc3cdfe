// handoff_host_check.hip — stand-alone host check of oth_line_step_cpu and of the optimal-line
// loop built on it (endgame.optimal_line's host path, restated here in C: the host side of a
// self-play solver hand-off) for sanitizer builds (never loaded into Python, never run on a GPU):
//
//   cd alphazero-othello_amd && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 \
//     -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//     -DAZ_BUILD_ID='"check"' ../scripts/handoff_host_check.hip csrc/line_step.hip \
//     csrc/solve_moves.hip csrc/board.hip -o /tmp/handoff_host_check && /tmp/handoff_host_check
//
// Seeded roots (positions with 0..9 empties from random playouts, mixed with overlapping boards
// and roots above max_empties) at n = 1, 63, 64, 65 and 1000, in heap buffers of exactly the
// sizes the entry points are given (rows: n * stride entries) so that a read or write past
// either end is caught.  Every row of every line is compared with a plain recursive negamax
// (its own code, not solve_deep.h): the position, pi, the lowest optimal action, z, the count of
// rows, the root's score, the terminal end of the line.  A node limit and the argument checks
// are touched as well.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../alphazero-othello_amd/csrc/bitboard.h"
#include "../include/az_othello.h"

static uint64_t rng_state = 0x2545F4914F6CDD1Dull;
static uint64_t rng() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}

static int negamax(uint64_t own, uint64_t opp, int alpha, int beta, bool passed) {
  uint64_t m = azb::legal(own, opp);
  if (!m) {
    if (passed || !azb::legal(opp, own)) return azb::popc(own) - azb::popc(opp);
    return -negamax(opp, own, -beta, -alpha, true);
  }
  int best = -65;
  while (m) {
    const int sq = __builtin_ctzll(m);
    m &= m - 1;
    const uint64_t f = azb::flips(own, opp, sq);
    const int v = -negamax(opp ^ f, (own | (1ull << sq)) ^ f, -beta, -(alpha > best ? alpha : best),
                           false);
    if (v > best) best = v;
    if (best >= beta) break;
  }
  return best;
}

// a position with `target` empties (or the end of a random playout before that)
static void playout(int target, uint64_t* own, uint64_t* opp) {
  uint64_t o = azb::kInitOwn, p = azb::kInitOpp;
  for (;;) {
    if (64 - azb::popc(o | p) <= target) break;
    uint64_t m = azb::legal(o, p);
    if (!m) {
      if (!azb::legal(p, o)) break;
      const uint64_t t = o;
      o = p;
      p = t;
      continue;
    }
    int k = (int)(rng() % (uint64_t)azb::popc(m));
    while (k--) m &= m - 1;
    const int sq = __builtin_ctzll(m);
    const uint64_t f = azb::flips(o, p, sq);
    const uint64_t no = p ^ f, np = (o | (1ull << sq)) ^ f;
    o = no;
    p = np;
  }
  *own = o;
  *opp = p;
}

static int sign(int v) { return (v > 0) - (v < 0); }

// the true value of every available action, -128 elsewhere; returns how many there are
static int truth(uint64_t o, uint64_t p, int* row) {
  for (int a = 0; a < 65; ++a) row[a] = AZ_MOVES_NONE;
  uint64_t m = azb::legal(o, p);
  int k = 0;
  if (!m) {
    if (!azb::legal(p, o)) return 0;
    row[64] = -negamax(p, o, -65, 65, true);
    return 1;
  }
  while (m) {
    const int sq = __builtin_ctzll(m);
    m &= m - 1;
    const uint64_t f = azb::flips(o, p, sq);
    row[sq] = -negamax(p ^ f, (o | (1ull << sq)) ^ f, -65, 65, false);
    ++k;
  }
  return k;
}

struct Line {  // the buffers of one optimal-line run over n roots, each of its exact size
  int64_t n;
  int stride;
  uint64_t *wo, *wp, *row_own, *row_opp;
  int8_t *values, *score, *root_score;
  int32_t* count;
  uint8_t *done, *row_act;
  float *row_pi, *row_z;
};

static Line make_line(int64_t n, int stride) {
  Line L;
  L.n = n;
  L.stride = stride;
  const size_t r = (size_t)n * stride;
  L.wo = (uint64_t*)malloc((size_t)n * 8);
  L.wp = (uint64_t*)malloc((size_t)n * 8);
  L.values = (int8_t*)malloc((size_t)n * 65);
  L.score = (int8_t*)malloc((size_t)n);
  L.root_score = (int8_t*)malloc((size_t)n);
  L.count = (int32_t*)calloc((size_t)n, 4);
  L.done = (uint8_t*)calloc((size_t)n, 1);
  L.row_own = (uint64_t*)malloc(r * 8);
  L.row_opp = (uint64_t*)malloc(r * 8);
  L.row_pi = (float*)malloc(r * 65 * 4);
  L.row_act = (uint8_t*)malloc(r);
  L.row_z = (float*)malloc(r * 4);
  memset(L.root_score, 77, (size_t)n);
  memset(L.row_pi, 0x7f, r * 65 * 4);
  return L;
}

static void free_line(Line& L) {
  free(L.wo), free(L.wp), free(L.values), free(L.score), free(L.root_score), free(L.count);
  free(L.done), free(L.row_own), free(L.row_opp), free(L.row_pi), free(L.row_act), free(L.row_z);
}

// the ply loop of endgame.optimal_line; returns the plies run, -1 on an error code
static int run_line(Line& L, const uint64_t* own, const uint64_t* opp, int max_empties,
                    uint64_t node_limit) {
  memcpy(L.wo, own, (size_t)L.n * 8);
  memcpy(L.wp, opp, (size_t)L.n * 8);
  for (int ply = 0; ply <= L.stride; ++ply) {
    if (oth_solve_moves_cpu(L.wo, L.wp, L.n, max_empties, AZ_MOVES_OPTIMAL, node_limit, L.values,
                            L.score, nullptr) != AZ_OK)
      return -1;
    int32_t live = -1;
    if (oth_line_step_cpu(L.wo, L.wp, L.values, L.score, L.n, L.stride, ply == 0, L.count, L.done,
                          L.root_score, L.row_own, L.row_opp, L.row_pi, L.row_act, L.row_z,
                          &live) != AZ_OK)
      return -1;
    int32_t open = 0;
    for (int64_t i = 0; i < L.n; ++i) open += !L.done[i];
    if (open != live) return -1;
    if (live == 0) return ply + 1;
  }
  return -1;
}

int main() {
  const int kE = 9;
  const int64_t sizes[] = {1, 63, 64, 65, 1000};
  int bad = 0;
  long long roots = 0, rows = 0, passes = 0, ties = 0, empty = 0, skipped = 0, aborted = 0;
  for (const int64_t n : sizes) {
    uint64_t* own = (uint64_t*)malloc((size_t)n * 8);
    uint64_t* opp = (uint64_t*)malloc((size_t)n * 8);
    for (int64_t i = 0; i < n; ++i) {
      playout((int)(rng() % 11), &own[i], &opp[i]);  // 0..10 empties: 10 is above kE
      if (rng() % 16 == 0) own[i] |= opp[i] & (0ull - opp[i]);  // overlapping: opp's lowest stone
    }
    Line L = make_line(n, 2 * kE);
    if (run_line(L, own, opp, kE, 1ull << 31) < 0)
      return printf("line loop failed: %s\n", az_last_error()), 1;
    for (int64_t i = 0; i < n; ++i) {
      const int e = 64 - azb::popc(own[i] | opp[i]);
      bool ok = L.done[i] == 1 && L.wo[i] == ~0ull && L.wp[i] == ~0ull;
      if ((own[i] & opp[i]) != 0 || e > kE) {
        ok &= L.root_score[i] == AZ_SOLVE_SKIPPED && L.count[i] == 0;
        ++skipped;
      } else {
        const int root = negamax(own[i], opp[i], -65, 65, false);
        ok &= L.root_score[i] == root && L.count[i] <= 2 * e;
        uint64_t o = own[i], p = opp[i];
        int side = 1;
        empty += L.count[i] == 0;
        for (int t = 0; t < L.count[i] && ok; ++t) {
          const int64_t r = i * L.stride + t;
          int want[65];
          const int k = truth(o, p, want);
          int top = -65, hits = 0, act = -1;
          for (int a = 0; a < 65; ++a)
            if (want[a] != AZ_MOVES_NONE && want[a] > top) top = want[a];
          for (int a = 64; a >= 0; --a)
            if (want[a] == top) ++hits, act = a;
          ok &= k > 0 && top == side * root;
          ok &= L.row_own[r] == o && L.row_opp[r] == p && L.row_act[r] == act;
          ok &= L.row_z[r] == (float)sign(top);
          const float w = (float)(1.0 / (double)hits);
          for (int a = 0; a < 65; ++a) ok &= L.row_pi[r * 65 + a] == (want[a] == top ? w : 0.0f);
          passes += act == 64;
          ties += hits > 1;
          if (!ok) break;
          uint64_t no, np;
          azb::play(o, p, act, act == 64 ? 0ull : azb::flips(o, p, act), &no, &np);
          o = no;
          p = np;
          side = -side;
          ++rows;
        }
        // the line ends where the game does, at the root's score
        ok &= !azb::legal(o, p) && !azb::legal(p, o);
        ok &= side * (azb::popc(o) - azb::popc(p)) == root;
      }
      if (!ok) {
        ++bad;
        printf("n=%lld root %lld (%d empties): score %d, %d rows\n", (long long)n, (long long)i, e,
               (int)L.root_score[i], (int)L.count[i]);
      }
    }
    // a node limit of 6 per search: every root is aborted without rows, or has the line above
    Line A = make_line(n, 2 * kE);
    if (run_line(A, own, opp, kE, 6) < 0) return printf("limited loop failed\n"), 1;
    for (int64_t i = 0; i < n; ++i) {
      bool ok = A.done[i] == 1;
      if (A.root_score[i] == AZ_SOLVE_ABORTED) {
        ok &= A.count[i] == 0;
        ++aborted;
      } else {
        ok &= A.root_score[i] == L.root_score[i] && A.count[i] == L.count[i];
        const int64_t r = i * L.stride;
        const size_t c = (size_t)L.count[i];
        ok &= memcmp(A.row_own + r, L.row_own + r, c * 8) == 0;
        ok &= memcmp(A.row_opp + r, L.row_opp + r, c * 8) == 0;
        ok &= memcmp(A.row_pi + r * 65, L.row_pi + r * 65, c * 65 * 4) == 0;
        ok &= memcmp(A.row_act + r, L.row_act + r, c) == 0;
        ok &= memcmp(A.row_z + r, L.row_z + r, c * 4) == 0;
      }
      bad += !ok;
    }
    roots += n;
    free_line(L), free_line(A), free(own), free(opp);
  }
  // a step on finished roots writes nothing; the argument checks
  {
    Line L = make_line(1, 4);
    uint64_t o = azb::kInitOwn, p = azb::kInitOpp;
    L.wo[0] = o, L.wp[0] = p, L.done[0] = 1, L.score[0] = 0;
    memset(L.values, 0, 65);
    int32_t live = 9;
    bad += oth_line_step_cpu(L.wo, L.wp, L.values, L.score, 1, 4, 0, L.count, L.done, L.root_score,
                             L.row_own, L.row_opp, L.row_pi, L.row_act, L.row_z, &live) != AZ_OK;
    bad += live != 0 || L.count[0] != 0 || L.wo[0] != o || L.root_score[0] != 77;
    bad += oth_line_step_cpu(L.wo, L.wp, L.values, L.score, 1, 0, 0, L.count, L.done, L.root_score,
                             L.row_own, L.row_opp, L.row_pi, L.row_act, L.row_z,
                             &live) != AZ_ERR_ARG;
    bad += oth_line_step_cpu(L.wo, L.wp, L.values, L.score, 1, 41, 0, L.count, L.done,
                             L.root_score, L.row_own, L.row_opp, L.row_pi, L.row_act, L.row_z,
                             &live) != AZ_ERR_ARG;
    bad += oth_line_step_cpu(L.wo, L.wp, L.values, L.score, -1, 4, 0, L.count, L.done,
                             L.root_score, L.row_own, L.row_opp, L.row_pi, L.row_act, L.row_z,
                             &live) != AZ_ERR_ARG;
    bad += oth_line_step_cpu(L.wo, L.wp, nullptr, L.score, 1, 4, 0, L.count, L.done, L.root_score,
                             L.row_own, L.row_opp, L.row_pi, L.row_act, L.row_z,
                             &live) != AZ_ERR_ARG;
    bad += oth_line_step_cpu(L.wo, L.wp, L.values, L.score, 1, 4, 0, L.count, L.done, L.root_score,
                             L.row_own, L.row_opp, L.row_pi, L.row_act, L.row_z,
                             nullptr) != AZ_ERR_ARG;
    bad += oth_line_step_cpu(nullptr, nullptr, nullptr, nullptr, 0, 4, 1, nullptr, nullptr, nullptr,
                             nullptr, nullptr, nullptr, nullptr, nullptr, &live) != AZ_OK;
    free_line(L);
  }
  printf("handoff_host_check: %lld roots, %lld rows (%lld passes, %lld with tied optimal moves), "
         "%lld empty lines, %lld skipped, %lld aborted at 6 nodes, %d mismatches\n",
         roots, rows, passes, ties, empty, skipped, aborted, bad);
  return bad != 0;
}
