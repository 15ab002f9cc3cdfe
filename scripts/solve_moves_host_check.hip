// solve_moves_host_check.hip — stand-alone host check of oth_solve_moves_cpu for sanitizer
// builds (never loaded into Python, never run on a GPU):
//
//   cd alphazero-othello_amd && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 \
//     -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//     -DAZ_BUILD_ID='"check"' ../scripts/solve_moves_host_check.hip csrc/solve_moves.hip \
//     csrc/board.hip -o /tmp/solve_moves_host_check && /tmp/solve_moves_host_check
//
// Seeded roots (positions with 0..11 empties from random playouts, mixed with overlapping
// boards) at n = 1, 63, 64, 65 and 1000, in heap buffers of exactly n * 65 / n bytes (n * 8
// for the node counts) so that a read or write past either end is caught.  Every row of the
// three modes is compared with a plain recursive negamax (its own code, not solve_deep.h);
// the node limit and the argument checks are touched as well.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../alphazero-othello_amd/csrc/bitboard.h"
#include "../include/az_othello.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
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

// the true table of one root: exact value of every available action, -128 elsewhere;
// returns the number of available actions
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

int main() {
  const int kE = 9;
  const int64_t sizes[] = {1, 63, 64, 65, 1000};
  int bad = 0;
  long long roots = 0, searched = 0, rows_none = 0, aborted = 0;
  unsigned long long nodes_total = 0;
  for (const int64_t n : sizes) {
    // exactly n entries on the heap: the sanitizer sees a read or write one past either end
    uint64_t* own = (uint64_t*)malloc((size_t)n * 8);
    uint64_t* opp = (uint64_t*)malloc((size_t)n * 8);
    int8_t* values = (int8_t*)malloc((size_t)n * 65);
    int8_t* score = (int8_t*)malloc((size_t)n);
    uint64_t* nodes = (uint64_t*)malloc((size_t)n * 8);
    int8_t* lim_values = (int8_t*)malloc((size_t)n * 65);
    int8_t* lim_score = (int8_t*)malloc((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
      playout((int)(rng() % 12), &own[i], &opp[i]);
      if (rng() % 16 == 0) own[i] |= opp[i] & (0ull - opp[i]);  // overlapping: opp's lowest stone
    }
    for (int mode = 0; mode < 3; ++mode) {
      memset(values, 77, (size_t)n * 65);
      memset(score, 77, (size_t)n);
      int rc = oth_solve_moves_cpu(own, opp, n, kE, mode, 1ull << 31, values, score, nodes);
      if (rc != AZ_OK) return printf("oth_solve_moves_cpu failed: %s\n", az_last_error()), 1;
      for (int64_t i = 0; i < n; ++i) {
        const int8_t* row = values + i * 65;
        const int e = 64 - azb::popc(own[i] | opp[i]);
        int want[65];
        bool ok = true;
        if ((own[i] & opp[i]) != 0 || e > kE) {
          for (int a = 0; a < 65; ++a) ok &= row[a] == AZ_MOVES_NONE;
          ok &= score[i] == AZ_SOLVE_SKIPPED && nodes[i] == 0;
          rows_none += mode == 0;
        } else {
          const int k = truth(own[i], opp[i], want);
          int top = -65;
          for (int a = 0; a < 65; ++a)
            if (want[a] != AZ_MOVES_NONE && want[a] > top) top = want[a];
          if (k == 0) {
            for (int a = 0; a < 65; ++a) ok &= row[a] == AZ_MOVES_NONE;
            ok &= score[i] == azb::popc(own[i]) - azb::popc(opp[i]) && nodes[i] == 1;
            rows_none += mode == 0;
          } else {
            searched += mode == 0;
            ok &= nodes[i] > (uint64_t)k;
            for (int a = 0; a < 65; ++a) {
              const int w = want[a], g = row[a];
              if (w == AZ_MOVES_NONE)
                ok &= g == AZ_MOVES_NONE;
              else if (mode == AZ_MOVES_SCORES)
                ok &= g == w;
              else if (mode == AZ_MOVES_WLD)
                ok &= g == sign(w);
              else
                ok &= w == top ? g == top : (w <= g && g <= top - 1);
            }
            ok &= score[i] == (mode == AZ_MOVES_WLD ? sign(top) : top);
          }
        }
        if (!ok) {
          ++bad;
          printf("n=%lld root %lld mode %d (%d empties): score %d\n", (long long)n, (long long)i,
                 mode, e, (int)score[i]);
        }
        nodes_total += nodes[i];
      }
      // a node limit of 6 per search: a root is aborted (all NONE, -127) or equal to the above
      rc = oth_solve_moves_cpu(own, opp, n, kE, mode, 6, lim_values, lim_score, nullptr);
      bad += rc != AZ_OK;
      for (int64_t i = 0; i < n; ++i) {
        bool ok = true;
        if (lim_score[i] == AZ_SOLVE_ABORTED) {
          for (int a = 0; a < 65; ++a) ok &= lim_values[i * 65 + a] == AZ_MOVES_NONE;
          aborted += mode == 0;
        } else {
          ok &= lim_score[i] == score[i] && memcmp(lim_values + i * 65, values + i * 65, 65) == 0;
        }
        bad += !ok;
      }
    }
    roots += n;
    free(own), free(opp), free(values), free(score), free(nodes), free(lim_values), free(lim_score);
  }
  uint64_t one = 0;
  int8_t row[65], sc = 5;
  bad += oth_solve_moves_cpu(&one, &one, 1, 21, 0, 100, row, &sc, nullptr) != AZ_ERR_ARG;
  bad += oth_solve_moves_cpu(&one, &one, 1, -1, 0, 100, row, &sc, nullptr) != AZ_ERR_ARG;
  bad += oth_solve_moves_cpu(&one, &one, 1, 12, 3, 100, row, &sc, nullptr) != AZ_ERR_ARG;
  bad += oth_solve_moves_cpu(&one, &one, -1, 12, 0, 100, row, &sc, nullptr) != AZ_ERR_ARG;
  bad += oth_solve_moves_cpu(nullptr, nullptr, 1, 12, 0, 100, row, &sc, nullptr) != AZ_ERR_ARG;
  bad += oth_solve_moves_cpu(nullptr, nullptr, 0, 12, 0, 100, nullptr, nullptr, nullptr) != AZ_OK;
  bad += sc != 5;
  printf("solve_moves_host_check: %lld roots x 3 modes, %lld searched, %lld all-NONE, %lld aborted "
         "at 6 nodes, %llu nodes, %d mismatches\n",
         roots, searched, rows_none, aborted, nodes_total, bad);
  return bad != 0;
}
