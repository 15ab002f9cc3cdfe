// leaf_solve_host_check.hip — stand-alone host check of az_leaf_solve_cpu for sanitizer builds
// (never loaded into Python, never run on a GPU):
//
//   cd alphazero-othello_amd && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 \
//     -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//     -DAZ_BUILD_ID='"check"' ../scripts/leaf_solve_host_check.hip csrc/leaf_solve.hip \
//     csrc/board.hip -o /tmp/leaf_solve_host_check && /tmp/leaf_solve_host_check
//
// Seeded rows (positions with 0..14 empties from random playouts, written as planes, mixed
// with all-zero rows and with rows whose values sit just inside the decoding thresholds) at
// R = 1, 63, 64, 65 and 1000, in heap buffers of exactly R rows so that a read or write past
// either end is caught.  Every row's value is compared with a plain recursive negamax (its
// own code, not solve_deep.h) where the row is to be solved, and with its sentinel's bits
// elsewhere; the node limit, the counters and the argument checks are touched as well.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

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

static float sentinel(int64_t r) { return 0.25f + (float)r / 4096.0f; }

int main() {
  const int kE = 8;
  const int64_t sizes[] = {1, 63, 64, 65, 1000};
  int bad = 0;
  long long rows_total = 0, solved_total = 0, kept_total = 0;
  unsigned long long nodes_total = 0;
  for (const int64_t R : sizes) {
    std::vector<uint64_t> own(R), opp(R);
    // exactly R rows on the heap: the sanitizer sees a read or write one past either end
    float* x = (float*)malloc((size_t)R * 64 * sizeof(float));
    float* v = (float*)malloc((size_t)R * sizeof(float));
    for (int64_t r = 0; r < R; ++r) {
      const uint64_t kind = rng() % 8;
      if (kind == 0) {
        own[r] = opp[r] = 0;  // no leaf
      } else {
        playout((int)(rng() % 15), &own[r], &opp[r]);
      }
      // planes; every third row with values just inside the thresholds instead of +-1 / 0
      const bool soft = r % 3 == 2;
      for (int i = 0; i < 64; ++i) {
        float f = ((own[r] >> i) & 1) ? 1.0f : (((opp[r] >> i) & 1) ? -1.0f : 0.0f);
        if (soft) f = f > 0 ? 0.51f : (f < 0 ? -0.51f : ((i & 1) ? 0.49f : -0.49f));
        x[r * 64 + i] = f;
      }
      v[r] = sentinel(r);
    }
    uint64_t stats[3] = {~0ull, ~0ull, ~0ull};
    int rc = az_leaf_solve_cpu(x, v, R, kE, 1ull << 31, stats);
    if (rc != AZ_OK) return printf("az_leaf_solve_cpu failed: %s\n", az_last_error()), 1;
    uint64_t want_solved = 0;
    for (int64_t r = 0; r < R; ++r) {
      const int e = 64 - azb::popc(own[r] | opp[r]);
      const float s = sentinel(r);
      bool ok;
      if (e >= 1 && e <= kE) {
        const int sc = negamax(own[r], opp[r], -65, 65, false);
        ok = v[r] == (sc > 0 ? 1.0f : (sc < 0 ? -1.0f : 0.0f));
        ++want_solved;
      } else {
        ok = memcmp(&v[r], &s, sizeof(float)) == 0;
        ++kept_total;
      }
      if (!ok) {
        ++bad;
        printf("R=%lld row %lld (%d empties): value %g\n", (long long)R, (long long)r, e, v[r]);
      }
    }
    bad += stats[0] != want_solved || stats[1] != 0 || stats[2] < want_solved;
    rows_total += R;
    solved_total += (long long)stats[0];
    nodes_total += stats[2];
    // a node limit of 1: only searches that end at their root finish (a terminal root); every
    // other task keeps its sentinel, and the two counters add up to the tasks
    for (int64_t r = 0; r < R; ++r) v[r] = sentinel(r);
    rc = az_leaf_solve_cpu(x, v, R, kE, 1, stats);
    bad += rc != AZ_OK || stats[0] + stats[1] != want_solved;
    uint64_t written = 0;
    for (int64_t r = 0; r < R; ++r) {
      const float s = sentinel(r);
      written += memcmp(&v[r], &s, sizeof(float)) != 0;
    }
    bad += written != stats[0];
    // NULL stats
    bad += az_leaf_solve_cpu(x, v, R, kE, 256, nullptr) != AZ_OK;
    free(x);
    free(v);
  }
  float one[64] = {0}, val = 0.5f;
  bad += az_leaf_solve_cpu(one, &val, 1, 0, 256, nullptr) != AZ_ERR_ARG;
  bad += az_leaf_solve_cpu(one, &val, 1, 13, 256, nullptr) != AZ_ERR_ARG;
  bad += az_leaf_solve_cpu(one, &val, 1, 6, 0, nullptr) != AZ_ERR_ARG;
  bad += az_leaf_solve_cpu(one, &val, -1, 6, 256, nullptr) != AZ_ERR_ARG;
  bad += az_leaf_solve_cpu(nullptr, nullptr, 1, 6, 256, nullptr) != AZ_ERR_ARG;
  bad += az_leaf_solve_cpu(nullptr, nullptr, 0, 6, 256, nullptr) != AZ_OK;
  bad += val != 0.5f;
  printf("leaf_solve_host_check: %lld rows, %lld solved, %lld kept, %llu nodes, %d mismatches\n",
         rows_total, solved_total, kept_total, nodes_total, bad);
  return bad != 0;
}
