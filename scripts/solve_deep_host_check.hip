// solve_deep_host_check.hip — stand-alone host check of oth_solve_deep_cpu for sanitizer
// builds (never loaded into Python, never run on a GPU):
//
//   cd alphazero-othello_amd && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 \
//     -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//     -DAZ_BUILD_ID='"check"' ../scripts/solve_deep_host_check.hip csrc/solve_deep.hip \
//     csrc/board.hip -o /tmp/solve_deep_host_check && /tmp/solve_deep_host_check
//
// 480 positions with 1..12 empties from seeded random playouts, each solved in the full
// window and in a seeded random window, and compared with a plain recursive negamax (its own
// code, not solve_deep.h) that scores every root move in the full window: the window
// contract of the score, and `best` by its exact value.  The skip / abort / argument
// conventions are touched as well.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../alphazero-othello_amd/csrc/bitboard.h"
#include "../include/az_othello.h"

static uint64_t rng_state = 0xD1B54A32D192ED03ull;
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

int main() {
  const int kMax = 12;
  std::vector<uint64_t> own, opp;
  while (own.size() < 480) {
    uint64_t o = azb::kInitOwn, p = azb::kInitOpp;
    const int target = 1 + (int)(rng() % kMax);
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
    own.push_back(o);
    opp.push_back(p);
  }
  const int64_t n = (int64_t)own.size();
  int bad = 0, inside = 0, high = 0, low = 0;
  uint64_t total = 0;
  for (int64_t i = 0; i < n; ++i) {
    // the exact value of every root move, and the exact score
    int value[64], want = AZ_SOLVE_SKIPPED;
    for (int a = 0; a < 64; ++a) value[a] = -1000;
    const bool searched = 64 - azb::popc(own[i] | opp[i]) <= kMax;
    uint64_t m = searched ? azb::legal(own[i], opp[i]) : 0;
    if (searched && !m) want = negamax(own[i], opp[i], -65, 65, false);
    if (m) want = -65;
    for (uint64_t r = m; r; r &= r - 1) {
      const int sq = __builtin_ctzll(r);
      const uint64_t f = azb::flips(own[i], opp[i], sq);
      value[sq] = -negamax(opp[i] ^ f, (own[i] | (1ull << sq)) ^ f, -65, 65, false);
      if (value[sq] > want) want = value[sq];
    }
    for (int pass = 0; pass < 2; ++pass) {
      int alpha = -65, beta = 65;
      if (pass) {
        alpha = -64 + (int)(rng() % 128);                   // -64..63
        beta = alpha + 1 + (int)(rng() % (rng() % 2 ? 4 : 64));
        if (beta > 64) beta = 64;
      }
      int8_t v;
      uint8_t b;
      uint64_t nodes;
      const int rc = oth_solve_deep_cpu(&own[i], &opp[i], 1, kMax, alpha, beta, 1ull << 31, &v, &b,
                                        &nodes);
      if (rc != AZ_OK) return printf("oth_solve_deep_cpu failed: %s\n", az_last_error()), 1;
      total += nodes;
      bool ok;
      if (!searched) {
        ok = v == AZ_SOLVE_SKIPPED && b == 255;
      } else {
        if (want > alpha && want < beta) {
          ok = v == want;
          ++inside;
        } else if (want >= beta) {
          ok = v >= beta && v <= want;
          ++high;
        } else {
          ok = v >= want && v <= alpha;
          ++low;
        }
        if (!m) {
          ok = ok && b == 64;
        } else {
          ok = ok && b < 64 && value[b] > -1000;
          if (ok && v > alpha && v < beta) ok = value[b] == want;
          if (ok && v >= beta) ok = value[b] >= beta;
        }
      }
      if (!ok) {
        ++bad;
        printf("position %lld window (%d, %d): got (%d, %d), exact %d\n", (long long)i, alpha,
               beta, v, b, want);
      }
    }
  }
  // conventions: limit, skip, bad arguments, NULL nodes, n = 0
  std::vector<int8_t> score(n);
  std::vector<uint8_t> best(n);
  std::vector<uint64_t> nodes(n);
  int rc = oth_solve_deep_cpu(own.data(), opp.data(), n, kMax, -1, 1, 3, score.data(), best.data(),
                              nullptr);
  bad += rc != AZ_OK;
  for (int64_t i = 0; i < n; ++i)
    bad += score[i] == AZ_SOLVE_ABORTED && best[i] != 255;
  rc = oth_solve_deep_cpu(own.data(), opp.data(), n, 0, -65, 65, 1000, score.data(), best.data(),
                          nodes.data());
  bad += rc != AZ_OK;
  for (int64_t i = 0; i < n; ++i)
    bad += (64 - azb::popc(own[i] | opp[i]) > 0) && score[i] != AZ_SOLVE_SKIPPED;
  bad += oth_solve_deep_cpu(own.data(), opp.data(), n, 21, -65, 65, 1000, score.data(),
                            best.data(), nullptr) != AZ_ERR_ARG;
  bad += oth_solve_deep_cpu(own.data(), opp.data(), n, 12, 5, 5, 1000, score.data(), best.data(),
                            nullptr) != AZ_ERR_ARG;
  bad += oth_solve_deep_cpu(own.data(), opp.data(), n, 12, -66, 5, 1000, score.data(),
                            best.data(), nullptr) != AZ_ERR_ARG;
  bad += oth_solve_deep_cpu(nullptr, nullptr, 0, 12, -65, 65, 1000, nullptr, nullptr, nullptr) !=
         AZ_OK;
  printf("solve_deep_host_check: %lld positions, %llu nodes, windows inside / high / low "
         "%d / %d / %d, %d mismatches\n", (long long)n, (unsigned long long)total, inside, high,
         low, bad);
  return bad != 0;
}
