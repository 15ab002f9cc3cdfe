// solve_host_check.hip — stand-alone host check of oth_solve_cpu for sanitizer builds (never
// loaded into Python, never run on a GPU):
//
//   cd alphazero-othello_amd && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 \
//     -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//     -DAZ_BUILD_ID='"check"' ../scripts/solve_host_check.hip csrc/solve.hip csrc/board.hip \
//     -o /tmp/solve_host_check && /tmp/solve_host_check
//
// 400 positions with 1..10 empties from seeded random playouts; every result is compared
// with a plain recursive negamax without pruning windows narrower than the full one at the
// root (its own code, not solve.h), and the skip / abort / argument conventions are touched.
#include <stdio.h>
#include <stdlib.h>

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

int main() {
  std::vector<uint64_t> own, opp;
  while (own.size() < 400) {
    uint64_t o = azb::kInitOwn, p = azb::kInitOpp;
    const int target = 1 + (int)(rng() % 10);
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
  std::vector<int8_t> score(n);
  std::vector<uint8_t> best(n);
  std::vector<uint64_t> nodes(n);
  int rc = oth_solve_cpu(own.data(), opp.data(), n, 10, 1ull << 31, score.data(), best.data(),
                         nodes.data());
  if (rc != AZ_OK) return printf("oth_solve_cpu failed: %s\n", az_last_error()), 1;
  int bad = 0;
  uint64_t total = 0;
  for (int64_t i = 0; i < n; ++i) {
    total += nodes[i];
    int want = AZ_SOLVE_SKIPPED, wbest = 255;
    if (64 - azb::popc(own[i] | opp[i]) <= 10) {
      uint64_t m = azb::legal(own[i], opp[i]);
      wbest = 64;
      if (!m) {
        want = negamax(own[i], opp[i], -65, 65, false);
      } else {
        want = -65;
        while (m) {
          const int sq = __builtin_ctzll(m);
          m &= m - 1;
          const uint64_t f = azb::flips(own[i], opp[i], sq);
          const int v = -negamax(opp[i] ^ f, (own[i] | (1ull << sq)) ^ f, -65, 65, false);
          if (v > want) want = v, wbest = sq;
        }
      }
    }
    if (score[i] != want || best[i] != wbest) {
      ++bad;
      printf("position %lld: got (%d, %d), want (%d, %d)\n", (long long)i, score[i], best[i], want,
             wbest);
    }
  }
  // conventions: limit, skip, bad argument, NULL nodes, n = 0
  rc = oth_solve_cpu(own.data(), opp.data(), n, 10, 3, score.data(), best.data(), nullptr);
  bad += rc != AZ_OK;
  rc = oth_solve_cpu(own.data(), opp.data(), n, 0, 1000, score.data(), best.data(), nodes.data());
  bad += rc != AZ_OK;
  for (int64_t i = 0; i < n; ++i)
    bad += (64 - azb::popc(own[i] | opp[i]) > 0) && score[i] != AZ_SOLVE_SKIPPED;
  bad += oth_solve_cpu(own.data(), opp.data(), n, 15, 1000, score.data(), best.data(), nullptr) !=
         AZ_ERR_ARG;
  bad += oth_solve_cpu(nullptr, nullptr, 0, 12, 1000, nullptr, nullptr, nullptr) != AZ_OK;
  printf("solve_host_check: %lld positions, %llu nodes, %d mismatches\n", (long long)n,
         (unsigned long long)total, bad);
  return bad != 0;
}
