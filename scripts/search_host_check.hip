// search_host_check.hip — stand-alone host check of oth_search_cpu / oth_eval_cpu for
// sanitizer builds (never loaded into Python, never run on a GPU):
//
//   cd alphazero-othello_amd && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 \
//     -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//     -DAZ_BUILD_ID='"check"' ../scripts/search_host_check.hip csrc/search.hip csrc/board.hip \
//     -o /tmp/search_host_check && /tmp/search_host_check
//
// 300 positions from seeded random playouts of 0..59 plies, searched at depth 1..5; every
// result is compared with a plain recursive negamax without pruning and a square-by-square
// evaluation (its own code, not search.h), and the skip / abort / argument conventions are
// touched.
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

static const int kTable[4][8] = {{100, -20, 10, 5, 5, 10, -20, 100},
                                 {-20, -50, -2, -2, -2, -2, -50, -20},
                                 {10, -2, -1, -1, -1, -1, -2, 10},
                                 {5, -2, -1, -1, -1, -1, -2, 5}};

static int leaf(uint64_t own, uint64_t opp, uint64_t lo, uint64_t lp) {
  int h = 0;
  for (int r = 0; r < 8; ++r)
    for (int c = 0; c < 8; ++c) {
      const int w = kTable[r < 4 ? r : 7 - r][c];
      h += w * ((int)((own >> (r * 8 + c)) & 1) - (int)((opp >> (r * 8 + c)) & 1));
    }
  return h + 12 * (azb::popc(lo) - azb::popc(lp));
}

static int negamax(uint64_t own, uint64_t opp, int depth) {
  const uint64_t lo = azb::legal(own, opp), lp = azb::legal(opp, own);
  if (!lo && !lp) {
    const int d = azb::popc(own) - azb::popc(opp);
    return d == 0 ? 0 : (d > 0 ? 10000 + 100 * d : -(10000 - 100 * d));
  }
  if (depth == 0) return leaf(own, opp, lo, lp);
  if (!lo) return -negamax(opp, own, depth);
  int best = -AZ_SEARCH_INF;
  for (uint64_t m = lo; m; m &= m - 1) {
    const int sq = __builtin_ctzll(m);
    const uint64_t f = azb::flips(own, opp, sq);
    const int v = -negamax(opp ^ f, (own | (1ull << sq)) ^ f, depth - 1);
    if (v > best) best = v;
  }
  return best;
}

int main() {
  std::vector<uint64_t> own, opp;
  while (own.size() < 300) {
    uint64_t o = azb::kInitOwn, p = azb::kInitOpp;
    int plies = (int)(rng() % 60);
    while (plies-- > 0) {
      uint64_t m = azb::legal(o, p);
      if (!m) {
        if (!azb::legal(p, o)) break;  // a finished game: a terminal root
        if (rng() % 2 == 0) break;  // keep the pass-only position as a root
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
  std::vector<int16_t> value(n), ev(n);
  std::vector<uint8_t> best(n);
  std::vector<uint64_t> nodes(n);
  int bad = 0;
  uint64_t total = 0;
  if (oth_eval_cpu(own.data(), opp.data(), n, ev.data()) != AZ_OK)
    return printf("oth_eval_cpu failed: %s\n", az_last_error()), 1;
  for (int64_t i = 0; i < n; ++i) bad += ev[i] != negamax(own[i], opp[i], 0);
  for (int depth = 1; depth <= 5; ++depth) {
    // deeper levels on fewer positions: the unpruned reference grows tenfold per ply
    const int64_t cnt = depth <= 3 ? n : (depth == 4 ? 100 : 30);
    int rc = oth_search_cpu(own.data(), opp.data(), cnt, depth, 1ull << 31, value.data(),
                            best.data(), nodes.data());
    if (rc != AZ_OK) return printf("oth_search_cpu failed: %s\n", az_last_error()), 1;
    for (int64_t i = 0; i < cnt; ++i) {
      total += nodes[i];
      const int want = negamax(own[i], opp[i], depth);
      int wbest = 64;
      for (uint64_t m = azb::legal(own[i], opp[i]); m; m &= m - 1) {
        const int sq = __builtin_ctzll(m);
        const uint64_t f = azb::flips(own[i], opp[i], sq);
        if (-negamax(opp[i] ^ f, (own[i] | (1ull << sq)) ^ f, depth - 1) == want) {
          wbest = sq;
          break;
        }
      }
      if (value[i] != want || best[i] != wbest || nodes[i] < 1) {
        ++bad;
        printf("depth %d position %lld: got (%d, %d), want (%d, %d)\n", depth, (long long)i,
               value[i], best[i], want, wbest);
      }
    }
  }
  // conventions: limit (1 and small), overlap, bad depth, NULL nodes, n = 0
  for (uint64_t limit : {1ull, 7ull}) {
    bad += oth_search_cpu(own.data(), opp.data(), n, 5, limit, value.data(), best.data(),
                          nullptr) != AZ_OK;
    for (int64_t i = 0; i < n; ++i) {
      const bool term = !azb::legal(own[i], opp[i]) && !azb::legal(opp[i], own[i]);
      if (term) bad += value[i] == AZ_SEARCH_ABORTED || best[i] != 64;
      if (!term && limit == 1) bad += value[i] != AZ_SEARCH_ABORTED || best[i] != 255;
    }
  }
  std::vector<uint64_t> both(n);
  for (int64_t i = 0; i < n; ++i) both[i] = own[i] | opp[i];
  bad += oth_search_cpu(both.data(), opp.data(), n, 3, 1000, value.data(), best.data(),
                        nodes.data()) != AZ_OK;
  for (int64_t i = 0; i < n; ++i)
    bad += value[i] != AZ_SEARCH_SKIPPED || best[i] != 255 || nodes[i] != 0;
  bad += oth_search_cpu(own.data(), opp.data(), n, 0, 1000, value.data(), best.data(), nullptr) !=
         AZ_ERR_ARG;
  bad += oth_search_cpu(own.data(), opp.data(), n, AZ_SEARCH_MAX_DEPTH + 1, 1000, value.data(),
                        best.data(), nullptr) != AZ_ERR_ARG;
  bad += oth_search_cpu(nullptr, nullptr, 0, 3, 1000, nullptr, nullptr, nullptr) != AZ_OK;
  bad += oth_eval_cpu(nullptr, nullptr, 0, nullptr) != AZ_OK;
  // the deepest stack: depth 10 under a node limit that ends every search
  bad += oth_search_cpu(own.data(), opp.data(), n, AZ_SEARCH_MAX_DEPTH, 20000, value.data(),
                        best.data(), nodes.data()) != AZ_OK;
  printf("search_host_check: %lld positions, %llu nodes, %d mismatches\n", (long long)n,
         (unsigned long long)total, bad);
  return bad != 0;
}
