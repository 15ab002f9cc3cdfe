// records_host_check.hip — stand-alone host check of oth_records_cpu for sanitizer builds
// (never loaded into Python, never run on a GPU):
//
//   cd alphazero-othello_amd && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 \
//     -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//     -DAZ_BUILD_ID='"check"' ../scripts/records_host_check.hip csrc/records.hip csrc/board.hip \
//     -o /tmp/records_host_check && /tmp/records_host_check
//
// 600 seeded random playouts shaped like the tests' fixture -- passes written and left out,
// lines cut short, one entry overwritten by a random byte, strides 64 / 80 / 128, with and
// without start positions and winners, pass rows on and off, row limits that overflow -- into
// output buffers of exactly max_rows * n elements, so a store past a row limit or a game's
// line is an error the sanitizer reports.  Every game is also replayed by a plain
// legal-mask loop of this file's own (not records.h) and the row counts, statuses, stop
// indices and final positions compared.
#include <stdio.h>
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

struct Want {
  int rows, status, bad;
  uint64_t own, opp;
  int colour;
};

// the rules of include/az_othello.h restated on the legal mask
static Want replay(const uint8_t* line, int stride, uint64_t own, uint64_t opp, int max_rows,
                   bool pass_rows) {
  Want w{0, -1, 255, own, opp, 1};
  auto swap = [&] {
    const uint64_t t = w.own;
    w.own = w.opp;
    w.opp = t;
    w.colour = -w.colour;
  };
  for (int i = 0; i < stride && w.status < 0; ++i) {
    const int a = line[i];
    if (a == 255) break;
    const uint64_t m = azb::legal(w.own, w.opp), mo = azb::legal(w.opp, w.own);
    bool ok = false;
    if (a < 64)
      ok = ((m ? m : mo) >> a) & 1;  // the mover's placement, or the opponent's after a pass
    else if (a == 64)
      ok = !m && mo;
    if (!ok) {
      w.status = AZ_REC_ILLEGAL;
      w.bad = i;
      break;
    }
    if (a < 64 && !m) {  // the inserted pass
      if (pass_rows) {
        if (w.rows >= max_rows) {
          w.status = AZ_REC_OVERFLOW;
          w.bad = i;
          break;
        }
        ++w.rows;
      }
      swap();
    }
    if (a == 64 ? pass_rows : true) {
      if (w.rows >= max_rows) {
        w.status = AZ_REC_OVERFLOW;
        w.bad = i;
        break;
      }
      ++w.rows;
    }
    if (a == 64) {
      swap();
    } else {
      const uint64_t f = azb::flips(w.own, w.opp, a);
      const uint64_t no = w.opp ^ f, np = (w.own | (1ull << a)) ^ f;
      w.own = no;
      w.opp = np;
      w.colour = -w.colour;
    }
  }
  if (w.status < 0)
    w.status = (azb::legal(w.own, w.opp) || azb::legal(w.opp, w.own)) ? AZ_REC_UNFINISHED
                                                                     : AZ_REC_TERMINAL;
  return w;
}

int main() {
  const int n = 600;
  int bad = 0;
  long long total_rows = 0;
  const int strides[3] = {64, 80, 128};
  for (int cfg = 0; cfg < 24; ++cfg) {
    const int stride = strides[cfg % 3];
    const bool pass_rows = (cfg / 3) & 1, written = (cfg / 6) & 1, starts = (cfg / 12) & 1;
    const int max_rows = cfg % 4 == 3 ? 37 : (cfg % 4 == 2 ? 128 : stride);
    std::vector<uint8_t> acts((size_t)n * stride, 255);
    std::vector<uint64_t> own0(n), opp0(n);
    std::vector<int8_t> winner(n);
    for (int g = 0; g < n; ++g) {
      uint64_t o = azb::kInitOwn, p = azb::kInitOpp;
      int len = 0, skip = starts ? (int)(rng() % 12) : 0;
      own0[g] = o;
      opp0[g] = p;
      uint8_t* line = &acts[(size_t)g * stride];
      while (len < stride) {
        uint64_t m = azb::legal(o, p);
        int a = 64;
        if (!m) {
          if (!azb::legal(p, o)) break;
          const uint64_t t = o;
          o = p;
          p = t;
        } else {
          int k = (int)(rng() % (uint64_t)azb::popc(m));
          while (k--) m &= m - 1;
          a = __builtin_ctzll(m);
          const uint64_t f = azb::flips(o, p, a);
          const uint64_t no = p ^ f, np = (o | (1ull << a)) ^ f;
          o = no;
          p = np;
        }
        if (skip > 0) {  // still before the start position
          --skip;
          own0[g] = o;
          opp0[g] = p;
          continue;
        }
        if (a < 64 || written) line[len++] = (uint8_t)a;
      }
      const int kind = (int)(rng() % 3);
      if (kind == 1) {  // cut short
        len = (int)(rng() % (uint64_t)(len + 1));
        memset(line + len, 255, (size_t)(stride - len));
      }
      if (kind == 2 && len > 0) line[rng() % (uint64_t)len] = (uint8_t)rng();
      winner[g] = (int8_t)((int)(rng() % 3) - 1);
    }
    const size_t rows = (size_t)max_rows * n;
    std::vector<uint64_t> own_o(rows), opp_o(rows), fown(n), fopp(n);
    std::vector<uint8_t> act_o(rows), ply_o(rows), status(n), badp(n);
    std::vector<int8_t> z_o(rows), fcol(n), fdiff(n);
    std::vector<int32_t> n_rows(n);
    const int rc = oth_records_cpu(acts.data(), stride, starts ? own0.data() : nullptr,
                                   starts ? opp0.data() : nullptr,
                                   cfg & 1 ? winner.data() : nullptr, n, max_rows,
                                   pass_rows ? AZ_REC_PASS_ROWS : 0, own_o.data(), opp_o.data(),
                                   act_o.data(), z_o.data(), ply_o.data(), n_rows.data(),
                                   status.data(), badp.data(), fown.data(), fopp.data(),
                                   fcol.data(), fdiff.data());
    if (rc != AZ_OK) return printf("oth_records_cpu failed: %s\n", az_last_error()), 1;
    for (int g = 0; g < n; ++g) {
      const Want w = replay(&acts[(size_t)g * stride], stride, own0[g], opp0[g], max_rows,
                            pass_rows);
      total_rows += n_rows[g];
      const bool same = w.rows == n_rows[g] && w.status == status[g] && w.bad == badp[g] &&
                        w.own == fown[g] && w.opp == fopp[g] && w.colour == fcol[g];
      if (!same) {
        ++bad;
        printf("cfg %d game %d: got (%d, %d, %d), want (%d, %d, %d)\n", cfg, g, n_rows[g],
               status[g], badp[g], w.rows, w.status, w.bad);
      }
    }
  }
  // conventions: n = 0 with null buffers, bad stride, bad row limit
  bad += oth_records_cpu(nullptr, 64, nullptr, nullptr, nullptr, 0, 64, 0, nullptr, nullptr,
                         nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                         nullptr, nullptr) != AZ_OK;
  bad += oth_records_cpu(nullptr, 24, nullptr, nullptr, nullptr, 0, 64, 0, nullptr, nullptr,
                         nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                         nullptr, nullptr) != AZ_ERR_ARG;
  bad += oth_records_cpu(nullptr, 64, nullptr, nullptr, nullptr, 0, 129, 0, nullptr, nullptr,
                         nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                         nullptr, nullptr) != AZ_ERR_ARG;
  printf("records_host_check: 24 configurations x %d games, %lld rows, %d mismatches\n", n,
         total_rows, bad);
  return bad != 0;
}
