// pair_host_check.cpp — a stand-alone check of wfa_hip_pair_host (pywfa_amd/csrc/host_pair.cpp) on the edge cases of the pairing rule,
// meant to be built with the host statements under a sanitizer (no GPU, no Python):
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude tools/pair_host_check.cpp
//       pywfa_amd/csrc/host_pair.cpp pywfa_amd/csrc/host_place.cpp -o pair_host_check     (one command), then ./pair_host_check
// Every array is heap-allocated at its exact size, so that a read or write past an end is seen.
#include <limits.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "wfa_hip.h"

struct Hit { int32_t i, j; uint8_t rev; int32_t score, status, ts, te; };
struct Par { int32_t min_score = INT32_MIN, full_gap = 24, min_insert = 0, max_insert = 1000, unpaired = 0; };
typedef std::vector<std::vector<int32_t>> Mates;   // empty: interleaved

static int failures = 0;

static void run(const char* name, int64_t nreads, const std::vector<Hit>& hits, int64_t nfrag, const Mates& mates, Par par, int want_rc,
                const std::vector<int32_t>& want_rows, const std::vector<uint8_t>& want_flags, bool with_outputs = true) {
  const size_t n = hits.size();
  std::vector<int32_t> i(n), j(n), score(n), status(n), ts(n), te(n), m1, m2;
  std::vector<uint8_t> rev(n), flags(n, 9), pair_flags(n, 9);
  for (size_t h = 0; h < n; ++h) {
    i[h] = hits[h].i; j[h] = hits[h].j; rev[h] = hits[h].rev; score[h] = hits[h].score; status[h] = hits[h].status;
    ts[h] = hits[h].ts; te[h] = hits[h].te;
  }
  for (const std::vector<int32_t>& m : mates) { m1.push_back(m[0]); m2.push_back(m[1]); }
  std::vector<int32_t> rows((size_t)(nreads > 0 ? nreads : 0) * WFA_HIP_PLACE_COLS, 7);
  std::vector<int32_t> pair_rows((size_t)(nfrag > 0 ? nfrag : 0) * WFA_HIP_PAIR_COLS, 7);
  char msg[256];
  const int rc = wfa_hip_pair_host(nreads, (int64_t)n, n ? i.data() : nullptr, n ? j.data() : nullptr, n ? rev.data() : nullptr,
                                   n ? score.data() : nullptr, n ? status.data() : nullptr, n ? ts.data() : nullptr, n ? te.data() : nullptr,
                                   par.min_score, par.full_gap, par.min_insert, par.max_insert, par.unpaired, nfrag,
                                   mates.empty() ? nullptr : m1.data(), mates.empty() ? nullptr : m2.data(),
                                   with_outputs && !rows.empty() ? rows.data() : nullptr, with_outputs && n ? flags.data() : nullptr,
                                   pair_rows.empty() ? nullptr : pair_rows.data(), with_outputs && n ? pair_flags.data() : nullptr, msg, sizeof(msg));
  bool ok = rc == want_rc;
  if (ok && rc == WFA_HIP_OK) ok = pair_rows == want_rows && (!with_outputs || pair_flags == want_flags);
  if (ok && rc != WFA_HIP_OK) {   // a message, and nothing written
    ok = msg[0] != 0;
    for (int32_t v : rows) ok = ok && v == 7;
    for (int32_t v : pair_rows) ok = ok && v == 7;
    for (size_t h = 0; h < n; ++h) ok = ok && flags[h] == 9 && pair_flags[h] == 9;
  }
  printf("%-66s %s\n", name, ok ? "ok" : "FAILED");
  if (!ok) {
    ++failures;
    printf("  rc %d (want %d) msg '%s'\n  pair rows:", rc, want_rc, msg);
    for (int32_t v : pair_rows) printf(" %d", v);
    printf("\n  pair flags:");
    for (uint8_t v : pair_flags) printf(" %d", v);
    printf("\n");
  }
}

int main() {
  const int32_t MIN = INT32_MIN, MAX = INT32_MAX;
  const int OK = WFA_HIP_OK, BAD = WFA_HIP_EINVAL;
  const std::vector<Hit> one = {{0, 0, 0, -4, 0, 100, 250}, {1, 0, 1, -4, 0, 300, 450}};
  const std::vector<int32_t> alone = {0, 1, 0, MIN, MIN, 0, 60, 60, 0, 0, 0, 0}, joined = {0, 1, 1, -8, MIN, 60, 60, 60, 350, 1, 0, 0};
  Par p;
  run("no reads, no hits, no fragments", 0, {}, 0, {}, p, OK, {}, {});
  run("no hits", 2, {}, 1, {}, p, OK, {-1, -1, 0, MIN, MIN, 0, 0, 0, 0, 0, 0, 0}, {});
  run("no fragment", 2, one, 0, {}, p, OK, {}, {3, 3});
  run("one proper pairing", 2, one, 1, {}, p, OK, joined, {3, 3});
  run("... without the nullable outputs", 2, one, 1, {}, p, OK, joined, {}, false);
  run("a mate without a hit", 2, {{0, 0, 0, -4, 0, 100, 250}}, 1, {}, p, OK, {0, -1, 0, MIN, MIN, 0, 60, 0, 0, 0, 0, 0}, {3});
  run("the same strand", 2, {{0, 0, 0, -4, 0, 100, 250}, {1, 0, 0, -4, 0, 300, 450}}, 1, {}, p, OK, alone, {3, 3});
  run("two texts", 2, {{0, 0, 0, -4, 0, 100, 250}, {1, 1, 1, -4, 0, 300, 450}}, 1, {}, p, OK, alone, {3, 3});
  run("the reverse hit in front of the forward one", 2, {{0, 0, 0, -4, 0, 300, 450}, {1, 0, 1, -4, 0, 100, 250}}, 1, {}, p, OK, alone, {3, 3});
  run("the reverse hit starts a base early", 2, {{0, 0, 0, -4, 0, 100, 250}, {1, 0, 1, -4, 0, 99, 300}}, 1, {}, p, OK, alone, {3, 3});
  run("the forward hit ends a base late", 2, {{0, 0, 0, -4, 0, 100, 400}, {1, 0, 1, -4, 0, 200, 399}}, 1, {}, p, OK, alone, {3, 3});
  run("an empty interval", 2, {{0, 0, 0, -4, 0, 100, 100}, {1, 0, 1, -4, 0, 300, 450}}, 1, {}, p, OK, alone, {3, 3});
  p.min_insert = 350; p.max_insert = 350;
  run("insert at both bounds", 2, one, 1, {}, p, OK, joined, {3, 3});
  p.min_insert = 351; p.max_insert = 1000;
  run("insert below min_insert", 2, one, 1, {}, p, OK, alone, {3, 3});
  p.min_insert = 0; p.max_insert = 349;
  run("insert above max_insert", 2, one, 1, {}, p, OK, alone, {3, 3});
  p = Par();
  const std::vector<Hit> un = {{0, 0, 0, -4, 0, 100, 250}, {0, 1, 0, -20, 0, 100, 250}, {1, 1, 1, -6, 0, 300, 450}, {1, 0, 0, 0, 0, 5000, 5150}};
  p.unpaired = 21;
  run("rejected by unpaired", 2, un, 1, {}, p, OK, {0, 3, 0, MIN, MIN, 0, 40, 15, 0, 1, 0, 0}, {3, 1, 1, 3});
  p.unpaired = 22;
  run("accepted at the boundary of unpaired", 2, un, 1, {}, p, OK, {1, 2, 1, -26, MIN, 60, 60, 60, 350, 1, 0, 0}, {1, 3, 3, 1});
  p = Par();
  run("runner-ups at the same place and at others", 2,
      {{0, 0, 0, -4, 0, 100, 250}, {0, 0, 0, -8, 0, 110, 260}, {1, 0, 1, -4, 0, 300, 450}, {0, 0, 0, -8, 0, 600, 750}, {1, 0, 1, -6, 0, 800, 950}},
      1, {}, p, OK, {0, 2, 1, -8, -10, 5, 10, 5, 350, 5, 0, 0}, {3, 2, 3, 1, 1});
  p.unpaired = 24;
  run("a chosen hit off its read's single-end locus", 2,
      {{0, 0, 0, 0, 0, 5000, 5150}, {0, 0, 0, -10, 0, 100, 250}, {1, 0, 1, -4, 0, 300, 450}, {1, 0, 1, -4, 0, 700, 850}}, 1, {}, p, OK,
      {1, 2, 1, -14, -14, 0, 0, 0, 350, 2, 1, 0}, {1, 3, 3, 1});
  p = Par();
  run("pair scores above INT32_MAX", 2, {{0, 0, 0, MAX, 0, 100, 250}, {1, 0, 1, MAX, 0, 300, 450}, {1, 0, 1, MAX - 1, 0, 700, 850}}, 1, {}, p, OK,
      {0, 1, 1, MAX, MAX, 2, 60, 2, 350, 2, 0, 0}, {3, 3, 1});
  run("pair scores below INT32_MIN", 2, {{0, 0, 0, MIN, 0, 100, 250}, {1, 0, 1, MIN, 0, 300, 450}, {1, 0, 1, MIN, 0, 700, 850}}, 1, {}, p, OK,
      {0, 1, 1, MIN + 1, MIN + 1, 0, 60, 0, 350, 2, 1, 0}, {3, 3, 1});
  run("the extremes of the intervals", 2, {{0, 0, 0, -1, 0, 0, MAX}, {1, 0, 1, -1, 0, 0, MAX}}, 1, {}, p, OK, alone, {3, 3});
  p.max_insert = MAX;
  run("... and of max_insert", 2, {{0, 0, 0, -1, 0, 0, MAX}, {1, 0, 1, -1, 0, 0, MAX}}, 1, {}, p, OK, {0, 1, 1, -2, MIN, 60, 60, 60, MAX, 1, 0, 0}, {3, 3});
  p = Par();
  run("mates as arrays, the second fragment first, a read in none", 5,
      {{2, 0, 0, -4, 0, 100, 250}, {0, 0, 1, -4, 0, 300, 450}, {1, 0, 1, 0, 0, 300, 450}, {4, 0, 0, -2, 0, 1, 9}}, 2, {{3, 1}, {0, 2}}, p, OK,
      {-1, 2, 0, MIN, MIN, 0, 0, 60, 0, 0, 0, 0, 1, 0, 1, -8, MIN, 60, 60, 60, 350, 1, 0, 0}, {3, 3, 3, 3});
  // 256 x 256 eligible pairings are joined, 257 x 256 are not
  for (int n1 = 256; n1 <= 257; ++n1) {
    std::vector<Hit> blk;
    for (int h = 0; h < n1; ++h) blk.push_back({0, 0, 0, h ? -1 : 0, 0, 100, 250});
    for (int g = 0; g < 256; ++g) blk.push_back({1, 0, 1, g ? -1 : 0, 0, 300, 450});
    std::vector<uint8_t> fl((size_t)n1 + 256, 2);
    fl[0] = 3; fl[(size_t)n1] = 3;
    if (n1 == 256) run("256 x 256 pairings", 2, blk, 1, {}, p, OK, {0, 256, 1, 0, MIN, 60, 60, 60, 350, 65536, 0, 0}, fl);
    else run("257 x 256 pairings: overflow", 2, blk, 1, {}, p, OK, {0, 257, 0, MIN, MIN, 0, 60, 60, 0, 0, 0, 1}, fl);
  }
  // refusals: a message, nothing written
  run("refused: what the placement rule refuses", 2, {{0, 0, 0, -4, 0, 5, 4}}, 1, {}, p, BAD, {}, {});
  run("refused: a negative nfrag", 2, one, -1, {}, p, BAD, {}, {});
  run("refused: 2 nfrag > nreads, interleaved", 3, one, 2, {}, p, BAD, {}, {});
  run("refused: a mate outside the reads", 4, one, 2, {{0, 1}, {2, 4}}, p, BAD, {}, {});
  run("refused: a negative mate", 4, one, 1, {{-1, 1}}, p, BAD, {}, {});
  run("refused: a fragment of one read", 4, one, 2, {{0, 1}, {3, 3}}, p, BAD, {}, {});
  run("refused: a read named by two fragments", 4, one, 2, {{0, 1}, {2, 0}}, p, BAD, {}, {});
  run("refused: the last read named twice (the bitmap's last bit)", 64, one, 2, {{63, 1}, {2, 63}}, p, BAD, {}, {});
  p.min_insert = -1;
  run("refused: min_insert < 0", 2, one, 1, {}, p, BAD, {}, {});
  p.min_insert = 10; p.max_insert = 9;
  run("refused: max_insert < min_insert", 2, one, 1, {}, p, BAD, {}, {});
  p = Par(); p.unpaired = -1;
  run("refused: unpaired < 0", 2, one, 1, {}, p, BAD, {}, {});
  p = Par(); p.full_gap = 0;
  run("refused: full_gap 0", 2, one, 1, {}, p, BAD, {}, {});
  {   // exactly one of the mate arrays
    std::vector<int32_t> m(1, 0), pr(WFA_HIP_PAIR_COLS, 7);
    char msg[256];
    const int rc1 = wfa_hip_pair_host(2, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, MIN, 24, 0, 1000, 0, 1, m.data(), nullptr,
                                      nullptr, nullptr, pr.data(), nullptr, msg, sizeof(msg));
    const int rc2 = wfa_hip_pair_host(2, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, MIN, 24, 0, 1000, 0, 1, nullptr, m.data(),
                                      nullptr, nullptr, pr.data(), nullptr, nullptr, 0);
    const bool ok = rc1 == BAD && rc2 == BAD && msg[0] != 0 && pr == std::vector<int32_t>(WFA_HIP_PAIR_COLS, 7);
    printf("%-66s %s\n", "refused: exactly one of mate1 / mate2", ok ? "ok" : "FAILED");
    failures += ok ? 0 : 1;
  }
  printf(failures ? "%d FAILED\n" : "all ok\n", failures);
  return failures ? 1 : 0;
}
