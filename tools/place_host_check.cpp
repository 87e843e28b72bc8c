// place_host_check.cpp — a stand-alone check of wfa_hip_place_host (pywfa_amd/csrc/host_place.cpp) on the edge cases of the placement
// rule, meant to be built with the host statement under a sanitizer (no GPU, no Python):
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude tools/place_host_check.cpp
//       pywfa_amd/csrc/host_place.cpp -o place_host_check     (one command), then ./place_host_check
// Every array is heap-allocated at its exact size, so that a read or write past an end is seen.
#include <limits.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "wfa_hip.h"

struct Hit { int32_t i, j; uint8_t rev; int32_t score, status, ts, te; };

static int failures = 0;

static void run(const char* name, int64_t nreads, const std::vector<Hit>& hits, int32_t min_score, int32_t full_gap, int want_rc,
                const std::vector<int32_t>& want_rows, const std::vector<uint8_t>& want_flags, bool with_reverse = true) {
  const size_t n = hits.size();
  std::vector<int32_t> i(n), j(n), score(n), status(n), ts(n), te(n);
  std::vector<uint8_t> rev(n), flags(n, 9);
  for (size_t h = 0; h < n; ++h) {
    i[h] = hits[h].i; j[h] = hits[h].j; rev[h] = hits[h].rev; score[h] = hits[h].score; status[h] = hits[h].status;
    ts[h] = hits[h].ts; te[h] = hits[h].te;
  }
  std::vector<int32_t> rows((size_t)(nreads > 0 ? nreads : 0) * WFA_HIP_PLACE_COLS, 7);
  char msg[256];
  const int rc = wfa_hip_place_host(nreads, (int64_t)n, n ? i.data() : nullptr, n ? j.data() : nullptr, with_reverse && n ? rev.data() : nullptr,
                                    n ? score.data() : nullptr, n ? status.data() : nullptr, n ? ts.data() : nullptr, n ? te.data() : nullptr,
                                    min_score, full_gap, rows.empty() ? nullptr : rows.data(), n ? flags.data() : nullptr, msg, sizeof(msg));
  bool ok = rc == want_rc;
  if (ok && rc == WFA_HIP_OK) ok = rows == want_rows && flags == want_flags;
  if (ok && rc != WFA_HIP_OK) ok = msg[0] != 0;
  printf("%-58s %s\n", name, ok ? "ok" : "FAILED");
  if (!ok) {
    ++failures;
    printf("  rc %d (want %d) msg '%s'\n  rows:", rc, want_rc, msg);
    for (int32_t v : rows) printf(" %d", v);
    printf("\n  flags:");
    for (uint8_t v : flags) printf(" %d", v);
    printf("\n");
  }
}

int main() {
  const int32_t MIN = INT32_MIN, MAX = INT32_MAX;
  run("no hits", 2, {}, MIN, 24, WFA_HIP_OK, {-1, MIN, MIN, 0, 0, 0, 0, 0, -1, MIN, MIN, 0, 0, 0, 0, 0}, {});
  run("no reads, no hits", 0, {}, MIN, 1, WFA_HIP_OK, {}, {});
  run("all ineligible", 1, {{0, 0, 0, -4, 1, 0, 100}, {0, 0, 0, -9, 0, 0, 100}}, -8, 24, WFA_HIP_OK, {-1, MIN, MIN, 0, 0, 0, 0, 0}, {0, 0});
  run("one hit", 2, {{1, 2, 1, -12, 0, 30, 180}}, MIN, 24, WFA_HIP_OK, {-1, MIN, MIN, 0, 0, 0, 0, 0, 0, -12, MIN, 60, 1, 0, 30, 180}, {3});
  run("a tie broken by the hit number", 1, {{0, 0, 0, -8, 0, 500, 650}, {0, 0, 0, -8, 0, 0, 150}}, MIN, 24, WFA_HIP_OK,
      {0, -8, -8, 0, 2, 1, 500, 650}, {3, 1});
  run("2 ov == min on the right, one base less", 1, {{0, 0, 0, 0, 0, 0, 100}, {0, 0, 0, -4, 0, 50, 150}, {0, 0, 0, -8, 0, 51, 151}}, MIN, 24,
      WFA_HIP_OK, {0, 0, -8, 20, 3, 0, 0, 100}, {3, 2, 1});
  run("2 ov == min on the left, one base less", 1, {{0, 0, 0, -8, 0, 49, 149}, {0, 0, 0, -4, 0, 50, 150}, {0, 0, 0, 0, 0, 100, 200}}, MIN, 24,
      WFA_HIP_OK, {2, 0, -8, 20, 3, 0, 100, 200}, {1, 2, 3});
  run("an empty interval inside the primary", 1, {{0, 0, 0, 0, 0, 0, 100}, {0, 0, 0, -3, 0, 40, 40}}, MIN, 1, WFA_HIP_OK,
      {0, 0, -3, 60, 2, 0, 0, 100}, {3, 1});
  run("another strand at the same place", 1, {{0, 1, 0, -4, 0, 10, 160}, {0, 1, 1, -6, 0, 10, 160}}, MIN, 4, WFA_HIP_OK,
      {0, -4, -6, 30, 2, 0, 10, 160}, {3, 1});
  run("... which is the same place without strands", 1, {{0, 1, 0, -4, 0, 10, 160}, {0, 1, 1, -6, 0, 10, 160}}, MIN, 4, WFA_HIP_OK,
      {0, -4, MIN, 60, 2, 0, 10, 160}, {3, 2}, false);
  run("full_gap - 1 behind", 1, {{0, 0, 0, -10, 0, 0, 9}, {0, 0, 0, -33, 0, 50, 59}}, MIN, 24, WFA_HIP_OK, {0, -10, -33, 57, 2, 0, 0, 9}, {3, 1});
  run("full_gap behind", 1, {{0, 0, 0, -10, 0, 0, 9}, {0, 0, 0, -34, 0, 50, 59}}, MIN, 24, WFA_HIP_OK, {0, -10, -34, 60, 2, 0, 0, 9}, {3, 1});
  run("full_gap + 1 behind", 1, {{0, 0, 0, -10, 0, 0, 9}, {0, 0, 0, -35, 0, 50, 59}}, MIN, 24, WFA_HIP_OK, {0, -10, -35, 60, 2, 0, 0, 9}, {3, 1});
  run("a runner-up at INT32_MIN", 1, {{0, 0, 0, MIN + 5, 0, 0, 9}, {0, 1, 0, MIN, 0, 0, 9}}, MIN, 24, WFA_HIP_OK,
      {0, MIN + 5, MIN, 12, 2, 0, 0, 9}, {3, 1});
  run("the extremes of score and interval", 1, {{0, 0, 0, MAX, 0, 0, MAX}, {0, 0, 0, MIN, 0, 1, MAX}, {0, 1, 0, MIN, 0, 0, MAX}}, MIN, MAX,
      WFA_HIP_OK, {0, MAX, MIN, 60, 3, 0, 0, MAX}, {3, 2, 1});
  run("refused: i outside the reads", 3, {{0, 0, 0, 0, 0, 0, 1}, {3, 0, 0, 0, 0, 0, 1}}, MIN, 24, WFA_HIP_EINVAL, {}, {});
  run("refused: a negative j", 3, {{0, -1, 0, 0, 0, 0, 1}}, MIN, 24, WFA_HIP_EINVAL, {}, {});
  run("refused: a negative text_start", 3, {{0, 0, 0, 0, 0, -1, 1}}, MIN, 24, WFA_HIP_EINVAL, {}, {});
  run("refused: text_end below text_start", 3, {{0, 0, 0, 0, 0, 5, 4}}, MIN, 24, WFA_HIP_EINVAL, {}, {});
  run("refused: full_gap 0", 3, {{0, 0, 0, 0, 0, 0, 1}}, MIN, 0, WFA_HIP_EINVAL, {}, {});
  // a group that is long, interleaved with another read's
  std::vector<Hit> many;
  for (int h = 0; h < 1000; ++h) many.push_back({h & 1, h % 3, (uint8_t)(h % 2), -(h % 7), h % 11 == 0 ? 1 : 0, 10 * (h % 13), 10 * (h % 13) + 50});
  std::vector<int32_t> rows(2 * WFA_HIP_PLACE_COLS);
  std::vector<uint8_t> flags(1000);
  {
    std::vector<int32_t> i, j, score, status, ts, te;
    std::vector<uint8_t> rev;
    for (const Hit& h : many) { i.push_back(h.i); j.push_back(h.j); rev.push_back(h.rev); score.push_back(h.score); status.push_back(h.status); ts.push_back(h.ts); te.push_back(h.te); }
    const int rc = wfa_hip_place_host(2, 1000, i.data(), j.data(), rev.data(), score.data(), status.data(), ts.data(), te.data(), -5, 3,
                                      rows.data(), flags.data(), nullptr, 0);
    const bool ok = rc == WFA_HIP_OK && rows[0] == 14 && rows[1] == 0 && rows[8] == 7 && rows[9] == 0;   // the first eligible hits of score 0
    printf("%-58s %s\n", "1000 interleaved hits of two reads", ok ? "ok" : "FAILED");
    failures += ok ? 0 : 1;
  }
  printf(failures ? "%d FAILED\n" : "all ok\n", failures);
  return failures ? 1 : 0;
}
