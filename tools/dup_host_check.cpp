// dup_host_check.cpp — a stand-alone check of wfa_hip_duplicates_host (pywfa_amd/csrc/host_dup.cpp) on fixed cases of the duplicate
// rule, meant to be built with the host statements under a sanitizer (no GPU, no Python):
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude tools/dup_host_check.cpp
//       pywfa_amd/csrc/host_dup.cpp pywfa_amd/csrc/host_pair.cpp pywfa_amd/csrc/host_place.cpp -o dup_host_check
//   (one command), then ./dup_host_check
// Every array is heap-allocated at its exact size, so that a read or write past an end is seen.
#include <limits.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "wfa_hip.h"

struct Hit { int32_t i, j; uint8_t rev; int32_t score, status, ts, te; };

static int failures = 0;

// mates: empty for interleaved fragments, else (mate1, mate2) per fragment.  want_reads / want_pairs: the rows, row-major
static void run(const char* name, int64_t nreads, const std::vector<Hit>& hits, int64_t nfrag, const std::vector<int32_t>& mates,
                const std::vector<int32_t>& text_len, int want_rc, const std::vector<int32_t>& want_reads,
                const std::vector<int32_t>& want_pairs) {
  const size_t n = hits.size();
  std::vector<int32_t> i(n), j(n), score(n), status(n), ts(n), te(n), m1, m2;
  std::vector<uint8_t> rev(n);
  for (size_t h = 0; h < n; ++h) {
    i[h] = hits[h].i; j[h] = hits[h].j; rev[h] = hits[h].rev; score[h] = hits[h].score; status[h] = hits[h].status;
    ts[h] = hits[h].ts; te[h] = hits[h].te;
  }
  for (size_t f = 0; f + 1 < mates.size(); f += 2) { m1.push_back(mates[f]); m2.push_back(mates[f + 1]); }
  std::vector<int32_t> reads((size_t)(nreads > 0 ? nreads : 0) * WFA_HIP_DUP_COLS, 7), pairs((size_t)(nfrag > 0 ? nfrag : 0) * WFA_HIP_DUP_COLS, 7);
  char msg[256];
  const int rc = wfa_hip_duplicates_host(nreads, (int64_t)n, n ? i.data() : nullptr, n ? j.data() : nullptr, n ? rev.data() : nullptr,
                                         n ? score.data() : nullptr, n ? status.data() : nullptr, n ? ts.data() : nullptr,
                                         n ? te.data() : nullptr, INT32_MIN, 24, 0, 1000, 0, nfrag, mates.empty() ? nullptr : m1.data(),
                                         mates.empty() ? nullptr : m2.data(), (int64_t)text_len.size(),
                                         text_len.empty() ? nullptr : text_len.data(), reads.empty() ? nullptr : reads.data(),
                                         pairs.empty() ? nullptr : pairs.data(), msg, sizeof(msg));
  bool ok = rc == want_rc;
  if (ok && rc == WFA_HIP_OK) ok = reads == want_reads && pairs == want_pairs;
  if (ok && rc != WFA_HIP_OK) {
    ok = msg[0] != 0;
    for (int32_t v : reads) ok = ok && v == 7;
    for (int32_t v : pairs) ok = ok && v == 7;
  }
  printf("%-64s %s\n", name, ok ? "ok" : "FAILED");
  if (!ok) {
    ++failures;
    printf("  rc %d (want %d) msg '%s'\n  read rows:", rc, want_rc, msg);
    for (int32_t v : reads) printf(" %d", v);
    printf("\n  pair rows:");
    for (int32_t v : pairs) printf(" %d", v);
    printf("\n");
  }
}

int main() {
  // a fragment: mate 1 forward at [100, 150), mate 2 reverse at [300, 350)
  auto frag = [](int32_t f, int32_t ts, int32_t te, int32_t s1, int32_t s2, bool flip) {
    return std::vector<Hit>{{2 * f, 0, (uint8_t)(flip ? 1 : 0), s1, 0, flip ? te - 50 : ts, flip ? te : ts + 50},
                            {2 * f + 1, 0, (uint8_t)(flip ? 0 : 1), s2, 0, flip ? ts : te - 50, flip ? ts + 50 : te}};
  };
  auto join = [](std::vector<std::vector<Hit>> parts) {
    std::vector<Hit> all;
    for (auto& p : parts) all.insert(all.end(), p.begin(), p.end());
    return all;
  };
  run("no reads, no texts, no fragments", 0, {}, 0, {}, {}, WFA_HIP_OK, {}, {});
  run("no hits: no unit", 2, {}, 1, {}, {500}, WFA_HIP_OK, {-1, 0, 0, 0, -1, 0, 0, 0}, {-1, 0, 0, 0});
  run("one fragment: alone", 2, frag(0, 100, 350, -4, -4, false), 1, {}, {500}, WFA_HIP_OK, {-1, 0, 0, 0, -1, 0, 0, 0}, {0, 1, 0, 0});
  run("two copies: the better score is the representative", 4, join({frag(0, 100, 350, -4, -4, false), frag(1, 100, 350, 0, -4, false)}), 2,
      {}, {500}, WFA_HIP_OK, {-1, 0, 1, 0, -1, 0, 1, 0, -1, 0, 0, 0, -1, 0, 0, 0}, {1, 2, 1, 0, 1, 2, 0, 0});
  run("a tie: the smaller number", 4, join({frag(0, 100, 350, -4, 0, false), frag(1, 100, 350, 0, -4, false)}), 2, {}, {500}, WFA_HIP_OK,
      {-1, 0, 0, 0, -1, 0, 0, 0, -1, 0, 1, 0, -1, 0, 1, 0}, {0, 2, 0, 0, 0, 2, 1, 0});
  run("F1R2 and F2R1 with the same ends: two groups", 4, join({frag(0, 100, 350, -4, -4, false), frag(1, 100, 350, 0, 0, true)}), 2, {}, {500},
      WFA_HIP_OK, {-1, 0, 0, 0, -1, 0, 0, 0, -1, 0, 0, 0, -1, 0, 0, 0}, {0, 1, 0, 0, 1, 1, 0, 0});
  run("the same start, another end: two groups", 4, join({frag(0, 100, 350, -4, -4, false), frag(1, 100, 351, 0, 0, false)}), 2, {}, {500},
      WFA_HIP_OK, {-1, 0, 0, 0, -1, 0, 0, 0, -1, 0, 0, 0, -1, 0, 0, 0}, {0, 1, 0, 0, 1, 1, 0, 0});
  run("mates as arrays, backwards", 4, join({frag(0, 100, 350, -4, -4, false), frag(1, 100, 350, 0, 0, false)}), 2, {1, 0, 3, 2}, {500},
      WFA_HIP_OK, {-1, 0, 1, 0, -1, 0, 1, 0, -1, 0, 0, 0, -1, 0, 0, 0}, {1, 2, 1, 0, 1, 2, 0, 0});
  run("single-end: forward reads by their start", 3, {{0, 0, 0, -4, 0, 10, 60}, {1, 0, 0, -2, 0, 10, 50}, {2, 0, 0, 0, 0, 11, 60}}, 0, {}, {500},
      WFA_HIP_OK, {1, 2, 1, 0, 1, 2, 0, 0, 2, 1, 0, 0}, {});
  run("single-end: reverse reads of two lengths by their end", 3, {{0, 0, 1, -4, 0, 10, 60}, {1, 0, 1, -4, 0, 20, 60}, {2, 0, 0, 0, 0, 59, 99}}, 0,
      {}, {500}, WFA_HIP_OK, {0, 2, 0, 0, 0, 2, 1, 0, 2, 1, 0, 0}, {});
  run("a reverse read that ends with its text; position 0", 2, {{0, 0, 1, -4, 0, 450, 500}, {1, 0, 0, -4, 0, 0, 50}}, 0, {}, {500}, WFA_HIP_OK,
      {0, 1, 0, 0, 1, 1, 0, 0}, {});
  run("b outside the text: alone", 2, {{0, 0, 0, -4, 0, 500, 550}, {1, 0, 0, -4, 0, 500, 550}}, 0, {}, {500}, WFA_HIP_OK,
      {0, 1, 0, 0, 1, 1, 0, 0}, {});
  run("an ineligible hit, an empty interval: no units", 2, {{0, 0, 0, -4, 1, 10, 60}, {1, 0, 0, -4, 0, 10, 10}}, 0, {}, {500}, WFA_HIP_OK,
      {-1, 0, 0, 0, -1, 0, 0, 0}, {});
  run("a fragment that is not proper: its mates are read units", 4,
      {{0, 0, 0, -4, 0, 10, 60}, {1, 1, 1, -4, 0, 10, 60}, {2, 0, 0, 0, 0, 10, 60}}, 1, {}, {500, 500}, WFA_HIP_OK,
      {2, 2, 1, 0, 1, 1, 0, 0, 2, 2, 0, 0, -1, 0, 0, 0}, {-1, 0, 0, 0});
  {
    // one bucket of WFA_HIP_DUP_MAX_BUCKET + 1 forward reads is not resolved; with one read less it is
    for (int extra = 0; extra < 2; ++extra) {
      const int32_t n = WFA_HIP_DUP_MAX_BUCKET + extra;
      std::vector<Hit> hits;
      std::vector<int32_t> want;
      for (int32_t r = 0; r < n; ++r) {
        hits.push_back(Hit{r, 0, 0, r == 5 ? 0 : -4, 0, 10, 60});
        const int32_t row[4] = {extra ? r : 5, extra ? 1 : n, extra ? 0 : (r == 5 ? 0 : 1), extra};
        want.insert(want.end(), row, row + 4);
      }
      run(extra ? "4 097 units in one bucket: overflow" : "4 096 units in one bucket: one group", n, hits, 0, {}, {500}, WFA_HIP_OK, want, {});
    }
  }
  run("refused: j past the texts", 2, {{0, 1, 0, -4, 0, 10, 60}}, 0, {}, {500}, WFA_HIP_EINVAL, {}, {});
  run("refused: a negative text length", 2, {{0, 0, 0, -4, 0, 10, 60}}, 0, {}, {-5}, WFA_HIP_EINVAL, {}, {});
  run("refused: what the pairing refuses (a read in two fragments)", 4, {{0, 0, 0, -4, 0, 10, 60}}, 2, {0, 1, 1, 2}, {500}, WFA_HIP_EINVAL, {}, {});
  run("refused: what the placement refuses (a read past the reads)", 2, {{2, 0, 0, -4, 0, 10, 60}}, 1, {}, {500}, WFA_HIP_EINVAL, {}, {});
  printf(failures ? "dup_host_check: %d FAILED\n" : "dup_host_check: ok\n", failures);
  return failures ? 1 : 0;
}
