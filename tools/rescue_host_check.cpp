// rescue_host_check.cpp — a stand-alone check of wfa_hip_rescue_host (pywfa_amd/csrc/host_rescue.cpp) on fixed cases of the rescue
// rule, meant to be built with the host statements under a sanitizer (no GPU, no Python):
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude tools/rescue_host_check.cpp
//       pywfa_amd/csrc/host_rescue.cpp pywfa_amd/csrc/host_pair.cpp pywfa_amd/csrc/host_place.cpp -o rescue_host_check
//   (one command), then ./rescue_host_check
// Every array is heap-allocated at its exact size, so that a read or write past an end is seen.
#include <limits.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "wfa_hip.h"

struct Hit { int32_t i, j; uint8_t rev; int32_t score, status, ts, te; };
struct Par { int32_t min_insert, max_insert, pad, min_len, anchor_mapq; };

static int failures = 0;

static void run(const char* name, int64_t nreads, const std::vector<Hit>& hits, int64_t nfrag, const std::vector<int32_t>& mates,
                const std::vector<int32_t>& read_len, const std::vector<int32_t>& text_len, Par par, int64_t cap, int want_rc,
                int64_t want_count, const std::vector<int32_t>& want_rows) {
  const size_t n = hits.size();
  std::vector<int32_t> i(n), j(n), score(n), status(n), ts(n), te(n), m1, m2;
  std::vector<uint8_t> rev(n);
  for (size_t h = 0; h < n; ++h) {
    i[h] = hits[h].i; j[h] = hits[h].j; rev[h] = hits[h].rev; score[h] = hits[h].score; status[h] = hits[h].status;
    ts[h] = hits[h].ts; te[h] = hits[h].te;
  }
  for (size_t f = 0; f + 1 < mates.size(); f += 2) { m1.push_back(mates[f]); m2.push_back(mates[f + 1]); }
  std::vector<int32_t> rows((size_t)(cap > 0 ? cap : 0) * WFA_HIP_RESCUE_COLS, 7);
  int64_t count = -9;
  char msg[256];
  const int rc = wfa_hip_rescue_host(nreads, (int64_t)n, n ? i.data() : nullptr, n ? j.data() : nullptr, n ? rev.data() : nullptr,
                                     n ? score.data() : nullptr, n ? status.data() : nullptr, n ? ts.data() : nullptr, n ? te.data() : nullptr,
                                     INT32_MIN, 24, par.min_insert, par.max_insert, 0, nfrag, mates.empty() ? nullptr : m1.data(),
                                     mates.empty() ? nullptr : m2.data(), read_len.empty() ? nullptr : read_len.data(),
                                     (int64_t)text_len.size(), text_len.empty() ? nullptr : text_len.data(), par.pad, par.min_len,
                                     par.anchor_mapq, cap, &count, rows.empty() ? nullptr : rows.data(), msg, sizeof(msg));
  bool ok = rc == want_rc;
  if (ok && rc == WFA_HIP_OK) {
    ok = count == want_count;
    const size_t written = (size_t)(count < cap ? count : cap) * WFA_HIP_RESCUE_COLS;
    for (size_t q = 0; ok && q < rows.size(); ++q) ok = rows[q] == (q < written ? want_rows[q] : 7);
  }
  if (ok && rc != WFA_HIP_OK) {
    ok = msg[0] != 0 && count == -9;
    for (int32_t v : rows) ok = ok && v == 7;
  }
  printf("%-64s %s\n", name, ok ? "ok" : "FAILED");
  if (!ok) {
    ++failures;
    printf("  rc %d (want %d) count %lld (want %lld) msg '%s'\n  rows:", rc, want_rc, (long long)count, (long long)want_count, msg);
    for (int32_t v : rows) printf(" %d", v);
    printf("\n");
  }
}

int main() {
  const int32_t MAX = INT32_MAX;
  const Par P{150, 600, 16, 0, 0};
  const std::vector<Hit> one = {{0, 0, 0, -4, 0, 1000, 1150}};
  const std::vector<Hit> two = {{0, 0, 0, -4, 0, 100, 250}, {1, 1, 1, -4, 0, 100, 250}};
  run("no reads, no texts, no fragments", 0, {}, 0, {}, {}, {}, P, 0, WFA_HIP_OK, 0, {});
  run("no hits: no anchor", 2, {}, 1, {}, {150, 100}, {5000}, P, 2, WFA_HIP_OK, 0, {});
  run("a forward anchor", 2, one, 1, {}, {150, 100}, {5000}, P, 2, WFA_HIP_OK, 1, {1, 0, 1034, 582, 1, 0, 0, 0});
  run("a reverse anchor", 2, {{0, 0, 1, -4, 0, 1000, 1150}}, 1, {}, {150, 100}, {5000}, P, 2, WFA_HIP_OK, 1, {1, 0, 534, 582, 0, 0, 0, 0});
  run("two windows, clipped at 0 and at the text's end", 2, two, 1, {}, {150, 100}, {5000, 300}, P, 2, WFA_HIP_OK, 2,
      {1, 0, 134, 582, 1, 0, 0, 0, 0, 1, 0, 266, 0, 0, 1, 0});
  run("cap below the count", 2, two, 1, {}, {150, 100}, {5000, 300}, P, 1, WFA_HIP_OK, 2, {1, 0, 134, 582, 1, 0, 0, 0});
  run("the counting call", 2, two, 1, {}, {150, 100}, {5000, 300}, P, 0, WFA_HIP_OK, 2, {});
  run("min_len drops the clipped window", 2, two, 1, {}, {150, 100}, {5000, 300}, Par{150, 600, 16, 267, 0}, 2, WFA_HIP_OK, 1,
      {1, 0, 134, 582, 1, 0, 0, 0});
  run("a proper pairing is not rescued", 2, {{0, 0, 0, -4, 0, 1000, 1150}, {1, 0, 1, -4, 0, 1300, 1450}}, 1, {}, {150, 100}, {5000}, P, 2,
      WFA_HIP_OK, 0, {});
  run("an empty interval is no anchor", 2, {{0, 0, 0, -4, 0, 1000, 1000}}, 1, {}, {150, 100}, {5000}, P, 2, WFA_HIP_OK, 0, {});
  run("anchor_mapq refuses a tie", 2, {{0, 0, 0, -4, 0, 1000, 1150}, {0, 0, 0, -4, 0, 3000, 3150}}, 1, {}, {150, 100}, {5000},
      Par{150, 600, 16, 0, 1}, 2, WFA_HIP_OK, 0, {});
  run("ts and max_insert next to 2^31 - 1", 2, {{0, 0, 0, -4, 0, MAX - 200, MAX - 50}}, 1, {}, {150, 100}, {MAX}, Par{0, MAX, 16, 0, 0}, 2,
      WFA_HIP_OK, 1, {1, 0, MAX - 316, 316, 1, 0, 0, 0});
  run("pad of 2^31 - 1 on a reverse anchor", 2, {{0, 0, 1, -4, 0, 10, 160}}, 1, {}, {150, 100}, {MAX}, Par{0, MAX, MAX, 0, 0}, 2, WFA_HIP_OK, 1,
      {1, 0, 0, MAX, 0, 0, 0, 0});
  run("mates as arrays, backwards", 4, {{2, 0, 0, -4, 0, 1000, 1150}}, 2, {3, 2, 1, 0}, {1, 2, 3, 40}, {5000}, P, 4, WFA_HIP_OK, 1,
      {3, 0, 1094, 522, 1, 0, 0, 0});
  run("refused: j past the texts", 2, two, 1, {}, {150, 100}, {5000}, P, 2, WFA_HIP_EINVAL, 0, {});
  run("refused: a negative pad", 2, one, 1, {}, {150, 100}, {5000}, Par{150, 600, -1, 0, 0}, 2, WFA_HIP_EINVAL, 0, {});
  run("refused: anchor_mapq = 61", 2, one, 1, {}, {150, 100}, {5000}, Par{150, 600, 16, 0, 61}, 2, WFA_HIP_EINVAL, 0, {});
  run("refused: a negative read length", 2, one, 1, {}, {150, -1}, {5000}, P, 2, WFA_HIP_EINVAL, 0, {});
  run("refused: a negative text length", 2, one, 1, {}, {150, 100}, {-5}, P, 2, WFA_HIP_EINVAL, 0, {});
  run("refused: what the pairing refuses (a read in two fragments)", 4, one, 2, {0, 1, 1, 2}, {1, 2, 3, 4}, {5000}, P, 2, WFA_HIP_EINVAL, 0, {});
  run("refused: a negative cap", 2, one, 1, {}, {150, 100}, {5000}, P, -1, WFA_HIP_EINVAL, 0, {});
  printf(failures ? "rescue_host_check: %d FAILED\n" : "rescue_host_check: ok\n", failures);
  return failures ? 1 : 0;
}
