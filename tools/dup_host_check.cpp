// dup_host_check.cpp — a stand-alone check of wfa_hip_duplicates_host, wfa_hip_duplicates_host_ex, wfa_hip_ops_clips and
// wfa_hip_qsum_host (pywfa_amd/csrc/host_dup.cpp) on fixed cases of the duplicate rule, its unclipped ends and its representative by
// base quality, meant to be built with the host statements under a sanitizer (no GPU, no Python):
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

struct Hit { int32_t i, j; uint8_t rev; int32_t score, status, ts, te; int32_t lead = 0, trail = 0; };

static int failures = 0;

// mates: empty for interleaved fragments, else (mate1, mate2) per fragment.  want_reads / want_pairs: the rows, row-major
// flags < 0: wfa_hip_duplicates_host; else wfa_hip_duplicates_host_ex with the hits' clips, `flags` and `qsum` (empty: NULL)
static void run_ex(const char* name, int64_t nreads, const std::vector<Hit>& hits, int64_t nfrag, const std::vector<int32_t>& mates,
                   const std::vector<int32_t>& text_len, int want_rc, const std::vector<int32_t>& want_reads,
                   const std::vector<int32_t>& want_pairs, int flags, const std::vector<int32_t>& qsum) {
  const size_t n = hits.size();
  std::vector<int32_t> i(n), j(n), score(n), status(n), ts(n), te(n), lead(n), trail(n), m1, m2;
  std::vector<uint8_t> rev(n);
  for (size_t h = 0; h < n; ++h) {
    i[h] = hits[h].i; j[h] = hits[h].j; rev[h] = hits[h].rev; score[h] = hits[h].score; status[h] = hits[h].status;
    ts[h] = hits[h].ts; te[h] = hits[h].te; lead[h] = hits[h].lead; trail[h] = hits[h].trail;
  }
  for (size_t f = 0; f + 1 < mates.size(); f += 2) { m1.push_back(mates[f]); m2.push_back(mates[f + 1]); }
  std::vector<int32_t> reads((size_t)(nreads > 0 ? nreads : 0) * WFA_HIP_DUP_COLS, 7), pairs((size_t)(nfrag > 0 ? nfrag : 0) * WFA_HIP_DUP_COLS, 7);
  char msg[256];
  int rc;
  if (flags < 0)
    rc = wfa_hip_duplicates_host(nreads, (int64_t)n, n ? i.data() : nullptr, n ? j.data() : nullptr, n ? rev.data() : nullptr,
                                 n ? score.data() : nullptr, n ? status.data() : nullptr, n ? ts.data() : nullptr, n ? te.data() : nullptr,
                                 INT32_MIN, 24, 0, 1000, 0, nfrag, mates.empty() ? nullptr : m1.data(), mates.empty() ? nullptr : m2.data(),
                                 (int64_t)text_len.size(), text_len.empty() ? nullptr : text_len.data(), reads.empty() ? nullptr : reads.data(),
                                 pairs.empty() ? nullptr : pairs.data(), msg, sizeof(msg));
  else
    rc = wfa_hip_duplicates_host_ex(nreads, (int64_t)n, n ? i.data() : nullptr, n ? j.data() : nullptr, n ? rev.data() : nullptr,
                                    n ? score.data() : nullptr, n ? status.data() : nullptr, n ? ts.data() : nullptr, n ? te.data() : nullptr,
                                    INT32_MIN, 24, 0, 1000, 0, nfrag, mates.empty() ? nullptr : m1.data(), mates.empty() ? nullptr : m2.data(),
                                    (int64_t)text_len.size(), text_len.empty() ? nullptr : text_len.data(), reads.empty() ? nullptr : reads.data(),
                                    pairs.empty() ? nullptr : pairs.data(), n ? lead.data() : nullptr, n ? trail.data() : nullptr, flags,
                                    qsum.empty() ? nullptr : qsum.data(), msg, sizeof(msg));
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

static void run(const char* name, int64_t nreads, const std::vector<Hit>& hits, int64_t nfrag, const std::vector<int32_t>& mates,
                const std::vector<int32_t>& text_len, int want_rc, const std::vector<int32_t>& want_reads,
                const std::vector<int32_t>& want_pairs) {
  run_ex(name, nreads, hits, nfrag, mates, text_len, want_rc, want_reads, want_pairs, -1, {});
}

static void check(const char* name, bool ok) {
  printf("%-64s %s\n", name, ok ? "ok" : "FAILED");
  if (!ok) ++failures;
}

// wfa_hip_ops_clips on one op string (heap-allocated at its exact size)
static void clips(const char* name, const std::vector<uint8_t>& ops, int32_t plen, int32_t tlen, int32_t want_lead, int32_t want_trail) {
  int32_t lead = 7, trail = 7;
  const int rc = wfa_hip_ops_clips(ops.empty() ? nullptr : ops.data(), (int64_t)ops.size(), plen, tlen, &lead, &trail);
  check(name, rc == WFA_HIP_OK && lead == want_lead && trail == want_trail);
}

static std::vector<uint8_t> ops_of(const char* head, size_t run, char c, const char* tail) {
  std::vector<uint8_t> v(head, head + strlen(head));
  v.insert(v.end(), run, (uint8_t)c);
  v.insert(v.end(), tail, tail + strlen(tail));
  return v;
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
  // ---- unclipped ends and the representative by base quality (wfa_hip_duplicates_host_ex) ----
  const int U = WFA_HIP_DUP_UNCLIPPED, Q = WFA_HIP_DUP_BY_QUALITY;
  const std::vector<Hit> fwd = {{0, 0, 0, 0, 0, 100, 150, 0, 0}, {1, 0, 0, -4, 0, 101, 150, 1, 0}};
  run_ex("flags 0 with clips: the core rule", 2, fwd, 0, {}, {500}, WFA_HIP_OK, {0, 1, 0, 0, 1, 1, 0, 0}, {}, 0, {});
  run_ex("unclipped: a first-base mismatch joins its group", 2, fwd, 0, {}, {500}, WFA_HIP_OK, {0, 2, 0, 0, 0, 2, 1, 0}, {}, U, {});
  run_ex("unclipped: reverse reads through trail", 2, {{0, 0, 1, 0, 0, 100, 150, 0, 0}, {1, 0, 1, -4, 0, 110, 148, 3, 2}}, 0, {}, {500}, WFA_HIP_OK,
         {0, 2, 0, 0, 0, 2, 1, 0}, {}, U, {});
  {
    std::vector<Hit> two = join({frag(0, 100, 350, -4, -4, false), frag(1, 101, 349, 0, 0, false)});
    two[2].lead = 1; two[3].trail = 1;
    run_ex("unclipped: a pair unit through lead of F and trail of R", 4, two, 2, {}, {500}, WFA_HIP_OK,
           {-1, 0, 1, 0, -1, 0, 1, 0, -1, 0, 0, 0, -1, 0, 0, 0}, {1, 2, 1, 0, 1, 2, 0, 0}, U, {});
    run_ex("the same by core: two groups", 4, two, 2, {}, {500}, WFA_HIP_OK, {-1, 0, 0, 0, -1, 0, 0, 0, -1, 0, 0, 0, -1, 0, 0, 0},
           {0, 1, 0, 0, 1, 1, 0, 0}, 0, {});
    run_ex("by quality: the sum of both mates decides", 4, two, 2, {}, {500}, WFA_HIP_OK, {-1, 0, 0, 0, -1, 0, 0, 0, -1, 0, 1, 0, -1, 0, 1, 0},
           {0, 2, 0, 0, 0, 2, 1, 0}, U | Q, {900, 900, 1000, 700});
    run_ex("by quality: saturated sums tie, the smaller number", 4, two, 2, {}, {500}, WFA_HIP_OK,
           {-1, 0, 0, 0, -1, 0, 0, 0, -1, 0, 1, 0, -1, 0, 1, 0}, {0, 2, 0, 0, 0, 2, 1, 0}, U | Q, {INT32_MAX, 5, INT32_MAX, INT32_MAX});
    run_ex("refused: an unknown flag bit", 4, two, 2, {}, {500}, WFA_HIP_EINVAL, {}, {}, 4, {});
    run_ex("refused: the quality flag without sums", 4, two, 2, {}, {500}, WFA_HIP_EINVAL, {}, {}, Q, {});
    run_ex("refused: sums without the quality flag", 4, two, 2, {}, {500}, WFA_HIP_EINVAL, {}, {}, U, {1, 1, 1, 1});
    run_ex("refused: a negative sum", 4, two, 2, {}, {500}, WFA_HIP_EINVAL, {}, {}, Q, {1, 1, -1, 1});
    two[1].lead = -1;
    run_ex("refused: a negative clip", 4, two, 2, {}, {500}, WFA_HIP_EINVAL, {}, {}, U, {});
  }
  run_ex("unclipped: b = -1 and b = tlen are alone, 0 and tlen - 1 are not", 8,
         {{0, 0, 0, 0, 0, 0, 50, 1, 0}, {1, 0, 0, 0, 0, 0, 50, 1, 0}, {2, 0, 1, 0, 0, 450, 500, 0, 1}, {3, 0, 1, 0, 0, 450, 500, 0, 1},
          {4, 0, 0, 0, 0, 1, 50, 1, 0}, {5, 0, 0, 0, 0, 0, 50, 0, 0}, {6, 0, 1, 0, 0, 450, 499, 0, 1}, {7, 0, 1, 0, 0, 450, 500, 0, 0}}, 0, {}, {500},
         WFA_HIP_OK, {0, 1, 0, 0, 1, 1, 0, 0, 2, 1, 0, 0, 3, 1, 0, 0, 4, 2, 0, 0, 4, 2, 1, 0, 6, 2, 0, 0, 6, 2, 1, 0}, {}, U, {});
  run_ex("unclipped: clips saturate at 65 535", 3,
         {{0, 0, 0, 0, 0, 70000, 70050, 65535, 0}, {1, 0, 0, 0, 0, 70000, 70050, 65536, 0}, {2, 0, 0, 0, 0, 70000, 70050, 65534, 0}}, 0, {}, {80000},
         WFA_HIP_OK, {0, 2, 0, 0, 0, 2, 1, 0, 2, 1, 0, 0}, {}, U, {});
  run_ex("unclipped: clips above the cap are one value", 4,
         {{0, 0, 0, 0, 0, 100, 150, 0, 0}, {1, 0, 1, 0, 0, 900, 1000, 0, INT32_MAX}, {2, 0, 0, 0, 0, 100, 150, 0, 0}, {3, 0, 1, 0, 0, 900, 1000, 0, 1 << 20}},
         2, {}, {5000}, WFA_HIP_OK, {-1, 0, 0, 0, -1, 0, 0, 0, -1, 0, 1, 0, -1, 0, 1, 0}, {0, 2, 0, 0, 0, 2, 1, 0}, U, {});
  {
    const int32_t top = INT32_MAX;
    const std::vector<Hit> far = {{0, 0, 0, 0, 0, top - 900, top - 850, 0, 0}, {1, 0, 1, 0, 0, top - 100, top, 0, 1},
                                  {2, 0, 0, 0, 0, top - 900, top - 850, 0, 0}, {3, 0, 1, 0, 0, top - 100, top, 0, 1}};
    run_ex("an end at INT32_MAX by core: one group", 4, far, 2, {}, {top}, WFA_HIP_OK, {-1, 0, 0, 0, -1, 0, 0, 0, -1, 0, 1, 0, -1, 0, 1, 0},
           {0, 2, 0, 0, 0, 2, 1, 0}, 0, {});
    run_ex("unclipped: a pair unit's end beyond int32 is alone", 4, far, 2, {}, {top}, WFA_HIP_OK,
           {-1, 0, 0, 0, -1, 0, 0, 0, -1, 0, 0, 0, -1, 0, 0, 0}, {0, 1, 0, 0, 1, 1, 0, 0}, U, {});
  }
  // ---- wfa_hip_ops_clips ----
  clips("clips: XM", ops_of("XM", 0, 'M', ""), 2, 2, 1, 0);
  clips("clips: DXM", ops_of("DXM", 0, 'M', ""), 3, 2, 2, 0);
  clips("clips: MX", ops_of("MX", 0, 'M', ""), 2, 2, 0, 1);
  clips("clips: MDD", ops_of("MDD", 0, 'M', ""), 3, 1, 0, 2);
  clips("clips: IIXMIMDXI", ops_of("IIXMIMDXI", 0, 'M', ""), 5, 7, 1, 2);
  clips("clips: no M", ops_of("XXDI", 0, 'M', ""), 3, 3, 0, 0);
  clips("clips: empty", {}, 0, 0, 0, 0);
  clips("clips: plen 0", ops_of("XM", 0, 'M', ""), 0, 2, 0, 0);
  clips("clips: 65 535 D in front", ops_of("", 65535, 'D', "M"), 65536, 1, 65535, 0);
  clips("clips: 65 536 D in front saturate", ops_of("", 65536, 'D', "M"), 65537, 1, 65535, 0);
  clips("clips: 70 000 X behind saturate", ops_of("M", 70000, 'X', ""), 70001, 70001, 0, 65535);
  {
    int32_t a = 7, b = 7;
    const std::vector<uint8_t> xm = ops_of("XM", 0, 'M', "");
    check("clips refused: a NULL output, NULL ops, negative lengths",
          wfa_hip_ops_clips(xm.data(), 2, 2, 2, nullptr, &b) == WFA_HIP_EINVAL && wfa_hip_ops_clips(xm.data(), 2, 2, 2, &a, nullptr) == WFA_HIP_EINVAL &&
          wfa_hip_ops_clips(nullptr, 2, 2, 2, &a, &b) == WFA_HIP_EINVAL && wfa_hip_ops_clips(xm.data(), -1, 2, 2, &a, &b) == WFA_HIP_EINVAL &&
          wfa_hip_ops_clips(xm.data(), 2, -1, 2, &a, &b) == WFA_HIP_EINVAL && wfa_hip_ops_clips(xm.data(), 2, 2, -1, &a, &b) == WFA_HIP_EINVAL &&
          a == 7 && b == 7);
  }
  // ---- wfa_hip_qsum_host ----
  {
    const std::vector<uint8_t> q = {0, 14, 15, 16, 93, 2};
    int32_t out = 7;
    check("qsum: min_quality 0", wfa_hip_qsum_host(q.data(), (int64_t)q.size(), 0, &out) == WFA_HIP_OK && out == 140);
    check("qsum: min_quality 15", wfa_hip_qsum_host(q.data(), (int64_t)q.size(), 15, &out) == WFA_HIP_OK && out == 124);
    check("qsum: min_quality 93", wfa_hip_qsum_host(q.data(), (int64_t)q.size(), 93, &out) == WFA_HIP_OK && out == 93);
    check("qsum: no bases", wfa_hip_qsum_host(nullptr, 0, 15, &out) == WFA_HIP_OK && out == 0);
    const std::vector<uint8_t> big((size_t)INT32_MAX / 93 + 1, 93);
    check("qsum: the greatest exact sum", wfa_hip_qsum_host(big.data(), (int64_t)big.size() - 1, 93, &out) == WFA_HIP_OK && out == 93 * (INT32_MAX / 93));
    check("qsum: saturated", wfa_hip_qsum_host(big.data(), (int64_t)big.size(), 0, &out) == WFA_HIP_OK && out == INT32_MAX);
    out = 7;
    check("qsum refused: min_quality 94 and -1, NULL pointers, a negative length",
          wfa_hip_qsum_host(q.data(), 6, 94, &out) == WFA_HIP_EINVAL && wfa_hip_qsum_host(q.data(), 6, -1, &out) == WFA_HIP_EINVAL &&
          wfa_hip_qsum_host(nullptr, 6, 15, &out) == WFA_HIP_EINVAL && wfa_hip_qsum_host(q.data(), -1, 15, &out) == WFA_HIP_EINVAL &&
          wfa_hip_qsum_host(q.data(), 6, 15, nullptr) == WFA_HIP_EINVAL && out == 7);
  }
  printf(failures ? "dup_host_check: %d FAILED\n" : "dup_host_check: ok\n", failures);
  return failures ? 1 : 0;
}
