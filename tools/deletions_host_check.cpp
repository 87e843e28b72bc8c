// deletions_host_check.cpp — a stand-alone check of wfa_hip_ops_deletions and wfa_hip_deletions_host (pywfa_amd/csrc/host_cigar.cpp)
// on hand-made op strings and rows, meant to be built with the host statements under a sanitizer (no GPU, no Python):
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude tools/deletions_host_check.cpp
//       pywfa_amd/csrc/host_cigar.cpp -o deletions_host_check     (one command), then ./deletions_host_check
// Every array is heap-allocated at its exact size, so that a read or write past an end is seen.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "wfa_hip.h"

static int failures = 0;

static void report(const char* name, bool ok) {
  printf("%-66s %s\n", name, ok ? "ok" : "FAILED");
  failures += ok ? 0 : 1;
}

// "41M3I49M" -> one letter per op
static std::vector<uint8_t> expand(const char* cigar) {
  std::vector<uint8_t> out;
  for (const char* p = cigar; *p;) {
    char* end = nullptr;
    const long n = strtol(p, &end, 10);
    out.insert(out.end(), (size_t)n, (uint8_t)*end);
    p = end + 1;
  }
  return out;
}

// the records of `cigar` against `want` (h, n, h, n, ...), with every capacity from 0 to two above the count
static void ops(const char* name, const char* cigar, int slack_p, int slack_t, std::vector<int32_t> want) {
  const std::vector<uint8_t> o = expand(cigar);
  int32_t plen = slack_p, tlen = slack_t;
  for (uint8_t c : o) { plen += (c == 'M' || c == 'X' || c == 'D'); tlen += (c == 'M' || c == 'X' || c == 'I'); }
  const int64_t n = (int64_t)want.size() / 2;
  bool ok = true;
  for (int64_t cap = 0; cap <= n + 2; ++cap) {
    std::vector<int32_t> recs((size_t)cap * 2, -7);
    int64_t count = -1;
    const int rc = wfa_hip_ops_deletions(o.empty() ? nullptr : o.data(), (int64_t)o.size(), plen, tlen, cap, &count, cap ? recs.data() : nullptr);
    ok = ok && rc == WFA_HIP_OK && count == n;
    for (int64_t k = 0; k < cap; ++k)
      for (int x = 0; x < 2; ++x) ok = ok && recs[(size_t)(2 * k + x)] == (k < n ? want[(size_t)(2 * k + x)] : -7);
  }
  report(name, ok);
}

struct Rec { int64_t row; int32_t n; };

// the rows of wfa_hip_deletions_host over `len` rows of depth `depth[g]` (all of it in column 0 but the column-5 share `del5[g]`)
static void host(const char* name, std::vector<int32_t> depth, std::vector<int32_t> del5, std::vector<Rec> records, int32_t min_depth,
                 int32_t permille, std::vector<std::vector<int32_t>> want) {
  const int64_t len = (int64_t)depth.size();
  std::vector<int32_t> counts((size_t)len * WFA_HIP_PILEUP_COLS, 0), starts((size_t)len, 0);
  for (int64_t g = 0; g < len; ++g) { counts[(size_t)g * 8] = depth[(size_t)g] - del5[(size_t)g]; counts[(size_t)g * 8 + 5] = del5[(size_t)g]; }
  std::vector<int64_t> row;
  std::vector<int32_t> n;
  for (const Rec& r : records) {
    row.push_back(r.row); n.push_back(r.n);
    if (r.row >= 0 && r.row < len) starts[(size_t)r.row] += 1;
  }
  const int64_t nw = (int64_t)want.size();
  bool ok = true;
  for (int64_t cap = 0; cap <= nw + 2; ++cap) {
    std::vector<int32_t> rows((size_t)cap * WFA_HIP_DELETION_COLS, -7);
    int64_t count = -1;
    const int rc = wfa_hip_deletions_host(len ? counts.data() : nullptr, len ? starts.data() : nullptr, len, 3, 100, min_depth, permille,
                                          (int64_t)row.size(), row.empty() ? nullptr : row.data(), n.empty() ? nullptr : n.data(), cap, &count,
                                          cap ? rows.data() : nullptr);
    ok = ok && rc == WFA_HIP_OK && count == nw;
    for (int64_t k = 0; k < cap; ++k)
      for (int x = 0; x < WFA_HIP_DELETION_COLS; ++x)
        ok = ok && rows[(size_t)(k * WFA_HIP_DELETION_COLS + x)] == (k < nw ? want[(size_t)k][(size_t)x] : -7);
  }
  report(name, ok);
}

int main() {
  unsetenv("WFA_HIP_DEL_MAX_READS");
  ops("one run", "41M3I49M", 0, 0, {41, 3});
  ops("two runs, an X beside the second", "5M1I3M1X2I4M", 1, 2, {5, 1, 10, 2});
  ops("runs in front of and behind the core are no records", "2I1M1X3I1D1M1I1M2I", 0, 0, {4, 3, 8, 1});
  ops("an I run directly followed by a D run", "3M3I2D3M", 0, 0, {3, 3});
  ops("a D run directly followed by an I run", "2M2D3I1M1X1I1M", 0, 0, {2, 3, 7, 1});
  ops("alternating I and D", "1M1I1D1I1D1I1M", 0, 0, {1, 1, 2, 1, 3, 1});
  ops("a run of 70, longer than a round", "30M70I90M", 0, 0, {30, 70});
  ops("a run that fills ops 64 .. 127", "64M64I2M", 0, 0, {64, 64});
  ops("a run that ends at op 63", "59M5I9M", 0, 0, {59, 5});
  ops("a run that starts at op 64", "64M5I9M", 0, 0, {64, 5});
  ops("a run that ends at op 127, a D, a run from op 129", "123M5I1D5I2M", 0, 0, {123, 5, 128, 5});
  ops("no M", "2X1I", 0, 0, {});
  ops("only I", "3I", 0, 0, {});
  ops("length 1", "1M", 0, 0, {});
  ops("empty", "", 0, 0, {});
  {
    const std::vector<uint8_t> o = expand("2M1I2M");
    std::vector<int32_t> recs(4, -7);
    int64_t count = -1;
    bool ok = wfa_hip_ops_deletions(o.data(), 5, 3, 5, 2, &count, recs.data()) == WFA_HIP_EINVAL &&       // the ops consume more pattern
              wfa_hip_ops_deletions(o.data(), 5, 4, 4, 2, &count, recs.data()) == WFA_HIP_EINVAL &&       // ... more text
              wfa_hip_ops_deletions(o.data(), -1, 4, 5, 2, &count, recs.data()) == WFA_HIP_EINVAL && wfa_hip_ops_deletions(nullptr, 5, 4, 5, 2, &count, recs.data()) == WFA_HIP_EINVAL &&
              wfa_hip_ops_deletions(o.data(), 5, 4, 5, -1, &count, recs.data()) == WFA_HIP_EINVAL && wfa_hip_ops_deletions(o.data(), 5, 4, 5, 2, nullptr, recs.data()) == WFA_HIP_EINVAL &&
              wfa_hip_ops_deletions(o.data(), 5, 4, 5, 2, &count, nullptr) == WFA_HIP_EINVAL;
    ok = ok && count == -1 && recs == std::vector<int32_t>(4, -7);
    report("refused: ops that outrun the pair, negative values, missing pointers", ok);
  }

  // rows: j = 3, pos = 100 + row, depth, S, allele_count, allele_len, alleles, overflow
  host("two lengths, 5 against 4", {9, 9, 9, 9, 9}, {0, 9, 9, 4, 4}, {{1, 2}, {1, 4}, {1, 2}, {1, 4}, {1, 2}, {1, 4}, {1, 2}, {1, 4}, {1, 2}}, 8, 500,
       {{3, 101, 9, 9, 5, 2, 2, 0}});
  host("an exact tie: the shorter", {8, 8, 8, 8}, {8, 8, 4, 0}, {{0, 3}, {0, 2}, {0, 3}, {0, 2}, {0, 3}, {0, 2}, {0, 3}, {0, 2}}, 1, 500, {{3, 100, 8, 8, 4, 2, 2, 0}});
  host("a nested deletion is a row of its own", {11, 11, 11, 11}, {6, 11, 11, 6}, {{0, 4}, {0, 4}, {0, 4}, {0, 4}, {0, 4}, {0, 4}, {1, 2}, {1, 2}, {1, 2}, {1, 2}, {1, 2}},
       1, 200, {{3, 100, 11, 6, 6, 4, 1, 0}, {3, 101, 11, 5, 5, 2, 1, 0}});
  host("... and below the bar at min_frac 0.5", {11, 11, 11, 11}, {6, 11, 11, 6}, {{0, 4}, {0, 4}, {0, 4}, {0, 4}, {0, 4}, {0, 4}, {1, 2}, {1, 2}, {1, 2}, {1, 2}, {1, 2}},
       1, 500, {{3, 100, 11, 6, 6, 4, 1, 0}});
  host("the majority rule: 2 S > depth", {4, 4, 5}, {2, 2, 3}, {{0, 1}, {0, 1}, {2, 9}, {2, 9}, {2, 8}}, 1, 0, {{3, 102, 5, 3, 2, 9, 2, 0}});
  host("min_depth", {3, 8}, {3, 8}, {{0, 1}, {0, 1}, {0, 1}, {1, 1}, {1, 1}, {1, 1}, {1, 1}, {1, 1}, {1, 1}, {1, 1}, {1, 1}}, 8, 1, {{3, 101, 8, 8, 8, 1, 1, 0}});
  host("records outside the rows are skipped; a run may reach past them", {2, 2}, {0, 2}, {{-1, 5}, {1, 70}, {1, 70}, {2, 1}, {7, 3}}, 1, 1000, {{3, 101, 2, 2, 2, 70, 1, 0}});
  host("no rows", {}, {}, {{0, 1}}, 1, 500, {});
  host("no records", {5, 5}, {0, 0}, {}, 1, 1, {});
  setenv("WFA_HIP_DEL_MAX_READS", "3", 1);
  host("the limit lowered to 3: an overflow row", {4, 4}, {4, 3}, {{0, 1}, {0, 1}, {0, 2}, {0, 2}, {1, 6}, {1, 6}, {1, 7}}, 1, 500,
       {{3, 100, 4, 4, 0, 0, 0, 1}, {3, 101, 4, 3, 2, 6, 2, 0}});
  setenv("WFA_HIP_DEL_MAX_READS", "0", 1);
  host("the limit is at least 1", {4, 4}, {1, 2}, {{0, 5}, {1, 6}, {1, 6}}, 1, 1, {{3, 100, 4, 1, 1, 5, 1, 0}, {3, 101, 4, 2, 0, 0, 0, 1}});
  unsetenv("WFA_HIP_DEL_MAX_READS");
  {
    const std::vector<int32_t> counts(16, 1), starts(2, 1);
    const std::vector<int64_t> row = {0, 1};
    std::vector<int32_t> n = {1, 1}, rows(16, -7);
    int64_t count = -1;
    const auto call = [&](const int32_t* c, const int32_t* s, int64_t len, int32_t md, int32_t pm, int64_t nrec, const int64_t* rr, const int32_t* rn, int64_t cap,
                          int64_t* cnt, int32_t* out) { return wfa_hip_deletions_host(c, s, len, 0, 0, md, pm, nrec, rr, rn, cap, cnt, out); };
    bool ok = call(counts.data(), starts.data(), 2, 1, 1, 2, row.data(), n.data(), 2, &count, rows.data()) == WFA_HIP_OK && count == 2;
    count = -1; rows.assign(16, -7);
    ok = ok && call(nullptr, starts.data(), 2, 1, 500, 2, row.data(), n.data(), 2, &count, rows.data()) == WFA_HIP_EINVAL &&
         call(counts.data(), nullptr, 2, 1, 500, 2, row.data(), n.data(), 2, &count, rows.data()) == WFA_HIP_EINVAL &&
         call(counts.data(), starts.data(), -1, 1, 500, 2, row.data(), n.data(), 2, &count, rows.data()) == WFA_HIP_EINVAL &&
         call(counts.data(), starts.data(), 2, 0, 500, 2, row.data(), n.data(), 2, &count, rows.data()) == WFA_HIP_EINVAL &&
         call(counts.data(), starts.data(), 2, 1, -1, 2, row.data(), n.data(), 2, &count, rows.data()) == WFA_HIP_EINVAL &&
         call(counts.data(), starts.data(), 2, 1, 1001, 2, row.data(), n.data(), 2, &count, rows.data()) == WFA_HIP_EINVAL &&
         call(counts.data(), starts.data(), 2, 1, 500, -2, row.data(), n.data(), 2, &count, rows.data()) == WFA_HIP_EINVAL &&
         call(counts.data(), starts.data(), 2, 1, 500, 2, nullptr, n.data(), 2, &count, rows.data()) == WFA_HIP_EINVAL &&
         call(counts.data(), starts.data(), 2, 1, 500, 2, row.data(), nullptr, 2, &count, rows.data()) == WFA_HIP_EINVAL &&
         call(counts.data(), starts.data(), 2, 1, 500, 2, row.data(), n.data(), -1, &count, rows.data()) == WFA_HIP_EINVAL &&
         call(counts.data(), starts.data(), 2, 1, 500, 2, row.data(), n.data(), 2, nullptr, rows.data()) == WFA_HIP_EINVAL &&
         call(counts.data(), starts.data(), 2, 1, 500, 2, row.data(), n.data(), 2, &count, nullptr) == WFA_HIP_EINVAL;
    n[1] = 0;
    ok = ok && call(counts.data(), starts.data(), 2, 1, 500, 2, row.data(), n.data(), 2, &count, rows.data()) == WFA_HIP_EINVAL;
    ok = ok && count == -1 && rows == std::vector<int32_t>(16, -7);
    report("refused: parameters out of range, missing pointers, a record of length 0", ok);
  }
  printf(failures ? "%d FAILED\n" : "all ok\n", failures);
  return failures ? 1 : 0;
}
