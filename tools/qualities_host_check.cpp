// qualities_host_check.cpp — a stand-alone check of wfa_hip_ops_pileup_quals and wfa_hip_genotypes_quals_host
// (pywfa_amd/csrc/host_cigar.cpp) on hand-made op strings at the edges of the rule of "base qualities", meant to be built with the
// host statements under a sanitizer (no GPU, no Python):
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude tools/qualities_host_check.cpp
//       pywfa_amd/csrc/host_cigar.cpp -o qualities_host_check     (one command), then ./qualities_host_check
// Every array is heap-allocated at its exact size, so that a read or write past an end is seen: the I that takes the qualities of
// positions v - 1 and v is the place where an index could leave the pattern.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "wfa_hip.h"

static int failures = 0;

static void report(const char* name, bool ok) {
  printf("%-74s %s\n", name, ok ? "ok" : "FAILED");
  failures += ok ? 0 : 1;
}

// one pair under (min_base_quality, quality_cap): the rows and the quality rows, heap arrays of the exact sizes
struct Pair {
  std::vector<int32_t> rows, qrows;
  int rc;
  Pair(const char* ops, const char* pattern, std::vector<uint8_t> quals, int32_t tlen, int32_t mbq, int32_t cap)
      : rows((size_t)tlen * 8, 0), qrows((size_t)tlen * 8, 0) {
    const std::vector<uint8_t> o(ops, ops + strlen(ops)), p(pattern, pattern + strlen(pattern));
    rc = wfa_hip_ops_pileup_quals(o.empty() ? nullptr : o.data(), (int64_t)o.size(), p.empty() ? nullptr : p.data(), (int32_t)p.size(), tlen,
                                  quals.empty() ? nullptr : quals.data(), mbq, cap, rows.empty() ? nullptr : rows.data(),
                                  qrows.empty() ? nullptr : qrows.data());
  }
  int32_t c(int h, int col) const { return rows[(size_t)h * 8 + col]; }
  int32_t q(int h, int col) const { return qrows[(size_t)h * 8 + col]; }
  int64_t sum(const std::vector<int32_t>& v) const { int64_t s = 0; for (int32_t x : v) s += x; return s; }
};

int main() {
  {  // an I directly after the core's first M: min(Qc(0), Qc(1)); the C under it (Q 10) is filtered at 13
    const Pair p("MIMM", "ACG", {30, 10, 50}, 4, 13, 40);
    report("an I directly after the core's first M", p.rc == WFA_HIP_OK && p.c(0, 0) == 1 && p.q(0, 0) == 30 && p.c(1, 5) == 1 && p.q(1, 5) == 10 &&
                                                         p.sum(p.rows) == 3 && p.c(3, 2) == 1 && p.q(3, 2) == 40 && p.sum(p.qrows) == 80);
  }
  {  // a D run as the last op before the last M: counted at the last M's row, with the quality of its FIRST base
    const Pair p("MMDDM", "ACGTA", {30, 31, 7, 90, 33}, 3, 0, 40);
    report("a D run as the last op before the last M", p.rc == WFA_HIP_OK && p.c(2, 6) == 1 && p.q(2, 6) == 7 && p.c(2, 0) == 1 && p.q(2, 0) == 33 &&
                                                           p.sum(p.rows) == 4 && p.sum(p.qrows) == 30 + 31 + 7 + 33);
  }
  {  // a pair whose only M is one base: the Xs in front of it and the gaps behind it are outside the core
    const Pair p("XXMIID", "ACGT", {40, 41, 12, 9}, 5, 0, 93);
    report("a pair whose only M is one base", p.rc == WFA_HIP_OK && p.sum(p.rows) == 1 && p.c(2, 2) == 1 && p.sum(p.qrows) == 12);
  }
  {  // min_base_quality = 0 gives the rows of wfa_hip_ops_pileup
    const char* ops = "DMXIMDDMIIM";
    const char* pat = "TACGNACT";
    const Pair p(ops, pat, {1, 13, 12, 93, 2, 40, 41, 0}, 8, 0, 40);
    std::vector<int32_t> plain(8 * 8, 0);
    const int rc = wfa_hip_ops_pileup((const uint8_t*)ops, (int64_t)strlen(ops), (const uint8_t*)pat, 8, 8, plain.data());
    report("min_base_quality = 0 gives the rows of wfa_hip_ops_pileup", p.rc == WFA_HIP_OK && rc == WFA_HIP_OK && plain == p.rows && p.sum(p.qrows) > 0);
    // and at 93 no M or X is left, while the gaps count as before
    const Pair f(ops, pat, {1, 13, 12, 93, 2, 40, 41, 0}, 8, 93, 93);
    int64_t letters = 0;
    for (int h = 0; h < 8; ++h) for (int col : {0, 1, 2, 3, 4, 7}) letters += f.c(h, col);
    bool gaps = true;
    for (int h = 0; h < 8; ++h) gaps = gaps && f.c(h, 5) == plain[(size_t)h * 8 + 5] && f.c(h, 6) == plain[(size_t)h * 8 + 6];
    report("min_base_quality = 93: only the base of quality 93 and the gaps remain", f.rc == WFA_HIP_OK && letters == 1 && gaps);
  }
  {  // an X under the threshold adds nothing at all, not even the mismatch; the cap of 1
    const Pair p("MXM", "ANG", {13, 12, 14}, 3, 13, 1);
    report("an X under the threshold adds no letter and no mismatch", p.rc == WFA_HIP_OK && p.sum(p.rows) == 2 && p.c(1, 4) == 0 && p.c(1, 7) == 0 &&
                                                                          p.sum(p.qrows) == 2);
  }
  {  // refusals add nothing
    bool ok = true;
    for (const auto& b : std::vector<std::pair<int32_t, int32_t>>{{-1, 40}, {94, 40}, {0, 0}, {0, 94}}) {
      const Pair p("MM", "AC", {1, 2}, 2, b.first, b.second);
      ok = ok && p.rc == WFA_HIP_EINVAL && p.sum(p.rows) == 0 && p.sum(p.qrows) == 0;
    }
    const Pair over("MM", "AC", {1, 94}, 2, 0, 40), outruns("MMM", "AC", {1, 2}, 3, 0, 40);
    ok = ok && over.rc == WFA_HIP_EINVAL && over.sum(over.rows) == 0 && outruns.rc == WFA_HIP_EINVAL && outruns.sum(outruns.rows) == 0;
    const Pair nothing("", "", {}, 0, 0, 40);
    report("refusals add nothing; an empty pair needs no arrays", ok && nothing.rc == WFA_HIP_OK);
  }
  {  // the genotypes: L0 = qsum[alt], L1 = 3 (R + A), L2 = qsum[r]; the insertion keeps err_q * R
    const int32_t BIG = 2147483647;
    const int32_t c[][8] = {{17, 3, 0, 0, 0, 0, 0, 3}, {3, 17, 0, 0, 0, 0, 0, 17}, {4, 0, 0, 0, 0, 0, 9, 0}, {10, 0, 0, 0, 0, 10, 0, 0}, {BIG, BIG, 0, 0, 0, 0, 0, 0}};
    const int32_t q[][8] = {{600, 30, 0, 0, 0, 0, 0, 0}, {6, 600, 0, 0, 0, 0, 0, 0}, {100, 0, 0, 0, 0, 0, 5, 0}, {61, 0, 0, 0, 0, 400, 0, 0}, {BIG, BIG - 50, 0, 0, 0, 0, 0, 0}};
    const int32_t want[][4] = {{0, 30, -1, -1}, {2, 54, -1, -1}, {-1, -1, 2, 5}, {1, 1, -1, -1}, {0, 50, -1, -1}};
    const int64_t n = 5;
    std::vector<int32_t> counts((size_t)n * 8), qsums((size_t)n * 8), rows((size_t)n * WFA_HIP_GENOTYPE_COLS, -7);
    std::vector<uint8_t> ref((size_t)n, 'A');
    for (int64_t g = 0; g < n; ++g) for (int x = 0; x < 8; ++x) { counts[(size_t)(g * 8 + x)] = c[g][x]; qsums[(size_t)(g * 8 + x)] = q[g][x]; }
    int64_t count = -1;
    bool ok = wfa_hip_genotypes_quals_host(counts.data(), qsums.data(), nullptr, ref.data(), n, 0, 0, 1, 100, 20, 0, n, &count, rows.data()) == WFA_HIP_OK && count == n;
    for (int64_t g = 0; ok && g < n; ++g)
      for (int x = 0; x < 4; ++x) ok = ok && rows[(size_t)(g * 16 + 8 + x)] == want[g][x] && rows[(size_t)(g * 16 + 12 + x)] == -1;
    report("quality-weighted genotypes: the three costs, the insertion, 64 bits", ok);
    std::vector<int32_t> untouched((size_t)n * WFA_HIP_GENOTYPE_COLS, -7);
    count = -1;
    ok = wfa_hip_genotypes_quals_host(counts.data(), nullptr, nullptr, ref.data(), n, 0, 0, 1, 100, 20, 0, n, &count, untouched.data()) == WFA_HIP_EINVAL &&
         wfa_hip_genotypes_quals_host(counts.data(), qsums.data(), nullptr, ref.data(), n, 0, 0, 1, 100, 20, 1, n, &count, untouched.data()) == WFA_HIP_EINVAL &&
         wfa_hip_genotypes_quals_host(counts.data(), qsums.data(), nullptr, ref.data(), n, 0, 0, 1, 100, 61, 0, n, &count, untouched.data()) == WFA_HIP_EINVAL &&
         count == -1;
    for (size_t i = 0; ok && i < untouched.size(); ++i) ok = untouched[i] == -7;
    report("genotype refusals write nothing", ok);
  }
  printf(failures ? "%d FAILED\n" : "all ok\n", failures);
  return failures ? 1 : 0;
}
