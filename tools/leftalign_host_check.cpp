// leftalign_host_check.cpp — a stand-alone check of wfa_hip_ops_left_align (pywfa_amd/csrc/host_cigar.cpp) on the edge cases of the
// left-alignment rule, meant to be built with the host statement under a sanitizer (no GPU, no Python):
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude tools/leftalign_host_check.cpp
//       pywfa_amd/csrc/host_cigar.cpp -o leftalign_host_check     (one command), then ./leftalign_host_check
// Every array is heap-allocated at its exact size, so that a read or write past an end is seen.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "wfa_hip.h"

static int failures = 0;

// "41M1D49M" -> one letter per op
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

static void run(const char* name, const char* cigar, const std::string& pattern, const std::string& text, int want_rc, const char* want,
                int64_t want_moved, int64_t want_merges) {
  std::vector<uint8_t> ops = expand(cigar), before = ops, P(pattern.begin(), pattern.end()), T(text.begin(), text.end());
  std::vector<int64_t> stats(2, -5);
  const int rc = wfa_hip_ops_left_align(ops.empty() ? nullptr : ops.data(), (int64_t)ops.size(), P.empty() ? nullptr : P.data(), (int32_t)P.size(),
                                        T.empty() ? nullptr : T.data(), (int32_t)T.size(), stats.data());
  bool ok = rc == want_rc;
  if (ok && rc == WFA_HIP_OK) ok = ops == expand(want) && stats[0] == want_moved && stats[1] == want_merges;
  if (ok && rc != WFA_HIP_OK) ok = ops == before && stats[0] == -5 && stats[1] == -5;
  if (ok && rc == WFA_HIP_OK) {   // a second application changes nothing
    std::vector<uint8_t> again = ops;
    ok = wfa_hip_ops_left_align(again.empty() ? nullptr : again.data(), (int64_t)again.size(), P.empty() ? nullptr : P.data(), (int32_t)P.size(),
                                T.empty() ? nullptr : T.data(), (int32_t)T.size(), nullptr) == WFA_HIP_OK && again == ops;
  }
  printf("%-58s %s\n", name, ok ? "ok" : "FAILED");
  if (!ok) {
    ++failures;
    printf("  rc %d (want %d), stats %lld %lld, ops %.*s\n", rc, want_rc, (long long)stats[0], (long long)stats[1], (int)ops.size(), (const char*)ops.data());
  }
}

int main() {
  const std::string L = "TGCATCGATTCGAGCTAGCTTGACCGTATCGGATCCGTAG", R = "CTGGATCCTAGGCTTAGCGATCGTAGGCTAACGTTAGCGT";   // 40 + 40
  const std::string A8 = L + "G" + std::string(8, 'A') + "C" + R;
  run("one extra A in the read", "49M1D41M", L + "G" + std::string(9, 'A') + "C" + R, A8, WFA_HIP_OK, "41M1D49M", 1, 0);
  run("one missing A", "48M1I41M", L + "G" + std::string(7, 'A') + "C" + R, A8, WFA_HIP_OK, "41M1I48M", 1, 0);
  run("an extra CA in (CA)5", "50M2D41M", L + "CACACACACACAG" + R, L + "CACACACACAG" + R, WFA_HIP_OK, "40M2D51M", 1, 0);
  run("a missing CA in (CA)5", "48M2I41M", L + "CACACACAG" + R, L + "CACACACACAG" + R, WFA_HIP_OK, "40M2I49M", 1, 0);
  run("stopped by an X inside the repeat", "4M1X4M1D3M", "GAAATAAAAACGT", "GAAAAAAAACGT", WFA_HIP_OK, "4M1X1D7M", 1, 0);
  run("one op behind the core's first M", "5M1D2M", "AAAAAACG", "AAAAACG", WFA_HIP_OK, "1M1D6M", 1, 0);
  run("... behind a leading X", "1X4M1D2M", "CAAAAACG", "GAAAACG", WFA_HIP_OK, "1X1M1D5M", 1, 0);
  run("a run at the very first and last letters", "1M1I1M", "AA", "AAA", WFA_HIP_OK, "1M1I1M", 0, 0);
  run("leading and trailing runs stay", "2D4M1I", "AAAAAA", "AAAAA", WFA_HIP_OK, "2D4M1I", 0, 0);
  run("an I run stopped by a D run", "2M2D3M1I2M", "GCTTAAAAG", "GCAAAAAG", WFA_HIP_OK, "2M2D1I5M", 1, 0);
  run("a merge of two I runs", "2M1I2M1I3M", "GAAAACT", "GAAAAAACT", WFA_HIP_OK, "1M2I6M", 2, 1);
  run("a merge of two D runs", "2M1D2M1D3M", "GAAAAAACT", "GAAAACT", WFA_HIP_OK, "1M2D6M", 2, 1);
  run("no M", "2X1I", "AC", "GTA", WFA_HIP_OK, "2X1I", 0, 0);
  run("length 1: M", "1M", "A", "A", WFA_HIP_OK, "1M", 0, 0);
  run("length 1: D, no text", "1D", "A", "", WFA_HIP_OK, "1D", 0, 0);
  run("empty", "", "", "", WFA_HIP_OK, "", 0, 0);
  run("a homopolymer of 300 with a run of 70", "250M70D50M", std::string(370, 'C'), std::string(300, 'C'), WFA_HIP_OK, "1M70D299M", 1, 0);
  run("refused: the ops consume more pattern", "5M1D2M", "AAAAACG", "AAAAACG", WFA_HIP_EINVAL, "", 0, 0);
  run("refused: the ops consume less text", "5M1D2M", "AAAAAACG", "AAAAACGT", WFA_HIP_EINVAL, "", 0, 0);
  {
    std::vector<uint8_t> ops = expand("3M");
    const uint8_t s[3] = {'A', 'C', 'G'};
    const bool ok = wfa_hip_ops_left_align(ops.data(), -1, s, 3, s, 3, nullptr) == WFA_HIP_EINVAL && wfa_hip_ops_left_align(nullptr, 3, s, 3, s, 3, nullptr) == WFA_HIP_EINVAL &&
                    wfa_hip_ops_left_align(ops.data(), 3, nullptr, 3, s, 3, nullptr) == WFA_HIP_EINVAL && wfa_hip_ops_left_align(ops.data(), 3, s, 3, s, -3, nullptr) == WFA_HIP_EINVAL;
    printf("%-58s %s\n", "refused: negative lengths and missing pointers", ok ? "ok" : "FAILED");
    failures += ok ? 0 : 1;
  }
  printf(failures ? "%d FAILED\n" : "all ok\n", failures);
  return failures ? 1 : 0;
}
