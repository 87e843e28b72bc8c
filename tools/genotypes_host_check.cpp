// genotypes_host_check.cpp — a stand-alone check of wfa_hip_sites_host and wfa_hip_genotypes_host (pywfa_amd/csrc/host_cigar.cpp) on
// the edges of the genotype rule, meant to be built with the host statements under a sanitizer (no GPU, no Python):
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude tools/genotypes_host_check.cpp
//       pywfa_amd/csrc/host_cigar.cpp -o genotypes_host_check     (one command), then ./genotypes_host_check
// Every array is heap-allocated at its exact size, so that a read or write past an end is seen; the counters near 2^31 would overflow
// a 32-bit sum or product.
#include <stdint.h>
#include <stdio.h>
#include <vector>
#include "wfa_hip.h"

static int failures = 0;

static void report(const char* name, bool ok) {
  printf("%-66s %s\n", name, ok ? "ok" : "FAILED");
  failures += ok ? 0 : 1;
}

struct Row { int32_t c[8], f[8]; uint8_t ref; int32_t gt, gq, ins_gt, ins_gq; };   // what columns 8..11 must be (min 1, permille 100, err_q 20)

int main() {
  const int32_t BIG = 2147483647;
  const Row hand[] = {
      {{17, 3, 0, 0, 0, 0, 0, 3}, {9, 1, 0, 0, 0, 0, 0, 1}, 'A', 0, 0, -1, -1},              // L0 = L1 = 60: the tie goes to 0/0
      {{3, 17, 0, 0, 0, 0, 0, 17}, {1, 9, 0, 0, 0, 0, 0, 9}, 'A', 1, 0, -1, -1},             // L1 = L2 = 60: the tie goes to 0/1
      {{0, 9, 0, 0, 0, 0, 0, 9}, {0, 4, 0, 0, 0, 0, 0, 4}, 'A', 2, 27, -1, -1},              // R = 0
      {{0, 0, 11, 0, 0, 0, 0, 11}, {0, 0, 11, 0, 0, 0, 0, 11}, 'T', 2, 33, -1, -1},          // A = depth
      {{4, 0, 0, 0, 0, 0, 9, 0}, {2, 0, 0, 0, 0, 0, 5, 0}, 'A', -1, -1, 2, 27},              // c6 > depth: R clamps to 0
      {{BIG, BIG - 1, 0, 0, 0, 0, 0, 0}, {BIG / 2, BIG / 3, 0, 0, 0, 0, 0, 0}, 'A', 1, 99, -1, -1},   // 64-bit sums and products
      {{6, 5, 0, 0, 2, 0, 0, 5}, {3, 2, 0, 0, 1, 0, 0, 2}, 'N', 1, 16, -1, -1},              // r = 4: R = 2, A = 6: L = 120, 24, 40
      {{10, 0, 0, 0, 0, 10, 10, 0}, {5, 0, 0, 0, 0, 10, 0, 0}, 'A', 1, 99, 1, 99},           // alt = deleted; an insertion
      {{30, 0, 0, 0, 0, 0, 0, 0}, {15, 0, 0, 0, 0, 0, 0, 0}, 'A', -2, -2, -2, -2},           // no event: no row
  };
  const int64_t n = (int64_t)(sizeof(hand) / sizeof(hand[0]));
  std::vector<int32_t> counts((size_t)n * 8), fwd((size_t)n * 8);
  std::vector<uint8_t> ref((size_t)n);
  for (int64_t g = 0; g < n; ++g) {
    for (int x = 0; x < 8; ++x) { counts[(size_t)(g * 8 + x)] = hand[g].c[x]; fwd[(size_t)(g * 8 + x)] = hand[g].f[x]; }
    ref[(size_t)g] = hand[g].ref;
  }
  int64_t count = -1, want = 0;
  for (int64_t g = 0; g < n; ++g) want += hand[g].gt != -2;
  std::vector<int32_t> rows((size_t)want * WFA_HIP_GENOTYPE_COLS, -7);
  bool ok = wfa_hip_genotypes_host(counts.data(), fwd.data(), ref.data(), n, 3, 1000, 1, 100, 20, 0, want, &count, rows.data()) == WFA_HIP_OK && count == want;
  int64_t k = 0;
  for (int64_t g = 0; ok && g < n; ++g) {
    if (hand[g].gt == -2) continue;
    const int32_t* r = rows.data() + k++ * WFA_HIP_GENOTYPE_COLS;
    ok = r[0] == 3 && r[1] == 1000 + g && r[8] == hand[g].gt && r[9] == hand[g].gq && r[10] == hand[g].ins_gt && r[11] == hand[g].ins_gq && r[15] == hand[g].f[6];
    if (!ok) printf("  row %lld: gt %d gq %d ins_gt %d ins_gq %d\n", (long long)g, r[8], r[9], r[10], r[11]);
  }
  report("hand-made rows: ties, R = 0, A = depth, the clamp, 2^31, r = 4", ok);

  // columns 0..7 are the site rows; without the forward rows the last four columns are -1
  std::vector<int32_t> sites((size_t)want * WFA_HIP_SITE_COLS, -7), plain((size_t)want * WFA_HIP_GENOTYPE_COLS, -7);
  int64_t nsites = -1, nplain = -1;
  ok = wfa_hip_sites_host(counts.data(), ref.data(), n, 3, 1000, 1, 100, want, &nsites, sites.data()) == WFA_HIP_OK && nsites == want &&
       wfa_hip_genotypes_host(counts.data(), nullptr, ref.data(), n, 3, 1000, 1, 100, 20, 0, want, &nplain, plain.data()) == WFA_HIP_OK && nplain == want;
  for (int64_t r = 0; ok && r < want; ++r) {
    for (int x = 0; x < 8; ++x) ok = ok && sites[(size_t)(r * 8 + x)] == rows[(size_t)(r * 16 + x)] && plain[(size_t)(r * 16 + x)] == rows[(size_t)(r * 16 + x)];
    for (int x = 12; x < 16; ++x) ok = ok && plain[(size_t)(r * 16 + x)] == -1;
  }
  report("columns 0..7 equal the site rows; not tracking: columns 12..15 are -1", ok);

  // the strand filter: the fourth row's reads are all forward; the eighth row's deletion is forward only, its insertion reverse only
  std::vector<int32_t> strict((size_t)want * WFA_HIP_GENOTYPE_COLS, -7);
  int64_t nstrict = -1;
  ok = wfa_hip_genotypes_host(counts.data(), fwd.data(), ref.data(), n, 3, 1000, 1, 100, 20, 1, want, &nstrict, strict.data()) == WFA_HIP_OK && nstrict == want - 2;
  report("min_alt_strand = 1 drops the rows seen on one strand", ok);

  // capacities: the count is the full number, rows behind the written ones stay
  for (int64_t cap : {(int64_t)0, want - 1, want, want + 5}) {
    std::vector<int32_t> part((size_t)cap * WFA_HIP_GENOTYPE_COLS, -7);
    int64_t c = -1;
    ok = wfa_hip_genotypes_host(counts.data(), fwd.data(), ref.data(), n, 3, 1000, 1, 100, 20, 0, cap, &c, cap ? part.data() : nullptr) == WFA_HIP_OK && c == want;
    for (int64_t i = 0; ok && i < cap * WFA_HIP_GENOTYPE_COLS; ++i) ok = part[(size_t)i] == (i < want * WFA_HIP_GENOTYPE_COLS ? rows[(size_t)i] : -7);
    char name[64];
    snprintf(name, sizeof(name), "capacity %lld", (long long)cap);
    report(name, ok);
  }

  // refusals write nothing
  count = -1;
  std::vector<int32_t> untouched((size_t)want * WFA_HIP_GENOTYPE_COLS, -7);
  const int32_t bad[][4] = {{0, 100, 20, 0}, {1, 0, 20, 0}, {1, 1001, 20, 0}, {1, 100, 0, 0}, {1, 100, 61, 0}, {1, 100, 20, -1}};
  ok = true;
  for (const auto& b : bad)
    ok = ok && wfa_hip_genotypes_host(counts.data(), fwd.data(), ref.data(), n, 0, 0, b[0], b[1], b[2], b[3], want, &count, untouched.data()) == WFA_HIP_EINVAL;
  ok = ok && wfa_hip_genotypes_host(counts.data(), nullptr, ref.data(), n, 0, 0, 1, 100, 20, 1, want, &count, untouched.data()) == WFA_HIP_EINVAL &&
       wfa_hip_genotypes_host(counts.data(), fwd.data(), ref.data(), -1, 0, 0, 1, 100, 20, 0, want, &count, untouched.data()) == WFA_HIP_EINVAL &&
       wfa_hip_genotypes_host(counts.data(), fwd.data(), ref.data(), n, 0, 0, 1, 100, 20, 0, -1, &count, untouched.data()) == WFA_HIP_EINVAL &&
       wfa_hip_genotypes_host(counts.data(), fwd.data(), ref.data(), n, 0, 0, 1, 100, 20, 0, want, nullptr, untouched.data()) == WFA_HIP_EINVAL &&
       wfa_hip_genotypes_host(counts.data(), fwd.data(), ref.data(), n, 0, 0, 1, 100, 20, 0, want, &count, nullptr) == WFA_HIP_EINVAL &&
       wfa_hip_genotypes_host(nullptr, fwd.data(), ref.data(), n, 0, 0, 1, 100, 20, 0, want, &count, untouched.data()) == WFA_HIP_EINVAL && count == -1;
  for (size_t i = 0; ok && i < untouched.size(); ++i) ok = untouched[i] == -7;
  report("refusals write nothing", ok);
  ok = wfa_hip_genotypes_host(nullptr, nullptr, nullptr, 0, 0, 0, 1, 100, 20, 0, 0, &count, nullptr) == WFA_HIP_OK && count == 0;
  report("an empty range needs no arrays", ok);
  printf(failures ? "%d FAILED\n" : "all ok\n", failures);
  return failures ? 1 : 0;
}
