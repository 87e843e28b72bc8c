// host_kmer.hpp — the k-mer walk on ASCII sequences that the host statements of the seed finder share (host_seed.cpp: clusters;
// host_chain.cpp: chains): valid k-mers and their 2-bit codes, and one read's matches against the indexed positions of a text set.
// Host code only (g++).
#pragma once
#include <stdint.h>
#include <algorithm>
#include <vector>

namespace wfa {
namespace hostk {

// the 2-bit code of a letter of ACGT (wfa_hip_pack_2bit: (c >> 1) & 3), -1 for every other byte
struct CodeTable {
  int8_t v[256];
  CodeTable() { for (int c = 0; c < 256; ++c) v[c] = (c == 'A' || c == 'C' || c == 'G' || c == 'T') ? (int8_t)((c >> 1) & 3) : (int8_t)-1; }
};
inline int code_of(uint8_t c) { static const CodeTable table; return table.v[c]; }

inline uint8_t complement(uint8_t c) {
  switch (c) { case 'A': return 'T'; case 'T': return 'A'; case 'C': return 'G'; case 'G': return 'C'; default: return c; }
}

// calls f(p, code) for every valid k-mer of seq[0 .. len): p + k <= len and k letters of ACGT; base p + i in bits 2 i .. 2 i + 1
template <class F>
void each_kmer(const uint8_t* seq, int64_t len, int k, F f) {
  uint32_t code = 0;
  int run = 0;   // letters of ACGT that end at the current base
  for (int64_t e = 0; e < len; ++e) {
    const int c = code_of(seq[e]);
    if (c < 0) { run = 0; code = 0; continue; }
    code = (code >> 2) | ((uint32_t)c << (2 * (k - 1)));
    if (++run >= k) f(e - k + 1, code);
  }
}

struct ReadKmer { uint32_t code; int32_t s, r; };
struct Match { uint32_t first; int32_t j, t; };   // first: the first entry of rk with the code

// One read against the text set.  rk: the valid k-mers of both strands of the read (s = 0: the read, s = 1: its reverse complement),
// sorted by code; occ[f], at the first entry f of a code: occ() of that code over the whole set; matches: the indexed positions that
// carry one of the read's codes (the first max_occ of a code: a code over max_occ is dropped by its occ).  Returns the number of
// (read k-mer, indexed position) pairs of the codes with occ <= max_occ.
inline int64_t read_matches(const uint8_t* read, int32_t L, int64_t ntexts, const uint8_t* texts, const int64_t* t_off, const int32_t* t_len,
                            int k, int stride, int max_occ, std::vector<ReadKmer>& rk, std::vector<int64_t>& occ, std::vector<Match>& matches) {
  rk.clear(); occ.clear(); matches.clear();
  std::vector<uint8_t> rc_read((size_t)L);
  for (int32_t p = 0; p < L; ++p) rc_read[(size_t)p] = complement(read[L - 1 - p]);
  each_kmer(read, L, k, [&](int64_t r, uint32_t code) { rk.push_back({code, 0, (int32_t)r}); });
  each_kmer(rc_read.data(), L, k, [&](int64_t r, uint32_t code) { rk.push_back({code, 1, (int32_t)r}); });
  if (rk.empty()) return 0;
  std::sort(rk.begin(), rk.end(), [](const ReadKmer& a, const ReadKmer& b) { return a.code < b.code; });
  std::vector<uint64_t> seen(1024, 0);   // the low 16 bits of the read's codes: most text positions stop here
  for (const ReadKmer& x : rk) seen[(x.code & 0xFFFFu) >> 6] |= 1ull << (x.code & 63u);
  occ.assign(rk.size(), 0);
  const uint64_t* const seen_bits = seen.data();
  for (int64_t jt = 0; jt < ntexts; ++jt)
    each_kmer(texts + t_off[jt], t_len[jt], k, [&, seen_bits](int64_t t, uint32_t code) {
      if (!((seen_bits[(code & 0xFFFFu) >> 6] >> (code & 63u)) & 1ull) || t % stride != 0) return;
      const auto it = std::lower_bound(rk.begin(), rk.end(), code, [](const ReadKmer& a, uint32_t c) { return a.code < c; });
      if (it == rk.end() || it->code != code) return;
      const uint32_t first = (uint32_t)(it - rk.begin());
      occ[first] += 1;
      if (occ[first] <= max_occ) matches.push_back({first, (int32_t)jt, (int32_t)t});
    });
  int64_t pairs = 0;
  for (size_t f = 0; f < rk.size();) {
    size_t e = f;
    while (e < rk.size() && rk[e].code == rk[f].code) ++e;
    if (occ[f] > 0 && occ[f] <= max_occ) pairs += occ[f] * (int64_t)(e - f);
    f = e;
  }
  return pairs;
}

}  // namespace hostk
}  // namespace wfa
