// host_kmer.hpp — the k-mer walk on ASCII sequences that the host statements of the seed finder share (host_seed.cpp: clusters;
// host_chain.cpp: chains): valid k-mers and their 2-bit codes, the (w,k)-minimizers of a sequence (include/wfa_hip.h, "minimizers"),
// and one read's matches against the indexed positions of a text set.  Host code only (g++).
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

// reverse complement of a k-mer code: the 2-bit groups in reverse order, each letter complemented (code ^ 2: A 0 <-> T 2, C 1 <-> G 3)
inline uint32_t rc_code(uint32_t code, int k) {
  uint32_t out = 0;
  for (int i = 0; i < k; ++i) out |= (((code >> (2 * i)) & 3u) ^ 2u) << (2 * (k - 1 - i));
  return out;
}

inline uint32_t mix32(uint32_t h) {
  h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
  return h;
}

static const uint64_t KEY_INF = ~0ull;   // above every mix32 value

// selected[p] = 1 when p is a (w,k)-minimizer of seq[0 .. len), 0 otherwise: key(p) finite, and with l / r the consecutive positions
// left / right of p whose keys are >= key(p) (+inf included; positions outside the sequence are +inf), each capped at w - 1,
// l + r + 1 >= w
inline void minimizer_flags(const uint8_t* seq, int64_t len, int k, int w, uint8_t* selected) {
  std::vector<uint64_t> key((size_t)len, KEY_INF);
  each_kmer(seq, len, k, [&](int64_t p, uint32_t code) { key[(size_t)p] = mix32(std::min(code, rc_code(code, k))); });
  const auto key_at = [&](int64_t p) { return p < 0 || p >= len ? KEY_INF : key[(size_t)p]; };
  for (int64_t p = 0; p < len; ++p) {
    selected[p] = 0;
    if (key[(size_t)p] == KEY_INF) continue;
    int l = 0, r = 0;
    while (l < w - 1 && key_at(p - 1 - l) >= key[(size_t)p]) ++l;
    while (r < w - 1 && key_at(p + 1 + r) >= key[(size_t)p]) ++r;
    selected[p] = l + r + 1 >= w ? 1 : 0;
  }
}

struct ReadKmer { uint32_t code; int32_t s, r; };
struct Match { uint32_t first; int32_t j, t; };   // first: the first entry of rk with the code

// One read against the text set.  rk: the valid k-mers of both strands of the read (s = 0: the read, s = 1: its reverse complement),
// sorted by code; occ[f], at the first entry f of a code: occ() of that code over the whole set; matches: the indexed positions that
// carry one of the read's codes (the first max_occ of a code: a code over max_occ is dropped by its occ).  Returns the number of
// (read k-mer, indexed position) pairs of the codes with occ <= max_occ.
// w = 0: the stride index (text positions with t % stride == 0, every read position).  w >= 1: the minimizer index (the text positions
// that are minimizers of their text, the read positions that are minimizers of R_s; stride plays no part).
inline int64_t read_matches(const uint8_t* read, int32_t L, int64_t ntexts, const uint8_t* texts, const int64_t* t_off, const int32_t* t_len,
                            int k, int stride, int w, int max_occ, std::vector<ReadKmer>& rk, std::vector<int64_t>& occ,
                            std::vector<Match>& matches) {
  rk.clear(); occ.clear(); matches.clear();
  std::vector<uint8_t> rc_read((size_t)L);
  for (int32_t p = 0; p < L; ++p) rc_read[(size_t)p] = complement(read[L - 1 - p]);
  std::vector<uint8_t> sel;   // the minimizer flags of the sequence at hand
  const uint8_t* sel_bits = nullptr;
  const auto select = [&](const uint8_t* seq, int64_t len) {
    if (w < 1) return;
    sel.assign((size_t)len + 1, 0);
    minimizer_flags(seq, len, k, w, sel.data());
    sel_bits = sel.data();
  };
  select(read, L);
  each_kmer(read, L, k, [&](int64_t r, uint32_t code) { if (!sel_bits || sel_bits[r]) rk.push_back({code, 0, (int32_t)r}); });
  select(rc_read.data(), L);
  each_kmer(rc_read.data(), L, k, [&](int64_t r, uint32_t code) { if (!sel_bits || sel_bits[r]) rk.push_back({code, 1, (int32_t)r}); });
  if (rk.empty()) return 0;
  std::sort(rk.begin(), rk.end(), [](const ReadKmer& a, const ReadKmer& b) { return a.code < b.code; });
  std::vector<uint64_t> seen(1024, 0);   // the low 16 bits of the read's codes: most text positions stop here
  for (const ReadKmer& x : rk) seen[(x.code & 0xFFFFu) >> 6] |= 1ull << (x.code & 63u);
  occ.assign(rk.size(), 0);
  const uint64_t* const seen_bits = seen.data();
  for (int64_t jt = 0; jt < ntexts; ++jt) {
    select(texts + t_off[jt], t_len[jt]);
    each_kmer(texts + t_off[jt], t_len[jt], k, [&, seen_bits](int64_t t, uint32_t code) {
      if (!((seen_bits[(code & 0xFFFFu) >> 6] >> (code & 63u)) & 1ull) || (sel_bits ? !sel_bits[t] : t % stride != 0)) return;
      const auto it = std::lower_bound(rk.begin(), rk.end(), code, [](const ReadKmer& a, uint32_t c) { return a.code < c; });
      if (it == rk.end() || it->code != code) return;
      const uint32_t first = (uint32_t)(it - rk.begin());
      occ[first] += 1;
      if (occ[first] <= max_occ) matches.push_back({first, (int32_t)jt, (int32_t)t});
    });
  }
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
