// host_chain.cpp — co-linear chaining of a read's anchors stated for ONE read in plain C++ (include/wfa_hip.h: wfa_hip_chains_host),
// needing no GPU: what wfa_hip_seed_index_chain writes into the read's row, computed from the definitions on the ASCII sequences.
// Host code only (g++).  Also the parameter check the device entry shares with it (every refusal names its parameter and its value).
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <vector>
#include "wfa_hip.h"
#include "host_kmer.hpp"

namespace wfa {

int seed_check_index(int k, int stride, int max_occ, char* msg, size_t cap);   // host_seed.cpp
int seed_check_minimizer(int k, int w, int max_occ, char* msg, size_t cap);

static int refuse_chain(char* msg, size_t cap, const char* what, long long value, const char* want) {
  if (msg && cap) snprintf(msg, cap, "seed chain: %s = %lld is out of range (%s)", what, value, want);
  return WFA_HIP_EINVAL;
}

int seed_check_chain(int n, int min_hits, int min_score, int lookback, int max_dist, int band, int pad, int max_anchors, char* msg, size_t cap) {
  if (n < 1 || n > WFA_HIP_SEED_MAX_N) return refuse_chain(msg, cap, "n", n, "1 .. 16");
  if (min_hits < 1) return refuse_chain(msg, cap, "min_hits", min_hits, "at least 1");
  if (min_score < 0) return refuse_chain(msg, cap, "min_score", min_score, "at least 0");
  if (lookback < 1 || lookback > WFA_HIP_CHAIN_MAX_LOOKBACK) return refuse_chain(msg, cap, "lookback", lookback, "1 .. 64");
  if (max_dist < 1 || max_dist > (1 << 20)) return refuse_chain(msg, cap, "max_dist", max_dist, "1 .. 1048576");
  if (band < 0 || band > (1 << 16)) return refuse_chain(msg, cap, "band", band, "0 .. 65536");
  if (pad < 0) return refuse_chain(msg, cap, "pad", pad, "at least 0");
  if (max_anchors < 1 || max_anchors > WFA_HIP_CHAIN_MAX_ANCHORS) return refuse_chain(msg, cap, "max_anchors", max_anchors, "1 .. 65536");
  return WFA_HIP_OK;
}

}  // namespace wfa

namespace {

using namespace wfa::hostk;

struct Anchor {
  int32_t s, r, j, t;
  int32_t f, cnt, d_lo, d_hi, r_first;
  bool covered;
};

inline int32_t gap_cost(int32_t g, int k) {
  if (g == 0) return 0;
  return ((g * k) >> 6) + ((31 - __builtin_clz((uint32_t)g)) >> 1);
}

// the one body of wfa_hip_chains_host (w = 0: the stride index) and wfa_hip_chains_host_minimizer (w >= 1: stride plays no part)
int chains_host(const uint8_t* read, int32_t read_len, int64_t ntexts, const uint8_t* texts, const int64_t* t_off, const int32_t* t_len,
                int k, int stride, int w, int max_occ, int n, int min_hits, int min_score, int lookback, int max_dist, int band, int pad,
                int max_anchors, int32_t* j, int32_t* reverse, int32_t* text_start, int32_t* text_len, int32_t* hits, int32_t* score,
                int32_t* pattern_start, int32_t* pattern_len, uint8_t* overflow, char* msg, size_t msg_cap) {
  if (msg && msg_cap) msg[0] = '\0';
  int rc = w ? wfa::seed_check_minimizer(k, w, max_occ, msg, msg_cap) : wfa::seed_check_index(k, stride, max_occ, msg, msg_cap);
  if (rc == WFA_HIP_OK) rc = wfa::seed_check_chain(n, min_hits, min_score, lookback, max_dist, band, pad, max_anchors, msg, msg_cap);
  if (rc != WFA_HIP_OK) return rc;
  if (read_len < 0 || ntexts < 0 || (read_len > 0 && !read) || (ntexts > 0 && (!t_off || !t_len)) || !j || !reverse || !text_start ||
      !text_len || !hits || !score || !pattern_start || !pattern_len || !overflow) {
    if (msg && msg_cap) snprintf(msg, msg_cap, "chains: a negative length or a missing array");
    return WFA_HIP_EINVAL;
  }
  for (int64_t q = 0; q < ntexts; ++q)
    if (t_len[q] < 0 || t_off[q] < 0 || (t_len[q] > 0 && !texts)) {
      if (msg && msg_cap) snprintf(msg, msg_cap, "chains: a negative length or offset of text %lld", (long long)q);
      return WFA_HIP_EINVAL;
    }
  for (int q = 0; q < n; ++q) {
    j[q] = -1; reverse[q] = 0; text_start[q] = 0; text_len[q] = 0; hits[q] = 0; score[q] = 0; pattern_start[q] = 0; pattern_len[q] = 0;
  }
  *overflow = 0;
  const int32_t L = read_len;
  std::vector<ReadKmer> rk;
  std::vector<int64_t> occ;
  std::vector<Match> matches;
  const int64_t N = read_matches(read, L, ntexts, texts, t_off, t_len, k, stride, w, max_occ, rk, occ, matches);
  if (N > max_anchors) { *overflow = 1; return WFA_HIP_OK; }
  if (N == 0) return WFA_HIP_OK;
  // the anchors, in the order of a scan along the read: (s, r, j, t)
  std::vector<Anchor> an;
  an.reserve((size_t)N);
  for (const Match& m : matches) {
    if (occ[m.first] > max_occ) continue;
    for (size_t e = m.first; e < rk.size() && rk[e].code == rk[m.first].code; ++e) {
      const int32_t d = m.t - rk[e].r;
      an.push_back({rk[e].s, rk[e].r, m.j, m.t, k, 1, d, d, rk[e].r, false});
    }
  }
  std::sort(an.begin(), an.end(), [](const Anchor& a, const Anchor& b) {
    return a.s != b.s ? a.s < b.s : a.r != b.r ? a.r < b.r : a.j != b.j ? a.j < b.j : a.t < b.t;
  });
  // chaining: the best of the `lookback` anchors before it, the nearest on a tie, when it is worth more than the anchor alone
  for (size_t a = 0; a < an.size(); ++a) {
    Anchor& x = an[a];
    int32_t best = k;
    int64_t from = -1;
    for (int64_t b = (int64_t)a - 1; b >= 0 && b >= (int64_t)a - lookback; --b) {
      const Anchor& y = an[(size_t)b];
      if (y.s != x.s || y.j != x.j) continue;
      const int32_t dr = x.r - y.r, dt = x.t - y.t;
      if (dr <= 0 || dt <= 0 || dr > max_dist || dt > max_dist) continue;
      const int32_t g = dt > dr ? dt - dr : dr - dt;
      if (g > band) continue;
      const int32_t v = y.f + std::min(std::min(dr, dt), (int32_t)k) - gap_cost(g, k);
      if (v > best) { best = v; from = b; }   // (b walks down: a later equal value does not replace the nearer one)
    }
    if (from >= 0) {
      const Anchor& y = an[(size_t)from];
      x.f = best; x.cnt = y.cnt + 1; x.d_lo = std::min(y.d_lo, x.d_lo); x.d_hi = std::max(y.d_hi, x.d_hi); x.r_first = y.r_first;
    }
  }
  // selection: the uncovered chain end of largest f, the first in the order on a tie; its window covers the anchors inside it
  for (int q = 0; q < n; ++q) {
    int64_t pick = -1;
    for (size_t a = 0; a < an.size(); ++a) {
      const Anchor& x = an[a];
      if (x.covered || x.cnt < min_hits || x.f < min_score) continue;
      if (pick < 0 || x.f > an[(size_t)pick].f) pick = (int64_t)a;
    }
    if (pick < 0) break;
    const Anchor c = an[(size_t)pick];
    const int64_t ts = std::max<int64_t>(0, (int64_t)c.d_lo - pad), te = std::min<int64_t>(t_len[c.j], (int64_t)c.d_hi + L + pad);
    j[q] = c.j; reverse[q] = c.s; text_start[q] = (int32_t)ts; text_len[q] = (int32_t)(te - ts); hits[q] = c.cnt; score[q] = c.f;
    pattern_start[q] = c.s ? L - (c.r + k) : c.r_first;
    pattern_len[q] = c.r + k - c.r_first;
    for (Anchor& x : an)
      if (x.s == c.s && x.j == c.j && ts <= x.t && (int64_t)x.t + k <= te) x.covered = true;
  }
  return WFA_HIP_OK;
}

}  // namespace

extern "C" int wfa_hip_chains_host(const uint8_t* read, int32_t read_len, int64_t ntexts, const uint8_t* texts, const int64_t* t_off,
                                   const int32_t* t_len, int k, int stride, int max_occ, int n, int min_hits, int min_score, int lookback,
                                   int max_dist, int band, int pad, int max_anchors, int32_t* j, int32_t* reverse, int32_t* text_start,
                                   int32_t* text_len, int32_t* hits, int32_t* score, int32_t* pattern_start, int32_t* pattern_len,
                                   uint8_t* overflow, char* msg, size_t msg_cap) {
  return chains_host(read, read_len, ntexts, texts, t_off, t_len, k, stride, 0, max_occ, n, min_hits, min_score, lookback, max_dist, band,
                     pad, max_anchors, j, reverse, text_start, text_len, hits, score, pattern_start, pattern_len, overflow, msg, msg_cap);
}

extern "C" int wfa_hip_chains_host_minimizer(const uint8_t* read, int32_t read_len, int64_t ntexts, const uint8_t* texts,
                                             const int64_t* t_off, const int32_t* t_len, int k, int w, int max_occ, int n, int min_hits,
                                             int min_score, int lookback, int max_dist, int band, int pad, int max_anchors, int32_t* j,
                                             int32_t* reverse, int32_t* text_start, int32_t* text_len, int32_t* hits, int32_t* score,
                                             int32_t* pattern_start, int32_t* pattern_len, uint8_t* overflow, char* msg, size_t msg_cap) {
  if (msg && msg_cap) msg[0] = '\0';
  const int rc = wfa::seed_check_minimizer(k, w, max_occ, msg, msg_cap);   // (w = 0 is the body's word for the stride index: refused here)
  if (rc != WFA_HIP_OK) return rc;
  return chains_host(read, read_len, ntexts, texts, t_off, t_len, k, 1, w, max_occ, n, min_hits, min_score, lookback, max_dist, band, pad,
                     max_anchors, j, reverse, text_start, text_len, hits, score, pattern_start, pattern_len, overflow, msg, msg_cap);
}
