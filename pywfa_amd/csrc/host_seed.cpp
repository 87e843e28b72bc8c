// host_seed.cpp — the seed finder stated for ONE read in plain C++ (include/wfa_hip.h: wfa_hip_seeds_host), needing no GPU: what
// wfa_hip_seed_index_query writes into the read's row, computed from the definitions on the ASCII sequences.  Host code only (g++).
// Also the parameter checks the device entries share with it (every refusal names its parameter and its value).
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <string>
#include <vector>
#include "wfa_hip.h"
#include "host_kmer.hpp"

namespace wfa {

static int refuse(char* msg, size_t cap, const char* what, long long value, const char* want) {
  if (msg && cap) snprintf(msg, cap, "seed index: %s = %lld is out of range (%s)", what, value, want);
  return WFA_HIP_EINVAL;
}

int seed_check_index(int k, int stride, int max_occ, char* msg, size_t cap) {
  if (k < 8 || k > 15) return refuse(msg, cap, "k", k, "8 .. 15");
  if (stride < 1) return refuse(msg, cap, "stride", stride, "at least 1");
  if (max_occ < 1) return refuse(msg, cap, "max_occ", max_occ, "at least 1");
  return WFA_HIP_OK;
}

int seed_check_minimizer(int k, int w, int max_occ, char* msg, size_t cap) {
  if (k < 8 || k > 15) return refuse(msg, cap, "k", k, "8 .. 15");
  if (w < 1 || w > WFA_HIP_MINIMIZER_MAX_W) return refuse(msg, cap, "w", w, "1 .. 32");
  if (max_occ < 1) return refuse(msg, cap, "max_occ", max_occ, "at least 1");
  return WFA_HIP_OK;
}

int seed_check_query(int n, int min_hits, int gap, int pad, int max_hits, char* msg, size_t cap) {
  if (n < 1 || n > WFA_HIP_SEED_MAX_N) return refuse(msg, cap, "n", n, "1 .. 16");
  if (min_hits < 1) return refuse(msg, cap, "min_hits", min_hits, "at least 1");
  if (gap < 0) return refuse(msg, cap, "gap", gap, "at least 0");
  if (pad < 0) return refuse(msg, cap, "pad", pad, "at least 0");
  if (max_hits < 1 || max_hits > WFA_HIP_SEED_MAX_HITS) return refuse(msg, cap, "max_hits", max_hits, "1 .. 4096");
  return WFA_HIP_OK;
}

}  // namespace wfa

namespace {

using namespace wfa::hostk;
struct Hit { int32_t s, j, d; };

// the one body of wfa_hip_seeds_host (w = 0: the stride index) and wfa_hip_seeds_host_minimizer (w >= 1: stride plays no part)
int seeds_host(const uint8_t* read, int32_t read_len, int64_t ntexts, const uint8_t* texts, const int64_t* t_off, const int32_t* t_len,
               int k, int stride, int w, int max_occ, int n, int min_hits, int gap, int pad, int max_hits, int32_t* j, int32_t* reverse,
               int32_t* text_start, int32_t* text_len, int32_t* hits, uint8_t* overflow, char* msg, size_t msg_cap) {
  if (msg && msg_cap) msg[0] = '\0';
  int rc = w ? wfa::seed_check_minimizer(k, w, max_occ, msg, msg_cap) : wfa::seed_check_index(k, stride, max_occ, msg, msg_cap);
  if (rc == WFA_HIP_OK) rc = wfa::seed_check_query(n, min_hits, gap, pad, max_hits, msg, msg_cap);
  if (rc != WFA_HIP_OK) return rc;
  if (read_len < 0 || ntexts < 0 || (read_len > 0 && !read) || (ntexts > 0 && (!t_off || !t_len)) || !j || !reverse || !text_start ||
      !text_len || !hits || !overflow) {
    if (msg && msg_cap) snprintf(msg, msg_cap, "seeds: a negative length or a missing array");
    return WFA_HIP_EINVAL;
  }
  for (int64_t q = 0; q < ntexts; ++q)
    if (t_len[q] < 0 || t_off[q] < 0 || (t_len[q] > 0 && !texts)) {
      if (msg && msg_cap) snprintf(msg, msg_cap, "seeds: a negative length or offset of text %lld", (long long)q);
      return WFA_HIP_EINVAL;
    }
  for (int q = 0; q < n; ++q) { j[q] = -1; reverse[q] = 0; text_start[q] = 0; text_len[q] = 0; hits[q] = 0; }
  *overflow = 0;
  const int32_t L = read_len;
  // the valid k-mers of both strands of the read by code, the indexed positions that carry one of them, and the hits: every match of
  // a k-mer that is not masked, once per entry of the read with that code
  std::vector<ReadKmer> rk;
  std::vector<int64_t> occ;           // at the first entry of a code
  std::vector<Match> matches;
  const int64_t H = read_matches(read, L, ntexts, texts, t_off, t_len, k, stride, w, max_occ, rk, occ, matches);
  if (rk.empty()) return WFA_HIP_OK;
  if (H > max_hits) { *overflow = 1; return WFA_HIP_OK; }
  std::vector<Hit> hit;
  for (const Match& m : matches) {
    if (occ[m.first] > max_occ) continue;
    for (size_t e = m.first; e < rk.size() && rk[e].code == rk[m.first].code; ++e) hit.push_back({rk[e].s, m.j, m.t - rk[e].r});
  }
  std::sort(hit.begin(), hit.end(), [](const Hit& a, const Hit& b) {
    return a.s != b.s ? a.s < b.s : a.j != b.j ? a.j < b.j : a.d < b.d;
  });
  // clusters: maximal runs of one (s, j) whose neighbouring d differ by at most gap
  struct Cluster { int32_t c, s, j, d_lo, d_hi; };
  std::vector<Cluster> cl;
  for (size_t b = 0; b < hit.size();) {
    size_t e = b + 1;
    while (e < hit.size() && hit[e].s == hit[b].s && hit[e].j == hit[b].j && (int64_t)hit[e].d - hit[e - 1].d <= gap) ++e;
    if ((int64_t)(e - b) >= min_hits) cl.push_back({(int32_t)(e - b), hit[b].s, hit[b].j, hit[b].d, hit[e - 1].d});
    b = e;
  }
  std::stable_sort(cl.begin(), cl.end(), [](const Cluster& a, const Cluster& b) { return a.c > b.c; });   // (cl is in (s, j, d_lo) order)
  for (size_t q = 0; q < cl.size() && q < (size_t)n; ++q) {
    const Cluster& c = cl[q];
    const int64_t ts = std::max<int64_t>(0, (int64_t)c.d_lo - pad), te = std::min<int64_t>(t_len[c.j], (int64_t)c.d_hi + L + pad);
    j[q] = c.j; reverse[q] = c.s; text_start[q] = (int32_t)ts; text_len[q] = (int32_t)(te - ts); hits[q] = c.c;
  }
  return WFA_HIP_OK;
}

}  // namespace

extern "C" int wfa_hip_seeds_host(const uint8_t* read, int32_t read_len, int64_t ntexts, const uint8_t* texts, const int64_t* t_off,
                                  const int32_t* t_len, int k, int stride, int max_occ, int n, int min_hits, int gap, int pad,
                                  int max_hits, int32_t* j, int32_t* reverse, int32_t* text_start, int32_t* text_len, int32_t* hits,
                                  uint8_t* overflow, char* msg, size_t msg_cap) {
  return seeds_host(read, read_len, ntexts, texts, t_off, t_len, k, stride, 0, max_occ, n, min_hits, gap, pad, max_hits, j, reverse,
                    text_start, text_len, hits, overflow, msg, msg_cap);
}

extern "C" int wfa_hip_seeds_host_minimizer(const uint8_t* read, int32_t read_len, int64_t ntexts, const uint8_t* texts, const int64_t* t_off,
                                            const int32_t* t_len, int k, int w, int max_occ, int n, int min_hits, int gap, int pad,
                                            int max_hits, int32_t* j, int32_t* reverse, int32_t* text_start, int32_t* text_len,
                                            int32_t* hits, uint8_t* overflow, char* msg, size_t msg_cap) {
  if (msg && msg_cap) msg[0] = '\0';
  const int rc = wfa::seed_check_minimizer(k, w, max_occ, msg, msg_cap);   // (w = 0 is the body's word for the stride index: refused here)
  if (rc != WFA_HIP_OK) return rc;
  return seeds_host(read, read_len, ntexts, texts, t_off, t_len, k, 1, w, max_occ, n, min_hits, gap, pad, max_hits, j, reverse,
                    text_start, text_len, hits, overflow, msg, msg_cap);
}

extern "C" int wfa_hip_minimizers_host(const uint8_t* seq, int64_t len, int k, int w, uint8_t* selected, char* msg, size_t msg_cap) {
  if (msg && msg_cap) msg[0] = '\0';
  const int rc = wfa::seed_check_minimizer(k, w, 1, msg, msg_cap);
  if (rc != WFA_HIP_OK) return rc;
  if (len < 0 || (len > 0 && (!seq || !selected))) {
    if (msg && msg_cap) snprintf(msg, msg_cap, "minimizers: a negative length or a missing array");
    return WFA_HIP_EINVAL;
  }
  minimizer_flags(seq, len, k, w, selected);
  return WFA_HIP_OK;
}
