// host_pair.cpp — host only, needs no GPU: the pairing rule of include/wfa_hip.h ("pairing") stated in plain C++ over arrays of hits
// (wfa_hip_pair_host), built on the placement rule of host_place.cpp, and the checks the device entry shares with it
// (wfa_hip_placer_run_pairs in wfa_hip.hip).  The pair kernel of k_place.hip is held to this statement.
#include <stdint.h>
#include <stdio.h>
#include <limits.h>
#include <vector>
#include "wfa_hip.h"

namespace wfa {

// the parameters and the fragments of one run: 0 <= min_insert <= max_insert, unpaired >= 0, nfrag >= 0, both mate arrays or neither,
// every mate inside [0, nreads), the two mates of a fragment distinct, no read named twice (a bitmap over the reads)
int pair_check(int64_t nreads, int32_t min_insert, int32_t max_insert, int32_t unpaired, int64_t nfrag, const int32_t* mate1,
               const int32_t* mate2, char* msg, size_t cap) {
  if (min_insert < 0 || max_insert < min_insert) {
    if (msg) snprintf(msg, cap, "pairing: min_insert = %d, max_insert = %d are out of range (0 <= min_insert <= max_insert)",
                      (int)min_insert, (int)max_insert);
    return WFA_HIP_EINVAL;
  }
  if (unpaired < 0) { if (msg) snprintf(msg, cap, "pairing: unpaired = %d is out of range (at least 0)", (int)unpaired); return WFA_HIP_EINVAL; }
  if (nfrag < 0) { if (msg) snprintf(msg, cap, "pairing: a negative number of fragments (%lld)", (long long)nfrag); return WFA_HIP_EINVAL; }
  if ((mate1 == nullptr) != (mate2 == nullptr)) {
    if (msg) snprintf(msg, cap, "pairing: %s is missing (both mate arrays, or neither for interleaved mates)", mate1 ? "mate2" : "mate1");
    return WFA_HIP_EINVAL;
  }
  if (!mate1) {
    if (nfrag > nreads / 2) {
      if (msg) snprintf(msg, cap, "pairing: %lld interleaved fragments need %lld reads, there are %lld", (long long)nfrag,
                        (long long)(2 * nfrag), (long long)nreads);
      return WFA_HIP_EINVAL;
    }
    return WFA_HIP_OK;
  }
  std::vector<uint64_t> seen((size_t)((nreads + 63) / 64), 0);
  for (int64_t f = 0; f < nfrag; ++f) {
    const int32_t m[2] = {mate1[f], mate2[f]};
    for (int s = 0; s < 2; ++s) {
      if (m[s] < 0 || m[s] >= nreads) {
        if (msg) snprintf(msg, cap, "pairing: mate out of range at fragment %lld: mate%d = %d over %lld reads", (long long)f, s + 1,
                          (int)m[s], (long long)nreads);
        return WFA_HIP_EINVAL;
      }
    }
    if (m[0] == m[1]) {
      if (msg) snprintf(msg, cap, "pairing: the mates of fragment %lld are one read: mate1 = mate2 = %d", (long long)f, (int)m[0]);
      return WFA_HIP_EINVAL;
    }
    for (int s = 0; s < 2; ++s) {
      uint64_t& word = seen[(size_t)(m[s] >> 6)];
      const uint64_t bit = 1ull << (m[s] & 63);
      if (word & bit) {
        if (msg) snprintf(msg, cap, "pairing: read %d is named by two fragments, the second time at fragment %lld as mate%d", (int)m[s],
                          (long long)f, s + 1);
        return WFA_HIP_EINVAL;
      }
      word |= bit;
    }
  }
  return WFA_HIP_OK;
}

}  // namespace wfa

namespace {

inline int32_t saturate(int64_t v) {
  return (int32_t)(v < (int64_t)INT32_MIN + 1 ? (int64_t)INT32_MIN + 1 : v > (int64_t)INT32_MAX ? (int64_t)INT32_MAX : v);
}

}  // namespace

extern "C" int wfa_hip_pair_host(int64_t nreads, int64_t nhits, const int32_t* i, const int32_t* j, const uint8_t* reverse,
                                 const int32_t* score, const int32_t* status, const int32_t* text_start, const int32_t* text_end,
                                 int32_t min_score, int32_t full_gap, int32_t min_insert, int32_t max_insert, int32_t unpaired,
                                 int64_t nfrag, const int32_t* mate1, const int32_t* mate2, int32_t* rows, uint8_t* flags,
                                 int32_t* pair_rows, uint8_t* pair_flags, char* msg, size_t msg_cap) {
  if (msg && msg_cap) msg[0] = 0;
  // the single-end rows and flags into arrays of this call: a refusal of the placement rule leaves the caller's untouched
  std::vector<int32_t> se((size_t)(nreads > 0 ? nreads : 0) * WFA_HIP_PLACE_COLS);
  std::vector<uint8_t> sf((size_t)(nhits > 0 && nhits <= (int64_t)INT32_MAX ? nhits : 0));
  int rc = wfa_hip_place_host(nreads, nhits, i, j, reverse, score, status, text_start, text_end, min_score, full_gap,
                              se.empty() ? nullptr : se.data(), sf.empty() ? nullptr : sf.data(), msg, msg_cap);
  if (rc != WFA_HIP_OK) return rc;
  rc = wfa::pair_check(nreads, min_insert, max_insert, unpaired, nfrag, mate1, mate2, msg, msg_cap);
  if (rc != WFA_HIP_OK) return rc;
  if (nfrag > 0 && !pair_rows) { if (msg) snprintf(msg, msg_cap, "pairing: a missing array"); return WFA_HIP_EINVAL; }

  auto eligible = [&](int64_t h) { return status[h] == 0 && score[h] >= min_score; };
  auto rev_of = [&](int64_t h) { return reverse && reverse[h] ? 1 : 0; };
  auto same_locus = [&](int64_t h, int64_t p) {                 // SAME LOCUS of "placement", p in the role of the primary
    if (h == p || j[h] != j[p] || rev_of(h) != rev_of(p)) return false;
    const int64_t te = text_end[h] < text_end[p] ? text_end[h] : text_end[p];
    const int64_t ts = text_start[h] > text_start[p] ? text_start[h] : text_start[p];
    const int64_t ov = te - ts, len_h = (int64_t)text_end[h] - text_start[h], len_p = (int64_t)text_end[p] - text_start[p];
    return ov > 0 && 2 * ov >= (len_h < len_p ? len_h : len_p);
  };
  // PROPER of a pairing of eligible hits; *insert receives te_R - ts_F
  auto proper_pairing = [&](int64_t h, int64_t g, int64_t* insert) {
    if (j[h] != j[g] || rev_of(h) == rev_of(g)) return false;
    if (text_end[h] <= text_start[h] || text_end[g] <= text_start[g]) return false;
    const int64_t F = rev_of(h) ? g : h, R = rev_of(h) ? h : g;
    if (text_start[F] > text_start[R] || text_end[F] > text_end[R]) return false;
    *insert = (int64_t)text_end[R] - text_start[F];
    return *insert >= min_insert && *insert <= max_insert;
  };

  std::vector<std::vector<int64_t>> group((size_t)nreads);      // the ELIGIBLE hit numbers of every read, ascending
  for (int64_t h = 0; h < nhits; ++h)
    if (eligible(h)) group[(size_t)i[h]].push_back(h);
  if (rows) for (size_t q = 0; q < se.size(); ++q) rows[q] = se[q];
  if (flags) for (size_t q = 0; q < sf.size(); ++q) flags[q] = sf[q];
  if (pair_flags) for (size_t q = 0; q < sf.size(); ++q) pair_flags[q] = sf[q];

  for (int64_t f = 0; f < nfrag; ++f) {
    const int64_t r1 = mate1 ? mate1[f] : 2 * f, r2 = mate2 ? mate2[f] : 2 * f + 1;
    const int32_t* s1 = se.data() + r1 * WFA_HIP_PLACE_COLS;
    const int32_t* s2 = se.data() + r2 * WFA_HIP_PLACE_COLS;
    const std::vector<int64_t>&g1 = group[(size_t)r1], &g2 = group[(size_t)r2];
    int32_t* row = pair_rows + f * WFA_HIP_PAIR_COLS;
    // not proper: the single-end primaries
    row[0] = s1[0]; row[1] = s2[0]; row[2] = 0; row[3] = INT32_MIN; row[4] = INT32_MIN; row[5] = 0; row[6] = s1[3]; row[7] = s2[3];
    row[8] = 0; row[9] = 0; row[10] = 0; row[11] = 0;
    if ((int64_t)g1.size() * (int64_t)g2.size() > (int64_t)WFA_HIP_PAIR_MAX_PAIRINGS) { row[11] = 1; continue; }
    int64_t bh = -1, bg = -1, best = 0, best_insert = 0, pairings = 0;
    for (int64_t h : g1)
      for (int64_t g : g2) {
        int64_t insert;
        if (!proper_pairing(h, g, &insert)) continue;
        ++pairings;
        const int64_t ps = (int64_t)score[h] + score[g];
        if (bh < 0 || ps > best) { bh = h; bg = g; best = ps; best_insert = insert; }   // (ascending h, then g: the first of the greatest)
      }
    row[9] = (int32_t)pairings;
    if (bh < 0 || best + unpaired < (int64_t)s1[1] + s2[1]) continue;
    bool any = false;
    int64_t second = 0, ties = 0;
    for (int64_t h : g1) {
      const bool at_h = h == bh || same_locus(h, bh);
      for (int64_t g : g2) {
        int64_t insert;
        if (!proper_pairing(h, g, &insert)) continue;
        if (at_h && (g == bg || same_locus(g, bg))) continue;     // at the chosen place (the chosen pairing among them)
        const int64_t ps = (int64_t)score[h] + score[g];
        if (!any || ps > second) second = ps;
        any = true;
        if (ps == best) ++ties;
      }
    }
    int32_t mapq = 60;
    if (any) {
      const int64_t q = 60 * (best - second) / full_gap;          // (best >= second: a floor division)
      mapq = (int32_t)(q < 60 ? q : 60);
    }
    row[0] = (int32_t)bh; row[1] = (int32_t)bg; row[2] = 1; row[3] = saturate(best); row[4] = any ? saturate(second) : INT32_MIN;
    row[5] = mapq;
    row[6] = sf[(size_t)bh] >= 2 && s1[3] > mapq ? s1[3] : mapq;
    row[7] = sf[(size_t)bg] >= 2 && s2[3] > mapq ? s2[3] : mapq;
    row[8] = (int32_t)best_insert; row[10] = (int32_t)ties;
    if (pair_flags) {
      for (int64_t h : g1) pair_flags[h] = h == bh ? 3 : same_locus(h, bh) ? 2 : 1;
      for (int64_t g : g2) pair_flags[g] = g == bg ? 3 : same_locus(g, bg) ? 2 : 1;
    }
  }
  return WFA_HIP_OK;
}
