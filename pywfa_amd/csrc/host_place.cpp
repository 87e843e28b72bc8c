// host_place.cpp — host only, needs no GPU: the placement rule of include/wfa_hip.h ("placement") stated in plain C++ over arrays of
// hits (wfa_hip_place_host), and the checks the device entries share with it (wfa_hip_placer_add / _add_hits / _run in wfa_hip.hip).
// The kernels of k_place.hip are held to this statement.
#include <stdint.h>
#include <stdio.h>
#include <limits.h>
#include <vector>
#include "wfa_hip.h"

namespace wfa {

// the hits [0, n) of one add, `base` hits being recorded already: every i inside [0, nreads), no negative j or text_start, no
// text_end below its text_start (text_end NULL: a batch's pairs, whose ends the device derives), the total within 2^31 - 1
int place_check_hits(int64_t nreads, int64_t base, int64_t n, const int32_t* i, const int32_t* j, const int32_t* text_start,
                     const int32_t* text_end, char* msg, size_t cap) {
  if (n < 0) { if (msg) snprintf(msg, cap, "placement: a negative number of hits (%lld)", (long long)n); return WFA_HIP_EINVAL; }
  if (base + n > (int64_t)INT32_MAX) {
    if (msg) snprintf(msg, cap, "placement: %lld + %lld hits are more than 2^31 - 1", (long long)base, (long long)n);
    return WFA_HIP_EINVAL;
  }
  if (n > 0 && (!i || !j)) { if (msg) snprintf(msg, cap, "placement: the index arrays i and j are missing"); return WFA_HIP_EINVAL; }
  for (int64_t q = 0; q < n; ++q) {
    if (i[q] < 0 || i[q] >= nreads) {
      if (msg) snprintf(msg, cap, "placement: read index out of range at position %lld of the hit list: i = %d over %lld reads",
                        (long long)q, (int)i[q], (long long)nreads);
      return WFA_HIP_EINVAL;
    }
    if (j[q] < 0) {
      if (msg) snprintf(msg, cap, "placement: negative text index at position %lld of the hit list: j = %d", (long long)q, (int)j[q]);
      return WFA_HIP_EINVAL;
    }
    if (text_start && text_start[q] < 0) {
      if (msg) snprintf(msg, cap, "placement: negative text start at position %lld of the hit list: text_start = %d", (long long)q,
                        (int)text_start[q]);
      return WFA_HIP_EINVAL;
    }
    if (text_start && text_end && text_end[q] < text_start[q]) {
      if (msg) snprintf(msg, cap, "placement: text_end below text_start at position %lld of the hit list: [%d, %d)", (long long)q,
                        (int)text_start[q], (int)text_end[q]);
      return WFA_HIP_EINVAL;
    }
  }
  return WFA_HIP_OK;
}

int place_check_run(int32_t full_gap, char* msg, size_t cap) {
  if (full_gap < 1) {
    if (msg) snprintf(msg, cap, "placement: full_gap = %d is out of range (at least 1)", (int)full_gap);
    return WFA_HIP_EINVAL;
  }
  return WFA_HIP_OK;
}

}  // namespace wfa

extern "C" int wfa_hip_place_host(int64_t nreads, int64_t nhits, const int32_t* i, const int32_t* j, const uint8_t* reverse,
                                  const int32_t* score, const int32_t* status, const int32_t* text_start, const int32_t* text_end,
                                  int32_t min_score, int32_t full_gap, int32_t* rows, uint8_t* flags, char* msg, size_t msg_cap) {
  if (msg && msg_cap) msg[0] = 0;
  if (nreads < 0) { if (msg) snprintf(msg, msg_cap, "placement: a negative number of reads (%lld)", (long long)nreads); return WFA_HIP_EINVAL; }
  int rc = wfa::place_check_run(full_gap, msg, msg_cap);
  if (rc != WFA_HIP_OK) return rc;
  if (nhits > (int64_t)INT32_MAX) return wfa::place_check_hits(nreads, 0, nhits, nullptr, nullptr, nullptr, nullptr, msg, msg_cap);
  if ((nhits > 0 && (!score || !status || !text_start || !text_end)) || (nreads > 0 && !rows)) {
    if (msg) snprintf(msg, msg_cap, "placement: a missing array");
    return WFA_HIP_EINVAL;
  }
  rc = wfa::place_check_hits(nreads, 0, nhits, i, j, text_start, text_end, msg, msg_cap);
  if (rc != WFA_HIP_OK) return rc;

  auto eligible = [&](int64_t h) { return status[h] == 0 && score[h] >= min_score; };
  std::vector<std::vector<int64_t>> group((size_t)nreads);     // the hit numbers of every read, ascending
  for (int64_t h = 0; h < nhits; ++h) {
    group[(size_t)i[h]].push_back(h);
    if (flags) flags[h] = 0;
  }
  for (int64_t r = 0; r < nreads; ++r) {
    int32_t* row = rows + r * WFA_HIP_PLACE_COLS;
    int64_t p = -1;
    int32_t hits = 0;
    for (int64_t h : group[(size_t)r]) {
      if (!eligible(h)) continue;
      ++hits;
      if (p < 0 || score[h] > score[p]) p = h;                 // (ascending numbers: the first of the greatest)
    }
    if (p < 0) {
      row[0] = -1; row[1] = INT32_MIN; row[2] = INT32_MIN; row[3] = 0; row[4] = 0; row[5] = 0; row[6] = 0; row[7] = 0;
      continue;
    }
    const int rev_p = reverse && reverse[p] ? 1 : 0;
    const int64_t len_p = (int64_t)text_end[p] - text_start[p];
    bool any = false;
    int32_t second = INT32_MIN, ties = 0;
    for (int64_t h : group[(size_t)r]) {
      if (!eligible(h)) continue;
      if (h == p) { if (flags) flags[h] = 3; continue; }
      const int rev_h = reverse && reverse[h] ? 1 : 0;
      const int64_t te = text_end[h] < text_end[p] ? text_end[h] : text_end[p];
      const int64_t ts = text_start[h] > text_start[p] ? text_start[h] : text_start[p];
      const int64_t ov = te - ts, len_h = (int64_t)text_end[h] - text_start[h];
      const bool same = j[h] == j[p] && rev_h == rev_p && ov > 0 && 2 * ov >= (len_h < len_p ? len_h : len_p);
      if (flags) flags[h] = same ? 2 : 1;
      if (same) continue;
      if (!any || score[h] > second) second = score[h];
      any = true;
      if (score[h] == score[p]) ++ties;
    }
    int32_t mapq = 60;
    if (any) {
      const int64_t q = 60 * ((int64_t)score[p] - second) / full_gap;   // (score[p] >= second: a floor division)
      mapq = (int32_t)(q < 60 ? q : 60);
    }
    row[0] = (int32_t)p; row[1] = score[p]; row[2] = any ? second : INT32_MIN; row[3] = mapq; row[4] = hits; row[5] = ties;
    row[6] = text_start[p]; row[7] = text_end[p];
  }
  return WFA_HIP_OK;
}
