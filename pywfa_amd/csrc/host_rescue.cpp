// host_rescue.cpp — host only, needs no GPU: the rescue rule of include/wfa_hip.h ("rescue") stated in plain C++ over arrays of hits
// (wfa_hip_rescue_host), built on the pairing rule of host_pair.cpp, and the checks the device entry shares with it
// (wfa_hip_placer_rescue in api_place.hip).  The kernels of k_rescue.hip are held to this statement.
#include <stdint.h>
#include <stdio.h>
#include <limits.h>
#include <vector>
#include "wfa_hip.h"

namespace wfa {

// the parameters of one rescue: pad, min_len and cap at least 0, anchor_mapq in 0 .. 60, a count, rows where cap > 0
int rescue_check(int32_t pad, int32_t min_len, int32_t anchor_mapq, int64_t cap, const int64_t* count, const int32_t* rows, char* msg,
                 size_t msg_cap) {
  if (pad < 0 || min_len < 0) {
    if (msg) snprintf(msg, msg_cap, "rescue: pad = %d, min_len = %d are out of range (at least 0)", (int)pad, (int)min_len);
    return WFA_HIP_EINVAL;
  }
  if (anchor_mapq < 0 || anchor_mapq > 60) {
    if (msg) snprintf(msg, msg_cap, "rescue: anchor_mapq = %d is out of range (0 .. 60)", (int)anchor_mapq);
    return WFA_HIP_EINVAL;
  }
  if (cap < 0) { if (msg) snprintf(msg, msg_cap, "rescue: cap = %lld is out of range (at least 0)", (long long)cap); return WFA_HIP_EINVAL; }
  if (!count || (cap > 0 && !rows)) { if (msg) snprintf(msg, msg_cap, "rescue: a missing array (%s)", count ? "rows" : "count"); return WFA_HIP_EINVAL; }
  return WFA_HIP_OK;
}

// the window of mate o from its partner's primary (j_a, reverse_a, [ts_a, te_a)): false when it is dropped
bool rescue_window(int32_t reverse_a, int32_t ts_a, int32_t te_a, int32_t len_o, int32_t tlen, int32_t min_insert, int32_t max_insert,
                   int32_t pad, int32_t min_len, int32_t* start, int32_t* len) {
  int64_t lo, hi;
  if (!reverse_a) {
    lo = (int64_t)ts_a + min_insert - len_o - pad;
    hi = (int64_t)ts_a + max_insert + pad;
  } else {
    lo = (int64_t)te_a - max_insert - pad;
    hi = (int64_t)te_a - min_insert + len_o + pad;
  }
  if (lo < 0) lo = 0;
  if (hi > tlen) hi = tlen;
  if (hi - lo < (min_len > 1 ? min_len : 1)) return false;
  *start = (int32_t)lo; *len = (int32_t)(hi - lo);   // (0 <= lo < hi <= tlen)
  return true;
}

}  // namespace wfa

extern "C" int wfa_hip_rescue_host(int64_t nreads, int64_t nhits, const int32_t* i, const int32_t* j, const uint8_t* reverse,
                                   const int32_t* score, const int32_t* status, const int32_t* text_start, const int32_t* text_end,
                                   int32_t min_score, int32_t full_gap, int32_t min_insert, int32_t max_insert, int32_t unpaired,
                                   int64_t nfrag, const int32_t* mate1, const int32_t* mate2, const int32_t* read_len, int64_t ntexts,
                                   const int32_t* text_len, int32_t pad, int32_t min_len, int32_t anchor_mapq, int64_t cap,
                                   int64_t* count, int32_t* rows, char* msg, size_t msg_cap) {
  if (msg && msg_cap) msg[0] = 0;
  int rc = wfa::rescue_check(pad, min_len, anchor_mapq, cap, count, rows, msg, msg_cap);
  if (rc != WFA_HIP_OK) return rc;
  if (ntexts < 0) { if (msg) snprintf(msg, msg_cap, "rescue: a negative number of texts (%lld)", (long long)ntexts); return WFA_HIP_EINVAL; }
  if ((nreads > 0 && !read_len) || (ntexts > 0 && !text_len)) {
    if (msg) snprintf(msg, msg_cap, "rescue: a missing array (%s)", nreads > 0 && !read_len ? "read_len" : "text_len");
    return WFA_HIP_EINVAL;
  }
  for (int64_t r = 0; r < nreads; ++r)
    if (read_len[r] < 0) {
      if (msg) snprintf(msg, msg_cap, "rescue: negative length of read %lld: read_len = %d", (long long)r, (int)read_len[r]);
      return WFA_HIP_EINVAL;
    }
  for (int64_t t = 0; t < ntexts; ++t)
    if (text_len[t] < 0) {
      if (msg) snprintf(msg, msg_cap, "rescue: negative length of text %lld: text_len = %d", (long long)t, (int)text_len[t]);
      return WFA_HIP_EINVAL;
    }
  // the pair rule by the host statement, into arrays of this call (its refusals leave the caller's outputs untouched)
  // (more fragments than reads name a read twice: refused below, nothing to size for)
  std::vector<int32_t> se((size_t)(nreads > 0 ? nreads : 0) * WFA_HIP_PLACE_COLS);
  std::vector<int32_t> pr((size_t)(nfrag > 0 && nfrag <= nreads ? nfrag : 0) * WFA_HIP_PAIR_COLS);
  rc = wfa_hip_pair_host(nreads, nhits, i, j, reverse, score, status, text_start, text_end, min_score, full_gap, min_insert, max_insert,
                         unpaired, nfrag, mate1, mate2, se.empty() ? nullptr : se.data(), nullptr, pr.empty() ? nullptr : pr.data(), nullptr,
                         msg, msg_cap);
  if (rc != WFA_HIP_OK) return rc;
  for (int64_t h = 0; h < nhits; ++h)
    if (j[h] >= ntexts) {
      if (msg) snprintf(msg, msg_cap, "rescue: text index out of range at position %lld of the hit list: j = %d over %lld texts",
                        (long long)h, (int)j[h], (long long)ntexts);
      return WFA_HIP_EINVAL;
    }

  int64_t n = 0;
  for (int64_t f = 0; f < nfrag; ++f) {
    const int32_t* row = pr.data() + f * WFA_HIP_PAIR_COLS;
    if (row[2] != 0 || row[9] != 0 || row[11] != 0) continue;   // proper, pairings, overflow: not a rescued fragment
    const int64_t m[2] = {mate1 ? mate1[f] : 2 * f, mate2 ? mate2[f] : 2 * f + 1};
    for (int s = 0; s < 2; ++s) {
      const int32_t* srow = se.data() + m[s] * WFA_HIP_PLACE_COLS;
      const int32_t a = srow[0];
      if (a < 0 || text_end[a] <= text_start[a] || srow[3] < anchor_mapq) continue;
      const int32_t rev_a = reverse && reverse[a] ? 1 : 0;
      const int64_t o = m[1 - s];
      int32_t start, len;
      if (!wfa::rescue_window(rev_a, text_start[a], text_end[a], read_len[o], text_len[j[a]], min_insert, max_insert, pad, min_len, &start, &len))
        continue;
      if (n < cap) {
        int32_t* w = rows + n * WFA_HIP_RESCUE_COLS;
        w[0] = (int32_t)o; w[1] = j[a]; w[2] = start; w[3] = len; w[4] = 1 - rev_a; w[5] = (int32_t)f; w[6] = a; w[7] = 0;
      }
      ++n;
    }
  }
  *count = n;
  return WFA_HIP_OK;
}
