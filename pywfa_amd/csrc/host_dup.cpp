// host_dup.cpp — host only, needs no GPU: the duplicate rule of include/wfa_hip.h ("duplicates") stated in plain C++ over arrays of hits
// (wfa_hip_duplicates_host_ex; wfa_hip_duplicates_host is a call of it), built on the pairing rule of host_pair.cpp, the clips of one
// op string (wfa_hip_ops_clips), the summed base quality of one read (wfa_hip_qsum_host), and the checks the device entries share with
// them (wfa_hip_placer_duplicates_ex and wfa_hip_placer_add_hits_clips in api_place.hip).  The kernels of k_dup.hip and the record
// kernel's clip word are held to these statements.
#include <stdint.h>
#include <stdio.h>
#include <limits.h>
#include <algorithm>
#include <vector>
#include "wfa_hip.h"

namespace wfa {

// the outputs of one run: read_rows where there are reads, pair_rows where there are fragments
int dup_check(int64_t nreads, int64_t nfrag, const int32_t* read_rows, const int32_t* pair_rows, char* msg, size_t cap) {
  if ((nreads > 0 && !read_rows) || (nfrag > 0 && !pair_rows)) {
    if (msg) snprintf(msg, cap, "duplicates: a missing array (%s)", nreads > 0 && !read_rows ? "read_rows" : "pair_rows");
    return WFA_HIP_EINVAL;
  }
  return WFA_HIP_OK;
}

// flags and what goes with them: no unknown bit; the quality flag and a quality source come together; min_quality 0 .. 93
int dup_check_flags(int flags, bool have_quals, int32_t min_quality, char* msg, size_t cap) {
  const int known = WFA_HIP_DUP_UNCLIPPED | WFA_HIP_DUP_BY_QUALITY;
  const char* what = nullptr;
  if (flags & ~known) what = "an unknown flag bit";
  else if ((flags & WFA_HIP_DUP_BY_QUALITY) && !have_quals) what = "WFA_HIP_DUP_BY_QUALITY without qualities";
  else if (!(flags & WFA_HIP_DUP_BY_QUALITY) && have_quals) what = "qualities without WFA_HIP_DUP_BY_QUALITY";
  if (what) { if (msg) snprintf(msg, cap, "duplicates: flags = %d: %s", flags, what); return WFA_HIP_EINVAL; }
  if ((flags & WFA_HIP_DUP_BY_QUALITY) && (min_quality < 0 || min_quality > WFA_HIP_MAX_QUALITY)) {
    if (msg) snprintf(msg, cap, "duplicates: min_quality = %d is out of range (0 .. %d)", (int)min_quality, WFA_HIP_MAX_QUALITY);
    return WFA_HIP_EINVAL;
  }
  return WFA_HIP_OK;
}

// the clips of n hits about to be appended behind `base` (either array nullable: 0)
int dup_check_clips(int64_t base, int64_t n, const int32_t* lead, const int32_t* trail, char* msg, size_t cap) {
  for (int64_t q = 0; q < n; ++q)
    if ((lead && lead[q] < 0) || (trail && trail[q] < 0)) {
      if (msg) snprintf(msg, cap, "clips: a negative clip at position %lld of the hit list: lead = %d, trail = %d", (long long)(base + q),
                        lead ? (int)lead[q] : 0, trail ? (int)trail[q] : 0);
      return WFA_HIP_EINVAL;
    }
  return WFA_HIP_OK;
}

}  // namespace wfa

extern "C" int wfa_hip_ops_clips(const uint8_t* ops, int64_t ops_len, int32_t plen, int32_t tlen, int32_t* lead, int32_t* trail) {
  if (!lead || !trail || ops_len < 0 || (ops_len > 0 && !ops) || plen < 0 || tlen < 0) return WFA_HIP_EINVAL;
  *lead = *trail = 0;
  if (ops_len == 0 || plen == 0 || tlen == 0) return WFA_HIP_OK;
  int64_t first = -1, last = -1;
  for (int64_t k = 0; k < ops_len; ++k)
    if (ops[k] == 'M') { if (first < 0) first = k; last = k; }
  if (first < 0) return WFA_HIP_OK;
  int64_t l = 0, t = 0;
  for (int64_t k = 0; k < first; ++k) l += ops[k] == 'X' || ops[k] == 'D';
  for (int64_t k = last + 1; k < ops_len; ++k) t += ops[k] == 'X' || ops[k] == 'D';
  *lead = (int32_t)std::min<int64_t>(l, WFA_HIP_CLIP_MAX);
  *trail = (int32_t)std::min<int64_t>(t, WFA_HIP_CLIP_MAX);
  return WFA_HIP_OK;
}

extern "C" int wfa_hip_qsum_host(const uint8_t* quals, int64_t len, int32_t min_quality, int32_t* out) {
  if (!out || len < 0 || (len > 0 && !quals) || min_quality < 0 || min_quality > WFA_HIP_MAX_QUALITY) return WFA_HIP_EINVAL;
  int64_t sum = 0;
  for (int64_t k = 0; k < len; ++k)
    if ((int32_t)quals[k] >= min_quality) sum += quals[k];
  *out = (int32_t)std::min<int64_t>(sum, INT32_MAX);
  return WFA_HIP_OK;
}

namespace {

// one UNIT of the rule; the order is (text, bucket position, kind, the rest of the key), then best first: greatest score, smallest number
struct Unit {
  int32_t j; int64_t b;
  int32_t kind;        // pair units: `first` (1 or 2); read units: 3 forward, 4 reverse — a pair unit and a read unit never share a key
  int32_t end;         // pair units: te_R; read units: 0
  int32_t score, unit;
  bool pair;
  bool same_bucket(const Unit& o) const { return j == o.j && b == o.b; }
  bool same_key(const Unit& o) const { return same_bucket(o) && kind == o.kind && end == o.end; }
  bool operator<(const Unit& o) const {
    if (j != o.j) return j < o.j;
    if (b != o.b) return b < o.b;
    if (kind != o.kind) return kind < o.kind;
    if (end != o.end) return end < o.end;
    if (score != o.score) return score > o.score;
    return unit < o.unit;
  }
};

}  // namespace

extern "C" int wfa_hip_duplicates_host_ex(int64_t nreads, int64_t nhits, const int32_t* i, const int32_t* j, const uint8_t* reverse,
                                          const int32_t* score, const int32_t* status, const int32_t* text_start, const int32_t* text_end,
                                          int32_t min_score, int32_t full_gap, int32_t min_insert, int32_t max_insert, int32_t unpaired,
                                          int64_t nfrag, const int32_t* mate1, const int32_t* mate2, int64_t ntexts, const int32_t* text_len,
                                          int32_t* read_rows, int32_t* pair_rows, const int32_t* lead, const int32_t* trail, int flags,
                                          const int32_t* qsum, char* msg, size_t msg_cap) {
  if (msg && msg_cap) msg[0] = 0;
  int rc = wfa::dup_check_flags(flags, qsum != nullptr, 0, msg, msg_cap);
  if (rc != WFA_HIP_OK) return rc;
  rc = wfa::dup_check_clips(0, nhits > 0 ? nhits : 0, lead, trail, msg, msg_cap);
  if (rc != WFA_HIP_OK) return rc;
  for (int64_t r = 0; qsum && r < nreads; ++r)
    if (qsum[r] < 0) {
      if (msg) snprintf(msg, msg_cap, "duplicates: a negative quality sum of read %lld: qsum = %d", (long long)r, (int)qsum[r]);
      return WFA_HIP_EINVAL;
    }
  if (ntexts < 0) { if (msg) snprintf(msg, msg_cap, "duplicates: a negative number of texts (%lld)", (long long)ntexts); return WFA_HIP_EINVAL; }
  if (ntexts > 0 && !text_len) { if (msg) snprintf(msg, msg_cap, "duplicates: a missing array (text_len)"); return WFA_HIP_EINVAL; }
  for (int64_t t = 0; t < ntexts; ++t)
    if (text_len[t] < 0) {
      if (msg) snprintf(msg, msg_cap, "duplicates: negative length of text %lld: text_len = %d", (long long)t, (int)text_len[t]);
      return WFA_HIP_EINVAL;
    }
  // the pair rule by the host statement, into arrays of this call (its refusals leave the caller's outputs untouched)
  std::vector<int32_t> se((size_t)(nreads > 0 ? nreads : 0) * WFA_HIP_PLACE_COLS);
  std::vector<int32_t> pr((size_t)(nfrag > 0 && nfrag <= nreads ? nfrag : 0) * WFA_HIP_PAIR_COLS);
  rc = wfa_hip_pair_host(nreads, nhits, i, j, reverse, score, status, text_start, text_end, min_score, full_gap, min_insert, max_insert,
                             unpaired, nfrag, mate1, mate2, se.empty() ? nullptr : se.data(), nullptr, pr.empty() ? nullptr : pr.data(), nullptr,
                             msg, msg_cap);
  if (rc != WFA_HIP_OK) return rc;
  for (int64_t h = 0; h < nhits; ++h)
    if (j[h] >= ntexts) {
      if (msg) snprintf(msg, msg_cap, "duplicates: text index out of range at position %lld of the hit list: j = %d over %lld texts",
                        (long long)h, (int)j[h], (long long)ntexts);
      return WFA_HIP_EINVAL;
    }
  rc = wfa::dup_check(nreads, nfrag, read_rows, pair_rows, msg, msg_cap);
  if (rc != WFA_HIP_OK) return rc;

  auto rev_of = [&](int64_t h) { return reverse && reverse[h] ? 1 : 0; };
  // the interval the keys and buckets are made of: the core, or the unclipped one (64-bit, the clips saturated)
  const bool unclipped = (flags & WFA_HIP_DUP_UNCLIPPED) != 0, by_quality = (flags & WFA_HIP_DUP_BY_QUALITY) != 0;
  auto clip = [&](const int32_t* c, int64_t h) { return unclipped && c ? std::min<int64_t>(c[h], WFA_HIP_CLIP_MAX) : (int64_t)0; };
  auto start_of = [&](int64_t h) { return (int64_t)text_start[h] - clip(lead, h); };
  auto end_of = [&](int64_t h) { return (int64_t)text_end[h] + clip(trail, h); };
  auto lone_row = [&](int32_t* rows, int64_t at) {
    int32_t* w = rows + at * WFA_HIP_DUP_COLS;
    w[0] = (int32_t)at; w[1] = 1; w[2] = 0; w[3] = 0;
  };
  auto row = [](int32_t* rows, int64_t at, int32_t rep, int32_t size, int32_t dup, int32_t overflow) {
    int32_t* w = rows + at * WFA_HIP_DUP_COLS;
    w[0] = rep; w[1] = size; w[2] = dup; w[3] = overflow;
  };
  // UNITS: the pair units first, then the reads no pair unit owns
  std::vector<Unit> units;
  std::vector<uint8_t> owned((size_t)nreads, 0);   // 1: a mate of a pair unit
  for (int64_t r = 0; r < nreads; ++r) row(read_rows, r, -1, 0, 0, 0);
  for (int64_t f = 0; f < nfrag; ++f) {
    row(pair_rows, f, -1, 0, 0, 0);
    const int32_t* p = pr.data() + f * WFA_HIP_PAIR_COLS;
    if (p[2] != 1) continue;
    const int64_t r1 = mate1 ? mate1[f] : 2 * f, r2 = mate2 ? mate2[f] : 2 * f + 1;
    owned[(size_t)r1] = owned[(size_t)r2] = 1;
    const int32_t h = p[0], g = p[1];
    const bool h_fwd = rev_of(h) == 0;
    const int32_t F = h_fwd ? h : g, R = h_fwd ? g : h;
    const int64_t end = end_of(R);
    if (end > (int64_t)INT32_MAX) { lone_row(pair_rows, f); continue; }   // a key coordinate beyond int32: alone, overflow 0
    const int32_t sc = by_quality ? (int32_t)std::min<int64_t>((int64_t)qsum[r1] + qsum[r2], INT32_MAX) : p[3];
    units.push_back(Unit{j[F], start_of(F), h_fwd ? 1 : 2, (int32_t)end, sc, (int32_t)f, true});
  }
  for (int64_t r = 0; r < nreads; ++r) {
    if (owned[(size_t)r]) continue;
    const int32_t* s = se.data() + r * WFA_HIP_PLACE_COLS;
    const int32_t h = s[0];
    if (h < 0 || text_end[h] <= text_start[h]) continue;
    const int rv = rev_of(h);
    units.push_back(Unit{j[h], rv ? end_of(h) - 1 : start_of(h), rv ? 4 : 3, 0, by_quality ? qsum[r] : s[1], (int32_t)r, false});
  }
  std::sort(units.begin(), units.end());
  // BUCKETS, and inside them the GROUPS: both are runs of the sorted units, a group's first unit its representative
  for (size_t b0 = 0; b0 < units.size();) {
    size_t b1 = b0 + 1;
    while (b1 < units.size() && units[b1].same_bucket(units[b0])) ++b1;
    const Unit& u0 = units[b0];
    const bool outside = u0.b < 0 || u0.b >= (int64_t)text_len[u0.j];
    const bool overflow = !outside && b1 - b0 > (size_t)WFA_HIP_DUP_MAX_BUCKET;
    for (size_t g0 = b0; g0 < b1;) {
      size_t g1 = g0 + 1;
      while (g1 < b1 && units[g1].same_key(units[g0])) ++g1;
      for (size_t q = g0; q < g1; ++q) {
        const Unit& u = units[q];
        const bool alone = outside || overflow;
        const int32_t rep = alone ? u.unit : units[g0].unit, size = alone ? 1 : (int32_t)(g1 - g0);
        const int32_t dup = rep != u.unit ? 1 : 0, ovf = overflow ? 1 : 0;
        if (!u.pair) { row(read_rows, u.unit, rep, size, dup, ovf); continue; }
        row(pair_rows, u.unit, rep, size, dup, ovf);
        const int64_t f = u.unit;
        row(read_rows, mate1 ? mate1[f] : 2 * f, -1, 0, dup, ovf);
        row(read_rows, mate2 ? mate2[f] : 2 * f + 1, -1, 0, dup, ovf);
      }
      g0 = g1;
    }
    b0 = b1;
  }
  return WFA_HIP_OK;
}

extern "C" int wfa_hip_duplicates_host(int64_t nreads, int64_t nhits, const int32_t* i, const int32_t* j, const uint8_t* reverse,
                                       const int32_t* score, const int32_t* status, const int32_t* text_start, const int32_t* text_end,
                                       int32_t min_score, int32_t full_gap, int32_t min_insert, int32_t max_insert, int32_t unpaired,
                                       int64_t nfrag, const int32_t* mate1, const int32_t* mate2, int64_t ntexts, const int32_t* text_len,
                                       int32_t* read_rows, int32_t* pair_rows, char* msg, size_t msg_cap) {
  return wfa_hip_duplicates_host_ex(nreads, nhits, i, j, reverse, score, status, text_start, text_end, min_score, full_gap, min_insert,
                                    max_insert, unpaired, nfrag, mate1, mate2, ntexts, text_len, read_rows, pair_rows, nullptr, nullptr, 0,
                                    nullptr, msg, msg_cap);
}
