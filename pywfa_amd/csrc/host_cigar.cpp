// host_cigar.cpp — host-only text helpers of the C ABI (include/wfa_hip.h): what pywfa prints through WFA2-lib's
// cigar_print_pretty (align.pyx:445-459 -> alignment/cigar.c:778-863), as a string a binding can write wherever it likes.
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <map>
#include <stdlib.h>
#include <string>
#include <string.h>
#include <vector>
#include "wfa_hip.h"

namespace {
// "{n}{op}" runs of ops[0..len) (cigar.c:705-739); with_matches = false leaves the M runs out
void append_runs(std::string& out, const uint8_t* ops, int64_t len, bool with_matches, bool fold_mismatches) {
  int64_t i = 0;
  char num[24];
  while (i < len) {
    const uint8_t op = (fold_mismatches && ops[i] == 'X') ? (uint8_t)'M' : ops[i];
    int64_t j = i + 1;
    while (j < len && ((fold_mismatches && ops[j] == 'X') ? (uint8_t)'M' : ops[j]) == op) ++j;
    if (with_matches || op != 'M') { snprintf(num, sizeof(num), "%lld", (long long)(j - i)); out += num; out += (char)op; }
    i = j;
  }
}
}  // namespace

extern "C" int64_t wfa_hip_cigar_sprint_pretty(const uint8_t* ops, int64_t ops_len, const uint8_t* pattern, int32_t plen,
                                               const uint8_t* text, int32_t tlen, char* out, int64_t cap) {
  if (ops_len < 0 || plen < 0 || tlen < 0 || (ops_len > 0 && !ops) || (plen > 0 && !pattern) || (tlen > 0 && !text) || (cap > 0 && !out)) return WFA_HIP_EINVAL;
  std::string rp, rg, rt;
  rp.reserve((size_t)ops_len + 16); rg.reserve((size_t)ops_len + 16); rt.reserve((size_t)ops_len + 16);
  int32_t pp = 0, tp = 0;
  for (int64_t i = 0; i < ops_len; ++i) {
    const uint8_t op = ops[i];
    const bool hp = pp < plen, ht = tp < tlen;
    if (op == 'M' || op == 'X') {
      if (!hp || !ht) break;   // (an op string that outruns its sequences: nothing more to draw)
      const bool same = pattern[pp] == text[tp];
      // a match is drawn '|', a mismatch ' '; an op that contradicts the sequences is marked 'X' (cigar.c:799-821)
      rg += (op == 'M') ? (same ? '|' : 'X') : (same ? 'X' : ' ');
      rp += (char)pattern[pp++]; rt += (char)text[tp++];
    } else if (op == 'I') {
      if (!ht) break;
      rp += '-'; rg += ' '; rt += (char)text[tp++];
    } else if (op == 'D') {
      if (!hp) break;
      rp += (char)pattern[pp++]; rg += ' '; rt += '-';
    }
  }
  // whatever the op string leaves unaligned follows, marked '?' (cigar.c:836-847)
  const int32_t rest_p = plen - pp, rest_t = tlen - tp;
  rp.append(reinterpret_cast<const char*>(pattern) + pp, (size_t)rest_p);
  rt.append(reinterpret_cast<const char*>(text) + tp, (size_t)rest_t);
  rg.append((size_t)(rest_p > rest_t ? rest_p : rest_t), '?');
  std::string s = "      ALIGNMENT ";
  append_runs(s, ops, ops_len, true, false);
  s += "\n      ETRACE    ";
  append_runs(s, ops, ops_len, false, false);
  s += "\n      CIGAR     ";
  append_runs(s, ops, ops_len, true, true);   // SAM style without '=' / 'X' (cigar_print_SAM_CIGAR(.., false))
  s += "\n      PATTERN    " + rp + "\n                 " + rg + "\n      TEXT       " + rt + "\n";
  if (cap > 0) {
    const size_t ncopy = s.size() < (size_t)cap - 1 ? s.size() : (size_t)cap - 1;
    memcpy(out, s.data(), ncopy);
    out[ncopy] = '\0';
  }
  return (int64_t)s.size();
}

// ---- the two reductions of an op string, stated for one pair in plain C (the kernels: wfa_summary.hpp, k_pileup.hip) ----------------

namespace {
// the aligned core [first M, last M] of ops[0..len); false: no M
bool aligned_core(const uint8_t* ops, int64_t len, int64_t* first, int64_t* last) {
  int64_t f = 0, l = len - 1;
  while (f < len && ops[f] != 'M') ++f;
  if (f >= len) return false;
  while (ops[l] != 'M') --l;
  *first = f; *last = l;
  return true;
}
}  // namespace

extern "C" int wfa_hip_ops_summary(const uint8_t* ops, int64_t ops_len, int32_t plen, int32_t tlen, int32_t* out10) {
  if (ops_len < 0 || plen < 0 || tlen < 0 || (ops_len > 0 && !ops) || !out10) return WFA_HIP_EINVAL;
  for (int k = 0; k < WFA_HIP_SUMMARY_COLS; ++k) out10[k] = 0;
  for (int64_t i = 0; i < ops_len; ++i) {
    const uint8_t c = ops[i];
    const bool run_start = i == 0 || ops[i - 1] != c;
    if (c == 'M') out10[0] += 1;
    else if (c == 'X') out10[1] += 1;
    else if (c == 'I') { out10[2] += 1; out10[4] += run_start; }
    else if (c == 'D') { out10[3] += 1; out10[5] += run_start; }
  }
  if (ops_len == 0 || plen == 0 || tlen == 0) return WFA_HIP_OK;
  // locations (align.pyx:797-831 with a threshold of 1): the ops in front of the first and behind the last M stripped; without an
  // M both scans run through the whole string
  int64_t first = ops_len, last = -1;
  (void)aligned_core(ops, ops_len, &first, &last);
  int32_t ps = 0, ts = 0, pe = plen, te = tlen;
  for (int64_t i = 0; i < first; ++i) { const uint8_t c = ops[i]; ps += (c == 'D' || c == 'X'); ts += (c == 'I' || c == 'X'); }
  for (int64_t i = ops_len - 1; i > last; --i) { const uint8_t c = ops[i]; pe -= (c == 'D' || c == 'X'); te -= (c == 'I' || c == 'X'); }
  out10[6] = ps; out10[7] = pe; out10[8] = ts; out10[9] = te;
  return WFA_HIP_OK;
}

extern "C" int wfa_hip_ops_pileup(const uint8_t* ops, int64_t ops_len, const uint8_t* pattern, int32_t plen, int32_t tlen, int32_t* rows) {
  if (ops_len < 0 || plen < 0 || tlen < 0 || (ops_len > 0 && !ops) || (plen > 0 && !pattern) || (tlen > 0 && !rows)) return WFA_HIP_EINVAL;
  // an op string that outruns its pair is refused before anything is added
  int64_t nv = 0, nh = 0;
  for (int64_t i = 0; i < ops_len; ++i) { const uint8_t c = ops[i]; nv += (c == 'M' || c == 'X' || c == 'D'); nh += (c == 'M' || c == 'X' || c == 'I'); }
  if (nv > plen || nh > tlen) return WFA_HIP_EINVAL;
  int64_t first = 0, last = -1;
  if (!aligned_core(ops, ops_len, &first, &last)) return WFA_HIP_OK;
  int32_t v = 0, h = 0;
  for (int64_t i = 0; i <= last; ++i) {
    const uint8_t c = ops[i];
    const bool in = i >= first;
    int32_t* row = rows + (int64_t)WFA_HIP_PILEUP_COLS * h;
    if (c == 'M' || c == 'X') {
      if (in) {
        const uint8_t l = pattern[v];
        row[l == 'A' ? 0 : l == 'C' ? 1 : l == 'G' ? 2 : l == 'T' ? 3 : 4] += 1;
        if (c == 'X') row[7] += 1;
      }
      ++v; ++h;
    } else if (c == 'I') {
      if (in) row[5] += 1;
      ++h;
    } else if (c == 'D') {
      if (in && ops[i - 1] != 'D') row[6] += 1;   // (inside the core a D has an op in front of it)
      ++v;
    }
  }
  return WFA_HIP_OK;
}

// the pileup with base qualities (include/wfa_hip.h, "base qualities"): quals[v] is the quality of pattern[v]
extern "C" int wfa_hip_ops_pileup_quals(const uint8_t* ops, int64_t ops_len, const uint8_t* pattern, int32_t plen, int32_t tlen, const uint8_t* quals,
                                        int32_t min_base_quality, int32_t quality_cap, int32_t* rows, int32_t* qrows) {
  if (ops_len < 0 || plen < 0 || tlen < 0 || (ops_len > 0 && !ops) || (plen > 0 && (!pattern || !quals)) || (tlen > 0 && (!rows || !qrows)) ||
      min_base_quality < 0 || min_base_quality > WFA_HIP_MAX_QUALITY || quality_cap < 1 || quality_cap > WFA_HIP_MAX_QUALITY)
    return WFA_HIP_EINVAL;
  for (int32_t v = 0; v < plen; ++v) if (quals[v] > WFA_HIP_MAX_QUALITY) return WFA_HIP_EINVAL;
  int64_t nv = 0, nh = 0;
  for (int64_t i = 0; i < ops_len; ++i) { const uint8_t c = ops[i]; nv += (c == 'M' || c == 'X' || c == 'D'); nh += (c == 'M' || c == 'X' || c == 'I'); }
  if (nv > plen || nh > tlen) return WFA_HIP_EINVAL;
  int64_t first = 0, last = -1;
  if (!aligned_core(ops, ops_len, &first, &last)) return WFA_HIP_OK;
  const auto capped = [&](int32_t x) { return std::min<int32_t>(quals[x], quality_cap); };
  int32_t v = 0, h = 0;
  for (int64_t i = 0; i <= last; ++i) {
    const uint8_t c = ops[i];
    const bool in = i >= first;
    int32_t* row = rows + (int64_t)WFA_HIP_PILEUP_COLS * h;
    int32_t* qrow = qrows + (int64_t)WFA_HIP_PILEUP_COLS * h;
    if (c == 'M' || c == 'X') {
      if (in && quals[v] >= min_base_quality) {
        const uint8_t l = pattern[v];
        const int col = l == 'A' ? 0 : l == 'C' ? 1 : l == 'G' ? 2 : l == 'T' ? 3 : 4;
        row[col] += 1; qrow[col] += capped(v);
        if (c == 'X') { row[7] += 1; qrow[7] += capped(v); }
      }
      ++v; ++h;
    } else if (c == 'I') {
      if (in) {
        // the read bases on either side of the text base it lacks; one outside the pattern is left out
        int32_t qq = -1;
        if (v - 1 >= 0 && v - 1 < plen) qq = capped(v - 1);
        if (v < plen) qq = qq < 0 ? capped(v) : std::min(qq, capped(v));
        row[5] += 1; qrow[5] += std::max(qq, 0);
      }
      ++h;
    } else if (c == 'D') {
      if (in && ops[i - 1] != 'D') { row[6] += 1; qrow[6] += capped(v); }   // (inside the core a D has an op in front of it)
      ++v;
    }
  }
  return WFA_HIP_OK;
}

// ---- left alignment: the rewrite of one pair's op string, stated in plain C (the kernel: wfa_leftalign.hpp, k_leftalign.hip) --------

extern "C" int wfa_hip_ops_left_align(uint8_t* ops, int64_t ops_len, const uint8_t* pattern, int32_t plen, const uint8_t* text, int32_t tlen,
                                      int64_t* stats) {
  if (ops_len < 0 || plen < 0 || tlen < 0 || (ops_len > 0 && !ops) || (plen > 0 && !pattern) || (tlen > 0 && !text)) return WFA_HIP_EINVAL;
  // an op string that does not consume exactly its pair is refused before anything is rewritten
  int64_t nv = 0, nh = 0;
  for (int64_t i = 0; i < ops_len; ++i) { const uint8_t c = ops[i]; nv += (c == 'M' || c == 'X' || c == 'D'); nh += (c == 'M' || c == 'X' || c == 'I'); }
  if (nv != plen || nh != tlen) return WFA_HIP_EINVAL;
  int64_t moved_runs = 0, merges = 0, first = 0, last = -1;
  if (aligned_core(ops, ops_len, &first, &last)) {
    int64_t v = 0, h = 0;   // the positions in front of op i
    for (int64_t i = 0; i < last;) {
      const uint8_t c = ops[i];
      if (i <= first || (c != 'I' && c != 'D')) { v += (c == 'M' || c == 'X' || c == 'D'); h += (c == 'M' || c == 'X' || c == 'I'); ++i; continue; }
      int64_t a = i, L = 0;
      while (ops[a + L] == c) ++L;   // (the core ends with an M)
      const int64_t end = a + L;     // the ops in front of `end` keep their letter counts: v and h there do not depend on the rewrite
      const uint8_t* S = (c == 'I') ? text : pattern;
      int64_t x = (c == 'I') ? h : v;
      bool moved = false;
      for (;;) {
        while (a - 1 > first && ops[a - 1] == 'M' && S[x - 1] == S[x + L - 1]) {
          ops[a - 1] = c; ops[a + L - 1] = 'M';
          --a; --x; moved = true;
        }
        if (!(moved && a - 1 > first && ops[a - 1] == c)) break;
        int64_t n = 0;               // the run in front has become a part of this one
        while (ops[a - 1 - n] == c) ++n;   // (the core begins with an M)
        a -= n; x -= n; L += n; ++merges;
      }
      moved_runs += moved;
      if (c == 'I') h += end - i; else v += end - i;
      i = end;
    }
  }
  if (stats) { stats[0] = moved_runs; stats[1] = merges; }
  return WFA_HIP_OK;
}

// ---- calls and sites: the two reductions of pileup rows against their reference bytes (the kernels: wfa_calls.hpp, k_calls.hip) ----

namespace {
int ref_col(uint8_t b) { return b == 'A' ? 0 : b == 'C' ? 1 : b == 'G' ? 2 : b == 'T' ? 3 : 4; }
int64_t depth_of(const int32_t* c) {
  int64_t d = 0;
  for (int x = 0; x < 6; ++x) d += c[x];
  return d;
}
}  // namespace

extern "C" int wfa_hip_calls_host(const int32_t* counts, const uint8_t* ref, int64_t len, int32_t min_depth, uint8_t* out) {
  if (len < 0 || min_depth < 1 || (len > 0 && (!counts || !ref || !out))) return WFA_HIP_EINVAL;
  for (int64_t g = 0; g < len; ++g) {
    const int32_t* c = counts + g * WFA_HIP_PILEUP_COLS;
    const int64_t depth = depth_of(c);
    if (depth < min_depth) { out[g] = 6; continue; }
    const int r = ref_col(ref[g]);
    int best = 0;
    for (int x = 1; x < 6; ++x) if (c[x] > c[best]) best = x;   // the smallest of the greatest
    if (c[r] == c[best]) best = r;
    out[g] = (uint8_t)(best | (2 * (int64_t)c[6] > depth ? 8 : 0));
  }
  return WFA_HIP_OK;
}

extern "C" int wfa_hip_sites_host(const int32_t* counts, const uint8_t* ref, int64_t len, int32_t seq, int64_t start, int32_t min_depth,
                                  int32_t min_permille, int64_t cap, int64_t* count, int32_t* rows) {
  if (len < 0 || min_depth < 1 || min_permille < 1 || min_permille > 1000 || cap < 0 || !count || (len > 0 && (!counts || !ref)) ||
      (cap > 0 && !rows))
    return WFA_HIP_EINVAL;
  int64_t n = 0;
  for (int64_t g = 0; g < len; ++g) {
    const int32_t* c = counts + g * WFA_HIP_PILEUP_COLS;
    const int64_t depth = depth_of(c);
    if (depth < min_depth) continue;
    const int r = ref_col(ref[g]);
    int alt = -1;
    for (int x = 0; x < 6; ++x) if (x != r && (alt < 0 || c[x] > c[alt])) alt = x;
    const int64_t A = c[alt], ins = c[6];
    const bool snv = A >= 1 && 1000 * A >= (int64_t)min_permille * depth;
    const bool has_ins = ins >= 1 && 1000 * ins >= (int64_t)min_permille * depth;
    if (!snv && !has_ins) continue;
    if (n < cap) {
      int32_t* row = rows + n * WFA_HIP_SITE_COLS;
      row[0] = seq; row[1] = (int32_t)(start + g); row[2] = r; row[3] = snv ? alt : -1; row[4] = (int32_t)depth;
      row[5] = c[r]; row[6] = snv ? c[alt] : 0; row[7] = c[6];
    }
    ++n;
  }
  *count = n;
  return WFA_HIP_OK;
}

// ---- genotyped sites: the sites under the strand filter, a diploid genotype per event (the kernels: wfa_calls.hpp, k_calls.hip) ----

namespace {
// GENOTYPE: the index of the smallest of L0, L1, L2 (the smaller index on a tie) and min(99, second smallest - smallest)
void genotype_of(int64_t R, int64_t A, int32_t err_q, int32_t* gt, int32_t* gq) {
  const int64_t L[3] = {(int64_t)err_q * A, 3 * (R + A), (int64_t)err_q * R};
  int best = 0;
  for (int k = 1; k < 3; ++k) if (L[k] < L[best]) best = k;
  const int64_t second = std::min(L[(best + 1) % 3], L[(best + 2) % 3]);
  *gt = best;
  *gq = (int32_t)std::min<int64_t>(99, second - L[best]);
}
}  // namespace

extern "C" int wfa_hip_genotypes_host(const int32_t* counts, const int32_t* counts_fwd, const uint8_t* ref, int64_t len, int32_t seq, int64_t start,
                                      int32_t min_depth, int32_t min_permille, int32_t err_q, int32_t min_alt_strand, int64_t cap, int64_t* count,
                                      int32_t* rows) {
  if (len < 0 || min_depth < 1 || min_permille < 1 || min_permille > 1000 || err_q < 1 || err_q > 60 || min_alt_strand < 0 ||
      (min_alt_strand > 0 && !counts_fwd) || cap < 0 || !count || (len > 0 && (!counts || !ref)) || (cap > 0 && !rows))
    return WFA_HIP_EINVAL;
  int64_t n = 0;
  for (int64_t g = 0; g < len; ++g) {
    const int32_t* c = counts + g * WFA_HIP_PILEUP_COLS;
    const int32_t* f = counts_fwd ? counts_fwd + g * WFA_HIP_PILEUP_COLS : nullptr;
    const int64_t depth = depth_of(c);
    if (depth < min_depth) continue;
    const int r = ref_col(ref[g]);
    int alt = -1;
    for (int x = 0; x < 6; ++x) if (x != r && (alt < 0 || c[x] > c[alt])) alt = x;
    const int64_t A = c[alt], ins = c[6];
    bool snv = A >= 1 && 1000 * A >= (int64_t)min_permille * depth;
    bool has_ins = ins >= 1 && 1000 * ins >= (int64_t)min_permille * depth;
    if (min_alt_strand > 0) {
      snv = snv && f[alt] >= min_alt_strand && A - f[alt] >= min_alt_strand;
      has_ins = has_ins && f[6] >= min_alt_strand && ins - f[6] >= min_alt_strand;
    }
    if (!snv && !has_ins) continue;
    if (n < cap) {
      int32_t* row = rows + n * WFA_HIP_GENOTYPE_COLS;
      row[0] = seq; row[1] = (int32_t)(start + g); row[2] = r; row[3] = snv ? alt : -1; row[4] = (int32_t)depth;
      row[5] = c[r]; row[6] = snv ? c[alt] : 0; row[7] = c[6];
      row[8] = row[9] = row[10] = row[11] = -1;
      if (snv) genotype_of(c[r], A, err_q, &row[8], &row[9]);
      if (has_ins) genotype_of(std::max<int64_t>(0, depth - ins), ins, err_q, &row[10], &row[11]);
      row[12] = row[13] = row[14] = row[15] = -1;
      if (f) { row[12] = (int32_t)depth_of(f); row[13] = f[r]; row[14] = snv ? f[alt] : 0; row[15] = f[6]; }
    }
    ++n;
  }
  *count = n;
  return WFA_HIP_OK;
}

namespace {
// GENOTYPE over three given costs
void genotype_of_costs(int64_t L0, int64_t L1, int64_t L2, int32_t* gt, int32_t* gq) {
  const int64_t L[3] = {L0, L1, L2};
  int best = 0;
  for (int k = 1; k < 3; ++k) if (L[k] < L[best]) best = k;
  const int64_t second = std::min(L[(best + 1) % 3], L[(best + 2) % 3]);
  *gt = best;
  *gq = (int32_t)std::min<int64_t>(99, second - L[best]);
}
}  // namespace

// the genotyped sites with the costs of "base qualities": the selection, the filter and the rows of wfa_hip_genotypes_host
extern "C" int wfa_hip_genotypes_quals_host(const int32_t* counts, const int32_t* qsums, const int32_t* counts_fwd, const uint8_t* ref, int64_t len,
                                            int32_t seq, int64_t start, int32_t min_depth, int32_t min_permille, int32_t err_q,
                                            int32_t min_alt_strand, int64_t cap, int64_t* count, int32_t* rows) {
  if (len < 0 || min_depth < 1 || min_permille < 1 || min_permille > 1000 || err_q < 1 || err_q > 60 || min_alt_strand < 0 ||
      (min_alt_strand > 0 && !counts_fwd) || cap < 0 || !count || (len > 0 && (!counts || !qsums || !ref)) || (cap > 0 && !rows))
    return WFA_HIP_EINVAL;
  int64_t n = 0;
  for (int64_t g = 0; g < len; ++g) {
    const int32_t* c = counts + g * WFA_HIP_PILEUP_COLS;
    const int32_t* qs = qsums + g * WFA_HIP_PILEUP_COLS;
    const int32_t* f = counts_fwd ? counts_fwd + g * WFA_HIP_PILEUP_COLS : nullptr;
    const int64_t depth = depth_of(c);
    if (depth < min_depth) continue;
    const int r = ref_col(ref[g]);
    int alt = -1;
    for (int x = 0; x < 6; ++x) if (x != r && (alt < 0 || c[x] > c[alt])) alt = x;
    const int64_t A = c[alt], ins = c[6];
    bool snv = A >= 1 && 1000 * A >= (int64_t)min_permille * depth;
    bool has_ins = ins >= 1 && 1000 * ins >= (int64_t)min_permille * depth;
    if (min_alt_strand > 0) {
      snv = snv && f[alt] >= min_alt_strand && A - f[alt] >= min_alt_strand;
      has_ins = has_ins && f[6] >= min_alt_strand && ins - f[6] >= min_alt_strand;
    }
    if (!snv && !has_ins) continue;
    if (n < cap) {
      int32_t* row = rows + n * WFA_HIP_GENOTYPE_COLS;
      row[0] = seq; row[1] = (int32_t)(start + g); row[2] = r; row[3] = snv ? alt : -1; row[4] = (int32_t)depth;
      row[5] = c[r]; row[6] = snv ? c[alt] : 0; row[7] = c[6];
      row[8] = row[9] = row[10] = row[11] = -1;
      if (snv) genotype_of_costs(qs[alt], 3 * ((int64_t)c[r] + A), qs[r], &row[8], &row[9]);
      if (has_ins) {
        const int64_t R = std::max<int64_t>(0, depth - ins);
        genotype_of_costs(qs[6], 3 * (R + ins), (int64_t)err_q * R, &row[10], &row[11]);
      }
      row[12] = row[13] = row[14] = row[15] = -1;
      if (f) { row[12] = (int32_t)depth_of(f); row[13] = f[r]; row[14] = snv ? f[alt] : 0; row[15] = f[6]; }
    }
    ++n;
  }
  *count = n;
  return WFA_HIP_OK;
}

// ---- insertions: a pair's records, and the allele rule over rows and records (the kernels: wfa_insertions.hpp, k_pileup.hip, k_insertions.hip) ----

extern "C" int wfa_hip_ops_insertions(const uint8_t* ops, int64_t ops_len, const uint8_t* pattern, int32_t plen, int32_t tlen, int64_t cap,
                                      int64_t* count, int32_t* recs, int64_t cols_cap, int64_t* cols_count, uint8_t* cols) {
  if (ops_len < 0 || plen < 0 || tlen < 0 || (ops_len > 0 && !ops) || (plen > 0 && !pattern) || cap < 0 || cols_cap < 0 || !count || !cols_count ||
      (cap > 0 && !recs) || (cols_cap > 0 && !cols))
    return WFA_HIP_EINVAL;
  // an op string that outruns its pair is refused before anything is written (as wfa_hip_ops_pileup refuses it)
  int64_t nv = 0, nh = 0;
  for (int64_t i = 0; i < ops_len; ++i) { const uint8_t c = ops[i]; nv += (c == 'M' || c == 'X' || c == 'D'); nh += (c == 'M' || c == 'X' || c == 'I'); }
  if (nv > plen || nh > tlen) return WFA_HIP_EINVAL;
  int64_t nrec = 0, ncols = 0, first = 0, last = -1;
  if (aligned_core(ops, ops_len, &first, &last)) {
    int32_t v = 0, h = 0;
    for (int64_t i = 0; i <= last;) {
      const uint8_t c = ops[i];
      if (c != 'D') { v += (c == 'M' || c == 'X'); h += (c == 'M' || c == 'X' || c == 'I'); ++i; continue; }
      int64_t e = i;
      while (ops[e] == 'D') ++e;   // (the core ends with an M)
      const int32_t n = (int32_t)(e - i);
      if (i > first) {             // a run of the core: one record
        if (nrec < cap) {
          int32_t* r = recs + 3 * nrec;
          r[0] = h; r[1] = n; r[2] = (int32_t)ncols;
          if (ncols + n <= cols_cap)
            for (int32_t k = 0; k < n; ++k) cols[ncols + k] = (uint8_t)ref_col(pattern[v + k]);
        }
        ++nrec; ncols += n;
      }
      v += n; i = e;
    }
  }
  *count = nrec; *cols_count = ncols;
  return WFA_HIP_OK;
}

extern "C" int wfa_hip_insertions_host(const int32_t* counts, int64_t len, int32_t seq, int64_t start, int32_t min_depth, int32_t min_permille,
                                       int64_t nrec, const int64_t* rec_row, const int32_t* rec_n, const int64_t* rec_off, const uint8_t* cols,
                                       int64_t ncols, int64_t cap, int64_t* count, int32_t* rows, int64_t bases_cap, int64_t* bases_count,
                                       uint8_t* bases) {
  if (len < 0 || min_depth < 1 || min_permille < 0 || min_permille > 1000 || nrec < 0 || ncols < 0 || cap < 0 || bases_cap < 0 || !count ||
      !bases_count || (len > 0 && !counts) || (nrec > 0 && (!rec_row || !rec_n || !rec_off)) || (ncols > 0 && !cols) || (cap > 0 && !rows) ||
      (bases_cap > 0 && !bases))
    return WFA_HIP_EINVAL;
  for (int64_t r = 0; r < nrec; ++r)
    if (rec_n[r] < 0 || rec_off[r] < 0 || rec_off[r] + rec_n[r] > ncols) return WFA_HIP_EINVAL;
  const char* env = getenv("WFA_HIP_INS_MAX_READS");
  const int64_t max_reads = std::max<int64_t>(1, env && *env ? atoll(env) : WFA_HIP_INS_MAX_READS);
  // the records of every row, in the order they were given (the rule does not depend on it)
  std::vector<std::vector<int64_t>> at((size_t)len);
  for (int64_t r = 0; r < nrec; ++r)
    if (rec_row[r] >= 0 && rec_row[r] < len) at[(size_t)rec_row[r]].push_back(r);
  int64_t n = 0, nb = 0;
  typedef std::pair<int32_t, std::vector<uint8_t>> Allele;   // (n, letters): its natural order is the rule's tie order
  for (int64_t g = 0; g < len; ++g) {
    const int32_t* c = counts + g * WFA_HIP_PILEUP_COLS;
    const int64_t depth = depth_of(c), c6 = c[6];
    if (depth < min_depth) continue;
    if (min_permille > 0 ? !(c6 >= 1 && 1000 * c6 >= (int64_t)min_permille * depth) : !(2 * c6 > depth)) continue;
    const bool overflow = c6 > max_reads;
    std::map<Allele, int64_t> alleles;
    if (!overflow)
      for (int64_t r : at[(size_t)g]) alleles[Allele(rec_n[r], std::vector<uint8_t>(cols + rec_off[r], cols + rec_off[r] + rec_n[r]))] += 1;
    const Allele* best = nullptr;
    int64_t best_count = 0;
    for (const auto& kv : alleles)   // ascending (n, letters): the first of the greatest count
      if (kv.second > best_count) { best = &kv.first; best_count = kv.second; }
    const int32_t alen = best ? best->first : 0;
    if (n < cap) {
      int32_t* row = rows + n * WFA_HIP_INSERTION_COLS;
      row[0] = seq; row[1] = (int32_t)(start + g); row[2] = (int32_t)depth; row[3] = c[6];
      row[4] = (int32_t)best_count; row[5] = alen; row[6] = (int32_t)alleles.size(); row[7] = overflow ? 1 : 0;
      if (nb + alen <= bases_cap)
        for (int32_t k = 0; k < alen; ++k) bases[nb + k] = (uint8_t)"ACGTN"[best->second[(size_t)k] > 4 ? 4 : best->second[(size_t)k]];
    }
    ++n; nb += alen;
  }
  *count = n; *bases_count = nb;
  return WFA_HIP_OK;
}

// ---- deletions: a pair's records, and the allele rule over rows, starts and records (the kernels: wfa_deletions.hpp, k_deletions.hip) ----

extern "C" int wfa_hip_ops_deletions(const uint8_t* ops, int64_t ops_len, int32_t plen, int32_t tlen, int64_t cap, int64_t* count, int32_t* recs) {
  if (ops_len < 0 || plen < 0 || tlen < 0 || (ops_len > 0 && !ops) || cap < 0 || !count || (cap > 0 && !recs)) return WFA_HIP_EINVAL;
  // an op string that outruns its pair is refused before anything is written (as wfa_hip_ops_pileup refuses it)
  int64_t nv = 0, nh = 0;
  for (int64_t i = 0; i < ops_len; ++i) { const uint8_t c = ops[i]; nv += (c == 'M' || c == 'X' || c == 'D'); nh += (c == 'M' || c == 'X' || c == 'I'); }
  if (nv > plen || nh > tlen) return WFA_HIP_EINVAL;
  int64_t nrec = 0, first = 0, last = -1;
  if (aligned_core(ops, ops_len, &first, &last)) {
    int32_t h = 0;
    for (int64_t i = 0; i <= last;) {
      const uint8_t c = ops[i];
      if (c != 'I') { h += (c == 'M' || c == 'X'); ++i; continue; }
      int64_t e = i;
      while (ops[e] == 'I') ++e;   // (the core ends with an M)
      const int32_t n = (int32_t)(e - i);
      if (i > first) {             // a run of the core: one record, whatever stands beside it (a D run neither breaks nor joins it)
        if (nrec < cap) { recs[2 * nrec] = h; recs[2 * nrec + 1] = n; }
        ++nrec;
      }
      h += n; i = e;
    }
  }
  *count = nrec;
  return WFA_HIP_OK;
}

extern "C" int wfa_hip_deletions_host(const int32_t* counts, const int32_t* starts, int64_t len, int32_t seq, int64_t start, int32_t min_depth,
                                      int32_t min_permille, int64_t nrec, const int64_t* rec_row, const int32_t* rec_n, int64_t cap,
                                      int64_t* count, int32_t* rows) {
  if (len < 0 || min_depth < 1 || min_permille < 0 || min_permille > 1000 || nrec < 0 || cap < 0 || !count || (len > 0 && (!counts || !starts)) ||
      (nrec > 0 && (!rec_row || !rec_n)) || (cap > 0 && !rows))
    return WFA_HIP_EINVAL;
  for (int64_t r = 0; r < nrec; ++r)
    if (rec_n[r] < 1) return WFA_HIP_EINVAL;
  const char* env = getenv("WFA_HIP_DEL_MAX_READS");
  const int64_t max_reads = std::max<int64_t>(1, env && *env ? atoll(env) : WFA_HIP_DEL_MAX_READS);
  // the lengths of the records that start at every row, in the order they were given (the rule does not depend on it)
  std::vector<std::vector<int32_t>> at((size_t)len);
  for (int64_t r = 0; r < nrec; ++r)
    if (rec_row[r] >= 0 && rec_row[r] < len) at[(size_t)rec_row[r]].push_back(rec_n[r]);
  int64_t n = 0;
  for (int64_t g = 0; g < len; ++g) {
    const int32_t* c = counts + g * WFA_HIP_PILEUP_COLS;
    const int64_t depth = depth_of(c), S = starts[g];
    if (depth < min_depth) continue;
    if (min_permille > 0 ? !(S >= 1 && 1000 * S >= (int64_t)min_permille * depth) : !(2 * S > depth)) continue;
    const bool overflow = S > max_reads;
    std::map<int32_t, int64_t> alleles;
    if (!overflow)
      for (int32_t m : at[(size_t)g]) alleles[m] += 1;
    int32_t best = 0;
    int64_t best_count = 0;
    for (const auto& kv : alleles)   // ascending n: the first of the greatest count
      if (kv.second > best_count) { best = kv.first; best_count = kv.second; }
    if (n < cap) {
      int32_t* row = rows + n * WFA_HIP_DELETION_COLS;
      row[0] = seq; row[1] = (int32_t)(start + g); row[2] = (int32_t)depth; row[3] = starts[g];
      row[4] = (int32_t)best_count; row[5] = best; row[6] = (int32_t)alleles.size(); row[7] = overflow ? 1 : 0;
    }
    ++n;
  }
  *count = n;
  return WFA_HIP_OK;
}
