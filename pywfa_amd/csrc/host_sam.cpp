// host_sam.cpp — host only, needs no GPU: the SAM fields of ONE pair from its op string and its text letters, the rule of
// include/wfa_hip.h ("SAM fields") stated in plain C++ (wfa_hip_ops_sam).  The kernels of k_sam.hip are held to this statement.
#include <stdint.h>
#include <string>
#include "wfa_hip.h"

namespace {

inline bool pattern_op(uint8_t c) { return c == 'M' || c == 'X' || c == 'D'; }
inline bool text_op(uint8_t c) { return c == 'M' || c == 'X' || c == 'I'; }
// the SAM letter of an op: the library's D inserts into the read, its I deletes from it
inline char sam_letter(uint8_t c, bool eqx) { return c == 'M' ? (eqx ? '=' : 'M') : c == 'X' ? (eqx ? 'X' : 'M') : c == 'D' ? 'I' : 'D'; }

}  // namespace

extern "C" int wfa_hip_ops_sam(const uint8_t* ops, int64_t ops_len, const uint8_t* text, int32_t tlen, int32_t plen, int flags,
                               int32_t* row8, uint8_t* cigar, int64_t cigar_cap, uint8_t* md, int64_t md_cap) {
  if (ops_len < 0 || tlen < 0 || plen < 0 || cigar_cap < 0 || md_cap < 0 || !row8) return WFA_HIP_EINVAL;
  if ((ops_len > 0 && !ops) || (tlen > 0 && !text) || (cigar_cap > 0 && !cigar) || (md_cap > 0 && !md)) return WFA_HIP_EINVAL;
  if (flags & ~(WFA_HIP_SAM_EQX | WFA_HIP_SAM_CORE)) return WFA_HIP_EINVAL;
  const bool eqx = flags & WFA_HIP_SAM_EQX, core = flags & WFA_HIP_SAM_CORE;
  int64_t v = 0, h = 0, f = -1, l = -1;
  for (int64_t k = 0; k < ops_len; ++k) {
    const uint8_t c = ops[k];
    if (c != 'M' && c != 'X' && c != 'I' && c != 'D') return WFA_HIP_EINVAL;
    v += pattern_op(c); h += text_op(c);
    if (c == 'M' || (c == 'X' && !core)) { if (f < 0) f = k; l = k; }
  }
  if (v != plen || h != tlen) return WFA_HIP_EINVAL;
  int32_t row[WFA_HIP_SAM_COLS] = {-1, 0, 0, 0, 0, 0, 0, 0};
  std::string cg, m;
  if (f >= 0) {
    int32_t pos = 0, ref_len = 0, clip_left = 0, clip_right = 0, nm = 0, query_len = 0;
    for (int64_t k = 0; k < f; ++k) { pos += ops[k] == 'X' || ops[k] == 'I'; clip_left += ops[k] == 'X' || ops[k] == 'D'; }
    for (int64_t k = l + 1; k < ops_len; ++k) clip_right += ops[k] == 'X' || ops[k] == 'D';
    if (clip_left) cg += std::to_string(clip_left) + "S";
    int64_t t = pos;      // the text offset of op k
    int32_t run = 0;      // M ops since the last MD event
    for (int64_t k = f; k <= l;) {
      const char s = sam_letter(ops[k], eqx);
      int64_t e = k;
      while (e <= l && sam_letter(ops[e], eqx) == s) ++e;
      cg += std::to_string(e - k) + s;
      for (; k < e; ++k) {
        const uint8_t c = ops[k];
        ref_len += text_op(c); query_len += pattern_op(c); nm += c != 'M';
        if (c == 'M') ++run;
        else if (c == 'X') { m += std::to_string(run); m += (char)text[t]; run = 0; }
        else if (c == 'I') {
          if (ops[k - 1] != 'I') { m += std::to_string(run); m += '^'; run = 0; }
          m += (char)text[t];
        }
        t += text_op(c);
      }
    }
    m += std::to_string(run);
    if (clip_right) cg += std::to_string(clip_right) + "S";
    const int32_t mapped[WFA_HIP_SAM_COLS] = {pos, ref_len, clip_left, clip_right, nm, (int32_t)cg.size(), (int32_t)m.size(), query_len};
    for (int k = 0; k < WFA_HIP_SAM_COLS; ++k) row[k] = mapped[k];
  }
  if ((int64_t)cg.size() > cigar_cap || (int64_t)m.size() > md_cap) return WFA_HIP_EINVAL;
  for (int k = 0; k < WFA_HIP_SAM_COLS; ++k) row8[k] = row[k];
  for (size_t k = 0; k < cg.size(); ++k) cigar[k] = (uint8_t)cg[k];
  for (size_t k = 0; k < m.size(); ++k) md[k] = (uint8_t)m[k];
  return WFA_HIP_OK;
}
