// k_pileup.hip — the pileup reduction (wfa_pileup.hpp: PileupArgs; wfa_hip_pileup_add in wfa_hip.hip).
// One wave per pair, grid-stride.  Every store is an int32 atomicAdd into the table; a lane adds only for an op of the aligned core
// whose text position lies inside the pair's text window, and the host has checked that the window lies inside its sequence, so an op
// string that disagreed with its pair's lengths could lose counts but never leave the table.
#include <algorithm>
#include "wfa_pileup.hpp"

namespace wfa {

__global__ void __launch_bounds__(256) wfa_pileup_kernel(PileupArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const unsigned long long lower = (1ull << lane) - 1ull;
  for (int64_t q = wave; q < a.npairs; q += nwaves) {
    if (a.status[q] != 0 || (a.keep && a.keep[q] == 0)) continue;
    const int len = a.cigar_len[q];
    if (len <= 0) continue;
    const uint8_t* p = a.ops + a.cigar_begin[q];
    // the aligned core: first M .. last M
    int first = -1, last = -1;
    for (int base = 0; base < len && first < 0; base += 64) {
      const int i = base + lane;
      const unsigned long long mm = __ballot(i < len && p[i] == 'M');
      if (mm) first = base + __builtin_ctzll(mm);
    }
    if (first < 0) continue;
    for (int top = len; top > 0 && last < 0; top -= 64) {
      const int i = top - 64 + lane;
      const unsigned long long mm = __ballot(i >= 0 && p[i] == 'M');
      if (mm) last = top - 64 + (63 - __builtin_clzll(mm));
    }
    const WfaPairMeta m = a.meta[q];
    const int jq = a.j[q];
    const int64_t ts = a.t_start ? a.t_start[q] : 0;
    // (checked on the host; here so that nothing a caller passes can move a store out of the table)
    if (jq < 0 || jq >= a.nseq || ts < 0 || ts + m.tlen > a.seq_len[jq]) continue;
    int32_t* row0 = a.table + a.seq_off[jq] + ts;
    const bool on_bytes = a.bytes != nullptr && a.flags[q] != 0;
    const uint8_t* pb = on_bytes ? a.bytes + a.pboff[q] : nullptr;
    const uint32_t* pw = a.words + m.p_woff;
    int vbase = 0, hbase = 0;
    unsigned long long carry_d = 0;
    for (int base = 0; base <= last; base += 64) {
      const int i = base + lane;
      const uint32_t c = (i < len) ? p[i] : 0u;
      const unsigned long long bm = __ballot(c == 'M'), bx = __ballot(c == 'X'), bi = __ballot(c == 'I'), bd = __ballot(c == 'D');
      const unsigned long long bv = bm | bx | bd, bh = bm | bx | bi;
      const int v = vbase + __builtin_popcountll(bv & lower);
      const int h = hbase + __builtin_popcountll(bh & lower);
      const bool d_start = ((bd & ~((bd << 1) | carry_d)) >> lane) & 1ull;
      vbase += __builtin_popcountll(bv); hbase += __builtin_popcountll(bh); carry_d = bd >> 63;
      if (i < first || i > last || h >= m.tlen) continue;
      int32_t* row = row0 + h;
      if (c == 'M' || c == 'X') {
        if (v < m.plen) {
          const int col = on_bytes ? wfa_pileup_letter_col(pb[v]) : wfa_pileup_code_col((pw[v >> 4] >> (2 * (v & 15))) & 3u);
          atomicAdd(row + (int64_t)col * a.total, 1);
          if (c == 'X') atomicAdd(row + (int64_t)WFA_PILEUP_MISMATCH * a.total, 1);
        }
      } else if (c == 'I') {
        atomicAdd(row + (int64_t)WFA_PILEUP_DEL * a.total, 1);
      } else if (d_start) {
        atomicAdd(row + (int64_t)WFA_PILEUP_INS * a.total, 1);
      }
    }
  }
}

int launch_pileup(const PileupArgs& a, int cu_count, hipStream_t stream) {
  if (a.npairs <= 0) return 0;
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((a.npairs + 3) / 4, (int64_t)cu_count * 16));
  hipLaunchKernelGGL(wfa_pileup_kernel, dim3(grid), dim3(256), 0, stream, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace wfa
