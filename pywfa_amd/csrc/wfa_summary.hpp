// wfa_summary.hpp — device-side result surface, per pair (wfa_hip_batch_summary): what identity / NM filters and clipping decisions
// read off an alignment, reduced from the op strings where they lie.  Per pair WFA_HIP_SUMMARY_COLS int32: the numbers of M, X, I and
// D ops, the numbers of maximal I and D runs, and the `locations` of wfa_rle.hpp (pattern_start, pattern_end, text_start, text_end:
// the ops before the first and behind the last M stripped; all zero for an empty pair or an empty op string).
// One wave per pair (grid-stride), 64 ops per round: every count is a popcount of a wave ballot, a run start is an op whose lower
// neighbour (the lane below, or the last op of the round before) is another letter, and the flanks fall out of the same ballots — the
// ops in front of the first M, and those behind the last M seen so far.  One pass over the op bytes, no atomics; lanes 0 .. 9 store
// the row.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wfa_common.hpp"

namespace wfa {

#define WFA_SUMMARY_COLS 10

// What one wave gathers from one op string.  The record kernel of the placer (k_place.hip) takes the same walk for head_t and tail_t
// alone, so that its text interval is columns 8 and 9 of the summary by construction.
struct SummaryScan {
  int nm, nx, ni, nd, ri, rd;
  int head_p, head_t, tail_p, tail_t;   // pattern / text bases consumed in front of the first M, behind the last M
};

// The walk: all 64 lanes of the wave call it with the same p and len; every lane returns the same values.
__device__ inline SummaryScan summary_scan(const uint8_t* __restrict__ p, int len, int lane) {
  int nm = 0, nx = 0, ni = 0, nd = 0, ri = 0, rd = 0;
  int head_p = 0, head_t = 0, tail_p = 0, tail_t = 0;
  bool found = false;
  unsigned long long carry_i = 0, carry_d = 0;           // the last op of the round before was an I / a D
  for (int base = 0; base < len; base += 64) {
    const int i = base + lane;
    const uint32_t c = (i < len) ? p[i] : 0u;
    const unsigned long long bm = __ballot(c == 'M'), bx = __ballot(c == 'X'), bi = __ballot(c == 'I'), bd = __ballot(c == 'D');
    nm += __builtin_popcountll(bm); nx += __builtin_popcountll(bx);
    ni += __builtin_popcountll(bi); nd += __builtin_popcountll(bd);
    ri += __builtin_popcountll(bi & ~((bi << 1) | carry_i));
    rd += __builtin_popcountll(bd & ~((bd << 1) | carry_d));
    carry_i = bi >> 63; carry_d = bd >> 63;
    const unsigned long long bp = bd | bx, bt = bi | bx;
    if (bm) {
      if (!found) {
        const unsigned long long below = (1ull << __builtin_ctzll(bm)) - 1ull;
        head_p += __builtin_popcountll(bp & below); head_t += __builtin_popcountll(bt & below);
        found = true;
      }
      const unsigned long long above = ~((2ull << (63 - __builtin_clzll(bm))) - 1ull);
      tail_p = __builtin_popcountll(bp & above); tail_t = __builtin_popcountll(bt & above);
    } else {
      if (!found) { head_p += __builtin_popcountll(bp); head_t += __builtin_popcountll(bt); }
      tail_p += __builtin_popcountll(bp); tail_t += __builtin_popcountll(bt);
    }
  }
  return SummaryScan{nm, nx, ni, nd, ri, rd, head_p, head_t, tail_p, tail_t};
}

#ifndef WFA_SUMMARY_SCAN_ONLY   // (a second translation unit takes the walk without defining the kernel again)
__global__ void __launch_bounds__(256)
wfa_summary_kernel(const uint8_t* __restrict__ ops, const int64_t* __restrict__ cigar_begin, const int32_t* __restrict__ cigar_len,
                   const WfaPairMeta* __restrict__ meta, int64_t n, int32_t* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t pair = wave; pair < n; pair += nwaves) {
    const int len = cigar_len[pair];
    const int plen = meta[pair].plen, tlen = meta[pair].tlen;
    const SummaryScan s = summary_scan(ops + cigar_begin[pair], len, lane);
    const bool zero = (len == 0) || plen == 0 || tlen == 0;
    int v = 0;
    switch (lane) {
      case 0: v = s.nm; break; case 1: v = s.nx; break; case 2: v = s.ni; break; case 3: v = s.nd; break;
      case 4: v = s.ri; break; case 5: v = s.rd; break;
      case 6: v = zero ? 0 : s.head_p; break; case 7: v = zero ? 0 : plen - s.tail_p; break;
      case 8: v = zero ? 0 : s.head_t; break; case 9: v = zero ? 0 : tlen - s.tail_t; break;
      default: break;
    }
    if (lane < WFA_SUMMARY_COLS) out[WFA_SUMMARY_COLS * pair + lane] = v;
  }
}
#endif

}  // namespace wfa
