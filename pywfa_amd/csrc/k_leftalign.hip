// k_leftalign.hip — left alignment of a batch's op strings in place (wfa_leftalign.hpp: LeftAlignArgs; wfa_hip_batch_left_align in
// api_pileup.hip).  One wave per pair, grid-stride; every quantity that steers the walk comes out of a ballot, so it is wave-uniform.
//
// ORDERING.  The string stays in global memory (an op string is as long as plen + tlen: tens of thousands of bytes for long reads, too
// much to stage in LDS for every wave), and a later step of the same wave reads ops that other lanes of the wave have just rewritten:
// the M ops a run left behind are what the next run moves over, and the merge test reads the op in front of the moved run.  Every
// rewrite is therefore followed by a workgroup-scope fence before any lane loads an op again: it keeps the compiler from moving or
// reusing loads across the stores and makes the wave wait (s_waitcnt vmcnt(0)) until its stores have left it; the loads behind it go
// down the same vector-memory path of the same CU and see them.  No other wave touches the pair.  Only pairs that move a run pay it.
//
// BOUNDS.  Every op index that is loaded or stored lies in (first, last] of the pair's own [0, cigar_len): the candidate test asks
// a - 1 - k > first before its load, the run scans stop in front of `last`, and a run [a, a + L) keeps a + L <= last through shifts
// and merges.  Every letter index is checked against 0 and plen / tlen before its load.  An op string that disagreed with its pair's
// lengths could stop a run early, never read or write outside its pair.  A byte has one writer per rewrite (the two stretches that
// change are disjoint).
#include <algorithm>
#include "wfa_leftalign.hpp"

namespace wfa {

// the letters of one sequence of a pair: its bytes (a flagged pair) or its 2-bit codes
struct LeftAlignSeq { const uint8_t* b; const uint32_t* w; int n; };
__device__ __forceinline__ uint32_t left_align_letter(const LeftAlignSeq& s, int i) {
  return s.b ? (uint32_t)s.b[i] : (s.w[i >> 4] >> (2 * (i & 15))) & 3u;
}

__global__ void __launch_bounds__(256) wfa_left_align_kernel(LeftAlignArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  unsigned long long moved_runs = 0, merges = 0;   // of this wave (wave-uniform)
  for (int64_t q = wave; q < a.npairs; q += nwaves) {
    if (a.status[q] != 0) continue;
    const int len = a.cigar_len[q];
    if (len < 3) continue;
    uint8_t* p = a.ops + a.cigar_begin[q];
    // the aligned core first M .. last M, and the first gap op behind the first M
    int first = -1, last = -1, gap = -1;
    for (int base = 0; base < len; base += 64) {
      const int i = base + lane;
      const uint32_t c = (i < len) ? p[i] : 0u;
      const unsigned long long bm = __ballot(c == 'M'), bg = __ballot(c == 'I' || c == 'D');
      if (bm) {
        if (first < 0) first = base + __builtin_ctzll(bm);
        last = base + 63 - __builtin_clzll(bm);
      }
      if (gap < 0 && first >= 0 && bg) {
        const int skip = first - base + 1;   // the lanes of this round up to the first M
        const unsigned long long g = skip <= 0 ? bg : skip >= 64 ? 0ull : bg & (~0ull << skip);
        if (g) gap = base + __builtin_ctzll(g);
      }
    }
    if (first < 0 || gap < 0 || gap >= last) continue;   // no gap run inside the core: no store
    const WfaPairMeta m = a.meta[q];
    const bool on_bytes = a.bytes != nullptr && a.pboff != nullptr && a.tboff != nullptr && a.flags[q] != 0;
    const LeftAlignSeq P{on_bytes ? a.bytes + a.pboff[q] : nullptr, a.words + m.p_woff, m.plen};
    const LeftAlignSeq T{on_bytes ? a.bytes + a.tboff[q] : nullptr, a.words + m.t_woff, m.tlen};
    int pos = 0, v = 0, h = 0;   // v, h: the pattern and text positions in front of op `pos`
    while (pos < last) {
      const int i = pos + lane;
      const uint32_t c = (i < len) ? p[i] : 0u;
      const unsigned long long bm = __ballot(c == 'M'), bx = __ballot(c == 'X'), bi = __ballot(c == 'I'), bd = __ballot(c == 'D');
      const unsigned long long bv = bm | bx | bd, bh = bm | bx | bi;
      const unsigned long long cand = __ballot((c == 'I' || c == 'D') && i > first && i < last);
      if (!cand) {
        v += __builtin_popcountll(bv); h += __builtin_popcountll(bh); pos += 64;
        continue;
      }
      const int k = __builtin_ctzll(cand);
      const unsigned long long below = (1ull << k) - 1ull;
      v += __builtin_popcountll(bv & below); h += __builtin_popcountll(bh & below);
      const int a0 = pos + k;
      const bool is_i = (bi >> k) & 1ull;
      const uint32_t kind = is_i ? 'I' : 'D';
      int L0 = 0;   // the run [a0, a0 + L0): it ends in front of the core's last M
      for (;;) {
        const int idx = a0 + L0 + lane;
        const unsigned long long stop = ~__ballot(idx < last && p[idx] == kind);
        if (stop) { L0 += __builtin_ctzll(stop); break; }
        L0 += 64;
      }
      const LeftAlignSeq S = is_i ? T : P;
      int at = a0, L = L0, x = is_i ? h : v;
      bool moved = false;
      for (;;) {
        int d = 0;   // how far the run moves: 64 candidates a round
        for (;;) {
          const int idx = at - 1 - d - lane, sx = x - 1 - d - lane, sy = sx + L;
          const bool ok = idx > first && sx >= 0 && sy < S.n && p[idx] == 'M' && left_align_letter(S, sx) == left_align_letter(S, sy);
          const unsigned long long stop = ~__ballot(ok);
          if (stop) { d += __builtin_ctzll(stop); break; }
          d += 64;
        }
        if (d > 0) {
          // the run becomes [at - d, at - d + L): min(d, L) ops change at either end of [at - d, at + L), every other op keeps its letter
          const int n = min(d, L);
          for (int t = lane; t < n; t += 64) { p[at - d + t] = (uint8_t)kind; p[at + L - 1 - t] = (uint8_t)'M'; }
          __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");   // (ORDERING above)
          at -= d; x -= d; moved = true;
        }
        if (!moved || at - 1 <= first) break;
        if ((uint32_t)__builtin_amdgcn_readfirstlane((int)p[at - 1]) != kind) break;
        int n = 0;   // the run in front is of the same kind: one run with it from here on
        for (;;) {
          const int idx = at - 1 - n - lane;
          const unsigned long long stop = ~__ballot(idx > first && p[idx] == kind);
          if (stop) { n += __builtin_ctzll(stop); break; }
          n += 64;
        }
        at -= n; x -= n; L += n; ++merges;
      }
      moved_runs += moved ? 1u : 0u;
      if (is_i) h += L0; else v += L0;   // (the ops in front of the run's old end keep their letter counts)
      pos = a0 + L0;
    }
  }
  if (lane == 0) {
    if (moved_runs) atomicAdd(a.stats, moved_runs);
    if (merges) atomicAdd(a.stats + 1, merges);
  }
}

int launch_left_align(const LeftAlignArgs& a, int cu_count, hipStream_t stream) {
  if (a.npairs <= 0) return 0;
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((a.npairs + 3) / 4, (int64_t)cu_count * 16));
  hipLaunchKernelGGL(wfa_left_align_kernel, dim3(grid), dim3(256), 0, stream, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace wfa
