// k_pairs.hip — the generator of an indexed batch (wfa_cross.hpp: PairsGenArgs, filled by IndexedPairs::generate for batch_build_list in wfa_hip.hip).
// A workgroup takes WFA_PAIRS_CHUNK listed pairs per round, in two steps:
//  1. thread t = pair t of the chunk: its indices, the sets' tables (lengths, word / byte offsets, flags), the words its slot needs; an
//     exclusive prefix sum of those over the chunk (wave shuffles, the four wave totals through LDS) on top of the chunk's base gives
//     every slot's place; the thread stores the pair's metadata (consecutive threads, consecutive 16-byte records);
//  2. groups of 1 << log2g lanes take the chunk's pairs in turn: lane w moves word w of the slot (the pattern's words, the text's
//     right behind), so a slot is stored as one contiguous segment and each sequence is read as one.
// Every word is written by a vector store from the lane that read it; nothing is read back, nothing is atomic.
#include <algorithm>
#include "wfa_cross.hpp"

namespace wfa {

static_assert(WFA_PAIRS_CHUNK == 256, "one pair per thread of a 256-thread workgroup");

__global__ void __launch_bounds__(256) wfa_pairs_gen_kernel(PairsGenArgs a) {
  __shared__ uint32_t s_psrc[WFA_PAIRS_CHUNK], s_tsrc[WFA_PAIRS_CHUNK], s_dst[WFA_PAIRS_CHUNK], s_nw[WFA_PAIRS_CHUNK];
  __shared__ uint32_t s_wave[4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int G = 1 << a.log2g, gl = t & (G - 1), g0 = t >> a.log2g, ng = WFA_PAIRS_CHUNK >> a.log2g;
  const int64_t chunks = (a.npairs + WFA_PAIRS_CHUNK - 1) / WFA_PAIRS_CHUNK;
  for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
    const int64_t q = c * WFA_PAIRS_CHUNK + t;
    const bool live = q < a.npairs;
    WfaPairMeta m;
    m.p_woff = 0; m.t_woff = 0; m.plen = 0; m.tlen = 0;
    uint32_t nwp = 0, nw = 0, psrc = 0, tsrc = 0;
    int32_t ip = 0, jt = 0;
    bool slot = false;
    if (live) {
      ip = a.i[q]; jt = a.j[q];
      m.plen = a.p_len[ip]; m.tlen = a.t_len[jt];
      psrc = a.p_woff[ip]; tsrc = a.t_woff[jt];
      slot = m.plen <= WFA_FAST_MAX_LEN && m.tlen <= WFA_FAST_MAX_LEN;
      if (slot) { nwp = (uint32_t)(m.plen + 15) >> 4; nw = nwp + ((uint32_t)(m.tlen + 15) >> 4); }
    }
    uint32_t inc = nw;   // inclusive prefix over the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t v = __shfl_up(inc, off);
      if (lane >= off) inc += v;
    }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    uint32_t dst = a.chunk_base[c] + inc - nw;
    for (int w = 0; w < wave; ++w) dst += s_wave[w];
    if (live) {
      if (slot) { m.p_woff = dst; m.t_woff = dst + nwp; }
      else { m.p_woff = psrc; m.t_woff = tsrc + a.t_wshift; }   // (the batch's copy of the sets' words)
      a.meta[q] = m;
      if (a.lists) {
        const int f = a.all_bytes | a.p_flag[ip] | a.t_flag[jt];
        a.flags[q] = (uint8_t)(f ? 1 : 0);
        if (f) { a.pboff[q] = a.p_boff[ip]; a.tboff[q] = a.t_boff[jt] + a.t_bshift; }
      }
    }
    s_psrc[t] = psrc; s_tsrc[t] = tsrc; s_dst[t] = dst; s_nw[t] = nwp | (nw << 16);
    __syncthreads();
    for (int k = g0; k < WFA_PAIRS_CHUNK; k += ng) {
      const uint32_t v = s_nw[k], np = v & 0xffffu, ntot = v >> 16;
      const uint32_t ps = s_psrc[k], ts = s_tsrc[k], d = s_dst[k];
      for (uint32_t w = (uint32_t)gl; w < ntot; w += (uint32_t)G)
        a.words[d + w] = w < np ? a.p_words[ps + w] : a.t_words[ts + (w - np)];
    }
    __syncthreads();   // (the next round overwrites the chunk's LDS tables)
  }
}

int launch_pairs_gen(const PairsGenArgs& a, int cu_count, hipStream_t stream) {
  if (a.npairs <= 0) return 0;
  if (a.log2g < 0 || a.log2g > 6) return -1;
  const int64_t chunks = (a.npairs + WFA_PAIRS_CHUNK - 1) / WFA_PAIRS_CHUNK;
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(chunks, (int64_t)cu_count * 64));
  hipLaunchKernelGGL(wfa_pairs_gen_kernel, dim3(grid), dim3(256), 0, stream, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace wfa
