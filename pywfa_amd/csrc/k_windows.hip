// k_windows.hip — the generator of a windowed batch (wfa_cross.hpp: WindowsGenArgs, filled by WindowPairs::generate for batch_build_list in wfa_hip.hip).
// The shape of k_pairs.hip: a workgroup takes WFA_PAIRS_CHUNK listed pairs per round, in two steps:
//  1. thread t = pair t of the chunk: its indices, windows and strand, the words and (a byte pair) the bytes its slots need; two
//     exclusive prefix sums over the chunk (wave shuffles, the four wave totals through LDS) on top of the chunk's bases place the word
//     slot and the byte slot; the thread stores the pair's metadata;
//  2. groups of 1 << log2g lanes take the chunk's pairs in turn, the pattern window and then the text window: lane w loads ONE source
//     word (neighbouring lanes, neighbouring words: ascending for a forward window, descending for a reversed one), takes the word next
//     to it from the lane beside it (only the group's edge lane loads a second one), and builds and stores slot word w
//     (wfa_window_word: funnel shift by the start's residue; reversed: bit reversal, swap inside the 2-bit groups, XOR).  The same
//     groups fill the byte slot of a byte pair, four bytes per lane and store.
// A load never leaves its sequence's own words or bytes (words beyond either end read as zero), every slot word is written once by a
// vector store from the lane that built it; nothing is read back, nothing is atomic.
#include <algorithm>
#include "wfa_cross.hpp"

namespace wfa {

static_assert(WFA_PAIRS_CHUNK == 256, "one pair per thread of a 256-thread workgroup");

template <typename T>
__device__ inline T wave_inclusive(T v, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const T u = __shfl_up(v, off);
    if (lane >= off) v += u;
  }
  return v;
}

__device__ inline uint32_t complement_byte(uint32_t c) {
  switch (c) {
    case 'A': return 'T'; case 'T': return 'A'; case 'C': return 'G'; case 'G': return 'C';
    case 'a': return 't'; case 't': return 'a'; case 'c': return 'g'; case 'g': return 'c';
    default: return c;
  }
}

// the words of one window into its slot: `first0` = the first source base of slot word 0 (wfa_window_first), `nws` = the sequence's words
__device__ inline void gather_words(const uint32_t* __restrict__ src, uint32_t nws, int32_t first0, int32_t len, bool rev,
                                    uint32_t* __restrict__ dst, int gl, int G) {
  const uint32_t n = (uint32_t)(len + 15) >> 4;
  const int32_t w0 = first0 >> 4, dir = rev ? -1 : 1;
  const int edge = rev ? 0 : G - 1;
  for (uint32_t wb = 0; wb < n; wb += (uint32_t)G) {   // (the same trips for every lane of the group: they shuffle)
    const uint32_t w = wb + (uint32_t)gl;
    const int32_t si = w0 + dir * (int32_t)w;
    const uint32_t lo = (uint32_t)si < nws ? src[si] : 0u;
    uint32_t hi = rev ? __shfl_up(lo, 1, G) : __shfl_down(lo, 1, G);
    if (gl == edge) hi = (uint32_t)(si + 1) < nws ? src[si + 1] : 0u;
    if (w < n) dst[w] = wfa_window_word(lo, hi, (int64_t)first0 + 16 * dir * (int32_t)w, len, w, rev);
  }
}

// the bytes of one window into its byte slot (whole 32-bit words, zero behind the window)
__device__ inline void gather_bytes(const uint8_t* __restrict__ src, int32_t len, bool rev, uint8_t* __restrict__ dst, int gl, int G) {
  const uint32_t nd = (uint32_t)(len + 3) >> 2;
  for (uint32_t d = (uint32_t)gl; d < nd; d += (uint32_t)G) {
    uint32_t v = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int32_t pos = 4 * (int32_t)d + k;
      if (pos < len) v |= (rev ? complement_byte(src[len - 1 - pos]) : (uint32_t)src[pos]) << (8 * k);
    }
    reinterpret_cast<uint32_t*>(dst)[d] = v;
  }
}

__global__ void __launch_bounds__(256) wfa_windows_gen_kernel(WindowsGenArgs a) {
  __shared__ uint32_t s_psrc[WFA_PAIRS_CHUNK], s_tsrc[WFA_PAIRS_CHUNK], s_pnws[WFA_PAIRS_CHUNK], s_tnws[WFA_PAIRS_CHUNK], s_dst[WFA_PAIRS_CHUNK];
  __shared__ int32_t s_pfirst[WFA_PAIRS_CHUNK], s_tfirst[WFA_PAIRS_CHUNK], s_plen[WFA_PAIRS_CHUNK], s_tlen[WFA_PAIRS_CHUNK];
  __shared__ uint32_t s_opt[WFA_PAIRS_CHUNK];
  __shared__ int64_t s_pbsrc[WFA_PAIRS_CHUNK], s_tbsrc[WFA_PAIRS_CHUNK], s_bdst[WFA_PAIRS_CHUNK];
  __shared__ uint32_t s_wave[4];
  __shared__ uint64_t s_bwave[4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int G = 1 << a.log2g, gl = t & (G - 1), g0 = t >> a.log2g, ng = WFA_PAIRS_CHUNK >> a.log2g;
  const int64_t chunks = (a.npairs + WFA_PAIRS_CHUNK - 1) / WFA_PAIRS_CHUNK;
  for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
    const int64_t q = c * WFA_PAIRS_CHUNK + t;
    const bool live = q < a.npairs;
    WfaPairMeta m;
    m.p_woff = 0; m.t_woff = 0; m.plen = 0; m.tlen = 0;
    uint32_t nwp = 0, nw = 0, opt = 0;
    uint64_t nbp = 0, nb = 0;
    int32_t ip = 0, jt = 0, ps = 0, ts = 0, pl_seq = 0, tl_seq = 0;
    if (live) {
      ip = a.i[q]; jt = a.j[q];
      pl_seq = a.p_len[ip]; tl_seq = a.t_len[jt];
      ps = a.p_start ? a.p_start[q] : 0; ts = a.t_start ? a.t_start[q] : 0;
      m.plen = a.p_wlen ? a.p_wlen[q] : pl_seq - ps;
      m.tlen = a.t_wlen ? a.t_wlen[q] : tl_seq - ts;
      opt = (a.opt ? a.opt[q] : 0u) | (a.all_bytes ? (uint32_t)WFA_WIN_BYTES : 0u);
      nwp = (uint32_t)(m.plen + 15) >> 4; nw = nwp + ((uint32_t)(m.tlen + 15) >> 4);
      if (opt & WFA_WIN_BYTES) { nbp = ((uint64_t)m.plen + 3) & ~(uint64_t)3; nb = nbp + (((uint64_t)m.tlen + 3) & ~(uint64_t)3); }
    }
    const uint32_t inc = wave_inclusive(nw, lane);
    if (lane == 63) s_wave[wave] = inc;
    uint64_t binc = 0;
    if (a.lists) {
      binc = wave_inclusive(nb, lane);
      if (lane == 63) s_bwave[wave] = binc;
    }
    __syncthreads();
    uint32_t dst = a.chunk_base[c] + inc - nw;
    for (int w = 0; w < wave; ++w) dst += s_wave[w];
    int64_t bdst = 0;
    if (a.lists) {
      bdst = a.chunk_bbase[c] + (int64_t)(binc - nb);
      for (int w = 0; w < wave; ++w) bdst += (int64_t)s_bwave[w];
    }
    if (live) {
      m.p_woff = dst; m.t_woff = dst + nwp;
      a.meta[q] = m;
      if (a.lists) {
        const bool f = (opt & WFA_WIN_BYTES) != 0;
        a.flags[q] = (uint8_t)(f ? 1 : 0);
        if (f) { a.pboff[q] = bdst; a.tboff[q] = bdst + (int64_t)nbp; }
      }
    }
    const bool rev = (opt & WFA_WIN_REVERSE) != 0;
    s_psrc[t] = live ? a.p_woff[ip] : 0u; s_tsrc[t] = live ? a.t_woff[jt] : 0u;
    s_pnws[t] = (uint32_t)(pl_seq + 15) >> 4; s_tnws[t] = (uint32_t)(tl_seq + 15) >> 4;
    s_pfirst[t] = (int32_t)wfa_window_first(ps, m.plen, 0, rev); s_tfirst[t] = ts;
    s_plen[t] = m.plen; s_tlen[t] = m.tlen;
    s_dst[t] = dst; s_opt[t] = opt;
    if (a.lists) {
      s_pbsrc[t] = live ? a.p_boff[ip] + ps : 0; s_tbsrc[t] = live ? a.t_boff[jt] + ts : 0;
      s_bdst[t] = bdst;
    }
    __syncthreads();
    for (int k = g0; k < WFA_PAIRS_CHUNK; k += ng) {
      const int32_t pl = s_plen[k], tl = s_tlen[k];
      const uint32_t o = s_opt[k], d = s_dst[k];
      const bool r = (o & WFA_WIN_REVERSE) != 0;
      gather_words(a.p_words + s_psrc[k], s_pnws[k], s_pfirst[k], pl, r, a.words + d, gl, G);
      gather_words(a.t_words + s_tsrc[k], s_tnws[k], s_tfirst[k], tl, false, a.words + d + ((uint32_t)(pl + 15) >> 4), gl, G);
      if (a.lists && (o & WFA_WIN_BYTES)) {
        uint8_t* bd = a.bytes + s_bdst[k];
        gather_bytes(a.p_bytes + s_pbsrc[k], pl, r, bd, gl, G);
        gather_bytes(a.t_bytes + s_tbsrc[k], tl, false, bd + (((int64_t)pl + 3) & ~(int64_t)3), gl, G);
      }
    }
    __syncthreads();   // (the next round overwrites the chunk's LDS tables)
  }
}

int launch_windows_gen(const WindowsGenArgs& a, int cu_count, hipStream_t stream) {
  if (a.npairs <= 0) return 0;
  if (a.log2g < 2 || a.log2g > 6) return -1;
  const int64_t chunks = (a.npairs + WFA_PAIRS_CHUNK - 1) / WFA_PAIRS_CHUNK;
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(chunks, (int64_t)cu_count * 64));
  hipLaunchKernelGGL(wfa_windows_gen_kernel, dim3(grid), dim3(256), 0, stream, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace wfa
