// k_chain.hip — the chaining kernel on the seed index (wfa_chain.hpp: rule, workspace and the kernel's outline; wfa_hip_seed_index_chain
// in wfa_hip.hip).
// Stores: the gather and the chain write the workgroup's own slab (blockIdx.x < the grid the workspace was sized for) at anchor slots
// below max_anchors; the selection writes row i < npat of the result arrays, columns below n, overflow[i], and f of slab slots below N.
#include <algorithm>
#include "k_seed.hpp"
#include "wfa_chain.hpp"

namespace wfa {

#define WFA_CHAIN_SAT 65537u   // a thread's anchor count saturates here (above any max_anchors): 512 of them still fit 32 bits

__device__ inline uint32_t chain_occ(const ChainArgs& a, uint32_t code, uint32_t* first) {
  const uint32_t b0 = a.table[code], cnt = a.table[code + 1] - b0;
  *first = b0;
  return cnt > a.max_occ ? 0u : cnt;
}

__device__ inline uint32_t chain_wave_max(uint32_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = max(v, (uint32_t)__shfl_xor(v, off));
  return v;
}

// maximum of a 64-bit key over the 256 threads of a workgroup; s_red: 4 words of LDS, free again when the call returns
__device__ inline uint64_t chain_block_max(uint64_t v, uint64_t* s_red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t lo = __shfl_xor((uint32_t)v, off), hi = __shfl_xor((uint32_t)(v >> 32), off);
    const uint64_t u = ((uint64_t)hi << 32) | lo;
    v = u > v ? u : v;
  }
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  const uint64_t a = s_red[0] > s_red[1] ? s_red[0] : s_red[1], b = s_red[2] > s_red[3] ? s_red[2] : s_red[3];
  __syncthreads();
  return a > b ? a : b;
}

// cost(0) = 0, cost(g) = ((g * k) >> 6) + (floor(log2 g) >> 1)
__device__ inline int32_t chain_cost(int32_t g, int k) {
  return g == 0 ? 0 : ((g * k) >> 6) + ((31 - __clz(g)) >> 1);
}

// the cnt records of a bucket to the anchor slots at .. at + cnt of read position r, ordered by (j, t): a record's place is the number
// of records of its bucket below it (the records are distinct)
__device__ inline void chain_place(const SeedRec* recs, uint32_t first, uint32_t cnt, uint32_t at, int32_t r, uint32_t cap,
                                   int32_t* aj, int32_t* at_, int32_t* ar) {
  for (uint32_t u = 0; u < cnt; ++u) {
    const SeedRec rec = recs[first + u];
    uint32_t rank = 0;
    for (uint32_t v = 0; v < cnt; ++v) {
      const SeedRec o = recs[first + v];
      rank += (o.j < rec.j || (o.j == rec.j && o.t < rec.t)) ? 1u : 0u;
    }
    const uint32_t slot = at + rank;
    if (slot < cap) { aj[slot] = rec.j; at_[slot] = rec.t; ar[slot] = r; }
  }
}

template <bool MINI>   // MINI: the index is a minimizer index (a.w >= 1), only the read's minimizers give anchors
__global__ void __launch_bounds__(256) wfa_chain_kernel(ChainArgs a, int64_t npat) {
  __shared__ uint32_t s_red[4];
  __shared__ uint64_t s_red64[4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, k = a.k, n = a.n;
  const uint32_t cap = a.max_anchors;
  int32_t* const slab = a.slab + (size_t)blockIdx.x * WFA_CHAIN_PLANES * cap;
  int32_t *const aj = slab, *const at = slab + cap, *const ar = slab + 2 * (size_t)cap, *const af = slab + 3 * (size_t)cap,
          *const acnt = slab + 4 * (size_t)cap, *const alo = slab + 5 * (size_t)cap, *const ahi = slab + 6 * (size_t)cap,
          *const afirst = slab + 7 * (size_t)cap;
  for (int64_t i = blockIdx.x; i < npat; i += gridDim.x) {
    const int32_t L = a.p.len[i];
    const uint32_t w0 = a.p.woff[i];
    const int32_t npos = L - k + 1;   // k-mer starts of one strand (<= 0: the read is shorter than k)
    const int32_t per = npos > 0 ? (npos + 255) / 256 : 0;
    const int64_t all = max(npos, 0);
    const int32_t q0 = (int32_t)min((int64_t)t * per, all), q1 = (int32_t)min((int64_t)q0 + per, all);   // the thread's k-mer starts
    // 1. count: the anchors of the thread's range on either strand, and its place in (s, r) order
    uint32_t c0 = 0, c1 = 0;
    for (int32_t q = q0; q < q1; ++q) {
      uint32_t code, first;
      if (!seed_read_kmer<MINI>(a.p, w0, L, q, k, a.w, &code)) continue;
      c0 = min(c0 + min(chain_occ(a, code, &first), WFA_CHAIN_SAT), WFA_CHAIN_SAT);
      c1 = min(c1 + min(chain_occ(a, seed_rc(code, k), &first), WFA_CHAIN_SAT), WFA_CHAIN_SAT);
    }
    uint32_t N0, N1;
    const uint32_t e0 = seed_block_exclusive(c0, s_red, &N0);
    const uint32_t e1 = seed_block_exclusive(c1, s_red, &N1);
    const uint32_t N = N0 + N1;
    const bool overflow = N > cap;   // (no thread saturated otherwise: the places are exact)
    if (t == 0) a.overflow[i] = overflow ? 1 : 0;
    int slot = 0;
    if (!overflow && N > 0) {
      // 2. gather: strand 0 up the range; strand 1 down it (r = L - k - q), its place counted from the far end of the read (under
      // a minimizer index from the same positions q: the minimizers of the reverse complement are the mirrored positions)
      uint32_t p0 = e0, p1 = N0 + (N1 - (e1 + c1));
      for (int32_t q = q0; q < q1; ++q) {
        uint32_t code, first;
        if (!seed_read_kmer<MINI>(a.p, w0, L, q, k, a.w, &code)) continue;
        const uint32_t cnt = chain_occ(a, code, &first);
        chain_place(a.recs, first, cnt, p0, q, cap, aj, at, ar);
        p0 += cnt;
      }
      for (int32_t q = q1 - 1; q >= q0; --q) {
        uint32_t code, first;
        if (!seed_read_kmer<MINI>(a.p, w0, L, q, k, a.w, &code)) continue;
        const uint32_t cnt = chain_occ(a, seed_rc(code, k), &first);
        chain_place(a.recs, first, cnt, p1, L - k - q, cap, aj, at, ar);
        p1 += cnt;
      }
      __syncthreads();
      // 3. chain: a wave per strand; anchor x of the round is in lane x, the last 64 anchors' state in the lane of their index % 64
      if (wave < 2) {
        const uint32_t begin = wave ? N0 : 0u, end = wave ? N : N0;
        int32_t hj = -1, ht = 0, hr = 0, hf = 0, hcnt = 0, hlo = 0, hhi = 0, hfirst = 0;   // (j = -1: the lane holds no anchor yet)
        for (uint32_t base = begin; base < end; base += 64) {
          const uint32_t mine = base + lane;
          const bool have = mine < end;
          const int32_t nj = have ? aj[mine] : -1, nt = have ? at[mine] : 0, nr = have ? ar[mine] : 0;
          const int round = (int)min(64u, end - base);
          for (int x = 0; x < round; ++x) {
            const int32_t xj = __shfl(nj, x), xt = __shfl(nt, x), xr = __shfl(nr, x);
            const int dist = ((x - lane - 1) & 63) + 1;   // the lane's anchor lies this far before anchor x in the order
            const int32_t dr = xr - hr, dt = xt - ht;
            const bool near = hj == xj && dist <= a.lookback && dr > 0 && dt > 0 && dr <= a.max_dist && dt <= a.max_dist;
            const int32_t g = near ? abs(dt - dr) : 0;
            const int32_t v = hf + min(min(dr, dt), k) - chain_cost(g, k);
            const uint32_t key = (near && g <= a.band && v > k) ? ((uint32_t)v << 7) | (uint32_t)(64 - dist) : 0u;
            const uint32_t best = chain_wave_max(key);
            const int32_t d = xt - xr;
            // (the winner's lane is read by every lane, winner or none: no cross-lane read under a branch)
            const int w = (x - (64 - (int)(best & 127u))) & 63;
            const int32_t wcnt = __shfl(hcnt, w), wlo = __shfl(hlo, w), whi = __shfl(hhi, w), wfirst = __shfl(hfirst, w);
            const bool adopt = best != 0u;
            const int32_t f = adopt ? (int32_t)(best >> 7) : k, cnt = adopt ? wcnt + 1 : 1, lo = adopt ? min(wlo, d) : d,
                          hi = adopt ? max(whi, d) : d, first = adopt ? wfirst : xr;
            if (lane == x) { hj = xj; ht = xt; hr = xr; hf = f; hcnt = cnt; hlo = lo; hhi = hi; hfirst = first; }
          }
          if (have) { af[mine] = hf; acnt[mine] = hcnt; alo[mine] = hlo; ahi[mine] = hhi; afirst[mine] = hfirst; }
        }
      }
      __syncthreads();
      // 4. select: thread x looks after the anchors x, x + 256, ...; the chosen anchor's planes are read by every thread
      for (; slot < n; ++slot) {
        uint64_t mine = 0;
        for (uint32_t e = t; e < N; e += 256) {
          const int32_t f = af[e];
          if (f >= 0 && f >= a.min_score && acnt[e] >= a.min_hits) {
            const uint64_t key = ((uint64_t)(uint32_t)f << 32) | (uint64_t)(0xFFFFFFFFu - e);
            mine = key > mine ? key : mine;
          }
        }
        const uint64_t best = chain_block_max(mine, s_red64);
        if (best == 0) break;   // (the same in every thread)
        const uint32_t e = 0xFFFFFFFFu - (uint32_t)best;
        const int32_t s = e >= N0 ? 1 : 0, jt = aj[e];
        const int64_t tl = (jt >= 0 && jt < a.t_nseq) ? a.t_len[jt] : 0;
        const int64_t lo_w = (int64_t)alo[e] - a.pad, hi_w = (int64_t)ahi[e] + L + a.pad;
        const int64_t ts = lo_w > 0 ? lo_w : 0, te = hi_w < tl ? hi_w : tl;
        if (t == 0) {
          const int64_t o = i * n + slot;
          const int32_t r = ar[e], first = afirst[e];
          a.j[o] = jt; a.reverse[o] = s; a.text_start[o] = (int32_t)ts; a.text_len[o] = (int32_t)(te - ts); a.hits[o] = acnt[e];
          a.score[o] = (int32_t)(best >> 32);
          a.pattern_start[o] = s ? L - (r + k) : first; a.pattern_len[o] = r + k - first;
        }
        for (uint32_t c = t; c < N; c += 256) {
          const int64_t ct = at[c];
          if ((c >= N0 ? 1 : 0) == s && aj[c] == jt && ts <= ct && ct + k <= te) af[c] = -1;
        }
      }
      // (the next read's gather lies behind the barriers of its scans: no thread is still reading this read's planes then)
    }
    for (int q = slot + t; q < n; q += 256) {
      const int64_t o = i * n + q;
      a.j[o] = -1; a.reverse[o] = 0; a.text_start[o] = 0; a.text_len[o] = 0; a.hits[o] = 0; a.score[o] = 0; a.pattern_start[o] = 0;
      a.pattern_len[o] = 0;
    }
  }
}

unsigned chain_grid(int64_t npat, int cu_count) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(npat, (int64_t)cu_count * WFA_CHAIN_BLOCKS_PER_CU));
}

int launch_chain(const ChainArgs& a, int64_t npat, unsigned grid, hipStream_t stream) {
  if (npat <= 0) return 0;
  if (a.k < WFA_SEED_MIN_K || a.k > WFA_SEED_MAX_K || a.n < 1 || a.n > WFA_SEED_MAX_N || a.lookback < 1 || a.lookback > WFA_CHAIN_MAX_LOOKBACK ||
      a.max_anchors < 1 || a.max_anchors > WFA_CHAIN_MAX_ANCHORS || !a.slab || grid < 1 || a.w < 0 || a.w > WFA_SEED_MAX_W)
    return -1;
  if (a.w >= 1) hipLaunchKernelGGL(wfa_chain_kernel<true>, dim3(grid), dim3(256), 0, stream, a, npat);
  else hipLaunchKernelGGL(wfa_chain_kernel<false>, dim3(grid), dim3(256), 0, stream, a, npat);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace wfa
