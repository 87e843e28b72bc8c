// k_seed.hip — the seed finder's kernels (wfa_seed.hpp: layout, rule and the kernels' outline; wfa_hip_seed_index_* in wfa_hip.hip).
// Stores: the count / fill kernels add into table[code] (code < 4^k by its mask) and write record slots below the records' capacity;
// the scan writes the table's own 4^k + 1 counters and its chunk sums; the query writes row i < npat of the result arrays, columns
// below n, and overflow[i].
#include <algorithm>
#include "k_seed.hpp"

namespace wfa {

// ---- build -------------------------------------------------------------------------------------------------------------------

// the sequence that owns word g of the set's table: the last one that starts at or before it (empty sequences own no word)
__device__ inline int64_t seed_owner(const SeedSetView& s, uint32_t g) {
  int64_t lo = 0, hi = s.nseq;   // first sequence that starts behind g
  while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (s.woff[mid] > g) hi = mid; else lo = mid + 1; }
  return lo - 1;
}

template <bool FILL>
__global__ void __launch_bounds__(256) wfa_seed_positions_kernel(SeedBuildArgs a, uint32_t cap) {
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  const uint32_t kbits = (1u << (2 * a.k)) - 1u, kones = (1u << a.k) - 1u;
  for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < a.t.nwords; g += nthreads) {
    const int64_t j = seed_owner(a.t, (uint32_t)g);
    if (j < 0) continue;
    const int32_t len = a.t.len[j], p0 = 16 * (int32_t)((uint32_t)g - a.t.woff[j]);
    if (p0 + a.k > len) continue;
    const uint64_t v = ((uint64_t)a.t.words[g + 1] << 32) | a.t.words[g];
    const uint32_t m = a.t.mask ? (uint32_t)a.t.mask[g] | ((uint32_t)a.t.mask[g + 1] << 16) : 0u;
    for (int u = 0; u < 16; ++u) {
      const int32_t p = p0 + u;
      if (p + a.k > len) break;
      if (a.stride > 1 && p % a.stride != 0) continue;
      if ((m >> u) & kones) continue;
      const uint32_t code = (uint32_t)(v >> (2 * u)) & kbits;
      if (!FILL) {
        atomicAdd(&a.table[code], 1u);
      } else {
        const uint32_t slot = atomicSub(&a.table[code], 1u) - 1u;
        if (slot < cap) { SeedRec r; r.j = (int32_t)j; r.t = p; a.recs[slot] = r; }
      }
    }
  }
}

// the minimizer form: the same thread per word, the same stores; a position is taken when it is a minimizer of ITS sequence (keys and
// neighbours from the owner's first word and length: beyond its last k-mer start the neighbours are +inf, whatever word follows).
// Count and fill run the one predicate on the same words, so they select identically.
template <bool FILL>
__global__ void __launch_bounds__(256) wfa_seed_minimizer_positions_kernel(SeedBuildArgs a, uint32_t cap) {
  const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < a.t.nwords; g += nthreads) {
    const int64_t j = seed_owner(a.t, (uint32_t)g);
    if (j < 0) continue;
    const uint32_t w0 = a.t.woff[j];
    const int32_t len = a.t.len[j], p0 = 16 * (int32_t)((uint32_t)g - w0);
    for (int u = 0; u < 16; ++u) {
      const int32_t p = p0 + u;
      if (p + a.k > len) break;
      uint32_t code;
      const uint64_t kp = seed_key(a.t, w0, len, p, a.k, &code);
      if (kp == WFA_SEED_KEY_INF || !seed_selected(a.t, w0, len, p, a.k, a.w, kp)) continue;
      if (!FILL) {
        atomicAdd(&a.table[code], 1u);
      } else {
        const uint32_t slot = atomicSub(&a.table[code], 1u) - 1u;
        if (slot < cap) { SeedRec r; r.j = (int32_t)j; r.t = p; a.recs[slot] = r; }
      }
    }
  }
}

// chunk sums of the table's counters, and the k-mers over max_occ
__global__ void __launch_bounds__(256) wfa_seed_scan_reduce_kernel(SeedBuildArgs a, uint64_t count) {
  __shared__ uint32_t s_red[4];
  const uint64_t base = (uint64_t)blockIdx.x * WFA_SEED_SCAN_CHUNK + (uint64_t)threadIdx.x * 16;
  uint32_t sum = 0, over = 0;
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    const uint32_t c = base + u < count ? a.table[base + u] : 0u;
    sum += c; over += c > a.max_occ ? 1u : 0u;
  }
  sum = seed_block_sum(sum, s_red);
  over = seed_block_sum(over, s_red);
  if (threadIdx.x == 0) {
    a.bsum[blockIdx.x] = sum;
    if (over) atomicAdd(a.masked, over);
  }
}

// the chunk sums to their exclusive prefix, in place: one workgroup, 256 sums per round
__global__ void __launch_bounds__(256) wfa_seed_scan_top_kernel(uint32_t* bsum, uint32_t chunks) {
  __shared__ uint32_t s_red[4];
  uint32_t carry = 0;
  for (uint32_t b0 = 0; b0 < chunks; b0 += 256) {
    const uint32_t i = b0 + threadIdx.x;
    const uint32_t v = i < chunks ? bsum[i] : 0u;
    uint32_t total;
    const uint32_t ex = seed_block_exclusive(v, s_red, &total);
    if (i < chunks) bsum[i] = carry + ex;
    carry += total;
  }
}

// every counter to the inclusive prefix of the whole table: the END of its bucket
__global__ void __launch_bounds__(256) wfa_seed_scan_apply_kernel(SeedBuildArgs a, uint64_t count) {
  __shared__ uint32_t s_red[4];
  const uint64_t base = (uint64_t)blockIdx.x * WFA_SEED_SCAN_CHUNK + (uint64_t)threadIdx.x * 16;
  uint32_t c[16];
  uint32_t sum = 0;
#pragma unroll
  for (int u = 0; u < 16; ++u) { c[u] = base + u < count ? a.table[base + u] : 0u; sum += c[u]; }
  uint32_t total;
  uint32_t run = a.bsum[blockIdx.x] + seed_block_exclusive(sum, s_red, &total);
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    run += c[u];
    if (base + u < count) a.table[base + u] = run;
  }
}

static unsigned positions_grid(uint64_t nwords) { return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((nwords + 255) / 256, 1u << 16)); }

int launch_seed_count(const SeedBuildArgs& a, hipStream_t stream) {
  if (a.t.nwords == 0) return 0;
  if (a.w >= 1) hipLaunchKernelGGL(wfa_seed_minimizer_positions_kernel<false>, dim3(positions_grid(a.t.nwords)), dim3(256), 0, stream, a, 0u);
  else hipLaunchKernelGGL(wfa_seed_positions_kernel<false>, dim3(positions_grid(a.t.nwords)), dim3(256), 0, stream, a, 0u);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_seed_scan(const SeedBuildArgs& a, hipStream_t stream) {
  const uint64_t count = (1ull << (2 * a.k)) + 1;
  const unsigned chunks = (unsigned)((count + WFA_SEED_SCAN_CHUNK - 1) / WFA_SEED_SCAN_CHUNK);
  hipLaunchKernelGGL(wfa_seed_scan_reduce_kernel, dim3(chunks), dim3(256), 0, stream, a, count);
  hipLaunchKernelGGL(wfa_seed_scan_top_kernel, dim3(1), dim3(256), 0, stream, a.bsum, chunks);
  hipLaunchKernelGGL(wfa_seed_scan_apply_kernel, dim3(chunks), dim3(256), 0, stream, a, count);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_seed_fill(const SeedBuildArgs& a, uint32_t cap, hipStream_t stream) {
  if (a.t.nwords == 0 || cap == 0) return 0;
  if (a.w >= 1) hipLaunchKernelGGL(wfa_seed_minimizer_positions_kernel<true>, dim3(positions_grid(a.t.nwords)), dim3(256), 0, stream, a, cap);
  else hipLaunchKernelGGL(wfa_seed_positions_kernel<true>, dim3(positions_grid(a.t.nwords)), dim3(256), 0, stream, a, cap);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---- query -------------------------------------------------------------------------------------------------------------------

#define WFA_SEED_SAT 8192u   // a thread's hit count saturates here (above any max_hits): 256 of them still fit 32 bits

__device__ inline uint32_t seed_occ(const SeedQueryArgs& a, uint32_t code, uint32_t* first) {
  const uint32_t b0 = a.table[code], cnt = a.table[code + 1] - b0;
  *first = b0;
  return cnt > a.max_occ ? 0u : cnt;
}

template <bool MINI>   // MINI: the index is a minimizer index (a.w >= 1), only the read's minimizers are looked up
__global__ void __launch_bounds__(256) wfa_seed_query_kernel(SeedQueryArgs a, int64_t npat) {
  __shared__ uint64_t s_key[WFA_SEED_MAX_HITS];
  __shared__ uint16_t s_seg[2][WFA_SEED_MAX_HITS];
  __shared__ uint32_t s_red[4];
  __shared__ uint32_t s_fill;
  const int t = threadIdx.x, k = a.k, n = a.n;
  for (int64_t i = blockIdx.x; i < npat; i += gridDim.x) {
    const int32_t L = a.p.len[i];
    const uint32_t w0 = a.p.woff[i];
    const int32_t npos = L - k + 1;   // k-mer starts of one strand (<= 0: the read is shorter than k)
    // 1. the read's hits, both strands
    uint32_t mine = 0;
    for (int32_t q = t; q < npos; q += 256) {
      uint32_t code, first;
      if (!seed_read_kmer<MINI>(a.p, w0, L, q, k, a.w, &code)) continue;
      mine = min(mine + min(seed_occ(a, code, &first), WFA_SEED_SAT), WFA_SEED_SAT);
      mine = min(mine + min(seed_occ(a, seed_rc(code, k), &first), WFA_SEED_SAT), WFA_SEED_SAT);
    }
    if (t == 0) s_fill = 0u;
    const uint32_t H = seed_block_sum(mine, s_red);   // (its barriers also publish s_fill)
    const bool overflow = H > (uint32_t)a.max_hits;
    if (t == 0) a.overflow[i] = overflow ? 1 : 0;
    int slot = 0;
    if (!overflow && H > 0) {
      // 2. the hits as keys: strand | text | d biased to unsigned, so that the keys' order is the order of (s, j, d)
      for (int32_t q = t; q < npos; q += 256) {
        uint32_t code;
        if (!seed_read_kmer<MINI>(a.p, w0, L, q, k, a.w, &code)) continue;
        for (int s = 0; s < 2; ++s) {
          uint32_t first;
          const uint32_t cnt = seed_occ(a, s ? seed_rc(code, k) : code, &first);
          if (cnt == 0) continue;
          const int32_t r = s ? L - k - q : q;
          const uint32_t at = atomicAdd(&s_fill, cnt);
          for (uint32_t u = 0; u < cnt; ++u) {
            const SeedRec rec = a.recs[first + u];
            if (at + u < WFA_SEED_MAX_HITS)
              s_key[at + u] = ((uint64_t)s << 63) | ((uint64_t)(uint32_t)rec.j << 32) | (uint64_t)((uint32_t)(rec.t - r) ^ 0x80000000u);
          }
        }
      }
      uint32_t N = 2;
      while (N < H) N <<= 1;
      for (uint32_t e = H + t; e < N; e += 256) s_key[e] = ~0ull;
      __syncthreads();
      // 3. bitonic sort of the N keys
      for (uint32_t size = 2; size <= N; size <<= 1) {
        for (uint32_t st = size >> 1; st > 0; st >>= 1) {
          for (uint32_t x = t; x < (N >> 1); x += 256) {
            const uint32_t lo = 2 * x - (x & (st - 1));
            const uint64_t ka = s_key[lo], kb = s_key[lo + st];
            if ((ka > kb) == ((lo & size) == 0)) { s_key[lo] = kb; s_key[lo + st] = ka; }
          }
          __syncthreads();
        }
      }
      // 4. cluster starts, carried to every hit of the cluster by a max-scan
      for (uint32_t e = t; e < H; e += 256) {
        bool start = e == 0;
        if (!start) {
          const uint64_t ka = s_key[e - 1], kb = s_key[e];
          start = (ka >> 32) != (kb >> 32) || (uint32_t)kb - (uint32_t)ka > a.gap;
        }
        s_seg[0][e] = start ? (uint16_t)e : (uint16_t)0;
      }
      __syncthreads();
      int cur = 0;
      for (uint32_t off = 1; off < H; off <<= 1) {
        for (uint32_t e = t; e < H; e += 256) {
          const uint16_t v = s_seg[cur][e], u = e >= off ? s_seg[cur][e - off] : (uint16_t)0;
          s_seg[cur ^ 1][e] = v > u ? v : u;
        }
        cur ^= 1;
        __syncthreads();
      }
      // 5. the best n clusters: hits descending, then the start's place in the sorted hits ascending (= (s, j, d_lo) ascending)
      const uint16_t* seg = s_seg[cur];
      int64_t prev = -1;
      for (; slot < n; ++slot) {
        uint32_t best = 0xFFFFFFFFu;
        for (uint32_t e = t; e < H; e += 256) {
          if (e + 1 < H && seg[e + 1] != e + 1) continue;   // (not the last hit of its cluster)
          const uint32_t st = seg[e], c = e - st + 1;
          if ((int64_t)c < (int64_t)a.min_hits) continue;
          const uint32_t rk = ((WFA_SEED_MAX_HITS - c) << 12) | st;
          if ((int64_t)rk > prev) best = min(best, rk);
        }
        best = seed_block_min(best, s_red);
        if (best == 0xFFFFFFFFu) break;
        prev = best;
        if (t == 0) {
          const uint32_t st = best & 4095u, c = WFA_SEED_MAX_HITS - (best >> 12);
          const uint64_t k0 = s_key[st], k1 = s_key[st + c - 1];
          const int32_t jt = (int32_t)((k0 >> 32) & 0x7FFFFFFFu);
          const int64_t d_lo = (int32_t)((uint32_t)k0 ^ 0x80000000u), d_hi = (int32_t)((uint32_t)k1 ^ 0x80000000u);
          const int64_t tl = (jt < a.t_nseq) ? a.t_len[jt] : 0;
          const int64_t lo_w = d_lo - a.pad, hi_w = d_hi + L + a.pad;
          const int64_t ts = lo_w > 0 ? lo_w : 0, te = hi_w < tl ? hi_w : tl;
          const int64_t o = i * n + slot;
          a.j[o] = jt; a.reverse[o] = (int32_t)(k0 >> 63); a.text_start[o] = (int32_t)ts; a.text_len[o] = (int32_t)(te - ts); a.hits[o] = (int32_t)c;
        }
      }
      __syncthreads();   // (the next read overwrites the keys)
    }
    for (int q = slot + t; q < n; q += 256) {
      const int64_t o = i * n + q;
      a.j[o] = -1; a.reverse[o] = 0; a.text_start[o] = 0; a.text_len[o] = 0; a.hits[o] = 0;
    }
  }
}

int launch_seed_query(const SeedQueryArgs& a, int64_t npat, int cu_count, hipStream_t stream) {
  if (npat <= 0) return 0;
  if (a.k < WFA_SEED_MIN_K || a.k > WFA_SEED_MAX_K || a.n < 1 || a.n > WFA_SEED_MAX_N || a.max_hits < 1 || a.max_hits > WFA_SEED_MAX_HITS || a.w < 0 ||
      a.w > WFA_SEED_MAX_W)
    return -1;
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(npat, (int64_t)cu_count * 12));
  if (a.w >= 1) hipLaunchKernelGGL(wfa_seed_query_kernel<true>, dim3(grid), dim3(256), 0, stream, a, npat);
  else hipLaunchKernelGGL(wfa_seed_query_kernel<false>, dim3(grid), dim3(256), 0, stream, a, npat);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace wfa
