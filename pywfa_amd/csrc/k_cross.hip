// k_cross.hip — translation unit of the cross-product kernels (wfa_cross.hpp): band generator, scatter into the dense matrix, ordered
// compaction of the completed pairs, top-k per row.  Every result is written by vector stores from the thread that owns it.
#include <algorithm>
#include "wfa_cross.hpp"

namespace wfa {

// pairs of the upper triangle (columns j >= i) in the rows before row i, n columns
__device__ __forceinline__ int64_t cross_tri_before(int64_t i, int64_t n) { return i * n - (i * (i - 1)) / 2; }

// band pair q -> (i, j).  Triangle: the root of i^2 - (2n + 1) i + 2g = 0 as a first guess, then exact integer steps
__device__ __forceinline__ void cross_decode(int tri, int64_t n, int64_t r0, int64_t tri0, int64_t q, int64_t* i, int64_t* j) {
  if (!tri) {
    const int64_t r = q / n;
    *i = r0 + r; *j = q - r * n;
    return;
  }
  const int64_t g = tri0 + q;
  const double b = 2.0 * (double)n + 1.0;
  double d = b * b - 8.0 * (double)g;
  if (d < 0.0) d = 0.0;
  int64_t r = (int64_t)((b - sqrt(d)) * 0.5);
  if (r < 0) r = 0;
  if (r > n - 1) r = n - 1;
  while (r + 1 < n && cross_tri_before(r + 1, n) <= g) ++r;
  while (r > 0 && cross_tri_before(r, n) > g) --r;
  *i = r; *j = r + (g - cross_tri_before(r, n));
}

__global__ void __launch_bounds__(256) wfa_cross_gen_kernel(CrossGenArgs a) {
  const int64_t rb0 = a.lists ? a.row_bytes[a.r0] : 0;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < a.npairs; q += (int64_t)gridDim.x * 256) {
    int64_t i, j;
    cross_decode(a.tri, a.n, a.r0, a.tri0, q, &i, &j);
    WfaPairMeta m;
    m.p_woff = a.p_woff[i]; m.t_woff = a.t_woff[j] + a.t_wshift; m.plen = a.p_len[i]; m.tlen = a.t_len[j];
    if (m.plen <= WFA_FAST_MAX_LEN && m.tlen <= WFA_FAST_MAX_LEN) {   // (the pair's slot: pattern words, text words right behind)
      const uint32_t o = a.slot_base + (uint32_t)q * a.slot_words, nwp = (uint32_t)(m.plen + 15) >> 4, nwt = (uint32_t)(m.tlen + 15) >> 4;
      for (uint32_t w = 0; w < nwp; ++w) a.words[o + w] = a.words[m.p_woff + w];
      for (uint32_t w = 0; w < nwt; ++w) a.words[o + nwp + w] = a.words[m.t_woff + w];
      m.p_woff = o; m.t_woff = o + nwp;
    }
    a.meta[q] = m;
    if (!a.lists) continue;
    const int pf = a.all_bytes | a.p_flag[i], tf = a.all_bytes | a.t_flag[j];
    const int64_t rbi = a.row_bytes[i] - rb0;                                      // byte pairs of the band before row i
    const int64_t row_pairs = a.tri ? cross_tri_before(i, a.n) - a.tri0 : (i - a.r0) * a.n;   // pairs of the band before row i
    const int64_t c0 = a.tri ? i : 0;                                              // first column of row i
    const int64_t cf = a.col_flag[j] - a.col_flag[c0];                            // flagged columns of the row before column j
    if (pf | tf) {
      a.pboff[q] = a.p_boff[i]; a.tboff[q] = a.t_boff[j] + a.t_bshift; a.flags[q] = 1;
      a.list_bytes[rbi + (pf ? j - c0 : cf)] = (uint32_t)q;
    } else {
      a.flags[q] = 0;
      a.list_packed[row_pairs - rbi + (j - c0) - cf] = (uint32_t)q;
    }
  }
}

__global__ void __launch_bounds__(256) wfa_cross_scatter_kernel(CrossResArgs a) {
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < a.npairs; q += (int64_t)gridDim.x * 256) {
    int64_t i, j;
    cross_decode(a.tri, a.n, a.r0, a.tri0, q, &i, &j);
    const int32_t s = a.score[q], st = a.status[q];
    a.dense_score[i * a.n + j] = s; a.dense_status[i * a.n + j] = st;
    if (a.mirror && i != j) { a.dense_score[j * a.n + i] = s; a.dense_status[j * a.n + i] = st; }
  }
}

__device__ __forceinline__ bool cross_keep(const CrossResArgs& a, int64_t q, int64_t* i, int64_t* j) {
  if (q >= a.npairs) return false;
  cross_decode(a.tri, a.n, a.r0, a.tri0, q, i, j);
  return a.status[q] == 0 && (!a.upper || *j > *i);
}

// pass 1: completed pairs per workgroup of WFA_CROSS_CHUNK pairs
__global__ void __launch_bounds__(256) wfa_cross_count_kernel(CrossResArgs a) {
  __shared__ uint32_t wsum[4];
  const int64_t base = (int64_t)blockIdx.x * WFA_CROSS_CHUNK;
  uint32_t cnt = 0;
  for (int r = 0; r < WFA_CROSS_CHUNK / 256; ++r) {
    int64_t i, j;
    cnt += cross_keep(a, base + r * 256 + threadIdx.x, &i, &j) ? 1u : 0u;
  }
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) a.blk_count[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// pass 2 (one workgroup): exclusive prefix of the counts in place, the band's total
__global__ void __launch_bounds__(1024) wfa_cross_scan_kernel(CrossResArgs a, uint32_t nblk) {
  __shared__ uint32_t part[1024];
  const uint32_t t = threadIdx.x, per = (nblk + 1023u) / 1024u;
  const uint32_t lo = min(nblk, t * per), hi = min(nblk, lo + per);
  uint32_t s = 0;
  for (uint32_t k = lo; k < hi; ++k) s += a.blk_count[k];
  part[t] = s;
  __syncthreads();
  for (uint32_t off = 1; off < 1024u; off <<= 1) {   // inclusive scan (Hillis-Steele)
    const uint32_t v = t >= off ? part[t - off] : 0u;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  uint32_t run = part[t] - s;
  for (uint32_t k = lo; k < hi; ++k) { const uint32_t c = a.blk_count[k]; a.blk_count[k] = run; run += c; }
  if (t == 1023u) a.band_count[0] = part[1023];
}

// pass 3: every workgroup writes its completed pairs in pair order from its offset (wave ballots, wave totals in LDS)
__global__ void __launch_bounds__(256) wfa_cross_write_kernel(CrossResArgs a) {
  __shared__ uint32_t wtot[4];
  const int64_t base = (int64_t)blockIdx.x * WFA_CROSS_CHUNK;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t pos = a.blk_count[blockIdx.x];
  for (int r = 0; r < WFA_CROSS_CHUNK / 256; ++r) {
    const int64_t q = base + r * 256 + threadIdx.x;
    int64_t i = 0, j = 0;
    const bool keep = cross_keep(a, q, &i, &j);
    const unsigned long long mask = __ballot(keep);
    if (lane == 0) wtot[wave] = (uint32_t)__popcll(mask);
    __syncthreads();
    uint32_t woff = 0, total = 0;
    for (int w = 0; w < 4; ++w) { woff += (w < wave) ? wtot[w] : 0u; total += wtot[w]; }
    if (keep) {
      const uint32_t at = pos + woff + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
      a.out_i[at] = (int32_t)i; a.out_j[at] = (int32_t)j; a.out_score[at] = a.score[q];
    }
    pos += total;
    __syncthreads();
  }
}

// ---- top-k per row (wfa_cross.hpp: CrossTopkArgs) ----

__device__ __forceinline__ uint64_t topk_key(int32_t score, int64_t j) {
  return ((uint64_t)((uint32_t)score ^ 0x80000000u) << 32) | (uint64_t)(~(uint32_t)j);
}

__device__ __forceinline__ uint64_t umax64(uint64_t a, uint64_t b) { return a > b ? a : b; }
__device__ __forceinline__ uint64_t umin64(uint64_t a, uint64_t b) { return a < b ? a : b; }

// the wave's LDS writes visible to its own later reads (and not moved across by the compiler)
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// 64 keys, one per lane, sorted in descending order across the wave (bitonic: lane t ends with rank t)
__device__ __forceinline__ uint64_t wave_sort_desc(uint64_t v, int lane) {
#pragma unroll
  for (int size = 2; size <= 64; size <<= 1)
#pragma unroll
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      const uint64_t o = __shfl_xor(v, stride);
      v = (((lane & size) == 0) == ((lane & stride) == 0)) ? umax64(v, o) : umin64(v, o);
    }
  return v;
}

// the 64 largest of a descending list and 64 candidates, descending
__device__ __forceinline__ uint64_t wave_merge_desc(uint64_t list, uint64_t c, int lane) {
  c = wave_sort_desc(c, lane);
  uint64_t v = umax64(list, __shfl_xor(c, 63));   // (descending against ascending: the larger halves, a bitonic sequence)
#pragma unroll
  for (int stride = 32; stride > 0; stride >>= 1) {
    const uint64_t o = __shfl_xor(v, stride);
    v = ((lane & stride) == 0) ? umax64(v, o) : umin64(v, o);
  }
  return v;
}

struct WaveTopk {
  uint64_t list;   // lane t: the rank-t key so far (0: empty)
  uint64_t bar;    // wave-uniform: the list's k-th key; a candidate must be larger
  int fill;        // keys waiting in buf
  int k, lane;
  uint64_t* buf;   // 128 keys of LDS, the wave's own

  __device__ __forceinline__ void merge(uint64_t c) {
    list = wave_merge_desc(list, c, lane);
    bar = __shfl(list, k - 1);
  }
  // one candidate per lane (0: none)
  __device__ __forceinline__ void push(uint64_t key) {
    const bool in = key > bar;
    const unsigned long long mask = __ballot(in);
    if (mask == 0) return;
    if (in) buf[fill + __popcll(mask & ((1ull << lane) - 1ull))] = key;
    fill += __popcll(mask);
    if (fill < 64) return;
    wave_lds_sync();
    const uint64_t c = buf[lane];
    const bool more = lane + 64 < fill;
    const uint64_t rest = more ? buf[lane + 64] : 0ull;
    wave_lds_sync();
    if (more) buf[lane] = rest;
    fill -= 64;
    merge(c);
  }
  __device__ __forceinline__ void flush() {
    if (fill == 0) return;
    wave_lds_sync();
    const uint64_t c = lane < fill ? buf[lane] : 0ull;
    wave_lds_sync();
    fill = 0;
    merge(c);
  }
};

// the band's pair index of cell (i, first column of row i)
__device__ __forceinline__ int64_t topk_row_base(const CrossTopkArgs& a, int64_t i) {
  return a.tri ? cross_tri_before(i, a.n) - a.tri0 : (i - a.r0) * a.n;
}

// the cells [lo, hi) of band row i (cell x = column c0 + x)
__device__ __forceinline__ void topk_row_cells(const CrossTopkArgs& a, WaveTopk& t, int64_t i, int64_t lo, int64_t hi) {
  const int64_t base = topk_row_base(a, i), c0 = a.tri ? i : 0;
  for (int64_t x0 = lo; x0 < hi; x0 += 64) {
    const int64_t x = x0 + t.lane, j = c0 + x;
    uint64_t key = 0;
    if (x < hi && a.status[base + x] == 0 && !(a.ava && j == i)) key = topk_key(a.score[base + x], j);
    t.push(key);
  }
}

// row pass: wave = (band row, chunk)
__global__ void __launch_bounds__(256) wfa_cross_topk_rows_kernel(CrossTopkArgs a) {
  __shared__ uint64_t bufs[4][128];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t w = (int64_t)blockIdx.x * 4 + wave;
  if (w >= (a.r1 - a.r0) * a.nch) return;
  const int64_t r = w / a.nch, c = w - r * a.nch, i = a.r0 + r;
  const int64_t len = a.n - (a.tri ? i : 0), lo = c * a.chunk;
  if (lo >= len) return;   // (a shorter row of a triangle band: no such chunk, the merge reads none)
  WaveTopk t{0ull, 0ull, 0, a.k, lane, bufs[wave]};
  topk_row_cells(a, t, i, lo, min(len, lo + a.chunk));
  t.flush();
  if (lane < a.k) a.part[w * a.k + lane] = t.list;
}

// merge: wave = target row (band rows; triangle: every row from r0 on)
__global__ void __launch_bounds__(256) wfa_cross_topk_merge_kernel(CrossTopkArgs a) {
  __shared__ uint64_t bufs[4][128];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t row = a.r0 + (int64_t)blockIdx.x * 4 + wave;
  if (row >= (a.tri ? a.n : a.r1)) return;
  uint64_t* run = a.run + row * a.k;
  WaveTopk t{lane < a.k ? run[lane] : 0ull, 0ull, 0, a.k, lane, bufs[wave]};
  t.bar = __shfl(t.list, a.k - 1);
  if (row < a.r1) {   // the row's own cells
    const int64_t len = a.n - (a.tri ? row : 0);
    if (a.nch > 0) {
      const uint64_t* p = a.part + (row - a.r0) * a.nch * a.k;
      const int64_t cnt = min(a.nch, (len + a.chunk - 1) / a.chunk) * a.k;
      for (int64_t x0 = 0; x0 < cnt; x0 += 64) t.push(x0 + lane < cnt ? p[x0 + lane] : 0ull);
    } else {
      topk_row_cells(a, t, row, 0, len);
    }
  }
  if (a.tri) {   // column `row` of the band's rows above it: cells (i, row), i < row, mirrored
    const int64_t iend = min(a.r1, row);
    for (int64_t i0 = a.r0; i0 < iend; i0 += 64) {
      const int64_t i = i0 + lane;
      uint64_t key = 0;
      if (i < iend) {
        const int64_t q = cross_tri_before(i, a.n) - a.tri0 + (row - i);
        if (a.status[q] == 0) key = topk_key(a.score[q], i);
      }
      t.push(key);
    }
  }
  t.flush();
  if (lane < a.k) run[lane] = t.list;
}

static unsigned cross_grid(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, (int64_t)1 << 16)); }

int launch_cross_gen(const CrossGenArgs& a, hipStream_t stream) {
  if (a.npairs <= 0) return 0;
  hipLaunchKernelGGL(wfa_cross_gen_kernel, dim3(cross_grid(a.npairs)), dim3(256), 0, stream, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_cross_scatter(const CrossResArgs& a, hipStream_t stream) {
  if (a.npairs <= 0) return 0;
  hipLaunchKernelGGL(wfa_cross_scatter_kernel, dim3(cross_grid(a.npairs)), dim3(256), 0, stream, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// a.blk_count holds (npairs + WFA_CROSS_CHUNK - 1) / WFA_CROSS_CHUNK words; a.out_* hold npairs entries
int launch_cross_compact(const CrossResArgs& a, hipStream_t stream) {
  if (a.npairs <= 0) return 0;
  const uint32_t nblk = (uint32_t)((a.npairs + WFA_CROSS_CHUNK - 1) / WFA_CROSS_CHUNK);
  hipLaunchKernelGGL(wfa_cross_count_kernel, dim3(nblk), dim3(256), 0, stream, a);
  hipLaunchKernelGGL(wfa_cross_scan_kernel, dim3(1), dim3(1024), 0, stream, a, nblk);
  hipLaunchKernelGGL(wfa_cross_write_kernel, dim3(nblk), dim3(256), 0, stream, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// a.part holds (r1 - r0) * nch * k keys when nch > 0; a.run holds k keys per row of the run
int launch_cross_topk(const CrossTopkArgs& a, hipStream_t stream) {
  if (a.r1 <= a.r0 || a.k < 1 || a.k > WFA_CROSS_MAX_K) return a.r1 <= a.r0 ? 0 : -1;
  if (a.nch > 0) {
    const int64_t waves = (a.r1 - a.r0) * a.nch;
    hipLaunchKernelGGL(wfa_cross_topk_rows_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, stream, a);
  }
  const int64_t rows = (a.tri ? a.n : a.r1) - a.r0;
  hipLaunchKernelGGL(wfa_cross_topk_merge_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace wfa
