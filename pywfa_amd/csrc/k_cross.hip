// k_cross.hip — translation unit of the cross-product kernels (wfa_cross.hpp): band generator, scatter into the dense matrix, ordered
// compaction of the completed pairs.  Every result is written by vector stores from the thread that owns it.
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

}  // namespace wfa
