// k_insertions.hip — the reduction of a pileup's insertion log to one allele per reported row, and the 64-bit scan both sides of the
// log use (wfa_insertions.hpp: the rule, the layout and the kernels' outline; wfa_hip_pileup_insertions in api_pileup.hip).
// Stores: the scan out[i] for i <= n; the select kernels chunk_count[ch] / row `rank` of sel_g, bucket_size and rows for rank < nsel;
// fill a slot below its row's bucket size; reduce and letters row `row` < nsel / < out_rows, letters below out_bases.  Every index
// read from the log is checked against the log's size before it is used.
#include <algorithm>
#include "k_seed.hpp"   // (the workgroup sum of the seed kernels)
#include "wfa_insertions.hpp"

namespace wfa {

// ---- exclusive 64-bit scan of 32-bit values: one workgroup, 2 048 values per round (8 per thread) ---------------------------------------
__global__ void __launch_bounds__(256) wfa_ins_scan_kernel(const uint32_t* in, int stride, uint64_t* out, int64_t n) {
  __shared__ uint64_t s_red[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint64_t carry = 0;
  for (int64_t b0 = 0; b0 < n; b0 += 2048) {
    const int64_t i0 = b0 + (int64_t)threadIdx.x * 8;
    uint32_t v[8];
    uint64_t mine = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) { v[k] = i0 + k < n ? in[(i0 + k) * stride] : 0u; mine += v[k]; }
    unsigned long long inc = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const unsigned long long u = __shfl_up(inc, off);
      if (lane >= off) inc += u;
    }
    if (lane == 63) s_red[wave] = inc;
    __syncthreads();
    uint64_t before = 0;
    for (int w = 0; w < wave; ++w) before += s_red[w];
    const uint64_t total = s_red[0] + s_red[1] + s_red[2] + s_red[3];
    __syncthreads();
    uint64_t run = carry + before + inc - mine;
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (i0 + k < n) { out[i0 + k] = run; run += v[k]; }
    carry += total;
  }
  if (threadIdx.x == 0) out[n] = carry;
}

int launch_ins_scan(const uint32_t* in, int stride, uint64_t* out, int64_t n, hipStream_t stream) {
  hipLaunchKernelGGL(wfa_ins_scan_kernel, dim3(1), dim3(256), 0, stream, in, stride, out, std::max<int64_t>(n, 0));
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---- select: the reported rows, in ascending global index ---------------------------------------------------------------------------------
// whether base i of the run is a reported row (false behind the run's end); its depth and c6
__device__ inline bool ins_flag(const CallsArgs& a, int64_t i, int64_t* depth, int32_t* c6) {
  if (i >= a.n) return false;
  const int64_t g = a.g0 + i;
  int64_t d = 0;
#pragma unroll
  for (int x = 0; x < 6; ++x) d += a.table[(int64_t)x * a.total + g];
  *depth = d;
  *c6 = a.table[(int64_t)WFA_PILEUP_INS * a.total + g];
  return ins_selected(d, *c6, a.min_depth, a.min_permille);
}

__global__ void __launch_bounds__(256) wfa_ins_select_count_kernel(CallsArgs a) {
  __shared__ uint32_t s_red[4];
  for (int64_t ch = blockIdx.x; ch < a.chunks; ch += gridDim.x) {
    const int64_t i0 = ch * a.chunk;
    uint32_t mine = 0;   // the rows of this wave's rounds (the same in every lane)
    for (int64_t t = threadIdx.x; t < a.chunk; t += 256) {
      int64_t depth; int32_t c6;
      mine += (uint32_t)__builtin_popcountll(__ballot(ins_flag(a, i0 + t, &depth, &c6)));
    }
    const uint32_t sum = seed_block_sum((threadIdx.x & 63) == 0 ? mine : 0u, s_red);
    if (threadIdx.x == 0) a.chunk_count[ch] = sum;
  }
}

__global__ void __launch_bounds__(256) wfa_ins_select_kernel(InsArgs a) {
  __shared__ uint32_t s_red[4];
  const CallsArgs& c = a.c;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long lower = (1ull << lane) - 1ull;
  for (int64_t ch = blockIdx.x; ch < c.chunks; ch += gridDim.x) {
    uint64_t run = c.chunk_off[ch];
    if (c.chunk_off[ch + 1] == run) continue;   // (uniform over the workgroup)
    const int64_t i0 = ch * c.chunk;
    for (int64_t t0 = 0; t0 < c.chunk; t0 += 256) {
      const int64_t i = i0 + t0 + threadIdx.x;
      int64_t depth = 0; int32_t c6 = 0;
      const bool sel = t0 + threadIdx.x < c.chunk && ins_flag(c, i, &depth, &c6);
      const unsigned long long m = __ballot(sel);
      if (lane == 0) s_red[wave] = (uint32_t)__builtin_popcountll(m);
      __syncthreads();
      uint32_t before = 0;
      for (int w = 0; w < wave; ++w) before += s_red[w];
      const uint32_t total = s_red[0] + s_red[1] + s_red[2] + s_red[3];
      __syncthreads();
      const uint64_t rank = run + before + (uint32_t)__builtin_popcountll(m & lower);
      run += total;
      if (!sel || rank >= (uint64_t)a.nsel) continue;
      const int64_t g = c.g0 + i;
      int64_t lo = 0, hi = c.nseq;   // the first sequence that starts behind g; its predecessor owns g
      while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (c.seq_off[mid] > g) hi = mid; else lo = mid + 1; }
      const int64_t j = lo - 1;
      const bool overflow = c6 > a.max_reads;
      a.sel_g[rank] = g;
      a.bucket_size[rank] = overflow ? 0u : (uint32_t)c6;
      int4* row = reinterpret_cast<int4*>(a.rows + rank * WFA_INSERTION_COLS);
      row[0] = make_int4((int32_t)j, (int32_t)(g - c.seq_off[j]), (int32_t)depth, c6);
      row[1] = make_int4(0, 0, 0, overflow ? 1 : 0);
    }
  }
}

// ---- fill: every record of the log into the bucket of its row ----------------------------------------------------------------------------
__global__ void __launch_bounds__(256) wfa_ins_fill_kernel(InsArgs a) {
  const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < a.nrec; r += nthreads) {
    const int64_t g = a.records[r].g;
    if (g < a.c.g0 || g >= a.c.g0 + a.c.n) continue;
    int64_t lo = 0, hi = a.nsel;   // the first selected row at or behind g
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (a.sel_g[mid] < g) lo = mid + 1; else hi = mid; }
    if (lo >= a.nsel || a.sel_g[lo] != g) continue;
    const uint32_t size = a.bucket_size[lo];
    if (size == 0) continue;
    const uint32_t slot = atomicAdd(a.bucket_fill + lo, 1u);
    if (slot < size && a.bucket_off[lo] + slot < (uint64_t)a.nrec) a.bucket[a.bucket_off[lo] + slot] = r;   // (the buckets are sized from c6, the array from the log)
  }
}

// ---- reduce: a wave per row ----------------------------------------------------------------------------------------------------------------
// a record's length, 0 for one whose letters would leave the log
__device__ inline int32_t ins_len(const InsArgs& a, const InsRecord& r, int64_t nbases) {
  return (r.n > 0 && r.off >= 0 && r.off + r.n <= nbases) ? r.n : 0;
}

// (n, letters) of x against y: negative, 0, positive
__device__ inline int ins_compare(const uint8_t* bases, int64_t xo, int32_t xn, int64_t yo, int32_t yn) {
  if (xn != yn) return xn < yn ? -1 : 1;
  for (int32_t k = 0; k < xn; ++k) {
    const int d = (int)bases[xo + k] - (int)bases[yo + k];
    if (d) return d;
  }
  return 0;
}

__global__ void __launch_bounds__(256) wfa_ins_reduce_kernel(InsArgs a, int64_t nbases) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t row = wave; row < a.nsel; row += nwaves) {
    const uint64_t room = a.bucket_off[row] < (uint64_t)a.nrec ? (uint64_t)a.nrec - a.bucket_off[row] : 0;
    const uint32_t m = (uint32_t)min((uint64_t)min(a.bucket_fill[row], a.bucket_size[row]), room);   // the slots that were written
    const int64_t* bucket = a.bucket + a.bucket_off[row];
    uint32_t best_count = 0, distinct = 0;
    long long best = -1;
    int64_t best_off = 0; int32_t best_n = 0;
    for (uint32_t t = lane; t < m; t += 64) {
      const int64_t r = bucket[t];
      const InsRecord x = a.records[r];
      const int32_t xn = ins_len(a, x, nbases);
      uint32_t count = 0;
      bool first_slot = true;
      for (uint32_t s = 0; s < m; ++s) {
        const InsRecord y = a.records[bucket[s]];
        if (ins_compare(a.bases, x.off, xn, y.off, ins_len(a, y, nbases)) == 0) { ++count; if (s < t) first_slot = false; }
      }
      distinct += first_slot ? 1u : 0u;
      if (count > best_count || (count == best_count && ins_compare(a.bases, x.off, xn, best_off, best_n) < 0)) {
        best_count = count; best = r; best_off = x.off; best_n = xn;
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const uint32_t oc = __shfl_xor(best_count, off);
      const long long ob = __shfl_xor(best, off);
      const long long oo = __shfl_xor((long long)best_off, off);
      const int32_t on = __shfl_xor(best_n, off);
      if (oc > best_count || (oc == best_count && oc > 0 && ins_compare(a.bases, oo, on, best_off, best_n) < 0)) {
        best_count = oc; best = ob; best_off = oo; best_n = on;
      }
      distinct += __shfl_xor(distinct, off);
    }
    if (lane == 0) {
      int32_t* out = a.rows + row * WFA_INSERTION_COLS;
      out[4] = (int32_t)best_count; out[5] = best_n; out[6] = (int32_t)distinct;
      a.best[row] = best;
      a.allele_len[row] = (uint32_t)best_n;
    }
  }
}

__global__ void __launch_bounds__(256) wfa_ins_letters_kernel(InsArgs a, int64_t out_rows, int64_t out_bases) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t row = wave; row < out_rows; row += nwaves) {
    const int64_t r = a.best[row];
    const int64_t n = a.allele_len[row], at = (int64_t)a.letter_off[row];
    if (r < 0 || at + n > out_bases) continue;
    const int64_t from = a.records[r].off;
    for (int64_t k = lane; k < n; k += 64) {
      const uint32_t col = a.bases[from + k];
      a.letters[at + k] = (uint8_t)(col == 0 ? 'A' : col == 1 ? 'C' : col == 2 ? 'G' : col == 3 ? 'T' : 'N');
    }
  }
}

static unsigned chunk_grid(int64_t chunks) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(chunks, 1 << 16)); }
static unsigned wave_grid(int64_t waves, int cu_count) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((waves + 3) / 4, (int64_t)cu_count * 16)); }

int launch_ins_select_count(const InsArgs& a, hipStream_t stream) {
  if (a.c.chunks > 0) hipLaunchKernelGGL(wfa_ins_select_count_kernel, dim3(chunk_grid(a.c.chunks)), dim3(256), 0, stream, a.c);
  if (hipGetLastError() != hipSuccess) return -1;
  return launch_sites_scan(a.c, stream);
}

int launch_ins_select(const InsArgs& a, hipStream_t stream) {
  if (a.c.chunks <= 0 || a.nsel <= 0) return 0;
  hipLaunchKernelGGL(wfa_ins_select_kernel, dim3(chunk_grid(a.c.chunks)), dim3(256), 0, stream, a);
  if (hipGetLastError() != hipSuccess) return -1;
  return launch_ins_scan(a.bucket_size, 1, a.bucket_off, a.nsel, stream);
}

int launch_ins_reduce(const InsArgs& a, int64_t nbases, int cu_count, hipStream_t stream) {
  if (a.nsel <= 0) return 0;
  if (a.nrec > 0) {
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((a.nrec + 255) / 256, (int64_t)cu_count * 32));
    hipLaunchKernelGGL(wfa_ins_fill_kernel, dim3(grid), dim3(256), 0, stream, a);
  }
  hipLaunchKernelGGL(wfa_ins_reduce_kernel, dim3(wave_grid(a.nsel, cu_count)), dim3(256), 0, stream, a, nbases);
  if (hipGetLastError() != hipSuccess) return -1;
  return launch_ins_scan(a.allele_len, 1, a.letter_off, a.nsel, stream);
}

int launch_ins_letters(const InsArgs& a, int64_t out_rows, int64_t out_bases, int cu_count, hipStream_t stream) {
  if (out_rows <= 0 || out_bases <= 0) return 0;
  hipLaunchKernelGGL(wfa_ins_letters_kernel, dim3(wave_grid(out_rows, cu_count)), dim3(256), 0, stream, a, out_rows, out_bases);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace wfa
