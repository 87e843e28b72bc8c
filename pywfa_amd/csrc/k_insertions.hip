// k_insertions.hip — the reduction of a pileup's insertion log to one allele per reported row (wfa_insertions.hpp: the rule, the layout
// and the kernels' outline; k_select.hpp: the select's passes and the fill; wfa_hip_pileup_insertions in api_pileup.hip).
// Stores: the select kernels chunk_count[ch] / row `rank` of sel_g, bucket_size and rows for rank < nsel; fill a slot below its row's
// bucket size and below nrec; reduce and letters row `row` < nsel / < out_rows, letters below out_bases.  Every index read from the
// log is checked against the log's size before it is used.
#include "k_select.hpp"
#include "wfa_insertions.hpp"

namespace wfa {

// ---- select: the reported rows, in ascending global index; fill: every record of the log into the bucket of its row (k_select.hpp) ------
__global__ void __launch_bounds__(256) wfa_ins_select_count_kernel(CallsArgs a) {
  const int32_t* c6 = a.table + (int64_t)WFA_PILEUP_INS * a.total;
  select_count(a, [&](int64_t i) { int64_t depth; int32_t E; return event_flag(a, c6, i, &depth, &E); });
}

__global__ void __launch_bounds__(256) wfa_ins_select_kernel(InsArgs a) { event_select(a, a.c.table + (int64_t)WFA_PILEUP_INS * a.c.total); }

__global__ void __launch_bounds__(256) wfa_ins_fill_kernel(InsArgs a) {
  event_fill(a, [](int64_t r, const InsRecord&) { return r; });
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

int launch_ins_select_count(const InsArgs& a, hipStream_t stream) {
  if (a.c.chunks > 0) hipLaunchKernelGGL(wfa_ins_select_count_kernel, dim3(chunk_grid(a.c.chunks)), dim3(256), 0, stream, a.c);
  if (hipGetLastError() != hipSuccess) return -1;
  return launch_sites_scan(a.c, stream);
}

int launch_ins_select(const InsArgs& a, hipStream_t stream) {
  if (a.c.chunks <= 0 || a.nsel <= 0) return 0;
  hipLaunchKernelGGL(wfa_ins_select_kernel, dim3(chunk_grid(a.c.chunks)), dim3(256), 0, stream, a);
  if (hipGetLastError() != hipSuccess) return -1;
  return launch_scan64(a.bucket_size, 1, a.bucket_off, a.nsel, stream);
}

int launch_ins_reduce(const InsArgs& a, int64_t nbases, int cu_count, hipStream_t stream) {
  if (a.nsel <= 0) return 0;
  if (a.nrec > 0) hipLaunchKernelGGL(wfa_ins_fill_kernel, dim3(thread_grid(a.nrec, cu_count)), dim3(256), 0, stream, a);
  hipLaunchKernelGGL(wfa_ins_reduce_kernel, dim3(wave_grid(a.nsel, cu_count)), dim3(256), 0, stream, a, nbases);
  if (hipGetLastError() != hipSuccess) return -1;
  return launch_scan64(a.allele_len, 1, a.letter_off, a.nsel, stream);
}

int launch_ins_letters(const InsArgs& a, int64_t out_rows, int64_t out_bases, int cu_count, hipStream_t stream) {
  if (out_rows <= 0 || out_bases <= 0) return 0;
  hipLaunchKernelGGL(wfa_ins_letters_kernel, dim3(wave_grid(out_rows, cu_count)), dim3(256), 0, stream, a, out_rows, out_bases);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace wfa
