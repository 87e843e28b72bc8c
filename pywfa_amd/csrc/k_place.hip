// k_place.hip — placement of reads (wfa_place.hpp: rule, layout and the kernels' outline; wfa_hip_placer_* in wfa_hip.hip).
// Stores: the record kernels write out[q] for q < npairs (the host has grown the records to hold them); the count / scatter kernels
// touch count[i] only for i < nreads and order[slot] only for slot < nhits (the host has checked every i; the guards are here so
// that nothing a caller passes can move a store out of its array); the scan writes count[0 .. nreads] and bsum[chunk]; the place
// kernel writes row r < nreads and flags[h] for h < nhits read from order[].
#include <algorithm>
#define WFA_SUMMARY_SCAN_ONLY
#include "wfa_summary.hpp"   // (summary_scan: the walk that gives the summary's text_start / text_end)
#include "k_seed.hpp"        // (the workgroup sum and exclusive scan of the seed kernels)
#include "wfa_place.hpp"

namespace wfa {

__device__ inline PlaceHit place_hit_of(const PlaceRecordArgs& a, int64_t q, int32_t ts, int32_t te) {
  PlaceHit h;
  h.i = a.i[q]; h.j = a.j[q]; h.reverse = (a.reverse && a.reverse[q]) ? 1 : 0; h.status = a.status[q];
  h.score = a.score[q]; h.ts = ts; h.te = te; h.spare = 0;
  return h;
}

__device__ inline void place_store(PlaceHit* dst, const PlaceHit& h) {
  int4* d = reinterpret_cast<int4*>(dst);
  d[0] = make_int4(h.i, h.j, h.reverse, h.status);
  d[1] = make_int4(h.score, h.ts, h.te, h.spare);
}

__device__ inline PlaceHit place_load(const PlaceHit* src) {
  const int4* s = reinterpret_cast<const int4*>(src);
  const int4 a = s[0], b = s[1];
  PlaceHit h;
  h.i = a.x; h.j = a.y; h.reverse = a.z; h.status = a.w; h.score = b.x; h.ts = b.y; h.te = b.z; h.spare = b.w;
  return h;
}

// scope full: the aligned core of the pair's op string, in text coordinates
__global__ void __launch_bounds__(256) wfa_place_record_full_kernel(PlaceRecordArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t q = wave; q < a.npairs; q += nwaves) {
    const int len = a.cigar_len[q];
    const int plen = a.meta[q].plen, tlen = a.meta[q].tlen;
    const SummaryScan s = summary_scan(a.ops + a.cigar_begin[q], len, lane);
    const bool zero = (len == 0) || plen == 0 || tlen == 0;
    const int32_t t0 = a.t_start ? a.t_start[q] : 0;
    if (lane == 0) place_store(a.out + q, place_hit_of(a, q, t0 + (zero ? 0 : s.head_t), t0 + (zero ? 0 : tlen - s.tail_t)));
  }
}

// scope score: the whole text window
__global__ void __launch_bounds__(256) wfa_place_record_score_kernel(PlaceRecordArgs a) {
  const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < a.npairs; q += nthreads) {
    const int32_t t0 = a.t_start ? a.t_start[q] : 0;
    place_store(a.out + q, place_hit_of(a, q, t0, t0 + a.meta[q].tlen));
  }
}

template <bool SCATTER>
__global__ void __launch_bounds__(256) wfa_place_hits_kernel(PlaceArgs a) {
  const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  for (int64_t h = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; h < a.nhits; h += nthreads) {
    const int32_t i = a.hits[h].i;
    if (i < 0 || i >= a.nreads) continue;
    if (!SCATTER) {
      atomicAdd(&a.count[i], 1u);
    } else {
      const uint32_t slot = atomicSub(&a.count[i], 1u) - 1u;
      if (slot < (uint64_t)a.nhits) a.order[slot] = (uint32_t)h;
    }
  }
}

// chunk sums of the counters
__global__ void __launch_bounds__(256) wfa_place_scan_reduce_kernel(PlaceArgs a) {
  __shared__ uint32_t s_red[4];
  const int64_t n = a.nreads + 1;
  const int64_t base = (int64_t)blockIdx.x * WFA_PLACE_SCAN_CHUNK + (int64_t)threadIdx.x * 16;
  uint32_t sum = 0;
#pragma unroll
  for (int u = 0; u < 16; ++u) sum += base + u < n ? a.count[base + u] : 0u;
  sum = seed_block_sum(sum, s_red);
  if (threadIdx.x == 0) a.bsum[blockIdx.x] = sum;
}

// the chunk sums to their exclusive prefix, in place: one workgroup, 256 sums per round
__global__ void __launch_bounds__(256) wfa_place_scan_top_kernel(uint32_t* bsum, uint32_t chunks) {
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

// every counter to the inclusive prefix over all of them: the END of its read's group
__global__ void __launch_bounds__(256) wfa_place_scan_apply_kernel(PlaceArgs a) {
  __shared__ uint32_t s_red[4];
  const int64_t n = a.nreads + 1;
  const int64_t base = (int64_t)blockIdx.x * WFA_PLACE_SCAN_CHUNK + (int64_t)threadIdx.x * 16;
  uint32_t c[16];
  uint32_t sum = 0;
#pragma unroll
  for (int u = 0; u < 16; ++u) { c[u] = base + u < n ? a.count[base + u] : 0u; sum += c[u]; }
  uint32_t total;
  uint32_t run = a.bsum[blockIdx.x] + seed_block_exclusive(sum, s_red, &total);
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    run += c[u];
    if (base + u < n) a.count[base + u] = run;
  }
}

__device__ inline unsigned long long place_wave_max64(unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t lo = __shfl_xor((uint32_t)v, off), hi = __shfl_xor((uint32_t)(v >> 32), off);
    const unsigned long long u = ((unsigned long long)hi << 32) | lo;
    v = u > v ? u : v;
  }
  return v;
}
__device__ inline int32_t place_wave_max32(int32_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off));
  return v;
}

__global__ void __launch_bounds__(256) wfa_place_kernel(PlaceArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const uint64_t nhits = (uint64_t)a.nhits;
  for (int64_t r = wave; r < a.nreads; r += nwaves) {
    const uint64_t beg = a.count[r], stop = a.count[r + 1], end = stop < nhits ? stop : nhits;
    // pass 1: the primary
    unsigned long long key = 0;
    for (uint64_t t = beg + lane; t < end; t += 64) {
      const uint32_t h = a.order[t];
      if (h >= nhits) continue;
      const PlaceHit x = place_load(a.hits + h);
      if (x.status != 0 || x.score < a.min_score) continue;
      const unsigned long long k = ((unsigned long long)((uint32_t)x.score ^ 0x80000000u) << 32) | (uint32_t)~h;
      key = k > key ? k : key;
    }
    key = place_wave_max64(key);
    int v;
    if (key == 0) {   // no eligible hit: the flags of the group are all 0
      for (uint64_t t = beg + lane; t < end; t += 64) {
        const uint32_t h = a.order[t];
        if (a.flags && h < nhits) a.flags[h] = 0;
      }
      v = lane == 0 ? -1 : (lane == 1 || lane == 2) ? INT32_MIN : 0;
    } else {
      const uint32_t p = ~(uint32_t)key;
      const PlaceHit hp = place_load(a.hits + p);
      const int64_t len_p = (int64_t)hp.te - hp.ts;
      // pass 2: every hit against the primary
      uint32_t hits = 0, ties = 0, others = 0;
      int32_t second = INT32_MIN;
      for (uint64_t t = beg + lane; t < end; t += 64) {
        const uint32_t h = a.order[t];
        if (h >= nhits) continue;
        const PlaceHit x = place_load(a.hits + h);
        uint8_t flag = 0;
        if (x.status == 0 && x.score >= a.min_score) {
          hits += 1;
          if (h == p) {
            flag = 3;
          } else {
            const int64_t ov = (int64_t)min(x.te, hp.te) - (int64_t)max(x.ts, hp.ts);
            const int64_t len_h = (int64_t)x.te - x.ts;
            const bool same = x.j == hp.j && x.reverse == hp.reverse && ov > 0 && 2 * ov >= (len_h < len_p ? len_h : len_p);
            flag = same ? 2 : 1;
            if (!same) { others += 1; second = max(second, x.score); ties += x.score == hp.score ? 1u : 0u; }
          }
        }
        if (a.flags) a.flags[h] = flag;
      }
      hits = seed_wave_sum(hits); ties = seed_wave_sum(ties); others = seed_wave_sum(others);
      second = place_wave_max32(second);
      int32_t mapq = 60;
      if (others) {
        const int64_t q = 60 * ((int64_t)hp.score - second) / a.full_gap;   // (score_p >= second: a floor division)
        mapq = (int32_t)(q < 60 ? q : 60);
      }
      switch (lane) {
        case 0: v = (int32_t)p; break; case 1: v = hp.score; break; case 2: v = second; break; case 3: v = mapq; break;
        case 4: v = (int32_t)hits; break; case 5: v = (int32_t)ties; break; case 6: v = hp.ts; break; case 7: v = hp.te; break;
        default: v = 0; break;
      }
    }
    if (lane < WFA_PLACE_COLS) a.rows[WFA_PLACE_COLS * r + lane] = v;
  }
}

int launch_place_record(const PlaceRecordArgs& a, bool full, int cu_count, hipStream_t stream) {
  if (a.npairs <= 0) return 0;
  if (full) {
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((a.npairs + 3) / 4, (int64_t)cu_count * 16));
    hipLaunchKernelGGL(wfa_place_record_full_kernel, dim3(grid), dim3(256), 0, stream, a);
  } else {
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((a.npairs + 255) / 256, (int64_t)cu_count * 8));
    hipLaunchKernelGGL(wfa_place_record_score_kernel, dim3(grid), dim3(256), 0, stream, a);
  }
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

static unsigned hits_grid(int64_t nhits) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((nhits + 255) / 256, 1 << 16)); }

int launch_place_group(const PlaceArgs& a, hipStream_t stream) {
  const unsigned chunks = (unsigned)((a.nreads + 1 + WFA_PLACE_SCAN_CHUNK - 1) / WFA_PLACE_SCAN_CHUNK);
  if (a.nhits > 0) hipLaunchKernelGGL(wfa_place_hits_kernel<false>, dim3(hits_grid(a.nhits)), dim3(256), 0, stream, a);
  hipLaunchKernelGGL(wfa_place_scan_reduce_kernel, dim3(chunks), dim3(256), 0, stream, a);
  hipLaunchKernelGGL(wfa_place_scan_top_kernel, dim3(1), dim3(256), 0, stream, a.bsum, chunks);
  hipLaunchKernelGGL(wfa_place_scan_apply_kernel, dim3(chunks), dim3(256), 0, stream, a);
  if (a.nhits > 0) hipLaunchKernelGGL(wfa_place_hits_kernel<true>, dim3(hits_grid(a.nhits)), dim3(256), 0, stream, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_place(const PlaceArgs& a, int cu_count, hipStream_t stream) {
  if (a.nreads <= 0) return 0;
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((a.nreads + 3) / 4, (int64_t)cu_count * 16));
  hipLaunchKernelGGL(wfa_place_kernel, dim3(grid), dim3(256), 0, stream, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace wfa
