// k_place.hip — placement of reads (wfa_place.hpp: rule, layout and the kernels' outline; wfa_hip_placer_* in wfa_hip.hip).
// Stores: the record kernels write out[q] for q < npairs (the host has grown the records to hold them); the count / scatter kernels
// touch count[i] only for i < nreads and order[slot] only for slot < nhits (the host has checked every i; the guards are here so
// that nothing a caller passes can move a store out of its array); the scan writes count[0 .. nreads] and bsum[chunk]; the place
// kernel writes row r < nreads and flags[h] for h < nhits read from order[]; the pair kernel writes row f < nfrag and pair_flags[h]
// for h < nhits read from order[], and reads rows / count only for mates inside [0, nreads).
#include <algorithm>
#define WFA_SUMMARY_SCAN_ONLY
#include "wfa_summary.hpp"   // (summary_scan: the walk that gives the summary's text_start / text_end)
#include "k_seed.hpp"        // (the workgroup sum and exclusive scan of the seed kernels)
#include "wfa_place.hpp"

namespace wfa {

__device__ inline PlaceHit place_hit_of(const PlaceRecordArgs& a, int64_t q, int32_t ts, int32_t te, int32_t clips) {
  PlaceHit h;
  h.i = a.i[q]; h.j = a.j[q]; h.reverse = (a.reverse && a.reverse[q]) ? 1 : 0; h.status = a.status[q];
  h.score = a.score[q]; h.ts = ts; h.te = te; h.clips = clips;
  return h;
}

__device__ inline void place_store(PlaceHit* dst, const PlaceHit& h) {
  int4* d = reinterpret_cast<int4*>(dst);
  d[0] = make_int4(h.i, h.j, h.reverse, h.status);
  d[1] = make_int4(h.score, h.ts, h.te, h.clips);
}

__device__ inline PlaceHit place_load(const PlaceHit* src) {
  const int4* s = reinterpret_cast<const int4*>(src);
  const int4 a = s[0], b = s[1];
  PlaceHit h;
  h.i = a.x; h.j = a.y; h.reverse = a.z; h.status = a.w; h.score = b.x; h.ts = b.y; h.te = b.z; h.clips = b.w;
  return h;
}

// scope full: the aligned core of the pair's op string, in text coordinates, and the pattern bases on either side of it
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
    const int32_t clips = zero || s.nm == 0 ? 0 : place_clip_word(s.head_p, s.tail_p);
    if (lane == 0) place_store(a.out + q, place_hit_of(a, q, t0 + (zero ? 0 : s.head_t), t0 + (zero ? 0 : tlen - s.tail_t), clips));
  }
}

// scope score: the whole text window
__global__ void __launch_bounds__(256) wfa_place_record_score_kernel(PlaceRecordArgs a) {
  const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < a.npairs; q += nthreads) {
    const int32_t t0 = a.t_start ? a.t_start[q] : 0;
    place_store(a.out + q, place_hit_of(a, q, t0, t0 + a.meta[q].tlen, 0));
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

// ---- the scan of n counters, in place (launch_place_scan: the group step's nreads + 1 counters, the rescue's 2 nfrag + 1) ----

// chunk sums of the counters
__global__ void __launch_bounds__(256) wfa_place_scan_reduce_kernel(const uint32_t* count, int64_t n, uint32_t* bsum) {
  __shared__ uint32_t s_red[4];
  const int64_t base = (int64_t)blockIdx.x * WFA_PLACE_SCAN_CHUNK + (int64_t)threadIdx.x * 16;
  uint32_t sum = 0;
#pragma unroll
  for (int u = 0; u < 16; ++u) sum += base + u < n ? count[base + u] : 0u;
  sum = seed_block_sum(sum, s_red);
  if (threadIdx.x == 0) bsum[blockIdx.x] = sum;
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

// every counter to the inclusive prefix over all of them (the group step: the END of its read's group)
__global__ void __launch_bounds__(256) wfa_place_scan_apply_kernel(uint32_t* count, int64_t n, const uint32_t* bsum) {
  __shared__ uint32_t s_red[4];
  const int64_t base = (int64_t)blockIdx.x * WFA_PLACE_SCAN_CHUNK + (int64_t)threadIdx.x * 16;
  uint32_t c[16];
  uint32_t sum = 0;
#pragma unroll
  for (int u = 0; u < 16; ++u) { c[u] = base + u < n ? count[base + u] : 0u; sum += c[u]; }
  uint32_t total;
  uint32_t run = bsum[blockIdx.x] + seed_block_exclusive(sum, s_red, &total);
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    run += c[u];
    if (base + u < n) count[base + u] = run;
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


// ---- pairing (wfa_place.hpp: "pair") ----

// SAME LOCUS of x against p, for x != p (the caller's test)
__device__ inline bool place_same_locus(const PlaceHit& x, const PlaceHit& p) {
  const int64_t ov = (int64_t)min(x.te, p.te) - (int64_t)max(x.ts, p.ts);
  const int64_t len_x = (int64_t)x.te - x.ts, len_p = (int64_t)p.te - p.ts;
  return x.j == p.j && x.reverse == p.reverse && ov > 0 && 2 * ov >= (len_x < len_p ? len_x : len_p);
}

// PROPER of a pairing of two eligible hits; *insert = te_R - ts_F
__device__ inline bool pair_proper(const PlaceHit& x, const PlaceHit& y, int32_t min_insert, int32_t max_insert, int64_t* insert) {
  if (x.j != y.j || x.reverse == y.reverse || x.te <= x.ts || y.te <= y.ts) return false;
  const PlaceHit& F = x.reverse ? y : x;
  const PlaceHit& R = x.reverse ? x : y;
  *insert = (int64_t)R.te - F.ts;
  return F.ts <= R.ts && F.te <= R.te && *insert >= min_insert && *insert <= max_insert;
}

// the slot pair (p / n2, p % n2) of a lane's p = lane, lane + 64, ...: one division per fragment
struct PairWalk {
  uint32_t s1, s2, q64, r64, n2;
  __device__ PairWalk(int lane, uint32_t n2_) : s1((uint32_t)lane / n2_), s2((uint32_t)lane % n2_), q64(64u / n2_), r64(64u % n2_), n2(n2_) {}
  __device__ void next() {
    s1 += q64; s2 += r64;
    if (s2 >= n2) { s2 -= n2; s1 += 1; }
  }
};

__device__ inline int32_t pair_saturate(int64_t v) {
  return (int32_t)(v < (int64_t)INT32_MIN + 1 ? (int64_t)INT32_MIN + 1 : v > (int64_t)INT32_MAX ? (int64_t)INT32_MAX : v);
}

#define WFA_PAIR_BIAS (1ll << 33)   // a pair score + the bias is positive: key 0 is "none"

__global__ void __launch_bounds__(256) wfa_pair_kernel(PairArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const PlaceArgs& P = a.place;
  const uint64_t nhits = (uint64_t)P.nhits;
  const int32_t min_score = P.min_score;
  for (int64_t f = wave; f < a.nfrag; f += nwaves) {
    const int64_t r1 = a.mate1 ? (int64_t)a.mate1[f] : 2 * f, r2 = a.mate2 ? (int64_t)a.mate2[f] : 2 * f + 1;
    if (r1 < 0 || r1 >= P.nreads || r2 < 0 || r2 >= P.nreads) continue;   // (wave-uniform; the host has checked the mates)
    const int32_t* se1 = P.rows + WFA_PLACE_COLS * r1;
    const int32_t* se2 = P.rows + WFA_PLACE_COLS * r2;
    const int32_t hit1 = se1[0], sc1 = se1[1], mq1 = se1[3], e1 = se1[4];
    const int32_t hit2 = se2[0], sc2 = se2[1], mq2 = se2[3], e2 = se2[4];
    const uint64_t beg1 = P.count[r1], stop1 = P.count[r1 + 1], end1 = stop1 < nhits ? stop1 : nhits;
    const uint64_t beg2 = P.count[r2], stop2 = P.count[r2 + 1], end2 = stop2 < nhits ? stop2 : nhits;
    const uint32_t n1 = end1 > beg1 ? (uint32_t)(end1 - beg1) : 0u, n2 = end2 > beg2 ? (uint32_t)(end2 - beg2) : 0u;
    const uint64_t total = (uint64_t)n1 * n2;
    const bool overflow = (int64_t)e1 * e2 > (int64_t)WFA_PAIR_MAX_PAIRINGS;
    const bool join = !overflow && e1 > 0 && e2 > 0 && total > 0;            // (wave-uniform)
    uint32_t pairings = 0, ch = ~0u, cg = ~0u;
    unsigned long long top = 0;
    if (join) {
      // pass 1: the proper pairings, and the best of them
      unsigned long long key = 0;
      uint32_t kh = ~0u, kg = ~0u;
      PairWalk w(lane, n2);
      for (uint64_t p = lane; p < total; p += 64) {
        const uint32_t h = P.order[beg1 + w.s1], g = P.order[beg2 + w.s2];
        w.next();
        if (h >= nhits || g >= nhits) continue;
        const PlaceHit x = place_load(P.hits + h);
        if (x.status != 0 || x.score < min_score) continue;
        const PlaceHit y = place_load(P.hits + g);
        if (y.status != 0 || y.score < min_score) continue;
        int64_t ins;
        if (!pair_proper(x, y, a.min_insert, a.max_insert, &ins)) continue;
        pairings += 1;
        const unsigned long long k = (unsigned long long)((int64_t)x.score + y.score + WFA_PAIR_BIAS);
        if (k > key || (k == key && (h < kh || (h == kh && g < kg)))) { key = k; kh = h; kg = g; }
      }
      pairings = seed_wave_sum(pairings);
      top = place_wave_max64(key);
      ch = seed_wave_min(top != 0 && key == top ? kh : ~0u);
      cg = seed_wave_min(top != 0 && key == top && kh == ch ? kg : ~0u);
    }
    int decided = 0;
    if (lane == 0 && top != 0) decided = (int64_t)top - WFA_PAIR_BIAS + a.unpaired >= (int64_t)sc1 + sc2 ? 1 : 0;
    const bool proper = __shfl(decided, 0) != 0 && ch < nhits && cg < nhits;
    int v;
    if (!proper) {
      switch (lane) {
        case 0: v = hit1; break; case 1: v = hit2; break; case 3: case 4: v = INT32_MIN; break; case 6: v = mq1; break;
        case 7: v = mq2; break; case 9: v = (int32_t)pairings; break; case 11: v = overflow ? 1 : 0; break; default: v = 0; break;
      }
    } else {
      const PlaceHit hc = place_load(P.hits + ch), gc = place_load(P.hits + cg);
      const int64_t best = (int64_t)top - WFA_PAIR_BIAS;
      // pass 2: every proper pairing against the chosen place
      uint32_t ties = 0, others = 0;
      unsigned long long sec = 0;
      PairWalk w(lane, n2);
      for (uint64_t p = lane; p < total; p += 64) {
        const uint32_t h = P.order[beg1 + w.s1], g = P.order[beg2 + w.s2];
        w.next();
        if (h >= nhits || g >= nhits) continue;
        const PlaceHit x = place_load(P.hits + h);
        if (x.status != 0 || x.score < min_score) continue;
        const PlaceHit y = place_load(P.hits + g);
        if (y.status != 0 || y.score < min_score) continue;
        int64_t ins;
        if (!pair_proper(x, y, a.min_insert, a.max_insert, &ins)) continue;
        if ((h == ch || place_same_locus(x, hc)) && (g == cg || place_same_locus(y, gc))) continue;
        const unsigned long long k = (unsigned long long)((int64_t)x.score + y.score + WFA_PAIR_BIAS);
        others += 1; ties += k == top ? 1u : 0u;
        sec = k > sec ? k : sec;
      }
      ties = seed_wave_sum(ties); others = seed_wave_sum(others);
      sec = place_wave_max64(sec);
      const int64_t second = (int64_t)sec - WFA_PAIR_BIAS;
      int32_t mapq = 60;
      if (others) {
        const int64_t q = 60 * (best - second) / P.full_gap;   // (best >= second: a floor division)
        mapq = (int32_t)(q < 60 ? q : 60);
      }
      const int32_t m1 = P.flags[ch] >= 2 ? max(mapq, mq1) : mapq, m2 = P.flags[cg] >= 2 ? max(mapq, mq2) : mapq;
      const int64_t insert = hc.reverse ? (int64_t)hc.te - gc.ts : (int64_t)gc.te - hc.ts;
      if (a.pair_flags) {
        for (uint64_t t = beg1 + lane; t < end1; t += 64) {
          const uint32_t h = P.order[t];
          if (h >= nhits) continue;
          const PlaceHit x = place_load(P.hits + h);
          a.pair_flags[h] = (x.status != 0 || x.score < min_score) ? 0 : h == ch ? 3 : place_same_locus(x, hc) ? 2 : 1;
        }
        for (uint64_t t = beg2 + lane; t < end2; t += 64) {
          const uint32_t g = P.order[t];
          if (g >= nhits) continue;
          const PlaceHit y = place_load(P.hits + g);
          a.pair_flags[g] = (y.status != 0 || y.score < min_score) ? 0 : g == cg ? 3 : place_same_locus(y, gc) ? 2 : 1;
        }
      }
      switch (lane) {
        case 0: v = (int32_t)ch; break; case 1: v = (int32_t)cg; break; case 2: v = 1; break; case 3: v = pair_saturate(best); break;
        case 4: v = others ? pair_saturate(second) : INT32_MIN; break; case 5: v = mapq; break; case 6: v = m1; break;
        case 7: v = m2; break; case 8: v = (int32_t)insert; break; case 9: v = (int32_t)pairings; break;
        case 10: v = (int32_t)ties; break; default: v = 0; break;
      }
    }
    if (lane < WFA_PAIR_COLS) a.pair_rows[WFA_PAIR_COLS * f + lane] = v;
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

// count[0 .. n) to its inclusive prefix sums in three passes; bsum holds ceil(n / WFA_PLACE_SCAN_CHUNK) words
int launch_place_scan(uint32_t* count, int64_t n, uint32_t* bsum, hipStream_t stream) {
  if (n <= 0) return 0;
  const unsigned chunks = (unsigned)((n + WFA_PLACE_SCAN_CHUNK - 1) / WFA_PLACE_SCAN_CHUNK);
  hipLaunchKernelGGL(wfa_place_scan_reduce_kernel, dim3(chunks), dim3(256), 0, stream, count, n, bsum);
  hipLaunchKernelGGL(wfa_place_scan_top_kernel, dim3(1), dim3(256), 0, stream, bsum, chunks);
  hipLaunchKernelGGL(wfa_place_scan_apply_kernel, dim3(chunks), dim3(256), 0, stream, count, n, bsum);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_place_group(const PlaceArgs& a, hipStream_t stream) {
  if (a.nhits > 0) hipLaunchKernelGGL(wfa_place_hits_kernel<false>, dim3(hits_grid(a.nhits)), dim3(256), 0, stream, a);
  if (launch_place_scan(a.count, a.nreads + 1, a.bsum, stream) != 0) return -1;
  if (a.nhits > 0) hipLaunchKernelGGL(wfa_place_hits_kernel<true>, dim3(hits_grid(a.nhits)), dim3(256), 0, stream, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_place(const PlaceArgs& a, int cu_count, hipStream_t stream) {
  if (a.nreads <= 0) return 0;
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((a.nreads + 3) / 4, (int64_t)cu_count * 16));
  hipLaunchKernelGGL(wfa_place_kernel, dim3(grid), dim3(256), 0, stream, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_pair(const PairArgs& a, int cu_count, hipStream_t stream) {
  if (a.nfrag <= 0) return 0;
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((a.nfrag + 3) / 4, (int64_t)cu_count * 16));
  hipLaunchKernelGGL(wfa_pair_kernel, dim3(grid), dim3(256), 0, stream, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace wfa
