// k_dup.hip — duplicate marking after placement (wfa_dup.hpp: rule, layout and the kernels' outline; wfa_hip_placer_duplicates in
// api_place.hip).
// Stores: qsum writes qsum[r] only for r < nreads, and loads the bytes [off[r], off[r] + len[r]) of the quality set and no other (the host
// has checked that the set covers the reads); key writes owned[r], rec[r] and read_rows row r only for r < nreads, frag_rows row f for f < nfrag, and adds to plane[bucket]
// only for 0 <= bucket < nbases; the scan writes plane[0 .. nbases] and bsum[chunk]; scatter subtracts from plane[bucket] under the same
// guard and writes sorted[slot] only for slot < nreads; resolve writes the rows of units and mates inside [0, nfrag) and [0, nreads).
// Loads are guarded the way the pair and rescue kernels guard them: a mate outside [0, nreads), a hit number outside [0, nhits) or a
// text outside the text set makes no unit (the host has checked all three; the guards are here so that nothing a caller passes can
// move an access out of its array), and resolve clamps a bucket's range to the records in use.
#include <algorithm>
#include "wfa_dup.hpp"

namespace wfa {

__device__ inline void dup_store_row(int32_t* rows, int64_t at, int32_t rep, int32_t size, int32_t dup, int32_t overflow) {
  *reinterpret_cast<int4*>(rows + WFA_DUP_COLS * at) = make_int4(rep, size, dup, overflow);
}

__device__ inline void dup_store_unit(DupUnit* dst, const DupUnit& u) {
  int4* d = reinterpret_cast<int4*>(dst);
  d[0] = make_int4((int32_t)(uint32_t)((uint64_t)u.bucket & 0xffffffffull), (int32_t)(uint32_t)((uint64_t)u.bucket >> 32), u.kind, u.end);
  d[1] = make_int4(u.score, u.unit, u.m1, u.m2);
}

__device__ inline DupUnit dup_load_unit(const DupUnit* src) {
  const int4* s = reinterpret_cast<const int4*>(src);
  const int4 a = s[0], b = s[1];
  DupUnit u;
  u.bucket = (int64_t)(((uint64_t)(uint32_t)a.y << 32) | (uint32_t)a.x);
  u.kind = a.z; u.end = a.w; u.score = b.x; u.unit = b.y; u.m1 = b.z; u.m2 = b.w;
  return u;
}

__device__ inline DupUnit dup_no_unit() {
  DupUnit u;
  u.bucket = 0; u.kind = 0; u.end = 0; u.score = 0; u.unit = -1; u.m1 = -1; u.m2 = -1;
  return u;
}

// the bucket of position b on text j, or -1: b outside the text (or j outside the set)
__device__ inline int64_t dup_bucket(const DupArgs& a, int32_t j, int64_t b) {
  if (j < 0 || (int64_t)j >= a.ntexts || b < 0 || b >= (int64_t)a.text_len[j]) return -1;
  const int64_t at = a.boff[j] + b;
  return at >= 0 && at < a.nbases ? at : -1;
}

// the unclipped start and end of a record (its clip word: wfa_place.hpp), 64-bit
__device__ inline int64_t dup_start(const DupArgs& a, const int4& h1) {
  return (int64_t)h1.y - ((a.flags & WFA_DUP_UNCLIPPED) ? place_clip_lead(h1.w) : 0);
}
__device__ inline int64_t dup_end(const DupArgs& a, const int4& h1) {
  return (int64_t)h1.z + ((a.flags & WFA_DUP_UNCLIPPED) ? place_clip_trail(h1.w) : 0);
}

__global__ void __launch_bounds__(256) wfa_dup_key_fragments_kernel(DupArgs a) {
  const PairArgs& A = a.pair;
  const PlaceArgs& P = A.place;
  const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  for (int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; f < A.nfrag; f += nthreads) {
    const int4 pr = *reinterpret_cast<const int4*>(A.pair_rows + WFA_PAIR_COLS * f);   // hit1, hit2, proper, score
    const int64_t r1 = A.mate1 ? (int64_t)A.mate1[f] : 2 * f, r2 = A.mate2 ? (int64_t)A.mate2[f] : 2 * f + 1;
    const bool inside = r1 >= 0 && r1 < P.nreads && r2 >= 0 && r2 < P.nreads && r1 != r2;
    if (!inside || pr.z != 1 || pr.x < 0 || (int64_t)pr.x >= P.nhits || pr.y < 0 || (int64_t)pr.y >= P.nhits) {
      dup_store_row(a.frag_rows, f, -1, 0, 0, 0);
      continue;
    }
    a.owned[r1] = 1; a.owned[r2] = 2;
    const int4* h = reinterpret_cast<const int4*>(P.hits + pr.x);
    const int4* g = reinterpret_cast<const int4*>(P.hits + pr.y);
    const int4 h0 = h[0], h1 = h[1], g1 = g[1];   // i, j, reverse, status | score, ts, te, clips
    const bool h_fwd = h0.z == 0;
    DupUnit u;
    const int64_t end = dup_end(a, h_fwd ? g1 : h1);   // te_R, or ue_R
    u.kind = h_fwd ? 1 : 2; u.end = 0; u.score = pr.w; u.unit = (int32_t)f; u.m1 = (int32_t)r1; u.m2 = (int32_t)r2;
    if (a.flags & WFA_DUP_BY_QUALITY) {
      const int64_t q = (int64_t)a.qsum[r1] + a.qsum[r2];
      u.score = (int32_t)(q > (int64_t)INT32_MAX ? (int64_t)INT32_MAX : q);
    }
    u.bucket = end > (int64_t)INT32_MAX ? -1 : dup_bucket(a, h0.y, dup_start(a, h_fwd ? h1 : g1));
    if (u.bucket < 0) {   // b outside the text (or an end beyond int32): alone, and its mates follow it
      dup_store_row(a.frag_rows, f, (int32_t)f, 1, 0, 0);
      dup_store_row(a.read_rows, r1, -1, 0, 0, 0);
      dup_store_row(a.read_rows, r2, -1, 0, 0, 0);
      dup_store_unit(a.rec + r1, dup_no_unit());
      continue;
    }
    u.end = (int32_t)end;   // (it fits: the test above)
    dup_store_unit(a.rec + r1, u);
    atomicAdd(&a.plane[u.bucket], 1u);
  }
}

__global__ void __launch_bounds__(256) wfa_dup_key_reads_kernel(DupArgs a) {
  const PlaceArgs& P = a.pair.place;
  const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < P.nreads; r += nthreads) {
    const uint8_t own = a.owned[r];
    if (own == 1) continue;                                            // the slot holds its fragment's record
    if (own != 0) { dup_store_unit(a.rec + r, dup_no_unit()); continue; }   // mate 2 of a pair unit: its row comes from the fragment
    const int4* se = reinterpret_cast<const int4*>(P.rows + WFA_PLACE_COLS * r);
    const int4 s0 = se[0], s1 = se[1];   // hit, score, second, mapq | hits, ties, text_start, text_end
    if (s0.x < 0 || (int64_t)s0.x >= P.nhits || s1.w <= s1.z) {
      dup_store_row(a.read_rows, r, -1, 0, 0, 0);
      dup_store_unit(a.rec + r, dup_no_unit());
      continue;
    }
    const int4* hp = reinterpret_cast<const int4*>(P.hits + s0.x);
    const int4 h0 = hp[0];   // i, j, reverse, status
    const bool rev = h0.z != 0;
    DupUnit u;
    u.kind = rev ? 4 : 3; u.end = 0; u.score = (a.flags & WFA_DUP_BY_QUALITY) ? a.qsum[r] : s0.y; u.unit = (int32_t)r; u.m1 = -1; u.m2 = -1;
    int64_t p5 = rev ? (int64_t)s1.w - 1 : (int64_t)s1.z;
    if (a.flags & WFA_DUP_UNCLIPPED) {   // (the row's interval is the primary's: the clip word comes from its record)
      const int4 h1 = hp[1];             // score, ts, te, clips
      p5 = rev ? dup_end(a, h1) - 1 : dup_start(a, h1);
    }
    u.bucket = dup_bucket(a, h0.y, p5);
    if (u.bucket < 0) {
      dup_store_row(a.read_rows, r, (int32_t)r, 1, 0, 0);
      dup_store_unit(a.rec + r, dup_no_unit());
      continue;
    }
    dup_store_unit(a.rec + r, u);
    atomicAdd(&a.plane[u.bucket], 1u);
  }
}

__global__ void __launch_bounds__(256) wfa_dup_scatter_kernel(DupArgs a) {
  const int64_t nreads = a.pair.place.nreads;
  const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < nreads; r += nthreads) {
    const DupUnit u = dup_load_unit(a.rec + r);
    if (u.kind == 0 || u.bucket < 0 || u.bucket >= a.nbases) continue;
    const uint32_t slot = atomicSub(&a.plane[u.bucket], 1u) - 1u;
    if ((int64_t)slot < nreads) dup_store_unit(a.sorted + slot, u);
  }
}

__global__ void __launch_bounds__(256) wfa_dup_resolve_kernel(DupArgs a) {
  const int64_t nreads = a.pair.place.nreads, nfrag = a.pair.nfrag;
  const int64_t have = a.plane[a.nbases], nunits = have < nreads ? have : nreads;
  const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < nunits; t += nthreads) {
    const DupUnit u = dup_load_unit(a.sorted + t);
    if (u.kind == 0 || u.bucket < 0 || u.bucket >= a.nbases) continue;
    const int64_t beg = a.plane[u.bucket], stop = a.plane[u.bucket + 1], end = stop < nunits ? stop : nunits;
    int32_t rep = u.unit, size = 1, overflow = 0;
    if (end - beg > WFA_DUP_MAX_BUCKET) {
      overflow = 1;
    } else {
      unsigned long long top = 0;
      size = 0;
      for (int64_t q = beg; q < end; ++q) {
        const int4* s = reinterpret_cast<const int4*>(a.sorted + q);
        const int4 k = s[0];   // bucket (two words), kind, end
        if (k.z != u.kind || k.w != u.end) continue;
        const int4 v = s[1];   // score, unit, m1, m2
        const unsigned long long key = ((unsigned long long)((uint32_t)v.x ^ 0x80000000u) << 32) | (uint32_t)~(uint32_t)v.y;
        top = key > top ? key : top;
        size += 1;
      }
      rep = (int32_t)~(uint32_t)top;   // (the walk meets the unit itself: size >= 1)
    }
    const int32_t dup = rep != u.unit ? 1 : 0;
    if (u.kind >= 3) {
      if (u.unit >= 0 && u.unit < nreads) dup_store_row(a.read_rows, u.unit, rep, size, dup, overflow);
    } else {
      if (u.unit >= 0 && u.unit < nfrag) dup_store_row(a.frag_rows, u.unit, rep, size, dup, overflow);
      if (u.m1 >= 0 && u.m1 < nreads) dup_store_row(a.read_rows, u.m1, -1, 0, dup, overflow);
      if (u.m2 >= 0 && u.m2 < nreads) dup_store_row(a.read_rows, u.m2, -1, 0, dup, overflow);
    }
  }
}

// ---- qsum (wfa_dup.hpp) ----

// the bytes of a word that are at least minq, summed
__device__ inline uint32_t dup_qsum_word(uint32_t w, uint32_t minq) {
  uint32_t s = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t q = (w >> (8 * k)) & 0xffu;
    s += q >= minq ? q : 0u;
  }
  return s;
}

__global__ void __launch_bounds__(256) wfa_dup_qsum_kernel(DupQsumArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const uint32_t minq = (uint32_t)a.min_quality;
  for (int64_t r = wave; r < a.nreads; r += nwaves) {
    const int64_t len = a.len[r] > 0 ? a.len[r] : 0;
    const uint8_t* p = a.quals + a.off[r];
    // [0, head) and [head + 16 * chunks, len) by bytes, the chunks between them 16-byte aligned: all of it inside [0, len)
    const int64_t to_edge = (int64_t)((16u - (uint32_t)((uintptr_t)p & 15u)) & 15u);
    const int64_t head = to_edge < len ? to_edge : len;
    const int64_t chunks = (len - head) >> 4, tail_at = head + (chunks << 4), tail = len - tail_at;
    unsigned long long sum = 0;
    if (lane < head) { const uint32_t q = p[lane]; sum += q >= minq ? q : 0u; }
    if (lane >= 16 && lane - 16 < tail) { const uint32_t q = p[tail_at + lane - 16]; sum += q >= minq ? q : 0u; }
    const uint4* c = reinterpret_cast<const uint4*>(p + head);
    for (int64_t k = lane; k < chunks; k += 64) {
      const uint4 v = c[k];
      sum += dup_qsum_word(v.x, minq) + dup_qsum_word(v.y, minq) + dup_qsum_word(v.z, minq) + dup_qsum_word(v.w, minq);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const uint32_t lo = __shfl_xor((uint32_t)sum, off), hi = __shfl_xor((uint32_t)(sum >> 32), off);
      sum += ((unsigned long long)hi << 32) | lo;
    }
    if (lane == 0) a.qsum[r] = (int32_t)(sum > (unsigned long long)INT32_MAX ? (unsigned long long)INT32_MAX : sum);
  }
}

int launch_dup_qsum(const DupQsumArgs& a, int cu_count, hipStream_t stream) {
  if (a.nreads <= 0) return 0;
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((a.nreads + 3) / 4, (int64_t)cu_count * 16));
  hipLaunchKernelGGL(wfa_dup_qsum_kernel, dim3(grid), dim3(256), 0, stream, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_dup(const DupArgs& a, int cu_count, hipStream_t stream) {
  const int64_t nreads = a.pair.place.nreads, nfrag = a.pair.nfrag;
  if (nreads <= 0) return 0;
  const unsigned rgrid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((nreads + 255) / 256, (int64_t)cu_count * 8));
  const unsigned fgrid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((nfrag + 255) / 256, (int64_t)cu_count * 8));
  if (nfrag > 0) hipLaunchKernelGGL(wfa_dup_key_fragments_kernel, dim3(fgrid), dim3(256), 0, stream, a);
  hipLaunchKernelGGL(wfa_dup_key_reads_kernel, dim3(rgrid), dim3(256), 0, stream, a);
  if (launch_place_scan(a.plane, a.nbases + 1, a.bsum, stream) != 0) return -1;
  hipLaunchKernelGGL(wfa_dup_scatter_kernel, dim3(rgrid), dim3(256), 0, stream, a);
  hipLaunchKernelGGL(wfa_dup_resolve_kernel, dim3(rgrid), dim3(256), 0, stream, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace wfa
