// k_seed.hpp — device helpers of the seed kernels (k_seed.hip; the layout and the rule: wfa_seed.hpp).
#pragma once
#include "wfa_seed.hpp"

namespace wfa {

// reverse complement of a k-mer code: the 2-bit groups reversed (bit reversal, swap inside each group), moved down to bit 0, code ^ 2
__device__ inline uint32_t seed_rc(uint32_t code, int k) {
  uint32_t v = __builtin_bitreverse32(code);
  v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
  return (v >> (32 - 2 * k)) ^ (0xAAAAAAAAu & ((1u << (2 * k)) - 1u));
}

// the k-mer at base p of the sequence whose first word is w0: false when one of its k letters is outside ACGT.  The caller has
// checked p + k <= len, so the second word is the sequence's own whenever one of its bits is used (behind the table: zero words).
__device__ inline bool seed_kmer(const SeedSetView& s, uint32_t w0, int32_t p, int k, uint32_t* code) {
  const uint32_t wi = w0 + ((uint32_t)p >> 4), r = (uint32_t)p & 15u;
  const uint64_t v = (((uint64_t)s.words[wi + 1] << 32) | s.words[wi]) >> (2u * r);
  *code = (uint32_t)v & ((1u << (2 * k)) - 1u);
  if (!s.mask) return true;
  const uint32_t m = ((uint32_t)s.mask[wi] | ((uint32_t)s.mask[wi + 1] << 16)) >> r;
  return (m & ((1u << k) - 1u)) == 0u;
}

// ---- minimizers (include/wfa_hip.h, "minimizers"; the choice of recomputing keys: wfa_seed.hpp) ----------------------------------------

#define WFA_SEED_KEY_INF (~0ull)   // above every mix32 value

__device__ inline uint32_t seed_mix32(uint32_t h) {
  h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
  return h;
}

// key(p) of the sequence of length len whose first word is w0: mix32 of the canonical code, +inf outside the sequence (p < 0 or
// p + k > len: no word is read) or over a masked letter; *code: the forward code of a finite key
__device__ inline uint64_t seed_key(const SeedSetView& s, uint32_t w0, int32_t len, int32_t p, int k, uint32_t* code) {
  if (p < 0 || p + k > len || !seed_kmer(s, w0, p, k, code)) return WFA_SEED_KEY_INF;
  return seed_mix32(min(*code, seed_rc(*code, k)));
}

// whether position p with the finite key kp is a (w,k)-minimizer of its sequence: l / r neighbours with key >= kp on either side,
// each capped at w - 1, l + r + 1 >= w.  The neighbours' keys are recomputed from the sequence's own words; the walk to the right
// stops as soon as the sum is reached.
__device__ inline bool seed_selected(const SeedSetView& s, uint32_t w0, int32_t len, int32_t p, int k, int w, uint64_t kp) {
  uint32_t c;
  int run = 1;   // l + r + 1
  for (int l = 1; l < w && seed_key(s, w0, len, p - l, k, &c) >= kp; ++l) ++run;
  for (int r = 1; r < w && run < w && seed_key(s, w0, len, p + r, k, &c) >= kp; ++r) ++run;
  return run >= w;
}

// the k-mer at p as the query kernels take it: valid and, under a minimizer index (w >= 1), a minimizer of the read
template <bool MINI>
__device__ inline bool seed_read_kmer(const SeedSetView& s, uint32_t w0, int32_t len, int32_t p, int k, int w, uint32_t* code) {
  if (!MINI) return seed_kmer(s, w0, p, k, code);
  const uint64_t kp = seed_key(s, w0, len, p, k, code);
  return kp != WFA_SEED_KEY_INF && seed_selected(s, w0, len, p, k, w, kp);
}

__device__ inline uint32_t seed_wave_sum(uint32_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
__device__ inline uint32_t seed_wave_min(uint32_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = min(v, (uint32_t)__shfl_xor(v, off));
  return v;
}
__device__ inline uint32_t seed_wave_inclusive(uint32_t v, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t u = __shfl_up(v, off);
    if (lane >= off) v += u;
  }
  return v;
}

// over the 256 threads of a workgroup; s_red: 4 words of LDS, free again when the call returns
__device__ inline uint32_t seed_block_sum(uint32_t v, uint32_t* s_red) {
  v = seed_wave_sum(v);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  v = s_red[0] + s_red[1] + s_red[2] + s_red[3];
  __syncthreads();
  return v;
}
__device__ inline uint32_t seed_block_min(uint32_t v, uint32_t* s_red) {
  v = seed_wave_min(v);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  v = min(min(s_red[0], s_red[1]), min(s_red[2], s_red[3]));
  __syncthreads();
  return v;
}
// exclusive prefix of v over the workgroup's threads, and the workgroup's total
__device__ inline uint32_t seed_block_exclusive(uint32_t v, uint32_t* s_red, uint32_t* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t inc = seed_wave_inclusive(v, lane);
  if (lane == 63) s_red[wave] = inc;
  __syncthreads();
  uint32_t base = 0;
  for (int w = 0; w < wave; ++w) base += s_red[w];
  *total = s_red[0] + s_red[1] + s_red[2] + s_red[3];
  __syncthreads();
  return base + inc - v;
}

}  // namespace wfa
