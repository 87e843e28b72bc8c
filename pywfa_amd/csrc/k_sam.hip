// k_sam.hip — the SAM fields of a batch's pairs (wfa_sam.hpp: SamArgs and the outline; wfa_hip_batch_sam_counts / _sam_strings in
// api_sam.hip).  One wave per pair, grid-stride; everything that steers the walk comes out of a ballot, so it is wave-uniform.  The two
// passes are one function: pass 1 sums the token lengths it computes, pass 2 places and stores the same tokens.
//
// BOUNDS.  Every op index that is loaded lies in [0, cigar_len) of the pair's own string: a lane's own op and the two neighbours of a
// round (base - 1 with base > 0, base + 64 below the length).  A text letter is loaded only for an offset below tlen.  Pass 2 stores a
// byte only below the pair's own length of the string (columns 5 and 6 of its row, which sized the buffers), so a string that
// disagreed with pass 1 would be cut short, never written outside its pair's bytes.  A byte has one writer: the tokens' places are a
// prefix sum of their lengths.
#include "k_select.hpp"   // (launch_scan64, wave_grid, the wave sums of the seed kernels)
#include "wfa_sam.hpp"

namespace wfa {

// decimal digits of v: by comparisons (up to 10)
__device__ __forceinline__ int sam_digits(uint32_t v) {
  return 1 + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) + (v >= 10000000u) +
         (v >= 100000000u) + (v >= 1000000000u);
}
// out[at .. at + nd) = the nd digits of v, as far as they lie below cap
__device__ __forceinline__ void sam_put_number(uint8_t* out, int at, int cap, uint32_t v, int nd) {
  for (int k = nd - 1; k >= 0; --k) {
    const uint32_t d = v / 10u;
    if (at + k < cap) out[at + k] = (uint8_t)('0' + (v - d * 10u));
    v = d;
  }
}
__device__ __forceinline__ void sam_put(uint8_t* out, int at, int cap, uint32_t byte) {
  if (at < cap) out[at] = (uint8_t)byte;
}
// the SAM letter of an op, 0 for a byte that is no op: the library's D inserts into the read, its I deletes from it
__device__ __forceinline__ uint32_t sam_letter(uint32_t c, bool eqx) {
  return c == 'M' ? (eqx ? '=' : 'M') : c == 'X' ? (eqx ? 'X' : 'M') : c == 'D' ? 'I' : c == 'I' ? 'D' : 0u;
}

template <bool WRITE>
__device__ __forceinline__ void sam_pair(const SamArgs& a, int64_t q, int lane) {
  const bool eqx = (a.sam_flags & 1) != 0, core = (a.sam_flags & 2) != 0;
  int4* row = reinterpret_cast<int4*>(a.rows + q * WFA_SAM_COLS);
  int cap_c = 0, cap_m = 0, clip_left = 0, clip_right = 0;
  if (WRITE) {
    const int4 r0 = row[0], r1 = row[1];
    if (r0.x < 0) return;   // UNMAPPED: no bytes
    clip_left = r0.z; clip_right = r0.w; cap_c = r1.y; cap_m = r1.z;
  }
  // the span: first anchor op .. last anchor op
  int len = 0, f = -1, l = -1;
  const uint8_t* p = a.ops;
  if (a.status[q] == 0) {
    len = a.cigar_len[q];
    p += a.cigar_begin[q];
    for (int base = 0; base < len; base += 64) {
      const int i = base + lane;
      const uint32_t c = (i < len) ? p[i] : 0u;
      const unsigned long long ba = __ballot(c == 'M' || (c == 'X' && !core));
      if (ba) {
        if (f < 0) f = base + __builtin_ctzll(ba);
        l = base + 63 - __builtin_clzll(ba);
      }
    }
  }
  if (f < 0) {
    if (!WRITE && lane == 0) { row[0] = make_int4(-1, 0, 0, 0); row[1] = make_int4(0, 0, 0, 0); }
    return;
  }
  const WfaPairMeta m = a.meta[q];
  const uint8_t* tb = (WRITE && a.bytes != nullptr && a.tboff != nullptr && a.flags[q] != 0) ? a.bytes + a.tboff[q] : nullptr;
  const uint32_t* tw = a.words + m.t_woff;
  uint8_t* out_c = WRITE ? a.cigar + a.cigar_off[q] : nullptr;
  uint8_t* out_m = WRITE ? a.md + a.md_off[q] : nullptr;
  const unsigned long long lower = (1ull << lane) - 1ull;
  int h0 = 0;          // text bases in front of this round
  int cstart = f;      // the start of the CIGAR run that is open when the round begins
  int mrun = 0;        // M ops of the span since the last MD event
  int cpos = 0, mpos = 0;   // pass 1: the bytes so far; pass 2: where the round's first token goes
  int pos = 0, ref_len = 0, nm = 0, query_len = 0;
  if (WRITE && clip_left > 0) {
    cpos = sam_digits((uint32_t)clip_left) + 1;
    if (lane == 0) { sam_put_number(out_c, 0, cap_c, (uint32_t)clip_left, cpos - 1); sam_put(out_c, cpos - 1, cap_c, 'S'); }
  }
  for (int base = 0; base < len; base += 64) {
    const int i = base + lane;
    const uint32_t c = (i < len) ? p[i] : 0u;
    uint32_t prev = __shfl_up(c, 1), next = __shfl_down(c, 1);
    if (lane == 0) prev = base > 0 ? p[base - 1] : 0u;
    if (lane == 63) next = base + 64 < len ? p[base + 64] : 0u;
    const unsigned long long bm = __ballot(c == 'M'), bx = __ballot(c == 'X'), bi = __ballot(c == 'I'), bd = __ballot(c == 'D');
    const bool in = i >= f && i <= l;
    const unsigned long long bin = __ballot(in);
    if (!WRITE) {
      const unsigned long long bbefore = __ballot(i < f), bafter = __ballot(i > l);
      pos += __builtin_popcountll((bx | bi) & bbefore);
      clip_left += __builtin_popcountll((bx | bd) & bbefore);
      clip_right += __builtin_popcountll((bx | bd) & bafter);
      ref_len += __builtin_popcountll((bm | bx | bi) & bin);
      nm += __builtin_popcountll((bx | bi | bd) & bin);
      query_len += __builtin_popcountll((bm | bx | bd) & bin);
    }
    // CIGAR: the lane at a run's last op holds its token
    const uint32_t mc = sam_letter(c, eqx);
    const bool is_start = in && mc != 0u && (i == f || sam_letter(prev, eqx) != mc);
    const bool is_end = in && mc != 0u && (i == l || sam_letter(next, eqx) != mc);
    const unsigned long long bs = __ballot(is_start);
    uint32_t run_len = 0, ctok = 0;
    if (is_end) {
      const unsigned long long mine = bs & (lower | (1ull << lane));
      const int start = mine ? base + 63 - __builtin_clzll(mine) : cstart;
      run_len = (uint32_t)(i - start + 1);
      ctok = (uint32_t)sam_digits(run_len) + 1u;
    }
    if (bs) cstart = base + 63 - __builtin_clzll(bs);
    // MD: the lane of an event (an X, the first I of a run) holds the number in front of it; a further I its letter alone
    const bool is_x = in && c == 'X', is_i = in && c == 'I', first_i = is_i && prev != 'I';
    const bool event = is_x || first_i;
    const unsigned long long be = __ballot(event), bmi = bm & bin;
    uint32_t md_run = 0, mtok = 0;
    if (event) {
      const unsigned long long earlier = be & lower;
      md_run = earlier ? (uint32_t)__builtin_popcountll(bmi & lower & ~((2ull << (63 - __builtin_clzll(earlier))) - 1ull))
                       : (uint32_t)(mrun + __builtin_popcountll(bmi & lower));
      mtok = (uint32_t)sam_digits(md_run) + (first_i ? 2u : 1u);
    } else if (is_i) {
      mtok = 1u;
    }
    if (be) mrun = __builtin_popcountll(bmi & ~((2ull << (63 - __builtin_clzll(be))) - 1ull));
    else mrun += __builtin_popcountll(bmi);
    // the two token lengths in one word: a round's sums stay below 64 x 12
    const uint32_t both = ctok | (mtok << 16);
    if (WRITE) {
      const uint32_t inc = seed_wave_inclusive(both, lane);
      if (ctok) {
        const int at = cpos + (int)(inc & 0xffffu) - (int)ctok;
        sam_put_number(out_c, at, cap_c, run_len, (int)ctok - 1);
        sam_put(out_c, at + (int)ctok - 1, cap_c, mc);
      }
      if (mtok) {
        const int h = h0 + __builtin_popcountll((bm | bx | bi) & lower);   // the text offset of this op
        uint32_t letter = 'N';
        if (h < m.tlen) letter = tb ? (uint32_t)tb[h] : (0x47544341u >> (8u * ((tw[h >> 4] >> (2 * (h & 15))) & 3u))) & 0xffu;   // codes (c >> 1) & 3: A C T G
        int at = mpos + (int)(inc >> 16) - (int)mtok;
        if (event) {
          const int nd = (int)mtok - (first_i ? 2 : 1);
          sam_put_number(out_m, at, cap_m, md_run, nd);
          at += nd;
          if (first_i) sam_put(out_m, at++, cap_m, '^');
        }
        sam_put(out_m, at, cap_m, letter);
      }
      const uint32_t total = (uint32_t)__shfl((int)inc, 63);
      cpos += (int)(total & 0xffffu); mpos += (int)(total >> 16);
    } else {
      const uint32_t total = seed_wave_sum(both);
      cpos += (int)(total & 0xffffu); mpos += (int)(total >> 16);
    }
    h0 += __builtin_popcountll(bm | bx | bi);
  }
  // the right clip, and the MD string's last number
  const int nd_last = sam_digits((uint32_t)mrun);
  if (WRITE) {
    if (lane == 0) {
      if (clip_right > 0) {
        const int nd = sam_digits((uint32_t)clip_right);
        sam_put_number(out_c, cpos, cap_c, (uint32_t)clip_right, nd);
        sam_put(out_c, cpos + nd, cap_c, 'S');
      }
      sam_put_number(out_m, mpos, cap_m, (uint32_t)mrun, nd_last);
    }
  } else if (lane == 0) {
    const int cigar_len = cpos + (clip_left > 0 ? sam_digits((uint32_t)clip_left) + 1 : 0) + (clip_right > 0 ? sam_digits((uint32_t)clip_right) + 1 : 0);
    row[0] = make_int4(pos, ref_len, clip_left, clip_right);
    row[1] = make_int4(nm, cigar_len, mpos + nd_last, query_len);
  }
}

template <bool WRITE>
__global__ void __launch_bounds__(256) wfa_sam_kernel(SamArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t q = wave; q < a.npairs; q += nwaves) sam_pair<WRITE>(a, q, lane);
}

int launch_sam_counts(const SamArgs& a, uint64_t* cigar_off, uint64_t* md_off, int cu_count, hipStream_t stream) {
  if (a.npairs <= 0) return 0;
  hipLaunchKernelGGL(wfa_sam_kernel<false>, dim3(wave_grid(a.npairs, cu_count)), dim3(256), 0, stream, a);
  if (hipGetLastError() != hipSuccess) return -1;
  const uint32_t* rows = reinterpret_cast<const uint32_t*>(a.rows);
  if (launch_scan64(rows + 5, WFA_SAM_COLS, cigar_off, a.npairs, stream) != 0) return -1;
  return launch_scan64(rows + 6, WFA_SAM_COLS, md_off, a.npairs, stream);
}

int launch_sam_strings(const SamArgs& a, int cu_count, hipStream_t stream) {
  if (a.npairs <= 0) return 0;
  hipLaunchKernelGGL(wfa_sam_kernel<true>, dim3(wave_grid(a.npairs, cu_count)), dim3(256), 0, stream, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace wfa
