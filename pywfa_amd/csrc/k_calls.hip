// k_calls.hip — calls, sites and genotyped sites of a pileup (wfa_calls.hpp: rule, layout and the kernels' outline; k_select.hpp: the
// count and scatter passes; wfa_hip_pileup_calls / _sites / _genotypes in api_pileup.hip), and the two scans of the pileup family.
// Stores: the calls kernel writes out[i] for i < n; the count kernels chunk_count[ch] for ch < chunks; the chunk scan chunk_off[i] for
// i <= chunks; the 64-bit scan out[i] for i <= n; the scatter kernels row `rank` only where rank < cap.  The host has checked that
// [g0, g0 + n) lies inside the table and the byte blob.
#include "k_select.hpp"

namespace wfa {

__global__ void __launch_bounds__(256) wfa_calls_kernel(CallsArgs a) {
  const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += nthreads)
    a.out[i] = calls_code(calls_load(a, a.g0 + i), a.min_depth);
}

// ---- the scans: one workgroup each --------------------------------------------------------------------------------------------------------
// the chunk counts to their exclusive prefix in 64 bits, chunk_off[chunks] the total: 256 counts per round
__global__ void __launch_bounds__(256) wfa_sites_scan_kernel(CallsArgs a) {
  __shared__ uint32_t s_red[4];
  uint64_t carry = 0;
  for (int64_t b0 = 0; b0 < a.chunks; b0 += 256) {
    const int64_t i = b0 + threadIdx.x;
    const uint32_t v = i < a.chunks ? a.chunk_count[i] : 0u;
    uint32_t total;   // (256 chunks of at most 2^20 bases: below 2^32)
    const uint32_t ex = seed_block_exclusive(v, s_red, &total);
    if (i < a.chunks) a.chunk_off[i] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) a.chunk_off[a.chunks] = carry;
}

// exclusive 64-bit scan of 32-bit values read with a stride: 2 048 values per round (8 per thread)
__global__ void __launch_bounds__(256) wfa_scan64_kernel(const uint32_t* in, int stride, uint64_t* out, int64_t n) {
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

// ---- sites ---------------------------------------------------------------------------------------------------------------------------------
// whether base i of the run is a site (false behind the run's end)
__device__ inline bool sites_flag(const CallsArgs& a, int64_t i, CallsBase* b, int* alt, bool* snv) {
  if (i >= a.n) return false;
  *b = calls_load(a, a.g0 + i);
  return calls_site(*b, a.min_depth, a.min_permille, alt, snv);
}

__global__ void __launch_bounds__(256) wfa_sites_count_kernel(CallsArgs a) {
  select_count(a, [&](int64_t i) { CallsBase b; int alt; bool snv; return sites_flag(a, i, &b, &alt, &snv); });
}

__global__ void __launch_bounds__(256) wfa_sites_scatter_kernel(CallsArgs a) {
  select_scatter(a, (uint64_t)a.cap, [&](int64_t i, bool live, auto rank_of) {
    CallsBase b; int alt; bool snv;
    uint64_t rank;
    if (!rank_of(live && sites_flag(a, i, &b, &alt, &snv), &rank)) return;
    const int64_t g = a.g0 + i, j = select_owner(a, g);
    int32_t ref_count = b.c[0];
#pragma unroll
    for (int x = 1; x < 5; ++x) if (x == b.r) ref_count = b.c[x];
    int32_t alt_count = 0;
#pragma unroll
    for (int x = 0; x < 6; ++x) if (x == alt) alt_count = b.c[x];
    int4* row = reinterpret_cast<int4*>(a.rows + rank * WFA_SITE_COLS);
    row[0] = make_int4((int32_t)j, (int32_t)(g - a.seq_off[j]), b.r, snv ? alt : -1);
    row[1] = make_int4((int32_t)b.depth, ref_count, snv ? alt_count : 0, b.c[6]);
  });
}

// ---- genotyped sites: the same three passes, the predicate with the strand filter, rows of WFA_GENOTYPE_COLS (wfa_calls.hpp) --------
// Loads of the forward table stay at global indices in [g0, g0 + n) of planes 0..6, as the table's; the host has checked that it
// exists when min_alt_strand > 0.

// column x (0..5, wave-divergent) of the seven counters of a base
__device__ inline int32_t geno_pick(const int32_t* c, int x) {
  int32_t v = c[0];
#pragma unroll
  for (int k = 1; k < 6; ++k) if (k == x) v = c[k];
  return v;
}

// whether base i of the run is reported (false behind the run's end); *snv, *ins: its two events after the strand filter
__device__ inline bool geno_flag(const GenoArgs& a, int64_t i, CallsBase* b, int* alt, bool* snv, bool* ins) {
  const CallsArgs& c = a.c;
  if (i >= c.n) return false;
  *b = calls_load(c, c.g0 + i);
  if (!calls_site(*b, c.min_depth, c.min_permille, alt, snv)) return false;
  *ins = calls_ins(*b, c.min_permille);
  if (a.min_alt_strand > 0) {
    const int64_t g = c.g0 + i, mas = a.min_alt_strand;
    const int64_t fa = a.fwd[(int64_t)*alt * c.total + g], f6 = a.fwd[(int64_t)WFA_PILEUP_INS * c.total + g];
    *snv = *snv && fa >= mas && (int64_t)geno_pick(b->c, *alt) - fa >= mas;
    *ins = *ins && f6 >= mas && (int64_t)b->c[6] - f6 >= mas;
  }
  return *snv || *ins;
}

__global__ void __launch_bounds__(256) wfa_genotypes_count_kernel(GenoArgs a) {
  select_count(a.c, [&](int64_t i) { CallsBase b; int alt; bool snv, ins; return geno_flag(a, i, &b, &alt, &snv, &ins); });
}

// The scatter pass.  QUALS: with the costs of "base qualities" (include/wfa_hip.h): the costs of an event are sums of the quality
// table qtab, loaded at this base only, in the planes of the event's columns (0..6, at global indices in [g0, g0 + n), as the
// table's); the ranks, the rows and the stores are the same.  Without QUALS qtab is not read.
template <bool QUALS>
__device__ __forceinline__ void geno_scatter(const GenoArgs& a, const int32_t* qtab) {
  const CallsArgs& c = a.c;
  select_scatter(c, (uint64_t)c.cap, [&](int64_t i, bool live, auto rank_of) {
    CallsBase b; int alt; bool snv, ins;
    uint64_t rank;
    if (!rank_of(live && geno_flag(a, i, &b, &alt, &snv, &ins), &rank)) return;
    const int64_t g = c.g0 + i, j = select_owner(c, g);
    const int32_t ref_count = geno_pick(b.c, b.r), alt_count = geno_pick(b.c, alt);
    int32_t gt = -1, gq = -1, ins_gt = -1, ins_gq = -1;
    if (snv) {
      if (QUALS) calls_genotype_costs(qtab[(int64_t)alt * c.total + g], 3 * ((int64_t)ref_count + alt_count), qtab[(int64_t)b.r * c.total + g], &gt, &gq);
      else calls_genotype(ref_count, alt_count, a.err_q, &gt, &gq);
    }
    if (ins) {
      const int64_t R = b.depth > b.c[6] ? b.depth - b.c[6] : 0;
      if (QUALS) calls_genotype_costs(qtab[(int64_t)WFA_PILEUP_INS * c.total + g], 3 * (R + b.c[6]), (int64_t)a.err_q * R, &ins_gt, &ins_gq);
      else calls_genotype(R, b.c[6], a.err_q, &ins_gt, &ins_gq);
    }
    int4 strands = make_int4(-1, -1, -1, -1);
    if (a.fwd) {
      int32_t f[7];
      int64_t depth_fwd = 0;
#pragma unroll
      for (int x = 0; x < 7; ++x) f[x] = a.fwd[(int64_t)x * c.total + g];
#pragma unroll
      for (int x = 0; x < 6; ++x) depth_fwd += f[x];
      strands = make_int4((int32_t)depth_fwd, geno_pick(f, b.r), snv ? geno_pick(f, alt) : 0, f[6]);
    }
    int4* row = reinterpret_cast<int4*>(c.rows + rank * WFA_GENOTYPE_COLS);
    row[0] = make_int4((int32_t)j, (int32_t)(g - c.seq_off[j]), b.r, snv ? alt : -1);
    row[1] = make_int4((int32_t)b.depth, ref_count, snv ? alt_count : 0, b.c[6]);
    row[2] = make_int4(gt, gq, ins_gt, ins_gq);
    row[3] = strands;
  });
}

// (two kernels, so that the one without qualities compiles to the code it had before there were any)
__global__ void __launch_bounds__(256) wfa_genotypes_scatter_kernel(GenoArgs a) { geno_scatter<false>(a, nullptr); }
__global__ void __launch_bounds__(256) wfa_genotypes_quals_scatter_kernel(GenoArgs a, const int32_t* qtab) { geno_scatter<true>(a, qtab); }

int launch_scan64(const uint32_t* in, int stride, uint64_t* out, int64_t n, hipStream_t stream) {
  hipLaunchKernelGGL(wfa_scan64_kernel, dim3(1), dim3(256), 0, stream, in, stride, out, std::max<int64_t>(n, 0));
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_calls(const CallsArgs& a, int cu_count, hipStream_t stream) {
  if (a.n <= 0) return 0;
  hipLaunchKernelGGL(wfa_calls_kernel, dim3(thread_grid(a.n, cu_count)), dim3(256), 0, stream, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_sites_scan(const CallsArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(wfa_sites_scan_kernel, dim3(1), dim3(256), 0, stream, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_sites_count(const CallsArgs& a, hipStream_t stream) {
  if (a.chunks > 0) hipLaunchKernelGGL(wfa_sites_count_kernel, dim3(chunk_grid(a.chunks)), dim3(256), 0, stream, a);
  return launch_sites_scan(a, stream);
}

int launch_sites_scatter(const CallsArgs& a, hipStream_t stream) {
  if (a.chunks <= 0 || a.cap <= 0) return 0;
  hipLaunchKernelGGL(wfa_sites_scatter_kernel, dim3(chunk_grid(a.chunks)), dim3(256), 0, stream, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_genotypes_count(const GenoArgs& a, hipStream_t stream) {
  if (a.min_alt_strand > 0 && !a.fwd) return -1;
  if (a.c.chunks > 0) hipLaunchKernelGGL(wfa_genotypes_count_kernel, dim3(chunk_grid(a.c.chunks)), dim3(256), 0, stream, a);
  return launch_sites_scan(a.c, stream);
}

int launch_genotypes_scatter(const GenoArgs& a, bool quals, const int32_t* qtab, hipStream_t stream) {
  if (a.c.chunks <= 0 || a.c.cap <= 0) return 0;
  if ((quals && !qtab) || (a.min_alt_strand > 0 && !a.fwd)) return -1;
  if (quals) hipLaunchKernelGGL(wfa_genotypes_quals_scatter_kernel, dim3(chunk_grid(a.c.chunks)), dim3(256), 0, stream, a, qtab);
  else hipLaunchKernelGGL(wfa_genotypes_scatter_kernel, dim3(chunk_grid(a.c.chunks)), dim3(256), 0, stream, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace wfa
