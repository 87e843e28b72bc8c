// wfa_calls.hpp — two reductions of a pileup table against its reference letters (wfa_hip_pileup_calls / _sites): one call byte per
// base, and the ordered rows of the bases where the reads disagree with the reference.
//
// Rule (include/wfa_hip.h, "calls and sites"; wfa_hip_calls_host / wfa_hip_sites_host in host_cigar.cpp are its plain statement,
// needing no GPU): per base the counters c0..c7 of the table, the reference column r of its byte, depth = c0 + .. + c5 in 64 bits.
//   call  6 below min_depth, else the greatest of c0..c5 (r among equals, else the smallest) | 8 when 2 * c6 > depth
//   site  depth >= min_depth and (the greatest non-reference column A has A >= 1, 1000 A >= permille * depth, or the same for c6)
//
// Layout: the table is a plane per column (wfa_pileup.hpp), a base's place in a plane its GLOBAL index seq_off[j] + pos; the set's
// byte blob holds the sequences back to back, so the reference byte of a base sits at the same global index.  A range of one
// sequence, and every sequence (seq = -1), are both one run [g0, g0 + n) of global indices, and ascending global index is ascending
// (j, pos).  Neighbouring lanes take neighbouring bases: seven coalesced int32 reads and one byte per base, 29 bytes.
//
// Kernels (k_calls.hip; the count and the scatter pass are the templates of k_select.hpp, which the genotypes and the two logs'
// reports instantiate under predicates of their own):
//   calls    a thread per base, grid-stride; one byte stored per base.
//   sites    three passes over chunks of `chunk` bases (a multiple of 64; WFA_HIP_CALLS_CHUNK), no atomics, no waiting on other
//            workgroups:
//     count    a workgroup per chunk: the predicate per base, ballot + popcount per wave, a workgroup sum -> chunk_count[chunk]
//     scan     one workgroup: the exclusive prefix of the chunk counts (64-bit) -> chunk_off[0 .. chunks], the last one the total
//     scatter  a workgroup per chunk: the predicate again, a site's rank = chunk_off[chunk] + the sites of the rounds and waves in
//              front of it + the popcount of the ballot below its lane; rows of rank < cap are written.  The sequence of a site is
//              the last one that starts at or before its global index (a binary search in seq_off, as the seed positions kernel's).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wfa_pileup.hpp"

namespace wfa {

#define WFA_SITE_COLS 8

struct CallsArgs {
  const int32_t* table;      // WFA_PILEUP_COLS planes of `total` counters
  int64_t total;
  const uint8_t* ref;        // the set's byte blob: the reference byte of global base g is ref[g]
  int64_t g0, n;             // the run of global base indices [g0, g0 + n)
  int32_t min_depth, min_permille;
  // calls
  uint8_t* out;              // [n]
  // sites
  int64_t chunk, chunks;     // bases per chunk (a multiple of 64), chunks = ceil(n / chunk)
  uint32_t* chunk_count;     // [chunks]
  uint64_t* chunk_off;       // [chunks + 1]
  const int64_t* seq_off;    // [nseq] first global index of a sequence
  int64_t nseq;
  int64_t cap;               // rows of `rows`
  int32_t* rows;             // [cap x WFA_SITE_COLS]
};

struct CallsBase { int32_t c[7]; int r; int64_t depth; };

__device__ inline CallsBase calls_load(const CallsArgs& a, int64_t g) {
  CallsBase b;
#pragma unroll
  for (int x = 0; x < 7; ++x) b.c[x] = a.table[(int64_t)x * a.total + g];
  b.r = wfa_pileup_letter_col(a.ref[g]);
  b.depth = 0;
#pragma unroll
  for (int x = 0; x < 6; ++x) b.depth += b.c[x];
  return b;
}

__host__ __device__ inline uint8_t calls_code(const CallsBase& b, int32_t min_depth) {
  if (b.depth < min_depth) return 6;
  int best = 0, cb = b.c[0], cr = b.c[0];
#pragma unroll
  for (int x = 1; x < 6; ++x) {
    if (b.c[x] > cb) { cb = b.c[x]; best = x; }
    if (x == b.r) cr = b.c[x];
  }
  if (cr == cb) best = b.r;
  return (uint8_t)(best | (2 * (int64_t)b.c[6] > b.depth ? 8 : 0));
}

// whether the base is a site; *alt, *snv: its greatest non-reference column and whether that one qualifies
__host__ __device__ inline bool calls_site(const CallsBase& b, int32_t min_depth, int32_t min_permille, int* alt, bool* snv) {
  int best = -1, cb = 0;
#pragma unroll
  for (int x = 0; x < 6; ++x)
    if (x != b.r && (best < 0 || b.c[x] > cb)) { cb = b.c[x]; best = x; }
  const int64_t bar = (int64_t)min_permille * b.depth;
  *alt = best;
  *snv = cb >= 1 && 1000 * (int64_t)cb >= bar;
  const bool ins = b.c[6] >= 1 && 1000 * (int64_t)b.c[6] >= bar;
  return b.depth >= min_depth && (*snv || ins);
}

// ---- genotyped sites (include/wfa_hip.h, "strands and genotypes"; wfa_hip_genotypes_host in host_cigar.cpp is the plain statement) ----
// The sites' three passes under a predicate with a strand filter, and rows of 16 columns: the site row, a diploid genotype and its
// confidence for the SNV and for the insertion event, and the forward counts.  The forward table (the pileup's second table, same
// planes and stride; nullptr on a pileup that does not track strands) is read only at bases that pass the sites' own predicate: in
// the count pass only when min_alt_strand > 0, in the scatter pass for the row's last four columns.  A row is four int4 stores.
#define WFA_GENOTYPE_COLS 16

struct GenoArgs {
  CallsArgs c;               // the run, the parameters of SITE, the chunks; rows: [cap x WFA_GENOTYPE_COLS]
  const int32_t* fwd;        // the forward table or nullptr
  int32_t err_q, min_alt_strand;
};

// the `ins` condition of SITE
__host__ __device__ inline bool calls_ins(const CallsBase& b, int32_t min_permille) {
  return b.c[6] >= 1 && 1000 * (int64_t)b.c[6] >= (int64_t)min_permille * b.depth;
}

// GENOTYPE over three given costs L0, L1, L2 (homozygous reference, heterozygous, homozygous alternate): the smallest, the smaller
// index on a tie; gq = min(99, second smallest - smallest)
__host__ __device__ inline void calls_genotype_costs(int64_t L0, int64_t L1, int64_t L2, int32_t* gt, int32_t* gq) {
  int best = 0;
  int64_t lo = L0, next = L1 < L2 ? L1 : L2;
  if (L1 < lo) { best = 1; lo = L1; next = L0 < L2 ? L0 : L2; }
  if (L2 < lo) { best = 2; lo = L2; next = L0 < L1 ? L0 : L1; }
  const int64_t d = next - lo;
  *gt = best;
  *gq = (int32_t)(d < 99 ? d : 99);
}

// GENOTYPE of an event with R reference and A alternate reads: the costs L0 = err_q A, L1 = 3 (R + A), L2 = err_q R.  (Under "base
// qualities", include/wfa_hip.h, the costs are sums of capped qualities instead.)
__host__ __device__ inline void calls_genotype(int64_t R, int64_t A, int32_t err_q, int32_t* gt, int32_t* gq) {
  calls_genotype_costs((int64_t)err_q * A, 3 * (R + A), (int64_t)err_q * R, gt, gq);
}

// whether a base with E events of a log (c6 of the insertions, starts[g] of the deletions) is a reported row of that log's report
// (include/wfa_hip.h, "insertions" / "deletions": the ins condition of SITE on E, or bit 3 of CALL on E under min_permille 0)
__host__ __device__ inline bool event_selected(int64_t depth, int32_t E, int32_t min_depth, int32_t min_permille) {
  if (depth < min_depth) return false;
  if (min_permille > 0) return E >= 1 && 1000 * (int64_t)E >= (int64_t)min_permille * depth;
  return 2 * (int64_t)E > depth;
}

int launch_calls(const CallsArgs& a, int cu_count, hipStream_t stream);
int launch_sites_count(const CallsArgs& a, hipStream_t stream);     // count + scan: chunk_off[chunks] is the number of sites
int launch_sites_scatter(const CallsArgs& a, hipStream_t stream);
int launch_sites_scan(const CallsArgs& a, hipStream_t stream);      // the scan alone, over chunk counts another count kernel wrote (the two logs' selects)
int launch_genotypes_count(const GenoArgs& a, hipStream_t stream);  // count + scan, as launch_sites_count
// the scatter pass; quals: with the costs of "base qualities" from qtab, the pileup's quality table (the table's planes and stride), read
// only at bases that are reported, in the planes of the events' columns.  The count pass is the same for both: the selection is.
int launch_genotypes_scatter(const GenoArgs& a, bool quals, const int32_t* qtab, hipStream_t stream);

}  // namespace wfa
