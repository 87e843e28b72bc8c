// wfa_seed.hpp — the seed finder (wfa_hip_seed_index_*): an exact-match k-mer index over a resident text set, built on the device,
// and the query that turns the reads of a pattern set into candidate windows for wfa_hip_batch_create_windows / wfa_hip_pileup_add.
//
// Rule (include/wfa_hip.h; wfa_hip_seeds_host in host_seed.cpp is its plain statement for one read, needing no GPU): every valid
// k-mer of the read, on either strand, at read position r matches the indexed text positions (j, t) of the same 2-bit code unless the
// code occurs more than max_occ times; a match is a hit (s, j, d = t - r); the read's hits sorted by (s, j, d) fall into clusters
// (maximal runs of one (s, j) whose neighbouring d differ by at most `gap`); the n clusters with the most hits (at least min_hits;
// ties to the smaller (s, j, d_lo)) become windows [max(0, d_lo - pad), min(tl[j], d_hi + L + pad)) of text j.
//
// Layout of the index on the device (a direct-addressed counting sort, no device sort):
//   table    4^k + 1 uint32: bucket x of k-mer code x is records [table[x], table[x + 1])          4^k * 4 BYTES (k = 13: 256 MiB,
//                                                                                                   k = 15: 4 GiB), its own allocation
//   records  one {j, t} int32 pair per indexed position, in bucket order (order inside a bucket:    8 BYTES PER INDEXED POSITION
//            whatever the fill's atomics gave — the rule above sorts a read's hits, so it is harmless)
// and, copied from the set so that the index outlives it, the texts' lengths (4 bytes per sequence).
// A k-mer code: base p + i of the sequence in bits 2 i .. 2 i + 1 (wfa_hip_pack_2bit's codes: A 0, C 1, T 2, G 3), i.e. the funnel
// shift of two neighbouring words of the set by the residue of p, cut to 2 k bits.  The reverse strand of a read needs no second pass
// over its words: the k-mer at position r of the reverse complement is the reverse complement of the k-mer at L - k - r (the 2-bit
// groups reversed: a bit reversal and a swap inside each group, then code ^ 2).
// Letters outside ACGT: one bit per base, 16 bits per word of the set in the words' own layout (mask[w] beside words[w]), built on
// the host from the runs wfa_hip_seqset_create keeps and uploaded once per set, when the set has such a letter at all.
//
// Kernels (k_seed.hip):
//   wfa_seed_positions_kernel<FILL>                one thread per word of the text set (its 16 start positions).  Count: an atomicAdd
//       per valid position with t % stride == 0 into table[code]; fill: its record slot by an atomicSub on the bucket's END
//   wfa_seed_scan_{reduce,top,apply}_kernel        the hand-written inclusive scan of the table in chunks of 4096 counters (chunk
//       sums, a one-workgroup scan of those, the chunks again); the reduce pass also counts the k-mers over max_occ.  After the
//       fill every bucket's end has walked down to its start: table[x] is the exclusive prefix, table[4^k] the total.
//   wfa_seed_query_kernel                          one 256-thread workgroup per read, grid-stride: a counting pass (the read's hits
//       H, both strands; H > max_hits: overflow, no seeds), a gather of the hits into LDS as 64-bit keys (s | j | d biased), a
//       bitonic sort of the next power of two, cluster starts carried to every hit by a max-scan in LDS (two uint16 planes), and up
//       to n rounds of a workgroup-wide minimum over the cluster ends' rank keys.  LDS: 32 KB of keys + 16 KB of scan planes.
//       Every store goes to row i of the M x n result arrays or to overflow[i]; the gather checks its LDS slot against the capacity.
//
// Minimizers (include/wfa_hip.h, "minimizers"; w >= 1 in the argument blocks below, w = 0: the stride index, whose kernels and code
// paths are the ones above, untouched).  The table, the scan and the records are the same; only WHICH positions enter differs:
//   wfa_seed_minimizer_positions_kernel<FILL>      the sibling of the positions kernel, a thread per word of the text set again: of
//       its 16 positions it takes those that are minimizers of the owning sequence.
//   wfa_seed_query_kernel<true>, wfa_chain_kernel<true>   the same kernels with the read's positions filtered the same way (<false>
//       is the code as it was).
// The selection RECOMPUTES the neighbours' keys from the sequence's own words (k_seed.hpp: seed_key, seed_selected) in all three
// kernels, instead of staging a tile of keys in LDS: a key is two cached word reads, a funnel shift, a bit reversal and five
// multiply/xor steps; the walk stops at the first smaller key, which for hashed keys comes after about ln w steps on either side (at
// most 2 (w - 1) keys for a position inside a run of ties or beside a sequence end); and a neighbour is addressed by (first word,
// length) of ITS sequence, so a workgroup's tile edge, a short sequence inside a tile and the counting pass versus the gather pass are
// not cases: every pass evaluates one predicate on the same words.  The query kernel keeps its 48 KB of LDS as they were and no
// kernel gains an array, so none needs scratch (the resource figures: DESIGN.md §6.4).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace wfa {

#define WFA_SEED_MIN_K 8
#define WFA_SEED_MAX_K 15
#define WFA_SEED_MAX_W 32
#define WFA_SEED_MAX_N 16
#define WFA_SEED_MAX_HITS 4096      // the LDS key array of the query kernel
#define WFA_SEED_SCAN_CHUNK 4096    // counters per workgroup of the table scan (256 threads x 16)

struct SeedRec { int32_t j, t; };

// the 2-bit table of a set as the kernels read it
struct SeedSetView {
  const uint32_t* words;    // the set's word table (4 zero words behind it)
  const uint16_t* mask;     // [nwords + 4] one bit per base outside ACGT, or nullptr: the set has no such letter
  const uint32_t* woff;     // [nseq] first word of a sequence
  const int32_t* len;       // [nseq]
  int64_t nseq;
  uint64_t nwords;
};

struct SeedBuildArgs {
  SeedSetView t;
  int k, stride;
  int w;                    // 0: the stride index; 1 .. WFA_SEED_MAX_W: the minimizer index (stride plays no part)
  uint32_t max_occ;
  uint32_t* table;          // [4^k + 1]
  SeedRec* recs;            // [total]
  uint32_t* bsum;           // [chunks] the scan's chunk sums
  uint32_t* masked;         // [1] k-mers with more than max_occ positions
};

struct SeedQueryArgs {
  SeedSetView p;
  const uint32_t* table; const SeedRec* recs; const int32_t* t_len; int64_t t_nseq;
  int k;
  int w;                    // of the index: 0, or the minimizer window
  uint32_t max_occ;
  int n, min_hits, max_hits;
  uint32_t gap;
  int32_t pad;
  int32_t *j, *reverse, *text_start, *text_len, *hits;   // [npat x n]
  uint8_t* overflow;                                      // [npat]
};

int launch_seed_count(const SeedBuildArgs& a, hipStream_t stream);
int launch_seed_scan(const SeedBuildArgs& a, hipStream_t stream);
int launch_seed_fill(const SeedBuildArgs& a, uint32_t cap, hipStream_t stream);   // cap: the records' capacity
int launch_seed_query(const SeedQueryArgs& a, int64_t npat, int cu_count, hipStream_t stream);

}  // namespace wfa
