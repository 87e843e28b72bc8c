// wfa_chain.hpp — co-linear chaining on the seed index (wfa_hip_seed_index_chain): from the reads of a pattern set and the index of
// wfa_seed.hpp, the best chains of every read's anchors as candidate windows, text and pattern side, for
// wfa_hip_batch_create_windows / wfa_hip_pileup_add.  The index and its build are those of wfa_seed.hpp, untouched.
//
// Rule (include/wfa_hip.h, "chains"; wfa_hip_chains_host in host_chain.cpp is its plain statement for one read, needing no GPU): the
// read's anchors (s, r, j, t) sorted by (s, r, j, t); each adopts, of the `lookback` anchors before it, the eligible one (same s and j,
// 0 < dr, dt <= max_dist, |dt - dr| <= band) of largest f(b) + min(dr, dt, k) - cost(|dt - dr|), the nearest on a tie, when that is more
// than k; n rounds take the uncovered anchor of largest f (cnt >= min_hits, f >= min_score; the first in the order on a tie), whose
// window [max(0, d_lo - pad), min(tl[j], d_hi + L + pad)) covers the anchors of its (s, j) inside it.
//
// Workspace (HBM, its own allocation, kept on the index): one SLAB per workgroup of the launch, 8 int32 planes of max_anchors entries
// (j, t, r | f, cnt, d_lo, d_hi, r_first): 32 BYTES x max_anchors PER RESIDENT WORKGROUP.  A covered anchor has f = -1.
//
// Kernel (k_chain.hip), wfa_chain_kernel: one 256-thread workgroup per read, grid-stride.  Thread x owns a contiguous range of the
// read's k-mer starts.
//   count    both strands' bucket sizes over the thread's range (saturating), two workgroup prefix scans: N_0, N_1 and the thread's
//            place in (s, r) order (strand 1 runs down the read: its place counts from the far end).  N > max_anchors: overflow.
//   gather   the range again: a position's records go to its (s, r) place, each at the number of records of its bucket with a
//            smaller (j, t) — the rank inside the bucket, occ^2 compares, `records` left as built.  No sort.
//   chain    wave 0 chains strand 0, wave 1 strand 1, 64 anchors per round: lane l loads anchor base + l (coalesced), the round's
//            anchors are then taken in order, each broadcast to the wave.  The last 64 anchors' state lives IN REGISTERS, anchor a in
//            lane a % 64, so every lane holds exactly one candidate and evaluates it; a wave maximum over value << 7 | 64 - distance
//            picks the best, nearest first; the winner's state is read across lanes and the anchor's own replaces the lane's.  After
//            the round lane l stores anchor base + l's state (coalesced).  No LDS ring, no barrier inside a strand.
//   select   n rounds of a workgroup maximum over f << 32 | ~index; thread 0 writes the row's column and publishes the window, all
//            threads cover (f = -1) the anchors inside it.
// Every store goes to row i < M of the result arrays, columns below n, to overflow[i], or to the workgroup's own slab below max_anchors.
#pragma once
#include "wfa_seed.hpp"

namespace wfa {

#define WFA_CHAIN_MAX_LOOKBACK 64
#define WFA_CHAIN_MAX_ANCHORS 65536
#define WFA_CHAIN_PLANES 8            // int32 planes of a slab
#define WFA_CHAIN_BLOCKS_PER_CU 4     // resident workgroups per CU the launch asks for (the workspace is sized by the grid)

struct ChainArgs {
  SeedSetView p;
  const uint32_t* table; const SeedRec* recs; const int32_t* t_len; int64_t t_nseq;
  int k;
  int w;                    // of the index: 0, or the minimizer window (wfa_seed.hpp)
  uint32_t max_occ;
  int n, min_hits, min_score, lookback, max_dist, band;
  int32_t pad;
  uint32_t max_anchors;
  int32_t* slab;                                           // [grid x WFA_CHAIN_PLANES x max_anchors]
  int32_t *j, *reverse, *text_start, *text_len, *hits, *score, *pattern_start, *pattern_len;   // [npat x n]
  uint8_t* overflow;                                       // [npat]
};

unsigned chain_grid(int64_t npat, int cu_count);           // the workgroups of a launch over npat reads
int launch_chain(const ChainArgs& a, int64_t npat, unsigned grid, hipStream_t stream);

}  // namespace wfa
