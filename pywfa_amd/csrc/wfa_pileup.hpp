// wfa_pileup.hpp — device-side result surface, per reference position (wfa_hip_pileup_*): the pairs of a full-scope batch taken as
// reads (patterns) aligned against windows of a resident text set, reduced into per-base counters where the op strings lie.
//
// Rule (include/wfa_hip.h; wfa_hip_ops_pileup in host_cigar.cpp is its plain statement for one pair, needing no GPU): walk the op
// string with pattern position v and text position h from 0; only the ops of the aligned core, first M .. last M, add, to row
// g = t_start + h of the pair's text:
//   M  +1 to the column of pattern letter v                        v, h advance
//   X  +1 to the column of pattern letter v, +1 to `mismatch`      v, h advance
//   I  +1 to `deleted` (a text base the read lacks)                h advances
//   D  +1 to `insertion-before`, once per maximal D run            v advances
// Columns: A C G T other | deleted | insertion-before | mismatch (WFA_PILEUP_COLS).
//
// Table layout on the device: one PLANE per column, plane c = table[c * total .. + total), a text base's place in a plane its
// sequence's prefix offset plus its position.  The lanes of a wave hold neighbouring ops of one pair, hence neighbouring rows g: in
// this layout the atomics of a wave's M ops on one letter fall into one or two 256-byte stretches of that letter's plane, where a
// row-major table (8 counters per base) would spread them over 64 rows of 32 bytes each (the one-lane-per-row shape).
//
// Kernel (k_pileup.hip; wfa_pileup_kernel<MODE, STRANDS, QUALS>, one launcher, launch_pileup): one wave per pair, grid-stride; a first
// pass finds the first and the last M with ballots (as the location pass of wfa_rle.hpp), a second pass takes 64 ops per round: v and
// h of a lane are the running bases plus the popcounts of the pattern- / text-consuming ballots below the lane; at most two no-return
// int32 atomicAdds per op.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wfa_common.hpp"

namespace wfa {

#define WFA_PILEUP_COLS 8
#define WFA_PILEUP_DEL 5
#define WFA_PILEUP_INS 6
#define WFA_PILEUP_MISMATCH 7

// column of an ASCII pattern letter / of a 2-bit code (A 0, C 1, T 2, G 3: wfa_hip_pack_2bit)
__host__ __device__ inline int wfa_pileup_letter_col(uint32_t c) {
  return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 4;
}
__host__ __device__ inline int wfa_pileup_code_col(uint32_t code) { return (int)((code ^ (code >> 1)) & 3u); }

struct PileupArgs {
  // the batch (after its run)
  const uint8_t* ops; const int64_t* cigar_begin; const int32_t* cigar_len; const int32_t* status;
  const WfaPairMeta* meta;
  const uint32_t* words;     // the pairs' 2-bit patterns (meta[q].p_woff)
  const uint8_t* bytes;      // the bytes of the flagged pairs (pboff[q]); nullptr: no pair is flagged
  const int64_t* pboff;
  const uint8_t* flags;
  int64_t npairs;
  // the list
  const int32_t* j;          // [npairs] text sequence of pair q
  const int32_t* t_start;    // [npairs] or nullptr: 0
  const uint8_t* keep;       // [npairs] or nullptr: every pair
  // the table
  const int64_t* seq_off;    // [nseq] first base of a sequence in a plane
  const int32_t* seq_len;    // [nseq]
  int64_t nseq;
  int64_t total;             // bases of the set = the plane stride
  int32_t* table;            // WFA_PILEUP_COLS planes
};

// Strands (include/wfa_hip.h, "strands and genotypes"; opt-in): a pileup that tracks them keeps a second table of the same 8 planes,
// plane stride and layout, the FORWARD table: a pair with reverse[q] == 0 makes every add a second time, at the same row and column
// of that table.  Reverse counts are total - forward and are never stored.  A pair's strand is uniform over its wave, so the second
// atomicAdd brings no divergence; a kernel compiled without the flag never reads this struct.
struct PileupStrandArgs {
  const uint8_t* reverse;    // [npairs] or nullptr: every pair is forward
  int32_t* fwd;              // WFA_PILEUP_COLS planes of PileupArgs::total counters
};

// Base qualities (include/wfa_hip.h, "base qualities"; opt-in): a pileup that tracks them keeps one more table of the same 8 planes,
// plane stride and layout, the QUALITY table, and every op that adds a count adds a capped phred value at the same row and column of
// it.  The quality of pattern position v of pair q is that of the stored read i[q], seen through the window [s, s + plen) with
// s = p_start[q]: byte s + v of a forward pair, s + plen - 1 - v of a reverse one.  An M or X whose quality lies under
// min_base_quality adds nothing to any table.  One byte load per lane (two on an I op), contiguous over the wave; the strand is the
// pair's, so the direction is uniform over the wave.  A kernel compiled without the flag never reads this struct.
struct PileupQualArgs {
  const uint8_t* quals;      // the quality set's bytes, raw phred, read after read
  const int64_t* qoff;       // [nreads] first byte of a read
  const int32_t* qlen;       // [nreads]
  int64_t nreads;
  const int32_t* i;          // [npairs] read of pair q
  const int32_t* p_start;    // [npairs] or nullptr: 0
  const uint8_t* reverse;    // [npairs] or nullptr: every pair is forward
  int32_t min_base_quality, quality_cap;
  int32_t* qtab;             // WFA_PILEUP_COLS planes of PileupArgs::total sums
};

// The table kernel in the form its arguments ask for (k_pileup.hip): g: with the insertion log's records and column bytes (the count
// pass before it: launch_pileup_count, wfa_insertions.hpp); s: and the forward table; u: and the quality table.  nullptr: without.
struct InsLogArgs;
int launch_pileup(const PileupArgs& a, const InsLogArgs* g, const PileupStrandArgs* s, const PileupQualArgs* u, int cu_count, hipStream_t stream);

}  // namespace wfa
