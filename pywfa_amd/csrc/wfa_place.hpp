// wfa_place.hpp — device-side result surface, per READ (wfa_hip_placer_*): the hits of any number of batches recorded where they lie,
// grouped by read, and every read reduced to one row — its primary hit, the runner-up at another locus, a mapping quality, counts —
// with one flag byte per hit.  32 bytes per read and 1 byte per hit cross PCIe.
//
// Rule (include/wfa_hip.h, "placement"; wfa_hip_place_host in host_place.cpp is its plain statement, needing no GPU).  A hit is
// eligible iff status == 0 && score >= min_score.  The primary p of a read is its eligible hit of greatest score, the smallest hit
// number on a tie.  Eligible h is at p's locus iff h != p, same j, same strand, and ov = min(te) - max(ts) has ov > 0 and
// 2 ov >= min(te_h - ts_h, te_p - ts_p).  second / ties are over the eligible hits that are neither p nor at its locus; mapq is 60
// without one, else min(60, 60 (score_p - second) / full_gap).
//
// Layout on the device, 37 bytes per hit: a 32-byte record (PlaceHit: two 16-byte loads), its 4-byte slot in the grouped order, its
// flag byte; per read a 4-byte counter and the 32-byte row.  The records are appended in hit-number order and never move: a hit's
// number is its index.
//
// Kernels (k_place.hip):
//   record   per pair of a batch after its run, one PlaceHit.  Scope full: a wave per pair, the walk of wfa_summary.hpp
//            (summary_scan: 64 ops per round, ballots) for the text bases in front of the first and behind the last M, so that the
//            interval is columns 8 and 9 of the summary; the same walk's pattern bases in front of the first and behind the last M,
//            each saturated at WFA_PLACE_CLIP_MAX, go into the record's clip word (the record stays 32 bytes).  Scope score: a
//            thread per pair, the whole window, clips 0.
//   group    count (a thread per hit, one atomicAdd on its read's counter), an inclusive scan of the nreads + 1 counters in the
//            three passes of the seed index's table (chunk sums, their prefix in one workgroup, apply: a counter becomes the END of
//            its group), scatter (a thread per hit: atomicSub on the counter gives its slot, the counter ends as the group's BEGIN,
//            counter[nreads] stays the number of hits).  The order inside a group depends on scheduling; nothing below does.
//   place    one wave per read, grid-stride; the lanes stride the group.  Pass 1: the wave-wide maximum of the 64-bit key
//            (score ^ 0x80000000) << 32 | ~hit number — greatest score, then smallest number; eligible keys are never 0.  Pass 2: the
//            same-locus test against p's record, the flags, and wave reductions for second (a maximum), ties, hits and the number
//            of runner-up candidates.  Groups longer than 64 loop; lanes 0 .. 7 store the row.  No LDS.
//            A READ WITH A VERY LARGE GROUP IS SERVED BY ONE WAVE (two passes of group / 64 rounds).
//   pair     (include/wfa_hip.h, "pairing"; wfa_hip_pair_host in host_pair.cpp is its plain statement.)  After group and place, so it
//            reads count / order, the single-end rows and the single-end flags in HBM.  One wave per fragment, grid-stride.  With
//            n1, n2 the sizes of the mates' groups, the lanes stride the n1 x n2 slot pairs p -> (p / n2, p % n2) — the slot pair
//            is advanced by (64 / n2, 64 % n2) a round, no division in the loop — and load both records (two 16-byte loads each);
//            a pair with an ineligible slot is skipped, not compacted, so the rounds of a pass are n1 n2 / 64 while the rule's
//            bound E1 E2 <= WFA_PAIR_MAX_PAIRINGS is on the eligible ones (E from the single-end rows; over the bound: no join).
//            Pass 1: the number of proper pairings and the best one by three wave-wide reductions: the maximum of the biased 64-bit
//            pair score, the minimum h among the lanes that hold it, the minimum g among those.  Lane 0 decides `proper` against
//            the single-end scores and broadcasts it.  Pass 2 (proper only): the same-place test against the two chosen records,
//            wave reductions for second, ties and the number of runner-up candidates.  Then the lanes stride each mate's group
//            once for pair_flags (which the host entry has filled with the single-end flags beforehand, a device copy: reads in
//            no fragment and fragments that are not proper keep them); lanes 0 .. 11 store the row.  No LDS, no atomics.
//   rescue   (include/wfa_hip.h, "rescue"; wfa_hip_rescue_host in host_rescue.cpp is its plain statement; k_rescue.hip.)  After pair,
//            so it reads the pair rows, the single-end rows and the records in HBM, and the length arrays of the two sequence sets.
//            2 nfrag slots, slot s = (fragment s / 2, anchoring mate s % 2), a thread per slot, grid-stride.  decide: the pair row's
//            proper / pairings / overflow, the anchoring mate's single-end hit and mapq, the anchor's record (two 16-byte loads),
//            len(o) and tlen(j_a); it writes 0 / 1 at counter s + 1 (counter 0 is 0).  The scan of the group step
//            (launch_place_scan) over the 2 nfrag + 1 counters makes counter s the EXCLUSIVE prefix of slot s and the last one the
//            number of windows.  emit recomputes the window and stores its 32-byte row at counter s as two 16-byte stores, when
//            that is below the caller's capacity.  The order is the scan's, never arrival order; no atomics, no LDS but the scan's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wfa_common.hpp"

namespace wfa {

#define WFA_PLACE_COLS 8
#define WFA_PLACE_SCAN_CHUNK 4096   // counters per workgroup of the scan: 256 threads x 16
#define WFA_PLACE_CLIP_MAX 65535    // a clip saturates here: two of them share the record's last word

struct alignas(16) PlaceHit {
  int32_t i, j, reverse, status;   // read, text, strand (0 / 1), the pair's status
  int32_t score, ts, te, clips;    // its score, the text interval [ts, te) in coordinates of text j; clips: lead | trail << 16
                                   // (include/wfa_hip.h, "clips": the pattern bases in front of the first and behind the last M)
};

struct PlaceRecordArgs {
  // the batch (after its run)
  const int32_t* score; const int32_t* status; const WfaPairMeta* meta;
  const uint8_t* ops; const int64_t* cigar_begin; const int32_t* cigar_len;   // scope full only
  int64_t npairs;
  // the list
  const int32_t* i; const int32_t* j;
  const int32_t* t_start;    // [npairs] or nullptr: 0
  const uint8_t* reverse;    // [npairs] or nullptr: forward
  PlaceHit* out;             // [npairs]: the placer's records from its first free one
};

struct PlaceArgs {
  const PlaceHit* hits; int64_t nhits;
  int64_t nreads;
  uint32_t* count;           // [nreads + 1]: zero before the count pass; ends after the scan; begins (and [nreads] = nhits) after the scatter
  uint32_t* bsum;            // [ceil((nreads + 1) / WFA_PLACE_SCAN_CHUNK)]
  uint32_t* order;           // [nhits] hit numbers, group by group
  int32_t min_score, full_gap;
  int32_t* rows;             // [nreads x WFA_PLACE_COLS]
  uint8_t* flags;            // [nhits]
};

// the clip word of a record, and its halves
__host__ __device__ inline int32_t place_clip_word(int64_t lead, int64_t trail) {
  const uint32_t l = (uint32_t)(lead < 0 ? 0 : lead > WFA_PLACE_CLIP_MAX ? WFA_PLACE_CLIP_MAX : lead);
  const uint32_t t = (uint32_t)(trail < 0 ? 0 : trail > WFA_PLACE_CLIP_MAX ? WFA_PLACE_CLIP_MAX : trail);
  return (int32_t)(l | (t << 16));
}
__host__ __device__ inline int32_t place_clip_lead(int32_t word) { return (int32_t)((uint32_t)word & 0xffffu); }
__host__ __device__ inline int32_t place_clip_trail(int32_t word) { return (int32_t)((uint32_t)word >> 16); }

int launch_place_record(const PlaceRecordArgs& a, bool full, int cu_count, hipStream_t stream);
int launch_place_scan(uint32_t* count, int64_t n, uint32_t* bsum, hipStream_t stream);   // count[0 .. n) to its inclusive prefix, in place
int launch_place_group(const PlaceArgs& a, hipStream_t stream);   // count, scan, scatter (a.count zeroed by the caller)
int launch_place(const PlaceArgs& a, int cu_count, hipStream_t stream);

#define WFA_PAIR_COLS 12
#define WFA_PAIR_MAX_PAIRINGS 65536

struct PairArgs {
  PlaceArgs place;           // after launch_place_group and launch_place: count / order, rows and flags (flags never nullptr here)
  int32_t min_insert, max_insert, unpaired;
  int64_t nfrag;
  const int32_t* mate1;      // [nfrag], or both nullptr: fragment f is reads 2 f and 2 f + 1
  const int32_t* mate2;
  int32_t* pair_rows;        // [nfrag x WFA_PAIR_COLS]
  uint8_t* pair_flags;       // [nhits] holding the single-end flags, or nullptr
};

int launch_pair(const PairArgs& a, int cu_count, hipStream_t stream);

#define WFA_RESCUE_COLS 8

struct RescueArgs {
  PairArgs pair;             // after launch_pair: the records, the single-end rows and the pair rows
  const int32_t* read_len; int64_t npatterns;   // the pattern set's lengths (npatterns >= place.nreads: the host has checked)
  const int32_t* text_len; int64_t ntexts;      // the text set's lengths (every j < ntexts: the host has checked)
  int32_t pad, min_len, anchor_mapq;
  uint32_t* slot;            // [2 nfrag + 1]: slot[0] = 0 and slot[s + 1] = 0 / 1 after decide; exclusive prefixes (slot[2 nfrag]: the count) after the scan
  uint32_t* bsum;            // [ceil((2 nfrag + 1) / WFA_PLACE_SCAN_CHUNK)]
  int64_t cap;               // rows of `out`
  int32_t* out;              // [cap x WFA_RESCUE_COLS], 16-byte aligned
};

int launch_rescue(const RescueArgs& a, int cu_count, hipStream_t stream);   // decide, scan, emit

}  // namespace wfa
