// wfa_dup.hpp — duplicate marking after placement (wfa_hip_placer_duplicates): the fragments and reads of a placer that lie at the same
// place with the same ends, grouped on the device where the records lie; 16 bytes per read and per fragment cross PCIe.
//
// Rule (include/wfa_hip.h, "duplicates"; wfa_hip_duplicates_host in host_dup.cpp is its plain statement, needing no GPU).  After group,
// place and pair: a PAIR UNIT is a proper fragment, key (j, ts_F, te_R, first), score the pair row's, bucket position ts_F; a READ UNIT
// is a read that no pair unit owns and whose single-end primary has a non-empty interval, key (j, reverse, p5), p5 = ts forward and
// te - 1 reverse, score the single-end one's, bucket position p5.  A group is the units of one kind with equal keys, its representative
// the unit of greatest score, then of smallest number.  A bucket — all units of one (j, b) — above WFA_DUP_MAX_BUCKET units is not
// resolved: each of its units is alone with overflow = 1.  A unit whose b is outside its text is alone with overflow = 0.
// Under WFA_DUP_UNCLIPPED the coordinates of keys and buckets are the unclipped ones (ts - lead, te + trail, from the clip word of the
// records the key kernels load anyway); `end` then carries ue_R and the bucket us_F, so the record stays 32 bytes and scan, scatter
// and resolve are the same.  Under WFA_DUP_BY_QUALITY a unit's score is the summed base quality of its read(s), from qsum[].
//
// Layout on the device, kept on the placer from the first call on: a plane of one 4-byte counter per base of the text set and one
// more, direct-addressed by the set's resident base offsets (bucket = boff[j] + b), with the scan's chunk sums; 32 bytes per read for
// the unit records (DupUnit: two 16-byte loads) and 32 more for their bucket-ordered copy; one byte per read that says who owns it.
// THE PLANE GROWS WITH THE TEXT SET, NOT WITH THE READS; a hashed plane is not built.  A unit's record lies at the slot of its read
// (a read unit) or of its mate 1 (a pair unit): a read is in at most one fragment, so no two units share a slot.
//
// Kernels (k_dup.hip), after the pair kernel, so they read the pair rows, the single-end rows and the records in HBM:
//   qsum     (WFA_DUP_BY_QUALITY only, before key.)  A wave per read, grid-stride.  The read's bytes between its first and last 16-byte
//            boundary are taken as 16-byte loads, a lane a chunk; the up to 15 bytes in front and behind by one predicated byte load
//            a lane: NO LOAD TOUCHES A BYTE OUTSIDE THE READ.  Per byte a compare with min_quality and an add, 64-bit lane sums, a
//            wave reduction by shuffles, lane 0 stores the sum saturated to INT32_MAX.  No LDS, no atomics.
//   key      two launches.  fragments: a thread per fragment, grid-stride.  A proper fragment marks its mates in the owner plane (1 for
//            mate 1, whose slot holds the record, 2 for mate 2), loads its two chosen records and, with b inside the text, stores the
//            unit record and does one atomicAdd on plane[bucket]; with b outside it stores its final row (alone) and an empty record.
//            Any other fragment stores the row -1, 0, 0, 0.  reads: a thread per read.  An owner byte of 1 leaves the slot alone, 2
//            empties it; a read nobody owns is a read unit (record and atomicAdd, or its final row when b is outside the text) or no
//            unit (row -1, 0, 0, 0 and an empty record).  Every slot and every row that resolve does not write is written here.
//   scan     launch_place_scan (k_place.hip) over the nbases + 1 counters: a counter becomes the END of its bucket.
//   scatter  a thread per slot: atomicSub on the counter gives a record its place in bucket order, the counter ends as the bucket's
//            BEGIN and plane[nbases] stays the number of units; the record is copied there with two 16-byte stores.  The order
//            inside a bucket is arrival order; nothing below depends on it.
//   resolve  a thread per bucket-ordered record, grid-stride.  A bucket above the cap: the overflow row.  Otherwise it walks the
//            bucket's records (contiguous) and keeps, over the members whose kind and end equal its own, their number and the maximum
//            of the 64-bit key (score ^ 0x80000000) << 32 | ~unit — greatest score, then smallest number: both are order-free.  One
//            16-byte store per row; a pair unit also stores -1, 0, dup, overflow for its two mates.  No LDS.  Typical buckets hold
//            1 - 3 records; the cap bounds the walk at WFA_DUP_MAX_BUCKET records a thread.
#pragma once
#include "wfa_place.hpp"

namespace wfa {

#define WFA_DUP_COLS 4
#define WFA_DUP_MAX_BUCKET 4096
#define WFA_DUP_UNCLIPPED 1     // DupArgs::flags: keys and buckets on the unclipped ends
#define WFA_DUP_BY_QUALITY 2    // DupArgs::flags: scores from qsum

struct alignas(16) DupUnit {
  int64_t bucket;            // boff[j] + b, inside [0, nbases)
  int32_t kind, end;         // 0: no unit; pair units: `first` (1 / 2) and te_R; read units: 3 forward / 4 reverse and 0
  int32_t score, unit;       // the unit's score and number (fragment or read)
  int32_t m1, m2;            // pair units: the two mates' reads; read units: -1
};

struct DupArgs {
  PairArgs pair;             // after launch_pair: the records, the single-end rows and the pair rows
  const int64_t* boff;       // the text set's base offsets, lengths and number of sequences (every j < ntexts: the host has checked)
  const int32_t* text_len; int64_t ntexts;
  int64_t nbases;            // the bases of the text set
  uint32_t* plane;           // [nbases + 1]: zero before key; bucket ends after the scan; bucket begins ([nbases]: the units) after scatter
  uint32_t* bsum;            // [ceil((nbases + 1) / WFA_PLACE_SCAN_CHUNK)]
  DupUnit* rec;              // [nreads] by slot
  DupUnit* sorted;           // [nreads] in bucket order, the first plane[nbases] in use
  uint8_t* owned;            // [nreads]: zero before key
  int32_t* read_rows;        // [nreads x WFA_DUP_COLS], 16-byte aligned
  int32_t* frag_rows;        // [nfrag x WFA_DUP_COLS], 16-byte aligned (pair.pair_rows are the pairing's)
  int flags;                 // WFA_DUP_UNCLIPPED: keys and buckets on the unclipped ends; WFA_DUP_BY_QUALITY: scores from qsum
  const int32_t* qsum;       // [nreads] after launch_dup_qsum, under WFA_DUP_BY_QUALITY (else nullptr)
};

// the summed base qualities of every read (k_dup.hip: a wave per read)
struct DupQsumArgs {
  const uint8_t* quals;      // the quality set's bytes, read r at off[r], len[r] of them
  const int64_t* off; const int32_t* len;
  int64_t nreads;
  int32_t min_quality;
  int32_t* qsum;             // [nreads]
};

int launch_dup_qsum(const DupQsumArgs& a, int cu_count, hipStream_t stream);

int launch_dup(const DupArgs& a, int cu_count, hipStream_t stream);   // key, scan, scatter, resolve (plane and owned zeroed by the caller)

}  // namespace wfa
