// wfa_insertions.hpp — what the reads insert: the pileup's optional log of insertion records and its reduction to one allele per
// reported row (wfa_hip_pileup_track_insertions / _insertion_stats / _insertions).
//
// Rule (include/wfa_hip.h, "insertions"; wfa_hip_ops_insertions / wfa_hip_insertions_host in host_cigar.cpp are its plain statement,
// needing no GPU): every maximal D run of a contributing pair's aligned core that the pileup counts into column 6 is one record
// (g, n, letters): g the global row the run increments, n its length, letters the columns 0..4 of pattern[v .. v + n).  The allele
// of a row is the (n, letters) with the most records; ties go to the smaller n, then to the lexicographically smaller columns.
//
// Record side (k_pileup.hip): the log is two arrays that grow by doubling, InsRecord[records] and one column byte per inserted
// base.  An add with tracking on is count -> exclusive scan -> scatter, no atomics for the log:
//   count    wfa_pileup_kernel<PILEUP_COUNT>: a wave per pair, the walk of the table kernel without a store to the table;
//            pair_count[q] = {records, inserted bases} of pair q (zero for a pair that does not contribute)
//   scan     wfa_scan64_kernel twice (k_select.hpp, k_calls.hip): the exclusive 64-bit prefixes, the two totals behind them
//            (downloaded: 16 bytes; the log grows before anything is added)
//   scatter  wfa_pileup_kernel<PILEUP_TRACK>: the table kernel, which also writes pair q's records from its scanned record offset and
//            its column bytes from its scanned base offset.  Every D op of a counted run writes its own column byte (its place: the
//            pair's base offset + the counted D ops in front of it); the lane at a run's start writes the record when the run ends
//            inside the 64-op round, otherwise the run stays OPEN: its row, its place in the two arrays and its length so far are
//            carried wave-uniformly into the next rounds, and lane 0 writes the record in the round where the run ends.
//
// Reduction (k_insertions.hip), wfa_hip_pileup_insertions:
//   select   the chunk count / scan / scatter of the sites (wfa_calls.hpp, k_select.hpp) under event_selected(depth, c6): the selected
//            rows' global indices in ascending order, their row columns j, pos, depth, ins_count, overflow, and a bucket size per
//            row (c6; 0 for an overflow row)
//   scan     the bucket sizes -> bucket offsets
//   fill     (k_select.hpp, shared with the deletions) a thread per record of the log: a binary search of its row among the selected
//            ones; a record on a selected row takes the next free slot of that row's bucket (an atomic counter per row: the order
//            inside a bucket is whatever scheduling gives, and nothing that is written out depends on it)
//   reduce   a wave per row: every record's multiplicity among the bucket's records, the best under the total order above, and the
//            number of distinct alleles (the records without an equal one in a lower slot) -> allele_count, allele_len, alleles
//   scan     allele_len -> the letters' offsets, the last one the total
//   letters  a wave per row: the best record's columns as ASCII A C G T N at the row's offset
// The work of the one wave that serves a row is bounded by WFA_HIP_INS_MAX_READS (records per row; more: an overflow row).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wfa_calls.hpp"

namespace wfa {

#define WFA_INSERTION_COLS 8

struct InsRecord {
  int64_t g;        // global row: seq_off[j] + t_start + h
  int64_t off;      // first column byte of the run in the base log
  int32_t n;        // the run's length
  int32_t spare;
};
static_assert(sizeof(InsRecord) == 24, "24 bytes per record (include/wfa_hip.h states the cost)");

struct InsPairCount { uint32_t records, bases; };

// the record side of an add: what the count and track kernels take beside PileupArgs
struct InsLogArgs {
  InsPairCount* pair_count;     // [npairs]           COUNT writes, the scans read
  uint64_t* rec_off;            // [npairs + 1]       the scan writes; TRACK: pair q's first record, relative to rec_base
  uint64_t* base_off;           // [npairs + 1]       the scan writes; TRACK: pair q's first column byte, relative to base_base
  InsRecord* records;           // the log
  uint8_t* bases;
  int64_t rec_base, base_base;  // records / bytes of the log before this add
  int64_t rec_cap, base_cap;    // allocated records / bytes: no store at or behind them
};

struct InsArgs {
  CallsArgs c;                  // the table, the run [g0, g0 + n), the parameters, the chunks (ref unused: the rule needs no letters)
  int32_t max_reads;
  // the selected rows
  int64_t nsel;
  int64_t* sel_g;               // [nsel] ascending global index
  uint32_t* bucket_size;        // [nsel] c6, 0 for an overflow row
  uint64_t* bucket_off;         // [nsel + 1]
  uint32_t* bucket_fill;        // [nsel] zeroed: the slots taken
  int64_t* bucket;              // [bucket_off[nsel]] record indices
  int32_t* rows;                // [nsel x WFA_INSERTION_COLS]
  int64_t* best;                // [nsel] the record whose letters are the row's allele (-1: none)
  uint32_t* allele_len;         // [nsel]
  uint64_t* letter_off;         // [nsel + 1]
  uint8_t* letters;             // the letters that are asked for: a prefix of letter_off[nsel] bytes
  // the log
  const InsRecord* records; const uint8_t* bases; int64_t nrec;
};

// the record side (k_pileup.hip): the count form of the table kernel + the two scans; the tracking form is launch_pileup's (wfa_pileup.hpp)
int launch_pileup_count(const PileupArgs& a, const InsLogArgs& g, int cu_count, hipStream_t stream);

int launch_ins_select_count(const InsArgs& a, hipStream_t stream);   // count + scan: c.chunk_off[c.chunks] is the number of rows
int launch_ins_select(const InsArgs& a, hipStream_t stream);         // scatter of the rows + the scan of the bucket sizes
int launch_ins_reduce(const InsArgs& a, int64_t nbases, int cu_count, hipStream_t stream);   // fill + reduce + the scan of allele_len (nbases: bytes of the log)
// the letters of the first out_rows rows that end at or before out_bases
int launch_ins_letters(const InsArgs& a, int64_t out_rows, int64_t out_bases, int cu_count, hipStream_t stream);

}  // namespace wfa
