// wfa_deletions.hpp — what the reads delete: the pileup's optional log of deletion runs, its starts plane, and the reduction to one
// deletion length per reported row (wfa_hip_pileup_track_deletions / _deletion_stats / _read_deletion_starts / _deletions).
//
// Rule (include/wfa_hip.h, "deletions"; wfa_hip_ops_deletions / wfa_hip_deletions_host in host_cigar.cpp are its plain statement,
// needing no GPU): every maximal I run of a contributing pair's aligned core is one record (g, n): g the global row of the run's first
// deleted base, n its length.  starts[g] counts the records that start at row g; the allele of a row is the n with the most records
// among those that start there, ties to the smaller n.  The records that COVER a row are that row's column 5.
//
// Record side (k_deletions.hip): the log is one array that grows by doubling, DelRecord[records]; the starts plane is one int32 per
// text base, zeroed when tracking is turned on.  The table kernels do not know of the log: an add with tracking on runs them as
// ever and then one more pass over the op strings, count -> exclusive scan -> scatter:
//   count    wfa_del_count_kernel: a wave per pair, the core and h found as pileup_walk finds them (h = the running base + the
//            popcount of the text-consuming ballot below the lane); pair_count[q] = {records, deleted bases} of pair q (zero for a
//            pair that does not contribute).  A run's start is an I whose predecessor — the lane below, or the last op of the previous
//            round — is not a counted I.
//   scan     wfa_scan64_kernel twice (k_select.hpp, k_calls.hip): the exclusive 64-bit prefixes, the two totals behind them
//            (downloaded: 16 bytes; the log grows before anything is written)
//   scatter  wfa_del_scatter_kernel: the same walk; the lane at a run's start writes (g, n) at the pair's scanned offset + the starts
//            in front of it when the run ends inside the 64-op round, otherwise the run stays OPEN (the scheme wfa_insertions.hpp
//            describes for D runs): its row, its slot and its length so far are carried wave-uniformly into the next rounds, and lane 0
//            writes the record in the round where the run ends.  Whoever writes a record makes its one no-return atomicAdd on
//            starts[g].  There is no letter array: the reference has the letters.
// An I op is counted under the condition of the table kernel's column 5 (inside the core, h < tlen), so a run of an op string that
// outran its pair is cut where column 5 stops counting it, and g always lies inside the pair's text, hence inside the plane.
//
// Reduction (k_deletions.hip), wfa_hip_pileup_deletions:
//   select   the chunk count / scan / scatter of the sites (wfa_calls.hpp, k_select.hpp) under event_selected(depth, S = starts[g]):
//            the selected rows' global indices in ascending order, their columns j, pos, depth, del_count, overflow, and a bucket size
//            per row (S; 0 for an overflow row)
//   scan     the bucket sizes -> bucket offsets
//   fill     (k_select.hpp, shared with the insertions) a thread per record of the log: a binary search of its row among the selected
//            ones; a record on a selected row puts its length into the next free slot of that row's bucket (an atomic counter per
//            row: the order inside a bucket is whatever scheduling gives, and nothing that is written out depends on it)
//   reduce   a wave per row: every length's multiplicity among the bucket's lengths, the best under (count descending, n ascending),
//            and the number of distinct lengths (the slots without an equal one in a lower slot)
// The work of the one wave that serves a row is bounded by WFA_HIP_DEL_MAX_READS (records per row; more: an overflow row).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wfa_calls.hpp"

namespace wfa {

#define WFA_DELETION_COLS 8

struct DelRecord {
  int64_t g;        // global row of the first deleted base: seq_off[j] + t_start + h
  int32_t n;        // the run's length
  int32_t spare;
};
static_assert(sizeof(DelRecord) == 16, "16 bytes per record (include/wfa_hip.h states the cost)");

struct DelPairCount { uint32_t records, bases; };

// the record side of an add: what the count and scatter kernels take beside PileupArgs
struct DelLogArgs {
  DelPairCount* pair_count;     // [npairs]           count writes, the scans read
  uint64_t* rec_off;            // [npairs + 1]       the scan writes; scatter: pair q's first record, relative to rec_base
  uint64_t* base_off;           // [npairs + 1]       the scan writes; its last entry is the deleted bases of the add
  DelRecord* records;           // the log
  int64_t rec_base;             // records of the log before this add
  int64_t rec_cap;              // allocated records: no store at or behind them
  int32_t* starts;              // [PileupArgs::total] the starts plane
};

struct DelArgs {
  CallsArgs c;                  // the table, the run [g0, g0 + n), the parameters, the chunks (ref unused: the rule needs no letters)
  const int32_t* starts;        // [c.total]
  int32_t max_reads;
  // the selected rows
  int64_t nsel;
  int64_t* sel_g;               // [nsel] ascending global index
  uint32_t* bucket_size;        // [nsel] S, 0 for an overflow row
  uint64_t* bucket_off;         // [nsel + 1]
  uint32_t* bucket_fill;        // [nsel] zeroed: the slots taken
  int32_t* bucket;              // [nrec] the lengths of the records, row by row
  int32_t* rows;                // [nsel x WFA_DELETION_COLS]
  // the log
  const DelRecord* records; int64_t nrec;
};

int launch_del_count(const PileupArgs& a, const DelLogArgs& g, int cu_count, hipStream_t stream);     // count + the two scans
int launch_del_scatter(const PileupArgs& a, const DelLogArgs& g, int cu_count, hipStream_t stream);   // the records and the starts plane

int launch_del_select_count(const DelArgs& a, hipStream_t stream);   // count + scan: c.chunk_off[c.chunks] is the number of rows
int launch_del_select(const DelArgs& a, hipStream_t stream);         // scatter of the rows + the scan of the bucket sizes
int launch_del_reduce(const DelArgs& a, int cu_count, hipStream_t stream);   // fill + reduce

}  // namespace wfa
