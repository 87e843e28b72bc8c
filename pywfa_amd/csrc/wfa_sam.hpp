// wfa_sam.hpp — the SAM fields of every pair of a full-scope batch, made on the device (wfa_hip_batch_sam_counts / _sam_strings).
//
// Rule (include/wfa_hip.h, "SAM fields"; wfa_hip_ops_sam in host_sam.cpp is its plain statement for one pair, needing no GPU): the
// span is first anchor op .. last anchor op (M and X, or M alone under WFA_HIP_SAM_CORE); the row counts ops in front of, inside and
// behind it; the CIGAR is the span's maximal runs with the letters swapped (the library's D is SAM's I) between two soft clips; the MD
// string is the span's match runs, mismatched text letters and deleted text letters.
//
// Kernels (k_sam.hip): one wave per pair, grid-stride, 64 ops a round, as wfa_rle_kernel and the left-align kernel; no atomics, no LDS.
//   pass 1  ballots find the span, popcounts under masks give the row, the two string lengths are the sums of the lanes' token
//           lengths: rows[q] (8 int32).
//   scan    launch_scan64 (k_select.hpp) over columns 5 and 6: cigar_off[0 .. n], md_off[0 .. n], 64-bit, on the device.
//   pass 2  the same walk; a wave prefix sum of the token lengths plus a carry across rounds gives every lane the place of its token,
//           and the lane stores its bytes.  An UNMAPPED pair stores nothing.
// A CIGAR token is emitted by the lane at its run's LAST op (the run's length is not known at its first op when it crosses a round);
// the run's start is the highest run start at or below the lane, or the one carried in.  An MD number is emitted by the lane of the
// event behind it (an X, or the first I of a run) from the M ops since the last event, carried across rounds; the final number after
// the last round.  Letters come from the pair's 2-bit words (meta[q].t_woff), or from its bytes (tboff) when the pair is flagged for
// the byte kernels, exactly as the left-align kernel reads them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wfa_common.hpp"

#define WFA_SAM_COLS 8

namespace wfa {

struct SamArgs {
  // the batch (after its run, and after a left alignment if there was one)
  const uint8_t* ops; const int64_t* cigar_begin; const int32_t* cigar_len; const int32_t* status;
  const WfaPairMeta* meta;
  const uint32_t* words;     // the pairs' 2-bit letters (meta[q].t_woff)
  const uint8_t* bytes;      // the bytes of the flagged pairs (tboff[q]); nullptr: no pair is flagged
  const int64_t* tboff;
  const uint8_t* flags;
  int64_t npairs;
  int sam_flags;             // WFA_HIP_SAM_EQX | WFA_HIP_SAM_CORE
  int32_t* rows;             // npairs x WFA_SAM_COLS: written by pass 1, read by pass 2
  // pass 2
  const uint64_t* cigar_off; const uint64_t* md_off;   // npairs + 1 each: the scans of columns 5 and 6
  uint8_t* cigar; uint8_t* md;                         // cigar_off[npairs] and md_off[npairs] bytes
};

int launch_sam_counts(const SamArgs& a, uint64_t* cigar_off, uint64_t* md_off, int cu_count, hipStream_t stream);   // pass 1 and the two scans
int launch_sam_strings(const SamArgs& a, int cu_count, hipStream_t stream);                                          // pass 2

}  // namespace wfa
