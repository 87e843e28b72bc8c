// wfa_leftalign.hpp — left alignment of the op strings of a full-scope batch, in place on the device (wfa_hip_batch_left_align).
//
// Rule (include/wfa_hip.h, "left alignment"; wfa_hip_ops_left_align in host_cigar.cpp is its plain statement for one pair, needing no
// GPU): inside the aligned core, first M .. last M, every maximal I or D run, in ascending op order over the string as already
// rewritten, moves left over M ops while the letter that enters the run at its left end equals the letter that leaves it at its right
// end (S[x - 1] == S[x + L - 1], S the text for I and the pattern for D); a run that has moved and meets a run of its own kind becomes
// one run with it and goes on.  An X, a gap of the other kind or the core's first M stops it.
//
// Kernel (k_leftalign.hip): one wave per pair, grid-stride, as the pileup.  One ballot pass over the string finds the first M, the last
// M and the first gap op behind the first M; a pair without a gap op inside its core — most short reads at a few per cent — leaves
// without a store.  The runs are then taken in order by the whole wave: the distance of a shift is found 64 candidates at a time (lane
// k tests ops[a - 1 - k] == 'M', a - 1 - k > first and S[x - 1 - k] == S[x + L - 1 - k]; the first failing lane ends it, 64 passing
// lanes ask for another round), and the min(distance, L) ops that change at either end of the stretch are stored by the lanes in
// parallel.  Letters come from the pair's 2-bit words (meta[q].p_woff / t_woff), or from its bytes (pboff / tboff) when the pair is
// flagged for the byte kernels.  The two statistics are device counters; a wave adds its own sums once, when it has moved something.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wfa_common.hpp"

namespace wfa {

struct LeftAlignArgs {
  // the batch (after its run); ops is rewritten in place
  uint8_t* ops; const int64_t* cigar_begin; const int32_t* cigar_len; const int32_t* status;
  const WfaPairMeta* meta;
  const uint32_t* words;     // the pairs' 2-bit letters (meta[q].p_woff, t_woff)
  const uint8_t* bytes;      // the bytes of the flagged pairs (pboff[q], tboff[q]); nullptr: no pair is flagged
  const int64_t* pboff; const int64_t* tboff;
  const uint8_t* flags;
  int64_t npairs;
  unsigned long long* stats; // [0] runs moved, [1] merges (zeroed by the host)
};

int launch_left_align(const LeftAlignArgs& a, int cu_count, hipStream_t stream);

}  // namespace wfa
