// wfa_cross.hpp — all-vs-all and many-vs-many score matrices (wfa_hip_cross_run, csrc/wfa_hip.hip): the pair metadata of a band of
// the cross product, generated on the device from two sequence sets packed once (wfa_hip_seqset_create), and what is done with the
// band's results (scatter into the dense matrix, ordered compaction of the completed pairs).  Kernels in k_cross.hip.
//
// Layout.  A set is one word-aligned run of 2-bit words per sequence (the batch layout of wfa_pack.hpp).  A run joins the sets' words
// in one table (the text set's offsets shifted behind the pattern set's) followed by one slot per band pair: the register stages
// (wfa_lane.hpp, wfa_seg.hpp) fetch a pair's pattern and text words in ONE load, the text's right behind the pattern's, so the
// generator copies both sequences of a pair of up to WFA_FAST_MAX_LEN bases into its slot; a longer pair points into the sets' words
// (every other stage reads pattern and text through their own offsets).  A band = rows r0 .. r1 of the rectangle (all n columns:
// band pair q = (q / n, q % n)) or of the upper triangle (columns j >= i: pair q is global triangular index tri0 + q, decoded exactly
// in integers).  Pairs holding a letter outside ACGT (either sequence flagged, or every pair when the wildcard is one of ACGT) are
// aligned on their bytes: their slot in the band's byte work list follows from two host prefix sums (byte pairs per row, flagged
// columns), so the band's 2-bit / byte split is known on the host without reading anything back.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wfa_common.hpp"

namespace wfa {

struct CrossGenArgs {
  const uint32_t* p_woff; const int32_t* p_len; const int64_t* p_boff; const uint8_t* p_flag;   // rows (pattern set)
  const uint32_t* t_woff; const int32_t* t_len; const int64_t* t_boff; const uint8_t* t_flag;   // columns (text set)
  uint32_t* words;          // the run's word table: the sets' words, then a slot of slot_words per band pair (from slot_base)
  uint32_t slot_base, slot_words;
  uint32_t t_wshift;        // the text set's first word in the table
  int64_t t_bshift;         // ... and its first byte in the joined byte blob
  const int64_t* row_bytes; // [rows + 1]: byte pairs in the rows before row i (the whole rectangle / triangle)
  const int64_t* col_flag;  // [n + 1]: flagged columns before column j
  int64_t n;                // columns
  int64_t r0;               // first row of the band
  int64_t tri0;             // triangle: global index of the band's first pair
  int64_t npairs;
  int tri;                  // 1: upper-triangle band (columns j >= i)
  int all_bytes;            // 1: every pair on its bytes (the wildcard is one of ACGT)
  int lists;                // 1: the band holds byte pairs: write both work lists
  WfaPairMeta* meta;
  int64_t* pboff;
  int64_t* tboff;
  uint8_t* flags;
  uint32_t* list_packed;
  uint32_t* list_bytes;
};

struct CrossResArgs {
  const int32_t* score;     // the band's results (pair q)
  const int32_t* status;
  int64_t n, r0, tri0, npairs;
  int tri;
  int upper;                // completed pairs: keep j > i only (all-vs-all)
  int mirror;               // scatter: also write (j, i)
  int32_t* dense_score;     // scatter: the M x N matrix
  int32_t* dense_status;
  uint32_t* blk_count;      // compaction: per-workgroup counts, then (scan) their exclusive prefix
  uint32_t* band_count;     // compaction: the band's total
  int32_t* out_i;           // compaction: the band's list, band-local positions
  int32_t* out_j;
  int32_t* out_score;
};

#define WFA_CROSS_CHUNK 4096   // pairs per workgroup of the compaction (256 threads x 16 rounds)

int launch_cross_gen(const CrossGenArgs& a, hipStream_t stream);
int launch_cross_scatter(const CrossResArgs& a, hipStream_t stream);
int launch_cross_compact(const CrossResArgs& a, hipStream_t stream);

}  // namespace wfa
