// wfa_cross.hpp — all-vs-all and many-vs-many score matrices (wfa_hip_cross_run, csrc/wfa_hip.hip): the pair metadata of a band of
// the cross product, generated on the device from two sequence sets packed once (wfa_hip_seqset_create), and what is done with the
// band's results (scatter into the dense matrix, ordered compaction of the completed pairs, top-k per row).  Kernels in k_cross.hip.
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

// Top-k per row (wfa_hip_cross_run_k, WFA_HIP_CROSS_TOPK).  A candidate is one 64-bit key, ((uint32)(score ^ 0x80000000) << 32) |
// (uint32)~j: the k best cells of a row are its k largest keys (larger score first, then smaller j); key 0 is "empty" (it decodes to
// j = -1, score = INT32_MIN) and no cell has it.  Every wave keeps a list of 64 keys sorted in descending order across its lanes (lane t:
// rank t) and a wave-uniform bar, the list's k-th key: cells that beat it are compacted into 128 keys of LDS by ballot, and the list is
// merged with them (bitonic, across lanes) only when 64 are waiting.  Per band, after the band's alignment, in two launches on the stream:
//  * row pass (only where a band row is longer than `chunk`): one wave per (band row, chunk of `chunk` cells) writes its chunk's k best
//    keys to part[(row - r0) * nch + chunk];
//  * merge: one wave per target row reads the row's running list (k keys in HBM, sorted), merges the row's own cells (or its chunk
//    lists) and, in a triangle band, the cells (i, row) of the band's rows i < row (the mirrored column: cell (i, j) of the upper
//    triangle is also a candidate of row j), and writes the list back.  Each row is owned by one wave of one launch: no atomics, the
//    result is the same whatever the band and chunk sizes.
struct CrossTopkArgs {
  const int32_t* score;     // the band's results (pair q)
  const int32_t* status;
  int64_t n, r0, r1, tri0;
  int tri;                  // upper-triangle band: row i holds columns j >= i; the merge also takes the columns (rows r0 .. n)
  int ava;                  // all-vs-all: the diagonal cell is no candidate
  int k;                    // 1 .. WFA_CROSS_MAX_K
  int64_t chunk;            // cells per chunk of the row pass (a multiple of 64)
  int64_t nch;              // chunks per band row; 0: no row pass, the merge reads the rows' cells itself
  uint64_t* part;           // row pass: k keys per (band row, chunk)
  uint64_t* run;            // the running lists: k keys per target row, descending
};

#define WFA_CROSS_MAX_K 64

// Indexed batches (wfa_hip_batch_create_indexed): pair q of a list is (patterns[i[q]], texts[j[q]]).  The layout is the explicit batch's
// (wfa_hip.hip batch_build): the slots of the pairs of up to WFA_FAST_MAX_LEN bases stand back to back in list order, each as long as
// its pair needs (pattern words, text words right behind); a longer pair points into the batch's copy of the sets' words.  The host
// (wfa_hip.hip: batch_build_list over IndexedPairs) knows every slot's place from the sets' lengths; it sends one word offset per WFA_PAIRS_CHUNK pairs (chunk_base), and the chunk's
// workgroup finds its pairs' slots with a prefix sum over their word counts.  Kernel in k_pairs.hip.
#define WFA_PAIRS_CHUNK 256   // pairs per workgroup round (256 threads: one pair each for the metadata, then groups of lanes over words)

struct PairsGenArgs {
  const uint32_t* p_words; const uint32_t* p_woff; const int32_t* p_len; const int64_t* p_boff; const uint8_t* p_flag;   // the pattern set
  const uint32_t* t_words; const uint32_t* t_woff; const int32_t* t_len; const int64_t* t_boff; const uint8_t* t_flag;   // the text set
  const int32_t* i;         // [npairs] index into the pattern set
  const int32_t* j;         // [npairs] index into the text set
  const uint32_t* chunk_base;   // [chunks]: the first slot word of pair chunk * WFA_PAIRS_CHUNK in `words`
  uint32_t* words;          // the batch's word table: (the sets' words when a listed pair is longer than a slot may be,) then the slots
  uint32_t t_wshift;        // the text set's first word in the table (long pairs)
  int64_t t_bshift;         // the text set's first byte in the batch's byte blob
  int64_t npairs;
  int log2g;                // lanes per pair of the copy: 1 << log2g (the longest slot's words rounded up to a power of two, at most 64)
  int all_bytes;            // 1: every pair on its bytes (the wildcard is one of ACGT)
  int lists;                // 1: the list holds byte pairs: write pboff / tboff / flags
  WfaPairMeta* meta;
  int64_t* pboff;
  int64_t* tboff;
  uint8_t* flags;
};

int launch_pairs_gen(const PairsGenArgs& a, int cu_count, hipStream_t stream);

// Windowed batches (wfa_hip_batch_create_windows): pair q of a list is a window of patterns[i[q]], on either strand, against a window
// of texts[j[q]].  A window starts at any base, so nothing of a set can be used in place: EVERY pair gets a word slot, whatever its
// length (the explicit batch's layout: pattern words, text words right behind, slots back to back in list order), re-based to bit 0 of
// its first word, and a pair aligned on its bytes also gets a byte slot holding the two materialised windows (each rounded up to whole
// 32-bit words, zero behind the window).  The batch owns the slots and nothing else of the sets.  The host (wfa_hip.hip: batch_build_list over WindowPairs) sends one word offset and
// one byte offset per WFA_PAIRS_CHUNK pairs; the chunk's workgroup places its pairs' slots with two prefix sums.  Kernel in
// k_windows.hip; wfa_window_word below is the gather of one slot word, shared with the host statement of it (wfa_hip_window_2bit).
#define WFA_WIN_REVERSE 1   // opt[q]: the pattern window is reverse-complemented
#define WFA_WIN_BYTES 2     // opt[q]: a window of the pair holds a letter outside ACGT (the host looked it up in the sets' runs)

struct WindowsGenArgs {
  const uint32_t* p_words; const uint32_t* p_woff; const int32_t* p_len; const int64_t* p_boff; const uint8_t* p_bytes;   // the pattern set
  const uint32_t* t_words; const uint32_t* t_woff; const int32_t* t_len; const int64_t* t_boff; const uint8_t* t_bytes;   // the text set
  const int32_t* i;         // [npairs] index into the pattern set
  const int32_t* j;         // [npairs] index into the text set
  const int32_t* p_start;   // [npairs] or nullptr: 0
  const int32_t* p_wlen;    // [npairs] or nullptr: to the end of the sequence
  const int32_t* t_start;
  const int32_t* t_wlen;
  const uint8_t* opt;       // [npairs] WFA_WIN_* or nullptr: forward, no byte pairs but under all_bytes
  const uint32_t* chunk_base;    // [chunks]: the first slot word of pair chunk * WFA_PAIRS_CHUNK in `words`
  const int64_t* chunk_bbase;    // [chunks]: its first slot byte in `bytes` (lists only)
  uint32_t* words;          // the batch's word table: the slots
  uint8_t* bytes;           // the batch's byte blob: the byte slots
  int64_t npairs;
  int log2g;                // lanes per pair of the gather: 1 << log2g
  int all_bytes;            // 1: every pair on its bytes (the wildcard is one of ACGT)
  int lists;                // 1: the list holds byte pairs: write pboff / tboff / flags and the byte slots
  WfaPairMeta* meta;
  int64_t* pboff;
  int64_t* tboff;
  uint8_t* flags;
};

int launch_windows_gen(const WindowsGenArgs& a, int cu_count, hipStream_t stream);

// Word w of a window of `len` bases from base `start` of a packed sequence, re-based to bit 0, zero beyond `len`.  `lo` / `hi` are the
// source words wfa_window_src(...) and the one after it (0 where the sequence has none).  Forward: the funnel shift of the two by the
// start's residue.  Reverse: the same funnel shift ending at base start + len - 1 - 16 w, then the 2-bit groups reversed (a bit
// reversal and a swap of each group's two bits) and complemented (code ^ 2).
__host__ __device__ inline int64_t wfa_window_first(int64_t start, int32_t len, uint32_t w, bool rev) {   // first source base of word w (may be < start)
  return rev ? start + len - 16 - 16 * (int64_t)w : start + 16 * (int64_t)w;
}
__host__ __device__ inline uint32_t wfa_window_word(uint32_t lo, uint32_t hi, int64_t first, int32_t len, uint32_t w, bool rev) {
  const uint32_t sh = 2u * (uint32_t)(first & 15);
#if defined(__HIP_DEVICE_COMPILE__)
  uint32_t v = __builtin_amdgcn_alignbit(hi, lo, sh);
  if (rev) v = __builtin_bitreverse32(v);
#else
  uint32_t v = sh ? (lo >> sh) | (hi << (32u - sh)) : lo;
  if (rev) {
    v = ((v >> 16) | (v << 16));
    v = ((v >> 8) & 0x00FF00FFu) | ((v & 0x00FF00FFu) << 8);
    v = ((v >> 4) & 0x0F0F0F0Fu) | ((v & 0x0F0F0F0Fu) << 4);
    v = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2);
    v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
  }
#endif
  if (rev) v = (((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1)) ^ 0xAAAAAAAAu;
  const int32_t cnt = len - 16 * (int32_t)w;
  return cnt >= 16 ? v : v & ((1u << (2 * cnt)) - 1u);
}

int launch_cross_topk(const CrossTopkArgs& a, hipStream_t stream);

int launch_cross_gen(const CrossGenArgs& a, hipStream_t stream);
int launch_cross_scatter(const CrossResArgs& a, hipStream_t stream);
int launch_cross_compact(const CrossResArgs& a, hipStream_t stream);

}  // namespace wfa
