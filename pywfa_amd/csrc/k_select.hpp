// k_select.hpp — the ranked select of the pileup reports, once (k_calls.hip, k_insertions.hip, k_deletions.hip; outline: wfa_calls.hpp):
// the count pass and the scatter pass over chunks of bases as templates over a predicate and a row, the owner search, the fill of the
// two logs' buckets, and the grids and the 64-bit scan the pileup kernels share.  Every report instantiates the passes in __global__ kernels of
// its own, so a report's code does not move when another report's predicate or row does.
#pragma once
#include <algorithm>
#include "k_seed.hpp"   // (the workgroup sum of the seed kernels)
#include "wfa_calls.hpp"

namespace wfa {

// ---- grids ---------------------------------------------------------------------------------------------------------------------------------
// a workgroup per chunk of bases
inline unsigned chunk_grid(int64_t chunks) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(chunks, 1 << 16)); }
// a wave per item (a pair, a row), four to a workgroup
inline unsigned wave_grid(int64_t waves, int cu_count) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((waves + 3) / 4, (int64_t)cu_count * 16)); }
// a thread per item, grid-stride
inline unsigned thread_grid(int64_t n, int cu_count) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, (int64_t)cu_count * 32)); }

// out[0 .. n] = the exclusive 64-bit prefix of `n` 32-bit values read with a stride of `stride` words, out[n] the total: one workgroup
// (k_calls.hip).  Stores: out[i] for i <= n.
int launch_scan64(const uint32_t* in, int stride, uint64_t* out, int64_t n, hipStream_t stream);

// ---- the two passes over the chunks of c (256 threads; `chunk` bases per chunk, a multiple of 64) ----------------------------------------
// count: chunk_count[ch] for ch < chunks.  flag(i) -> bool: whether base i of the run is selected (false behind the run's end, which
// the predicate checks itself).
template <class Flag>
__device__ __forceinline__ void select_count(const CallsArgs& c, Flag flag) {
  __shared__ uint32_t s_red[4];
  for (int64_t ch = blockIdx.x; ch < c.chunks; ch += gridDim.x) {
    const int64_t i0 = ch * c.chunk;
    uint32_t mine = 0;   // the selected bases of this wave's rounds (the same in every lane)
    for (int64_t t = threadIdx.x; t < c.chunk; t += 256) mine += (uint32_t)__builtin_popcountll(__ballot(flag(i0 + t)));
    const uint32_t sum = seed_block_sum((threadIdx.x & 63) == 0 ? mine : 0u, s_red);
    if (threadIdx.x == 0) c.chunk_count[ch] = sum;
  }
}

// the sequence that owns global base g: the last one that starts at or before it
__device__ inline int64_t select_owner(const CallsArgs& c, int64_t g) {
  int64_t lo = 0, hi = c.nseq;   // the first sequence that starts behind g; its predecessor owns g
  while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (c.seq_off[mid] > g) hi = mid; else lo = mid + 1; }
  return lo - 1;
}

// scatter: body(i, live, rank_of) runs for base i in every round of every chunk that is not skipped, in all 256 threads at once;
// live: i lies inside the chunk.  The body evaluates its predicate into locals of its own (they are the row's inputs, and stay the
// kernel's, so the compiler places them as if the loop were written out there) and calls rank_of(selected, &rank) exactly once, before
// it diverges: that is the ballot and the two barriers.  rank_of returns whether this base is selected with rank < limit; a selected
// base's rank = chunk_off[chunk] + the selected ones of the rounds and waves in front of it + the popcount of the ballot below its
// lane, so ranks ascend with the global index.  Empty chunks and chunks that start at or behind the limit are skipped whole.  (The
// two log selects pass the total as the limit: no non-empty chunk starts at or behind it, and no rank reaches it.)
template <class Body>
__device__ __forceinline__ void select_scatter(const CallsArgs& c, uint64_t limit, Body body) {
  __shared__ uint32_t s_red[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long lower = (1ull << lane) - 1ull;
  for (int64_t ch = blockIdx.x; ch < c.chunks; ch += gridDim.x) {
    uint64_t run = c.chunk_off[ch];
    if (run >= limit || c.chunk_off[ch + 1] == run) continue;   // (uniform over the workgroup)
    const int64_t i0 = ch * c.chunk;
    for (int64_t t0 = 0; t0 < c.chunk; t0 += 256)
      body(i0 + t0 + threadIdx.x, t0 + threadIdx.x < c.chunk, [&](bool sel, uint64_t* rank) {
        const unsigned long long m = __ballot(sel);
        if (lane == 0) s_red[wave] = (uint32_t)__builtin_popcountll(m);
        __syncthreads();
        uint32_t before = 0;
        for (int w = 0; w < wave; ++w) before += s_red[w];
        const uint32_t total = s_red[0] + s_red[1] + s_red[2] + s_red[3];
        __syncthreads();
        *rank = run + before + (uint32_t)__builtin_popcountll(m & lower);
        run += total;
        return sel && *rank < limit;
      });
  }
}

// ---- the reported rows of a log (InsArgs / DelArgs: the same fields under the same names) ---------------------------------------------------
// whether base i of the run is a reported row of a log whose events per base are events[g] (c6 / starts[g]); false behind the run's end
__device__ inline bool event_flag(const CallsArgs& c, const int32_t* events, int64_t i, int64_t* depth, int32_t* E) {
  if (i >= c.n) return false;
  const int64_t g = c.g0 + i;
  int64_t d = 0;
#pragma unroll
  for (int x = 0; x < 6; ++x) d += c.table[(int64_t)x * c.total + g];
  *depth = d;
  *E = events[g];
  return event_selected(d, *E, c.min_depth, c.min_permille);
}

// the scatter pass of a log's select.  Stores: row `rank` of sel_g, bucket_size and rows, rank < nsel.
template <class Args>
__device__ __forceinline__ void event_select(const Args& a, const int32_t* events) {
  const CallsArgs& c = a.c;
  select_scatter(c, (uint64_t)a.nsel, [&](int64_t i, bool live, auto rank_of) {
    int64_t depth = 0; int32_t E = 0;
    uint64_t rank;
    if (!rank_of(live && event_flag(c, events, i, &depth, &E), &rank)) return;
    const int64_t g = c.g0 + i, j = select_owner(c, g);
    const bool overflow = E > a.max_reads;
    a.sel_g[rank] = g;
    a.bucket_size[rank] = overflow ? 0u : (uint32_t)E;
    int4* row = reinterpret_cast<int4*>(a.rows + rank * 8);   // (WFA_INSERTION_COLS, WFA_DELETION_COLS)
    row[0] = make_int4((int32_t)j, (int32_t)(g - c.seq_off[j]), (int32_t)depth, E);
    row[1] = make_int4(0, 0, 0, overflow ? 1 : 0);
  });
}

// fill: a thread per record of the log, grid-stride; a record on a selected row puts slot(r, record) into the next free slot of its
// row's bucket.  Stores: a slot below its row's bucket size and below nrec (the buckets are sized from the table, the array from the log).
template <class Args, class Slot>
__device__ __forceinline__ void event_fill(const Args& a, Slot slot) {
  const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < a.nrec; r += nthreads) {
    const auto rec = a.records[r];
    if (rec.g < a.c.g0 || rec.g >= a.c.g0 + a.c.n) continue;
    int64_t lo = 0, hi = a.nsel;   // the first selected row at or behind g
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (a.sel_g[mid] < rec.g) lo = mid + 1; else hi = mid; }
    if (lo >= a.nsel || a.sel_g[lo] != rec.g) continue;
    const uint32_t size = a.bucket_size[lo];
    if (size == 0) continue;
    const uint32_t at = atomicAdd(a.bucket_fill + lo, 1u);
    if (at < size && a.bucket_off[lo] + at < (uint64_t)a.nrec) a.bucket[a.bucket_off[lo] + at] = slot(r, rec);
  }
}

}  // namespace wfa
