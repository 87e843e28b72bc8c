// k_deletions.hip — the record side of a pileup's deletion log and its reduction to one deletion length per reported row
// (wfa_deletions.hpp: the rule, the layout and the kernels' outline; k_select.hpp: the select's passes and the fill; pileup_deletions_count / _scatter and wfa_hip_pileup_deletions in api_pileup.hip).
// Stores: count pair_count[q] for q < npairs; scatter a record at an index below rec_cap and one atomicAdd on starts[g], g inside the
// pair's text window, which the kernel checks to lie inside its sequence as the table kernel does; the select kernels
// chunk_count[ch] / row `rank` of sel_g, bucket_size and rows for rank < nsel; fill a slot below its row's bucket size and below
// nrec; reduce row `row` < nsel.  Every index read from the log is checked against the selected rows before it is used.
#include "k_select.hpp"
#include "wfa_deletions.hpp"

namespace wfa {

// ---- the record side: a wave per pair, 64 ops per round --------------------------------------------------------------------------------
// SCATTER false: pair_count[q] of a contributing pair (the host zeroes the array).  SCATTER true: the pair's records from its scanned
// offset, and starts[g] += 1 per record.  The lines up to the window check are pileup_walk's (k_pileup.hip), written out in both:
// behind a shared function the scatter kernel here ran 4 % longer and the table kernel took 6 more VGPRs.  The carry of an open run
// reads like pileup_walk's too but closes on another ballot: here on dv, the COUNTED I ops, there on every D op of the round.
template <bool SCATTER>
__device__ __forceinline__ void del_walk(const PileupArgs& a, const DelLogArgs& g) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const unsigned long long lower = (1ull << lane) - 1ull;
  for (int64_t q = wave; q < a.npairs; q += nwaves) {
    if (a.status[q] != 0 || (a.keep && a.keep[q] == 0)) continue;
    const int len = a.cigar_len[q];
    if (len <= 0) continue;
    const uint8_t* p = a.ops + a.cigar_begin[q];
    // the aligned core: first M .. last M
    int first = -1, last = -1;
    for (int base = 0; base < len && first < 0; base += 64) {
      const int i = base + lane;
      const unsigned long long mm = __ballot(i < len && p[i] == 'M');
      if (mm) first = base + __builtin_ctzll(mm);
    }
    if (first < 0) continue;
    for (int top = len; top > 0 && last < 0; top -= 64) {
      const int i = top - 64 + lane;
      const unsigned long long mm = __ballot(i >= 0 && p[i] == 'M');
      if (mm) last = top - 64 + (63 - __builtin_clzll(mm));
    }
    const WfaPairMeta m = a.meta[q];
    const int jq = a.j[q];
    const int64_t ts = a.t_start ? a.t_start[q] : 0;
    // (checked on the host; here so that nothing a caller passes can move a store out of the plane)
    if (jq < 0 || jq >= a.nseq || ts < 0 || ts + m.tlen > a.seq_len[jq]) continue;
    const int64_t g0 = a.seq_off[jq] + ts;
    int hbase = 0;
    unsigned long long carry = 0;   // whether the last op of the previous round was a counted I
    // wave-uniform: the pair's records and deleted bases so far; the run that is open across a round boundary
    uint32_t nrec = 0, nbase = 0;
    int64_t rec0 = 0, open_rec = -1, open_g = 0;
    int32_t open_n = 0;
    if (SCATTER) rec0 = g.rec_base + (int64_t)g.rec_off[q];
    for (int base = 0; base <= last; base += 64) {
      const int i = base + lane;
      const uint32_t c = (i < len) ? p[i] : 0u;
      const unsigned long long bi = __ballot(c == 'I'), bh = bi | __ballot(c == 'M' || c == 'X');
      const int h = hbase + __builtin_popcountll(bh & lower);
      // the I ops column 5 counts; a run lies inside the core whole (the core begins and ends with an M), h < tlen cuts only its end
      const unsigned long long dv = __ballot(c == 'I' && i >= first && i <= last && h < m.tlen);
      const unsigned long long sv = dv & ~((dv << 1) | carry);
      if (SCATTER) {
        if (open_rec >= 0) {   // the open run goes on: over the leading counted I ops of this round
          const unsigned long long nd = ~dv;
          const int lead = nd ? __builtin_ctzll(nd) : 64;
          open_n += lead;
          if (lead < 64) {
            if (lane == 0 && open_rec < g.rec_cap) {
              g.records[open_rec] = DelRecord{open_g, open_n, 0};
              atomicAdd(g.starts + open_g, 1);
            }
            open_rec = -1;
          }
        }
        const unsigned long long x = ~(dv >> lane);
        const int nin = x ? __builtin_ctzll(x) : 64;   // the counted I ops of this round from this lane on
        if (((sv >> lane) & 1ull) && lane + nin < 64) {
          const int64_t r = rec0 + nrec + __builtin_popcountll(sv & lower);
          if (r < g.rec_cap) {
            g.records[r] = DelRecord{g0 + h, nin, 0};
            atomicAdd(g.starts + g0 + h, 1);
          }
        }
        // a run that starts in this round and reaches its end stays open
        if (dv >> 63) {
          const unsigned long long nd = ~dv;
          const int t = nd ? __builtin_clzll(nd) : 64, s = 64 - t;
          const int hs = __shfl(h, s & 63);
          if ((sv >> (s & 63)) & 1ull) {
            const unsigned long long below = (1ull << (s & 63)) - 1ull;
            open_rec = rec0 + nrec + __builtin_popcountll(sv & below);
            open_g = g0 + hs;
            open_n = t;
          }
        }
      }
      nrec += (uint32_t)__builtin_popcountll(sv); nbase += (uint32_t)__builtin_popcountll(dv);
      hbase += __builtin_popcountll(bh); carry = dv >> 63;
    }
    if (!SCATTER && lane == 0) g.pair_count[q] = DelPairCount{nrec, nbase};
  }
}

__global__ void __launch_bounds__(256) wfa_del_count_kernel(PileupArgs a, DelLogArgs g) { del_walk<false>(a, g); }
__global__ void __launch_bounds__(256) wfa_del_scatter_kernel(PileupArgs a, DelLogArgs g) { del_walk<true>(a, g); }

int launch_del_count(const PileupArgs& a, const DelLogArgs& g, int cu_count, hipStream_t stream) {
  if (a.npairs <= 0) return 0;
  hipLaunchKernelGGL(wfa_del_count_kernel, dim3(wave_grid(a.npairs, cu_count)), dim3(256), 0, stream, a, g);
  if (hipGetLastError() != hipSuccess) return -1;
  const uint32_t* counts = reinterpret_cast<const uint32_t*>(g.pair_count);
  if (launch_scan64(counts, 2, g.rec_off, a.npairs, stream) != 0) return -1;
  return launch_scan64(counts + 1, 2, g.base_off, a.npairs, stream);
}

int launch_del_scatter(const PileupArgs& a, const DelLogArgs& g, int cu_count, hipStream_t stream) {
  if (a.npairs <= 0) return 0;
  if (!g.starts) return -1;
  hipLaunchKernelGGL(wfa_del_scatter_kernel, dim3(wave_grid(a.npairs, cu_count)), dim3(256), 0, stream, a, g);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---- select: the reported rows, in ascending global index; fill: the length of every record of the log into the bucket of its row
// (k_select.hpp) ----------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) wfa_del_select_count_kernel(DelArgs a) {
  select_count(a.c, [&](int64_t i) { int64_t depth; int32_t E; return event_flag(a.c, a.starts, i, &depth, &E); });
}

__global__ void __launch_bounds__(256) wfa_del_select_kernel(DelArgs a) { event_select(a, a.starts); }

__global__ void __launch_bounds__(256) wfa_del_fill_kernel(DelArgs a) {
  event_fill(a, [](int64_t, const DelRecord& rec) { return rec.n; });
}

// ---- reduce: a wave per row ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) wfa_del_reduce_kernel(DelArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t row = wave; row < a.nsel; row += nwaves) {
    const uint64_t room = a.bucket_off[row] < (uint64_t)a.nrec ? (uint64_t)a.nrec - a.bucket_off[row] : 0;
    const uint32_t m = (uint32_t)min((uint64_t)min(a.bucket_fill[row], a.bucket_size[row]), room);   // the slots that were written
    const int32_t* bucket = a.bucket + a.bucket_off[row];
    uint32_t best_count = 0, distinct = 0;
    int32_t best_n = 0;
    for (uint32_t t = lane; t < m; t += 64) {
      const int32_t xn = bucket[t];
      uint32_t count = 0;
      bool first_slot = true;
      for (uint32_t s = 0; s < m; ++s)
        if (bucket[s] == xn) { ++count; if (s < t) first_slot = false; }
      distinct += first_slot ? 1u : 0u;
      if (count > best_count || (count == best_count && xn < best_n)) { best_count = count; best_n = xn; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const uint32_t oc = __shfl_xor(best_count, off);
      const int32_t on = __shfl_xor(best_n, off);
      if (oc > best_count || (oc == best_count && oc > 0 && on < best_n)) { best_count = oc; best_n = on; }
      distinct += __shfl_xor(distinct, off);
    }
    if (lane == 0) {
      int32_t* out = a.rows + row * WFA_DELETION_COLS;
      out[4] = (int32_t)best_count; out[5] = best_n; out[6] = (int32_t)distinct;
    }
  }
}

int launch_del_select_count(const DelArgs& a, hipStream_t stream) {
  if (a.c.chunks > 0) hipLaunchKernelGGL(wfa_del_select_count_kernel, dim3(chunk_grid(a.c.chunks)), dim3(256), 0, stream, a);
  if (hipGetLastError() != hipSuccess) return -1;
  return launch_sites_scan(a.c, stream);
}

int launch_del_select(const DelArgs& a, hipStream_t stream) {
  if (a.c.chunks <= 0 || a.nsel <= 0) return 0;
  hipLaunchKernelGGL(wfa_del_select_kernel, dim3(chunk_grid(a.c.chunks)), dim3(256), 0, stream, a);
  if (hipGetLastError() != hipSuccess) return -1;
  return launch_scan64(a.bucket_size, 1, a.bucket_off, a.nsel, stream);
}

int launch_del_reduce(const DelArgs& a, int cu_count, hipStream_t stream) {
  if (a.nsel <= 0) return 0;
  if (a.nrec > 0) hipLaunchKernelGGL(wfa_del_fill_kernel, dim3(thread_grid(a.nrec, cu_count)), dim3(256), 0, stream, a);
  hipLaunchKernelGGL(wfa_del_reduce_kernel, dim3(wave_grid(a.nsel, cu_count)), dim3(256), 0, stream, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace wfa
