// k_pileup.hip — the pileup reduction (wfa_pileup.hpp: PileupArgs; wfa_hip_pileup_add in api_pileup.hip) and the record side of the
// insertion log (wfa_insertions.hpp: InsLogArgs).
// One wave per pair, grid-stride.  Every store to the table is an int32 atomicAdd; a lane adds only for an op of the aligned core
// whose text position lies inside the pair's text window, and the host and the kernel have checked that the window lies
// inside its sequence, so an op string that disagreed with its pair's lengths could lose counts but never leave the table.  The
// stranded forms add a second time at the same offset of the forward table, the forms with qualities once more at the same offset of
// the quality table, each an allocation of the table's size.  The log's stores are plain: a record and a column byte have one writer,
// at an index below the allocated size (checked at the store); the count form stores pair_count[q], q < npairs, and nothing else.
// The forms are the instantiations of one kernel template, picked by the one launcher from the argument structs it is given.
#include "k_select.hpp"   // (the wave grid, the 64-bit scan)
#include "wfa_insertions.hpp"

namespace wfa {

enum { PILEUP_TABLE = 0, PILEUP_COUNT = 1, PILEUP_TRACK = 2 };

// The walk of a pair's op string.  PILEUP_TABLE: the adds to the table (g unused).  PILEUP_COUNT: no store but pair_count[q] of a
// contributing pair (the host zeroes the array).  PILEUP_TRACK: the adds and the pair's records and column bytes.
// STRANDS (TABLE and TRACK; wfa_pileup.hpp: PileupStrandArgs): a forward pair repeats every add at the same row and column of the
// forward table.  The strand is the pair's, so it is uniform over the wave; without STRANDS `s` is not read.
// QUALS (TABLE and TRACK; wfa_pileup.hpp: PileupQualArgs): every add of a count comes with an add of a capped quality at the same row
// and column of the quality table, an allocation of the table's size; an M or X under min_base_quality adds nothing to any table.
// The log's records do not depend on the qualities.  Every quality load is at an index in [0, qn) behind the window's first byte, and
// qn is the pair's pattern length only where the window lies inside its read of the set (else 0: nothing is loaded).  Without QUALS
// `u` is not read.
template <int MODE, bool STRANDS, bool QUALS>
__device__ __forceinline__ void pileup_walk(const PileupArgs& a, const InsLogArgs& g, const PileupStrandArgs& s, const PileupQualArgs& u) {
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
    // (checked on the host; here so that nothing a caller passes can move a store out of the table)
    if (jq < 0 || jq >= a.nseq || ts < 0 || ts + m.tlen > a.seq_len[jq]) continue;
    int32_t* row0 = a.table + a.seq_off[jq] + ts;
    // the forward table has the table's size and layout: the same offsets stay inside it
    const bool fwd = STRANDS && (s.reverse == nullptr || s.reverse[q] == 0);
    int32_t* frow0 = STRANDS ? s.fwd + a.seq_off[jq] + ts : nullptr;
    const bool on_bytes = a.bytes != nullptr && a.flags[q] != 0;
    const uint8_t* pb = on_bytes ? a.bytes + a.pboff[q] : nullptr;
    const uint32_t* pw = a.words + m.p_woff;
    // the window's quality bytes: position x of the pattern is byte x of them, byte qn - 1 - x on the reverse strand
    const uint8_t* qb = nullptr;
    int qn = 0;
    bool qrev = false;
    int32_t* qrow0 = QUALS ? u.qtab + a.seq_off[jq] + ts : nullptr;
    if (QUALS) {
      const int rq = u.i[q];
      const int64_t ps = u.p_start ? u.p_start[q] : 0;
      // (checked on the host; here so that nothing a caller passes can move a load out of the quality bytes)
      if (rq >= 0 && rq < u.nreads && ps >= 0 && m.plen > 0 && ps + m.plen <= u.qlen[rq]) { qb = u.quals + u.qoff[rq] + ps; qn = m.plen; }
      qrev = u.reverse != nullptr && u.reverse[q] != 0;
    }
    int vbase = 0, hbase = 0;
    unsigned long long carry_d = 0;
    // the log (wave-uniform): the pair's counted runs and D ops so far; the run that is open across a round boundary
    uint32_t nrec = 0, nbase = 0;
    int64_t rec0 = 0, b0 = 0, open_rec = -1, open_off = 0, open_g = 0;
    int32_t open_n = 0;
    if (MODE == PILEUP_TRACK) { rec0 = g.rec_base + (int64_t)g.rec_off[q]; b0 = g.base_base + (int64_t)g.base_off[q]; }
    for (int base = 0; base <= last; base += 64) {
      const int i = base + lane;
      const uint32_t c = (i < len) ? p[i] : 0u;
      const unsigned long long bm = __ballot(c == 'M'), bx = __ballot(c == 'X'), bi = __ballot(c == 'I'), bd = __ballot(c == 'D');
      const unsigned long long bv = bm | bx | bd, bh = bm | bx | bi;
      const int v = vbase + __builtin_popcountll(bv & lower);
      const int h = hbase + __builtin_popcountll(bh & lower);
      const bool d_start = ((bd & ~((bd << 1) | carry_d)) >> lane) & 1ull;
      if (MODE != PILEUP_TABLE) {
        // a run's D ops share its h, so a run is counted whole or not at all; the core begins and ends with an M, so no run leaves it
        const bool inside = i >= first && i <= last && h < m.tlen;
        const unsigned long long dv = __ballot(c == 'D' && inside), sv = __ballot(d_start && inside);
        if (MODE == PILEUP_TRACK) {
          if (open_rec >= 0) {   // the open run goes on: over the leading D ops of this round
            const unsigned long long nd = ~bd;
            const int lead = nd ? __builtin_ctzll(nd) : 64;
            open_n += lead;
            if (lead < 64) {
              if (lane == 0 && open_rec < g.rec_cap) g.records[open_rec] = InsRecord{open_g, open_off, open_n, 0};
              open_rec = -1;
            }
          }
          const int64_t my_off = b0 + nbase + __builtin_popcountll(dv & lower);
          if (c == 'D' && inside && my_off < g.base_cap)
            g.bases[my_off] = (uint8_t)(v >= m.plen ? 4 : on_bytes ? wfa_pileup_letter_col(pb[v]) : wfa_pileup_code_col((pw[v >> 4] >> (2 * (v & 15))) & 3u));
          const unsigned long long x = ~(bd >> lane);
          const int nin = x ? __builtin_ctzll(x) : 64;   // the D ops of this round from this lane on
          if (d_start && inside && lane + nin < 64) {
            const int64_t r = rec0 + nrec + __builtin_popcountll(sv & lower);
            if (r < g.rec_cap) g.records[r] = InsRecord{a.seq_off[jq] + ts + h, my_off, nin, 0};
          }
          // a counted run that starts in this round and reaches its end stays open
          if (bd >> 63) {
            const unsigned long long nd = ~bd;
            const int t = nd ? __builtin_clzll(nd) : 64, s = 64 - t;
            const int hs = __shfl(h, s & 63);
            if ((sv >> (s & 63)) & 1ull) {
              const unsigned long long below = (1ull << (s & 63)) - 1ull;
              open_rec = rec0 + nrec + __builtin_popcountll(sv & below);
              open_off = b0 + nbase + __builtin_popcountll(dv & below);
              open_g = a.seq_off[jq] + ts + hs;
              open_n = t;
            }
          }
        }
        nrec += (uint32_t)__builtin_popcountll(sv); nbase += (uint32_t)__builtin_popcountll(dv);
      }
      vbase += __builtin_popcountll(bv); hbase += __builtin_popcountll(bh); carry_d = bd >> 63;
      if (MODE == PILEUP_COUNT) continue;
      if (i < first || i > last || h >= m.tlen) continue;
      int32_t* row = row0 + h;
      int32_t* frow = frow0 + h;
      int32_t* qrow = qrow0 + h;
      // this lane's quality: of position v (an M or X, and a D run's first base), or the smaller of positions v - 1 and v (an I)
      int qv = 0;
      bool pass = true;
      if (QUALS) {
        const int x0 = c == 'I' ? v - 1 : v;
        int q0 = -1, q1 = -1;
        if (x0 >= 0 && x0 < qn) q0 = qb[qrev ? qn - 1 - x0 : x0];
        if (c == 'I' && v < qn) q1 = qb[qrev ? qn - 1 - v : v];
        pass = q0 >= u.min_base_quality;   // (asked of an M or X only; a position without a byte never passes)
        qv = q0 < 0 ? q1 : (q1 < 0 || q0 < q1) ? q0 : q1;
        qv = qv < 0 ? 0 : qv < u.quality_cap ? qv : u.quality_cap;
      }
      if (c == 'M' || c == 'X') {
        if (v < m.plen && (!QUALS || pass)) {
          const int col = on_bytes ? wfa_pileup_letter_col(pb[v]) : wfa_pileup_code_col((pw[v >> 4] >> (2 * (v & 15))) & 3u);
          atomicAdd(row + (int64_t)col * a.total, 1);
          if (STRANDS && fwd) atomicAdd(frow + (int64_t)col * a.total, 1);
          if (QUALS) atomicAdd(qrow + (int64_t)col * a.total, qv);
          if (c == 'X') {
            atomicAdd(row + (int64_t)WFA_PILEUP_MISMATCH * a.total, 1);
            if (STRANDS && fwd) atomicAdd(frow + (int64_t)WFA_PILEUP_MISMATCH * a.total, 1);
            if (QUALS) atomicAdd(qrow + (int64_t)WFA_PILEUP_MISMATCH * a.total, qv);
          }
        }
      } else if (c == 'I') {
        atomicAdd(row + (int64_t)WFA_PILEUP_DEL * a.total, 1);
        if (STRANDS && fwd) atomicAdd(frow + (int64_t)WFA_PILEUP_DEL * a.total, 1);
        if (QUALS) atomicAdd(qrow + (int64_t)WFA_PILEUP_DEL * a.total, qv);
      } else if (d_start) {
        atomicAdd(row + (int64_t)WFA_PILEUP_INS * a.total, 1);
        if (STRANDS && fwd) atomicAdd(frow + (int64_t)WFA_PILEUP_INS * a.total, 1);
        if (QUALS) atomicAdd(qrow + (int64_t)WFA_PILEUP_INS * a.total, qv);
      }
    }
    if (MODE == PILEUP_COUNT && lane == 0) g.pair_count[q] = InsPairCount{nrec, nbase};
  }
}

// one kernel per form; a form reads only the argument structs its flags name
template <int MODE, bool STRANDS, bool QUALS>
__global__ void __launch_bounds__(256) wfa_pileup_kernel(PileupArgs a, InsLogArgs g, PileupStrandArgs s, PileupQualArgs u) {
  pileup_walk<MODE, STRANDS, QUALS>(a, g, s, u);
}

int launch_pileup_count(const PileupArgs& a, const InsLogArgs& g, int cu_count, hipStream_t stream) {
  if (a.npairs <= 0) return 0;
  hipLaunchKernelGGL((wfa_pileup_kernel<PILEUP_COUNT, false, false>), dim3(wave_grid(a.npairs, cu_count)), dim3(256), 0, stream, a, g,
                     PileupStrandArgs{}, PileupQualArgs{});
  if (hipGetLastError() != hipSuccess) return -1;
  const uint32_t* counts = reinterpret_cast<const uint32_t*>(g.pair_count);
  if (launch_scan64(counts, 2, g.rec_off, a.npairs, stream) != 0) return -1;
  return launch_scan64(counts + 1, 2, g.base_off, a.npairs, stream);
}

int launch_pileup(const PileupArgs& a, const InsLogArgs* g, const PileupStrandArgs* s, const PileupQualArgs* u, int cu_count, hipStream_t stream) {
  if (a.npairs <= 0) return 0;
  if ((s && !s->fwd) || (u && !(u->quals && u->qoff && u->qlen && u->i && u->qtab))) return -1;
  using Kernel = void (*)(PileupArgs, InsLogArgs, PileupStrandArgs, PileupQualArgs);
  static const Kernel forms[2][2][2] = {   // [g][s][u]
      {{wfa_pileup_kernel<PILEUP_TABLE, false, false>, wfa_pileup_kernel<PILEUP_TABLE, false, true>},
       {wfa_pileup_kernel<PILEUP_TABLE, true, false>, wfa_pileup_kernel<PILEUP_TABLE, true, true>}},
      {{wfa_pileup_kernel<PILEUP_TRACK, false, false>, wfa_pileup_kernel<PILEUP_TRACK, false, true>},
       {wfa_pileup_kernel<PILEUP_TRACK, true, false>, wfa_pileup_kernel<PILEUP_TRACK, true, true>}}};
  hipLaunchKernelGGL(forms[g != nullptr][s != nullptr][u != nullptr], dim3(wave_grid(a.npairs, cu_count)), dim3(256), 0, stream, a,
                     g ? *g : InsLogArgs{}, s ? *s : PileupStrandArgs{}, u ? *u : PileupQualArgs{});
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace wfa
