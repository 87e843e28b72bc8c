// k_rescue.hip — mate rescue: the window list of the fragments without a proper pairing (wfa_place.hpp: rule, layout and the
// kernels' outline; wfa_hip_placer_rescue in api_place.hip).
// Stores: decide writes slot[0] and slot[s + 1] for s < 2 nfrag; the scan writes slot[0 .. 2 nfrag] and bsum[chunk]; emit writes the
// row slot[s] of `out` only when slot[s] < cap.  Loads are guarded the way the pair kernel guards them: a mate outside [0, nreads),
// a hit number outside [0, nhits), a read outside the pattern set or a text outside the text set makes no window (the host has
// checked all four; the guards are here so that nothing a caller passes can move an access out of its array).
#include <algorithm>
#include "wfa_place.hpp"

namespace wfa {

struct RescueRow { int32_t i, j, start, len, reverse, fragment, anchor; };

// the window of slot s, or false: fragment s / 2 is not rescued, mate s % 2 is no anchor, or the window is dropped
__device__ inline bool rescue_slot(const RescueArgs& a, int64_t s, RescueRow* w) {
  const PairArgs& A = a.pair;
  const PlaceArgs& P = A.place;
  const int64_t f = s >> 1;
  const int m = (int)(s & 1);
  const int32_t* pr = A.pair_rows + WFA_PAIR_COLS * f;
  if (pr[2] != 0 || pr[9] != 0 || pr[11] != 0) return false;   // proper, pairings, overflow
  const int64_t r1 = A.mate1 ? (int64_t)A.mate1[f] : 2 * f, r2 = A.mate2 ? (int64_t)A.mate2[f] : 2 * f + 1;
  const int64_t ra = m ? r2 : r1, ro = m ? r1 : r2;
  if (ra < 0 || ra >= P.nreads || ro < 0 || ro >= P.nreads || ro >= a.npatterns) return false;
  const int32_t* se = P.rows + WFA_PLACE_COLS * ra;
  const int32_t hit = se[0], mapq = se[3];
  if (hit < 0 || (int64_t)hit >= P.nhits || mapq < a.anchor_mapq) return false;
  const int4* rec = reinterpret_cast<const int4*>(P.hits + hit);
  const int4 x = rec[0], y = rec[1];   // i, j, reverse, status | score, ts, te, clips
  const int32_t j = x.y, rev = x.z, ts = y.y, te = y.z;
  if (te <= ts || j < 0 || (int64_t)j >= a.ntexts) return false;
  const int64_t len_o = a.read_len[ro], tlen = a.text_len[j];
  int64_t lo, hi;
  if (!rev) {
    lo = (int64_t)ts + A.min_insert - len_o - a.pad;
    hi = (int64_t)ts + A.max_insert + a.pad;
  } else {
    lo = (int64_t)te - A.max_insert - a.pad;
    hi = (int64_t)te - A.min_insert + len_o + a.pad;
  }
  lo = lo < 0 ? 0 : lo;
  hi = hi > tlen ? tlen : hi;
  if (hi - lo < (int64_t)(a.min_len > 1 ? a.min_len : 1)) return false;
  w->i = (int32_t)ro; w->j = j; w->start = (int32_t)lo; w->len = (int32_t)(hi - lo); w->reverse = 1 - (rev ? 1 : 0);
  w->fragment = (int32_t)f; w->anchor = hit;
  return true;
}

__global__ void __launch_bounds__(256) wfa_rescue_decide_kernel(RescueArgs a) {
  const int64_t nslots = 2 * a.pair.nfrag;
  const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t0 == 0) a.slot[0] = 0u;
  for (int64_t s = t0; s < nslots; s += nthreads) {
    RescueRow w;
    a.slot[s + 1] = rescue_slot(a, s, &w) ? 1u : 0u;
  }
}

__global__ void __launch_bounds__(256) wfa_rescue_emit_kernel(RescueArgs a) {
  const int64_t nslots = 2 * a.pair.nfrag;
  const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < nslots; s += nthreads) {
    RescueRow w;
    if (!rescue_slot(a, s, &w)) continue;
    const int64_t at = a.slot[s];
    if (at >= a.cap) continue;
    int4* d = reinterpret_cast<int4*>(a.out + WFA_RESCUE_COLS * at);
    d[0] = make_int4(w.i, w.j, w.start, w.len);
    d[1] = make_int4(w.reverse, w.fragment, w.anchor, 0);
  }
}

int launch_rescue(const RescueArgs& a, int cu_count, hipStream_t stream) {
  const int64_t nslots = 2 * a.pair.nfrag;
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((nslots + 255) / 256, (int64_t)cu_count * 8));
  hipLaunchKernelGGL(wfa_rescue_decide_kernel, dim3(grid), dim3(256), 0, stream, a);
  if (launch_place_scan(a.slot, nslots + 1, a.bsum, stream) != 0) return -1;
  if (nslots > 0 && a.cap > 0) hipLaunchKernelGGL(wfa_rescue_emit_kernel, dim3(grid), dim3(256), 0, stream, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace wfa
