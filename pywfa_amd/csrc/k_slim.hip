// k_slim.hip — translation unit of the slim form of the banded kernel (wfa_slim.hpp) for ONE unit of wfa_shapes.hpp, compiled once
// per index (-DWFA_TU_INDEX=i, csrc/build.sh): the penalty shape band_unit_shape(i) — the leading gap-affine shapes, then gap-affine-2p.
#include "wfa_slim.hpp"

namespace wfa {
static_assert(WFA_TU_INDEX >= 0 && WFA_TU_INDEX < band_unit_count, "WFA_TU_INDEX must name a unit of band_unit_shape()");

constexpr PenaltyShape S = band_unit_shape(WFA_TU_INDEX);

template <>
int launch_slim_unit<WFA_TU_INDEX>(const BandArgs& a, int nch, bool full, long long grid, hipStream_t stream) {
  return launch_slim_shape<S.X, S.OE, S.E, S.OE2, S.E2>(a, nch, full, grid, stream);
}
template <>
int launch_slim_mailbox_unit<WFA_TU_INDEX>(const BandArgs& a, bool full, hipStream_t stream, SlimMailbox* mb) {
  return launch_slim_mailbox_shape<S.X, S.OE, S.E, S.OE2, S.E2>(a, full, stream, mb);   // (-1 for gap-affine-2p: no such kernel)
}
}  // namespace wfa
