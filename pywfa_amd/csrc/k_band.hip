// k_band.hip — translation units of the banded register kernels (wfa_band.hpp), csrc/build.sh: one per unit of wfa_shapes.hpp
// (-DWFA_TU_INDEX=i: the penalty shape band_unit_shape(i) — the leading gap-affine shapes, then gap-affine-2p), and one for the
// walks over the history and the expansion of their run records into op bytes (-DWFA_BAND_WALK_KERNELS=1).
#include "wfa_band.hpp"

namespace wfa {
#ifdef WFA_BAND_WALK_KERNELS
int launch_band_bt(const BandArgs& a, int nch, hipStream_t stream) { return launch_band_bt_impl(a, nch, stream); }
int launch_lane_expand(const BandArgs& a, hipStream_t walk_stream, hipStream_t expand_stream) { return launch_lane_expand_impl(a, walk_stream, expand_stream); }
#else
static_assert(WFA_TU_INDEX >= 0 && WFA_TU_INDEX < band_unit_count, "WFA_TU_INDEX must name a unit of band_unit_shape()");

constexpr PenaltyShape S = band_unit_shape(WFA_TU_INDEX);

template <>
int launch_band_unit<WFA_TU_INDEX>(const BandArgs& a, int nch, bool full, bool adapt, bool seqlds, long long grid, hipStream_t stream) {
  return launch_band_shape<S.X, S.OE, S.E, S.OE2, S.E2>(a, nch, full, adapt, seqlds, grid, stream);
}
#endif
}  // namespace wfa
