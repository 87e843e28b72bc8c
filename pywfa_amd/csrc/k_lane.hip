// k_lane.hip — translation units of the lane-per-pair kernel (wfa_lane.hpp), one per penalty shape of affine_shapes
// (wfa_shapes.hpp; -DWFA_TU_INDEX=i, csrc/build.sh).
#include "wfa_lane.hpp"

namespace wfa {
static_assert(WFA_TU_INDEX >= 0 && WFA_TU_INDEX < affine_shape_count, "WFA_TU_INDEX must name a shape of affine_shapes");

constexpr PenaltyShape S = affine_shapes[WFA_TU_INDEX];

template <>
int launch_lane_unit<WFA_TU_INDEX>(unsigned grid, size_t smem, hipStream_t stream, const FastArgs& a, int slot_words, int refill_min, bool full, int heur, int nrp) {
  return launch_lane_shape<S.X, S.OE, S.E, lane_shape_widths[WFA_TU_INDEX]>(grid, smem, stream, a, slot_words, refill_min, full, heur, nrp);
}
}  // namespace wfa
