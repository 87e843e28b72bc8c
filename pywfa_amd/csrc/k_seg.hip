// k_seg.hip — translation unit of the segmented register kernels (wfa_seg.hpp) for ONE penalty shape of affine_shapes
// (wfa_shapes.hpp): compiled once per shape index (-DWFA_TU_INDEX=i, csrc/build.sh) so that the shapes build in parallel.
#include "wfa_seg.hpp"

namespace wfa {
static_assert(WFA_TU_INDEX >= 0 && WFA_TU_INDEX < affine_shape_count, "WFA_TU_INDEX must name a shape of affine_shapes");

constexpr PenaltyShape S = affine_shapes[WFA_TU_INDEX];

template <>
int launch_seg_unit<WFA_TU_INDEX>(int w, bool lazy, unsigned grid, hipStream_t stream, const FastArgs& a) {
  return launch_seg_shape<S.X, S.OE, S.E>(w, lazy, grid, stream, a);
}
template <>
int launch_seg_full_unit<WFA_TU_INDEX>(int w, unsigned grid, hipStream_t stream, const FastArgs& a) {
  return launch_seg_full_shape<S.X, S.OE, S.E>(w, grid, stream, a);
}
template <>
int launch_seg_heur_unit<WFA_TU_INDEX>(unsigned grid, hipStream_t stream, const FastArgs& a) {
  return launch_seg_heur_shape<S.X, S.OE, S.E>(grid, stream, a);
}
}  // namespace wfa
