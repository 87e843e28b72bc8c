// wfa_shapes.hpp — the penalty shapes the register kernels (wfa_lane.hpp, wfa_seg.hpp, wfa_band.hpp, wfa_slim.hpp) are built for.
// A shape is (x, o + e, e [, o2 + e2, e2]) / gcd: the kernels take it as template arguments and step the score by the gcd.  This
// header holds the tables, the normalisation of a configuration to its shape, the look-up of a shape in the tables and the
// dispatch from a run-time index to the per-shape entry points.  csrc/build.sh compiles k_lane.hip and k_seg.hip once per entry of
// affine_shapes, k_band.hip and k_slim.hip once per band unit (below): a new shape is one line here and its index there.
#pragma once
#include "wfa_rtc_compat.hpp"
#ifndef __HIPCC_RTC__
#include <type_traits>
#endif
#include "wfa_common.hpp"

namespace wfa {

struct PenaltyShape { int g, X, OE, E, OE2, E2; };   // g: the gcd (the score step); OE2 = E2 = 0: gap-affine

// Gap-affine.  The first is pywfa's default 4/6/2 (also 2/3/1, 8/12/4, ...); the others are the usual short-read / long-read
// presets 4/4/2, 4/6/1, 3/4/1, 6/5/3, 5/0/3 and unit costs 1/1/1.  The index of an entry is its translation unit's WFA_TU_INDEX.
constexpr PenaltyShape affine_shapes[] = {
  {1, 2, 4, 1, 0, 0},
  {1, 2, 3, 1, 0, 0},
  {1, 4, 7, 1, 0, 0},
  {1, 3, 5, 1, 0, 0},
  {1, 6, 8, 3, 0, 0},
  {1, 5, 3, 3, 0, 0},
  {1, 1, 2, 1, 0, 0},
};
constexpr int affine_shape_count = (int)(sizeof(affine_shapes) / sizeof(affine_shapes[0]));
// The narrow first stage of the lane kernel (wfa_lane.hpp, NRP = 4: 8 diagonals) is built for every entry; these are the further widths
// an entry gets, one bit per NRP (5: 10 diagonals, 6: 12) — a width is listed only where the kernel compiles without scratch at the
// waves per SIMD its rings allow.
constexpr unsigned LW5 = 1u << 5, LW6 = 1u << 6;
constexpr unsigned lane_shape_widths[] = {
  LW5 | LW6,
  LW5 | LW6,
  LW5 | LW6,
  LW5 | LW6,
  LW5 | LW6,
  LW5 | LW6,
  LW5 | LW6,
};
static_assert(sizeof(lane_shape_widths) / sizeof(lane_shape_widths[0]) == affine_shape_count, "one entry per shape of affine_shapes");
constexpr bool lane_shape_has_width(int shape_idx, int nrp) {
  return shape_idx >= 0 && shape_idx < affine_shape_count && (nrp == 4 || ((nrp == 5 || nrp == 6) && (lane_shape_widths[shape_idx] & (1u << nrp)) != 0u));
}
// The lane and the segmented kernels are built for all of them, the banded and the slim kernels for this many leading entries.
constexpr int band_shape_count = 4;
// Gap-affine-2p (banded and slim kernels only): pywfa's default 4/6/2/24/1.
constexpr PenaltyShape affine2p_shapes[] = {
  {1, 4, 8, 2, 25, 1},
};
constexpr int affine2p_shape_count = (int)(sizeof(affine2p_shapes) / sizeof(affine2p_shapes[0]));
static_assert(band_shape_count <= affine_shape_count, "the banded kernels take leading entries of affine_shapes");

// Units of k_band.hip / k_slim.hip: the leading gap-affine shapes, then the gap-affine-2p shapes (k_band.hip has one more unit
// behind them: the walks).
constexpr int band_unit_count = band_shape_count + affine2p_shape_count;
constexpr PenaltyShape band_unit_shape(int unit) {
  return unit < band_shape_count ? affine_shapes[unit] : affine2p_shapes[unit - band_shape_count];
}

constexpr int find_shape(const PenaltyShape* table, int n, const PenaltyShape& s) {
  for (int i = 0; i < n; ++i)
    if (table[i].X == s.X && table[i].OE == s.OE && table[i].E == s.E && table[i].OE2 == s.OE2 && table[i].E2 == s.E2) return i;
  return -1;
}
// index of `s` in affine_shapes (gap-affine) or in affine2p_shapes (s.OE2 > 0); -1: the library has no instantiation of it
constexpr int builtin_shape(const PenaltyShape& s) {
  return s.OE2 > 0 ? find_shape(affine2p_shapes, affine2p_shape_count, s) : find_shape(affine_shapes, affine_shape_count, s);
}
// the unit of k_band.hip / k_slim.hip built for `s`; -1: none (a shape only the lane and segmented kernels have, or no built-in shape)
constexpr int band_unit(const PenaltyShape& s) {
  const int i = builtin_shape(s);
  if (i < 0) return -1;
  if (s.OE2 > 0) return band_shape_count + i;
  return i < band_shape_count ? i : -1;
}

// the penalties in score units -> their shape (oe2 = 0: gap-affine)
inline PenaltyShape penalty_shape(int x, int oe, int e, int oe2, int e2) {
  int g = gcd_int(gcd_int(x, oe), e);
  if (oe2 > 0) g = gcd_int(gcd_int(g, oe2), e2);
  return PenaltyShape{g, x / g, oe / g, e / g, oe2 > 0 ? oe2 / g : 0, oe2 > 0 ? e2 / g : 0};
}
// ... of a configuration (two: gap-affine-2p)
inline PenaltyShape penalty_shape(const WfaDevConfig& c, bool two) {
  return penalty_shape(c.x, c.o1 + c.e1, c.e1, two ? c.o2 + c.e2 : 0, two ? c.e2 : 0);
}
// ... of the launch arguments of the banded and slim kernels (BandArgs, wfa_band.hpp: x, oe, e, oe2, e2 in score units and their gcd)
template <class Args>
inline PenaltyShape penalty_shape_of_args(const Args& a) {
  return PenaltyShape{a.g, a.x / a.g, a.oe / a.g, a.e / a.g, a.oe2 > 0 ? a.oe2 / a.g : 0, a.oe2 > 0 ? a.e2 / a.g : 0};
}

#ifndef __HIPCC_RTC__
// Per-shape entry points: a family header declares `template <int I> int launch_x_unit(...)` and never defines it; its k_*.hip
// specialises it for I = WFA_TU_INDEX over that entry of the table — one specialisation per object file, found by the linker.
// From a run-time index: f(std::integral_constant<int, I>) for the I == idx of [0, N); -1 when there is none.
template <int N, class F>
inline int with_shape_index(int idx, F&& f) {
  if constexpr (N > 0) return idx == N - 1 ? f(std::integral_constant<int, N - 1>()) : with_shape_index<N - 1>(idx, f);
  else return -1;
}
#endif

}  // namespace wfa
