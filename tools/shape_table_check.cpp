// shape_table_check.cpp — host-only check of the penalty-shape table (csrc/wfa_shapes.hpp) and of what the launchers of the register
// kernels decide from it: the normalisation and look-up of a shape, the names of the run-time instantiations (the on-disk code-object
// cache is keyed on them: byte-exact), and the route of a banded / slim launch (csrc/wfa_band.hpp: band_route, slim_launches).
// No GPU is involved: the run-time compiler and the per-unit entry points are stand-ins defined here.  tests/test_shape_table.py builds
// and runs it; exit status 0 = every check passed.  With --dump it also prints every name and every route it looked at.
#include <cstdio>
#include <cstring>
#include <string>
#include "wfa_lane.hpp"
#include "wfa_seg.hpp"
#include "wfa_band.hpp"

static bool g_rtc_available = true, g_rtc_force_all = false, g_dump = false;
static int g_failures = 0, g_checks = 0;

namespace wfa {
bool rtc_available() { return g_rtc_available; }
bool rtc_force_all() { return g_rtc_force_all; }
int rtc_launch(const char*, const std::string&, unsigned, unsigned, size_t, hipStream_t, const void*, size_t) { return 0; }
}  // namespace wfa

using namespace wfa;

#define CHECK(cond, ...)                                                  \
  do {                                                                    \
    ++g_checks;                                                           \
    if (!(cond)) { ++g_failures; printf("FAILED %s:%d: %s — ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
  } while (0)

static WfaDevConfig config(int x, int o, int e, int o2 = 0, int e2 = 0) {
  WfaDevConfig c;
  memset(&c, 0, sizeof(c));
  c.x = x; c.o1 = o; c.e1 = e; c.o2 = o2; c.e2 = e2; c.rtc = 1; c.wildcard = -1;
  return c;
}
static bool is_shape(const PenaltyShape& s, int g, int X, int OE, int E, int OE2 = 0, int E2 = 0) {
  return s.g == g && s.X == X && s.OE == OE && s.E == E && s.OE2 == OE2 && s.E2 == E2;
}

// ---- normalisation and look-up: penalties as (x, o, e [, o2, e2])
static void check_shapes() {
  const int same[3][4] = {{4, 6, 2, 2}, {2, 3, 1, 1}, {8, 12, 4, 4}};   // x, o, e, gcd: all pywfa's default shape
  for (const auto& p : same) {
    const PenaltyShape s = penalty_shape(config(p[0], p[1], p[2]), false);
    CHECK(is_shape(s, p[3], 2, 4, 1), "%d/%d/%d -> g %d (%d, %d, %d)", p[0], p[1], p[2], s.g, s.X, s.OE, s.E);
    CHECK(builtin_shape(s) == 0 && band_unit(s) == 0, "%d/%d/%d -> index %d", p[0], p[1], p[2], builtin_shape(s));
  }
  const int presets[6][4] = {{2, 2, 1, 1}, {4, 6, 1, 2}, {3, 4, 1, 3}, {6, 5, 3, 4}, {5, 0, 3, 5}, {1, 1, 1, 6}};   // x, o, e, index
  for (const auto& p : presets) {
    PenaltyShape s;
    const WfaDevConfig c = config(p[0], p[1], p[2]);
    CHECK(seg_shape(c, &s) == p[3] && builtin_shape(s) == p[3], "%d/%d/%d -> index %d", p[0], p[1], p[2], builtin_shape(s));
    // the banded and the slim kernels are built for the leading four only
    CHECK(band_unit(s) == (p[3] < 4 ? p[3] : -1), "%d/%d/%d -> band unit %d", p[0], p[1], p[2], band_unit(s));
  }
  CHECK(affine_shape_count == 7 && band_shape_count == 4 && affine2p_shape_count == 1 && band_unit_count == 5, "table sizes");
  {
    PenaltyShape s;
    const WfaDevConfig c = config(5, 6, 2);
    CHECK(seg_shape(c, &s) == WFA_SHAPE_RTC, "5/6/2 takes the run-time path");
    CHECK(is_shape(s, 1, 5, 8, 2) && builtin_shape(s) == -1 && band_unit(s) == -1, "5/6/2 -> (%d, %d, %d) index %d", s.X, s.OE, s.E, builtin_shape(s));
    g_rtc_available = false;
    CHECK(seg_shape(c, &s) == -1, "5/6/2 without hipRTC");
    g_rtc_available = true;
    g_rtc_force_all = true;
    CHECK(seg_shape(config(4, 6, 2), &s) == WFA_SHAPE_RTC, "4/6/2 with every shape forced through the run-time path");
    g_rtc_force_all = false;
  }
  {
    const PenaltyShape s = penalty_shape(config(4, 6, 2, 24, 1), true);
    CHECK(is_shape(s, 1, 4, 8, 2, 25, 1), "2p 4/6/2/24/1 -> (%d, %d, %d, %d, %d)", s.X, s.OE, s.E, s.OE2, s.E2);
    CHECK(builtin_shape(s) == 0 && band_unit(s) == 4, "2p 4/6/2/24/1 -> entry %d, unit %d", builtin_shape(s), band_unit(s));
    const PenaltyShape t = penalty_shape(config(3, 4, 2, 12, 1), true);
    CHECK(is_shape(t, 1, 3, 6, 2, 13, 1) && builtin_shape(t) == -1 && band_unit(t) == -1, "2p 3/4/2/12/1 -> entry %d", builtin_shape(t));
    CHECK(band_supported(config(4, 6, 2, 24, 1), 5) && band_supported(config(3, 4, 2, 12, 1), 5) && band_supported(config(6, 5, 3), 3), "band_supported");
    g_rtc_available = false;
    CHECK(band_supported(config(4, 6, 2, 24, 1), 5) && !band_supported(config(3, 4, 2, 12, 1), 5) && !band_supported(config(6, 5, 3), 3), "band_supported without hipRTC");
    g_rtc_available = true;
  }
  for (int u = 0; u < band_unit_count; ++u) CHECK(band_unit(band_unit_shape(u)) == u, "band unit %d", u);
}

// ---- the launch arguments of a banded stage
struct Shape5 { const char* what; int x, oe, e, oe2, e2; };   // score units
static const Shape5 k_shapes[] = {
  {"built-in", 4, 8, 2, 0, 0}, {"run-time", 5, 8, 2, 0, 0}, {"lane-only built-in", 6, 8, 3, 0, 0},
  {"2p built-in", 4, 8, 2, 25, 1}, {"2p run-time", 3, 6, 2, 13, 1},
};
static BandArgs band_args(const Shape5& s, int heur, int slim, int split, int pb, int h16, int win) {
  BandArgs a;
  memset(&a, 0, sizeof(a));
  a.x = s.x; a.oe = s.oe; a.e = s.e; a.oe2 = s.oe2; a.e2 = s.e2;
  a.g = penalty_shape(s.x, s.oe, s.e, s.oe2, s.e2).g;
  a.heur = heur; a.slim = slim; a.split = split; a.pb = pb; a.h16 = h16; a.win = win;
  return a;
}

// ---- names of the run-time instantiations: literal, because code objects cached on disk are found by them
static void check_name(const std::string& got, const char* want) {
  if (g_dump) printf("name %s\n", got.c_str());
  CHECK(got == want, "got \"%s\", want \"%s\"", got.c_str(), want);
}
static void check_names() {
  const PenaltyShape s = penalty_shape(config(5, 6, 2), false);   // (5, 8, 2)
  check_name(lane_rtc_name(s, false, 0, 0), "wfa::wfa_lane_kernel<5, 8, 2, false, false>");
  check_name(lane_rtc_name(s, true, 0, 0), "wfa::wfa_lane_kernel<5, 8, 2, true, false>");
  check_name(lane_rtc_name(s, false, 1, 0), "wfa::wfa_lane_kernel<5, 8, 2, false, true>");
  check_name(lane_rtc_name(s, false, 2, 0), "wfa::wfa_lane_kernel<5, 8, 2, false, true, 0, 16>");
  check_name(lane_rtc_name(s, true, 0, 1), "wfa::wfa_lane_kernel<5, 8, 2, true, false, 1>");
  check_name(seg_rtc_name(s, 16, true, false, false, 0), "wfa::wfa_seg_kernel<5, 8, 2, 16, true, false, false>");
  check_name(seg_rtc_name(s, 32, false, false, true, 0), "wfa::wfa_seg_kernel<5, 8, 2, 32, false, false, true>");
  check_name(seg_rtc_name(s, 64, false, true, false, 2), "wfa::wfa_seg_kernel<5, 8, 2, 64, false, true, false, 2>");
  // banded: the form is the route's (slim = 0: the slim kernel takes nothing)
  auto band_name = [](const Shape5& sh, int split, int pb, int nch, bool full, bool adapt, bool seqlds) {
    const BandRoute r = band_route(band_args(sh, adapt ? 1 : 0, 0, split, pb, 1, 0), nch, full, adapt, seqlds);
    CHECK(r.kind == BandRoute::BAND_RTC, "%s: kind %d", sh.what, (int)r.kind);
    return band_rtc_name(r.shape, r.form, nch, full, adapt, seqlds);
  };
  check_name(band_name(k_shapes[1], 1, 1, 4, true, true, true), "wfa::wfa_band_kernel<4, true, true, true, true, true, 5, 8, 2, 0, 0>");
  check_name(band_name(k_shapes[1], 0, 1, 2, true, false, false), "wfa::wfa_band_kernel<2, true, false, false, false, false, 5, 8, 2, 0, 0>");
  check_name(band_name(k_shapes[1], 1, 1, 1, false, true, true), "wfa::wfa_band_kernel<1, false, true, true, false, false, 5, 8, 2, 0, 0>");
  check_name(band_name(k_shapes[4], 1, 0, 4, true, true, true), "wfa::wfa_band_kernel_w3<4, true, true, true, false, true, 3, 6, 2, 13, 1>");
  check_name(band_name(k_shapes[4], 1, 1, 4, true, true, true), "wfa::wfa_band_kernel<4, true, true, true, true, true, 3, 6, 2, 13, 1>");
  check_name(band_name(k_shapes[4], 1, 1, 3, true, false, true), "wfa::wfa_band_kernel_w4<3, true, false, true, true, true, 3, 6, 2, 13, 1>");
  // slim
  const PenaltyShape t = penalty_shape(3, 6, 2, 13, 1);
  check_name(slim_rtc_name(s, 2, 0, false), "wfa::wfa_slim_kernel<2, 0, 5, 8, 2, 0, 0>");
  check_name(slim_rtc_name(s, 2, 1, false), "wfa::wfa_slim_kernel<2, 1, 5, 8, 2, 0, 0>");
  check_name(slim_rtc_name(s, 4, 2, false), "wfa::wfa_slim_kernel_tail<4, 2, 5, 8, 2, 0, 0>");
  check_name(slim_rtc_name(s, 4, 1, true), "wfa::wfa_slim_kernel_tail<4, 1, 5, 8, 2, 0, 0, true>");
  check_name(slim_rtc_name(t, 3, 0, false), "wfa::wfa_slim_kernel_2p<3, 0, 3, 6, 2, 13, 1>");
  check_name(slim_rtc_name(t, 4, 2, false), "wfa::wfa_slim_kernel_tail<4, 2, 3, 6, 2, 13, 1>");
}

// ---- the route of a launch against a second statement of the rules, one function per consumer (what the walk is told, what is
// launched) and the shape numbers spelled out, so that a slip in the table or in band_route shows
static bool old_slim_takes(const BandArgs& a, int nch, bool full, bool adapt, bool seqlds) {
  if (!a.slim || !seqlds || a.debug != 0) return false;
  if (adapt ? a.heur != 1 : a.heur != 0) return false;
  if (nch == (a.oe2 > 0 ? 3 : 2)) return !full || (a.split ? a.pb != 0 : a.h16 != 0);
  if (a.win) return nch == 4 && a.oe2 == 0 && (!full || (a.split && a.pb != 0));
  if (nch == 4) return !full || (a.split ? (a.pb != 0 && a.oe2 == 0) : a.h16 != 0);
  return false;
}
static int old_unit(const BandArgs& a) {
  const int g = a.g, X = a.x / g, OE = a.oe / g, E = a.e / g;
  if (a.oe2 > 0) return (X == 4 && OE == 8 && E == 2 && a.oe2 / g == 25 && a.e2 / g == 1) ? 4 : -1;
  if (X == 2 && OE == 4 && E == 1) return 0;
  if (X == 2 && OE == 3 && E == 1) return 1;
  if (X == 4 && OE == 7 && E == 1) return 2;
  if (X == 3 && OE == 5 && E == 1) return 3;
  return -1;
}
static bool old_slim_rtc_shape_ok(const BandArgs& a) {
  const int g = a.g, X = a.x / g, OE = a.oe / g, E = a.e / g, OE2 = a.oe2 / g, E2 = a.e2 / g;
  if (OE2 == 0) return (X > OE ? X : OE) <= 12 && E <= 3;
  return X < OE && OE < OE2 && X <= 8 && E <= 3 && E2 >= 1 && E2 <= 2 && OE2 - X <= 40;
}
static bool old_slim_launches(const BandArgs& a, int nch, bool full, bool adapt, bool seqlds) {
  if (!old_slim_takes(a, nch, full, adapt, seqlds) || (g_rtc_force_all && g_rtc_available)) return false;
  if (old_unit(a) >= 0) return true;
  return old_slim_rtc_shape_ok(a) && g_rtc_available;
}
static BandRoute::Kind old_launch_band(const BandArgs& a, int nch, bool full, bool adapt, bool seqlds) {
  if (g_rtc_force_all && g_rtc_available) return BandRoute::BAND_RTC;
  if (old_unit(a) >= 0) return old_slim_takes(a, nch, full, adapt, seqlds) ? BandRoute::SLIM_UNIT : BandRoute::BAND_UNIT;
  if (old_slim_takes(a, nch, full, adapt, seqlds) && old_slim_rtc_shape_ok(a)) return BandRoute::SLIM_RTC;
  return BandRoute::BAND_RTC;
}

static void check_routes() {
  long rows = 0;
  for (int env = 0; env < 3; ++env) {   // hipRTC works; it does not; every shape forced through it
    g_rtc_available = env != 1; g_rtc_force_all = env == 2;
    for (const Shape5& sh : k_shapes)
      for (int nch = 1; nch <= 4; ++nch)
        for (int bits = 0; bits < 256; ++bits)
          for (int heur = 0; heur <= 2; ++heur)
            for (int slim = 0; slim <= 1; ++slim) {
              const bool full = bits & 1, adapt = bits & 2, seqlds = bits & 4;
              const BandArgs a = band_args(sh, heur, slim, (bits >> 3) & 1, (bits >> 4) & 1, (bits >> 5) & 1, (bits >> 6) & 1);
              if (bits & 128) continue;   // (seven flags)
              const BandRoute r = band_route(a, nch, full, adapt, seqlds);
              const bool slim_route = r.kind == BandRoute::SLIM_UNIT || r.kind == BandRoute::SLIM_RTC;
              const bool launches = slim_launches(a, nch, full, adapt, seqlds);
              ++rows;
              if (g_dump) printf("route %d %s nch %d full %d adapt %d seqlds %d split %d pb %d h16 %d win %d heur %d slim %d -> kind %d unit %d launches %d\n", env,
                                 sh.what, nch, full, adapt, seqlds, a.split, a.pb, a.h16, a.win, heur, slim, (int)r.kind,
                                 (r.kind == BandRoute::SLIM_UNIT || r.kind == BandRoute::BAND_UNIT) ? r.unit : -1, launches);
              const char* fmt = "%s nch %d flags %d heur %d slim %d env %d";
              CHECK(r.kind == old_launch_band(a, nch, full, adapt, seqlds), fmt, sh.what, nch, bits, heur, slim, env);
              CHECK(r.unit == old_unit(a), fmt, sh.what, nch, bits, heur, slim, env);
              CHECK(launches == old_slim_launches(a, nch, full, adapt, seqlds), fmt, sh.what, nch, bits, heur, slim, env);
              // what sets BandArgs::pb_raw is "the route is slim" wherever a launch is made: a shape without a unit is launched only
              // where hipRTC works (band_supported)
              if (g_rtc_available || r.unit >= 0) CHECK(launches == slim_route, fmt, sh.what, nch, bits, heur, slim, env);
              // the form, as launch_band_rtc / launch_band_t / launch_band_k chose it
              const bool split = full && a.split, pb = split && a.pb;
              const int kernel = (a.oe2 > 0 && nch == 3) ? 4 : (a.oe2 > 0 && nch == 4 && !pb) ? 3 : 0;
              CHECK(r.form.kernel == kernel && r.form.pb == pb && r.form.split == split, fmt, sh.what, nch, bits, heur, slim, env);
            }
  }
  g_rtc_available = true; g_rtc_force_all = false;
  CHECK(rows == 3L * 5 * 4 * 128 * 3 * 2, "rows %ld", rows);
}

int main(int argc, char** argv) {
  g_dump = argc > 1 && strcmp(argv[1], "--dump") == 0;
  check_shapes();
  check_names();
  check_routes();
  printf("%d checks, %d failed\n", g_checks, g_failures);
  return g_failures ? 1 : 0;
}
