// wave_tracer_amd — the polarisation view of a Stokes film (degrees and angles of polarisation, the film through an analyser, Stokes sums, the
// false-colour picture): the arithmetic the device kernels (kernels_polar.hip) and their host twin share.
//
// Planes.  Each of the film's channels: plane c is the Stokes vector (I, Q, U, V) of the developed values of film planes  c * 4 + s,  the f32
// wtgpu_develop writes, widened to f64.  FP_LUMINANCE (3-channel films) adds the vector  .2126 S_r + .7152 S_g + .0722 S_b,  component by
// component in f64, the three products added left to right and NOT clamped at 0: linear in S, which tm_luminance's max(0, .) is not.
// Arithmetic.  From the f64 components only f64  + - x /,  comparisons and sqrt — IEEE 754 fixes the result of each, and the library is built
// with -ffp-contract=off, so nothing is fused:
//   lin = sqrt(Q Q + U U)    pol = sqrt((Q Q + U U) + V V)    dolp = lin / I    dop = pol / I    docp = V / I
//   analyser = 1/2 (I + Q c2 + U s2),  c2 = cos 2 theta and s2 = sin 2 theta supplied by the caller as doubles
//   aolp = 1/2 pol_atan2(U, Q) in (-pi/2, pi/2]    chi = 1/2 pol_atan2(V, lin)
// No libm function is called: device and host agree on every value bit for bit, the angles included.  Each result is rounded to f32 once.
// pol_atan2.  Octant reduction by comparisons (|y| against |x|, the signs), a further reduction to |z| <= tan(pi/8) by
// atan(t) = pi/4 + atan((t - 1) / (t + 1)), then the odd Taylor polynomial of DEGREE 23 (twelve terms, Horner in z z).  The series alternates
// with decreasing terms, so what it leaves out is below the first omitted term, tan(pi/8)^25 / 25 < 1.1e-11; the roundings of the twenty-odd
// f64 operations add less than 1e-15.  BOUND: |pol_atan2(y, x) - atan2(y, x)| < 1.2e-11 rad, three decades inside the 1e-8 asked of it.
// A zero of either sign counts as +0 (y = -0, x < 0 gives +pi), and pol_atan2(0, 0) = 0: aolp = 0 where lin == 0.
// Membership.  A pixel is a member iff no mask is given or mask[pixel] > 0 (a NaN mask value excludes).
// Classes.  A member is, per plane, exactly one of
//   non-finite  any of I, Q, U, V is NaN or infinite: counted in n_nonfinite; every map value is THE quiet NaN 0x7fc00000; no sum, no maximum;
//   dark        finite and not I > 0: counted in n_dark; dolp, dop, docp, aolp, chi are 0, analyser is still computed; no sum, no maximum;
//   lit         the rest; counted in n_over as well iff (Q Q + U U) + V V > I I — more polarised than bright, a noise diagnostic.
// Record per plane.  n members, the three counts, max_dop = max dop over the lit pixels and argmax, the row-major index of the pixel that has it —
// the lowest on a tie; 0 and UINT64_MAX where no pixel is lit (fc_best_t's total order: wt/film_compare.h) — and six f64 sums over the lit
// pixels, of I, Q, U, V, lin and pol, each in the fixed order of wt/film_stats.h (+0.0 for every other pixel).
// Maps.  [height][width][planes][k] f32, the k maps chosen by the bits of `maps` in the order of film_polar_map_e; 0 for an excluded pixel.
// Picture.  Of ONE plane, every pixel (the mask becomes the alpha, as in the tonemap kernel): hue = aolp / pi + 1/2 (f64 from the f32 map value,
// rounded once), saturation = clamp01(dolp x sat_gain) (f32), value = clamp01(tm_apply(op, I)); hue and saturation are 0 for a pixel that is not
// lit; HSV -> RGB by the sextant formula in f32 with  x + -  only; a NaN value gives the quiet NaN in all three (code 0 in the integer formats).
#pragma once
#include "film_compare.h"

namespace wt {

enum film_polar_flag_e : uint32_t { FP_LUMINANCE = FS_LUMINANCE };
enum film_polar_map_e : uint32_t { FP_DOLP = 0, FP_DOP = 1, FP_DOCP = 2, FP_AOLP = 3, FP_CHI = 4, FP_ANALYSER = 5, kFpMaps = 6 };
enum film_polar_sum_e : uint32_t { FP_SUM_I = 0, FP_SUM_Q = 1, FP_SUM_U = 2, FP_SUM_V = 3, FP_SUM_LIN = 4, FP_SUM_POL = 5, kFpSums = 6 };

// wtgpu_film_polar as the kernels fill it (wt/film_compare.h: count is n_nonfinite, n_dark, n_over; best is max_dop)
using film_polar_rec_t = film_best_rec_t<kFpSums>;
static_assert(sizeof(film_polar_rec_t) == 96, "wtgpu_film_polar");

// what a kernel is told (by value)
struct film_polar_args_t {
    double c2, s2;            // the analyser: cos 2 theta, sin 2 theta
    uint32_t maps, n_maps;    // the bits of the maps asked for, and how many they are
    uint32_t picture_plane, format;
    float sat_gain;
    tonemap_args_t tm;        // op, inv_gamma, db_min, db_len (mode and table are unused)
};

WT_HD bool fp_finite(double x) {
    unsigned long long u;
    __builtin_memcpy(&u, &x, 8);
    return (u & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}
WT_HD float fp_quiet_nan() {
    const uint32_t u = 0x7fc00000u;
    float nan;
    __builtin_memcpy(&nan, &u, 4);
    return nan;
}

constexpr double kFpPi = 3.14159265358979323846, kFpHalfPi = 1.57079632679489661923, kFpQuarterPi = 0.78539816339744830962;
constexpr double kFpTanPi8 = 0.41421356237309504880;   // tan(pi / 8) = sqrt(2) - 1

// atan2(y, x) for finite y, x (see the head of the file for the reduction, the polynomial's degree and the bound)
WT_HD double pol_atan2(double y, double x) {
    const double ax = x < 0.0 ? -x : x + 0.0, ay = y < 0.0 ? -y : y + 0.0;   // (-0 + 0 = +0)
    const bool swap = ay > ax;
    const double mx = swap ? ay : ax, mn = swap ? ax : ay;
    if (!(mx > 0.0)) return 0.0;
    // atan(mn / mx) in [0, pi/4]:  z = mn / mx,  or past tan(pi/8)  pi/4 + atan(z) with z = (mn - mx) / (mn + mx) in [-tan(pi/8), 0]
    const bool upper = mn > kFpTanPi8 * mx;
    const double z = (upper ? mn - mx : mn) / (upper ? mn + mx : mx), w = z * z;
    double p = -1.0 / 23.0;
    p = p * w + 1.0 / 21.0;
    p = p * w - 1.0 / 19.0;
    p = p * w + 1.0 / 17.0;
    p = p * w - 1.0 / 15.0;
    p = p * w + 1.0 / 13.0;
    p = p * w - 1.0 / 11.0;
    p = p * w + 1.0 / 9.0;
    p = p * w - 1.0 / 7.0;
    p = p * w + 1.0 / 5.0;
    p = p * w - 1.0 / 3.0;
    p = p * w + 1.0;
    double a = z * p;
    a = upper ? kFpQuarterPi + a : a;
    a = swap ? kFpHalfPi - a : a;
    a = x < 0.0 ? kFpPi - a : a;
    return y < 0.0 ? -a : a;
}

// What one pixel gives for one plane: its class, its six addends (all +0.0 unless it is a lit member), its dop for the maximum, and the six
// map values of the pixel whether it is a member or not (the maps' 0 for an excluded pixel is the caller's).
struct fp_plane_t {
    uint32_t nonfinite, dark, lit, over;   // 0 or 1, of a member
    double add[kFpSums];
    double dop;
    float map[kFpMaps];
    bool is_lit;                           // the class without the membership (the picture shows every pixel)
};
WT_HD fp_plane_t fp_plane(double I, double Q, double U, double V, bool included, double c2, double s2) {
    fp_plane_t r;
    const bool fin = fp_finite(I) && fp_finite(Q) && fp_finite(U) && fp_finite(V);
    const bool lit = fin && I > 0.0;
    r.is_lit = lit;
    r.nonfinite = included && !fin ? 1u : 0u;
    r.dark = included && fin && !lit ? 1u : 0u;
    r.lit = included && lit ? 1u : 0u;
    // (a pixel that is not lit goes through the arithmetic as the unit vector (1, 0, 0, 0): no NaN, no division by 0)
    const double i = lit ? I : 1.0, q = lit ? Q : 0.0, u = lit ? U : 0.0, v = lit ? V : 0.0;
    const double l2 = q * q + u * u, p2 = l2 + v * v;
    const double lin = sqrt(l2), pol = sqrt(p2);
    const double dolp = lin / i, dop = pol / i, docp = v / i;
    const double aolp = 0.5 * pol_atan2(u, q), chi = 0.5 * pol_atan2(v, lin);
    const double analyser = 0.5 * ((I + Q * c2) + U * s2);
    r.over = r.lit && p2 > i * i ? 1u : 0u;
    const bool take = r.lit != 0u;
    r.add[FP_SUM_I] = take ? i : 0.0;
    r.add[FP_SUM_Q] = take ? q : 0.0;
    r.add[FP_SUM_U] = take ? u : 0.0;
    r.add[FP_SUM_V] = take ? v : 0.0;
    r.add[FP_SUM_LIN] = take ? lin : 0.0;
    r.add[FP_SUM_POL] = take ? pol : 0.0;
    r.dop = take ? dop : 0.0;
    const float nan = fp_quiet_nan();
    r.map[FP_DOLP] = !fin ? nan : lit ? (float)dolp : 0.f;
    r.map[FP_DOP] = !fin ? nan : lit ? (float)dop : 0.f;
    r.map[FP_DOCP] = !fin ? nan : lit ? (float)docp : 0.f;
    r.map[FP_AOLP] = !fin ? nan : lit ? (float)aolp : 0.f;
    r.map[FP_CHI] = !fin ? nan : lit ? (float)chi : 0.f;
    r.map[FP_ANALYSER] = !fin ? nan : (float)analyser;
    return r;
}
// the maximum's candidate of a pixel: only a lit member is one (fc_best_merge's order is total)
WT_HD void fp_best_take(fc_best_t& m, const fp_plane_t& r, unsigned long long pixel) { fc_best_merge(m, r.dop, r.lit ? pixel : kFcNoPixel); }

// The Stokes vector of plane c of a pixel from its developed values x[channel * 4 + s]: a channel's own, or (c == channels) the luminance's.
WT_HD void fp_stokes(const float* x, uint32_t c, uint32_t channels, double S[4]) {
    for (uint32_t s = 0; s < 4; ++s)
        S[s] = c < channels ? (double)x[c * 4 + s] : (.2126 * (double)x[s] + .7152 * (double)x[4 + s]) + .0722 * (double)x[8 + s];
}

// The picture's colour of a pixel: I as the f32 the tonemap operator takes, the plane's result.
WT_HD void fp_colour(const film_polar_args_t& a, float I, const fp_plane_t& r, float rgb[3]) {
    const float val = tm_clamp01(tm_apply(a.tm, I));
    if (!(val == val)) {
        rgb[0] = rgb[1] = rgb[2] = fp_quiet_nan();
        return;
    }
    const float hue = r.is_lit ? (float)((double)r.map[FP_AOLP] / kFpPi + 0.5) : 0.f;
    const float sg = r.map[FP_DOLP] * a.sat_gain;                                   // (inf x 0: no saturation)
    const float sat = r.is_lit && sg == sg ? tm_clamp01(sg) : 0.f;
    const float h6 = hue * 6.f;
    uint32_t sextant = (uint32_t)h6;
    sextant = sextant > 5u ? 5u : sextant;     // hue = 1 is the end of the sixth sextant (f = 1: the colour of hue 0)
    const float f = h6 - (float)sextant;
    const float p = val * (1.f - sat), q = val * (1.f - sat * f), t = val * (1.f - sat * (1.f - f));
    rgb[0] = sextant == 0u || sextant == 5u ? val : sextant == 1u ? q : sextant == 4u ? t : p;
    rgb[1] = sextant == 1u || sextant == 2u ? val : sextant == 3u ? q : sextant == 0u ? t : p;
    rgb[2] = sextant == 3u || sextant == 4u ? val : sextant == 5u ? q : sextant == 2u ? t : p;
}

}   // namespace wt
