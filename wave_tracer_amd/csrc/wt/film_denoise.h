// wave_tracer_amd — denoising a film from its two half-films: the dual-buffer non-local-means filter of Rousselle, Knaus and Zwicker (2012).  The
// arithmetic the device kernels (kernels_denoise.hip) and their host twin share.
//
// Inputs.  Two film sets A and B of the scene's size (render_to_noise's halves), developed with spe_a / spe_b: a_i(p), b_i(p) are develop_plane of
// plane i of pixel p, the f32 wtgpu_develop writes, i < P = channels x stokes.  The guide planes are Stokes component 0 of each channel
// (plane c * stokes, c < C = channels = 1 or 3).  Everything below is f32  + - x /,  comparisons and integer / bit operations; no libm function
// is called and the library is built with -ffp-contract=off, so device and host agree on every value bit for bit.
// Variance.  e_c(p) = ((a_c - b_c) (a_c - b_c)) x 0.5f (dn_e);  v_c(p) = (sum of e_c over the 3 x 3 neighbourhood, coordinates clamped to the film,
// rows top to bottom and left to right inside a row, the first term first) x (1.0f / 9.0f) (dn_var9).
// Distance.  For the guide buffer y (a or b), a pixel p and a candidate q = p + (dx, dy), |dx|, |dy| <= r:
//   d_c(p, q) = ((y_c(p) - y_c(q))^2 - alpha (v_c(p) + min(v_c(p), v_c(q)))) / (eps + k2 (v_c(p) + v_c(q)))      (dn_term; k2 = k x k in f32, once)
//   s(p, q) = d_0 [+ d_1 + d_2], left to right
//   h(p, q) = s(p + (-f, 0), q + (-f, 0)) + ... + s(p + (f, 0), q + (f, 0)), left to right
//   D(p, q) = (h(p + (0, -f), q + (0, -f)) + ... + h(p + (0, f), q + (0, f)), top to bottom) x inv_norm,  inv_norm = 1.0f / (C (2f + 1)^2) in f32, once.
// The coordinates of a patch are clamped to the film, p's and q's separately: with u = p + (i, j) NOT clamped the patch term is
// S_d(u) = s(clamp(u), clamp(u + d)), a function of u alone — which is what lets the kernel compute S_d once per tile and offset and sum it
// separably, in exactly the order a naive loop (j outside, i inside) has.
// Weight.  dn_weight(D): 0 if D is a NaN; 1 if D <= 0; else dn_exp2_neg(D x log2 e).  No cutoff: the weight is continuous in D.
// dn_exp2_neg(t) = 2^-t for t >= 0: 0 if not t < 126 (the result would be 2^-126 or less; a NaN gives 0 too); else n = (int)(t + 0.5), the nearest
// integer, g = t - n in [-0.5, 0.5] (exact), z = g x (-ln 2), |z| <= 0.34658; e^z by its Taylor polynomial of DEGREE 7 (Horner), times 2^-n built
// from exponent bits (exact: 1 <= 127 - n <= 127, and the product is a normal number: beyond 125.5 the polynomial is above 1).  2^-0 is exactly 1.
// BOUND: what the polynomial leaves out is at most |z|^8 / 8! e^|z| < 0.34658^8 / 40320 x 1.4143 = 7.3e-9, against e^z >= 0.7071 a relative
// 1.04e-8; the rounding of z moves the result by at most 2^-24 x 0.34658 = 2.1e-8; the seven multiply-add pairs of the Horner form round fourteen
// times at 2^-24 = 6e-8 each, of which the inner ones are damped by |z| <= 0.35: below 2.2e-7 together.  Relative error < 2.6e-7, inside the 1e-6
// asked of it (measured over a sweep of 0 .. 200: tests/golden/denoise_measured.json).
// Candidates.  q must lie inside the film (not clamped), be VALID — all P planes of a and of b finite at q — and, with a mask, have mask(q) > 0.
// Filter.  For (x, y) = (a, b), then (b, a): the weights come from y; over the candidates in row-major order of (dy, dx), sequentially in f32 from
// +0: sw += w and, for every plane i, acc_i += w x (x_i(q) - x_i(p)); a candidate whose weight is not > 0 adds nothing.  fx_i(p) = x_i(p) + acc_i / sw,
// and x_i(p) itself where acc_i / sw == 0 (x + 0 would turn a -0 into +0).  The same weights serve all P planes: a Stokes vector is filtered as
// one thing.
// Pass-through.  A pixel that is not valid, not in the mask, or for which either direction's sw is not > 0 (next to a non-finite pixel, where v is
// not finite) gives out_i = (a_i + b_i) x 0.5f and residual_i = (a_i - b_i) x 0.5f.
// Outputs.  out_i = (fa_i + fb_i) x 0.5f, residual_i = (fa_i - fb_i) x 0.5f, [height][width][P] f32; a NaN is stored as THE quiet NaN 0x7fc00000.
// A constant film is a fixed point and r = 0 returns (a + b) x 0.5f, both bit for bit.
// Guides (wtgpu_film_denoise_guided_*; Rousselle, Manzi and Zwicker 2013's min(w_colour, w_feature) with ONE exponential).  A guide buffer
// g[H][W][G] f32, 0 <= G <= 8, with a scale s_g >= 0 per plane, and optionally an id plane id[H][W] u32.  Feature distance, pointwise (no patch):
//   F(p, q) = sum over g of ((g_g(p) - g_g(q))^2 x s_g), sequentially from +0 in plane order (dn_feature).
// With Dc = D(p, q) x inv_norm: dn_guided(Dc, F) is F where F is a NaN, else F > Dc ? F : Dc, and w = dn_weight(dn_guided(Dc, F)); a NaN Dc
// still gives 0.  A non-finite guide value at p or q makes F infinite or a NaN (inf x 0 is a NaN), so the weight is 0: a pixel whose own guide
// is not finite has sw = 0 and passes through by the rule above, and is nobody's candidate.  With the flag SAME_ID a candidate must also
// have id(q) == id(p): a candidate condition like `valid` and the mask (the pixel itself always qualifies).  F = +0 everywhere (all scales 0,
// finite guides; or G = 0) changes no weight: 0 > Dc only where Dc < 0, where both weights are 1.
#pragma once
#include "core.h"
#include "tonemap.h"

namespace wt {

constexpr uint32_t kDnMaxWindow = 10, kDnMaxPatch = 3, kDnMaxPlanes = 12;

// what a kernel is told (by value)
struct film_denoise_args_t {
    uint32_t r, f;
    float k2, alpha, eps, inv_norm;
};

constexpr float kDnLog2e = 1.44269504088896340736f, kDnMinusLn2 = -0.69314718055994530942f;

WT_HD bool dn_finite(float x) {
    uint32_t u;
    __builtin_memcpy(&u, &x, 4);
    return (u & 0x7f800000u) != 0x7f800000u;
}
// a NaN becomes THE quiet NaN
WT_HD float dn_canon(float x) {
    if (x == x) return x;
    const uint32_t u = 0x7fc00000u;
    float nan;
    __builtin_memcpy(&nan, &u, 4);
    return nan;
}

// 2^-t for t >= 0 (the head of the file has the reduction, the polynomial's degree and the bound)
WT_HD float dn_exp2_neg(float t) {
    if (!(t < 126.f)) return 0.f;
    const int n = (int)(t + 0.5f);
    const float g = t - (float)n, z = g * kDnMinusLn2;
    float p = 1.f / 5040.f;
    p = p * z + 1.f / 720.f;
    p = p * z + 1.f / 120.f;
    p = p * z + 1.f / 24.f;
    p = p * z + 1.f / 6.f;
    p = p * z + 0.5f;
    p = p * z + 1.f;
    p = p * z + 1.f;
    const uint32_t u = (uint32_t)(127 - n) << 23;
    float scale;
    __builtin_memcpy(&scale, &u, 4);
    return p * scale;
}
WT_HD float dn_weight(float D) {
    if (!(D == D)) return 0.f;
    if (D <= 0.f) return 1.f;
    return dn_exp2_neg(D * kDnLog2e);
}

// the guides of a call: G planes with their scales, and whether a candidate must carry the pixel's id
constexpr uint32_t kDnMaxGuides = 8, kDnSameId = 1;
struct film_denoise_guides_t {
    uint32_t n, flags;
    float scale[kDnMaxGuides];
};
// one plane's term of F, and what F does to the colour distance (the head of the file)
WT_HD float dn_feature_term(float gp, float gq, float s) {
    const float d = gp - gq;
    return (d * d) * s;
}
WT_HD float dn_guided(float Dc, float F) {
    if (!(F == F)) return F;
    return F > Dc ? F : Dc;
}

WT_HD float dn_e(float a, float b) {
    const float d = a - b;
    return (d * d) * 0.5f;
}
// e[9]: the 3 x 3 neighbourhood, row-major
WT_HD float dn_var9(const float* e) {
    float s = e[0];
    for (int i = 1; i < 9; ++i) s += e[i];
    return s * (1.0f / 9.0f);
}
WT_HD float dn_term(float yp, float yq, float vp, float vq, const film_denoise_args_t& a) {
    const float d = yp - yq, m = vq < vp ? vq : vp;
    return (d * d - a.alpha * (vp + m)) / (a.eps + a.k2 * (vp + vq));
}
// fx from a direction's sums (sw > 0)
WT_HD float dn_filtered(float x, float acc, float sw) {
    const float t = acc / sw;
    return t == 0.f ? x : x + t;
}
WT_HD uint32_t dn_clamp(int v, uint32_t n) { return v < 0 ? 0u : (uint32_t)v >= n ? n - 1u : (uint32_t)v; }

}   // namespace wt
