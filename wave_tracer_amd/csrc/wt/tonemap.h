// wave_tracer_amd — film development and tonemapping, per pixel: the arithmetic the device kernels (kernels_develop.hip) and their host twins share.
//
// Reference: render_context_t::develop (src/scene/render.cpp:245-291, film_storage.hpp:256-287) for the developed value;
//            tonemap_t (src/sensor/response/tonemap.cpp:51-66 the scalar operators, :72-106 the three modes);
//            colourspace::luminance and sRGB::from_linear (include/wt/spectrum/colourspace/RGB/RGB.hpp:155-157, 194-198);
//            m::clamp01 (include/wt/math/common.hpp:508-511).
// All of it is f32 (the reference's f_t) except the development, which divides and adds in f64 like wtgpu_develop.  The library is built with
// -ffp-contract=off: no multiply-add below is fused, on either side.
//
// Colour maps: the reference takes them from tinycolormap (a third-party header that is absent from its checkout), so parity with its Magma /
// Turbo / ... tables is NOT pinned here.  A map is a table of n >= 2 RGB entries the caller supplies (imageio.colour_table samples `grey` and
// the polynomial fit of `turbo`), sampled at v (n - 1) with linear interpolation between neighbours.
// The `function` operator (a user expression, tonemap.cpp:53) is read by the scene reader and refused by the entry points.
#pragma once
#include "core.h"

namespace wt {

enum tonemap_op_e : int32_t { TM_LINEAR = 0, TM_GAMMA = 1, TM_SRGB = 2, TM_DB = 3, TM_FUNCTION = 4 };   // tonemap_e (tonemap.hpp:38-54)
enum tonemap_mode_e : int32_t { TM_SELECT = 0, TM_NORMAL = 1, TM_COLOURMAP = 2 };                       // tonemap_mode_e (tonemap.hpp:59-71)
enum tonemap_format_e : uint32_t { TM_F32 = 0, TM_U8 = 1, TM_U16 = 2 };

// what a kernel is told (by value): the operator with its constants as the reference's constructor keeps them, and the colour table
struct tonemap_args_t {
    int32_t op, mode;
    float inv_gamma;        // rg = 1 / gamma (tonemap.cpp:55)
    float db_min, db_len;   // r.min and r.length() = max - min (tonemap.cpp:60-65)
    const float* table;     // table_n x RGB (may be null when the mode needs no map)
    uint32_t table_n;
};

// render.cpp:245-291 as wtgpu_develop states it: value / weight (0 where the weight is 0) + light x (1 / spe), in f64, then one conversion.
WT_HD double develop_scale(uint64_t spe) { return spe > 0 ? 1.0 / double(spe) : 0.0; }
WT_HD float develop_plane(double value, double w, double light, double sl) {
    const double v = w != 0 ? value / w : 0.0;
    return (float)(v + light * sl);
}

// m::clamp01 = glm::clamp(v, 0, 1) = min(max(v, 0), 1) with glm's max(x, y) = (x < y) ? y : x and min(x, y) = (y < x) ? y : x (common.hpp:508-511):
// a NaN fails both comparisons and comes back as NaN, a negative value (and -inf) becomes 0, -0 stays -0, +inf becomes 1.
WT_HD float tm_clamp01(float v) { return fminf_(fmaxf_(v, 0.f), 1.f); }

// RGB.hpp:194-198 (the argument is already clamped: tonemap.cpp:57)
WT_HD float tm_srgb_from_linear(float x) {
    if (x <= .0031308f) return fmaxf_(0.f, 12.92f * x);
    return 1.055f * powf(x, float(1. / 2.4)) - .055f;
}
// tonemap.cpp:51-66.  dB of a negative value is NaN (logf), of +inf 1, of 0 exactly 0.
WT_HD float tm_apply(const tonemap_args_t& t, float x) {
    switch (t.op) {
    case TM_GAMMA: return powf(tm_clamp01(x), t.inv_gamma);
    case TM_SRGB: return tm_srgb_from_linear(tm_clamp01(x));
    case TM_DB: {
        if (x == 0.f) return 0.f;
        const float db = float(10. / 2.302585092994045684) * logf(x);   // 10 / std::numbers::ln10_v<f_t>, a constant of type f_t
        return tm_clamp01((db - t.db_min) / t.db_len);
    }
    default: return x;   // TM_LINEAR
    }
}
// RGB.hpp:155-157: max(0, dot((.2126, .7152, .0722), rgb)); glm's dot of two vec3 adds the three products left to right.  max(0, NaN) = 0.
WT_HD float tm_luminance(float r, float g, float b) { return fmaxf_(0.f, .2126f * r + .7152f * g + .0722f * b); }

// The colour of map value v: clamped to [0, 1] as tinycolormap::GetColor does, position v (n - 1), entries i and i + 1 (i <= n - 2) mixed as
// a (1 - f) + b f — exact on an entry (f = 0 and, at v = 1, f = 1).  A NaN gives a NaN colour.
WT_HD void tm_table_colour(const float* table, uint32_t n, float v, float rgb[3]) {
    const float c = tm_clamp01(v);
    if (!(c == c)) {
        rgb[0] = rgb[1] = rgb[2] = c;
        return;
    }
    const float pos = c * float(n - 1);
    uint32_t i = (uint32_t)pos;
    if (i > n - 2) i = n - 2;
    const float f = pos - float(i);
    const float *a = table + 3 * (size_t)i, *b = a + 3;
    for (int k = 0; k < 3; ++k) rgb[k] = a[k] * (1.f - f) + b[k] * f;
}
// does this mode send `channels` developed values through the colour map?  (tonemap.cpp:91-106)
WT_HD bool tm_uses_map(int32_t mode, uint32_t channels) { return mode == TM_COLOURMAP || (mode == TM_SELECT && channels == 1); }

// tonemap_t::operator() for one pixel: v holds `channels` (1 or 3) developed values.  tonemap.cpp:72-89: through the map the operator is applied
// to the value or to the luminance; otherwise per channel, a single value repeated three times.
WT_HD void tm_pixel(const tonemap_args_t& t, const float* v, uint32_t channels, float rgb[3]) {
    if (tm_uses_map(t.mode, channels)) {
        const float x = channels == 1 ? v[0] : tm_luminance(v[0], v[1], v[2]);
        tm_table_colour(t.table, t.table_n, tm_apply(t, x), rgb);
    } else if (channels == 1) {
        rgb[0] = rgb[1] = rgb[2] = tm_apply(t, v[0]);
    } else
        for (int k = 0; k < 3; ++k) rgb[k] = tm_apply(t, v[k]);
}

// 8- and 16-bit codes: (uint)(clamp01(x) max + 0.5); a NaN is code 0.
WT_HD uint32_t tm_quantise(float x, float max_code) {
    const float c = tm_clamp01(x);
    if (!(c == c)) return 0u;
    return (uint32_t)(c * max_code + .5f);
}

// One pixel, developed → tonemapped → stored: `comps` = 3, or 4 with `alpha` behind the colour (f32: its bits; integer formats: quantised).
WT_HD void tm_store(void* out, size_t pixel, uint32_t format, uint32_t comps, const float rgb[3], float alpha) {
    if (format == TM_F32) {
        float* o = static_cast<float*>(out) + pixel * comps;
        o[0] = rgb[0], o[1] = rgb[1], o[2] = rgb[2];
        if (comps == 4) o[3] = alpha;
    } else if (format == TM_U8) {
        uint8_t* o = static_cast<uint8_t*>(out) + pixel * comps;
        for (int k = 0; k < 3; ++k) o[k] = (uint8_t)tm_quantise(rgb[k], 255.f);
        if (comps == 4) o[3] = (uint8_t)tm_quantise(alpha, 255.f);
    } else {
        uint16_t* o = static_cast<uint16_t*>(out) + pixel * comps;
        for (int k = 0; k < 3; ++k) o[k] = (uint16_t)tm_quantise(rgb[k], 65535.f);
        if (comps == 4) o[3] = (uint16_t)tm_quantise(alpha, 65535.f);
    }
}

}   // namespace wt
