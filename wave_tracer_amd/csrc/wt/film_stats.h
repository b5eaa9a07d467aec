// wave_tracer_amd — film statistics (range, histogram, sum): the arithmetic the device kernels (kernels_stats.hip) and their host twin share.
// What a pixel's planes are (fs_planes), the flags and the summation order are also the film comparison's (wt/film_compare.h) and, for the
// developed values, the tonemapper's (kernels_develop.hip).
//
// Element value.  x = develop_plane(...) of wt/tonemap.h, the f32 wtgpu_develop writes, of plane  channel * stokes + stokes_component — or, from a
// developed film, that f32 as it lies there (film_src_t: the one statement of the two sources, for all the film passes);  with
// FS_LUMINANCE a 3-channel film has a fourth plane, tm_luminance of the three developed values (taken before FS_ABS).  FS_ABS: fabsf(x), for the
// signed Stokes components Q / U / V (a NaN stays a NaN).
// Membership.  A pixel's elements are included iff no mask is given or mask[pixel] > 0 (a NaN mask value excludes).
// Classes.  An included element is exactly one of: NaN;  x < 0;  x == 0;  0 < x < edge[0] (below);  x >= edge[bins] (above);  bin i with
// edge[i] <= x < edge[i + 1].  edge[] holds bins + 1 strictly increasing f32 thresholds in x's own scale, built ONCE on the host in f64 and
// rounded (fs_edge): linear  lo + i (hi - lo) / bins,  dB  10^((lo + i (hi - lo) / bins) / 10).  No logf runs per element, so every count is the
// same on both sides, bit for bit.  bins = 0: the single edge of lo splits the positive elements into below and above.
// Extrema.  min / max / min_positive over the non-NaN included elements under the total order of fs_key (-0 sorts below +0), so they do not
// depend on the order the elements are met in; NaN when there is no such element.
// Sum.  f64, over the non-NaN included elements, in ONE fixed order: the plane's elements in row-major order in chunks of kFsChunk = 256, a chunk
// reduced by the butterfly pairing a[i] += a[i + d] (i < d) for d = 128, 64, ... 1 with +0.0 for excluded, NaN and missing elements; the
// chunk sums reduced by the same rule, level after level, until one number is left (fs_level_count).  Only additions: nothing to contract.
#pragma once
#include <type_traits>

#include "core.h"
#include "tonemap.h"

namespace wt {

enum film_stats_flag_e : uint32_t { FS_ABS = 1u, FS_LUMINANCE = 2u };
enum film_stats_scale_e : uint32_t { FS_LINEAR = 0u, FS_DB = 1u };
constexpr uint32_t kFsMaxBins = 4096;
constexpr uint32_t kFsMaxPlanes = 4;    // three channels and the luminance
constexpr uint32_t kFsChunk = 256;

// wtgpu_film_stats as the kernels fill it: the three extrema travel as keys until the last kernel turns them into floats
struct film_stats_rec_t {
    unsigned long long n, n_nan, n_negative, n_zero, n_below, n_above;
    uint32_t min_inv, max_key, minpos_inv, pad;   // ~fs_key of the minima (so that all three grow, from 0 = "no element"), fs_key of the maximum
    double sum;
};
static_assert(sizeof(film_stats_rec_t) == 72, "wtgpu_film_stats");

// edge i of the table, in f64 until the one rounding (the host builds the table; nothing on the device calls this)
inline float fs_edge(uint32_t scale, double lo, double hi, uint32_t bins, uint32_t i) {
    const double t = bins ? lo + double(i) * (hi - lo) / double(bins) : lo;
    return (float)(scale == FS_DB ? std::pow(10.0, t / 10.0) : t);
}

// A key that orders the non-NaN floats as the reals order them, -0 below +0: unsigned comparison of keys = comparison of values.  No value
// maps to 0 or to 0xffffffff (the keys of the NaNs with all mantissa bits set), which is what makes 0 the mark of "no element".
WT_HD uint32_t fs_key(float x) {
    uint32_t u;
    __builtin_memcpy(&u, &x, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
WT_HD float fs_unkey(uint32_t k) {
    if (k == 0u) k = 0x7fc00000u ^ 0x80000000u;   // no element: a quiet NaN
    const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    float x;
    __builtin_memcpy(&x, &u, 4);
    return x;
}

enum film_stats_class_e : uint32_t { FS_NAN = 0, FS_NEGATIVE = 1, FS_ZERO = 2, FS_BELOW = 3, FS_ABOVE = 4, FS_BIN = 5 };
// The class of an element; for FS_BIN the bin's index goes to `bin`.  The search keeps edge[lo] <= x < edge[hi].
WT_HD uint32_t fs_classify(float x, const float* edge, uint32_t bins, uint32_t& bin) {
    if (!(x == x)) return FS_NAN;
    if (x < 0.f) return FS_NEGATIVE;
    if (x == 0.f) return FS_ZERO;
    if (x < edge[0]) return FS_BELOW;
    if (x >= edge[bins]) return FS_ABOVE;
    uint32_t lo = 0, hi = bins;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (x >= edge[mid]) lo = mid;
        else hi = mid;
    }
    bin = lo;
    return FS_BIN;
}

// What a film pass reads its elements from (wtgpu_film_source), in two forms; THE place that knows them — fs_planes, the polarisation view's
// loaders (kernels_polar.hip) and the host twins read a film through it and nothing else does.  An element is plane  c * stokes + s  of a pixel,
// element index  pixel * planes + c * stokes + s;  what it needs of its pixel (the accumulators' weight word) is fetched once per pixel.
//   film_src_t<false>  the accumulators as wtgpu_render fills them: develop_plane of value / weight / light with sl = develop_scale(spe);
//   film_src_t<true>   a developed film [height][width][channels][stokes] f32 (wtgpu_develop's, a denoiser's): the element as it is, any f32.
template <bool kDeveloped>
struct film_src_t;
typedef float film_quad_t __attribute__((vector_size(16), aligned(4)));   // four consecutive elements of a developed film, wherever they lie
typedef float film_quad_aligned_t __attribute__((vector_size(16)));
template <>
struct film_src_t<false> {
    static constexpr bool developed = false;
    const double *value, *weight, *light;
    double sl;
    WT_HD const double* first() const { return value; }
    WT_HD double pixel_word(uint64_t pixel) const { return weight[pixel]; }
    WT_HD float element(uint64_t e, double w) const { return develop_plane(value[e], w, light[e], sl); }
    WT_HD float element_of(uint64_t e, uint32_t planes) const { return develop_plane(value[e], weight[e / planes], light[e], sl); }   // (a lane per element: k_develop's mapping)
};
template <>
struct film_src_t<true> {
    static constexpr bool developed = true;
    const float* film;
    static constexpr const double *weight = nullptr, *light = nullptr;   // (what a launch passes in the unused arguments)
    static constexpr double sl = 0.0;
    WT_HD const float* first() const { return film; }
    WT_HD double pixel_word(uint64_t) const { return 0.0; }
    WT_HD float element(uint64_t e, double) const { return film[e]; }
    WT_HD float element_of(uint64_t e, uint32_t) const { return film[e]; }
    WT_HD film_quad_t element4(uint64_t quad) const { return reinterpret_cast<const film_quad_t*>(film)[quad]; }   // elements 4 quad .. 4 quad + 3
};
using film_acc_t = film_src_t<false>;
using film_dev_t = film_src_t<true>;
// The kernels take a source as the four arguments they always took (the pointers __restrict__, which a struct's members cannot say): the first is
// the developed film where the kernel is compiled for one, and the other three are then null and not read.
template <bool kDeveloped>
using film_elem_t = std::conditional_t<kDeveloped, float, double>;
WT_HD film_acc_t film_src(const double* value, const double* weight, const double* light, double sl) { return film_acc_t{value, weight, light, sl}; }
WT_HD film_dev_t film_src(const float* developed, const double*, const double*, double) { return film_dev_t{developed}; }

// A pixel's planes: the element values of planes  c * stokes + s  of its `channels` channels, behind them — with `luminance`, 3-channel films
// only — the luminance of the three, taken before FS_ABS; then FS_ABS of all.  x: channels + luminance floats.
template <bool kDeveloped>
WT_HD void fs_planes(const film_src_t<kDeveloped>& f, uint64_t pixel, uint32_t channels, uint32_t stokes, uint32_t s, bool luminance, uint32_t flags, float* x) {
    const double w = f.pixel_word(pixel);
    const uint64_t base = pixel * (channels * stokes) + s;
    for (uint32_t c = 0; c < channels; ++c) x[c] = f.element(base + c * stokes, w);
    if (luminance) x[channels] = tm_luminance(x[0], x[1], x[2]);
    for (uint32_t c = 0; c < channels + (luminance ? 1u : 0u); ++c) x[c] = (flags & FS_ABS) ? fabsf(x[c]) : x[c];
}
// what an element adds to its plane's sum
WT_HD double fs_addend(float x, bool included) { return included && x == x ? (double)x : 0.0; }

// The butterfly over one chunk (host form; the device holds four elements per lane and pairs them the same way: kernels_film.h).
inline double fs_chunk_sum(double a[kFsChunk]) {
    for (uint32_t d = kFsChunk / 2; d; d >>= 1)
        for (uint32_t i = 0; i < d; ++i) a[i] += a[i + d];
    return a[0];
}
// sums per level: n elements -> ceil(n / 256) chunk sums -> ... -> 1.  A single chunk sum IS the sum (no further level adds +0.0 to it).
WT_HD uint64_t fs_chunks(uint64_t n) { return (n + kFsChunk - 1) / kFsChunk; }
WT_HD uint64_t fs_scratch_len(uint64_t n_elements) {   // doubles of scratch one plane needs for all its levels
    uint64_t total = 0, n = fs_chunks(n_elements);
    for (;;) {
        total += n;
        if (n <= 1) return total;
        n = fs_chunks(n);
    }
}
// The levels above the chunks (host form; kernels_film.h has the device's): `sums` holds a plane's n_chunks chunk sums and, behind them, room for
// every further level (fs_scratch_len).  Each level is written behind the one it reads; returns the one number left, +0.0 where there is no chunk.
inline double fs_reduce_levels(double* sums, uint64_t n_chunks) {
    double* in = sums;
    uint64_t n = n_chunks;
    while (n > 1) {
        double* out = in + n;
        const uint64_t m = fs_chunks(n);
        for (uint64_t chunk = 0; chunk < m; ++chunk) {
            double a[kFsChunk];
            for (uint32_t i = 0; i < kFsChunk; ++i) a[i] = chunk * kFsChunk + i < n ? in[chunk * kFsChunk + i] : 0.0;
            out[chunk] = fs_chunk_sum(a);
        }
        in = out;
        n = m;
    }
    return n ? in[0] : 0.0;
}

}   // namespace wt
