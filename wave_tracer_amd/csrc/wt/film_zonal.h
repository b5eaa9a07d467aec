// wave_tracer_amd — zonal film statistics (one record per (zone, plane) of a film under a u32 label plane): the arithmetic the device kernels
// (kernels_zonal.hip) and their host twin share.  Elements, planes, membership, classes and extrema are the film statistics' (wt/film_stats.h:
// fs_planes, fs_classify, fs_key); what is new here is the sum.
//
// Zone.  A member pixel with zones[p] < n_zones belongs to that zone; any other member pixel (0xFFFFFFFF, "no hit", included) to none.
// Sum.  The EXACT sum of the zone's finite f32 elements, rounded ONCE to the nearest f64 (ties to even; +0.0 where the sum is zero) — so it does
// not depend on the order the addends arrive in, atomics may deliver them in any, and it equals math.fsum.  A finite f32 is m x 2^(sh - 149) with
// m < 2^24 and sh = max(e, 1) - 1 <= 253 (e: the biased exponent; subnormals have e = 0 and no hidden bit).  The accumulator of a (zone, plane)
// is kFzWords = 9 two's-complement 64-bit words, word k of weight 2^(32 k - 149): fz_split cuts m << (sh & 31), which is below 2^55, into its low
// 32 bits for word sh >> 5 (at most 7) and the rest for the next word, both negated for a negative x.  A word gains less than 2^32 in magnitude
// per element and a film has fewer than 2^31 pixels (the entry points refuse more), so no word overflows whatever the order.  fz_round
// propagates the carries, takes sign and magnitude, finds the top bit and builds the f64's bits from the top 53 bits, the guard bit and the
// sticky bit: integer operations only, no libm call, the same function on both sides.  (The magnitude is below 2^(31 + 24 + 253) = 2^308 units
// of 2^-149: the result is always a normal f64 and never overflows.)
#pragma once
#include "film_stats.h"

namespace wt {

constexpr uint32_t kFzWords = 9;
constexpr uint32_t kFzMaxZones = 65536;
constexpr uint64_t kFzMaxZoneBins = 1ull << 20;   // n_zones x bins
constexpr uint64_t kFzMaxPixels = 1ull << 31;     // films of this many pixels or more are refused
// the counts of a record, in the order of wtgpu_film_zonal: n, then fs_classify's classes outside the bins and the infinities
enum film_zonal_count_e : uint32_t { FZ_N = 0, FZ_NAN = 1, FZ_INF = 2, FZ_NEGATIVE = 3, FZ_ZERO = 4, FZ_BELOW = 5, FZ_ABOVE = 6, FZ_COUNTS = 7 };
WT_HD uint32_t fz_count_of(uint32_t cls) { return cls == FS_NAN ? FZ_NAN : cls == FS_NEGATIVE ? FZ_NEGATIVE : cls == FS_ZERO ? FZ_ZERO : cls == FS_BELOW ? FZ_BELOW : FZ_ABOVE; }

// what a (zone, plane) accumulates in global memory and in the host twin's tables; all zero = nothing met
struct film_zonal_slot_t {
    unsigned long long w[kFzWords];
    unsigned long long count[FZ_COUNTS];
    uint32_t min_inv, max_key;   // ~fs_key of the minimum and fs_key of the maximum, so that both grow from 0 = "no element"
};
static_assert(sizeof(film_zonal_slot_t) == 136, "film_zonal_slot_t");
// wtgpu_film_zonal
struct film_zonal_rec_t {
    unsigned long long count[FZ_COUNTS];
    float min, max;
    double sum;
};
static_assert(sizeof(film_zonal_rec_t) == 72, "wtgpu_film_zonal");

WT_HD uint32_t fz_bits(float x) {
    uint32_t u;
    __builtin_memcpy(&u, &x, 4);
    return u;
}
WT_HD bool fz_finite(float x) { return (fz_bits(x) & 0x7f800000u) != 0x7f800000u; }
WT_HD bool fz_inf(float x) { return (fz_bits(x) & 0x7fffffffu) == 0x7f800000u; }

// A finite x -> the word k its low part goes to, and the two addends (of words k and k + 1) as two's-complement 64-bit integers.  false: x is a
// zero and adds nothing.
WT_HD bool fz_split(float x, uint32_t& k, unsigned long long& lo, unsigned long long& hi) {
    const uint32_t u = fz_bits(x), e = (u >> 23) & 0xffu, frac = u & 0x7fffffu;
    const uint32_t m = e ? (frac | 0x800000u) : frac, sh = (e ? e : 1u) - 1u;
    if (m == 0u) return false;
    const unsigned long long v = (unsigned long long)m << (sh & 31u);   // < 2^55
    k = sh >> 5;
    lo = v & 0xffffffffull;
    hi = v >> 32;
    if (u & 0x80000000u) lo = 0ull - lo, hi = 0ull - hi;
    return true;
}
// the plain form: words[kFzWords] of one thread
WT_HD void fz_add(unsigned long long* words, float x) {
    uint32_t k;
    unsigned long long lo, hi;
    if (!fz_split(x, k, lo, hi)) return;
    words[k] += lo;
    words[k + 1] += hi;
}

// The words' value, sum of (int64)words[k] x 2^(32 k - 149), rounded to the nearest f64, ties to even.
WT_HD double fz_round(const unsigned long long* words) {
    constexpr uint32_t kLimbs = kFzWords + 1;   // 320 bits: the magnitude is below 2^308
    uint32_t limb[kLimbs + 2];                  // (two zero limbs behind them: the 64-bit window reads three)
    long long carry = 0;
    for (uint32_t j = 0; j < kLimbs; ++j) {
        const long long lo = j < kFzWords ? (long long)(words[j] & 0xffffffffull) : 0ll;
        const long long hi = j > 0 ? ((long long)words[j - 1] >> 32) : 0ll;   // arithmetic: the word's signed upper half
        const long long acc = lo + hi + carry;
        limb[j] = (uint32_t)((unsigned long long)acc & 0xffffffffull);
        carry = acc >> 32;
    }
    limb[kLimbs] = limb[kLimbs + 1] = 0u;
    const bool negative = carry < 0;   // what is left is the sign: 0 or -1
    if (negative) {
        unsigned long long c = 1;
        for (uint32_t j = 0; j < kLimbs; ++j) {
            c += (unsigned long long)(~limb[j]);
            limb[j] = (uint32_t)(c & 0xffffffffull);
            c >>= 32;
        }
    }
    int top = -1;
    for (int j = (int)kLimbs - 1; j >= 0 && top < 0; --j)
        if (limb[j]) {
            int b = 31;
            while (!(limb[j] >> b)) --b;
            top = 32 * j + b;
        }
    unsigned long long bits = 0;
    if (top >= 0) {
        unsigned long long mant;   // 53 bits, the top one set
        if (top <= 52) {
            mant = ((unsigned long long)limb[1] << 32 | limb[0]) << (52 - top);   // exact
        } else {
            const uint32_t p = (uint32_t)top - 52u, g = p - 1u;   // the mantissa's lowest bit, the guard bit
            const uint32_t lw = p >> 5, off = p & 31u;
            const unsigned long long lo64 = (unsigned long long)limb[lw + 1] << 32 | limb[lw];
            mant = (off ? (lo64 >> off) | ((unsigned long long)limb[lw + 2] << (64u - off)) : lo64) & ((1ull << 53) - 1ull);
            const uint32_t guard = (limb[g >> 5] >> (g & 31u)) & 1u;
            uint32_t sticky = limb[g >> 5] & ((1u << (g & 31u)) - 1u);
            for (uint32_t j = 0; j < (g >> 5); ++j) sticky |= limb[j];
            if (guard && (sticky || (mant & 1ull))) ++mant;   // 2^53 after the increment: the addition below carries into the exponent
        }
        bits = ((unsigned long long)(top + 874) << 52) + (mant - (1ull << 52));   // biased exponent top - 149 + 1023
    }
    if (negative) bits |= 1ull << 63;
    double r;
    __builtin_memcpy(&r, &bits, 8);
    return r;
}

// A slot of the accumulating tables -> the record: the sum rounded, the keys turned into floats (NaN where there was no element).
WT_HD film_zonal_rec_t fz_finish(const film_zonal_slot_t& s) {
    film_zonal_rec_t r;
    for (uint32_t i = 0; i < FZ_COUNTS; ++i) r.count[i] = s.count[i];
    r.min = fs_unkey(s.min_inv ? ~s.min_inv : 0u);
    r.max = fs_unkey(s.max_key);
    r.sum = fz_round(s.w);
    return r;
}
// What a pixel of a zone is painted with: the zone's mean over its finite elements as one f32, 0 where it has none.
WT_HD float fz_paint(const film_zonal_rec_t& r) {
    const unsigned long long n_finite = r.count[FZ_N] - r.count[FZ_NAN] - r.count[FZ_INF];
    return n_finite ? (float)(r.sum / (double)n_finite) : 0.f;
}

}   // namespace wt
