// A stand-alone program over fz_add / fz_round (wave_tracer_amd/csrc/wt/film_zonal.h), for a sanitizer build (tests/test_film_zonal.py compiles it with
// -fsanitize=undefined,address and runs it as a child process): the shifts are where undefined behaviour would hide.  Every finite f32 exponent
// with the smallest, the largest and a middle mantissa, both signs, subnormals and zeros goes through fz_add — alone, where the rounded sum must
// be the element itself, and all together; then hand-made words through fz_round: every position of the top bit, ties, a carry out of the 53 bits,
// the largest and smallest totals nine words hold in 320 bits, an exact zero from non-zero words.  Prints "ok <elements>" and returns 0.
#include <cstdio>
#include <cstring>
#include <vector>

#include "wt/film_zonal.h"

using namespace wt;

static float from_bits(uint32_t u) {
    float x;
    std::memcpy(&x, &u, 4);
    return x;
}
static uint64_t bits_of(double d) {
    uint64_t u;
    std::memcpy(&u, &d, 8);
    return u;
}

int main() {
    std::vector<float> xs;
    for (uint32_t e = 0; e < 255; ++e)
        for (uint32_t frac : {0u, 1u, 0x2aaaaau, 0x400000u, 0x7fffffu})
            for (uint32_t sign : {0u, 0x80000000u}) xs.push_back(from_bits(sign | e << 23 | frac));
    int bad = 0;
    // one element: the sum is the element
    for (float x : xs) {
        unsigned long long w[kFzWords] = {0};
        fz_add(w, x);
        const double r = fz_round(w);
        if (bits_of(r) != bits_of(x == 0.f ? 0.0 : (double)x)) ++bad, std::printf("single element %a -> %a\n", (double)x, r);
    }
    // all of them, in two orders: the same words, and (every element is there with both signs) an exact zero
    unsigned long long a[kFzWords] = {0}, b[kFzWords] = {0};
    for (size_t i = 0; i < xs.size(); ++i) fz_add(a, xs[i]), fz_add(b, xs[xs.size() - 1 - i]);
    if (std::memcmp(a, b, sizeof a) != 0) ++bad, std::printf("the words depend on the order\n");
    if (bits_of(fz_round(a)) != 0) ++bad, std::printf("x and -x do not cancel: %a\n", fz_round(a));
    // the positive ones, 2^31 / 1024 times over (a word gains less than 2^32 per element): no word may wrap into its neighbour's meaning
    unsigned long long c[kFzWords] = {0};
    for (int rep = 0; rep < 4; ++rep)
        for (float x : xs)
            if (x > 0.f) fz_add(c, x);
    double want = 0.0;   // (a plain f64 sum is within a few ulps: this guards the magnitude, the tests hold the bits against math.fsum)
    for (float x : xs)
        if (x > 0.f) want += 4.0 * (double)x;
    const double got = fz_round(c);
    if (!(got > want * (1 - 1e-12) && got < want * (1 + 1e-12))) ++bad, std::printf("sum %a against %a\n", got, want);
    // hand-made words: a single bit at every position of the 9 x 64 bits that nine words in 320 bits can hold, and its negative
    for (uint32_t k = 0; k < kFzWords; ++k)
        for (uint32_t bit = 0; bit < (k == kFzWords - 1 ? 62u : 64u); ++bit) {
            unsigned long long w[kFzWords] = {0};
            w[k] = 1ull << bit;
            const double p = fz_round(w);
            for (uint32_t i = 0; i < kFzWords; ++i) w[i] = 0ull - w[i];
            const double n = fz_round(w);
            // word k, bit b: 2^(32 k + b - 149) if b < 63, else -2^(32 k + 63 - 149) (the word's sign bit)
            const int ex = (int)(32 * k + bit) - 149;
            const double v = std::ldexp(bit == 63 ? -1.0 : 1.0, ex);   // (the negative of a word's sign bit is itself)
            if (bits_of(p) != bits_of(v) || bits_of(n) != bits_of(bit == 63 ? v : -v)) ++bad, std::printf("word %u bit %u: %a / %a against %a\n", k, bit, p, n, v);
        }
    // ties to even, and a carry out of the 53 bits: N = 2^53 + 1 -> 2^53, 2^53 + 3 -> 2^53 + 4, 2^54 - 1 -> 2^54, at every shift
    for (uint32_t shift = 0; shift < 250; ++shift) {
        const unsigned long long N[3] = {(1ull << 53) + 1, (1ull << 53) + 3, (1ull << 54) - 1};
        const double want_units[3] = {9007199254740992.0, 9007199254740996.0, 18014398509481984.0};
        for (int i = 0; i < 3; ++i) {
            unsigned long long w[kFzWords] = {0};
            const uint32_t k = shift >> 5, off = shift & 31u;   // N << off is below 2^86: its low 32 bits in word k, the rest (below 2^54) in word k + 1
            const unsigned __int128 v = (unsigned __int128)N[i] << off;
            w[k] = (unsigned long long)(v & 0xffffffffu);
            w[k + 1] = (unsigned long long)(v >> 32);
            const double r = fz_round(w), v_want = std::ldexp(want_units[i], (int)(32 * k + off) - 149);
            if (bits_of(r) != bits_of(v_want)) ++bad, std::printf("tie %d at shift %u: %a against %a\n", i, shift, r, v_want);
        }
    }
    // an exact zero from non-zero words, and the extremes of 320 bits
    {
        unsigned long long w[kFzWords] = {1ull << 32, ~0ull, 0, 0, 0, 0, 0, 0, 0};   // 2^32 - 1 x 2^32
        if (bits_of(fz_round(w)) != 0) ++bad, std::printf("zero from words: %a\n", fz_round(w));
        unsigned long long hi[kFzWords], lo[kFzWords];
        for (uint32_t k = 0; k < kFzWords; ++k) hi[k] = 0x7fffffffffffffffull, lo[k] = 0x8000000000000000ull;
        hi[kFzWords - 1] >>= 1, lo[kFzWords - 1] = 0ull - (1ull << 62);
        const double h = fz_round(hi), l = fz_round(lo);
        if (!(h > 0 && l < 0 && h < 1e52 && l > -1e52)) ++bad, std::printf("extremes: %a %a\n", h, l);
    }
    if (bad) return 1;
    std::printf("ok %zu\n", xs.size());
    return 0;
}
