// A stand-alone program over the host functions of wave_tracer_amd/csrc/wt/film_distance.h, for a sanitizer build (tests/test_film_distance.py compiles
// it with -fsanitize=undefined,address and runs it as a child process): the site test (the segments' member test, inverted or not, under a mask
// with NaN, zero, negative and -0 entries), the candidate's key and its order, the column step and pick — the tie that goes to the negative
// offset, the 16-bit range at the largest height —, the row step at the far corners of the largest sensor, where a signed product would overflow,
// the outward search's end and the group rule.  A small plane is then transformed with the header's steps and held against a brute force over
// all (pixel, site) pairs.  Prints "ok <checks>" and returns 0.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "wt/film_distance.h"

using namespace wt;

static int bad = 0, checks = 0;
#define CHECK(cond)                                                \
    do {                                                           \
        ++checks;                                                  \
        if (!(cond)) ++bad, std::printf("line %d: %s\n", __LINE__, #cond); \
    } while (0)

int main() {
    // sites
    const uint32_t classes[6] = {0u, 7u, kSegNone, 7u, 0xfffffffeu, 3u};
    const float mask[6] = {1.f, 0.f, 1.f, std::nanf(""), 1e-45f, -0.f};
    const bool member[6] = {true, false, false, false, true, false};
    for (uint32_t p = 0; p < 6; ++p) {
        CHECK(dist_site(classes, mask, p, false) == member[p] && dist_site(classes, mask, p, true) == !member[p]);
        CHECK(dist_site(nullptr, nullptr, p, false) && !dist_site(nullptr, nullptr, p, true));
        CHECK(dist_site(classes, nullptr, p, false) == (classes[p] != kSegNone));
    }
    // keys: (d², index) in this order; "no site" after every site
    CHECK(dist_before(dist_key(4u, 900u), dist_key(5u, 0u)) && dist_before(dist_key(4u, 3u), dist_key(4u, 4u)) && !dist_before(dist_key(4u, 4u), dist_key(4u, 4u)));
    CHECK(dist_before(dist_key(0x7fffffffu, 0x3fffffffu), kDistNoKey) && dist_key_d2(kDistNoKey) == kDistNone && dist_key_index(kDistNoKey) == kDistNone);
    CHECK(dist_key_d2(dist_key(25u, 311u)) == 25u && dist_key_index(dist_key(25u, 311u)) == 311u);
    // the column step: down a column of the largest height with its one site on top, and up one with its site at the bottom
    {
        int run = kDistNoDy;
        CHECK(dist_col_step(run, false, -1) == kDistNoDy && dist_col_step(run, false, +1) == kDistNoDy);
        run = dist_col_step(run, true, -1);
        for (uint32_t y = 1; y < kDistMaxSide; ++y) run = dist_col_step(run, false, -1);
        CHECK(run == -32767 && (int16_t)run == run && run != kDistNoDy);
        run = dist_col_step(kDistNoDy, true, +1);
        for (uint32_t y = 1; y < kDistMaxSide; ++y) run = dist_col_step(run, false, +1);
        CHECK(run == 32767 && (int16_t)run == run);
        CHECK(dist_col_step(-5, true, -1) == 0 && dist_col_step(5, true, +1) == 0);
    }
    // the pick: a tie goes to the negative offset (the upper site has the smaller index)
    CHECK(dist_col_pick(-3, 3) == -3 && dist_col_pick(-3, 2) == 2 && dist_col_pick(-2, 3) == -2 && dist_col_pick(0, 0) == 0);
    CHECK(dist_col_pick(kDistNoDy, 4) == 4 && dist_col_pick(-4, kDistNoDy) == -4 && dist_col_pick(kDistNoDy, kDistNoDy) == kDistNoDy);
    CHECK(dist_col_pick(-32767, 32767) == -32767 && dist_col_pick(-32767, 32766) == 32766);
    CHECK(dist_abs_dy(kDistNoDy) == 0xffffu && dist_abs_dy(-32767) == 32767u && dist_abs_dy(32767) == 32767u && dist_abs_dy(0) == 0u);
    // the row step at the corners of the largest sensor
    {
        const uint32_t W = kDistMaxSide, last = kDistMaxSide - 1u;
        const unsigned long long far = dist_row_cand(32767, 0u, last, 0u, W);      // from (0, 0) to the site (last, last)
        CHECK(dist_key_d2(far) == 2u * 32767u * 32767u && dist_key_d2(far) < 0x80000000u && dist_key_index(far) == last * W + last);
        const unsigned long long back = dist_row_cand(-32767, last, 0u, last, W);   // from (last, last) to the site (0, 0)
        CHECK(dist_key_d2(back) == 2u * 32767u * 32767u && dist_key_index(back) == 0u);
        CHECK(dist_row_cand(kDistNoDy, 5u, 9u, 3u, W) == kDistNoKey);
        unsigned long long best = kDistNoKey;
        dist_row_try(best, kDistNoDy, 0u, 1u, 0u, W);
        CHECK(best == kDistNoKey);
        dist_row_try(best, 2, 2u, 0u, 0u, 37u);   // the site (0, 2) seen from (2, 0)
        dist_row_try(best, 0, 2u, 2u, 0u, 37u);   // the pixel itself
        CHECK(best == dist_key(0u, 2u));
        // the end of the outward search: a column at k² == best can still tie, one beyond cannot; both sides outside the plane
        CHECK(!dist_row_done(dist_key(25u, 0u), 5u, 100u, 1000u) && dist_row_done(dist_key(25u, 0u), 6u, 100u, 1000u) && !dist_row_done(kDistNoKey, 32767u, 32767u, W));
        CHECK(dist_row_done(kDistNoKey, 33u, 4u, 37u) && !dist_row_done(kDistNoKey, 32u, 4u, 37u) && !dist_row_done(kDistNoKey, 5u, 4u, 37u) && dist_row_done(kDistNoKey, 1u, 0u, 1u));
        // the group rule: skipped where it cannot reach or tie
        CHECK(dist_group_skipped(dist_key(25u, 0u), 3u, 5u) && !dist_group_skipped(dist_key(25u, 0u), 3u, 4u) && !dist_group_skipped(dist_key(25u, 0u), 5u, 0u));
        CHECK(dist_group_skipped(kDistNoKey, 1u, 0xffffu) && !dist_group_skipped(kDistNoKey, 32767u, 32767u) && dist_group_skipped(dist_key(0u, 0u), 1u, 0u));
        CHECK(dist_max_key(7u, 0u) > dist_max_key(7u, 1u) && dist_max_key(8u, 900u) > dist_max_key(7u, 0u) && dist_max_key(0u, 0x3fffffffu) > 0ull);
    }
    // a plane: the header's steps against a brute force over all pairs, both ways round
    const uint32_t W = 23, H = 17;
    std::vector<uint32_t> cls(W * H);
    std::vector<float> m(W * H);
    uint32_t state = 2024u;
    for (uint32_t p = 0; p < W * H; ++p) {
        state = state * 1664525u + 1013904223u;
        cls[p] = (state >> 24) % 9u == 0u ? 1u : kSegNone;
        m[p] = (state >> 16) % 5u == 0u ? 0.f : 1.f;
    }
    for (int invert = 0; invert < 2; ++invert) {
        std::vector<int16_t> dy(W * H);
        uint32_t n_sites = 0;
        for (uint32_t x = 0; x < W; ++x) {
            int run = kDistNoDy;
            for (uint32_t y = 0; y < H; ++y) {
                const bool site = dist_site(cls.data(), m.data(), y * W + x, invert != 0);
                n_sites += site ? 1u : 0u;
                dy[y * W + x] = (int16_t)(run = dist_col_step(run, site, -1));
            }
            run = kDistNoDy;
            for (uint32_t y = H; y-- > 0u;) {
                run = dist_col_step(run, dy[y * W + x] == 0, +1);
                dy[y * W + x] = (int16_t)dist_col_pick(dy[y * W + x], run);
            }
        }
        CHECK(n_sites > 10u && n_sites < W * H - 10u);
        uint32_t wrong = 0, searched = 0;
        for (uint32_t y = 0; y < H; ++y)
            for (uint32_t x = 0; x < W; ++x) {
                unsigned long long best = kDistNoKey, all = kDistNoKey;
                for (uint32_t k = 0; k < W && !dist_row_done(best, k, x, W); ++k, ++searched) {
                    if (k <= x) dist_row_try(best, dy[y * W + x - k], x, x - k, y, W);
                    if (k > 0u && x + k < W) dist_row_try(best, dy[y * W + x + k], x, x + k, y, W);
                }
                for (uint32_t c = 0; c < W; ++c) dist_row_try(all, dy[y * W + c], x, c, y, W);   // every column, whatever the search skipped
                unsigned long long brute = kDistNoKey;
                for (uint32_t q = 0; q < W * H; ++q)
                    if (dist_site(cls.data(), m.data(), q, invert != 0)) {
                        const int dx = (int)(q % W) - (int)x, ddy = (int)(q / W) - (int)y;
                        const unsigned long long key = dist_key((uint32_t)(dx * dx + ddy * ddy), q);
                        if (dist_before(key, brute)) brute = key;
                    }
                wrong += best != brute || all != brute ? 1u : 0u;
            }
        CHECK(wrong == 0u);
        CHECK(searched < W * H * W);   // the search ends early
    }
    if (bad) return 1;
    std::printf("ok %d\n", checks);
    return 0;
}
