// wave_tracer_amd — exact Euclidean distance transform of a label plane with the nearest site (wtgpu_film_distance_*): the definitions the device
// kernels (kernels_distance.hip) and their host twin share.  All arithmetic is integer — squared pixel distances and pixel indices — so both sides
// agree bit for bit.
//
// Site.       The members of wt/film_segments.h (seg_class), or with DIST_INVERT the pixels that are no members.  The film's outside holds no site.
// Candidate.  A site seen from a pixel, as one 64-bit key (d² << 32) | index, index the site's row-major pixel index: keys compare as (d², index)
//             does, the order is total, and kDistNoKey — larger than every site's key — is "no site" (its halves are the 0xFFFFFFFF both planes
//             then hold).  A sensor is at most kDistMaxSide pixels wide and high: d² <= 2 x 32767² < 2^31, an index stays below 2^30.
// The decomposition rests on two facts:
//   1. Within one column c the best site for row y under (d², index) is the vertically nearest one: (x - c)² is the same for all of the column's
//      sites, so d² orders them by |dy|.  Where the one above and the one below are equally far the upper one wins, because its index
//      (y + dy) W + c is the smaller — hence dist_col_pick's strict comparison: a tie goes to the negative offset.
//   2. The global minimum under (d², index) is the minimum over the columns of each column's best candidate: a minimum over a union of sets is the
//      minimum of the sets' minima, whatever the (total) order — and for the same reason it depends on no order in which columns are visited.
// Column step: dist_col_step / dist_col_pick give the signed offset dy to the column's best site row per pixel, kDistNoDy where the column holds
// none.  Row step: dist_row_try takes column c's candidate for pixel (x, y) into the best key; dist_row_done says when an outward search over
// columns x -+ k, k = 0, 1, ..., has nothing left to find.
#pragma once
#include "core.h"
#include "film_segments.h"

namespace wt {

constexpr uint32_t kDistNone = 0xffffffffu;                  // dist2 and nearest where the plane holds no site
constexpr unsigned long long kDistNoKey = ~0ull;             // the candidate "no site"
constexpr uint32_t kDistMaxSide = 32768u;                    // wider or higher sensors are refused
constexpr int kDistNoDy = -32768;                            // the 16-bit offset "no site in this column"
enum film_distance_flag_e : uint32_t { DIST_INVERT = 1 };

// the membership test is the segments'; a site is a member, or with `invert` a pixel that is none
WT_HD bool dist_site(const uint32_t* classes, const float* mask, uint64_t p, bool invert) { return (seg_class(classes, mask, p) != kSegNone) != invert; }

// ---- candidates ---------------------------------------------------------------------------------------------------------------------------------
WT_HD unsigned long long dist_key(uint32_t d2, uint32_t index) { return ((unsigned long long)d2 << 32) | index; }
WT_HD uint32_t dist_key_d2(unsigned long long key) { return (uint32_t)(key >> 32); }
WT_HD uint32_t dist_key_index(unsigned long long key) { return (uint32_t)key; }
// (d², index) of a before b
WT_HD bool dist_before(unsigned long long a, unsigned long long b) { return a < b; }

// ---- the column step ------------------------------------------------------------------------------------------------------------------------------
// One walk along a column: the offset to the last site met, from the previous row's offset.  dir = -1 walking down (the site lies above: the
// offset falls), +1 walking up.  A column of at most kDistMaxSide rows keeps |offset| <= 32767.
WT_HD int dist_col_step(int prev, bool site, int dir) { return site ? 0 : (prev == kDistNoDy ? kDistNoDy : prev + dir); }
// the better of the offsets to the nearest site above (down <= 0) and below (up >= 0), either of which may be kDistNoDy; fact 1: up must be
// strictly nearer to win
WT_HD int dist_col_pick(int down, int up) {
    if (up == kDistNoDy) return down;
    if (down == kDistNoDy) return up;
    return up < -down ? up : down;
}
// |dy| for the groups' minima: 0xFFFF for kDistNoDy, above every offset
WT_HD uint32_t dist_abs_dy(int dy) { return dy == kDistNoDy ? 0xffffu : (uint32_t)(dy < 0 ? -dy : dy); }

// ---- the row step ---------------------------------------------------------------------------------------------------------------------------------
// column c's best candidate seen from pixel (x, y) of a plane W wide, dy the column's offset in row y
WT_HD unsigned long long dist_row_cand(int dy, uint32_t x, uint32_t c, uint32_t y, uint32_t W) {
    if (dy == kDistNoDy) return kDistNoKey;
    const uint32_t dx = x > c ? x - c : c - x;
    return dist_key(dx * dx + (uint32_t)(dy * dy), (uint32_t)((int)y + dy) * W + c);
}
// fact 2: best = min(best, column c's candidate)
WT_HD void dist_row_try(unsigned long long& best, int dy, uint32_t x, uint32_t c, uint32_t y, uint32_t W) {
    const unsigned long long cand = dist_row_cand(dy, x, c, y, W);
    if (dist_before(cand, best)) best = cand;
}
// An outward search that has taken every column at |dx| < k is done when k² > best d² — a column at |dx| >= k cannot reach the best, while one at
// k² == best d² can still tie it, and the smaller index then wins — or when both x - k and x + k lie outside the plane.  k <= 32767: k² fits.
WT_HD bool dist_row_done(unsigned long long best, uint32_t k, uint32_t x, uint32_t W) { return k * k > dist_key_d2(best) || (k > x && x + k >= W); }
// the same for a whole span of columns whose nearest lies `edge` columns away and whose smallest |dy| is min_dy (0xFFFF: no site in it): it
// cannot reach or tie the best
WT_HD bool dist_group_skipped(unsigned long long best, uint32_t edge, uint32_t min_dy) { return min_dy == 0xffffu || edge * edge + min_dy * min_dy > dist_key_d2(best); }

// the key of the maximum: (d², lowest pixel index) as one number whose maximum is wanted
WT_HD unsigned long long dist_max_key(uint32_t d2, uint32_t pixel) { return ((unsigned long long)d2 << 32) | (uint32_t)~pixel; }

}   // namespace wt
