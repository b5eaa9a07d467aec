// wave_tracer_amd — connected segments of a label plane (wtgpu_film_segments_*): the definitions the device kernels (kernels_segments.hip) and
// their host twin share.  There is no floating-point arithmetic here beyond the mask's comparison, so both sides agree bit for bit.
//
// Member.  Pixel p is a member iff (there is no mask or mask[p] > 0 — false for a NaN) and its class is not 0xFFFFFFFF, the id maps' "no hit".
//          Without a class plane every pixel has class 0.  seg_class gives a member's class and kSegNone for a pixel that is no member, so
// Link.    two neighbours are linked iff seg_linked(seg_class(p), seg_class(q)): both members, the same class.
// Record.  What is kept of a segment: class, area, smallest pixel index, inclusive bounding box, u64 coordinate sums.  Two records of one
//          segment merge by integer +, min and max (seg_merge), so the order in which pixels arrive does not matter.
#pragma once
#include "core.h"

namespace wt {

constexpr uint32_t kSegNone = 0xffffffffu;        // no member / no segment / the class "no hit"
constexpr uint64_t kSegMaxPixels = 1ull << 31;    // sensors of this many pixels or more are refused (pixel indices and areas are u32)
enum film_segments_flag_e : uint32_t { SEG_DIAGONAL = 1 };

WT_HD uint32_t seg_class(const uint32_t* classes, const float* mask, uint64_t p) {
    if (mask && !(mask[p] > 0.f)) return kSegNone;
    return classes ? classes[p] : 0u;
}
WT_HD bool seg_linked(uint32_t class_a, uint32_t class_b) { return class_a != kSegNone && class_a == class_b; }

// wtgpu_film_segment
struct film_segment_t {
    uint32_t klass, area, first, x0, y0, x1, y1, pad;
    unsigned long long sum_x, sum_y;
};
static_assert(sizeof(film_segment_t) == 48, "wtgpu_film_segment");

// the record of `n` pixels of class `klass` that lie side by side in row y from x on, the first of them pixel p
WT_HD film_segment_t seg_of_run(uint32_t klass, uint32_t p, uint32_t x, uint32_t y, uint32_t n) {
    return film_segment_t{klass, n, p, x, y, x + n - 1u, y, 0u, (unsigned long long)n * x + (unsigned long long)n * (n - 1u) / 2u, (unsigned long long)n * y};
}
// a += b, two parts of one segment
WT_HD void seg_merge(film_segment_t& a, const film_segment_t& b) {
    a.area += b.area;
    a.first = a.first < b.first ? a.first : b.first;
    a.x0 = a.x0 < b.x0 ? a.x0 : b.x0;
    a.y0 = a.y0 < b.y0 ? a.y0 : b.y0;
    a.x1 = a.x1 > b.x1 ? a.x1 : b.x1;
    a.y1 = a.y1 > b.y1 ? a.y1 : b.y1;
    a.sum_x += b.sum_x;
    a.sum_y += b.sum_y;
}

}   // namespace wt
