// wave_tracer_amd — line-of-sight maps (wtgpu_line_of_sight / wtgpu_line_of_sight_host, csrc/kernels_los.hip): which emitters a sensor element,
// or a caller's point, can see.  The points of a virtual-plane sensor are those of its own sampling (wt/sources.h: vplane_element_point), the
// visibility test is the integrators' (wt/bvh.h: ads_shadow_ray): nothing is restated here.  f32 + - x /, comparisons and sqrtf only (no libm
// call: spot_falloff's acosf is deliberately not part of this), so the device kernels and the host twin, which run los_point, los_sample,
// seq_add, los_mean and los_nearest_step, agree bit for bit.
#pragma once
#include "bvh.h"
#include "sources.h"

namespace wt {

// bits of wtgpu_los_spec::maps (per element and emitter), ::elem and ::ids (per element), in the order of the floats / words, and of ::flags
enum los_map_e : uint32_t { LOS_VISIBLE = 1, LOS_DISTANCE = 2, LOS_DIRECTION = 4, LOS_COS = 8, LOS_ALL_MAPS = 15 };
enum los_elem_e : uint32_t { LOS_POINT = 1, LOS_NEAREST_DISTANCE = 2, LOS_ALL_ELEM = 3 };
enum los_id_e : uint32_t { LOS_N_VISIBLE = 1, LOS_NEAREST = 2, LOS_ALL_IDS = 3 };
enum los_flag_e : uint32_t { LOS_FRONT_ONLY = 1, LOS_ALL_FLAGS = 1 };
constexpr uint32_t kLosMaxSamples = 4096, kLosMaxEmitters = 32, kLosNone = 0xFFFFFFFFu;
// the floats of a pair (element, emitter), all maps asked for: 0 visible (of the pair, not of a sample), 1 distance, 2-4 direction, 5 cos
constexpr uint32_t kLosFloats = 6;
constexpr uint32_t kLosVectorMaps = LOS_DIRECTION | LOS_COS;   // the maps whose sums a VISIBLE / DISTANCE / ids query does not keep

// A query as the kernels and the host twin take it: the spec after its checks, the selection resolved.  points / normals / mask: null, or one
// entry per element (device memory for the kernels, host memory for the twin).
struct los_query_t {
    uint32_t samples, maps, elem, ids, flags, n_emitters;
    uint32_t emitters[kLosMaxEmitters];   // indices into scene_t::emitters
    float t_min;
    uint64_t seed;
    const float* points;    // [height][width][3], or null: the elements of the virtual-plane sensor
    const float* normals;   // [height][width][3], or null (caller points without a normal; the sensor's elements have frame.n)
    const float* mask;      // [height][width], or null: an element with mask <= 0 traces nothing
};

WT_HD uint32_t los_map_floats(uint32_t maps) {
    return (maps & LOS_VISIBLE ? 1u : 0u) + (maps & LOS_DISTANCE ? 1u : 0u) + (maps & LOS_DIRECTION ? 3u : 0u) + (maps & LOS_COS ? 1u : 0u);
}
WT_HD uint32_t los_elem_floats(uint32_t elem) { return (elem & LOS_POINT ? 3u : 0u) + (elem & LOS_NEAREST_DISTANCE ? 1u : 0u); }
WT_HD uint32_t los_id_words(uint32_t ids) { return (ids & LOS_N_VISIBLE ? 1u : 0u) + (ids & LOS_NEAREST ? 1u : 0u); }
// where float j of the full set goes among a pair's floats for the chosen `maps` (as fh_slot); -1: its map is not asked for
WT_HD int los_slot(uint32_t maps, uint32_t j) {
    const uint32_t bit = j == 0 ? LOS_VISIBLE : j == 1 ? LOS_DISTANCE : j < 5 ? LOS_DIRECTION : LOS_COS;
    const uint32_t first = j == 0 ? 0u : j == 1 ? 1u : j < 5 ? 2u : 5u;
    return maps & bit ? (int)(los_map_floats(maps & (bit - 1u)) + (j - first)) : -1;
}
WT_HD bool los_has_normal(const los_query_t& q) { return q.points ? q.normals != nullptr : true; }

// The point a sample starts from, its normal (0 where there is none) and whether it counts at all: the element is not masked out and every
// coordinate is finite.  A point that does not count is (0, 0, 0) and adds 0 to every sum.
struct los_point_t {
    vec3 p, n;
    bool ok;
};
// Sample s of element (px, py): a caller's point, or the sensor's own — with `samples` >= 1 at the offset drawn from
// make_sampler(seed, (py W + px) samples + s, STREAM_LOS), with 0 the element's centre (the same statement with the offset (0, 0), no draw).
WT_HD los_point_t los_point(const scene_t& sc, const los_query_t& q, uint32_t px, uint32_t py, uint32_t s) {
    const uint64_t el = (uint64_t)py * sc.sensor.width + px;
    los_point_t r;
    r.p = r.n = vec3{0.f, 0.f, 0.f};
    r.ok = false;
    if (q.mask && !(q.mask[el] > 0.f)) return r;
    vec3 p;
    if (q.points) {
        p = vec3{q.points[el * 3], q.points[el * 3 + 1], q.points[el * 3 + 2]};
        if (q.normals) r.n = vec3{q.normals[el * 3], q.normals[el * 3 + 1], q.normals[el * 3 + 2]};
    } else {
        vec2 o{0.f, 0.f};
        if (q.samples) {
            sampler_t smp = make_sampler(q.seed, el * q.samples + s, STREAM_LOS);
            o = sampler_r2(smp) - vec2{.5f, .5f};
        }
        p = vplane_element_point(sc.sensor, px, py, o);
        r.n = sc.sensor.frame.n;
    }
    if (!(finitef(p.x) && finitef(p.y) && finitef(p.z))) {
        r.n = vec3{0.f, 0.f, 0.f};
        return r;
    }
    r.p = p;
    r.ok = true;
    return r;
}

// What the query reads of an emitter's record: seven words, read once per pair (k_los_pair) or once per emitter by the whole wavefront (k_los_sample).
struct los_target_t {
    int32_t type;
    vec3 position, n;   // n: the direction TO a directional emitter
};
WT_HD los_target_t los_target(const emitter_t& e) { return {e.type, e.position, e.frame.n}; }

// What a sample sees of one emitter (v[0] is not used): the distance, the direction to it and its cosine with the normal — all 0 for a sample
// that does not count (its point does not, or the emitter is not at a finite distance > 0) — and whether the emitter is visible from it.
struct los_sample_t {
    float v[kLosFloats];
    bool visible;
};
WT_HD los_sample_t los_sample(const scene_t& sc, const los_query_t& q, const los_point_t& pt, const los_target_t& e, const stack_ref_t& stack) {
    los_sample_t r;
    for (uint32_t j = 0; j < kLosFloats; ++j) r.v[j] = 0.f;
    r.visible = false;
    if (!pt.ok) return r;
    vec3 dir;
    float dist = 0.f;
    range_t range{q.t_min, WT_INF};
    if (e.type == EMIT_DIRECTIONAL)
        dir = e.n;   // (its distance counts as 0)
    else {
        const vec3 v = e.position - pt.p;
        dist = length(v);
        if (!(finitef(dist) && dist > 0.f)) return r;
        dir = v / dist;
        range.max = dist;
    }
    const float c = los_has_normal(q) ? dot(dir, pt.n) : 0.f;
    r.v[1] = dist;
    r.v[2] = dir.x, r.v[3] = dir.y, r.v[4] = dir.z;
    r.v[5] = c;
    if ((q.flags & LOS_FRONT_ONLY) && los_has_normal(q) && !(c > 0.f)) return r;
    r.visible = !ads_shadow_ray(sc, pt.p, dir, range, stack);
    return r;
}

// float j of a pair from its sum (wt/core.h: seq_add) over ALL samples: the visible share, or the mean; the same division serves the mean point
WT_HD float los_mean(float sum, uint32_t samples) { return sum / float(samples ? samples : 1u); }
WT_HD float los_visible(uint32_t n_visible, uint32_t samples) { return float(n_visible) / float(samples ? samples : 1u); }

// The sums of a pair by one thread: its samples in order.
struct los_sums_t {
    uint32_t n_visible;
    float v[kLosFloats];
};
template <bool vectors>
WT_HD los_sums_t los_pair(const scene_t& sc, const los_query_t& q, uint32_t px, uint32_t py, const los_target_t& e, const stack_ref_t& stack) {
    los_sums_t a;
    a.n_visible = 0;
    for (uint32_t j = 0; j < kLosFloats; ++j) a.v[j] = 0.f;
    const uint32_t n = q.samples ? q.samples : 1u;
    for (uint32_t s = 0; s < n; ++s) {
        const los_point_t pt = los_point(sc, q, px, py, s);
        const los_sample_t r = los_sample(sc, q, pt, e, stack);
        a.n_visible += r.visible ? 1u : 0u;
        a.v[1] = seq_add(s == 0, a.v[1], r.v[1]);
        if (vectors) {
#pragma unroll
            for (uint32_t j = 2; j < kLosFloats; ++j) a.v[j] = seq_add(s == 0, a.v[j], r.v[j]);
        }
    }
    return a;
}
// The pair's floats, contiguous, in bit order (the slots come in the order of j).
WT_HD void los_write_pair(const los_sums_t& a, uint32_t samples, uint32_t maps, float* m) {
#pragma unroll
    for (uint32_t j = 0; j < kLosFloats; ++j)
        if (los_slot(maps, j) >= 0) *m++ = j == 0 ? los_visible(a.n_visible, samples) : los_mean(a.v[j], samples);
}
// The sum of an element's sample points, in sample order.
WT_HD vec3 los_point_sum(const scene_t& sc, const los_query_t& q, uint32_t px, uint32_t py) {
    vec3 sum{0.f, 0.f, 0.f};
    const uint32_t n = q.samples ? q.samples : 1u;
    for (uint32_t s = 0; s < n; ++s) {
        const los_point_t pt = los_point(sc, q, px, py, s);
        sum = vec3{seq_add(s == 0, sum.x, pt.p.x), seq_add(s == 0, sum.y, pt.p.y), seq_add(s == 0, sum.z, pt.p.z)};
    }
    return sum;
}

// What an element knows of its emitters, taken in the order of the selection: how many it sees (at least one visible sample) and the nearest
// of those by mean distance — the lowest index wins a tie, a directional emitter counts with distance 0.
struct los_nearest_t {
    uint32_t n_visible, nearest;
    float distance;
};
WT_HD los_nearest_t los_nearest_none() { return {0u, kLosNone, 0.f}; }
WT_HD void los_nearest_step(los_nearest_t& a, uint32_t k, uint32_t n_visible, float mean_distance) {
    if (!n_visible) return;
    ++a.n_visible;
    if (a.nearest == kLosNone || mean_distance < a.distance) a.nearest = k, a.distance = mean_distance;
}
// The element's floats and ids, contiguous, in bit order.  m / id may be null when no bit of theirs is set.
WT_HD void los_write_element(const los_nearest_t& a, vec3 point_sum, uint32_t samples, uint32_t elem, uint32_t ids, float* m, uint32_t* id) {
    if (elem & LOS_POINT) *m++ = los_mean(point_sum.x, samples), *m++ = los_mean(point_sum.y, samples), *m++ = los_mean(point_sum.z, samples);
    if (elem & LOS_NEAREST_DISTANCE) *m++ = a.distance;
    if (ids & LOS_N_VISIBLE) *id++ = a.n_visible;
    if (ids & LOS_NEAREST) *id++ = a.nearest;
}

}   // namespace wt
