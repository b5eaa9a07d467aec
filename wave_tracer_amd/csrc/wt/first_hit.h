// wave_tracer_amd — first-hit maps of a perspective sensor (wtgpu_first_hit / wtgpu_first_hit_host, csrc/kernels_firsthit.hip): what a pixel's
// primary rays see first — coverage, depth, position, the geometric and the shading normal, uv, facing, shape and triangle ids.  The rays are
// the sensor mask's (wt/sources.h: persp_sample_mean_ray; `samples` = 0: the one ray through the pixel's centre, no draw), the hit is the ray
// query's (wt/bvh.h: ads_intersect_ray) and the surface is the integrators' (wt/beam.h: make_surface, normal maps included): nothing is
// restated here.  The device kernels and the host twin run fh_sample, seq_add and fh_mean, so they agree bit for bit.
#pragma once
#include "beam.h"
#include "bvh.h"
#include "sources.h"

namespace wt {

// bits of wtgpu_first_hit_spec::maps, in the order of the floats of a pixel, and of ::ids
enum first_hit_map_e : uint32_t {
    FH_COVERAGE = 1, FH_DEPTH = 2, FH_POSITION = 4, FH_NORMAL_GEO = 8, FH_NORMAL_SHADING = 16, FH_UV = 32, FH_FACING = 64, FH_ALL_MAPS = 127
};
enum first_hit_id_e : uint32_t { FH_SHAPE = 1, FH_TRIANGLE = 2, FH_ALL_IDS = 3 };
constexpr uint32_t kFhSurfaceMaps = FH_NORMAL_GEO | FH_NORMAL_SHADING | FH_UV;   // the maps that need make_surface
constexpr uint32_t kFhMaxSamples = 4096;
// the floats of a sample, all maps asked for: 0 coverage (of the pixel, not of a sample), 1 depth, 2-4 position, 5-7 geometric normal,
// 8-10 shading normal, 11-12 uv, 13 facing
constexpr uint32_t kFhFloats = 14;

WT_HD uint32_t fh_map_floats(uint32_t maps) {
    return (maps & FH_COVERAGE ? 1u : 0u) + (maps & FH_DEPTH ? 1u : 0u) + (maps & FH_POSITION ? 3u : 0u) + (maps & FH_NORMAL_GEO ? 3u : 0u) +
           (maps & FH_NORMAL_SHADING ? 3u : 0u) + (maps & FH_UV ? 2u : 0u) + (maps & FH_FACING ? 1u : 0u);
}
WT_HD uint32_t fh_id_words(uint32_t ids) { return (ids & FH_SHAPE ? 1u : 0u) + (ids & FH_TRIANGLE ? 1u : 0u); }
// where float j of the full set goes among the pixel's floats for the chosen `maps`: the floats of the lower bits, then its place in its own
// map; -1: its map is not asked for
WT_HD int fh_slot(uint32_t maps, uint32_t j) {
    const uint32_t bit = j == 0 ? FH_COVERAGE : j == 1 ? FH_DEPTH : j < 5 ? FH_POSITION : j < 8 ? FH_NORMAL_GEO : j < 11 ? FH_NORMAL_SHADING : j < 13 ? FH_UV : FH_FACING;
    const uint32_t first = j == 0 ? 0u : j == 1 ? 1u : j < 5 ? 2u : j < 8 ? 5u : j < 11 ? 8u : j < 13 ? 11u : 13u;
    return maps & bit ? (int)(fh_map_floats(maps & (bit - 1u)) + (j - first)) : -1;
}

// what one sample sees (v[0] is not used)
struct fh_sample_t {
    uint32_t shape, tri;
    float v[kFhFloats];
};
// the running sums of a pixel over its hitting samples, and the ids of the first of them
struct fh_sums_t {
    uint32_t n_hit;
    uint32_t shape, tri;
    float v[kFhFloats];
};

// The ray of sample s of pixel (px, py): with `samples` >= 1 the mask's ray (the draws of make_sampler(seed, p * samples + s, STREAM_MASK)),
// with 0 the ray through the pixel's centre — the same statement with the offset (0, 0).
WT_HD void fh_ray(const sensor_t& sn, uint32_t px, uint32_t py, uint32_t samples, uint32_t s, uint64_t seed, vec3& ro, vec3& rd) {
    if (samples) {
        const uint64_t pixel = (uint64_t)py * sn.width + px;
        sampler_t smp = make_sampler(seed, pixel * samples + s, STREAM_MASK);
        persp_sample_mean_ray(sn, px, py, smp, ro, rd);
    } else
        persp_mean_ray(sn, px, py, vec2{0.f, 0.f}, ro, rd);
}

// Sample s of a pixel: FALSE if its ray hits nothing (r is then all 0 and no id).  surface = false leaves the normals and uv 0 (no tri_shade
// load, no frames).
template <bool surface>
WT_HD bool fh_sample(const scene_t& sc, uint32_t px, uint32_t py, uint32_t samples, uint32_t s, uint64_t seed, const stack_ref_t& stack, fh_sample_t& r) {
    r.shape = r.tri = 0xFFFFFFFFu;
    for (uint32_t j = 0; j < kFhFloats; ++j) r.v[j] = 0.f;
    vec3 ro, rd;
    fh_ray(sc.sensor, px, py, samples, s, seed, ro, rd);
    ray_hit_t h;
    if (!ads_intersect_ray(sc, ro, rd, range_t{0.f, WT_INF}, stack, h)) return false;
    const tri_meta_t m = sc.tri_meta[h.tuid];
    r.shape = m.shape_idx;
    r.tri = m.shape_tri_idx;
    const vec3 wp = ro + rd * h.dist;
    r.v[1] = h.dist;
    r.v[2] = wp.x, r.v[3] = wp.y, r.v[4] = wp.z;
    if (surface) {
        const surface_t srf = make_surface(sc, h.tuid, sc.tri_geo[h.tuid].n, vec2{h.bx, h.by}, wp);
        r.v[5] = srf.geo.n.x, r.v[6] = srf.geo.n.y, r.v[7] = srf.geo.n.z;
        r.v[8] = srf.shading.n.x, r.v[9] = srf.shading.n.y, r.v[10] = srf.shading.n.z;
        r.v[11] = srf.uv.x, r.v[12] = srf.uv.y;
    }
    r.v[13] = h.front_face ? 1.f : 0.f;
    return true;
}

// the mean of a sum (wt/core.h: seq_add) over n_hit hitting samples (0 without a hit: the sum is 0)
WT_HD float fh_hit_mean(float sum, uint32_t n_hit) { return sum / (n_hit ? float(n_hit) : 1.f); }
// float j of a pixel from its sum over n_hit hitting samples of `samples`: the coverage, or the mean
WT_HD float fh_mean(uint32_t j, float sum, uint32_t n_hit, uint32_t samples) {
    return j == 0 ? float(n_hit) / float(samples ? samples : 1u) : fh_hit_mean(sum, n_hit);
}

// A pixel by one thread: its samples in order, each hit added to the sums.
template <bool surface>
WT_HD fh_sums_t fh_pixel(const scene_t& sc, uint32_t px, uint32_t py, uint32_t samples, uint64_t seed, const stack_ref_t& stack) {
    fh_sums_t a;
    a.n_hit = 0;
    a.shape = a.tri = 0xFFFFFFFFu;
    for (uint32_t j = 0; j < kFhFloats; ++j) a.v[j] = 0.f;
    const uint32_t n = samples ? samples : 1u;
    for (uint32_t s = 0; s < n; ++s) {
        fh_sample_t r;
        if (!fh_sample<surface>(sc, px, py, samples, s, seed, stack, r)) continue;
        const bool first = a.n_hit == 0;
        if (first) a.shape = r.shape, a.tri = r.tri;
#pragma unroll
        for (uint32_t j = 1; j < kFhFloats; ++j) a.v[j] = seq_add(first, a.v[j], r.v[j]);
        ++a.n_hit;
    }
    return a;
}

// The pixel's K floats and Ki ids, contiguous, in bit order.  m / id may be null when no bit of theirs is set.
WT_HD void fh_write(const fh_sums_t& a, uint32_t samples, uint32_t maps, uint32_t ids, float* m, uint32_t* id) {
#pragma unroll
    for (uint32_t j = 0; j < kFhFloats; ++j)
        if (fh_slot(maps, j) >= 0) *m++ = fh_mean(j, a.v[j], a.n_hit, samples);   // (the slots come in the order of j)
    if (ids & FH_SHAPE) *id++ = a.shape;
    if (ids & FH_TRIANGLE) *id++ = a.tri;
}

}   // namespace wt
