// wave_tracer_amd — by-geometry sensor masks (include/wt/sensor/mask/mask.hpp, src/sensor/mask.cpp:28-66; see wtgpu_kernels.h for the list of
// kernel translation units).  For every pixel of a perspective sensor, `samples` jittered primary rays (the sensor's own pixel sampling at
// k = 0) are traced to their closest hit; the mask is the share of them whose first hit lies on a shape that does NOT match the mask's regex
// (a miss counts as nothing).  The reference accumulates 1 / float(samples) per such sample in a float: the integer count is reproduced
// here as that same sequential f32 sum (mask_value), so the device, the host threads and the reference agree bit for bit.
// No render kernel is compiled here.
#include "kernels_maps.h"

namespace wtk {

// mask.cpp:48-57: one sample of pixel (px, py) — TRUE if its mean ray hits a shape whose flag is 0 (the id does not match the regex).
// Sample s of pixel p draws from make_sampler(seed, p * samples + s, STREAM_MASK); ray query of k_trace_rays over the default range [0, inf).
WT_HD bool mask_sample_counts(const scene_t& sc, const uint8_t* shape_matches, uint32_t px, uint32_t py, uint32_t samples, uint32_t s, uint64_t seed,
                              const stack_ref_t& stack) {
    const uint64_t pixel = (uint64_t)py * sc.sensor.width + px;
    sampler_t smp = make_sampler(seed, pixel * samples + s, STREAM_MASK);
    vec3 ro, rd;
    persp_sample_mean_ray(sc.sensor, px, py, smp, ro, rd);
    ray_hit_t h;
    if (!ads_intersect_ray(sc, ro, rd, range_t{0.f, WT_INF}, stack, h)) return false;
    return shape_matches[sc.tri_meta[h.tuid].shape_idx] == 0;
}
// `bmp(x,y,0) += 1/float(samples)` n times (mask.cpp:57), in that order
WT_HD float mask_value(uint32_t n, uint32_t samples) {
    const float inc = 1.f / float(samples);
    float v = 0.f;
    for (uint32_t i = 0; i < n; ++i) v += inc;
    return v;
}

// One lane per pixel (kernels_maps.h: on_lane_element): the lane traces the pixel's samples one after the other.
__global__ void __launch_bounds__(kBlock) k_sensor_mask_lane(scene_t sc, const uint8_t* shape_matches, uint32_t samples, uint64_t seed, float* out) {
    __shared__ stack_entry_t lds[kLdsStack * kBlock];
    const uint32_t W = sc.sensor.width;
    on_lane_element(lds, W * sc.sensor.height, [&](uint32_t p, const stack_ref_t& stack) {
        uint32_t n = 0;
        for (uint32_t s = 0; s < samples; ++s) n += mask_sample_counts(sc, shape_matches, p % W, p / W, samples, s, seed, stack) ? 1u : 0u;
        out[p] = mask_value(n, samples);
    });
}

// One lane per sample (samples <= 64; kernels_maps.h: sample_lane): the count of a pixel is the popcount of its lanes' bits in one ballot,
// written by the pixel's first lane.  Every lane reaches the ballot.
__global__ void __launch_bounds__(kBlock) k_sensor_mask_wave(scene_t sc, const uint8_t* shape_matches, uint32_t samples, uint64_t seed, float* out) {
    __shared__ stack_entry_t lds[kLdsStack * kBlock];
    const uint32_t W = sc.sensor.width;
    const sample_lane_t l = sample_lane(samples, W * sc.sensor.height);
    bool counts = false;
    if (l.active) {
        stack_entry_t spill[kSpillStack];
        stack_ref_t stack;
        lds_stack(lds, spill, stack);
        counts = mask_sample_counts(sc, shape_matches, (uint32_t)(l.p % W), (uint32_t)(l.p / W), samples, l.s, seed, stack);
    }
    const unsigned long long bits = __ballot(counts);
    if (l.active && l.s == 0) out[l.p] = mask_value((uint32_t)__popcll(group_bits(bits, l, samples)), samples);
}

int sensor_mask_launch(const scene_t& sc, hipStream_t stream, const uint8_t* d_shape_matches, uint32_t samples, uint64_t seed, float* d_out) {
    const uint64_t npix = (uint64_t)sc.sensor.width * sc.sensor.height;
    if (npix == 0 || samples == 0) return 0;
    // one lane per sample wherever a pixel's samples fit one wavefront: on the MI355X the radio overview (1440 x 1080, 32 samples) takes
    // 1.90 ms against 2.44 ms with one lane per pixel (median of 15 calls each, alternated); beyond 64 samples one lane per pixel
    if (samples <= 64u)
        hipLaunchKernelGGL(k_sensor_mask_wave, dim3(sample_blocks(npix, samples)), dim3(kBlock), 0, stream, sc, d_shape_matches, samples, seed, d_out);
    else
        hipLaunchKernelGGL(k_sensor_mask_lane, dim3(lane_blocks(npix)), dim3(kBlock), 0, stream, sc, d_shape_matches, samples, seed, d_out);
    return (int)hipGetLastError();
}

// The same computation on host threads, from the host description (kernels_maps.h: on_elements).
void sensor_mask_host(const scene_t& sc, const uint8_t* shape_matches, uint32_t samples, uint64_t seed, uint32_t n_threads, float* out) {
    on_elements(sc, n_threads, [&](uint32_t x, uint32_t y, size_t p, const stack_ref_t& stack) {
        uint32_t n = 0;
        for (uint32_t s = 0; s < samples; ++s) n += mask_sample_counts(sc, shape_matches, x, y, samples, s, seed, stack) ? 1u : 0u;
        out[p] = mask_value(n, samples);
    });
}

}   // namespace wtk
