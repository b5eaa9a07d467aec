// wave_tracer_amd — first-hit maps of a perspective sensor (wtgpu_first_hit / wtgpu_first_hit_host; see wtgpu_kernels.h for the list of kernel
// translation units): per pixel the mean, over the primary rays that hit, of depth, position, normals, uv and facing, the share of rays that
// hit, and the shape and triangle of the first ray that does.  The rays are the sensor mask's (kernels_mask.hip) and the arithmetic is
// wt/first_hit.h's, which the host twin below runs too: device and host agree bit for bit.  No render kernel is compiled here.
#include "kernels_film.h"   // (on_threads)
#include "wt/first_hit.h"

namespace wtk {

// One lane per pixel, as k_sensor_mask_lane (the ray through the centre, more than 64 samples, WTGPU_FIRST_HIT_PER_SAMPLE=0): the lane traces the pixel's samples one after the other and keeps the sums in registers, then
// writes its K floats and Ki ids contiguously.  surface: any of the maps that need make_surface is asked for (depth / position / coverage /
// id queries load no tri_shade record and build no frame).
template <bool surface>
__global__ void __launch_bounds__(kBlock) k_first_hit(scene_t sc, uint32_t samples, uint64_t seed, uint32_t maps, uint32_t ids, float* out_maps,
                                                      uint32_t* out_ids) {
    __shared__ stack_entry_t lds[kLdsStack * kBlock];
    const uint32_t W = sc.sensor.width, npix = W * sc.sensor.height;
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= npix) return;
    stack_entry_t spill[kSpillStack];
    stack_ref_t stack;
    lds_stack(lds, spill, stack);
    const fh_sums_t a = fh_pixel<surface>(sc, p % W, p / W, samples, seed, stack);
    fh_write(a, samples, maps, ids, out_maps + (size_t)p * fh_map_floats(maps), out_ids + (size_t)p * fh_id_words(ids));
}

// One lane per sample (1 <= samples <= 64), as k_sensor_mask_wave: a wavefront holds 64 / samples pixels, lanes [g * samples, (g + 1) * samples)
// the samples of its g-th.  When every lane of the block has finished its ray the LDS of the stacks is free: each lane leaves its sample's floats
// and ids there (float j of thread t at [j * kBlock + t]), and lane j of a pixel's group — lanes j, j + samples, ... where a group is narrower
// than the floats — adds float j of the group's hitting samples in sample order, first term first, and stores the mean: the sums are the ones
// one thread would form, and neighbouring lanes store neighbouring floats.  Every lane reaches the ballot and the barriers.
constexpr uint32_t kFhExchange = kFhFloats + 2;   // floats per lane in the exchange: the sample's floats, its shape and its triangle
static_assert(kFhExchange * sizeof(float) <= kLdsStack * sizeof(stack_entry_t), "the exchange of the per-sample form must fit the LDS of the stacks");
template <bool surface>
__global__ void __launch_bounds__(kBlock) k_first_hit_wave(scene_t sc, uint32_t samples, uint64_t seed, uint32_t maps, uint32_t ids, float* out_maps,
                                                           uint32_t* out_ids) {
    __shared__ stack_entry_t lds[kLdsStack * kBlock];
    const uint32_t W = sc.sensor.width, npix = W * sc.sensor.height;
    const uint32_t per_wave = 64u / samples;
    const uint32_t lane = threadIdx.x & 63u, g = lane / samples, s = lane - g * samples;
    const uint64_t p = ((blockIdx.x * (uint64_t)kBlock + threadIdx.x) >> 6) * per_wave + g;
    const bool active = g < per_wave && p < npix;
    fh_sample_t r;
    bool hit = false;
    if (active) {
        stack_entry_t spill[kSpillStack];
        stack_ref_t stack;
        lds_stack(lds, spill, stack);
        hit = fh_sample<surface>(sc, (uint32_t)(p % W), (uint32_t)(p / W), samples, s, seed, stack, r);
    }
    const unsigned long long bits = __ballot(hit);
    __syncthreads();   // no lane of the block reads its stack any more
    float* ex = reinterpret_cast<float*>(lds);
    uint32_t* exu = reinterpret_cast<uint32_t*>(lds);
    if (hit) {
#pragma unroll
        for (uint32_t j = 1; j < kFhFloats; ++j) ex[j * kBlock + threadIdx.x] = r.v[j];
        exu[kFhFloats * kBlock + threadIdx.x] = r.shape;
        exu[(kFhFloats + 1) * kBlock + threadIdx.x] = r.tri;
    }
    __syncthreads();
    if (!active) return;
    const unsigned long long mine = samples == 64u ? bits : (bits >> (g * samples)) & ((1ull << samples) - 1ull);
    const uint32_t n_hit = (uint32_t)__popcll(mine), first_lane = threadIdx.x - s;   // (the group's first thread)
    float* m = out_maps + (size_t)p * fh_map_floats(maps);
    for (uint32_t j = s; j < kFhFloats; j += samples) {
        const int slot = fh_slot(maps, j);
        if (slot < 0) continue;
        float sum = 0.f;
        bool first = true;
        if (j != 0)
            for (uint32_t t = 0; t < samples; ++t)
                if ((mine >> t) & 1ull) {
                    sum = fh_add(first, sum, ex[j * kBlock + first_lane + t]);
                    first = false;
                }
        m[slot] = fh_mean(j, sum, n_hit, samples);
    }
    if (s == 0 && ids) {
        const uint32_t t = n_hit ? first_lane + (uint32_t)__ffsll((long long)mine) - 1u : 0u;
        uint32_t* id = out_ids + (size_t)p * fh_id_words(ids);
        if (ids & FH_SHAPE) *id++ = n_hit ? exu[kFhFloats * kBlock + t] : 0xFFFFFFFFu;
        if (ids & FH_TRIANGLE) *id++ = n_hit ? exu[(kFhFloats + 1) * kBlock + t] : 0xFFFFFFFFu;
    }
}

// per_sample (WTGPU_FIRST_HIT_PER_SAMPLE): one lane per sample wherever a pixel's samples fit one wavefront; else, and for the ray through the
// centre, one lane per pixel
template <bool surface>
static void first_hit_launch_as(const scene_t& sc, hipStream_t stream, uint32_t samples, uint64_t seed, uint32_t maps, uint32_t ids, uint32_t per_sample,
                                float* d_maps, uint32_t* d_ids) {
    const uint64_t npix = (uint64_t)sc.sensor.width * sc.sensor.height;
    if (per_sample && samples >= 1u && samples <= 64u) {
        const uint64_t waves = (npix + 64u / samples - 1) / (64u / samples);
        const uint64_t blocks = (waves * 64u + kBlock - 1) / kBlock;
        hipLaunchKernelGGL(k_first_hit_wave<surface>, dim3((uint32_t)blocks), dim3(kBlock), 0, stream, sc, samples, seed, maps, ids, d_maps, d_ids);
    } else
        hipLaunchKernelGGL(k_first_hit<surface>, dim3((uint32_t)((npix + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, sc, samples, seed, maps, ids, d_maps,
                           d_ids);
}
int first_hit_launch(const scene_t& sc, hipStream_t stream, uint32_t samples, uint64_t seed, uint32_t maps, uint32_t ids, uint32_t per_sample, float* d_maps,
                     uint32_t* d_ids) {
    if ((uint64_t)sc.sensor.width * sc.sensor.height == 0) return 0;
    if (maps & kFhSurfaceMaps)
        first_hit_launch_as<true>(sc, stream, samples, seed, maps, ids, per_sample, d_maps, d_ids);
    else
        first_hit_launch_as<false>(sc, stream, samples, seed, maps, ids, per_sample, d_maps, d_ids);
    return (int)hipGetLastError();
}

// The same on host threads, one task per row, with a stack of the device's size (kLdsStack + kSpillStack entries: a full stack drops the same
// children on both), as sensor_mask_host.
void first_hit_host(const scene_t& sc, uint32_t samples, uint64_t seed, uint32_t maps, uint32_t ids, uint32_t n_threads, float* out_maps, uint32_t* out_ids) {
    const uint32_t W = sc.sensor.width, H = sc.sensor.height;
    const size_t K = fh_map_floats(maps), Ki = fh_id_words(ids);
    const bool surface = (maps & kFhSurfaceMaps) != 0;
    on_threads(H, n_threads, [&](auto claim) {
        stack_entry_t entries[kLdsStack + kSpillStack];
        const stack_ref_t stack = make_stack_ref(entries, 1, kLdsStack + kSpillStack, kLdsStack + kSpillStack, nullptr);
        for (uint32_t y = (uint32_t)claim(); y < H; y = (uint32_t)claim())
            for (uint32_t x = 0; x < W; ++x) {
                const fh_sums_t a = surface ? fh_pixel<true>(sc, x, y, samples, seed, stack) : fh_pixel<false>(sc, x, y, samples, seed, stack);
                const size_t p = (size_t)y * W + x;
                fh_write(a, samples, maps, ids, out_maps + p * K, out_ids + p * Ki);
            }
    });
}

}   // namespace wtk
