// wave_tracer_amd — first-hit maps of a perspective sensor (wtgpu_first_hit / wtgpu_first_hit_host; see wtgpu_kernels.h for the list of kernel
// translation units): per pixel the mean, over the primary rays that hit, of depth, position, normals, uv and facing, the share of rays that
// hit, and the shape and triangle of the first ray that does.  The rays are the sensor mask's (kernels_mask.hip), the lane shapes are
// kernels_maps.h's and the arithmetic is wt/first_hit.h's, which the host twin below runs too: device and host agree bit for bit.  No render
// kernel is compiled here.
#include "kernels_maps.h"
#include "wt/first_hit.h"

namespace wtk {

// One lane per pixel (the ray through the centre, more than 64 samples, WTGPU_FIRST_HIT_PER_SAMPLE=0): the lane keeps the sums in registers, then
// writes its K floats and Ki ids contiguously.  surface: any of the maps that need make_surface is asked for (depth / position / coverage /
// id queries load no tri_shade record and build no frame).
template <bool surface>
__global__ void __launch_bounds__(kBlock) k_first_hit(scene_t sc, uint32_t samples, uint64_t seed, uint32_t maps, uint32_t ids, float* out_maps,
                                                      uint32_t* out_ids) {
    __shared__ stack_entry_t lds[kLdsStack * kBlock];
    const uint32_t W = sc.sensor.width;
    on_lane_element(lds, W * sc.sensor.height, [&](uint32_t p, const stack_ref_t& stack) {
        const fh_sums_t a = fh_pixel<surface>(sc, p % W, p / W, samples, seed, stack);
        fh_write(a, samples, maps, ids, out_maps + (size_t)p * fh_map_floats(maps), out_ids + (size_t)p * fh_id_words(ids));
    });
}

// One lane per sample (1 <= samples <= 64).  Each hitting lane leaves its sample's floats and ids in the exchange, and lane j of a pixel's group —
// lanes j, j + samples, ... where a group is narrower than the floats — adds float j of the group's hitting samples and stores the mean:
// neighbouring lanes store neighbouring floats.  Every lane reaches the ballot and the barriers.
constexpr uint32_t kFhExchange = kFhFloats + 2;   // words per lane in the exchange: the sample's floats, its shape and its triangle
template <bool surface>
__global__ void __launch_bounds__(kBlock) k_first_hit_wave(scene_t sc, uint32_t samples, uint64_t seed, uint32_t maps, uint32_t ids, float* out_maps,
                                                           uint32_t* out_ids) {
    __shared__ stack_entry_t lds[kLdsStack * kBlock];
    exchange_fits<kFhExchange>();
    const uint32_t W = sc.sensor.width;
    const sample_lane_t l = sample_lane(samples, W * sc.sensor.height);
    fh_sample_t r;
    bool hit = false;
    if (l.active) {
        stack_entry_t spill[kSpillStack];
        stack_ref_t stack;
        lds_stack(lds, spill, stack);
        hit = fh_sample<surface>(sc, (uint32_t)(l.p % W), (uint32_t)(l.p / W), samples, l.s, seed, stack, r);
    }
    const unsigned long long bits = __ballot(hit);
    __syncthreads();   // no lane of the block reads its stack any more
    float* ex = reinterpret_cast<float*>(lds);
    uint32_t* exu = reinterpret_cast<uint32_t*>(lds);
    if (hit) {
#pragma unroll
        for (uint32_t j = 1; j < kFhFloats; ++j) ex[exchange_at(j, threadIdx.x)] = r.v[j];
        exu[exchange_at(kFhFloats, threadIdx.x)] = r.shape;
        exu[exchange_at(kFhFloats + 1, threadIdx.x)] = r.tri;
    }
    __syncthreads();
    if (!l.active) return;
    const unsigned long long mine = group_bits(bits, l, samples);
    const uint32_t n_hit = (uint32_t)__popcll(mine);
    float* m = out_maps + (size_t)l.p * fh_map_floats(maps);
    for (uint32_t j = l.s; j < kFhFloats; j += samples) {
        const int slot = fh_slot(maps, j);
        if (slot >= 0) m[slot] = fh_mean(j, j ? group_sum(ex, j, l, samples, mine) : 0.f, n_hit, samples);
    }
    if (l.s == 0 && ids) {
        uint32_t* id = out_ids + (size_t)l.p * fh_id_words(ids);
        if (ids & FH_SHAPE) *id++ = group_first_word(exu, kFhFloats, l, mine);
        if (ids & FH_TRIANGLE) *id++ = group_first_word(exu, kFhFloats + 1, l, mine);
    }
}

// per_sample (WTGPU_FIRST_HIT_PER_SAMPLE): one lane per sample wherever a pixel's samples fit one wavefront; else, and for the ray through the
// centre, one lane per pixel
template <bool surface>
static void first_hit_launch_as(const scene_t& sc, hipStream_t stream, uint32_t samples, uint64_t seed, uint32_t maps, uint32_t ids, uint32_t per_sample,
                                float* d_maps, uint32_t* d_ids) {
    const uint64_t npix = (uint64_t)sc.sensor.width * sc.sensor.height;
    if (per_sample && samples >= 1u && samples <= 64u)
        hipLaunchKernelGGL(k_first_hit_wave<surface>, dim3(sample_blocks(npix, samples)), dim3(kBlock), 0, stream, sc, samples, seed, maps, ids, d_maps, d_ids);
    else
        hipLaunchKernelGGL(k_first_hit<surface>, dim3(lane_blocks(npix)), dim3(kBlock), 0, stream, sc, samples, seed, maps, ids, d_maps, d_ids);
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

// The same on host threads (kernels_maps.h: on_elements).
void first_hit_host(const scene_t& sc, uint32_t samples, uint64_t seed, uint32_t maps, uint32_t ids, uint32_t n_threads, float* out_maps, uint32_t* out_ids) {
    const size_t K = fh_map_floats(maps), Ki = fh_id_words(ids);
    const bool surface = (maps & kFhSurfaceMaps) != 0;
    on_elements(sc, n_threads, [&](uint32_t x, uint32_t y, size_t p, const stack_ref_t& stack) {
        const fh_sums_t a = surface ? fh_pixel<true>(sc, x, y, samples, seed, stack) : fh_pixel<false>(sc, x, y, samples, seed, stack);
        fh_write(a, samples, maps, ids, out_maps + p * K, out_ids + p * Ki);
    });
}

}   // namespace wtk
