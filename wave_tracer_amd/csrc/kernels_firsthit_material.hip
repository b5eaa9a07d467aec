// wave_tracer_amd — first-hit material maps of a perspective sensor (wtgpu_first_hit_material / wtgpu_first_hit_material_host; see wtgpu_kernels.h
// for the list of kernel translation units): per pixel and requested wavenumber the mean, over the primary rays that hit, of the diffuse albedo,
// the specular reflectance of the smooth interface, the mask opacity, the roughness and the emitted radiance of what the ray meets, and the
// material index and leaf type of the first ray that hits.  The rays are kernels_firsthit.hip's, the lane shapes are kernels_maps.h's and the
// arithmetic is wt/first_hit_material.h's, which the host twin below runs too: device and host agree bit for bit.  No render kernel is compiled here.
#include "kernels_maps.h"
#include "wt/first_hit_material.h"

namespace wtk {

// One lane per pixel (the ray through the centre, more than 64 samples, WTGPU_FIRST_HIT_PER_SAMPLE=0): the lane keeps the sums in registers, then
// writes its K floats and Ki ids contiguously.  specular: the SPECULAR map is asked for (the other queries compile no Fresnel code).
template <bool specular>
__global__ void __launch_bounds__(kBlock) k_first_hit_material(scene_t sc, fhm_query_t q, float* out_maps, uint32_t* out_ids) {
    __shared__ stack_entry_t lds[kLdsStack * kBlock];
    const uint32_t W = sc.sensor.width;
    on_lane_element(lds, W * sc.sensor.height, [&](uint32_t p, const stack_ref_t& stack) {
        const fhm_sums_t a = fhm_pixel<specular>(sc, q, p % W, p / W, stack);
        fhm_write(a, q, out_maps + (size_t)p * fhm_map_floats(q.maps, q.n_k), out_ids + (size_t)p * fhm_id_words(q.ids));
    });
}

// One lane per sample (1 <= samples <= 64).  Each hitting lane leaves its sample's requested floats in the exchange in the order of the output
// (float `slot`) and its two ids behind them, and lane j of a pixel's group — lanes j, j + samples, ... where a group is narrower than the floats
// — adds float j of the group's hitting samples and stores the mean: neighbouring lanes store neighbouring floats.  The full query, 5 maps x 4
// wavenumbers + 2 ids = 22 words per lane, fits the stacks' LDS (kLdsStack entries of 8 bytes: 40 words at the default 20) in ONE round; a build
// with fewer than 11 entries is refused.  Every lane reaches the ballot and the barriers.
constexpr uint32_t kFhmExchange = kFhmFloats + 2;   // words per lane in the exchange: the sample's floats, its material and its leaf type
template <bool specular>
__global__ void __launch_bounds__(kBlock) k_first_hit_material_wave(scene_t sc, fhm_query_t q, float* out_maps, uint32_t* out_ids) {
    __shared__ stack_entry_t lds[kLdsStack * kBlock];
    exchange_fits<kFhmExchange>();
    const uint32_t W = sc.sensor.width, samples = q.samples;
    const sample_lane_t l = sample_lane(samples, W * sc.sensor.height);
    fhm_sample_t r;
    bool hit = false;
    if (l.active) {
        stack_entry_t spill[kSpillStack];
        stack_ref_t stack;
        lds_stack(lds, spill, stack);
        hit = fhm_sample<specular>(sc, q, (uint32_t)(l.p % W), (uint32_t)(l.p / W), l.s, stack, r);
    }
    const unsigned long long bits = __ballot(hit);
    __syncthreads();   // no lane of the block reads its stack any more
    float* ex = reinterpret_cast<float*>(lds);
    uint32_t* exu = reinterpret_cast<uint32_t*>(lds);
    if (hit) {
#pragma unroll
        for (uint32_t i = 0; i < kFhmMaps; ++i)
#pragma unroll
            for (uint32_t j = 0; j < kFhmMaxK; ++j)
                if (((q.maps >> i) & 1u) && j < q.n_k) ex[exchange_at(fhm_slot(q.maps, q.n_k, i, j), threadIdx.x)] = r.v[i * kFhmMaxK + j];
        exu[exchange_at(kFhmFloats, threadIdx.x)] = r.material;
        exu[exchange_at(kFhmFloats + 1, threadIdx.x)] = r.type;
    }
    __syncthreads();
    if (!l.active) return;
    const unsigned long long mine = group_bits(bits, l, samples);
    const uint32_t n_hit = (uint32_t)__popcll(mine), K = fhm_map_floats(q.maps, q.n_k);
    float* m = out_maps + (size_t)l.p * K;
    for (uint32_t slot = l.s; slot < K; slot += samples) m[slot] = fh_hit_mean(group_sum(ex, slot, l, samples, mine), n_hit);
    if (l.s == 0 && q.ids) {
        uint32_t* id = out_ids + (size_t)l.p * fhm_id_words(q.ids);
        if (q.ids & FHM_MATERIAL) *id++ = group_first_word(exu, kFhmFloats, l, mine);
        if (q.ids & FHM_TYPE) *id++ = group_first_word(exu, kFhmFloats + 1, l, mine);
    }
}

// per_sample (WTGPU_FIRST_HIT_PER_SAMPLE): one lane per sample wherever a pixel's samples fit one wavefront; else, and for the ray through the
// centre, one lane per pixel
template <bool specular>
static void first_hit_material_launch_as(const scene_t& sc, hipStream_t stream, const fhm_query_t& q, uint32_t per_sample, float* d_maps, uint32_t* d_ids) {
    const uint64_t npix = (uint64_t)sc.sensor.width * sc.sensor.height;
    if (per_sample && q.samples >= 1u && q.samples <= 64u)
        hipLaunchKernelGGL(k_first_hit_material_wave<specular>, dim3(sample_blocks(npix, q.samples)), dim3(kBlock), 0, stream, sc, q, d_maps, d_ids);
    else
        hipLaunchKernelGGL(k_first_hit_material<specular>, dim3(lane_blocks(npix)), dim3(kBlock), 0, stream, sc, q, d_maps, d_ids);
}
int first_hit_material_launch(const scene_t& sc, hipStream_t stream, const fhm_query_t& q, uint32_t per_sample, float* d_maps, uint32_t* d_ids) {
    if ((uint64_t)sc.sensor.width * sc.sensor.height == 0) return 0;
    if (q.maps & FHM_SPECULAR)
        first_hit_material_launch_as<true>(sc, stream, q, per_sample, d_maps, d_ids);
    else
        first_hit_material_launch_as<false>(sc, stream, q, per_sample, d_maps, d_ids);
    return (int)hipGetLastError();
}

// The same on host threads (kernels_maps.h: on_elements).
void first_hit_material_host(const scene_t& sc, const fhm_query_t& q, uint32_t n_threads, float* out_maps, uint32_t* out_ids) {
    const size_t K = fhm_map_floats(q.maps, q.n_k), Ki = fhm_id_words(q.ids);
    const bool specular = (q.maps & FHM_SPECULAR) != 0;
    on_elements(sc, n_threads, [&](uint32_t x, uint32_t y, size_t p, const stack_ref_t& stack) {
        const fhm_sums_t a = specular ? fhm_pixel<true>(sc, q, x, y, stack) : fhm_pixel<false>(sc, q, x, y, stack);
        fhm_write(a, q, out_maps + p * K, out_ids + p * Ki);
    });
}

}   // namespace wtk
