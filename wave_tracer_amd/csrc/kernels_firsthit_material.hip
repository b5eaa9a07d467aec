// wave_tracer_amd — first-hit material maps of a perspective sensor (wtgpu_first_hit_material / wtgpu_first_hit_material_host; see wtgpu_kernels.h
// for the list of kernel translation units): per pixel and requested wavenumber the mean, over the primary rays that hit, of the diffuse albedo,
// the specular reflectance of the smooth interface, the mask opacity, the roughness and the emitted radiance of what the ray meets, and the
// material index and leaf type of the first ray that hits.  The rays are kernels_firsthit.hip's and the arithmetic is wt/first_hit_material.h's,
// which the host twin below runs too: device and host agree bit for bit.  No render kernel is compiled here.
#include "kernels_film.h"   // (on_threads)
#include "wt/first_hit_material.h"

namespace wtk {

// One lane per pixel, as k_first_hit (the ray through the centre, more than 64 samples, WTGPU_FIRST_HIT_PER_SAMPLE=0): the lane traces the pixel's
// samples one after the other and keeps the sums in registers, then writes its K floats and Ki ids contiguously.  specular: the SPECULAR map is
// asked for (the other queries compile no Fresnel code).
template <bool specular>
__global__ void __launch_bounds__(kBlock) k_first_hit_material(scene_t sc, fhm_query_t q, float* out_maps, uint32_t* out_ids) {
    __shared__ stack_entry_t lds[kLdsStack * kBlock];
    const uint32_t W = sc.sensor.width, npix = W * sc.sensor.height;
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= npix) return;
    stack_entry_t spill[kSpillStack];
    stack_ref_t stack;
    lds_stack(lds, spill, stack);
    const fhm_sums_t a = fhm_pixel<specular>(sc, q, p % W, p / W, stack);
    fhm_write(a, q, out_maps + (size_t)p * fhm_map_floats(q.maps, q.n_k), out_ids + (size_t)p * fhm_id_words(q.ids));
}

// One lane per sample (1 <= samples <= 64), as k_first_hit_wave: a wavefront holds 64 / samples pixels, lanes [g * samples, (g + 1) * samples)
// the samples of its g-th.  When every lane of the block has finished its ray the LDS of the stacks is free: each hitting lane leaves its
// sample's requested floats there in the order of the output (float `slot` of thread t at [slot * kBlock + t]) and its two ids behind them, and
// lane j of a pixel's group — lanes j, j + samples, ... where a group is narrower than the floats — adds float j of the group's hitting samples
// in sample order, first term first, and stores the mean: the sums are the ones one thread would form, and neighbouring lanes store neighbouring
// floats.  The full query, 5 maps x 4 wavenumbers + 2 ids = 22 words per lane, fits the stacks' LDS (kLdsStack entries of 8 bytes: 40 words at
// the default 20) in ONE round; a build with fewer than 11 entries is refused below.  Every lane reaches the ballot and the barriers.
constexpr uint32_t kFhmExchange = kFhmFloats + 2;   // words per lane in the exchange: the sample's floats, its material and its leaf type
static_assert(kFhmExchange * sizeof(float) <= kLdsStack * sizeof(stack_entry_t), "the exchange of the per-sample form must fit the LDS of the stacks");
template <bool specular>
__global__ void __launch_bounds__(kBlock) k_first_hit_material_wave(scene_t sc, fhm_query_t q, float* out_maps, uint32_t* out_ids) {
    __shared__ stack_entry_t lds[kLdsStack * kBlock];
    const uint32_t W = sc.sensor.width, npix = W * sc.sensor.height;
    const uint32_t samples = q.samples, per_wave = 64u / samples;
    const uint32_t lane = threadIdx.x & 63u, g = lane / samples, s = lane - g * samples;
    const uint64_t p = ((blockIdx.x * (uint64_t)kBlock + threadIdx.x) >> 6) * per_wave + g;
    const bool active = g < per_wave && p < npix;
    fhm_sample_t r;
    bool hit = false;
    if (active) {
        stack_entry_t spill[kSpillStack];
        stack_ref_t stack;
        lds_stack(lds, spill, stack);
        hit = fhm_sample<specular>(sc, q, (uint32_t)(p % W), (uint32_t)(p / W), s, stack, r);
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
                if (((q.maps >> i) & 1u) && j < q.n_k) ex[fhm_slot(q.maps, q.n_k, i, j) * kBlock + threadIdx.x] = r.v[i * kFhmMaxK + j];
        exu[kFhmFloats * kBlock + threadIdx.x] = r.material;
        exu[(kFhmFloats + 1) * kBlock + threadIdx.x] = r.type;
    }
    __syncthreads();
    if (!active) return;
    const unsigned long long mine = samples == 64u ? bits : (bits >> (g * samples)) & ((1ull << samples) - 1ull);
    const uint32_t n_hit = (uint32_t)__popcll(mine), first_lane = threadIdx.x - s;   // (the group's first thread)
    const uint32_t K = fhm_map_floats(q.maps, q.n_k);
    float* m = out_maps + (size_t)p * K;
    for (uint32_t slot = s; slot < K; slot += samples) {
        float sum = 0.f;
        bool first = true;
        for (uint32_t t = 0; t < samples; ++t)
            if ((mine >> t) & 1ull) {
                sum = fh_add(first, sum, ex[slot * kBlock + first_lane + t]);
                first = false;
            }
        m[slot] = fhm_mean(sum, n_hit);
    }
    if (s == 0 && q.ids) {
        const uint32_t t = n_hit ? first_lane + (uint32_t)__ffsll((long long)mine) - 1u : 0u;
        uint32_t* id = out_ids + (size_t)p * fhm_id_words(q.ids);
        if (q.ids & FHM_MATERIAL) *id++ = n_hit ? exu[kFhmFloats * kBlock + t] : 0xFFFFFFFFu;
        if (q.ids & FHM_TYPE) *id++ = n_hit ? exu[(kFhmFloats + 1) * kBlock + t] : 0xFFFFFFFFu;
    }
}

// per_sample (WTGPU_FIRST_HIT_PER_SAMPLE): one lane per sample wherever a pixel's samples fit one wavefront; else, and for the ray through the
// centre, one lane per pixel
template <bool specular>
static void first_hit_material_launch_as(const scene_t& sc, hipStream_t stream, const fhm_query_t& q, uint32_t per_sample, float* d_maps, uint32_t* d_ids) {
    const uint64_t npix = (uint64_t)sc.sensor.width * sc.sensor.height;
    if (per_sample && q.samples >= 1u && q.samples <= 64u) {
        const uint64_t waves = (npix + 64u / q.samples - 1) / (64u / q.samples);
        const uint64_t blocks = (waves * 64u + kBlock - 1) / kBlock;
        hipLaunchKernelGGL(k_first_hit_material_wave<specular>, dim3((uint32_t)blocks), dim3(kBlock), 0, stream, sc, q, d_maps, d_ids);
    } else
        hipLaunchKernelGGL(k_first_hit_material<specular>, dim3((uint32_t)((npix + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, sc, q, d_maps, d_ids);
}
int first_hit_material_launch(const scene_t& sc, hipStream_t stream, const fhm_query_t& q, uint32_t per_sample, float* d_maps, uint32_t* d_ids) {
    if ((uint64_t)sc.sensor.width * sc.sensor.height == 0) return 0;
    if (q.maps & FHM_SPECULAR)
        first_hit_material_launch_as<true>(sc, stream, q, per_sample, d_maps, d_ids);
    else
        first_hit_material_launch_as<false>(sc, stream, q, per_sample, d_maps, d_ids);
    return (int)hipGetLastError();
}

// The same on host threads, one task per row, with a stack of the device's size (kLdsStack + kSpillStack entries: a full stack drops the same
// children on both), as first_hit_host.
void first_hit_material_host(const scene_t& sc, const fhm_query_t& q, uint32_t n_threads, float* out_maps, uint32_t* out_ids) {
    const uint32_t W = sc.sensor.width, H = sc.sensor.height;
    const size_t K = fhm_map_floats(q.maps, q.n_k), Ki = fhm_id_words(q.ids);
    const bool specular = (q.maps & FHM_SPECULAR) != 0;
    on_threads(H, n_threads, [&](auto claim) {
        stack_entry_t entries[kLdsStack + kSpillStack];
        const stack_ref_t stack = make_stack_ref(entries, 1, kLdsStack + kSpillStack, kLdsStack + kSpillStack, nullptr);
        for (uint32_t y = (uint32_t)claim(); y < H; y = (uint32_t)claim())
            for (uint32_t x = 0; x < W; ++x) {
                const fhm_sums_t a = specular ? fhm_pixel<true>(sc, q, x, y, stack) : fhm_pixel<false>(sc, q, x, y, stack);
                const size_t p = (size_t)y * W + x;
                fhm_write(a, q, out_maps + p * K, out_ids + p * Ki);
            }
    });
}

}   // namespace wtk
