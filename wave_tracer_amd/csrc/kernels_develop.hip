// wave_tracer_amd — film development and tonemapping on the device (see wtgpu_kernels.h for the list of kernel translation units): what the host
// did with three downloaded f64 accumulators (render_context_t::develop, src/scene/render.cpp:245-291; tonemap_t, src/sensor/response/tonemap.cpp)
// done where the films are.  k_develop writes the developed f32 film; k_develop_tonemap develops the planes of one Stokes component, applies the
// operator, the mode and the colour table, appends an optional mask as alpha and writes f32 / 8-bit / 16-bit pixels — the developed values
// never reach memory.  The arithmetic is wt/tonemap.h's, shared with the host twins at the end of the file.  Both kernels stream: every film
// byte is read once, and the time is the memory system's.  k_develop_tonemap is also compiled for a developed f32 film as its source (what k_develop
// or a denoiser wrote; wt/film_stats.h: film_src_t).  No render kernel is compiled here.
#include "kernels_film.h"

namespace wtk {

constexpr int kDevelopBlock = 256;
constexpr uint32_t kTableLdsEntries = kMaxTonemapTable;   // 12 KiB of LDS when the table is staged

// ---- k_develop: f64 films [H][W][P], [H][W] -> f32 [H][W][P] -------------------------------------------------------------------------------
// kPerPixel = false: one lane per PLANE element — lane i reads value[i], light[i] (consecutive lanes, consecutive 8-byte words: every load
// instruction covers 512 contiguous bytes) and weight[i / P] (P neighbours share a word), and writes out[i].
// kPerPixel = true: one lane per pixel, which walks its P planes (8 P contiguous bytes per lane; consecutive lanes are 8 P bytes apart).
template <uint32_t P, bool kPerPixel>
__global__ void __launch_bounds__(kDevelopBlock) k_develop(const double* __restrict__ value, const double* __restrict__ weight, const double* __restrict__ light,
                                                           double sl, uint64_t npix, float* __restrict__ out) {
    const uint64_t i = blockIdx.x * (uint64_t)kDevelopBlock + threadIdx.x;
    if (kPerPixel) {
        if (i >= npix) return;
        const double w = weight[i];
#pragma unroll
        for (uint32_t c = 0; c < P; ++c) out[i * P + c] = develop_plane(value[i * P + c], w, light[i * P + c], sl);
    } else {
        if (i >= npix * P) return;
        out[i] = develop_plane(value[i], weight[i / P], light[i], sl);
    }
}

// ---- k_develop_tonemap: the fused form, one lane per pixel ---------------------------------------------------------------------------------
// A pixel's C = 1 or 3 developed values (planes c * stokes + s) meet in one lane — the luminance, the table lookup and the pixel's single 4- to
// 16-byte store need them together — so the lane-per-plane mapping of k_develop has nothing to offer here.  kLdsTable: the block copies the
// colour table (at most kTableLdsEntries entries) to LDS first; otherwise the lanes read it through the caches.
// kDev (a developed film, in `value`; wt/film_stats.h: film_src): the same lane per pixel, its C floats by 4-byte loads `stokes` floats apart —
// contiguous across the wavefront for a monochromatic or RGB film (12 bytes a lane, which no 16-byte load fits); of a polarimetric film one
// component in four is wanted, and a vector load per lane would fetch the same lines for the same bytes.  No alignment is asked of the film.
template <bool kDev, uint32_t C, bool kLdsTable>
__global__ void __launch_bounds__(kDevelopBlock) k_develop_tonemap(const film_elem_t<kDev>* __restrict__ value, const double* __restrict__ weight,
                                                                   const double* __restrict__ light, double sl, uint32_t stokes, uint32_t s, tonemap_args_t t,
                                                                   const float* __restrict__ mask, uint32_t format, uint64_t npix, void* __restrict__ out) {
    __shared__ float lds_table[kLdsTable ? 3 * kTableLdsEntries : 1];
    if (kLdsTable && tm_uses_map(t.mode, C)) {
        for (uint32_t k = threadIdx.x; k < 3 * t.table_n; k += kDevelopBlock) lds_table[k] = t.table[k];
        __syncthreads();
        t.table = lds_table;
    }
    const uint64_t p = blockIdx.x * (uint64_t)kDevelopBlock + threadIdx.x;
    if (p >= npix) return;
    float v[C], rgb[3];
    fs_planes(film_src(value, weight, light, sl), p, C, stokes, s, false, 0u, v);
    tm_pixel(t, v, C, rgb);
    if (!mask) {
        tm_store(out, p, format, 3, rgb, 0.f);
        return;
    }
    // four components: one store per pixel (tm_store's bytes, little endian)
    const float a = mask[p];
    if (format == TM_F32)
        static_cast<float4*>(out)[p] = make_float4(rgb[0], rgb[1], rgb[2], a);
    else if (format == TM_U8)
        static_cast<uint32_t*>(out)[p] = tm_quantise(rgb[0], 255.f) | tm_quantise(rgb[1], 255.f) << 8 | tm_quantise(rgb[2], 255.f) << 16 | tm_quantise(a, 255.f) << 24;
    else
        static_cast<uint2*>(out)[p] = make_uint2(tm_quantise(rgb[0], 65535.f) | tm_quantise(rgb[1], 65535.f) << 16,
                                                 tm_quantise(rgb[2], 65535.f) | tm_quantise(a, 65535.f) << 16);
}

static uint32_t blocks_for(uint64_t n) { return (uint32_t)((n + kDevelopBlock - 1) / kDevelopBlock); }

template <uint32_t P>
static void develop_launch_p(hipStream_t stream, const double* v, const double* w, const double* l, double sl, uint64_t npix, bool per_pixel, float* out) {
    if (per_pixel)
        hipLaunchKernelGGL((k_develop<P, true>), dim3(blocks_for(npix)), dim3(kDevelopBlock), 0, stream, v, w, l, sl, npix, out);
    else
        hipLaunchKernelGGL((k_develop<P, false>), dim3(blocks_for(npix * P)), dim3(kDevelopBlock), 0, stream, v, w, l, sl, npix, out);
}
int develop_launch(const sensor_t& sn, hipStream_t stream, const double* d_value, const double* d_weight, const double* d_light, uint64_t spe,
                   uint32_t per_pixel, float* d_out) {
    const uint64_t npix = (uint64_t)sn.width * sn.height;
    if (npix == 0) return 0;
    const double sl = develop_scale(spe);
    // One lane per plane element unless the knob says otherwise.  On the MI355X (tools/bench_develop.py: median of 15 launches each, alternated,
    // device events): the polarimetric room film (1920 x 1088, P = 12; 426 MB read, 100 MB written) 0.102 - 0.104 ms against 0.132 - 0.134 ms with one
    // lane per pixel, whose lanes sit 96 bytes apart; the cornell film (1440 x 1440, P = 3) 0.031 - 0.033 against 0.029 - 0.030 ms (two runs).
    switch (film_planes(sn)) {
    case 1: develop_launch_p<1>(stream, d_value, d_weight, d_light, sl, npix, per_pixel != 0, d_out); break;
    case 3: develop_launch_p<3>(stream, d_value, d_weight, d_light, sl, npix, per_pixel != 0, d_out); break;
    case 4: develop_launch_p<4>(stream, d_value, d_weight, d_light, sl, npix, per_pixel != 0, d_out); break;
    case 12: develop_launch_p<12>(stream, d_value, d_weight, d_light, sl, npix, per_pixel != 0, d_out); break;
    default: return (int)hipErrorInvalidValue;   // (film_planes: 1 or 3 channels x 1 or 4 Stokes components)
    }
    return (int)hipGetLastError();
}

template <bool kDev, uint32_t C>
static void tonemap_launch_c(hipStream_t stream, const film_elem_t<kDev>* v, const double* w, const double* l, double sl, uint32_t stokes, uint32_t s, const tonemap_args_t& t,
                             const float* mask, uint32_t format, bool lds_table, uint64_t npix, void* out) {
    if (lds_table)
        hipLaunchKernelGGL((k_develop_tonemap<kDev, C, true>), dim3(blocks_for(npix)), dim3(kDevelopBlock), 0, stream, v, w, l, sl, stokes, s, t, mask, format, npix, out);
    else
        hipLaunchKernelGGL((k_develop_tonemap<kDev, C, false>), dim3(blocks_for(npix)), dim3(kDevelopBlock), 0, stream, v, w, l, sl, stokes, s, t, mask, format, npix, out);
}
int develop_tonemap_launch(const sensor_t& sn, hipStream_t stream, const wtgpu_film_source& film, const tonemap_args_t& t, uint32_t s, const float* d_mask, uint32_t format, uint32_t lds_table, void* d_out) {
    const uint64_t npix = (uint64_t)sn.width * sn.height;
    if (npix == 0) return 0;
    const uint32_t stokes = film_stokes(sn);
    const bool lds = lds_table != 0 && t.table_n <= kTableLdsEntries;
    // The table is read through the caches unless the knob says otherwise: with every pixel going through a 256-entry table (colourmap mode,
    // 8-bit RGBA out; same tool, same method) 0.043 - 0.044 ms against 0.044 - 0.045 ms with the table staged in LDS on the cornell film, 0.101 - 0.108
    // against 0.100 - 0.108 ms on the room film (two runs) — no difference to be had, so the block does not spend a barrier and 3 KB of copies on
    // it.  To RGBA8 in normal mode the kernel takes 0.040 ms on the cornell film and 0.086 ms on the room film back to back, 0.042 and 0.28 - 0.30 ms
    // when the GPU has idled for 100 ms before the launch.
    if (!film_dispatch(sn.channels, false, [&](auto c, auto) {
            film_source_dispatch(film, [&](auto src) {
                tonemap_launch_c<decltype(src)::developed, decltype(c)::value>(stream, src.first(), src.weight, src.light, src.sl, stokes, s, t, d_mask, format, lds, npix, d_out);
            });
        }))
        return (int)hipErrorInvalidValue;
    return (int)hipGetLastError();
}

// ---- the host twin: the same wt/tonemap.h functions on host threads, one task per row -------------------------------------------------------
template <class Src>
static void develop_tonemap_host_of(const sensor_t& sn, const Src& film, const tonemap_args_t& t, uint32_t s, const float* mask, uint32_t format, uint32_t n_threads, void* out) {
    const uint32_t W = sn.width, H = sn.height, C = sn.channels, stokes = film_stokes(sn);
    on_threads(H, n_threads, [&](auto claim) {
        for (uint64_t y = claim(); y < H; y = claim())
            for (uint32_t x = 0; x < W; ++x) {
                const size_t p = (size_t)y * W + x;
                float v[3] = {0.f, 0.f, 0.f}, rgb[3];
                fs_planes(film, p, C, stokes, s, false, 0u, v);
                tm_pixel(t, v, C, rgb);
                tm_store(out, p, format, mask ? 4u : 3u, rgb, mask ? mask[p] : 0.f);
            }
    });
}
void develop_tonemap_host(const sensor_t& sn, const wtgpu_film_source& film, const tonemap_args_t& t, uint32_t s, const float* mask, uint32_t format, uint32_t n_threads,
                          void* out) {
    film_source_dispatch(film, [&](auto src) { develop_tonemap_host_of(sn, src, t, s, mask, format, n_threads, out); });
}

}   // namespace wtk
