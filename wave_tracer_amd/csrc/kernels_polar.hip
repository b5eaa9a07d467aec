// wave_tracer_amd — the polarisation view of a Stokes film on the device (see wtgpu_kernels.h for the list of kernel translation units): what
// a user of a polarimetric film had to download twelve planes of three f64 accumulators for.  k_film_polar reads the films once, develops in
// registers (the developed values never reach memory), and gives per plane — each channel, and the luminance's Stokes vector where asked for —
// the chunk sums of the six Stokes sums in the fixed order of wt/film_stats.h, one record per wavefront with its counts and its largest degree
// of polarisation, the maps asked for and the false-colour picture of one plane; kernels_film.h's k_film_finish reduces the chunk sums level
// after level and merges the wavefronts' records.  No atomics: every field is the same whatever the schedule.  The arithmetic is
// wt/film_polar.h's, shared with the host twin at the end of the file, and calls no libm function: every count, the maximum and its pixel, the
// six sums and the maps — the two angles among them — are the same on both sides, bit for bit.  The same kernel is compiled for a developed f32
// film as its source (wt/film_stats.h: film_src_t), with loaders of its own.  No render kernel is compiled here.
#include "kernels_film.h"
#include "wt/film_polar.h"

namespace wtk {

// a pixel's maps of one plane, the chosen ones in the order of their bits; 0 for a pixel the mask excludes
WT_HD void fp_store_maps(float* maps, uint64_t pixel, uint32_t plane, uint32_t planes, const film_polar_args_t& a, const fp_plane_t& r, bool included) {
    float* o = maps + (pixel * planes + plane) * a.n_maps;
    uint32_t k = 0;
#pragma unroll
    for (uint32_t m = 0; m < kFpMaps; ++m)
        if (a.maps >> m & 1u) o[k++] = included ? r.map[m] : 0.f;
}

// ---- k_film_polar: f64 films [H][W][C x 4], [H][W] (or a developed f32 film [H][W][C x 4]) -> chunk sums, wavefront records, maps, picture ---------------------------------------------
// One lane per pixel, in the chunk geometry of kernels_film.h.  The loads are unconditional (a pixel past the film's end re-reads the last one)
// so that all of a chunk's are in flight together; `included` gates what they give.  A chunk's developed Stokes components stay in registers as
// f32 (4 C per pixel) while ONE plane at a time has its twenty-four f64 addends live.  Counts and the largest degree of polarisation are
// per-lane registers over all the wavefront's chunks, reduced once at its end.
// kStaged = false: a lane loads the 4 C planes of its own pixels (8-byte loads, consecutive lanes 32 C bytes apart); all hundred loads of an RGB
// chunk are in flight at once, at 282 - 314 VGPRs: one wavefront per SIMD.
// kStaged = true (the default: film_polar_launch has the measurement): the wavefront reads its chunk's 256 x 4 C plane elements as k_develop does — lane i element i of every 64, each load instruction
// 512 contiguous bytes — develops them there and leaves the f32 in its own 1024 C floats of LDS, from which the pixels' lanes take one plane's
// Stokes vector at a time (16-byte reads); nothing of it is shared between wavefronts, so there is no barrier.
// kDev (a developed film, in `value`; wt/film_stats.h: film_src), where a pixel's 4 C floats are 16 C contiguous bytes and all of them are wanted:
// kStaged = false: a lane takes its own pixel's floats, which the compiler gathers into C 16-byte loads (consecutive lanes 16 C bytes apart: an
// RGB wavefront's three load instructions cover the same 3072 contiguous bytes between them);
// kStaged = true: lane i takes FOUR consecutive elements, 4 i .. 4 i + 3 of every 256, with one 16-byte load (film_dev_t::element4) and leaves
// them in LDS with one 16-byte write — each load instruction 1024 contiguous bytes, 4 C of them for a chunk, where one element per lane would
// be 16 C instructions of 256 bytes.  The loads ask no alignment beyond a float's (the device reads a 16-byte vector at any 4-byte address).
template <bool kDev, uint32_t C, bool kLum, bool kStaged>
__global__ void __launch_bounds__(kFilmBlock) k_film_polar(const film_elem_t<kDev>* __restrict__ value, const double* __restrict__ weight, const double* __restrict__ light, double sl,
                                                           film_polar_args_t a, const float* __restrict__ mask, uint64_t npix, double* __restrict__ sums,
                                                           uint64_t sums_stride, film_wave_rec_t* __restrict__ wrec, float* __restrict__ maps, void* __restrict__ picture) {
    constexpr uint32_t NP = C + (kLum ? 1u : 0u), P = C * 4u;
    __shared__ __attribute__((aligned(16))) float lds_x[kStaged ? kFilmWaves * kFsChunk * P : 4];
    float* const xs = lds_x + (kStaged ? (threadIdx.x >> 6) * kFsChunk * P : 0u);   // the wavefront's own part
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t n_chunks = fs_chunks(npix), n_waves = film_waves(), wave = film_first_chunk();
    const film_src_t<kDev> film = film_src(value, weight, light, sl);
    fc_best_t best[NP];
    uint32_t n_nonfinite[NP], n_dark[NP], n_over[NP], n_included = 0;
#pragma unroll
    for (uint32_t c = 0; c < NP; ++c) n_nonfinite[c] = n_dark[c] = n_over[c] = 0u;
    for (uint64_t chunk = wave; chunk < n_chunks; chunk += n_waves) {
        float x[4][kStaged ? 1 : P], alpha[4];
        bool included[4];
        if (kStaged) {
            if constexpr (kDev) {
                const uint64_t first = chunk * (kFsChunk * P / 4u), n_quads = npix * (P / 4u);   // (P = 4 C: a film is whole quads)
#pragma unroll
                for (uint32_t i = 0; i < P; ++i) {
                    const uint64_t e = first + i * 64u + lane, q = e < n_quads ? e : n_quads - 1;
                    reinterpret_cast<film_quad_aligned_t*>(xs)[i * 64u + lane] = film.element4(q);
                }
            } else {
                const uint64_t first = chunk * kFsChunk * P, n_elements = npix * P;
#pragma unroll 8
                for (uint32_t i = 0; i < 4u * P; ++i) {
                    const uint64_t e = first + i * 64u + lane, q = e < n_elements ? e : n_elements - 1;
                    xs[i * 64u + lane] = film.element_of(q, P);
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint64_t p = chunk_element(chunk, j), q = p < npix ? p : npix - 1;
            alpha[j] = mask ? mask[q] : 0.f;
            included[j] = p < npix && (!mask || alpha[j] > 0.f);
            if (!kStaged) {
                const double w = film.pixel_word(q);
#pragma unroll
                for (uint32_t k = 0; k < (kStaged ? 1u : P); ++k) x[j][k] = film.element(q * P + k, w);
            }
            n_included += included[j] ? 1u : 0u;
        }
#pragma unroll
        for (uint32_t c = 0; c < NP; ++c) {
            double t[kFpSums][4];
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                const uint64_t p = chunk_element(chunk, j);
                double S[4];
                fp_stokes(kStaged ? xs + (j * 64u + lane) * P : x[j], c, C, S);
                const fp_plane_t r = fp_plane(S[0], S[1], S[2], S[3], included[j], a.c2, a.s2);
                n_nonfinite[c] += r.nonfinite;
                n_dark[c] += r.dark;
                n_over[c] += r.over;
                fp_best_take(best[c], r, p);
#pragma unroll
                for (uint32_t k = 0; k < kFpSums; ++k) t[k][j] = r.add[k];
                if (p < npix) {
                    if (maps) fp_store_maps(maps, p, c, NP, a, r, included[j]);
                    if (picture && c == a.picture_plane) {
                        float rgb[3];
                        fp_colour(a, (float)S[0], r, rgb);
                        tm_store(picture, p, a.format, mask ? 4u : 3u, rgb, alpha[j]);
                    }
                }
            }
#pragma unroll
            for (uint32_t k = 0; k < kFpSums; ++k) film_store_chunk_sum(sums + (c * kFpSums + k) * sums_stride + chunk, t[k]);
        }
        if (kStaged) {   // the next chunk's elements go where this one's were read
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
    }
    film_store_wave_recs(wrec, n_waves, wave, n_included, n_nonfinite, n_dark, n_over, best);
}

int film_polar_launch(const sensor_t& sn, hipStream_t stream, uint32_t n_cus, const wtgpu_film_source& film, uint32_t flags, const film_polar_args_t& a, uint32_t staged, const float* d_mask, void* d_rec, double* d_sums, void* d_wave, float* d_maps,
                      void* d_picture) {
    const uint64_t npix = (uint64_t)sn.width * sn.height;
    if (npix == 0 || film_stokes(sn) != 4) return (int)hipErrorInvalidValue;
    const bool lum = (flags & FP_LUMINANCE) != 0;
    const uint64_t stride = fs_scratch_len(npix);
    const uint32_t blocks = film_rec_blocks(npix, n_cus);
    film_wave_rec_t* wrec = static_cast<film_wave_rec_t*>(d_wave);
    // The staged form unless the knob says otherwise.  On the MI355X (tools/bench_film_polar.py, profiles/film_polar_bench.json: the polarimetric room
    // film, 1920 x 1088, P = 12, 418 MB read; median of 15 calls each, alternated, between device events, the finish kernel and the copy of the
    // records included): records alone 0.220 ms staged against 0.279 ms with every lane loading its own pixels (0.207 against 0.286 in an earlier
    // run); with the luminance's plane and all six maps (201 MB written) 0.430 against 0.447 ms.  k_develop reads the same film in 0.102 ms.
    // From a developed film of the same size (100 MB read; tools/bench_film_developed.py, profiles/film_developed_bench.json, same method): records
    // with the luminance's plane 0.194 ms staged against 0.263 ms per lane (the accumulators in that run: 0.246 against 0.351), so one knob serves both.
    if (!film_dispatch(sn.channels, lum, [&](auto c, auto l) {
            film_source_dispatch(film, [&](auto src) {
                constexpr bool kDev = decltype(src)::developed;
                if (staged)
                    hipLaunchKernelGGL((k_film_polar<kDev, decltype(c)::value, decltype(l)::value, true>), dim3(blocks), dim3(kFilmBlock), 0, stream, src.first(), src.weight, src.light,
                                       src.sl, a, d_mask, npix, d_sums, stride, wrec, d_maps, d_picture);
                else
                    hipLaunchKernelGGL((k_film_polar<kDev, decltype(c)::value, decltype(l)::value, false>), dim3(blocks), dim3(kFilmBlock), 0, stream, src.first(), src.weight, src.light,
                                       src.sl, a, d_mask, npix, d_sums, stride, wrec, d_maps, d_picture);
            });
        }))
        return (int)hipErrorInvalidValue;
    if (const hipError_t e = hipGetLastError()) return (int)e;
    return film_finish_launch<kFpSums>(stream, sn.channels + (lum ? 1u : 0u), d_rec, d_sums, npix, d_wave, blocks);
}

// ---- the host twin: the same wt/film_polar.h functions per pixel in kernels_film.h's film_records_host -------------------------------------------
template <class Src>
static void film_polar_host_of(const sensor_t& sn, const Src& film, uint32_t flags, const film_polar_args_t& a, const float* mask, uint32_t n_threads, void* out_rec, float* maps,
                               void* picture) {
    const uint32_t C = sn.channels, P = C * 4u, NP = C + ((flags & FP_LUMINANCE) ? 1u : 0u);
    const uint64_t npix = (uint64_t)sn.width * sn.height;
    film_records_host<kFpSums>(npix, NP, mask, n_threads, static_cast<film_polar_rec_t*>(out_rec), [&](uint64_t p, bool included, film_element_t<kFpSums>* e) {
        float x[12] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (p < npix)
            for (uint32_t k = 0; k < P; ++k) x[k] = film.element_of(p * P + k, P);
        for (uint32_t c = 0; c < NP; ++c) {
            double S[4];
            fp_stokes(x, c, C, S);
            const fp_plane_t r = fp_plane(S[0], S[1], S[2], S[3], included, a.c2, a.s2);
            e[c].count[0] = r.nonfinite, e[c].count[1] = r.dark, e[c].count[2] = r.over;
            e[c].best = fc_best_t{};
            fp_best_take(e[c].best, r, p);
            for (uint32_t k = 0; k < kFpSums; ++k) e[c].add[k] = r.add[k];
            if (p >= npix) continue;
            if (maps) fp_store_maps(maps, p, c, NP, a, r, included);
            if (picture && c == a.picture_plane) {
                float rgb[3];
                fp_colour(a, (float)S[0], r, rgb);
                tm_store(picture, p, a.format, mask ? 4u : 3u, rgb, mask ? mask[p] : 0.f);
            }
        }
    });
}
void film_polar_host(const sensor_t& sn, const wtgpu_film_source& film, uint32_t flags, const film_polar_args_t& a, const float* mask, uint32_t n_threads, void* out_rec,
                     float* maps, void* picture) {
    film_source_dispatch(film, [&](auto src) { film_polar_host_of(sn, src, flags, a, mask, n_threads, out_rec, maps, picture); });
}

}   // namespace wtk
