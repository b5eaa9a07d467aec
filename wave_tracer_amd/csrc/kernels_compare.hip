// wave_tracer_amd — comparison of two films on the device (see wtgpu_kernels.h for the list of kernel translation units): what parity checks, A/B
// runs and the half-film noise estimate used to download two sets of three f64 accumulators for.  k_film_compare reads both sets once,
// develops in registers (the developed values never reach memory), writes the chunk sums of the five sums in the fixed order of
// wt/film_stats.h, one record per wavefront with its counts and its largest difference, and — where asked for — the difference plane;
// kernels_film.h's k_film_finish reduces the chunk sums level after level and merges the wavefronts' records.  No atomics: every field is the same
// whatever the schedule.  The arithmetic is wt/film_compare.h's, shared with the host twin at the end of the file: every count, the maximum and
// its pixel, the five sums and the difference plane are the same on both sides, bit for bit.  Either operand may be a developed f32 film instead
// (wt/film_stats.h: film_src_t; four instantiations by operand).  No render kernel is compiled here.
#include "kernels_film.h"
#include "wt/film_compare.h"

namespace wtk {

// ---- k_film_compare: two films, each f64 accumulators [H][W][P], [H][W] or a developed f32 film [H][W][P] -> chunk sums, wavefront records, difference plane ------------------------------
// One lane per pixel, in the chunk geometry of kernels_film.h.  The loads are unconditional (a pixel past the film's end re-reads the last
// one) so that all of a chunk's are in flight together; `included` gates what they give.  A chunk's developed pairs stay in registers as f32
// while ONE plane at a time has its twenty f64 addends live.  Counts and the largest difference are per-lane registers over all the wavefront's chunks, reduced once at its end.
// kDevA / kDevB (that operand is a developed film, in a_value / b_value; wt/film_stats.h: film_src), four combinations: the same lane per pixel
// and the same unconditional loads, a developed operand's C floats by 4-byte loads `stokes` floats apart for the reasons k_film_stats gives
// (kernels_stats.hip) — contiguous across the wavefront for a monochromatic or RGB film, one component in four of a polarimetric one.
template <bool kDevA, bool kDevB, uint32_t C, bool kLum>
__global__ void __launch_bounds__(kFilmBlock) k_film_compare(const film_elem_t<kDevA>* __restrict__ a_value, const double* __restrict__ a_weight, const double* __restrict__ a_light,
                                                             double sl_a, const film_elem_t<kDevB>* __restrict__ b_value, const double* __restrict__ b_weight,
                                                             const double* __restrict__ b_light, double sl_b, uint32_t stokes, uint32_t s, uint32_t flags, double eps,
                                                             const float* __restrict__ mask, uint64_t npix, double* __restrict__ sums, uint64_t sums_stride,
                                                             film_wave_rec_t* __restrict__ wrec, float* __restrict__ diff) {
    constexpr uint32_t NP = C + (kLum ? 1u : 0u);
    const uint64_t n_chunks = fs_chunks(npix), n_waves = film_waves(), wave = film_first_chunk();
    const film_src_t<kDevA> film_a = film_src(a_value, a_weight, a_light, sl_a);
    const film_src_t<kDevB> film_b = film_src(b_value, b_weight, b_light, sl_b);
    fc_best_t best[NP];
    uint32_t n_nonfinite[NP], n_mismatch[NP], n_differ[NP], n_included = 0;
#pragma unroll
    for (uint32_t c = 0; c < NP; ++c) n_nonfinite[c] = n_mismatch[c] = n_differ[c] = 0u;
    for (uint64_t chunk = wave; chunk < n_chunks; chunk += n_waves) {
        float xa[NP][4], xb[NP][4];
        bool included[4];
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint64_t p = chunk_element(chunk, j), q = p < npix ? p : npix - 1;
            included[j] = p < npix && (!mask || mask[q] > 0.f);
            float a[NP], b[NP];
            fs_planes(film_a, q, C, stokes, s, kLum, flags, a);
            fs_planes(film_b, q, C, stokes, s, kLum, flags, b);
#pragma unroll
            for (uint32_t c = 0; c < NP; ++c) xa[c][j] = a[c], xb[c][j] = b[c];
            n_included += included[j] ? 1u : 0u;
            if (diff && p < npix) {
#pragma unroll
                for (uint32_t c = 0; c < NP; ++c) diff[p * NP + c] = fc_diff(xa[c][j], xb[c][j], included[j]);
            }
        }
#pragma unroll
        for (uint32_t c = 0; c < NP; ++c) {
            double t[kFcSums][4];
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                const fc_pair_t r = fc_pair(xa[c][j], xb[c][j], included[j], eps);
                n_nonfinite[c] += r.nonfinite;
                n_mismatch[c] += r.mismatch;
                n_differ[c] += r.differ;
                fc_best_take(best[c], r.abs_d, chunk_element(chunk, j));
#pragma unroll
                for (uint32_t k = 0; k < kFcSums; ++k) t[k][j] = r.add[k];
            }
#pragma unroll
            for (uint32_t k = 0; k < kFcSums; ++k) film_store_chunk_sum(sums + (c * kFcSums + k) * sums_stride + chunk, t[k]);
        }
    }
    film_store_wave_recs(wrec, n_waves, wave, n_included, n_nonfinite, n_mismatch, n_differ, best);
}

// the wavefronts' records of a records pass (this one and kernels_polar.hip's), kFsMaxPlanes planes
size_t film_rec_wave_bytes(uint64_t npix, uint32_t n_cus) { return (size_t)kFsMaxPlanes * film_rec_blocks(npix, n_cus) * kFilmWaves * sizeof(film_wave_rec_t); }

int film_compare_launch(const sensor_t& sn, hipStream_t stream, uint32_t n_cus, const wtgpu_film_source& a, const wtgpu_film_source& b, uint32_t s, uint32_t flags, double eps,
                        const float* d_mask, void* d_rec, double* d_sums, void* d_wave, float* d_diff) {
    const uint64_t npix = (uint64_t)sn.width * sn.height;
    if (npix == 0) return (int)hipErrorInvalidValue;
    const bool lum = (flags & FS_LUMINANCE) != 0;
    const uint64_t stride = fs_scratch_len(npix);
    const uint32_t blocks = film_rec_blocks(npix, n_cus), stokes = film_stokes(sn);
    film_wave_rec_t* wrec = static_cast<film_wave_rec_t*>(d_wave);
    if (!film_dispatch(sn.channels, lum, [&](auto c, auto l) {
            film_source_dispatch(a, [&](auto fa) {
                film_source_dispatch(b, [&](auto fb) {
                    hipLaunchKernelGGL((k_film_compare<decltype(fa)::developed, decltype(fb)::developed, decltype(c)::value, decltype(l)::value>), dim3(blocks), dim3(kFilmBlock), 0,
                                       stream, fa.first(), fa.weight, fa.light, fa.sl, fb.first(), fb.weight, fb.light, fb.sl, stokes, s, flags, eps, d_mask, npix, d_sums, stride, wrec,
                                       d_diff);
                });
            });
        }))
        return (int)hipErrorInvalidValue;
    if (const hipError_t e = hipGetLastError()) return (int)e;
    return film_finish_launch<kFcSums>(stream, sn.channels + (lum ? 1u : 0u), d_rec, d_sums, npix, d_wave, blocks);
}

// ---- the host twin: the same wt/film_compare.h functions per pixel in kernels_film.h's film_records_host -----------------------------------------
template <class SrcA, class SrcB>
static void film_compare_host_of(const sensor_t& sn, const SrcA& film_a, const SrcB& film_b, uint32_t s, uint32_t flags, double eps, const float* mask, uint32_t n_threads,
                                 void* out_rec, float* diff) {
    const uint32_t C = sn.channels, stokes = film_stokes(sn), NP = C + ((flags & FS_LUMINANCE) ? 1u : 0u);
    const uint64_t npix = (uint64_t)sn.width * sn.height;
    film_records_host<kFcSums>(npix, NP, mask, n_threads, static_cast<film_compare_rec_t*>(out_rec), [&](uint64_t p, bool included, film_element_t<kFcSums>* e) {
        float xa[kFsMaxPlanes] = {0.f, 0.f, 0.f, 0.f}, xb[kFsMaxPlanes] = {0.f, 0.f, 0.f, 0.f};
        if (included) {
            fs_planes(film_a, p, C, stokes, s, NP > C, flags, xa);
            fs_planes(film_b, p, C, stokes, s, NP > C, flags, xb);
        }
        for (uint32_t c = 0; c < NP; ++c) {
            const fc_pair_t r = fc_pair(xa[c], xb[c], included, eps);
            e[c].count[0] = r.nonfinite, e[c].count[1] = r.mismatch, e[c].count[2] = r.differ;
            e[c].best = fc_best_t{};
            fc_best_take(e[c].best, r.abs_d, p);   // (only a pair with |d| > 0 is a candidate)
            for (uint32_t k = 0; k < kFcSums; ++k) e[c].add[k] = r.add[k];
            if (p < npix && diff) diff[p * NP + c] = fc_diff(xa[c], xb[c], included);
        }
    });
}
void film_compare_host(const sensor_t& sn, const wtgpu_film_source& a, const wtgpu_film_source& b, uint32_t s, uint32_t flags, double eps, const float* mask, uint32_t n_threads,
                       void* out_rec, float* diff) {
    film_source_dispatch(a, [&](auto fa) {
        film_source_dispatch(b, [&](auto fb) { film_compare_host_of(sn, fa, fb, s, flags, eps, mask, n_threads, out_rec, diff); });
    });
}

}   // namespace wtk
