// wave_tracer_amd — comparison of two films on the device (see wtgpu_kernels.h for the list of kernel translation units): what parity checks, A/B
// runs and the half-film noise estimate used to download two sets of three f64 accumulators for.  k_film_compare reads both sets once,
// develops in registers (the developed values never reach memory), writes the chunk sums of the five sums in the fixed order of
// wt/film_stats.h, one record per wavefront with its counts and its largest difference, and — where asked for — the difference plane;
// k_film_compare_finish reduces the chunk sums level after level and merges the wavefronts' records.  No atomics: every field is the same
// whatever the schedule.  The arithmetic is wt/film_compare.h's, shared with the host twin at the end of the file: every count, the maximum and
// its pixel, the five sums and the difference plane are the same on both sides, bit for bit.  No render kernel is compiled here.
#include <cstring>
#include <mutex>

#include "kernels_film.h"
#include "wt/film_compare.h"

namespace wtk {

// A lane's u32 counts cannot overflow: it meets four pixels per chunk and a wavefront takes at most kFilmMaxChunksPerWave chunks, so a
// wavefront's counts stay below 64 x 4 x 2^20 = 2^28.
constexpr uint32_t kCompareBlocksPerCU = 8;

// what a wavefront leaves behind for one plane
struct fc_wave_rec_t {
    double max_abs;
    unsigned long long pixel;
    uint32_t n, nonfinite, mismatch, differ;
};
static_assert(sizeof(fc_wave_rec_t) == 32, "fc_wave_rec_t");

// the largest difference of a wavefront's lanes, by the distances of kernels_film.h's reductions
WT_D fc_best_t fc_wave_best(fc_best_t m) {
#pragma unroll
    for (int d = 32; d; d >>= 1) {
        const double v = __shfl_down(m.v, d, 64);
        const unsigned long long p = __shfl_down(m.pixel, d, 64);
        fc_best_merge(m, v, p);
    }
    return m;
}

// ---- k_film_compare: two sets of f64 films [H][W][P], [H][W] -> chunk sums, wavefront records, difference plane ------------------------------
// One lane per pixel, in the chunk geometry of kernels_film.h.  The loads are unconditional (a pixel past the film's end re-reads the last
// one) so that all of a chunk's are in flight together; `included` gates what they give.  A chunk's developed pairs stay in registers as f32
// while ONE plane at a time has its twenty f64 addends live.  Counts and the largest difference are per-lane registers over all the wavefront's chunks, reduced once at its end.
template <uint32_t C, bool kLum>
__global__ void __launch_bounds__(kFilmBlock) k_film_compare(const double* __restrict__ a_value, const double* __restrict__ a_weight, const double* __restrict__ a_light,
                                                             double sl_a, const double* __restrict__ b_value, const double* __restrict__ b_weight,
                                                             const double* __restrict__ b_light, double sl_b, uint32_t stokes, uint32_t s, uint32_t flags, double eps,
                                                             const float* __restrict__ mask, uint64_t npix, double* __restrict__ sums, uint64_t sums_stride,
                                                             fc_wave_rec_t* __restrict__ wrec, float* __restrict__ diff) {
    constexpr uint32_t NP = C + (kLum ? 1u : 0u);
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t n_chunks = fs_chunks(npix), n_waves = film_waves(), wave = film_first_chunk();
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
            fs_planes(a_value, a_light, a_weight[q], sl_a, q, C, stokes, s, kLum, flags, a);
            fs_planes(b_value, b_light, b_weight[q], sl_b, q, C, stokes, s, kLum, flags, b);
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
            for (uint32_t k = 0; k < kFcSums; ++k) {
                const double v = chunk_sum(t[k][0], t[k][1], t[k][2], t[k][3]);
                if (lane == 0) sums[(c * kFcSums + k) * sums_stride + chunk] = v;
            }
        }
    }
    // every wavefront of the grid leaves its records, also one that met no chunk: the finish kernel reads them all
    const unsigned long long n_all = wave_sum_u64(n_included);
#pragma unroll
    for (uint32_t c = 0; c < NP; ++c) {
        const fc_best_t m = fc_wave_best(best[c]);
        const unsigned long long nf = wave_sum_u64(n_nonfinite[c]), mm = wave_sum_u64(n_mismatch[c]), df = wave_sum_u64(n_differ[c]);
        if (lane == 0) wrec[c * n_waves + wave] = fc_wave_rec_t{m.v, m.pixel, (uint32_t)n_all, (uint32_t)nf, (uint32_t)mm, (uint32_t)df};
    }
}

// ---- k_film_compare_finish: kFcSums + 1 blocks per plane ----------------------------------------------------------------------------------------
// Block (c, k < kFcSums) reduces the chunk sums of sum k of plane c (film_reduce_levels).  Block (c, kFcSums) merges the wavefronts' records of
// plane c: integer counts, and a maximum whose order is total.  Every field of the record is written, so nobody has to clear it.
__global__ void __launch_bounds__(kFilmBlock) k_film_compare_finish(film_compare_rec_t* __restrict__ rec, double* sums, uint64_t sums_stride, uint64_t n_chunks,
                                                                    const fc_wave_rec_t* __restrict__ wrec, uint64_t n_waves) {
    const uint32_t lane = threadIdx.x & 63u, c = blockIdx.x / (kFcSums + 1u), k = blockIdx.x % (kFcSums + 1u);
    if (k < kFcSums) {
        const double sum = film_reduce_levels(sums + (c * kFcSums + k) * sums_stride, n_chunks);
        if (threadIdx.x == 0) rec[c].sum[k] = sum;
        return;
    }
    __shared__ double s_best_v[kFilmWaves];
    __shared__ unsigned long long s_best_pixel[kFilmWaves];
    __shared__ unsigned long long s_count[kFilmWaves][4];
    fc_best_t m;
    unsigned long long cnt[4] = {0ull, 0ull, 0ull, 0ull};
    for (uint64_t w = threadIdx.x; w < n_waves; w += kFilmBlock) {
        const fc_wave_rec_t r = wrec[c * n_waves + w];
        fc_best_merge(m, r.max_abs, r.pixel);
        cnt[0] += r.n, cnt[1] += r.nonfinite, cnt[2] += r.mismatch, cnt[3] += r.differ;
    }
    m = fc_wave_best(m);
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) cnt[i] = wave_sum_u64(cnt[i]);
    if (lane == 0) {
        s_best_v[threadIdx.x >> 6] = m.v;
        s_best_pixel[threadIdx.x >> 6] = m.pixel;
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) s_count[threadIdx.x >> 6][i] = cnt[i];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t w = 1; w < kFilmWaves; ++w) {
            fc_best_merge(m, s_best_v[w], s_best_pixel[w]);
            for (uint32_t i = 0; i < 4; ++i) cnt[i] += s_count[w][i];
        }
        film_compare_rec_t& r = rec[c];
        r.n = cnt[0], r.n_nonfinite = cnt[1], r.n_nonfinite_mismatch = cnt[2], r.n_differ = cnt[3];
        r.max_abs = m.v;
        r.argmax = m.pixel;
    }
}

// kCompareBlocksPerCU blocks per CU at most (1920 x 1088: 8160 chunks on 2040 blocks, one per wavefront)
static uint32_t film_compare_blocks(uint64_t npix, uint32_t n_cus) { return film_grid_blocks(npix, n_cus, kCompareBlocksPerCU); }
size_t film_compare_wave_bytes(uint64_t npix, uint32_t n_cus) { return (size_t)kFsMaxPlanes * film_compare_blocks(npix, n_cus) * kFilmWaves * sizeof(fc_wave_rec_t); }

int film_compare_launch(const sensor_t& sn, hipStream_t stream, uint32_t n_cus, const double* a_value, const double* a_weight, const double* a_light, uint64_t spe_a,
                        const double* b_value, const double* b_weight, const double* b_light, uint64_t spe_b, uint32_t s, uint32_t flags, double eps, const float* d_mask,
                        void* d_rec, double* d_sums, void* d_wave, float* d_diff) {
    const uint64_t npix = (uint64_t)sn.width * sn.height;
    if (npix == 0) return (int)hipErrorInvalidValue;
    const double sl_a = develop_scale(spe_a), sl_b = develop_scale(spe_b);
    const bool lum = (flags & FS_LUMINANCE) != 0;
    const uint64_t n_chunks = fs_chunks(npix), stride = fs_scratch_len(npix);
    const uint32_t blocks = film_compare_blocks(npix, n_cus), stokes = film_stokes(sn);
    const uint64_t n_waves = (uint64_t)blocks * kFilmWaves;
    film_compare_rec_t* rec = static_cast<film_compare_rec_t*>(d_rec);
    fc_wave_rec_t* wrec = static_cast<fc_wave_rec_t*>(d_wave);
    if (!film_dispatch(sn.channels, lum, [&](auto c, auto l) {
            hipLaunchKernelGGL((k_film_compare<decltype(c)::value, decltype(l)::value>), dim3(blocks), dim3(kFilmBlock), 0, stream, a_value, a_weight, a_light, sl_a, b_value,
                               b_weight, b_light, sl_b, stokes, s, flags, eps, d_mask, npix, d_sums, stride, wrec, d_diff);
        }))
        return (int)hipErrorInvalidValue;
    if (const hipError_t e = hipGetLastError()) return (int)e;
    hipLaunchKernelGGL(k_film_compare_finish, dim3((sn.channels + (lum ? 1u : 0u)) * (kFcSums + 1u)), dim3(kFilmBlock), 0, stream, rec, d_sums, stride, n_chunks, wrec, n_waves);
    return (int)hipGetLastError();
}

// ---- the host twin: the same wt/film_compare.h functions on host threads, one task per chunk; the counts are integers, a chunk's sums are one
// thread's and the maximum's order is total, so the result does not depend on the number of threads --------------------------------------------
void film_compare_host(const sensor_t& sn, const double* a_value, const double* a_weight, const double* a_light, uint64_t spe_a, const double* b_value,
                       const double* b_weight, const double* b_light, uint64_t spe_b, uint32_t s, uint32_t flags, double eps, const float* mask, uint32_t n_threads,
                       void* out_rec, float* diff) {
    const uint32_t C = sn.channels, stokes = film_stokes(sn), NP = C + ((flags & FS_LUMINANCE) ? 1u : 0u);
    const uint64_t npix = (uint64_t)sn.width * sn.height, n_chunks = fs_chunks(npix), stride = fs_scratch_len(npix);
    const double sl_a = develop_scale(spe_a), sl_b = develop_scale(spe_b);
    film_compare_rec_t* rec = static_cast<film_compare_rec_t*>(out_rec);
    std::memset(rec, 0, NP * sizeof(film_compare_rec_t));
    std::vector<double> sums((size_t)NP * kFcSums * std::max<uint64_t>(stride, 1), 0.0);
    std::vector<fc_best_t> best(NP);
    std::mutex merge;
    on_threads(n_chunks, n_threads, [&](auto claim) {
        std::vector<film_compare_rec_t> my(NP, film_compare_rec_t{});
        std::vector<fc_best_t> my_best(NP);
        std::vector<double> a((size_t)kFsMaxPlanes * kFcSums * kFsChunk);
        for (uint64_t chunk = claim(); chunk < n_chunks; chunk = claim()) {
            for (uint32_t i = 0; i < kFsChunk; ++i) {
                const uint64_t p = chunk * kFsChunk + i;
                const bool included = p < npix && (!mask || mask[p] > 0.f);
                float xa[kFsMaxPlanes] = {0.f, 0.f, 0.f, 0.f}, xb[kFsMaxPlanes] = {0.f, 0.f, 0.f, 0.f};
                if (included) {
                    fs_planes(a_value, a_light, a_weight[p], sl_a, p, C, stokes, s, NP > C, flags, xa);
                    fs_planes(b_value, b_light, b_weight[p], sl_b, p, C, stokes, s, NP > C, flags, xb);
                }
                for (uint32_t c = 0; c < NP; ++c) {
                    const fc_pair_t r = fc_pair(xa[c], xb[c], included, eps);
                    for (uint32_t k = 0; k < kFcSums; ++k) a[((size_t)c * kFcSums + k) * kFsChunk + i] = r.add[k];
                    if (p < npix && diff) diff[p * NP + c] = fc_diff(xa[c], xb[c], included);
                    if (!included) continue;
                    ++my[c].n;
                    my[c].n_nonfinite += r.nonfinite, my[c].n_nonfinite_mismatch += r.mismatch, my[c].n_differ += r.differ;
                    fc_best_take(my_best[c], r.abs_d, p);
                }
            }
            for (uint32_t c = 0; c < NP; ++c)
                for (uint32_t k = 0; k < kFcSums; ++k) sums[((size_t)c * kFcSums + k) * stride + chunk] = fs_chunk_sum(&a[((size_t)c * kFcSums + k) * kFsChunk]);
        }
        std::lock_guard<std::mutex> lock(merge);
        for (uint32_t c = 0; c < NP; ++c) {
            film_compare_rec_t& r = rec[c];
            r.n += my[c].n, r.n_nonfinite += my[c].n_nonfinite, r.n_nonfinite_mismatch += my[c].n_nonfinite_mismatch, r.n_differ += my[c].n_differ;
            fc_best_merge(best[c], my_best[c].v, my_best[c].pixel);
        }
    });
    // the levels above the chunks (k_film_compare_finish)
    for (uint32_t c = 0; c < NP; ++c) {
        for (uint32_t k = 0; k < kFcSums; ++k) rec[c].sum[k] = fs_reduce_levels(sums.data() + ((size_t)c * kFcSums + k) * stride, n_chunks);
        rec[c].max_abs = best[c].v;
        rec[c].argmax = best[c].pixel;
    }
}

}   // namespace wtk
