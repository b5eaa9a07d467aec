// wave_tracer_amd — what the film kernels (kernels_develop.hip, kernels_stats.hip, kernels_compare.hip, kernels_polar.hip, kernels_denoise.hip) and their host twins share beyond the
// arithmetic of wt/film_stats.h: the chunk geometry of the fixed summation order on a wavefront, the reduction of the chunk sums, the grid that
// follows the film, the choice of a kernel by (channels, luminance) and by the film's source (film_source_dispatch), and the host threads of the twins (the sensor-element maps' too: kernels_maps.h).
//
// Chunk geometry.  A block is kFilmBlock = 256 threads, four wavefronts; a wavefront owns whole chunks of kFsChunk = 256 elements.  Wavefront g
// of the grid takes chunks g, g + waves, ... (film_first_chunk, film_waves); of chunk k lane l holds elements 256 k + 64 j + l, j = 0 .. 3 (four
// loads of 64 consecutive elements: chunk_element), so the butterfly's distances 128 and 64 are the lane's own (d0 + d2) + (d1 + d3) and the rest
// are shuffles (chunk_sum): no LDS, no barrier per chunk.
#pragma once
#include <algorithm>
#include <atomic>
#include <mutex>
#include <thread>
#include <type_traits>
#include <vector>

#include "wtgpu_kernels.h"
#include "wt/film_compare.h"

namespace wtk {

constexpr int kFilmBlock = 256;
constexpr uint32_t kFilmWaves = kFilmBlock / 64;
static_assert(kFsChunk == 4 * 64, "a lane holds four elements of a chunk");
// A wavefront takes at most this many chunks (the grid grows with the film beyond that): what keeps the kernels' u32 counts from overflowing.
constexpr uint64_t kFilmMaxChunksPerWave = 1ull << 20;

// ---- reductions over a wavefront, distances 32 .. 1: lane i takes lane i + d; lane 0 ends with the result of the 64 -------------------------
WT_D double wave_sum_f64(double t) {
#pragma unroll
    for (int d = 32; d; d >>= 1) t += __shfl_down(t, d, 64);
    return t;
}
WT_D unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int d = 32; d; d >>= 1) v += __shfl_down(v, d, 64);
    return v;
}
WT_D uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
    for (int d = 32; d; d >>= 1) v = max(v, (uint32_t)__shfl_down((int)v, d, 64));
    return v;
}

// the best of a wavefront's lanes (wt/film_compare.h: fc_best_t, whose order is total)
WT_D fc_best_t wave_best(fc_best_t m) {
#pragma unroll
    for (int d = 32; d; d >>= 1) {
        const double v = __shfl_down(m.v, d, 64);
        const unsigned long long p = __shfl_down(m.pixel, d, 64);
        fc_best_merge(m, v, p);
    }
    return m;
}

// ---- the chunk loop ---------------------------------------------------------------------------------------------------------------------------
WT_D uint64_t film_first_chunk() { return (uint64_t)blockIdx.x * kFilmWaves + (threadIdx.x >> 6); }   // also the wavefront's index in the grid
WT_D uint64_t film_waves() { return (uint64_t)gridDim.x * kFilmWaves; }
WT_D uint64_t chunk_element(uint64_t chunk, uint32_t j) { return chunk * kFsChunk + j * 64u + (threadIdx.x & 63u); }
// the chunk's sum (in lane 0) from every lane's four addends
WT_D double chunk_sum(double d0, double d1, double d2, double d3) { return wave_sum_f64((d0 + d2) + (d1 + d3)); }

// The levels above the chunks, by one block (wt/film_stats.h: fs_reduce_levels is the host's): a plane's n_chunks chunk sums are reduced by the
// same rule, level after level (a 1920 x 1088 film: 8160 -> 32 -> 1), each level written behind the one it reads.  Returns the one number
// left — +0.0 where there is no chunk — to thread 0, which stores it, and +0.0 to the others.
WT_D double film_reduce_levels(double* sums, uint64_t n_chunks) {
    double* in = sums;
    uint64_t n = n_chunks;
    while (n > 1) {
        double* out = in + n;
        const uint64_t m = fs_chunks(n);
        for (uint64_t chunk = threadIdx.x >> 6; chunk < m; chunk += kFilmWaves) {
            double d[4];
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                const uint64_t i = chunk_element(chunk, j);
                d[j] = i < n ? in[i] : 0.0;
            }
            const double t = chunk_sum(d[0], d[1], d[2], d[3]);
            if ((threadIdx.x & 63u) == 0) out[chunk] = t;
        }
        __threadfence_block();
        __syncthreads();
        in = out;
        n = m;
    }
    return n && threadIdx.x == 0 ? in[0] : 0.0;
}

// ---- the "sums + counts + best" pass (k_film_compare, k_film_polar): K sums, three counts of classes and the best pixel per plane -------------
// What a wavefront leaves behind for one plane.  A lane's u32 counts cannot overflow: it meets four pixels per chunk and a wavefront takes at
// most kFilmMaxChunksPerWave chunks, so a wavefront's counts stay below 64 x 4 x 2^20 = 2^28.
struct film_wave_rec_t {
    double best;
    unsigned long long pixel;
    uint32_t n, count[3];
};
static_assert(sizeof(film_wave_rec_t) == 32, "film_wave_rec_t");
constexpr uint32_t kFilmRecBlocksPerCU = 8;

// one of a plane's chunk sums from every lane's four addends, stored by lane 0
WT_D void film_store_chunk_sum(double* out, const double (&d)[4]) {
    const double v = chunk_sum(d[0], d[1], d[2], d[3]);
    if ((threadIdx.x & 63u) == 0) *out = v;
}
// The end of the main kernel: every wavefront of the grid leaves its records, also one that met no chunk (the finish kernel reads them all),
// from its lanes' members, counts and best of each of the NP planes.  (n_waves and wave are the kernel's own values: recomputed here they cost
// both kernels two scalar registers, and a store helper over all K sums moved their vector registers; profiles/film_shared_kernel_resources.txt.)
template <uint32_t NP>
WT_D void film_store_wave_recs(film_wave_rec_t* wrec, uint64_t n_waves, uint64_t wave, uint32_t n_included, const uint32_t (&c0)[NP], const uint32_t (&c1)[NP], const uint32_t (&c2)[NP],
                               const fc_best_t (&best)[NP]) {
    const unsigned long long n_all = wave_sum_u64(n_included);
#pragma unroll
    for (uint32_t c = 0; c < NP; ++c) {
        const fc_best_t m = wave_best(best[c]);
        const unsigned long long s0 = wave_sum_u64(c0[c]), s1 = wave_sum_u64(c1[c]), s2 = wave_sum_u64(c2[c]);
        if ((threadIdx.x & 63u) == 0) wrec[c * n_waves + wave] = film_wave_rec_t{m.v, m.pixel, (uint32_t)n_all, {(uint32_t)s0, (uint32_t)s1, (uint32_t)s2}};
    }
}

// k_film_finish: K + 1 blocks per plane.  Block (c, k < K) reduces the chunk sums of sum k of plane c (film_reduce_levels).  Block (c, K) merges
// the wavefronts' records of plane c: integer counts, and a maximum whose order is total.  Every field of the record is written, so nobody has
// to clear it.
template <uint32_t K>
__global__ void __launch_bounds__(kFilmBlock) k_film_finish(film_best_rec_t<K>* __restrict__ rec, double* sums, uint64_t sums_stride, uint64_t n_chunks,
                                                            const film_wave_rec_t* __restrict__ wrec, uint64_t n_waves) {
    const uint32_t lane = threadIdx.x & 63u, c = blockIdx.x / (K + 1u), k = blockIdx.x % (K + 1u);
    if (k < K) {
        const double sum = film_reduce_levels(sums + (c * K + k) * sums_stride, n_chunks);
        if (threadIdx.x == 0) rec[c].sum[k] = sum;
        return;
    }
    __shared__ double s_best_v[kFilmWaves];
    __shared__ unsigned long long s_best_pixel[kFilmWaves];
    __shared__ unsigned long long s_count[kFilmWaves][4];
    fc_best_t m;
    unsigned long long cnt[4] = {0ull, 0ull, 0ull, 0ull};
    for (uint64_t w = threadIdx.x; w < n_waves; w += kFilmBlock) {
        const film_wave_rec_t r = wrec[c * n_waves + w];
        fc_best_merge(m, r.best, r.pixel);
        cnt[0] += r.n, cnt[1] += r.count[0], cnt[2] += r.count[1], cnt[3] += r.count[2];
    }
    m = wave_best(m);
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
        film_best_rec_t<K>& r = rec[c];
        r.n = cnt[0], r.count[0] = cnt[1], r.count[1] = cnt[2], r.count[2] = cnt[3];
        r.best = m.v;
        r.argmax = m.pixel;
    }
}

// The grid follows the film: one wavefront per chunk while that is fewer than blocks_per_cu blocks per CU (a 37 x 23 film: one block, of which
// one wavefront has a partial chunk), then that many blocks whose wavefronts stride over the chunks, and more again only where a wavefront
// would exceed kFilmMaxChunksPerWave.
inline uint32_t film_grid_blocks(uint64_t npix, uint32_t n_cus, uint32_t blocks_per_cu) {
    const uint64_t n_chunks = fs_chunks(npix), quads = (n_chunks + kFilmWaves - 1) / kFilmWaves;
    const uint64_t need = (n_chunks + kFilmWaves * kFilmMaxChunksPerWave - 1) / (kFilmWaves * kFilmMaxChunksPerWave);
    return (uint32_t)std::min<uint64_t>(quads, std::max<uint64_t>((uint64_t)std::max(1u, n_cus) * blocks_per_cu, need));
}

// the grid of a records pass: kFilmRecBlocksPerCU blocks per CU at most (1920 x 1088: 8160 chunks on 2040 blocks, one per wavefront);
// film_rec_wave_bytes (wtgpu_kernels.h; kernels_compare.hip) has the bytes of its wavefronts' records
inline uint32_t film_rec_blocks(uint64_t npix, uint32_t n_cus) { return film_grid_blocks(npix, n_cus, kFilmRecBlocksPerCU); }
// the finish kernel behind a records pass of `planes` planes
template <uint32_t K>
int film_finish_launch(hipStream_t stream, uint32_t planes, void* d_rec, double* d_sums, uint64_t npix, const void* d_wave, uint32_t blocks) {
    hipLaunchKernelGGL(k_film_finish<K>, dim3(planes * (K + 1u)), dim3(kFilmBlock), 0, stream, static_cast<film_best_rec_t<K>*>(d_rec), d_sums, fs_scratch_len(npix), fs_chunks(npix),
                       static_cast<const film_wave_rec_t*>(d_wave), (uint64_t)blocks * kFilmWaves);
    return (int)hipGetLastError();
}

// The kernels are compiled for 1 channel, 3 channels, and 3 channels with their luminance: fn(C, kLum) gets the film's as constants
// (decltype(C)::value).  false: not a film these kernels read, and fn has not run.
template <class F>
bool film_dispatch(uint32_t channels, bool luminance, F&& fn) {
    if (channels == 1 && !luminance)
        fn(std::integral_constant<uint32_t, 1>{}, std::false_type{});
    else if (channels == 3 && !luminance)
        fn(std::integral_constant<uint32_t, 3>{}, std::false_type{});
    else if (channels == 3)
        fn(std::integral_constant<uint32_t, 3>{}, std::true_type{});
    else
        return false;
    return true;
}

// The kernels and the twins are compiled for the source kind as well: fn(src) gets the film_src_t (wt/film_stats.h) of a wtgpu_film_source that
// has passed the entry point's check — a developed film, or the accumulators with their develop_scale(spe).
template <class F>
void film_source_dispatch(const wtgpu_film_source& f, F&& fn) {
    if (f.developed)
        fn(film_dev_t{f.developed});
    else
        fn(film_acc_t{f.value, f.weight, f.light, develop_scale(f.spe)});
}

// The host twins' threads:worker(claim) runs once on each of n_threads threads (0: one per hardware thread; never more than there are items;
// the caller's is one of them) and takes items with  for (i = claim(); i < n_items; i = claim()).  What a thread keeps to itself — a stack,
// partial records — lives in the worker's own frame.
template <class F>
void on_threads(uint64_t n_items, uint32_t n_threads, F&& worker) {
    std::atomic<uint64_t> next{0};
    auto run = [&]() { worker([&]() { return next++; }); };
    if (n_threads == 0) n_threads = std::max(1u, std::thread::hardware_concurrency());
    n_threads = (uint32_t)std::min<uint64_t>(n_threads, std::max<uint64_t>(1, n_items));
    std::vector<std::thread> pool;
    for (uint32_t t = 1; t < n_threads; ++t) pool.emplace_back(run);
    run();
    for (auto& t : pool) t.join();
}

// The host twin of a records pass: per_pixel(p, included, e) fills e[c], c < NP, for pixel p (also for the p >= npix that fill the last chunk,
// never included) — the three counts, the maximum's candidate and the K addends of each plane — and does its own side stores.  One task per
// chunk; the counts are integers, a chunk's sums are one thread's and the maximum's order is total, so the result does not depend on the number
// of threads.
template <uint32_t K>
struct film_element_t {
    uint32_t count[3];   // 0 or 1
    fc_best_t best;
    double add[K];
};
template <uint32_t K, class F>
void film_records_host(uint64_t npix, uint32_t NP, const float* mask, uint32_t n_threads, film_best_rec_t<K>* rec, F&& per_pixel) {
    const uint64_t n_chunks = fs_chunks(npix), stride = fs_scratch_len(npix);
    std::fill_n(rec, NP, film_best_rec_t<K>{});
    std::vector<double> sums((size_t)NP * K * std::max<uint64_t>(stride, 1), 0.0);
    std::vector<fc_best_t> best(NP);
    std::mutex merge;
    on_threads(n_chunks, n_threads, [&](auto claim) {
        struct counts_t {
            unsigned long long n = 0, count[3] = {0, 0, 0};
        };
        std::vector<counts_t> my(NP);
        std::vector<fc_best_t> my_best(NP);
        std::vector<double> t((size_t)kFsMaxPlanes * K * kFsChunk);
        film_element_t<K> e[kFsMaxPlanes];
        for (uint64_t chunk = claim(); chunk < n_chunks; chunk = claim()) {
            for (uint32_t i = 0; i < kFsChunk; ++i) {
                const uint64_t p = chunk * kFsChunk + i;
                const bool included = p < npix && (!mask || mask[p] > 0.f);
                per_pixel(p, included, e);
                for (uint32_t c = 0; c < NP; ++c) {
                    for (uint32_t k = 0; k < K; ++k) t[((size_t)c * K + k) * kFsChunk + i] = e[c].add[k];
                    my[c].n += included ? 1u : 0u;
                    for (uint32_t j = 0; j < 3; ++j) my[c].count[j] += e[c].count[j];
                    fc_best_merge(my_best[c], e[c].best.v, e[c].best.pixel);
                }
            }
            for (uint32_t c = 0; c < NP; ++c)
                for (uint32_t k = 0; k < K; ++k) sums[((size_t)c * K + k) * stride + chunk] = fs_chunk_sum(&t[((size_t)c * K + k) * kFsChunk]);
        }
        std::lock_guard<std::mutex> lock(merge);
        for (uint32_t c = 0; c < NP; ++c) {
            rec[c].n += my[c].n;
            for (uint32_t j = 0; j < 3; ++j) rec[c].count[j] += my[c].count[j];
            fc_best_merge(best[c], my_best[c].v, my_best[c].pixel);
        }
    });
    // the levels above the chunks (k_film_finish)
    for (uint32_t c = 0; c < NP; ++c) {
        for (uint32_t k = 0; k < K; ++k) rec[c].sum[k] = fs_reduce_levels(sums.data() + ((size_t)c * K + k) * stride, n_chunks);
        rec[c].best = best[c].v;
        rec[c].argmax = best[c].pixel;
    }
}

}   // namespace wtk
