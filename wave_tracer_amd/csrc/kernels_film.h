// wave_tracer_amd — what the film kernels (kernels_develop.hip, kernels_stats.hip, kernels_compare.hip, kernels_polar.hip, kernels_denoise.hip) and their host twins share beyond the
// arithmetic of wt/film_stats.h: the chunk geometry of the fixed summation order on a wavefront, the reduction of the chunk sums, the grid that
// follows the film, the choice of a kernel by (channels, luminance), and the host threads of the twins (kernels_mask.hip's too).
//
// Chunk geometry.  A block is kFilmBlock = 256 threads, four wavefronts; a wavefront owns whole chunks of kFsChunk = 256 elements.  Wavefront g
// of the grid takes chunks g, g + waves, ... (film_first_chunk, film_waves); of chunk k lane l holds elements 256 k + 64 j + l, j = 0 .. 3 (four
// loads of 64 consecutive elements: chunk_element), so the butterfly's distances 128 and 64 are the lane's own (d0 + d2) + (d1 + d3) and the rest
// are shuffles (chunk_sum): no LDS, no barrier per chunk.
#pragma once
#include <algorithm>
#include <atomic>
#include <thread>
#include <type_traits>
#include <vector>

#include "wtgpu_kernels.h"
#include "wt/film_stats.h"

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

// The grid follows the film: one wavefront per chunk while that is fewer than blocks_per_cu blocks per CU (a 37 x 23 film: one block, of which
// one wavefront has a partial chunk), then that many blocks whose wavefronts stride over the chunks, and more again only where a wavefront
// would exceed kFilmMaxChunksPerWave.
inline uint32_t film_grid_blocks(uint64_t npix, uint32_t n_cus, uint32_t blocks_per_cu) {
    const uint64_t n_chunks = fs_chunks(npix), quads = (n_chunks + kFilmWaves - 1) / kFilmWaves;
    const uint64_t need = (n_chunks + kFilmWaves * kFilmMaxChunksPerWave - 1) / (kFilmWaves * kFilmMaxChunksPerWave);
    return (uint32_t)std::min<uint64_t>(quads, std::max<uint64_t>((uint64_t)std::max(1u, n_cus) * blocks_per_cu, need));
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

// The host twins' threads: worker(claim) runs once on each of n_threads threads (0: one per hardware thread; never more than there are items;
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

}   // namespace wtk
