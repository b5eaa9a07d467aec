// wave_tracer_amd — film statistics on the device (see wtgpu_kernels.h for the list of kernel translation units): what choosing a dB range or an
// exposure used to download the three f64 accumulators for.  k_film_stats reads them once, develops in registers (the developed values never
// reach memory, as in k_develop_tonemap), classifies every element against an edge table staged in LDS, counts the bins in a per-block LDS
// histogram, takes the extrema and writes the chunk sums of the fixed summation order; k_film_stats_finish reduces the chunk sums and turns
// the extrema's keys into floats.  The arithmetic is wt/film_stats.h's, shared with the host twin at the end of the file: every counter, every
// bin, the extrema and the sum are the same on both sides, bit for bit.  Measured on the MI355X (tools/bench_film_stats.py, docs/FEATURES.md): 0.39 ms
// for the 418 MB of the polarimetric 1920 x 1088 film, 1.06 TB/s — a fifth of k_develop's rate on the same film: the per-element work, not the
// memory system, sets the time.  The same kernel is compiled for a developed f32 film as its source (wt/film_stats.h: film_src_t).  No render kernel
// is compiled here.
#include <cstring>
#include <mutex>

#include "kernels_film.h"

namespace wtk {

// Two instantiations by LDS: 4 (cap + 1 + planes x cap) bytes with cap = 1024 (20 KB at four planes: several blocks per CU) or 4096 (80 KB of the
// CU's 160: one block).  There is no overflow path: bins <= kFsMaxBins is checked before the launch.
constexpr uint32_t kStatsSmallBins = 1024;
// A block's u32 bins cannot overflow: a wavefront takes at most kFilmMaxChunksPerWave chunks, so a block counts at most 4 x 2^20 x 256 = 2^30
// elements per plane.
constexpr uint32_t kStatsBlocksPerCU = 4;

// ---- k_film_stats: f64 films [H][W][P], [H][W] (or a developed f32 film [H][W][P]) -> records, histogram, chunk sums ----------------------------------------------------------
// One lane per pixel, its C = 1 or 3 developed values of Stokes component s (and their luminance) in registers, in the chunk geometry of
// kernels_film.h.  The loads are conditional: an excluded pixel's films are not read.
// Bins: LDS atomics on the block's u32 histogram, flushed with 64-bit global atomics at the end (non-zero bins only).  The five classes
// outside the bins and n are wavefront-uniform counts (ballots): zeros of an unlit background would otherwise all hit one LDS word.
// Extrema: per lane as keys (fs_key) over all its chunks, one wavefront reduction and one global atomic each at the end.
// kDev (a developed film, in `value`; wt/film_stats.h: film_src): the same lane per pixel, which takes its C floats with 4-byte loads, `stokes`
// floats apart.  A monochromatic or RGB film's 4 C bytes per lane are contiguous across the wavefront (an RGB wavefront's three load instructions
// cover the same 768 bytes, every line of them used); of a polarimetric film the pass wants one component in four, so three quarters of each
// line are fetched for nothing — 48 bytes per pixel at most against the accumulators' 200, and a vector load per lane would fetch the same
// lines to throw the same bytes away in registers.  No vector load, so no alignment is asked of the film.
template <bool kDev, uint32_t C, bool kLum, uint32_t kBinCap>
__global__ void __launch_bounds__(kFilmBlock) k_film_stats(const film_elem_t<kDev>* __restrict__ value, const double* __restrict__ weight, const double* __restrict__ light,
                                                           double sl, uint32_t stokes, uint32_t s, uint32_t flags, const float* __restrict__ mask, uint64_t npix,
                                                           const float* __restrict__ edges, uint32_t bins, film_stats_rec_t* __restrict__ rec,
                                                           unsigned long long* __restrict__ hist, double* __restrict__ sums, uint64_t sums_stride) {
    constexpr uint32_t NP = C + (kLum ? 1u : 0u);
    __shared__ float s_edge[kBinCap + 1];
    __shared__ uint32_t s_hist[NP * kBinCap];
    for (uint32_t k = threadIdx.x; k <= bins; k += kFilmBlock) s_edge[k] = edges[k];
    for (uint32_t k = threadIdx.x; k < NP * bins; k += kFilmBlock) s_hist[k] = 0u;
    __syncthreads();

    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t n_chunks = fs_chunks(npix), n_waves = film_waves();
    const film_src_t<kDev> film = film_src(value, weight, light, sl);
    uint32_t min_inv[NP], max_key[NP], minpos_inv[NP], count[NP][FS_BIN];   // count: the same in every lane
    uint32_t n_included = 0;
#pragma unroll
    for (uint32_t c = 0; c < NP; ++c) {
        min_inv[c] = max_key[c] = minpos_inv[c] = 0u;
#pragma unroll
        for (uint32_t k = 0; k < FS_BIN; ++k) count[c][k] = 0u;
    }
    for (uint64_t chunk = film_first_chunk(); chunk < n_chunks; chunk += n_waves) {
        double d[NP][4];
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint64_t p = chunk_element(chunk, j);
            const bool included = p < npix && (!mask || mask[p] > 0.f);
            float x[NP];
#pragma unroll
            for (uint32_t c = 0; c < NP; ++c) x[c] = 0.f;
            if (included) fs_planes(film, p, C, stokes, s, kLum, flags, x);
            n_included += (uint32_t)__popcll(__ballot(included));
#pragma unroll
            for (uint32_t c = 0; c < NP; ++c) {
                uint32_t bin = 0, cls = FS_BIN + 1;   // (FS_BIN + 1: not an element)
                if (included) {
                    cls = fs_classify(x[c], s_edge, bins, bin);
                    if (cls == FS_BIN) atomicAdd(&s_hist[c * bins + bin], 1u);
                    if (cls != FS_NAN) {
                        const uint32_t key = fs_key(x[c]);
                        min_inv[c] = max(min_inv[c], ~key);
                        max_key[c] = max(max_key[c], key);
                        if (cls >= FS_BELOW) minpos_inv[c] = max(minpos_inv[c], ~key);
                    }
                }
#pragma unroll
                for (uint32_t k = 0; k < FS_BIN; ++k) count[c][k] += (uint32_t)__popcll(__ballot(cls == k));
                d[c][j] = fs_addend(x[c], included);
            }
        }
#pragma unroll
        for (uint32_t c = 0; c < NP; ++c) {
            const double t = chunk_sum(d[c][0], d[c][1], d[c][2], d[c][3]);
            if (lane == 0) sums[c * sums_stride + chunk] = t;
        }
    }
#pragma unroll
    for (uint32_t c = 0; c < NP; ++c) {
        const uint32_t a = wave_max_u32(min_inv[c]), b = wave_max_u32(max_key[c]), m = wave_max_u32(minpos_inv[c]);
        if (lane == 0) {
            if (n_included) atomicAdd(&rec[c].n, (unsigned long long)n_included);
            if (count[c][FS_NAN]) atomicAdd(&rec[c].n_nan, (unsigned long long)count[c][FS_NAN]);
            if (count[c][FS_NEGATIVE]) atomicAdd(&rec[c].n_negative, (unsigned long long)count[c][FS_NEGATIVE]);
            if (count[c][FS_ZERO]) atomicAdd(&rec[c].n_zero, (unsigned long long)count[c][FS_ZERO]);
            if (count[c][FS_BELOW]) atomicAdd(&rec[c].n_below, (unsigned long long)count[c][FS_BELOW]);
            if (count[c][FS_ABOVE]) atomicAdd(&rec[c].n_above, (unsigned long long)count[c][FS_ABOVE]);
            if (a) atomicMax(&rec[c].min_inv, a);
            if (b) atomicMax(&rec[c].max_key, b);
            if (m) atomicMax(&rec[c].minpos_inv, m);
        }
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < NP * bins; k += kFilmBlock)
        if (const uint32_t v = s_hist[k]) atomicAdd(&hist[k], (unsigned long long)v);
}

// ---- k_film_stats_finish: one block per plane ---------------------------------------------------------------------------------------------
// Reduces the plane's chunk sums (film_reduce_levels); then the sum goes into the record and the extrema's keys become floats (NaN where no
// element was met).
__global__ void __launch_bounds__(kFilmBlock) k_film_stats_finish(film_stats_rec_t* __restrict__ rec, double* sums, uint64_t sums_stride, uint64_t n_chunks) {
    const double sum = film_reduce_levels(sums + blockIdx.x * sums_stride, n_chunks);
    if (threadIdx.x == 0) {
        film_stats_rec_t& r = rec[blockIdx.x];
        r.sum = sum;
        r.min_inv = __float_as_uint(fs_unkey(r.min_inv ? ~r.min_inv : 0u));
        r.max_key = __float_as_uint(fs_unkey(r.max_key));
        r.minpos_inv = __float_as_uint(fs_unkey(r.minpos_inv ? ~r.minpos_inv : 0u));
    }
}

template <bool kDev, uint32_t C, bool kLum>
static void film_stats_launch_c(hipStream_t stream, uint32_t blocks, const film_elem_t<kDev>* v, const double* w, const double* l, double sl, uint32_t stokes, uint32_t s, uint32_t flags,
                                const float* mask, uint64_t npix, const float* edges, uint32_t bins, film_stats_rec_t* rec, unsigned long long* hist, double* sums,
                                uint64_t stride) {
    if (bins <= kStatsSmallBins)
        hipLaunchKernelGGL((k_film_stats<kDev, C, kLum, kStatsSmallBins>), dim3(blocks), dim3(kFilmBlock), 0, stream, v, w, l, sl, stokes, s, flags, mask, npix, edges, bins, rec,
                           hist, sums, stride);
    else
        hipLaunchKernelGGL((k_film_stats<kDev, C, kLum, kFsMaxBins>), dim3(blocks), dim3(kFilmBlock), 0, stream, v, w, l, sl, stokes, s, flags, mask, npix, edges, bins, rec, hist,
                           sums, stride);
}
int film_stats_launch(const sensor_t& sn, hipStream_t stream, uint32_t n_cus, const wtgpu_film_source& film, uint32_t s, uint32_t flags, const float* d_mask, const float* d_edges, uint32_t bins, void* d_rec, unsigned long long* d_hist, double* d_sums) {
    const uint64_t npix = (uint64_t)sn.width * sn.height;
    if (npix == 0 || bins > kFsMaxBins) return (int)hipErrorInvalidValue;
    const bool lum = (flags & FS_LUMINANCE) != 0;
    const uint64_t n_chunks = fs_chunks(npix), stride = fs_scratch_len(npix);
    // kStatsBlocksPerCU blocks per CU at most (1920 x 1088: 8160 chunks on 1024 blocks, two per wavefront): each block flushes its histogram once,
    // so more blocks mean more global atomics.
    const uint32_t blocks = film_grid_blocks(npix, n_cus, kStatsBlocksPerCU);
    film_stats_rec_t* rec = static_cast<film_stats_rec_t*>(d_rec);
    if (!film_dispatch(sn.channels, lum, [&](auto c, auto l) {
            film_source_dispatch(film, [&](auto src) {
                film_stats_launch_c<decltype(src)::developed, decltype(c)::value, decltype(l)::value>(stream, blocks, src.first(), src.weight, src.light, src.sl, film_stokes(sn), s,
                                                                                                      flags, d_mask, npix, d_edges, bins, rec, d_hist, d_sums, stride);
            });
        }))
        return (int)hipErrorInvalidValue;
    if (const hipError_t e = hipGetLastError()) return (int)e;
    hipLaunchKernelGGL(k_film_stats_finish, dim3(sn.channels + (lum ? 1u : 0u)), dim3(kFilmBlock), 0, stream, rec, d_sums, stride, n_chunks);
    return (int)hipGetLastError();
}

// ---- the host twin: the same wt/film_stats.h functions on host threads, one task per chunk; the counts are integers and a chunk's sum is one
// thread's, so the result does not depend on the number of threads -----------------------------------------------------------------------------
template <class Src>
static void film_stats_host_of(const sensor_t& sn, const Src& film, uint32_t s, uint32_t flags, const float* mask, const float* edges, uint32_t bins, uint32_t n_threads,
                               void* out_rec, unsigned long long* out_hist) {
    const uint32_t C = sn.channels, stokes = film_stokes(sn), NP = C + ((flags & FS_LUMINANCE) ? 1u : 0u);
    const uint64_t npix = (uint64_t)sn.width * sn.height, n_chunks = fs_chunks(npix), stride = fs_scratch_len(npix);
    film_stats_rec_t* rec = static_cast<film_stats_rec_t*>(out_rec);
    std::memset(rec, 0, NP * sizeof(film_stats_rec_t));
    if (out_hist) std::memset(out_hist, 0, (size_t)NP * bins * sizeof(unsigned long long));
    std::vector<double> sums((size_t)NP * std::max<uint64_t>(stride, 1), 0.0);
    std::mutex merge;
    on_threads(n_chunks, n_threads, [&](auto claim) {
        std::vector<film_stats_rec_t> my(NP, film_stats_rec_t{});
        std::vector<unsigned long long> my_hist((size_t)NP * bins, 0ull);
        double a[kFsMaxPlanes][kFsChunk];
        for (uint64_t chunk = claim(); chunk < n_chunks; chunk = claim()) {
            for (uint32_t i = 0; i < kFsChunk; ++i) {
                const uint64_t p = chunk * kFsChunk + i;
                const bool included = p < npix && (!mask || mask[p] > 0.f);
                float x[kFsMaxPlanes] = {0.f, 0.f, 0.f, 0.f};
                if (included) fs_planes(film, p, C, stokes, s, NP > C, flags, x);
                for (uint32_t c = 0; c < NP; ++c) {
                    a[c][i] = fs_addend(x[c], included);
                    if (!included) continue;
                    film_stats_rec_t& r = my[c];
                    uint32_t bin = 0;
                    const uint32_t cls = fs_classify(x[c], edges, bins, bin);
                    ++r.n;
                    ++*(cls == FS_NAN ? &r.n_nan : cls == FS_NEGATIVE ? &r.n_negative : cls == FS_ZERO ? &r.n_zero : cls == FS_BELOW ? &r.n_below : cls == FS_ABOVE ? &r.n_above : &my_hist[(size_t)c * bins + bin]);
                    if (cls == FS_NAN) continue;
                    const uint32_t key = fs_key(x[c]);
                    r.min_inv = std::max(r.min_inv, ~key);
                    r.max_key = std::max(r.max_key, key);
                    if (cls >= FS_BELOW) r.minpos_inv = std::max(r.minpos_inv, ~key);
                }
            }
            for (uint32_t c = 0; c < NP; ++c) sums[c * stride + chunk] = fs_chunk_sum(a[c]);
        }
        std::lock_guard<std::mutex> lock(merge);
        for (uint32_t c = 0; c < NP; ++c) {
            film_stats_rec_t& r = rec[c];
            r.n += my[c].n, r.n_nan += my[c].n_nan, r.n_negative += my[c].n_negative, r.n_zero += my[c].n_zero, r.n_below += my[c].n_below, r.n_above += my[c].n_above;
            r.min_inv = std::max(r.min_inv, my[c].min_inv);
            r.max_key = std::max(r.max_key, my[c].max_key);
            r.minpos_inv = std::max(r.minpos_inv, my[c].minpos_inv);
        }
        if (out_hist)
            for (size_t k = 0; k < my_hist.size(); ++k) out_hist[k] += my_hist[k];
    });
    // the levels above the chunks, and the keys (k_film_stats_finish)
    for (uint32_t c = 0; c < NP; ++c) {
        film_stats_rec_t& r = rec[c];
        r.sum = fs_reduce_levels(sums.data() + c * stride, n_chunks);
        const float mn = fs_unkey(r.min_inv ? ~r.min_inv : 0u), mx = fs_unkey(r.max_key), mp = fs_unkey(r.minpos_inv ? ~r.minpos_inv : 0u);
        std::memcpy(&r.min_inv, &mn, 4);
        std::memcpy(&r.max_key, &mx, 4);
        std::memcpy(&r.minpos_inv, &mp, 4);
    }
}
void film_stats_host(const sensor_t& sn, const wtgpu_film_source& film, uint32_t s, uint32_t flags, const float* mask, const float* edges, uint32_t bins, uint32_t n_threads,
                     void* out_rec, unsigned long long* out_hist) {
    film_source_dispatch(film, [&](auto src) { film_stats_host_of(sn, src, s, flags, mask, edges, bins, n_threads, out_rec, out_hist); });
}

}   // namespace wtk
