// wave_tracer_amd — zonal film statistics on the device (see wtgpu_kernels.h for the list of kernel translation units): one pass over a film under a
// u32 label plane (first_hit's SHAPE, line_of_sight's NEAREST, distance rings, block cells) that keeps a statistics record per (zone, plane) —
// what a masked wtgpu_film_stats_device call per class used to cost.  Elements, planes, membership, classes and extrema are the film statistics'
// (wt/film_stats.h); the sum is exact and order-free (wt/film_zonal.h: nine integer words per (zone, plane), rounded once), so atomics may deliver
// the addends in any order and device and host twin still agree on every field bit for bit.  k_film_zonal accumulates, in one of two forms that
// must agree; k_film_zonal_finish rounds the sums and turns the keys into floats; k_film_zonal_paint writes every pixel's zone mean as a
// developed film.  The host twin is at the end of the file.  No render kernel is compiled here.
#include <cstring>
#include <mutex>

#include "kernels_film.h"
#include "wt/film_zonal.h"

namespace wtk {

// Each block flushes its table once (LDS form), so more blocks mean more global atomics: the film statistics' grid.
constexpr uint32_t kZonalBlocksPerCU = 4;
// LDS form: taken wherever the table fits what a launch may ask for (WTGPU_FILM_ZONAL_LDS = 1, the default).  Measured (tools/bench_film_zonal.py,
// docs/FEATURES.md): wherever it fits, the LDS form is 7 to 165 times faster than the global form, whose lanes meet in a few words of global
// memory — also at 41 KB and 64.8 KB of table, where three blocks and two blocks share a CU's 160 KB of LDS — so there is no smaller budget.
constexpr uint32_t kZonalLdsMax = 64u << 10;

// Dynamic LDS of a launch: the edge table (both forms; padded to whole 8 bytes), and for the LDS form a table of `slots` = n_zones x planes
// entries of nine u64 words, seven u32 counts, two keys and the zone's bins.
inline uint64_t zonal_lds_bytes(uint64_t slots, uint32_t bins) {
    return (((uint64_t)bins + 2u) & ~1ull) * 4u + slots * (kFzWords * 8u + FZ_COUNTS * 4u + 2u * 4u + (uint64_t)bins * 4u);
}

// Where a lane's atomics go: the block's table in LDS (u32 counts and bins: a block meets fewer than 2^31 elements) or the scratch in global memory.
template <bool kLds>
struct zonal_table_t {
    unsigned long long* w;     // LDS: [slots][kFzWords]
    uint32_t *cnt, *key, *bin; // LDS: [slots][FZ_COUNTS], [slots][2], [slots][bins]
    film_zonal_slot_t* slot;   // global
    unsigned long long* hist;  // global: [slots][bins]
    uint32_t bins;
    WT_D void word(uint32_t s, uint32_t k, unsigned long long v) const {
        if constexpr (kLds) atomicAdd(&w[s * kFzWords + k], v);
        else atomicAdd(&slot[s].w[k], v);
    }
    WT_D void count(uint32_t s, uint32_t i, uint32_t v) const {
        if constexpr (kLds) atomicAdd(&cnt[s * FZ_COUNTS + i], v);
        else atomicAdd(&slot[s].count[i], (unsigned long long)v);
    }
    WT_D void keys(uint32_t s, uint32_t min_inv, uint32_t max_key) const {
        if constexpr (kLds) atomicMax(&key[2 * s], min_inv), atomicMax(&key[2 * s + 1], max_key);
        else atomicMax(&slot[s].min_inv, min_inv), atomicMax(&slot[s].max_key, max_key);
    }
    WT_D void bin_add(uint32_t s, uint32_t b) const {
        if constexpr (kLds) atomicAdd(&bin[(uint64_t)s * bins + b], 1u);
        else atomicAdd(&hist[(uint64_t)s * bins + b], 1ull);
    }
};

// ---- k_film_zonal: a film (f64 accumulators or a developed f32 film), zones [H][W] u32 -> slots, histogram, n_outside ----------------------------
// One lane per pixel in the chunk geometry of kernels_film.h.  The loads are conditional on membership: the zone of a pixel the mask excludes and
// the films of a pixel outside every zone are not read.  A wavefront whose member lanes share one zone (labels from maps are spatially coherent)
// forms its counts from ballots and its extrema from a wavefront reduction, one atomic each: zeros of an unlit background would otherwise all hit
// one word.  The words of the sum and the bins are per-lane atomics in both cases; a zero issues none.
// kLds: the atomics go to the block's table in LDS, flushed at the end with 64-bit global atomics and atomicMax, non-zero entries only; else
// straight to global memory.  Both forms add the same integers, so they agree bit for bit.
template <bool kDev, uint32_t C, bool kLum, bool kLds>
__global__ void __launch_bounds__(kFilmBlock) k_film_zonal(const film_elem_t<kDev>* __restrict__ value, const double* __restrict__ weight, const double* __restrict__ light,
                                                           double sl, uint32_t stokes, uint32_t s, uint32_t flags, const uint32_t* __restrict__ zones,
                                                           const float* __restrict__ mask, uint64_t npix, const float* __restrict__ edges, uint32_t bins, uint32_t n_zones,
                                                           film_zonal_slot_t* __restrict__ slots, unsigned long long* __restrict__ hist,
                                                           unsigned long long* __restrict__ n_outside) {
    constexpr uint32_t NP = C + (kLum ? 1u : 0u);
    extern __shared__ unsigned long long s_dyn[];
    const uint32_t n_slots = kLds ? n_zones * NP : 0u;
    unsigned long long* s_w = s_dyn;
    float* s_edge = reinterpret_cast<float*>(s_w + (uint64_t)n_slots * kFzWords);
    uint32_t* s_cnt = reinterpret_cast<uint32_t*>(s_edge + (((uint64_t)bins + 2u) & ~1ull));
    uint32_t* s_key = s_cnt + (uint64_t)n_slots * FZ_COUNTS;
    uint32_t* s_bin = s_key + (uint64_t)n_slots * 2u;
    const uint64_t n_small = (uint64_t)n_slots * (FZ_COUNTS + 2u + bins);   // counts, keys and bins lie in a row
    for (uint32_t k = threadIdx.x; k <= bins; k += kFilmBlock) s_edge[k] = edges[k];
    for (uint64_t k = threadIdx.x; k < (uint64_t)n_slots * kFzWords; k += kFilmBlock) s_w[k] = 0ull;
    for (uint64_t k = threadIdx.x; k < n_small; k += kFilmBlock) s_cnt[k] = 0u;
    __syncthreads();

    const zonal_table_t<kLds> tab{s_w, s_cnt, s_key, s_bin, slots, hist, bins};
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t n_chunks = fs_chunks(npix), n_waves = film_waves();
    const film_src_t<kDev> film = film_src(value, weight, light, sl);
    uint32_t n_out = 0;   // the same in every lane
    for (uint64_t chunk = film_first_chunk(); chunk < n_chunks; chunk += n_waves) {
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint64_t p = chunk_element(chunk, j);
            const bool included = p < npix && (!mask || mask[p] > 0.f);
            const uint32_t z = included ? zones[p] : 0xffffffffu;
            const bool member = included && z < n_zones;
            n_out += (uint32_t)__popcll(__ballot(included && !member));
            const unsigned long long members = __ballot(member);
            if (!members) continue;   // (the same in every lane)
            float x[NP];
#pragma unroll
            for (uint32_t c = 0; c < NP; ++c) x[c] = 0.f;
            if (member) fs_planes(film, p, C, stokes, s, kLum, flags, x);
            const uint32_t z0 = (uint32_t)__shfl((int)z, __ffsll((long long)members) - 1, 64);
            const bool one_zone = __ballot(member && z != z0) == 0ull;
#pragma unroll
            for (uint32_t c = 0; c < NP; ++c) {
                uint32_t bin = 0, cls = FS_BIN + 1, key = 0;   // (FS_BIN + 1: not an element)
                bool inf = false;
                if (member) {
                    cls = fs_classify(x[c], s_edge, bins, bin);
                    inf = fz_inf(x[c]);
                    if (cls != FS_NAN) key = fs_key(x[c]);
                }
                if (one_zone) {
                    const uint32_t slot = z0 * NP + c;
                    uint32_t cnt[FZ_COUNTS];
                    cnt[FZ_N] = (uint32_t)__popcll(members);
                    cnt[FZ_INF] = (uint32_t)__popcll(__ballot(inf));
#pragma unroll
                    for (uint32_t k = 0; k < FS_BIN; ++k) cnt[fz_count_of(k)] = (uint32_t)__popcll(__ballot(cls == k));
                    const uint32_t a = wave_max_u32(key ? ~key : 0u), b = wave_max_u32(key);
                    if (lane == 0) {
#pragma unroll
                        for (uint32_t k = 0; k < FZ_COUNTS; ++k)
                            if (cnt[k]) tab.count(slot, k, cnt[k]);
                        if (b) tab.keys(slot, a, b);
                    }
                } else if (member) {
                    const uint32_t slot = z * NP + c;
                    tab.count(slot, FZ_N, 1u);
                    if (cls < FS_BIN) tab.count(slot, fz_count_of(cls), 1u);
                    if (inf) tab.count(slot, FZ_INF, 1u);
                    if (key) tab.keys(slot, ~key, key);
                }
                if (member) {
                    const uint32_t slot = z * NP + c;
                    if (cls == FS_BIN) tab.bin_add(slot, bin);
                    uint32_t k;
                    unsigned long long lo, hi;
                    if (fz_finite(x[c]) && fz_split(x[c], k, lo, hi)) {
                        tab.word(slot, k, lo);
                        if (hi) tab.word(slot, k + 1u, hi);
                    }
                }
            }
        }
    }
    if (lane == 0 && n_out) atomicAdd(n_outside, (unsigned long long)n_out);
    if constexpr (kLds) {
        __syncthreads();
        for (uint64_t k = threadIdx.x; k < (uint64_t)n_slots * kFzWords; k += kFilmBlock)
            if (const unsigned long long v = s_w[k]) atomicAdd(&slots[k / kFzWords].w[k % kFzWords], v);
        for (uint64_t k = threadIdx.x; k < (uint64_t)n_slots * FZ_COUNTS; k += kFilmBlock)
            if (const uint32_t v = s_cnt[k]) atomicAdd(&slots[k / FZ_COUNTS].count[k % FZ_COUNTS], (unsigned long long)v);
        for (uint32_t k = threadIdx.x; k < n_slots; k += kFilmBlock)
            if (const uint32_t b = s_key[2 * k + 1]) atomicMax(&slots[k].min_inv, s_key[2 * k]), atomicMax(&slots[k].max_key, b);
        for (uint64_t k = threadIdx.x; k < (uint64_t)n_slots * bins; k += kFilmBlock)
            if (const uint32_t v = s_bin[k]) atomicAdd(&hist[k], (unsigned long long)v);
    }
}

// ---- k_film_zonal_finish: one thread per (zone, plane); every field of the record is written ------------------------------------------------------
__global__ void __launch_bounds__(kFilmBlock) k_film_zonal_finish(const film_zonal_slot_t* __restrict__ slots, uint32_t n_slots, film_zonal_rec_t* __restrict__ rec) {
    const uint32_t i = blockIdx.x * kFilmBlock + threadIdx.x;
    if (i < n_slots) rec[i] = fz_finish(slots[i]);
}

// ---- k_film_zonal_paint: one lane per element of paint [H][W][planes] ------------------------------------------------------------------------------
__global__ void __launch_bounds__(kFilmBlock) k_film_zonal_paint(const uint32_t* __restrict__ zones, const float* __restrict__ mask, uint64_t npix, uint32_t planes, uint32_t n_zones,
                                                                 const film_zonal_rec_t* __restrict__ rec, float* __restrict__ paint) {
    const uint64_t e = (uint64_t)blockIdx.x * kFilmBlock + threadIdx.x;
    if (e >= npix * planes) return;
    const uint64_t p = e / planes;
    const uint32_t c = (uint32_t)(e % planes);
    float v = 0.f;
    if (!mask || mask[p] > 0.f) {
        const uint32_t z = zones[p];
        if (z < n_zones) v = fz_paint(rec[(uint64_t)z * planes + c]);
    }
    paint[e] = v;
}

bool film_zonal_lds_fits(uint32_t n_zones, uint32_t planes, uint32_t bins) { return zonal_lds_bytes((uint64_t)n_zones * planes, bins) <= kZonalLdsMax; }

template <bool kDev, uint32_t C, bool kLum>
static void film_zonal_launch_c(hipStream_t stream, uint32_t blocks, bool lds, const film_elem_t<kDev>* v, const double* w, const double* l, double sl, uint32_t stokes, uint32_t s,
                                uint32_t flags, const uint32_t* zones, const float* mask, uint64_t npix, const float* edges, uint32_t bins, uint32_t n_zones,
                                film_zonal_slot_t* slots, unsigned long long* hist, unsigned long long* n_outside) {
    constexpr uint32_t NP = C + (kLum ? 1u : 0u);
    if (lds)
        hipLaunchKernelGGL((k_film_zonal<kDev, C, kLum, true>), dim3(blocks), dim3(kFilmBlock), (size_t)zonal_lds_bytes((uint64_t)n_zones * NP, bins), stream, v, w, l, sl, stokes, s,
                           flags, zones, mask, npix, edges, bins, n_zones, slots, hist, n_outside);
    else
        hipLaunchKernelGGL((k_film_zonal<kDev, C, kLum, false>), dim3(blocks), dim3(kFilmBlock), (size_t)zonal_lds_bytes(0, bins), stream, v, w, l, sl, stokes, s, flags, zones, mask,
                           npix, edges, bins, n_zones, slots, hist, n_outside);
}
int film_zonal_launch(const sensor_t& sn, hipStream_t stream, uint32_t n_cus, const wtgpu_film_source& film, uint32_t s, uint32_t flags, const uint32_t* d_zones, const float* d_mask,
                      const float* d_edges, uint32_t bins, uint32_t n_zones, uint32_t lds_form, uint32_t max_blocks, void* d_slots, unsigned long long* d_hist,
                      unsigned long long* d_outside, void* d_rec, float* d_paint) {
    const uint64_t npix = (uint64_t)sn.width * sn.height;
    if (npix == 0 || npix >= kFzMaxPixels || bins > kFsMaxBins || n_zones == 0 || n_zones > kFzMaxZones || (uint64_t)n_zones * bins > kFzMaxZoneBins) return (int)hipErrorInvalidValue;
    const bool lum = (flags & FS_LUMINANCE) != 0;
    const uint32_t planes = sn.channels + (lum ? 1u : 0u), n_slots = n_zones * planes;
    // lds_form: the caller's choice (wtgpu_film_zonal_device: WTGPU_FILM_ZONAL_LDS and film_zonal_lds_fits); a table that does not fit is refused here
    const bool lds = lds_form != 0;
    if (lds && !film_zonal_lds_fits(n_zones, planes, bins)) return (int)hipErrorInvalidValue;
    // max_blocks (WTGPU_FILM_ZONAL_BLOCKS): 0, or a cap on the grid — a wavefront then takes more chunks (a film has fewer than 2^31 pixels, so
    // neither a block's u32 counts nor a wavefront's n_out overflow even with one block)
    uint32_t blocks = film_grid_blocks(npix, n_cus, kZonalBlocksPerCU);
    if (max_blocks) blocks = std::min(blocks, max_blocks);
    film_zonal_slot_t* slots = static_cast<film_zonal_slot_t*>(d_slots);
    film_zonal_rec_t* rec = static_cast<film_zonal_rec_t*>(d_rec);
    if (!film_dispatch(sn.channels, lum, [&](auto c, auto l) {
            film_source_dispatch(film, [&](auto src) {
                film_zonal_launch_c<decltype(src)::developed, decltype(c)::value, decltype(l)::value>(stream, blocks, lds, src.first(), src.weight, src.light, src.sl, film_stokes(sn), s,
                                                                                                      flags, d_zones, d_mask, npix, d_edges, bins, n_zones, slots, d_hist, d_outside);
            });
        }))
        return (int)hipErrorInvalidValue;
    if (const hipError_t e = hipGetLastError()) return (int)e;
    hipLaunchKernelGGL(k_film_zonal_finish, dim3((n_slots + kFilmBlock - 1) / kFilmBlock), dim3(kFilmBlock), 0, stream, slots, n_slots, rec);
    if (const hipError_t e = hipGetLastError()) return (int)e;
    if (d_paint) {
        const uint64_t n_elem = npix * planes;   // below 2^33: fewer than 2^25 blocks
        hipLaunchKernelGGL(k_film_zonal_paint, dim3((uint32_t)((n_elem + kFilmBlock - 1) / kFilmBlock)), dim3(kFilmBlock), 0, stream, d_zones, d_mask, npix, planes, n_zones, rec, d_paint);
    }
    return (int)hipGetLastError();
}

// ---- the host twin: the same wt/film_zonal.h functions on host threads, one task per chunk, a private table per thread; the tables are merged
// by integer addition and max, so the result does not depend on the number of threads ------------------------------------------------------------
template <class Src>
static void film_zonal_host_of(const sensor_t& sn, const Src& film, uint32_t s, uint32_t flags, const uint32_t* zones, const float* mask, const float* edges, uint32_t bins,
                               uint32_t n_zones, uint32_t n_threads, void* out_rec, unsigned long long* out_hist, unsigned long long* out_outside, float* paint) {
    const uint32_t C = sn.channels, stokes = film_stokes(sn), NP = C + ((flags & FS_LUMINANCE) ? 1u : 0u);
    const uint64_t npix = (uint64_t)sn.width * sn.height, n_chunks = fs_chunks(npix);
    const size_t n_slots = (size_t)n_zones * NP;
    film_zonal_rec_t* rec = static_cast<film_zonal_rec_t*>(out_rec);
    std::vector<film_zonal_slot_t> all(n_slots, film_zonal_slot_t{});
    if (out_hist) std::memset(out_hist, 0, n_slots * bins * sizeof(unsigned long long));
    unsigned long long outside = 0;
    // a thread's private table is as large as the result: no more threads than 256 MB of tables
    const size_t table_bytes = n_slots * (sizeof(film_zonal_slot_t) + (size_t)bins * sizeof(unsigned long long));
    if (n_threads == 0) n_threads = std::max(1u, std::thread::hardware_concurrency());
    n_threads = (uint32_t)std::max<size_t>(1, std::min<size_t>(n_threads, ((size_t)256 << 20) / std::max<size_t>(table_bytes, 1)));
    std::mutex merge;
    on_threads(n_chunks, n_threads, [&](auto claim) {
        std::vector<film_zonal_slot_t> my(n_slots, film_zonal_slot_t{});
        std::vector<unsigned long long> my_hist(n_slots * bins, 0ull);
        unsigned long long my_outside = 0;
        for (uint64_t chunk = claim(); chunk < n_chunks; chunk = claim()) {
            for (uint32_t i = 0; i < kFsChunk; ++i) {
                const uint64_t p = chunk * kFsChunk + i;
                if (!(p < npix && (!mask || mask[p] > 0.f))) continue;
                const uint32_t z = zones[p];
                if (z >= n_zones) {
                    ++my_outside;
                    continue;
                }
                float x[kFsMaxPlanes] = {0.f, 0.f, 0.f, 0.f};
                fs_planes(film, p, C, stokes, s, NP > C, flags, x);
                for (uint32_t c = 0; c < NP; ++c) {
                    const size_t slot = (size_t)z * NP + c;
                    film_zonal_slot_t& r = my[slot];
                    uint32_t bin = 0;
                    const uint32_t cls = fs_classify(x[c], edges, bins, bin);
                    ++r.count[FZ_N];
                    if (cls < FS_BIN) ++r.count[fz_count_of(cls)];
                    else ++my_hist[slot * bins + bin];
                    if (fz_inf(x[c])) ++r.count[FZ_INF];
                    if (cls == FS_NAN) continue;
                    const uint32_t key = fs_key(x[c]);
                    r.min_inv = std::max(r.min_inv, ~key);
                    r.max_key = std::max(r.max_key, key);
                    if (fz_finite(x[c])) fz_add(r.w, x[c]);
                }
            }
        }
        std::lock_guard<std::mutex> lock(merge);
        outside += my_outside;
        for (size_t k = 0; k < n_slots; ++k) {
            film_zonal_slot_t& r = all[k];
            for (uint32_t i = 0; i < kFzWords; ++i) r.w[i] += my[k].w[i];
            for (uint32_t i = 0; i < FZ_COUNTS; ++i) r.count[i] += my[k].count[i];
            r.min_inv = std::max(r.min_inv, my[k].min_inv);
            r.max_key = std::max(r.max_key, my[k].max_key);
        }
        if (out_hist)
            for (size_t k = 0; k < my_hist.size(); ++k) out_hist[k] += my_hist[k];
    });
    // the sums' one rounding and the keys (k_film_zonal_finish), the painted film (k_film_zonal_paint)
    for (size_t k = 0; k < n_slots; ++k) rec[k] = fz_finish(all[k]);
    *out_outside = outside;
    if (paint)
        on_threads(n_chunks, n_threads, [&](auto claim) {
            for (uint64_t chunk = claim(); chunk < n_chunks; chunk = claim())
                for (uint64_t p = chunk * kFsChunk; p < std::min(npix, (chunk + 1) * kFsChunk); ++p) {
                    const bool member = (!mask || mask[p] > 0.f) && zones[p] < n_zones;
                    for (uint32_t c = 0; c < NP; ++c) paint[p * NP + c] = member ? fz_paint(rec[(size_t)zones[p] * NP + c]) : 0.f;
                }
        });
}
void film_zonal_host(const sensor_t& sn, const wtgpu_film_source& film, uint32_t s, uint32_t flags, const uint32_t* zones, const float* mask, const float* edges, uint32_t bins,
                     uint32_t n_zones, uint32_t n_threads, void* out_rec, unsigned long long* out_hist, unsigned long long* out_outside, float* paint) {
    film_source_dispatch(film, [&](auto src) { film_zonal_host_of(sn, src, s, flags, zones, mask, edges, bins, n_zones, n_threads, out_rec, out_hist, out_outside, paint); });
}

}   // namespace wtk
