// wave_tracer_amd — exact Euclidean distance transform of a label plane on the device, with the nearest site (see wtgpu_kernels.h for the list of
// kernel translation units): how far each pixel is from the nearest covered pixel, how deep inside its hole it lies, which region is nearest.
// Sites, candidates, the column step and the row step are wt/film_distance.h's; squared distances are integers and ties go to the smaller pixel
// index, so the result depends on no order of execution and device and host twin agree bit for bit.
//
// The phases are separate launches — a kernel boundary is what makes one phase's plain stores visible to the next across the per-XCD L2s:
//   k_dist_columns  one lane per column: dy[y][x] = the signed 16-bit offset to the column's best site row (fact 1 of the header), the number of
//                   sites from ballots, and min |dy| of every 64-column group of every row (one wavefront reduction per row: a wavefront's lanes
//                   ARE one group here, so every minimum is taken once, not once per block of the row pass that reads it)
//   k_dist_rows     one lane per pixel: the minimum over the columns of each column's candidate (fact 2), dist2 and nearest, and (max d², lowest
//                   index) by one 64-bit atomic max per wavefront
// The host twin is at the end of the file.  No render kernel is compiled here.
#include <cstring>

#include "kernels_film.h"
#include "wt/film_distance.h"

namespace wtk {

// what comes back to the host; zeroed before the launches
struct dist_head_t {
    unsigned long long n_sites, max_key;
    uint32_t pad[4];
};
static_assert(sizeof(dist_head_t) == kDistHeadBytes, "dist_head_t");

constexpr uint32_t kDistRowsInFlight = 8;   // k_dist_columns: rows whose loads are issued before the first of them is used
constexpr uint32_t kDistHalo = 128;         // k_dist_rows: columns of the row staged in LDS on either side of the block's own kFilmBlock

WT_D uint32_t wave_min_u32(uint32_t v) {
#pragma unroll
    for (int d = 32; d; d >>= 1) v = min(v, (uint32_t)__shfl_down((int)v, d, 64));
    return v;
}
WT_D unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int d = 32; d; d >>= 1) {
        const unsigned long long o = __shfl_down(v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}

// ---- k_dist_columns: one lane per column, a wavefront per block on 64 consecutive columns ----------------------------------------------------------
// Down: the offset to the nearest site at or above, row by row (dist_col_step); the words of kDistRowsInFlight rows are loaded first — they
// do not depend on each other: the kernel is compiled per (class plane or none, mask or none), so no branch stands between them —, then the chain
// runs over registers.  Up: a site is where the down offset is 0, so only the offsets are read
// again; the offset to the nearest site at or below, the pick of the two (dist_col_pick: a tie goes to the negative offset), and the group's
// min |dy|.  Both loops are counted by the height and wait for nobody.  A lane beyond the width loads and stores nothing and is no site.
template <bool kClasses, bool kMask>
__global__ void __launch_bounds__(64) k_dist_columns(const uint32_t* __restrict__ classes, const float* __restrict__ mask, uint32_t width, uint32_t height, uint32_t invert,
                                                     int16_t* __restrict__ dy, uint16_t* __restrict__ group_min, uint32_t n_groups, dist_head_t* head) {
    const uint32_t lane = threadIdx.x, x = blockIdx.x * 64u + lane;
    const bool valid = x < width;
    uint32_t n_sites = 0;   // (the same in every lane; below 2^31: the sensor's pixels)
    int run = kDistNoDy;
    for (uint32_t y0 = 0; y0 < height; y0 += kDistRowsInFlight) {
        // the rows' words first, without a branch between them (a lane or row outside the plane reads pixel 0 and is no site); dist_site then
        // runs on the registers
        uint32_t klass[kDistRowsInFlight];
        float included[kDistRowsInFlight];
#pragma unroll
        for (uint32_t j = 0; j < kDistRowsInFlight; ++j) {
            const uint64_t p = valid && y0 + j < height ? (uint64_t)(y0 + j) * width + x : 0u;
            klass[j] = kClasses ? classes[p] : 0u;
            included[j] = kMask ? mask[p] : 1.f;
        }
#pragma unroll
        for (uint32_t j = 0; j < kDistRowsInFlight; ++j) {
            if (y0 + j >= height) break;   // (the same in every lane)
            const bool site = valid && dist_site(kClasses ? &klass[j] : nullptr, kMask ? &included[j] : nullptr, 0u, invert != 0u);
            n_sites += (uint32_t)__popcll(__ballot(site));
            run = dist_col_step(run, site, -1);
            if (valid) dy[(uint64_t)(y0 + j) * width + x] = (int16_t)run;
        }
    }
    if (lane == 0u && n_sites) atomicAdd(&head->n_sites, (unsigned long long)n_sites);
    run = kDistNoDy;
    for (uint32_t y1 = height; y1 > 0u; y1 -= min(y1, kDistRowsInFlight)) {   // rows y1 - 1, y1 - 2, ...
        int down[kDistRowsInFlight];
#pragma unroll
        for (uint32_t j = 0; j < kDistRowsInFlight; ++j) down[j] = valid && j < y1 ? (int)dy[(uint64_t)(y1 - 1u - j) * width + x] : kDistNoDy;
#pragma unroll
        for (uint32_t j = 0; j < kDistRowsInFlight; ++j) {
            if (j >= y1) break;   // (the same in every lane)
            const uint32_t y = y1 - 1u - j;
            run = dist_col_step(run, valid && down[j] == 0, +1);
            const int best = dist_col_pick(down[j], run);
            if (valid) dy[(uint64_t)y * width + x] = (int16_t)best;
            const uint32_t m = wave_min_u32(dist_abs_dy(best));
            if (lane == 0u) group_min[(uint64_t)y * n_groups + blockIdx.x] = (uint16_t)m;
        }
    }
}

// ---- k_dist_rows: one lane per pixel; a block on kFilmBlock consecutive columns of one row, a wavefront on one 64-column group of it -----------------
// The row's offsets for the block's columns and kDistHalo on either side are staged in LDS; beyond |dx| = kDistHalo they are read from global memory.
// Near search: each lane takes columns x -+ k for k = 0, 1, ... and keeps the best (d², index) until dist_row_done; the loop is wave-uniform
// (__any) and k stays below the width — its step bound: no column lies further — or, with kGroups, below 64 + 1.
// kGroups (WTGPU_FILM_DISTANCE_GROUPS): beyond |dx| = 64 the lanes that are not done go on group by group, g -+ j for j = 1, 2, ...: a group is
// skipped where for every such lane (distance to its nearer edge)² + (its min |dy|)² cannot reach or tie the lane's best (dist_group_skipped);
// otherwise each lane loads one of its 64 offsets and all lanes take all 64 by shuffles.  A side ends where every lane's edge distance alone is
// out of reach; j stays below the number of groups + 1.  Columns met twice do no harm: a minimum under a total order (fact 2).
// Both forms give the same bits.  No loop waits for another wavefront.
template <bool kGroups>
__global__ void __launch_bounds__(kFilmBlock) k_dist_rows(const int16_t* __restrict__ dy, const uint16_t* __restrict__ group_min, uint32_t width, uint32_t n_groups,
                                                          uint32_t* __restrict__ dist2, uint32_t* __restrict__ nearest, dist_head_t* head) {
    __shared__ int16_t s_dy[kFilmBlock + 2u * kDistHalo];
    const uint32_t y = blockIdx.y, x_block = blockIdx.x * kFilmBlock, x = x_block + threadIdx.x, lane = threadIdx.x & 63u;
    const int16_t* row = dy + (uint64_t)y * width;
    const int x_window = (int)x_block - (int)kDistHalo;   // the window's first column
    for (uint32_t i = threadIdx.x; i < kFilmBlock + 2u * kDistHalo; i += kFilmBlock) {
        const int c = x_window + (int)i;
        s_dy[i] = c >= 0 && c < (int)width ? row[c] : (int16_t)kDistNoDy;
    }
    __syncthreads();
    const bool valid = x < width;
    unsigned long long best = kDistNoKey;
    bool done = !valid;
    // one step of the outward search, the same in every lane; false: every lane of the wavefront is done.  at(c): the offset of column c < width
    auto step = [&](uint32_t k, auto&& at) -> bool {
        done = done || dist_row_done(best, k, x, width);
        if (!__any(!done)) return false;
        if (!done) {
            if (k <= x) dist_row_try(best, at(x - k), x, x - k, y, width);
            if (k > 0u && x + k < width) dist_row_try(best, at(x + k), x, x + k, y, width);
        }
        return true;
    };
    // up to |dx| = kDistHalo every lane's columns lie in the window: LDS reads only; further out global reads only (two loops, so that neither is a
    // load through a generic pointer)
    const uint32_t k_end = kGroups ? 65u : width;   // the step bound
    static_assert(kDistHalo >= 64u, "the group form's near search stays inside the window");
    bool more = true;
    uint32_t k = 0;
    for (; more && k < k_end && k <= kDistHalo; ++k) more = step(k, [&](uint32_t c) { return (int)s_dy[c - (uint32_t)x_window]; });   // (x_window <= c: modular, the window may begin left of column 0)
    if (!kGroups)
        for (; more && k < k_end; ++k) more = step(k, [&](uint32_t c) { return (int)row[c]; });
    if (kGroups) {
        // every column at |dx| <= 64 has been taken by the lanes that are not done
        const uint32_t g = x >> 6;   // (the same in every lane)
        const uint16_t* gmin = group_min + (uint64_t)y * n_groups;
        bool left = true, right = true;
        for (uint32_t j = 1; j <= n_groups && (left || right); ++j) {
            if (left) {
                const bool there = j <= g;
                const uint32_t edge = there ? x - (((g - j) << 6) + 63u) : 0u;   // the group's last column is its nearer edge
                left = there && __any(!done && edge * edge <= dist_key_d2(best));
                if (left && __any(!done && !dist_group_skipped(best, edge, gmin[g - j]))) {
                    const uint32_t c0 = (g - j) << 6;
                    const int mine = (int)row[c0 + lane];   // (a group left of the wavefront's is whole)
#pragma unroll 8
                    for (uint32_t i = 0; i < 64u; ++i) dist_row_try(best, __shfl(mine, (int)i, 64), x, c0 + i, y, width);
                }
            }
            if (right) {
                const bool there = g + j < n_groups;
                const uint32_t edge = there ? ((g + j) << 6) - x : 0u;
                right = there && __any(!done && edge * edge <= dist_key_d2(best));
                if (right && __any(!done && !dist_group_skipped(best, edge, gmin[g + j]))) {
                    const uint32_t c0 = (g + j) << 6;
                    const int mine = c0 + lane < width ? (int)row[c0 + lane] : kDistNoDy;   // (kDistNoDy: no candidate, whatever its column)
#pragma unroll 8
                    for (uint32_t i = 0; i < 64u; ++i) dist_row_try(best, __shfl(mine, (int)i, 64), x, c0 + i, y, width);
                }
            }
        }
    }
    const uint32_t p = y * width + x;
    if (valid) {
        dist2[p] = dist_key_d2(best);
        if (nearest) nearest[p] = dist_key_index(best);
    }
    // (a lane beyond the width holds key 0, below every pixel's: ~p > 0)
    const unsigned long long key = wave_max_u64(valid ? dist_max_key(dist_key_d2(best), p) : 0ull);
    if (lane == 0u) atomicMax(&head->max_key, key);
}

// the scratch of a call in bytes: the offsets (16 bits per pixel), then the groups' minima (16 bits per row and group)
static uint32_t dist_groups(uint32_t width) { return (width + 63u) / 64u; }
static uint64_t dist_dy_bytes(uint64_t npix) { return (npix * sizeof(int16_t) + 15u) & ~(uint64_t)15u; }
uint64_t film_distance_scratch_bytes(uint32_t width, uint32_t height) {
    return dist_dy_bytes((uint64_t)width * height) + (uint64_t)height * dist_groups(width) * sizeof(uint16_t);
}

int film_distance_launch(const sensor_t& sn, hipStream_t stream, uint32_t groups, uint32_t flags, const uint32_t* d_classes, const float* d_mask, uint32_t* d_dist2,
                         uint32_t* d_nearest, void* d_head, void* d_work) {
    const uint32_t W = sn.width, H = sn.height;
    if (W == 0 || H == 0 || W > kDistMaxSide || H > kDistMaxSide || (flags & ~(uint32_t)DIST_INVERT)) return (int)hipErrorInvalidValue;
    const uint32_t n_groups = dist_groups(W);
    dist_head_t* head = static_cast<dist_head_t*>(d_head);
    int16_t* dy = static_cast<int16_t*>(d_work);
    uint16_t* group_min = reinterpret_cast<uint16_t*>(static_cast<unsigned char*>(d_work) + dist_dy_bytes((uint64_t)W * H));
    if (const hipError_t e = hipMemsetAsync(head, 0, sizeof(dist_head_t), stream)) return (int)e;
    const auto columns = d_classes ? (d_mask ? k_dist_columns<true, true> : k_dist_columns<true, false>) : (d_mask ? k_dist_columns<false, true> : k_dist_columns<false, false>);
    hipLaunchKernelGGL(columns, dim3(n_groups), dim3(64), 0, stream, d_classes, d_mask, W, H, flags & DIST_INVERT, dy, group_min, n_groups, head);
    const dim3 grid((W + kFilmBlock - 1u) / kFilmBlock, H), block(kFilmBlock);   // (H <= 32768: within the grid's second dimension)
    if (groups)
        hipLaunchKernelGGL(k_dist_rows<true>, grid, block, 0, stream, dy, group_min, W, n_groups, d_dist2, d_nearest, head);
    else
        hipLaunchKernelGGL(k_dist_rows<false>, grid, block, 0, stream, dy, group_min, W, n_groups, d_dist2, d_nearest, head);
    return (int)hipGetLastError();
}

// ---- the host twin: the same column step over the columns, the same outward search over the rows.  Integers and a total order: the result does
// not depend on the number of threads ------------------------------------------------------------------------------------------------------------
void film_distance_host(const sensor_t& sn, uint32_t flags, const uint32_t* classes, const float* mask, uint32_t n_threads, uint32_t* dist2, uint32_t* nearest,
                        unsigned long long* info) {
    const uint32_t W = sn.width, H = sn.height;
    const bool invert = (flags & DIST_INVERT) != 0;
    std::vector<int16_t> dy((size_t)W * H);
    std::atomic<unsigned long long> n_sites{0};
    on_threads(W, n_threads, [&](auto claim) {
        unsigned long long mine = 0;
        for (uint64_t x = claim(); x < W; x = claim()) {
            int run = kDistNoDy;
            for (uint32_t y = 0; y < H; ++y) {
                const bool site = dist_site(classes, mask, (uint64_t)y * W + x, invert);
                mine += site ? 1u : 0u;
                dy[(size_t)y * W + x] = (int16_t)(run = dist_col_step(run, site, -1));
            }
            run = kDistNoDy;
            for (uint32_t y = H; y-- > 0u;) {
                int16_t& d = dy[(size_t)y * W + x];
                run = dist_col_step(run, d == 0, +1);
                d = (int16_t)dist_col_pick(d, run);
            }
        }
        n_sites += mine;
    });
    std::mutex merge;
    unsigned long long max_key = 0;
    on_threads(H, n_threads, [&](auto claim) {
        unsigned long long my_max = 0;
        for (uint64_t y = claim(); y < H; y = claim()) {
            const int16_t* row = dy.data() + (size_t)y * W;
            for (uint32_t x = 0; x < W; ++x) {
                unsigned long long best = kDistNoKey;
                for (uint32_t k = 0; k < W && !dist_row_done(best, k, x, W); ++k) {   // (the step bound is the device's)
                    if (k <= x) dist_row_try(best, row[x - k], x, x - k, (uint32_t)y, W);
                    if (k > 0u && x + k < W) dist_row_try(best, row[x + k], x, x + k, (uint32_t)y, W);
                }
                const uint32_t p = (uint32_t)y * W + x;
                dist2[p] = dist_key_d2(best);
                if (nearest) nearest[p] = dist_key_index(best);
                my_max = std::max(my_max, dist_max_key(dist_key_d2(best), p));
            }
        }
        std::lock_guard<std::mutex> lock(merge);
        max_key = std::max(max_key, my_max);
    });
    info[0] = n_sites.load();
    info[1] = (uint32_t)~(uint32_t)max_key;   // argmax
    info[2] = max_key >> 32;                  // max_dist2
}

}   // namespace wtk
