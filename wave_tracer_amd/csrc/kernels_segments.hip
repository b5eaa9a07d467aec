// wave_tracer_amd — connected segments of a label plane on the device (see wtgpu_kernels.h for the list of kernel translation units): which REGION
// a pixel lies in, where the id maps and zone planes say which CLASS — coverage holes, the shadow behind one building, one visible fragment of a
// shape.  Members, links and the record are wt/film_segments.h's; a segment is a connected component of the link graph, named by its smallest
// pixel index, and kept segments are numbered in ascending order of that index: the result depends on no order of execution, there is no
// floating-point arithmetic, and device and host twin agree bit for bit.
//
// The phases are separate launches — a kernel boundary is what makes one phase's plain stores visible to the next across the per-XCD L2s:
//   k_seg_runs     parent[p] = the start of p's horizontal run within the wavefront's 64 consecutive pixels (one ballot, no atomics)
//   k_seg_merge    union-find over the links the runs did not see: the only phase where wavefronts race
//                  (WTGPU_FILM_SEGMENTS_TILED=1 takes k_seg_tile + k_seg_border in place of these two: a tile labelled in LDS, then the tile borders)
//   k_seg_roots    root[p] = find(p) into a second array (parent is only read), area[root] += 1
//   k_seg_count / k_seg_scan / k_seg_number   an exclusive prefix sum over the kept roots in pixel order: their ids
//   k_seg_relabel  segments[p] = id[root[p]], the counts, the records of the first max_records segments
// All per-pixel passes run in the chunk geometry of kernels_film.h, where lane l of a load holds pixel 64 m + l.  The host twin is at the end of
// the file.  No render kernel is compiled here.
#include <cstring>

#include "kernels_film.h"
#include "wt/film_segments.h"

namespace wtk {

constexpr uint32_t kSegBlocksPerCU = 8;

// what comes back to the host ahead of the records; zeroed before the launches
struct seg_head_t {
    unsigned long long n_segments, n_dropped, n_members, n_dropped_pixels;
    uint32_t overflow, pad[3];
};
static_assert(sizeof(seg_head_t) == kSegHeadBytes, "seg_head_t");

// ---- find: up the parents to the root ---------------------------------------------------------------------------------------------------------
// Invariant of parent[]: parent[x] <= x, and parent[x] lies in x's component; a root has parent[x] == x.  `load(i)` reads parent[i].  At most
// `bound` loads (a chain of distinct, falling indices below n needs no more than n); a chain that is longer, or a parent above its child (which
// no phase writes), sets `overflow` and ends the walk where it is — always at an index below n.  A bug ends as a refusal, never as a hung card.
template <class Load>
WT_HD uint32_t seg_find(const Load& load, uint32_t x, uint32_t bound, bool& overflow) {
    for (uint32_t step = 0; step < bound; ++step) {
        const uint32_t up = load(x);
        if (up == x) return x;
        if (up > x) break;
        x = up;
    }
    overflow = true;
    return x;
}
struct seg_plain_load_t {
    const uint32_t* parent;
    WT_HD uint32_t operator()(uint32_t i) const { return parent[i]; }
};
// Inside k_seg_merge other wavefronts' atomics change parent[] and the XCDs' L2s are not coherent: a relaxed agent-scope load bypasses this CU's
// L1, but may still return an older value.  By the invariant an older value is still an ancestor of x, so a walk over stale values ends at an
// ancestor — not necessarily the root — and the atomic in seg_union decides.
struct seg_racing_load_t {
    const uint32_t* parent;
    WT_D uint32_t operator()(uint32_t i) const { return __hip_atomic_load(parent + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};

// A tile's parents in LDS while its wavefronts race: LDS is one memory for the block, so the load is merely kept from being hoisted or reused.
struct seg_lds_load_t {
    const uint32_t* parent;
    WT_D uint32_t operator()(uint32_t i) const { return __hip_atomic_load(parent + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
};

// ---- union of the components of a and b (both members, below n) ----------------------------------------------------------------------------------
// atomicMin on the larger ancestor towards the smaller.  If the atomic returns the larger ancestor itself it was a root and now hangs below the
// smaller: done.  If it returns something else, `old` < a, then a had got a parent in the meantime: parent[a] is now min(old, b), both of which
// lie in the united component, and what is left to unite is old with b — strictly smaller indices, so the loop ends by its own atomics and
// waits for nobody.  The step bound is the pixel count; hitting it, or a walk that did, sets the overflow word and leaves.
// Load: how racing parents are read — seg_racing_load_t in global memory, seg_lds_load_t in a tile's LDS (n is then the tile's pixel count).
template <class Load>
WT_D void seg_union(uint32_t* parent, uint32_t a, uint32_t b, uint32_t n, uint32_t* overflow_word) {
    const Load load{parent};
    bool overflow = false;
    for (uint32_t step = 0; step < n; ++step) {
        a = seg_find(load, a, n, overflow);
        b = seg_find(load, b, n, overflow);
        if (overflow) break;
        if (a == b) return;
        if (a < b) {
            const uint32_t t = a;
            a = b, b = t;
        }
        const uint32_t old = atomicMin(parent + a, b);
        if (old == a) return;
        if (old > a) {   // (no phase writes this)
            overflow = true;
            break;
        }
        a = old;
    }
    atomicOr(overflow_word, 1u);
}

// how many of a load's roots (k_seg_roots) or ids (k_seg_relabel) a wavefront gathers by ballots and reductions before it falls back to one atomic per run
constexpr uint32_t kSegLeaders = 2;

// the length of the run of lanes that starts at this lane, from the ballot of the lanes that start one (this lane's bit is set)
WT_D uint32_t seg_run_length(unsigned long long heads, uint32_t lane) {
    const unsigned long long rest = lane == 63u ? 0ull : heads >> (lane + 1u);
    return rest ? (uint32_t)__ffsll((long long)rest) : 64u - lane;
}

// ---- k_seg_runs: one lane per pixel; no atomics ----------------------------------------------------------------------------------------------------
// parent[p] = the first pixel of p's horizontal run within the 64 consecutive pixels of the load: one ballot of "linked to the left neighbour"
// (false in lane 0, whose left neighbour another load holds, and at x = 0: rows do not wrap), and the highest clear bit at or below the lane.
// A pixel that is no member gets kSegNone.
__global__ void __launch_bounds__(kFilmBlock) k_seg_runs(const uint32_t* __restrict__ classes, const float* __restrict__ mask, uint32_t npix, uint32_t width,
                                                         uint32_t* __restrict__ parent) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t n_chunks = fs_chunks(npix), n_waves = film_waves();
    for (uint64_t chunk = film_first_chunk(); chunk < n_chunks; chunk += n_waves) {
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint64_t p = chunk_element(chunk, j);
            const bool in = p < npix;
            const uint32_t c = in ? seg_class(classes, mask, p) : kSegNone;
            const uint32_t c_left = (uint32_t)__shfl_up((int)c, 1, 64);
            const bool linked = lane > 0u && in && (uint32_t)p % width != 0u && seg_linked(c, c_left);
            const unsigned long long starts = ~__ballot(linked) & (~0ull >> (63u - lane));   // (bit 0 is always set)
            const uint32_t start = 63u - (uint32_t)__clzll((long long)starts);
            if (in) parent[p] = c == kSegNone ? kSegNone : (uint32_t)p - (lane - start);
        }
    }
}

// ---- k_seg_merge: the links k_seg_runs did not see ---------------------------------------------------------------------------------------------------
// The left link of lane 0 of each load, and the links to the row above.  A link is skipped where other links, which are made or implied in turn,
// already join its two ends (c = the pixel's class; "linked" = a member of class c):
//   up (p, p - W)            skipped where p - 1 and p - W - 1 are linked too: p ~ p - 1 is a left link (never skipped), p - 1 ~ p - W - 1 is the up link
//                            of p - 1 (made, or skipped by this rule at x - 1: by induction on x it holds, at x = 0 nothing is skipped), and
//                            p - W - 1 ~ p - W is a left link of the row above.
//   up-left (p, p - W - 1)   skipped where p - W is linked (p ~ p - W is the up link, p - W ~ p - W - 1 a left link) or p - 1 is (p ~ p - 1 a left
//                            link, p - 1 ~ p - W - 1 the up link of p - 1).
//   up-right (p, p - W + 1)  skipped where p - W is linked (p ~ p - W, p - W ~ p - W + 1 a left link) or p + 1 is (p ~ p + 1 the left link of p + 1,
//                            p + 1 ~ p - W + 1 its up link).
// No chain of implications passes through a diagonal link, so none is circular.
template <bool kDiagonal>
__global__ void __launch_bounds__(kFilmBlock) k_seg_merge(const uint32_t* __restrict__ classes, const float* __restrict__ mask, uint32_t npix, uint32_t width,
                                                          uint32_t* parent, uint32_t* overflow_word) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t n_chunks = fs_chunks(npix), n_waves = film_waves();
    for (uint64_t chunk = film_first_chunk(); chunk < n_chunks; chunk += n_waves) {
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint64_t p64 = chunk_element(chunk, j);
            if (p64 >= npix) continue;
            const uint32_t p = (uint32_t)p64, c = seg_class(classes, mask, p);
            if (c == kSegNone) continue;
            const uint32_t x = p % width;
            const bool has_left = x > 0u, has_up = p >= width;
            const bool left = has_left && seg_linked(c, seg_class(classes, mask, p - 1u));
            if (left && lane == 0u) seg_union<seg_racing_load_t>(parent, p, p - 1u, npix, overflow_word);
            if (!has_up) continue;
            const bool up = seg_linked(c, seg_class(classes, mask, p - width));
            const bool up_left = has_left && seg_linked(c, seg_class(classes, mask, p - width - 1u));
            if (up) {
                if (!(left && up_left)) seg_union<seg_racing_load_t>(parent, p, p - width, npix, overflow_word);
            } else if (kDiagonal) {
                if (up_left && !left) seg_union<seg_racing_load_t>(parent, p, p - width - 1u, npix, overflow_word);
                if (x + 1u < width && seg_linked(c, seg_class(classes, mask, p - width + 1u)) && !seg_linked(c, seg_class(classes, mask, p + 1u)))
                    seg_union<seg_racing_load_t>(parent, p, p - width + 1u, npix, overflow_word);
            }
        }
    }
}

// ---- the tiled form of the two kernels above (WTGPU_FILM_SEGMENTS_TILED) ----------------------------------------------------------------------------
// k_seg_tile: a block labels a tile of kSegTileW x kSegTileH pixels in LDS.  Each of the four wavefronts takes every fourth row of the tile, a lane
// per pixel: the same runs as k_seg_runs (one ballot per row), then the links to the row above WITHIN the tile by the same union, with ds_min_u32
// for the atomic, under k_seg_merge's skip rules (which hold inside a tile as they do in the plane: lane 0 of a tile row has no left link here, as
// x = 0 has none there).  Indices in LDS are tile-local, row-major, so the smaller local index is the smaller global one and a tile-local root is
// the first pixel of its part of the segment.  At the end parent[p] = the GLOBAL index of p's tile-local root: every chain inside a tile has
// length one.  k_seg_border then unions, in global memory, the links that cross a tile border — every one of them, none skipped: a link is
// either inside one tile, where k_seg_tile made or implied it, or crosses a border.
constexpr uint32_t kSegTileW = 64, kSegTileH = 32, kSegTilePixels = kSegTileW * kSegTileH;
static_assert(kSegTileW == 64 && kSegTileH % kFilmWaves == 0, "a wavefront takes whole tile rows, a lane per pixel");

template <bool kDiagonal>
__global__ void __launch_bounds__(kFilmBlock) k_seg_tile(const uint32_t* __restrict__ classes, const float* __restrict__ mask, uint32_t width, uint32_t height, uint32_t tiles_x,
                                                         uint32_t* __restrict__ parent, uint32_t* overflow_word) {
    __shared__ uint32_t s_class[kSegTilePixels], s_parent[kSegTilePixels];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t x = (blockIdx.x % tiles_x) * kSegTileW + lane, y_tile = (blockIdx.x / tiles_x) * kSegTileH;
    for (uint32_t row = wave; row < kSegTileH; row += kFilmWaves) {
        const uint32_t y = y_tile + row;
        const uint32_t c = x < width && y < height ? seg_class(classes, mask, (uint64_t)y * width + x) : kSegNone;
        const uint32_t c_left = (uint32_t)__shfl_up((int)c, 1, 64);
        const bool linked = lane > 0u && seg_linked(c, c_left);
        const unsigned long long starts = ~__ballot(linked) & (~0ull >> (63u - lane));   // (bit 0 is always set)
        const uint32_t start = 63u - (uint32_t)__clzll((long long)starts);
        s_class[row * kSegTileW + lane] = c;
        s_parent[row * kSegTileW + lane] = c == kSegNone ? kSegNone : row * kSegTileW + start;
    }
    __syncthreads();
    for (uint32_t row = wave ? wave : kFilmWaves; row < kSegTileH; row += kFilmWaves) {   // (the tile's first row has no row above)
        const uint32_t i = row * kSegTileW + lane, c = s_class[i];
        if (c == kSegNone) continue;
        const bool left = lane > 0u && seg_linked(c, s_class[i - 1u]);
        const bool up = seg_linked(c, s_class[i - kSegTileW]);
        const bool up_left = lane > 0u && seg_linked(c, s_class[i - kSegTileW - 1u]);
        if (up) {
            if (!(left && up_left)) seg_union<seg_lds_load_t>(s_parent, i, i - kSegTileW, kSegTilePixels, overflow_word);
        } else if (kDiagonal) {
            if (up_left && !left) seg_union<seg_lds_load_t>(s_parent, i, i - kSegTileW - 1u, kSegTilePixels, overflow_word);
            if (lane < 63u && seg_linked(c, s_class[i - kSegTileW + 1u]) && !seg_linked(c, s_class[i + 1u]))
                seg_union<seg_lds_load_t>(s_parent, i, i - kSegTileW + 1u, kSegTilePixels, overflow_word);
        }
    }
    __syncthreads();
    const seg_plain_load_t load{s_parent};
    bool overflow = false;
    for (uint32_t row = wave; row < kSegTileH; row += kFilmWaves) {
        const uint32_t y = y_tile + row, i = row * kSegTileW + lane;
        if (!(x < width && y < height)) continue;
        uint32_t r = kSegNone;
        if (s_parent[i] != kSegNone) {
            const uint32_t local = seg_find(load, i, kSegTilePixels, overflow);
            r = (y_tile + local / kSegTileW) * width + (x - lane) + local % kSegTileW;
        }
        parent[(uint64_t)y * width + x] = r;
    }
    if (overflow) atomicOr(overflow_word, 1u);
}

template <bool kDiagonal>
__global__ void __launch_bounds__(kFilmBlock) k_seg_border(const uint32_t* __restrict__ classes, const float* __restrict__ mask, uint32_t npix, uint32_t width,
                                                           uint32_t* parent, uint32_t* overflow_word) {
    const uint64_t n_chunks = fs_chunks(npix), n_waves = film_waves();
    for (uint64_t chunk = film_first_chunk(); chunk < n_chunks; chunk += n_waves) {
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint64_t p64 = chunk_element(chunk, j);
            if (p64 >= npix) continue;
            const uint32_t p = (uint32_t)p64, x = p % width, y = p / width;
            const bool first_column = x % kSegTileW == 0u, last_column = x % kSegTileW == kSegTileW - 1u, first_row = y % kSegTileH == 0u;
            if (!first_column && !first_row && !(kDiagonal && last_column)) continue;   // no link of p to the left or upwards leaves its tile
            const uint32_t c = seg_class(classes, mask, p);
            if (c == kSegNone) continue;
            if (first_column && x > 0u && seg_linked(c, seg_class(classes, mask, p - 1u))) seg_union<seg_racing_load_t>(parent, p, p - 1u, npix, overflow_word);
            if (y == 0u) continue;
            if (first_row && seg_linked(c, seg_class(classes, mask, p - width))) seg_union<seg_racing_load_t>(parent, p, p - width, npix, overflow_word);
            if (!kDiagonal) continue;
            if ((first_row || first_column) && x > 0u && seg_linked(c, seg_class(classes, mask, p - width - 1u)))
                seg_union<seg_racing_load_t>(parent, p, p - width - 1u, npix, overflow_word);
            if ((first_row || last_column) && x + 1u < width && seg_linked(c, seg_class(classes, mask, p - width + 1u)))
                seg_union<seg_racing_load_t>(parent, p, p - width + 1u, npix, overflow_word);
        }
    }
}

// ---- k_seg_roots: root[p] = find(p), area[root] += 1 --------------------------------------------------------------------------------------------------
// parent[] is only read (plain loads: the merge has ended).  Atomics on one word are served one after the other, and the pixels of a film-sized
// segment all add to one: so a wavefront adds to area[] as seldom as it can.  Of every load, up to kSegLeaders times, the first lane not yet
// counted names its root, a ballot counts the lanes that share it, and the count joins what the wavefront holds for that root in registers
// (held across loads and chunks, written with one atomic when another root takes its place and at the end); what is left after that adds per run
// of consecutive lanes with one root.
__global__ void __launch_bounds__(kFilmBlock) k_seg_roots(const uint32_t* __restrict__ parent, uint32_t npix, uint32_t* __restrict__ root, uint32_t* __restrict__ area,
                                                          uint32_t* overflow_word) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t n_chunks = fs_chunks(npix), n_waves = film_waves();
    const seg_plain_load_t load{parent};
    bool overflow = false;
    uint32_t held_root = kSegNone, held = 0;   // the same in every lane
    for (uint64_t chunk = film_first_chunk(); chunk < n_chunks; chunk += n_waves) {
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint64_t p = chunk_element(chunk, j);
            const bool in = p < npix;
            uint32_t r = kSegNone;
            if (in && parent[p] != kSegNone) r = seg_find(load, (uint32_t)p, npix, overflow);
            if (in) root[p] = r;
            bool pending = r != kSegNone;
            for (uint32_t k = 0; k < kSegLeaders; ++k) {
                const unsigned long long todo = __ballot(pending);
                if (!todo) break;   // (the same in every lane)
                const uint32_t r0 = (uint32_t)__shfl((int)r, __ffsll((long long)todo) - 1, 64);
                const uint32_t n = (uint32_t)__popcll(__ballot(pending && r == r0));
                if (r0 != held_root) {
                    if (held && lane == 0u) atomicAdd(area + held_root, held);
                    held_root = r0, held = 0;
                }
                held += n;
                pending = pending && r != r0;
            }
            const uint32_t r_left = (uint32_t)__shfl_up((int)r, 1, 64);
            const bool run_head = lane == 0u || r != r_left;
            const uint32_t len = seg_run_length(__ballot(run_head), lane);
            if (run_head && pending) atomicAdd(area + r, len);   // (a run has one root: it is pending as a whole or not at all)
        }
    }
    if (held && lane == 0u) atomicAdd(area + held_root, held);
    if (overflow) atomicOr(overflow_word, 1u);
}

// whether pixel p is the root of a segment, and whether that segment is kept
WT_D bool seg_is_root(const uint32_t* root, uint64_t p, uint32_t npix) { return p < npix && root[p] == (uint32_t)p; }

// ---- k_seg_count: the kept roots of every chunk; the dropped segments -------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kFilmBlock) k_seg_count(const uint32_t* __restrict__ root, const uint32_t* __restrict__ area, uint32_t npix, uint32_t min_area,
                                                          uint32_t* __restrict__ chunk_count, seg_head_t* head) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t n_chunks = fs_chunks(npix), n_waves = film_waves();
    uint32_t n_dropped = 0;   // the same in every lane
    for (uint64_t chunk = film_first_chunk(); chunk < n_chunks; chunk += n_waves) {
        uint32_t n_kept = 0;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint64_t p = chunk_element(chunk, j);
            const bool is_root = seg_is_root(root, p, npix), kept = is_root && area[p] >= min_area;
            n_kept += (uint32_t)__popcll(__ballot(kept));
            n_dropped += (uint32_t)__popcll(__ballot(is_root && !kept));
        }
        if (lane == 0u) chunk_count[chunk] = n_kept;
    }
    if (lane == 0u && n_dropped) atomicAdd(&head->n_dropped, (unsigned long long)n_dropped);
}

// ---- k_seg_scan: ONE block; chunk_offset = the exclusive prefix sum of chunk_count, 256 chunks per turn with a carry; the total is K -------------------
__global__ void __launch_bounds__(kFilmBlock) k_seg_scan(const uint32_t* __restrict__ chunk_count, uint64_t n_chunks, uint32_t* __restrict__ chunk_offset, seg_head_t* head) {
    __shared__ uint32_t s_wave[kFilmWaves];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t carry = 0;   // (K is below 2^31)
    for (uint64_t base = 0; base < n_chunks; base += kFilmBlock) {
        const uint64_t i = base + threadIdx.x;
        const uint32_t v = i < n_chunks ? chunk_count[i] : 0u;
        uint32_t incl = v;
#pragma unroll
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint32_t t = (uint32_t)__shfl_up((int)incl, d, 64);
            if (lane >= d) incl += t;
        }
        if (lane == 63u) s_wave[wave] = incl;
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (uint32_t k = 0; k < kFilmWaves; ++k) {
            before += k < wave ? s_wave[k] : 0u;
            total += s_wave[k];
        }
        if (i < n_chunks) chunk_offset[i] = carry + before + incl - v;
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) head->n_segments = carry;
}

// ---- k_seg_number: ident[root] = the chunk's offset + the rank among the chunk's kept roots; the records' fields that need no atomics -------------------
__global__ void __launch_bounds__(kFilmBlock) k_seg_number(const uint32_t* __restrict__ classes, const uint32_t* __restrict__ root, const uint32_t* __restrict__ area, uint32_t npix,
                                                           uint32_t min_area, const uint32_t* __restrict__ chunk_offset, uint32_t max_records, uint32_t* __restrict__ ident,
                                                           film_segment_t* __restrict__ rec) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t n_chunks = fs_chunks(npix), n_waves = film_waves();
    for (uint64_t chunk = film_first_chunk(); chunk < n_chunks; chunk += n_waves) {
        uint32_t next = chunk_offset[chunk];
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint64_t p = chunk_element(chunk, j);
            const bool is_root = seg_is_root(root, p, npix);
            const uint32_t a = is_root ? area[p] : 0u;
            const bool kept = is_root && a >= min_area;
            const unsigned long long b = __ballot(kept);
            const uint32_t id = next + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
            next += (uint32_t)__popcll(b);
            if (is_root) ident[p] = kept ? id : kSegNone;
            // the box grows from the empty one and the sums from zero: k_seg_relabel's atomics
            if (kept && id < max_records) rec[id] = film_segment_t{classes ? classes[p] : 0u, a, (uint32_t)p, kSegNone, kSegNone, 0u, 0u, 0u, 0ull, 0ull};
        }
    }
}

// ---- k_seg_relabel: the plane, the counts, the records ----------------------------------------------------------------------------------------------------
// The records grow by native integer atomics: u64 add for the sums, u32 min / max for the box.  As in k_seg_roots a wavefront issues them as seldom
// as it can: of every load, up to kSegLeaders times, the first lane not yet gathered names its id, the lanes that share it are reduced across the
// wavefront (they may lie in more than one row) and merged (seg_merge) into the part of that id's record which lane 0 holds in registers across
// loads and chunks, written when another id takes its place and at the end; what is left after that adds per run of consecutive lanes of one row
// with one id (seg_of_run).
__global__ void __launch_bounds__(kFilmBlock) k_seg_relabel(const uint32_t* __restrict__ root, const uint32_t* __restrict__ ident, uint32_t npix, uint32_t width, uint32_t max_records,
                                                            uint32_t* __restrict__ segments, film_segment_t* rec, seg_head_t* head) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t n_chunks = fs_chunks(npix), n_waves = film_waves();
    uint32_t n_members = 0, n_dropped_pixels = 0;   // the same in every lane; below 2^31
    uint32_t held_id = kSegNone;                    // the same in every lane
    film_segment_t held{};                          // lane 0's; area = 0: nothing held (the record's area is k_seg_number's, this one only says "not empty")
    auto flush = [&]() {
        if (lane == 0u && held.area) {
            film_segment_t& t = rec[held_id];
            atomicAdd(&t.sum_x, held.sum_x);
            atomicAdd(&t.sum_y, held.sum_y);
            atomicMin(&t.x0, held.x0);
            atomicMax(&t.x1, held.x1);
            atomicMin(&t.y0, held.y0);
            atomicMax(&t.y1, held.y1);
        }
    };
    for (uint64_t chunk = film_first_chunk(); chunk < n_chunks; chunk += n_waves) {
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint64_t p = chunk_element(chunk, j);
            const bool in = p < npix;
            const uint32_t r = in ? root[p] : kSegNone;
            const uint32_t id = r != kSegNone ? ident[r] : kSegNone;
            if (in) segments[p] = id;
            n_members += (uint32_t)__popcll(__ballot(r != kSegNone));
            n_dropped_pixels += (uint32_t)__popcll(__ballot(r != kSegNone && id == kSegNone));
            const uint32_t x = in ? (uint32_t)p % width : 0u, y = in ? (uint32_t)p / width : 0u;
            bool pending = id < max_records;   // (kSegNone is not below it)
            for (uint32_t k = 0; k < kSegLeaders; ++k) {
                const unsigned long long todo = __ballot(pending);
                if (!todo) break;   // (the same in every lane)
                const uint32_t id0 = (uint32_t)__shfl((int)id, __ffsll((long long)todo) - 1, 64);
                const bool mine = pending && id == id0;
                film_segment_t part{};
                part.area = (uint32_t)__popcll(__ballot(mine));
                part.first = kSegNone;
                part.sum_x = wave_sum_u64(mine ? x : 0u);
                part.sum_y = wave_sum_u64(mine ? y : 0u);
                part.x0 = ~wave_max_u32(mine ? ~x : 0u);
                part.y0 = ~wave_max_u32(mine ? ~y : 0u);
                part.x1 = wave_max_u32(mine ? x : 0u);
                part.y1 = wave_max_u32(mine ? y : 0u);
                if (id0 != held_id) {
                    flush();
                    held_id = id0, held = film_segment_t{};
                }
                if (held.area == 0u) held = part;   // (meaningful in lane 0, where the reductions end)
                else seg_merge(held, part);
                pending = pending && !mine;
            }
            const uint32_t id_left = (uint32_t)__shfl_up((int)id, 1, 64);
            const bool run_head = lane == 0u || id != id_left || x == 0u;
            const uint32_t len = seg_run_length(__ballot(run_head), lane);
            if (run_head && pending) {   // (a run has one id: it is pending as a whole or not at all)
                const film_segment_t run = seg_of_run(0u, (uint32_t)p, x, y, len);
                film_segment_t& t = rec[id];
                atomicAdd(&t.sum_x, run.sum_x);
                atomicAdd(&t.sum_y, run.sum_y);
                atomicMin(&t.x0, run.x0);
                atomicMax(&t.x1, run.x1);
                atomicMin(&t.y0, run.y0);
                atomicMax(&t.y1, run.y1);
            }
        }
    }
    flush();
    if (lane == 0u) {
        if (n_members) atomicAdd(&head->n_members, (unsigned long long)n_members);
        if (n_dropped_pixels) atomicAdd(&head->n_dropped_pixels, (unsigned long long)n_dropped_pixels);
    }
}

// the scratch of a call in 32-bit words: parent (later the ids), root and area per pixel, count and offset per chunk
uint64_t film_segments_scratch_words(uint64_t npix) { return 3u * npix + 2u * fs_chunks(npix); }

int film_segments_launch(const sensor_t& sn, hipStream_t stream, uint32_t n_cus, uint32_t tiled, uint32_t flags, uint32_t min_area, uint32_t max_records, const uint32_t* d_classes,
                         const float* d_mask, uint32_t* d_segments, void* d_head, void* d_records, uint32_t* d_work) {
    const uint64_t npix64 = (uint64_t)sn.width * sn.height;
    if (npix64 == 0 || npix64 >= kSegMaxPixels || (flags & ~(uint32_t)SEG_DIAGONAL)) return (int)hipErrorInvalidValue;
    const uint32_t npix = (uint32_t)npix64, width = sn.width;
    const uint64_t n_chunks = fs_chunks(npix);
    min_area = std::max(min_area, 1u);
    // the ids take the parents' place: k_seg_roots is the last to read a parent, k_seg_number the first to write an id, at roots only
    uint32_t *parent = d_work, *ident = d_work, *root = parent + npix, *area = root + npix, *chunk_count = area + npix, *chunk_offset = chunk_count + n_chunks;
    seg_head_t* head = static_cast<seg_head_t*>(d_head);
    film_segment_t* rec = static_cast<film_segment_t*>(d_records);
    const dim3 grid(film_grid_blocks(npix, n_cus, kSegBlocksPerCU)), block(kFilmBlock);
    if (const hipError_t e = hipMemsetAsync(head, 0, sizeof(seg_head_t), stream)) return (int)e;
    if (const hipError_t e = hipMemsetAsync(area, 0, (size_t)npix * sizeof(uint32_t), stream)) return (int)e;
    if (tiled) {
        const uint32_t tiles_x = (width + kSegTileW - 1u) / kSegTileW, tiles_y = (sn.height + kSegTileH - 1u) / kSegTileH;   // (fewer than 2^31 / 64 + 2^31 / 32 tiles)
        const dim3 tiles(tiles_x * tiles_y);
        if (flags & SEG_DIAGONAL) {
            hipLaunchKernelGGL(k_seg_tile<true>, tiles, block, 0, stream, d_classes, d_mask, width, sn.height, tiles_x, parent, &head->overflow);
            hipLaunchKernelGGL(k_seg_border<true>, grid, block, 0, stream, d_classes, d_mask, npix, width, parent, &head->overflow);
        } else {
            hipLaunchKernelGGL(k_seg_tile<false>, tiles, block, 0, stream, d_classes, d_mask, width, sn.height, tiles_x, parent, &head->overflow);
            hipLaunchKernelGGL(k_seg_border<false>, grid, block, 0, stream, d_classes, d_mask, npix, width, parent, &head->overflow);
        }
    } else {
        hipLaunchKernelGGL(k_seg_runs, grid, block, 0, stream, d_classes, d_mask, npix, width, parent);
        if (flags & SEG_DIAGONAL)
            hipLaunchKernelGGL(k_seg_merge<true>, grid, block, 0, stream, d_classes, d_mask, npix, width, parent, &head->overflow);
        else
            hipLaunchKernelGGL(k_seg_merge<false>, grid, block, 0, stream, d_classes, d_mask, npix, width, parent, &head->overflow);
    }
    hipLaunchKernelGGL(k_seg_roots, grid, block, 0, stream, parent, npix, root, area, &head->overflow);
    hipLaunchKernelGGL(k_seg_count, grid, block, 0, stream, root, area, npix, min_area, chunk_count, head);
    hipLaunchKernelGGL(k_seg_scan, dim3(1), block, 0, stream, chunk_count, n_chunks, chunk_offset, head);
    hipLaunchKernelGGL(k_seg_number, grid, block, 0, stream, d_classes, root, area, npix, min_area, chunk_offset, max_records, ident, rec);
    hipLaunchKernelGGL(k_seg_relabel, grid, block, 0, stream, root, ident, npix, width, max_records, d_segments, rec, head);
    return (int)hipGetLastError();
}

// seg_find by itself on a hand-made parent array (wtgpu_test_film_segments_find): the bound and the flag, on the host
uint32_t film_segments_find_host(const uint32_t* parent, uint32_t x, uint32_t bound, bool& overflow) { return seg_find(seg_plain_load_t{parent}, x, bound, overflow); }

// ---- the host twin: a sequential two-pass union-find.  The answer is canonical, so any algorithm gives it; n_threads is accepted and not used ------
void film_segments_host(const sensor_t& sn, uint32_t flags, uint32_t min_area, uint32_t max_records, const uint32_t* classes, const float* mask, uint32_t /*n_threads*/,
                        uint32_t* segments, unsigned long long* info, void* out_records) {
    const uint32_t W = sn.width, H = sn.height, npix = W * H;
    const bool diagonal = (flags & SEG_DIAGONAL) != 0;
    min_area = std::max(min_area, 1u);
    std::vector<uint32_t> parent(npix), cls(npix);
    auto find = [&](uint32_t x) {
        while (parent[x] != x) x = parent[x] = parent[parent[x]];   // (path halving)
        return x;
    };
    auto unite = [&](uint32_t a, uint32_t b) {
        a = find(a), b = find(b);
        if (a != b) parent[std::max(a, b)] = std::min(a, b);
    };
    for (uint32_t p = 0; p < npix; ++p) cls[p] = seg_class(classes, mask, p), parent[p] = p;
    for (uint32_t y = 0, p = 0; y < H; ++y)
        for (uint32_t x = 0; x < W; ++x, ++p) {
            const uint32_t c = cls[p];
            if (c == kSegNone) continue;
            if (x > 0 && seg_linked(c, cls[p - 1])) unite(p, p - 1);
            if (y == 0) continue;
            if (seg_linked(c, cls[p - W])) unite(p, p - W);
            if (diagonal && x > 0 && seg_linked(c, cls[p - W - 1])) unite(p, p - W - 1);
            if (diagonal && x + 1 < W && seg_linked(c, cls[p - W + 1])) unite(p, p - W + 1);
        }
    // the smaller index is always the parent, so a root is its segment's first pixel and the roots come in the order of the numbering.  ident[root]: first
    // the root's place among the roots, where its record is gathered; then the segment's number
    std::vector<uint32_t> ident(npix, kSegNone);
    uint32_t n_roots = 0;
    for (uint32_t p = 0; p < npix; ++p)
        if (cls[p] != kSegNone && parent[p] == p) ident[p] = n_roots++;
    std::vector<film_segment_t> all(n_roots);   // (area 0: nothing met yet)
    unsigned long long n_members = 0, n_dropped = 0, n_dropped_pixels = 0;
    for (uint32_t y = 0, p = 0; y < H; ++y)
        for (uint32_t x = 0; x < W; ++x, ++p) {
            if (cls[p] == kSegNone) continue;
            ++n_members;
            film_segment_t& r = all[ident[find(p)]];
            const film_segment_t one = seg_of_run(cls[p], p, x, y, 1u);
            if (r.area == 0) r = one;
            else seg_merge(r, one);
        }
    film_segment_t* rec = static_cast<film_segment_t*>(out_records);
    uint32_t K = 0;
    for (uint32_t p = 0; p < npix; ++p) {
        if (cls[p] == kSegNone || parent[p] != p) continue;
        const film_segment_t& r = all[ident[p]];
        if (r.area < min_area) {
            ++n_dropped, n_dropped_pixels += r.area;
            ident[p] = kSegNone;
            continue;
        }
        if (K < max_records) rec[K] = r;
        ident[p] = K++;
    }
    for (uint32_t p = 0; p < npix; ++p) segments[p] = cls[p] == kSegNone ? kSegNone : ident[find(p)];
    info[0] = K, info[1] = n_dropped, info[2] = n_members, info[3] = n_dropped_pixels;
}

}   // namespace wtk
