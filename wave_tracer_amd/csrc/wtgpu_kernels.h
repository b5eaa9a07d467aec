// wave_tracer_amd — what the kernel translation units (kernels_*.hip) and the host side (wtgpu*.hip, wtgpu_host.h) share: the slice state, the launch block,
// the device-side queue helpers, the work-item vocabulary of the render kernels (queue item -> sample id, pool, vertex stores, bucket, counters,
// traversal-record words) and the kernels' declarations.  The kernels of one batch, in launch order:
//   kernels_walk.hip    k_generate, k_interact (pass A; k_interact_coop: with cooperative record I/O; k_classify + k_interact_sorted / _diffuse /
//                       _dielectric / _spm / _any: by material class), k_edges, k_interact_b (pass B), k_light_rounds (a batch's thin last rounds)
//   kernels_trace.hip   k_trace_refill (body: kernels_trace_refill.h, which k_light_rounds runs too), the staged k_tr_axis / _cone / _policy / _tail,
//                       k_trace_heavy (+ the per-query kernels of the traversal parity tests, the PMC calibration copy)
//   kernels_fsd.hip     k_flux_split, k_flux_tasks, k_interact_c_prep, _wide, _hard_tries, _commit (Fraunhofer interactions: power sums, rejection sampling in
//                       three lane shapes; k_interact_c, k_interact_c_hard: the one-wavefront-per-walk form, WTGPU_PASS_C_TIERS=0)
//   kernels_path.hip    k_path_generate, _fsd, _interact, _edges, _interact_b, _nee, _flush (plt_path)
//   kernels_connect.hip k_connect_enum, _scan, _class / _strat (+ _open), the staged _eval / _shadow / _mis, _splat / _splat_tiled
//   kernels_test.hip    test entry points of the wave-cooperative Fraunhofer / UTD forms and of the material layer (wtgpu_test_hooks.h)
//   kernels_mask.hip    k_sensor_mask_wave / k_sensor_mask_lane: by-geometry sensor masks (not part of a render)
//   kernels_firsthit.hip k_first_hit / k_first_hit_wave: first-hit maps of a perspective sensor — depth, position, normals, uv, ids (not part of a render)
//   kernels_firsthit_material.hip k_first_hit_material / k_first_hit_material_wave: first-hit material maps — albedo, specular reflectance, opacity, roughness, emission, material ids (not part of a render)
//   kernels_los.hip     k_los_sample / k_los_pair: line-of-sight maps — which emitters a sensor element or a caller's point sees (not part of a render)
//   kernels_maps.h      what the last four share on the device and in their host twins: the two lane shapes (one lane per element, one lane per sample) with
//                       their grids, a group's share of a ballot, the exchange through the LDS of the stacks and its sums in sample order, the host twins' loop
//   kernels_develop.hip k_develop / k_develop_tonemap: film development and tonemapping (not part of a render)
//   kernels_stats.hip   k_film_stats / k_film_stats_finish: range, histogram and sum of a film (not part of a render)
//   kernels_zonal.hip   k_film_zonal / k_film_zonal_finish / k_film_zonal_paint: a statistics record per (zone, plane) of a film under a label plane (not part of a render)
//   kernels_segments.hip k_seg_runs / _merge (or k_seg_tile / _border) / _roots / _count / _scan / _number / _relabel: connected segments of a label plane by union-find (not part of a render)
//   kernels_distance.hip k_dist_columns / k_dist_rows: exact Euclidean distance transform of a label plane with the nearest site (not part of a render)
//   kernels_compare.hip k_film_compare (+ k_film_finish): difference statistics of two films (not part of a render)
//   kernels_polar.hip   k_film_polar (+ k_film_finish): polarisation maps, Stokes sums and false-colour picture of a Stokes film (not part of a render)
//   kernels_denoise.hip k_denoise_prepare / _variance / k_denoise_filter: the dual-buffer non-local-means filter of two half-films (not part of a render)
//   kernels_film.h      what the last five share on the device and in their host twins: chunk geometry, level reduction, grid, dispatch, host threads; and what
//                       a "sums + counts + best" pass (compare, polar) is besides its per-pixel arithmetic: wavefront records, k_film_finish, the host twin's scaffold
// One translation unit per group: they compile in parallel (the single file took four minutes) and a kernel's registers are not at the mercy of
// its neighbours' inlining decisions.  Kernels are launched across translation units through their host-side handles (external linkage: hence
// the NAMED namespace).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/wtgpu.h"
#include "wt/bdpt.h"
#include "wt/coop.h"
#include "wt/coop_fsd.h"
#include "wt/coop_utd.h"
#include "wt/path.h"

using namespace wt;
namespace wt {
struct tonemap_args_t;   // wt/tonemap.h (kernels_develop.hip and the entry points that launch it)
struct film_polar_args_t;   // wt/film_polar.h (kernels_polar.hip and its entry points)
struct film_denoise_args_t;   // wt/film_denoise.h (kernels_denoise.hip and its entry points)
struct film_denoise_guides_t;
struct los_query_t;   // wt/los.h (kernels_los.hip and its entry points)
struct fhm_query_t;   // wt/first_hit_material.h (kernels_firsthit_material.hip and its entry points)
}

namespace wtk {


// Register budgets (second __launch_bounds__ argument = minimum waves per SIMD => 512 / n unified VGPRs per lane).
#ifndef WTGPU_LB_TRACE
#define WTGPU_LB_TRACE 3
#endif
#ifndef WTGPU_LB_HEAVY
#define WTGPU_LB_HEAVY 3   // 142 VGPRs, no spills, no scratch frame, with the wave-uniform state in scalar registers (wt/coop.h: uniform(); before: 236 VGPRs => 2)
#endif
#ifndef WTGPU_LB_INTERACT
#define WTGPU_LB_INTERACT 3   // (round 6, with the bicubic texture path in the kernel: 4 / 3 / 2 waves per SIMD -> 29.1-29.3 / 29.9-30.2 / 30.2 Msamples/s; until round 5: 4)
#endif
#ifndef WTGPU_LB_INTERACT_B
#define WTGPU_LB_INTERACT_B 3
#endif
#ifndef WTGPU_LB_INTERACT_C
#define WTGPU_LB_INTERACT_C 3
#endif
#ifndef WTGPU_LB_FLUX
#define WTGPU_LB_FLUX 3
#endif
#ifndef WTGPU_LB_CONNECT
#define WTGPU_LB_CONNECT 2   // 355 -> 105 spilled registers (the rest of its frame are the two vertices and beams of a connection)
#endif
constexpr uint32_t kFluxTaskTris = 2048;   // default size of a region-sum task (k_flux_split / k_flux_tasks)
constexpr int kBlock = 128;
#ifndef WTGPU_LDS_STACK
#define WTGPU_LDS_STACK 20
#endif
constexpr int kLdsStack = WTGPU_LDS_STACK;   // LDS-resident stack entries per lane
constexpr uint32_t kConeBudget = 96;     // work units (1 per cone-triangle test, 2 per node) one lane may spend on a cone query before it is handed to a wavefront (with lane refill, round 3: 32 / 48 / 64 / 96 / 128 -> 14.6 / 14.8 / 15.2 / 14.4 / 12.8 Msamples/s; round 2's kernel without refill: optimum 28-32)
constexpr int kSpillStack = 64 - kLdsStack;   // scratch spill entries per lane (total 64, the reference's ray stack size)

// control block of one state slice (device memory)
enum : uint32_t { CTL_STRAT_HEAD_OPEN = 25, CTL_UTD_COUNT0 = 26, CTL_UTD_COUNT1 = 27, CTL_FSDQ_COUNT0 = 28, CTL_FSDQ_COUNT1 = 29, CTL_FSDQ_HEAD = 30, CTL_NEEQ_COUNT = 31, CTL_NEEQ_HEAD = 32, CTL_COUNT0 = 0, CTL_COUNT1 = 1, CTL_HEAD_TRACE = 2, CTL_HEAD_INTERACT = 3, CTL_HEAVY_COUNT = 4, CTL_HEAVY_HEAD = 5, CTL_FSD_COUNTER = 6,
                  CTL_ROUNDS = 7, CTL_STRAT_HEAD = 8, CTL_INTB_COUNT = 9, CTL_INTB_HEAD = 10, CTL_GATHER_COUNT = 11, CTL_GATHER_HEAD = 12, CTL_INTC_COUNT = 13, CTL_INTC_HEAD = 14, CTL_FTASK_COUNT = 15, CTL_FTASK_HEAD = 16, CTL_FSPLIT_HEAD = 17, CTL_EPOOL_COUNT = 18, CTL_FSD_ECOUNTER = 19, CTL_INTD_COUNT = 20, CTL_INTD_HEAD = 21, CTL_BACK0 = 22, CTL_BACK1 = 23,
                  CTL_TPOL_COUNT0 = 41, CTL_TPOL_COUNT1 = 42, CTL_TPOL_HEAD = 43, CTL_TCONE_COUNT0 = 44, CTL_TCONE_COUNT1 = 45, CTL_TCONE_HEAD = 46,   // the staged trace kernels' queues (trace_stage_t)
                  CTL_CLS_COUNT0 = 33, CTL_CLS_HEAD0 = 37,   // the material-sorted pass A: sizes and dequeue heads of the kNumWalkClasses class queues (k_classify / k_interact_cls)
                  CTL_LIGHT_DONE = 47, CTL_LIGHT_STOP = 48,   // k_light_rounds: whole rounds it ran, the stage the host has to continue the next one from (0: none)
                  CTL_PCW_COUNT = 49, CTL_PCW_HEAD = 50, CTL_PCC_COUNT = 51, CTL_PCC_HEAD = 52,   // pass C in tiers: the wide queue and the commit queue (k_interact_c_prep's own queue is pass C's: CTL_INTC_*)
                  CTL_WORDS = 56 };   // (CTL_BACK*: see queue_append)   // (CTL_GATHER_*: queue of k_edges)
constexpr uint32_t kTriListWords = 128;   // per-walk list storage: 64 triangle ids, or (after coop_gather) up to 96 edge ids
constexpr uint32_t kGatherMarker = 0xFFFFFFFEu;   // trav.tuid of a walk whose interaction region was gathered
// ... and whose Fraunhofer aperture k_edges built as well (pool slot in trav.by): with segments — the walk is already queued for pass
// C — or without (pass B commits the restart)
constexpr uint32_t kApertureMarker = 0xFFFFFFFDu, kNullApertureMarker = 0xFFFFFFFCu;
__host__ __device__ inline bool is_region_marker(uint32_t t) { return t == kGatherMarker || t == kApertureMarker; }
// connection strategies (s,t) are bucketed by (min(t, kKeyDim-1), min(s, kKeyDim-1)): one bucket per strategy up to 18 vertices per subpath; a
// bucket of the last row / column holds every longer strategy of its sample (an item of such a bucket loops over them, k_connect_strat)
// (kMaxVerts + 2: up to max_depth = 16 — 18 vertices per subpath — every strategy has its own bucket and k_connect_strat_open is not launched;
// launching it for nothing cost 35 % of a pass with four streams: a 256-register, 22-KB-LDS grid that waits for free CUs holds up the other
// streams' dispatches)
constexpr uint32_t kKeyDim = kMaxVerts + 2, kNumKeys = kKeyDim * kKeyDim;
// The class form of the connections (k_connect_class) buckets SAMPLES by the same key grid: (min(nT, kKeyDim-1), min(nS, kKeyDim-1)), the lengths of
// a sample's two subpaths.  Its wavefronts take the classes in the order of descending tk x sk — the number of strategies of a sample of the class,
// near enough — so that the rare deep classes, hundreds of strategies per item, start first and are not the kernel's tail.  Rank of a key in
// that order (ties: the smaller key first); the ranks of the kNumKeys keys are a permutation of 0 .. kNumKeys - 1.
__host__ __device__ constexpr uint32_t class_key_work(uint32_t key) { return (key / kKeyDim) * (key % kKeyDim); }
__host__ __device__ constexpr uint32_t class_key_rank(uint32_t key) {
    uint32_t r = 0;
    for (uint32_t k = 0; k < kNumKeys; ++k)
        if (class_key_work(k) > class_key_work(key) || (class_key_work(k) == class_key_work(key) && k < key)) ++r;
    return r;
}
__host__ __device__ constexpr bool class_key_open(uint32_t key) { return key / kKeyDim == kKeyDim - 1 || key % kKeyDim == kKeyDim - 1; }
// strat_prefix in the class form, all by RANK: [0, kNumKeys] start of the class in the flattened item space, every class padded to whole
// wavefronts (64 items of a grab are then 64 samples of ONE class); [kClassCount + r] its samples; [kClassKey + r] its key
constexpr uint32_t kClassCount = kNumKeys + 1, kClassKey = kClassCount + kNumKeys, kClassTableWords = kClassKey + kNumKeys;

struct device_state_t {
    uint64_t cap = 0;   // samples per batch
    uint32_t max_verts = 0;
    uint32_t walk_words = 0;   // words of one walk record (walk_t, or path_walk_t for plt_path scenes)
    size_t vert_words = 0;     // words of one walk's vertex array (max_verts x kVertexWords)
    uint32_t* walks = nullptr;    // [kWalkWords][2cap]
    uint32_t* verts = nullptr;    // [max_verts*kVertexWords][2cap]
    uint32_t* ctx = nullptr;      // [kCtxWords][cap]
    uint32_t* trav = nullptr;     // [kTravWords][2cap]
    uint32_t* tris = nullptr;     // [kMaxConeTris][2cap]
    uint32_t* queue[2] = {nullptr, nullptr};
    uint32_t* heavy_queue = nullptr;   // walks whose traversal exceeded the per-lane budget
    uint32_t* intb_queue = nullptr;    // walks whose interaction takes the expensive (no primary triangle) path
    uint32_t* gather_queue = nullptr;  // ... of those, the ones whose triangle list overflowed (coop_gather first)
    uint32_t* intc_queue = nullptr;    // ... and the ones that built a Fraunhofer aperture with edges (sampled in pass C)
    uint32_t* intd_queue = nullptr;    // ... of those, the ones whose rejection sampling outlasts kEasyTries tries (k_interact_c_hard); behind it, same allocation: pass_c_wide_queue, pass_c_commit_queue
    uint2* ftasks = nullptr;           // (walk, subtree) tasks of the intercepted-power sums of overflowed regions (k_flux_split / k_flux_tasks)
    uint32_t ftask_cap = 0;
    double* facc = nullptr;            // [2cap] their accumulators
    uint32_t* epool = nullptr;         // edge-id lists of the gathered regions of one round (bump allocator, k_edges)
    uint32_t epool_cap = 0;
    uint32_t* ctl = nullptr;           // [CTL_WORDS] queue sizes, dequeue heads, FSD pool bump counter, rounds done
    fsd_aperture_t* fsd_hdr = nullptr;
    fsd_edge_t* fsd_edges = nullptr;
    uint32_t fsd_cap = 0;
    uint32_t fsd_ecap = 0;            // segment records of all apertures of a batch (bump allocator)
    uint32_t* strat_items = nullptr;    // [kNumKeys][cap] sample indices bucketed by connection strategy (s,t) (class form: by the subpath lengths (nT, nS))
    uint32_t* strat_count = nullptr;    // [kNumKeys]
    uint32_t* strat_prefix = nullptr;   // [kClassTableWords]: [kNumKeys + 1] prefix sums by key (class form: by rank, then the classes' sizes and keys, see kClassCount)
    double* lacc = nullptr;             // [4][cap] per-sample sum of the t>1 strategies' fluxes
    unsigned long long* counters = nullptr;   // bdpt_counters_t + 2 (shared by all slices)
    const struct bdpt_ext_t* ext = nullptr;   // more plt_bdpt state behind one pointer (device memory; the launch block must stay below 1 KB, see path_state_t)
};
// plt_bdpt only — like path_state_t a device-resident block that kernels reach through one pointer of the launch block.
struct bdpt_ext_t {
    // material-sorted pass A: walk class of every triangle (wt/bdpt.h: walk_class_of_triangle, built at upload) and the round's class queues
    const unsigned char* tri_class = nullptr;
    uint32_t* cls_queue = nullptr;   // [kNumWalkClasses][2 cap]
    // staged connections: the connections that wait for their shadow ray (k_connect_eval -> k_connect_shadow -> k_connect_mis)
    // The strategy items of a batch are connected in CHUNKS of pend_cap items (in bucket order), each chunk through the three kernels in turn: a
    // chunk's connections cannot outnumber its items, so the pending list cannot overflow whatever the scene's depth.  chunk_ctl: kChunkCtlWords
    // counters per chunk (zeroed by k_connect_scan).
    struct conn_pending_t* pend = nullptr;
    uint32_t* surv = nullptr;        // [pend_cap] the pending connections whose ray arrived (indices into pend)
    uint32_t* chunk_ctl = nullptr;   // [n_chunks][kChunkCtlWords]
    uint32_t pend_cap = 0, n_chunks = 0;
};
enum : uint32_t { CHUNK_EVAL_HEAD = 0, CHUNK_PEND_COUNT = 1, CHUNK_PEND_HEAD = 2, CHUNK_SURV_COUNT = 3, CHUNK_MIS_HEAD = 4, kChunkCtlWords = 8 };
struct conn_pending_t {   // 52 B
    uint32_t i;    // sample of the batch
    uint32_t st;   // s | t << 16 | kPendShadow
    float L[4];    // flux of the unoccluded connection
    float o[3], d[3], dist;   // the shadow ray
};
// plt_path only — a device-resident block the path kernels get a pointer to (launch_args_t stays below 1024 bytes: by-value kernel
// arguments beyond that cost 40 % of a plt_bdpt pass with four streams, measured: 976 -> 1048 bytes, 15.4 -> 11.1 Msamples/s).
struct path_state_t {
    // plt_path: wedge records of the walks' UTD apertures, two pools used alternately (round parity: an aperture built in round r is evaluated in
    // round r + 1), each reset when its round begins; queues of the wave-per-walk UTD kernels and what they exchange with k_path_interact
    utd_edge_rec_t* utd[2] = {nullptr, nullptr};
    uint32_t utd_cap = 0;
    uint32_t* fsdq[2] = {nullptr, nullptr};   // walks that carry an aperture into the next round (k_path_fsd evaluates it there)
    uint32_t* neeq = nullptr;                  // walks with a deferred next-event estimation of this round (k_path_nee)
    float* fsd_f = nullptr;                    // [cap] k_path_fsd's result per walk
    path_nee_rec_t* nee_recs = nullptr;        // [cap]
    uint2* gather_info = nullptr;              // [cap] k_path_edges' result per walk: (offset into the round's edge pool, number of ids)
};
constexpr size_t kWalkWords = sizeof(walk_t) / 4;
constexpr size_t kCtxWords = sizeof(sample_ctx_t) / 4;
constexpr size_t kTravWords = sizeof(trav_result_t) / 4;
#define WT_TRAV_WORD(field) (offsetof(trav_result_t, field) / 4)
// The staged trace kernels (k_tr_axis / k_tr_cone / k_tr_policy / k_tr_tail, kernels_trace.hip) keep a walk's traversal state in memory between
// their stages: the traced envelope and the policy's state.  The records live BEHIND the slice's traversal records, the two queues behind its heavy
// queue (same allocations: the launch block is at its 984-byte limit, see path_state_t).
struct trace_stage_t {
    cone_t env;
    axis_walk_t aw;
};
constexpr size_t kStageWords = sizeof(trace_stage_t) / 4;
constexpr size_t kNumCounters = sizeof(bdpt_counters_t) / sizeof(unsigned long long);
constexpr size_t kProfSlots = 224;   // WTGPU_PROFILE scratch counters behind the public ones (from kPassCTierSlot on: the tier counts of pass C, kept whenever statistics are)
constexpr size_t kDroppedSlot = kNumCounters + kProfSlots;   // ... and behind those: children a full cooperative traversal stack could not hold (wt/coop.h)


struct launch_args_t {
    scene_t sc;
    device_state_t st;
    film_t film;
    uint64_t seed;
    uint64_t j0;        // first global work item of this batch
    uint32_t nb;        // samples in this batch
    uint32_t npix;
    uint64_t sample_begin;
    uint32_t count_stats;
    uint32_t cone_budget;
    uint32_t flux_task_tris;   // k_flux_split: largest subtree handed to one wavefront of k_flux_tasks
    uint32_t heavy_probe;   // k_trace_heavy: any-hit probe of the near slab before the handed-over cone query too
    uint32_t coop_aperture_min;   // regions with at least this many classified edges get their aperture built by k_edges' wavefront
    uint32_t profile;   // WTGPU_PROFILE=1: clock64() breakdown of the heavy traversals into counters[kNumCounters..]
    uint32_t split_queues;   // round queues keep sensor and emitter walks apart (queue_append); 0: one mixed queue (A/B)
    uint32_t lane_cache, heavy_cache;   // diagnostic switches of the remembered rejecting triangles (wt::traverse_axis / coop_traverse); default on
    uint32_t collect_list;    // bit 0: the cone queries keep the bounded triangle list of the interaction region; bit 1: primary triangles from the axis query always (wtgpu.hip)
};

WT_D uint32_t* trace_stage_words(const launch_args_t& a) { return a.st.trav + kTravWords * 2 * (size_t)a.st.cap; }   // [2 cap][kStageWords]
WT_D uint32_t* trace_pol_queue(const launch_args_t& a) { return a.st.heavy_queue + 2 * (size_t)a.st.cap; }
WT_D uint32_t* trace_cone_queue(const launch_args_t& a) { return a.st.heavy_queue + 4 * (size_t)a.st.cap; }
// ---- pass C in tiers (kernels_fsd.hip: k_interact_c_prep -> k_interact_c_wide -> k_interact_c_hard_tries -> k_interact_c_commit) ----------------------
// Two more [2 cap] queues behind the hard queue (same allocation, like the two above): the walks whose first kPrepTries tries were all rejected, and
// the walks whose outcome is known and waits for k_interact_c_commit.
WT_D uint32_t* pass_c_wide_queue(const launch_args_t& a) { return a.st.intd_queue + 2 * (size_t)a.st.cap; }
WT_D uint32_t* pass_c_commit_queue(const launch_args_t& a) { return a.st.intd_queue + 4 * (size_t)a.st.cap; }
// The OUTCOME of a walk's rejection sampling, from the kernel that found it to k_interact_c_commit: the first four words of the walk's
// triangle-list slot (st.tris) — [0] kOutcomeAccepted | index of the accepted try (0: every try was rejected), [1] x.x, [2] x.y, [3] f of that try.
// The slot is dead at that point: its last reader in a round is the intercepted-power sum of k_interact_c_prep (a wavefront writes a walk's
// outcome after the group's sum has consumed every loaded triangle id); the try kernels read the aperture pool only; the commit re-enters
// bdpt_walk_step with known_no_primary, have_aperture and resolved set, which skips the list scan, the edge gathering and the power sum — the
// step's three readers of the list; and the next round's trace kernels rewrite the list before anything reads it again.
constexpr uint32_t kOutcomeAccepted = 0x80000000u;   // (a try index is below kFsdMaxEdges x 1024 = 2^22)
WT_D uint32_t* pass_c_outcome(const launch_args_t& a, uint32_t w) { return a.st.tris + (size_t)w * kTriListWords; }
WT_D void pass_c_store_outcome(const launch_args_t& a, uint32_t w, const fsd_outcome_t& r) {
    uint32_t* o = pass_c_outcome(a, w);
    o[0] = r.acc ? (kOutcomeAccepted | r.t_acc) : 0u;
    o[1] = __float_as_uint(r.x.x);
    o[2] = __float_as_uint(r.x.y);
    o[3] = __float_as_uint(r.f);
}
WT_D fsd_outcome_t pass_c_load_outcome(const launch_args_t& a, uint32_t w) {
    const uint32_t* o = pass_c_outcome(a, w);
    const uint32_t o0 = o[0];
    return fsd_outcome_t{(o0 & kOutcomeAccepted) != 0u ? 1u : 0u, o0 & ~kOutcomeAccepted, vec2{__uint_as_float(o[1]), __uint_as_float(o[2])}, __uint_as_float(o[3])};
}
constexpr uint32_t kPrepTries = 8;   // tries of k_interact_c_prep: one per lane of a walk's group of eight
// WTGPU_PROFILE=3, pass C by aperture size (index into st.counters + kNumCounters, + bin = floor(log2(segments)) < 16): walks, tries, clock ticks of
// power sum + tries, of the commit and of fetch + load; the wide and hard tries of the tiers: ticks and walks
constexpr size_t kPassCProfWalks = 8, kPassCProfTries = 24, kPassCProfTicks = 40, kPassCProfCommitTicks = 96, kPassCProfLoadTicks = 112, kPassCProfWideTicks = 128,
                 kPassCProfWideWalks = 144;
WT_D int pass_c_prof_bin(uint32_t n_edges) { return 31 - __clz((int)max(n_edges, 1u)); }
// statistics of the tiers, behind the WTGPU_PROFILE slots proper (index into st.counters + kNumCounters): walks settled by the prep / wide / hard
// kernel, pass-C walks, rounds with a pass-C queue / whose queue is no multiple of kPrepTries / is shorter, the lengths of the first such queues
constexpr size_t kPassCTierSlot = 160, kPassCWalksSlot = 163, kPassCRoundsSlot = 164, kPassCQueueSlot = 168, kPassCQueueSlots = kProfSlots - kPassCQueueSlot;
// (block size as a constant: blockDim would pull 256 bytes of hidden kernel arguments into the kernel-argument segment)
WT_D void lds_stack(stack_entry_t* lds, stack_entry_t* spill, stack_ref_t& s, uint32_t block = kBlock) {
    s = make_stack_ref(lds + threadIdx.x, block, kLdsStack + kSpillStack, kLdsStack, spill);
}

WT_D void flush_counters(unsigned long long* g, const bdpt_counters_t& c) {
    const unsigned long long* p = reinterpret_cast<const unsigned long long*>(&c);
#pragma unroll
    for (size_t i = 0; i < kNumCounters; ++i) {
        unsigned long long v = p[i];
        // wave reduction (64 lanes)
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(&g[i], v);
    }
}

// walk id -> (sample index, stream)
WT_D void walk_ident(const launch_args_t& a, uint32_t w, uint32_t& i, uint32_t& stream) {
    if (w < a.st.cap) {
        i = w;
        stream = STREAM_SENSOR_WALK;
    } else {
        i = w - (uint32_t)a.st.cap;
        stream = STREAM_EMITTER_WALK;
    }
}
// The round queues hold the two kinds of walks apart: sensor walks are appended from the front of the array (count CTL_COUNT*), emitter
// walks from its end backwards (count CTL_BACK*).  A traversal costs an emitter walk of the headline workload 5-10x what it costs a
// sensor walk (wide beams from the spots against pixel-sized beams from the camera): wavefronts that hold one kind waste fewer lanes.
// queue item -> walk id; the first round's queue is the identity over [0,nb) (sensor walks) and [cap,cap+nb) (emitter walks)
WT_D uint32_t queue_count(const uint32_t* ctl, int in) { return ctl[CTL_COUNT0 + in] + ctl[CTL_BACK0 + in]; }
WT_D uint32_t queue_walk(const launch_args_t& a, const uint32_t* ctl, int in, uint32_t qi, int first_round) {
    if (first_round) return qi < a.nb ? qi : (uint32_t)a.st.cap + (qi - a.nb);
    const uint32_t front = ctl[CTL_COUNT0 + in];
    return qi < front ? a.st.queue[in][qi] : a.st.queue[in][2 * (size_t)a.st.cap - 1 - (qi - front)];
}
// The next `inc` entries of a device queue for one WAVEFRONT: lane 0 moves the head, every lane gets the old value.
// Until round 5 every persistent loop began with `if (threadIdx.x == 0) word = atomicAdd(head, 1); __syncthreads(); item = word; __syncthreads();`
// (one-wavefront blocks) or the same through a shuffle, and in round 5 that stopped k_path_fsd in one of two build layouts.  What
// the compiler did, read off the ISA: the loop body ENDS with `if (threadIdx.x == 0) result[w] = f;` and BEGINS with `if (threadIdx.x == 0)
// …atomicAdd…`; the two branches on the same condition were threaded across the back edge (lane 0: store, then atomic; the others: neither), the
// join — the read of the shared word / the readfirstlane — became the header of a loop with TWO back edges, these were split into nested loops,
// and the structuriser ran the inner one (lanes 1-63, which skip the atomic) to completion while lane 0 waited outside: 63 lanes re-read the
// same item (the stale shared word, or lane 1's zero) for ever.  The barriers of a one-wavefront block compile to nothing, so nothing stood in
// the way.  Two things stand in the way here: a convergent marker IN FRONT of the branch (a block that holds one is not duplicated, and
// threading an edge through the loop header means duplicating it), and a lane index the optimiser does not connect with threadIdx.x.
// (Measured alternatives, run r5n / r5o: every lane issues the atomic, lane 0 adding `inc` and the others 0 — correct, and 1 % of a pass slower:
// the compiler's scan over lane-dependent addends costs a wavefront-per-item kernel ~1 us per item; every lane adding 1 — free, but correct
// only where the compiler folds the 64 atomics into one, which it does for pointers it knows to be global and not for the chunk words of the
// staged connections: five parity tests failed.)
WT_D bool wave_first_lane() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) == 0u; }
WT_D uint32_t wave_grab0(uint32_t* head, uint32_t inc) {
    __builtin_amdgcn_wave_barrier();
    uint32_t old = 0;
    if (wave_first_lane()) old = atomicAdd(head, inc);
    __builtin_amdgcn_wave_barrier();
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)old);
}
WT_D uint32_t wave_grab(uint32_t* head) { return wave_grab0(head, 64u); }        // 64 queue items, one per lane: the first lane's
WT_D uint32_t wave_grab_item(uint32_t* head) { return wave_grab0(head, 1u); }    // one queue item for a one-wavefront block
// One value from lane 0 of a one-wavefront block to all of its lanes, for values that only lane 0 may compute (an allocation).  Call sites keep
// a convergent operation (a barrier, a shuffle) between this and any earlier `if (threadIdx.x == 0)`, see above.
WT_D uint32_t wave_bcast0(uint32_t v) {
    __builtin_amdgcn_wave_barrier();
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}
// wave-aggregated append of `w` (for lanes with `pred`) to a device queue
WT_D void wave_append(uint32_t* queue, uint32_t* count, bool pred, uint32_t w) {
    const unsigned long long m = __ballot(pred);
    if (!m) return;
    const int lane = threadIdx.x & 63;
    const int leader = __ffsll((long long)m) - 1;
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(count, (uint32_t)__popcll(m));
    base = (uint32_t)__shfl((int)base, leader, 64);
    if (pred) queue[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = w;
}

// ... of walk `w` (for lanes with `pred`) to round queue `out`: sensor walks (and plt_path's) at the front, emitter walks at the back
WT_D void queue_append(const launch_args_t& a, uint32_t* ctl, int out, bool pred, uint32_t w) {
    const bool back = pred && w >= a.st.cap && a.split_queues;
    wave_append(a.st.queue[out], ctl + CTL_COUNT0 + out, pred && !back, w);
    const unsigned long long m = __ballot(back);
    if (!m) return;
    const int lane = threadIdx.x & 63;
    const int leader = __ffsll((long long)m) - 1;
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(ctl + CTL_BACK0 + out, (uint32_t)__popcll(m));
    base = (uint32_t)__shfl((int)base, leader, 64);
    if (back) a.st.queue[out][2 * (size_t)a.st.cap - 1 - (base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull)))] = w;
}

// ---- the work-item vocabulary of the walk, path and connection kernels ------------------------------------------------------------------------
// What every kernel form does with a queue item before its own logic starts, written once: straight-line code, called from INSIDE the persistent
// loops (the `for (;;)`, the grab and the `break` stay written out in each kernel, see wave_grab0).
// sample i of the batch -> the id its random streams are keyed by; `pix`: its sensor element
WT_D uint64_t sample_id_of(const launch_args_t& a, uint32_t i, uint32_t& pix) {
    const uint64_t j = a.j0 + i;
    pix = (uint32_t)(j % a.npix);
    const uint64_t smp = a.sample_begin + j / a.npix;
    return ((uint64_t)pix << 32) | (smp & 0xFFFFFFFFull);
}
WT_D uint64_t sample_id_of(const launch_args_t& a, uint32_t i) {
    uint32_t pix;
    return sample_id_of(a, i, pix);
}
WT_D fsd_pool_t fsd_pool_of(const launch_args_t& a) {
    return fsd_pool_t{a.st.fsd_hdr, a.st.fsd_edges, a.st.ctl + CTL_FSD_COUNTER, a.st.fsd_cap, a.st.ctl + CTL_FSD_ECOUNTER, a.st.fsd_ecap};
}
// the vertex array of walk w; of sample i's sensor / emitter subpath
WT_D vertex_store_t walk_vertices(const launch_args_t& a, size_t w) { return vertex_store_t{a.st.verts, a.st.vert_words, w}; }
WT_D vertex_store_t sensor_vertices(const launch_args_t& a, uint32_t i) { return walk_vertices(a, i); }
WT_D vertex_store_t emitter_vertices(const launch_args_t& a, uint32_t i) { return walk_vertices(a, (size_t)a.st.cap + i); }
// Item idx of a flattened bucket space -> its bucket: the LAST key of [0, n) whose prefix is <= idx (prefix[0] = 0; empty buckets share their
// successor's prefix and are never the last).  Class form: the table is by rank and every class starts at a multiple of 64, so the 64 items of
// a grab have the bucket of the first.  (always_inline: left to itself the compiler made it a CALL in k_connect_strat, the table a flat pointer.)
__host__ __device__ constexpr __attribute__((always_inline)) uint32_t bucket_of(const uint32_t* prefix, uint32_t idx, uint32_t n = kNumKeys) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (prefix[mid] <= idx)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}
namespace bucket_of_check {
constexpr uint32_t front[] = {0, 0, 0, 3, 5};          // keys 0, 1 empty; 2: [0,3); 3: [3,5)
constexpr uint32_t middle[] = {0, 2, 2, 2, 5};         // 0: [0,2); 1, 2 empty; 3: [2,5)
constexpr uint32_t back[] = {0, 3, 5, 5, 5};           // 0: [0,3); 1: [3,5); 2, 3 empty
constexpr uint32_t ranks[] = {0, 64, 64, 192, 256};    // class form: 64 items, none, 128, 64
static_assert(bucket_of(front, 0, 4) == 2 && bucket_of(front, 2, 4) == 2 && bucket_of(front, 3, 4) == 3 && bucket_of(front, 4, 4) == 3, "empty buckets at the front");
static_assert(bucket_of(middle, 0, 4) == 0 && bucket_of(middle, 1, 4) == 0 && bucket_of(middle, 2, 4) == 3 && bucket_of(middle, 4, 4) == 3, "empty buckets in the middle");
static_assert(bucket_of(back, 0, 4) == 0 && bucket_of(back, 2, 4) == 0 && bucket_of(back, 3, 4) == 1 && bucket_of(back, 4, 4) == 1, "empty buckets at the end");
static_assert(bucket_of(ranks, 0, 4) == 0 && bucket_of(ranks, 64, 4) == 2 && bucket_of(ranks, 128, 4) == 2 && bucket_of(ranks, 192, 4) == 3, "classes start at multiples of 64");
static_assert(bucket_of(front, 0, 1) == 0, "one key");
}   // namespace bucket_of_check
// index of a counter in st.counters; one counter summed over the wavefront, added by lane 0.  (Kernels that touch two or three counters zero and
// flush those alone: flush_counters over all of them costs registers.)
#define WT_COUNTER_SLOT(field) (offsetof(bdpt_counters_t, field) / sizeof(unsigned long long))
WT_D void flush_counter(const launch_args_t& a, size_t slot, unsigned long long v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(a.st.counters + slot, v);
}
// one word of walk w's traversal record, as it is / as a float (macros: `field` is a member of trav_result_t, not an expression; WT_TRAV_U is an
// lvalue: `WT_TRAV_U(a, w, tuid) = marker`)
WT_D uint32_t& trav_word(const launch_args_t& a, uint32_t w, size_t word) { return a.st.trav[(size_t)w * kTravWords + word]; }
#define WT_TRAV_U(a, w, field) trav_word(a, w, WT_TRAV_WORD(field))
#define WT_TRAV_F(a, w, field) __uint_as_float(WT_TRAV_U(a, w, field))
WT_D vec3 trav_origin(const launch_args_t& a, uint32_t w) { return vec3{WT_TRAV_F(a, w, origin.x), WT_TRAV_F(a, w, origin.y), WT_TRAV_F(a, w, origin.z)}; }
// The classified-edge ids coop_gather left behind (g, eg) -> a block of the round's edge pool, sorted: any number of them in bitmap mode, the sorted
// 96-entry list for scenes with more than kCoopEdgeBits classified edges.  (Until round 4 that list went into the walk's triangle-list slot, which a
// later pass may still read as triangles.)  Returns the block's offset; n_edges: ids written, dropped: ids lost.  One wavefront, all lanes.
WT_D uint32_t edges_to_pool(const launch_args_t& a, const gather_out_t& g, coop_edges_t& eg, uint32_t& n_edges, uint32_t& dropped) {
    const bool bitmap = a.sc.n_edges <= kCoopEdgeBits;
    n_edges = bitmap ? coop_edge_count(a.sc, eg) : g.n_edges;
    dropped = bitmap ? 0u : g.edge_overflow;
    const uint32_t off = wave_grab0(a.st.ctl + CTL_EPOOL_COUNT, n_edges);
    if (off + n_edges > a.st.epool_cap) {   // pool exhausted (8M ids per round): reported, cannot happen in the shipped scenes
        dropped += n_edges;
        n_edges = 0;
    } else if (bitmap)
        coop_edge_write(a.sc, eg, a.st.epool + off, n_edges);
    else
        for (uint32_t j = threadIdx.x; j < n_edges; j += 64) a.st.epool[off + j] = eg.edge_ids[j];
    return off;
}
// a batch begins: every queue empty, every head and bump allocator at 0 (the generate kernels then set CTL_COUNT0, the first round's queue)
WT_D void ctl_reset_batch(uint32_t* ctl) {
    ctl[CTL_COUNT1] = 0;
    ctl[CTL_BACK0] = ctl[CTL_BACK1] = 0;
    ctl[CTL_UTD_COUNT0] = ctl[CTL_UTD_COUNT1] = ctl[CTL_FSDQ_COUNT0] = ctl[CTL_FSDQ_COUNT1] = ctl[CTL_FSDQ_HEAD] = ctl[CTL_NEEQ_COUNT] = ctl[CTL_NEEQ_HEAD] = 0;   // plt_path's
    ctl[CTL_HEAD_TRACE] = ctl[CTL_HEAD_INTERACT] = ctl[CTL_HEAVY_COUNT] = ctl[CTL_HEAVY_HEAD] = ctl[CTL_FSD_COUNTER] = ctl[CTL_ROUNDS] = 0;
    ctl[CTL_TPOL_COUNT0] = ctl[CTL_TPOL_COUNT1] = ctl[CTL_TPOL_HEAD] = ctl[CTL_TCONE_COUNT0] = ctl[CTL_TCONE_COUNT1] = ctl[CTL_TCONE_HEAD] = 0;   // the staged trace kernels' queues
    ctl[CTL_INTB_COUNT] = ctl[CTL_INTB_HEAD] = ctl[CTL_GATHER_COUNT] = ctl[CTL_GATHER_HEAD] = ctl[CTL_INTC_COUNT] = ctl[CTL_INTC_HEAD] = 0;
    ctl[CTL_FTASK_COUNT] = ctl[CTL_FTASK_HEAD] = ctl[CTL_FSPLIT_HEAD] = ctl[CTL_EPOOL_COUNT] = ctl[CTL_FSD_ECOUNTER] = 0;
    ctl[CTL_INTD_COUNT] = ctl[CTL_INTD_HEAD] = 0;
    ctl[CTL_PCW_COUNT] = ctl[CTL_PCW_HEAD] = ctl[CTL_PCC_COUNT] = ctl[CTL_PCC_HEAD] = 0;
}
// pass A of a round begins (one lane of the grid): the trace queues are ready for the NEXT round's k_trace
WT_D void interact_round_begin(uint32_t* ctl) {
    ctl[CTL_HEAVY_COUNT] = 0;
    ctl[CTL_HEAVY_HEAD] = 0;
    ctl[CTL_HEAD_TRACE] = 0;
}

// ---- wave-cooperative record transfer -------------------------------------------------------------------------------------------------------
// The per-walk records are record-major in memory (one contiguous record per walk) and the walks a wavefront holds are scattered over the batch.
// A lane that loads its own record word by word makes every load INSTRUCTION touch 64 different cache lines for 4 bytes each (57 instructions x
// 64 lines for a walk); a lane that stores its record word by word leaves 64 partially written lines behind every instruction, which the L2
// evicts before the other 85 words of a vertex arrive (measured, run r5g: k_interact moves 82 GB per step for 13 GB of records).  Here the
// wavefront moves the records of its lanes ONE RECORD AT A TIME, consecutive lanes on consecutive words (a 228-byte walk = one instruction
// touching 2-3 lines), through an LDS buffer of kIoRows rows that the owning lanes then read / have written row-wise (odd pitch: no bank
// conflicts): 64 x 3 line visits instead of 57 x 64.  Half a wavefront at a time, so that the buffer is 11 KB per wavefront.
constexpr int kIoRows = 32;
template <int W>
constexpr int io_pitch() { return (W & 1) ? W : W + 1; }
// `idx`: the lane's record, `valid`: the lane takes part; lds: this wavefront's buffer (>= kIoRows * io_pitch<W>() words)
template <int W, class T>
WT_D void wave_load_records(const uint32_t* base, size_t stride, uint32_t idx, bool valid, uint32_t* lds, T& out) {
    static_assert(sizeof(T) == 4 * W, "record size");
    constexpr int P = io_pitch<W>();
    const int lane = threadIdx.x & 63;
    uint32_t* o = reinterpret_cast<uint32_t*>(&out);
    const unsigned long long all = __ballot(valid);
#pragma unroll 1
    for (int h = 0; h < 2; ++h) {
        unsigned long long m = all & (h ? 0xFFFFFFFF00000000ull : 0x00000000FFFFFFFFull);
        while (m) {
            const int r = __ffsll((long long)m) - 1;
            m &= m - 1;
            const uint32_t* src = base + (size_t)__builtin_amdgcn_readlane(idx, r) * stride;
#pragma unroll
            for (int w0 = 0; w0 < W; w0 += 64)
                if (w0 + lane < W) lds[(r & 31) * P + w0 + lane] = src[w0 + lane];
        }
        __builtin_amdgcn_wave_barrier();
        if (valid && (lane >> 5) == h) {
#pragma unroll
            for (int i = 0; i < W; ++i) o[i] = lds[(lane & 31) * P + i];
        }
        __builtin_amdgcn_wave_barrier();
    }
}
// ... `off`: word offset of the lane's record behind base + idx * stride (a vertex of the walk's vertex array)
template <int W, class T>
WT_D void wave_store_records(uint32_t* base, size_t stride, uint32_t idx, uint32_t off, bool valid, uint32_t* lds, const T& in) {
    static_assert(sizeof(T) == 4 * W, "record size");
    constexpr int P = io_pitch<W>();
    const int lane = threadIdx.x & 63;
    const uint32_t* o = reinterpret_cast<const uint32_t*>(&in);
    const unsigned long long all = __ballot(valid);
    if (!all) return;
#pragma unroll 1
    for (int h = 0; h < 2; ++h) {
        if (valid && (lane >> 5) == h) {
#pragma unroll
            for (int i = 0; i < W; ++i) lds[(lane & 31) * P + i] = o[i];
        }
        __builtin_amdgcn_wave_barrier();
        unsigned long long m = all & (h ? 0xFFFFFFFF00000000ull : 0x00000000FFFFFFFFull);
        while (m) {
            const int r = __ffsll((long long)m) - 1;
            m &= m - 1;
            uint32_t* dst = base + (size_t)__builtin_amdgcn_readlane(idx, r) * stride + __builtin_amdgcn_readlane(off, r);
#pragma unroll
            for (int w0 = 0; w0 < W; w0 += 64)
                if (w0 + lane < W) dst[w0 + lane] = lds[(r & 31) * P + w0 + lane];
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// ---- kernels (definitions: kernels_*.hip)
constexpr uint32_t kFlushGrid = 64;          // k_path_flush
constexpr int kEnumBlock = 1024;             // k_connect_enum
constexpr uint32_t kSplatBlock = 64, kSplatCols = kSplatBlock + 2;  // k_connect_splat_tiled: elements of a row segment (one wavefront), columns of its LDS tile
// ... and the launches its blocks are spread over: phase = 2 x (row % 3) + (segment % 2).  A block's tile reaches one row up and down and one
// column left and right, so two blocks of one phase — at least three rows or two segments apart — never touch the same film element, and the up to
// six tiles that meet in an element are added in the order of the phases.  Grid of a phase: splat_phase_rows x splat_phase_segments blocks.
constexpr uint32_t kSplatPhases = 6;
__host__ __device__ constexpr uint32_t splat_segments(uint32_t width) { return (width + kSplatBlock - 1) / kSplatBlock; }
__host__ __device__ constexpr uint32_t splat_phase_rows(uint32_t phase, uint32_t height) { return (height + 2u - phase / 2u) / 3u; }        // rows phase / 2, + 3, ... below height
__host__ __device__ constexpr uint32_t splat_phase_segments(uint32_t phase, uint32_t segs) { return (segs + 1u - (phase & 1u)) / 2u; }    // segments phase % 2, + 2, ... below segs
__host__ __device__ constexpr uint32_t splat_block_row(uint32_t phase, uint32_t block, uint32_t phase_segs) { return phase / 2u + 3u * (block / phase_segs); }
__host__ __device__ constexpr uint32_t splat_block_segment(uint32_t phase, uint32_t block, uint32_t phase_segs) { return (phase & 1u) + 2u * (block % phase_segs); }
// every (row, segment) of a height x segs film belongs to exactly one block of exactly one phase, and no grid reaches outside the film
__host__ __device__ constexpr bool splat_phases_cover(uint32_t height, uint32_t segs) {
    uint32_t seen[8 * 8] = {};
    for (uint32_t phase = 0; phase < kSplatPhases; ++phase) {
        const uint32_t ps = splat_phase_segments(phase, segs), n = splat_phase_rows(phase, height) * ps;
        for (uint32_t b = 0; b < n; ++b) {
            const uint32_t r = splat_block_row(phase, b, ps), s = splat_block_segment(phase, b, ps);
            if (r >= height || s >= segs || r % 3u != phase / 2u || s % 2u != (phase & 1u)) return false;
            ++seen[r * 8 + s];
        }
    }
    for (uint32_t r = 0; r < height; ++r)
        for (uint32_t s = 0; s < segs; ++s)
            if (seen[r * 8 + s] != 1) return false;
    return true;
}
static_assert(splat_phases_cover(1, 1) && splat_phases_cover(2, 1) && splat_phases_cover(3, 2) && splat_phases_cover(4, 2) && splat_phases_cover(5, 3) && splat_phases_cover(6, 4) &&
              splat_phases_cover(7, 5) && splat_phases_cover(8, 8) && splat_phases_cover(7, 1) && splat_phases_cover(1, 6),
              "heights 0, 1, 2 mod 3; even and odd segment counts");
static_assert(splat_segments(1) == 1 && splat_segments(64) == 1 && splat_segments(65) == 2 && splat_segments(1440) == 23 && splat_segments(1920) == 30, "segments of a row");
#ifndef WTGPU_HARD_BLOCK
#define WTGPU_HARD_BLOCK 256
#endif
__global__ void k_generate(launch_args_t a);
__global__ void k_trace_refill(launch_args_t a, int in, int first_round, uint32_t round);
__global__ void k_trace_sm(launch_args_t a, int in, int first_round, uint32_t round);
__global__ void k_tr_axis(launch_args_t a, int in, int first_round, uint32_t round);
__global__ void k_tr_cone(launch_args_t a, uint32_t it);
__global__ void k_tr_policy(launch_args_t a, uint32_t it);
__global__ void k_tr_tail(launch_args_t a, uint32_t it);
__global__ void k_trace_heavy(launch_args_t a);
__global__ void k_trace_heavy_prof(launch_args_t a);   // the same with the phase clocks of WTGPU_PROFILE=2
__global__ void k_interact(launch_args_t a, int in, int first_round);
__global__ void k_classify(launch_args_t a, int in, int first_round);
__global__ void k_interact_diffuse(launch_args_t a, int in);
__global__ void k_interact_dielectric(launch_args_t a, int in);
__global__ void k_interact_spm(launch_args_t a, int in);
__global__ void k_interact_any(launch_args_t a, int in);
__global__ void k_interact_sorted(launch_args_t a, int in);
__global__ void k_interact_coop(launch_args_t a, int in, int first_round);
__global__ void k_edges(launch_args_t a);
__global__ void k_interact_b(launch_args_t a, int in);
__global__ void k_light_rounds(launch_args_t a, int in, uint32_t round, uint32_t max_rounds);
__global__ void k_flux_split(launch_args_t a);
__global__ void k_flux_tasks(launch_args_t a);
__global__ void k_interact_c(launch_args_t a, int in);
__global__ void k_interact_c_hard(launch_args_t a, int in);
__global__ void k_interact_c_prep(launch_args_t a, uint32_t thin_below, uint32_t easy_tries);
__global__ void k_interact_c_wide(launch_args_t a, uint32_t easy_tries);
__global__ void k_interact_c_hard_tries(launch_args_t a, uint32_t easy_tries);
__global__ void k_interact_c_commit(launch_args_t a, int in);
__global__ void k_path_generate(launch_args_t a);
__global__ void k_path_fsd(launch_args_t a, const path_state_t* __restrict__ ps, uint32_t round);
__global__ void k_path_edges(launch_args_t a, const path_state_t* __restrict__ ps);
__global__ void k_path_interact(launch_args_t a, const path_state_t* __restrict__ ps, int in, int first_round, uint32_t round);
__global__ void k_path_interact_b(launch_args_t a, const path_state_t* __restrict__ ps, int in, uint32_t round);
__global__ void k_path_nee(launch_args_t a, const path_state_t* __restrict__ ps, uint32_t round);
__global__ void k_path_flush(launch_args_t a, int in);
__global__ void k_connect_enum(launch_args_t a, uint32_t by_class);
__global__ void k_connect_scan(launch_args_t a, uint32_t by_class);
__global__ void k_connect_strat(launch_args_t a);
__global__ void k_connect_strat_open(launch_args_t a);
__global__ void k_connect_class(launch_args_t a);
__global__ void k_connect_class_open(launch_args_t a);
__global__ void k_connect_eval(launch_args_t a, uint32_t chunk);
__global__ void k_connect_shadow(launch_args_t a, uint32_t chunk);
__global__ void k_connect_mis(launch_args_t a, uint32_t chunk);
__global__ void k_connect_splat(launch_args_t a);
__global__ void k_connect_splat_tiled(launch_args_t a, uint32_t phase);
__global__ void k_calib_copy(const uint32_t* in, uint32_t* out, size_t n);
__global__ void k_trace_rays(scene_t sc, const float* rays, uint32_t n, float* dist, uint32_t* tuid, float* bary, uint32_t* front);
__global__ void k_traverse_cones(scene_t sc, const float* cones, uint32_t n, uint32_t cap, float* dist, uint32_t* flags, uint32_t* ntris, uint32_t* out_tris,
                                 uint32_t* scratch_tris);
__global__ void k_query_regions(scene_t sc, const float* cones, uint32_t n, uint32_t edge_cap, float* dist, uint32_t* flags, uint32_t* primary, uint32_t* ntris,
                                uint32_t* nedges, uint32_t* edges, float* flux, unsigned long long* dropped);
// kernels_test.hip: launches of the test entry points (wtgpu_test_hooks.h); return a hipError_t
int test_fsd_apertures(const scene_t& sc, hipStream_t stream, const float* d_cones, const float* d_sk, const uint32_t* d_ids, const uint32_t* d_n_ids,
                       uint32_t n, uint32_t id_cap, uint32_t pool_cap, uint32_t mode, uint32_t* d_hdr, float* d_segs);
int test_utd_sums(const scene_t& sc, hipStream_t stream, const float* d_queries, const uint32_t* d_ids, const uint32_t* d_n_ids, uint32_t n, uint32_t id_cap,
                  uint32_t utd_cap, uint32_t* d_recs, uint32_t* d_hdr, uint32_t* d_edges);
int test_bsdf_queries(const scene_t& sc, hipStream_t stream, const uint32_t* d_queries, uint32_t n, int form, uint32_t* d_out);
int test_source_queries(const scene_t& sc, hipStream_t stream, const uint32_t* d_queries, uint32_t n, uint32_t* d_out);
int test_flux_queries(const scene_t& sc, hipStream_t stream, const uint32_t* d_queries, uint32_t n, uint32_t* d_out);
// kernels_mask.hip: by-geometry sensor masks (wtgpu_sensor_mask / wtgpu_sensor_mask_host).  shape_matches: one byte per shape, 1 = the id matches
// the mask's regex.  The launch returns a hipError_t.
int sensor_mask_launch(const scene_t& sc, hipStream_t stream, const uint8_t* d_shape_matches, uint32_t samples, uint64_t seed, float* d_out);
void sensor_mask_host(const scene_t& sc, const uint8_t* shape_matches, uint32_t samples, uint64_t seed, uint32_t n_threads, float* out);
// kernels_firsthit.hip: first-hit maps of a perspective sensor (wtgpu_first_hit / wtgpu_first_hit_host; wt/first_hit.h).  maps / ids: the bits of
// wtgpu_first_hit_spec; d_maps: [height][width][fh_map_floats(maps)] f32, d_ids: [height][width][fh_id_words(ids)] u32, each may be null when no
// bit of its group is set.  samples 0: the ray through the pixel's centre.  per_sample: the measured alternative (WTGPU_FIRST_HIT_PER_SAMPLE).  The launch
// returns a hipError_t.
int first_hit_launch(const scene_t& sc, hipStream_t stream, uint32_t samples, uint64_t seed, uint32_t maps, uint32_t ids, uint32_t per_sample, float* d_maps,
                     uint32_t* d_ids);
void first_hit_host(const scene_t& sc, uint32_t samples, uint64_t seed, uint32_t maps, uint32_t ids, uint32_t n_threads, float* out_maps, uint32_t* out_ids);
// kernels_firsthit_material.hip: first-hit material maps of a perspective sensor (wtgpu_first_hit_material / wtgpu_first_hit_material_host;
// wt/first_hit_material.h).  q: the spec after its checks; d_maps: [height][width][fhm_map_floats(q.maps, q.n_k)] f32, d_ids:
// [height][width][fhm_id_words(q.ids)] u32, each may be null when no bit of its group is set.  per_sample: WTGPU_FIRST_HIT_PER_SAMPLE, as
// first_hit_launch.  The launch returns a hipError_t.
int first_hit_material_launch(const scene_t& sc, hipStream_t stream, const fhm_query_t& q, uint32_t per_sample, float* d_maps, uint32_t* d_ids);
void first_hit_material_host(const scene_t& sc, const fhm_query_t& q, uint32_t n_threads, float* out_maps, uint32_t* out_ids);
// kernels_los.hip: line-of-sight maps (wtgpu_line_of_sight / wtgpu_line_of_sight_host; wt/los.h).  q: the spec after its checks, the selection resolved,
// 1 .. 32 emitters; its points / normals / mask and d_maps [height][width][E][los_map_floats], d_elem [height][width][los_elem_floats], d_ids
// [height][width][los_id_words] are device memory for the launch and host memory for the twin, each may be null when no bit of its group is set.
// per_sample: the measured alternative (WTGPU_LOS_PER_SAMPLE).  The launch returns a hipError_t.
int los_launch(const scene_t& sc, hipStream_t stream, const los_query_t& q, uint32_t per_sample, float* d_maps, float* d_elem, uint32_t* d_ids);
void los_host(const scene_t& sc, const los_query_t& q, uint32_t n_threads, float* out_maps, float* out_elem, uint32_t* out_ids);
// kernels_develop.hip: film development and tonemapping (wtgpu_develop_device / wtgpu_tonemap_device / wtgpu_tonemap_host).  Films as wtgpu_render
// fills them, or — the passes that take a wtgpu_film_source, here and below — a developed f32 film, one of the two after the entry point's check
// (film_source_check; device memory for a launch, host memory for a twin); `t.table` is a DEVICE pointer for the launch and a host pointer for the
// host twin; s: the Stokes component; d_mask: null, or one f32 per pixel that becomes the fourth component.  per_pixel / lds_table: the measured alternatives (WTGPU_DEVELOP_PER_PIXEL, WTGPU_TONEMAP_LDS_TABLE).
// The launches return a hipError_t.
constexpr uint32_t kMaxTonemapTable = 1024;   // entries of a colour table
int develop_launch(const sensor_t& sn, hipStream_t stream, const double* d_value, const double* d_weight, const double* d_light, uint64_t spe,
                   uint32_t per_pixel, float* d_out);
int develop_tonemap_launch(const sensor_t& sn, hipStream_t stream, const wtgpu_film_source& film, const tonemap_args_t& t, uint32_t s, const float* d_mask, uint32_t format, uint32_t lds_table, void* d_out);
void develop_tonemap_host(const sensor_t& sn, const wtgpu_film_source& film, const tonemap_args_t& t, uint32_t s,
                          const float* mask, uint32_t format, uint32_t n_threads, void* out);
// kernels_stats.hip: film statistics (wtgpu_film_stats_device / wtgpu_film_stats_host; wt/film_stats.h).  Films as wtgpu_render fills them; s: the Stokes
// component; flags: FS_ABS | FS_LUMINANCE; edges: bins + 1 thresholds (DEVICE for the launch); rec: film_stats_rec_t per plane and hist: [planes][bins],
// both ZEROED by the caller of the launch (the host twin clears its own); d_sums: kFsMaxPlanes x fs_scratch_len(pixels) doubles.  Two kernels on
// `stream`; the launch returns a hipError_t.
int film_stats_launch(const sensor_t& sn, hipStream_t stream, uint32_t n_cus, const wtgpu_film_source& film, uint32_t s, uint32_t flags, const float* d_mask, const float* d_edges, uint32_t bins, void* d_rec, unsigned long long* d_hist, double* d_sums);
void film_stats_host(const sensor_t& sn, const wtgpu_film_source& film, uint32_t s, uint32_t flags, const float* mask,
                     const float* edges, uint32_t bins, uint32_t n_threads, void* out_rec, unsigned long long* out_hist);
// kernels_zonal.hip: zonal film statistics (wtgpu_film_zonal_device / wtgpu_film_zonal_host; wt/film_zonal.h).  A film source as above; d_zones: [height][width]
// u32; edges as for the statistics; n_zones: 1 .. 65536.  lds_form: 1 the LDS form (only where film_zonal_lds_fits), 0 the global form; max_blocks: WTGPU_FILM_ZONAL_BLOCKS.  d_slots: film_zonal_slot_t per
// (zone, plane), d_hist: [n_zones][planes][bins] and d_outside: one count, all three ZEROED by the caller of the launch; d_rec: film_zonal_rec_t per
// (zone, plane), every field written; d_paint: null or [height][width][planes] f32.  Two or three kernels on `stream`; the launch returns a hipError_t.
// film_zonal_lds_fits: whether the LDS form's table of a call fits the 64 KB a launch may ask for.
bool film_zonal_lds_fits(uint32_t n_zones, uint32_t planes, uint32_t bins);
int film_zonal_launch(const sensor_t& sn, hipStream_t stream, uint32_t n_cus, const wtgpu_film_source& film, uint32_t s, uint32_t flags, const uint32_t* d_zones, const float* d_mask,
                      const float* d_edges, uint32_t bins, uint32_t n_zones, uint32_t lds_form, uint32_t max_blocks, void* d_slots, unsigned long long* d_hist,
                      unsigned long long* d_outside, void* d_rec, float* d_paint);
void film_zonal_host(const sensor_t& sn, const wtgpu_film_source& film, uint32_t s, uint32_t flags, const uint32_t* zones, const float* mask, const float* edges, uint32_t bins,
                     uint32_t n_zones, uint32_t n_threads, void* out_rec, unsigned long long* out_hist, unsigned long long* out_outside, float* paint);
// kernels_segments.hip: connected segments of a label plane (wtgpu_film_segments_device / wtgpu_film_segments_host; wt/film_segments.h).  d_classes: null or
// [height][width] u32; d_mask: null or [height][width] f32; flags: SEG_DIAGONAL; d_segments: [height][width] u32, every pixel written.  d_head: kSegHeadBytes
// (n_segments, n_dropped, n_members, n_dropped_pixels as u64, then the overflow word: not zero where a union-find loop hit its step bound, and the plane
// is then not to be read); d_records: max_records film_segment_t, of which the first min(n_segments, max_records) are written; d_work:
// film_segments_scratch_words(pixels) u32.  tiled: the form of the first two phases, 1 k_seg_tile + k_seg_border, 0 k_seg_runs + k_seg_merge (WTGPU_FILM_SEGMENTS_TILED).  The launch clears what has to be cleared.  Two memsets and seven kernels on `stream`; returns a hipError_t.
constexpr size_t kSegHeadBytes = 48;
uint64_t film_segments_scratch_words(uint64_t npix);
int film_segments_launch(const sensor_t& sn, hipStream_t stream, uint32_t n_cus, uint32_t tiled, uint32_t flags, uint32_t min_area, uint32_t max_records, const uint32_t* d_classes,
                         const float* d_mask, uint32_t* d_segments, void* d_head, void* d_records, uint32_t* d_work);
// info: the four u64 of wtgpu_film_segments_info; out_records: max_records film_segment_t (may be null with max_records == 0)
void film_segments_host(const sensor_t& sn, uint32_t flags, uint32_t min_area, uint32_t max_records, const uint32_t* classes, const float* mask, uint32_t n_threads,
                        uint32_t* segments, unsigned long long* info, void* out_records);
// the kernels' find by itself on the host: up parent[] from x with at most `bound` loads; overflow is set where the bound is hit or a parent lies above its child
uint32_t film_segments_find_host(const uint32_t* parent, uint32_t x, uint32_t bound, bool& overflow);
// kernels_distance.hip: distance transform of a label plane (wtgpu_film_distance_device / wtgpu_film_distance_host; wt/film_distance.h).  d_classes: null or
// [height][width] u32; d_mask: null or [height][width] f32; flags: DIST_INVERT; d_dist2: [height][width] u32, every pixel written; d_nearest: null or the
// same.  d_head: kDistHeadBytes (n_sites u64, then the key of the maximum: max d² << 32 | ~argmax); d_work: film_distance_scratch_bytes(width, height)
// bytes, aligned to 16.  groups: the form of k_dist_rows, 1 with the group level, 0 the outward search alone (WTGPU_FILM_DISTANCE_GROUPS).  The launch
// clears what has to be cleared.  One memset and two kernels on `stream`; returns a hipError_t.
constexpr size_t kDistHeadBytes = 32;
uint64_t film_distance_scratch_bytes(uint32_t width, uint32_t height);
int film_distance_launch(const sensor_t& sn, hipStream_t stream, uint32_t groups, uint32_t flags, const uint32_t* d_classes, const float* d_mask, uint32_t* d_dist2,
                         uint32_t* d_nearest, void* d_head, void* d_work);
// nearest may be null; info: n_sites, argmax, max_dist2
void film_distance_host(const sensor_t& sn, uint32_t flags, const uint32_t* classes, const float* mask, uint32_t n_threads, uint32_t* dist2, uint32_t* nearest,
                        unsigned long long* info);
// kernels_compare.hip: comparison of two films (wtgpu_film_compare_device / wtgpu_film_compare_host; wt/film_compare.h).  Two sets of films as wtgpu_render fills
// them (the same pointers twice are fine); s: the Stokes component; flags: FS_ABS | FS_LUMINANCE; eps: finite, > 0.  d_rec: film_compare_rec_t per plane;
// d_sums: kFsMaxPlanes x kFcSums x fs_scratch_len(pixels) doubles; d_wave: film_rec_wave_bytes(pixels, n_cus) bytes (the polarisation view's too) — none of them has to be
// cleared; d_diff: null or [height][width][planes] f32.  Two kernels on `stream`; the launch returns a hipError_t.
size_t film_rec_wave_bytes(uint64_t npix, uint32_t n_cus);
int film_compare_launch(const sensor_t& sn, hipStream_t stream, uint32_t n_cus, const wtgpu_film_source& a, const wtgpu_film_source& b, uint32_t s, uint32_t flags, double eps, const float* d_mask,
                        void* d_rec, double* d_sums, void* d_wave, float* d_diff);
void film_compare_host(const sensor_t& sn, const wtgpu_film_source& a, const wtgpu_film_source& b, uint32_t s, uint32_t flags, double eps, const float* mask, uint32_t n_threads,
                       void* out_rec, float* diff);
// kernels_polar.hip: the polarisation view of a Stokes film (wtgpu_film_polar_device / wtgpu_film_polar_host; wt/film_polar.h).  Films of a polarimetric
// sensor as wtgpu_render fills them; flags: FP_LUMINANCE; a: the analyser, the maps' bits and the picture's plane, format and operator.  d_rec:
// film_polar_rec_t per plane; d_sums: kFsMaxPlanes x kFpSums x fs_scratch_len(pixels) doubles; d_wave: film_rec_wave_bytes(pixels, n_cus) bytes — none of
// them has to be cleared; d_maps: null or [height][width][planes][a.n_maps] f32; d_picture: null or [height][width][3, or 4 with a mask] in a.format.
// staged: the measured alternative (WTGPU_FILM_POLAR_STAGED).  Two kernels on `stream`; the launch returns a hipError_t.
int film_polar_launch(const sensor_t& sn, hipStream_t stream, uint32_t n_cus, const wtgpu_film_source& film, uint32_t flags, const film_polar_args_t& a, uint32_t staged, const float* d_mask, void* d_rec, double* d_sums, void* d_wave, float* d_maps,
                      void* d_picture);
void film_polar_host(const sensor_t& sn, const wtgpu_film_source& film, uint32_t flags, const film_polar_args_t& a,
                     const float* mask, uint32_t n_threads, void* out_rec, float* maps, void* picture);
// kernels_denoise.hip: the dual-buffer non-local-means filter of two half-films (wtgpu_film_denoise_device / wtgpu_film_denoise_host; wt/film_denoise.h).
// Two film sets as wtgpu_render fills them (they may be the same memory); a: the radii, k x k, alpha, eps and the patch norm.  d_scratch:
// film_denoise_scratch_floats(sn) floats, none of which has to be cleared; d_out, d_residual (may be null): [height][width][planes] f32.  fused: both
// directions in one launch of k_denoise_filter (1) or one launch each (0); WTGPU_FILM_DENOISE_FUSED, whose default chooses by the film's planes.  Three or four kernels on `stream`; the launch
// returns a hipError_t.  film_denoise_exp2_neg: wt/film_denoise.h's dn_exp2_neg element by element, for the test of its bound.
size_t film_denoise_scratch_floats(const sensor_t& sn);
int film_denoise_launch(const sensor_t& sn, hipStream_t stream, const double* a_value, const double* a_weight, const double* a_light, uint64_t spe_a,
                        const double* b_value, const double* b_weight, const double* b_light, uint64_t spe_b, const film_denoise_args_t& a, uint32_t fused,
                        const float* d_mask, float* d_scratch, float* d_out, float* d_residual);
void film_denoise_host(const sensor_t& sn, const double* a_value, const double* a_weight, const double* a_light, uint64_t spe_a, const double* b_value,
                       const double* b_weight, const double* b_light, uint64_t spe_b, const film_denoise_args_t& a, const float* mask, uint32_t n_threads,
                       float* out, float* residual, const film_denoise_guides_t* gd = nullptr, const float* guide = nullptr, const uint32_t* ids = nullptr);
// The guided filter (wtgpu_film_denoise_guided_*; wt/film_denoise.h "Guides"): gd the plane count, flags and scales; d_guide [height][width][gd.n] f32
// (null iff gd.n == 0), d_ids [height][width] u32 (null iff not SAME_ID); guide_lds: WTGPU_FILM_DENOISE_GUIDE_LDS (1: the candidate square's guide planes
// in LDS where they fit into 64 KB beside the rest, else and with 0 from global memory).  The host twin takes the same three through its last arguments.
int film_denoise_guided_launch(const sensor_t& sn, hipStream_t stream, const double* a_value, const double* a_weight, const double* a_light, uint64_t spe_a,
                               const double* b_value, const double* b_weight, const double* b_light, uint64_t spe_b, const film_denoise_args_t& a, uint32_t fused,
                               const film_denoise_guides_t& gd, uint32_t guide_lds, const float* d_guide, const uint32_t* d_ids, const float* d_mask,
                               float* d_scratch, float* d_out, float* d_residual);
void film_denoise_exp2_neg(const float* t, uint64_t n, float* out);

}   // namespace wtk
using namespace wtk;
