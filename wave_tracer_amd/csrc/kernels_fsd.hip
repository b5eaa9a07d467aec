// wave_tracer_amd — the wave-per-walk parts of a Fraunhofer interaction: region power sums (k_flux_*), rejection sampling (k_interact_c*) (see wtgpu_kernels.h for the list of kernel translation units).
#include "wtgpu_kernels.h"

namespace wtk {

// Intercepted power of interaction regions that overflowed the bounded list (find_closest_triangle's sum over ALL region triangles,
// plt_bdpt_detail.hpp:391-416) for the pass-C walks.  Such regions hold 10^3..10^5 triangles (a wide emitter beam over a finely
// tessellated mesh), 5000 on average in the headline workload: one wavefront per region would leave the round waiting for the
// largest one (measured: 27 ms for a 130,000-triangle region).  k_flux_split cuts the part of the tree that overlaps the region
// into subtrees of <= kFluxTaskTris (2048; swept 128 / 512 / 2048: 247 / 216 / 208 ms per pass) triangles, k_flux_tasks sums every subtree on whichever wavefront is free (f64 atomics).
__global__ void __launch_bounds__(64, 3) k_flux_split(launch_args_t a) {
    __shared__ coop_gather_shared_t sh;
    coop_set_dropped_counter(sh, a.st.counters + kDroppedSlot);
    uint32_t* ctl = a.st.ctl;
    const uint32_t n = ctl[CTL_INTC_COUNT];
    const int lane = threadIdx.x & 63;
    // 64 queue items per grab: every lane looks at one walk's marker (most pass-C walks have a region that fitted its list and need no
    // split — bidir_room: 400,000 items a round, a few thousand to split; one item per grab was 11.5 ms of a 125-ms batch there), the
    // wavefront then cuts the regions of the flagged ones, one after the other
    for (;;) {
        const uint32_t base = wave_grab(ctl + CTL_FSPLIT_HEAD);
        if (base >= n) break;
        uint32_t w_mine = 0;
        bool need = false;
        if (base + (uint32_t)lane < n) {
            w_mine = a.st.intc_queue[base + lane];
            need = is_region_marker(WT_TRAV_U(a, w_mine, tuid));
        }
        unsigned long long m = __ballot(need);
        while (m) {
            const int src = __ffsll((long long)m) - 1;
            m &= m - 1;
            const uint32_t w = (uint32_t)__shfl((int)w_mine, src, 64);   // block-uniform
            const walk_trace_in_t wk = walk_load_trace_in(a.st.walks, a.st.walk_words, w);
            const cone_t tcone = walk_trace_envelope(a.sc, wk);
            const float beam_dist = WT_TRAV_F(a, w, dist), region_depth = WT_TRAV_F(a, w, region_depth);
            if (threadIdx.x == 0) a.st.facc[w] = 0.0;
            coop_split(a.sc, tcone, range_t{beam_dist, beam_dist + region_depth}, sh, a.flux_task_tris, [&](int32_t ptr) {
                const uint32_t idx = atomicAdd(ctl + CTL_FTASK_COUNT, 1u);
                if (idx < a.st.ftask_cap)
                    a.st.ftasks[idx] = make_uint2(w, (uint32_t)ptr);
                else
                    atomicAdd(a.st.counters + WT_COUNTER_SLOT(fsd_pool_overflow), 1ull);   // reported; cannot happen below 4M tasks per batch
            });
            __syncthreads();
        }
    }
}
__global__ void __launch_bounds__(64, WTGPU_LB_FLUX) k_flux_tasks(launch_args_t a) {
    __shared__ coop_gather_shared_t sh;
    coop_set_dropped_counter(sh, a.st.counters + kDroppedSlot);
    uint32_t* ctl = a.st.ctl;
    const uint32_t n = min(ctl[CTL_FTASK_COUNT], a.st.ftask_cap);
    for (;;) {
        const uint32_t item = wave_grab_item(ctl + CTL_FTASK_HEAD);
        if (item >= n) break;
        const uint2 task = a.st.ftasks[item];
        const uint32_t w = task.x;
        walk_t wk;
        soa_load(a.st.walks, a.st.walk_words, w, wk);   // uniform address: broadcast
        const float beam_dist = WT_TRAV_F(a, w, dist), region_depth = WT_TRAV_F(a, w, region_depth);
        const bool want_front = WT_TRAV_U(a, w, front_face) != 0;
        const range_t izr{beam_dist, beam_dist + region_depth};
        const vec3 sd3 = beam_footprint(wk.beam, beam_dist) / kBeamEnvelope;
        const cone_t tcone = walk_trace_envelope(a.sc, wk);
        unsigned long long gst[2] = {0, 0};
        const double flux = coop_gather(a.sc, tcone, izr, wk.beam.env, cone_frame(wk.beam.env), izr, vec2{sd3.x, sd3.y}, want_front, sh, true, false,
                                        a.profile ? gst : nullptr, (int32_t)task.y).flux;
        if (threadIdx.x == 0) {
            if (flux != 0.0) unsafeAtomicAdd(&a.st.facc[w], flux);
            if (a.profile) {   // WTGPU_PROFILE=1: sizes of the gathered regions
                atomicAdd(a.st.counters + kNumCounters + 0, 1ull);
                atomicAdd(a.st.counters + kNumCounters + 1, gst[0]);
                atomicAdd(a.st.counters + kNumCounters + 2, gst[1]);
                atomicMax(a.st.counters + kNumCounters + 4, gst[0]);
            }
        }
        __syncthreads();
    }
}

// Pass C: the walks of pass B whose Fraunhofer aperture has edges, ONE WAVEFRONT PER WALK.  What a single lane would do serially
// is spread over the 64 lanes: the intercepted-power integral over every triangle of the interaction region (find_closest_triangle,
// plt_bdpt_detail.hpp:391-416 — coop_gather walks the WHOLE region, however many triangles it holds: the reference's unbounded list)
// and the rejection sampling (64 tries per step; tries own their random draws, the lowest accepted try wins like in the sequential
// loop); lane 0 then re-enters bdpt_walk_step with the outcome (vertex append, beam transform, Russian roulette).
//
// The number of tries is wildly non-uniform: most apertures accept within the first 64, but the acceptance probability is
// |sum of amplitudes|^2 / (n x sum of |amplitudes|^2) and the loop runs up to n x 1024 tries (fsd.h: fsd_max_tries, the reference's
// cap) — in the headline workload apertures of 8..15 segments average 1,650 tries and account for 2/3 of this pass's arithmetic
// (WTGPU_PROFILE=3), with single walks keeping one wavefront busy for a millisecond while the round waits.  BLOCK = 64 (k_interact_c)
// therefore gives up after kEasyTries tries and queues the walk for BLOCK = 256 (k_interact_c_hard): four wavefronts per walk, 256
// tries per step, continuing at try kEasyTries.
constexpr uint32_t kEasyTries = 512;
constexpr uint32_t kStageSegs = 256;

// ---- The pieces every form of pass C is put together from, each written once: straight-line code, called from INSIDE the persistent loops --------
// A walk of the pass-C queue as pass B left it.  fsd_max_tries(ap) holds once ap.recp_I does (pass_c_set_recp_I, in this kernel or an earlier one).
struct pass_c_walk_t {
    uint32_t w, slot, base;   // the walk, the pool slot of its aperture, the first draw of try 0 (try t owns the kFsdDrawsPerTry draws from base + t x that)
    fsd_aperture_t ap;
    fsd_edges_ref_t ed;
    sampler_t ss;             // the walk's stream at draw 0
};
WT_D pass_c_walk_t pass_c_load_walk(const launch_args_t& a, const fsd_pool_t& pool, uint32_t w) {
    uint32_t i, stream;
    walk_ident(a, w, i, stream);
    const uint64_t sample_id = sample_id_of(a, i);
    const uint32_t rng_draws = a.st.walks[(size_t)w * a.st.walk_words + WT_WALK_WORD(rng_draws)];
    pass_c_walk_t c;
    c.w = w;
    c.slot = WT_TRAV_U(a, w, by);   // left by pass B
    c.ap = pool.hdr[c.slot];
    c.ed = fsd_pool_edges(pool, c.slot);
    c.ss = make_sampler(a.seed, sample_id, stream, 0);
    c.base = fsd_tries_base(make_sampler(a.seed, sample_id, stream, rng_draws));
    return c;
}
// The intercepted power of a LISTED interaction region (same z-slab, cone and facing as the reference's list-based sum; bdpt_walk_step computes the
// same sum triangle by triangle): its inputs, one triangle's share, and the sum with a lane per triangle — xor butterfly 32 .. 1, the tree that
// k_interact_c_prep's groups of eight reproduce in their own evaluation order.  A region that overflowed the bounded list carries a marker: it was
// summed over all of its triangles by k_flux_split / k_flux_tasks.
struct pass_c_region_t {
    cone_t benv;   // the beam's own envelope (not offset for tracing)
    frame_t bframe;
    range_t izr;
    vec2 sigma;
    bool front;
    uint32_t ntris;
    const uint32_t* tl;
};
WT_D pass_c_region_t pass_c_load_region(const launch_args_t& a, uint32_t w) {
    const walk_trace_in_t wk = walk_load_trace_in(a.st.walks, a.st.walk_words, w);   // (uniform address, or the lanes of a group read the same words)
    const float tr_dist = WT_TRAV_F(a, w, dist), tr_depth = WT_TRAV_F(a, w, region_depth);
    const vec2 axes = cone_axes(wk.env, tr_dist);
    return pass_c_region_t{wk.env, cone_frame(wk.env), range_t{tr_dist, tr_dist + tr_depth}, vec2{axes.x / kBeamEnvelope, axes.y / kBeamEnvelope},
                           WT_TRAV_U(a, w, front_face) != 0, WT_TRAV_U(a, w, ntris), a.st.tris + (size_t)w * kTriListWords};
}
WT_D double pass_c_region_triangle(const launch_args_t& a, const pass_c_region_t& g, uint32_t j) {
    return (double)region_triangle_flux(a.sc, g.bframe, g.benv, g.izr, g.sigma, g.tl[j], g.front);
}
WT_D double pass_c_region_power_wave(const launch_args_t& a, uint32_t w, int lane) {   // (w: uniform over the wavefront)
    if (is_region_marker(WT_TRAV_U(a, w, tuid))) return a.st.facc[w];
    const pass_c_region_t g = pass_c_load_region(a, w);
    double flux = (uint32_t)lane < g.ntris ? pass_c_region_triangle(a, g, (uint32_t)lane) : 0.0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) flux += __shfl_xor(flux, off, 64);
    return flux;
}
WT_D void pass_c_set_recp_I(const fsd_pool_t& pool, uint32_t slot, fsd_aperture_t& ap, double flux, bool lead) {
    const float I = (float)(1.0 - flux);
    ap.recp_I = I > 0.f ? 1.f / I : 0.f;
    if (lead) pool.hdr[slot] = ap;
}
// Rejection sampling, tries t_begin .. t_end - 1 of walk `c`, BLOCK tries per step, one per thread: the lowest accepted try of a step ends the loop —
// one wavefront finds it by ballot, four through s_tmin / s_res between real barriers (every thread of the block makes the same calls).
template <int BLOCK>
WT_D fsd_outcome_t pass_c_try_loop(const launch_args_t& a, const pass_c_walk_t& c, const fsd_edges_ref_t& edr, uint32_t t_begin, uint32_t t_end, uint32_t* s_tmin, float* s_res) {
    const uint32_t tid = threadIdx.x;
    fsd_outcome_t o{0u, 0u, vec2{0.f, 0.f}, 0.f};
    for (uint32_t t0 = t_begin; t0 < t_end && !o.acc; t0 += BLOCK) {
        const uint32_t t = t0 + tid;
        fsd_try_t r{{0.f, 0.f}, 0.f, 0u};
        if (t < t_end) r = fsd_try(a.sc, c.ap, edr, sampler_at(c.ss, c.base + t * kFsdDrawsPerTry));
        if (BLOCK == 64) {
            const unsigned long long am = __ballot(r.accept != 0);
            if (am) {
                const int wl = __ffsll((long long)am) - 1;
                o = fsd_outcome_t{1u, t0 + (uint32_t)wl, vec2{__shfl(r.x.x, wl, 64), __shfl(r.x.y, wl, 64)}, __shfl(r.f, wl, 64)};
            }
        } else {   // the lowest accepted try of the block
            if (tid == 0) *s_tmin = 0xFFFFFFFFu;
            __syncthreads();
            if (r.accept) atomicMin(s_tmin, t);
            __syncthreads();
            const uint32_t tm = *s_tmin;
            if (tm != 0xFFFFFFFFu) {
                if (t == tm) {
                    s_res[0] = r.x.x;
                    s_res[1] = r.x.y;
                    s_res[2] = r.f;
                }
                __syncthreads();
                o = fsd_outcome_t{1u, tm, vec2{s_res[0], s_res[1]}, s_res[2]};
            }
            __syncthreads();
        }
    }
    return o;
}
// A try reads every segment of the aperture twice (segment selection by a linear scan of the pdfs, then the density / scattering-function sums):
// the segments are staged in the block's s_seg once per walk (larger apertures are read from the pool).
template <int BLOCK>
WT_D fsd_outcome_t pass_c_tries(const launch_args_t& a, const pass_c_walk_t& c, uint32_t t_begin, uint32_t t_end, fsd_edge_t* s_seg, uint32_t* s_tmin, float* s_res) {
    // (the three cases in this order, not as early returns: those gave the tries-only kernels another register allocation, 69 VGPRs for 73;
    // profiles/pass_c_shared_kernel_resources.txt)
    fsd_outcome_t o{0u, 0u, vec2{0.f, 0.f}, 0.f};
    if (t_begin >= t_end) {   // (nothing to try here: a dead aperture, a boundary at kPrepTries)
    } else if (c.ap.n_edges <= kStageSegs) {
        __syncthreads();   // (the previous walk's tries are done with the buffer)
        for (uint32_t k = threadIdx.x; k < c.ap.n_edges; k += BLOCK) s_seg[k] = c.ed.p[k];
        __syncthreads();
        o = pass_c_try_loop<BLOCK>(a, c, fsd_edges_ref_t{s_seg, 1}, t_begin, t_end, s_tmin, s_res);
    } else
        o = pass_c_try_loop<BLOCK>(a, c, c.ed, t_begin, t_end, s_tmin, s_res);
    return o;
}
// The commit of ONE walk by the calling lane: bdpt_walk_step re-entered with the outcome of the tries (fsd_defer_resolved: the aperture's header holds
// recp_I by now) — vertex append, beam transform, Russian roulette.  TRUE: the walk goes on.  (With known_no_primary set the step makes no BVH query.)
WT_D bool pass_c_commit_walk(const launch_args_t& a, const fsd_pool_t& pool, uint32_t w, const fsd_outcome_t& o, bdpt_counters_t* ctr, const stack_ref_t* stack) {
    uint32_t i, stream;
    walk_ident(a, w, i, stream);
    const uint64_t sample_id = sample_id_of(a, i);
    walk_t wk;
    soa_load(a.st.walks, a.st.walk_words, w, wk);
    trav_result_t tr;
    soa_load(a.st.trav, kTravWords, w, tr);
    const uint32_t slot = __float_as_uint(tr.by);   // left by pass B
    const fsd_aperture_t ap = pool.hdr[slot];
    const uint32_t base = fsd_tries_base(make_sampler(a.seed, sample_id, stream, wk.rng_draws));
    fsd_defer_t defer = fsd_defer_resolved(ap, slot, base, fsd_max_tries(ap), o);
    const uint_list_t tris{a.st.tris + (size_t)w * kTriListWords, 1u, kMaxConeTris};
    const vertex_store_t vs = walk_vertices(a, w);
    const bool cont = bdpt_walk_step<2>(a.sc, wk, tr, tris, vs, pool, a.seed, sample_id, stream, ctr, stack, &defer);
    wk.active = cont ? 1u : 0u;
    soa_store(a.st.walks, a.st.walk_words, w, wk);
    return cont;
}

// ---- One wavefront (BLOCK = 64) or four (BLOCK = 256) per walk: the body of five kernels ----------------------------------------------------------
//   START  kStartPower: the walks of pass C's own queue — the power sum with a lane per triangle, then the tries from 0 (BLOCK = 64)
//          kStartPrep:  the wide queue — k_interact_c_prep's groups summed the power and rejected tries 0 .. kPrepTries - 1 (BLOCK = 64)
//          kStartEasy:  the hard queue — a one-wavefront form rejected every try below easy_tries (BLOCK = 256)
//   COMMIT true:  the A/B reference (k_interact_c, k_interact_c_hard; easy_tries = kEasyTries): thread 0 resumes the step right here
//          false: the tiers: the outcome goes to the commit queue.  easy_tries (>= kPrepTries): kEasyTries, or what the tests set to drive walks
//                 into every tier (WTGPU_PASS_C_EASY_TRIES) — results do not depend on it.
enum pass_c_start_t { kStartPower, kStartPrep, kStartEasy };
template <int BLOCK, pass_c_start_t START, bool COMMIT>
WT_D void interact_c_wave_body(const launch_args_t& a, int in, uint32_t easy_tries) {
    constexpr bool HARD = BLOCK > 64, POWER = START == kStartPower;
    static_assert(HARD == (START == kStartEasy), "four wavefronts per walk from easy_tries on, one below");
    __shared__ uint32_t s_item;
    __shared__ uint32_t s_tmin;
    __shared__ float s_res[3];
    __shared__ stack_entry_t lds[8];   // COMMIT: the resumed step does no BVH queries; lane 0's stack is a formality
    __shared__ fsd_edge_t s_seg[kStageSegs];   // the walk's aperture segments (7 KB; larger apertures are read from the pool)
    uint32_t* ctl = a.st.ctl;
    const uint32_t n = ctl[HARD ? CTL_INTD_COUNT : (POWER ? CTL_INTC_COUNT : CTL_PCW_COUNT)];
    const uint32_t* queue_in = HARD ? a.st.intd_queue : (POWER ? a.st.intc_queue : pass_c_wide_queue(a));
    uint32_t* commit_queue = pass_c_commit_queue(a);
    unsigned long long* prof = a.st.counters + kNumCounters;
    const int tid = threadIdx.x, lane = threadIdx.x & 63;
    bdpt_counters_t ctr;
    memset(&ctr, 0, sizeof(ctr));
    const fsd_pool_t pool = fsd_pool_of(a);
    unsigned long long settled = 0, settled_early = 0;
    for (;;) {
        const long long pl0 = COMMIT && a.profile == 3 ? clock64() : 0;
        uint32_t item = 0;
        if (HARD) {   // four wavefronts: through the shared word, between real barriers — the first one BEFORE the branch on the thread index
            __syncthreads();   // (wtgpu_kernels.h: wave_grab0 says why; it also keeps the last iteration's readers ahead of the write)
            if (tid == 0) s_item = atomicAdd(ctl + CTL_INTD_HEAD, 1u);
            __syncthreads();
            item = s_item;
        } else
            item = wave_grab_item(ctl + (POWER ? CTL_INTC_HEAD : CTL_PCW_HEAD));
        if (item >= n) break;
        pass_c_walk_t c = pass_c_load_walk(a, pool, queue_in[item]);
        const long long pc0 = a.profile == 3 ? clock64() : 0;
        if (POWER) pass_c_set_recp_I(pool, c.slot, c.ap, pass_c_region_power_wave(a, c.w, lane), lane == 0);
        const uint32_t max_tries = fsd_max_tries(c.ap);
        const uint32_t t_begin = HARD ? easy_tries : (POWER ? 0u : kPrepTries), t_end = HARD ? max_tries : (max_tries < easy_tries ? max_tries : easy_tries);
        const fsd_outcome_t o = pass_c_tries<BLOCK>(a, c, t_begin, t_end, s_seg, &s_tmin, s_res);
        const int bin = pass_c_prof_bin(c.ap.n_edges);
        if (a.profile == 3 && tid == 0) {   // WTGPU_PROFILE=3: cost by aperture size; the wide and hard tries of the tiers apart from prep's (and the thin rounds')
            atomicAdd(prof + (COMMIT || POWER ? kPassCProfWalks : kPassCProfWideWalks) + bin, 1ull);
            atomicAdd(prof + kPassCProfTries + bin, (unsigned long long)(o.acc ? o.t_acc + 1u - t_begin : t_end - t_begin));
            atomicAdd(prof + (COMMIT || POWER ? kPassCProfTicks : kPassCProfWideTicks) + bin, (unsigned long long)(clock64() - pc0));
            if (COMMIT) atomicAdd(prof + kPassCProfLoadTicks + bin, (unsigned long long)(pc0 - pl0));
        }
        const bool hand_over = !HARD && !o.acc && t_end < max_tries;   // none of the first easy_tries tries accepted: four wavefronts take over
        if constexpr (COMMIT) {
            const long long pm0 = a.profile == 3 ? clock64() : 0;
            if (hand_over) {
                if (lane == 0) a.st.intd_queue[atomicAdd(ctl + CTL_INTD_COUNT, 1u)] = c.w;
                continue;
            }
            bool cont = false;
            if (tid == 0) {
                const stack_ref_t stack = make_stack_ref(lds, 1, 8, 8, nullptr);
                cont = pass_c_commit_walk(a, pool, c.w, o, &ctr, &stack);
                if (a.profile == 3) atomicAdd(prof + kPassCProfCommitTicks + bin, (unsigned long long)(clock64() - pm0));
            }
            if (tid < 64) queue_append(a, ctl, 1 - in, cont, c.w);
        } else if (tid == 0) {
            if (hand_over) {
                a.st.intd_queue[atomicAdd(ctl + CTL_INTD_COUNT, 1u)] = c.w;
            } else {
                pass_c_store_outcome(a, c.w, o);
                commit_queue[atomicAdd(ctl + CTL_PCC_COUNT, 1u)] = c.w;
                if (POWER && (o.acc ? o.t_acc < kPrepTries : max_tries <= kPrepTries))   // (what the groups of eight would have settled: counted as theirs)
                    ++settled_early;
                else
                    ++settled;
            }
        }
    }
    if constexpr (COMMIT) {
        if (a.count_stats && tid < 64) flush_counters(a.st.counters, ctr);
    } else {
        if (a.count_stats && tid == 0 && settled) atomicAdd(prof + kPassCTierSlot + (HARD ? 2 : 1), settled);
        if (POWER && a.count_stats && tid == 0 && settled_early) atomicAdd(prof + kPassCTierSlot, settled_early);
    }
}
__global__ void __launch_bounds__(64, WTGPU_LB_INTERACT_C) k_interact_c(launch_args_t a, int in) { interact_c_wave_body<64, kStartPower, true>(a, in, kEasyTries); }
__global__ void __launch_bounds__(WTGPU_HARD_BLOCK) k_interact_c_hard(launch_args_t a, int in) { interact_c_wave_body<WTGPU_HARD_BLOCK, kStartEasy, true>(a, in, kEasyTries); }

// ---- Pass C in TIERS (WTGPU_PASS_C_TIERS=1, the default; the two kernels above are the A/B reference) -------------------------------------------
// The one-wavefront form runs three parts of very different width on one wavefront per walk: the power sum (lane = triangle of the list: 10-20 lanes),
// the tries (64 lanes, of which every try behind the first accepted one is wasted — most apertures accept within a handful) and the commit
// (ONE lane: 57 + 86 record words, beam transform, roulette) — 13 of 64 lanes per vector instruction on the headline workload.  Here each part
// has the lane shape that fits it:
//   k_interact_c_prep        8 lanes per walk, 8 walks per wavefront (the shape of k_path_fsd): power sum, recp_I, tries 0 .. 7
//   k_interact_c_wide        one wavefront per walk that prep did not settle: tries 8 .. easy_tries, 64 per step
//   k_interact_c_hard_tries  four wavefronts per walk that outlasts easy_tries
//   k_interact_c_commit      lane = walk (the shape of pass B): bdpt_walk_step with the outcome
// A try's draws depend on its index only and the lowest accepted try wins in every tier, so the accepted try is the one k_interact_c finds (the
// wide and hard tiers run its very loop, pass_c_tries); recp_I is the same sum in the same tree (below); the commit is the same pass_c_commit_walk.
// Per walk nothing differs, only the order of the next round's queue and of the film's atomic adds.
//
// The power sum, bit for bit: pass_c_region_power_wave holds triangle j in lane j (0 beyond the list) and reduces by xor 32, 16, 8, 4, 2, 1.  f64 addition
// is commutative, so after the first three steps lane s < 8 holds ((v[s] + v[s+32]) + (v[s+16] + v[s+48])) + ((v[s+8] + v[s+40]) + (v[s+24] + v[s+56])).
// Group lane s evaluates exactly those eight triangles, t_k = v[s + 8k], adds them in that order, and the group finishes with xor 4, 2, 1.
//
// THIN ROUNDS.  Groups pay where walks outnumber the wavefronts: a group's lane sums ceil(ntris / 8) triangles one after the other, and the tiers
// run one after the other.  From the fourth round or so a batch's pass-C queue holds fewer walks than the grid has wavefronts x 8, the pass is
// bound by the LATENCY of its longest walk, and one wavefront per walk is the shorter way (measured, one stream, us per round of prep + wide
// against k_interact_c: 1365 / 3103 in round 0, 567 / 469 in round 3, 240 / 100 in rounds 9-14).  A round whose queue holds at most `thin_below`
// walks (the host: WTGPU_PASS_C_THIN, 8, x the grid's wavefronts) therefore runs interact_c_wave_body<64, kStartPower, false> right here: power sum with
// a lane per triangle, tries from 0 with 64 lanes, outcome to the commit queue — k_interact_c without its commit; the wide queue stays empty.
__global__ void __launch_bounds__(64, WTGPU_LB_INTERACT_C) k_interact_c_prep(launch_args_t a, uint32_t thin_below, uint32_t easy_tries) {
    uint32_t* ctl = a.st.ctl;
    const uint32_t n = ctl[CTL_INTC_COUNT];
    const int lane = threadIdx.x & 63;
    const uint32_t s = (uint32_t)lane & (kPrepTries - 1u), group = (uint32_t)lane / kPrepTries;
    const fsd_pool_t pool = fsd_pool_of(a);
    uint32_t* wide_queue = pass_c_wide_queue(a);
    uint32_t* commit_queue = pass_c_commit_queue(a);
    unsigned long long* prof = a.st.counters + kNumCounters;
    unsigned long long settled = 0;
    if (a.count_stats && blockIdx.x == 0 && threadIdx.x == 0 && n > 0) {   // the round's pass-C queue, for the tests of the tiers
        atomicAdd(prof + kPassCWalksSlot, (unsigned long long)n);
        const unsigned long long r = atomicAdd(prof + kPassCRoundsSlot, 1ull);
        if (n % kPrepTries) atomicAdd(prof + kPassCRoundsSlot + 1, 1ull);
        if (n < kPrepTries) atomicAdd(prof + kPassCRoundsSlot + 2, 1ull);
        if (r < kPassCQueueSlots) prof[kPassCQueueSlot + r] = n;
    }
    if (n <= thin_below) {   // (uniform over the grid)
        interact_c_wave_body<64, kStartPower, false>(a, 0, easy_tries);
        return;
    }
    for (;;) {
        const long long pl0 = a.profile == 3 ? clock64() : 0;
        const uint32_t base0 = wave_grab0(ctl + CTL_INTC_HEAD, 64u / kPrepTries);   // eight walks per wavefront, eight lanes each
        if (base0 >= n) break;
        const uint32_t item = base0 + group;
        const bool have = item < n;
        pass_c_walk_t c;   // (a group without a walk: zeros, which nobody reads)
        memset(&c, 0, sizeof(c));
        uint32_t max_tries = 0;
        bool marker = false;
        double flux = 0.0;
        if (have) {
            c = pass_c_load_walk(a, pool, a.st.intc_queue[item]);
            marker = is_region_marker(WT_TRAV_U(a, c.w, tuid));
            if (marker) {   // the region overflowed the bounded list: summed over all of it by k_flux_split / k_flux_tasks
                flux = a.st.facc[c.w];
            } else {
                const pass_c_region_t g = pass_c_load_region(a, c.w);
                double t0 = 0.0, t1 = 0.0, t2 = 0.0, t3 = 0.0, t4 = 0.0, t5 = 0.0, t6 = 0.0, t7 = 0.0;   // t_k: triangle s + 8 k of the list
#pragma unroll 1
                for (uint32_t k = 0; s + kPrepTries * k < g.ntris && k < 8u; ++k) {
                    const double f = pass_c_region_triangle(a, g, s + kPrepTries * k);
                    t0 = k == 0u ? f : t0;
                    t1 = k == 1u ? f : t1;
                    t2 = k == 2u ? f : t2;
                    t3 = k == 3u ? f : t3;
                    t4 = k == 4u ? f : t4;
                    t5 = k == 5u ? f : t5;
                    t6 = k == 6u ? f : t6;
                    t7 = k == 7u ? f : t7;
                }
                flux = ((t0 + t4) + (t2 + t6)) + ((t1 + t5) + (t3 + t7));
            }
        }
        // (every lane of the wavefront: the groups that hold a region marker, or no walk, add their own value to itself — and drop the result)
        double fsum = flux;
#pragma unroll
        for (int off = (int)kPrepTries / 2; off > 0; off >>= 1) fsum += __shfl_xor(fsum, off, 64);
        if (!marker) flux = fsum;
        if (have) {
            pass_c_set_recp_I(pool, c.slot, c.ap, flux, s == 0u);
            max_tries = fsd_max_tries(c.ap);
        }
        const long long pc0 = a.profile == 3 ? clock64() : 0;
        // ---- tries 0 .. 7, one per lane of the group; the segments come from the pool (the L1 serves the group's repeats)
        fsd_try_t r{{0.f, 0.f}, 0.f, 0u};
        if (have && s < max_tries) r = fsd_try(a.sc, c.ap, c.ed, sampler_at(c.ss, c.base + s * kFsdDrawsPerTry));
        const uint32_t am = (uint32_t)(__ballot(r.accept != 0) >> (group * kPrepTries)) & ((1u << kPrepTries) - 1u);   // the group's accepted tries
        const uint32_t t_acc = am ? (uint32_t)__ffs((int)am) - 1u : 0u;
        const int wl = (int)(group * kPrepTries + t_acc);   // (within the group; without an accepted try: its first lane, whose zeros nobody reads)
        const fsd_outcome_t o{am ? 1u : 0u, t_acc, vec2{__shfl(r.x.x, wl, 64), __shfl(r.x.y, wl, 64)}, __shfl(r.f, wl, 64)};
        // ---- accepted, or no try left (a dead aperture, max_tries = 0): the outcome for the commit; else the wide kernel goes on at try 8
        const bool lead = have && s == 0u;
        const bool settle = lead && (o.acc || max_tries <= kPrepTries);
        if (settle) {
            pass_c_store_outcome(a, c.w, o);
            ++settled;
        }
        wave_append(commit_queue, ctl + CTL_PCC_COUNT, settle, c.w);
        wave_append(wide_queue, ctl + CTL_PCW_COUNT, lead && !settle, c.w);
        if (a.profile == 3) {   // WTGPU_PROFILE=3: pass-C cost by aperture size (bin = floor(log2(segments))); a wavefront's clocks, shared out among its walks
            const long long pt = clock64();
            const long long ng = (long long)__popcll(__ballot(lead));
            if (lead) {
                const int bin = pass_c_prof_bin(c.ap.n_edges);
                atomicAdd(prof + kPassCProfWalks + bin, 1ull);
                atomicAdd(prof + kPassCProfTries + bin, (unsigned long long)(o.acc ? o.t_acc + 1u : min(max_tries, kPrepTries)));
                atomicAdd(prof + kPassCProfLoadTicks + bin, (unsigned long long)((pc0 - pl0) / ng));
                atomicAdd(prof + kPassCProfTicks + bin, (unsigned long long)((pt - pc0) / ng));
            }
        }
    }
    if (a.count_stats) flush_counter(a, kNumCounters + kPassCTierSlot, settled);
}

// Tries only (pass_c_tries, the segments staged in LDS), for the walks whose first kPrepTries tries were rejected: BLOCK = 64 from try kPrepTries to
// easy_tries, BLOCK = 256 from there to the end.  The aperture's header holds recp_I since k_interact_c_prep.
__global__ void __launch_bounds__(64, WTGPU_LB_INTERACT_C) k_interact_c_wide(launch_args_t a, uint32_t easy_tries) { interact_c_wave_body<64, kStartPrep, false>(a, 0, easy_tries); }
__global__ void __launch_bounds__(WTGPU_HARD_BLOCK) k_interact_c_hard_tries(launch_args_t a, uint32_t easy_tries) { interact_c_wave_body<WTGPU_HARD_BLOCK, kStartEasy, false>(a, 0, easy_tries); }

// The commit, lane = walk of the commit queue (the shape of pass B, interact_body<1>): pass_c_commit_walk, which k_interact_c's lane 0 runs alone,
// with the outcome record — and the walk goes to the next round's queue.  (No traversal stack: the step makes no BVH query, as in pass B.)
__global__ void __launch_bounds__(kBlock, WTGPU_LB_INTERACT_B) k_interact_c_commit(launch_args_t a, int in) {
    uint32_t* ctl = a.st.ctl;
    const uint32_t n = ctl[CTL_PCC_COUNT];
    const uint32_t* commit_queue = pass_c_commit_queue(a);
    bdpt_counters_t ctr;
    memset(&ctr, 0, sizeof(ctr));
    const fsd_pool_t pool = fsd_pool_of(a);
    for (;;) {
        const uint32_t base0 = wave_grab(ctl + CTL_PCC_HEAD);
        if (base0 >= n) break;
        const uint32_t qi = base0 + (threadIdx.x & 63);
        const bool valid = qi < n;
        bool cont = false;
        uint32_t w = 0;
        const long long pm0 = a.profile == 3 ? clock64() : 0;
        if (valid) {
            w = commit_queue[qi];
            cont = pass_c_commit_walk(a, pool, w, pass_c_load_outcome(a, w), &ctr, nullptr);
        }
        if (a.profile == 3) {   // (a wavefront's clocks, shared out among its walks)
            const long long dt = clock64() - pm0, nv = (long long)__popcll(__ballot(valid));
            if (valid) atomicAdd(a.st.counters + kNumCounters + kPassCProfCommitTicks + pass_c_prof_bin(pool.hdr[WT_TRAV_U(a, w, by)].n_edges), (unsigned long long)(dt / nv));
        }
        queue_append(a, ctl, 1 - in, cont, w);
    }
    if (a.count_stats) flush_counters(a.st.counters, ctr);
}

}   // namespace wtk
