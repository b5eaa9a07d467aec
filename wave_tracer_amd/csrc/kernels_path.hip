// wave_tracer_amd — plt_path (see wtgpu_kernels.h for the list of kernel translation units).
#include "wtgpu_kernels.h"

namespace wtk {

// ---- plt_path: one walk per sample; k_trace / k_trace_heavy are shared with plt_bdpt (they only read the walk_t
// prefix of the walk record), the interaction step is path_walk_step (wt/path.h): UTD evaluation of the previous aperture (shadow
// rays through the LDS stack), primary triangle, edge query, aperture construction, NEE / sensing splats (f64 atomics), sampling.
__global__ void __launch_bounds__(kBlock) k_path_generate(launch_args_t a) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i == 0) {
        ctl_reset_batch(a.st.ctl);
        a.st.ctl[CTL_COUNT0] = a.nb;
    }
    if (i >= a.nb) return;
    uint32_t pix;
    const uint64_t sample_id = sample_id_of(a, i, pix);
    path_walk_t pw;
    path_generate(a.sc, a.seed, sample_id, pix % a.sc.sensor.width, pix / a.sc.sensor.width, pw);
    soa_store(a.st.walks, a.st.walk_words, i, pw);
}

#ifdef WTGPU_FSD_WATCH
extern "C" int wtgpu_debug_set_watch(unsigned int* host_mapped) {
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_watch), &host_mapped, sizeof(host_mapped));
}
#endif
// coop_do_fsd (wt/coop_utd.h): G lanes per aperture.  The apertures of the city-block workload hold 11 wedges on average: one aperture per wavefront leaves 5 of 6 lanes without a wedge.
#ifndef WTGPU_FSD_GROUP
#define WTGPU_FSD_GROUP 8   // (etoile 720 x 540: 64 / 32 / 16 / 8 lanes per aperture -> 61.8 / 73.3 / 80.6 / 84.6 Msamples/s, profiles/r06_ab_experiments.log)
#endif

// plt_path, before the interaction step: the coherent UTD sum of the aperture the walk built in the previous round towards this round's
// interaction point (plt_path_detail.hpp:616-636) — one wavefront per walk, queue filled by the previous round's k_path_interact.
__global__ void __launch_bounds__(64, 3) k_path_fsd(launch_args_t a, const path_state_t* __restrict__ ps, uint32_t round) {
    const path_state_t& P = *ps;
    __shared__ stack_entry_t lds[kLdsStack * 64];
    uint32_t* ctl = a.st.ctl;
    const uint32_t qin = round & 1u;
    const uint32_t n = ctl[CTL_FSDQ_COUNT0 + qin];
    stack_entry_t spill[kSpillStack];
    stack_ref_t stack;
    lds_stack(lds, spill, stack, 64u);
    bdpt_counters_t ctr;
    memset(&ctr, 0, sizeof(ctr));
    const utd_edge_rec_t* prev_pool = P.utd[(round + 1u) & 1u];
    constexpr int G = WTGPU_FSD_GROUP, NG = 64 / G;
    const uint32_t group = (threadIdx.x & 63u) / (uint32_t)G;
    for (;;) {
        const uint32_t base = wave_grab0(ctl + CTL_FSDQ_HEAD, (uint32_t)NG);   // NG walks per wavefront, G lanes each
        if (base >= n) break;
        const uint32_t item = base + group;
        uint32_t w = 0;
        bool have = item < n;
        if (have) {
            w = P.fsdq[qin][item];
            have = WT_TRAV_U(a, w, empty) == 0;   // (an empty record: the step ends before do_fsd, plt_path_detail.hpp:577-581)
        }
        // (the lanes of a group read the same words: one record per group; fields the sum does not use are never loaded)
        path_walk_t pw;
        memset(&pw, 0, sizeof(pw));
        vec3 interaction_wp{0.f, 0.f, 0.f};
        if (have) {
            soa_load(a.st.walks, a.st.walk_words, w, pw);
            interaction_wp = trav_origin(a, w) + WT_TRAV_F(a, w, dist) * pw.w.beam.env.d;
        }
        const float f = coop_do_fsd<G>(a.sc, pw.prev_beam.env, path_geo_prev(pw.w), interaction_wp, pw.ap, prev_pool + pw.ap.edge_offset, pw.w.beam.k, stack, &ctr, have);
        if (have && (threadIdx.x & (uint32_t)(G - 1)) == 0) P.fsd_f[w] = f;
    }
    if (a.count_stats) flush_counters(a.st.counters, ctr);
}

// plt_path, the classified-edge set of regions the per-lane means cannot hold (path_defer_t::need_gather): one wavefront per walk.  Non-ballistic
// hit: the triangles of the interaction region [dist, dist + depth] of the traced cone.  Ballistic hit: the reference's cone query around the hit
// (plt_path_detail.hpp:645-650: closest cone hit inside dist -+ z / 2, then every triangle inside the final slab) — closest hit by the
// wave-cooperative query, then a walk of that slab.  Edge ids through the LDS bitmap: any number, sorted, into the round's edge pool.
__global__ void __launch_bounds__(64, 2) k_path_edges(launch_args_t a, const path_state_t* __restrict__ ps) {
    const path_state_t& P = *ps;
    __shared__ coop_shared_t csh;
    __shared__ coop_gather_shared_t sh;
    __shared__ coop_edges_t eg;
    coop_set_dropped_counter(csh, a.st.counters + kDroppedSlot);
    coop_set_dropped_counter(sh, a.st.counters + kDroppedSlot);
    uint32_t* ctl = a.st.ctl;
    const uint32_t n = ctl[CTL_GATHER_COUNT];
    for (;;) {
        const uint32_t item = wave_grab_item(ctl + CTL_GATHER_HEAD);
        if (item >= n) break;
        const uint32_t w = a.st.gather_queue[item];
        const walk_trace_in_t wk = walk_load_trace_in(a.st.walks, a.st.walk_words, w);   // uniform address: broadcast
        const float dist = WT_TRAV_F(a, w, dist), depth = WT_TRAV_F(a, w, region_depth);
        const vec3 origin = trav_origin(a, w);
        const bool ballistic = WT_TRAV_U(a, w, ballistic) || cone_is_ray(wk.env);
        cone_t cone = wk.env;
        range_t slab{dist, dist + depth};
        bool any = true;
        if (!ballistic)
            cone.o = origin;   // the traced (self-intersection-offset) cone, like the record's triangles
        else {
            const float zdist = cone_axes(cone, dist).x * kMajorAxisToZScale;
            const range_t sr{dist - zdist / 2.f, dist + zdist / 2.f};
            cone_hit_t ch;
            const uint_list_t none{nullptr, 1u, 0u};
            coop_cone(a.sc, cone, sr, 1.f, csh, none, ch);
            any = ch.ntris + ch.overflow > 0;
            slab = cone_search_range(cone, sr, ch.dist, 1.f);
            __syncthreads();
        }
        uint32_t n_edges = 0, off = 0, dropped = 0;
        if (any) {
            const gather_out_t g = coop_gather(a.sc, cone, slab, cone, cone_frame(cone), slab, vec2{1.f, 1.f}, false, sh, false, true, nullptr, 1, &eg);
            __syncthreads();
            // (every id list goes into the round's edge pool: the walk's triangle-list slot is read again as triangles by PASS 1)
            off = edges_to_pool(a, g, eg, n_edges, dropped);
        }
        if (threadIdx.x == 0) {
            P.gather_info[w] = make_uint2(off, n_edges);
            if (dropped && a.count_stats) atomicAdd(a.st.counters + WT_COUNTER_SLOT(edge_overflow), (unsigned long long)dropped);
        }
        __syncthreads();
    }
}

// PASS 0: the round's queue; walks whose classified-edge set needs a wavefront are only queued for k_path_edges.  PASS 1: those walks, with it.
template <int PASS>
WT_D void path_interact_body(const launch_args_t& a, const path_state_t& P, int in, int first_round, uint32_t round) {
    __shared__ stack_entry_t lds[kLdsStack * kBlock];
    uint32_t* ctl = a.st.ctl;
    const uint32_t n = PASS ? ctl[CTL_GATHER_COUNT] : queue_count(ctl, in);
    if (!PASS && blockIdx.x == 0 && threadIdx.x == 0) interact_round_begin(ctl);
    bdpt_counters_t ctr;
    memset(&ctr, 0, sizeof(ctr));
    stack_entry_t spill[kSpillStack];
    stack_ref_t stack;
    lds_stack(lds, spill, stack);
    const uint32_t stream = a.sc.opts.integrator == INTEGRATOR_PATH_FORWARD ? STREAM_EMITTER_WALK : STREAM_SENSOR_WALK;
    const utd_pool_t pool{P.utd[round & 1u], ctl + CTL_UTD_COUNT0 + (round & 1u), P.utd_cap};
    const utd_edge_rec_t* prev_pool = P.utd[(round + 1u) & 1u];
    for (;;) {
        const uint32_t base = wave_grab(ctl + (PASS ? CTL_INTB_HEAD : CTL_HEAD_INTERACT));
        if (base >= n) break;
        const uint32_t qi = base + (threadIdx.x & 63);
        bool cont = false, carries_fsd = false, nee = false, gather = false;
        uint32_t w = 0;
        if (qi < n) {
            w = PASS ? a.st.gather_queue[qi] : queue_walk(a, ctl, in, qi, first_round);
            const uint64_t sample_id = sample_id_of(a, w);   // (one walk per sample)
            path_walk_t pw;
            soa_load(a.st.walks, a.st.walk_words, w, pw);
            trav_result_t tr;
            soa_load(a.st.trav, kTravWords, w, tr);
            uint32_t* slot = a.st.tris + (size_t)w * kTriListWords;
            const uint_list_t tris{slot, 1u, kMaxConeTris, reinterpret_cast<float*>(slot + kMaxConeTris)};
            path_defer_t defer;
            defer.have_prev_f = pw.has_fsd;   // evaluated by k_path_fsd (this round), one lane per wedge
            defer.prev_f = pw.has_fsd ? P.fsd_f[w] : 0.f;
            defer.defer_nee = 1;
            defer.nee_pending = 0;
            defer.split_gather = PASS ? 0u : 1u;
            defer.need_gather = 0;
            defer.has_gather = PASS ? 1u : 0u;
            defer.gather_n = 0;
            defer.gather_edges = nullptr;
            if (PASS) {
                const uint2 gi = P.gather_info[w];
                defer.gather_n = gi.y;
                defer.gather_edges = a.st.epool + gi.x;
            }
            cont = path_walk_step(a.sc, pw, tr, tris, prev_pool, pool, a.film, a.seed, sample_id, stream, stack, &ctr, &defer);
            gather = defer.need_gather != 0;
            if (!gather) {
                if (!cont) path_finish(a.sc, a.film, pw);
                pw.w.active = cont ? 1u : 0u;
                soa_store(a.st.walks, a.st.walk_words, w, pw);
                carries_fsd = cont && pw.has_fsd;
                nee = defer.nee_pending != 0;
                if (nee) P.nee_recs[w] = defer.nee;
            }
        }
        if (!PASS) wave_append(a.st.gather_queue, ctl + CTL_GATHER_COUNT, gather, w);
        queue_append(a, ctl, 1 - in, cont && !gather, w);
        wave_append(P.fsdq[(round + 1u) & 1u], ctl + CTL_FSDQ_COUNT0 + ((round + 1u) & 1u), carries_fsd, w);
        wave_append(P.neeq, ctl + CTL_NEEQ_COUNT, nee, w);
    }
    if (a.count_stats) flush_counters(a.st.counters, ctr);
}
#ifndef WTGPU_LB_PATH
#define WTGPU_LB_PATH 2
#endif
__global__ void __launch_bounds__(kBlock, WTGPU_LB_PATH) k_path_interact(launch_args_t a, const path_state_t* __restrict__ ps, int in, int first_round, uint32_t round) { path_interact_body<0>(a, *ps, in, first_round, round); }
__global__ void __launch_bounds__(kBlock, WTGPU_LB_PATH) k_path_interact_b(launch_args_t a, const path_state_t* __restrict__ ps, int in, uint32_t round) { path_interact_body<1>(a, *ps, in, 0, round); }

// plt_path, after the interaction step: next-event estimation towards the virtual sensor through the aperture the step just built (nee_forward,
// plt_path_detail.hpp:474-518) — one wavefront per walk: coherent UTD sum (coop_do_fsd), beam transform, integrate_beams, light-image splat.
__global__ void __launch_bounds__(64, 3) k_path_nee(launch_args_t a, const path_state_t* __restrict__ ps, uint32_t round) {
    const path_state_t& P = *ps;
    __shared__ stack_entry_t lds[kLdsStack * 64];
    uint32_t* ctl = a.st.ctl;
    const uint32_t n = ctl[CTL_NEEQ_COUNT];
    stack_entry_t spill[kSpillStack];
    stack_ref_t stack;
    lds_stack(lds, spill, stack, 64u);
    bdpt_counters_t ctr;
    memset(&ctr, 0, sizeof(ctr));
    const utd_edge_rec_t* cur_pool = P.utd[round & 1u];
    constexpr int G = WTGPU_FSD_GROUP, NG = 64 / G;
    const uint32_t group = (threadIdx.x & 63u) / (uint32_t)G;
    for (;;) {
        const uint32_t base = wave_grab0(ctl + CTL_NEEQ_HEAD, (uint32_t)NG);   // NG walks per wavefront, G lanes each
        if (base >= n) break;
        const uint32_t item = base + group;
        const bool have = item < n;
        const uint32_t w = have ? P.neeq[item] : 0u;
        // what the coherent sum reads of the walk's record (the whole record — two beams — only in the lane that splats)
        cone_t env;
        memset(&env, 0, sizeof(env));
        env.d = vec3{0.f, 0.f, 1.f};
        path_geo_t src_geo{vec3{0.f, 0.f, 0.f}, 0u, vec3{0.f, 0.f, 1.f}, kInvalid};
        vec3 dst{0.f, 0.f, 0.f};
        float k = 0.f;
        utd_aperture_t ap;
        memset(&ap, 0, sizeof(ap));
        if (have) {
            const path_nee_rec_t& r = P.nee_recs[w];
            env = r.beam.env;
            src_geo = path_geo_t{r.src_wp, r.src_kind, r.src_ng, r.src_tuid};
            dst = r.sd_beam.env.o;
            k = r.beam.k;
            soa_load(a.st.walks + offsetof(path_walk_t, ap) / 4, a.st.walk_words, w, ap);   // the aperture k_path_interact just stored
        }
        const float f = coop_do_fsd<G>(a.sc, env, src_geo, dst, ap, cur_pool + ap.edge_offset, k, stack, &ctr, have);
        if (have && (threadIdx.x & (uint32_t)(G - 1)) == 0 && f != 0.f) {
            const path_nee_rec_t r = P.nee_recs[w];
            beam_t fsd_beam = r.beam;
            beam_transform_region_interaction(fsd_beam, r.interaction_wp, r.dist, -r.sd_beam.env.d, f);
            const stokes_t sL = integrate_beams(r.sd_beam, fsd_beam);
            film_splat_direct(a.sc, a.film, r.element, sL * r.recp_spectral_pd, k);
            ctr.connections++;
            ctr.light_splats++;
        }
    }
    if (a.count_stats) flush_counters(a.st.counters, ctr);
}

// walks still active after the last round (iteration cap): backward transport splats what they gathered
__global__ void __launch_bounds__(kBlock) k_path_flush(launch_args_t a, int in) {
    const uint32_t n = queue_count(a.st.ctl, in);
    for (uint32_t qi = blockIdx.x * kBlock + threadIdx.x; qi < n; qi += kFlushGrid * kBlock) {
        const uint32_t w = queue_walk(a, a.st.ctl, in, qi, 0);
        path_walk_t pw;
        soa_load(a.st.walks, a.st.walk_words, w, pw);
        path_finish(a.sc, a.film, pw);
    }
}

}   // namespace wtk
