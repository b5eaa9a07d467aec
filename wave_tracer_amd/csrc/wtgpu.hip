// wave_tracer_amd — the batch driver of the HIP (gfx950 / CDNA4) wavefront implementation of plt_bdpt / plt_path behind the C-ABI
// (include/wtgpu.h): wtgpu_render*, wtgpu_join, timings.  wtgpu_host.h lists the other units of the host side.
//
// A render call cuts its samples into batches of the slice size (wtgpu_upload.hip: size_batches) and hands them round-robin to the state slices,
// each with its own HIP stream: the long tails of one batch — a handful of slow walks — overlap the bulk of the others.  The host reads
// nothing back while it enqueues; wtgpu_render_async returns with the last batches still PENDING, wtgpu_join finishes them.
// One batch, in launch order (batch_launcher_t):
//   first part   k_generate (k_path_generate), then the ROUNDS its walks are expected to need (expected_rounds: the recent batches' mean + a
//                margin).  A round: per-lane traversal (k_trace_refill, or the forms of wtgpu_trace_ab.hip), wave-cooperative traversal of the
//                handed-over queries (k_trace_heavy), pass A (k_interact), edges + pass B, region sums, pass C.  Every round kernel is
//                persistent: a fixed grid whose wavefronts grab queue items through a device-side head counter, the queue length comes from
//                the slice's control block.  Behind the rounds ONE launch of k_light_rounds (plt_bdpt): whatever the last walks still need,
//                round after round in one block, until the queue is empty or a walk needs a stage it does not hold; then a copy of the
//                control block to pinned memory and an event.
//   looks        when the slice is needed again, at wtgpu_join or before results are read, the host waits for that event (serve_pending:
//                whichever pending batch has its control block back is served) and LOOKS at it (finish_look): queue empty -> second part;
//                else more rounds (8, then 16, 32, 64; or the rest of the round the light kernel stopped in), light rounds and another copy.
//   second part  the connections (k_connect_*; plt_path: k_path_flush), the control block's final snapshot, the batch's closing event.
// All per-walk / per-sample state lives in HBM as one contiguous record per walk (wt::soa_load / soa_store, record-major).
//
// There is no CPU fallback: every entry point that computes requires a HIP device.
#include "wtgpu_host.h"

thread_local std::string g_err;

static void note_rounds(wtgpu_scene* s, uint32_t n) { s->rounds_hist[s->rounds_hist_n++ % 8u] = n; }
// Waits for one in-flight batch record and folds its event timings / control-block snapshot into the accumulators.
static int drain_rec(wtgpu_scene* s, chunk_rec_t& r) {
    if (!r.busy) return WTGPU_OK;
    HIP_CHECK(hipEventSynchronize(r.ev[r.ev_final]));
    const uint32_t rounds = r.h_ctl[CTL_ROUNDS];
    s->cap_hits += r.h_ctl[CTL_COUNT0 + (r.rounds_launched & 1u)] + r.h_ctl[CTL_BACK0 + (r.rounds_launched & 1u)];   // walks still active after the last round
    s->acc[4] += rounds;
    s->acc[5] += rounds;
    s->acc[6] += 1;
    s->rounds_launched_total += r.rounds_launched;
    if (s->knobs.timing) {
        // (an event pair that cannot be resolved contributes 0 ms: timings are diagnostics, the render itself has completed)
        auto elapsed = [](hipEvent_t a, hipEvent_t b) {
            float ms = 0.f;
            return hipEventElapsedTime(&ms, a, b) == hipSuccess ? ms : 0.f;
        };
        s->acc[0] += elapsed(r.ev[0], r.ev[1]);
        size_t e = 1;
        for (uint32_t k = 0; k < r.rounds_timed; ++k, e += 6) {
            static const int slot[6] = {1, 7, 2, 8, 9, 10};   // trace, heavy trace, pass A, edges + pass B, region flux, pass C
            for (int q = 0; q < 6; ++q) s->acc[slot[q]] += elapsed(r.ev[e + q], r.ev[e + q + 1]);
        }
        s->acc[3] += elapsed(r.ev[e], r.ev[r.ev_final]);   // (the connections' bracket: from the last timed round's end to the batch's end)
    }
    r.busy = false;
    return WTGPU_OK;
}

// ---- enqueueing a batch -------------------------------------------------------------------------------------------------------------
// The launches of one batch, in two parts with the host's looks between them (the file header has the sequence).  Nothing is ever dropped that a
// blind launch of every round (as until round 4) would have kept.
// Why: ~25 of the 96 rounds have work; the other ~70 x 9 launches only find an empty queue, and cost 2.6 % of a pass on the headline
// workload and 3 % on the 720 x 540 film (run r4r: the same build launching 96 / 48 / 32 rounds).
struct batch_launcher_t {
    wtgpu_scene* s;
    const wtgpu_scene::knobs_t& K;
    uint32_t grid_round = 0, grid_heavy = 0;
    bool path_mode = false;
    bool ev_fail = false;
    // WTGPU_HOST_PROF: host time spent inside each kind of launch call, per label.  A call site gets its slot when it first runs (hp_slot); the
    // fast path — neither knob set — never comes near any of this.
    static constexpr int kHpSlots = 64;
    bool hp_on = false, trace_on = false;
    double hp_t[kHpSlots] = {0};
    unsigned long hp_n[kHpSlots] = {0};
    static const char** hp_labels() {
        static const char* labels[kHpSlots] = {nullptr};
        return labels;
    }
    static int hp_slot(const char* label) {   // the slot of a label (labels are string literals; beyond kHpSlots - 1 labels the last slot collects the rest)
        static std::mutex m;
        std::lock_guard<std::mutex> l(m);
        const char** labels = hp_labels();
        int i = 0;
        while (i < kHpSlots - 1 && labels[i] && std::strcmp(labels[i], label) != 0) ++i;
        if (!labels[i]) labels[i] = label;
        return i;
    }
    explicit batch_launcher_t(wtgpu_scene* s_) : s(s_), K(s_->knobs) {
        // persistent grids: enough blocks to fill the 256 CUs; wavefronts pull work until the queue is empty
        grid_round = s->n_cus * K.round_blocks_per_cu;
        grid_heavy = s->n_cus * K.heavy_waves_per_cu;
        path_mode = s->host.opts.integrator != INTEGRATOR_BDPT;
        hp_on = K.host_prof != 0;
        trace_on = K.trace_launch != 0;
    }
#define HP_LAUNCH(kernel, ...)                                                                                            \
    do {                                                                                                                  \
        if (trace_on) {   /* WTGPU_TRACE_LAUNCH=1 (bring-up aid): every launch is named and waited for — the last line names a kernel that hangs */ \
            fprintf(stderr, "[wtgpu launch] %s ...", #kernel);                                                            \
            hipLaunchKernelGGL(kernel, __VA_ARGS__);                                                                      \
            const hipError_t e_ = hipDeviceSynchronize();                                                                 \
            fprintf(stderr, " done (%s)\n", hipGetErrorString(e_));                                                       \
        } else if (hp_on) {                                                                                                      \
            static const int slot_ = hp_slot(#kernel);                                                                    \
            const auto t0_ = std::chrono::steady_clock::now();                                                            \
            hipLaunchKernelGGL(kernel, __VA_ARGS__);                                                                      \
            hp_t[slot_] += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0_).count();     \
            hp_n[slot_]++;                                                                                                \
        } else                                                                                                            \
            hipLaunchKernelGGL(kernel, __VA_ARGS__);                                                                      \
    } while (0)
    void rec(chunk_rec_t& r, hipStream_t st_) {
        const auto hp0_ = std::chrono::steady_clock::now();
        if (s->knobs.timing && r.ev_used + 1 >= r.ev.size()) return;   // (rounds beyond what the event array holds — a batch with a very long walk — are not timed: the last event is the batch's)
        if (s->knobs.timing && hipEventRecord(r.ev[r.ev_used++], st_) != hipSuccess) ev_fail = true;
        if (hp_on) { static const int slot_ = hp_slot("hipEventRecord"); hp_t[slot_] += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - hp0_).count(); hp_n[slot_]++; }
    }
    uint32_t g_full(uint32_t nb) const { return std::min<uint32_t>(grid_round, ((path_mode ? 1u : 2u) * nb + kBlock - 1) / kBlock); }
    void generate(const launch_args_t& a, chunk_rec_t& r, hipStream_t st_) {
        r.ev_used = 0;
        r.rounds_launched = 0;
        r.rounds_timed = 0;
        rec(r, st_);
        if (path_mode)
            HP_LAUNCH(k_path_generate, dim3((a.nb + kBlock - 1) / kBlock), dim3(kBlock), 0, st_, a);
        else
            HP_LAUNCH(k_generate, dim3((a.nb + kBlock - 1) / kBlock), dim3(kBlock), 0, st_, a);
        rec(r, st_);
    }
    // stage_from (plt_bdpt): the first round of the range begins at this stage — 0 trace, 1 wave-cooperative trace, 3 k_edges, 5 region sums (a round k_light_rounds stopped in)
    int rounds(const launch_args_t& a, const path_state_t* ps, chunk_rec_t& r, hipStream_t st_, uint32_t r_begin, uint32_t r_end, int stage_from = 0) {
        const uint32_t nb = a.nb, walks_per_sample = path_mode ? 1u : 2u, gf = g_full(nb);
        const uint32_t grid_div_b = K.grid_div_b, grid_div_c = K.grid_div_c, grid_mul_flux = K.grid_mul_flux;   // persistent grids of the expensive-interaction passes relative to the round's
        const int dbg_stage = (int)K.dbg_stage;
        for (uint32_t round = r_begin; round < r_end; ++round) {
            const int in = (int)(round & 1u), first = round == 0 ? 1 : 0;
            if (s->knobs.timing && r.ev_used + 7 < r.ev.size()) r.rounds_timed++;   // (rec() below records this round's six events only while they fit)
            if (round == K.stagger_round && K.stagger_round > 0) {
                HIP_CHECK(hipEventRecord(r.ev_stagger, st_));
                s->ev_stagger_last = r.ev_stagger;
            }
            // the queue roughly halves every round and is normally empty after ~25: later rounds get smaller persistent grids
            // (an empty launch costs its grid size; a grid that turns out too small only takes longer, the wavefronts loop)
            uint32_t g0, gh;
            if (K.decay_q > 0) {
                // geometric schedule: the queue of round r holds ~ N q^r walks (q ~ 0.55 in the headline workload); grids follow with a safety
                // factor — an undersized persistent grid only takes longer, an oversized one on a short queue holds up the other streams
                const double f = std::min(1.0, (double)K.decay_c * std::pow(K.decay_q * .01, (double)round));
                g0 = std::max<uint32_t>(2u, (uint32_t)(gf * f));
                gh = std::max<uint32_t>(2u, (uint32_t)(std::min<uint32_t>(grid_heavy, walks_per_sample * nb) * f));
            } else {
                const uint32_t shrink = round < K.shrink_r1 ? 1u : (round < K.shrink_r2 ? K.shrink_f1 : K.shrink_f2);
                g0 = std::max<uint32_t>(1u, gf / shrink);
                gh = std::max<uint32_t>(1u, std::min<uint32_t>(grid_heavy, walks_per_sample * nb) / (round < K.shrink_r1 ? 1u : (round < K.shrink_r2 ? K.shrink_h1 : 32u)));
            }
            const int sf = round == r_begin ? stage_from : 0;
            if (sf <= 0 && dbg_stage >= 2 + 3 * (int)round) {
                if (round < K.trace_ab) {
                    const int rc = trace_ab_round(s, a, st_, in, first, round, g0);
                    if (rc) return rc;
                } else if (K.trace_sm || (K.trace_staged && round < K.trace_staged_rounds))
                    launch_trace_alt(s, a, st_, in, first, round, g0);
                else
                    HP_LAUNCH(k_trace_refill, dim3(g0), dim3(kBlock), 0, st_, a, in, first, round);
            }
            rec(r, st_);
            if (sf <= 1 && dbg_stage >= 3 + 3 * (int)round) {
                if (a.profile == 2)
                    HP_LAUNCH(k_trace_heavy_prof, dim3(gh), dim3(64), 0, st_, a);
                else
                    HP_LAUNCH(k_trace_heavy, dim3(gh), dim3(64), 0, st_, a);
            }
            rec(r, st_);
            if (path_mode) {
                if (round > 0) HP_LAUNCH(k_path_fsd, dim3(gh), dim3(64), 0, st_, a, ps, round);
                if (dbg_stage >= 4 + 3 * (int)round) HP_LAUNCH(k_path_interact, dim3(g0), dim3(kBlock), 0, st_, a, ps, in, first, round);
                HP_LAUNCH(k_path_edges, dim3(gh), dim3(64), 0, st_, a, ps);
                HP_LAUNCH(k_path_interact_b, dim3(std::max<uint32_t>(1u, g0 / 2u)), dim3(kBlock), 0, st_, a, ps, in, round);
                HP_LAUNCH(k_path_nee, dim3(gh), dim3(64), 0, st_, a, ps, round);
                rec(r, st_);
                rec(r, st_);
                rec(r, st_);
                rec(r, st_);
                continue;
            }
            if (sf > 2) {
            } else if (K.sorted_interact) {
                HP_LAUNCH(k_classify, dim3(g0), dim3(kBlock), 0, st_, a, in, first);
                if (K.sorted_interact >= 2)
                    HP_LAUNCH(k_interact_sorted, dim3(g0), dim3(kBlock), 0, st_, a, in);
                else {
                HP_LAUNCH(k_interact_diffuse, dim3(std::max<uint32_t>(1u, g0 / K.grid_div_cls[0])), dim3(kBlock), 0, st_, a, in);
                HP_LAUNCH(k_interact_dielectric, dim3(std::max<uint32_t>(1u, g0 / K.grid_div_cls[1])), dim3(kBlock), 0, st_, a, in);
                HP_LAUNCH(k_interact_spm, dim3(std::max<uint32_t>(1u, g0 / K.grid_div_cls[2])), dim3(kBlock), 0, st_, a, in);
                HP_LAUNCH(k_interact_any, dim3(std::max<uint32_t>(1u, g0 / K.grid_div_cls[3])), dim3(kBlock), 0, st_, a, in);
                }
            } else if (K.coop_io)
                HP_LAUNCH(k_interact_coop, dim3(g0), dim3(kBlock), 0, st_, a, in, first);
            else
                HP_LAUNCH(k_interact, dim3(g0), dim3(kBlock), 0, st_, a, in, first);
            rec(r, st_);
            if (sf <= 3) HP_LAUNCH(k_edges, dim3(gh), dim3(64), 0, st_, a);
            if (sf <= 4) HP_LAUNCH(k_interact_b, dim3(std::max<uint32_t>(1u, g0 / grid_div_b)), dim3(kBlock), 0, st_, a, in);
            rec(r, st_);
            HP_LAUNCH(k_flux_split, dim3(std::max<uint32_t>(1u, gh / 4u)), dim3(64), 0, st_, a);
            HP_LAUNCH(k_flux_tasks, dim3(std::max<uint32_t>(1u, gh * grid_mul_flux)), dim3(64), 0, st_, a);
            rec(r, st_);
            if (K.pass_c_tiers) {   // pass C in three lane shapes (kernels_fsd.hip): groups of eight lanes, then whole wavefronts for the tries that are left, then a lane per walk
                const uint32_t g_prep = std::max<uint32_t>(1u, gh / grid_div_c);
                // (a queue of at most WTGPU_PASS_C_THIN walks per wavefront of the grid: one wavefront per walk inside k_interact_c_prep, the thin rounds' shorter way)
                const uint32_t thin_below = (uint32_t)std::min<uint64_t>((uint64_t)K.pass_c_thin * g_prep, 0xFFFFFFFFull);
                HP_LAUNCH(k_interact_c_prep, dim3(g_prep), dim3(64), 0, st_, a, thin_below, K.pass_c_easy_tries);
                HP_LAUNCH(k_interact_c_wide, dim3(std::max<uint32_t>(1u, gh / grid_div_c)), dim3(64), 0, st_, a, K.pass_c_easy_tries);
                HP_LAUNCH(k_interact_c_hard_tries, dim3(std::max<uint32_t>(1u, gh / K.grid_div_hard)), dim3(WTGPU_HARD_BLOCK), 0, st_, a, K.pass_c_easy_tries);
                HP_LAUNCH(k_interact_c_commit, dim3(std::max<uint32_t>(1u, g0 / grid_div_b)), dim3(kBlock), 0, st_, a, in);
            } else {
                HP_LAUNCH(k_interact_c, dim3(std::max<uint32_t>(1u, gh / grid_div_c)), dim3(64), 0, st_, a, in);
                HP_LAUNCH(k_interact_c_hard, dim3(std::max<uint32_t>(1u, gh / K.grid_div_hard)), dim3(WTGPU_HARD_BLOCK), 0, st_, a, in);
            }
            rec(r, st_);
        }
        r.rounds_launched = r_end;
        return WTGPU_OK;
    }
    // k_light_rounds (kernels_walk.hip) behind the rounds launched so far: whatever the batch's last walks still need, in one launch of one block
    // (nothing, when the queue is empty; plt_bdpt only)
    void light(const launch_args_t& a, hipStream_t st_, uint32_t launched) {
        if (path_mode || !K.light_rounds || launched >= K.max_rounds) return;
        HP_LAUNCH(k_light_rounds, dim3(1), dim3(kBlock), 0, st_, a, (int)(launched & 1u), launched, K.max_rounds - launched);
    }
    // after the batch's last round: connections (plt_bdpt) / what is left of the walks (plt_path), the control block's snapshot, the closing event
    int tail(const launch_args_t& a, chunk_rec_t& r, hipStream_t st_) {
        const uint32_t nb = a.nb, gf = g_full(nb);
        if (path_mode) {
            HP_LAUNCH(k_path_flush, dim3(kFlushGrid), dim3(kBlock), 0, st_, a, (int)(r.rounds_launched & 1u));
        } else {
            const bool open = (uint32_t)s->host.opts.max_depth + 2 >= kKeyDim - 1;
            // staged connections (chunked, see upload_impl); subpaths beyond 17 vertices (open-ended strategy buckets: an item there holds several
            // strategies) keep a one-kernel form
            const bool staged = K.staged_connect && !open;
            // the one-kernel forms: by length class (an item is a sample, k_connect_class) or by strategy (an item is one strategy, k_connect_strat)
            const uint32_t by_class = !staged && K.connect_class ? 1u : 0u;
            HP_LAUNCH(k_connect_enum, dim3((nb + kEnumBlock - 1) / kEnumBlock), dim3(kEnumBlock), 0, st_, a, by_class);
            HP_LAUNCH(k_connect_scan, dim3(1), dim3(64), 0, st_, a, by_class);
            if (staged) {
                for (uint32_t c = 0; c < s->n_chunks; ++c) {
                    const uint32_t g = c == 0 ? gf : std::max<uint32_t>(1u, gf / 8u);   // (later chunks are normally empty: small grids, they only loop longer when not)
                    HP_LAUNCH(k_connect_eval, dim3(g), dim3(kBlock), 0, st_, a, c);
                    HP_LAUNCH(k_connect_shadow, dim3(g), dim3(kBlock), 0, st_, a, c);
                    HP_LAUNCH(k_connect_mis, dim3(g), dim3(kBlock), 0, st_, a, c);
                }
            } else if (by_class) {
                HP_LAUNCH(k_connect_class, dim3(gf), dim3(kBlock), 0, st_, a);
                if (open) HP_LAUNCH(k_connect_class_open, dim3(std::max<uint32_t>(1u, gf / 8u)), dim3(kBlock), 0, st_, a);
            } else {
                HP_LAUNCH(k_connect_strat, dim3(gf), dim3(kBlock), 0, st_, a);
                if (open) HP_LAUNCH(k_connect_strat_open, dim3(std::max<uint32_t>(1u, gf / 8u)), dim3(kBlock), 0, st_, a);
            }
            // (the tiled splat pays off when the batch holds most of the film's elements: it visits every row segment of the film)
            const uint32_t fw = a.film.width, fh = a.film.height, planes = film_planes(s->host.sensor);
            if (K.tiled_splat && s->host.sensor.rf_radius <= 1 && planes <= 16 && (uint64_t)nb * 2u >= (uint64_t)a.npix) {
                // one launch per (row % 3, segment % 2): the tiles that meet in a film element are added in a fixed order (kernels_connect.hip)
                for (uint32_t phase = 0; phase < kSplatPhases; ++phase) {
                    const uint32_t rows = splat_phase_rows(phase, fh), segs = splat_phase_segments(phase, splat_segments(fw));
                    if (rows * segs) HP_LAUNCH(k_connect_splat_tiled, dim3(rows * segs), dim3(kSplatBlock), 3 * kSplatCols * (planes + 1) * sizeof(double), st_, a, phase);
                }
            } else
                HP_LAUNCH(k_connect_splat, dim3((nb + kBlock - 1) / kBlock), dim3(kBlock), 0, st_, a);
        }
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(r.h_ctl, a.st.ctl, CTL_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, st_));
        r.ev_final = s->knobs.timing ? r.ev_used : 0;
        HIP_CHECK(hipEventRecord(r.ev[r.ev_final], st_));
        if (ev_fail) return fail(WTGPU_ERR_HIP, "hipEventRecord failed");
        r.busy = true;
        return WTGPU_OK;
    }
#undef HP_LAUNCH
    void report() const {
        if (!hp_on) return;
        const char* const* labels = hp_labels();
        for (int i = 0; i < kHpSlots; ++i)
            if (hp_n[i]) fprintf(stderr, "[host prof] %-22s %6lu calls %9.1f us total %7.2f us each\n", labels[i], hp_n[i], hp_t[i], hp_t[i] / hp_n[i]);
    }
};
static_assert(sizeof(launch_args_t) <= sizeof(wtgpu_scene::pending_t::args), "pending_t::args holds a launch block");

// rounds to launch up front: what the recent batches needed ON AVERAGE + a small margin.  (Not their maximum: the number of rounds a batch needs
// is set by its single longest walk — 36 on average on the headline workload, now and then 60 — and a batch that needs more than expected only
// costs another look, 8 rounds at a time.)  WTGPU_FIRST_ROUNDS forces a number: tests use 2, 96 = as before round 4.
static uint32_t expected_rounds(const wtgpu_scene* s) {
    if (s->knobs.first_rounds) return s->knobs.first_rounds;
    if (s->rounds_hist_n == 0) return std::min<uint32_t>(kMaxWalkIters, 32u);   // nothing seen yet: a guess
    const uint32_t n = std::min<uint32_t>(s->rounds_hist_n, 8u);
    uint32_t sum = 0;
    for (uint32_t i = 0; i < n; ++i) sum += s->rounds_hist[i];
    const uint32_t mean = (sum + n - 1) / n;
    // (Batches that need THOUSANDS of rounds — bidir_room: a handful of walks restart behind empty apertures 1800-3800 times per 4.2 M-sample batch — are
    // not given them up front: 4096 rounds are 37,000 launches, 330 ms of host time per batch, measured 11.9 Msamples/s against 15.8 with the rounds
    // added as the host sees the queue still filled.  Both are far from the 36.1 of WTGPU_MAX_ROUNDS=96, which drops those walks: DESIGN.md §0.)
    return std::min<uint32_t>(kMaxWalkIters, mean + s->knobs.rounds_margin);
}
// One LOOK at the batch pending on slice k, whose ev_mid has completed (its control block is in r.h_mid): is the round queue empty?  Then the
// connections (the batch's second part) are enqueued and the batch is no longer pending.  If not — a batch whose walks outlasted the expectation —
// the next rounds are enqueued with another copy of the control block behind them, and the batch waits for its next look.
static int finish_look(wtgpu_scene* s, size_t k, batch_launcher_t& L) {
    wtgpu_scene::pending_t& p = s->pending[k];
    chunk_rec_t& r = *p.rec;
    launch_args_t a;
    std::memcpy(&a, p.args, sizeof(a));
    hipStream_t st_ = s->streams[k];
    uint32_t& launched = p.launched;
    const bool light = !L.path_mode && s->knobs.light_rounds != 0;   // (a k_light_rounds launch stands behind the rounds enqueued so far)
    uint32_t stop = 0;
    if (light && launched < s->knobs.max_rounds) {
        launched += r.h_mid[CTL_LIGHT_DONE];
        stop = r.h_mid[CTL_LIGHT_STOP];
        s->light_rounds_run += r.h_mid[CTL_LIGHT_DONE];
    }
    bool done = false;
    if (s->knobs.tail_diag) {   // WTGPU_TAIL_DIAG: why the host was called back, printed at exit
        static unsigned long long looks = 0, by_stop[8] = {0}, light_done = 0, left_sum = 0;
        static bool reg = false;
        if (!reg) { reg = true; atexit([] { fprintf(stderr, "[tail diag] looks %llu (stop 0/1/2/3/4: %llu %llu %llu %llu %llu), light rounds %llu, walks left at looks (sum) %llu\n", looks, by_stop[0], by_stop[1], by_stop[2], by_stop[3], by_stop[4], light_done, left_sum); }); }
        looks++; by_stop[stop < 8 ? stop : 7]++; light_done += light ? r.h_mid[CTL_LIGHT_DONE] : 0;
        left_sum += r.h_mid[CTL_COUNT0 + (launched & 1u)] + r.h_mid[CTL_BACK0 + (launched & 1u)];
    }
    if (stop >= 1 && stop <= 3) {
        // a walk needs a stage the light kernel does not hold: the rest of THAT round by the ordinary kernels, then light again
        static const int from[4] = {0, 1, 3, 5};
        const int rc = L.rounds(a, s->d_path_slices[k], r, st_, launched, launched + 1, from[stop]);
        if (rc) return rc;
        launched += 1;
    } else {
        const uint32_t q = launched & 1u;
        const uint32_t left = r.h_mid[CTL_COUNT0 + q] + r.h_mid[CTL_BACK0 + q];
        if (left == 0) {
            note_rounds(s, std::min<uint32_t>(r.h_mid[CTL_ROUNDS], kMaxWalkIters));
            done = true;
        } else if (launched >= s->knobs.max_rounds)
            done = true;   // (WTGPU_MAX_ROUNDS: what is left is dropped and counted, drain_rec)
        else {
            s->round_fallbacks++;
            const uint32_t next = std::min<uint32_t>(s->knobs.max_rounds, launched + p.rounds_step);
            const int rc = L.rounds(a, s->d_path_slices[k], r, st_, launched, next);
            if (rc) return rc;
            launched = next;
            p.rounds_step = std::min<uint32_t>(64u, p.rounds_step * 2u);   // (a batch far beyond its expectation is not looked at every 8 rounds)
        }
    }
    if (done) {
        p.active = false;
        r.rounds_launched = launched;
        return L.tail(a, r, st_);
    }
    L.light(a, st_, launched);
    HIP_CHECK(hipMemcpyAsync(r.h_mid, a.st.ctl, CTL_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipEventRecord(r.ev_mid, st_));
    return WTGPU_OK;
}
// Serves the pending batches — whichever has its control block back gets its look (finish_look) — until the one on slice k (k = npos: every one)
// is finished.  The calling thread waits here for the GPU; it does not wait for ONE batch while another's stream stands idle behind a finished
// first part (round 6: a batch of bidir_room needs fifteen looks, a hundred light rounds apart, for the walks that restart thousands of times).
static int serve_pending(wtgpu_scene* s, size_t k, batch_launcher_t& L) {
    const size_t n = s->pending.size();
    for (;;) {
        bool any = false, progressed = false;
        for (size_t j = 0; j < n; ++j) {
            wtgpu_scene::pending_t& p = s->pending[j];
            if (!p.active) continue;
            if (k != (size_t)-1 && !s->pending[k].active) break;
            any = true;
            const hipError_t q = hipEventQuery(p.rec->ev_mid);
            if (q == hipSuccess) {
                const int rc = finish_look(s, j, L);
                if (rc) return rc;
                progressed = true;
            } else if (q != hipErrorNotReady)
                HIP_CHECK(q);
            else
                (void)hipGetLastError();   // (not ready is not an error: nothing of it may reach the next hipGetLastError check)
        }
        if (k != (size_t)-1 ? !s->pending[k].active : !any) return WTGPU_OK;
        if (!progressed) {
            std::this_thread::sleep_for(std::chrono::microseconds(20));   // (0 / 5 / 20 / 100 us measured alike: the looks, not the polling, are the tail)
        }
    }
}
static int finish_all_pending(wtgpu_scene* s) {
    bool any = false;
    for (const auto& p : s->pending) any = any || p.active;
    if (!any) return WTGPU_OK;
    batch_launcher_t L(s);
    return serve_pending(s, (size_t)-1, L);
}
int drain_all(wtgpu_scene* s) {
    {
        const int rc = finish_all_pending(s);
        if (rc) return rc;
    }
    for (auto& r : s->recs) {
        const int rc = drain_rec(s, r);
        if (rc) return rc;
    }
    return WTGPU_OK;
}

extern "C" {

const char* wtgpu_last_error(void) { return g_err.c_str(); }

int wtgpu_join(wtgpu_scene* s, void* stream_) {
    if (!s || !s->uploaded) return fail(WTGPU_ERR_INVALID, "scene not uploaded");
    hipStream_t caller = static_cast<hipStream_t>(stream_);
    device_guard_t guard(s->device);
    {   // (blocks until the first parts of the pending batches have run: their second parts are enqueued here)
        const int rc = finish_all_pending(s);
        if (rc) return rc;
    }
    for (size_t k = 0; k < s->slices.size(); ++k) {
        HIP_CHECK(hipEventRecord(s->ev_done[k], s->streams[k]));
        HIP_CHECK(hipStreamWaitEvent(caller, s->ev_done[k], 0));
    }
    return WTGPU_OK;
}

int wtgpu_render(wtgpu_scene* s, void* stream_, double* d_value, double* d_weight, double* d_light, uint64_t sb, uint64_t se, uint64_t seed) {
    const int rc = wtgpu_render_async(s, stream_, d_value, d_weight, d_light, sb, se, seed);
    return rc ? rc : wtgpu_join(s, stream_);
}

int wtgpu_render_async(wtgpu_scene* s, void* stream_, double* d_value, double* d_weight, double* d_light, uint64_t sb, uint64_t se, uint64_t seed) {
    if (!s || !s->uploaded) return fail(WTGPU_ERR_INVALID, "scene not uploaded");
    if (!d_value || !d_weight || !d_light || se < sb) return fail(WTGPU_ERR_INVALID, "bad film pointers / sample range");
    hipStream_t caller = static_cast<hipStream_t>(stream_);
    device_guard_t guard(s->device);
    const scene_t& h = s->host;
    const uint64_t npix = (uint64_t)h.sensor.width * h.sensor.height;
    const uint64_t total = npix * (se - sb);
    if (total == 0) return WTGPU_OK;
    launch_args_t a;
    static_assert(sizeof(launch_args_t) <= 984, "by-value kernel arguments beyond 1 KB serialise the streams (see path_state_t)");
    a.sc = s->dev;
    a.film = film_t{d_value, d_weight, d_light, h.sensor.width, h.sensor.height, h.sensor.channels};
    a.seed = seed;
    a.npix = (uint32_t)npix;
    a.sample_begin = sb;
    const wtgpu_scene::knobs_t& K = s->knobs;   // environment knobs, read once at upload
    a.count_stats = K.count_stats;
    a.cone_budget = K.cone_budget;
    a.profile = K.profile;
    a.coop_aperture_min = K.coop_aperture_min;
    a.heavy_probe = K.heavy_probe;
    a.split_queues = K.split_queues;
    a.lane_cache = K.lane_cache;
    a.heavy_cache = K.heavy_cache;
    a.flux_task_tris = K.flux_task_tris;
    // Bounded triangle lists (64) are the fast path of an interaction region; a region that overflows its list is handled exactly by
    // walks of the WHOLE region: primary triangle (resolve_primary), classified edges (k_edges), intercepted power (k_flux_*).
    // WTGPU_NO_LISTS=1 (plt_bdpt, diagnostic): no lists at all, every region is gathered.
    // bit 0: the cone queries keep the region's bounded triangle list; bit 1 (plt_bdpt, WTGPU_PRIMARY_AXIS=1): the triangle under the beam axis of EVERY
    // diffusive hit comes from the trace kernels' axis query (as it does for regions beyond the list), not from a scan of the list in pass A
    a.collect_list = ((h.opts.integrator != INTEGRATOR_BDPT || !K.no_lists) ? 1u : 0u) | ((h.opts.integrator == INTEGRATOR_BDPT && K.primary_axis) ? 2u : 0u);
    batch_launcher_t L(s);

    // the internal streams start after everything already enqueued on the caller's stream ...
    HIP_CHECK(hipEventRecord(s->ev_begin, caller));
    const size_t n_slices = s->slices.size();
    std::vector<char> used(n_slices, 0);
    const uint64_t cap = s->slices[0].cap;
    for (uint64_t j0 = 0; j0 < total; j0 += cap) {
        const size_t k = s->slice_next++ % n_slices;
        hipStream_t st_ = s->streams[k];
        {   // the batch that still holds this slice gets its second part first (the host waits for its first part here: by now the other
            // slices' batches have been enqueued behind it, so the GPU is not idle meanwhile)
            const int rc = s->pending[k].active ? serve_pending(s, k, L) : WTGPU_OK;
            if (rc) return rc;
        }
        if (!used[k]) {
            HIP_CHECK(hipStreamWaitEvent(st_, s->ev_begin, 0));
            used[k] = 1;
        }
        chunk_rec_t& r = s->recs[s->rec_next];
        s->rec_next = (s->rec_next + 1) % s->recs.size();
        int rc = drain_rec(s, r);   // recycles the oldest record (blocks only when > recs.size() batches are in flight)
        if (rc) return rc;
        const uint32_t nb = (uint32_t)std::min<uint64_t>(cap, total - j0);
        // WTGPU_STAGGER_ROUND=r (diagnostic, default off): a batch starts when the previous one (on the previous stream) has finished its round r.
        // Measured on the headline workload with 4 streams: r = 0 / 3 / 6 / 10 / 16 -> 151 / 150 / 161 / 200 / 263 ms per pass: the first
        // rounds ARE most of a batch, holding the next batch back only idles the GPU.
        if (K.stagger_round > 0 && s->ev_stagger_last && n_slices > 1) HIP_CHECK(hipStreamWaitEvent(st_, s->ev_stagger_last, 0));
        a.st = s->slices[k];
        a.j0 = j0;
        a.nb = nb;
        const uint32_t r1 = expected_rounds(s);
        L.generate(a, r, st_);
        rc = L.rounds(a, s->d_path_slices[k], r, st_, 0, r1);
        if (rc) return rc;
        HIP_CHECK(hipGetLastError());
        L.light(a, st_, r1);   // (the batch's last walks — a handful that restart thousands of times in some scenes — without another host round trip)
        HIP_CHECK(hipMemcpyAsync(r.h_mid, a.st.ctl, CTL_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, st_));
        HIP_CHECK(hipEventRecord(r.ev_mid, st_));
        wtgpu_scene::pending_t& p = s->pending[k];
        std::memcpy(p.args, &a, sizeof(a));
        p.rec = &r;
        p.launched = r1;
        p.rounds_step = 8;
        p.active = true;

    }
    L.report();
    // (wtgpu_join enqueues what is pending and makes the caller's stream continue after all of it)
    s->samples_rendered += total;
    return WTGPU_OK;
}

int wtgpu_last_render_timings(wtgpu_scene* s, float out[12]) {
    if (!s || !out || !s->uploaded) return fail(WTGPU_ERR_INVALID, "scene not uploaded");
    const int rc = drain_all(s);
    if (rc) return rc;
    for (int i = 0; i < 12; ++i) out[i] = (float)s->acc[i];
    out[11] = s->acc[6] > 0 ? (float)((double)s->rounds_launched_total / s->acc[6]) : (float)kMaxWalkIters;   // rounds launched per batch (mean)
    return WTGPU_OK;
}

}   // extern "C"
