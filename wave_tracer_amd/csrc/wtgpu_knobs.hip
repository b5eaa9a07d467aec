// wave_tracer_amd — the table of the environment knobs and read_knobs (wtgpu_knobs.h).  Plain C++: nothing here needs the HIP headers; it is a
// .hip unit only so that it is compiled with the flags of the other units (a -DWT_MAX_WALK_ITERS reaches its clamps as well).
// A knob is one line: to add one, add a field to knobs_t and a line here.  Tuning knobs change speed, never results, unless their help says so.
#include "wtgpu_knobs.h"

#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>

#include "wt/bdpt.h"

using wt::kMaxWalkIters;
using wt::kWalkIterLimit;

#define K(field) &knobs_t::field
static constexpr long long kU32 = 0xFFFFFFFFll;
const knob_t kKnobs[] = {
    // ---- what the kernels are told (launch_args_t)
    {"WTGPU_CONE_BUDGET", K(cone_budget), KNOB_U32, kKnobConeBudget, 0, kU32, "work units one lane may spend on a cone query before it is handed to a wavefront (wtgpu_kernels.h: kConeBudget)"},
    {"WTGPU_COUNT_STATS", K(count_stats), KNOB_U32, 1, 0, kU32, "0: the kernels keep no statistics (wtgpu_kernels.h: launch_args_t::count_stats)"},
    {"WTGPU_SPLIT_QUEUES", K(split_queues), KNOB_U32, 1, 0, kU32, "round queues keep sensor and emitter walks apart; 0: one mixed queue (A/B)"},
    {"WTGPU_LANE_CACHE", K(lane_cache), KNOB_U32, 1, 0, kU32, "0 (diagnostic): the per-lane traversal without its remembered rejecting triangles"},
    {"WTGPU_HEAVY_CACHE", K(heavy_cache), KNOB_U32, 1, 0, kU32, "0 (diagnostic): the wave-cooperative traversal without its remembered rejecting triangles"},
    {"WTGPU_HEAVY_PROBE", K(heavy_probe), KNOB_U32, 1, 0, kU32, "k_trace_heavy: any-hit probe of the near slab before the handed-over cone query too; 0: off"},
    {"WTGPU_COOP_APERTURE_MIN", K(coop_aperture_min), KNOB_U32, 8, 0, kU32, "segments from which an aperture is built by a wavefront; 0xFFFFFFFF: every aperture by a single lane of pass B"},
    {"WTGPU_FLUX_TASK_TRIS", K(flux_task_tris), KNOB_U32, kKnobFluxTaskTris, 64, kU32, "triangles per region-sum task (k_flux_split / k_flux_tasks; wtgpu_kernels.h: kFluxTaskTris)"},
    {"WTGPU_PROFILE", K(profile), KNOB_U32, 0, 0, kU32, "1 / 2 / 3: in-kernel clock breakdowns, printed by wtgpu_get_counters (wtgpu_counters.hip)"},
    {"WTGPU_NO_LISTS", K(no_lists), KNOB_PRESENT, 0, 0, 1, "set (any value; plt_bdpt, diagnostic): no bounded triangle lists, every interaction region is gathered"},
    {"WTGPU_PRIMARY_AXIS", K(primary_axis), KNOB_U32, 0, 0, kU32, "1 (plt_bdpt): the triangle under the beam axis of every diffusive hit comes from the trace kernels' axis query"},
    // ---- slices and batches (wtgpu_scene.hip: size_batches / alloc_slice)
    {"WTGPU_STREAMS", K(streams), KNOB_INT, 3, 1, INT_MAX, "state slices = internal streams; ms per pass at 1 / 2 / 3 / 4 / 6 / 8: 158 / 142 / 130 / 142 / 157 / 206 (headline)"},
    {"WTGPU_STATE_GB", K(state_gb), KNOB_INT, 224, 1, INT_MAX, "budget of the per-batch state of all slices, GB (of the MI355X's 288; never more than 85 % of what is free): deep scenes get smaller batches"},
    {"WTGPU_TIMING", K(timing), KNOB_NONZERO, 1, 0, 1, "0: no per-kernel HIP events (wtgpu_last_render_timings reads zeros)"},
    {"WTGPU_CONN_POOL", K(conn_pool), KNOB_U32, 16, 1, kU32, "staged connections: pending connections per sample of a chunk"},
    // ---- rounds of a batch (wtgpu.hip: expected_rounds, finish_look)
    {"WTGPU_FIRST_ROUNDS", K(first_rounds), KNOB_U32, 0, 0, kMaxWalkIters, "rounds launched up front; 0: adaptive (the recent batches' mean + WTGPU_ROUNDS_MARGIN); tests use 2, 96 = as before round 4"},
    {"WTGPU_ROUNDS_MARGIN", K(rounds_margin), KNOB_U32, 2, 0, kU32, "rounds added to the recent batches' mean"},
    {"WTGPU_LIGHT_ROUNDS", K(light_rounds), KNOB_U32, 1, 0, kU32, "0: the rounds beyond the expected ones as ordinary rounds only (k_light_rounds off)"},
    {"WTGPU_MAX_ROUNDS", K(max_rounds), KNOB_U32, kWalkIterLimit, 8, kWalkIterLimit, "rounds a batch may get before its surviving walks are dropped and counted (CHANGES RESULTS below the default, wt/bdpt.h kWalkIterLimit: nothing is dropped in any workload seen; 96 = rounds 1-5)"},
    {"WTGPU_STAGGER_ROUND", K(stagger_round), KNOB_U32, 0, 0, kMaxWalkIters - 1, "r > 0 (diagnostic): a batch starts when the previous one has finished its round r; 0: all streams start at once.  4 streams, r = 0 / 3 / 6 / 10 / 16: 151 / 150 / 161 / 200 / 263 ms per pass"},
    // ---- persistent-grid sizes (wtgpu.hip: batch_launcher_t::rounds)
    {"WTGPU_SHRINK_R1", K(shrink_r1), KNOB_U32, 8, 0, kU32, "from this round on the round kernels' grids are divided by WTGPU_SHRINK_F1 (heavy: WTGPU_SHRINK_H1)"},
    {"WTGPU_SHRINK_F1", K(shrink_f1), KNOB_U32, 4, 1, kU32, "see WTGPU_SHRINK_R1"},
    {"WTGPU_SHRINK_R2", K(shrink_r2), KNOB_U32, 16, 0, kU32, "from this round on the grids are divided by WTGPU_SHRINK_F2 (heavy: 32)"},
    {"WTGPU_SHRINK_F2", K(shrink_f2), KNOB_U32, 32, 1, kU32, "see WTGPU_SHRINK_R2"},
    {"WTGPU_SHRINK_H1", K(shrink_h1), KNOB_U32, 4, 1, kU32, "see WTGPU_SHRINK_R1"},
    {"WTGPU_DECAY_Q", K(decay_q), KNOB_U32, 0, 0, kU32, "per cent; > 0: grids follow WTGPU_DECAY_C x q^round instead of the step schedule above"},
    {"WTGPU_DECAY_C", K(decay_c), KNOB_U32, 4, 1, kU32, "safety factor of the geometric schedule"},
    {"WTGPU_HEAVY_WAVES", K(heavy_waves_per_cu), KNOB_U32, 8, 1, kU32, "wavefronts per CU of the wave-per-item kernels; swept 6 / 8 / 10 / 12 / 16 / 24 / 32: 169.6 / 168.0 / 171.6 / 174.3 / 176 / 181 / 183 ms per pass"},
    {"WTGPU_ROUND_BLOCKS", K(round_blocks_per_cu), KNOB_U32, 8, 1, kU32, "blocks per CU of the round kernels' persistent grids"},
    {"WTGPU_GRID_B", K(grid_div_b), KNOB_U32, 4, 1, kU32, "pass B's grid relative to the round's (divisor)"},
    {"WTGPU_GRID_C", K(grid_div_c), KNOB_U32, 1, 1, kU32, "pass C's grid (divisor); 2 until round 4; 1: bidir_room 33.6 -> 33.9, cornell 25.15 -> 25.35 Msamples/s, pass C's bracket 69 -> 56 / 93 -> 65 ms"},
    {"WTGPU_GRID_HARD", K(grid_div_hard), KNOB_U32, 4, 1, kU32, "k_interact_c_hard's grid (divisor)"},
    {"WTGPU_GRID_FLUX", K(grid_mul_flux), KNOB_U32, 2, 1, kU32, "k_flux_tasks' grid (multiplier)"},
    // ---- alternative kernel forms (A/B; DESIGN.md §4 has the measurements: the one-kernel forms are 1-6 % faster on the headline workload and
    //      are the default; the sorted / staged forms move a third of the bytes)
    {"WTGPU_SORTED_INTERACT", K(sorted_interact), KNOB_U32, 0, 0, kU32, "pass A: 0 k_interact (one kernel, every walk); 1 k_classify + one kernel per material class; 2 k_classify + k_interact_sorted"},
    {"WTGPU_COOP_IO", K(coop_io), KNOB_U32, 0, 0, kU32, "1: pass A with wave-cooperative record transfers (k_interact_coop)"},
    {"WTGPU_STAGED_CONNECT", K(staged_connect), KNOB_U32, 0, 0, kU32, "connections: 0 k_connect_strat (one kernel per strategy item); 1 k_connect_eval -> k_connect_shadow -> k_connect_mis, in chunks"},
    {"WTGPU_CONNECT_CLASS", K(connect_class), KNOB_U32, 1, 0, kU32, "connections (the one-kernel form): 0 k_connect_strat (an item is one strategy of a sample); 1 k_connect_class (an item is a sample, bucketed by the lengths of its subpaths, all of its strategies in a row; DESIGN.md §4)"},
    {"WTGPU_PASS_C_TIERS", K(pass_c_tiers), KNOB_U32, 1, 0, 1, "pass C: 1 in three lane shapes (k_interact_c_prep: 8 lanes per walk, power sum and tries 0-7; k_interact_c_wide / _hard_tries: tries only; k_interact_c_commit: lane = walk); 0 k_interact_c / k_interact_c_hard, one wavefront per walk (A/B; the results do not depend on it; DESIGN.md §4)"},
    {"WTGPU_PASS_C_EASY_TRIES", K(pass_c_easy_tries), KNOB_U32, 512, 8, kU32, "pass C in tiers: the try from which four wavefronts take a walk over (kernels_fsd.hip: kEasyTries); the tests move it to drive walks into every tier, the results do not depend on it"},
    {"WTGPU_PASS_C_THIN", K(pass_c_thin), KNOB_U32, 8, 0, kU32, "pass C in tiers: a round whose queue holds at most this many walks per wavefront of k_interact_c_prep's grid takes one wavefront per walk there (the thin rounds are bound by their longest walk, not by lanes); 0: groups of eight always (the tests); the results do not depend on it"},
    {"WTGPU_TILED_SPLAT", K(tiled_splat), KNOB_U32, 1, 0, kU32, "0: the plain per-sample splat kernel"},
    {"WTGPU_TRACE_STAGED", K(trace_staged), KNOB_U32, 1, 0, kU32, "1: the traversal in stages (k_tr_axis / k_tr_cone / k_tr_policy / k_tr_tail) ..."},
    {"WTGPU_TRACE_STAGES", K(trace_stages), KNOB_U32, 3, 1, 16, "... with this many cone stages before the tail ..."},
    {"WTGPU_TRACE_STAGED_ROUNDS", K(trace_staged_rounds), KNOB_U32, 4, 0, kU32, "... for the first so many rounds of a batch (the long ones: a stage is a launch, and a short round is bound by its launches)"},
    {"WTGPU_TRACE_SM", K(trace_sm), KNOB_U32, 0, 0, kU32, "1: the phase-machine trace kernel (k_trace_sm)"},
    {"WTGPU_TRACE_AB", K(trace_ab), KNOB_U32, 0, 0, kU32, "n: the first n rounds replay their trace queue through both trace kernels, timed, outputs compared (wtgpu_trace_ab.hip)"},
    {"WTGPU_DEVELOP_PER_PIXEL", K(develop_per_pixel), KNOB_U32, 0, 0, 1, "k_develop: 0 one lane per plane element; 1 one lane per pixel (A/B: tools/bench_develop.py)"},
    {"WTGPU_TONEMAP_LDS_TABLE", K(tonemap_lds_table), KNOB_U32, 0, 0, 1, "k_develop_tonemap: 1 every block stages the colour table in LDS; 0 the lanes read it through the caches (A/B: tools/bench_develop.py)"},
    {"WTGPU_FILM_POLAR_STAGED", K(film_polar_staged), KNOB_U32, 1, 0, 1, "k_film_polar: 1 a wavefront loads its chunk's planes contiguously, develops them and hands them to the pixels' lanes through LDS; 0 every lane loads its own pixels' planes (A/B: tools/bench_film_polar.py)"},
    {"WTGPU_FILM_DENOISE_FUSED", K(film_denoise_fused), KNOB_U32, 2, 0, 2, "k_denoise_filter: 1 a block filters both directions (A by B's weights, B by A's) in one launch and keeps the first in registers; 0 one launch per direction, the first leaving its result in scratch memory; 2 whichever was measured faster for the film's planes: 1 up to 4 planes, 0 for 12 (A/B: tools/bench_film_denoise.py)"},
    {"WTGPU_FILM_DENOISE_GUIDE_LDS", K(film_denoise_guide_lds), KNOB_U32, 0, 0, 1, "k_denoise_filter, guided: 1 the guide planes of the candidate square go into LDS beside the halo where the sum fits 64 KB (from global memory where it does not); 0 every lane reads g(q) from global memory where it reads x(q) (A/B: tools/bench_film_denoise_guided.py; the results do not depend on it)"},
    {"WTGPU_FIRST_HIT_PER_SAMPLE", K(first_hit_per_sample), KNOB_U32, 1, 0, 1, "k_first_hit: 1 one lane per sample where a pixel's samples fit a wavefront (k_first_hit_wave: the lanes of a pixel exchange their samples through LDS, lane j sums float j in sample order); 0 one lane per pixel always (A/B: tools/bench_first_hit.py; the results do not depend on it); k_first_hit_material / k_first_hit_material_wave follow it too (tools/bench_first_hit_material.py)"},
    {"WTGPU_LOS_PER_SAMPLE", K(los_per_sample), KNOB_U32, 1, 0, 1, "wtgpu_line_of_sight: 1 one lane per (element, sample) where the sensor's own elements are sampled and an element's samples fit a wavefront (k_los_sample: the lanes walk the emitters together and exchange their samples through LDS, lane j sums float j in sample order); 0 one lane per (element, emitter) always (k_los_pair) (A/B: tools/bench_los.py; the results do not depend on it)"},
    {"WTGPU_FILM_ZONAL_LDS", K(film_zonal_lds), KNOB_U32, 1, 0, 1, "k_film_zonal: 1 every block accumulates in a table in LDS wherever the table of n_zones x planes entries fits the 64 KB a launch may ask for, and flushes it once (measured 7 to 165 times faster wherever it fits); 0 the atomics go straight to global memory always (A/B: tools/bench_film_zonal.py; both forms are exact, the results do not depend on it)"},
    {"WTGPU_FILM_ZONAL_BLOCKS", K(film_zonal_blocks), KNOB_U32, 0, 0, kU32, "k_film_zonal: n > 0 caps the grid at n blocks (the tests: one wavefront takes many chunks of a small film); 0 the film statistics' rule (kernels_film.h: film_grid_blocks); the results do not depend on it"},
    {"WTGPU_FILM_SEGMENTS_TILED", K(film_segments_tiled), KNOB_U32, 0, 0, 1, "wtgpu_film_segments_device, the first two phases: 1 a block labels a tile of 64 x 32 pixels in LDS (k_seg_tile: the row runs and a union-find with ds_min_u32) and the global merge unions across tile borders only (k_seg_border); 0 the row runs of a wavefront's 64 pixels (k_seg_runs) and every remaining link in global memory (k_seg_merge), the default: measured level with the tiled form on percolation and spiral planes and 7 to 22 % faster on coherent ones; the tiled form is ahead on one plane of 28, critical percolation with 8 neighbours at 1920 x 1088, at 0.85 - 0.88 (docs/FEATURES.md; A/B: tools/bench_film_segments.py; the result is canonical and does not depend on it)"},
    {"WTGPU_FILM_DISTANCE_GROUPS", K(film_distance_groups), KNOB_U32, 1, 0, 1, "wtgpu_film_distance_device, k_dist_rows: 1 a lane's outward search over the columns ends at |dx| = 64 and goes on group by group, a 64-column group being skipped where (distance to its nearer edge)^2 + (its min |dy|)^2 cannot reach or tie the best; 0 the outward search alone, column by column to the end (docs/FEATURES.md; A/B: tools/bench_film_distance.py; the result is canonical and does not depend on it)"},
    // ---- diagnostics and bring-up aids
    {"WTGPU_DEBUG_STAGE", K(dbg_stage), KNOB_INT, 1 << 30, INT_MIN, INT_MAX, "bring-up aid: stops launching the round kernels after stage n (INVALID RESULTS)"},
    {"WTGPU_HOST_PROF", K(host_prof), KNOB_PRESENT, 0, 0, 1, "set: host time spent inside each kind of launch call, printed per render call"},
    {"WTGPU_TRACE_LAUNCH", K(trace_launch), KNOB_PRESENT, 0, 0, 1, "set (bring-up aid): every launch is named and waited for — the last line names a kernel that hangs"},
    {"WTGPU_TAIL_DIAG", K(tail_diag), KNOB_PRESENT, 0, 0, 1, "set: why the host was called back for a pending batch, printed at exit (DESIGN.md §9)"},
    {"WTGPU_TRACE_AB_VERBOSE", K(trace_ab_verbose), KNOB_PRESENT, 0, 0, 1, "set: one line per round replayed by WTGPU_TRACE_AB"},
};
#undef K
const size_t kNumKnobs = sizeof(kKnobs) / sizeof(kKnobs[0]);

void read_knobs(knobs_t& k) {
    for (size_t i = 0; i < kNumKnobs; ++i) {
        const knob_t& d = kKnobs[i];
        const char* e = getenv(d.name);
        long long v = d.dflt;
        if (d.kind == KNOB_PRESENT) v = e ? 1 : 0;
        else if (e && d.kind == KNOB_U32) v = std::min<long long>(std::max<long long>(0, strtoll(e, nullptr, 10)), kU32);   // negative -> 0; the whole uint32 range
        else if (e && d.kind == KNOB_INT) v = atoi(e);
        else if (e) v = atoi(e) != 0;
        k.*d.field = (uint32_t)std::min(d.hi, std::max(d.lo, v));
    }
    // WTGPU_GRID_CLS=a,b,c,d (beside the table: four values): grids of the per-class kernels of WTGPU_SORTED_INTERACT=1 relative to the round's
    // (divisors, >= 1; diffuse, dielectric, spm, any).  Values the string does not give keep their defaults.
    unsigned v[4] = {1, 4, 2, 4};
    if (const char* e = getenv("WTGPU_GRID_CLS")) sscanf(e, "%u,%u,%u,%u", &v[0], &v[1], &v[2], &v[3]);
    for (int c = 0; c < 4; ++c) k.grid_div_cls[c] = std::max(1u, v[c]);
}
