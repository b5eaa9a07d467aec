// wave_tracer_amd — the environment knobs of the host driver: their values (knobs_t) and THE table that describes them (kKnobs: name, field,
// default, range, one line of help).  Every knob is read once per wtgpu_scene_upload, by read_knobs, and nowhere else.  Plain C++ (no HIP
// headers): the table can be compiled and checked without a GPU (tests/test_source_rules.py reads the names from wtgpu_knobs.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

struct knobs_t {
    uint32_t cone_budget, count_stats, split_queues, lane_cache, heavy_cache, heavy_probe, coop_aperture_min, flux_task_tris, profile, no_lists, primary_axis;
    uint32_t streams, state_gb, timing, conn_pool;
    uint32_t first_rounds, rounds_margin, light_rounds, max_rounds, stagger_round;
    uint32_t shrink_r1, shrink_f1, shrink_r2, shrink_f2, shrink_h1, decay_q, decay_c;
    uint32_t heavy_waves_per_cu, round_blocks_per_cu, grid_div_b, grid_div_c, grid_div_hard, grid_mul_flux;
    uint32_t sorted_interact, coop_io, staged_connect, connect_class, tiled_splat, pass_c_tiers, pass_c_easy_tries, pass_c_thin;
    uint32_t trace_staged, trace_stages, trace_staged_rounds, trace_sm, trace_ab;
    uint32_t develop_per_pixel, tonemap_lds_table, film_polar_staged, film_denoise_fused, film_denoise_guide_lds, first_hit_per_sample, los_per_sample, film_zonal_lds, film_zonal_blocks, film_segments_tiled, film_distance_groups;
    uint32_t dbg_stage;   // an int (WTGPU_DEBUG_STAGE may be negative), kept in 32 bits like the rest: read it as (int)dbg_stage
    uint32_t host_prof, trace_launch, tail_diag, trace_ab_verbose;
    uint32_t grid_div_cls[4];   // WTGPU_GRID_CLS, beside the table
};

enum knob_kind_t {
    KNOB_U32,       // strtoll, clamped to [0, 0xFFFFFFFF] (negative -> 0), then to [lo, hi]
    KNOB_INT,       // atoi, clamped to [lo, hi]
    KNOB_NONZERO,   // atoi(value) != 0
    KNOB_PRESENT    // 1 when the variable is in the environment, whatever its value
};
struct knob_t {
    const char* name;
    uint32_t knobs_t::*field;
    knob_kind_t kind;
    long long dflt, lo, hi;   // unset: dflt (it lies within [lo, hi])
    const char* help;
};
#pragma GCC visibility push(hidden)   // (internal to libwtgpu.so)
extern const knob_t kKnobs[];
extern const size_t kNumKnobs;
// defaults that are constants of wtgpu_kernels.h (HIP): written out in the table, asserted equal where both are visible (wtgpu_host.h)
constexpr uint32_t kKnobConeBudget = 96, kKnobFluxTaskTris = 2048;

void read_knobs(knobs_t& k);
#pragma GCC visibility pop
