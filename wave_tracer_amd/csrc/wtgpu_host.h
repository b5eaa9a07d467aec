// wave_tracer_amd — what the units of the host driver share: the scene object behind the C-ABI's handle, the record of a batch in flight, error
// reporting and the few functions one unit needs of another.  The units (Makefile: HOST_TUS; wtgpu_unity.hip includes them all):
//   wtgpu.hip            the batch driver: wtgpu_render*, wtgpu_join, timings
//   wtgpu_scene.hip      scene creation (named / xml / description), comparison, info, destruction — host memory only
//   wtgpu_upload.hip     wtgpu_scene_upload: scene arrays, batch sizing, one slice's allocations; release_device
//   wtgpu_knobs.hip      the environment knobs: one table, read_knobs (wtgpu_knobs.h; plain C++)
//   wtgpu_trace_ab.hip   WTGPU_TRACE_AB replay harness, the alternative forms of the per-lane traversal
//   wtgpu_counters.hip   wtgpu_get_counters and its profile printers, reset
//   wtgpu_queries.hip    ray / cone / region queries, sensor masks, the test probes
//   wtgpu_film.hip       what reads films: develop and tonemap, film statistics, film comparison, the polarisation view, the denoiser
//   wtgpu_control.hip    cancel / pause / resume / capture / progressive render; the RCCL film reduction
#pragma once
#include <hip/hip_runtime.h>
#include <chrono>

#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <memory>
#include <mutex>
#include <thread>
#include <string>
#include <vector>

#include "wtgpu_kernels.h"
#include "wtgpu_test_hooks.h"
#include "wtgpu_knobs.h"
#include "host/scene_builder.h"

static_assert(kKnobConeBudget == kConeBudget && kKnobFluxTaskTris == kFluxTaskTris, "wtgpu_knobs.h repeats two defaults of wtgpu_kernels.h");

#pragma GCC visibility push(hidden)   // (what one unit needs of another stays internal to libwtgpu.so)
extern thread_local std::string g_err;   // wtgpu.hip: what wtgpu_last_error returns
inline int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
#define HIP_CHECK(x)                                                                                         \
    do {                                                                                                     \
        hipError_t e_ = (x);                                                                                 \
        if (e_ != hipSuccess) return fail(WTGPU_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_));    \
    } while (0)

struct chunk_rec_t {
    std::vector<hipEvent_t> ev;   // [0] start, [1] after generate, then 6 per LAUNCHED round, last used: after connect
    uint32_t* h_ctl = nullptr;    // pinned snapshot of the slice's control block after the batch
    uint32_t* h_mid = nullptr;    // ... and after the rounds launched up front (wtgpu_render_async, then every finish_look): is the queue empty?
    hipEvent_t ev_mid = nullptr;
    hipEvent_t ev_stagger = nullptr;   // recorded after the batch's round `stagger_round`: the next batch (on the next stream) starts there
    uint32_t rounds_launched = 0;
    uint32_t rounds_timed = 0;   // ... of which bracketed by timing events (6 per round, in launch order)
    size_t ev_used = 0;           // timing events recorded so far (the next one closes the batch)
    size_t ev_final = 0;          // index of the event recorded after the batch's last kernel
    bool busy = false;
};

// What a film feature (wtgpu_film.hip) keeps with the scene from its first call on: its results on the device (the statistics: records, histogram
// and edge table; the comparison and the polarisation view: records, then the wavefronts' records), their head pinned on the host, and the chunk sums of every level of the
// fixed summation order (wt/film_stats.h: fs_scratch_len).
struct film_scratch_t {
    unsigned char* d_block = nullptr;
    unsigned char* h_block = nullptr;
    double* d_sums = nullptr;
};

struct wtgpu_scene {
    std::unique_ptr<wth::scene_builder_t> builder;   // owns the host arrays (named scenes)
    scene_t host{};                                  // host-pointer scene
    scene_t dev{};                                   // device-pointer scene
    std::vector<void*> dev_allocs;
    int device = -1;
    uint32_t n_cus = 0;   // compute units of the device, read at upload: what the persistent grids and the film kernels' grids are sized by
    bool uploaded = false;
    std::vector<device_state_t> slices;              // per-batch path state, one slice per internal stream
    std::vector<const path_state_t*> d_path_slices;  // ... and its plt_path part (device copies)
    const unsigned char* d_tri_class = nullptr;       // walk class of every triangle (bdpt_ext_t::tri_class)
    uint32_t pend_cap = 0, n_chunks = 0;              // staged connections: items per chunk, chunks per batch (bdpt_ext_t)
    std::vector<hipStream_t> streams;
    std::vector<hipEvent_t> ev_done;
    hipEvent_t ev_begin = nullptr;
    hipEvent_t ev_stagger_last = nullptr;   // the previous batch's stagger event (owned by its record)
    std::vector<chunk_rec_t> recs;                   // in-flight batch records (events + control block snapshot)
    size_t rec_next = 0;
    size_t slice_next = 0;   // batches go round-robin over the slices ACROSS render calls (a call with one batch does not always land on stream 0)
    // A batch is enqueued in two parts (wtgpu_render_async / finish_look): generation + the rounds its walks are EXPECTED to need, and —
    // once the host has seen that the round queue is empty (or has launched the remaining rounds) — the connections.  Between the two it is
    // `pending` on its slice; the next batch of that slice, wtgpu_join and everything that reads results finish it first.
    struct pending_t {
        bool active = false;
        unsigned char args[1024];   // the batch's launch block (launch_args_t, defined below)
        chunk_rec_t* rec = nullptr;
        uint32_t launched = 0, rounds_step = 8;   // rounds enqueued so far; rounds to add at the next look (finish_look)
    };
    std::vector<pending_t> pending;   // per slice
    uint32_t rounds_hist[8] = {0};    // rounds with work of the last batches seen (the expectation is their mean + WTGPU_ROUNDS_MARGIN: expected_rounds)
    uint32_t rounds_hist_n = 0;
    uint64_t round_fallbacks = 0;     // looks that found the round queue still filled (the batch got more rounds, 8 at first, then 16, 32, 64: finish_look)
    uint64_t rounds_launched_total = 0;
    std::string stats;
    double lut_power[2] = {0, 0};
    double acc[12] = {0};                             // accumulated timings since the last reset (see wtgpu_last_render_timings)
    uint64_t samples_rendered = 0;
    uint64_t cap_hits = 0;
    std::atomic<int> cancel{0};
    std::atomic<int> paused{0};
    std::mutex capture_mutex;
    wtgpu_capture_cb capture_cb = nullptr;   // pending `capture intermediate` (under capture_mutex)
    void* capture_user = nullptr;
    uint32_t* query_scratch = nullptr;   // wtgpu_traverse_cones
    size_t query_scratch_bytes = 0;
    wth::scene_file_extras_t file;       // shape ids and the sensor mask of a scene file: host state only, not part of the flattened scene
    uint8_t* d_mask_flags = nullptr;     // wtgpu_sensor_mask: the shape flags of the last call on the device, and their pinned staging copy;
    uint8_t* h_mask_flags = nullptr;     // both are reused once ev_mask (recorded behind that call's kernel) has passed
    hipEvent_t ev_mask = nullptr;
    float* d_tm_table = nullptr;         // wtgpu_tonemap_device: the colour table of the last call (kMaxTonemapTable entries), staged the same way
    float* h_tm_table = nullptr;
    hipEvent_t ev_tm = nullptr;
    film_scratch_t fs, fc, fp;           // wtgpu_film_stats_device, wtgpu_film_compare_device, wtgpu_film_polar_device
    // wtgpu_film_zonal_device: records, edge table, histogram, n_outside and the accumulating slots on the device, all but the slots pinned on the host;
    // sized by the call and grown when a later call needs more
    unsigned char* d_zonal = nullptr;
    unsigned char* h_zonal = nullptr;
    size_t d_zonal_bytes = 0, h_zonal_bytes = 0;
    uint32_t zonal_last_lds = 0xFFFFFFFFu;   // the form the last wtgpu_film_zonal_device call took: 1 LDS, 0 global (wtgpu_test_film_zonal_form)
    // wtgpu_film_segments_device: the head (counts, overflow word) and the records on the device and pinned on the host, the union-find's arrays on the
    // device; sized by the call and grown when a later call needs more
    unsigned char* d_segments = nullptr;
    unsigned char* h_segments = nullptr;
    size_t d_segments_bytes = 0, h_segments_bytes = 0;
    uint32_t segments_last_overflow = 0xFFFFFFFFu;   // the overflow word of the last wtgpu_film_segments_device call (wtgpu_test_film_segments_form)
    uint32_t segments_last_tiled = 0xFFFFFFFFu;      // the form that call took: 1 tiled, 0 global
    // wtgpu_film_distance_device: the head (site count, key of the maximum) on the device and pinned on the host, the column offsets and the groups'
    // minima on the device; sized by the call and grown when a later call needs more
    unsigned char* d_distance = nullptr;
    unsigned char* h_distance = nullptr;
    size_t d_distance_bytes = 0;
    uint32_t distance_last_groups = 0xFFFFFFFFu;     // the form the last wtgpu_film_distance_device call took: 1 with the group level, 0 without (wtgpu_test_film_distance_form)
    float* d_denoise = nullptr;          // wtgpu_film_denoise_device: the developed half-films, their variance and what one direction leaves for the other
    // WTGPU_TRACE_AB (diagnostic, tests/test_gpu_traversal.py): accumulated over the replayed rounds — milliseconds of k_trace_refill / k_trace_sm on the
    // same queue, words of their outputs that differ (traversal records + triangle lists + heavy-queue checksums), walks replayed
    double ab_ms[2] = {0, 0};
    uint64_t ab_mismatch = 0, ab_walks = 0, ab_rounds = 0;
    uint64_t light_rounds_run = 0;   // rounds k_light_rounds ran (diagnostic)
    using knobs_t = ::knobs_t;   // environment knobs, read ONCE per upload: wtgpu_knobs.h has the table
    knobs_t knobs{};
};

// restores the calling thread's current device when an entry point returns
struct device_guard_t {
    int prev = -1;
    explicit device_guard_t(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
        else prev = -1;
    }
    ~device_guard_t() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

template <class T>
int upload(wtgpu_scene* s, const T* src, size_t n, const T** dst) {
    *dst = nullptr;
    if (n == 0 || !src) return WTGPU_OK;
    void* p = nullptr;
    HIP_CHECK(hipMalloc(&p, n * sizeof(T)));
    s->dev_allocs.push_back(p);
    HIP_CHECK(hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice));
    *dst = static_cast<const T*>(p);
    return WTGPU_OK;
}
template <class T>
int dmalloc(wtgpu_scene* s, T** p, size_t n) {
    void* q = nullptr;
    hipError_t e = hipMalloc(&q, n * sizeof(T));
    if (e != hipSuccess) return fail(WTGPU_ERR_OOM, std::string("hipMalloc of ") + std::to_string(n * sizeof(T)) + " bytes: " + hipGetErrorString(e));
    s->dev_allocs.push_back(q);
    *p = static_cast<T*>(q);
    return WTGPU_OK;
}


// the variable-length arrays of a flattened scene: how far the records of the scene reach into them (wtgpu_scene.hip)
struct scene_extents_t {
    size_t spec_words = 0;          // spectra_data
    size_t tex_words = 0;           // texture_data: bitmaps, function tables and the sampling tables of textured area emitters
    size_t shape_tris = 0;          // shape_tri_tuid (shape_tri_cdf: + n_shapes)
    size_t kd_words = 0;            // kdist_data as wtgpu_scene_upload sees it: the n_emitters records of kdists, discrete ones skipped
    size_t cmp_kdists = 0, cmp_kd_words = 0;   // kdists / kdist_data as wtgpu_scene_compare sees them: max(emitter.k_dist) + 1 records, none skipped
};
// ---- what one unit needs of another
scene_extents_t scene_extents(const scene_t& sc);
void release_device(wtgpu_scene* s);   // wtgpu_upload.hip
void film_scratch_free(film_scratch_t& f);   // wtgpu_film.hip
int drain_all(wtgpu_scene* s);         // wtgpu.hip: finishes the pending batches, waits for every batch in flight
// wtgpu_trace_ab.hip
void launch_trace_alt(const wtgpu_scene* s, const launch_args_t& a, hipStream_t st_, int in, int first, uint32_t round, uint32_t g0);
int trace_ab_round(wtgpu_scene* s, const launch_args_t& a, hipStream_t st_, int in, int first, uint32_t round, uint32_t g0);
#pragma GCC visibility pop
