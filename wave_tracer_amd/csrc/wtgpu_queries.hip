// wave_tracer_amd — entry points that are neither a render nor read a film (wtgpu_film.hip): ray / cone / region queries, by-geometry sensor
// masks, first-hit maps, first-hit material maps, line-of-sight maps, the probes of the kernel tests (wtgpu_test_hooks.h), the PMC calibration copy.
#include "wtgpu_host.h"
#include "wt/first_hit.h"
#include "wt/first_hit_material.h"
#include "wt/flux_probe.h"
#include "wt/los.h"
#include "wt/sources_probe.h"

// ---- what the entries of the sensor-element maps (mask, first hit, first-hit material, line of sight) share ----------------------------------
// One group of bits of a map spec with the caller's array for it (out_name NULL: flags, which select no output).
struct spec_group_t {
    uint32_t bits, known;
    const char* unknown;   // "map bits (1 COVERAGE .. 64 FACING)"
    const void* out;
    const char *requested, *out_name;   // "maps", "maps"
};
// The checks the specs share, in this order: no unknown bit in any group, something requested (none: "no map and no id bit"), and an array for
// every group that is.  who: the feature's name in the messages.
static int check_groups(const std::string& who, const char* none, std::initializer_list<spec_group_t> groups) {
    bool any = false;
    for (const spec_group_t& g : groups) {
        if (g.bits & ~g.known) return fail(WTGPU_ERR_INVALID, who + ": unknown " + g.unknown);
        any = any || (g.out_name && g.bits);
    }
    if (!any) return fail(WTGPU_ERR_INVALID, who + ": nothing requested (" + none + ")");
    for (const spec_group_t& g : groups)
        if (g.out_name && g.bits && !g.out) return fail(WTGPU_ERR_INVALID, who + ": " + g.requested + " requested, but the " + g.out_name + " pointer is NULL");
    return WTGPU_OK;
}
// The tail of a device entry: body() runs with the uploaded scene's device current; launch_rc() turns what a launcher returns into the entry's code.
template <class F>
static int on_scene_device(wtgpu_scene* s, F&& body) {
    if (!s->uploaded) return fail(WTGPU_ERR_INVALID, "scene not uploaded");
    device_guard_t guard(s->device);
    return body();
}
static int launch_rc(const char* kernel, int e) { return e ? fail(WTGPU_ERR_HIP, std::string(kernel) + ": " + hipGetErrorString((hipError_t)e)) : WTGPU_OK; }
// The tail of a host entry: the twin's exceptions (a thread that cannot start, an allocation) become the entry's code.
template <class F>
static int on_host(F&& twin) {
    try {
        twin();
    } catch (const std::exception& e) {
        return fail(WTGPU_ERR_INVALID, e.what());
    }
    return WTGPU_OK;
}

extern "C" {

int wtgpu_trace_rays(wtgpu_scene* s, void* stream_, const float* d_rays, uint32_t n, float* d_dist, uint32_t* d_tuid, float* d_bary, uint32_t* d_front) {
    if (!s || !s->uploaded) return fail(WTGPU_ERR_INVALID, "scene not uploaded");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    hipLaunchKernelGGL(k_trace_rays, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, s->dev, d_rays, n, d_dist, d_tuid, d_bary, d_front);
    HIP_CHECK(hipGetLastError());
    return WTGPU_OK;
}
int wtgpu_traverse_cones(wtgpu_scene* s, void* stream_, const float* d_cones, uint32_t n, uint32_t cap, float* d_dist, uint32_t* d_flags,
                         uint32_t* d_ntris, uint32_t* d_tris) {
    if (!s || !s->uploaded) return fail(WTGPU_ERR_INVALID, "scene not uploaded");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    // scratch for the bounded lists (ids + distances), kept with the scene between calls
    const size_t need = (size_t)n * kMaxConeTris * 4 * 2;
    if (need > s->query_scratch_bytes) {
        device_guard_t guard(s->device);
        void* p = nullptr;
        HIP_CHECK(hipMalloc(&p, need));
        s->dev_allocs.push_back(p);   // (the old block, if any, is released with the scene)
        s->query_scratch = static_cast<uint32_t*>(p);
        s->query_scratch_bytes = need;
    }
    hipLaunchKernelGGL(k_traverse_cones, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, s->dev, d_cones, n, cap, d_dist, d_flags, d_ntris,
                       d_tris, s->query_scratch);
    HIP_CHECK(hipGetLastError());
    return WTGPU_OK;
}

int wtgpu_query_regions(wtgpu_scene* s, void* stream_, const float* d_cones, uint32_t n, uint32_t edge_cap, float* d_dist, uint32_t* d_flags,
                        uint32_t* d_primary, uint32_t* d_ntris, uint32_t* d_nedges, uint32_t* d_edges, float* d_flux) {
    if (!s || !s->uploaded) return fail(WTGPU_ERR_INVALID, "scene not uploaded");
    if (n == 0) return WTGPU_OK;
    hipLaunchKernelGGL(k_query_regions, dim3(n), dim3(64), 0, static_cast<hipStream_t>(stream_), s->dev, d_cones, n, edge_cap, d_dist, d_flags, d_primary,
                       d_ntris, d_nedges, d_edges, d_flux, s->slices[0].counters + kDroppedSlot);
    HIP_CHECK(hipGetLastError());
    return WTGPU_OK;
}

// ---- sensor masks (include/wt/sensor/mask/mask.hpp, src/sensor/mask.cpp:28-108) ----------------------------------------------------------
int wtgpu_scene_shape_id(const wtgpu_scene* s, uint32_t shape, const char** id) {
    if (!s || !id) return fail(WTGPU_ERR_INVALID, "null argument");
    if (shape >= s->host.n_shapes) return fail(WTGPU_ERR_INVALID, "shape index out of range");
    *id = shape < s->file.shape_ids.size() ? s->file.shape_ids[shape].c_str() : "";
    return WTGPU_OK;
}
int wtgpu_scene_sensor_mask_spec(const wtgpu_scene* s, wtgpu_sensor_mask_spec* out) {
    if (!s || !out) return fail(WTGPU_ERR_INVALID, "null argument");
    out->present = s->file.has_mask ? 1 : 0;
    out->samples = s->file.mask_samples;
    out->regex = s->file.mask_regex.c_str();
    out->shape_flags = s->file.has_mask && !s->file.mask_flags.empty() ? s->file.mask_flags.data() : nullptr;
    out->n_shapes = s->host.n_shapes;
    return WTGPU_OK;
}
// the flags a mask call uses (NULL: the scene file's), after the checks both forms share
static int mask_flags_for(const wtgpu_scene* s, const uint8_t* shape_flags, uint32_t samples, const uint8_t** flags) {
    if (s->host.sensor.type != SENSOR_PERSPECTIVE)
        return fail(WTGPU_ERR_INVALID, "sensor masks need a perspective sensor (only the perspective loader reads a <sensor_mask>: src/sensor/perspective.cpp:98)");
    if (samples == 0 || samples > 65536) return fail(WTGPU_ERR_INVALID, "sensor mask: 1 .. 65536 samples per pixel expected");
    if (!shape_flags && !s->file.has_mask) return fail(WTGPU_ERR_INVALID, "the scene has no <sensor_mask>: pass one flag per shape");
    *flags = shape_flags ? shape_flags : s->file.mask_flags.data();
    return WTGPU_OK;
}
int wtgpu_sensor_mask(wtgpu_scene* s, void* stream_, const uint8_t* shape_flags, uint32_t samples, uint64_t seed, float* d_out) {
    if (!s || !d_out) return fail(WTGPU_ERR_INVALID, "null argument");
    const uint8_t* flags = nullptr;
    if (const int rc = mask_flags_for(s, shape_flags, samples, &flags)) return rc;
    return on_scene_device(s, [&]() -> int {
        hipStream_t stream = static_cast<hipStream_t>(stream_);
        const size_t n = std::max<size_t>(1, s->host.n_shapes);
        if (!s->ev_mask) {
            uint8_t* d = nullptr;
            if (const int rc = dmalloc(s, &d, n)) return rc;
            HIP_CHECK(hipHostMalloc((void**)&s->h_mask_flags, n, hipHostMallocDefault));
            HIP_CHECK(hipEventCreateWithFlags(&s->ev_mask, hipEventDisableTiming));
            s->d_mask_flags = d;
        } else
            HIP_CHECK(hipEventSynchronize(s->ev_mask));   // the previous call's kernel has read the buffers
        if (s->host.n_shapes) std::memcpy(s->h_mask_flags, flags, s->host.n_shapes);
        HIP_CHECK(hipMemcpyAsync(s->d_mask_flags, s->h_mask_flags, n, hipMemcpyHostToDevice, stream));
        if (const int rc = launch_rc("k_sensor_mask", sensor_mask_launch(s->dev, stream, s->d_mask_flags, samples, seed, d_out))) return rc;
        HIP_CHECK(hipEventRecord(s->ev_mask, stream));
        return WTGPU_OK;
    });
}
int wtgpu_sensor_mask_host(const wtgpu_scene* s, const uint8_t* shape_flags, uint32_t samples, uint64_t seed, uint32_t n_threads, float* out) {
    if (!s || !out) return fail(WTGPU_ERR_INVALID, "null argument");
    const uint8_t* flags = nullptr;
    if (const int rc = mask_flags_for(s, shape_flags, samples, &flags)) return rc;
    return on_host([&] { sensor_mask_host(s->host, flags, samples, seed, n_threads, out); });
}

// ---- first-hit maps (wt/first_hit.h, kernels_firsthit.hip) ---------------------------------------------------------------------------------
// the checks both forms share
static int first_hit_check(const wtgpu_scene* s, const wtgpu_first_hit_spec* spec, const float* maps, const uint32_t* ids) {
    if (!s || !spec) return fail(WTGPU_ERR_INVALID, "null argument");
    if (s->host.sensor.type != SENSOR_PERSPECTIVE)
        return fail(WTGPU_ERR_INVALID, "first-hit maps need a perspective sensor (a virtual-plane sensor has no primary ray through a pixel)");
    if (spec->samples > kFhMaxSamples) return fail(WTGPU_ERR_INVALID, "first-hit maps: 0 .. 4096 samples per pixel expected");
    return check_groups("first-hit maps", "no map and no id bit", {{spec->maps, FH_ALL_MAPS, "map bits (1 COVERAGE .. 64 FACING)", maps, "maps", "maps"},
                                                                  {spec->ids, FH_ALL_IDS, "id bits (1 SHAPE, 2 TRIANGLE)", ids, "ids", "ids"}});
}
int wtgpu_first_hit(wtgpu_scene* s, void* stream, const wtgpu_first_hit_spec* spec, float* d_maps, uint32_t* d_ids) {
    if (const int rc = first_hit_check(s, spec, d_maps, d_ids)) return rc;
    return on_scene_device(s, [&] {
        return launch_rc("k_first_hit", first_hit_launch(s->dev, static_cast<hipStream_t>(stream), spec->samples, spec->seed, spec->maps, spec->ids,
                                                        s->knobs.first_hit_per_sample, d_maps, d_ids));
    });
}
int wtgpu_first_hit_host(const wtgpu_scene* s, const wtgpu_first_hit_spec* spec, uint32_t n_threads, float* maps, uint32_t* ids) {
    if (const int rc = first_hit_check(s, spec, maps, ids)) return rc;
    return on_host([&] { first_hit_host(s->host, spec->samples, spec->seed, spec->maps, spec->ids, n_threads, maps, ids); });
}

// ---- first-hit material maps (wt/first_hit_material.h, kernels_firsthit_material.hip) ------------------------------------------------------
// the checks both forms share, and the query the kernels and the host twin take
static int first_hit_material_check(const wtgpu_scene* s, const wtgpu_first_hit_material_spec* spec, const float* maps, const uint32_t* ids, fhm_query_t& q) {
    if (!s || !spec) return fail(WTGPU_ERR_INVALID, "null argument");
    if (s->host.sensor.type != SENSOR_PERSPECTIVE)
        return fail(WTGPU_ERR_INVALID, "first-hit material maps need a perspective sensor (a virtual-plane sensor has no primary ray through a pixel)");
    if (spec->n_k < 1 || spec->n_k > kFhmMaxK) return fail(WTGPU_ERR_INVALID, "first-hit material maps: 1 .. 4 wavenumbers expected (n_k)");
    for (uint32_t j = 0; j < spec->n_k; ++j)
        if (!finitef(spec->k[j]) || !(spec->k[j] > 0.f))
            return fail(WTGPU_ERR_INVALID, "first-hit material maps: wavenumber " + std::to_string(j) + " is not finite and > 0 (k in 1/mm)");
    if (spec->samples > kFhMaxSamples) return fail(WTGPU_ERR_INVALID, "first-hit material maps: 0 .. 4096 samples per pixel expected");
    if (const int rc = check_groups("first-hit material maps", "no map and no id bit",
                                    {{spec->maps, FHM_ALL_MAPS, "map bits (1 ALBEDO .. 16 EMISSION)", maps, "maps", "maps"},
                                     {spec->ids, FHM_ALL_IDS, "id bits (1 MATERIAL, 2 TYPE)", ids, "ids", "ids"}}))
        return rc;
    q.samples = spec->samples, q.maps = spec->maps, q.ids = spec->ids, q.n_k = spec->n_k, q.seed = spec->seed;
    for (uint32_t j = 0; j < kFhmMaxK; ++j) q.k[j] = j < spec->n_k ? spec->k[j] : 0.f;
    return WTGPU_OK;
}
int wtgpu_first_hit_material(wtgpu_scene* s, void* stream, const wtgpu_first_hit_material_spec* spec, float* d_maps, uint32_t* d_ids) {
    fhm_query_t q;
    if (const int rc = first_hit_material_check(s, spec, d_maps, d_ids, q)) return rc;
    return on_scene_device(s, [&] {
        return launch_rc("k_first_hit_material", first_hit_material_launch(s->dev, static_cast<hipStream_t>(stream), q, s->knobs.first_hit_per_sample, d_maps, d_ids));
    });
}
int wtgpu_first_hit_material_host(const wtgpu_scene* s, const wtgpu_first_hit_material_spec* spec, uint32_t n_threads, float* maps, uint32_t* ids) {
    fhm_query_t q;
    if (const int rc = first_hit_material_check(s, spec, maps, ids, q)) return rc;
    return on_host([&] { first_hit_material_host(s->host, q, n_threads, maps, ids); });
}
// One wavenumber per spectral channel of the sensor: the line of a discrete response, the response-weighted mean over the knots of a table.
int wtgpu_scene_channel_wavenumbers(const wtgpu_scene* s, float k[4]) {
    if (!s || !k) return fail(WTGPU_ERR_INVALID, "null argument");
    const scene_t& sc = s->host;
    for (uint32_t c = 0; c < 4; ++c) k[c] = 0.f;
    for (uint32_t c = 0; c < sc.sensor.channels && c < 4; ++c) {
        const int id = sc.sensor.response_spec[c];
        const std::string ch = "channel wavenumbers: channel " + std::to_string(c);
        if (id < 0 || (uint32_t)id >= sc.n_spectra) return fail(WTGPU_ERR_INVALID, ch + " has no response spectrum");
        const spectrum_t sp = sc.spectra[id];
        if (sp.type == SPEC_DISCRETE) {
            k[c] = sp.kmin;
            continue;
        }
        if (sp.type != SPEC_TABLE) return fail(WTGPU_ERR_INVALID, ch + " has a constant response: it singles out no wavenumber");
        double num = 0., den = 0.;
        for (uint32_t i = 0; i < sp.count; ++i) {
            const double ki = sp.count > 1 ? (double)sp.kmin + ((double)sp.kmax - (double)sp.kmin) * (double)i / (double)(sp.count - 1) : (double)sp.kmin;
            const double R = sc.spectra_data[sp.offset + i];
            num += ki * R, den += R;
        }
        if (!(den > 0.)) return fail(WTGPU_ERR_INVALID, ch + " has an all-zero response: it singles out no wavenumber");
        k[c] = (float)(num / den);
    }
    return WTGPU_OK;
}

// ---- line-of-sight maps (wt/los.h, kernels_los.hip) ------------------------------------------------------------------------------------------
// the checks both forms share, and the query the kernels and the host twin take
static int los_check(const wtgpu_scene* s, const wtgpu_los_spec* spec, const float* points, const float* normals, const float* mask, const float* maps,
                     const float* elem, const uint32_t* ids, los_query_t& q) {
    if (!s || !spec) return fail(WTGPU_ERR_INVALID, "null argument");
    const scene_t& sc = s->host;
    if (!points && sc.sensor.type != SENSOR_VIRTUAL_PLANE)
        return fail(WTGPU_ERR_INVALID, "line of sight: without points the elements of a virtual-plane sensor are meant, and this sensor is not one (pass points, for example the POSITION map of wtgpu_first_hit)");
    if (points && spec->samples != 0) return fail(WTGPU_ERR_INVALID, "line of sight: caller points take samples = 0 (a point is not sampled)");
    if (spec->samples > kLosMaxSamples) return fail(WTGPU_ERR_INVALID, "line of sight: 0 .. 4096 samples per element expected");
    if (const int rc = check_groups("line of sight", "no map, no element and no id bit",
                                    {{spec->maps, LOS_ALL_MAPS, "map bits (1 VISIBLE, 2 DISTANCE, 4 DIRECTION, 8 COS)", maps, "maps", "maps"},
                                     {spec->elem, LOS_ALL_ELEM, "element bits (1 POINT, 2 NEAREST_DISTANCE)", elem, "element floats", "elem"},
                                     {spec->ids, LOS_ALL_IDS, "id bits (1 N_VISIBLE, 2 NEAREST)", ids, "ids", "ids"},
                                     {spec->flags, LOS_ALL_FLAGS, "flag bits (1 FRONT_ONLY)", nullptr, nullptr, nullptr}}))
        return rc;
    const bool has_normal = !points || normals;
    if ((spec->maps & LOS_COS) && !has_normal) return fail(WTGPU_ERR_INVALID, "line of sight: COS needs a normal (caller points without normals)");
    if ((spec->flags & LOS_FRONT_ONLY) && !has_normal) return fail(WTGPU_ERR_INVALID, "line of sight: FRONT_ONLY needs a normal (caller points without normals)");
    if (!(spec->t_min >= 0.f) || !finitef(spec->t_min)) return fail(WTGPU_ERR_INVALID, "line of sight: t_min must be finite and >= 0");
    if (spec->n_emitters > kLosMaxEmitters) return fail(WTGPU_ERR_INVALID, "line of sight: at most 32 emitters per call");
    q.samples = spec->samples, q.maps = spec->maps, q.elem = spec->elem, q.ids = spec->ids, q.flags = spec->flags;
    q.t_min = spec->t_min, q.seed = spec->seed;
    q.points = points, q.normals = points ? normals : nullptr, q.mask = mask;
    q.n_emitters = 0;
    for (uint32_t i = 0; i < kLosMaxEmitters; ++i) q.emitters[i] = 0;
    if (spec->n_emitters == 0) {
        for (uint32_t i = 0; i < sc.n_emitters; ++i) {
            if (sc.emitters[i].type == EMIT_AREA) continue;
            if (q.n_emitters == kLosMaxEmitters) return fail(WTGPU_ERR_INVALID, "line of sight: the scene has more than 32 emitters that are not area emitters: select at most 32 per call");
            q.emitters[q.n_emitters++] = i;
        }
        if (!q.n_emitters) return fail(WTGPU_ERR_INVALID, "line of sight: empty selection (the scene has no point, spot or directional emitter)");
    } else
        for (uint32_t k = 0; k < spec->n_emitters; ++k) {
            const uint32_t i = spec->emitters[k];
            if (i >= sc.n_emitters) return fail(WTGPU_ERR_INVALID, "line of sight: emitter index " + std::to_string(i) + " out of range (the scene has " + std::to_string(sc.n_emitters) + ")");
            if (sc.emitters[i].type == EMIT_AREA) return fail(WTGPU_ERR_INVALID, "line of sight: emitter " + std::to_string(i) + " is an area emitter (point, spot and directional emitters only)");
            for (uint32_t j = 0; j < k; ++j)
                if (spec->emitters[j] == i) return fail(WTGPU_ERR_INVALID, "line of sight: emitter " + std::to_string(i) + " is selected twice");
            q.emitters[q.n_emitters++] = i;
        }
    return WTGPU_OK;
}
int wtgpu_line_of_sight(wtgpu_scene* s, void* stream, const wtgpu_los_spec* spec, const float* d_points, const float* d_normals, const float* d_mask,
                        float* d_maps, float* d_elem, uint32_t* d_ids) {
    los_query_t q;
    if (const int rc = los_check(s, spec, d_points, d_normals, d_mask, d_maps, d_elem, d_ids, q)) return rc;
    return on_scene_device(s, [&] { return launch_rc("k_los", los_launch(s->dev, static_cast<hipStream_t>(stream), q, s->knobs.los_per_sample, d_maps, d_elem, d_ids)); });
}
int wtgpu_line_of_sight_host(const wtgpu_scene* s, const wtgpu_los_spec* spec, const float* points, const float* normals, const float* mask,
                             uint32_t n_threads, float* maps, float* elem, uint32_t* ids) {
    los_query_t q;
    if (const int rc = los_check(s, spec, points, normals, mask, maps, elem, ids, q)) return rc;
    return on_host([&] { los_host(s->host, q, n_threads, maps, elem, ids); });
}

int wtgpu_test_fsd_apertures(wtgpu_scene* s, void* stream, const float* d_cones, const float* d_sk, const uint32_t* d_ids, const uint32_t* d_n_ids,
                             uint32_t n, uint32_t id_cap, uint32_t pool_cap, uint32_t mode, uint32_t* d_hdr, float* d_segs) {
    if (!s || !s->uploaded) return fail(WTGPU_ERR_INVALID, "scene not uploaded");
    if (mode > 1 || id_cap == 0 || pool_cap == 0) return fail(WTGPU_ERR_INVALID, "wtgpu_test_fsd_apertures: mode 0 / 1, id_cap and pool_cap > 0");
    HIP_CHECK((hipError_t)test_fsd_apertures(s->dev, static_cast<hipStream_t>(stream), d_cones, d_sk, d_ids, d_n_ids, n, id_cap, pool_cap, mode, d_hdr, d_segs));
    return WTGPU_OK;
}
int wtgpu_test_utd_sums(wtgpu_scene* s, void* stream, const float* d_queries, const uint32_t* d_ids, const uint32_t* d_n_ids, uint32_t n, uint32_t id_cap,
                        uint32_t utd_cap, uint32_t* d_recs, uint32_t* d_hdr, uint32_t* d_edges) {
    if (!s || !s->uploaded) return fail(WTGPU_ERR_INVALID, "scene not uploaded");
    if (id_cap == 0 || utd_cap == 0) return fail(WTGPU_ERR_INVALID, "wtgpu_test_utd_sums: id_cap and utd_cap > 0");
    HIP_CHECK((hipError_t)test_utd_sums(s->dev, static_cast<hipStream_t>(stream), d_queries, d_ids, d_n_ids, n, id_cap, utd_cap, d_recs, d_hdr, d_edges));
    return WTGPU_OK;
}

int wtgpu_test_bsdf_queries(wtgpu_scene* s, void* stream, const uint32_t* d_queries, uint32_t n, int form, uint32_t* d_out) {
    if (!s || !s->uploaded) return fail(WTGPU_ERR_INVALID, "scene not uploaded");
    if (form < -1 || form > (int)MAT_SURFACE_SPM) return fail(WTGPU_ERR_INVALID, "wtgpu_test_bsdf_queries: form -1, 0, 1 or 2");
    HIP_CHECK((hipError_t)test_bsdf_queries(s->dev, static_cast<hipStream_t>(stream), d_queries, n, form, d_out));
    return WTGPU_OK;
}

int wtgpu_test_source_queries(wtgpu_scene* s, void* stream_, const uint32_t* d_queries, uint32_t n, uint32_t* d_out) {
    if (!s || !s->uploaded) return fail(WTGPU_ERR_INVALID, "scene not uploaded");
    if (n == 0) return WTGPU_OK;
    if (!d_queries || !d_out) return fail(WTGPU_ERR_INVALID, "null argument");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    device_guard_t guard(s->device);
    std::vector<uint32_t> q((size_t)n * kSourceProbeQueryWords);
    HIP_CHECK(hipMemcpyAsync(q.data(), d_queries, q.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    for (uint32_t i = 0; i < n; ++i)
        if (!source_probe_query_ok(s->host, q.data() + (size_t)i * kSourceProbeQueryWords))
            return fail(WTGPU_ERR_INVALID, "wtgpu_test_source_queries: query " + std::to_string(i) + ": op, emitter index or tuid out of range");
    HIP_CHECK((hipError_t)test_source_queries(s->dev, stream, d_queries, n, d_out));
    return WTGPU_OK;
}

int wtgpu_test_flux_queries(wtgpu_scene* s, void* stream_, const uint32_t* d_queries, uint32_t n, uint32_t* d_out) {
    if (!s || !s->uploaded) return fail(WTGPU_ERR_INVALID, "scene not uploaded");
    if (n == 0) return WTGPU_OK;
    if (!d_queries || !d_out) return fail(WTGPU_ERR_INVALID, "null argument");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    device_guard_t guard(s->device);
    std::vector<uint32_t> q((size_t)n * kFluxProbeQueryWords);
    HIP_CHECK(hipMemcpyAsync(q.data(), d_queries, q.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    for (uint32_t i = 0; i < n; ++i)
        if (!flux_probe_query_ok(s->host, q.data() + (size_t)i * kFluxProbeQueryWords))
            return fail(WTGPU_ERR_INVALID, "wtgpu_test_flux_queries: query " + std::to_string(i) + ": op or tuid out of range");
    HIP_CHECK((hipError_t)test_flux_queries(s->dev, stream, d_queries, n, d_out));
    return WTGPU_OK;
}

int wtgpu_test_connect_class_order(uint32_t* keys, uint32_t cap, uint32_t* n_keys, uint32_t* key_dim) {
    if (!n_keys || !key_dim) return fail(WTGPU_ERR_INVALID, "wtgpu_test_connect_class_order: null argument");
    *n_keys = kNumKeys;
    *key_dim = kKeyDim;
    if (!keys || cap < kNumKeys) return WTGPU_OK;   // (the sizes only)
    for (uint32_t r = 0; r < kNumKeys; ++r) keys[r] = 0xFFFFFFFFu;
    for (uint32_t k = 0; k < kNumKeys; ++k) {
        const uint32_t r = class_key_rank(k);
        if (r < kNumKeys) keys[r] = k;
    }
    return WTGPU_OK;
}

int wtgpu_test_connect_class_items(wtgpu_scene* s, uint32_t slice, uint32_t* table, uint32_t* items, uint32_t items_cap, uint32_t* n_items) {
    if (!s || !s->uploaded || !table || !items || !n_items || slice >= s->slices.size()) return fail(WTGPU_ERR_INVALID, "wtgpu_test_connect_class_items: uploaded scene, a slice of it");
    if (s->host.opts.integrator != INTEGRATOR_BDPT) return fail(WTGPU_ERR_INVALID, "wtgpu_test_connect_class_items: plt_bdpt scenes");
    device_guard_t guard(s->device);
    {
        const int rc = drain_all(s);
        if (rc) return rc;
    }
    HIP_CHECK(hipDeviceSynchronize());
    const device_state_t& st = s->slices[slice];
    HIP_CHECK(hipMemcpy(table, st.strat_prefix, kClassTableWords * sizeof(uint32_t), hipMemcpyDeviceToHost));
    uint64_t n = 0;
    for (uint32_t r = 0; r < kNumKeys; ++r) {
        const uint32_t c = table[kClassCount + r], key = table[kClassKey + r];
        if (key >= kNumKeys || c > st.cap || n + c > items_cap) return fail(WTGPU_ERR_INVALID, "wtgpu_test_connect_class_items: not a class table (was the batch connected by k_connect_class?) or items_cap too small");
        if (c) HIP_CHECK(hipMemcpy(items + n, st.strat_items + (size_t)key * st.cap, c * sizeof(uint32_t), hipMemcpyDeviceToHost));
        n += c;
    }
    *n_items = (uint32_t)n;
    return WTGPU_OK;
}

int wtgpu_calibrate_copy(uint64_t n_dwords, int repeats) {
    uint32_t *in = nullptr, *out = nullptr;
    HIP_CHECK(hipMalloc((void**)&in, n_dwords * 4));
    HIP_CHECK(hipMalloc((void**)&out, n_dwords * 4));
    HIP_CHECK(hipMemset(in, 1, n_dwords * 4));
    for (int r = 0; r < repeats; ++r) hipLaunchKernelGGL(k_calib_copy, dim3(256 * 32), dim3(256), 0, 0, in, out, (size_t)n_dwords);
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipFree(in));
    HIP_CHECK(hipFree(out));
    return WTGPU_OK;
}

}   // extern "C"
