// wave_tracer_amd — entry points that are not a render: ray / cone / region queries, by-geometry sensor masks, the probes of the kernel tests
// (wtgpu_test_hooks.h), the PMC calibration copy, develop and tonemap, film statistics.
#include "wtgpu_host.h"
#include "wt/sources_probe.h"
#include "wt/tonemap.h"
#include "wt/film_stats.h"
#include "wt/film_compare.h"

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
    if (!s->uploaded) return fail(WTGPU_ERR_INVALID, "scene not uploaded");
    device_guard_t guard(s->device);
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
    const int e = sensor_mask_launch(s->dev, stream, s->d_mask_flags, samples, seed, d_out);
    if (e) return fail(WTGPU_ERR_HIP, std::string("k_sensor_mask: ") + hipGetErrorString((hipError_t)e));
    HIP_CHECK(hipEventRecord(s->ev_mask, stream));
    return WTGPU_OK;
}
int wtgpu_sensor_mask_host(const wtgpu_scene* s, const uint8_t* shape_flags, uint32_t samples, uint64_t seed, uint32_t n_threads, float* out) {
    if (!s || !out) return fail(WTGPU_ERR_INVALID, "null argument");
    const uint8_t* flags = nullptr;
    if (const int rc = mask_flags_for(s, shape_flags, samples, &flags)) return rc;
    try {
        sensor_mask_host(s->host, flags, samples, seed, n_threads, out);
    } catch (const std::exception& e) {
        return fail(WTGPU_ERR_INVALID, e.what());
    }
    return WTGPU_OK;
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

int wtgpu_develop(const wtgpu_scene* s, const double* value, const double* weight, const double* light, uint64_t spe, float* out) {
    if (!s || !value || !weight || !light || !out) return fail(WTGPU_ERR_INVALID, "null argument");
    const sensor_t& sn = s->host.sensor;
    const double sl = develop_scale(spe);
    for (size_t p = 0; p < (size_t)sn.width * sn.height; ++p)
        for (uint32_t c = 0, P = film_planes(sn); c < P; ++c) out[p * P + c] = develop_plane(value[p * P + c], weight[p], light[p * P + c], sl);
    return WTGPU_OK;
}

// ---- development and tonemapping where the films are (kernels_develop.hip; wt/tonemap.h) ---------------------------------------------------
int wtgpu_scene_tonemap_spec(const wtgpu_scene* s, wtgpu_tonemap_spec* out) {
    if (!s || !out) return fail(WTGPU_ERR_INVALID, "null argument");
    const wth::scene_file_extras_t& f = s->file;
    const bool rgb = s->host.sensor.channels == 3;
    out->present = f.has_tonemap ? 1 : 0;
    // absent: sRGB / normal for an RGB response (RGB.cpp:91-93: create_sRGB), linear / select for a monochromatic one (monochromatic.cpp:65-66)
    out->op = f.has_tonemap ? f.tonemap_op : rgb ? TM_SRGB : TM_LINEAR;
    out->mode = f.has_tonemap ? f.tonemap_mode : rgb ? TM_NORMAL : TM_SELECT;
    out->gamma = f.tonemap_gamma;
    out->db_min = f.tonemap_db_min;
    out->db_max = f.tonemap_db_max;
    out->colourmap = f.tonemap_colourmap.c_str();
    out->function = f.tonemap_function.c_str();
    return WTGPU_OK;
}

// the polynomial fit of the Turbo map imageio.colourmap evaluates, and the identity: the two maps the library can tabulate itself
static void builtin_table(bool turbo, std::vector<float>& tab) {
    const uint32_t n = 256;
    tab.resize(3 * n);
    static const double c4[3][4] = {{.13572138, 4.61539260, -42.66032258, 132.13108234}, {.09140261, 2.19418839, 4.84296658, -14.18503333}, {.10667330, 12.64194608, -60.58204836, 110.36276771}};
    static const double c2[3][2] = {{-152.94239396, 59.28637943}, {4.27729857, 2.82956604}, {-89.90310912, 27.34824973}};
    for (uint32_t i = 0; i < n; ++i) {
        const double v = double(i) / double(n - 1), v2 = v * v, v3 = v2 * v;
        for (int k = 0; k < 3; ++k) {
            const double x = c4[k][0] + c4[k][1] * v + c4[k][2] * v2 + c4[k][3] * v3 + c2[k][0] * (v2 * v2) + c2[k][1] * (v3 * v2);
            tab[3 * i + k] = turbo ? (float)std::min(1.0, std::max(0.0, x)) : (float)v;
        }
    }
}
static bool same_name(const std::string& a, const char* b) {
    if (a.size() != std::strlen(b)) return false;
    for (size_t i = 0; i < a.size(); ++i)
        if (std::tolower((unsigned char)a[i]) != b[i]) return false;
    return true;
}
// The operator a tonemap call uses after the checks both forms share: `tm` (NULL: the scene's own spec, whose map must be one the library can
// tabulate), the Stokes component, the format.  args.table points at the caller's table or into `own` (host memory), or is null when the mode
// sends nothing through a map.
static int tonemap_args_for(const wtgpu_scene* s, const wtgpu_tonemap* tm, uint32_t stokes_component, uint32_t format, tonemap_args_t& args, std::vector<float>& own) {
    const sensor_t& sn = s->host.sensor;
    if (sn.channels != 1 && sn.channels != 3) return fail(WTGPU_ERR_INVALID, "tonemap: a film of 1 or 3 channels expected");
    if (stokes_component >= film_stokes(sn))
        return fail(WTGPU_ERR_INVALID, "tonemap: stokes_component " + std::to_string(stokes_component) + " out of range (the film has " + std::to_string(film_stokes(sn)) + ")");
    if (format > TM_U16) return fail(WTGPU_ERR_INVALID, "tonemap: format 0 (f32), 1 (u8) or 2 (u16) expected");
    wtgpu_tonemap_spec spec{};
    (void)wtgpu_scene_tonemap_spec(s, &spec);
    const int32_t op = tm ? tm->op : spec.op, mode = tm ? tm->mode : spec.mode;
    const float gamma = tm ? tm->gamma : spec.gamma, db_min = tm ? tm->db_min : spec.db_min, db_max = tm ? tm->db_max : spec.db_max;
    if (op == TM_FUNCTION) return fail(WTGPU_ERR_INVALID, "tonemap: the 'function' operator is not supported (the expression is read from the scene file, not evaluated)");
    if (op < TM_LINEAR || op > TM_FUNCTION) return fail(WTGPU_ERR_INVALID, "tonemap: operator 0 (linear), 1 (gamma), 2 (sRGB) or 3 (dB) expected");
    if (mode < TM_SELECT || mode > TM_COLOURMAP) return fail(WTGPU_ERR_INVALID, "tonemap: mode 0 (select), 1 (normal) or 2 (colourmap) expected");
    if (op == TM_GAMMA && !(gamma > 0.f)) return fail(WTGPU_ERR_INVALID, "(tonemap operator loader) 'gamma' must be positive");
    if (op == TM_DB && !(db_max - db_min > 0.f)) return fail(WTGPU_ERR_INVALID, "(tonemap operator loader) expected valid 'db' range to be provided");
    args.op = op;
    args.mode = mode;
    args.inv_gamma = 1.f / gamma;
    args.db_min = db_min;
    args.db_len = db_max - db_min;
    args.table = nullptr;
    args.table_n = 0;
    if (!tm_uses_map(mode, sn.channels)) return WTGPU_OK;
    if (tm && tm->table) {
        if (tm->table_n < 2 || tm->table_n > kMaxTonemapTable) return fail(WTGPU_ERR_INVALID, "tonemap: a colour table of 2 .. " + std::to_string(kMaxTonemapTable) + " RGB entries expected");
        args.table = tm->table;
        args.table_n = tm->table_n;
        return WTGPU_OK;
    }
    if (tm) return fail(WTGPU_ERR_INVALID, "tonemap: this mode maps the film through a colour table: pass one");
    const bool turbo = same_name(s->file.tonemap_colourmap, "turbo");
    if (!turbo && !same_name(s->file.tonemap_colourmap, "grey"))
        return fail(WTGPU_ERR_INVALID, "tonemap: the scene's colour map \"" + s->file.tonemap_colourmap + "\" is not one the library tabulates (grey, turbo): pass a table");
    builtin_table(turbo, own);
    args.table = own.data();
    args.table_n = (uint32_t)(own.size() / 3);
    return WTGPU_OK;
}

int wtgpu_develop_device(wtgpu_scene* s, void* stream_, const double* d_value, const double* d_weight, const double* d_light, uint64_t spe, float* d_out) {
    if (!s || !d_value || !d_weight || !d_light || !d_out) return fail(WTGPU_ERR_INVALID, "null argument");
    if (!s->uploaded) return fail(WTGPU_ERR_INVALID, "scene not uploaded");
    device_guard_t guard(s->device);
    const int e = develop_launch(s->host.sensor, static_cast<hipStream_t>(stream_), d_value, d_weight, d_light, spe, s->knobs.develop_per_pixel, d_out);
    if (e) return fail(WTGPU_ERR_HIP, std::string("k_develop: ") + hipGetErrorString((hipError_t)e));
    return WTGPU_OK;
}
int wtgpu_tonemap_device(wtgpu_scene* s, void* stream_, const double* d_value, const double* d_weight, const double* d_light, uint64_t spe, const wtgpu_tonemap* tm,
                         uint32_t stokes_component, const float* d_mask, uint32_t format, void* d_out) {
    if (!s || !d_value || !d_weight || !d_light || !d_out) return fail(WTGPU_ERR_INVALID, "null argument");
    tonemap_args_t args{};
    std::vector<float> own;
    if (const int rc = tonemap_args_for(s, tm, stokes_component, format, args, own)) return rc;
    if (!s->uploaded) return fail(WTGPU_ERR_INVALID, "scene not uploaded");
    if ((uintptr_t)d_out % 16) return fail(WTGPU_ERR_INVALID, "tonemap: d_out must be aligned to 16 bytes");
    device_guard_t guard(s->device);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (args.table) {   // the table goes to the device behind everything already on `stream`, through a pinned copy made before the call returns
        const size_t bytes = (size_t)kMaxTonemapTable * 3 * sizeof(float);
        if (!s->ev_tm) {
            float* d = nullptr;
            if (const int rc = dmalloc(s, &d, (size_t)kMaxTonemapTable * 3)) return rc;
            HIP_CHECK(hipHostMalloc((void**)&s->h_tm_table, bytes, hipHostMallocDefault));
            HIP_CHECK(hipEventCreateWithFlags(&s->ev_tm, hipEventDisableTiming));
            s->d_tm_table = d;
        } else
            HIP_CHECK(hipEventSynchronize(s->ev_tm));   // the previous call's kernel has read the buffers
        std::memcpy(s->h_tm_table, args.table, (size_t)args.table_n * 3 * sizeof(float));
        HIP_CHECK(hipMemcpyAsync(s->d_tm_table, s->h_tm_table, (size_t)args.table_n * 3 * sizeof(float), hipMemcpyHostToDevice, stream));
        args.table = s->d_tm_table;
    }
    const int e = develop_tonemap_launch(s->host.sensor, stream, d_value, d_weight, d_light, spe, args, stokes_component, d_mask, format, s->knobs.tonemap_lds_table, d_out);
    if (e) return fail(WTGPU_ERR_HIP, std::string("k_develop_tonemap: ") + hipGetErrorString((hipError_t)e));
    if (args.table) HIP_CHECK(hipEventRecord(s->ev_tm, stream));
    return WTGPU_OK;
}
int wtgpu_tonemap_host(const wtgpu_scene* s, const double* value, const double* weight, const double* light, uint64_t spe, const wtgpu_tonemap* tm,
                       uint32_t stokes_component, const float* mask, uint32_t format, uint32_t n_threads, void* out) {
    if (!s || !value || !weight || !light || !out) return fail(WTGPU_ERR_INVALID, "null argument");
    tonemap_args_t args{};
    std::vector<float> own;
    if (const int rc = tonemap_args_for(s, tm, stokes_component, format, args, own)) return rc;
    try {
        develop_tonemap_host(s->host.sensor, value, weight, light, spe, args, stokes_component, mask, format, n_threads, out);
    } catch (const std::exception& e) {
        return fail(WTGPU_ERR_INVALID, e.what());
    }
    return WTGPU_OK;
}

// ---- film statistics (kernels_stats.hip; wt/film_stats.h) -----------------------------------------------------------------------------------
static_assert(sizeof(wtgpu_film_stats) == sizeof(film_stats_rec_t), "the kernels' record is wtgpu_film_stats");
// what a spec says by itself, and its edge table
static int film_stats_edges_for(const wtgpu_film_stats_spec* spec, float* edges) {
    if (spec->scale > FS_DB) return fail(WTGPU_ERR_INVALID, "film_stats: scale 0 (linear) or 1 (dB) expected");
    if (spec->flags & ~(FS_ABS | FS_LUMINANCE)) return fail(WTGPU_ERR_INVALID, "film_stats: flags 1 (ABS) and 2 (LUMINANCE) expected");
    if (spec->bins > kFsMaxBins) return fail(WTGPU_ERR_INVALID, "film_stats: bins " + std::to_string(spec->bins) + " above the " + std::to_string(kFsMaxBins) + " the histogram holds");
    if (!std::isfinite(spec->lo) || (spec->bins > 0 && !std::isfinite(spec->hi))) return fail(WTGPU_ERR_INVALID, "film_stats: a finite range expected");
    if (spec->bins > 0 && !(spec->lo < spec->hi)) return fail(WTGPU_ERR_INVALID, "film_stats: lo < hi expected with bins > 0");
    for (uint32_t i = 0; i <= spec->bins; ++i) {
        edges[i] = fs_edge(spec->scale, spec->lo, spec->hi, spec->bins, i);
        if (!std::isfinite(edges[i]) || (i > 0 && !(edges[i - 1] < edges[i])))
            return fail(WTGPU_ERR_INVALID, "film_stats: degenerate edges: edge " + std::to_string(i) + " of " + std::to_string(spec->bins) + " is not above edge " +
                                               std::to_string(i ? i - 1 : 0) + " after rounding to f32 (fewer bins or a wider range)");
    }
    return WTGPU_OK;
}
// ... and against the scene's film; planes: records per call
static int film_stats_check(const wtgpu_scene* s, const wtgpu_film_stats_spec* spec, uint32_t& planes) {
    const sensor_t& sn = s->host.sensor;
    if (sn.channels != 1 && sn.channels != 3) return fail(WTGPU_ERR_INVALID, "film_stats: a film of 1 or 3 channels expected");
    if (spec->stokes_component >= film_stokes(sn))
        return fail(WTGPU_ERR_INVALID, "film_stats: stokes_component " + std::to_string(spec->stokes_component) + " out of range (the film has " + std::to_string(film_stokes(sn)) + ")");
    if ((spec->flags & FS_LUMINANCE) && sn.channels != 3) return fail(WTGPU_ERR_INVALID, "film_stats: LUMINANCE needs a 3-channel film (this one has " + std::to_string(sn.channels) + ")");
    planes = sn.channels + ((spec->flags & FS_LUMINANCE) ? 1u : 0u);
    return WTGPU_OK;
}
int wtgpu_film_stats_edges(const wtgpu_film_stats_spec* spec, float* edges) {
    if (!spec || !edges) return fail(WTGPU_ERR_INVALID, "null argument");
    if (spec->bins > kFsMaxBins) return film_stats_edges_for(spec, nullptr);   // (refused before anything is written)
    return film_stats_edges_for(spec, edges);
}

// the scene's scratch block: records, histogram, edge table — on the device and, pinned, on the host
constexpr size_t kFsRecBytes = kFsMaxPlanes * sizeof(film_stats_rec_t), kFsHistBytes = (size_t)kFsMaxPlanes * kFsMaxBins * sizeof(uint64_t);
constexpr size_t kFsEdgeOffset = kFsRecBytes + kFsHistBytes, kFsBlockBytes = kFsEdgeOffset + (kFsMaxBins + 1) * sizeof(float);

int wtgpu_film_stats_device(wtgpu_scene* s, void* stream_, const double* d_value, const double* d_weight, const double* d_light, uint64_t spe,
                            const wtgpu_film_stats_spec* spec, const float* d_mask, wtgpu_film_stats* out, uint64_t* hist) {
    if (!s || !d_value || !d_weight || !d_light || !spec || !out || (!hist && spec->bins > 0)) return fail(WTGPU_ERR_INVALID, "null argument");
    uint32_t planes = 0;
    float edges[kFsMaxBins + 1];
    if (const int rc = film_stats_edges_for(spec, edges)) return rc;
    if (const int rc = film_stats_check(s, spec, planes)) return rc;
    if (!s->uploaded) return fail(WTGPU_ERR_INVALID, "scene not uploaded");
    const sensor_t& sn = s->host.sensor;
    const uint64_t npix = (uint64_t)sn.width * sn.height;
    if (npix == 0) return fail(WTGPU_ERR_INVALID, "film_stats: the film has no pixels");
    device_guard_t guard(s->device);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!s->d_fs) {   // first use: the block, its pinned copy, the chunk sums of this scene's film (all levels, kFsMaxPlanes planes)
        unsigned char* d = nullptr;
        double* sums = nullptr;
        if (const int rc = dmalloc(s, &d, kFsBlockBytes)) return rc;
        if (const int rc = dmalloc(s, &sums, (size_t)kFsMaxPlanes * fs_scratch_len(npix))) return rc;
        HIP_CHECK(hipHostMalloc((void**)&s->h_fs, kFsBlockBytes, hipHostMallocDefault));
        int n_cu = 256;
        (void)hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, s->device);
        s->fs_cus = (uint32_t)std::max(1, n_cu);
        s->d_fs_sums = sums;
        s->d_fs = d;
    }
    // The call waits for its own result below, so the block is free again when it returns.
    const size_t result_bytes = kFsRecBytes + (size_t)planes * spec->bins * sizeof(uint64_t), edge_bytes = (spec->bins + 1) * sizeof(float);
    std::memcpy(s->h_fs + kFsEdgeOffset, edges, edge_bytes);
    HIP_CHECK(hipMemcpyAsync(s->d_fs + kFsEdgeOffset, s->h_fs + kFsEdgeOffset, edge_bytes, hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipMemsetAsync(s->d_fs, 0, result_bytes, stream));
    const int e = film_stats_launch(sn, stream, s->fs_cus, d_value, d_weight, d_light, spe, spec->stokes_component, spec->flags, d_mask,
                                    reinterpret_cast<const float*>(s->d_fs + kFsEdgeOffset), spec->bins, s->d_fs, reinterpret_cast<unsigned long long*>(s->d_fs + kFsRecBytes),
                                    s->d_fs_sums);
    if (e) return fail(WTGPU_ERR_HIP, std::string("k_film_stats: ") + hipGetErrorString((hipError_t)e));
    HIP_CHECK(hipMemcpyAsync(s->h_fs, s->d_fs, result_bytes, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    std::memcpy(out, s->h_fs, planes * sizeof(wtgpu_film_stats));
    if (spec->bins) std::memcpy(hist, s->h_fs + kFsRecBytes, (size_t)planes * spec->bins * sizeof(uint64_t));
    return WTGPU_OK;
}
int wtgpu_film_stats_host(const wtgpu_scene* s, const double* value, const double* weight, const double* light, uint64_t spe, const wtgpu_film_stats_spec* spec,
                          const float* mask, uint32_t n_threads, wtgpu_film_stats* out, uint64_t* hist) {
    if (!s || !value || !weight || !light || !spec || !out || (!hist && spec->bins > 0)) return fail(WTGPU_ERR_INVALID, "null argument");
    uint32_t planes = 0;
    float edges[kFsMaxBins + 1];
    if (const int rc = film_stats_edges_for(spec, edges)) return rc;
    if (const int rc = film_stats_check(s, spec, planes)) return rc;
    try {
        film_stats_host(s->host.sensor, value, weight, light, spe, spec->stokes_component, spec->flags, mask, edges, spec->bins, n_threads, out,
                        reinterpret_cast<unsigned long long*>(hist));
    } catch (const std::exception& e) {
        return fail(WTGPU_ERR_INVALID, e.what());
    }
    return WTGPU_OK;
}


// ---- film comparison (kernels_compare.hip; wt/film_compare.h) -------------------------------------------------------------------------------
static_assert(sizeof(wtgpu_film_compare) == sizeof(film_compare_rec_t), "the kernels' record is wtgpu_film_compare");
// what a spec says by itself and against the scene's film; planes: records per call
static int film_compare_check(const wtgpu_scene* s, const wtgpu_film_compare_spec* spec, uint32_t& planes) {
    const sensor_t& sn = s->host.sensor;
    if (spec->flags & ~(FC_ABS | FC_LUMINANCE)) return fail(WTGPU_ERR_INVALID, "film_compare: flags 1 (ABS) and 2 (LUMINANCE) expected");
    if (!std::isfinite(spec->eps) || !(spec->eps > 0.0)) return fail(WTGPU_ERR_INVALID, "film_compare: a finite eps > 0 expected");
    if (sn.channels != 1 && sn.channels != 3) return fail(WTGPU_ERR_INVALID, "film_compare: a film of 1 or 3 channels expected");
    if (spec->stokes_component >= film_stokes(sn))
        return fail(WTGPU_ERR_INVALID, "film_compare: stokes_component " + std::to_string(spec->stokes_component) + " out of range (the film has " + std::to_string(film_stokes(sn)) + ")");
    if ((spec->flags & FC_LUMINANCE) && sn.channels != 3) return fail(WTGPU_ERR_INVALID, "film_compare: LUMINANCE needs a 3-channel film (this one has " + std::to_string(sn.channels) + ")");
    planes = sn.channels + ((spec->flags & FC_LUMINANCE) ? 1u : 0u);
    return WTGPU_OK;
}
constexpr size_t kFcRecBytes = kFsMaxPlanes * sizeof(film_compare_rec_t);

int wtgpu_film_compare_device(wtgpu_scene* s, void* stream_, const double* a_value, const double* a_weight, const double* a_light, uint64_t spe_a, const double* b_value,
                              const double* b_weight, const double* b_light, uint64_t spe_b, const wtgpu_film_compare_spec* spec, const float* d_mask,
                              wtgpu_film_compare* out, float* d_diff) {
    if (!s || !a_value || !a_weight || !a_light || !b_value || !b_weight || !b_light || !spec || !out) return fail(WTGPU_ERR_INVALID, "null argument");
    uint32_t planes = 0;
    if (const int rc = film_compare_check(s, spec, planes)) return rc;
    if (!s->uploaded) return fail(WTGPU_ERR_INVALID, "scene not uploaded");
    const sensor_t& sn = s->host.sensor;
    const uint64_t npix = (uint64_t)sn.width * sn.height;
    if (npix == 0) return fail(WTGPU_ERR_INVALID, "film_compare: the film has no pixels");
    device_guard_t guard(s->device);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!s->d_fc) {   // first use: the records, their pinned copy, the chunk sums (all levels, kFsMaxPlanes planes of kFcSums sums) and the wavefronts' records
        unsigned char *d = nullptr, *wave = nullptr;
        double* sums = nullptr;
        int n_cu = 256;
        (void)hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, s->device);
        const uint32_t cus = (uint32_t)std::max(1, n_cu);
        if (const int rc = dmalloc(s, &d, kFcRecBytes)) return rc;
        if (const int rc = dmalloc(s, &sums, (size_t)kFsMaxPlanes * kFcSums * fs_scratch_len(npix))) return rc;
        if (const int rc = dmalloc(s, &wave, film_compare_wave_bytes(npix, cus))) return rc;
        HIP_CHECK(hipHostMalloc((void**)&s->h_fc, kFcRecBytes, hipHostMallocDefault));
        s->fc_cus = cus;
        s->d_fc_sums = sums;
        s->d_fc_wave = wave;
        s->d_fc = d;
    }
    // The call waits for its own result below, so the block is free again when it returns.
    const int e = film_compare_launch(sn, stream, s->fc_cus, a_value, a_weight, a_light, spe_a, b_value, b_weight, b_light, spe_b, spec->stokes_component, spec->flags, spec->eps,
                                      d_mask, s->d_fc, s->d_fc_sums, s->d_fc_wave, d_diff);
    if (e) return fail(WTGPU_ERR_HIP, std::string("k_film_compare: ") + hipGetErrorString((hipError_t)e));
    HIP_CHECK(hipMemcpyAsync(s->h_fc, s->d_fc, planes * sizeof(film_compare_rec_t), hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    std::memcpy(out, s->h_fc, planes * sizeof(wtgpu_film_compare));
    return WTGPU_OK;
}
int wtgpu_film_compare_host(const wtgpu_scene* s, const double* a_value, const double* a_weight, const double* a_light, uint64_t spe_a, const double* b_value,
                            const double* b_weight, const double* b_light, uint64_t spe_b, const wtgpu_film_compare_spec* spec, const float* mask, uint32_t n_threads,
                            wtgpu_film_compare* out, float* diff) {
    if (!s || !a_value || !a_weight || !a_light || !b_value || !b_weight || !b_light || !spec || !out) return fail(WTGPU_ERR_INVALID, "null argument");
    uint32_t planes = 0;
    if (const int rc = film_compare_check(s, spec, planes)) return rc;
    try {
        film_compare_host(s->host.sensor, a_value, a_weight, a_light, spe_a, b_value, b_weight, b_light, spe_b, spec->stokes_component, spec->flags, spec->eps, mask, n_threads,
                          out, diff);
    } catch (const std::exception& e) {
        return fail(WTGPU_ERR_INVALID, e.what());
    }
    return WTGPU_OK;
}

}   // extern "C"
