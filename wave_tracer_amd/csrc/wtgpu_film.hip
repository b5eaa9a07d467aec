// wave_tracer_amd — the entry points that read films: develop, the tonemap spec / device / host calls (kernels_develop.hip), film statistics
// (kernels_stats.hip), zonal film statistics (kernels_zonal.hip), connected segments of a label plane (kernels_segments.hip), its distance transform (kernels_distance.hip), film comparison (kernels_compare.hip), the polarisation view (kernels_polar.hip) and the denoiser of two half-films (kernels_denoise.hip); what they check of a film
// and keep with the scene between calls.  The four passes that read a film take a wtgpu_film_source — the accumulators or a developed f32 film — and
// the accumulator-taking entry points are those calls with an accumulator source.
#include <cstddef>

#include "wtgpu_host.h"
#include "wt/tonemap.h"
#include "wt/film_stats.h"
#include "wt/film_zonal.h"
#include "wt/film_segments.h"
#include "wt/film_distance.h"
#include "wt/film_compare.h"
#include "wt/film_polar.h"
#include "wt/film_denoise.h"

// The film a call reads, the Stokes component and the FS_* flags it asks for -> planes: the planes per call (channels, + 1 with FS_LUMINANCE).
// `what` opens the message.
static int film_planes_for(const wtgpu_scene* s, const char* what, uint32_t stokes_component, uint32_t flags, uint32_t& planes) {
    const sensor_t& sn = s->host.sensor;
    const std::string w = std::string(what) + ": ";
    if (sn.channels != 1 && sn.channels != 3) return fail(WTGPU_ERR_INVALID, w + "a film of 1 or 3 channels expected");
    if (stokes_component >= film_stokes(sn))
        return fail(WTGPU_ERR_INVALID, w + "stokes_component " + std::to_string(stokes_component) + " out of range (the film has " + std::to_string(film_stokes(sn)) + ")");
    if ((flags & FS_LUMINANCE) && sn.channels != 3) return fail(WTGPU_ERR_INVALID, w + "LUMINANCE needs a 3-channel film (this one has " + std::to_string(sn.channels) + ")");
    planes = sn.channels + ((flags & FS_LUMINANCE) ? 1u : 0u);
    return WTGPU_OK;
}

// A film source (wtgpu_film_source) is exactly one of its two forms.  `what` opens the message, `which` names the operand where there are two.
static int film_source_check(const char* what, const char* which, const wtgpu_film_source* f) {
    const std::string w = std::string(what) + ": " + which;
    const int n_acc = (f->value ? 1 : 0) + (f->weight ? 1 : 0) + (f->light ? 1 : 0);
    if (f->developed && n_acc) return fail(WTGPU_ERR_INVALID, w + "film source: both forms are set (the accumulators value / weight / light, or a developed film: one of them)");
    if (!f->developed && n_acc == 0) return fail(WTGPU_ERR_INVALID, w + "film source: neither form is set (the accumulators value / weight / light, or a developed film)");
    if (n_acc != 0 && n_acc != 3) return fail(WTGPU_ERR_INVALID, w + "film source: the accumulators are value, weight and light together (" + std::to_string(n_acc) + " of the 3 set)");
    return WTGPU_OK;
}
// the source an accumulator-taking entry point stands for
static wtgpu_film_source accumulators(const double* value, const double* weight, const double* light, uint64_t spe) {
    return wtgpu_film_source{value, weight, light, spe, nullptr};
}

// A feature's scratch is allocated at its first call: d_bytes on the device, the first h_bytes of them pinned on the host, n_sums chunk sums.
static int film_scratch_alloc(wtgpu_scene* s, film_scratch_t& f, size_t d_bytes, size_t h_bytes, size_t n_sums) {
    if (f.d_block) return WTGPU_OK;
    unsigned char* d = nullptr;
    double* sums = nullptr;
    if (const int rc = dmalloc(s, &d, d_bytes)) return rc;
    if (const int rc = dmalloc(s, &sums, n_sums)) return rc;
    HIP_CHECK(hipHostMalloc((void**)&f.h_block, h_bytes, hipHostMallocDefault));
    f.d_sums = sums;
    f.d_block = d;
    return WTGPU_OK;
}
void film_scratch_free(film_scratch_t& f) {   // (the device's parts are freed with dev_allocs)
    if (f.h_block) (void)hipHostFree(f.h_block);
    f = film_scratch_t{};
}

// What the device entry of a film pass does after its own spec checks: the two refusals all of them share, then body(stream, npix) with the
// scene's device current.  `what` opens the message.
template <class F>
static int film_on_device(wtgpu_scene* s, void* stream_, const char* what, F&& body) {
    if (!s->uploaded) return fail(WTGPU_ERR_INVALID, "scene not uploaded");
    const uint64_t npix = (uint64_t)s->host.sensor.width * s->host.sensor.height;
    if (npix == 0) return fail(WTGPU_ERR_INVALID, std::string(what) + ": the film has no pixels");
    device_guard_t guard(s->device);
    return body(static_cast<hipStream_t>(stream_), npix);
}
// The records at the head of a feature's block — rec_bytes of them, and whatever else the first block_bytes hold — come back through the pinned
// copy.  The call waits for its own result, so the block is free again when it returns.
static int film_records_back(film_scratch_t& f, hipStream_t stream, void* out, size_t rec_bytes, size_t block_bytes = 0) {
    HIP_CHECK(hipMemcpyAsync(f.h_block, f.d_block, std::max(rec_bytes, block_bytes), hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    std::memcpy(out, f.h_block, rec_bytes);
    return WTGPU_OK;
}
// The scratch of a records pass of K sums (compare, polar), allocated at first use: the records with the wavefronts' records behind them, the
// pinned copy of the former, the chunk sums (all levels, kFsMaxPlanes planes of K sums).
template <uint32_t K>
constexpr size_t kFilmRecBytes = kFsMaxPlanes * sizeof(film_best_rec_t<K>);
template <uint32_t K>
static int film_rec_scratch(wtgpu_scene* s, film_scratch_t& f, uint64_t npix) {
    static_assert(kFilmRecBytes<K> % 32 == 0, "the wavefronts' records (32 bytes each) follow the records in one block");
    return film_scratch_alloc(s, f, kFilmRecBytes<K> + film_rec_wave_bytes(npix, s->n_cus), kFilmRecBytes<K>, (size_t)kFsMaxPlanes * K * fs_scratch_len(npix));
}
// a host twin's call: what it throws (an allocation) is the call's error
template <class F>
static int film_on_host(F&& twin) {
    try {
        twin();
    } catch (const std::exception& e) {
        return fail(WTGPU_ERR_INVALID, e.what());
    }
    return WTGPU_OK;
}

extern "C" {

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
// What an operator's choice and numbers say by themselves (the tonemap calls' and the polarisation picture's).  `what` opens the messages about
// the choice, `loader` those worded as the reference's operator loader words them.
static int tonemap_op_check(int32_t op, int32_t mode, float gamma, float db_min, float db_max, const std::string& what, const std::string& loader) {
    if (op == TM_FUNCTION) return fail(WTGPU_ERR_INVALID, what + "the 'function' operator is not supported (the expression is read from the scene file, not evaluated)");
    if (op < TM_LINEAR || op > TM_FUNCTION) return fail(WTGPU_ERR_INVALID, what + "operator 0 (linear), 1 (gamma), 2 (sRGB) or 3 (dB) expected");
    if (mode < TM_SELECT || mode > TM_COLOURMAP) return fail(WTGPU_ERR_INVALID, what + "mode 0 (select), 1 (normal) or 2 (colourmap) expected");
    if (op == TM_GAMMA && !(gamma > 0.f)) return fail(WTGPU_ERR_INVALID, loader + "'gamma' must be positive");
    if (op == TM_DB && !(db_max - db_min > 0.f)) return fail(WTGPU_ERR_INVALID, loader + "expected valid 'db' range to be provided");
    return WTGPU_OK;
}
// The operator a tonemap call uses after the checks both forms share: `tm` (NULL: the scene's own spec, whose map must be one the library can
// tabulate), the Stokes component, the format.  args.table points at the caller's table or into `own` (host memory), or is null when the mode
// sends nothing through a map.
static int tonemap_args_for(const wtgpu_scene* s, const wtgpu_tonemap* tm, uint32_t stokes_component, uint32_t format, tonemap_args_t& args, std::vector<float>& own) {
    const sensor_t& sn = s->host.sensor;
    uint32_t planes = 0;
    if (const int rc = film_planes_for(s, "tonemap", stokes_component, 0u, planes)) return rc;
    if (format > TM_U16) return fail(WTGPU_ERR_INVALID, "tonemap: format 0 (f32), 1 (u8) or 2 (u16) expected");
    wtgpu_tonemap_spec spec{};
    (void)wtgpu_scene_tonemap_spec(s, &spec);
    const int32_t op = tm ? tm->op : spec.op, mode = tm ? tm->mode : spec.mode;
    const float gamma = tm ? tm->gamma : spec.gamma, db_min = tm ? tm->db_min : spec.db_min, db_max = tm ? tm->db_max : spec.db_max;
    if (const int rc = tonemap_op_check(op, mode, gamma, db_min, db_max, "tonemap: ", "(tonemap operator loader) ")) return rc;
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
int wtgpu_tonemap_source_device(wtgpu_scene* s, void* stream_, const wtgpu_film_source* film, const wtgpu_tonemap* tm, uint32_t stokes_component, const float* d_mask,
                                uint32_t format, void* d_out) {
    if (!s || !film || !d_out) return fail(WTGPU_ERR_INVALID, "null argument");
    if (const int rc = film_source_check("tonemap", "", film)) return rc;
    tonemap_args_t args{};
    std::vector<float> own;
    if (const int rc = tonemap_args_for(s, tm, stokes_component, format, args, own)) return rc;
    // (a scene that is not uploaded is refused first, as it always was: film_on_device says so)
    if (s->uploaded && (uintptr_t)d_out % 16) return fail(WTGPU_ERR_INVALID, "tonemap: d_out must be aligned to 16 bytes");
    return film_on_device(s, stream_, "tonemap", [&](hipStream_t stream, uint64_t) -> int {
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
        const int e = develop_tonemap_launch(s->host.sensor, stream, *film, args, stokes_component, d_mask, format, s->knobs.tonemap_lds_table, d_out);
        if (e) return fail(WTGPU_ERR_HIP, std::string("k_develop_tonemap: ") + hipGetErrorString((hipError_t)e));
        if (args.table) HIP_CHECK(hipEventRecord(s->ev_tm, stream));
        return WTGPU_OK;
    });
}
int wtgpu_tonemap_source_host(const wtgpu_scene* s, const wtgpu_film_source* film, const wtgpu_tonemap* tm, uint32_t stokes_component, const float* mask, uint32_t format,
                              uint32_t n_threads, void* out) {
    if (!s || !film || !out) return fail(WTGPU_ERR_INVALID, "null argument");
    if (const int rc = film_source_check("tonemap", "", film)) return rc;
    tonemap_args_t args{};
    std::vector<float> own;
    if (const int rc = tonemap_args_for(s, tm, stokes_component, format, args, own)) return rc;
    return film_on_host([&] { develop_tonemap_host(s->host.sensor, *film, args, stokes_component, mask, format, n_threads, out); });
}
// the accumulators' entry points: the same calls with an accumulator source
int wtgpu_tonemap_device(wtgpu_scene* s, void* stream_, const double* d_value, const double* d_weight, const double* d_light, uint64_t spe, const wtgpu_tonemap* tm,
                         uint32_t stokes_component, const float* d_mask, uint32_t format, void* d_out) {
    if (!s || !d_value || !d_weight || !d_light || !d_out) return fail(WTGPU_ERR_INVALID, "null argument");
    const wtgpu_film_source film = accumulators(d_value, d_weight, d_light, spe);
    return wtgpu_tonemap_source_device(s, stream_, &film, tm, stokes_component, d_mask, format, d_out);
}
int wtgpu_tonemap_host(const wtgpu_scene* s, const double* value, const double* weight, const double* light, uint64_t spe, const wtgpu_tonemap* tm,
                       uint32_t stokes_component, const float* mask, uint32_t format, uint32_t n_threads, void* out) {
    if (!s || !value || !weight || !light || !out) return fail(WTGPU_ERR_INVALID, "null argument");
    const wtgpu_film_source film = accumulators(value, weight, light, spe);
    return wtgpu_tonemap_source_host(s, &film, tm, stokes_component, mask, format, n_threads, out);
}

// ---- film statistics (kernels_stats.hip; wt/film_stats.h) -----------------------------------------------------------------------------------
static_assert(sizeof(wtgpu_film_stats) == sizeof(film_stats_rec_t), "the kernels' record is wtgpu_film_stats");
// what a spec says by itself, and its edge table
static int film_stats_edges_for(const wtgpu_film_stats_spec* spec, float* edges, const std::string& what = "film_stats") {
    if (spec->scale > FS_DB) return fail(WTGPU_ERR_INVALID, what + ": scale 0 (linear) or 1 (dB) expected");
    if (spec->flags & ~(FS_ABS | FS_LUMINANCE)) return fail(WTGPU_ERR_INVALID, what + ": flags 1 (ABS) and 2 (LUMINANCE) expected");
    if (spec->bins > kFsMaxBins) return fail(WTGPU_ERR_INVALID, what + ": bins " + std::to_string(spec->bins) + " above the " + std::to_string(kFsMaxBins) + " the histogram holds");
    if (!std::isfinite(spec->lo) || (spec->bins > 0 && !std::isfinite(spec->hi))) return fail(WTGPU_ERR_INVALID, what + ": a finite range expected");
    if (spec->bins > 0 && !(spec->lo < spec->hi)) return fail(WTGPU_ERR_INVALID, what + ": lo < hi expected with bins > 0");
    for (uint32_t i = 0; i <= spec->bins; ++i) {
        edges[i] = fs_edge(spec->scale, spec->lo, spec->hi, spec->bins, i);
        if (!std::isfinite(edges[i]) || (i > 0 && !(edges[i - 1] < edges[i])))
            return fail(WTGPU_ERR_INVALID, what + ": degenerate edges: edge " + std::to_string(i) + " of " + std::to_string(spec->bins) + " is not above edge " +
                                               std::to_string(i ? i - 1 : 0) + " after rounding to f32 (fewer bins or a wider range)");
    }
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

int wtgpu_film_stats_source_device(wtgpu_scene* s, void* stream_, const wtgpu_film_source* film, const wtgpu_film_stats_spec* spec, const float* d_mask, wtgpu_film_stats* out,
                                   uint64_t* hist) {
    if (!s || !film || !spec || !out || (!hist && spec->bins > 0)) return fail(WTGPU_ERR_INVALID, "null argument");
    if (const int rc = film_source_check("film_stats", "", film)) return rc;
    uint32_t planes = 0;
    float edges[kFsMaxBins + 1];
    if (const int rc = film_stats_edges_for(spec, edges)) return rc;
    if (const int rc = film_planes_for(s, "film_stats", spec->stokes_component, spec->flags, planes)) return rc;
    return film_on_device(s, stream_, "film_stats", [&](hipStream_t stream, uint64_t npix) -> int {
        // first use: the block, its pinned copy, the chunk sums of this scene's film (all levels, kFsMaxPlanes planes)
        film_scratch_t& f = s->fs;
        if (const int rc = film_scratch_alloc(s, f, kFsBlockBytes, kFsBlockBytes, (size_t)kFsMaxPlanes * fs_scratch_len(npix))) return rc;
        const size_t hist_bytes = (size_t)planes * spec->bins * sizeof(uint64_t), edge_bytes = (spec->bins + 1) * sizeof(float);
        std::memcpy(f.h_block + kFsEdgeOffset, edges, edge_bytes);
        HIP_CHECK(hipMemcpyAsync(f.d_block + kFsEdgeOffset, f.h_block + kFsEdgeOffset, edge_bytes, hipMemcpyHostToDevice, stream));
        HIP_CHECK(hipMemsetAsync(f.d_block, 0, kFsRecBytes + hist_bytes, stream));
        const int e = film_stats_launch(s->host.sensor, stream, s->n_cus, *film, spec->stokes_component, spec->flags, d_mask,
                                        reinterpret_cast<const float*>(f.d_block + kFsEdgeOffset), spec->bins, f.d_block,
                                        reinterpret_cast<unsigned long long*>(f.d_block + kFsRecBytes), f.d_sums);
        if (e) return fail(WTGPU_ERR_HIP, std::string("k_film_stats: ") + hipGetErrorString((hipError_t)e));
        if (const int rc = film_records_back(f, stream, out, planes * sizeof(wtgpu_film_stats), kFsRecBytes + hist_bytes)) return rc;
        if (spec->bins) std::memcpy(hist, f.h_block + kFsRecBytes, hist_bytes);
        return WTGPU_OK;
    });
}
int wtgpu_film_stats_source_host(const wtgpu_scene* s, const wtgpu_film_source* film, const wtgpu_film_stats_spec* spec, const float* mask, uint32_t n_threads,
                                 wtgpu_film_stats* out, uint64_t* hist) {
    if (!s || !film || !spec || !out || (!hist && spec->bins > 0)) return fail(WTGPU_ERR_INVALID, "null argument");
    if (const int rc = film_source_check("film_stats", "", film)) return rc;
    uint32_t planes = 0;
    float edges[kFsMaxBins + 1];
    if (const int rc = film_stats_edges_for(spec, edges)) return rc;
    if (const int rc = film_planes_for(s, "film_stats", spec->stokes_component, spec->flags, planes)) return rc;
    return film_on_host([&] {
        film_stats_host(s->host.sensor, *film, spec->stokes_component, spec->flags, mask, edges, spec->bins, n_threads, out, reinterpret_cast<unsigned long long*>(hist));
    });
}
int wtgpu_film_stats_device(wtgpu_scene* s, void* stream_, const double* d_value, const double* d_weight, const double* d_light, uint64_t spe,
                            const wtgpu_film_stats_spec* spec, const float* d_mask, wtgpu_film_stats* out, uint64_t* hist) {
    if (!s || !d_value || !d_weight || !d_light || !spec || !out || (!hist && spec->bins > 0)) return fail(WTGPU_ERR_INVALID, "null argument");
    const wtgpu_film_source film = accumulators(d_value, d_weight, d_light, spe);
    return wtgpu_film_stats_source_device(s, stream_, &film, spec, d_mask, out, hist);
}
int wtgpu_film_stats_host(const wtgpu_scene* s, const double* value, const double* weight, const double* light, uint64_t spe, const wtgpu_film_stats_spec* spec,
                          const float* mask, uint32_t n_threads, wtgpu_film_stats* out, uint64_t* hist) {
    if (!s || !value || !weight || !light || !spec || !out || (!hist && spec->bins > 0)) return fail(WTGPU_ERR_INVALID, "null argument");
    const wtgpu_film_source film = accumulators(value, weight, light, spe);
    return wtgpu_film_stats_source_host(s, &film, spec, mask, n_threads, out, hist);
}

// ---- zonal film statistics (kernels_zonal.hip; wt/film_zonal.h) ---------------------------------------------------------------------------------
static_assert(sizeof(wtgpu_film_zonal) == sizeof(film_zonal_rec_t) && offsetof(wtgpu_film_zonal, n_above) == offsetof(film_zonal_rec_t, count) + FZ_ABOVE * 8 &&
                  offsetof(wtgpu_film_zonal, n_inf) == offsetof(film_zonal_rec_t, count) + FZ_INF * 8 && offsetof(wtgpu_film_zonal, min) == offsetof(film_zonal_rec_t, min) &&
                  offsetof(wtgpu_film_zonal, sum) == offsetof(film_zonal_rec_t, sum),
              "the kernels' record is wtgpu_film_zonal");
// What both entry points check: the film statistics' refusals in their words, then the zones'.  planes: records per zone; edges: the spec's table.
static int film_zonal_check(const wtgpu_scene* s, const wtgpu_film_source* film, const wtgpu_film_zonal_spec* spec, const uint32_t* zones, const wtgpu_film_zonal* out,
                            const uint64_t* hist, const uint64_t* n_outside, uint32_t& planes, float* edges) {
    if (!s || !film || !spec) return fail(WTGPU_ERR_INVALID, "null argument");
    if (!zones) return fail(WTGPU_ERR_INVALID, "film_zonal: a zone plane expected (zones is NULL)");
    if (!out || !n_outside) return fail(WTGPU_ERR_INVALID, "film_zonal: out and n_outside expected (one of them is NULL)");
    if (const int rc = film_source_check("film_zonal", "", film)) return rc;
    const wtgpu_film_stats_spec fs{spec->stokes_component, spec->scale, spec->bins, spec->flags, spec->lo, spec->hi};
    if (const int rc = film_stats_edges_for(&fs, edges, "film_zonal")) return rc;
    if (const int rc = film_planes_for(s, "film_zonal", spec->stokes_component, spec->flags, planes)) return rc;
    if (spec->n_zones == 0 || spec->n_zones > kFzMaxZones)
        return fail(WTGPU_ERR_INVALID, "film_zonal: n_zones " + std::to_string(spec->n_zones) + " out of range (1 .. " + std::to_string(kFzMaxZones) + ")");
    if ((uint64_t)spec->n_zones * spec->bins > kFzMaxZoneBins)
        return fail(WTGPU_ERR_INVALID, "film_zonal: n_zones x bins = " + std::to_string((uint64_t)spec->n_zones * spec->bins) + " above the " + std::to_string(kFzMaxZoneBins) +
                                           " the histogram holds");
    if ((uint64_t)s->host.sensor.width * s->host.sensor.height >= kFzMaxPixels)
        return fail(WTGPU_ERR_INVALID, "film_zonal: a film of 2^31 pixels or more (a word of the exact sum could overflow)");
    if (!hist && spec->bins > 0) return fail(WTGPU_ERR_INVALID, "film_zonal: bins > 0 without a histogram (hist is NULL)");
    return WTGPU_OK;
}

int wtgpu_film_zonal_device(wtgpu_scene* s, void* stream_, const wtgpu_film_source* film, const wtgpu_film_zonal_spec* spec, const uint32_t* d_zones, const float* d_mask,
                            wtgpu_film_zonal* out, uint64_t* hist, uint64_t* n_outside, float* d_paint) {
    uint32_t planes = 0;
    float edges[kFsMaxBins + 1];
    if (const int rc = film_zonal_check(s, film, spec, d_zones, out, hist, n_outside, planes, edges)) return rc;
    return film_on_device(s, stream_, "film_zonal", [&](hipStream_t stream, uint64_t) -> int {
        // the block: records | edge table | histogram | n_outside | slots.  The first four come back through the pinned copy (which also carries the
        // edge table to the device); everything behind the edge table is cleared.  The call waits for its result, so the block is free again when
        // it returns.
        const size_t n_slots = (size_t)spec->n_zones * planes, rec_bytes = n_slots * sizeof(film_zonal_rec_t), edge_bytes = (((size_t)spec->bins + 2) & ~(size_t)1) * sizeof(float);
        const size_t hist_bytes = n_slots * spec->bins * sizeof(uint64_t), off_edge = rec_bytes, off_hist = off_edge + edge_bytes, off_outside = off_hist + hist_bytes;
        const size_t off_slots = off_outside + sizeof(uint64_t), total = off_slots + n_slots * sizeof(film_zonal_slot_t);
        if (s->d_zonal_bytes < total) {
            unsigned char* old = s->d_zonal;
            s->d_zonal = nullptr, s->d_zonal_bytes = 0;   // (reset first: a failed free leaves nothing behind for the next call)
            if (old) HIP_CHECK(hipFree(old));
            void* p = nullptr;
            if (const hipError_t e = hipMalloc(&p, total)) return fail(WTGPU_ERR_OOM, std::string("hipMalloc of ") + std::to_string(total) + " bytes: " + hipGetErrorString(e));
            s->d_zonal = static_cast<unsigned char*>(p), s->d_zonal_bytes = total;
        }
        if (s->h_zonal_bytes < off_slots) {
            unsigned char* old = s->h_zonal;
            s->h_zonal = nullptr, s->h_zonal_bytes = 0;
            if (old) HIP_CHECK(hipHostFree(old));
            HIP_CHECK(hipHostMalloc((void**)&s->h_zonal, off_slots, hipHostMallocDefault));
            s->h_zonal_bytes = off_slots;
        }
        unsigned char* d = s->d_zonal;
        std::memcpy(s->h_zonal + off_edge, edges, (spec->bins + 1) * sizeof(float));
        HIP_CHECK(hipMemcpyAsync(d + off_edge, s->h_zonal + off_edge, edge_bytes, hipMemcpyHostToDevice, stream));
        HIP_CHECK(hipMemsetAsync(d + off_hist, 0, total - off_hist, stream));
        // the LDS form wherever its table fits a launch, unless WTGPU_FILM_ZONAL_LDS=0
        const uint32_t lds = s->knobs.film_zonal_lds && film_zonal_lds_fits(spec->n_zones, planes, spec->bins) ? 1u : 0u;
        s->zonal_last_lds = lds;
        const int e = film_zonal_launch(s->host.sensor, stream, s->n_cus, *film, spec->stokes_component, spec->flags, d_zones, d_mask, reinterpret_cast<const float*>(d + off_edge),
                                        spec->bins, spec->n_zones, lds, s->knobs.film_zonal_blocks, d + off_slots,
                                        reinterpret_cast<unsigned long long*>(d + off_hist), reinterpret_cast<unsigned long long*>(d + off_outside), d, d_paint);
        if (e) return fail(WTGPU_ERR_HIP, std::string("k_film_zonal: ") + hipGetErrorString((hipError_t)e));
        HIP_CHECK(hipMemcpyAsync(s->h_zonal, d, off_slots, hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        std::memcpy(out, s->h_zonal, rec_bytes);
        if (spec->bins) std::memcpy(hist, s->h_zonal + off_hist, hist_bytes);
        std::memcpy(n_outside, s->h_zonal + off_outside, sizeof(uint64_t));
        return WTGPU_OK;
    });
}
int wtgpu_film_zonal_host(const wtgpu_scene* s, const wtgpu_film_source* film, const wtgpu_film_zonal_spec* spec, const uint32_t* zones, const float* mask, uint32_t n_threads,
                          wtgpu_film_zonal* out, uint64_t* hist, uint64_t* n_outside, float* paint) {
    uint32_t planes = 0;
    float edges[kFsMaxBins + 1];
    if (const int rc = film_zonal_check(s, film, spec, zones, out, hist, n_outside, planes, edges)) return rc;
    return film_on_host([&] {
        film_zonal_host(s->host.sensor, *film, spec->stokes_component, spec->flags, zones, mask, edges, spec->bins, spec->n_zones, n_threads, out,
                        reinterpret_cast<unsigned long long*>(hist), reinterpret_cast<unsigned long long*>(n_outside), paint);
    });
}
int wtgpu_test_film_zonal_form(const wtgpu_scene* s, uint32_t* lds) {
    if (!s || !lds) return fail(WTGPU_ERR_INVALID, "null argument");
    *lds = s->zonal_last_lds;
    return WTGPU_OK;
}
// the exact sum by itself (tests): words[9] += the addends of x[n], finite elements only; *out = fz_round(words)
int wtgpu_test_fz_sum(uint64_t* words, const float* x, uint64_t n, double* out) {
    if (!words || (!x && n) || !out) return fail(WTGPU_ERR_INVALID, "null argument");
    unsigned long long w[kFzWords];
    for (uint32_t k = 0; k < kFzWords; ++k) w[k] = words[k];
    for (uint64_t i = 0; i < n; ++i)
        if (fz_finite(x[i])) fz_add(w, x[i]);
    for (uint32_t k = 0; k < kFzWords; ++k) words[k] = w[k];
    *out = fz_round(w);
    return WTGPU_OK;
}

// ---- connected segments of a label plane (kernels_segments.hip; wt/film_segments.h) -----------------------------------------------------------------
static_assert(sizeof(wtgpu_film_segment) == sizeof(film_segment_t) && offsetof(wtgpu_film_segment, first) == offsetof(film_segment_t, first) &&
                  offsetof(wtgpu_film_segment, y1) == offsetof(film_segment_t, y1) && offsetof(wtgpu_film_segment, sum_y) == offsetof(film_segment_t, sum_y),
              "the kernels' record is wtgpu_film_segment");
static_assert(sizeof(wtgpu_film_segments_info) == 4 * sizeof(unsigned long long) && sizeof(wtgpu_film_segments_info) <= kSegHeadBytes, "the head opens with wtgpu_film_segments_info");
// what both entry points check
static int film_segments_check(const wtgpu_scene* s, const wtgpu_film_segments_spec* spec, const uint32_t* segments, const wtgpu_film_segments_info* info,
                               const wtgpu_film_segment* records) {
    if (!s || !spec) return fail(WTGPU_ERR_INVALID, "null argument");
    if (!segments || !info) return fail(WTGPU_ERR_INVALID, "film_segments: segments and info expected (one of them is NULL)");
    if (!records && spec->max_records > 0) return fail(WTGPU_ERR_INVALID, "film_segments: max_records " + std::to_string(spec->max_records) + " without records (records is NULL)");
    if (spec->flags & ~(uint32_t)SEG_DIAGONAL) return fail(WTGPU_ERR_INVALID, "film_segments: flags 0 or 1 (DIAGONAL) expected, got " + std::to_string(spec->flags));
    if ((uint64_t)s->host.sensor.width * s->host.sensor.height >= kSegMaxPixels)
        return fail(WTGPU_ERR_INVALID, "film_segments: a sensor of 2^31 pixels or more (pixel indices and areas are 32-bit)");
    return WTGPU_OK;
}

int wtgpu_film_segments_device(wtgpu_scene* s, void* stream_, const wtgpu_film_segments_spec* spec, const uint32_t* d_classes, const float* d_mask, uint32_t* d_segments,
                               wtgpu_film_segments_info* info, wtgpu_film_segment* records) {
    if (const int rc = film_segments_check(s, spec, d_segments, info, records)) return rc;
    if (!s->uploaded) return fail(WTGPU_ERR_INVALID, "film_segments: scene not uploaded");
    return film_on_device(s, stream_, "film_segments", [&](hipStream_t stream, uint64_t npix) -> int {
        // the block: head | records | the union-find's arrays.  Head and records come back through the pinned copy; there are never more
        // segments than pixels.  The call waits for its result, so the block is free again when it returns.
        const uint32_t max_records = (uint32_t)std::min<uint64_t>(spec->max_records, npix);
        const size_t off_work = kSegHeadBytes + (size_t)max_records * sizeof(film_segment_t), total = off_work + (size_t)film_segments_scratch_words(npix) * sizeof(uint32_t);
        if (s->d_segments_bytes < total) {
            unsigned char* old = s->d_segments;
            s->d_segments = nullptr, s->d_segments_bytes = 0;   // (reset first: a failed free leaves nothing behind for the next call)
            if (old) HIP_CHECK(hipFree(old));
            void* p = nullptr;
            if (const hipError_t e = hipMalloc(&p, total)) return fail(WTGPU_ERR_OOM, std::string("hipMalloc of ") + std::to_string(total) + " bytes: " + hipGetErrorString(e));
            s->d_segments = static_cast<unsigned char*>(p), s->d_segments_bytes = total;
        }
        if (s->h_segments_bytes < off_work) {
            unsigned char* old = s->h_segments;
            s->h_segments = nullptr, s->h_segments_bytes = 0;
            if (old) HIP_CHECK(hipHostFree(old));
            HIP_CHECK(hipHostMalloc((void**)&s->h_segments, off_work, hipHostMallocDefault));
            s->h_segments_bytes = off_work;
        }
        unsigned char* d = s->d_segments;
        s->segments_last_overflow = 0xFFFFFFFFu;
        s->segments_last_tiled = s->knobs.film_segments_tiled ? 1u : 0u;
        const int e = film_segments_launch(s->host.sensor, stream, s->n_cus, s->segments_last_tiled, spec->flags, spec->min_area, max_records, d_classes, d_mask, d_segments, d, d + kSegHeadBytes,
                                           reinterpret_cast<uint32_t*>(d + off_work));
        if (e) return fail(WTGPU_ERR_HIP, std::string("k_seg: ") + hipGetErrorString((hipError_t)e));
        // the head first: it says how many records there are
        HIP_CHECK(hipMemcpyAsync(s->h_segments, d, kSegHeadBytes, hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        uint32_t overflow = 0;
        std::memcpy(&overflow, s->h_segments + sizeof(wtgpu_film_segments_info), sizeof overflow);
        s->segments_last_overflow = overflow;
        if (overflow)
            return fail(WTGPU_ERR_HIP, "film_segments: a union-find loop hit its step bound (the pixel count): the library's fault, not the planes'; the segment plane holds nothing to be read");
        std::memcpy(info, s->h_segments, sizeof *info);
        const size_t n_rec = (size_t)std::min<uint64_t>(info->n_segments, max_records);
        if (n_rec) {
            HIP_CHECK(hipMemcpyAsync(s->h_segments + kSegHeadBytes, d + kSegHeadBytes, n_rec * sizeof(film_segment_t), hipMemcpyDeviceToHost, stream));
            HIP_CHECK(hipStreamSynchronize(stream));
            std::memcpy(records, s->h_segments + kSegHeadBytes, n_rec * sizeof(film_segment_t));
        }
        return WTGPU_OK;
    });
}
int wtgpu_film_segments_host(const wtgpu_scene* s, const wtgpu_film_segments_spec* spec, const uint32_t* classes, const float* mask, uint32_t n_threads, uint32_t* segments,
                             wtgpu_film_segments_info* info, wtgpu_film_segment* records) {
    if (const int rc = film_segments_check(s, spec, segments, info, records)) return rc;
    return film_on_host([&] {
        unsigned long long counts[4];
        film_segments_host(s->host.sensor, spec->flags, spec->min_area, spec->max_records, classes, mask, n_threads, segments, counts, records);
        *info = wtgpu_film_segments_info{counts[0], counts[1], counts[2], counts[3]};
    });
}
int wtgpu_test_film_segments_form(const wtgpu_scene* s, uint32_t* form, uint32_t* overflow) {
    if (!s || !form || !overflow) return fail(WTGPU_ERR_INVALID, "null argument");
    *form = s->segments_last_tiled;
    *overflow = s->segments_last_overflow;
    return WTGPU_OK;
}
int wtgpu_test_film_segments_find(const uint32_t* parent, uint32_t n, uint32_t x, uint32_t bound, uint32_t* root, uint32_t* overflow) {
    if (!parent || !root || !overflow || x >= n) return fail(WTGPU_ERR_INVALID, "film_segments_find: parent, root, overflow and x < n expected");
    for (uint32_t i = 0; i < n; ++i)
        if (parent[i] >= n) return fail(WTGPU_ERR_INVALID, "film_segments_find: parent[" + std::to_string(i) + "] is not below n");
    bool over = false;
    *root = film_segments_find_host(parent, x, bound, over);
    *overflow = over ? 1u : 0u;
    return WTGPU_OK;
}

// ---- distance transform of a label plane (kernels_distance.hip; wt/film_distance.h) -------------------------------------------------------------------
static_assert(sizeof(wtgpu_film_distance_info) == 24 && offsetof(wtgpu_film_distance_info, max_dist2) == 16, "wtgpu_film_distance_info");
// what both entry points check
static int film_distance_check(const wtgpu_scene* s, const wtgpu_film_distance_spec* spec, const uint32_t* dist2, const wtgpu_film_distance_info* info) {
    if (!s || !spec) return fail(WTGPU_ERR_INVALID, "null argument");
    if (!dist2 || !info) return fail(WTGPU_ERR_INVALID, "film_distance: dist2 and info expected (one of them is NULL)");
    if (spec->flags & ~(uint32_t)DIST_INVERT) return fail(WTGPU_ERR_INVALID, "film_distance: flags 0 or 1 (INVERT) expected, got " + std::to_string(spec->flags));
    if (s->host.sensor.width > kDistMaxSide || s->host.sensor.height > kDistMaxSide)
        return fail(WTGPU_ERR_INVALID, "film_distance: a sensor wider or higher than 32768 pixels (squared distances stay below 2^31 and a vertical offset fits 16 bits)");
    return WTGPU_OK;
}

int wtgpu_film_distance_device(wtgpu_scene* s, void* stream_, const wtgpu_film_distance_spec* spec, const uint32_t* d_classes, const float* d_mask, uint32_t* d_dist2,
                               uint32_t* d_nearest, wtgpu_film_distance_info* info) {
    if (const int rc = film_distance_check(s, spec, d_dist2, info)) return rc;
    if (!s->uploaded) return fail(WTGPU_ERR_INVALID, "film_distance: scene not uploaded");
    return film_on_device(s, stream_, "film_distance", [&](hipStream_t stream, uint64_t) -> int {
        // the block: head | the column offsets and the groups' minima.  The head comes back through the pinned copy; the call waits for its result,
        // so the block is free again when it returns.
        const size_t total = kDistHeadBytes + (size_t)film_distance_scratch_bytes(s->host.sensor.width, s->host.sensor.height);
        if (s->d_distance_bytes < total) {
            unsigned char* old = s->d_distance;
            s->d_distance = nullptr, s->d_distance_bytes = 0;   // (reset first: a failed free leaves nothing behind for the next call)
            if (old) HIP_CHECK(hipFree(old));
            void* p = nullptr;
            if (const hipError_t e = hipMalloc(&p, total)) return fail(WTGPU_ERR_OOM, std::string("hipMalloc of ") + std::to_string(total) + " bytes: " + hipGetErrorString(e));
            s->d_distance = static_cast<unsigned char*>(p), s->d_distance_bytes = total;
        }
        if (!s->h_distance) HIP_CHECK(hipHostMalloc((void**)&s->h_distance, kDistHeadBytes, hipHostMallocDefault));
        unsigned char* d = s->d_distance;
        s->distance_last_groups = s->knobs.film_distance_groups ? 1u : 0u;
        const int e = film_distance_launch(s->host.sensor, stream, s->distance_last_groups, spec->flags, d_classes, d_mask, d_dist2, d_nearest, d, d + kDistHeadBytes);
        if (e) return fail(WTGPU_ERR_HIP, std::string("k_dist: ") + hipGetErrorString((hipError_t)e));
        HIP_CHECK(hipMemcpyAsync(s->h_distance, d, kDistHeadBytes, hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        unsigned long long head[2];
        std::memcpy(head, s->h_distance, sizeof head);
        *info = wtgpu_film_distance_info{head[0], (uint32_t)~(uint32_t)head[1], (uint32_t)(head[1] >> 32), 0u};
        return WTGPU_OK;
    });
}
int wtgpu_film_distance_host(const wtgpu_scene* s, const wtgpu_film_distance_spec* spec, const uint32_t* classes, const float* mask, uint32_t n_threads, uint32_t* dist2,
                             uint32_t* nearest, wtgpu_film_distance_info* info) {
    if (const int rc = film_distance_check(s, spec, dist2, info)) return rc;
    if ((uint64_t)s->host.sensor.width * s->host.sensor.height == 0) return fail(WTGPU_ERR_INVALID, "film_distance: the film has no pixels");
    return film_on_host([&] {
        unsigned long long out[3];
        film_distance_host(s->host.sensor, spec->flags, classes, mask, n_threads, dist2, nearest, out);
        *info = wtgpu_film_distance_info{out[0], out[1], (uint32_t)out[2], 0u};
    });
}
int wtgpu_test_film_distance_form(const wtgpu_scene* s, uint32_t* groups) {
    if (!s || !groups) return fail(WTGPU_ERR_INVALID, "null argument");
    *groups = s->distance_last_groups;
    return WTGPU_OK;
}

// ---- film comparison (kernels_compare.hip; wt/film_compare.h) -------------------------------------------------------------------------------
// wtgpu_film_compare and wtgpu_film_polar are film_best_rec_t (wt/film_compare.h): n, three counts, argmax, the maximum, the sums
#define FILM_BEST_REC_IS(T, K, first_count, best_, first_sum)                                                                                                    \
    static_assert(sizeof(T) == sizeof(film_best_rec_t<K>) && offsetof(T, n) == offsetof(film_best_rec_t<K>, n) &&                                               \
                      offsetof(T, first_count) == offsetof(film_best_rec_t<K>, count) && offsetof(T, argmax) == offsetof(film_best_rec_t<K>, argmax) &&         \
                      offsetof(T, best_) == offsetof(film_best_rec_t<K>, best) && offsetof(T, first_sum) == offsetof(film_best_rec_t<K>, sum),                  \
                  "the kernels' record is " #T)
FILM_BEST_REC_IS(wtgpu_film_compare, kFcSums, n_nonfinite, max_abs, sum_abs);
FILM_BEST_REC_IS(wtgpu_film_polar, kFpSums, n_nonfinite, max_dop, sum_i);
// what a spec says by itself and against the scene's film; planes: records per call
static int film_compare_check(const wtgpu_scene* s, const wtgpu_film_compare_spec* spec, uint32_t& planes) {
    if (spec->flags & ~(FS_ABS | FS_LUMINANCE)) return fail(WTGPU_ERR_INVALID, "film_compare: flags 1 (ABS) and 2 (LUMINANCE) expected");
    if (!std::isfinite(spec->eps) || !(spec->eps > 0.0)) return fail(WTGPU_ERR_INVALID, "film_compare: a finite eps > 0 expected");
    return film_planes_for(s, "film_compare", spec->stokes_component, spec->flags, planes);
}

int wtgpu_film_compare_source_device(wtgpu_scene* s, void* stream_, const wtgpu_film_source* a, const wtgpu_film_source* b, const wtgpu_film_compare_spec* spec,
                                     const float* d_mask, wtgpu_film_compare* out, float* d_diff) {
    if (!s || !a || !b || !spec || !out) return fail(WTGPU_ERR_INVALID, "null argument");
    if (const int rc = film_source_check("film_compare", "A: ", a)) return rc;
    if (const int rc = film_source_check("film_compare", "B: ", b)) return rc;
    uint32_t planes = 0;
    if (const int rc = film_compare_check(s, spec, planes)) return rc;
    return film_on_device(s, stream_, "film_compare", [&](hipStream_t stream, uint64_t npix) -> int {
        film_scratch_t& f = s->fc;
        if (const int rc = film_rec_scratch<kFcSums>(s, f, npix)) return rc;
        const int e = film_compare_launch(s->host.sensor, stream, s->n_cus, *a, *b, spec->stokes_component, spec->flags, spec->eps, d_mask, f.d_block, f.d_sums, f.d_block + kFilmRecBytes<kFcSums>, d_diff);
        if (e) return fail(WTGPU_ERR_HIP, std::string("k_film_compare: ") + hipGetErrorString((hipError_t)e));
        return film_records_back(f, stream, out, planes * sizeof(wtgpu_film_compare));
    });
}
int wtgpu_film_compare_source_host(const wtgpu_scene* s, const wtgpu_film_source* a, const wtgpu_film_source* b, const wtgpu_film_compare_spec* spec, const float* mask,
                                   uint32_t n_threads, wtgpu_film_compare* out, float* diff) {
    if (!s || !a || !b || !spec || !out) return fail(WTGPU_ERR_INVALID, "null argument");
    if (const int rc = film_source_check("film_compare", "A: ", a)) return rc;
    if (const int rc = film_source_check("film_compare", "B: ", b)) return rc;
    uint32_t planes = 0;
    if (const int rc = film_compare_check(s, spec, planes)) return rc;
    return film_on_host([&] { film_compare_host(s->host.sensor, *a, *b, spec->stokes_component, spec->flags, spec->eps, mask, n_threads, out, diff); });
}
int wtgpu_film_compare_device(wtgpu_scene* s, void* stream_, const double* a_value, const double* a_weight, const double* a_light, uint64_t spe_a, const double* b_value,
                              const double* b_weight, const double* b_light, uint64_t spe_b, const wtgpu_film_compare_spec* spec, const float* d_mask,
                              wtgpu_film_compare* out, float* d_diff) {
    if (!s || !a_value || !a_weight || !a_light || !b_value || !b_weight || !b_light || !spec || !out) return fail(WTGPU_ERR_INVALID, "null argument");
    const wtgpu_film_source a = accumulators(a_value, a_weight, a_light, spe_a), b = accumulators(b_value, b_weight, b_light, spe_b);
    return wtgpu_film_compare_source_device(s, stream_, &a, &b, spec, d_mask, out, d_diff);
}
int wtgpu_film_compare_host(const wtgpu_scene* s, const double* a_value, const double* a_weight, const double* a_light, uint64_t spe_a, const double* b_value,
                            const double* b_weight, const double* b_light, uint64_t spe_b, const wtgpu_film_compare_spec* spec, const float* mask, uint32_t n_threads,
                            wtgpu_film_compare* out, float* diff) {
    if (!s || !a_value || !a_weight || !a_light || !b_value || !b_weight || !b_light || !spec || !out) return fail(WTGPU_ERR_INVALID, "null argument");
    const wtgpu_film_source a = accumulators(a_value, a_weight, a_light, spe_a), b = accumulators(b_value, b_weight, b_light, spe_b);
    return wtgpu_film_compare_source_host(s, &a, &b, spec, mask, n_threads, out, diff);
}

// ---- the polarisation view of a Stokes film (kernels_polar.hip; wt/film_polar.h) ------------------------------------------------------------
// what a spec says by itself and against the scene's film; planes: records per call; a: what the kernels are told
static int film_polar_check(const wtgpu_scene* s, const wtgpu_film_polar_spec* spec, uint32_t& planes, film_polar_args_t& a) {
    const sensor_t& sn = s->host.sensor;
    if (film_stokes(sn) != 4) return fail(WTGPU_ERR_INVALID, "film_polar: a polarimetric film expected (this one has " + std::to_string(film_stokes(sn)) + " Stokes component)");
    if (sn.channels != 1 && sn.channels != 3) return fail(WTGPU_ERR_INVALID, "film_polar: a film of 1 or 3 channels expected");
    if (spec->flags & ~(uint32_t)FP_LUMINANCE) return fail(WTGPU_ERR_INVALID, "film_polar: flag 2 (LUMINANCE) expected");
    if ((spec->flags & FP_LUMINANCE) && sn.channels != 3) return fail(WTGPU_ERR_INVALID, "film_polar: LUMINANCE needs a 3-channel film (this one has " + std::to_string(sn.channels) + ")");
    if (spec->maps >> kFpMaps) return fail(WTGPU_ERR_INVALID, "film_polar: map bits 1 (DOLP), 2 (DOP), 4 (DOCP), 8 (AOLP), 16 (CHI) and 32 (ANALYSER) expected");
    if (!std::isfinite(spec->c2) || !std::isfinite(spec->s2)) return fail(WTGPU_ERR_INVALID, "film_polar: finite c2 and s2 expected");
    if (!std::isfinite(spec->sat_gain) || spec->sat_gain < 0.f) return fail(WTGPU_ERR_INVALID, "film_polar: a finite sat_gain >= 0 expected");
    planes = sn.channels + ((spec->flags & FP_LUMINANCE) ? 1u : 0u);
    if (spec->picture_plane >= planes)
        return fail(WTGPU_ERR_INVALID, "film_polar: picture_plane " + std::to_string(spec->picture_plane) + " out of range (the call has " + std::to_string(planes) + ")");
    if (spec->format > TM_U16) return fail(WTGPU_ERR_INVALID, "film_polar: format 0 (f32), 1 (u8) or 2 (u16) expected");
    const wtgpu_tonemap& tm = spec->tonemap;
    if (const int rc = tonemap_op_check(tm.op, TM_NORMAL, tm.gamma, tm.db_min, tm.db_max, "film_polar: ", "film_polar: ")) return rc;   // (the picture has no mode)
    a = film_polar_args_t{};
    a.c2 = spec->c2, a.s2 = spec->s2;
    a.maps = spec->maps;
    for (uint32_t m = 0; m < kFpMaps; ++m) a.n_maps += spec->maps >> m & 1u;
    a.picture_plane = spec->picture_plane, a.format = spec->format;
    a.sat_gain = spec->sat_gain;
    a.tm.op = tm.op;
    a.tm.mode = TM_NORMAL;
    a.tm.inv_gamma = tm.op == TM_GAMMA ? 1.f / tm.gamma : 1.f;
    a.tm.db_min = tm.db_min;
    a.tm.db_len = tm.db_max - tm.db_min;
    return WTGPU_OK;
}

int wtgpu_film_polar_source_device(wtgpu_scene* s, void* stream_, const wtgpu_film_source* film, const wtgpu_film_polar_spec* spec, const float* d_mask, wtgpu_film_polar* out,
                                   float* d_maps, void* d_picture) {
    if (!s || !film || !spec || !out) return fail(WTGPU_ERR_INVALID, "null argument");
    if (const int rc = film_source_check("film_polar", "", film)) return rc;
    uint32_t planes = 0;
    film_polar_args_t a{};
    if (const int rc = film_polar_check(s, spec, planes, a)) return rc;
    if (d_maps && a.n_maps == 0) return fail(WTGPU_ERR_INVALID, "film_polar: d_maps without a map bit");
    return film_on_device(s, stream_, "film_polar", [&](hipStream_t stream, uint64_t npix) -> int {
        film_scratch_t& f = s->fp;
        if (const int rc = film_rec_scratch<kFpSums>(s, f, npix)) return rc;
        const int e = film_polar_launch(s->host.sensor, stream, s->n_cus, *film, spec->flags, a, s->knobs.film_polar_staged, d_mask, f.d_block,
                                        f.d_sums, f.d_block + kFilmRecBytes<kFpSums>, d_maps, d_picture);
        if (e) return fail(WTGPU_ERR_HIP, std::string("k_film_polar: ") + hipGetErrorString((hipError_t)e));
        return film_records_back(f, stream, out, planes * sizeof(wtgpu_film_polar));
    });
}
int wtgpu_film_polar_source_host(const wtgpu_scene* s, const wtgpu_film_source* film, const wtgpu_film_polar_spec* spec, const float* mask, uint32_t n_threads,
                                 wtgpu_film_polar* out, float* maps, void* picture) {
    if (!s || !film || !spec || !out) return fail(WTGPU_ERR_INVALID, "null argument");
    if (const int rc = film_source_check("film_polar", "", film)) return rc;
    uint32_t planes = 0;
    film_polar_args_t a{};
    if (const int rc = film_polar_check(s, spec, planes, a)) return rc;
    if (maps && a.n_maps == 0) return fail(WTGPU_ERR_INVALID, "film_polar: maps without a map bit");
    return film_on_host([&] { film_polar_host(s->host.sensor, *film, spec->flags, a, mask, n_threads, out, maps, picture); });
}
int wtgpu_film_polar_device(wtgpu_scene* s, void* stream_, const double* d_value, const double* d_weight, const double* d_light, uint64_t spe,
                            const wtgpu_film_polar_spec* spec, const float* d_mask, wtgpu_film_polar* out, float* d_maps, void* d_picture) {
    if (!s || !d_value || !d_weight || !d_light || !spec || !out) return fail(WTGPU_ERR_INVALID, "null argument");
    const wtgpu_film_source film = accumulators(d_value, d_weight, d_light, spe);
    return wtgpu_film_polar_source_device(s, stream_, &film, spec, d_mask, out, d_maps, d_picture);
}
int wtgpu_film_polar_host(const wtgpu_scene* s, const double* value, const double* weight, const double* light, uint64_t spe, const wtgpu_film_polar_spec* spec,
                          const float* mask, uint32_t n_threads, wtgpu_film_polar* out, float* maps, void* picture) {
    if (!s || !value || !weight || !light || !spec || !out) return fail(WTGPU_ERR_INVALID, "null argument");
    const wtgpu_film_source film = accumulators(value, weight, light, spe);
    return wtgpu_film_polar_source_host(s, &film, spec, mask, n_threads, out, maps, picture);
}

// ---- denoising a film from its two half-films (kernels_denoise.hip; wt/film_denoise.h) -------------------------------------------------------
// what a spec says by itself and against the scene's film; a: what the kernels are told
static int film_denoise_check(const wtgpu_scene* s, const wtgpu_film_denoise_spec* spec, film_denoise_args_t& a) {
    const sensor_t& sn = s->host.sensor;
    if (sn.channels != 1 && sn.channels != 3) return fail(WTGPU_ERR_INVALID, "film_denoise: a film of 1 or 3 channels expected");
    if (spec->window_radius > kDnMaxWindow)
        return fail(WTGPU_ERR_INVALID, "film_denoise: window_radius " + std::to_string(spec->window_radius) + " out of range (0 .. " + std::to_string(kDnMaxWindow) + ")");
    if (spec->patch_radius > kDnMaxPatch)
        return fail(WTGPU_ERR_INVALID, "film_denoise: patch_radius " + std::to_string(spec->patch_radius) + " out of range (0 .. " + std::to_string(kDnMaxPatch) + ")");
    if (spec->flags) return fail(WTGPU_ERR_INVALID, "film_denoise: no flags are defined (0 expected)");
    if (!std::isfinite(spec->k) || !(spec->k > 0.f)) return fail(WTGPU_ERR_INVALID, "film_denoise: a finite k > 0 expected");
    if (!std::isfinite(spec->alpha) || spec->alpha < 0.f) return fail(WTGPU_ERR_INVALID, "film_denoise: a finite alpha >= 0 expected");
    if (!std::isfinite(spec->eps) || !(spec->eps > 0.f)) return fail(WTGPU_ERR_INVALID, "film_denoise: a finite eps > 0 expected");
    static_assert(kFsMaxPlanes * 3 == kDnMaxPlanes, "three channels of four Stokes components");
    a = film_denoise_args_t{};
    a.r = spec->window_radius, a.f = spec->patch_radius;
    a.k2 = spec->k * spec->k;
    a.alpha = spec->alpha, a.eps = spec->eps;
    const uint32_t side = 2u * a.f + 1u;
    a.inv_norm = 1.0f / (float)(sn.channels * side * side);
    return WTGPU_OK;
}

// what the guides say by themselves and against the pointers that come with them; gd: what the kernels and the host twin are told
static int film_denoise_guides_check(const wtgpu_film_denoise_guides* guides, const void* guide, const void* ids, film_denoise_guides_t& gd) {
    static_assert(sizeof(wtgpu_film_denoise_guides) == sizeof(film_denoise_guides_t) && kDnMaxGuides == 8, "the public struct is the header's");
    if (guides->n_guides > kDnMaxGuides)
        return fail(WTGPU_ERR_INVALID, "film_denoise_guided: n_guides " + std::to_string(guides->n_guides) + " out of range (0 .. " + std::to_string(kDnMaxGuides) + ")");
    if (guides->flags & ~kDnSameId) return fail(WTGPU_ERR_INVALID, "film_denoise_guided: unknown flag bits (1 SAME_ID is the only one)");
    const bool same_id = (guides->flags & kDnSameId) != 0;
    if (guides->n_guides == 0 && !same_id)
        return fail(WTGPU_ERR_INVALID, "film_denoise_guided: neither guides nor SAME_ID: this is the unguided call (wtgpu_film_denoise_device / _host)");
    for (uint32_t g = 0; g < guides->n_guides; ++g)
        if (!std::isfinite(guides->scale[g]) || guides->scale[g] < 0.f)
            return fail(WTGPU_ERR_INVALID, "film_denoise_guided: scale " + std::to_string(g) + ": a finite value >= 0 expected");
    if (guides->n_guides > 0 && !guide) return fail(WTGPU_ERR_INVALID, "film_denoise_guided: n_guides > 0 without a guide buffer");
    if (guides->n_guides == 0 && guide) return fail(WTGPU_ERR_INVALID, "film_denoise_guided: a guide buffer with n_guides = 0");
    if (same_id && !ids) return fail(WTGPU_ERR_INVALID, "film_denoise_guided: SAME_ID without an id plane");
    if (!same_id && ids) return fail(WTGPU_ERR_INVALID, "film_denoise_guided: an id plane without SAME_ID");
    gd = film_denoise_guides_t{};
    gd.n = guides->n_guides, gd.flags = guides->flags;
    for (uint32_t g = 0; g < gd.n; ++g) gd.scale[g] = guides->scale[g];
    return WTGPU_OK;
}

// The two device entries: `guides` (with d_guide, d_ids) where the call is the guided one.
static int film_denoise_device(wtgpu_scene* s, void* stream_, const double* a_value, const double* a_weight, const double* a_light, uint64_t spe_a, const double* b_value,
                               const double* b_weight, const double* b_light, uint64_t spe_b, const wtgpu_film_denoise_spec* spec, bool guided,
                               const wtgpu_film_denoise_guides* guides, const float* d_guide, const uint32_t* d_ids, const float* d_mask, float* d_out, float* d_residual) {
    if (!s || !a_value || !a_weight || !a_light || !b_value || !b_weight || !b_light || !spec || (guided && !guides) || !d_out) return fail(WTGPU_ERR_INVALID, "null argument");
    film_denoise_args_t a{};
    if (const int rc = film_denoise_check(s, spec, a)) return rc;
    film_denoise_guides_t gd{};
    if (guided)
        if (const int rc = film_denoise_guides_check(guides, d_guide, d_ids, gd)) return rc;
    return film_on_device(s, stream_, "film_denoise", [&](hipStream_t stream, uint64_t) -> int {
        const sensor_t& sn = s->host.sensor;
        // first use: the developed half-films, their variance, what one direction leaves for the other (the guides are read where the caller has
        // them).  Nothing comes back to the host, so the call does not wait; calls on different streams would share the scratch memory and must be
        // ordered by the caller.
        if (!s->d_denoise)
            if (const int rc = dmalloc(s, &s->d_denoise, film_denoise_scratch_floats(sn))) return rc;
        // Both directions in one launch up to 4 planes, one launch each for 12, unless the knob says otherwise: film_denoise_launch has the measurement.
        const uint32_t fused = s->knobs.film_denoise_fused == 2 ? (film_planes(sn) <= 4 ? 1u : 0u) : s->knobs.film_denoise_fused;
        const int e = guided ? film_denoise_guided_launch(sn, stream, a_value, a_weight, a_light, spe_a, b_value, b_weight, b_light, spe_b, a, fused, gd,
                                                          s->knobs.film_denoise_guide_lds, d_guide, d_ids, d_mask, s->d_denoise, d_out, d_residual)
                             : film_denoise_launch(sn, stream, a_value, a_weight, a_light, spe_a, b_value, b_weight, b_light, spe_b, a, fused, d_mask, s->d_denoise, d_out,
                                                   d_residual);
        if (e) return fail(WTGPU_ERR_HIP, std::string(guided ? "k_denoise_filter (guided): " : "k_denoise_filter: ") + hipGetErrorString((hipError_t)e));
        return WTGPU_OK;
    });
}
static int film_denoise_on_host(const wtgpu_scene* s, const double* a_value, const double* a_weight, const double* a_light, uint64_t spe_a, const double* b_value,
                                const double* b_weight, const double* b_light, uint64_t spe_b, const wtgpu_film_denoise_spec* spec, bool guided,
                                const wtgpu_film_denoise_guides* guides, const float* guide, const uint32_t* ids, const float* mask, uint32_t n_threads, float* out,
                                float* residual) {
    if (!s || !a_value || !a_weight || !a_light || !b_value || !b_weight || !b_light || !spec || (guided && !guides) || !out) return fail(WTGPU_ERR_INVALID, "null argument");
    film_denoise_args_t a{};
    if (const int rc = film_denoise_check(s, spec, a)) return rc;
    film_denoise_guides_t gd{};
    if (guided)
        if (const int rc = film_denoise_guides_check(guides, guide, ids, gd)) return rc;
    return film_on_host([&] {
        film_denoise_host(s->host.sensor, a_value, a_weight, a_light, spe_a, b_value, b_weight, b_light, spe_b, a, mask, n_threads, out, residual, guided ? &gd : nullptr,
                          guided ? guide : nullptr, guided ? ids : nullptr);
    });
}

int wtgpu_film_denoise_device(wtgpu_scene* s, void* stream_, const double* a_value, const double* a_weight, const double* a_light, uint64_t spe_a, const double* b_value,
                              const double* b_weight, const double* b_light, uint64_t spe_b, const wtgpu_film_denoise_spec* spec, const float* d_mask, float* d_out,
                              float* d_residual) {
    return film_denoise_device(s, stream_, a_value, a_weight, a_light, spe_a, b_value, b_weight, b_light, spe_b, spec, false, nullptr, nullptr, nullptr, d_mask, d_out, d_residual);
}
int wtgpu_film_denoise_host(const wtgpu_scene* s, const double* a_value, const double* a_weight, const double* a_light, uint64_t spe_a, const double* b_value,
                            const double* b_weight, const double* b_light, uint64_t spe_b, const wtgpu_film_denoise_spec* spec, const float* mask, uint32_t n_threads,
                            float* out, float* residual) {
    return film_denoise_on_host(s, a_value, a_weight, a_light, spe_a, b_value, b_weight, b_light, spe_b, spec, false, nullptr, nullptr, nullptr, mask, n_threads, out, residual);
}
int wtgpu_film_denoise_guided_device(wtgpu_scene* s, void* stream_, const double* a_value, const double* a_weight, const double* a_light, uint64_t spe_a,
                                     const double* b_value, const double* b_weight, const double* b_light, uint64_t spe_b, const wtgpu_film_denoise_spec* spec,
                                     const wtgpu_film_denoise_guides* guides, const float* d_guide, const uint32_t* d_ids, const float* d_mask, float* d_out,
                                     float* d_residual) {
    return film_denoise_device(s, stream_, a_value, a_weight, a_light, spe_a, b_value, b_weight, b_light, spe_b, spec, true, guides, d_guide, d_ids, d_mask, d_out, d_residual);
}
int wtgpu_film_denoise_guided_host(const wtgpu_scene* s, const double* a_value, const double* a_weight, const double* a_light, uint64_t spe_a, const double* b_value,
                                   const double* b_weight, const double* b_light, uint64_t spe_b, const wtgpu_film_denoise_spec* spec,
                                   const wtgpu_film_denoise_guides* guides, const float* guide, const uint32_t* ids, const float* mask, uint32_t n_threads, float* out,
                                   float* residual) {
    return film_denoise_on_host(s, a_value, a_weight, a_light, spe_a, b_value, b_weight, b_light, spe_b, spec, true, guides, guide, ids, mask, n_threads, out, residual);
}
int wtgpu_test_dn_exp2_neg(const float* t, uint64_t n, float* out) {
    if (!t || !out) return fail(WTGPU_ERR_INVALID, "null argument");
    film_denoise_exp2_neg(t, n, out);
    return WTGPU_OK;
}

}   // extern "C"
