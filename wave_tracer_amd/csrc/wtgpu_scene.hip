// wave_tracer_amd — the scene object on the host: creation (bundled scene / scene file / flattened description), comparison (test hook), info,
// destruction.  Nothing here touches the device except wtgpu_scene_destroy's release (wtgpu_upload.hip).
#include "wtgpu_host.h"
#include "scene_abi_check.h"

// How far the scene's records reach into its variable-length arrays.  Upload and comparison agree on the spectrum words (SPEC_TABLE is the one
// spectrum type with data: wt/scene.h).  They do NOT agree on the k-distributions, and each keeps its own numbers: upload copies the n_emitters
// records of kdists and skips discrete ones; comparison walks max(emitter.k_dist) + 1 records and skips none.
scene_extents_t scene_extents(const scene_t& h) {
    scene_extents_t ex;
    for (uint32_t i = 0; i < h.n_shapes; ++i) ex.shape_tris += h.shapes[i].tri_count;
    for (uint32_t i = 0; i < h.n_spectra; ++i)
        if (h.spectra[i].type == SPEC_TABLE) ex.spec_words = std::max(ex.spec_words, (size_t)h.spectra[i].offset + (size_t)h.spectra[i].count * (h.spectra[i].is_complex ? 2 : 1));
    for (uint32_t i = 0; i < h.n_textures; ++i)
        if (h.textures[i].type == TEX_BITMAP)
            ex.tex_words = std::max(ex.tex_words, (size_t)h.textures[i].offset + (size_t)h.textures[i].width * h.textures[i].height * h.textures[i].channels);
        else if (h.textures[i].type == TEX_FUNCTION)
            ex.tex_words = std::max(ex.tex_words, (size_t)h.textures[i].offset + (size_t)h.textures[i].width);
    for (uint32_t i = 0; i < h.n_emitters; ++i)   // the texel tables of textured area emitters live in texture_data as well (validated at upload)
        if (h.emitters[i].type == EMIT_AREA && h.emitters[i].radiance_tex > 0) ex.tex_words = std::max(ex.tex_words, (size_t)h.emitters[i].tab + (size_t)h.emitters[i].tab_words);
    if (h.kdists) {
        for (uint32_t i = 0; i < h.n_emitters; ++i)
            if (!h.kdists[i].discrete) ex.kd_words = std::max(ex.kd_words, (size_t)h.kdists[i].offset + 2 * (size_t)h.kdists[i].count);
        for (uint32_t i = 0; i < h.n_emitters; ++i) ex.cmp_kdists = std::max<size_t>(ex.cmp_kdists, (size_t)h.emitters[i].k_dist + 1);
        for (size_t i = 0; i < ex.cmp_kdists; ++i) ex.cmp_kd_words = std::max<size_t>(ex.cmp_kd_words, h.kdists[i].offset + 2 * (size_t)h.kdists[i].count);
    }
    return ex;
}

static void finish_built_scene(wtgpu_scene* s) {
    s->host = s->builder->scene();
    s->stats = s->builder->stats();
    s->lut_power[0] = s->builder->fsd_lut_power(0);
    s->lut_power[1] = s->builder->fsd_lut_power(1);
}
// the parameter block both creating forms copy; what they default differently they set themselves
static wth::scene_params_t scene_params_of(const wtgpu_scene_params& in) {
    wth::scene_params_t p{};
    p.res = in.res;
    p.max_depth = in.max_depth;
    p.fsd = in.fsd;
    p.mis = in.mis;
    p.rr = in.rr;
    p.force_ray_tracing = in.force_ray_tracing;
    p.mesh_detail = in.mesh_detail;
    p.lut_n_theta = in.lut_n_theta;
    p.lut_m = in.lut_m;
    p.polarimetric = in.polarimetric;
    return p;
}

extern "C" {

int wtgpu_scene_create_named_hooks(const char* name, const wtgpu_scene_params* params, const wtgpu_test_hooks* hooks, wtgpu_scene** out) {
    if (!name || !params || !out) return fail(WTGPU_ERR_INVALID, "null argument");
    try {
        auto s = std::make_unique<wtgpu_scene>();
        s->builder = std::make_unique<wth::scene_builder_t>();
        wth::scene_params_t p = scene_params_of(*params);
        if (!p.res) p.res = 256;
        p.debug_only_s = hooks ? hooks->only_s : 0u;
        p.debug_only_t = hooks ? hooks->only_t : 0u;
        p.crop_of = hooks ? hooks->crop_of : 0u;
        if (!wth::build_named_scene(name, p, *s->builder)) return fail(WTGPU_ERR_INVALID, std::string("unknown scene ") + name);
        finish_built_scene(s.get());
        *out = s.release();
        return WTGPU_OK;
    } catch (const std::exception& e) {
        return fail(WTGPU_ERR_INVALID, e.what());
    }
}
int wtgpu_scene_create_named(const char* name, const wtgpu_scene_params* params, wtgpu_scene** out) {
    return wtgpu_scene_create_named_hooks(name, params, nullptr, out);
}

int wtgpu_scene_create_from_xml(const char* path, const char* const* defines, uint32_t n_defines, const wtgpu_scene_params* params, wtgpu_scene** out) {
    if (!path || !out || (n_defines && !defines)) return fail(WTGPU_ERR_INVALID, "null argument");
    try {
        auto s = std::make_unique<wtgpu_scene>();
        s->builder = std::make_unique<wth::scene_builder_t>();
        wth::scene_params_t p{};
        p.max_depth = p.fsd = p.mis = p.rr = -1;   // (as the file says)
        p.mesh_detail = 1;
        if (params) p = scene_params_of(*params);
        std::vector<std::string> defs;
        for (uint32_t i = 0; i < n_defines; ++i) {
            if (!defines[i]) return fail(WTGPU_ERR_INVALID, "null define");
            defs.emplace_back(defines[i]);
        }
        wth::build_scene_from_xml(path, defs, p, *s->builder, &s->file);
        finish_built_scene(s.get());
        *out = s.release();
        return WTGPU_OK;
    } catch (const std::exception& e) {
        return fail(WTGPU_ERR_INVALID, e.what());
    }
}

// Test hook: field-by-field comparison of two flattened scenes (every array the description names, byte for byte).  0: identical;
// 1: different — `what` names the first difference.
// `only`: nullptr = everything, else one of "sensor", "opts", "emitters" (records that do not depend on the geometry: a scene file whose
// meshes are absent can still be checked for what else it describes)
static int scene_compare(const wtgpu_scene* a, const wtgpu_scene* b, const char* only, char* what, size_t n_what) {
    if (!a || !b) return fail(WTGPU_ERR_INVALID, "null scene");
    const scene_t &x = a->host, &y = b->host;
    std::string diff;
    const std::string part = only ? only : "";
    auto wanted = [&](const char* name) {
        if (part.empty()) return true;
        const std::string n(name);
        if (part == "sensor") return n == "sensor";
        if (part == "opts") return n == "opts";
        if (part == "emitters") return n == "n_emitters" || n == "emitters" || n == "emitter_cdf";
        return false;
    };
    auto cnt = [&](const char* name, uint64_t u, uint64_t v) {
        if (!wanted(name)) return;
        if (diff.empty() && u != v) diff = std::string(name) + ": " + std::to_string(u) + " vs " + std::to_string(v);
    };
    auto arr = [&](const char* name, const void* u, const void* v, size_t bytes, size_t elem) {
        if (!wanted(name)) return;
        if (!diff.empty() || bytes == 0) return;
        if (!u || !v) {
            if (u != v) diff = std::string(name) + ": missing array";
            return;
        }
        if (std::memcmp(u, v, bytes) != 0) {
            size_t k = 0;
            while (k < bytes && ((const unsigned char*)u)[k] == ((const unsigned char*)v)[k]) ++k;
            diff = std::string(name) + ": element " + std::to_string(k / elem) + ", byte " + std::to_string(k % elem);
        }
    };
    cnt("n_tris", x.n_tris, y.n_tris);
    cnt("n_edges", x.n_edges, y.n_edges);
    cnt("n_nodes", x.n_nodes, y.n_nodes);
    cnt("n_leaves", x.n_leaves, y.n_leaves);
    cnt("n_shapes", x.n_shapes, y.n_shapes);
    cnt("n_materials", x.n_materials, y.n_materials);
    cnt("n_spectra", x.n_spectra, y.n_spectra);
    cnt("n_emitters", x.n_emitters, y.n_emitters);
    cnt("n_textures", x.n_textures, y.n_textures);
    cnt("lut.n_theta", x.lut.n_theta, y.lut.n_theta);
    cnt("lut.m", x.lut.m, y.lut.m);
    arr("sensor", &x.sensor, &y.sensor, sizeof(sensor_t), sizeof(sensor_t));
    arr("opts", &x.opts, &y.opts, sizeof(integrator_opts_t), sizeof(integrator_opts_t));
    arr("world_min", &x.world_min, &y.world_min, sizeof(vec3), sizeof(vec3));
    arr("world_max", &x.world_max, &y.world_max, sizeof(vec3), sizeof(vec3));
    arr("tri_geo", x.tri_geo, y.tri_geo, sizeof(tri_geo_t) * x.n_tris, sizeof(tri_geo_t));
    arr("tri_meta", x.tri_meta, y.tri_meta, sizeof(tri_meta_t) * x.n_tris, sizeof(tri_meta_t));
    arr("tri_shade", x.tri_shade, y.tri_shade, sizeof(tri_shade_t) * x.n_tris, sizeof(tri_shade_t));
    arr("edges", x.edges, y.edges, sizeof(edge_t) * x.n_edges, sizeof(edge_t));
    arr("nodes", x.nodes, y.nodes, sizeof(bvh8_node_t) * x.n_nodes, sizeof(bvh8_node_t));
    arr("leaves", x.leaves, y.leaves, sizeof(bvh8_leaf_t) * x.n_leaves, sizeof(bvh8_leaf_t));
    arr("shapes", x.shapes, y.shapes, sizeof(shape_t) * x.n_shapes, sizeof(shape_t));
    arr("materials", x.materials, y.materials, sizeof(material_t) * x.n_materials, sizeof(material_t));
    arr("spectra", x.spectra, y.spectra, sizeof(spectrum_t) * x.n_spectra, sizeof(spectrum_t));
    arr("textures", x.textures, y.textures, sizeof(texture_t) * x.n_textures, sizeof(texture_t));
    arr("emitters", x.emitters, y.emitters, sizeof(emitter_t) * x.n_emitters, sizeof(emitter_t));
    arr("emitter_cdf", x.emitter_cdf, y.emitter_cdf, sizeof(float) * (x.n_emitters + 1), sizeof(float));
    if (diff.empty() && part.empty()) {
        const scene_extents_t ex = scene_extents(x);
        arr("spectra_data", x.spectra_data, y.spectra_data, sizeof(float) * ex.spec_words, sizeof(float));
        arr("kdists", x.kdists, y.kdists, sizeof(kdist_t) * ex.cmp_kdists, sizeof(kdist_t));
        arr("kdist_data", x.kdist_data, y.kdist_data, sizeof(float) * ex.cmp_kd_words, sizeof(float));
        arr("lut.icdf_theta1", x.lut.icdf_theta1, y.lut.icdf_theta1, sizeof(float) * x.lut.n_theta, sizeof(float));
        arr("lut.icdf_theta2", x.lut.icdf_theta2, y.lut.icdf_theta2, sizeof(float) * x.lut.n_theta, sizeof(float));
        arr("lut.icdf1", x.lut.icdf1, y.lut.icdf1, sizeof(float) * (size_t)x.lut.m * x.lut.m, sizeof(float));
        arr("lut.icdf2", x.lut.icdf2, y.lut.icdf2, sizeof(float) * (size_t)x.lut.m * x.lut.m, sizeof(float));
    }
    if (what && n_what) {
        std::strncpy(what, diff.c_str(), n_what - 1);
        what[n_what - 1] = 0;
    }
    return diff.empty() ? 0 : 1;
}
int wtgpu_scene_compare(const wtgpu_scene* a, const wtgpu_scene* b, char* what, size_t n_what) { return scene_compare(a, b, nullptr, what, n_what); }
int wtgpu_scene_compare_part(const wtgpu_scene* a, const wtgpu_scene* b, const char* part, char* what, size_t n_what) {
    if (!part) return fail(WTGPU_ERR_INVALID, "null part");
    return scene_compare(a, b, part, what, n_what);
}

int wtgpu_scene_create_from_desc(const wtgpu_scene_desc* desc, wtgpu_scene** out) {
    if (!desc || !out) return fail(WTGPU_ERR_INVALID, "null argument");
    auto s = std::make_unique<wtgpu_scene>();
    std::memcpy(&s->host, desc, sizeof(scene_t));   // identical layouts: scene_abi_check.h
    if (s->host.n_tris > 0 && (!s->host.tri_geo || !s->host.tri_meta || !s->host.tri_shade || !s->host.nodes)) return fail(WTGPU_ERR_INVALID, "scene description lacks geometry arrays");
    s->stats = "{}";
    *out = s.release();
    return WTGPU_OK;
}

int wtgpu_scene_get_info(const wtgpu_scene* s, wtgpu_scene_info* info) {
    if (!s || !info) return fail(WTGPU_ERR_INVALID, "null argument");
    const scene_t& h = s->host;
    info->width = h.sensor.width;
    info->height = h.sensor.height;
    info->channels = h.sensor.channels;
    info->stokes = film_stokes(h.sensor);
    info->integrator = h.opts.integrator;
    info->n_tris = h.n_tris;
    info->n_edges = h.n_edges;
    info->n_nodes = h.n_nodes;
    info->n_leaves = h.n_leaves;
    info->n_shapes = h.n_shapes;
    info->n_emitters = h.n_emitters;
    info->n_materials = h.n_materials;
    info->max_depth = h.opts.max_depth;
    info->sensor_type = (uint32_t)h.sensor.type;
    info->fsd_lut_power[0] = s->lut_power[0];
    info->fsd_lut_power[1] = s->lut_power[1];
    const uint64_t mv = (uint64_t)h.opts.max_depth + 2;
    info->bytes_per_sample_state = 4ull * (2 * (kWalkWords + mv * kVertexWords + kTravWords + kMaxConeTris) + kCtxWords);
    return WTGPU_OK;
}

const wtgpu_scene_desc* wtgpu_scene_host_desc(const wtgpu_scene* s) { return s ? reinterpret_cast<const wtgpu_scene_desc*>(&s->host) : nullptr; }
const char* wtgpu_scene_stats_json(const wtgpu_scene* s) { return s ? s->stats.c_str() : "{}"; }

void wtgpu_scene_destroy(wtgpu_scene* s) {
    if (!s) return;
    release_device(s);
    delete s;
}

}   // extern "C"
