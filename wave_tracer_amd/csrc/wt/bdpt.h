// wave_tracer_amd — the bidirectional PLT integrator `plt_bdpt`: path vertices, subpath random walks, subpath
// connections and MIS.
//
// Reference: src/integrator/plt_bdpt.cpp:43-148 (per-sample loop),
//            include/wt/integrator/plt_bdpt/plt_bdpt_detail.hpp:70-183 (walk data), 192-346 (interactions),
//            348-419 (find_closest_triangle), 421-526 (random_walk), 528-581 (subpath generation),
//            604-720 (MIS), 722-745 (connect_and_integrate), 747-923 (connect_subpaths);
//            include/wt/integrator/plt_bdpt/vertex.hpp:49-565.
//
// The reference's recursion / std::vector<vertex_t> / unique_ptr<fsd> arena become: an explicit walk state, a
// strided vertex store (one SoA "plane" per vertex index) and a pool of fixed-capacity FSD apertures.  The
// functions here are the building blocks shared by the HIP wavefront kernels (wtgpu.hip) and by the scalar
// per-sample CPU loop of the checker (oracle/).
#pragma once
#include <cstddef>

#include "bvh.h"
#include "film.h"
#include "fsd.h"

namespace wt {

// Subpath lengths are not bounded at compile time (the reference's max_depth is a plain integer, src/integrator/plt_bdpt.cpp:111,169):
// vertex stores are sized from the scene's max_depth, the MIS weights stream over the vertices (bdpt_mis_weight).  kMaxVerts only sets the
// resolution of the device's strategy buckets: strategies with s or t >= kMaxVerts share the last bucket of their row / column.
constexpr uint32_t kMaxVerts = 18;
// Trace / interact rounds a subpath may take (device: rounds launched per batch; CPU checker: iterations of its walk loops — one definition for
// both).  The reference recurses without such a cap (plt_bdpt_detail.hpp:421-526): vertices are bounded by max_depth, but null interactions and
// restarts behind empty apertures add rounds without adding vertices.  Walks still active after the last round are dropped and COUNTED
// (wtgpu_counters::walk_iteration_cap_hits): none in the cornell / etoile workloads, 29 of 4.2 M samples of the full-size bidir_room test.
// 128 rounds were measured in round 4: 16 of 4.2 M still reach the cap (those beams restart behind empty apertures over and over — a longer
// loop is not what they lack) and the 32 more empty rounds per batch cost 2-4 % of a pass.  Kept at 96.
// Round 6: no walk is dropped at 96 any more.  kMaxWalkIters is what the device driver launches WITHOUT LOOKING at most (and what its per-round
// timing events are sized for); a batch whose round queue is not empty after that keeps getting rounds, eight at a time, until it is
// (wtgpu.hip: finish_look), and the checker's loops run to kWalkIterLimit — a bound against a walk that never ends, 43 x the old cap, counted
// like before if it is ever reached (walk_iteration_cap_hits; the full-size tests assert zero).
#ifndef WT_MAX_WALK_ITERS
#define WT_MAX_WALK_ITERS 96
#endif
constexpr uint32_t kMaxWalkIters = WT_MAX_WALK_ITERS;
constexpr uint32_t kWalkIterLimit = 4096;
constexpr uint32_t kMaxConeTris = 64;    // device cap of the cone query's triangle list
#ifdef WT_ORACLE_UNBOUNDED
constexpr uint32_t kMaxEdgeIds = 16384;  // CPU checker: effectively unbounded
#else
constexpr uint32_t kMaxEdgeIds = 96;     // cap of the de-duplicated edge set of one interaction region
#endif

enum vertex_type_e : uint32_t { VT_SENSOR = 0, VT_EMITTER = 1, VT_SURFACE = 2, VT_MEDIUM = 3, VT_FSD = 4 };
enum geo_kind_e : uint32_t { GEO_NONE = 0, GEO_POINT = 1, GEO_SURFACE = 2 };

struct vertex_t {
    uint32_t type;
    uint32_t transport;
    uint32_t delta;
    uint32_t fraunhofer_fsd;
    float pdf_fwd, pdf_bwd;
    float rr_weight;
    int32_t ref;          // emitter index (emitter vertex), material index (surface vertex)
    int32_t emitter_of_shape;   // surface vertex: emitter attached to the hit shape (-1 none)
    uint32_t fsd_slot;    // aperture pool slot (fsd vertex)
    uint32_t geo_kind;
    uint32_t has_beam;
    surface_t surf;       // GEO_POINT: only surf.wp is meaningful
    beam_t beam;          // beam arriving at this vertex
};
constexpr size_t kVertexWords = sizeof(vertex_t) / 4;
// A vertex without its beam (the first 43 of its 89 words) plus the beam's wavenumber: all that the densities of the MIS weights
// (vertex_t::pdf, vertex.hpp:444-487) read of a vertex.  Same member names as vertex_t, so the helpers below take either.
struct vertex_nb_t {
    uint32_t type;
    uint32_t transport;
    uint32_t delta;
    uint32_t fraunhofer_fsd;
    float pdf_fwd, pdf_bwd;
    float rr_weight;
    int32_t ref;
    int32_t emitter_of_shape;
    uint32_t fsd_slot;
    uint32_t geo_kind;
    uint32_t has_beam;
    surface_t surf;
    struct {
        float k;
    } beam;
};
static_assert(offsetof(vertex_nb_t, beam) == offsetof(vertex_t, beam) && offsetof(vertex_nb_t, surf) == offsetof(vertex_t, surf), "vertex_nb_t is a prefix of vertex_t");

// vertex store: vertex v of walk `idx` = words at base[idx*stride + v*kVertexWords + w] (stride = words of one walk's vertex array)
struct vertex_store_t {
    uint32_t* base;
    size_t stride;
    size_t idx;
    // Device, optional: the vertex a step appends is kept in `*stage` (its index in *staged_idx) instead of being written lane by lane — the
    // kernel writes the staged vertices of a wavefront afterwards, record by record with consecutive lanes on consecutive words (wtgpu_kernels.h:
    // wave_store_records).  Words stored into the staged vertex later (its rr_weight: walk_continue) go to the staged copy.
    vertex_t* stage = nullptr;
    uint32_t* staged_idx = nullptr;
    WT_HD void load(uint32_t v, vertex_t& out) const { soa_load(base + (size_t)v * kVertexWords, stride, idx, out); }
    // the beam-less part of a vertex (+ its wavenumber)
    WT_HD void load(uint32_t v, vertex_nb_t& out) const {
        const uint32_t* b = base + (size_t)v * kVertexWords + idx * stride;
        uint32_t* w = reinterpret_cast<uint32_t*>(&out);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (size_t i = 0; i < offsetof(vertex_t, beam) / 4; ++i) w[i] = b[i];
        out.beam.k = load_word<float>(v, (offsetof(vertex_t, beam) + offsetof(beam_t, k)) / 4);
    }
    WT_HD vec3 load_wp(uint32_t v) const {
        constexpr size_t o = (offsetof(vertex_t, surf) + offsetof(surface_t, wp)) / 4;
        return vec3{load_word<float>(v, o), load_word<float>(v, o + 1), load_word<float>(v, o + 2)};
    }
    WT_HD void store(uint32_t v, const vertex_t& in) const {
        if (stage) {
            *stage = in;
            *staged_idx = v;
            return;
        }
        soa_store(base + (size_t)v * kVertexWords, stride, idx, in);
    }
    template <class F>
    WT_HD void store_word(uint32_t v, size_t word, F value) const {
        static_assert(sizeof(F) == 4, "");
        uint32_t w;
        __builtin_memcpy(&w, &value, 4);
        if (stage && *staged_idx == v) {
            reinterpret_cast<uint32_t*>(stage)[word] = w;
            return;
        }
        base[idx * stride + (size_t)v * kVertexWords + word] = w;
    }
    template <class F>
    WT_HD F load_word(uint32_t v, size_t word) const {
        const uint32_t w = base[idx * stride + (size_t)v * kVertexWords + word];
        F f;
        __builtin_memcpy(&f, &w, 4);
        return f;
    }
};
#define WT_VWORD(field) (offsetof(vertex_t, field) / 4)

struct fsd_pool_t {
    fsd_aperture_t* hdr;
    fsd_edge_t* edges;     // segment records of all apertures (every aperture owns the range its header names)
    uint32_t* counter;     // bump allocator of aperture slots
    uint32_t cap;
    uint32_t* edge_counter;   // bump allocator of segment records (nullptr: every slot owns kFsdMaxEdges records — CPU checker)
    uint32_t edge_cap;
};
WT_HD fsd_edges_ref_t fsd_pool_edges(const fsd_pool_t& p, uint32_t slot) {
    return fsd_edges_ref_t{p.edges + (size_t)p.hdr[slot].edge_offset, 1};
}
// storage for an aperture of up to `need` segments; FALSE: the segment pool is exhausted
WT_HD bool fsd_pool_alloc_edges(const fsd_pool_t& p, uint32_t slot, uint32_t need, fsd_aperture_t& ap) {
    if (!p.edge_counter) {
        ap.edge_offset = slot * kFsdMaxEdges;
        ap.edge_cap = kFsdMaxEdges;
        return true;
    }
    if (need > kFsdMaxEdges) need = kFsdMaxEdges;
    uint32_t off = 0;
    if (need) {
#if defined(__HIP_DEVICE_COMPILE__)
        off = atomicAdd(p.edge_counter, need);
#else
        off = __atomic_fetch_add(p.edge_counter, need, __ATOMIC_RELAXED);
#endif
    }
    ap.edge_offset = off;
    ap.edge_cap = need;
    if ((size_t)off + need > p.edge_cap) {
        ap.edge_offset = 0;
        ap.edge_cap = 0;
        return false;
    }
    return true;
}
WT_HD uint32_t fsd_pool_alloc(const fsd_pool_t& p) {
#if defined(__HIP_DEVICE_COMPILE__)
    // one atomic per wavefront: the lanes that allocate together (the active lanes of this divergent branch) share it
    const unsigned long long m = __ballot(1);
    const int lane = (int)(threadIdx.x & 63u);
    const int leader = __ffsll((long long)m) - 1;
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(p.counter, (uint32_t)__popcll(m));
    base = (uint32_t)__shfl((int)base, leader, 64);
    return base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
#else
    return __atomic_fetch_add(p.counter, 1u, __ATOMIC_RELAXED);
#endif
}

// ---- vertex helpers (vertex.hpp) --------------------------------------------------------------------
template <class V>
WT_HD vec3 vertex_wp(const V& v) { return v.surf.wp; }
template <class V>
WT_HD bool vertex_is_on_surface(const scene_t& sc, const V& v) {
    return v.type == VT_SURFACE || (v.type == VT_EMITTER && emitter_is_area(sc.emitters[v.ref])) ||
           (v.type == VT_SENSOR && v.geo_kind == GEO_SURFACE);
}
template <class V>
WT_HD bool vertex_has_real_surface(const scene_t& sc, const V& v) {
    return v.type == VT_SURFACE || (v.type == VT_EMITTER && emitter_is_area(sc.emitters[v.ref]));
}
// ng()/ns(): sensors report (0,0,1) (vertex.hpp:271-287)
template <class V>
WT_HD vec3 vertex_ng(const scene_t& sc, const V& v) { return vertex_has_real_surface(sc, v) ? v.surf.geo.n : vec3{0, 0, 1}; }
template <class V>
WT_HD vec3 vertex_ns(const scene_t& sc, const V& v) { return vertex_has_real_surface(sc, v) ? v.surf.shading.n : vec3{0, 0, 1}; }
WT_HD bool vertex_is_interaction(const vertex_t& v) { return v.type == VT_FSD || v.type == VT_SURFACE || v.type == VT_MEDIUM; }
WT_HD bool vertex_on_emitter(const vertex_t& v) { return v.type == VT_EMITTER || (v.type == VT_SURFACE && v.emitter_of_shape >= 0); }
template <class V>
WT_HD int vertex_get_emitter(const V& v) { return v.type == VT_EMITTER ? v.ref : v.emitter_of_shape; }
template <class V>
WT_HD bool vertex_is_delta_emitter(const scene_t& sc, const V& v) {
    return v.type == VT_EMITTER && (emitter_is_delta_direction(sc.emitters[v.ref]) || emitter_is_delta_position(sc.emitters[v.ref]));
}
template <class V>
WT_HD bool vertex_is_delta_sensor(const scene_t& sc, const V& v) {
    return v.type == VT_SENSOR && (sensor_is_delta_direction(sc.sensor) || sensor_is_delta_position(sc.sensor));
}
WT_HD bool vertex_is_connectible(const scene_t& sc, const vertex_t& v) {
    switch (v.type) {
    case VT_FSD: return true;
    case VT_EMITTER: return !emitter_is_delta_direction(sc.emitters[v.ref]);
    case VT_SENSOR: return !sensor_is_delta_direction(sc.sensor);
    case VT_SURFACE: return !material_is_delta_only(sc, v.ref, v.beam.k);
    default: return false;
    }
}
WT_HD vec3 geo_offseted_ray_origin(const scene_t& sc, const vertex_t& v, vec3 ro, vec3 rd) {
    return v.geo_kind == GEO_SURFACE ? surface_offseted_ray_origin(sc, v.surf, ro, rd) : ro;
}

// convert_directional_density_to_area (vertex.hpp:224-243)
template <class V>
WT_HD float convert_directional_density_to_area(const scene_t& sc, float dpdf_tagged, vec3 p, const V& next) {
    const float dens = pd_density_or_zero(dpdf_tagged);
    if (dens == 0.f) return 0.f;
    const vec3 d = vertex_wp(next) - p;
    const float d2 = length2(d);
    if (d2 == 0.f) return WT_INF;
    float ppdf = dens * (1.f / d2);
    if (vertex_is_on_surface(sc, next)) ppdf *= fabsf(dot(vertex_ng(sc, next), normalize(d)));
    return ppdf;
}
template <class V, class N>
WT_HD float vertex_pdf_next_from_sensor(const scene_t& sc, const V& v, const N& next) {
    const vec3 dl = vertex_wp(next) - vertex_wp(v);
    const float recp_dist2 = 1.f / length2(dl);
    const vec3 d = dl * sqrtf(recp_dist2);
    const float dpdf = pd_density_or_zero(sensor_pdf_direction(sc, d));
    float ppdf = dpdf * recp_dist2;
    if (vertex_is_on_surface(sc, next)) ppdf *= fabsf(dot(vertex_ng(sc, next), d));
    return ppdf;
}
WT_HD float vertex_pdf_sensor(const scene_t& sc) { return pd_density_or_zero(sensor_pdf_position(sc)); }
template <class V, class N>
WT_HD float vertex_pdf_next_from_emitter(const scene_t& sc, const V& v, const N& next) {
    const vec3 dl = vertex_wp(next) - vertex_wp(v);
    const float recp_dist2 = 1.f / length2(dl);
    const vec3 d = dl * sqrtf(recp_dist2);
    const int ei = vertex_get_emitter(v);
    if (emitter_is_infinite(sc.emitters[ei])) return directional_pdf_target_position(sc.emitters[ei], vertex_wp(next));   // vertex.hpp:532-536
    const float dpdf = pd_density_or_zero(emitter_pdf_direction(sc, ei, d, vertex_has_real_surface(sc, v) ? &v.surf : nullptr));
    float ppdf = dpdf * recp_dist2;
    if (vertex_is_on_surface(sc, next)) ppdf *= fabsf(dot(vertex_ng(sc, next), d));
    return ppdf;
}
template <class V>
WT_HD float vertex_pdf_emitter(const scene_t& sc, const V& v) {
    const int ei = vertex_get_emitter(v);
    return sc.emitters[ei].select_pmf * pd_density_or_zero(emitter_pdf_position(sc, ei, vertex_has_real_surface(sc, v) ? &v.surf : nullptr));
}
// vertex_t::pdf (vertex.hpp:444-487); of `prev` only the position matters
template <class V, class N>
WT_HD float vertex_pdf(const scene_t& sc, const fsd_pool_t& pool, const V& v, vec3 prev_wp, const N& next, uint32_t mode) {
    if (v.type == VT_EMITTER) return vertex_pdf_next_from_emitter(sc, v, next);
    if (v.type == VT_SENSOR) return vertex_pdf_next_from_sensor(sc, v, next);
    const vec3 p = vertex_wp(v);
    const vec3 wiworld = normalize(prev_wp - p);
    const vec3 woworld = normalize(vertex_wp(next) - p);
    float pdf = 0.f;
    if (v.type == VT_SURFACE) {
        const vec3 wi = to_local(v.surf.shading, wiworld), wo = to_local(v.surf.shading, woworld);
        pdf = material_pdf(sc, v.ref, wi, wo, v.beam.k, mode, v.surf.uv);
    } else if (v.type == VT_FSD) {
        const fsd_aperture_t ap = pool.hdr[v.fsd_slot];
        pdf = fsd_pdf(ap, fsd_pool_edges(pool, v.fsd_slot), to_local(ap.frame, woworld));
    }
    return convert_directional_density_to_area(sc, pdf, p, next);
}

// vertex_t::interact (vertex.hpp:330-413): beam arriving at `v` transformed towards `next`.
// (of `next` only its position matters)
WT_HD bool vertex_interact(const scene_t& sc, const fsd_pool_t& pool, const vertex_t& v, vec3 next_wp, bool ignore_fsd, beam_t& out) {
    const vec3 wiworld = -v.beam.env.d;
    const float k = v.beam.k;
    float f = 0.f;
    if (v.fraunhofer_fsd && !ignore_fsd) {
        const fsd_aperture_t ap = pool.hdr[v.fsd_slot];
        const vec3 woworld = normalize(next_wp - vertex_wp(v));
        f = fsd_pdf(ap, fsd_pool_edges(pool, v.fsd_slot), to_local(ap.frame, woworld));
    }
    if (v.type == VT_SURFACE) {
        const surface_t& srf = v.surf;
        const vec3 woworld = normalize(next_wp - vertex_wp(v));
        const vec3 wi = to_local(srf.shading, wiworld), wo = to_local(srf.shading, woworld);
        const vec3 ng = srf.geo.n, ns = srf.shading.n;
        const float wig = dot(wiworld, ng), wog = dot(woworld, ng);
        const float wis = wi.z, wos = wo.z;
        if (wig * wis <= 0.f || wog * wos <= 0.f) return false;
        mueller_t M = material_f(sc, v.ref, wi, wo, k, v.transport, v.surf.uv);
        float scale = 1.f / fabsf(wos);
        if (!veq(ns, ng)) scale *= shading_normals_correction_scale(v.transport, wig, wog, wis, wos);
        M = M * scale;
        if (f > 0.f) M = M + mueller_identity() * f;
        if (mueller_mean_intensity(M) == 0.f) return false;
        out = v.beam;
        beam_transform_surface_interaction(out, srf, woworld, M, 1.f);
        return true;
    }
    if (v.type == VT_FSD) {
        const vec3 p = vertex_wp(v);
        const float beam_dist = dot(p - v.beam.env.o, v.beam.env.d);
        const vec3 woworld = normalize(next_wp - p);
        out = v.beam;
        beam_transform_region_interaction(out, p, beam_dist, woworld, f);
        return true;
    }
    return false;
}

// integrator::shadow (traversal.hpp:319-333).  What the ray between two path vertices needs of them: position and, for a vertex on a
// surface, the triangle and geometric normal of its self-intersection offset (intersection.cpp:148-185).
struct conn_end_t {
    vec3 wp, ng;
    uint32_t geo_kind, tuid;
};
template <class V>
WT_HD conn_end_t conn_end_of(const V& v) { return conn_end_t{v.surf.wp, v.surf.geo.n, v.geo_kind, v.surf.tuid}; }
WT_HD vec3 conn_end_offseted_origin(const scene_t& sc, const conn_end_t& e, vec3 ro, vec3 rd) {   // (geo_offseted_ray_origin / surface_offseted_ray_origin)
    if (e.geo_kind != GEO_SURFACE || e.tuid == kInvalid) return ro;
    const tri_geo_t g = sc.tri_geo[e.tuid];
    const vec3 err = triangle_fp_errors(g.a, g.b, g.c, ro);
    const float offset_dist = dot(err, vabs(e.ng));
    const vec3 offset = offset_dist * e.ng;
    return ro + (dot(rd, offset) >= 0.f ? offset : -offset);
}
struct shadow_ray_t {
    vec3 o, d;
    float dist;
};
WT_HD shadow_ray_t conn_shadow_ray(const scene_t& sc, const conn_end_t& a, const conn_end_t& b) {
    const vec3 rd = normalize(b.wp - a.wp);
    const vec3 o = conn_end_offseted_origin(sc, a, a.wp, rd);
    const vec3 t = conn_end_offseted_origin(sc, b, b.wp, -rd);
    const float dist = length(t - o);
    return shadow_ray_t{o, (t - o) / dist, dist};
}
// TRUE if occluded
WT_HD bool bdpt_shadow(const scene_t& sc, const vertex_t& a, const vertex_t& b, const stack_ref_t& stack, bvh_counters_t* ctr) {
    const shadow_ray_t r = conn_shadow_ray(sc, conn_end_of(a), conn_end_of(b));
    return ads_shadow_ray(sc, r.o, r.d, range_t{0.f, r.dist}, stack, ctr);
}

// ---- walk state -----------------------------------------------------------------------------------------
struct walk_t {
    beam_t beam;
    float pdf_from_prev;   // tagged solid-angle pd of sampling the next vertex from the last one
    float throughput, rr_weight;
    uint32_t nverts;
    uint32_t active;
    uint32_t rng_draws;
    // cached data of the last vertex (vertices.back())
    vec3 prev_wp, prev_ng;
    uint32_t prev_on_surface;
    uint32_t prev_offset_tuid;   // triangle used for the self-intersection offset (kInvalid: none)
};

#define WT_WALK_NVERTS_WORD (offsetof(walk_t, nverts) / 4)

struct sample_ctx_t {
    float k;
    float recp_spectral_pd;
    float k_density;
    sensor_element_t element;
};

struct bdpt_counters_t {
    unsigned long long segments, ray_queries, cone_queries, vertices, connections, shadow_rays;
    unsigned long long cone_tri_overflow, edge_overflow, fsd_edge_overflow, fsd_pool_overflow, fsd_interactions, null_interactions;
    unsigned long long surface_interactions, light_splats;
};

WT_HD void walk_cache_prev(const scene_t& sc, walk_t& w, const vertex_t& v) {
    w.prev_wp = vertex_wp(v);
    w.prev_ng = vertex_ng(sc, v);
    w.prev_on_surface = vertex_is_on_surface(sc, v);
    w.prev_offset_tuid = v.geo_kind == GEO_SURFACE ? v.surf.tuid : kInvalid;
}

// plt_bdpt.cpp:54-87 + generate_{sensor,emitter}_subpath: draws the spectral/emitter/sensor samples and creates
// vertex 0 of both subpaths.
WT_HD void bdpt_generate(const scene_t& sc, uint64_t seed, uint64_t sample_id, uint32_t px, uint32_t py, sample_ctx_t& ctx, walk_t& sw, walk_t& ew,
                         const vertex_store_t& svs, const vertex_store_t& evs) {
    sampler_t smp = make_sampler(seed, sample_id, STREAM_SCENE);
    const emitter_k_sample_t ek = scene_sample_emitter_and_spectrum(sc, smp);
    const float k = ek.wavenumber.k;
    const emitter_sample_t es = emitter_sample(sc, ek.emitter, k, smp);
    const bool disc = pd_is_discrete(ek.wavenumber.wpd);
    ctx.k = k;
    ctx.recp_spectral_pd = disc ? 1.f / pd_mass(ek.wavenumber.wpd) : 1.f / scene_sum_spectral_pdf(sc, k);
    ctx.k_density = disc ? pd_mass(ek.wavenumber.wpd) : ek.wavenumber.wpd;
    const sensor_sample_t ss = sensor_sample(sc, px, py, k, smp);
    ctx.element = ss.element;

    vertex_t v;
    // create_sensor (vertex.hpp:77-88)
    v.type = VT_SENSOR;
    v.transport = TRANSPORT_BACKWARD;
    v.delta = 0;
    v.fraunhofer_fsd = 0;
    v.pdf_fwd = -1.f;
    v.pdf_bwd = pd_density_or_zero(ss.ppd);
    v.rr_weight = 1.f;
    v.ref = -1;
    v.emitter_of_shape = -1;
    v.fsd_slot = kInvalid;
    v.has_beam = 1;
    v.beam = ss.beam;
    if (ss.has_surface) {
        v.geo_kind = GEO_SURFACE;
        v.surf = ss.surface;
    } else {
        v.geo_kind = GEO_POINT;
        v.surf = make_dummy_surface(vec3{0, 0, 1}, ss.beam.env.o);
    }
    svs.store(0, v);
    sw.beam = ss.beam;
    sw.pdf_from_prev = ss.dpd;
    sw.throughput = 1.f;
    sw.rr_weight = 1.f;
    sw.nverts = 1;
    sw.active = 1;
    sw.rng_draws = 0;
    walk_cache_prev(sc, sw, v);

    // create_emitter (vertex.hpp:111-121)
    v.type = VT_EMITTER;
    v.transport = TRANSPORT_FORWARD;
    v.pdf_fwd = pd_density_or_zero(es.ppd) * ek.emitter_pdf;
    v.pdf_bwd = -1.f;
    v.ref = ek.emitter;
    v.beam = es.beam;
    if (es.has_surface) {
        v.geo_kind = GEO_SURFACE;
        v.surf = es.surface;
    } else {
        v.geo_kind = GEO_POINT;
        v.surf = make_dummy_surface(vec3{0, 0, 1}, es.beam.env.o);
    }
    evs.store(0, v);
    ew.beam = es.beam;
    ew.pdf_from_prev = es.dpd;
    ew.throughput = 1.f;
    ew.rr_weight = 1.f;
    ew.nverts = 1;
    ew.active = 1;
    ew.rng_draws = 0;
    walk_cache_prev(sc, ew, v);
}

// The part of walk_t the trace kernels need (19 of its 57 words), loaded field by field straight into registers.
struct walk_trace_in_t {
    cone_t env;
    float k;
    vec3 prev_ng;
    uint32_t prev_offset_tuid;
};
template <class F>
WT_HD F soa_word(const uint32_t* base, size_t stride, size_t idx, size_t word) {
    static_assert(sizeof(F) == 4, "");
    const uint32_t w = base[idx * stride + word];
    F f;
    __builtin_memcpy(&f, &w, 4);
    return f;
}
#define WT_WALK_WORD(field) (offsetof(walk_t, field) / 4)
WT_HD walk_trace_in_t walk_load_trace_in(const uint32_t* base, size_t stride, size_t idx) {
    walk_trace_in_t r;
    r.env.o = {soa_word<float>(base, stride, idx, WT_WALK_WORD(beam.env.o.x)), soa_word<float>(base, stride, idx, WT_WALK_WORD(beam.env.o.y)),
               soa_word<float>(base, stride, idx, WT_WALK_WORD(beam.env.o.z))};
    r.env.d = {soa_word<float>(base, stride, idx, WT_WALK_WORD(beam.env.d.x)), soa_word<float>(base, stride, idx, WT_WALK_WORD(beam.env.d.y)),
               soa_word<float>(base, stride, idx, WT_WALK_WORD(beam.env.d.z))};
    r.env.x = {soa_word<float>(base, stride, idx, WT_WALK_WORD(beam.env.x.x)), soa_word<float>(base, stride, idx, WT_WALK_WORD(beam.env.x.y)),
               soa_word<float>(base, stride, idx, WT_WALK_WORD(beam.env.x.z))};
    r.env.x0 = soa_word<float>(base, stride, idx, WT_WALK_WORD(beam.env.x0));
    r.env.tan_alpha = soa_word<float>(base, stride, idx, WT_WALK_WORD(beam.env.tan_alpha));
    r.env.e = soa_word<float>(base, stride, idx, WT_WALK_WORD(beam.env.e));
    r.env.one_over_e = soa_word<float>(base, stride, idx, WT_WALK_WORD(beam.env.one_over_e));
    r.env.z_apex = soa_word<float>(base, stride, idx, WT_WALK_WORD(beam.env.z_apex));
    r.k = soa_word<float>(base, stride, idx, WT_WALK_WORD(beam.k));
    r.prev_ng = {soa_word<float>(base, stride, idx, WT_WALK_WORD(prev_ng.x)), soa_word<float>(base, stride, idx, WT_WALK_WORD(prev_ng.y)),
                 soa_word<float>(base, stride, idx, WT_WALK_WORD(prev_ng.z))};
    r.prev_offset_tuid = soa_word<uint32_t>(base, stride, idx, WT_WALK_WORD(prev_offset_tuid));
    return r;
}
WT_HD cone_t walk_trace_envelope(const scene_t& sc, const walk_trace_in_t& w) {
    cone_t env = w.env;
    if (w.prev_offset_tuid != kInvalid) {
        const tri_geo_t g = sc.tri_geo[w.prev_offset_tuid];
        const vec3 err = triangle_fp_errors(g.a, g.b, g.c, env.o);
        const float offset_dist = dot(err, vabs(w.prev_ng));
        const vec3 offset = offset_dist * w.prev_ng;
        env.o = env.o + (dot(env.d, offset) >= 0.f ? offset : -offset);
    }
    return env;
}

// envelope used for tracing the next segment (traversal.hpp:276-288): origin offset away from the last surface
WT_HD cone_t walk_trace_envelope(const scene_t& sc, const walk_t& w) {
    cone_t env = w.beam.env;
    if (w.prev_offset_tuid != kInvalid) {
        const tri_geo_t g = sc.tri_geo[w.prev_offset_tuid];
        const vec3 err = triangle_fp_errors(g.a, g.b, g.c, env.o);
        const float offset_dist = dot(err, vabs(w.prev_ng));
        const vec3 offset = offset_dist * w.prev_ng;
        env.o = env.o + (dot(env.d, offset) >= 0.f ? offset : -offset);
    }
    return env;
}

// bdpt_walk_data_t::append_vertex (plt_bdpt_detail.hpp:95-121)
WT_HD bool walk_append_vertex(const scene_t& sc, walk_t& w, const vertex_store_t& vs, vertex_t& v, float pdf_fwd, float pdf_revr) {
    if (veq(w.prev_wp, vertex_wp(v))) return false;
    // pdf of sampling v from the previous vertex
    const float pv = convert_directional_density_to_area(sc, w.pdf_from_prev, w.prev_wp, v);
    if (v.transport == TRANSPORT_FORWARD)
        v.pdf_fwd = pv;
    else
        v.pdf_bwd = pv;
    v.beam = w.beam;
    v.has_beam = 1;
    // reversed pdf of the previous vertex (sampling prev from v)
    {
        const float dens = pd_density_or_zero(pdf_revr);
        float prev_rev = 0.f;
        if (dens != 0.f) {
            const vec3 d = w.prev_wp - vertex_wp(v);
            const float d2 = length2(d);
            if (d2 == 0.f)
                prev_rev = WT_INF;
            else {
                prev_rev = dens * (1.f / d2);
                if (w.prev_on_surface) prev_rev *= fabsf(dot(w.prev_ng, normalize(d)));
            }
        }
        // pdf_reversed(): backward transport -> pdf_fwd, forward -> pdf_bwd
        vs.store_word(w.nverts - 1, v.transport == TRANSPORT_BACKWARD ? WT_VWORD(pdf_fwd) : WT_VWORD(pdf_bwd), prev_rev);
    }
    w.pdf_from_prev = pdf_fwd;
    vs.store(w.nverts, v);
    w.nverts++;
    walk_cache_prev(sc, w, v);
    return true;
}

// continue_walk (plt_bdpt_detail.hpp:167-182)
WT_HD bool walk_continue(const scene_t& sc, walk_t& w, const vertex_store_t& vs, bool allow_RR, sampler_t& smp) {
    if ((int)w.nverts > sc.opts.max_depth + 1) return false;
    if (!allow_RR || !sc.opts.RR) return true;
    vs.store_word(w.nverts - 1, WT_VWORD(rr_weight), w.rr_weight);
    const float r = w.throughput < 1.f ? fmaxf_(w.throughput, .5f) : 1.f;
    if (sampler_r(smp) <= r) {
        const float scale = 1.f / r;
        w.rr_weight *= scale;
        w.throughput *= scale;
        return true;
    }
    return false;
}

// Power of the beam's wavefront that one triangle of the interaction region intercepts (find_closest_triangle,
// plt_bdpt_detail.hpp:391-416): clipped to the region's z-slab, projected to the cross-section at its centre, Gaussian integral.
WT_HD float region_triangle_flux(const scene_t& sc, const frame_t& beam_frame, const cone_t& envelope, const range_t& izr, vec2 sigma, uint32_t tuid,
                                 bool want_front) {
    const tri_geo_t g = sc.tri_geo[tuid];
    const bool front_face = dot(g.n, -envelope.d) > 0.f;
    if (front_face != want_front) return 0.f;
    return region_local_triangle_flux(envelope, izr, centre(izr), sigma, to_local(beam_frame, g.a - envelope.o), to_local(beam_frame, g.b - envelope.o),
                                      to_local(beam_frame, g.c - envelope.o));
}

// One random-walk step after the beam has been traced (plt_bdpt_detail.hpp:421-526 minus the traverse() call).
// Hand-over record of a Fraunhofer-FSD rejection loop that a device lane could not finish within kFsdInlineTries (fsd.h):
// pending = the step returned early, nothing committed; resolved = the wavefront found the outcome, re-run the step with it.
struct fsd_defer_t {
    uint32_t split_no_primary, no_primary;   // in: defer walks without a primary triangle; out: this walk is one
    uint32_t known_no_primary;               // in: the first pass already found no primary triangle (skip the search)
    // in: a wavefront already walked an interaction region too large for the bounded triangle list (coop_gather, coop.h):
    // intercepted power fraction and the sorted classified-edge set of the WHOLE region
    uint32_t has_gather, gather_n_edges, gather_edge_overflow;
    float gather_flux;
    const uint32_t* gather_edges;
    // in (pass B): do not sample apertures that turn out to have edges, hand the walk to the sampling pass; out: this walk is one
    // (its aperture is in pool slot `slot`).  in (pass C): the aperture of this walk exists already in `slot`
    uint32_t defer_sampling, to_sampling_pass, have_aperture;
    uint32_t pending, resolved;
    uint32_t slot, base, next_try, end_draws;
    fsd_sample_t fs;
#ifdef WTGPU_STEP_PROF
    long long marks[8];
#endif
};
// Nothing asked of the step and nothing handed to it (`fs` is written by whoever resolves the loop): what every kernel starts its record from.
WT_HD fsd_defer_t fsd_defer_none() {
    fsd_defer_t d;
    d.pending = d.resolved = 0;
    d.slot = d.base = d.next_try = d.end_draws = 0;
    d.defer_sampling = d.to_sampling_pass = d.have_aperture = 0;
    d.split_no_primary = d.known_no_primary = d.no_primary = 0;
    d.has_gather = d.gather_n_edges = d.gather_edge_overflow = 0;
    d.gather_flux = 0.f;
    d.gather_edges = nullptr;
    return d;
}
// What a rejection loop that ran outside the step found: the lowest accepted try, its point and scattering function — or no accepted try.
struct fsd_outcome_t {
    uint32_t acc, t_acc;
    vec2 x;
    float f;
};
// The record of a walk whose loop over aperture `ap` (pool slot `slot`, tries keyed from draw `base`) ended with `o`: no primary triangle, the
// aperture exists, the sample is final.  Without an accepted try the walk's stream moves past the last try (max_tries = 0 wraps to `base`).
WT_HD fsd_defer_t fsd_defer_resolved(const fsd_aperture_t& ap, uint32_t slot, uint32_t base, uint32_t max_tries, const fsd_outcome_t& o) {
    fsd_defer_t d = fsd_defer_none();
    d.known_no_primary = d.have_aperture = d.resolved = 1;
    d.slot = slot;
    d.base = base;
    d.fs = fsd_finalize(ap, o.acc != 0u, o.x, o.f);
    d.end_draws = fsd_draws_after(base, o.acc ? o.t_acc : max_tries - 1u);
    return d;
}

#if defined(WTGPU_STEP_PROF) && defined(__HIP_DEVICE_COMPILE__)
#define WT_STEP_MARK(i) \
    if (defer) defer->marks[i] = clock64()   // profiling hook of debug builds (-DWTGPU_STEP_PROF)
#else
#define WT_STEP_MARK(i) ((void)0)
#endif
// Returns TRUE if the walk continues (another segment must be traced).
// MODE 0: everything (CPU checker).  Device: MODE 1 compiles only the surface-interaction branch (k_interact; walks without a
// primary triangle leave through `defer`), MODE 2 only the no-primary branch (k_interact_b) — smaller kernels, smaller frames.
template <int MODE = 0, class TriList>
WT_HD bool bdpt_walk_step(const scene_t& sc, walk_t& w, const trav_result_t& tr, const TriList& tris, const vertex_store_t& vs,
                          const fsd_pool_t& pool, uint64_t seed, uint64_t sample_id, uint32_t stream, bdpt_counters_t* ctr,
                          const stack_ref_t* primary_query_stack = nullptr, fsd_defer_t* defer = nullptr) {
    if (tr.empty) return false;   // no intersection (TODO in the reference: infinite emitters)
    sampler_t smp = make_sampler(seed, sample_id, stream, w.rng_draws);
    beam_t& beam = w.beam;
    const float beam_dist = tr.dist;
    const range_t izr{beam_dist, beam_dist + tr.region_depth};
    const bool is_ballistic = tr.ballistic || beam_is_ray(beam);
    const vec3 origin_wp = tr.origin;
    const vec3 interaction_wp = origin_wp + izr.min * beam.env.d;
    const frame_t beam_frame = cone_frame(beam.env);
    const cone_t envelope = beam.env;
    const vec3 sd3 = beam_footprint(beam, beam_dist) / kBeamEnvelope;   // std_dev
    const vec2 sigma{sd3.x, sd3.y};

    // primary triangle
    uint32_t primary = kInvalid;
    ray_tri_hit_t phit{WT_INF, 0.f, 0.f};
    // summed in f64 (the reference sums in f32, plt_bdpt_detail.hpp:391-416): a beam over a dense mesh is almost entirely blocked, 1 - flux
    // is small, and the f32 rounding of a sum of 10^3..10^4 terms (~1e-4) decides 1/I; an accurate sum is at least order-independent
    double integrated_flux = 0.0;
    if (is_ballistic) {
        primary = tr.tuid;
        phit.dist = tr.dist;
        phit.bx = tr.bx;
        phit.by = tr.by;
    } else {
        // find_closest_triangle (plt_bdpt_detail.hpp:362-419).
        // Device variant (primary_query_stack != nullptr): the cone query's triangle list is bounded on the device
        // (kMaxConeTris) while the reference's is an unbounded std::vector; the triangle under the beam axis is therefore
        // found with a BVH *ray* query over the same z-slab instead of scanning the list.  Whenever the list is complete both
        // select the same triangle (closest axis hit inside the slab); the CPU checker keeps the reference's list scan.
        // The BVH query is only needed when the list was actually truncated (tr.overflow > 0, a few per cent of the segments);
        // a complete list is scanned like the reference does (a handful of ray-triangle tests instead of a tree traversal).
        if (defer && defer->known_no_primary) {
            // second pass of a walk the first pass found no primary triangle for
        } else if (tr.aborted == 2) {
            // device: the trace kernels resolved the primary of this overflowed region already (g8.h: g8_resolve_primary)
            if (tr.tuid != kInvalid) {
                primary = tr.tuid;
                phit.dist = tr.pdist;
                phit.bx = tr.bx;
                phit.by = tr.by;
            }
        } else if (primary_query_stack && tr.overflow > 0) {
            const float wtol = cone_intersection_tolerance(origin_wp, sc.world_min, sc.world_max, sc.world_max);
            ray_hit_t rh;
            if (ads_intersect_ray(sc, origin_wp, beam.env.d, grow(izr, wtol), *primary_query_stack, rh)) {
                const tri_geo_t g = sc.tri_geo[rh.tuid];
                const float fptol = cone_intersection_tolerance(origin_wp, g.a, g.b, g.c);
                if (contains(grow(izr, fptol), rh.dist)) {
                    primary = rh.tuid;
                    phit.dist = rh.dist;
                    phit.bx = rh.bx;
                    phit.by = rh.by;
                }
            }
        } else
        for (uint32_t i = 0; i < tr.ntris; ++i) {
            const uint32_t tuid = tris[i];
            const tri_geo_t g = sc.tri_geo[tuid];
            const float fptol = cone_intersection_tolerance(origin_wp, g.a, g.b, g.c);
            ray_tri_hit_t h;
            if (intersect_ray_tri(origin_wp, beam.env.d, g.a, g.b, g.c, grow(izr, fptol), h) && h.dist < phit.dist) {
                primary = tuid;
                phit = h;
            }
        }
        // Device, first pass (k_interact): the beam axis misses every listed triangle — what follows (footprint integrals over
        // the whole list, edge gathering, aperture construction, FSD sampling) costs ~50x a surface interaction and concerns
        // ~8 % of the walks; those are handed to a second pass (k_interact_b) so that they do not stall the other 63 lanes.
        if (primary == kInvalid && defer && defer->split_no_primary) {
            defer->no_primary = 1;
            return false;   // nothing has been committed
        }
        WT_STEP_MARK(0);
    }

    bool do_RR = true;
    bool ok = true;
    bool took_surface = false;
    if constexpr (MODE != 2) {
    if (primary != kInvalid) {
        took_surface = true;
        // ---- sample_surface_interaction (plt_bdpt_detail.hpp:192-270)
        const tri_geo_t g = sc.tri_geo[primary];
        const vec3 sampled_tri_wp = origin_wp + envelope.d * phit.dist;
        surface_t srf = make_surface(sc, primary, g.n, vec2{phit.bx, phit.by}, sampled_tri_wp);
        srf.footprint = beam_surface_footprint_static(beam, srf, beam_dist);
        const shape_t shp = sc.shapes[srf.shape];
        const float k = beam.k;
        const uint32_t transport = beam.transport;
        const vec3 ng = srf.geo.n, ns = srf.shading.n;
        const vec3 wiworld = -beam.env.d;
        const vec3 wi = to_local(srf.shading, wiworld);
        const float wig = dot(wiworld, ng), wis = wi.z;
        ok = wig * wis > 0.f;
        bsdf_sample_t bs;
        if (ok) {
            bs = material_sample(sc, shp.material, wi, k, transport, smp, srf.uv);
            ok = bs.valid && bs.dpd != 0.f;
        }
        if (ok) {
            const bool is_delta = pd_is_discrete(bs.dpd);
            const vec3 wo = bs.wo;
            const vec3 woworld = normalize(to_world(srf.shading, wo));
            const float wog = dot(woworld, ng), wos = wo.z;
            if (ctr) ctr->surface_interactions++;
            ok = wog * wos > 0.f;
            if (ok) {
                const float pdf_revr = material_pdf(sc, shp.material, wo, wi, k, flip_transport(transport), srf.uv);
                vertex_t v;
                v.type = VT_SURFACE;
                v.transport = transport;
                v.delta = is_delta;
                v.fraunhofer_fsd = 0;
                v.pdf_fwd = v.pdf_bwd = -1.f;
                v.rr_weight = 1.f;
                v.ref = shp.material;
                v.emitter_of_shape = shp.emitter;
                v.fsd_slot = kInvalid;
                v.geo_kind = GEO_SURFACE;
                v.surf = srf;
                ok = walk_append_vertex(sc, w, vs, v, bs.dpd, pdf_revr);
                if (ok) {
                    if (ctr) ctr->vertices++;
                    float ws = 1.f;
                    if (!veq(ns, ng)) ws *= shading_normals_correction_scale(transport, wig, wog, wis, wos);
                    // transform_surface_interaction (plt_bdpt_detail.hpp:123-136)
                    beam_transform_surface_interaction(beam, srf, woworld, bs.M, ws);
                    w.throughput *= ws * mueller_mean_intensity(bs.M);
                    if (transport == TRANSPORT_BACKWARD && bs.eta != 1.f) w.throughput /= sqr(bs.eta);
                }
            }
        }
    }
    }
    if constexpr (MODE != 1) {
    if (!took_surface) {
        WT_STEP_MARK(1);
        // gather the ordered, de-duplicated edge set of the interaction region (traversal_common.hpp:124-148)
        uint32_t edge_ids[kMaxEdgeIds];
        const uint32_t* eids = edge_ids;
        uint32_t n_edge_ids = 0;
        const bool have_ap = defer && (defer->resolved || defer->have_aperture);   // built by an earlier execution of this step
        if (have_ap) {
            n_edge_ids = 1;
        } else if (sc.opts.FSD && !is_ballistic && defer && defer->has_gather) {
            // device: the sorted edge set of the WHOLE region, gathered by a wavefront (any length: used in place)
            n_edge_ids = defer->gather_n_edges;
            eids = defer->gather_edges;
            if (ctr) ctr->edge_overflow += defer->gather_edge_overflow;
        } else if (sc.opts.FSD && !is_ballistic) {
            for (uint32_t i = 0; i < tr.ntris; ++i) {
                const tri_meta_t m = sc.tri_meta[tris[i]];
                for (int e = 0; e < 3; ++e) {
                    const uint32_t id = m.edge[e];
                    if (id == kInvalid) continue;
                    uint32_t pos = 0;
                    while (pos < n_edge_ids && edge_ids[pos] < id) ++pos;
                    if (pos < n_edge_ids && edge_ids[pos] == id) continue;
                    if (n_edge_ids == kMaxEdgeIds) {
                        if (ctr) ctr->edge_overflow++;
                        continue;
                    }
                    for (uint32_t j = n_edge_ids; j > pos; --j) edge_ids[j] = edge_ids[j - 1];
                    edge_ids[pos] = id;
                    ++n_edge_ids;
                }
            }
        }
        WT_STEP_MARK(2);
        if (n_edge_ids > 0) {
            // ---- sample_fraunhofer_fsd_interaction (plt_bdpt_detail.hpp:287-346)
            const bool resume = defer && defer->resolved;   // second pass of a deferred FSD interaction: the aperture exists already
            const uint32_t slot = have_ap ? defer->slot : fsd_pool_alloc(pool);
            if (slot >= pool.cap) {
                if (ctr) ctr->fsd_pool_overflow++;
                ok = false;
            } else {
                fsd_aperture_t ap;
                if (have_ap) {
                    ap = pool.hdr[slot];
                } else {
                    // size the aperture's storage first (the reference's is a std::vector): an upper bound of its segment count
                    uint32_t need = 0;
                    if (pool.edge_counter) {
                        const vec2 cse = sigma * kBeamEnvelope;
                        const float max_len = .33f * fmaxf_(cse.x, cse.y);
                        for (uint32_t ei = 0; ei < n_edge_ids; ++ei) need += fsd_count_segments(sc, beam_frame, envelope, cse, max_len, eids[ei]);
                    }
                    if (!fsd_pool_alloc_edges(pool, slot, need, ap) && ctr) ctr->fsd_pool_overflow++;
                }
                const fsd_edges_ref_t ed{pool.edges + (size_t)ap.edge_offset, 1};
                if (!have_ap) {
                    fsd_build_aperture(sc, beam_frame, beam.k, 1.f, envelope, eids, n_edge_ids, sigma, ap, ed);
                    WT_STEP_MARK(3);
                    if (ctr && ap.overflow) ctr->fsd_edge_overflow += ap.overflow;
                    pool.hdr[slot] = ap;
                    // Device, pass B: one walk in eight of this pass ends up here with a real aperture; the intercepted-power
                    // integrals and the rejection sampling are left to a pass of its own (k_interact_c) where all 64 lanes of a
                    // wavefront do that work instead of a handful.
                    if (ap.n_edges > 0 && defer && defer->defer_sampling) {
                        defer->to_sampling_pass = 1;
                        defer->slot = slot;
                        return false;   // nothing has been committed
                    }
                }
                // Fraction of the beam's power the listed triangles intercept (find_closest_triangle, plt_bdpt_detail.hpp:391-416).
                // The reference computes it whenever the beam axis misses every triangle; its only consumer is the normalisation
                // 1/I of this aperture's scattering function, so it is evaluated only when the aperture has edges (one in seven
                // of the regions with classified edges; none of the null interactions) — same value, no RNG involved.
                if (ap.n_edges > 0 && !resume) {
                    if (defer && defer->has_gather) {
                        integrated_flux = defer->gather_flux;
                    } else {
                        for (uint32_t i = 0; i < tr.ntris; ++i)
                            integrated_flux += region_triangle_flux(sc, beam_frame, envelope, izr, sigma, tris[i], tr.front_face != 0);
                    }
                    const float I = (float)(1.0 - integrated_flux);
                    ap.recp_I = I > 0.f ? 1.f / I : 0.f;
                    pool.hdr[slot] = ap;
                }
                if (ap.n_edges == 0) {
                    beam_transform_restart(beam, interaction_wp, beam_dist);
                    do_RR = false;
                } else {
                    fsd_sample_t fs;
                    if (!defer) {
                        fs = fsd_sample(sc, ap, ed, smp);
                    } else if (resume) {
                        fs = defer->fs;
                        sampler_seek(smp, defer->end_draws);
                    } else {
                        // device: a lane runs the first kFsdInlineTries tries of the rejection loop itself; if none is accepted the
                        // rest is finished by its whole wavefront (64 tries per step) and this step is re-entered with the result.
                        const uint32_t max_tries = fsd_max_tries(ap), base = fsd_tries_base(smp);
                        const uint32_t t1 = max_tries < kFsdInlineTries ? max_tries : kFsdInlineTries;
                        fsd_try_t r{{0.f, 0.f}, 0.f, 0u};
                        const uint32_t t = fsd_run_tries(sc, ap, ed, smp, base, 0, t1, r);
                        if (t == 0xFFFFFFFFu && t1 < max_tries) {
                            defer->pending = 1;
                            defer->slot = slot;
                            defer->base = base;
                            defer->next_try = t1;
                            return false;   // nothing has been committed; the caller re-runs the step once `defer` is resolved
                        }
                        const bool accepted = t != 0xFFFFFFFFu;
                        sampler_seek(smp, fsd_draws_after(base, accepted ? t : max_tries - 1u));
                        fs = fsd_finalize(ap, accepted, r.x, r.f);
                    }
                    ok = !(fs.dpd == 0.f || fs.weight == 0.f);
                    if (ok) {
                        if (ctr) ctr->fsd_interactions++;
                        const vec3 woworld = to_world(ap.frame, fs.wo);
                        vertex_t v;
                        v.type = VT_FSD;
                        v.transport = beam.transport;
                        v.delta = 0;
                        v.fraunhofer_fsd = 1;
                        v.pdf_fwd = v.pdf_bwd = -1.f;
                        v.rr_weight = 1.f;
                        v.ref = -1;
                        v.emitter_of_shape = -1;
                        v.fsd_slot = slot;
                        v.geo_kind = GEO_POINT;
                        v.surf = make_dummy_surface(vec3{0, 0, 1}, interaction_wp);
                        ok = walk_append_vertex(sc, w, vs, v, fs.dpd, fs.dpd);
                        if (ok) {
                            if (ctr) ctr->vertices++;
                            beam_transform_region_interaction(beam, interaction_wp, beam_dist, woworld, fs.weight);
                            w.throughput *= fs.weight;
                        }
                    }
                }
            }
        } else {
            // ---- null interaction (plt_bdpt_detail.hpp:273-284)
            do_RR = false;
            beam_transform_restart(beam, interaction_wp, beam_dist);
            if (ctr) ctr->null_interactions++;
        }
    }
    }
    WT_STEP_MARK(4);
    bool cont = false;
    if (ok) cont = walk_continue(sc, w, vs, do_RR, smp);
    WT_STEP_MARK(5);
    w.rng_draws = smp.draws;
    return cont;
}

// ---- the surface interaction on its own: what the device's material-sorted pass A runs -----------------------------------------------
// Pass A of a round (the walks whose beam axis meets a triangle of the interaction region: 92 % of them) is cut in two on the device:
//   bdpt_classify      finds the primary triangle exactly as bdpt_walk_step does (ballistic hit / the trace kernels' axis hit of an overflowed
//                      region / scan of the region's list) and names the walk's CLASS: the leaf type of the hit shape's material when that is not
//                      a wrapper, WCLS_ANY otherwise; walks without a primary triangle leave for pass B, walks that hit nothing end;
//   bdpt_surface_step  sample_surface_interaction (plt_bdpt_detail.hpp:192-270) + append_vertex + transform + continue_walk for ONE class, so
//                      that a wavefront of the class kernel runs one BSDF's code (src/bsdf/diffuse.cpp:23-71, dielectric.cpp:26-72,
//                      surface_spm.cpp:40-201) and the kernel carries only that BSDF's registers.
// bdpt_surface_step reads and writes the walk RECORD (its 32-bit words, in memory) field by field, each where the step needs it, and writes
// the new vertex as its parts become known — header, surface, a straight copy of the arriving beam — instead of holding walk_t (57 words),
// vertex_t (86) and the traversal record (17) in registers across the BSDF: same operands, same operations, same order as the surface
// branch of bdpt_walk_step (the CPU checker can run its walks through this pair: oracle_set_split_step, tests/test_oracle.py).
enum walk_class_e : uint32_t { WCLS_DIFFUSE = 0, WCLS_DIELECTRIC = 1, WCLS_SPM = 2, WCLS_ANY = 3, kNumWalkClasses = 4, WCLS_NO_PRIMARY = 4, WCLS_END = 5 };
struct primary_hit_t {
    uint32_t tuid;
    float dist, bx, by;
};
WT_HD uint32_t walk_class_of_material_type(int32_t type) { return type >= 0 && type < (int32_t)MAT_COMPOSITE ? (uint32_t)type : (uint32_t)WCLS_ANY; }
WT_HD uint32_t walk_class_of_triangle(const scene_t& sc, uint32_t tuid) {
    return walk_class_of_material_type(sc.materials[sc.shapes[sc.tri_meta[tuid].shape_idx].material].type);
}
// `tri_class`: walk_class_of_triangle for every triangle, one byte each (device: built at upload), or nullptr
template <class TriList>
WT_HD uint32_t bdpt_classify(const scene_t& sc, vec3 beam_d, bool beam_ray, const trav_result_t& tr, const TriList& tris, const unsigned char* tri_class, primary_hit_t& ph) {
    ph.tuid = kInvalid;
    ph.dist = WT_INF;
    ph.bx = ph.by = 0.f;
    if (tr.empty) return WCLS_END;
    const bool is_ballistic = tr.ballistic || beam_ray;
    if (is_ballistic) {
        ph.tuid = tr.tuid;
        ph.dist = tr.dist;
        ph.bx = tr.bx;
        ph.by = tr.by;
    } else if (tr.aborted == 2) {
        if (tr.tuid != kInvalid) {
            ph.tuid = tr.tuid;
            ph.dist = tr.pdist;
            ph.bx = tr.bx;
            ph.by = tr.by;
        }
    } else {
        const range_t izr{tr.dist, tr.dist + tr.region_depth};
        for (uint32_t i = 0; i < tr.ntris; ++i) {
            const uint32_t tuid = tris[i];
            const tri_geo_t g = sc.tri_geo[tuid];
            const float fptol = cone_intersection_tolerance(tr.origin, g.a, g.b, g.c);
            ray_tri_hit_t h;
            if (intersect_ray_tri(tr.origin, beam_d, g.a, g.b, g.c, grow(izr, fptol), h) && h.dist < ph.dist) {
                ph.tuid = tuid;
                ph.dist = h.dist;
                ph.bx = h.bx;
                ph.by = h.by;
            }
        }
    }
    if (ph.tuid == kInvalid) return WCLS_NO_PRIMARY;
    return tri_class ? (uint32_t)tri_class[ph.tuid] : walk_class_of_triangle(sc, ph.tuid);
}

// the words of a walk record in memory
struct walk_rec_t {
    uint32_t* p;
    template <class F>
    WT_HD F get(size_t word) const {
        static_assert(sizeof(F) == 4, "");
        const uint32_t w = p[word];
        F f;
        __builtin_memcpy(&f, &w, 4);
        return f;
    }
    template <class F>
    WT_HD void set(size_t word, F value) const {
        static_assert(sizeof(F) == 4, "");
        uint32_t w;
        __builtin_memcpy(&w, &value, 4);
        p[word] = w;
    }
    WT_HD vec3 get3(size_t word) const { return vec3{get<float>(word), get<float>(word + 1), get<float>(word + 2)}; }
    WT_HD void set3(size_t word, vec3 v) const {
        set(word, v.x);
        set(word + 1, v.y);
        set(word + 2, v.z);
    }
};
// CLS: MAT_DIFFUSE / MAT_DIELECTRIC / MAT_SURFACE_SPM — the walk's class, the material is an unwrapped BSDF of that type — or -1 (WCLS_ANY).
// Returns TRUE if the walk continues.  A walk that ends leaves its record as it is, except for what an appended vertex changed.
template <int CLS>
WT_HD bool bdpt_surface_step(const scene_t& sc, const walk_rec_t& wr, vec3 origin_wp, float beam_dist, const primary_hit_t& ph, const vertex_store_t& vs, uint64_t seed,
                             uint64_t sample_id, uint32_t stream, bdpt_counters_t* ctr) {
    sampler_t smp = make_sampler(seed, sample_id, stream, wr.get<uint32_t>(WT_WALK_WORD(rng_draws)));
    cone_t env;
    {
        uint32_t* e = reinterpret_cast<uint32_t*>(&env);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (size_t i = 0; i < sizeof(cone_t) / 4; ++i) e[i] = wr.p[WT_WALK_WORD(beam.env) + i];
    }
    const float k = wr.get<float>(WT_WALK_WORD(beam.k));
    const uint32_t transport = wr.get<uint32_t>(WT_WALK_WORD(beam.transport));
    // ---- sample_surface_interaction (plt_bdpt_detail.hpp:192-270)
    const uint32_t primary = ph.tuid;
    const vec3 gn = sc.tri_geo[primary].n;
    const vec3 sampled_tri_wp = origin_wp + env.d * ph.dist;
    surface_t srf = make_surface(sc, primary, gn, vec2{ph.bx, ph.by}, sampled_tri_wp);
    srf.footprint = cone_surface_footprint_static(env, srf, beam_dist);
    const shape_t shp = sc.shapes[srf.shape];
    const vec3 ng = srf.geo.n, ns = srf.shading.n;
    const vec3 wiworld = -env.d;
    const vec3 wi = to_local(srf.shading, wiworld);
    const float wig = dot(wiworld, ng), wis = wi.z;
    if (!(wig * wis > 0.f)) return false;
    const bsdf_sample_t bs = material_sample<CLS>(sc, shp.material, wi, k, transport, smp, srf.uv);
    if (!(bs.valid && bs.dpd != 0.f)) return false;
    const bool is_delta = pd_is_discrete(bs.dpd);
    const vec3 wo = bs.wo;
    const vec3 woworld = normalize(to_world(srf.shading, wo));
    const float wog = dot(woworld, ng), wos = wo.z;
    if (ctr) ctr->surface_interactions++;
    if (!(wog * wos > 0.f)) return false;
    const float pdf_revr = material_pdf<CLS>(sc, shp.material, wo, wi, k, flip_transport(transport), srf.uv);
    // ---- append_vertex (plt_bdpt_detail.hpp:95-121; walk_append_vertex above)
    const vec3 prev_wp = wr.get3(WT_WALK_WORD(prev_wp));
    if (veq(prev_wp, srf.wp)) return false;
    uint32_t nverts = wr.get<uint32_t>(WT_WALK_WORD(nverts));
    {
        struct {
            uint32_t type;
            int32_t ref;
            uint32_t geo_kind;
            const surface_t& surf;
        } vview{VT_SURFACE, shp.material, GEO_SURFACE, srf};
        const float pv = convert_directional_density_to_area(sc, wr.get<float>(WT_WALK_WORD(pdf_from_prev)), prev_wp, vview);
        const uint32_t hdr[12] = {VT_SURFACE,
                                  transport,
                                  is_delta ? 1u : 0u,
                                  0u,
                                  __builtin_bit_cast(uint32_t, transport == TRANSPORT_FORWARD ? pv : -1.f),
                                  __builtin_bit_cast(uint32_t, transport == TRANSPORT_FORWARD ? -1.f : pv),
                                  __builtin_bit_cast(uint32_t, 1.f),
                                  (uint32_t)shp.material,
                                  (uint32_t)shp.emitter,
                                  kInvalid,
                                  (uint32_t)GEO_SURFACE,
                                  1u};
        static_assert(WT_VWORD(type) == 0 && WT_VWORD(transport) == 1 && WT_VWORD(delta) == 2 && WT_VWORD(fraunhofer_fsd) == 3 && WT_VWORD(pdf_fwd) == 4 && WT_VWORD(pdf_bwd) == 5 &&
                          WT_VWORD(rr_weight) == 6 && WT_VWORD(ref) == 7 && WT_VWORD(emitter_of_shape) == 8 && WT_VWORD(fsd_slot) == 9 && WT_VWORD(geo_kind) == 10 &&
                          WT_VWORD(has_beam) == 11 && WT_VWORD(surf) == 12,
                      "vertex_t header layout");
        uint32_t* vp = vs.base + vs.idx * vs.stride + (size_t)nverts * kVertexWords;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int i = 0; i < 12; ++i) vp[i] = hdr[i];
        const uint32_t* sw = reinterpret_cast<const uint32_t*>(&srf);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (size_t i = 0; i < sizeof(surface_t) / 4; ++i) vp[WT_VWORD(surf) + i] = sw[i];
        // the arriving beam: a copy of the walk's (its envelope is in registers already)
        const uint32_t* ew = reinterpret_cast<const uint32_t*>(&env);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (size_t i = 0; i < sizeof(cone_t) / 4; ++i) vp[WT_VWORD(beam) + i] = ew[i];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (size_t i = sizeof(cone_t) / 4; i < sizeof(beam_t) / 4; ++i) vp[WT_VWORD(beam) + i] = wr.p[WT_WALK_WORD(beam) + i];
        // reversed pdf of the previous vertex (sampling prev from v)
        const float dens = pd_density_or_zero(pdf_revr);
        float prev_rev = 0.f;
        if (dens != 0.f) {
            const vec3 d = prev_wp - srf.wp;
            const float d2 = length2(d);
            if (d2 == 0.f)
                prev_rev = WT_INF;
            else {
                prev_rev = dens * (1.f / d2);
                if (wr.get<uint32_t>(WT_WALK_WORD(prev_on_surface))) prev_rev *= fabsf(dot(wr.get3(WT_WALK_WORD(prev_ng)), normalize(d)));
            }
        }
        vs.store_word(nverts - 1, transport == TRANSPORT_BACKWARD ? WT_VWORD(pdf_fwd) : WT_VWORD(pdf_bwd), prev_rev);
        ++nverts;
        wr.set(WT_WALK_WORD(pdf_from_prev), bs.dpd);
        wr.set(WT_WALK_WORD(nverts), nverts);
        // walk_cache_prev
        wr.set3(WT_WALK_WORD(prev_wp), srf.wp);
        wr.set3(WT_WALK_WORD(prev_ng), ng);
        wr.set(WT_WALK_WORD(prev_on_surface), 1u);
        wr.set(WT_WALK_WORD(prev_offset_tuid), srf.tuid);
    }
    if (ctr) ctr->vertices++;
    float ws = 1.f;
    if (!veq(ns, ng)) ws *= shading_normals_correction_scale(transport, wig, wog, wis, wos);
    // ---- transform_surface_interaction (plt_bdpt_detail.hpp:123-136; beam.hpp:379-398)
    {
        beam_t b;
        float sid;
        b.env = cone_through_surface_footprint(srf, srf.wp, woworld, env.tan_alpha, &sid);
        b.k = k;
        b.transport = transport;
        uint32_t* bw = reinterpret_cast<uint32_t*>(&b);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (size_t i = offsetof(beam_t, frame) / 4; i < sizeof(beam_t) / 4; ++i) bw[i] = wr.p[WT_WALK_WORD(beam) + i];
        beam_apply_bsdf(b, ws * bs.M, woworld, srf, cone_frame(b.env));
        b.self_intersection_distance = sid;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (size_t i = 0; i < sizeof(beam_t) / 4; ++i) wr.p[WT_WALK_WORD(beam) + i] = bw[i];
    }
    float throughput = wr.get<float>(WT_WALK_WORD(throughput)) * (ws * mueller_mean_intensity(bs.M));
    if (transport == TRANSPORT_BACKWARD && bs.eta != 1.f) throughput /= sqr(bs.eta);
    // ---- continue_walk (plt_bdpt_detail.hpp:167-182; walk_continue above)
    bool cont = true;
    float rr_weight = wr.get<float>(WT_WALK_WORD(rr_weight));
    if ((int)nverts > sc.opts.max_depth + 1)
        cont = false;
    else if (sc.opts.RR) {
        vs.store_word(nverts - 1, WT_VWORD(rr_weight), rr_weight);
        const float r = throughput < 1.f ? fmaxf_(throughput, .5f) : 1.f;
        if (sampler_r(smp) <= r) {
            const float scale = 1.f / r;
            rr_weight *= scale;
            throughput *= scale;
        } else
            cont = false;
    }
    wr.set(WT_WALK_WORD(throughput), throughput);
    wr.set(WT_WALK_WORD(rr_weight), rr_weight);
    wr.set(WT_WALK_WORD(rng_draws), smp.draws);
    return cont;
}

// ---- connections -------------------------------------------------------------------------------------------
// random stream of the (s,t) connection: one per strategy (short subpaths keep the ids of rounds 1-2; longer ones follow behind them)
WT_HD uint32_t connect_stream(int s, int t) {
    if (s < 32 && t < 32) return STREAM_CONNECT + (uint32_t)t * 32u + (uint32_t)s;
    return STREAM_CONNECT + 1024u + (uint32_t)t * 4096u + (uint32_t)s;
}
struct connect_ret_t {
    stokes_t L;
    vertex_t temporary_vert;
    uint32_t has_temp;
    sensor_element_t element;
    uint32_t has_element;
    // DEFER (bdpt_connect<true>): the connection's shadow ray has not been traced — L is the flux of the unoccluded connection, `ray` the ray
    // integrator::shadow would cast (need_shadow = 0: the strategy casts none, or L is zero already)
    shadow_ray_t ray;
    uint32_t need_shadow;
};

// connect_and_integrate (plt_bdpt_detail.hpp:722-745).  DEFER: the ray is handed out instead of being traced (the device traces the rays of
// all connections of a batch in one kernel of their own, all lanes busy: k_connect_shadow).
template <bool DEFER>
WT_HD stokes_t connect_and_integrate(const scene_t& sc, const beam_t& db, const conn_end_t& dv, const beam_t& eb, const conn_end_t& ev, const stack_ref_t& stack,
                                     bdpt_counters_t* ctr, bvh_counters_t* bctr, connect_ret_t& ret) {
    if (beam_intensity(db) == 0.f || beam_intensity(eb) == 0.f) return stokes_zero();
    if (ctr) ctr->shadow_rays++;
    const shadow_ray_t ray = conn_shadow_ray(sc, dv, ev);
    if (DEFER) {
        const stokes_t L = integrate_beams(db, eb);
        if (L.s[0] > 0.f) {   // (otherwise the strategy contributes nothing whatever the ray meets: bdpt_strategy)
            ret.ray = ray;
            ret.need_shadow = 1;
        }
        return L;
    }
    if (ads_shadow_ray(sc, ray.o, ray.d, range_t{0.f, ray.dist}, stack, bctr)) return stokes_zero();
    return integrate_beams(db, eb);
}

WT_HD void make_temp_vertex(vertex_t& v, uint32_t type, uint32_t transport, int ref, bool has_surface, const surface_t& surface, vec3 p) {
    v.type = type;
    v.transport = transport;
    v.delta = 0;
    v.fraunhofer_fsd = 0;
    v.pdf_fwd = v.pdf_bwd = -1.f;
    v.rr_weight = 1.f;
    v.ref = ref;
    v.emitter_of_shape = -1;
    v.fsd_slot = kInvalid;
    v.has_beam = 0;
    if (has_surface) {
        v.geo_kind = GEO_SURFACE;
        v.surf = surface;
    } else {
        v.geo_kind = GEO_POINT;
        v.surf = make_dummy_surface(vec3{0, 0, 1}, p);
    }
}
// vertex_is_connectible from the vertex store: the three words it reads
WT_HD bool vertex_store_connectible(const scene_t& sc, const vertex_store_t& vs, uint32_t idx) {
    struct {
        uint32_t type;
        int32_t ref;
        struct {
            float k;
        } beam;
    } v{vs.load_word<uint32_t>(idx, WT_VWORD(type)), vs.load_word<int32_t>(idx, WT_VWORD(ref)), {vs.load_word<float>(idx, WT_VWORD(beam) + offsetof(beam_t, k) / 4)}};
    switch (v.type) {
    case VT_FSD: return true;
    case VT_EMITTER: return !emitter_is_delta_direction(sc.emitters[v.ref]);
    case VT_SENSOR: return !sensor_is_delta_direction(sc.sensor);
    case VT_SURFACE: return !material_is_delta_only(sc, v.ref, v.beam.k);
    default: return false;
    }
}

// connect_subpaths (plt_bdpt_detail.hpp:747-923).  nS/nT = number of vertices of the emitter/sensor subpaths.
// (The vertices of a connection are loaded one at a time, each dropped once the beam it sends towards the other has been formed: two
// vertex_t and their two beams at once are 258 registers on the device.)
template <bool DEFER = false>
WT_HD void bdpt_connect(const scene_t& sc, const fsd_pool_t& pool, const vertex_store_t& svs, const vertex_store_t& evs, int s, int t,
                        uint64_t seed, uint64_t sample_id, const stack_ref_t& stack, connect_ret_t& ret, bdpt_counters_t* ctr, bvh_counters_t* bctr) {
    ret.L = stokes_zero();
    ret.has_temp = 0;
    ret.has_element = 0;
    ret.need_shadow = 0;
    sampler_t smp = make_sampler(seed, sample_id, connect_stream(s, t));
    if (ctr) ctr->connections++;

    if (s == 0) {
        vertex_t last;
        svs.load(t - 1, last);
        if (vertex_on_emitter(last)) {
            beam_t QE = last.beam;
            beam_scale(QE, last.rr_weight);
            ret.L = emitter_Li(sc, vertex_get_emitter(last), QE, last.surf);
        }
    } else if (t == 0) {
        if (sensor_is_virtual(sc.sensor)) {
            vertex_t last;
            evs.load(s - 1, last);
            vertex_nb_t current;
            evs.load(s - 2, current);
            const vec3 wp_end = vertex_wp(last);
            const beam_t& beam = last.beam;
            const float dist = length(wp_end - beam.env.o);
            sensor_direct_connection_t dc = vplane_Si(sc, beam, range_t{0.f, dist});
            if (dc.valid) {
                ret.element = dc.element;
                ret.has_element = 1;
                float wgt = current.rr_weight;
                if (vertex_is_on_surface(sc, current) && (current.type == VT_FSD || current.type == VT_SURFACE || current.type == VT_MEDIUM) && !current.delta)
                    wgt /= fabsf(dot(dc.beam.env.d, vertex_ns(sc, current)));
                wgt /= fabsf(dot(dc.beam.env.d, dc.surface.geo.n));
                beam_scale(dc.beam, wgt);
                make_temp_vertex(ret.temporary_vert, VT_SENSOR, TRANSPORT_BACKWARD, -1, true, dc.surface, dc.beam.env.o);
                ret.has_temp = 1;
                ret.L = integrate_beams(dc.beam, beam);
            }
        }
    } else if (s == 1) {
        vertex_t last;
        svs.load(t - 1, last);
        if (vertex_is_connectible(sc, last)) {
            const float k = last.beam.k;
            const vec3 wp = vertex_wp(last);
            emitter_direct_sample_t ed = scene_sample_emitter_direct(sc, wp, k, smp);
            if ((pd_is_discrete(ed.dpd) || ed.dpd != 0.f) && beam_intensity(ed.beam) > 0.f) {
                float wgt = last.rr_weight;
                if (vertex_is_on_surface(sc, last)) wgt *= fabsf(dot(ed.beam.env.d, vertex_ns(sc, last)));
                beam_scale(ed.beam, wgt);
                make_temp_vertex(ret.temporary_vert, VT_EMITTER, TRANSPORT_FORWARD, ed.emitter, ed.has_surface, ed.surface, ed.beam.env.o);
                ret.has_temp = 1;
                beam_t db;
                if (vertex_interact(sc, pool, last, vertex_wp(ret.temporary_vert), false, db))
                    ret.L = connect_and_integrate<DEFER>(sc, db, conn_end_of(last), ed.beam, conn_end_of(ret.temporary_vert), stack, ctr, bctr, ret);
            }
        }
    } else if (t == 1) {
        vertex_t last;
        evs.load(s - 1, last);
        const bool is_virtual = sensor_is_virtual(sc.sensor);
        const bool do_direct = (is_virtual || last.type != VT_FSD) && vertex_is_connectible(sc, last);
        if (do_direct) {
            sensor_direct_sample_t sd = sensor_sample_direct(sc, vertex_wp(last), last.beam.k, smp);
            if ((pd_is_discrete(sd.dpd) || sd.dpd != 0.f) && beam_intensity(sd.beam) > 0.f) {
                float wgt = last.rr_weight;
                if (vertex_is_on_surface(sc, last)) wgt *= fabsf(dot(sd.beam.env.d, vertex_ns(sc, last)));
                beam_scale(sd.beam, wgt);
                make_temp_vertex(ret.temporary_vert, VT_SENSOR, TRANSPORT_BACKWARD, -1, sd.has_surface, sd.surface, sd.beam.env.o);
                ret.has_temp = 1;
                beam_t eb;
                if (vertex_interact(sc, pool, last, vertex_wp(ret.temporary_vert), false, eb)) {
                    ret.L = connect_and_integrate<DEFER>(sc, sd.beam, conn_end_of(ret.temporary_vert), eb, conn_end_of(last), stack, ctr, bctr, ret);
                    ret.element = sd.element;
                    ret.has_element = 1;
                }
            }
        }
    } else {
        const vec3 ev_wp = evs.load_wp(s - 1), sv_wp = svs.load_wp(t - 1);
        const vec3 dl = ev_wp - sv_wp;
        if (vertex_store_connectible(sc, evs, s - 1) && vertex_store_connectible(sc, svs, t - 1) && !(dl.x == 0.f && dl.y == 0.f && dl.z == 0.f)) {
            beam_t eb, db;
            conn_end_t ev_end, sv_end;
            vec3 ev_ns, sv_ns;
            bool ev_on, sv_on, heb, hdb = false;
            float ev_rr, sv_rr;
            {
                vertex_t ev;
                evs.load(s - 1, ev);
                heb = vertex_interact(sc, pool, ev, sv_wp, true, eb);
                ev_end = conn_end_of(ev);
                ev_ns = vertex_ns(sc, ev);
                ev_on = vertex_is_on_surface(sc, ev);
                ev_rr = ev.rr_weight;
            }
            if (heb) {
                vertex_t sv;
                svs.load(t - 1, sv);
                hdb = vertex_interact(sc, pool, sv, ev_wp, true, db);
                sv_end = conn_end_of(sv);
                sv_ns = vertex_ns(sc, sv);
                sv_on = vertex_is_on_surface(sc, sv);
                sv_rr = sv.rr_weight;
            }
            if (heb && hdb) {
                const float recp_d2 = 1.f / length2(dl);
                const vec3 d = dl * sqrtf(recp_d2);
                float wev = ev_rr;
                float wsv = sv_rr * recp_d2;
                if (sv_on) wev *= fabsf(dot(sv_ns, d));
                if (ev_on) wsv *= fabsf(dot(ev_ns, d));
                beam_scale(db, wsv);
                beam_scale(eb, wev);
                ret.L = connect_and_integrate<DEFER>(sc, db, sv_end, eb, ev_end, stack, ctr, bctr, ret);
            }
        }
    }
}
// The temporary vertex (and the sensor element) of a t = 0 (virtual sensor), s = 1 or t = 1 connection once more, from the same random
// numbers — what the MIS weight and the light-image splat of the strategy need of bdpt_connect's outcome.  (Device: the connection's flux
// waits for its shadow ray in a 52-byte record; the 43 words of the temporary vertex are cheaper to form again than to carry along.)
WT_HD void bdpt_connect_temp(const scene_t& sc, const vertex_store_t& svs, const vertex_store_t& evs, int s, int t, uint64_t seed, uint64_t sample_id, vertex_nb_t& tv,
                             sensor_element_t& element, bool& has_element) {
    has_element = false;
    vertex_t tmp;
    bool has_temp = false;
    sampler_t smp = make_sampler(seed, sample_id, connect_stream(s, t));
    if (s == 0) {
    } else if (t == 0) {
        if (sensor_is_virtual(sc.sensor)) {
            vertex_t last;
            evs.load(s - 1, last);
            const float dist = length(vertex_wp(last) - last.beam.env.o);
            const sensor_direct_connection_t dc = vplane_Si(sc, last.beam, range_t{0.f, dist});
            if (dc.valid) {
                element = dc.element;
                has_element = true;
                make_temp_vertex(tmp, VT_SENSOR, TRANSPORT_BACKWARD, -1, true, dc.surface, dc.beam.env.o);
                has_temp = true;
            }
        }
    } else if (s == 1) {
        const emitter_direct_sample_t ed = scene_sample_emitter_direct(sc, svs.load_wp(t - 1), svs.load_word<float>(t - 1, WT_VWORD(beam) + offsetof(beam_t, k) / 4), smp);
        make_temp_vertex(tmp, VT_EMITTER, TRANSPORT_FORWARD, ed.emitter, ed.has_surface, ed.surface, ed.beam.env.o);
        has_temp = true;
    } else if (t == 1) {
        const sensor_direct_sample_t sd = sensor_sample_direct(sc, evs.load_wp(s - 1), evs.load_word<float>(s - 1, WT_VWORD(beam) + offsetof(beam_t, k) / 4), smp);
        make_temp_vertex(tmp, VT_SENSOR, TRANSPORT_BACKWARD, -1, sd.has_surface, sd.surface, sd.beam.env.o);
        has_temp = true;
        element = sd.element;
        has_element = true;
    }
    if (has_temp) __builtin_memcpy(&tv, &tmp, offsetof(vertex_t, beam));
    tv.beam.k = 0.f;
}

// bdpt_compute_mis_weight (plt_bdpt_detail.hpp:604-720).  The reference copies every vertex's densities into arrays
// (bdpt_populate_subpaths_pdfs), overwrites the few entries the connection changes, and then forms the running products; here the
// changed entries are computed first and the products read each vertex's three words (pdf_fwd, pdf_bwd, delta) straight from the
// vertex store, newest vertex first — the same numbers in the same order without per-thread arrays (which live in scratch memory on
// the device) and without a cap on the path length.  Vertices enter the densities without their beams (vertex_nb_t), the
// predecessors with their position only.
// `tv`: the connection's temporary vertex (vertex_t or its beam-less part vertex_nb_t: the densities read nothing else of it).
template <class TV>
WT_HD float bdpt_mis_weight(const scene_t& sc, const fsd_pool_t& pool, const vertex_store_t& svs, const vertex_store_t& evs, int s, int t, const TV& tv) {
    if (s + t <= 2) return 1.f;
    // entries of the sensor (s*) / emitter (e*) subpath arrays that the connection overrides: `last` = index n-1, `prev` = n-2, `first` = 0
    float srev_last = 0.f, srev_prev = 0.f, spdf_first = 0.f, erev_last = 0.f, erev_prev = 0.f, epdf_first = 0.f;
    bool has_srev_last = false, has_srev_prev = false, has_spdf_first = false, has_erev_last = false, has_erev_prev = false, has_epdf_first = false;
    if (s == 0) {
        vertex_nb_t last, prev;
        svs.load(t - 1, last);
        svs.load(t - 2, prev);
        srev_last = vertex_pdf_emitter(sc, last);
        srev_prev = vertex_pdf_next_from_emitter(sc, last, prev);
        has_srev_last = has_srev_prev = true;
    } else if (t == 0) {
        vertex_nb_t prev;
        evs.load(s - 2, prev);
        erev_last = vertex_pdf_sensor(sc);
        if (sensor_is_virtual(sc.sensor))
            erev_prev = vertex_pdf_next_from_sensor(sc, tv, prev);
        else {
            vertex_nb_t last;
            evs.load(s - 1, last);
            erev_prev = vertex_pdf_next_from_sensor(sc, last, prev);
        }
        has_erev_last = has_erev_prev = true;
    } else if (s == 1) {
        vertex_nb_t last;
        svs.load(t - 1, last);
        srev_last = vertex_pdf_next_from_emitter(sc, tv, last);
        erev_last = vertex_pdf(sc, pool, last, svs.load_wp(t - 2), tv, TRANSPORT_BACKWARD);   // (index 0 = s - 1)
        epdf_first = vertex_pdf_emitter(sc, tv);
        has_srev_last = has_erev_last = has_epdf_first = true;
    } else if (t == 1) {
        vertex_nb_t last;
        evs.load(s - 1, last);
        erev_last = vertex_pdf_next_from_sensor(sc, tv, last);
        srev_last = vertex_pdf(sc, pool, last, evs.load_wp(s - 2), tv, TRANSPORT_FORWARD);   // (index 0 = t - 1)
        spdf_first = vertex_pdf_sensor(sc);
        has_erev_last = has_srev_last = has_spdf_first = true;
    } else {
        vertex_nb_t ev, sv;
        evs.load(s - 1, ev);
        svs.load(t - 1, sv);
        const vec3 ev_prev_wp = evs.load_wp(s - 2), sv_prev_wp = svs.load_wp(t - 2);
        // (of the predecessors as `next`: position, surface normal and what vertex_is_on_surface reads)
        vertex_nb_t ev_prev, sv_prev;
        evs.load(s - 2, ev_prev);
        svs.load(t - 2, sv_prev);
        erev_last = vertex_pdf(sc, pool, sv, sv_prev_wp, ev, TRANSPORT_BACKWARD);
        erev_prev = vertex_pdf(sc, pool, ev, vertex_wp(sv), ev_prev, TRANSPORT_BACKWARD);
        srev_last = vertex_pdf(sc, pool, ev, ev_prev_wp, sv, TRANSPORT_FORWARD);
        srev_prev = vertex_pdf(sc, pool, sv, vertex_wp(ev), sv_prev, TRANSPORT_FORWARD);
        has_erev_last = has_erev_prev = has_srev_last = has_srev_prev = true;
    }
    bool delta_emitter, delta_sensor;
    if (s == 1)
        delta_emitter = vertex_is_delta_emitter(sc, tv);
    else if (s > 1) {
        struct {
            uint32_t type;
            int32_t ref;
        } ev0{evs.load_word<uint32_t>(0, WT_VWORD(type)), evs.load_word<int32_t>(0, WT_VWORD(ref))};
        delta_emitter = vertex_is_delta_emitter(sc, ev0);
    } else
        delta_emitter = true;
    if (t == 1)
        delta_sensor = vertex_is_delta_sensor(sc, tv);
    else if (t > 1) {
        struct {
            uint32_t type;
        } sv0{svs.load_word<uint32_t>(0, WT_VWORD(type))};
        delta_sensor = vertex_is_delta_sensor(sc, sv0);
    } else
        delta_sensor = true;

    // The running products read three words per vertex, newest vertex first.  They are FETCHED FOUR VERTICES AT A TIME before the arithmetic of
    // the first of them: one load per loop iteration is one dependent memory round trip per vertex on the device (wave-uniform trip counts: the
    // 64 items of a wavefront share (s, t)), and this kernel is bound by such round trips.  Same operands, same order of operations.
    float sum_Ri = 0.f, ri = 1.f;
    {
        // sensor subpath, i = t-1 .. 0: fwd = pdf_bwd, rev = pdf_fwd; the connection vertex counts as non-delta
        bool del_i = false;   // sdel[t-1] = 0
        for (int i0 = t - 1; i0 >= 0; i0 -= 4) {
            float F[4], R[4];
            uint32_t D[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int i = i0 - j;
                F[j] = R[j] = 0.f;
                D[j] = 0u;
                if (i >= 0) {
                    F[j] = svs.load_word<float>(i, WT_VWORD(pdf_bwd));
                    R[j] = svs.load_word<float>(i, WT_VWORD(pdf_fwd));
                    if (i > 0) D[j] = svs.load_word<uint32_t>(i - 1, WT_VWORD(delta));
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int i = i0 - j;
                if (i < 0) break;
                const float f = (i == 0 && has_spdf_first) ? spdf_first : F[j];
                const float rv = (i == t - 1 && has_srev_last) ? srev_last : ((i == t - 2 && has_srev_prev) ? srev_prev : R[j]);
                const bool del_prev = i > 0 ? D[j] != 0 : delta_sensor;
                const float fwd = (finitef(f) && f > FLT_EPSILON) ? f : 1.f;
                const float rev = (finitef(rv) && rv > FLT_EPSILON) ? rv : 1.f;
                ri *= rev / fwd;
                if (!del_i && !del_prev) sum_Ri += ri;
                del_i = del_prev;
            }
        }
    }
    ri = 1.f;
    {
        bool del_i = false;   // edel[s-1] = 0
        for (int i0 = s - 1; i0 >= 0; i0 -= 4) {
            float F[4], R[4];
            uint32_t D[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int i = i0 - j;
                F[j] = R[j] = 0.f;
                D[j] = 0u;
                if (i >= 0) {
                    F[j] = evs.load_word<float>(i, WT_VWORD(pdf_fwd));
                    R[j] = evs.load_word<float>(i, WT_VWORD(pdf_bwd));
                    if (i > 0) D[j] = evs.load_word<uint32_t>(i - 1, WT_VWORD(delta));
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int i = i0 - j;
                if (i < 0) break;
                const float f = (i == 0 && has_epdf_first) ? epdf_first : F[j];
                const float rv = (i == s - 1 && has_erev_last) ? erev_last : ((i == s - 2 && has_erev_prev) ? erev_prev : R[j]);
                const bool del_prev = i > 0 ? D[j] != 0 : delta_emitter;
                const float fwd = (finitef(f) && f > FLT_EPSILON) ? f : 1.f;
                const float rev = (finitef(rv) && rv > FLT_EPSILON) ? rv : 1.f;
                ri *= rev / fwd;
                if (!del_i && !del_prev) sum_Ri += ri;
                del_i = del_prev;
            }
        }
    }
    return 1.f / (1.f + sum_Ri);
}

// What follows the connection of strategy (s,t) with flux L > 0 (plt_bdpt.cpp:113-140): MIS weight, the light-image splat of the t <= 1
// strategies (performed here), the flux to be accumulated into the sample's L for t > 1 (returned).
template <class TV>
WT_HD stokes_t bdpt_strategy_finish(const scene_t& sc, const fsd_pool_t& pool, const film_t& film, const vertex_store_t& svs, const vertex_store_t& evs, int s, int t,
                                    const sample_ctx_t& ctx, const stokes_t& L, const TV& tv, const sensor_element_t& element, bool has_element, bdpt_counters_t* ctr) {
    float mis;
    if (sc.opts.debug_only_s || sc.opts.debug_only_t)
        mis = ctx.recp_spectral_pd;
    else if (sc.opts.MIS)
        mis = bdpt_mis_weight(sc, pool, svs, evs, s, t, tv) * ctx.recp_spectral_pd;
    else
        mis = 1.f / (float(s + t + 1) * ctx.k_density);
    const stokes_t flux = L * mis;
    if (t > 1) return flux;
    if (has_element) {
        film_splat_direct(sc, film, element, flux, ctx.k);
        if (ctr) ctr->light_splats++;
    }
    return stokes_zero();
}
// One (s,t) strategy of plt_bdpt.cpp:105-140.  Returns the flux to be accumulated into L (t>1) and performs the
// light-image splat itself for t<=1.
// STAGED (CPU checker only, oracle_set_staged_connect): the connection the way the device's three connection kernels run it — flux without
// the shadow ray, the ray, then MIS and splat with the temporary vertex formed again (bdpt_connect_temp) — must give the same numbers.
template <bool STAGED = false>
WT_HD stokes_t bdpt_strategy(const scene_t& sc, const fsd_pool_t& pool, const film_t& film, const vertex_store_t& svs, const vertex_store_t& evs, int s,
                             int t, const sample_ctx_t& ctx, uint64_t seed, uint64_t sample_id, const stack_ref_t& stack, bdpt_counters_t* ctr,
                             bvh_counters_t* bctr) {
    connect_ret_t cr;
    bdpt_connect<STAGED>(sc, pool, svs, evs, s, t, seed, sample_id, stack, cr, ctr, bctr);
    if (!(cr.L.s[0] > 0.f)) return stokes_zero();
    if (STAGED) {
        if (cr.need_shadow && ads_shadow_ray(sc, cr.ray.o, cr.ray.d, range_t{0.f, cr.ray.dist}, stack, bctr)) return stokes_zero();
        vertex_nb_t tv;
        sensor_element_t element;
        bool has_element;
        bdpt_connect_temp(sc, svs, evs, s, t, seed, sample_id, tv, element, has_element);
        return bdpt_strategy_finish(sc, pool, film, svs, evs, s, t, ctx, cr.L, tv, element, has_element, ctr);
    }
    return bdpt_strategy_finish(sc, pool, film, svs, evs, s, t, ctx, cr.L, cr.temporary_vert, cr.element, cr.has_element != 0, ctr);
}

// The (s,t) loop of plt_bdpt.cpp:105-146 for one sample, given both finished subpaths.
template <bool STAGED = false>
WT_HD void bdpt_connect_all(const scene_t& sc, const fsd_pool_t& pool, const film_t& film, const vertex_store_t& svs, const vertex_store_t& evs, int nT,
                            int nS, const sample_ctx_t& ctx, uint64_t seed, uint64_t sample_id, const stack_ref_t& stack, bdpt_counters_t* ctr,
                            bvh_counters_t* bctr) {
    stokes_t L = stokes_zero();
    for (int t = 0; t <= nT; ++t)
        for (int s = 0; s <= nS; ++s) {
            const int depth = t + s - 2;
            if ((t == 1 && s == 1) || depth < 0) continue;
            if (!sc.opts.emitter_direct && s == 1) continue;
            if (!sc.opts.sensor_direct && t == 1) continue;
            if (depth > sc.opts.max_depth) break;
            if (sc.opts.debug_only_s && (int)sc.opts.debug_only_s - 1 != s) continue;
            if (sc.opts.debug_only_t && (int)sc.opts.debug_only_t - 1 != t) continue;
            L = L + bdpt_strategy<STAGED>(sc, pool, film, svs, evs, s, t, ctx, seed, sample_id, stack, ctr, bctr);
        }
#if defined(WTGPU_DEBUG_PRINT) && defined(__HIP_DEVICE_COMPILE__)
    if (ctx.element.x == 0 && ctx.element.y == 0)
        printf("dbg3 L=%g nT=%d nS=%d ch=%u rfs=%g r=%d\n", L.s[0], nT, nS, sc.sensor.channels, sc.sensor.rfilter_sigma, sc.sensor.rf_radius);
#endif
    film_splat(sc, film, ctx.element, L, ctx.k);
}

}   // namespace wt
