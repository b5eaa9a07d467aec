// wave_tracer_amd — per-query probes of the diffraction code for the tests (host and device): the device hooks wtgpu_test_fsd_apertures /
// wtgpu_test_utd_sums (kernels_test.hip) and their CPU-checker counterparts oracle_fsd_apertures / oracle_utd_sums (oracle/oracle.cpp) share
// the query layouts and the sequential forms below, so that their outputs can be compared position by position.  No render path includes this.
//
// Fraunhofer query: beam cone (10 floats, the layout of wtgpu_query_regions: o, d, tan_alpha, x0, eccentricity, wavelength [m]), {sigma.x,
// sigma.y, k}, an edge-id list.  Output header (kFsdProbeWords words): ok, n_edges, overflow, dead, P0, P0_pdf, psi02 (f32 bits), edge_cap;
// then the segment records (fsd_edge_t) at [0, n_edges) of the query's own segment pool.
// UTD query (kUtdProbeQueryFloats floats): source cone (10), destination point (3), interaction point (3), region frame t, b, n (9), region
// size (3), wi (3), k.  Output header (kUtdProbeWords words): n_edges, overflow, direct (bit 0: the source cone contains the destination,
// bit 1: the direct path is shadowed), direct phase argument, (|ts|^2 + |th|^2) / 2 of coop_do_fsd<1>, <8>, <64> and of path_do_fsd; per
// wedge (kUtdProbeEdgeWords words): bit 0 utd_f_edge accepted it, bit 1 / bit 2 the shadow ray to the source / the destination is blocked,
// the phase argument k_times_len(k, ro + ri), Ds, Dh, ri, ro.
#pragma once
#include "path.h"

namespace wt {

constexpr uint32_t kFsdProbeWords = 8;
constexpr uint32_t kFsdProbeSegWords = sizeof(fsd_edge_t) / 4;
constexpr uint32_t kUtdProbeQueryFloats = 32;
constexpr uint32_t kUtdProbeWords = 8;
constexpr uint32_t kUtdProbeEdgeWords = 8;
static_assert(kFsdProbeSegWords == 7, "fsd_edge_t layout of the probe output");

WT_HD uint32_t probe_bits(float f) {
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    return u;
}
WT_HD cone_t probe_cone(const float* c) {
    const vec3 d = normalize(vec3{c[3], c[4], c[5]});
    return make_cone(vec3{c[0], c[1], c[2]}, d, build_orthogonal_frame(d).t, c[6], c[8], c[7]);
}

// The sequential aperture as bdpt_walk_step builds it (wt/bdpt.h): an upper bound of the segment count sizes the allocation, then
// fsd_build_aperture in the beam's own frame.  This is the path of every aperture when WTGPU_COOP_APERTURE_MIN exceeds its edge count.
template <class Ids>
WT_HD bool probe_fsd_sequential(const scene_t& sc, const cone_t& beam, float k, vec2 sigma, const Ids& eids, uint32_t n_ids, const fsd_pool_t& pool,
                                uint32_t slot, fsd_aperture_t& ap) {
    const frame_t fr = cone_frame(beam);
    const vec2 cse = sigma * kBeamEnvelope;
    const float max_len = .33f * fmaxf_(cse.x, cse.y);
    uint32_t need = 0;
    for (uint32_t i = 0; i < n_ids; ++i) need += fsd_count_segments(sc, fr, beam, cse, max_len, eids[i]);
    const bool ok = fsd_pool_alloc_edges(pool, slot, need, ap);
    const fsd_edges_ref_t ed{pool.edges + (size_t)ap.edge_offset, 1};
    fsd_build_aperture(sc, fr, k, 1.f, beam, eids, n_ids, sigma, ap, ed);
    return ok;
}
WT_HD void probe_fsd_header(bool ok, const fsd_aperture_t& ap, uint32_t* hdr) {
    hdr[0] = ok ? 1u : 0u;
    hdr[1] = ap.n_edges;
    hdr[2] = ap.overflow;
    hdr[3] = ap.dead;
    hdr[4] = probe_bits(ap.P0);
    hdr[5] = probe_bits(ap.P0_pdf);
    hdr[6] = probe_bits(ap.psi02);
    hdr[7] = ap.edge_cap;
}

struct utd_probe_query_t {
    cone_t src_cone;
    vec3 dst, iwp;
    frame_t rframe;
    vec3 rsize, wi;
    float k;
};
WT_HD utd_probe_query_t utd_probe_query(const float* q) {
    utd_probe_query_t Q;
    Q.src_cone = probe_cone(q);
    Q.dst = vec3{q[10], q[11], q[12]};
    Q.iwp = vec3{q[13], q[14], q[15]};
    Q.rframe = frame_t{{q[16], q[17], q[18]}, {q[19], q[20], q[21]}, {q[22], q[23], q[24]}};
    Q.rsize = vec3{q[25], q[26], q[27]};
    Q.wi = vec3{q[28], q[29], q[30]};
    Q.k = q[31];
    return Q;
}
// utd_build_aperture into `recs` (utd_cap records: wedges beyond are counted in ap.overflow)
template <class Ids>
WT_HD void probe_utd_build(const scene_t& sc, const utd_probe_query_t& Q, const Ids& eids, uint32_t n_ids, uint32_t utd_cap, utd_edge_rec_t* recs,
                           utd_aperture_t& ap) {
    ap.edge_offset = 0;
    ap.edge_cap = utd_cap;
    utd_build_aperture(sc, Q.iwp, Q.rframe, Q.rsize, Q.wi, Q.k, eids, n_ids, ap, utd_edges_ref_t{recs, 1});
}
// what path_do_fsd / coop_do_fsd decide per wedge and for the direct path (both shadow rays of every accepted wedge are traced here)
WT_HD void probe_utd_terms(const scene_t& sc, const utd_probe_query_t& Q, const utd_aperture_t& ap, const utd_edge_rec_t* recs, const stack_ref_t& stack,
                           uint32_t* hdr, uint32_t* edges) {
    const vec3 src = Q.src_cone.o;
    const path_geo_t src_geo = path_geo_point(src), dst_geo = path_geo_point(Q.dst);
    for (uint32_t i = 0; i < ap.n_edges; ++i) {
        uint32_t* o = edges + (size_t)i * kUtdProbeEdgeWords;
        for (uint32_t w = 0; w < kUtdProbeEdgeWords; ++w) o[w] = 0u;
        utd_diffracting_edge_t f;
        if (!utd_f_edge(sc, ap, recs[i], src, Q.dst, f)) continue;
        const path_geo_t eintr = path_geo_edge(f.edge, f.p);
        const bool s_src = path_shadow(sc, eintr, src_geo, stack, nullptr), s_dst = path_shadow(sc, eintr, dst_geo, stack, nullptr);
        o[0] = 1u | (s_src ? 2u : 0u) | (s_dst ? 4u : 0u);
        o[1] = probe_bits(k_times_len(Q.k, f.ro + f.ri));
        o[2] = probe_bits(f.utd.Ds.re);
        o[3] = probe_bits(f.utd.Ds.im);
        o[4] = probe_bits(f.utd.Dh.re);
        o[5] = probe_bits(f.utd.Dh.im);
        o[6] = probe_bits(f.ri);
        o[7] = probe_bits(f.ro);
    }
    hdr[0] = ap.n_edges;
    hdr[1] = ap.overflow;
    const bool in = cone_contains(Q.src_cone, Q.dst);
    const bool shadowed = in && path_shadow(sc, src_geo, dst_geo, stack, nullptr);
    hdr[2] = (in ? 1u : 0u) | (shadowed ? 2u : 0u);
    hdr[3] = probe_bits(k_times_len(Q.k, length(Q.dst - src)));
}
// the sequential sum (path_do_fsd) reduced like coop_do_fsd's result
WT_HD float probe_utd_sequential(const scene_t& sc, const utd_probe_query_t& Q, const utd_aperture_t& ap, utd_edge_rec_t* recs, const stack_ref_t& stack) {
    const cpair_t t = path_do_fsd(sc, Q.src_cone, path_geo_point(Q.src_cone.o), Q.dst, ap, utd_edges_ref_t{recs, 1}, Q.k, stack, nullptr);
    return (cnorm(t.ts) + cnorm(t.th)) / 2.f;
}

}   // namespace wt
