// wave_tracer_amd — per-query probe of the emitter / sensor / wavenumber layer (wt/sources.h) for the tests (host and device): the device hook
// wtgpu_test_source_queries (kernels_test.hip: k_test_sources) and its CPU-checker counterpart oracle_source_queries (oracle/oracle.cpp) share
// the layouts and the function below, so that their outputs can be compared word by word.  No render path includes this.
//
// Query (kSourceProbeQueryWords 32-bit words, f32 bits unless stated):
//   [0] op (u32, SRC_OP_*)   [1] i0 (u32): emitter index (spectrum .. Li), pixel x (sense)   [2] i1 (u32): pixel y (sense), tuid (Li)
//   [3] k [1/mm]   [4, 7) a world point: wp (emit_direct, sense_direct), the beam's origin (Li, Si)   [7, 10) a direction (Li, Si)
//   [10, 12) barycentrics (Li)   [12] an explicit uniform (kdist)   [13, 15) range min, max (Si)
//   [15, 17) sampler seed (lo, hi)   [17, 19) sample id (lo, hi)   [19] stream   [20] start draw   [21, 24) 0
// Output (kSourceProbeWords words, f32 bits unless stated):
//   [0]        A (u32): the emitter chosen (spectrum, emit_direct), `valid` (Si)
//   [1]        has_surface (u32)
//   [2]        draws the op consumed (u32)
//   [3, 11)    the first 8 uniforms of the query's stream from its start draw (a copy of the sampler): an f64 restatement replays the
//              sample maps from them
//   [11, 16)   scalars s0 .. s4, per op:
//                spectrum     emitter_pdf, k, tagged wpd, scene_sum_spectral_pdf(query k)
//                kdist        k, tagged wpd, kdist_pdf(query k), kdist_pdf(sampled k)
//                emit         tagged ppd, tagged dpd, emitter_pdf_position, emitter_pdf_direction (both at the sample)
//                emit_direct  emitter_pdf, tagged dpd
//                Li           the 4 Stokes words, emitter_pdf_position at the query's surface (a textured emitter: area_table_pdf)
//                sense        tagged ppd, tagged dpd, sensor_pdf_position, sensor_pdf_direction(beam direction)
//                sense_direct 0, tagged dpd, 0, sensor_pdf_direction(beam direction)
//   [16, 59)   the beam: envelope o (3), d (3), x (3), x0, tan_alpha, e, one_over_e, z_apex; k; self_intersection_distance; transport (u32);
//              frame t, b, n (9); scale; rad (16)
//   [59, 71)   the surface: wp (3), geo.n (3), uv (2), bary (2), tuid (u32), shape (u32)
//   [71, 75)   the sensor element: x (u32), y (u32), offset (2)
//   [75, 80)   0
// Words an op does not produce are 0.  A query whose op, emitter index or tuid is out of range writes zeros only.
//
// Words behind a libm call (device vs checker: compared within a bound; every other float word is bit-identical, both sides running the
// same f32 arithmetic with -ffp-contract=off and correctly rounded division and sqrtf):
//   emit          the beam's envelope o (directional: concentric_disk), d, x, frame and rad[0..4) (spot: cosf / sinf / acosf; point: cosf /
//                 sinf; area: cosf / sinf), the area emitter's tagged dpd and emitter_pdf_direction (cosine_hemisphere)
//   emit          textured area emitters: ceilf(sqrtf()) picks the cell -> the discrete decision, in the band
//   emit_direct   rad[0..4) of a spot (acosf in spot_falloff)
//   sense         virtual plane: d, x, frame, scale, tagged dpd, sensor_pdf_direction (cosine_hemisphere)
//   Li            none;  sense (perspective), sense_direct, Si, spectrum, kdist: none
#pragma once
#include "sources.h"

namespace wt {

enum source_probe_op_e : uint32_t {
    SRC_OP_SPECTRUM = 0, SRC_OP_KDIST = 1, SRC_OP_EMIT = 2, SRC_OP_EMIT_DIRECT = 3, SRC_OP_LI = 4, SRC_OP_SENSE = 5, SRC_OP_SENSE_DIRECT = 6,
    SRC_OP_SI = 7, SRC_OP_COUNT = 8
};
constexpr uint32_t kSourceProbeQueryWords = 24;
constexpr uint32_t kSourceProbeWords = 80;
constexpr uint32_t kSourceProbeUniforms = 8;
constexpr uint32_t kSourceProbeScalars = 11, kSourceProbeBeam = 16, kSourceProbeSurface = 59, kSourceProbeElement = 71;

WT_HD uint32_t source_probe_bits(float f) {
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    return u;
}
WT_HD float source_probe_float(uint32_t u) {
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}
WT_HD void source_probe_vec3(uint32_t* o, vec3 v) {
    o[0] = source_probe_bits(v.x);
    o[1] = source_probe_bits(v.y);
    o[2] = source_probe_bits(v.z);
}
WT_HD void source_probe_beam(uint32_t* out, const beam_t& b) {
    uint32_t* o = out + kSourceProbeBeam;
    source_probe_vec3(o, b.env.o);
    source_probe_vec3(o + 3, b.env.d);
    source_probe_vec3(o + 6, b.env.x);
    o[9] = source_probe_bits(b.env.x0);
    o[10] = source_probe_bits(b.env.tan_alpha);
    o[11] = source_probe_bits(b.env.e);
    o[12] = source_probe_bits(b.env.one_over_e);
    o[13] = source_probe_bits(b.env.z_apex);
    o[14] = source_probe_bits(b.k);
    o[15] = source_probe_bits(b.self_intersection_distance);
    o[16] = b.transport;
    source_probe_vec3(o + 17, b.frame.t);
    source_probe_vec3(o + 20, b.frame.b);
    source_probe_vec3(o + 23, b.frame.n);
    o[26] = source_probe_bits(b.scale);
    for (int i = 0; i < 16; ++i) o[27 + i] = source_probe_bits(b.rad[i]);
}
WT_HD void source_probe_surface(uint32_t* out, const surface_t& s) {
    uint32_t* o = out + kSourceProbeSurface;
    source_probe_vec3(o, s.wp);
    source_probe_vec3(o + 3, s.geo.n);
    o[6] = source_probe_bits(s.uv.x);
    o[7] = source_probe_bits(s.uv.y);
    o[8] = source_probe_bits(s.bary.x);
    o[9] = source_probe_bits(s.bary.y);
    o[10] = s.tuid;
    o[11] = s.shape;
}
WT_HD void source_probe_element(uint32_t* out, const sensor_element_t& e) {
    uint32_t* o = out + kSourceProbeElement;
    o[0] = e.x;
    o[1] = e.y;
    o[2] = source_probe_bits(e.offset.x);
    o[3] = source_probe_bits(e.offset.y);
}

// what a host entry point checks before it runs a query (the probe itself writes zeros for such a query)
WT_HD bool source_probe_query_ok(const scene_t& sc, const uint32_t* q) {
    const uint32_t op = q[0];
    if (op >= SRC_OP_COUNT) return false;
    if ((op == SRC_OP_KDIST || op == SRC_OP_EMIT || op == SRC_OP_LI) && q[1] >= sc.n_emitters) return false;
    if ((op == SRC_OP_SPECTRUM || op == SRC_OP_EMIT_DIRECT) && sc.n_emitters == 0) return false;
    if (op == SRC_OP_LI && q[2] >= sc.n_tris) return false;
    return true;
}

WT_HD void probe_source(const scene_t& sc, const uint32_t* q, uint32_t* out) {
    for (uint32_t i = 0; i < kSourceProbeWords; ++i) out[i] = 0u;
    if (!source_probe_query_ok(sc, q)) return;
    const uint32_t op = q[0], i0 = q[1], i1 = q[2];
    const float k = source_probe_float(q[3]);
    const vec3 p{source_probe_float(q[4]), source_probe_float(q[5]), source_probe_float(q[6])};
    const vec3 d{source_probe_float(q[7]), source_probe_float(q[8]), source_probe_float(q[9])};
    const vec2 bary{source_probe_float(q[10]), source_probe_float(q[11])};
    const float u = source_probe_float(q[12]);
    const range_t range{source_probe_float(q[13]), source_probe_float(q[14])};
    const uint64_t seed = (uint64_t)q[15] | ((uint64_t)q[16] << 32), sample_id = (uint64_t)q[17] | ((uint64_t)q[18] << 32);
    const uint32_t stream = q[19], draw0 = q[20];
    sampler_t smp = make_sampler(seed, sample_id, stream, draw0);
    {
        sampler_t c = smp;
        for (uint32_t i = 0; i < kSourceProbeUniforms; ++i) out[3 + i] = source_probe_bits(sampler_r(c));
    }
    uint32_t* s = out + kSourceProbeScalars;
    switch (op) {
    case SRC_OP_SPECTRUM: {
        const emitter_k_sample_t r = scene_sample_emitter_and_spectrum(sc, smp);
        out[0] = (uint32_t)r.emitter;
        s[0] = source_probe_bits(r.emitter_pdf);
        s[1] = source_probe_bits(r.wavenumber.k);
        s[2] = source_probe_bits(r.wavenumber.wpd);
        s[3] = source_probe_bits(scene_sum_spectral_pdf(sc, k));
    } break;
    case SRC_OP_KDIST: {
        const kdist_t kd = sc.kdists[sc.emitters[i0].k_dist];
        const wavenumber_sample_t r = kdist_sample(sc, kd, u);
        s[0] = source_probe_bits(r.k);
        s[1] = source_probe_bits(r.wpd);
        s[2] = source_probe_bits(kdist_pdf(sc, kd, k));
        s[3] = source_probe_bits(kdist_pdf(sc, kd, r.k));
    } break;
    case SRC_OP_EMIT: {
        const emitter_sample_t r = emitter_sample(sc, (int)i0, k, smp);
        out[1] = r.has_surface;
        s[0] = source_probe_bits(r.ppd);
        s[1] = source_probe_bits(r.dpd);
        s[2] = source_probe_bits(emitter_pdf_position(sc, (int)i0, r.has_surface ? &r.surface : nullptr));
        s[3] = source_probe_bits(emitter_pdf_direction(sc, (int)i0, r.beam.env.d, r.has_surface ? &r.surface : nullptr));
        source_probe_beam(out, r.beam);
        if (r.has_surface) source_probe_surface(out, r.surface);
    } break;
    case SRC_OP_EMIT_DIRECT: {
        const emitter_direct_sample_t r = scene_sample_emitter_direct(sc, p, k, smp);
        out[0] = (uint32_t)r.emitter;
        out[1] = r.has_surface;
        s[0] = source_probe_bits(r.emitter_pdf);
        s[1] = source_probe_bits(r.dpd);
        source_probe_beam(out, r.beam);
        if (r.has_surface) source_probe_surface(out, r.surface);
    } break;
    case SRC_OP_LI: {
        const beam_t S = make_backward_beam(p, d, 1.f, k, sg_source(0.f, 0.f, k));
        const surface_t surface = make_surface_at_bary(sc, i1, bary);
        const stokes_t L = emitter_Li(sc, (int)i0, S, surface);
        for (int i = 0; i < 4; ++i) s[i] = source_probe_bits(L.s[i]);
        s[4] = source_probe_bits(emitter_pdf_position(sc, (int)i0, &surface));
        out[1] = 1u;
        source_probe_surface(out, surface);
    } break;
    case SRC_OP_SENSE: {
        const sensor_sample_t r = sensor_sample(sc, i0, i1, k, smp);
        out[1] = r.has_surface;
        s[0] = source_probe_bits(r.ppd);
        s[1] = source_probe_bits(r.dpd);
        s[2] = source_probe_bits(sensor_pdf_position(sc));
        s[3] = source_probe_bits(sensor_pdf_direction(sc, r.beam.env.d));
        source_probe_beam(out, r.beam);
        source_probe_element(out, r.element);
        if (r.has_surface) source_probe_surface(out, r.surface);
    } break;
    case SRC_OP_SENSE_DIRECT: {
        const sensor_direct_sample_t r = sensor_sample_direct(sc, p, k, smp);
        out[1] = r.has_surface;
        s[1] = source_probe_bits(r.dpd);
        s[3] = source_probe_bits(sensor_pdf_direction(sc, r.beam.env.d));
        source_probe_beam(out, r.beam);
        source_probe_element(out, r.element);
        if (r.has_surface) source_probe_surface(out, r.surface);
    } break;
    default: {   // SRC_OP_SI
        if (sc.sensor.type != SENSOR_VIRTUAL_PLANE) break;
        const beam_t B = make_forward_beam(p, d, 1.f, k, sg_source(0.f, 0.f, k));
        const sensor_direct_connection_t r = vplane_Si(sc, B, range);
        out[0] = r.valid ? 1u : 0u;
        if (r.valid) {
            out[1] = 1u;
            source_probe_beam(out, r.beam);
            source_probe_element(out, r.element);
            source_probe_surface(out, r.surface);
        }
    } break;
    }
    out[2] = smp.draws - draw0;
}

}   // namespace wt
