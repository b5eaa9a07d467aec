// wave_tracer_amd — per-query probe of the material layer (wt/bsdf.h) for the tests (host and device): the device hook wtgpu_test_bsdf_queries
// (kernels_test.hip: k_test_bsdf) and its CPU-checker counterpart oracle_bsdf_queries (oracle/oracle.cpp) share the layouts and the function
// below, so that their outputs can be compared word by word.  No render path includes this.
//
// Query (kBsdfProbeQueryWords 32-bit words): material id, wi (3), wo (3) in the local shading frame, k [1/mm], transport, uv (2), sampler
// seed (lo, hi), sample id (lo, hi), stream, start draw, 0.
// Output (kBsdfProbeWords words, f32 bits unless stated):
//   [0]       flags (u32): bit 0 the form applies (the class form: an unwrapped material of that leaf type), bit 1 material_sample's `valid`
//   [1, 17)   material_f(wi, wo) (row-major Mueller)
//   [17]      material_pdf(wi, wo)
//   [18, 21)  sampled wo;  [21] tagged dpd;  [22] eta;  [23, 39) weighted bsdf M
//   [39]      material_pdf(sampled wo, wi) with the flipped transport: the reverse density bdpt_surface_step stores
//   [40]      draws the sample consumed (u32)
//   [41, 47)  the first 6 uniforms of the query's stream from its start draw (a copy of the sampler): an f64 restatement replays the sample
//             map from them
//   [47]      0
// Form: -1 the generic material_f / material_pdf / material_sample; MAT_DIFFUSE, MAT_DIELECTRIC, MAT_SURFACE_SPM the class forms of the
// material-sorted interaction pass (material_pdf<CLS>, material_sample<CLS>; material_f has no class form: both forms write the generic
// one).  A class form on a material of another type or on a wrapper writes flags = 0 and zeros.
#pragma once
#include "bsdf.h"

namespace wt {

constexpr uint32_t kBsdfProbeQueryWords = 18;
constexpr uint32_t kBsdfProbeWords = 48;
constexpr uint32_t kBsdfProbeUniforms = 6;

WT_HD uint32_t bsdf_probe_bits(float f) {
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    return u;
}
WT_HD float bsdf_probe_float(uint32_t u) {
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}

template <int CLS>
WT_HD void probe_bsdf(const scene_t& sc, const uint32_t* q, uint32_t* out) {
    for (uint32_t i = 0; i < kBsdfProbeWords; ++i) out[i] = 0u;
    const int mat = (int)q[0];
    if (CLS >= 0 && sc.materials[mat].type != CLS) return;
    const vec3 wi{bsdf_probe_float(q[1]), bsdf_probe_float(q[2]), bsdf_probe_float(q[3])};
    const vec3 wo{bsdf_probe_float(q[4]), bsdf_probe_float(q[5]), bsdf_probe_float(q[6])};
    const float k = bsdf_probe_float(q[7]);
    const uint32_t transport = q[8];
    const vec2 uv{bsdf_probe_float(q[9]), bsdf_probe_float(q[10])};
    const uint64_t seed = (uint64_t)q[11] | ((uint64_t)q[12] << 32), sample_id = (uint64_t)q[13] | ((uint64_t)q[14] << 32);
    const uint32_t stream = q[15], draw0 = q[16];
    uint32_t flags = 1u;
    {
        const mueller_t F = material_f(sc, mat, wi, wo, k, transport, uv);
        for (int i = 0; i < 16; ++i) out[1 + i] = bsdf_probe_bits(F.m[i]);
    }
    out[17] = bsdf_probe_bits(material_pdf<CLS>(sc, mat, wi, wo, k, transport, uv));
    sampler_t smp = make_sampler(seed, sample_id, stream, draw0);
    {
        sampler_t u = smp;
        for (uint32_t i = 0; i < kBsdfProbeUniforms; ++i) out[41 + i] = bsdf_probe_bits(sampler_r(u));
    }
    const bsdf_sample_t bs = material_sample<CLS>(sc, mat, wi, k, transport, smp, uv);
    if (bs.valid) flags |= 2u;
    out[18] = bsdf_probe_bits(bs.wo.x);
    out[19] = bsdf_probe_bits(bs.wo.y);
    out[20] = bsdf_probe_bits(bs.wo.z);
    out[21] = bsdf_probe_bits(bs.dpd);
    out[22] = bsdf_probe_bits(bs.eta);
    for (int i = 0; i < 16; ++i) out[23 + i] = bsdf_probe_bits(bs.M.m[i]);
    out[39] = bsdf_probe_bits(material_pdf<CLS>(sc, mat, bs.wo, wi, k, flip_transport(transport), uv));
    out[40] = smp.draws - draw0;
    out[0] = flags;
}

}   // namespace wt
