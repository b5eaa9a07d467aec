// wave_tracer_amd — first-hit material maps of a perspective sensor (wtgpu_first_hit_material / wtgpu_first_hit_material_host,
// csrc/kernels_firsthit_material.hip): what the material under a pixel is at up to four wavenumbers — diffuse albedo, specular reflectance of the
// smooth interface for the view direction, mask opacity, roughness, emitted radiance, and the material's index and leaf type.  The rays, the hit
// and the surface are wt/first_hit.h's (fh_ray, ads_intersect_ray, make_surface), the material is the integrators' (wt/bsdf.h: material_resolve,
// material_reflectance, material_IOR; wt/polar.h: fresnel, fresnel_reflection) and the radiance is the emitters' (wt/sources.h:
// area_spectral_radiance): nothing is restated here.  The device kernels and the host twin run fhm_sample, seq_add and fh_hit_mean, so they agree
// bit for bit (a function texture with libm opcodes excepted: wt/scene.h texture_function).
#pragma once
#include "bsdf.h"
#include "first_hit.h"

namespace wt {

// bits of wtgpu_first_hit_material_spec::maps, in the order of the maps of a pixel (each n_k floats), and of ::ids
enum first_hit_material_map_e : uint32_t { FHM_ALBEDO = 1, FHM_SPECULAR = 2, FHM_OPACITY = 4, FHM_ROUGHNESS = 8, FHM_EMISSION = 16, FHM_ALL_MAPS = 31 };
enum first_hit_material_id_e : uint32_t { FHM_MATERIAL = 1, FHM_TYPE = 2, FHM_ALL_IDS = 3 };
constexpr uint32_t kFhmMaps = 5, kFhmMaxK = 4;
constexpr uint32_t kFhmFloats = kFhmMaps * kFhmMaxK;   // the floats of a sample, all maps at four wavenumbers: float [map * kFhmMaxK + j]

// the spec after its checks
struct fhm_query_t {
    uint32_t samples, maps, ids, n_k;
    float k[kFhmMaxK];   // [1/mm]
    uint64_t seed;
};

WT_HD uint32_t fhm_bit_count(uint32_t bits) {
    uint32_t n = 0;
#pragma unroll
    for (uint32_t i = 0; i < kFhmMaps; ++i) n += (bits >> i) & 1u;
    return n;
}
WT_HD uint32_t fhm_map_floats(uint32_t maps, uint32_t n_k) { return fhm_bit_count(maps & FHM_ALL_MAPS) * n_k; }
WT_HD uint32_t fhm_id_words(uint32_t ids) { return (ids & FHM_MATERIAL ? 1u : 0u) + (ids & FHM_TYPE ? 1u : 0u); }
// where value j of map i (bit 1 << i) goes among the pixel's floats: the maps of the lower bits, n_k floats each, then j
WT_HD uint32_t fhm_slot(uint32_t maps, uint32_t n_k, uint32_t i, uint32_t j) { return fhm_bit_count(maps & ((1u << i) - 1u)) * n_k + j; }

// what one sample sees
struct fhm_sample_t {
    uint32_t material, type;
    float v[kFhmFloats];
};
// the running sums of a pixel over its hitting samples, and the ids of the first of them
struct fhm_sums_t {
    uint32_t n_hit;
    uint32_t material, type;
    float v[kFhmFloats];
};

// The unpolarised power reflectance of the smooth interface of a dielectric or surface_spm material for the local view direction wi (after the
// two-sided flip): with transmission the reflection share material_sample and material_pdf_leaf use, 1 - (Ts + Tp) / 2 at Re(eta); for a
// conductor or lossy wall (|rs|^2 + |rp|^2) / 2 at the complex eta, 0 from behind (fresnel_reflection).
WT_HD float fhm_interface_reflectance(const scene_t& sc, const material_t& m, vec3 wi, float k) {
    const cplx eta = material_IOR(sc, m, k);
    if (IOR_has_transmission(eta)) {
        const fresnel_t f = fresnel(cplx{eta.re, 0.f}, wi, vec3{0, 0, 1});
        return 1.f - (f.Ts + f.Tp) / 2.f;
    }
    const fresnel_conductor_t f = fresnel_reflection(eta, wi, vec3{0, 0, 1});
    return (cnorm(f.rs) + cnorm(f.rp)) * 0.5f;
}

// The maps of one sample at one wavenumber: v[i] is map i (0 where the bit is not set: nothing of it is evaluated); type: the leaf type,
// 0xFFFFFFFF without a BSDF at k.  uv: the surface's; wi: the view direction in the shading frame; emitter: the shape's area emitter seen from
// its front, or -1.
struct fhm_values_t {
    float v[kFhmMaps];
    uint32_t type;
};
template <bool specular>
WT_HD fhm_values_t fhm_eval(const scene_t& sc, uint32_t maps, int mat, vec2 uv, vec3 wi, int emitter, float k) {
    fhm_values_t r;
#pragma unroll
    for (uint32_t i = 0; i < kFhmMaps; ++i) r.v[i] = 0.f;
    r.type = 0xFFFFFFFFu;
    if (emitter >= 0) {   // (does not depend on the BSDF; area_spectral_radiance reads the surface's uv only)
        surface_t srf;
        srf.uv = uv;
        r.v[4] = area_spectral_radiance(sc, sc.emitters[emitter], srf, k);
    }
    material_t m;
    material_wrap_t wr;
    if (!material_resolve(sc, mat, k, uv, m, wr)) return r;
    r.type = (uint32_t)m.type;
    if (m.two_sided) wi = two_sided_flip(wi, wi.z);
    const float a = wr.masked ? wr.alpha : 1.f;
    if ((maps & FHM_ALBEDO) && m.type == MAT_DIFFUSE && wi.z > 0.f) r.v[0] = material_reflectance(sc, m, k, uv) * m.scale * a;
    if (specular && (m.type == MAT_DIELECTRIC || m.type == MAT_SURFACE_SPM) && wi.z != 0.f)
        r.v[1] = fhm_interface_reflectance(sc, m, wi, k) * m.refl_scale * m.scale * a;
    if (maps & FHM_OPACITY) r.v[2] = a;
    if ((maps & FHM_ROUGHNESS) && m.type == MAT_SURFACE_SPM) r.v[3] = m.roughness;
    return r;
}

// wavenumber J of a sample, if it is asked for
template <bool specular, uint32_t J>
WT_HD void fhm_sample_k(const scene_t& sc, const fhm_query_t& q, int mat, vec2 uv, vec3 wi, int emitter, fhm_sample_t& r) {
    if (J >= q.n_k) return;
    const fhm_values_t e = fhm_eval<specular>(sc, q.maps, mat, uv, wi, emitter, q.k[J]);
    if (J == 0) r.type = e.type;
#pragma unroll
    for (uint32_t i = 0; i < kFhmMaps; ++i) r.v[i * kFhmMaxK + J] = e.v[i];
}

// Sample s of a pixel: FALSE if its ray hits nothing (r is then all 0 and no id).  specular: the SPECULAR bit is set (else no Fresnel code).
template <bool specular>
WT_HD bool fhm_sample(const scene_t& sc, const fhm_query_t& q, uint32_t px, uint32_t py, uint32_t s, const stack_ref_t& stack, fhm_sample_t& r) {
    r.material = r.type = 0xFFFFFFFFu;
#pragma unroll
    for (uint32_t j = 0; j < kFhmFloats; ++j) r.v[j] = 0.f;
    vec3 ro, rd;
    fh_ray(sc.sensor, px, py, q.samples, s, q.seed, ro, rd);
    ray_hit_t h;
    if (!ads_intersect_ray(sc, ro, rd, range_t{0.f, WT_INF}, stack, h)) return false;
    const vec3 wp = ro + rd * h.dist;
    const surface_t srf = make_surface(sc, h.tuid, sc.tri_geo[h.tuid].n, vec2{h.bx, h.by}, wp);
    const shape_t sh = sc.shapes[srf.shape];
    const vec3 wi = to_local(srf.shading, -rd);
    const int emitter = ((q.maps & FHM_EMISSION) && sh.emitter >= 0 && dot(-rd, srf.geo.n) > 0.f) ? sh.emitter : -1;
    r.material = (uint32_t)sh.material;
    // One copy of the material layer per wavenumber, each under its j < n_k guard, so that every value has a register of its own.  (Written out:
    // asked to unroll a loop over j the compiler declines — four copies are beyond its size limit — and r.v, indexed by j, moves to scratch.)
    fhm_sample_k<specular, 0>(sc, q, sh.material, srf.uv, wi, emitter, r);
    fhm_sample_k<specular, 1>(sc, q, sh.material, srf.uv, wi, emitter, r);
    fhm_sample_k<specular, 2>(sc, q, sh.material, srf.uv, wi, emitter, r);
    fhm_sample_k<specular, 3>(sc, q, sh.material, srf.uv, wi, emitter, r);
    return true;
}

// A pixel by one thread: its samples in order, each hit added to the sums.
template <bool specular>
WT_HD fhm_sums_t fhm_pixel(const scene_t& sc, const fhm_query_t& q, uint32_t px, uint32_t py, const stack_ref_t& stack) {
    fhm_sums_t a;
    a.n_hit = 0;
    a.material = a.type = 0xFFFFFFFFu;
#pragma unroll
    for (uint32_t j = 0; j < kFhmFloats; ++j) a.v[j] = 0.f;
    const uint32_t n = q.samples ? q.samples : 1u;
    for (uint32_t s = 0; s < n; ++s) {
        fhm_sample_t r;
        if (!fhm_sample<specular>(sc, q, px, py, s, stack, r)) continue;
        const bool first = a.n_hit == 0;
        if (first) a.material = r.material, a.type = r.type;
#pragma unroll
        for (uint32_t j = 0; j < kFhmFloats; ++j) a.v[j] = seq_add(first, a.v[j], r.v[j]);
        ++a.n_hit;
    }
    return a;
}

// The pixel's K floats and Ki ids, contiguous, in bit order.  m / id may be null when no bit of theirs is set.
WT_HD void fhm_write(const fhm_sums_t& a, const fhm_query_t& q, float* m, uint32_t* id) {
#pragma unroll
    for (uint32_t i = 0; i < kFhmMaps; ++i)
#pragma unroll
        for (uint32_t j = 0; j < kFhmMaxK; ++j)
            if (((q.maps >> i) & 1u) && j < q.n_k) *m++ = fh_hit_mean(a.v[i * kFhmMaxK + j], a.n_hit);   // (the slots come in this order)
    if (q.ids & FHM_MATERIAL) *id++ = a.material;
    if (q.ids & FHM_TYPE) *id++ = a.type;
}

}   // namespace wt
