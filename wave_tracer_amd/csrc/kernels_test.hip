// wave_tracer_amd — test entry points of the wave-cooperative diffraction kernels (wtgpu_test_hooks.h; see wtgpu_kernels.h for the list of kernel
// translation units).  Each runs the cooperative form and the sequential form it replaces on the same explicit queries (wt/diffraction_probe.h:
// layouts), one query at a time; the material layer's queries run in the generic or the class form (wt/bsdf_probe.h); the emitter / sensor /
// wavenumber layer's one op per query (wt/sources_probe.h), the region power integral's likewise (wt/flux_probe.h).  No render kernel is compiled here.
#include "wt/bsdf_probe.h"
#include "wt/diffraction_probe.h"
#include "wt/flux_probe.h"
#include "wt/sources_probe.h"
#include "wtgpu_kernels.h"

namespace wtk {

// One 64-thread block per query.  mode 0: coop_build_aperture (wt/coop_fsd.h, the k_edges form); mode 1: the sequential build on lane 0.
// Every query owns the segment pool segs[q * pool_cap, (q + 1) * pool_cap): its allocator starts at 0 and refuses requests beyond pool_cap.
__global__ void __launch_bounds__(64) k_test_fsd_apertures(scene_t sc, const float* cones, const float* sk, const uint32_t* ids, const uint32_t* n_ids,
                                                           uint32_t id_cap, uint32_t pool_cap, uint32_t mode, uint32_t* hdr, fsd_edge_t* segs) {
    __shared__ uint32_t edge_counter;
    const uint32_t q = blockIdx.x;
    if (threadIdx.x == 0) edge_counter = 0;
    __syncthreads();
    const cone_t beam = probe_cone(cones + (size_t)q * 10);
    const vec2 sigma{sk[3 * q], sk[3 * q + 1]};
    const float k = sk[3 * q + 2];
    const uint32_t* eids = ids + (size_t)q * id_cap;
    const uint32_t n = n_ids[q] < id_cap ? n_ids[q] : id_cap;
    const fsd_pool_t pool{nullptr, segs + (size_t)q * pool_cap, nullptr, 1u, &edge_counter, pool_cap};
    fsd_aperture_t ap;
    if (mode == 0) {
        const bool ok = coop_build_aperture(sc, cone_frame(beam), k, beam, eids, n, sigma, pool, 0u, ap);
        if (threadIdx.x == 0) probe_fsd_header(ok, ap, hdr + (size_t)q * kFsdProbeWords);
    } else if (threadIdx.x == 0) {
        const bool ok = probe_fsd_sequential(sc, beam, k, sigma, eids, n, pool, 0u, ap);
        probe_fsd_header(ok, ap, hdr + (size_t)q * kFsdProbeWords);
    }
}

// One lane per query: utd_build_aperture, the per-wedge decisions and path_do_fsd (header word 7).
__global__ void __launch_bounds__(64) k_test_utd_build(scene_t sc, const float* queries, const uint32_t* ids, const uint32_t* n_ids, uint32_t id_cap,
                                                       uint32_t n, uint32_t utd_cap, utd_edge_rec_t* recs, uint32_t* hdr, uint32_t* edges) {
    __shared__ stack_entry_t lds[kLdsStack * 64];
    stack_entry_t spill[kSpillStack];
    stack_ref_t stack;
    lds_stack(lds, spill, stack, 64u);
    const uint32_t q = blockIdx.x * 64 + threadIdx.x;
    if (q >= n) return;
    const utd_probe_query_t Q = utd_probe_query(queries + (size_t)q * kUtdProbeQueryFloats);
    const uint32_t m = n_ids[q] < id_cap ? n_ids[q] : id_cap;
    utd_edge_rec_t* r = recs + (size_t)q * utd_cap;
    utd_aperture_t ap;
    probe_utd_build(sc, Q, ids + (size_t)q * id_cap, m, utd_cap, r, ap);
    uint32_t* h = hdr + (size_t)q * kUtdProbeWords;
    probe_utd_terms(sc, Q, ap, r, stack, h, edges + (size_t)q * utd_cap * kUtdProbeEdgeWords);
    const float f = probe_utd_sequential(sc, Q, ap, r, stack);
    h[7] = probe_bits(f);
}

// 64 / G queries per 64-thread block, G lanes each (k_path_fsd's layout): coop_do_fsd<G> on the apertures k_test_utd_build left behind.  The groups
// past the last query hold no aperture and only take part in the shuffles (have = false), like the tail of k_path_fsd's queue.
template <int G>
__global__ void __launch_bounds__(64) k_test_utd_coop(scene_t sc, const float* queries, uint32_t n, uint32_t utd_cap, const utd_edge_rec_t* recs,
                                                      uint32_t* hdr, uint32_t word) {
    __shared__ stack_entry_t lds[kLdsStack * 64];
    stack_entry_t spill[kSpillStack];
    stack_ref_t stack;
    lds_stack(lds, spill, stack, 64u);
    const uint32_t q = blockIdx.x * (64u / G) + threadIdx.x / G;
    const bool have = q < n;
    const uint32_t qq = have ? q : 0u;
    const utd_probe_query_t Q = utd_probe_query(queries + (size_t)qq * kUtdProbeQueryFloats);
    utd_aperture_t ap;
    memset(&ap, 0, sizeof(ap));
    if (have) {
        ap.n_edges = hdr[(size_t)q * kUtdProbeWords];
        ap.overflow = hdr[(size_t)q * kUtdProbeWords + 1];
        ap.k = Q.k;
        ap.interaction_wp = Q.iwp;
        ap.edge_cap = utd_cap;
    }
    const float f = coop_do_fsd<G>(sc, Q.src_cone, path_geo_point(Q.src_cone.o), Q.dst, ap, recs + (size_t)qq * utd_cap, Q.k, stack, nullptr, have);
    if (have && (threadIdx.x & (G - 1)) == 0) hdr[(size_t)q * kUtdProbeWords + word] = probe_bits(f);
}

// One lane per material query (wt/bsdf_probe.h); `form`: -1 generic, else the class form of that leaf type.
template <int CLS>
__global__ void __launch_bounds__(64) k_test_bsdf(scene_t sc, const uint32_t* queries, uint32_t n, uint32_t* out) {
    const uint32_t q = blockIdx.x * 64 + threadIdx.x;
    if (q >= n) return;
    probe_bsdf<CLS>(sc, queries + (size_t)q * kBsdfProbeQueryWords, out + (size_t)q * kBsdfProbeWords);
}

// One lane per query of the emitter / sensor / wavenumber layer (wt/sources_probe.h).
__global__ void __launch_bounds__(64) k_test_sources(scene_t sc, const uint32_t* queries, uint32_t n, uint32_t* out) {
    const uint32_t q = blockIdx.x * 64 + threadIdx.x;
    if (q >= n) return;
    probe_source(sc, queries + (size_t)q * kSourceProbeQueryWords, out + (size_t)q * kSourceProbeWords);
}

// One lane per query of the region power integral (wt/flux_probe.h).
__global__ void __launch_bounds__(64) k_test_flux(scene_t sc, const uint32_t* queries, uint32_t n, uint32_t* out) {
    const uint32_t q = blockIdx.x * 64 + threadIdx.x;
    if (q >= n) return;
    probe_flux(sc, queries + (size_t)q * kFluxProbeQueryWords, out + (size_t)q * kFluxProbeWords);
}

int test_fsd_apertures(const scene_t& sc, hipStream_t stream, const float* d_cones, const float* d_sk, const uint32_t* d_ids, const uint32_t* d_n_ids,
                       uint32_t n, uint32_t id_cap, uint32_t pool_cap, uint32_t mode, uint32_t* d_hdr, float* d_segs) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_test_fsd_apertures, dim3(n), dim3(64), 0, stream, sc, d_cones, d_sk, d_ids, d_n_ids, id_cap, pool_cap, mode, d_hdr,
                       reinterpret_cast<fsd_edge_t*>(d_segs));
    return (int)hipGetLastError();
}

int test_utd_sums(const scene_t& sc, hipStream_t stream, const float* d_queries, const uint32_t* d_ids, const uint32_t* d_n_ids, uint32_t n, uint32_t id_cap,
                  uint32_t utd_cap, uint32_t* d_recs, uint32_t* d_hdr, uint32_t* d_edges) {
    if (n == 0) return 0;
    utd_edge_rec_t* recs = reinterpret_cast<utd_edge_rec_t*>(d_recs);
    hipLaunchKernelGGL(k_test_utd_build, dim3((n + 63) / 64), dim3(64), 0, stream, sc, d_queries, d_ids, d_n_ids, id_cap, n, utd_cap, recs, d_hdr, d_edges);
    hipLaunchKernelGGL(k_test_utd_coop<1>, dim3((n + 63) / 64), dim3(64), 0, stream, sc, d_queries, n, utd_cap, recs, d_hdr, 4u);
    hipLaunchKernelGGL(k_test_utd_coop<8>, dim3((n + 7) / 8), dim3(64), 0, stream, sc, d_queries, n, utd_cap, recs, d_hdr, 5u);
    hipLaunchKernelGGL(k_test_utd_coop<64>, dim3(n), dim3(64), 0, stream, sc, d_queries, n, utd_cap, recs, d_hdr, 6u);
    return (int)hipGetLastError();
}

int test_bsdf_queries(const scene_t& sc, hipStream_t stream, const uint32_t* d_queries, uint32_t n, int form, uint32_t* d_out) {
    if (n == 0) return 0;
    const dim3 grid((n + 63) / 64), block(64);
    switch (form) {
        case MAT_DIFFUSE: hipLaunchKernelGGL(k_test_bsdf<MAT_DIFFUSE>, grid, block, 0, stream, sc, d_queries, n, d_out); break;
        case MAT_DIELECTRIC: hipLaunchKernelGGL(k_test_bsdf<MAT_DIELECTRIC>, grid, block, 0, stream, sc, d_queries, n, d_out); break;
        case MAT_SURFACE_SPM: hipLaunchKernelGGL(k_test_bsdf<MAT_SURFACE_SPM>, grid, block, 0, stream, sc, d_queries, n, d_out); break;
        default: hipLaunchKernelGGL(k_test_bsdf<-1>, grid, block, 0, stream, sc, d_queries, n, d_out); break;
    }
    return (int)hipGetLastError();
}

int test_source_queries(const scene_t& sc, hipStream_t stream, const uint32_t* d_queries, uint32_t n, uint32_t* d_out) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_test_sources, dim3((n + 63) / 64), dim3(64), 0, stream, sc, d_queries, n, d_out);
    return (int)hipGetLastError();
}

int test_flux_queries(const scene_t& sc, hipStream_t stream, const uint32_t* d_queries, uint32_t n, uint32_t* d_out) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_test_flux, dim3((n + 63) / 64), dim3(64), 0, stream, sc, d_queries, n, d_out);
    return (int)hipGetLastError();
}

}   // namespace wtk
