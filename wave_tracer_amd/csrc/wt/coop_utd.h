// wave_tracer_amd — the coherent UTD sum of one aperture by a group of lanes (device only): k_path_fsd / k_path_nee (kernels_path.hip) and the
// test entry point wtgpu_test_utd_sums (kernels_test.hip) include it.  The sequential form it replaces is path_do_fsd (wt/path.h).
#pragma once
#if defined(__HIPCC__)
#include "coop.h"
#include "path.h"

namespace wt {

// do_fsd (plt_path_detail.hpp:311-346) by ONE WAVEFRONT: lane = wedge (strided over apertures of any size) — the Fermat point on the wedge, the
// UTD coefficients and the two shadow rays (per-lane any-hit traversals on the lane's LDS stack) — coherent sums in f64 by wave reduction; the
// direct path is evaluated redundantly by all lanes (uniform control flow).  Returns (|ts|^2 + |th|^2) / 2.
// G: lanes per aperture (a power of two <= 64; the 64 / G apertures of a wavefront are independent: shuffles stay inside an aligned group of G lanes).
template <int G>
WT_D float coop_do_fsd(const scene_t& sc, const cone_t& cone_from_src, const path_geo_t& src_geo, vec3 dst, const utd_aperture_t& ap, const utd_edge_rec_t* recs,
                                    float k, const stack_ref_t& stack, bdpt_counters_t* ctr, bool have = true) {   // have = false: the group holds no aperture (it only takes part in the shuffles)
    const int lane = threadIdx.x & (G - 1);
    const vec3 src = cone_from_src.o;
    const path_geo_t dst_geo = path_geo_point(dst);
    double tsr = 0, tsi = 0, thr = 0, thi = 0;
    for (uint32_t i = (uint32_t)lane; have && i < ap.n_edges; i += (uint32_t)G) {
        utd_diffracting_edge_t f;
        WT_WATCH_ADD(12);
        if (lane == 0) WT_WATCH(13, i);
        if (lane == 0) WT_WATCH(14, ap.n_edges);
        if (lane == 0) WT_WATCH(5, i);
        if (!utd_f_edge(sc, ap, recs[i], src, dst, f)) continue;
        if (lane == 0) WT_WATCH(6, i);
        const path_geo_t eintr = path_geo_edge(f.edge, f.p);
        WT_WATCH_ADD(15);
        if (path_shadow(sc, eintr, src_geo, stack, ctr) || path_shadow(sc, eintr, dst_geo, stack, ctr)) continue;
        const cplx phase = cpolar(1.f, -k_times_len(k, f.ro + f.ri));
        const cplx a = phase * f.utd.Ds, b = phase * f.utd.Dh;
        tsr += a.re;
        tsi += a.im;
        thr += b.re;
        thi += b.im;
    }
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) {
        tsr += __shfl_xor(tsr, off, 64);
        tsi += __shfl_xor(tsi, off, 64);
        thr += __shfl_xor(thr, off, 64);
        thi += __shfl_xor(thi, off, 64);
    }
    cplx ts{(float)tsr, (float)tsi}, th{(float)thr, (float)thi};
    if (have && cone_contains(cone_from_src, dst)) {
        bdpt_counters_t* c0 = lane == 0 ? ctr : nullptr;
        if (!path_shadow(sc, src_geo, dst_geo, stack, c0)) {
            const cplx phase = cpolar(1.f, -k_times_len(k, length(dst - src)));
            ts = ts + phase;
            th = th + phase;
        }
    }
    return (cnorm(ts) + cnorm(th)) / 2.f;
}

}   // namespace wt
#endif
