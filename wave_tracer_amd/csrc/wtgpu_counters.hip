// wave_tracer_amd — the counters of a scene: wtgpu_get_counters with the profile printers of WTGPU_PROFILE and of the -DWTGPU_*_PROF builds, reset.
#include "wtgpu_host.h"

extern "C" {

int wtgpu_get_counters(wtgpu_scene* s, wtgpu_counters* out) {
    if (!s || !out || !s->uploaded) return fail(WTGPU_ERR_INVALID, "scene not uploaded");
    bdpt_counters_t c;
    {
        const int rc = drain_all(s);
        if (rc) return rc;
    }
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(&c, s->slices[0].counters, sizeof(c), hipMemcpyDeviceToHost));
    out->samples = s->samples_rendered;
    out->segments = c.segments;
    out->ray_queries = c.ray_queries;
    out->cone_queries = c.cone_queries;
    out->vertices = c.vertices;
    out->connections = c.connections;
    out->shadow_rays = c.shadow_rays;
    out->cone_tri_overflow = c.cone_tri_overflow;
    out->edge_overflow = c.edge_overflow;
    out->fsd_edge_overflow = c.fsd_edge_overflow;
    out->fsd_pool_overflow = c.fsd_pool_overflow;
    out->fsd_interactions = c.fsd_interactions;
    out->null_interactions = c.null_interactions;
    out->surface_interactions = c.surface_interactions;
    out->light_splats = c.light_splats;
    out->walk_iteration_cap_hits = s->cap_hits;
    {
        unsigned long long dropped = 0;   // (per scene since round 4: the slot behind the profile counters)
        HIP_CHECK(hipMemcpy(&dropped, s->slices[0].counters + kDroppedSlot, sizeof(dropped), hipMemcpyDeviceToHost));
        out->traversal_stack_dropped = dropped;
    }
#ifdef WTGPU_STEP_PROF
    {
        unsigned long long p[8];
        HIP_CHECK(hipMemcpy(p, s->slices[0].counters + kNumCounters, sizeof(p), hipMemcpyDeviceToHost));
        fprintf(stderr, "[wtgpu step prof] pass-B walks %llu (with aperture %llu); total Mticks: scan %.1f pre %.1f edges %.1f integrals+aperture %.1f sample+append %.1f continue %.1f\n", p[7], p[6],
                double(p[0]) * 1e-6, double(p[1]) * 1e-6, double(p[2]) * 1e-6, double(p[3]) * 1e-6, double(p[4]) * 1e-6, double(p[5]) * 1e-6);
    }
#endif
#ifdef WTGPU_COOP_PROF
    if (getenv("WTGPU_PROFILE")) {
        unsigned long long p[12];
        HIP_CHECK(hipMemcpy(p, s->slices[0].counters + kNumCounters, sizeof(p), hipMemcpyDeviceToHost));
        const double n = p[4] ? double(p[4]) : 1.;
        fprintf(stderr, "[coop prof] items %llu; per item ticks: A.pop %.0f A.node+test %.0f A.push %.0f B1.filter %.0f flush+phaseB %.0f; per item: phase-B entries %.1f, candidates %.0f, filter batches %.1f, exact batches %.1f\n", p[4], p[0] / n, p[1] / n,
                p[2] / n, p[7] / n, p[6] / n, p[10] / n, p[11] / n, p[8] / n, p[9] / n);
    }
#endif
    if (s->knobs.profile == 1) {
        unsigned long long p[8];
        HIP_CHECK(hipMemcpy(p, s->slices[0].counters + kNumCounters, sizeof(p), hipMemcpyDeviceToHost));
        fprintf(stderr, "[wtgpu profile] flux tasks: %llu, candidates %llu (max %llu per task), exact-tested %llu; k_edges: %llu walks, %llu edges, %llu apertures built\n", p[0], p[1], p[4], p[2], p[5], p[6], p[3]);
    }
    if (s->knobs.profile == 3) {
        unsigned long long p[kProfSlots];
        HIP_CHECK(hipMemcpy(p, s->slices[0].counters + kNumCounters, sizeof(p), hipMemcpyDeviceToHost));
        fprintf(stderr, "[wtgpu profile] pass C by aperture size (slice 0): bin=log2(segments) items tries/item kticks/item total-Mticks\n");
        for (int b = 0; b < 16; ++b) {
            const unsigned long long n = p[kPassCProfWalks + b];
            if (n) fprintf(stderr, "[wtgpu profile]   C %2d %8llu %10.1f %10.1f %10.1f   fetch+load %.1f commit %.1f kticks/item\n", b, n, double(p[kPassCProfTries + b]) / n, double(p[kPassCProfTicks + b]) / n * 1e-3, double(p[kPassCProfTicks + b]) * 1e-6, double(p[kPassCProfLoadTicks + b]) / n * 1e-3, double(p[kPassCProfCommitTicks + b]) / n * 1e-3);
        }
        if (s->knobs.pass_c_tiers) {   // the tiered form: the lines above hold prep's sum (fetch+load) and prep's tries (kticks/item), tries/item over all tiers
            fprintf(stderr, "[wtgpu profile] pass C in tiers (slice 0): walks settled by prep %llu, wide %llu, hard %llu; wide + hard tries by aperture size: bin items kticks/item total-Mticks\n",
                    p[kPassCTierSlot], p[kPassCTierSlot + 1], p[kPassCTierSlot + 2]);
            for (int b = 0; b < 16; ++b)
                if (p[kPassCProfWideWalks + b]) fprintf(stderr, "[wtgpu profile]   W %2d %8llu %10.1f %10.1f\n", b, p[kPassCProfWideWalks + b], double(p[kPassCProfWideTicks + b]) / p[kPassCProfWideWalks + b] * 1e-3, double(p[kPassCProfWideTicks + b]) * 1e-6);
        }
        fprintf(stderr, "[wtgpu profile] pass B by gathered scene edges: bin items kticks/item total-Mticks\n");
        for (int b = 0; b < 16; ++b)
            if (p[56 + b]) fprintf(stderr, "[wtgpu profile]   B %2d %8llu %10.1f %10.1f\n", b, p[56 + b], double(p[72 + b]) / p[56 + b] * 1e-3, double(p[72 + b]) * 1e-6);
    }
#ifdef WTGPU_REFILL_PROF
    {
        unsigned long long p[16];
        HIP_CHECK(hipMemcpy(p, s->slices[0].counters + kNumCounters, sizeof(p), hipMemcpyDeviceToHost));
        const char* nm[6] = {"serve", "fetch", "store", "nodes", "leaf", "(ray in fetch)"};
        for (int i = 0; i < 6; ++i) fprintf(stderr, "[refill prof] %-16s %10.1f Mticks  lanes %.1f\n", nm[i], p[i] * 1e-6, p[i] ? double(p[8 + i]) / p[i] : 0.);
    }
#endif
#ifdef WTGPU_SM_PROF
    {
        unsigned long long p[64];
        HIP_CHECK(hipMemcpy(p, s->slices[0].counters + kNumCounters, sizeof(p), hipMemcpyDeviceToHost));
        const char* nm[7] = {"serve", "fetch", "aw_next", "store", "NODE", "TRI", "EXACT"};
        for (int i = 0; i < 7; ++i)
            fprintf(stderr, "[sm prof] %-8s %10.1f Mticks  %10.2f Msteps  %7.0f ticks/step  lanes %.1f\n", nm[i], p[32 + i] * 1e-6, p[48 + i] * 1e-6, p[48 + i] ? double(p[32 + i]) / p[48 + i] : 0.,
                    p[32 + i] ? double(p[40 + i]) / p[32 + i] : 0.);
    }
#endif
    if (s->knobs.profile == 2) {
        unsigned long long p[8];
        HIP_CHECK(hipMemcpy(p, s->slices[0].counters + kNumCounters, sizeof(p), hipMemcpyDeviceToHost));
        fprintf(stderr, "[wtgpu profile] heavy items %llu: clock ticks ray %llu probe %llu cone %llu total %llu (per item: ray %.0f probe %.0f cone %.0f total %.0f; cone+probe phase A %.0f phase B %.0f; phase-A steps %.1f entries %.1f)\n", p[4], p[0],
                p[1], p[2], p[3], p[4] ? double(p[0]) / p[4] : 0., p[4] ? double(p[1]) / p[4] : 0., p[4] ? double(p[2]) / p[4] : 0., p[4] ? double(p[3]) / p[4] : 0., p[4] ? double(p[5]) / p[4] : 0., p[4] ? double(p[6]) / p[4] : 0., p[4] ? double(p[7] & 0xffffffffull) / p[4] : 0., p[4] ? double(p[7] >> 32) / p[4] : 0.);
    }
    return WTGPU_OK;
}
int wtgpu_reset_counters(wtgpu_scene* s) {
    if (!s || !s->uploaded) return fail(WTGPU_ERR_INVALID, "scene not uploaded");
    {
        const int rc = drain_all(s);
        if (rc) return rc;
    }
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemset(s->slices[0].counters, 0, (kNumCounters + kProfSlots + 1) * sizeof(unsigned long long)));
    s->samples_rendered = 0;
    s->cap_hits = 0;
    for (double& v : s->acc) v = 0;
    s->rounds_launched_total = 0;
    return WTGPU_OK;
}

int wtgpu_test_profile_counters(wtgpu_scene* s, unsigned long long* out, uint32_t n) {
    if (!s || !out || !s->uploaded || n > kProfSlots) return fail(WTGPU_ERR_INVALID, "wtgpu_test_profile_counters: uploaded scene, n <= kProfSlots");
    {
        const int rc = drain_all(s);
        if (rc) return rc;
    }
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(out, s->slices[0].counters + kNumCounters, n * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return WTGPU_OK;
}

}   // extern "C"
