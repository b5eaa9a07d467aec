/* Test hooks of the bundled scenes — NOT part of the public C-ABI (include/wtgpu.h); exported for tests/ only. */
#pragma once
#include "../../include/wtgpu.h"
#ifdef __cplusplus
extern "C" {
#endif
typedef struct wtgpu_test_hooks {
    uint32_t only_s, only_t; /* 0 = all strategies; v>0 evaluates only s (t) = v-1 with unit MIS weight */
    uint32_t crop_of;        /* perspective sensors: 0 = off; v>0: the res x res film is the central crop of a v x v film (same pixel pitch,
                              * hence the same beam footprints, as the full-size render) */
} wtgpu_test_hooks;
int wtgpu_scene_create_named_hooks(const char* name, const wtgpu_scene_params* params, const wtgpu_test_hooks* hooks, wtgpu_scene** out);
/* field-by-field (byte-for-byte) comparison of two flattened scenes: 0 identical, 1 different (`what`: the first difference) */
int wtgpu_scene_compare(const wtgpu_scene* a, const wtgpu_scene* b, char* what, size_t n_what);
/* the same restricted to one part: "sensor", "opts" or "emitters" (records that do not depend on the geometry) */
int wtgpu_scene_compare_part(const wtgpu_scene* a, const wtgpu_scene* b, const char* part, char* what, size_t n_what);
/* WTGPU_TRACE_AB=n (environment, read at upload): the first n rounds of every batch replay their trace queue through k_trace_refill and k_trace_sm (the
 * pipeline continues from the second one's output).  Accumulated since upload: event-timed milliseconds of each kernel, words of their outputs
 * (traversal records, triangle lists, heavy-queue checksums) that differ, walks and rounds replayed. */
int wtgpu_trace_ab_stats(wtgpu_scene* s, double* ms_refill, double* ms_sm, uint64_t* differing_words, uint64_t* walks, uint64_t* rounds);
/* The WTGPU_PROFILE scratch counters (accumulated since upload; n <= 128).  WTGPU_PROFILE=1: [3] apertures with segments built by k_edges'
 * wavefront (coop_build_aperture), [5] walks k_edges gathered, [6] edge ids they gathered. */
int wtgpu_test_profile_counters(wtgpu_scene* s, unsigned long long* out, uint32_t n);
/* Per-query entry points of the diffraction kernels (kernels_test.hip; layouts: wt/diffraction_probe.h).  Device pointers, asynchronous on `stream`;
 * the edge ids must be < the scene's edge count (not checked).  The CPU checker has the same entry points (oracle/oracle.cpp: oracle_fsd_apertures,
 * oracle_utd_sums).
 * wtgpu_test_fsd_apertures: one Fraunhofer aperture per query from an explicit edge-id list (n x id_cap, the first n_ids[q] used), built by
 *   coop_build_aperture (mode 0) or by the sequential form after the sizing of bdpt_walk_step (mode 1), each query in a segment pool of its own
 *   of pool_cap records (a smaller pool forces fsd_pool_alloc_edges to fail).  hdr: n x 8 words; segs: n x pool_cap segment records (7 floats).
 * wtgpu_test_utd_sums: one UTD aperture per query (utd_build_aperture into n x utd_cap records `recs`) and its coherent sum by coop_do_fsd<1>,
 *   <8>, <64> and path_do_fsd.  hdr: n x 8 words; edges: n x utd_cap x 8 words. */
int wtgpu_test_fsd_apertures(wtgpu_scene* s, void* stream, const float* d_cones, const float* d_sk, const uint32_t* d_ids, const uint32_t* d_n_ids,
                             uint32_t n, uint32_t id_cap, uint32_t pool_cap, uint32_t mode, uint32_t* d_hdr, float* d_segs);
int wtgpu_test_utd_sums(wtgpu_scene* s, void* stream, const float* d_queries, const uint32_t* d_ids, const uint32_t* d_n_ids, uint32_t n, uint32_t id_cap,
                        uint32_t utd_cap, uint32_t* d_recs, uint32_t* d_hdr, uint32_t* d_edges);
/* Per-query entry point of the material layer (kernels_test.hip: k_test_bsdf; layouts: wt/bsdf_probe.h): n queries of 18 words, n x 48 output
 * words, device pointers, asynchronous on `stream`.  form -1: the generic material_f / material_pdf / material_sample; 0, 1, 2 (diffuse,
 * dielectric, surface_spm): the class forms of the material-sorted interaction pass.  Material ids must be < the scene's material count (not
 * checked).  The CPU checker's counterpart (generic form only): oracle/oracle.cpp: oracle_bsdf_queries. */
int wtgpu_test_bsdf_queries(wtgpu_scene* s, void* stream, const uint32_t* d_queries, uint32_t n, int form, uint32_t* d_out);
/* Per-query entry point of the emitter / sensor / wavenumber layer (kernels_test.hip: k_test_sources; layouts: wt/sources_probe.h): n queries
 * of 24 words, n x 80 output words, device pointers.  The queries are read back and checked first (this call waits for `stream`): an op
 * outside the table, an emitter index >= the scene's count or a tuid >= its triangle count returns WTGPU_ERR_INVALID and launches nothing.
 * The CPU checker's counterpart: oracle/oracle.cpp: oracle_source_queries. */
int wtgpu_test_source_queries(wtgpu_scene* s, void* stream, const uint32_t* d_queries, uint32_t n, uint32_t* d_out);
/* Per-query entry point of the region power integral (kernels_test.hip: k_test_flux; layouts: wt/flux_probe.h): n queries of 20 words, n x 36
 * output words, device pointers.  The queries are read back and checked first (this call waits for `stream`): an op outside the table or a
 * tuid >= the scene's triangle count returns WTGPU_ERR_INVALID and launches nothing.  The CPU checker's counterpart: oracle/oracle.cpp:
 * oracle_flux_queries. */
int wtgpu_test_flux_queries(wtgpu_scene* s, void* stream, const uint32_t* d_queries, uint32_t n, uint32_t* d_out);
/* The class form of the connections (k_connect_class, WTGPU_CONNECT_CLASS=1).  N = n_keys = key_dim x key_dim length classes, key = tk * key_dim + sk
 * (the capped subpath lengths of a class).
 * wtgpu_test_connect_class_order: N and key_dim; with cap >= N also the keys in the order the kernel's wavefronts take the classes, descending
 *   tk x sk, as the host computes it (wtgpu_kernels.h: class_key_rank).
 * wtgpu_test_connect_class_items: what the LAST batch connected on state slice `slice` left behind.  table: 3 N + 1 words, all by rank — [0, N]
 *   start of the class in the flattened item space (classes padded to multiples of 64), [N + 1 + r] its samples, [2 N + 1 + r] its key (the
 *   device's order); items: the samples (indices into the batch) of all classes in that order, unpadded; n_items: how many.  Waits for
 *   everything in flight. */
int wtgpu_test_connect_class_order(uint32_t* keys, uint32_t cap, uint32_t* n_keys, uint32_t* key_dim);
int wtgpu_test_connect_class_items(wtgpu_scene* s, uint32_t slice, uint32_t* table, uint32_t* items, uint32_t items_cap, uint32_t* n_items);
/* out[i] = dn_exp2_neg(t[i]) of wt/film_denoise.h (2^-t for t >= 0, the film denoiser's weight function), on the host: for the test of its bound. */
int wtgpu_test_dn_exp2_neg(const float* t, uint64_t n, float* out);
/* The zonal statistics' exact sum by itself (wt/film_zonal.h), on the host: fz_add of the finite ones of x[n] onto words[9] (left as they then are),
 * *out = fz_round(words).  n = 0 rounds hand-made words. */
int wtgpu_test_fz_sum(uint64_t* words, const float* x, uint64_t n, double* out);
/* The form of k_film_zonal that the scene's last wtgpu_film_zonal_device call launched: *lds = 1 the LDS form, 0 the global form, 0xFFFFFFFF no call
 * yet.  Both forms give the same bits, so only this tells a test which one ran. */
int wtgpu_test_film_zonal_form(const wtgpu_scene* s, uint32_t* lds);
/* The segments' union-find walk by itself (csrc/kernels_segments.hip: seg_find), on the host: up parent[n] from x with at most `bound` loads.  *root: where
 * the walk ended; *overflow: 1 where the bound was hit or a parent lies above its child (the kernels then refuse), else 0. */
int wtgpu_test_film_segments_find(const uint32_t* parent, uint32_t n, uint32_t x, uint32_t bound, uint32_t* root, uint32_t* overflow);
/* The scene's last wtgpu_film_segments_device call: *form = 1 the tiled form of its first two phases, 0 the global form (both give the same
 * bits, so only this tells a test which one ran), *overflow = its overflow word (0: no loop hit its step bound); both 0xFFFFFFFF before the first call. */
int wtgpu_test_film_segments_form(const wtgpu_scene* s, uint32_t* form, uint32_t* overflow);
/* The form of k_dist_rows that the scene's last wtgpu_film_distance_device call launched: *groups = 1 with the group level, 0 the outward search
 * alone, 0xFFFFFFFF no call yet.  Both forms give the same bits, so only this tells a test which one ran. */
int wtgpu_test_film_distance_form(const wtgpu_scene* s, uint32_t* groups);
#ifdef __cplusplus
}
#endif
