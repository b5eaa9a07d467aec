/* wtgpu.h — C-ABI of the MI355X-native wave_tracer hot path (libwtgpu.so).
 *
 * Drop-in seam (seam S1): this library replaces the block fan-out of the reference's render loop,
 *     scene_renderer_t::render()                    src/scene/render.cpp:381-579
 *       -> block_renderer_t -> integrator_t::integrate(ctx, block, pixel, spp)     src/scene/render.cpp:99-113,
 *                                                                                  include/wt/integrator/integrator.hpp:44-57
 * i.e. everything between "scene + ADS are built" and "film storage is developed".  The host keeps scene parsing
 * and image I/O; it hands over a flattened scene description and gets back the
 * three linear film accumulators  value = sum(w*v), weight = sum(w), light = sum(light-image splats), exactly the
 * quantities film_storage_t holds (include/wt/sensor/film/film_storage.hpp:196-252), from which
 *     pixel = value/weight + light/spe        (film_storage.hpp:256-287, src/scene/render.cpp:245-291).
 * Development and tonemapping run on either side: on the device, where the films are (wtgpu_develop_device, wtgpu_tonemap_device: the
 * host downloads a finished picture instead of three f64 accumulators), or on the host (wtgpu_develop, wtgpu_tonemap_host).
 *
 * The integrator is part of the flattened scene: plt_bdpt (src/integrator/plt_bdpt.cpp:43-148) or plt_path in either transport
 * direction (src/integrator/plt_path.cpp:39-50); polarimetric sensors get four Stokes planes per channel.
 *
 * Plain C types only; opaque handles; int status returns (0 = ok); no exceptions cross the boundary.
 * One wtgpu_scene may be uploaded to one device per process (one process per GPU).
 */
#ifndef WTGPU_H
#define WTGPU_H

#include <stddef.h>
#include <stdint.h>

#include "wtgpu_scene.h" /* wtgpu_scene_desc: the flattened scene (plain C structs) */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct wtgpu_scene wtgpu_scene;
typedef struct wtgpu_comm wtgpu_comm;

enum { WTGPU_OK = 0, WTGPU_ERR_INVALID = 1, WTGPU_ERR_NO_DEVICE = 2, WTGPU_ERR_HIP = 3, WTGPU_ERR_OOM = 4, WTGPU_ERR_OVERFLOW = 5, WTGPU_CANCELLED = 6,
       WTGPU_ERR_COMM = 7 };

/* Parameters of a bundled scene; negative/zero fields select the scene file's defaults.
 * Mirrors the CLI `-D res=..` defines + integrator attributes the reference reads
 * (src/main.cpp:805-928; src/integrator/plt_bdpt.cpp:169-174). */
typedef struct wtgpu_scene_params {
    uint32_t res;
    int32_t max_depth;
    int32_t fsd;
    int32_t mis;
    int32_t rr;
    int32_t force_ray_tracing; /* --ray-tracing (include/wt/wt_context.hpp:43) */
    int32_t mesh_detail;       /* 0: low-poly stand-ins, 1: full tessellation */
    uint32_t lut_n_theta, lut_m; /* resolution of the regenerated Fraunhofer iCDF LUT (0: default) */
    int32_t polarimetric;      /* >0: polarimetric sensor — the film stores the 4 Stokes components per channel
                                * (sensor `polarimetric` attribute, include/wt/sensor/sensor/perspective.hpp:185-330) */
} wtgpu_scene_params;

typedef struct wtgpu_scene_info {
    uint32_t width, height, channels;
    uint32_t n_tris, n_edges, n_nodes, n_leaves, n_shapes, n_emitters, n_materials;
    int32_t max_depth;
    uint32_t sensor_type; /* 0 perspective, 1 virtual_plane */
    double fsd_lut_power[2]; /* integrals of the regenerated LUT densities (compare: PA1, PA2 of fsd.hpp:59-61) */
    uint64_t bytes_per_sample_state; /* device bytes of per-sample path/vertex state */
    uint32_t stokes;      /* film components per channel: 1 (intensity) or 4 (polarimetric sensor: I, Q, U, V) */
    uint32_t integrator;  /* 0 plt_bdpt, 1 plt_path forward, 2 plt_path backward */
} wtgpu_scene_info;

/* Device counters (the reference's stat collectors: include/wt/integrator/stats.hpp:27-83, include/wt/ads/ads_stats.hpp),
 * the inputs of the algorithmic-bytes formula of SURVEY.md §8(d). */
typedef struct wtgpu_counters {
    uint64_t samples;
    uint64_t segments, ray_queries, cone_queries, vertices, connections, shadow_rays;
    uint64_t cone_tri_overflow, edge_overflow, fsd_edge_overflow, fsd_pool_overflow, fsd_interactions, null_interactions;
    uint64_t surface_interactions, light_splats;
    uint64_t walk_iteration_cap_hits;
    uint64_t traversal_stack_dropped;   /* children a full wave-cooperative traversal stack (512 entries) could not hold: must be 0 */
} wtgpu_counters;

/* Host-side scene baking (no GPU needed): builds one of the bundled scenes
 * ("double_slits" = scenes/diffraction_simple/double_slits.xml, "cornell_box" = scenes/cornell-box/box.xml stand-in,
 * "furnace" = test scene).  Replaces scene_bootstrap_t<xml_loader_t,bvh8w_constructor_t> (src/main.cpp:634-648). */
int wtgpu_scene_create_named(const char* name, const wtgpu_scene_params* params, wtgpu_scene** out);

/* Wraps an already flattened scene (include/wtgpu_scene.h; host pointers that must outlive the handle).  This is the entry point a
 * port of the reference's own loader calls. */
int wtgpu_scene_create_from_desc(const wtgpu_scene_desc* scene_desc_host, wtgpu_scene** out);

/* Reader of the reference's XML scene format (src/scene/loader/): 14 of the 15 scene files the reference ships load
 * as they are (tests/test_xml_scene.py::test_which_of_the_shipped_scene_files_load) — <default> defines and "$name" substitution, expressions
 * with units, <include>, enabled=..., shared elements and <ref>s (bsdfs, textures, spectra, transforms); plt_bdpt / plt_path integrators; <sampler> of type
 * independent / uniform / sobolld (all served by the library's counter-based streams); perspective and virtual-plane sensors with array films (RGB / monochromatic response, polarimetric flag); spot, directional, point and area
 * emitters; diffuse, dielectric, surface_spm (dirac / fractal / gaussian profile, constant or textured roughness), twosided, scale (constant,
 * spectrum, texture), mask, normalmap and composite BSDFs; constant, checkerboard, bitmap (PNG, PFM, OpenEXR: scan-line files, NONE / RLE / ZIPS / ZIP, read through half precision), scale, transform, function and mix
 * textures; spectra by constant, rgb, blackbody, discrete, piecewise linear, ITU material, or material / emitter name (baked tables or the
 * database files of data/ior, data/emission); rectangle, cube, sphere, cylinder, prism, lens shapes and PLY / OBJ meshes with general to_world
 * transforms (a Git-LFS pointer in place of an asset: a stand-in, or skipped with -Dwtgpu_missing_assets=skip).  OBJ meshes take a material group with `mtl` (the reference's filter).  Not read: textured area-emitter
 * radiance, JPEG images, tiled / deep / PIZ-compressed EXR files; `sobolld`'s low-discrepancy point set itself is not reproduced (a scene that asks for it
 * renders with the same counter-based streams as every other sampler type).  `defines`: n_defines strings "name=value", the -D
 * defines of the reference's command line (src/main.cpp:805-928).  params (may be NULL): res (becomes the define "res" unless given), max_depth /
 * fsd / mis / rr / force_ray_tracing overrides, lut_* resolution, polarimetric.  Anything outside that vocabulary fails with a message. */
int wtgpu_scene_create_from_xml(const char* path, const char* const* defines, uint32_t n_defines, const wtgpu_scene_params* params, wtgpu_scene** out);

int wtgpu_scene_get_info(const wtgpu_scene* scene, wtgpu_scene_info* info);

/* The flattened description of a handle (for CPU-side checkers and tools). */
const wtgpu_scene_desc* wtgpu_scene_host_desc(const wtgpu_scene* scene);

/* Copies the flattened scene to `device` and allocates the per-sample path state: three slices (one internal stream each), each for a
 * batch of up to `max_batch_samples` samples (0: one sample per sensor element, at most 4 M; at most 16 M), shrunk to fit the memory budget —
 * WTGPU_STATE_GB (default 224) and never more than 85 % of the device's free memory.  A render call is cut into batches of that size; larger
 * batches are faster (every batch pays its own thin tail: DESIGN.md, section 0; bench.py renders ~4 M samples per batch).  Refuses runtime
 * settings that are known to serialise the internal streams (an explicit HSA_KERNARG_POOL_SIZE < 4 MiB;
 * WTGPU_ALLOW_SLOW_RUNTIME=1 overrides).  Fails with WTGPU_ERR_NO_DEVICE when
 * no HIP device is present: there is no CPU fallback. */
int wtgpu_scene_upload(wtgpu_scene* scene, int device, uint64_t max_batch_samples);

/* Renders sample indices [sample_begin, sample_end) of every sensor element (the `spp` loop of
 * integrator_t::integrate for all pixels) and accumulates into the caller-owned DEVICE film buffers
 *     d_value  [height][width][channels][stokes] f64,  d_weight [height][width] f64,  d_light [height][width][channels][stokes] f64.
 * `stream` is a hipStream_t (NULL = default stream).  The work runs on internal streams that start after everything already on
 * `stream`, and `stream` continues after them: synchronise `stream` before reading the films.  (The call returns once the LAST part of
 * the work is enqueued; since round 4 a batch of samples is enqueued in two parts with a look at its round queue in between, so the
 * calling thread waits for most of the work to have run — see wtgpu_join.)  RNG: Philox-4x32-10 keyed by `seed`, counter = (pixel, sample, stream). */
int wtgpu_render(wtgpu_scene* scene, void* stream, double* d_value, double* d_weight, double* d_light, uint64_t sample_begin, uint64_t sample_end,
                 uint64_t seed);

/* The two halves of wtgpu_render.  wtgpu_render_async enqueues the work behind everything already on `stream` but does not make
 * `stream` wait for it, so consecutive calls (more samples into the same accumulators) pipeline on the GPU; wtgpu_join makes
 * `stream` continue after everything enqueued so far.  Nothing may read or overwrite the films between an async render and its
 * join.  A batch is enqueued in two parts: generation and the rounds its walks are expected to need, and — after the host has seen
 * its round queue empty (looking again every 8 rounds otherwise) — the connections.  wtgpu_render_async enqueues the first part of
 * its batches (and the second part of whichever earlier batch still holds the state slice it reuses: it may wait for that one);
 * wtgpu_join WAITS on the host for the first parts of the batches still pending (serving whichever is ready first), enqueues their second parts, and makes `stream`
 * continue after them. */
int wtgpu_render_async(wtgpu_scene* scene, void* stream, double* d_value, double* d_weight, double* d_light, uint64_t sample_begin,
                       uint64_t sample_end, uint64_t seed);
int wtgpu_join(wtgpu_scene* scene, void* stream);

/* The render seam's control surface (scene_renderer_t: progress callback + terminate interrupt polled between jobs,
 * include/wt/scene/scene_renderer.hpp:42-62, src/scene/render.cpp:306-368).  Renders [sample_begin, sample_end) in chunks of
 * `chunk_spp` samples per element (0: 1), BLOCKING: after every chunk `stream` is synchronised, progress(samples_done, samples_total,
 * user) is called (may be NULL) and the interrupts are processed (cancel below; pause / resume / capture intermediate further down); a non-zero return of the callback or a wtgpu_cancel() from any thread
 * ends the render after the current chunk with WTGPU_CANCELLED — the films then hold exactly the completed chunks
 * (*spe_done samples per element; may be NULL), which is what the reference's `capture intermediate` develops. */
typedef int (*wtgpu_progress_cb)(uint64_t samples_done, uint64_t samples_total, void* user);
int wtgpu_render_progressive(wtgpu_scene* scene, void* stream, double* d_value, double* d_weight, double* d_light, uint64_t sample_begin,
                             uint64_t sample_end, uint64_t seed, uint32_t chunk_spp, wtgpu_progress_cb progress, void* user, uint64_t* spe_done);
int wtgpu_cancel(wtgpu_scene* scene);   /* thread-safe; cleared when the next wtgpu_render_progressive starts; also lifts a pause (a full reset) */
/* The renderer's other three interrupts (include/wt/scene/interrupts.hpp; scene_renderer_t::process_interrupts, src/scene/render.cpp:329-368),
 * all thread-safe, all taking effect at the next chunk boundary of a running wtgpu_render_progressive:
 *   wtgpu_pause / wtgpu_resume      the render thread stops launching (it polls every millisecond) until resumed or cancelled; the films hold
 *                                   exactly the completed chunks while it waits.  A pause is STICKY: issued while no render runs it holds the
 *                                   next wtgpu_render_progressive after its first chunk; wtgpu_resume or wtgpu_cancel lift it.
 *   wtgpu_capture_intermediate      `capture intermediate`: the render thread calls capture(samples_per_element_done, user) ONCE at the next chunk
 *                                   boundary (also while paused), with `stream` synchronised — the films then hold exactly the completed chunks and
 *                                   the callback may download / develop them (wtgpu_develop) — and carries on in the state it was in, like the
 *                                   reference, which pauses, develops and restores the paused state.  One request may be pending at a time (a
 *                                   second one replaces it); a request made while no render runs is served by the next render's first boundary. */
int wtgpu_pause(wtgpu_scene* scene);
int wtgpu_resume(wtgpu_scene* scene);
typedef void (*wtgpu_capture_cb)(uint64_t samples_per_element_done, void* user);
int wtgpu_capture_intermediate(wtgpu_scene* scene, wtgpu_capture_cb capture, void* user);

/* Multi-GPU, one process per GPU: samples are sharded by sample index, every rank renders into its own films, and
 * the three linear accumulators are summed onto `root` with one RCCL reduce each over xGMI — film_storage_t's merge of per-worker
 * images (include/wt/sensor/film/film_storage.hpp:276-287,411-413) across devices.  Rank 0 creates the id (WTGPU_COMM_ID_BYTES) and
 * hands it to the other ranks by whatever means the host has (MPI, a file, torch.distributed); every rank then calls wtgpu_comm_create
 * with the device its scene is uploaded to.  n_value = width*height*channels*stokes doubles, n_weight = width*height. */
#define WTGPU_COMM_ID_BYTES 128
int wtgpu_comm_unique_id(void* id_out);
int wtgpu_comm_create(int world_size, int rank, int device, const void* id, wtgpu_comm** out);
int wtgpu_film_reduce(wtgpu_comm* comm, void* stream, double* d_value, double* d_weight, double* d_light, uint64_t n_value, uint64_t n_weight,
                      int root);
void wtgpu_comm_destroy(wtgpu_comm* comm);

/* Per-query ADS entry points (ads_t::intersect(ray) / integrator::traverse(cone), include/wt/ads/ads.hpp:71-113,
 * include/wt/integrator/traversal.hpp:94-172) on device-resident arrays; used by the traversal parity tests.
 * rays:  n x {ox,oy,oz, dx,dy,dz, tmin,tmax}            cones: n x {ox,oy,oz, dx,dy,dz, tan_alpha, x0, ecc, lambda_m} */
int wtgpu_trace_rays(wtgpu_scene* scene, void* stream, const float* d_rays, uint32_t n, float* d_dist, uint32_t* d_tuid, float* d_bary,
                     uint32_t* d_front);
int wtgpu_traverse_cones(wtgpu_scene* scene, void* stream, const float* d_cones, uint32_t n, uint32_t cap, float* d_dist, uint32_t* d_flags,
                         uint32_t* d_ntris, uint32_t* d_tris);

/* Region summaries of n cone queries (same cone layout): the traversal policy's hit (dist, flags: 1 empty, 2 ballistic, 4 front face),
 * the triangle under the beam axis (find_closest_triangle, plt_bdpt_detail.hpp:362-389; 0xFFFFFFFF: none) and — for diffusive hits — the
 * interaction region [dist, dist + 2 x major axis] walked IN FULL, whatever its size (the reference's unbounded record,
 * include/wt/ads/traversal_common.hpp:124-148): triangle count, number + sorted ids (first edge_cap) of its classified edges, and the
 * fraction of a Gaussian beam (sigma = cross-section axes / 3) its triangles facing like the closest one intercept
 * (plt_bdpt_detail.hpp:391-416).  Used by the parity tests of regions beyond the device's 64-triangle fast path. */
int wtgpu_query_regions(wtgpu_scene* scene, void* stream, const float* d_cones, uint32_t n, uint32_t edge_cap, float* d_dist, uint32_t* d_flags,
                        uint32_t* d_primary, uint32_t* d_ntris, uint32_t* d_nedges, uint32_t* d_edges, float* d_flux);

/* By-geometry sensor masks (include/wt/sensor/mask/mask.hpp, src/sensor/mask.cpp:28-108), what the reference's CLI writes as the alpha channel
 * of `<sensor>_tonemapped_masked` (src/main.cpp:315-326).  A scene file's perspective sensor may hold <sensor_mask type="by-geometry"> with a
 * mask_id_regex (src/sensor/perspective.cpp:98); it is kept beside the flattened scene, which it does not change.
 *
 * The element id of shape `shape` (the scene's shape order = tri_meta_t::shape_idx): the element's `id`, "__unnamed_$<n>" for unnamed enabled
 * top-level elements (src/scene/loader/loader.cpp:131-133); "" for bundled scenes and wtgpu_scene_create_from_desc.  Valid while the handle lives. */
int wtgpu_scene_shape_id(const wtgpu_scene* scene, uint32_t shape, const char** id);
/* The scene file's mask (mask_t::load, src/sensor/mask.cpp:76-108).  `samples` is always 32: the loader reads a `samples` attribute but never
 * passes it to the mask (mask.hpp:44-52).  shape_flags[i] = 1 if std::regex_match(id of shape i, regex) (ECMAScript, the whole id). */
typedef struct wtgpu_sensor_mask_spec {
    int32_t present;              /* 0: no <sensor_mask> (the other fields are empty) */
    uint32_t samples;
    const char* regex;
    const uint8_t* shape_flags;   /* n_shapes bytes, valid while the handle lives */
    uint32_t n_shapes;
} wtgpu_sensor_mask_spec;
int wtgpu_scene_sensor_mask_spec(const wtgpu_scene* scene, wtgpu_sensor_mask_spec* out);
/* mask_t::create_mask (src/sensor/mask.cpp:28-66) on the device, into the caller's DEVICE buffer d_out [height][width] f32, on `stream`: per pixel
 * `samples` rays of the sensor's own pixel sampling (perspective.hpp:229-262, k = 0), each traced to its closest hit (ads_t::intersect); a hit on a
 * shape whose flag is 0 adds 1 / float(samples), in sequence (a miss adds nothing).  shape_flags: n_shapes bytes on the host, 1 = "matches the
 * regex", copied before the call returns; NULL = the scene file's flags.  RNG: sample s of pixel p draws from the stream (seed, p * samples + s).
 * Needs an uploaded scene with a perspective sensor (WTGPU_ERR_INVALID otherwise); touches neither films nor counters. */
int wtgpu_sensor_mask(wtgpu_scene* scene, void* stream, const uint8_t* shape_flags, uint32_t samples, uint64_t seed, float* d_out);
/* The same computation on `n_threads` host threads (0: all cores) from the host description, into HOST memory out [height][width]: the
 * reference's own CPU job, bit for bit what wtgpu_sensor_mask computes.  No device needed. */
int wtgpu_sensor_mask_host(const wtgpu_scene* scene, const uint8_t* shape_flags, uint32_t samples, uint64_t seed, uint32_t n_threads, float* out);

/* First-hit maps of a perspective sensor ("AOVs", "G-buffer"): what every pixel's primary rays see first — how far, where, which way it faces,
 * where on its texture, which shape and triangle.  Noise-free guides for a feature-aware filter and, for a radio scene, the building under a pixel.
 *   rays     samples >= 1: exactly the rays of wtgpu_sensor_mask for the same `samples` and `seed` — sample s of pixel p draws from the stream
 *            (seed, p * samples + s) through the sensor's own pixel sampling (perspective.hpp:229-262, k = 0), range [0, inf).  samples == 0: one
 *            ray per pixel through the pixel's centre, the same statement with the offset (0, 0); no draw, `seed` is not used.  At most 4096.
 *   sample   of a ray that hits: dist (ads_t::intersect), wp = origin + direction x dist, and the surface record the integrators shade with
 *            (intersection_surface_t, src/interaction/intersection.cpp:33-72) at that triangle, barycentric point and wp — the shading frame
 *            includes the `normalmap` wrapper (bsdf/normalmap.hpp:48-62).
 *   maps     [height][width][K] f32, K = the floats of the bits of `maps`, in bit order:
 *              1  COVERAGE        1  float(n_hit) / float(samples) (samples == 0 counts as 1), n_hit = the rays of the pixel that hit
 *              2  DEPTH           1  dist
 *              4  POSITION        3  wp
 *              8  NORMAL_GEO      3  the geometric normal as the triangle has it, NOT flipped towards the camera
 *             16  NORMAL_SHADING  3  the shading normal
 *             32  UV              2  the texture coordinates ((0, 0) on a mesh without them)
 *             64  FACING          1  1 if the ray meets the triangle's front (dot(n, direction) <= 0), else 0
 *            Every map but COVERAGE is the MEAN over the hitting samples: an f32 sum in sample order s = 0, 1, ..., first term first, divided
 *            once by float(n_hit).  Mean normals are not renormalised: a length below 1 marks a pixel that sees an edge.  A pixel that no
 *            sample hits holds 0 in every float map.
 *   ids      [height][width][Ki] u32, of the first sample in order that hits: 1 SHAPE, the shape's index (the order of wtgpu_scene_shape_id);
 *            2 TRIANGLE, the triangle's index within its shape.  0xFFFFFFFF for a pixel without a hit.
 * Errors (WTGPU_ERR_INVALID with a message): a sensor that is not perspective (a virtual-plane sensor has no primary ray in this sense), unknown
 * map or id bits, samples > 4096, a requested group whose pointer is NULL, nothing requested.  A group that is not requested may be NULL. */
typedef struct wtgpu_first_hit_spec {
    uint32_t samples;
    uint32_t maps /* 1 COVERAGE, 2 DEPTH, 4 POSITION, 8 NORMAL_GEO, 16 NORMAL_SHADING, 32 UV, 64 FACING */, ids /* 1 SHAPE, 2 TRIANGLE */, pad;
    uint64_t seed;
} wtgpu_first_hit_spec;
/* On the device, into the caller's DEVICE buffers, asynchronously on `stream`: one kernel — one lane per sample up to 64 samples, one lane per
 * pixel beyond and for the centre ray (WTGPU_FIRST_HIT_PER_SAMPLE=0: always); the result does not depend on the form.  Needs an uploaded scene
 * (WTGPU_ERR_INVALID otherwise); counts nothing and touches neither films nor counters. */
int wtgpu_first_hit(wtgpu_scene* scene, void* stream, const wtgpu_first_hit_spec* spec, float* d_maps, uint32_t* d_ids);
/* The same on `n_threads` host threads (0: all cores) from the host description, into HOST memory: bit for bit what wtgpu_first_hit computes, and
 * the result does not depend on n_threads.  No device needed. */
int wtgpu_first_hit_host(const wtgpu_scene* scene, const wtgpu_first_hit_spec* spec, uint32_t n_threads, float* maps, uint32_t* ids);

/* First-hit material maps of a perspective sensor: what the MATERIAL under a pixel is at chosen wavenumbers — the albedo guide of a feature-aware
 * filter (a checkerboard, a bitmap or a mask pattern on a flat wall is constant in every geometric map) and, for a radio scene, the specular
 * reflectance of the wall under a pixel at the carrier.
 *   rays     exactly those of the first-hit maps above for the same `samples` and `seed` (samples == 0: the ray through the pixel's centre),
 *            with the same hit, wp and surface record.  At most 4096.
 *   sample   of a ray that hits shape S, with direction d: mat = S's material, uv = the surface's, wi = -d in the shading frame.  Per requested
 *            wavenumber k[j], j < n_k <= 4, in 1/mm: the wrappers of mat are followed down to a leaf BSDF m at k[j] (composite bins, masks,
 *            scale and two_sided wrappers, textured roughness); ok = there is one.  wi' = wi mirrored to z >= 0 if m is two-sided, else wi;
 *            a = the accumulated mask opacity, 1 without a mask.
 *   maps     [height][width][K] f32, K = n_k x the number of set bits of `maps`; the maps in bit order, the n_k values of a map adjacent:
 *              1  ALBEDO     m diffuse and wi'.z > 0: clamp01(reflectance spectrum(k) x texture(uv, k)) x m's scale x a, else 0
 *              2  SPECULAR   m dielectric or surface_spm and wi'.z != 0: the unpolarised power reflectance of the SMOOTH interface for wi' x
 *                            m's reflection scale x m's scale x a, else 0.  With eta = the relative IOR at k[j]: where the material transmits
 *                            (Im(eta)^2 / |eta|^2 <= 0.01) 1 - (Ts + Tp) / 2 of the Fresnel equations at Re(eta), the reflection share the
 *                            BSDF's own sampling uses; otherwise (a conductor, a lossy wall) (|rs|^2 + |rp|^2) / 2 at the complex eta,
 *                            which is 0 from behind.
 *              4  OPACITY    a
 *              8  ROUGHNESS  m surface_spm: its perceptual roughness (after a roughness texture), else 0
 *             16  EMISSION   S carries an area emitter and dot(-d, geometric normal) > 0: its spectral radiance at uv and k[j], else 0
 *            Every float but EMISSION is 0 when !ok.  Every value is the MEAN over the hitting samples: an f32 sum in sample order, first term
 *            first, divided once by float(n_hit).  A pixel that no sample hits holds 0.  A value is a point sample at k[j], not an integral
 *            over a channel's response.
 *   ids      [height][width][Ki] u32, of the first sample in order that hits: 1 MATERIAL, the index of S's material; 2 TYPE, the leaf type at
 *            k[0] (0 diffuse, 1 dielectric, 2 surface_spm), 0xFFFFFFFF without a BSDF at k[0].  0xFFFFFFFF for a pixel without a hit.
 * Function textures whose programs use libm (pow, sin, ...) are evaluated, but only the others are bit-identical between device and host.
 * A wavenumber outside the support of a material's tabulated IOR meets the table's 0 there: SPECULAR is then not finite (the renderer never
 * draws such a wavenumber; a caller can).
 * Errors (WTGPU_ERR_INVALID with a message): a sensor that is not perspective, unknown map or id bits, n_k outside 1 .. 4, a k[j] that is not
 * finite and > 0, samples > 4096, a requested group whose pointer is NULL, nothing requested.  A group that is not requested may be NULL. */
typedef struct wtgpu_first_hit_material_spec {
    uint32_t samples;
    uint32_t maps /* 1 ALBEDO, 2 SPECULAR, 4 OPACITY, 8 ROUGHNESS, 16 EMISSION */, ids /* 1 MATERIAL, 2 TYPE */, n_k /* 1 .. 4 */;
    float k[4];
    uint64_t seed;
} wtgpu_first_hit_material_spec;
/* On the device, into the caller's DEVICE buffers, asynchronously on `stream`: one kernel, in the two lane shapes of the first-hit maps
 * (WTGPU_FIRST_HIT_PER_SAMPLE chooses, the result does not depend on it).  Needs an uploaded scene (WTGPU_ERR_INVALID otherwise); counts nothing
 * and touches neither films nor counters. */
int wtgpu_first_hit_material(wtgpu_scene* scene, void* stream, const wtgpu_first_hit_material_spec* spec, float* d_maps, uint32_t* d_ids);
/* The same on `n_threads` host threads (0: all cores) from the host description, into HOST memory: bit for bit what the device call computes,
 * and the result does not depend on n_threads.  No device needed. */
int wtgpu_first_hit_material_host(const wtgpu_scene* scene, const wtgpu_first_hit_material_spec* spec, uint32_t n_threads, float* maps, uint32_t* ids);
/* One wavenumber [1/mm] per spectral channel of the sensor, k[c] for c < channels and 0 beyond — a natural choice of k above: the line of a
 * discrete response; for a tabulated response the response-weighted mean sum(k_i R_i) / sum(R_i) over the table's own knots, in f64, rounded
 * to f32.  A constant or all-zero response singles out no wavenumber: WTGPU_ERR_INVALID with a message. */
int wtgpu_scene_channel_wavenumbers(const wtgpu_scene* scene, float k[4]);

/* Line-of-sight maps: which emitters a sensor element — or a caller's point — can see.  LOS / NLOS is the basic partition of a propagation study,
 * and from a perspective sensor's first-hit positions the same query is a noise-free shadow plane per lamp.
 *   points   d_points == NULL: the elements of a VIRTUAL-PLANE sensor.  Sample s of element (px, py) is the point the sensor's own sampling forms
 *            (virtual_plane_sensor.hpp, the point of sensor_t::sample) at the offset o = r2 - (.5, .5) drawn from the stream
 *            (seed, (py W + px) samples + s) of the line-of-sight maps: origin + ((px + o.x + .5) element_extent.x) t + ((py + o.y + .5)
 *            element_extent.y) b; samples == 0: the element's centre, o = (0, 0), no draw.  At most 4096.  The normal is the sensor's.
 *            d_points [height][width][3] f32 (for example the POSITION map of wtgpu_first_hit): one point per element of the sensor's film
 *            whatever its type, samples must be 0; d_normals [height][width][3] or NULL: their normals.
 *   target   of selected emitter e from point p.  Point and spot emitters: v = position - p, dist = |v|, dir = v / dist, the ray's range is
 *            [t_min, dist].  Directional emitters: dir = the direction to the emitter, range [t_min, inf), dist counts as 0.  Area emitters are
 *            refused.  t_min >= 0 keeps a surface point from shadowing itself.
 *   visible  a sample sees the emitter when dist is finite and > 0 (point and spot emitters), every coordinate of p is finite, with flag 1
 *            FRONT_ONLY dot(dir, n) > 0, and the shadow query (ads_t::shadow) finds nothing in the range.  A sample that fails one of the first
 *            two adds 0 to every sum.
 *   maps     [height][width][E][K] f32 per element and selected emitter, K = the floats of the bits of `maps`, in bit order:
 *              1  VISIBLE    1  float(n_visible) / float(samples) (samples == 0 counts as 1)
 *              2  DISTANCE   1  dist
 *              4  DIRECTION  3  dir (the mean is not renormalised)
 *              8  COS        1  dot(dir, n); needs a normal
 *            Every map but VISIBLE is the MEAN over ALL samples: an f32 sum in sample order, first term first, divided once by float(samples).
 *   elem     [height][width][Ke] f32 per element: 1 POINT (3), the mean sample point; 2 NEAREST_DISTANCE (1), the DISTANCE of the NEAREST emitter
 *            (0 without one).
 *   ids      [height][width][Ki] u32 per element: 1 N_VISIBLE, the selected emitters with at least one visible sample; 2 NEAREST, the index
 *            WITHIN THE SELECTION of the one of those with the smallest mean distance (the lowest index wins a tie, a directional emitter counts
 *            with 0), 0xFFFFFFFF without one.
 *   emitters n_emitters == 0: every emitter that is not an area emitter, in the scene's selection order (the emitter_list of
 *            wtgpu_scene_stats_json); else emitters[0 .. n_emitters), indices in that order, at most 32, none twice.
 *   d_mask   NULL, or [height][width] f32: an element with mask <= 0 traces nothing and holds 0 in every float, 0 / 0xFFFFFFFF in the ids — as an
 *            element whose point is not finite does.
 * Errors (WTGPU_ERR_INVALID with a message): no points and a sensor that is not virtual-plane, points with samples != 0, samples > 4096, more than
 * 32 emitters, an emitter index out of range, repeated or of an area emitter, an empty selection, unknown bits, COS or FRONT_ONLY without a
 * normal, t_min negative or not finite, a requested group whose pointer is NULL, nothing requested.  A group that is not requested may be NULL. */
typedef struct wtgpu_los_spec {
    uint32_t samples;
    uint32_t maps /* 1 VISIBLE, 2 DISTANCE, 4 DIRECTION, 8 COS */, elem /* 1 POINT, 2 NEAREST_DISTANCE */, ids /* 1 N_VISIBLE, 2 NEAREST */;
    uint32_t flags /* 1 FRONT_ONLY */, n_emitters;
    uint32_t emitters[32];
    float t_min;
    uint32_t pad;
    uint64_t seed;
} wtgpu_los_spec;
/* On the device, from and into the caller's DEVICE buffers, asynchronously on `stream`: one kernel — one lane per (element, sample) for the
 * sensor's own elements at 1 .. 64 samples, one lane per (element, emitter) otherwise (WTGPU_LOS_PER_SAMPLE=0: always); the result does not
 * depend on the form.  Needs an uploaded scene (WTGPU_ERR_INVALID otherwise); counts nothing and touches neither films nor counters. */
int wtgpu_line_of_sight(wtgpu_scene* scene, void* stream, const wtgpu_los_spec* spec, const float* d_points, const float* d_normals, const float* d_mask,
                        float* d_maps, float* d_elem, uint32_t* d_ids);
/* The same on `n_threads` host threads (0: all cores) from the host description, from and into HOST memory: bit for bit what
 * wtgpu_line_of_sight computes, and the result does not depend on n_threads.  No device needed. */
int wtgpu_line_of_sight_host(const wtgpu_scene* scene, const wtgpu_los_spec* spec, const float* points, const float* normals, const float* mask,
                             uint32_t n_threads, float* maps, float* elem, uint32_t* ids);

/* Profiling aid: `repeats` launches of a streaming copy of n_dwords 32-bit words (one dword per lane, coalesced: the access width
 * of the SoA path state) with a known byte count, used to calibrate rocprofv3's FETCH_SIZE / WRITE_SIZE (tools/profile_round.sh). */
int wtgpu_calibrate_copy(uint64_t n_dwords, int repeats);

/* Accumulated device counters since upload / last reset. */
int wtgpu_get_counters(wtgpu_scene* scene, wtgpu_counters* out);
int wtgpu_reset_counters(wtgpu_scene* scene);

/* Device time [ms] per kernel, ACCUMULATED over all wtgpu_render calls since upload / the last wtgpu_reset_counters, measured
 * with hipEvents on the internal streams the kernels are launched on (waits for the in-flight batches):
 * out[0]=generate, out[1]=trace (sum over rounds), out[2]=interact first pass (sum), out[3]=connect (4 kernels), out[4]=rounds with work,
 * out[5]=trace launches with work, out[6]=batches, out[7]=cooperative (heavy) trace (sum), out[8]=region edge sets + second
 * interaction pass (k_edges, k_interact_b), out[9]=region power sums (k_flux_split, k_flux_tasks), out[10]=Fraunhofer sampling pass
 * (k_interact_c), out[11] mean number of rounds launched per batch.  Batches run concurrently on
 * several streams, so the sums may exceed the wall time. */
int wtgpu_last_render_timings(wtgpu_scene* scene, float out[12]);

/* Host-side film development (render_context_t::develop, src/scene/render.cpp:245-291):
 * out[h][w][c] = value/weight (0 if weight==0) + light * (1/spe). */
int wtgpu_develop(const wtgpu_scene* scene, const double* value, const double* weight, const double* light, uint64_t spe, float* out);

/* The same development on the device, on `stream`: d_value / d_weight / d_light as wtgpu_render fills them, d_out [height][width][channels][stokes]
 * f32 in DEVICE memory — bit for bit what wtgpu_develop computes from the downloaded films.  Needs an uploaded scene (WTGPU_ERR_INVALID
 * otherwise); touches neither films nor counters. */
int wtgpu_develop_device(wtgpu_scene* scene, void* stream, const double* d_value, const double* d_weight, const double* d_light, uint64_t spe, float* d_out);

/* Tonemapping (tonemap_t: include/wt/sensor/response/tonemap/tonemap.hpp, src/sensor/response/tonemap.cpp:29-106).
 *   op    0 linear, 1 gamma: pow(clamp01(x), 1/gamma), 2 sRGB transfer of clamp01(x), 3 dB: clamp01((10 log10 x - db_min) / (db_max - db_min)), 0 for
 *         x == 0, NaN for x < 0; 4 function (a user expression: read from scene files, refused by the tonemap calls)
 *   mode  0 select (colour map for a 1-channel film, per channel for RGB), 1 normal (per channel; a single channel is repeated), 2 colourmap
 *         (the value, or the BT.709 luminance of RGB, through the map)
 * A colour map is a table of table_n (2 .. 1024) RGB f32 triples, sampled at v (table_n - 1) with linear interpolation.  The reference takes
 * its maps from tinycolormap, which is absent from its checkout: their tables are not reproduced (the library tabulates `grey` and `turbo`).
 *
 * The <tonemap> of the scene file's <response> (tonemap_t::load, tonemap.cpp:127-176), kept beside the flattened scene, which it does not change.
 * present = 0: the file has none (or there is no file) and op / mode are the response's defaults — sRGB / normal for an RGB film
 * (src/sensor/response/RGB.cpp:91-93), linear / select for a monochromatic one (monochromatic.cpp:65-66); colourmap is then "Magma"
 * (tonemap.hpp:80).  The strings are valid while the handle lives. */
typedef struct wtgpu_tonemap_spec {
    int32_t present, op, mode;
    float gamma, db_min, db_max;
    const char* colourmap;   /* the map's name as the file spells it */
    const char* function;    /* op 4: the expression's text */
} wtgpu_tonemap_spec;
int wtgpu_scene_tonemap_spec(const wtgpu_scene* scene, wtgpu_tonemap_spec* out);
typedef struct wtgpu_tonemap {
    int32_t op, mode;
    float gamma, db_min, db_max;
    const float* table;      /* HOST pointer, copied before the call returns; may be NULL when the mode sends nothing through a map */
    uint32_t table_n;
} wtgpu_tonemap;
/* Develops the planes of ONE Stokes component (plane index channel * stokes + stokes_component; < stokes of the scene, WTGPU_ERR_INVALID otherwise),
 * tonemaps them and writes [height][width][3] pixels — [height][width][4] with d_mask (DEVICE, [height][width] f32, e.g. wtgpu_sensor_mask's
 * result; may be NULL) as the fourth component — in `format`: 0 f32 (the alpha is the mask's bits), 1 8-bit, 2 16-bit codes (uint)(clamp01(x) max + 0.5),
 * NaN = code 0 (the alpha is quantised the same way).  One kernel on `stream`; the developed values never reach memory.  d_out: DEVICE, aligned to
 * 16 bytes.  tm = NULL: the scene's own spec; if that needs a colour map which is neither grey nor turbo the call fails and says to pass a
 * table.  Needs an uploaded scene (WTGPU_ERR_INVALID otherwise); touches neither films nor counters. */
int wtgpu_tonemap_device(wtgpu_scene* scene, void* stream, const double* d_value, const double* d_weight, const double* d_light, uint64_t spe,
                         const wtgpu_tonemap* tm, uint32_t stokes_component, const float* d_mask, uint32_t format, void* d_out);
/* The same computation on `n_threads` host threads (0: all cores) from HOST films into HOST memory; mask: HOST, may be NULL.  No device needed.
 * Bit for bit the device's wherever the operator calls no libm function (linear; the quantisation and the table lookup in every case). */
int wtgpu_tonemap_host(const wtgpu_scene* scene, const double* value, const double* weight, const double* light, uint64_t spe,
                       const wtgpu_tonemap* tm, uint32_t stokes_component, const float* mask, uint32_t format, uint32_t n_threads, void* out);

/* Film statistics: range, histogram and sum of the developed planes of ONE Stokes component — what choosing a dB range or an exposure needs,
 * and the distribution of received power over a coverage map — without the developed film leaving the device.
 *   planes   the film's channels (plane c: the developed value of film plane c * stokes + stokes_component, bit for bit wtgpu_develop's), plus one
 *            with flag 2 LUMINANCE (3-channel films only): the BT.709 luminance max(0, .2126 r + .7152 g + .0722 b) of the three, as the tonemap's
 *            colourmap mode computes it.  Flag 1 ABS: every element is |x| (the signed Stokes components Q / U / V).
 *   members  all elements, or with a mask ([height][width] f32, e.g. wtgpu_sensor_mask's result) those of the pixels where mask > 0.
 *   classes  a member is exactly one of: NaN; x < 0; x == 0; 0 < x < edge[0] (below); x >= edge[bins] (above); bin i with edge[i] <= x < edge[i+1].
 *   edges    bins + 1 strictly increasing f32 thresholds in x's own scale, computed once in f64 and rounded: scale 0 linear
 *            lo + i (hi - lo) / bins, scale 1 dB 10^((lo + i (hi - lo) / bins) / 10) with lo / hi in dB.  bins = 0: the one edge of lo.
 *   record   n members; min / max / min_positive over the members that are not NaN (NaN if there is none; -0 sorts below +0); sum in f64 over the
 *            same members in one fixed order (chunks of 256 in row-major order, each reduced pairwise at distances 128, 64 .. 1, the chunk
 *            sums reduced the same way), so device and host agree on every field bit for bit.
 * Errors (WTGPU_ERR_INVALID with a message): stokes_component >= the film's stokes, bins > 4096, lo >= hi with bins > 0 (or a value that is not
 * finite), LUMINANCE on a film that is not 3-channel, unknown scale or flags, edges that rounding made equal. */
typedef struct wtgpu_film_stats_spec {
    uint32_t stokes_component, scale /* 0 linear, 1 dB */, bins /* 0 .. 4096 */, flags /* 1 ABS, 2 LUMINANCE */;
    float lo, hi;
} wtgpu_film_stats_spec;
typedef struct wtgpu_film_stats {
    uint64_t n, n_nan, n_negative, n_zero, n_below, n_above;
    float min, max, min_positive, pad;
    double sum;
} wtgpu_film_stats;
/* the edge table of a spec: edges[bins + 1] (needs no scene; checks what it can of the spec) */
int wtgpu_film_stats_edges(const wtgpu_film_stats_spec* spec, float* edges);
/* On the device, on `stream`: one pass over d_value / d_weight / d_light (as wtgpu_render fills them) that develops in registers, then a small
 * kernel and the copy of the result, for which the call waits: out[planes] and hist[planes][bins] are HOST memory (hist may be NULL if bins == 0).
 * d_mask: DEVICE, may be NULL.  Needs an uploaded scene (WTGPU_ERR_INVALID otherwise); its scratch memory is allocated at the first call and
 * freed with the scene; touches neither films nor counters. */
int wtgpu_film_stats_device(wtgpu_scene* scene, void* stream, const double* d_value, const double* d_weight, const double* d_light, uint64_t spe,
                            const wtgpu_film_stats_spec* spec, const float* d_mask, wtgpu_film_stats* out, uint64_t* hist);
/* The same on `n_threads` host threads (0: all cores) from HOST films; the result does not depend on n_threads.  No device needed. */
int wtgpu_film_stats_host(const wtgpu_scene* scene, const double* value, const double* weight, const double* light, uint64_t spe,
                          const wtgpu_film_stats_spec* spec, const float* mask, uint32_t n_threads, wtgpu_film_stats* out, uint64_t* hist);

/* Film comparison: difference statistics of two sets of films of this scene's size, A and B, without either leaving the device — parity and A/B
 * checks, and the half-film noise estimate (two films that took alternating sample ranges: ||a - b|| / ||a + b|| from sum_sq, sum_a_sq, sum_b_sq).
 *   planes   as for the film statistics: the film's channels (plane c: the developed values xa, xb of film plane c * stokes + stokes_component of
 *            A with spe_a and of B with spe_b, bit for bit wtgpu_develop's), plus one with flag 2 LUMINANCE (3-channel films only); flag 1 ABS
 *            compares |xa| with |xb|.
 *   members  all pixels, or with a mask ([height][width] f32) those where mask > 0.
 *   classes  a member pair is non-finite (either value is NaN or infinite: counted in n_nonfinite, and in n_nonfinite_mismatch unless both are NaN
 *            or xa == xb; it enters no sum and not the maximum) or finite: d = (double)xa - (double)xb, counted in n_differ iff xa != xb (-0 and
 *            +0 do not differ).
 *   record   n members and the three counts; max_abs = max |d| over the finite pairs and argmax, the row-major index of the pixel that has it,
 *            the lowest on a tie — 0 and UINT64_MAX where no finite pair differs; five f64 sums over the finite pairs: sum_abs |d|, sum_sq d d,
 *            sum_a_sq xa xa, sum_b_sq xb xb, sum_rel d d / (xb xb + eps), each in the fixed order of the film statistics' sum, so device and host
 *            agree on every field bit for bit.
 *   diff     optional: [height][width][planes] f32, xa - xb as one f32 subtraction (whatever that gives for a non-finite pair; a NaN is stored
 *            as the quiet NaN 0x7fc00000), 0 for a pixel the mask excludes.
 * Errors (WTGPU_ERR_INVALID with a message): stokes_component >= the film's stokes, LUMINANCE on a film that is not 3-channel, unknown flags, an
 * eps that is not finite and > 0.  spe = 0 is what it is to wtgpu_develop: no light term. */
typedef struct wtgpu_film_compare_spec {
    uint32_t stokes_component, flags /* 1 ABS, 2 LUMINANCE */;
    double eps;
} wtgpu_film_compare_spec;
typedef struct wtgpu_film_compare {
    uint64_t n, n_nonfinite, n_nonfinite_mismatch, n_differ, argmax;
    double max_abs, sum_abs, sum_sq, sum_a_sq, sum_b_sq, sum_rel;
} wtgpu_film_compare;
/* On the device, on `stream`: one pass over both sets (as wtgpu_render fills them; A and B may be the same memory) that develops in registers and
 * writes d_diff (DEVICE, may be NULL) on its way, then a small kernel and the copy of the records, for which the call waits: out[planes] is HOST
 * memory.  d_mask: DEVICE, may be NULL.  Needs an uploaded scene (WTGPU_ERR_INVALID otherwise); its scratch memory is allocated at the first call
 * and freed with the scene; touches neither films nor counters. */
int wtgpu_film_compare_device(wtgpu_scene* scene, void* stream, const double* a_value, const double* a_weight, const double* a_light, uint64_t spe_a,
                              const double* b_value, const double* b_weight, const double* b_light, uint64_t spe_b, const wtgpu_film_compare_spec* spec,
                              const float* d_mask, wtgpu_film_compare* out, float* d_diff);
/* The same on `n_threads` host threads (0: all cores) from HOST films; diff: HOST, may be NULL; the result does not depend on n_threads.  No device needed. */
int wtgpu_film_compare_host(const wtgpu_scene* scene, const double* a_value, const double* a_weight, const double* a_light, uint64_t spe_a,
                            const double* b_value, const double* b_weight, const double* b_light, uint64_t spe_b, const wtgpu_film_compare_spec* spec,
                            const float* mask, uint32_t n_threads, wtgpu_film_compare* out, float* diff);

/* Polarisation view of a polarimetric film (stokes == 4): degrees and angles of polarisation, the film through an analyser, Stokes sums and the
 * false-colour polarisation picture, all derived from the four developed components together without the film leaving the device.
 *   planes   the film's channels (plane c: the Stokes vector (I, Q, U, V) of the developed values of film planes c * 4 + s, bit for bit
 *            wtgpu_develop's, widened to f64), plus one with flag 2 LUMINANCE (3-channel films only): the vector .2126 S_r + .7152 S_g + .0722 S_b,
 *            component by component in f64, added left to right and NOT clamped at 0 (linear in S, unlike the tonemap's luminance).
 *   values   lin = sqrt(Q Q + U U), pol = sqrt((Q Q + U U) + V V), dolp = lin / I, dop = pol / I, docp = V / I, analyser = (I + Q c2 + U s2) / 2 with
 *            c2 = cos 2 theta, s2 = sin 2 theta of the analyser's angle, aolp = atan2(U, Q) / 2 in (-pi/2, pi/2] and chi = atan2(V, lin) / 2, in f64 with
 *            + - x / and sqrt only; the arc tangent is the library's own polynomial (absolute error below 1.2e-11 rad; a zero of either sign counts as
 *            +0, aolp = 0 where lin == 0), so that device and host agree on every value bit for bit.  Each is rounded to f32 once.
 *   members  all pixels, or with a mask ([height][width] f32) those where mask > 0.
 *   classes  a member is, per plane, non-finite (any of I, Q, U, V is NaN or infinite: counted in n_nonfinite, every map value the quiet NaN
 *            0x7fc00000), dark (finite and not I > 0: counted in n_dark; dolp, dop, docp, aolp, chi are 0, analyser is computed) or lit; only lit
 *            pixels enter the sums and the maximum, and a lit pixel is counted in n_over iff (Q Q + U U) + V V > I I (more polarised than bright: noise).
 *   record   n members and the three counts; max_dop = max dop over the lit pixels and argmax, the row-major index of the pixel that has it, the
 *            lowest on a tie — 0 and UINT64_MAX where no pixel is lit; six f64 sums over the lit pixels, of I, Q, U, V, lin and pol, each in the
 *            fixed order of the film statistics' sum, so device and host agree on every field bit for bit.
 *   maps     optional: [height][width][planes][k] f32, the k maps chosen by the bits of `maps` in the order 1 DOLP, 2 DOP, 4 DOCP, 8 AOLP, 16 CHI,
 *            32 ANALYSER; 0 for a pixel the mask excludes.
 *   picture  optional: the false-colour view of plane `picture_plane`, [height][width][3] — [height][width][4] with the mask as the fourth
 *            component, as wtgpu_tonemap_device appends it — in `format` (0 f32, 1 8-bit, 2 16-bit codes; NaN = code 0): hue = aolp / pi + 1/2,
 *            saturation = clamp01(dolp x sat_gain), value = clamp01(op(I)) with the operator, gamma and dB range of `tonemap` (its mode and table are
 *            not used), HSV -> RGB by the sextant formula in f32; hue and saturation are 0 for a pixel that is not lit.  Every pixel is shown.
 * Errors (WTGPU_ERR_INVALID with a message): a film that is not polarimetric, LUMINANCE on a film that is not 3-channel, unknown flag or map bits,
 * c2, s2 or sat_gain that is not finite, sat_gain < 0, picture_plane >= planes, an unknown format or operator (the `function` operator is refused as
 * the tonemap calls refuse it).  A zeroed spec is valid: no luminance, no maps, a linear picture of plane 0 without saturation. */
typedef struct wtgpu_film_polar_spec {
    uint32_t flags /* 2 LUMINANCE */, maps /* 1 DOLP, 2 DOP, 4 DOCP, 8 AOLP, 16 CHI, 32 ANALYSER */, picture_plane, format /* 0 f32, 1 u8, 2 u16 */;
    double c2, s2;
    float sat_gain, pad;
    wtgpu_tonemap tonemap;
} wtgpu_film_polar_spec;
typedef struct wtgpu_film_polar {
    uint64_t n, n_nonfinite, n_dark, n_over, argmax;
    double max_dop, sum_i, sum_q, sum_u, sum_v, sum_lin, sum_pol;
} wtgpu_film_polar;
/* On the device, on `stream`: one pass over d_value / d_weight / d_light (as wtgpu_render fills them) that develops in registers and writes d_maps
 * and d_picture (DEVICE, each may be NULL) on its way, then a small kernel and the copy of the records, for which the call waits: out[planes] is
 * HOST memory.  d_mask: DEVICE, may be NULL.  Needs an uploaded scene (WTGPU_ERR_INVALID otherwise); its scratch memory is allocated at the first
 * call and freed with the scene; touches neither films nor counters. */
int wtgpu_film_polar_device(wtgpu_scene* scene, void* stream, const double* d_value, const double* d_weight, const double* d_light, uint64_t spe,
                            const wtgpu_film_polar_spec* spec, const float* d_mask, wtgpu_film_polar* out, float* d_maps, void* d_picture);
/* The same on `n_threads` host threads (0: all cores) from HOST films; maps, picture: HOST, may be NULL; the result does not depend on n_threads.
 * No device needed.  The picture is bit for bit the device's with the linear operator (the others call libm: within one code). */
int wtgpu_film_polar_host(const wtgpu_scene* scene, const double* value, const double* weight, const double* light, uint64_t spe,
                          const wtgpu_film_polar_spec* spec, const float* mask, uint32_t n_threads, wtgpu_film_polar* out, float* maps, void* picture);

/* The four film passes above on either kind of film: the accumulators, or a DEVELOPED film — what wtgpu_develop_device and the denoisers
 * (wtgpu_film_denoise_device, its guided form; the filtered film and the residual) write, so that a denoised film is shown, measured and compared
 * where it lies.  A source is exactly one of the two forms:
 *   value, weight, light + spe   the accumulators as wtgpu_render fills them; an element is wtgpu_develop's value of them;
 *   developed                    [height][width][channels][stokes] f32; an element is the f32 as it lies there — any f32: NaNs of any payload,
 *                                infinities, -0 and subnormals are what each pass's rules above say they are.  spe is not read.  No alignment
 *                                beyond a float's is asked of the pointer.
 * Both forms set, neither, or a partly set accumulator triple: WTGPU_ERR_INVALID with a message.  Everything behind the element value — planes,
 * luminance, ABS, classes, the sums' fixed order, extrema, records, maps, operator, mode, table, quantisation, mask — is the same code, so a pass
 * on wtgpu_develop's output of a set of accumulators gives what it gives on the accumulators, bit for bit.  The remaining arguments, the errors
 * and their messages are the sibling's; the *_device forms take DEVICE memory in the sources, the *_host forms HOST memory.  The comparison takes
 * two sources in any combination (a denoised film against a long render's accumulators; the same memory twice is fine).  The entry points above
 * are these with accumulator sources. */
typedef struct wtgpu_film_source {
    const double *value, *weight, *light;   /* the accumulators, with spe ... */
    uint64_t spe;
    const float* developed;                 /* ... or a developed film */
} wtgpu_film_source;
int wtgpu_tonemap_source_device(wtgpu_scene* scene, void* stream, const wtgpu_film_source* film, const wtgpu_tonemap* tm, uint32_t stokes_component,
                                const float* d_mask, uint32_t format, void* d_out);
int wtgpu_tonemap_source_host(const wtgpu_scene* scene, const wtgpu_film_source* film, const wtgpu_tonemap* tm, uint32_t stokes_component, const float* mask,
                              uint32_t format, uint32_t n_threads, void* out);
int wtgpu_film_stats_source_device(wtgpu_scene* scene, void* stream, const wtgpu_film_source* film, const wtgpu_film_stats_spec* spec, const float* d_mask,
                                   wtgpu_film_stats* out, uint64_t* hist);
int wtgpu_film_stats_source_host(const wtgpu_scene* scene, const wtgpu_film_source* film, const wtgpu_film_stats_spec* spec, const float* mask, uint32_t n_threads,
                                 wtgpu_film_stats* out, uint64_t* hist);
int wtgpu_film_compare_source_device(wtgpu_scene* scene, void* stream, const wtgpu_film_source* a, const wtgpu_film_source* b, const wtgpu_film_compare_spec* spec,
                                     const float* d_mask, wtgpu_film_compare* out, float* d_diff);
int wtgpu_film_compare_source_host(const wtgpu_scene* scene, const wtgpu_film_source* a, const wtgpu_film_source* b, const wtgpu_film_compare_spec* spec,
                                   const float* mask, uint32_t n_threads, wtgpu_film_compare* out, float* diff);
int wtgpu_film_polar_source_device(wtgpu_scene* scene, void* stream, const wtgpu_film_source* film, const wtgpu_film_polar_spec* spec, const float* d_mask,
                                   wtgpu_film_polar* out, float* d_maps, void* d_picture);
int wtgpu_film_polar_source_host(const wtgpu_scene* scene, const wtgpu_film_source* film, const wtgpu_film_polar_spec* spec, const float* mask, uint32_t n_threads,
                                 wtgpu_film_polar* out, float* maps, void* picture);

/* Zonal film statistics: ONE pass over a film under a u32 label plane that keeps a statistics record per (zone, plane) — received power under line
 * of sight against without it, per best-server cell (line_of_sight's NEAREST), per distance ring, per shape or material under a camera pixel
 * (first_hit's ids), per block of cells — where a masked wtgpu_film_stats call per class would take one pass each.
 *   elements, planes, members   the film statistics' on either kind of source: the film's channels (+ 1 with flag 2 LUMINANCE), flag 1 ABS, mask > 0.
 *   zone      zones[height][width] u32: a member pixel with zones[p] < n_zones belongs to that zone; any other member pixel (0xFFFFFFFF, the id
 *             maps' "no hit", included) to none and is counted once in *n_outside.  1 <= n_zones <= 65536.
 *   record    out[n_zones][planes]: n members; the film statistics' classes against the same edge table (wtgpu_film_stats_edges of the spec's
 *             scale, bins, lo, hi); n_inf counts the infinite elements (also counted as negative or above); min / max over the elements that are
 *             not NaN (NaN if there is none; -0 sorts below +0).  hist[n_zones][planes][bins]; n_zones x bins <= 2^20.
 *   sum       over the zone's FINITE elements: the exact real sum rounded once to the nearest f64 (ties to even; +0.0 where it is zero) — not the
 *             film statistics' pairwise sum.  It does not depend on the order of the additions, so device and host agree on every field bit for
 *             bit, and it is what Python's math.fsum gives.
 *   paint     optional: [height][width][planes] f32, every pixel painted with (float)(sum / (double)(n - n_nan - n_inf)) of its zone — the zone means
 *             as a developed film, which the tonemap calls show; 0 for a pixel the mask excludes, one outside every zone, or a zone without a
 *             finite element.
 * Errors (WTGPU_ERR_INVALID with a message): everything the film statistics refuse, in their words; n_zones of 0 or above 65536; n_zones x bins
 * above 2^20; zones, out or n_outside NULL; hist NULL with bins > 0; a film of 2^31 pixels or more. */
typedef struct wtgpu_film_zonal_spec {
    uint32_t stokes_component, scale /* 0 linear, 1 dB */, bins /* 0 .. 4096 */, flags /* 1 ABS, 2 LUMINANCE */, n_zones /* 1 .. 65536 */;
    float lo, hi;
} wtgpu_film_zonal_spec;
typedef struct wtgpu_film_zonal {
    uint64_t n, n_nan, n_inf, n_negative, n_zero, n_below, n_above;
    float min, max;
    double sum;
} wtgpu_film_zonal;
/* On the device, on `stream`: one pass over the film and d_zones (DEVICE; d_mask and d_paint: DEVICE, each may be NULL), two small kernels and the
 * copy of the result, for which the call waits: out, hist (may be NULL if bins == 0) and n_outside are HOST memory.  Needs an uploaded scene
 * (WTGPU_ERR_INVALID otherwise); its scratch memory is sized by the call, grown when a later call needs more and freed with the scene; touches
 * neither films nor counters. */
int wtgpu_film_zonal_device(wtgpu_scene* scene, void* stream, const wtgpu_film_source* film, const wtgpu_film_zonal_spec* spec, const uint32_t* d_zones,
                            const float* d_mask, wtgpu_film_zonal* out, uint64_t* hist, uint64_t* n_outside, float* d_paint);
/* The same on `n_threads` host threads (0: all cores) from HOST memory; the result does not depend on n_threads.  No device needed. */
int wtgpu_film_zonal_host(const wtgpu_scene* scene, const wtgpu_film_source* film, const wtgpu_film_zonal_spec* spec, const uint32_t* zones, const float* mask,
                          uint32_t n_threads, wtgpu_film_zonal* out, uint64_t* hist, uint64_t* n_outside, float* paint);

/* Connected segments of a label plane: which REGION a pixel lies in, where the id maps and zone planes say which class — the coverage holes below
 * a threshold, the shadow behind one building (line_of_sight's n_visible == 0), one visible fragment of a shape.  The result is canonical: it
 * depends on no order of execution and holds no floating-point number, so device and host agree bit for bit.
 *   inputs    classes[height][width] u32 or NULL (every pixel has class 0); mask[height][width] f32 or NULL.
 *   member    pixel p is a member iff (mask == NULL or mask[p] > 0 — a NaN is not) and classes[p] != 0xFFFFFFFF (the id maps' "no hit").
 *   link      two members are linked iff they have the same class and are neighbours: the 4 edge neighbours, with flag 1 DIAGONAL the 4 corner
 *             neighbours as well.  Rows do not wrap.
 *   segment   a connected component of the link graph.  first: its smallest row-major pixel index; area: its pixel count; klass: its class;
 *             x0, y0, x1, y1: its inclusive bounding box; sum_x, sum_y: the sums of its pixels' coordinates (the centroid is sum / area).
 *   kept      a segment is kept iff area >= max(min_area, 1); kept segments are numbered 0 .. K - 1 in ascending `first`.
 *   segments  [height][width] u32: the number of the pixel's segment; 0xFFFFFFFF for a pixel that is no member or whose segment was dropped.
 *             wtgpu_film_zonal_* takes this plane as `zones` as it is.
 *   info      n_segments = K, n_dropped (segments), n_members (pixels), n_dropped_pixels (members of dropped segments).
 *   records   optional, HOST memory: the first min(K, max_records) kept segments; max_records may be 0 with records == NULL.
 * Errors (WTGPU_ERR_INVALID with a message opened by "film_segments:"): segments or info NULL; records NULL with max_records > 0; flags other than
 * 0 / 1; a sensor of 2^31 pixels or more; the device call without an upload. */
typedef struct wtgpu_film_segments_spec {
    uint32_t flags /* 1 DIAGONAL */, min_area, max_records, pad;
} wtgpu_film_segments_spec;
typedef struct wtgpu_film_segments_info {
    uint64_t n_segments, n_dropped, n_members, n_dropped_pixels;
} wtgpu_film_segments_info;
typedef struct wtgpu_film_segment {
    uint32_t klass, area, first, x0, y0, x1, y1, pad;
    uint64_t sum_x, sum_y;
} wtgpu_film_segment;
/* On the device, on `stream`: d_classes, d_mask (each may be NULL) and d_segments are DEVICE memory; info and records are HOST memory, and the call
 * waits for them.  A union-find in global memory (csrc/kernels_segments.hip); every one of its loops carries a step bound, and a call in which one
 * was hit returns WTGPU_ERR_HIP with a message, d_segments then holding nothing to be read.  Needs an uploaded scene; its scratch memory is
 * sized by the call, grown when a later call needs more and freed with the scene; touches neither films nor counters. */
int wtgpu_film_segments_device(wtgpu_scene* scene, void* stream, const wtgpu_film_segments_spec* spec, const uint32_t* d_classes, const float* d_mask,
                               uint32_t* d_segments, wtgpu_film_segments_info* info, wtgpu_film_segment* records);
/* The same from HOST memory; n_threads is accepted (0: all cores) and the result does not depend on it.  No device needed. */
int wtgpu_film_segments_host(const wtgpu_scene* scene, const wtgpu_film_segments_spec* spec, const uint32_t* classes, const float* mask, uint32_t n_threads,
                             uint32_t* segments, wtgpu_film_segments_info* info, wtgpu_film_segment* records);

/* Distance transform of a label plane: how FAR a pixel lies from the nearest site, exactly, and which site that is — distance to coverage, depth
 * inside a hole and its deepest point, the nearest region, rings around a region, erode / dilate by a radius.  The result holds no
 * floating-point number and ties are broken by pixel index, so device and host agree bit for bit.
 *   inputs    classes[height][width] u32 or NULL (every pixel has class 0); mask[height][width] f32 or NULL.
 *   member    as for wtgpu_film_segments_*: (mask == NULL or mask[p] > 0 — a NaN is not) and classes[p] != 0xFFFFFFFF.
 *   site      the members; with flag 1 INVERT the pixels that are no members.  The film's outside holds no site.
 *   dist2     [height][width] u32: the minimum over the sites s of (x - xs)^2 + (y - ys)^2; 0 on a site; 0xFFFFFFFF everywhere where the plane has no site.
 *   nearest   optional [height][width] u32: the row-major index of a site at that distance, of several the smallest index; 0xFFFFFFFF without a site.
 *   info      n_sites: the number of sites; max_dist2: the maximum of dist2 over all pixels; argmax: the lowest pixel index that attains it.  No
 *             special cases: an all-sites plane gives 0 / 0, a plane without a site 0xFFFFFFFF / 0.
 * Errors (WTGPU_ERR_INVALID with a message opened by "film_distance:"): dist2 or info NULL; flags other than 0 / 1; a sensor wider or higher than
 * 32768 pixels (so that every dist2 stays below 2^31 and a vertical offset fits 16 bits); the device call without an upload. */
typedef struct wtgpu_film_distance_spec {
    uint32_t flags /* 1 INVERT */, pad[3];
} wtgpu_film_distance_spec;
typedef struct wtgpu_film_distance_info {
    uint64_t n_sites, argmax;
    uint32_t max_dist2, pad;
} wtgpu_film_distance_info;
/* On the device, on `stream`: d_classes, d_mask (each may be NULL), d_dist2 and d_nearest (may be NULL) are DEVICE memory; info is HOST memory, and
 * the call waits for it.  Two kernels (csrc/kernels_distance.hip): the columns, then the rows; their loops are counted by the height and the
 * width and wait for nobody.  Needs an uploaded scene; its scratch memory (16 bits per pixel and a little more) is sized by the call, grown when
 * a later call needs more and freed with the scene; touches neither films nor counters. */
int wtgpu_film_distance_device(wtgpu_scene* scene, void* stream, const wtgpu_film_distance_spec* spec, const uint32_t* d_classes, const float* d_mask,
                               uint32_t* d_dist2, uint32_t* d_nearest, wtgpu_film_distance_info* info);
/* The same from HOST memory; n_threads: 0 all cores, and the result does not depend on it.  nearest may be NULL.  No device needed. */
int wtgpu_film_distance_host(const wtgpu_scene* scene, const wtgpu_film_distance_spec* spec, const uint32_t* classes, const float* mask, uint32_t n_threads,
                             uint32_t* dist2, uint32_t* nearest, wtgpu_film_distance_info* info);

/* Denoising a film from its two half-films A and B (two renders of disjoint sample ranges, as render_to_noise keeps them) without the films leaving
 * the device: the dual-buffer non-local-means filter of Rousselle, Knaus and Zwicker 2012 — the weights that filter one half are computed from the
 * other, the per-pixel variance comes from (a - b)^2, and the difference of the two filtered halves estimates the error that is left.
 *   planes     all P = channels x stokes planes of a pixel are filtered with ONE set of weights (a Stokes vector is filtered as one thing): a_i, b_i are
 *              the developed values of plane i with spe_a / spe_b, bit for bit wtgpu_develop's.  The guide planes, from which the weights come, are
 *              Stokes component 0 of each channel.
 *   variance   e_c = (a_c - b_c)^2 / 2 per guide plane; v_c = the mean of e_c over the 3 x 3 neighbourhood, coordinates clamped to the film.
 *   weights    of a candidate q = p + (dx, dy), |dx|, |dy| <= window_radius, for the guide buffer y: the mean over the patch of (2 patch_radius + 1)^2
 *              pixels (coordinates clamped to the film, p's and q's separately) and the guide planes of
 *                ((y_c(p) - y_c(q))^2 - alpha (v_c(p) + min(v_c(p), v_c(q)))) / (eps + k^2 (v_c(p) + v_c(q)))
 *              is D; w = 1 where D <= 0, exp(-D) otherwise (the library's own polynomial: relative error below 1e-6; 0 from 2^-126 down), 0 for a NaN.
 *              There is no cutoff.  A candidate lies inside the film, is valid (every plane of a and of b finite there) and, with a mask
 *              ([height][width] f32), has mask > 0.
 *   filter     fa_i(p) = a_i(p) + sum_q w_b(p, q) (a_i(q) - a_i(p)) / sum_q w_b(p, q) with the weights of guide b, fb likewise with the weights of
 *              guide a; the sums run over the candidates in row-major order of (dy, dx), in f32.
 *   out        (fa_i + fb_i) / 2;  residual (may be NULL): (fa_i - fb_i) / 2.  Both [height][width][channels][stokes] f32, the layout of
 *              wtgpu_develop_device's result.  A pixel that is not valid, not in the mask, or has no positive sum of weights (next to a non-finite pixel)
 *              passes through: out = (a_i + b_i) / 2, residual = (a_i - b_i) / 2.  A NaN is stored as 0x7fc00000.
 * All arithmetic is f32 + - x / in one fixed order (wt/film_denoise.h) and calls no libm function: device and host agree on every value bit for
 * bit; a constant film comes back as itself and window_radius 0 gives (a + b) / 2, both bit for bit.
 * Errors (WTGPU_ERR_INVALID with a message): window_radius > 10, patch_radius > 3, k not finite or <= 0, alpha not finite or < 0, eps not finite
 * or <= 0, nonzero flags, a film whose channel count is not 1 or 3. */
typedef struct wtgpu_film_denoise_spec {
    uint32_t window_radius /* r: 0 .. 10 */, patch_radius /* f: 0 .. 3 */, flags /* none yet: must be 0 */, pad;
    float k /* 0.45 */, alpha /* 1 */, eps /* 1e-10 */, pad2;
} wtgpu_film_denoise_spec;
/* On the device, on `stream`: a_* / b_* are the DEVICE films of the two halves as wtgpu_render fills them (A and B may be the same memory), d_mask
 * DEVICE or NULL, d_out and d_residual (may be NULL) DEVICE.  Nothing returns to the host, so the call is asynchronous on `stream`.  Needs an
 * uploaded scene (WTGPU_ERR_INVALID otherwise); its scratch memory (the developed halves, 3 P + 2 channels floats and two bytes per pixel) is allocated
 * at the first call, shared by all calls — order calls on different streams yourself — and freed with the scene; touches neither films nor counters. */
int wtgpu_film_denoise_device(wtgpu_scene* scene, void* stream, const double* a_value, const double* a_weight, const double* a_light, uint64_t spe_a,
                              const double* b_value, const double* b_weight, const double* b_light, uint64_t spe_b, const wtgpu_film_denoise_spec* spec,
                              const float* d_mask, float* d_out, float* d_residual);
/* The same on `n_threads` host threads (0: all cores) from HOST films; mask, residual: HOST, may be NULL; the result does not depend on n_threads.
 * No device needed.  Naive per pixel and candidate (seconds for a full-size film): the reference the device is held to, not a fast path. */
int wtgpu_film_denoise_host(const wtgpu_scene* scene, const double* a_value, const double* a_weight, const double* a_light, uint64_t spe_a,
                            const double* b_value, const double* b_weight, const double* b_light, uint64_t spe_b, const wtgpu_film_denoise_spec* spec,
                            const float* mask, uint32_t n_threads, float* out, float* residual);

/* The same filter steered by noise-free feature planes (Rousselle, Manzi and Zwicker 2013: min(w_colour, w_feature), here with one exponential) —
 * what wtgpu_first_hit produces: normals, depth, coverage, shape ids.  Colour-only weights cannot keep what is weaker than the noise; a guide can.
 *   guide      d_guide[height][width][n_guides] f32, 0 <= n_guides <= 8, with scale[g] finite and >= 0 per plane.
 *   distance   F(p, q) = sum over g of ((g_g(p) - g_g(q))^2 x scale[g]), sequentially from +0 in plane order; pointwise, no patch.
 *   weight     with D the colour distance above: w = weight(F) where F is a NaN (0), else weight(F > D ? F : D).  A NaN D still gives 0.
 *   non-finite a non-finite guide value at p or q gives weight 0: such a pixel is nobody's candidate, has no positive sum itself and passes through.
 *   ids        with flag 1 (SAME_ID) a candidate must also have d_ids[q] == d_ids[p] ([height][width] u32): a candidate condition like the mask.
 * Everything else — variance, patch distance, orders, pass-through, one set of weights for all planes and both directions — is the unguided call's.
 * All scales 0 with finite guides, or one id everywhere, give the unguided result bit for bit; a guide that separates regions by F >= 126 / log2 e
 * equals SAME_ID with the region index.  f32 + - x and comparisons only: device and host agree bit for bit.
 * Errors (WTGPU_ERR_INVALID with a message): n_guides > 8, unknown flag bits, a scale that is not finite or negative, a guide / id pointer missing
 * where it is needed or given where it is not used (d_guide NULL iff n_guides == 0, d_ids NULL iff not SAME_ID), neither guides nor SAME_ID (that
 * is the unguided call), and everything the unguided call refuses, with its messages (spec->flags stays 0). */
typedef struct wtgpu_film_denoise_guides {
    uint32_t n_guides /* 0 .. 8 */, flags /* 1 SAME_ID */;
    float scale[8];
} wtgpu_film_denoise_guides;
/* On the device, asynchronous on `stream`; d_guide, d_ids DEVICE.  Needs an uploaded scene; uses the unguided call's scratch memory and no more;
 * touches neither films nor counters. */
int wtgpu_film_denoise_guided_device(wtgpu_scene* scene, void* stream, const double* a_value, const double* a_weight, const double* a_light, uint64_t spe_a,
                                     const double* b_value, const double* b_weight, const double* b_light, uint64_t spe_b, const wtgpu_film_denoise_spec* spec,
                                     const wtgpu_film_denoise_guides* guides, const float* d_guide, const uint32_t* d_ids, const float* d_mask, float* d_out,
                                     float* d_residual);
/* The same from HOST memory on `n_threads` host threads (0: all cores): the reference the device is held to, bit for bit. */
int wtgpu_film_denoise_guided_host(const wtgpu_scene* scene, const double* a_value, const double* a_weight, const double* a_light, uint64_t spe_a,
                                   const double* b_value, const double* b_weight, const double* b_light, uint64_t spe_b, const wtgpu_film_denoise_spec* spec,
                                   const wtgpu_film_denoise_guides* guides, const float* guide, const uint32_t* ids, const float* mask, uint32_t n_threads,
                                   float* out, float* residual);

void wtgpu_scene_destroy(wtgpu_scene* scene);
const char* wtgpu_last_error(void);
const char* wtgpu_scene_stats_json(const wtgpu_scene* scene);

#ifdef __cplusplus
}
#endif
#endif /* WTGPU_H */
