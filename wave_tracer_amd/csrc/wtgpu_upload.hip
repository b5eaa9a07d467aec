// wave_tracer_amd — wtgpu_scene_upload: the scene's arrays to the device, the size of a batch, the state of each slice; and their release.
#include "wtgpu_host.h"

// The HIP runtime stages by-value kernel arguments in a 1 MiB ring per stream; a batch enqueues ~1000 launches of ~1 KB, and a full ring blocks
// the enqueueing thread until the GPU has caught up — which serialises the internal streams.  Ask for 16 MiB before the runtime reads its
// settings (it does so at its first use; a process that initialised HIP earlier sets HSA_KERNARG_POOL_SIZE itself).  This is
// only a default (a host's own setting wins) and takes effect only if the runtime has not initialised yet; g_env_by_host records whether the
// host had set it itself, wtgpu_scene_upload refuses a setting that is KNOWN to serialise the streams (runtime_settings_ok).
static int g_env_by_host = 0;   // bit 0: HSA_KERNARG_POOL_SIZE was in the environment when the library was loaded
__attribute__((constructor)) static void wtgpu_runtime_settings() {
    if (getenv("HSA_KERNARG_POOL_SIZE")) g_env_by_host |= 1;
    setenv("HSA_KERNARG_POOL_SIZE", "16777216", 0);
}
// The runtime setting the stream pipeline needs.  An explicit setting that is too small is an ERROR (it would silently cost
// 30-50 % — WTGPU_ALLOW_SLOW_RUNTIME=1 overrides); a setting this library had to default itself is reported once: it is in effect only if HIP
// was not initialised before libwtgpu.so was loaded, which cannot be queried.
static int runtime_settings_ok(std::string& why) {
    const char* k = getenv("HSA_KERNARG_POOL_SIZE");
    const long ring = k ? atol(k) : (1l << 20);
    if (getenv("WTGPU_ALLOW_SLOW_RUNTIME")) return 1;
    if (ring < (4l << 20)) {
        why = "HSA_KERNARG_POOL_SIZE=" + std::string(k ? k : "(unset)") + ": a batch enqueues ~900 launches of ~1 KB of kernel arguments; with a ring below 4 MiB the enqueueing "
              "thread blocks and the streams serialise; export HSA_KERNARG_POOL_SIZE=16777216 before the HIP runtime initialises, or WTGPU_ALLOW_SLOW_RUNTIME=1";
        return 0;
    }
    if (!(g_env_by_host & 1) && !getenv("WTGPU_QUIET")) {
        static bool told = false;
        if (!told) fprintf(stderr, "[wtgpu] note: HSA_KERNARG_POOL_SIZE=16777216 defaulted by libwtgpu.so; effective only if the HIP runtime had not initialised before the library was loaded "
                           "(a host that uses HIP earlier exports it itself, INTEGRATION.md)\n");
        told = true;
    }
    return 1;
}

// step 1: the flattened scene's arrays, plus what the device keeps next to them (bounding spheres, quantised nodes, triangle classes)
static int upload_scene_arrays(wtgpu_scene* s) {
    const scene_t& h = s->host;
    scene_t d = h;
    int rc;
#define UP(field, n) \
    if ((rc = upload(s, h.field, (size_t)(n), &d.field)) != WTGPU_OK) return rc;
    {   // the triangles, and behind them — same allocation — their bounding spheres (coop_tri_spheres, wt/coop.h: the first filter of the
        // wave-cooperative queries)
        d.tri_geo = nullptr;
        if (h.n_tris > 0 && h.tri_geo) {
            const size_t nt = h.n_tris;
            std::vector<float> sph(4 * nt);
            for (size_t i = 0; i < nt; ++i) tri_bounding_sphere(h.tri_geo[i].a, h.tri_geo[i].b, h.tri_geo[i].c, &sph[4 * i]);
            void* p = nullptr;
            HIP_CHECK(hipMalloc(&p, nt * (sizeof(tri_geo_t) + 16)));
            s->dev_allocs.push_back(p);
            HIP_CHECK(hipMemcpy(p, h.tri_geo, nt * sizeof(tri_geo_t), hipMemcpyHostToDevice));
            HIP_CHECK(hipMemcpy(static_cast<char*>(p) + nt * sizeof(tri_geo_t), sph.data(), nt * 16, hipMemcpyHostToDevice));
            d.tri_geo = static_cast<const tri_geo_t*>(p);
        }
    }
    UP(tri_meta, h.n_tris)
    UP(tri_shade, h.n_tris)
    UP(edges, h.n_edges)
    {   // the nodes, and behind them — same allocation — the 128-byte nodes of the per-lane traversals and their grid (wt/bvh.h: lane_nodes)
        d.nodes = nullptr;
        if (h.n_nodes > 0 && h.nodes) {
            const size_t nn = h.n_nodes;
            vec3 mn{WT_INF, WT_INF, WT_INF}, mx{-WT_INF, -WT_INF, -WT_INF};
            for (size_t i = 0; i < nn; ++i)
                for (int c = 0; c < 8; ++c)
                    if (h.nodes[i].child[c] != 0) {
                        mn = vmin(mn, vec3{h.nodes[i].minx[c], h.nodes[i].miny[c], h.nodes[i].minz[c]});
                        mx = vmax(mx, vec3{h.nodes[i].maxx[c], h.nodes[i].maxy[c], h.nodes[i].maxz[c]});
                    }
            const qgrid_t g = qgrid_make(mn, mx);
            std::vector<bvh8_qnode_t> qn(nn);
            bool ok = finitef(mn.x) && finitef(mn.y) && finitef(mn.z) && finitef(mx.x) && finitef(mx.y) && finitef(mx.z);
            for (size_t i = 0; i < nn && ok; ++i) ok = qnode_make(h.nodes[i], g, qn[i]);
            if (!ok) return fail(WTGPU_ERR_INVALID, "the scene's BVH boxes cannot be enclosed by the 16-bit node grid (non-finite or out-of-range box)");
            const float gw[8] = {g.origin.x, g.origin.y, g.origin.z, g.cell.x, g.cell.y, g.cell.z, 0.f, 0.f};
            void* p = nullptr;
            HIP_CHECK(hipMalloc(&p, nn * (sizeof(bvh8_node_t) + sizeof(bvh8_qnode_t)) + sizeof(gw)));
            s->dev_allocs.push_back(p);
            HIP_CHECK(hipMemcpy(p, h.nodes, nn * sizeof(bvh8_node_t), hipMemcpyHostToDevice));
            HIP_CHECK(hipMemcpy(static_cast<char*>(p) + nn * sizeof(bvh8_node_t), qn.data(), nn * sizeof(bvh8_qnode_t), hipMemcpyHostToDevice));
            HIP_CHECK(hipMemcpy(static_cast<char*>(p) + nn * (sizeof(bvh8_node_t) + sizeof(bvh8_qnode_t)), gw, sizeof(gw), hipMemcpyHostToDevice));
            d.nodes = static_cast<const bvh8_node_t*>(p);
        }
    }
    UP(leaves, h.n_leaves)
    UP(shapes, h.n_shapes)
    const scene_extents_t ex = scene_extents(h);
    UP(shape_tri_tuid, ex.shape_tris)
    UP(shape_tri_cdf, ex.shape_tris + h.n_shapes)
    UP(materials, h.n_materials)
    UP(spectra, h.n_spectra)
    UP(spectra_data, ex.spec_words)
    UP(textures, h.n_textures)
    for (uint32_t i = 0; i < h.n_emitters; ++i)   // textured area emitters: their texel tables live in texture_data (scene_extents counts them)
        if (h.emitters[i].type == EMIT_AREA && h.emitters[i].radiance_tex > 0) {
            const emitter_t& e = h.emitters[i];
            if ((uint32_t)e.radiance_tex > h.n_textures || h.textures[e.radiance_tex - 1].type != TEX_BITMAP || e.shape < 0 || (uint32_t)e.shape >= h.n_shapes ||
                e.tab_words < h.shapes[e.shape].tri_count * 5ull + 1)
                return fail(WTGPU_ERR_INVALID, "area emitter " + std::to_string(i) + ": radiance_tex must name a bitmap texture and tab / tab_words the emitter's sampling tables (wt/sources.h area_table_*)");
        }
    UP(texture_data, ex.tex_words)
    UP(emitters, h.n_emitters)
    UP(emitter_cdf, h.n_emitters + 1)
    UP(kdists, h.n_emitters)
    UP(kdist_data, ex.kd_words)
    if ((rc = upload(s, h.lut.icdf_theta1, h.lut.m ? h.lut.n_theta : 0, &d.lut.icdf_theta1)) != WTGPU_OK) return rc;
    if ((rc = upload(s, h.lut.icdf_theta2, h.lut.m ? h.lut.n_theta : 0, &d.lut.icdf_theta2)) != WTGPU_OK) return rc;
    if ((rc = upload(s, h.lut.icdf1, (size_t)h.lut.m * h.lut.m, &d.lut.icdf1)) != WTGPU_OK) return rc;
    if ((rc = upload(s, h.lut.icdf2, (size_t)h.lut.m * h.lut.m, &d.lut.icdf2)) != WTGPU_OK) return rc;
#undef UP
    s->dev = d;
    s->d_tri_class = nullptr;
    if (h.n_tris > 0 && h.opts.integrator == INTEGRATOR_BDPT) {   // the material-sorted pass A: class of every triangle (wt/bdpt.h: walk_class_of_triangle)
        std::vector<unsigned char> cls(h.n_tris);
        for (uint32_t t = 0; t < h.n_tris; ++t) cls[t] = (unsigned char)walk_class_of_triangle(h, t);
        if ((rc = upload(s, cls.data(), cls.size(), &s->d_tri_class)) != WTGPU_OK) return rc;
    }
    return WTGPU_OK;
}

// step 3, per slice (it stands before step 2, whose budget estimates what it allocates): the path state of one batch of up to `batch_cap` samples, its stream and its event
static int alloc_slice(wtgpu_scene* s, uint32_t k, uint64_t batch_cap, unsigned long long* counters) {
    const scene_t& h = s->host;
    int rc;
    device_state_t& st = s->slices[k];
    st.cap = batch_cap;
    st.max_verts = (uint32_t)h.opts.max_depth + 2;
    st.walk_words = (uint32_t)(h.opts.integrator != INTEGRATOR_BDPT ? kPathWalkWords : kWalkWords);
    st.vert_words = (size_t)st.max_verts * kVertexWords;
    st.counters = counters;
    const size_t W2 = 2 * (size_t)st.cap;
    const bool path_mode = h.opts.integrator != INTEGRATOR_BDPT;   // plt_path: no vertex store / strategy buckets / Fraunhofer pool
    if ((rc = dmalloc(s, &st.walks, (path_mode ? kPathWalkWords : kWalkWords) * W2))) return rc;
    {
        path_state_t P;
        P.utd_cap = path_mode ? (uint32_t)std::min<uint64_t>(48ull * st.cap + 65536, 1ull << 28) : 1u;   // measured mean on the 576-building etoile: 11 wedges per aperture
        for (int q = 0; q < 2; ++q) {
            if ((rc = dmalloc(s, &P.utd[q], (size_t)P.utd_cap))) return rc;
            if ((rc = dmalloc(s, &P.fsdq[q], path_mode ? (size_t)st.cap : 1))) return rc;
        }
        if ((rc = dmalloc(s, &P.neeq, path_mode ? (size_t)st.cap : 1))) return rc;
        if ((rc = dmalloc(s, &P.fsd_f, path_mode ? (size_t)st.cap : 1))) return rc;
        if ((rc = dmalloc(s, &P.nee_recs, path_mode ? (size_t)st.cap : 1))) return rc;
        if ((rc = dmalloc(s, &P.gather_info, path_mode ? (size_t)st.cap : 1))) return rc;
        path_state_t* dP = nullptr;
        if ((rc = dmalloc(s, &dP, 1))) return rc;
        HIP_CHECK(hipMemcpy(dP, &P, sizeof(P), hipMemcpyHostToDevice));
        s->d_path_slices.push_back(dP);
    }
    if (!path_mode) {
        bdpt_ext_t X;
        X.tri_class = s->d_tri_class;
        if (s->knobs.sorted_interact && (rc = dmalloc(s, &X.cls_queue, (size_t)kNumWalkClasses * W2))) return rc;
        // staged connections: the strategy items of a batch are connected in chunks of pend_cap = `conn_pool` (16; WTGPU_CONN_POOL) x batch size
        // items — a chunk's pending connections cannot outnumber its items; as many chunks as a batch of this scene's depth can hold items for
        // (every (s,t) with s + t - 2 <= max_depth for every sample: 186 per sample at max_depth 16 => 12 chunks, all but the first one or two empty)
        X.pend_cap = (uint32_t)std::min<uint64_t>((uint64_t)s->knobs.conn_pool * st.cap + 4096, 0xFFFFFF00ull);
        if (s->knobs.staged_connect) {
            uint64_t pairs = 0;
            const int md = h.opts.max_depth;
            for (int t = 0; t <= md + 2; ++t)
                for (int q = 0; q <= md + 2; ++q)
                    if (t + q - 2 >= 0 && t + q - 2 <= md && !(t == 1 && q == 1)) ++pairs;
            X.n_chunks = (uint32_t)((pairs * st.cap + X.pend_cap - 1) / X.pend_cap);
            if ((rc = dmalloc(s, &X.pend, (size_t)X.pend_cap))) return rc;
            if ((rc = dmalloc(s, &X.surv, (size_t)X.pend_cap))) return rc;
            if ((rc = dmalloc(s, &X.chunk_ctl, (size_t)X.n_chunks * kChunkCtlWords))) return rc;
        } else
            X.pend_cap = 0;
        s->pend_cap = X.pend_cap;
        s->n_chunks = X.n_chunks;
        bdpt_ext_t* dX = nullptr;
        if ((rc = dmalloc(s, &dX, 1))) return rc;
        HIP_CHECK(hipMemcpy(dX, &X, sizeof(X), hipMemcpyHostToDevice));
        st.ext = dX;
    }
    if ((rc = dmalloc(s, &st.verts, path_mode ? 1 : (size_t)st.max_verts * kVertexWords * W2))) return rc;
    if ((rc = dmalloc(s, &st.ctx, kCtxWords * (size_t)st.cap))) return rc;
    if ((rc = dmalloc(s, &st.trav, (kTravWords + kStageWords) * W2))) return rc;   // (+ the staged trace kernels' records: trace_stage_words)
    if ((rc = dmalloc(s, &st.tris, (size_t)kTriListWords * W2))) return rc;
    if ((rc = dmalloc(s, &st.queue[0], W2))) return rc;
    if ((rc = dmalloc(s, &st.queue[1], W2))) return rc;
    if ((rc = dmalloc(s, &st.heavy_queue, 3 * W2))) return rc;   // (+ the staged trace kernels' two queues: trace_pol_queue / trace_cone_queue)
    if ((rc = dmalloc(s, &st.intb_queue, W2))) return rc;
    if ((rc = dmalloc(s, &st.gather_queue, W2))) return rc;
    if ((rc = dmalloc(s, &st.intc_queue, W2))) return rc;
    if ((rc = dmalloc(s, &st.intd_queue, (path_mode ? 1 : 3) * W2))) return rc;   // (+ pass C's wide and commit queues: pass_c_wide_queue / pass_c_commit_queue)
    st.ftask_cap = path_mode ? 1u : (1u << 22);
    if ((rc = dmalloc(s, &st.ftasks, (size_t)st.ftask_cap))) return rc;
    if ((rc = dmalloc(s, &st.facc, path_mode ? 1 : W2))) return rc;
    st.epool_cap = 1u << 23;
    if ((rc = dmalloc(s, &st.epool, (size_t)st.epool_cap))) return rc;
    if ((rc = dmalloc(s, &st.ctl, (size_t)CTL_WORDS))) return rc;
    HIP_CHECK(hipMemset(st.ctl, 0, CTL_WORDS * sizeof(uint32_t)));
    st.fsd_cap = (h.opts.FSD && !h.opts.force_ray_tracing && !path_mode) ? (uint32_t)std::min<uint64_t>(W2, 1u << 22) : 1u;
    if ((rc = dmalloc(s, &st.fsd_hdr, st.fsd_cap))) return rc;
    // apertures own variable-size ranges of one segment pool: 64 records per sample in flight (measured mean of the headline
    // workload: 1.6 per sample; an aperture holds up to kFsdMaxEdges = 4096)
    st.fsd_ecap = st.fsd_cap > 1 ? (uint32_t)std::min<uint64_t>(64ull * st.cap + kFsdMaxEdges, 1ull << 28) : 1u;
    if ((rc = dmalloc(s, &st.fsd_edges, (size_t)st.fsd_ecap))) return rc;
    if ((rc = dmalloc(s, &st.strat_items, path_mode ? 1 : (size_t)kNumKeys * st.cap))) return rc;
    if ((rc = dmalloc(s, &st.strat_count, (size_t)kNumKeys))) return rc;
    if ((rc = dmalloc(s, &st.strat_prefix, (size_t)kClassTableWords))) return rc;
    if ((rc = dmalloc(s, &st.lacc, 4 * (size_t)st.cap))) return rc;
    HIP_CHECK(hipMemset(st.strat_count, 0, kNumKeys * sizeof(uint32_t)));
    HIP_CHECK(hipStreamCreateWithFlags(&s->streams[k], hipStreamNonBlocking));
    HIP_CHECK(hipEventCreateWithFlags(&s->ev_done[k], hipEventDisableTiming));
    return WTGPU_OK;
}

// step 2: how many slices, and samples per batch.
// per-batch path state: `n_slices` slices (one internal stream each), EACH holding a batch of up to `max_batch` samples.
// Three internal streams: the tails of one batch overlap the bulk of the others.  A single batch already fills the GPU in its first rounds, so
// more streams only add contention — measured with an unthrottled enqueue (16 MiB kernel-argument ring), ms per pass at 1 / 2 / 3 / 4 / 6 / 8
// streams: 158 / 142 / 130 / 142 / 157 / 206 (headline); etoile 66 vs 78, bidir_room 69 vs 82 at 3 vs 4.
// Batches as LARGE as the memory allows: every batch runs its ~30 rounds down to a thin tail, so the cost of the tails is per batch, not
// per sample — measured on the headline workload (2.07 M samples per pass, three streams), samples per batch 0.23 / 0.35 / 0.69 / 1.38 /
// 2.07 M -> 218 / 175 / 130 / 115 / 101 ms per pass.  288 GB of HBM are there to be used: three slices of a whole 1440^2 pass are 93 GB.
// The budget below is an ESTIMATE of what alloc_slice above allocates, not its sum term by term: the four pass queues, heavy_queue, facc, lacc and
// strat_items are covered only by the `+ 2048`.
static uint64_t size_batches(const wtgpu_scene* s, uint64_t max_batch, uint32_t& n_slices) {
    const scene_t& h = s->host;
    const uint64_t npix = (uint64_t)h.sensor.width * h.sensor.height;
    n_slices = s->knobs.streams;   // WTGPU_STREAMS
    uint64_t batch_cap = max_batch ? std::min<uint64_t>(max_batch, 1u << 24) : std::min<uint64_t>(npix, 1u << 22);
    n_slices = (uint32_t)std::min<uint64_t>(n_slices, std::max<uint64_t>(1, batch_cap / 64));
    {   // the vertex stores grow with max_depth (2 x (max_depth + 2) vertices of 356 B per sample): keep the state of all slices within a budget
        // (WTGPU_STATE_GB, default 224 of the 288 GB, and never more than 85 % of what is free) by shrinking the batches of deep scenes — more, smaller batches, same results
        const bool pm = h.opts.integrator != INTEGRATOR_BDPT;
        const uint64_t mv = (uint64_t)h.opts.max_depth + 2;
        uint64_t per_sample = 4ull * (2 * ((pm ? kPathWalkWords : kWalkWords) + (pm ? 0 : mv * kVertexWords) + kTravWords + kStageWords + 2 + kTriListWords) + kCtxWords) + 64ull * 28ull + 2048ull;
        // plt_path: two wedge pools of 48 records per walk, the deferred-NEE records, the queues of the wave-per-walk kernels
        if (pm) per_sample += 2ull * 48ull * sizeof(utd_edge_rec_t) + sizeof(path_nee_rec_t) + 3ull * 4ull + 4ull + sizeof(uint2);
        else per_sample += (s->knobs.staged_connect ? (uint64_t)s->knobs.conn_pool * (sizeof(conn_pending_t) + 4ull) : 0ull) + (s->knobs.sorted_interact ? 4ull * 2ull * kNumWalkClasses : 0ull);   // pending connections, class queues
        uint64_t budget = (uint64_t)s->knobs.state_gb << 30;   // WTGPU_STATE_GB, default 224 of the MI355X's 288 GB (three slices of a two-pass 1440^2 batch are 186 GB)
        // ... and within what the device has free right now (another scene, torch's caching allocator, a smaller GPU): 85 % of it, the rest is
        // for the per-slice pools (edge ids, region-sum tasks, Fraunhofer segments: ~0.3 GB per slice) and the caller's films
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b > 0) budget = std::min<uint64_t>(budget, (uint64_t)((double)free_b * 0.85));
        const uint64_t fixed = (uint64_t)n_slices * ((1ull << 23) * 4ull + (1ull << 22) * 8ull + (64ull << 20));   // pools that do not scale with the batch
        budget = budget > 2 * fixed ? budget - fixed : budget / 2;
        const uint64_t fit = std::max<uint64_t>(4096, budget / per_sample / n_slices);
        if (batch_cap > fit) batch_cap = fit;
    }
    return batch_cap;
}

static int upload_impl(wtgpu_scene* s, uint64_t max_batch) {
    read_knobs(s->knobs);
    int n_cu = 256;
    (void)hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, s->device);
    s->n_cus = (uint32_t)std::max(1, n_cu);
    int rc;
    if ((rc = upload_scene_arrays(s)) != WTGPU_OK) return rc;
    uint32_t n_slices = 0;
    const uint64_t batch_cap = size_batches(s, max_batch, n_slices);
    unsigned long long* counters = nullptr;
    if ((rc = dmalloc(s, &counters, kNumCounters + kProfSlots + 1))) return rc;
    HIP_CHECK(hipMemset(counters, 0, (kNumCounters + kProfSlots + 1) * sizeof(unsigned long long)));
    s->slices.resize(n_slices);
    s->streams.resize(n_slices);
    s->ev_done.resize(n_slices);
    for (uint32_t k = 0; k < n_slices; ++k)
        if ((rc = alloc_slice(s, k, batch_cap, counters)) != WTGPU_OK) return rc;
    HIP_CHECK(hipEventCreateWithFlags(&s->ev_begin, hipEventDisableTiming));
    // in-flight batch records: events for per-kernel timings + pinned snapshot of the control block
    s->recs.resize(4 * (size_t)n_slices);
    s->pending.assign(n_slices, wtgpu_scene::pending_t{});
    for (auto& r : s->recs) {
        r.ev.resize(s->knobs.timing ? 3 + 6 * (size_t)kMaxWalkIters : 1);
        for (auto& e : r.ev) HIP_CHECK(hipEventCreate(&e));
        HIP_CHECK(hipHostMalloc((void**)&r.h_ctl, CTL_WORDS * sizeof(uint32_t), hipHostMallocDefault));
        HIP_CHECK(hipHostMalloc((void**)&r.h_mid, CTL_WORDS * sizeof(uint32_t), hipHostMallocDefault));
        HIP_CHECK(hipEventCreateWithFlags(&r.ev_mid, hipEventDisableTiming));
        HIP_CHECK(hipEventCreateWithFlags(&r.ev_stagger, hipEventDisableTiming));
    }
    s->uploaded = true;
    return WTGPU_OK;
}

void release_device(wtgpu_scene* s) {
    if (s->device < 0) return;
    device_guard_t guard(s->device);
    (void)hipDeviceSynchronize();
    for (void* p : s->dev_allocs) (void)hipFree(p);
    s->dev_allocs.clear();
    for (auto& r : s->recs) {
        for (auto& e : r.ev)
            if (e) (void)hipEventDestroy(e);
        if (r.h_ctl) (void)hipHostFree(r.h_ctl);
        if (r.h_mid) (void)hipHostFree(r.h_mid);
        if (r.ev_mid) (void)hipEventDestroy(r.ev_mid);
        if (r.ev_stagger) (void)hipEventDestroy(r.ev_stagger);
    }
    s->recs.clear();
    s->pending.clear();
    for (auto& e : s->ev_done)
        if (e) (void)hipEventDestroy(e);
    s->ev_done.clear();
    s->ev_stagger_last = nullptr;
    if (s->ev_begin) (void)hipEventDestroy(s->ev_begin);
    s->ev_begin = nullptr;
    for (auto& st_ : s->streams)
        if (st_) (void)hipStreamDestroy(st_);
    s->streams.clear();
    s->slices.clear();
    s->d_path_slices.clear();
    s->d_tri_class = nullptr;
    s->pend_cap = s->n_chunks = 0;
    s->d_mask_flags = nullptr;   // (freed with dev_allocs)
    if (s->h_mask_flags) (void)hipHostFree(s->h_mask_flags);
    s->h_mask_flags = nullptr;
    if (s->ev_mask) (void)hipEventDestroy(s->ev_mask);
    s->ev_mask = nullptr;
    s->d_tm_table = nullptr;     // (freed with dev_allocs)
    if (s->h_tm_table) (void)hipHostFree(s->h_tm_table);
    s->h_tm_table = nullptr;
    if (s->ev_tm) (void)hipEventDestroy(s->ev_tm);
    s->ev_tm = nullptr;
    film_scratch_free(s->fs);
    film_scratch_free(s->fc);
    film_scratch_free(s->fp);
    s->d_denoise = nullptr;      // (freed with dev_allocs)
    if (s->d_zonal) (void)hipFree(s->d_zonal);   // (its own allocation: it grows with the calls)
    if (s->h_zonal) (void)hipHostFree(s->h_zonal);
    s->d_zonal = s->h_zonal = nullptr;
    s->d_zonal_bytes = s->h_zonal_bytes = 0;
    s->zonal_last_lds = 0xFFFFFFFFu;
    if (s->d_segments) (void)hipFree(s->d_segments);
    if (s->h_segments) (void)hipHostFree(s->h_segments);
    s->d_segments = s->h_segments = nullptr;
    s->d_segments_bytes = s->h_segments_bytes = 0;
    s->segments_last_overflow = s->segments_last_tiled = 0xFFFFFFFFu;
    if (s->d_distance) (void)hipFree(s->d_distance);
    if (s->h_distance) (void)hipHostFree(s->h_distance);
    s->d_distance = s->h_distance = nullptr;
    s->d_distance_bytes = 0;
    s->distance_last_groups = 0xFFFFFFFFu;
    s->uploaded = false;
}

extern "C" {

int wtgpu_scene_upload(wtgpu_scene* s, int device, uint64_t max_batch) {
    if (!s) return fail(WTGPU_ERR_INVALID, "null scene");
    if (s->uploaded) return fail(WTGPU_ERR_INVALID, "scene already uploaded");
    {
        std::string why;
        if (!runtime_settings_ok(why)) return fail(WTGPU_ERR_INVALID, why);
    }
    int ndev = 0;
    const hipError_t dc = hipGetDeviceCount(&ndev);
    if (dc != hipSuccess || ndev == 0)
        return fail(WTGPU_ERR_NO_DEVICE, std::string("no HIP device present (there is no CPU fallback): hipGetDeviceCount -> ") + hipGetErrorString(dc) +
                                             ", count " + std::to_string(ndev));
    if (device < 0 || device >= ndev) return fail(WTGPU_ERR_NO_DEVICE, "invalid device index");
    device_guard_t guard(device);
    s->device = device;
    const int rc_up = upload_impl(s, max_batch);
    if (rc_up != WTGPU_OK) release_device(s);   // nothing half-uploaded stays behind: a retry starts from scratch
    return rc_up;
}

}   // extern "C"
