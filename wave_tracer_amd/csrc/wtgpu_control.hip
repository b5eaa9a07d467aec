// wave_tracer_amd — the render-seam control surface (cancel / pause / resume / capture, the progressive render) and the multi-GPU film reduction.
#include "wtgpu_host.h"
#include <rccl/rccl.h>

struct wtgpu_comm {
    ncclComm_t comm = nullptr;
    int device = -1, world = 0, rank = 0;
};

extern "C" {

// ---- render-seam control surface --------------------------------------------------------------------------------------------
int wtgpu_cancel(wtgpu_scene* s) {
    if (!s) return fail(WTGPU_ERR_INVALID, "null scene");
    s->cancel.store(1, std::memory_order_relaxed);
    s->paused.store(0, std::memory_order_relaxed);   // cancel is a full reset: a pause that was in force does not hold up the NEXT render (pause itself is sticky)
    return WTGPU_OK;
}
int wtgpu_pause(wtgpu_scene* s) {
    if (!s) return fail(WTGPU_ERR_INVALID, "null scene");
    s->paused.store(1, std::memory_order_relaxed);
    return WTGPU_OK;
}
int wtgpu_resume(wtgpu_scene* s) {
    if (!s) return fail(WTGPU_ERR_INVALID, "null scene");
    s->paused.store(0, std::memory_order_relaxed);
    return WTGPU_OK;
}
int wtgpu_capture_intermediate(wtgpu_scene* s, wtgpu_capture_cb capture, void* user) {
    if (!s || !capture) return fail(WTGPU_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> l(s->capture_mutex);
    s->capture_cb = capture;
    s->capture_user = user;
    return WTGPU_OK;
}
int wtgpu_render_progressive(wtgpu_scene* s, void* stream_, double* d_value, double* d_weight, double* d_light, uint64_t sb, uint64_t se, uint64_t seed,
                             uint32_t chunk_spp, wtgpu_progress_cb progress, void* user, uint64_t* spe_done) {
    if (!s || !s->uploaded) return fail(WTGPU_ERR_INVALID, "scene not uploaded");
    if (se < sb) return fail(WTGPU_ERR_INVALID, "bad sample range");
    if (spe_done) *spe_done = 0;
    s->cancel.store(0, std::memory_order_relaxed);
    const uint64_t step = chunk_spp ? chunk_spp : 1;
    const uint64_t npix = (uint64_t)s->host.sensor.width * s->host.sensor.height;
    device_guard_t guard(s->device);
    // a pending `capture intermediate` at a chunk boundary: the stream is idle, the films hold the completed chunks
    auto serve_capture = [&](uint64_t done) {
        wtgpu_capture_cb cb = nullptr;
        void* cu = nullptr;
        {
            std::lock_guard<std::mutex> l(s->capture_mutex);
            cb = s->capture_cb;
            cu = s->capture_user;
            s->capture_cb = nullptr;
        }
        if (cb) cb(done, cu);
    };
    for (uint64_t b = sb; b < se; b += step) {
        const uint64_t e = std::min(se, b + step);
        const int rc = wtgpu_render(s, stream_, d_value, d_weight, d_light, b, e, seed);
        if (rc) return rc;
        HIP_CHECK(hipStreamSynchronize(static_cast<hipStream_t>(stream_)));
        if (spe_done) *spe_done = e - sb;
        const bool stop = progress && progress((e - sb) * npix, (se - sb) * npix, user) != 0;
        serve_capture(e - sb);
        // paused: nothing is launched until wtgpu_resume (or a cancel); captures are still served (the reference's capture needs the paused state)
        while (s->paused.load(std::memory_order_relaxed) && !s->cancel.load(std::memory_order_relaxed) && !stop && e < se) {
            std::this_thread::sleep_for(std::chrono::milliseconds(1));
            serve_capture(e - sb);
        }
        if ((stop || s->cancel.load(std::memory_order_relaxed)) && e < se) return fail(WTGPU_CANCELLED, "render cancelled");
    }
    return WTGPU_OK;
}

// ---- multi-GPU film reduction (RCCL) ----------------------------------------------------------------------------------------
#define NCCL_CHECK(x)                                                                                             \
    do {                                                                                                         \
        ncclResult_t r_ = (x);                                                                                   \
        if (r_ != ncclSuccess) return fail(WTGPU_ERR_COMM, std::string(#x) + ": " + ncclGetErrorString(r_));      \
    } while (0)
static_assert(sizeof(ncclUniqueId) == WTGPU_COMM_ID_BYTES, "ncclUniqueId size");
int wtgpu_comm_unique_id(void* id_out) {
    if (!id_out) return fail(WTGPU_ERR_INVALID, "null argument");
    ncclUniqueId id;
    NCCL_CHECK(ncclGetUniqueId(&id));
    std::memcpy(id_out, &id, sizeof(id));
    return WTGPU_OK;
}
int wtgpu_comm_create(int world, int rank, int device, const void* id_, wtgpu_comm** out) {
    if (!id_ || !out || world < 1 || rank < 0 || rank >= world) return fail(WTGPU_ERR_INVALID, "bad communicator arguments");
    device_guard_t guard(device);
    auto c = std::make_unique<wtgpu_comm>();
    c->device = device;
    c->world = world;
    c->rank = rank;
    ncclUniqueId id;
    std::memcpy(&id, id_, sizeof(id));
    NCCL_CHECK(ncclCommInitRank(&c->comm, world, id, rank));
    *out = c.release();
    return WTGPU_OK;
}
int wtgpu_film_reduce(wtgpu_comm* c, void* stream_, double* d_value, double* d_weight, double* d_light, uint64_t n_value, uint64_t n_weight, int root) {
    if (!c || !c->comm || !d_value || !d_weight || !d_light || root < 0 || root >= c->world) return fail(WTGPU_ERR_INVALID, "bad reduce arguments");
    device_guard_t guard(c->device);
    hipStream_t st = static_cast<hipStream_t>(stream_);
    // one group: the three planes travel together (cornell 1440^2: 116 MB per rank, ~1.5 ms on a ring over xGMI)
    NCCL_CHECK(ncclGroupStart());
    NCCL_CHECK(ncclReduce(d_value, d_value, (size_t)n_value, ncclDouble, ncclSum, root, c->comm, st));
    NCCL_CHECK(ncclReduce(d_weight, d_weight, (size_t)n_weight, ncclDouble, ncclSum, root, c->comm, st));
    NCCL_CHECK(ncclReduce(d_light, d_light, (size_t)n_value, ncclDouble, ncclSum, root, c->comm, st));
    NCCL_CHECK(ncclGroupEnd());
    return WTGPU_OK;
}
void wtgpu_comm_destroy(wtgpu_comm* c) {
    if (!c) return;
    if (c->comm) {
        device_guard_t guard(c->device);
        (void)ncclCommDestroy(c->comm);
    }
    delete c;
}

}   // extern "C"
