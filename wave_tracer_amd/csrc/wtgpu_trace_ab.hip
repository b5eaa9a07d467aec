// wave_tracer_amd — the per-lane traversal of a round in its alternative forms, and the harness that replays a round through both.
#include "wtgpu_host.h"

// ---- WTGPU_TRACE_AB: in-situ replay of a round's trace queue through both per-lane trace kernels (the "replay harness": each variant sees exactly the
// queue, walk records and scene the pipeline produced, so what is timed is the real mix of beam widths and what is compared is every word they write)
extern "C" {
__global__ void __launch_bounds__(256) k_ab_compare(const uint32_t* x, const uint32_t* y, size_t n, unsigned long long* out) {
    unsigned long long bad = 0;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) bad += x[i] != y[i] ? 1u : 0u;
    for (int off = 32; off > 0; off >>= 1) bad += __shfl_down(bad, off, 64);
    if ((threadIdx.x & 63) == 0 && bad) atomicAdd(out, bad);
}
__global__ void __launch_bounds__(256) k_ab_queue_sums(const uint32_t* q, const uint32_t* count, unsigned long long* out) {   // order-independent checksums of a queue
    unsigned long long s1 = 0, s2 = 0;
    const uint32_t n = *count;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        s1 += q[i];
        s2 += (unsigned long long)q[i] * 2654435761ull + ((unsigned long long)q[i] << 7 ^ q[i]);
    }
    for (int off = 32; off > 0; off >>= 1) {
        s1 += __shfl_down(s1, off, 64);
        s2 += __shfl_down(s2, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(out, s1);
        atomicAdd(out + 1, s2);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(out + 2, (unsigned long long)n);
}
int wtgpu_trace_ab_stats(wtgpu_scene* s, double* ms_refill, double* ms_sm, uint64_t* differing_words, uint64_t* walks, uint64_t* rounds) {
    if (!s) return fail(WTGPU_ERR_INVALID, "null scene");
    if (ms_refill) *ms_refill = s->ab_ms[0];
    if (ms_sm) *ms_sm = s->ab_ms[1];
    if (differing_words) *differing_words = s->ab_mismatch;
    if (walks) *walks = s->ab_walks;
    if (rounds) *rounds = s->ab_rounds;
    return WTGPU_OK;
}
}   // extern "C"
// the per-lane traversal of a round in its alternative forms (the default, k_trace_refill, is launched by batch_launcher_t::rounds itself)
void launch_trace_alt(const wtgpu_scene* s, const launch_args_t& a, hipStream_t st_, int in, int first, uint32_t round, uint32_t g0) {
    const wtgpu_scene::knobs_t& K = s->knobs;
    if (K.trace_staged) {
        hipLaunchKernelGGL(k_tr_axis, dim3(g0), dim3(kBlock), 0, st_, a, in, first, round);
        for (uint32_t it = 0; it < K.trace_stages; ++it) {
            const uint32_t g = std::max<uint32_t>(1u, g0 >> std::min(it, 4u));   // (the queues shrink from stage to stage; a grid that is too small only loops longer)
            if (it > 0) hipLaunchKernelGGL(k_tr_policy, dim3(g), dim3(kBlock), 0, st_, a, it);
            hipLaunchKernelGGL(k_tr_cone, dim3(g), dim3(kBlock), 0, st_, a, it);
        }
        hipLaunchKernelGGL(k_tr_tail, dim3(std::max<uint32_t>(1u, g0 >> 3)), dim3(kBlock), 0, st_, a, K.trace_stages);
    } else
        hipLaunchKernelGGL(k_trace_sm, dim3(g0), dim3(kBlock), 0, st_, a, in, first, round);
}
int trace_ab_round(wtgpu_scene* s, const launch_args_t& a, hipStream_t st_, int in, int first, uint32_t round, uint32_t g0) {
    const size_t n_trav = 2 * (size_t)a.st.cap * kTravWords, n_tris = 2 * (size_t)a.st.cap * kTriListWords;
    uint32_t *b_trav = nullptr, *b_tris = nullptr;
    unsigned long long* d_out = nullptr;
    uint32_t h_n[2] = {0, 0};
    HIP_CHECK(hipMalloc(&b_trav, n_trav * 4));
    HIP_CHECK(hipMalloc(&b_tris, n_tris * 4));
    HIP_CHECK(hipMalloc(&d_out, 8 * sizeof(unsigned long long)));
    HIP_CHECK(hipMemsetAsync(d_out, 0, 8 * sizeof(unsigned long long), st_));
    hipEvent_t ev[4];
    for (auto& e : ev) HIP_CHECK(hipEventCreate(&e));
    HIP_CHECK(hipMemcpyAsync(h_n, a.st.ctl + CTL_COUNT0 + in, 4, hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipMemcpyAsync(h_n + 1, a.st.ctl + CTL_BACK0 + in, 4, hipMemcpyDeviceToHost, st_));
    // A: k_trace_refill
    HIP_CHECK(hipEventRecord(ev[0], st_));
    hipLaunchKernelGGL(k_trace_refill, dim3(g0), dim3(kBlock), 0, st_, a, in, first, round);
    HIP_CHECK(hipEventRecord(ev[1], st_));
    HIP_CHECK(hipMemcpyAsync(b_trav, a.st.trav, n_trav * 4, hipMemcpyDeviceToDevice, st_));
    HIP_CHECK(hipMemcpyAsync(b_tris, a.st.tris, n_tris * 4, hipMemcpyDeviceToDevice, st_));
    hipLaunchKernelGGL(k_ab_queue_sums, dim3(64), dim3(256), 0, st_, a.st.heavy_queue, a.st.ctl + CTL_HEAVY_COUNT, d_out + 1);
    // the queue again from its start, an empty heavy queue
    HIP_CHECK(hipMemsetAsync(a.st.ctl + CTL_HEAD_TRACE, 0, 4, st_));
    HIP_CHECK(hipMemsetAsync(a.st.ctl + CTL_HEAVY_COUNT, 0, 4, st_));
    // B: the alternative form the knobs select (k_trace_sm, or the staged kernels)
    HIP_CHECK(hipEventRecord(ev[2], st_));
    launch_trace_alt(s, a, st_, in, first, round, g0);
    HIP_CHECK(hipEventRecord(ev[3], st_));
    hipLaunchKernelGGL(k_ab_compare, dim3(2048), dim3(256), 0, st_, b_trav, a.st.trav, n_trav, d_out);
    hipLaunchKernelGGL(k_ab_compare, dim3(2048), dim3(256), 0, st_, b_tris, a.st.tris, n_tris, d_out);
    hipLaunchKernelGGL(k_ab_queue_sums, dim3(64), dim3(256), 0, st_, a.st.heavy_queue, a.st.ctl + CTL_HEAVY_COUNT, d_out + 4);
    unsigned long long h_out[8];
    HIP_CHECK(hipMemcpyAsync(h_out, d_out, sizeof(h_out), hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipStreamSynchronize(st_));
    float ms_a = 0.f, ms_b = 0.f;
    (void)hipEventElapsedTime(&ms_a, ev[0], ev[1]);
    (void)hipEventElapsedTime(&ms_b, ev[2], ev[3]);
    const uint64_t bad = h_out[0] + (h_out[1] != h_out[4]) + (h_out[2] != h_out[5]) + (h_out[3] != h_out[6]);
    s->ab_ms[0] += ms_a;
    s->ab_ms[1] += ms_b;
    s->ab_mismatch += bad;
    s->ab_walks += (uint64_t)h_n[0] + h_n[1];
    s->ab_rounds++;
    if (s->knobs.trace_ab_verbose)
        fprintf(stderr, "[trace ab] round %2u: %8u walks  refill %8.3f ms  alt %8.3f ms  heavy %llu / %llu  differing words %llu\n", round, h_n[0] + h_n[1], ms_a, ms_b,
                h_out[3], h_out[6], (unsigned long long)bad);
    for (auto& e : ev) (void)hipEventDestroy(e);
    (void)hipFree(b_trav);
    (void)hipFree(b_tris);
    (void)hipFree(d_out);
    return WTGPU_OK;
}
