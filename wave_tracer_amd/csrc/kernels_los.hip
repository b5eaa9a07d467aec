// wave_tracer_amd — line-of-sight maps (wtgpu_line_of_sight / wtgpu_line_of_sight_host; see wtgpu_kernels.h for the list of kernel translation
// units): per sensor element (or caller's point) and selected emitter the share of the element's samples that see the emitter and the means of
// distance, direction and cosine; per element the mean point, how many emitters it sees and the nearest of them.  The arithmetic is wt/los.h's,
// which the host twin below runs too: device and host agree bit for bit.  Stacks as kernels_mask.hip's; the per-sample lane shape, its exchange and
// the host twin's loop are kernels_maps.h's.  No render kernel is compiled here.
#include "kernels_maps.h"
#include "wt/los.h"

namespace wtk {

// One lane per (element, emitter) (the element's centre, more than 64 samples, caller points, WTGPU_LOS_PER_SAMPLE=0): a block holds kBlock / E
// elements, lanes [g * E, (g + 1) * E) the emitters of its g-th — they start from the same points, so their rays begin in the same nodes.  The
// lane traces its pair's samples one after the other, keeps the sums in registers and writes its K floats contiguously.  When every lane of the
// block has finished, the LDS of the stacks is free: each lane leaves what its pair adds to the element there, and the element's first lane
// takes the emitters in order (los_nearest_step).  Every lane reaches the barriers.  vectors: a direction or cosine map is asked for.
template <bool vectors>
__global__ void __launch_bounds__(kBlock) k_los_pair(scene_t sc, los_query_t q, float* out_maps, float* out_elem, uint32_t* out_ids) {
    __shared__ stack_entry_t lds[kLdsStack * kBlock];
    const uint32_t W = sc.sensor.width, E = q.n_emitters;
    const uint64_t npix = (uint64_t)W * sc.sensor.height;
    const uint32_t per_block = kBlock / E, g = threadIdx.x / E, k = threadIdx.x - g * E;
    const uint64_t p = (uint64_t)blockIdx.x * per_block + g;
    const bool active = g < per_block && p < npix;
    const uint32_t px = active ? (uint32_t)(p % W) : 0u, py = active ? (uint32_t)(p / W) : 0u;
    los_sums_t a;
    a.n_visible = 0;
    a.v[1] = 0.f;
    if (active) {
        stack_entry_t spill[kSpillStack];
        stack_ref_t stack;
        lds_stack(lds, spill, stack);
        a = los_pair<vectors>(sc, q, px, py, los_target(sc.emitters[q.emitters[k]]), stack);
        if (q.maps) los_write_pair(a, q.samples, q.maps, out_maps + (p * E + k) * los_map_floats(q.maps));
    }
    if (!(q.elem | q.ids)) return;   // (the same for every lane)
    __syncthreads();   // no lane of the block reads its stack any more
    float* ex = reinterpret_cast<float*>(lds);
    uint32_t* exu = reinterpret_cast<uint32_t*>(lds);
    exu[threadIdx.x] = a.n_visible;
    ex[kBlock + threadIdx.x] = los_mean(a.v[1], q.samples);
    __syncthreads();
    if (!active || k != 0) return;
    los_nearest_t near = los_nearest_none();
    for (uint32_t j = 0; j < E; ++j) los_nearest_step(near, j, exu[threadIdx.x + j], ex[kBlock + threadIdx.x + j]);
    const vec3 ps = q.elem & LOS_POINT ? los_point_sum(sc, q, px, py) : vec3{0.f, 0.f, 0.f};
    los_write_element(near, ps, q.samples, q.elem, q.ids, out_elem + p * los_elem_floats(q.elem), out_ids + p * los_id_words(q.ids));
}

// One lane per (element, sample) (the sensor's own elements, 1 <= samples <= 64).  A lane forms its point once and walks the selected emitters —
// the emitter is the same for the whole wavefront: its record is kept in scalar registers, and the rays end in one place.  Per emitter: the count
// of the visible samples is the popcount of the group's bits in one ballot; each lane leaves its sample's floats in the exchange and lane j of an
// element's group adds float j of ALL the group's samples (the means are over all samples, the zeros of the hidden ones included) and
// stores the mean: neighbouring lanes store neighbouring floats.  The group's first lane also takes the emitter into the element's count and
// nearest (los_nearest_step), and sums the points where the mean point is asked for.  Every lane reaches the ballots and the barriers.
WT_D float wave_uniform(float x) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x))); }
template <bool vectors>
__global__ void __launch_bounds__(kBlock) k_los_sample(scene_t sc, los_query_t q, float* out_maps, float* out_elem, uint32_t* out_ids) {
    __shared__ stack_entry_t lds[kLdsStack * kBlock];
    exchange_fits<kLosFloats>();
    const uint32_t W = sc.sensor.width, E = q.n_emitters, samples = q.samples;
    const sample_lane_t l = sample_lane(samples, (uint64_t)W * sc.sensor.height);
    float* ex = reinterpret_cast<float*>(lds);
    stack_entry_t spill[kSpillStack];
    stack_ref_t stack;
    lds_stack(lds, spill, stack);
    los_point_t pt;
    pt.p = pt.n = vec3{0.f, 0.f, 0.f};
    pt.ok = false;
    if (l.active) pt = los_point(sc, q, (uint32_t)(l.p % W), (uint32_t)(l.p / W), l.s);
    vec3 ps{0.f, 0.f, 0.f};
    if (q.elem & LOS_POINT) {   // (the same for every lane)
        ex[exchange_at(0, threadIdx.x)] = pt.p.x, ex[exchange_at(1, threadIdx.x)] = pt.p.y, ex[exchange_at(2, threadIdx.x)] = pt.p.z;
        __syncthreads();
        if (l.active && l.s == 0)   // (group_sum's sum of the three rows in one pass: row after row the full query took 0.96 ms in place of 0.93)
            for (uint32_t t = 0; t < samples; ++t)
                ps = vec3{seq_add(t == 0, ps.x, ex[exchange_at(0, l.first + t)]), seq_add(t == 0, ps.y, ex[exchange_at(1, l.first + t)]),
                          seq_add(t == 0, ps.z, ex[exchange_at(2, l.first + t)])};
        __syncthreads();
    }
    const uint32_t K = los_map_floats(q.maps);
    const bool need_nearest = (q.ids | (q.elem & LOS_NEAREST_DISTANCE)) != 0;
    los_nearest_t near = los_nearest_none();
    for (uint32_t k = 0; k < E; ++k) {
        los_sample_t r;
#pragma unroll
        for (uint32_t j = 0; j < kLosFloats; ++j) r.v[j] = 0.f;
        r.visible = false;
        // the same record for every lane: the first lane's words, which the compiler then keeps in scalar registers (168 -> 154 VGPRs with all maps)
        const los_target_t lane_e = los_target(sc.emitters[q.emitters[k]]);
        const los_target_t e{__builtin_amdgcn_readfirstlane(lane_e.type),
                             vec3{wave_uniform(lane_e.position.x), wave_uniform(lane_e.position.y), wave_uniform(lane_e.position.z)},
                             vec3{wave_uniform(lane_e.n.x), wave_uniform(lane_e.n.y), wave_uniform(lane_e.n.z)}};
        if (pt.ok) r = los_sample(sc, q, pt, e, stack);
        const unsigned long long bits = __ballot(r.visible);
        __syncthreads();   // no lane of the block reads its stack any more
        ex[exchange_at(1, threadIdx.x)] = r.v[1];
        if (vectors) {
#pragma unroll
            for (uint32_t j = 2; j < kLosFloats; ++j) ex[exchange_at(j, threadIdx.x)] = r.v[j];
        }
        __syncthreads();
        if (l.active) {
            const uint32_t n_visible = (uint32_t)__popcll(group_bits(bits, l, samples));
            float* m = out_maps + (l.p * E + k) * K;
            for (uint32_t j = l.s; j < kLosFloats; j += samples) {
                const int slot = los_slot(q.maps, j);
                if (slot >= 0) m[slot] = j == 0 ? los_visible(n_visible, samples) : los_mean(group_sum(ex, j, l, samples), samples);
            }
            if (l.s == 0 && need_nearest) los_nearest_step(near, k, n_visible, los_mean(group_sum(ex, 1, l, samples), samples));
        }
        __syncthreads();   // the sums are read: the stacks may be used again
    }
    if (l.active && l.s == 0 && (q.elem | q.ids))
        los_write_element(near, ps, samples, q.elem, q.ids, out_elem + l.p * los_elem_floats(q.elem), out_ids + l.p * los_id_words(q.ids));
}

// per_sample (WTGPU_LOS_PER_SAMPLE): one lane per sample wherever the sensor's own elements are sampled and an element's samples fit one
// wavefront — on the MI355X the bundled etoile (720 x 540, one emitter, 32 samples, every map) takes 0.93 ms against 2.86 ms with one lane per
// pair (median of 15 calls each, alternated: tools/bench_los.py) —; else — the centre, more than 64 samples, caller points — one lane per
// (element, emitter)
template <bool vectors>
static void los_launch_as(const scene_t& sc, hipStream_t stream, const los_query_t& q, uint32_t per_sample, float* d_maps, float* d_elem, uint32_t* d_ids) {
    const uint64_t npix = (uint64_t)sc.sensor.width * sc.sensor.height;
    if (per_sample && !q.points && q.samples >= 1u && q.samples <= 64u)
        hipLaunchKernelGGL(k_los_sample<vectors>, dim3(sample_blocks(npix, q.samples)), dim3(kBlock), 0, stream, sc, q, d_maps, d_elem, d_ids);
    else {
        const uint64_t per_block = kBlock / q.n_emitters;
        hipLaunchKernelGGL(k_los_pair<vectors>, dim3((uint32_t)((npix + per_block - 1) / per_block)), dim3(kBlock), 0, stream, sc, q, d_maps, d_elem, d_ids);
    }
}
int los_launch(const scene_t& sc, hipStream_t stream, const los_query_t& q, uint32_t per_sample, float* d_maps, float* d_elem, uint32_t* d_ids) {
    if ((uint64_t)sc.sensor.width * sc.sensor.height == 0 || q.n_emitters == 0 || q.n_emitters > kLosMaxEmitters) return 0;
    if (q.maps & kLosVectorMaps)
        los_launch_as<true>(sc, stream, q, per_sample, d_maps, d_elem, d_ids);
    else
        los_launch_as<false>(sc, stream, q, per_sample, d_maps, d_elem, d_ids);
    return (int)hipGetLastError();
}

// The same on host threads (kernels_maps.h: on_elements).
void los_host(const scene_t& sc, const los_query_t& q, uint32_t n_threads, float* out_maps, float* out_elem, uint32_t* out_ids) {
    const uint32_t E = q.n_emitters;
    const size_t K = los_map_floats(q.maps), Ke = los_elem_floats(q.elem), Ki = los_id_words(q.ids);
    const bool vectors = (q.maps & kLosVectorMaps) != 0;
    on_elements(sc, n_threads, [&](uint32_t x, uint32_t y, size_t p, const stack_ref_t& stack) {
        los_nearest_t near = los_nearest_none();
        for (uint32_t k = 0; k < E; ++k) {
            const los_target_t e = los_target(sc.emitters[q.emitters[k]]);
            const los_sums_t a = vectors ? los_pair<true>(sc, q, x, y, e, stack) : los_pair<false>(sc, q, x, y, e, stack);
            if (q.maps) los_write_pair(a, q.samples, q.maps, out_maps + (p * E + k) * K);
            los_nearest_step(near, k, a.n_visible, los_mean(a.v[1], q.samples));
        }
        if (!(q.elem | q.ids)) return;
        const vec3 ps = q.elem & LOS_POINT ? los_point_sum(sc, q, x, y) : vec3{0.f, 0.f, 0.f};
        los_write_element(near, ps, q.samples, q.elem, q.ids, out_elem + p * Ke, out_ids + p * Ki);
    });
}

}   // namespace wtk
