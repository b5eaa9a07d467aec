// wave_tracer_amd — subpath connections of plt_bdpt: class / strategy buckets, connections + MIS, film splat (see wtgpu_kernels.h for the list of kernel translation units).
#include "wtgpu_kernels.h"

namespace wtk {

// ---- connections ------------------------------------------------------------------------------------------------------------------
// plt_bdpt.cpp:105-146 loops over all (s,t) pairs of a sample.  One thread per sample, samples taken as they come, would leave a wavefront
// executing the UNION of its 64 samples' pairs (~80 iterations with ~10 lanes' worth of work: subpath lengths are geometric).  What a wavefront
// needs is 64 lanes that run the same (s,t) in every iteration.  Two forms give it that (WTGPU_CONNECT_CLASS):
// class-major (k_connect_class, 1) — two samples whose subpaths have the same lengths (nT, nS) have the same valid strategies (strategy_valid
// reads nothing else), so the work item is a SAMPLE and the buckets are the length classes:
//   k_connect_enum  : every sample appends its index ONCE, to the bucket (min(nT, K), min(nS, K)) (block-aggregated: LDS counts, one global
//                     atomic per bucket and block),
//   k_connect_scan  : prefix sum over the 19x19 bucket sizes in the order of descending nT x nS (class_key_rank), every class padded to whole
//                     wavefronts,
//   k_connect_class : persistent; a wavefront grabs 64 items of the flattened space = 64 samples of ONE class and runs the class's strategies
//                     in a row, t outer, s inner: the class, the loop counters and the validity test are wave-uniform; context, vertex stores
//                     and pool are set up once per sample; all of a sample's vertices are fetched by one wavefront within one item, vertex
//                     t-1 by consecutive iterations; the t>1 fluxes are summed in the lane (f64, fixed order) and written once; t<=1
//                     strategies splat into the light image directly.  k_connect_class_open: the classes of the last row / column,
//   k_connect_splat : one film splat per sample with the summed flux (film.hpp:214-342).
// strategy-major (k_connect_strat, 0; the A/B reference, and what the staged form below enumerates) — the work item is one strategy of a sample:
//   k_connect_enum  : every sample appends its index to one bucket per valid (s,t) pair,
//   k_connect_scan  : prefix sum over the bucket sizes,
//   k_connect_strat : persistent; 64 consecutive items of the flattened bucket space = 64 samples with the SAME (s,t); the t>1 fluxes are
//                     summed per sample with f64 atomics.  A sample's ~3.5 vertices are fetched again by each of its ~10 strategies, each in
//                     another wavefront at another time.
WT_D bool strategy_valid(const integrator_opts_t& o, int s, int t, int nS, int nT) {
    const int depth = t + s - 2;
    if (t > nT || s > nS) return false;
    if ((t == 1 && s == 1) || depth < 0 || depth > o.max_depth) return false;
    if (!o.emitter_direct && s == 1) return false;
    if (!o.sensor_direct && t == 1) return false;
    if (o.debug_only_s && (int)o.debug_only_s - 1 != s) return false;
    if (o.debug_only_t && (int)o.debug_only_t - 1 != t) return false;
    return true;
}
// bucket (sk, tk): does it hold a valid strategy of a sample with nS / nT vertices?  (the last row / column stands for every s / t >= kKeyDim-1)
WT_D bool strategy_class_valid(const integrator_opts_t& o, int sk, int tk, int nS, int nT) {
    const int K = (int)kKeyDim - 1;
    const int t1 = tk < K ? tk : nT, s1 = sk < K ? sk : nS;
    for (int t = tk; t <= t1; ++t)
        for (int s = sk; s <= s1; ++s)
            if (strategy_valid(o, s, t, nS, nT)) return true;
    return false;
}
WT_D int wave_max_i(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
    return v;
}

// Block-aggregated bucket append: 1024 samples per block count their valid (s,t) pairs per bucket in LDS, reserve one range per
// bucket with ONE global atomic each, and fill it.  (Wave-aggregated global atomics on the ~30 hot bucket counters serialised in
// L2: PMC SQ_WAIT_ANY 99 % of this kernel's wave cycles, 9.5 ms per pass.)
__global__ void __launch_bounds__(kEnumBlock) k_connect_enum(launch_args_t a, uint32_t by_class) {
    __shared__ uint32_t s_cnt[kNumKeys], s_base[kNumKeys];
    const uint32_t i = blockIdx.x * kEnumBlock + threadIdx.x;
    for (uint32_t k = threadIdx.x; k < kNumKeys; k += kEnumBlock) s_cnt[k] = 0;
    int nT = -1, nS = -1;
    if (i < a.nb) {
        nT = (int)a.st.walks[(size_t)(i) * a.st.walk_words + WT_WALK_NVERTS_WORD];
        nS = (int)a.st.walks[(size_t)(a.st.cap + i) * a.st.walk_words + WT_WALK_NVERTS_WORD];
        if (!by_class) {   // (k_connect_class writes every sample's sum)
#pragma unroll
            for (int c = 0; c < 4; ++c) a.st.lacc[(size_t)c * a.st.cap + i] = 0.0;
        }
    }
    __syncthreads();
    const int K = (int)kKeyDim - 1;
    const int kT = nT < K ? nT : K, kS = nS < K ? nS : K;
    // the keys of this sample.  Class form: its length class, ONE key — EVERY sample of the batch is appended (one without a valid strategy runs
    // none and gets its zero sum).  Strategy form: the buckets that hold a valid strategy of it.  (A thread behind the batch has none: kT = kS = -1.)
    auto each_key = [&](auto&& f) __attribute__((always_inline)) {
        if (by_class) {
            if (i < a.nb) f((uint32_t)max(kT, 0) * kKeyDim + (uint32_t)max(kS, 0));
            return;
        }
        for (int tk = 0; tk <= kT; ++tk)
            for (int sk = 0; sk <= kS; ++sk)
                if (strategy_class_valid(a.sc.opts, sk, tk, nS, nT)) f((uint32_t)tk * kKeyDim + (uint32_t)sk);
    };
    each_key([&](uint32_t key) { atomicAdd(&s_cnt[key], 1u); });
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < kNumKeys; k += kEnumBlock) {
        const uint32_t c = s_cnt[k];
        s_base[k] = c ? atomicAdd(a.st.strat_count + k, c) : 0u;
        s_cnt[k] = 0;
    }
    __syncthreads();
    each_key([&](uint32_t key) { a.st.strat_items[(size_t)key * a.st.cap + s_base[key] + atomicAdd(&s_cnt[key], 1u)] = i; });
}
__global__ void __launch_bounds__(64) k_connect_scan(launch_args_t a, uint32_t by_class) {
    __shared__ uint32_t s_key[kNumKeys];   // class form: the key of every rank
    if (a.st.ext)   // the counters of the staged connections' chunks
        for (uint32_t q = threadIdx.x; q < a.st.ext->n_chunks * kChunkCtlWords; q += 64) a.st.ext->chunk_ctl[q] = 0;
    if (by_class)
        for (uint32_t k = threadIdx.x; k < kNumKeys; k += 64) s_key[class_key_rank(k)] = k;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t acc = 0;
        for (uint32_t r = 0; r < kNumKeys; ++r) {
            const uint32_t k = by_class ? s_key[r] : r;
            const uint32_t c = a.st.strat_count[k];
            a.st.strat_prefix[r] = acc;
            if (by_class) {
                a.st.strat_prefix[kClassCount + r] = c;
                a.st.strat_prefix[kClassKey + r] = k;
                acc += (c + 63u) & ~63u;   // (at most 63 x kNumKeys idle lanes per batch)
            } else
                acc += c;
            a.st.strat_count[k] = 0;   // ready for the next batch
        }
        a.st.strat_prefix[kNumKeys] = acc;
        a.st.ctl[CTL_STRAT_HEAD] = 0;
        a.st.ctl[CTL_STRAT_HEAD_OPEN] = 0;
    }
}
// OPEN = false: the buckets with one strategy each (all of them while no subpath exceeds 17 vertices).  OPEN = true (k_connect_strat_open): the
// buckets of the last row / column, whose items loop over every longer strategy of their sample — a kernel of its own so that the loop and
// the subpath lengths it needs do not weigh on the common case's registers.
template <bool OPEN>
WT_D void connect_strat_body(const launch_args_t& a) {
    __shared__ stack_entry_t lds[kLdsStack * kBlock];
    __shared__ uint32_t s_prefix[kNumKeys + 1];
    constexpr int K = (int)kKeyDim - 1;
    // flattened item space: OPEN = false all buckets (items of the open ones are skipped), OPEN = true the open buckets only
    if (!OPEN) {
        for (uint32_t k = threadIdx.x; k <= kNumKeys; k += kBlock) s_prefix[k] = a.st.strat_prefix[k];
    } else if (threadIdx.x == 0) {
        uint32_t acc = 0;
        for (uint32_t k = 0; k < kNumKeys; ++k) {
            s_prefix[k] = acc;
            if ((int)(k / kKeyDim) == K || (int)(k % kKeyDim) == K) acc += a.st.strat_prefix[k + 1] - a.st.strat_prefix[k];
        }
        s_prefix[kNumKeys] = acc;
    }
    __syncthreads();
    const uint32_t total = s_prefix[kNumKeys];
    bdpt_counters_t ctr;
    memset(&ctr, 0, sizeof(ctr));
    stack_entry_t spill[kSpillStack];
    stack_ref_t stack;
    lds_stack(lds, spill, stack);
    const fsd_pool_t pool = fsd_pool_of(a);
    for (;;) {
        const uint32_t base = wave_grab(a.st.ctl + (OPEN ? CTL_STRAT_HEAD_OPEN : CTL_STRAT_HEAD));
        const uint32_t idx = base + (threadIdx.x & 63);   // (in front of the break: behind it this kernel spills 263 registers instead of 204, 0.5 % of a pass in this form)
        if (base >= total) break;
        if (idx < total) {
            const uint32_t key = bucket_of(s_prefix, idx);
            const int tk = (int)(key / kKeyDim), sk = (int)(key % kKeyDim);
            if (!OPEN && (tk == K || sk == K)) continue;   // (k_connect_strat_open's)
            const uint32_t i = a.st.strat_items[(size_t)key * a.st.cap + (idx - s_prefix[key])];
            const uint64_t sample_id = sample_id_of(a, i);
            sample_ctx_t ctx;
            soa_load(a.st.ctx, kCtxWords, i, ctx);
            const vertex_store_t svs = sensor_vertices(a, i), evs = emitter_vertices(a, i);
            auto one = [&](int s, int t) __attribute__((always_inline)) {
                const stokes_t flux = bdpt_strategy(a.sc, pool, a.film, svs, evs, s, t, ctx, a.seed, sample_id, stack, &ctr, nullptr);
                if (t > 1) {
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        if (flux.s[c] != 0.f) unsafeAtomicAdd(&a.st.lacc[(size_t)c * a.st.cap + i], (double)flux.s[c]);
                }
            };
            if constexpr (!OPEN) {
                one(sk, tk);
            } else {
                const int nT = (int)a.st.walks[(size_t)i * a.st.walk_words + WT_WALK_NVERTS_WORD];
                const int nS = (int)a.st.walks[((size_t)a.st.cap + i) * a.st.walk_words + WT_WALK_NVERTS_WORD];
                const int t1 = tk == K ? nT : tk, s1 = sk == K ? nS : sk;
                for (int t = tk; t <= t1; ++t)
                    for (int s = sk; s <= s1; ++s)
                        if (strategy_valid(a.sc.opts, s, t, nS, nT)) one(s, t);
            }
        }
    }
    if (a.count_stats) flush_counters(a.st.counters, ctr);
}
__global__ void __launch_bounds__(kBlock, WTGPU_LB_CONNECT) k_connect_strat(launch_args_t a) { connect_strat_body<false>(a); }
__global__ void __launch_bounds__(kBlock, WTGPU_LB_CONNECT) k_connect_strat_open(launch_args_t a) { connect_strat_body<true>(a); }
// The class form.  OPEN = false: the classes whose subpath lengths ARE their key (all of them while no subpath exceeds 17 vertices): the strategies
// of an item are a wave-uniform loop.  OPEN = true (k_connect_class_open): the classes of the last row / column, whose samples have subpaths of
// different lengths >= 18 — trip counts per lane, read from the walks; a kernel of its own so that the common case does not carry them.
template <bool OPEN>
WT_D void connect_class_body(const launch_args_t& a) {
    __shared__ stack_entry_t lds[kLdsStack * kBlock];
    __shared__ uint32_t s_prefix[kNumKeys + 1], s_count[kNumKeys], s_key[kNumKeys];
    for (uint32_t r = threadIdx.x; r < kNumKeys; r += kBlock) {
        s_count[r] = a.st.strat_prefix[kClassCount + r];
        s_key[r] = a.st.strat_prefix[kClassKey + r];
    }
    // flattened item space: OPEN = false all classes (wavefronts that grab items of an open one skip them), OPEN = true the open classes only
    if (!OPEN) {
        for (uint32_t r = threadIdx.x; r <= kNumKeys; r += kBlock) s_prefix[r] = a.st.strat_prefix[r];
    } else if (threadIdx.x == 0) {
        uint32_t acc = 0;
        for (uint32_t r = 0; r < kNumKeys; ++r) {
            s_prefix[r] = acc;
            if (class_key_open(a.st.strat_prefix[kClassKey + r])) acc += (a.st.strat_prefix[kClassCount + r] + 63u) & ~63u;
        }
        s_prefix[kNumKeys] = acc;
    }
    __syncthreads();
    const uint32_t total = s_prefix[kNumKeys];
    const uint32_t lane = threadIdx.x & 63;
    bdpt_counters_t ctr;
    memset(&ctr, 0, sizeof(ctr));
    stack_entry_t spill[kSpillStack];
    stack_ref_t stack;
    lds_stack(lds, spill, stack);
    const fsd_pool_t pool = fsd_pool_of(a);
    for (;;) {
        const uint32_t base = wave_grab(a.st.ctl + (OPEN ? CTL_STRAT_HEAD_OPEN : CTL_STRAT_HEAD));
        if (base >= total) break;
        // class of this wavefront's 64 items (classes start at multiples of 64: one class per grab)
        const uint32_t rank = uniform(bucket_of(s_prefix, base)), key = uniform(s_key[rank]);
        const int tk = (int)(key / kKeyDim), sk = (int)(key % kKeyDim);
        const uint32_t off = base - uniform(s_prefix[rank]) + lane;
        if (class_key_open(key) == OPEN && off < uniform(s_count[rank])) {   // (the open classes' items: k_connect_class_open's)
            const uint32_t i = a.st.strat_items[(size_t)key * a.st.cap + off];
            const uint64_t sample_id = sample_id_of(a, i);
            sample_ctx_t ctx;
            soa_load(a.st.ctx, kCtxWords, i, ctx);
            const vertex_store_t svs = sensor_vertices(a, i), evs = emitter_vertices(a, i);
            int nT = tk, nS = sk;
            if constexpr (OPEN) {
                nT = (int)a.st.walks[(size_t)i * a.st.walk_words + WT_WALK_NVERTS_WORD];
                nS = (int)a.st.walks[((size_t)a.st.cap + i) * a.st.walk_words + WT_WALK_NVERTS_WORD];
            }
            double sum[4] = {0.0, 0.0, 0.0, 0.0};   // the sample's t>1 flux, in the fixed (t, s) order
            for (int t = 0; t <= nT; ++t)
                for (int s = 0; s <= nS; ++s)
                    if (strategy_valid(a.sc.opts, s, t, nS, nT)) {
                        const stokes_t flux = bdpt_strategy(a.sc, pool, a.film, svs, evs, s, t, ctx, a.seed, sample_id, stack, &ctr, nullptr);
                        if (t > 1) {
#pragma unroll
                            for (int c = 0; c < 4; ++c) sum[c] += (double)flux.s[c];
                        }
                    }
#pragma unroll
            for (int c = 0; c < 4; ++c) a.st.lacc[(size_t)c * a.st.cap + i] = sum[c];
        }
    }
    if (a.count_stats) flush_counters(a.st.counters, ctr);   // once per wavefront
}
__global__ void __launch_bounds__(kBlock, WTGPU_LB_CONNECT) k_connect_class(launch_args_t a) { connect_class_body<false>(a); }
__global__ void __launch_bounds__(kBlock, WTGPU_LB_CONNECT) k_connect_class_open(launch_args_t a) { connect_class_body<true>(a); }
// ---- staged connections (WTGPU_STAGED_CONNECT=1; the one-kernel forms above are the default) ---
// A connection is three things with very different shapes: forming the two connecting beams (two vertex loads, two BSDF evaluations, ~200
// registers), one any-hit ray (a BVH stack, ~90 registers, a run time that varies by two orders of magnitude), and the MIS weight (a stream
// over both subpaths).  One kernel for all three (k_connect_strat) carries the union of their registers — 256 + a 1.5-KB frame, two wavefronts
// per SIMD — and runs the ray with whatever lanes still have a connection.  Here:
//   k_connect_eval    lane / (sample, s, t), items bucketed by strategy as before: bdpt_connect<DEFER> — everything of connect_subpaths but the
//                     ray; connections with flux > 0 go into the pending list (52 B: sample, (s,t), flux, ray).  The items of a batch are taken
//                     in CHUNKS of as many items as the list has records, each chunk through the three kernels in turn: the list cannot
//                     overflow, whatever the depth of the scene (bdpt_ext_t);
//   k_connect_shadow  lane / pending connection, ALL lanes: the any-hit ray (src/ads/bvh8w.cpp:556-603), survivors compacted;
//   k_connect_mis     lane / survivor: the temporary vertex of the s = 1 / t = 1 / virtual-sensor strategies formed again from the same random
//                     numbers (bdpt_connect_temp), streaming MIS weight (plt_bdpt_detail.hpp:604-720), flux sum or light-image splat.
// Same functions, same numbers as the one-piece form (the CPU checker runs both: tests/test_oracle.py::test_staged_connections_are_the_connections).
constexpr uint32_t kPendShadow = 0x80000000u;   // conn_pending_t::st: the connection waits for its ray (t in bits 16..30, s in bits 0..15)
WT_D void pending_append(const launch_args_t& a, uint32_t* cctl, bool keep, uint32_t i, int s, int t, const connect_ret_t& cr) {
    const bdpt_ext_t& x = *a.st.ext;
    const unsigned long long m = __ballot(keep);
    if (!m) return;
    const int lane = threadIdx.x & 63;
    const int leader = __ffsll((long long)m) - 1;
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(cctl + CHUNK_PEND_COUNT, (uint32_t)__popcll(m));
    base = (uint32_t)__shfl((int)base, leader, 64);
    const uint32_t slot = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    if (!keep || slot >= x.pend_cap) return;   // (cannot happen: a chunk holds pend_cap items, each yields at most one connection)
    conn_pending_t r;
    r.i = i;
    r.st = (uint32_t)s | ((uint32_t)t << 16) | (cr.need_shadow ? kPendShadow : 0u);
#pragma unroll
    for (int c = 0; c < 4; ++c) r.L[c] = cr.L.s[c];
    r.o[0] = cr.ray.o.x, r.o[1] = cr.ray.o.y, r.o[2] = cr.ray.o.z;
    r.d[0] = cr.ray.d.x, r.d[1] = cr.ray.d.y, r.d[2] = cr.ray.d.z;
    r.dist = cr.ray.dist;
    x.pend[slot] = r;
}
#ifndef WTGPU_LB_EVAL
#define WTGPU_LB_EVAL 2
#endif
__global__ void __launch_bounds__(kBlock, WTGPU_LB_EVAL) k_connect_eval(launch_args_t a, uint32_t chunk) {
    __shared__ uint32_t s_prefix[kNumKeys + 1];
    for (uint32_t k = threadIdx.x; k <= kNumKeys; k += kBlock) s_prefix[k] = a.st.strat_prefix[k];
    __syncthreads();
    const bdpt_ext_t& x = *a.st.ext;
    uint32_t* cctl = x.chunk_ctl + (size_t)chunk * kChunkCtlWords;
    const uint32_t total = s_prefix[kNumKeys];
    const uint64_t begin = (uint64_t)chunk * x.pend_cap;
    if (begin >= total) return;   // (the host launches the chunks a batch of this depth can need at most: most are empty)
    const uint32_t span = (uint32_t)min<uint64_t>(x.pend_cap, total - begin);
    bdpt_counters_t ctr;
    ctr.connections = ctr.shadow_rays = 0;
    const stack_ref_t no_stack = make_stack_ref(nullptr, 0, 0, 0, nullptr);   // (bdpt_connect<true> traces nothing)
    const fsd_pool_t pool = fsd_pool_of(a);
    for (;;) {
        const uint32_t base = wave_grab(cctl + CHUNK_EVAL_HEAD);
        if (base >= span) break;
        const uint32_t off = base + (threadIdx.x & 63);
        if (off < span) {
            const uint32_t idx = (uint32_t)begin + off;
            const uint32_t key = bucket_of(s_prefix, idx);
            const int t = (int)(key / kKeyDim), s = (int)(key % kKeyDim);
            const uint32_t i = a.st.strat_items[(size_t)key * a.st.cap + (idx - s_prefix[key])];
            const uint64_t sample_id = sample_id_of(a, i);
            const vertex_store_t svs = sensor_vertices(a, i), evs = emitter_vertices(a, i);
            connect_ret_t cr;
            bdpt_connect<true>(a.sc, pool, svs, evs, s, t, a.seed, sample_id, no_stack, cr, &ctr, nullptr);
            pending_append(a, cctl, cr.L.s[0] > 0.f, i, s, t, cr);
        }
    }
    if (a.count_stats) {
        flush_counter(a, WT_COUNTER_SLOT(connections), ctr.connections);
        flush_counter(a, WT_COUNTER_SLOT(shadow_rays), ctr.shadow_rays);
    }
}

__global__ void __launch_bounds__(kBlock, 4) k_connect_shadow(launch_args_t a, uint32_t chunk) {
    __shared__ stack_entry_t lds[kLdsStack * kBlock];
    stack_entry_t spill[kSpillStack];
    stack_ref_t stack;
    lds_stack(lds, spill, stack);
    const bdpt_ext_t& x = *a.st.ext;
    uint32_t* cctl = x.chunk_ctl + (size_t)chunk * kChunkCtlWords;
    const uint32_t n = min(cctl[CHUNK_PEND_COUNT], x.pend_cap);
    if (n == 0) return;
    for (;;) {
        const uint32_t base = wave_grab(cctl + CHUNK_PEND_HEAD);
        if (base >= n) break;
        const uint32_t idx = base + (threadIdx.x & 63);
        bool alive = false;
        if (idx < n) {
            const conn_pending_t& r = x.pend[idx];
            alive = true;
            if (r.st & kPendShadow) alive = !ads_shadow_ray(a.sc, vec3{r.o[0], r.o[1], r.o[2]}, vec3{r.d[0], r.d[1], r.d[2]}, range_t{0.f, r.dist}, stack, nullptr);
        }
        wave_append(x.surv, cctl + CHUNK_SURV_COUNT, alive, idx);
    }
}

#ifndef WTGPU_LB_MIS
#define WTGPU_LB_MIS 2
#endif
__global__ void __launch_bounds__(kBlock, WTGPU_LB_MIS) k_connect_mis(launch_args_t a, uint32_t chunk) {
    const bdpt_ext_t& x = *a.st.ext;
    uint32_t* cctl = x.chunk_ctl + (size_t)chunk * kChunkCtlWords;
    const uint32_t n = cctl[CHUNK_SURV_COUNT];
    if (n == 0) return;
    const fsd_pool_t pool = fsd_pool_of(a);
    bdpt_counters_t ctr;
    ctr.light_splats = 0;
    for (;;) {
        const uint32_t base = wave_grab(cctl + CHUNK_MIS_HEAD);
        if (base >= n) break;
        const uint32_t k = base + (threadIdx.x & 63);
        if (k < n) {   // (no divergent `continue` in front of the loop header's grab: wave_grab0 assumes a converged wavefront)
            const conn_pending_t& r = x.pend[x.surv[k]];
            const uint32_t i = r.i, st = r.st;
            const int s = (int)(st & 0xFFFFu), t = (int)((st >> 16) & 0x7FFFu);
            stokes_t L;
    #pragma unroll
            for (int c = 0; c < 4; ++c) L.s[c] = r.L[c];
            const uint64_t sample_id = sample_id_of(a, i);
            sample_ctx_t ctx;
            soa_load(a.st.ctx, kCtxWords, i, ctx);
            const vertex_store_t svs = sensor_vertices(a, i), evs = emitter_vertices(a, i);
            vertex_nb_t tv;
            sensor_element_t element;
            bool has_element = false;
            if (s <= 1 || t <= 1) bdpt_connect_temp(a.sc, svs, evs, s, t, a.seed, sample_id, tv, element, has_element);
            const stokes_t flux = bdpt_strategy_finish(a.sc, pool, a.film, svs, evs, s, t, ctx, L, tv, element, has_element, &ctr);
            if (t > 1) {
    #pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (flux.s[c] != 0.f) unsafeAtomicAdd(&a.st.lacc[(size_t)c * a.st.cap + i], (double)flux.s[c]);
            }
        }
    }
    if (a.count_stats) flush_counter(a, WT_COUNTER_SLOT(light_splats), ctr.light_splats);
}

__global__ void __launch_bounds__(kBlock) k_connect_splat(launch_args_t a) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.nb) return;
    sample_ctx_t ctx;
    soa_load(a.st.ctx, kCtxWords, i, ctx);
    stokes_t L;
#pragma unroll
    for (int c = 0; c < 4; ++c) L.s[c] = (float)a.st.lacc[(size_t)c * a.st.cap + i];
    film_splat(a.sc, a.film, ctx.element, L, ctx.k);
}

// The same splat for batches that cover (most of) the film: one block per 64-element row segment accumulates the footprints of its
// elements' samples in an LDS tile (3 rows x 66 columns x (planes + 1) f64, plane-major) and adds the tile to the film once.  Per sample the
// plain kernel issues 9 x (planes + 1) f64 atomics on addresses its neighbours in the wavefront hit too — 117 for the Stokes film of the
// polarimetric workload, where it took 19.7 ms of a 204-ms batch (run r4t) — the tile turns them into LDS atomics and one global add per tile
// entry.  Same weights, same products, f64 sums in another order — a FIXED one: a film element gets the sums of up to six tiles (three rows x two
// neighbouring segments), and where a bright element lies next to a dark one these do not add up exactly, so the last bit of the film depended on
// which block came first (two renders of one batch differed in a few elements by one ulp: tests/test_gpu_heavy_uniform.py).  Hence one WAVEFRONT
// per block — the order inside a tile is the program's — and the blocks in kSplatPhases launches, one after the other on the batch's stream, by
// (row % 3, segment % 2): no two blocks of a launch touch the same film element.  Reconstruction-filter radius <= 1 (the host launches the plain kernel
// otherwise); a sample whose element is not where the block expects it (never, for the sensors built so far) goes to the film directly.
__global__ void __launch_bounds__(kSplatBlock) k_connect_splat_tiled(launch_args_t a, uint32_t phase) {
    extern __shared__ double tile[];   // [planes + 1][3][kSplatCols]
    const sensor_t& sn = a.sc.sensor;
    const uint32_t W = a.film.width, H = a.film.height;
    const uint32_t S = film_stokes(sn), P = sn.channels * S, PL = P + 1;
    // this launch's blocks: rows phase / 2, + 3, ...; of each, the segments phase % 2, + 2, ...  (wtgpu_kernels.h: kSplatPhases)
    const uint32_t spr = splat_phase_segments(phase, splat_segments(W));
    const uint32_t row = splat_block_row(phase, blockIdx.x, spr), x0 = splat_block_segment(phase, blockIdx.x, spr) * kSplatBlock;
    const uint32_t n_px = 3 * kSplatCols;
    for (uint32_t q = threadIdx.x; q < n_px * PL; q += kSplatBlock) tile[q] = 0.0;
    __syncthreads();
    const uint32_t x = x0 + threadIdx.x;
    if (x < W && row < H) {
        const uint64_t p = (uint64_t)row * W + x;
        // the samples of this batch that belong to element p: work items i with (j0 + i) % npix == p
        const uint64_t first = (p + a.npix - (a.j0 % a.npix)) % a.npix;
        for (uint64_t i = first; i < a.nb; i += a.npix) {
            sample_ctx_t ctx;
            soa_load(a.st.ctx, kCtxWords, i, ctx);
            stokes_t L;
#pragma unroll
            for (int c = 0; c < 4; ++c) L.s[c] = (float)a.st.lacc[(size_t)c * a.st.cap + i];
            // film_splat (wt/film.h) with the tile in place of the film
            film_splat_footprint(a.sc, W, H, ctx.element, L, ctx.k, [&](int xx, int y, float w, const float* val, uint32_t) {
                const int ty = y - ((int)row - 1), tx = xx - ((int)x0 - 1);
                if (ty >= 0 && ty < 3 && tx >= 0 && tx < (int)kSplatCols) {
                    const uint32_t q = (uint32_t)ty * kSplatCols + (uint32_t)tx;
                    unsafeAtomicAdd(&tile[q], (double)w);
                    for (uint32_t c = 0; c < P; ++c) unsafeAtomicAdd(&tile[(size_t)(1 + c) * n_px + q], (double)(w * val[c]));
                } else
                    film_splat_add(a.film, xx, y, w, val, P);
            });
        }
    }
    __syncthreads();
    for (uint32_t q = threadIdx.x; q < n_px; q += kSplatBlock) {
        const int y = (int)row - 1 + (int)(q / kSplatCols), xx = (int)x0 - 1 + (int)(q % kSplatCols);
        if (y < 0 || y >= (int)H || xx < 0 || xx >= (int)W) continue;
        const size_t pix = (size_t)y * W + xx;
        const double wsum = tile[q];
        if (wsum != 0.0) film_add(&a.film.weight[pix], wsum);
        for (uint32_t c = 0; c < P; ++c) {
            const double v = tile[(size_t)(1 + c) * n_px + q];
            if (v != 0.0) film_add(&a.film.value[pix * P + c], v);
        }
    }
}

}   // namespace wtk
