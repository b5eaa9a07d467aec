// wave_tracer_amd — what the sensor-element map kernels (kernels_mask.hip, kernels_firsthit.hip, kernels_firsthit_material.hip, kernels_los.hip)
// and their host twins share besides the arithmetic of their wt/ headers: the two lane shapes with their grids, a group's share of a ballot, the
// exchange through the LDS of the stacks with its sequential sums, and the host twin's loop over the elements.  A new map is a sample function
// plus calls into this header.
//
// One lane per element: lane p of the grid takes element p and traces its samples one after the other (on_lane_element, lane_blocks).
// One lane per sample (1 <= samples <= 64): a wavefront holds 64 / samples elements, lanes [g * samples, (g + 1) * samples) the samples of its
// g-th (sample_lane, sample_blocks); the lanes beyond the last whole group and the groups beyond the last element are not active, but reach every
// ballot and barrier of the kernel like the others.  What a group's lanes found comes together in two ways: one bit per sample in a ballot
// (group_bits), and floats through the LDS of the stacks once every lane of the block has finished its rays — word j of thread t at
// exchange_at(j, t) — which a lane adds up over the group in sample order, first term first (group_sum): the sum one thread would form.
#pragma once
#include "kernels_film.h"   // (on_threads)

namespace wtk {

// ---- one lane per element ---------------------------------------------------------------------------------------------------------------------
inline uint32_t lane_blocks(uint64_t n_elem) { return (uint32_t)((n_elem + kBlock - 1) / kBlock); }
// f(p, stack) on the lane of element p < n_elem, with the lane's stack in `lds` (kLdsStack * kBlock entries) and scratch
template <class F>
WT_D void on_lane_element(stack_entry_t* lds, uint32_t n_elem, F&& f) {
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n_elem) return;
    stack_entry_t spill[kSpillStack];
    stack_ref_t stack;
    lds_stack(lds, spill, stack);
    f(p, stack);
}

// ---- one lane per sample ----------------------------------------------------------------------------------------------------------------------
inline uint32_t sample_blocks(uint64_t n_elem, uint32_t samples) {
    const uint64_t waves = (n_elem + 64u / samples - 1) / (64u / samples);
    return lane_blocks(waves * 64u);
}
struct sample_lane_t {
    uint32_t g, s;    // the lane's group within the wavefront, its sample within the group
    uint32_t first;   // the group's first thread (of the block)
    uint64_t p;       // the group's element
    bool active;
};
WT_D sample_lane_t sample_lane(uint32_t samples, uint64_t n_elem) {
    const uint32_t per_wave = 64u / samples, lane = threadIdx.x & 63u, g = lane / samples, s = lane - g * samples;
    const uint64_t p = ((blockIdx.x * (uint64_t)kBlock + threadIdx.x) >> 6) * per_wave + g;
    return {g, s, threadIdx.x - s, p, g < per_wave && p < n_elem};
}
// the group's share of a ballot, sample t in bit t (a shift by 64 is undefined: a group of 64 is the wavefront)
WT_D unsigned long long group_bits(unsigned long long bits, const sample_lane_t& l, uint32_t samples) {
    return samples == 64u ? bits : (bits >> (l.g * samples)) & ((1ull << samples) - 1ull);
}

// The exchange: `words` 32-bit words per thread in the LDS of the stacks, word j of thread t at exchange_at(j, t).  The kernel's own barriers
// stand between the last use of a stack and the first store, between the stores and the loads, and before the stacks are used again.
template <uint32_t words>
constexpr void exchange_fits() {
    static_assert(words * sizeof(float) <= kLdsStack * sizeof(stack_entry_t), "the exchange of the per-sample form must fit the LDS of the stacks");
}
WT_D uint32_t exchange_at(uint32_t j, uint32_t t) { return j * kBlock + t; }
// word j summed over the group's samples in sample order, first term first: over those whose bit is set in `mask` (0 where none is) ...
WT_D float group_sum(const float* ex, uint32_t j, const sample_lane_t& l, uint32_t samples, unsigned long long mask) {
    float sum = 0.f;
    bool first = true;
    for (uint32_t t = 0; t < samples; ++t)
        if ((mask >> t) & 1ull) {
            sum = seq_add(first, sum, ex[exchange_at(j, l.first + t)]);
            first = false;
        }
    return sum;
}
// ... and over ALL of them, zeros included (the line-of-sight means).  The same sum as with every bit of the mask set, without the test per
// sample: with it k_los_sample's VISIBLE query took 0.83 ms in place of 0.79 on the MI355X.
WT_D float group_sum(const float* ex, uint32_t j, const sample_lane_t& l, uint32_t samples) {
    float sum = 0.f;
    for (uint32_t t = 0; t < samples; ++t) sum = seq_add(t == 0, sum, ex[exchange_at(j, l.first + t)]);
    return sum;
}
// word j of the first sample whose bit is set in `mask`; 0xFFFFFFFF where none is
WT_D uint32_t group_first_word(const uint32_t* exu, uint32_t j, const sample_lane_t& l, unsigned long long mask) {
    return mask ? exu[exchange_at(j, l.first + (uint32_t)__ffsll((long long)mask) - 1u)] : 0xFFFFFFFFu;
}

// ---- the host twins -----------------------------------------------------------------------------------------------------------------------------
// f(x, y, p, stack) for every element p = y * width + x of the sensor on n_threads host threads (on_threads), one task per row (the reference's
// own CPU job).  The stack holds kLdsStack + kSpillStack entries like a device lane's: a full stack drops the same children on both.
template <class F>
void on_elements(const scene_t& sc, uint32_t n_threads, F&& f) {
    const uint32_t W = sc.sensor.width, H = sc.sensor.height;
    on_threads(H, n_threads, [&](auto claim) {
        stack_entry_t entries[kLdsStack + kSpillStack];
        const stack_ref_t stack = make_stack_ref(entries, 1, kLdsStack + kSpillStack, kLdsStack + kSpillStack, nullptr);
        for (uint32_t y = (uint32_t)claim(); y < H; y = (uint32_t)claim())
            for (uint32_t x = 0; x < W; ++x) f(x, y, (size_t)y * W + x, stack);
    });
}

}   // namespace wtk
