// wave_tracer_amd — denoising a film from its two half-films on the device (see wtgpu_kernels.h for the list of kernel translation units): the
// dual-buffer non-local-means filter of Rousselle, Knaus and Zwicker (2012), whose arithmetic and orders are wt/film_denoise.h's, shared with the
// host twin at the end of the file.  The first neighbourhood kernel of the film side:
//   k_denoise_prepare   one lane per pixel: develops A and B once into f32 planes [H][W][P], writes the pixel's valid byte and e_c of its guide planes;
//   k_denoise_variance  one lane per pixel: v_c from the 3 x 3 neighbourhood of e_c;
//   k_denoise_filter    one 256-thread block per 16 x 16 tile, the guide planes and variances of the tile's halo in LDS (below).
// No atomics, every sum in one order: out and residual are the host twin's bit for bit.  No render kernel is compiled here.
#include "kernels_film.h"
#include "wt/film_denoise.h"

namespace wtk {

constexpr uint32_t kDnTile = 16;                                              // a block's tile: kDnTile x kDnTile pixels, one per thread
constexpr uint32_t kDnMaxHalo = kDnTile + 2 * (kDnMaxWindow + kDnMaxPatch);   // 42: the tile, the window and the patch either side
constexpr uint32_t kDnMaxRegion = kDnTile + 2 * kDnMaxPatch;                  // 22: where a tile's pixels have their patches
constexpr uint32_t kDnMaxCand = kDnTile + 2 * kDnMaxWindow;                   // 36: where a tile's pixels have their candidates
static_assert(kDnTile * kDnTile == kFilmBlock, "one thread per pixel of the tile");

// The scratch memory of a call, in floats, every part a multiple of four floats long: the developed planes of A and of B, what the first direction
// leaves for the second when each has a launch of its own, e and v of the guide planes, then the two byte planes (valid; first direction has a sum).
struct dn_layout_t {
    size_t xa, xb, fa, e, v, valid, fa_ok, total;
};
static size_t dn_round4(size_t n) { return (n + 3) / 4 * 4; }
static dn_layout_t dn_layout(const sensor_t& sn) {
    const size_t npix = (size_t)sn.width * sn.height, planes = dn_round4(npix * film_planes(sn)), guides = dn_round4(npix * sn.channels), bytes = dn_round4((npix + 3) / 4);
    dn_layout_t l{};
    l.xa = 0, l.xb = planes, l.fa = 2 * planes, l.e = 3 * planes, l.v = l.e + guides, l.valid = l.v + guides, l.fa_ok = l.valid + bytes, l.total = l.fa_ok + bytes;
    return l;
}
size_t film_denoise_scratch_floats(const sensor_t& sn) { return dn_layout(sn).total; }

// ---- k_denoise_prepare: f64 films of A and B -> f32 planes, valid byte, e of the guide planes -------------------------------------------------
template <uint32_t C, uint32_t ST>
__global__ void __launch_bounds__(kFilmBlock) k_denoise_prepare(const double* __restrict__ a_value, const double* __restrict__ a_weight, const double* __restrict__ a_light,
                                                                double sl_a, const double* __restrict__ b_value, const double* __restrict__ b_weight,
                                                                const double* __restrict__ b_light, double sl_b, uint64_t npix, float* __restrict__ xa,
                                                                float* __restrict__ xb, float* __restrict__ e, unsigned char* __restrict__ valid) {
    constexpr uint32_t P = C * ST;
    const uint64_t p = blockIdx.x * (uint64_t)kFilmBlock + threadIdx.x;
    if (p >= npix) return;
    const double wa = a_weight[p], wb = b_weight[p];
    bool ok = true;
    float ga[C], gb[C];
#pragma unroll
    for (uint32_t i = 0; i < P; ++i) {
        const float a = develop_plane(a_value[p * P + i], wa, a_light[p * P + i], sl_a), b = develop_plane(b_value[p * P + i], wb, b_light[p * P + i], sl_b);
        xa[p * P + i] = a;
        xb[p * P + i] = b;
        ok = ok && dn_finite(a) && dn_finite(b);
        if (i % ST == 0) ga[i / ST] = a, gb[i / ST] = b;
    }
#pragma unroll
    for (uint32_t c = 0; c < C; ++c) e[p * C + c] = dn_e(ga[c], gb[c]);
    valid[p] = ok ? 1 : 0;
}

// ---- k_denoise_variance: e [H][W][C] -> v [H][W][C] ------------------------------------------------------------------------------------------
template <uint32_t C>
__global__ void __launch_bounds__(kFilmBlock) k_denoise_variance(const float* __restrict__ e, uint32_t W, uint32_t H, float* __restrict__ v) {
    const uint64_t p = blockIdx.x * (uint64_t)kFilmBlock + threadIdx.x;
    if (p >= (uint64_t)W * H) return;
    const int x = (int)(p % W), y = (int)(p / W);
#pragma unroll
    for (uint32_t c = 0; c < C; ++c) {
        float n[9];
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int i = 0; i < 3; ++i) n[j * 3 + i] = e[((uint64_t)dn_clamp(y + j - 1, H) * W + dn_clamp(x + i - 1, W)) * C + c];
        v[p * C + c] = dn_var9(n);
    }
}

// ---- k_denoise_filter: one block per 16 x 16 tile ---------------------------------------------------------------------------------------------
// LDS (dynamic, sized by the call's r and f: 31 KB with r = 7, f = 2, C = 3, so that five blocks share a CU's 160 KB where the largest halo's
// 46 KB would leave room for three).  Of the tile's halo of S = 16 + 2 (r + f) pixels a side, read with clamped coordinates: the variances v_c (the same for both directions) and
// the guide planes y_c of ONE guide buffer at a time — at most 42 x 42 x 6 floats = 42 KB with r = 10, f = 3, C = 3; a byte per pixel of the
// 16 + 2 r square says whether it may be a candidate (inside the film, valid, in the mask).  Per window offset d, in row-major order of (dy, dx):
// the block puts S_d(u) = s(u, u + d) for the (16 + 2 f)^2 pixels u that the tile's patches cover into LDS (C distance terms per pixel and offset
// where the naive form has C (2 f + 1)^2), then the horizontal sums h for the tile's 16 columns of those 16 + 2 f rows, left to right, then every
// thread takes its pixel's vertical sum, top to bottom, the weight, and accumulates the P planes of x(q) - x(p) from the developed planes in global
// memory (consecutive lanes read consecutive pixels).  Two barriers per offset: S_d is complete before h reads it, h before D reads it; the next
// offset's S_d is written after the barrier behind h, its h after the barrier behind its S_d.
// kMode 0: both directions in one launch, the first direction's result in registers.  1 / 2: the first / the second direction alone; the first
// leaves fa and whether it had a sum in `fa_buf` / `fa_ok`, where the second finds them (the measured alternative: film_denoise_launch).
// kGuided (wtgpu_film_denoise_guided_device; wt/film_denoise.h, "Guides"): the last argument carries the guide buffer, the id plane and the scales, G a
// run-time value.  The id plane of the candidate square goes into LDS behind the candidate bytes (SAME_ID: a candidate condition, tested before the
// patch sum is read); every lane holds g(p) in registers and takes g(q) either from global memory, where it also reads x(q) (staged = 0), or from
// the G planes of the candidate square in LDS, plane-major (staged = 1: dn_guided_staged decides, by WTGPU_FILM_DENOISE_GUIDE_LDS and by what
// fits into 64 KB).  F and the id test come before the weight; x(q) is read only where w > 0.  The unguided instantiations take an empty struct
// there and contain none of this.
struct dn_guide_args_t {
    const float* g;          // [H][W][G], null with G = 0
    const uint32_t* ids;     // [H][W], null without SAME_ID
    uint32_t staged;
    film_denoise_guides_t gd;
};
struct dn_no_guides_t {};
template <bool kGuided>
using dn_guide_arg = std::conditional_t<kGuided, dn_guide_args_t, dn_no_guides_t>;

template <uint32_t C, uint32_t ST, int kMode, bool kGuided>
__global__ void __launch_bounds__(kFilmBlock) k_denoise_filter(const float* __restrict__ xa, const float* __restrict__ xb, const float* __restrict__ var,
                                                               const unsigned char* __restrict__ valid, const float* __restrict__ mask, film_denoise_args_t a,
                                                               uint32_t W, uint32_t H, float* fa_buf, unsigned char* fa_ok, float* __restrict__ out,
                                                               float* __restrict__ residual, dn_guide_arg<kGuided> ga) {
    constexpr uint32_t P = C * ST, T = kDnTile;
    extern __shared__ __attribute__((aligned(16))) float dn_lds[];   // dn_filter_lds_bytes: sized by the call's radii, not by the largest
    const int r = (int)a.r, f = (int)a.f, R = r + f;
    const uint32_t S = T + 2u * (uint32_t)R, T2 = T + 2u * a.f, SO = T + 2u * a.r, n2f = 2u * a.f, SS = S * S;
    float* const s_v = dn_lds;                  // [C][S x S]
    float* const s_y = s_v + C * SS;            // [C][S x S]
    float* const s_s = s_y + C * SS;            // [T2 x T2]
    float* const s_h = s_s + T2 * T2;           // [T2 x T]
    unsigned char* const s_ok = reinterpret_cast<unsigned char*>(s_h + T2 * T);   // [SO x SO]
    const uint32_t SO2 = SO * SO;
    uint32_t G = 0;
    bool same_id = false, staged = false;
    uint32_t* s_id = nullptr;                   // [SO x SO] with SAME_ID
    float* s_g = nullptr;                       // [G][SO x SO] where the guides are staged
    if constexpr (kGuided) {
        G = ga.gd.n, same_id = (ga.gd.flags & kDnSameId) != 0, staged = ga.staged != 0;
        s_id = reinterpret_cast<uint32_t*>(s_ok + (SO2 + 3u) / 4u * 4u);
        s_g = reinterpret_cast<float*>(s_id + (same_id ? SO2 : 0u));
    }
    const int x0 = (int)(blockIdx.x * T), y0 = (int)(blockIdx.y * T);
    const uint32_t tid = threadIdx.x, tx = tid & (T - 1u), ty = tid / T;
    const uint32_t px = (uint32_t)x0 + tx, py = (uint32_t)y0 + ty;
    const bool inside = px < W && py < H;
    const uint64_t p = inside ? (uint64_t)py * W + px : 0u;

    for (uint32_t idx = tid; idx < S * S; idx += kFilmBlock) {
        const uint64_t g = (uint64_t)dn_clamp(y0 - R + (int)(idx / S), H) * W + dn_clamp(x0 - R + (int)(idx % S), W);
#pragma unroll
        for (uint32_t c = 0; c < C; ++c) s_v[c * SS + idx] = var[g * C + c];
    }
    for (uint32_t idx = tid; idx < SO * SO; idx += kFilmBlock) {
        const int qx = x0 - r + (int)(idx % SO), qy = y0 - r + (int)(idx / SO);
        bool ok = qx >= 0 && qy >= 0 && (uint32_t)qx < W && (uint32_t)qy < H;
        uint64_t g = 0;
        if (ok) {
            g = (uint64_t)qy * W + (uint32_t)qx;
            ok = valid[g] != 0 && (!mask || mask[g] > 0.f);
        }
        s_ok[idx] = ok ? 1 : 0;
        if constexpr (kGuided) {   // (what is no candidate is never looked up)
            if (same_id) s_id[idx] = ok ? ga.ids[g] : 0u;
            if (staged)
                for (uint32_t k = 0; k < G; ++k) s_g[k * SO2 + idx] = ok ? ga.g[g * G + k] : 0.f;
        }
    }
    float gp[kDnMaxGuides];
    uint32_t idp = 0;
    if constexpr (kGuided) {
#pragma unroll
        for (uint32_t k = 0; k < kDnMaxGuides; ++k) gp[k] = inside && k < G ? ga.g[p * G + k] : 0.f;
        if (same_id && inside) idp = ga.ids[p];
    }
    // the (at most two) region pixels u and row sums this thread computes per offset: where u is in the halo, where the row sum starts in the region
    const uint32_t n_region = T2 * T2, n_rows = T2 * T;
    uint32_t hu[2], hs[2];
#pragma unroll
    for (uint32_t k = 0; k < 2; ++k) {
        const uint32_t idx = tid + k * kFilmBlock;
        hu[k] = (idx / T2 + (uint32_t)r) * S + idx % T2 + (uint32_t)r;
        hs[k] = (idx / T) * T2 + idx % T;
    }
    const uint32_t cand0 = (ty + (uint32_t)r) * SO + tx + (uint32_t)r;   // this thread's pixel among the candidates

    float fa[P];
    bool active = false, fa_has_sum = false, has_sum = false;
    float fx[P], xp[P];
#pragma unroll
    for (uint32_t i = 0; i < P; ++i) fa[i] = fx[i] = xp[i] = 0.f;

    for (int dir = (kMode == 2 ? 1 : 0); dir < (kMode == 1 ? 1 : 2); ++dir) {
        const float* __restrict__ x = dir == 0 ? xa : xb;
        const float* __restrict__ y = dir == 0 ? xb : xa;
        __syncthreads();   // (the other direction's last S_d has been read)
        for (uint32_t idx = tid; idx < S * S; idx += kFilmBlock) {
            const uint64_t g = (uint64_t)dn_clamp(y0 - R + (int)(idx / S), H) * W + dn_clamp(x0 - R + (int)(idx % S), W);
#pragma unroll
            for (uint32_t c = 0; c < C; ++c) s_y[c * SS + idx] = y[g * P + c * ST];
        }
        __syncthreads();
        active = inside && s_ok[cand0] != 0;
        float acc[P], sw = 0.f;
#pragma unroll
        for (uint32_t i = 0; i < P; ++i) acc[i] = 0.f;
        if (active) {
#pragma unroll
            for (uint32_t i = 0; i < P; ++i) xp[i] = x[p * P + i];
        }
        for (int dy = -r; dy <= r; ++dy)
            for (int dx = -r; dx <= r; ++dx) {
                const int doff = dy * (int)S + dx;
#pragma unroll
                for (uint32_t k = 0; k < 2; ++k) {
                    const uint32_t idx = tid + k * kFilmBlock;
                    if (idx < n_region) {
                        const uint32_t u = hu[k], q = (uint32_t)((int)u + doff);
                        float s = dn_term(s_y[u], s_y[q], s_v[u], s_v[q], a);
#pragma unroll
                        for (uint32_t c = 1; c < C; ++c) s += dn_term(s_y[c * SS + u], s_y[c * SS + q], s_v[c * SS + u], s_v[c * SS + q], a);
                        s_s[idx] = s;
                    }
                }
                __syncthreads();
#pragma unroll
                for (uint32_t k = 0; k < 2; ++k) {
                    const uint32_t idx = tid + k * kFilmBlock;
                    if (idx < n_rows) {
                        float h = s_s[hs[k]];
                        for (uint32_t i = 1; i <= n2f; ++i) h += s_s[hs[k] + i];
                        s_h[idx] = h;
                    }
                }
                __syncthreads();
                const uint32_t cq = (uint32_t)((int)cand0 + dy * (int)SO + dx);
                bool cand = active && s_ok[cq] != 0;
                if constexpr (kGuided) {
                    if (cand && same_id) cand = s_id[cq] == idp;
                }
                if (cand) {
                    const uint64_t q = (uint64_t)((int64_t)p + (int64_t)dy * (int64_t)W + dx);
                    float D = s_h[ty * T + tx];
                    for (uint32_t j = 1; j <= n2f; ++j) D += s_h[(ty + j) * T + tx];
                    float Dc = D * a.inv_norm;
                    if constexpr (kGuided) {
                        float F = 0.f;
                        if (staged) {
#pragma unroll
                            for (uint32_t k = 0; k < kDnMaxGuides; ++k)
                                if (k < G) F += dn_feature_term(gp[k], s_g[k * SO2 + cq], ga.gd.scale[k]);
                        } else {
                            const float* __restrict__ gq = ga.g + q * G;
#pragma unroll
                            for (uint32_t k = 0; k < kDnMaxGuides; ++k)
                                if (k < G) F += dn_feature_term(gp[k], gq[k], ga.gd.scale[k]);
                        }
                        Dc = dn_guided(Dc, F);
                    }
                    const float w = dn_weight(Dc);
                    if (w > 0.f) {
                        sw += w;
                        const float* __restrict__ xq = x + q * P;
#pragma unroll
                        for (uint32_t i = 0; i < P; ++i) acc[i] += w * (xq[i] - xp[i]);
                    }
                }
            }
        has_sum = sw > 0.f;
        if (active && has_sum) {
#pragma unroll
            for (uint32_t i = 0; i < P; ++i) fx[i] = dn_filtered(xp[i], acc[i], sw);
        }
        if (kMode == 0 && dir == 0) {
            fa_has_sum = has_sum;
#pragma unroll
            for (uint32_t i = 0; i < P; ++i) fa[i] = fx[i];
        }
    }
    if (!inside) return;
    if (kMode == 1) {
        fa_ok[p] = active && has_sum ? 1 : 0;
#pragma unroll
        for (uint32_t i = 0; i < P; ++i) fa_buf[p * P + i] = fx[i];
        return;
    }
    if (kMode == 2) {
        fa_has_sum = fa_ok[p] != 0;
#pragma unroll
        for (uint32_t i = 0; i < P; ++i) fa[i] = fa_buf[p * P + i];
    }
    const bool filtered = active && fa_has_sum && has_sum;
#pragma unroll
    for (uint32_t i = 0; i < P; ++i) {
        const float u = filtered ? fa[i] : xa[p * P + i], w = filtered ? fx[i] : xb[p * P + i];
        out[p * P + i] = dn_canon((u + w) * 0.5f);
        if (residual) residual[p * P + i] = dn_canon((u - w) * 0.5f);
    }
}

// the filter's LDS for a call's radii: v and y of the halo, S_d, its row sums, the candidate bytes (rounded up to whole floats)
// guided: + a word per candidate for the ids (SAME_ID) and, where the guides are staged, n_staged planes of the candidate square
static size_t dn_filter_lds_bytes(uint32_t C, uint32_t r, uint32_t f, bool ids = false, uint32_t n_staged = 0) {
    const size_t S = kDnTile + 2 * (r + f), T2 = kDnTile + 2 * f, SO = kDnTile + 2 * r;
    return (2 * C * S * S + T2 * T2 + T2 * kDnTile + (SO * SO + 3) / 4 + (ids ? SO * SO : 0) + n_staged * SO * SO) * sizeof(float);
}
constexpr size_t kDnMaxLds = 65536;   // what a launch may ask for without an attribute
static_assert((2 * 3 * kDnMaxHalo * kDnMaxHalo + kDnMaxRegion * kDnMaxRegion + kDnMaxRegion * kDnTile + (kDnMaxCand * kDnMaxCand + 3) / 4 + kDnMaxCand * kDnMaxCand) *
                      sizeof(float) <= kDnMaxLds,
              "the largest halo and its id plane fit the 64 KB a launch may ask for without an attribute");
// The guides go into LDS where the knob asks for it and they fit beside the rest; from global memory otherwise.  Which form: on the MI355X
// (tools/bench_film_denoise_guided.py, profiles/film_denoise_guided_bench.json: window 7, patch 2, five planes and ids; median of 15 calls each,
// alternated, beside the unguided call at 5.02 / 7.40 ms in the same run) from global memory 7.69 ms on the cornell film (P = 3) and 10.77 ms on the
// polarimetric room film (P = 12), staged 8.54 and 10.71 ms: 18 KB more LDS leave three blocks per CU where the id plane alone leaves four, and
// the loads it saves were served by the caches.  The knob's default is therefore 0.
static bool dn_guided_staged(uint32_t C, const film_denoise_args_t& a, const film_denoise_guides_t& gd, uint32_t knob) {
    return knob != 0 && gd.n > 0 && dn_filter_lds_bytes(C, a.r, a.f, (gd.flags & kDnSameId) != 0, gd.n) <= kDnMaxLds;
}

template <uint32_t C, uint32_t ST, bool kGuided>
static void denoise_launch_cs(hipStream_t stream, const double* a_value, const double* a_weight, const double* a_light, double sl_a, const double* b_value,
                              const double* b_weight, const double* b_light, double sl_b, const film_denoise_args_t& a, bool fused, const float* d_mask, uint32_t W,
                              uint32_t H, float* xa, float* xb, float* fa, float* e, float* v, unsigned char* valid, unsigned char* fa_ok, float* d_out,
                              float* d_residual, const dn_guide_arg<kGuided>& ga, size_t lds) {
    const uint64_t npix = (uint64_t)W * H;
    const dim3 pixels((uint32_t)((npix + kFilmBlock - 1) / kFilmBlock)), tiles((W + kDnTile - 1) / kDnTile, (H + kDnTile - 1) / kDnTile), block(kFilmBlock);
    hipLaunchKernelGGL((k_denoise_prepare<C, ST>), pixels, block, 0, stream, a_value, a_weight, a_light, sl_a, b_value, b_weight, b_light, sl_b, npix, xa, xb, e, valid);
    hipLaunchKernelGGL((k_denoise_variance<C>), pixels, block, 0, stream, e, W, H, v);
    if (fused) {
        hipLaunchKernelGGL((k_denoise_filter<C, ST, 0, kGuided>), tiles, block, lds, stream, xa, xb, v, valid, d_mask, a, W, H, fa, fa_ok, d_out, d_residual, ga);
    } else {
        hipLaunchKernelGGL((k_denoise_filter<C, ST, 1, kGuided>), tiles, block, lds, stream, xa, xb, v, valid, d_mask, a, W, H, fa, fa_ok, d_out, d_residual, ga);
        hipLaunchKernelGGL((k_denoise_filter<C, ST, 2, kGuided>), tiles, block, lds, stream, xa, xb, v, valid, d_mask, a, W, H, fa, fa_ok, d_out, d_residual, ga);
    }
}

template <bool kGuided>
static int denoise_launch(const sensor_t& sn, hipStream_t stream, const double* a_value, const double* a_weight, const double* a_light, uint64_t spe_a,
                          const double* b_value, const double* b_weight, const double* b_light, uint64_t spe_b, const film_denoise_args_t& a, uint32_t fused,
                          const float* d_mask, float* d_scratch, float* d_out, float* d_residual, const dn_guide_arg<kGuided>& ga, bool ids, uint32_t n_staged) {
    const uint32_t W = sn.width, H = sn.height, stokes = film_stokes(sn);
    if ((uint64_t)W * H == 0 || (stokes != 1 && stokes != 4) || a.r > kDnMaxWindow || a.f > kDnMaxPatch) return (int)hipErrorInvalidValue;
    // Which form: on the MI355X (tools/bench_film_denoise.py, profiles/film_denoise_bench.json: window 7, patch 2; median of 15 calls each, alternated,
    // all the call's kernels between device events) both directions in one launch take 4.77 ms on the cornell film (1440 x 1440, P = 3) and 7.60 ms on
    // the polarimetric room film (1920 x 1088, P = 12), one launch per direction 4.85 and 7.17 ms (an earlier run: 4.80 / 7.50 against 4.89 / 7.11): the
    // caller (wtgpu_film_denoise_device) takes the fused form up to 4 planes and two launches for 12, whose fused form needs 104 VGPRs.
    const dn_layout_t l = dn_layout(sn);
    float* const s = d_scratch;
    unsigned char* const valid = reinterpret_cast<unsigned char*>(s + l.valid);
    unsigned char* const fa_ok = reinterpret_cast<unsigned char*>(s + l.fa_ok);
    const double sl_a = develop_scale(spe_a), sl_b = develop_scale(spe_b);
    if (!film_dispatch(sn.channels, false, [&](auto c, auto) {
            constexpr uint32_t C = decltype(c)::value;
            const size_t lds = dn_filter_lds_bytes(C, a.r, a.f, ids, n_staged);
            if (stokes == 1)
                denoise_launch_cs<C, 1, kGuided>(stream, a_value, a_weight, a_light, sl_a, b_value, b_weight, b_light, sl_b, a, fused != 0, d_mask, W, H, s + l.xa, s + l.xb,
                                                 s + l.fa, s + l.e, s + l.v, valid, fa_ok, d_out, d_residual, ga, lds);
            else
                denoise_launch_cs<C, 4, kGuided>(stream, a_value, a_weight, a_light, sl_a, b_value, b_weight, b_light, sl_b, a, fused != 0, d_mask, W, H, s + l.xa, s + l.xb,
                                                 s + l.fa, s + l.e, s + l.v, valid, fa_ok, d_out, d_residual, ga, lds);
        }))
        return (int)hipErrorInvalidValue;
    return (int)hipGetLastError();
}

int film_denoise_launch(const sensor_t& sn, hipStream_t stream, const double* a_value, const double* a_weight, const double* a_light, uint64_t spe_a,
                        const double* b_value, const double* b_weight, const double* b_light, uint64_t spe_b, const film_denoise_args_t& a, uint32_t fused,
                        const float* d_mask, float* d_scratch, float* d_out, float* d_residual) {
    return denoise_launch<false>(sn, stream, a_value, a_weight, a_light, spe_a, b_value, b_weight, b_light, spe_b, a, fused, d_mask, d_scratch, d_out, d_residual,
                                 dn_no_guides_t{}, false, 0);
}

// The guided call: the same three or four kernels, the filter in its guided instantiation.  guide_lds: WTGPU_FILM_DENOISE_GUIDE_LDS.
int film_denoise_guided_launch(const sensor_t& sn, hipStream_t stream, const double* a_value, const double* a_weight, const double* a_light, uint64_t spe_a,
                               const double* b_value, const double* b_weight, const double* b_light, uint64_t spe_b, const film_denoise_args_t& a, uint32_t fused,
                               const film_denoise_guides_t& gd, uint32_t guide_lds, const float* d_guide, const uint32_t* d_ids, const float* d_mask,
                               float* d_scratch, float* d_out, float* d_residual) {
    if (gd.n > kDnMaxGuides || (gd.n > 0) != (d_guide != nullptr) || ((gd.flags & kDnSameId) != 0) != (d_ids != nullptr)) return (int)hipErrorInvalidValue;
    const bool ids = (gd.flags & kDnSameId) != 0, staged = dn_guided_staged(sn.channels, a, gd, guide_lds);
    const dn_guide_args_t ga{d_guide, d_ids, staged ? 1u : 0u, gd};
    return denoise_launch<true>(sn, stream, a_value, a_weight, a_light, spe_a, b_value, b_weight, b_light, spe_b, a, fused, d_mask, d_scratch, d_out, d_residual, ga,
                                ids, staged ? gd.n : 0u);
}

// ---- the host twin: the same wt/film_denoise.h functions on host threads, naive per pixel and candidate in the header's orders; every pixel is
// one thread's, so the result does not depend on the number of threads.  gd (may be null: the unguided call), guide, ids: wt/film_denoise.h's guides ----
void film_denoise_host(const sensor_t& sn, const double* a_value, const double* a_weight, const double* a_light, uint64_t spe_a, const double* b_value,
                       const double* b_weight, const double* b_light, uint64_t spe_b, const film_denoise_args_t& a, const float* mask, uint32_t n_threads,
                       float* out, float* residual, const film_denoise_guides_t* gd, const float* guide, const uint32_t* ids) {
    const uint32_t G = gd ? gd->n : 0u;
    const bool same_id = gd && (gd->flags & kDnSameId) != 0;
    const uint32_t W = sn.width, H = sn.height, C = sn.channels, ST = film_stokes(sn), P = C * ST;
    const uint64_t npix = (uint64_t)W * H;
    const double sl_a = develop_scale(spe_a), sl_b = develop_scale(spe_b);
    std::vector<float> xa(npix * P), xb(npix * P), e(npix * C), v(npix * C);
    std::vector<unsigned char> ok(npix);
    on_threads(H, n_threads, [&](auto claim) {
        for (uint64_t row = claim(); row < H; row = claim())
            for (uint64_t p = row * W; p < (row + 1) * W; ++p) {
                bool fin = true;
                for (uint32_t i = 0; i < P; ++i) {
                    xa[p * P + i] = develop_plane(a_value[p * P + i], a_weight[p], a_light[p * P + i], sl_a);
                    xb[p * P + i] = develop_plane(b_value[p * P + i], b_weight[p], b_light[p * P + i], sl_b);
                    fin = fin && dn_finite(xa[p * P + i]) && dn_finite(xb[p * P + i]);
                }
                for (uint32_t c = 0; c < C; ++c) e[p * C + c] = dn_e(xa[p * P + c * ST], xb[p * P + c * ST]);
                ok[p] = fin && (!mask || mask[p] > 0.f) ? 1 : 0;
            }
    });
    on_threads(H, n_threads, [&](auto claim) {
        for (uint64_t row = claim(); row < H; row = claim())
            for (uint32_t x = 0; x < W; ++x)
                for (uint32_t c = 0; c < C; ++c) {
                    float n[9];
                    for (int j = 0; j < 3; ++j)
                        for (int i = 0; i < 3; ++i) n[j * 3 + i] = e[((uint64_t)dn_clamp((int)row + j - 1, H) * W + dn_clamp((int)x + i - 1, W)) * C + c];
                    v[(row * W + x) * C + c] = dn_var9(n);
                }
    });
    const int r = (int)a.r, f = (int)a.f;
    on_threads(H, n_threads, [&](auto claim) {
        for (uint64_t row = claim(); row < H; row = claim())
            for (uint32_t px = 0; px < W; ++px) {
                const int py = (int)row;
                const uint64_t p = row * W + px;
                float fx[2][kDnMaxPlanes];
                bool filtered = ok[p] != 0;
                for (int dir = 0; dir < 2 && filtered; ++dir) {
                    const float* x = dir == 0 ? xa.data() : xb.data();
                    const float* y = dir == 0 ? xb.data() : xa.data();
                    float acc[kDnMaxPlanes], sw = 0.f;
                    for (uint32_t i = 0; i < P; ++i) acc[i] = 0.f;
                    for (int dy = -r; dy <= r; ++dy)
                        for (int dx = -r; dx <= r; ++dx) {
                            const int qx = (int)px + dx, qy = py + dy;
                            if (qx < 0 || qy < 0 || (uint32_t)qx >= W || (uint32_t)qy >= H) continue;
                            const uint64_t q = (uint64_t)qy * W + (uint32_t)qx;
                            if (!ok[q] || (same_id && ids[q] != ids[p])) continue;
                            float D = 0.f;
                            for (int j = -f; j <= f; ++j) {
                                float h = 0.f;
                                for (int i = -f; i <= f; ++i) {
                                    const uint64_t u = (uint64_t)dn_clamp(py + j, H) * W + dn_clamp((int)px + i, W), t = (uint64_t)dn_clamp(qy + j, H) * W + dn_clamp(qx + i, W);
                                    float s = dn_term(y[u * P], y[t * P], v[u * C], v[t * C], a);
                                    for (uint32_t c = 1; c < C; ++c) s += dn_term(y[u * P + c * ST], y[t * P + c * ST], v[u * C + c], v[t * C + c], a);
                                    h = i == -f ? s : h + s;
                                }
                                D = j == -f ? h : D + h;
                            }
                            float Dc = D * a.inv_norm;
                            if (gd) {
                                float F = 0.f;
                                for (uint32_t g = 0; g < G; ++g) F += dn_feature_term(guide[p * G + g], guide[q * G + g], gd->scale[g]);
                                Dc = dn_guided(Dc, F);
                            }
                            const float w = dn_weight(Dc);
                            if (w > 0.f) {
                                sw += w;
                                for (uint32_t i = 0; i < P; ++i) acc[i] += w * (x[q * P + i] - x[p * P + i]);
                            }
                        }
                    filtered = sw > 0.f;
                    if (filtered)
                        for (uint32_t i = 0; i < P; ++i) fx[dir][i] = dn_filtered(x[p * P + i], acc[i], sw);
                }
                for (uint32_t i = 0; i < P; ++i) {
                    const float u = filtered ? fx[0][i] : xa[p * P + i], w = filtered ? fx[1][i] : xb[p * P + i];
                    out[p * P + i] = dn_canon((u + w) * 0.5f);
                    if (residual) residual[p * P + i] = dn_canon((u - w) * 0.5f);
                }
            }
    });
}

void film_denoise_exp2_neg(const float* t, uint64_t n, float* out) {
    for (uint64_t i = 0; i < n; ++i) out[i] = dn_exp2_neg(t[i]);
}

}   // namespace wtk
