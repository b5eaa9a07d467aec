// oracle/flux64.cpp — f64 restatement of the region power integral.            *** TEST INFRASTRUCTURE ***
//
// What the f32 code of wt/gauss.h, wt/cone.h (clip_triangle_z, cone_project_local, region_local_triangle_flux) and wt/bdpt.h
// (region_triangle_flux) computes, derived again in plain double precision and by other means: the standard-normal mass of a polygon by
// strips in y with the x-integral in closed form (erfc) and adaptive bisection in y, a Sutherland-Hodgman clip against the slab, the central
// projection from the envelope's apex.  Of wt/ it includes only the scene record it reads triangles from.  tests/flux_probe.py wraps the
// entry points; tests/test_flux_probe.py pins them on their own (closed forms, scipy, additivity) before anything is held against them.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <thread>
#include <vector>

#include "../wave_tracer_amd/csrc/wt/scene.h"

namespace {

struct P2 {
    double x, y;
};
struct P3 {
    double x, y, z;
};
constexpr double kCap = 12.0;              // the mass of the standard normal beyond |x| or |y| = 12 is < 1e-32
constexpr double kAgree = 1e-14;           // two levels of the bisection agree to this
constexpr double kInvSqrt2 = 0.70710678118654752440, kInvSqrt2Pi = 0.39894228040143267794;

// one strip: phi(y) (Phi(xr(y)) - Phi(xl(y))) with both sides linear in y
struct strip_t {
    double xl0, ml, xr0, mr;
    double operator()(double y) const {
        double xl = xl0 + ml * y, xr = xr0 + mr * y;
        if (xl + xr < 0.0) {   // mirrored: the difference of two small erfc values rather than of two values near 2
            const double t = xl;
            xl = -xr;
            xr = -t;
        }
        return kInvSqrt2Pi * std::exp(-0.5 * y * y) * 0.5 * (std::erfc(xl * kInvSqrt2) - std::erfc(xr * kInvSqrt2));
    }
};
double gl8(const strip_t& f, double a, double b) {
    static const double X[4] = {0.18343464249564980494, 0.52553240991632898582, 0.79666647741362673959, 0.96028985649753623168};
    static const double W[4] = {0.36268378337836198297, 0.31370664587788728734, 0.22238103445337447054, 0.10122853629037625915};
    const double c = 0.5 * (a + b), r = 0.5 * (b - a);
    double s = 0.0;
    for (int i = 0; i < 4; ++i) s += W[i] * (f(c + r * X[i]) + f(c - r * X[i]));
    return s * r;
}
double adaptive(const strip_t& f, double a, double b, double whole, int depth) {
    const double m = 0.5 * (a + b);
    const double l = gl8(f, a, m), r = gl8(f, m, b);
    if (std::fabs(l + r - whole) <= kAgree || depth >= 40) return l + r;
    return adaptive(f, a, m, l, depth + 1) + adaptive(f, m, b, r, depth + 1);
}

// Sutherland-Hodgman against one half-space  s (v[axis] - bound) <= 0  (inclusive); in -> out, returns the new count
template <class P, class Get, class Mix>
int clip_half(const P* in, int n, P* out, double bound, double s, Get get, Mix mix) {
    int m = 0;
    for (int i = 0; i < n; ++i) {
        const P &p = in[i], &q = in[(i + 1) % n];
        const double dp = s * (get(p) - bound), dq = s * (get(q) - bound);
        const bool pin = dp <= 0.0, qin = dq <= 0.0;
        if (pin) out[m++] = p;
        if (pin != qin) out[m++] = mix(p, q, (bound - get(p)) / (get(q) - get(p)), bound);
    }
    return m;
}

// standard-normal mass of a convex polygon (either orientation)
double polygon_mass(const P2* poly, int n) {
    P2 a[16], b[16];
    for (int i = 0; i < n; ++i) a[i] = poly[i];
    const auto gx = [](const P2& p) { return p.x; };
    const auto gy = [](const P2& p) { return p.y; };
    const auto mx = [](const P2& p, const P2& q, double t, double bound) { return P2{bound, p.y + t * (q.y - p.y)}; };
    const auto my = [](const P2& p, const P2& q, double t, double bound) { return P2{p.x + t * (q.x - p.x), bound}; };
    n = clip_half(a, n, b, kCap, 1.0, gx, mx);
    n = clip_half(b, n, a, -kCap, -1.0, gx, mx);
    n = clip_half(a, n, b, kCap, 1.0, gy, my);
    n = clip_half(b, n, a, -kCap, -1.0, gy, my);
    if (n < 3) return 0.0;
    double ys[16];
    for (int i = 0; i < n; ++i) ys[i] = a[i].y;
    std::sort(ys, ys + n);
    double total = 0.0;
    for (int k = 0; k + 1 < n; ++k) {
        const double y0 = ys[k], y1 = ys[k + 1];
        if (!(y1 > y0)) continue;
        const double ym = 0.5 * (y0 + y1);
        // the edges that span the strip: the leftmost and the rightmost at its middle
        bool have = false;
        double xmin = 0, xmax = 0;
        strip_t f{0, 0, 0, 0};
        for (int i = 0; i < n; ++i) {
            const P2 &p = a[i], &q = a[(i + 1) % n];
            if (p.y == q.y || std::min(p.y, q.y) > y0 || std::max(p.y, q.y) < y1) continue;
            const double m = (q.x - p.x) / (q.y - p.y), x0 = p.x - m * p.y, xm = x0 + m * ym;
            if (!have || xm < xmin) {
                xmin = xm;
                f.xl0 = x0;
                f.ml = m;
            }
            if (!have || xm > xmax) {
                xmax = xm;
                f.xr0 = x0;
                f.mr = m;
            }
            have = true;
        }
        if (!have || !(xmax > xmin)) continue;
        // pieces of at most 0.5 in y and in the x run of either side before the bisection starts, so that no feature of the integrand (width
        // >= 1 in x or y) falls between the nodes of the first level
        const double dy = y1 - y0;
        const double run = std::max(dy, std::max(std::fabs(f.ml), std::fabs(f.mr)) * dy);
        const int pieces = (int)std::min(64.0, std::max(1.0, std::ceil(run / 0.5)));
        for (int p = 0; p < pieces; ++p) {
            const double lo = y0 + dy * p / pieces, hi = p + 1 == pieces ? y1 : y0 + dy * (p + 1) / pieces;
            total += adaptive(f, lo, hi, gl8(f, lo, hi), 0);
        }
    }
    return std::min(1.0, std::max(0.0, total));
}

int clip_slab(const P3* tri, double zmin, double zmax, P3* out) {
    P3 a[8], b[8];
    for (int i = 0; i < 3; ++i) a[i] = tri[i];
    const auto gz = [](const P3& p) { return p.z; };
    const auto mz = [](const P3& p, const P3& q, double t, double bound) { return P3{p.x + t * (q.x - p.x), p.y + t * (q.y - p.y), bound}; };
    int n = 3;
    if (std::isfinite(zmin)) {
        n = clip_half(a, n, b, zmin, -1.0, gz, mz);
        for (int i = 0; i < n; ++i) a[i] = b[i];
    }
    if (std::isfinite(zmax)) {
        n = clip_half(a, n, b, zmax, 1.0, gz, mz);
        for (int i = 0; i < n; ++i) a[i] = b[i];
    }
    for (int i = 0; i < n; ++i) out[i] = a[i];
    return n;
}

double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// cone: o (3), d (3), x (3), tan_alpha, x0.  want_front < 0: no facing test.  Returns the flux; *facing: dot(n, -d) > 0; *nverts: vertices of the
// clipped polygon
double region_flux(const double* cone, const double* izr, const double* sigma, const double* tri, const double* nrm, int want_front, int* facing,
                   int* nverts) {
    const double *o = cone, *d = cone + 3, *x = cone + 6, ta = cone[9], x0 = cone[10];
    const double y[3] = {d[1] * x[2] - d[2] * x[1], d[2] * x[0] - d[0] * x[2], d[0] * x[1] - d[1] * x[0]};
    const bool front = -dot3(nrm, d) > 0.0;
    if (facing) *facing = front ? 1 : 0;
    if (nverts) *nverts = 0;
    P3 l[3];
    for (int i = 0; i < 3; ++i) {
        const double v[3] = {tri[3 * i] - o[0], tri[3 * i + 1] - o[1], tri[3 * i + 2] - o[2]};
        l[i] = P3{dot3(v, x), dot3(v, y), dot3(v, d)};
    }
    P3 poly[8];
    const int n = clip_slab(l, izr[0], izr[1], poly);
    if (nverts) *nverts = n;
    if (want_front >= 0 && front != (want_front != 0)) return 0.0;
    if (n < 3 || sigma[0] == 0.0 || sigma[1] == 0.0) return 0.0;
    // central projection from the apex onto the cross-section at the slab's centre (the identity for a ray): lines stay lines
    const double csz = 0.5 * (izr[0] + izr[1]);
    const bool ray = ta == 0.0 && x0 == 0.0;
    P2 p[8];
    for (int i = 0; i < n; ++i) {
        const double s = ray ? 1.0 : (ta * csz + x0) / std::fabs(ta * poly[i].z + x0);
        p[i] = P2{poly[i].x * s / sigma[0], poly[i].y * s / sigma[1]};
    }
    double flux = 0.0;
    for (int i = 1; i + 1 < n; ++i) {
        const P2 t[3] = {p[0], p[i], p[i + 1]};
        flux += polygon_mass(t, 3);
    }
    return flux;
}

}   // namespace

extern "C" {

// the standard-normal mass of the triangle (a, b, c) in canonical coordinates
double ref_gauss_triangle(const double* a, const double* b, const double* c) {
    const P2 t[3] = {{a[0], a[1]}, {b[0], b[1]}, {c[0], c[1]}};
    return polygon_mass(t, 3);
}
void ref_gauss_triangles(const double* abc /* n x 6 */, uint32_t n, double* out) {
    for (uint32_t i = 0; i < n; ++i) out[i] = ref_gauss_triangle(abc + 6 * (size_t)i, abc + 6 * (size_t)i + 2, abc + 6 * (size_t)i + 4);
}
// the part of a triangle (9 doubles) with zmin <= z <= zmax (an infinite bound: no plane): vertex count, vertices to out (up to 5 x 3)
int ref_clip_slab(const double* tri, double zmin, double zmax, double* out) {
    const P3 t[3] = {{tri[0], tri[1], tri[2]}, {tri[3], tri[4], tri[5]}, {tri[6], tri[7], tri[8]}};
    P3 poly[8];
    const int n = clip_slab(t, zmin, zmax, poly);
    for (int i = 0; i < n; ++i) {
        out[3 * i] = poly[i].x;
        out[3 * i + 1] = poly[i].y;
        out[3 * i + 2] = poly[i].z;
    }
    return n;
}
// one triangle of a region: cone = o, d, x, tan_alpha, x0 (11 doubles); tri: 9 doubles in the world frame; nrm: its normal; want_front 0 / 1,
// or -1 for no facing test
double ref_region_flux(const double* cone, const double* izr, const double* sigma, const double* tri, const double* nrm, int want_front, int* facing,
                       int* nverts) {
    return region_flux(cone, izr, sigma, tri, nrm, want_front, facing, nverts);
}
void ref_region_fluxes(uint32_t n, const double* cones /* n x 11 */, const double* izr /* n x 2 */, const double* sigma /* n x 2 */,
                       const double* tris /* n x 9 */, const double* nrm /* n x 3 */, const int* want_front, double* flux, int* facing, int* nverts) {
    for (uint32_t i = 0; i < n; ++i)
        flux[i] = region_flux(cones + 11 * (size_t)i, izr + 2 * (size_t)i, sigma + 2 * (size_t)i, tris + 9 * (size_t)i, nrm + 3 * (size_t)i, want_front[i],
                              facing + i, nverts + i);
}
// the f64 sum of the above over a list of triangle ids of the scene (ids >= its triangle count are skipped)
double ref_region_sum(const void* scene_host, const double* cone, const double* izr, const double* sigma, const uint32_t* ids, uint32_t n, int want_front) {
    const wt::scene_t& sc = *static_cast<const wt::scene_t*>(scene_host);
    const uint32_t n_threads = n < 512 ? 1u : std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    std::vector<double> part(n_threads, 0.0);
    const auto work = [&](uint32_t t) {
        double s = 0.0;
        for (uint32_t i = (uint32_t)((uint64_t)n * t / n_threads), e = (uint32_t)((uint64_t)n * (t + 1) / n_threads); i < e; ++i) {
            if (ids[i] >= sc.n_tris) continue;
            const wt::tri_geo_t& g = sc.tri_geo[ids[i]];
            const double tri[9] = {g.a.x, g.a.y, g.a.z, g.b.x, g.b.y, g.b.z, g.c.x, g.c.y, g.c.z}, nrm[3] = {g.n.x, g.n.y, g.n.z};
            s += region_flux(cone, izr, sigma, tri, nrm, want_front, nullptr, nullptr);
        }
        part[t] = s;
    };
    if (n_threads == 1)
        work(0);
    else {
        std::vector<std::thread> th;
        for (uint32_t t = 0; t < n_threads; ++t) th.emplace_back(work, t);
        for (auto& t : th) t.join();
    }
    double sum = 0.0;
    for (double p : part) sum += p;
    return sum;
}

}   // extern "C"
