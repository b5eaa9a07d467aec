"""oracle/indep/second_source.py — SECOND SOURCES of geometric primitives in double precision.        *** TEST INFRASTRUCTURE ***

Independent derivations (numpy f64, no wt/ header, no line of the restated algorithms) of quantities the physics headers compute, for
tests/test_second_source.py.  Where the other risky primitives have theirs: Fresnel coefficients and the Mueller matrix of a diagonal Jones
matrix — tests/test_kat.py (complex closed forms, Kronecker construction); UTD Ds / Dh — tests/test_kat_utd.py (Sommerfeld's exact half-plane
solution); the Fraunhofer edge sum (alpha_1 / alpha_2 / Psi / ASF, fsd.hpp:65-146) — fraunhofer_boundary_integral and polygon_fourier_integral
below (quadrature of the integrals the closed forms are the antiderivatives of).

cone_tri_min_z: the closest distance along the axis at which an elliptic cone  x^2 + (e y)^2 <= (z tan_alpha + x0)^2  meets a triangle
inside a z-slab (what intersect_cone_tri returns; the reference: include/wt/math/intersect/cone.hpp:550-626 via cone-plane and cone-edge
intersections in 3-D).  Here: a small convex programme in the triangle's barycentric plane — minimise the linear function z(u, v) over
{u, v >= 0, u + v <= 1} ∩ {g(u, v) <= 0} ∩ {zmin <= z <= zmax}, g the cone's quadratic form restricted to the plane — solved by enumerating
the KKT candidates: vertices, edge/cone and edge/slab crossings, the stationary points of z on g = 0 (Lagrange), and the slab's near plane."""
import numpy as np


def _quad_roots(a, b, c):
    if abs(a) < 1e-300:
        return [] if abs(b) < 1e-300 else [-c / b]
    D = b * b - 4 * a * c
    if D < 0:
        return []
    s = np.sqrt(D)
    q = -0.5 * (b + (s if b >= 0 else -s))
    r = [q / a]
    if abs(q) > 1e-300:
        r.append(c / q)
    return r


def cone_tri_min_z(P, tan_alpha, x0, e, zmin, zmax):
    """P: 3 x 3 triangle vertices in the cone's local frame (z along the axis, x the major axis).  Returns the minimal z or None."""
    P = np.asarray(P, np.float64)
    scale = max(1.0, float(np.abs(P).max()))
    A0, E1, E2 = P[0], P[1] - P[0], P[2] - P[0]
    w = np.array([1.0, e, 0.0])

    def point(u, v):
        return A0 + u * E1 + v * E2

    def g_of(p):
        r = p[2] * tan_alpha + x0
        return p[0] ** 2 + (e * p[1]) ** 2 - r * r

    def feasible(u, v, tol=1e-9):
        if u < -tol or v < -tol or u + v > 1 + tol:
            return None
        p = point(u, v)
        r = p[2] * tan_alpha + x0
        if r < -tol * scale or p[2] < zmin - tol * scale or p[2] > zmax + tol * scale:
            return None
        if g_of(p) > 1e-9 * scale * scale:
            return None
        return p[2]

    cands = []
    # vertices
    for (u, v) in ((0, 0), (1, 0), (0, 1)):
        cands.append((u, v))
    # edges: (u, v) = q0 + t dq
    for q0, dq in (((0.0, 0.0), (1.0, 0.0)), ((0.0, 0.0), (0.0, 1.0)), ((1.0, 0.0), (-1.0, 1.0))):
        a = point(*q0)
        d = point(q0[0] + dq[0], q0[1] + dq[1]) - a
        # g(a + t d) = (ax + t dx)^2 + e^2 (ay + t dy)^2 - ((az + t dz) ta + x0)^2
        ra, rd = a[2] * tan_alpha + x0, d[2] * tan_alpha
        qa = d[0] ** 2 + (e * d[1]) ** 2 - rd * rd
        qb = 2 * (a[0] * d[0] + e * e * a[1] * d[1] - ra * rd)
        qc = a[0] ** 2 + (e * a[1]) ** 2 - ra * ra
        ts = _quad_roots(qa, qb, qc)
        for zz in (zmin, zmax):
            if np.isfinite(zz) and abs(d[2]) > 1e-300:
                ts.append((zz - a[2]) / d[2])
        for t in ts:
            if -1e-12 <= t <= 1 + 1e-12:
                cands.append((q0[0] + t * dq[0], q0[1] + t * dq[1]))
    # g restricted to the plane: g(q) = q^T H q + 2 h^T q + c0
    def quad_form(Ea, Eb):
        return Ea[0] * Eb[0] + e * e * Ea[1] * Eb[1] - (Ea[2] * tan_alpha) * (Eb[2] * tan_alpha)
    r0 = A0[2] * tan_alpha + x0
    H = np.array([[quad_form(E1, E1), quad_form(E1, E2)], [quad_form(E1, E2), quad_form(E2, E2)]])
    h = np.array([A0[0] * E1[0] + e * e * A0[1] * E1[1] - r0 * E1[2] * tan_alpha, A0[0] * E2[0] + e * e * A0[1] * E2[1] - r0 * E2[2] * tan_alpha])
    c0 = A0[0] ** 2 + (e * A0[1]) ** 2 - r0 * r0
    zg = np.array([E1[2], E2[2]])
    # Lagrange: H q + h = mu zg, g(q) = 0
    if abs(np.linalg.det(H)) > 1e-14 * (np.abs(H).max() ** 2 + 1e-300) and np.abs(zg).max() > 1e-300:
        Hi = np.linalg.inv(H)
        qh, qz = -Hi @ h, Hi @ zg                      # q = qh + mu qz
        a2 = qz @ H @ qz
        b2 = 2 * (qh @ H @ qz + h @ qz)
        c2 = qh @ H @ qh + 2 * h @ qh + c0
        for mu in _quad_roots(a2, b2, c2):
            q = qh + mu * qz
            cands.append((q[0], q[1]))
    best = None
    for (u, v) in cands:
        z = feasible(u, v)
        if z is not None and (best is None or z < best):
            best = z
    # the slab's near plane: the triangle's section at z = zmin may cross the cone's disk although no candidate above lies on it
    if np.isfinite(zmin) and np.abs(zg).max() > 1e-300 and (best is None or best > zmin):
        # points of the (u, v) triangle with z = zmin: a segment; g along it is a quadratic
        pts = []
        for q0, dq in (((0.0, 0.0), (1.0, 0.0)), ((0.0, 0.0), (0.0, 1.0)), ((1.0, 0.0), (-1.0, 1.0))):
            za = point(*q0)[2]
            zb = point(q0[0] + dq[0], q0[1] + dq[1])[2]
            if abs(zb - za) > 1e-300:
                t = (zmin - za) / (zb - za)
                if -1e-12 <= t <= 1 + 1e-12:
                    pts.append(np.array([q0[0] + t * dq[0], q0[1] + t * dq[1]]))
        if len(pts) >= 2:
            qa_, qb_ = pts[0], pts[-1]
            for cand in pts[1:]:
                if np.linalg.norm(cand - qa_) > np.linalg.norm(qb_ - qa_):
                    qb_ = cand
            dq = qb_ - qa_
            a3 = dq @ H @ dq
            b3 = 2 * (qa_ @ H @ dq + h @ dq)
            c3 = qa_ @ H @ qa_ + 2 * h @ qa_ + c0
            ts = [0.0, 1.0]
            if abs(a3) > 1e-300:
                ts.append(min(1.0, max(0.0, -b3 / (2 * a3))))
            gmin = min(a3 * t * t + b3 * t + c3 for t in ts)
            if gmin <= 1e-9 * scale * scale and zmin * tan_alpha + x0 >= 0:
                best = zmin
    return best


def cone_contains(p, tan_alpha, x0, e, zmin, zmax):
    """A point (local frame) inside the cone within the slab."""
    r = p[2] * tan_alpha + x0
    return zmin <= p[2] <= zmax and r >= 0 and p[0] ** 2 + (e * p[1]) ** 2 <= r * r


# ---- Fraunhofer aperture: the edge sum of fsd.hpp:65-146 against the integrals it is the closed form of -------------------------------------
_GL_X, _GL_W = np.polynomial.legendre.leggauss(64)
_GL_X, _GL_W = (_GL_X + 1) / 2, _GL_W / 2


def fraunhofer_boundary_integral(segments, xi):
    """The far-field amplitude of an aperture given by boundary segments, as the LINE integral Stokes' theorem turns the Fourier integral of
    the aperture into:  B(xi) = sum_j (xi x e_j) / |xi|^2  *  int_0^1 c_j(t) exp(-i xi . (a_j + t e_j)) dt,  c_j(t) = ca_j + t (cb_j - ca_j)
    the (linearly interpolated) field amplitude along segment j from a_j to a_j + e_j.  64-point Gauss-Legendre per segment, f64.  The
    reference evaluates the same integral in closed form per segment — alpha_2 (the sinc term) for the mean amplitude, alpha_1 (its
    derivative) for the slope, times |e|^2 and the phase of the segment's midpoint (fsd.hpp:65-121) — and squares the sum: ASF = |B|^2 / (2 pi)^2.
    segments: iterable of (a[2], e[2], ca, cb)."""
    xi = np.asarray(xi, np.float64)
    B = 0j
    for a, e, ca, cb in segments:
        a, e = np.asarray(a, np.float64), np.asarray(e, np.float64)
        ph = np.exp(-1j * ((a[0] + _GL_X * e[0]) * xi[0] + (a[1] + _GL_X * e[1]) * xi[1]))
        B += (xi[0] * e[1] - xi[1] * e[0]) / (xi[0] ** 2 + xi[1] ** 2) * np.sum(_GL_W * (ca + _GL_X * (cb - ca)) * ph)
    return B


def fraunhofer_boundary_terms(a, e, ca, cb, xi):
    """The per-segment terms of fraunhofer_boundary_integral for arrays of segments (a[n,2], e[n,2], ca[n], cb[n]) at one direction: the same
    64-point rule, vectorised over the segments.  Their sum is B(xi)."""
    xi = np.asarray(xi, np.float64)
    a, e = np.asarray(a, np.float64), np.asarray(e, np.float64)
    ca, cb = np.asarray(ca, np.float64), np.asarray(cb, np.float64)
    px = a[:, 0:1] + _GL_X[None, :] * e[:, 0:1]
    py = a[:, 1:2] + _GL_X[None, :] * e[:, 1:2]
    ph = np.exp(-1j * (px * xi[0] + py * xi[1]))
    c = ca[:, None] + _GL_X[None, :] * (cb - ca)[:, None]
    return (xi[0] * e[:, 1] - xi[1] * e[:, 0]) / (xi[0] ** 2 + xi[1] ** 2) * np.sum(_GL_W[None, :] * c * ph, axis=1)


def polygon_fourier_integral(P, xi, n=40):
    """int_P exp(-i xi . x) d^2x over a simple polygon (vertices P[n,2]) by fan triangulation from P[0] and a Duffy-transformed tensor
    Gauss-Legendre rule per triangle (signed areas: any simple polygon).  The physics behind the edge sum: for a uniformly lit aperture
    |B(xi)| equals |this| — the Fraunhofer pattern IS the Fourier transform of the aperture."""
    P = np.asarray(P, np.float64)
    xi = np.asarray(xi, np.float64)
    g, w = np.polynomial.legendre.leggauss(n)
    g, w = (g + 1) / 2, w / 2
    U, V = np.meshgrid(g, g, indexing="ij")
    W = np.outer(w, w) * (1 - U)
    S, T = U, V * (1 - U)
    tot = 0j
    for i in range(1, len(P) - 1):
        a, b, c = P[0], P[i], P[i + 1]
        J = (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])
        X = a[0] + S * (b[0] - a[0]) + T * (c[0] - a[0])
        Y = a[1] + S * (b[1] - a[1]) + T * (c[1] - a[1])
        tot += J * np.sum(W * np.exp(-1j * (xi[0] * X + xi[1] * Y)))
    return tot


# ---------------------------------------------------------------------------------------------------------------------------------------------
# The material layer in f64 (tests/bsdf_probe.py): diffuse, dielectric and surface_spm with the Dirac, gaussian and fractal profiles, restated
# from the reference's formulas (scalar Python floats / complex: IEEE double and double complex).  It follows the reference, not ideal
# physics, including its asymmetries: f() evaluates Fresnel with Re(eta) and alpha(wi, wo), sample() with the complex eta and alpha(wi, wi),
# pdf() always applies the reflection / transmission split with Re(eta) and alpha(wi, wi) (src/bsdf/surface_spm.cpp:40-201).
# Directions are in the local shading frame (z: the normal); a `leaf` is a dict: type ("diffuse" | "dielectric" | "spm"), eta (complex,
# exterior / interior), refl (diffuse reflectance), profile ("dirac" | "fractal" | "gaussian"), roughness, gamma, sigma (gaussian, [1/mm],
# 0: roughness-parametrised), refl_scale, trans_scale.
import cmath as _cm
import math as _m

_MEANK = 2 * _m.pi / 550e-6                  # fractal.hpp:80: wavelen_to_wavenum(550 nm) [1/mm]
_MAX_GGX_ALPHA, _MAX_T = 0.75, 70.0 ** 2     # fractal.hpp:26-27
_F32_EPS = 2.0 ** -23


def spm_fresnel(eta, w, n=(0.0, 0.0, 1.0)):
    """fresnel.hpp:74-117: the coefficients of an interface of relative index eta (complex) seen from w; the refraction and every coefficient
    use the REAL index refract() returns.  -> dict t, eta (real), Z, rs, rp, ts, tp, Ts, Tp"""
    if eta == 1:
        return dict(t=(-w[0], -w[1], -w[2]), eta=1.0, Z=1.0, rs=0j, rp=0j, ts=1 + 0j, tp=1 + 0j, Ts=1.0, Tp=1.0)
    wn = w[0] * n[0] + w[1] * n[1] + w[2] * n[2]
    abs_cosi = abs(wn)
    # refract about n: express w in a frame where n is z (the callers use n = z or a half vector m)
    wt = (w[0] - wn * n[0], w[1] - wn * n[1], w[2] - wn * n[2])
    e = eta.real if wn > 0 else 1 / eta.real
    cost2 = 1 - e * e * (1 - wn * wn)
    if abs_cosi == 0 or cost2 < 0:
        return dict(t=(0.0, 0.0, 1.0), eta=e, Z=1.0, rs=1 + 0j, rp=1 + 0j, ts=0j, tp=0j, Ts=0.0, Tp=0.0)
    cost = _m.sqrt(cost2)
    s = 1.0 if wn >= 0 else -1.0
    t = tuple(-e * wt[i] - cost * s * n[i] for i in range(3))
    lt = _m.sqrt(sum(x * x for x in t))
    t = tuple(x / lt for x in t)
    rs = (e * abs_cosi - cost) / (e * abs_cosi + cost)
    rp = (abs_cosi - e * cost) / (abs_cosi + e * cost)
    ts, tp = rs + 1, (rp + 1) * e
    Z = abs(cost / (e * abs_cosi))
    return dict(t=t, eta=e, Z=Z, rs=complex(rs), rp=complex(rp), ts=complex(ts), tp=complex(tp), Ts=min(1.0, Z * ts * ts), Tp=min(1.0, Z * tp * tp))


def spm_fresnel_reflection(eta, w, n=(0.0, 0.0, 1.0)):
    """fresnel.hpp:128-144: the (conductor) reflection amplitudes with the complex index; 0 from below the normal"""
    wn = w[0] * n[0] + w[1] * n[1] + w[2] * n[2]
    if eta == 1 or wn < 0:
        return 0j, 0j
    t = _cm.sqrt(1 - (1 - wn * wn) * eta * eta)
    return (eta * wn - t) / (eta * wn + t), (wn - eta * t) / (wn + eta * t)


def mueller_from_jones(fs, fp):
    """The Mueller matrix of the diagonal Jones matrix diag(fs, fp) (mueller.hpp:294-316), row-major 4 x 4"""
    Rs, Rp = abs(fs) ** 2, abs(fp) ** 2
    x = fp * fs.conjugate()
    M = np.zeros(16)
    M[0] = M[5] = (Rs + Rp) / 2
    M[1] = M[4] = (Rs - Rp) / 2
    M[10] = M[15] = x.real
    M[11], M[14] = x.imag, -x.imag
    return M


def mueller_fresnel_rt(eta, reflection, w, n=(0.0, 0.0, 1.0)):
    """mueller.hpp:318-347: reflection -> the conductor amplitudes, transmission -> Z x the dielectric transmission amplitudes"""
    if reflection:
        return mueller_from_jones(*spm_fresnel_reflection(eta, w, n))
    f = spm_fresnel(eta, w, n)
    return f["Z"] * mueller_from_jones(f["ts"], f["tp"])


def _roughness_T(r):
    """fractal.hpp:29-34 (roughness_to_T) at 550 nm, and roughness_to_alpha (fractal.hpp:45-47)"""
    a2 = min(max(r, 0.0), _MAX_GGX_ALPHA) ** 2
    T = _MAX_T if a2 == 0 else min(_MAX_T, (1 - a2) / (4 * _MEANK ** 2 * a2))
    return T, (r / 9) ** 2


def profile_params(leaf, k):
    """fractal.hpp:76-103 / gaussian.hpp:94-117: (T or sigma2, sigma2_norm, alpha); the normalisations with expm1 / log1p (exact in f64)"""
    if leaf["profile"] == "fractal":
        T, alpha = _roughness_T(leaf["roughness"])
        s = (leaf["gamma"] - 1) / 2
        return T, 1 / -_m.expm1(-s * _m.log1p(k * k * T)), alpha
    if leaf["sigma"] > 0:
        sigma2 = leaf["sigma"] ** 2
        alpha = sigma2
    else:
        T, alpha = _roughness_T(leaf["roughness"])
        sigma2 = 1 / T
    return sigma2, 1 / -_m.expm1(-(k * k / 2 / sigma2)), alpha


def profile_alpha(leaf, wiz, woz, k):
    """the specular fraction exp(-((|wi.z| + |wo.z|) k)^2 alpha) (fractal.hpp:137-145, gaussian.hpp:156-163); 1 for Dirac"""
    if leaf["profile"] == "dirac":
        return 1.0
    return _m.exp(-((abs(wiz) + abs(woz)) * k) ** 2 * profile_params(leaf, k)[2])


def profile_delta_only(leaf):
    """is_delta_only (fractal.hpp:166-177, gaussian.hpp:165-169): a textured roughness has no mean value, so only Dirac is delta-only then"""
    if leaf.get("delta_only_by_mean"):
        return leaf["profile"] == "dirac"
    return leaf["profile"] == "dirac" or (leaf["roughness"] == 0 and not (leaf["profile"] == "gaussian" and leaf["sigma"] > 0))


def profile_psd_z(leaf, zx, zy, k):
    """the PSD at spatial frequency z [1/mm] (fractal.hpp:105-113, gaussian.hpp:120-128)"""
    P, norm, _ = profile_params(leaf, k)
    z2 = zx * zx + zy * zy
    if leaf["profile"] == "fractal":
        g = leaf["gamma"]
        return norm * (k * k * (g - 1) * P / (2 * _m.pi)) / (1 + P * z2) ** ((g + 1) / 2)
    e = _m.exp(-z2 / 2 / P)
    return 0.0 if e <= _F32_EPS else norm * (k * k * e / (2 * _m.pi * P))


def _gauss_max_phi(r, l):
    if r < _F32_EPS or l < _F32_EPS:
        return _m.pi
    return max(1e-2, _m.acos(min(1.0, max(-1.0, (r * r + l * l - 1) / (2 * r * l)))))


def profile_pdf(leaf, wi, wo, k):
    """the profile's sampling density of wo (fractal.hpp:209-229; gaussian.hpp:55-75 detail::boxmueller_truncated_pdf); 0 for Dirac"""
    if leaf["profile"] == "dirac":
        return 0.0
    if leaf["profile"] == "gaussian":
        s2 = profile_params(leaf, k)[0] / (k * k)
        mx, my = -wi[0], -wi[1]
        d2 = mx * mx + my * my
        l, coso = _m.sqrt(min(1.0, d2)), _m.sqrt(max(0.0, 1 - d2))
        r2 = (wo[0] - mx) ** 2 + (wo[1] - my) ** 2
        return .5 * _m.exp(-.5 * r2 / s2) / (_gauss_max_phi(_m.sqrt(r2), l) * s2) * coso
    zx, zy = wi[0] + wo[0], wi[1] + wo[1]
    fk = _m.hypot(zx, zy)
    s = _m.sqrt(max(0.0, 1 - wi[2] ** 2))
    phi_max = _m.pi if fk == 0 or s == 0 else _m.acos(min(1.0, max(-1.0, (fk * fk + s * s - 1) / (2 * fk * s))))
    w = phi_max / _m.pi
    return abs(wo[2]) * profile_psd_z(leaf, zx * k, zy * k, k) / w if w > 1e-2 else 0.0


def profile_sample(leaf, wi, k, u0, u1):
    """the profiles' sample maps from two uniforms: fractal.cpp:27-69 (Holzschuch & Pacanowski), gaussian.hpp:205-228 + 26-53 (truncated
    Box-Muller); the truncation masses with expm1 / log1p.  -> (wo, pdf, psd)"""
    if leaf["profile"] == "gaussian":
        P = profile_params(leaf, k)[0]
        s2 = P / (k * k)
        mx, my = -wi[0], -wi[1]
        d2 = mx * mx + my * my
        l, coso = _m.sqrt(min(1.0, d2)), _m.sqrt(max(0.0, 1 - d2))
        phi_i = _m.atan2(my, mx) if (mx != 0 or my != 0) else 0.0
        om = -_m.expm1(-.5 * (1 + l) ** 2 / s2) * (1 - max(_F32_EPS, u0))      # 1 - x
        x = 1 - om
        r = _m.sqrt(-2 * s2 * _m.log1p(-om))
        mp = _gauss_max_phi(r, l)
        phi = phi_i + _m.pi + mp * (2 * u1 - 1)
        wx, wy = r * _m.cos(phi) + mx, r * _m.sin(phi) + my
        pdf = .5 * x / (mp * s2) * coso
        psd = profile_psd_z(leaf, k * (wx - mx), k * (wy - my), k)
    else:
        T = profile_params(leaf, k)[0]
        g = leaf["gamma"]
        s = _m.sqrt(max(0.0, 1 - wi[2] ** 2))
        phi_i = _m.atan2(wi[1], wi[0]) if s > 0 else 0.0
        M = -_m.expm1(-(g - 1) / 2 * _m.log1p(k * k * T * (1 + s) ** 2))
        f = _m.sqrt(_m.expm1(-2 / (g - 1) * _m.log1p(-M * u0))) / _m.sqrt(T)
        fk = f / k
        phi_max = _m.pi if f == 0 or s == 0 else _m.acos(min(1.0, max(-1.0, (fk * fk + s * s - 1) / (2 * fk * s))))
        phf = phi_i + (2 * u1 - 1) * phi_max
        zx, zy = f * _m.cos(phf), f * _m.sin(phf)
        wx, wy = zx / k - wi[0], zy / k - wi[1]
        psd = profile_psd_z(leaf, zx, zy, k)
        w = phi_max / _m.pi
        z0 = _m.sqrt(max(0.0, 1 - wx * wx - wy * wy))
        pdf = z0 * psd / w if w > 1e-2 else 0.0
    z = _m.sqrt(max(0.0, 1 - wx * wx - wy * wy))
    return (wx, wy, z if wi[2] >= 0 else -z), pdf, psd


def spm_flip_wo(wo, eta):
    """surface_spm.cpp:28-36"""
    sc = eta if wo[2] > 0 else 1 / eta
    x, y = wo[0] * sc, wo[1] * sc
    l2 = x * x + y * y
    return (1.0, 0.0, 0.0) if l2 > 1 else (x, y, (-1.0 if wo[2] > 0 else 1.0) * _m.sqrt(max(0.0, 1 - l2)))


def spm_has_transmission(eta, leaf=None):
    """surface_spm.cpp:39: |Im eta|^2 / |eta|^2 <= 1e-2 (a leaf's `has_tr`, where given, decides instead: the caller's choice of side for an
    eta on the threshold itself)"""
    if leaf is not None and "has_tr" in leaf:
        return leaf["has_tr"]
    return abs(eta.imag) ** 2 / abs(eta) ** 2 <= 1e-2


def _half(wi, wo):
    h = [wi[i] + wo[i] for i in range(3)]
    if wi[2] < 0:
        h = [-x for x in h]
    l = _m.sqrt(sum(x * x for x in h))
    return tuple(x / l for x in h) if l > 0 else (float("nan"),) * 3


def leaf_f(leaf, wi, wo, k, backward):
    """bsdf f with the cosine foreshortening (diffuse.cpp:23-35, surface_spm.cpp:40-73); the dielectric is delta only: 0"""
    if leaf["type"] == "diffuse":
        M = np.zeros(16)
        M[0] = wo[2] / _m.pi * leaf["refl"] if (wi[2] > 0 and wo[2] > 0) else 0.0
        return M
    if leaf["type"] == "dielectric":
        return np.zeros(16)
    eta = leaf["eta"]
    refl = wi[2] * wo[2] >= 0
    if wi[2] == 0 or wo[2] == 0 or profile_delta_only(leaf) or (not refl and not spm_has_transmission(eta, leaf)):
        return np.zeros(16)
    awo = wo if refl else spm_flip_wo(wo, eta.real)
    alpha = profile_alpha(leaf, wi[2], awo[2], k)
    J = (1 / eta.real if wi[2] < 0 else eta.real) ** 2 if (not refl and backward) else 1.0
    F = mueller_fresnel_rt(complex(eta.real, 0), refl, wi, _half(wi, awo))
    psd = profile_psd_z(leaf, k * (wi[0] + awo[0]), k * (wi[1] + awo[1]), k) if leaf["profile"] != "dirac" else 0.0
    return (1 - alpha) * J * abs(wo[2]) * psd * (leaf["refl_scale"] if refl else leaf["trans_scale"]) * F


def leaf_pdf(leaf, wi, wo, k):
    """diffuse.cpp:63-71, dielectric (delta only: 0), surface_spm.cpp:165-196"""
    if leaf["type"] == "dielectric":
        return 0.0
    if leaf["type"] == "diffuse":
        return wo[2] / _m.pi if (wi[2] > 0 and wo[2] > 0) else 0.0
    eta = leaf["eta"]
    refl = wi[2] * wo[2] >= 0
    if wi[2] == 0 or wo[2] == 0 or (not refl and not spm_has_transmission(eta, leaf)):
        return 0.0
    awo = wo if refl else spm_flip_wo(wo, eta.real)
    alpha = profile_alpha(leaf, wi[2], wi[2], k)
    f = spm_fresnel(complex(eta.real, 0), wi)
    pt = (f["Ts"] + f["Tp"]) / 2
    return (1 - alpha) * profile_pdf(leaf, wi, awo, k) * ((1 - pt) if refl else pt)


def _cosine_hemisphere(u0, u1):
    """sampler.hpp:171-190 (Shirley-Chiu concentric map) and the cosine lift"""
    ox, oy = 2 * u0 - 1, 2 * u1 - 1
    if ox == 0 and oy == 0:
        r, th = 0.0, 0.0
    elif abs(ox) > abs(oy):
        r, th = ox, _m.pi / 4 * (oy / ox)
    else:
        r, th = oy, _m.pi / 2 - _m.pi / 4 * (ox / oy)
    x, y = r * _m.cos(th), r * _m.sin(th)
    return (x, y, _m.sqrt(max(0.0, 1 - x * x - y * y)))


def leaf_sample(leaf, wi, k, backward, u):
    """the leaf's sample from the uniforms u[...] in their order of use (diffuse.cpp:37-61, dielectric.cpp:26-72, surface_spm.cpp:75-157).
    -> dict valid, wo, dpd (tagged: a discrete mass negated), discrete, eta, M (the weighted bsdf), lobe ("specular" | "scatter"),
    reflection, used (uniforms consumed), and per decision (uniform index, f64 threshold) in `decisions`"""
    r = dict(valid=False, wo=(0.0, 0.0, 1.0), dpd=0.0, discrete=False, eta=1.0, M=np.zeros(16), lobe=None, reflection=None, used=0, decisions=[])
    i = 0
    if leaf["type"] == "diffuse":
        if wi[2] <= 0:
            return r
        wo = _cosine_hemisphere(u[0], u[1])
        M = np.zeros(16)
        M[0] = leaf["refl"]
        r.update(valid=True, wo=wo, dpd=wo[2] / _m.pi, M=M, lobe="scatter", reflection=True, used=2)
        return r
    if leaf["type"] == "dielectric":
        f = spm_fresnel(complex(leaf["eta"].real, 0), wi)
        T = (f["Ts"] + f["Tp"]) / 2
        refl = u[0] >= T
        r["decisions"].append((0, T))
        r["used"] = 1
        pdf = 1 - T if refl else T
        sc = leaf["refl_scale"] if refl else leaf["trans_scale"]
        if sc == 0:
            return r
        if refl:
            M = sc * mueller_from_jones(f["rs"], f["rp"])
            wo = (-wi[0], -wi[1], wi[2])
        else:
            M = f["Z"] * sc * mueller_from_jones(f["ts"], f["tp"]) * (f["eta"] ** 2 if backward else 1.0)
            wo = f["t"]
        r.update(valid=True, wo=wo, dpd=-1.0, discrete=True, eta=f["eta"], M=M / pdf, lobe="specular", reflection=refl)
        return r
    eta = leaf["eta"]
    alpha = profile_alpha(leaf, wi[2], wi[2], k)
    # the reference's alpha is an f_t = float: exp(-a) is 0 below the f32 range and 1 within half an ulp of 1, which decides whether
    # the specular resp. the scattered lobe exists; near those limits the f32 evaluation may go either way (decision index -1: the band)
    if alpha < 2.0 ** -149 or 1 - alpha < 2.0 ** -25:
        alpha = 0.0 if alpha < .5 else 1.0
    elif alpha < 2.0 ** -120 or 1 - alpha < 2.0 ** -22:
        r["decisions"].append((-1, alpha))
    has_spec, has_scat = alpha > 0, alpha < 1
    has_tr = spm_has_transmission(eta, leaf)
    if wi[2] == 0 or (not has_spec and not has_scat):
        return r
    pdf, spec = 1.0, has_spec
    if has_spec and has_scat:
        if alpha == 1:
            spec = True
        else:
            spec = u[i] < alpha
            r["decisions"].append((i, alpha))
            i += 1
        pdf = alpha if spec else 1 - alpha
    f = spm_fresnel(eta, wi)
    pt = (f["Ts"] + f["Tp"]) / 2
    refl = True
    if has_tr:
        refl = u[i] >= pt
        r["decisions"].append((i, pt))
        i += 1
        pdf *= (1 - pt) if refl else pt
    J = f["eta"] ** 2 if (not refl and backward) else 1.0
    sc = leaf["refl_scale"] if refl else leaf["trans_scale"]
    r["used"] = i
    if sc == 0 or (not refl and not has_tr):
        return r
    if spec:
        wo = (-wi[0], -wi[1], wi[2]) if refl else f["t"]
        F = mueller_fresnel_rt(eta, refl, wi)
        r.update(valid=True, wo=wo, dpd=-pdf, discrete=True, eta=1.0 if refl else f["eta"], M=F * (alpha * J * sc / pdf), lobe="specular",
                 reflection=refl)
        return r
    pwo, ppdf, psd = profile_sample(leaf, wi, k, u[i], u[i + 1])
    r["used"] = i + 2
    F = mueller_fresnel_rt(eta, refl, wi, _half(wi, pwo))
    wo = pwo if refl else spm_flip_wo(pwo, eta.real)
    if not refl:   # spm_flip_wo's l2 > 1 (no refracted direction: wo = (1,0,0)) decided within rounding
        sc_ = eta.real if pwo[2] > 0 else 1 / eta.real
        if abs((pwo[0] * sc_) ** 2 + (pwo[1] * sc_) ** 2 - 1) < 1e-5:
            r["decisions"].append((-1, 1.0))
    pdf *= ppdf
    r.update(valid=True, wo=wo, dpd=pdf, eta=1.0 if refl else f["eta"], M=F * ((1 - alpha) * J * abs(wo[2]) * psd * sc / pdf) if pdf != 0 else np.full(16, np.inf),
             lobe="scatter", reflection=refl)
    return r
