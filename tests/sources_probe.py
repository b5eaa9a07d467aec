"""Per-query checks of the emitter / sensor / wavenumber layer (wt/sources_probe.h): the CPU checker's entry point oracle_source_queries, the
query sets both test files use, and an f64 restatement of every op written against the reference's formulas (spot.hpp / spot.cpp, area.hpp /
area.cpp, point.cpp, directional.hpp / directional.cpp, shape.cpp, perspective.hpp, virtual_plane_sensor.hpp / .cpp, scene_sensor.cpp,
sampler.hpp, beam_geometry.hpp), not against wt/sources.h.

The f64 side reads the baked records back through the checker's accessors (oracle_emitter_record, oracle_sensor_record, oracle_kdist_table,
...), widens them to f64 and replays the sample maps from the uniforms the probe copies out.  Spectra and radiance textures are inputs of this
layer: their f32 values come from the checker (kat_spectrum, oracle_texture_spectral).

Decisions.  Comparisons between stored f32 numbers (a uniform against a cdf knot, k against kmin) are exact in f64 and need no band.  A decision
on a COMPUTED quantity (a point against the target disk's rim, dn > 0, the floor of a film position, inside / outside the film, u.x + u.y > 1)
goes through `Decider`: within BAND_ULPS f32 ulps of its threshold the query is `in the band`.  A random set skips such queries (counted, at
most 1 %); an edge set, which sits on thresholds by construction, evaluates the f64 side under each admissible branch and is compared under the
branch whose discrete outputs equal the f32 code's: the decision the f32 code took.

Conditioning.  f64_with_bound returns, per float word, the spread of the f64 result when the query's inputs (world point, direction, k,
barycentrics, the uniforms) move by one f32 ulp: what an f32 evaluation cannot resolve (1 / recp_dist2, 1 / dn, 1 / recp_dpd, dir / |dir.z|)."""
import ctypes as C
import itertools
import math
import os

import numpy as np

from oracle_util import load_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEXTURED_XML = os.path.join(ROOT, "tests", "data", "xml", "textured_emitter.xml")
QW, OW, NU = 24, 80, 8
OPS = ("spectrum", "kdist", "emit", "emit_direct", "Li", "sense", "sense_direct", "Si")
OP = {n: i for i, n in enumerate(OPS)}
EMIT_SPOT, EMIT_AREA, EMIT_POINT, EMIT_DIRECTIONAL = 0, 1, 2, 3
SENSOR_PERSPECTIVE, SENSOR_VIRTUAL_PLANE = 0, 1
INVALID = 0xFFFFFFFF
EPS32 = 2.0 ** -23
BAND_ULPS = 8
F32_BELOW_1 = float(np.nextafter(np.float32(1), np.float32(0)))

V3 = ("<f4", 3)
EMITTER_DTYPE = np.dtype([("type", "<i4"), ("spectrum", "<i4"), ("scale", "<f4"), ("pse_scale", "<f4"), ("position", *V3), ("t", *V3), ("b", *V3),
                          ("n", *V3), ("cutoff", "<f4"), ("falloff", "<f4"), ("cos_cutoff", "<f4"), ("cos_falloff", "<f4"), ("recp_cutoff_range", "<f4"),
                          ("max_tan_alpha", "<f4"), ("extent", "<f4"), ("target_radius", "<f4"), ("target_area", "<f4"), ("far_dist", "<f4"),
                          ("tan_alpha_at_target", "<f4"), ("shape", "<i4"), ("radiance_tex", "<i4"), ("tab", "<u4"), ("tab_words", "<u4"),
                          ("select_pmf", "<f4"), ("k_dist", "<i4")])
SENSOR_DTYPE = np.dtype([("type", "<i4"), ("width", "<u4"), ("height", "<u4"), ("channels", "<u4"), ("polarimetric", "<u4"), ("ray_trace_only", "<u4"),
                         ("rfilter_sigma", "<f4"), ("rf_radius", "<i4"), ("flip_x", "<u4"), ("flip_y", "<u4"), ("response_spec", "<i4", 4),
                         ("position", *V3), ("t", *V3), ("b", *V3), ("n", *V3), ("inv_cam", "<f4", 16), ("cam", "<f4", 16), ("ddir_dx", *V3),
                         ("ddir_dy", *V3), ("sensor_area", "<f4"), ("element_extent_x", "<f4"), ("sourcing_tan_alpha", "<f4"), ("pse_scale", "<f4"),
                         ("origin", *V3), ("extent", "<f4", 2), ("element_extent", "<f4", 2), ("recp_area", "<f4"), ("requested_tan_alpha", "<f4")])
KDIST_DTYPE = np.dtype([("discrete", "<i4"), ("kmin", "<f4"), ("kmax", "<f4"), ("offset", "<u4"), ("count", "<u4")])
SHAPE_DTYPE = np.dtype([("material", "<i4"), ("emitter", "<i4"), ("surface_area", "<f4"), ("recp_surface_area", "<f4"), ("tri_offset", "<u4"),
                        ("tri_count", "<u4")])

# output words (wt/sources_probe.h)
W_A, W_HAS_SURFACE, W_DRAWS, W_U, W_S, W_BEAM, W_SURF, W_ELEM = 0, 1, 2, 3, 11, 16, 59, 71
B_O, B_D, B_X, B_X0, B_TA, B_E, B_OOE, B_ZAPEX, B_K, B_SID, B_TRANSPORT, B_FRAME, B_SCALE, B_RAD = 0, 3, 6, 9, 10, 11, 12, 13, 14, 15, 16, 17, 26, 27
# float fields compared against f64: name -> output word indices
FIELDS = {"s0": [W_S], "s1": [W_S + 1], "s2": [W_S + 2], "s3": [W_S + 3], "s4": [W_S + 4],
          "beam.o": [W_BEAM + B_O + i for i in range(3)], "beam.d": [W_BEAM + B_D + i for i in range(3)], "beam.x0": [W_BEAM + B_X0],
          "beam.tan_alpha": [W_BEAM + B_TA], "beam.z_apex": [W_BEAM + B_ZAPEX], "beam.k": [W_BEAM + B_K], "beam.scale": [W_BEAM + B_SCALE],
          "beam.rad0": [W_BEAM + B_RAD], "surf.wp": [W_SURF + i for i in range(3)], "surf.n": [W_SURF + 3 + i for i in range(3)],
          "surf.uv": [W_SURF + 6, W_SURF + 7], "surf.bary": [W_SURF + 8, W_SURF + 9], "elem.offset": [W_ELEM + 2, W_ELEM + 3]}
# discrete words compared against f64
DISCRETE = {"A": W_A, "has_surface": W_HAS_SURFACE, "draws": W_DRAWS, "transport": W_BEAM + B_TRANSPORT, "tuid": W_SURF + 10, "shape": W_SURF + 11,
            "elem.x": W_ELEM, "elem.y": W_ELEM + 1}
# the scalar words that are tagged densities, per op (their sign is the tag)
TAGGED = {"spectrum": ["s2"], "kdist": ["s1"], "emit": ["s0", "s1"], "emit_direct": ["s1"], "sense": ["s0", "s1"], "sense_direct": ["s1"]}
DISCRETE_WORDS = sorted(set(DISCRETE.values()))
FLOAT_WORDS = [w for w in range(W_S, OW) if w not in DISCRETE_WORDS]


def libm_words(op, etype, stype):
    """The float words of an op's output behind a libm call (sinf, cosf, acosf; ceilf(sqrtf()) and roundf only pick table cells): the list at
    the top of wt/sources_probe.h.  Every other float word is bit-identical between the device and the checker."""
    beam = lambda *parts: [W_BEAM + p + i for p, n in parts for i in range(n)]
    direction = [(B_D, 3), (B_X, 3), (B_FRAME, 9)]
    if op == "emit":
        if etype == EMIT_SPOT:      # uniform_cone (cosf, sinf), spot_falloff (acosf)
            return beam(*direction, (B_RAD, 4))
        if etype == EMIT_POINT:     # uniform_sphere (cosf, sinf)
            return beam(*direction)
        if etype == EMIT_DIRECTIONAL:   # concentric_disk (cosf, sinf): the target point
            return beam((B_O, 3))
        return beam(*direction, (B_RAD, 4)) + [W_S + 1, W_S + 3]      # cosine_hemisphere: d, dn -> dpd, the beam's weight
    if op == "emit_direct" and etype == EMIT_SPOT:
        return beam((B_RAD, 4))     # spot_falloff (acosf)
    if op == "sense" and stype == SENSOR_VIRTUAL_PLANE:   # cosine_hemisphere
        return beam(*direction, (B_SCALE, 1)) + [W_S + 1, W_S + 3]
    return []


def _p(a):
    return a.ctypes.data


def f32(x):
    return float(np.float32(x))


def f32bits(x):
    return np.float32(x).view(np.uint32)


def k_of(lam_mm):
    return f32(2 * math.pi / lam_mm)


def oracle_source_queries(sc, q, expect=0):
    lib = load_oracle()
    lib.oracle_source_queries.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    q = np.ascontiguousarray(q, np.uint32)
    assert q.ndim == 2 and q.shape[1] == QW
    out = np.zeros((len(q), OW), np.uint32)
    rc = lib.oracle_source_queries(sc.host_desc(), _p(q), len(q), _p(out))
    assert rc == expect, rc
    return out


class Records:
    """the baked records of a scene, read back through the checker's accessors and widened to f64"""

    def __init__(self, sc):
        self.sc, self.lib, self.h = sc, load_oracle(), sc.host_desc()
        lib = self.lib
        for name in ("oracle_emitter_record", "oracle_kdist_record", "oracle_shape_record"):
            getattr(lib, name).argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
        lib.oracle_sensor_record.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        lib.oracle_kdist_table.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
        lib.oracle_emitter_cdf.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
        lib.oracle_shape_tables.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        lib.oracle_triangle_record.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.oracle_texture_data.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
        lib.oracle_texture_spectral.argtypes = [C.c_void_p, C.c_uint32, C.c_float, C.c_float, C.c_float]
        lib.oracle_texture_spectral.restype = C.c_float
        lib.kat_spectrum.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_void_p]
        lib.kat_spectrum.restype = C.c_float
        self.n_emitters = int(sc.info.n_emitters)
        self.n_tris = int(sc.info.n_tris)
        self.emitters = [self._rec("oracle_emitter_record", EMITTER_DTYPE, i) for i in range(self.n_emitters)]
        s = np.zeros(1, SENSOR_DTYPE)
        assert lib.oracle_sensor_record(self.h, _p(s), SENSOR_DTYPE.itemsize) == 0
        self.sensor = s[0]
        self.emitter_cdf = np.zeros(self.n_emitters + 1, np.float32)
        assert lib.oracle_emitter_cdf(self.h, self.n_emitters + 1, _p(self.emitter_cdf)) == 0
        self.kdists = []
        for i in range(self.n_emitters):
            d = self._rec("oracle_kdist_record", KDIST_DTYPE, i)
            n = 0 if d["discrete"] else 2 * int(d["count"])
            tab = np.zeros(max(n, 1), np.float32)
            assert lib.oracle_kdist_table(self.h, i, n, _p(tab)) == 0
            self.kdists.append((d, tab[:n // 2].copy(), tab[n // 2:n].copy()))
        self._shapes, self._tris, self._tabs = {}, {}, {}

    def _rec(self, fn, dtype, i):
        r = np.zeros(1, dtype)
        assert getattr(self.lib, fn)(self.h, i, _p(r), dtype.itemsize) == 0, (fn, i)
        return r[0]

    def shape(self, i):
        if i not in self._shapes:
            sh = self._rec("oracle_shape_record", SHAPE_DTYPE, i)
            cdf, tuid = np.zeros(int(sh["tri_count"]) + 1, np.float32), np.zeros(int(sh["tri_count"]), np.uint32)
            assert self.lib.oracle_shape_tables(self.h, i, _p(cdf), _p(tuid)) == 0
            self._shapes[i] = (sh, cdf, tuid)
        return self._shapes[i]

    def tri(self, tuid):
        if tuid not in self._tris:
            geo, shade, meta = np.zeros(12, np.float32), np.zeros(19, np.uint32), np.zeros(2, np.uint32)
            assert self.lib.oracle_triangle_record(self.h, tuid, _p(geo), _p(shade), _p(meta)) == 0
            g = geo.astype(np.float64).reshape(4, 3)
            sf = shade.view(np.float32).astype(np.float64)
            self._tris[tuid] = dict(a=g[0], b=g[1], c=g[2], n=g[3], uv=(sf[9:11], sf[11:13], sf[13:15]), has_uv=int(shade[18]), shape=int(meta[0]),
                                    shape_tri=int(meta[1]))
        return self._tris[tuid]

    def table(self, ei):
        """a textured area emitter's texel tables (wt/sources.h: area_table_*): the triangle cdf, per triangle (texels, 1 / texels,
        texel_to_area_density, its cell cdf)"""
        if ei not in self._tabs:
            e = self.emitters[ei]
            w = np.zeros(int(e["tab_words"]), np.float32)
            assert self.lib.oracle_texture_data(self.h, int(e["tab"]), len(w), _p(w)) == 0
            T = int(self.shape(int(e["shape"]))[0]["tri_count"])
            tris = []
            for t in range(T):
                h = w[T + 1 + 4 * t:T + 5 + 4 * t]
                texels, off = int(h[0]), int(h[3])
                tris.append((texels, h[1], h[2], w[off:off + texels * (texels + 1) // 2 + 1]))
            self._tabs[ei] = (w[:T + 1], tris)
        return self._tabs[ei]

    def spectrum(self, sid, k):
        if sid < 0:
            return 1.0
        im = C.c_float(0)
        return float(self.lib.kat_spectrum(self.h, int(sid), float(k), C.byref(im)))

    def radiance_texture(self, tex, uv, k):
        return float(self.lib.oracle_texture_spectral(self.h, int(tex), f32(uv[0]), f32(uv[1]), float(k)))


# ------------------------------------------------------------------------------------------------ decisions
class Decider:
    """Decisions on computed quantities.  `forced`: the branch to take for the i-th decision found in the band (None: the f64 one)."""

    def __init__(self, forced=()):
        self.forced, self.band = list(forced), []

    def _pick(self, natural, other):
        i = len(self.band)
        self.band.append((natural, other))
        return other if i < len(self.forced) and self.forced[i] else natural

    def gt(self, x, thr, scale=None):
        """x > thr"""
        s = max(abs(thr), abs(x)) if scale is None else scale
        r = x > thr
        if abs(x - thr) <= BAND_ULPS * EPS32 * s or (s == 0 and x == thr):
            return self._pick(r, not r)
        return r

    def trunc(self, x):
        """(uint32_t)x of a film coordinate: towards zero, so that -1 < x < 0 is element 0 as well (the reference converts the same way)"""
        return 0 if -1 < x < BAND_ULPS * EPS32 else self.floor(x)

    def floor(self, x):
        n = math.floor(x)
        tol = BAND_ULPS * EPS32 * max(abs(x), 1.0)
        if x - n <= tol:
            return self._pick(n, n - 1)
        if n + 1 - x <= tol:
            return self._pick(n, n + 1)
        return n


# ------------------------------------------------------------------------------------------------ f64 pieces
def _v(x):
    return np.asarray(x, np.float64)


def _norm(v):
    return v / math.sqrt(float(v @ v))


def _frame(r):
    return _v(r["t"]), _v(r["b"]), _v(r["n"])


def _to_world(fr, v):
    return fr[0] * v[0] + fr[1] * v[1] + (fr[2] * v[2] if len(v) > 2 else 0.0)


def _to_local(fr, v):
    return _v([fr[0] @ v, fr[1] @ v, fr[2] @ v])


def icdf(cdf, u):
    """the interval i with cdf[i] <= u < cdf[i + 1] (discrete_distribution_t::icdf): exact on f32 numbers"""
    i = int(np.searchsorted(cdf, np.float32(u), side="right")) - 1
    return min(max(i, 0), len(cdf) - 2)


def concentric_disk(u):
    """sampler.hpp: Shirley's concentric map"""
    ox, oy = 2 * u[0] - 1, 2 * u[1] - 1
    if ox == 0 and oy == 0:
        return _v([0.0, 0.0])
    if abs(ox) > abs(oy):
        r, th = ox, math.pi / 4 * (oy / ox)
    else:
        r, th = oy, math.pi / 2 - math.pi / 4 * (ox / oy)
    return _v([r * math.cos(th), r * math.sin(th)])


def cosine_hemisphere(u):
    d = concentric_disk(u)
    return _v([d[0], d[1], math.sqrt(max(0.0, 1 - d[0] * d[0] - d[1] * d[1]))])


def mub_tan_alpha(length_m, k):
    """beam_geometry.hpp: minimum-uncertainty beam, sqrt(SBP) envelope^2 / (k length)"""
    return 0.5 * 9.0 / (k * length_m * 1000.0) if length_m > 0 else 0.0


def sourced(length, tan_alpha, scale=1.0):
    """a source of `length` and half-angle tan_alpha after phase_space_extent().enlarge(scale): (x0, tan_alpha)"""
    if scale == 1.0:
        return math.sqrt(length * length), tan_alpha
    return math.sqrt(length * length * scale * scale), tan_alpha * scale


def wavelength_m(k):
    return 2 * math.pi / (k * 1000.0)


def emitter_geometry(e, k):
    t = int(e["type"])
    scale = float(e["pse_scale"])
    if t == EMIT_DIRECTIONAL:
        ta = float(e["tan_alpha_at_target"])
        length = 0.5 * 9.0 / (k * 1000.0 * ta) if ta > 0 else 0.0
        return sourced(length, ta, scale)
    length = float(e["extent"]) if (t != EMIT_AREA and e["extent"] > 0) else 10 * wavelength_m(k)
    x0, ta = sourced(length, mub_tan_alpha(length, k), scale)
    if t == EMIT_SPOT:
        ta = min(ta, float(e["max_tan_alpha"]))
    return x0, ta


def sensor_geometry(s, k):
    if int(s["type"]) == SENSOR_PERSPECTIVE:
        return sourced(float(s["element_extent_x"]) * 0.25 * 3.0, float(s["sourcing_tan_alpha"]), float(s["pse_scale"]))
    length = (float(s["element_extent"][0]) + float(s["element_extent"][1])) / 2 * 0.25 * 3.0
    ta = float(s["requested_tan_alpha"])
    return length, (ta if ta >= 0 else mub_tan_alpha(length, k))


def spot_falloff(e, cos_theta):
    if cos_theta <= float(e["cos_cutoff"]):
        return 0.0
    if cos_theta >= float(e["cos_falloff"]):
        return 1.0
    return (float(e["cutoff"]) - math.acos(min(1.0, cos_theta))) * float(e["recp_cutoff_range"])


def spot_falloff_spread(e, cos_theta):
    """the change of the falloff when cos_theta, the argument of acos, moves by one f32 ulp of 1 (what the f32 code cannot resolve: the
    falloff's slope is recp_cutoff_range / sin(theta))"""
    w = spot_falloff(e, cos_theta)
    return max(abs(spot_falloff(e, cos_theta + s * EPS32) - w) for s in (-1, 1))


def kdist_pdf(kd, k):
    d, pdf, _ = kd
    kmin, kmax = float(d["kmin"]), float(d["kmax"])
    if d["discrete"]:
        return 1.0 if k == kmin else 0.0
    if k < kmin or k > kmax:
        return 0.0
    n = int(d["count"])
    x = (k - kmin) / (kmax - kmin) * (n - 1)
    l = min(int(x), n - 2)
    f = x - l
    return float(pdf[l]) * (1 - f) + float(pdf[l + 1]) * f


def kdist_sample(kd, u):
    """the inverse of the piecewise-linear density's cdf: in the interval of u, the density is p0 + s t with s = (p1 - p0) / dk, and t solves
    p0 t + s t^2 / 2 = u - cdf[i]: t = 2 du / (p0 + sqrt(p0^2 + 2 s du)), the root that is stable for either sign of s and reduces to du / p0
    for s = 0.  p0 = 0 with du = 0 (u on the knot that ends a stretch of zero density): the start of the segment."""
    d, pdf, cdf = kd
    if d["discrete"]:
        return float(d["kmin"]), -1.0
    n = int(d["count"])
    i = icdf(cdf, u)
    kmin, kmax = float(d["kmin"]), float(d["kmax"])
    dk = (kmax - kmin) / (n - 1)
    p0, p1 = float(pdf[i]), float(pdf[i + 1])
    du = u - float(cdf[i])
    den = p0 + math.sqrt(max(0.0, p0 * p0 + 2 * (p1 - p0) / dk * du))
    t = min(max(2 * du / den if den > 0 else 0.0, 0.0), dk)
    return kmin + (i * dk + t), p0 + (p1 - p0) * (t / dk)


def surface_at(R, tuid, bary):
    """intersection_surface_t(shape, tri, bary): the point and the uv at the barycentrics"""
    t = R.tri(tuid)
    bz = 1 - bary[0] - bary[1]
    wp = t["a"] * bary[0] + t["b"] * bary[1] + t["c"] * bz
    uv = t["uv"][0] * bary[0] + t["uv"][1] * bary[1] + t["uv"][2] * bz if t["has_uv"] else _v([0.0, 0.0])
    return dict(wp=wp, n=t["n"], uv=uv, bary=_v(bary), tuid=tuid, shape=t["shape"])


def table_cell_ab(cell):
    """row b and column a of cell number `cell` (rows b = 0 .. hold the cells a = 0 .. b): integers, exactly"""
    b = (math.isqrt(8 * cell + 1) - 1) // 2
    return cell - b * (b + 1) // 2, b


def area_table_pdf(R, ei, surf, dec):
    """sampling_data_t::pdf (area.cpp:297-319): the density of the cell that holds the surface's barycentrics.  The reference indexes its
    table with whatever the rounding gives (on a triangle's border: one past a row); wt/sources.h clamps the row into the table and the
    column into the row, a documented deviation, and the clamp below restates THAT, deliberately: on the borders this function pins the
    project's decision, not the reference's undefined read."""
    e = R.emitters[ei]
    if surf["shape"] != int(e["shape"]):
        return 0.0
    tcdf, tris = R.table(ei)
    tid = R.tri(surf["tuid"])["shape_tri"]
    texels, _, dens, cdf = tris[tid]
    if texels == 0:
        return 0.0
    # round(x - .5) = floor(x) away from the integers; the cells are clamped into the table
    fa = dec.floor(float(surf["bary"][0]) * texels)
    fb = dec.floor((1 - float(surf["bary"][1])) * texels)
    b = min(max(fb, 0), texels - 1)
    a = min(max(fa, 0), b)
    cell = b * (b + 1) // 2 + a
    return (float(tcdf[tid + 1]) - float(tcdf[tid])) * (float(cdf[cell + 1]) - float(cdf[cell])) * float(dens)


def area_sample_position(R, ei, u, dec):
    """-> (surface, ppd, uniforms used).  shape_t::sample_position (shape.cpp) resp. sampling_data_t::sample (area.cpp)"""
    e = R.emitters[ei]
    sh, cdf, tuids = R.shape(int(e["shape"]))
    if e["radiance_tex"] > 0:
        tcdf, tris = R.table(ei)
        tid = icdf(tcdf, u[0])
        tpdf = float(tcdf[tid + 1]) - float(tcdf[tid])
        texels, step, dens, ccdf = tris[tid]
        cell = icdf(ccdf, u[1])
        cpdf = float(ccdf[cell + 1]) - float(ccdf[cell])
        a, b = table_cell_ab(cell)
        step = float(step)
        alpha = min(max(a * step + u[2] * step, 0.0), 1.0)
        beta = min(max(1 - (b * step + u[3] * step), 0.0), 1 - alpha)
        return surface_at(R, int(tuids[tid]), (alpha, beta)), tpdf * cpdf * float(dens), 4
    tid = icdf(cdf, u[2])
    bary = (u[0], u[1])
    if dec.gt(u[0] + u[1], 1.0):
        bary = (1 - u[0], 1 - u[1])
    return surface_at(R, int(tuids[tid]), bary), float(sh["recp_surface_area"]), 3


def area_radiance(R, e, surf, k):
    if e["radiance_tex"] > 0:
        return float(e["scale"]) * R.radiance_texture(int(e["radiance_tex"]) - 1, surf["uv"], k)
    return R.spectrum(int(e["spectrum"]), k) * float(e["scale"])


def _beam(o, d, geom, k, transport, rad0=None, scale=None):
    x0, ta = geom
    return {"beam.o": _v(o), "beam.d": _v(d), "beam.x0": [x0], "beam.tan_alpha": [ta], "beam.z_apex": [(-x0 / ta) if (x0 != 0 or ta != 0) else -math.inf],
            "beam.k": [k], "beam.scale": [1.0 if scale is None else scale], "beam.rad0": [1.0 if rad0 is None else rad0], "transport": transport}


def _surf(s):
    return {"surf.wp": s["wp"], "surf.n": s["n"], "surf.uv": s["uv"], "surf.bary": s["bary"], "tuid": s["tuid"], "shape": s["shape"], "has_surface": 1}


def _dummy(n, p):
    return {"surf.wp": _v(p), "surf.n": _v(n), "surf.uv": _v([0.0, 0.0]), "surf.bary": _v([-1.0, -1.0]), "tuid": INVALID, "shape": INVALID, "has_surface": 1}


def emitter_sample_direct(R, ei, wp, k, u, dec):
    """-> (outputs, uniforms used).  spot.cpp / point.cpp / directional.cpp / area.cpp: sample_direct"""
    e = R.emitters[ei]
    t = int(e["type"])
    I = R.spectrum(int(e["spectrum"]), k) * float(e["scale"])
    geom = emitter_geometry(e, k)
    pos, fr = _v(e["position"]), _frame(e)
    if t in (EMIT_SPOT, EMIT_POINT):
        dl = wp - pos
        d2 = float(dl @ dl)
        d = dl / math.sqrt(d2)
        w = spot_falloff(e, float(_to_local(fr, d)[2])) if t == EMIT_SPOT else 1.0
        extra = {"beam.rad0": I * spot_falloff_spread(e, float(_to_local(fr, d)[2])) / d2} if t == EMIT_SPOT else {}
        return dict(_beam(pos, d, geom, k, 0, rad0=I * w / d2), s1=[-1.0], has_surface=0, extra_spread=extra), 0
    if t == EMIT_DIRECTIONAL:
        l = _to_local(fr, wp - pos)
        r = float(e["target_radius"])
        inside = not dec.gt(l[0] * l[0] + l[1] * l[1], r * r)
        target = pos + _to_world(fr, l[:2])
        return dict(_beam(target + float(e["far_dist"]) * fr[2], -fr[2], geom, k, 0, rad0=I if inside else 0.0), s1=[-1.0], has_surface=0), 0
    surf, ppd, used = area_sample_position(R, ei, u, dec)
    if e["radiance_tex"] > 0:
        ppd = area_table_pdf(R, ei, surf, dec)      # pdf_direct evaluates pdf_position at the sampled surface
    dl = wp - surf["wp"]
    d = _norm(dl)
    dn = float(d @ surf["n"])
    front = dec.gt(dn, 0.0, scale=1.0)
    dn = max(dn, 1e-300) if front else dn       # (a branch forced inside the band)
    dpd = ppd * float(dl @ dl) / dn if front else 0.0
    rad = area_radiance(R, e, surf, k) * max(0.0, dn) / dpd if dpd > 0 else 0.0
    return dict(_beam(surf["wp"], d, geom, k, 0, rad0=rad), s1=[dpd], **_surf(surf)), used


def f64_query(R, q, u, forced=()):
    """the f64 outputs of one query: {field or discrete word: value}, the Decider (its band list)"""
    dec = Decider(forced)
    name = OPS[int(q[0])]
    i0, i1 = int(q[1]), int(q[2])
    fl = q[3:15].view(np.float32).astype(np.float64)
    k, p, d, bary, ux, rng = float(fl[0]), fl[1:4], fl[4:7], fl[7:9], float(fl[9]), (float(fl[10]), float(fl[11]))
    u = [float(x) for x in u]
    s = R.sensor
    o = {"draws": 0}
    if name == "spectrum":
        ei = icdf(R.emitter_cdf, u[0])
        kk, wpd = kdist_sample(R.kdists[ei], u[1])
        o.update(A=ei, s0=[float(R.emitters[ei]["select_pmf"])], s1=[kk], s2=[wpd], draws=2,
                 s3=[sum(float(R.emitters[i]["select_pmf"]) * kdist_pdf(R.kdists[i], k) for i in range(R.n_emitters))])
    elif name == "kdist":
        kk, wpd = kdist_sample(R.kdists[i0], ux)
        # the density at the sampled k, evaluated at the k the f32 code returns (an input of kdist_pdf), is checked as a property
        o.update(s0=[kk], s1=[wpd], s2=[kdist_pdf(R.kdists[i0], k)], s3=[abs(wpd) if R.kdists[i0][0]["discrete"] else wpd])
        dd, pdf, _ = R.kdists[i0]
        if not dd["discrete"]:      # s3 is kdist_pdf at the ROUNDED k: the density's steepest slope x one ulp of k
            dk = (float(dd["kmax"]) - float(dd["kmin"])) / (int(dd["count"]) - 1)
            j = min(max(int((kk - float(dd["kmin"])) / dk), 1), int(dd["count"]) - 3)
            slope = max(abs(float(pdf[m + 1]) - float(pdf[m])) for m in (j - 1, j, j + 1)) / dk
            o["extra_spread"] = {"s3": slope * EPS32 * kk}
    elif name == "emit":
        e = R.emitters[i0]
        t = int(e["type"])
        I = R.spectrum(int(e["spectrum"]), k) * float(e["scale"])
        geom = emitter_geometry(e, k)
        pos, fr = _v(e["position"]), _frame(e)
        if t == EMIT_SPOT:
            cc = float(e["cos_cutoff"])
            sa = 2 * math.pi * (1 - cc)
            cos_t = 1 + u[0] * (cc - 1)
            sin_t = math.sqrt(max(0.0, 1 - cos_t * cos_t))
            phi = 2 * math.pi * u[1]
            lw = _v([math.cos(phi) * sin_t, math.sin(phi) * sin_t, cos_t])
            dpd = 1 / sa
            o.update(_beam(pos, _to_world(fr, lw), geom, k, 0, rad0=I * spot_falloff(e, cos_t) / dpd), s0=[-1.0], s1=[dpd], s2=[-1.0], s3=[dpd],
                     has_surface=0, draws=2, extra_spread={"beam.rad0": I * spot_falloff_spread(e, cos_t) / dpd})
        elif t == EMIT_DIRECTIONAL:
            pt = concentric_disk(u[:2]) * float(e["target_radius"])
            wp = pos + _to_world(fr, pt)
            area = float(e["target_area"])
            o.update(_beam(wp + float(e["far_dist"]) * fr[2], -fr[2], geom, k, 0, rad0=I * area), s0=[1 / area], s1=[-1.0], s2=[0.0], s3=[-1.0],
                     has_surface=0, draws=2)
        elif t == EMIT_POINT:
            z = 1 - 2 * u[0]
            rr = math.sqrt(max(0.0, 1 - z * z))
            phi = 2 * math.pi * u[1]
            o.update(_beam(pos, _v([rr * math.cos(phi), rr * math.sin(phi), z]), geom, k, 0, rad0=I * 4 * math.pi), s0=[-1.0], s1=[1 / (4 * math.pi)],
                     s2=[-1.0], s3=[1 / (4 * math.pi)], has_surface=0, draws=2)
        else:
            surf, ppd, used = area_sample_position(R, i0, u, dec)
            dl = cosine_hemisphere(u[used:used + 2])
            dn = float(dl[2])
            n = surf["n"]
            dpd = dn / math.pi
            live = dec.gt(dn * dn, 0.0, scale=1.0) and ppd > 0
            rad = area_radiance(R, e, surf, k) * math.pi / ppd if live else 0.0     # radiance dn / (dn / pi ppd)
            # the direction in the world: the tangent frame of the surface is not restated; d.n = dn and |d| = 1 are (properties)
            o.update(_beam(surf["wp"], [math.nan] * 3, geom, k, 0, rad0=rad), s0=[ppd], s1=[dpd], s3=[dpd], **_surf(surf), draws=used + 2)
            o["s2"] = [area_table_pdf(R, i0, surf, dec) if e["radiance_tex"] > 0 else float(R.shape(int(e["shape"]))[0]["recp_surface_area"])]
            o["dn"] = dn
            del n
    elif name == "emit_direct":
        ei = icdf(R.emitter_cdf, u[0])
        r, used = emitter_sample_direct(R, ei, p, k, u[1:], dec)
        pmf = float(R.emitters[ei]["select_pmf"])
        r["beam.rad0"] = [r["beam.rad0"][0] / pmf]
        r["extra_spread"] = {f: v / pmf for f, v in r.get("extra_spread", {}).items()}
        o.update(r, A=ei, s0=[pmf], draws=1 + used)
    elif name == "Li":
        e = R.emitters[i0]
        surf = surface_at(R, i1, bary)
        L = 0.0
        if int(e["type"]) == EMIT_AREA:
            dn = float(-d @ surf["n"])
            if dec.gt(dn, 0.0, scale=math.sqrt(float(d @ d))):
                L = area_radiance(R, e, surf, k)       # radiance max(0, dn) / dn
        # emitter_pdf_position at the explicit surface: the cell density of a textured emitter, else the shape's uniform density
        t_ = int(e["type"])
        if t_ == EMIT_AREA:
            ppd = area_table_pdf(R, i0, surf, dec) if e["radiance_tex"] > 0 else float(R.shape(int(e["shape"]))[0]["recp_surface_area"])
        else:
            ppd = 0.0 if t_ == EMIT_DIRECTIONAL else -1.0
        o.update(_surf(surf), s0=[L], s1=[0.0], s2=[0.0], s3=[0.0], s4=[ppd])
    elif name == "sense":
        geom = sensor_geometry(s, k)
        fr = _frame(s)
        off = _v([u[0] - .5, u[1] - .5])
        if int(s["type"]) == SENSOR_PERSPECTIVE:
            M = _v(s["inv_cam"]).reshape(4, 4)
            h = M @ _v([i0 + .5, i1 + .5, 1.0, 1.0])
            centre = h[:3] / h[3]
            dl = _norm(centre + off[0] * _v(s["ddir_dx"]) + off[1] * _v(s["ddir_dy"]))
            recp = float(s["sensor_area"]) / (0.01 * 0.01) * dl[2] ** 3
            back = _to_local(fr, _to_world(fr, dl))       # pdf_direction(dir): the baked frame is orthonormal to f32 rounding only
            o.update(_beam(_v(s["position"]), _to_world(fr, dl), geom, k, 1, scale=1.0), s0=[-1.0], s1=[1 / recp], s2=[-1.0],
                     s3=[1 / (float(s["sensor_area"]) / (0.01 * 0.01) * back[2] ** 3)],
                     has_surface=0, draws=2)
        else:
            ee = _v(s["element_extent"])
            pt = _v(s["origin"]) + (i0 + off[0] + .5) * ee[0] * fr[0] + (i1 + off[1] + .5) * ee[1] * fr[1]
            wo = cosine_hemisphere(u[2:4])
            dpd = float(wo[2]) / math.pi
            area = 1 / float(s["recp_area"])
            # Se = 1 / (pi area) max(0, wo.n), times area / dpd
            scale = (1 / math.pi) * float(s["recp_area"]) * float(wo[2]) * area / dpd if dpd > 0 else 0.0
            back = _to_local(fr, _to_world(fr, wo))
            o.update(_beam(pt, _to_world(fr, wo), geom, k, 1, scale=scale), s0=[1 / area], s1=[dpd], s2=[float(s["recp_area"])],
                     s3=[max(float(back[2]), 0.0) / math.pi],
                     **_dummy(fr[2], pt), draws=4)
        o.update({"elem.x": i0, "elem.y": i1, "elem.offset": off})
    elif name == "sense_direct":
        geom = sensor_geometry(s, k)
        fr = _frame(s)
        if int(s["type"]) == SENSOR_PERSPECTIVE:
            dl = p - _v(s["position"])
            d2 = float(dl @ dl)
            wd = dl / math.sqrt(d2)
            loc = _to_local(fr, wd)
            recp = float(s["sensor_area"]) / (0.01 * 0.01) * loc[2] ** 3
            inside = dec.gt(float(loc[2]), 2.0 ** -23, scale=1.0)
            ex = ey = 0
            off = _v([math.nan, math.nan])
            if inside:
                pl = loc / max(abs(loc[2]), 1e-300)
                h = _v(s["cam"]).reshape(4, 4) @ _v([pl[0], pl[1], 1.0, 1.0])
                fp = h[:2] / h[3]
                W, H = int(s["width"]), int(s["height"])
                ex, ey = dec.floor(float(fp[0])), dec.floor(float(fp[1]))
                off = _v([fp[0] - ex - .5, fp[1] - ey - .5])
                inside = 0 <= ex < W and 0 <= ey < H
                if not inside:
                    ex = ey = 0
                    off = _v([math.nan, math.nan])
            o.update(_beam(_v(s["position"]), wd, geom, k, 1, scale=(1 / recp) / d2 if inside else 0.0), s1=[-1.0],
                     s3=[1 / recp if loc[2] > 2.0 ** -23 else 0.0], has_surface=0)
            o.update({"elem.x": ex, "elem.y": ey, "elem.offset": off, "inside": inside, "pdf_z": float(loc[2])})
        else:
            ext, ee = _v(s["extent"]), _v(s["element_extent"])
            spl = _v([u[0] * ext[0], u[1] * ext[1]])
            sp = _v(s["origin"]) + spl[0] * fr[0] + spl[1] * fr[1]
            efp = spl / ee
            ex, ey = dec.floor(float(efp[0])), dec.floor(float(efp[1]))
            dl = p - sp
            d2 = float(dl @ dl)
            wd = dl / math.sqrt(d2)
            z = float(wd @ fr[2])
            front = dec.gt(z, 0.0, scale=1.0)
            z = max(z, 1e-300) if front else z       # (a branch forced inside the band)
            dpd = float(s["recp_area"]) * d2 / z if front else 0.0
            # Se = 1 / (pi area) max(0, z), times 1 / dpd / z
            scale = (1 / math.pi) * float(s["recp_area"]) * max(0.0, z) / dpd / z if front and dpd > 0 else 0.0
            o.update(_beam(sp, wd, geom, k, 1, scale=scale), s1=[dpd], s3=[max(z, 0.0) / math.pi], **_dummy(fr[2], sp), draws=2)
            o.update({"elem.x": ex, "elem.y": ey, "elem.offset": _v([efp[0] - ex - .5, efp[1] - ey - .5])})
    else:       # Si (virtual_plane_sensor.cpp): the central ray against the sensor's rectangle
        o["A"] = 0
        if int(s["type"]) == SENSOR_VIRTUAL_PLANE:
            fr = _frame(s)
            ext, ee, org = _v(s["extent"]), _v(s["element_extent"]), _v(s["origin"])
            dn = float(-d @ fr[2])
            dlen = math.sqrt(float(d @ d))
            if dec.gt(dn, 0.0, scale=dlen) and dn != 0:
                tt = float((org - p) @ fr[2]) / float(d @ fr[2])
                hit = p + tt * d
                lx, ly = float((hit - org) @ fr[0]), float((hit - org) @ fr[1])
                sc_ = max(abs(tt) * dlen, float(np.abs(p).max()), ext.max())
                inside = dec.gt(lx, 0.0, scale=sc_) and dec.gt(ly, 0.0, scale=sc_) and not dec.gt(lx, ext[0], scale=sc_) and \
                    not dec.gt(ly, ext[1], scale=sc_)
                in_range = (dec.gt(tt, rng[0], scale=max(abs(tt), abs(rng[0]))) if math.isfinite(rng[0]) else rng[0] < 0) and \
                    (not dec.gt(tt, rng[1], scale=max(abs(tt), abs(rng[1]))) if math.isfinite(rng[1]) else rng[1] > 0)
                if inside and in_range:
                    efp = _v([lx, ly]) / ee
                    ex, ey = dec.trunc(float(efp[0])), dec.trunc(float(efp[1]))
                    geom = sensor_geometry(s, k)
                    scale = (1 / math.pi) * float(s["recp_area"])       # W max(0, dn) / dn
                    o.update(_beam(hit, -d, geom, k, 1, scale=scale), **_dummy(fr[2], hit), A=1)
                    o.update({"elem.x": ex, "elem.y": ey, "elem.offset": _v([efp[0] - ex - .5, efp[1] - ey - .5])})
                    # the hit point o + t d is rounded to f32 before element_for_position reads it: one ulp of its largest coordinate,
                    # in elements
                    ulp = EPS32 * max(float(np.abs(hit).max()), float(np.abs(p).max()))
                    o["extra_spread"] = {"elem.offset": 2 * ulp / float(ee.min()), "beam.o": ulp, "surf.wp": ulp}
    return o, dec


def f64_vector(o):
    """the float words of an f64 result as one vector [OW] (nan: not restated)"""
    v = np.full(OW, np.nan)
    for name, words in FIELDS.items():
        if name in o:
            v[words] = np.asarray(o[name], np.float64)
    return v


def _perturbed(q, u):
    """the query with its float arguments and the uniforms moved by one f32 ulp, one group at a time"""
    out = []
    for sl in (slice(3, 4), slice(4, 7), slice(7, 10), slice(10, 12), slice(12, 13)):
        if not q[sl].any():
            continue
        for step in (np.float32(np.inf), np.float32(-np.inf)):
            qq = q.copy()
            qq[sl] = np.nextafter(q[sl].view(np.float32), step).view(np.uint32)
            out.append((qq, u))
    if int(q[0]) not in (OP["kdist"], OP["Li"], OP["Si"]):
        for sgn in (1, -1):
            out.append((q, np.clip(np.asarray(u, np.float64) + sgn * 2.0 ** -24, 0.0, F32_BELOW_1)))
    return out


def f64_with_bound(R, q, u, forced=()):
    """(f64 result, value vector [OW], conditioning spread [OW], Decider)"""
    ref, dec = f64_query(R, q, u, forced)
    v0 = f64_vector(ref)
    spread = np.zeros(OW)
    key = lambda o: tuple(o.get(n) for n in DISCRETE)
    for qq, uu in _perturbed(q, u):
        r, _ = f64_query(R, qq, uu, forced)
        if key(r) != key(ref):
            continue
        with np.errstate(invalid="ignore"):
            d = np.abs(f64_vector(r) - v0)
        spread = np.fmax(spread, np.where(np.isnan(d), 0.0, d))
    return ref, v0, spread, dec


# ------------------------------------------------------------------------------------------------ queries
def make_query(op, i0=0, i1=0, k=0.0, p=(0, 0, 0), d=(0, 0, 0), bary=(0, 0), u=0.0, rng=(0.0, np.inf), seed=0x50CE, sample_id=0, stream=0, draw=0):
    q = np.zeros(QW, np.uint32)
    q[0], q[1], q[2] = OP[op], i0, i1
    q[3] = f32bits(k)
    q[4:7] = np.asarray(p, np.float32).view(np.uint32)
    q[7:10] = np.asarray(d, np.float32).view(np.uint32)
    q[10:12] = np.asarray(bary, np.float32).view(np.uint32)
    q[12] = f32bits(u)
    q[13:15] = np.asarray(rng, np.float32).view(np.uint32)
    q[15], q[16] = seed & 0xFFFFFFFF, seed >> 32
    q[17], q[18] = sample_id & 0xFFFFFFFF, sample_id >> 32
    q[19], q[20] = stream, draw
    return q


def _up(x, n=1):
    x = np.float32(x)
    for _ in range(n):
        x = np.nextafter(x, np.float32(np.inf))
    return float(x)


def _dn(x, n=1):
    x = np.float32(x)
    for _ in range(n):
        x = np.nextafter(x, np.float32(-np.inf))
    return float(x)


def _unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def scene_ks(R, rng, n):
    """wavenumbers inside the scene's emitters' distributions (an emitter's spectrum is 0 outside its own)"""
    ks = []
    for d, _, _ in R.kdists:
        lo, hi = float(d["kmin"]), float(d["kmax"] if not d["discrete"] else d["kmin"])
        ks += [f32(lo + (hi - lo) * x) for x in rng.random(n)]
    return ks


def world_box(R):
    """a box around the scene's sources and sensor: where the random world points fall"""
    pts = [_v(e["position"]) for e in R.emitters if int(e["type"]) != EMIT_AREA] + [_v(R.sensor["position"]), _v(R.sensor["origin"])]
    for ei, e in enumerate(R.emitters):
        if int(e["type"]) == EMIT_AREA:
            for t in R.shape(int(e["shape"]))[2][:4]:
                pts.append(R.tri(int(t))["a"])
    pts = np.array(pts)
    c, r = pts.mean(axis=0), max(1.0, float(np.abs(pts - pts.mean(axis=0)).max()))
    return c, 2 * r


def random_set(R, rng, n=360):
    """n queries of every op (that the scene's sensor and emitters support)"""
    qs = []
    c, r = world_box(R)
    s = R.sensor
    W, H = int(s["width"]), int(s["height"])
    ks = scene_ks(R, rng, 8)
    sid = itertools.count()
    kw = lambda: dict(sample_id=next(sid), stream=int(rng.integers(0, 3)), draw=int(rng.integers(0, 16)), seed=int(rng.integers(1, 2 ** 40)))
    pick_k = lambda: ks[int(rng.integers(len(ks)))]
    area = [i for i, e in enumerate(R.emitters) if int(e["type"]) == EMIT_AREA]
    for _ in range(n):
        ei = int(rng.integers(R.n_emitters))
        wp = c + r * (2 * rng.random(3) - 1)
        qs.append(make_query("spectrum", k=pick_k(), **kw()))
        qs.append(make_query("kdist", i0=ei, k=pick_k(), u=f32(rng.random()), **kw()))
        qs.append(make_query("emit", i0=ei, k=pick_k(), **kw()))
        qs.append(make_query("emit_direct", k=pick_k(), p=wp, **kw()))
        qs.append(make_query("sense", i0=int(rng.integers(W)), i1=int(rng.integers(H)), k=pick_k(), **kw()))
        if int(s["type"]) == SENSOR_PERSPECTIVE:   # points in front of the camera, most of them inside its frustum
            fr = _frame(s)
            z = 10 ** rng.uniform(-1, 1)
            lx, ly = (rng.random(2) * 2 - 1) * z * 0.6
            wp = _v(s["position"]) + _to_world(fr, _v([lx, ly, z]))
        qs.append(make_query("sense_direct", k=pick_k(), p=wp, **kw()))
        if area:
            ai = area[int(rng.integers(len(area)))]
            tuids = R.shape(int(R.emitters[ai]["shape"]))[2]
            tu = int(tuids[int(rng.integers(len(tuids)))])
            b = rng.random(2)
            b = 1 - b if b.sum() > 1 else b
            n_ = R.tri(tu)["n"]
            d = _unit(rng)
            d = -d if (d @ n_ > 0) == (rng.random() < .8) else d      # 80 % arrive from the front
            qs.append(make_query("Li", i0=ai, i1=tu, k=pick_k(), p=surface_at(R, tu, b)["wp"] - d, d=d, bary=b, **kw()))
        if int(s["type"]) == SENSOR_VIRTUAL_PLANE:
            fr = _frame(s)
            ext = _v(s["extent"])
            tgt = _v(s["origin"]) + rng.uniform(-.1, 1.1) * ext[0] * fr[0] + rng.uniform(-.1, 1.1) * ext[1] * fr[1]
            d = _unit(rng)
            d = -d if (d @ fr[2] > 0) == (rng.random() < .8) else d
            dist = 10 ** rng.uniform(-2, 1)
            qs.append(make_query("Si", k=pick_k(), p=tgt - dist * d, d=d, **kw()))
    return np.array(qs, np.uint32)


def edge_set(R, rng):
    """the explicit edges of the scene's emitters and sensor (see the module's tests for the list)"""
    qs = []
    s = R.sensor
    W, H = int(s["width"]), int(s["height"])
    ks = scene_ks(R, rng, 2)
    k0 = ks[0]
    sid = itertools.count(1 << 20)
    kw = lambda: dict(sample_id=next(sid), draw=int(rng.integers(0, 16)))
    for ei, e in enumerate(R.emitters):
        d, pdf, cdf = R.kdists[ei]
        t = int(e["type"])
        # kdist: u = 0, the largest f32 below 1, on every cdf knot and its f32 neighbours; the pdf at kmin, kmax, just outside both, on knots
        us = [0.0, F32_BELOW_1] + ([] if d["discrete"] else [x for c in cdf[:-1] for x in (float(c), _up(c), _dn(c)) if 0 <= x < 1])
        kmin, kmax = float(d["kmin"]), float(d["kmax"] if not d["discrete"] else d["kmin"])
        kq = [kmin, kmax, _dn(kmin), _up(kmax), _up(kmin), _dn(kmax)]
        if not d["discrete"]:
            n = int(d["count"])
            kq += [f32(kmin + (kmax - kmin) * j / (n - 1)) for j in range(1, n - 1, max(1, n // 16))]
        # every knot of the scene's first table; of the others every 32nd; the f32 neighbours of every 16th knot asked
        first = ei == next((j for j, kd in enumerate(R.kdists) if not kd[0]["discrete"]), -1)
        if not d["discrete"]:
            knots = np.unique(cdf[cdf < 1])
            knots = knots if first else knots[::32]
            us = [0.0, F32_BELOW_1] + [float(c) for c in knots] + [x for c in knots[::16] for x in (_up(c), _dn(c)) if 0 <= x < 1]
        for j, u in enumerate(us):
            qs.append(make_query("kdist", i0=ei, k=kq[j % len(kq)], u=u))
        for kk in kq:
            qs.append(make_query("kdist", i0=ei, k=kk, u=0.5))
            qs.append(make_query("spectrum", k=kk, **kw()))
        pos, fr = _v(e["position"]), _frame(e)
        # k from 380 nm to 10 GHz: the 10 lambda default extent and the max_tan_alpha clamp (the spectrum may be 0 there: the geometry is not)
        for lam in (380e-6, 550e-6, 2e-3, 1.0, 299.792458 / 60, 299.792458 / 10):
            qs.append(make_query("emit", i0=ei, k=k_of(lam), **kw()))
        if t == EMIT_SPOT:
            # the axis, directions at / one ulp inside / outside cos_cutoff and cos_falloff (the local z they reach is the f32 code's), at
            # distances 1e-4 .. 1e4
            for c in [1.0] + [x for cc in (float(e["cos_cutoff"]), float(e["cos_falloff"])) for x in (cc, _up(cc), _dn(cc), _up(cc, 4), _dn(cc, 4))]:
                for dist in (1e-4, 1e-2, 1.0, 1e2, 1e4):
                    for phi in (0.0, 1.0, 2.5, 4.0):
                        sn = math.sqrt(max(0.0, 1 - c * c))
                        qs.append(make_query("emit_direct", k=k0, p=pos + dist * _to_world(fr, _v([sn * math.cos(phi), sn * math.sin(phi), c])), **kw()))
            # ... and points whose f32 local z (spot_local_z_f32) is bit for bit on, one ulp above and one ulp below cos_cutoff and
            # cos_falloff, found by scanning azimuths and distances
            for thr in (e["cos_cutoff"], e["cos_falloff"]):
                want = {float(thr): 0, float(np.nextafter(thr, np.float32(2))): 0, float(np.nextafter(thr, np.float32(-2))): 0}
                cc = float(thr)
                sn = math.sqrt(max(0.0, 1 - cc * cc))
                for j in range(6000):
                    if min(want.values()) >= 8:
                        break
                    phi, dist = 0.37 * j, 0.5 + 0.013 * j
                    wp = (pos + dist * _to_world(fr, _v([sn * math.cos(phi), sn * math.sin(phi), cc]))).astype(np.float32)
                    z = float(spot_local_z_f32(e, wp))
                    if z in want and want[z] < 8:
                        want[z] += 1
                        for _ in range(4 if R.n_emitters > 1 else 1):      # (the emitter is drawn per query)
                            qs.append(make_query("emit_direct", k=k0, p=wp, **kw()))
        elif t == EMIT_POINT:
            for dist in (1e-4, 1e-2, 1.0, 1e2, 1e4):
                qs.append(make_query("emit_direct", k=k0, p=pos + dist * _unit(rng), **kw()))
        elif t == EMIT_DIRECTIONAL:
            # world points inside, on and outside the target disk's rim
            r = float(e["target_radius"])
            for rr in (0.0, .5 * r, _dn(r, 2), r, _up(r, 2), 1.5 * r):
                for phi in (0.0, 0.7, 2.0, 3.0, 4.4):
                    for h in (0.0, -3.0, 5.0):
                        qs.append(make_query("emit_direct", k=k0, p=pos + _to_world(fr, _v([rr * math.cos(phi), rr * math.sin(phi), h])), **kw()))
        else:
            # barycentrics on the three edges and corners (Li and, for a textured emitter, area_table_pdf through emit_direct / Li's surface);
            # the beam grazing, exactly tangent and from behind
            tuids = R.shape(int(e["shape"]))[2]
            for tu in [int(x) for x in tuids[:2]]:
                tri = R.tri(tu)
                n_ = tri["n"]
                tang = _norm(tri["b"] - tri["a"])
                for b in [(1, 0), (0, 1), (0, 0), (.5, .5), (.5, 0), (0, .5), (.25, .25), (F32_BELOW_1, 0), (1 / 3, 1 / 3),
                          (1 / 12, 1 / 12), (.25, .5), (.5, .25), (1 / 6, 0), (0, 5 / 6)]:      # (and borders of a 12-texel table's cells)
                    for d in (-n_, _norm(-n_ + tang), _norm(-1e-3 * n_ + tang), _norm(-1e-6 * n_ + tang), tang, _norm(1e-6 * n_ + tang), n_):
                        qs.append(make_query("Li", i0=ei, i1=tu, k=k0, p=surface_at(R, tu, b)["wp"] - d, d=d, bary=b, **kw()))
            for _ in range(8):
                qs.append(make_query("emit", i0=ei, k=k0, **kw()))
    # one non-area emitter asked for Li (no radiance)
    if R.n_tris:
        qs.append(make_query("Li", i0=0, i1=0, k=k0, p=(0, 0, 1), d=(0, 0, -1), bary=(.3, .3)))
    fr = _frame(s)
    if int(s["type"]) == SENSOR_PERSPECTIVE:
        pos = _v(s["position"])
        M = _v(s["inv_cam"]).reshape(4, 4)
        def on_film(fx, fy, dist=2.0):
            h = M @ _v([fx, fy, 1.0, 1.0])
            return pos + dist * _to_world(fr, _norm(h[:3] / h[3]))
        for px, py in ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)):
            for _ in range(4):
                qs.append(make_query("sense", i0=px, i1=py, k=k0, **kw()))
        # points that project onto, just inside and just outside each film border, and onto pixel boundaries
        for edge in (0.0, float(W)):
            for dlt in (0.0, 1e-6, -1e-6, 1e-3, -1e-3):
                for other in (.5, H / 2, H - .5):
                    qs.append(make_query("sense_direct", k=k0, p=on_film(edge + dlt, other), **kw()))
                    qs.append(make_query("sense_direct", k=k0, p=on_film(other * W / H, edge * H / W + dlt), **kw()))
        for fx in (1.0, W / 2, W - 1.0):
            qs.append(make_query("sense_direct", k=k0, p=on_film(fx, fx * H / W), **kw()))
        # ... and points whose f32 film coordinate (persp_film_f32) is bit for bit on, one ulp inside and one ulp outside the far borders,
        # and within 1e-5 of the near borders on either side, found by scanning
        for axis, lim in ((0, np.float32(W)), (1, np.float32(H))):
            want = {float(lim): 0, float(np.nextafter(lim, np.float32(0))): 0, float(np.nextafter(lim, np.float32(np.inf))): 0}
            for j in range(12000):
                if min(want.values()) >= 6:
                    break
                other = (0.3 + 0.61 * j) % (H if axis == 0 else W)
                at = float(lim) + (0.0, -1e-6, 2e-6)[j % 3] + (0.0 if j < 600 else 1e-5 * ((j * 7) % 61 - 30))      # (a frame that is not quite orthonormal shifts the film)
                wp = on_film(at, other, 1.0 + 0.0137 * j) if axis == 0 else on_film(other, at, 1.0 + 0.0137 * j)
                v = float(persp_film_f32(s, wp.astype(np.float32))[1 + axis])
                if v in want and want[v] < 6:
                    want[v] += 1
                    qs.append(make_query("sense_direct", k=k0, p=wp, **kw()))
            for j in range(12):
                other = (0.3 + 0.61 * j) % (H if axis == 0 else W)
                for dlt in (2e-6, -2e-6):
                    qs.append(make_query("sense_direct", k=k0, p=on_film(dlt, other) if axis == 0 else on_film(other, dlt), **kw()))
        # behind the camera, and dir_local.z around FLT_EPSILON
        for z in (-1.0, -1e-3, 0.0, .5 * EPS32, _dn(EPS32), EPS32, _up(EPS32), 2 * EPS32, 1e-5):
            for x in (1.0, -3.0):
                qs.append(make_query("sense_direct", k=k0, p=pos + _to_world(fr, _v([x, .3, z * math.hypot(x, .3)])), **kw()))
    else:
        ext, org = _v(s["extent"]), _v(s["origin"])
        for px, py in ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)):
            for _ in range(4):
                qs.append(make_query("sense", i0=px, i1=py, k=k0, **kw()))
                qs.append(make_query("sense_direct", k=k0, p=org + fr[2] * 0.5 + rng.random() * ext[0] * fr[0], **kw()))
        # Si onto each border, each corner and the shared diagonal, from the front, from the back and parallel to the plane
        targets = [(0, .5), (1, .5), (.5, 0), (.5, 1), (0, 0), (1, 0), (0, 1), (1, 1), (.5, .5), (.25, .75), (.75, .25), (.3, .3), (F32_BELOW_1, .5),
                   (.5, F32_BELOW_1), (1 / W, 1 / H), (.5 + .5 / W, .5)]
        for tx, ty in targets:
            tgt = org + tx * ext[0] * fr[0] + ty * ext[1] * fr[1]
            for d in (-fr[2], _norm(-fr[2] + .5 * fr[0]), _norm(-fr[2] - .3 * fr[1] + .2 * fr[0]), fr[2], fr[0]):
                qs.append(make_query("Si", k=k0, p=tgt - 0.7 * d, d=d, **kw()))
        qs.append(make_query("Si", k=k0, p=org + .5 * ext[0] * fr[0] + .5 * ext[1] * fr[1] + fr[2], d=-fr[2], rng=(0.0, 0.5)))      # out of range
        qs.append(make_query("Si", k=k0, p=org + .5 * ext[0] * fr[0] + .5 * ext[1] * fr[1] + fr[2], d=-fr[2], rng=(0.0, 1.0)))      # range.max on the plane
    return np.array(qs, np.uint32)


SCENES = ("cornell_box", "sunlit", "etoile", "double_slits", "bidir_room", "textured_emitter")


def load_scene(Scene, name):
    if name == "textured_emitter":
        return Scene.from_xml(TEXTURED_XML, res=16)
    if name == "bidir_room":
        return Scene(name, res=16, polarimetric=1)
    if name == "cornell_box":
        return Scene(name, res=16, mesh_detail=0, lut=(32, 32))
    return Scene(name, res=16)


def source_sets(Scene, seed=23):
    """[(scene name, Scene, Records, {"random": q, "edge": q})] with a fixed seed"""
    out = []
    for i, name in enumerate(SCENES):
        sc = load_scene(Scene, name)
        R = Records(sc)
        rng = np.random.default_rng(seed + i)
        edge = np.array(list(edge_set(R, rng)) + knot_queries(name, R, scene_ks(R, rng, 1)[0]), np.uint32)
        out.append((name, sc, R, {"random": random_set(R, np.random.default_rng(1000 + seed + i)), "edge": edge}))
    return out


# ------------------------------------------------------------------------------------------------ comparison
def discrete_of(row):
    return {n: int(row[w]) for n, w in DISCRETE.items()}


def _match(ref, row, name):
    """the discrete words of an f64 result against an output row -> list of differing names"""
    bad = []
    for n, w in DISCRETE.items():
        if n in ref and int(ref[n]) & 0xFFFFFFFF != int(row[w]):
            bad.append(n)
    f = row.view(np.float32)
    for n in TAGGED.get(name, []):
        if n in ref and (ref[n][0] < 0) != bool(np.signbit(f[FIELDS[n][0]])) and ref[n][0] != 0:
            bad.append("tag:" + n)
    return bad


def compare_f64(R, q, out, tol, kind):
    """`out` (checker or device) against f64, query by query.  kind "random": a query with a decision in the band is skipped and counted.
    kind "edge": it is compared under the admissible branch whose discrete words equal the output's; no query is skipped.
    -> (worst error per (op, field), band count, failures, per-op query counts)"""
    worst, band, fails, counts = {}, 0, [], {}
    fmax = {}
    f_out = out.view(np.float32).astype(np.float64)
    for name, words in FIELDS.items():
        for op in range(len(OPS)):
            m = q[:, 0] == op
            with np.errstate(invalid="ignore"):
                vals = np.abs(f_out[m][:, words]) if m.any() else np.zeros((0, 1))
            vals = vals[np.isfinite(vals)]
            fmax[(op, name)] = float(vals.max()) if vals.size else 0.0
    for i in range(len(q)):
        op = int(q[i, 0])
        name = OPS[op]
        counts[name] = counts.get(name, 0) + 1
        u = out[i, W_U:W_U + NU].view(np.float32)
        ref, v0, spread, dec = f64_with_bound(R, q[i], u)
        if dec.band:
            band += 1
            if kind == "random":
                continue
            # the branch the f32 code took: the first admissible combination whose discrete words match
            # (flipping one decision can bring further ones into play: six slots.)  Among the admissible branches whose discrete words equal
            # the output's, the one closest in the float words: a decision that shows in no discrete word (which table cell a barycentric
            # on a cell border reads) is compared under the branch the f32 code took as well.
            found, seen = None, set()
            for forced in sorted(itertools.product((False, True), repeat=6), key=sum):
                r2, dec2 = f64_query(R, q[i], u, forced)
                sig = tuple(forced[:len(dec2.band)])
                if sum(forced) > sum(sig) or sig in seen:
                    continue
                seen.add(sig)
                if _match(r2, out[i], name):
                    continue
                r2, v2, s2, _ = f64_with_bound(R, q[i], u, forced)
                e2 = _field_errors(op, r2, v2, s2, f_out[i], fmax)
                if found is None or max(e2.values(), default=0.0) < max(found[1].values(), default=0.0):
                    found = (r2, e2)
                    v0 = v2
            if found is None:
                fails.append((i, name, "no admissible branch matches", discrete_of(out[i])))
                continue
            ref, errs = found
        else:
            bad = _match(ref, out[i], name)
            if bad:
                fails.append((i, name, "discrete", bad, {n: ref.get(n) for n in DISCRETE}, discrete_of(out[i])))
                continue
            errs = _field_errors(op, ref, v0, spread, f_out[i], fmax)
        for fld, e in errs.items():
            key = (name, fld)
            worst[key] = max(worst.get(key, 0.0), e)
            if e > tol.get(key, tol["default"]):
                fails.append((i, name, fld, e, f_out[i][FIELDS[fld]].tolist(), v0[FIELDS[fld]].tolist()))
    return worst, band, fails, counts


def _field_errors(op, ref, v0, spread, got, fmax):
    errs = {}
    for fld, words in FIELDS.items():
        if fld not in ref:
            continue
        r, g, sp = v0[words], got[words], spread[words]
        if np.isnan(r).any():
            continue
        if not np.isfinite(r).all():
            errs[fld] = 0.0 if np.array_equal(r, g) else np.inf
            continue
        if not np.isfinite(g).all():
            errs[fld] = np.inf
            continue
        floor = max(float(np.abs(r).max()), 1e-3 * fmax[(op, fld)], 1e-300)
        errs[fld] = float(np.max(np.maximum(np.abs(g - r) - sp - ref.get("extra_spread", {}).get(fld, 0.0), 0.0)) / floor)
    return errs


def check_properties(R, q, out):
    """identities between an op's own outputs (no tolerance beyond the words' own rounding) -> list of failures"""
    fails = []
    f = out.view(np.float32)
    s = R.sensor
    W, H = int(s["width"]), int(s["height"])
    # how far the baked frames are from orthonormal (f32 rounding of the host's look-at): what to_local(to_world(d)) and |d| = 1 can hold to
    defect = max(float(np.abs(np.array(_frame(r)) @ np.array(_frame(r)).T - np.eye(3)).max()) for r in [s] + list(R.emitters))
    ftol = 4e-6 + 4 * defect
    for i in range(len(q)):
        name = OPS[int(q[i, 0])]
        S = f[i, W_S:W_S + 4]
        bm = f[i, W_BEAM:W_BEAM + 43].astype(np.float64)
        live = bool(bm[B_SCALE] != 0 and bm[B_RAD] != 0)
        if name == "kdist" and S[3] != abs(S[1]):
            # kdist_pdf(sampled k) == wpd: the pdf is piecewise linear and k = kmin + (i dk + t) is rounded: |dpdf| <= |slope| ulp(k)
            d, pdf, _ = R.kdists[int(q[i, 1])]
            slope = 0.0 if d["discrete"] else float(np.abs(np.diff(pdf.astype(np.float64))).max()) / ((float(d["kmax"]) - float(d["kmin"])) / (int(d["count"]) - 1))
            if not abs(float(S[3]) - abs(float(S[1]))) <= 4 * slope * EPS32 * float(d["kmax"]) + 4e-6 * abs(float(S[1])):
                fails.append((i, name, "kdist_pdf(sampled k) != wpd", float(S[3]), float(S[1])))
        if name in ("emit", "sense"):
            directional = name == "emit" and int(R.emitters[int(q[i, 1])]["type"]) == EMIT_DIRECTIONAL
            # (an infinite emitter has no position density: its ppd is that of the target disk, emitter_pdf_position is 0)
            if (S[2] != S[0] and not (directional and S[2] == 0)) or (S[3] != S[1] and abs(float(S[3]) - float(S[1])) > (8 * EPS32 + 4 * defect) * abs(float(S[1]))):
                fails.append((i, name, "pdf at the sample != its ppd / dpd", S.tolist()))
        # vplane_Si on the far border returns element == width (height) with offset -.5, as the reference's element_for_position does: the
        # splat clips it.  Pinned: sense and sense_direct stay inside the film, Si reaches width / height and no further.
        edge = 1 if name == "Si" else 0
        if name in ("sense", "sense_direct", "Si") and live and not (out[i, W_ELEM] < W + edge and out[i, W_ELEM + 1] < H + edge):
            fails.append((i, name, "element outside the film", int(out[i, W_ELEM]), int(out[i, W_ELEM + 1])))
        if name in ("emit", "emit_direct", "sense", "sense_direct") or (name == "Si" and out[i, W_A]):
            d, x = bm[B_D:B_D + 3], bm[B_X:B_X + 3]
            fr = bm[B_FRAME:B_FRAME + 9].reshape(3, 3)
            if not (abs(d @ d - 1) < ftol and abs(x @ x - 1) < ftol and abs(d @ x) < ftol and np.abs(fr[0] - x).max() == 0 and np.abs(fr[2] - d).max() == 0
                    and np.abs(fr[1] - np.cross(d, x)).max() < ftol and bm[B_E] == 1 and bm[B_OOE] == 1):
                fails.append((i, name, "envelope frame", d.tolist(), x.tolist()))
        if name == "emit" and out[i, W_HAS_SURFACE]:
            n = f[i, W_SURF + 3:W_SURF + 6].astype(np.float64)
            dn = float(bm[B_D:B_D + 3] @ n)
            if not abs(dn / math.pi - float(S[1])) <= ftol:
                fails.append((i, name, "dpd != d.n / pi", dn / math.pi, float(S[1])))
    return fails


def sense_roundtrip_queries(R, q, out):
    """for every `sense` query a query that comes back along its beam from 1.5 units away: sense_direct at that point (perspective sensor,
    which projects the point onto the film) resp. Si of a beam from that point (virtual plane).  -> (queries, the rows of `q` they belong to)"""
    f = out.view(np.float32)
    persp = int(R.sensor["type"]) == SENSOR_PERSPECTIVE
    rows, src = [], []
    for i in np.flatnonzero(q[:, 0] == OP["sense"]):
        o, d = f[i, W_BEAM:W_BEAM + 3].astype(np.float64), f[i, W_BEAM + 3:W_BEAM + 6].astype(np.float64)
        if not persp and d @ _v(R.sensor["n"]) < 0.05:      # (a grazing beam: the hit point along it is ill-conditioned)
            continue
        qq = q[i].copy()
        qq[0] = OP["sense_direct"] if persp else OP["Si"]
        qq[1] = qq[2] = 0
        qq[4:7] = (o + 1.5 * d).astype(np.float32).view(np.uint32)
        qq[7:10] = (-d).astype(np.float32).view(np.uint32)
        qq[13:15] = np.asarray([0.0, np.inf], np.float32).view(np.uint32)
        rows.append(qq)
        src.append(i)
    return np.array(rows, np.uint32).reshape(-1, QW), np.array(src, int)


def roundtrip_failures(R, q, out, back_q, back_out, src):
    """the film position (element + .5 + offset) a beam comes back to equals the one `sense` left from, to the rounding of the projection:
    (16 ulp + 4 x the frame's defect) x the film's size, and for the virtual plane the rounding of the far point over the element extent
    -> (that tolerance in elements, failures)"""
    s = R.sensor
    W, H = int(s["width"]), int(s["height"])
    defect = float(np.abs(np.array(_frame(s)) @ np.array(_frame(s)).T - np.eye(3)).max())
    tol = (16 * EPS32 + 4 * defect) * max(W, H)
    if int(s["type"]) == SENSOR_VIRTUAL_PLANE:
        far = float(np.abs(back_q[:, 4:7].view(np.float32)).max()) if len(back_q) else 0.0
        tol += 8 * EPS32 * max(far, 1.0) / float(min(s["element_extent"]))
    fails, fo = [], out.view(np.float32)
    fb = back_out.view(np.float32)
    for j, i in enumerate(src):
        a = np.array([out[i, W_ELEM] + .5 + float(fo[i, W_ELEM + 2]), out[i, W_ELEM + 1] + .5 + float(fo[i, W_ELEM + 3])])
        b = np.array([back_out[j, W_ELEM] + .5 + float(fb[j, W_ELEM + 2]), back_out[j, W_ELEM + 1] + .5 + float(fb[j, W_ELEM + 3])])
        alive = fb[j, W_BEAM + B_SCALE] != 0
        # (a sample within rounding of the film's border may come back just outside it: sense_direct then carries no importance)
        on_border = min(a[0], a[1], W - a[0], H - a[1]) <= tol
        if (not alive and not on_border) or (alive and not np.abs(a - b).max() <= tol):
            fails.append((int(i), a.tolist(), b.tolist(), bool(alive)))
    return tol, fails


def spot_local_z_f32(e, wp):
    """local_wo.z of emitter_sample_direct's spot branch in the f32 arithmetic of the code (no contraction; dot = (x x + y y) + z z): the
    number spot_falloff compares with cos_cutoff, bit for bit"""
    f = np.float32
    dl = np.asarray(wp, f) - e["position"]
    l2 = f(f(dl[0] * dl[0]) + f(dl[1] * dl[1])) + f(dl[2] * dl[2])
    d = dl * np.sqrt(f(1) / f(l2), dtype=f)
    n = e["n"]
    return f(f(f(d[0] * n[0]) + f(d[1] * n[1])) + f(d[2] * n[2]))


def spot_cutoff_rows(R, q, out):
    """emit_direct on a spot: a direction whose f32 local z is <= cos_cutoff carries exactly no intensity (compute_falloff's first branch, at
    the decision the f32 code took) -> (rows with z == cos_cutoff exactly, rows with z <= cos_cutoff, failures); spot_falloff_census
    counts the rows on and one ulp beside both thresholds"""
    n_eq = n_le = 0
    fails = []
    f = out.view(np.float32)
    for i in np.flatnonzero(q[:, 0] == OP["emit_direct"]):
        e = R.emitters[int(out[i, W_A])]
        if int(e["type"]) != EMIT_SPOT:
            continue
        with np.errstate(all="ignore"):
            z = spot_local_z_f32(e, q[i, 4:7].view(np.float32))
        if z <= e["cos_cutoff"]:
            n_le += 1
            n_eq += int(z == e["cos_cutoff"])
            if f[i, W_BEAM + B_RAD] != 0:
                fails.append((int(i), float(z), float(e["cos_cutoff"]), float(f[i, W_BEAM + B_RAD])))
    return n_eq, n_le, fails


def philox_uniform_bits(seed, sample_ids, stream, block):
    """Philox-4x32-10 as the sampler uses it (key = the run seed, counter = (sample id lo, hi, stream, draw / 4)) -> [n, 4] u32: the 24
    bits of the four draws of that block (a uniform is bits x 2^-24)"""
    M0, M1, mask, s32 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0xFFFFFFFF), np.uint64(32)
    sid = np.asarray(sample_ids, np.uint64)
    c0, c1 = sid & mask, sid >> s32
    c2, c3 = np.full_like(sid, stream), np.full_like(sid, block)
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & mask, (p0 >> s32) ^ c3 ^ k1, p0 & mask
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & mask, (k1 + np.uint64(0xBB67AE85)) & mask
    return (np.stack([c0, c1, c2, c3], axis=1) >> np.uint64(8)).astype(np.uint32)


def find_uniforms(seed, bits, n_ids=1 << 25, stream=0):
    """(sample id, draw) pairs of stream `stream` whose uniform is bits x 2^-24, for every value in `bits`: how the constants below were
    found (a scan of n_ids counters, about 10 s per 2^25) -> {bits: [(sample id, draw)]}"""
    want, out = np.asarray(sorted(bits), np.uint32), {}
    for base in range(0, n_ids, 1 << 21):
        b = philox_uniform_bits(seed, np.arange(base, base + (1 << 21), dtype=np.uint64), stream, 0)
        for i, j in zip(*np.nonzero(np.isin(b, want))):
            out.setdefault(int(b[i, j]), []).append((base + int(i), int(j)))
    return out


# (sample id, draw) of seed EDGE_SEED, stream 0, whose uniform is the largest f32 below 1 (find_uniforms(EDGE_SEED, [0xFFFFFF], 1 << 26))
EDGE_SEED = 0x50CE
MAX_UNIFORM_IDS = [(153523, 2), (1494555, 1), (5712082, 1), (7743105, 1), (12053879, 2), (14425581, 0), (16826321, 3), (39126204, 3)]
# (sample id, start draw) whose stream carries a uniform exactly on a cdf knot of the scene's tables, at the position the op reads it: the
# emitter-selection cdf (uniform 0 of spectrum / emit_direct), a plain area emitter's triangle cdf (uniform 2 of emit), a textured emitter's
# triangle cdf (uniform 0 of emit) and cell cdfs (uniform 1 of emit).  Found with find_uniforms on the knots that are multiples of 2^-24;
# knot_census recounts them against the tables as baked, so a table that changes shows up as a failed count, not as a silent miss.
KNOT_IDS = {
    "cornell_box": {"emitter": [(2156583, 0), (8010474, 1), (7742563, 0), (11714292, 2)], "tri": [(266902, 0), (3670246, 1), (4278056, 0), (4290821, 1), (5360955, 0)]},
    "bidir_room": {"emitter": [(6983978, 0), (14605717, 1), (9901395, 2), (4335171, 3)]},
    "textured_emitter": {"tri": [(320153, 0), (3519166, 1), (3714808, 0), (2518866, 2)],
                         "cell": [(7640, 0), (281694, 1), (474907, 2), (730626, 2), (752668, 1), (850329, 2), (253173, 0), (638966, 0), (1832163, 0), (1852492, 2)]},
}


def knot_queries(name, R, k0):
    """the queries of MAX_UNIFORM_IDS and KNOT_IDS for scene `name`"""
    qs = []
    s = R.sensor
    W, H = int(s["width"]), int(s["height"])
    wp = world_box(R)[0] + .37
    for sid, draw in MAX_UNIFORM_IDS:
        for d0 in {draw, max(draw - 1, 0)}:      # the largest uniform as the first and as the second draw of the op
            base = dict(sample_id=sid, seed=EDGE_SEED, draw=d0)
            qs.append(make_query("sense", i0=W - 1, i1=H - 1, k=k0, **base))
            qs.append(make_query("sense_direct", k=k0, p=_v(s["origin"]) + _v(s["position"]) + 2 * _frame(s)[2] + .1, **base))
            qs.append(make_query("emit_direct", k=k0, p=wp, **base))
            qs.append(make_query("spectrum", k=k0, **base))
            qs += [make_query("emit", i0=ei, k=k0, **base) for ei in range(R.n_emitters)]
    ids = KNOT_IDS.get(name, {})
    for sid, draw in ids.get("emitter", []):
        qs.append(make_query("spectrum", k=k0, sample_id=sid, seed=EDGE_SEED, draw=draw))
        qs.append(make_query("emit_direct", k=k0, p=wp, sample_id=sid, seed=EDGE_SEED, draw=draw))
    area = [i for i, e in enumerate(R.emitters) if int(e["type"]) == EMIT_AREA]
    for sid, draw in ids.get("tri", []) + ids.get("cell", []):
        qs += [make_query("emit", i0=ei, k=k0, sample_id=sid, seed=EDGE_SEED, draw=draw) for ei in area]
    return qs


def knot_census(R, q, out):
    """what the edge set really holds, counted from the uniforms the probe copied out and the tables as baked: queries whose first or
    second uniform is the largest f32 below 1 (per op), whose emitter-selection uniform is on a knot of the emitter cdf, emit queries whose
    triangle uniform is on a triangle-cdf knot / whose cell uniform is on a knot of the chosen triangle's cell cdf; kdist queries with u
    on a knot with cdf > 0, in a segment that starts at density 0, and on discrete tables"""
    c = {"max_u": {}, "emitter_knot": 0, "tri_knot": 0, "cell_knot": 0, "kdist_knot": 0, "kdist_p0_zero": 0, "kdist_discrete": 0, "kdist_knots_of_table": 0}
    u = out[:, W_U:W_U + NU].view(np.float32)
    top = np.float32(F32_BELOW_1)
    inner = R.emitter_cdf[1:-1]
    knots0 = None
    for i in range(len(q)):
        name = OPS[int(q[i, 0])]
        if name in ("sense", "sense_direct", "emit", "emit_direct", "spectrum") and (u[i, 0] == top or u[i, 1] == top):
            c["max_u"][name] = c["max_u"].get(name, 0) + 1
        if name in ("spectrum", "emit_direct") and u[i, 0] in inner:
            c["emitter_knot"] += 1
        if name == "emit" and int(R.emitters[int(q[i, 1])]["type"]) == EMIT_AREA:
            ei = int(q[i, 1])
            e = R.emitters[ei]
            if e["radiance_tex"] > 0:
                tcdf, tris = R.table(ei)
                c["tri_knot"] += int(u[i, 0] in tcdf[1:-1])
                c["cell_knot"] += int(u[i, 1] in tris[icdf(tcdf, float(u[i, 0]))][3][1:-1])
            else:
                c["tri_knot"] += int(u[i, 2] in R.shape(int(e["shape"]))[1][1:-1])
        if name == "kdist":
            d, pdf, cdf = R.kdists[int(q[i, 1])]
            ux = q[i, 12:13].view(np.float32)[0]
            if d["discrete"]:
                c["kdist_discrete"] += 1
                continue
            on = ux in cdf and ux > 0
            c["kdist_knot"] += int(on)
            c["kdist_p0_zero"] += int(pdf[icdf(cdf, float(ux))] == 0)
    for ei, (d, pdf, cdf) in enumerate(R.kdists):      # the table whose every knot is asked
        if not d["discrete"]:
            m = (q[:, 0] == OP["kdist"]) & (q[:, 1] == ei)
            asked = set(q[m, 12].tolist())
            c["kdist_knots_of_table"] = max(c["kdist_knots_of_table"], sum(int(int(np.float32(x).view(np.uint32)) in asked) for x in np.unique(cdf) if x < 1))
            c["kdist_table_knots"] = int((np.unique(cdf) < 1).sum())
            break
    return c


def _dot32(a, b):
    f = np.float32
    return f(f(f(a[0] * b[0]) + f(a[1] * b[1])) + f(a[2] * b[2]))


def persp_film_f32(s, wp):
    """sensor_sample_direct's perspective branch in the f32 arithmetic of the code, bit for bit (no contraction, dot = (x x + y y) + z z,
    the matrix rows summed left to right): (dir_local.z, fp.x, fp.y), the numbers its `inside` test compares with 0, width and height"""
    f = np.float32
    with np.errstate(all="ignore"):
        dl = np.asarray(wp, f) - s["position"]
        wd = dl * np.sqrt(f(1) / _dot32(dl, dl), dtype=f)
        loc = np.array([_dot32(wd, s["t"]), _dot32(wd, s["b"]), _dot32(wd, s["n"])], f)
        pl = loc / np.abs(loc[2])
        M = s["cam"]
        row = lambda r: f(f(f(f(M[4 * r] * pl[0]) + f(M[4 * r + 1] * pl[1])) + f(M[4 * r + 2] * f(1))) + f(M[4 * r + 3] * f(1)))
        return loc[2], f(row(0) / row(3)), f(row(1) / row(3))


def film_border_rows(R, q, out):
    """sense_direct on a perspective sensor: the sample carries importance exactly where the f32 numbers of persp_film_f32 say it is inside
    the film (the decision the f32 code took) -> (census: queries with a film coordinate exactly on / one ulp inside / one ulp outside the
    far borders width and height, and within 1e-5 of the near border 0 on either side, and with dir_local.z within 2 ulps of FLT_EPSILON;
    failures)"""
    s = R.sensor
    c = {"on": 0, "ulp_in": 0, "ulp_out": 0, "zero_in": 0, "zero_out": 0, "z_eps": 0}
    fails = []
    if int(s["type"]) != SENSOR_PERSPECTIVE:
        return c, fails
    f = np.float32
    fo = out.view(f)
    eps = f(EPS32)
    for i in np.flatnonzero(q[:, 0] == OP["sense_direct"]):
        z, fx, fy = persp_film_f32(s, q[i, 4:7].view(f))
        W, H = f(s["width"]), f(s["height"])
        inside = bool(z > eps and fx >= 0 and fy >= 0 and fx < W and fy < H)
        if inside != bool(fo[i, W_BEAM + B_SCALE] != 0):
            fails.append((int(i), float(z), float(fx), float(fy), float(fo[i, W_BEAM + B_SCALE])))
        if inside and (int(fx) != int(out[i, W_ELEM]) or int(fy) != int(out[i, W_ELEM + 1])):
            fails.append((int(i), "element", float(fx), float(fy), int(out[i, W_ELEM]), int(out[i, W_ELEM + 1])))
        for v, lim in ((fx, W), (fy, H)):
            c["on"] += int(v == lim)
            c["ulp_in"] += int(v == np.nextafter(lim, f(0)))
            c["ulp_out"] += int(v == np.nextafter(lim, f(np.inf)))
            c["zero_in"] += int(0 <= v < 1e-5)
            c["zero_out"] += int(-1e-5 < v < 0)
        c["z_eps"] += int(abs(float(z) - EPS32) <= 2 * EPS32 * EPS32)
    return c, fails


def spot_falloff_census(R, q, out):
    """emit_direct rows on spots whose f32 local z is exactly on / one ulp above / one ulp below cos_cutoff and cos_falloff"""
    f = np.float32
    c = {k: 0 for k in ("cutoff_on", "cutoff_up", "cutoff_dn", "falloff_on", "falloff_up", "falloff_dn")}
    for i in np.flatnonzero(q[:, 0] == OP["emit_direct"]):
        e = R.emitters[int(out[i, W_A])]
        if int(e["type"]) != EMIT_SPOT:
            continue
        with np.errstate(all="ignore"):
            z = spot_local_z_f32(e, q[i, 4:7].view(f))
        for nm in ("cutoff", "falloff"):
            t = e["cos_" + nm]
            c[nm + "_on"] += int(z == t)
            c[nm + "_up"] += int(z == np.nextafter(t, f(2)))
            c[nm + "_dn"] += int(z == np.nextafter(t, f(-2)))
    return c


def nonfinite_rows(q, out):
    """rows with a float word that is neither finite nor the -inf apex of a ray.  The film offset of a sense_direct sample that carries no
    importance (beam scale 0: outside the film or behind the sensor; every caller drops it) is exempt: for a point in the sensor's plane the
    projection dir / |dir.z| is inf / inf, in the reference as here."""
    f = out.view(np.float32).copy()
    dead = (q[:, 0] == OP["sense_direct"]) & (f[:, W_BEAM + B_SCALE] == 0)
    f[np.ix_(dead, FIELDS["elem.offset"])] = 0
    w = f[:, FLOAT_WORDS]
    return np.flatnonzero(~(np.isfinite(w) | np.isneginf(w)).all(axis=1))
