"""Per-query checks of the material layer (wt/bsdf_probe.h): the CPU checker's entry point oracle_bsdf_queries, the query sets both test files
use, and the f64 reference (oracle/indep/second_source.py, restated from the reference's formulas) with its conditioning.

A query is a material id, wi and wo in the local frame, k, transport, uv and a sampler position; the outputs are material_f, material_pdf,
material_sample (valid, wo, tagged dpd, eta, weighted bsdf M), the reverse density at the sampled wo and the first uniforms of the stream.
The f64 reference replays material_sample's sample map from those uniforms.  Its bound per query is the conditioning of the f64 result: the
largest change of each output when wi, wo, k and the uniforms move by a few f32 ulps (what an f32 evaluation cannot resolve), so that the
same assertion holds at normal incidence and within an ulp of the critical angle."""
import ctypes as C
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "indep"))
import second_source as ss  # noqa: E402

from oracle_util import load_oracle  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XML = os.path.join(ROOT, "tests", "data", "xml", "bsdf_probe.xml")
QW, OW = 18, 48
TRANSPORT_FORWARD, TRANSPORT_BACKWARD = 0, 1
MAT_DIFFUSE, MAT_DIELECTRIC, MAT_SURFACE_SPM, MAT_COMPOSITE, MAT_MASK = 0, 1, 2, 3, 4
PROFILES = {0: "dirac", 1: "fractal", 2: "gaussian"}
# wavelengths of the query sets [mm]: 380 nm, 550 nm, 2 um, 60 GHz, 10 GHz
WAVELENGTHS = {"380nm": 380e-6, "550nm": 550e-6, "2um": 2e-3, "60GHz": 299.792458 / 60, "10GHz": 299.792458 / 10}

MATERIAL_DTYPE = np.dtype([("type", "<i4"), ("two_sided", "<u4"), ("scale", "<f4"), ("refl_spec", "<i4"), ("refl_tex_scale", "<f4"), ("ior_spec", "<i4"),
                           ("ext_ior_spec", "<i4"), ("profile", "<i4"), ("roughness", "<f4"), ("gamma", "<f4"), ("gauss_sigma", "<f4"), ("refl_scale", "<f4"),
                           ("trans_scale", "<f4"), ("n_bins", "<u4"), ("bin_kmin", "<f4", 4), ("bin_kmax", "<f4", 4), ("bin_child", "<i4", 4), ("nested", "<i4"),
                           ("mask_alpha", "<f4"), ("refl_tex", "<u4"), ("mask_tex", "<u4"), ("normal_tex", "<u4"), ("normal_flip", "<u4"), ("scale_spec", "<u4"),
                           ("scale_tex", "<u4"), ("rough_tex", "<u4")])


TEXTURE_DTYPE = np.dtype([("type", "<i4"), ("rgba", "<f4", 4), ("col1", "<i4"), ("col2", "<i4"), ("m", "<f4", 4), ("t", "<f4", 2), ("scale", "<f4"),
                          ("width", "<u4"), ("height", "<u4"), ("channels", "<u4"), ("offset", "<u4"), ("bilinear", "<u4"), ("uwrap", "<u4"), ("vwrap", "<u4")])
TEX_CONSTANT, TEX_CHECKERBOARD, TEX_BITMAP, TEX_FUNCTION = 0, 1, 2, 3
WRAP_BLACK, WRAP_WHITE, WRAP_CLAMP, WRAP_REPEAT, WRAP_MIRROR = 0, 1, 2, 3, 4


def _p(a):
    return a.ctypes.data


def k_of(lam_mm):
    return float(np.float32(2 * math.pi / lam_mm))


def f32bits(x):
    return np.float32(x).view(np.uint32)


def oracle_bsdf_queries(sc, q):
    lib = load_oracle()
    lib.oracle_bsdf_queries.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    q = np.ascontiguousarray(q, np.uint32)
    out = np.zeros((len(q), OW), np.uint32)
    assert lib.oracle_bsdf_queries(sc.host_desc(), _p(q), len(q), _p(out)) == 0
    return out


def material_record(sc, mat):
    lib = load_oracle()
    lib.oracle_material_record.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
    rec = np.zeros(1, MATERIAL_DTYPE)
    assert lib.oracle_material_record(sc.host_desc(), mat, _p(rec), MATERIAL_DTYPE.itemsize) == 0
    return rec[0]


def texture_record(sc, tid):
    lib = load_oracle()
    lib.oracle_texture_record.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
    rec = np.zeros(1, TEXTURE_DTYPE)
    assert lib.oracle_texture_record(sc.host_desc(), tid, _p(rec), TEXTURE_DTYPE.itemsize) == 0
    return rec[0]


def texture_texels(sc, t):
    """a bitmap texture's texels [height, width, channels] (f32)"""
    lib = load_oracle()
    lib.oracle_texture_data.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    n = int(t["width"]) * int(t["height"]) * int(t["channels"])
    out = np.zeros(n, np.float32)
    assert lib.oracle_texture_data(sc.host_desc(), int(t["offset"]), n, _p(out)) == 0
    return out.reshape(int(t["height"]), int(t["width"]), int(t["channels"]))


def _wrap(mode, c, dim):
    """texture2d_storage.hpp:80-97 (the restatement of tests/test_textures.py: test_wrap_modes_and_texel_addressing); -1: outside"""
    if 0 <= c < dim:
        return c
    return {WRAP_BLACK: -1, WRAP_WHITE: -1, WRAP_CLAMP: min(max(c, 0), max(1, dim) - 1), WRAP_REPEAT: c % dim,
            WRAP_MIRROR: (lambda m2: 2 * dim - 1 - m2 if m2 >= dim else m2)(c % (2 * dim))}[mode]


def _roundf(x):
    return math.copysign(math.floor(abs(x) + 0.5), x)


class F64Texture:
    """The luminance textures of a scene (constant, checkerboard, nearest / bilinear bitmap, with their transform and scale wrappers), looked
    up in f64 after the f32 texel addressing (checkerboard.hpp:72-79, texture2d.hpp:233-310, transform.hpp:35-44, scale.hpp:95-97).  The
    texel coordinates are computed in f32, like test_textures.py's restatement: which texel a uv on a texel edge or a wrap seam reads is the
    f32 arithmetic's decision; the values are interpolated in f64."""

    def __init__(self, sc):
        self.sc, self.recs, self.texels = sc, {}, {}

    def rec(self, i):
        if i not in self.recs:
            self.recs[i] = texture_record(self.sc, i)
        return self.recs[i]

    def texel(self, t, tid, x, y):
        x, y = _wrap(int(t["uwrap"]), x, int(t["width"])), _wrap(int(t["vwrap"]), y, int(t["height"]))
        if x < 0 or y < 0:
            return 0.0 if (int(t["uwrap"]) if x < 0 else int(t["vwrap"])) == WRAP_BLACK else 1.0
        if tid not in self.texels:
            self.texels[tid] = texture_texels(self.sc, t)
        return float(self.texels[tid][y, x, 0])

    def value(self, tid, uv):
        f32 = np.float32
        u, v = f32(uv[0]), f32(uv[1])
        scale = 1.0
        for _ in range(4):
            t = self.rec(tid)
            assert int(t["type"]) != TEX_FUNCTION and (int(t["type"]) != TEX_BITMAP or int(t["channels"]) < 3), "luminance textures only"
            u, v = t["m"][0] * u + t["m"][1] * v + t["t"][0], t["m"][2] * u + t["m"][3] * v + t["t"][1]
            scale *= float(t["scale"])
            if int(t["type"]) == TEX_CHECKERBOARD:
                tid = int(t["col1"]) if (int(u) % 2 == int(v) % 2) else int(t["col2"])
                continue
            if int(t["type"]) == TEX_CONSTANT:
                return float(t["rgba"][0]) * scale
            assert int(t["bilinear"]) in (0, 1), "nearest / bilinear bitmaps only"
            x = f32(t["width"]) * u - f32(.5)
            y = f32(t["height"]) * (f32(1) - v) - f32(.5)      # (v is flipped: texture2d.hpp:368)
            if int(t["bilinear"]) == 0:
                r = self.texel(t, tid, int(_roundf(float(x))), int(_roundf(float(y))))
            else:
                ix, iy = int(np.floor(x)), int(np.floor(y))
                fx, fy = float(x - np.floor(x)), float(y - np.floor(y))
                a = self.texel(t, tid, ix, iy) * (1 - fx) + self.texel(t, tid, ix + 1, iy) * fx
                b = self.texel(t, tid, ix, iy + 1) * (1 - fx) + self.texel(t, tid, ix + 1, iy + 1) * fx
                r = a * (1 - fy) + b * fy
            return max(0.0, r) * scale
        return 0.0


def uv_set(sc, tids):
    """uv of the textures `tids`: texel centres, texel edges and wrap seams (and their f32 neighbours) of the finest grid among them (a
    bitmap's texels, a checkerboard's cells after its transform)"""
    n = 1
    for tid in tids:
        seen = [tid]
        while seen:
            t = texture_record(sc, seen.pop())
            cells = max(abs(float(t["m"][0])), abs(float(t["m"][3])), 1.0)
            if int(t["type"]) == TEX_BITMAP:
                n = max(n, int(t["width"]), int(t["height"]))
            elif int(t["type"]) == TEX_CHECKERBOARD:
                n = max(n, int(round(cells)))
                seen += [int(t["col1"]), int(t["col2"])]
    f32 = np.float32
    up = lambda x: float(np.nextafter(f32(x), f32(2)))
    dn = lambda x: float(np.nextafter(f32(x), f32(-1)))
    e = 1.0 / n
    centres = [(.5 * e, .5 * e), ((n - .5) * e, .5 * e), (.5 * e, (n - .5) * e)]
    edges = [(e, .5 * e), (dn(e), .5 * e), (.5 * e, e), (.5 * e, up(e)), (e, e)]
    seams = [(0.0, .5 * e), (dn(0.0), .5 * e), (1.0, .5 * e), (dn(1.0), .5 * e), (up(1.0), (n - .5) * e), (.5 * e, 0.0), (.5 * e, 1.0), (.5 * e, dn(0.0))]
    return centres + edges + seams


def ior_has_transmission_f32(eta_ext, eta_int):
    """IOR_has_transmission (surface_spm.cpp:39) in the f32 arithmetic of material_IOR's complex division (wt/core.h): the decision the f32 code
    takes for a material on the threshold |Im eta|^2 / |eta|^2 = 1e-2"""
    f32 = np.float32
    a, b = (f32(eta_ext.real), f32(eta_ext.imag)), (f32(eta_int.real), f32(eta_int.imag))
    d = b[0] * b[0] + b[1] * b[1]
    re, im = (a[0] * b[0] + a[1] * b[1]) / d, (a[1] * b[0] - a[0] * b[1]) / d
    return bool(abs(im) * abs(im) / (re * re + im * im) <= f32(1e-2))


def at_transmission_threshold(leaf):
    return leaf is not None and leaf["type"] == "spm" and abs(abs(leaf["eta"].imag) ** 2 / abs(leaf["eta"]) ** 2 - 1e-2) <= 1e-6


def spectrum(sc, sid, k):
    """the scene's spectrum value at k (f32: the inputs of the material layer, not part of it)"""
    if sid < 0:
        return 1 + 0j
    lib = load_oracle()
    lib.kat_spectrum.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_void_p]
    lib.kat_spectrum.restype = C.c_float
    im = C.c_float(0)
    re = lib.kat_spectrum(sc.host_desc(), int(sid), float(k), C.byref(im))
    return complex(float(re), float(im.value))


# ------------------------------------------------------------------------------------------------ f64 reference
class F64Material:
    """One material id of a scene, resolved like the reference's wrapper chain: composite (composite.hpp:84-135: the bin [kmin, kmax) that
    holds k, none: no BSDF), mask (mask.cpp:24-92), two_sided (two_sided.cpp:20-55), scale (scale.hpp:78-97), then the leaf."""

    def __init__(self, sc, mat):
        self.sc, self.mat = sc, mat
        self.recs = {}
        self.tex = F64Texture(sc)

    def rec(self, i):
        if i not in self.recs:
            self.recs[i] = material_record(self.sc, i)
        return self.recs[i]

    def textures(self):
        """the texture ids the material's records use"""
        out, todo = set(), [self.mat]
        while todo:
            m = self.rec(todo.pop())
            out |= {int(m[f]) - 1 for f in ("refl_tex", "mask_tex", "scale_tex", "rough_tex") if m[f]}
            if m["type"] == MAT_MASK:
                todo.append(int(m["nested"]))
            elif m["type"] == MAT_COMPOSITE:
                todo += [int(m["bin_child"][b]) for b in range(int(m["n_bins"]))]
        return sorted(out)

    def resolve(self, k, uv=(0.0, 0.0)):
        """-> (leaf dict or None, two_sided, scale, mask alpha or None, mask under two_sided)"""
        m = self.rec(self.mat)
        two, scale, alpha, mask_two = False, 1.0, None, False
        for _ in range(4):
            if m["type"] < MAT_COMPOSITE:
                break
            two |= bool(m["two_sided"])
            scale *= float(m["scale"])
            assert not m["scale_spec"], "spectral scales are not in the query sets"
            if m["scale_tex"]:
                scale *= self.tex.value(int(m["scale_tex"]) - 1, uv)
            if m["type"] == MAT_MASK:
                a = self.tex.value(int(m["mask_tex"]) - 1, uv) if m["mask_tex"] else float(m["mask_alpha"])
                alpha = (1.0 if alpha is None else alpha) * min(1.0, max(0.0, a))
                mask_two = two
                child = int(m["nested"])
            else:
                child = -1
                for b in range(int(m["n_bins"])):
                    if m["bin_kmin"][b] <= np.float32(k) < m["bin_kmax"][b]:
                        child = int(m["bin_child"][b])
                        break
            if child < 0:
                return None, False, 1.0, None, False
            m = self.rec(child)
        assert m["type"] < MAT_COMPOSITE
        assert not m["scale_spec"], "spectral scales are not in the query sets"
        t = int(m["type"])
        leaf = {"type": ("diffuse", "dielectric", "spm")[t], "refl_scale": float(m["refl_scale"]), "trans_scale": float(m["trans_scale"])}
        if m["scale_tex"]:
            scale *= self.tex.value(int(m["scale_tex"]) - 1, uv)
        if t == MAT_DIFFUSE:
            tex = self.tex.value(int(m["refl_tex"]) - 1, uv) if m["refl_tex"] else 1.0
            leaf["refl"] = min(1.0, max(0.0, spectrum(self.sc, m["refl_spec"], k).real * float(m["refl_tex_scale"]) * tex))
        else:
            ext, inner = spectrum(self.sc, m["ext_ior_spec"], k), spectrum(self.sc, m["ior_spec"], k)
            leaf["eta"] = ext / inner
            rough = self.tex.value(int(m["rough_tex"]) - 1, uv) if m["rough_tex"] else float(m["roughness"])
            leaf.update(profile=PROFILES[int(m["profile"])], roughness=rough, gamma=float(m["gamma"]), sigma=float(m["gauss_sigma"]),
                        delta_only_by_mean=bool(m["rough_tex"]))
            if at_transmission_threshold(leaf):
                leaf["has_tr"] = ior_has_transmission_f32(ext, inner)   # on the threshold: the interface the f32 code decided on
        return leaf, two or bool(m["two_sided"]), scale * float(m["scale"]), alpha, mask_two


def _flip(w, z):
    return w if z >= 0 else (w[0], w[1], -w[2])


def f64_query(fm, wi, wo, k, transport, u, uv=(0.0, 0.0)):
    """the f64 outputs of one query: dict f[16], pdf, sample (ss.leaf_sample's dict + null lobe), pdf_rev"""
    leaf, two, scale, alpha, mask_two = fm.resolve(k, uv)
    back = transport == TRANSPORT_BACKWARD
    none = dict(valid=False, wo=(0.0, 0.0, 1.0), dpd=0.0, discrete=False, eta=1.0, M=np.zeros(16), lobe=None, reflection=None, used=0, decisions=[])
    if leaf is None:
        return dict(f=np.zeros(16), pdf=0.0, sample=none, pdf_rev=0.0, leaf=None, cond={"f": 0.0, "p": 0.0, "r": 0.0})

    def f_of(a, b):
        if alpha == 0.0:
            return np.zeros(16)
        if two:
            a, b = _flip(a, a[2]), _flip(b, a[2])
        return ss.leaf_f(leaf, a, b, k, back) * scale * (alpha if alpha is not None else 1.0)

    def pdf_of(a, b, tr):
        if alpha is not None:
            if mask_two:
                a, b = _flip(a, a[2]), _flip(b, a[2])
            if a[2] <= 0 or b[2] <= 0:
                return 0.0
        if two:
            a, b = _flip(a, a[2]), _flip(b, a[2])
        return ss.leaf_pdf(leaf, a, b, k) * (alpha if alpha is not None else 1.0)

    s = None
    nn, ui = 1.0, 0
    if alpha is not None:
        pn = 1.0 if (wi[2] == 0 if mask_two else wi[2] <= 0) else 1 - alpha
        if pn == 1.0 or (pn != 0.0 and u[0] < pn):
            M = np.zeros(16)
            M[[0, 5, 10, 15]] = (1 - alpha) / pn
            s = dict(none, valid=True, wo=(-wi[0], -wi[1], -wi[2]), dpd=-pn, discrete=True, M=M, lobe="null", reflection=False,
                     used=0 if pn == 1.0 else 1, decisions=[] if pn == 1.0 else [(0, pn)])
        else:
            if pn != 0.0:
                ui = 1
            nn = 1 - pn
    if s is None:
        wl = _flip(wi, wi[2]) if two else wi
        s = ss.leaf_sample(leaf, wl, k, back, u[ui:])
        s["used"] += ui
        s["decisions"] = ([(0, 1 - nn)] if ui else []) + [(d + ui if d >= 0 else d, p) for d, p in s["decisions"]]
        if s["valid"]:
            if two:
                s["wo"] = _flip(s["wo"], wi[2])
            s["M"] = s["M"] * scale
            if alpha is not None:
                s["dpd"] *= nn
                s["M"] = s["M"] * (alpha / nn)
    rev = pdf_of(s["wo"], wi, 1 - transport)
    # the reference's (1 - alpha) factor cancels in f32 when alpha -> 1 (long wavelengths, small roughness, grazing light): its relative
    # rounding 2^-24 alpha / (1 - alpha) per query, for f (alpha(wi, wo)), pdf and the sample (alpha(wi, wi)), the reverse pdf
    c = {"f": 0.0, "p": 0.0, "r": 0.0}
    if leaf["type"] == "spm" and leaf["profile"] != "dirac":
        def cond(a, b):
            al = ss.profile_alpha(leaf, a, b, k)
            return 2.0 ** -24 * al / max(1 - al, 1e-300)
        wof = _flip(wo, wi[2]) if two else wo
        awo = wof if wi[2] * wo[2] >= 0 else ss.spm_flip_wo(wof, leaf["eta"].real)
        c = {"f": cond(wi[2], awo[2]), "p": cond(wi[2], wi[2]), "r": cond(s["wo"][2], s["wo"][2])}
    return dict(f=f_of(wi, wo), pdf=pdf_of(wi, wo, transport), sample=s, pdf_rev=rev, leaf=leaf, cond=c)


# ------------------------------------------------------------------------------------------------ queries
def make_query(mat, wi, wo, k, transport, uv=(0.0, 0.0), seed=0x5EED, sample_id=0, stream=1, draw=0):
    q = np.zeros(QW, np.uint32)
    q[0] = mat
    q[1:4] = np.asarray(wi, np.float32).view(np.uint32)
    q[4:7] = np.asarray(wo, np.float32).view(np.uint32)
    q[7] = f32bits(k)
    q[8] = transport
    q[9:11] = np.asarray(uv, np.float32).view(np.uint32)
    q[11], q[12] = seed & 0xFFFFFFFF, seed >> 32
    q[13], q[14] = sample_id & 0xFFFFFFFF, sample_id >> 32
    q[15], q[16] = stream, draw
    return q


def _dir(z, phi):
    z = np.float32(z)
    s = np.float32(math.sqrt(max(0.0, 1.0 - float(z) * float(z))))
    return (np.float32(s * math.cos(phi)), np.float32(s * math.sin(phi)), z)


WI_Z = [1.0, 0.5, 1e-2, 1e-4, 1e-6, 0.0]


def angle_set(rng, eta=None):
    """(wi, wo) pairs: wi.z in WI_Z on both sides (and -0.0), wo the mirror direction, wo.z = 0, the transmitted direction, random directions on
    both sides; with a real eta, wi within a few ulps of the critical angle on both sides of it"""
    pairs = []
    zs = [z for z in WI_Z] + [-z for z in WI_Z if z != 0] + [-0.0]
    if eta is not None and abs(eta) > 0 and eta != 1:
        e = eta if eta > 1 else 1 / eta                    # the TIR side: from the denser medium
        cz = np.float32(math.sqrt(1 - 1 / (e * e)))
        side = -1.0 if eta < 1 else 1.0                    # wi.z > 0 sees eta, wi.z < 0 sees 1 / eta (refract)
        c = cz
        for _ in range(4):
            c = np.nextafter(c, np.float32(0))
        for _ in range(9):
            zs.append(side * float(c))
            c = np.nextafter(c, np.float32(1))
    for z in zs:
        phi = float(rng.uniform(0, 2 * math.pi))
        wi = _dir(z, phi)
        wos = [(-wi[0], -wi[1], wi[2]), (np.float32(math.cos(phi + 1)), np.float32(math.sin(phi + 1)), np.float32(0.0))]
        for _ in range(2):
            wos.append(_dir(rng.uniform(0.02, 1.0) * (1 if rng.random() < .5 else -1), rng.uniform(0, 2 * math.pi)))
        wos.append(_dir(-float(wi[2]) * 0.8, phi + math.pi))
        for wo in wos:
            pairs.append((wi, wo))
    return pairs


def scene_materials(sc):
    return [material_record(sc, i) for i in range(sc.info.n_materials)]


def query_set(sc, mats, ks, rng, transports=(TRANSPORT_FORWARD, TRANSPORT_BACKWARD), n_textured_angles=8):
    """the queries of `mats` (material ids) at wavenumbers `ks` -> (q [n,18] u32, meta list of (mat, k)).  A textured material is queried at
    every uv of uv_set (texel centres, texel edges, wrap seams) with `n_textured_angles` of its (wi, wo) pairs (the grazing ones first);
    the others at uv = (0, 0)."""
    qs, meta = [], []
    for mat in mats:
        fm = F64Material(sc, mat)
        tids = fm.textures()
        uvs = uv_set(sc, tids) if tids else [(0.0, 0.0)]
        for k in ks:
            try:
                leaf = fm.resolve(k)[0]
            except ZeroDivisionError:   # a tabulated IOR outside its table (0 there): not a material-layer query
                continue
            eta = leaf["eta"].real if leaf is not None and "eta" in leaf else None
            pairs = angle_set(rng, eta)
            if tids:
                pairs = sorted(pairs, key=lambda p: abs(float(p[0][2])))[:n_textured_angles // 2] + \
                    [pairs[int(j)] for j in rng.choice(len(pairs), n_textured_angles - n_textured_angles // 2, replace=False)]
            for uv in uvs:
                for wi, wo in pairs:
                    for tr in transports:
                        qs.append(make_query(mat, wi, wo, k, tr, uv=uv, sample_id=len(qs), draw=int(rng.integers(0, 16))))
                        meta.append((mat, k))
    return np.array(qs, np.uint32), meta


def bsdf_sets(Scene, rng):
    """(label, scene, q, meta) of the query sets: the bundled scenes' materials and tests/data/xml/bsdf_probe.xml, k at the five wavelengths
    and, for the composite, on its bin edges"""
    ks = [k_of(l) for l in WAVELENGTHS.values()]
    out = []
    xml = Scene.from_xml(XML)
    out.append(("bsdf_probe", xml, *query_set(xml, range(xml.info.n_materials), ks, rng)))
    cb = Scene("cornell_box", res=8, mesh_detail=0, lut=(32, 32))
    out.append(("cornell_box", cb, *query_set(cb, range(cb.info.n_materials), ks, rng)))
    fs = Scene("furnace_spm", res=8)
    out.append(("furnace_spm", fs, *query_set(fs, range(fs.info.n_materials), ks, rng)))
    for name in ("furnace_wall_mask", "furnace_wall_mask_one"):     # masks of opacity 0.6 and 1 (bsdf_probe.xml: 0)
        fw = Scene(name, res=8)
        out.append((name, fw, *query_set(fw, range(fw.info.n_materials), ks, rng)))
    # textured reflectances and masks (host/scenes.cpp: build_textured): checkerboard, nearest / bilinear bitmaps, the wrap modes
    for name in ("tex_const", "tex_checker", "tex_bitmap", "tex_bilinear_flat", "tex_bilinear_ramp", "tex_mask"):
        tx = Scene(name, res=8)
        out.append((name, tx, *query_set(tx, range(tx.info.n_materials), ks[:3], rng)))
    fc = Scene("furnace_wall_composite", res=8)
    edges = set()
    for i in range(fc.info.n_materials):
        m = material_record(fc, i)
        for b in range(int(m["n_bins"])):
            for e in (m["bin_kmin"][b], m["bin_kmax"][b]):
                if np.isfinite(e) and e > 0:
                    edges.update(float(x) for x in (e, np.nextafter(e, np.float32(0)), np.nextafter(e, np.float32(np.inf))))
    out.append(("furnace_wall_composite", fc, *query_set(fc, range(fc.info.n_materials), sorted(edges) + ks, rng)))
    return out


# ------------------------------------------------------------------------------------------------ outputs
def decode(out):
    """out [n,48] u32 -> dict of arrays"""
    f = out.view(np.float32)
    return {"applies": (out[:, 0] & 1) != 0, "valid": (out[:, 0] & 2) != 0, "f": f[:, 1:17], "pdf": f[:, 17], "wo": f[:, 18:21], "dpd": f[:, 21],
            "eta": f[:, 22], "M": f[:, 23:39], "pdf_rev": f[:, 39], "draws": out[:, 40], "u": f[:, 41:47]}


def lobe_of(wi_z, wo, dpd, valid):
    """the discrete outcome of a sample: (valid, discrete, reflection); a null-lobe pass is discrete and a transmission"""
    if not valid:
        return (False, None, None)
    return (True, bool(np.signbit(np.float32(dpd))), bool(float(wi_z) * float(wo[2]) >= 0) if not (float(wo[2]) == 0) else None)


def _vals(r):
    s = r["sample"]
    return np.concatenate([r["f"], [r["pdf"]], np.asarray(s["wo"], float), [s["dpd"], s["eta"]], s["M"], [r["pdf_rev"]]])


def _uv(q):
    return tuple(float(x) for x in q[9:11].view(np.float32))


def f64_outputs(fm, q, u):
    wi = tuple(float(x) for x in q[1:4].view(np.float32))
    wo = tuple(float(x) for x in q[4:7].view(np.float32))
    k = float(q[7:8].view(np.float32)[0])
    return f64_query(fm, wi, wo, k, int(q[8]), [float(x) for x in u], _uv(q))


def f64_with_bound(fm, q, u, eps=4 * 2.0 ** -24):
    """(reference result, value vector [41], conditioning bound [41]): the spread of the f64 outputs when wi, wo, k and the uniforms move by
    eps relative (a few f32 ulps), for the runs whose discrete outcome does not change"""
    ref = f64_outputs(fm, q, u)
    v0 = _vals(ref)
    spread = np.zeros_like(v0)
    wi = np.array(q[1:4].view(np.float32), float)
    wo = np.array(q[4:7].view(np.float32), float)
    k = float(q[7:8].view(np.float32)[0])
    uu = np.array(u, float)
    perturb = [(wi * (1 + s * eps), wo, k, uu) for s in (-1, 1)] + [(wi, wo * (1 + s * eps), k, uu) for s in (-1, 1)] + \
              [(wi, wo, k * (1 + s * eps), uu) for s in (-1, 1)] + [(wi, wo, k, np.clip(uu + s * 2.0 ** -24, 0, 1 - 2.0 ** -24)) for s in (-1, 1)]
    dsp = {}
    for a, b, kk, us in perturb:
        r = f64_query(fm, tuple(a), tuple(b), kk, int(q[8]), list(us), _uv(q))
        for (i0, p0), (i1, p1) in zip(ref["sample"]["decisions"], r["sample"]["decisions"]):
            if i0 == i1 and i0 >= 0:
                dsp[i0] = max(dsp.get(i0, 0.0), abs(p1 - p0))
        if (r["sample"]["valid"], r["sample"]["discrete"], r["sample"]["reflection"], r["sample"]["lobe"]) != \
                (ref["sample"]["valid"], ref["sample"]["discrete"], ref["sample"]["reflection"], ref["sample"]["lobe"]):
            continue
        with np.errstate(invalid="ignore"):
            d = np.abs(_vals(r) - v0)
        spread = np.maximum(spread, np.where(np.isfinite(d), d, np.inf))
    ref["dspread"] = dsp
    return ref, v0, spread


def in_band(ref, u, rel=1e-4):
    """True where a deciding uniform lies within `rel` of its f64 threshold, or within 16 x the threshold's conditioning spread (near the
    critical angle the Fresnel transmittance moves fast)"""
    return any(i < 0 or abs(float(u[i]) - p) <= rel * max(1e-3, p) + 2.0 ** -23 + 16 * ref.get("dspread", {}).get(i, 0.0)
               for i, p in ref["sample"]["decisions"] if i < len(u))


GRAZING = 1e-3
FIELDS = {"f": slice(0, 16), "pdf": slice(16, 17), "wo": slice(17, 20), "dpd": slice(20, 21), "eta": slice(21, 22), "M": slice(22, 38), "pdf_rev": slice(38, 39)}


def compare_f64(sc, q, out, tol, relfloor=None):
    """The outputs `out` (checker or device, generic form) against the f64 reference, query by query: the discrete outcomes equal outside the
    rounding band; per field the error |got - ref| beyond 16 x the conditioning spread, relative to max(|ref|, 1e-3 of the field's largest
    entry), for the Mueller matrices f and M relative to their largest entry;
    fields where the f64 value is not finite are checked for finiteness only.  A material on IOR_has_transmission's threshold is compared
    under the interface decision of the f32 code (ior_has_transmission_f32).  -> (worst error per field and material kind, band count,
    failures, queries on the transmission threshold)"""
    d = decode(out)
    fms = {}
    worst, band, fails, n_thr = {}, 0, [], 0
    for i in range(len(q)):
        mat = int(q[i, 0])
        fm = fms.setdefault((id(sc), mat), F64Material(sc, mat))
        ref, v0, spread = f64_with_bound(fm, q[i], d["u"][i])
        kind = _kind(ref["leaf"])
        n_thr += int("has_tr" in (ref["leaf"] or {}))
        got_s = lobe_of(q[i, 3:4].view(np.float32)[0], d["wo"][i], d["dpd"][i], d["valid"][i])
        s = ref["sample"]
        ref_s = (s["valid"], s["discrete"] if s["valid"] else None, (s["reflection"] if s["lobe"] != "null" else False) if s["valid"] else None)
        if None in (got_s[2], ref_s[2]):     # a sampled wo.z of exactly 0: reflection / transmission not readable from the output
            got_s, ref_s = got_s[:2], ref_s[:2]
        if got_s != ref_s:
            if in_band(ref, d["u"][i]):
                band += 1
                continue
            fails.append((i, "outcome", got_s, ref_s))
            continue
        if int(d["draws"][i]) != s["used"] and not in_band(ref, d["u"][i]):
            fails.append((i, "draws", int(d["draws"][i]), s["used"]))
        got = np.concatenate([d["f"][i], [d["pdf"][i]], d["wo"][i], [d["dpd"][i], d["eta"][i]], d["M"][i], [d["pdf_rev"][i]]]).astype(float)
        wiz, woz = abs(float(q[i, 3:4].view(np.float32)[0])), abs(float(q[i, 6:7].view(np.float32)[0]))
        for name, sl in FIELDS.items():
            if name in ("wo", "dpd", "eta", "M", "pdf_rev") and not s["valid"]:
                continue
            # grazing directions (|z| < GRAZING): the reference's f32 forms take sqrt(1 - z^2), 1 - wn^2 and acos near +-1 there, which
            # do not resolve z; those values are checked for finiteness (and the discrete outcomes above) only
            if wiz < GRAZING or (name in ("f", "pdf") and woz < GRAZING) or (name == "pdf_rev" and abs(float(s["wo"][2])) < GRAZING):
                continue
            g, r, sp = got[sl], v0[sl], spread[sl]
            if not np.isfinite(r).all() or not np.isfinite(sp).all():
                continue
            scale = max(np.abs(r).max(), 1e-30)
            cnd = ref["cond"]["f" if name == "f" else ("r" if name == "pdf_rev" else "p")]
            err = np.abs(g - r) - 16 * sp - 8 * cnd * np.abs(r)
            # (Mueller matrices relative to their largest entry: an entry like (Rs - Rp) / 2 cancels and carries the rounding of Rs and Rp)
            e = float(np.max(np.maximum(err, 0) / np.maximum(np.abs(r), (1.0 if name in ("f", "M") else 1e-3) * scale)))
            key = (kind, name)
            worst[key] = max(worst.get(key, 0.0), e)
            if e > tol.get((kind.rsplit("_", 1)[0], name), tol.get(name, tol["default"])):
                fails.append((i, name, g.tolist(), r.tolist(), sp.tolist()))
    return worst, band, fails, n_thr


def _kind(leaf):
    if leaf is None:
        return "none"
    if leaf["type"] != "spm":
        return leaf["type"]
    return "spm_" + leaf["profile"] + ("_T" if ss.spm_has_transmission(leaf["eta"], leaf) else "_R")
