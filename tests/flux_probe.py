"""Query sets, decoders and ctypes wrappers of the region power integral's probe (wt/flux_probe.h: oracle_flux_queries on the host,
Scene.flux_queries on the device) and of its f64 reference (oracle/flux64.cpp).  TEST INFRASTRUCTURE ONLY.

Every set is a (queries [n, 20] u32, classes [n] str) pair built from a fixed seed.  The reference reads the f32 words of the query widened
to f64, so that both sides start from the same numbers.  A class is the unit the worst errors are recorded and bounded by
(tests/golden/flux_measured.json: twin/<class> from the CPU checker, device/<class> from the MI355X)."""
import ctypes as C
import json
import math
import os

import numpy as np

import parity
from oracle_util import load_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEASURED = os.path.join(ROOT, "tests", "golden", "flux_measured.json")
RECORD_OUT = os.path.join(os.path.dirname(parity._OUT), "flux_measured.json")   # next to the record of tests/parity.py

OPS = ("gauss", "wavefront", "region_local", "region_tuid")
GAUSS, WAVEFRONT, REGION_LOCAL, REGION_TUID = range(4)
QW, OW = 20, 36
W_FLUX, W_AUX, W_VERTS, W_PROJ = 0, 1, 2, 17
MAJOR_AXIS_TO_Z = 2.0          # wt/cone.h: kMajorAxisToZScale
BEAM_ENVELOPE = 3.0            # wt/beam.h: kBeamEnvelope (envelope = 3 sigma)
GAUSS_SCALES = (0.01, 0.03, 0.06, 0.1, 0.5, 1.5, 3.0, 8.0)
GAUSS_OFFSETS = (0.0, 1.0, 3.0, 5.0)
SWITCH = 0.01                  # wt/gauss.h: the edge-midpoint rule below this largest squared edge


def _p(a):
    return a.ctypes.data


def f32(x):
    return np.asarray(x, np.float32)


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def floats(q):
    """the words of a query / output array as f32 widened to f64"""
    return np.ascontiguousarray(q, np.uint32).view(np.float32).astype(np.float64)


# ------------------------------------------------------------------------------------------------ wrappers
def _lib():
    lib = load_oracle()
    if not getattr(lib, "_flux_ready", False):
        vp, u32, dbl, i32 = C.c_void_p, C.c_uint32, C.c_double, C.c_int
        lib.oracle_flux_queries.argtypes = [vp, vp, u32, vp]
        lib.oracle_region_triangles.argtypes = [vp, vp, u32, u32, vp, vp, vp]
        lib.ref_gauss_triangles.argtypes = [vp, u32, vp]
        lib.ref_gauss_triangles.restype = None
        lib.ref_clip_slab.argtypes = [vp, dbl, dbl, vp]
        lib.ref_region_fluxes.argtypes = [u32] + [vp] * 9
        lib.ref_region_fluxes.restype = None
        lib.ref_region_sum.argtypes = [vp, vp, vp, vp, vp, u32, i32]
        lib.ref_region_sum.restype = dbl
        lib.oracle_triangle_record.argtypes = [vp, u32, vp, vp, vp]
        lib._flux_ready = True
    return lib


def oracle_flux_queries(sc, q, expect=0):
    """the CPU checker's probe_flux (the twin of the device hook)"""
    q = np.ascontiguousarray(q, np.uint32)
    assert q.ndim == 2 and q.shape[1] == QW
    out = np.zeros((len(q), OW), np.uint32)
    rc = _lib().oracle_flux_queries(sc.host_desc(), _p(q), len(q), _p(out))
    assert rc == expect, rc
    return out


def ref_gauss(tris):
    """standard-normal mass of n triangles [n, 6] (f64)"""
    t = np.ascontiguousarray(tris, np.float64).reshape(-1, 6)
    out = np.zeros(len(t))
    _lib().ref_gauss_triangles(_p(t), len(t), _p(out))
    return out


def ref_clip(tri, zmin, zmax):
    """the part of a triangle [3, 3] inside zmin <= z <= zmax (an infinite bound: no plane) -> vertices [m, 3]"""
    t = np.ascontiguousarray(tri, np.float64).reshape(9)
    out = np.zeros(15)
    n = _lib().ref_clip_slab(_p(t), float(zmin), float(zmax), _p(out))
    return out[:3 * n].reshape(n, 3)


def ref_region_fluxes(cones, izr, sigma, tris, nrm, want_front):
    """n triangles, each with a region of its own: cones [n, 11] (o, d, x, tan_alpha, x0), izr [n, 2], sigma [n, 2], tris [n, 9] (world), nrm [n, 3],
    want_front [n] (0 / 1, -1: no facing test) -> flux, facing, polygon vertex count"""
    a = [np.ascontiguousarray(v, np.float64) for v in (cones, izr, sigma, tris, nrm)]
    n = len(a[0])
    wf = np.ascontiguousarray(want_front, np.int32)
    flux, facing, nverts = np.zeros(n), np.zeros(n, np.int32), np.zeros(n, np.int32)
    _lib().ref_region_fluxes(n, *[_p(v) for v in a], _p(wf), _p(flux), _p(facing), _p(nverts))
    return flux, facing, nverts


def ref_region_sum(sc, cone, izr, sigma, ids, want_front):
    cone, izr, sigma = (np.ascontiguousarray(v, np.float64) for v in (cone, izr, sigma))
    ids = np.ascontiguousarray(ids, np.uint32)
    return _lib().ref_region_sum(sc.host_desc(), _p(cone), _p(izr), _p(sigma), _p(ids), len(ids), int(want_front))


def oracle_region_triangles(sc, cones, cap):
    """the checker's unbounded record per cone after the final-slab filter -> (ntris [n], ids [n, cap], rec [n, 16]: o, d, x, tan_alpha, x0, izr,
    sigma, front_face)"""
    cones = np.ascontiguousarray(cones, np.float32)
    n = len(cones)
    ntris, ids, rec = np.zeros(n, np.uint32), np.zeros((n, cap), np.uint32), np.zeros((n, 16), np.float32)
    assert _lib().oracle_region_triangles(sc.host_desc(), _p(cones), n, cap, _p(ntris), _p(ids), _p(rec)) == 0
    return ntris, ids, rec


def triangle_geometry(sc, tuids):
    """a, b, c, n of the scene's triangles [n, 12] as baked (f32)"""
    lib = _lib()
    out = np.zeros((len(tuids), 12), np.float32)
    shade, meta = np.zeros(19, np.uint32), np.zeros(2, np.uint32)
    for i, t in enumerate(tuids):
        assert lib.oracle_triangle_record(sc.host_desc(), int(t), _p(out[i]), _p(shade), _p(meta)) == 0
    return out


# ------------------------------------------------------------------------------------------------ committed measurements
def measured():
    with open(MEASURED) as f:
        return json.load(f)


def recording():
    return bool(os.environ.get("PARITY_RECORD"))


def record(values):
    """PARITY_RECORD=1: merge {label: value} into flux_measured.json in the record directory of tests/parity.py (copied to tests/golden/ by hand and committed with the change)"""
    os.makedirs(os.path.dirname(RECORD_OUT), exist_ok=True)
    try:
        with open(RECORD_OUT) as f:
            rec = json.load(f)
    except (OSError, ValueError):
        rec = {}
    rec.update({k: float(v) for k, v in values.items()})
    with open(RECORD_OUT, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)


# ------------------------------------------------------------------------------------------------ builders
def _unit2(rng, n):
    t = rng.uniform(0, 2 * math.pi, n)
    return np.stack([np.cos(t), np.sin(t)], 1)


def _gauss_rows(tris):
    q = np.zeros((len(tris), QW), np.uint32)
    q[:, 0] = GAUSS
    q[:, 1:7] = bits(np.asarray(tris).reshape(-1, 6))
    return q


def random_canonical_triangles(rng, scale, offset, n):
    """n triangles of the given scale [sigma] centred `offset` sigma off the axis"""
    return (offset * _unit2(rng, n))[:, None, :] + rng.normal(scale=scale, size=(n, 3, 2))


def gauss_set(seed=31, per_class=400):
    """scales x offsets (class gauss_s<scale>), the neighbourhood of the midpoint-rule switch, both orientations, the explicit edges, scale 50"""
    rng = np.random.default_rng(seed)
    qs, cls = [], []

    def add(tris, name):
        rows = _gauss_rows(tris)
        qs.append(rows)
        cls.extend([name] * len(rows))

    for s in GAUSS_SCALES:
        for o in GAUSS_OFFSETS:
            add(random_canonical_triangles(rng, s, o, per_class), f"gauss_s{s:g}")
    # the longest squared edge within 1 % of the switch, on both sides (f32 rounding of the vertices moves it by 1e-7 relative at most)
    for side in (-1.0, 1.0):
        n = 200
        L = np.sqrt(SWITCH * (1 + side * rng.uniform(1e-4, 1e-2, n)))
        a = rng.uniform(0, 3, n)[:, None] * _unit2(rng, n)
        u = _unit2(rng, n)
        b = a + L[:, None] * u
        # the third vertex inside the lens of the two circles of radius 0.9 L: both other edges are shorter
        c = a + 0.5 * L[:, None] * u + (rng.uniform(0.1, 0.6, n) * L)[:, None] * np.stack([-u[:, 1], u[:, 0]], 1)
        add(np.stack([a, b, c], 1), "gauss_switch")
    t = random_canonical_triangles(rng, 1.0, 1.0, 200)
    add(t, "gauss_orient")
    add(t[:, [0, 2, 1]], "gauss_orient")
    edge = []
    # zero area: collinear vertices on lines of dyadic coordinates (area2 is exact), a repeated vertex
    for k0, k1, k2 in ((0, 1, 2), (0, 3, -2), (1, 5, 9), (-4, 0, 4)):
        for base, d in (((0.5, 0.25), (1.0, 2.0)), ((0.0, 0.0), (0.5, -0.25)), ((-1.5, 2.0), (0.0, 1.0)), ((3.0, 1.0), (0.125, 0.0))):
            edge.append([[base[0] + k * d[0], base[1] + k * d[1]] for k in (k0, k1, k2)])
    for a, b in (((0.3, -0.2), (1.1, 0.7)), ((0.0, 0.0), (2.0, 1.0)), ((-3.0, 0.004), (0.02, 0.01))):
        edge += [[a, a, b], [a, b, b], [a, b, a]]
    n_zero = len(edge)
    # an edge whose line passes through the origin exactly (h == 0: axis-parallel and diagonal lines), a vertex at the origin
    for third in ((1.5, 0.7), (-0.3, 2.0), (0.05, -0.04), (6.0, -7.0)):
        edge += [[(0.0, -1.0), (0.0, 2.0), third], [(-0.5, 0.0), (4.0, 0.0), third], [(-1.0, -1.0), (2.5, 2.5), third], [(0.75, -0.75), (-3.0, 3.0), third],
                 [(0.0, 0.0), third, (third[1], -third[0])], [(0.0, 0.0), (0.004 * third[0], 0.004 * third[1]), (-0.003 * third[1], 0.005 * third[0])]]
    # edges at a small distance h from the axis spanning +-20 (the half plane beyond them, to e^-100), in the four directions
    known = {}
    for h in (1e-4, 1e-3, 0.02, 0.1):
        for j in range(4):
            known[len(edge) + j] = 0.5 * math.erfc(float(np.float32(h)) / math.sqrt(2))   # (the query holds h in f32)
        edge += [[(-20.0, h), (20.0, h), (0.0, 15.0)], [(20.0, -h), (-20.0, -h), (0.0, -15.0)], [(h, 20.0), (h, -20.0), (15.0, 0.0)],
                 [(-h, 20.0), (-15.0, 0.0), (-h, -20.0)]]
    # sides that begin beyond s = 8 along their line: the whole side is the closed-form tail
    for h in (0.01, 0.3, 1.0, 2.5):
        edge += [[(h, 9.0), (h, 30.0), (h + 5.0, 20.0)], [(-30.0, -h), (-8.5, -h), (-12.0, h + 3.0)], [(h, 8.25), (h + 0.5, 40.0), (-h - 1.0, 25.0)],
                 [(h, -9.0), (h, 30.0), (h + 40.0, 9.0)]]
    # the known answers of tests/test_kat.py: everything, the half plane, the quadrant, far away, the half plane beyond 0.02
    big = 50.0
    known.update({len(edge): 1.0, len(edge) + 1: 0.5, len(edge) + 2: 0.25, len(edge) + 3: 0.0})
    edge += [[(-big, -big), (big, -big), (0.0, big)], [(0.0, -big), (big, 0.0), (0.0, big)], [(0.0, 0.0), (big, 0.0), (0.0, big)],
             [(10.0, 10.0), (11.0, 10.0), (10.0, 11.0)]]
    add(np.array(edge, np.float64), "gauss_edges")
    for o in GAUSS_OFFSETS:
        add(random_canonical_triangles(rng, 50.0, o, per_class), "gauss_scale50")
    q = np.concatenate(qs)
    first = int(np.nonzero(np.array(cls) == "gauss_edges")[0][0])
    # zero_area: rows whose result is exactly 0; known: {row: closed form} (to the 2e-6 of tests/test_kat.py; the triangles reach 15 .. 50 sigma)
    info = {"zero_area": first + np.arange(n_zero), "known": {first + k: v for k, v in known.items()}}
    return q, np.array(cls), info


def wavefront_set(seed=32, n=2000):
    """sigma ratios 1 .. 100 (either axis the longer one), triangles of every scale of the GAUSS set in metres; sigma.x == 0 or sigma.y == 0"""
    rng = np.random.default_rng(seed)
    sx = 10 ** rng.uniform(-4, -2, n)
    ratio = 10 ** rng.uniform(0, 2, n)
    ratio[:50] = 1.0
    sigma = np.stack([sx, sx / ratio], 1)
    swap = rng.random(n) < 0.5
    sigma[swap] = sigma[swap][:, ::-1]
    scale = np.array(GAUSS_SCALES)[rng.integers(0, len(GAUSS_SCALES), n)]
    offs = np.array(GAUSS_OFFSETS)[rng.integers(0, len(GAUSS_OFFSETS), n)]
    tri = ((offs[:, None] * _unit2(rng, n))[:, None, :] + rng.normal(size=(n, 3, 2)) * scale[:, None, None]) * sigma[:, None, :]
    x = rng.normal(scale=1.5, size=(n, 2)) * sigma
    x[:20] = 0.0
    q = np.zeros((n, QW), np.uint32)
    q[:, 0] = WAVEFRONT
    q[:, 1:3] = bits(sigma)
    q[:, 3:9] = bits(tri.reshape(n, 6))
    q[:, 9:11] = bits(x)
    cls = ["wavefront"] * n
    zero = []
    for sg in ((0.0, 1e-3), (1e-3, 0.0), (0.0, 0.0)):
        for xx in ((0.0, 0.0), (1e-4, 0.0), (0.0, -2e-3), (-0.0, 0.0)):
            r = np.zeros(QW, np.uint32)
            r[0] = WAVEFRONT
            r[1:3] = bits(sg)
            r[3:9] = bits([-1e-3, -1e-3, 2e-3, -1e-3, 0.0, 3e-3])
            r[9:11] = bits(xx)
            zero.append(r)
    q = np.concatenate([q, np.array(zero, np.uint32)])
    cls += ["wavefront_zero_sigma"] * len(zero)
    return q, np.array(cls), {}


ENVELOPES = ("round", "elliptic", "x0_zero", "ray")
REGION_KINDS = ("inside", "cross_min", "cross_max", "cross_both", "outside", "on_min", "on_max", "edge_in_plane")


def _one_over_e(ecc):
    """wt/cone.h: make_cone, in f32"""
    return np.sqrt(np.maximum(np.float32(0), np.float32(1) - f32(ecc) * f32(ecc)), dtype=np.float32)


def region_local_set(seed=33, per_envelope=1000):
    """The four envelope kinds x where the triangle lies against the slab.  The slab is the walk's: [dist, dist + 2 x major axis at dist], sigma =
    axes / 3 (a pure ray has no footprint: its sigma and slab depth are drawn directly).  Triangle sizes 0.03 .. 30 x the footprint."""
    rng = np.random.default_rng(seed)
    rows, cls, kinds = [], [], []
    for env in ENVELOPES:
        for i in range(per_envelope):
            ta = 0.0 if env == "ray" else 10 ** rng.uniform(-3, -0.8)
            x0 = 0.0 if env in ("ray", "x0_zero") else 10 ** rng.uniform(-5.5, -4)
            ecc = rng.uniform(0.3, 0.95) if env == "elliptic" else 0.0
            ta, x0, ecc = np.float32(ta), np.float32(x0), np.float32(ecc)
            dist = np.float32(rng.uniform(0.005, 0.02))
            if env == "ray":
                r = np.float32(10 ** rng.uniform(-5, -3))
            else:
                r = np.float32(ta * dist + x0)                      # cone_axes(dist).x in f32 (-ffp-contract=off: two roundings)
            sigma = f32([r / np.float32(BEAM_ENVELOPE), (r * _one_over_e(ecc)) / np.float32(BEAM_ENVELOPE)])
            zmin, zmax = dist, np.float32(dist + np.float32(MAJOR_AXIS_TO_Z) * r)
            depth = float(zmax) - float(zmin)
            # a vertex ON a plane: 9 per envelope (the count of sub-triangles may differ from the f64 polygon's there; under 1 % of the set)
            kind = REGION_KINDS[5 + i // 3] if i < 9 else REGION_KINDS[(i % 6) % 5]
            size = float(r) * 10 ** rng.uniform(math.log10(0.03), math.log10(30))
            centre = rng.normal(scale=float(r) * 0.7, size=2)
            xy = centre + rng.normal(scale=size, size=(3, 2))
            # every other vertex at least 2e-6 (the slabs are 6e-6 deep at least) from both planes
            inside = lambda m: rng.uniform(float(zmin) + max(2e-6, 1e-3 * depth), float(zmax) - max(2e-6, 1e-3 * depth), m)
            below = lambda m: float(zmin) - 2e-6 - rng.uniform(0.01, 1.5, m) * max(size, depth)
            above = lambda m: float(zmax) + 2e-6 + rng.uniform(0.01, 1.5, m) * max(size, depth)
            if kind == "inside":
                z = inside(3)
            elif kind == "cross_min":
                z = np.concatenate([below(1), inside(1), inside(1) if rng.random() < 0.5 else below(1)])
            elif kind == "cross_max":
                z = np.concatenate([above(1), inside(1), inside(1) if rng.random() < 0.5 else above(1)])
            elif kind == "cross_both":
                z = np.concatenate([below(1), above(1), [inside(1), below(1), above(1)][rng.integers(0, 3)]])
            elif kind == "outside":
                z = below(3) if rng.random() < 0.5 else above(3)
            elif kind == "on_min":
                z = np.concatenate([[float(zmin)], [inside(1), below(1), above(1)][rng.integers(0, 3)], [inside(1), below(1)][rng.integers(0, 2)]])
            elif kind == "on_max":
                z = np.concatenate([[float(zmax)], [inside(1), below(1), above(1)][rng.integers(0, 3)], [inside(1), above(1)][rng.integers(0, 2)]])
            else:
                plane = float(zmin) if rng.random() < 0.5 else float(zmax)
                z = np.concatenate([[plane, plane], [inside(1), below(1), above(1)][rng.integers(0, 3)]])
            perm = rng.permutation(3)
            tri = np.concatenate([xy, np.asarray(z, np.float64).reshape(3, 1)], 1)[perm]
            if env != "ray":   # keep the triangle in front of the apex, where the projection is defined (z tan_alpha + x0 > 0)
                zap = -float(x0) / float(ta)
                tri[:, 2] = np.maximum(tri[:, 2], zap + 0.05 * (float(zmin) - zap))
            q = np.zeros(QW, np.uint32)
            q[0] = REGION_LOCAL
            q[1:4] = bits([ta, x0, ecc])
            q[4:6] = bits([zmin, zmax])
            q[6:8] = bits(sigma)
            q[8:17] = bits(tri.reshape(9))
            rows.append(q)
            cls.append("region_local_" + env)
            kinds.append(kind)
    return np.array(rows, np.uint32), np.array(cls), {"kind": np.array(kinds)}


def _orthogonal(d, rng):
    v = rng.normal(size=3)
    v -= d * np.dot(v, d)
    return v / np.linalg.norm(v)


def region_tuid_set(sc, seed=34, n=3000):
    """cornell_box, mesh_detail 0: random triangles, cones aimed at a point of the triangle from 5 .. 20 mm, the slab around the hit as the walk
    builds it (shifted by up to a slab depth either way, so that the triangle also crosses its planes), both want_front values"""
    rng = np.random.default_rng(seed)
    n_tris = sc.info.n_tris
    tuids = rng.integers(0, n_tris, n)
    geo = triangle_geometry(sc, tuids).astype(np.float64)
    q = np.zeros((n, QW), np.uint32)
    q[:, 0] = REGION_TUID
    for i in range(n):
        a, b, c = geo[i, 0:3], geo[i, 3:6], geo[i, 6:9]
        u, v = rng.random(2)
        if u + v > 1:
            u, v = 1 - u, 1 - v
        ta = np.float32(10 ** rng.uniform(-3, -0.8))
        x0 = np.float32(10 ** rng.uniform(-6, -4))
        ecc = np.float32(rng.uniform(0.3, 0.9) if i % 2 else 0.0)
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        dist = rng.uniform(0.005, 0.02)
        r = float(ta) * dist + float(x0)
        p = a + u * (b - a) + v * (c - a) + _orthogonal(d, rng) * rng.uniform(0, 1.5) * r
        o = p - d * dist
        zmin = np.float32(dist + rng.uniform(-1, 1) * MAJOR_AXIS_TO_Z * r)
        rr = np.float32(ta * zmin + x0)
        zmax = np.float32(zmin + np.float32(MAJOR_AXIS_TO_Z) * rr)
        sigma = f32([rr / np.float32(BEAM_ENVELOPE), (rr * _one_over_e(ecc)) / np.float32(BEAM_ENVELOPE)])
        q[i, 1:4] = bits(o)
        q[i, 4:7] = bits(d)
        q[i, 7:10] = bits(_orthogonal(d, rng))
        q[i, 10:13] = bits([ta, x0, ecc])
        q[i, 13:15] = bits([zmin, zmax])
        q[i, 15:17] = bits(sigma)
        q[i, 17] = tuids[i]
        q[i, 18] = i // 2 % 2
    return q, np.array(["region_tuid"] * n), {}


def cornell(Scene):
    return Scene("cornell_box", res=16, mesh_detail=0, lut=(32, 32))


def flux_sets(Scene):
    """{set name: (q, classes, info)} and the scene the REGION_TUID queries are about (the other ops read no scene record)"""
    sc = cornell(Scene)
    return sc, {"gauss": gauss_set(), "wavefront": wavefront_set(), "region_local": region_local_set(), "region_tuid": region_tuid_set(sc)}


# ------------------------------------------------------------------------------------------------ the f64 reference of a set
def reference(sc, q, out=None):
    """per query: flux (the integral), aux (WAVEFRONT: the intensity), facing and nverts (REGION_*: the f64 facing bit and polygon vertex count;
    -1 elsewhere), band (REGION_TUID: |dot(n, d)|; REGION_LOCAL: the smallest distance of a vertex from a slab plane).
    REGION_TUID: flux_world is the integral from the world-frame triangle, local the f64 beam-frame vertices and local_unit the rounding unit of
    their f32 evaluation (8 x 2^-24 x the L1 norm of vertex - origin: the subtraction, cross(d, x), three products and two sums).  With `out`
    (the probe's output, whose beam-frame vertices are the same bits on the host and on the device) flux is the integral from THOSE vertices:
    a beam 10 um wide 20 mm from its origin turns the 1e-9 m rounding of the f32 frame change into 1e-4 sigma, which is the conditioning of
    the input and not an error of the integral; the frame change is compared on its own (local against out's vertices within local_unit)."""
    q = np.ascontiguousarray(q, np.uint32)
    f = floats(q)
    n = len(q)
    flux, aux, facing, nverts, band = np.zeros(n), np.zeros(n), np.full(n, -1), np.full(n, -1), np.full(n, np.inf)
    op = q[:, 0]
    m = op == GAUSS
    if m.any():
        flux[m] = ref_gauss(f[m, 1:7])
    m = op == WAVEFRONT
    if m.any():
        sg = f[m, 1:3]
        ok = (sg != 0).all(axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            tri = f[m, 3:9].reshape(-1, 3, 2) / sg[:, None, :]
            u = f[m, 9:11] / sg
            inten = np.exp(-0.5 * (u ** 2).sum(axis=1)) / (2 * math.pi * sg[:, 0] * sg[:, 1])
        fl = np.zeros(m.sum())
        fl[ok] = ref_gauss(tri[ok].reshape(-1, 6))
        at0 = (f[m, 9:11] == 0).all(axis=1)
        inten[~ok] = np.where(at0[~ok], np.inf, 0.0)
        flux[m], aux[m] = fl, inten
    m = op == REGION_LOCAL
    if m.any():
        k = int(m.sum())
        cones = np.zeros((k, 11))
        cones[:, 5] = 1.0
        cones[:, 6] = 1.0
        cones[:, 9], cones[:, 10] = f[m, 1], f[m, 2]
        nrm = np.zeros((k, 3))
        flux[m], _, nverts[m] = ref_region_fluxes(cones, f[m, 4:6], f[m, 6:8], f[m, 8:17], nrm, np.full(k, -1))
        z = f[m][:, [10, 13, 16]]
        band[m] = np.minimum(np.abs(z - f[m, 4:5]), np.abs(z - f[m, 5:6])).min(axis=1)
    m = op == REGION_TUID
    if m.any():
        geo = triangle_geometry(sc, q[m, 17]).astype(np.float64)
        cones = np.concatenate([f[m, 1:10], f[m, 10:12]], 1)
        want = q[m, 18].astype(np.int32)
        flux[m], facing[m], nverts[m] = ref_region_fluxes(cones, f[m, 13:15], f[m, 15:17], geo[:, :9], geo[:, 9:12], want)
        band[m] = np.abs((geo[:, 9:12] * f[m, 4:7]).sum(axis=1))
        o, d, x = f[m, 1:4], f[m, 4:7], f[m, 7:10]
        v = geo[:, :9].reshape(-1, 3, 3) - o[:, None, :]
        extra = {"flux_world": flux[m].copy(), "local": np.stack([(v * a[:, None, :]).sum(axis=2) for a in (x, np.cross(d, x), d)], 2),
                 "local_unit": 8 * 2.0 ** -24 * np.abs(v).sum(axis=2), "rows": np.nonzero(m)[0]}
        if out is not None:
            k = int(m.sum())
            ident = np.zeros((k, 11))
            ident[:, 5] = ident[:, 6] = 1.0
            ident[:, 9:11] = f[m, 10:12]
            fl, _, nv = ref_region_fluxes(ident, f[m, 13:15], f[m, 15:17], floats(out[m, W_VERTS:W_VERTS + 9]), np.zeros((k, 3)), np.full(k, -1))
            flux[m], nverts[m] = np.where(facing[m] == want, fl, 0.0), nv
        return {"flux": flux, "aux": aux, "facing": facing, "nverts": nverts, "band": band, **extra}
    return {"flux": flux, "aux": aux, "facing": facing, "nverts": nverts, "band": band}


def out_flux(out):
    return floats(out[:, W_FLUX])


def cpu_bound(ref):
    """the project's bound for this integral (tests/test_kat.py::test_gaussian_triangle_integral)"""
    return 2e-6 + 1e-5 * ref


def intensity_unit(q):
    """The f32 rounding of wavefront_intensity relative to its value, u = 2^-24 being the largest relative error of one rounding: each of ux^2,
    uy^2 carries 3 u (the division twice, the product), their sum 4 u, which expf turns into 4 |exponent| u relative; the factor in front 4 u
    (the constant, the product of the sigmas, the division, the product with expf) and expf itself up to 2 ulp = 4 u: (4 |exponent| + 8) u."""
    f = floats(q)
    with np.errstate(divide="ignore", invalid="ignore"):
        u = f[:, 9:11] / f[:, 1:3]
    return (4 * 0.5 * (u ** 2).sum(axis=1) + 8) * 2.0 ** -24


def class_errors(cls, err):
    return {str(c): float(err[cls == c].max()) for c in sorted(set(cls))}


# ------------------------------------------------------------------------------------------------ whole regions
def region_reference(sc, cones, cap=1 << 16):
    """The f64 sum (ref_region_sum) over the triangle ids of the checker's unbounded record, per cone: (ntris, sum); 0 triangles for a ballistic
    or empty query.  The record's envelope, slab, sigma and facing are the f32 values the checker summed with."""
    ntris, ids, rec = oracle_region_triangles(sc, cones, cap)
    assert ntris.max() <= cap
    sums = np.zeros(len(cones))
    r = rec.astype(np.float64)
    for i in np.nonzero(ntris)[0]:
        sums[i] = ref_region_sum(sc, r[i, :11], r[i, 11:13], r[i, 13:15], ids[i, :ntris[i]], int(rec[i, 15]))
    return ntris, sums


def whole_region_cones():
    """region_cones(120, 18), the cones of the issue that asked for this test, and 120 more of the same family: the first 120 alone hold 22
    regions of more than 64 triangles but only 2 of more than 2000; together 44 and 10"""
    from test_gpu_traversal import region_cones
    return np.concatenate([region_cones(120, 18), region_cones(120, 19)])


def whole_region_scene(Scene):
    return Scene("cornell_box", res=16, mesh_detail=1, lut=(32, 32))
