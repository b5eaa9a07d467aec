"""Per-query checks of the diffraction kernels (wt/diffraction_probe.h): the CPU checker's entry points oracle_fsd_apertures / oracle_utd_sums,
the query sets both test files use, and the f64 references.

Fraunhofer: the zero-order power of an aperture is re-evaluated from the segment records a build wrote, in f64, by the boundary line integral
(second_source.fraunhofer_boundary_terms), at the eight probe directions of fsd_build_finish.  UTD: the coherent sum over the accepted, visible
wedges plus the direct term, in f64, from the phase arguments and coefficients the evaluation reported (the phase argument is f32 in every form:
k_times_len)."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "indep"))
from second_source import fraunhofer_boundary_terms  # noqa: E402

from oracle_util import load_oracle  # noqa: E402

K_FSD_P0_SIGMA = np.float32(0.288675134594813 / 4)
K_FSD_DEAD_RATIO = 1e-10
K_FSD_MAX_EDGES = 4096
UTD_CAP = 48                 # records per aperture in the UTD tests: the per-walk share of the device's wedge pool (wtgpu_upload.hip: 48 per walk)
_INV_SQRT2 = 0.70710678118654752440
PROBE_DIRS = np.array([[-_INV_SQRT2, -_INV_SQRT2], [-1, 0], [-_INV_SQRT2, _INV_SQRT2], [0, 1], [_INV_SQRT2, _INV_SQRT2], [1, 0],
                       [_INV_SQRT2, -_INV_SQRT2], [0, -1]], np.float32)


def _p(a):
    return a.ctypes.data


def oracle_fsd_apertures(sc, cones, sk, ids, n_ids, pool_cap=K_FSD_MAX_EDGES):
    lib = load_oracle()
    lib.oracle_fsd_apertures.argtypes = [C.c_void_p] * 5 + [C.c_uint32] * 3 + [C.c_void_p] * 2
    ids = np.ascontiguousarray(ids, np.uint32)
    n, id_cap = ids.shape
    n_ids = np.ascontiguousarray(n_ids, np.uint32)
    assert (n_ids <= id_cap).all() and all((ids[i, :n_ids[i]] < sc.info.n_edges).all() for i in range(n))
    cones, sk = np.ascontiguousarray(cones, np.float32), np.ascontiguousarray(sk, np.float32)
    hdr = np.zeros((n, 8), np.uint32)
    segs = np.zeros((n, pool_cap, 7), np.float32)
    assert lib.oracle_fsd_apertures(sc.host_desc(), _p(cones), _p(sk), _p(ids), _p(n_ids), n, id_cap, pool_cap, _p(hdr), _p(segs)) == 0
    return hdr, segs


def oracle_utd_sums(sc, queries, ids, n_ids, utd_cap=UTD_CAP):
    lib = load_oracle()
    lib.oracle_utd_sums.argtypes = [C.c_void_p] * 4 + [C.c_uint32] * 3 + [C.c_void_p] * 3
    ids = np.ascontiguousarray(ids, np.uint32)
    n, id_cap = ids.shape
    n_ids = np.ascontiguousarray(n_ids, np.uint32)
    assert (n_ids <= id_cap).all() and all((ids[i, :n_ids[i]] < sc.info.n_edges).all() for i in range(n))
    queries = np.ascontiguousarray(queries, np.float32)
    hdr = np.zeros((n, 8), np.uint32)
    edges = np.zeros((n, utd_cap, 8), np.uint32)
    recs = np.zeros((n, utd_cap, 3), np.uint32)
    assert lib.oracle_utd_sums(sc.host_desc(), _p(queries), _p(ids), _p(n_ids), n, id_cap, utd_cap, _p(recs), _p(hdr), _p(edges)) == 0
    return hdr, edges, recs


def fsd_header(hdr):
    """hdr [n,8] u32 -> dict of arrays"""
    f = hdr.view(np.float32)
    return {"ok": hdr[:, 0], "n_edges": hdr[:, 1], "overflow": hdr[:, 2], "dead": hdr[:, 3], "P0": f[:, 4], "P0_pdf": f[:, 5], "psi02": f[:, 6],
            "edge_cap": hdr[:, 7]}


def pad_ids(lists):
    """list of edge-id lists -> (ids [n, id_cap] padded with 0xFFFFFFFF, n_ids [n])"""
    cap = max(1, max(len(x) for x in lists))
    ids = np.full((len(lists), cap), 0xFFFFFFFF, np.uint32)
    for i, x in enumerate(lists):
        ids[i, :len(x)] = x
    return ids, np.array([len(x) for x in lists], np.uint32)


# ------------------------------------------------------------------------------------------------ Fraunhofer
def fsd_reference(segs, n_edges, k):
    """f64 zero-order power of one aperture from its segment records (e, v, ab, iab, pdf; fsd units): B_j at the eight probe directions
    |xi| = 3 kFsdP0Sigma by the boundary integral, ASF = |sum B|^2 / (2 pi)^2.  -> psi02, P0, acc (= 8 psi02), inc (incoherent sum), and the
    rounding bound of an f32 accumulation of acc (for the `dead` band)."""
    s = np.asarray(segs[:n_edges], np.float64)
    e, v = s[:, 0:2], s[:, 2:4]
    ab, iab = s[:, 4], s[:, 5]
    a = v - e / 2
    ca, cb = iab + ab / 2, iab - ab / 2
    acc = inc = bound = 0.0
    for d in PROBE_DIRS.astype(np.float32):
        xi = (np.float32(3.0) * K_FSD_P0_SIGMA * d).astype(np.float64)
        B = fraunhofer_boundary_terms(a, e, ca, cb, xi) / (2 * np.pi) if n_edges else np.zeros(0, complex)
        # fsd_alpha1 / fsd_alpha2 (restating fsd.hpp) return 0 where xi . e == 0 in f32 (a removable singularity of the closed form, where the
        # integral is |e|^2 (ca + cb) / (2 |xi x e|) != 0): the reference's convention, kept, so such a segment contributes nothing here either.
        # For those terms the comparison checks consistency with that convention, not the physics: on the axis-aligned rims of double_slits
        # it removes them at 4 of the 8 probe directions.
        xf = np.float32(3.0) * K_FSD_P0_SIGMA * d
        zx = xf[0] * segs[:n_edges, 0].astype(np.float32) + xf[1] * segs[:n_edges, 1].astype(np.float32)
        B = np.where(zx == 0, 0, B)
        A = B.sum()
        acc += abs(A) ** 2
        inc += (np.abs(B) ** 2).sum()
        # f32 partial sums of n terms: |error| <= n u sum |B_j|, and the same again for the terms' own rounding
        dA = (n_edges + 2) * 2.0 ** -24 * np.abs(B).sum()
        bound += 2 * abs(A) * dA + dA * dA
    psi02 = acc / 8
    P0 = 2 * np.pi * float(K_FSD_P0_SIGMA) ** 2 * psi02 / float(k) ** 2
    return {"psi02": psi02, "P0": P0, "acc": acc, "inc": inc, "acc_bound": bound}


def fsd_dead_band(ref):
    """True where |acc - kFsdDeadRatio inc| is within the rounding of an f32 evaluation of acc (the two forms may then decide `dead` differently)."""
    return abs(ref["acc"] - K_FSD_DEAD_RATIO * ref["inc"]) <= ref["acc_bound"] + 1e-6 * K_FSD_DEAD_RATIO * ref["inc"]


def fsd_rel_err(got, ref, scale):
    """the error form of test_second_source's edge-sum test: relative, with a floor of 1e-6 of the aperture's incoherent power"""
    return abs(float(got) - ref) / max(ref, 1e-6 * scale, 1e-30)


def cone(o, d, tan_alpha, x0, ecc=0.0, lam_m=5e-5):
    d = np.asarray(d, np.float64)
    d = d / np.linalg.norm(d)
    return np.array([*o, *d, tan_alpha, x0, ecc, lam_m], np.float32)


def beam_sigma(c, dist):
    """wavefront std-dev of a cone at distance `dist` (cone_axes / kBeamEnvelope, as the render's regions: oracle_query_regions)"""
    r = np.float32(c[6]) * np.float32(dist) + np.float32(c[7])
    e = np.float32(np.sqrt(1 - np.float64(c[8]) ** 2))
    from_axes = np.array([r, r / e], np.float32) / np.float32(3.0)   # kBeamEnvelope
    return from_axes


def double_slits_beams():
    """Beams from the spot emitter (z = -500 mm) onto the screen with the two slits (z = -15 mm): centred (the symmetric aperture) and
    off-centre, narrow (one rim pair) to wide (all four rims), lambda = 50 um."""
    out = []
    for x, y, tan_a in [(0.0, 0.0, 3.5e-3), (0.0, 0.0, 1.2e-3), (3e-4, 0.0, 2e-3), (-2e-4, 1e-3, 6e-4), (4e-4, -2e-3, 1e-3), (0.0, 5e-3, 2.5e-3)]:
        c = cone((x, y, -0.5), (0, 0, 1), tan_a, 1e-5)
        out.append(c)
    return np.array(out, np.float32)


def k_of(lam_m):
    return np.float32(2 * np.pi / (lam_m * 1e3))


def segments_per_edge(sc, c, sk):
    """segment count of every scene edge alone in the aperture of beam `c` (the host's sequential build)"""
    n = sc.info.n_edges
    ids = np.arange(n, dtype=np.uint32)[:, None]
    hdr, _ = oracle_fsd_apertures(sc, np.repeat(c[None], n, 0), np.repeat(sk[None], n, 0), ids, np.ones(n, np.uint32), pool_cap=64)
    return hdr[:, 1] + hdr[:, 2]


def fsd_query_set(sc, beams, dist, counts, rng, long_ids=800):
    """Hand-built edge-id lists per beam: for every count in `counts` a random draw (with repetition when the scene has fewer) from the edges that
    give the beam segments, mixed with edges that give none; plus one list of `long_ids` ids of the longest edges (segment totals beyond
    kFsdMaxEdges).  -> cones, sk, list of id lists"""
    cones, sks, lists = [], [], []
    for c in beams:
        sk = np.array([*beam_sigma(c, dist), k_of(c[9])], np.float32)
        spe = segments_per_edge(sc, c, sk)
        live = np.nonzero(spe > 0)[0]
        dead = np.nonzero(spe == 0)[0]
        if len(live) == 0:
            continue
        for m in counts:
            n_live = m if m < 4 else max(1, (3 * m) // 4)
            pick = np.concatenate([rng.choice(live, n_live, replace=n_live > len(live)), rng.choice(dead, m - n_live, replace=m - n_live > len(dead))])
            rng.shuffle(pick)
            cones.append(c), sks.append(sk), lists.append(pick[:m].astype(np.uint32))
        if long_ids:
            best = live[np.argsort(-spe[live])][:4]
            cones.append(c), sks.append(sk), lists.append(np.resize(best, long_ids).astype(np.uint32))
    return np.array(cones, np.float32), np.array(sks, np.float32), lists


# ------------------------------------------------------------------------------------------------ UTD
def utd_terms(hdr, edges):
    """per query: accepted mask, visible mask (accepted, neither shadow ray blocked), phase arguments, Ds, Dh (complex), direct term flags"""
    n = int(hdr[0])
    e = edges[:n]
    f = e.view(np.float32)
    acc = (e[:, 0] & 1) != 0
    vis = acc & ((e[:, 0] & 6) == 0)
    Ds = f[:, 2].astype(np.float64) + 1j * f[:, 3]
    Dh = f[:, 4].astype(np.float64) + 1j * f[:, 5]
    return acc, vis, f[:, 1].astype(np.float64), Ds, Dh


def utd_reference(hdr, edges):
    """f64 coherent sum of one query -> (intensity (|ts|^2 + |th|^2) / 2, its magnitude scale ((sum|Ds| + 1)^2 + (sum|Dh| + 1)^2) / 2)"""
    acc, vis, phi, Ds, Dh = utd_terms(hdr, edges)
    ph = np.exp(-1j * phi[vis])
    ts, th = (ph * Ds[vis]).sum(), (ph * Dh[vis]).sum()
    if (hdr[2] & 3) == 1:
        d = np.exp(-1j * np.float64(hdr[3:4].view(np.float32)[0]))
        ts, th = ts + d, th + d
    I = (abs(ts) ** 2 + abs(th) ** 2) / 2
    scale = ((np.abs(Ds[vis]).sum() + 1) ** 2 + (np.abs(Dh[vis]).sum() + 1) ** 2) / 2
    return I, scale


ETOILE_TX = np.array([80.1, 193.8, 21.0])


def etoile_utd_queries(sc, sizes, rng, per_size=6):
    """Interaction points at the corners and roof edges of the city blocks, wi from the transmitter, destinations on both sides of the shadow
    boundaries; the edge-id lists are drawn so that the aperture has exactly `size` wedges (infinite region: every listed edge whose faces are not
    both turned away from wi is a wedge).  -> queries [n,32], id lists"""
    n_edges = sc.info.n_edges
    # which edges face a given wi: build with single-id lists on the host
    qs, lists = [], []
    for size in sizes:
        made = 0
        tries = 0
        while made < per_size and tries < 50:
            tries += 1
            ang = np.deg2rad(22.5 + 30.0 * rng.integers(0, 12))
            R = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]])
            corner = R @ np.array([150.0 + 180.0 * rng.integers(0, 2), 30.0 * rng.choice([-1, 1]), rng.uniform(2, 20)])
            src = ETOILE_TX
            wi = (src - corner) / np.linalg.norm(src - corner)
            # destination: across the corner from the source (every other query: on its side), turned by up to +-40 deg, at 20-150 m
            away = -wi.copy()
            t = np.deg2rad(rng.uniform(-40, 40) + (150 if made % 2 else 0))
            Rz = np.array([[np.cos(t), -np.sin(t), 0], [np.sin(t), np.cos(t), 0], [0, 0, 1]])
            dst = corner + (Rz @ away) * rng.uniform(20, 150)
            dst[2] = rng.uniform(1.5, 30)
            q = np.zeros(32, np.float32)
            q[:10] = cone(src, dst - src + rng.normal(scale=5, size=3), 0.05, 1e-2, 0.0, 0.03)   # wide cone: the direct path is usually inside
            q[10:13], q[13:16] = dst, corner
            q[16:25] = [1, 0, 0, 0, 1, 0, 0, 0, 1]
            q[25:28] = np.inf
            q[28:31] = wi
            q[31] = k_of(0.0299792458)
            one = np.repeat(q[None], n_edges, 0)
            h, e1, _ = oracle_utd_sums(sc, one, np.arange(n_edges, dtype=np.uint32)[:, None], np.ones(n_edges, np.uint32), utd_cap=1)
            facing = np.nonzero(h[:, 0] + h[:, 1] > 0)[0]
            if len(facing) < min(size, 49):
                continue
            # the wedges that diffract towards dst unobstructed first (up to half of the aperture), then the others
            lit = facing[(e1[facing, 0, 0] & 7) == 1]
            rest = np.setdiff1d(facing, lit)
            n_lit = min(len(lit), (size + 1) // 2)
            pick = np.concatenate([rng.choice(lit, n_lit, replace=False), rng.choice(rest, size - n_lit, replace=size - n_lit > len(rest))])
            others = np.setdiff1d(np.arange(n_edges), facing)
            lst = np.concatenate([pick, rng.choice(others, min(len(others), 3), replace=False)]) if size else rng.choice(others, 3, replace=False)
            rng.shuffle(lst)
            qs.append(q), lists.append(lst.astype(np.uint32))
            made += 1
    return np.array(qs, np.float32), lists
