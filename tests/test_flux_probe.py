"""The region power integral on the host, query by query: the f64 reference (oracle/flux64.cpp) pinned on its own — closed forms, additivity,
scipy, the clipper's areas — and then the CPU checker's twin of the device probe (wt/flux_probe.h: oracle_flux_queries; wt/gauss.h, wt/cone.h:
clip_triangle_z / cone_project_local / region_local_triangle_flux, wt/bdpt.h: region_triangle_flux) against it on the sets of
tests/flux_probe.py.  The device is held against both in tests/test_gpu_flux.py.

Bounds.  |twin - ref| <= 2e-6 + 1e-5 ref is the project's bound for this integral (tests/test_kat.py::test_gaussian_triangle_integral); it
holds for every class but the triangles of scale 50 sigma, whose bound is 2 x the worst error measured on the committed set
(tests/golden/flux_measured.json: twin/gauss_scale50).  The same file holds the twin's worst absolute error per class (the intensity: relative);
this test recomputes them and asserts that none has grown by more than a factor of 2.  PARITY_RECORD=1 writes the values measured to
flux_measured.json in the record directory of tests/parity.py instead of comparing with the committed ones."""
import math

import numpy as np
import pytest

import flux_probe as fp


def _twin_and_reference(sc, q):
    out = fp.oracle_flux_queries(sc, q)
    return out, fp.reference(sc, q, out)


@pytest.fixture(scope="module")
def scene_and_sets(built):
    from wave_tracer_amd import Scene
    sc, qs = fp.flux_sets(Scene)
    return sc, {name: (q, cls, info, *_twin_and_reference(sc, q)) for name, (q, cls, info) in qs.items()}


@pytest.fixture(scope="module")
def sets(scene_and_sets):
    return scene_and_sets[1]


# ------------------------------------------------------------------------------------------------ the reference alone
def _rot(t):
    return np.array([[math.cos(t), -math.sin(t)], [math.sin(t), math.cos(t)]])


def test_reference_closed_forms(built):
    """whole plane 1, half plane 0.5 erfc(h / sqrt 2) for h in {0, 1e-4, 0.02, 1, 3} (in several directions), quadrant 0.25: each to 1e-12"""
    B = 1e3
    assert abs(fp.ref_gauss([[-B, -B, B, -B, 0, B]])[0] - 1.0) < 1e-12
    for h in (0.0, 1e-4, 0.02, 1.0, 3.0):
        want = 0.5 * math.erfc(h / math.sqrt(2))
        for t in (0.0, 0.3, math.pi / 2, 2.0, -2.7):
            tri = np.array([[h, -B], [h, B], [B, 0.0]]) @ _rot(t).T
            got = fp.ref_gauss([tri.ravel()])[0]
            assert abs(got - want) < 1e-12, (h, t, got, want)
            assert abs(fp.ref_gauss([tri[[0, 2, 1]].ravel()])[0] - want) < 1e-12          # the other orientation
    for t in (0.0, 0.3, -1.1):
        tri = np.array([[0.0, 0.0], [B, 0.0], [0.0, B]]) @ _rot(t).T
        assert abs(fp.ref_gauss([tri.ravel()])[0] - 0.25) < 1e-12
    assert fp.ref_gauss([[0.5, 0.25, 1.5, 2.25, 2.5, 4.25]])[0] == 0.0                    # collinear


def test_reference_is_additive():
    """the 8 x 8-sigma square, rotated by 0.3 and shifted by (0.37, -0.21), cut into cells of 0.05, 0.0714, 0.12 and 1.0 (two triangles each):
    the sum of the parts equals the two-triangle value to 1e-9"""
    R, shift = _rot(0.3), np.array([0.37, -0.21])
    corners = np.array([[-4.0, -4.0], [4.0, -4.0], [4.0, 4.0], [-4.0, 4.0]]) @ R.T + shift
    whole = fp.ref_gauss([corners[[0, 1, 2]].ravel(), corners[[0, 2, 3]].ravel()]).sum()
    assert 0.99 < whole < 1.0
    for cell in (0.05, 0.0714, 0.12, 1.0):
        n = int(math.ceil(8.0 / cell))
        g = np.minimum(-4.0 + cell * np.arange(n + 1), 4.0)
        x0, y0 = np.meshgrid(g[:-1], g[:-1], indexing="ij")
        x1, y1 = np.meshgrid(g[1:], g[1:], indexing="ij")
        p00, p10, p11, p01 = (np.stack([a.ravel(), b.ravel()], 1) @ R.T + shift for a, b in ((x0, y0), (x1, y0), (x1, y1), (x0, y1)))
        tris = np.concatenate([np.concatenate([p00, p10, p11], 1), np.concatenate([p00, p11, p01], 1)])
        parts = fp.ref_gauss(tris)
        total = math.fsum(parts)
        print(f"cells of {cell}: {len(tris)} triangles, sum - whole = {total - whole:.2e}")
        assert abs(total - whole) < 1e-9, (cell, total, whole)


def test_reference_against_scipy():
    """a dozen random triangles of every scale against scipy.integrate.dblquad over the barycentric domain, to 1e-9"""
    from scipy import integrate
    rng = np.random.default_rng(5)
    for i in range(12):
        scale = (0.1, 0.5, 1.5, 3.0)[i % 4]
        a, b, c = rng.normal(scale=scale, size=(3, 2)) + rng.normal(scale=0.7, size=2)
        J = abs((b - a)[0] * (c - a)[1] - (b - a)[1] * (c - a)[0])
        f = lambda v, u: math.exp(-0.5 * float(np.sum((a + u * (b - a) + v * (c - a)) ** 2))) / (2 * math.pi) * J
        want, _ = integrate.dblquad(f, 0, 1, 0, lambda u: 1 - u, epsabs=1e-12, epsrel=1e-12)
        got = fp.ref_gauss([np.concatenate([a, b, c])])[0]
        assert abs(got - want) < 1e-9, (i, got, want)


def _area(poly):
    if len(poly) < 3:
        return 0.0
    return sum(0.5 * np.linalg.norm(np.cross(poly[i] - poly[0], poly[i + 1] - poly[0])) for i in range(1, len(poly) - 1))


def test_reference_clipping():
    """Sutherland-Hodgman against the slab: the clipped polygon's area is at most the triangle's, equals it for a triangle inside the slab, and the
    parts below, inside and above the slab add up to the triangle's area to 1e-12 relative"""
    rng = np.random.default_rng(6)
    counts = {}
    for i in range(400):
        tri = rng.normal(size=(3, 3))
        zmin = rng.uniform(-1.5, 1.0)
        zmax = zmin + rng.uniform(0.01, 2.0)
        if i % 5 == 0:
            tri[:, 2] = rng.uniform(zmin, zmax, 3)
        full = _area(tri)
        mid = fp.ref_clip(tri, zmin, zmax)
        below, above = fp.ref_clip(tri, -np.inf, zmin), fp.ref_clip(tri, zmax, np.inf)
        counts[len(mid)] = counts.get(len(mid), 0) + 1
        assert _area(mid) <= full * (1 + 1e-12)
        assert ((mid[:, 2] >= zmin - 1e-15) & (mid[:, 2] <= zmax + 1e-15)).all()
        if i % 5 == 0:
            assert len(mid) == 3 and abs(_area(mid) - full) <= 1e-12 * full
        assert abs(_area(below) + _area(mid) + _area(above) - full) <= 1e-12 * full, (i, _area(below), _area(mid), _area(above), full)
    print("polygon vertex counts:", counts)
    assert counts.get(0, 0) and counts.get(3, 0) and counts.get(4, 0) and counts.get(5, 0)


# ------------------------------------------------------------------------------------------------ the twin against f64
def twin_errors(sets):
    """{class: worst |twin - ref|} over every set, plus wavefront_intensity (relative) — what flux_measured.json holds as twin/<class>"""
    errs = {}
    for name, (q, cls, info, out, ref) in sets.items():
        errs.update(fp.class_errors(cls, np.abs(fp.out_flux(out) - ref["flux"])))
        if name == "wavefront":
            m = cls == "wavefront"
            inten = fp.floats(out[m, fp.W_AUX])
            errs["wavefront_intensity"] = float((np.abs(inten - ref["aux"][m]) / ref["aux"][m]).max())
        if name == "region_tuid":   # (for information: the integral from the world-frame triangle, input conditioning included)
            errs["region_tuid_world"] = float(np.abs(fp.out_flux(out) - ref["flux_world"]).max())
    return errs


def test_twin_against_f64(sets):
    """every flux word within 2e-6 + 1e-5 ref of the f64 integral (scale 50: 2 x the committed measurement), finite and in [0, 1]; the intensity
    within its rounding unit (flux_probe.intensity_unit); the per-class worst errors have not grown beyond 2 x the committed ones"""
    errs = twin_errors(sets)
    for k, v in sorted(errs.items()):
        print(f"twin/{k}: {v:.3e}")
    if fp.recording():
        fp.record({f"twin/{k}": v for k, v in errs.items()})
    committed = fp.measured() if not fp.recording() else None
    for name, (q, cls, info, out, ref) in sets.items():
        got = fp.out_flux(out)
        assert np.isfinite(got).all() and (got >= 0).all() and (got <= 1).all(), name
        err = np.abs(got - ref["flux"])
        normal = cls != "gauss_scale50"
        bad = np.nonzero(normal & (err > fp.cpu_bound(ref["flux"])))[0]
        assert not len(bad), (name, len(bad), [(int(i), cls[i], got[i], ref["flux"][i]) for i in bad[:5]])
        if name == "wavefront":
            m = cls == "wavefront"
            inten = fp.floats(out[m, fp.W_AUX])
            rel = np.abs(inten - ref["aux"][m]) / ref["aux"][m]
            assert np.isfinite(inten).all() and (rel <= fp.intensity_unit(q[m])).all(), float((rel / fp.intensity_unit(q[m])).max())
    assert len(errs) >= 19, sorted(errs)
    q, cls, info, out, ref = sets["region_tuid"]
    dl = np.abs(fp.floats(out[:, fp.W_VERTS:fp.W_VERTS + 9]).reshape(-1, 3, 3) - ref["local"]) / ref["local_unit"][:, :, None]
    over = np.abs(fp.out_flux(out) - ref["flux_world"]) > fp.cpu_bound(ref["flux_world"])
    print(f"region_tuid: beam-frame vertices within {dl.max():.2f} of their rounding unit; from the world-frame triangle {int(over.sum())} of {len(q)} "
          f"queries beyond 2e-6 + 1e-5 ref, worst {errs['region_tuid_world']:.2e} (the conditioning of the f32 frame change)")
    assert dl.max() <= 1.0
    if committed is not None:
        assert errs["gauss_scale50"] <= 2 * committed["twin/gauss_scale50"], (errs["gauss_scale50"], committed["twin/gauss_scale50"])
        for k, v in errs.items():
            if k != "region_tuid_world":
                assert v <= 2 * committed[f"twin/{k}"], (k, v, committed[f"twin/{k}"])


def test_twin_exact_results(sets):
    """exact zeros: zero-area triangles, a vanishing sigma, triangles wholly outside the slab, the wrong facing; the intensity of a vanishing
    sigma is inf on the axis and 0 off it; the closed forms of tests/test_kat.py; the branch word on both sides of the switch"""
    q, cls, info, out, ref = sets["gauss"]
    got = fp.out_flux(out)
    assert len(info["zero_area"]) >= 20 and (out[info["zero_area"], fp.W_FLUX] == 0).all() and (ref["flux"][info["zero_area"]] == 0).all()
    for row, want in info["known"].items():
        assert abs(got[row] - want) < 2e-6 and abs(ref["flux"][row] - want) < 1e-12, (row, got[row], ref["flux"][row], want)
    assert len(info["known"]) == 20
    sw = cls == "gauss_switch"
    f = fp.floats(q[sw, 1:7]).astype(np.float32).reshape(-1, 3, 2)
    e2 = np.stack([((f[:, i] - f[:, (i + 1) % 3]) ** 2).sum(axis=1, dtype=np.float32) for i in range(3)], 1).max(axis=1)
    assert (np.abs(e2 / fp.SWITCH - 1) < 0.0101).all()
    branch = out[sw, fp.W_AUX]
    assert (branch == (e2 < np.float32(fp.SWITCH))).all() and 150 < branch.sum() < 250
    small, large = np.isin(cls, ["gauss_s0.01", "gauss_s0.03"]), np.isin(cls, ["gauss_s3", "gauss_s8", "gauss_scale50"])
    assert out[small, fp.W_AUX].mean() > 0.9 and out[large, fp.W_AUX].mean() < 0.01
    ori = np.nonzero(cls == "gauss_orient")[0]
    h = len(ori) // 2
    assert np.abs(got[ori[:h]] - got[ori[h:]]).max() < 2e-6 and (ref["flux"][ori[:h]] > 1e-3).sum() > 50

    q, cls, info, out, ref = sets["wavefront"]
    z = np.nonzero(cls == "wavefront_zero_sigma")[0]
    assert len(z) == 12 and (out[z, fp.W_FLUX] == 0).all()
    at0 = (fp.floats(q[z, 9:11]) == 0).all(axis=1)
    assert at0.sum() == 6 and (out[z[at0], fp.W_AUX] == fp.bits(np.inf)).all() and (out[z[~at0], fp.W_AUX] == 0).all()
    ratio = fp.floats(q[cls == "wavefront", 1]) / fp.floats(q[cls == "wavefront", 2])
    assert ratio.min() < 0.011 and ratio.max() > 90 and (np.abs(np.log(ratio)) < 0.01).sum() >= 50

    q, cls, info, out, ref = sets["region_local"]
    outside = info["kind"] == "outside"
    assert outside.sum() > 300 and (out[outside, fp.W_FLUX] == 0).all() and (out[outside, fp.W_AUX] == 0).all() and (ref["flux"][outside] == 0).all()

    q, cls, info, out, ref = sets["region_tuid"]
    wrong = out[:, fp.W_AUX] != q[:, 18]
    assert 0.3 < wrong.mean() < 0.7 and (out[wrong, fp.W_FLUX] == 0).all()
    assert (fp.out_flux(out)[~wrong] > 1e-3).sum() > 300


def test_twin_clip_counts_and_facing(sets):
    """`tris` equals the f64 polygon's vertex count minus 2 unless a vertex lies within 1e-6 of a slab plane (counted, at most 1 % of the set); the
    facing bit equals the f64 one outside |dot(n, d)| < 1e-6 (counted, at most 1 %); what the sets hold"""
    q, cls, info, out, ref = sets["region_local"]
    want = np.maximum(ref["nverts"] - 2, 0)
    near = ref["band"] < 1e-6
    tris = out[:, fp.W_AUX].astype(np.int64)
    census = {k: int((info["kind"] == k).sum()) for k in fp.REGION_KINDS}
    print(f"region_local: {len(q)} queries, {int(near.sum())} with a vertex within 1e-6 of a slab plane ({int((tris != want)[near].sum())} of them counted differently); "
          f"tris histogram {np.bincount(tris, minlength=4).tolist()}; kinds {census}")
    assert (tris[~near] == want[~near]).all(), np.nonzero((tris != want) & ~near)[0][:10]
    assert near.sum() <= len(q) // 100
    hist = np.bincount(tris, minlength=4)
    assert hist[0] > 300 and hist[1] > 500 and hist[2] > 300 and hist[3] > 150, hist
    assert near.sum() >= 30 and all(census[k] >= 12 for k in fp.REGION_KINDS), census
    clipped = (tris >= 1) & ~((fp.floats(q[:, [10, 13, 16]]) >= fp.floats(q[:, 4:5])) & (fp.floats(q[:, [10, 13, 16]]) <= fp.floats(q[:, 5:6]))).all(axis=1)
    assert clipped.sum() > 1000
    for env in fp.ENVELOPES:
        assert (cls == "region_local_" + env).sum() >= 1000
    fsize = np.abs(fp.floats(q[:, 8:17]).reshape(-1, 3, 3)[:, :, :2]).max(axis=(1, 2)) / (3 * fp.floats(q[:, 6]))
    assert fsize.min() < 0.1 and fsize.max() > 30

    q, cls, info, out, ref = sets["region_tuid"]
    band = ref["band"] < 1e-6
    print(f"region_tuid: {len(q)} queries, {int(band.sum())} inside |dot(n, d)| < 1e-6; tris of the scene {len(set(q[:, 17].tolist()))}")
    assert band.sum() <= len(q) // 100
    assert (out[~band, fp.W_AUX] == ref["facing"][~band]).all()
    assert q[:, 18].sum() == len(q) // 2 and 0.3 < out[:, fp.W_AUX].mean() < 0.7


def test_invalid_queries_are_rejected(scene_and_sets):
    """an op outside the table or a tuid >= the scene's triangle count: 1, nothing is run"""
    sc, sets = scene_and_sets
    q = sets["region_tuid"][0][:2].copy()
    q[1, 17] = sc.info.n_tris
    fp.oracle_flux_queries(sc, q, expect=1)
    q = sets["gauss"][0][:2].copy()
    q[0, 0] = len(fp.OPS)
    fp.oracle_flux_queries(sc, q, expect=1)


def test_whole_region_sums_twin_against_f64(built):
    """The checker's region sums (oracle_query_regions: f32 contributions of region_triangle_flux summed in f64, over the unbounded record and over
    a brute-force scan of the final slab) on the cones of the device test against ref_region_sum over the record's triangle ids.  The worst
    error, committed as twin/region_sum, is the yardstick of the device's (tests/test_gpu_flux.py) and may not grow beyond 2 x.  It is the
    conditioning of the f32 change to the beam frame (see flux_probe.reference), largest on regions of one or two triangles; the regions above
    2000 triangles are printed on their own."""
    from wave_tracer_amd import Scene
    from test_gpu_traversal import oracle_regions
    sc = fp.whole_region_scene(Scene)
    cones = fp.whole_region_cones()
    o = oracle_regions(sc, cones)
    ntris, ref = fp.region_reference(sc, cones)
    diff = (o["flags"] & 3) == 0
    assert diff.sum() > 200 and (ntris[diff] == o["ntris"][diff, 0]).all() and (o["ntris"][diff, 0] == o["ntris"][diff, 1]).all()
    assert (ntris > 64).sum() >= 20 and (ntris > 2000).sum() >= 5 and (ntris[~diff] == 0).all()
    err = np.abs(o["flux"][diff].astype(np.float64) - ref[diff, None])
    big = ntris[diff] > 2000
    print(f"twin/region_sum: {err[:, 1].max():.3e} over {int(diff.sum())} regions (the record's sum: {err[:, 0].max():.3e}); above 2000 triangles "
          f"({int(big.sum())} regions, largest {int(ntris.max())}): {err[big, 1].max():.3e}")
    assert np.isfinite(o["flux"]).all() and (o["flux"] >= 0).all()      # (triangles behind one another in a region count twice: a sum may exceed 1)
    assert err.max() < 1e-3
    if fp.recording():
        fp.record({"twin/region_sum": err[:, 1].max()})
    else:
        assert err[:, 1].max() <= 2 * fp.measured()["twin/region_sum"], (err[:, 1].max(), fp.measured()["twin/region_sum"])
