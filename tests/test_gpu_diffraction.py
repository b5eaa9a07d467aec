"""The wave-cooperative diffraction kernels query by query (wtgpu_test_fsd_apertures / wtgpu_test_utd_sums, kernels_test.hip): coop_build_aperture
(wt/coop_fsd.h) against the sequential build it replaces, on the device and in the CPU checker, and coop_do_fsd<G> (wt/coop_utd.h) for G = 1, 8, 64
against path_do_fsd — both against the f64 references of tests/diffraction_probe.py.  Then whole renders with every aperture built by either
form (WTGPU_COOP_APERTURE_MIN)."""
import numpy as np
import pytest

import diffraction_probe as dp
import parity
from oracle_util import oracle_render
from test_diffraction_probe import FSD_COUNTS, UTD_SIZES, utd_check

pytestmark = pytest.mark.gpu


def _scene(name, **kw):
    from wave_tracer_amd import Scene
    sc = Scene(name, **kw)
    sc.upload(0)
    return sc


def _fsd_sets():
    """(scene, cones, sk, id lists) of the query sets: double_slits hand-built lists (0..96 ids, 800 ids past the kFsdMaxEdges clamp, the
    symmetric aperture) and cornell_box (mesh_detail 1) region edge sets from wtgpu_query_regions"""
    from test_gpu_traversal import region_cones
    sc = _scene("double_slits", res=96, lut=(64, 64))
    out = [(sc, *dp.fsd_query_set(sc, dp.double_slits_beams(), 0.485, FSD_COUNTS, np.random.default_rng(5)))]
    sc2 = _scene("cornell_box", res=16, mesh_detail=1, lut=(32, 32))
    cones = region_cones(300, 18)
    g = sc2.query_regions(cones)
    keep = [i for i in range(len(cones)) if (g["flags"][i] & 3) == 0 and g["nedges"][i] > 0]
    lists = [g["edges"][i, :g["nedges"][i]] for i in keep]
    sks = np.array([[*dp.beam_sigma(cones[i], g["dist"][i]), dp.k_of(cones[i, 9])] for i in keep], np.float32)
    out.append((sc2, cones[keep], sks, lists))
    return out


def _rel(a, b, floor):
    return np.abs(a.astype(np.float64) - b) / np.maximum(np.maximum(np.abs(b.astype(np.float64)), floor), 1e-30)


def test_fraunhofer_cooperative_against_sequential_and_f64(built):
    """Per aperture: coop_build_aperture (mode 0), the device's sequential build (mode 1) and the checker's sequential build agree on ok / n_edges /
    overflow exactly; the segment records (e, v, a_b, iab_2) of the two device forms are bit-identical and in the same order ("same arithmetic on
    the same operands", wt/coop_fsd.h); pdf, P0, P0_pdf, psi02 agree to 1e-6, or to n u (u = 2^-24: the a-priori rounding bound of the
    sequential form's f32 sums of n terms) where n > 16; psi02 and P0 of both against the f64 boundary integral to 2e-4 (the
    tolerance of test_second_source's edge sum); the pdfs + P0_pdf sum to 1; `dead` agrees outside the rounding band."""
    worst = {"coop_vs_seq_small": 0.0, "coop_vs_seq_large": 0.0, "pdf_vs_seq_small": 0.0, "pdf_vs_seq_large": 0.0, "coop_f64": 0.0, "seq_f64": 0.0,
             "pdf_coop": 0.0, "pdf_seq": 0.0}
    band = total = n_dead = 0
    for sc, cones, sks, lists in _fsd_sets():
        ids, n_ids = dp.pad_ids(lists)
        hc, sc_ = sc.fsd_apertures(cones, sks, ids, n_ids, mode=0)
        hs, ss = sc.fsd_apertures(cones, sks, ids, n_ids, mode=1)
        ho, so = dp.oracle_fsd_apertures(sc, cones, sks, ids, n_ids)
        c, s, o = dp.fsd_header(hc), dp.fsd_header(hs), dp.fsd_header(ho)
        for key in ("ok", "n_edges", "overflow", "edge_cap"):
            assert (c[key] == s[key]).all() and (s[key] == o[key]).all(), key
        assert (c["ok"] == 1).all()
        for i in range(len(cones)):
            n = int(c["n_edges"][i])
            assert np.array_equal(sc_[i, :n, :6].view(np.uint32), ss[i, :n, :6].view(np.uint32)), (i, n)
            assert np.allclose(ss[i, :n, :6], so[i, :n, :6], rtol=1e-5, atol=1e-6 * np.abs(so[i, :n, :6]).max(initial=0)), i   # host libm
            ref = dp.fsd_reference(ss[i], n, sks[i, 2])
            floor = 1e-6 * ref["inc"] / 8
            # 1e-6, or the a-priori bound n u (u = 2^-24) of the sequential form's f32 sum of n terms where that is larger (n > 16)
            tol = max(1e-6, n * 2.0 ** -24)
            small = "small" if n <= 16 else "large"
            e = max(_rel(sc_[i, :n, 6], ss[i, :n, 6], 0).max(initial=0), _rel(c["P0_pdf"][i:i + 1], s["P0_pdf"][i:i + 1], 1e-7)[0])
            assert e <= tol, (i, n, e)
            worst["pdf_vs_seq_" + small] = max(worst["pdf_vs_seq_" + small], e)
            pf = ref["P0"] / max(ref["psi02"], 1e-300)
            for key, fl in (("psi02", floor), ("P0", floor * pf)):
                e = _rel(c[key][i:i + 1], s[key][i:i + 1], fl)[0]
                assert e <= tol, (i, n, key, c[key][i], s[key][i])
                worst["coop_vs_seq_" + small] = max(worst["coop_vs_seq_" + small], e)
            ec = max(dp.fsd_rel_err(c["psi02"][i], ref["psi02"], ref["inc"] / 8), dp.fsd_rel_err(c["P0"][i], ref["P0"], ref["inc"] / 8 * pf))
            es = max(dp.fsd_rel_err(s["psi02"][i], ref["psi02"], ref["inc"] / 8), dp.fsd_rel_err(s["P0"][i], ref["P0"], ref["inc"] / 8 * pf))
            assert ec < 2e-4 and es < 2e-4, (i, ec, es)
            worst["coop_f64"], worst["seq_f64"] = max(worst["coop_f64"], ec), max(worst["seq_f64"], es)
            tc = sc_[i, :n, 6].astype(np.float64).sum() + c["P0_pdf"][i]
            ts = ss[i, :n, 6].astype(np.float64).sum() + s["P0_pdf"][i]
            assert abs(tc - 1) < 1e-6 and abs(ts - 1) < 2 * tol, (i, n, tc, ts)
            worst["pdf_coop"], worst["pdf_seq"] = max(worst["pdf_coop"], abs(tc - 1)), max(worst["pdf_seq"], abs(ts - 1))
            if dp.fsd_dead_band(ref):
                band += 1
            else:
                assert c["dead"][i] == s["dead"][i] == o["dead"][i], (i, ref["acc"], ref["inc"])
            n_dead += int(c["dead"][i])
            total += 1
        assert (c["overflow"] > 0).any() or sc.name != "double_slits"
    print(f"Fraunhofer, {total} apertures: coop vs sequential, <= 16 / > 16 segments: psi02 / P0 worst {worst['coop_vs_seq_small']:.1e} / "
          f"{worst['coop_vs_seq_large']:.1e}, pdf / P0_pdf {worst['pdf_vs_seq_small']:.1e} / {worst['pdf_vs_seq_large']:.1e}; vs f64: coop {worst['coop_f64']:.1e}, "
          f"sequential {worst['seq_f64']:.1e}; |sum pdf - 1|: coop {worst['pdf_coop']:.1e}, sequential {worst['pdf_seq']:.1e}; dead {n_dead}, "
          f"inside the rounding band of `dead` {band}")


def test_fraunhofer_pool_exhaustion_both_forms(built):
    """A segment pool smaller than the request: both device forms report ok = 0, an empty aperture and every produced segment in `overflow`,
    exactly as the checker does (test_diffraction_probe.test_host_fraunhofer_pool_exhaustion)."""
    sc = _scene("double_slits", res=96, lut=(64, 64))
    cones, sks, lists = dp.fsd_query_set(sc, dp.double_slits_beams(), 0.485, [7, 9, 33], np.random.default_rng(6), long_ids=0)
    ids, n_ids = dp.pad_ids(lists)
    o = dp.fsd_header(dp.oracle_fsd_apertures(sc, cones, sks, ids, n_ids, 3)[0])
    assert (o["ok"] == 0).sum() >= 5
    for mode in (0, 1):
        g = dp.fsd_header(sc.fsd_apertures(cones, sks, ids, n_ids, pool_cap=3, mode=mode)[0])
        for key in ("ok", "n_edges", "overflow", "edge_cap", "P0_pdf"):
            assert np.array_equal(g[key], o[key]), (mode, key)


def test_utd_cooperative_sums_against_sequential_and_f64(built):
    """etoile (mesh_detail 0), apertures of 0..60 wedges (48 records: beyond, `overflow`), a query count that is not a multiple of 64 / G (the
    last wavefront's groups hold no aperture).  Per wedge the device's decisions (utd_f_edge, both shadow rays) equal the checker's and Ds / Dh
    equal wedge_UTD on the host to 1e-5; the intensities of coop_do_fsd<1,8,64> and path_do_fsd agree with the f64 sum to 1e-6 of its
    magnitude scale, the cooperative ones query by query at least as close as path_do_fsd and bit-identical to each other; the results of the queries beside the empty groups equal launches
    with n = 1."""
    sc = _scene("etoile", res=64, mesh_detail=0)
    qs, lists = dp.etoile_utd_queries(sc, UTD_SIZES, np.random.default_rng(7))
    n = len(qs) if len(qs) % 8 else len(qs) - 3
    qs, lists = qs[:n], lists[:n]
    assert n % 8 and n % 64
    ids, n_ids = dp.pad_ids(lists)
    hg, eg, rg = sc.utd_sums(qs, ids, n_ids)
    ho, eo, ro = dp.oracle_utd_sums(sc, qs, ids, n_ids)
    assert np.array_equal(hg[:, :3], ho[:, :3]) and np.array_equal(rg, ro)
    flips = n_far = n_wedges = 0
    far = []
    d_worst = 0.0
    for i in range(n):
        m = int(hg[i, 0])
        assert np.array_equal(eg[i, :m, 0] & 1, eo[i, :m, 0] & 1), i
        flips += int((eg[i, :m, 0] != eo[i, :m, 0]).sum())
        fg, fo = eg[i, :m, 1:8].view(np.float32), eo[i, :m, 1:8].view(np.float32)
        D = np.abs(fo[:, 1:5]).max(axis=1, initial=0)
        dD = np.abs(fg[:, 1:5] - fo[:, 1:5]).max(axis=1, initial=0) / np.maximum(D, 1e-30)
        d_worst = max(d_worst, dD.max(initial=0))
        n_far += int((dD > 1e-5).sum())
        for j in np.nonzero(dD > 1e-5)[0]:
            far.append((i, int(j), float(dD[j]), fo[j, 1:5].tolist(), fg[j, 1:5].tolist(), float(fo[j, 5]), float(fo[j, 6])))
        n_wedges += int((eo[i, :m, 0] & 1).sum())
        assert np.allclose(fg[:, 0], fo[:, 0], rtol=1e-6), i
    # Ds / Dh: the same code on both sides; host and device libm (atan2f, tanf, cosf of the UTD terms) differ in the last bits, and a few
    # wedges carry that further (measured: 4 of 220 wedges at 1.1e-5..3.5e-5 of their coefficient, the rest below 1e-5)
    print(f"UTD coefficients device vs host: worst relative difference {d_worst:.1e}, {n_far} of {n_wedges} wedges beyond 1e-5")
    for f in far[:12]:
        print("  wedge beyond 1e-5: query %d wedge %d rel %.1e host Ds,Dh %s device %s ri %.3g ro %.3g" % f)
    assert flips == 0 and n_far <= max(2, n_wedges // 50) and d_worst < 1e-4, (flips, n_far, n_wedges, d_worst)
    errs = {w: utd_check(hg, eg, w) for w in (4, 5, 6, 7)}
    # f64 partial sums are the same number to ~1e-16 in any order: the three cooperative forms round them to the same f32 values (and then
    # do the same arithmetic) unless a sum lies within 1e-16 of an f32 rounding boundary — bit-identical results wherever >= 2 wedges add up
    multi = np.array([dp.utd_terms(hg[i], eg[i])[1].sum() >= 2 for i in range(n)])
    same = (hg[:, 4] == hg[:, 5]) & (hg[:, 5] == hg[:, 6])
    print(f"UTD, {n} apertures: worst |I - I_f64| / scale: coop G=1 {errs[4].max():.1e}, G=8 {errs[5].max():.1e}, G=64 {errs[6].max():.1e}, "
          f"path_do_fsd {errs[7].max():.1e} (means {errs[4].mean():.1e} / {errs[5].mean():.1e} / {errs[6].mean():.1e} / {errs[7].mean():.1e}); "
          f"G = 1 / 8 / 64 bit-identical in {int(same[multi].sum())} of the {int(multi.sum())} sums of >= 2 wedges")
    for w, e in errs.items():
        assert e.max() < 1e-6, (w, e.max())
    # per query: the cooperative ts / th are the f32 roundings of (nearly) exact sums, path_do_fsd's are f32 accumulations; what follows (direct
    # term, |.|^2) is the same arithmetic, which may move either result by a few ulps of the scale
    for w in (4, 5, 6):
        worse = errs[w] > errs[7] + 4 * 2.0 ** -24
        assert not worse.any(), (w, np.nonzero(worse)[0], errs[w][worse], errs[7][worse])
    assert multi.sum() >= 10 and (~same[multi]).sum() <= 1, (int(multi.sum()), int((~same[multi]).sum()))
    for i in range(max(0, n - 6), n):
        h1, _, _ = sc.utd_sums(qs[i:i + 1], ids[i:i + 1], n_ids[i:i + 1])
        assert np.array_equal(h1[0, 4:8], hg[i, 4:8]), i


@pytest.mark.parametrize("name,res,spp,kw", [("cornell_box", 32, 2, {"mesh_detail": 1, "lut": (128, 128), "crop_of": 1440})])
def test_render_with_either_aperture_form(built, monkeypatch, name, res, spp, kw):
    """Whole renders with every aperture of a gathered region built by k_edges' wavefront (WTGPU_COOP_APERTURE_MIN=0), the default split (8 edge
    ids) and every aperture built by one lane of pass B (4294967295).  The knob only acts on the regions k_edges gathers (a bounded list that
    overflowed or holds more than kMaxEdgeIds / 3 triangles), hence the bench geometry (mesh_detail 1, the central crop of the 1440^2 film).
    WTGPU_PROFILE=1 counts the apertures with segments k_edges built: > 0 at 0, none at 4294967295, and at the default fewer than at 0 (the
    regions of 1..7 edge ids went to pass B: both forms ran in one render).  The diffraction counters are the same in the three renders and each
    film matches the CPU checker."""
    from wave_tracer_amd import Scene, develop, render
    monkeypatch.setenv("WTGPU_PROFILE", "1")
    sc0 = Scene(name, res=res, **kw)
    ov, ow, ol, oc = oracle_render(sc0, 0, spp, 17)
    cpu = develop(sc0, ov, ow, ol, spp).astype(np.float64)
    counters, coop, films = {}, {}, {}
    for setting in ("0", None, "4294967295"):
        if setting is None:
            monkeypatch.delenv("WTGPU_COOP_APERTURE_MIN", raising=False)
        else:
            monkeypatch.setenv("WTGPU_COOP_APERTURE_MIN", setting)
        sc = Scene(name, res=res, **kw)
        v, w, l = render(sc, spp, seed=17, device=0)
        gpu = develop(sc, v, w, l, spp).astype(np.float64)
        c = sc.counters()
        counters[setting] = {k: c[k] for k in ("fsd_interactions", "fsd_edge_overflow", "fsd_pool_overflow")}
        p = sc.profile_counters(8)
        coop[setting] = (p[3], p[5])   # (apertures built by k_edges' wavefront, walks k_edges gathered)
        films[setting] = gpu
        assert np.isfinite(gpu).all()
        parity.check(f"aperture_form/{name}-{setting}", np.abs(gpu - cpu).sum() / max(1e-300, np.abs(cpu).sum()), 2e-2)
        sc.close()
    diff = np.abs(films["0"] - films["4294967295"]).sum() / max(1e-300, np.abs(films["4294967295"]).sum())
    print(f"aperture forms, {name}: (cooperative apertures, gathered walks) {coop}; counters {counters}; film 0 vs 4294967295 rel L1 {diff:.1e}")
    assert coop["0"][0] > 0 and coop["4294967295"][0] == 0 and 0 < coop[None][0] < coop["0"][0], coop
    assert coop["0"][1] == coop[None][1] == coop["4294967295"][1], coop
    assert counters["0"] == counters[None] == counters["4294967295"], counters
    assert counters["0"]["fsd_interactions"] > 0
