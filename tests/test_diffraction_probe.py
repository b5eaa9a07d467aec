"""The sequential diffraction forms of the CPU checker, one query at a time, against f64 references (tests/diffraction_probe.py): the Fraunhofer
aperture build (fsd_build_aperture after the sizing of bdpt_walk_step) and the coherent UTD sum (path_do_fsd).  The device's cooperative forms
are held against the same references and against these host results in tests/test_gpu_diffraction.py."""
import numpy as np

import diffraction_probe as dp

FSD_COUNTS = [0, 1, 2, 7, 8, 9, 63, 64, 65, 95, 96]
UTD_SIZES = [0, 1, 7, 8, 9, 11, 47, 48, 60]


def _scene(name, **kw):
    from wave_tracer_amd import Scene
    return Scene(name, **kw)


def _fsd_checks(sc, cones, sks, lists, pool_cap=dp.K_FSD_MAX_EDGES, tol=2e-4):
    ids, n_ids = dp.pad_ids(lists)
    hdr, segs = dp.oracle_fsd_apertures(sc, cones, sks, ids, n_ids, pool_cap)
    h = dp.fsd_header(hdr)
    worst = {"psi02": 0.0, "P0": 0.0, "pdf_sum": 0.0}
    band = 0
    for i in range(len(cones)):
        n = int(h["n_edges"][i])
        assert n + h["overflow"][i] <= max(1, n_ids[i]) * 16, i      # at most ~6 segments per scene edge
        ref = dp.fsd_reference(segs[i], n, sks[i, 2])
        scale = ref["inc"] / 8
        e_psi = dp.fsd_rel_err(h["psi02"][i], ref["psi02"], scale)
        e_p0 = dp.fsd_rel_err(h["P0"][i], ref["P0"], scale * ref["P0"] / max(ref["psi02"], 1e-300))
        total = segs[i, :n, 6].astype(np.float64).sum() + h["P0_pdf"][i]
        assert e_psi < tol and e_p0 < tol, (i, h["psi02"][i], ref["psi02"], h["P0"][i], ref["P0"])
        assert abs(total - 1) < 2e-6 * max(1, n / 16), (i, n, total)
        if dp.fsd_dead_band(ref):
            band += 1
        else:
            assert h["dead"][i] == (n >= 2 and ref["acc"] < dp.K_FSD_DEAD_RATIO * ref["inc"]), (i, ref["acc"], ref["inc"])
        worst["psi02"], worst["P0"] = max(worst["psi02"], e_psi), max(worst["P0"], e_p0)
        worst["pdf_sum"] = max(worst["pdf_sum"], abs(total - 1))
    return h, segs, worst, band


def test_host_fraunhofer_apertures_against_f64_double_slits(built):
    """double_slits: beams from the spot onto the slit screen (the centred one: the symmetric aperture whose amplitudes cancel), hand-built
    edge-id lists of 0..96 ids and one of 800 ids of the longest rims (segment totals beyond kFsdMaxEdges = 4096: the clamp of
    fsd_pool_alloc_edges, counted in `overflow`).  psi02 / P0 against the boundary integral in f64, the pdfs + P0_pdf sum to 1, `dead` as the f64
    sums decide outside the rounding band."""
    sc = _scene("double_slits", res=96, lut=(64, 64))
    rng = np.random.default_rng(5)
    cones, sks, lists = dp.fsd_query_set(sc, dp.double_slits_beams(), 0.485, FSD_COUNTS, rng)
    h, segs, worst, band = _fsd_checks(sc, cones, sks, lists)
    assert (h["overflow"] > 0).sum() >= 1 and (h["n_edges"] == dp.K_FSD_MAX_EDGES).sum() >= 1     # the clamp was reached
    assert (h["n_edges"] > 64).sum() >= 4 and (h["n_edges"] == 0).sum() >= 1
    print(f"host Fraunhofer (double_slits, {len(cones)} apertures): worst psi02 {worst['psi02']:.1e}, P0 {worst['P0']:.1e}, |sum pdf - 1| "
          f"{worst['pdf_sum']:.1e}; dead {int(h['dead'].sum())}, inside the rounding band {band}")


def test_host_fraunhofer_apertures_against_f64_cornell_regions(built):
    """cornell_box (mesh_detail 1): the classified-edge sets of whole interaction regions (oracle_query_regions, equal to brute force)."""
    from test_gpu_traversal import oracle_regions, region_cones
    sc = _scene("cornell_box", res=16, mesh_detail=1, lut=(32, 32))
    cones = region_cones(60, 18)
    o = oracle_regions(sc, cones, edge_cap=1024)
    keep = [i for i in range(len(cones)) if (o["flags"][i] & 3) == 0 and o["nedges"][i, 1] > 0]
    assert len(keep) >= 10
    lists = [o["edges_slab"][i, :min(o["nedges"][i, 1], 1024)] for i in keep]
    sks = np.array([[*dp.beam_sigma(cones[i], o["dist"][i]), dp.k_of(cones[i, 9])] for i in keep], np.float32)
    h, segs, worst, band = _fsd_checks(sc, cones[keep], sks, lists)
    n_ids = np.array([len(x) for x in lists])
    assert (n_ids >= 8).sum() >= 3 and (n_ids < 8).sum() >= 3
    print(f"host Fraunhofer (cornell regions, {len(keep)} apertures of {n_ids.min()}..{n_ids.max()} ids): worst psi02 {worst['psi02']:.1e}, "
          f"P0 {worst['P0']:.1e}; inside the dead band {band}")


def test_host_fraunhofer_pool_exhaustion(built):
    """A segment pool smaller than the aperture's request: fsd_pool_alloc_edges fails, ok = 0, the aperture is empty (P0_pdf = 1) and every
    segment the build produced is counted in `overflow` — the numbers a pool of its own size gives in n_edges."""
    sc = _scene("double_slits", res=96, lut=(64, 64))
    rng = np.random.default_rng(6)
    cones, sks, lists = dp.fsd_query_set(sc, dp.double_slits_beams(), 0.485, [7, 9, 33], rng, long_ids=0)
    ids, n_ids = dp.pad_ids(lists)
    big, _ = dp.oracle_fsd_apertures(sc, cones, sks, ids, n_ids, 4096)
    small, _ = dp.oracle_fsd_apertures(sc, cones, sks, ids, n_ids, 3)
    b, s = dp.fsd_header(big), dp.fsd_header(small)
    need = b["edge_cap"]
    fail = need > 3
    assert fail.sum() >= 5 and (b["ok"] == 1).all()
    assert (s["ok"][fail] == 0).all() and (s["n_edges"][fail] == 0).all() and (s["P0_pdf"][fail] == 1).all()
    assert (s["overflow"][fail] == b["n_edges"][fail] + b["overflow"][fail]).all()
    assert (s["ok"][~fail] == 1).all() and (s["n_edges"][~fail] == b["n_edges"][~fail]).all()


def utd_check(hdr, edges, which):
    """worst |I - I_f64| / scale over the queries for the header word `which` (4..6 coop_do_fsd<1,8,64>, 7 path_do_fsd)"""
    errs = []
    for i in range(len(hdr)):
        ref, scale = dp.utd_reference(hdr[i], edges[i])
        errs.append(abs(float(hdr[i, which:which + 1].view(np.float32)[0]) - ref) / scale)
    return np.array(errs)


def test_host_utd_sums_against_f64(built):
    """etoile (mesh_detail 0): building corners lit from the transmitter, destinations on both sides of the shadow boundaries, apertures of
    0..60 wedges (48 = the record capacity of the test: beyond it utd_build_aperture counts `overflow`).  path_do_fsd (f32 sums) against the f64
    sum of the same terms, relative to the magnitude scale (sum |D| + 1)^2 of the sum (coherent sums cancel)."""
    sc = _scene("etoile", res=64, mesh_detail=0)
    rng = np.random.default_rng(7)
    qs, lists = dp.etoile_utd_queries(sc, UTD_SIZES, rng)
    ids, n_ids = dp.pad_ids(lists)
    hdr, edges, recs = dp.oracle_utd_sums(sc, qs, ids, n_ids)
    sizes = hdr[:, 0] + hdr[:, 1]
    assert set(UTD_SIZES) <= set(sizes.tolist()), sorted(set(sizes.tolist()))
    assert (hdr[:, 1] > 0).sum() >= 1 and (hdr[:, 0] <= dp.UTD_CAP).all()
    vis = sum(dp.utd_terms(hdr[i], edges[i])[1].sum() for i in range(len(hdr)))
    acc = sum(dp.utd_terms(hdr[i], edges[i])[0].sum() for i in range(len(hdr)))
    assert vis >= 10 and acc > vis and ((hdr[:, 2] & 3) == 1).sum() >= 3 and ((hdr[:, 2] & 3) == 3).sum() >= 1
    e = utd_check(hdr, edges, 7)
    assert e.max() < 1e-6, e.max()
    print(f"host UTD ({len(hdr)} apertures, {acc} accepted wedges, {vis} visible): path_do_fsd vs f64 worst {e.max():.1e}")
