"""The film passes on a DEVELOPED f32 film on the MI355X (wtgpu_tonemap_source_device, wtgpu_film_stats_source_device,
wtgpu_film_compare_source_device, wtgpu_film_polar_source_device; the developed instantiations of k_develop_tonemap, k_film_stats, k_film_compare
and k_film_polar) against the host twins on the same film, bit for bit — the operators that call libm within one code, the project's rule for
them.  The twins are held to numpy restatements by tests/test_film_developed.py, whose drawn films (payload NaNs, -0, subnormals, infinities) are
used here: at 37 x 23 (851 pixels: a part of one block, a chunk that ends inside the film), 256 x 192 (192 chunks: a second level of sums) and,
P = 12, 257 x 256 (257 chunks, then 2, then 1: the finish loop runs twice).  Then the device on develop_device's output against the device on the
accumulators; the chain the feature exists for — render, denoise, view and measure the denoised film where it lies; and what the calls leave alone."""
import ctypes as C

import numpy as np
import pytest

import test_film_developed as cpu
from test_film_compare import FIELDS as COMPARE_FIELDS
from test_film_compare import films_of
from test_film_developed import COMPARE_DERIVED, STATS_KEYS, TMS
from test_film_polar import DERIVED as POLAR_DERIVED
from test_film_polar import FIELDS as POLAR_FIELDS
from test_film_polar import MAPS, NO_PIXEL, PICTURE_TMS, POLAR, THETA, polar_films
from test_film_stats import F32, LEVELS, PLANES, checker, option_cases, same_bits, stats_scene
from test_film_stats import to_device as _to_device
from test_tonemap import grey_table, random_table

pytestmark = pytest.mark.gpu

SIZES = [(37, 23), (256, 192)]
SPE = 7


@pytest.fixture(scope="module")
def scenes(built, tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_film_developed")
    return {(w, h, P): stats_scene(d, P, w, h).upload(0) for w, h in SIZES + [LEVELS] for P in (sorted(PLANES) if (w, h) != LEVELS else (12,))}


def drawn(size, P, seed, polar=False):
    """test_film_developed.drawn_film at another size"""
    _, _, channels, stokes = PLANES[P]
    return cpu.drawn_film(channels, stokes, seed, polar, height=size[1], width=size[0])


def host(t, fmt="f32"):
    a = t.cpu().numpy()
    return a.view(np.uint16) if fmt == "u16" else a


def same_dict(got, want, keys, label):
    to_host = lambda t: t if isinstance(t, np.ndarray) else t.cpu().numpy()
    for k in keys:
        assert same_bits(to_host(got[k]), to_host(want[k])), (label, k)


def within_one_code(g, h, label):
    g, h = g.astype(np.int64), h.astype(np.int64)
    assert g.shape == h.shape and np.abs(g - h).max() <= 1, (label, int(np.abs(g - h).max()))


# ---- 5. device = host twin on the same developed film ---------------------------------------------------------------------------------------------
def _statistics(scenes, size, P, seed):
    sc = scenes[size + (P,)]
    _, _, channels, stokes = PLANES[P]
    film = drawn(size, P, seed)
    d_film, d_mask = _to_device(sc, (film, checker(size[1], size[0])))
    mask = checker(size[1], size[0])
    for bins in (0, 7, 4096):
        for s, abs_, lum, masked in option_cases(channels, stokes):
            kw = dict(stokes_component=s, scale="dB", range=(-50.0, 10.0), bins=bins, abs=abs_, luminance=lum)
            got = sc.film_stats_developed_device(d_film, mask=d_mask if masked else None, **kw)
            want = sc.film_stats_developed_host(film, mask=mask if masked else None, threads=16, **kw)
            same_dict(got, want, STATS_KEYS, (size, P, bins, s, abs_, lum, masked))
            assert got["n_nan"][:channels].all() and (got["n"] == (int((mask > 0).sum()) if masked else size[0] * size[1])).all()


def _comparison(scenes, size, P, seed):
    sc = scenes[size + (P,)]
    _, _, channels, stokes = PLANES[P]
    w, h = size
    a, b = drawn(size, P, seed), drawn(size, P, seed + 1)
    b.reshape(w * h, -1)[1] = F32(1.0)
    acc = films_of(P, seed + 2, h, w)
    mask = checker(h, w)
    d_a, d_b, d_mask = _to_device(sc, (a, b, mask))
    d_acc = _to_device(sc, acc)
    for s, abs_, lum, masked in option_cases(channels, stokes):
        kw = dict(stokes_component=s, abs=abs_, luminance=lum, eps=3e-9, diff=True)
        for label, (x, spe_x, d_x), (y, spe_y, d_y) in (("dev/dev", (a, None, d_a), (b, None, d_b)), ("dev/acc", (a, None, d_a), (acc, SPE, d_acc)),
                                                         ("acc/dev", (acc, SPE, d_acc), (b, None, d_b))):
            got = sc.film_compare_device(d_x, spe_x, d_y, spe_y, mask=d_mask if masked else None, **kw)
            want = sc.film_compare_host(x, spe_x, y, spe_y, mask=mask if masked else None, threads=16, **kw)
            same_dict(got, want, COMPARE_FIELDS + COMPARE_DERIVED + ("diff",), (size, P, label, s, abs_, lum, masked))
            assert got["n_nonfinite"].all() and got["n_differ"].all() and (got["argmax"] < w * h).all()
    # the same memory twice
    got = sc.film_compare_device(d_a, None, d_a, None)
    assert not got["n_differ"].any() and not got["n_nonfinite_mismatch"].any() and (got["argmax"] == NO_PIXEL).all()


def _polarisation(sc, size, P, seed):
    w, h = size
    channels = POLAR[P]
    film = drawn(size, P, seed, polar=True)
    mask = checker(h, w)
    d_film, d_mask = _to_device(sc, (film, mask))
    k = 0
    for lum in ((False, True) if channels == 3 else (False,)):
        for masked in (False, True):
            for fmt in ("f32", "u8", "u16"):
                k += 1
                kw = dict(luminance=lum, maps=MAPS, analyser=THETA, picture=True, picture_plane=k % (channels + lum), fmt=fmt, sat_gain=(1.0, 2.5)[k % 2])
                got = sc.film_polar_developed_device(d_film, mask=d_mask if masked else None, **kw)
                want = sc.film_polar_developed_host(film, mask=mask if masked else None, threads=16, **kw)
                label = (size, P, lum, masked, fmt)
                same_dict(got, want, POLAR_FIELDS + POLAR_DERIVED, label)
                same_dict(got["maps"], want["maps"], MAPS, label)
                assert same_bits(host(got["picture"], fmt), want["picture"]), (label, "picture")
                assert got["n_nonfinite"].all() and got["n_dark"].all() and (got["argmax"] < w * h).all() and (got["sum_pol"] > 0).all()
    bare = sc.film_polar_developed_device(d_film, luminance=channels == 3)
    same_dict(bare, sc.film_polar_developed_host(film, luminance=channels == 3), POLAR_FIELDS, (size, P, "records alone"))
    for tm in PICTURE_TMS:
        for fmt in ("u8", "u16"):
            kw = dict(picture=True, picture_plane=channels - 1, tm=tm, fmt=fmt, sat_gain=1.5)
            g, hh = host(sc.film_polar_developed_device(d_film, mask=d_mask, **kw)["picture"], fmt), sc.film_polar_developed_host(film, mask=mask, **kw)["picture"]
            within_one_code(g, hh, (size, P, tm, fmt))
            assert np.array_equal(g[..., 3], hh[..., 3])


@pytest.mark.parametrize("P", sorted(PLANES))
@pytest.mark.parametrize("size", SIZES)
def test_statistics_equal_the_host_twin(scenes, size, P):
    _statistics(scenes, size, P, 100 + P)


def test_statistics_equal_the_host_twin_over_two_levels(scenes):
    _statistics(scenes, LEVELS, 12, 112)


@pytest.mark.parametrize("P", sorted(PLANES))
@pytest.mark.parametrize("size", SIZES)
def test_comparison_equals_the_host_twin(scenes, size, P):
    _comparison(scenes, size, P, 200 + P)


def test_comparison_equals_the_host_twin_over_two_levels(scenes):
    _comparison(scenes, LEVELS, 12, 212)


@pytest.mark.parametrize("staged", ["1", "0"])
@pytest.mark.parametrize("size,P", [(size, P) for size in SIZES for P in sorted(POLAR)] + [(LEVELS, 12)])
def test_polarisation_view_equals_the_host_twin(built, tmp_path, monkeypatch, size, P, staged):
    """both loaders of k_film_polar (WTGPU_FILM_POLAR_STAGED): four elements per lane through LDS, and every lane its own pixel's"""
    monkeypatch.setenv("WTGPU_FILM_POLAR_STAGED", staged)
    _polarisation(stats_scene(tmp_path, P, *size).upload(0), size, P, 300 + P)


@pytest.mark.parametrize("P", sorted(PLANES))
@pytest.mark.parametrize("size", SIZES)
def test_tonemap_equals_the_host_twin(scenes, size, P):
    sc = scenes[size + (P,)]
    _, _, channels, stokes = PLANES[P]
    film = drawn(size, P, 400 + P)
    mask = checker(size[1], size[0])
    d_film, d_mask = _to_device(sc, (film, mask))
    k = 0
    for tm in TMS:
        for mode in ("select", "normal", "colourmap"):
            for s in range(stokes):
                for fmt in ("f32", "u8", "u16"):
                    k += 1
                    t = dict(tm, mode=mode, table=random_table(5) if k % 2 else grey_table())
                    masked = k % 3 == 0
                    g = host(sc.tonemap_developed_device(d_film, t, s, mask=d_mask if masked else None, fmt=fmt), fmt)
                    h = sc.tonemap_developed_host(film, t, s, mask=mask if masked else None, fmt=fmt, threads=16)
                    label = (size, P, tm, mode, s, fmt, masked)
                    if tm["op"] == "linear":
                        assert g.dtype == h.dtype and same_bits(g, h), label
                    elif fmt != "f32":
                        within_one_code(g, h, label)


# ---- 6. the device on develop_device's output = the device on the accumulators -----------------------------------------------------------------
@pytest.mark.parametrize("P", sorted(PLANES))
def test_develop_device_output_gives_what_the_accumulators_give(scenes, P):
    """Every field, map and picture, bit for bit — the pictures of the operators that call libm too: the two instantiations of a kernel run the same
    device code on the same f32 (measured on the MI355X: no code differs; docs/FEATURES.md)."""
    size = SIZES[1]
    w, h = size
    sc = scenes[size + (P,)]
    _, _, channels, stokes = PLANES[P]
    films = polar_films(h, w, channels, 500 + P) if stokes == 4 else films_of(P, 500 + P, h, w)
    other = films_of(P, 600 + P, h, w)
    mask = checker(h, w)
    d_films, d_other = _to_device(sc, films), _to_device(sc, other)
    d_mask, = _to_device(sc, (mask,))
    d_film, d_film_other = sc.develop_device(*d_films, SPE), sc.develop_device(*d_other, 5)
    for s, abs_, lum, masked in option_cases(channels, stokes):
        m = d_mask if masked else None
        kw = dict(stokes_component=s, abs=abs_, luminance=lum, mask=m)
        same_dict(sc.film_stats_developed_device(d_film, range=(-50.0, 10.0), bins=256, **kw), sc.film_stats_device(*d_films, SPE, range=(-50.0, 10.0), bins=256, **kw), STATS_KEYS,
                  (P, "stats", s, abs_, lum, masked))
        want = sc.film_compare_device(d_films, SPE, d_other, 5, diff=True, **kw)
        for a, spe_a, b, spe_b in ((d_film, None, d_film_other, None), (d_film, None, d_other, 5), (d_films, SPE, d_film_other, None)):
            same_dict(sc.film_compare_device(a, spe_a, b, spe_b, diff=True, **kw), want, COMPARE_FIELDS + COMPARE_DERIVED + ("diff",), (P, "compare", s, abs_, lum, masked))
        for tm in TMS:
            for fmt in ("f32", "u8"):
                t = dict(tm, mode="normal")
                g, a = host(sc.tonemap_developed_device(d_film, t, s, mask=m, fmt=fmt)), host(sc.tonemap_device(*d_films, SPE, t, s, mask=m, fmt=fmt))
                assert same_bits(g, a), (P, "tonemap", tm, s, fmt)
    if stokes == 4:
        for lum in ((False, True) if channels == 3 else (False,)):
            for tm in TMS:
                kw = dict(luminance=lum, maps=MAPS, analyser=THETA, mask=d_mask, picture=True, picture_plane=channels - 1 + lum, tm=tm, fmt="u8", sat_gain=2.0)
                got, want = sc.film_polar_developed_device(d_film, **kw), sc.film_polar_device(*d_films, SPE, **kw)
                same_dict(got, want, POLAR_FIELDS + POLAR_DERIVED, (P, "polar", lum))
                for k in MAPS:
                    assert same_bits(host(got["maps"][k]), host(want["maps"][k])), (P, "polar", lum, k)
                assert same_bits(host(got["picture"]), host(want["picture"])), (P, "polar picture", lum, tm)


# ---- 7. the chain the feature exists for ---------------------------------------------------------------------------------------------------------
def test_a_denoised_film_is_viewed_and_measured_where_it_lies(built):
    import torch
    from wave_tracer_amd import Scene
    from wave_tracer_amd.render import denoise, quality, render_to_noise, view
    sc = Scene("cornell_box", polarimetric=1, res=24, mesh_detail=0, crop_of=1440, lut=(64, 64)).upload(0)
    merged, spp, _, (d_a, d_b) = render_to_noise(sc, 0.0, max_spp=8, chunk_spp=4, seed=3, halves=True)
    torch.cuda.synchronize(merged[0].device)
    assert spp == 8
    d_film = sc.film_denoise_device(d_a, 4, d_b, 4)["film"]
    film = d_film.cpu().numpy()
    ref = tuple(t.cpu().numpy() for t in merged)
    assert np.isfinite(film).all() and film.any()
    tm = {"op": "linear", "mode": "normal"}
    for fmt in ("f32", "u8", "u16"):
        assert same_bits(host(sc.tonemap_developed_device(d_film, tm, fmt=fmt), fmt), sc.tonemap_developed_host(film, tm, fmt=fmt)), fmt
    same_dict(sc.film_stats_developed_device(d_film, luminance=True), sc.film_stats_developed_host(film, luminance=True), STATS_KEYS, "stats")
    kw = dict(luminance=True, maps=MAPS, analyser=THETA, picture=True, picture_plane=3, fmt="u8", sat_gain=2.0)
    got, want = sc.film_polar_developed_device(d_film, **kw), sc.film_polar_developed_host(film, **kw)
    same_dict(got, want, POLAR_FIELDS + POLAR_DERIVED + ("picture",), "polar")
    same_dict(got["maps"], want["maps"], MAPS, "polar maps")
    assert (got["mean_dolp"] > 0).all() and not got["n_nonfinite"].any()
    got, want = sc.film_compare_device(d_film, None, merged, 8, luminance=True, diff=True), sc.film_compare_host(film, None, ref, 8, luminance=True, diff=True)
    same_dict(got, want, COMPARE_FIELDS + COMPARE_DERIVED + ("diff",), "compare")
    assert got["n_differ"].all() and (got["rel_l2"] > 0).all()
    # render.denoise(view=True) returns that picture; render.quality that record
    out = denoise(sc, d_a, d_b, 4, view=True)
    assert same_bits(host(out["film"]), film) and same_bits(host(out["picture"]), host(view(sc, d_film)))
    within_one_code(host(out["picture"]), view(sc, film), "the scene's own operator (sRGB) calls libm")
    assert out["picture"].dtype == torch.uint8 and tuple(out["picture"].shape) == (24, 24, 3) and out["picture"].any()
    q = quality(sc, d_film, merged, 8, luminance=True)
    assert same_bits(q["rel_l2"], want["rel_l2"]) and same_bits(quality(sc, film, ref, 8, luminance=True)["rel_l2"], want["rel_l2"])


# ---- 8. side effects and refusals ------------------------------------------------------------------------------------------------------------------
def test_the_passes_between_renders_change_nothing(built):
    import torch
    from wave_tracer_amd import Scene, render
    sc = Scene("furnace_path", polarimetric=1, res=32, lut=(32, 32)).upload(0)
    sc.reset_counters()
    a = render(sc, 2, seed=6)
    ca = sc.counters()
    sc.reset_counters()
    d_a = _to_device(sc, a)
    d_film = sc.develop_device(*d_a, 2)
    kept = d_film.clone()
    lum = sc.spectral_channels == 3
    stats = sc.film_stats_developed_device(d_film, luminance=lum)
    polar = sc.film_polar_developed_device(d_film, luminance=lum, maps=MAPS, picture=True)
    comp = sc.film_compare_device(d_film, None, d_a, 2, luminance=lum)
    picture = sc.tonemap_developed_device(d_film, {"op": "linear", "mode": "normal"}, fmt="u8")
    torch.cuda.synchronize(d_film.device)
    assert all(v == 0 for v in sc.counters().values()) and (stats["sum"] > 0).all() and (polar["sum_i"] > 0).all() and not comp["n_differ"].any() and picture.any()
    assert torch.equal(kept.view(torch.int32), d_film.view(torch.int32))
    b = render(sc, 2, seed=6)
    assert sc.counters() == ca and ca["samples"] > 0
    for x, y in zip(a, b):
        assert np.array_equal(x != 0, y != 0) and np.allclose(x, y, rtol=1e-12, atol=0)
    assert all(same_bits(x, t.cpu().numpy()) for x, t in zip(a, d_a))


def test_a_mask_that_excludes_everything(scenes):
    for size in SIZES:
        sc = scenes[size + (12,)]
        w, h = size
        film = drawn(size, 12, 9, polar=True)
        mask = np.zeros((h, w), F32)
        mask[0, 0] = np.nan
        d_film, d_mask = _to_device(sc, (film, mask))
        stats = sc.film_stats_developed_device(d_film, range=(-50.0, 10.0), luminance=True, mask=d_mask)
        same_dict(stats, sc.film_stats_developed_host(film, range=(-50.0, 10.0), luminance=True, mask=mask), STATS_KEYS, size)
        assert not stats["n"].any() and np.isnan(stats["min"]).all() and not stats["hist"].any()
        polar = sc.film_polar_developed_device(d_film, luminance=True, mask=d_mask, maps=MAPS, picture=True, fmt="u8")
        same_dict(polar, sc.film_polar_developed_host(film, luminance=True, mask=mask, maps=MAPS, picture=True, fmt="u8"), POLAR_FIELDS + ("picture",), size)
        assert not polar["n"].any() and (polar["argmax"] == NO_PIXEL).all() and not any(host(m).any() for m in polar["maps"].values())
        comp = sc.film_compare_device(d_film, None, d_film, None, mask=d_mask, diff=True)
        assert not comp["n"].any() and not host(comp["diff"]).any()
        picture = host(sc.tonemap_developed_device(d_film, {"op": "linear", "mode": "normal"}, mask=d_mask, fmt="u8"))
        assert picture[..., :3].any() and not picture[..., 3].any()


def test_refusals(built, tmp_path, scenes):
    """WTGPU_ERR_INVALID (1) from the entry points themselves without an upload; the Python methods refuse before they get there, and refuse a
    film of another dtype, size, device or layout."""
    import torch
    from wave_tracer_amd import WtgpuError
    from wave_tracer_amd.api import FilmCompare, FilmCompareSpec, FilmPolar, FilmPolarSpec, FilmSource, FilmStats, FilmStatsSpec, load_library
    sc = stats_scene(tmp_path, 4)
    dev = torch.device("cuda", 0)
    film = torch.zeros((23, 37, 1, 4), dtype=torch.float32, device=dev)
    for call in (lambda: sc.tonemap_developed_device(film), lambda: sc.film_stats_developed_device(film), lambda: sc.film_polar_developed_device(film),
                 lambda: sc.film_compare_device(film, None, film, None)):
        with pytest.raises(WtgpuError, match="upload"):
            call()
    lib = load_library()
    src = FilmSource(None, None, None, 0, film.data_ptr())
    out = torch.zeros((23, 37, 4), dtype=torch.float32, device=dev)
    srec, crec, prec = FilmStats(), FilmCompare(), FilmPolar()
    sspec, cspec, pspec = FilmStatsSpec(0, 1, 0, 0, -50.0, 10.0), FilmCompareSpec(0, 0, 1e-4), FilmPolarSpec()
    for rc in (lib.wtgpu_tonemap_source_device(sc.handle, None, C.byref(src), None, 0, None, 0, out.data_ptr()),
               lib.wtgpu_film_stats_source_device(sc.handle, None, C.byref(src), C.byref(sspec), None, C.cast(C.pointer(srec), C.c_void_p), None),
               lib.wtgpu_film_compare_source_device(sc.handle, None, C.byref(src), C.byref(src), C.byref(cspec), None, C.cast(C.pointer(crec), C.c_void_p), None),
               lib.wtgpu_film_polar_source_device(sc.handle, None, C.byref(src), C.byref(pspec), None, C.cast(C.pointer(prec), C.c_void_p), None, None)):
        assert rc == 1 and b"scene not uploaded" in lib.wtgpu_last_error()
    up = scenes[SIZES[0] + (4,)]
    neither = FilmSource(None, None, None, 0, None)
    assert lib.wtgpu_film_stats_source_device(up.handle, None, C.byref(neither), C.byref(sspec), None, C.cast(C.pointer(srec), C.c_void_p), None) == 1
    assert b"neither form is set" in lib.wtgpu_last_error()
    for bad in (film.double(), film[:, :36], film.cpu(), torch.zeros((23, 37, 2, 4), dtype=torch.float32, device=dev)[:, :, ::2], film.cpu().numpy()):
        for call in (lambda f: up.tonemap_developed_device(f), lambda f: up.film_stats_developed_device(f), lambda f: up.film_polar_developed_device(f),
                     lambda f: up.film_compare_device(f, None, film, None), lambda f: up.film_compare_device(film, None, f, None)):
            with pytest.raises(ValueError, match=r"film: a contiguous torch.float32 tensor \[23, 37, 1, 4\] \(3404 elements\) on cuda:0 expected"):
                call(bad)
