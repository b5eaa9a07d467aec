"""The film passes on a DEVELOPED f32 film (wtgpu_film_source; wtgpu_tonemap_source_host, wtgpu_film_stats_source_host, wtgpu_film_compare_source_host,
wtgpu_film_polar_source_host; render.view, render.quality) on the CPU.  Three things are held:
  the same result from either source — a twin on wtgpu_develop's output of a set of accumulators gives what the accumulators' twin gives, every
    record field, histogram bin, difference plane, map and picture byte, for every operator (both run the same host code on the same f32);
  a film that develop did not write — f32 drawn here, with a payload NaN, -0, a subnormal and both infinities — against the numpy restatements of
    tests/test_film_stats.py, test_film_compare.py, test_film_polar.py and test_tonemap.py, applied to the film itself;
  the refusals, each with its message, and the Python forms."""
import ctypes as C

import numpy as np
import pytest

import test_film_polar
import test_film_stats
import test_tonemap
from test_film_compare import EDGES, QUIET_NAN, films_of, restate_compare
from test_film_compare import FIELDS as COMPARE_FIELDS
from test_film_compare import check_against_restatement as check_compare
from test_film_polar import DERIVED as POLAR_DERIVED
from test_film_polar import FIELDS as POLAR_FIELDS
from test_film_polar import MAPS, PICTURE_TMS, POLAR, THETA, polar_films, restate_polar
from test_film_polar import check_against_restatement as check_polar
from test_film_stats import F32, PLANES, H, W, checker, option_cases, restate_edges, restate_stats, same_bits, stats_scene
from test_film_stats import check_against_restatement as check_stats
from test_tonemap import grey_table, quantise, random_table

pytestmark = pytest.mark.filterwarnings("ignore:invalid value encountered in cast")      # numpy, widening the signalling NaN of PAYLOAD_NAN

SPE = 7
COMPARE_DERIVED = ("rmse", "mean_abs", "rel_l2", "rel_mse")
STATS_KEYS = ("n", "n_nan", "n_negative", "n_zero", "n_below", "n_above", "min", "max", "min_positive", "sum", "hist", "edges")
TMS = [{"op": "linear"}, {"op": "gamma", "gamma": 2.2}, {"op": "sRGB"}, {"op": "dB", "db_range": (-60.0, 0.0)}]
PAYLOAD_NAN = np.array([0x7fc12345, 0xffc00001, 0x7f800001], np.uint32).view(F32)      # quiet with a payload, its negative, a signalling one


@pytest.fixture(scope="module")
def scenes(built, tmp_path_factory):
    d = tmp_path_factory.mktemp("film_developed")
    return {P: stats_scene(d, P) for P in PLANES}


def developed(sc, films, spe=SPE):
    """wtgpu_develop's output of the accumulators: [H, W, P] f32"""
    from wave_tracer_amd.render import develop
    out = develop(sc, *films, spe)
    assert out.dtype == F32 and out.flags.c_contiguous
    return out


def same_dict(a, b, keys, label):
    for k in keys:
        assert same_bits(a[k], b[k]), (label, k, a[k], b[k])


# ---- 1. the same result from either source ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", sorted(PLANES))
def test_statistics_from_either_source(scenes, P):
    sc = scenes[P]
    _, _, channels, stokes = PLANES[P]
    films = films_of(P, 900 + P)
    film = developed(sc, films)
    assert np.isnan(film).any() and np.isinf(film).any() and (film == 0).any() and (film < 0).any()
    mask = checker(H, W)
    for bins in (0, 7, 4096):
        for s, abs_, lum, masked in option_cases(channels, stokes):
            kw = dict(stokes_component=s, scale="dB", range=(-50.0, 10.0), bins=bins, abs=abs_, luminance=lum, mask=mask if masked else None)
            want = sc.film_stats_host(*films, SPE, threads=3, **kw)
            for threads in (1, 5):
                same_dict(sc.film_stats_developed_host(film, threads=threads, **kw), want, STATS_KEYS, (P, bins, s, abs_, lum, masked, threads))
    # the two-pass form (range=None) takes the same range from either
    films = test_film_stats.stats_films(H, W, channels, stokes, 905 + P, EDGES, infinities=False)
    a, b = sc.film_stats_developed_host(developed(sc, films), scale="linear"), sc.film_stats_host(*films, SPE, scale="linear")
    assert a["range"] == b["range"]
    same_dict(a, b, STATS_KEYS, (P, "range=None"))


@pytest.mark.parametrize("P", sorted(PLANES))
def test_comparison_from_every_combination_of_sources(scenes, P):
    sc = scenes[P]
    _, _, channels, stokes = PLANES[P]
    fa, fb = films_of(P, 910 + P), films_of(P, 920 + P)
    da, db = developed(sc, fa, 5), developed(sc, fb, SPE)
    mask = checker(H, W)
    for s, abs_, lum, masked in option_cases(channels, stokes):
        kw = dict(stokes_component=s, abs=abs_, luminance=lum, mask=mask if masked else None, eps=3e-9, diff=True)
        want = sc.film_compare_host(fa, 5, fb, SPE, threads=3, **kw)
        assert want["n_nonfinite"].all() and want["n_differ"].all()
        for label, a, spe_a, b, spe_b in (("dev/acc", da, None, fb, SPE), ("acc/dev", fa, 5, db, None), ("dev/dev", da, None, db, 123)):
            for threads in (1, 5):
                got = sc.film_compare_host(a, spe_a, b, spe_b, threads=threads, **kw)
                same_dict(got, want, COMPARE_FIELDS + COMPARE_DERIVED + ("diff",), (P, label, s, abs_, lum, masked, threads))
    # the same memory twice
    got = sc.film_compare_host(da, None, da, None)
    assert not got["n_differ"].any() and not got["n_nonfinite_mismatch"].any() and not got["sum_sq"].any()


@pytest.mark.parametrize("P", sorted(PLANES))
def test_tonemap_from_either_source(scenes, P):
    sc = scenes[P]
    _, _, channels, stokes = PLANES[P]
    films = test_tonemap.make_films(H, W, channels, stokes, 31, "edges")
    film = developed(sc, films)
    mask = checker(H, W)
    k = 0
    for tm in TMS:
        for mode in ("select", "normal", "colourmap"):
            for s in range(stokes):
                for fmt in ("f32", "u8", "u16"):
                    k += 1
                    t = dict(tm, mode=mode, table=random_table(5) if k % 2 else grey_table())
                    m = mask if k % 3 == 0 else None
                    want = sc.tonemap_host(*films, SPE, t, s, mask=m, fmt=fmt, threads=3)
                    for threads in (1, 5):
                        got = sc.tonemap_developed_host(film, t, s, mask=m, fmt=fmt, threads=threads)
                        assert got.dtype == want.dtype and same_bits(got, want), (P, tm, mode, s, fmt, m is not None, threads)


@pytest.mark.parametrize("P", sorted(POLAR))
def test_polarisation_view_from_either_source(scenes, P):
    sc = scenes[P]
    channels = POLAR[P]
    films = polar_films(H, W, channels, 940 + P)
    film = developed(sc, films)
    mask = checker(H, W)
    k = 0
    for lum in ((False, True) if channels == 3 else (False,)):
        for masked in (False, True):
            for tm in TMS:
                for fmt in ("f32", "u8", "u16"):
                    k += 1
                    kw = dict(luminance=lum, maps=MAPS, analyser=THETA, mask=mask if masked else None, picture=True, picture_plane=k % (channels + lum), tm=tm, fmt=fmt,
                              sat_gain=(1.0, 2.5)[k % 2])
                    want = sc.film_polar_host(*films, SPE, threads=3, **kw)
                    for threads in (1, 5):
                        got = sc.film_polar_developed_host(film, threads=threads, **kw)
                        label = (P, lum, masked, tm, fmt, threads)
                        same_dict(got, want, POLAR_FIELDS + POLAR_DERIVED + ("picture",), label)
                        same_dict(got["maps"], want["maps"], MAPS, label)


# ---- 2. a developed film that develop did not write -------------------------------------------------------------------------------------------
def drawn_film(channels, stokes, seed, polar=False, height=H, width=W):
    """[height, width, P] f32 drawn here: log-uniform values of both signs (Stokes vectors for `polar`), and in the first odd pixels of every plane the NaNs
    of PAYLOAD_NAN, -0, +0, the smallest subnormal, the largest, both infinities and a negative value."""
    rng = np.random.default_rng(seed)
    n, P = height * width, channels * stokes
    if polar:
        i = 10.0 ** rng.uniform(-3.0, 1.0, (n, channels, 1))
        x = np.concatenate((i, i * rng.uniform(-0.7, 0.7, (n, channels, 3))), axis=2).reshape(n, P).astype(F32)
    else:
        x = (10.0 ** rng.uniform(-7.0, 2.0, (n, P))).astype(F32)
        x[rng.random((n, P)) < 0.2] *= F32(-1)
    special = list(PAYLOAD_NAN) + [F32(-0.0), F32(0.0), F32(1e-45), np.array([0x007fffff], np.uint32).view(F32)[0], F32(np.inf), F32(-np.inf), F32(-1.0)]
    for k, e in enumerate(special):
        x[2 * k + 1] = e
        if polar:     # the special value in ONE component of an otherwise lit vector, the components in turn
            x[2 * k + 1] = np.tile(np.where(np.arange(4) == k % 4, e, F32(0.25)), channels)
    return np.ascontiguousarray(x.reshape(height, width, P))


@pytest.fixture
def the_film_itself(monkeypatch):
    """The restatements develop their films with restate_develop: here what they are given as `value` IS the developed film."""
    for module in (test_film_stats, test_film_polar, test_tonemap):
        monkeypatch.setattr(module, "restate_develop", lambda value, weight, light, spe: value)


@pytest.mark.parametrize("P", sorted(PLANES))
def test_statistics_of_a_drawn_film(scenes, the_film_itself, P):
    sc = scenes[P]
    _, _, channels, stokes = PLANES[P]
    film = drawn_film(channels, stokes, 50 + P)
    bits = film.copy()
    mask = checker(H, W)
    for scale, (lo, hi) in test_film_stats.RANGES.items():
        for bins in (0, 7, 4096):
            edges = restate_edges(scale, lo, hi, bins)
            for s, abs_, lum, masked in option_cases(channels, stokes):
                m = mask if masked else None
                got = sc.film_stats_developed_host(film, stokes_component=s, scale=scale, range=(lo, hi), bins=bins, abs=abs_, luminance=lum, mask=m, threads=3)
                want = restate_stats(test_film_stats.elements(channels, stokes, (film, None, None), None, s, abs_, lum), edges, m)
                check_stats(got, want, (P, scale, bins, s, abs_, lum, masked))
                if not masked and not lum:
                    assert (got["n_nan"] == len(PAYLOAD_NAN)).all() and (got["n_zero"] >= 2).all() and same_bits(got["max"], np.full(channels, np.inf, F32))
                    assert same_bits(got["min_positive"], np.full(channels, 1e-45, F32))      # the subnormal is an element like any other
                    assert abs_ or same_bits(got["min"], np.full(channels, -np.inf, F32))
    assert same_bits(film, bits)


@pytest.mark.parametrize("P", sorted(PLANES))
def test_comparison_of_drawn_films(scenes, the_film_itself, P):
    sc = scenes[P]
    _, _, channels, stokes = PLANES[P]
    a, b = drawn_film(channels, stokes, 60 + P), drawn_film(channels, stokes, 70 + P)
    b.reshape(H * W, -1)[1] = F32(1.0)          # a payload NaN against a number; pixels 3 and 5 hold NaN against NaN
    b.reshape(H * W, -1)[7] = F32(0.0)          # -0 against +0: they do not differ
    mask = checker(H, W)
    for s, abs_, lum, masked in option_cases(channels, stokes):
        m = mask if masked else None
        got = sc.film_compare_host(a, None, b, None, stokes_component=s, abs=abs_, luminance=lum, mask=m, eps=1e-4, diff=True, threads=3)
        xa, xb = (test_film_stats.elements(channels, stokes, (f, None, None), None, s, abs_, lum) for f in (a, b))
        check_compare(got, restate_compare(xa, xb, m, 1e-4), (P, s, abs_, lum, masked))
        d = got["diff"].reshape(H * W, -1)
        if not masked:
            assert (got["n_nonfinite"][:channels] >= 5).all() and (got["n_nonfinite_mismatch"][:channels] >= 1).all()
            assert same_bits(d[[1, 3, 5], :channels], np.full((3, channels), QUIET_NAN, F32))     # the canonical quiet NaN, whatever the payloads were


@pytest.mark.parametrize("P", sorted(POLAR))
def test_polarisation_view_of_a_drawn_film(scenes, the_film_itself, P):
    import math
    sc = scenes[P]
    channels = POLAR[P]
    film = drawn_film(channels, 4, 80 + P, polar=True)
    x = test_film_polar.stokes_of((film, None, None), channels)
    c2, s2 = math.cos(2 * THETA), math.sin(2 * THETA)
    mask = checker(H, W)
    for lum in ((False, True) if channels == 3 else (False,)):
        for m in (None, mask):
            want = restate_polar(x, lum, m, c2, s2)
            got = sc.film_polar_developed_host(film, luminance=lum, maps=MAPS, analyser=THETA, mask=m, threads=3)
            worst = check_polar(got, want, (P, lum, m is not None), (H, W, channels + lum))
            assert worst <= test_film_polar.BOUND, worst
            if m is None:
                assert all(k >= 5 for k in want["n_nonfinite"]) and all(want["n_dark"]) and (got["argmax"] < H * W).all()
    # the linear picture against the restatement, every format
    want = restate_polar(x, False, None, c2, s2)
    aolp = sc.film_polar_developed_host(film, maps=("aolp",))["maps"]["aolp"].reshape(H * W, -1)
    for plane in range(channels):
        rgb = test_film_polar.restate_picture(want, aolp, plane, {"op": "linear"}, 2.5)
        for fmt in ("f32", "u8", "u16"):
            got = sc.film_polar_developed_host(film, picture=True, picture_plane=plane, fmt=fmt, sat_gain=2.5)["picture"]
            assert same_bits(got.reshape(H * W, 3), test_film_polar.codes(rgb, fmt)), (P, plane, fmt)


@pytest.mark.parametrize("P", sorted(PLANES))
def test_linear_picture_of_a_drawn_film(scenes, the_film_itself, P):
    sc = scenes[P]
    _, _, channels, stokes = PLANES[P]
    film = drawn_film(channels, stokes, 90 + P)
    mask = checker(H, W)
    for mode in ("select", "normal", "colourmap"):
        for table in (grey_table(), random_table(5)):
            tm = {"op": "linear", "mode": mode, "table": table}
            for s in range(stokes):
                want = test_tonemap.restate(channels, stokes, film, np.ones((H, W)), None, None, tm, s, T=F32)
                got = sc.tonemap_developed_host(film, tm, s, threads=3)
                # (a NaN goes through the linear operator with whatever payload it has: the pictures agree on where the NaNs are and on every other bit)
                assert np.array_equal(np.isnan(got), np.isnan(want)) and same_bits(np.where(np.isnan(got), F32(0), got), np.where(np.isnan(want), F32(0), want)), (P, mode, s)
                for fmt in ("u8", "u16"):
                    q = sc.tonemap_developed_host(film, tm, s, mask=mask, fmt=fmt)
                    assert np.array_equal(q[..., :3].astype(np.int64), quantise(want, fmt)) and np.array_equal(q[..., 3].astype(np.int64), quantise(mask, fmt)), (P, mode, s, fmt)


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_refused_sources_say_why(scenes):
    from wave_tracer_amd.api import FilmCompare, FilmCompareSpec, FilmPolar, FilmPolarSpec, FilmSource, FilmStats, FilmStatsSpec, load_library
    lib = load_library()
    sc = scenes[12]
    v, w, l = (np.ascontiguousarray(t) for t in polar_films(H, W, 3, 1))
    film = developed(sc, (v, w, l))
    acc = FilmSource(v.ctypes.data, w.ctypes.data, l.ctypes.data, SPE, None)
    dev = FilmSource(None, None, None, 0, film.ctypes.data)
    both = FilmSource(v.ctypes.data, w.ctypes.data, l.ctypes.data, SPE, film.ctypes.data)
    neither = FilmSource(None, None, None, SPE, None)
    partial = FilmSource(v.ctypes.data, None, l.ctypes.data, SPE, None)
    dev_and_one = FilmSource(None, w.ctypes.data, None, SPE, film.ctypes.data)
    out = np.zeros((H, W, 3), F32)
    srec, crec, prec = (FilmStats * 4)(), (FilmCompare * 4)(), (FilmPolar * 4)()
    sspec, cspec, pspec = FilmStatsSpec(0, 1, 0, 0, -50.0, 10.0), FilmCompareSpec(0, 0, 1e-4), FilmPolarSpec()
    calls = {
        "tonemap": lambda s: lib.wtgpu_tonemap_source_host(sc.handle, C.byref(s), None, 0, None, 0, 1, out.ctypes.data),
        "film_stats": lambda s: lib.wtgpu_film_stats_source_host(sc.handle, C.byref(s), C.byref(sspec), None, 1, C.cast(srec, C.c_void_p), None),
        "film_polar": lambda s: lib.wtgpu_film_polar_source_host(sc.handle, C.byref(s), C.byref(pspec), None, 1, C.cast(prec, C.c_void_p), None, None),
        "film_compare: A": lambda s: lib.wtgpu_film_compare_source_host(sc.handle, C.byref(s), C.byref(acc), C.byref(cspec), None, 1, C.cast(crec, C.c_void_p), None),
        "film_compare: B": lambda s: lib.wtgpu_film_compare_source_host(sc.handle, C.byref(dev), C.byref(s), C.byref(cspec), None, 1, C.cast(crec, C.c_void_p), None),
    }
    for what, call in calls.items():
        for source, message in ((both, "both forms are set"), (dev_and_one, "both forms are set"), (neither, "neither form is set"), (partial, "2 of the 3 set")):
            assert call(source) == 1, (what, message)
            err = lib.wtgpu_last_error().decode()
            assert err.startswith(what + ": ") and "film source" in err and message in err, (what, message, err)
        assert call(acc) == 0 and call(dev) == 0, (what, lib.wtgpu_last_error())
    # a null source, and what the siblings refuse, in the siblings' words
    assert lib.wtgpu_film_stats_source_host(sc.handle, None, C.byref(sspec), None, 1, C.cast(srec, C.c_void_p), None) == 1 and b"null argument" in lib.wtgpu_last_error()
    assert lib.wtgpu_film_compare_source_host(sc.handle, C.byref(dev), None, C.byref(cspec), None, 1, C.cast(crec, C.c_void_p), None) == 1 and b"null argument" in lib.wtgpu_last_error()


def test_developed_calls_refuse_what_their_siblings_refuse(scenes):
    from wave_tracer_amd import WtgpuError
    mono, rgb, pol = scenes[1], scenes[3], scenes[12]
    fm, fr, fp = (np.zeros((H, W, P), F32) for P in (1, 3, 12))
    with pytest.raises(WtgpuError, match=r"stokes_component 1 out of range \(the film has 1\)"):
        mono.film_stats_developed_host(fm, stokes_component=1, range=(-50, 10))
    with pytest.raises(WtgpuError, match="bins 4097 above the 4096"):
        rgb.film_stats_developed_host(fr, range=(-50, 10), bins=4097)
    with pytest.raises(WtgpuError, match=r"LUMINANCE needs a 3-channel film \(this one has 1\)"):
        mono.film_stats_developed_host(fm, range=(-50, 10), luminance=True)
    with pytest.raises(WtgpuError, match="film_compare: a finite eps > 0 expected"):
        rgb.film_compare_host(fr, None, fr, None, eps=0.0)
    with pytest.raises(WtgpuError, match=r"film_compare: stokes_component 4 out of range"):
        pol.film_compare_host(fp, None, fp, None, stokes_component=4)
    with pytest.raises(WtgpuError, match="film_polar: a polarimetric film expected"):
        rgb.film_polar_developed_host(fr)
    with pytest.raises(WtgpuError, match=r"film_polar: picture_plane 3 out of range \(the call has 3\)"):
        pol.film_polar_developed_host(fp, picture=True, picture_plane=3)
    with pytest.raises(WtgpuError, match="'function' operator is not supported"):
        rgb.tonemap_developed_host(fr, {"op": "function"})
    with pytest.raises(WtgpuError, match="expected valid 'db' range"):
        rgb.tonemap_developed_host(fr, {"op": "dB", "db_range": (0.0, 0.0)})
    with pytest.raises(WtgpuError, match=r"tonemap: stokes_component 4 out of range"):
        pol.tonemap_developed_host(fp, {"op": "linear"}, 4)
    # the film itself, in Python: dtype, size, layout
    for call in (lambda f: rgb.tonemap_developed_host(f), lambda f: rgb.film_stats_developed_host(f, range=(-50, 10)), lambda f: rgb.film_compare_host(f, None, fr, None),
                 lambda f: rgb.film_compare_host(fr, None, f, None), lambda f: rgb.film_polar_developed_host(f)):
        for bad in (fr.astype(np.float64), fm, np.zeros((H, W, 6), F32)[..., ::2]):
            with pytest.raises(ValueError, match=r"film: a contiguous float32 array \[23, 37, 3, 1\] \(2553 elements\) expected"):
                call(bad)
    with pytest.raises(ValueError, match="mask of the scene's size"):
        rgb.film_stats_developed_host(fr, range=(-50, 10), mask=np.zeros(5, F32))


# ---- 4. the Python forms ----------------------------------------------------------------------------------------------------------------------
def test_view_takes_the_range_auto_db_range_gives(scenes):
    from wave_tracer_amd.render import auto_db_range, view
    for P in (1, 3, 12):
        sc = scenes[P]
        films = test_film_stats.stats_films(H, W, sc.spectral_channels, sc.stokes, 500 + P, EDGES, infinities=False)
        film = developed(sc, films)
        mask = checker(H, W)
        for m in (None, mask):
            rng_dev, rng_acc = auto_db_range(sc, film, None, mask=m), auto_db_range(sc, films, SPE, mask=m)
            assert rng_dev == rng_acc and rng_dev[0] < rng_dev[1]
            got = view(sc, film, {"op": "dB", "mode": "normal"}, mask=m)
            want = sc.tonemap_developed_host(film, {"op": "dB", "mode": "normal", "db_range": rng_dev}, mask=m, fmt="u8")
            assert got.dtype == np.uint8 and got.shape == (H, W, 4 if m is not None else 3) and same_bits(got, want) and got[..., :3].any()
        # a range that is given is kept; another format, component and operator go through
        assert same_bits(view(sc, film, {"op": "dB", "mode": "normal", "db_range": (-20.0, 5.0)}, fmt="u16"),
                         sc.tonemap_developed_host(film, {"op": "dB", "mode": "normal", "db_range": (-20.0, 5.0)}, fmt="u16"))
        assert same_bits(view(sc, film, {"op": "linear", "mode": "normal"}, fmt="f32", stokes_component=sc.stokes - 1),
                         sc.tonemap_host(*films, SPE, {"op": "linear", "mode": "normal"}, sc.stokes - 1))


def test_denoise_view_and_quality_on_numpy_films(scenes):
    from wave_tracer_amd.render import denoise, quality, view
    sc = scenes[12]
    finite = lambda films: (np.where(np.isfinite(films[0]), films[0], 0.5),) + films[1:]      # (a dB range is taken from the denoised film below)
    fa, fb, ref = (finite(polar_films(H, W, 3, seed)) for seed in (21, 22, 23))
    kw = dict(window=2, patch=1)
    plain = denoise(sc, fa, fb, SPE, **kw)
    assert sorted(plain) == ["film", "residual", "residual_rel"]            # the default: the dict as it was
    for v, picture_kw in ((True, {}), ({"tm": {"op": "dB", "mode": "normal"}, "fmt": "u16", "stokes_component": 1}, None)):
        out = denoise(sc, fa, fb, SPE, view=v, **kw)
        assert sorted(out) == ["film", "picture", "residual", "residual_rel"] and same_bits(out["film"], plain["film"])
        assert same_bits(out["picture"], view(sc, plain["film"], **(v if picture_kw is None else picture_kw))) and out["picture"].shape == (H, W, 3)
    q = quality(sc, plain["film"], ref, 9, luminance=True, mask=checker(H, W))
    want = sc.film_compare_host(plain["film"], None, ref, 9, luminance=True, mask=checker(H, W))
    same_dict(q, want, COMPARE_FIELDS + COMPARE_DERIVED, "quality")
    with np.errstate(all="ignore"):
        assert same_bits(q["rel_l2"], np.sqrt(q["sum_sq"] / q["sum_b_sq"])) and (q["rel_l2"] > 0).all() and q["rel_l2"].shape == (4,)
